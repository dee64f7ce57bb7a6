"""hy_table_scan's ColumnVsValue scans at the limits of every column type: the device against the CPU oracle's bytes (assert_scan_equal) AND
against the plain truth of tests/scan_edge_truth.py (the PosList, as bytes), for every (condition, literal) of scan_edge_truth.predicates --
every limit value under the six comparisons, about thirty BETWEEN pairs in the four forms, IS [NOT] NULL, NaN literals on the float types --
over every layout the scan reads in place.  No tolerance anywhere, no case skipped at run time: FrameOfReference exists for int32 only and
NaN rows only where a layout can hold them (unencoded, RunLength), and the parametrisation leaves the rest out.

Which kernel copy a case reaches.  The library reports no path of a one-column scan (hy_debug_scan_trace only stamps times), and no option
switches between its instantiations, so the cases reach them by construction, by the rule of hy_column_create: a data column whose chunks are all
aligned W-byte vectors of one W (unencoded int32: 4; Dictionary / FrameOfReference: their element width; BitPackingVectors of at most 16 bits:
the class 16) takes the streaming scan_slices<W>; every other column -- mixed widths, int64 / float / double values, RunLength, wider
BitPackingVectors, reference columns -- takes a generic instantiation (scan_slices<0> / <8>).  Every streaming case has a twin with one chunk of
another width, which sends the same rows through the generic copy; the widths are asserted.  A sorted chunk's JOB_RANGE is not reported
either: the flagged and the not-flagged column must give the same bytes, which the oracle (it ignores the flag) and the truth pin."""
import numpy as np
import pytest

import scan_edge_truth as T
from golden import known_answers as KA
from hyrise_amd import abi, storage
from hyrise_amd.operators import scan_project_aggregate, table_scan, table_scan_expression
from hyrise_amd.storage import DeviceColumn
from support import assert_scan_equal, oracle_scan
from test_device_memory_columns_gpu import widen
from test_scan_edges_oracle import CONDITION_OF, all_rows, column_of, predicate_of
from test_scan_gpu import SORT_OF

pytestmark = pytest.mark.gpu

NAMES = list(T.TYPES)
FLOATS = [n for n in NAMES if T.is_float(n)]
BOTH_FLAGS = (0, abi.SCAN_MATERIALIZE_ALL_MATCH)
TYPE_OF = {name: storage.TYPE_OF_NP[np.dtype(t)] for name, t in T.TYPES.items()}


def scan_all(name, host, chunks, nullable, context, dev=None, flags=(0,), ordered=True, with_nan=None):
    """Every predicate of the type over one column: device == oracle (bytes, counts, states, offsets) and device == truth (PosList, counts).
    ordered = False (PosLists over several chunks: matches come out by referenced chunk): the device's RowIDs are sorted before they meet the truth's."""
    dev = dev or DeviceColumn(host)
    with_nan = T.is_float(name) if with_nan is None else with_nan
    for condition, literal, literal2 in T.predicates(name, with_nan=with_nan):
        predicate = predicate_of(name, condition, literal, literal2, nullable)
        pairs, counts = T.truth(chunks, condition, literal, literal2)
        for f in flags:
            where = f"{context} {condition} {literal!r} {literal2!r} flags {f}"
            got = table_scan(dev, predicate, flags=f)
            assert_scan_equal(got, oracle_scan(host, predicate, flags=f), where)
            rows = all_rows(got)
            if not ordered:
                rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
            assert [int(c) for c in got.counts[:len(counts)]] == counts, f"counts against the truth: {where}"
            assert rows.tobytes() == pairs.tobytes(), f"PosList against the truth: {where}"
    return dev


def one_width(host):
    return len({(s.width, s.bits > 16) for s in host.segments}) == 1


# ---- Unencoded ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nullable", [True, False], ids=["nullable", "not_null"])
def test_unencoded(device, name, nullable):
    """ValueSegments.  int32: the streaming scan_slices<4>, and -- the odd tail as a Dictionary segment of 1-byte value ids -- the generic copy over
    the same rows; int64 / float / double columns only have the generic copy (eval8's KIND_I64 / KIND_F32 / KIND_F64 blocks)."""
    values, nulls = T.limit_column(name)
    chunks = T.split(values, nulls if nullable else None)
    host = column_of(chunks, abi.ENC_UNENCODED)
    assert one_width(host)
    scan_all(name, host, chunks, nullable, f"unencoded {name}", flags=BOTH_FLAGS)
    if name == "int32":
        mixed = storage.HostColumn(host.segments[:2] + [storage.encode_segment(*chunks[2], abi.ENC_DICTIONARY)], host.data_type)
        assert mixed.segments[2].width == 1 and not one_width(mixed)
        scan_all(name, mixed, chunks, nullable, "unencoded int32, generic instantiation", flags=BOTH_FLAGS)


@pytest.mark.parametrize("name", FLOATS)
def test_unencoded_nan_rows(device, name):
    values, nulls = T.limit_column(name, nan=True)
    chunks = T.split(values, nulls)
    scan_all(name, column_of(chunks, abi.ENC_UNENCODED), chunks, True, f"unencoded {name} with NaN rows", flags=BOTH_FLAGS)


# ---- Dictionary ---------------------------------------------------------------------------------------------------------------------------
def dictionary_columns(name, width, nullable):
    """-> (chunks, the column with `width`-byte value ids in every chunk, its twin with another width in the odd tail)."""
    values, nulls = T.limit_column(name, pool=150 if width == 1 else 3_000)
    chunks = T.split(values, nulls if nullable else None)
    own = column_of(chunks, abi.ENC_DICTIONARY)
    assert [s.width for s in own.segments] == ([1, 1, 1] if width == 1 else [2, 2, 1])
    same = storage.HostColumn([s if s.width == width else widen(s, width) for s in own.segments], own.data_type)
    tail = own.segments[2] if width != 1 else widen(own.segments[2], 2)
    return chunks, same, storage.HostColumn(same.segments[:2] + [tail], own.data_type)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("width", [1, 2, 4])
def test_dictionary(device, name, width):
    """Value ids of 1, 2 and 4 bytes (scan_slices<1|2|4>: the packed 16-bit tests of the narrow ones), and the generic copy over the twin.  The limit
    values are in every dictionary, so lower_bound / upper_bound land on id 0, on the last id and on INVALID_VALUE_ID; a float dictionary holds one
    of -0.0 / 0.0 and is searched with both."""
    for nullable in (True, False):
        chunks, same, twin = dictionary_columns(name, width, nullable)
        assert one_width(same) and not one_width(twin) and same.segments[0].width == width
        scan_all(name, same, chunks, nullable, f"dictionary {name} width {width} nullable {nullable}", flags=BOTH_FLAGS)
        scan_all(name, twin, chunks, nullable, f"dictionary {name} width {width} nullable {nullable}, generic instantiation")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pool", [150, 3_000], ids=["8_bits", "13_bits"])
def test_bit_packed_dictionary(device, name, pool):
    """BitPackingVectors of at most 16 bits: the streaming scan_slices<16>."""
    values, nulls = T.limit_column(name, pool=pool)
    chunks = T.split(values, nulls)
    host = storage.HostColumn([storage.bit_pack_segment(s) for s in column_of(chunks, abi.ENC_DICTIONARY).segments], TYPE_OF[name])
    assert all(s.width == 0 and s.bits <= 16 for s in host.segments) and max(s.bits for s in host.segments) >= (8 if pool == 150 else 12)
    scan_all(name, host, chunks, True, f"bit-packed dictionary {name} pool {pool}")


# ---- FrameOfReference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packing", ["fixed_width", "bit_packed"])
@pytest.mark.parametrize("nullable", [True, False], ids=["nullable", "not_null"])
def test_frame_of_reference(device, packing, nullable):
    """Blocks whose minimum is INT32_MIN with offsets up to 2^32 - 1, blocks that end at INT32_MAX, blocks around zero -- next to each other in one
    chunk: the scan compares offsets against `lo - block minimum` modulo 2^32.  Fixed width: 4-byte offsets in every chunk (scan_slices<4>), 2-byte
    offsets in every chunk (scan_slices<2>), and the wide chunk in front of the narrow ones (generic).  Bit-packed: 32 bits (generic) and at most
    10 bits (scan_slices<16>)."""
    columns = {}
    for narrow in (False, True):
        values, nulls = T.frame_of_reference_column(narrow)
        chunks = T.split(values, nulls if nullable else None, T.FOR_SIZES)
        columns[narrow] = (chunks, column_of(chunks, abi.ENC_FRAME_OF_REFERENCE))
    (wide_chunks, wide), (narrow_chunks, narrow) = columns[False], columns[True]
    assert [s.width for s in wide.segments] == [4, 4, 4] and [s.width for s in narrow.segments] == [2, 2, 2]
    assert int(wide.segments[0].aux[0]) == np.iinfo(np.int32).min and int(wide.segments[0].data[:2048].max()) == 2**32 - 1
    mixed_chunks = [wide_chunks[0]] + narrow_chunks[1:]
    mixed = storage.HostColumn([wide.segments[0]] + narrow.segments[1:], abi.TYPE_INT)
    cases = [("4-byte offsets", wide_chunks, wide), ("2-byte offsets", narrow_chunks, narrow), ("mixed widths, generic instantiation", mixed_chunks, mixed)]
    if packing == "bit_packed":
        cases = [(f"{what}, bit-packed", chunks, storage.HostColumn([storage.bit_pack_segment(s) for s in host.segments], abi.TYPE_INT)) for what, chunks, host in cases[:2]]
        assert cases[0][2].segments[0].bits == 32 and max(s.bits for s in cases[1][2].segments) == 10
    for what, chunks, host in cases:
        scan_all("int32", host, chunks, nullable, f"frame of reference, {what}")


# ---- RunLength ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nan", [(n, False) for n in NAMES] + [(n, True) for n in FLOATS], ids=lambda x: x if isinstance(x, str) else ("nan_runs" if x else "finite"))
def test_run_length(device, name, nan):
    """RunLength segments read in place (eval_run, eval8_run_length): NULL runs, runs of the limit values, runs of 2500 and 3000 rows (longer than the
    2048 rows a wave walks), 300 runs of one row; the float variants with NaN runs."""
    values, nulls = T.run_column(name, nan=nan)
    chunks = T.split(values, nulls)
    host = storage.HostColumn([storage.encode_run_length(v, m) for v, m in chunks], TYPE_OF[name])
    ends = np.asarray(host.segments[0].aux, dtype=np.int64)
    lengths = np.diff(np.concatenate([[-1], ends]))
    assert lengths.max() > 2_048 and (lengths == 1).sum() >= 100 and host.segments[0].nulls.any()
    scan_all(name, host, chunks, True, f"run length {name} nan {nan}")


# ---- sorted chunks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sort_mode", KA.SORTED_SEGMENT_SORT_MODES)
def test_sorted_chunks(device, name, sort_mode):
    """Chunks that hold the sorted limit values (with duplicates; one among 3000 random values): the matching block begins at row 0, ends at the last
    row, is empty, or is the whole chunk.  Flagged, prepare_jobs finds the block with 64-ary searches and the scan only stores (JOB_RANGE: no hook
    reports it); not flagged, every row is tested.  Same bytes either way, in every layout."""
    chunks = T.sorted_chunks(name, sort_mode.startswith("Ascending"), sort_mode.endswith("NullsLast"))
    kinds = ["Unencoded", "Dictionary", "RunLength", "BitPackedDictionary"] + (["FrameOfReference"] if name == "int32" else [])
    for kind in kinds:
        def encode(values, nulls):
            if kind == "RunLength":
                return storage.encode_run_length(values, nulls)
            segment = storage.encode_segment(values, nulls, {"Unencoded": abi.ENC_UNENCODED, "FrameOfReference": abi.ENC_FRAME_OF_REFERENCE}.get(kind, abi.ENC_DICTIONARY))
            return storage.bit_pack_segment(segment) if kind.startswith("BitPacked") else segment
        for flagged in (True, False):
            host = storage.HostColumn([encode(v, m) for v, m in chunks], TYPE_OF[name])
            for segment in host.segments:
                segment.sorted_by = SORT_OF[sort_mode] if flagged else 0
            scan_all(name, host, chunks, True, f"sorted {sort_mode} {kind} {name} flagged {flagged}")


# ---- reference columns --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("base_layout", ["Unencoded", "Dictionary"])
def test_reference_columns(device, name, base_layout):
    """The limit column behind PosLists: an EntireChunkPosList per chunk, PosLists over one chunk (ascending, and shuffled), and a shuffled PosList over all
    chunks with NULL_ROW_IDs (matches come out by referenced chunk: compared with the oracle in that order, with the truth as a set)."""
    rng = np.random.default_rng(55)
    values, nulls = T.limit_column(name, pool=3_000 if base_layout == "Dictionary" else None)
    base_chunks = T.split(values, nulls)
    base = column_of(base_chunks, abi.ENC_DICTIONARY if base_layout == "Dictionary" else abi.ENC_UNENCODED)
    base_dev = DeviceColumn(base)

    def rows_of(chunk, offsets):
        return np.stack([np.full(len(offsets), chunk, dtype=np.uint32), np.asarray(offsets, dtype=np.uint32)], axis=1)

    def behind(pos):
        """(values, nulls) a PosList stands for; a NULL_ROW_ID is a NULL."""
        missing = pos[:, 1] == 0xFFFFFFFF
        out_values, out_nulls = np.zeros(len(pos), dtype=values.dtype), missing.copy()
        for c, (chunk_values, chunk_nulls) in enumerate(base_chunks):
            here = ~missing & (pos[:, 0] == c)
            out_values[here], out_nulls[here] = chunk_values[pos[here, 1]], chunk_nulls[pos[here, 1]]
        return out_values, out_nulls

    ascending = rows_of(0, np.sort(rng.choice(T.SIZES[0], 3_000, replace=False)))
    shuffled = rows_of(1, rng.permutation(T.SIZES[1])[:700])
    drawn = rng.integers(0, T.N, 4_000)
    starts = np.concatenate([[0], np.cumsum(T.SIZES)])
    chunk_of = np.searchsorted(starts, drawn, side="right") - 1
    everywhere = np.stack([chunk_of, drawn - starts[chunk_of]], axis=1).astype(np.uint32)
    everywhere[rng.random(len(everywhere)) < 0.03] = 0xFFFFFFFF
    for what, pos_lists, single, ordered in (("entire chunks and single-chunk PosLists", [0, 1, 2, ascending, shuffled], [0, 1, 2, 0, 1], True),
                                            ("a PosList over all chunks", [everywhere, ascending], [None, 0], False)):
        host = storage.make_reference_column(base, pos_lists, single)
        chunks = [base_chunks[p] if isinstance(p, int) else behind(p) for p in pos_lists]
        dev = DeviceColumn(host, refs={id(base): base_dev})
        scan_all(name, host, chunks, True, f"reference over {base_layout} {name}: {what}", dev=dev, ordered=ordered)


# ---- the other consumers of the scan's jobs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scan_project_aggregate_counts(device, name):
    """hy_scan_project_aggregate reads the job table of prepare_scan_jobs: COUNT(*) WHERE x <= MAX / x > MIN / x BETWEEN MIN AND MAX (floats: the infinities)."""
    values, nulls = T.limit_column(name)
    chunks = T.split(values, nulls)
    dev = DeviceColumn(column_of(chunks, abi.ENC_UNENCODED))
    low, high = T.limits(name)[0], T.limits(name)[-1]
    for condition, literal, literal2 in (("<=", high, None), (">", low, None), ("between_inclusive", low, high)):
        want = sum(T.truth(chunks, condition, literal, literal2)[1])
        got = scan_project_aggregate([(dev, predicate_of(name, condition, literal, literal2, True))], [], [(abi.AGG_COUNT, None)])
        assert 0 < want < T.N and got.n_groups == 1 and got.column(0) == [want], f"{name} COUNT(*) WHERE x {condition} {literal!r} {literal2!r}"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("layout", ["Unencoded", "Dictionary"])
def test_expression_scan(device, name, layout):
    """hy_table_scan_expression: `column <comparison> literal` as a one-comparison program (compare_typed's comparison, not the job table's), every limit
    value -- both ends of the type among them -- as the literal."""
    values, nulls = T.limit_column(name, pool=3_000 if layout == "Dictionary" else None)
    chunks = T.split(values, nulls)
    dev = DeviceColumn(column_of(chunks, abi.ENC_DICTIONARY if layout == "Dictionary" else abi.ENC_UNENCODED))
    for condition in T.COMPARISONS:
        for literal in T.single_literals(name):
            pairs, counts = T.truth(chunks, condition, literal)
            got = table_scan_expression(("cmp", CONDITION_OF[condition], dev, (TYPE_OF[name], literal)))
            assert [int(c) for c in got.counts[:len(counts)]] == counts and got.matches[:got.total].tobytes() == pairs.tobytes(), f"{name} {layout} x {condition} {literal!r}"
