"""The LIKE family with the dictionaries matched on the device: hy_like_matches (csrc/like.hip) against the project's host matcher
(hyrise_amd.like.dictionary_matches, which tests/test_host_like_matcher.py and tests/test_oracle_like.py pin to the reference's expected
tables), and hy_table_scan_like against hy_table_scan fed with the host matcher's bitmaps and against the CPU oracle fed with the same."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.like import dictionary_matches
from hyrise_amd.operators import like_match_words, like_matches, make_predicate, table_scan, table_scan_like
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary
from like_cases import SPECIAL_CHARS_CASES, STRING_TABLE_CASES, StringTable, expected_rows
from placed_columns import PlacedArray
from support import assert_scan_equal, build_column, oracle_scan, result_rows
from test_like_gpu import WORDS, random_string_column

pytestmark = pytest.mark.gpu

LIKE_CONDITIONS = (abi.PRED_LIKE, abi.PRED_NOT_LIKE, abi.PRED_LIKE_INSENSITIVE, abi.PRED_NOT_LIKE_INSENSITIVE)
ENTRY_COUNTS = (0, 1, 63, 64, 65, 257)


def assert_matches_equal(got, want, context):
    assert len(got) == len(want), context
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{context}: chunk {c} differs at entries {np.flatnonzero(g != w)[:8].tolist()}"


# ---- the reference's cases through table_scan_like -------------------------------------------------------------------------------------------
def check_like_scan(table, dev, dev_dict, condition, pattern, expected, line):
    predicate = table.predicate(condition, pattern)
    got = table_scan_like(dev, dev_dict, pattern, condition, nullable=table.tbl.nullable[table.string_column])
    assert_scan_equal(got, table_scan(dev, predicate), f"table_scan_string_test.cpp:{line} against host bitmaps")
    assert_scan_equal(got, oracle_scan(table.column, predicate), f"table_scan_string_test.cpp:{line} against the oracle")
    assert table.rows_of(result_rows(got)) == expected_rows(expected), f"table_scan_string_test.cpp:{line}"


@pytest.mark.parametrize("line,condition,pattern,expected", STRING_TABLE_CASES)
def test_like_on_dictionary_segments(device, line, condition, pattern, expected):
    table = StringTable("int_string_like.tbl", 5)
    check_like_scan(table, DeviceColumn(table.column), DeviceStringDictionary(table.dictionaries), condition, pattern, expected, line)


@pytest.mark.parametrize("line,condition,pattern,expected", SPECIAL_CHARS_CASES)
def test_like_special_characters(device, line, condition, pattern, expected):
    table = StringTable("int_string_like_special_chars.tbl", 2)
    check_like_scan(table, DeviceColumn(table.column), DeviceStringDictionary(table.dictionaries), condition, pattern, expected, line)


@pytest.mark.parametrize("line,condition,pattern,expected", [c for c in STRING_TABLE_CASES if c[0] in (151, 178, 242, 265)])
def test_like_on_referenced_dictionary_segments(device, line, condition, pattern, expected):
    """The reference column's dictionary is the referenced data column's."""
    table = StringTable("int_string_like.tbl", 5)
    a = build_column(table.tbl.columns[0], None, 5, abi.ENC_UNENCODED)
    first = table_scan(DeviceColumn(a), make_predicate(abi.PRED_GREATER_THAN, abi.TYPE_INT, 0), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    pos_lists = [first.pos_list(c).copy() for c in range(a.n_chunks)]
    referencing = storage.make_reference_column(table.column, pos_lists, list(range(a.n_chunks)))
    base_dev = DeviceColumn(table.column)
    ref_dev = DeviceColumn(referencing, refs={id(table.column): base_dev})
    dev_dict = DeviceStringDictionary(table.dictionaries)
    predicate = table.predicate(condition, pattern)
    got = table_scan_like(ref_dev, dev_dict, pattern, condition, nullable=table.tbl.nullable[table.string_column])
    assert_scan_equal(got, table_scan(ref_dev, predicate), f"table_scan_string_test.cpp:{line} against host bitmaps")
    assert_scan_equal(got, oracle_scan(referencing, predicate), f"table_scan_string_test.cpp:{line} against the oracle")
    data_rows = [tuple(pos_lists[chunk][offset]) for chunk, offset in result_rows(got)]
    assert table.rows_of(data_rows) == expected_rows(expected)


# ---- the matcher against the host matcher ----------------------------------------------------------------------------------------------------
def random_dictionaries(rng, entry_counts=ENTRY_COUNTS, alphabet=b"abA", longest=12):
    return [[bytes(rng.choice(list(alphabet), rng.integers(0, longest + 1)).tolist()) for _ in range(n)] for n in entry_counts]


def random_patterns(rng, count):
    return [bytes(rng.choice(list(b"ab%_"), rng.integers(0, 9)).tolist()) for _ in range(count)]


@pytest.mark.parametrize("condition", LIKE_CONDITIONS)
def test_random_patterns_against_the_host_matcher(device, condition):
    """Backtracking (`%a%b`, `_%_`), the insensitive fold and every entry count around a word and a workgroup, bit for bit."""
    rng = np.random.default_rng(100 + condition)
    dictionaries = random_dictionaries(rng)
    dev_dict = DeviceStringDictionary(dictionaries)
    assert dev_dict.word_offsets.tolist() == [0, 0, 1, 2, 3, 5, 10]
    for pattern in random_patterns(rng, 1500):
        assert_matches_equal(like_matches(dev_dict, pattern, condition), dictionary_matches(dictionaries, pattern, condition), f"pattern {pattern!r} condition {condition}")


def test_fixed_length_layout_equals_the_offsets_layout(device):
    rng = np.random.default_rng(12)
    dictionaries = random_dictionaries(rng)
    by_offsets, fixed = DeviceStringDictionary(dictionaries), DeviceStringDictionary(dictionaries, fixed_length=12)
    assert fixed.word_offsets.tolist() == by_offsets.word_offsets.tolist()
    for i, pattern in enumerate(random_patterns(rng, 1500)):
        for condition in LIKE_CONDITIONS:
            want = like_matches(by_offsets, pattern, condition)
            assert_matches_equal(like_matches(fixed, pattern, condition), want, f"pattern {pattern!r} condition {condition}")
            assert np.array_equal(like_match_words(fixed, pattern, condition), like_match_words(by_offsets, pattern, condition))   # (tail bits too)
            if i % 50 == 0:
                assert_matches_equal(want, dictionary_matches(dictionaries, pattern, condition), f"pattern {pattern!r} condition {condition}")


BYTE_ENTRIES = [b"", b"\x00", b"\x00\x00", b"a\x00b", b"a", b"b", b"ab", b"aab", b"\n", b"a\nb", b"%", b"_", b"%_", b"a%b", b"100%", b"_x_", bytes(range(0x80, 0x100)),
                b"\xff", b"\x80a\xfe", b"\xc3\xa4", b"A\xc3\x84", b"a" * 400 + b"b", b"a" * 400, b"x" * 256, b"x" * 255, b"x" * 257]
BYTE_PATTERNS = [b"", b"%", b"_", b"%%", b"_%_", b"__", b"%a%b" * 64, b"%a%b%a%b%a%b%a%b", b"x" * 256, b"x" * 255 + b"_", b"_" * 256, b"%\x00%", b"\x00", b"a\x00b", b"a_b",
                 b"%\xff", b"\x80%", b"%\n%", b"a\nb", b"%\xc3%", b"_\xa4", b"a%", b"%b", b"%ab", b"\\%", b"100_", b"A%"]


def test_bytes_are_bytes(device):
    """The empty string, 0x00 / 0x80-0xFF / newline / `%` / `_` as data, the longest pattern, and `%a%b%a%b...` against aaaa...ab."""
    assert max(len(p) for p in BYTE_PATTERNS) == abi.MAX_LIKE_PATTERN
    dictionaries = [BYTE_ENTRIES, [], BYTE_ENTRIES[::-1]]
    dev_dict = DeviceStringDictionary(dictionaries)
    for pattern in BYTE_PATTERNS:
        for condition in LIKE_CONDITIONS:
            want = dictionary_matches(dictionaries, pattern, condition)
            assert_matches_equal(like_matches(dev_dict, pattern, condition), want, f"pattern {pattern[:24]!r} ({len(pattern)} bytes) condition {condition}")
    # 64 times `%a%b` needs 64 b's, each behind an a: the host matcher's regex takes minutes over these two entries, so they are checked
    # against what the pattern says by construction
    pairs = DeviceStringDictionary([[b"ab" * 64, b"ab" * 63 + b"a", b"ba" * 64, b"xaxb" * 64 + b"x", b"ab" * 63 + b"b"]])
    assert like_matches(pairs, b"%a%b" * 64, abi.PRED_LIKE)[0].tolist() == [True, False, False, False, False]
    assert like_matches(pairs, b"%a%b" * 63 + b"%ab%", abi.PRED_NOT_LIKE)[0].tolist() == [False, True, True, True, True]   # (63 pairs, then "ab" side by side)
    assert like_matches(pairs, b"%A%B" * 64, abi.PRED_LIKE_INSENSITIVE)[0].tolist() == [True, False, False, False, False]
    with pytest.raises(abi.HyriseAmdError) as refused:
        like_matches(dev_dict, b"x" * 257, abi.PRED_LIKE)
    assert refused.value.status == abi.ERR_UNSUPPORTED


def test_a_long_string_among_short_ones(device):
    """One 100 000-byte entry: its workgroup reads global memory in place, its neighbours stage theirs in LDS; the results do not say which."""
    rng = np.random.default_rng(3)
    long_entry = bytes(rng.choice(list(b"ab"), 100_000).tolist())[:-6] + b"needle"
    short = [b"aa%d" % i for i in range(300)] + [b"needle", b"a needle b", b"needl"]
    entries = short[:130] + [long_entry] + short[130:]          # the long one in the first workgroup of the chunk, short ones on both sides
    dictionaries = [entries, short, [long_entry], short + [long_entry]]
    dev_dict = DeviceStringDictionary(dictionaries)
    for condition, pattern in ((abi.PRED_LIKE, b"%needle"), (abi.PRED_NOT_LIKE, b"%needle%"), (abi.PRED_LIKE, b"aa1_"), (abi.PRED_LIKE_INSENSITIVE, b"%B%NEEDLE"),
                               (abi.PRED_LIKE, b"%needlf"), (abi.PRED_LIKE, long_entry[:200] + b"%"), (abi.PRED_LIKE, b"%"), (abi.PRED_LIKE, b"_")):
        assert_matches_equal(like_matches(dev_dict, pattern, condition), dictionary_matches(dictionaries, pattern, condition), f"pattern {pattern[:24]!r} condition {condition}")


def test_seventy_thousand_entries_in_one_chunk(device):
    """One chunk whose dictionary has 70 000 p_type-like entries, every one of them used: 274 matcher workgroups for the chunk, u32 attribute
    vectors in the scan (a value id past 65 535 does not fit two bytes).  The matcher against the host matcher, the scan against
    hy_table_scan with the host's bitmaps and against the oracle."""
    rng = np.random.default_rng(70_000)
    pool = [b" ".join((WORDS[rng.integers(len(WORDS))], WORDS[rng.integers(len(WORDS))], b"%06d" % i)) for i in range(70_000)]
    segments, dictionaries = [], []
    for values, null_fraction in (([pool[i] for i in rng.permutation(70_000)] + [pool[i] for i in rng.integers(0, 70_000, 3_000)], 0.0),
                                  ([pool[i] for i in rng.integers(0, 70_000, 5_000)], 0.1)):
        nulls = rng.random(len(values)) < null_fraction if null_fraction else None
        segment, dictionary = storage.encode_string_dictionary(values, nulls)
        segments.append(segment)
        dictionaries.append(dictionary)
    host = storage.HostColumn(segments, abi.TYPE_STRING)
    assert len(dictionaries[0]) == 70_000 and host.segments[0].width == 4 and host.segments[0].aux_size == 70_000
    assert int(host.segments[0].data.max()) == 69_999 and host.segments[1].width == 2
    dev, dev_dict = DeviceColumn(host), DeviceStringDictionary(dictionaries)
    assert dev_dict.word_offsets.tolist()[:2] == [0, (70_000 + 63) // 64]
    for condition, pattern in ((abi.PRED_LIKE, "%BRASS%"), (abi.PRED_NOT_LIKE, "PROMO%"), (abi.PRED_LIKE, "%06999_"), (abi.PRED_LIKE_INSENSITIVE, "%steel %"),
                               (abi.PRED_NOT_LIKE, "%"), (abi.PRED_LIKE, "%POLISHED%TIN%")):
        host_matches = dictionary_matches(dictionaries, pattern, condition)
        assert_matches_equal(like_matches(dev_dict, pattern, condition), host_matches, f"pattern {pattern} cond {condition}")
        predicate = make_predicate(condition, abi.TYPE_STRING, nullable=True, dictionary_matches=host_matches)
        for flags in (0, abi.SCAN_CHUNK_REGIONS):
            got = table_scan_like(dev, dev_dict, pattern, condition, nullable=True, flags=flags)
            assert_scan_equal(got, table_scan(dev, predicate, flags=flags), f"pattern {pattern} cond {condition} flags {flags} against host bitmaps")
            assert_scan_equal(got, oracle_scan(host, predicate, flags=flags), f"pattern {pattern} cond {condition} flags {flags} against the oracle")
    assert like_matches(dev_dict, "%069999", abi.PRED_LIKE)[0].sum() == 1   # (an entry whose value id needs the third byte is found)


SCAN_CASES = ((abi.PRED_LIKE, "%BRASS%"), (abi.PRED_NOT_LIKE, "PROMO%"), (abi.PRED_LIKE, "%0_1"), (abi.PRED_NOT_LIKE, "%"), (abi.PRED_LIKE_INSENSITIVE, "%steel %"),
              (abi.PRED_LIKE, "%POLISHED%TIN%"), (abi.PRED_LIKE, "%nothing%"))


def device_result_as_host(result, n_chunks):
    matches, offsets, counts, chunk_state = (t.cpu().numpy() for t in result)
    return matches.view(np.uint32), offsets.astype(np.uint64), counts.view(np.uint32), chunk_state


@pytest.mark.parametrize("distinct,chunk_size", [(40, 20_000), (3_000, 20_000), (70_000, 150_000)])
@pytest.mark.parametrize("null_fraction", [0.0, 0.1])
def test_scan_parity_on_random_string_columns(device, distinct, chunk_size, null_fraction):
    """hy_table_scan_like == hy_table_scan with the host matcher's bitmaps == the oracle with the same: u8 and u16 attribute vectors (the
    third shape draws 150 000 rows from 70 000 strings and ends with about 61 800 entries per chunk: u16 still; u32 is
    test_seventy_thousand_entries_in_one_chunk), a dictionary of several matcher workgroups per chunk, NULLs, both layouts of a host result, a device result, excluded chunks."""
    rng = np.random.default_rng(distinct)
    host, dictionaries = random_string_column(rng, 4 * chunk_size + 1234, chunk_size, distinct, null_fraction)
    dev, dev_dict = DeviceColumn(host), DeviceStringDictionary(dictionaries)
    nullable = null_fraction > 0
    for condition, pattern in SCAN_CASES:
        host_matches = dictionary_matches(dictionaries, pattern, condition)
        assert_matches_equal(like_matches(dev_dict, pattern, condition), host_matches, f"distinct {distinct} pattern {pattern}")
        predicate = make_predicate(condition, abi.TYPE_STRING, nullable=nullable, dictionary_matches=host_matches)
        context = f"distinct {distinct} pattern {pattern} cond {condition}"
        for flags in (0, abi.SCAN_CHUNK_REGIONS):
            got = table_scan_like(dev, dev_dict, pattern, condition, nullable=nullable, flags=flags)
            assert_scan_equal(got, table_scan(dev, predicate, flags=flags), f"{context} flags {flags} against host bitmaps")
            assert_scan_equal(got, oracle_scan(host, predicate, flags=flags), f"{context} flags {flags} against the oracle")
        want = table_scan(dev, predicate, excluded_chunks=[1, 4])
        assert_scan_equal(table_scan_like(dev, dev_dict, pattern, condition, nullable=nullable, excluded=[1, 4]), want, f"{context} excluded chunks")
        assert want.counts[1] == 0 and want.counts[4] == 0
        # a device result: chunk regions in the caller's device memory
        want = table_scan(dev, predicate)
        matches, offsets, counts, chunk_state = device_result_as_host(table_scan_like(dev, dev_dict, pattern, condition, nullable=nullable, device=True), host.n_chunks)
        assert np.array_equal(counts, want.counts[:host.n_chunks]) and np.array_equal(chunk_state, want.chunk_state[:host.n_chunks]), context
        row_base = np.concatenate([[0], np.cumsum([s.size for s in host.segments])])
        assert np.array_equal(offsets, row_base), context
        for c in range(host.n_chunks):
            if want.chunk_state[c] != abi.CHUNK_ALL_MATCH:
                assert np.array_equal(matches[int(row_base[c]):int(row_base[c]) + int(counts[c])], want.pos_list(c)), f"{context} chunk {c}"


# ---- caller-owned device dictionaries and what lies around the outputs -----------------------------------------------------------------
class PlacedDictionary:
    """An HY_MEM_DEVICE hy_string_dictionary whose chars begin `chars_residue` bytes behind a 16-byte boundary inside a larger tensor and
    whose offsets lie on 4 bytes only, with filler around both (tests/placed_columns.py PlacedArray)."""

    def __init__(self, dictionaries, chars_residue, fill):
        self.lib = abi.load_library()
        self.n_chunks, self.n_entries = len(dictionaries), [len(d) for d in dictionaries]
        self.arrays = []
        chunks = (abi.StringDictionaryChunk * max(1, self.n_chunks))()
        for c, dictionary in enumerate(dictionaries):
            chars, offsets = storage.pack_string_dictionary(dictionary)
            placed_chars = PlacedArray(len(chars), chars_residue, fill, contents=chars)
            placed_offsets = PlacedArray(offsets.nbytes, 4, fill, contents=offsets)
            self.arrays += [placed_chars, placed_offsets]
            chunks[c].n_entries, chunks[c].string_length = len(dictionary), 0
            chunks[c].chars, chunks[c].offsets = placed_chars.pointer, placed_offsets.pointer
        self.handle = C.c_void_p()
        abi.check(self.lib.hy_string_dictionary_create(chunks, self.n_chunks, abi.MEM_DEVICE, C.byref(self.handle)))
        self.word_offsets = np.zeros(self.n_chunks + 1, dtype=np.uint64)
        abi.check(self.lib.hy_string_dictionary_match_layout(self.handle, self.word_offsets.ctypes.data))

    def assert_untouched(self):
        for array in self.arrays:
            array.assert_untouched()

    def __del__(self):
        if self.handle:
            self.lib.hy_string_dictionary_destroy(self.handle)


@pytest.mark.parametrize("chars_residue", [1, 3, 8])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_caller_owned_dictionary_at_any_byte_address(device, chars_residue, fill):
    rng = np.random.default_rng(chars_residue)
    dictionaries = random_dictionaries(rng, entry_counts=(65, 0, 257, 1, 700), alphabet=b"abA\x00\xff", longest=40)
    placed = PlacedDictionary(dictionaries, chars_residue, fill)
    uploaded = DeviceStringDictionary(dictionaries)
    for pattern in random_patterns(rng, 40) + [b"", b"%", b"%\x00%", b"%\xff_"]:
        for condition in LIKE_CONDITIONS:
            want = dictionary_matches(dictionaries, pattern, condition)
            assert_matches_equal(like_matches(placed, pattern, condition), want, f"placed at {chars_residue}, pattern {pattern!r} condition {condition}")
            assert_matches_equal(like_matches(uploaded, pattern, condition), want, f"uploaded, pattern {pattern!r} condition {condition}")
    placed.assert_untouched()


def test_words_around_match_words_stay_unchanged(device):
    lib = abi.load_library()
    rng = np.random.default_rng(8)
    dictionaries = random_dictionaries(rng)
    dev_dict = DeviceStringDictionary(dictionaries)
    total = int(dev_dict.word_offsets[-1])
    for condition, pattern in ((abi.PRED_LIKE, b"%a%"), (abi.PRED_NOT_LIKE, b"%a%"), (abi.PRED_NOT_LIKE_INSENSITIVE, b"nothing")):
        want = like_matches(dev_dict, pattern, condition)
        want_words = like_match_words(dev_dict, pattern, condition)
        for c, n in enumerate(ENTRY_COUNTS):   # tail bits of a chunk's last word are zero, under NOT too
            if n % 64:
                assert int(want_words[int(dev_dict.word_offsets[c + 1]) - 1]) >> (n % 64) == 0
        host_words = np.full(total + 8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        abi.check(lib.hy_like_matches(dev_dict.handle, pattern, len(pattern), condition, abi.MEM_HOST, host_words[4:].ctypes.data))
        assert np.array_equal(host_words[4:4 + total], want_words) and (host_words[:4] == 0x5A5A5A5A5A5A5A5A).all() and (host_words[4 + total:] == 0x5A5A5A5A5A5A5A5A).all()
        for fill in (0x00, 0xFF):
            placed = PlacedArray(8 * total, 8, fill, guard=64)
            abi.check(lib.hy_like_matches(dev_dict.handle, pattern, len(pattern), condition, abi.MEM_DEVICE, placed.pointer))
            abi.check(lib.hy_synchronize())
            inside, guards_intact = placed.read(np.uint64)
            assert guards_intact and np.array_equal(inside, want_words), (condition, fill)
        assert_matches_equal(want, dictionary_matches(dictionaries, pattern, condition), f"pattern {pattern!r}")
