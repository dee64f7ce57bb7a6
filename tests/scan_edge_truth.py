"""A plain truth for `column <condition> literal [AND literal2]` (TableScan's ColumnVsValue / ColumnBetween / ColumnIsNull) at the limits of
every column type, plus the columns and the literals that tests/test_scan_edges_oracle.py (the CPU oracle against this truth) and
tests/test_scan_edges_gpu.py (the device against both) share.

The truth is a second, independent statement of the semantics: numpy comparisons, element by element, in the column's own type (np.int32 /
np.int64 / np.float32 / np.float64 compare like C++'s int32_t / int64_t / float / double).  It imports nothing from oracle/ or hyrise_amd/;
conditions are named by strings and the test files map the ABI's constants onto them.
  - a NULL row never matches a value condition; IS NULL / IS NOT NULL go by the null flag alone
  - floats follow IEEE: a NaN (row or literal) matches only <>, -0.0 == 0.0
  - BETWEEN is `lower (<|<=) x (<|<=) upper`; reversed bounds match nothing
"""
import numpy as np

COMPARISONS = ("=", "<>", "<", "<=", ">", ">=")
BETWEENS = ("between_inclusive", "between_lower_exclusive", "between_upper_exclusive", "between_exclusive")
NULL_TESTS = ("is_null", "is_not_null")
CONDITIONS = COMPARISONS + BETWEENS + NULL_TESTS

TYPES = {"int32": np.int32, "int64": np.int64, "float32": np.float32, "float64": np.float64}
SIZES = (8_203, 2_051, 5)     # an 8192-row slice plus a partial group, a FrameOfReference block plus 3 rows, an odd tail
N = sum(SIZES)


# ---- the truth ----------------------------------------------------------------------------------------------------------------------------
def row_matches(values, nulls, condition, literal=None, literal2=None):
    """bool per row of one chunk.  values: array of the column's type; nulls: bool array or None."""
    values = np.asarray(values)
    t = values.dtype.type
    valid = np.ones(len(values), dtype=bool) if nulls is None else ~np.asarray(nulls, dtype=bool)
    if condition == "is_null":
        return ~valid
    if condition == "is_not_null":
        return valid
    with np.errstate(invalid="ignore"):
        a = t(literal)
        if condition in COMPARISONS:
            hit = {"=": values == a, "<>": values != a, "<": values < a, "<=": values <= a, ">": values > a, ">=": values >= a}[condition]
        else:
            b = t(literal2)
            lower = values >= a if condition in ("between_inclusive", "between_upper_exclusive") else values > a
            upper = values <= b if condition in ("between_inclusive", "between_lower_exclusive") else values < b
            hit = lower & upper
    return hit & valid


def truth(chunks, condition, literal=None, literal2=None):
    """chunks: [(values, nulls or None)] -> (matching (chunk, offset) pairs in row order as uint32 [n, 2], matches per chunk as a list)."""
    pairs, counts = [], []
    for c, (values, nulls) in enumerate(chunks):
        offsets = np.flatnonzero(row_matches(values, nulls, condition, literal, literal2)).astype(np.uint32)
        pairs.append(np.stack([np.full(len(offsets), c, dtype=np.uint32), offsets], axis=1).reshape(-1, 2))
        counts.append(len(offsets))
    return (np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.uint32)), counts


def split(values, nulls, sizes=SIZES):
    """One column's rows as the chunks `truth` takes."""
    out, begin = [], 0
    for size in sizes:
        out.append((values[begin:begin + size], None if nulls is None else nulls[begin:begin + size]))
        begin += size
    assert begin == len(values)
    return out


# ---- limit values -------------------------------------------------------------------------------------------------------------------------
def limits(name):
    t = TYPES[name]
    if name == "int32":
        lo, hi = np.iinfo(t).min, np.iinfo(t).max
        return np.array([lo, lo + 1, -2**16 - 1, -1, 0, 1, 2**16, hi - 1, hi], dtype=t)
    if name == "int64":   # pairs that agree in the low word and differ in the high one (0 / 2^32, 1 / 2^32 + 1, -1 / 2^32 - 1), and the other way round
        lo, hi = np.iinfo(t).min, np.iinfo(t).max
        return np.array([lo, lo + 1, -2**32 - 1, -2**32, -2**31 - 1, -1, 0, 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**53 + 1, hi - 1, hi], dtype=t)
    info = np.finfo(t)
    denormal = np.nextafter(t(0), t(1))
    exact = t(2.0 ** (info.nmant + 1)) + t(1)            # 2^24 + 1 / 2^53 + 1, rounded to even: 2^24 / 2^53
    return np.array([-np.inf, -info.max, -1, -info.tiny, -denormal, -0.0, 0.0, denormal, info.tiny, 1, exact, info.max, np.inf], dtype=t)


def nan_patterns(name):
    """The default quiet NaN, one with the sign bit set, one with another payload."""
    if name == "float32":
        return np.array([0x7FC00000, 0xFFC00000, 0x7FC12345], dtype=np.uint32).view(np.float32)
    return np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000012345678], dtype=np.uint64).view(np.float64)


def is_float(name):
    return name.startswith("float")


def random_values(rng, name, n):
    """Values over the type's whole range: every integer; for floats every finite bit pattern (both signs, denormals, the huge)."""
    t = TYPES[name]
    if not is_float(name):
        return rng.integers(np.iinfo(t).min, np.iinfo(t).max, n, dtype=t, endpoint=True)
    bits = rng.integers(0, 1 << (32 if name == "float32" else 63), n, dtype=np.uint64)
    if name == "float64":
        bits |= rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    values = bits.astype(np.uint32).view(np.float32) if name == "float32" else bits.view(np.float64)
    values = values.copy()
    broken = ~np.isfinite(values)
    values[broken] = (rng.standard_normal(int(broken.sum())) * 1000).astype(t)
    return values


# ---- columns ------------------------------------------------------------------------------------------------------------------------------
def limit_column(name, pool=None, nan=False, seed=0, n=N):
    """(values, nulls): about 30 % limit values, the rest random over the type's range (or drawn from `pool` distinct random values: a dictionary
    of a chosen size), 10 % NULLs.  The non-nullable twin is the same values with nulls = None.  nan: about 5 % NaN rows, all three patterns."""
    rng = np.random.default_rng(1_000 + seed + sum(map(ord, name)))
    edge = limits(name)
    values = random_values(rng, name, n) if pool is None else random_values(rng, name, pool)[rng.integers(0, pool, n)]
    at_limit = rng.random(n) < 0.3
    values[at_limit] = edge[rng.integers(0, len(edge), int(at_limit.sum()))]
    values[:len(edge)] = edge                               # every limit value at least once in the first chunk ...
    values[n - 5:n] = edge[[0, -1, len(edge) // 2, 0, -1]]   # ... and both ends in the odd tail
    if nan:
        patterns = nan_patterns(name)
        holds_nan = np.flatnonzero(rng.random(n) < 0.05)
        values[holds_nan] = patterns[rng.integers(0, len(patterns), len(holds_nan))]
        values[holds_nan[:3]] = patterns
    nulls = rng.random(n) < 0.1
    return values, nulls


def run_column(name, nan=False, seed=0, n=N):
    """(values, nulls) in runs: two runs longer than a wave's 2048 rows, 300 runs of one row, runs of 2 .. 60 rows; every third run holds a limit
    value, about 15 % of the runs are NULL, with nan about 5 % hold a NaN."""
    rng = np.random.default_rng(2_000 + seed + sum(map(ord, name)))
    lengths = [2_500, 1, 1, 3_000] + [1] * 300
    while sum(lengths) < n:
        lengths.append(int(rng.integers(2, 61)))
    lengths = np.array(lengths)
    order = rng.permutation(len(lengths) - 4) + 4            # (the long runs stay in front: they lie inside the first chunk)
    lengths = np.concatenate([lengths[:4], lengths[order]])
    edge = limits(name)
    per_run = random_values(rng, name, len(lengths))
    per_run[::3] = edge[rng.integers(0, len(edge), len(per_run[::3]))]
    per_run[:len(edge) * 3:3] = edge
    if nan:
        patterns = nan_patterns(name)
        holds_nan = np.flatnonzero(rng.random(len(lengths)) < 0.05)
        per_run[holds_nan] = patterns[rng.integers(0, len(patterns), len(holds_nan))]
        per_run[[1, 2, 5]] = patterns                        # (rows 2500 and 2501: two NaN runs of one row next to each other)
    null_run = rng.random(len(lengths)) < 0.15
    null_run[0] = False
    return np.repeat(per_run, lengths)[:n].copy(), np.repeat(null_run, lengths)[:n].copy()


def sorted_chunks(name, ascending, nulls_last, seed=0):
    """Chunks sorted on their own: [(values, nulls)].  Chunk 0: the limit values (duplicated) among 3000 random values, 100 NULLs (several rounds of
    a 64-ary search); chunk 1: every limit value one to four times, no NULL; chunk 2: MIN MIN mid MAX MAX and one NULL."""
    rng = np.random.default_rng(3_000 + seed + sum(map(ord, name)))
    edge = limits(name)
    bodies = [(np.concatenate([np.repeat(edge, 3), random_values(rng, name, 3_000)]), 100),
              (np.repeat(edge, rng.integers(1, 5, len(edge))), 0),
              (edge[[0, 0, len(edge) // 2, -1, -1]], 1)]
    chunks = []
    for body, n_null in bodies:
        body = np.sort(body)
        if not ascending:
            body = body[::-1]
        filler, holes = np.zeros(n_null, dtype=body.dtype), np.ones(n_null, dtype=bool)
        values = np.concatenate([body, filler] if nulls_last else [filler, body])
        nulls = np.concatenate([np.zeros(len(body), dtype=bool), holes] if nulls_last else [holes, np.zeros(len(body), dtype=bool)])
        chunks.append((values, nulls))
    return chunks


FOR_SIZES = (3 * 2_048 + 3, 2_051, 5)


def frame_of_reference_column(narrow, seed=0):
    """int32 (values, nulls) for FOR_SIZES.  Chunk 0: three 2048-row blocks next to each other -- minimum INT32_MIN with offsets up to 2^32 - 1,
    values in [INT32_MAX - 200, INT32_MAX], values in [-300, 300] -- and three more rows.  narrow = False: the first recipe everywhere else too
    (4-byte offsets in every chunk).  narrow = True: chunk 0 without the first recipe (the last two, then the second again), so that every
    offset of the column fits 10 bits."""
    rng = np.random.default_rng(4_000 + seed + narrow)
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max

    def recipe(which, n):
        if which == 0:
            values = rng.integers(lo, hi, n, dtype=np.int32, endpoint=True)
            values[:2] = (lo, hi)                            # offsets 0 and 2^32 - 1
        elif which == 1:
            values = rng.integers(hi - 200, hi, n, dtype=np.int32, endpoint=True)
            values[:2] = (hi - 200, hi)
        else:
            values = rng.integers(-300, 300, n, dtype=np.int32, endpoint=True)
            values[:3] = (-300, 0, 300)
        return values

    if narrow:
        parts = [recipe(1, 2_048), recipe(2, 2_048), recipe(1, 2_048), recipe(2, 3), recipe(1, 2_048), recipe(2, 3), recipe(2, 5)]
    else:
        parts = [recipe(0, 2_048), recipe(1, 2_048), recipe(2, 2_048), recipe(0, 3), recipe(0, 2_051), recipe(0, 5)]
    values = np.concatenate(parts)
    nulls = rng.random(len(values)) < 0.1
    nulls[[0, 1, 2_048, 2_049, 4_096, 4_097, 4_098]] = False   # (the rows that pin the blocks' minima and widths)
    nulls[len(values) - 5:len(values) - 3] = False
    return values, nulls


# ---- literals -----------------------------------------------------------------------------------------------------------------------------
def single_literals(name):
    """Every limit value, as the one literal of the six comparisons."""
    return list(limits(name))


def between_pairs(name):
    t = TYPES[name]
    if not is_float(name):
        lo, hi = int(np.iinfo(t).min), int(np.iinfo(t).max)
        pairs = [(lo, hi), (lo, lo), (hi, hi), (hi, lo), (lo, lo + 1), (hi - 1, hi), (lo + 1, hi - 1), (lo + 1, lo), (hi, hi - 1), (lo + 1, lo + 1), (hi - 1, hi - 1),
                 (-1, 0), (0, 0), (0, 1), (-1, 1), (1, -1), (-1, -1), (lo, -1), (lo, 0), (0, hi), (-1, hi), (1, hi),
                 (-2**16 - 1, 2**16), (2**16, -2**16 - 1), (2**16, 2**16)]
        if name == "int32":
            pairs += [(-10**9, 10**9), (-2 * 10**9, -10**9), (10**9, 2 * 10**9), (-5, 5), (12_345, 2**30), (-2**30, -12_345)]
        else:
            pairs += [(2**32 - 1, 2**32 + 1), (-1, 2**32), (-2**32 - 1, -2**32), (-2**31 - 1, 2**31), (2**32, 2**32), (0, 2**32 - 1), (1, 2**32 + 1), (2**32 + 1, 1),
                      (2**53 + 1, 2**53 + 1), (2**32, hi), (lo, -2**32 - 1), (-4 * 10**18, 4 * 10**18), (10**18, 8 * 10**18), (-8 * 10**18, -10**18), (-2**40, 2**40)]
        return [(t(a), t(b)) for a, b in pairs]
    edge = limits(name)
    inf, big, tiny, denormal, exact = edge[-1], edge[-2], edge[8], edge[7], edge[10]
    zero, one, huge, small = t(0.0), t(1), t(1e30), t(1e-30)
    pairs = [(-big, big), (-big, -big), (big, big), (big, -big), (-zero, zero), (zero, -zero), (zero, zero), (-zero, -zero), (-inf, inf), (inf, -inf), (-inf, -inf), (inf, inf),
             (-denormal, denormal), (denormal, -denormal), (-tiny, tiny), (denormal, tiny), (zero, denormal), (-denormal, -zero), (-inf, -big), (big, inf), (-inf, zero),
             (-zero, inf), (one, exact), (exact, exact), (-one, one), (one, -one), (-one, -zero), (zero, one), (-huge, huge), (-small, small), (small, huge), (-huge, -small)]
    return [(t(a), t(b)) for a, b in pairs]


def nan_literals(name):
    """-> (single literals, between pairs) that hold a NaN."""
    t = TYPES[name]
    nan = nan_patterns(name)
    return [nan[0], nan[1]], [(nan[0], t(1)), (t(-1), nan[0]), (nan[0], nan[2]), (-t(np.inf), nan[1])]


def predicates(name, with_nan=False):
    """Every (condition, literal, literal2) of one column type: the six comparisons with every limit value, the four BETWEEN forms with every
    pair, IS NULL and IS NOT NULL; with_nan (float types): the same with literals that are NaN."""
    out = [(c, v, None) for c in COMPARISONS for v in single_literals(name)]
    out += [(c, a, b) for c in BETWEENS for a, b in between_pairs(name)]
    out += [(c, None, None) for c in NULL_TESTS]
    if with_nan:
        singles, pairs = nan_literals(name)
        out += [(c, v, None) for c in COMPARISONS for v in singles]
        out += [(c, a, b) for c in BETWEENS for a, b in pairs]
    return out
