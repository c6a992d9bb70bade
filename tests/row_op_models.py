"""Plain numpy / Python statements of the row-moving operators of include/hipspark.h (gathers, string assembly, the
small device utilities), and the input sets tests/test_gpu_row_ops.py feeds them.

The models are checked against brute-force loops in tests/test_row_op_models.py, which also asserts that every input
set built here stays inside the preconditions of the operator it is meant for - both without a GPU.  A string column
is a list of ``bytes``, one per row; ``column_arrays`` gives the (lens, data, offs) arrays the device holds."""

from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1
MAX_STR = 255  # a BlockFile length byte


# ---- models -------------------------------------------------------------------------------------------------------
def gather_fixed(src, idx, n_eff):
    """out[i] = src[idx[i]] for i < n_eff; an index outside the source reads as zero.  -> (values, any index bad)"""
    idx = np.asarray(idx[:n_eff], dtype=np.int64)
    bad = (idx < 0) | (idx >= len(src))
    out = np.zeros(len(idx), dtype=src.dtype)
    out[~bad] = src[idx[~bad]]
    return out, bool(bad.any())


def gather_strings(lens, data, idx):
    """Row idx[i] of the column (lens, data); idx None = every row in order; an index outside the column gathers the
    empty string.  -> (list of bytes, any index bad)"""
    data = bytes(data)
    offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    rows = range(len(lens)) if idx is None else [int(r) for r in idx]
    out, bad = [], False
    for r in rows:
        if 0 <= r < len(lens):
            out.append(data[offs[r]: offs[r] + int(lens[r])])
        else:
            out.append(b"")
            bad = True
    return out, bad


def concat(parts, n):
    """Row-wise '+' of the parts (a column = list of bytes, or a literal bytes); a row is the first 255 bytes of the
    Python concatenation.  -> (lens uint8[n], all bytes, any row was longer than 255)"""
    lens, out, too_long = np.zeros(n, dtype=np.uint8), [], False
    for i in range(n):
        text = b"".join(p if isinstance(p, bytes) else p[i] for p in parts)
        too_long = too_long or len(text) > MAX_STR
        text = text[:MAX_STR]
        lens[i] = len(text)
        out.append(text)
    return lens, b"".join(out), too_long


def dict_combine(codes, strides):
    acc = np.zeros(len(codes[0]), dtype=np.uint32)
    for c, s in zip(codes, strides):
        acc += c.astype(np.uint32) * np.uint32(s)
    return (acc & 0xFF).astype(np.uint8)


def quantise_f64(x):
    """-> (x as float32, overflow: some result is infinite where the input was finite)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = x.astype(np.float32)
    return y, bool((np.isinf(y) & np.isfinite(x)).any())


def quantise_i64(x):
    """-> (the low 32 bits as int32, overflow: some value lies outside [-2**31, 2**31))"""
    x = np.asarray(x, dtype=np.int64)
    y = (x.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return y, bool(((x < INT32_MIN) | (x > INT32_MAX)).any())


def exclusive_scan(x):
    """-> start[n + 1], start[n] = the total"""
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(x, dtype=np.int64))])


def lower_bound(sorted_list, q):
    return np.searchsorted(np.asarray(sorted_list, dtype=np.int64), np.asarray(q, dtype=np.int64), "left").astype(np.int64)


def expand_by_bounds(bounds, values, n):
    n_seg = len(values)
    seg = np.searchsorted(np.asarray(bounds[:n_seg], dtype=np.int64), np.arange(n, dtype=np.int64), "right") - 1
    return np.asarray(values, dtype=np.int64)[seg]


def remap(codes, lut):
    return np.asarray(lut, dtype=np.uint8)[np.asarray(codes, dtype=np.uint8)]


def minmax(x):
    """-> (min, max); of nothing: (INT32_MAX, INT32_MIN)"""
    return (int(np.min(x)), int(np.max(x))) if len(x) else (INT32_MAX, INT32_MIN)


# ---- helpers ------------------------------------------------------------------------------------------------------
def column_arrays(rows):
    """list of bytes -> (lens uint8[n], data uint8[total], offs int64[n + 1])"""
    lens = np.array([len(r) for r in rows], dtype=np.uint8)
    data = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return lens, data, exclusive_scan(lens)


def rows_of(lens, data):
    return gather_strings(lens, data, None)[0]


# ---- input sets: gathers ------------------------------------------------------------------------------------------
GATHER_SIZES = [0, 1, 255, 256, 257, 5000]
GATHER_ABOVE_CAP = 65536 * 256 + 257  # grid_for's 65536 blocks of 256 lanes, and a ragged rest


def gather_source(elem_bytes, src_rows, seed=1):
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[elem_bytes]
    rng = np.random.default_rng(seed)
    return rng.integers(1, np.iinfo(dt).max, src_rows, dtype=dt, endpoint=True)  # never zero: zero marks a refused row


def gather_indices(n, src_rows, seed=2):
    """name -> int64[n], every index inside [0, src_rows)"""
    rng = np.random.default_rng(seed)
    return {
        "repeats": rng.integers(0, max(src_rows // 3, 1), n).astype(np.int64),
        "reversed": (np.arange(n, dtype=np.int64)[::-1] % src_rows).copy(),
        "same_row": np.full(n, src_rows - 1, dtype=np.int64),
    }


def n_dev_values(n):
    """The device-side counts a capped operator is run with (None = no count); n + 7 is larger than n, where n rules."""
    return [None] + sorted({v for v in (0, 1, n - 1, n, n + 7) if v >= 0})


def guarded_indices(n, src_rows, seed=3):
    """Good indices with a few -1 and src_rows among them - the only out-of-range values used anywhere."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, src_rows, n).astype(np.int64)
    where = rng.choice(n, size=6, replace=False)
    idx[where[:3]] = -1
    idx[where[3:]] = src_rows
    return idx


GRID_LENGTHS = list(range(18))
LONG_LENGTHS = [24, 31, 32, 33, 255]
LAST_ROW_LENGTHS = [1, 7, 8, 9, 16]


def alignment_grid_column(seed=4, last_len=None):
    """A variable-length column whose rows start at every residue 0..7 (given an 8-aligned buffer) with every length
    0..17, plus the long lengths; payload over all 256 byte values.  last_len: one more row of that length at the end,
    which then ends on the last byte of the payload.  -> list of bytes"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(0, 18, 3000), LONG_LENGTHS, LONG_LENGTHS]).astype(np.int64)
    rng.shuffle(lens)
    if last_len is not None:
        lens = np.concatenate([lens, [last_len]])
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    data[:2] = [0x00, 0xFF]
    return rows_of(lens, data)


def alignment_pairs(rows):
    """{(start offset % 8, length)} of a column"""
    lens, _, offs = column_arrays(rows)
    return {(int(o) % 8, int(ln)) for o, ln in zip(offs[:-1], lens)}


def fixed_width_column(width, n, seed=5):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n * width, dtype=np.uint8).tobytes()
    return [data[i * width: (i + 1) * width] for i in range(n)]


def string_gather_indices(n_src, seed=6):
    """name -> int64 index list (None: identity) into a column of n_src rows"""
    rng = np.random.default_rng(seed)
    return {
        "permutation": rng.permutation(n_src).astype(np.int64),
        "repeats": rng.integers(0, n_src, n_src + 300).astype(np.int64),
        "identity": None,
    }


# ---- input sets: concatenation ------------------------------------------------------------------------------------
# a part: ("var",) variable-length column, ("fixed", w) fixed-length column, ("lit", bytes), ("empty",) all-empty column
CONCAT_CASES = {
    # name: (parts, {n: totals of the special rows})
    "one": ([("var",)], {0: [], 1: [], 257: [255], 3000: [255]}),
    "two": ([("var",), ("lit", b"-x")], {0: [], 1: [256], 257: [255, 256], 3000: [255, 256, 257]}),
    "three": ([("fixed", 3), ("lit", b""), ("var",)], {0: [], 1: [], 257: [255], 3000: [255, 256, 258]}),
    "eight_mixed": ([("var",), ("lit", b"::"), ("fixed", 4), ("empty",), ("var",), ("lit", b""), ("fixed", 16), ("var",)],
                    {0: [], 1: [300], 257: [255, 256, 300], 3000: [255, 256, 300, 787]}),
    "eight_var": ([("var",)] * 8, {0: [], 1: [2040], 257: [255, 256, 300, 2040], 3000: [255, 256, 300, 2040]}),
}
CONCAT_SIZES = [0, 1, 257, 3000]


def concat_inputs(name, n, seed=7):
    """-> (parts for ``concat``, part specs, rows holding a special total: {row: total}).  Ordinary rows are short and
    never empty; a special row of total T sits between ordinary rows, and where any total is over-long the LAST row is
    one too (a write past its 255 bytes lands in the canary)."""
    specs, by_n = CONCAT_CASES[name]
    totals = list(by_n[n])
    rng = np.random.default_rng(seed + n)
    static = sum(s[1] if s[0] == "fixed" else len(s[1]) if s[0] == "lit" else 0 for s in specs)
    n_var = sum(s[0] == "var" for s in specs)
    special = {}
    if totals:
        if n == 1:
            special[0] = totals[0]
        else:
            step = n // (len(totals) + 1)
            assert step >= 2
            for k, t in enumerate(totals):
                special[(k + 1) * step] = t
            if max(totals) > MAX_STR:
                special[n - 1] = max(totals)
    var_lens = rng.integers(0, 13, (n, n_var))
    var_lens[:, 0] += 1  # no ordinary row is empty
    for row, t in special.items():
        left = t - static
        assert 0 <= left <= MAX_STR * n_var, (name, t)
        for k in range(n_var):
            var_lens[row, k] = min(MAX_STR, left)
            left -= var_lens[row, k]
    parts, k = [], 0
    for s in specs:
        if s[0] == "var":
            col_lens = var_lens[:, k]
            parts.append(rows_of(col_lens, rng.integers(0, 256, int(col_lens.sum()), dtype=np.uint8)))
            k += 1
        elif s[0] == "fixed":
            parts.append(fixed_width_column(s[1], n, seed=seed + 31 * len(parts)))
        elif s[0] == "lit":
            parts.append(s[1])
        else:
            parts.append([b""] * n)
    return parts, specs, special


# ---- input sets: dictionaries -------------------------------------------------------------------------------------
DICT_SIZES = [(256,), (16, 16), (4, 8, 8), (2, 2, 2, 32)]
DICT_ROWS = [0, 1, 15, 16, 17, 4095, 4096, 4097]
DICT_ABOVE_CAP = 8192 * 256 * 16 + 33  # hsj_grid's 8192 blocks of 256 lanes of 16 rows, and a ragged rest


def dict_strides(sizes):
    """As Device.dict_concat computes them: the last part varies fastest."""
    strides, acc = [], 1
    for sz in reversed(sizes):
        strides.insert(0, acc)
        acc *= sz
    return strides


def dict_codes(sizes, n, seed=8):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, sz, n).astype(np.uint8) for sz in sizes]


# ---- input sets: quantisation -------------------------------------------------------------------------------------
def quantise_f64_inputs(seed=9):
    rng = np.random.default_rng(seed)
    f32max = float(np.finfo(np.float32).max)
    half_ulp_max = 2.0**103  # half the distance between the two largest finite f32
    one, ulp = 1.0, 2.0**-23
    sub = 2.0**-149  # the smallest f32 subnormal
    ties = [one + ulp / 2, one + 3 * ulp / 2, one + 5 * ulp / 2, 2.0**24 + 1.0, 2.0**24 + 3.0,  # even below / odd below
            0.5 * sub, 1.5 * sub, 2.5 * sub, 3.5 * sub, (2**23 - 0.5) * sub, (2**23 + 0.5) * sub]
    edges = [0.0, f32max, np.nextafter(f32max, np.inf), np.nextafter(f32max, 0.0), f32max + half_ulp_max,
             np.nextafter(f32max + half_ulp_max, 0.0), np.nextafter(f32max + half_ulp_max, np.inf), 2.0**128, 1e39, 1e308,
             2.0**-126, np.nextafter(2.0**-126, 0.0), np.nextafter(2.0**-126, 1.0), 2.0**-127, 2.0**-149, 2.0**-150,
             np.nextafter(2.0**-150, 0.0), np.nextafter(2.0**-150, 1.0), 1.5 * 2.0**-150, 2.0**-151, 5e-324, 1e-50]
    near = [np.nextafter(t, 0.0) for t in ties] + [np.nextafter(t, np.inf) for t in ties]
    pos = np.array(edges + ties + near, dtype=np.float64)
    between = rng.random(200) * 2.0**-126
    scaled = rng.normal(size=1000) * np.exp2(rng.integers(-160, 131, 1000).astype(np.float64))
    return np.concatenate([pos, -pos, between, -between, [np.inf, -np.inf, np.nan], scaled])


def quantise_i64_inputs():
    return np.array([0, 1, -1, 2**31, -(2**31), 2**31 - 1, -(2**31) - 1, 2**62, -(2**62), 2**32, 2**32 + 5, INT64_MAX,
                     INT64_MIN], dtype=np.int64)


QUANT_MANY_COLS = [1, 2, 15, 16]
QUANT_MANY_ROWS = [1, 255, 257, 5000]


def quantise_many_inputs(n_cols, n, seed=10):
    """-> [(kind, values)], kind 'f64' / 'i64' alternating.  Ordinary values everywhere; the LAST row of every column
    overflows, so a count that stops short of it must leave the flags alone."""
    rng = np.random.default_rng(seed + n_cols)
    cols = []
    for c in range(n_cols):
        if c % 2 == 0:
            v = rng.normal(size=n) * np.exp2(rng.integers(-160, 100, n).astype(np.float64))
            v[-1] = 1e39 * (c + 1)
            cols.append(("f64", v))
        else:
            v = rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True).astype(np.int64)
            v[-1] = 2**31 + c
            cols.append(("i64", v))
    return cols


# ---- input sets: scan, searches -----------------------------------------------------------------------------------
SCAN_ROUND = 2048 * 2048  # elements one k_scan_tiles round covers: 2048 tile sums of 2048-element tiles
SCAN_SIZES = [0, 1, 2047, 2048, 2049, SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1]


def scan_values(seed=11):
    """SCAN_ROUND + 1 values in [0, 2**40): every size of SCAN_SIZES is a prefix of it."""
    return np.random.default_rng(seed).integers(0, 2**40, SCAN_ROUND + 1).astype(np.int64)


def lower_bound_lists(seed=12):
    """name -> ascending int64 list with runs of duplicates"""
    rng = np.random.default_rng(seed)
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "one": np.array([42], dtype=np.int64),
        "runs": np.sort(rng.integers(-60, 60, 1000) * 1000).astype(np.int64),
        "wide": np.sort(np.concatenate([rng.integers(INT64_MIN + 1, INT64_MAX, 990), [INT64_MIN + 1] * 5, [INT64_MAX - 1] * 5])).astype(np.int64),
    }


def lower_bound_queries(sorted_list):
    """Below, equal to and above every distinct value, and the two ends of int64."""
    d = np.unique(sorted_list).astype(object)
    q = [INT64_MIN, INT64_MAX, 0]
    for v in d:
        q += [max(v - 1, INT64_MIN), v, min(v + 1, INT64_MAX)]
    return np.array(q, dtype=np.int64)


def lower_bound_caps(sorted_list):
    """Device-side lengths: 0, and one that cuts the longest run of duplicates in two."""
    caps = [0]
    if len(sorted_list) > 1:
        vals, first, counts = np.unique(sorted_list, return_index=True, return_counts=True)
        k = int(np.argmax(counts))
        if counts[k] > 1:
            caps.append(int(first[k] + counts[k] // 2))
    return caps


EXPAND_ABOVE_CAP = 4096 * 256 + 300  # hs_expand_by_bounds' 4096 blocks of 256 lanes, and a ragged rest


def expand_cases(seed=13):
    """name -> (bounds int64[n_seg + 1], values int64[n_seg], n)"""
    rng = np.random.default_rng(seed)

    def from_sizes(sizes, n=None):
        bounds = exclusive_scan(np.array(sizes, dtype=np.int64))
        values = rng.integers(INT64_MIN, INT64_MAX, len(sizes)).astype(np.int64)
        return bounds, values, int(bounds[-1]) if n is None else n

    big = rng.integers(0, 2 * EXPAND_ABOVE_CAP // 1000, 1000)
    big[[0, 500, 501, 999]] = 0
    big[700] += EXPAND_ABOVE_CAP - big.sum() if big.sum() < EXPAND_ABOVE_CAP else 0
    return {
        "one_owns_all": from_sizes([777]),
        "two": from_sizes([300, 1]),
        "two_first_empty": from_sizes([0, 50]),
        "seven_with_gaps": from_sizes([0, 5, 0, 0, 259, 1, 0]),  # empty at the front, two in a row inside, at the end
        "all_but_one_empty": from_sizes([0, 0, 0, 600, 0, 0, 0]),
        "bounds_past_n": from_sizes([10, 20, 30], n=25),  # bounds[n_seg] > n: the last segments own nothing
        "thousand": from_sizes(rng.integers(0, 4, 1000)),
        "thousand_above_cap": from_sizes(big, n=EXPAND_ABOVE_CAP),
    }


# ---- input sets: remap, min / max ---------------------------------------------------------------------------------
REMAP_SIZES = [0, 1, 255, 2049, 4096 * 2048 + 77]  # the last: hsj_grid's 4096 blocks of 2048 rows, and a ragged rest


def remap_luts(seed=14):
    return {"permutation": np.random.default_rng(seed).permutation(256).astype(np.uint8),
            "constant": np.full(256, 0x7B, dtype=np.uint8)}


def remap_codes(n, seed=15):
    codes = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if n >= 256:
        codes[:256] = np.arange(256, dtype=np.uint8)[::-1]
    return codes


MINMAX_SIZES = [0, 1, 2, 3, 4, 5, 1023, 1024 * 4096 + 3]  # the last: hsj_grid's 1024 blocks of 4096 rows, and a rest
MINMAX_PLACINGS = ["max_last", "min_last", "max_first", "min_first", "limits"]
MINMAX_BODY = 1000  # ordinary elements lie in [-MINMAX_BODY, MINMAX_BODY]
MINMAX_SLACK = (-2_000_000, 2_000_000)  # written behind the n elements: beyond every element but the int32 limits


def minmax_values(n, placing, seed=16):
    rng = np.random.default_rng(seed)
    x = rng.integers(-MINMAX_BODY, MINMAX_BODY, n, endpoint=True).astype(np.int32)
    if n == 0:
        return x
    if placing == "max_last":
        x[-1] = MINMAX_BODY + 5
    elif placing == "min_last":
        x[-1] = -MINMAX_BODY - 5
    elif placing == "max_first":
        x[0] = MINMAX_BODY + 5
    elif placing == "min_first":
        x[0] = -MINMAX_BODY - 5
    else:
        x[rng.integers(0, n)] = INT32_MIN
        x[rng.integers(0, n)] = INT32_MAX  # (of one element: the later write stays)
    return x
