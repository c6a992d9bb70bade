"""The numpy models of tests/row_op_models.py against brute-force Python loops, and the preconditions of every input
set tests/test_gpu_row_ops.py uses - so that the GPU tests rest on statements that were checked without a GPU and no
GPU case is silently vacuous."""

from __future__ import annotations

import struct

import numpy as np
import pytest

from tests import row_op_models as m


def _rng(seed):
    return np.random.default_rng(seed)


# ---- models against loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
def test_gather_fixed_model(dtype):
    src = _rng(1).integers(1, 200, 37).astype(dtype)
    idx = np.concatenate([_rng(2).integers(0, 37, 40), [-1, 37, 0, 36]]).astype(np.int64)
    for n_eff in (0, 1, 40, 42, 44):
        got, bad = m.gather_fixed(src, idx, n_eff)
        want = [int(src[r]) if 0 <= r < 37 else 0 for r in idx[:n_eff]]
        assert got.dtype == dtype and got.tolist() == want
        assert bad == any(not 0 <= r < 37 for r in idx[:n_eff])


def test_gather_strings_model():
    rows = [b"", b"a", b"\x00\xff", b"hello world", b"", b"z" * 255]
    lens, data, offs = m.column_arrays(rows)
    assert offs.tolist() == [0, 0, 1, 3, 14, 14, 269] and bytes(data) == b"".join(rows)
    assert m.gather_strings(lens, data, None) == (rows, False)
    idx = [5, 0, 3, 3, 2]
    assert m.gather_strings(lens, data, idx) == ([rows[r] for r in idx], False)
    assert m.gather_strings(lens, data, [1, -1, 6, 2]) == ([b"a", b"", b"", b"\x00\xff"], True)
    assert m.gather_strings(lens[:0], data[:0], None) == ([], False)


def test_concat_model():
    a = [b"x" * k for k in (0, 1, 200, 255, 100)]
    b = [b"y" * k for k in (0, 3, 55, 1, 155)]
    lens, data, too_long = m.concat([a, b"--", b], 5)
    want = []
    for i in range(5):
        text = bytearray()
        for part in (a[i], b"--", b[i]):
            for ch in part:
                if len(text) < 255:
                    text.append(ch)
        want.append(bytes(text))
    assert lens.tolist() == [2, 6, 255, 255, 255] == [len(w) for w in want]
    assert data == b"".join(want) and too_long
    lens2, data2, long2 = m.concat([a, b], 2)
    assert lens2.tolist() == [0, 4] and data2 == b"xyyy" and long2 is False
    lens3, _, long3 = m.concat([a[4:], b"", b[4:]], 1)
    assert lens3.tolist() == [255] and long3 is False  # 255 exactly is not too long
    lens0, data0, long0 = m.concat([a], 0)
    assert lens0.tolist() == [] and data0 == b"" and not long0


@pytest.mark.parametrize("sizes", m.DICT_SIZES)
def test_dict_combine_model(sizes):
    strides = m.dict_strides(sizes)
    codes = m.dict_codes(sizes, 40)
    want = [sum(int(c[i]) * s for c, s in zip(codes, strides)) & 0xFF for i in range(40)]
    assert m.dict_combine(codes, strides).tolist() == want
    # mixed radix, the last part fastest: the code is the rank of the digit tuple
    digits = np.array(np.unravel_index(np.arange(int(np.prod(sizes))), sizes)).astype(np.uint8)
    assert m.dict_combine(list(digits), strides).tolist() == [v & 0xFF for v in range(int(np.prod(sizes)))]


def test_quantise_f64_model_is_struct_pack():
    """The reference writes a FLOAT with struct.pack('<f') (io.py:94): it keeps subnormals, rounds to nearest even and
    raises OverflowError for a finite value that does not fit."""
    x = m.quantise_f64_inputs()
    got, _ = m.quantise_f64(x)
    bits = got.view(np.uint32)
    raised = []
    for v, b in zip(x.tolist(), bits.tolist()):
        try:
            packed = struct.unpack("<I", struct.pack("<f", v))[0]
        except OverflowError:
            raised.append(v)
            assert b & 0x7FFFFFFF == 0x7F800000  # the model says infinite
            continue
        assert packed == b or (v != v and b & 0x7FC00000 == 0x7FC00000), (v, hex(packed), hex(b))
    assert m.quantise_f64(x)[1] is True and raised
    for v in raised:
        assert m.quantise_f64(np.array([v]))[1] is True
    keep = np.array([v for v in x.tolist() if v not in raised])
    assert m.quantise_f64(keep)[1] is False  # +-inf and NaN among them: no overflow
    # subnormal results, the tie to even in both parities
    f = lambda v: int(m.quantise_f64(np.array([v]))[0].view(np.uint32)[0])  # noqa: E731
    assert [f(2.0**-150), f(1.5 * 2.0**-150), f(1.5 * 2.0**-149), f(2.5 * 2.0**-149), f(2.0**-127)] == [0, 1, 2, 2, 1 << 22]
    assert [f(1 + 2.0**-24), f(1 + 3 * 2.0**-24)] == [0x3F800000, 0x3F800002]


def test_quantise_i64_model():
    x = m.quantise_i64_inputs()
    got, over = m.quantise_i64(x)
    for v, g in zip(x.tolist(), got.tolist()):
        low = v & 0xFFFFFFFF
        assert g == (low - 2**32 if low >= 2**31 else low)
    assert over
    for v in x.tolist():
        assert m.quantise_i64(np.array([v]))[1] == (not -(2**31) <= v < 2**31)


def test_exclusive_scan_model():
    x = _rng(3).integers(0, 2**40, 50)
    want, run = [], 0
    for v in x.tolist():
        want.append(run)
        run += v
    assert m.exclusive_scan(x).tolist() == want + [run]
    assert m.exclusive_scan(np.zeros(0, dtype=np.int64)).tolist() == [0]


def test_lower_bound_model():
    for name, lst in m.lower_bound_lists().items():
        lst = lst[:60]
        q = m.lower_bound_queries(lst)
        want = [sum(1 for v in lst.tolist() if v < x) for x in q.tolist()]
        assert m.lower_bound(lst, q).tolist() == want, name


def _expand_loop(bounds, values, n):
    out = []
    for i in range(n):
        hit = [s for s in range(len(values)) if bounds[s] <= i < bounds[s + 1]]
        assert len(hit) == 1
        out.append(int(values[hit[0]]))
    return out


def test_expand_by_bounds_model():
    seen = 0
    for name, (bounds, values, n) in m.expand_cases().items():
        if n > 2000:
            continue
        seen += 1
        assert m.expand_by_bounds(bounds, values, n).tolist() == _expand_loop(bounds.tolist(), values, n), name
    assert seen >= 6
    # duplicate bounds = empty segments: front, two in a row, end
    assert m.expand_by_bounds([0, 0, 2, 2, 2, 3, 3], [10, 11, 12, 13, 14, 15], 3).tolist() == [11, 11, 14]


def test_remap_and_minmax_models():
    lut = m.remap_luts()["permutation"]
    codes = m.remap_codes(300)
    assert m.remap(codes, lut).tolist() == [int(lut[c]) for c in codes.tolist()]
    assert m.minmax(np.zeros(0, dtype=np.int32)) == (m.INT32_MAX, m.INT32_MIN)
    x = m.minmax_values(37, "limits")
    lo, hi = m.INT32_MAX, m.INT32_MIN
    for v in x.tolist():
        lo, hi = min(lo, v), max(hi, v)
    assert m.minmax(x) == (lo, hi) == (m.INT32_MIN, m.INT32_MAX)


# ---- preconditions of the GPU input sets --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [s for s in m.GATHER_SIZES if s])
def test_gather_index_sets_stay_in_range(n):
    for src_rows in (1, n + 3):
        sets = m.gather_indices(n, src_rows)
        assert set(sets) == {"repeats", "reversed", "same_row"}
        for name, idx in sets.items():
            assert idx.dtype == np.int64 and len(idx) == n and idx.min() >= 0 and idx.max() < src_rows, name
        if src_rows > 1 and n > 100:
            assert len(np.unique(sets["repeats"])) < n  # it does repeat
            assert (np.diff(sets["reversed"]) < 0).all()
    assert (m.gather_source(1, 300) != 0).all()
    assert m.n_dev_values(n)[0] is None and {0, 1, n - 1, n, n + 7} <= set(m.n_dev_values(n)[1:])


def test_guarded_indices_hold_only_the_two_permitted_bad_values():
    for n, src_rows in [(300, 100), (40, 7)]:
        idx = m.guarded_indices(n, src_rows)
        bad = idx[(idx < 0) | (idx >= src_rows)]
        assert sorted(bad.tolist()) == [-1] * 3 + [src_rows] * 3
    assert m.GATHER_ABOVE_CAP > 65536 * 256 and m.DICT_ABOVE_CAP > 8192 * 256 * 16 and m.EXPAND_ABOVE_CAP > 4096 * 256


@pytest.mark.parametrize("last_len", [None] + m.LAST_ROW_LENGTHS)
def test_alignment_grid_is_complete(last_len):
    rows = m.alignment_grid_column(last_len=last_len)
    pairs = m.alignment_pairs(rows)
    missing = [(r, ln) for r in range(8) for ln in m.GRID_LENGTHS if (r, ln) not in pairs]
    assert not missing
    lens = {len(r) for r in rows}
    assert set(m.LONG_LENGTHS) <= lens and max(lens) == 255
    payload = b"".join(rows)
    assert set(payload) == set(range(256))
    if last_len is not None:
        assert len(rows[-1]) == last_len and payload.endswith(rows[-1])
    # not in any regular order: lengths neither ascending nor periodic in 8
    ln = [len(r) for r in rows]
    assert ln != sorted(ln) and ln[:64] != ln[8:72]
    for name, idx in m.string_gather_indices(len(rows)).items():
        if idx is not None:
            assert idx.min() >= 0 and idx.max() < len(rows), name
    assert sorted(m.string_gather_indices(len(rows))["permutation"].tolist()) == list(range(len(rows)))


@pytest.mark.parametrize("name", list(m.CONCAT_CASES))
@pytest.mark.parametrize("n", m.CONCAT_SIZES)
def test_concat_inputs_hold_their_special_rows(name, n):
    parts, specs, special = m.concat_inputs(name, n)
    assert len(parts) == len(specs) <= 8
    for p, s in zip(parts, specs):
        if s[0] == "lit":
            assert p == s[1]
        else:
            assert len(p) == n and all(len(r) <= 255 for r in p)
            if s[0] == "fixed":
                assert all(len(r) == s[1] for r in p)
            if s[0] == "empty":
                assert all(r == b"" for r in p)
    totals = [sum(len(p) if isinstance(p, bytes) else len(p[i]) for p in parts) for i in range(n)]
    for row, t in special.items():
        assert totals[row] == t
    for i, t in enumerate(totals):
        if i not in special:
            assert 1 <= t <= 120  # ordinary rows: short, never empty
    for row, t in special.items():
        if t > 255 and row + 1 < n and row + 1 not in special:
            assert totals[row + 1] >= 1  # the row after an over-long row has a first byte of its own
    assert sorted(set(special.values())) == sorted(set(m.CONCAT_CASES[name][1][n]))
    assert m.concat(parts, n)[2] == any(t > 255 for t in totals)


def test_concat_cases_cover_the_totals_and_kinds():
    assert sorted(len(specs) for specs, _ in m.CONCAT_CASES.values()) == [1, 2, 3, 8, 8]
    kinds = {s[0] for specs, _ in m.CONCAT_CASES.values() for s in specs}
    assert kinds == {"var", "fixed", "lit", "empty"}
    assert any(s == ("lit", b"") for specs, _ in m.CONCAT_CASES.values() for s in specs)
    totals = {t for _, by_n in m.CONCAT_CASES.values() for ts in by_n.values() for t in ts}
    assert {255, 256, 300, 2040} <= totals
    assert any(not ts for _, by_n in m.CONCAT_CASES.values() for n, ts in by_n.items() if n)  # a call without a long row


@pytest.mark.parametrize("sizes", m.DICT_SIZES)
def test_dictionary_products_fit_a_code_byte(sizes):
    assert 1 <= len(sizes) <= 4 and int(np.prod(sizes)) <= 256
    strides = m.dict_strides(sizes)
    assert strides[-1] == 1
    for n in m.DICT_ROWS:
        codes = m.dict_codes(sizes, n)
        assert all(len(c) == n and c.dtype == np.uint8 for c in codes)
        if n:
            assert all(int(c.max()) < sz for c, sz in zip(codes, sizes))
            assert max(sum(int(c[i]) * s for c, s in zip(codes, strides)) for i in range(n)) <= 255
    assert sorted({len(s) for s in m.DICT_SIZES}) == [1, 2, 3, 4]


def test_quantise_inputs_hold_the_named_values():
    x = m.quantise_f64_inputs()
    f32max = float(np.finfo(np.float32).max)
    bits = set(x.view(np.uint64).tolist())
    for v in [0.0, -0.0, f32max, -f32max, np.nextafter(f32max, np.inf), np.nextafter(f32max, 0.0), f32max + 2.0**103,
              2.0**-126, 2.0**-127, 2.0**-149, 2.0**-150, 1.5 * 2.0**-150, 1 + 2.0**-24, 1 + 3 * 2.0**-24, np.inf, -np.inf]:
        assert int(np.float64(v).view(np.uint64)) in bits, v
    assert np.isnan(x).sum() == 1
    y, _ = m.quantise_f64(x)
    tiny = np.abs(y[np.isfinite(y)])
    assert ((tiny > 0) & (tiny < 2.0**-126)).sum() > 100  # results in the f32 subnormal range
    i = m.quantise_i64_inputs().tolist()
    assert {2**31, -(2**31), 2**31 - 1, -(2**31) - 1, 2**62} <= set(i)
    for n_cols in m.QUANT_MANY_COLS:
        for n in m.QUANT_MANY_ROWS:
            cols = m.quantise_many_inputs(n_cols, n)
            assert len(cols) == n_cols and all(len(v) == n for _, v in cols)
            if n_cols > 1:
                assert {k for k, _ in cols} == {"f64", "i64"}
            for kind, v in cols:
                model = m.quantise_f64 if kind == "f64" else m.quantise_i64
                assert model(v)[1] is True and model(v[:-1])[1] is False  # only the last row overflows


def test_scan_values_pass_2_to_the_53():
    x = m.scan_values()
    assert len(x) == m.SCAN_ROUND + 1 and x.min() >= 0 and x.max() < 2**40
    assert int(x[: m.SCAN_ROUND - 1].sum()) > 2**53
    assert m.SCAN_ROUND == 2048 * 2048 and {m.SCAN_ROUND - 1, m.SCAN_ROUND, m.SCAN_ROUND + 1, 0, 1, 2047, 2048, 2049} == set(m.SCAN_SIZES)


def test_lower_bound_lists_are_ascending_with_runs():
    lists = m.lower_bound_lists()
    assert sorted(len(v) for v in lists.values()) == [0, 1, 1000, 1000]
    for name, lst in lists.items():
        assert lst.dtype == np.int64 and (np.diff(lst.astype(object)) >= 0).all(), name
        q = m.lower_bound_queries(lst)
        assert {m.INT64_MIN, m.INT64_MAX} <= set(q.tolist())
        for v in np.unique(lst).tolist()[:50]:
            assert {v - 1, v, v + 1} <= set(q.tolist())
        for cap in m.lower_bound_caps(lst):
            assert 0 <= cap <= len(lst)
    runs = lists["runs"]
    assert len(np.unique(runs)) < 200  # runs of duplicates
    caps = m.lower_bound_caps(runs)
    assert caps[0] == 0 and len(caps) == 2
    assert runs[caps[1] - 1] == runs[caps[1]]  # the cap falls inside a run


def test_expand_cases_meet_their_preconditions():
    cases = m.expand_cases()
    assert {len(v) for _, v, _ in cases.values()} >= {1, 2, 7, 1000}
    for name, (bounds, values, n) in cases.items():
        n_seg = len(values)
        assert len(bounds) == n_seg + 1 and bounds[0] == 0 and (np.diff(bounds) >= 0).all() and bounds[n_seg] >= n > 0, name
    sizes = np.diff(cases["seven_with_gaps"][0]).tolist()
    assert sizes[0] == 0 and sizes[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(sizes[1:-1], sizes[2:-1]))
    assert cases["thousand_above_cap"][2] == m.EXPAND_ABOVE_CAP
    big = np.diff(cases["thousand_above_cap"][0])
    assert big[0] == 0 and big[500] == 0 and big[501] == 0 and big[-1] == 0


def test_remap_and_minmax_inputs():
    luts = m.remap_luts()
    assert sorted(luts["permutation"].tolist()) == list(range(256)) and len(set(luts["constant"].tolist())) == 1
    assert luts["permutation"].tolist() != list(range(256))
    assert set(m.remap_codes(2049).tolist()) == set(range(256))
    assert m.REMAP_SIZES[-1] > 4096 * 2048 and m.MINMAX_SIZES[-1] > 1024 * 4096
    for n in m.MINMAX_SIZES[:-1]:
        for placing in m.MINMAX_PLACINGS:
            x = m.minmax_values(n, placing)
            assert len(x) == n and x.dtype == np.int32
            if n == 0:
                continue
            lo, hi = m.minmax(x)
            if placing == "limits":
                assert hi == m.INT32_MAX and (n == 1 or lo == m.INT32_MIN or x.tolist().count(m.INT32_MAX) == 1)
                continue
            assert m.MINMAX_SLACK[0] < lo and hi < m.MINMAX_SLACK[1]  # the slack values would change either result
            if n > 1:
                pos = n - 1 if placing.endswith("last") else 0
                ext = hi if placing.startswith("max") else lo
                assert x[pos] == ext and x.tolist().count(ext) == 1  # the extreme sits there and nowhere else
