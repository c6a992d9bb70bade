"""The row-moving operators of include/hipspark.h at the C ABI, with no query engine in between: fixed-width and
STRING gathers, string concatenation, dictionary-code combination, quantisation, the int64 scan, lower bound, segment
expansion, byte remap and int32 min / max - each against its numpy statement in tests/row_op_models.py (verified on
the CPU by tests/test_row_op_models.py), bit for bit.

Canary rule: every output buffer is allocated at least 64 elements longer than the operator needs and pre-filled with
a fixed non-zero pattern; after every call everything past the last element the operator owns - and, where a
device-side count caps the call, every element at or beyond that count - must still hold the pattern.  Status bits go
to a flags word of the test's own, zeroed per test."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import row_op_models as m

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = 1, 2
GUARD = 64  # canary elements behind every output; source elements either side of a guarded view


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


@pytest.fixture()
def flags(dev):
    import torch

    word = dev.empty(1, torch.int32)
    word.zero_()
    return word


def _flags(word) -> int:
    return int(word.item()) & 0xFFFFFFFF


def _torch_dtype(np_dtype):
    import torch

    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[np.dtype(np_dtype).itemsize]


def _canary(dtype) -> int:
    return int.from_bytes(b"\x5a" * dtype.itemsize, "little")


def _out(dev, n, dtype, guard=GUARD):
    """An output buffer of n elements followed by `guard` canary elements, all of it pre-filled with the canary."""
    t = dev.empty(n + guard, dtype)
    t.fill_(_canary(dtype))
    return t


def _canary_intact(t, owned) -> bool:
    return bool((t[owned:] == _canary(t.dtype)).all().item())


def _host(t, np_dtype):
    return t.cpu().numpy().view(np_dtype)


def _up(dev, arr):
    """Upload a numpy array under an integer torch dtype of the same width (bit patterns, not values)."""
    arr = np.ascontiguousarray(arr)
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[arr.dtype.itemsize]
    return dev.to_device(arr.view(signed), _torch_dtype(arr.dtype))


def _up_whole(dev, arr):
    """Upload into the front of a buffer GUARD elements longer and return the WHOLE buffer: an array of no elements
    still gives the entry point a valid pointer (a zero-length tensor has none)."""
    arr = np.ascontiguousarray(arr)
    whole = dev.empty(len(arr) + GUARD, _torch_dtype(arr.dtype))
    whole.zero_()
    whole[: len(arr)] = _up(dev, arr)
    return whole


def _count(dev, value):
    import torch

    return None if value is None else dev.to_device(np.array([value], dtype=np.int64), torch.int64)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- hs_gather_fixed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", m.GATHER_SIZES)
@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
def test_gather_fixed(dev, flags, elem_bytes, n):
    import torch

    from minispark_amd import hipspark as hs

    for src_rows in sorted({1, n + 3}):
        src = m.gather_source(elem_bytes, src_rows)
        d_src = _up(dev, src)
        for name, idx in m.gather_indices(n, src_rows).items():
            d_idx = dev.to_device(idx, torch.int64)
            for cap in m.n_dev_values(n):
                d_cap = _count(dev, cap)
                out = _out(dev, n, d_src.dtype)
                hs.check(dev.lib.hs_gather_fixed(dev.stream, d_src.data_ptr(), elem_bytes, src_rows, d_idx.data_ptr(), n,
                                                 _ptr(d_cap), out.data_ptr(), flags.data_ptr()))
                n_eff = n if cap is None else min(n, cap)
                want, bad = m.gather_fixed(src, idx, n_eff)
                what = (name, src_rows, cap)
                assert not bad and np.array_equal(_host(out[:n_eff], src.dtype), want), what
                assert _canary_intact(out, n_eff), what  # rows [n_eff, n) and the tail are untouched
    assert _flags(flags) == 0


def test_gather_fixed_above_the_grid_cap(dev, flags):
    """More rows than 65536 blocks x 256 lanes: every lane runs its grid-stride loop a second time."""
    import torch

    from minispark_amd import hipspark as hs

    n, src_rows = m.GATHER_ABOVE_CAP, 100_003
    d_src = dev.empty(src_rows, torch.uint8)
    d_src.random_(1, 256)
    d_idx = dev.empty(n, torch.int64)
    d_idx.random_(0, src_rows)
    out = _out(dev, n, torch.uint8)
    hs.check(dev.lib.hs_gather_fixed(dev.stream, d_src.data_ptr(), 1, src_rows, d_idx.data_ptr(), n, None, out.data_ptr(),
                                     flags.data_ptr()))
    assert torch.equal(out[:n], d_src[d_idx])
    assert _canary_intact(out, n) and _flags(flags) == 0


def test_gather_fixed_refuses_other_widths(dev, flags):
    import torch

    d_src = dev.to_device(np.arange(12, dtype=np.uint8), torch.uint8)
    d_idx = dev.to_device(np.arange(4, dtype=np.int64), torch.int64)
    out = _out(dev, 12, torch.uint8)
    rc = dev.lib.hs_gather_fixed(dev.stream, d_src.data_ptr(), 3, 4, d_idx.data_ptr(), 4, None, out.data_ptr(), flags.data_ptr())
    assert rc == E_ARG
    assert _canary_intact(out, 0) and _flags(flags) == 0


@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
def test_gather_fixed_index_guard(dev, flags, elem_bytes):
    """Indices -1 and src_rows (the only out-of-range values used): zeros in exactly those rows, HS_FLAG_BAD_PROGRAM.
    The source is a view into the middle of a larger buffer, so even an unchecked read stays inside the allocation -
    and would return the non-zero neighbour, not the zero expected."""
    import torch

    from minispark_amd import hipspark as hs

    n, src_rows = 300, 100
    whole = m.gather_source(elem_bytes, src_rows + 2 * GUARD)
    src = whole[GUARD: GUARD + src_rows]
    d_src = _up(dev, whole)[GUARD: GUARD + src_rows]
    idx = m.guarded_indices(n, src_rows)
    d_idx = dev.to_device(idx, torch.int64)
    out = _out(dev, n, d_src.dtype)
    hs.check(dev.lib.hs_gather_fixed(dev.stream, d_src.data_ptr(), elem_bytes, src_rows, d_idx.data_ptr(), n, None,
                                     out.data_ptr(), flags.data_ptr()))
    want, bad = m.gather_fixed(src, idx, n)
    assert bad and _flags(flags) == hs.FLAG_BAD_PROGRAM
    got = _host(out[:n], src.dtype)
    assert np.array_equal(got, want)
    assert np.array_equal(got == 0, (idx < 0) | (idx >= src_rows))
    assert _canary_intact(out, n)


# ---- STRING gather: hs_gather_str_lens + hs_str_offsets + hs_gather_str_bytes -------------------------------------
class _StrCol:
    """A STRING column on the device, optionally as a view into larger buffers (GUARD rows / bytes either side)."""

    def __init__(self, dev, rows, fixed_len=-1, guarded=False):
        import torch

        from minispark_amd import hipspark as hs

        lens, data, offs = m.column_arrays(rows)
        self.rows, self.n, self.np_lens, self.np_data = rows, len(rows), lens, data
        if guarded:  # neighbours an unchecked row -1 / n would read: length 1 at offset 0, inside the payload
            lens = np.concatenate([np.ones(GUARD, np.uint8), lens, np.ones(GUARD, np.uint8)])
            offs = np.concatenate([np.zeros(GUARD, np.int64), offs, np.zeros(GUARD, np.int64)])
            data = np.concatenate([np.full(GUARD, 0x77, np.uint8), data, np.full(GUARD, 0x77, np.uint8)])
        lo = GUARD if guarded else 0
        self.lens = dev.to_device(lens, torch.uint8)[lo: lo + self.n]
        self.data = dev.to_device(data, torch.uint8)[lo: lo + len(self.np_data)]
        self.offs = dev.to_device(offs, torch.int64)[lo: lo + self.n + 1] if fixed_len < 0 else None
        self.hs = hs.hs_col()
        self.hs.kind = hs.STR
        self.hs.fixed_len = fixed_len
        self.hs.data = self.data.data_ptr()
        self.hs.lens = self.lens.data_ptr()
        self.hs.offs = _ptr(self.offs)


def _offsets(dev, lens, n):
    """hs_str_offsets over lens[0 .. n) into a canaried buffer -> (offs tensor, total)."""
    import torch

    from minispark_amd import hipspark as hs

    offs = _out(dev, n + 1, torch.int64)
    minmax = dev.empty(2, torch.int32)
    ws = dev.workspace(dev.lib.hs_scan_ws_bytes(n))
    hs.check(dev.lib.hs_str_offsets(dev.stream, lens.data_ptr(), n, offs.data_ptr(), minmax.data_ptr(), ws.data_ptr()))
    assert _canary_intact(offs, n + 1)
    return offs, int(offs[n].item())


def _gather_strings(dev, flags, col, idx, null_data=False):
    """The sequence Device.gather_col runs, every output canaried.  -> (lens, payload bytes)"""
    import torch

    from minispark_amd import hipspark as hs

    n = col.n if idx is None else len(idx)
    d_idx = None if idx is None else dev.to_device(idx, torch.int64)
    out_lens = _out(dev, n, torch.uint8)
    hs.check(dev.lib.hs_gather_str_lens(dev.stream, C.byref(col.hs), col.n, _ptr(d_idx), n, out_lens.data_ptr(), flags.data_ptr()))
    assert _canary_intact(out_lens, n)
    offs, total = _offsets(dev, out_lens, n)
    out_data = _out(dev, total, torch.uint8)
    hs.check(dev.lib.hs_gather_str_bytes(dev.stream, C.byref(col.hs), col.n, _ptr(d_idx), n, offs.data_ptr(),
                                         None if null_data else out_data.data_ptr()))
    assert _canary_intact(out_data, total)  # to the byte
    lens = out_lens[:n].cpu().numpy()
    assert np.array_equal(offs[: n + 1].cpu().numpy(), m.exclusive_scan(lens))
    return lens, out_data[:total].cpu().numpy().tobytes()


def _assert_gathered(dev, flags, col, idx, **kw):
    want_rows, bad = m.gather_strings(col.np_lens, col.np_data, idx)
    lens, payload = _gather_strings(dev, flags, col, idx, **kw)
    assert lens.tolist() == [len(r) for r in want_rows]
    assert payload == b"".join(want_rows)
    return bad


@pytest.mark.parametrize("last_len", [None] + m.LAST_ROW_LENGTHS)
def test_gather_strings_over_the_alignment_grid(dev, flags, last_len):
    """Every start address modulo 8 with every length 0..17 (hs_str_words16: one, two or three aligned words and a funnel
    shift), the byte loop above 16, and - last_len - a string that ends on the last byte of its buffer."""
    rows = m.alignment_grid_column(last_len=last_len)
    col = _StrCol(dev, rows)
    assert col.data.data_ptr() % 8 == 0  # the grid's residues are address residues
    assert col.data.numel() == sum(len(r) for r in rows)
    for name, idx in m.string_gather_indices(len(rows)).items():
        if last_len is not None and idx is not None:
            idx = np.concatenate([idx, [len(rows) - 1]])  # the last row, gathered last too
        assert not _assert_gathered(dev, flags, col, idx), name
    assert _flags(flags) == 0


@pytest.mark.parametrize("width", [0, 3, 16, 17])
def test_gather_strings_of_fixed_width(dev, flags, width):
    rows = m.fixed_width_column(width, 700)
    col = _StrCol(dev, rows, fixed_len=width)
    for name, idx in m.string_gather_indices(len(rows)).items():
        assert not _assert_gathered(dev, flags, col, idx), name
    assert _flags(flags) == 0


def test_gather_strings_all_empty_and_no_rows(dev, flags):
    import torch

    from minispark_amd import hipspark as hs

    col = _StrCol(dev, [b""] * 300)
    idx = m.string_gather_indices(300)["repeats"]
    assert not _assert_gathered(dev, flags, col, idx)
    assert not _assert_gathered(dev, flags, col, idx, null_data=True)  # nothing to write: out_data may be NULL
    # n = 0: nothing is launched, nothing is written
    some = _StrCol(dev, m.alignment_grid_column()[:50])
    empty_idx = np.zeros(0, dtype=np.int64)
    lens, payload = _gather_strings(dev, flags, some, empty_idx)
    assert lens.tolist() == [] and payload == b""
    out = _out(dev, 0, torch.uint8)
    hs.check(dev.lib.hs_gather_str_lens(dev.stream, C.byref(some.hs), some.n, None, 0, out.data_ptr(), flags.data_ptr()))
    assert _canary_intact(out, 0) and _flags(flags) == 0


@pytest.mark.parametrize("fixed", [False, True])
def test_gather_strings_index_guard(dev, flags, fixed):
    """Rows -1 and src_rows gather the empty string and raise HS_FLAG_BAD_PROGRAM; lens, offs and payload are views
    into larger buffers, so an unchecked read would stay inside them (and gather one 0x77 byte instead)."""
    from minispark_amd import hipspark as hs

    rows = m.fixed_width_column(5, 120) if fixed else m.alignment_grid_column()[:120]
    col = _StrCol(dev, rows, fixed_len=5 if fixed else -1, guarded=True)
    idx = m.guarded_indices(400, len(rows))
    assert _assert_gathered(dev, flags, col, idx)
    assert _flags(flags) == hs.FLAG_BAD_PROGRAM


# ---- string concatenation: hs_concat_lens + hs_str_offsets + hs_concat_bytes --------------------------------------
def _concat_parts(dev, parts, specs):
    """hs_col array for the parts, built the way Device.concat_strings builds it.  -> (array, tensors kept alive)"""
    import torch

    from minispark_amd import hipspark as hs

    arr, keep = (hs.hs_col * max(len(parts), 1))(), []
    for i, (part, spec) in enumerate(zip(parts, specs)):
        if spec[0] == "lit":
            lit = dev.to_device(np.frombuffer(part or b"\0", dtype=np.uint8), torch.uint8)
            keep.append(lit)
            c = hs.hs_col()
            c.kind = -1
            c.fixed_len = len(part)
            c.data = lit.data_ptr()
            arr[i] = c
        else:
            col = _StrCol(dev, part, fixed_len=spec[1] if spec[0] == "fixed" else 0 if spec[0] == "empty" else -1)
            keep.append(col)
            arr[i] = col.hs
    return arr, keep


@pytest.mark.parametrize("n", m.CONCAT_SIZES)
@pytest.mark.parametrize("name", list(m.CONCAT_CASES))
def test_concat(dev, flags, name, n):
    """1, 2, 3 and 8 parts of every kind; rows of exactly 255 bytes stay whole, longer ones keep their first 255 bytes and
    raise HS_FLAG_STR_TOO_LONG, and the row behind such a row starts with its own first byte."""
    import torch

    from minispark_amd import hipspark as hs

    parts, specs, special = m.concat_inputs(name, n)
    arr, keep = _concat_parts(dev, parts, specs)
    want_lens, want_bytes, too_long = m.concat(parts, n)
    out_lens = _out(dev, n, torch.uint8)
    hs.check(dev.lib.hs_concat_lens(dev.stream, arr, len(parts), n, out_lens.data_ptr(), flags.data_ptr()))
    assert _canary_intact(out_lens, n)
    assert np.array_equal(out_lens[:n].cpu().numpy(), want_lens)
    assert _flags(flags) == (hs.FLAG_STR_TOO_LONG if too_long else 0)
    offs, total = _offsets(dev, out_lens, n)
    assert total == len(want_bytes)
    # 4096 canary bytes: a row written without the clamp (up to 2040 bytes) would still end inside the buffer
    out_data = _out(dev, total, torch.uint8, guard=4096)
    hs.check(dev.lib.hs_concat_bytes(dev.stream, arr, len(parts), n, offs.data_ptr(), out_data.data_ptr()))
    assert _canary_intact(out_data, total)
    got = out_data[:total].cpu().numpy().tobytes()
    starts = m.exclusive_scan(want_lens)
    for row, t in special.items():  # named first, so that a failure says which row
        lo, hi = int(starts[row]), int(starts[min(row + 2, n)])
        assert got[lo:hi] == want_bytes[lo:hi], f"row {row} of total {t} and the row behind it"
    assert got == want_bytes
    assert too_long == any(t > 255 for t in special.values())
    del keep


def test_concat_refuses_nine_parts(dev, flags):
    import torch

    parts = [[b"ab"] * 4] * 9
    arr, keep = _concat_parts(dev, parts, [("var",)] * 9)
    out_lens = _out(dev, 4, torch.uint8)
    assert dev.lib.hs_concat_lens(dev.stream, arr, 9, 4, out_lens.data_ptr(), flags.data_ptr()) == E_LIMIT
    offs = dev.to_device(np.arange(5, dtype=np.int64) * 18, torch.int64)
    out_data = _out(dev, 72, torch.uint8)
    assert dev.lib.hs_concat_bytes(dev.stream, arr, 9, 4, offs.data_ptr(), out_data.data_ptr()) == E_LIMIT
    assert _canary_intact(out_lens, 0) and _canary_intact(out_data, 0) and _flags(flags) == 0
    del keep


# ---- hs_dict_combine ----------------------------------------------------------------------------------------------
def _dict_args(code_tensors, strides):
    ptrs = (C.c_void_p * len(code_tensors))(*[t.data_ptr() for t in code_tensors])
    strd = (C.c_int32 * len(strides))(*strides)
    return ptrs, strd


@pytest.mark.parametrize("n", m.DICT_ROWS)
@pytest.mark.parametrize("sizes", m.DICT_SIZES)
def test_dict_combine(dev, sizes, n):
    """16 rows per lane from 16-byte loads: whole groups, ragged tails of 1 and 15 rows, and not one byte written past n."""
    import torch

    from minispark_amd import hipspark as hs

    strides = m.dict_strides(sizes)
    codes = m.dict_codes(sizes, n)
    d_codes = [_up_whole(dev, c) for c in codes]
    out = _out(dev, n, torch.uint8)
    ptrs, strd = _dict_args(d_codes, strides)
    hs.check(dev.lib.hs_dict_combine(dev.stream, len(sizes), ptrs, strd, n, out.data_ptr()))
    assert np.array_equal(out[:n].cpu().numpy(), m.dict_combine(codes, strides))
    assert _canary_intact(out, n)


def test_dict_combine_above_the_grid_cap(dev):
    """More 16-row groups than 8192 blocks x 256 lanes: the grid-stride loop runs, and the last group is ragged."""
    import torch

    from minispark_amd import hipspark as hs

    n, sizes = m.DICT_ABOVE_CAP, (16, 16)
    strides = m.dict_strides(sizes)
    d_codes = []
    for sz in sizes:
        t = dev.empty(n, torch.uint8)
        t.random_(0, sz)
        d_codes.append(t)
    out = _out(dev, n, torch.uint8)
    ptrs, strd = _dict_args(d_codes, strides)
    hs.check(dev.lib.hs_dict_combine(dev.stream, 2, ptrs, strd, n, out.data_ptr()))
    want = d_codes[0] * strides[0] + d_codes[1] * strides[1]  # uint8 arithmetic wraps: the low byte
    assert want.dtype == torch.uint8 and torch.equal(out[:n], want)
    assert int(want.max().item()) == 255 and _canary_intact(out, n)


def test_dict_combine_refuses_bad_arguments(dev):
    import torch

    n = 100
    d_codes = [dev.to_device(c, torch.uint8) for c in m.dict_codes((2, 2, 2, 2, 2), n + 1)]
    out = _out(dev, n + 1, torch.uint8)
    ptrs, strd = _dict_args(d_codes, [16, 8, 4, 2, 1])
    assert dev.lib.hs_dict_combine(dev.stream, 0, ptrs, strd, n, out.data_ptr()) == E_ARG
    assert dev.lib.hs_dict_combine(dev.stream, 5, ptrs, strd, n, out.data_ptr()) == E_ARG
    assert dev.lib.hs_dict_combine(dev.stream, 2, ptrs, strd, n, out[1:].data_ptr()) == E_ARG  # unaligned output
    ptrs, strd = _dict_args([d_codes[0], d_codes[1][1:]], [2, 1])
    assert dev.lib.hs_dict_combine(dev.stream, 2, ptrs, strd, n, out.data_ptr()) == E_ARG  # unaligned codes
    assert _canary_intact(out, 0)


# ---- hs_quantise, hs_quantise_many --------------------------------------------------------------------------------
def _quantise(dev, flags, kind, values, cap=None):
    """One hs_quantise call into a canaried buffer -> (result bits as uint32 over [0, n_eff), flags word)."""
    import torch

    from minispark_amd import hipspark as hs

    n = len(values)
    d_src = _up(dev, values)
    d_cap = _count(dev, cap)
    out = _out(dev, n, torch.int32)
    flags.zero_()
    hs.check(dev.lib.hs_quantise(dev.stream, d_src.data_ptr(), hs.F64 if kind == "f64" else hs.I64, n, _ptr(d_cap),
                                 out.data_ptr(), flags.data_ptr()))
    n_eff = n if cap is None else min(n, cap)
    assert _canary_intact(out, n_eff)
    return _host(out[:n_eff], np.uint32), _flags(flags)


def _quantise_model(kind, values):
    from minispark_amd import hipspark as hs

    if kind == "f64":
        want, over = m.quantise_f64(values)
        return want.view(np.uint32), hs.FLAG_FLT_OVERFLOW if over else 0
    want, over = m.quantise_i64(values)
    return want.view(np.uint32), hs.FLAG_INT_OVERFLOW if over else 0


def test_quantise_f64_rounds_like_struct_pack(dev, flags):
    """f64 -> f32 as numpy / struct.pack('<f') do it (reference io.py:94): round to nearest even, subnormal results kept,
    the largest finite value and its neighbours, +-inf and NaN without a flag."""
    from minispark_amd import hipspark as hs

    x = m.quantise_f64_inputs()
    want, want_flags = _quantise_model("f64", x)
    got, got_flags = _quantise(dev, flags, "f64", x)
    differ = np.nonzero(got != want)[0]
    assert differ.size == 0, [(float(x[i]).hex(), hex(int(got[i])), hex(int(want[i]))) for i in differ[:8]]
    assert got_flags == want_flags == hs.FLAG_FLT_OVERFLOW
    # the flag row by row, on the rows where it could go either way: raised exactly where the model says
    edge = np.nonzero((np.abs(x) >= 2.0**127) | ~np.isfinite(x))[0]
    assert np.isinf(x[edge]).sum() == 2 and np.isnan(x[edge]).sum() == 1
    for i in edge.tolist():
        w, wf = _quantise_model("f64", x[i: i + 1])
        g, gf = _quantise(dev, flags, "f64", x[i: i + 1])
        assert (int(g[0]), gf) == (int(w[0]), wf), float(x[i]).hex()
    # and not otherwise: everything that fits, +-inf and NaN included, in one call
    fits = x[~(np.isinf(m.quantise_f64(x)[0]) & np.isfinite(x))]
    got, got_flags = _quantise(dev, flags, "f64", fits)
    assert np.array_equal(got, _quantise_model("f64", fits)[0]) and got_flags == 0


def test_quantise_i64_checks_the_int32_range(dev, flags):
    x = m.quantise_i64_inputs()
    want, want_flags = _quantise_model("i64", x)
    got, got_flags = _quantise(dev, flags, "i64", x)
    assert np.array_equal(got, want) and got_flags == want_flags != 0
    for i in range(len(x)):
        g, gf = _quantise(dev, flags, "i64", x[i: i + 1])
        w, wf = _quantise_model("i64", x[i: i + 1])
        assert (int(g[0]), gf) == (int(w[0]), wf), int(x[i])


@pytest.mark.parametrize("n", m.QUANT_MANY_ROWS)
def test_quantise_respects_the_device_count(dev, flags, n):
    for kind, values in m.quantise_many_inputs(2, n):
        for cap in m.n_dev_values(n):
            n_eff = n if cap is None else min(n, cap)
            want, want_flags = _quantise_model(kind, values[:n_eff])
            got, got_flags = _quantise(dev, flags, kind, values, cap)  # (asserts the canary from n_eff on)
            assert np.array_equal(got, want) and got_flags == want_flags, (kind, cap)


@pytest.mark.parametrize("n", m.QUANT_MANY_ROWS)
@pytest.mark.parametrize("n_cols", m.QUANT_MANY_COLS)
def test_quantise_many(dev, flags, n_cols, n):
    """Up to 16 mixed-kind columns in one launch: each equal to hs_quantise of that column and to the model; a device
    count - 0 included, where the kernel must not divide by it - leaves the rows behind it and the flags alone."""
    import torch

    from minispark_amd import hipspark as hs

    cols = m.quantise_many_inputs(n_cols, n)
    d_srcs = [_up(dev, v) for _, v in cols]
    kinds = (C.c_int32 * n_cols)(*[hs.F64 if k == "f64" else hs.I64 for k, _ in cols])
    srcs = (C.c_void_p * n_cols)(*[t.data_ptr() for t in d_srcs])
    single = [_quantise(dev, flags, k, v)[0] for k, v in cols]
    for cap in [None, 0, 1, n - 1, n + 7]:
        n_eff = n if cap is None else min(n, cap)
        d_cap = _count(dev, cap)
        outs = [_out(dev, n, torch.int32) for _ in cols]
        dsts = (C.c_void_p * n_cols)(*[t.data_ptr() for t in outs])
        flags.zero_()
        hs.check(dev.lib.hs_quantise_many(dev.stream, n_cols, srcs, kinds, n, _ptr(d_cap), dsts, flags.data_ptr()))
        want_flags = 0
        for c, (kind, values) in enumerate(cols):
            want, f = _quantise_model(kind, values[:n_eff])
            want_flags |= f
            got = _host(outs[c][:n_eff], np.uint32)
            assert np.array_equal(got, want) and np.array_equal(got, single[c][:n_eff]), (c, kind, cap)
            assert _canary_intact(outs[c], n_eff), (c, kind, cap)
        assert _flags(flags) == want_flags, cap


def test_quantise_many_refuses_seventeen_columns(dev, flags):
    import torch

    from minispark_amd import hipspark as hs

    d_src = dev.to_device(np.arange(8, dtype=np.int64), torch.int64)
    out = _out(dev, 8, torch.int32)
    kinds = (C.c_int32 * 17)(*[hs.I64] * 17)
    srcs = (C.c_void_p * 17)(*[d_src.data_ptr()] * 17)
    dsts = (C.c_void_p * 17)(*[out.data_ptr()] * 17)
    assert dev.lib.hs_quantise_many(dev.stream, 17, srcs, kinds, 8, None, dsts, flags.data_ptr()) == E_ARG
    assert _canary_intact(out, 0) and _flags(flags) == 0


# ---- hs_exclusive_scan_i64 ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_input(dev):
    """The values, their device copy and their scan, made once for every size (each size is a prefix)."""
    import torch

    values = m.scan_values()
    return values, dev.to_device(values, torch.int64), m.exclusive_scan(values)


@pytest.mark.parametrize("n", m.SCAN_SIZES)
def test_exclusive_scan_i64(dev, scan_input, n):
    """Tiles of 2048 elements, 2048 tile sums per k_scan_tiles round with a carry between rounds; sums pass 2^53, so
    anything but int64 arithmetic shows."""
    import torch

    from minispark_amd import hipspark as hs

    values, d_values, scanned = scan_input
    start = _out(dev, n + 1, torch.int64)
    ws = dev.workspace(dev.lib.hs_scan_ws_bytes(n))
    hs.check(dev.lib.hs_exclusive_scan_i64(dev.stream, d_values.data_ptr(), n, start.data_ptr(), ws.data_ptr()))
    assert np.array_equal(start[: n + 1].cpu().numpy(), scanned[: n + 1])  # start[n] is the total
    assert _canary_intact(start, n + 1)
    if n >= m.SCAN_ROUND - 1:
        assert int(scanned[n]) > 2**53


def test_exclusive_scan_i64_of_zeros(dev):
    import torch

    from minispark_amd import hipspark as hs

    n = 5000
    d_values = dev.to_device(np.zeros(n, dtype=np.int64), torch.int64)
    start = _out(dev, n + 1, torch.int64)
    ws = dev.workspace(dev.lib.hs_scan_ws_bytes(n))
    hs.check(dev.lib.hs_exclusive_scan_i64(dev.stream, d_values.data_ptr(), n, start.data_ptr(), ws.data_ptr()))
    assert not start[: n + 1].any().item() and _canary_intact(start, n + 1)


# ---- hs_lower_bound_i64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "one", "runs", "wide"])
def test_lower_bound_i64(dev, name):
    import torch

    from minispark_amd import hipspark as hs

    lst = m.lower_bound_lists()[name]
    q = m.lower_bound_queries(lst)
    d_list = dev.to_device(lst, torch.int64)
    d_q = dev.to_device(q, torch.int64)
    for cap in [None, len(lst) + 7] + m.lower_bound_caps(lst):
        n_eff = len(lst) if cap is None else min(len(lst), cap)
        d_cap = _count(dev, cap)
        out = _out(dev, len(q), torch.int64)
        hs.check(dev.lib.hs_lower_bound_i64(dev.stream, d_list.data_ptr(), len(lst), _ptr(d_cap), d_q.data_ptr(), len(q),
                                            out.data_ptr()))
        assert np.array_equal(out[: len(q)].cpu().numpy(), m.lower_bound(lst[:n_eff], q)), cap
        assert _canary_intact(out, len(q)), cap
    out = _out(dev, 0, torch.int64)
    hs.check(dev.lib.hs_lower_bound_i64(dev.stream, d_list.data_ptr(), len(lst), None, d_q.data_ptr(), 0, out.data_ptr()))
    assert _canary_intact(out, 0)  # no queries: nothing written


# ---- hs_expand_by_bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(m.expand_cases()))
def test_expand_by_bounds(dev, name):
    """Empty segments at the front, inside (two in a row) and at the end; one segment owning everything; more rows than
    4096 blocks x 256 lanes."""
    import torch

    from minispark_amd import hipspark as hs

    bounds, values, n = m.expand_cases()[name]
    d_bounds, d_values = dev.to_device(bounds, torch.int64), dev.to_device(values, torch.int64)
    out = _out(dev, n, torch.int64)
    hs.check(dev.lib.hs_expand_by_bounds(dev.stream, d_bounds.data_ptr(), d_values.data_ptr(), len(values), n, out.data_ptr()))
    assert np.array_equal(out[:n].cpu().numpy(), m.expand_by_bounds(bounds, values, n))
    assert _canary_intact(out, n)


def test_expand_by_bounds_refuses_no_segments(dev):
    import torch

    d_bounds = dev.to_device(np.array([0], dtype=np.int64), torch.int64)
    d_values = dev.to_device(np.array([7], dtype=np.int64), torch.int64)
    out = _out(dev, 4, torch.int64)
    assert dev.lib.hs_expand_by_bounds(dev.stream, d_bounds.data_ptr(), d_values.data_ptr(), 0, 4, out.data_ptr()) == E_ARG
    assert _canary_intact(out, 0)


# ---- hs_remap_u8 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", m.REMAP_SIZES)
@pytest.mark.parametrize("lut_name", ["permutation", "constant"])
def test_remap_u8(dev, lut_name, n):
    import torch

    from minispark_amd import hipspark as hs

    lut = m.remap_luts()[lut_name]
    codes = m.remap_codes(n)
    d_lut, d_codes = dev.to_device(lut, torch.uint8), _up_whole(dev, codes)
    out = _out(dev, n, torch.uint8)
    hs.check(dev.lib.hs_remap_u8(dev.stream, d_codes.data_ptr(), n, d_lut.data_ptr(), out.data_ptr()))
    assert np.array_equal(out[:n].cpu().numpy(), m.remap(codes, lut))
    assert _canary_intact(out, n)


# ---- hs_minmax_i32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placing", m.MINMAX_PLACINGS)
@pytest.mark.parametrize("n", m.MINMAX_SIZES)
def test_minmax_i32(dev, n, placing):
    """16-byte loads that reach past n: the elements behind n hold values below and above every real one, written through
    the un-narrowed tensor, so a load that forgot its `< n` guard changes the answer."""
    import torch

    from minispark_amd import hipspark as hs

    x = m.minmax_values(n, placing)
    whole = dev.empty(n + GUARD, torch.int32)
    whole[n:] = torch.tensor(m.MINMAX_SLACK * (GUARD // 2), dtype=torch.int32)
    whole[:n] = torch.from_numpy(x)
    out = _out(dev, 2, torch.int32)
    hs.check(dev.lib.hs_minmax_i32(dev.stream, whole.data_ptr(), n, out.data_ptr()))
    assert tuple(out[:2].tolist()) == m.minmax(x)
    assert _canary_intact(out, 2)


def test_minmax_i32_refuses_an_unaligned_pointer(dev):
    import torch

    whole = dev.to_device(np.arange(40, dtype=np.int32), torch.int32)
    out = _out(dev, 2, torch.int32)
    assert dev.lib.hs_minmax_i32(dev.stream, whole[1:].data_ptr(), 8, out.data_ptr()) == E_ARG
    assert _canary_intact(out, 0)
