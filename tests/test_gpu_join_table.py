"""hs_join_table_plan / build / count / fill (csrc/hs_radix.hip) driven directly: every route of the general join through
the one table handle, pairs against the searchsorted model of the reference's loop (tasks.py:201-240: probe row, then build
row ascending), and the overflow ladder - plan again without the route whose window overflowed."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_join_str_windows import DevStr, model_pairs

pytestmark = pytest.mark.gpu

DENSE, HASH, HASH_STR, GLOBAL = 1, 2, 3, 4
ALL = 0x1E


class DevInts:
    """An INTEGER (or, with np.int64, TIMESTAMP) key column on the device, with the slack the four-keys-a-lane probes read."""

    def __init__(self, values: np.ndarray) -> None:
        import torch

        from minispark_amd import hipspark as hs

        self.data = torch.from_numpy(np.concatenate([values, np.zeros(16, values.dtype)])).cuda()
        self.n = len(values)
        self.col = hs.hs_col(hs.I32 if values.dtype == np.int32 else hs.I64, -1, self.data.data_ptr(), None, None)


def plan(build, probe, routes, key_range=(0, -1)):
    from minispark_amd import hipspark as hs

    t = hs.hs_join_table()
    hs.check(hs.load_library().hs_join_table_plan(C.byref(build.col), C.byref(probe.col), build.n, probe.n, key_range[0], key_range[1],
                                                  routes, C.byref(t)), "hs_join_table_plan")
    return t


def run(build, probe, routes, key_range=(0, -1)):
    """plan + build + count (+ scan + fill unless a window overflowed) -> (route, left, right, status, flags)."""
    import torch

    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    t = plan(build, probe, routes, key_range)
    assert t.route and routes & 1 << t.route
    dev, n_probe = "cuda", probe.n
    stream = torch.cuda.current_stream().cuda_stream
    table = torch.empty(t.table_bytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(t.ws_bytes, 256) + 64, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(max(n_probe, 1) + 2, dtype=torch.int64, device=dev)
    aux = torch.empty(int(lib.hs_join_dense_aux_bytes(n_probe)) // 8 + 2, dtype=torch.int64, device=dev)
    hs.check(lib.hs_join_table_build(stream, C.byref(t), C.byref(build.col), table.data_ptr(), ws.data_ptr(), status.data_ptr(),
                                     flags.data_ptr()), "hs_join_table_build")
    hs.check(lib.hs_join_table_count(stream, C.byref(t), C.byref(build.col), C.byref(probe.col), n_probe, table.data_ptr(),
                                     counts.data_ptr(), aux.data_ptr()), "hs_join_table_count")
    if int(status.item()) != 0:
        return t.route, None, None, int(status.item()), int(flags.item())
    start = torch.empty(n_probe + 1, dtype=torch.int64, device=dev)
    sws = torch.empty(int(lib.hs_scan_ws_bytes(max(n_probe, 1))) + 64, dtype=torch.uint8, device=dev)
    hs.check(lib.hs_exclusive_scan_i64(stream, counts.data_ptr(), n_probe, start.data_ptr(), sws.data_ptr()), "hs_exclusive_scan_i64")
    n_out = int(start[n_probe].item())
    left = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
    right = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
    hs.check(lib.hs_join_table_fill(stream, C.byref(t), C.byref(build.col), C.byref(probe.col), n_probe, table.data_ptr(),
                                    aux.data_ptr(), start.data_ptr(), left.data_ptr(), right.data_ptr()), "hs_join_table_fill")
    torch.cuda.synchronize()
    return t.route, left[:n_out].cpu().numpy(), right[:n_out].cpu().numpy(), 0, int(flags.item())


def test_every_route_gives_the_same_pairs_on_one_integer_input():
    """700 build rows with duplicates and one key many times, 5000 probe rows with misses: each route forced by the mask."""
    rng = np.random.default_rng(28)
    bkeys = rng.integers(-300, 300, 700).astype(np.int32)
    bkeys[rng.integers(0, 700, 40)] = bkeys[0]
    pkeys = rng.integers(-400, 400, 5000).astype(np.int32)
    build, probe = DevInts(bkeys), DevInts(pkeys)
    want_l, want_r = model_pairs(bkeys, pkeys)
    assert 0 < np.isin(pkeys, bkeys).sum() < 5000 and len(want_l) > np.isin(pkeys, bkeys).sum()  # misses, and keys with several partners
    key_range = (int(bkeys.min()), int(bkeys.max()))
    assert plan(build, probe, ALL, key_range).route == DENSE
    for route in (DENSE, HASH, GLOBAL):
        got_route, left, right, status, flags = run(build, probe, 1 << route, key_range)
        assert got_route == route and status == 0 and flags == 0
        assert np.array_equal(right, want_r) and np.array_equal(left, want_l), route
    assert plan(build, probe, 1 << HASH_STR, key_range).route == 0  # (INTEGER keys: the STRING windows do not hold them)
    # ... so the fourth route runs on the same keys as decimal strings
    sbuild, sprobe = DevStr([b"%d" % k for k in bkeys.tolist()]), DevStr([b"%d" % k for k in pkeys.tolist()])
    got_route, left, right, status, flags = run(sbuild, sprobe, 1 << HASH_STR)
    assert got_route == HASH_STR and status == 0 and flags == 0
    assert np.array_equal(right, want_r) and np.array_equal(left, want_l)


def test_one_build_row_against_five_probe_rows():
    build, probe = DevInts(np.array([7], np.int32)), DevInts(np.array([7, 3, 7, -7, 7], np.int32))
    for routes, want in ((ALL, DENSE), (ALL & ~(1 << DENSE), HASH), (1 << GLOBAL, GLOBAL)):
        route, left, right, status, flags = run(build, probe, routes, (7, 7))
        assert route == want and status == 0 and flags == 0
        assert left.tolist() == [0, 0, 0] and right.tolist() == [0, 2, 4]


def test_string_keys_through_the_windows_and_the_global_table():
    lwords = [b"apple", b"banana", b"a-long-key-beyond-seven-bytes", b"apple", b"", b"a-long-key-beyond-seven-byteS"]
    rwords = [b"", b"apple", b"cherry", b"a-long-key-beyond-seven-bytes", b"banana", b"apple"]
    build, probe = DevStr(lwords), DevStr(rwords)
    want = [(li, ri) for ri, w in enumerate(rwords) for li, v in enumerate(lwords) if v == w]
    for routes, want_route in ((ALL, HASH_STR), (ALL & ~(1 << HASH_STR), GLOBAL)):
        route, left, right, status, flags = run(build, probe, routes)
        assert route == want_route and status == 0 and flags == 0
        assert list(zip(left.tolist(), right.tolist())) == want


def test_i64_keys_plan_the_global_table():
    rng = np.random.default_rng(64)
    bkeys, pkeys = rng.integers(-50, 50, 300) * (1 << 33), rng.integers(-60, 60, 900) * (1 << 33)
    route, left, right, status, flags = run(DevInts(bkeys), DevInts(pkeys), ALL)
    assert route == GLOBAL and status == 0 and flags == 0
    want_l, want_r = model_pairs(bkeys, pkeys)
    assert np.array_equal(right, want_r) and np.array_equal(left, want_l)


def test_an_overflowing_window_reports_dict_full_and_the_next_plan_is_the_global_table():
    """The key set of test_a_hash_window_that_overflows_hands_the_join_to_the_global_table (tests/test_gpu_kernels.py)."""
    from minispark_amd import hipspark as hs

    def mix32(k):
        k = k.astype(np.uint64)
        h = (k * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
        return h ^ (h >> np.uint64(16))

    n_left = 4000
    windows = (n_left * 7 // 4 + 511) >> 9
    cand = np.arange(0, 4_000_000, dtype=np.int64)
    in_window_0 = cand[((mix32(cand) * np.uint64(windows)) >> np.uint64(32)) == 0]
    left = np.concatenate([in_window_0[:1100], cand[:n_left - 1100] + 5_000_000]).astype(np.int32)
    left[-1] = 2_000_000_000
    right = np.concatenate([left[::3], np.array([7, -9], dtype=np.int32)])
    build, probe = DevInts(left), DevInts(right)
    key_range = (int(left.min()), int(left.max()))
    routes = ALL
    route, _, _, status, flags = run(build, probe, routes, key_range)
    assert route == HASH and status == hs.FLAG_DICT_FULL and flags == 0
    routes &= ~(1 << route)
    route, got_l, got_r, status, flags = run(build, probe, routes, key_range)
    assert route == GLOBAL and status == 0 and flags == 0
    want_l, want_r = model_pairs(left, right)
    assert np.array_equal(got_r, want_r) and np.array_equal(got_l, want_l)
