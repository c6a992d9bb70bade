"""hs_join_hash_str_* (csrc/hs_radix.hip): the STRING-key join's hash windows assembled in LDS, per operator.  Pairs against a
numpy model of the reference's loop (tasks.py:201-240: probe row, then build row ascending), the documented hash bits
recomputed on the host, two keys of one fingerprint in one window, and a window with more keys than slots."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FNV_BASIS, FNV_PRIME = np.uint64(0xCBF29CE484222325), np.uint64(0x100000001B3)


def fnv1a(mat: np.ndarray, lens: np.ndarray | None = None) -> np.ndarray:
    """64-bit FNV-1a of every row of a uint8 matrix (the first lens[i] bytes of row i)."""
    h = np.full(mat.shape[0], FNV_BASIS, dtype=np.uint64)
    for j in range(mat.shape[1]):
        live = np.ones(mat.shape[0], bool) if lens is None else lens > j
        h2 = (h ^ mat[:, j].astype(np.uint64)) * FNV_PRIME
        h = np.where(live, h2, h)
    return h


def fmix64(x: np.ndarray) -> np.ndarray:
    """MurmurHash3's 64-bit finaliser (hs_mix64)."""
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def key_hash(mat: np.ndarray, lens: np.ndarray | None = None) -> np.ndarray:
    """The windows' hash m = fmix64(FNV-1a(key)) (include/hipspark.h, hs_join_hash_str_*)."""
    return fmix64(fnv1a(mat, lens))


def window_of(m: np.ndarray, windows: int) -> np.ndarray:  # the header's bits: (m >> 32) * windows >> 32
    return (((m >> np.uint64(32)) * np.uint64(windows)) >> np.uint64(32)).astype(np.int64)


def model_pairs(bcodes: np.ndarray, pcodes: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Pairs of equal codes ordered by probe row, then build row."""
    order = np.argsort(bcodes, kind="stable")
    sk = bcodes[order]
    lo, hi = np.searchsorted(sk, pcodes, "left"), np.searchsorted(sk, pcodes, "right")
    cnt = hi - lo
    right = np.repeat(np.arange(len(pcodes), dtype=np.int64), cnt)
    before = np.cumsum(cnt) - cnt
    idx = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(before, cnt) + np.repeat(lo, cnt)
    return order[idx].astype(np.int64), right


class DevStr:
    """A variable-length STRING column on the device (lens, offsets, payload) from a list of byte strings."""

    def __init__(self, values: list[bytes]) -> None:
        import torch

        from minispark_amd import hipspark as hs

        lens = np.array([len(v) for v in values], np.uint8)
        offs = np.zeros(len(values) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        data = np.frombuffer(b"".join(values) + b"\0" * 8, np.uint8)
        self.lens = torch.from_numpy(lens.copy()).cuda() if len(values) else torch.zeros(1, dtype=torch.uint8, device="cuda")
        self.offs = torch.from_numpy(offs).cuda()
        self.data = torch.from_numpy(data.copy()).cuda()
        self.n = len(values)
        self.col = hs.hs_col(hs.STR, -1, self.data.data_ptr(), self.lens.data_ptr(), self.offs.data_ptr())


class DevFixed:
    """A STRING column of one fixed width from a uint8 matrix [n, width]."""

    def __init__(self, mat: np.ndarray) -> None:
        import torch

        from minispark_amd import hipspark as hs

        self.data = torch.from_numpy(np.concatenate([mat.reshape(-1), np.zeros(16, np.uint8)])).cuda()
        self.n = mat.shape[0]
        self.col = hs.hs_col(hs.STR, mat.shape[1], self.data.data_ptr(), None, None)


def run_join(build, probe):
    """build + count + scan + hs_join_dense_fill -> (left, right, status, flags, table, slots)."""
    import torch

    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    nb, np_ = build.n, probe.n
    slots = int(lib.hs_join_hash_str_slots(nb))
    assert slots > 0
    dev = "cuda"
    table = torch.empty(slots, dtype=torch.int64, device=dev)
    rows = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    lcount = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.hs_join_hash_str_ws_bytes(nb)), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hs.check(lib.hs_join_hash_str_build(stream, C.byref(build.col), nb, table.data_ptr(), rows.data_ptr(), lcount.data_ptr(),
                                        ws.data_ptr(), status.data_ptr(), flags.data_ptr()), "hs_join_hash_str_build")
    counts = torch.empty(max(np_, 1) + 2, dtype=torch.int64, device=dev)
    aux = torch.empty(int(lib.hs_join_dense_aux_bytes(np_)) // 8 + 2, dtype=torch.int64, device=dev)
    hs.check(lib.hs_join_hash_str_count(stream, C.byref(build.col), C.byref(probe.col), np_, nb, table.data_ptr(), rows.data_ptr(),
                                        lcount.data_ptr(), counts.data_ptr(), aux.data_ptr()), "hs_join_hash_str_count")
    start = torch.empty(np_ + 1, dtype=torch.int64, device=dev)
    sws = torch.empty(int(lib.hs_scan_ws_bytes(max(np_, 1))), dtype=torch.uint8, device=dev)
    hs.check(lib.hs_exclusive_scan_i64(stream, counts.data_ptr(), np_, start.data_ptr(), sws.data_ptr()), "scan")
    n_out = int(start[np_].item())
    left = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
    right = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
    if n_out:
        hs.check(lib.hs_join_dense_fill(stream, np_, rows.data_ptr(), aux.data_ptr(), start.data_ptr(), left.data_ptr(),
                                        right.data_ptr()), "hs_join_dense_fill")
    torch.cuda.synchronize()
    return (left[:n_out].cpu().numpy(), right[:n_out].cpu().numpy(), int(status.item()), int(flags.item()),
            table.cpu().numpy().view(np.uint64), slots)


def _digits(v: np.ndarray, width: int, lead: int = ord("K")) -> np.ndarray:
    """[n, width] uint8: a letter, then v in decimal with leading zeros."""
    out = np.empty((len(v), width), np.uint8)
    out[:, 0] = lead
    x = v.astype(np.int64).copy()
    for j in range(width - 1, 0, -1):
        out[:, j] = ord("0") + x % 10
        x //= 10
    return out


@pytest.mark.parametrize("nb", [1, 5, 4099, 1 << 20, 20_000_000])
def test_pairs_match_the_model(nb):
    """Fixed 12-byte keys, duplicates on both sides, probes that miss; 20 M build rows use the 1024-slot windows."""
    rng = np.random.default_rng(nb)
    span = max(nb * 3 // 4, 1)
    bcodes = rng.integers(0, span, nb)
    np_ = min(max(3 * nb, 7), 24_000_000)
    pcodes = rng.integers(0, span + span // 3 + 1, np_)
    left, right, status, flags, table, slots = run_join(DevFixed(_digits(bcodes, 12)), DevFixed(_digits(pcodes, 12)))
    assert status == 0 and flags == 0
    want_l, want_r = model_pairs(bcodes, pcodes)
    assert np.array_equal(right, want_r) and np.array_equal(left, want_l)
    if nb == 4099:  # the documented bits: every build key's fingerprint sits in its window
        L = 512 if nb < 19_000_000 else 1024
        windows = slots // L
        m = key_hash(_digits(bcodes, 12))
        win, fp = window_of(m, windows), (m & np.uint64(0xFFFFFFFF))
        stored = (table & np.uint64(0xFFFFFFFF)).reshape(windows, L)
        used = (table >> np.uint64(32)).reshape(windows, L) != np.uint64(0xFFFFFFFF)
        for w, f in zip(win[:500], fp[:500]):
            assert np.any(used[w] & (stored[w] == f))


def test_keys_of_every_length_and_near_misses():
    """0 .. 40 bytes, the empty string, keys that differ only in their last byte, duplicates on both sides."""
    rng = np.random.default_rng(7)
    base = [bytes(rng.integers(97, 123, int(rng.integers(0, 41))).astype(np.uint8)) for _ in range(300)]
    base += [b"", b"a", b"ab", b"x" * 17, b"x" * 16 + b"y", b"x" * 40, b"x" * 39 + b"z"]
    base += [b[:-1] + bytes([b[-1] ^ 1]) for b in base if len(b) > 0][:100]
    base = list(dict.fromkeys(base))
    code = {k: i for i, k in enumerate(base)}
    build = [base[i] for i in rng.integers(0, len(base), 5000)]
    extra = [b"nomatch" + bytes([i]) for i in range(20)]
    probe = [base[i] for i in rng.integers(0, len(base), 9000)] + extra
    left, right, status, flags, _, _ = run_join(DevStr(build), DevStr(probe))
    assert status == 0 and flags == 0
    pc = np.array([code.get(k, -1 - i) for i, k in enumerate(probe)])
    want_l, want_r = model_pairs(np.array([code[k] for k in build]), pc)
    assert np.array_equal(right, want_r) and np.array_equal(left, want_l)


def _candidates(n: int, width: int = 8) -> np.ndarray:
    return _digits(np.arange(n), width, lead=ord("c"))


def test_a_fingerprint_collision_matches_only_itself():
    """Two different 8-byte keys of the same 32-bit fingerprint (brute force over 2^22 candidates); with a small build side
    every key lands in window 0: the two become two slots and each probe key finds only its own build row."""
    cand = _candidates(1 << 22)
    fp = key_hash(cand) & np.uint64(0xFFFFFFFF)
    order = np.argsort(fp, kind="stable")
    same = np.nonzero(fp[order][1:] == fp[order][:-1])[0]
    assert len(same) > 0
    a, b = cand[order[same[0]]], cand[order[same[0] + 1]]
    assert bytes(a) != bytes(b)
    build = [bytes(a), bytes(b), b"other"]
    probe = [bytes(b), bytes(a), b"other", bytes(a) + b"!", bytes(b)]
    left, right, status, flags, _, _ = run_join(DevStr(build), DevStr(probe))
    assert status == 0 and flags == 0
    assert right.tolist() == [0, 1, 2, 4] and left.tolist() == [1, 0, 2, 1]


def overflow_keys(n: int = 600) -> list[bytes]:
    """n distinct keys that all hash to window 0 of an n-row build side (more keys than the window's 512 slots)."""
    windows = (n * 7 // 4 + 511) >> 9
    cand = _candidates(1 << 16)
    win = window_of(key_hash(cand), windows)
    picked = cand[win == 0][:n]
    assert len(picked) == n
    return [bytes(r) for r in picked]


def test_a_window_with_more_keys_than_slots_reports_dict_full():
    keys = overflow_keys()
    _, _, status, flags, _, _ = run_join(DevStr(keys), DevStr(keys[:10]))
    from minispark_amd import hipspark as hs

    assert status == hs.FLAG_DICT_FULL and flags == 0


def test_unique_keys_of_consecutive_digits_do_not_crowd_a_window():
    """4 Mi unique keys that differ only in their trailing digits (FNV-1a's high bits alone crowded a few windows with such
    keys): no window overflows and every probe finds its one row."""
    nb = 1 << 22
    rng = np.random.default_rng(3)
    bcodes = rng.permutation(nb)
    pcodes = rng.integers(0, nb, 2 * nb)
    left, right, status, flags, _, _ = run_join(DevFixed(_digits(bcodes, 12)), DevFixed(_digits(pcodes, 12)))
    assert status == 0 and flags == 0
    want_l, want_r = model_pairs(bcodes, pcodes)
    assert np.array_equal(right, want_r) and np.array_equal(left, want_l)
