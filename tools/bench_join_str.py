"""STRING-key join microbenchmark: the LDS-assembled hash windows (hs_join_hash_str_*) against the global-memory table
(hs_join_build / count / fill), 16 Mi unique 12-byte build keys x 64 Mi probe rows (every probe row matches once), timed with
HIP events on the launch stream (median of 5).  Writes the report to stdout and, with --out, to a file.
Usage: python tools/bench_join_str.py [--build 16M] [--probe 64M] [--out profiles/r05_join_str_64M.txt]"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402

PEAK = 8000.0  # GB/s


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def keys12(values: torch.Tensor) -> torch.Tensor:
    """[n] int64 -> [n * 12 + 16] uint8: 'K' + the value in 11 decimal digits per row (a fixed-width STRING column)."""
    out = torch.empty(values.numel(), 12, dtype=torch.uint8, device="cuda")
    out[:, 0] = ord("K")
    x = values.clone()
    for j in range(11, 0, -1):
        out[:, j] = (48 + x % 10).to(torch.uint8)
        x //= 10
    return torch.cat([out.reshape(-1), torch.zeros(16, dtype=torch.uint8, device="cuda")])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", type=float, default=16 * 2**20)
    ap.add_argument("--probe", type=float, default=64 * 2**20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nb, np_ = int(a.build), int(a.probe)
    lib = hs.load_library()
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    bvals = torch.randperm(nb, device="cuda", generator=g)
    pvals = torch.randint(0, nb, (np_,), device="cuda", generator=g)
    bdata, pdata = keys12(bvals), keys12(pvals)
    bk = hs.hs_col(hs.STR, 12, bdata.data_ptr(), None, None)
    pk = hs.hs_col(hs.STR, 12, pdata.data_ptr(), None, None)
    stream = torch.cuda.current_stream().cuda_stream
    e = lambda n, dt: torch.empty(n, dtype=dt, device="cuda")  # noqa: E731
    lines = [f"STRING-key join: {nb} unique 12-byte build keys x {np_} probe rows (each matches once); MI355X, HBM peak {PEAK:.0f} GB/s"]

    # the hash windows
    slots = int(lib.hs_join_hash_str_slots(nb))
    table, rows, lcount = e(slots, torch.int64), e(nb, torch.int32), e(nb, torch.int32)
    ws = e(int(lib.hs_join_hash_str_ws_bytes(nb)), torch.uint8)
    status, flags = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    counts, aux = e(np_ + 2, torch.int64), e(int(lib.hs_join_dense_aux_bytes(np_)) // 8 + 2, torch.int64)
    start, sws = e(np_ + 1, torch.int64), e(int(lib.hs_scan_ws_bytes(np_)), torch.uint8)
    left, right = e(np_, torch.int64), e(np_, torch.int64)

    def w_build():
        hs.check(lib.hs_join_hash_str_build(stream, C.byref(bk), nb, table.data_ptr(), rows.data_ptr(), lcount.data_ptr(), ws.data_ptr(),
                                            status.data_ptr(), flags.data_ptr()))

    def w_count():
        hs.check(lib.hs_join_hash_str_count(stream, C.byref(bk), C.byref(pk), np_, nb, table.data_ptr(), rows.data_ptr(),
                                            lcount.data_ptr(), counts.data_ptr(), aux.data_ptr()))

    def scan():
        hs.check(lib.hs_exclusive_scan_i64(stream, counts.data_ptr(), np_, start.data_ptr(), sws.data_ptr()))

    def w_fill():
        hs.check(lib.hs_join_dense_fill(stream, np_, rows.data_ptr(), aux.data_ptr(), start.data_ptr(), left.data_ptr(), right.data_ptr()))

    tb = timed(w_build)
    tc = timed(w_count)
    scan()
    tf = timed(w_fill)
    torch.cuda.synchronize()
    ok = int(status.item()) == 0 and int(flags.item()) == 0 and int(start[np_].item()) == np_
    ok = ok and bool(torch.equal(bvals[left.cpu().to(torch.int64).cuda()[:1_000_000]], pvals[:1_000_000]))
    # bytes every pass has to move at least: build = key bytes in + the table (8 B/slot) + rows / list counts out;
    # count = probe keys in + one 8-byte slot + one 12-byte build key compare + counts / aux out; fill = aux + offsets in, pairs out
    b_build = nb * 12 + slots * 8 + nb * 8
    b_count = np_ * (12 + 8 + 12 + 8 + 8)
    b_fill = np_ * (8 + 8 + 16)
    lines.append(f"windows   build        {tb:8.3f} ms  {nb / tb / 1e6:7.2f} G keys/s  {b_build / tb / 1e6 / PEAK * 100:5.1f}% of HBM peak"
                 f"  ({slots} slots; status {int(status.item())})")
    lines.append(f"windows   count        {tc:8.3f} ms  {b_count / tc / 1e6 / PEAK * 100:5.1f}% of HBM peak")
    lines.append(f"windows   fill         {tf:8.3f} ms  {b_fill / tf / 1e6 / PEAK * 100:5.1f}% of HBM peak")
    lines.append(f"windows   count + fill {tc + tf:8.3f} ms   (pairs checked against the keys: {'ok' if ok else 'MISMATCH'})")
    del table, rows, lcount, ws

    # the global-memory table
    cap = 16
    while cap < 2 * nb:
        cap *= 2
    tkeys, treps, sstart, grows = e(cap, torch.int64), e(cap, torch.int64), e(cap + 1, torch.int64), e(nb, torch.int64)
    gws = e(int(lib.hs_join_build_ws_bytes(nb, cap)), torch.uint8)

    def g_build():
        hs.check(lib.hs_join_build(stream, C.byref(bk), nb, cap, tkeys.data_ptr(), treps.data_ptr(), sstart.data_ptr(), grows.data_ptr(),
                                   gws.data_ptr(), flags.data_ptr()))

    def g_count():
        hs.check(lib.hs_join_count(stream, C.byref(bk), C.byref(pk), np_, cap, tkeys.data_ptr(), treps.data_ptr(), sstart.data_ptr(),
                                   counts.data_ptr()))

    def g_fill():
        hs.check(lib.hs_join_fill(stream, C.byref(bk), C.byref(pk), np_, cap, tkeys.data_ptr(), treps.data_ptr(), sstart.data_ptr(),
                                  grows.data_ptr(), start.data_ptr(), left.data_ptr(), right.data_ptr()))

    gb = timed(g_build)
    gc = timed(g_count)
    scan()
    gf = timed(g_fill)
    lines.append(f"global    build        {gb:8.3f} ms  {nb / gb / 1e6:7.2f} G keys/s")
    lines.append(f"global    count + fill {gc + gf:8.3f} ms  (count {gc:.3f}, fill {gf:.3f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
