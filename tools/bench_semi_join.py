"""LEFT SEMI / LEFT ANTI join microbenchmark (hs_keyset_build / hs_keyset_probe), HIP events on the launch
stream, median and min - max of --reps runs after warm-up.  --build INTEGER keys (every key of the range about once) against
--probe keys drawn from the same range, over
  (dense)  a key range of --build slots
  (spread) a key range of 32 x --build slots
Every case is timed next to the only form the engine had before the key set, on the same arrays: hs_join_dense_build +
hs_join_dense_count (the CSR over key slots, then the count pass).  The two forms alternate inside every repetition, so a
busy neighbour slows both.  The probe's mask is checked against torch.isin once per case.
--sweep times the build alone at HIPSPARK_KEYSET_L = 16 .. 19 and several HIPSPARK_KEYSET_CHUNK, one child process per
setting (the knobs are read once per process).  --e2e runs `orders LEFT SEMI JOIN lineitem` on synthetic tables of that scale
factor through the engine (wall time of collect_columns, which ends in the result's read-back).
Usage: python tools/bench_semi_join.py [--build 16M] [--probe 64M] [--reps 9] [--sweep] [--e2e 10] [--out FILE]"""
from __future__ import annotations

import argparse
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def size(text: str) -> int:
    return int(float(text[:-1]) * (1 << 20)) if text[-1] in "Mm" else int(text)


def event_ms(fn) -> float:
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(ts: list[float]) -> str:
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:8.3f} ms ({ts[0]:.3f} - {ts[-1]:.3f})"


def make_keys(n_build: int, n_probe: int, slots: int, seed: int):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    key_min = -(slots // 3)
    build = (torch.randint(0, slots, (n_build,), device="cuda", generator=g, dtype=torch.int64) + key_min).to(torch.int32)
    probe = (torch.randint(-slots // 8, slots + slots // 8, (n_probe,), device="cuda", generator=g, dtype=torch.int64) + key_min)
    return build, probe.to(torch.int32), key_min


class Forms:
    """the key set and the dense CSR over one pair of key arrays"""

    def __init__(self, build, probe, key_min: int, slots: int) -> None:
        import torch

        from minispark_amd import hipspark as hs

        self.hs, self.lib = hs, hs.load_library()
        lib = self.lib
        self.build, self.probe, self.key_min, self.slots = build, probe, key_min, slots
        nb, npr = build.numel(), probe.numel()
        u8 = lambda nbytes: torch.empty(int(nbytes) + 256, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.stream = torch.cuda.current_stream().cuda_stream
        self.flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.bitmap, self.ks_ws, self.mask = u8(lib.hs_keyset_bitmap_bytes(slots)), u8(lib.hs_keyset_ws_bytes(nb, slots)), u8(npr)
        self.words, self.rows, self.list_count = u8(slots * 4), u8(nb * 4), u8(nb * 4)
        self.jd_ws, self.counts, self.aux = u8(lib.hs_join_dense_ws_bytes(nb, slots)), u8(npr * 8), u8(lib.hs_join_dense_aux_bytes(npr))

    def keyset_build(self) -> None:
        b = self.build
        self.hs.check(self.lib.hs_keyset_build(self.stream, b.data_ptr(), b.numel(), self.key_min, self.slots, self.bitmap.data_ptr(),
                                               self.ks_ws.data_ptr(), self.flags.data_ptr()), "hs_keyset_build")

    def keyset_probe(self) -> None:
        p = self.probe
        self.hs.check(self.lib.hs_keyset_probe(self.stream, p.data_ptr(), p.numel(), self.key_min, self.slots, self.bitmap.data_ptr(),
                                               0, self.mask.data_ptr()), "hs_keyset_probe")

    def dense_build(self) -> None:
        b = self.build
        self.hs.check(self.lib.hs_join_dense_build(self.stream, b.data_ptr(), b.numel(), self.key_min, self.slots, self.words.data_ptr(),
                                                   self.rows.data_ptr(), self.list_count.data_ptr(), self.jd_ws.data_ptr(),
                                                   self.flags.data_ptr()), "hs_join_dense_build")

    def dense_count(self) -> None:
        p = self.probe
        self.hs.check(self.lib.hs_join_dense_count(self.stream, p.data_ptr(), p.numel(), self.key_min, self.slots, self.words.data_ptr(),
                                                   self.rows.data_ptr(), self.list_count.data_ptr(), self.counts.data_ptr(),
                                                   self.aux.data_ptr()), "hs_join_dense_count")


def micro(a, lines: list[str]) -> None:
    import torch

    nb, npr = size(a.build), size(a.probe)
    for name, slots in (("dense", nb), ("spread", 32 * nb)):
        build, probe, key_min = make_keys(nb, npr, slots, 25)
        f = Forms(build, probe, key_min, slots)
        steps = [("hs_keyset_build", f.keyset_build, nb), ("hs_keyset_probe", f.keyset_probe, npr),
                 ("hs_join_dense_build", f.dense_build, nb), ("hs_join_dense_count", f.dense_count, npr)]
        for _, fn, _ in steps:  # warm-up: code objects, the attributes a kernel asks for once
            fn()
            fn()
        torch.cuda.synchronize()
        times: dict[str, list[float]] = {n: [] for n, _, _ in steps}
        for _ in range(a.reps):  # the forms alternate inside a repetition
            for n, fn, _ in steps:
                times[n].append(event_ms(fn))
        assert int(f.flags[0].item()) == 0, "a build flagged a key outside the declared range"
        lines.append(f"({name}) {nb} build keys over {slots} slots (key_min {key_min}) x {npr} probe keys")
        for n, _, keys in steps:
            md = sorted(times[n])[len(times[n]) // 2]
            lines.append(f"    {n:22s} {spread(times[n])}   {keys / md / 1e6:8.2f} G keys/s")
        for part in ("build", "count"):
            new, old = times["hs_keyset_" + ("build" if part == "build" else "probe")], times["hs_join_dense_" + part]
            verdict = "below" if max(new) < min(old) else "overlaps" if min(new) <= max(old) else "ABOVE"
            lines.append(f"    key set {'build' if part == 'build' else 'probe'} range {verdict} the dense form's {part} range "
                         f"(median ratio {sorted(old)[len(old) // 2] / sorted(new)[len(new) // 2]:.2f}x)")
        want = torch.isin(probe, build)
        got = f.mask[:npr].to(torch.bool)
        dense = f.counts[: npr * 8].view(torch.int64) != 0
        lines.append(f"    check: mask == isin(probe, build): {bool(torch.equal(got, want))}; dense counts agree: "
                     f"{bool(torch.equal(dense, want))}; members {int(want.sum())}")
        del f, build, probe


def sweep_child(a) -> None:
    """one (L, chunk) setting, read from the environment by the library: build times over both ranges -> one line"""
    import torch

    nb = size(a.build)
    out = []
    for slots in (nb, 32 * nb):
        build, probe, key_min = make_keys(nb, 1024, slots, 25)
        f = Forms(build, probe, key_min, slots)
        f.keyset_build()
        f.keyset_build()
        torch.cuda.synchronize()
        out.append(spread([event_ms(f.keyset_build) for _ in range(a.reps)]))
        del f
    print(f"SWEEP L={os.environ.get('HIPSPARK_KEYSET_L', 'default')} chunk={os.environ.get('HIPSPARK_KEYSET_CHUNK', 'default'):>8s}   "
          f"dense {out[0]}   spread {out[1]}", flush=True)


def sweep(a, lines: list[str]) -> None:
    lines.append(f"hs_keyset_build alone, {size(a.build)} keys, per HIPSPARK_KEYSET_L / HIPSPARK_KEYSET_CHUNK (one process each):")
    for L in (16, 17, 18, 19):
        for chunk in (16384, 65536, 262144):
            env = dict(os.environ, HIPSPARK_KEYSET_L=str(L), HIPSPARK_KEYSET_CHUNK=str(chunk))
            proc = subprocess.run([sys.executable, __file__, "--sweep-child", "--build", a.build, "--reps", str(a.reps)], env=env,
                                  capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:
                raise SystemExit(f"sweep child L={L} chunk={chunk} failed:\n{proc.stdout[-1000:]}{proc.stderr[-2000:]}")
            lines.extend("    " + ln[6:] for ln in proc.stdout.splitlines() if ln.startswith("SWEEP "))


def end_to_end(a, lines: list[str]) -> None:
    import tempfile

    from minispark_amd import synth, workloads
    from minispark_amd.execution import HipExecutionEngine

    n_li = synth.lineitem_rows(a.e2e)
    n_ord = synth.orders_rows(n_li)
    with tempfile.TemporaryDirectory() as tmp, HipExecutionEngine(device=0) as engine:
        li_path, ord_path = Path(tmp) / "lineitem.bin", Path(tmp) / "orders.bin"
        engine.attach_device_table(li_path, synth.make_lineitem(engine.dev, li_path, n_li, with_orderkey=True))
        engine.attach_device_table(ord_path, synth.make_orders(engine.dev, ord_path, n_ord))
        api = workloads.engine_api(engine)
        C = api.Col
        on = (C("o_orderkey") == C("l_orderkey")) & (C("l_quantity") > 45)
        for how in ("left_semi", "left_anti"):
            frame = api.DataFrame().table(str(ord_path)).join(api.DataFrame().table(str(li_path)), on=on, how=how)
            ts, rows = [], 0
            for i in range(a.reps + 1):
                t0 = time.perf_counter()
                cols = frame.collect_columns()
                ts.append((time.perf_counter() - t0) * 1e3)
                rows = len(next(iter(cols.values())))
            lines.append(f"(e2e) orders {how} lineitem ON o_orderkey = l_orderkey AND l_quantity > 45, synthetic sf={a.e2e:g}: "
                         f"{n_ord} orders x {n_li} lines -> {rows} rows; wall {spread(ts[1:])} after one warm-up run; "
                         f"path {engine.dev.last_semi_join}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="16M")
    ap.add_argument("--probe", default="64M")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-child", action="store_true")
    ap.add_argument("--e2e", type=float, default=0.0)
    ap.add_argument("--no-micro", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.sweep_child:
        sweep_child(a)
        return
    import torch

    lines = [f"tools/bench_semi_join.py --build {a.build} --probe {a.probe} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, host "
             f"{socket.gethostname()}, torch {torch.__version__}]",
             "events on the launch stream; median (min - max) ms, keys/s at the median"]
    if not a.no_micro:
        micro(a, lines)
    if a.sweep:
        sweep(a, lines)
    if a.e2e:
        end_to_end(a, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
