"""What a conditional aggregate costs: bucketed sums in one scan (CASE WHEN) against the plain sum and against one scan per
bucket, GROUP BY l_returnflag over the synthetic lineitem, through HipExecutionEngine.

  (a)  SUM(l_extendedprice)                                                               price + key
  (a') the same behind WHERE l_discount >= 0.0 (keeps every row)                          price + discount + key
  (a2) SUM(l_extendedprice), SUM(l_extendedprice * l_discount)                            the same columns, two accumulators,
       one multiply where (b) has a compare and a select: what the second accumulator costs without a CASE
  (b)  SUM(CASE WHEN l_discount > 0.05 THEN l_extendedprice ELSE 0.0 END), SUM(l_extendedprice)   the same columns as (a')
  (c)  what a build without CASE offers: SUM(l_extendedprice) WHERE l_discount > 0.05, then the same WHERE l_discount <= 0.05
       - two scans, their times added

Per repeat every query runs once, in turn (drift of the box hits all of them alike).  Two clocks per query: `step` = a HIP
event pair on the launch stream around collect() (scan, merge, hand-over; the collect ends with the result on the host),
`kernel` = the scan kernel's own event pair.  Reported: median (min - max) over --reps, and (b)/(a), (b)/(a'), (b)/(a2),
(b)/(c) at the medians next to the spread of every query itself.
Usage: python tools/bench_case_when.py [--sf 100] [--reps 20] [--warmup 3] [--out FILE]"""
from __future__ import annotations

import argparse
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import synth  # noqa: E402
from minispark_amd.dataframe import DataFrame  # noqa: E402
from minispark_amd.execution import HipExecutionEngine  # noqa: E402
from minispark_amd.sql import Col, Functions as F  # noqa: E402


A1 = "a'"


def queries(engine, path: str) -> dict:
    def table():
        return DataFrame(engine).table(path)

    price, disc, key = Col("l_extendedprice"), Col("l_discount"), Col("l_returnflag")
    out = {
        "a": [table().group_by(key).agg(F.sum(price).alias("s"))],
        "a'": [table().filter(disc >= 0.0).group_by(key).agg(F.sum(price).alias("s"))],
        "a2": [table().group_by(key).agg(F.sum(price).alias("s"), F.sum(price * disc).alias("sd"))],
        "c": [table().filter(disc > 0.05).group_by(key).agg(F.sum(price).alias("s")),
              table().filter(disc <= 0.05).group_by(key).agg(F.sum(price).alias("s"))],
    }
    if hasattr(F, "when"):  # a library without CASE times (a), (a') and (c) only
        out["b"] = [table().group_by(key).agg(F.sum(F.when(disc > 0.05, price).otherwise(0.0)).alias("hi"), F.sum(price).alias("s"))]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = synth.lineitem_rows(a.sf)
    lines = [f"tools/bench_case_when.py --sf {a.sf:g} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, torch {torch.__version__}]",
             f"rows={rows}; GROUP BY l_returnflag; median (min - max) ms over {a.reps} repeats, every query once per repeat"]
    with HipExecutionEngine(device=0, work_folder=Path(tempfile.mkdtemp(prefix="hipspark_case_"))) as engine:
        path = Path(tempfile.mkdtemp(prefix="hipspark_case_t_")) / "lineitem.bin"
        engine.attach_device_table(path, synth.make_lineitem(engine.dev, path, rows))
        qs = queries(engine, str(path))
        engine.dev.time_scan_kernel(True)
        results, scans = {}, {}
        for name, frames in qs.items():  # set-up: compile, record, first replay
            for _ in range(max(a.warmup, 3)):
                results[name] = [f.collect() for f in frames]
            scans[name] = dict(engine.dev.last_scan)
        step = {name: [] for name in qs}
        kernel = {name: [] for name in qs}
        stream = torch.cuda.current_stream(engine.dev.device)
        for _ in range(a.reps):
            for name, frames in qs.items():
                s_ms = k_ms = 0.0
                for f in frames:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f.collect()
                    e1.record(stream)
                    e1.synchronize()
                    s_ms += e0.elapsed_time(e1)
                    k_ms += engine.dev.scan_kernel_ms()
                step[name].append(s_ms)
                kernel[name].append(k_ms)
        for name in qs:
            s, k = step[name], kernel[name]
            lines.append(f"({name:<2}) step {statistics.median(s):8.3f} ms ({min(s):.3f} - {max(s):.3f})   kernel "
                         f"{statistics.median(k):8.3f} ms ({min(k):.3f} - {max(k):.3f})   {len(qs[name])} scan(s)   "
                         f"kernel spread (max - min) / median {(max(k) - min(k)) / statistics.median(k):.4f}, "
                         f"(p75 - p25) / median {(statistics.quantiles(k, n=4)[2] - statistics.quantiles(k, n=4)[0]) / statistics.median(k):.4f}")
        med = {name: statistics.median(kernel[name]) for name in qs}
        smed = {name: statistics.median(step[name]) for name in qs}
        if "b" in qs:
            lines.append(f"kernel  (b)/(a) = {med['b'] / med['a']:.4f}   (b)/(a') = {med['b'] / med[A1]:.4f}   "
                         f"(b)/(a2) = {med['b'] / med['a2']:.4f}   (b)/(c) = {med['b'] / med['c']:.4f}")
            lines.append(f"step    (b)/(a) = {smed['b'] / smed['a']:.4f}   (b)/(a') = {smed['b'] / smed[A1]:.4f}   "
                         f"(b)/(a2) = {smed['b'] / smed['a2']:.4f}   (b)/(c) = {smed['b'] / smed['c']:.4f}")
            # the buckets of (c) are (b)'s columns: hi = the first scan's sums, s = both scans' sums added
            hi_b = {r["l_returnflag"]: r["hi"] for r in results["b"][0]}
            hi_c = {r["l_returnflag"]: r["s"] for r in results["c"][0]}
            lines.append(f"check: (b).hi against (c)'s first scan per group (f32 of differently grouped f64 sums): "
                         f"{ {k: (hi_b[k], hi_c.get(k)) for k in sorted(hi_b)} }")
        lines.append(f"scan of (a): {scans['a']}")
        if "b" in qs:
            lines.append(f"scan of (b): {scans['b']}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
