"""What a GROUP BY over two columns costs: the packed composite key against the single key and against today's emulation by
string concatenation, over the synthetic lineitem with l_shipmode, through HipExecutionEngine.

  (a)  GROUP BY l_returnflag                                                       one code byte as the key
  (b)  SELECT l_returnflag + '-' + l_shipmode AS k, ... GROUP BY k                 the emulation: one code byte of the product
       dictionary (k_dict_combine), a glued STRING column in the result
  (c)  GROUP BY (l_returnflag, l_shipmode)                                         the key tuple: two code bytes packed by
       hs_key_pack, grouped as a fixed-length string of two bytes, cut back into the two columns by hs_key_unpack

all with SUM(l_extendedprice), SUM(l_quantity), COUNT().  A library without the key tuple times (a) and (b) only.

Per repeat every query runs once, in turn (drift of the box hits all of them alike).  Two clocks per query: `step` = a HIP
event pair on the launch stream around collect() (pack, scan, merge, unpack, hand-over; the collect ends with the result on
the host), `kernel` = the scan kernel's own event pair.  The pack kernel is timed on its own as well - an event pair around
Device.pack_key over the two code-byte columns - against its algorithmic bytes (sum of the part widths + W) x rows.
Reported: median (min - max) over --reps, (c)/(a) and (c)/(b) at the medians.
Usage: python tools/bench_group_by_keys.py [--sf 100] [--reps 20] [--warmup 3] [--out FILE]"""
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

HBM_PEAK = 8.0e12  # bytes / s, MI355X specification


def aggregates() -> list:
    return [F.sum(Col("l_extendedprice")).alias("s"), F.sum(Col("l_quantity")).alias("q"), F.count()]


def queries(engine, path: str) -> dict:
    def table():
        return DataFrame(engine).table(path)

    flag, mode = Col("l_returnflag"), Col("l_shipmode")
    out = {
        "a": table().group_by(flag).agg(*aggregates()),
        "b": (table().select((flag + "-" + mode).alias("k"), Col("l_extendedprice"), Col("l_quantity"))
              .group_by(Col("k")).agg(*aggregates())),
    }
    try:
        out["c"] = table().group_by(flag, mode).agg(*aggregates())
    except TypeError:  # a library whose group_by takes one column
        pass
    return out


def spread(values: list) -> str:
    return f"{statistics.median(values):8.3f} ms ({min(values):.3f} - {max(values):.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = synth.lineitem_rows(a.sf)
    lines = [f"tools/bench_group_by_keys.py --sf {a.sf:g} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, torch {torch.__version__}]",
             f"rows={rows}; SUM(l_extendedprice), SUM(l_quantity), COUNT(); median (min - max) ms over {a.reps} repeats, "
             "every query once per repeat"]
    with HipExecutionEngine(device=0, work_folder=Path(tempfile.mkdtemp(prefix="hipspark_keys_"))) as engine:
        path = Path(tempfile.mkdtemp(prefix="hipspark_keys_t_")) / "lineitem.bin"
        table = synth.make_lineitem(engine.dev, path, rows, with_shipmode=True)
        engine.attach_device_table(path, table)
        qs = queries(engine, str(path))
        engine.dev.time_scan_kernel(True)
        results, scans = {}, {}
        for name, frame in qs.items():  # set-up: dictionaries, compile, record, first replay
            for _ in range(max(a.warmup, 3)):
                results[name] = frame.collect()
            scans[name] = dict(engine.dev.last_scan)
        step = {name: [] for name in qs}
        kernel = {name: [] for name in qs}
        stream = torch.cuda.current_stream(engine.dev.device)
        for _ in range(a.reps):
            for name, frame in qs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                frame.collect()
                e1.record(stream)
                e1.synchronize()
                step[name].append(e0.elapsed_time(e1))
                kernel[name].append(engine.dev.scan_kernel_ms())
        for name in qs:
            lines.append(f"({name}) step {spread(step[name])}   scan kernel {spread(kernel[name])}   groups {len(results[name])}   "
                         f"tier {scans[name].get('tier')}, group_cap {scans[name].get('group_cap')}")
        smed = {name: statistics.median(step[name]) for name in qs}
        kmed = {name: statistics.median(kernel[name]) for name in qs}
        lines.append(f"step         (b)/(a) = {smed['b'] / smed['a']:.4f}" + (
            f"   (c)/(a) = {smed['c'] / smed['a']:.4f}   (c)/(b) = {smed['c'] / smed['b']:.4f}" if "c" in qs else ""))
        lines.append(f"scan kernel  (b)/(a) = {kmed['b'] / kmed['a']:.4f}" + (
            f"   (c)/(a) = {kmed['c'] / kmed['a']:.4f}   (c)/(b) = {kmed['c'] / kmed['b']:.4f}" if "c" in qs else ""))
        if "c" in qs:
            from minispark_amd.device import DBatch  # noqa: PLC0415

            names = [n for n, _ in table.schema]
            ids = [names.index("l_returnflag"), names.index("l_shipmode")]
            batch = DBatch([table.schema[i] for i in ids], [table.columns[i] for i in ids], rows)
            spec = engine.dev.key_spec(batch, [0, 1])
            packs = []
            for rep in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                packed = engine.dev.pack_key(batch, [0, 1])
                e1.record(stream)
                e1.synchronize()
                if rep >= 3:
                    packs.append(e0.elapsed_time(e1))
                del packed
            moved = (sum(p.width for p in spec.parts) + spec.width) * rows
            rate = moved / (statistics.median(packs) * 1e-3)
            lines.append(f"pack kernel (hs_key_pack, parts {[p.width for p in spec.parts]} -> W = {spec.width}) {spread(packs)}   "
                         f"{moved / 1e9:.3f} GB algorithmic = {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the "
                         f"{HBM_PEAK / 1e12:g} TB/s HBM peak; {100 * statistics.median(packs) / smed['c']:.1f} % of (c)'s step")
            glued = sorted(r["k"] for r in results["b"])
            tupled = sorted(f"{r['l_returnflag']}-{r['l_shipmode']}" for r in results["c"])
            lines.append(f"check: (c)'s tuples are (b)'s glued keys: {glued == tupled} ({len(tupled)} groups)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
