"""Whole-table aggregate benchmark: the Q6-shaped query of minispark_amd/workloads.py (a selective WHERE and one SUM, no
GROUP BY) over the synthetic lineitem, through HipExecutionEngine.

  keyless     df.filter(...).agg(SUM(l_extendedprice * l_discount))           reads 3 x f32 + i64 = 20 B/row
  --const-key the same WHERE and SUM under GROUP BY l_orderkey, with l_orderkey holding ONE value in every row: the only
              spelling a build without DataFrame.agg has (run it there for the parent comparison)   24 B/row

Per repeat: ms/step = wall time of --steps collect() calls after --warmup, kernel ms = median of the scan kernel's HIP
event pair; reported as the median and min - max over --repeats.  Algorithmic bytes = the stored widths of the columns
read x rows; fraction of 8 TB/s from the kernel time.
Usage: python tools/bench_global_agg.py [--sf 10] [--steps 20] [--warmup 3] [--repeats 5] [--const-key] [--out FILE]"""
from __future__ import annotations

import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs, synth  # noqa: E402
from minispark_amd.constants import ColumnType  # noqa: E402
from minispark_amd.device import DCol  # noqa: E402
from minispark_amd.execution import HipExecutionEngine  # noqa: E402
from minispark_amd.workloads import engine_api, q6  # noqa: E402


STORED_WIDTH = {ColumnType.INTEGER: 4, ColumnType.FLOAT: 4, ColumnType.TIMESTAMP: 8}


def stored_bytes_per_row(task, schema) -> int:
    """Sum of the stored widths of the table columns the query names (filters, key, aggregate arguments)."""
    names: set[str] = set()
    for node in task.task_chain:
        exprs = [getattr(node, "condition", None), getattr(node, "group_by_column", None), *getattr(node, "agg_columns", [])]
        for expr in exprs:
            if expr is not None:
                names.update(c.name for c in expr.all_nested_columns if type(c).__name__ == "Col")
    types = dict(schema)
    return sum(STORED_WIDTH[types[n]] for n in names)  # (a STRING column has no fixed width: KeyError, on purpose)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--const-key", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = synth.lineitem_rows(a.sf)
    lines = []
    with HipExecutionEngine(device=0, work_folder=Path(tempfile.mkdtemp(prefix="hipspark_gagg_"))) as engine:
        path = Path(tempfile.mkdtemp(prefix="hipspark_gagg_t_")) / "lineitem.bin"
        table = synth.make_lineitem(engine.dev, path, rows)
        if a.const_key:
            table.columns[0] = DCol(hs.I32, torch.full((rows,), 7, dtype=torch.int32, device=engine.dev.device), rows)
        engine.attach_device_table(path, table)
        frame = q6(engine_api(engine), str(path), group_by="l_orderkey" if a.const_key else None)
        engine.dev.time_scan_kernel(True)
        for _ in range(a.warmup):
            result = frame.collect()
        step_ms, kernel_ms = [], []
        for _ in range(a.repeats):
            ks = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                frame.collect()
                ks.append(engine.dev.scan_kernel_ms())
            step_ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            kernel_ms.append(statistics.median(ks))
        bytes_per_row = stored_bytes_per_row(frame.task, table.schema)
        gb = rows * bytes_per_row / 1e9
        k = statistics.median(kernel_ms)
        lines.append(f"sf={a.sf:g} rows={rows} "
                     f"mode={'const-key GROUP BY' if a.const_key else 'keyless agg'} scan={engine.dev.last_scan}")
        lines.append(f"result {result}")
        lines.append(f"ms/step   median {statistics.median(step_ms):.4f}  min {min(step_ms):.4f}  max {max(step_ms):.4f}  "
                     f"({a.repeats} repeats x {a.steps} steps)")
        lines.append(f"kernel ms median {k:.4f}  min {min(kernel_ms):.4f}  max {max(kernel_ms):.4f}  (event pair)")
        lines.append(f"algorithmic bytes {gb:.3f} GB ({bytes_per_row} B/row) -> {gb / k * 1e3:.1f} GB/s = "
                     f"{gb / k * 1e3 / 8000:.4f} of 8 TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
