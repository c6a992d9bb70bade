"""The HBM (radix) aggregation tier behind the native scan stage against the engine's per-operator route:
    python tools/bench_stage_hbm.py [rows] [groups_per_block] [warmup] [steps]
One synthetic lineitem-like table (k INTEGER with ~groups_per_block values in every block, v FLOAT, q FLOAT) written as a
BlockFile of ROWS_PER_BLOCK-row blocks; `GROUP BY k` with SUM(v) + COUNT, once without and once with a WHERE that keeps about
half the rows, through HipExecutionEngine (collect_columns) and through NativeStage(hbm_tier=True).  Prints the median and the
min - max of either route, and the per-kernel times of one step of either route (hs_trace_begin / hs_trace_end)."""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

os.environ.setdefault("TZ", "UTC")
time.tzset()
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from minispark_amd import constants, hipspark as hs
from minispark_amd.constants import ColumnType as T
from minispark_amd.dataframe import DataFrame
from minispark_amd.execution import HipExecutionEngine
from minispark_amd.io import BlockFile
from minispark_amd.sql import Col, Functions as F
from minispark_amd.stage import NativeEngine, NativeStage

rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 59_986_052
groups = int(float(sys.argv[2])) if len(sys.argv) > 2 else 125_000
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
scratch = Path(tempfile.mkdtemp(prefix="hs_stage_hbm_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None))
constants.SHUFFLE_FOLDER = scratch / "shuffle"
rng = np.random.default_rng(1)
path = scratch / "t.bin"
per = constants.ROWS_PER_BLOCK
blocks = []
for lo in range(0, rows, per):
    n = min(per, rows - lo)
    blocks.append([rng.integers(0, groups, n).astype(np.int32), rng.uniform(900, 105_000, n).astype(np.float32),
                   rng.uniform(0, 1, n).astype(np.float32)])
BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("v", T.FLOAT), ("q", T.FLOAT)], blocks)
print(f"{rows} rows in {len(blocks)} blocks, ~{groups} keys per block", flush=True)
del blocks


def kernel_times(lib, stream, run, top=14):
    """One more step with every launch of the library bracketed by events -> its per-kernel times, summed by name."""
    if lib.hs_trace_begin(stream) != 0:
        return
    run()
    slices = (hs.hs_trace_slice * 512)()
    n = C.c_int32(0)
    if lib.hs_trace_end(stream, slices, 512, C.byref(n)) != 0:
        return
    total = {}
    for s in list(slices)[: n.value]:
        name = s.name.decode(errors="replace")
        total[name] = total.get(name, 0.0) + s.dur_us
    print(f"        {sum(total.values()) / 1e3:9.3f} ms  in {n.value} launches", flush=True)
    for name, us in sorted(total.items(), key=lambda kv: -kv[1])[:top]:
        print(f"        {us / 1e3:9.3f} ms  {name}", flush=True)


def report(label, times):
    ms = [t * 1e3 for t in times]
    print(f"{label}: median {statistics.median(ms):9.2f} ms  min {min(ms):9.2f}  max {max(ms):9.2f}  ({len(ms)} steps)", flush=True)


for where in (False, True):
    def query(engine):
        df = DataFrame(engine).table(str(path))
        if where:
            df = df.filter(Col("q") < 0.5)
        return df.group_by(Col("k")).agg(F.sum(Col("v")).alias("s"), F.count())

    tag = "WHERE q < 0.5" if where else "no WHERE"
    engine = HipExecutionEngine(0)
    q = query(engine)
    times = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        cols = q.collect_columns()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    report(f"engine  ({tag})", times)
    order = np.argsort(cols["k"], kind="stable")
    kernel_times(engine.dev._raw_lib, engine.dev.stream, q.collect_columns)
    engine.__exit__(None, None, None)
    with NativeEngine(0) as native:
        stage = NativeStage(native, query(object()).task, hbm_tier=True)
        times = []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            flags, nrows = C.c_uint32(0), C.c_int64(0)
            hs.check(stage.lib.hs_stage_run(stage.handle, None, C.byref(flags), C.byref(nrows)), "hs_stage_run")
            raw = stage.raw_columns()
            if i >= warmup:
                times.append(time.perf_counter() - t0)
        report(f"native  ({tag})", times)
        stats = stage.stats()
        print(f"        tier {stats['tier']}, {stats['partial_rows']} partial rows, {stats['result_rows']} result rows", flush=True)
        names = [n for n, _ in stage.schema]
        got = dict(zip(names, raw))
        norder = np.argsort(got["k"], kind="stable")
        assert np.array_equal(got["k"][norder], cols["k"][order]) and np.array_equal(got["s"][norder], cols["s"][order])

        def step():
            hs.check(stage.lib.hs_stage_run(stage.handle, None, C.byref(flags), C.byref(nrows)), "hs_stage_run")

        kernel_times(stage.lib, None, step)
        stage.close()
