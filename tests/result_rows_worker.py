"""One rank of the two-rank tests of the operators over result rows (ORDER BY, SELECT DISTINCT, the window items):
`result_rows_worker.py <module> <function> <golden name> <out.json> [--runs N] [--hex-floats]` runs the query that
`<module>.<function>(api, paths)` builds over the tables of the golden set through HipExecutionEngine.enable_distributed
(gloo), N times (2).  Every rank scans its share of the tables; rank 0 gathers the rows, runs the operator over them and
writes what it read back: one list of values per row, or with --hex-floats one object per row, its floats as hex."""

from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

os.environ["TZ"] = "UTC"
time.tzset()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("module")
    ap.add_argument("function")
    ap.add_argument("golden")
    ap.add_argument("out", type=Path)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--hex-floats", action="store_true")
    a = ap.parse_args()
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api
    from tests.conftest import load_golden

    build = getattr(importlib.import_module(a.module), a.function)
    constants.SHUFFLE_FOLDER = a.out.parent / f"shuffle_r{rank}"
    golden = load_golden(a.golden)
    with HipExecutionEngine(device=0) as engine:
        engine.enable_distributed(dist)
        runs = [build(engine_api(engine), golden["paths"]).collect() for _ in range(a.runs)]
    assert all(run == runs[0] for run in runs), "a repeated query must return the same rows"
    if rank != 0:
        assert runs[0] == [], f"rank {rank} must not own result rows"
    elif a.hex_floats:
        a.out.write_text(json.dumps([{k: (v.hex() if type(v) is float else v) for k, v in r.items()} for r in runs[0]]))
    else:
        a.out.write_text(json.dumps([list(r.values()) for r in runs[0]]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
