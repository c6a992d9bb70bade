"""Child process of tests/test_gpu_global_agg.py: `global_agg_worker.py forms|ranks <out.json> <table>`.

forms: every WHERE of the test module through one engine in THIS process (the evaluator form, HIPSPARK_JIT, is read once
       per process), rows written with floats as hex and the number of compiled-program launches.
ranks: one rank of the two-rank run (gloo): three of the WHEREs through HipExecutionEngine.enable_distributed; rank 0
       writes the rows it read back, the other rank must own none."""

from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

os.environ["TZ"] = "UTC"
time.tzset()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def hexed(rows: list) -> list:
    return [{k: (v.hex() if type(v) is float else v) for k, v in r.items()} for r in rows]


def main() -> None:
    mode, out_path, table = sys.argv[1], Path(sys.argv[2]), sys.argv[3]
    import ctypes as C

    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from tests.test_gpu_global_agg import WHERES, all_aggs, whole

    if mode == "forms":
        constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_{out_path.stem}"
        with HipExecutionEngine(device=0) as engine:
            rows = {name: hexed(whole(engine, table, cond, all_aggs).collect()) for name, cond in WHERES.items()}
            counters = (C.c_int32 * 4)()
            engine.dev._raw_lib.hs_jit_stats(counters)
        out_path.write_text(json.dumps({"rows": rows, "jit_launches": int(counters[1])}))
        return
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_r{rank}"
    got = {}
    with HipExecutionEngine(device=0) as engine:
        engine.enable_distributed(dist)
        for name in ("none", "empties_a_middle_unit", "empties_everything"):
            frame = whole(engine, table, WHERES[name], all_aggs)
            runs = [frame.collect() for _ in range(3)]
            assert runs[0] == runs[1] == runs[2], "a repeated query must return the same rows"
            if rank != 0:
                assert runs[0] == [], f"rank {rank} must not own result rows"
            got[name] = hexed(runs[0])
    if rank == 0:
        out_path.write_text(json.dumps(got))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
