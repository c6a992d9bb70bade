"""One rank of the two-rank sliding frame test (tests/test_gpu_window_frames.py): `window_frames_worker.py <out.json>` runs
a select with a ranking item, a sliding sum, a sliding maximum, a sliding LAST_VALUE, QUALIFY and ORDER BY through
HipExecutionEngine.enable_distributed (gloo); every rank scans its share of the table, rank 0 gathers the rows, computes
the windows over them and writes what it read back."""

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


def main() -> None:
    out_path = Path(sys.argv[1])
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api
    from tests.conftest import load_golden
    from tests.test_gpu_window_frames import two_rank_frame

    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_r{rank}"
    golden = load_golden("q1_multiblock")
    with HipExecutionEngine(device=0) as engine:
        engine.enable_distributed(dist)
        runs = [two_rank_frame(engine_api(engine), golden["paths"]).collect() for _ in range(2)]
    assert runs[0] == runs[1], "a repeated query must return the same rows"
    if rank == 0:
        out_path.write_text(json.dumps([list(r.values()) for r in runs[0]]))
    else:
        assert runs[0] == [], f"rank {rank} must not own result rows"
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
