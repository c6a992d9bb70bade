"""One rank of the two-rank ORDER BY test (tests/test_gpu_order_by.py): `order_by_worker.py <out.json>` runs the
many_groups GROUP BY with ORDER BY ... LIMIT through HipExecutionEngine.enable_distributed (gloo) and rank 0 writes
the rows it read back (floats as hex)."""

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
    from tests.test_gpu_order_by import many_groups_sorted

    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_r{rank}"
    golden = load_golden("many_groups")
    with HipExecutionEngine(device=0) as engine:
        engine.enable_distributed(dist)
        frame = many_groups_sorted(engine_api(engine), golden["paths"])
        runs = [frame.collect() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2], "a repeated query must return the same rows"
    if rank == 0:
        out_path.write_text(json.dumps([{k: (v.hex() if type(v) is float else v) for k, v in r.items()} for r in runs[0]]))
    else:
        assert runs[0] == [], f"rank {rank} must not own result rows"
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
