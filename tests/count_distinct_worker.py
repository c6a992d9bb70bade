"""Worker of tests/test_gpu_count_distinct.py.

`count_distinct_worker.py tiers <table> <out.json>`: the three tier queries of the test over the generated table, in a
process of its own so that the switches in its environment (HIPSPARK_JIT=0, HIPSPARK_SHORT_TAIL=0) are read at start-up;
the rows go to <out.json>.
`count_distinct_worker.py ranks <out.json>`: one rank of a two-rank world (gloo, both on GPU 0): COUNT(DISTINCT) must raise
its NotImplementedError on every rank, before a collective, and the same query without it must still run afterwards."""

from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

os.environ["TZ"] = "UTC"
time.tzset()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def tiers(table: str, out_path: Path) -> None:
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api
    from tests.test_gpu_count_distinct import TIER_KEYS, tier_frame

    constants.SHUFFLE_FOLDER = out_path.parent / "shuffle_worker"
    with HipExecutionEngine(device=0) as engine:
        api = engine_api(engine)
        rows = {key: [list(r.values()) for r in tier_frame(api, table, key).collect()] for key in TIER_KEYS}
        counters = (C.c_int32 * 3)()
        engine.dev._raw_lib.hs_jit_stats(counters)  # [1] = launches of run-time compiled kernels in this process
        switches = {"short_tail": engine.short_tail_enabled, "jit_launches": int(counters[1])}
    out_path.write_text(json.dumps({"rows": rows, "switches": switches}))


def ranks(out_path: Path) -> None:
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api
    from tests.conftest import load_golden

    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_r{rank}"
    table = load_golden("q1_multiblock")["paths"]["lineitem"]
    with HipExecutionEngine(device=0) as engine:
        engine.enable_distributed(dist)
        api = engine_api(engine)
        C, F = api.Col, api.F
        refused = ""
        try:
            api.DataFrame().table(table).group_by(C("l_returnflag")).agg(F.count_distinct(C("l_shipmode")), F.count()).collect()
        except NotImplementedError as e:
            refused = str(e)
        # no rank is left in a collective: the same query without the distinct item runs on both
        plain = api.DataFrame().table(table).group_by(C("l_returnflag")).agg(F.count()).collect()
    Path(f"{out_path}.rank{rank}").write_text(json.dumps({"refused": refused, "rows": [list(r.values()) for r in plain]}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    if sys.argv[1] == "tiers":
        tiers(sys.argv[2], Path(sys.argv[3]))
    else:
        ranks(Path(sys.argv[2]))
