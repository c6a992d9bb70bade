"""Child process of tests/test_gpu_date_parts.py: `date_parts_worker.py <out.json> <table>`.

The worker queries of the test module through one engine in THIS process - the evaluator form (HIPSPARK_JIT) is read once
per process - rows written with floats as hex and timestamps as text, next to the number of compiled-program launches."""

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


def main() -> None:
    out_path, table = Path(sys.argv[1]), sys.argv[2]
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from tests.test_gpu_date_parts import WORKER_QUERIES, hexed

    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_{out_path.stem}"
    with HipExecutionEngine(device=0) as engine:
        got = {name: hexed(engine.sql(text.format(t=table)).collect()) for name, text in WORKER_QUERIES.items()}
        counters = (C.c_int32 * 3)()
        engine.dev._raw_lib.hs_jit_stats(counters)
    got["jit_launches"] = int(counters[1])
    out_path.write_text(json.dumps(got))


if __name__ == "__main__":
    main()
