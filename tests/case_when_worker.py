"""Child process of tests/test_gpu_case_when.py: `case_when_worker.py <out.json> <table>`.

The grouped (Q12-shaped) and the keyless CASE query of the test module through one engine in THIS process - the evaluator
form (HIPSPARK_JIT) and dictionary coding (HIPSPARK_DICT) are read once per process - rows written with floats as hex,
next to the number of compiled-program launches and whether string columns were dictionary-coded."""

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


def hexed(rows: list) -> list:
    return [{k: (v.hex() if type(v) is float else v) for k, v in r.items()} for r in rows]


def main() -> None:
    out_path, table = Path(sys.argv[1]), sys.argv[2]
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine
    from tests.test_gpu_case_when import GROUPED_SQL, KEYLESS_SQL

    constants.SHUFFLE_FOLDER = out_path.parent / f"shuffle_{out_path.stem}"
    with HipExecutionEngine(device=0) as engine:
        got = {"grouped": hexed(engine.sql(GROUPED_SQL.format(t=table)).collect()),
               "keyless": hexed(engine.sql(KEYLESS_SQL.format(t=table)).collect()),
               "dict_enabled": bool(engine.dict_enabled)}
        counters = (C.c_int32 * 3)()
        engine.dev._raw_lib.hs_jit_stats(counters)
    got["jit_launches"] = int(counters[1])
    out_path.write_text(json.dumps(got))


if __name__ == "__main__":
    main()
