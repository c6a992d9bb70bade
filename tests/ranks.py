"""The launcher of the tests that run one query on several ranks: `run_ranks(argv)` starts one process per rank with the
environment torch.distributed reads (a free port on this host) and waits for them.  tests/test_gpu_distributed.py has its
own `_spawn_ranks`, which batches cases and returns the log."""

from __future__ import annotations

import os
import socket
import subprocess
import sys
import time


def run_ranks(argv, world=2, limit=240, env=None):
    """`python *argv` once per rank, RANK = 0 .. world - 1, `env` on top of this process's environment.  Asserts that every
    rank ended with 0 inside `limit` seconds; the failure shows the tail of every rank's output."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(world):
        rank_env = dict(os.environ, **(env or {}), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, *map(str, argv)], env=rank_env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    deadline = time.monotonic() + limit
    while (time.monotonic() < deadline and any(p.poll() is None for p in procs)
           and all(p.poll() in (None, 0) for p in procs)):
        try:
            next(p for p in procs if p.poll() is None).wait(timeout=0.5)
        except subprocess.TimeoutExpired:
            pass
    for p in procs:  # the first failure (or the time limit) ends the other ranks too
        if p.poll() is None:
            p.kill()
    logs = [p.communicate()[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(f"--- rank {r} ---\n{log[-2500:]}" for r, log in enumerate(logs))
