"""The general join feeding a GROUP BY behind the stage ABI (hs_join_group_stage_*), end to end: 16 Mi build rows (every key
twice) x 64 Mi probe rows, grouped by a 5-value build-side STRING, SUM(probe FLOAT x build INTEGER) and COUNT().  One run
= WHERE-less side scans, JoinJob ordering, the join, the gathers through the pair rows, the shared-dictionary aggregate and
the tail; the tables are read into HBM once by prepare.  Wall time of hs_join_group_stage_run (it returns after its last
readback), median of --reps after one warm-up run.  Then the aggregate alone through the per-operator ABI on the same shapes
(pairs in JoinJob order, two per probe row): hs_agg_shared over pair-indexed columns (HS_PAIR) against hs_gather_fixed of
the columns + the same compiled hs_agg_shared over the gathered ones, timed with HIP events; both routes gather the 1-byte
key.  Bytes per pair are counted from the shapes (algorithmic), not measured.
Usage: python tools/bench_join_group.py [--build 16M] [--probe 64M] [--reps 5] [--dir /tmp/jg] [--out FILE]"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from minispark_amd.constants import ColumnType as T  # noqa: E402
from minispark_amd.io import BlockFile, StrCol  # noqa: E402

NAMES = [b"1-URGENT", b"2-HIGH", b"3-MEDIUM", b"4-NOT SPECIFIED", b"5-LOW"]
BLOCK = 1 << 21


def size(text: str) -> int:
    return int(float(text[:-1]) * (1 << 20)) if text[-1] in "Mm" else int(text)


def str_col(codes: np.ndarray) -> StrCol:
    lens = np.array([len(n) for n in NAMES], np.uint8)[codes]
    table = np.zeros((len(NAMES), max(len(n) for n in NAMES)), np.uint8)
    for i, n in enumerate(NAMES):
        table[i, : len(n)] = np.frombuffer(n, np.uint8)
    rows = table[codes]
    return StrCol(lens, rows[np.arange(rows.shape[1])[None, :] < lens[:, None]])


def write(path: Path, schema, cols) -> None:
    n = len(cols[0])
    blocks = []
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        blocks.append([str_col(c[0][lo:hi]) if isinstance(c, tuple) else c[lo:hi] for c in cols])
    BlockFile(path).write_raw_blocks(schema, blocks)


def per_operator(blob, nb: int, np_: int, reps: int) -> list[str]:
    """The aggregate of `blob` over 2 * np_ pairs on both routes -> report lines."""
    import ctypes as C

    import torch

    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    dev = "cuda"
    torch.manual_seed(7)
    half = nb // 2
    keys = torch.randperm(half, device=dev)  # build rows k and k + half hold key keys[k]
    posof = torch.empty_like(keys)
    posof[keys] = torch.arange(half, device=dev)
    table = {(0, 1): torch.randint(0, 5, (nb,), device=dev, dtype=torch.uint8),   # bs as code bytes
             (0, 2): torch.randint(1, 10, (nb,), device=dev, dtype=torch.int32),  # bi
             (1, 1): torch.randint(1, 100, (np_,), device=dev).float()}          # pf
    pk = torch.randint(0, half, (np_,), device=dev)
    part = pk % 10
    porder = torch.sort(part, stable=True).indices
    b0 = posof[pk[porder]]
    n = 2 * np_
    zeros = torch.zeros(8, dtype=torch.int64, device=dev)  # (a lane reads four pair rows at once)
    rows = {1: torch.cat([porder.repeat_interleave(2), zeros]), 0: torch.cat([torch.stack([b0, b0 + half], 1).reshape(-1), zeros])}
    unit_rows = [0] + (torch.cumsum(torch.bincount(part, minlength=10), 0) * 2).tolist()
    ur = (C.c_int64 * 11)(*unit_rows)
    geom = hs.hs_agg_geom()
    hs.check(lib.hs_agg_shared_geom(ur, 10, blob.spec.n_acc, 16, C.byref(geom)), "hs_agg_shared_geom")
    chunks = (hs.hs_chunk * geom.n_chunks)()
    chunk0 = (C.c_int64 * 11)()
    hs.check(lib.hs_agg_partial_chunks(ur, 10, C.byref(geom), chunks, chunk0), "hs_agg_partial_chunks")
    d_chunks = torch.frombuffer(bytearray(chunks), dtype=torch.uint8).to(dev)
    slots = 10 * geom.pad
    out_rep = torch.empty(slots, dtype=torch.int64, device=dev)
    out_acc = torch.empty(slots * max(blob.spec.n_acc, 1), dtype=torch.int64, device=dev)
    ngroups = torch.empty(11, dtype=torch.int32, device=dev)
    ws = torch.zeros(geom.ws_bytes // 8 + 64, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    key = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    gathered = {i: torch.empty(n + 16, dtype=torch.int32, device=dev) for i in range(blob.n_cols)}
    stream = torch.cuda.current_stream().cuda_stream

    def gather(src, width, side, dst):
        hs.check(lib.hs_gather_fixed(stream, src.data_ptr(), width, src.numel(), rows[side].data_ptr(), n, None, dst.data_ptr(),
                                     flags.data_ptr()), "hs_gather_fixed")

    def cols_for(pairs: bool):
        cols = (hs.hs_col * blob.n_cols)()
        for i in range(blob.n_cols):
            side, col = blob.col_side[i], blob.col_ids[i]
            src = table[(side, col)]
            if i == blob.key_slot:
                cols[i].kind, cols[i].fixed_len, cols[i].data = hs.STR, 1, key.data_ptr()
            elif pairs:
                cols[i].kind = hs.PAIR | (hs.F32 if src.dtype == torch.float32 else hs.I32)
                cols[i].fixed_len, cols[i].data, cols[i].offs = -1, src.data_ptr(), rows[side].data_ptr()
            else:
                cols[i].kind = hs.F32 if src.dtype == torch.float32 else hs.I32
                cols[i].fixed_len, cols[i].data = -1, gathered[i].data_ptr()
        return cols

    def run(pairs: bool, agg_only: bool):
        if not agg_only:
            gather(table[(0, 1)], 1, 0, key)
            for i in range(blob.n_cols):
                if i != blob.key_slot and not pairs:
                    gather(table[(blob.col_side[i], blob.col_ids[i])], 4, blob.col_side[i], gathered[i])
        hs.check(lib.hs_agg_shared(stream, cols_for(pairs), blob.n_cols, blob.key_slot, C.byref(blob.prog), C.byref(blob.spec),
                                   d_chunks.data_ptr(), 10, C.byref(geom), out_rep.data_ptr(), out_acc.data_ptr(),
                                   ngroups.data_ptr(), ws.data_ptr(), flags.data_ptr(), None, None), "hs_agg_shared")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]

    run(True, False)
    run(False, False)
    torch.cuda.synchronize()
    assert int(flags.item()) == 0, f"device flags {int(flags.item()):#x}"
    res = {(p, o): timed(lambda p=p, o=o: run(p, o)) for p in (True, False) for o in (True, False)}
    n_arg = blob.n_cols - 1
    key_b, pair_b, gath_b = 8 + 1 + 1, 1 + n_arg * (8 + 4), n_arg * (8 + 4 + 4) + 1 + n_arg * 4
    return [f"aggregate alone over {n} pairs (per-operator ABI, HIP events, median of {reps}):",
            f"  pair-indexed: hs_agg_shared {res[(True, True)]:.3f} ms; with the key gather {res[(True, False)]:.3f} ms"
            f" ({key_b + pair_b} B/pair from the shapes)",
            f"  gathered:     hs_agg_shared {res[(False, True)]:.3f} ms; with the key + {n_arg} column gathers {res[(False, False)]:.3f} ms"
            f" ({key_b + gath_b} B/pair from the shapes)"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="16M")
    ap.add_argument("--probe", default="64M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", type=Path, default=Path("/tmp/hipspark_join_group"))
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    nb, np_ = size(a.build), size(a.probe)
    rng = np.random.default_rng(7)
    a.dir.mkdir(parents=True, exist_ok=True)
    keys = rng.permutation(nb // 2).astype(np.int32)
    bk = np.concatenate([keys, keys])  # every key twice
    codes = rng.integers(0, len(NAMES), nb)
    # (a tuple marks the column written as a STRING column of those name codes)
    write(a.dir / "b.bin", [("bk", T.INTEGER), ("bs", T.STRING), ("bi", T.INTEGER)],
          [bk, (codes,), rng.integers(1, 10, nb).astype(np.int32)])
    write(a.dir / "p.bin", [("pk", T.INTEGER), ("pf", T.FLOAT)],
          [rng.integers(0, nb // 2, np_).astype(np.int32), rng.integers(1, 100, np_).astype(np.float32)])

    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions as F
    from minispark_amd.stage import NativeEngine, NativeJoinGroupStage

    q = (DataFrame(object()).table(str(a.dir / "b.bin")).join(DataFrame(object()).table(str(a.dir / "p.bin")),
                                                              on=Col("bk") == Col("pk"), how="inner")
         .group_by(Col("bs")).agg(F.sum(Col("pf") * Col("bi")).alias("w"), F.count()))
    lines = [f"join feeding a GROUP BY through hs_join_group_stage: {nb} build rows (each key twice) x {np_} probe rows"]
    with NativeEngine(0) as engine:
        t0 = time.perf_counter()
        stage = NativeJoinGroupStage(engine, q.task)
        lines.append(f"prepare (native reader, both tables, dictionary of the key): {time.perf_counter() - t0:.3f} s")
        rows = stage.run(a.dir / "out.bin")
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            stage.run(a.dir / "out.bin")
            ts.append(time.perf_counter() - t0)
        stats = stage.stats()
        stage.close()
    med = sorted(ts)[len(ts) // 2]
    lines += per_operator(stage.blob, nb, np_, a.reps)
    lines.append(f"stats: {stats}")
    lines.append(f"hs_join_group_stage_run: median {med * 1e3:.2f} ms of {a.reps} (all: {', '.join(f'{t * 1e3:.2f}' for t in ts)})")
    lines.append(f"  {stats['pairs'] / med / 1e9:.2f} G pairs/s, {np_ / med / 1e9:.2f} G probe rows/s")
    lines.append(f"groups: {len(rows)}, COUNT total {sum(r['count'] for r in rows) if rows and 'count' in rows[0] else '?'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        a.out.write_text(text + "\n")


if __name__ == "__main__":
    main()
