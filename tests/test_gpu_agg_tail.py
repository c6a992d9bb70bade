"""The aggregate tail of include/hipspark.h at the C ABI, with no query engine in between: hs_agg_finish with a
projection, hs_agg_units_merge, hs_agg_units_to_slab, hs_agg_pack and hs_slab_unpack over hand-built device buffers,
each against its Python statement in tests/agg_tail_models.py (pinned on the CPU by tests/test_agg_tail_models.py),
bit for bit - every operator here has one sequential order, so nothing takes a tolerance.

Canary rule (as tests/test_gpu_row_ops.py): every output buffer is at least 64 elements longer than the operator
needs and pre-filled with a fixed non-zero pattern; after every call everything the operator does not own must still
hold the pattern.  Status bits go to a flags word of the test's own.

hs_agg_finish numbers its groups by dictionary slot, and hs_agg_units_merge places keys by hash: both outputs are
compared as mappings from key bytes (key words) to the row's bytes, never by position."""

from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np
import pytest

from tests import agg_tail_models as m

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = 1, 2
GUARD = 64
CANARY = 0x5A
MERGE_LDS_MAX = 150 * 1024  # HS_MERGE_LDS_MAX of csrc/hs_agg.hip


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


@pytest.fixture()
def flags(dev):
    import torch

    word = dev.empty(1, torch.int32)
    word.zero_()
    return word


def _flags(word) -> int:
    return int(word.item()) & 0xFFFFFFFF


def _bytes_out(dev, nbytes):
    """nbytes of output followed by GUARD * 8 canary bytes, all pre-filled with the canary."""
    import torch

    t = dev.empty(nbytes + GUARD * 8, torch.uint8)
    t.fill_(CANARY)
    return t


def _intact(t, owned) -> bool:
    return bool((t[owned:] == CANARY).all().item())


def _assert_same_bytes(got, want, what=""):
    """Byte arrays equal; on a mismatch the message names the first differing offset and how many bytes differ."""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.flatnonzero(got != want)
    if len(diff):
        at = int(diff[0])
        raise AssertionError(f"{what}: {len(diff)} bytes differ, first at offset {at}: got {bytes(got[at: at + 8]).hex()} "
                             f"want {bytes(want[at: at + 8]).hex()}")


def _up(dev, arr):
    import torch

    return dev.to_device(np.ascontiguousarray(arr).view(np.uint8).reshape(-1), torch.uint8)


# ---- keys -------------------------------------------------------------------------------------------------------------
def _key_bytes(hs, kind, key_len):
    return key_len if kind == hs.STR else {hs.I32: 4, hs.F32: 4, hs.I64: 8, hs.F64: 8, hs.U8: 1}[kind]


def _encode_key(hs, kind, value) -> bytes:
    if kind == hs.STR:
        return value
    return struct.pack({hs.I32: "<i", hs.F32: "<f", hs.I64: "<q", hs.F64: "<d", hs.U8: "<B"}[kind], value)


def _key_candidates(hs, rng, kind, key_len, n):
    """n distinct keys of the kind as Python values (what the model groups by); the float sets hold 0.0 AND -0.0."""
    if kind == hs.I32:
        return [int(v) for v in rng.choice(np.arange(-50, 50), size=n, replace=False)]
    if kind == hs.I64:
        return [int(v) * (2**32 + 3) for v in rng.choice(np.arange(-50, 50), size=n, replace=False)]
    if kind == hs.U8:
        return [int(v) for v in rng.choice(np.arange(0, 256), size=n, replace=False)]
    if kind == hs.STR:
        out: list[bytes] = []
        while len(out) < n:
            text = bytes(rng.integers(65, 91, key_len).astype(np.uint8))
            if text not in out:
                out.append(text)
        return out
    pool = [1.5, -2.25, 1e10, -3e-5, 7.0, 0.1, -0.1, 123456.789, 2.0**-20, -65536.0][: n - 2]
    to = (lambda v: float(np.float32(v))) if kind == hs.F32 else float
    return [to(pool[0]), to(pool[1]), 0.0, -0.0] + [to(v) for v in pool[2:]]


# ---- slabs ------------------------------------------------------------------------------------------------------------
BIG = float(np.float32(1e30))


def _build_slabs(hs, rng, world, units, cap, key_kind, key_len, keys, first_zero=0.0, all_padding=False):
    """`world` slabs of units * cap rows: key column, an F32 and an I32 accumulator column.  Block b (order key b) is
    unit b // world of rank b % world; a unit holds a key at most once, at scattered rows; block 2 holds no rows; every
    unused row carries order key -1 and canary bytes.  keys[0] meets 1e30, -1e30, 1.0 in its first three blocks (the sum
    shows the merge order), keys[1] meets integers next to 2**31 (the sums pass it).
    -> (slabs uint8[world][nbytes], layout, model rows (order, rank-major row, key, (float, int)))"""
    import torch

    from minispark_amd.distributed import SlabLayout

    kb, m_rows = _key_bytes(hs, key_kind, key_len), units * cap
    layout = SlabLayout.build(m_rows, [(kb, torch.uint8), (4, torch.float32), (4, torch.int32)])
    slabs = np.full((world, layout.nbytes), CANARY, dtype=np.uint8)
    slabs[:, 0:16] = 0
    rows, seen0 = [], 0
    zeros = [k for k in keys if isinstance(k, float) and k == 0.0]
    for b in range(world * units):
        rank, u = b % world, b // world
        view = slabs[rank]
        order = view[layout.order_offset: layout.order_offset + 8 * m_rows].view(np.int64)
        order[u * cap: (u + 1) * cap] = -1
        if b == 2 or all_padding:
            continue
        rest = [k for k in keys[2:] if rng.random() < 0.6 and not (isinstance(k, float) and k == 0.0)]
        rng.shuffle(rest)
        present = list(keys[:2]) + rest
        if zeros and (b == 0 or rng.random() < 0.6):  # one zero per unit at most: the two are ONE key to the merge
            z = first_zero if b == 0 else zeros[int(rng.integers(0, len(zeros)))]
            present.append(z)
        present = present[:cap]
        for j, pos in enumerate(rng.permutation(cap)[: len(present)]):
            key, row = present[j], u * cap + int(pos)
            f = float(np.float32(rng.normal(0, 1e3)))
            i = int(rng.integers(1, 10**6)) * (1 if rng.random() < 0.5 else -1)
            if key == keys[0]:  # (the candidates put the zeros third and fourth: keys[0] and keys[1] are never one)
                f = [BIG, -BIG, 1.0][seen0] if seen0 < 3 else f
                seen0 += 1
            if key == keys[1]:
                i = 2**31 - 1 - int(rng.integers(0, 1000))
            order[row] = b
            view[layout.columns[0].offset + row * kb: layout.columns[0].offset + (row + 1) * kb] = np.frombuffer(
                _encode_key(hs, key_kind, key), dtype=np.uint8)
            view[layout.columns[1].offset + 4 * row: layout.columns[1].offset + 4 * row + 4] = np.frombuffer(struct.pack("<f", f), dtype=np.uint8)
            view[layout.columns[2].offset + 4 * row: layout.columns[2].offset + 4 * row + 4] = np.frombuffer(struct.pack("<i", i), dtype=np.uint8)
            rows.append((b, rank * m_rows + row, key, (f, i)))
    return slabs, layout, rows


def _slab_desc(hs, layout, key_kind, key_len, acc_kinds):
    desc = hs.hs_slab_desc()
    desc.slab_rows, desc.stride, desc.order_off, desc.key_off = layout.slab_rows, layout.nbytes, layout.order_offset, layout.columns[0].offset
    desc.key_kind, desc.key_len, desc.n_acc = key_kind, key_len, len(acc_kinds)
    for a, kind in enumerate(acc_kinds):
        desc.acc_off[a], desc.acc_kind[a] = layout.columns[1 + a].offset, kind
    return desc


def _finish_lds(world, slab_rows, stride, n_fold, n_order, cap, image_bytes):
    """The byte formula of hs_agg_finish (csrc/hs_agg.hip): -> (LDS bytes of the merge + projection stack, whether the
    slabs, the merged cells and the image move into LDS as well).  A test cannot observe the variant; it can choose it."""
    n_rows = world * slab_rows
    lds = cap * 16 + n_rows * n_fold * 8 + n_rows * 12 + cap * 16 + n_order * 8 + 16
    total = ((lds + 15) & ~15) + 9 * 64 * 8
    extra = ((world * stride + 15) & ~15) + ((cap * 8 * (n_fold + 2) + 15) & ~15) + image_bytes
    return total, stride % 8 == 0 and total + extra <= MERGE_LDS_MAX


class _Finish:
    """One hs_agg_finish call set up from a lowering: offsets assigned, buffers with canaries, the image decoded."""

    def __init__(self, dev, hs, slabs, layout, key_kind, key_len, fin, prog, outs, n_order, merge_cap, acc_kinds=None):
        self.dev, self.hs, self.fin, self.prog, self.outs = dev, hs, fin, prog, outs
        self.world, self.n_order, self.cap = slabs.shape[0], n_order, merge_cap
        self.kb = _key_bytes(hs, key_kind, key_len)
        self.desc = _slab_desc(hs, layout, key_kind, key_len, acc_kinds or [hs.F32, hs.I32])
        pos, self.offsets, self.widths = 16, [], []
        for o, (src, _, kind) in enumerate(outs):
            width = self.kb if src == 0 else 8 if kind == hs.I64 else 4
            fin.outs[o].offset = pos
            self.offsets.append(pos)
            self.widths.append(width)
            pos = (pos + merge_cap * width + 15) & ~15
        self.image_bytes = pos
        self.gathered = _up(dev, slabs)
        self.result = _bytes_out(dev, self.image_bytes)
        self.scratch_bytes = int(dev.lib.hs_agg_finish_scratch_bytes(merge_cap, fin.n_fold))
        self.scratch = _bytes_out(dev, self.scratch_bytes)
        self.slab_flags = 0
        for r in range(self.world):
            self.slab_flags |= int(slabs[r, 0:4].view(np.uint32)[0])

    def variant_is_small(self):
        return _finish_lds(self.world, self.desc.slab_rows, self.desc.stride, self.fin.n_fold, self.n_order, self.cap,
                           self.image_bytes)[1]

    def launch(self, flags, n_order=None, cap=None):
        return self.dev.lib.hs_agg_finish(self.dev.stream, self.gathered.data_ptr(), self.world, C.byref(self.desc),
                                          C.byref(self.fin), C.byref(self.prog) if self.prog is not None else None,
                                          self.n_order if n_order is None else n_order, self.cap if cap is None else cap,
                                          self.result.data_ptr(), self.scratch.data_ptr(), flags.data_ptr(), None)

    def untouched(self):
        return _intact(self.result, 0) and _intact(self.scratch, 0)

    def image(self):
        """-> (header flags, number of groups, {key bytes: [column bytes]}); checks `done` and both canaries."""
        host = self.result.cpu().numpy()
        assert int(host[4:8].view(np.uint32)[0]) == 1, "the done word"
        assert _intact(self.result, self.image_bytes) and _intact(self.scratch, self.scratch_bytes)
        ng = int(host[8:16].view(np.int64)[0])
        assert 0 <= ng <= self.cap
        key_col = [o for o, (src, _, _) in enumerate(self.outs) if src == 0][0]
        table = {}
        for g in range(ng):
            cells = [bytes(host[off + g * w: off + (g + 1) * w]) for off, w in zip(self.offsets, self.widths)]
            assert cells[key_col] not in table, "a key came out twice"
            table[cells[key_col]] = cells
        return int(host[0:4].view(np.uint32)[0]), ng, table


def _expected(hs, rows, model_folds, schema, project, outs, key_kind):
    """The models composed: fold, project, store.  -> ({key bytes: [column bytes or None]}, flags)"""
    groups = m.fold_partials(rows, model_folds)
    values, flag_bits = m.project(groups, project, schema)
    table = {}
    for key, vals in zip(groups, values):
        cells = []
        for (src, _, kind), v in zip(outs, vals):
            if src == 0:
                cells.append(_encode_key(hs, key_kind, key))
            elif v is None:
                cells.append(None)
            else:
                data, f = m.store(v, kind)
                flag_bits |= f
                cells.append(data)
        table[_encode_key(hs, key_kind, key)] = cells
    return table, flag_bits


def _assert_image(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for key, cells in want.items():
        for o, cell in enumerate(cells):
            if cell is not None:  # None: the reference raises there and has no bytes
                assert got[key][o] == cell, (what, key, o, got[key][o].hex(), cell.hex())


# ---- the projection: lowered, and re-assembled by hand --------------------------------------------------------------------
def _merged_schema(T, key_type):
    return [("k", key_type), ("sf", T.FLOAT), ("nf", T.FLOAT), ("xf", T.FLOAT), ("si", T.INTEGER), ("ni", T.INTEGER), ("xi", T.INTEGER)]


AGG_TO_ACC = [0, 0, 0, 1, 1, 1]  # one slab column folded three times with different ops, twice over


def _aggs():
    from minispark_amd.sql import Col, Functions as F

    return [F.sum(Col("sf")), F.min(Col("nf")), F.max(Col("xf")), F.sum(Col("si")), F.min(Col("ni")), F.max(Col("xi"))]


def _model_folds():
    return [(0, m.SUM), (0, m.MIN), (0, m.MAX), (1, m.SUM), (1, m.MIN), (1, m.MAX)]


def _wide_projection(T):
    """(expression, stored type) per result column; every computed column is `a <op> b` over two merged columns - the
    shape the host-side decoder of hs_agg_finish turns into its direct (group, entry) evaluation."""
    from minispark_amd.sql import Col

    cols = [
        (Col("k"), None),
        (Col("sf"), T.FLOAT), (Col("nf"), T.FLOAT), (Col("xf"), T.FLOAT),
        (Col("si"), T.TIMESTAMP), (Col("ni"), T.INTEGER), (Col("xi"), T.INTEGER),  # merged aggregates as F32 / I64 / I32
        ((Col("sf") / Col("si")).alias("a1"), T.FLOAT),    # float / int: I2F on the top cell
        ((Col("si") / Col("xf")).alias("a2"), T.FLOAT),    # int / float: I2F on the cell below
        ((Col("si") / Col("xi")).alias("a3"), T.FLOAT),    # int / int: both
        ((Col("sf") - Col("xf")).alias("d1"), T.FLOAT),
        ((Col("xf") - Col("sf")).alias("d2"), T.FLOAT),
        ((Col("ni") - Col("xi")).alias("d3"), T.INTEGER),
        ((Col("ni") * Col("xi")).alias("mu"), T.TIMESTAMP),
        ((Col("si") + Col("xi")).alias("pl"), T.TIMESTAMP),  # int + int stored as I64
        ((Col("k") + Col("si")).alias("ks"), T.TIMESTAMP),  # the key as an operand: program slot with prog_src = -1
        ((Col("sf") * Col("k")).alias("sk"), T.FLOAT),
    ]
    return cols


def _twin(T, cols):
    """The same columns plus one the decoder must refuse (a literal operand; three operands): the decoder then gives up
    on the WHOLE program, and every column goes through the one-wave interpreter."""
    from minispark_amd.sql import Col, Lit

    return cols[:9] + [((Col("sf") + Lit(0.5)).alias("t1"), T.FLOAT)] + cols[9:] + [
        ((Col("sf") + Col("ni") * Col("xi")).alias("t2"), T.FLOAT)]


def _reverse_sequences(prog):
    """Hand re-assembly: the `... OUT o` sequences of a program in reverse order.  Every sequence starts from an empty
    stack, so the program computes the same outputs - but prog_out[] no longer follows the program order."""
    from minispark_amd import hipspark as hs

    seqs, cur = [], []
    for i in range(prog.n_ins):
        cur.append(int(prog.ins[i]))
        if cur[-1] & 0xFF == hs.OP_OUT:
            seqs.append(cur)
            cur = []
    assert not cur and len(seqs) >= 2
    for i, w in enumerate(w for seq in reversed(seqs) for w in seq):
        prog.ins[i] = w
    return prog


def _lower(hs, T, key_kind, key_type, cols):
    from minispark_amd.lowering import lower_finish

    schema = _merged_schema(T, key_type)
    project = [e for e, _ in cols]
    out_schema = [(f"c{o}", key_type if t is None else t) for o, (_, t) in enumerate(cols)]
    fin, prog, outs = lower_finish(AGG_TO_ACC, [hs.F32, hs.I32], key_kind, _aggs(), schema, project, out_schema)
    return schema, project, fin, prog, outs


def _decoder_accepts(hs, prog) -> bool:
    """Whether the program is made of `LD LD [I2F] [I2F] <arith> OUT` sequences only (the shape csrc/hs_agg.hip decodes)."""
    arith = {hs.OP_ADD_F, hs.OP_SUB_F, hs.OP_MUL_F, hs.OP_DIV_F, hs.OP_ADD_I, hs.OP_SUB_I, hs.OP_MUL_I}
    ops = [int(prog.ins[i]) & 0xFF for i in range(prog.n_ins)]
    i = 0
    while i < len(ops):
        if ops[i: i + 2] != [hs.OP_LD, hs.OP_LD]:
            return False
        i += 2
        while i < len(ops) and ops[i] == hs.OP_I2F:
            i += 1
        if i + 1 >= len(ops) or ops[i] not in arith or ops[i + 1] != hs.OP_OUT:
            return False
        i += 2
    return True


FORMS = ["simple", "twin", "simple-reversed", "twin-reversed"]


def _projection_case(dev, flags, world, units, cap, key_kind, form, want_small):
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(1000 * world + 10 * units + cap)
    n_keys = 6 if cap <= 8 else 10
    keys = _key_candidates(hs, rng, key_kind, 0, n_keys)
    slabs, layout, rows = _build_slabs(hs, rng, world, units, cap, key_kind, 0, keys)
    slabs[world - 1, 0:4].view(np.uint32)[0] = hs.FLAG_STR_TOO_LONG  # a remote status bit reaches the image header
    cols = _wide_projection(T)
    if form.startswith("twin"):
        cols = _twin(T, cols)
    schema, project, fin, prog, outs = _lower(hs, T, key_kind, T.INTEGER, cols)
    if form.endswith("reversed"):
        prog = _reverse_sequences(prog)
    assert _decoder_accepts(hs, prog) == form.startswith("simple")
    merge_cap = 16 if n_keys <= 8 else 32
    run = _Finish(dev, hs, slabs, layout, key_kind, 0, fin, prog, outs, world * units, merge_cap)
    assert run.variant_is_small() == want_small
    want, want_flags = _expected(hs, rows, _model_folds(), schema, project, outs, key_kind)
    assert len(want) >= 4
    images = []
    for _ in range(2):  # a second launch over the same buffers: the same image, the status words clean again
        assert run.launch(flags) == 0
        images.append(run.image())
        assert _flags(flags) == 0
    assert images[0] == images[1]
    got_flags, ng, got = images[0]
    assert got_flags == want_flags | hs.FLAG_STR_TOO_LONG and ng == len(want)
    _assert_image(got, want, form)
    return want_flags


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("world,units,cap", [(1, 5, 4), (3, 5, 4), (8, 5, 4), (1, 9, 8), (3, 9, 8), (8, 9, 8)])
def test_finish_projection_all_in_lds(dev, flags, world, units, cap, form):
    """hs_agg_finish with a projection over slabs that fit the all-in-LDS variant (at most 8 x 72 rows x 6 folds: 41 KB of
    merge state + 12 KB of slabs, against 150 KB).  SUM / MIN / MAX over the F32 and the I32 slab column (each column
    folded three times), negative I32 keys, scattered padding rows, a unit without rows, a sum that cancels only in block
    order, integer sums past 2**31; merged aggregates written as F32 / I32 / I64; float / int, int / float and int / int
    quotients (I2F on the top cell, the cell below, both), a - b beside b - a, k + SUM(x) and SUM(x) * k on the key.
    Each projection runs as `LD LD [I2F] op OUT` sequences (decoded on the host into direct evaluation), as a twin with
    two more columns the decoder refuses (the whole program then runs in the interpreter), and both again with the
    sequences re-assembled in reverse, so that prog_out[] differs from the program order.  Which path ran follows from
    the program's shape and cannot be observed from outside; all four must equal the model bit for bit."""
    from minispark_amd import hipspark as hs

    assert _projection_case(dev, flags, world, units, cap, hs.I32, form, want_small=True) == 0


@pytest.mark.parametrize("form", FORMS)
def test_finish_projection_from_global_memory(dev, flags, form):
    """2 slabs x 960 rows x 6 folds: 119 KB of merge state + projection stack fit LDS, another 38 KB of slabs do not
    (> 150 KB together), so slabs, merged cells and image stay in global memory.  120 blocks: the lane-group fold."""
    from minispark_amd import hipspark as hs

    assert _projection_case(dev, flags, 2, 60, 16, hs.I32, form, want_small=False) == 0


@pytest.mark.parametrize("form", ["simple", "twin"])
def test_finish_projection_reads_an_i64_key(dev, flags, form):
    """k + SUM(x) and SUM(x) * k with keys beyond 32 bits: the program's key slot (prog_src = -1) reads 8-byte elements."""
    from minispark_amd import hipspark as hs

    assert _projection_case(dev, flags, 3, 5, 4, hs.I64, form, want_small=True) == 0


KEY_CASES = [("I64", 0), ("F32", 0), ("F64", 0), ("U8", 0), ("STR", 1), ("STR", 2), ("STR", 4)]


@pytest.mark.parametrize("kind_name,key_len", KEY_CASES)
def test_finish_key_kinds(dev, flags, kind_name, key_len):
    """Every key kind the slab holds, under an AVG-shaped projection.  The float sets hold 0.0 and -0.0 in different
    blocks: they are one group (as Python dict keys), and the key bytes written are those of the group's first row in
    merge order - once a 0.0, once a -0.0."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col

    key_kind = getattr(hs, kind_name)
    key_type = {"I64": T.TIMESTAMP, "F32": T.FLOAT, "F64": T.FLOAT, "U8": T.INTEGER, "STR": T.STRING}[kind_name]
    cols = [(Col("k"), None), ((Col("sf") / Col("si")).alias("avg"), T.FLOAT), (Col("xi"), T.INTEGER), (Col("nf"), T.FLOAT)]
    for first_zero in ([0.0, -0.0] if kind_name in ("F32", "F64") else [0.0]):
        rng = np.random.default_rng(77 + key_len)
        keys = _key_candidates(hs, rng, key_kind, key_len, 7)
        slabs, layout, rows = _build_slabs(hs, rng, 3, 5, 8, key_kind, key_len, keys, first_zero=first_zero)
        schema, project, fin, prog, outs = _lower(hs, T, key_kind, key_type, cols)
        run = _Finish(dev, hs, slabs, layout, key_kind, key_len, fin, prog, outs, 15, 16)
        want, want_flags = _expected(hs, rows, _model_folds(), schema, project, outs, key_kind)
        assert run.launch(flags) == 0
        got_flags, ng, got = run.image()
        assert (got_flags, ng, _flags(flags)) == (want_flags, len(want), 0)
        _assert_image(got, want, (kind_name, first_zero))
        if kind_name in ("F32", "F64"):
            signs = {math.copysign(1.0, r[2]) for r in rows if r[2] == 0.0}
            assert signs == {1.0, -1.0}  # both zeros are among the partial rows ...
            assert _encode_key(hs, key_kind, first_zero) in got and _encode_key(hs, key_kind, -first_zero) not in got


def test_finish_over_nothing_but_padding(dev, flags):
    """Every row carries order key -1: zero groups, and the header still says so (flags, done, count)."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(5)
    slabs, layout, rows = _build_slabs(hs, rng, 3, 5, 4, hs.I32, 0, [1, 2, 3], all_padding=True)
    slabs[1, 0:4].view(np.uint32)[0] = hs.FLAG_DICT_FULL
    schema, project, fin, prog, outs = _lower(hs, T, hs.I32, T.INTEGER, _wide_projection(T))
    run = _Finish(dev, hs, slabs, layout, hs.I32, 0, fin, prog, outs, 15, 16)
    assert not rows and run.launch(flags) == 0
    assert run.image() == (hs.FLAG_DICT_FULL, 0, {}) and _flags(flags) == 0


def _hand_slabs(hs, world, cap, partials):
    """Slabs of ONE unit per rank (block = rank) from {key: [(rank, float, int)]}: I32 key, an F32 and an I32 column."""
    import torch

    from minispark_amd.distributed import SlabLayout

    layout = SlabLayout.build(cap, [(4, torch.uint8), (4, torch.float32), (4, torch.int32)])
    slabs = np.full((world, layout.nbytes), CANARY, dtype=np.uint8)
    slabs[:, 0:16] = 0
    used, rows = [0] * world, []
    for r in range(world):
        slabs[r, layout.order_offset: layout.order_offset + 8 * cap].view(np.int64)[:] = -1
    for key, parts in partials.items():
        for rank, f, i in parts:
            row = used[rank]
            used[rank] += 1
            f = struct.unpack("<f", struct.pack("<f", f))[0]
            v = slabs[rank]
            v[layout.order_offset + 8 * row: layout.order_offset + 8 * row + 8].view(np.int64)[0] = rank
            for c, data in zip(layout.columns, (struct.pack("<i", key), struct.pack("<f", f), struct.pack("<i", i))):
                v[c.offset + 4 * row: c.offset + 4 * row + 4] = np.frombuffer(data, dtype=np.uint8)
            rows.append((rank, rank * cap + row, key, (f, i)))
    return slabs, layout, rows


def _hand_case(dev, flags, partials, cols, twin=False, world=3, cap=8, merge_cap=8):
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col, Lit

    slabs, layout, rows = _hand_slabs(hs, world, cap, partials)
    if twin:
        cols = cols + [((Col("sf") + Lit(0.5)).alias("t1"), T.FLOAT)]
    schema, project, fin, prog, outs = _lower(hs, T, hs.I32, T.INTEGER, cols)
    assert prog is None or _decoder_accepts(hs, prog) != twin
    run = _Finish(dev, hs, slabs, layout, hs.I32, 0, fin, prog, outs, world, merge_cap)
    want, want_flags = _expected(hs, rows, _model_folds(), schema, project, outs, hs.I32)
    assert run.launch(flags) == 0
    got_flags, ng, got = run.image()
    assert ng == len(want) and _flags(flags) == 0
    _assert_image(got, want)
    return got_flags, want_flags


F32_MAX = 3.4028234663852886e38


@pytest.mark.parametrize("name,partials,stored,flag", [
    ("finite sum beyond f32", [(0, 2e38, 1), (1, 1.5e38, 1)], "FLOAT", "FLT"),
    ("negative finite sum beyond f32", [(0, -2e38, 1), (2, -1.5e38, 1)], "FLOAT", "FLT"),
    ("infinite sum", [(0, float("inf"), 1), (1, 1.0, 1)], "FLOAT", None),
    ("largest f32", [(0, F32_MAX, 1)], "FLOAT", None),
    ("2**24 + 1 rounds to even", [(0, 16777216.0, 1), (1, 1.0, 1)], "FLOAT", None),
    ("integer sum is 2**31", [(0, 0.0, 2**31 - 1), (1, 0.0, 1)], "INTEGER", "INT"),
    ("integer sum is 2**31 - 1", [(0, 0.0, 2**31 - 2), (1, 0.0, 1)], "INTEGER", None),
    ("integer sum below -2**31", [(0, 0.0, -2**31), (2, 0.0, -1)], "INTEGER", "INT"),
    ("integer sum is -2**31", [(0, 0.0, -2**31 + 1), (2, 0.0, -1)], "INTEGER", None),
    ("integer sum past 2**31 as I64", [(0, 0.0, 2**31 - 1), (1, 0.0, 2**31 - 1), (2, 0.0, 2**31 - 1)], "TIMESTAMP", None),
])
def test_finish_stored_kinds_flag_exactly_what_the_reference_cannot_write(dev, flags, name, partials, stored, flag):
    """A merged aggregate (src 1) written as F32 / I32 / I64: HS_FLAG_FLT_OVERFLOW / HS_FLAG_INT_OVERFLOW exactly when
    struct.pack('<f') / int.to_bytes(4) raise OverflowError; the other groups' bytes are right either way."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col

    data = {5: partials, -6: [(0, 1.5, 10), (1, 2.5, 20)], 7: [(2, -1.0, -3)]}
    cols = [(Col("k"), None), (Col("sf") if stored == "FLOAT" else Col("si"), getattr(T, stored)), (Col("xf"), T.FLOAT)]
    got_flags, want_flags = _hand_case(dev, flags, data, cols)
    literal = {None: 0, "FLT": hs.FLAG_FLT_OVERFLOW, "INT": hs.FLAG_INT_OVERFLOW}[flag]
    assert got_flags == want_flags == literal, name


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("case", ["zero divisor", "product beyond int32", "neither"])
def test_finish_projection_flags_come_from_one_group(dev, flags, case, twin):
    """A quotient whose divisor is zero in exactly one group (HS_FLAG_DIV_ZERO), an int * int stored as I32 that overflows
    in exactly one group (HS_FLAG_INT_OVERFLOW): the flag is raised, every other group's bytes are still right, and with
    neither no flag is raised - through the decoded form and through the interpreter."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col

    data = {5: [(0, 1.0, 3), (1, 2.0, -3)], -6: [(0, 1.5, 10), (1, 2.5, 20)], 7: [(2, -1.0, 46341)], 8: [(1, 4.0, 46340)]}
    cols = [(Col("k"), None), ((Col("ni") * Col("xi")).alias("sq"), T.INTEGER)]
    if case != "product beyond int32":
        data.pop(7)  # 46341 ** 2 > 2**31 - 1 >= 46340 ** 2
    if case == "zero divisor":  # SUM(i) of key 5 is 3 - 3
        cols += [((Col("sf") / Col("si")).alias("q1"), T.FLOAT), ((Col("xi") / Col("si")).alias("q2"), T.FLOAT)]
    else:
        cols.append(((Col("sf") / Col("xi")).alias("q1"), T.FLOAT))
    got_flags, want_flags = _hand_case(dev, flags, data, cols, twin=twin)
    literal = {"zero divisor": hs.FLAG_DIV_ZERO, "product beyond int32": hs.FLAG_INT_OVERFLOW, "neither": 0}[case]
    assert got_flags == want_flags == literal


def test_finish_reports_a_full_merge_table(dev, flags):
    """Five groups against a merge capacity of four: HS_FLAG_MERGE_FULL in the image header."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col

    slabs, layout, _ = _hand_slabs(hs, 2, 8, {k: [(0, 1.0, 1), (1, 2.0, 2)] for k in (1, -2, 3, -4, 5)})
    _, _, fin, prog, outs = _lower(hs, T, hs.I32, T.INTEGER, [(Col("k"), None), (Col("sf"), T.FLOAT)])
    run = _Finish(dev, hs, slabs, layout, hs.I32, 0, fin, prog, outs, 2, 4)
    assert run.launch(flags) == 0
    got_flags, ng, _ = run.image()
    assert got_flags == hs.FLAG_MERGE_FULL and ng == 4 and _flags(flags) == 0


def test_finish_refuses_bad_arguments_without_launching(dev, flags):
    """HS_E_ARG / HS_E_LIMIT are decided on the host: nothing is launched, result and scratch keep their canaries."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.sql import Col

    cols = [(Col("k"), None), (Col("sf"), T.FLOAT), ((Col("sf") / Col("si")).alias("avg"), T.FLOAT)]
    slabs, layout, _ = _hand_slabs(hs, 2, 8, {1: [(0, 1.0, 1), (1, 2.0, 2)]})

    runs = []

    def fresh(key_kind=hs.I32, key_len=0):
        _, _, fin, prog, outs = _lower(hs, T, hs.I32, T.INTEGER, cols)
        runs.append(_Finish(dev, hs, slabs, layout, key_kind, key_len, fin, prog, outs, 2, 8))
        return runs[-1]

    run = fresh()
    assert run.launch(flags, cap=12) == E_ARG and run.launch(flags, cap=0) == E_ARG  # not a power of two
    assert run.launch(flags, n_order=0) == E_ARG and run.launch(flags, n_order=65537) == E_ARG
    assert fresh(hs.STR, 3).launch(flags) == E_ARG
    run.fin.fold_src[0] = 2  # the slab has two accumulator columns
    assert run.launch(flags) == E_ARG
    run = fresh()
    run.fin.fold_src[0] = -1
    assert run.launch(flags) == E_ARG
    run = fresh()
    run.fin.outs[1].offset = 8  # inside the header
    assert run.launch(flags) == E_ARG
    run = fresh()
    run.prog = None  # a src-2 output without a program
    assert run.launch(flags) == E_ARG
    assert all(r.untouched() for r in runs) and _flags(flags) == 0
    run = fresh()
    assert run.launch(flags) == 0 and run.image()[1] == 1  # guard: the same call, left alone, is accepted


def test_finish_refuses_rows_beyond_the_lds_tier(dev, flags):
    """8 slabs x 4096 rows x 3 folds need 32768 * (3 * 8 + 12) = 1.1 MB of LDS against 150 KB: HS_E_LIMIT, no launch."""
    import torch

    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.distributed import SlabLayout
    from minispark_amd.lowering import lower_finish
    from minispark_amd.sql import Col, Functions as F

    layout = SlabLayout.build(4096, [(4, torch.uint8), (4, torch.float32), (4, torch.int32)])
    slabs = np.zeros((8, layout.nbytes), dtype=np.uint8)
    schema = [("k", T.INTEGER), ("a", T.FLOAT), ("b", T.INTEGER), ("c", T.INTEGER)]
    fin, prog, outs = lower_finish([0, 1, 1], [hs.F32, hs.I32], hs.I32, [F.sum(Col("a")), F.sum(Col("b")), F.max(Col("c"))],
                                   schema, [Col("k"), (Col("a") / Col("b")).alias("avg")], [("k", T.INTEGER), ("avg", T.FLOAT)])
    assert fin.n_fold == 3
    run = _Finish(dev, hs, slabs, layout, hs.I32, 0, fin, prog, outs, 64, 64)
    assert run.launch(flags) == E_LIMIT
    assert run.untouched() and _flags(flags) == 0


# ---- hs_agg_units_merge ---------------------------------------------------------------------------------------------------
SPEC_A = [(m.SUM, 0), (m.MIN, 1), (m.MAX, 0), (m.SUM, 1)]
SPEC_B = [(m.MIN, 0), (m.MAX, 1), (m.SUM, 0), (m.MIN, 1)]


def _spec(hs, pairs):
    spec = hs.hs_agg_spec()
    spec.n_acc = len(pairs)
    for a, (op, is_int) in enumerate(pairs):
        spec.op[a], spec.is_int[a] = op, is_int
    return spec


def _random_cell(rng, is_int):
    if is_int:
        return m.i64_bits(int(rng.integers(-2**40, 2**40)))
    return m.f64_bits(float(rng.normal(0, 1e6)))


def _rank_tables(rng, world, n_units, cap, pairs, universe):
    """Per rank (keys, cells): every rank holds a random subset of universe[u] for unit u, at arbitrary slots (a table is
    read slot by slot: where the hash would have put a key does not matter); free slots hold garbage cells."""
    na, tables = len(pairs), []
    for _ in range(world):
        keys = np.full(n_units * cap, m.EMPTY, dtype=np.uint64)
        cells = rng.integers(0, 2**63, n_units * cap * na, dtype=np.uint64)
        for u in range(n_units):
            mine = [k for k in universe[u] if rng.random() < 0.6]
            for k, s in zip(mine, rng.permutation(cap)[: len(mine)]):
                at = u * cap + int(s)
                keys[at] = k
                for a, (_, is_int) in enumerate(pairs):
                    cells[at * na + a] = _random_cell(rng, is_int)
        tables.append((keys, cells))
    return tables


def _gathered(tables, header_flags=None):
    parts = []
    for r, (keys, cells) in enumerate(tables):
        head = np.zeros(16, dtype=np.uint8)
        head[4:16] = CANARY
        head[0:4].view(np.uint32)[0] = header_flags[r] if header_flags else 0
        parts += [head, keys.view(np.uint8), cells.view(np.uint8)]
    return np.concatenate(parts)


def _run_units_merge(dev, hs, flags, tables, n_units, cap, pairs, header_flags=None, expect=0):
    world, na = len(tables), len(pairs)
    d_in = _up(dev, _gathered(tables, header_flags))
    out_keys = _bytes_out(dev, n_units * cap * 8)
    out_acc = _bytes_out(dev, n_units * cap * na * 8)
    rc = dev.lib.hs_agg_units_merge(dev.stream, d_in.data_ptr(), world, n_units, cap, C.byref(_spec(hs, pairs)),
                                    out_keys.data_ptr(), out_acc.data_ptr(), flags.data_ptr())
    assert rc == expect
    if expect:
        assert _intact(out_keys, 0) and _intact(out_acc, 0)
        return None
    assert _intact(out_keys, n_units * cap * 8) and _intact(out_acc, n_units * cap * na * 8)
    keys = out_keys[: n_units * cap * 8].cpu().numpy().view(np.uint64)
    cells = out_acc[: n_units * cap * na * 8].cpu().numpy().view(np.uint64)
    got = {}
    for u in range(n_units):
        table = {}
        for s in range(u * cap, (u + 1) * cap):
            k = int(keys[s])
            if k != m.EMPTY:  # (a free slot holds exactly the empty word: anything else is read as a key and must match)
                assert k not in table, "a key occupies two slots"
                table[k] = [int(c) for c in cells[s * na: (s + 1) * na]]
        got[u] = table
    return got, keys, cells


def _universe(rng, n_units, cap, fill):
    """Key words per unit: INTEGER keys of both signs under the unit's id."""
    return [[m.int_key_word(int(v), u) for v in rng.choice(np.arange(-5000, 5000), size=max(1, int(cap * fill)), replace=False)]
            for u in range(n_units)]


@pytest.mark.parametrize("world,n_units,cap,pairs", [
    (1, 1, 16, [(m.SUM, 0)]), (2, 7, 256, SPEC_A), (8, 127, 16, SPEC_B), (2, 1, 1024, SPEC_A), (8, 7, 1024, [(m.MAX, 1)]),
    (2, 127, 256, [(m.MIN, 0)]), (8, 1, 256, SPEC_B), (1, 7, 16, SPEC_A), (2, 127, 16, [(m.SUM, 1)])])
def test_units_merge_folds_raw_cells_in_rank_order(dev, flags, world, n_units, cap, pairs):
    """Raw unit tables of `world` ranks over overlapping key subsets -> one table per unit: per unit a mapping from key
    word to un-rounded 64-bit cells, equal to the rank-order fold bit for bit (SUM / MIN / MAX over f64 and i64 cells
    from their identities; unit_cap 1024 exceeds the 256-lane workgroup).  With eight ranks, one key of unit 0 meets
    1e30, -1e30, 1.0 on ranks 1, 4 and 6 only: taken in rank order the sum is 1.0, in reverse order 0.0."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(world * 100_000 + n_units * 1000 + cap + len(pairs))
    universe = _universe(rng, n_units, cap, 0.6)
    tables = _rank_tables(rng, world, n_units, cap, pairs, universe)
    float_sums = [a for a, (op, is_int) in enumerate(pairs) if op == m.SUM and not is_int]
    if world == 8 and float_sums:
        k, na = universe[0][0], len(pairs)
        for rank, v in zip((1, 4, 6), (1e30, -1e30, 1.0)):
            keys, cells = tables[rank]
            where = np.flatnonzero(keys[:cap] == k)
            at = int(where[0]) if len(where) else int(np.flatnonzero(keys[:cap] == m.EMPTY)[0])
            keys[at] = k
            for a, (_, is_int) in enumerate(pairs):
                cells[at * na + a] = m.f64_bits(v) if a in float_sums else _random_cell(rng, is_int)
        for rank in (0, 2, 3, 5, 7):
            tables[rank][0][:cap][tables[rank][0][:cap] == k] = m.EMPTY
    want, over = m.units_merge(tables, pairs, cap)
    assert not over
    got, _, _ = _run_units_merge(dev, hs, flags, tables, n_units, cap, pairs)
    assert _flags(flags) == 0
    for u in range(n_units):
        assert got[u] == want[u], u
    if world == 8 and float_sums:
        assert got[0][universe[0][0]][float_sums[0]] == m.f64_bits(1.0)


@pytest.mark.parametrize("cap", [16, 1024])
def test_units_merge_capacity_edge(dev, flags, cap):
    """A unit whose union of keys over the ranks is exactly unit_cap merges completely without a flag; one key more and
    HS_FLAG_DICT_FULL is raised while every other unit is still right."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(cap)
    pairs, n_units, world = SPEC_A, 3, 2
    universe = _universe(rng, n_units, cap, 0.5)
    universe[1] = _universe(rng, 2, cap, 1.0)[1]  # cap keys under unit id 1
    tables = _rank_tables(rng, world, n_units, cap, pairs, universe)
    na = len(pairs)
    for r, part in enumerate((universe[1][: cap * 3 // 4], universe[1][cap // 4:])):  # overlapping, union = all cap keys
        keys, cells = tables[r]
        keys[cap: 2 * cap] = m.EMPTY
        for k, s in zip(part, rng.permutation(cap)[: len(part)]):
            keys[cap + int(s)] = k
            for a, (_, is_int) in enumerate(pairs):
                cells[(cap + int(s)) * na + a] = _random_cell(rng, is_int)
    want, over = m.units_merge(tables, pairs, cap)
    assert not over and len(want[1]) == cap
    got, keys, _ = _run_units_merge(dev, hs, flags, tables, n_units, cap, pairs)
    assert _flags(flags) == 0 and got == want
    assert (keys[cap: 2 * cap] != m.EMPTY).all()

    extra = m.int_key_word(9999, 1)
    assert extra not in universe[1]
    keys1 = tables[1][0]
    free = cap + int(np.flatnonzero(keys1[cap: 2 * cap] == m.EMPTY)[0])
    keys1[free] = extra
    want, over = m.units_merge(tables, pairs, cap)
    assert over == {1}
    got, _, _ = _run_units_merge(dev, hs, flags, tables, n_units, cap, pairs)
    assert _flags(flags) == hs.FLAG_DICT_FULL
    assert got[0] == want[0] and got[2] == want[2]
    assert len(got[1]) == cap and all(want[1][k] == cells for k, cells in got[1].items())  # one key of rank 1 is missing


def test_units_merge_status_and_refusals(dev, flags):
    """A status bit in the LAST rank's header reaches *flags; n_units = 128 and unit_cap = 24 are HS_E_ARG, no launch."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(3)
    pairs = [(m.SUM, 0)]
    tables = _rank_tables(rng, 3, 2, 16, pairs, _universe(rng, 2, 16, 0.5))
    got, _, _ = _run_units_merge(dev, hs, flags, tables, 2, 16, pairs, header_flags=[0, 0, hs.FLAG_STR_TOO_LONG])
    assert _flags(flags) == hs.FLAG_STR_TOO_LONG and got == m.units_merge(tables, pairs, 16)[0]
    flags.zero_()
    big = _rank_tables(rng, 1, 128, 16, pairs, _universe(rng, 128, 16, 0.5))
    _run_units_merge(dev, hs, flags, big, 128, 16, pairs, expect=E_ARG)
    odd = _rank_tables(rng, 1, 2, 24, pairs, _universe(rng, 2, 24, 0.5))
    _run_units_merge(dev, hs, flags, odd, 2, 24, pairs, expect=E_ARG)
    assert _flags(flags) == 0


# ---- hs_agg_units_to_slab ---------------------------------------------------------------------------------------------------
SLAB_SPEC = [(m.SUM, 0), (m.SUM, 1), (m.MIN, 0)]


def _slab_layout(hs, slab_rows, kb, pairs):
    import torch

    from minispark_amd.distributed import SlabLayout

    layout = SlabLayout.build(slab_rows, [(kb, torch.uint8)] + [(4, torch.int32)] * len(pairs))
    desc = {"unit_cap": None, "slab_rows": slab_rows, "nbytes": layout.nbytes, "order_off": layout.order_offset,
            "key_off": layout.columns[0].offset, "key_bytes": kb, "acc_off": [c.offset for c in layout.columns[1:]]}
    return layout, desc


def _unit_keys(rng, key_name, kb, n_units, cap, fill):
    keys = np.full(n_units * cap, m.EMPTY, dtype=np.uint64)
    for u in range(n_units):
        n = max(1, int(cap * fill))
        if key_name == "I32":
            words = [m.int_key_word(int(v), u) for v in rng.choice(np.arange(-2**31, 2**31, 2**20 + 7), size=n, replace=False)]
            words[0] = m.int_key_word(-1 - u, u)
        elif key_name == "U8":
            words = [m.int_key_word(int(v), u) for v in rng.choice(np.arange(256), size=min(n, 200), replace=False)]
        else:
            texts = {bytes(rng.integers(33, 127, kb).astype(np.uint8)) for _ in range(n if kb > 1 else min(n, 60))}
            words = [m.str_key_word(t, u) for t in texts]
        for w, s in zip(words, rng.permutation(cap)[: len(words)]):
            keys[u * cap + int(s)] = w
    return keys


def _run_to_slab(dev, hs, flags, keys, cells, n_units, cap, pairs, key_kind, key_len, slab_rows, expect=0, acc_kinds=None):
    kb = _key_bytes(hs, key_kind, key_len)
    layout, desc = _slab_layout(hs, slab_rows, kb, pairs)
    desc["unit_cap"] = cap
    slab = _bytes_out(dev, layout.nbytes)
    cdesc = _slab_desc(hs, layout, key_kind, key_len, acc_kinds or [hs.I32 if it else hs.F32 for _, it in pairs])
    d_keys, d_cells = _up(dev, keys), _up(dev, cells)  # (named: a tensor lives as long as its name)
    rc = dev.lib.hs_agg_units_to_slab(dev.stream, d_keys.data_ptr(), d_cells.data_ptr(), n_units, cap,
                                      C.byref(_spec(hs, pairs)), slab.data_ptr(), C.byref(cdesc), flags.data_ptr())
    assert rc == expect
    if expect:
        assert _intact(slab, 0)
        return None
    assert _intact(slab, layout.nbytes)
    return slab[: layout.nbytes].cpu().numpy(), layout, desc


SLAB_KEYS = [("I32", 0), ("U8", 0), ("STR", 1), ("STR", 2), ("STR", 4)]


@pytest.mark.parametrize("n_units,cap,slab_rows", [(127, 256, 127 * 256), (3, 16, 64)])
@pytest.mark.parametrize("key_name,key_len", SLAB_KEYS)
def test_units_to_slab_matches_the_model(dev, flags, key_name, key_len, n_units, cap, slab_rows):
    """Raw unit tables -> exchange slab, the whole slab byte for byte: order key u or -1, the key rebuilt from the low bytes
    of the key word (negative INTEGER keys, the table byte, packed strings), cells rounded once per unit.  Free slots and
    the rows past n_units * unit_cap get order key -1 and nothing else: their key and accumulator bytes, and the slab's
    header, keep the canary.  127 x 256 rows are twice what the 64 x 256 launch covers in one pass."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(n_units + key_len)
    key_kind = getattr(hs, key_name)
    kb = _key_bytes(hs, key_kind, key_len)
    keys = _unit_keys(rng, key_name, kb, n_units, cap, 0.55)
    cells = np.empty((n_units * cap, 3), dtype=np.uint64)
    cells[:, 0] = (rng.normal(0, 1e6, n_units * cap) + 1e-3).view(np.uint64)
    cells[:, 1] = rng.integers(-2**31, 2**31, n_units * cap).astype(np.int64).view(np.uint64)
    cells[:, 2] = rng.normal(0, 50, n_units * cap).view(np.uint64)
    cells = cells.reshape(-1)
    slab, layout, desc = _run_to_slab(dev, hs, flags, keys, cells, n_units, cap, SLAB_SPEC, key_kind, key_len, slab_rows)
    want, want_flags, undefined = m.units_to_slab(keys, cells, SLAB_SPEC, desc, np.full(layout.nbytes, CANARY, dtype=np.uint8))
    assert want_flags == 0 and not undefined and _flags(flags) == 0
    _assert_same_bytes(slab, want, key_name)
    order = slab[desc["order_off"]: desc["order_off"] + 8 * slab_rows].view(np.int64)
    assert (order[n_units * cap:] == -1).all() and (order >= 0).sum() == (keys != m.EMPTY).sum()


@pytest.mark.parametrize("name,cell,flag", [
    ("2**31 in an INTEGER cell", (1, m.i64_bits(2**31)), "INT"),
    ("-2**31 - 1 in an INTEGER cell", (1, m.i64_bits(-2**31 - 1)), "INT"),
    ("INT32 extremes", (1, m.i64_bits(-2**31)), None),
    ("a finite 3.5e38", (0, m.f64_bits(3.5e38)), "FLT"),
    ("an infinite cell", (0, m.f64_bits(float("-inf"))), None),
    ("a NaN cell", (0, 0x7FF8000000000000), None),
    ("2**24 + 1 rounds once", (0, m.f64_bits(float(2**24 + 1))), None),
    ("a FLOAT MIN left at its identity", (2, m.f64_bits(float(2**31 - 1))), "TYPE"),
    ("a FLOAT MIN one below its identity", (2, m.f64_bits(float(2**31 - 2))), None),
])
def test_units_to_slab_rounding_and_flags(dev, flags, name, cell, flag):
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(11)
    n_units, cap = 3, 16
    keys = _unit_keys(rng, "I32", 4, n_units, cap, 0.5)
    cells = np.empty(n_units * cap * 3, dtype=np.uint64)
    cells[0::3], cells[1::3], cells[2::3] = m.f64_bits(1.25), m.i64_bits(2**31 - 1), m.f64_bits(-7.5)
    at = int(np.flatnonzero(keys[cap:] != m.EMPTY)[0]) + cap  # an occupied slot of unit 1
    cells[3 * at + cell[0]] = cell[1]
    slab, layout, desc = _run_to_slab(dev, hs, flags, keys, cells, n_units, cap, SLAB_SPEC, hs.I32, 0, 64)
    want, want_flags, undefined = m.units_to_slab(keys, cells, SLAB_SPEC, desc, np.full(layout.nbytes, CANARY, dtype=np.uint8))
    literal = {None: 0, "INT": hs.FLAG_INT_OVERFLOW, "FLT": hs.FLAG_FLT_OVERFLOW, "TYPE": hs.FLAG_TYPE_ASSERT}[flag]
    assert _flags(flags) == want_flags == literal, name
    for off, n in undefined:  # the reference raises there and writes nothing: no bytes to compare
        want[off: off + n] = slab[off: off + n]
    _assert_same_bytes(slab, want, name)


def test_units_to_slab_refusals(dev, flags):
    """HS_E_LIMIT for a key that cannot be rebuilt from a key word (I64); HS_E_ARG when a slab column's kind does not match
    the aggregate, or the slab is shorter than the tables.  Nothing is launched."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(2)
    keys = _unit_keys(rng, "I32", 4, 3, 16, 0.5)
    cells = np.zeros(3 * 16 * 3, dtype=np.uint64)
    _run_to_slab(dev, hs, flags, keys, cells, 3, 16, SLAB_SPEC, hs.I64, 0, 64, expect=E_LIMIT)
    _run_to_slab(dev, hs, flags, keys, cells, 3, 16, SLAB_SPEC, hs.I32, 0, 64, expect=E_ARG, acc_kinds=[hs.F32, hs.F32, hs.F32])
    _run_to_slab(dev, hs, flags, keys, cells, 3, 16, SLAB_SPEC, hs.I32, 0, 64, expect=E_ARG, acc_kinds=[hs.I32, hs.I32, hs.F32])
    _run_to_slab(dev, hs, flags, keys, cells, 3, 16, SLAB_SPEC, hs.I32, 0, 47, expect=E_ARG)
    assert _flags(flags) == 0


def test_units_merge_to_slab_finish_chain(dev, flags):
    """hs_agg_units_merge over 3 ranks -> hs_agg_units_to_slab -> hs_agg_finish (world 1) with an AVG-shaped projection,
    each stage fed with the stage before on the device, against the models composed the same way.  A key value occurs in
    several units, so the final fold crosses units (in unit order) after the one rounding per unit."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.lowering import lower_finish
    from minispark_amd.sql import Col, Functions as F

    rng = np.random.default_rng(41)
    world, n_units, cap, pairs = 3, 5, 16, [(m.SUM, 0), (m.SUM, 1), (m.MAX, 0)]
    values = [int(v) for v in rng.choice(np.arange(-40, 40), size=12, replace=False)]
    universe = [[m.int_key_word(v, u) for v in values if rng.random() < 0.7] for u in range(n_units)]
    tables = _rank_tables(rng, world, n_units, cap, pairs, universe)
    na = len(pairs)
    for keys, cells in tables:  # counts and sums of a plausible size (the chain must not overflow on its way)
        cells[1::na] = rng.integers(1, 1000, len(keys)).astype(np.uint64)
    spec = _spec(hs, pairs)
    d_in = _up(dev, _gathered(tables))
    out_keys, out_acc = _bytes_out(dev, n_units * cap * 8), _bytes_out(dev, n_units * cap * na * 8)
    assert dev.lib.hs_agg_units_merge(dev.stream, d_in.data_ptr(), world, n_units, cap, C.byref(spec), out_keys.data_ptr(),
                                      out_acc.data_ptr(), flags.data_ptr()) == 0
    slab_rows = n_units * cap
    layout, desc = _slab_layout(hs, slab_rows, 4, pairs)
    desc["unit_cap"] = cap
    cdesc = _slab_desc(hs, layout, hs.I32, 0, [hs.F32, hs.I32, hs.F32])
    slab = _bytes_out(dev, layout.nbytes)
    slab[:16] = 0  # the header of a rank's own slab: flags, pad, row count
    assert dev.lib.hs_agg_units_to_slab(dev.stream, out_keys.data_ptr(), out_acc.data_ptr(), n_units, cap, C.byref(spec),
                                        slab.data_ptr(), C.byref(cdesc), flags.data_ptr()) == 0
    schema = [("k", T.INTEGER), ("s", T.FLOAT), ("c", T.INTEGER), ("x", T.FLOAT)]
    project = [Col("k"), (Col("s") / Col("c")).alias("avg"), Col("x"), Col("c")]
    out_schema = [("k", T.INTEGER), ("avg", T.FLOAT), ("x", T.FLOAT), ("c", T.INTEGER)]
    fin, prog, outs = lower_finish([0, 1, 2], [hs.F32, hs.I32, hs.F32], hs.I32,
                                   [F.sum(Col("s")), F.sum(Col("c")), F.max(Col("x"))], schema, project, out_schema)
    assert _flags(flags) == 0
    host_slab = slab[: layout.nbytes].cpu().numpy().reshape(1, -1)
    run = _Finish(dev, hs, host_slab, layout, hs.I32, 0, fin, prog, outs, n_units, 32, acc_kinds=[hs.F32, hs.I32, hs.F32])
    run.gathered = slab  # the device buffer the stage before wrote, not a copy of it
    assert run.launch(flags) == 0
    got_flags, ng, got = run.image()

    merged, over = m.units_merge(tables, pairs, cap)
    assert not over
    keys = np.full(n_units * cap, m.EMPTY, dtype=np.uint64)
    cells = np.zeros(n_units * cap * na, dtype=np.uint64)
    for u, table in merged.items():  # slot positions are the hash's business: any placement gives the same rows per unit
        for s, (k, acc) in enumerate(sorted(table.items())):
            keys[u * cap + s] = k
            cells[(u * cap + s) * na: (u * cap + s + 1) * na] = np.array(acc, dtype=np.uint64)
    model_slab, slab_flags, undefined = m.units_to_slab(keys, cells, pairs, desc)
    assert slab_flags == 0 and not undefined
    rows = []
    order = model_slab[desc["order_off"]: desc["order_off"] + 8 * slab_rows].view(np.int64)
    col = [model_slab[off: off + 4 * slab_rows] for off in [desc["key_off"]] + desc["acc_off"]]
    for r in range(slab_rows):
        rows.append((int(order[r]), r, int(col[0].view(np.int32)[r]),
                     (float(col[1].view(np.float32)[r]), int(col[2].view(np.int32)[r]), float(col[3].view(np.float32)[r]))))
    want, want_flags = _expected(hs, rows, [(0, m.SUM), (1, m.SUM), (2, m.MAX)], schema, project, outs, hs.I32)
    assert (got_flags, ng, _flags(flags)) == (want_flags, len(want), 0) and want_flags == 0
    assert len(want) >= 8
    _assert_image(got, want)


# ---- hs_agg_pack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("n_units,group_cap", [(300, 4), (5, 64), (7, 128), (3, 600)])
def test_agg_pack_matches_the_model(dev, flags, n_units, group_cap, with_ids):
    """Dense pack of slot arrays: units with no group, units with ngroups = group_cap, occupied slots anywhere in the unit;
    an F32 and an I32 output column; pack_start[n_units] is the total and rows past it are untouched.  300 units take the
    one-workgroup kernel twice round its scan, group_cap > 64 takes the workgroup-per-unit kernel (600 slots: three
    rounds of its 256 lanes)."""
    from minispark_amd import hipspark as hs

    rng = np.random.default_rng(n_units * 1000 + group_cap)
    slots = n_units * group_cap
    rep = np.full(slots, -1, dtype=np.int64)
    ngroups = np.zeros(n_units, dtype=np.int32)
    for u in range(n_units):
        n = [0, group_cap, int(rng.integers(0, group_cap + 1))][min(u % 5, 2)]
        ngroups[u] = n
        rep[u * group_cap + rng.permutation(group_cap)[:n]] = rng.integers(0, 10**6, n)
    acc = np.empty(slots * 2, dtype=np.uint64)
    for s in range(slots):
        acc[2 * s], acc[2 * s + 1] = m.f64_bits(float(rng.normal(0, 1e4)) + 1e-3), m.i64_bits(int(rng.integers(-2**31, 2**31)))
    unit_ids = (rng.permutation(n_units * 3)[:n_units]).astype(np.int64) if with_ids else None
    start, out_rep, cols, out_unit = m.pack(rep, acc, ngroups, group_cap, [hs.F32, hs.I32], unit_ids)
    total = int(start[-1])
    assert total == len(out_rep) and 0 in ngroups and group_cap in ngroups

    d_start = _bytes_out(dev, (n_units + 1) * 8)
    d_rep, d_unit = _bytes_out(dev, total * 8), _bytes_out(dev, total * 8)
    d_cols = [_bytes_out(dev, total * 4), _bytes_out(dev, total * 4)]
    col_ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in d_cols])
    kinds = (C.c_int32 * 2)(hs.F32, hs.I32)
    spec = _spec(hs, [(m.SUM, 0), (m.SUM, 1)])
    d_in = [_up(dev, rep), _up(dev, acc), _up(dev, ngroups)]
    d_ids = _up(dev, unit_ids) if with_ids else None
    hs.check(dev.lib.hs_agg_pack(dev.stream, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(),
                                 n_units, group_cap, C.byref(spec), d_start.data_ptr(), d_rep.data_ptr(), col_ptrs, kinds,
                                 d_ids.data_ptr() if with_ids else None, d_unit.data_ptr()), "hs_agg_pack")
    assert np.array_equal(d_start[: (n_units + 1) * 8].cpu().numpy().view(np.int64), start)
    assert np.array_equal(d_rep[: total * 8].cpu().numpy().view(np.int64), out_rep)
    assert np.array_equal(d_unit[: total * 8].cpu().numpy().view(np.int64), out_unit)
    for got, want in zip(d_cols, cols):
        assert np.array_equal(got[: total * 4].cpu().numpy(), want)
        assert _intact(got, total * 4)
    assert _intact(d_start, (n_units + 1) * 8) and _intact(d_rep, total * 8) and _intact(d_unit, total * 8)

    if not with_ids:  # without out_unit nothing is written there
        d_unit.fill_(CANARY)
        hs.check(dev.lib.hs_agg_pack(dev.stream, d_in[0].data_ptr(), d_in[1].data_ptr(),
                                     d_in[2].data_ptr(), n_units, group_cap, C.byref(spec), d_start.data_ptr(),
                                     d_rep.data_ptr(), col_ptrs, kinds, None, None), "hs_agg_pack")
        assert _intact(d_unit, 0) and np.array_equal(d_rep[: total * 8].cpu().numpy().view(np.int64), out_rep)
    assert _flags(flags) == 0


# ---- hs_slab_unpack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,counts", [(1, [200]), (3, [333, 0, 57]), (3, [1, 333, 332])])
def test_slab_unpack_matches_the_model(dev, flags, world, counts):
    """All-gathered slabs -> rank-major columns of 1, 4 and 8 bytes per row, the header flags per rank, and order keys with
    -1 on the rows at or beyond each rank's own count (333 rows per slab: more than one workgroup, an odd tail)."""
    import torch

    from minispark_amd import hipspark as hs
    from minispark_amd.distributed import SlabLayout

    rng = np.random.default_rng(world + counts[0])
    rows = 333
    layout = SlabLayout.build(rows, [(1, torch.uint8), (4, torch.int32), (8, torch.int64)])
    g = rng.integers(1, 256, (world, layout.nbytes)).astype(np.uint8)  # padding and dead rows hold noise
    for r in range(world):
        g[r, 0:4].view(np.int32)[0] = [hs.FLAG_DIV_ZERO, 0, hs.FLAG_STR_TOO_LONG | hs.FLAG_DICT_FULL][r]
        g[r, 8:16].view(np.int64)[0] = counts[r]
        g[r, 16: 16 + 8 * rows].view(np.int64)[:] = rng.integers(0, 1000, rows)
    offs = [c.offset for c in layout.columns]
    widths = [c.row_bytes for c in layout.columns]
    want_flags, want_order, want_cols = m.slab_unpack(g.reshape(-1), world, layout.nbytes, rows, layout.order_offset, offs, widths)
    d_flags, d_order = _bytes_out(dev, world * 4), _bytes_out(dev, world * rows * 8)
    d_cols = [_bytes_out(dev, world * rows * w) for w in widths]
    d_g = _up(dev, g)
    hs.check(dev.lib.hs_slab_unpack(dev.stream, d_g.data_ptr(), world, layout.nbytes, rows, layout.order_offset, 3,
                                    (C.c_int64 * 3)(*offs), (C.c_int32 * 3)(*widths),
                                    (C.c_void_p * 3)(*[t.data_ptr() for t in d_cols]), d_flags.data_ptr(), d_order.data_ptr()),
             "hs_slab_unpack")
    assert np.array_equal(d_flags[: world * 4].cpu().numpy().view(np.int32), want_flags) and _intact(d_flags, world * 4)
    assert np.array_equal(d_order[: world * rows * 8].cpu().numpy().view(np.int64), want_order)
    assert _intact(d_order, world * rows * 8)
    assert sum(int((want_order[r * rows: (r + 1) * rows] >= 0).sum()) for r in range(world)) == sum(counts)
    for t, want, w in zip(d_cols, want_cols, widths):
        assert np.array_equal(t[: world * rows * w].cpu().numpy(), want) and _intact(t, world * rows * w)
    assert _flags(flags) == 0
