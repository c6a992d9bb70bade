"""The device's string predicates at the C ABI: hs_like / hs_str_cmp (csrc/hs_device.h) through hs_eval and hs_agg_scalar,
hand-built hs_col / hs_program, against tests/string_predicate_model.py (the reference's regex; Python bytes order).  Every
case runs in the run-time compiled form and in the interpreter form, and hs_jit_stats says which one ran.  Answers are
booleans: equality is exact.  One engine-level case at the end puts the same strings on either side of the dictionary cap."""

from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from tests import string_predicate_model as M
from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu

FORMS = [pytest.param(1, id="jit"), pytest.param(0, id="interpreter")]
PREFILL = 0xA5  # what output bytes hold before a launch: a row nobody wrote keeps it


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- programs -------------------------------------------------------------------------------------------------
def ins(op: int, sp: int, a: int = 0, b: int = 0, c: int = 0) -> int:
    return op | (sp << 8) | (a << 16) | (b << 32) | (c << 48)


def program(instructions: list[int], literals: list[bytes | int]):
    """hs_program: a `bytes` literal goes to the pool and its literal word is (pool offset << 32 | length); equal strings
    share their pool bytes but keep their own literal slot, so padding a program by repeating a string costs no pool."""
    from minispark_amd import hipspark as hs

    p = hs.hs_program()
    pool = bytearray()
    assert len(instructions) <= hs.HS_MAX_INS and len(literals) <= hs.HS_MAX_LIT
    for i, lit in enumerate(literals):
        if isinstance(lit, int):
            p.lit[i] = lit & 0xFFFFFFFFFFFFFFFF
            continue
        off = pool.find(lit) if lit else 0
        if off < 0:
            off = len(pool)
            pool += lit
        p.lit[i] = (off << 32) | len(lit)
    assert len(pool) <= hs.HS_MAX_POOL, len(pool)
    for i, b in enumerate(pool):
        p.pool[i] = b
    for i, w in enumerate(instructions):
        p.ins[i] = w
    p.n_ins, p.n_lit = len(instructions), len(literals)
    return p


def like_program(patterns: list[bytes], slot: int = 0):
    """HS_OP_LIKE pattern i; HS_OP_OUT i - for HS_MAX_OUTS patterns: ONE instruction shape whatever the patterns are."""
    from minispark_amd import hipspark as hs

    assert len(patterns) == hs.HS_MAX_OUTS
    code = []
    for i in range(len(patterns)):
        code += [ins(hs.OP_LIKE, 0, a=slot, b=i), ins(hs.OP_OUT, 1, a=i)]
    return program(code, patterns)


def blocks_of_16(patterns: list[bytes], pool_cap: int = 256) -> list[tuple[list[bytes], int]]:
    """Cut `patterns` into programs of exactly 16 whose bytes fit the literal pool: (block, how many of its patterns are its
    own); a short block is padded by repeating its first pattern."""
    out: list[list[bytes]] = []
    cur: list[bytes] = []
    for p in patterns:
        if len(cur) == 16 or sum(len(x) for x in cur) + len(p) > pool_cap:
            out.append(cur)
            cur = []
        cur.append(p)
    if cur:
        out.append(cur)
    return [(b + [b[0]] * (16 - len(b)), len(b)) for b in out]


# ---- columns --------------------------------------------------------------------------------------------------
class Column:
    """A STRING hs_col over tensors this object keeps alive.  Ragged: lens, offs = exclusive prefix sum, payload; the
    payload may sit at a byte shift inside its buffer.  Fixed: payload of n * width bytes, offs NULL."""

    def __init__(self, dev, strings: list[bytes], fixed: int | None = None, shift: int = 0):
        import torch

        from minispark_amd import hipspark as hs

        self.strings, self.n = strings, len(strings)
        lens = np.array([len(s) for s in strings], dtype=np.uint8)
        assert all(len(s) <= 255 for s in strings)
        payload = np.frombuffer(b"".join(strings), dtype=np.uint8)
        # the bytes in front of a shifted payload are 'a's too: a word load that starts before the first string sees them
        host = np.concatenate([np.full(shift, ord("a"), np.uint8), payload])
        self.buf = dev.to_device(host, torch.uint8)
        self.data = self.buf[shift:]
        self.lens = dev.to_device(lens, torch.uint8)
        self.offs = None
        col = hs.hs_col()
        col.kind = hs.STR
        col.data = self.data.data_ptr()
        col.lens = self.lens.data_ptr()
        if fixed is None:
            offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
            self.offs = dev.to_device(offs, torch.int64)
            col.fixed_len, col.offs = -1, self.offs.data_ptr()
        else:
            assert all(len(s) == fixed for s in strings)
            col.fixed_len, col.offs = fixed, None
        self.hs = col


def int_column(dev, values: np.ndarray):
    import torch

    from minispark_amd import hipspark as hs

    t = dev.to_device(values.astype(np.int32), torch.int32)
    col = hs.hs_col()
    col.kind, col.fixed_len, col.data = hs.I32, -1, t.data_ptr()
    return col, t


# ---- running, and knowing which form ran ---------------------------------------------------------------------
class Form:
    """`with Form(dev, jit) as f:` switches the evaluator form, counts the launches that CAN take the compiled form, and on
    the way out restores the compiled form and checks hs_jit_stats: every such launch ran compiled (jit) or none did
    (interpreter), nothing failed to compile, and at most `max_compiled` programs were produced."""

    def __init__(self, dev, jit: int, max_compiled: int = 1):
        self.dev, self.lib, self.jit, self.max_compiled = dev, dev._raw_lib, jit, max_compiled
        self.launches = 0

    def stats(self) -> list[int]:
        counters = (C.c_int32 * 4)()
        self.lib.hs_jit_stats(counters)
        return [int(counters[i]) for i in range(3)]  # programs compiled, compiled launches, compile failures

    def __enter__(self):
        self.before = self.stats()
        self.dev.reset_flags()
        self.lib.hs_jit_set_enabled(self.jit)
        return self

    def __exit__(self, exc_type, exc, tb):
        self.lib.hs_jit_set_enabled(1)
        if exc_type is not None:
            return False
        compiled, launched, failed = (now - was for now, was in zip(self.stats(), self.before))
        assert failed == 0, "a program failed to compile"
        assert launched == (self.launches if self.jit else 0), \
            f"{launched} compiled launches of {self.launches}: the {'compiled' if self.jit else 'interpreter'} form was not the one exercised"
        assert compiled <= (self.max_compiled if self.jit else 0), f"{compiled} programs compiled for one instruction shape"
        assert self.dev.read_flags() == 0
        return False

    def eval(self, cols: list, prog, n: int, n_outs: int, sel: np.ndarray | None = None, nrows_dev: int | None = None) -> np.ndarray:
        """hs_eval with n_outs boolean outputs -> [n_outs, n] bytes as the device left them (PREFILL where nothing wrote)."""
        import torch

        from minispark_amd import hipspark as hs

        dev = self.dev
        stride = (n + 15) // 16 * 16 + 16  # every output starts 16-byte aligned (the compiled form needs it)
        out = torch.full((n_outs * stride + 64,), PREFILL, dtype=torch.uint8, device=dev.device)
        assert out.data_ptr() % 16 == 0
        arr = (hs.hs_col * len(cols))(*cols)
        outs = (C.c_void_p * n_outs)(*[out.data_ptr() + o * stride for o in range(n_outs)])
        kinds = (C.c_int32 * n_outs)(*([hs.U8] * n_outs))
        d_sel = dev.to_device(sel.astype(np.int64), torch.int64) if sel is not None else None
        d_n = dev.to_device(np.array([nrows_dev], dtype=np.int64), torch.int64) if nrows_dev is not None else None
        hs.check(self.lib.hs_eval(dev.stream, arr, len(cols), C.byref(prog), d_sel.data_ptr() if d_sel is not None else None, n,
                                  d_n.data_ptr() if d_n is not None else None, outs, kinds, n_outs, dev.flags.data_ptr()),
                 "hs_eval")
        if sel is None:  # a row list always takes the interpreter kernel (hs_eval: the compiled form reads whole columns)
            self.launches += 1
        host = out.cpu().numpy()
        assert (host[n_outs * stride:] == PREFILL).all()
        got = host[: n_outs * stride].reshape(n_outs, stride)
        assert (got[:, n:] == PREFILL).all(), "a byte behind the last row was written"
        return got[:, :n]


def like_matrix(form: Form, col: Column, patterns: list[bytes]) -> np.ndarray:
    """[len(patterns), col.n] answers of the device, sixteen patterns per launch."""
    rows = []
    for block, own in blocks_of_16(patterns):
        got = form.eval([col.hs], like_program(block), col.n, 16)
        assert (got[own:] == got[0]).all(), "a repeated pattern answered differently"
        rows.append(got[:own])
    return np.concatenate(rows)


def want_like(strings: list[bytes], patterns: list[bytes]) -> np.ndarray:
    return np.array([[M.like(s.decode(), p.decode()) for s in strings] for p in patterns], dtype=np.uint8)


def assert_like(got: np.ndarray, strings: list[bytes], patterns: list[bytes], what: str) -> None:
    want = want_like(strings, patterns)
    assert set(np.unique(got).tolist()) <= {0, 1}, f"{what}: an output byte is neither 0 nor 1"
    bad = np.argwhere(got != want)
    newline = sum(1 for p, r in bad if strings[r].endswith(b"\n"))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} answers differ from the regex ({newline} of them on strings that "
                           f"end in a newline); first: " + ", ".join(f"{strings[r]!r} LIKE {patterns[p]!r} -> {got[p, r]}" for p, r in bad[:6]))


EX_STRINGS = [s.encode() for s in M.EXHAUSTIVE_STRINGS]
EX_PATTERNS = [p.encode() for p in M.EXHAUSTIVE_PATTERNS]


# ---- LIKE -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jit", FORMS)
def test_like_exhaustive_on_a_ragged_column(dev, jit):
    """121 strings over {a, b, newline} x 156 patterns over {a, b, %, _, newline}: 18,876 answers in ten launches of one
    instruction shape (patterns are literals: they do not enter the compiled program's identity)."""
    col = Column(dev, EX_STRINGS)
    assert len(blocks_of_16(EX_PATTERNS)) == 10
    with Form(dev, jit) as form:
        got = like_matrix(form, col, EX_PATTERNS)
        assert form.launches == 10
    assert got.shape == (156, 121)
    assert_like(got, EX_STRINGS, EX_PATTERNS, "ragged")


@pytest.mark.parametrize("jit", FORMS)
def test_like_exhaustive_on_fixed_width_columns(dev, jit):
    """The same strings grouped by length into fixed-width columns (fixed_len 0 .. 4, offs NULL)."""
    with Form(dev, jit) as form:
        for width in range(5):
            strings = [s for s in EX_STRINGS if len(s) == width]
            col = Column(dev, strings, fixed=width)
            assert_like(like_matrix(form, col, EX_PATTERNS), strings, EX_PATTERNS, f"fixed_len {width}")
        assert form.launches == 50


def alignment_grid(fill: bytes) -> list[bytes]:
    """Rows whose prefix sum puts a string 'a' * L, L = 0 .. 16, at every payload offset residue 0 .. 7 (136 of them), the
    rows between them runs of `fill` of the length that takes the offset there.  Every row is checked, the filler rows too; the
    last string ends on the payload's last byte."""
    rows: list[bytes] = []
    at = 0
    placed = set()
    for length in range(17):
        for residue in range(8):
            gap = (residue - at) % 8
            if gap:
                rows.append(fill * gap)
                at += gap
            placed.add((length, at % 8))
            rows.append(b"a" * length)
            at += length
    assert len(placed) == 136
    return rows


GRID_PATTERNS = ([b"a" * n for n in range(18)] + [b"_" * n for n in range(1, 18)] + [b"a" * n + b"_" for n in range(16)]
                 + [b"%a", b"a%", b"%b%", b"%b", b"b%", b"%", b"%_", b"_%a", b"%aa_", b"%a_a%", b"a%a", b"b%b", b"_b%", b"%ba%"])


@pytest.mark.parametrize("shift", [0, 1, 5, 7])
@pytest.mark.parametrize("jit", FORMS)
def test_like_register_path_at_every_start_alignment(dev, jit, shift):
    """hs_str_words16 assembles a string of <= 16 bytes from up to three aligned words by a funnel shift: every length at
    every start address modulo 8, with neighbours that change the answer if one of their bytes leaks in ('a' * L among 'a's
    against 'a' * L, '_' * L, 'a' * L + '_'; among 'b's against '%b%') or if one of the string's own is dropped.  The payload
    view starts 0, 1, 5 or 7 bytes into its buffer."""
    with Form(dev, jit) as form:
        for fill in (b"a", b"b"):
            strings = alignment_grid(fill)
            col = Column(dev, strings, shift=shift)
            assert (col.data.data_ptr() - shift) % 8 == 0
            assert_like(like_matrix(form, col, GRID_PATTERNS), strings, GRID_PATTERNS, f"grid among {fill!r}, shift {shift}")


LONG_STRINGS = [s.encode() for s in M.LONG_STRINGS]
LONG_PATTERNS = [p.encode() for p in M.LONG_PATTERNS]


@pytest.mark.parametrize("jit", FORMS)
def test_like_across_the_16_byte_boundary_and_on_long_strings(dev, jit):
    """LONG_CASES: lengths 15, 16, 17, 18, 24, 64, 255 - registers up to 16 bytes, memory beyond - with backtracking runs,
    interior newlines, one and two trailing newlines; as one ragged column and as fixed-width columns of 16, 17 and 255."""
    with Form(dev, jit) as form:
        col = Column(dev, LONG_STRINGS)
        assert_like(like_matrix(form, col, LONG_PATTERNS), LONG_STRINGS, LONG_PATTERNS, "ragged")
        for width in (16, 17, 255):
            strings = [s for s in LONG_STRINGS if len(s) == width]
            assert len(strings) >= 8
            col = Column(dev, strings, fixed=width)
            assert_like(like_matrix(form, col, LONG_PATTERNS), strings, LONG_PATTERNS, f"fixed_len {width}")
        # the same strings 1 byte into their buffer: the memory path reads bytes, the register path whole words
        col = Column(dev, LONG_STRINGS, shift=1)
        assert_like(like_matrix(form, col, LONG_PATTERNS), LONG_STRINGS, LONG_PATTERNS, "ragged, shift 1")


TAIL_PATTERNS = [b"", b"a", b"a%", b"_", b"%\n", b"%", b"%b", b"a_", b"\n", b"_\n", b"%a%", b"b%\n", b"__", b"%_", b"ab", b"a\n"]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 121])
@pytest.mark.parametrize("jit", FORMS)
def test_like_row_count_tails_and_row_lists(dev, jit, n):
    """The first n exhaustive strings: whole (the compiled form evaluates four rows per lane: n = 1, 3, 5, 121 end in a
    guarded quad), and through a row list that reverses them - output i is input sel[i]; a row list takes the interpreter
    kernel in either form."""
    strings = [s for s in EX_STRINGS if len(s) >= 1][:n] if n < 121 else EX_STRINGS  # (short prefixes of the list are all b'')
    assert len(strings) == n
    col = Column(dev, strings)
    prog = like_program(TAIL_PATTERNS)
    with Form(dev, jit) as form:
        got = form.eval([col.hs], prog, n, 16)
        assert_like(got, strings, TAIL_PATTERNS, f"n {n}")
        sel = np.arange(n)[::-1].copy()
        got = form.eval([col.hs], prog, n, 16, sel=sel)
        assert_like(got, [strings[i] for i in sel], TAIL_PATTERNS, f"n {n}, reversed row list")
        assert form.launches == 1


@pytest.mark.parametrize("count", [0, 1, 6, 7, 120, 121, 500])
@pytest.mark.parametrize("jit", FORMS)
def test_like_stops_at_the_device_row_count(dev, jit, count):
    """nrows_dev caps nrows: rows at or beyond it keep the byte the output held before the launch."""
    col = Column(dev, EX_STRINGS)
    with Form(dev, jit) as form:
        got = form.eval([col.hs], like_program(TAIL_PATTERNS), 121, 16, nrows_dev=count)
    live = min(count, 121)
    assert_like(got[:, :live], EX_STRINGS[:live], TAIL_PATTERNS, f"device count {count}")
    assert (got[:, live:] == PREFILL).all(), "a row at or beyond the device row count was written"


# ---- comparisons ------------------------------------------------------------------------------------------------
def want_cmp(left: list[bytes], right: list[bytes]) -> np.ndarray:
    return np.array([[M.cmp(a, b, code) for a, b in zip(left, right)] for code in M.CMP_CODES], dtype=np.uint8)


def assert_cmp(got: np.ndarray, left: list[bytes], right: list[bytes], what: str) -> None:
    want = want_cmp(left, right)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {want.size} answers differ from bytes order; first: "
                           + ", ".join(f"{left[r]!r} cmp{c} {right[r]!r} -> {got[c, r]}" for c, r in bad[:6]))


def literal_pairs() -> list[tuple[bytes, bytes]]:
    """Every distinct CMP_STRINGS entry as a literal, two per program (one instruction shape), paired longest with shortest so
    that the 255-byte literal shares its pool with the empty one and every pair fits HS_MAX_POOL."""
    lits = sorted(set(M.CMP_STRINGS), key=lambda s: (len(s), s))
    pairs = []
    while lits:
        short = lits.pop(0)
        long_ = lits.pop() if lits else short
        assert len(short) + len(long_) <= 256
        pairs.append((long_, short))
    assert len(pairs[0][0]) == 255 and pairs[0][1] == b""
    return pairs


@pytest.mark.parametrize("jit", FORMS)
def test_strcmp_lit_all_six_codes(dev, jit):
    """HS_OP_STRCMP_LIT, codes 0 .. 5, every CMP_STRINGS entry as the literal (the empty one and the 255-byte one in one
    program) against a ragged column of all of them and a fixed-width column of the 16-byte ones.  Bytes 0x80 .. 0xff order
    after 0x7f; a prefix orders first; a zero byte is a byte."""
    from minispark_amd import hipspark as hs

    code = []
    for lit in range(2):
        for cmp_code in M.CMP_CODES:
            code += [ins(hs.OP_STRCMP_LIT, 0, a=0, b=lit, c=cmp_code), ins(hs.OP_OUT, 1, a=lit * 6 + cmp_code)]
    ragged = Column(dev, M.CMP_STRINGS)
    sixteen = [s for s in M.CMP_STRINGS if len(s) == 16]
    assert len(sixteen) >= 5
    fixed = Column(dev, sixteen, fixed=16)
    with Form(dev, jit) as form:
        for pair in literal_pairs():
            prog = program(code, list(pair))
            for col in (ragged, fixed):
                got = form.eval([col.hs], prog, col.n, 12)
                for k, lit in enumerate(pair):
                    assert_cmp(got[6 * k: 6 * k + 6], col.strings, [lit] * col.n, f"literal {lit[:20]!r} ({len(lit)} bytes)")


def strcmp_col_program(a: int, b: int):
    from minispark_amd import hipspark as hs

    code = []
    for cmp_code in M.CMP_CODES:
        code += [ins(hs.OP_STRCMP_COL, 0, a=a, b=b, c=cmp_code), ins(hs.OP_OUT, 1, a=cmp_code)]
    return program(code, [])


@pytest.mark.parametrize("jit", FORMS)
def test_strcmp_col_all_six_codes(dev, jit):
    """HS_OP_STRCMP_COL over the cross product of CMP_STRINGS as two columns: ragged x ragged, fixed x ragged, ragged x
    fixed, fixed x fixed of different widths (and of one width), and a column compared with itself."""
    S = M.CMP_STRINGS
    prog = strcmp_col_program(0, 1)
    by_len = lambda n: [s for s in S if len(s) == n]  # noqa: E731
    with Form(dev, jit, max_compiled=2) as form:
        def check(left: list[bytes], right: list[bytes], fixed_left, fixed_right, what):
            a = [x for x in left for _ in right]
            b = [y for _ in left for y in right]
            ca, cb = Column(dev, a, fixed=fixed_left), Column(dev, b, fixed=fixed_right)
            assert_cmp(form.eval([ca.hs, cb.hs], prog, len(a), 6), a, b, what)

        check(S, S, None, None, "ragged x ragged")
        for width in (16, 255, 1, 0):
            check(by_len(width), S, width, None, f"fixed {width} x ragged")
        check(S, by_len(17), None, 17, "ragged x fixed 17")
        for wa, wb in ((16, 17), (17, 16), (8, 9), (1, 1), (0, 1), (255, 255), (16, 16)):
            assert by_len(wa) and by_len(wb)
            check(by_len(wa), by_len(wb), wa, wb, f"fixed {wa} x fixed {wb}")
        col = Column(dev, S)
        assert_cmp(form.eval([col.hs], strcmp_col_program(0, 0), col.n, 6), S, S, "a column with itself")


# ---- inside a fused scan ----------------------------------------------------------------------------------------
def scalar_scan(dev, lib, cols, n_cols: int, prog, units: list[int]):
    """hs_agg_scalar with two INTEGER sums over the row ranges `units` -> (out_acc [n_units, 2], out_rows, out_ngroups)."""
    import torch

    from minispark_amd import hipspark as hs

    n_units = len(units) - 1
    host_units = (C.c_int64 * len(units))(*units)
    geom = hs.hs_agg_geom()
    hs.check(lib.hs_agg_scalar_geom(host_units, n_units, 2, C.byref(geom)), "hs_agg_scalar_geom")
    chunks = np.zeros((max(int(geom.n_chunks), 1), 4), dtype=np.int64)
    chunk0 = np.zeros(n_units + 1, dtype=np.int64)
    hs.check(lib.hs_agg_partial_chunks(host_units, n_units, C.byref(geom), chunks.ctypes.data_as(C.POINTER(hs.hs_chunk)),
                                       chunk0.ctypes.data_as(C.POINTER(C.c_int64))), "hs_agg_partial_chunks")
    d_chunks, d_chunk0 = dev.to_device(chunks.reshape(-1)), dev.to_device(chunk0)
    ws = dev.workspace(geom.ws_bytes).zero_()
    spec = hs.hs_agg_spec()
    spec.n_acc = 2
    for a in range(2):
        spec.op[a], spec.is_int[a] = hs.AGG_SUM, 1
    acc = torch.zeros(n_units * 2 + 2, dtype=torch.int64, device=dev.device)
    rows = torch.full((n_units + 2,), -7, dtype=torch.int64, device=dev.device)
    rep = torch.full((n_units + 2,), -7, dtype=torch.int64, device=dev.device)
    ngroups = torch.full((n_units + 2,), -7, dtype=torch.int32, device=dev.device)
    hs.check(lib.hs_agg_scalar(dev.stream, cols, n_cols, C.byref(prog), C.byref(spec), d_chunks.data_ptr(), d_chunk0.data_ptr(),
                               n_units, C.byref(geom), acc.data_ptr(), rows.data_ptr(), rep.data_ptr(), ngroups.data_ptr(),
                               ws.data_ptr(), dev.flags.data_ptr(), None, None), "hs_agg_scalar")
    return (acc.cpu().numpy()[: n_units * 2].reshape(n_units, 2), rows.cpu().numpy()[:n_units], rep.cpu().numpy()[:n_units],
            ngroups.cpu().numpy()[:n_units])


@pytest.mark.parametrize("n,units", [(121, [0, 121]), (121, [0, 50, 121]), (120, [0, 120]), (3, [0, 3]), (121, [0, 1, 2, 7, 121])])
@pytest.mark.parametrize("jit", FORMS)
def test_like_as_the_filter_of_a_keyless_scan(dev, jit, n, units):
    """hs_agg_scalar: LIKE; HS_OP_FILTER; SUM(1); SUM(i32 column) - the quad interpreter's sink.live(j) arm and the
    generated `live ? ... : 0`.  Row counts that are and are not multiples of 4, units that start inside a row quad."""
    from minispark_amd import hipspark as hs

    strings = EX_STRINGS[121 - n:]  # the longest strings: the short prefix of the list is all but empty
    values = (np.arange(n, dtype=np.int64) * 7919 % 2003 - 1000).astype(np.int32)
    icol, keep = int_column(dev, values)
    scol = Column(dev, strings)
    cols = (hs.hs_col * 2)(icol, scol.hs)  # numeric slots first, strings after (as the lowering assigns them)
    code = [ins(hs.OP_LIKE, 0, a=1, b=0), ins(hs.OP_FILTER, 1), ins(hs.OP_LIT, 0, a=1), ins(hs.OP_AGG, 1, a=0),
            ins(hs.OP_LD, 0, a=0), ins(hs.OP_AGG, 1, a=1)]
    patterns = [b"a", b"a%", b"_", b"", b"%\n", b"%", b"%b\n"]
    with Form(dev, jit) as form:
        for pattern in patterns:
            acc, rows, rep, ngroups = scalar_scan(dev, form.lib, cols, 2, program(code, [pattern, 1]), units)
            form.launches += 1
            for u, (lo, hi) in enumerate(zip(units, units[1:])):
                hit = [r for r in range(lo, hi) if M.like(strings[r].decode(), pattern.decode())]
                what = f"pattern {pattern!r}, unit {u} rows {lo}..{hi}"
                assert int(rows[u]) == len(hit), what
                if hit:
                    assert (int(rep[u]), int(ngroups[u])) == (u, 1), what
                    assert acc[u].tolist() == [len(hit), int(values[hit].astype(np.int64).sum())], what
                else:
                    assert (int(rep[u]), int(ngroups[u])) == (-1, 0), what
    del keep


# ---- either side of the dictionary cap, through the engine ------------------------------------------------------------
CAP_SPECIALS = ["AIR", "AIR\n", "REG AIR\n", "\n", "", "x\ny"]
CAP_PATTERNS = ["AIR", "%AIR", "%AIR%", "_", "%", "", "x_y"]


def _cap_table(path, distinct: int, seed: int):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile, StrCol

    rng = random.Random(seed)
    words = CAP_SPECIALS + [f"w{i:03d}" + ("\n" if i % 5 == 0 else "") for i in range(distinct - len(CAP_SPECIALS))]
    n = 1200
    s = words + [rng.choice(words[: 12]) for _ in range(n - len(words))]  # every word once, the special ones often
    rng.shuffle(s)
    k = np.array([rng.randrange(5) for _ in range(n)], np.int32)
    assert len(set(s)) == distinct
    BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("s", T.STRING)],
                                     [[k[:500], StrCol.from_strings(s[:500])], [k[500:], StrCol.from_strings(s[500:])]])


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine(device=0) as e:
        yield e


@pytest.mark.parametrize("distinct", [40, 400])
def test_like_answers_do_not_depend_on_the_dictionary(engine, tmp_path, distinct):
    """The same strings in a column of 40 distinct values (dictionary-coded at table open: the host's regex decides) and of
    400 (plain: the device matcher decides), against the oracle."""
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from oracle.py_engine import run_query
    from tests.queries import api_namespace

    path = tmp_path / f"cap{distinct}.bin"
    _cap_table(path, distinct, seed=distinct)

    def queries(e):
        api = api_namespace(lambda: DataFrame(e), Col, Functions, Lit)
        for p in CAP_PATTERNS:
            yield p, "count", api.DataFrame().table(str(path)).filter(api.Col("s").like(p)).group_by(api.Col("k")).agg(api.F.count())
            yield p, "select", api.DataFrame().table(str(path)).filter(api.Col("s").like(p)).select(api.Col("s"))

    want = {(p, shape): run_query(frame.task) for p, shape, frame in queries(object())}
    assert sum(len(r) for r in want[("AIR", "select")]) > 0
    for p, shape, frame in queries(engine):
        assert_rows_match(frame.collect(), want[(p, shape)])
    table = engine._table(path)
    coded = [c.dict is not None for i, c in table.columns.items() if table.schema[i][0] == "s"]
    assert coded == [distinct <= 256], "the column did not land on the side of the dictionary cap this case is about"
