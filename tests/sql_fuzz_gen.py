"""Random queries over the whole SQL language, each as a description for tests/sql_model.py AND as SQL text for the engine.

``random_query(seed, folder)`` -> (tables, description, sql_text).  Three tables with distinct column names, so a join
needs no alias: A (the FROM table), B (the inner join's right side) and C (the semi / anti join's right side: after an inner
join the left side already holds B's names, and a name both inputs hold is a ``ValueError`` of the semi join).  Each has

    id  unique, shuffled INTEGER            dk  dense INTEGER join key           sk  INTEGER over all of int32, with INT32_MIN,
    i   INTEGER in [-50, 50]                d   INTEGER, +-1 2 4 8: a divisor        INT32_MAX, 0 and -1 present
    f   FLOAT, k/8 in [-2, 2], 0.0 among    g   FLOAT, k/8 in [-1, 1], never 0    w   STRING, five values of three bytes
    s   STRING, hundreds of values of 0..20 bytes, '' among them                  t   TIMESTAMP 1969 - 2031, whole seconds

under the prefixes '', 'b_' and 'c_'.  ``w`` has one fixed length so that it may be part of a composite GROUP BY key with the
dictionaries on and off.

Exactness.  Every FLOAT is a small multiple of 1/8 and every divisor a power of two, so each expression value is a multiple
of 2^-gran with magnitude at most ``mag``; the generator tracks both and lets only expressions with mag * 2^gran <= 64 into
SUM / AVG (INTEGER: mag <= 10 000).  The largest input is 200 000 joined rows: 200 000 * 64 < 2^24, so every SUM, per-unit
partial and window prefix is an exact f32 (i32), and no summation order can change a bit.  AVG's one division is correctly
rounded whatever the order.  ``-0.0`` can arise from a product with a zero; such expressions stay out of MIN / MAX, whose
answer for a zero of both signs is documented as unspecified (known divergences).

Coverage by construction.  What must occur in every window of 64 seeds is drawn by ROTATION over the seed, not at random: the
query's shape and the one-row tables (seed mod 16; a one-row table sits under a row form without LIMIT that reads it - B and
C are joined there, the one-row A has no WHERE and no QUALIFY - so that what the engine makes of it is compared), the semi / anti join with its key kind and condition (seed mod 5 and the
block of five), the value of LIMIT, the number of window items, the window functions, frames, frame ends and spellings, the type
LAG / LEAD copy and the kind of COUNT(DISTINCT)'s argument.  FEATURES names each of them; tests/test_sql_fuzz_cpu.py asserts four
seeds for each and one for every pair of PAIRED.  Everything else is random.

Determinism by construction (sql_model.Result.determined): LIMIT 1 / 5 comes with ORDER BY keys that end in columns unique
over the result; a tie-sensitive window over grouped rows orders by all the group keys.

REFUSALS lists what the engine documents as refused and the generator therefore never writes.
"""

from __future__ import annotations

import random
from datetime import datetime, timedelta
from pathlib import Path

from tests import sql_model as M
from tests.sql_model import Agg, Bin, Case, Col, DatePart, DateTrunc, Join, Like, Lit, Query, Table, Win

# what DESIGN.md documents as refused, and how the generator stays clear of it
REFUSALS = [
    ("4.4", "ORDER BY / DISTINCT / window keys: at most HS_MAX_COLS (12) columns; DISTINCT over more than 12 result columns",
     "at most 12 result columns, at most 3 ORDER BY keys, at most 8 window key columns"),
    ("4.4", "ORDER BY, DISTINCT and window items over a result produced in block ranges (HIPSPARK_HBM_BUDGET)", "no budget is set"),
    ("4.4a", "mixing aggregates and plain columns without GROUP BY; arithmetic over aggregates", "aggregate-only select lists"),
    ("4.4a", "an aggregate without GROUP BY that reads more than 8 numeric columns among its filters and arguments (ExecutionError)",
     "filters, arguments and COUNT(DISTINCT) marks are counted; beyond 8 the WHERE, then the last aggregates, are left out"),
    ("4.4b", "CASE with STRING / TIMESTAMP / boolean branches; CASE nested beyond the stack depth; the simple form",
     "INTEGER / FLOAT branches, no CASE inside a CASE"),
    ("4.4c", "a FLOAT part; a STRING part with neither a dictionary nor one fixed length; a packed key wider than 16 bytes; "
     "an expression as a part; a column named twice", "parts from dk i d sk w t and date-part aliases, widths summed"),
    ("4.4d", "a date function over anything but a TIMESTAMP value; an unknown unit", "t and DATE_TRUNC(t) only"),
    ("4.4e", "COUNT(DISTINCT) next to a FLOAT or computed GROUP BY key; a STRING-valued or boolean argument expression",
     "no FLOAT keys at all; a STRING argument is a plain column"),
    ("4.4f", "RANK / DENSE_RANK without ORDER BY; a frame on a ranking function; more than 8 window items; window keys or "
     "arguments that are expressions or other window items", "at most 3 items over names of the un-windowed result"),
    ("4.4g", "a window aggregate over a STRING / TIMESTAMP column; a sum or prefix that leaves i32", "numeric arguments, bounded"),
    ("4.4h", "LAG / LEAD without k and default, a default of another type, a frame on LAG / LEAD / NTILE; a STRING argument",
     "k and a typed default always, INTEGER / FLOAT / TIMESTAMP arguments"),
    ("4.4i", "ROWS n PRECEDING without BETWEEN, an UNBOUNDED end next to a finite one, GROUPS, a RANGE of values",
     "ROWS BETWEEN (n PRECEDING | CURRENT ROW) AND (m FOLLOWING | CURRENT ROW) only"),
    ("4.4j", "a FLOAT or mixed-type key; a condition over left columns or both sides; a name both inputs hold; N ranks",
     "INTEGER = INTEGER or STRING = STRING, conditions over C's columns, table C after a join with B"),
    ("4.4e", "COUNT(DISTINCT e) where the text of e begins with '(' or '-': DISTINCT is then read as a function or a column "
     "(SemanticError 'Unsupported function: DISTINCT' / AssertionError 'COUNT takes no argument')",
     "the argument is written without outer parentheses and never begins with a negative literal"),
    ("4.5", "LIKE over a string expression (a concatenation): LoweringError 'LIKE is supported on plain string columns only'",
     "LIKE reads a STRING column"),
    ("parser", "NOT; decimal literals; GROUP BY a, b without parentheses; HAVING without GROUP BY; MIN / MAX / AVG calls in HAVING",
     "integer literals; HAVING names MIN / MAX by alias and calls COUNT / SUM / COUNT(DISTINCT)"),
]

W_VALUES = ["AIR", "RAI", "MAI", "SHP", "TRK"]
S_ALPHABET = "abAB_% -x"
S_PATTERNS = ["%a%", "a%", "%b", "_", "__%", "%", "%a_b%", "", "%-%", "%A%B%"]
BIG_SEEDS = tuple(range(1001, 1009))  # (no seed of the LIMIT 0 class among them)
SUM_FLOAT, SUM_INT, CELL_INT = 64, 10_000, 2_000_000_000
EPOCH_LO, EPOCH_HI = datetime(1969, 1, 1), datetime(2031, 12, 31)


class X:
    """an expression with what the generator knows about it"""

    def __init__(self, e, kind, mag=0.0, gran=0, nz=False, zero=True):
        self.e, self.kind, self.mag, self.gran, self.nz, self.zero = e, kind, mag, gran, nz, zero

    @property
    def summable(self) -> bool:
        if self.kind == M.FLOAT:
            return self.gran >= 0 and self.mag * (1 << self.gran) <= SUM_FLOAT
        return self.kind == M.INTEGER and self.mag <= SUM_INT


NOT_SUMMABLE = -1  # gran of a FLOAT that is no multiple of a power of two (an AVG)


def make_table(rng: random.Random, prefix: str, n: int, dense: int, sparse_pool: list, s_pool: list, t_pool: list) -> tuple:
    ids = list(range(n))
    rng.shuffle(ids)
    sparse = [rng.choice(sparse_pool) for _ in range(n)]
    for at, v in zip(rng.sample(range(n), min(n, 4)), (M.I32_MIN, M.I32_MAX, 0, -1)):
        sparse[at] = v
    columns = {
        "id": ids,
        "dk": [rng.randrange(dense) for _ in range(n)],
        "sk": sparse,
        "i": [rng.randint(-50, 50) for _ in range(n)],
        "d": [rng.choice([-4, -2, -1, 1, 2, 4, 8]) for _ in range(n)],
        "f": [rng.randint(-16, 16) / 8 for _ in range(n)],
        "g": [rng.choice([-1, 1]) * rng.randint(1, 8) / 8 for _ in range(n)],
        "w": [rng.choice(W_VALUES[:3] if prefix == "c_" else W_VALUES) for _ in range(n)],  # C: so that an anti join on w keeps rows
        "s": [rng.choice(s_pool) for _ in range(n)],
        "t": [rng.choice(t_pool) for _ in range(n)],
    }
    kinds = {"id": M.INTEGER, "dk": M.INTEGER, "sk": M.INTEGER, "i": M.INTEGER, "d": M.INTEGER, "f": M.FLOAT, "g": M.FLOAT,
             "w": M.STRING, "s": M.STRING, "t": M.TIMESTAMP}
    schema = [(prefix + name, kinds[name]) for name in columns]
    rows = [dict(zip([n for n, _ in schema], cells)) for cells in zip(*columns.values())]
    return schema, rows


def write_table(path: Path, table: Table) -> None:
    from oracle import blockfile

    code = {M.INTEGER: blockfile.INTEGER, M.STRING: blockfile.STRING, M.FLOAT: blockfile.FLOAT, M.TIMESTAMP: blockfile.TIMESTAMP}
    columns = [[r[name] for r in table.rows] for name, _ in table.schema]
    blockfile.write_blockfile(path, [(name, code[kind]) for name, kind in table.schema], columns, table.rows_per_block)


def make_tables(seed: int, folder: Path | None) -> dict:
    rng = random.Random(7_000_003 * (seed + 1))
    big = seed in BIG_SEEDS
    if big:
        sizes, blocks, dense = (40_000, 300, 300), (6, 2, 2), 100
    else:
        # the one-row tables by rotation over row-form classes that carry no LIMIT, so that every window of 64 seeds holds
        # four of each, READ by the query (random_query joins B / C there) and with an answer to compare
        c = seed % len(SHAPES)
        sizes = (1 if c == ONE_ROW["A"] else rng.choice([7] * 3 + [200] * 9 + [3000] * 12),
                 1 if c == ONE_ROW["B"] else rng.choice([50, 400]), 1 if c == ONE_ROW["C"] else rng.choice([50, 400]))
        blocks, dense = (rng.choice([1, 2, 5]), rng.choice([1, 3]), rng.choice([1, 3])), 40
    sparse_pool = [rng.randint(M.I32_MIN, M.I32_MAX) for _ in range(250)] + [M.I32_MIN, M.I32_MAX, 0, -1]
    s_pool = [""] + ["".join(rng.choice(S_ALPHABET) for _ in range(rng.randint(0, 20))) for _ in range(300)]
    span = int((EPOCH_HI - EPOCH_LO).total_seconds())
    t_pool = [EPOCH_LO + timedelta(seconds=rng.randrange(span)) for _ in range(150)]
    t_pool += [datetime(1969, 12, 28, 23, 59, 59), datetime(1970, 1, 1), datetime(2000, 2, 29, 12, 0, 0)]
    tables = {}
    for name, prefix, n, nblocks in zip("ABC", ("", "b_", "c_"), sizes, blocks):
        schema, rows = make_table(rng, prefix, n, dense + (5 if name != "A" else 0), sparse_pool, s_pool, t_pool)
        per = max(1, -(-n // nblocks) + (1 if nblocks > 1 and n > nblocks else 0))  # ragged: the last block is shorter
        tables[name] = Table(name, schema, rows, per, path=name)
        if folder is not None:
            tables[name].path = str(Path(folder) / f"{name}.bin")
            write_table(Path(tables[name].path), tables[name])
    return tables


# ---- expressions ----------------------------------------------------------------------------------------------------------
class Gen:
    def __init__(self, rng: random.Random, prefixes: tuple, old: bool = False) -> None:
        self.r, self.prefixes = rng, prefixes  # the tables whose columns are in scope
        self.old = old  # the language oracle/py_engine.py knows: no CASE, no date functions

    def col(self, name: str, prefix: str | None = None) -> X:
        p = self.r.choice(self.prefixes) if prefix is None else prefix
        info = {"id": (M.INTEGER, 40_000, 0, True), "dk": (M.INTEGER, 110, 0, True), "sk": (M.INTEGER, 1 << 31, 0, True),
                "i": (M.INTEGER, 50, 0, True), "d": (M.INTEGER, 8, 0, False), "f": (M.FLOAT, 2, 3, True),
                "g": (M.FLOAT, 1, 3, False), "w": (M.STRING, 0, 0, True), "s": (M.STRING, 0, 0, True),
                "t": (M.TIMESTAMP, 0, 0, True)}[name]
        return X(Col(p + name), info[0], info[1], info[2], False, info[3])

    def int_expr(self, depth: int = 0, limit: float = CELL_INT) -> X:
        r = self.r
        for _ in range(8):
            x = self._int_expr(depth)
            if x.mag <= limit:
                return x
        return self.col("i")

    def _int_expr(self, depth: int) -> X:
        r = self.r
        if depth >= 2 or r.random() < 0.4:
            pick = r.random()
            if pick < 0.7:
                return self.col(r.choice(["i", "i", "d", "dk", "id"]))
            if pick < 0.85:
                v = r.randint(-9, 9)
                return X(Lit(v), M.INTEGER, abs(v), 0, False, v == 0)
            return self.date_part() if not self.old else self.col("d")
        op = r.choice(["+", "-", "*", "*", "case"] if not self.old else ["+", "-", "*"])
        if op == "case":
            return self.case(self.int_expr(depth + 1), self.int_expr(depth + 1))
        a, b = self.int_expr(depth + 1), self.int_expr(depth + 1)
        if op == "*":
            return X(Bin("*", a.e, b.e), M.INTEGER, a.mag * b.mag, 0, False, a.zero or b.zero)
        return X(Bin(op, a.e, b.e), M.INTEGER, a.mag + b.mag, 0, False, True)

    def date_part(self) -> X:
        part = self.r.choice(M.DATE_PARTS)
        arg = self.ts_expr()
        return X(DatePart(part, arg.e), M.INTEGER, {"year": 2031, "dayofyear": 366}.get(part, 60), 0, False, part in ("hour", "minute", "second"))

    def ts_expr(self) -> X:
        t = self.col("t")
        if self.r.random() < 0.45 and not self.old:
            return X(DateTrunc(self.r.choice(M.TRUNC_UNITS + ("week", "week", "month")), t.e), M.TIMESTAMP)
        return t

    def case(self, a: X, b: X) -> X:
        kind = M.FLOAT if M.FLOAT in (a.kind, b.kind) else M.INTEGER
        return X(Case(self.cond(1, simple=True), a.e, b.e), kind, max(a.mag, b.mag), max(a.gran, b.gran), a.nz or b.nz,
                 a.zero or b.zero)

    def float_expr(self, depth: int = 0, summable: bool = False, no_nz: bool = False) -> X:
        for _ in range(12):
            x = self._float_expr(depth)
            if (x.summable or not summable) and not (no_nz and x.nz) and x.mag * (1 << x.gran) <= 1 << 20:
                return x
        return self.col("g")

    def _float_expr(self, depth: int) -> X:
        r = self.r
        if depth >= 2 or r.random() < 0.35:
            return self.col(r.choice(["f", "g"]))
        op = r.choice(["+", "-", "*", "mix", "/", "idiv", "case"] if not self.old else ["+", "-", "*", "mix", "/", "idiv"])
        a = self.float_expr(depth + 1)
        if op == "case":
            b = self.float_expr(depth + 1) if r.random() < 0.6 else self.int_expr(2, limit=60)
            return self.case(a, b) if r.random() < 0.5 else self.case(b, a)
        if op == "mix":  # INT op FLOAT promotes
            b = self.int_expr(2, limit=60)
            return X(Bin("*", a.e, b.e) if r.random() < 0.5 else Bin("*", b.e, a.e), M.FLOAT, a.mag * b.mag, a.gran,
                     a.nz or a.zero or b.zero, a.zero or b.zero)
        if op == "/":
            d = self.col("d")
            return X(Bin("/", a.e, d.e), M.FLOAT, a.mag, a.gran + 3, a.nz or a.zero, a.zero)
        if op == "idiv":  # INTEGER / INTEGER is FLOAT
            n, d = self.int_expr(2, limit=60), self.col("d")
            return X(Bin("/", n.e, d.e), M.FLOAT, n.mag, 3, n.zero, n.zero)
        b = self.float_expr(depth + 1)
        if op == "*":
            return X(Bin("*", a.e, b.e), M.FLOAT, a.mag * b.mag, a.gran + b.gran, a.nz or b.nz or a.zero or b.zero, a.zero or b.zero)
        return X(Bin(op, a.e, b.e), M.FLOAT, a.mag + b.mag, max(a.gran, b.gran), a.nz and (b.nz or op == "-"), True)

    def str_expr(self) -> X:
        r = self.r
        pick = r.random()
        if pick < 0.5:
            return self.col(r.choice(["s", "w"]))
        a, b = self.col(r.choice(["s", "w"])), self.col(r.choice(["s", "w"]))
        e = Bin("+", Bin("+", a.e, Lit(r.choice(["", "-", " / "]))), b.e) if pick < 0.8 else Bin("+", a.e, b.e)
        return X(e, M.STRING)

    def num_cond(self, simple: bool) -> object:
        r = self.r
        op = r.choice(["<", "<=", ">", ">=", "!=", "<", "<=", ">", ">=", "!=", "="])
        if simple and r.random() < 0.6:  # a column against a literal or its neighbour: true for a good share of the rows
            if r.random() < 0.6:
                return Bin(op, self.col(r.choice(["i", "d", "dk"])).e, Lit(r.choice([-8, -1, 0, 2, 5, 20])))
            return Bin(op, self.col("f").e, self.col("g").e)
        if r.random() < 0.5:
            a = self.int_expr(2 if simple else 1)
            b = self.int_expr(2) if r.random() < 0.5 else X(Lit(r.randint(-20, 20)), M.INTEGER)
        else:
            a, b = self.float_expr(2 if simple else 1), self.float_expr(2)
        if a.e == b.e:
            b = X(Lit(r.randint(-1, 1)), M.INTEGER)
        if not simple and r.random() < 0.3 and not self.old:  # CASE on either side of the comparison
            c = self.case(self.int_expr(2), self.int_expr(2))
            a, b = (c, b) if r.random() < 0.5 else (a, c)
        return Bin(op, a.e, b.e)

    def str_cond(self) -> object:
        r = self.r
        if r.random() < 0.5:
            arg = self.col("s").e if r.random() < 0.7 else next(n for n in _walk(self.str_expr().e) if isinstance(n, Col))
            return Like(arg, r.choice(S_PATTERNS if arg.name.endswith("s") else ["%A%", "_A_", "%I%", "S%", "%K", "%"]))  # (REFUSALS: a column, never the concatenation)
        if r.random() < 0.5:
            return Bin(r.choice(["=", "!=", "<", ">="]), self.col("w").e, Lit(r.choice(W_VALUES)))
        return Bin(r.choice(["<", "<=", ">", ">=", "!="]), self.col("s").e, Lit(r.choice(["", "a", "B", "_x", "ab"])))

    def ts_cond(self) -> object:
        r = self.r
        day = lambda lo=4_000, hi=19_000: (EPOCH_LO + timedelta(days=r.randrange(lo, hi))).strftime("%Y-%m-%d")  # noqa: E731
        t = self.col("t").e
        if r.random() < 0.5:
            lo, hi = day(0, 9_000), day(14_000, 23_000)
            return Bin("and", Bin(">=", t, Lit(lo)), Bin("<=", t, Lit(hi + " 12:30:00")))  # BETWEEN
        return Bin(r.choice(["<", "<=", ">", ">="]), self.ts_expr().e, Lit(day()))

    def part_cond(self) -> object:
        x = self.date_part()
        middle = {"year": 1999, "quarter": 2, "month": 6, "day": 15, "hour": 12, "minute": 30, "second": 30, "dayofweek": 3,
                  "dayofyear": 180}[x.e.part]
        return Bin(self.r.choice(["<", ">=", "!=", "<=", "="]), x.e, Lit(middle))

    def cond(self, depth: int = 0, simple: bool = False, kinds: tuple = ("num", "num", "str", "ts", "part")) -> object:
        r = self.r
        kind = r.choice(kinds if not self.old else [k for k in kinds if k != "part"])
        make = {"num": lambda: self.num_cond(simple), "str": self.str_cond, "ts": self.ts_cond,
                "part": self.part_cond}[kind]
        if simple or depth >= 1 or r.random() < 0.6:
            return make()
        # AND / OR over conditions of one kind: the engine types a comparison by its operands and refuses mixed kinds
        return Bin(r.choice(["and", "or", "or", "or"]), make(), make())


# ---- SQL text -------------------------------------------------------------------------------------------------------------
_OPS = {"=": "=", "!=": "!=", "<": "<", "<=": "<=", ">": ">", ">=": ">=", "+": "+", "-": "-", "*": "*", "/": "/"}


def sql_expr(e) -> str:
    if isinstance(e, Col):
        return e.name
    if isinstance(e, Lit):
        return f"'{e.value}'" if isinstance(e.value, str) else str(e.value)
    if isinstance(e, Like):
        return f"{sql_expr(e.arg)} LIKE '{e.pattern}'"
    if isinstance(e, Case):
        return f"CASE WHEN {sql_expr(e.cond)} THEN {sql_expr(e.then)} ELSE {sql_expr(e.other)} END"
    if isinstance(e, DatePart):
        return f"{e.part.upper()}({sql_expr(e.arg)})"
    if isinstance(e, DateTrunc):
        return f"DATE_TRUNC('{e.unit}', {sql_expr(e.arg)})"
    if isinstance(e, Agg):
        if e.kind == "count":
            return "COUNT()"
        return f"COUNT(DISTINCT {_bare(e.arg)})" if e.kind == "count_distinct" else f"{e.kind.upper()}({sql_expr(e.arg)})"
    assert isinstance(e, Bin), e
    if e.op in ("and", "or"):
        if (e.op == "and" and isinstance(e.left, Bin) and e.left.op == ">=" and isinstance(e.right, Bin) and e.right.op == "<="
                and e.left.left == e.right.left and isinstance(e.left.left, Col) and isinstance(e.left.right, Lit)
                and isinstance(e.left.right.value, str)):
            return f"{sql_expr(e.left.left)} BETWEEN {sql_expr(e.left.right)} AND {sql_expr(e.right.right)}"
        return f"({sql_expr(e.left)}) {e.op.upper()} ({sql_expr(e.right)})"
    if e.op in ("+", "-", "*", "/"):
        return f"({sql_expr(e.left)} {e.op} {sql_expr(e.right)})"
    return f"{sql_expr(e.left)} {_OPS[e.op]} {sql_expr(e.right)}"


def _bare(e) -> str:
    """an expression without its outer parentheses: ``COUNT(DISTINCT (a + b))`` reads a function called DISTINCT (REFUSALS)"""
    text = sql_expr(e)
    return text[1:-1] if isinstance(e, Bin) and e.op in ("+", "-", "*", "/") else text


def sql_window(w: Win, spelling: int) -> str:
    head = {"row_number": "ROW_NUMBER()", "rank": "RANK()", "dense_rank": "DENSE_RANK()", "count": "COUNT()",
            "ntile": f"NTILE({w.buckets})"}.get(w.kind)
    if head is None:
        if w.kind in ("lag", "lead"):
            default = f"'{w.default}'" if isinstance(w.default, str) else str(w.default)
            head = f"{w.kind.upper()}({w.arg}, {w.offset}, {default})"
        else:
            head = f"{w.kind.upper()}({w.arg})"
    parts = []
    if w.partition:
        parts.append("PARTITION BY " + ", ".join(w.partition))
    if w.order:
        parts.append("ORDER BY " + ", ".join(f"{n}{'' if asc and spelling % 2 else ' ASC' if asc else ' DESC'}" for n, asc in w.order))
    if isinstance(w.frame, tuple):
        lo = "CURRENT ROW" if w.frame[1] == 0 and spelling % 4 else f"{w.frame[1]} PRECEDING"
        hi = "CURRENT ROW" if w.frame[2] == 0 and spelling % 4 != 1 else f"{w.frame[2]} FOLLOWING"
        parts.append(f"ROWS BETWEEN {lo} AND {hi}")
    elif w.frame == "rows":
        parts.append(["ROWS UNBOUNDED PRECEDING", "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW",
                      "ROWS BETWEEN UNBOUNDED PRECEDING", "ROWS UNBOUNDED PRECEDING AND CURRENT ROW"][spelling % 4])
    elif w.frame in ("range", "partition") and spelling // 4:  # RANGE through the last peer: the default, spelled out
        parts.append(["RANGE UNBOUNDED PRECEDING", "RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"][spelling // 4 - 1])
    return f"{head} OVER ({' '.join(parts)}) AS {w.name}"


# ---- the query ------------------------------------------------------------------------------------------------------------
SHAPES = ("global", "group1", "groupn", "rows", "rows", "group1", "groupn", "rows", "groupn", "group1", "groupn", "rows", "rows",
          "group1", "groupn", "rows")
ONE_ROW = {"A": 7, "B": 15, "C": 4}  # table -> the seeds (mod 16) in which it has one row: row forms without a LIMIT
LIMIT_CLASS = {0: 8, 1: 0, 5: (2, 5, 11, 14), 1_000_000: (3, 6, 9, 12)}  # LIMIT value -> the seeds (mod 16) that carry it
# offsets of three rotations that share the seed (ROWS spelling, RANGE spelling, kind of frame): one of the settings under which
# every entry of FEATURES reaches four of seeds 0..63 - the rotations are not independent of each other, the offsets untangle them
OFFSETS = [1, 1, 1]
N_WINDOWS = (2, 3, 0, 3, 3, 3, 1, 3, 3, 3, 3, 2, 3, 3, 0, 3)  # window items by seed mod 16
FRAMED = ("sum", "avg", "min", "max", "count", "first_value", "last_value")
WINDOW_KINDS = ("row_number", "rank", "dense_rank", "sum", "avg", "min", "max", "count", "lag", "lead", "first_value", "last_value",
                "ntile")


def random_query(seed: int, folder: Path | None = None, old: bool = False) -> tuple:
    """``old``: only what the reference's language has - filters, projections, one inner join, GROUP BY on one column with SUM /
    MIN / MAX / AVG / COUNT and HAVING - so that oracle/py_engine.py can run the same text"""
    tables = make_tables(seed, folder)
    r = random.Random(seed)
    shape = SHAPES[seed % len(SHAPES)]
    if old:
        shape = "rows" if shape in ("rows", "global") else "group1"
    text: list[str] = []

    # joins
    joins, prefixes = [], ("",)
    rich = 0.25 if shape == "global" else 0.0  # the few queries without GROUP BY carry more of everything else
    klass = seed % 16
    if r.random() < 0.35 + rich or klass == ONE_ROW["B"] and not old:  # (the one-row B is joined)
        joins.append(Join("inner", "B", "dk", "b_dk"))
        prefixes = ("", "", "b_")
    if (seed % 5 < 2 or klass == ONE_ROW["C"]) and not old:  # by rotation: semi / anti x three key kinds x with / without a condition
        kind = ("semi", "anti")[seed % 5] if seed % 5 < 2 else ("anti", "semi")[seed // 16 % 2]  # (the one-row C is joined)
        combo = seed // 5 % 6
        key = ("dk", "sk", "w")[combo % 3]
        cond = None
        if combo >= 3:
            cond = Gen(r, ("c_",)).cond(1, simple=True, kinds=("str",) if key == "w" else ("num",))
        joins.append(Join(kind, "C", key, "c_" + key, cond))
    g = Gen(r, prefixes, old)
    from_text = f"FROM '{tables['A'].path}'"
    for j in joins:
        if j.kind == "inner":
            from_text += f" {r.choice(['JOIN', 'INNER JOIN', 'LEFT JOIN'])} '{tables['B'].path}' ON {j.left_key} = {j.right_key}"
        else:
            word = {"semi": r.choice(["SEMI JOIN", "LEFT SEMI JOIN"]), "anti": r.choice(["ANTI JOIN", "LEFT ANTI JOIN"])}[j.kind]
            on = f"{j.left_key} = {j.right_key}" if r.random() < 0.5 else f"{j.right_key} = {j.left_key}"
            from_text += f" {word} '{tables['C'].path}' ON {on}" + (f" AND {sql_expr(j.cond)}" if j.cond is not None else "")

    where = g.cond() if r.random() < 0.55 else None
    if klass == ONE_ROW["A"] and not old:
        where = None  # the one row of A reaches the answer: what the scan of a one-row table gives is compared

    # the result rows: name -> X, and the names that together are unique over them
    items: list[tuple[str, X]] = []
    select_text: list[str] = []
    group, key_items, aggs, having = None, [], [], None
    inner = any(j.kind == "inner" for j in joins)
    if shape == "rows":
        distinct = (r.random() < 0.4 or seed % 16 == 11) and not old  # (11: a LIMIT 5 that cuts what DISTINCT leaves)
        if distinct:
            pool = [g.col("w"), g.col("dk"), g.col("d"), g.col("i"), X(DatePart("year", g.col("t").e), M.INTEGER, 2031),
                    g.case(X(Lit(1), M.INTEGER, 1), X(Lit(0), M.INTEGER, 0)), g.col("g"),
                    X(DateTrunc(r.choice(["year", "quarter", "week"]), g.col("t").e), M.TIMESTAMP)]
            for n, x in enumerate(r.sample(pool, r.randint(1, 2))):
                items.append((x.e.name if isinstance(x.e, Col) else f"e{n}", x))
            unique: list | None = None  # every result column, window columns among them
        else:
            items.append(("id", g.col("id", "")))
            if inner:
                items.append(("b_id", g.col("id", "b_")))
            items.append((lambda x: (x.e.name, x))(g.col(r.choice(["w", "d", "dk"]))))  # something with ties to rank by
            if not old:
                items += [("t", g.col("t", "")), ("g", g.col("g", ""))]  # a cell of every type for LAG / LEAD to copy
            for n in range(r.randint(1, 4)):
                x = r.choice([g.int_expr, g.float_expr, g.str_expr, g.str_expr, g.ts_expr, g.date_part if not old else g.float_expr,
                              lambda: g.col(r.choice(["i", "f", "g", "w", "s", "t", "sk", "dk"]))])()
                name = x.e.name if isinstance(x.e, Col) else f"e{n}"
                if name not in [n_ for n_, _ in items]:
                    items.append((name, x))
            unique = ["id", "b_id"] if inner else ["id"]
        select_text = [name if isinstance(x.e, Col) and x.e.name == name else f"{sql_expr(x.e)} AS {name}" for name, x in items]
    else:
        distinct = (r.random() < 0.15 or shape == "global" and seed // 16 % 2 == 1) and not old
        if shape == "group1":
            keys = [r.choice(["dk", "i", "w", "s", "t", "t", "sk", "y", "y", "d"] if not old else ["dk", "i", "w", "s", "t", "sk", "d"])]
        elif shape == "groupn":
            while True:
                keys = r.sample(["dk", "i", "w", "t", "y", "d", "sk", "m"], r.randint(2, 3 if seed % 16 in LIMIT_CLASS[5] else 4))
                if sum({"t": 8, "w": 1, "m": 8}.get(k, 4) for k in keys) <= 16:
                    break
        else:
            keys = []
        key_x = {}
        for k in keys:
            if k == "y":
                part = r.choice(["year", "month", "dayofweek", "quarter", "hour"])
                key_x[k] = X(DatePart(part, Col("t")), M.INTEGER, 2031)
                key_items.append((k, key_x[k].e))
            elif k == "m":
                key_x[k] = X(DateTrunc(r.choice(["year", "month", "week"]), Col("t")), M.TIMESTAMP)
                key_items.append((k, key_x[k].e))
            else:
                key_x[k] = g.col(k, "")
        n_aggs = r.randint(1, 4)
        for n in range(n_aggs):
            kind = r.choice(["sum", "sum", "min", "max", "avg", "count", "count", "count_distinct", "count_distinct"][: 7 if old else 9])
            if shape == "global" and n == 0:
                kind = "count_distinct"
            name = f"a{n}"
            if kind == "count":
                if any(a.kind == "count" for a in aggs):
                    continue
                aggs.append(Agg("count", None, name))
                items.append((name, X(Col(name), M.INTEGER, 1)))
                continue
            if kind == "count_distinct":
                while True:  # the argument's kind by rotation: INTEGER, FLOAT, STRING, date part
                    x = [lambda: g.int_expr(1) if r.random() < 0.5 else g.col(r.choice(["dk", "sk", "i"])),
                         lambda: g.float_expr(1) if r.random() < 0.6 else g.col("f"), lambda: g.col(r.choice(["s", "w"])),
                         g.date_part][(seed + n) % 4]()
                    if isinstance(x.e, Case) or (seed + n) % 4 == 0 and x.kind != M.INTEGER:
                        continue
                    if _bare(x.e)[0] not in "(-":  # (REFUSALS: the parser reads DISTINCT as a name there)
                        break
                aggs.append(Agg(kind, x.e, name))
                items.append((name, X(Col(name), M.INTEGER, 1)))
                continue
            if shape == "global" and n == 1:
                x = g.case(g.int_expr(2, limit=60), g.int_expr(2, limit=60))
            elif r.random() < 0.5:
                x = g.int_expr(0, limit=SUM_INT if kind in ("sum", "avg") else CELL_INT)
                if kind in ("min", "max") and r.random() < 0.3:
                    x = g.col("sk")
            else:
                x = g.float_expr(0, summable=kind in ("sum", "avg"), no_nz=kind in ("min", "max"))
            aggs.append(Agg(kind, x.e, name))
            out = X(Col(name), M.FLOAT if kind == "avg" else x.kind, x.mag, NOT_SUMMABLE if kind == "avg" else x.gran, x.nz)
            items.append((name, out))
        if shape == "global":  # REFUSALS 4.4a: the fused scan holds 8 column slots: filters, arguments and COUNT(DISTINCT) marks
            def slots() -> int:
                read = {n.name for e in [where] + [a.arg for a in aggs] if e is not None for n in _walk(e) if isinstance(n, Col)}
                return len(read) + sum(a.kind == "count_distinct" for a in aggs)

            if slots() > 8:
                where = None
            while slots() > 8:
                items = [it for it in items if it[0] != aggs[-1].name]
                aggs.pop()
        for k in reversed(keys):
            items.insert(0, (k, X(Col(k), key_x[k].kind, key_x[k].mag)))
        select_text = [f"{sql_expr(key_x[k].e)} AS {k}" if k in dict(key_items) else k for k in keys]
        select_text += [f"{sql_expr(a)} AS {a.name}" for a in aggs]
        if keys and r.random() < 0.5:
            pick = r.random() if not old else r.choice([0.1, 0.7, 0.9])
            if pick < 0.35 or not aggs:
                extra = Agg("count", None, "_having_count")
                hidden = [extra] if not any(a.kind == "count" for a in aggs) else []
                name = next((a.name for a in aggs if a.kind == "count"), "_having_count")
                having, having_text = Bin(">=", Col(name), Lit(r.choice([1, 2, 2]))), "COUNT() >= "
                having_text += str(having.right.value)
            elif pick < 0.65:
                x = r.choice([g.col("dk"), g.col("i"), g.col("w"), g.date_part(), g.col("sk")])
                extra = Agg("count_distinct", x.e, "_having_cd")
                hidden = [extra]
                having = Bin(r.choice([">", ">=", ">="]), Col("_having_cd"), Lit(1))
                having_text = f"COUNT(DISTINCT {_bare(x.e)}) {having.op} 1"
            elif pick < 0.85:
                x = r.choice([g.col("i"), X(Bin("*", g.col("i").e, g.col("d").e), M.INTEGER), X(Bin("-", g.col("i").e, g.col("d").e), M.INTEGER)])
                hidden = [Agg("sum", x.e, "_having_sum")]
                having = Bin(r.choice(["<", ">="]), Col("_having_sum"), Lit(r.choice([0, 0, 10, -10])))
                having_text = f"SUM({sql_expr(x.e)}) {having.op} {having.right.value}"
            else:
                a = r.choice(aggs)
                hidden = []
                having = Bin(r.choice(["<", ">=", "!="]), Col(a.name), Lit(r.choice([0, 1, 2])))
                having_text = f"{a.name} {having.op} {having.right.value}"
            aggs_all = aggs + hidden
        else:
            having_text, aggs_all = None, list(aggs)
        group = tuple(keys)
        unique = list(keys)

    # window items over the names of the result
    windows, spellings = [], []
    names = [n for n, _ in items]
    info = dict(items)
    numeric = [n for n in names if info[n].kind in (M.INTEGER, M.FLOAT)]
    n_windows = 0 if old or not numeric else N_WINDOWS[seed % 16]
    if shape == "rows" and distinct:
        n_windows = min(n_windows, 3 - len(items))  # at most three columns: ORDER BY can name them all, so LIMIT may cut
    coarse = [n for n, x in items if isinstance(x.e, (Col, DatePart)) and x.e != Col("id") and x.e != Col("b_id")
              and x.kind != M.FLOAT and (group is None or len(group) > 1 or n not in group)]
    specs = []
    for n in range(n_windows):
        if specs and (len(specs) == 2 or n != 1):  # the second item brings the second spec
            partition, order = r.choice(specs)
        else:
            partition = tuple(r.sample(names, r.choice([0, 1, 1, 2]) if len(names) > 1 else 0))
            rest = [k for k in names if k not in partition]
            order = tuple((k, r.random() < 0.6) for k in r.sample(rest, min(len(rest), r.choice([0, 1, 1, 2]))))
            specs.append((partition, order))
        # the first two by rotation, so that a window of consecutive seeds holds every function
        kind = (WINDOW_KINDS[seed % 13], FRAMED[(seed - seed // 8) % 7],
                (FRAMED + ("rank", "dense_rank", "row_number", "ntile", "rank"))[seed // 3 % 12])[n]
        if n == 2 and shape == "rows" and not distinct:  # the row form holds a cell of every type: LAG / LEAD copy them in turn
            kind = ("lag", "lead")[seed // 16 % 2]
        frame, arg, offset, default, buckets = None, None, None, None, None
        if kind in ("sum", "avg"):
            args = [c for c in numeric if info[c].summable]
            if not args:
                kind = "count"
            else:
                arg = r.choice(args)
        if kind in ("min", "max"):
            args = [c for c in numeric if not info[c].nz]
            arg = r.choice(args) if args else None
            kind = kind if args else "count"
        if kind in ("lag", "lead", "first_value", "last_value"):
            arg = r.choice([c for c in names if info[c].kind in (M.INTEGER, M.FLOAT, M.TIMESTAMP)])
        if kind in ("lag", "lead"):
            for wanted in ((M.TIMESTAMP, M.FLOAT, M.INTEGER), (M.FLOAT, M.TIMESTAMP, M.INTEGER),
                           (M.INTEGER, M.FLOAT, M.TIMESTAMP))[(seed + seed // 16 + n) % 3]:  # a default of each type, by rotation
                if any(info[c].kind == wanted for c in names):
                    arg = next(c for c in names if info[c].kind == wanted)
                    break
            offset = r.choice([0, 1, 1, 2, 5])
            default = {M.INTEGER: r.choice([0, -1, 77]), M.FLOAT: r.choice([-1.5, 2.5, 0.125]),
                       M.TIMESTAMP: r.choice(["1970-01-01", "2001-02-03 04:05:06"])}[info[arg].kind]
        if kind == "ntile":
            buckets = r.choice([1, 2, 3, 7, 100])
        if kind in ("rank", "dense_rank") and (not order or coarse):  # peers, so that the two differ
            few = [k for k in coarse if info[k].mag <= 1 or group is None or k in group] or coarse or names  # columns with ties
            order = ((r.choice(few), r.random() < 0.5),)
            others = [k for k in few if k != order[0][0]]
            partition = (r.choice(others),) if others and group is None and r.random() < 0.5 else ()
            specs.append((partition, order))
        if kind in ("sum", "avg", "min", "max", "count", "first_value", "last_value"):
            idx = seed * 3 + n  # the frame, its ends and its spelling by rotation over the items
            pick = (idx + OFFSETS[2]) % 4
            if pick in (0, 2):
                frame = ("between", (0, 1, 2, 7, 0)[idx // 2 % 5], (0, 1, 2, 7, 0)[(idx // 2 + idx // 10) % 5])
            elif pick == 1:
                frame = "rows"
            else:
                frame = "range" if order else "partition"
        sensitive = kind in M.TIE_SENSITIVE or frame == "rows" or isinstance(frame, tuple)
        if group is not None and sensitive:  # grouped rows come in no order: all the keys decide
            have = [k for k, _ in order]
            order = order + tuple((k, r.random() < 0.5) for k in group if k not in have and k not in partition)
            if frame == "partition" and order:
                frame = "range"  # no frame clause behind an ORDER BY: through the last peer
        windows.append(Win(kind, f"w{n}", arg, partition, order, frame, offset, default, buckets))
        spellings.append((seed // 4 + n + OFFSETS[0]) % 4 + 4 * ((seed // 2 + seed // 16 + n + OFFSETS[1]) % 3))
    window_text = [sql_window(w, s) for w, s in zip(windows, spellings)]

    qualify = None
    if windows and klass != ONE_ROW["A"] and seed % 3 == 0:  # by rotation
        counting = [w for w in windows if w.kind in ("row_number", "rank", "dense_rank", "ntile", "count")]
        w = r.choice(counting or windows)  # a condition that drops rows, where there is one
        if w.kind in ("row_number", "rank", "dense_rank", "ntile", "count"):
            qualify = Bin(r.choice(["<=", "<=", ">=", "!="]), Col(w.name), Lit(r.choice([2, 2, 3])))
        elif w.arg is not None and info[w.arg].kind != M.TIMESTAMP:
            qualify = Bin(r.choice([">=", "!=", "!="]), Col(w.name), Lit(r.choice([0, 0, -1])))
            if w.kind in ("sum", "min", "max", "avg") and info[w.arg].kind == M.INTEGER and info[w.arg].mag <= 1:
                qualify = Bin(">=", Col(w.name), Lit(1))  # over a count
        else:
            qualify = Bin(r.choice(["<", ">="]), Col(w.name), Lit("2001-01-01"))

    all_names = names + [w.name for w in windows]
    if unique is None:
        unique = list(all_names)
    order_by: tuple = ()
    limit = None
    if r.random() < 0.5 + rich and not old:
        order_by = tuple((k, r.random() < 0.6) for k in r.sample(all_names, min(len(all_names), r.randint(1, 3))))
    limit = next((v for v, at in LIMIT_CLASS.items() if seed % 16 == at or isinstance(at, tuple) and seed % 16 in at), None)
    if old:
        limit = None
    if limit is not None:  # by rotation: every value of LIMIT in four seeds of sixteen... of 64
        if not order_by:
            order_by = tuple((k, r.random() < 0.6) for k in r.sample(all_names, min(len(all_names), r.randint(1, 3))))
        if limit in (1, 5) and shape != "global":
            if len(unique) > 3:
                limit = 1_000_000
            else:
                head = [(k, asc) for k, asc in order_by if k not in unique][: 3 - len(unique)]
                order_by = tuple(head) + tuple((k, r.random() < 0.5) for k in unique)

    if group is None:
        q = Query("A", tuple(joins), where, tuple((n, x.e) for n, x in items), None, (), (), None, tuple(windows), qualify,
                  distinct, order_by, limit)
    else:
        q = Query("A", tuple(joins), where, tuple(names), group, tuple(key_items), tuple(aggs_all), having, tuple(windows),
                  qualify, distinct, order_by, limit)
    sql = f"SELECT {'DISTINCT ' if distinct else ''}{', '.join(select_text + window_text)} {from_text}"
    if where is not None:
        sql += f" WHERE {sql_expr(where)}"
    if group:
        sql += f" GROUP BY {group[0]}" if len(group) == 1 and r.random() < 0.7 else f" GROUP BY ({', '.join(group)})"
        if having is not None:
            sql += f" HAVING {having_text}"
    if qualify is not None:
        sql += f" QUALIFY {sql_expr(qualify)}"
    if order_by:
        sql += " ORDER BY " + ", ".join(f"{k}{'' if asc and r.random() < 0.5 else ' ASC' if asc else ' DESC'}" for k, asc in order_by)
    if limit is not None:
        sql += f" LIMIT {limit}"
    return tables, q, sql + ";"


# ---- what a query exercises -------------------------------------------------------------------------------------------------
def _walk(e):
    yield e
    for f in ("left", "right", "arg", "cond", "then", "other"):
        child = getattr(e, f, None)
        if child is not None and not isinstance(child, (str, int, float)):
            yield from _walk(child)


def _kind_of(e) -> str:
    """of a COUNT(DISTINCT) argument, from its shape"""
    if isinstance(e, DatePart):
        return "date part"
    names = [n.name for n in _walk(e) if isinstance(n, Col)]
    if isinstance(e, Col) and e.name.endswith(("s", "w")):
        return "STRING"
    floaty = any(n.endswith(("f", "g")) for n in names) or any(isinstance(n, Bin) and n.op == "/" for n in _walk(e))
    return "FLOAT" if floaty else "INTEGER"


def features(q: Query, sql: str, tables: dict | None = None) -> set:
    import re

    out = set()
    read = {"A"} | {j.table for j in q.joins}
    for name, table in (tables or {}).items():
        if len(table.rows) == 1 and name in read:  # a table the query reads
            out.add(f"{name} of one row")
    for a in q.aggs:
        if a.kind == "count_distinct" and not a.name.startswith("_having"):
            out.add("COUNT(DISTINCT) of " + _kind_of(a.arg))
    for j in q.joins:
        if j.kind != "inner":
            out.add(f"semi key {j.left_key} {'with' if j.cond is not None else 'without'} condition")
    if q.limit is not None:
        out.add("LIMIT " + {0: "0", 1: "1", 5: "5"}.get(q.limit, "beyond the rows"))
    for w in q.windows:
        if w.kind in ("lag", "lead"):
            out.add("default " + ("TIMESTAMP" if isinstance(w.default, str) else "FLOAT" if isinstance(w.default, float) else "INTEGER"))
        if isinstance(w.frame, tuple):
            out.add(f"sliding n={w.frame[1]}")
            out.add(f"sliding m={w.frame[2]}")
    for text in SPELLINGS:
        if re.search(SPELLINGS[text], sql):
            out.add(text)
    exprs = [q.where] + [j.cond for j in q.joins] + [a.arg for a in q.aggs] + [e for _, e in q.key_items] + [q.having, q.qualify]
    if q.group is None:
        exprs += [e for _, e in q.select]
    nodes = [n for e in exprs if e is not None for n in _walk(e)]
    for j in q.joins:
        out.add("inner join" if j.kind == "inner" else "semi/anti join")
        if j.kind != "inner":
            out.add(j.kind)
            out.add({"dk": "semi key dense", "sk": "semi key sparse", "w": "semi key string"}[j.left_key])
            out.add("semi with condition" if j.cond is not None else "semi without condition")
    if q.where is not None:
        out.add("where")
    if any(isinstance(n, Case) for n in nodes):
        out.add("CASE")
    if any(isinstance(n, (DatePart, DateTrunc)) for n in nodes):
        out.add("date part")
    if any(isinstance(n, DateTrunc) for n in nodes):
        out.add("DATE_TRUNC")
    if any(isinstance(n, Like) for n in nodes):
        out.add("LIKE")
    if " BETWEEN '" in sql:
        out.add("BETWEEN")
    if any(isinstance(n, Bin) and n.op == "+" and isinstance(n.right, Col) and n.right.name.endswith(("s", "w")) for n in nodes):
        out.add("concat")
    if q.where is not None and any(isinstance(n, Case) for n in _walk(q.where)):
        out.add("CASE in WHERE")
    if q.group is None:
        out.add("row form")
    elif not q.group:
        out.add("global aggregate")
    else:
        out.add("multi-key GROUP BY" if len(q.group) > 1 else "single-key GROUP BY")
        if q.key_items:
            out.add("date-part key")
        if "w" in q.group:
            out.add("coded string key")
        if "t" in q.group:
            out.add("timestamp key")
    for a in q.aggs:
        if not a.name.startswith("_having"):
            out.add({"count_distinct": "COUNT(DISTINCT)"}.get(a.kind, a.kind.upper()))
        if a.arg is not None and any(isinstance(n, Case) for n in _walk(a.arg)):
            out.add("CASE in aggregate")
    if q.having is not None:
        out.add("HAVING")
        if any(a.name == "_having_cd" for a in q.aggs):
            out.add("HAVING COUNT(DISTINCT)")
            out.add("COUNT(DISTINCT)")
    for w in q.windows:
        out.add("window item")
        out.add("window " + w.kind)
        if isinstance(w.frame, tuple):
            out.add("sliding frame")
        elif w.frame is not None:
            out.add("frame " + w.frame)
        if any(not asc for _, asc in w.order):
            out.add("window DESC")
    if len({(w.partition, w.order) for w in q.windows}) > 1:
        out.add("two window specs")
    if q.qualify is not None:
        out.add("QUALIFY")
    if q.distinct:
        out.add("DISTINCT")
    if q.order_by:
        out.add("ORDER BY")
        if any(not asc for _, asc in q.order_by):
            out.add("ORDER BY DESC")
    if q.limit is not None:
        out.add("LIMIT")
        if q.order_by:
            out.add("ORDER BY + LIMIT")
    return out


SPELLINGS = {
    "ROWS UNBOUNDED PRECEDING": r"[( ]ROWS UNBOUNDED PRECEDING\)",
    "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": r"[( ]ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW\)",
    "ROWS BETWEEN UNBOUNDED PRECEDING": r"[( ]ROWS BETWEEN UNBOUNDED PRECEDING\)",
    "ROWS UNBOUNDED PRECEDING AND CURRENT ROW": r"[( ]ROWS UNBOUNDED PRECEDING AND CURRENT ROW\)",
    "RANGE UNBOUNDED PRECEDING": r"[( ]RANGE UNBOUNDED PRECEDING\)",
    "RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": r"[( ]RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW\)",
    "no frame clause behind ORDER BY": r"(SUM|AVG|MIN|MAX|COUNT|FIRST_VALUE|LAST_VALUE)\([a-z_0-9]*\) OVER \([^)]*(ASC|DESC|ORDER BY [a-z_0-9, ]*)\)",
    "CURRENT ROW as the lower end": r"ROWS BETWEEN CURRENT ROW AND ",
    "CURRENT ROW as the upper end": r"ROWS BETWEEN (\d+ PRECEDING|CURRENT ROW) AND CURRENT ROW\)",
    "0 PRECEDING / 0 FOLLOWING": r"BETWEEN 0 PRECEDING|AND 0 FOLLOWING",
}
FEATURES = (
    "A of one row", "B of one row", "C of one row", "LIMIT 0", "LIMIT 1", "LIMIT 5", "LIMIT beyond the rows",
    "default INTEGER", "default FLOAT", "default TIMESTAMP", "sliding n=0", "sliding n=1", "sliding n=2", "sliding n=7",
    "sliding m=0", "sliding m=1", "sliding m=2", "sliding m=7", "sliding frame wider than its partition", *SPELLINGS,
    "COUNT(DISTINCT) of INTEGER", "COUNT(DISTINCT) of FLOAT", "COUNT(DISTINCT) of STRING", "COUNT(DISTINCT) of date part",
    "semi key dk with condition", "semi key dk without condition", "semi key sk with condition", "semi key sk without condition",
    "semi key w with condition", "semi key w without condition",
    "inner join", "semi", "anti", "semi key dense", "semi key sparse", "semi key string", "semi with condition",
    "semi without condition", "where", "CASE", "CASE in WHERE", "CASE in aggregate", "date part", "DATE_TRUNC", "LIKE", "BETWEEN",
    "concat", "row form", "global aggregate", "single-key GROUP BY", "multi-key GROUP BY", "date-part key", "coded string key",
    "timestamp key", "SUM", "MIN", "MAX", "AVG", "COUNT", "COUNT(DISTINCT)", "HAVING", "HAVING COUNT(DISTINCT)", "window item",
    "window row_number", "window rank", "window dense_rank", "window sum", "window avg", "window min", "window max", "window count",
    "window lag", "window lead", "window first_value", "window last_value", "window ntile", "sliding frame", "frame rows",
    "frame range", "frame partition", "window DESC", "two window specs", "QUALIFY", "DISTINCT", "ORDER BY", "ORDER BY DESC", "LIMIT",
    "ORDER BY + LIMIT",
)
PAIRED = ("inner join", "semi/anti join", "multi-key GROUP BY", "global aggregate", "COUNT(DISTINCT)", "CASE", "date part",
          "window item", "QUALIFY", "DISTINCT", "ORDER BY + LIMIT")
EXCLUSIVE = {frozenset(("multi-key GROUP BY", "global aggregate"))}  # the pairs the language does not allow
