"""Model of the string predicates (no GPU, no torch): what LIKE and the six string comparisons must answer, and the
corpora the CPU tests (tests/test_string_predicates_cpu.py) and the GPU tests (tests/test_gpu_string_predicates.py) share.

LIKE is the reference's formula, verbatim (sql.py:178-179, 194; oracle/py_engine.py:72): the pattern is escaped, `%` becomes
`.*`, `_` becomes `.`, and `re.match("^...$", s)` decides.  Two properties of Python's regex follow and are part of the
contract: `.` does not match '\\n' (so `%` and `_` never cross a newline), and `$` also matches just before ONE trailing
'\\n' (so 'AIR\\n' LIKE 'AIR' is true).

String order is byte order (include/hipspark.h: STRING compares like memcmp, a prefix sorts first), which Python's `bytes`
implements; the compare codes are the header's: 0 lt, 1 le, 2 gt, 3 ge, 4 eq, 5 ne."""

from __future__ import annotations

import functools
import itertools
import random
import re

LT, LE, GT, GE, EQ, NE = range(6)
CMP_CODES = (LT, LE, GT, GE, EQ, NE)


@functools.lru_cache(maxsize=None)
def _regex(pattern: str) -> "re.Pattern[str]":
    return re.compile("^" + re.escape(pattern).replace("%", ".*").replace("_", ".") + "$")


def like(s: str, pattern: str) -> bool:
    return re.match(_regex(pattern), s) is not None


def cmp(a: bytes, b: bytes, code: int) -> bool:
    if code == LT:
        return a < b
    if code == LE:
        return a <= b
    if code == GT:
        return a > b
    if code == GE:
        return a >= b
    if code == EQ:
        return a == b
    if code == NE:
        return a != b
    raise ValueError(f"compare code {code}")


def like_loop(s: bytes, pattern: bytes) -> bool:
    """The device matcher (hs_like_impl in csrc/hs_device.h, like_match in oracle/q45_oracle.c) restated: one backtrack
    point, `_` and the run of a `%` refuse '\\n', anchored at both ends - the answer of a regex whose `$` matches at the
    very end only."""
    si = pi = 0
    star_p, star_s = -1, 0
    while si < len(s):
        if pi < len(pattern) and pattern[pi] == 0x25:  # '%'
            star_p, star_s = pi, si
            pi += 1
        elif pi < len(pattern) and ((pattern[pi] == 0x5F and s[si] != 0x0A) or (pattern[pi] != 0x5F and pattern[pi] == s[si])):
            pi += 1
            si += 1
        elif star_p >= 0 and s[star_s] != 0x0A:
            pi = star_p + 1
            star_s += 1
            si = star_s
        else:
            return False
    while pi < len(pattern) and pattern[pi] == 0x25:
        pi += 1
    return pi == len(pattern)


def like_repaired(s: bytes, pattern: bytes) -> bool:
    """The formula the kernel implements: the loop, and - only when it failed and the string ends in '\\n' - the loop once
    more without that byte (Python's `$` before one trailing newline)."""
    return like_loop(s, pattern) or (len(s) > 0 and s[-1] == 0x0A and like_loop(s[:-1], pattern))


def _words(alphabet: str, max_len: int) -> list[str]:
    return ["".join(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


EXHAUSTIVE_STRINGS = _words("ab\n", 4)      # 121
EXHAUSTIVE_PATTERNS = _words("ab%_\n", 3)   # 156
assert len(EXHAUSTIVE_STRINGS) == 121 and len(EXHAUSTIVE_PATTERNS) == 156

# ---- the 16 / 17 boundary (registers up to 16 bytes, memory beyond) and long strings ------------------------------
LONG_LENGTHS = (15, 16, 17, 18, 24, 64, 255)


def _long_strings(n: int) -> list[str]:
    half = n // 2
    out = [
        "a" * (n - 1) + "b",                               # the backtracking run
        "a" * (n - 2) + "b\n",                             # ... ending in the newline `$` forgives
        "a" * n,                                           # no b at all: every `%` runs to the end and fails
        "a" * (n - 3) + "b\n\n",                           # two trailing newlines: only one is forgiven
        "a" * half + "\n" + "a" * (n - half - 2) + "b",    # an interior newline `%` and `_` must not cross
        "a" * half + "\n" + "a" * (n - half - 3) + "b\n",  # ... with a trailing one
        ("ab" * n)[:n],                                    # alternating: every literal restarts the backtrack point
        ("ab" * n)[: n - 1] + "\n",
        "b" + "a" * (n - 2) + "\n",
        "\n" + "a" * (n - 2) + "b",                        # a leading newline
    ]
    assert all(len(s) == n for s in out)
    return out


LONG_STRINGS = [s for n in LONG_LENGTHS for s in _long_strings(n)]
# at most 12 bytes each; one pattern with four `%` (the reference's regex needs ~0.3 s for a 255-byte string it rejects,
# which bounds how many such patterns a quick test can afford)
LONG_PATTERNS = ["%a%a%a%b", "%ab", "a%_b", "%_", "%", "", "a%", "%b", "%\n", "%b\n", "a%\n%b", "%a\n%", "_%_", "%b_",
                 "a%b\n", "%\n\n", "%_\n", "b%", "\n%b", "a%ab", "%ba", "aaaaaaaaaaa%", "%aaaaaaaaab", "a%a\na%b",
                 "%aaaab\n", "_%\n_%", "ab%", "%ab\n", "a_%_b", "%a_", "__%", "%a%b%"]
assert len(LONG_PATTERNS) == 32 and all(len(p) <= 12 for p in LONG_PATTERNS)
LONG_CASES = [(s, p) for s in LONG_STRINGS for p in LONG_PATTERNS]
for _n in LONG_LENGTHS:  # every length with and without a trailing newline
    assert {s.endswith("\n") for s in LONG_STRINGS if len(s) == _n} == {True, False}

# ---- comparisons: byte strings, high bytes included (never routed through LIKE or StrCol.from_strings) ---------------


def _differ_at(pos: int, total: int) -> tuple[bytes, bytes]:
    """Two strings of `total` bytes that agree up to byte `pos` and differ there by 0x7f against 0x80 - the pair a signed
    byte compare orders the wrong way round; the bytes behind `pos` would decide the other way if they were looked at."""
    head = bytes((i * 7 + 1) & 0x7F or 1 for i in range(pos))
    return head + b"\x7f" + b"\xff" * (total - pos - 1), head + b"\x80" + b"\x00" * (total - pos - 1)


def _cmp_strings() -> list[bytes]:
    out = [b"", b"\x00", b"\x01", b"\x7f", b"\x80", b"\xff"]
    out += [b"a", b"ab", b"abc", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghijklmnop", b"abcdefghijklmnopq"]  # prefixes
    out += [b"\x00\x00", b"a\x00", b"ab\x00"]  # a zero byte is a byte: longer than, and after, its prefix
    for pos, total in ((0, 3), (7, 8), (7, 12), (8, 9), (8, 16), (15, 16), (15, 17), (16, 17), (16, 40), (254, 255)):
        out += _differ_at(pos, total)
    out += [b"x" * 255, b"x" * 254]
    out += [b"ab", b"abcdefgh", b"x" * 255, b"", b"\x80"]  # equal pairs: the cross product meets them off the diagonal too
    return out


CMP_STRINGS = _cmp_strings()
assert max(len(s) for s in CMP_STRINGS) == 255


def random_pairs(seed: int, count: int, max_len: int = 40) -> list[tuple[str, str]]:
    """Seeded (string, pattern) pairs over {a, b, newline} / {a, b, %, _, newline}: strings up to `max_len` bytes, patterns
    up to 6 - newlines and wildcards frequent enough that most pairs are decided late."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        s = "".join(rng.choice("aab\n") for _ in range(rng.randint(0, max_len)))
        if rng.random() < 0.3:
            s += "\n"
        p = "".join(rng.choice("ab%%_\n") for _ in range(rng.randint(0, 6)))
        out.append((s, p))
    return out
