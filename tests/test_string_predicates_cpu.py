"""String predicates without a GPU: the formula the device matcher implements (tests/string_predicate_model.py restates
the loop of csrc/hs_device.h) against the reference's regex, and the C oracle's copy of that loop against the same model."""

from __future__ import annotations

import numpy as np

from tests import string_predicate_model as M


def test_corpora_have_the_shapes_the_gpu_tests_rely_on():
    assert len(set(M.EXHAUSTIVE_STRINGS)) == 121 and len(set(M.EXHAUSTIVE_PATTERNS)) == 156
    assert {len(s) for s in M.LONG_STRINGS} == set(M.LONG_LENGTHS)
    assert all(set(s) <= set("ab\n") for s in M.LONG_STRINGS)
    for n in (0, 7, 8, 15, 16, 254):  # pairs that first differ at these bytes
        assert any(len(a) > n and len(b) > n and a[:n] == b[:n] and a[n] != b[n]
                   for a in M.CMP_STRINGS for b in M.CMP_STRINGS), n
    assert any(a != b and b.startswith(a) for a in M.CMP_STRINGS for b in M.CMP_STRINGS)
    assert len(M.CMP_STRINGS) > len(set(M.CMP_STRINGS))  # equal pairs off the diagonal


def test_model_knows_pythons_anchor_and_dot():
    for s, p in [("AIR\n", "AIR"), ("ab\n", "a%"), ("a\n", "_"), ("\n", ""), ("AIR\n", "%AIR%"), ("\n", "%")]:
        assert M.like(s, p), (s, p)
    for s, p in [("AIR\n\n", "AIR"), ("\n", "_"), ("a\nb", "a%b"), ("a\nb", "a_b"), ("\n\n", ""), ("\nAIR", "AIR"),
                 ("a.c", "abc"), ("abc", "a.c")]:
        assert not M.like(s, p), (s, p)
    assert M.like("a\nb", "a\nb") and M.like("a.c", "a.c") and M.like("a\nb", "a%\n%b")


def test_compare_model_is_unsigned_byte_order():
    assert M.cmp(b"\x7f", b"\x80", M.LT) and M.cmp(b"", b"\x00", M.LT) and M.cmp(b"a", b"a\x00", M.LT)
    for a in M.CMP_STRINGS[:12]:
        for b in M.CMP_STRINGS[:12]:
            d = (a > b) - (a < b)
            assert [M.cmp(a, b, c) for c in M.CMP_CODES] == [d < 0, d <= 0, d > 0, d >= 0, d == 0, d != 0]


def test_the_loop_alone_misses_exactly_the_trailing_newline():
    """The loop without the second run (the matcher as it stood) disagrees with the regex on 619 of the 18,876 exhaustive
    pairs, every one a string ending in a newline: what the GPU tests must see fail on an unrepaired library."""
    wrong = [(s, p) for s in M.EXHAUSTIVE_STRINGS for p in M.EXHAUSTIVE_PATTERNS
             if M.like_loop(s.encode(), p.encode()) != M.like(s, p)]
    assert len(wrong) == 619 and all(s.endswith("\n") for s, _ in wrong)
    assert all(M.like(s, p) for s, p in wrong)  # the loop only ever says false where the regex says true


def test_the_repaired_formula_is_the_regex():
    for s in M.EXHAUSTIVE_STRINGS:
        bs = s.encode()
        for p in M.EXHAUSTIVE_PATTERNS:
            assert M.like_repaired(bs, p.encode()) == M.like(s, p), (s, p)
    for s, p in M.LONG_CASES:
        assert M.like_repaired(s.encode(), p.encode()) == M.like(s, p), (len(s), s[-4:], p)
    for s, p in M.random_pairs(20251020, 20_000):
        assert M.like_repaired(s.encode(), p.encode()) == M.like(s, p), (s, p)


def test_c_oracle_matcher_is_the_regex():
    from oracle import q45_native

    for s in M.EXHAUSTIVE_STRINGS:
        bs = s.encode()
        for p in M.EXHAUSTIVE_PATTERNS:
            assert q45_native.like_match(bs, p.encode()) == M.like(s, p), (s, p)
    for s, p in M.LONG_CASES:
        assert q45_native.like_match(s.encode(), p.encode()) == M.like(s, p), (len(s), s[-4:], p)
    for s, p in M.random_pairs(7, 5_000):
        assert q45_native.like_match(s.encode(), p.encode()) == M.like(s, p), (s, p)


def test_c_oracle_config5_filters_by_the_regex():
    """q5_run (the config-5 restatement) over a dictionary whose entries end in newlines: the groups that survive the LIKE
    and their counts are the model's."""
    from oracle import q45_native

    modes = ["AIR", "AIR\n", "REG AIR\n", "\n", "", "x\ny", "AIR\n\n", "RAIL"]
    rng = np.random.default_rng(5)
    n = 4000
    flag = rng.choice(np.frombuffer(b"ANR", np.uint8), n)
    mode = rng.integers(0, len(modes), n).astype(np.uint8)
    qty = rng.integers(1, 50, n).astype(np.float32)
    disc = (rng.integers(0, 10, n) / 100).astype(np.float32)
    for pattern in ["AIR", "%AIR%", "_", "", "%", "%AIR", "x_y", "x%y", "AIR\n", "%\n"]:
        rows = q45_native.run_strkey_like(flag, mode, modes, qty, disc, [1500, 0, 2500], pattern)
        got = {r["k"]: r["count"] for r in rows}
        want: dict[str, int] = {}
        for f, m in zip(flag.tolist(), mode.tolist()):
            if M.like(modes[m], pattern):
                key = f"{chr(f)}-{modes[m]}"
                want[key] = want.get(key, 0) + 1
        assert got == want, pattern
