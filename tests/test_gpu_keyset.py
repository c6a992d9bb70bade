"""The key-set kernels of the LEFT SEMI / LEFT ANTI join at the C ABI (hs_keyset_build, hs_keyset_probe, hs_mask_from_counts):
every word of the bitmap against the words plain Python sets bit by bit, every mask byte against Python set membership -
nothing is computed, so nothing is tolerated.  Every build starts from a buffer filled with 0xFF (the build owes every word,
the rounding and the slack included), every mask carries sentinel bytes past its rows, and both are followed by guard bytes
no kernel may touch.  Tile, partition and chunk sizes are read from the source."""

from __future__ import annotations

import re

import numpy as np
import pytest

from minispark_amd import hipspark as hs
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _constants():
    text = (ROOT / "minispark_amd" / "csrc" / "hs_radix.hip").read_text()
    env: dict[str, int] = {"HS_WAVE": 64}
    for m in re.finditer(r"constexpr int (\w+) = ([^;]+);", text):
        try:
            env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))  # noqa: S307 - the repository's own source
        except Exception:  # noqa: BLE001, S112 - an expression over names this reader does not follow
            continue
    return env


_K = _constants()
RX_TILE, L, CHUNK, SLACK = _K["RX_TILE"], _K["KS_L"], _K["KS_CHUNK"], _K["KS_SLACK"]
PART = 1 << L
ROWS = [0, 1, 63, 64, 65, RX_TILE - 1, RX_TILE, RX_TILE + 1, 3 * RX_TILE + 17]
GUARD, SENTINEL = 64, 0x7E
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def test_the_sizes_were_found_in_the_code():
    assert RX_TILE == 8192 and 16 <= L <= 19 and CHUNK >= 1024 and SLACK == 64


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


def device_i32(dev, values):
    import torch

    arr = np.asarray(values, dtype=np.int64).astype(np.int32)
    t = torch.empty(len(arr) + 16, dtype=torch.int32, device=dev.device)  # (a pointer of its own even without rows)
    t[: len(arr)].copy_(torch.from_numpy(arr))
    assert t.data_ptr() % 16 == 0
    return t


def expected_words(build, key_min, slots):
    """word index -> word, set bit by bit: bit (s & 31) of word (s >> 5) for every build key key_min + s"""
    words: dict[int, int] = {}
    for k in set(int(v) for v in build):
        s = k - key_min
        assert 0 <= s < slots
        words[s >> 5] = words.get(s >> 5, 0) | (1 << (s & 31))
    return words


def build(dev, keys_dev, n, key_min, slots, bitmap=None):
    """hs_keyset_build into a buffer of 0xFF bytes + guard -> (the buffer as int32 words, the words of the bitmap)"""
    import torch

    lib = dev.lib
    nbytes = int(lib.hs_keyset_bitmap_bytes(slots))
    assert nbytes % 16 == 0 and nbytes >= (slots + 31) // 32 * 4 + SLACK
    if bitmap is None:
        bitmap = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev.device)
    ws_bytes = int(lib.hs_keyset_ws_bytes(n, slots))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=dev.device)
    dev.flags.zero_()
    hs.check(lib.hs_keyset_build(dev.stream, keys_dev.data_ptr(), n, key_min, slots, bitmap.data_ptr(), ws.data_ptr(),
                                 dev.flags.data_ptr()), "hs_keyset_build")
    return bitmap, nbytes // 4


def check_bitmap(bitmap, n_words, want):
    """every non-zero word of the buffer is a wanted one with the wanted bits; the guard behind it is untouched"""
    import torch

    words = bitmap[: n_words * 4].view(dtype=torch.int32)
    at = words.nonzero().flatten()
    got = dict(zip(at.cpu().tolist(), (int(v) & 0xFFFFFFFF for v in words[at].cpu().tolist())))
    assert got == want
    assert bool((bitmap[n_words * 4:] == 0xFF).all()), "the build wrote past the bitmap"


def probe(dev, bitmap, key_min, slots, probe_keys, anti):
    import torch

    n = len(probe_keys)
    keys = device_i32(dev, probe_keys)
    mask = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev.device)
    hs.check(dev.lib.hs_keyset_probe(dev.stream, keys.data_ptr(), n, key_min, slots, bitmap.data_ptr(), anti, mask.data_ptr()),
             "hs_keyset_probe")
    host = mask.cpu().numpy()
    assert (host[n:] == SENTINEL).all(), "mask bytes past n were written"
    return host[:n]


def run_case(dev, build_keys, key_min, slots, probe_keys):
    """build + exact bitmap check + semi and anti probes against Python set membership"""
    keys = device_i32(dev, build_keys)
    bitmap, n_words = build(dev, keys, len(build_keys), key_min, slots)
    assert dev.read_flags() == 0
    check_bitmap(bitmap, n_words, expected_words(build_keys, key_min, slots))
    members = set(int(v) for v in build_keys)
    want = np.array([1 if int(k) in members else 0 for k in probe_keys], dtype=np.uint8)
    semi = probe(dev, bitmap, key_min, slots, probe_keys, 0)
    anti = probe(dev, bitmap, key_min, slots, probe_keys, 1)
    assert np.array_equal(semi, want)
    assert np.array_equal(anti, 1 - want)  # the exact complement
    return bitmap


def some_probes(rng, build_keys, key_min, slots, n):
    """n probe keys: members, non-members inside the range and keys just outside it, shuffled"""
    hi = key_min + slots - 1
    inside = rng.integers(key_min, hi + 1, size=n, dtype=np.int64)
    if len(build_keys):
        take = rng.random(n) < 0.5
        inside[take] = np.asarray(build_keys, dtype=np.int64)[rng.integers(0, len(build_keys), size=int(take.sum()))]
    outside = rng.random(n) < 0.1
    inside[outside] = np.clip(np.where(rng.random(int(outside.sum())) < 0.5, key_min - 1 - rng.integers(0, 5, int(outside.sum())),
                                       hi + 1 + rng.integers(0, 5, int(outside.sum()))), I32_MIN, I32_MAX)
    return inside


# ---- rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_build", ROWS)
def test_build_row_counts_through_one_partition_pass(dev, n_build):
    """two partitions (slots just past 2^L): the keys go through one pass of RX_TILE-row tiles"""
    rng = np.random.default_rng(100 + n_build)
    key_min, slots = -12345, PART + 4097
    keys = rng.integers(key_min, key_min + slots, size=n_build, dtype=np.int64)
    run_case(dev, keys, key_min, slots, some_probes(rng, keys, key_min, slots, 1001))


@pytest.mark.parametrize("n_probe", [*ROWS, 2, 6, 66, RX_TILE + 3])
def test_probe_row_counts(dev, n_probe):
    rng = np.random.default_rng(200 + n_probe)
    key_min, slots = 7, 5000
    keys = rng.integers(key_min, key_min + slots, size=700, dtype=np.int64)
    run_case(dev, keys, key_min, slots, some_probes(rng, keys, key_min, slots, n_probe))


def test_the_probe_row_counts_cover_every_remainder():
    assert {n % 4 for n in [*ROWS, 2, 6, 66, RX_TILE + 3]} == {0, 1, 2, 3}


# ---- ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 31, 32, 33, PART - 1, PART, PART + 1])
def test_ranges_around_a_word_and_a_partition(dev, slots):
    key_min = -40
    picks = {0, slots - 1, slots // 2, min(31, slots - 1), min(32, slots - 1), max(slots - 2, 0)}
    picks |= {s for s in (PART - 2, PART - 1, PART) if 0 <= s < slots}  # either side of the partition boundary, the last bit
    keys = [key_min + s for s in sorted(picks)]
    probes = sorted({key_min + s + d for s in picks for d in (-1, 0, 1)} | {key_min - 1, key_min + slots, key_min + slots + 31})
    run_case(dev, keys, key_min, slots, probes)


def test_a_two_pass_geometry_with_a_handful_of_keys(dev):
    slots = PART << 9  # 2^9 partitions: two passes
    key_min = -(slots // 2)
    picks = [0, 1, PART - 1, PART, PART + 1, 255 * PART + 17, 256 * PART, slots - PART, slots - 33, slots - 1]
    keys = [key_min + s for s in picks]
    run_case(dev, keys, key_min, slots, [k + d for k in keys for d in (-1, 0, 1)])


def test_the_full_int32_range(dev):
    keys = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX]
    probes = sorted({min(max(k + d, I32_MIN), I32_MAX) for k in keys for d in (-1, 0, 1)})
    run_case(dev, keys, I32_MIN, 1 << 32, probes)


def test_an_empty_build_side_writes_zeros(dev):
    bitmap = run_case(dev, [], 5, 1000, [4, 5, 6, 1004, 1005])
    assert not bool(bitmap[: 1000 // 8].any())


# ---- out of range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_min", [100, I32_MAX - 1999, I32_MIN])
def test_probe_keys_outside_the_range_are_no_members(dev, key_min):
    """... also where key - key_min wraps in 32 bits onto a set slot: with key_min = 2^31 - 2000 the key -2^31 + 5 lies
    2^32 - 1005 below slot 1005, and 1005 is what a 32-bit subtraction makes of it"""
    slots = 2000
    keys = [key_min + s for s in (0, 5, 1005, 1999)]
    wrapped = [w for w in (k - (1 << 32) for k in keys) if w >= I32_MIN] + [w for w in (k + (1 << 32) for k in keys) if w <= I32_MAX]
    around = [key_min - 1, key_min - 2, key_min + slots, key_min + slots + 1, I32_MIN, I32_MIN + 5, I32_MIN + 1005, -1, 0,
              I32_MAX, I32_MAX - 994]
    probes = [p for p in [*wrapped, *around, *keys] if I32_MIN <= p <= I32_MAX]
    run_case(dev, keys, key_min, slots, probes)


def test_a_build_key_outside_the_range_raises_the_flag_and_sets_no_bit(dev):
    key_min, slots = 50, 100
    keys = [50, 149, 49, 150, 70]
    t = device_i32(dev, keys)
    bitmap, n_words = build(dev, t, len(keys), key_min, slots)
    assert dev.read_flags() & hs.FLAG_BAD_PROGRAM
    dev.flags.zero_()
    check_bitmap(bitmap, n_words, expected_words([50, 149, 70], key_min, slots))


# ---- crowding --------------------------------------------------------------------------------------------------------------
def test_one_key_repeated_over_several_chunks(dev):
    key_min, slots = -3, 7
    keys = np.full(2 * CHUNK + 5, key_min + 3, dtype=np.int64)
    run_case(dev, keys, key_min, slots, list(range(key_min - 2, key_min + slots + 2)))


def test_a_crowded_partition_next_to_a_quiet_one(dev):
    """partition 0 holds several chunks (merged with atomic ORs over its zeroed words), partition 1 a few keys (plain stores)"""
    rng = np.random.default_rng(7)
    key_min, slots = 1000, PART + 100
    crowd = rng.integers(key_min, key_min + PART, size=2 * CHUNK + 7, dtype=np.int64)
    quiet = np.array([key_min + PART, key_min + PART + 33, key_min + slots - 1], dtype=np.int64)
    keys = rng.permutation(np.concatenate([crowd, quiet]))
    run_case(dev, keys, key_min, slots, some_probes(rng, keys, key_min, slots, 4099))


def test_all_keys_distinct(dev):
    rng = np.random.default_rng(8)
    n = 3 * RX_TILE + 17
    keys = rng.permutation(n).astype(np.int64) * 3 - 1000  # every third slot
    run_case(dev, keys, -1000, 3 * n, some_probes(rng, keys, -1000, 3 * n, 2050))


# ---- hygiene ---------------------------------------------------------------------------------------------------------------
def test_a_reused_buffer_needs_no_memset_and_two_runs_give_equal_bytes(dev):
    rng = np.random.default_rng(9)
    key_min, slots = 0, PART + 77
    first = rng.integers(0, slots, size=RX_TILE + 5, dtype=np.int64)
    second = rng.integers(0, slots, size=300, dtype=np.int64)
    bitmap = run_case(dev, first, key_min, slots, first[:50])
    once = bitmap.clone()
    again, n_words = build(dev, device_i32(dev, first), len(first), key_min, slots, bitmap=bitmap)
    assert bool((again == once).all())
    # another key set into the same, now dirty, buffer: exactly its own bits
    reused, n_words = build(dev, device_i32(dev, second), len(second), key_min, slots, bitmap=bitmap)
    check_bitmap(reused, n_words, expected_words(second, key_min, slots))
    assert dev.read_flags() == 0


# ---- hs_mask_from_counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, RX_TILE + 3])
def test_mask_from_counts(dev, n):
    import torch

    rng = np.random.default_rng(300 + n)
    counts = rng.choice(np.array([0, 0, 1, 2, 1 << 31, 1 << 40, (1 << 63) - 1], dtype=np.int64), size=n)
    c = torch.empty(n + 8, dtype=torch.int64, device=dev.device)
    c[:n].copy_(torch.from_numpy(counts))
    for anti in (0, 1):
        mask = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev.device)
        hs.check(dev.lib.hs_mask_from_counts(dev.stream, c.data_ptr(), n, anti, mask.data_ptr()), "hs_mask_from_counts")
        host = mask.cpu().numpy()
        assert np.array_equal(host[:n], ((counts != 0).astype(np.uint8)) ^ anti)
        assert (host[n:] == SENTINEL).all()
