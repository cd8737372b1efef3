"""Parity verify swept by position: a wrong byte at every byte offset of a
shard, in every tile slot, in every lane of the locate pass, and in a batch
long enough for the locate kernel's second grid-stride round.

gf_verify_kernel compares four dwords per lane per row; verify_locate_kernel
ANDs the lanes' candidate sets over 64 lanes (shuffles), 4 waves (LDS
atomics) and a stride loop over the shard's dwords.  test_gpu_verify.py puts
the wrong byte at 0, S-1 and one random interior position per block, so a
dropped dword, lane, wave or stride round is caught there only by luck; here
every one of them decides some block's word.  Each block's word differs from
its neighbours', so a bit OR-ed into the wrong block's word shows.

Every expectation is by construction (test_gpu_verify.single, or mask = all
rows + UNLOCATED) and is also compared with the restated definition
(test_gpu_verify.expected) through test_gpu_verify.check, which asserts 0 for
every untouched block."""
import numpy as np
import pytest

from conftest import SEED
from test_gpu_verify import UNLOCATED, check, clean, expected, run_device, single

pytestmark = pytest.mark.gpu


def copies(O, shape):
    data, parity = clean(O, shape)
    return data.copy(), parity.copy()


def flip(data, parity, k, b, idx, pos, val):
    """XOR val into byte pos of shard idx (data 0..k-1, then parity) of block b."""
    if idx < k:
        data[b, idx, pos] ^= val
    else:
        parity[b, idx - k, pos] ^= val


# (k, m, S): n = S blocks, block b wrong at byte b
BYTE_SHAPES = [
    (3, 2, 4160),   # straight-line body, stored parity loaded early, a tile across two blocks (86 MB)
    (5, 5, 1088),   # chunk loop, R = 6 with one padded row, parity loaded late, flat tiles across ~4 blocks
]


@pytest.mark.parametrize("k,m,S", BYTE_SHAPES, ids=["rs%d_%d_S%d" % s for s in BYTE_SHAPES])
def test_every_byte_position(codec, O, k, m, S):
    """Block b has one wrong byte at position p = b, in shard p % (k + m),
    bit 1 << (p % 8): every lane, dword and byte of the verify compare and
    every lane, wave and stride round of the locate pass decides one word."""
    shape = (k, m, S, S)
    data, parity = copies(O, shape)
    want = {}
    for p in range(S):
        idx = p % (k + m)
        flip(data, parity, k, p, idx, p, 1 << (p % 8))
        want[p] = single(k, m, idx)
    check(O, codec, shape, data, parity, set(want), want)


def test_every_tile_slot_at_64_byte_shards(codec, O):
    """RS(3,2) x 64 B, 64 blocks per tile, 4096 blocks: block b is wrong at
    byte (b // 64 + b) % 64 of shard b % 5, so each (tile slot, byte) pair
    occurs once."""
    shape = (3, 2, 64, 4096)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    want, seen = {}, set()
    for b in range(n):
        pos = (b // 64 + b) % 64
        seen.add((b % 64, pos))
        flip(data, parity, k, b, b % 5, pos, 1 << (b % 8))
        want[b] = single(k, m, b % 5)
    assert len(seen) == 64 * 64
    check(O, codec, shape, data, parity, set(want), want)


def test_disqualifying_byte_in_every_lane(codec, O):
    """RS(4,3) x 1088 B: 272 dwords, so the locate pass's 256 lanes plus a
    second stride round for lanes 0..15.  m = 3: two wrong data shards can
    never pass for one (test_gpu_verify's docstring), so in (a)-(c) the one
    byte of shard j2 empties the candidate set wherever it lies, and a
    reduction that drops one lane's, wave's or stride round's set locates j1:
      (a) j1 wrong at a byte of dword 0, j2 at byte 4 w + w % 4, w = 1..271
      (b) j1 wrong at a byte of dword 271, j2 at byte 4 w + w % 4, w = 0..270
      (c) j1 XOR-ed with nonzero bytes everywhere, j2 wrong at a byte of dword
          w, w = 0..271 (that byte has two wrong shards)
      (d) control: j1 wrong at one byte of every dword -> located at j1
    Wrong blocks are the odd ones; the even ones stay clean."""
    k, m, S = 4, 3, 1088
    W = S // 4
    assert W == 272
    cases = ([("a", w) for w in range(1, W)] + [("b", w) for w in range(W - 1)] +
             [("c", w) for w in range(W)] + [("d", j) for j in range(k)])
    shape = (k, m, S, 2 * len(cases) + 1)
    data, parity = copies(O, shape)
    rng = np.random.default_rng(SEED + 70)
    want = {}
    for c, (fam, w) in enumerate(cases):
        b = 2 * c + 1
        if fam == "d":
            j1 = w
            data[b, j1, 4 * np.arange(W) + np.arange(W) % 4] ^= rng.integers(1, 256, W, dtype=np.uint8)
            want[b] = single(k, m, j1)
            continue
        j1 = w % k
        j2 = (j1 + 1 + (w // k) % (k - 1)) % k
        assert j1 != j2
        if fam == "a":
            data[b, j1, w % 4] ^= int(rng.integers(1, 256))
        elif fam == "b":
            data[b, j1, 4 * (W - 1) + w % 4] ^= int(rng.integers(1, 256))
        else:
            data[b, j1] ^= rng.integers(1, 256, S, dtype=np.uint8)
        data[b, j2, 4 * w + w % 4] ^= int(rng.integers(1, 256))
        want[b] = ((1 << m) - 1, UNLOCATED)
    check(O, codec, shape, data, parity, set(want), want)


def test_locate_second_grid_round(codec, O):
    """launch_verify_locate caps its grid at 2048 workgroups of 64 verdict
    words (ec_kernels.hip; this test follows that cap), so block 2048 * 64 is
    the first of workgroup 0's second round.  RS(3,2) x 64 B, n = 2048 * 64 +
    64 + 3 (42 MB): one wrong byte, each in a different shard, in the first
    and last block of round one's first and last workgroups and of round
    two's two workgroups (the second a partial one), and two data shards
    wrong at different bytes (unlocated at any m >= 2: each byte alone names
    another shard) inside round two.  Every other word is 0."""
    GRID, WORDS = 2048, 64
    shape = (3, 2, 64, GRID * WORDS + 64 + 3)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    want = {}
    first2 = GRID * WORDS
    for i, b in enumerate([0, 63, 64, first2 - 1, first2, first2 + 63, first2 + 64, n - 1]):
        idx = i % (k + m)
        flip(data, parity, k, b, idx, (11 * i + 3) % S, 1 << (i % 8))
        want[b] = single(k, m, idx)
    two = first2 + 10
    data[two, 0, 5] ^= 0x21
    data[two, 2, 40] ^= 0x84
    want[two] = ((1 << m) - 1, UNLOCATED)
    from memo_amd import ec
    got = run_device(codec, k, m, data, parity)
    assert np.count_nonzero(got) == len(want), np.flatnonzero(got)[:16]
    assert np.array_equal(got, expected(O, k, m, S, data, parity, set(want)))
    mask, shard = ec.split_verdict(got)
    for b, w in want.items():
        assert (int(mask[b]), int(shard[b])) == w, (b, hex(int(got[b])))


def test_all_64_words_of_a_group_flagged(codec, O):
    """RS(10,4) x 448 B, 130 blocks, every one wrong (shard b % 14): the
    locate pass's ballot is all ones and its block loop takes 64 turns."""
    shape = (10, 4, 448, 130)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    want = {}
    for b in range(n):
        flip(data, parity, k, b, b % 14, (b * 37) % S, 1 << (b % 8))
        want[b] = single(k, m, b % 14)
    check(O, codec, shape, data, parity, set(want), want)
