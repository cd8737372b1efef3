"""The cases of tests/wide_cases.py proven without a GPU, before
tests/test_gpu_wide_offsets.py puts them on the device: they can fail.

At the same shapes with every boundary 2^16 times lower (2^15 and 2^16 in
place of 2^31 and 2^32) a numpy model of each call runs over the whole
buffers, once honestly and once per offset role with that role's offsets cut
to 15 and to 16 bits: what the call reads from an input buffer, where it
writes its output, which verdict word it writes.  The comparison the device
tests use must accept the honest result and reject every narrow one.

Also held here: the reduced reference equals the full one on these shapes,
every planted byte lies where the method says, and the arithmetic the method
rests on (2^31 and 2^32 are multiples neither of 7 * 4096 nor of a block
stride)."""
import numpy as np
import pytest
import torch

import wide_cases as W
from guarded import FILL

BITS = (15, 16)


def materialize(lay):
    return W.fill(torch.empty(lay.total, dtype=torch.uint8), lay).numpy()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


MAC = {"encode_A": lambda: W.encode_case(W.SMALL_A), "encode_C": lambda: W.encode_case(W.SMALL_C),
       "rebuild_A": lambda: W.rebuild_case(W.SMALL_A), "rebuild_C": lambda: W.rebuild_case(W.SMALL_C),
       "rebuild_uniform_A": lambda: W.rebuild_case(W.SMALL_A, uniform=True)}


def pair_n(shape, x):
    """Blocks of RS(4,4) with k + x shards so that `have` just passes the
    upper boundary, and 5 more."""
    return -(-shape["bounds"][1] // ((shape["k"] + x) * shape["S"])) + 5


VERDICT = {
    "verify_A": lambda: W.VerdictCase("verify", W.SMALL_A, 2),
    "verify_B": lambda: W.VerdictCase("verify", W.SMALL_B, 2, m=2),
    "verify_C": lambda: W.VerdictCase("verify", W.SMALL_C, 2),
    "check_A_x1": lambda: W.VerdictCase("check", W.SMALL_A, 1),
    "check_A_x2": lambda: W.VerdictCase("check", W.SMALL_A, 2),
    "check_B_x1": lambda: W.VerdictCase("check", W.SMALL_B, 1, m=1),
    "check_B_x2": lambda: W.VerdictCase("check", W.SMALL_B, 2, m=2),
    "check_C": lambda: W.VerdictCase("check", W.SMALL_C, 2),
    "correct_A": lambda: W.VerdictCase("correct", W.SMALL_A, 2),
    "correct_B": lambda: W.VerdictCase("correct", W.SMALL_B, 2, m=2),
    "correct_C": lambda: W.VerdictCase("correct", W.SMALL_C, 2),
    "pair_A_x3": lambda: W.VerdictCase("pair", W.SMALL_A, 3, m=4, n=pair_n(W.SMALL_A, 3)),
    "pair_A_x4": lambda: W.VerdictCase("pair", W.SMALL_A, 4, m=4, n=pair_n(W.SMALL_A, 4)),
    "pair_B_x3": lambda: W.VerdictCase("pair", W.reduced_b(3, small=True), 3, m=4),
    "pair_B_x4": lambda: W.VerdictCase("pair", W.reduced_b(4, small=True), 4, m=4),
}
_MADE = {}


def made(name):
    if name not in _MADE:
        _MADE[name] = (MAC.get(name) or VERDICT[name])()
    return _MADE[name]


# ------------------------------------------------------------ the arithmetic

def test_boundaries_are_no_multiple_of_a_period_or_stride():
    for bound in (1 << 31, 1 << 32):
        assert bound % (W.PERIOD * W.TILE) != 0
    assert (1 << 32) % (W.PERIOD * W.TILE) == 16384
    S = W.SHAPE_A["S"]
    assert S == 1052736 and S % W.TILE == 64 and 2 * S * W.SHAPE_A["n"] == 4305690240 > 1 << 32
    # A displacement by a boundary never maps a block onto the same template:
    # it is no multiple of seven block strides, for any buffer (parity, data,
    # have at x = 1..4); in shape A it is no multiple of one stride either.
    # (Shape C's data and parity strides are powers of two and do divide the
    # boundaries, by a number of blocks that is 1, 2 or 4 mod 7.)
    for s in (W.SHAPE_A, W.SMALL_A, W.SHAPE_C, W.SMALL_C):
        for rows in (2, 4, 5, 6, 7, 8):
            for bound in s["bounds"]:
                assert bound % (W.PERIOD * rows * s["S"]), (s["S"], rows)
                assert bound % (rows * s["S"]) or s["S"] in (64, 2), (s["S"], rows)
    for s in (W.SHAPE_B, W.SMALL_B):
        for bound in s["bounds"]:
            assert bound % s["period"] and s["S"] % s["period"] and s["S"] > s["bounds"][0]
        assert 2 * s["S"] > s["bounds"][1]                 # shard 2 starts past the upper boundary
    assert W.SHAPE_B["S"] == 2147496000
    for x in (3, 4):                                       # check_pair's cut shape B
        for s in (W.reduced_b(x), W.reduced_b(x, small=True)):
            lo, hi = s["bounds"]
            assert (1 + x) * s["S"] < hi < (2 + x) * s["S"] and s["S"] < lo < 3 * s["S"]
            assert s["S"] % s["tile"] and s["S"] % s["period"]         # a partial last tile and period
    assert W.SHAPE_C["n"] > 1 << 25 and 4 * 64 * W.SHAPE_C["n"] > 1 << 33 and 2 * 64 * W.SHAPE_C["n"] > 1 << 32


# ------------------------------------------------------------- MAC calls

def run_mac(case, role=None, bits=None):
    inp = materialize(case.inp)
    seen = W.narrow_read(inp, bits) if role == "input" else inp
    res = W.model_mac(case, seen)
    out = W.narrow_write(res, bits, FILL) if role == "output" else res
    return W.problems("out", t(out), case.out) + W.problems("in", t(inp), case.inp)


@pytest.mark.parametrize("name", list(MAC))
def test_mac_honest_accepted_narrow_rejected(name):
    case = made(name)
    assert run_mac(case) == []
    for bits in BITS:
        assert case.inp.total > 1 << bits and case.out.total > 1 << bits
        for role in ("input", "output"):
            assert run_mac(case, role, bits), (name, role, bits)


def test_mac_templates_differ():
    for name in MAC:
        case = made(name)
        for lay in (case.inp, case.out):
            assert len({r.tobytes() for r in lay.tmpl}) == len(lay.tmpl)
    assert len({r.tobytes() for r in made("rebuild_A").in_idx}) > 1
    assert len({r.tobytes() for r in made("rebuild_uniform_A").in_idx}) == 1


# ---------------------------------------------------------- verdict calls

def run_verdict(case, group, role=None, bits=None):
    planted = case.planted(group)
    bufs = {name: materialize(lay.flipped(planted[name])) for name, (_, _, lay) in case.bufs.items()}
    seen = {name: W.narrow_read(a, bits) if role == name else a for name, a in bufs.items()}
    words, after = W.model_verdict(case, seen)
    if role == "verdict":
        words = W.narrow_write(words, bits, W.WORD_FILL)
    want, left = case.expected(group)
    msgs = W.word_problems("verdict", words, want)
    for name, (_, _, lay) in case.bufs.items():
        got = bufs[name].copy()
        at = np.flatnonzero(after[name] != seen[name])     # the bytes the call rewrites
        got[at % (1 << bits) if role == "output" else at] = after[name][at]
        msgs += W.problems(name, t(got), lay.flipped(left[name]))
    return msgs


def roles(case, bits):
    out = [name for name, (_, _, lay) in case.bufs.items() if lay.total > 1 << bits]
    if case.n > 1 << bits:
        out.append("verdict")
    if case.kind == "correct":
        out.append("output")
    return out


@pytest.mark.parametrize("name", list(VERDICT))
def test_verdict_honest_accepted_narrow_rejected(name):
    case = made(name)
    for group in case.groups:
        assert run_verdict(case, group) == [], name
    # Rejected by the calls of the case between them, as the device test makes
    # them all: one block that is wrong anyway can hide a displaced read (at
    # x = 1 every wrong block reads alike), its clean call cannot.
    assert max(off for g in case.groups for _, off, _ in g) >= 1 << max(BITS)
    for bits in BITS:
        rs = roles(case, bits)
        assert set(case.bufs) <= set(rs), (name, bits)     # every input buffer passes both boundaries
        for role in rs:
            assert any(run_verdict(case, g, role, bits) for g in reversed(case.groups)), (name, role, bits)


def test_every_role_meets_both_boundaries():
    seen = {(r, bits) for name in VERDICT for bits in BITS for r in roles(made(name), bits)}
    for bits in BITS:
        assert {("have", bits), ("data", bits), ("parity", bits), ("verdict", bits), ("output", bits)} <= seen


@pytest.mark.parametrize("name", list(VERDICT))
def test_reduced_reference_equals_the_full_one(name):
    case = made(name)
    for group in case.groups:
        assert case.expected(group) == case.expected(group, full=True)
        words, _ = case.expected(group)
        assert all(words.values()) and bool(words) == bool(group), "a planted block reads clean"


@pytest.mark.parametrize("name", list(VERDICT))
def test_plants_lie_where_the_method_says(name):
    case = made(name)
    S, tile = case.S, case.code.tile
    lo, hi = case.code.bounds
    places = W.plant_places(case)
    labels = [p[0] for p in places]
    assert labels[0] == "first" and labels[-2:] == ["last", "last"]
    for buf, (rows, pos0, lay) in case.bufs.items():
        assert lay.total == case.n * rows * S > hi
        assert ("lo", buf, lo) in places and ("hi", buf, hi) in places
    for label, buf, off in places:
        rows, pos0, lay = case.bufs[buf]
        b, q, i = case.where(buf, off)
        if label == "first":
            assert b == 0
        elif label == "last":
            assert b == case.n - 1 and q == case.kx - 1 and i // tile == (S - 1) // tile
            assert i in (S - 1, (S - 1) // tile * tile) and S % tile   # a partial tile's two ends
        else:
            bound = lo if label == "lo" else hi
            start = b * rows * S + (q - pos0) * S
            assert start <= bound < start + S                 # the shard that holds the boundary byte
            assert case.n > 1 or start < bound                # one block: the shard straddles it
    planted = [f for g in case.groups for f in g]
    for label, buf, off in places:
        assert any(f[0] == buf and f[1] == off for f in planted), (label, off)
    if case.n > 1:
        assert len(case.groups) == 2
        moved = {(buf, off + hi) for buf, off, _ in case.groups[1]}
        assert {(buf, off) for label, buf, off in places if off >= hi and label != "last"} <= moved
        high = set(case.by_block(case.groups[0])) - set(case.by_block(case.groups[1]))
        assert high                                           # their words must stay 0 in the second call
    else:
        assert case.groups[0] == [] and all(case.groups[1:])
    if case.kind == "pair":
        for g in case.groups:
            for b, flips in case.by_block(g).items():
                shards = {q for q, _, _ in flips}
                assert len(shards) == 2 and case.kx - 1 in shards
                assert any(i // tile == (S - 1) // tile for q, i, _ in flips if q == case.kx - 1) or \
                    len([f for f in flips if f[0] == case.kx - 1]) == 1   # the plant itself, not in its last tile


def test_pair_cases_name_pairs_and_corrections_mend():
    named = 0
    for name in VERDICT:
        case = made(name)
        for g in case.groups:
            words, left = case.expected(g)
            if case.kind == "pair":
                named += sum(1 for w in words.values() if w >> 25)
            if case.kind == "correct":
                assert all(w & W.CORRECTED for w in words.values())
                assert not any(left.values())
    assert named >= 8
