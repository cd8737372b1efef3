"""The compiled multiply-accumulate bodies and the codes that reach them.

The MAC of memo_amd/csrc/ec_kernels.hip is compiled once per (KC, R): shard
chunk KC = mac_kchunk(k, R), row bound R = mac_rbound(r), with r = m for
encode and verify and r = e (lost shards per block) for rebuild; and each
pair once more per kernel family.  This helper holds, without a GPU and
without a test function,

  COMPILED      the (KC, R) pairs the dispatch switches serve, as a literal:
                tests/test_mac_bodies_plan.py holds it to the text of
                ec_kernels.hip.  A new body needs an entry here, and the
                sweep of tests/test_gpu_mac_bodies.py then has to reach it.
  codes()       the (k, r) codes the sweep runs, derived from ec.mac_rbound /
                ec.mac_kchunk: every body at k == KC where it has one, the
                4-shard chunk loop at k < 4, every k % 4 and MEMO_EC_MAX_K,
                every R dense (r == R) and with its largest padding.
  flat()        plan_segment's choice (memo_ec.cpp) between the flat mapping
  edge_sizes()  and tiles inside one block for per-block tables, and the two
                shard sizes on either side of it.

flat() and edge_sizes() restate the planner only to CHOOSE INPUTS: shard
sizes at which a tile stages close to its capacity of table slots.  They
judge nothing.  Every byte a kernel writes at those sizes is compared with
the CPU oracle; if the restatement drifts from the planner the sweep still
checks bytes, merely at a less telling size, and test_mac_bodies_plan.py
reports what it can see of the drift (the constants are read from the
sources' text, not typed in).

plan_segment also has a branch for per-block table IMAGES (tab_bstride != 0)
with C < MAC_TILE columns per shard: many image sets of one tile in LDS.
It cannot be reached: the only caller that passes per-block images is the
rows rebuild with rows_images() true, and rows_images() refuses shards of
less than image_min_tiles >= 1 whole tiles (C >= MAC_TILE); image_min_tiles
= 0 turns images off altogether.  flat("images", ...) restates the branch
all the same, as the planner has it.
"""
import functools
import os
import re

from memo_amd import ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memo_amd", "csrc")

# (KC, R): launch_mac / launch_mac_ragged of ec_kernels.hip
COMPILED = frozenset(
    [(KC, R) for KC in (2, 3, 4, 10, 16) for R in (1, 2, 3, 4, 6, 8, 12, 16)] +
    [(KC, R) for KC in (6, 12, 14) for R in (1, 2, 3, 4)])

MAX_K, MAX_M = ec.MAX_K, ec.MAX_M
LANES = 256  # lanes of a workgroup: the literal 256u of plan_segment's staging bounds


def body(k, r):
    """(KC, R) of the body that multiplies k input shards into r output rows."""
    R = ec.mac_rbound(r)
    return ec.mac_kchunk(k, R), R


def kpad(k, r):
    KC = body(k, r)[0]
    return -(-k // KC) * KC


def row_bounds():
    return sorted({ec.mac_rbound(r) for r in range(1, MAX_M + 1)})


def row_counts():
    """Every row bound dense (r == R) and with its largest padding (r = the
    previous bound + 1)."""
    bounds = row_bounds()
    return sorted(set(bounds) | {lo + 1 for lo in bounds[:-1]})


def straight_ks():
    """k with a straight-line body of its own (at R = 1: the most there are)."""
    return [k for k in range(1, MAX_K + 1) if ec.mac_kchunk(k, 1) == k]


def loop_ks():
    """k for the KC = 4 chunk loop: one below the chunk, the smallest k above
    it of every k % 4, a k whose R = 16 tables fill the flat mapping's slots
    at two sets per tile (16 x 36 = 576), and MEMO_EC_MAX_K."""
    loop = [k for k in range(1, MAX_K + 1) if k != 4 and ec.mac_kchunk(k, 1) == 4]
    below = [k for k in loop if k < 4][:1]
    residues = [min(k for k in loop if k > 4 and k % 4 == q) for q in (1, 3, 0, 2)]
    return below + residues + [33, MAX_K]


def codes():
    """The (k, r) codes of the sweep, in a fixed order."""
    return [(k, r) for k in straight_ks() + loop_ks() for r in row_counts()]


def codes_of(KC):
    return [(k, r) for (k, r) in codes() if body(k, r)[0] == KC]


# ------------------------------------------------- the planner's constants
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    """`constexpr <type> name = <int> [* <int> ...];` in a source text."""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9uU* ]+);" % re.escape(name), text)
    assert m, name
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f.strip().rstrip("uU"))
    return v


@functools.lru_cache(maxsize=None)
def _constants():
    h, c = _text("ec_kernels.h"), _text("memo_ec.cpp")
    return {"MAC_TILE": _constant(h, "MAC_TILE"), "MAC_COEF_REGS": _constant(h, "MAC_COEF_REGS"),
            "MAC_TAB_REGS": _constant(h, "MAC_TAB_REGS"), "kLdsBudget": _constant(c, "kLdsBudget")}


def constants():
    """MAC_TILE, MAC_COEF_REGS and MAC_TAB_REGS from the text of ec_kernels.h,
    kLdsBudget from the text of memo_ec.cpp."""
    return dict(_constants())


def sets_per_tile(C, tile):
    """Blocks a tile of `tile` columns can touch when a shard has C columns."""
    return (tile - 1 + C - 1) // C + 1


def flat(mode, k, r, S):
    """plan_segment's mapping of a segment with PER-BLOCK tables, restated:
    True = flat (a tile spans blocks, sets_per_tile(C) table sets in LDS),
    False = tiles inside one block.  mode: "rows" / "fused" (tables built in
    LDS from per-block coefficient rows: 20 bytes per slot, one pad slot per
    set, at most MAC_COEF_REGS coefficients staged per lane) or "images"
    (per-block table images through HBM: 32 bytes per slot, and a tile
    across blocks stages every set in MAC_TAB_REGS dwords per lane).  It
    chooses test inputs and judges nothing (module docstring)."""
    c = constants()
    per = body(k, r)[1] * kpad(k, r)
    C = S // 16
    sets = sets_per_tile(C, c["MAC_TILE"])
    if mode in ("rows", "fused"):
        return sets * (per + 1) * 20 <= c["kLdsBudget"] and sets * per <= LANES * c["MAC_COEF_REGS"]
    assert mode == "images", mode
    if C >= c["MAC_TILE"] and sets * per * 8 > LANES * c["MAC_TAB_REGS"]:
        return False
    return sets * per * 32 <= c["kLdsBudget"]


# Shard sizes past this one all plan alike: from C = MAC_TILE columns on a
# tile touches two blocks at the most.
S_TOP = 8192


def edge_sizes(mode, k, r):
    """(the largest multiple of 64 that is not flat, the smallest that is),
    or None where every size is flat or none is.  The decision is monotone
    in S for these modes (sets_per_tile falls as C grows), which
    test_mac_bodies_plan.py checks.  Like flat(), this only chooses the
    shard sizes a test runs; the oracle judges every byte written there."""
    sizes = range(64, S_TOP + 64, 64)
    first = next((S for S in sizes if flat(mode, k, r, S)), None)
    if first is None or first == 64:
        return None
    return first - 64, first
