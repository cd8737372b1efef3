"""Every compiled multiply-accumulate body in every kernel family on the
MI355X, against the CPU oracle.

The MAC of ec_kernels.hip is compiled per (KC, R) (tests/mac_bodies.py) and
again per family: gf_mac_kernel's encode and rows instances,
gf_mac_images_kernel, gf_rebuild_kernel (fused), gf_verify_kernel and the two
ragged kernels.  This module runs the 180 codes of mac_bodies.codes() --
every body at k == KC where there is one, the chunk loop at k < KC, every
k % 4 and k = 64, every row bound dense and with its largest padding --
through each family.  Every buffer of every call is guarded
(tests/guarded.py); the judge is the oracle, bit for bit (oracle.encode,
oracle.gather, oracle.erasures), and for verdict words the restated
definition of tests/test_gpu_verify.py.  There is no tolerance.

Shapes (a tile is 256 columns of 16 bytes):
  S = 64,   n = 1     one tile, 4 live columns of 256
  S = 64,   n = 130   64 blocks per tile where the plan is flat, a partial
                      last tile
  S = 4160, n = 3     a tile across two blocks, or a 4-column second tile
  the two mac_bodies.edge_sizes of the code (families with per-block
  tables): the sizes on either side of the planner's flat / non-flat
  decision, where a flat tile stages the most table slots; with n = 5 and,
  where five blocks do not fill a tile, with the blocks of two whole tiles
  and one more, so that a tile holds as many table sets as that size allows

A test id is one (family, KC): it loops over that KC's codes and the shapes
and reports every failing case, not the first.
"""
import numpy as np
import pytest

import mac_bodies as B
import ragged_cases as RC
import test_gpu_ragged as RG
import test_gpu_verify as V
from conftest import REBUILD_PATHS, SEED
from guarded import Guarded
from test_gpu_bounds import Cases, run_encode, run_rebuild, run_verify

pytestmark = pytest.mark.gpu

COMMON = [(64, 1), (64, 130), (4160, 3)]   # (S, n)
KCS = sorted({KC for KC, _ in B.COMPILED})
KC_IDS = ["kc%d" % KC for KC in KCS]
# the settings of conftest.REBUILD_PATHS that pick a kernel by themselves
SETTINGS = ["fused", "lds", "images"]
PATH_NAME = {"fused": "fused", "lds": "rows", "images": "images"}  # Codec.rebuild_path's word
# the ragged size list: many blocks in a tile, a straddle, a zero size, a
# multi-tile block, a short tail.  Registered under this name for
# test_gpu_ragged.clean when a test first needs it (never at import: the
# other ragged modules parametrise over RC.LISTS).
RAGGED_NAME, RAGGED_SIZES = "mac_bodies", [64, 4032, 64, 0, 4160, 64]


def setting(codec, name):
    v, t, cf = REBUILD_PATHS[name]
    return codec.options(rebuild_path=v, image_min_tiles=t, image_min_coefs=cf)


def clean(O, k, m, S, n):
    """(data n x k x S, parity n x m x S), seeded data and the oracle's
    parity, computed once per shape and read only (test_gpu_verify.clean)."""
    return V.clean(O, (k, m, S, n))


def attempt(cases, label, fn, *args, **kw):
    """A helper that asserts by itself, as one case of `cases`."""
    try:
        return fn(*args, **kw)
    except AssertionError as exc:
        cases.failed.append("%s:\n%s" % (label, exc))


# ------------------------------------------------------------ a. dispatch
@pytest.mark.parametrize("k0", range(1, B.MAX_K + 1, 16), ids=lambda k0: "k%d_%d" % (k0, k0 + 15))
def test_every_code_has_a_body(codec, O, k0):
    """Every (k, m) the ABI takes, at the smallest tile: a (k, R) that the
    library's mac_kchunk / mac_rbound map to a pair that is not compiled
    comes back as an error, a body that is wrong there as wrong bytes.  This
    holds ec.mac_kchunk / ec.mac_rbound, from which the sweep below is
    derived, to the C++ functions: the codes they call covered would
    otherwise run other bodies than the test believes."""
    cases = Cases()
    for k in range(k0, k0 + 16):
        for m in range(1, B.MAX_M + 1):
            data, par = clean(O, k, m, 64, 1)
            run_encode(codec, cases, "rs%d_%d" % (k, m), k, m, 64, 1, data.reshape(1, k * 64),
                       par.reshape(1, m * 64))
    cases.done()


# -------------------------------------------------------------- b. encode
@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_encode(codec, O, KC):
    cases = Cases()
    for k, m in B.codes_of(KC):
        for S, n in COMMON:
            data, par = clean(O, k, m, S, n)
            run_encode(codec, cases, "rs%d_%d S=%d n=%d" % (k, m, S, n), k, m, S, n,
                       data.reshape(n, k * S), par.reshape(n, m * S))
    cases.done()


# -------------------------------------------------------------- c. verify
def corruptions(k, m, S):
    """(shard, byte): the last byte of the last data shard (the chunk loop's
    tail shard), the last byte of the last parity row (the row next to the
    padding), byte 0 of parity row 0."""
    return [(k - 1, S - 1), (k + m - 1, S - 1), (k, 0)]


def victims(k, m, n):
    """block -> corruption number: three blocks in different tiles where n
    allows; a single block takes one of the three, by the code."""
    if n == 1:
        return {0: (k + m) % 3}
    if n == 3:
        return {0: 0, 1: 1, 2: 2}
    return {0: 0, n // 2 - 1: 1, n - 1: 2}


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_verify(codec, O, KC):
    """A clean batch reads all 0 (padded rows R > m are not compared); then
    one call with up to three corrupted blocks: each word is the
    definition's, every other word 0.  R <= 4 takes the early parity loads
    (PV_EARLY), k <= 16 verify_locate_kernel<16>, k > 16 <MEMO_EC_MAX_K>."""
    cases = Cases()
    for k, m in B.codes_of(KC):
        for S, n in COMMON:
            label = "rs%d_%d S=%d n=%d" % (k, m, S, n)
            data, par = clean(O, k, m, S, n)
            run_verify(codec, cases, label + " clean", k, m, S, n, data, par, np.zeros(n, np.uint32))
            data, par = data.copy(), par.copy()
            hit = victims(k, m, n)
            for b, c in hit.items():
                shard, pos = corruptions(k, m, S)[c]
                if shard < k:
                    data[b, shard, pos] ^= 0x10
                else:
                    par[b, shard - k, pos] ^= 0x10
            want = V.expected(O, k, m, S, data, par, set(hit))
            assert np.count_nonzero(want) == len(hit), label
            run_verify(codec, cases, label + " corrupted", k, m, S, n, data, par, want)
    cases.done()


# -------------------------------------------------------------- d. ragged
def ragged_clean(O, k, m):
    RC.LISTS.setdefault(RAGGED_NAME, RAGGED_SIZES)
    return RG.clean(O, RAGGED_NAME, k, m)


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_ragged_encode(codec, O, KC):
    cases = Cases()
    for k, m in B.codes_of(KC):
        ragged_clean(O, k, m)
        attempt(cases, "rs%d_%d" % (k, m), RG.encode_checked, codec, O, RAGGED_NAME, k, m)
    cases.done()


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_ragged_verify(codec, O, KC):
    """Clean, then the three corruptions of test_verify in blocks 0, 2 and 4
    (64 bytes in a shared tile; 64 bytes behind a straddling block; the
    multi-tile block)."""
    cases = Cases()
    for k, m in B.codes_of(KC):
        sizes, data, par = ragged_clean(O, k, m)
        label = "rs%d_%d" % (k, m)
        attempt(cases, label + " clean", RG.verify_checked, codec, O, k, m, sizes, data, par, set())
        data, par = data.copy(), par.copy()
        for c, b in enumerate((0, 2, 4)):
            shard, pos = corruptions(k, m, sizes[b])[c]
            RG.flip(sizes, k, m, data, par, b, shard, pos)
        want = attempt(cases, label + " corrupted", RG.verify_checked, codec, O, k, m, sizes, data, par,
                       {0, 2, 4})
        if want is not None:
            assert np.flatnonzero(want).tolist() == [0, 2, 4], label
    cases.done()


# ------------------------------------------------------------- e. rebuild
def rebuild_codes(KC):
    """(k, m, e): e = m = r of every code, and m = 16 beside it for
    r in {1, 4} (lost indices up to k + 15, the LW0 table of another code)."""
    out = []
    for k, r in B.codes_of(KC):
        out.append((k, r, r))
        if r in (1, 4):
            out.append((k, B.MAX_M, r))
    return out


_PATTERNS = {}


def patterns(O, k, m, e, n):
    """Per-block random survivor sets (oracle.erasures) in random order: k of
    the k + m - e shards that are left, the lost shards in random order
    too.  Computed once, read only."""
    if (k, m, e, n) in _PATTERNS:
        return _PATTERNS[(k, m, e, n)]
    rng = np.random.default_rng(SEED ^ (k * 4099 + m * 131 + e * 7 + n))
    _, l = O.erasures(SEED, 1000 * k + 16 * m + e, n, k, m, e)
    s = np.zeros((n, k), np.uint8)
    for b in range(n):
        left = np.setdiff1d(np.arange(k + m, dtype=np.uint8), l[b])
        s[b] = rng.permutation(left)[:k]
        l[b] = rng.permutation(l[b])
    s.setflags(write=False)
    l.setflags(write=False)
    _PATTERNS[(k, m, e, n)] = (s, l)
    return s, l


def edge_shapes(mode, k, e):
    """(S, n) at the code's edge sizes: n = 5, and enough blocks for two whole
    tiles and one more (only then does a flat tile of small shards touch
    every block, and build every table set, it has room for)."""
    out = []
    for S in B.edge_sizes(mode, k, e) or ():
        full = -(-2 * B.LANES // (S // 16)) + 1
        out += [(S, 5)] + ([(S, full)] if full > 5 else [])
    return out


def rebuild_ref(O, k, m, e, S, n, uniform=False):
    """(surv_idx, lost_idx, the survivors, the lost shards) of n blocks."""
    if m == e and (S, n) in COMMON:
        data, par = clean(O, k, m, S, n)
    else:  # not kept: the edge sizes and the m = 16 codes are used once per setting
        rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + S * 31 + n))
        data = rng.integers(0, 256, size=(n, k, S), dtype=np.uint8)
        par = O.encode(k, m, S, data.reshape(n, k * S))
    s, l = patterns(O, k, m, e, n)
    if uniform:
        s, l = np.tile(s[0], (n, 1)), np.tile(l[0], (n, 1))
    data, par = data.reshape(n, k * S), par.reshape(n, m * S)
    return s, l, O.gather(k, m, S, data, par, s), O.gather(k, m, S, data, par, l)


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
@pytest.mark.parametrize("path", ["fused", "lds"])
def test_rebuild_tables_built_per_tile(codec, O, path, KC):
    """gf_rebuild_kernel (fused) and gf_mac_kernel's rows instance with
    tables built in LDS ("lds"), at the common shapes and on both sides of
    the planner's flat / non-flat decision."""
    mode = PATH_NAME[path]
    cases = Cases()
    with setting(codec, path):
        for k, m, e in rebuild_codes(KC):
            for S, n in COMMON + edge_shapes(mode, k, e):
                assert codec.rebuild_path(n, k, S, e) == mode
                run_rebuild(codec, cases, "rs%d_%d e=%d S=%d n=%d" % (k, m, e, S, n), k, m, S, n,
                            rebuild_ref(O, k, m, e, S, n))
    cases.done()


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_rebuild_images(codec, O, KC):
    """Per-block table images through HBM (gf_mac_images_kernel): whole
    tiles only.  Up to R * kpad = 64 a tile spans two blocks' image sets,
    staged in registers; above it tiles stay inside a block."""
    cases = Cases()
    with setting(codec, "images"):
        for k, m, e in rebuild_codes(KC):
            for S, n in [(4096, 3), (4160, 3)]:
                assert codec.uses_images(k, S, e) and codec.rebuild_path(n, k, S, e) == "images"
                run_rebuild(codec, cases, "rs%d_%d e=%d S=%d n=%d" % (k, m, e, S, n), k, m, S, n,
                            rebuild_ref(O, k, m, e, S, n))
    cases.done()


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_rebuild_uniform(codec, O, KC):
    """One pattern for the whole batch: gf_mac_kernel's encode instance over
    a shared table image of the decode rows."""
    cases = Cases()
    for k, m, e in rebuild_codes(KC):
        for S, n in COMMON:
            run_rebuild(codec, cases, "rs%d_%d e=%d S=%d n=%d" % (k, m, e, S, n), k, m, S, n,
                        rebuild_ref(O, k, m, e, S, n, uniform=True), uniform=True)
    cases.done()


# ---------------------------------------------------- f. raised row bound
RAISED = {k: [(1, 16), (2, 6), (3, 8), (5, 12)] for k in (2, 3, 4, 10, 16, 5)}
RAISED.update({k: [(1, 4)] for k in (6, 12, 14)})
SMALL, LARGE = (64, 67), (4160, 3)


@pytest.mark.parametrize("k", sorted(RAISED), ids=lambda k: "k%d" % k)
def test_raised_row_bound(codec, O, k):
    """Two segments of one k in one call whose r differ: both take the body
    of the larger bound, the small one with coef_rows < R.  Both must be
    exact and the guards around the small segment's output intact: rows
    e..R-1 are written nowhere.  The small segment is 67 blocks of 64 bytes,
    the large one 3 of 4160; one encode_segments call, and one
    rebuild_segments call per rebuild setting (under "images" the large
    segment's image tiles join the rows launch of the small one)."""
    cases = Cases()
    for r_small, r_big in RAISED[k]:
        assert B.body(k, r_small)[0] == B.body(k, r_big)[0]
        assert B.body(k, r_small)[1] < B.body(k, r_big)[1]
        geo = [(r_small,) + SMALL, (r_big,) + LARGE]
        label = "k=%d r=%d+%d" % (k, r_small, r_big)
        g = Guarded()
        segs, want = [], {}
        for i, (m, S, n) in enumerate(geo):
            data, par = clean(O, k, m, S, n)
            segs.append((k, m, S, n, g.input("seg%d.data" % i, data.reshape(n, k * S)),
                         g.output("seg%d.parity" % i, (n, m * S))))
            want["seg%d.parity" % i] = par
        codec.encode_segments(segs)
        codec.synchronize()
        cases.check(label + " encode_segments", g, **want)
        for path in SETTINGS:
            g = Guarded()
            segs, want = [], {}
            for i, (e, S, n) in enumerate(geo):
                s, l, surv, lost = rebuild_ref(O, k, e, e, S, n)
                segs.append(dict(k=k, m=e, surv=g.input("seg%d.surv" % i, surv),
                                 surv_idx=g.input("seg%d.surv_idx" % i, s),
                                 lost_idx=g.input("seg%d.lost_idx" % i, l),
                                 out=g.output("seg%d.out" % i, (n, e * S))))
                want["seg%d.out" % i] = lost
            with setting(codec, path):
                # the setting did what the test believes (the class's bound is r_big's)
                small = "lds" if path == "images" else path  # no images below one whole tile
                assert codec.rebuild_path(LARGE[1], k, LARGE[0], r_big) == PATH_NAME[path]
                assert codec.rebuild_path(SMALL[1], k, SMALL[0], r_big) == PATH_NAME[small]
                codec.rebuild_segments(segs)
                codec.synchronize()
            cases.check("%s rebuild_segments %s" % (label, path), g, **want)
    cases.done()
