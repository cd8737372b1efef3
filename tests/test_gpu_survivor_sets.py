"""Survivor-set faults over every index range, lane group and tile slot.

A survivor set is validated six times: on the host (host_decode_rows, behind
the shared-pattern calls) and in five device paths, each with its own bit-set
layout -- decode_coef_wide_kernel<L> (three words by sv >> 5, lost index r in
lv[r / L] of lane r % L), decode_rows_k_kernel<K,MM> (one word by sv & 31 and
an OR of all indices for anything past 31), decode_coef_kernel<KMAX> (three
words, the word index clamped), and the fused rebuild's wave-local
dec_wave_set<KC,R> and its workgroup-wide dec_phase_b / dec_phase_c.  A miss
is silent: the block is rebuilt from a singular set, the call returns OK and
the bytes are garbage.  One status word serves a whole call, so a fault that
a path misses hides behind any other fault of the batch: every fault also
runs alone between two valid blocks.

Ground truth: a set is valid exactly when oracle.decode_matrix does not
raise -- a duplicate survivor or any index >= k + m is a fault; a lost index
that is a survivor, or one lost index twice, is valid.  test_catalogue_* holds
the whole catalogue to that on machines without a GPU.

Codes (k, m), each for what it reaches:
  (3, 2)    L = 4 wide, exact-k K = 3 MM = 4, wave-local fused
  (4, 16)   lost indices in lv[1..3], exact-k MM = 16, fused R > 4 lanes: the
            phase path with kin == KC (e = 5, 16; e = 1 is wave-local)
  (5, 3)    L = 8, generic, fused chunk loop
  (6, 3)    the 8-lane wave-local fused decode (KC = 6: 32 blocks per pass),
            exact-k K = 6
  (10, 4)   the headline code; 16 blocks per wave-local pass, so a 64-block
            tile has late passes
  (16, 16)  nt = 32: exact-k with valid = ~0, where only the OR of all
            indices sees index 32
  (20, 12)  nt = 32, not exact-k
  (20, 13)  nt = 33: index 32 is the first valid bit of word 1
  (33, 12)  the <64> instances, nt = 45
  (48, 16)  nt = 64
  (49, 16)  nt = 65: index 64 is the first bit of word 2
  (64, 16)  nt = 80

Catalogue, per code and e in {1, m} (and 5 for (4, 16)); every entry changes
one seeded valid set (survivors in random order), `a` being an index absent
from its survivors:
  D(i, j, v)  survivor positions i < j both hold v; (i, j) in {(0, 1),
              (0, k-1), (k-2, k-1)}, v in {0, 31, 32, 63, 64, nt-1} below nt
  R(i, v)     survivor position i in {0, k-1} holds v in {nt, a+32, a+64,
              96 + (a & 31), 128, 255}, those that are >= nt and <= 255: the
              ones that alias a modulo 32 pass a popcount check
  L(r, v)     lost position r in {0, e-1} (and 4, 5, 15 for (4, 16)) holds
              v in {nt, 128, 255}
  controls    (valid: rows = the oracle's) a lost index that is a survivor,
              one lost index twice, survivors in descending order, lost =
              the absent indices in ascending order (all m of them at e = m)
"""
import functools

import numpy as np
import pytest

from conftest import SEED
from guarded import FILL, Guarded
from test_gpu_parity import DECODE_KERNELS, dev, host

gpu = pytest.mark.gpu

ESINGULAR = -4
CODES = [(3, 2), (4, 16), (5, 3), (6, 3), (10, 4), (16, 16), (20, 12), (20, 13), (33, 12), (48, 16),
         (49, 16), (64, 16)]
CODE_IDS = ["rs%d_%d" % c for c in CODES]


def es_of(k, m):
    return sorted({1, m} | ({5} if (k, m) == (4, 16) else set()))


class Entry:
    def __init__(self, label, fault, surv, lost):
        self.label, self.fault = label, fault
        self.surv = np.ascontiguousarray(surv, dtype=np.uint8)
        self.lost = np.ascontiguousarray(lost, dtype=np.uint8)
        self.surv.setflags(write=False)
        self.lost.setflags(write=False)

    def __repr__(self):
        return self.label


def base_set(k, m, e):
    """(survivors, lost, absent) of the valid set every entry starts from."""
    rng = np.random.default_rng(SEED ^ (k * 4099 + m * 131 + e))
    perm = rng.permutation(k + m)
    return perm[:k].copy(), perm[k:k + e].copy(), perm[k:].copy()


@functools.lru_cache(maxsize=None)
def catalogue(k, m, e):
    """The entries of (k, m, e), faults first, in the module docstring's order."""
    nt = k + m
    surv0, lost0, absent = base_set(k, m, e)
    a = int(absent[0])
    out = []
    pairs = list(dict.fromkeys([(0, 1), (0, k - 1), (k - 2, k - 1)]))
    for i, j in pairs:
        assert 0 <= i < j < k
        for v in sorted({0, 31, 32, 63, 64, nt - 1}):
            if v < nt:
                s = surv0.copy()
                s[i] = s[j] = v
                out.append(Entry("D(%d,%d,%d)" % (i, j, v), True, s, lost0))
    for i in (0, k - 1):
        for v in dict.fromkeys([nt, a + 32, a + 64, 96 + (a & 31), 128, 255]):
            if nt <= v <= 255:
                s = surv0.copy()
                s[i] = v
                out.append(Entry("R(%d,%d)[a=%d]" % (i, v, a), True, s, lost0))
    for r in sorted({0, e - 1} | ({4, 5, 15} if (k, m) == (4, 16) else set())):
        if r < e:
            for v in (nt, 128, 255):
                l = lost0.copy()
                l[r] = v
                out.append(Entry("L(%d,%d)" % (r, v), True, surv0, l))
    l = lost0.copy()
    l[0] = surv0[k // 2]
    out.append(Entry("control:lost_is_survivor", False, surv0, l))
    if e >= 2:
        l = lost0.copy()
        l[1] = l[0]
        out.append(Entry("control:lost_twice", False, surv0, l))
    out.append(Entry("control:descending", False, np.sort(surv0)[::-1], lost0))
    out.append(Entry("control:lost_absent_ascending", False, surv0, np.sort(absent)[:e]))
    return tuple(out)


def faults(k, m, e):
    return [x for x in catalogue(k, m, e) if x.fault]


def controls(k, m, e):
    return [x for x in catalogue(k, m, e) if not x.fault]


def aliasing(k, m, e):
    """The R entries whose value is an absent index plus a multiple of 32."""
    a = int(base_set(k, m, e)[2][0])
    return [x for x in faults(k, m, e) if x.label.startswith("R(") and
            int(x.surv[int(x.label[2:].split(",")[0])]) in (a + 32, a + 64, 96 + (a & 31))]


def valid_by_definition(k, m, surv, lost):
    nt = k + m
    return len(set(surv.tolist())) == k and max(surv.tolist()) < nt and max(lost.tolist()) < nt


def oracle_rows(O, k, m, surv, lost):
    """The oracle's decode rows, or None when it refuses the set."""
    try:
        return O.decode_matrix(k, m, surv, lost)
    except ValueError:
        return None


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_catalogue_classification(O, k, m):
    """Every entry is what the catalogue says it is, by the oracle (valid
    exactly when decode_matrix does not raise) and by the definition; every
    kind is present at every e, and the aliasing R entries exist where a path
    depends on them (k + m <= 32: the exact-k kernel's one-word mask)."""
    nt = k + m
    for e in es_of(k, m):
        cat = catalogue(k, m, e)
        assert len({x.label for x in cat}) == len(cat)
        for x in cat:
            assert x.surv.shape == (k,) and x.lost.shape == (e,)
            ok = oracle_rows(O, k, m, x.surv, x.lost) is not None
            assert ok == (not x.fault), (k, m, e, x.label)
            assert valid_by_definition(k, m, x.surv, x.lost) == (not x.fault), (k, m, e, x.label)
        kinds = [x.label[0] for x in cat]
        assert kinds.count("D") == 3 * sum(v < nt for v in {0, 31, 32, 63, 64, nt - 1})
        assert kinds.count("R") >= 2 * 3 and kinds.count("L") >= 3
        assert kinds.count("c") == (4 if e >= 2 else 3)
        al = aliasing(k, m, e)
        assert al, (k, m, e)
        if nt <= 32:
            a = int(base_set(k, m, e)[2][0])
            # a + 32 lands on a's own bit of the one-word mask: K distinct
            # bits, none past nt
            hit = [x for x in al if (a + 32) in x.surv.tolist()]
            assert len(hit) == 2
            for x in hit:
                bits = {int(v) & 31 for v in x.surv}
                assert len(bits) == k and max(bits) < nt
    if (k, m) == (4, 16):
        assert {"L(4,20)", "L(5,128)", "L(15,255)"} <= {x.label for x in catalogue(k, m, 16)}
        assert {"L(4,20)"} <= {x.label for x in catalogue(k, m, 5)}


# ------------------------------------------------------------------ batches
def filler(k, m, e, count, salt):
    """`count` valid sets in random survivor order (lost: data, parity or
    survivor shards)."""
    rng = np.random.default_rng(SEED ^ (k * 7919 + m * 271 + e * 17 + salt))
    s = np.stack([rng.permutation(k + m)[:k] for _ in range(count)]).astype(np.uint8)
    l = np.stack([rng.permutation(k + m)[:e] for _ in range(count)]).astype(np.uint8)
    return s, l


def place(k, m, e, n, at):
    """A batch of n blocks: entry at[b] in block b, valid filler sets in the
    rest.  Returns (surv_idx, lost_idx)."""
    s, l = filler(k, m, e, n, 1)
    for b, x in at.items():
        s[b], l[b] = x.surv, x.lost
    return s, l


@functools.lru_cache(maxsize=None)
def alternating(k, m, e):
    """Every catalogue entry in its own block, valid blocks on both sides:
    (surv_idx, lost_idx, {block: entry})."""
    cat = catalogue(k, m, e)
    at = {2 * i + 1: x for i, x in enumerate(cat)}
    s, l = place(k, m, e, 2 * len(cat) + 1, at)
    return frozen(s), frozen(l), at


def lanes(k):
    """Lanes per block of the fused wave-local decode (dec_lanes<KC>) for
    k <= 16, of the column-per-lane decode beyond."""
    return 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


@functools.lru_cache(maxsize=None)
def tiled(k, m, e):
    """The same entries ordered by tile slot for S = 64 (64 blocks per flat
    tile): faults at slots 0, G-1, G, 2G and 63 of successive tiles, G =
    256 / L blocks decoded per pass and 2G the first slot of a late pass
    (slots past 63 do not exist for that L); controls at free slots of tile
    0; three more valid blocks as a partial last tile."""
    G = 256 // lanes(k)
    slots = sorted({s for s in (0, G - 1, G, 2 * G, 63) if s < 64})
    fs, cs = faults(k, m, e), controls(k, m, e)
    tiles = -(-len(fs) // len(slots))
    at = {}
    for i, x in enumerate(fs):
        at[64 * (i // len(slots)) + slots[i % len(slots)]] = x
    free = [s for s in range(2, 62) if s not in slots and s - 1 not in slots and s + 1 not in slots]
    for x, s in zip(cs, free[::3]):
        at[s] = x
    assert len(at) == len(fs) + len(cs)
    s, l = place(k, m, e, 64 * tiles + 3, at)
    return frozen(s), frozen(l), at


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rows_of(k, m, e, layout):
    """Expected decode rows of a layout's batch (zero for a faulty block)."""
    from oracle import oracle as O
    s, l, at = layout(k, m, e)
    want = np.zeros((s.shape[0], e * k), np.uint8)
    for b in range(s.shape[0]):
        if not (b in at and at[b].fault):
            want[b] = O.decode_matrix(k, m, s[b], l[b]).reshape(-1)
    return frozen(want)


@functools.lru_cache(maxsize=None)
def shards(k, m, S, nmax):
    """(data, parity) of nmax blocks by the oracle, computed once."""
    from oracle import oracle as O
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + S))
    data = rng.integers(0, 256, size=(nmax, k * S), dtype=np.uint8)
    return frozen(data), frozen(O.encode(k, m, S, data, threads=4))


def rebuild_case(O, k, m, S, s, l, at):
    """(survivor bytes, expected out) of a batch: survivors gathered at the
    indices clamped into range (a faulty block's bytes do not matter, an
    invalid index is never used as an address), out = the true lost shards,
    zero for a faulty block."""
    n, nt = s.shape[0], k + m
    data, par = shards(k, m, S, max(n, 8))
    data, par = data[:n], par[:n]
    sv = O.gather(k, m, S, data, par, np.minimum(s, nt - 1))
    want = O.gather(k, m, S, data, par, np.minimum(l, nt - 1))
    for b, x in at.items():
        if x.fault:
            want[b] = 0
    return sv, want


def preset(*shape):
    """A device buffer of 0xA5 (copied from the host: complete on return,
    whatever stream the codec runs on)."""
    return dev(np.full(shape, FILL, np.uint8))


def sync_code(codec):
    from memo_amd import ec
    try:
        codec.synchronize()
    except ec.MemoECError as ex:
        return ex.code
    return 0


def raised_once(codec, fails, label):
    """synchronize reports ESINGULAR once; a second one is clean."""
    rc = sync_code(codec)
    if rc != ESINGULAR:
        fails.append("%s: synchronize gave %d, want %d" % (label, rc, ESINGULAR))
    rc = sync_code(codec)
    if rc != 0:
        fails.append("%s: second synchronize gave %d, want 0" % (label, rc))


def blocks_differ(fails, label, got, want, at):
    """Names every block of `got` that is not `want` (n x bytes each)."""
    for b in np.flatnonzero((got != want).any(axis=1)):
        x = at.get(int(b))
        what = x.label if x else "valid block"
        if x and x.fault:
            fails.append("%s: block %d %s: not all zero (%d nonzero bytes, first 0x%02X)"
                         % (label, b, what, np.count_nonzero(got[b]), got[b][np.flatnonzero(got[b])[0]]))
        else:
            fails.append("%s: block %d %s: differs from the oracle at %d byte(s)"
                         % (label, b, what, np.count_nonzero(got[b] != want[b])))


def guards(fails, label, g, **want):
    try:
        g.check(**want)
    except AssertionError as exc:
        fails.append("%s:\n%s" % (label, exc))


def done(fails):
    assert not fails, "%d failure(s)\n%s" % (len(fails), "\n".join(fails[:40]))


# --------------------------------------------------------------- decode rows
@gpu
@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("kernel", list(DECODE_KERNELS))
def test_decode_rows_faults(codec, O, kernel, k, m):
    """memo_ec_decode_rows on each decode kernel: the whole catalogue in one
    batch (rows guarded, preset 0xA5: a faulty block's e * k bytes are all
    zero, every other block the oracle's rows, ESINGULAR once), then every
    fault alone between two valid blocks at e = m (it must raise by itself,
    and zero its own rows only) and every control alone (it must not)."""
    fails = []
    with codec.options(**DECODE_KERNELS[kernel]):
        for e in es_of(k, m):
            s, l, at = alternating(k, m, e)
            want = rows_of(k, m, e, alternating)
            n = s.shape[0]
            label = "decode_rows[%s] rs(%d,%d) e=%d" % (kernel, k, m, e)
            g = Guarded("device")
            rows = g.output("rows", (n, e * k))
            codec.decode_rows(k, m, g.input("surv_idx", s), g.input("lost_idx", l), rows)
            raised_once(codec, fails, label)
            blocks_differ(fails, label, host(rows), want, at)
            guards(fails, label, g, rows=want)
        e = m
        (fs, fl), label = filler(k, m, e, 2, 2), "alone[%s] rs(%d,%d) e=%d" % (kernel, k, m, e)
        w0, w2 = O.decode_matrix(k, m, fs[0], fl[0]).reshape(-1), O.decode_matrix(k, m, fs[1], fl[1]).reshape(-1)
        for x in catalogue(k, m, e):
            s, l = np.stack([fs[0], x.surv, fs[1]]), np.stack([fl[0], x.lost, fl[1]])
            mid = np.zeros(e * k, np.uint8) if x.fault else O.decode_matrix(k, m, x.surv, x.lost).reshape(-1)
            rows = preset(3, e * k)
            codec.decode_rows(k, m, dev(s), dev(l), rows)
            rc = sync_code(codec)
            if rc != (ESINGULAR if x.fault else 0):
                fails.append("%s %s: synchronize gave %d" % (label, x.label, rc))
            if sync_code(codec) != 0:
                fails.append("%s %s: the error was not cleared" % (label, x.label))
            blocks_differ(fails, "%s %s" % (label, x.label), host(rows), np.stack([w0, mid, w2]), {1: x})
    done(fails)


BANDS = [(1, 8), (9, 16), (17, 32), (33, 48), (49, 64)]


@functools.lru_cache(maxsize=None)
def band_ref(lo, hi, n=24):
    """[(k, m, e, surv_idx, lost_idx, the oracle's rows)] of a band of k."""
    from oracle import oracle as O
    out = []
    for k in range(lo, hi + 1):
        for m in range(1, 17):
            rng = np.random.default_rng(k * 1000 + m)
            for e in sorted({1, (m + 1) // 2, m}):
                s = np.stack([rng.permutation(k + m)[:k] for _ in range(n)]).astype(np.uint8)
                l = np.stack([rng.permutation(k + m)[:e] for _ in range(n)]).astype(np.uint8)
                rows = np.stack([O.decode_matrix(k, m, s[b], l[b]) for b in range(n)])
                out.append((k, m, e, frozen(s), frozen(l), frozen(rows.reshape(n, e * k))))
    return out


@gpu
@pytest.mark.parametrize("band", BANDS, ids=["k%d_%d" % b for b in BANDS])
@pytest.mark.parametrize("kernel", list(DECODE_KERNELS))
def test_decode_rows_every_code(codec, O, kernel, band):
    """Every k in 1..64 with every m in 1..16, e in {1, (m+1)//2, m}: 24
    blocks per call (six workgroups of the 64-lane kernel, a partial one of
    the one-lane kernels), random survivor orders, lost shards that are data,
    parity or survivors (unit rows), every block against the oracle."""
    fails = []
    with codec.options(**DECODE_KERNELS[kernel]):
        for k, m, e, s, l, want in band_ref(*band):
            rows = preset(s.shape[0], e * k)
            codec.decode_rows(k, m, dev(s), dev(l), rows)
            rc = sync_code(codec)
            if rc:
                fails.append("(%d,%d) e=%d: synchronize gave %d" % (k, m, e, rc))
            got = host(rows)
            for b in np.flatnonzero((got != want).any(axis=1)):
                fails.append("(k, m, e, block) = (%d, %d, %d, %d)" % (k, m, e, b))
    done(fails)


# ------------------------------------------------------------------ rebuild
def run_rebuild(codec, O, fails, label, k, m, S, s, l, at):
    sv, want = rebuild_case(O, k, m, S, s, l, at)
    n, e = l.shape
    g = Guarded("device")
    out = g.output("out", (n, e * S))
    codec.rebuild(k, m, g.input("surv_idx", s), g.input("surv", sv), g.input("lost_idx", l), out)
    raised_once(codec, fails, label)
    blocks_differ(fails, label, host(out), want, at)
    guards(fails, label, g, out=want)


def pick(entries, prefix):
    return [x for x in entries if x.label.startswith(prefix)]


@gpu
@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_rebuild_faults(codec, O, rebuild_path, k, m):
    """memo_ec_rebuild_batch on every device rebuild path.  S = 64: the
    catalogue ordered by tile slot (tiled), so the fused kernel meets a fault
    in the first and last group of its first pass, the first group of its
    second and of a late pass, and the tile's last block.  S = 4160 (a whole
    tile per shard: the images path forms table images in HBM): the last D,
    the first aliasing R and the last L between valid blocks.  out is guarded
    and preset 0xA5: a faulty block reads all zero, every other block is the
    true lost shards, ESINGULAR is raised once."""
    fails = []
    for e in es_of(k, m):
        s, l, at = tiled(k, m, e)
        run_rebuild(codec, O, fails, "rebuild[%s] rs(%d,%d) e=%d S=64" % (rebuild_path, k, m, e), k, m, 64, s, l, at)
        fs = faults(k, m, e)
        three = [pick(fs, "D(")[-1], aliasing(k, m, e)[0], pick(fs, "L(")[-1]]
        at = {2 * i + 1: x for i, x in enumerate(three)}
        s, l = place(k, m, e, 7, at)
        run_rebuild(codec, O, fails, "rebuild[%s] rs(%d,%d) e=%d S=4160" % (rebuild_path, k, m, e), k, m, 4160,
                    s, l, at)
    done(fails)


@gpu
@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_uniform_pattern_faults(codec, O, k, m):
    """Every fault as a shared pattern (host_decode_rows): rebuild_uniform and
    a uniform segment of rebuild_segments return ESINGULAR themselves and
    enqueue nothing (out still reads 0xA5, synchronize is clean); a valid
    pattern straight afterwards -- the base set and the controls in turn --
    rebuilds the true shards, so no refused pattern was cached."""
    from memo_amd import ec
    S, n = 64, 3
    data, par = shards(k, m, S, 8)
    data, par = data[:n], par[:n]
    fails = []
    for e in es_of(k, m):
        surv0, lost0, _ = base_set(k, m, e)
        good = [(surv0.astype(np.uint8), lost0.astype(np.uint8))] + [(x.surv, x.lost) for x in controls(k, m, e)]
        g = Guarded("device")
        sv0 = g.input("surv", O.gather(k, m, S, data, par, np.tile(good[0][0], (n, 1))))
        out = g.output("out", (n, e * S))
        for i, x in enumerate(faults(k, m, e)):
            label = "rs(%d,%d) e=%d %s" % (k, m, e, x.label)
            for name, call in (("rebuild_uniform", lambda: codec.rebuild_uniform(k, m, x.surv, sv0, x.lost, out)),
                               ("rebuild_segments", lambda: codec.rebuild_segments(
                                   [dict(k=k, m=m, surv_idx=x.surv, surv=sv0, lost_idx=x.lost, out=out,
                                         uniform=True)]))):
                try:
                    call()
                    fails.append("%s: %s returned OK" % (label, name))
                except ec.MemoECError as ex:
                    if ex.code != ESINGULAR:
                        fails.append("%s: %s gave %d" % (label, name, ex.code))
            su, lu = good[i % len(good)]
            o2 = preset(n, e * S)
            codec.rebuild_uniform(k, m, su, dev(O.gather(k, m, S, data, par, np.tile(su, (n, 1)))), lu, o2)
            rc = sync_code(codec)
            if rc:
                fails.append("%s: synchronize after the valid pattern gave %d" % (label, rc))
            if not np.array_equal(host(o2), O.gather(k, m, S, data, par, np.tile(lu, (n, 1)))):
                fails.append("%s: the valid pattern after it is rebuilt wrong" % label)
        guards(fails, "rs(%d,%d) e=%d: refused calls" % (k, m, e), g)  # out all 0xA5, guards whole
    done(fails)
