"""tests/mac_bodies.py against the sources, without a GPU: the codes of the
sweep reach exactly the compiled (KC, R) bodies and their forks, the dispatch
switches of ec_kernels.hip read as COMPILED, and edge_sizes() returns shard
sizes on opposite sides of the planner's flat / non-flat decision."""
import re

import pytest

import mac_bodies as B
from memo_amd import ec

PER_BLOCK_MODES = ("rows", "fused")


# ------------------------------------------------------------------ codes()
def test_codes_reach_exactly_the_compiled_bodies():
    codes = B.codes()
    assert len(codes) == len(set(codes)) == 180
    assert all(1 <= k <= ec.MAX_K and 1 <= r <= ec.MAX_M for k, r in codes)
    assert {B.body(k, r) for k, r in codes} == B.COMPILED
    assert len(B.COMPILED) == 52
    for KC in sorted({KC for KC, _ in B.COMPILED}):
        assert {B.body(k, r) for k, r in B.codes_of(KC)} == {b for b in B.COMPILED if b[0] == KC}


def test_every_padded_bound_runs_dense_and_padded():
    for KC, R in sorted(B.COMPILED):
        if R not in (6, 8, 12, 16):
            continue
        rs = {r for k, r in B.codes() if B.body(k, r) == (KC, R)}
        assert R in rs, (KC, R)
        assert any(r < R for r in rs), (KC, R)
        # the largest padding: one row more than the bound below
        below = max(b for b in B.row_bounds() if b < R)
        assert below + 1 in rs, (KC, R)


def test_every_straight_line_body_runs_at_k_equal_kc():
    for KC, R in sorted(B.COMPILED):
        if KC in (2, 3, 4, 10, 16):
            assert any(k == KC for k, r in B.codes() if B.body(k, r) == (KC, R)), (KC, R)
    # k = 6, 12, 14 have a body of their own up to R = 4 and fall to the
    # 4-shard chunk loop above it
    for k in (6, 12, 14):
        assert {B.body(k, r)[0] for _, r in B.codes() if r <= 4} == {k}
        assert {B.body(k, r)[0] for kk, r in B.codes() if kk == k and r > 4} == {4}


def test_the_chunk_loop_runs_every_tail():
    ks = {k for k, r in B.codes_of(4)}
    assert any(k < 4 for k in ks)
    for q in range(4):
        assert any(k > 4 and k % 4 == q for k in ks), q
    assert ec.MAX_K == 64 and 64 in ks
    # and each of those k at every row bound
    for k in ks:
        assert {B.body(k, r)[1] for kk, r in B.codes_of(4) if kk == k} >= \
            ({6, 8, 12, 16} if k in (6, 12, 14) else set(B.row_bounds())), k


# ------------------------------------------------------- the dispatch text
def function_body(text, name):
    """The text between the braces of the definition of `name` (the only
    place where the name is followed by a parenthesis: calls of the
    templates name their arguments in angle brackets first)."""
    at = [m.end() for m in re.finditer(r"\b%s\(" % re.escape(name), text)]
    assert len(at) == 1, (name, len(at))
    lo = text.index("{", at[0])
    depth = 0
    for i in range(lo, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[lo + 1:i]
    raise AssertionError("unbalanced braces after %s" % name)


def case_numbers(body):
    return [int(x) for x in re.findall(r"\bcase (\d+):", body)]


def macro_numbers(body):
    return [int(x) for x in re.findall(r"\bMEMO_EC_R\((\d+)\)", body)]


def test_function_body_and_tokens():
    text = "int f(int a) { switch (a) { case 1: case 22: return g<3>(a); } MEMO_EC_R(4) MEMO_EC_R(x) }\n" \
           "int h() { return f<1>(2); }"
    body = function_body(text, "f")
    assert body.strip().startswith("switch") and body.strip().endswith("MEMO_EC_R(x)")
    assert case_numbers(body) == [1, 22] and macro_numbers(body) == [4]
    with pytest.raises(AssertionError):
        function_body(text, "g")


def dispatched(text):
    """(the pairs launch_mac serves, the pairs launch_mac_ragged serves), read
    from the switch labels of ec_kernels.hip."""
    rows_all = set(macro_numbers(function_body(text, "launch_mac_r")))
    rows_r4 = set(case_numbers(function_body(text, "launch_mac_r4")))
    assert rows_all and rows_r4 and not macro_numbers(function_body(text, "launch_mac_r4"))
    mac = set()
    cases = re.findall(r"\bcase (\d+): return (launch_mac_r4?)<(\d+)>\(R,", function_body(text, "launch_mac"))
    assert len(cases) == len(case_numbers(function_body(text, "launch_mac")))
    for label, fn, arg in cases:
        assert label == arg
        mac |= {(int(arg), R) for R in (rows_all if fn == "launch_mac_r" else rows_r4)}
    # ragged: rows for every KC, then more rows for the KC of an `if constexpr`
    body = function_body(text, "launch_ragged_r")
    head, sep, tail = body.partition("if constexpr")
    assert sep
    rows_head, rows_tail = set(macro_numbers(head)), set(macro_numbers(tail))
    wide = {int(x) for x in re.findall(r"\bKC == (\d+)", tail)}
    assert rows_head and rows_tail and wide
    ragged = set()
    cases = re.findall(r"\bcase (\d+): return launch_ragged_r<(\d+)>\(R,", function_body(text, "launch_mac_ragged"))
    assert len(cases) == len(case_numbers(function_body(text, "launch_mac_ragged")))
    for label, arg in cases:
        assert label == arg
        KC = int(arg)
        ragged |= {(KC, R) for R in rows_head | (rows_tail if KC in wide else set())}
    return mac, ragged


def test_dispatch_text_matches_compiled():
    """Whoever adds or drops a body changes these switches: COMPILED, and
    with it the sweep of test_gpu_mac_bodies.py, has to follow."""
    mac, ragged = dispatched(B._text("ec_kernels.hip"))
    assert mac == B.COMPILED, sorted(mac ^ B.COMPILED)
    assert ragged == B.COMPILED, sorted(ragged ^ B.COMPILED)


def test_python_restatement_stays_inside_the_compiled_bodies():
    """ec.mac_rbound / ec.mac_kchunk over every code the ABI takes: a compiled
    body, enough rows, whole chunks.  (That the C++ functions agree is for
    the GPU: test_gpu_mac_bodies.test_every_code_has_a_body.)"""
    for k in range(1, ec.MAX_K + 1):
        for r in range(1, ec.MAX_M + 1):
            KC, R = B.body(k, r)
            assert (KC, R) in B.COMPILED, (k, r)
            assert r <= R and B.kpad(k, r) % KC == 0 and k <= B.kpad(k, r) < k + KC, (k, r)


# -------------------------------------------------------------- edge_sizes()
def test_constants_come_from_the_sources():
    c = B.constants()
    assert set(c) == {"MAC_TILE", "MAC_COEF_REGS", "MAC_TAB_REGS", "kLdsBudget"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    assert B._constant("constexpr size_t kX = 3 * 5u * 1024;", "kX") == 15360
    # the tile of guarded.py's guard arithmetic and of the shapes in the sweep
    assert c["MAC_TILE"] == B.LANES == 256


@pytest.mark.parametrize("mode", PER_BLOCK_MODES)
def test_flat_is_monotone_in_the_shard_size(mode):
    for k, r in B.codes():
        seen = [B.flat(mode, k, r, S) for S in range(64, B.S_TOP + 64, 64)]
        assert seen == sorted(seen), (k, r)  # False ... False True ... True
        # and past S_TOP nothing changes any more
        assert B.flat(mode, k, r, 1 << 20) == seen[-1] == B.flat(mode, k, r, (1 << 20) + 64), (k, r)


@pytest.mark.parametrize("mode", PER_BLOCK_MODES)
def test_edge_sizes_lie_on_both_sides_of_the_decision(mode):
    pairs = 0
    for k, r in B.codes():
        per = B.body(k, r)[1] * B.kpad(k, r)
        e = B.edge_sizes(mode, k, r)
        if 24 <= per <= 768:
            assert e is not None, (k, r, per)
        if e is None:
            assert len({B.flat(mode, k, r, S) for S in range(64, B.S_TOP + 64, 64)}) == 1, (k, r)
            continue
        lo, hi = e
        assert lo % 64 == 0 and hi % 64 == 0 and 64 <= lo and hi == lo + 64, (k, r, e)
        assert not B.flat(mode, k, r, lo) and B.flat(mode, k, r, hi), (k, r, e)
        pairs += 1
    assert pairs >= 100


def test_edge_sizes_at_the_ends_of_the_range():
    """R * kpad = 24 flips between 64 and 128 bytes, 576 and 768 between 4032
    and 4096; below 24 every size is flat, at 1024 none is."""
    def per(k, r):
        return B.body(k, r)[1] * B.kpad(k, r)
    assert per(4, 6) == 24 and B.edge_sizes("rows", 4, 6) == (64, 128)
    assert per(33, 16) == 576 and B.edge_sizes("fused", 33, 16) == (4032, 4096)
    assert per(64, 12) == 768 and B.edge_sizes("rows", 64, 12) == (4032, 4096)
    assert per(10, 2) == 20 and B.edge_sizes("rows", 10, 2) is None and B.flat("rows", 10, 2, 64)
    assert per(64, 16) == 1024 and B.edge_sizes("fused", 64, 16) is None
    assert not B.flat("fused", 64, 16, 1 << 20)


def test_images_span_blocks_up_to_64_slots():
    """Per-block table images at whole-tile shards: a tile across two blocks
    stages both sets in registers up to R * kpad = 64, tiles stay inside a
    block above it (the two image shapes of the sweep)."""
    for k, r in B.codes():
        per = B.body(k, r)[1] * B.kpad(k, r)
        for S in (4096, 4160):
            assert B.flat("images", k, r, S) == (per <= 64), (k, r, S)
