"""memo_ec_correct_pair_batch without a GPU: the header declares it and adds no
macro, the binding exports it, every argument error of memo_ec_check_batch
comes back the same way before the ctx is touched (the ctx here is a zeroed
buffer no device call could survive), Codec.correct_pair refuses bad buffers
before the library, the new plan header has its place in both source lists,
and the built library carries the call's two kernels under their own names."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

EINVAL, ERANGE = -1, -6
HOST, PINNED, DEVICE = 0, 1, 2


def header():
    with open(os.path.join(ROOT, "include", "memo_ec.h")) as f:
        return f.read()


def test_header_declares_the_call_and_no_new_macro():
    txt = header()
    decl = re.search(r"int\s+memo_ec_correct_pair_batch\s*\(([^)]*)\)\s*;", txt)
    assert decl, "memo_ec_correct_pair_batch not declared"
    assert " ".join(decl.group(1).split()) == (
        "memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n, const uint8_t *have_idx, "
        "uint8_t *have, uint32_t *verdict, int where")
    assert re.search(r"#define\s+MEMO_EC_VERSION\s+2\b", txt)  # a backwards-compatible addition
    macros = sorted(set(re.findall(r"#define\s+(MEMO_EC_VERDICT_\w+)", txt)))
    assert macros == ["MEMO_EC_VERDICT_CORRECTED", "MEMO_EC_VERDICT_HAS_PAIR", "MEMO_EC_VERDICT_INVALID",
                      "MEMO_EC_VERDICT_MASK", "MEMO_EC_VERDICT_SHARD", "MEMO_EC_VERDICT_SHARD2",
                      "MEMO_EC_VERDICT_UNLOCATED"]


def test_binding_exports_and_sources():
    from memo_amd import correct_pair_ref, ec
    assert "memo_ec_correct_pair_batch" in ec.EXPORTS
    assert hasattr(ctypes.CDLL(ec.LIB_PATH), "memo_ec_correct_pair_batch")
    assert ec._lib().memo_ec_version() == 2
    assert callable(ec.Codec.correct_pair)
    assert correct_pair_ref.VERDICT_CORRECTED == 1 << 24
    names = [os.path.basename(p) for p in ec.BUILD_SOURCES]
    assert names.index("correct_pair_plan.h") == names.index("check_pair_logic.h") + 1
    assert names.index("correct_plan.h") == names.index("check_plan.h") + 1
    with open(os.path.join(ROOT, "memo_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    ids = re.search(r"^ID_SRCS := (.*)$", mk, re.M).group(1).split()
    assert [os.path.basename(p) for p in ids] == names  # one order: build_id() == source_id()
    for rule in re.findall(r"^\S*ec_kernels\.o: (.*)$", mk, re.M):
        assert "correct_pair_plan.h" in rule.split()
    assert ec.source_id() == ec.build_id()


@pytest.fixture(scope="module")
def call():
    """memo_ec_correct_pair_batch over a ctx that is 4 KiB of zeros: an
    argument error has to come back before anything reads it."""
    from memo_amd import ec
    fake = ctypes.create_string_buffer(4096)
    fn = ec._lib().memo_ec_correct_pair_batch

    def f(k=10, m=4, x=4, S=64, n=1, idx=0x1000, have=0x1000, verdict=0x1000, where=DEVICE, ctx=True):
        return fn(ctypes.addressof(fake) if ctx else None, k, m, x, S, n, idx or None, have or None,
                  verdict or None, where)
    return f


def test_null_ctx(call):
    assert call(ctx=False) == EINVAL
    assert call(ctx=False, x=0) == EINVAL


# the cases of tests/test_check_abi.py, one for one
@pytest.mark.parametrize("kw", [
    dict(x=-1), dict(x=5), dict(m=0, x=1),
    dict(S=65), dict(S=32), dict(S=4096 + 16),
    dict(idx=0), dict(verdict=0), dict(have=0),
    dict(have=0x1008), dict(have=0x1008, where=PINNED), dict(have=0x1001, where=PINNED),
    dict(verdict=0x1002), dict(verdict=0x1002, where=HOST), dict(verdict=0x1001, where=PINNED),
    dict(where=3), dict(where=-1), dict(where=3, x=0), dict(where=7, n=0),
    dict(k=0), dict(m=-1),
], ids=lambda kw: "_".join("%s%s" % (a, hex(b) if b > 255 else b) for a, b in kw.items()))
def test_einval_before_any_device_work(call, kw):
    assert call(**kw) == EINVAL


@pytest.mark.parametrize("kw", [
    dict(k=65), dict(m=17, x=1), dict(S=1 << 32), dict(S=(1 << 32) + 64),
    dict(S=1 << 20, n=(1 << 30) // 14 + 1),          # n * (k + x) * S just past 2^50
    dict(S=0, have=0, n=(1 << 50) // 14 + 1),        # S == 0: the index rows alone
], ids=["k", "m", "S", "S_64", "bytes", "index_bytes"])
def test_erange_before_any_device_work(call, kw):
    assert call(**kw) == ERANGE


def test_empty_calls_return_ok_and_touch_nothing(call):
    assert call(x=0) == 0
    assert call(x=0, idx=0, have=0, verdict=0) == 0
    assert call(n=0) == 0
    assert call(n=0, idx=0, have=0, verdict=0, S=0) == 0
    assert call(x=0, S=65) == 0  # nothing to judge: as the check, the rest is not looked at


def test_same_answers_as_the_check_and_the_correction(call):
    """Argument for argument the calls agree, the order of the checks
    included (two errors at once give the first one's code)."""
    from memo_amd import ec
    fake = ctypes.create_string_buffer(4096)
    for other in (ec._lib().memo_ec_check_batch, ec._lib().memo_ec_correct_batch, ec._lib().memo_ec_check_pair_batch):
        for kw in [dict(x=5), dict(S=65), dict(have=0x1008), dict(verdict=0x1002), dict(where=3), dict(k=65),
                   dict(S=1 << 32), dict(x=0), dict(n=0), dict(S=0, have=0, n=(1 << 50) // 14 + 1),
                   dict(k=65, x=5), dict(x=5, where=3), dict(where=3, S=65), dict(S=65, k=65),
                   dict(S=1 << 32, have=0x1008), dict(S=(1 << 32) + 1), dict(m=17, where=9)]:
            a = dict(k=10, m=4, x=4, S=64, n=1, idx=0x1000, have=0x1000, verdict=0x1000, where=DEVICE)
            a.update(kw)
            want = other(ctypes.addressof(fake), a["k"], a["m"], a["x"], a["S"], a["n"], a["idx"] or None,
                         a["have"] or None, a["verdict"] or None, a["where"])
            assert call(**kw) == want, kw


def no_ctx():
    from memo_amd import ec
    return ec.Codec.__new__(ec.Codec)  # no ctx: every check must raise before any call


def test_codec_correct_pair_refuses_bad_buffers_before_the_library():
    c = no_ctx()
    idx = np.tile(np.arange(14, dtype=np.uint8), (3, 1))
    have = np.zeros((3, 14 * 64), np.uint8)
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx.reshape(-1), have)                       # flat have_idx, no x
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, np.zeros((3, 15), np.uint8), have)           # x > m
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx[:, :9], have)                            # x < 0
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx, have[:, :-1].copy())                    # not n x (k + x) shards
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx, have, S=128)                            # have too short for S
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx, have, n=4)                              # have_idx too short for n
    with pytest.raises(ValueError):
        c.correct_pair(10, 4, idx, have, verdict=np.zeros(2, np.uint32))   # verdict too short
    with pytest.raises(TypeError):
        c.correct_pair(10, 4, idx, have, verdict=np.zeros(3, np.int64))
    with pytest.raises(TypeError):
        c.correct_pair(10, 4, idx.astype(np.int32), have)


def test_library_has_the_two_kernels():
    """correct_pair_list_kernel and gf_correct_pair_kernel, the latter for the
    eight shard chunks the MAC is compiled for, are in the gfx950 code object."""
    from memo_amd import ec
    with open(ec.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"_ZN7memo_ec24correct_pair_list_kernelENS_15CorrectPairArgsE" in blob
    for kc in (2, 3, 4, 6, 10, 12, 14, 16):
        assert b"_ZN7memo_ec22gf_correct_pair_kernelILi%dEEEvNS_15CorrectPairArgsE" % kc in blob, kc
    for kc in (1, 5, 8):
        assert b"_ZN7memo_ec22gf_correct_pair_kernelILi%dEEEvNS_15CorrectPairArgsE" % kc not in blob, kc
