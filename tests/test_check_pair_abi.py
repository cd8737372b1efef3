"""memo_ec_check_pair_batch without a GPU: the header declares it and its two
macros, the binding exports it, every argument error of memo_ec_check_batch
comes back before the ctx is touched (the ctx here is a zeroed buffer no
device call could survive), and the built library carries check_pair_kernel
under its own name."""
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


def test_header_declares_the_call_and_its_macros():
    txt = header()
    decl = re.search(r"int\s+memo_ec_check_pair_batch\s*\(([^)]*)\)\s*;", txt)
    assert decl, "memo_ec_check_pair_batch not declared"
    assert " ".join(decl.group(1).split()) == (
        "memo_ec_ctx *ctx, int k, int m, int x, size_t S, size_t n, const uint8_t *have_idx, "
        "const uint8_t *have, uint32_t *verdict, int where")
    assert re.search(r"#define\s+MEMO_EC_VERDICT_HAS_PAIR\(v\)", txt)
    assert re.search(r"#define\s+MEMO_EC_VERDICT_SHARD2\(v\)", txt)
    assert re.search(r"#define\s+MEMO_EC_VERSION\s+2\b", txt)  # a backwards-compatible addition
    assert "not a proof" in txt[txt.index("TWO wrong"):decl.start()]


def test_macros_compile_to_the_documented_bits(tmp_path):
    """The two macros, compiled from the header itself by the host compiler."""
    import subprocess
    from test_ragged_plan import compiler
    src = tmp_path / "macros.c"
    src.write_text('#include <stdio.h>\n#include "memo_ec.h"\n'
                   "int main(void) {\n"
                   "  unsigned w[] = {0u, 0x00FF000Fu, 0x0003000Fu, 0x0103000Fu, 0xFFFFFFFFu,\n"
                   "                  0xFu | (3u << 16) | (14u << 25), 0x3u | (0u << 16) | (80u << 25)};\n"
                   "  for (unsigned i = 0; i < sizeof w / sizeof *w; ++i)\n"
                   '    printf("%d %u %u\\n", MEMO_EC_VERDICT_HAS_PAIR(w[i]) ? 1 : 0,\n'
                   "           MEMO_EC_VERDICT_HAS_PAIR(w[i]) ? MEMO_EC_VERDICT_SHARD2(w[i]) : 0u,\n"
                   "           MEMO_EC_VERDICT_SHARD(w[i]));\n"
                   "  return 0;\n}\n")
    exe = str(tmp_path / "macros")
    cc = compiler()[0]
    subprocess.check_call([cc, "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")[:7]
    assert out == ["0 0 0", "0 0 255", "0 0 3", "0 0 3", "0 0 255", "1 13 3", "1 79 0"]


def test_binding_exports_and_source_list():
    from memo_amd import ec
    assert "memo_ec_check_pair_batch" in ec.EXPORTS
    assert hasattr(ctypes.CDLL(ec.LIB_PATH), "memo_ec_check_pair_batch")
    assert callable(ec.Codec.check_pair) and callable(ec.split_verdict_pair)
    names = [os.path.basename(p) for p in ec.BUILD_SOURCES]
    assert "check_pair_logic.h" in names
    with open(os.path.join(ROOT, "memo_amd", "csrc", "Makefile")) as f:
        ids = re.search(r"^ID_SRCS := (.*)$", f.read(), re.M).group(1).split()
    assert [os.path.basename(p) for p in ids] == names  # one order: build_id() == source_id()


@pytest.fixture(scope="module")
def call():
    """memo_ec_check_pair_batch over a ctx that is 4 KiB of zeros: an argument
    error has to come back before anything reads it."""
    from memo_amd import ec
    fake = ctypes.create_string_buffer(4096)
    fn = ec._lib().memo_ec_check_pair_batch

    def f(k=10, m=4, x=4, S=64, n=1, idx=0x1000, have=0x1000, verdict=0x1000, where=DEVICE, ctx=True):
        return fn(ctypes.addressof(fake) if ctx else None, k, m, x, S, n, idx or None, have or None,
                  verdict or None, where)
    return f


def test_null_ctx(call):
    assert call(ctx=False) == EINVAL
    assert call(ctx=False, x=0) == EINVAL


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


def test_errors_come_in_the_checks_order(call):
    """Where two things are wrong, the answer is memo_ec_check_batch's."""
    from memo_amd import ec
    fake = ctypes.create_string_buffer(4096)
    chk = ec._lib().memo_ec_check_batch
    for kw in [dict(k=65, x=9), dict(k=65, where=9), dict(x=9, where=9), dict(S=65, n=1 << 60),
               dict(S=1 << 32, have=0x1001), dict(m=17, x=-1), dict(x=0, k=65), dict(n=0, S=1 << 32)]:
        a = dict(k=10, m=4, x=4, S=64, n=1, idx=0x1000, have=0x1000, verdict=0x1000, where=DEVICE)
        a.update(kw)
        want = chk(ctypes.addressof(fake), a["k"], a["m"], a["x"], a["S"], a["n"], a["idx"], a["have"],
                   a["verdict"], a["where"])
        assert call(**kw) == want, kw


def test_empty_calls_return_ok_and_touch_nothing(call):
    assert call(x=0) == 0
    assert call(x=0, idx=0, have=0, verdict=0) == 0
    assert call(n=0) == 0
    assert call(n=0, idx=0, have=0, verdict=0, S=0) == 0
    assert call(x=0, S=65) == 0  # nothing to judge: as the check, the rest is not looked at


def test_codec_check_pair_refuses_bad_buffers_before_the_library():
    from memo_amd import ec
    c = ec.Codec.__new__(ec.Codec)  # no ctx: every check must raise before any call
    idx = np.tile(np.arange(14, dtype=np.uint8), (3, 1))
    have = np.zeros((3, 14 * 64), np.uint8)
    with pytest.raises(ValueError):
        c.check_pair(10, 4, idx.reshape(-1), have)                       # flat have_idx, no x
    with pytest.raises(ValueError):
        c.check_pair(10, 4, np.zeros((3, 15), np.uint8), have)           # x > m
    with pytest.raises(ValueError):
        c.check_pair(10, 4, idx, have[:, :-1].copy())                    # not n x (k + x) shards
    with pytest.raises(ValueError):
        c.check_pair(10, 4, idx, have, verdict=np.zeros(2, np.uint32))   # verdict too short
    with pytest.raises(TypeError):
        c.check_pair(10, 4, idx.astype(np.int32), have)


def test_library_has_the_pair_kernel():
    """check_pair_kernel, both instantiations, in the gfx950 code object."""
    from memo_amd import ec
    with open(ec.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"_ZN7memo_ec17check_pair_kernelILi16EEEvNS_9CheckArgsE" in blob
    assert b"_ZN7memo_ec17check_pair_kernelILi64EEEvNS_9CheckArgsE" in blob
