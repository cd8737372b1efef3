"""memo_ec_encode_ragged / memo_ec_verify_ragged without a GPU: the header
declares both with the agreed argument lists, the binding and the built
library carry them and the three ragged kernels, argument errors return
before any GPU work, and the layout arithmetic is the documented one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ragged_cases as RC


def header():
    with open(os.path.join(ROOT, "include", "memo_ec.h")) as f:
        return f.read()


def declared_args(name):
    decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert decl, "%s not declared" % name
    return " ".join(decl.group(1).split())


def test_header_declares_both_calls():
    assert declared_args("memo_ec_encode_ragged") == (
        "memo_ec_ctx *ctx, int k, int m, size_t n, const size_t *sizes, "
        "const uint8_t *data, uint8_t *parity, int where")
    assert declared_args("memo_ec_verify_ragged") == (
        "memo_ec_ctx *ctx, int k, int m, size_t n, const size_t *sizes, "
        "const uint8_t *data, const uint8_t *parity, uint32_t *verdict, int where")
    txt = header()
    assert re.search(r"#define\s+MEMO_EC_VERSION\s+2\b", txt)  # a compatible addition
    assert re.search(r"cannot be captured into a HIP graph", " ".join(txt.split()).replace("* ", ""))


def test_binding_and_library_export_both():
    from memo_amd import ec
    lib = ctypes.CDLL(ec.LIB_PATH)
    for name in ("memo_ec_encode_ragged", "memo_ec_verify_ragged"):
        assert name in ec.EXPORTS
        assert hasattr(lib, name), name
    for attr in ("encode_ragged", "verify_ragged"):
        assert callable(getattr(ec.Codec, attr))
    assert ec._lib().memo_ec_version() == 2


def test_library_has_the_ragged_kernels():
    from memo_amd import ec
    with open(ec.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    # <KC = 10 | 16, R = 4, NT> of the encode and the verify, and the locate pass
    for kc in (10, 16):
        assert re.search(rb"_ZN7memo_ec20gf_mac_ragged_kernelILi%dELi4ELb1EEEvNS_12RaggedLaunchE" % kc, blob)
        assert re.search(rb"_ZN7memo_ec23gf_verify_ragged_kernelILi%dELi4ELb1EEEvNS_12RaggedLaunchE" % kc, blob)
    assert re.search(rb"_ZN7memo_ec27verify_locate_ragged_kernelILi16EEEvNS_16RaggedLocateArgsE", blob)
    assert re.search(rb"_ZN7memo_ec27verify_locate_ragged_kernelILi64EEEvNS_16RaggedLocateArgsE", blob)


def test_build_id_covers_the_planning_header():
    from memo_amd import ec
    names = [os.path.basename(p) for p in ec.BUILD_SOURCES]
    assert "ragged_plan.h" in names
    mk = open(os.path.join(ROOT, "memo_amd", "csrc", "Makefile")).read()
    ids = re.search(r"^ID_SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert [os.path.basename(p) for p in ids] == names  # same sources, same order


def test_argument_errors_come_before_any_gpu_work():
    """With a NULL ctx nothing can be enqueued: every refusal below is the
    host's.  The sizes are judged first (MEMO_EC_ERANGE = -6 shows through a
    NULL ctx), then the ctx (MEMO_EC_EINVAL = -1)."""
    from memo_amd import ec
    L = ec._lib()

    def both(k, m, n, sz):
        a = L.memo_ec_encode_ragged(None, k, m, n, sz, None, None, ec.DEVICE)
        b = L.memo_ec_verify_ragged(None, k, m, n, sz, None, None, None, ec.DEVICE)
        assert a == b
        return a

    ok = (ctypes.c_size_t * 3)(64, 128, 0)
    assert both(10, 4, 3, ok) == -1                       # valid sizes: the NULL ctx
    assert both(10, 4, 3, None) == -1                     # NULL sizes with n > 0
    for bad in (1, 65, 4096 + 16, 1 << 32, (1 << 32) + 64):
        assert both(10, 4, 3, (ctypes.c_size_t * 3)(64, bad, 128)) == -1, bad
    assert both(65, 4, 3, ok) == -6                       # k > MEMO_EC_MAX_K, as the uniform calls
    big = (1 << 32) - 64                                  # the largest valid size
    many = (ctypes.c_size_t * 4097)(*([big] * 4097))      # T just above 2^44
    assert both(64, 16, 4097, many) == -6                 # k * T >= 2^50
    assert both(1, 1, 4097, many) == -1                   # in range: the NULL ctx again
    many[4096] = 65
    assert both(64, 16, 4097, many) == -1                 # an invalid size wins over the range


def test_ragged_offsets_on_C():
    from memo_amd import ec
    off = ec.ragged_offsets(RC.C)
    assert off.dtype == np.uint64
    assert off.tolist() == [0, 4032, 4096, 8256, 16512, 16576, 16576, 16768, 16768]
    assert off.tolist() == RC.offsets(RC.C)
    assert ec.ragged_offsets([]).tolist() == [0]
    with pytest.raises(ValueError):
        ec.ragged_offsets([64, -64])


@pytest.mark.parametrize("sizes", [RC.F1, RC.F2], ids=["100x192", "7x4160"])
def test_uniform_sizes_give_the_uniform_layout(sizes):
    """With every S[b] equal, shard j of block b sits where the (n, k, S)
    array of memo_ec_encode_batch has it, data and parity alike."""
    from memo_amd import ec
    n, S = len(sizes), sizes[0]
    off = ec.ragged_offsets(sizes)
    for per in (10, 4):
        flat = np.arange(n * per * S, dtype=np.int64)
        cube = flat.reshape(n, per, S)
        for b in (0, 1, n // 2, n - 1):
            for j in (0, per - 1):
                lo = per * int(off[b]) + j * S
                assert np.array_equal(flat[lo:lo + S], cube[b, j])
                assert np.array_equal(RC.shard(flat, per, sizes, b, j), cube[b, j])
    assert int(off[-1]) == n * S


def test_binding_checks_buffer_lengths():
    """Codec.encode_ragged refuses buffers shorter than the sizes need before
    it calls the library (no ctx here: the check must come first)."""
    from memo_amd import ec
    c = ec.Codec.__new__(ec.Codec)
    with pytest.raises(ValueError):
        c.encode_ragged(10, 4, [64, 128], np.zeros(10 * 192 - 1, np.uint8), np.zeros(4 * 192, np.uint8))
    with pytest.raises(ValueError):
        c.encode_ragged(10, 4, [64, 128], np.zeros(10 * 192, np.uint8), np.zeros(4 * 192 - 1, np.uint8))
