"""memo_ec_verify_batch without a GPU: the header declares it and the verdict
fields, the Python binding takes the words apart the same way, and the built
library carries the verify kernels under their own names."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def header():
    with open(os.path.join(ROOT, "include", "memo_ec.h")) as f:
        return f.read()


def test_header_declares_verify_and_verdict_fields():
    txt = header()
    decl = re.search(r"int\s+memo_ec_verify_batch\s*\(([^)]*)\)\s*;", txt)
    assert decl, "memo_ec_verify_batch not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("memo_ec_ctx *ctx, int k, int m, size_t S, size_t n, const uint8_t *data, "
                    "const uint8_t *parity, uint32_t *verdict, int where")
    assert re.search(r"#define\s+MEMO_EC_VERDICT_MASK\(v\)\s+\(\(uint32_t\)\(v\)\s*&\s*0xFFFFu\)", txt)
    assert re.search(r"#define\s+MEMO_EC_VERDICT_SHARD\(v\)\s+\(\(\(uint32_t\)\(v\)\s*>>\s*16\)\s*&\s*0xFFu\)", txt)
    assert re.search(r"#define\s+MEMO_EC_VERDICT_UNLOCATED\s+0xFFu", txt)
    assert re.search(r"#define\s+MEMO_EC_VERSION\s+2\b", txt)  # a backwards-compatible addition


def test_binding_exports_and_constants():
    from memo_amd import ec
    assert "memo_ec_verify_batch" in ec.EXPORTS
    assert ec.VERDICT_UNLOCATED == 0xFF
    lib = ctypes.CDLL(ec.LIB_PATH)
    assert hasattr(lib, "memo_ec_verify_batch")
    # argument checks come before any GPU work
    assert ec._lib().memo_ec_verify_batch(None, 10, 4, 64, 1, None, None, None, 2) == -1


def test_split_verdict_round_trips():
    from memo_amd import ec
    assert ec.split_verdict(0) == (0, 0)
    assert ec.split_verdict(0xF | (7 << 16)) == (0xF, 7)
    assert ec.split_verdict(0x4 | (0xFF << 16)) == (0x4, ec.VERDICT_UNLOCATED)
    for mask in [1, 2, 0x8000, 0xFFFF, 0x1234]:
        for shard in [0, 1, 63, 64, 79, ec.VERDICT_UNLOCATED]:
            w = mask | (shard << 16)  # the word as the header lays it out
            assert w < 1 << 24
            assert ec.split_verdict(w) == (mask, shard)
    # arrays: numpy uint32, and int32 words (what a torch tensor holds) read as unsigned
    words = np.array([0, 0xF | (3 << 16), 0x8000 | (0xFF << 16)], dtype=np.uint32)
    for arr in (words, words.view(np.int32)):
        mask, shard = ec.split_verdict(arr)
        assert mask.tolist() == [0, 0xF, 0x8000] and shard.tolist() == [0, 3, 0xFF]
    import torch
    mask, shard = ec.split_verdict(torch.from_numpy(words.view(np.int32).copy()))
    assert mask.tolist() == [0, 0xF, 0x8000] and shard.tolist() == [0, 3, 0xFF]


def test_verdict_buffer_checks():
    """The check Codec.verify puts every verdict buffer through: 32-bit words
    (numpy uint32 / torch int32), contiguous, at least n of them."""
    import torch
    from memo_amd import ec
    ptr, where = ec._ptr_words(np.zeros(4, np.uint32), 4)
    assert ptr and where == ec.HOST
    t = torch.zeros(6, dtype=torch.int32)
    assert ec._ptr_words(t, 4) == (t.data_ptr(), ec.HOST)
    for bad in (np.zeros(4, np.int64), np.zeros(4, np.uint8), torch.zeros(4, dtype=torch.int64), [0] * 4):
        with pytest.raises(TypeError):
            ec._ptr_words(bad, 4)
    for short in (np.zeros(3, np.uint32), torch.zeros(3, dtype=torch.int32),
                  torch.zeros(8, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError):
            ec._ptr_words(short, 4)


def test_library_has_the_verify_kernels():
    """gf_verify_kernel (its own name, so traces tell it from an encode) and
    verify_locate_kernel are in the gfx950 code object."""
    from memo_amd import ec
    with open(ec.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"gf_verify_kernel" in blob
    assert b"verify_locate_kernel" in blob
    # the instantiations of the bench's codes: <KC = 10 | 16, R = 4, NT>
    assert re.search(rb"_ZN7memo_ec16gf_verify_kernelILi10ELi4ELb1EEEvNS_9MacLaunchE", blob)
    assert re.search(rb"_ZN7memo_ec16gf_verify_kernelILi16ELi4ELb1EEEvNS_9MacLaunchE", blob)
