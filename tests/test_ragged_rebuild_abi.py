"""memo_ec_rebuild_ragged without a GPU: the symbol is exported and bound,
the version stays 2, a null ctx is refused, and Codec.rebuild_ragged refuses
bad arguments before the library is called (the Codec here has no ctx: a
call that reached the library would not raise ValueError)."""
import ctypes

import numpy as np
import pytest


def test_symbol_is_exported_and_bound():
    from memo_amd import ec
    assert "memo_ec_rebuild_ragged" in ec.EXPORTS
    assert hasattr(ctypes.CDLL(ec.LIB_PATH), "memo_ec_rebuild_ragged")
    L = ec._lib()
    assert L.memo_ec_rebuild_ragged.argtypes is not None and len(L.memo_ec_rebuild_ragged.argtypes) == 12
    assert L.memo_ec_version() == 2


def test_null_ctx_and_sizes_are_refused():
    from memo_amd import ec
    L = ec._lib()
    ok = (ctypes.c_size_t * 2)(64, 128)
    idx = (ctypes.c_uint8 * 32)()
    buf = (ctypes.c_uint8 * 4096)()
    call = L.memo_ec_rebuild_ragged
    assert call(None, 10, 4, 2, ok, idx, buf, idx, 1, 0, buf, ec.HOST) == -1
    assert call(None, 10, 4, 2, ok, idx, buf, idx, 1, 1, buf, ec.DEVICE) == -1
    # the sizes are judged before the ctx, as for the other ragged calls
    assert call(None, 10, 4, 2, (ctypes.c_size_t * 2)(64, 96), idx, buf, idx, 1, 0, buf, ec.HOST) == -1
    assert call(None, 10, 4, 2, None, idx, buf, idx, 1, 0, buf, ec.HOST) == -1
    assert call(None, 65, 4, 2, ok, idx, buf, idx, 1, 0, buf, ec.HOST) == -6   # k > MEMO_EC_MAX_K


@pytest.fixture
def c():
    from memo_amd import ec
    return ec.Codec.__new__(ec.Codec)  # no ctx: every check must raise before any call


def bufs(sizes, k=10, e=2):
    n, T = len(sizes), sum(sizes)
    return (np.zeros((n, k), np.uint8), np.zeros(k * T, np.uint8), np.zeros((n, e), np.uint8),
            np.zeros(e * T, np.uint8))


def test_wrapper_refuses_bad_sizes(c):
    si, s, li, o = bufs([64, 128])
    for sizes in ([64, 96], [64, 1 << 32], [64, -64], [64.0, 128.0]):
        with pytest.raises(ValueError):
            c.rebuild_ragged(10, 4, sizes, si, s, li, o)


def test_wrapper_refuses_short_buffers(c):
    sizes = [64, 128]
    si, s, li, o = bufs(sizes)
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, si, s[:-1], li, o)
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, si, s, li, o[:-1])
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, list(range(10)), s, [10, 11], o[:-1], uniform=True)


def test_wrapper_refuses_more_lost_shards_than_parity(c):
    sizes = [64, 128]
    si, s, li, o = bufs(sizes, e=5)
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, si, s, li, o)
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, list(range(10)), s, [10, 11, 12, 13, 9], o, uniform=True)


def test_wrapper_refuses_wrong_pattern_shapes(c):
    sizes = [64, 128]
    si, s, li, o = bufs(sizes)
    with pytest.raises(ValueError):                      # one row short
        c.rebuild_ragged(10, 4, sizes, si[:1], s, li, o)
    with pytest.raises(ValueError):
        c.rebuild_ragged(10, 4, sizes, si, s, li[:1], o)
    with pytest.raises(ValueError):                      # k columns wanted
        c.rebuild_ragged(10, 4, sizes, si[:, :9], s, li, o)
    with pytest.raises(ValueError):                      # flat where n x k is wanted
        c.rebuild_ragged(10, 4, sizes, si.reshape(-1), s, li, o)
    with pytest.raises(ValueError):                      # shared pattern: k survivors
        c.rebuild_ragged(10, 4, sizes, [0, 1, 2], s, [10, 11], o, uniform=True)
    with pytest.raises(ValueError):                      # per-block arrays passed as shared
        c.rebuild_ragged(10, 4, sizes, si, s, li, o, uniform=True)
