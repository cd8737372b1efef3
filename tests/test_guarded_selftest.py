"""The guarded-buffer harness (tests/guarded.py) can fail: a fake call on
pageable buffers that commits each kind of violation is caught, with the
buffer, the side and the offsets named, and a fake call that commits none
passes.  No GPU: the comparison is a pure function over numpy arrays, and
this is the evidence for it that tests/test_gpu_bounds.py rests on."""
import numpy as np
import pytest

import guarded
from guarded import FILL, GUARD, Guarded

N_IN, N_OUT = 640, 256


def setup():
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, N_IN, dtype=np.uint8)
    want = (data[:N_OUT] ^ 0x5C).astype(np.uint8)
    want[want == FILL] ^= 1  # a correct output byte that equals the preset proves nothing
    g = Guarded("pageable")
    src = g.input("data", data)
    dst = g.output("parity", N_OUT)
    return g, src, dst, want


def good_call(g, dst, want):
    dst[:] = want


def test_pattern_is_not_constant_and_not_the_fill():
    p = guarded.pattern(GUARD)
    assert GUARD == 8192 and GUARD % 64 == 0
    assert len(set(p.tolist())) == 256
    assert p[0] == 11 and p[1] == 48 and p[7] == (37 * 7 + 11) & 0xFF
    # no run of the pattern reads as preset output bytes
    assert not np.any((p[:-1] == FILL) & (p[1:] == FILL))


def test_layout():
    g, src, dst, want = setup()
    for name, view in (("data", src), ("parity", dst)):
        b = g.bufs[name]
        assert view.ctypes.data % 64 == 0
        assert np.shares_memory(view, b.raw)
        assert b.lo >= GUARD and b.end - b.lo - view.size == GUARD
        assert np.array_equal(b.raw[:b.lo], guarded.pattern(b.lo))
        assert np.array_equal(b.raw[b.end - GUARD:b.end], guarded.pattern(GUARD))
    assert np.all(dst == FILL)
    assert Guarded("pageable").input("x", np.zeros(64, np.uint8), shift=17).ctypes.data % 64 == 17


def test_clean_call_passes():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    g.check(parity=want)


def test_untouched_output_must_be_named_or_stay_preset():
    g, src, dst, want = setup()
    g.check()  # nothing written, nothing expected
    good_call(g, dst, want)
    with pytest.raises(AssertionError, match="parity: output payload is not the expected bytes"):
        g.check()


def test_one_byte_before_the_payload_is_caught():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    b = g.bufs["parity"]
    b.raw[b.lo - 1] ^= 0xFF
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    msg = str(ei.value)
    assert "parity: guard before the payload written: 1 byte(s) differ, first at -1, last at -1" in msg
    assert "data:" not in msg and "after" not in msg and "output payload" not in msg


def test_sixteen_bytes_after_the_payload_are_caught():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    b = g.bufs["parity"]
    hi = b.lo + N_OUT
    b.raw[hi:hi + 16] ^= 0xFF  # one column's worth of stores past the end
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    msg = str(ei.value)
    assert "parity: guard after the payload written: 16 byte(s) differ, first at 0, last at 15" in msg
    assert "before" not in msg and "data:" not in msg


def test_last_guard_byte_is_looked_at():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    b = g.bufs["data"]
    b.raw[b.end - 1] ^= 1
    b.raw[0] ^= 1
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    msg = str(ei.value)
    assert "data: guard after the payload written: 1 byte(s) differ, first at %d, last at %d" % (
        GUARD - 1, GUARD - 1) in msg
    assert "data: guard before the payload written: 1 byte(s) differ, first at %d" % -b.lo in msg


def test_flipped_input_byte_is_caught():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    src[100] ^= 0x01
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    msg = str(ei.value)
    assert "data: input payload changed: 1 byte(s) differ, first at 100, last at 100" in msg
    assert "parity" not in msg


def test_output_byte_left_at_the_preset_is_caught():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    dst[N_OUT - 1] = FILL
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    msg = str(ei.value)
    assert "parity: output payload is not the expected bytes: 1 byte(s) differ, first at %d, last at %d" % (
        N_OUT - 1, N_OUT - 1) in msg
    assert "got 0xA5" in msg and "guard" not in msg


def test_every_violation_is_reported_at_once():
    g, src, dst, want = setup()
    good_call(g, dst, want)
    b = g.bufs["parity"]
    b.raw[b.lo - 1] ^= 0xFF
    b.raw[b.lo + N_OUT + 4095] ^= 0xFF
    src[0] ^= 0x80
    dst[3] ^= 0x10
    with pytest.raises(AssertionError) as ei:
        g.check(parity=want)
    assert len(str(ei.value).splitlines()) == 4


def test_words_view_and_wrong_names():
    g = Guarded("pageable")
    g.output("verdict", 12)
    w = g.words("verdict")
    assert w.dtype == np.uint32 and w.size == 3 and np.all(w == 0xA5A5A5A5)
    w[:] = 0
    g.check(verdict=np.zeros(3, np.uint32))
    with pytest.raises(AssertionError):
        g.check(nosuch=np.zeros(3, np.uint32))
    with pytest.raises(AssertionError):
        g.check(verdict=np.zeros(2, np.uint32))  # the expected bytes cover the whole payload
