"""Guarded buffers: every buffer of a call sits inside one larger allocation,

    [ guard | payload | guard ]

so that a store past either end of the payload lands in bytes the test owns
and looks at, instead of in a neighbour the caching allocator handed out.

Each guard is GUARD = 8192 bytes: two 256-column tiles of one output row
(256 x 16 bytes each), i.e. the largest group of stores one tile makes to a
row, with a tile to spare.  It is a multiple of 64, and the payload starts
on a 64-byte boundary (plus `shift`, for the calls that must work at any
byte address).  A guard holds the position-dependent pattern
(37 * i + 11) & 0xFF, which is neither constant nor 0xA5; output payloads
are preset to FILL = 0xA5, input payloads hold the test data.

The same description gives device tensors, pinned host tensors and pageable
numpy arrays (Guarded(memory) / the `memory` of one buffer).  After the call
Guarded.check() asserts that every guard still holds its pattern, that every
input payload holds what was put in and that every output payload equals the
expected bytes; a failure names the buffer, the side and the first and last
offending offsets.  The comparison itself (violations) is a pure function
over numpy arrays: tests/test_guarded_selftest.py runs it without a GPU."""
import numpy as np

GUARD = 8192
FILL = 0xA5
MEMORIES = ("device", "pinned", "pageable")


def pattern(n):
    """The guard bytes: (37 * i + 11) & 0xFF for i < n."""
    return ((37 * np.arange(n, dtype=np.int64) + 11) & 0xFF).astype(np.uint8)


def _span(bad):
    return "%d byte(s) differ, first at %d, last at %d" % (bad.size, bad[0], bad[-1])


def violations(name, raw, lo, want, role):
    """What is wrong with one buffer after a call, as a list of messages
    (empty: nothing).  raw: the whole allocation (uint8), with the payload at
    [lo, lo + want.size), the pattern's first lo bytes before it and its
    first raw.size - lo - want.size bytes after it.  want: the bytes the
    payload must hold (an input's data, an output's expected result); role:
    "input" or "output", for the message.  Offsets in a message count from
    the payload's first byte (before-guard: negative) or, for the
    after-guard, from the first byte past the payload."""
    raw = np.asarray(raw).reshape(-1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    hi = lo + want.size
    assert raw.dtype == np.uint8 and 0 < lo and hi < raw.size
    out = []
    bad = np.flatnonzero(raw[:lo] != pattern(lo))
    if bad.size:
        out.append("%s: guard before the payload written: %s" % (name, _span(bad - lo)))
    bad = np.flatnonzero(raw[hi:] != pattern(raw.size - hi))
    if bad.size:
        out.append("%s: guard after the payload written: %s" % (name, _span(bad)))
    bad = np.flatnonzero(raw[lo:hi] != want)
    if bad.size:
        what = "input payload changed" if role == "input" else "output payload is not the expected bytes"
        at = int(bad[0])
        out.append("%s: %s: %s (got 0x%02X, want 0x%02X at %d)"
                   % (name, what, _span(bad), raw[lo + at], want[at], at))
    return out


def assert_clean(records):
    """records: (name, raw, lo, want, role) per buffer; raises AssertionError
    listing every violation of every buffer."""
    msgs = [m for r in records for m in violations(*r)]
    assert not msgs, "\n".join(msgs)


class _Buf:
    def __init__(self, name, role, memory, payload, shift):
        self.name, self.role, self.memory = name, role, memory
        payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.put = payload.copy()
        n = payload.size
        # 64 spare bytes: the payload is put on a 64-byte boundary (+ shift)
        # whatever the allocation's own alignment
        total = 64 + GUARD + shift + n + GUARD
        if memory == "pageable":
            self.raw = np.empty(total, dtype=np.uint8)
            base = self.raw.ctypes.data
        else:
            import torch
            self.raw = (torch.empty(total, dtype=torch.uint8, device="cuda") if memory == "device"
                        else torch.empty(total, dtype=torch.uint8).pin_memory())
            base = self.raw.data_ptr()
        pad = (-(base + GUARD)) % 64
        self.lo = pad + GUARD + shift
        self.end = self.lo + n + GUARD  # bytes of raw that are guard or payload
        assert (base + self.lo) % 64 == shift % 64
        image = np.concatenate([pattern(self.lo), payload, pattern(GUARD)])
        if memory == "pageable":
            self.raw[:self.end] = image
        elif memory == "device":
            self.raw[:self.end].copy_(torch.from_numpy(image))
        else:
            self.raw[:self.end].numpy()[:] = image

    def view(self):
        return self.raw[self.lo:self.end - GUARD]

    def snapshot(self):
        if self.memory == "pageable":
            return self.raw[:self.end].copy()
        return self.raw[:self.end].cpu().numpy().copy()


class Guarded:
    """The buffers of one call.  input() and output() return the payload as
    a uint8 view (torch tensor or numpy array) to hand to the call; check()
    judges every buffer made so far."""

    def __init__(self, memory="device"):
        assert memory in MEMORIES
        self.memory = memory
        self.bufs = {}

    def _add(self, name, role, payload, memory, shift, shape):
        assert name not in self.bufs, name
        b = _Buf(name, role, memory or self.memory, payload, shift)
        self.bufs[name] = b
        v = b.view()
        return v.reshape(shape) if isinstance(v, np.ndarray) else v.view(shape)

    def input(self, name, data, memory=None, shift=0):
        """A buffer the call only reads, holding `data`; `shift` moves the
        payload off its 64-byte boundary.  The view has data's shape for
        uint8 data and is flat bytes for any other dtype."""
        data = np.asarray(data)
        shape = data.shape if data.dtype == np.uint8 else (data.nbytes,)
        return self._add(name, "input", data, memory, shift, shape)

    def output(self, name, shape, memory=None, shift=0):
        """A uint8 buffer of `shape` (an int or a tuple) the call writes,
        preset to FILL."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        return self._add(name, "output", np.full(int(np.prod(shape)), FILL, np.uint8), memory, shift, shape)

    def words(self, name):
        """The payload of `name` as 32-bit words, for a verdict array (torch
        int32 / numpy uint32, as memo_amd.ec takes them)."""
        v = self.bufs[name].view()
        if isinstance(v, np.ndarray):
            return v.view(np.uint32)
        import torch
        return v.view(torch.int32)

    def check(self, **expected):
        """expected: name = the bytes an output payload must hold now (any
        dtype or shape, compared as bytes); an output not named must still
        be all FILL.  Inputs must hold what was put in, guards their
        pattern."""
        unknown = set(expected) - set(self.bufs)
        assert not unknown, unknown
        recs = []
        for b in self.bufs.values():
            assert b.role == "output" or b.name not in expected, b.name
            want = expected.get(b.name, b.put)
            want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
            assert want.size == b.put.size, (b.name, want.size, b.put.size)
            recs.append((b.name, b.snapshot(), b.lo, want, b.role))
        assert_clean(recs)
