"""Guarded device outputs for the in-process GPU tests: a payload inside a 0xA5 allocation whose bands either side must stand
after the launch under test (the pattern of tests/test_gpu_guard.py, whose own Guarded works on a raw HIP handle), and the PCM
range form run into such buffers."""
import numpy as np

from conftest import DevBuf

GUARD = 64 * 1024  # bytes of 0xA5 either side of what a launch may write


class Guarded:
    """`nbytes` of device memory `shift` bytes into a 0xA5 allocation with GUARD bytes either side: .ptr, .fetch() -> the
    payload's bytes, .take(dtype) -> the payload, both after checking that nothing around it was written; .untouched(): nothing
    was written at all.  The device is synchronised behind the fill: it is a hipMemset on the null stream, the launch under test
    goes to a context's non-blocking stream, which nothing orders behind it, and the fill could land on top of the outputs (seen
    on the MI355X: 267 of 300 fills did)."""

    def __init__(self, nbytes, shift=0):
        self.nbytes, self.shift = int(nbytes), int(shift)
        self.buf = DevBuf(2 * GUARD + self.shift + self.nbytes, fill=0xA5)
        assert self.buf.hip.hipDeviceSynchronize() == 0
        self.ptr = self.buf.ptr + GUARD + self.shift

    def fetch(self):
        raw = self.buf.read(np.uint8)
        lo, hi = GUARD + self.shift, GUARD + self.shift + self.nbytes
        assert np.all(raw[:lo] == 0xA5), f"bytes written BEFORE the output (first at {int(np.argmax(raw[:lo] != 0xA5)) - lo})"
        assert np.all(raw[hi:] == 0xA5), f"bytes written BEHIND the output (first at +{int(np.argmax(raw[hi:] != 0xA5))})"
        return raw[lo:hi].copy()

    def take(self, dtype):
        return self.fetch().view(dtype)

    def untouched(self):
        return bool(np.all(self.buf.read(np.uint8) == 0xA5))

    def free(self):
        self.buf.free()


def pcm_dev_range(call, count, shift=0, shift16=0, f32=True, i16=False):
    """A PCM range form into guarded buffers -> (f32 | None, int16 | None); the guards must stand.  call(d_f32 | None, d_i16 |
    None) queues the device form for `count` outputs and waits for it."""
    gf = Guarded(count * 4, shift) if f32 else None
    gi = Guarded(count * 2, shift16) if i16 else None
    try:
        call(gf.ptr if gf else None, gi.ptr if gi else None)
        return gf.take(np.float32) if gf else None, gi.take(np.int16) if gi else None
    finally:
        for g in (gf, gi):
            if g:
                g.free()
