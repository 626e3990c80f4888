"""The longest take the header admits — N_MAX = 0x7fffffff - 2 * MX_AUDIO_PAD samples, a padded image of 2^31 - 1 elements and
8 GiB — as a device buffer of zeros with six short "islands" of signal, and the means to state what a kernel must give there
without a host array of that size.

An island is 262 144 samples of noisy(accum_sweep(...)) with a seed of its own.  Where they sit (element index in the padded image =
sample + MX_AUDIO_PAD, byte offset = 4 x that):

  START  samples [65 536, 327 680)                  what a wrapped address from B4G lands on
  B2G    astride padded element 2^29                byte offset 2 GiB: the signed 32-bit line
  B4G    astride padded element 2^30                byte offset 4 GiB: the unsigned 32-bit line
  B6G    astride padded element 3 * 2^29            exactly 4 GiB above B2G
  J31    astride sample floor(2^31 * 147 / 160)     the 44.1 -> 48 kHz converter's output index passes 2^31 here
  END    the last 262 144 samples                   ends on N_MAX (odd); the trailing pad ends on the last int32 index

A byte offset truncated to 32 bits therefore reads OTHER signal, never the same zeros: from B6G it lands in B2G, from B4G in the
leading pad and START, from END (its last samples and the trailing pad) in B4G.

window(island, unit) gives the same samples at low addresses: the host array of samples [q, island end + margin) with q a multiple
of `unit`, built from the island's generator.  Uploaded as a take of its own it is the CONTROL: zeros before the file and zeros
before the island are the same thing to every kernel, and for END the control ends where the far take ends, so the last frame,
ceil(n / hop) and the reads into the trailing pad are the same case.  (tests/test_far_take_layout.py checks this arithmetic on the
CPU; tests/test_gpu_far_take.py holds every span-form entry point to "far == control, byte for byte".)"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from conftest import DevBuf, accum_sweep, loaded_hip, noisy

PAD = 32768                      # MX_AUDIO_PAD
N_MAX = 0x7fffffff - 2 * PAD     # 2 147 418 111: the longest take mx_audio_upload / mx_audio_wrap_device admit
IMAGE = N_MAX + 2 * PAD          # elements of the padded image: 2^31 - 1
ISLAND = 262144                  # samples of an island: 32-frame runs at hop 1024 plus an N = 32768 window
MARGIN = 65536
GIB = 1 << 30
J31_SAMPLE = (2 ** 31 * 147) // 160  # the input sample output 2^31 of 44 100 -> 48 000 reads (i_j = floor(j * 147 / 160))

# island -> its first sample
STARTS = {"START": 65536,
          "B2G": 2 ** 29 - ISLAND // 2 - PAD,
          "B4G": 2 ** 30 - ISLAND // 2 - PAD,
          "B6G": 3 * 2 ** 29 - ISLAND // 2 - PAD,
          "J31": J31_SAMPLE - ISLAND // 2,
          "END": N_MAX - ISLAND}
SEEDS = {name: 0x66617200 + k for k, name in enumerate(STARTS)}
# (island, the 32-bit line it straddles in bytes of the padded image)
LINES = {"B2G": 2 * GIB, "B4G": 4 * GIB, "B6G": 6 * GIB}
# island -> where a byte offset of it, truncated to 32 bits, lands
ALIASES = {"B6G": "B2G", "B4G": "START", "END": "B4G"}
SPAN_ISLANDS = ("B2G", "B4G", "B6G", "END")  # what every span form is run on


def span(island):
    """-> (first sample, one past the last)"""
    return STARTS[island], STARTS[island] + ISLAND


def byte_span(island):
    """-> byte offsets [lo, hi) of the island in the padded image"""
    lo, hi = span(island)
    return 4 * (lo + PAD), 4 * (hi + PAD)


@functools.lru_cache(maxsize=None)
def samples(island):
    """The island's 262 144 samples (read-only; no two islands share bytes: a seed and a sweep range each)."""
    k = list(STARTS).index(island)
    w = noisy(accum_sweep(ISLAND, f0=110.0 + 7.0 * k, f1=1760.0 - 31.0 * k), seed=SEEDS[island], level=1e-3)
    w.setflags(write=False)
    return w


def window_span(island, unit, margin=MARGIN):
    """-> (q, end): q the largest multiple of `unit` at or below island start - margin (not below 0), end = min(island end +
    margin, N_MAX).  Python integers."""
    lo, hi = span(island)
    return max(lo - margin, 0) // unit * unit, min(hi + margin, N_MAX)


def window(island, unit, margin=MARGIN):
    """-> (q, w): w the host array equal to the far take's samples [q, end) of window_span — zeros around the island's samples,
    built from the generator, never downloaded."""
    q, end = window_span(island, unit, margin)
    w = np.zeros(end - q, dtype=np.float32)
    lo, hi = span(island)
    for other in STARTS:  # (no window reaches a neighbouring island: the layout test holds that)
        assert other == island or span(other)[1] <= q or span(other)[0] >= end, (island, other)
    w[lo - q:hi - q] = samples(island)
    return q, w


def mem_info(hip=None):
    """-> (free, total) bytes of the current device (hipMemGetInfo)"""
    hip = hip or loaded_hip()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value, total.value


class FarTake:
    """The far take on the device: one DevBuf of IMAGE * 4 bytes of zeros, the islands written into it, wrapped as an Audio of
    N_MAX samples (.audio).  Skips the calling test where hipMemGetInfo reports less than the 8 GiB free; a hipMalloc that
    fails after that check fails the test."""

    def __init__(self, ctx):
        self.ctx, self.hip = ctx, loaded_hip()
        self.held = 0      # bytes this object and its tests hold on the device right now (what they declared through need())
        self.peak = 0
        self.buf = self.audio = None
        self.need(IMAGE * 4, "the far take's image")
        self.buf = DevBuf(IMAGE * 4, fill=0)
        for name in STARTS:
            self.buf.write(samples(name), offset=byte_span(name)[0])
        assert self.hip.hipDeviceSynchronize() == 0
        self.audio = ctx.wrap_device(self.buf.ptr, N_MAX)

    def need(self, nbytes, what):
        """Declares `nbytes` more of device memory for `what`; skips where hipMemGetInfo reports less free.  Give them back with
        release()."""
        free, total = mem_info(self.hip)
        if free < nbytes:
            pytest.skip(f"{what} needs {nbytes / GIB:.2f} GiB more of device memory ({(self.held + nbytes) / GIB:.2f} GiB at the "
                        f"peak); hipMemGetInfo reports {free / GIB:.2f} GiB free of {total / GIB:.2f} GiB")
        self.held += nbytes
        self.peak = max(self.peak, self.held)

    def release(self, nbytes):
        self.held -= nbytes

    def free(self):
        if self.audio is not None:
            self.audio.free()  # (not owned: the handle only)
            self.audio = None
        if self.buf is not None:
            self.buf.free()
            self.buf = None


@pytest.fixture(scope="module")
def far(gpu_ctx):
    """The far take, held for the whole of the importing file and freed at its end."""
    t0 = time.perf_counter()
    ft = FarTake(gpu_ctx)
    made = time.perf_counter() - t0
    yield ft
    print(f"far take: made in {made:.2f} s; peak device memory declared by this file {ft.peak / GIB:.2f} GiB")
    ft.free()
