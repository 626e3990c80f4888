"""Runs the gfx950 kernel's per-thread templates (melonix_amd/csrc/stft_core.h) thread by thread
on the CPU (tests/emu/stft_emu.cpp) and checks them against the oracle: index maps, LDS swizzle
closed forms (bijective, equal to t1_index), twiddles, the real-FFT split, the sliding window."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bad_samples as B
from conftest import SR, accum_sweep, mag_tol, noisy

HERE = os.path.dirname(os.path.abspath(__file__))


RANGES = [(48000, 48375), (0, 256), (-500, -100), (239744, 240000), (479900, 480300), (100000, 100001),
          (5000, 4000), (1000, 60000)]


@pytest.mark.parametrize("N,E", [(4096, 16), (16384, 32), (32768, 32)])
def test_single_frames(emu, oracle, N, E):
    w = noisy(accum_sweep(10 * SR))
    fp = C.POINTER(C.c_float)
    for (s, e) in RANGES:
        ref = oracle.spec_frame(w, N, s, e)
        for hop_mode in (0, 1):
            if hop_mode and e <= s:
                continue
            out = np.empty(N // 2, np.float32)
            rc = emu.emu_stft_frame(N, E, w.ctypes.data_as(fp), len(w), s, e, hop_mode, out.ctypes.data_as(fp))
            assert rc == 0, "LDS closed-form address differs from the swizzle, or is not a bijection"
            assert (np.abs(out - ref) <= mag_tol(ref[None])[0]).all()
            assert np.abs(out - ref).max() <= 1e-6 * max(ref.max(), 1e-30) + 1e-12  # in fact ~1e-7 of the peak


@pytest.mark.parametrize("N,E,hop,first,count", [(4096, 16, 256, 520, 43), (4096, 16, 256, 0, 40),
                                                  (16384, 32, 512, 0, 40), (16384, 32, 512, 250, 32),
                                                  (4096, 16, 512, 0, 24), (4096, 16, 512, 100, 20), (16384, 32, 1024, 3, 20),
                                                  (32768, 32, 1024, 0, 20), (32768, 32, 1024, 40, 18)])
def test_sliding_window(emu, oracle, N, E, hop, first, count):
    """The register image slid frame to frame stays within 1e-6 of the frame peak of the oracle
    (tolerance 2e-5): at most N/hop - 2 decays per point."""
    w = noisy(accum_sweep(3 * SR))
    fp = C.POINTER(C.c_float)
    out = np.empty((count, N // 2), np.float32)
    rc = emu.emu_stft_slide(N, E, hop, w.ctypes.data_as(fp), len(w), first, count, out.ctypes.data_as(fp))
    assert rc == 0
    ref = np.stack([oracle.spec_frame(w, N, (first + f) * hop, (first + f + 1) * hop) for f in range(count)])
    err = np.abs(out - ref)
    assert (err <= mag_tol(ref)).all()
    assert (err.max(axis=1) <= 1e-6 * ref.max(axis=1) + 1e-12).all()


BAD_PLANS = [("slide", 4096, 16, 256), ("circ", 4096, 16, 375), ("slide", 16384, 32, 512), ("circ", 32768, 32, 375)]
BAD_N = 24000


def bad_take():
    return noisy(accum_sweep(BAD_N))


def emu_rows(emu, kind, N, E, hop, w):
    """Every frame of the take as ONE run of the sliding (kind "slide") or the circular register image -> (rows, the functions'
    return value: the LDS-collision count, 0 for any input now that the emulation compares the stored points as bits)."""
    fp = C.POINTER(C.c_float)
    frames = B.frame_count(len(w), hop)
    out = np.empty((frames, N // 2), np.float32)
    fn = emu.emu_stft_slide if kind == "slide" else emu.emu_stft_circ
    w = np.ascontiguousarray(w, dtype=np.float32)
    return out, fn(N, E, hop, w.ctypes.data_as(fp), len(w), 0, frames, out.ctypes.data_as(fp))


@pytest.mark.parametrize("name", list(B.BAD))
@pytest.mark.parametrize("kind,N,E,hop", BAD_PLANS)
def test_a_bad_sample_stays_in_its_frames(emu, oracle, kind, N, E, hop, name):
    """A sample that is Inf or NaN: frame h = samples [(h+1)*hop - N, (h+1)*hop) has a row without a finite bin exactly when it
    holds the sample; every other row — the frames before the sample enters the register image and those after it has left,
    in the same run — keeps the clean take's bytes: the decay in registers does not smear it.  Where the oracle is asked for
    the same frames (N = 4096) its rows are finite exactly where the emulation's are."""
    w = bad_take()
    clean, rc = emu_rows(emu, kind, N, E, hop, w)
    assert rc == 0 and np.isfinite(clean).all()
    for pos, s in B.positions(BAD_N, hop, N - hop, hop).items():
        v = B.with_bad(w, s, B.BAD[name])
        rows, rc = emu_rows(emu, kind, N, E, hop, v)
        assert rc == 0, "the collision counter depends on the samples' values"
        hold = B.holding(BAD_N, hop, N - hop, hop, s)
        B.check_rows(rows, clean, hold, (kind, N, hop, name, pos))
        if N == 4096 and pos == "straddle":
            pick = np.unique(np.concatenate([np.nonzero(hold)[0][[0, -1]], np.nonzero(hold)[0][[0, -1]] + [-1, 1]]))
            ref = np.stack([oracle.spec_frame(v, N, int(h) * hop, (int(h) + 1) * hop) for h in pick])
            assert np.array_equal(np.isfinite(ref), np.isfinite(rows[pick])), (kind, name, pick)


@pytest.mark.parametrize("N,E,hop,first,count", [(4096, 16, 375, 0, 40), (4096, 16, 375, 360, 25), (4096, 16, 100, 3, 50),
                                                  (4096, 16, 384, 0, 24), (4096, 16, 257, 11, 24), (4096, 16, 1, 4000, 24),
                                                  (16384, 32, 375, 0, 50), (16384, 32, 512 - 1, 250, 20),
                                                  (32768, 32, 375, 0, 24), (32768, 32, 512, 270, 12), (32768, 32, 500, 5, 10)])
def test_circular_window(emu, oracle, N, E, hop, first, count):
    """Uniform hops that do not slide by whole slots: the circular register image (only the newest 2*hop samples
    fetched per frame, everything older aged by one multiply) stays within 1e-6 of the frame peak of the oracle —
    including frames that start before the file and end after it."""
    w = noisy(accum_sweep(3 * SR))
    fp = C.POINTER(C.c_float)
    out = np.empty((count, N // 2), np.float32)
    rc = emu.emu_stft_circ(N, E, hop, w.ctypes.data_as(fp), len(w), first, count, out.ctypes.data_as(fp))
    assert rc == 0
    ref = np.stack([oracle.spec_frame(w, N, (first + f) * hop, (first + f + 1) * hop) for f in range(count)])
    err = np.abs(out - ref)
    assert (err <= mag_tol(ref)).all()
    assert (err.max(axis=1) <= 1e-6 * ref.max(axis=1) + 1e-12).all()
