"""The N = 4096 STFT kernel's per-workgroup invariants on the CPU (tests/emu/hoist_emu.cpp), through the helpers the kernel
instantiates:

  * the row-side pick with its in-band tests taken once — row_band_mask and the mask / flag forms of row_pick_key — gives the key
    of the form that tests kmin and kmax per bin, on every 4-bin group of wave 0 for every band 0 <= kmin, kmax <= 255 (empty
    bands included), on magnitudes with ties, zeros, NaN payloads of either sign, infinities and denormals;
  * pass 3 with thread 0's first KH selected twiddles made once gives the bits of pass 3 with every select per call, for
    KH = 0 .. 7, for thread 0 (where the selects decide) and other threads (where they must change nothing)."""
import ctypes as C

import numpy as np
import pytest

import emu_build


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_build.shared_object("hoist_emu", ["hoist_emu.cpp"],
                                       ["stft_core.h", "pk_math.h", "stft_consts.inc"]))
    fp = C.POINTER(C.c_float)
    L.emu_hoist_pick_mismatches.restype = C.c_long
    L.emu_hoist_pick_mismatches.argtypes = [C.POINTER(C.c_long)]
    L.emu_hoist_pass3.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp]
    return L


def test_masked_row_pick_key_is_the_band_form_on_every_band_and_lane(emu):
    n = C.c_long()
    assert emu.emu_hoist_pick_mismatches(C.byref(n)) == 0
    assert n.value == 256 * 256 * 64 * 16


@pytest.mark.parametrize("t", [0, 1, 64, 127])
def test_hoisted_twiddle_selects_leave_pass3_bit_for_bit(emu, t):
    rng = np.random.default_rng(4096 + t)
    fp = C.POINTER(C.c_float)
    for kh in range(8):
        v = rng.standard_normal(32).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, 7)
        w = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32).ravel()
        ref, new = np.empty(32, np.float32), np.empty(32, np.float32)
        assert emu.emu_hoist_pass3(kh, t, v.ctypes.data_as(fp), w.ctypes.data_as(fp), ref.ctypes.data_as(fp),
                                   new.ctypes.data_as(fp)) == 0
        assert np.array_equal(ref.view(np.uint32), new.view(np.uint32)), (t, kh)
        assert not np.array_equal(ref, v)
