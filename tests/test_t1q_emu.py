"""The q-major T1 image and the one-reduction row-side pick of the N = 4096 STFT kernel on the CPU (tests/emu/t1q_emu.cpp), through
the helpers the kernel instantiates:

  * the layout: (j, q) -> 130 q + j is injective into the 2080-point image; the store form (one base, sixteen immediates) and the
    read form (one base, immediates 8 r) hit it for every thread; by the LDS's grouping rule every 32-lane ds_read_b64 group
    touches 32 different 8-byte slots mod 32 and every 16-lane ds_write_b64 group 16 different ones mod 16; the pass-2 twiddles
    are the table's, rows 14 and 15 from registers;
  * a whole frame through pass 1, the q-major image and pass 2 gives the XOR image's v[] bit for bit;
  * the one-reduction pick gives the record of max(row_pick_key) over the wavefront for every band 0 <= kmin <= kmax <= 255 and
    every lane, on magnitudes with ties inside a lane, across lanes and between in-band and out-of-band bins, zeros, NaN payloads
    of either sign, infinities and denormals."""
import ctypes as C

import numpy as np
import pytest

import emu_build


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_build.shared_object("t1q_emu", ["t1q_emu.cpp"], ["stft_core.h", "pk_math.h", "stft_consts.inc"]))
    fp = C.POINTER(C.c_float)
    for f in (L.emu_t1q_layout_violations, L.emu_t1q_pick_mismatches):
        f.restype = C.c_long
        f.argtypes = [C.POINTER(C.c_long)]
    L.emu_t1q_frame.restype = None
    L.emu_t1q_frame.argtypes = [fp, fp, fp]
    return L


def test_layout_is_injective_hit_by_both_forms_and_free_of_bank_conflicts(emu):
    n = C.c_long()
    assert emu.emu_t1q_layout_violations(C.byref(n)) == 0
    # the map, the stores, the reads, the twiddles, the read groups (4 x 16) and the write groups (8 x 16)
    assert n.value == 128 * 16 + 128 * 16 + 128 * 16 + 128 * 15 + 4 * 16 + 8 * 16


@pytest.mark.parametrize("kind", ["noise", "sweep", "nan", "huge"])
def test_a_frame_through_the_q_major_image_is_the_xor_image_bit_for_bit(emu, kind):
    rng = np.random.default_rng(130)
    frame = rng.standard_normal(4096).astype(np.float32)
    if kind == "sweep":
        frame = (0.5 * np.sin(np.cumsum(np.linspace(0.01, 0.4, 4096)))).astype(np.float32) / 8192
    elif kind == "nan":
        frame[2049] = np.nan
    elif kind == "huge":
        frame *= np.float32(1e37)  # overflows to infinities (and their differences to NaN) inside the butterflies
    fp = C.POINTER(C.c_float)
    a, b = np.empty(4096, np.float32), np.empty(4096, np.float32)
    emu.emu_t1q_frame(frame.ctypes.data_as(fp), a.ctypes.data_as(fp), b.ctypes.data_as(fp))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kind
    assert np.isnan(a).any() == (kind in ("nan", "huge")) and a.any()


def test_one_reduction_pick_is_the_maximum_key_on_every_band_and_lane(emu):
    n = C.c_long()
    assert emu.emu_t1q_pick_mismatches(C.byref(n)) == 0
    assert n.value > 256 * 257 // 2 * 64 * 3 * 2  # at least two patterns in every lane on every background, for every band
