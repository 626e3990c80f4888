"""The row-side pitch pick against the transform-side pick on the CPU (tests/emu/rowpick_emu.cpp): the rows of the sliding
N = 4096 emulation, then both picks lane by lane through the kernel's own helpers (stft_core.h: out_bin, band_mask,
row_pick_key).  The records agree bit for bit on every band the host hands to the row-side pick, and each is the lowest index
of the row's maximum over the band, compared on the bits."""
import ctypes as C

import numpy as np
import pytest

import emu_build
from conftest import accum_sweep

N = 4096
FRAMES = 37
BANDS = [(5, 150), (0, 0), (0, 255), (255, 255), (3, 4), (4, 7), (127, 129), (128, 128), (252, 255)]
NOT_ROW_SIDE = [(0, 256), (250, 300), (1024, 1024), (2047, 2047)]
REC = np.dtype([("bin", np.int32), ("mag", np.float32)])


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emu_build.shared_object("rowpick_emu", ["rowpick_emu.cpp"],
                                       ["stft_emu.cpp", "stft_core.h", "pk_math.h", "stft_tables.h", "stft_consts.inc"]))
    fp = C.POINTER(C.c_float)
    L.emu_stft_slide.argtypes = [C.c_int, C.c_int, C.c_int, fp, C.c_long, C.c_long, C.c_long, fp]
    L.emu_rowpick.argtypes = [fp, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def takes(hop):
    n = FRAMES * hop
    sweep = accum_sweep(n)
    bad = sweep.copy()
    bad[700] = np.nan
    bad[25 * hop + 17] = np.inf
    bad[18 * 256 - 20:18 * 256 + 280] = 0.0
    return {"sweep": sweep, "silence": np.zeros(n, np.float32), "dc": np.full(n, 0.25, np.float32), "bad": bad}


@pytest.mark.parametrize("hop", [256, 512])
def test_row_side_records_equal_transform_side_records(lib, hop):
    fp = C.POINTER(C.c_float)
    for name, w in takes(hop).items():
        rows = np.empty((FRAMES, N // 2), np.float32)
        assert lib.emu_stft_slide(N, 16, hop, w.ctypes.data_as(fp), len(w), 0, FRAMES, rows.ctypes.data_as(fp)) == 0
        if name == "bad":
            assert np.isnan(rows).all(axis=1).any() and np.isfinite(rows).all(axis=1).any()
        b = rows.view(np.uint32)
        for kmin, kmax in BANDS:
            old, new = np.zeros(FRAMES, REC), np.zeros(FRAMES, REC)
            assert lib.emu_rowpick(rows.ctypes.data_as(fp), FRAMES, kmin, kmax, old.ctypes.data, new.ctypes.data) == 0
            assert old.tobytes() == new.tobytes(), (name, hop, kmin, kmax)
            want = kmin + np.argmax(b[:, kmin:kmax + 1], axis=1)
            assert np.array_equal(new["bin"], want), (name, hop, kmin, kmax)
            assert np.array_equal(new["mag"].view(np.uint32), b[np.arange(FRAMES), want]), (name, hop, kmin, kmax)
            if name == "silence":
                assert (new["bin"] == kmin).all() and not new["mag"].any()
        for kmin, kmax in NOT_ROW_SIDE:
            assert lib.emu_rowpick(rows.ctypes.data_as(fp), FRAMES, kmin, kmax, None, None) == -1
