"""The row-side pitch pick of the N = 4096 STFT kernels: a bulk call that wants rows and pitch records with the whole band
below bin 256 picks the record where the finished row is flushed (wave 0, four consecutive bins to a lane); every other call
keeps the transform-side pick.  Both must give the same bits: the records of a rows + pitch call equal those of the pitch-only
call of the same build (which stays on the transform side), each record is the lowest index of the maximum of the call's own
row over the band — compared on the bits, as the key is — and the rows are those of a call without a pitch pointer.

101 frames: with 32-frame runs three whole runs and one of 5 frames, so the pick of a run's first frame, of the frames inside
the loop and of the flush after the loop are all there; run lengths 1 (every record leaves in the final flush), 8, 32 and the
context's default for the call (which is 1 for so short a call)."""
import numpy as np
import pytest

from conftest import accum_sweep

pytestmark = pytest.mark.gpu

N = 4096
FRAMES = 101
ROW_SIDE = [(-1, -1), (0, 0), (0, 255), (255, 255), (3, 4), (4, 7), (127, 129), (128, 128), (252, 255)]  # (-1, -1): the default, (5, 150)
FALL_BACK = [(0, 256), (250, 300), (1024, 1024), (2047, 2047)]


def takes(hop):
    n = FRAMES * hop
    sweep = accum_sweep(n)
    bad = sweep.copy()
    bad[3000] = np.nan
    bad[78 * hop + 17] = np.inf
    z0 = 40 * 256 - 20
    bad[z0:z0 + 300] = 0.0  # holds samples [40 * 256, 41 * 256): at hop 256 the whole newest hop of frame 40
    return {"sweep": sweep, "silence": np.zeros(n, np.float32), "dc": np.full(n, 0.25, np.float32), "bad": bad}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_records(p, q):
    return np.array_equal(p["bin"], q["bin"]) and np.array_equal(bits(p["mag"]), bits(q["mag"]))


def check_against_rows(pitch, rows, band, what):
    kmin, kmax = band
    kmax = min(kmax, N // 2 - 1)
    b = bits(rows)[:, kmin:kmax + 1]
    want = kmin + np.argmax(b, axis=1)  # the first of equal maxima: the lowest bin
    assert np.array_equal(pitch["bin"], want), what
    assert np.array_equal(bits(pitch["mag"]), bits(rows)[np.arange(len(rows)), want]), what


@pytest.mark.parametrize("run", [0, 1, 8, 32])
@pytest.mark.parametrize("hop", [256, 512, 375, 3000])  # the two sliding kernels, direct loads unaligned and aligned
def test_row_side_records_are_the_transform_side_records(gpu_ctx, mxlib, hop, run):
    default = mxlib.pitch_band(N, 48000)
    assert default == (5, 150)
    try:
        gpu_ctx.set_frames_per_block(run)
        for name, w in takes(hop).items():
            a = gpu_ctx.upload(w)
            rows_only, none = gpu_ctx.stft_hop(a, N, hop, want_pitch=False)
            assert none is None and rows_only.shape == (FRAMES, N // 2)
            if name == "bad":
                assert np.isnan(rows_only).all(axis=1).any() and np.isfinite(rows_only).all(axis=1).any()
            for band in ROW_SIDE + FALL_BACK:
                what = (name, hop, run, band)
                rows, both = gpu_ctx.stft_hop(a, N, hop, band=band)
                _, alone = gpu_ctx.stft_hop(a, N, hop, band=band, want_mags=False)
                assert same_records(both, alone), what
                assert np.array_equal(bits(rows), bits(rows_only)), what
                check_against_rows(both, rows, default if band == (-1, -1) else band, what)
                if name == "silence":
                    assert (both["bin"] == (default if band == (-1, -1) else band)[0]).all() and not both["mag"].any(), what
            a.free()
    finally:
        gpu_ctx.set_frames_per_block(0)


def test_ranges_mode_agrees_with_one_frame_runs(gpu_ctx):
    """The same frames as ranges (ranges mode keeps the transform-side pick): rows and records equal the bulk call's with one
    frame per workgroup, bit for bit, on the row-side and on the fall-back bands."""
    hop = 256
    w = takes(hop)["bad"]
    a = gpu_ctx.upload(w)
    h = np.arange(FRAMES)
    rr = np.stack([h * hop, (h + 1) * hop], axis=1).astype(np.int32)
    try:
        gpu_ctx.set_frames_per_block(1)
        for band in [(-1, -1), (0, 255), (252, 255), (250, 300)]:
            m1, p1 = gpu_ctx.stft_hop(a, N, hop, band=band)
            m2, p2 = gpu_ctx.stft_ranges(a, N, rr, band=band)
            assert np.array_equal(bits(m1), bits(m2)), band
            assert same_records(p1, p2), band
    finally:
        gpu_ctx.set_frames_per_block(0)
        a.free()
