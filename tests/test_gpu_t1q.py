"""The q-major T1 image and the one-reduction row-side pick of the N = 4096 STFT kernels.  A bulk call that wants rows and
records with the whole band below bin 256 takes both; a call whose band reaches bin 256 keeps the XOR image and the transform-side
pick — the same frame walk, the same slide arithmetic, the same run heads.  Neither change may move a bit, so the control is the
build's own other path:

  * rows of the in-band call are byte-equal to the rows of the call whose band reaches bin 256,
  * its records are byte-equal to the pitch-only call's of the same band (transform-side pick), and each is the lowest bin of
    the maximum of the call's own row over the band, compared on the bits as the key is,
  * with one frame per workgroup its rows are byte-equal to ranges mode's (every frame loaded directly: the frame-indexing check),
  * the words after the last row and the last record stay as they were.

Hops 256 and 512 (the two slides); frame counts 1, 2, 33 and 65: with 32-frame runs a lone head frame, a head and one slide, a
run head crossed at frame 32 with a last run of one frame, after one and after two whole runs; runs of 1 and 32 frames.  Takes: a
short sweep with seeded noise, and the same with a NaN in the middle (the frames that hold it are NaN in every bin: every key of
the band ties at the NaN's bits)."""
import numpy as np
import pytest

from conftest import DevBuf, accum_sweep, noisy

pytestmark = pytest.mark.gpu

N = 4096
HOPS = [256, 512]
COUNTS = [1, 2, 33, 65]
RUNS = [1, 32]
BANDS = [(5, 150), (0, 255), (4 * 10 + 1, 4 * 10 + 2)]  # the default band, all of wave 0's bins, two bins inside one lane
CONTROL = {(5, 150): (5, 256), (0, 255): (0, 256), (4 * 10 + 1, 4 * 10 + 2): (4 * 10 + 1, 300)}  # bands that reach bin 256
GUARD = 1024  # bytes watched after each output
FILL = 0xA5


def takes(hop, count):
    n = count * hop
    clean = noisy(accum_sweep(n), seed=4096 + hop + count)
    nan = clean.copy()
    nan[n // 2] = np.nan
    return {"sweep": clean, "nan": nan}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_records(p, q):
    return np.array_equal(p["bin"], q["bin"]) and np.array_equal(bits(p["mag"]), bits(q["mag"]))


def check_against_rows(pitch, rows, band, what):
    kmin, kmax = band
    b = bits(rows)[:, kmin:kmax + 1]
    want = kmin + np.argmax(b, axis=1)  # the first of equal maxima: the lowest bin
    assert np.array_equal(pitch["bin"], want), what
    assert np.array_equal(bits(pitch["mag"]), bits(rows)[np.arange(len(rows)), want]), what


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("hop", HOPS)
def test_rows_and_records_are_the_xor_image_and_transform_side_bits(gpu_ctx, hop, count, run):
    h = np.arange(count)
    rr = np.stack([h * hop, (h + 1) * hop], axis=1).astype(np.int32)
    try:
        gpu_ctx.set_frames_per_block(run)
        for name, w in takes(hop, count).items():
            a = gpu_ctx.upload(w)
            for band in BANDS:
                what = (name, hop, count, run, band)
                rows, both = gpu_ctx.stft_hop(a, N, hop, band=band)
                control, _ = gpu_ctx.stft_hop(a, N, hop, band=CONTROL[band])
                assert rows.shape == (count, N // 2)
                assert np.array_equal(bits(rows), bits(control)), what
                _, alone = gpu_ctx.stft_hop(a, N, hop, band=band, want_mags=False)
                assert same_records(both, alone), what
                check_against_rows(both, rows, band, what)
                if name == "nan":
                    assert np.isnan(rows).all(axis=1).any(), what
                    if count > 2 * N // hop:
                        assert np.isfinite(rows).all(axis=1).any(), what
                if run == 1:
                    ranged, rec = gpu_ctx.stft_ranges(a, N, rr, band=band)
                    assert np.array_equal(bits(rows), bits(ranged)), what
                    assert same_records(both, rec), what
            a.free()
    finally:
        gpu_ctx.set_frames_per_block(0)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("hop", HOPS)
def test_words_after_the_last_row_and_record_are_untouched(gpu_ctx, mxlib, hop, run):
    rec = np.dtype(mxlib.PITCH_DTYPE).itemsize
    try:
        gpu_ctx.set_frames_per_block(run)
        for count in COUNTS:
            a = gpu_ctx.upload(takes(hop, count)["sweep"])
            rows, both = gpu_ctx.stft_hop(a, N, hop, band=BANDS[0])
            d_m, d_p = DevBuf(count * (N // 2) * 4 + GUARD, FILL), DevBuf(count * rec + GUARD, FILL)
            assert d_m.hip.hipDeviceSynchronize() == 0  # the fill runs on the null stream, the kernel on the context's own
            gpu_ctx.stft_hop_dev(a, N, hop, 0, count, d_m.ptr, d_p.ptr, band=BANDS[0])
            gpu_ctx.synchronize()
            m, p = d_m.read(np.uint8), d_p.read(np.uint8)
            assert np.array_equal(m[:-GUARD].view(np.uint32), bits(rows).ravel()), (hop, count)
            assert np.array_equal(p[:-GUARD], np.ascontiguousarray(both).view(np.uint8)), (hop, count)
            assert (m[-GUARD:] == FILL).all() and (p[-GUARD:] == FILL).all(), (hop, count)
            d_m.free()
            d_p.free()
            a.free()
    finally:
        gpu_ctx.set_frames_per_block(0)
