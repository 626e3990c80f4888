"""The N = 4096 STFT kernels' per-workgroup invariants: the row-side pick's in-band tests are taken once per workgroup (one
lane mask per bin of a lane's four), thread 0's selected pass-3 twiddles are made once where the instantiation has the
registers, the row leaves through stores off one scalar base, and the magnitude scatter pairs its LDS writes.  None of it may
change a bit, so everything here is checked against the build's own other paths, not against recorded values:

  * the pitch records of a rows + pitch call equal the pitch-only call's (which keeps the transform-side pick),
  * its rows at the run heads equal those of the same frames with one frame per workgroup (every frame a run head: no
    hoisted state carried from frame to frame) — with direct loads that holds for every frame; a slid frame is the previous
    one aged and topped up, another rounding of the same frame, and lies within twice the suite's parity bound (conftest
    mag_tol: each of the two is within it of the exact row),
  * each record is the lowest bin of the maximum of the call's own row over the band, compared on the bits as the key is,
  * the words after the last row and the last record stay as they were.

Kernels: the two slides (hop 256, 512), direct loads unaligned (375) and aligned (3000).  Frame counts 1, 2, 33 and 65 with
32-frame runs: a lone head frame, a head and one slide, a run boundary with a one-frame remainder after one and after two whole
runs.  Bands: all of wave 0's bins, its first bin alone, its last bin alone, and a band whose ends are bins 4t + 1 and 4t + 2
of one lane (so that lane's four in-band tests differ).  An empty band does not reach a kernel: the call is refused."""
import numpy as np
import pytest

from conftest import DevBuf, accum_sweep, mag_tol

pytestmark = pytest.mark.gpu

N = 4096
RUN = 32
HOPS = [256, 512, 375, 3000]
SLIDES = (256, 512)
COUNTS = [1, 2, 33, 65]
BANDS = [(0, 255), (0, 0), (255, 255), (4 * 10 + 1, 4 * 10 + 2)]
GUARD = 1024  # bytes watched after each output
FILL = 0xA5


def takes(hop, count):
    n = count * hop
    sweep = accum_sweep(n)
    nan = sweep.copy()
    nan[n // 2] = np.nan
    return {"sweep": sweep, "silence": np.zeros(n, np.float32), "nan": nan}


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


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("hop", HOPS)
def test_records_and_rows_are_the_other_paths_bits(gpu_ctx, hop, count):
    try:
        for name, w in takes(hop, count).items():
            a = gpu_ctx.upload(w)
            gpu_ctx.set_frames_per_block(1)
            heads, _ = gpu_ctx.stft_hop(a, N, hop, want_pitch=False)
            assert heads.shape == (count, N // 2)
            if name == "nan":
                assert np.isnan(heads).all(axis=1).any()
            gpu_ctx.set_frames_per_block(RUN)
            for band in BANDS:
                what = (name, hop, count, band)
                rows, both = gpu_ctx.stft_hop(a, N, hop, band=band)
                _, alone = gpu_ctx.stft_hop(a, N, hop, band=band, want_mags=False)
                assert same_records(both, alone), what
                exact = slice(None, None, RUN if hop in SLIDES else 1)
                assert np.array_equal(bits(rows[exact]), bits(heads[exact])), what
                if name == "sweep":
                    assert (np.abs(rows - heads) <= 2 * mag_tol(heads)).all(), what
                check_against_rows(both, rows, band, what)
                if name == "silence":  # every key ties: the lowest bin of the band
                    assert (both["bin"] == band[0]).all() and not bits(both["mag"]).any(), what
            a.free()
    finally:
        gpu_ctx.set_frames_per_block(0)


@pytest.mark.parametrize("hop", HOPS)
def test_words_after_the_last_row_and_record_are_untouched(gpu_ctx, mxlib, hop):
    rec = np.dtype(mxlib.PITCH_DTYPE).itemsize
    try:
        gpu_ctx.set_frames_per_block(RUN)
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


def test_an_empty_band_is_refused(gpu_ctx, mxlib):
    """kmin > kmax after clamping never reaches a kernel (check_common): the status says so."""
    a = gpu_ctx.upload(accum_sweep(2 * 256))
    try:
        for band in [(7, 6), (255, 0), (3000, 4000)]:
            with pytest.raises(mxlib.MxError) as e:
                gpu_ctx.stft_hop(a, N, 256, band=band)
            assert e.value.code == mxlib._capi.MX_ERR_INVALID, band
    finally:
        a.free()
