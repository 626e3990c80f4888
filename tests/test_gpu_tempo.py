"""mx_tempo_smooth / mx_tempo_comb / mx_tempo_from_flux / mx_tempo_detect on the GPU against tests/tempo_ref.py (include/
melonix_amd.h "Tempo and grid-offset estimation").  Every comparison is for equal bytes: the definition leaves the device
nothing to approximate.  Plus what a bad call may touch, and the chain the estimate closes: detect tempo -> timing markers ->
render -> the onsets on the true grid."""
import ctypes as C

import numpy as np
import pytest

import tempo_ref as T
from conftest import DevBuf
from tempo_ref import same_estimate

pytestmark = pytest.mark.gpu

SR, HOP = T.SR, T.HOP
GUARD = 256  # bytes of 0xA5 either side of a device output


def _guarded(nbytes):
    return DevBuf(nbytes + 2 * GUARD, fill=0xA5)


def _inside(buf, nbytes, dtype):
    raw = buf.read(np.uint8)
    assert np.all(raw[:GUARD] == 0xA5) and np.all(raw[GUARD + nbytes:] == 0xA5), "a store outside the output"
    return raw[GUARD:GUARD + nbytes].view(dtype)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 767, 769])
def test_smoothing_equals_the_reference(gpu_ctx, count):
    rng = np.random.default_rng(count)
    o = rng.gamma(0.6, 4.0, count).astype(np.float32)
    if count >= 63:
        o[[0, 17, count - 1]] = [np.nan, np.inf, -np.inf]
    src, dst = DevBuf(count * 4), _guarded(count * 4)
    try:
        src.write(o)
        for W in (0, 1, 4, 32):
            want = T.smooth(o, W)
            assert np.isfinite(want).all()
            assert gpu_ctx.tempo_smooth(o, W).tobytes() == want.tobytes(), W  # the host form
            gpu_ctx.tempo_smooth_dev(src.ptr, count, W, dst.ptr + GUARD)
            gpu_ctx.synchronize()
            assert _inside(dst, count * 4, np.float32).tobytes() == want.tobytes(), W  # the device form, and only there
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("kind", T.COMB_CURVES)
def test_comb_equals_the_reference(gpu_ctx, mxlib, kind):
    for count in T.COMB_COUNTS:
        e, jobs, want = T.comb_case(kind, count)
        want = T.records_array(want, mxlib.COMB_DTYPE)
        got = gpu_ctx.tempo_comb(e, jobs)
        assert got.tobytes() == want.tobytes(), (kind, count, np.flatnonzero(got != want)[:5])
        # the device form over the same jobs in HBM, guard bands around the records
        j = np.array(jobs, dtype=mxlib.COMB_JOB_DTYPE)
        dc, dj, do = DevBuf(count * 4), DevBuf(j.nbytes), _guarded(want.nbytes)
        try:
            dc.write(e)
            dj.write(j)
            gpu_ctx.tempo_comb_dev(dc.ptr, count, dj.ptr, len(j), do.ptr + GUARD)
            gpu_ctx.synchronize()
            assert _inside(do, want.nbytes, np.uint8).tobytes() == want.tobytes(), (kind, count)
        finally:
            dc.free()
            dj.free()
            do.free()


@pytest.mark.parametrize("njobs", [1, 255, 257, 5000])
def test_comb_job_lists(gpu_ctx, mxlib, njobs):
    """A record depends on its job alone: lists of every length, the same job twice, a permuted list, overlapping segments."""
    count = 2049
    e, _, _ = T.comb_case("noise", count)
    rng = np.random.default_rng(njobs)
    pool = [(f, n, q) for q in T.COMB_PERIODS[:5] for f, n in ((0, count), (100, 700), (400, 900), (1500, 549), (2048, 1))]
    pool_ref = T.records_array(T.comb(e, pool), mxlib.COMB_DTYPE)
    pick = rng.integers(0, len(pool), njobs)
    if njobs > 1:
        pick[-1] = pick[0]  # the same job twice
    got = gpu_ctx.tempo_comb(e, [pool[i] for i in pick])
    assert got.tobytes() == pool_ref[pick].tobytes()
    perm = rng.permutation(njobs)
    assert gpu_ctx.tempo_comb(e, [pool[i] for i in pick[perm]]).tobytes() == got[perm].tobytes()


def test_comb_refuses_bad_jobs_before_any_launch(gpu_ctx, mxlib):
    from melonix_amd import _capi

    lib, ctx = _capi.lib(), gpu_ctx.handle
    e = np.ones(100, np.float32)
    good = (0, 100, 45 << 16)
    for bad in ((0, 0, 45 << 16), (-1, 10, 45 << 16), (0, 101, 45 << 16), (100, 1, 45 << 16), (50, 51, 45 << 16),
                (0, 100, (2 << 16) - 1), (0, 100, (4096 << 16) + 1)):
        for jobs in ([bad], [good, good, bad]):
            j = np.array(jobs, dtype=mxlib.COMB_JOB_DTYPE)
            out = np.full(len(j) * 16, 0xA5, dtype=np.uint8)
            assert lib.mx_tempo_comb(ctx, e.ctypes.data, len(e), j.ctypes.data, len(j), out.ctypes.data) == _capi.MX_ERR_INVALID, bad
            assert np.all(out == 0xA5), bad
    j = np.array([good], dtype=mxlib.COMB_JOB_DTYPE)
    out = np.full(16, 0xA5, dtype=np.uint8)
    for args in ((None, 100, j.ctypes.data, 1, out.ctypes.data), (e.ctypes.data, 100, None, 1, out.ctypes.data),
                 (e.ctypes.data, 100, j.ctypes.data, 1, None), (e.ctypes.data, 0, j.ctypes.data, 1, out.ctypes.data),
                 (e.ctypes.data, -1, j.ctypes.data, 1, out.ctypes.data), (e.ctypes.data, 100, j.ctypes.data, -1, out.ctypes.data)):
        assert lib.mx_tempo_comb(ctx, *args) == _capi.MX_ERR_INVALID, args
        assert lib.mx_tempo_comb_dev(ctx, *args) == _capi.MX_ERR_INVALID, args
    assert np.all(out == 0xA5)
    assert len(gpu_ctx.tempo_comb(e, np.zeros(0, dtype=mxlib.COMB_JOB_DTYPE))) == 0  # no jobs: nothing to do


def test_smoother_refusals_and_empty_inputs(gpu_ctx, mxlib):
    """A width out of range, null pointers, a negative count, an output on top of its input: refused before any launch."""
    from melonix_amd import _capi

    lib, ctx = _capi.lib(), gpu_ctx.handle
    buf = DevBuf(1024, fill=0xA5)
    try:
        for args in ((buf.ptr, 64, -1, buf.ptr + 512), (buf.ptr, 64, 33, buf.ptr + 512), (None, 64, 4, buf.ptr + 512),
                     (buf.ptr, 64, 4, None), (buf.ptr, -1, 4, buf.ptr + 512), (buf.ptr, 64, 4, buf.ptr),
                     (buf.ptr, 64, 4, buf.ptr + 252), (buf.ptr + 252, 64, 4, buf.ptr)):
            assert lib.mx_tempo_smooth_dev(ctx, *args) == _capi.MX_ERR_INVALID, args
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5)
        gpu_ctx.tempo_smooth_dev(buf.ptr, 64, 4, buf.ptr + 256)  # adjacent is not overlapping
        gpu_ctx.tempo_smooth_dev(0, 0, 4, 0)                     # no frames: nothing to do
        gpu_ctx.synchronize()
    finally:
        buf.free()
    host = np.ones(64, np.float32)
    assert lib.mx_tempo_smooth(ctx, host.ctypes.data, 64, 4, host.ctypes.data) == _capi.MX_ERR_INVALID
    assert lib.mx_tempo_smooth(ctx, host.ctypes.data, 32, 4, host.ctypes.data + 4 * 31) == _capi.MX_ERR_INVALID
    assert np.all(host == 1.0)
    assert len(gpu_ctx.tempo_smooth(np.zeros(0, np.float32))) == 0


@pytest.mark.parametrize("name", list(T.TAKES))
def test_estimates_equal_the_reference_on_the_takes(gpu_ctx, name):
    """mx_tempo_from_flux over the definition's flux, and mx_tempo_detect — whose flux is the GPU's own, so the reference is
    run over those bytes — field for field."""
    res, windows, _ = T.take_estimate(name)
    same_estimate(gpu_ctx.tempo_from_flux(T.take_flux(name), SR, HOP, want_windows=True), (res, windows))
    a = gpu_ctx.upload(T.take_wave(name))
    try:
        flux = gpu_ctx.onset_flux(a, SR, HOP)
        got = gpu_ctx.tempo_detect(a, SR, HOP, want_windows=True)
        assert gpu_ctx.tempo_detect(a, SR, HOP) == got[0]  # (windows NULL: the same estimate)
    finally:
        a.free()
    same_estimate(got, T.estimate(flux, SR, HOP))
    off, rel, length = T.grid_error(name, got[0])
    assert off + length * rel < 60.0 / (T.TAKES[name]["bpm"] * 4) / 4  # and the GPU's estimate is on the true grid too


def test_many_windows_a_first_frame_and_an_empty_take(gpu_ctx, mxlib):
    flux = T.take_flux("bpm100_jitter")
    kw = dict(window_frames=512, stride_frames=128)
    want = T.estimate(flux, SR, HOP, **kw)
    assert len(want[1]) > 10
    same_estimate(gpu_ctx.tempo_from_flux(flux, SR, HOP, want_windows=True, **kw), want)
    base = gpu_ctx.tempo_from_flux(flux, SR, HOP)
    moved = gpu_ctx.tempo_from_flux(flux, SR, HOP, first_frame=1000, want_windows=True)
    same_estimate(moved, T.estimate(flux, SR, HOP, first_frame=1000))
    g = 60.0 / base["bpm"]
    d = (moved[0]["offset"] - base["offset"] - 1000 * HOP / SR) % g
    assert moved[0]["bpm"] == base["bpm"] and min(d, g - d) < 1e-9
    empty = dict(bpm=0.0, offset=0.0, score=0.0, clarity=0.0, locked_frames=0, levels=0)
    for f in (np.zeros(0, np.float32), np.zeros(5000, np.float32)):
        res, win = gpu_ctx.tempo_from_flux(f, SR, HOP, want_windows=True)
        assert res == empty and len(win) == 0
    a = gpu_ctx.upload(np.zeros(2 * SR, np.float32))
    try:
        res, win = gpu_ctx.tempo_detect(a, SR, HOP, want_windows=True)
        assert res == empty and len(win) == 0
        # refusals: outputs untouched, MX_ERR_INVALID
        from melonix_amd import _capi
        lib = _capi.lib()
        for bad in (dict(bpm_min=29.0), dict(bpm_max=251.0), dict(per_octave=7), dict(smooth=33), dict(window_frames=63),
                    dict(stride_frames=0), dict(prior_bpm=0.0), dict(prior_octaves=float("nan")), dict(lock_ratio=1.5)):
            with pytest.raises(mxlib.MxError) as err:
                gpu_ctx.tempo_from_flux(flux, SR, HOP, **bad)
            assert err.value.code == -1, bad
            with pytest.raises(mxlib.MxError):
                gpu_ctx.tempo_detect(a, SR, HOP, **bad)
        for sr, hop in ((0, HOP), (SR, 0), (SR, 16385), (SR, 16), (SR, 12000)):  # (the last two: a period outside the Q16 range)
            t = _capi.Tempo(bpm=-7.0)
            assert lib.mx_tempo_from_flux(gpu_ctx.handle, flux.ctypes.data, len(flux), sr, hop, 0, None, C.byref(t), None, None) == -1
            assert lib.mx_tempo_detect(gpu_ctx.handle, a.handle, sr, hop, None, None, C.byref(t), None, None) == -1
            assert t.bpm == -7.0
        t = _capi.Tempo()
        assert lib.mx_tempo_from_flux(gpu_ctx.handle, flux.ctypes.data, len(flux), SR, HOP, -1, None, C.byref(t), None, None) == -1
        assert lib.mx_tempo_from_flux(gpu_ctx.handle, None, 10, SR, HOP, 0, None, C.byref(t), None, None) == -1
        assert lib.mx_tempo_from_flux(gpu_ctx.handle, flux.ctypes.data, len(flux), SR, HOP, 0, None, None, None, None) == -1
        win = C.c_void_p()
        assert lib.mx_tempo_from_flux(gpu_ctx.handle, flux.ctypes.data, len(flux), SR, HOP, 0, None, C.byref(t), C.byref(win), None) == -1
    finally:
        a.free()
    gpu_ctx.release_scratch()  # the work memory goes; the next call takes it again
    assert gpu_ctx.tempo_from_flux(flux, SR, HOP) == base


def test_detected_tempo_puts_the_rendered_onsets_on_the_true_grid(gpu_ctx, mxlib):
    """The 100 bpm take (+-10 ms jitter): mx_tempo_detect -> mx_timing_params{its bpm and offset, division 4} -> mx_onsets_detect
    -> mx_timing_markers -> mx_psola_render with the GPU's own f0 track -> detect again: every onset of the render within +-4
    frames of a line of the TRUE grid (lead + first_beat + k * 60 / (100 * 4)), the bound of the
    onset detector's own end-to-end case (test_notes_rendered_through_their_timing_markers_land_on_the_grid, which lives in
    tests/test_gpu_onset_facade.py).  The definitions alone stay inside it first: tests/test_tempo_host.py runs the same chain through tempo_ref,
    onset_ref, yin_ref and psola_ref on the CPU (0.12 to 1.63 frames off the true grid; the GPU gave the same figures)."""
    name = "bpm100_jitter"
    w, args = T.take_wave(name), T.TAKES[name]
    a = gpu_ctx.upload(w)
    try:
        t = gpu_ctx.tempo_detect(a, SR, HOP)
        onsets = gpu_ctx.onsets_detect(a, SR, HOP)
        markers = mxlib.timing_markers(onsets["sample"], len(w), SR, bpm=t["bpm"], offset=t["offset"], division=4)
        mk = [(int(m["sample"]), float(m["note"]), float(m["dTime"]), float(m["pitchBend"])) for m in markers]
        track = gpu_ctx.f0_track(a, SR, HOP)
        f32, _ = gpu_ctx.psola_render(a, SR, HOP, track, mk, want_i16=False)
    finally:
        a.free()
    b = gpu_ctx.upload(f32)
    try:
        again = gpu_ctx.onsets_detect(b, SR, HOP)
    finally:
        b.free()
    g = 60.0 / (args["bpm"] * 4)
    line = args.get("lead", 0.0) + 0.25
    dist = [abs(((o["sample"] / SR - line + g / 2) % g) - g / 2) * SR / HOP for o in again]
    print(f"{t['bpm']:.4f} bpm, offset {t['offset']:.4f} s; {len(onsets)} onsets, {len(again)} after the render, "
          f"frames off the true grid: {np.round(dist, 2).tolist()}")
    assert len(again) == len(onsets) >= 15
    assert max(dist) <= 4
