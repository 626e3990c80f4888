"""The host side of the onset detector (include/melonix_amd.h "Onset detection and tempo-grid timing markers"): mx_onset_pick
and mx_timing_markers against tests/onset_ref.py field for field, the properties of the time warp the markers make, the
refusals — and the kernel's per-lane arithmetic (csrc/onset_core.h) run lane by lane on the CPU against the binary64
definition.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import bad_samples as B
import emu_build
import onset_ref as R

SR = R.SR


def _same_picks(mx, flux, hop=256, first=0, **params):
    got = mx.onset_pick(flux, hop, first, **params)
    want = R.pick(flux, hop, first, **params)
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (int(g["sample"]), int(g["frame"])) == (w[0], w[1])
        assert g["strength"].tobytes() == w[2].tobytes() and g["margin"].tobytes() == w[3].tobytes(), (g, w)
    return got


def test_pick_defaults_and_random_arrays(mxlib):
    assert mxlib.onset_pick_params_default() == R.PICK_DEFAULTS
    rng = np.random.default_rng(7)
    total = 0
    for count in (2, 3, 17, 64, 500):
        for _ in range(6):
            flux = (rng.gamma(0.6, 4.0, count) * (rng.random(count) < 0.7)).astype(np.float32)
            total += len(_same_picks(mxlib, flux))
            total += len(_same_picks(mxlib, flux, hop=64, first=11, pre_max=1, post_max=2, pre_avg=4, post_avg=3, wait=2, ratio=1.25,
                                     delta=0.5))
            _same_picks(mxlib, flux, pre_max=0, post_max=0, pre_avg=0, post_avg=0, wait=0, ratio=0.0, delta=0.0)
    assert total > 50  # (the random curves do hold onsets)


def test_pick_crafted_curves(mxlib):
    z = np.zeros(40, dtype=np.float32)
    # a plateau: its first index wins
    p = z.copy()
    p[10:14] = 5.0
    assert [int(o["frame"]) for o in _same_picks(mxlib, p)] == [10]
    # two peaks inside `wait`: the first is kept, the second dropped although it is the larger
    p = z.copy()
    p[10], p[15] = 5.0, 9.0
    assert [int(o["frame"]) for o in _same_picks(mxlib, p)] == [10]
    assert [int(o["frame"]) for o in _same_picks(mxlib, p, wait=4)] == [10, 15]
    # a peak at frame 0 and one at the last frame (clipped windows; frame 0's mean is over two values only)
    p = z.copy()
    p[0], p[-1] = 8.0, 8.0
    assert [int(o["frame"]) for o in _same_picks(mxlib, p, post_avg=3)] == [0, 39]
    assert [int(o["frame"]) for o in _same_picks(mxlib, p)] == [39]
    # NaN and Inf count as 0
    p = z.copy()
    p[5], p[6], p[20], p[30] = np.nan, np.inf, 6.0, -np.inf
    assert [int(o["frame"]) for o in _same_picks(mxlib, p)] == [20]
    # count 0 and 1
    assert len(_same_picks(mxlib, np.zeros(0, np.float32))) == 0
    assert len(_same_picks(mxlib, np.array([0.5], np.float32))) == 0
    assert len(_same_picks(mxlib, np.array([7.0], np.float32))) == 0  # (its own mean, doubled, is above it)
    one = _same_picks(mxlib, np.array([7.0], np.float32), hop=100, first=3, ratio=0.5)
    assert [(int(o["sample"]), int(o["frame"])) for o in one] == [(300, 3)]
    assert one[0]["strength"] == np.float32(7.0) and one[0]["margin"] == np.float32(2.5)


def _same_markers(mx, anchors, n, sr=SR, base=(), **params):
    got = mx.timing_markers(anchors, n, sr, base=list(base) if len(base) else None, **params)
    want = R.timing_markers(anchors, n, sr, base=base, **params)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert int(g["sample"]) == w[0]
        for k, v in zip(("note", "dTime", "pitchBend"), w[1:]):
            assert np.float64(g[k]).tobytes() == np.float64(v).tobytes(), (k, g, w)
    return got


def _tuples(markers):
    return [(int(m["sample"]), float(m["note"]), float(m["dTime"]), float(m["pitchBend"])) for m in markers]


def _random_case(rng, n=3 * SR, nanchors=12, nbase=0):
    anchors = np.sort(rng.choice(np.arange(0, n), nanchors, replace=False)).astype(np.int32)
    base = []
    if nbase:
        bs = np.sort(rng.choice(np.arange(1, n), 2 * nbase, replace=False))
        for i in range(nbase):
            note, bend = float(rng.uniform(30, 70)), float(rng.uniform(-1, 1))
            base += [(int(bs[2 * i]), note, 0.0, bend), (int(bs[2 * i + 1]), note, 0.0, bend)]
    return anchors, base


def test_timing_markers_equal_the_reference(mxlib):
    assert mxlib.timing_params_default() == R.TIMING_DEFAULTS
    rng = np.random.default_rng(11)
    n = 3 * SR
    for trial in range(12):
        anchors, base = _random_case(rng, n, nanchors=int(rng.integers(0, 20)), nbase=int(rng.integers(0, 5)))
        if trial == 0:
            anchors = np.concatenate([[0], anchors[anchors > 0]]).astype(np.int32)  # (an anchor at sample 0 is dropped)
        if trial == 1 and len(base):
            anchors = np.unique(np.concatenate([anchors, [base[0][0], n - 1]])).astype(np.int32)  # (an anchor ON a base sample)
        params = {} if trial % 3 == 0 else dict(bpm=float(rng.uniform(30, 250)), division=int(rng.integers(1, 9)),
                                                offset=float(rng.uniform(-0.2, 0.2)), strength=float(rng.uniform(0, 1)),
                                                max_shift=float(rng.uniform(0, 0.2)), max_stretch=float(rng.uniform(1, 4)))
        out = _same_markers(mxlib, anchors, n, base=base, **params)
        assert len(out) == len(set(int(a) for a in anchors if a > 0) | set(b[0] for b in base))
        assert np.all(np.diff(out["sample"]) > 0)
        # every renderer takes the list: it passes mx_pv_render_length
        from melonix_amd import _capi
        assert _capi.lib().mx_pv_render_length(n, SR, _capi.markers_array(_tuples(out)), len(out)) > 0
    assert len(_same_markers(mxlib, np.zeros(0, np.int32), n)) == 0


def test_anchors_land_where_the_monotone_pass_puts_them(mxlib):
    rng = np.random.default_rng(5)
    n = 3 * SR
    for nbase in (0, 3):
        anchors, base = _random_case(rng, n, 15, nbase)
        out = _tuples(mxlib.timing_markers(anchors, n, SR, base=base or None, max_shift=0.05))
        a, T = R.anchor_times(anchors, SR, max_shift=0.05)
        for ai, Ti in zip(a, T):
            assert abs(mxlib.sample2time(out, SR, ai) - Ti) <= 1e-9
        assert np.all(np.diff(T) > 0)


def test_full_strength_puts_unclamped_anchors_on_grid_lines(mxlib):
    # onsets of a take played a little off a 120 bpm sixteenth grid (g = 0.125 s): shifts of up to 40 ms, far from both clamps
    g = 60.0 / (120.0 * 4)
    rng = np.random.default_rng(3)
    lines = np.array([2, 5, 8, 12, 15, 19, 22])
    anchors = np.round((lines * g + rng.uniform(-0.04, 0.04, len(lines))) * SR).astype(np.int32)
    out = _tuples(mxlib.timing_markers(anchors, 3 * SR, SR))
    for a, q in zip(anchors, lines):
        assert abs(mxlib.sample2time(out, SR, int(a)) - q * g) <= 1e-9
    # with an offset the lines move with it
    out = _tuples(mxlib.timing_markers(anchors, 3 * SR, SR, offset=0.01))
    for a, q in zip(anchors, lines):
        assert abs(mxlib.sample2time(out, SR, int(a)) - (0.01 + q * g)) <= 1e-9


def test_strength_zero_is_the_identity(mxlib):
    rng = np.random.default_rng(9)
    anchors, base = _random_case(rng, 3 * SR, 20, 3)
    out = mxlib.timing_markers(anchors, 3 * SR, SR, base=base, strength=0.0)
    assert len(out) >= 20 and np.all(out["dTime"] == 0.0)
    out = mxlib.timing_markers(anchors, 3 * SR, SR, strength=0.0)
    assert np.all(out["dTime"] == 0.0)


def test_the_bend_over_the_source_is_unchanged(mxlib):
    rng = np.random.default_rng(13)
    n = 3 * SR
    anchors, base = _random_case(rng, n, 14, 4)
    out = _tuples(mxlib.timing_markers(anchors, n, SR, base=base))
    assert any(abs(m[2]) > 1e-3 for m in out)  # (the warp does move things)
    for s in rng.integers(1, n - 1, 300):
        warped = mxlib.time2pitchbend(out, SR, n, mxlib.sample2time(out, SR, int(s)))
        assert abs(warped - mxlib.time2pitchbend(base, SR, n, int(s) / SR)) <= 1e-6, s
    # the notes: base markers keep theirs, inserted ones lie between their neighbours'
    by_sample = {m[0]: m for m in out}
    for b in base:
        assert by_sample[b[0]][1] == b[1] and by_sample[b[0]][3] == b[3]
    assert all(min(b[1] for b in base) <= m[1] <= max(b[1] for b in base) for m in out)


def test_a_clamped_pair_keeps_span_times_max_stretch(mxlib):
    # two anchors 10 ms apart, 1 ms either side of the midpoint between two grid lines 200 ms apart: sent to those lines the
    # span would stretch 20-fold; it keeps span * max_stretch
    a0 = int(round((1.0 + 0.1 - 0.005) * SR))
    a1 = a0 + int(0.01 * SR)
    params = dict(bpm=75.0, division=4, offset=0.0, max_shift=0.2, max_stretch=2.0)  # g = 0.2 s
    a, T = R.anchor_times([a0, a1], SR, **params)
    assert abs(T[0] - 1.0) < 1e-9  # the first goes down to the line at 1.0 s
    out = _tuples(mxlib.timing_markers([a0, a1], 2 * SR, SR, **params))
    t0, t1 = mxlib.sample2time(out, SR, a0), mxlib.sample2time(out, SR, a1)
    assert abs((t1 - t0) - 2.0 * (a1 - a0) / SR) <= 1e-9
    # and the other clamp: an anchor sent far back keeps span / max_stretch
    out = _tuples(mxlib.timing_markers([a0, a1 + 10], 2 * SR, SR, bpm=75.0, division=4, offset=-0.09, max_shift=0.2, max_stretch=4.0))
    t0, t1 = mxlib.sample2time(out, SR, a0), mxlib.sample2time(out, SR, a1 + 10)
    assert abs((t1 - t0) - (a1 + 10 - a0) / SR / 4.0) <= 1e-9


def test_refusals(mxlib):
    n = SR
    ok = np.array([1000, 2000], np.int32)

    def refused(fn, *args, **kw):
        with pytest.raises(mxlib.MxError) as e:
            fn(*args, **kw)
        assert e.value.code == -1, e.value

    refused(mxlib.timing_markers, ok, n, SR, base=[(500, 40.0, 0.01, 0.0)])      # a base marker with a shift of its own
    refused(mxlib.timing_markers, ok, n, SR, base=[(500, 40.0, 0.0, 0.0), (500, 40.0, 0.0, 0.0)])
    refused(mxlib.timing_markers, ok, n, SR, base=[(0, 40.0, 0.0, 0.0)])
    refused(mxlib.timing_markers, ok, n, SR, base=[(n, 40.0, 0.0, 0.0)])
    refused(mxlib.timing_markers, np.array([2000, 1000], np.int32), n, SR)      # unsorted
    refused(mxlib.timing_markers, np.array([1000, 1000], np.int32), n, SR)
    refused(mxlib.timing_markers, np.array([1000, n], np.int32), n, SR)
    refused(mxlib.timing_markers, np.array([-1, 1000], np.int32), n, SR)
    refused(mxlib.timing_markers, ok, n, 0)
    refused(mxlib.timing_markers, ok, 0, SR)
    for bad in (dict(bpm=29.9), dict(bpm=250.1), dict(bpm=float("nan")), dict(division=0), dict(division=65), dict(offset=float("inf")),
                dict(strength=-0.01), dict(strength=1.01), dict(max_shift=-1.0), dict(max_shift=float("nan")), dict(max_stretch=0.99),
                dict(max_stretch=4.01)):
        refused(mxlib.timing_markers, ok, n, SR, **bad)
    flux = np.ones(8, np.float32)
    for bad in (dict(pre_max=-1), dict(post_max=4097), dict(pre_avg=-1), dict(post_avg=5000), dict(wait=-1), dict(ratio=-0.5),
                dict(ratio=float("nan")), dict(delta=float("inf")), dict(delta=-1.0)):
        refused(mxlib.onset_pick, flux, 256, **bad)
    refused(mxlib.onset_pick, flux, 0)
    refused(mxlib.onset_pick, flux, 256, -1)
    refused(mxlib.onset_pick, flux, 16384, 2 ** 31 // 16384)  # frame centres beyond int32 samples


@pytest.fixture(scope="module")
def onset_emu():
    """tests/emu/onset_emu.cpp: the kernel's per-lane functions run lane by lane, in the walker's order."""
    L = C.CDLL(emu_build.shared_object("onset_emu", ["onset_emu.cpp"], ["onset_walk_emu.h", "onset_core.h"]))
    fp = C.POINTER(C.c_float)
    L.emu_onset_flux.argtypes = [fp, C.c_long, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, fp]

    def run(w, hop, first, count, lag=1, band=(1, 511), compress=100.0, run=8):
        w = np.ascontiguousarray(w, dtype=np.float32)
        out = np.zeros(count, dtype=np.float32)
        L.emu_onset_flux(w.ctypes.data_as(fp), len(w), hop, first, count, lag, band[0], band[1], compress, run, out.ctypes.data_as(fp))
        return out

    return run


def test_the_kernels_arithmetic_on_the_cpu(onset_emu):
    """One wavefront's 8 x 8 x 8 transform, split, compression and reduction against the binary64 definition within the
    project's f32-versus-f64 yardstick, and the same bytes whatever the run length or the launch split."""
    w = R.notes(0.005)[:SR]
    for lag, fmin, fmax in ((1, 0.0, 0.0), (3, 100.0, 5000.0)):
        ref = R.flux(w, SR, 256, lag=lag, fmin=fmin, fmax=fmax)
        got = onset_emu(w, 256, 0, len(ref), lag, R.band(SR, fmin, fmax))
        assert np.abs(got - ref).max() <= 2e-5 * ref.max() + 1e-9
        assert onset_emu(w, 256, 0, len(ref), lag, R.band(SR, fmin, fmax), run=5).tobytes() == got.tobytes()
        assert onset_emu(w, 256, 37, 50, lag, R.band(SR, fmin, fmax), run=7).tobytes() == got[37:87].tobytes()
    assert not onset_emu(np.zeros(5000, np.float32), 255, 0, 20).any()


BAD_TAKE = (8000, 24000)  # notes5's samples: the first note's attack (sample 12000) and 0.21 s of the bed before it


@pytest.mark.parametrize("name", list(B.BAD))
def test_a_bad_sample_on_the_cpu(onset_emu, name):
    """A NaN sample makes the frames that hold it, and the frames `lag` later, NaN — where onset_ref.flux is not finite, frame
    for frame; an Inf sample leaves its frames not finite; every other frame keeps the clean take's bytes; the same bytes
    whatever the run or a split inside the affected frames (tests/bad_samples.py; tests/test_gpu_bad_samples.py asks the
    same of the device)."""
    w = R.notes(0.005)[BAD_TAKE[0]:BAD_TAKE[1]]
    n = len(w)
    for pos, s in B.positions(n, 256, 512, 512).items():
        v = B.with_bad(w, s, B.BAD[name])
        for lag in (1, 4):
            with np.errstate(invalid="ignore"):
                ref = R.flux(v, SR, 256, lag=lag) if name == "nan" else None
            B.check_flux(lambda first, count, run: onset_emu(v, 256, first, count, lag, run=run or 8),
                         lambda first, count, run: onset_emu(w, 256, first, count, lag, run=run or 8), ref, n, 256, lag, s, name,
                         (name, pos, lag))


# The emulation's worst error at compress = 1e6 over lags 1..4 on test_lags_and_high_compression's take, in units of the
# yardstick 2e-5 * max + 1e-9 (measured: 0.41, 0.31, 0.26, 0.24 for lags 1..4; 0.032 at 1e4, 0.15 at 1e5).  The device is allowed
# DEVICE_FACTOR times this in tests/test_gpu_onset.py: its log1pf and sqrtf are not libm's, and the emulation cannot vouch for them.
EMU_ERROR_AT_1E6 = 0.41
DEVICE_FACTOR = 4.0


@pytest.mark.parametrize("lag", [1, 2, 3, 4])
def test_lags_and_high_compression_on_the_cpu(onset_emu, lag):
    """compress at 1e4 and at 1e6, the top of the accepted range, on a take with a noise floor (notes30's first second: the 1e-4
    bed under the notes).  log1p(compress * m) has slope compress at m = 0, so the f32 transform's noise on the quiet bins
    (about 1e-7 of the frame's peak) is no longer small against the curve once compress * level passes about 1e4.  At 1e4 the
    yardstick holds; at 1e6 the emulation's worst error is EMU_ERROR_AT_1E6 = 0.41 of the yardstick on this take (libm's
    log1pf and sqrtf), which this test pins: the device's bound is derived from it."""
    w = R.notes(0.030)[:SR]
    for compress, share in ((1e4, 1.0), (1e6, EMU_ERROR_AT_1E6)):
        ref = R.flux(w, SR, 256, lag=lag, compress=compress)
        got = onset_emu(w, 256, 0, len(ref), lag, compress=compress)
        err, tol = np.abs(got - ref).max(), 2e-5 * ref.max() + 1e-9
        print(f"lag {lag} compress {compress:g}: worst error {err:.3e} = {err / tol:.3f} x the yardstick {tol:.3e}")
        assert err <= share * tol, (lag, compress, err / tol)


def test_the_chain_with_a_nan_on_the_cpu(mxlib, onset_emu):
    """notes5 with one NaN: the picker reads the affected frames as 0, mx_onset_pick equals onset_ref.pick on the emulation's
    flux, and every onset of the clean take whose decision window [f - pre_avg, f + max(post_max, post_avg)] does not reach an
    affected frame survives unchanged — five of the six (the condition on the reference alone: at least three quarters)."""
    w = R.notes(0.005)
    v = B.with_bad(w, CHAIN_NAN, np.nan)
    frames = B.frame_count(len(w), 256)
    with np.errstate(invalid="ignore"):
        ref_clean, ref_bad = R.flux(w, SR, 256), R.flux(v, SR, 256)
    keep = chain_survivors(R.pick(ref_clean, 256), R.pick(ref_bad, 256), len(w), "reference")
    assert len(keep) >= 0.75 * len(R.pick(ref_clean, 256))
    flux = onset_emu(v, 256, 0, frames)
    _same_picks(mxlib, flux)
    chain_survivors(R.pick(onset_emu(w, 256, 0, frames), 256), R.pick(flux, 256), len(w), "emulation")


CHAIN_NAN = 290 * 256 + 100  # inside the pre_avg window of notes5's fourth onset (frame 304), clear of the other five


def chain_survivors(clean, bad, n, what, lag=1):
    """clean / bad: onset_ref.pick lists (or the library's records as such tuples) of notes5 without / with the NaN at CHAIN_NAN.
    -> the clean onsets whose decision window holds no affected frame; each must be in `bad` unchanged.  The window is
    [f - wait - pre_avg, f + post_max]: the frames the local maximum and the mean read, and those of any frame close enough
    before f to take its place under `wait` (the take's onsets lie 75 frames and more apart: no longer chain exists)."""
    p = R.PICK_DEFAULTS
    hold = B.holding(n, 256, 512, 512, CHAIN_NAN)
    affected = np.nonzero(hold | B.lagged(hold, lag))[0]
    keep = []
    for o in clean:
        f = o[1]
        lo, hi = f - p["wait"] - max(p["pre_avg"], p["pre_max"]), f + max(p["post_max"], p["post_avg"])
        if not ((affected >= lo) & (affected <= hi)).any():
            keep.append(o)
    have = {o[1]: o for o in bad}
    for o in keep:
        assert o[1] in have, (what, o)
        assert (o[0], np.float32(o[2]).tobytes(), np.float32(o[3]).tobytes()) == (have[o[1]][0], np.float32(have[o[1]][2]).tobytes(),
                                                                                  np.float32(have[o[1]][3]).tobytes()), (what, o)
    return keep


def test_onset_kernels_do_not_spill():
    """Every instantiation (lag 1 to 4) keeps its rows, twiddles and window in registers: scratch-free, inside 256 VGPRs, and the
    4.5 KiB transposition image is all the LDS it takes."""
    names, scratch, vgprs, lds = emu_build.resource_usage("onset_kernels.hip")
    assert len(names) == 4 and all("onset_flux_kernel" in n for n in names)
    assert scratch == [0] * 4 and max(vgprs) <= 256 and lds == [4608] * 4
