"""Pitch drift and vibrato inside notes without a GPU (include/melonix_amd.h "Pitch drift and vibrato inside notes", "PSOLA
follows a bend curve"): the kernels' arithmetic (csrc/contour_core.h) run on the CPU by tests/emu/contour_emu.cpp against
tests/contour_ref.py — stage B byte for byte, stage A by the tie rule —, the library's host logic and its PSOLA plan with a bend
curve against the same reference field for field, the refusals, the chain on a synthetic contour, the kernels' resources."""
import ctypes as C
import math

import numpy as np
import pytest

import contour_ref as R
import emu_build
import psola_formant_ref
import psola_ref

EMU_SOURCES = ["contour_emu.cpp", "contour_logic.cpp"]
SR, HOP = 48000, 256
INVALID = -1


class Emu:
    def __init__(self, so):
        self.L = C.CDLL(so)
        self.L.emu_contour_cents.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_float, C.c_void_p]
        self.L.emu_contour_cents.restype = None
        self.L.emu_contour_split.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p]
        self.L.emu_contour_check_params.argtypes = [C.c_void_p]
        self.L.emu_contour_check_spans.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p]

    def cents(self, track, sr, threshold=0.15, rms_floor=1e-3):
        track = np.ascontiguousarray(track, dtype=R.F0_DTYPE)
        out = np.empty(len(track), dtype=np.int32)
        self.L.emu_contour_cents(track.ctypes.data, len(track), sr, threshold, rms_floor, out.ctypes.data)
        return out

    def split(self, cents, spans, w, lag_min, lag_max, tile=256, stat_tile=1024):
        cents = np.ascontiguousarray(cents, dtype=np.int32)
        sp = np.array([tuple(s) for s in spans], dtype=R.SPAN_DTYPE)
        p = np.array([w, lag_min, lag_max], dtype=np.int32)
        rec, stat = np.empty(len(cents), dtype=R.REC_DTYPE), np.empty(len(sp), dtype=R.STAT_DTYPE)
        rc = self.L.emu_contour_split(cents.ctypes.data, len(cents), sp.ctypes.data, len(sp), p.ctypes.data, tile, stat_tile,
                                      rec.ctypes.data, stat.ctypes.data)
        assert rc == 0, rc
        return rec, stat

    def params_ok(self, w, lag_min, lag_max):
        p = np.array([w, lag_min, lag_max], dtype=np.int32)
        return self.L.emu_contour_check_params(p.ctypes.data) == 0

    def spans_ok(self, spans, count, cents=None):
        sp = np.array([tuple(s) for s in spans], dtype=R.SPAN_DTYPE)
        c = None if cents is None else np.ascontiguousarray(cents, dtype=np.int32)
        return self.L.emu_contour_check_spans(sp.ctypes.data, len(sp), count, None if c is None else c.ctypes.data) == 0


@pytest.fixture(scope="module")
def contour_emu():
    return Emu(emu_build.shared_object("contour_emu", EMU_SOURCES, ["contour_core.h", "contour_logic.h"]))


# ---- stage B: the emulation equals the reference exactly ----
@pytest.mark.parametrize("kind", ["voice", "negative", "constant"])
def test_split_equals_the_reference_over_the_span_shapes(contour_emu, kind):
    cents = R.case_cents(kind)
    for w in R.CASE_WIDTHS:
        for lag_min, lag_max in R.CASE_LAGS:
            want_rec, want_stat = R.split(cents, R.CASE_SPANS, w, lag_min, lag_max)
            rec, stat = contour_emu.split(cents, R.CASE_SPANS, w, lag_min, lag_max)
            assert rec.tobytes() == want_rec.tobytes(), (kind, w)
            assert stat.tobytes() == want_stat.tobytes(), (kind, w, lag_min, lag_max)
    if kind == "constant":
        assert not want_rec["vib"].any() and not want_stat["r0"].any()
    if kind == "negative":
        assert (cents[cents != R.NONE] < 0).all()
    # the last lag range, 200 .. 256, exceeds every span but the two longest: no lag, lag = 0
    assert [int(l) != 0 for l in want_stat["lag"]] == [F - 1 >= 200 for _, F in R.CASE_SPANS]
    assert not want_stat["r_lag"][want_stat["lag"] == 0].any()
    # outside every span
    inside = np.zeros(R.CASE_COUNT, dtype=bool)
    for first, F in R.CASE_SPANS:
        inside[first:first + F] = True
    assert (want_rec["smooth"][~inside] == R.NONE).all() and not want_rec["vib"][~inside].any()


def test_split_does_not_depend_on_the_tiling(contour_emu):
    cents = R.case_cents("voice")
    want = R.split(cents, R.CASE_SPANS, 23, 15, 62)
    for tile, stat_tile in [(1, 1), (7, 13), (64, 100), (256, 1024), (1000, 5000)]:
        rec, stat = contour_emu.split(cents, R.CASE_SPANS, 23, 15, 62, tile, stat_tile)
        assert rec.tobytes() == want[0].tobytes() and stat.tobytes() == want[1].tobytes(), (tile, stat_tile)


def test_one_long_span_equals_the_reference(contour_emu):
    cents = R.case_cents("voice", 70000, [(0, 70000)])
    want_rec, want_stat = R.split(cents, [(0, 70000)], 23, 15, 62)
    rec, stat = contour_emu.split(cents, [(0, 70000)], 23, 15, 62)
    assert rec.tobytes() == want_rec.tobytes() and stat.tobytes() == want_stat.tobytes()
    assert int(stat["lag"][0]) == 33  # one 5.7 Hz period at 187.5 frames/s is 32.9 frames


def test_the_mean_rounds_halves_up_and_floors_toward_minus_infinity(contour_emu):
    # two taps: (a + b) / 2 with a + b odd lies on a half; -3/2 -> -1, 3/2 -> 2
    for a, b, want in [(-2, -1, -1), (1, 2, 2), (-1, 0, 0), (-3, -2, -2), (-5, -5, -5)]:
        rec, _ = contour_emu.split([a, b], [(0, 2)], 1, 1, 1)
        ref, _ = R.split(np.array([a, b]), [(0, 2)], 1, 1, 1)
        # pass 1 gives [m, m], pass 2 the same m
        assert rec["smooth"].tolist() == [want, want] == ref["smooth"].tolist(), (a, b)


# ---- stage A ----
def stage_a_track():
    rng = np.random.default_rng(11)
    periods = np.concatenate([rng.uniform(27.0, 873.0, 3000), np.arange(27, 540, dtype=np.float64), [1e-3, 1e6, 2047.5]])
    return R.track_of(periods.astype(np.float32))


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
def test_cents_equal_the_reference_away_from_ties(contour_emu, sr):
    track = stage_a_track()
    voiced, x = R.cents_exact(track, sr)
    assert voiced.all()
    near = R.tie_distance(x) <= 1e-6
    assert not near.any()  # the periods are picked so that the reference alone leaves out none
    got, want = contour_emu.cents(track, sr), R.cents(track, sr)
    differ = got != want
    assert not (differ & ~near).any()
    assert (np.abs(got.astype(np.int64) - want)[differ] <= 1).all() and differ.sum() * 1000 <= len(track)
    if sr == 8000:
        assert (want[track["period"] > 600] < 0).all()  # negative at low sample rates


def test_unvoiced_frames_give_none(contour_emu):
    t = R.track_of(np.full(9, 200.0, dtype=np.float32))
    t["tau"][1] = 0
    t["aperiodicity"][2] = np.float32(0.15)  # (not below the threshold)
    t["rms"][3] = np.float32(0.5e-3)
    t["period"][4:8] = [np.nan, np.inf, 0.0, -3.0]
    t["aperiodicity"][8] = np.nan
    got = contour_emu.cents(t, SR)
    assert got.tolist() == R.cents(t, SR).tolist()
    assert (got[1:] == R.NONE).all() and got[0] == int(np.rint(16.0 * (1200.0 * np.log2(48000.0 / 200.0 / 55.0) + 2400.0)))


# ---- host logic ----
def notes_of(spans, notes, first_frame=0, mxlib=None):
    out = np.zeros(len(spans), dtype=mxlib.NOTE_DTYPE)
    for i, (first, F) in enumerate(spans):
        out[i] = (0, 0, first + first_frame, F, notes[i], 0.05, 0.1)
    return out


def test_default_parameters(mxlib):
    for sr, hop in [(48000, 256), (44100, 512), (8000, 64), (48000, 16384), (192000, 1), (1, 16384)]:
        assert mxlib.contour_params_default(sr, hop) == R.params_default(sr, hop), (sr, hop)
    assert mxlib.contour_params_default(48000, 256) == {"half_width": 23, "lag_min": 15, "lag_max": 63}
    assert mxlib.bend_params_default() == R.BEND_DEFAULTS


def test_spans_of_notes(mxlib):
    spans = [(3, 10), (13, 8), (40, 9)]
    notes = notes_of(spans, [45.0, 46.0, 47.0], first_frame=1000, mxlib=mxlib)
    got = mxlib.contour_spans(notes, 1000)
    assert got.tobytes() == R.spans_of(notes, 1000).tobytes() and [tuple(s) for s in got.tolist()] == spans
    assert len(mxlib.contour_spans(notes[:0], 0)) == 0


def test_vibrato_figures_are_field_exact(mxlib):
    cents = R.case_cents("voice")
    _, stat = R.split(cents, R.CASE_SPANS, 23, 15, 62)
    for s, (_, F) in zip(stat, R.CASE_SPANS):
        got, want = mxlib.contour_vibrato(s, F, SR, HOP), R.vibrato(s, F, SR, HOP)
        assert got == want, (F, got, want)
    assert any(v["rate_hz"] > 0 for v in (R.vibrato(s, F, SR, HOP) for s, (_, F) in zip(stat, R.CASE_SPANS)))
    zero = {"rate_hz": 0.0, "extent_cents": 0.0, "strength": 0.0, "drift_cents": 0.0}
    flat = R.split(R.case_cents("constant"), R.CASE_SPANS, 23, 15, 62)[1]
    assert mxlib.contour_vibrato(flat[4], 300, SR, HOP) == zero  # r0 == 0
    assert mxlib.contour_vibrato(stat[0], 2, SR, HOP) == zero    # lag == 0


def bend_case(mxlib, glide=8):
    """Notes with gaps of glide, glide + 1 and 0 frames, and one frame of gap."""
    spans = [(5, 40), (45 + glide, 30), (75 + glide + glide + 1, 20), (95 + 2 * glide + 1, 25), (121 + 2 * glide + 1, 12)]
    count = 160 + 2 * glide
    rng = np.random.default_rng(3)
    cents = np.full(count, R.NONE, dtype=np.int64)
    notes = []
    for first, F in spans:
        c = 16.0 * (4400.0 + 100.0 * len(notes)) + 300.0 * np.sin(np.arange(F) / 5.0) + rng.integers(-20, 21, F)
        cents[first:first + F] = np.rint(c)
        notes.append(float(np.median(cents[first:first + F])) / 1600.0)
    rec, _ = R.split(cents.astype(np.int32), spans, 5, 2, 10)
    return rec, notes_of(spans, notes, mxlib=mxlib), spans


@pytest.mark.parametrize("params", [{}, {"drift_amount": 1.0, "vibrato_scale": 0.0}, {"drift_amount": 0.0, "vibrato_scale": 2.0},
                                    {"drift_amount": 0.37, "vibrato_scale": 3.3, "glide_frames": 0},
                                    {"glide_frames": 9}, {"glide_frames": 1}])
def test_bend_is_field_exact(mxlib, params):
    rec, notes, spans = bend_case(mxlib)
    shift = np.array([0.25, -0.5, 0.0, 1.0 / 3.0, -0.125])
    for sh in (None, shift):
        got = mxlib.contour_bend(rec, notes, spans, sh, **params)
        want = R.bend(rec, notes, spans, sh, **dict(R.BEND_DEFAULTS, **params))
        assert got.tobytes() == want.tobytes(), (params, sh is None)
    glide = params.get("glide_frames", 8)
    gap8, gap9 = slice(45, 53), slice(83, 92)  # the gaps of 8 and 9 frames
    assert want[gap8].any() == (glide >= 8) and want[gap9].any() == (glide >= 9)
    assert not want[:5].any() and not want[-5:].any()


def test_bend_flattens_a_note_and_handles_a_single_note(mxlib):
    rec, notes, spans = bend_case(mxlib)
    one = mxlib.contour_bend(rec, notes[:1], spans[:1], None, drift_amount=1.0, vibrato_scale=0.0)
    assert one.tobytes() == R.bend(rec, notes[:1], spans[:1], None, 1.0, 0.0, 8).tobytes()
    assert not one[45:].any()
    # drift 1, vibrato 0, shift T - note: cents / 1600 + bend is T in every frame, to the float's rounding
    T = np.rint(notes["note"])
    b = mxlib.contour_bend(rec, notes, spans, T - notes["note"], drift_amount=1.0, vibrato_scale=0.0)
    for i, (first, F) in enumerate(spans):
        sl = slice(first, first + F)
        cents = rec["smooth"][sl].astype(np.float64) + rec["vib"][sl]
        assert np.abs(cents / 1600.0 + b[sl] - T[i]).max() < 1e-6
    assert len(mxlib.contour_bend(rec[:0], notes[:0], [], None)) == 0


# ---- the PSOLA plan with a bend curve ----
def plan_take(seconds=0.5, f0=220.0, unvoiced=(40, 50)):
    n = int(SR * seconds)
    count = (n + HOP - 1) // HOP
    periods = np.full(count, SR / f0) * (1.0 + 0.01 * np.sin(np.arange(count) / 7.0))
    voiced = np.ones(count, dtype=bool)
    voiced[unvoiced[0]:unvoiced[1]] = False
    return n, R.track_of(periods, voiced)


def bend_curve(count, seed=1):
    rng = np.random.default_rng(seed)
    return (0.8 * np.sin(np.arange(count) / 9.0) + rng.uniform(-0.1, 0.1, count)).astype(np.float32)


MARKERS = [(6000, 45.0, 0.0, 0.5), (18000, 45.0, 0.1, -0.75)]  # a bend ramp and a time-stretch
POINTS = [(0, -2.0), (12000, 3.0), (20000, 0.5)]


@pytest.mark.parametrize("markers", [[], MARKERS])
def test_plan_with_no_curve_or_zeros_is_the_plain_plan(mxlib, markers):
    n, track = plan_take()
    want, L = mxlib.psola_plan(n, SR, HOP, track, markers)
    wantf, Lf = mxlib.psola_plan_formant(n, SR, HOP, track, markers, POINTS)
    for curve in (None, np.zeros(len(track), dtype=np.float32), -np.zeros(len(track), dtype=np.float32)):
        got, Lg = mxlib.psola_plan_bend(n, SR, HOP, track, markers, curve)
        assert got.tobytes() == want.tobytes() and Lg == L
        gotf, Lgf = mxlib.psola_plan_formant_bend(n, SR, HOP, track, markers, POINTS, curve)
        assert gotf.tobytes() == wantf.tobytes() and Lgf == Lf
    assert len(want) > 100


@pytest.mark.parametrize("markers", [[], MARKERS])
def test_plan_with_a_curve_equals_the_reference(mxlib, markers):
    n, track = plan_take()
    curve = bend_curve(len(track))
    got, L = mxlib.psola_plan_bend(n, SR, HOP, track, markers, curve)
    want, Lw = R.plan_bend(n, SR, HOP, track, markers, curve)
    assert L == Lw and len(got) == len(want)
    for f in psola_ref.GRAIN_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
    assert got.tobytes() != mxlib.psola_plan(n, SR, HOP, track, markers)[0].tobytes()
    gotf, _ = mxlib.psola_plan_formant_bend(n, SR, HOP, track, markers, POINTS, curve)
    wantf, _ = R.plan_formant_bend(n, SR, HOP, track, markers, POINTS, curve)
    for f in psola_formant_ref.FGRAIN_DTYPE.names:
        assert np.array_equal(gotf[f], wantf[f]), f
    # the reference with no curve is psola_ref's own plan
    assert R.plan_bend(n, SR, HOP, track, markers, None)[0].tobytes() == psola_ref.plan(n, SR, HOP, track, markers)[0].tobytes()


def test_the_curve_follows_a_time_stretch(mxlib):
    """A constant period, a curve that is +3 semitones on source frames [30, 60) and 0 elsewhere, and a marker pair that
    stretches the first half of the file to twice its length: every voiced grain's spacing is its period over the ratio of
    the SOURCE frame its analysis mark reads, wherever the stretch has put the grain in the output."""
    n = 24000
    count = (n + HOP - 1) // HOP
    P = 200.0
    track = R.track_of(np.full(count, P))
    curve = np.zeros(count, dtype=np.float32)
    curve[30:60] = 3.0
    markers = [(12000, 45.0, 0.25, 0.0), (24000, 45.0, 0.0, 0.0)]  # 12000 samples take 0.25 s longer: twice as long
    g, L = mxlib.psola_plan_bend(n, SR, HOP, track, markers, curve)
    assert L > n + 11000
    s = g["centre"].astype(np.float64) + g["centre_frac"]
    a = psola_ref.marks(n, HOP, track)[0]
    frame = np.array([min(max(math.floor((a[m] + (2048.0 - P) / 2.0) / HOP + 0.5), 0), count - 1) for m in g["mark"]])
    ratio = np.where((frame >= 30) & (frame < 60), 2.0 ** (3.0 / 12.0), 1.0)
    assert np.abs(np.diff(s) - P / ratio[:-1]).max() < 1e-3  # (centre_frac is a float: 2^-24 of a few 10^4 samples)
    bent = s[:-1][ratio[:-1] > 1.0]
    # frames 30 .. 59 measure source samples 7552 - 924 .. 15232 - 924 (the tracker's lead at this period): the stretch puts
    # them at outputs 2 * 6628 = 13256 .. 24000 + (14308 - 12000) = 26308, give or take one (stretched) period
    assert abs(bent.min() - 13256) < 2 * P and abs(bent.max() - 26308) < 2 * P
    assert abs(len(bent) - (26308 - 13256) / (P / 2.0 ** 0.25)) < 3


# ---- refusals ----
def test_refusals(mxlib, contour_emu):
    from melonix_amd import _capi
    L = _capi.lib()
    E = contour_emu
    # parameters of the split
    for ok in [(0, 1, 1), (64, 1, 256), (23, 15, 63), (0, 256, 256)]:
        assert E.params_ok(*ok), ok
    for bad in [(-1, 1, 1), (65, 1, 1), (0, 0, 1), (0, 2, 1), (0, 1, 257), (0, 257, 257)]:
        assert not E.params_ok(*bad), bad
    # spans
    cents = np.full(100, 70000, dtype=np.int32)
    for ok in [[], [(0, 100)], [(0, 1), (1, 1), (99, 1)], [(10, 20), (30, 70)]]:
        assert E.spans_ok(ok, 100, cents), ok
    for bad in [[(0, 0)], [(-1, 5)], [(0, 101)], [(99, 2)], [(10, 20), (29, 5)], [(30, 5), (10, 5)], [(5, -2)], [(2 ** 31 - 1, 2 ** 31 - 1)]]:
        assert not E.spans_ok(bad, 100, cents), bad
    cents[50] = R.NONE
    assert E.spans_ok([(0, 50), (51, 49)], 100, cents) and not E.spans_ok([(0, 51)], 100, cents)
    # the entry points that take a context refuse a null one, and the rest of their arguments before any device call
    p = _capi.ContourParams(23, 15, 63)
    out = np.zeros(128, dtype=np.int64)
    assert L.mx_contour_cents(None, out.ctypes.data, 4, SR, 0.15, 1e-3, out.ctypes.data) == INVALID
    assert L.mx_contour_cents_dev(None, out.ctypes.data, 4, SR, 0.15, 1e-3, out.ctypes.data) == INVALID
    assert L.mx_contour_split(None, out.ctypes.data, 4, None, 0, C.byref(p), out.ctypes.data, None) == INVALID
    assert L.mx_contour_split_dev(None, out.ctypes.data, 4, None, 0, C.byref(p), out.ctypes.data, None) == INVALID
    assert L.mx_pitch_contour(None, out.ctypes.data, 4, SR, HOP, 0, None, 0, 0.15, 1e-3, None, out.ctypes.data, None) == INVALID
    # defaults
    q = _capi.ContourParams()
    for sr, hop in [(0, 256), (-1, 256), (SR, 0), (SR, 16385)]:
        assert L.mx_contour_params_default(sr, hop, C.byref(q)) == INVALID
    assert L.mx_contour_params_default(SR, HOP, None) == INVALID
    # spans of notes
    assert L.mx_contour_spans(None, 1, 0, out.ctypes.data) == INVALID and L.mx_contour_spans(out.ctypes.data, -1, 0, out.ctypes.data) == INVALID
    # vibrato
    stat = np.zeros(1, dtype=R.STAT_DTYPE)
    stat["lag"], stat["r0"], stat["r_lag"] = 10, 100, 50
    v = _capi.Vibrato()
    assert L.mx_contour_vibrato(stat.ctypes.data, 11, SR, HOP, C.byref(v)) == 0
    for frames, sr, hop in [(10, SR, HOP), (0, SR, HOP), (-4, SR, HOP), (11, 0, HOP), (11, SR, 0), (11, SR, 16385)]:
        assert L.mx_contour_vibrato(stat.ctypes.data, frames, sr, hop, C.byref(v)) == INVALID, (frames, sr, hop)
    assert L.mx_contour_vibrato(None, 11, SR, HOP, C.byref(v)) == INVALID and L.mx_contour_vibrato(stat.ctypes.data, 11, SR, HOP, None) == INVALID
    # bend
    rec, notes, spans = bend_case(mxlib)
    for bad in [{"drift_amount": -0.1}, {"drift_amount": 1.1}, {"drift_amount": math.nan}, {"vibrato_scale": -1.0},
                {"vibrato_scale": 4.5}, {"vibrato_scale": math.inf}, {"glide_frames": -1}]:
        with pytest.raises(mxlib.MxError):
            mxlib.contour_bend(rec, notes, spans, None, **bad)
    for bad_shift in (math.nan, math.inf):
        with pytest.raises(mxlib.MxError):
            mxlib.contour_bend(rec, notes, spans, [0.0, bad_shift, 0.0, 0.0, 0.0])
    with pytest.raises(mxlib.MxError):
        mxlib.contour_bend(rec, notes, [(5, 40), (44, 30)] + spans[2:], None)  # overlapping spans
    with pytest.raises(mxlib.MxError):
        mxlib.contour_bend(rec[:100], notes, spans, None)  # spans beyond the array
    nan_note = notes.copy()
    nan_note["note"][2] = math.nan
    with pytest.raises(mxlib.MxError):
        mxlib.contour_bend(rec, nan_note, spans, None)
    # the plan: a value of the curve that is not finite, and what the plain plan refuses
    n, track = plan_take()
    for bad in (math.nan, math.inf, -math.inf):
        curve = bend_curve(len(track))
        curve[17] = bad
        for call in (lambda: mxlib.psola_plan_bend(n, SR, HOP, track, [], curve),
                     lambda: mxlib.psola_plan_formant_bend(n, SR, HOP, track, [], POINTS, curve)):
            with pytest.raises(mxlib.MxError) as e:
                call()
            assert e.value.code == INVALID
    curve = bend_curve(len(track))
    for call in (lambda: mxlib.psola_plan_bend(n + HOP, SR, HOP, track, [], curve),  # count != frame_count(n, hop)
                 lambda: mxlib.psola_plan_bend(n, 0, HOP, track, [], curve),
                 lambda: mxlib.psola_plan_bend(n, SR, HOP, track, [], curve, unvoiced_period=8.0),
                 lambda: mxlib.psola_plan_formant_bend(n, SR, HOP, track, [], [(5, 0.0), (5, 1.0)], curve)):
        with pytest.raises(mxlib.MxError):
            call()


# ---- the chain on a synthetic contour ----
def chain(mxlib, contour_emu, x):
    """cents (binary64 units) of one 400-frame note -> the library's vibrato figures of the emulated split at the defaults."""
    cents = np.rint(x).astype(np.int32)
    p = mxlib.contour_params_default(SR, HOP)
    rec, stat = contour_emu.split(cents, [(0, len(cents))], p["half_width"], p["lag_min"], p["lag_max"])
    assert rec.tobytes() == R.split(cents, [(0, len(cents))], **p)[0].tobytes()
    return mxlib.contour_vibrato(stat[0], len(cents), SR, HOP), stat[0]


def test_chain_on_a_synthetic_contour(mxlib, contour_emu):
    """centre + a linear 30-cent drift + 40 cents x sin(2 pi 6 Hz) at 187.5 frames/s, 400 frames, the defaults.
    Observed: lag 31, extent_cents 38.23, drift_cents 27.25 beside the reference's 27.38 for the drift alone."""
    v, stat = chain(mxlib, contour_emu, R.synthetic_cents())
    assert int(stat["lag"]) == int(np.rint(R.FPS / 6.0)) == 31
    assert abs(v["rate_hz"] - 6.0) < 0.1
    # the 250 ms triangle passes about 5 % of a 6 Hz vibrato into `smooth`; the margin is twice that
    assert abs(v["extent_cents"] - 40.0) <= 4.0, v
    # the part of the 30 cents that is not lost at the clipped edges: the reference's split of the drift alone
    alone = np.rint(R.synthetic_cents(extent_cents=0.0)).astype(np.int32)
    p = R.params_default(SR, HOP)
    _, st = R.split(alone, [(0, 400)], **p)
    want = (float(st["max_smooth"][0]) - float(st["min_smooth"][0])) / 16.0
    assert 20.0 < want < 30.0
    assert abs(v["drift_cents"] - want) <= 0.1 * want, (v, want)
    assert v["strength"] > 0.9
    print(f"chain: lag {int(stat['lag'])}, extent_cents {v['extent_cents']:.2f}, drift_cents {v['drift_cents']:.2f} (drift alone {want:.2f})")


def test_emulation_under_the_sanitizers(tmp_path):
    out = emu_build.run_sanitized(tmp_path, "contour_emu_san", EMU_SOURCES, "CONTOUR_EMU_MAIN")
    assert "contour_emu ok" in out, out


def test_kernels_use_no_scratch_and_little_lds(mxlib):
    names, scratch, _, lds = emu_build.resource_usage("contour_kernels.hip")
    assert len(names) == 4
    assert scratch == [0] * 4
    assert max(lds) <= 8192, lds
