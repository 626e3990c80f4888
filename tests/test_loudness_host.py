"""Loudness and note levelling without a GPU (include/melonix_amd.h "Loudness and note levelling"): the K-weighting
coefficients against the formulas and the table of BS.1770-4; the kernel's per-lane arithmetic (csrc/loudness_core.h) run on the
CPU by tests/emu/loudness_emu.cpp against tests/loudness_ref.py, byte for byte; the library's host logic (curve, gating, note
loudness, levelling points, export gain) against the reference; known answers measured by the reference; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import emu_build
import loudness_ref as L

RATES = (48000, 44100, 8000)


def as_lib(mx, st):
    """reference records as the library's dtype (the same 16 bytes)"""
    return np.frombuffer(st.tobytes(), dtype=mx.LOUD_STEP_DTYPE)


@pytest.fixture(scope="module")
def emu(mxlib):
    lib = C.CDLL(emu_build.shared_object("loudness_emu", ["loudness_emu.cpp"], ["loudness_core.h", "step_core.h"]))
    lib.emu_loudness_steps.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p]

    def steps(w, sr, k, first_group=0, ngroups=None):
        w = np.ascontiguousarray(w, dtype=np.float32)
        S, _, nsteps, groups = L.geometry(len(w), sr)
        ngroups = groups - first_group if ngroups is None else ngroups
        out = np.zeros(max(min(L.G * (first_group + ngroups), nsteps) - L.G * first_group, 0), dtype=L.STEP_DTYPE)
        k = np.ascontiguousarray(k, dtype=np.float64)
        lib.emu_loudness_steps(w.ctypes.data, len(w), sr, first_group, ngroups, k.ctypes.data, out.ctypes.data)
        return out

    return steps


@pytest.fixture(scope="module")
def measured(mxlib):
    """name -> (sr, reference records, read-only): the takes the host logic is checked on, each filtered once."""
    sr = 48000
    nan_take = L.gated_take(sr).copy()
    nan_take[3 * sr + 77] = np.nan
    takes = {"gated": (sr, L.gated_take(sr)), "noise_partial": (sr, L.noise(5 * sr + 1234)), "nan": (sr, nan_take),
             "sine997": (sr, L.tone(sr, 997.0, 1.0, 1.5)), "sine997_441": (44100, L.tone(44100, 997.0, 1.0, 1.5)),
             "levelling": (L.LEVEL_SR, L.levelling_take()[0])}
    out = {}
    for name, (rate, w) in takes.items():
        st = L.steps(w, rate, mxlib.loudness_coeffs(rate))
        st.setflags(write=False)
        out[name] = (rate, st)
    return out


@pytest.mark.parametrize("sr", RATES + (384000, 96000))
def test_coefficients_are_the_formulas(mxlib, sr):
    got, ref = mxlib.loudness_coeffs(sr), L.coeffs(sr)
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (got, ref)
    assert got[5:8].tobytes() == np.array([1.0, -2.0, 1.0]).tobytes()


def test_coefficients_at_48k_are_the_table_of_bs1770(mxlib):
    got = mxlib.loudness_coeffs(48000)
    seven = np.concatenate([got[:5], got[8:]])
    table = np.array(L.BS1770_TABLE)
    print("relative difference to the table:", np.abs(seven - table) / np.abs(table))
    assert np.all(np.abs(seven - table) <= 1e-12 * np.abs(table))
    assert np.all(np.abs(np.concatenate([L.coeffs(48000)[:5], L.coeffs(48000)[8:]]) - table) <= 1e-12 * np.abs(table))


def test_geometry(mxlib):
    assert L.geometry(1, 48000)[:2] == (480, 4096) and L.geometry(1, 44100)[:2] == (441, 3764)
    assert L.geometry(1, 384000)[:2] == (3840, mxlib.MX_AUDIO_PAD) and L.geometry(1, 8000)[:2] == (80, 684)
    for sr in RATES + (384000, 11025):
        S = L.geometry(0, sr)[0]
        for n in (0, 1, S - 1, S, S + 1, 10 * S + 1, 12345678):
            assert mxlib.loudness_step_count(n, sr) == L.geometry(n, sr)[2], (n, sr)
    assert mxlib.loudness_step_count(-5, 48000) == 0
    assert mxlib.loudness_step_count(1000, 7999) == 0 and mxlib.loudness_step_count(1000, 384001) == 0


@pytest.mark.parametrize("sr", RATES)
def test_the_kernels_arithmetic_on_the_cpu(mxlib, emu, sr):
    """loudness_core.h, lane by lane, gives the reference's bytes: an odd length with a partial last step, several groups, the
    whole take and any split into group ranges."""
    k = mxlib.loudness_coeffs(sr)
    S = L.geometry(0, sr)[0]
    n = 3 * 10 * S + 1234 if sr != 44100 else 7 * 10 * S + 17
    w = L.noise(n, seed=sr)
    w[5 * S:6 * S] = 0.0
    w[6 * S] = -0.75
    ref = L.steps(w, sr, k)
    got = emu(w, sr, k)
    assert len(ref) == -(-n // S) and got.tobytes() == ref.tobytes()
    assert ref["samples"][-1] == n - (len(ref) - 1) * S and np.all(ref["samples"][:-1] == S)
    assert ref["peak"][6] == np.float32(0.75) and ref["peak"][5] == 0 and ref["energy"][5] > 0  # (the filter rings on)
    groups = L.geometry(n, sr)[3]
    parts = [emu(w, sr, k, 0, 2), emu(w, sr, k, 2, groups - 2)]
    assert b"".join(p.tobytes() for p in parts) == ref.tobytes()
    assert emu(w, sr, k, 1, 1).tobytes() == ref[10:20].tobytes()
    assert L.steps(w, sr, k, 1, 2).tobytes() == ref[10:30].tobytes()  # (and the reference's own split)


def test_smallest_lengths_on_the_cpu(mxlib, emu):
    sr = 8000
    k, S = mxlib.loudness_coeffs(sr), 80
    for n in (1, S - 1, S, S + 1, 10 * S, 10 * S + 1):
        w = L.noise(n, seed=n)
        ref = L.steps(w, sr, k)
        assert len(ref) == -(-n // S) and ref["samples"].sum() == n
        assert emu(w, sr, k).tobytes() == ref.tobytes(), n


def test_silence_and_the_power_of_two_law_on_the_cpu(mxlib, emu):
    sr = 8000
    k, S = mxlib.loudness_coeffs(sr), 80
    for w in (np.zeros(25 * S + 3, np.float32), np.full(25 * S + 3, -0.0, np.float32)):
        for st in (L.steps(w, sr, k), emu(w, sr, k)):
            assert st["energy"].tobytes() == np.zeros(len(st)).tobytes() and st["peak"].tobytes() == np.zeros(len(st), np.float32).tobytes()
    w = L.noise(25 * S + 3, seed=3)
    base = emu(w, sr, k)
    for p in (-7, 20, -20):
        scaled = emu(w * np.float32(2.0 ** p), sr, k)
        assert scaled["energy"].tobytes() == (base["energy"] * 4.0 ** p).tobytes(), p
        assert scaled["peak"].tobytes() == (base["peak"] * np.float32(2.0 ** p)).tobytes(), p
        assert L.steps(w * np.float32(2.0 ** p), sr, k).tobytes() == scaled.tobytes()


def _close(a, b, tol=1e-9):
    return (a == b) or (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


@pytest.mark.parametrize("name", ["gated", "noise_partial", "nan", "sine997", "levelling"])
def test_gating_and_curves_match_the_reference(mxlib, measured, name):
    """Gate decisions and counts exactly, values to 1e-9 LU (only log10 may differ by an ulp)."""
    sr, st = measured[name]
    rec = as_lib(mxlib, st)
    got, ref = mxlib.loudness_integrated(rec, sr), L.integrated(st, sr)
    print(name, got, ref)
    for key in ("blocks", "passed_abs", "passed_rel", "bad_blocks"):
        assert got[key] == ref[key], key
    assert np.float32(got["peak"]).tobytes() == np.float32(ref["peak"]).tobytes()
    for key in ("integrated", "momentary_max", "shortterm_max"):
        assert _close(got[key], ref[key]), key
    for window in (1, 40, 300):
        a, b = mxlib.loudness_curve(rec, sr, window), L.curve(st, sr, window)
        assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.array_equal(np.isnan(a), np.isnan(b)), window
        ok = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), ok) and np.all(np.abs(a[ok] - b[ok]) <= 1e-9), window
        assert np.all(np.isneginf(a[:window - 1]))
    if name == "noise_partial":  # the partial last step is in no window and no block
        assert st["samples"][-1] != L.geometry(0, sr)[0] and np.isneginf(mxlib.loudness_curve(rec, sr, 1)[-1])
        assert got["blocks"] == (len(st) - 1 - 40) // 10 + 1
    if name == "nan":
        assert got["bad_blocks"] > 0 and math.isfinite(got["integrated"])
    if name == "levelling":
        assert got["shortterm_max"] == -math.inf  # (shorter than 3 s)


def test_known_answers(measured):
    """Measured by the reference, not by the code under test.  BS.1770's own statement: a 0 dBFS 997 Hz sine reads -3.01 LKFS."""
    for name, expected in (("sine997", -3.0103), ("sine997_441", -3.0075)):
        sr, st = measured[name]
        m = L.integrated(st, sr)
        print(name, m["integrated"])
        assert abs(m["integrated"] - (-3.01)) <= 0.01 and abs(m["integrated"] - expected) <= 5e-4
        assert m["passed_rel"] == m["passed_abs"] == m["blocks"] > 0
    sr, st = measured["gated"]
    m = L.integrated(st, sr)
    print("gated", m)
    assert abs(m["integrated"] - (-23.3014)) <= 5e-4
    assert 0 < m["passed_rel"] < m["passed_abs"] == m["blocks"]  # the quiet blocks fall to the relative gate


def test_known_answers_through_the_library(mxlib, measured):
    for name in ("sine997", "sine997_441"):
        sr, st = measured[name]
        assert abs(mxlib.loudness_integrated(as_lib(mxlib, st), sr)["integrated"] + 3.01) <= 0.01
    sr, st = measured["gated"]
    m = mxlib.loudness_integrated(as_lib(mxlib, st), sr)
    assert abs(m["integrated"] + 23.3014) <= 5e-4 and m["passed_rel"] < m["passed_abs"]


def _notes(mx, spans):
    return np.array([(a, b, 0, 1, 45.0, 0.0, 0.0) for a, b in spans], dtype=mx.NOTE_DTYPE)


def test_note_loudness_matches_the_reference(mxlib, measured):
    sr, st = measured["levelling"]
    rec = as_lib(mxlib, st)
    truth = L.levelling_take()[1]
    S = L.geometry(0, sr)[0]
    spans = [(a + 480, b - 481) for a, b in truth]
    spans += [(0, 10), (S - 1, S), (S, 2 * S - 1), (S + 1, 2 * S - 1), (3 * S, 3 * S), (len(st) * S - 3 * S, int(st["samples"].sum()) - 1)]
    spans.sort()
    got, ref = mxlib.note_loudness(rec, sr, _notes(mxlib, spans)), L.note_loudness(st, sr, spans)
    print(got, ref)
    assert all(_close(float(a), float(b)) for a, b in zip(got, ref))
    assert np.isneginf(got[0]) and np.isneginf(ref[0])  # silence: zero energy
    sr, st = measured["nan"]
    spans = [(0, 4799), (3 * sr, 3 * sr + 4799), (5 * sr, 5 * sr + 100)]
    got, ref = mxlib.note_loudness(as_lib(mxlib, st), sr, _notes(mxlib, spans)), L.note_loudness(st, sr, spans)
    assert math.isnan(got[1]) and math.isnan(ref[1]) and _close(got[0], ref[0]) and _close(got[2], ref[2])


def test_levelling_points_and_export_gain_are_the_references_bytes(mxlib, measured):
    """The f32 amps byte for byte: both sides call the C library's pow on the same binary64 argument."""
    sr, st = measured["levelling"]
    truth = L.levelling_take()[1]
    spans = [(a + 480, b - 481) for a, b in truth]
    notes = _notes(mxlib, spans)
    lufs = L.note_loudness(st, sr, spans)
    print("note loudness of the levelling take:", lufs)
    for params in ({}, {"raise": 0.5}, {"lower": 0.25, "max_db": 3.0}, {"raise": 0.0, "lower": 0.0}, {"max_db": 0.0}):
        got, ref_got = mxlib.level_gain_points(notes, lufs, **params)
        want, ref_want = L.level_gain_points(spans, lufs, **params)
        assert ref_got == ref_want == sorted(lufs)[2]
        assert got.tobytes() == np.array(want, dtype=mxlib.GAIN_POINT_DTYPE).tobytes(), params
        if params in ({"raise": 0.0, "lower": 0.0}, {"max_db": 0.0}):
            assert np.all(got["amp"] == 1.0)
    assert mxlib.level_gain_points(notes, lufs, raise_=0.5)[0].tobytes() == mxlib.level_gain_points(notes, lufs, **{"raise": 0.5})[0].tobytes()
    odd = lufs.copy()
    odd[1], odd[3] = -np.inf, np.nan  # not finite: A = 1, and no part in the median (now of three values)
    got, ref_got = mxlib.level_gain_points(notes, odd)
    want, ref_want = L.level_gain_points(spans, odd)
    assert ref_got == ref_want == sorted([odd[0], odd[2], odd[4]])[1]
    assert got.tobytes() == np.array(want, dtype=mxlib.GAIN_POINT_DTYPE).tobytes() and got["amp"][2] == got["amp"][6] == 1.0
    even = lufs[:4]
    assert mxlib.level_gain_points(notes[:4], even)[1] == (sorted(even)[1] + sorted(even)[2]) / 2.0 == L.level_gain_points(spans[:4], even)[1]
    none, ref_none = mxlib.level_gain_points(notes[:0], lufs[:0])
    assert len(none) == 0 and math.isnan(ref_none)
    m = L.integrated(st, sr)
    for target, ceiling in ((-23.0, -1.0), (-14.0, -1.0), (-30.0, 0.0), (0.0, -6.0)):
        amp = mxlib.normalize_gain(m, target, ceiling)
        assert np.float32(amp).tobytes() == L.normalize_gain(m, target, ceiling).tobytes(), (target, ceiling)
    assert mxlib.normalize_gain(m, 0.0, -6.0) == np.float32(10 ** (-6 / 20) / m["peak"])  # the ceiling binds


def test_refusals_leave_the_outputs_untouched(mxlib, measured):
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    sr, st = measured["levelling"]
    rec = as_lib(mxlib, st).copy()
    n = len(rec)
    p = rec.ctypes.data
    marker = 12345.678
    out = np.full(n, marker)
    k = np.full(10, marker)
    for rate in (7999, 384001, 0, -48000):
        assert lib.mx_loudness_coeffs(rate, k.ctypes.data) == INVALID and np.all(k == marker)
        assert lib.mx_loudness_curve(p, n, rate, 40, out.ctypes.data) == INVALID
    assert lib.mx_loudness_coeffs(48000, None) == INVALID
    for window in (0, -1, 6001):
        assert lib.mx_loudness_curve(p, n, sr, window, out.ctypes.data) == INVALID
    assert lib.mx_loudness_curve(None, n, sr, 40, out.ctypes.data) == INVALID and lib.mx_loudness_curve(p, -1, sr, 40, out.ctypes.data) == INVALID
    assert lib.mx_loudness_curve(p, n, sr, 40, None) == INVALID
    broken = rec.copy()
    broken["samples"][3] = 481
    assert lib.mx_loudness_curve(broken.ctypes.data, n, sr, 40, out.ctypes.data) == INVALID
    broken["samples"][3] = 0
    assert lib.mx_loudness_curve(broken.ctypes.data, n, sr, 40, out.ctypes.data) == INVALID and np.all(out == marker)
    m = mxlib._capi.Loudness(integrated=marker)
    assert lib.mx_loudness_integrated(p, n, 100, C.byref(m)) == INVALID and lib.mx_loudness_integrated(None, n, sr, C.byref(m)) == INVALID
    assert lib.mx_loudness_integrated(p, n, sr, None) == INVALID and lib.mx_loudness_integrated(broken.ctypes.data, n, sr, C.byref(m)) == INVALID
    assert m.integrated == marker and b"samples" in lib.mx_last_error()
    lufs = np.full(2, marker)
    total = int(rec["samples"].sum())
    for spans in ([(-1, 100), (200, 300)], [(0, 100), (300, 200)], [(0, 100), (total - 10, total)]):
        notes = _notes(mxlib, spans)
        assert lib.mx_note_loudness(p, n, sr, notes.ctypes.data, 2, lufs.ctypes.data) == INVALID and np.all(lufs == marker), spans
    notes = _notes(mxlib, [(0, 100), (200, 300)])
    assert lib.mx_note_loudness(p, n, sr, None, 2, lufs.ctypes.data) == INVALID and lib.mx_note_loudness(p, n, sr, notes.ctypes.data, 2, None) == INVALID
    assert lib.mx_note_loudness(p, n, 5, notes.ctypes.data, 2, lufs.ctypes.data) == INVALID and np.all(lufs == marker)
    assert lib.mx_note_loudness(p, n, sr, notes.ctypes.data, 2, lufs.ctypes.data) == 0 and not np.any(lufs == marker)
    pts = np.zeros(4, dtype=mxlib.GAIN_POINT_DTYPE)
    pts["sample"] = -7
    ref = C.c_double(marker)
    values = np.array([-20.0, -30.0])

    def points(notes, params):
        return lib.mx_level_gain_points(notes.ctypes.data, len(notes), values.ctypes.data, params, pts.ctypes.data, C.byref(ref))

    for spans in ([(200, 300), (0, 100)], [(0, 100), (100, 300)], [(0, 100), (50, 300)], [(0, 0), (200, 300)]):
        assert points(_notes(mxlib, spans), None) == INVALID, spans
    for bad in ({"raise": -0.1}, {"raise": 1.5}, {"lower": 2.0}, {"lower": math.nan}, {"max_db": -1.0}, {"max_db": 40.5}, {"max_db": math.nan}):
        assert points(notes, mxlib._params_arg("level", bad)) == INVALID, bad
    assert lib.mx_level_gain_points(None, 2, values.ctypes.data, None, pts.ctypes.data, None) == INVALID
    assert lib.mx_level_gain_points(notes.ctypes.data, 2, None, None, pts.ctypes.data, None) == INVALID
    assert lib.mx_level_gain_points(notes.ctypes.data, 2, values.ctypes.data, None, None, None) == INVALID
    assert np.all(pts["sample"] == -7) and ref.value == marker
    assert lib.mx_level_gain_points(notes.ctypes.data, 2, values.ctypes.data, None, pts.ctypes.data, None) == 0 and pts["sample"][3] == 300
    amp = C.c_float(marker)
    good = dict(integrated=-20.0, momentary_max=-18.0, shortterm_max=-19.0, peak=0.5, blocks=9, passed_abs=9, passed_rel=9, bad_blocks=0)
    for change in ({"integrated": -math.inf}, {"integrated": math.nan}, {"peak": 0.0}, {"peak": math.inf}, {"peak": math.nan}):
        m = mxlib._capi.Loudness(**dict(good, **change))
        assert lib.mx_normalize_gain(C.byref(m), -23.0, -1.0, C.byref(amp)) == INVALID, change
    m = mxlib._capi.Loudness(**good)
    assert lib.mx_normalize_gain(C.byref(m), math.nan, -1.0, C.byref(amp)) == INVALID and lib.mx_normalize_gain(C.byref(m), -23.0, math.inf, C.byref(amp)) == INVALID
    assert lib.mx_normalize_gain(None, -23.0, -1.0, C.byref(amp)) == INVALID and lib.mx_normalize_gain(C.byref(m), -23.0, -1.0, None) == INVALID
    assert amp.value == np.float32(marker)
    assert lib.mx_normalize_gain(C.byref(m), -23.0, -1.0, C.byref(amp)) == 0 and amp.value == np.float32(10 ** (-3 / 20))
    with pytest.raises(mxlib.MxError):
        mxlib.loudness_curve(rec, sr, 0)
    with pytest.raises(ValueError):
        mxlib.level_gain_points(notes, values[:1])


def test_the_level_parameter_block(mxlib):
    """As tests/test_params_host.py checks the other kinds."""
    struct, fn = mxlib._PARAMS["level"]
    p = struct()
    getattr(mxlib._capi.lib(), fn)(C.byref(p))
    d = mxlib.level_params_default()
    assert d == {"raise": 1.0, "lower": 1.0, "max_db": 12.0} == L.LEVEL_DEFAULTS and list(d) == [k for k, _ in struct._fields_]
    assert mxlib.Context.level_params_default() == d
    assert mxlib._params_arg("level", {}) is None
    assert bytes(mxlib._params_arg("level", {}, never_null=True)._obj) == bytes(p)
    assert bytes(mxlib._params_arg("level", {"raise": 1.0})._obj) == bytes(p)
    assert bytes(mxlib._params_arg("level", {"max_db": 6})._obj) == bytes(struct(1.0, 1.0, 6.0))  # (an int for a double)
    with pytest.raises(TypeError):
        mxlib._params_arg("level", {"no_such_field": 1})
    mxlib._capi.lib().mx_level_params_default(None)  # (nothing to write: nothing happens)


def test_emulation_and_host_logic_under_sanitizers(tmp_path):
    out = emu_build.run_sanitized(tmp_path, "loudness_emu", ["loudness_emu.cpp", "loudness_logic.cpp"], "LOUDNESS_EMU_MAIN")
    assert "loudness_emu ok" in out


def test_the_kernel_needs_no_scratch_and_no_lds(mxlib):
    names, scratch, vgprs, lds = emu_build.resource_usage("loudness_kernels.hip")
    print(names, scratch, vgprs, lds)
    assert len(names) == 1 and scratch == [0] and lds == [0] and vgprs[0] <= 128
