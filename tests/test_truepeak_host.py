"""True peak, limiter and loudness range without a GPU (include/melonix_amd.h "True peak, limiter and loudness range"): the tap
table against its formula; the kernels' per-sample arithmetic (csrc/truepeak_core.h) run on the CPU by tests/emu/truepeak_emu.cpp
against tests/truepeak_ref.py, byte for byte; known answers of the meter and of the loudness range, measured by the reference;
the library's host logic against the reference; the refusals; sanitizers; the kernels' resources."""
import ctypes as C
import math

import numpy as np
import pytest

import emu_build
import loudness_ref as L
import truepeak_ref as T

RATES = (48000, 44100, 8000, 96000, 192000)


@pytest.fixture(scope="module")
def taps(mxlib):
    t = mxlib.true_peak_taps()
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def emu(mxlib):
    lib = C.CDLL(emu_build.shared_object("truepeak_emu", ["truepeak_emu.cpp"], ["truepeak_core.h", "step_core.h", "pcm16.h"]))
    lib.emu_true_peak_steps.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_long, C.c_void_p]
    lib.emu_limit.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]

    class Emu:
        @staticmethod
        def records(w, sr, first_step=0, nsteps=None):
            w = np.ascontiguousarray(w, dtype=np.float32)
            steps = -(-len(w) // T.step_samples(sr))
            nsteps = steps - first_step if nsteps is None else nsteps
            out = np.zeros(nsteps, dtype=T.STEP_DTYPE)
            lib.emu_true_peak_steps(w.ctypes.data, len(w), sr, first_step, nsteps, out.ctypes.data)
            return out

        @staticmethod
        def limit(w, sr, c, A):
            w = np.ascontiguousarray(w, dtype=np.float32)
            out, pcm = np.zeros(len(w), np.float32), np.zeros(len(w), np.int16)
            lib.emu_limit(w.ctypes.data, len(w), sr, np.float32(c), A, out.ctypes.data, pcm.ctypes.data)
            return out, pcm

    return Emu


def test_the_tap_table_is_the_formula(mxlib, taps):
    """To within 1 ulp of binary32; offset 3/4 is offset 1/4 reversed; every row sums to 1 within 3e-4 (the window's price)."""
    want = T.tap_formula()
    assert taps.shape == (3, 12) and taps.dtype == np.float32
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(taps.astype(np.float64) - want)
    print("largest error in ulps:", float((err / ulp).max()), "row sums - 1:", taps.astype(np.float64).sum(axis=1) - 1.0)
    assert np.all(err <= ulp)
    assert taps[2].tobytes() == taps[0][::-1].tobytes() and taps[1].tobytes() == taps[1][::-1].tobytes()
    assert np.all(np.abs(taps.astype(np.float64).sum(axis=1) - 1.0) <= 3e-4)


def test_geometry_and_defaults(mxlib):
    for sr, L_ in ((8000, 4), (44100, 4), (48000, 4), (88199, 4), (88200, 2), (96000, 2), (176399, 2), (176400, 1), (192000, 1), (384000, 1)):
        assert mxlib.true_peak_oversampling(sr) == L_ == T.oversampling(sr), sr
    assert mxlib.true_peak_oversampling(7999) == 0 and mxlib.true_peak_oversampling(384001) == 0
    for sr in RATES + (384000, 11025):
        d = mxlib.limit_params_default(sr)
        assert d == {"ceiling_amp": float(T.MINUS_1_DBTP), "lookahead": T.default_lookahead(sr)} and list(d) == ["ceiling_amp", "lookahead"]
    assert mxlib.limit_params_default(48000)["lookahead"] == 240 and mxlib.limit_params_default(384000)["lookahead"] == 1024


@pytest.mark.parametrize("sr", RATES)
def test_the_kernels_arithmetic_on_the_cpu(taps, emu, sr):
    """truepeak_core.h, sample by sample, gives the reference's bytes: records (whole and split) and the limiter, on noise with
    clicks at both ends, a length that ends in a partial step."""
    S = T.step_samples(sr)
    n = 5 * S + S // 2 + 3
    w = T.sparse_clicks(n, seed=sr)
    w[0], w[n - 1], w[2 * S] = 1.7, -1.2, 0.95
    ref = T.records(w, sr, taps)
    got = emu.records(w, sr)
    assert len(ref) == 6 and got.tobytes() == ref.tobytes()
    assert np.all(ref["true_peak"] >= ref["sample_peak"]) and ref["sample_peak"][0] == np.float32(1.7)
    assert emu.records(w, sr, 2, 3).tobytes() == ref[2:5].tobytes() == T.records(w, sr, taps, 2, 3).tobytes()
    if T.oversampling(sr) == 1:
        assert ref["true_peak"].tobytes() == ref["sample_peak"].tobytes()
    else:
        assert np.any(ref["true_peak"] > ref["sample_peak"])
    for A in (1, 2, 65, T.default_lookahead(sr)):
        out, pcm = T.limit(w, sr, taps, T.MINUS_1_DBTP, A)
        eo, ep = emu.limit(w, sr, T.MINUS_1_DBTP, A)
        assert eo.tobytes() == out.tobytes() and ep.tobytes() == pcm.tobytes(), A
        assert np.abs(out).max() <= T.MINUS_1_DBTP and out.tobytes() != w.tobytes()


@pytest.mark.parametrize("n", [1, 5, 6, 7, 479, 480, 481])
def test_smallest_lengths_on_the_cpu(taps, emu, n):
    sr = 48000
    w = T.clicks(n, seed=n)
    assert emu.records(w, sr).tobytes() == T.records(w, sr, taps).tobytes()
    for A in (1, 64, 1024):
        out, pcm = T.limit(w, sr, taps, np.float32(0.5), A)
        eo, ep = emu.limit(w, sr, np.float32(0.5), A)
        assert eo.tobytes() == out.tobytes() and ep.tobytes() == pcm.tobytes(), A


def test_the_laws_on_the_cpu(taps, emu):
    """Laws 1-4 of the definition on the reference and the emulation (the GPU tests repeat them on the device)."""
    sr, n, A, c = 48000, 4801, 64, T.MINUS_1_DBTP
    for name, make in T.SIGNALS.items():
        w = make(n)
        out, _ = T.limit(w, sr, taps, c, A)
        assert np.abs(out).max() <= c, name                                        # 1
        over = np.flatnonzero(T.peaks(w, sr, taps) > c)
        near = np.zeros(n, dtype=bool)
        for j in over:
            near[max(j - A, 0):j + A + 1] = True
        assert out[~near].tobytes() == w[~near].tobytes() and near.any() and (near.all() == (name in ("tone", "noise"))), name   # 2
        for k in (-7, -20):                                                        # 3
            f = np.float32(2.0 ** k)
            scaled, _ = emu.limit(w * f, sr, c * f, A)
            assert scaled.tobytes() == (out * f).tobytes(), (name, k)
            assert emu.records(w * f, sr).tobytes() == np.frombuffer((T.records(w, sr, taps).view(np.float32) * f).tobytes(), dtype=T.STEP_DTYPE).tobytes()
    for w in (np.zeros(1000, np.float32), np.full(1000, -0.0, np.float32)):       # 4
        for rec in (T.records(w, sr, taps), emu.records(w, sr)):
            assert rec.tobytes() == np.zeros(len(rec), dtype=T.STEP_DTYPE).tobytes()
        for out in (T.limit(w, sr, taps, c, A)[0], emu.limit(w, sr, c, A)[0]):
            assert out.tobytes() == w.tobytes()


def sine(sr, hz, amp, degrees, n=4800):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(n) / sr + math.radians(degrees))).astype(np.float32)


@pytest.mark.parametrize("div,degrees", [(4, 0.0), (4, 45.0), (6, 60.0), (8, 67.5)])
def test_known_answers_of_the_meter(taps, emu, div, degrees):
    """Sines of amplitude 0.5 at 48 kHz read -6.0 dBTP within +0.2 / -0.4 dB (the tolerance EBU Tech 3341 gives its true-peak
    cases); fs/4 at 45 degrees has a sample peak of -9.03 dBFS beside it.  Measured by the reference, the same bytes from the
    emulation.  (tests/truepeak_ref.py alone, on the CPU: amplitude 1 at fs/4, 45 degrees reads -0.002 dBTP; the worst
    under-read over 60 log-spaced sines from 100 Hz to 20 kHz at three phases is -0.161 dB, the scalloping of 4x: the next test.)"""
    sr = 48000
    w = sine(sr, sr / div, 0.5, degrees)
    rec = T.records(w, sr, taps)
    assert emu.records(w, sr).tobytes() == rec.tobytes()
    tp, sp = T.measure(rec[1:-1])  # (steady state: without the steps that hold the ends of the tone)
    print(f"fs/{div} at {degrees} degrees: {T.dbtp(tp):.4f} dBTP, sample peak {T.dbtp(sp):.4f} dBFS")
    assert -0.4 <= T.dbtp(tp) - (-6.0) <= 0.2
    if (div, degrees) == (4, 45.0):
        assert abs(T.dbtp(sp) - (-9.03)) <= 0.01
    full = np.float32(2.0) * w
    assert (div, degrees) != (4, 45.0) or abs(T.dbtp(T.measure(T.records(full, sr, taps)[1:-1])[0]) - (-0.002)) <= 0.002


def test_scalloping_of_the_meter(taps):
    """The worst under-read over sines from 100 Hz to 20 kHz at 48 kHz stays inside Tech 3341's -0.4 dB."""
    sr, worst = 48000, 0.0
    for hz in np.geomspace(100.0, 20000.0, 60):
        for degrees in (0.0, 33.0, 71.0):
            tp = T.measure(T.records(sine(sr, hz, 0.5, degrees, 2400), sr, taps)[1:-1])[0]
            worst = min(worst, T.dbtp(tp) - 20.0 * math.log10(0.5))
    print(f"worst under-read {worst:.3f} dB")
    assert -0.4 <= worst <= 0.0


def as_lib(mx, st):
    return np.frombuffer(st.tobytes(), dtype=mx.LOUD_STEP_DTYPE)


@pytest.mark.parametrize("first,second,expected", [(-20.0, -30.0, 10.0), (-20.0, -15.0, 5.0), (-40.0, -20.0, 20.0)])
def test_loudness_range_known_answers(mxlib, first, second, expected):
    """EBU Tech 3342's first three cases (1 kHz, 20 s + 20 s) and its tolerance of 1 LU; the records are the reference's, and the
    library's result equals the reference's field for field (log10 may differ by an ulp: 1e-9)."""
    sr = 48000
    w = np.concatenate([L.tone(sr, 1000.0, L.dbfs(first), 20.0), L.tone(sr, 1000.0, L.dbfs(second), 20.0)])
    st = L.steps(w, sr, mxlib.loudness_coeffs(sr))
    ref, got = T.loudness_range(st, sr), mxlib.loudness_range(as_lib(mxlib, st), sr)
    print(ref, got)
    assert abs(ref["lra"] - expected) <= 1.0 and abs(got["lra"] - expected) <= 1.0
    assert ref["values"] == got["values"] == (len(st) - 300) // 10 + 1 and ref["gated"] == got["gated"] > 0 and ref["bad"] == got["bad"] == 0
    for key in ("lra", "low_lufs", "high_lufs"):
        assert abs(got[key] - ref[key]) <= 1e-9, key


def test_loudness_range_edges(mxlib):
    """Shorter than one window, silence (nothing passes the absolute gate), a NaN energy, a partial last step."""
    sr, S = 48000, 480
    k = mxlib.loudness_coeffs(sr)
    short = L.steps(L.tone(sr, 1000.0, 0.1, 2.5), sr, k)
    silent = L.steps(np.zeros(4 * sr, np.float32), sr, k)
    take = L.tone(sr, 1000.0, 0.1, 4.0)[:4 * sr - 7].copy()
    bad = take.copy()
    bad[100] = np.nan
    for st, values, gated, nbad in ((short, 0, 0, 0), (silent, 11, 0, 0), (L.steps(take, sr, k), 10, 10, 0), (L.steps(bad, sr, k), 10, 9, 1)):
        ref, got = T.loudness_range(st, sr), mxlib.loudness_range(as_lib(mxlib, st), sr)
        assert (ref["values"], ref["gated"], ref["bad"]) == (got["values"], got["gated"], got["bad"]) == (values, gated, nbad)
        assert got["lra"] == ref["lra"] or abs(got["lra"] - ref["lra"]) <= 1e-9
        if gated == 0:
            assert got["lra"] == 0.0 and got["low_lufs"] == got["high_lufs"] == -math.inf


def test_normalize_gain_tp_is_the_references_bytes_and_refuses(mxlib):
    m = dict(integrated=-20.0, momentary_max=-18.0, shortterm_max=-19.0, peak=0.5, blocks=9, passed_abs=9, passed_rel=9, bad_blocks=0)
    for tp, target, ceiling in ((0.7, -23.0, -1.0), (0.7, -14.0, -1.0), (1.5, -16.0, -1.0), (0.25, -30.0, 0.0), (0.9, 0.0, -6.0)):
        assert np.float32(mxlib.normalize_gain_tp(m, tp, target, ceiling)).tobytes() == T.normalize_gain_tp(m, tp, target, ceiling).tobytes()
    assert mxlib.normalize_gain_tp(m, 0.9, 0.0, -6.0) == np.float32(10 ** (-6 / 20) / float(np.float32(0.9)))  # the ceiling binds
    assert mxlib.normalize_gain_tp(m, 0.5, -23.0, -1.0) == mxlib.normalize_gain(m, -23.0, -1.0)  # (the sample peak as the true peak)
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    marker = 12345.678
    amp = C.c_float(marker)
    good = mxlib._capi.Loudness(**m)
    for change in ({"integrated": -math.inf}, {"integrated": math.nan}):
        assert lib.mx_normalize_gain_tp(C.byref(mxlib._capi.Loudness(**dict(m, **change))), 0.7, -23.0, -1.0, C.byref(amp)) == INVALID, change
    for tp in (0.0, -0.5, math.inf, math.nan):
        assert lib.mx_normalize_gain_tp(C.byref(good), tp, -23.0, -1.0, C.byref(amp)) == INVALID, tp
    assert lib.mx_normalize_gain_tp(C.byref(good), 0.7, math.nan, -1.0, C.byref(amp)) == INVALID
    assert lib.mx_normalize_gain_tp(C.byref(good), 0.7, -23.0, math.inf, C.byref(amp)) == INVALID
    assert lib.mx_normalize_gain_tp(None, 0.7, -23.0, -1.0, C.byref(amp)) == INVALID and lib.mx_normalize_gain_tp(C.byref(good), 0.7, -23.0, -1.0, None) == INVALID
    assert amp.value == np.float32(marker)
    assert lib.mx_normalize_gain_tp(C.byref(good), 0.7, -23.0, -1.0, C.byref(amp)) == 0 and amp.value == np.float32(10 ** (-3 / 20))


def test_host_refusals_leave_the_outputs_untouched(mxlib):
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    assert lib.mx_true_peak_taps(None) == INVALID
    p = mxlib._capi.LimitParams(7.0, 7)
    for rate in (7999, 384001, 0, -48000):
        assert lib.mx_limit_params_default(rate, C.byref(p)) == INVALID
    assert lib.mx_limit_params_default(48000, None) == INVALID and (p.ceiling_amp, p.lookahead) == (7.0, 7)
    st = np.zeros(400, dtype=mxlib.LOUD_STEP_DTYPE)
    st["samples"] = 480
    r = mxlib._capi.LoudnessRange(lra=7.0)
    for rate in (7999, 384001):
        assert lib.mx_loudness_range(st.ctypes.data, len(st), rate, C.byref(r)) == INVALID
    assert lib.mx_loudness_range(None, len(st), 48000, C.byref(r)) == INVALID and lib.mx_loudness_range(st.ctypes.data, -1, 48000, C.byref(r)) == INVALID
    assert lib.mx_loudness_range(st.ctypes.data, len(st), 48000, None) == INVALID
    st["samples"][7] = 481
    assert lib.mx_loudness_range(st.ctypes.data, len(st), 48000, C.byref(r)) == INVALID and r.lra == 7.0
    st["samples"][7] = 480
    assert lib.mx_loudness_range(st.ctypes.data, len(st), 48000, C.byref(r)) == 0 and r.lra == 0.0 and r.values == 11
    with pytest.raises(mxlib.MxError):
        mxlib.limit_params_default(7999)


def test_emulation_and_host_logic_under_sanitizers(tmp_path):
    out = emu_build.run_sanitized(tmp_path, "truepeak_emu", ["truepeak_emu.cpp", "loudness_logic.cpp"], "TRUEPEAK_EMU_MAIN")
    assert "truepeak_emu ok" in out


def test_the_kernels_need_no_scratch_and_the_limiter_fits_its_lds(mxlib):
    names, scratch, vgprs, lds = emu_build.resource_usage("truepeak_kernels.hip")
    print(names, scratch, vgprs, lds)
    assert len(names) == 2 and scratch == [0, 0] and max(vgprs) <= 128
    assert "truepeak_steps_kernel" in names[0] and "limit_kernel" in names[1] and 0 < lds[1] <= 65536 and 0 < lds[0] <= 65536
