"""The dynamics compressor without a GPU (include/melonix_amd.h "Dynamics compressor"): the library's plan and curve against
tests/compress_ref.py's own binary64 formulas; the kernels' arithmetic in the kernels' lane mapping and launch geometry, run on
the CPU by tests/emu/compress_emu.cpp with every staged index checked, against the reference byte for byte — peaks, curve, f32
and int16 — at every listed length, rate and setting; the laws of the definition; the truncated warm-up against the whole
history; known answers measured by the reference; every refusal of the host side; sanitizers; the kernels' resources."""
import ctypes as C
import math

import numpy as np
import pytest

import compress_ref as R
import emu_build

SOURCES, HEADERS = ["compress_emu.cpp", "compress_logic.cpp"], ["compress_core.h", "compress_logic.h", "step_core.h", "pcm16.h"]
# the defaults; s = q (W = 16); a warm-up of several groups; K = 5; the largest K with a make-up gain
SETTINGS = {"defaults": {}, "instant": {"attack_ms": 0.0, "release_ms": 0.0}, "slow": {"attack_ms": 50.0, "release_ms": 2000.0},
            "look5": {"lookahead_ms": 5.0}, "look20": {"lookahead_ms": 20.0, "makeup_amp": 2.0}}
GROUP48 = 4096 * 48
LENGTHS = {48000: (0, 1, 47, 48, 49, GROUP48 - 1, GROUP48, GROUP48 + 1, 2 * GROUP48 + 777), 8000: (32768 + 5,), 44100: (180224 + 45,),
           384000: (1572864 + 1,)}


def load_emu(mxlib):
    """The emulation as an object: .make(params) -> what compress_ref.check_laws asks for, over the library's table and plan."""
    lib = C.CDLL(emu_build.shared_object("compress_emu", SOURCES, HEADERS))
    ll, vp = C.c_longlong, C.c_void_p
    CP = mxlib._capi.CompressParams
    P = C.POINTER(CP)
    lib.emu_compress_refuses.argtypes = [P]
    lib.emu_compress_plan.argtypes = [C.c_int, P, C.POINTER(mxlib._capi.CompressPlan)]
    lib.emu_compress_table.argtypes = [P, vp]
    lib.emu_compress_steps.argtypes, lib.emu_compress_steps.restype = [ll, C.c_int], ll
    lib.emu_compress_peaks.argtypes, lib.emu_compress_peaks.restype = [vp, ll, C.c_int, ll, ll, vp], ll
    lib.emu_compress_gain.argtypes, lib.emu_compress_gain.restype = [vp, ll, C.c_int, P, ll, ll, vp], ll
    lib.emu_compress.argtypes, lib.emu_compress.restype = [vp, ll, C.c_int, P, ll, ll, vp, vp], ll

    class Imp:
        def __init__(self, sr, p):
            self.sr, self.p = sr, p
            self.c = CP(*(p[k] for k in R.FIELDS))
            self.T, self.plan = mxlib.compress_curve(**p), mxlib.compress_plan(sr, **p)

        def run(self, x, first=0, count=None, pcm=False):
            x = np.ascontiguousarray(x, dtype=np.float32)
            count = len(x) - first if count is None else count
            out, i16 = np.zeros(count, np.float32), np.zeros(count, np.int16)
            bad = lib.emu_compress(x.ctypes.data, len(x), self.sr, C.byref(self.c), first, count, out.ctypes.data,
                                   i16.ctypes.data if pcm else None)
            assert bad == 0, bad
            return (out, i16) if pcm else out

        def gain(self, x, first_step=0, nsteps=None):
            x = np.ascontiguousarray(x, dtype=np.float32)
            nsteps = R.steps(len(x), self.sr) - first_step if nsteps is None else nsteps
            out = np.zeros(nsteps, np.int32)
            assert lib.emu_compress_gain(x.ctypes.data, len(x), self.sr, C.byref(self.c), first_step, nsteps, out.ctypes.data) == 0
            return out

        def peaks(self, x, first_step=0, nsteps=None):
            x = np.ascontiguousarray(x, dtype=np.float32)
            nsteps = R.steps(len(x), self.sr) - first_step if nsteps is None else nsteps
            out = np.zeros(nsteps, np.float32)
            assert lib.emu_compress_peaks(x.ctypes.data, len(x), self.sr, first_step, nsteps, out.ctypes.data) == 0
            return out

    class Emu:
        raw = lib

        @staticmethod
        def make(sr):
            return lambda p: Imp(sr, p)

    return Emu


@pytest.fixture(scope="module")
def emu(mxlib):
    return load_emu(mxlib)


def take_of(kind, n, sr, seed):
    return R.envelope_take(n, sr, seed) if kind == "envelope" else R.click_take(n, seed)


def test_plan_and_curve(mxlib, emu):
    """The library's curve within 1 LSB of the reference's own binary64 formula at every entry (a floor can flip under a libm
    ulp: 2^30 x a few ulp << 1), non-increasing and at least 1, at the settings and at the corners of the ranges; the plan's
    integers at five rates; the emulation's unit gives the library's."""
    corners = [dict(threshold_db=-60.0, ratio=100.0, knee_db=0.0), dict(threshold_db=-60.0, ratio=100.0, knee_db=24.0),
               dict(threshold_db=0.0, ratio=1.0, knee_db=24.0), dict(threshold_db=0.0, ratio=100.0, knee_db=0.0),
               dict(threshold_db=-33.3, ratio=2.5, knee_db=11.0)]
    for over in list(SETTINGS.values()) + corners:
        p = R.params(**over)
        T, want = mxlib.compress_curve(**p), R.curve(p)
        assert T.dtype == np.int32 and len(T) == R.CURVE == mxlib.COMPRESS_CURVE
        worst = int(np.abs(T.astype(np.int64) - want).max())
        print(over, "worst curve difference", worst, "LSB")
        assert worst <= 1
        assert np.all(np.diff(T) <= 0) and T.min() >= 1 and T[0] == R.ONE
        mine = np.zeros(R.CURVE, np.int32)
        emu.raw.emu_compress_table(C.byref(mxlib._capi.CompressParams(*(p[k] for k in R.FIELDS))), mine.ctypes.data)
        assert mine.tobytes() == T.tobytes()
    assert mxlib.compress_params_default(44100) == R.params()
    for sr, D in zip(R.RATES, (48, 44, 8, 384, 96)):
        for over in SETTINGS.values():
            p = R.params(**over)
            got, want = mxlib.compress_plan(sr, **p), R.plan(sr, p)
            assert got == want and got["D"] == D, (sr, over, got, want)
            q = mxlib._capi.CompressPlan()
            emu.raw.emu_compress_plan(sr, C.byref(mxlib._capi.CompressParams(*(p[k] for k in R.FIELDS))), C.byref(q))
            assert {k: getattr(q, k) for k, _ in q._fields_} == got
        for n in (0, 1, D - 1, D, D + 1, 2 ** 31 - 65537):
            assert mxlib.compress_steps(n, sr) == R.steps(n, sr) == emu.raw.emu_compress_steps(n, sr)
    assert mxlib.compress_plan(48000)["W"] == 1616 and mxlib.compress_plan(48000, release_ms=2000.0)["W"] == 32016
    assert mxlib.compress_plan(48000, **SETTINGS["instant"])["W"] == 16
    assert [mxlib.compress_plan(48000, lookahead_ms=v)["K"] for v in (0.0, 5.0, 20.0)] == [0, 5, 20]
    assert mxlib.compress_plan(44100, lookahead_ms=20.0)["K"] == 20 and mxlib.compress_plan(8000, lookahead_ms=0.4)["K"] == 0


def test_refusals_of_the_host_side(mxlib, emu):
    """Every field below and above its range, NaN, a make-up of 0, Inf or a subnormal; rates out of range; null pointers:
    MX_ERR_INVALID with a message, outputs untouched.  (The refusals that need a context: tests/test_gpu_compress.py.)"""
    lib, INVALID, CP = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID, mxlib._capi.CompressParams
    T, plan = np.full(R.CURVE, 7, np.int32), mxlib._capi.CompressPlan(7, 7, 7, 7, 7, 7)
    bad = []
    for k in R.FIELDS:
        lo, hi = R.RANGES[k]
        bad += [dict(R.DEFAULTS, **{k: v}) for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9)),
                                                     float("nan"))]
    bad += [dict(R.DEFAULTS, makeup_amp=v) for v in (0.0, float("inf"), 1e-40, -1.0)]
    for d in bad:
        c = CP(*(float(d[k]) for k in R.FIELDS))
        assert lib.mx_compress_curve(C.byref(c), T.ctypes.data) == INVALID and lib.mx_last_error(), d
        assert lib.mx_compress_plan_for(48000, C.byref(c), C.byref(plan)) == INVALID, d
        assert emu.raw.emu_compress_refuses(C.byref(c)) == 1, d
    for k in R.FIELDS:  # the ends of every range are legal
        for v in R.RANGES[k]:
            c = CP(*(float(dict(R.DEFAULTS, **{k: v})[f]) for f in R.FIELDS))
            assert emu.raw.emu_compress_refuses(C.byref(c)) == 0, (k, v)
    ok = CP(*(R.DEFAULTS[k] for k in R.FIELDS))
    for sr in (7999, 384001, 0, -1):
        assert lib.mx_compress_plan_for(sr, C.byref(ok), C.byref(plan)) == INVALID and lib.mx_compress_steps(100, sr) == INVALID
        assert lib.mx_compress_params_default(sr, C.byref(ok)) == INVALID
    assert lib.mx_compress_steps(-1, 48000) == INVALID
    assert lib.mx_compress_curve(C.byref(ok), None) == INVALID and lib.mx_compress_plan_for(48000, C.byref(ok), None) == INVALID
    assert lib.mx_compress_params_default(48000, None) == INVALID
    assert np.all(T == 7) and plan.D == 7 and plan.W == 7
    # null handles are refused before anything else is looked at
    f32, made = np.full(8, 7.0, np.float32), C.c_void_p(0x5A5A)
    assert lib.mx_compress(None, None, 48000, C.byref(ok), 0, 8, f32.ctypes.data, None) == INVALID
    assert lib.mx_compress_dev(None, None, 48000, C.byref(ok), 0, 8, f32.ctypes.data, None) == INVALID
    assert lib.mx_compress_gain(None, None, 48000, C.byref(ok), 0, 1, f32.ctypes.data) == INVALID
    assert lib.mx_compress_gain_dev(None, None, 48000, C.byref(ok), 0, 1, f32.ctypes.data) == INVALID
    assert lib.mx_compress_peaks_dev(None, None, 48000, 0, 1, f32.ctypes.data) == INVALID
    assert lib.mx_audio_compress(None, None, 48000, C.byref(ok), C.byref(made)) == INVALID and made.value == 0x5A5A
    assert np.all(f32 == 7.0)
    # NULL parameters are the defaults
    assert lib.mx_compress_curve(None, T.ctypes.data) == 0 and T.tobytes() == mxlib.compress_curve().tobytes()


@pytest.mark.parametrize("kind", ("envelope", "clicks"))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_emulation_is_the_reference_byte_for_byte(mxlib, emu, setting, kind):
    """Peaks, curve, f32 and int16, the table and the plan read from the library: at 48 kHz lengths 0, 1, 47 .. 49, a group of
    4096 x 48 samples and one either side, two groups and 777; 8 kHz, 44.1 kHz (D = 44) and 384 kHz."""
    p = R.params(**SETTINGS[setting])
    for sr, lengths in LENGTHS.items():
        imp = emu.make(sr)(p)
        for n in lengths:
            x = take_of(kind, n, sr, seed=n % 1000 + 1)
            pk, S, y, i16 = R.compress(x, imp.T, imp.plan, p["makeup_amp"])
            got, pcm = imp.run(x, pcm=True)
            B = R.steps(n, sr)
            assert imp.peaks(x).tobytes() == pk.tobytes(), (sr, n)
            assert imp.gain(x).tobytes() == S[:B].tobytes(), (sr, n)
            assert got.tobytes() == y.tobytes() and pcm.tobytes() == i16.tobytes(), (sr, n)
            if n > 5000:  # a range that starts and ends inside a step, past the first group's seam
                lo, hi = n // 2 - 1234, n - 7
                f, i = imp.run(x, lo, hi - lo, pcm=True)
                assert f.tobytes() == y[lo:hi].tobytes() and i.tobytes() == i16[lo:hi].tobytes(), (sr, n)
                assert imp.gain(x, B // 2 - 3, 11).tobytes() == S[B // 2 - 3:B // 2 + 8].tobytes()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_laws_on_the_cpu(emu, setting):
    R.check_laws(emu.make(48000), 48000, SETTINGS[setting])


def test_the_laws_at_44100(emu):
    R.check_laws(emu.make(44100), 44100, SETTINGS["look5"])


def test_truncated_against_untruncated_curve(mxlib):
    """The reference runs the recurrence over the whole history on envelope takes of five groups at releases of 100, 500 and
    2000 ms: the definition's truncated curve stays within 2^30 e^-16 + 2^24 / min(c) LSB of it.  MEASURED: 0 LSB at every step
    of every take."""
    sr, n = 48000, 5 * GROUP48 + 777
    for rel in (100.0, 500.0, 2000.0):
        p = R.params(release_ms=rel)
        T, pl = mxlib.compress_curve(**p), mxlib.compress_plan(sr, **p)
        for seed in (1, 2):
            pk = R.peaks(R.envelope_take(n, sr, seed), pl["D"])
            a, b = R.gains(pk, T, pl, truncated=True), R.gains(pk, T, pl, truncated=False)
            worst = int(np.abs(a - b).max())
            bound = R.ONE * math.exp(-16.0) + R.FULL / min(pl["c_att"], pl["c_rel"])
            print(f"release {rel} ms, seed {seed}: W = {pl['W']}, worst difference {worst} LSB (bound {bound:.0f}), lowest gain "
                  f"{R.reduction_db(b.min()):.1f} dB")
            assert worst <= bound


def test_known_answers(mxlib, emu):
    """Measured by the reference, never by the code under test.  DC of 0.5 at the defaults settles at (1 - 1/4)(20 log10 0.5 + 18)
    = 8.9846 dB of reduction, the margin twice the curve's interpolation error as the reference measures it over log-spaced levels
    (MEASURED: 3.4e-4 dB); a 997 Hz sine of amplitude 0.5 holds its steady reduction between -8.9841 and -8.9836 dB (MEASURED;
    asserted with the same margin around [-8.9846, -8.9836]); a step from silence to DC 0.5 reaches 1 - 1/e of its reduction in
    5 steps at the 5 ms attack, +-1."""
    sr = 48000
    p = R.params()
    imp = emu.make(sr)(p)
    T, pl = imp.T, imp.plan
    err = R.curve_error_db(T, p)
    exact = (1.0 - 1.0 / 4.0) * (20.0 * math.log10(0.5) + 18.0)
    dc = np.full(sr, 0.5, np.float32)
    t = np.arange(2 * sr) / sr
    sine = (0.5 * np.sin(2.0 * math.pi * 997.0 * t)).astype(np.float32)
    step = np.concatenate([np.zeros(4800, np.float32), np.full(sr, 0.5, np.float32)])
    for name, gain in (("reference", lambda x: R.gains(R.peaks(x, pl["D"]), T, pl)), ("emulation", imp.gain)):
        gdc = R.reduction_db(gain(dc)[-1])
        gs = R.reduction_db(gain(sine)[1000:])
        S = gain(step).astype(np.int64)
        q = int(R.targets(np.array([0.5], np.float32), T)[0])
        k = int(np.flatnonzero(R.ONE - S >= (1.0 - math.exp(-1.0)) * (R.ONE - q))[0]) - 100
        print(f"{name}: curve error {err:.2e} dB; DC {gdc:.4f} dB (exact {-exact:.4f}); sine {gs.min():.4f} .. {gs.max():.4f} dB; "
              f"attack {k} steps")
        assert err < 1e-3 and abs(gdc + exact) <= 2 * err
        assert -exact - 2 * err <= gs.min() and gs.max() <= -8.9836 + 2 * err
        assert abs(k - 5) <= 1


def test_the_chain_comes_out_louder(mxlib, emu):
    """The levelling take of DESIGN 5m scaled to peak at 1.5: the emulation's compressor at the defaults (= the reference's, by
    bytes), then tests/truepeak_ref.py's export chain on the compressed take — measure again, the gain to -12 LUFS, the limiter at
    -1 dBTP.  Without the compressor the limited take comes out at -14.30 LUFS: the limiter took what the gain gave.
    MEASURED with it: -13.22 LUFS at the defaults, 1.08 LU louder; asserted: louder than without, never above the target by more
    than the metering's 0.01."""
    import loudness_ref as L
    import truepeak_ref as T

    sr = L.LEVEL_SR
    w = L.levelling_take()[0]
    w = (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)
    p = R.params()
    imp = emu.make(sr)(p)
    y = imp.run(w)
    assert y.tobytes() == R.compress(w, imp.T, imp.plan, 1.0)[2].tobytes()
    k, taps = mxlib.loudness_coeffs(sr), mxlib.true_peak_taps()
    plain = T.export_chain(w, sr, k, taps, target_lufs=-12.0)["after"]["integrated"]
    ch = T.export_chain(y, sr, k, taps, target_lufs=-12.0)
    print(f"after the limiter: {plain:.2f} LUFS without the compressor, {ch['after']['integrated']:.2f} LUFS with it; the compressed "
          f"take measures {ch['before']['integrated']:.2f} LUFS, deepest reduction {R.reduction_db(imp.gain(w).min()):.2f} dB")
    assert abs(plain + 14.30) < 0.005, "DESIGN 5n's figure"
    assert plain < ch["after"]["integrated"] <= -12.0 + 0.01


def test_emulation_and_host_logic_under_sanitizers(tmp_path):
    assert "compress_emu ok" in emu_build.run_sanitized(tmp_path, "compress_emu", SOURCES, "COMPRESS_EMU_MAIN")


def test_the_kernels_need_no_scratch():
    """No scratch in any of the three kernels; static LDS only: the curve kernel's table of 2049 targets."""
    names, scratch, vgprs, lds = emu_build.resource_usage("compress_kernels.hip")
    print(names, scratch, vgprs, lds)
    want = ["compress_peaks_kernel", "compress_curve_kernel", "compress_apply_kernel"]
    assert len(names) == 3 and [k for k in want if any(k in n for n in names)] == want
    assert scratch == [0, 0, 0] and max(vgprs) <= 128
    assert sorted(lds) == [0, 0, 4 * R.CURVE]
