"""The PSOLA renderer on the GPU (mx_psola_synth*, mx_psola_render) against its f64 restatement tests/psola_ref.py on the
records it was actually given; what it is for — the pitch moves, the formants stay —; the shapes where the kernel can go
wrong, inside guard bands; the forms of the entry points; and the record check of the host-pointer form.

The yardstick is the project's f32-versus-f64 one (conftest.mag_tol, the phase vocoder's suite):
max |g - r| <= 2e-5 * max |r| + 1e-9 over a render, int16 within 1 LSB of the reference's conversion."""
import ctypes as C
import functools

import numpy as np
import pytest

import psola_ref
import yin_ref
from conftest import SR, mag_tol
from test_gpu_guard import Guarded, _to_device, _twice, hip  # noqa: F401  (hip: the module's HIP runtime fixture)
from test_psola_host import marker_sets, tracks

pytestmark = pytest.mark.gpu

HOP = 256
TILE = 1024  # outputs per workgroup of psola_kernels.hip
F0 = 150.0


def vowel(seconds=1.5, f0=F0, sr=SR):
    """Harmonics of f0 under resonances at 700 and 1200 Hz (the stronger one: the strongest harmonic is 1200 Hz)."""
    t = np.arange(int(seconds * sr)) / sr
    w = np.zeros(len(t))
    for k in range(1, int(0.45 * sr / f0)):
        f = k * f0
        amp = 0.05 / k + 0.6 / (1 + ((f - 700.0) / 90.0) ** 2) + 1.0 / (1 + ((f - 1200.0) / 90.0) ** 2)
        w += amp * np.sin(2 * np.pi * f * t + 0.7 * k * k)
    return (0.5 * w / np.abs(w).max()).astype(np.float32)


def noise(seconds=1.5, sr=SR):
    return np.random.default_rng(0x50534F4C).uniform(-0.3, 0.3, int(seconds * sr)).astype(np.float32)


def bend(n, st):
    return [(1, 0, 0.0, st), (n - 1, 0, 0.0, st)]


def check(g32, g16, ref, label):
    """The yardstick of the module docstring; prints the figures first."""
    err = float(np.abs(g32.astype(np.float64) - ref).max()) if len(ref) else 0.0
    tol = float(mag_tol(np.abs(ref)[None, :])[0, 0]) if len(ref) else 0.0
    lsb = int(np.abs(g16.astype(np.int32) - psola_ref.pcm16(ref).astype(np.int32)).max()) if len(ref) else 0
    print(f"psola {label}: {len(ref)} samples, max err {err:.3g} (tolerance {tol:.3g}), int16 off by at most {lsb}")
    assert err <= tol and lsb <= 1, label


def _sfx(g):
    """The record kind of g as the entry points spell it: "" for plain records, "_formant" for the formant shift's (this file's
    helpers below serve tests/test_gpu_psola_formant.py as well)."""
    return "_formant" if "step" in g.dtype.names else ""


def _synth(gpu_ctx, g):
    return getattr(gpu_ctx, "psola_synth" + _sfx(g))


def _synth_dev(gpu_ctx, g):
    return getattr(gpu_ctx, f"psola_synth{_sfx(g)}_dev")


@pytest.fixture(scope="module")
def takes(gpu_ctx):
    """name -> (samples, audio handle, f0 track): the vowel, white noise, and the two one after the other."""
    out = {}
    v, z = vowel(), noise()
    for name, w in (("vowel", v), ("noise", z), ("both", np.concatenate([v, z]))):
        a = gpu_ctx.upload(w)
        out[name] = (w, a, gpu_ctx.f0_track(a, SR, HOP))
    yield out
    for _, a, _ in out.values():
        a.free()


def _markers(n):
    return {"+4": bend(n, 4.0), "-5": bend(n, -5.0), "+12": bend(n, 12.0), "-12": bend(n, -12.0),
            "ramp, x1.5": [(1, 0, 0.0, -3.0), (n - 1, 0, 0.5 * (n - 2) / SR, 5.0)]}


@pytest.mark.parametrize("mn", ["+4", "-5", "+12", "-12", "ramp, x1.5"])
def test_parity_with_reference(gpu_ctx, mxlib, takes, mn):
    w, a, tr = takes["both"]
    g, L = mxlib.psola_plan(len(w), SR, HOP, tr, _markers(len(w))[mn])
    assert (np.unique(g["inv_half"]).size > 1) and len(g) > 300  # (voiced and unvoiced grains)
    f32, i16 = gpu_ctx.psola_synth(a, g, L)
    check(f32, i16, psola_ref.render(w, g, L), f"both, {mn}")


@pytest.mark.parametrize("name", ["vowel", "noise"])
def test_identity_without_markers(gpu_ctx, mxlib, takes, name):
    w, a, tr = takes[name]
    voiced = (tr["tau"] > 0) & (tr["aperiodicity"] < 0.15)
    assert voiced[8:-8].all() if name == "vowel" else not voiced.any()
    f32, i16 = gpu_ctx.psola_render(a, SR, HOP, tr, [])
    assert len(f32) == len(w) - 1
    check(f32, i16, w[:-1].astype(np.float64), f"identity, {name}")


def _median_note(periods):
    return float(np.median(24.0 + 12.0 * np.log2(SR / np.asarray(periods, dtype=np.float64) / 55.0)))


def _gpu_note(gpu_ctx, w):
    a = gpu_ctx.upload(w)
    try:
        tr = gpu_ctx.f0_track(a, SR, HOP)
    finally:
        a.free()
    ok = (tr["tau"] > 0) & (tr["aperiodicity"] < 0.15)
    return _median_note(tr["period"][ok])


def _ref_note(w):
    recs, _ = yin_ref.track(np.asarray(w, dtype=np.float64), SR, HOP)
    return _median_note([p for (t, p, ap, _) in recs if t > 0 and ap < 0.15])


@pytest.fixture(scope="module")
def input_notes(gpu_ctx):
    v = vowel()
    return _gpu_note(gpu_ctx, v), _ref_note(v)


@pytest.mark.parametrize("st", [4.0, -5.0])
def test_pitch_moves_by_the_bend(gpu_ctx, mxlib, takes, input_notes, st):
    """The median note of the render minus the input's: the GPU's own tracker on the GPU render against yin_ref on the
    reference render, within 1 cent (the period tolerance of tests/test_gpu_f0_decode.py)."""
    w, a, tr = takes["vowel"]
    g, L = mxlib.psola_plan(len(w), SR, HOP, tr, bend(len(w), st))
    f32, _ = gpu_ctx.psola_synth(a, g, L, want_i16=False)
    got = _gpu_note(gpu_ctx, f32) - input_notes[0]
    want = _ref_note(psola_ref.render(w, g, L)) - input_notes[1]
    print(f"psola pitch {st:+g} st: GPU render moved {got:+.5f} st, reference render {want:+.5f} st")
    assert abs(got - want) <= 0.01
    # ... and the reference itself lands on the bend: the tracker's parabolic refinement is good to about a cent on each of
    # the two takes it is asked about; 5 cents leave room for the frames at the render's tapering ends
    assert abs(want - st) <= 0.05


def _strongest_harmonic(w, lo=400.0, hi=2500.0):
    x = np.asarray(w, dtype=np.float64)[SR // 4: SR // 4 + 32768]
    mag = np.abs(np.fft.rfft(x * np.hanning(len(x))))
    f = np.fft.rfftfreq(len(x), 1.0 / SR)
    band = (f >= lo) & (f <= hi)
    return float(f[band][np.argmax(mag[band])])


def test_formants_stay(gpu_ctx, takes):
    w, a, tr = takes["vowel"]
    mk = bend(len(w), 4.0)
    f32, _ = gpu_ctx.psola_render(a, SR, HOP, tr, mk, want_i16=False)
    pv, _ = gpu_ctx.pv_render(a, SR, mk, want_i16=False)
    f_in, f_out, f_pv = _strongest_harmonic(w), _strongest_harmonic(f32), _strongest_harmonic(pv)
    print(f"strongest harmonic in 400-2500 Hz: input {f_in:.0f} Hz, PSOLA +4 st {f_out:.0f} Hz, pv_render +4 st {f_pv:.0f} Hz")
    assert abs(f_in - 1200.0) < 2.0
    assert abs(f_out - f_in) <= F0 * 2.0 ** (4.0 / 12.0)


def _hand_plan(L, H, spacing, src_off=0):
    """Grains of half-width H every `spacing` output samples over L outputs, written out by hand (no planner)."""
    s = np.arange(0.0, L + H, spacing)
    g = np.zeros(len(s), dtype=psola_ref.GRAIN_DTYPE)
    g["out_lo"] = np.maximum(0, np.floor(s - H) + 1)
    g["out_hi"] = np.minimum(L, np.ceil(s + H))
    g["centre"] = np.floor(s)
    g["centre_frac"] = s - np.floor(s)
    g["inv_half"] = 1.0 / H
    g["src_off"] = src_off
    g["src_frac"] = 0.25
    g["mark"] = np.arange(len(s))
    return g


@functools.lru_cache(maxsize=None)
def _shape_cases():
    """name -> (n, grain records, nsamples).  Where the kernel takes another path: the sizes around a tile, one sample, the
    densest and the widest grains, the two meeting, and plans that repeat or skip marks."""
    out = {}
    out["n=1, hand-made"] = (1, _hand_plan(7, 4.0, 1.5), 7)
    out["n=255, hand-made, two grains to a centre"] = (255, _hand_plan(254, 2.0, 0.5, src_off=-1), 254)
    # (the planner spaces grains by their own period over the ratio, at most 5 over a sample even where 2048 meets 27: the
    # 150 over a sample that records may ask for are written by hand)
    out["hand-made, 2048-sample windows 27 apart"] = (6000, _hand_plan(5999, 2048.0, 27.0), 5999)
    import melonix_amd as mx
    for n in (255, TILE, TILE + 1, TILE + 2, 2 * TILE + 1):  # L = n - 1
        out[f"L={n - 1}"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["blocks"], []))
    n = 4096
    out["period 2 at r = 2"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["period2"], bend(n, 12.0)))
    g, L = mx.psola_plan(n, SR, HOP, tracks(n)["period2"], [])
    g2 = np.repeat(g, 2)  # each grain twice, half a sample apart: consecutive grains share a centre
    g2["centre_frac"][1::2] = 0.5
    out["period 2, shared centres"] = (n, g2, L)
    n = 20000
    out["period 2048"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["period2048"], bend(n, -7.0)))
    out["2048 -> 27"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["abrupt"], bend(n, 12.0)))
    out["warp x4"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["voiced"], marker_sets(n, SR)["warp4"]))
    out["warp x1/4"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["voiced"], marker_sets(n, SR)["warp1/4"]))
    return out


def _run_shape(gpu_ctx, hip, w, g, L, label):  # noqa: F811
    """The device form on records g (either kind) between guard bands, twice, against the reference; and the host form on the
    same records (its record check passes them): the same bytes."""
    a = gpu_ctx.upload(w)
    d_g = _to_device(hip, g)
    try:
        def call(p):
            _synth_dev(gpu_ctx, g)(a, d_g.value, len(g), L, p[0], p[1])
        f32, i16 = _twice(hip, [L * 4, L * 2], [4 * 1, 2 * 1], call)
        f32, i16 = f32.view(np.float32), i16.view(np.int16)
        check(f32, i16, psola_ref.render(w, g, L), label)
        hf, hi16 = _synth(gpu_ctx, g)(a, g, L)
        assert hf.tobytes() == f32.tobytes() and hi16.tobytes() == i16.tobytes()
    finally:
        hip.hipFree(d_g)
        a.free()


@pytest.mark.parametrize("name", ["n=1, hand-made", "n=255, hand-made, two grains to a centre",
                                  "hand-made, 2048-sample windows 27 apart", "L=254", f"L={TILE - 1}", f"L={TILE}",
                                  f"L={TILE + 1}", f"L={2 * TILE}", "period 2 at r = 2", "period 2, shared centres", "period 2048",
                                  "2048 -> 27", "warp x4", "warp x1/4"])
def test_shapes_inside_guard_bands(gpu_ctx, hip, name):  # noqa: F811
    n, g, L = _shape_cases()[name]
    w = np.random.default_rng(n).uniform(-0.9, 0.9, n).astype(np.float32)
    if name == "hand-made, 2048-sample windows 27 apart":
        cover = np.zeros(L + 1, dtype=np.int64)
        np.add.at(cover, g["out_lo"], 1)
        np.add.at(cover, g["out_hi"], -1)
        assert np.cumsum(cover).max() >= 150  # (the widest windows at a short period's spacing: the longest walk per sample)
    _run_shape(gpu_ctx, hip, w, g, L, name)


def _device_and_empty_forms(gpu_ctx, hip, a, g, L, f32, i16):  # noqa: F811
    """The device form of records g (either kind) gives the host form's f32 / i16, with both outputs and with either alone; and
    the empty calls: no samples — nothing is touched; no grains — zeros."""
    dev, host = _synth_dev(gpu_ctx, g), _synth(gpu_ctx, g)
    d_g = _to_device(hip, g)
    try:
        def call(p):
            dev(a, d_g.value, len(g), L, p[0], p[1])
        df, di = _twice(hip, [L * 4, L * 2], [4 * 3, 2 * 3], call)
        assert df.tobytes() == f32.tobytes() and di.tobytes() == i16.tobytes()

        def call_f(p):
            dev(a, d_g.value, len(g), L, p[0], None)
        (df_only,) = _twice(hip, [L * 4], [4 * 1], call_f)
        assert df_only.tobytes() == f32.tobytes()

        def call_i(p):
            dev(a, d_g.value, len(g), L, None, p[0])
        (di_only,) = _twice(hip, [L * 2], [2 * 1], call_i)
        assert di_only.tobytes() == i16.tobytes()

        def call_0(p):
            dev(a, d_g.value, len(g), 0, p[0], p[1])
        e0 = _twice(hip, [64, 64], [4, 2], call_0)
        assert (e0[0] == 0xA5).all() and (e0[1] == 0xA5).all()

        def call_z(p):
            dev(a, None, 0, 1000, p[0], p[1])
        z = _twice(hip, [4000, 2000], [4, 2], call_z)
        assert not z[0].any() and not z[1].any()
    finally:
        hip.hipFree(d_g)
    zf, zi = host(a, g[:0], 1000)
    assert zf.shape == (1000,) and not zf.any() and not zi.any()
    ef, ei = host(a, g[:0], 0)
    assert len(ef) == 0 and len(ei) == 0


def test_forms(gpu_ctx, mxlib, hip, takes):  # noqa: F811
    w, a, tr = takes["both"]
    mk = _markers(len(w))["ramp, x1.5"]
    g, L = mxlib.psola_plan(len(w), SR, HOP, tr, mk)
    f32, i16 = gpu_ctx.psola_synth(a, g, L)
    again = gpu_ctx.psola_synth(a, g, L)
    assert again[0].tobytes() == f32.tobytes() and again[1].tobytes() == i16.tobytes()          # two runs
    only_f, none_i = gpu_ctx.psola_synth(a, g, L, want_i16=False)
    none_f, only_i = gpu_ctx.psola_synth(a, g, L, want_f32=False)
    assert none_i is None and none_f is None and only_f.tobytes() == f32.tobytes() and only_i.tobytes() == i16.tobytes()
    rf, ri = gpu_ctx.psola_render(a, SR, HOP, tr, mk)                                            # plan + synth in one call
    assert rf.tobytes() == f32.tobytes() and ri.tobytes() == i16.tobytes()
    _device_and_empty_forms(gpu_ctx, hip, a, g, L, f32, i16)

    def call_r(p):  # mx_psola_render_dev: host track and markers, device PCM
        m = mxlib._capi.markers_array(mk)
        mxlib._capi.check(mxlib._capi.lib().mx_psola_render_dev(gpu_ctx.handle, a.handle, SR, HOP, C.c_void_p(tr.ctypes.data), len(tr),
                                                                None, m, len(mk), C.c_void_p(p[0]), C.c_void_p(p[1])))
    rdf, rdi = _twice(hip, [L * 4, L * 2], [4 * 1, 2 * 1], call_r)
    assert rdf.tobytes() == f32.tobytes() and rdi.tobytes() == i16.tobytes()


def _putter(g, out):
    """put(name, field, value, at=the middle record): `out[name]` = g with that one field broken."""
    def put(name, field, value, at=len(g) // 2):
        b = g.copy()
        b[field][at] = value
        out[name] = b
    return put


def _bad_windows(g, L):
    """name -> records (either kind) with one of them broken: the 14 kinds of the record check that both kinds share."""
    k = len(g) // 2
    out = {}
    put = _putter(g, out)
    b = g.copy()
    b["centre"][k], b["centre_frac"][k] = g["centre"][k - 1], g["centre_frac"][k - 1]
    out["centre + centre_frac repeats"] = b
    b = g.copy()
    b[k - 1], b[k] = g[k], g[k - 1]
    out["centre + centre_frac falls"] = b
    put("out_lo < 0", "out_lo", -1, at=0)
    put("out_lo > out_hi", "out_lo", g["out_hi"][k] + 1)
    put("out_hi > nsamples", "out_hi", L + 1, at=len(g) - 1)
    put("window left of centre - 2049", "out_lo", g["centre"][k] - 2050)
    put("window right of centre + 2049", "out_hi", g["centre"][k] + 2051)
    put("inv_half NaN", "inv_half", np.nan)
    put("inv_half inf", "inv_half", np.inf)
    put("inv_half < 1/2048", "inv_half", np.float32(1 / 2049.0))
    put("inv_half negative", "inv_half", -0.01)
    put("centre_frac = 1", "centre_frac", 1.0)
    put("centre_frac < 0", "centre_frac", -0.25)
    put("centre_frac NaN", "centre_frac", np.nan)
    assert len(out) == 14
    return out


def _bad_records(g, L, n):
    """name -> records with one of them broken, one kind of mx_psola_synth's checks each."""
    k = len(g) // 2
    out = _bad_windows(g, L)
    put = _putter(g, out)
    put("src_frac = 1", "src_frac", 1.0)
    put("src_frac < 0", "src_frac", -0.25)
    put("src_frac NaN", "src_frac", np.nan)
    put("source left of the pad", "src_off", -int(g["out_lo"][k]) - 32768 - 1)
    put("source right of the pad", "src_off", n + 32768 - int(g["out_hi"][k]))
    return out


def _refused(gpu_ctx, lib, a, g, L, bads):
    """The host form of g's kind refuses every one of `bads` before anything is written, and counts out of range and null
    records (the device form too)."""
    host, dev = getattr(lib, "mx_psola_synth" + _sfx(g)), getattr(lib, f"mx_psola_synth{_sfx(g)}_dev")
    for name, b in bads.items():
        f32 = np.full(L, 7.0, dtype=np.float32)
        i16 = np.full(L, 77, dtype=np.int16)
        rc = host(gpu_ctx.handle, a.handle, C.c_void_p(b.ctypes.data), len(b), L, C.c_void_p(f32.ctypes.data), C.c_void_p(i16.ctypes.data))
        assert rc == -1 and b"grain" in lib.mx_last_error(), (name, rc, lib.mx_last_error())
        assert (f32 == 7.0).all() and (i16 == 77).all(), name
    gp = C.c_void_p(g.ctypes.data)
    assert host(gpu_ctx.handle, a.handle, gp, -1, L, None, None) == -1
    assert host(gpu_ctx.handle, a.handle, gp, len(g), -1, None, None) == -1
    assert host(gpu_ctx.handle, a.handle, gp, len(g), 2 ** 31, None, None) == -1
    assert host(gpu_ctx.handle, a.handle, None, len(g), L, None, None) == -1
    assert dev(gpu_ctx.handle, a.handle, None, len(g), L, None, None) == -1


def test_bad_records_are_refused_by_the_host_form(gpu_ctx, mxlib, takes):
    w, a, tr = takes["vowel"]
    g, L = mxlib.psola_plan(len(w), SR, HOP, tr, bend(len(w), 4.0))
    bads = _bad_records(g, L, len(w))
    assert len(bads) == 19
    _refused(gpu_ctx, mxlib._capi.lib(), a, g, L, bads)
    # ... and a track that does not fit the file, through the one-call form
    with pytest.raises(mxlib.MxError) as e:
        gpu_ctx.psola_render(a, SR, HOP, tr[:-1], [])
    assert e.value.code == -1
    # the good records still render
    f32, _ = gpu_ctx.psola_synth(a, g, L, want_i16=False)
    assert np.isfinite(f32).all() and np.abs(f32).max() > 0.1
