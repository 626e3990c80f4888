"""The formant shift of the PSOLA renderer on the GPU (mx_psola_synth_formant*, mx_psola_render_formant*) against its f64
restatement tests/psola_formant_ref.py on the records it was actually given; byte identity with the plain kernel where the
two read the same samples; delegation without points; the forms of the entry points; the shapes where the kernel can go wrong,
inside guard bands; what it is for — the envelope moves, the note does what the bend says —; and the record check of the
host-pointer form.

The yardstick is test_gpu_psola.py's (conftest.mag_tol): max |g - r| <= 2e-5 * max |r| + 1e-9 over a render, int16 within 1 LSB.
It holds here as there because the source positions are exact integers on both sides: only the interpolation and the two sums
are binary32 on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import psola_formant_ref as FR
from conftest import SR
from test_gpu_guard import _twice, hip  # noqa: F401  (hip: the module's HIP runtime fixture)
from test_gpu_psola import (HOP, TILE, _bad_windows, _device_and_empty_forms, _gpu_note, _hand_plan, _markers, _putter,  # noqa: F401
                            _ref_note, _refused, _run_shape, _strongest_harmonic, bend, check, input_notes, takes)
from test_psola_host import tracks

pytestmark = pytest.mark.gpu

PAD = 32768
LO, ONE, HI = 32768, 65536, 131072


def const(st):
    return [(0, st)]


@pytest.mark.parametrize("name", ["bend 0, formant +4", "bend 0, formant -3", "bend +4, formant -3", "bend -5, formant +5",
                                  "ramp x1.5, formant -5 -> +5"])
def test_parity_with_reference(gpu_ctx, mxlib, takes, name):  # noqa: F811
    w, a, tr = takes["both"]
    n = len(w)
    mk, pts = {"bend 0, formant +4": ([], const(4.0)), "bend 0, formant -3": ([], const(-3.0)),
               "bend +4, formant -3": (bend(n, 4.0), const(-3.0)), "bend -5, formant +5": (bend(n, -5.0), const(5.0)),
               "ramp x1.5, formant -5 -> +5": (_markers(n)["ramp, x1.5"], [(0, -5.0), (n - 1, 5.0)])}[name]
    fg, L = mxlib.psola_plan_formant(n, SR, HOP, tr, mk, pts)
    assert np.unique(fg["inv_half"]).size > 1 and len(fg) > 300  # (voiced and unvoiced grains)
    assert np.unique(fg["step"]).size > 100 if "->" in name else (fg["step"] == FR.step_of(pts[0][1])).all()
    f32, i16 = gpu_ctx.psola_synth_formant(a, fg, L)
    check(f32, i16, FR.render_formant(w, fg, L), f"formant, both, {name}")


def _plain_cases():
    """name -> (n, plain records with src_frac == 0, nsamples)."""
    import melonix_amd as mx
    out = {}
    for name, (n, g, L) in {"H 4, 1.5 apart": (255, _hand_plan(254, 4.0, 1.5, src_off=3), 254),
                            "H 2048, 27 apart": (6000, _hand_plan(5999, 2048.0, 27.0, src_off=-1), 5999),
                            "H 2, half a sample apart": (255, _hand_plan(254, 2.0, 0.5, src_off=-1), 254)}.items():
        g["src_frac"] = 0.0
        out[name] = (n, g, L)
    n = 20000
    out["planned, no markers"] = (n, *mx.psola_plan(n, SR, HOP, tracks(n)["blocks"], []))
    return out


@pytest.mark.parametrize("name", ["H 4, 1.5 apart", "H 2048, 27 apart", "H 2, half a sample apart", "planned, no markers"])
def test_step_one_records_give_the_plain_kernels_bytes(gpu_ctx, name):
    n, g, L = _plain_cases()[name]
    w = np.random.default_rng(n).uniform(-0.9, 0.9, n).astype(np.float32)
    a = gpu_ctx.upload(w)
    try:
        pf, pi = gpu_ctx.psola_synth(a, g, L)
        ff, fi = gpu_ctx.psola_synth_formant(a, FR.twin(g), L)
    finally:
        a.free()
    assert np.abs(pf).max() > 0.1
    assert ff.tobytes() == pf.tobytes() and fi.tobytes() == pi.tobytes()


def test_no_points_is_the_plain_render(gpu_ctx, mxlib, hip, takes):  # noqa: F811
    w, a, tr = takes["both"]
    mk = _markers(len(w))["ramp, x1.5"]
    pf, pi = gpu_ctx.psola_render(a, SR, HOP, tr, mk)
    ff, fi = gpu_ctx.psola_render_formant(a, SR, HOP, tr, mk, [])
    assert ff.tobytes() == pf.tobytes() and fi.tobytes() == pi.tobytes() and np.abs(pf).max() > 0.1
    L = len(pf)

    def call(p):  # the device form: host track and markers, device PCM
        m = mxlib._capi.markers_array(mk)
        mxlib._capi.check(mxlib._capi.lib().mx_psola_render_formant_dev(
            gpu_ctx.handle, a.handle, SR, HOP, C.c_void_p(tr.ctypes.data), len(tr), None, m, len(mk), None, 0, C.c_void_p(p[0]),
            C.c_void_p(p[1])))
    df, di = _twice(hip, [L * 4, L * 2], [4 * 1, 2 * 1], call)
    assert df.tobytes() == pf.tobytes() and di.tobytes() == pi.tobytes()


def test_forms(gpu_ctx, mxlib, hip, takes):  # noqa: F811
    w, a, tr = takes["both"]
    n = len(w)
    mk, pts = _markers(n)["ramp, x1.5"], [(0, -5.0), (n // 2, 2.0), (n - 1, 5.0)]
    fg, L = mxlib.psola_plan_formant(n, SR, HOP, tr, mk, pts)
    f32, i16 = gpu_ctx.psola_synth_formant(a, fg, L)
    again = gpu_ctx.psola_synth_formant(a, fg, L)
    assert again[0].tobytes() == f32.tobytes() and again[1].tobytes() == i16.tobytes()           # two runs
    only_f, none_i = gpu_ctx.psola_synth_formant(a, fg, L, want_i16=False)
    none_f, only_i = gpu_ctx.psola_synth_formant(a, fg, L, want_f32=False)
    assert none_i is None and none_f is None and only_f.tobytes() == f32.tobytes() and only_i.tobytes() == i16.tobytes()
    rf, ri = gpu_ctx.psola_render_formant(a, SR, HOP, tr, mk, pts)                                # plan + synth in one call
    assert rf.tobytes() == f32.tobytes() and ri.tobytes() == i16.tobytes()
    _device_and_empty_forms(gpu_ctx, hip, a, fg, L, f32, i16)

    def call_r(p):  # mx_psola_render_formant_dev
        m = mxlib._capi.markers_array(mk)
        pa = mxlib._formant_points(pts)
        mxlib._capi.check(mxlib._capi.lib().mx_psola_render_formant_dev(
            gpu_ctx.handle, a.handle, SR, HOP, C.c_void_p(tr.ctypes.data), len(tr), None, m, len(mk), C.c_void_p(pa.ctypes.data),
            len(pa), C.c_void_p(p[0]), C.c_void_p(p[1])))
    rdf, rdi = _twice(hip, [L * 4, L * 2], [4 * 1, 2 * 1], call_r)
    assert rdf.tobytes() == f32.tobytes() and rdi.tobytes() == i16.tobytes()
    # every record 1023 outputs later: the same samples 1023 outputs later, whatever tile they fall into
    sh = fg.copy()
    for f in ("out_lo", "out_hi", "centre"):
        sh[f] += 1023
    sf, si = gpu_ctx.psola_synth_formant(a, sh, L + 1023)
    assert not sf[:1023].any() and not si[:1023].any()
    assert sf[1023:].tobytes() == f32.tobytes() and si[1023:].tobytes() == i16.tobytes()


def _hand_fplan(L, H, spacing, step, src_q=0, src_shift=0):
    """Formant records of half-width H every `spacing` outputs over L outputs, by hand: grain k reads the source around its
    own centre + src_shift at `step` (a scalar, or one value per grain)."""
    g = _hand_plan(L, H, spacing)
    g["src_frac"] = 0.0
    out = FR.twin(g)
    out["src_idx"] = g["centre"] + src_shift
    out["src_q"] = src_q
    out["step"] = step if np.isscalar(step) else np.resize(np.asarray(step, dtype=np.uint32), len(out))
    return out


@functools.lru_cache(maxsize=None)
def _shape_cases():
    """name -> (n, formant records, nsamples): the smallest shapes at which the kernel can go wrong."""
    import melonix_amd as mx
    out = {}
    for step in (LO, HI):
        out[f"n=1, step {step}"] = (1, _hand_fplan(7, 4.0, 1.5, step), 7)
        out[f"n=255, step {step}"] = (255, _hand_fplan(254, 2.0, 0.5, step, src_q=40000, src_shift=-1), 254)
        n = 4096  # half-width 2, planned: a period of 2 at the limit of the curve
        out[f"half-width 2, step {step}"] = (n, *mx.psola_plan_formant(n, SR, HOP, tracks(n)["period2"], bend(n, 12.0),
                                                                        const(12.0 if step == HI else -12.0)))
    for n in (TILE, TILE + 1, TILE + 2, 2 * TILE + 1):  # L = n - 1
        out[f"L={n - 1}"] = (n, *mx.psola_plan_formant(n, SR, HOP, tracks(n)["blocks"], [], [(0, -7.0), (n - 1, 9.0)]))
    # the widest windows at twice the speed, the first grains on source sample 0 and the last on the file's last: the reads run
    # 4094 samples into the zeros before the file and 4097 behind it (a file shorter than one window)
    n, L = 3000, 9000
    g = _hand_fplan(L, 2048.0, 700.0, HI, src_q=65535)
    g = g[g["out_lo"] < g["out_hi"]]
    g["centre_frac"] = 0.5
    g["out_lo"], g["out_hi"] = np.maximum(0, g["centre"] - 2047), np.minimum(L, g["centre"] + 2049)
    assert len(g) == 16  # (centres 0, 700 .. 10500: grains 3 .. 9 have their whole window inside the outputs)
    g["src_idx"] = np.round(np.interp(np.arange(16), [4, 8], [0, n - 1])).astype(np.int32)
    lo = g["src_idx"].astype(np.int64) + ((65535 + HI * (g["out_lo"].astype(np.int64) - g["centre"])) >> 16)
    hi = g["src_idx"].astype(np.int64) + ((65535 + HI * (g["out_hi"].astype(np.int64) - 1 - g["centre"])) >> 16) + 1
    assert lo.min() == -4094 and hi.max() == n - 1 + 4097
    out["half-width 2048 at step 131072, into both pads"] = (n, g, L)
    out["src_q = 65535"] = (4096, _hand_fplan(4095, 100.0, 37.5, [LO, 70001, ONE, 99999, HI], src_q=65535, src_shift=5), 4095)
    g = _hand_fplan(5999, 2048.0, 27.0, np.arange(LO, HI, 431), src_q=12345)
    cover = np.zeros(6000, dtype=np.int64)
    np.add.at(cover, g["out_lo"], 1)
    np.add.at(cover, g["out_hi"], -1)
    assert np.cumsum(cover).max() >= 150
    out["150 grains over a sample"] = (6000, g, 5999)
    n = 20000
    g, L = mx.psola_plan_formant(n, SR, HOP, tracks(n)["wander"], [], [(0, -12.0), (n, 12.0)])  # (no markers: a mark per grain)
    assert len(g) > 50 and (np.diff(g["step"].astype(np.int64))[g["centre"][1:] < n] > 0).all()
    out["a new step in every grain"] = (n, g, L)
    return out


@pytest.mark.parametrize("name", [f"n=1, step {LO}", f"n=1, step {HI}", f"n=255, step {LO}", f"n=255, step {HI}",
                                  f"half-width 2, step {LO}", f"half-width 2, step {HI}", f"L={TILE - 1}", f"L={TILE}", f"L={TILE + 1}",
                                  f"L={2 * TILE}", "half-width 2048 at step 131072, into both pads", "src_q = 65535",
                                  "150 grains over a sample", "a new step in every grain"])
def test_shapes_inside_guard_bands(gpu_ctx, hip, name):  # noqa: F811
    n, g, L = _shape_cases()[name]
    w = np.random.default_rng(n).uniform(-0.9, 0.9, n).astype(np.float32)
    _run_shape(gpu_ctx, hip, w, g, L, f"formant, {name}")


@pytest.mark.parametrize("st,formant", [(0.0, 4.0), (0.0, -3.0), (4.0, 4.0)])
def test_envelope_moves_and_pitch_follows_the_bend(gpu_ctx, mxlib, takes, input_notes, st, formant):  # noqa: F811
    """The GPU render against the reference render of the same records: the strongest harmonic in 400-2500 Hz within 2 Hz (one
    and a half bins of _strongest_harmonic's 32768-point transform), the median note's move — the GPU's tracker on the GPU
    render, yin_ref on the reference render — within a cent."""
    w, a, tr = takes["vowel"]
    n = len(w)
    fg, L = mxlib.psola_plan_formant(n, SR, HOP, tr, bend(n, st) if st else [], const(formant))
    f32, _ = gpu_ctx.psola_synth_formant(a, fg, L, want_i16=False)
    ref = FR.render_formant(w, fg, L)
    f_gpu, f_ref = _strongest_harmonic(f32), _strongest_harmonic(ref)
    got = _gpu_note(gpu_ctx, f32) - input_notes[0]
    want = _ref_note(ref) - input_notes[1]
    print(f"formant {formant:+g} st, bend {st:+g} st: strongest harmonic GPU {f_gpu:.1f} Hz, reference {f_ref:.1f} Hz (1200 Hz moved by "
          f"the formant: {1200 * 2 ** (formant / 12):.0f}); median note moved {got:+.5f} st on the GPU, {want:+.5f} st in the reference")
    assert abs(f_gpu - f_ref) <= 2.0
    assert abs(got - want) <= 0.01


def _bad_records(g, L, n):
    """name -> records with one of them broken, one kind of mx_psola_synth_formant's checks each."""
    k = len(g) // 2
    out = {}
    put = _putter(g, out)
    put("step 32767", "step", 32767)
    put("step 131073", "step", 131073)
    put("step 0", "step", 0)
    put("src_q 65536", "src_q", 65536)
    # the first source index left of the pad by one, the last (+ 1) right of it by one
    lo_off = (int(g["src_q"][k]) + int(g["step"][k]) * (int(g["out_lo"][k]) - int(g["centre"][k]))) >> 16
    hi_off = (int(g["src_q"][k]) + int(g["step"][k]) * (int(g["out_hi"][k]) - 1 - int(g["centre"][k]))) >> 16
    put("source left of the pad", "src_idx", -PAD - 1 - lo_off)
    put("source right of the pad", "src_idx", n + PAD - 1 - hi_off)
    out.update(_bad_windows(g, L))  # (the plain kinds that still apply)
    return out, (lo_off, hi_off)


def test_bad_records_are_refused_by_the_host_form(gpu_ctx, mxlib, takes):  # noqa: F811
    w, a, tr = takes["vowel"]
    n = len(w)
    g, L = mxlib.psola_plan_formant(n, SR, HOP, tr, bend(n, 4.0), const(4.0))
    bads, (lo_off, hi_off) = _bad_records(g, L, n)
    assert len(bads) == 20
    _refused(gpu_ctx, mxlib._capi.lib(), a, g, L, bads)
    # ... a bad curve and a track that does not fit the file, through the one-call form
    for tr_, pts in ((tr, [(5, 1.0), (5, 2.0)]), (tr[:-1], const(1.0))):
        with pytest.raises(mxlib.MxError) as e:
            gpu_ctx.psola_render_formant(a, SR, HOP, tr_, [], pts)
        assert e.value.code == -1
    # the good records still render, and so do records that touch the first and the last sample of the pads exactly
    f32, _ = gpu_ctx.psola_synth_formant(a, g, L, want_i16=False)
    assert np.isfinite(f32).all() and np.abs(f32).max() > 0.1
    k = len(g) // 2
    for idx in (-PAD - lo_off, n + PAD - 2 - hi_off):
        edge = g.copy()
        edge["src_idx"][k] = idx
        e32, _ = gpu_ctx.psola_synth_formant(a, edge, L, want_i16=False)
        assert np.isfinite(e32).all()
