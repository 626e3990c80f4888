"""The formant planner (mx_psola_plan_formant, host code: no GPU) against its f64 restatement tests/psola_formant_ref.py, field
for field; the curves it refuses; the two instantiations of the kernel in the compiler's own report; and, on the reference
alone, what the definition promises: the envelope moves by the formant value, the note by the bend."""
import ctypes as C

import numpy as np
import pytest

import psola_formant_ref as FR
import psola_ref
import yin_ref
from conftest import SR
from test_abi import _resource_usage
from test_psola_host import HOP, marker_sets, tracks

TRACKS = ("voiced", "unvoiced", "blocks", "period2", "period2048", "abrupt", "garbage", "wander")
MARKERS = ("none", "const+4", "ramp", "warp4", "warp1/4", "bend+30", "bend-30")


def curves(n):
    """name -> (sample, semitones) points for a file of n samples."""
    return {
        "constant": [(0, 3.0), (max(n, 1), 3.0)],
        "ramp": [(0, -5.0), (max(n - 1, 1), 5.0)],
        "outside": [(-1000, -2.0), (n // 3, 4.0), (n + 5000, -6.0)],  # points before sample 0 and behind n
        "single": [(n // 2, -3.5)],
        "clamps": [(0, 12.0), (n // 4 + 1, 12.5), (n // 2 + 2, 40.0), (n // 2 + 3, -12.0), (3 * n // 4 + 4, -1e30)],
    }


def _cases():
    out = []
    for n in (1, 255, 4096):
        for tn in TRACKS:
            for mn in MARKERS:
                out.append((n, tn, mn))
    # (the long file: one plan per voicing pattern that changes along the take; the periods of 2 and the warps are covered above)
    out += [(72000, "voiced", "ramp"), (72000, "blocks", "warp4"), (72000, "wander", "warp1/4"), (72000, "abrupt", "const+4")]
    return out


@pytest.mark.parametrize("n,tn,mn", _cases())
def test_plan_matches_reference(mxlib, n, tn, mn):
    track, markers = tracks(n, HOP)[tn], marker_sets(n, SR)[mn]
    g, L = psola_ref.plan(n, SR, HOP, track, markers)
    marks = psola_ref.marks(n, HOP, track)[0] if len(g) else []
    pg, pL = mxlib.psola_plan(n, SR, HOP, track, markers)
    assert pL == L
    for cn, pts in curves(n).items():
        fg, fL = mxlib.psola_plan_formant(n, SR, HOP, track, markers, pts)
        ref = FR.formant_records(g, marks, pts)
        assert fL == L and len(fg) == len(ref), cn
        for f in fg.dtype.names:
            assert fg[f].tobytes() == ref[f].tobytes(), (cn, f, int(np.argmax(fg[f] != ref[f])))
        # marks, spacing and windows are the plain plan's
        for f in ("out_lo", "out_hi", "centre", "centre_frac", "inv_half"):
            assert fg[f].tobytes() == pg[f].tobytes(), (cn, f)
        if not len(fg):
            continue
        assert (fg["step"] >= 32768).all() and (fg["step"] <= 131072).all() and (fg["src_q"] < 65536).all()
        if cn == "constant":
            assert set(np.unique(fg["step"])) == {FR.step_of(3.0)}
        if cn == "clamps" and n >= 4096 and tn in ("voiced", "blocks", "wander", "period2"):  # both limits, exactly (ten marks and more)
            assert fg["step"].max() == 131072 and fg["step"].min() == 32768
        if cn == "ramp" and n >= 4096 and tn == "voiced" and mn == "none":  # a new step in every grain
            inside = fg["centre"][1:] < n - 1  # (the curve is constant behind its last point, and so are the marks behind the file)
            assert inside.sum() > 8 and (np.diff(fg["step"].astype(np.int64))[inside] > 0).all()


def test_plan_formant_is_the_reference_plan_formant(mxlib):
    """plan_formant() itself (the test above shares the plain plan among the curves)."""
    n = 4096
    track, markers = tracks(n, HOP)["blocks"], marker_sets(n, SR)["ramp"]
    pts = curves(n)["outside"]
    fg, L = mxlib.psola_plan_formant(n, SR, HOP, track, markers, pts, unvoiced_period=100.0)
    ref, rL = FR.plan_formant(n, SR, HOP, track, markers, pts, unvoiced_period=100.0)
    assert L == rL and fg.tobytes() == ref.tobytes()
    # ... and with a long curve handed in as a list of pairs: the wrapper's own array of the points has to outlive the call
    pts = [(40 * j - 2000, float(7.0 * np.sin(0.37 * j))) for j in range(1000)]
    fg, L = mxlib.psola_plan_formant(n, SR, HOP, track, markers, pts)
    ref, rL = FR.plan_formant(n, SR, HOP, track, markers, pts)
    assert L == rL and fg.tobytes() == ref.tobytes() and np.unique(fg["step"]).size > 10


def test_no_points_is_step_one(mxlib):
    for n, tn, mn in ((4096, "blocks", "ramp"), (72000, "wander", "warp4"), (255, "period2", "bend+30")):
        track, markers = tracks(n, HOP)[tn], marker_sets(n, SR)[mn]
        fg, L = mxlib.psola_plan_formant(n, SR, HOP, track, markers, [])
        g, pL = mxlib.psola_plan(n, SR, HOP, track, markers)
        assert L == pL and len(fg) == len(g) and (fg["step"] == 65536).all()
        # ... and reads where the plain record reads, to the Q16 the position is kept in: (centre + src_off) + src_frac
        pos = (fg["src_idx"].astype(np.int64) << 16) + fg["src_q"]
        plain = ((g["centre"].astype(np.int64) + g["src_off"]) << 16) + np.floor(g["src_frac"].astype(np.float64) * 65536 + 0.5).astype(np.int64)
        assert np.abs(pos - plain).max() <= 1


def test_bad_curves_and_arguments_are_refused(mxlib):
    n = 4096
    t = tracks(n)["voiced"]
    for pts in ([(100, 1.0), (50, 1.0)], [(100, 1.0), (100, 2.0)], [(0, float("nan"))], [(0, 1.0), (5, float("inf"))],
                [(0, 1.0), (5, float("-inf")), (9, 0.0)]):
        with pytest.raises(mxlib.MxError) as e:
            mxlib.psola_plan_formant(n, SR, HOP, t, [], pts)
        assert e.value.code == -1 and "formant" in str(e.value), pts
    # what mx_psola_plan refuses
    for kw in (dict(track=t[:-1]), dict(hop=0, track=t[:0]), dict(sr=0), dict(markers=[(100, 0, 0.0, 1.0), (50, 0, 0.0, 1.0)])):
        a = dict(sr=SR, hop=HOP, track=t, markers=[])
        a.update(kw)
        with pytest.raises(mxlib.MxError) as e:
            mxlib.psola_plan_formant(n, a["sr"], a["hop"], a["track"], a["markers"], [(0, 1.0)])
        assert e.value.code == -1, kw
    with pytest.raises(mxlib.MxError):
        mxlib.psola_plan_formant(n, SR, HOP, t, [], [(0, 1.0)], unvoiced_period=8.0)
    L = mxlib._capi.lib()
    cnt, ns, out = C.c_int64(), C.c_int64(), C.c_void_p()
    tp = C.c_void_p(t.ctypes.data)
    pts = np.array([(0, 1.0)], dtype=mxlib.FORMANT_POINT_DTYPE)
    pp = C.c_void_p(pts.ctypes.data)
    assert L.mx_psola_plan_formant(n, SR, HOP, tp, len(t), None, None, 0, pp, 1, None, C.byref(cnt), C.byref(ns)) == -1
    assert L.mx_psola_plan_formant(n, SR, HOP, tp, len(t), None, None, 0, pp, 1, C.byref(out), None, C.byref(ns)) == -1
    assert L.mx_psola_plan_formant(n, SR, HOP, tp, len(t), None, None, 0, pp, 1, C.byref(out), C.byref(cnt), None) == -1
    assert L.mx_psola_plan_formant(n, SR, HOP, tp, len(t), None, None, 0, None, 1, C.byref(out), C.byref(cnt), C.byref(ns)) == -1
    assert L.mx_psola_plan_formant(n, SR, HOP, tp, len(t), None, None, 0, pp, -1, C.byref(out), C.byref(cnt), C.byref(ns)) == -1
    assert out.value is None and b"formant" in L.mx_last_error()
    # the entry points that need a context refuse a null one before the device, points or not
    g = np.zeros(1, dtype=mxlib.PSOLA_FGRAIN_DTYPE)
    o = np.full(16, 7.0, dtype=np.float32)
    gp, op = C.c_void_p(g.ctypes.data), C.c_void_p(o.ctypes.data)
    assert L.mx_psola_synth_formant(None, None, gp, 1, 16, op, None) == -1
    assert L.mx_psola_synth_formant_dev(None, None, gp, 1, 16, op, None) == -1
    for npts in (0, 1):
        assert L.mx_psola_render_formant(None, None, SR, HOP, tp, len(t), None, None, 0, pp, npts, op, None) == -1
        assert L.mx_psola_render_formant_dev(None, None, SR, HOP, tp, len(t), None, None, 0, pp, npts, op, None) == -1
    assert b"null context" in L.mx_last_error() and (o == 7.0).all()


def test_both_kernel_instantiations_are_scratch_free():
    names, scratch, vgprs = _resource_usage("psola_kernels.hip")
    assert sum("psola_kernel" in x and "mx_psola_grain" in x for x in names) == 1, names
    assert sum("psola_kernel" in x and "mx_psola_fgrain" in x for x in names) == 1, names
    print("psola_kernels.hip:", list(zip(names, scratch, vgprs)))
    assert not [(x, s) for x, s in zip(names, scratch) if s != 0] and max(vgprs) <= 256


# ---- the definition on the reference alone: the table of DESIGN.md §5f ----
F0 = 150.0


@pytest.fixture(scope="module")
def vowel_take():
    from test_gpu_psola import _median_note, vowel
    w = vowel()
    recs, _ = yin_ref.track(w.astype(np.float64), SR, HOP)
    track = np.array(recs, dtype=[("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])
    note = _median_note([p for (t, p, ap, _) in recs if t > 0 and ap < 0.15])
    return w, track, note


@pytest.mark.parametrize("bend,formant", [(0.0, 4.0), (0.0, -3.0), (4.0, 4.0), (4.0, -3.0), (-5.0, 5.0)])
def test_reference_moves_envelope_and_note_apart(vowel_take, bend, formant):
    from test_gpu_psola import _ref_note, _strongest_harmonic
    w, track, note_in = vowel_take
    n = len(w)
    mk = [(1, 0, 0.0, bend), (n - 1, 0, 0.0, bend)] if bend else []
    fg, L = FR.plan_formant(n, SR, HOP, track, mk, [(0, formant)])
    y = FR.render_formant(w, fg, L)
    spacing = F0 * 2.0 ** (bend / 12.0)
    target = 1200.0 * 2.0 ** (formant / 12.0)
    peak = _strongest_harmonic(y)
    moved = _ref_note(y) - note_in
    print(f"formant ref: bend {bend:+g}, formant {formant:+g} st: strongest harmonic {peak:.0f} Hz (target {target:.0f}, harmonic "
          f"spacing {spacing:.0f}), median note moved {moved:+.5f} st")
    assert abs(peak - target) <= spacing
    assert abs(moved - bend) <= 0.05
