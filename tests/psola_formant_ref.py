"""The independent formant shift of the PSOLA renderer (include/melonix_amd.h, "Independent formant shift") restated in
binary64 on top of tests/psola_ref.py: plan_formant() is psola_ref.plan plus, per record, the curve's value at the grain's
analysis mark, the Q16 step and the Q16 source position of the grain's centre; psola_ref.render() adds these records up as it
does the plain ones."""
import math

import numpy as np

import psola_ref
from psola_ref import _LIBM
from psola_ref import render as render_formant  # noqa: F401  (it takes either record kind)

FGRAIN_DTYPE = np.dtype([("out_lo", "<i4"), ("out_hi", "<i4"), ("src_idx", "<i4"), ("src_q", "<u4"), ("centre", "<i4"),
                         ("centre_frac", "<f4"), ("inv_half", "<f4"), ("step", "<u4")])
ONE = 65536


def curve(points, x):
    """F(x): piecewise linear between the (sample, semitones) points — semitones as binary32 —, constant outside them."""
    if not len(points):
        return 0.0
    xs = [float(int(s)) for s, _ in points]
    ys = [float(np.float32(v)) for _, v in points]
    if x < xs[0]:
        return ys[0]
    if x >= xs[-1]:
        return ys[-1]
    j = max(i for i in range(len(xs)) if xs[i] <= x)
    return ys[j] + (x - xs[j]) * (ys[j + 1] - ys[j]) / (xs[j + 1] - xs[j])


def step_of(semitones):
    phi = float(_LIBM.exp2(semitones / 12.0))
    phi = 0.5 if not (phi >= 0.5) else (2.0 if phi > 2.0 else phi)
    return int(math.floor(phi * 65536.0 + 0.5))


def plan_formant(n, sr, hop, track, markers, points, **params):
    """-> (FGRAIN_DTYPE records, nsamples): psola_ref.plan's records with step, src_idx and src_q."""
    g, L = psola_ref.plan(n, sr, hop, track, markers, **params)
    return formant_records(g, psola_ref.marks(n, hop, track, **params)[0] if len(g) else [], points), L


def _window_of(g):
    """Formant records with the window fields of plain records g, the rest zero."""
    out = np.zeros(len(g), dtype=FGRAIN_DTYPE)
    for f in ("out_lo", "out_hi", "centre", "centre_frac", "inv_half"):
        out[f] = g[f]
    return out


def formant_records(g, a, points):
    """The formant records of plain records g over the analysis marks a (a test that plans one take under several curves
    computes g and a once)."""
    out = _window_of(g)
    for k in range(len(g)):
        am = a[int(g["mark"][k])]
        step = step_of(curve(points, am))
        p0 = am - (float(step) / 65536.0) * float(g["centre_frac"][k])
        q = int(math.floor(p0 * 65536.0 + 0.5))
        out["step"][k], out["src_idx"][k], out["src_q"][k] = step, q >> 16, q & 65535
    return out


def twin(g):
    """The formant records that read what plain records with src_frac == 0 read: step 65536, src_q 0."""
    assert not g["src_frac"].any()
    out = _window_of(g)
    out["src_idx"] = g["centre"] + g["src_off"]
    out["step"] = ONE
    return out
