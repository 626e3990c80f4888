"""The independent formant shift of the PSOLA renderer (include/melonix_amd.h, "Independent formant shift") restated in
binary64 on top of tests/psola_ref.py: plan_formant() is psola_ref.plan plus, per record, the curve's value at the grain's
analysis mark, the Q16 step and the Q16 source position of the grain's centre; render_formant() adds the grains up with the
positions in integer arithmetic (the Q16 step is the definition: nothing about a position is rounded here or on the device)
and the interpolation and the sums in binary64."""
import math

import numpy as np

import psola_ref
from psola_ref import PAD, _LIBM

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


def analysis_marks(n, hop, track, **params):
    """a_m of psola_ref.plan (the same recurrence; the plain records carry only the index m)."""
    p = dict(psola_ref.DEFAULTS)
    p.update(params)
    count = (n + hop - 1) // hop
    U = float(np.float32(p["unvoiced_period"]))
    voiced, period = psola_ref.voicing(track, p)
    a, am = [], 0.0
    while True:
        h = min(max(math.floor(am / float(hop) + 0.5), 0), count - 1)
        pm = float(period[h]) if voiced[h] else U
        if not (am - pm < float(n)):
            break
        a.append(am)
        am = am + pm
    return a


def step_of(semitones):
    phi = float(_LIBM.exp2(semitones / 12.0))
    phi = 0.5 if not (phi >= 0.5) else (2.0 if phi > 2.0 else phi)
    return int(math.floor(phi * 65536.0 + 0.5))


def plan_formant(n, sr, hop, track, markers, points, **params):
    """-> (FGRAIN_DTYPE records, nsamples): psola_ref.plan's records with step, src_idx and src_q."""
    g, L = psola_ref.plan(n, sr, hop, track, markers, **params)
    return formant_records(g, analysis_marks(n, hop, track, **params) if len(g) else [], points), L


def formant_records(g, a, points):
    """The formant records of plain records g over the analysis marks a (a test that plans one take under several curves
    computes g and a once)."""
    out = np.zeros(len(g), dtype=FGRAIN_DTYPE)
    for f in ("out_lo", "out_hi", "centre", "centre_frac", "inv_half"):
        out[f] = g[f]
    for k in range(len(g)):
        am = a[int(g["mark"][k])]
        step = step_of(curve(points, am))
        p0 = am - (float(step) / 65536.0) * float(g["centre_frac"][k])
        q = int(math.floor(p0 * 65536.0 + 0.5))
        out["step"][k], out["src_idx"][k], out["src_q"][k] = step, q >> 16, q & 65535
    return out


def render_formant(wav, fgrains, nsamples):
    """-> f64[nsamples]: the overlap-add of the records over `wav` (zeros outside the file), sums in ascending k."""
    n = len(wav)
    x = np.zeros(n + 2 * PAD, dtype=np.float64)
    x[PAD:PAD + n] = wav
    S = np.zeros(nsamples, dtype=np.float64)
    W = np.zeros(nsamples, dtype=np.float64)
    for g in fgrains:
        lo, hi = int(g["out_lo"]), int(g["out_hi"])
        if hi <= lo:
            continue
        i = np.arange(lo, hi, dtype=np.int64)
        u = ((i - int(g["centre"])).astype(np.float64) - float(g["centre_frac"])) * float(g["inv_half"])
        keep = np.abs(u) < 1.0
        i, u = i[keep], u[keep]
        w = 0.5 + 0.5 * np.cos(np.pi * u)
        pos = (int(g["src_idx"]) << 16) + int(g["src_q"]) + int(g["step"]) * (i - int(g["centre"]))
        j = (pos >> 16) + PAD
        f = (pos & 65535).astype(np.float64) / 65536.0
        S[i] += w * ((1.0 - f) * x[j] + f * x[j + 1])
        W[i] += w
    return np.where(W > 0, S / np.maximum(W, 0.25), 0.0)


def twin(g):
    """The formant records that read what plain records with src_frac == 0 read: step 65536, src_q 0."""
    assert not g["src_frac"].any()
    out = np.zeros(len(g), dtype=FGRAIN_DTYPE)
    for f in ("out_lo", "out_hi", "centre", "centre_frac", "inv_half"):
        out[f] = g[f]
    out["src_idx"] = g["centre"] + g["src_off"]
    out["step"] = ONE
    return out
