"""The PSOLA renderer's definition (include/melonix_amd.h, "Formant-preserving PSOLA rendering") restated in binary64:
plan() makes the grain records from an f0 track and the markers, render() adds grains up.  render() takes RECORDS — plain ones,
or the formant shift's (tests/psola_formant_ref.py) —, so the GPU is compared on the plan it was actually given.  The marker maps are the editor's piecewise-linear ones (the same the
marker-driven phase vocoder follows), written out here once more so that this file depends on nothing but numpy and the C
library's exp2 (the product's host code calls std::exp2; numpy's own differs in the last bit)."""
import ctypes
import ctypes.util
import math

import numpy as np

import pcm_extremes

MAX_HALF = 2048
PAD = 32768
DEFAULTS = {"threshold": np.float32(0.15), "rms_floor": np.float32(1e-3), "unvoiced_period": np.float32(256.0)}
GRAIN_DTYPE = np.dtype([("out_lo", "<i4"), ("out_hi", "<i4"), ("src_off", "<i4"), ("src_frac", "<f4"), ("centre", "<i4"),
                        ("centre_frac", "<f4"), ("inv_half", "<f4"), ("mark", "<i4")])

_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.exp2.restype = ctypes.c_double
_LIBM.exp2.argtypes = [ctypes.c_double]


class TimeMap:
    """The marker maps as pure functions of (markers, sr, n): sample2time, time2sample, time2pitchbend, duration."""

    def __init__(self, markers, sr, n):
        self.sr, self.n, self.segs = sr, n, []
        ps, pt, pb = 0, 0.0, 0.0
        for (s, _note, dt, b) in markers:
            s, dt, b = int(s), float(dt), float(b)
            rt = pt + 1.0 * (s - ps) / sr + dt
            self.segs.append((ps, s, pt, rt, pb, b))
            ps, pt, pb = s, rt, b
        self.last = (ps, pt, pb)

    def sample2time(self, v):
        if v <= 0:
            return 1.0 * v / self.sr
        for ps, s, pt, rt, _, _ in self.segs:
            if ps < v <= s:
                return pt + (v - ps) * (rt - pt) / (s - ps)
        return self.last[1] + 1.0 * (v - self.last[0]) / self.sr

    def duration(self):
        return self.sample2time(self.n - 1)

    def time2sample(self, t):
        if t <= 0:
            return int(t * self.sr)
        for ps, s, pt, rt, _, _ in self.segs:
            if pt < t <= rt:
                return int(ps + (t - pt) * (s - ps) / (rt - pt))
        return int(self.last[0] + (t - self.last[1]) * self.sr)

    def time2pitchbend(self, t):
        """-> binary32, as the editor's float return."""
        if t <= 0:
            return np.float32(0.0)
        for _, _, pt, rt, pb, b in self.segs:
            if pt < t <= rt:
                return np.float32(pb + (t - pt) * (b - pb) / (rt - pt))
        dur = self.duration()
        if t > dur:
            return np.float32(0.0)
        ls, lt, lb = self.last
        with np.errstate(all="ignore"):
            return np.float32(np.float64(lb) + np.float64(t - lt) * np.float64(0 - lb) / np.float64(dur - lt))


def render_length(n, sr, markers):
    """The number of output samples i with i / sr < duration() (mx_pv_render_length)."""
    dur = TimeMap(markers, sr, n).duration()
    sr = float(sr)
    L = int(math.ceil(dur * sr - 1e-12)) if dur > 0 else 0
    while L > 0 and (L - 1) / sr >= dur:
        L -= 1
    while L / sr < dur:
        L += 1
    return L


def voicing(track, params):
    """-> (voiced bool[count], period f64[count]) by the definition's rule."""
    thr, floor_ = np.float32(params["threshold"]), np.float32(params["rms_floor"])
    per = track["period"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = ((track["tau"] > 0) & (track["aperiodicity"].astype(np.float32) < thr) & (track["rms"].astype(np.float32) >= floor_)
             & np.isfinite(per) & (per >= np.float32(2.0)) & (per <= np.float32(MAX_HALF)))
    return v, per.astype(np.float64)


def marks(n, hop, track, **params):
    """The analysis marks of a file of n > 0 samples -> (a_m, the period at a_m, voiced at a_m), a list each."""
    p = dict(DEFAULTS)
    p.update(params)
    count = (n + hop - 1) // hop
    assert len(track) == count
    U = float(np.float32(p["unvoiced_period"]))
    voiced, period = voicing(track, p)

    def at(x):
        h = min(max(math.floor(x / float(hop) + 0.5), 0), count - 1)
        return (float(period[h]), True) if voiced[h] else (U, False)

    a, per, vo = [], [], []
    am = 0.0
    while True:
        pm, v = at(am)
        if not (am - pm < float(n)):
            break
        a.append(am)
        per.append(pm)
        vo.append(v)
        am = am + pm
    return a, per, vo


def plan(n, sr, hop, track, markers, **params):
    """-> (GRAIN_DTYPE records, nsamples)."""
    assert len(track) == (n + hop - 1) // hop
    L = render_length(n, sr, markers)
    if n == 0 or L == 0:
        return np.zeros(0, GRAIN_DTYPE), L
    a, per, vo = marks(n, hop, track, **params)
    a_arr = np.array(a, dtype=np.float64)

    tm = TimeMap(markers, sr, n)
    out = []
    s = 0.0
    while True:
        t = s / float(sr)
        src = max(tm.time2sample(t), 0)
        m = int(np.searchsorted(a_arr, float(src), side="right"))
        if m == len(a) or (m > 0 and float(src) - a[m - 1] < a[m] - float(src)):  # (ties: the higher index)
            m -= 1
        H = per[m]
        if not (s - H < float(L)):
            break
        r = 1.0
        if vo[m]:
            r = float(_LIBM.exp2(float(tm.time2pitchbend(t)) / 12.0))
            r = 0.5 if not (r >= 0.5) else (2.0 if r > 2.0 else r)
        d = a[m] - s
        so, cf = math.floor(d), math.floor(s)
        sf, cfr = np.float32(d - so), np.float32(s - cf)
        if sf >= np.float32(1.0):
            so, sf = so + 1, np.float32(0.0)
        if cfr >= np.float32(1.0):
            cf, cfr = cf + 1, np.float32(0.0)
        out.append((max(0, math.floor(s - H) + 1), min(L, math.ceil(s + H)), so, sf, cf, cfr, np.float32(1.0 / H), m))
        s = s + H / r
    return np.array(out, dtype=GRAIN_DTYPE), L


def _source(g, i):
    """Where outputs i of record g read the source -> (index, fraction).  A plain record: i + src_off and src_frac; a formant
    record: the Q16 position src_idx.src_q + step (i - centre) in integer arithmetic (the Q16 step is the definition: nothing
    about a position is rounded here or on the device)."""
    if "step" not in g.dtype.names:
        return i + int(g["src_off"]), float(g["src_frac"])
    pos = (int(g["src_idx"]) << 16) + int(g["src_q"]) + int(g["step"]) * (i - int(g["centre"]))
    return pos >> 16, (pos & 65535).astype(np.float64) / 65536.0


def render(wav, grains, nsamples):
    """-> f64[nsamples]: the overlap-add of the records (either kind) over `wav` (zeros outside the file), sums in ascending
    k, interpolation and sums in binary64."""
    n = len(wav)
    x = np.zeros(n + 2 * PAD, dtype=np.float64)
    x[PAD:PAD + n] = wav
    S = np.zeros(nsamples, dtype=np.float64)
    W = np.zeros(nsamples, dtype=np.float64)
    for g in grains:
        lo, hi = int(g["out_lo"]), int(g["out_hi"])
        if hi <= lo:
            continue
        i = np.arange(lo, hi, dtype=np.int64)
        u = ((i - int(g["centre"])).astype(np.float64) - float(g["centre_frac"])) * float(g["inv_half"])
        keep = np.abs(u) < 1.0
        i, u = i[keep], u[keep]
        w = 0.5 + 0.5 * np.cos(np.pi * u)
        j, f = _source(g, i)
        j = j + PAD
        S[i] += w * ((1.0 - f) * x[j] + f * x[j + 1])
        W[i] += w
    return np.where(W > 0, S / np.maximum(W, 0.25), 0.0)


def pcm16(y):
    """The int16 the definition takes of a binary32 sample: the clamped form, NaN -> 0."""
    return pcm_extremes.clamped_i16(y)
