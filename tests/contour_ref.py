"""The pitch-contour split's definition (include/melonix_amd.h, "Pitch drift and vibrato inside notes" and "PSOLA follows a bend
curve") restated: stage A in binary64, stage B in numpy int64 (prefix sums: the integers make every order equal), the host
logic (default parameters, spans, vibrato figures, bend curve) in Python floats operation for operation, and the PSOLA plan
with a bend curve on top of tests/psola_ref.py (its marks, time map, record layout and render are imported, not restated)."""
import math

import numpy as np

import psola_formant_ref
import psola_ref
from psola_ref import _LIBM, GRAIN_DTYPE, TimeMap, render_length

NONE = -2 ** 31
MAX_WIDTH, MAX_LAG = 64, 256
SPAN_DTYPE = np.dtype([("first", "<i4"), ("frames", "<i4")])
REC_DTYPE = np.dtype([("smooth", "<i4"), ("vib", "<i4")])
STAT_DTYPE = np.dtype([("sum_smooth", "<i8"), ("min_smooth", "<i4"), ("max_smooth", "<i4"), ("r0", "<i8"), ("lag", "<i4"),
                       ("reserved", "<i4"), ("r_lag", "<i8")])
F0_DTYPE = np.dtype([("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])
BEND_DEFAULTS = {"drift_amount": 1.0, "vibrato_scale": 1.0, "glide_frames": 8}


# ---- stage A ----
def cents_exact(track, sr, threshold=0.15, rms_floor=1e-3):
    """-> (voiced bool[count], the pre-rounding binary64 value of every frame (0 where unvoiced))."""
    thr, floor_ = np.float32(threshold), np.float32(rms_floor)
    per = track["period"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = ((track["tau"] > 0) & (track["aperiodicity"].astype(np.float32) < thr) & (track["rms"].astype(np.float32) >= floor_)
             & np.isfinite(per) & (per > np.float32(0)))
    x = np.zeros(len(track), dtype=np.float64)
    p = per[v].astype(np.float64)
    x[v] = 16.0 * (1200.0 * np.log2(float(sr) / p / 55.0) + 2400.0)
    return v, x


def cents(track, sr, threshold=0.15, rms_floor=1e-3):
    """-> int32[count]: NONE where the frame is unvoiced."""
    v, x = cents_exact(track, sr, threshold, rms_floor)
    return np.where(v, np.rint(x), NONE).astype(np.int64).astype(np.int32)


def tie_distance(x):
    """How far each pre-rounding value lies from the nearest rounding tie (k + 1/2), in units."""
    return np.abs(x - np.floor(x) - 0.5)


def track_of(periods, voiced=None, aperiodicity=0.05, rms=0.1):
    """F0 records with these f32 periods (tau: the period rounded, at least 1); voiced False: tau 0."""
    periods = np.asarray(periods, dtype=np.float32)
    t = np.zeros(len(periods), dtype=F0_DTYPE)
    t["period"] = periods
    t["tau"] = np.maximum(np.rint(periods), 1).astype(np.int32)
    t["aperiodicity"], t["rms"] = np.float32(aperiodicity), np.float32(rms)
    if voiced is not None:
        t["tau"][~np.asarray(voiced)] = 0
    return t


def periods_of(cents_f64, sr):
    """The f32 periods whose note is cents_f64 / 1600 (inverse of the note law, rounded to binary32)."""
    return (float(sr) / (55.0 * np.exp2((np.asarray(cents_f64, dtype=np.float64) / 16.0 - 2400.0) / 1200.0))).astype(np.float32)


# ---- stage B ----
def params_default(sr, hop):
    fps = float(sr) / float(hop)
    w = int(min(64.0, max(0.0, math.floor(0.125 * fps))))
    lag_min = int(min(256.0, max(1.0, math.floor(fps / 12.0))))
    lag_max = int(max(float(lag_min), min(256.0, math.ceil(fps / 3.0))))
    return {"half_width": w, "lag_min": lag_min, "lag_max": lag_max}


def box_mean(v, w):
    """mean(v, f) for every f of one span (v int64): the window clipped to the span, nearest with halves up, floor toward
    minus infinity."""
    F = len(v)
    cs = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    f = np.arange(F, dtype=np.int64)
    g0, g1 = np.maximum(f - w, 0), np.minimum(f + w, F - 1)
    S, c = cs[g1 + 1] - cs[g0], g1 - g0 + 1
    return np.floor_divide(2 * S + c, 2 * c)


def split(cents_i32, spans, half_width, lag_min, lag_max):
    """-> (REC_DTYPE[count], STAT_DTYPE[nspans]).  spans: (first, frames) pairs, sorted, disjoint, inside the array."""
    assert 0 <= half_width <= MAX_WIDTH and 1 <= lag_min <= lag_max <= MAX_LAG
    c64 = np.asarray(cents_i32, dtype=np.int64)
    rec = np.zeros(len(c64), dtype=REC_DTYPE)
    rec["smooth"] = NONE
    stat = np.zeros(len(spans), dtype=STAT_DTYPE)
    for i, (first, F) in enumerate(spans):
        first, F = int(first), int(F)
        v = c64[first:first + F]
        smooth = box_mean(box_mean(v, half_width), half_width)
        vib = v - smooth
        rec["smooth"][first:first + F] = smooth
        rec["vib"][first:first + F] = vib
        best_l, best_r = 0, 0
        for L in range(lag_min, min(lag_max, F - 1) + 1):
            r = int(np.dot(vib[:F - L], vib[L:]))
            if best_l == 0 or r > best_r:
                best_l, best_r = L, r
        stat[i] = (int(smooth.sum()), int(smooth.min()), int(smooth.max()), int(np.dot(vib, vib)), best_l, 0, best_r)
    return rec, stat


# ---- host logic ----
def spans_of(notes, first_frame=0):
    out = np.zeros(len(notes), dtype=SPAN_DTYPE)
    out["first"] = notes["first_frame"].astype(np.int64) - first_frame
    out["frames"] = notes["frames"]
    return out


def vibrato(stat, frames, sr, hop):
    """-> dict(rate_hz, extent_cents, strength, drift_cents) of one STAT_DTYPE record."""
    lag, r0 = int(stat["lag"]), int(stat["r0"])
    if lag == 0 or r0 == 0:
        return {"rate_hz": 0.0, "extent_cents": 0.0, "strength": 0.0, "drift_cents": 0.0}
    return {"rate_hz": float(sr) / float(hop) / float(lag),
            "extent_cents": math.sqrt(2.0 * float(r0) / float(frames)) / 16.0,
            "strength": (float(int(stat["r_lag"])) / float(r0)) * float(frames) / float(frames - lag),
            "drift_cents": (float(int(stat["max_smooth"])) - float(int(stat["min_smooth"]))) / 16.0}


def bend(rec, notes, spans, shift=None, drift_amount=1.0, vibrato_scale=1.0, glide_frames=8):
    """-> float32[count]: the bend curve of the definition."""
    out = np.zeros(len(rec), dtype=np.float32)
    for i, (first, F) in enumerate(spans):
        lo, hi = int(first), int(first) + int(F)
        sh = 0.0 if shift is None else float(shift[i])
        note = float(notes["note"][i])
        for h in range(lo, hi):
            drift = float(int(rec["smooth"][h])) / 1600.0 - note
            x = sh - drift_amount * drift
            v = (vibrato_scale - 1.0) * float(int(rec["vib"][h])) / 1600.0
            out[h] = np.float32(x + v)
        if i == 0:
            continue
        end = int(spans[i - 1][0]) + int(spans[i - 1][1])
        G = lo - end
        if G < 1 or G > glide_frames:
            continue
        x0, x1 = float(out[end - 1]), float(out[lo])
        for j in range(1, G + 1):
            out[end - 1 + j] = np.float32(x0 + (x1 - x0) * float(j) / float(G + 1))
    return out


# ---- the PSOLA plan with a bend curve ----
def plan_bend(n, sr, hop, track, markers, bend_curve, **params):
    """psola_ref.plan with the curve (None: psola_ref.plan's operations) -> (GRAIN_DTYPE records, nsamples)."""
    count = (n + hop - 1) // hop
    assert len(track) == count and (bend_curve is None or len(bend_curve) == count)
    L = render_length(n, sr, markers)
    if n == 0 or L == 0:
        return np.zeros(0, GRAIN_DTYPE), L
    a, per, vo = psola_ref.marks(n, hop, track, **params)
    # the frame whose measurement is centred on the mark: the tracker's frame h describes the signal (2048 - period) / 2 before h hop
    frame = [min(max(math.floor((x + (2048.0 - p) / 2.0) / float(hop) + 0.5), 0), count - 1) for x, p in zip(a, per)]
    a_arr = np.array(a, dtype=np.float64)
    tm = TimeMap(markers, sr, n)
    out = []
    s = 0.0
    while True:
        t = s / float(sr)
        src = max(tm.time2sample(t), 0)
        m = int(np.searchsorted(a_arr, float(src), side="right"))
        if m == len(a) or (m > 0 and float(src) - a[m - 1] < a[m] - float(src)):
            m -= 1
        H = per[m]
        if not (s - H < float(L)):
            break
        r = 1.0
        if vo[m]:
            b = float(tm.time2pitchbend(t))
            if bend_curve is not None:
                b = b + float(np.float32(bend_curve[frame[m]]))
            r = float(_LIBM.exp2(b / 12.0))
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


def plan_formant_bend(n, sr, hop, track, markers, points, bend_curve, **params):
    g, L = plan_bend(n, sr, hop, track, markers, bend_curve, **params)
    return psola_formant_ref.formant_records(g, psola_ref.marks(n, hop, track, **params)[0] if len(g) else [], points), L


# ---- the synthetic contour of the chain tests ----
FPS = 187.5  # 48000 / 256


def synthetic_cents(frames=400, centre=45.0, drift_cents=30.0, extent_cents=40.0, rate_hz=6.0, fps=FPS):
    """centre (a note) + a linear drift over the span + a sinusoidal vibrato -> binary64 units of 1/16 cent."""
    f = np.arange(frames, dtype=np.float64)
    return 16.0 * (100.0 * centre + drift_cents * f / float(frames - 1) + extent_cents * np.sin(2.0 * np.pi * rate_hz * f / fps))


# the spans of the device test: 700 frames
CASE_COUNT = 700
CASE_SPANS = [(0, 2), (2, 9), (20, 47), (70, 48), (130, 300), (440, 1), (441, 259)]
CASE_WIDTHS = [0, 1, 23, 64]
CASE_LAGS = [(1, 1), (15, 62), (200, 256)]


def case_cents(kind, count=CASE_COUNT, spans=CASE_SPANS, seed=5):
    """The device test's contour -> int32[count], NONE outside the spans.  'voice': a wandering contour with vibrato around note
    45; 'negative': the same far below zero (what sr 8000 and long periods give); 'constant': one value."""
    rng = np.random.default_rng(seed)
    f = np.arange(count, dtype=np.float64)
    x = 16.0 * (4500.0 + 35.0 * np.sin(2 * np.pi * 5.7 * f / FPS) + 20.0 * np.sin(2 * np.pi * 0.4 * f / FPS)) + rng.integers(-40, 41, count)
    if kind == "negative":
        x = x - 16.0 * 9000.0
    if kind == "constant":
        x = np.full(count, 16.0 * 4512.0)
    out = np.full(count, NONE, dtype=np.int64)
    for first, F in spans:
        out[first:first + F] = np.rint(x[first:first + F]).astype(np.int64)
    return out.astype(np.int32)
