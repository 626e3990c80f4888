"""Sibilant detection, protection and balance of include/melonix_amd.h ("Sibilant detection, protection and balance"),
restated in numpy binary64: features() is the definition the kernel is measured against; segments(), spans(), protect(),
gain_points() and apply_gain() repeat sibilant_logic.cpp / gain_core.h expression by expression (the library must equal them
field for field, the gain byte for byte).  Plus the synthetic take the defaults were chosen on, with its truth."""
import math

import numpy as np

SR = 48000
HOP = 256
FEATURE_DEFAULTS = dict(split_hz=3500.0)
SEGMENT_DEFAULTS = dict(share_on=0.6, share_off=0.4, level_floor=1e-3, zc_min=64, merge_gap=2, min_frames=6)
FEAT_DTYPE = np.dtype([("low", "<f8"), ("high", "<f8"), ("centroid", "<f8"), ("zero_crossings", "<i8")])


def split_bin(sr, split_hz=3500.0):
    return int(min(max(math.ceil(float(np.float32(split_hz)) * 1024.0 / sr), 1), 512))


def features(w, sr, hop, split_hz=3500.0, first=0, count=None):
    """The records of frames [first, first + count) (count None: to the end of the file) -> FEAT_DTYPE array (binary64)."""
    w32 = np.asarray(w, dtype=np.float32)
    n = len(w32)
    frames = -(-n // hop)
    count = frames - first if count is None else count
    ks = split_bin(sr, split_hz)
    pad = np.concatenate([np.zeros(512, np.float32), w32, np.zeros(512 + hop, np.float32)])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    k = np.arange(513, dtype=np.float64)
    out = np.zeros(count, dtype=FEAT_DTYPE)
    for i0 in range(0, count, 4096):
        sel = first + np.arange(i0, min(i0 + 4096, count))
        x = pad[(sel * hop)[:, None] + np.arange(1024)[None, :]]
        P = (np.abs(np.fft.rfft(x.astype(np.float64) * win, axis=1)) / 512.0) ** 2
        low, high = P[:, 1:ks].sum(axis=1), P[:, ks:512].sum(axis=1)
        tot = low + high
        mom = (P[:, 1:512] * k[1:512]).sum(axis=1)
        neg = x < 0  # zeros, -0 and NaN are "not negative"
        o = out[i0:i0 + len(sel)]
        o["low"], o["high"] = low, high
        with np.errstate(invalid="ignore", divide="ignore"):
            o["centroid"] = np.where(tot == 0, 0.0, mom / np.where(tot == 0, 1.0, tot))
        o["zero_crossings"] = np.count_nonzero(neg[:, 1:] != neg[:, :-1], axis=1)
    return out


def views(feat):
    """(level, share) per frame, from the records AS BINARY32 (what mx_sibilants is given)."""
    low, high = np.asarray(feat["low"], np.float32).astype(np.float64), np.asarray(feat["high"], np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = low + high
        ok = np.isfinite(s) & (s > 0)
        level = np.where(ok, np.sqrt(np.where(ok, s, 1.0)), 0.0)
        share = np.where(ok, high / np.where(ok, s, 1.0), 0.0)
    return level, share


def segments(feat, hop, first_frame=0, share_on=0.6, share_off=0.4, level_floor=1e-3, zc_min=64, merge_gap=2, min_frames=6):
    """-> list of (start_sample, end_sample, first_frame, frames, share f32, level f32)."""
    level, share = views(feat)
    zc = np.asarray(feat["zero_crossings"])
    runs, open_, start = [], False, 0
    for f in range(len(level)):
        loud = level[f] >= level_floor
        if not open_:
            if loud and share[f] >= share_on and zc[f] >= zc_min:
                open_, start = True, f
        elif not (loud and share[f] >= share_off):
            open_ = False
            runs.append([start, f - 1])
    if open_:
        runs.append([start, len(level) - 1])
    merged = []
    for a, b in runs:
        if merged and a - merged[-1][1] - 1 <= merge_gap:
            merged[-1][1] = b
        else:
            merged.append([a, b])
    out = []
    for a, b in merged:
        frames = b - a + 1
        if frames < min_frames:
            continue
        s, top = 0.0, 0.0
        for f in range(a, b + 1):
            s += share[f]
            if level[f] > top:
                top = level[f]
        out.append(((first_frame + a) * hop, (first_frame + b) * hop, first_frame + a, frames, np.float32(s / float(frames)), np.float32(top)))
    return out


def spans(sibs, ramp, n):
    """The merged, clipped spans (lo, start, end, hi) of (start_sample, end_sample, ...) tuples."""
    out = []
    for s in sibs:
        a, b = int(s[0]), int(s[1])
        if out and a - ramp <= out[-1][2] + ramp:
            out[-1][2] = b
        else:
            out.append([0, a, b, 0])
    for sp in out:
        sp[0], sp[3] = max(sp[1] - ramp, 0), min(sp[2] + ramp, n - 1)
    return [tuple(sp) for sp in out]


def _span_points(sp, edge, core):
    lo, a, b, hi = sp
    out = []
    if lo < a:
        out.append((lo, edge(lo)))
    out.append((a, core))
    if b > a:
        out.append((b, core))
    if hi > b:
        out.append((hi, edge(hi)))
    return out


def curve(points, x):
    """F(x) of "Independent formant shift" in binary64; points: (sample, semitones f32) pairs."""
    if not points:
        return 0.0
    x = float(x)
    if x < points[0][0]:
        return float(np.float32(points[0][1]))
    if x >= points[-1][0]:
        return float(np.float32(points[-1][1]))
    j = 0
    while points[j + 1][0] <= x:
        j += 1
    y0, y1 = float(np.float32(points[j][1])), float(np.float32(points[j + 1][1]))
    return y0 + (x - float(points[j][0])) * (y1 - y0) / (float(points[j + 1][0]) - float(points[j][0]))


def protect(points, sibs, ramp, n):
    """-> list of (sample, semitones f32)."""
    points = [(int(s), np.float32(v)) for s, v in points]
    if not points:
        return []
    out, j = [], 0
    for sp in spans(sibs, ramp, n):
        while j < len(points) and points[j][0] < sp[0]:
            out.append(points[j])
            j += 1
        out += _span_points(sp, lambda x: np.float32(curve(points, x)), np.float32(0.0))
        while j < len(points) and points[j][0] <= sp[3]:
            j += 1
    return out + points[j:]


def gain_points(sibs, db, ramp, n):
    """-> list of (sample, amp f32)."""
    amp = np.float32(math.pow(10.0, db / 20.0))
    out = []
    for sp in spans(sibs, ramp, n):
        out += _span_points(sp, lambda x: np.float32(1.0), amp)
    return out


def apply_gain(x, points):
    """out_i = (float)((double)x_i * g(i)) -> float32.  points: (sample, amp f32) pairs, a checked list; none: a copy."""
    x = np.asarray(x, dtype=np.float32)
    if not len(points):
        return x.copy()
    s = np.array([int(p[0]) for p in points], dtype=np.int64)
    a = np.array([np.float32(p[1]) for p in points], dtype=np.float64)
    i = np.arange(len(x), dtype=np.int64)
    j = np.searchsorted(s, i, side="right")  # the number of points whose sample is <= i
    j0, j1 = np.clip(j - 1, 0, len(s) - 1), np.clip(j, 0, len(s) - 1)
    den = np.where(s[j1] > s[j0], s[j1] - s[j0], 1).astype(np.float64)
    g = a[j0] + (a[j1] - a[j0]) * ((i - s[j0]).astype(np.float64) / den)
    g = np.where(j <= 0, a[0], np.where(j >= len(s), a[-1], g))
    return (x.astype(np.float64) * g).astype(np.float32)


# ---- the synthetic take ----
TAKE = (("vowel", 0.40, 150.0), ("s", 0.12, None), ("vowel", 0.38, 180.0), ("sh", 0.12, None), ("vowel", 0.30, 130.0), ("gap", 0.10, None),
        ("breath", 0.30, None), ("gap", 0.10, None), ("s_soft", 0.08, None), ("gap", 0.10, None))
NOISE = {"s": (4000.0, 9000.0, 0.05), "sh": (2500.0, 6000.0, 0.05), "breath": (100.0, 2000.0, 0.01), "s_soft": (5000.0, 10000.0, 0.01)}
CLICK = int(1.45 * SR)
SIBILANT_CLASSES = ("s", "sh", "s_soft")


def _bandnoise(rng, n, lo, hi, rms, sr):
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / sr)
    X[(f < lo) | (f > hi)] = 0
    y = np.fft.irfft(X, n)
    return y * rms / np.sqrt(np.mean(y ** 2))


def _vowel(n, f0, sr, amp=0.3):
    t = np.arange(n) / sr
    y = np.zeros(n)
    for h in range(1, 40):
        f = h * f0
        if f > 8000:
            break
        g = 1 / (1 + ((f - 700) / 120) ** 2) + 0.7 / (1 + ((f - 1200) / 150) ** 2) + 0.15 / (1 + ((f - 2600) / 200) ** 2) + 0.002
        y += g * np.sin(2 * np.pi * f * t)
    return amp * y / np.max(np.abs(y))


def take(sr=SR):
    """Vowels (harmonic, three formants), an "s" (4-9 kHz noise), an "sh" (2.5-6 kHz), a breath (< 2 kHz), a soft "s" 14 dB
    down, gaps, each part under 10 ms linear ramps, on the 1e-4 noise bed, a single-sample click inside the breath
    -> (float32 samples, [(class, first sample, one past the last)])."""
    rng = np.random.default_rng(7)
    parts, truth, at = [], [], 0
    for name, dur, f0 in TAKE:
        n = int(dur * sr)
        if name == "vowel":
            y = _vowel(n, f0, sr)
        elif name == "gap":
            y = np.zeros(n)
        else:
            y = _bandnoise(rng, n, *NOISE[name], sr)
        r = int(0.01 * sr)
        e = np.ones(n)
        e[:r], e[-r:] = np.linspace(0, 1, r), np.linspace(1, 0, r)
        parts.append(y * e)
        truth.append((name, at, at + n))
        at += n
    w = np.concatenate(parts) + 1e-4 * np.random.default_rng(1).standard_normal(at)
    w[CLICK] += 0.8
    return w.astype(np.float32), truth
