"""The onset detector and the timing markers of include/melonix_amd.h ("Onset detection and tempo-grid timing markers"),
restated in numpy binary64: flux() is the definition the kernel is measured against; pick() and timing_markers() repeat
onset_logic.cpp expression by expression (the library must equal them field for field).  Plus the synthetic signals the
defaults were chosen on."""
import math

import numpy as np

SR = 48000
HOP = 256
FLUX_DEFAULTS = dict(compress=100.0, lag=1, fmin=0.0, fmax=0.0)
PICK_DEFAULTS = dict(pre_max=3, post_max=3, pre_avg=25, post_avg=1, wait=8, ratio=2.0, delta=1.0)
TIMING_DEFAULTS = dict(bpm=120.0, division=4, offset=0.0, strength=1.0, max_shift=0.1, max_stretch=2.0)


def band(sr, fmin=0.0, fmax=0.0):
    fmax = sr / 2.0 if fmax == 0 else fmax
    return max(1, math.ceil(fmin * 1024.0 / sr)), min(511, math.floor(fmax * 1024.0 / sr))


def compressed_rows(w, hop, compress=100.0):
    """c_h[k], k < 513, of frames 0 .. ceil(n / hop) - 1 -> (frames, 513) float64."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    idx = np.arange(-(-n // hop))
    pad = np.concatenate([np.zeros(512), w, np.zeros(512 + hop)])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    out = np.empty((len(idx), 513))
    for i0 in range(0, len(idx), 4096):
        sel = idx[i0:i0 + 4096]
        fr = pad[(sel * hop)[:, None] + np.arange(1024)[None, :]] * win
        out[i0:i0 + 4096] = np.log1p(compress * np.abs(np.fft.rfft(fr, axis=1)) / 512.0)
    return out


def flux(w, sr, hop, compress=100.0, lag=1, fmin=0.0, fmax=0.0):
    """flux_h of every frame -> float64[ceil(n / hop)]."""
    kmin, kmax = band(sr, fmin, fmax)
    c = compressed_rows(w, hop, compress)[:, kmin:kmax + 1]
    prev = np.concatenate([np.zeros((lag, c.shape[1])), c[:-lag]]) if len(c) > lag else np.zeros_like(c)
    return np.maximum(c - prev, 0.0).sum(axis=1)


def pick(flux_values, hop, first_frame=0, pre_max=3, post_max=3, pre_avg=25, post_avg=1, wait=8, ratio=2.0, delta=1.0):
    """-> list of (sample, frame, strength f32, margin f32)."""
    f32 = np.asarray(flux_values, dtype=np.float32)
    o = np.where(np.isfinite(f32), f32.astype(np.float64), 0.0)
    count = len(o)
    out, last = [], -1
    for f in range(count):
        of = o[f]
        if not all(of > o[g] for g in range(max(0, f - pre_max), f)):
            continue
        if not all(of >= o[g] for g in range(f + 1, min(count - 1, f + post_max) + 1)):
            continue
        lo, hi = max(0, f - pre_avg), min(count - 1, f + post_avg)
        s = 0.0
        for g in range(lo, hi + 1):
            s += o[g]
        thr = ratio * (s / float(hi - lo + 1)) + delta
        if not of >= thr:
            continue
        if last >= 0 and not f - last > wait:
            continue
        last = f
        frame = first_frame + f
        out.append((frame * hop, frame, np.float32(of), np.float32(of - thr)))
    return out


def candidate_margins(flux_values, pre_max=3, post_max=3, pre_avg=25, post_avg=1, ratio=2.0, delta=1.0, **_):
    """o_f - threshold of every local-maximum candidate (the first two rules of pick(), before `wait`) -> (frames, margins)."""
    o = np.asarray(flux_values, dtype=np.float64)
    count = len(o)
    fr, mg = [], []
    for f in range(count):
        if not all(o[f] > o[g] for g in range(max(0, f - pre_max), f)):
            continue
        if not all(o[f] >= o[g] for g in range(f + 1, min(count - 1, f + post_max) + 1)):
            continue
        lo, hi = max(0, f - pre_avg), min(count - 1, f + post_avg)
        fr.append(f)
        mg.append(o[f] - (ratio * o[lo:hi + 1].mean() + delta))
    return np.array(fr, dtype=np.int64), np.array(mg)


def anchor_times(anchors, sr, bpm=120.0, division=4, offset=0.0, strength=1.0, max_shift=0.1, max_stretch=2.0):
    """(a_i > 0, T_i) of the monotone pass."""
    a = [int(x) for x in anchors if int(x) > 0]
    sr = float(sr)
    g = 60.0 / (bpm * float(division))
    T, Tprev, aprev = [], 0.0, 0
    for ai in a:
        t = ai / sr
        q = math.floor((t - offset) / g + 0.5)
        d = offset + q * g - t
        if abs(d) > max_shift:
            d = 0.0
        U = t + strength * d
        span = (ai - aprev) / sr
        lo, hi = span / max_stretch, span * max_stretch
        step = U - Tprev
        step = lo if step < lo else hi if step > hi else step
        Tprev = Tprev + step
        T.append(Tprev)
        aprev = ai
    return a, T


def timing_markers(anchors, n, sr, base=(), **params):
    """-> list of (sample, note, dTime, pitchBend).  base: (sample, note, dTime, pitchBend) tuples."""
    a, T = anchor_times(anchors, sr, **params)
    base = [(int(m[0]), float(m[1]), float(m[2]), float(m[3])) for m in base]
    nb = len(base)
    srf = float(sr)

    def W(s):
        k = 0
        while k < len(a) and s > a[k]:
            k += 1
        ps, pt = (a[k - 1], T[k - 1]) if k else (0, 0.0)
        if k < len(a):
            return pt + (s - ps) * (T[k] - pt) / (a[k] - ps)
        return pt + 1.0 * (s - ps) / srf

    out, ia, ib, sprev, wprev = [], 0, 0, 0, 0.0
    while ia < len(a) or ib < nb:
        if ib < nb and (ia >= len(a) or base[ib][0] <= a[ia]):
            s, note, _, pb = base[ib]
            if ia < len(a) and a[ia] == s:
                ia += 1
            ib += 1
        else:
            s = a[ia]
            ia += 1
            x0, y0, x1, y1 = 0, 0.0, n - 1, 0.0
            if ib > 0:
                x0, y0 = base[ib - 1][0], base[ib - 1][3]
            if ib < nb:
                x1, y1 = base[ib][0], base[ib][3]
            pb = y0 + (s - x0) * (y1 - y0) / (x1 - x0) if x1 > x0 else y0
            if nb == 0:
                note = 0.0
            elif ib == 0:
                note = base[0][1]
            elif ib == nb:
                note = base[nb - 1][1]
            else:
                note = base[ib - 1][1] + (s - base[ib - 1][0]) * (base[ib][1] - base[ib - 1][1]) / (base[ib][0] - base[ib - 1][0])
        w = W(s)
        dt = (w - wprev) - (s - sprev) / srf
        if abs(dt) < 1e-10:
            dt = 0.0
        out.append((s, note, dt, pb))
        sprev, wprev = s, w
    return out


# ---- the signals ----
DUR = 3.0
NOTE_STARTS = (0.25, 0.70, 1.10, 1.62, 2.05, 2.50)
NOTE_F0 = (220.0, 247.0, 262.0, 220.0, 330.0, 294.0)
CLICKS = (12000, 36000, 60001, 84000, 108000, 132000)
LEGATO_STARTS = (0.3, 1.2, 2.1)
LEGATO_F0 = (220.0, 247.0, 262.0)


def _bed(sr=SR):
    return 1e-4 * np.random.default_rng(1).standard_normal(int(DUR * sr))


def _harmonics(phase):
    return sum(np.sin(h * phase) / h for h in range(1, 6))


def notes(attack, sr=SR, amp=0.3):
    """Six decaying harmonic notes (five partials at 1/h), attack seconds of linear rise, e^{-3t} decay, each running until the
    next starts; a 100 ms fade at the end; on the 1e-4 noise bed."""
    n = int(DUR * sr)
    t = np.arange(n) / sr
    w = _bed(sr)
    ends = NOTE_STARTS[1:] + (DUR,)
    for t0, t1, f in zip(NOTE_STARTS, ends, NOTE_F0):
        i0, i1 = int(round(t0 * sr)), int(round(t1 * sr))
        tt = t[i0:i1] - t0
        env = np.minimum(tt / attack, 1.0) * np.exp(-3.0 * tt)
        w[i0:i1] += amp * env * _harmonics(2 * np.pi * f * tt)
    fade = int(0.1 * sr)
    w[-fade:] *= np.linspace(1.0, 0.0, fade)
    return w.astype(np.float32)


def legato(sr=SR, amp=0.3):
    """Three pitches one after the other with a continuous phase and no level dip: the first onset at 0.3 s (a 5 ms rise), pitch
    steps at 1.2 and 2.1 s; a 100 ms fade at the end."""
    n = int(DUR * sr)
    t = np.arange(n) / sr
    f = np.full(n, LEGATO_F0[0])
    f[t >= LEGATO_STARTS[1]] = LEGATO_F0[1]
    f[t >= LEGATO_STARTS[2]] = LEGATO_F0[2]
    phase = 2 * np.pi * np.cumsum(f) / sr
    env = np.clip((t - LEGATO_STARTS[0]) / 0.005, 0.0, 1.0)
    w = _bed(sr) + amp * env * _harmonics(phase)
    fade = int(0.1 * sr)
    w[-fade:] *= np.linspace(1.0, 0.0, fade)
    return w.astype(np.float32)


def vibrato(sr=SR, amp=0.3):
    """A held 220 Hz harmonic tone with a +-0.5 st, 5.5 Hz vibrato, already sounding at sample 0 (frame 0 is no onset: its flux
    is large, and so is the mean around it), with a 100 ms fade at the end (a cut at full level is an event)."""
    n = int(DUR * sr)
    t = np.arange(n) / sr
    f = 220.0 * 2.0 ** (0.5 * np.sin(2 * np.pi * 5.5 * t) / 12.0)
    phase = 2 * np.pi * np.cumsum(f) / sr
    w = _bed(sr) + amp * _harmonics(phase)
    fade = int(0.1 * sr)
    w[-fade:] *= np.linspace(1.0, 0.0, fade)
    return w.astype(np.float32)


def noise(sr=SR):
    return (0.1 * np.random.default_rng(1).standard_normal(int(DUR * sr))).astype(np.float32)


def clicks(sr=SR):
    w = _bed(sr)
    for c in CLICKS:
        w[c] += 0.8
    return w.astype(np.float32)


def signals():
    """name -> (samples, expected onset samples)"""
    return {
        "notes5": (notes(0.005), [int(round(t * SR)) for t in NOTE_STARTS]),
        "notes30": (notes(0.030), [int(round(t * SR)) for t in NOTE_STARTS]),
        "legato": (legato(), [int(round(t * SR)) for t in LEGATO_STARTS]),
        "vibrato": (vibrato(), []),
        "noise": (noise(), []),
        "clicks": (clicks(), list(CLICKS)),
    }
