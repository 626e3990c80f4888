"""The tempo estimator of include/melonix_amd.h ("Tempo and grid-offset estimation"), restated in numpy: smooth() and comb() are
the definitions the kernels must equal bit for bit (f32 products through np.float32 operations, a sequential binary64 running
sum, integer positions); estimate() repeats tempo_logic.cpp expression by expression with the math module (the library's libm).
Plus the synthetic takes the bounds of tests/test_tempo_host.py are stated on."""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

import onset_ref as R

SR = R.SR
HOP = R.HOP
TEMPO_DEFAULTS = dict(bpm_min=30.0, bpm_max=250.0, per_octave=64, smooth=4, window_frames=2048, stride_frames=512,
                      prior_bpm=120.0, prior_octaves=1.0, lock_ratio=0.5)
MIN_PERIOD, MAX_PERIOD = 2 << 16, 4096 << 16
F32 = np.float32

if hasattr(math, "exp2"):
    exp2 = math.exp2
else:  # (Python < 3.11: libm's own exp2, the function tempo_logic.cpp calls — pow(2, x) may differ from it in the last place)
    _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    _libm.exp2.restype, _libm.exp2.argtypes = ctypes.c_double, [ctypes.c_double]
    exp2 = _libm.exp2


def weights(W):
    return np.array([F32(0.5 + 0.5 * math.cos(math.pi * float(d) / float(W + 1))) for d in range(W + 1)], dtype=F32)


def smooth(o, W=4):
    """e_f of every frame -> float32[count]."""
    o = np.asarray(o, dtype=F32)
    z = np.where(np.isfinite(o), o, F32(0)).astype(F32)
    n, h = len(z), weights(W)
    pad = np.concatenate([np.zeros(W, F32), z, np.zeros(W, F32)])
    acc = np.zeros(n, dtype=F32)
    for d in range(-W, W + 1):
        acc = acc + h[abs(d)] * pad[W + d:W + d + n]
    assert acc.dtype == F32
    return acc


def comb_scores(e, first, frames, period):
    """score_phi of every phase of one job -> float32[nph]."""
    e = np.asarray(e, dtype=F32)
    count = len(e)
    first, frames, period = int(first), int(frames), int(period)
    nph = -(-period // 65536)
    start = (first + np.arange(nph, dtype=np.int64)) << 16
    lim = (first + frames - 1) << 16
    J = np.where(start > lim, 0, (lim - start) // period + 1)
    jmax = int(J.max())
    if jmax == 0:
        return np.zeros(nph, dtype=F32)
    j = np.arange(jmax, dtype=np.int64)
    pos = start[:, None] + j[None, :] * period
    idx = np.minimum(pos >> 16, count - 1)
    fr = (pos & 65535).astype(F32) * F32(2.0 ** -16)
    x = (F32(1) - fr) * e[idx] + fr * e[np.minimum(idx + 1, count - 1)]
    assert x.dtype == F32
    x = np.where(j[None, :] < J[:, None], x, F32(0)).astype(np.float64)  # (terms past a phase's J: + 0.0 changes nothing)
    S = np.add.accumulate(x, axis=1)[:, -1]  # sequential, ascending j
    return np.where(J > 0, (S / np.maximum(J, 1).astype(np.float64)).astype(F32), F32(0)).astype(F32)


def comb(e, jobs):
    """jobs: (first, frames, period_q16) each -> list of (score f32, phase, prev f32, next f32)."""
    out = []
    for first, frames, period in jobs:
        s = comb_scores(e, first, frames, period)
        nph = len(s)
        ph = int(np.argmax(s))  # (the first index that attains the maximum)
        out.append((s[ph], ph, s[(ph - 1) % nph], s[(ph + 1) % nph]))
    return out


def ladder(sr, hop, **params):
    """-> (fr, bpm_c, period_c, prior_c), or None where a period leaves the Q16 range."""
    p = dict(TEMPO_DEFAULTS, **params)
    fr = float(sr) / float(hop)
    bpm, period, prior = [], [], []
    c = 0
    while True:
        b = p["bpm_max"] * exp2(-float(c) / float(p["per_octave"]))
        if not b >= p["bpm_min"]:
            break
        q = math.floor(60.0 * fr / b * 65536.0 + 0.5)
        if not MIN_PERIOD <= q <= MAX_PERIOD:
            return None
        z = math.log2(b / p["prior_bpm"]) / p["prior_octaves"]
        bpm.append(b)
        period.append(int(q))
        prior.append(math.exp(-0.5 * (z * z)))
        c += 1
    return fr, bpm, period, prior


EMPTY = dict(bpm=0.0, offset=0.0, score=F32(0), clarity=F32(0), locked_frames=0, levels=0)


def estimate(flux, sr, hop, first_frame=0, details=None, smooth_fn=None, comb_fn=None, **params):
    """-> (dict of mx_tempo's fields, list of (first_frame, frames, bpm f32, score f32) windows).  details: a dict that
    receives A (the aggregated candidates), cstar, anchor and the levels' (first, len, period).  smooth_fn / comb_fn: stand-ins
    for smooth() and comb() with their signatures (tests/tools/tempo_hour.py runs the stages on the GPU through them)."""
    p = dict(TEMPO_DEFAULTS, **params)
    comb_fn = comb_fn or comb
    e = (smooth_fn or smooth)(flux, p["smooth"])
    count = len(e)
    total = float(np.add.accumulate(e.astype(np.float64))[-1]) if count else 0.0
    if not np.any(e != 0):
        return dict(EMPTY), []
    fr, bpms, periods, priors = ladder(sr, hop, **params)
    nc = len(periods)
    W, stride = p["window_frames"], p["stride_frames"]
    win = min(W, count)
    nw = 1 if count < W else (count - W) // stride + 1
    T = np.empty((nw, nc), dtype=F32)
    for i, (s, _, _, _) in enumerate(comb_fn(e, [(w * stride, win, q) for w in range(nw) for q in periods])):
        T[i // nc, i % nc] = s
    A = []
    for c in range(nc):
        s = 0.0
        for w in range(nw):
            s += float(T[w, c])
        A.append(s * priors[c])
    cstar = int(np.argmax(A))
    anchor = int(np.argmax(T[:, cstar]))
    windows = []
    for w in range(nw):
        cw = int(np.argmax([float(T[w, c]) * priors[c] for c in range(nc)]))
        windows.append((first_frame + w * stride, win, F32(60.0 * fr * 65536.0 / float(periods[cw])), T[w, cw]))

    period = periods[cstar]
    step = max(1, int(float(period) * (exp2(1.0 / float(p["per_octave"])) - 1.0) / 8.0))
    L = win
    centre = anchor * stride + win // 2
    base, kept, levels = 0.0, None, []
    while True:
        ln = min(L, count)
        first = min(max(centre - L // 2, 0), count - ln)
        ks = [k for k in range(-12, 13) if MIN_PERIOD <= period + k * step <= MAX_PERIOD]
        rec = comb_fn(e, [(first, ln, period + k * step) for k in ks])
        b = 0
        for i in range(1, len(rec)):
            ka, kb = abs(ks[i]), abs(ks[b])
            if rec[i][0] > rec[b][0] or (rec[i][0] == rec[b][0] and (ka < kb or (ka == kb and ks[i] < ks[b]))):
                b = i
        if not levels:
            base = float(rec[b][0])
        elif float(rec[b][0]) < p["lock_ratio"] * base:
            break
        period = period + ks[b] * step
        kept = (first, ln, rec[b])
        levels.append((first, ln, period))
        if ln == count:
            break
        L *= 8
        step = max(1, step // 8)

    first, ln, (score, phase, prv, nxt) = kept
    g = (float(period) / 65536.0) / fr
    sp, s0, sn = float(prv), float(score), float(nxt)
    curv = sp - 2.0 * s0 + sn
    delta = 0.0
    if curv < 0.0:
        delta = 0.5 * (sp - sn) / curv
        delta = -0.5 if delta < -0.5 else 0.5 if delta > 0.5 else delta
    offset = math.fmod((float(first_frame + first + phase) + delta) / fr, g)
    if offset < 0.0:
        offset += g
    if not offset < g:
        offset = 0.0
    mean = total / float(count)
    if details is not None:
        details.update(A=A, cstar=cstar, anchor=anchor, levels=levels, T=T, e=e)
    return dict(bpm=60.0 / g, offset=offset, score=F32(score), clarity=F32(s0 / mean) if mean > 0.0 else F32(0), locked_frames=ln,
                levels=len(levels)), windows


# ---- the takes ----
def take(bpm, dur, jitter=0.0, lead=0.0, per_beat=1, seed=1, drop=0.15, first_beat=0.25, sr=SR, amp=0.3, attack=0.005):
    """Decaying harmonic notes (onset_ref.notes' recipe: five partials at 1/h, a linear attack, e^{-3t} decay, each running
    until the next starts, on the 1e-4 noise bed, a 100 ms fade at the end) on the grid lead + first_beat + k * 60 / (bpm *
    per_beat), each moved by a seeded uniform +-jitter seconds, `drop` of them left out.  -> (samples f32, the onset times)."""
    rng = np.random.default_rng(seed)
    n = int(round((lead + dur) * sr))
    t = np.arange(n) / sr
    w = 1e-4 * rng.standard_normal(n)
    step = 60.0 / (bpm * per_beat)
    grid = np.arange(lead + first_beat, lead + dur - 0.2, step)
    keep = rng.random(len(grid)) >= drop
    keep[0] = True
    starts = (grid + rng.uniform(-jitter, jitter, len(grid)))[keep]
    ends = np.concatenate([starts[1:], [lead + dur]])
    for k, (t0, t1) in enumerate(zip(starts, ends)):
        i0, i1 = int(round(t0 * sr)), int(round(t1 * sr))
        tt = t[i0:i1] - t0
        env = np.minimum(tt / attack, 1.0) * np.exp(-3.0 * tt)
        w[i0:i1] += amp * env * R._harmonics(2 * np.pi * R.NOTE_F0[k % len(R.NOTE_F0)] * tt)
    fade = int(0.1 * sr)
    w[-fade:] *= np.linspace(1.0, 0.0, fade)
    return w.astype(F32), starts


# name -> take()'s arguments; the truth of each is its bpm, per_beat and the line at lead + first_beat
TAKES = {
    "bpm100_jitter": dict(bpm=100.0, dur=14.0, jitter=0.010, seed=11),
    "bpm132_half_beats": dict(bpm=132.0, dur=14.0, per_beat=2, seed=12),
    "bpm87_after_silence": dict(bpm=87.3, dur=40.0, lead=6.0, seed=13),
    "bpm120_exact": dict(bpm=120.0, dur=14.0, seed=14),
}


@functools.lru_cache(maxsize=None)
def take_wave(name):
    return take(**TAKES[name])[0]


@functools.lru_cache(maxsize=None)
def take_flux(name):
    """The take's onset strength by the binary64 definition (onset_ref.flux), as the f32 values an estimate takes."""
    return R.flux(take_wave(name), SR, HOP).astype(F32)


@functools.lru_cache(maxsize=None)
def take_estimate(name):
    details = {}
    res, windows = estimate(take_flux(name), SR, HOP, details=details)
    return res, windows, details


def grid_error(name, res):
    """(offset error modulo the finer of the true onset spacing and the estimated beat, seconds; |bpm error| / bpm against the
    nearest octave of the estimate; the take's length, seconds)."""
    a = TAKES[name]
    true_bpm = a["bpm"]
    m = min((0.25, 0.5, 1.0, 2.0, 4.0), key=lambda k: abs(res["bpm"] * k - true_bpm))
    q = min(60.0 / (true_bpm * a.get("per_beat", 1)), 60.0 / res["bpm"])
    line = a.get("lead", 0.0) + a.get("first_beat", 0.25)
    off = abs((res["offset"] - line + q / 2) % q - q / 2)
    return off, abs(res["bpm"] * m - true_bpm) / true_bpm, a.get("lead", 0.0) + a["dur"]


# ---- the comb shapes the CPU emulation and the GPU are both held to ----
# Q16 periods: 2.0, 2 + 1/65536, 45.0, 93.75, 375.5, 1000.25, 4096.0 (the last three: more than 256 phases, the strided path)
COMB_PERIODS = (2 << 16, (2 << 16) + 1, 45 << 16, 93 * 65536 + 49152, 375 * 65536 + 32768, 1000 * 65536 + 16384, 4096 << 16)
COMB_COUNTS = (1, 2, 65, 257, 2049)
COMB_CURVES = ("noise", "constant", "zeros", "spike")
SPIKE = F32(8.0)


def spike_frame(count):
    return count // 3


def comb_curve(kind, count):
    if kind == "noise":
        return np.abs(np.random.default_rng(1000 + count).standard_normal(count)).astype(F32)
    if kind == "constant":
        return np.full(count, 2.0, dtype=F32)  # (a power of two: every interpolation is exact, so every phase ties)
    e = np.zeros(count, dtype=F32)
    if kind == "spike":
        e[spike_frame(count)] = SPIKE
    return e


def comb_segments(count, period):
    """(first, frames): the whole curve, frame 0 alone, the last frame alone, a segment ending at count, one shorter than
    its period (its later phases have J = 0)."""
    half = count // 2
    short_first = min(3, count - 1)
    short = max(1, min(count - short_first, (-(-period // 65536)) // 2))
    return [(0, count), (0, 1), (count - 1, 1), (half, count - half), (short_first, short)]


def comb_jobs(count):
    return [(first, frames, q) for q in COMB_PERIODS for first, frames in comb_segments(count, q)]


@functools.lru_cache(maxsize=None)
def comb_case(kind, count):
    """-> (curve, jobs, the reference's records), computed once."""
    e = comb_curve(kind, count)
    e.setflags(write=False)
    jobs = comb_jobs(count)
    return e, jobs, comb(e, jobs)


def records_array(recs, dtype):
    out = np.zeros(len(recs), dtype=dtype)
    for i, (s, ph, pv, nx) in enumerate(recs):
        out[i] = (s, ph, pv, nx)
    return out


def same_estimate(got, want):
    """Every field of mx_tempo and of the window curve, byte for byte."""
    (g, gw), (w, ww) = got, want
    for k in ("bpm", "offset"):
        assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), (k, g, w)
    for k in ("score", "clarity"):
        assert np.float32(g[k]).tobytes() == np.float32(w[k]).tobytes(), (k, g, w)
    assert (int(g["locked_frames"]), int(g["levels"])) == (int(w["locked_frames"]), int(w["levels"])), (g, w)
    assert len(gw) == len(ww), (len(gw), len(ww))
    for a, b in zip(gw, ww):
        assert (int(a["first_frame"]), int(a["frames"])) == (int(b[0]), int(b[1]))
        assert a["bpm"].tobytes() == np.float32(b[2]).tobytes() and a["score"].tobytes() == np.float32(b[3]).tobytes(), (a, b)
