"""Loudness and note levelling of include/melonix_amd.h ("Loudness and note levelling"), restated in numpy binary64: steps() is
the definition the kernel must equal byte for byte (given the library's own coefficients: tan and pow may differ by an ulp
between libm and numpy); curve(), integrated(), note_loudness(), level_gain_points() and normalize_gain() repeat
loudness_logic.cpp expression by expression.  Plus the synthetic takes: tones, PCG noise, the levelling take."""
import functools
import math

import numpy as np

import sibilant_ref as SIB

G = 10
MIN_RATE, MAX_RATE = 8000, 384000
STEP_DTYPE = np.dtype([("energy", "<f8"), ("peak", "<f4"), ("samples", "<i4")])
ABS_GATE = float.fromhex("0x1.f791ec6e1d5b7p-24")  # 10^((-70 + 0.691) / 10)
OFFSET = -0.691
LEVEL_DEFAULTS = {"raise": 1.0, "lower": 1.0, "max_db": 12.0}
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0, b1, b2, a1, a2 of the shelf; a1, a2 of the high-pass
BS1770_TABLE = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                -1.99004745483398, 0.99007225036621)


def geometry(n, sr):
    """-> (S, W, steps, groups)"""
    S = (sr + 50) // 100
    W = 4 * ((32 * sr + 1499) // 1500)
    steps = -(-n // S) if n > 0 else 0
    return S, W, steps, -(-steps // G)


def coeffs(sr):
    """The ten K-weighting coefficients by the formulas of the header, in numpy."""
    f0, gain, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = np.power(10.0, gain / 20.0)
    Vb = np.power(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def steps(w, sr, k, first_group=0, ngroups=None):
    """The records of the steps of groups [first_group, first_group + ngroups) (None: to the end) -> STEP_DTYPE array.  k: the
    ten coefficients.  Vectorised across the groups, a loop over the W + G*S samples of a group."""
    x = np.asarray(w, dtype=np.float32)
    n = len(x)
    S, W, nsteps, groups = geometry(n, sr)
    ngroups = groups - first_group if ngroups is None else ngroups
    lo, hi = G * first_group, min(G * (first_group + ngroups), nsteps)
    if ngroups <= 0 or hi <= lo:
        return np.zeros(0, dtype=STEP_DTYPE)
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (np.float64(v) for v in k)
    gstart = (first_group + np.arange(ngroups, dtype=np.int64)) * (G * S)
    xp = np.concatenate([np.zeros(W, np.float32), x, np.zeros(G * S, np.float32)])  # xp[i + W] = x_i, zeros before the file
    s1, s2, t1, t2 = (np.zeros(ngroups) for _ in range(4))
    energy, peak = np.zeros((ngroups, G)), np.zeros((ngroups, G), dtype=np.float32)
    with np.errstate(all="ignore"):
        for t in range(W + G * S):
            x32 = xp[gstart + t]
            v = x32.astype(np.float64)
            y = b0 * v + s1
            s1 = (b1 * v - a1 * y) + s2
            s2 = b2 * v - a2 * y
            z = c0 * y + t1
            t1 = (c1 * y - d1 * z) + t2
            t2 = c2 * y - d2 * z
            if t < W:
                continue
            step = (t - W) // S
            live = gstart + (t - W) < n  # samples at or beyond n are not visited
            energy[:, step] = np.where(live, energy[:, step] + z * z, energy[:, step])
            m = np.abs(x32)
            peak[:, step] = np.where(live & (m > peak[:, step]), m, peak[:, step])
    out = np.zeros(hi - lo, dtype=STEP_DTYPE)
    out["energy"] = energy.reshape(-1)[:hi - lo]
    out["peak"] = peak.reshape(-1)[:hi - lo]
    out["samples"] = np.minimum(S, n - (lo + np.arange(hi - lo, dtype=np.int64)) * S)
    return out


def _lufs(mean_square):
    return OFFSET + 10.0 * (math.log10(mean_square) if mean_square > 0 else -math.inf if mean_square == 0 else math.nan)


def _sum(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


def curve(st, sr, window):
    S = geometry(0, sr)[0]
    out, full = np.full(len(st), -np.inf), 0
    for b in range(len(st)):
        full = full + 1 if st["samples"][b] == S else 0
        if full >= window:
            out[b] = _lufs(_sum(st["energy"][b - window + 1:b + 1]) / float(window * S))
    return out


def _curve_max(st, sr, window):
    m = -math.inf
    for v in curve(st, sr, window):
        if v > m:
            m = float(v)
    return m


def integrated(st, sr):
    """-> dict of mx_loudness' fields"""
    S = geometry(0, sr)[0]
    z, blocks, bad = [], 0, 0
    j = 0
    while 10 * j + 40 <= len(st):
        if np.all(st["samples"][10 * j:10 * j + 40] == S):
            blocks += 1
            zj = _sum(st["energy"][10 * j:10 * j + 40]) / float(40 * S)
            if math.isfinite(zj):
                z.append(zj)
            else:
                bad += 1
        j += 1
    gated = [v for v in z if v > ABS_GATE]
    value, passed = -math.inf, []
    if gated:
        gate = 0.1 * (_sum(gated) / float(len(gated)))
        passed = [v for v in gated if v > gate]
        value = _lufs(_sum(passed) / float(len(passed)))
    return {"integrated": value, "momentary_max": _curve_max(st, sr, 40), "shortterm_max": _curve_max(st, sr, 300),
            "peak": float(np.max(st["peak"])) if len(st) else 0.0, "blocks": blocks, "passed_abs": len(gated), "passed_rel": len(passed),
            "bad_blocks": bad}


def note_loudness(st, sr, notes):
    """notes: records or tuples whose first two values are start_sample, end_sample -> float64[nnotes]"""
    S = geometry(0, sr)[0]
    out = np.zeros(len(notes))
    for i, note in enumerate(notes):
        start, end = int(note[0]), int(note[1])
        lo, hi = -(-start // S), min((end + 1) // S, len(st))
        if hi <= lo:
            lo = ((start + end) // 2) // S
            hi = lo + 1
        e = st["energy"][lo:hi]
        out[i] = _lufs(_sum(e) / float(int(np.sum(st["samples"][lo:hi])))) if np.all(np.isfinite(e)) else math.nan
    return out


def level_gain_points(notes, lufs, **params):
    """-> ([(sample, amp f32)] * 2 per note, reference).  params: `raise` (also raise_), lower, max_db."""
    p = dict(LEVEL_DEFAULTS, **{k.rstrip("_"): v for k, v in params.items()})
    finite = sorted(float(v) for v in lufs if math.isfinite(v))
    k = len(finite)
    ref = math.nan if k == 0 else finite[k // 2] if k % 2 else (finite[k // 2 - 1] + finite[k // 2]) / 2.0
    out = []
    for note, v in zip(notes, lufs):
        amp = np.float32(1.0)
        if math.isfinite(v):
            d = ref - float(v)
            db = (p["raise"] if d > 0.0 else p["lower"]) * d
            db = min(max(db, -p["max_db"]), p["max_db"])
            amp = np.float32(math.pow(10.0, db / 20.0))
        out += [(int(note[0]), amp), (int(note[1]), amp)]
    return out, ref


def normalize_gain(m, target_lufs=-23.0, ceiling_db=-1.0):
    return np.float32(min(math.pow(10.0, (target_lufs - m["integrated"]) / 20.0),
                          math.pow(10.0, ceiling_db / 20.0) / float(np.float32(m["peak"]))))


# ---- the synthetic takes ----
def tone(sr, hz, amp, seconds, phase=0.0):
    i = np.arange(int(round(seconds * sr)), dtype=np.float64)
    return (amp * np.sin(2 * np.pi * hz * i / sr + phase)).astype(np.float32)


def dbfs(db):
    return 10.0 ** (db / 20.0)


def noise(n, seed=1770, amp=0.25):
    """uniform PCG64 noise in [-amp, amp)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def gated_take(sr=48000):
    """2 s at -33 dBFS, 4 s at -20 dBFS, 2 s at -33 dBFS of 1 kHz: the quiet blocks pass the absolute gate and fall to the
    relative one."""
    return np.concatenate([tone(sr, 1000.0, dbfs(-33.0), 2.0), tone(sr, 1000.0, dbfs(-20.0), 4.0), tone(sr, 1000.0, dbfs(-33.0), 2.0)])


LEVEL_SR = 48000
LEVEL_NOTES = ((0.5, 150.0), (0.06, 180.0), (0.25, 130.0), (0.12, 200.0), (0.5, 165.0))  # (amplitude, f0 Hz)
LEVEL_NOTE_S, LEVEL_GAP_S = 0.40, 0.10


@functools.lru_cache(maxsize=None)
def _levelling_take():
    sr, parts, truth, at = LEVEL_SR, [], [], 0
    ramp, gap = int(0.01 * sr), int(LEVEL_GAP_S * sr)
    for amp, f0 in LEVEL_NOTES:
        n = int(LEVEL_NOTE_S * sr)
        e = np.ones(n)
        e[:ramp], e[-ramp:] = np.linspace(0, 1, ramp), np.linspace(1, 0, ramp)
        parts += [np.zeros(gap), SIB._vowel(n, f0, sr, amp) * e]
        truth.append((at + gap, at + gap + n))
        at += gap + n
    parts.append(np.zeros(gap))
    w = np.concatenate(parts).astype(np.float32)
    w.setflags(write=False)
    return w, tuple(truth)


def levelling_take():
    """Five sung-vowel notes (sibilant_ref's harmonic vowel) at amplitudes 0.5 / 0.06 / 0.25 / 0.12 / 0.5 under 10 ms ramps,
    100 ms of silence around each, at 48 kHz -> (float32 samples (read-only), [(first sample, one past the last)] per note)."""
    return _levelling_take()


def level_chain(w, sr, k, notes, **params):
    """The levelling chain on the CPU: records, note loudness, points, the gained take, its records and note loudness ->
    dict(steps, lufs, points, reference, levelled, steps_after, lufs_after)."""
    st = steps(w, sr, k)
    lufs = note_loudness(st, sr, notes)
    points, ref = level_gain_points(notes, lufs, **params)
    levelled = SIB.apply_gain(w, points)
    after = steps(levelled, sr, k)
    return dict(steps=st, lufs=lufs, points=points, reference=ref, levelled=levelled, steps_after=after,
                lufs_after=note_loudness(after, sr, notes))


def spread(lufs):
    return float(np.max(lufs) - np.min(lufs))
