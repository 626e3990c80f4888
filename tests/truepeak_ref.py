"""True peak, limiter and loudness range of include/melonix_amd.h ("True peak, limiter and loudness range"), restated in numpy:
peaks(), records() and limit() are the definition the kernels must equal byte for byte, given the library's own tap table
(mx_true_peak_taps; tap_formula() is what a CPU test holds that table against); loudness_range() and normalize_gain_tp() repeat
the host logic expression by expression.  Plus the four synthetic takes of the limiter and the chain of the export."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import loudness_ref as L
import pcm_extremes as PCM
import sibilant_ref as SIB

STEP_DTYPE = np.dtype([("true_peak", "<f4"), ("sample_peak", "<f4")])
TAPS, BEFORE, AFTER = 12, 5, 6
UNITY = 1 << 30
MAX_LOOKAHEAD = 1024
MINUS_1_DBTP = np.float32(10.0 ** (-1.0 / 20.0))


def step_samples(sr):
    return (sr + 50) // 100


def oversampling(sr):
    return 4 if sr < 88200 else 2 if sr < 176400 else 1


def default_lookahead(sr):
    return min(MAX_LOOKAHEAD, (sr + 100) // 200)


def tap_formula():
    """c_u[d] for u = 1/4, 1/2, 3/4 and d = -5 .. 6 by the header's formula in binary64 -> float64[3, 12] (not yet rounded)."""
    out = np.zeros((3, TAPS))
    for r, u in enumerate((0.25, 0.5, 0.75)):
        for k in range(TAPS):
            v = (k - BEFORE) - u
            out[r, k] = math.sin(math.pi * v) / (math.pi * v) * (0.42 + 0.5 * math.cos(math.pi * v / 6.0) + 0.08 * math.cos(2.0 * math.pi * v / 6.0))
    return out


def library_taps():
    """The library's table (no device needed) -> float32[3, 12]"""
    import melonix_amd
    return melonix_amd.true_peak_taps()


def peaks(w, sr, taps):
    """p_i of every sample -> float32[n].  Binary32: each product rounded, then added, d ascending, from +0."""
    x = np.asarray(w, dtype=np.float32)
    n = len(x)
    xp = np.concatenate([np.zeros(BEFORE, np.float32), x, np.zeros(AFTER, np.float32)])  # xp[i + 5 + d] = x_{i + d}
    taps = np.asarray(taps, dtype=np.float32)
    with np.errstate(all="ignore"):
        p = np.where(np.isnan(x), np.float32(0), np.abs(x)).astype(np.float32)
        for row in {4: (0, 1, 2), 2: (1,), 1: ()}[oversampling(sr)]:
            y = np.zeros(n, dtype=np.float32)
            for k in range(TAPS):
                y = y + xp[k:k + n] * taps[row, k]
            a = np.abs(y)
            p = np.where(a > p, a, p)  # (a NaN compares false)
    assert p.dtype == np.float32
    return p


def records(w, sr, taps, first_step=0, nsteps=None):
    """The records of steps [first_step, first_step + nsteps) (None: to the end) -> STEP_DTYPE array."""
    x = np.asarray(w, dtype=np.float32)
    n, S = len(x), step_samples(sr)
    steps = -(-n // S) if n > 0 else 0
    nsteps = steps - first_step if nsteps is None else nsteps
    out = np.zeros(max(nsteps, 0), dtype=STEP_DTYPE)
    if nsteps <= 0:
        return out
    p = peaks(x, sr, taps)
    mag = np.where(np.isnan(x), np.float32(0), np.abs(x)).astype(np.float32)
    starts = (first_step + np.arange(nsteps)) * S
    hi = min((first_step + nsteps) * S, n)
    out["true_peak"] = np.maximum.reduceat(p[:hi], starts)
    out["sample_peak"] = np.maximum.reduceat(mag[:hi], starts)
    return out


def required_gain(p, c):
    """q in Q30 -> int64 array"""
    with np.errstate(all="ignore"):
        quotient = np.floor((np.float64(np.float32(c)) / p.astype(np.float64)) * 1073741824.0)
    over = p > np.float32(c)
    return np.where(over, quotient, float(UNITY)).astype(np.int64)


def gains(w, sr, taps, c, A):
    """s_i, the sums of A + 1 window minima -> int64[n]"""
    x = np.asarray(w, dtype=np.float32)
    n = len(x)
    q = required_gain(peaks(x, sr, taps), c)
    qp = np.concatenate([np.full(A, UNITY, np.int64), q, np.full(A, UNITY, np.int64)])  # qp[j + A] = q_j
    m = sliding_window_view(qp, A + 1).min(axis=1)  # m[t + A] = min q[t .. t + A], t = -A .. n - 1
    cs = np.concatenate([np.zeros(1, np.int64), np.cumsum(m, dtype=np.int64)])  # cs[k] = m_{-A} + .. + m_{-A + k - 1}
    i = np.arange(n)
    return cs[i + A + 1] - cs[i]  # t = i - A .. i


def limit(w, sr, taps, c, A):
    """-> (out float32[n], pcm int16[n])"""
    x = np.asarray(w, dtype=np.float32)
    s = gains(x, sr, taps, c, A)
    with np.errstate(all="ignore"):
        g = s.astype(np.float64) / float((A + 1) << 30)
        out = (x.astype(np.float64) * g).astype(np.float32)
    return out, PCM.clamped_i16(out)


def measure(rec):
    """-> (true peak, sample peak) of a take's records: the largest of each (never NaN)"""
    return (np.float32(rec["true_peak"].max(initial=0.0)), np.float32(rec["sample_peak"].max(initial=0.0)))


def dbtp(amp):
    return 20.0 * math.log10(float(amp)) if amp > 0 else -math.inf


# ---- loudness range and the export gain (host logic) ----
def loudness_range(st, sr):
    """-> dict of mx_loudness_range_result's fields, from loudness_ref.STEP_DTYPE records"""
    S = L.geometry(0, sr)[0]
    z, values, bad, full = [], 0, 0, 0
    for b in range(len(st)):
        full = full + 1 if st["samples"][b] == S else 0
        if b < 299 or (b - 299) % 10 or full < 300:
            continue
        values += 1
        zk = L._sum(st["energy"][b - 299:b + 1]) / float(300 * S)
        if math.isfinite(zk):
            z.append(zk)
        else:
            bad += 1
    gated = [v for v in z if v > L.ABS_GATE]
    kept = []
    if gated:
        gate = 0.01 * (L._sum(gated) / float(len(gated)))
        kept = sorted(v for v in gated if v > gate)
    out = {"lra": 0.0, "low_lufs": -math.inf, "high_lufs": -math.inf, "values": values, "gated": len(kept), "bad": bad}
    if kept:
        low = kept[int(math.floor((len(kept) - 1) * 0.10 + 0.5))]
        high = kept[int(math.floor((len(kept) - 1) * 0.95 + 0.5))]
        out.update(lra=10.0 * math.log10(high / low), low_lufs=L._lufs(low), high_lufs=L._lufs(high))
    return out


def normalize_gain_tp(m, true_peak, target_lufs=-23.0, ceiling_dbtp=-1.0):
    return np.float32(min(math.pow(10.0, (target_lufs - m["integrated"]) / 20.0),
                          math.pow(10.0, ceiling_dbtp / 20.0) / float(np.float32(true_peak))))


# ---- the synthetic takes ----
CLICKS = (0, 3, 2047, 2048, 2049, 4096, 9999)  # and n - 1


def vowel(n, sr=48000):
    """a swelling 150 Hz vowel (sibilant_ref's harmonic vowel) that peaks at 1.4"""
    v = SIB._vowel(max(n, 64), 150.0, sr, 1.0)[:n].astype(np.float64)  # (a single sample of it is 0: nothing to normalise)
    v *= np.sin(np.pi * (np.arange(n) + 0.5) / n) ** 2
    return (v * (1.4 / max(np.abs(v).max(), 1e-30))).astype(np.float32)


def quarter_tone(n, amp=1.3):
    """fs/4 at 45 degrees: every sample +-amp / sqrt 2, the waveform reaches amp"""
    return (amp * np.sin(np.pi / 2.0 * np.arange(n) + np.pi / 4.0)).astype(np.float32)


def noise(n, rms, seed=3341):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rms * rng.standard_normal(n)).astype(np.float32)


def clicks(n, seed=3342):
    """noise at 0.05 rms with clicks of 1.1 .. 2.5, alternating in sign, at CLICKS and n - 1 (those inside the take)"""
    w = noise(n, 0.05, seed)
    at = sorted({s for s in CLICKS + (n - 1,) if 0 <= s < n})
    for k, s in enumerate(at):
        w[s] = np.float32((1.1 + 1.4 * k / max(len(at) - 1, 1)) * (-1.0) ** k)
    return w


SIGNALS = {"vowel": vowel, "tone": quarter_tone, "noise": lambda n: noise(n, 0.5), "clicks": clicks}


def sparse_clicks(n, seed):
    """noise (loudness_ref's, +-0.25) with a click of 0.9 every 4099 samples: the records' take"""
    w = L.noise(n, seed=seed)
    w[::4099] = np.float32(0.9) * np.where(np.arange(len(w[::4099])) % 2, np.float32(-1), np.float32(1))
    return w


def export_chain(w, sr, k, taps, target_lufs=-16.0, c=MINUS_1_DBTP, A=None):
    """measure -> gain to target_lufs (mx_normalize_gain_tp without its ceiling term: the limiter holds the ceiling) -> limit ->
    measure again, on the CPU -> dict.  k: the library's K-weighting coefficients."""
    A = default_lookahead(sr) if A is None else A
    x = np.asarray(w, dtype=np.float32)
    before = L.integrated(L.steps(x, sr, k), sr)
    tp_before = measure(records(x, sr, taps))
    amp = np.float32(math.pow(10.0, (target_lufs - before["integrated"]) / 20.0))
    gained = SIB.apply_gain(x, [(0, amp)])
    out, pcm = limit(gained, sr, taps, c, A)
    after = L.integrated(L.steps(out, sr, k), sr)
    tp_after = measure(records(out, sr, taps))
    return dict(before=before, tp_before=tp_before, amp=amp, gained=gained, out=out, pcm=pcm, after=after, tp_after=tp_after)
