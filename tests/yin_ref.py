"""Float64 restatement of the build-defined YIN f0 tracker, notes and correction markers (definition:
include/melonix_amd.h, f0_kernels.hip).  Test-side only: the product never imports it.

track()          d through float64 FFTs and prefix sums (cross-checked against the literal double sum of step 1 by the
                 CPU suite); also returns d' so that the GPU tests can tell near-ties from disagreements
check_parity()   the GPU tests' comparison of a kernel track with track()'s
pcm16(), exact_scales()  test signals for the scale property (2^k x exact in f32)
detect_notes()   the same loop as f0_notes.cpp, in the same order of float64 operations (math.log2 = the C library's
                 log2): notes come out with equal doubles
correction_markers()
"""
from __future__ import annotations

import math

import numpy as np

N, W = 4096, 2048
SILENT = (0, 0.0, 1.0, 0.0)


def frames_of(w, hop, first, count):
    """x[f] = audio[(first+f)*hop - W + j], j < N, zeros outside the file (float64)."""
    w = np.asarray(w, dtype=np.float64)
    pad = np.concatenate([np.zeros(W), w, np.zeros(N + hop)])
    idx = (np.arange(first, first + count, dtype=np.int64) * hop)[:, None] + np.arange(N)[None, :]
    return pad[idx]


def tau_range(sr, fmin=55.0, fmax=1760.0):
    fmin, fmax = float(np.float32(fmin)), float(np.float32(fmax))
    return max(2, math.floor(sr / fmax)), min(W - 1, math.ceil(sr / fmin))


def diff_fft(x):
    """d(tau), tau = 0..W, per row of x (F x N): e0 + e_tau - 2 r(tau), clamped to >= 0."""
    a = np.zeros_like(x)
    a[:, :W] = x[:, :W]
    r = np.fft.irfft(np.conj(np.fft.rfft(a, axis=1)) * np.fft.rfft(x, axis=1), n=N, axis=1)[:, :W + 1]
    S = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(x * x, axis=1)], axis=1)
    tau = np.arange(W + 1)
    e = S[:, tau + W] - S[:, tau]
    return np.maximum(S[:, W:W + 1] + e - 2 * r, 0.0)


def diff_direct(x):
    """Step 1 literally: sum_{j<W} (x_j - x_{j+tau})^2 in double (one row)."""
    return np.array([float(np.sum((x[:W] - x[t:t + W]) ** 2)) for t in range(W + 1)])


def cmnd(d):
    """d'(tau): d(0)' = 1, d(tau) tau / sum_{j=1..tau} d(j), 1 where that sum is 0."""
    cs = np.cumsum(d[:, 1:], axis=1)
    tau = np.arange(1, W + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dp = np.where(cs == 0, 1.0, d[:, 1:] * tau / np.where(cs == 0, 1.0, cs))
    return np.concatenate([np.ones((d.shape[0], 1)), dp], axis=1)


def descend(dp_row, t, tmax):
    """Step 4's descent: forward from t while t+1 <= tmax and d'(t+1) < d'(t)."""
    while t + 1 <= tmax and dp_row[t + 1] < dp_row[t]:
        t += 1
    return t


def under(dp_row, tmin, tmax, theta):
    """Step 4 without the fallback: the end of the descent from the first tau in range with d' < theta, or 0 for none."""
    hit = np.nonzero(dp_row[tmin:tmax + 1] < theta)[0]
    return descend(dp_row, tmin + int(hit[0]), tmax) if len(hit) else 0


def pick(dp_row, tmin, tmax, theta):
    return under(dp_row, tmin, tmax, theta) or tmin + int(np.argmin(dp_row[tmin:tmax + 1]))


def refine(d_row, t):
    """Step 5: t + the clamped parabolic offset on d at t-1, t, t+1."""
    dm, d0, dq = d_row[t - 1], d_row[t], d_row[t + 1]
    den = 2 * (dm - 2 * d0 + dq)
    delta = (dm - dq) / den if den > 0 else 0.0
    return t + min(0.5, max(-0.5, delta))


def frame_chunks(w, hop, first, count, chunk):
    """The frames [first, first + count) in chunks: (c0, x, d, d') per chunk, c0 the chunk's first row."""
    for c0 in range(0, count, chunk):
        x = frames_of(w, hop, first + c0, min(chunk, count - c0))
        with np.errstate(invalid="ignore", over="ignore"):
            d = diff_fft(x)
            dp = cmnd(d)
        yield c0, x, d, dp


def default_count(n, hop, first, count):
    return -(-n // hop) - first if count is None else count


def track(w, sr, hop=256, first=0, count=None, fmin=55.0, fmax=1760.0, threshold=0.15, chunk=2048):
    """-> (records: list of (tau, period, aperiodicity, rms), dp: F x (W+1) d' rows, or None when not kept)."""
    tmin, tmax = tau_range(sr, fmin, fmax)
    theta = float(np.float32(threshold))
    recs, dps = [], []
    for _, x, d, dp in frame_chunks(w, hop, first, default_count(len(w), hop, first, count), chunk):
        dps.append(dp)
        rms = np.sqrt(np.sum(x * x, axis=1) / N)
        for i in range(x.shape[0]):
            if rms[i] == 0:
                recs.append(SILENT)
                continue
            t = pick(dp[i], tmin, tmax, theta)
            recs.append((t, refine(d[i], t), dp[i, t], rms[i]))
    return recs, np.concatenate(dps) if dps else np.zeros((0, W + 1))


def near_ties(dp, taus, tmin, tmax, theta, eps_theta=1e-4, eps_cmp=1e-4):
    """Frames whose decision a perturbation of d' could change: d' within eps_theta of theta at some tau <= tau*, or within
    eps_cmp of d'(tau*) at a competing candidate — tau*'s neighbours (the end of the descent) or, where nothing is under
    theta, any tau of the range (the argmin)."""
    out = np.zeros(len(taus), dtype=bool)
    for i, t in enumerate(taus):
        row = dp[i]
        if t <= 0:
            continue
        seg = row[tmin:t + 1]
        if np.any(np.abs(seg - theta) < eps_theta):
            out[i] = True
            continue
        if row[t] < theta:
            nb = [row[t - 1]] if t - 1 >= tmin else []
            if t + 1 <= tmax:
                nb.append(row[t + 1])
            out[i] = any(abs(v - row[t]) < eps_cmp for v in nb)
        else:
            others = np.delete(row[tmin:tmax + 1], t - tmin)
            out[i] = bool(np.any(np.abs(others - row[t]) < eps_cmp))
    return out


def pcm16(w):
    """w rounded to 16-bit PCM values m / 32768 (f32)."""
    return (np.round(np.asarray(w, np.float64) * 32768.0) / 32768.0).astype(np.float32)


def exact_scales(w, lo=-160, hi=140):
    """The k in [lo, hi) for which 2^k w is exact in f32 (finite, and scales back to w)."""
    ks = []
    with np.errstate(over="ignore", under="ignore"):
        for k in range(lo, hi):
            y = np.ldexp(w, k)
            if np.isfinite(y).all() and (np.ldexp(y, -k) == w).all():
                ks.append(k)
    return ks


REC_DTYPE = [("tau", "<i4"), ("period", "<f8"), ("aperiodicity", "<f8"), ("rms", "<f8")]
FLT_MIN = 2.0 ** -126


def check_parity(got, recs, dp, tmin, tmax, theta, label, eps=1e-4, cents=1.0, ap_abs=1e-4, ap_rel=1e-3, rms_rel=1e-5,
                 rms_floor=1e-30, rms_sub_abs=0.0, check_excused=False):
    """Asserts a kernel track (F0_DTYPE) against track()'s (recs, dp) and prints one summary line.  Silent frames are
    the reference's (rms == 0) and no others; tau is equal except on near-ties (eps: near_ties' eps_theta and eps_cmp);
    where it is equal the period is within `cents` and the aperiodicity within ap_abs + ap_rel * ref; rms is within
    rms_rel relative to max(ref, rms_floor), plus rms_sub_abs absolute where the reference's rms is below FLT_MIN (the f32
    field cannot hold more there).  check_excused: a frame excused as a near-tie must be one the reference's own d'
    nearly supports: the kernel's tau lies in range and its d' is within eps of the reference's d'(tau*), or d' is within
    eps of theta at some tau up to the later of the two.  -> (frames, frames whose tau differs on an excused near-tie)."""
    ref = np.array(recs, dtype=REC_DTYPE)
    assert len(got) == len(ref), label
    silent = ref["rms"] == 0
    loud = ~silent
    assert (got["tau"][silent] == 0).all() and (got["period"][silent] == 0).all(), label
    assert (got["aperiodicity"][silent] == 1).all() and (got["rms"][silent] == 0).all(), label
    assert (got["tau"][loud] > 0).all(), f"{label}: frames reported silent {np.nonzero(loud & (got['tau'] == 0))[0][:10]}"
    ties = near_ties(dp, ref["tau"], tmin, tmax, theta, eps_theta=eps, eps_cmp=eps)
    same = got["tau"] == ref["tau"]
    bad = ~same & ~ties
    excused = ~same & ties
    ap_err = np.abs(got["aperiodicity"] - ref["aperiodicity"])[same & loud]
    rms_err = np.abs(got["rms"] - ref["rms"])[loud]
    rms_den = np.maximum(ref["rms"], rms_floor)[loud]
    rms_rel_err = rms_err / rms_den
    c = np.abs(1200 * np.log2(got["period"][same & loud] / ref["period"][same & loud]))
    print(f"f0 parity {label}: {len(got)} frames, tau differs on {int((~same).sum())} "
          f"(near-tie frames {int(ties.sum())}), "
          f"period max {c.max() if len(c) else 0:.3g} cents, aperiodicity max err {ap_err.max() if len(ap_err) else 0:.2e}, "
          f"rms max rel {rms_rel_err.max() if len(rms_rel_err) else 0:.2e}")
    assert not bad.any(), f"{label}: tau differs outside near-ties at frames {np.nonzero(bad)[0][:10]}"
    if check_excused:
        for i in np.nonzero(excused)[0]:
            g, t, row = int(got["tau"][i]), int(ref["tau"][i]), dp[i]
            assert tmin <= g <= tmax and (abs(row[g] - row[t]) < eps
                                          or np.any(np.abs(row[tmin:max(g, t) + 1] - theta) < eps)), \
                f"{label}: frame {i} tau {g} (d' {row[g]:.6g}) against the reference's {t} (d' {row[t]:.6g})"
    assert (c <= cents).all(), label
    assert (ap_err <= ap_abs + ap_rel * ref["aperiodicity"][same & loud]).all(), label
    slack = np.where(ref["rms"] < FLT_MIN, rms_sub_abs, 0.0)[loud]
    assert (rms_rel_err <= rms_rel + slack / rms_den).all(), label
    return len(got), int(excused.sum())


# ---- notes and markers (host definitions, same float64 operations as f0_notes.cpp) ----
def period_note(period, sr):
    return 24.0 + 12.0 * math.log2(float(sr) / float(period) / 55.0)


def _median(vals):
    s = sorted(vals)
    k = len(s)
    return s[k // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) / 2.0


DEFAULT_PARAMS = dict(threshold=0.15, rms_floor=1e-3, max_jump=0.5, max_dev=0.75, min_frames=8)


def detect_notes(track, sr, hop, first=0, **params):
    """track: records with fields tau, period, aperiodicity, rms (float32 values).  -> list of tuples
    (start_sample, end_sample, first_frame, frames, note, aperiodicity (f32), spread (f32))."""
    p = dict(DEFAULT_PARAMS, **params)
    thr, floor = float(np.float32(p["threshold"])), float(np.float32(p["rms_floor"]))
    out, run, m = [], [], {}

    def close():
        if len(run) >= p["min_frames"]:
            note = _median([m[f] for f in run])
            ap, spread = 0.0, 0.0
            for f in run:
                ap += float(track[f]["aperiodicity"])
                spread = max(spread, abs(m[f] - note))
            s, e = run[0], run[-1]
            out.append(((first + s) * hop, (first + e) * hop, first + s, len(run), note,
                        float(np.float32(ap / len(run))), float(np.float32(spread))))
        run.clear()

    for f in range(len(track)):
        r = track[f]
        if not (int(r["tau"]) > 0 and float(r["aperiodicity"]) < thr and float(r["rms"]) >= floor):
            close()
            continue
        m[f] = period_note(float(r["period"]), sr)
        if run and (abs(m[f] - m[f - 1]) > p["max_jump"] or abs(m[f] - _median([m[g] for g in run])) > p["max_dev"]):
            close()
        run.append(f)
    close()
    return out


def snap(note, mask):
    base = math.floor(note)
    best, bestd = None, math.inf
    for k in range(-12, 14):
        c = base + k
        if mask and not (mask >> (c % 12)) & 1:
            continue
        d = abs(c - note)
        if d < bestd:
            best, bestd = float(c), d
    return best


def correction_markers(notes, strength=1.0, scale_mask=0):
    out = []
    for n in notes:
        start, end, note = int(n[0]), int(n[1]), float(n[4])
        b = strength * (snap(note, scale_mask) - note)
        out += [(start, note, 0.0, b), (end, note, 0.0, b)]
    return out
