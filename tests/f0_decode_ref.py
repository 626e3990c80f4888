"""Reference of the build-defined YIN candidate ladder and Viterbi f0 decoder (definition: include/melonix_amd.h,
f0_kernels.hip, f0_decode.hip).  Test-side only: the product never imports it.

ladder()          the four rungs per frame in float64 on yin_ref's d'
decode()          the decoder in Python integers, one frame after the other (the definition, literally)
decode_chunked()  the same path through the chunk scheme of f0_decode.hip: per-chunk min-plus products, one pass over the
                  chunks, a re-walk per chunk; the maps bp the same way backwards.  Integers: equal to decode() for any C
glitch_assertions()  what the decoder must do to GLITCH (the CPU suite on the reference, the GPU suite on the device)
glitch()          the GLITCH signal: a steady 220 Hz voice-like tone with two subharmonic and two second-partial bursts
"""
from __future__ import annotations

import math

import numpy as np

import yin_ref as Y

CANDS = 4
UNVOICED = 4
Q = 65536
INF = 1 << 56
BIG = 1 << 60  # "no path yet" in a chunk product's start row; above every sum of real costs, far from int64's end
RUNGS = (2.0, 1.0, 0.5, 0.25)
CAND_DTYPE = np.dtype([("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("cents", "<i4")])
CAND_REF_DTYPE = np.dtype([("tau", "<i4"), ("period", "<f8"), ("aperiodicity", "<f8"), ("cents", "<i4")])
F0_DTYPE = np.dtype([("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])
DEFAULT_PARAMS = dict(unvoiced_cost=0.3, jump_cost=0.1, switch_cost=0.5, max_jump_cents=1200)
GLITCH_SR, GLITCH_HOP = 48000, 256


def glitch():
    sr, n = GLITCH_SR, 96000
    t = np.arange(n) / sr
    ph = 2 * np.pi * 220 * t

    def b(c):
        return np.exp(-0.5 * ((t - c) / 0.012) ** 2)

    x = np.sin(ph) + 0.5 * np.sin(2 * ph + 0.3) + 0.3 * np.sin(3 * ph + 1.0)
    x = x * (1 + 0.7 * (b(0.5) + b(0.9)) * np.cos(ph / 2)) + 4 * (b(1.3) + b(1.6)) * np.sin(2 * ph + 0.7)
    x = 0.2 * x + 0.01 * np.random.default_rng(1).standard_normal(n)
    return x.astype(np.float32)


def glitch_assertions(plain, decoded, label):
    """CPU test 2 / GPU test 8: the plain track breaks into >= 3 notes; the decoded one is 1 note at 48 with no frame of
    8..F-9 unvoiced or further than 0.5 semitones from 48.  Prints the figures first."""
    sr, hop = GLITCH_SR, GLITCH_HOP
    pn = Y.detect_notes(plain, sr, hop)
    dn = Y.detect_notes(decoded, sr, hop, threshold=0.30)
    F = len(decoded)
    inner = np.arange(8, F - 8)
    off = [f for f in inner if not (decoded["tau"][f] > 0 and abs(Y.period_note(decoded["period"][f], sr) - 48.0) <= 0.5)]
    print(f"GLITCH {label}: plain notes {[round(n[4], 2) for n in pn]}, decoded notes {[round(n[4], 3) for n in dn]}, "
          f"decoded frames off in 8..F-9: {len(off)} of {len(inner)}")
    assert len(pn) >= 3
    assert len(dn) == 1 and abs(dn[0][4] - 48.0) < 0.1
    assert not off


def thetas(threshold):
    """theta_k = threshold x {2, 1, 1/2, 1/4}, formed in f32."""
    th = np.float32(threshold)
    return [float(np.float32(th * np.float32(m))) for m in RUNGS]


def cents_of(period, sr):
    return int(np.rint(1200.0 * math.log2(float(sr) / float(period) / 55.0))) + 2400


def ladder(w, sr, hop=256, first=0, count=None, fmin=55.0, fmax=1760.0, threshold=0.15, chunk=2048):
    """-> (cands: F x 4 CAND_REF_DTYPE, dp: F x (W+1) d' rows, rung_taus: F x 4 — the tau each rung picked before the
    duplicate rule, 0 where the rung is empty (slot 0: the fallback's tau)."""
    count = Y.default_count(len(w), hop, first, count)
    tmin, tmax = Y.tau_range(sr, fmin, fmax)
    th = thetas(threshold)
    cands = np.zeros((count, CANDS), dtype=CAND_REF_DTYPE)
    cands["aperiodicity"] = 1.0
    picked = np.zeros((count, CANDS), dtype=np.int64)
    dps = []
    for c0, x, d, dp in Y.frame_chunks(w, hop, first, count, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            energy = np.sum(x * x, axis=1)
        dps.append(dp)
        for i in range(x.shape[0]):
            if energy[i] == 0:
                continue
            taus = [Y.pick(dp[i], tmin, tmax, th[0])] + [Y.under(dp[i], tmin, tmax, th[k]) for k in range(1, CANDS)]
            picked[c0 + i] = taus
            for k, t in enumerate(taus):
                if t == 0 or t in taus[:k] or not np.isfinite(dp[i, t]):
                    continue
                period = Y.refine(d[i], t)
                cands[c0 + i, k] = (t, period, dp[i, t], cents_of(period, sr))
    return cands, (np.concatenate(dps) if dps else np.zeros((0, Y.W + 1))), picked


def to_f32(cands):
    """The ladder's records in the device's layout (f32 fields)."""
    out = np.zeros(cands.shape, dtype=CAND_DTYPE)
    for k in CAND_DTYPE.names:
        out[k] = cands[k]
    return out


def plain_track(recs):
    """yin_ref.track()'s records as an F0_DTYPE array."""
    return np.array([tuple(r) for r in recs], dtype=F0_DTYPE)


# ---- the decoder, in Python integers ----
def q(x):
    return int(np.rint(float(np.float32(x)) * Q))


def obs_cost(ap):
    """min(q(aperiodicity), 2Q) on the f32 value; at least 0, and 2Q for a NaN (a table from the host may hold anything)."""
    ap = float(np.float32(ap))
    if not ap < 2.0:
        return 2 * Q
    return int(np.rint(ap * Q)) if ap > 0.0 else 0


def _frames(cands, p):
    """Per frame: (filled[4], cents[4], O[5])."""
    qu = q(p["unvoiced_cost"])
    out = []
    for row in cands:
        filled = [int(row["tau"][j]) > 0 for j in range(CANDS)]
        cents = [int(row["cents"][j]) for j in range(CANDS)]
        O = [obs_cost(row["aperiodicity"][j]) if filled[j] else INF for j in range(CANDS)] + [qu]
        out.append((filled, cents, O))
    return out


def _trans(prev, cur, p):
    """T_f(i, j) between frame f-1 (prev) and f (cur); prev None (f = 0): all 0."""
    if prev is None:
        return [[0] * 5 for _ in range(5)]
    qj, qs, mj = q(p["jump_cost"]), q(p["switch_cost"]), int(p["max_jump_cents"])
    T = [[0] * 5 for _ in range(5)]
    for i in range(5):
        for j in range(5):
            if i == UNVOICED and j == UNVOICED:
                T[i][j] = 0
            elif i == UNVOICED or j == UNVOICED:
                T[i][j] = qs
            elif prev[0][i] and cur[0][j]:
                T[i][j] = qj * min(abs(cur[1][j] - prev[1][i]), mj) // 100
    return T


def _step(V, T, O):
    """V_f(j) = min_i (V_{f-1}(i) + T(i, j)) + O(j), bp the lowest i attaining it."""
    Vn, bp = [], []
    for j in range(5):
        best, bi = V[0] + T[0][j], 0
        for i in range(1, 5):
            c = V[i] + T[i][j]
            if c < best:
                best, bi = c, i
        Vn.append(best + O[j])
        bp.append(bi)
    return Vn, bp


def _records(track, cands, state):
    """The output records (field copies: every bit of the chosen slot and of track's rms)."""
    state = np.asarray(state, np.uint8)
    out = np.zeros(len(state), dtype=F0_DTYPE)
    out["aperiodicity"] = 1.0
    out["rms"] = track["rms"]
    v = np.nonzero(state != UNVOICED)[0]
    for k in ("tau", "period", "aperiodicity"):
        out[k][v] = cands[k][v, state[v]]
    return out


def _params(p):
    return dict(DEFAULT_PARAMS, **(p or {}))


def decode(track, cands, params=None):
    """-> (state: uint8 per frame, out: F0_DTYPE)."""
    p = _params(params)
    fr = _frames(cands, p)
    F = len(fr)
    if F == 0:
        return np.zeros(0, np.uint8), np.zeros(0, F0_DTYPE)
    V = [0] * 5
    bps = []
    for f in range(F):
        V, bp = _step(V, _trans(fr[f - 1] if f else None, fr[f], p), fr[f][2])
        bps.append(bp)
    s = V.index(min(V))
    state = np.zeros(F, np.uint8)
    for f in range(F - 1, -1, -1):
        state[f] = s
        s = bps[f][s]
    return state, _records(track, cands, state)


def decode_chunked(track, cands, C, params=None):
    """decode() through chunks of C frames, the way f0_decode.hip walks them."""
    p = _params(params)
    fr = _frames(cands, p)
    F = len(fr)
    if F == 0:
        return np.zeros(0, np.uint8), np.zeros(0, F0_DTYPE)
    chunks = [(a, min(a + C, F)) for a in range(0, F, C)]

    def walk(V, a, b, keep=None):
        for f in range(a, b):
            V, bp = _step(V, _trans(fr[f - 1] if f else None, fr[f], p), fr[f][2])
            if keep is not None:
                keep.append(bp)
        return V

    # 1. each chunk's product, row by row: the walk from the unit row e_i
    prods = [[walk([0 if k == i else BIG for k in range(5)], a, b) for i in range(5)] for a, b in chunks]
    # 2. V before every chunk's first frame (before frame 0: zeros; T_0 = 0)
    starts, V = [], [0] * 5
    for P in prods:
        starts.append(V)
        V = [min(V[i] + P[i][j] for i in range(5)) for j in range(5)]
    # 3. the re-walk: bp rows, each chunk's map (state at its last frame -> state before its first) and the last V
    bps, maps = [], []
    for (a, b), V0 in zip(chunks, starts):
        keep = []
        Vend = walk(V0, a, b, keep)
        m = list(range(5))
        for bp in keep:
            m = [m[bp[j]] for j in range(5)]
        bps += keep
        maps.append(m)
    assert Vend == V
    # 4. the state at every chunk's last frame, from the end
    s = Vend.index(min(Vend))
    ends = [0] * len(chunks)
    for c in range(len(chunks) - 1, -1, -1):
        ends[c] = s
        s = maps[c][s]
    # 5. the path inside each chunk
    state = np.zeros(F, np.uint8)
    for (a, b), s in zip(chunks, ends):
        for f in range(b - 1, a - 1, -1):
            state[f] = s
            s = bps[f][s]
    return state, _records(track, cands, state)


def random_table(rng, F, p_empty=0.3, stretches=((5, 9),)):
    """A candidate table with random empty slots, some wholly empty frames and the all-empty stretches [a, b) given."""
    c = np.zeros((F, CANDS), dtype=CAND_DTYPE)
    c["tau"] = rng.integers(20, 900, (F, CANDS))
    c["period"] = c["tau"] + rng.uniform(-0.5, 0.5, (F, CANDS)).astype(np.float32)
    # many small aperiodicities and some above the 2Q cap; cents: a slow walk, the slots octaves and a fifth around it
    c["aperiodicity"] = (2.5 * rng.random((F, CANDS)) ** 3).astype(np.float32)
    walk = 4800 + np.cumsum(rng.integers(-30, 31, F))
    c["cents"] = walk[:, None] + rng.choice([0, 0, 1200, -1200, 700], (F, CANDS)) + rng.integers(-20, 21, (F, CANDS))
    empty = rng.random((F, CANDS)) < p_empty
    empty[rng.random(F) < 0.1] = True
    for a, b in stretches:
        empty[a:b] = True
    c[empty] = (0, 0.0, 1.0, 0)
    tr = np.zeros(F, dtype=F0_DTYPE)
    tr["rms"] = rng.uniform(0.0, 1.0, F).astype(np.float32)
    tr["tau"] = c["tau"][:, 0]
    tr["period"] = c["period"][:, 0]
    tr["aperiodicity"] = c["aperiodicity"][:, 0]
    return tr, c
