"""The dynamics compressor of include/melonix_amd.h ("Dynamics compressor") restated in numpy, binary64 and Python integers: the
plan, the curve, the peaks, the targets, the branching one-pole with its truncated warm-up (and without it), the interpolated
product and the final quotient; the takes of the tests; and check_laws, which holds an implementation — the CPU emulation or the
device — to the laws the header states.  Shares no code with the library."""
import math

import numpy as np

ONE, FULL, GC, MAX_WARM, CURVE = 1 << 30, 1 << 24, 4096, 32768, 2049
BASE = (127 - 24) << 23
RATES = (48000, 44100, 8000, 384000, 96000)
FIELDS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "lookahead_ms", "makeup_amp")
DEFAULTS = dict(zip(FIELDS, (-18.0, 4.0, 6.0, 5.0, 100.0, 0.0, 1.0)))
RANGES = dict(zip(FIELDS, ((-60.0, 0.0), (1.0, 100.0), (0.0, 24.0), (0.0, 500.0), (0.0, 2000.0), (0.0, 20.0), (1.0 / 16, 16.0))))


def params(**over):
    """the defaults with `over`, every value as the binary32 the library reads"""
    assert set(over) <= set(FIELDS), over
    return {k: float(np.float32(over.get(k, DEFAULTS[k]))) for k in FIELDS}


def step_samples(sr):
    return (sr + 500) // 1000


def steps(n, sr):
    return -(-n // step_samples(sr))


def coefficient(D, sr, ms):
    if ms <= 0:
        return FULL
    return max(1, min(FULL, math.floor((1.0 - math.exp(-D / (sr * (ms / 1000.0)))) * FULL + 0.5)))


def plan(sr, p):
    D = step_samples(sr)
    ca, cr = coefficient(D, sr, p["attack_ms"]), coefficient(D, sr, p["release_ms"])
    return {"D": D, "K": math.floor(p["lookahead_ms"] * sr / (1000.0 * D) + 0.5), "c_att": ca, "c_rel": cr,
            "W": min(MAX_WARM, 16 * -(-FULL // min(ca, cr))), "Gc": GC}


def gain_db(level_db, p):
    """the static curve in dB, binary64"""
    o, knee, s = level_db - p["threshold_db"], p["knee_db"], 1.0 / p["ratio"] - 1.0
    if 2.0 * o <= -knee:
        return 0.0
    if abs(2.0 * o) < knee:
        return s * (o + knee / 2.0) ** 2 / (2.0 * knee)
    return s * o


def curve(p):
    T = np.empty(CURVE, dtype=np.int64)
    for j in range(CURVE):
        level = float(np.array([BASE + (j << 17)], dtype=np.uint32).view(np.float32)[0])
        T[j] = min(ONE, math.floor(10.0 ** (gain_db(20.0 * math.log10(level), p) / 20.0) * ONE))
    return np.minimum.accumulate(T)


def knee_floor(p):
    """the amplitude one table interval below the knee's lower edge: every level at or below it asks for unity (the table's
    entries lie 1/64 of their octave apart, and the entry above the edge pulls the interpolation between them below unity)"""
    return 10.0 ** ((p["threshold_db"] - p["knee_db"] / 2.0) / 20.0) / (1.0 + 1.0 / 64.0)


def peaks(x, D):
    x = np.asarray(x, dtype=np.float32)
    B = -(-len(x) // D)
    a = np.zeros(B * D, dtype=np.float32)
    a[:len(x)] = np.where(np.isnan(x), np.float32(0), np.abs(x))
    return a.reshape(B, D).max(axis=1) if B else np.zeros(0, np.float32)


def targets(pk, T):
    """q of float32 peaks -> int64"""
    T = np.concatenate([np.asarray(T, dtype=np.int64), [int(T[-1])]])
    pk = np.minimum(np.maximum(np.asarray(pk, dtype=np.float32), np.float32(2.0 ** -24)), np.float32(256.0))
    u = pk.view(np.uint32).astype(np.int64) - BASE
    j, r = u >> 17, u & 0x1FFFF
    return T[j] + (((T[j + 1] - T[j]) * r) >> 17)


def one_pole(s, q, ca, cr):
    if q < s:
        return s - (((s - q) * ca + FULL - 1) >> 24)
    return s + (((q - s) * cr + FULL - 1) >> 24)


def gains(pk, T, pl, truncated=True):
    """s_b of steps [0, B + K) as Python integers -> int64 array; truncated: each group from unity at its warm-up's start (the
    definition); otherwise one recurrence over the whole history"""
    q = [int(v) for v in targets(pk, T)]
    B, E, ca, cr, W = len(q), len(q) + pl["K"], pl["c_att"], pl["c_rel"], pl["W"]
    q += [ONE] * pl["K"]
    S = np.empty(E, dtype=np.int64)
    if not truncated:
        s = ONE
        for b in range(E):
            s = S[b] = one_pole(s, q[b], ca, cr)
        return S
    for g in range(-(-E // GC)):
        s = ONE
        for b in range(max(g * GC - W, 0), min((g + 1) * GC, E)):  # (below step 0 the target is unity and s stays there)
            s = one_pole(s, q[b], ca, cr)
            if b >= g * GC:
                S[b] = s
    return S


def apply(x, S, D, K, makeup):
    """out_i of every sample; S: s_b of [0, B + K)"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    i = np.arange(n, dtype=np.int64)
    b = i // D
    o = i - b * D
    Sx = np.concatenate([[ONE], np.asarray(S, dtype=np.int64)])  # Sx[u + 1] = s_u, u >= -1
    G = Sx[b + K] * (D - o) + Sx[b + K + 1] * o
    m = np.float64(np.float32(makeup))
    with np.errstate(all="ignore"):
        y = (((x.astype(np.float64) * m) * G.astype(np.float64)) / np.float64(D * ONE)).astype(np.float32)
    if m == 1.0:
        same = G == D * ONE
        y[same] = x[same]
    return y


def pcm16(y):
    y = np.asarray(y, dtype=np.float32)
    c = np.where(y < -1, np.float32(-1), np.where(y > 1, np.float32(1), np.where(np.isnan(y), np.float32(0), y)))
    return (c.astype(np.float64) * 32767.0).astype(np.int16)


def compress(x, T, pl, makeup, truncated=True):
    """-> (peaks f32 [B], s int32 [B + K], out f32 [n], int16 [n])"""
    pk = peaks(x, pl["D"])
    S = gains(pk, T, pl, truncated)
    y = apply(x, S, pl["D"], pl["K"], makeup)
    return pk, S.astype(np.int32), y, pcm16(y)


def reduction_db(S):
    return 20.0 * np.log10(np.asarray(S, dtype=np.float64) / ONE)


def curve_error_db(T, p, count=5000, seed=1):
    """the worst |interpolated table - formula| in dB over log-spaced levels from 1e-4 to 4"""
    lv = np.exp(np.random.default_rng(seed).uniform(math.log(1e-4), math.log(4.0), count)).astype(np.float32)
    q = targets(lv, T)
    return max(abs(20.0 * math.log10(int(v) / ONE) - gain_db(20.0 * math.log10(float(a)), p)) for a, v in zip(lv, q))


# ---- takes ----
def envelope_take(n, sr, seed, low_db=-50.0):
    """noise under a slow random level envelope: a new level from [low_db, 0] dB every 30 ms"""
    rng = np.random.default_rng(seed)
    seg = max(1, int(0.03 * sr))
    lev = np.repeat(10.0 ** (rng.uniform(low_db, 0.0, n // seg + 1) / 20.0), seg)[:n]
    return (rng.standard_normal(n) * 0.4 * lev).astype(np.float32)


def click_take(n, seed):
    """clicks of up to +-2 about every 1500 samples over a bed of -0.0f and +0.0f"""
    rng = np.random.default_rng(seed)
    x = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    at = np.flatnonzero(rng.random(n) < 1.0 / 1500.0)
    x[at] = rng.uniform(-2.0, 2.0, len(at)).astype(np.float32)
    return x


def cut_points(n, D):
    """inside a step, on a step, on a group seam and one sample either side of it"""
    seam = GC * D
    return sorted({c for c in (0, 1, D // 2 + 3 * D, 7 * D, seam - 1, seam, seam + 1, 2 * seam - 1, 2 * seam, n - 1, n) if 0 <= c <= n})


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_laws(make, sr, setting):
    """The laws of the header on an implementation.  make(params) -> an object with .T, .plan, .run(x, first=0, count=None) ->
    float32 outputs and .gain(x) -> s_b of [0, B); setting: fields over the defaults (makeup_amp is forced to 1 where a law
    speaks of the input's bytes)."""
    p = params(**setting)
    unit = dict(setting, makeup_amp=1.0)
    imp, imp1 = make(params(**setting)), make(params(**unit))
    pl, T = imp.plan, imp.T
    D, K, W = pl["D"], pl["K"], pl["W"]
    n = GC * D + 777
    x = envelope_take(n, sr, seed=11)
    whole = imp.run(x)
    # the implementation is the reference
    pk, S, y, _ = compress(x, T, pl, p["makeup_amp"])
    assert same(whole, y), "reference"
    assert same(imp.gain(x), S[:steps(n, sr)]), "reference gain"
    # split
    cuts = cut_points(n, D)
    assert same(np.concatenate([imp.run(x, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]), whole), "split"
    # ratio 1
    assert same(make(params(**dict(unit, ratio=1.0))).run(x), x), "ratio 1"
    # below the knee; silence
    quiet = (x * np.float32(0.999 * knee_floor(p) / np.abs(x).max())).astype(np.float32)
    assert np.abs(quiet).max() < knee_floor(p) and same(imp1.run(quiet), quiet), "below the knee"
    z = np.where(np.arange(3 * D + 5) % 3 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert same(imp.run(z), z), "silence"
    # steady state
    a, nst = np.float32(0.5), W + 512
    dc = np.full(nst * D, a, dtype=np.float32)
    dc[1::2] *= -1
    qa = int(targets(np.array([a], np.float32), T)[0])
    Sd, yd = imp.gain(dc), imp.run(dc)
    settled = int(np.flatnonzero(Sd != qa)[-1]) + 1 if (Sd != qa).any() else 0
    assert settled < nst - 8, ("steady state", settled, nst)
    m = float(np.float32(p["makeup_amp"]))
    tail = yd[(settled + 1) * D:] if K == 0 else yd[(settled + 1) * D:(nst - K - 1) * D]
    want = np.float32((float(a) * m) * float(qa * D) / float(D * ONE))
    assert len(tail) and np.all(np.abs(tail) == want), "steady state output"
    assert abs(float(want) - float(a) * m * qa / ONE) <= float(np.spacing(want)), "steady state value"
    # recovery
    burst = np.concatenate([envelope_take(20 * D, sr, seed=5, low_db=-6.0), np.resize(quiet, (W + 600) * D)]).astype(np.float32)
    Sb, yb = imp1.gain(burst), imp1.run(burst)
    low = np.flatnonzero(Sb != ONE)
    assert len(low) and low[-1] < len(Sb) - 8, ("recovery", low[-1] if len(low) else None, len(Sb))
    back = (int(low[-1]) + 2) * D
    assert same(yb[back:], burst[back:]), "recovery output"
    # monotone
    louder = x.copy()
    louder[5000:9000] *= np.float32(2.0)
    louder[n // 2] = np.float32(3.0)
    assert np.all(imp.gain(louder) <= imp.gain(x)), "monotone"
    # NaN in place of a sample that is not its step's largest
    b = (n // 3) // D
    t = b * D + int(np.argmin(np.abs(x[b * D:(b + 1) * D])))
    xn = x.copy()
    xn[t] = np.nan
    yn = imp.run(xn)
    assert np.isnan(yn[t]) and same(np.delete(yn, t), np.delete(whole, t)), "NaN"
    # Inf
    for t in (n // 3, GC * D - 5, n - 2):
        xi = x.copy()
        xi[t] = -np.inf if t % 2 else np.inf
        yi = imp.run(xi)
        before = max((t // D - K - 1) * D, 0)
        after = (((t // D + W) // GC + 1) * GC - K + 1) * D
        assert same(yi[:before], whole[:before]) and np.isinf(yi[t]), ("Inf before", t)
        assert same(yi[after:], whole[after:]), ("Inf after", t)
