"""Sample-rate conversion of include/melonix_amd.h ("Sample-rate conversion"), restated in numpy and Python integers: plan(),
length() and index_map() are the integers of the definition; table64() is the binary64 formula a CPU test holds the library's
table (mx_resample_taps) against; resample() is the definition the kernel must equal byte for byte, given that table; resample64()
is the same sum in binary64, what the quality of the binary32 sum is measured against; response() is the prototype's frequency
response.  Plus the takes and the reference chain of the export at another rate."""
import math

import numpy as np

import bad_samples as BAD
import loudness_ref as L
import sibilant_ref as SIB
import truepeak_ref as T

MIN_RATE, MAX_RATE = 8000, 384000
Z, MAX_PHASES, MAX_TAPS, BETA = 32, 1024, 512, 12.0

# in -> out of the ratios the tests walk: 147/160, 160/147, 1/2, 2/1, 6/1, 441/80, 147/640, 80/441
PAIRS = ((48000, 44100), (44100, 48000), (96000, 48000), (48000, 96000), (8000, 48000), (8000, 44100), (192000, 44100), (44100, 8000))


def plan(in_rate, out_rate):
    """-> {L, M, taps, half}, or None where the definition refuses the pair."""
    if not (MIN_RATE <= in_rate <= MAX_RATE and MIN_RATE <= out_rate <= MAX_RATE):
        return None
    g = math.gcd(in_rate, out_rate)
    L_, M = out_rate // g, in_rate // g
    if L_ == M:
        return {"L": 1, "M": 1, "taps": 0, "half": 0}
    H = -(-Z * max(L_, M) // L_)
    if L_ > MAX_PHASES or 2 * H > MAX_TAPS:
        return None
    return {"L": L_, "M": M, "taps": 2 * H, "half": H}


def length(n, p):
    return -(-n * p["L"] // p["M"])


def index_map(j, p):
    """(i_j, phi_j) in Python integers"""
    return (j * p["M"]) // p["L"], (j * p["M"]) % p["L"]


def bessel_i0(x):
    half, q, total = x / 2.0, 1.0, 1.0
    for k in range(1, 1000):
        q = q * half / float(k)
        term = q * q
        total = total + term
        if term < total * 2.0 ** -60:
            break
    return total


def table64(p):
    """h[phi][k] by the header's formula in binary64 -> float64[L, taps] (not yet rounded; the unit rows are exact)."""
    L_, M, T_, H = p["L"], p["M"], p["taps"], p["half"]
    s = L_ / M if L_ < M else 1.0
    i0_beta = bessel_i0(BETA)
    out = np.zeros((L_, T_))
    for phi in range(L_):
        if s == 1.0 and phi == 0:
            out[phi, H - 1] = 1.0
            continue
        row = []
        total = 0.0
        for k in range(T_):
            u = float(k - (H - 1)) - phi / L_
            v, t = s * u, u / float(H)
            sinc = 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
            a = max(1.0 - t * t, 0.0)
            row.append(s * sinc * (bessel_i0(BETA * math.sqrt(a)) / i0_beta))
            total = total + row[-1]
        out[phi] = [h / total for h in row]
    return out


def _windows(x, p, first, count, dtype):
    """(xp, start, phi): xp the take with H zeros either side; output first + r reads xp[start[r] + k], k < taps."""
    n, H = len(x), p["half"]
    j = first + np.arange(count, dtype=np.int64)
    t = j * np.int64(p["M"])
    i, phi = t // p["L"], t % p["L"]
    xp = np.concatenate([np.zeros(H, dtype), np.asarray(x, dtype), np.zeros(H + 1, dtype)])  # xp[s + H] = x_s
    return xp, i + 1, phi  # (i - (H - 1) + H)


def resample(x, p, taps, first=0, count=None):
    """Outputs [first, first + count) (None: to the end) -> float32.  Binary32: each product rounded, then added, k ascending,
    from +0.  taps: float32[L, taps], the library's table."""
    x = np.asarray(x, dtype=np.float32)
    count = length(len(x), p) - first if count is None else count
    if p["taps"] == 0:
        return x[first:first + count].copy()
    taps = np.asarray(taps, dtype=np.float32)
    xp, start, phi = _windows(x, p, first, count, np.float32)
    y = np.zeros(count, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(p["taps"]):
            y = y + xp[start + k] * taps[phi, k]
    assert y.dtype == np.float32
    return y


def resample64(x, p, taps, first=0, count=None):
    """The same sum in binary64 over the same (binary32) table -> float64."""
    x = np.asarray(x, dtype=np.float64)
    count = length(len(x), p) - first if count is None else count
    if p["taps"] == 0:
        return x[first:first + count].copy()
    taps = np.asarray(taps, dtype=np.float64)
    xp, start, phi = _windows(x, p, first, count, np.float64)
    y = np.zeros(count)
    with np.errstate(all="ignore"):
        for k in range(p["taps"]):
            y = y + xp[start + k] * taps[phi, k]
    return y


def affected(s, p, m):
    """bool[m]: the outputs j that read sample s: s - H <= i_j <= s + H - 1"""
    i = (np.arange(m, dtype=np.int64) * p["M"]) // p["L"]
    return (s - p["half"] <= i) & (i <= s + p["half"] - 1)


def check_laws(run, p, t, n=6007):
    """Laws 1-6 of the definition, written once for the emulation and the device: run(w, first=0, count=None) -> the float32
    outputs [first, first + count) of take w (None: to the end)."""
    L_, M, H = p["L"], p["M"], p["half"]
    w = take(n, seed=L_ + M)
    m = length(n, p)
    out = run(w)
    assert len(out) == m
    if L_ > M:                                                                                   # 1 unit rows
        j = np.arange(0, m, L_)
        assert len(j) > 3 and out[j].tobytes() == w[j * M // L_].tobytes()
    for k in (-7, -20):                                                                          # 2 scale
        f = np.float32(2.0 ** k)
        assert run(w * f).tobytes() == (out * f).tobytes(), k
    for silence in (np.zeros(n, np.float32), np.full(n, -0.0, np.float32)):                      # 3 silence
        assert run(silence).tobytes() == np.zeros(m, np.float32).tobytes()
    for s in (0, n // 2, n - 1):                                                                 # 4 locality
        hit = affected(s, p, m)
        moved = run(BAD.with_bad(w, s, np.float32(w[s] + 0.25)))
        assert moved[~hit].tobytes() == out[~hit].tobytes() and hit.any(), s
        nan = run(BAD.with_bad(w, s, BAD.BAD["nan"]))
        assert np.array_equal(np.isnan(nan), hit) and nan[~hit].tobytes() == out[~hit].tobytes(), s
    shifted = run(np.concatenate([np.zeros(M, np.float32), w]))                                  # 5 shift
    edge = (H + M) * L_ // M + L_ + 2  # outputs whose windows reach the file's ends
    assert shifted[L_ + edge:m + L_ - edge].tobytes() == out[edge:m - edge].tobytes() and m > 4 * edge
    cuts = (0, 1, m // 3, m // 3, (2 * m) // 3 + 1, m - 1, m)                                     # 6 split
    assert b"".join(run(w, lo, hi - lo).tobytes() for lo, hi in zip(cuts, cuts[1:])) == out.tobytes()


def response(p, taps, in_rate, hz):
    """|H(f)| of the table's prototype at the frequencies hz (Hz; the prototype runs at L * in_rate) -> float64, DC = 1."""
    L_, T_, H = p["L"], p["taps"], p["half"]
    u = (np.arange(T_)[None, :] - (H - 1)) - np.arange(L_)[:, None] / L_  # input samples from the output
    h = np.asarray(taps, dtype=np.float64).ravel()
    u = u.ravel()
    out = np.empty(len(hz))
    for a in range(0, len(hz), 256):
        ph = np.exp(-2j * np.pi * np.asarray(hz[a:a + 256])[:, None] * u[None, :] / in_rate)
        out[a:a + 256] = np.abs(ph @ h) / L_
    return out


def response_grid(p, taps, in_rate):
    """The same response on the dense grid of one FFT of the prototype (tap (phi, k) sits at sample (k - (H - 1)) L - phi of the
    rate L * in_rate), zero-padded to at least 64 times its length -> (hz, |H|) from 0 to the prototype's Nyquist rate, DC = 1."""
    L_, T_, H = p["L"], p["taps"], p["half"]
    at = (np.arange(T_)[None, :] - (H - 1)) * L_ - np.arange(L_)[:, None]
    proto = np.zeros(L_ * T_ + L_)
    proto[(at - at.min()).ravel()] = np.asarray(taps, dtype=np.float64).ravel()
    size = 1 << int(math.ceil(math.log2(64 * len(proto))))
    return np.fft.rfftfreq(size, 1.0 / (L_ * in_rate)), np.abs(np.fft.rfft(proto, size)) / L_


def db(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def take(n, seed):
    """noise with a click every 4099 samples (truepeak_ref's take of the records)"""
    return T.sparse_clicks(n, seed) if n else np.zeros(0, np.float32)


def band_noise(n, sr, hz, seed=5):
    """noise band-limited to hz by a brick wall in the frequency domain, peak 0.5 -> float64"""
    rng = np.random.Generator(np.random.PCG64(seed))
    spec = np.fft.rfft(rng.standard_normal(n))
    spec[np.fft.rfftfreq(n, 1.0 / sr) > hz] = 0.0
    w = np.fft.irfft(spec, n)
    return 0.5 * w / np.abs(w).max()


def export_chain_at(w, sr, out_rate, k_in, k_out, tp_taps, rs_taps, target_lufs, c=T.MINUS_1_DBTP):
    """measure at sr -> the gain to target_lufs -> convert to out_rate -> limit with the limiter's defaults at out_rate -> int16,
    then measure again at out_rate, on the CPU -> dict.  k_in / k_out: the library's K-weighting coefficients at the two rates."""
    x = np.asarray(w, dtype=np.float32)
    before = L.integrated(L.steps(x, sr, k_in), sr)
    amp = np.float32(math.pow(10.0, (target_lufs - before["integrated"]) / 20.0))
    gained = SIB.apply_gain(x, [(0, amp)])
    p = plan(sr, out_rate)
    converted = resample(gained, p, rs_taps)
    out, pcm = T.limit(converted, out_rate, tp_taps, c, T.default_lookahead(out_rate))
    after = L.integrated(L.steps(out, out_rate, k_out), out_rate)
    tp_after = T.measure(T.records(out, out_rate, tp_taps))
    return dict(amp=amp, gained=gained, converted=converted, out=out, pcm=pcm, after=after, tp_after=tp_after)
