"""The noise reduction of include/melonix_amd.h "Noise reduction" restated in numpy, binary64, with no code shared with the library:
framing, powers, print, raw and smoothed gains, the inverse transform and the overlap-add; the test takes; the yardstick; and
check_laws, the definition's consequences as assertions on any implementation (the CPU emulation, the device).  The two factors
`floor` and `sens` are the library's binary32 values (mx_denoise_factors), as the definition has every implementation read them."""
import numpy as np

N, H, BINS, LEAD = 1024, 256, 513, 3
W = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
SR = 48000


def frames(n: int) -> int:
    return -(-n // H) + LEAD


def spectra(x):
    """X_f[k] of every frame of the take: (F, 513) complex128"""
    x = np.asarray(x, dtype=np.float64)
    F = frames(len(x))
    padded = np.concatenate([np.zeros(LEAD * H), x, np.zeros((F - 1 - LEAD) * H + N - len(x))])
    idx = H * np.arange(F)[:, None] + np.arange(N)[None, :]
    with np.errstate(invalid="ignore"):
        return np.fft.rfft(padded[idx] * W, axis=1)


def powers(X):
    with np.errstate(invalid="ignore", over="ignore"):
        return (X.real ** 2 + X.imag ** 2) / (512.0 ** 2)


def region_frames(n: int, begin: int, end: int):
    """(first frame, count) of the frames wholly inside [begin, end), or None where the region is refused"""
    if begin < 0 or end < begin or end > n or end - begin < N:
        return None
    f0, f1 = LEAD + -(-begin // H), LEAD + (end - N) // H
    return (f0, f1 - f0 + 1) if f0 <= f1 and f1 - f0 + 1 <= 8192 else None


def noise_print(x, begin: int, end: int):
    f0, count = region_frames(len(x), begin, end)
    return powers(spectra(x)[f0:f0 + count]).mean(axis=0)


def smooth(g, axis: int):
    lo = np.concatenate([np.take(g, [0], axis), g, np.take(g, [-1], axis)], axis)
    n = g.shape[axis]
    return (np.take(lo, range(0, n), axis) + 2.0 * g + np.take(lo, range(2, n + 2), axis)) / 4.0


def gains(a, P, floor, sens):
    theta = float(sens) * np.asarray(P, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(a > theta, 1.0 - theta / a, 0.0)
    g = np.where(g < float(floor), float(floor), g)
    return smooth(smooth(g, 0), 1)


def denoise(x, P, floor, sens):
    """-> the cleaned take, float64"""
    n = len(x)
    X = spectra(x)
    G = gains(powers(X), P, floor, sens)
    with np.errstate(invalid="ignore"):
        y = np.fft.irfft(G * X, N, axis=1) * W * float(np.float32(2.0 / 3.0))
    F = len(X)
    acc = np.zeros((F - 1) * H + N)
    for f in range(F):  # ascending f
        acc[f * H:f * H + N] += y[f]
    return acc[LEAD * H:LEAD * H + n]


def pcm16(v):
    """the clamped conversion of the header's "PCM conversions", on float32 samples"""
    v = np.asarray(v, dtype=np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.clip(v, -1.0, 1.0)).astype(np.float64)
    return np.trunc(c * 32767.0).astype(np.int16)


def tolerance(ref):
    """the project's yardstick: 2e-5 max|ref| + 1e-9"""
    ref = np.asarray(ref, dtype=np.float64)
    m = float(np.nanmax(np.abs(ref))) if ref.size and not np.all(np.isnan(ref)) else 0.0
    return 2e-5 * m + 1e-9


def worst(got, ref):
    """max |got - ref| (NaNs must sit at the same places) as a fraction of the yardstick"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    if not got.size:
        return 0.0
    ok = ~np.isnan(ref)
    return float(np.abs(got - ref)[ok].max(initial=0.0)) / tolerance(ref)


def assert_close(got, ref, what=""):
    w = worst(got, ref)
    assert w <= 1.0, (what, w)
    return w


# ---- the takes ----
def vowel_take(noise=1e-2, seed=5, n=SR, onset=12000):
    """one second at 48 kHz: a 150 Hz vowel of 19 harmonics from sample `onset` on, over white noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    v = sum(np.sin(2.0 * np.pi * 150.0 * h * t + 0.3 * h) / h for h in range(1, 20))
    v = 0.25 * v / np.abs(v).max()
    v[:onset] = 0.0
    return (v + noise * rng.standard_normal(n)).astype(np.float32)


def noise_take(n=10007, level=1e-2, seed=6):
    return (level * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def click_take(n=10007, seed=7):
    w = (1e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    w[::997] = 0.8
    return w


def short_take():
    """a 10 ms file"""
    return vowel_take(n=480, onset=100, seed=8)


LENGTHS = (0, 1, 255, 256, 257, 1023, 1024, 1025, 10007)
SETTINGS = ((12.0, 6.0), (24.0, 6.0), (48.0, 12.0))  # (reduction, sensitivity) dB: the issue's three


def flat_print(level):
    return np.full(BINS, level, dtype=np.float32)


def db(x):
    return 20.0 * np.log10(x)


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


# ---- the laws ----
def check_laws(run, floor, sens, locality_at=None):
    """run(x, P, first=0, count=None) -> float32 outputs [first, first + count) of the cleaned take x under the print P with the
    factors (floor, sens).  The consequences of the header, as assertions."""
    x = np.concatenate([noise_take(1500, seed=11), vowel_take(n=2500, onset=0, seed=12)]).astype(np.float32)
    n = len(x)
    P = noise_print(x, 0, 1500).astype(np.float32)
    whole = run(x, P)
    assert whole.dtype == np.float32 and len(whole) == n
    assert_close(whole, denoise(x, P, floor, sens), "the law take")
    # split: any split of the output range gives the same bytes
    for cuts in ((0, 37, n), (0, 257, n), (0, 255, 256, 1023, 1024, 1025, n), (0, n // 3, n // 3, n)):
        parts = [run(x, P, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        assert b"".join(p.tobytes() for p in parts) == whole.tobytes(), cuts
    for j in (0, 1, 255, 256, 511, 512, n - 1):
        assert run(x, P, j, 1).tobytes() == whole[j:j + 1].tobytes(), j
    assert len(run(x, P, 17, 0)) == 0 and len(run(x, P, n, 0)) == 0
    # scale: x 2^k with P 4^k gives out 2^k, bit for bit
    for k in (-7, -20):
        s = np.float32(2.0 ** k)
        assert run(x * s, P * s * s).tobytes() == (whole * s).tobytes(), k
    # zero print: out = x within the yardstick (the transform pair's own error)
    assert_close(run(x, flat_print(0.0)), x, "zero print")
    # full reduction: a print of 1e6 times the take's largest power gives floor x
    top = float(powers(spectra(x)).max())
    full = flat_print(1e6 * top)
    assert_close(run(x, full), float(floor) * x.astype(np.float64), "full reduction")
    # silence gives zeros, of -0.0f samples too
    for z in (np.zeros(777, np.float32), np.full(777, -0.0, np.float32)):
        assert not run(z, P[:BINS]).view(np.uint32).any()
    # locality: a NaN at s
    clean_full = run(x, full)
    for s in (0, 255, 256, n - 1, 2000) if locality_at is None else locality_at:
        y = x.copy()
        y[s] = np.nan
        b = s // H
        lo, hi = max((b - 3) * H, 0), min((b + 4) * H, n)
        for pr, clean, reach in ((P, whole, 1), (full, clean_full, 0)):
            got = run(y, pr)
            nan = np.isnan(got)
            assert nan[lo:hi].all() and not nan[:lo].any() and not nan[hi:].any(), (s, int(nan.sum()), lo, hi)
            # the gains of the four frames are `floor`; the frames either side see them through the time smoothing (reach 1),
            # unless every gain is `floor` anyway (reach 0): beyond that no output changes a bit
            keep = np.ones(n, bool)
            keep[max((b - 3 - reach) * H, 0):min((b + 4 + reach) * H, n)] = False
            assert np.array_equal(got.view(np.uint32)[keep], clean.view(np.uint32)[keep]), (s, reach)
        assert_close(run(y, P), denoise(y, P, floor, sens), "a NaN take")
