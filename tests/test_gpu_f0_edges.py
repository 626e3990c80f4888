"""The YIN tracker's input space beyond test_gpu_f0.py's corner, against the f64 restatement (tests/yin_ref.py): sample
rates that put the search range in the second wavefront's half of the lag axis, bands on the run / wave boundaries and at
the W-1 clamp, thresholds, hops and first frames, short files and levels from subnormal to 1e30.  Then two exact
properties of the records, bit for bit: a record depends on its frame's samples alone (shift), and scaling the audio by a
power of two scales rms alone (scale)."""
import math

import numpy as np
import pytest

import yin_ref as Y

pytestmark = pytest.mark.gpu

HOP = 256


def _tone(sr, period, n, partials=(1.0,), amp=0.5):
    i = np.arange(n, dtype=np.float64)
    w = sum(a * np.sin(2 * np.pi * (k + 1) * i / period) for k, a in enumerate(partials) if a)
    return amp * w / max(1.0, sum(abs(a) for a in partials))


def _boundary_periods(tmin, tmax):
    """Periods that put tau* just below and just above each boundary in [tmin, tmax]: the ends of the range, the 16|17
    boundary of the first two threads' lag runs (thread t owns 16t+1 .. 16t+16) and the 1024|1025 wavefront boundary."""
    ps = [tmin + 0.2, tmin + 0.8, tmin - 0.3, tmax - 0.8, tmax - 0.2, tmax + 0.3]
    for b in (16.5, 1024.5):
        if tmin <= b - 0.5 and b + 0.5 <= tmax:
            ps += [b - 0.3, b + 0.3]
    return sorted({p for p in ps if p >= 2.1})


def _signals(sr, tmin, tmax):
    n = max(int(0.1 * sr), 6144)
    rng = np.random.default_rng(sr + 7 * tmin + tmax)
    mid = math.sqrt(tmin * tmax) + 0.2  # (not half-way between two lags: that is a tie by symmetry)
    s = {f"tone_p{p:g}": _tone(sr, p, n) for p in _boundary_periods(tmin, tmax)}
    s["missing_fundamental"] = _tone(sr, mid, 2 * n, partials=(0, 0.5, 0.33, 0.25, 0.2))
    s["noisy_tone"] = _tone(sr, mid, 2 * n) + 1e-3 * rng.uniform(-1, 1, 2 * n)
    s["noise"] = 0.3 * rng.uniform(-1, 1, 2 * n)
    s["silence"] = np.zeros(n)
    s["onset"] = np.concatenate([np.zeros(n), _tone(sr, mid, n)])
    return {k: v.astype(np.float32) for k, v in s.items()}


class Tally:
    """Frames and excused near-ties (tau differs, by the near-tie rule) over a configuration: at most `limit` of them."""

    def __init__(self, label, limit=0.005):
        self.label, self.limit, self.frames, self.excused = label, limit, 0, 0

    def add(self, r):
        self.frames += r[0]
        self.excused += r[1]

    def check(self):
        print(f"f0 parity {self.label}: tau excused as a near-tie on {self.excused} of {self.frames} frames "
              f"({100.0 * self.excused / max(self.frames, 1):.3f} %)")
        assert self.excused <= self.limit * self.frames, self.label


def _parity(ctx, w, sr, label, hop=HOP, first=0, count=None, fmin=55.0, fmax=1760.0, threshold=0.15, ap_rel=1e-3):
    a = ctx.upload(w)
    got = ctx.f0_track(a, sr, hop, first, count, fmin=fmin, fmax=fmax, threshold=threshold)
    a.free()
    recs, dp = Y.track(w, sr, hop, first, count, fmin=fmin, fmax=fmax, threshold=threshold)
    tmin, tmax = Y.tau_range(sr, fmin, fmax)
    r = Y.check_parity(got, recs, dp, tmin, tmax, float(np.float32(threshold)), label, eps=1e-4, cents=1.0,
                       ap_abs=1e-4, ap_rel=ap_rel, rms_rel=1e-5, rms_floor=0.0, rms_sub_abs=2.0 ** -149,
                       check_excused=True)
    return got, r


def _run_config(ctx, sr, fmin=55.0, fmax=1760.0, threshold=0.15, expect=None):
    tmin, tmax = Y.tau_range(sr, fmin, fmax)
    if expect is not None:
        assert (tmin, tmax) == expect, (sr, fmin, fmax)
    label = f"sr={sr} tau=[{tmin},{tmax}] theta={threshold:g}"
    # Where near-ties are the rule rather than the exception, more of them may flip (each one still checked against the
    # reference's d' by check_excused):
    # - theta = 0 takes the argmin on every frame, and a tone's d' has a near-zero minimum at every multiple of its
    #   period in range: which multiple wins is decided ~1e-6 below d' itself;
    # - with every lag >= 1024 the curvature of d' at a minimum, ~2 (2 pi / tau)^2 per lag^2, is under 7.5e-5: a minimum
    #   between two lags leaves them within ~1e-5, a few times the f32 d' error of a frame that holds one or two periods.
    limit = 0.25 if threshold == 0.0 else 0.02 if tmin >= 1024 else 0.005
    # threshold 3e38 starts the descent at tau_min = 2, where d of a tone of period ~1000-2000 is ~1e-5 of e0: its
    # e0 + e_tau - 2 r(tau) in f32 keeps only ~1e-3 to 1e-2 relative, and so does d' there
    ap_rel = 3e-2 if threshold > 1.0 else 1e-3
    tally = Tally(label, limit)
    for name, w in _signals(sr, tmin, tmax).items():
        got, r = _parity(ctx, w, sr, f"{label} {name}", fmin=fmin, fmax=fmax, threshold=threshold, ap_rel=ap_rel)
        tally.add(r)
        if tmin == tmax:
            assert (got["tau"][got["rms"] > 0] == tmin).all(), label
    tally.check()


# ---- 1. parity with the reference ----
@pytest.mark.parametrize("sr", [8000, 16000, 22050, 88200, 96000, 192000])
def test_sample_rates(gpu_ctx, sr):
    _run_config(gpu_ctx, sr)


# (sr, fmin, fmax, (tau_min, tau_max)): bands found by inverting floor(sr/fmax), ceil(sr/fmin) on the f32 band
BANDS = [
    (48000, 55.0, 48000.0, (2, 873)),                # fmax >= sr/2: tau_min clamps at 2
    (48000, 48000 / 16.5, 48000 / 2.5, (2, 17)),
    (48000, 48000 / 1023.5, 48000 / 16.5, (16, 1024)),
    (48000, 48000 / 1024.5, 48000 / 17.5, (17, 1025)),
    (48000, 48000 / 2046.5, 48000 / 1024.5, (1024, 2047)),
    (48000, 1.0, 48000 / 1025.5, (1025, 2047)),     # fmin below sr/(W-1): tau_max clamps at W-1
    (48000, 1.0, 48000.0, (2, 2047)),
    (48000, 46.875, 46.875, (1024, 1024)),          # 48000 / 46.875 = 1024 exactly
    (49200, 48.0, 48.0, (1025, 1025)),              # 49200 / 48 = 1025 exactly
    (48000, 48000 / 1024.5, 46.875, (1024, 1025)),  # two lags, one per wavefront
]


@pytest.mark.parametrize("sr,fmin,fmax,expect", BANDS, ids=[f"{b[3][0]}-{b[3][1]}" for b in BANDS])
def test_bands(gpu_ctx, sr, fmin, fmax, expect):
    _run_config(gpu_ctx, sr, fmin, fmax, expect=expect)


@pytest.mark.parametrize("threshold", [0.0, 0.05, 0.5, 1.0, 3e38])
@pytest.mark.parametrize("sr,fmin,fmax", [(48000, 55.0, 1760.0), (96000, 1.0, 48000.0)])
def test_thresholds(gpu_ctx, threshold, sr, fmin, fmax):
    _run_config(gpu_ctx, sr, fmin, fmax, threshold)


def _program(sr, secs, seed=5):
    """A harmonic glide 110 -> 880 Hz under 1e-3 noise with a gap that holds a silent stretch: voiced, unvoiced, onset
    and silent frames at any hop."""
    n = int(secs * sr)
    i = np.arange(n, dtype=np.float64)
    ph = np.cumsum(2 * np.pi * (110.0 * 8.0 ** (i / n)) / sr)
    w = 0.4 * np.sin(ph) + 0.15 * np.sin(2 * ph) + 0.05 * np.sin(3 * ph)
    w[n // 3:n // 3 + 8192] = 0.0
    w += 1e-3 * np.random.default_rng(seed).uniform(-1, 1, n)
    w[n // 3 + 512:n // 3 + 8192 - 512] = 0.0
    return w.astype(np.float32)


@pytest.mark.parametrize("hop", [1, 2, 3, 255, 257, 1000, 4095, 4096, 16384])
def test_hops_and_first_frames(gpu_ctx, hop):
    w = _program(48000, 1.0)
    F = -(-len(w) // hop)
    rng = np.random.default_rng(hop)
    tally = Tally(f"hop={hop}")
    for first in sorted({0, 1, int(rng.integers(1, F - 1)), F - 1}):
        count = min(F - first, 48)
        tally.add(_parity(gpu_ctx, w, 48000, f"hop={hop} first={first} count={count}", hop=hop, first=first,
                          count=count)[1])
    tally.check()


@pytest.mark.parametrize("hop", [256, 1])
def test_short_files(gpu_ctx, hop):
    rng = np.random.default_rng(hop + 1)
    tally = Tally(f"short files n >= 255 hop={hop}")
    for n in (1, 2, 3, 255, 2047, 2048, 2049, 4095, 4096, 4097):
        w = (_tone(48000, 109.3, n) + 1e-3 * rng.uniform(-1, 1, n)).astype(np.float32)
        r = _parity(gpu_ctx, w, 48000, f"n={n} hop={hop}", hop=hop)[1]
        # (a frame that holds one to three samples has d' flat to ~1e-6 over the range: which lag wins is noise in
        # either implementation, and the near-tie rule excuses it; such frames stay out of the excused fraction)
        if n >= 255:
            tally.add(r)
    tally.check()


def _level_signals():
    sr = 48000
    base = _tone(sr, sr / 220.0, sr, partials=(1, 0.5, 0.25), amp=1.0)
    out = {"tail_0.5_to_1e-42": 0.5 * base * np.exp(np.linspace(0.0, math.log(2e-42), sr))}
    for lv in (1e-20, 1e-24, 1e-30, 1e-40, 1e12, 1e30):
        out[f"level_{lv:g}"] = lv * base
    return {k: v.astype(np.float32) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(_level_signals()))
def test_levels(gpu_ctx, name):
    w = _level_signals()[name]
    assert np.isfinite(w).all() and (w != 0).sum() > len(w) // 2
    tally = Tally(f"level {name}")
    got, r = _parity(gpu_ctx, w, 48000, f"level {name}")
    tally.add(r)
    tally.check()
    x = Y.frames_of(w, HOP, 0, len(got))
    assert ((got["tau"] == 0) == ~x.any(axis=1)).all(), "a frame is silent exactly when its samples are all zero"


# ---- 2. exact properties ----
def _track(ctx, w, hop=HOP, count=None):
    a = ctx.upload(np.ascontiguousarray(w, dtype=np.float32))
    got = ctx.f0_track(a, 48000, hop, 0, count)
    a.free()
    return got


@pytest.mark.parametrize("hop", [255, 256, 257])
def test_shift_by_whole_hops(gpu_ctx, hop):
    w = _program(48000, 0.5, seed=hop)
    ref = _track(gpu_ctx, w, hop)
    assert (ref["tau"] > 0).sum() > len(ref) // 2 and (ref["tau"] == 0).any()
    for s in (1, 3, 17):
        got = _track(gpu_ctx, np.concatenate([np.zeros(s * hop, np.float32), w]), hop)
        assert len(got) == len(ref) + s
        assert got[s:].tobytes() == ref.tobytes(), (hop, s)
        zeros_only = (s - np.arange(s)) * hop >= Y.W  # frame h reads [h hop - W, h hop + W); w starts at s hop
        silent = np.array([Y.SILENT] * int(zeros_only.sum()), dtype=got.dtype)
        assert got[:s][zeros_only].tobytes() == silent.tobytes(), (hop, s)
    for extra in (1, hop, 3 * Y.N + 5):
        got = _track(gpu_ctx, np.concatenate([w, np.zeros(extra, np.float32)]), hop, count=len(ref))
        assert got.tobytes() == ref.tobytes(), (hop, extra)


def test_scale_by_powers_of_two(gpu_ctx):
    """Every k with 2^k x exact in f32 (16-bit PCM peaking below 1/2: k = -134 .. 129, the lowest with subnormal
    samples): tau, period and aperiodicity bit for bit, rms equal to ldexp(rms, k)."""
    w = Y.pcm16(_program(48000, 0.25, seed=9))
    ks = Y.exact_scales(w)
    assert ks[0] <= -130 and ks[-1] >= 120 and ks == list(range(ks[0], ks[-1] + 1)), (ks[0], ks[-1])
    ref = _track(gpu_ctx, w)
    assert (ref["tau"] > 0).sum() > len(ref) // 2
    for k in ks:
        got = _track(gpu_ctx, np.ldexp(w, k))
        for f in ("tau", "period", "aperiodicity"):
            assert got[f].tobytes() == ref[f].tobytes(), (k, f)
        assert got["rms"].tobytes() == np.ldexp(ref["rms"], k).tobytes(), k
    print(f"f0 scale: {len(ref)} frames bit for bit at 2^k x, k = {ks[0]} .. {ks[-1]}")
