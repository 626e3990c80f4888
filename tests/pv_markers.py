"""Seeded marker sets for the marker-driven phase vocoder (tests/test_pv.py: host plan vs oracle plan; tests/test_gpu_pv_edges.py:
render vs oracle render).  A marker is (sample, note, dTime, pitchBend), sorted by sample.  The sets reach what the time map allows:
markers before sample 0 (the first segment runs backward) and beyond the file, segments from about 2 s backward in warped time
(never matched: the map jumps) over stalls to 20-100x stretches, bends anywhere in [-48, 48] held, ramped or jumping from one end
to the other at a marker, last markers before n - 1 (the bend ramps to 0 at the duration) or none at all."""
import numpy as np

SR = 48000


def _segment_dtime(rng, length, sr):
    """dTime of a segment `length` samples long (the warped time it takes is |length|/sr + dTime)."""
    span = abs(length) / sr
    kind = rng.integers(0, 6)
    if kind == 0:
        return 0.0
    if kind == 1:  # stretch 1.5 .. 8x
        return (rng.uniform(1.5, 8.0) - 1.0) * span
    if kind == 2:  # stretch 20 .. 100x: stalls (less than one sample of analysis advance per frame)
        return (rng.uniform(20.0, 100.0) - 1.0) * span
    if kind == 3:  # squeeze 1.5 .. 6x
        return -(1.0 - 1.0 / rng.uniform(1.5, 6.0)) * span
    return -float(rng.uniform(0.0, 2.0))  # backward in warped time (-2 s .. 0): never matched, the map jumps over it


def _bend(rng):
    kind = rng.integers(0, 5)
    if kind == 0:
        return float(rng.choice([-48.0, 48.0]))
    if kind == 1:
        return 0.0
    return float(np.round(rng.uniform(-48.0, 48.0), 3))


def random_markers(rng, n, sr=SR, max_markers=6, short=1200):
    """One marker set for a file of n samples.  Segments stretched 20x or more are at most `short` samples long (a 100x stretch
    of `short` samples is 2.5 s of warped time at sr = 48 kHz), so that a plan stays a few thousand frames long."""
    k = int(rng.integers(0, max_markers + 1))
    lo, hi = -n // 2 - 20000, n + 20000
    samples = np.sort(rng.integers(lo, hi, size=k))
    if k >= 2 and rng.random() < 0.25:  # two markers on one sample: the bend jumps between them
        i = int(rng.integers(1, k))
        samples[i] = samples[i - 1]
    markers, prev = [], 0
    for j, s in enumerate(samples):
        s = int(s)
        dt = _segment_dtime(rng, s - prev, sr)
        if dt > 19.0 * abs(s - prev) / sr and abs(s - prev) > short:
            dt = dt * short / abs(s - prev)
        pb = _bend(rng)
        if j and rng.random() < 0.3:  # held from the previous marker (at +-48 too)
            pb = markers[-1][3]
        if j and samples[j - 1] == s and rng.random() < 0.5:
            pb = -markers[-1][3] if markers[-1][3] else 48.0  # flips sign at the marker (-48 -> +48 included)
            dt = 0.0
        markers.append((s, 0.0, float(dt), pb))
        prev = s
    if markers and rng.random() < 0.3:  # the last marker exactly at n - 1, as the editor writes one
        s, note, dt, pb = markers[-1]
        if s < n - 1:
            markers.append((n - 1, 0.0, 0.0, 0.0))
    return markers


def marker_sets(seed, count, n_range, sr=SR, **kw):
    """`count` (n, markers) pairs from one seed."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(n_range[0], n_range[1] + 1))
        out.append((n, random_markers(rng, n, sr, **kw)))
    return out
