"""What every frame walker owes a sample that is Inf or NaN, and a take far off full scale (include/melonix_amd.h: "Onset
strength", the sibilant "Features", the STFT's frame, the "Chroma record"): where the bad value is put, which frames hold it
by the header's frame geometry, and the assertions themselves, written once over a function that computes records —
the CPU emulations (tests/test_onset_host.py, test_sibilant_host.py, test_emu.py) and the device (tests/
test_gpu_bad_samples.py) are given the same ones.  A bad sample is data, not a fault: no kernel indexes memory by a
sample's value."""
import numpy as np

BAD = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}
RUNS = (1, 5, 32, 0)  # frames a walker takes; 0: the launch's default
STRADDLED = 5         # the run length at which one position lies in the last frame of a run and the first of the next


def frame_count(n, hop):
    return -(-n // hop)


def holding(n, hop, before, after, s):
    """Frames h of the bulk indexing whose samples [h*hop - before, h*hop + after) include sample s -> bool[frames].
    Onset, sibilant: before = after = 512.  Chroma: 2048, 2048.  STFT: frame h is [(h+1)*hop - N, (h+1)*hop): N - hop, hop."""
    h = np.arange(frame_count(n, hop), dtype=np.int64)
    return (h * hop - before <= s) & (s < h * hop + after)


def positions(n, hop, before, after):
    """name -> sample: the first, the last, mid-file, and one that frames k - 1 and k both hold, k a multiple of STRADDLED:
    the highest sample of frame k - 1, so the bad value enters in the last frame of one run and stays for the first of the next."""
    frames = frame_count(n, hop)
    k = STRADDLED * max(1, frames // (3 * STRADDLED))
    s = (k - 1) * hop + after - 1
    hold = holding(n, hop, before, after, s)
    assert 0 < s < n - 1 and s != n // 2 and k < frames and hold[k - 1] and hold[k] and not hold[:k - 1].any(), (n, hop, k, s)
    return {"first": 0, "last": n - 1, "mid": n // 2, "straddle": s}


def with_bad(w, s, value):
    v = np.array(w, dtype=np.float32, copy=True)
    v[s] = value
    return v


def lagged(hold, lag):
    """The frames `lag` after a holding frame."""
    out = np.zeros_like(hold)
    out[lag:] = hold[:-lag] if lag < len(hold) else False
    return out


def same_whatever_the_run_or_the_split(fn, frames, hold, what):
    """fn(first, count, run) -> records.  The whole curve at every run length, and two launches cut inside the affected frames
    (behind the first holding frame), give the bytes of the default launch."""
    whole = fn(0, frames, 0)
    for run in RUNS[:-1]:
        assert fn(0, frames, run).tobytes() == whole.tobytes(), (what, run)
    cut = int(np.nonzero(hold)[0][0]) + 1
    if 0 < cut < frames:
        for run in (0, STRADDLED):
            two = np.concatenate([fn(0, cut, run), fn(cut, frames - cut, run)])
            assert two.tobytes() == whole.tobytes(), (what, "cut", cut, run)
    return whole


def check_flux(fn, clean_fn, ref, n, hop, lag, s, name, what):
    """The onset flux of a take whose sample s is BAD[name].  fn / clean_fn(first, count, run) -> f32 flux of the bad / the clean
    take; ref: onset_ref.flux of the bad take (NaN case: np.isfinite must agree frame for frame), or None."""
    frames = frame_count(n, hop)
    hold = holding(n, hop, 512, 512, s)
    after = lagged(hold, lag)
    assert hold.any(), what
    got = same_whatever_the_run_or_the_split(fn, frames, hold, what)
    assert got.shape == (frames,)
    if name == "nan":
        assert np.isnan(got[hold | after]).all(), (what, np.nonzero((hold | after) & ~np.isnan(got))[0])
        assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (what, np.nonzero(np.isfinite(got) != np.isfinite(ref))[0])
    else:
        assert not np.isfinite(got[hold]).any(), (what, np.nonzero(hold & np.isfinite(got))[0])
    rest = ~(hold | after)
    clean = clean_fn(0, frames, 0)
    assert np.isfinite(clean).all() and got[rest].tobytes() == clean[rest].tobytes(), (what, np.nonzero(rest & (got != clean))[0])
    return got


def check_features(fn, clean_fn, ref_zc, n, hop, s, what):
    """The sibilant records of a take whose sample s is Inf or NaN; ref_zc: sibilant_ref.features(...)["zero_crossings"] of it."""
    frames = frame_count(n, hop)
    hold = holding(n, hop, 512, 512, s)
    assert hold.any(), what
    got = same_whatever_the_run_or_the_split(fn, frames, hold, what)
    assert not np.isfinite(got["low"][hold] + got["high"][hold]).any(), what
    assert np.array_equal(got["zero_crossings"], ref_zc), what
    clean = clean_fn(0, frames, 0)
    assert got[~hold].tobytes() == clean[~hold].tobytes(), (what, np.nonzero(~hold & (got["low"] != clean["low"]))[0])
    return got


SIB_SCALES = (-30, -8, 8, 30)


def check_scaled_features(got, clean, k, what):
    """Records of the take times 2^k against the clean take's: every product and sum of the transform scales exactly (no
    intermediate leaves the normal range for |k| <= 30 on a take at 1e-4 .. 1), so low and high are the clean bytes times 2^2k,
    the centroid (a ratio) and the crossings (signs) are the clean bytes."""
    for f in ("low", "high"):
        assert np.ldexp(clean[f], 2 * k).astype(np.float32).tobytes() == got[f].tobytes(), (what, k, f)
    assert got["centroid"].tobytes() == clean["centroid"].tobytes(), (what, k)
    assert got["zero_crossings"].tobytes() == clean["zero_crossings"].tobytes(), (what, k)


def check_rows(rows, clean_rows, hold, what):
    """Magnitude rows of a take with a bad sample: a holding frame's row has no finite bin, every other row is the clean bytes."""
    assert hold.any() and not np.isfinite(rows[hold]).any(), (what, np.nonzero(hold & np.isfinite(rows).any(axis=1))[0])
    assert rows[~hold].tobytes() == clean_rows[~hold].tobytes(), (what, np.nonzero(~hold & (rows != clean_rows).any(axis=1))[0])


CHROMA_SCALES = (-140, -40, 20, 60, 66, 80, 126)
CHROMA_ZERO = (-140, -40, 80, 126)  # below the absolute floor / the band maximum overflows: forty zeros (the emulation's)
CHROMA_EXACT = (20, 60)


def scaled(w, k):
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(w, dtype=np.float64), k).astype(np.float32)


def check_scaled_chroma(got, clean, k, what):
    """Records of the `chord` take times 2^k against the clean take's.  The transform scales exactly, and on this take the
    relative floor (rel x the band maximum, about 5e-3) is what decides, not the absolute one, so for k = 20 and 60:
      column 39 (the number of peaks)  the clean bytes: every peak decision compares values that all carry the factor;
      column 38 (the sum of m)         the clean bytes times 2^k;
      columns 0..37                    NOT exact: the place of a peak goes through ln m, and ln(2^k m) rounds where ln m did
                                       not, so the spread over the pitch classes and the phasor move in their last bits.
                                       They are left to check_records against key_ref on the scaled take."""
    got, clean = np.asarray(got, np.float32), np.asarray(clean, np.float32)
    assert np.isfinite(got).all(), (what, k)
    if k in CHROMA_ZERO:
        assert not got.any(), (what, k)
    if k in CHROMA_EXACT:
        assert got[:, 39].tobytes() == clean[:, 39].tobytes(), (what, k)
        assert got[:, 38].tobytes() == np.ldexp(clean[:, 38], k).astype(np.float32).tobytes(), (what, k)
