"""Every frame walker on the GPU with a sample that is NaN, +Inf or -Inf, and with takes far off full scale (include/
melonix_amd.h: "Onset strength", the sibilant "Features", the STFT's frame and mx_pitch, the "Chroma record"): the onset flux,
the sibilant records, the STFT rows with their pitch records and texels, the chroma records, and the chains that read them.
The assertions are tests/bad_samples.py's, the ones the CPU emulations pass (tests/test_onset_host.py, test_sibilant_host.py,
test_emu.py, test_key_host.py); which frames hold a sample comes from the header's frame geometry.  The bad value sits at
the first sample, the last, mid-file, and where the last frame of one run and the first of the next both hold it at
set_frames_per_block(5).  A bad sample is data, not a fault: no kernel indexes memory by a sample's value."""
import numpy as np
import pytest

import bad_samples as B
import onset_ref as R
import sibilant_ref as S
import tempo_ref as T
import test_onset_host as OH
import test_sibilant_host as SH
from test_emu import BAD_N, bad_take
from test_key_host import GUARD_SHARE, Case, check_records, emu as chroma_emu  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SR, HOP = R.SR, R.HOP


class Uploads:
    """Takes on the device, each uploaded once: .of(w) -> Audio; .free()."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def of(self, w):
        self.held.append(self.ctx.upload(w))
        return self.held[-1]

    def free(self):
        for a in self.held:
            a.free()
        self.held = []


@pytest.fixture()
def uploads(gpu_ctx):
    u = Uploads(gpu_ctx)
    yield u
    gpu_ctx.set_frames_per_block(0)
    u.free()


def pinned(ctx, run, call):
    """call() with the context's run length pinned to `run` (0: the default)."""
    ctx.set_frames_per_block(run)
    try:
        return call()
    finally:
        ctx.set_frames_per_block(0)


# ---- onset flux ----
@pytest.mark.parametrize("name", list(B.BAD))
def test_onset_flux(gpu_ctx, uploads, name):
    w = R.notes(0.005)[OH.BAD_TAKE[0]:OH.BAD_TAKE[1]]
    n, ctx = len(w), gpu_ctx
    a = uploads.of(w)
    for lag in (1, 4):
        clean = ctx.onset_flux(a, SR, HOP, lag=lag)
        for pos, s in B.positions(n, HOP, 512, 512).items():
            v = B.with_bad(w, s, B.BAD[name])
            b = uploads.of(v)
            with np.errstate(invalid="ignore"):
                ref = R.flux(v, SR, HOP, lag=lag) if name == "nan" else None
            B.check_flux(lambda first, count, run: pinned(ctx, run, lambda: ctx.onset_flux(b, SR, HOP, first, count, lag=lag)),
                         lambda first, count, run: clean[first:first + count], ref, n, HOP, lag, s, name, (name, pos, lag))


# ---- sibilant features ----
@pytest.mark.parametrize("name", list(B.BAD))
def test_sibilant_features(gpu_ctx, uploads, name):
    w = S.take()[0][SH.BAD_TAKE[0]:SH.BAD_TAKE[1]]
    n, ctx = len(w), gpu_ctx
    clean = ctx.sib_features(uploads.of(w), SR, HOP)
    for pos, s in B.positions(n, HOP, 512, 512).items():
        v = B.with_bad(w, s, B.BAD[name])
        b = uploads.of(v)
        with np.errstate(invalid="ignore"):
            zc = S.features(v, SR, HOP)["zero_crossings"]
        B.check_features(lambda first, count, run: pinned(ctx, run, lambda: ctx.sib_features(b, SR, HOP, first, count)),
                         lambda first, count, run: clean[first:first + count], zc, n, HOP, s, (name, pos))


def test_sibilant_levels_scale_exactly(gpu_ctx, uploads):
    """All of -30, -8, 8, 30 scale exactly on the emulation (tests/test_sibilant_host.py): all four are kept."""
    w = S.take()[0][SH.BAD_TAKE[0]:SH.BAD_TAKE[1]]
    clean = gpu_ctx.sib_features(uploads.of(w), SR, HOP)
    assert clean["low"].all() and clean["high"].all() and np.isfinite(clean["low"] + clean["high"]).all()
    for k in B.SIB_SCALES:
        B.check_scaled_features(gpu_ctx.sib_features(uploads.of(B.scaled(w, k)), SR, HOP), clean, k, "GPU")


# ---- STFT rows, pitch records, texels ----
STFT_PLANS = [("hop", 4096, 256), ("hop", 4096, 375), ("hop", 16384, 512), ("hop", 32768, 375), ("ranges", 4096, 256)]
TEXEL_SCALE = 2.0 ** 15


def check_pitch(pitch, clean_pitch, hold, band, what):
    """Pitch records beside rows that check_rows has passed: a holding frame's record has its bin inside the band and a mag that
    is not finite; every other record is the clean bytes."""
    assert pitch[~hold].tobytes() == clean_pitch[~hold].tobytes(), what
    assert ((pitch["bin"][hold] >= band[0]) & (pitch["bin"][hold] <= band[1])).all(), (what, pitch["bin"][hold])
    assert not np.isfinite(pitch["mag"][hold]).any(), (what, pitch["mag"][hold])


@pytest.mark.parametrize("name", list(B.BAD))
@pytest.mark.parametrize("mode,N,hop", STFT_PLANS)
def test_stft(mxlib, gpu_ctx, oracle, uploads, mode, N, hop, name):
    """Clean rows are compared at the same run length (the sliding windows restart at the head of every run, so a row's last
    bits depend on where the runs start); a holding frame's pitch record does not: whatever its row's non-finite bits, the
    record is the same at every run length and split."""
    ctx, w, n = gpu_ctx, bad_take(), BAD_N
    frames = B.frame_count(n, hop)
    band = mxlib.pitch_band(N, SR)
    ranges = np.array([(h * hop, (h + 1) * hop) for h in range(frames)], dtype=np.int32)
    a = uploads.of(w)
    if mode == "ranges":
        clean = {0: ctx.stft_ranges(a, N, ranges)}
        clean_rgb, clean_rgb_mags = ctx.stft_ranges_rgb(a, N, ranges, TEXEL_SCALE, want_mags=True)
        assert clean_rgb_mags.tobytes() == clean[0][0].tobytes()
    else:
        clean = {run: pinned(ctx, run, lambda: ctx.stft_hop(a, N, hop)) for run in (0, B.STRADDLED)}
    for pos, s in B.positions(n, hop, N - hop, hop).items():
        what = (mode, N, hop, name, pos)
        hold = B.holding(n, hop, N - hop, hop, s)
        v = B.with_bad(w, s, B.BAD[name])
        b = uploads.of(v)
        if mode == "ranges":
            rows, pitch = ctx.stft_ranges(b, N, ranges)
            B.check_rows(rows, clean[0][0], hold, what)
            check_pitch(pitch, clean[0][1], hold, band, what)
            rgb, rgb_mags = ctx.stft_ranges_rgb(b, N, ranges, TEXEL_SCALE, want_mags=True)
            B.check_rows(rgb_mags, clean[0][0], hold, what)
            assert rgb[~hold].tobytes() == clean_rgb[~hold].tobytes(), what
            assert ctx.stft_ranges_rgb(b, N, ranges, TEXEL_SCALE)[~hold].tobytes() == clean_rgb[~hold].tobytes(), what
            cut = int(np.nonzero(hold)[0][0]) + 1
            if cut < frames:
                assert ctx.stft_ranges(b, N, ranges[cut:], want_mags=False)[1][hold[cut:]].tobytes() == pitch[cut:][hold[cut:]].tobytes(), what
            continue
        held = None
        for run in (0, B.STRADDLED):
            rows, pitch = pinned(ctx, run, lambda: ctx.stft_hop(b, N, hop))
            B.check_rows(rows, clean[run][0], hold, what + (run,))
            check_pitch(pitch, clean[run][1], hold, band, what + (run,))
            held = pitch[hold] if held is None else held
            assert pitch[hold].tobytes() == held.tobytes(), what + (run,)
        for run in (1, 32):
            assert pinned(ctx, run, lambda: ctx.stft_hop(b, N, hop, want_mags=False))[1][hold].tobytes() == held.tobytes(), what + (run,)
        cut = int(np.nonzero(hold)[0][0]) + 1
        if cut < frames:
            tail = ctx.stft_hop(b, N, hop, cut, frames - cut, want_mags=False)[1]
            assert tail[hold[cut:]].tobytes() == pitch[cut:][hold[cut:]].tobytes(), what + ("cut", cut)
        if N == 4096 and pos == "straddle":  # the oracle on the same frames: finite exactly where the GPU's rows are
            at = np.nonzero(hold)[0][[0, -1]]
            pick = np.unique(np.concatenate([at, at + [-1, 1]]))
            ref = np.stack([oracle.spec_frame(v, N, int(h) * hop, (int(h) + 1) * hop) for h in pick])
            assert np.array_equal(np.isfinite(ref), np.isfinite(rows[pick])), what


# ---- chroma records over levels ----
@pytest.fixture(scope="module")
def chord(gpu_ctx):
    """The `chord` take with its reference, and the GPU's records of it."""
    import key_ref as K

    case = Case(K.chord())
    a = gpu_ctx.upload(case.w)
    try:
        return case, gpu_ctx.chroma(a, case.sr, case.hop)
    finally:
        a.free()


@pytest.mark.parametrize("k", B.CHROMA_SCALES)
def test_chroma_levels(gpu_ctx, uploads, chroma_emu, chord, k):
    """tests/test_key_host.py::test_levels_far_off_full_scale_on_the_cpu on the device: never Inf or NaN; forty zeros where the
    emulation gives forty zeros; at 2^20 and 2^60 the peak count and the weight scale byte for byte; the other columns inside
    key_ref's bound on the scaled take."""
    clean_case, clean = chord
    case = Case(B.scaled(clean_case.w, k))
    got = gpu_ctx.chroma(uploads.of(case.w), case.sr, case.hop)
    B.check_scaled_chroma(got, clean, k, "GPU")
    want = chroma_emu.chroma(case)
    zero_rows = ~want.any(axis=1)
    assert (k in B.CHROMA_ZERO) == bool(zero_rows.all()) and not got[zero_rows].any(), k
    if k not in B.CHROMA_ZERO:
        assert got[:, 38].all()
        worst, left_out = check_records(got, case, f"2^{k}")
        print(f"2^{k}: worst error / bound {worst:.4f}, {left_out} frames left out by the guard")
        assert left_out <= GUARD_SHARE * len(got)


# ---- the chains ----
def _onset_tuples(on):
    return [(int(o["sample"]), int(o["frame"]), np.float32(o["strength"]), np.float32(o["margin"])) for o in on]


def test_onset_and_tempo_chains_with_a_nan(gpu_ctx, uploads):
    """notes5 with one NaN (tests/test_onset_host.py::test_the_chain_with_a_nan_on_the_cpu): mx_onsets_detect is onset_ref.pick
    on the GPU's own flux, mx_tempo_detect is the reference estimate on that flux, and the clean take's onsets whose decision
    windows do not reach an affected frame survive unchanged."""
    w = R.notes(0.005)
    v = B.with_bad(w, OH.CHAIN_NAN, np.nan)
    a, b = uploads.of(w), uploads.of(v)
    flux = gpu_ctx.onset_flux(b, SR, HOP)
    hold = B.holding(len(w), HOP, 512, 512, OH.CHAIN_NAN)
    assert np.isnan(flux[hold | B.lagged(hold, 1)]).all() and np.isfinite(flux[~(hold | B.lagged(hold, 1))]).all()
    got = _onset_tuples(gpu_ctx.onsets_detect(b, SR, HOP))
    want = R.pick(flux, HOP)
    assert [(g[0], g[1], g[2].tobytes(), g[3].tobytes()) for g in got] == [(p[0], p[1], p[2].tobytes(), p[3].tobytes()) for p in want]
    clean = _onset_tuples(gpu_ctx.onsets_detect(a, SR, HOP))
    keep = OH.chain_survivors(clean, got, len(w), "GPU")
    assert len(clean) == 6 and len(keep) >= 0.75 * len(clean)
    T.same_estimate(gpu_ctx.tempo_detect(b, SR, HOP, want_windows=True), T.estimate(flux, SR, HOP))


def _segment_tuples(segs):
    return [(int(s["start_sample"]), int(s["end_sample"]), int(s["first_frame"]), int(s["frames"]), np.float32(s["share"]), np.float32(s["level"]))
            for s in segs]


def test_sibilant_chain_with_a_nan(gpu_ctx, uploads):
    """The synthetic take with one NaN inside a vowel: mx_sibilants_detect is sibilant_ref.segments on the GPU's own records, and
    the clean take's segments whose decision windows do not reach a holding frame survive unchanged."""
    w = S.take()[0]
    v = B.with_bad(w, SH.SIB_CHAIN_NAN, np.nan)
    a, b = uploads.of(w), uploads.of(v)
    rec = gpu_ctx.sib_features(b, SR, HOP)
    hold = B.holding(len(w), HOP, 512, 512, SH.SIB_CHAIN_NAN)
    assert not np.isfinite(rec["low"][hold] + rec["high"][hold]).any() and np.isfinite(rec["low"][~hold] + rec["high"][~hold]).all()
    got = _segment_tuples(gpu_ctx.sibilants_detect(b, SR, HOP))
    want = S.segments(rec, HOP)
    assert [g[:4] + (g[4].tobytes(), g[5].tobytes()) for g in got] == [tuple(s[:4]) + (s[4].tobytes(), s[5].tobytes()) for s in want]
    clean = _segment_tuples(gpu_ctx.sibilants_detect(a, SR, HOP))
    keep = SH.segment_survivors(clean, got, len(w), "GPU")
    assert len(clean) == 3 and len(keep) >= 0.75 * len(clean)
