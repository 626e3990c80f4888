"""Every kernel's addressing past 4 GiB and at the longest take the header admits (tests/far_take.py: N_MAX samples, an 8 GiB
image of zeros with islands of signal astride byte offsets 2, 4 and 6 GiB, astride the sample where the 44.1 -> 48 kHz converter's
output index passes 2^31, and on the take's last samples).

The common rule: an entry point run on the far take over the frames (steps, outputs) of an island must leave THE SAME BYTES as
the same call on the control — the island's samples uploaded as a take of their own, at low addresses — through the `_dev` forms
into buffers with 1 KiB of 0xA5 behind each output, which must survive; the control's output must be about signal; and the
control's output is then held to its family's reference by its family's checker, imported from the module that owns it.  The far
output is right by two steps that each exist on their own, and no number in this file is a tolerance.

The candidate ladder's checker is not a function of its own
(tests/test_gpu_f0_decode.py): the ladder's track is held to the plain tracker's bytes — which yin_ref.check_parity holds to the
reference — and its slots to the track's, field for field, as that module does."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import far_take as FT
import key_ref as K
import loudness_ref as L
import onset_ref as OR
import pcm_extremes as P
import psola_ref
import resample_ref as R
import sibilant_ref as S
import truepeak_ref as T
import yin_ref as Y
from conftest import SR, DevBuf, mag_tol
from far_take import far  # noqa: F401  (the module's far-take fixture)
from test_gpu_onset import flux_tol
from test_gpu_psola import _hand_plan
from test_gpu_psola import check as psola_check
from test_gpu_psola_formant import _hand_fplan
from test_gpu_stft import _check_pitch
from test_key_host import GUARD_SHARE, Case, check_records
from test_sibilant_host import check_features

pytestmark = pytest.mark.gpu

GUARD = 1024
N_MAX = FT.N_MAX
INT32_MAX = 2 ** 31 - 1
ISLANDS = FT.SPAN_ISLANDS  # B2G, B4G, B6G, END
ODD_HOP = 375


@pytest.fixture(scope="module")
def controls(gpu_ctx):
    """(island, unit, whole=False) -> (q, w, the uploaded control).  whole: w cut to a whole number of units (trailing zeros
    dropped; never for END, whose control ends where the far take ends), for the families whose last record of a take differs
    from a full one."""
    made = {}

    def get(island, unit, whole=False):
        key = (island, unit, whole and island != "END")
        if key not in made:
            q, w = FT.window(island, unit)
            if key[2]:
                w = w[:len(w) // unit * unit]
                assert len(w) - (FT.span(island)[1] - q) >= FT.MARGIN - unit
            w.setflags(write=False)
            made[key] = (q, w, gpu_ctx.upload(w))
        return made[key]

    yield get
    for _, _, a in made.values():
        a.free()


@contextlib.contextmanager
def run_pinned(ctx, g):
    ctx.set_frames_per_block(g)
    try:
        yield
    finally:
        ctx.set_frames_per_block(0)


class Outs:
    """One 0xA5 device buffer per size (None: an output not wanted) with GUARD bytes behind it.  The fill is a hipMemset on the
    null stream, the launches go to the context's non-blocking stream: the device is synchronised in between."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.bufs = [None if s is None else DevBuf(s + GUARD, fill=0xA5) for s in self.sizes]
        live = [b for b in self.bufs if b is not None]
        assert live and live[0].hip.hipDeviceSynchronize() == 0
        self.ptrs = [None if b is None else b.ptr for b in self.bufs]

    def fetch(self, what):
        out = []
        for s, b in zip(self.sizes, self.bufs):
            if b is None:
                out.append(None)
                continue
            raw = b.read(np.uint8)
            assert np.all(raw[s:] == 0xA5), f"{what}: bytes written behind an output (first at +{int(np.argmax(raw[s:] != 0xA5))})"
            out.append(raw[:s])
        return out

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def same_bytes(f, c, what):
    if not np.array_equal(f, c):
        bad = np.flatnonzero(f != c)
        raise AssertionError(f"{what}: the far take's output differs from the control's in {len(bad)} of {len(c)} bytes, "
                             f"first at byte {int(bad[0])}, last at byte {int(bad[-1])}")


def pair(ctx, sizes, far_call, ctl_call, what):
    """far_call(*ptrs) and ctl_call(*ptrs) into guarded buffers of `sizes` bytes -> the control's outputs (uint8 arrays, None
    where the size is None), after asserting that the far take's are the same bytes and that every guard stands."""
    fo, co = Outs(sizes), Outs(sizes)
    try:
        far_call(*fo.ptrs)
        ctl_call(*co.ptrs)
        ctx.synchronize()
        f, c = fo.fetch(what + ", far"), co.fetch(what + ", control")
    finally:
        fo.free()
        co.free()
    for k, (a, b) in enumerate(zip(f, c)):
        if b is not None:
            same_bytes(a, b, f"{what}, output {k}")
    return c


def frames_of(mx, n, hop):
    return int(mx.frame_count(n, hop))


# ---- span forms: the STFT ------------------------------------------------------------------------------------------------------

STFT_PLANS = [(4096, 256), (4096, 512), (4096, 375), (4096, 3000), (16384, 512), (16384, 375), (32768, 1024), (32768, 375)]
WIDE_BAND = (5, 256)  # reaches bin 256: the XOR image and the transform-side pick (tests/test_gpu_t1q.py)


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("N,hop", STFT_PLANS)
def test_stft_hop(gpu_ctx, mxlib, oracle, far, controls, island, N, hop):
    """mx_stft_hop_dev with 32-frame runs (the default run for so few frames is 1 and would never slide), the same relative first
    frame and count on both sides so that the run heads coincide: rows and records, rows alone, records alone; at N = 4096 with
    the default band (row-side pick, q-major image) and with one that reaches bin 256.

    The circular-window kernels (N = 16384 and 32768 at hop 375) keep a frame at the circular position (frame start) mod 2T of
    their register image (stft_core.h circ_geo; 2T = 512 and 1024), and a frame's last bits depend on it: their rows are the same
    under a translation by a multiple of 2T only.  Their unit is lcm(hop, 1024); both calls then start `skip` frames into the
    control, MARGIN before the island."""
    circular = N >= 16384 and hop == ODD_HOP
    q, w, ctl = controls(island, math.lcm(hop, 1024) if circular else hop)
    total, M = frames_of(mxlib, len(w), hop), N // 2
    skip = max(FT.span(island)[0] - q - FT.MARGIN, 0) // hop
    F, first = total - skip, q // hop + skip
    assert q % hop == 0 and (skip == 0 or circular) and first + F <= frames_of(mxlib, N_MAX, hop)
    if island == "END":
        assert first + F == frames_of(mxlib, N_MAX, hop)  # the far take's last frame is the control's last frame
    default = mxlib.pitch_band(N, SR)
    assert default == oracle.pitch_band(N, SR) and (N != 4096 or default[1] < 256)
    with run_pinned(gpu_ctx, 32):
        for band in [(-1, -1)] + ([WIDE_BAND] if N == 4096 else []):
            what = f"stft_hop_dev {island} N={N} hop={hop} band={band}"

            def far_call(m, p):
                gpu_ctx.stft_hop_dev(far.audio, N, hop, first, F, m, p, band=band)

            def ctl_call(m, p):
                gpu_ctx.stft_hop_dev(ctl, N, hop, skip, F, m, p, band=band)

            rows, recs = pair(gpu_ctx, [F * M * 4, F * 8], far_call, ctl_call, what)
            rows_alone, _ = pair(gpu_ctx, [F * M * 4, None], far_call, ctl_call, what + ", rows alone")
            _, recs_alone = pair(gpu_ctx, [None, F * 8], far_call, ctl_call, what + ", records alone")
            assert np.array_equal(rows_alone, rows) and np.array_equal(recs_alone, recs), what
            rows, recs = rows.view(np.float32).reshape(F, M), recs.view(mxlib.PITCH_DTYPE)
            assert rows.any() and (recs["mag"] > 0).sum() > F // 4, what  # about signal
            assert np.array_equal(recs["mag"], rows[np.arange(F), recs["bin"]]), what
            pick = skip + np.arange(F)  # the control against the oracle, every frame
            ref = np.stack([oracle.spec_frame(w, N, int(h) * hop, (int(h) + 1) * hop) for h in pick])
            tol = mag_tol(ref)
            err = np.abs(rows - ref)
            print(f"{what}: {F} frames, worst error / bound {float((err / tol).max()):.4f}")
            assert (err <= tol).all(), what
            lo, hi = default if band == (-1, -1) else band
            _check_pitch(recs, ref, (lo, hi), tol)


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("N", [4096, 16384, 32768])
def test_stft_ranges_and_texels(gpu_ctx, mxlib, oracle, far, controls, island, N):
    """mx_stft_ranges_dev and mx_stft_ranges_rgb_dev on int32 pairs: the far counterparts of the control's columns (display
    columns, one sample, a reversed pair, a wide one, the take's last samples and beyond); on END also the largest ends an int32
    holds."""
    from melonix_amd import _capi
    lib = _capi.lib()
    q, w, ctl = controls(island, ODD_HOP)
    n, M, k = len(w), N // 2, 2.0 ** 15
    lo = FT.span(island)[0] - q
    cols = [(lo + i * 375, lo + (i + 1) * 375) for i in range(0, 600, 25)]
    cols += [(lo + 100000, lo + 100001), (lo + 5000, lo + 4000), (lo + 1000, lo + 60000), (lo - 300, lo + 75), (n - 375, n), (n - 1, n),
             (n, n + 375), (0, 256)]
    far_cols = [(s + q, e + q) for s, e in cols]
    if island == "END":
        assert n + q == N_MAX
        far_cols += [(N_MAX - 100, N_MAX), (N_MAX - 1, INT32_MAX), (N_MAX, INT32_MAX)]
        cols += [(n - 100, n), (n - 1, INT32_MAX - q), (n, INT32_MAX - q)]
    cnt = len(cols)
    rc, rf = np.array(cols, dtype=np.int32), np.array(far_cols, dtype=np.int32)
    assert np.array_equal(rf.astype(np.int64) - rc, np.full((cnt, 2), q))
    d_rc, d_rf = DevBuf(rc.nbytes), DevBuf(rf.nbytes)
    d_rc.write(rc)
    d_rf.write(rf)
    try:
        what = f"stft_ranges_dev {island} N={N}"
        rows, recs = pair(gpu_ctx, [cnt * M * 4, cnt * 8],
                          lambda m, p: gpu_ctx.stft_ranges_dev(far.audio, N, d_rf.ptr, cnt, m, p),
                          lambda m, p: gpu_ctx.stft_ranges_dev(ctl, N, d_rc.ptr, cnt, m, p), what)

        def texels(audio, d_r):
            return lambda m, t: _capi.check(lib.mx_stft_ranges_rgb_dev(gpu_ctx.handle, audio.handle, N, C.c_void_p(d_r.ptr), cnt,
                                                                       k, C.c_void_p(m) if m else None, C.c_void_p(t)))

        rows_t, rgb = pair(gpu_ctx, [cnt * M * 4, cnt * M * 3], texels(far.audio, d_rf), texels(ctl, d_rc), what + ", texels")
        _, rgb_alone = pair(gpu_ctx, [None, cnt * M * 3], texels(far.audio, d_rf), texels(ctl, d_rc), what + ", texels alone")
    finally:
        d_rc.free()
        d_rf.free()
    assert np.array_equal(rows_t, rows) and np.array_equal(rgb_alone, rgb)
    rows, recs, rgb = rows.view(np.float32).reshape(cnt, M), recs.view(mxlib.PITCH_DTYPE), rgb.reshape(cnt, M, 3)
    assert rows[:24].any(axis=1).all() and (recs["mag"] > 0).sum() >= 24 and rgb.any()  # about signal
    ref = np.stack([oracle.spec_frame(w, N, s, e) for s, e in cols])
    tol = mag_tol(ref)
    err = np.abs(rows - ref)
    print(f"{what}: {cnt} columns, worst error / bound {float((err / tol).max()):.4f}")
    assert (err <= tol).all(), what
    _check_pitch(recs, ref, mxlib.pitch_band(N, SR), tol)
    assert np.array_equal(recs["mag"], rows[np.arange(cnt), recs["bin"]])
    assert np.array_equal(rgb, np.stack([oracle.colormap(m, k) for m in rows])), what


# ---- span forms: the frame walkers --------------------------------------------------------------------------------------------

def walker_pair(gpu_ctx, mxlib, far, controls, island, hop, sizes_per_frame, call, what):
    """call(audio, first, count, *ptrs) on both takes with the run pinned to 1 and to 32 -> (q, w, F, the control's outputs of
    the 32-frame runs)."""
    q, w, ctl = controls(island, hop)
    F, first = frames_of(mxlib, len(w), hop), q // hop
    assert first * hop == q
    if island == "END":
        assert first + F == frames_of(mxlib, N_MAX, hop)
    out = None
    for run in (1, 32):
        with run_pinned(gpu_ctx, run):
            out = pair(gpu_ctx, [None if s is None else F * s for s in sizes_per_frame], lambda *p: call(far.audio, first, F, *p),
                       lambda *p: call(ctl, 0, F, *p), f"{what} {island} hop={hop} run={run}")
    return q, w, F, out


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("hop", [256, ODD_HOP])
def test_f0_track_and_candidates(gpu_ctx, mxlib, far, controls, island, hop):
    """mx_f0_track_dev and mx_f0_candidates_dev.  The track against yin_ref; the ladder's own track is the plain one's bytes,
    and where the plain record is under the threshold exactly one slot holds its tau, period and aperiodicity."""
    q, w, F, (track,) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [16],
                                    lambda a, first, count, p: gpu_ctx.f0_track_dev(a, SR, hop, first, count, p), "f0_track_dev")
    _, _, _, (track2, cands) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [16, 64],
                                           lambda a, first, count, t, c: gpu_ctx.f0_candidates_dev(a, SR, hop, first, count, t, c),
                                           "f0_candidates_dev")
    _, _, _, (_, cands_alone) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [None, 64],
                                            lambda a, first, count, t, c: gpu_ctx.f0_candidates_dev(a, SR, hop, first, count, t, c),
                                            "f0_candidates_dev, no track")
    assert np.array_equal(track2, track) and np.array_equal(cands_alone, cands)
    track, cands = track.view(mxlib.F0_DTYPE), cands.view(mxlib.F0_CAND_DTYPE).reshape(F, 4)
    tmin, tmax = Y.tau_range(SR)
    recs, dp = Y.track(w, SR, hop)
    Y.check_parity(track, recs, dp, tmin, tmax, 0.15, f"far take {island} hop={hop}")
    under = np.nonzero((track["tau"] > 0) & (track["aperiodicity"] < np.float32(0.15)))[0]
    assert len(under) > F // 4  # about signal: voiced frames
    hit = cands["tau"][under] == track["tau"][under][:, None]
    assert (hit.sum(axis=1) == 1).all()
    slot = np.argmax(hit, axis=1)
    for k in ("period", "aperiodicity"):
        assert cands[k][under, slot].tobytes() == track[k][under].tobytes(), k


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("hop", [256, ODD_HOP])
def test_onset_flux(gpu_ctx, mxlib, far, controls, island, hop):
    """mx_onset_flux_dev at lag 1 and 4 against onset_ref.flux within test_gpu_onset.flux_tol."""
    for lag in (1, 4):
        q, w, F, (flux,) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [4],
                                       lambda a, first, count, p: gpu_ctx.onset_flux_dev(a, SR, hop, first, count, p, lag=lag),
                                       f"onset_flux_dev lag={lag}")
        flux = flux.view(np.float32)
        ref = OR.flux(w, SR, hop, lag=lag)
        assert flux.shape == ref.shape and np.all(np.isfinite(flux)) and (flux > 0).sum() > F // 4
        err, tol = np.abs(flux - ref).max(), flux_tol(ref)
        print(f"onset_flux {island} hop={hop} lag={lag}: max|flux| {ref.max():.3f}  worst error {err:.3e}  bound {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("hop", [256, ODD_HOP])
def test_sib_features(gpu_ctx, mxlib, far, controls, island, hop):
    """mx_sib_features_dev against sibilant_ref.features by test_sibilant_host.check_features."""
    q, w, F, (feat,) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [16],
                                   lambda a, first, count, p: gpu_ctx.sib_features_dev(a, SR, hop, first, count, p), "sib_features_dev")
    feat = feat.view(mxlib.SIB_FEAT_DTYPE)
    assert (feat["low"] > 0).sum() > F // 4 and (feat["zero_crossings"] > 0).sum() > F // 4
    check_features(feat, S.features(w, SR, hop), f"far take {island} hop={hop}")


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("hop", [256, ODD_HOP])
def test_chroma(gpu_ctx, mxlib, far, controls, island, hop):
    """mx_chroma_dev against key_ref.chroma by test_key_host.check_records."""
    q, w, F, (rec,) = walker_pair(gpu_ctx, mxlib, far, controls, island, hop, [4 * K.COLS],
                                  lambda a, first, count, p: gpu_ctx.chroma_dev(a, SR, hop, first, count, p), "chroma_dev")
    rec = rec.view(np.float32).reshape(F, K.COLS)
    assert (rec[:, 39] > 0).sum() > F // 4  # frames with peaks
    worst, left_out = check_records(rec, Case(w, sr=SR, hop=hop), f"far take {island} hop={hop}")
    print(f"chroma {island} hop={hop}: {F} frames, {left_out} left out by the guard, worst error / bound {worst:.4f}")
    assert left_out <= GUARD_SHARE * F


# ---- span forms: loudness and true-peak steps -------------------------------------------------------------------------------

@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("sr", [48000, 44100])
def test_loudness_steps(gpu_ctx, mxlib, far, controls, island, sr):
    """mx_loudness_steps_dev, the control a whole number of groups from a group's start: the references bytes."""
    unit = L.G * L.geometry(0, sr)[0]
    q, w, ctl = controls(island, unit, whole=True)
    steps = mxlib.loudness_step_count(len(w), sr)
    groups, first_group = -(-steps // L.G), q // unit
    if island == "END":
        assert mxlib.loudness_step_count(N_MAX, sr) == L.G * first_group + steps and steps % L.G  # the partial last group
    else:
        assert steps == L.G * groups
    (got,) = pair(gpu_ctx, [steps * 16], lambda p: gpu_ctx.loudness_steps_dev(far.audio, sr, first_group, groups, p),
                  lambda p: gpu_ctx.loudness_steps_dev(ctl, sr, 0, groups, p), f"loudness_steps_dev {island} sr={sr}")
    got = got.view(L.STEP_DTYPE)
    assert (got["energy"] > 0).sum() > steps // 4 and (got["peak"] > 0.4).any()
    assert got.tobytes() == L.steps(w, sr, mxlib.loudness_coeffs(sr)).tobytes()


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("sr", [48000, 44100])
def test_true_peak_steps(gpu_ctx, mxlib, far, controls, island, sr):
    """mx_true_peak_steps_dev from a step's start: the references bytes."""
    S_ = T.step_samples(sr)
    unit = L.G * S_
    q, w, ctl = controls(island, unit, whole=True)
    steps, first = mxlib.loudness_step_count(len(w), sr), q // S_
    if island == "END":
        assert mxlib.loudness_step_count(N_MAX, sr) == first + steps and len(w) % S_
    (got,) = pair(gpu_ctx, [steps * 8], lambda p: gpu_ctx.true_peak_steps_dev(far.audio, sr, first, steps, p),
                  lambda p: gpu_ctx.true_peak_steps_dev(ctl, sr, 0, steps, p), f"true_peak_steps_dev {island} sr={sr}")
    got = got.view(T.STEP_DTYPE)
    assert (got["true_peak"] > 0).sum() > steps // 4
    assert got.tobytes() == T.records(w, sr, mxlib.true_peak_taps()).tobytes()


# ---- span forms: the converter ------------------------------------------------------------------------------------------------

def _resample_case(mxlib, controls, island, pair_, unit):
    p, t = R.plan(*pair_), mxlib.resample_taps(*pair_)
    q, w, ctl = controls(island, unit)
    assert q % p["M"] == 0
    return p, t, q, w, ctl, q // p["M"] * p["L"]


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("pair_", [(48000, 44100), (96000, 48000)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_resample(gpu_ctx, mxlib, far, controls, island, pair_):
    """mx_resample_dev: the window starts on a multiple of M, the output offset is the matching multiple of L; every output of the
    control, the reference's bytes."""
    p, t, q, w, ctl, qo = _resample_case(mxlib, controls, island, pair_, 4800)
    m = mxlib.resample_length(len(w), *pair_)
    assert m == R.length(len(w), p)
    if island == "END":
        assert qo + m == mxlib.resample_length(N_MAX, *pair_)
    (got,) = pair(gpu_ctx, [m * 4], lambda o: gpu_ctx.resample_dev(far.audio, pair_[0], pair_[1], qo, m, o),
                  lambda o: gpu_ctx.resample_dev(ctl, pair_[0], pair_[1], 0, m, o), f"resample_dev {island} {pair_}")
    assert (got.view(np.float32) != 0).sum() > m // 2
    assert got.tobytes() == R.resample(w, p, t).tobytes()


@pytest.mark.parametrize("island", ["J31", "END"])
def test_resample_outputs_past_2_31(gpu_ctx, mxlib, far, controls, island):
    """44 100 -> 48 000: the 4096 outputs astride output index 2^31 (J31) and the last 4096 of the mx_resample_length outputs
    (END), whose indices lie above 2^31."""
    pair_ = (44100, 48000)
    p, t, q, w, ctl, qo = _resample_case(mxlib, controls, island, pair_, 4410)
    m_far = mxlib.resample_length(N_MAX, *pair_)
    assert m_far == 2337325836
    first = 2 ** 31 - 2048 if island == "J31" else m_far - 4096
    assert first - qo >= 0 and first - qo + 4096 <= R.length(len(w), p) and first + 4096 > 2 ** 31
    if island == "END":
        assert first - qo + 4096 == R.length(len(w), p)
    (got,) = pair(gpu_ctx, [4096 * 4], lambda o: gpu_ctx.resample_dev(far.audio, pair_[0], pair_[1], first, 4096, o),
                  lambda o: gpu_ctx.resample_dev(ctl, pair_[0], pair_[1], first - qo, 4096, o), f"resample_dev {island} {pair_}")
    assert (got.view(np.float32) != 0).sum() > 2048
    assert got.tobytes() == R.resample(w, p, t, first - qo, 4096).tobytes()


# ---- gathers with small outputs: records built by hand (the device forms do not validate them) --------------------------------

def _steps(mxlib, island, q, n):
    """A schedule of 36 steps over the island (control coordinates): rates either side of 1, staged grains and long ones, the
    outputs from 0; on END the last steps read the take's last samples.  -> (steps, nsamples)"""
    lo = FT.span(island)[0] - q
    rows, off = [], 0
    for k in range(36):
        rate = (1.0, 0.5, 1.5, 2.0, 0.75, 1.25)[k % 6]
        sz = (37, 29, 42, 48, 300, 1000)[(k // 2) % 6]
        glen = P.LONG_GRAIN if k % 4 == 3 else int(sz * rate) + 1
        assert (sz - 1) * rate < glen
        g0 = lo + 1000 + 7001 * k
        if island == "END" and k >= 32:
            g0 = n - glen - (35 - k) * 3  # the last one ends on the take's last sample
        rows.append((0.0, g0, glen, rate, 0.25, sz, off))
        off += sz
    st = np.zeros(len(rows), mxlib.STEP_DTYPE)
    for f, col in zip(("cursor", "grain_start", "grain_len", "rate", "next_first", "sz", "out_offset"), zip(*rows)):
        st[f] = col
    assert (st["grain_start"] >= lo).all() and (st["grain_start"] + st["grain_len"] <= n).all()
    return st, off + P.ARMS_TAIL


@pytest.mark.parametrize("island", ISLANDS)
def test_resynth(gpu_ctx, mxlib, oracle, far, controls, island):
    """mx_resynth_dev: grain_start in the island, out_offset from 0; the control's schedule is the same with grain_start - q.  f32
    against the lerp restated (pcm_extremes.arms_expected, same_floats), int16 the oracle's conversion of it."""
    q, w, ctl = controls(island, 256)
    st, total = _steps(mxlib, island, q, len(w))
    st_far = st.copy()
    st_far["grain_start"] = (st["grain_start"].astype(np.int64) + q).astype(np.int32)
    assert (st_far["grain_start"].astype(np.int64) - st["grain_start"] == q).all()
    d_c, d_f = DevBuf(st.nbytes), DevBuf(st.nbytes)
    d_c.write(st)
    d_f.write(st_far)
    try:
        f32, i16 = pair(gpu_ctx, [total * 4, total * 2], lambda f, i: gpu_ctx.resynth_dev(far.audio, d_f.ptr, len(st), total, f, i),
                        lambda f, i: gpu_ctx.resynth_dev(ctl, d_c.ptr, len(st), total, f, i), f"resynth_dev {island}")
        _, i16_alone = pair(gpu_ctx, [None, total * 2], lambda f, i: gpu_ctx.resynth_dev(far.audio, d_f.ptr, len(st), total, f, i),
                            lambda f, i: gpu_ctx.resynth_dev(ctl, d_c.ptr, len(st), total, f, i), f"resynth_dev {island}, int16 alone")
    finally:
        d_c.free()
        d_f.free()
    f32, i16 = f32.view(np.float32), i16.view(np.int16)
    assert np.array_equal(i16_alone.view(np.int16), i16) and (f32 != 0).sum() > total // 2
    want, _ = P.arms_expected(w, st, total)
    P.same_floats(f32, want, f"resynth_dev {island}")
    assert np.array_equal(i16, oracle.pcm_to_i16(want))


def _psola_sets(island, q, n, formant):
    """name -> (records in control coordinates, nsamples): grains that read across the island's first sample, its middle, and on
    END the take's last samples (and the trailing pad behind them); out_lo from 0."""
    lo = FT.span(island)[0] - q
    Ln = 5999
    places = {"first samples": lo - 3000, "middle": lo + 120000}
    if island == "END":
        places["last samples"] = n - Ln
    out = {}
    for name, at in places.items():
        if formant:
            g = _hand_fplan(Ln, 256.0, 64.0, [32768, 70001, 65536, 99999, 131072], src_q=12345, src_shift=at)
        else:
            g = _hand_plan(Ln, 256.0, 64.0, src_off=at)
        assert g["out_lo"].min() == 0
        out[name] = (g, Ln)
    return out


@pytest.mark.parametrize("island", ISLANDS)
@pytest.mark.parametrize("formant", [False, True], ids=["plain", "formant"])
def test_psola_synth(gpu_ctx, mxlib, far, controls, island, formant):
    """mx_psola_synth_dev and mx_psola_synth_formant_dev: src_off / src_idx moved into the island, and back by q for the control.
    f32 and int16 against psola_ref.render by test_gpu_psola.check."""
    q, w, ctl = controls(island, 256)
    field = "src_idx" if formant else "src_off"
    synth = gpu_ctx.psola_synth_formant_dev if formant else gpu_ctx.psola_synth_dev
    for name, (g, Ln) in _psola_sets(island, q, len(w), formant).items():
        what = f"psola_synth{'_formant' if formant else ''}_dev {island}, {name}"
        g_far = g.copy()
        g_far[field] = (g[field].astype(np.int64) + q).astype(np.int32)
        assert (g_far[field].astype(np.int64) - g[field] == q).all()
        d_c, d_f = DevBuf(g.nbytes), DevBuf(g.nbytes)
        d_c.write(g)
        d_f.write(g_far)
        try:
            f32, i16 = pair(gpu_ctx, [Ln * 4, Ln * 2], lambda f, i: synth(far.audio, d_f.ptr, len(g), Ln, f, i),
                            lambda f, i: synth(ctl, d_c.ptr, len(g), Ln, f, i), what)
            _, i16_alone = pair(gpu_ctx, [None, Ln * 2], lambda f, i: synth(far.audio, d_f.ptr, len(g), Ln, f, i),
                                lambda f, i: synth(ctl, d_c.ptr, len(g), Ln, f, i), what + ", int16 alone")
        finally:
            d_c.free()
            d_f.free()
        f32, i16 = f32.view(np.float32), i16.view(np.int16)
        assert np.array_equal(i16_alone.view(np.int16), i16) and (f32 != 0).sum() > Ln // 4, what
        psola_check(f32, i16, psola_ref.render(w, g, Ln), what)


# ---- whole-take forms ---------------------------------------------------------------------------------------------------------

ZEROS = (10 ** 9, 100000)  # a stretch of the far take that holds no island: (first sample, samples)


def _gain_points(mxlib):
    b4, end = FT.STARTS["B4G"], FT.STARTS["END"]
    pts = [(b4 + 1000, 0.37), (b4 + 100000, 2.5), (b4 + 200001, 0.5), (end + 5000, 1.5), (end + 260000, 0.01), (N_MAX - 3, 1.0)]
    return np.array([(s, np.float32(a)) for s, a in pts], dtype=mxlib.GAIN_POINT_DTYPE)


def test_audio_gain(gpu_ctx, mxlib, far, controls):
    """mx_audio_gain_dev over the whole far take: points inside B4G and END (B2G lies before the first, B6G on the ramp between
    them), translated by q for each control; windows read back with mx_audio_download; sibilant_ref.apply_gain's bytes."""
    far.need(FT.IMAGE * 4, "the gained far take")
    pts = _gain_points(mxlib)
    d_p = DevBuf(pts.nbytes)
    d_p.write(pts)
    got, out = {}, None
    try:
        out = gpu_ctx.audio_gain_dev(far.audio, d_p.ptr, len(pts))
        gpu_ctx.synchronize()
        assert out.n == N_MAX
        for island in ISLANDS:
            q, w, _ = controls(island, 4800)
            got[island] = gpu_ctx.audio_download(out, q, len(w))
        zeros = gpu_ctx.audio_download(out, *ZEROS)
        pads = gpu_ctx.audio_download(out, -FT.PAD, FT.PAD), gpu_ctx.audio_download(out, N_MAX, FT.PAD)
    finally:
        if out is not None:
            out.free()
        far.release(FT.IMAGE * 4)
        d_p.free()
    assert not zeros.view(np.uint32).any() and not pads[0].view(np.uint32).any() and not pads[1].view(np.uint32).any()
    for island in ISLANDS:
        q, w, ctl = controls(island, 4800)
        moved = pts.copy()
        moved["sample"] = (pts["sample"].astype(np.int64) - q).astype(np.int32)
        assert (moved["sample"].astype(np.int64) + q == pts["sample"]).all()
        d_m = DevBuf(moved.nbytes)
        d_m.write(moved)
        b = None
        try:
            b = gpu_ctx.audio_gain_dev(ctl, d_m.ptr, len(moved))
            gpu_ctx.synchronize()
            c = gpu_ctx.audio_download(b)
        finally:
            if b is not None:
                b.free()
            d_m.free()
        same_bytes(got[island].view(np.uint8), c.view(np.uint8), f"audio_gain_dev {island}")
        assert (c != w).sum() > FT.ISLAND // 2  # about signal, and the gain is not 1
        want = S.apply_gain(w, [(int(s), a) for s, a in moved])
        assert c.tobytes() == want.tobytes(), island


def test_audio_limit(gpu_ctx, mxlib, far, controls):
    """mx_audio_limit_dev over the whole far take with its int16 output, under a ceiling the islands exceed; windows of both read
    back; truepeak_ref.limit's bytes."""
    sr, c, A = 48000, np.float32(0.25), T.default_lookahead(48000)
    extra = FT.IMAGE * 4 + N_MAX * 2 + GUARD
    far.need(extra, "the limited far take and its int16")
    got, got16, out, pcm = {}, {}, None, None
    try:
        pcm = DevBuf(N_MAX * 2 + GUARD, fill=0xA5)
        assert pcm.hip.hipDeviceSynchronize() == 0
        out = gpu_ctx.limit_dev(far.audio, sr, d_pcm16=pcm.ptr, ceiling_amp=c)
        gpu_ctx.synchronize()
        assert out.n == N_MAX
        for island in ISLANDS:
            q, w, _ = controls(island, 4800)
            got[island] = gpu_ctx.audio_download(out, q, len(w))
            got16[island] = pcm.read(np.int16, offset=2 * q, count=len(w))
        zeros = gpu_ctx.audio_download(out, *ZEROS)
        zeros16 = pcm.read(np.int16, offset=2 * ZEROS[0], count=ZEROS[1])
        pads = gpu_ctx.audio_download(out, -FT.PAD, FT.PAD), gpu_ctx.audio_download(out, N_MAX, FT.PAD)
        assert np.all(pcm.read(np.uint8, offset=2 * N_MAX, count=GUARD) == 0xA5)
    finally:
        if out is not None:
            out.free()
        if pcm is not None:
            pcm.free()
        far.release(extra)
    assert not zeros.view(np.uint32).any() and not zeros16.any()
    assert not pads[0].view(np.uint32).any() and not pads[1].view(np.uint32).any()
    taps = mxlib.true_peak_taps()
    for island in ISLANDS:
        q, w, ctl = controls(island, 4800)
        c16 = Outs([len(w) * 2])
        b = None
        try:
            b = gpu_ctx.limit_dev(ctl, sr, d_pcm16=c16.ptrs[0], ceiling_amp=c)
            gpu_ctx.synchronize()
            cf = gpu_ctx.audio_download(b)
            (ci,) = c16.fetch(f"audio_limit_dev {island}, control")
        finally:
            if b is not None:
                b.free()
            c16.free()
        same_bytes(got[island].view(np.uint8), cf.view(np.uint8), f"audio_limit_dev {island}")
        same_bytes(got16[island].view(np.uint8), ci, f"audio_limit_dev {island}, int16")
        assert np.abs(cf).max() <= c and (cf != w).sum() > FT.ISLAND // 4  # the limiter worked
        want, want16 = T.limit(w, sr, taps, c, A)
        assert cf.tobytes() == want.tobytes() and ci.tobytes() == want16.tobytes(), island


# ---- the two refusals at the limit ----------------------------------------------------------------------------------------------

def test_wrap_device_refuses_more_than_the_kernels_can_index(gpu_ctx, mxlib, far):
    """mx_audio_wrap_device at the bound and one above it: upload's bound and message, the handle untouched."""
    from melonix_amd import _capi
    lib = _capi.lib()
    h = C.c_void_p(0x5A5A)
    assert lib.mx_audio_wrap_device(gpu_ctx.handle, C.c_void_p(far.buf.ptr), N_MAX + 1, C.byref(h)) == _capi.MX_ERR_INVALID
    assert h.value == 0x5A5A and b"longer than the reference's int sample indices allow" in lib.mx_last_error()
    assert lib.mx_audio_wrap_device(gpu_ctx.handle, C.c_void_p(far.buf.ptr), 2 ** 40, C.byref(h)) == _capi.MX_ERR_INVALID
    assert h.value == 0x5A5A
    host = np.zeros(1, np.float32)  # (the bound is checked before a sample is read)
    assert lib.mx_audio_upload(gpu_ctx.handle, C.c_void_p(host.ctypes.data), N_MAX + 1, C.byref(h)) == _capi.MX_ERR_INVALID
    assert h.value == 0x5A5A and b"longer than the reference's int sample indices allow" in lib.mx_last_error()
    assert lib.mx_audio_wrap_device(gpu_ctx.handle, C.c_void_p(far.buf.ptr), N_MAX, C.byref(h)) == 0  # at the bound
    assert h.value != 0x5A5A and lib.mx_audio_length(h) == N_MAX
    assert lib.mx_audio_free(gpu_ctx.handle, h) == 0


def test_audio_resample_refuses_a_take_no_kernel_could_walk(gpu_ctx, mxlib, far):
    """mx_audio_resample 44 100 -> 48 000 of the far take would make 2 337 325 836 samples: MX_ERR_INVALID before anything is
    allocated, *out untouched; the longest take whose result is at the bound is not refused for its length; the range forms keep
    serving outputs above 2^31 (test_resample_outputs_past_2_31, and the host form here)."""
    from melonix_amd import _capi
    lib = _capi.lib()
    free0 = FT.mem_info()[0]
    h = C.c_void_p(0x5A5A)
    assert lib.mx_audio_resample(gpu_ctx.handle, far.audio.handle, 44100, 48000, C.byref(h)) == _capi.MX_ERR_INVALID
    assert h.value == 0x5A5A and b"longer than the reference's int sample indices allow" in lib.mx_last_error()
    assert FT.mem_info()[0] >= free0 - (64 << 20)  # nothing of 8.7 GiB was allocated
    # one above the bound and at it: n_ok is the longest take whose result, ceil(n * 160 / 147) samples, is N_MAX itself
    p = R.plan(44100, 48000)
    n_ok = N_MAX * 147 // 160
    assert R.length(n_ok, p) == N_MAX and R.length(n_ok + 1, p) == N_MAX + 1
    over = gpu_ctx.wrap_device(far.buf.ptr, n_ok + 1)
    try:
        assert lib.mx_audio_resample(gpu_ctx.handle, over.handle, 44100, 48000, C.byref(h)) == _capi.MX_ERR_INVALID
        assert h.value == 0x5A5A
    finally:
        over.free()
    far.need(FT.IMAGE * 4, "the converted take at the bound")
    at, out = gpu_ctx.wrap_device(far.buf.ptr, n_ok), None
    try:
        out = gpu_ctx.resample(at, 44100, 48000)
        gpu_ctx.synchronize()
        assert out.n == N_MAX == lib.mx_audio_length(out.handle)
        last = gpu_ctx.audio_download(out, N_MAX - 4096, 4096 + 64)  # its last outputs (they read J31) and the pad behind them
        assert last[:4096].tobytes() == gpu_ctx.resample_range(at, 44100, 48000, N_MAX - 4096, 4096).tobytes()
        assert (last[:4096] != 0).sum() > 2048 and not last[4096:].view(np.uint32).any()
    finally:
        if out is not None:
            out.free()
        at.free()
        far.release(FT.IMAGE * 4)
    m = mxlib.resample_length(N_MAX, 44100, 48000)
    tail = gpu_ctx.resample_range(far.audio, 44100, 48000, m - 64, 64)  # the host range form above 2^31
    assert len(tail) == 64 and np.isfinite(tail).all() and tail.any()
