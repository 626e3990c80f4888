"""Pitch drift and vibrato corrected end to end (include/melonix_amd.h "Pitch drift and vibrato inside notes", "PSOLA follows a
bend curve") on a 2 s synthetic vowel: 150 Hz with harmonics under a fixed envelope, a 6 Hz +-40 cent vibrato and a 30-cent
upward drift.  Chain: mx_f0_track_decoded -> mx_detect_notes -> mx_pitch_contour -> mx_contour_bend -> mx_psola_render_bend.

The reference chain is the same in binary64 / numpy: yin_ref's track, the library's host note detection, contour_ref's cents,
split, bend and plan, psola_ref's render, yin_ref again.  Its figures (longest note, the defaults):
  input                   extent 34.08 cents, drift 24.44 cents (the tracker's 49 ms window passes 0.86 of the 40)
  drift 1, vibrato 0      extent  5.93 cents, drift  1.38 cents
  drift 0, vibrato 2      extent 62.52 cents
The GPU chain gives the same figures to these digits; its PCM is within 9.1e-8 of the reference render (tolerance 9.9e-6).
test_reference_chain_meets_the_conditions checks the conditions on it without a GPU."""
import ctypes as C

import numpy as np
import pytest

import contour_ref as R
import psola_ref
import yin_ref
from conftest import SR, DevBuf, mag_tol

HOP = 256
F0 = 150.0
# What parity (a) and the trackers' own agreement leave of a figure.  The GPU tracker's period is within 1 cent of yin_ref's per
# frame (the tolerance of tests/test_gpu_f0_decode.py and of test_gpu_psola.py's pitch test), on the input and again on the
# re-tracked output; the bend inherits the input's cent; a render within 2e-5 of full scale moves no period by a further cent.
# So a frame's output cents differ by at most 2 between the chains, a smoothed value by as much, drift (max - min) by 4, a vib
# value by 4 and extent (sqrt 2 x the rms of vib) by 4 sqrt 2 < 6.
DRIFT_TOL, EXTENT_TOL = 4.0, 6.0
# the widened take swings +-80 cents around a 30-cent drift: further from a note's median than mx_detect_notes' default 0.75
NOTE_MAX_DEV = 1.5
# ... and moves 3000 cents per second at its steepest, 150 cents inside one analysis window of the tracker: d' there rises to
# 0.33 on the reference render.  The re-tracked renders are read with this voicing threshold (the input with the default)
RETRACK_THRESHOLD = 0.4


def vowel(seconds=2.0, sr=SR):
    """Harmonics of a 150 Hz voice that drifts 30 cents up over the take under a 6 Hz vibrato of +-40 cents; the envelope
    (resonances at 700 and 1200 Hz) is a function of frequency, so it stays where it is while the harmonics move."""
    n = int(seconds * sr)
    t = np.arange(n) / sr
    cents = 30.0 * t / seconds + 40.0 * np.sin(2 * np.pi * 6.0 * t)
    f0 = F0 * 2.0 ** (cents / 1200.0)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    w = np.zeros(n)
    for k in range(1, int(0.4 * sr / (F0 * 1.05))):
        f = k * f0
        amp = 0.05 / k + 0.6 / (1 + ((f - 700.0) / 90.0) ** 2) + 1.0 / (1 + ((f - 1200.0) / 90.0) ** 2)
        w += amp * np.sin(k * phase + 0.7 * k * k)
    return (0.5 * w / np.abs(w).max()).astype(np.float32)


def ref_track(w):
    recs, _ = yin_ref.track(np.asarray(w, dtype=np.float64), SR, HOP)
    t = np.zeros(len(recs), dtype=R.F0_DTYPE)
    for i, (tau, per, ap, rms) in enumerate(recs):
        t[i] = (tau, per, ap, rms)
    return t


def figures(mxlib, track, split, threshold=0.15):
    """-> (notes, spans, rec, the vibrato figures of the longest note).  split(track, notes, spans, threshold) -> (rec, stat)."""
    notes = mxlib.detect_notes(track, SR, HOP, max_dev=NOTE_MAX_DEV, threshold=threshold)
    assert len(notes) >= 1
    spans = R.spans_of(notes)
    rec, stat = split(track, notes, spans, threshold)
    i = int(np.argmax(notes["frames"]))
    assert notes["frames"][i] >= 200  # (more than half of the 375 frames: the widened take loses a frame here and there)
    return notes, spans, rec, R.vibrato(stat[i], int(notes["frames"][i]), SR, HOP)


def ref_split(track, notes, spans, threshold):
    return R.split(R.cents(track, SR, threshold), [tuple(s) for s in spans.tolist()], **R.params_default(SR, HOP))


def reference_chain(mxlib, w, **bend_params):
    """-> (the input's figures, the corrected render's figures), everything in binary64 / numpy."""
    track = ref_track(w)
    notes, spans, rec, fin = figures(mxlib, track, ref_split)
    curve = R.bend(rec, notes, [tuple(s) for s in spans.tolist()], None, **dict(R.BEND_DEFAULTS, **bend_params))
    g, L = R.plan_bend(len(w), SR, HOP, track, [], curve)
    y = psola_ref.render(w, g, L)
    return fin, figures(mxlib, ref_track(y), ref_split, RETRACK_THRESHOLD)[3]


def gpu_chain(mxlib, ctx, a, w, **bend_params):
    """-> (the input's figures, the render's figures, track, curve, f32, int16) through the library alone."""
    def split(track, notes, spans, threshold):
        return ctx.pitch_contour(track, SR, HOP, notes, threshold=threshold)

    track = ctx.f0_track_decoded(a, SR, HOP)
    notes, spans, rec, fin = figures(mxlib, track, split)
    curve = mxlib.contour_bend(rec, notes, mxlib.contour_spans(notes), None, **bend_params)
    f32, i16 = ctx.psola_render_bend(a, SR, HOP, track, [], curve)
    b = ctx.upload(f32)
    try:
        fout = figures(mxlib, ctx.f0_track(b, SR, HOP), split, RETRACK_THRESHOLD)[3]
    finally:
        b.free()
    return fin, fout, track, curve, f32, i16


@pytest.fixture(scope="module")
def take():
    return vowel()


@pytest.fixture(scope="module")
def ref_flat(mxlib, take):
    return reference_chain(mxlib, take, drift_amount=1.0, vibrato_scale=0.0)


@pytest.fixture(scope="module")
def ref_wide(mxlib, take):
    return reference_chain(mxlib, take, drift_amount=0.0, vibrato_scale=2.0)


def test_reference_chain_meets_the_conditions(ref_flat, ref_wide):
    fin, fout = ref_flat
    print(f"reference chain: input extent {fin['extent_cents']:.2f} drift {fin['drift_cents']:.2f}; "
          f"flattened extent {fout['extent_cents']:.2f} drift {fout['drift_cents']:.2f}; widened extent {ref_wide[1]['extent_cents']:.2f}")
    # the tracker's window (2048 + tau samples, 49 ms) passes sinc(6 Hz x 49 ms) = 0.86 of the 40 cents, the triangle 0.95 of that
    assert 30.0 < fin["extent_cents"] < 40.0 and abs(fin["rate_hz"] - 6.0) < 0.15
    assert fout["extent_cents"] < 0.5 * fin["extent_cents"] and fout["drift_cents"] < 0.5 * fin["drift_cents"]
    assert ref_wide[1]["extent_cents"] > 1.5 * fin["extent_cents"]


@pytest.fixture(scope="module")
def audio(gpu_ctx, take):
    a = gpu_ctx.upload(take)
    yield a
    a.free()


@pytest.mark.gpu
def test_flattened_render(mxlib, gpu_ctx, take, audio, ref_flat):
    fin, fout, track, curve, f32, i16 = gpu_chain(mxlib, gpu_ctx, audio, take, drift_amount=1.0, vibrato_scale=0.0)
    # (a) the PCM against the reference's render of the plan the library made, by the PSOLA suite's yardstick:
    # max |g - r| <= 2e-5 max |r| + 1e-9, int16 within 1 LSB
    g, L = mxlib.psola_plan_bend(len(take), SR, HOP, track, [], curve)
    want_g, want_L = R.plan_bend(len(take), SR, HOP, track, [], curve)
    assert L == want_L == len(f32) and g.tobytes() == want_g.tobytes()
    ref = psola_ref.render(take, g, L)
    err, tol = float(np.abs(f32.astype(np.float64) - ref).max()), float(mag_tol(np.abs(ref)[None, :])[0, 0])
    lsb = int(np.abs(i16.astype(np.int32) - psola_ref.pcm16(ref).astype(np.int32)).max())
    print(f"render with the bend curve: {L} samples, {len(g)} grains, max err {err:.3g} (tolerance {tol:.3g}), int16 off by at most {lsb}")
    assert err <= tol and lsb <= 1
    # (b) the feature does something, and what it does is the reference chain's
    print(f"GPU chain: input extent {fin['extent_cents']:.2f} drift {fin['drift_cents']:.2f}; "
          f"flattened extent {fout['extent_cents']:.2f} drift {fout['drift_cents']:.2f}")
    assert fout["extent_cents"] < 0.5 * fin["extent_cents"] and fout["drift_cents"] < 0.5 * fin["drift_cents"]
    for got, want in ((fin, ref_flat[0]), (fout, ref_flat[1])):
        assert abs(got["extent_cents"] - want["extent_cents"]) <= EXTENT_TOL
        assert abs(got["drift_cents"] - want["drift_cents"]) <= DRIFT_TOL


@pytest.mark.gpu
def test_widened_vibrato(mxlib, gpu_ctx, take, audio, ref_wide):
    fin, fout, *_ = gpu_chain(mxlib, gpu_ctx, audio, take, drift_amount=0.0, vibrato_scale=2.0)
    print(f"GPU chain: input extent {fin['extent_cents']:.2f}; widened extent {fout['extent_cents']:.2f}")
    assert fout["extent_cents"] > 1.5 * fin["extent_cents"]
    assert abs(fout["extent_cents"] - ref_wide[1]["extent_cents"]) <= EXTENT_TOL


@pytest.mark.gpu
def test_a_zero_curve_is_the_plain_render(mxlib, gpu_ctx, take, audio):
    L = mxlib._capi.lib()
    track = gpu_ctx.f0_track_decoded(audio, SR, HOP)
    markers = [(30000, 45.0, 0.05, 2.0), (70000, 45.0, 0.0, -1.0)]
    m = mxlib._capi.markers_array(markers)
    n_out = psola_ref.render_length(len(take), SR, markers)
    zeros = np.zeros(len(track), dtype=np.float32)
    bufs = [DevBuf(4 * n_out + 128, fill=0xA5) for _ in range(4)]
    d16 = [DevBuf(2 * n_out + 128, fill=0xA5) for _ in range(2)]
    try:
        assert L.mx_psola_render_dev(gpu_ctx.handle, audio.handle, SR, HOP, track.ctypes.data, len(track), None, m, len(markers),
                                     C.c_void_p(bufs[0].ptr + 64), C.c_void_p(d16[0].ptr + 64)) == 0
        gpu_ctx.psola_render_bend_dev(audio, SR, HOP, track, markers, zeros, (), bufs[1].ptr + 64, d16[1].ptr + 64)
        gpu_ctx.psola_render_bend_dev(audio, SR, HOP, track, markers, None, (), bufs[2].ptr + 64, None)
        gpu_ctx.synchronize()
        plain = bufs[0].read(np.uint8)
        assert plain[:64].tobytes() == b"\xa5" * 64 and plain[64 + 4 * n_out:].tobytes() == b"\xa5" * 64
        assert bufs[1].read(np.uint8).tobytes() == plain.tobytes() == bufs[2].read(np.uint8).tobytes()
        assert d16[1].read(np.uint8).tobytes() == d16[0].read(np.uint8).tobytes()
        assert np.abs(bufs[0].read(np.float32, offset=64, count=n_out)).max() > 0.1
        # ... and with formant points it is the formant render
        points = [(0, 1.5), (60000, -2.0)]
        pts = np.array(points, dtype=mxlib.FORMANT_POINT_DTYPE)
        assert L.mx_psola_render_formant_dev(gpu_ctx.handle, audio.handle, SR, HOP, track.ctypes.data, len(track), None, m, len(markers),
                                             pts.ctypes.data, len(pts), C.c_void_p(bufs[0].ptr + 64), None) == 0
        gpu_ctx.psola_render_bend_dev(audio, SR, HOP, track, markers, zeros, points, bufs[3].ptr + 64, None)
        gpu_ctx.synchronize()
        assert bufs[3].read(np.uint8).tobytes() == bufs[0].read(np.uint8).tobytes() != plain.tobytes()
        # the host form, and a curve that is not finite
        f32, i16 = gpu_ctx.psola_render_bend(audio, SR, HOP, track, markers, zeros)
        assert f32.tobytes() == plain[64:64 + 4 * n_out].tobytes()
        zeros[100] = np.nan
        with pytest.raises(mxlib.MxError) as e:
            gpu_ctx.psola_render_bend_dev(audio, SR, HOP, track, markers, zeros, (), bufs[1].ptr + 64, None)
        assert e.value.code == -1
        assert bufs[1].read(np.uint8).tobytes() == plain.tobytes()  # refused before any launch
    finally:
        for b in bufs + d16:
            b.free()
