"""The YIN f0 tracker on the MI355X against its f64 restatement (tests/yin_ref.py), its launch-split and device forms, its
guard bands, the hour, and the end-to-end retune: f0_track -> detect_notes -> correction_markers -> export_wav / pv_render."""
import ctypes as C
import numpy as np
import pytest

import yin_ref as Y
from conftest import SR, DevBuf, accum_sweep, loaded_hip, noisy
from hip_timing import EventTimer

pytestmark = pytest.mark.gpu

HOP = 256


def _tones(sr, freqs, secs=0.4, partials=(1.0,)):
    i = np.arange(int(secs * sr), dtype=np.float64)
    out = []
    for f in freqs:
        w = sum(a * np.sin(2 * np.pi * (k + 1) * f * i / sr) for k, a in enumerate(partials) if a)
        out.append(0.5 * w / max(1.0, sum(abs(a) for a in partials)))
    return np.concatenate(out).astype(np.float32)


def _signals(sr):
    fr = np.geomspace(55.0, 1760.0, 24)
    i = np.arange(sr, dtype=np.float64)
    return {
        "tones": _tones(sr, fr),
        "harmonic": _tones(sr, [73.4, 146.8, 261.6, 440.0], partials=(1, 0.5, 0.33, 0.25, 0.2)),
        "missing_fundamental": _tones(sr, [110.0, 196.0], partials=(0, 0.5, 0.33, 0.25, 0.2)),
        "noisy": noisy((0.5 * np.sin(2 * np.pi * 220.0 * i / sr)).astype(np.float32)),
        "silence": np.zeros(sr // 2, np.float32),
        "sweep": accum_sweep(10 * sr, sr=sr),
    }



@pytest.mark.parametrize("sr", [48000, 44100])
def test_parity_with_the_reference(gpu_ctx, sr):
    tmin, tmax = Y.tau_range(sr)
    frames = ties_total = 0
    for name, w in _signals(sr).items():
        a = gpu_ctx.upload(w)
        got = gpu_ctx.f0_track(a, sr, HOP)
        a.free()
        recs, dp = Y.track(w, sr, HOP)
        # near-ties: d' within 1e-4 of theta at some tau <= tau*, or within 1e-4 of d'(tau*) at a competing candidate
        n, excused = Y.check_parity(got, recs, dp, tmin, tmax, 0.15, f"sr={sr} {name}", eps=1e-4, cents=1.0, ap_abs=1e-4,
                                    ap_rel=1e-3, rms_rel=1e-5)
        frames += n
        ties_total += excused
    # (at low f0 the curvature of d' at its minimum, ~2 (2 pi / T)^2 per lag^2, puts tau*'s neighbours within 1e-4 of it on
    # most frames: near-ties by the definition, though the kernel's d' is ~1e-6 from the reference's and agrees on them.
    # What may not exceed 0.5 % is the frames the rule actually excuses: near-ties whose tau differs.)
    print(f"f0 parity sr={sr}: tau excused as a near-tie on {ties_total} of {frames} frames ({100.0 * ties_total / frames:.3f} %)")
    assert ties_total < 0.005 * frames


def test_sub_launches_and_device_form(gpu_ctx):
    w = noisy(accum_sweep(6 * SR))
    a = gpu_ctx.upload(w)
    whole = gpu_ctx.f0_track(a, SR, HOP)
    F = len(whole)
    rng = np.random.default_rng(11)
    cuts = np.unique(np.concatenate([[0, F], rng.integers(1, F, 12)]))
    parts = np.concatenate([gpu_ctx.f0_track(a, SR, HOP, int(lo), int(hi - lo)) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert parts.tobytes() == whole.tobytes()
    d = DevBuf(F * 16, fill=0x5A)
    gpu_ctx.f0_track_dev(a, SR, HOP, 0, F, d.ptr)
    gpu_ctx.synchronize()
    assert d.read(np.uint8).tobytes() == whole.tobytes()
    d.free()
    a.free()


@pytest.mark.parametrize("first,count,hop", [(0, 1, 256), (3, 17, 256), (0, 100, 255), (50, 33, 1000)])
def test_guard_bands(gpu_ctx, first, count, hop):
    G, SENT = 64 * 1024, 0xA5
    w = noisy(accum_sweep(3 * SR))
    a = gpu_ctx.upload(w)
    ref = gpu_ctx.f0_track(a, SR, hop, first, count)
    for shift in (0, 4):
        buf = DevBuf(G + shift + count * 16 + G, fill=SENT)
        gpu_ctx.f0_track_dev(a, SR, hop, first, count, buf.ptr + G + shift)
        gpu_ctx.synchronize()
        host = buf.read(np.uint8)
        buf.free()
        lo, hi = G + shift, G + shift + count * 16
        assert (host[:lo] == SENT).all() and (host[hi:] == SENT).all()
        assert host[lo:hi].tobytes() == ref.tobytes()
    a.free()


def test_argument_errors(gpu_ctx, mxlib):
    """Every f0 entry point turns every bad argument down with MX_ERR_INVALID and writes no output: the tracker-side five
    share one parse, the decode forms one check.  Launches of at most four frames, or none."""
    from melonix_amd import _capi
    lib, ctx = _capi.lib(), gpu_ctx.handle
    a = gpu_ctx.upload(np.zeros(10000, np.float32))
    F = mxlib.frame_count(10000, HOP)
    # outputs, filled: host (track, cands, state) and device; sized for the four frames no case exceeds
    host = [np.full(n, 0x5A, np.uint8) for n in (4 * 16, 4 * 64, 4)]
    dev = [DevBuf(n, 0x5A) for n in (4 * 16, 4 * 64, 4)]
    (h_track, h_cands, h_state), (d_track, d_cands, d_state) = [[b.ctypes.data for b in host], [b.ptr for b in dev]]

    def untouched():
        return all((b == 0x5A).all() for b in host) and all((b.read() == 0x5A).all() for b in dev)

    for kw in (dict(sr=0), dict(hop=0), dict(hop=20000), dict(first=F - 1, count=2), dict(fmin=0.0), dict(fmin=-5.0),
               dict(fmin=1000.0, fmax=900.0), dict(fmin=10.0, fmax=20.0), dict(threshold=float("nan"))):
        args = dict(sr=SR, hop=HOP, first=0, count=4)
        args.update(kw)
        common = (ctx, a.handle, args["sr"], args["hop"], args["first"], args["count"], args.get("fmin", 55.0),
                  args.get("fmax", 1760.0), args.get("threshold", 0.15))
        for name, rc in (("mx_f0_track", lib.mx_f0_track(*common, h_track)),
                         ("mx_f0_track_dev", lib.mx_f0_track_dev(*common, d_track)),
                         ("mx_f0_candidates", lib.mx_f0_candidates(*common, h_track, h_cands)),
                         ("mx_f0_candidates_dev", lib.mx_f0_candidates_dev(*common, d_track, d_cands)),
                         ("mx_f0_track_decoded", lib.mx_f0_track_decoded(*common, None, h_track))):
            assert rc == _capi.MX_ERR_INVALID, (name, kw)
        assert untouched(), kw

    # the decode forms' own: a valid table of four frames, one bad argument at a time
    track = np.zeros(4, mxlib.F0_DTYPE)
    cands = np.zeros((4, 4), mxlib.F0_CAND_DTYPE)
    d_tin, d_cin = DevBuf(track.nbytes), DevBuf(cands.nbytes)
    good = (0.3, 0.1, 0.5, 1200)
    bad_params = [good[:k] + (v,) + good[k + 1:] for k in range(3) for v in (float("nan"), -1.0, 17.0)]
    bad_params += [good[:3] + (v,) for v in (-1, 12001)]
    for vals in bad_params:
        p = C.byref(_capi.F0DecodeParams(*vals))
        rcs = (lib.mx_f0_decode(ctx, track.ctypes.data, cands.ctypes.data, 4, p, h_track, h_state),
               lib.mx_f0_decode_dev(ctx, d_tin.ptr, d_cin.ptr, 4, p, d_track, d_state),
               lib.mx_f0_track_decoded(ctx, a.handle, SR, HOP, 0, 4, 55.0, 1760.0, 0.15, p, h_track))
        assert rcs == (_capi.MX_ERR_INVALID,) * 3, vals
        assert untouched(), vals
    for fn, t, c, o, st in ((lib.mx_f0_decode, track.ctypes.data, cands.ctypes.data, h_track, h_state),
                            (lib.mx_f0_decode_dev, d_tin.ptr, d_cin.ptr, d_track, d_state)):
        for call in ((t, c, -1, None, o, st), (None, c, 4, None, o, st), (t, None, 4, None, o, st), (t, c, 4, None, None, st)):
            assert fn(ctx, *call) == _capi.MX_ERR_INVALID, (fn.__name__, call)
            assert untouched(), (fn.__name__, call)
    for b in dev + [d_tin, d_cin]:
        b.free()
    a.free()


def test_the_hour(gpu_ctx, mxlib):
    n = 60 * 60 * SR
    w = accum_sweep(n)
    a = gpu_ctx.upload(w)
    F = mxlib.frame_count(n, HOP)
    assert F == 675000
    d = DevBuf(F * 16)
    gpu_ctx.set_stream(None)  # the null stream: the timer's events bracket exactly the launch
    try:
        t = EventTimer(loaded_hip()).timed({"f0": lambda: gpu_ctx.f0_track_dev(a, SR, HOP, 0, F, d.ptr)}, warm=2, runs=5)["f0"]
    finally:
        gpu_ctx.use_own_stream()
    med = t["median"]
    tr = d.read(np.uint8).view(mxlib.F0_DTYPE)
    d.free()
    a.free()
    h = np.arange(F)
    inner = (h * HOP >= 4096) & (h * HOP <= n - 4096)
    f_inst = 110.0 + (1760.0 - 110.0) * (h * HOP) / n
    cents = 1200 * np.log2(SR / tr["period"][inner] / f_inst[inner])
    print(f"f0 hour: {F} frames, median of 5 timed calls {med:.3f} ms ({t['min']:.3f} to {t['max']:.3f}); "
          f"analytic f0 within {np.abs(cents).max():.3f} cents (mean {cents.mean():+.4f})")
    assert np.abs(cents).max() <= 2.0
    assert med < 20.0


# ---- end to end: a detuned melody, retuned through the markers ----
MEL_NOTES = [45, 48, 50, 52, 55, 57]
MEL_CENTS = [+20, -30, +45, -45, +35, -20]


def melody(sr=SR):
    i = np.arange(int(0.4 * sr), dtype=np.float64)
    parts, starts, pos = [], [], 0
    for note, c in zip(MEL_NOTES, MEL_CENTS):
        f = 55.0 * 2 ** ((note + c / 100.0 - 24) / 12)
        tone = sum(a * np.sin(2 * np.pi * (k + 1) * f * i / sr) for k, a in enumerate((1, 0.5, 0.33, 0.25, 0.2)))
        env = np.minimum(1.0, np.minimum(i, i[::-1]) / (0.01 * sr))
        parts += [0.25 * tone * env, np.zeros(int(0.1 * sr))]
        starts.append(pos)
        pos += len(i) + int(0.1 * sr)
    return np.concatenate(parts).astype(np.float32), starts


def _retrack(ctx, mxlib, w):
    a = ctx.upload(w)
    tr = ctx.f0_track(a, SR, HOP)
    a.free()
    return mxlib.detect_notes(tr, SR, HOP)


def _check(notes, starts, targets):
    assert len(notes) == len(targets), f"{len(notes)} notes"
    for nt, s, t in zip(notes, starts, targets):
        assert abs(float(nt["note"]) - t) * 100 <= 10.0, (float(nt["note"]), t)
        assert abs(int(nt["start_sample"]) - s) <= HOP + 2048


def _wav_pcm(path):
    import wave
    with wave.open(str(path), "rb") as f:
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float32) / 32768.0


def test_end_to_end_retune(gpu_ctx, mxlib, tmp_path):
    w, starts = melody()
    notes = _retrack(gpu_ctx, mxlib, w)
    with pytest.raises(AssertionError):
        _check(notes, starts, MEL_NOTES)  # the input itself is detuned
    assert len(notes) == 6
    mk = mxlib.correction_markers(notes, 1.0, 0)
    targets = [float(m["note"] + m["pitchBend"]) for m in mk[::2]]
    assert targets == [float(x) for x in MEL_NOTES]
    spreads = {}
    # (a) the granular export
    path = tmp_path / "retuned.wav"
    gpu_ctx.export_wav(w, SR, list(mk), str(path), strict=False)
    g = _retrack(gpu_ctx, mxlib, _wav_pcm(path))
    spreads["granular"] = [round(100 * (float(nt["note"]) - t), 2) for nt, t in zip(g, MEL_NOTES)] if len(g) == 6 else len(g)
    # (b) the marker-driven phase vocoder
    a = gpu_ctx.upload(w)
    y, _ = gpu_ctx.pv_render(a, SR, list(mk), want_i16=False)
    a.free()
    p = _retrack(gpu_ctx, mxlib, y)
    spreads["pv"] = [round(100 * (float(nt["note"]) - t), 2) for nt, t in zip(p, MEL_NOTES)] if len(p) == 6 else len(p)
    print(f"f0 e2e: input notes {[round(float(x), 3) for x in notes['note']]}; retuned (cents off target) {spreads}")
    _check(p, starts, MEL_NOTES)
    _check(g, starts, MEL_NOTES)


def test_scale_mask_moves_a_note_to_the_nearest_allowed_class(gpu_ctx, mxlib):
    w, starts = melody()
    notes = _retrack(gpu_ctx, mxlib, w)
    mask = 0xFFF & ~(1 << (50 % 12))  # class of note 50 excluded: 50.45 goes to 51
    mk = mxlib.correction_markers(notes, 1.0, mask)
    targets = [float(m["note"] + m["pitchBend"]) for m in mk[::2]]
    assert targets == [45.0, 48.0, 51.0, 52.0, 55.0, 57.0]
    a = gpu_ctx.upload(w)
    y, _ = gpu_ctx.pv_render(a, SR, list(mk), want_i16=False)
    a.free()
    _check(_retrack(gpu_ctx, mxlib, y), starts, targets)
