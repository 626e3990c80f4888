"""True-peak records and the look-ahead limiter on the GPU (include/melonix_amd.h "True peak, limiter and loudness range"): byte
for byte tests/truepeak_ref.py's at the smallest shapes that can go wrong — lengths around the window and the step, look-aheads
around the powers of two of the sliding minimum, peaks at both ends of the file and astride the limiter's 2048-sample tiles —
whatever the launch split; the five laws of the definition; nothing written outside the outputs; the refusals; and the export
chain end to end."""
import ctypes as C

import numpy as np
import pytest

import bad_samples as BAD
import loudness_ref as L
import pcm_extremes as PCM
import truepeak_ref as T
from conftest import DevBuf
from guarded import Guarded

pytestmark = pytest.mark.gpu

RATES = (48000, 44100, 8000, 96000, 192000)
LENGTHS = (1, 5, 6, 7, 479, 480, 481, 4801, 10007)
LOOKAHEADS = (1, 2, 63, 64, 65, 240, 1024)
LIMIT_LENGTHS = (1, 7, 2047, 2048, 2049, 4097, 10007)
C1 = T.MINUS_1_DBTP


@pytest.fixture(scope="module")
def taps(mxlib):
    t = mxlib.true_peak_taps()
    t.setflags(write=False)
    return t


def dev_records(ctx, audio, sr, first_step, nsteps, shift=0):
    """The device form into a guarded buffer -> the records; the guards must stand."""
    g = Guarded(nsteps * 8, shift)
    try:
        ctx.true_peak_steps_dev(audio, sr, first_step, nsteps, g.ptr)
        ctx.synchronize()
        return g.take(T.STEP_DTYPE)
    finally:
        g.free()


def dev_limit(ctx, audio, sr, c, A, pcm_shift=0):
    """The device form with the int16 in a guarded buffer -> (samples, int16, the new image's two pads)."""
    g = Guarded(audio.n * 2, pcm_shift)
    b = None
    try:
        b = ctx.limit_dev(audio, sr, lookahead=A, d_pcm16=g.ptr, ceiling_amp=c)
        ctx.synchronize()
        pcm = g.take(np.int16)
        pad = 4096
        return (ctx.audio_download(b), pcm, ctx.audio_download(b, -pad, pad), ctx.audio_download(b, audio.n, pad))
    finally:
        if b is not None:
            b.free()
        g.free()


@pytest.mark.parametrize("sr", RATES)
def test_records_are_the_references_bytes(mxlib, gpu_ctx, taps, sr):
    """Noise with sparse clicks at every length around the 12-sample window and the step: the device and the host form."""
    for n in LENGTHS:
        w = T.sparse_clicks(n, seed=sr + n)
        ref = T.records(w, sr, taps)
        assert len(ref) == mxlib.loudness_step_count(n, sr)
        a = gpu_ctx.upload(w)
        try:
            dev = dev_records(gpu_ctx, a, sr, 0, len(ref))
            host = gpu_ctx.true_peak_steps(a, sr)
            tp, sp = gpu_ctx.true_peak(a, sr)
        finally:
            a.free()
        assert dev.tobytes() == ref.tobytes(), (sr, n)
        assert host.tobytes() == dev.tobytes() and host.dtype == mxlib.TP_STEP_DTYPE
        assert (tp, sp) == T.measure(ref) and np.all(ref["true_peak"] >= ref["sample_peak"])


@pytest.mark.parametrize("sr", (44100, 8000, 192000))
def test_same_records_whatever_the_split(gpu_ctx, taps, sr):
    """Single steps, uneven thirds (S = 441: steps that start at no multiple of 4 samples; 8 kHz: 51 steps to a workgroup, the
    splits cut its runs anywhere; 192 kHz: one step to a workgroup), the host form of a range, empty ranges."""
    S = T.step_samples(sr)
    n = 118 * S + S // 3
    w = T.sparse_clicks(n, seed=sr)
    ref = T.records(w, sr, taps)
    steps = len(ref)
    assert steps == 119
    a = gpu_ctx.upload(w)
    try:
        cuts = (0, 17, 17 + 61, steps)
        parts = [dev_records(gpu_ctx, a, sr, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        assert b"".join(p.tobytes() for p in parts) == ref.tobytes()
        for b in (0, 1, 50, 51, 52, steps - 2, steps - 1):
            assert dev_records(gpu_ctx, a, sr, b, 1).tobytes() == ref[b:b + 1].tobytes(), b
        assert dev_records(gpu_ctx, a, sr, 3, 7, shift=8).tobytes() == ref[3:10].tobytes()  # (8-byte aligned, not 16)
        assert gpu_ctx.true_peak_steps(a, sr, 100, 19).tobytes() == ref[100:].tobytes()
        assert len(gpu_ctx.true_peak_steps(a, sr, 5, 0)) == 0 and len(gpu_ctx.true_peak_steps(a, sr, steps, 0)) == 0
    finally:
        a.free()


@pytest.mark.parametrize("name", sorted(T.SIGNALS))
def test_limiter_is_the_references_bytes(gpu_ctx, taps, name):
    """f32 and int16 at every look-ahead around the powers of two and every length around the 2048-sample tile: peaks within A of
    both ends and astride the tile edges (the clicks sit at 0, 3, 2047, 2048, 2049, 4096, 9999 and n - 1)."""
    sr = 48000
    for n in LIMIT_LENGTHS:
        w = T.SIGNALS[name](n)
        a = gpu_ctx.upload(w)
        try:
            for A in LOOKAHEADS:
                want, want16 = T.limit(w, sr, taps, C1, A)
                b, got16 = gpu_ctx.limit(a, sr, lookahead=A, pcm16=True)
                try:
                    got = gpu_ctx.audio_download(b)
                finally:
                    b.free()
                assert got.tobytes() == want.tobytes(), (name, n, A, np.flatnonzero(got != want)[:8])
                assert got16.tobytes() == want16.tobytes(), (name, n, A)
        finally:
            a.free()


@pytest.mark.parametrize("sr", (44100, 96000, 192000, 8000))
def test_limiter_at_the_other_rates(gpu_ctx, taps, sr):
    """Oversampling 4, 2 and 1, the default look-ahead of each rate, another ceiling."""
    n, c = 6007, np.float32(0.5)
    w = T.clicks(n, seed=sr)
    A = T.default_lookahead(sr)
    want, want16 = T.limit(w, sr, taps, c, A)
    a = gpu_ctx.upload(w)
    try:
        got, got16, left, right = dev_limit(gpu_ctx, a, sr, c, None)
    finally:
        a.free()
    assert got.tobytes() == want.tobytes() and got16.tobytes() == want16.tobytes() and np.abs(got).max() <= c


def test_laws_1_to_4(gpu_ctx, taps):
    """|out| <= c; x's bytes wherever no peak within A is over c; the power-of-two law for k = -7 and -20, records too; silence."""
    sr, n, A = 48000, 10007, 240
    for name in sorted(T.SIGNALS):
        w = T.SIGNALS[name](n)
        a = gpu_ctx.upload(w)
        try:
            b = gpu_ctx.limit(a, sr, lookahead=A)
            out = gpu_ctx.audio_download(b)
            b.free()
            rec = gpu_ctx.true_peak_steps(a, sr)
        finally:
            a.free()
        assert np.abs(out).max() <= C1, name                                                         # 1
        near = np.zeros(n, dtype=bool)
        for j in np.flatnonzero(T.peaks(w, sr, taps) > C1):
            near[max(j - A, 0):j + A + 1] = True
        assert out[~near].tobytes() == w[~near].tobytes() and near.any() and not np.array_equal(out[near], w[near]), name   # 2
        for k in (-7, -20):                                                                          # 3
            f = np.float32(2.0 ** k)
            assert np.array_equal((w * f).astype(np.float64), w.astype(np.float64) * 2.0 ** k)       # exact in binary32
            a = gpu_ctx.upload(w * f)
            try:
                b = gpu_ctx.limit(a, sr, lookahead=A, ceiling_amp=C1 * f)
                scaled = gpu_ctx.audio_download(b)
                b.free()
                rec_scaled = gpu_ctx.true_peak_steps(a, sr)
            finally:
                a.free()
            assert scaled.tobytes() == (out * f).tobytes(), (name, k)
            assert rec_scaled.view(np.float32).tobytes() == (rec.view(np.float32) * f).tobytes(), (name, k)
    for w in (np.zeros(5000, np.float32), np.full(5000, -0.0, np.float32)):                         # 4
        a = gpu_ctx.upload(w)
        try:
            rec = gpu_ctx.true_peak_steps(a, sr)
            b, pcm = gpu_ctx.limit(a, sr, lookahead=A, pcm16=True)
            out = gpu_ctx.audio_download(b)
            b.free()
        finally:
            a.free()
        assert rec.tobytes() == np.zeros(len(rec), dtype=T.STEP_DTYPE).tobytes()
        assert out.tobytes() == w.tobytes() and not pcm.any()


@pytest.mark.parametrize("kind", sorted(BAD.BAD))
def test_law_5_a_bad_sample_stays_local(gpu_ctx, taps, kind):
    """A NaN or +-Inf at s = 0, mid-file and n - 1 changes no record outside the steps that hold samples of [s - 6, s + 5] and no
    output outside [s - A - 6, s + A + 6]; everything is the definition's (NaNs compared as NaN)."""
    sr, n, A, S = 48000, 4801, 65, 480
    w = T.noise(n, 0.5)
    clean_rec = T.records(w, sr, taps)
    clean_out, clean_pcm = T.limit(w, sr, taps, C1, A)
    for s in (0, n // 2, n - 1):
        x = BAD.with_bad(w, s, BAD.BAD[kind])
        a = gpu_ctx.upload(x)
        try:
            rec = gpu_ctx.true_peak_steps(a, sr)
            b, pcm = gpu_ctx.limit(a, sr, lookahead=A, pcm16=True)
            out = gpu_ctx.audio_download(b)
            b.free()
        finally:
            a.free()
        want_rec = T.records(x, sr, taps)
        want_out, want_pcm = T.limit(x, sr, taps, C1, A)
        assert rec.tobytes() == want_rec.tobytes() and not np.isnan(rec.view(np.float32)).any(), (kind, s)
        PCM.same_floats(out, want_out, (kind, s))
        assert pcm.tobytes() == want_pcm.tobytes()
        held = np.zeros(len(rec), dtype=bool)
        held[max(s - 6, 0) // S:min(s + 5, n - 1) // S + 1] = True
        assert rec[~held].tobytes() == clean_rec[~held].tobytes(), (kind, s)
        far = np.ones(n, dtype=bool)
        far[max(s - A - 6, 0):s + A + 7] = False
        assert out[far].tobytes() == clean_out[far].tobytes() and pcm[far].tobytes() == clean_pcm[far].tobytes(), (kind, s)
        if kind != "nan":
            assert rec["true_peak"][s // S] == np.inf and rec["sample_peak"][s // S] == np.inf


def test_guard_bands(gpu_ctx, taps):
    """Nothing is written around the records, the int16 samples or — in the new image — the samples: a launch that ends in a
    partial step, a limiter launch that ends in a partial tile (and a partial quad), outputs at shifted addresses (records at an
    odd multiple of 8 bytes; int16 at an odd element, where the 8-byte stores give way to single ones)."""
    sr, A = 44100, 240
    for n in (2048 + 1021, 4096, 3 * 441 + 2):
        w = T.clicks(n, seed=n)
        ref = T.records(w, sr, taps)
        want, want16 = T.limit(w, sr, taps, C1, A)
        a = gpu_ctx.upload(w)
        try:
            for shift in (0, 8, 24):
                assert dev_records(gpu_ctx, a, sr, 0, len(ref), shift).tobytes() == ref.tobytes(), (n, shift)
            assert dev_records(gpu_ctx, a, sr, len(ref) - 1, 1).tobytes() == ref[-1:].tobytes()
            for shift in (0, 2, 6, 8):
                got, got16, left, right = dev_limit(gpu_ctx, a, sr, C1, A, shift)
                assert got.tobytes() == want.tobytes() and got16.tobytes() == want16.tobytes(), (n, shift)
                assert not left.view(np.uint32).any() and not right.view(np.uint32).any(), (n, shift)  # the pads: +0.0f throughout
        finally:
            a.free()


@pytest.mark.parametrize("n", (1, 3, 2047, 2048, 2049))
def test_every_derived_audio_has_its_length_and_zero_pads(mxlib, gpu_ctx, taps, n):
    """The gain's copy (no points), the gain with points, the limiter without and with the int16: each a new object of n samples
    whose two pads — every one of their MX_AUDIO_PAD samples, read back through audio_download — are +0.0f, at lengths below a
    quad, one short of the limiter's tile, on it and one past it; freeing the object leaves the context and the source usable."""
    sr, A, pad = 48000, 64, mxlib.MX_AUDIO_PAD
    w = T.clicks(n, seed=n)
    limited = T.limit(w, sr, taps, C1, A)[0]
    a = gpu_ctx.upload(w)
    try:
        forms = (("copy", lambda: gpu_ctx.audio_gain(a, []), w),
                 ("gain", lambda: gpu_ctx.audio_gain(a, [(0, 0.5), (n, 2.0)]), None),
                 ("limit", lambda: gpu_ctx.limit(a, sr, lookahead=A), limited),
                 ("limit + int16", lambda: gpu_ctx.limit(a, sr, lookahead=A, pcm16=True)[0], limited))
        for name, make, want in forms:
            b = make()
            try:
                assert b.n == n and mxlib._capi.lib().mx_audio_length(b.handle) == n, name
                left, body, right = gpu_ctx.audio_download(b, -pad, pad), gpu_ctx.audio_download(b), gpu_ctx.audio_download(b, n, pad)
            finally:
                b.free()
            assert len(left) == pad == len(right) and len(body) == n, name
            assert not left.view(np.uint32).any() and not right.view(np.uint32).any(), name  # +0.0f throughout
            assert want is None or body.tobytes() == want.tobytes(), name
            assert gpu_ctx.audio_download(a).tobytes() == w.tobytes(), name
    finally:
        a.free()


def test_bad_arguments_are_refused_before_any_launch(mxlib, gpu_ctx, taps):
    sr, n = 48000, 4801
    w = T.clicks(n)
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    steps = 11
    a = gpu_ctx.upload(w)
    buf = DevBuf((steps + 2) * 8 + 2 * n, fill=0xA5)
    host = np.full((steps + 2) * 8, 0xA5, dtype=np.uint8)
    host16 = np.full(n, 0x5A5A, dtype=np.int16)
    try:
        for rate, first, count in ((7999, 0, 1), (384001, 0, 1), (0, 0, 1), (sr, -1, 1), (sr, 0, -1), (sr, 0, steps + 1), (sr, steps, 1),
                                   (sr, steps + 1, 0), (sr, 2, steps - 1), (sr, 1, 2 ** 62)):
            for name, out in (("mx_true_peak_steps_dev", buf.ptr), ("mx_true_peak_steps", host.ctypes.data)):
                assert getattr(lib, name)(gpu_ctx.handle, a.handle, rate, first, count, C.c_void_p(out)) == INVALID, (name, rate, first, count)
        for name, out in (("mx_true_peak_steps_dev", buf.ptr), ("mx_true_peak_steps", host.ctypes.data)):
            assert getattr(lib, name)(None, a.handle, sr, 0, 1, C.c_void_p(out)) == INVALID
            assert getattr(lib, name)(gpu_ctx.handle, None, sr, 0, 1, C.c_void_p(out)) == INVALID
            assert getattr(lib, name)(gpu_ctx.handle, a.handle, sr, 0, 1, None) == INVALID
        assert lib.mx_true_peak_steps_dev(gpu_ctx.handle, a.handle, sr, 0, 1, C.c_void_p(buf.ptr + 4)) == INVALID  # not 8-byte aligned
        assert b"aligned" in lib.mx_last_error()
        t, s = C.c_float(7.0), C.c_float(7.0)
        assert lib.mx_true_peak_measure(gpu_ctx.handle, a.handle, 7999, C.byref(t), C.byref(s)) == INVALID
        assert lib.mx_true_peak_measure(gpu_ctx.handle, None, sr, C.byref(t), C.byref(s)) == INVALID
        assert lib.mx_true_peak_measure(None, a.handle, sr, C.byref(t), C.byref(s)) == INVALID
        assert lib.mx_true_peak_measure(gpu_ctx.handle, a.handle, sr, None, None) == INVALID and (t.value, s.value) == (7.0, 7.0)
        assert lib.mx_true_peak_measure(gpu_ctx.handle, a.handle, sr, C.byref(t), None) == 0 and t.value == T.measure(T.records(w, sr, taps))[0]
        marker = 0x5A5A5A5A
        P = mxlib._capi.LimitParams
        tiny = float(np.float32(1e-39))  # subnormal
        bad = [(7999, P(0.5, 64)), (384001, P(0.5, 64)), (sr, P(0.0, 64)), (sr, P(-0.5, 64)), (sr, P(1.0000001, 64)), (sr, P(tiny, 64)),
               (sr, P(float("nan"), 64)), (sr, P(float("inf"), 64)), (sr, P(0.5, 0)), (sr, P(0.5, -1)), (sr, P(0.5, 1025))]
        for name, pcm in (("mx_audio_limit_dev", buf.ptr + (steps + 2) * 8), ("mx_audio_limit", host16.ctypes.data)):
            fn = getattr(lib, name)
            out = C.c_void_p(marker)
            for rate, p in bad:
                assert fn(gpu_ctx.handle, a.handle, rate, C.byref(p), C.byref(out), C.c_void_p(pcm)) == INVALID, (name, rate, p.ceiling_amp, p.lookahead)
            assert fn(None, a.handle, sr, None, C.byref(out), C.c_void_p(pcm)) == INVALID
            assert fn(gpu_ctx.handle, None, sr, None, C.byref(out), C.c_void_p(pcm)) == INVALID
            assert fn(gpu_ctx.handle, a.handle, sr, None, None, C.c_void_p(pcm)) == INVALID
            assert out.value == marker, name
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5) and np.all(host == 0xA5) and np.all(host16 == 0x5A5A)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.limit(a, sr, lookahead=1025)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.true_peak_steps(a, sr, 0, steps + 1)
        # the context works on: the defaults (params NULL), a ceiling of exactly 1, no int16, and an empty take
        out = C.c_void_p()
        assert lib.mx_audio_limit(gpu_ctx.handle, a.handle, sr, None, C.byref(out), None) == 0
        b = mxlib.Audio(gpu_ctx, out, n)
        assert gpu_ctx.audio_download(b).tobytes() == T.limit(w, sr, taps, C1, 240)[0].tobytes()
        b.free()
        b = gpu_ctx.limit(a, sr, lookahead=1, ceiling_amp=1.0)
        assert gpu_ctx.audio_download(b).tobytes() == T.limit(w, sr, taps, np.float32(1.0), 1)[0].tobytes()
        b.free()
        e = gpu_ctx.upload(np.zeros(0, np.float32))
        b, pcm = gpu_ctx.limit(e, sr, pcm16=True)
        assert b.n == 0 and len(pcm) == 0 and len(gpu_ctx.true_peak_steps(e, sr)) == 0 and gpu_ctx.true_peak(e, sr) == (0.0, 0.0)
        b.free()
        e.free()
    finally:
        buf.free()
        a.free()


def chain_take():
    """the levelling take of tests/test_gpu_loudness.py scaled to peak at 1.5"""
    w = L.levelling_take()[0]
    return (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)


@pytest.mark.parametrize("target", [-16.0, -12.0])
def test_the_export_chain_end_to_end(mxlib, gpu_ctx, taps, target):
    """measure -> gain to the target loudness (mx_normalize_gain_tp's loudness term: the limiter holds the ceiling) -> limit at
    -1 dBTP with the default look-ahead -> measure again, against tests/truepeak_ref.py export_chain: the gained and the limited
    samples, the int16 and the records by bytes; max |out| <= c; the integrated loudness off the target by no more than in the
    reference chain.  MEASURED, the re-metered true peak: at most c plus twice the reference chain's own overshoot on this take
    (doubled as DESIGN 5m doubles its residue; nothing where the bytes agree).  The reference chain, on the CPU: at -16 LUFS
    the gained take peaks at -1.994 dBTP, the limiter has nothing to do and the overshoot is 0 (the re-metered peak stays
    0.994 dB under c); at -12 LUFS it peaks at +2.006 dBTP, the limited take re-meters 2.0e-5 dB (2.0e-6 in amplitude) over c
    and its loudness comes out at -14.30 LUFS: the limiter took the rest."""
    sr = L.LEVEL_SR
    w = chain_take()
    k = mxlib.loudness_coeffs(sr)
    ref = T.export_chain(w, sr, k, taps, target_lufs=target)
    a = gpu_ctx.upload(w)
    made = []
    try:
        before = gpu_ctx.loudness_measure(a, sr)
        tp_before = gpu_ctx.true_peak(a, sr)
        assert tp_before == ref["tp_before"] and abs(before["integrated"] - ref["before"]["integrated"]) <= 1e-9
        amp = mxlib.normalize_gain_tp(before, tp_before[0], target, 200.0)  # (a ceiling far above: the loudness term alone)
        assert np.float32(amp).tobytes() == ref["amp"].tobytes()
        made.append(gpu_ctx.audio_gain(a, [(0, amp)]))
        assert gpu_ctx.audio_download(made[-1]).tobytes() == ref["gained"].tobytes()
        b, pcm = gpu_ctx.limit(made[-1], sr, ceiling_db=-1.0, pcm16=True)
        made.append(b)
        out = gpu_ctx.audio_download(b)
        after = gpu_ctx.loudness_measure(b, sr)
        tp_after = gpu_ctx.true_peak(b, sr)
        rec_after = gpu_ctx.true_peak_steps(b, sr)
    finally:
        for b in made:
            b.free()
        a.free()
    assert out.tobytes() == ref["out"].tobytes() and pcm.tobytes() == ref["pcm"].tobytes()
    assert rec_after.tobytes() == T.records(ref["out"], sr, taps).tobytes()
    assert np.abs(out).max() <= C1
    moved, ref_moved = abs(after["integrated"] - target), abs(ref["after"]["integrated"] - target)
    overshoot = max(float(ref["tp_after"][0]) - float(C1), 0.0)
    print(f"target {target}: loudness after {after['integrated']:.6f} LUFS (the reference chain {ref['after']['integrated']:.6f}); true peak after "
          f"{T.dbtp(tp_after[0]):+.4f} dBTP, the reference chain's {T.dbtp(ref['tp_after'][0]):+.4f} dBTP, c = {T.dbtp(C1):+.4f} dBTP")
    assert moved <= ref_moved + 1e-9
    assert float(tp_after[0]) <= float(C1) + 2.0 * overshoot
    assert (target == -16.0) == (out.tobytes() == ref["gained"].tobytes())  # the limiter works at -12 LUFS alone
