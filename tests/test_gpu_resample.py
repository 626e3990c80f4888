"""Sample-rate conversion on the GPU (include/melonix_amd.h "Sample-rate conversion"): byte for byte tests/resample_ref.py's over the
library's own table at the smallest shapes that can go wrong — the eight ratio classes (more phases than threads, the longest
windows, tables staged in LDS and tables read from memory), lengths around the period and the window, outputs at every 4-byte
alignment — whatever the launch split; products j M past 2^32; the six laws of the definition; nothing written outside the outputs;
the refusals; equal rates; and the export chain at another rate end to end."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as L
import resample_ref as R
import truepeak_ref as T
from conftest import DevBuf
from guarded import pcm_dev_range

pytestmark = pytest.mark.gpu

IDS = lambda p: f"{p[0]}-{p[1]}"  # noqa: E731
PAD = 4096  # the stretch of either pad that is read back


@pytest.fixture(scope="module")
def tables(mxlib):
    made = {}

    def get(pair):
        if pair not in made:
            t = mxlib.resample_taps(*pair)
            t.setflags(write=False)
            made[pair] = (R.plan(*pair), t)
        return made[pair]

    return get


def dev_range(ctx, audio, pair, first, count, shift=0):
    """The range form into a guarded buffer -> the outputs; the guards must stand."""
    return pcm_dev_range(lambda d, _: (ctx.resample_dev(audio, pair[0], pair[1], first, count, d), ctx.synchronize()), count, shift)[0]


@pytest.mark.parametrize("pair", R.PAIRS, ids=IDS)
def test_bytes_are_the_references(mxlib, gpu_ctx, tables, pair):
    """Noise with sparse clicks at lengths 0, 1, 2, M - 1, M, M + 1, T and 10007: the range form at output addresses shifted by 0, 4,
    8 and 12 bytes, the host form, and the new audio object with its length and both pads."""
    p, t = tables(pair)
    for n in (0, 1, 2, p["M"] - 1, p["M"], p["M"] + 1, p["taps"], 10007):
        w = R.take(n, seed=pair[0] + n)
        want = R.resample(w, p, t)
        m = len(want)
        assert m == mxlib.resample_length(n, *pair)
        a = gpu_ctx.upload(w)
        b = None
        try:
            for shift in (0, 4, 8, 12):
                got = dev_range(gpu_ctx, a, pair, 0, m, shift)
                assert got.tobytes() == want.tobytes(), (pair, n, shift, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
            assert gpu_ctx.resample_range(a, *pair).tobytes() == want.tobytes(), (pair, n)
            b = gpu_ctx.resample(a, *pair)
            assert b.n == m == mxlib._capi.lib().mx_audio_length(b.handle)
            body, left, right = gpu_ctx.audio_download(b), gpu_ctx.audio_download(b, -PAD, PAD), gpu_ctx.audio_download(b, m, PAD)
        finally:
            if b is not None:
                b.free()
            a.free()
        assert body.tobytes() == want.tobytes(), (pair, n)
        assert len(left) == PAD == len(right) and not left.view(np.uint32).any() and not right.view(np.uint32).any(), (pair, n)  # +0.0f


@pytest.mark.parametrize("pair", ((48000, 44100), (8000, 44100), (192000, 44100)), ids=IDS)
def test_same_bytes_whatever_the_split(gpu_ctx, tables, pair):
    """n = 20011 at 147 / 160, 441 / 80 (more phases than threads) and 147 / 640 (the longest window): single outputs, uneven
    thirds, empty ranges, ranges that end inside a tile, the host form of a range."""
    p, t = tables(pair)
    n = 20011
    w = R.take(n, seed=pair[1])
    want = R.resample(w, p, t)
    m = len(want)
    a = gpu_ctx.upload(w)
    try:
        cuts = (0, m // 3 - 7, m // 3 - 7, (2 * m) // 3 + 11, m)
        parts = [dev_range(gpu_ctx, a, pair, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        assert b"".join(x.tobytes() for x in parts) == want.tobytes()
        for j in (0, 1, 255, 256, 767, 768, 2047, 2048, 2049, m - 2, m - 1):
            assert dev_range(gpu_ctx, a, pair, j, 1).tobytes() == want[j:j + 1].tobytes(), j
        for lo, count in ((0, 100), (5, 2048 + 300), (300, min(4 * 2048 - 1, m - 400)), (m - 1000, 1000), (2047, 2), (m, 0), (17, 0)):
            assert dev_range(gpu_ctx, a, pair, lo, count, shift=4).tobytes() == want[lo:lo + count].tobytes(), (lo, count)
        assert gpu_ctx.resample_range(a, pair[0], pair[1], 1000, m - 1500).tobytes() == want[1000:m - 500].tobytes()
        assert len(gpu_ctx.resample_range(a, pair[0], pair[1], m, 0)) == 0
    finally:
        a.free()


def test_products_past_32_bits(mxlib, gpu_ctx, tables):
    """n = 9 800 000 at 8000 -> 44100 (441 / 80): the 4096 outputs astride j M = 2^32 and the last 4096, through the range form,
    from one upload."""
    pair = (8000, 44100)
    p, t = tables(pair)
    n = 9_800_000
    w = R.take(n, seed=32)
    m = R.length(n, p)
    j32 = 2 ** 32 // p["M"]
    assert m == mxlib.resample_length(n, *pair) and j32 + 2048 < m and (j32 - 1) * p["M"] < 2 ** 32 <= (j32 + 1) * p["M"]
    a = gpu_ctx.upload(w)
    try:
        for first in (j32 - 2048, m - 4096):
            got = dev_range(gpu_ctx, a, pair, first, 4096)
            want = R.resample(w, p, t, first, 4096)
            assert got.tobytes() == want.tobytes(), (first, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    finally:
        a.free()


@pytest.mark.parametrize("pair", ((48000, 44100), (44100, 48000), (8000, 44100), (192000, 44100)), ids=IDS)
def test_the_laws_on_the_device(gpu_ctx, tables, pair):
    """Laws 1-6 of the definition (tests/resample_ref.py check_laws, the assertions the emulation is held to)."""

    def run(w, first=0, count=None):
        a = gpu_ctx.upload(w)
        try:
            return gpu_ctx.resample_range(a, pair[0], pair[1], first, count)
        finally:
            a.free()

    R.check_laws(run, *tables(pair))


def test_refusals_write_nothing(mxlib, gpu_ctx):
    """Rates out of range, L > 1024, T > 512, a range outside [0, m), a null output with count > 0, a misaligned device output,
    null handles: MX_ERR_INVALID with a message, nothing written, *out untouched; the context works on."""
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    n = 4801
    w = R.take(n, seed=1)
    m = R.length(n, R.plan(48000, 44100))
    a = gpu_ctx.upload(w)
    buf = DevBuf(4 * m + 64, fill=0xA5)
    host = np.full(4 * m + 64, 0xA5, dtype=np.uint8)
    marker = 0x5A5A5A5A
    try:
        bad = [(7999, 44100, 0, 1), (48000, 384001, 0, 1), (0, 44100, 0, 1), (48000, -44100, 0, 1), (44100, 48001, 0, 1), (384000, 44100, 0, 1),
               (48000, 44100, -1, 1), (48000, 44100, 0, -1), (48000, 44100, 0, m + 1), (48000, 44100, m, 1), (48000, 44100, m + 1, 0),
               (48000, 44100, 2, m - 1), (48000, 44100, 1, 2 ** 62), (48000, 48000, 0, n + 1)]
        for name, out in (("mx_resample_dev", buf.ptr), ("mx_resample", host.ctypes.data)):
            fn = getattr(lib, name)
            for rin, rout, first, count in bad:
                assert fn(gpu_ctx.handle, a.handle, rin, rout, first, count, C.c_void_p(out)) == INVALID, (name, rin, rout, first, count)
                assert lib.mx_last_error(), (name, rin, rout, first, count)
            assert fn(gpu_ctx.handle, a.handle, 48000, 44100, 0, 1, None) == INVALID and b"null" in lib.mx_last_error()
            assert fn(None, a.handle, 48000, 44100, 0, 1, C.c_void_p(out)) == INVALID
            assert fn(gpu_ctx.handle, None, 48000, 44100, 0, 1, C.c_void_p(out)) == INVALID
        assert lib.mx_resample_dev(gpu_ctx.handle, a.handle, 48000, 44100, 0, 1, C.c_void_p(buf.ptr + 2)) == INVALID
        assert b"aligned" in lib.mx_last_error()
        made = C.c_void_p(marker)
        for rin, rout in ((7999, 44100), (48000, 384001), (44100, 48001), (384000, 44100)):
            assert lib.mx_audio_resample(gpu_ctx.handle, a.handle, rin, rout, C.byref(made)) == INVALID and lib.mx_last_error(), (rin, rout)
        assert lib.mx_audio_resample(None, a.handle, 48000, 44100, C.byref(made)) == INVALID
        assert lib.mx_audio_resample(gpu_ctx.handle, None, 48000, 44100, C.byref(made)) == INVALID
        assert lib.mx_audio_resample(gpu_ctx.handle, a.handle, 48000, 44100, None) == INVALID and made.value == marker
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5) and np.all(host == 0xA5)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.resample(a, 44100, 48001)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.resample_range(a, 48000, 44100, 0, m + 1)
        # the context works on: an empty range with a null output, and an empty take
        assert lib.mx_resample_dev(gpu_ctx.handle, a.handle, 48000, 44100, 5, 0, None) == 0
        assert lib.mx_resample(gpu_ctx.handle, a.handle, 48000, 44100, m, 0, None) == 0
        e = gpu_ctx.upload(np.zeros(0, np.float32))
        b = gpu_ctx.resample(e, 48000, 44100)
        assert b.n == 0 and len(gpu_ctx.resample_range(e, 48000, 44100)) == 0
        b.free()
        e.free()
    finally:
        buf.free()
        a.free()


def test_equal_rates_give_the_inputs_bytes(mxlib, gpu_ctx):
    """Every form copies: NaN payloads and -0.0f survive, the new object has the length and zeroed pads."""
    n = 5003
    w = R.take(n, seed=2)
    w[7], w[8] = np.float32(-0.0), np.float32(np.inf)
    w.view(np.uint32)[9] = 0x7FC12345  # a NaN with a payload
    a = gpu_ctx.upload(w)
    try:
        for sr in (8000, 44100, 384000):
            assert mxlib.resample_length(n, sr, sr) == n
            assert dev_range(gpu_ctx, a, (sr, sr), 0, n, shift=4).tobytes() == w.tobytes()
            assert dev_range(gpu_ctx, a, (sr, sr), 5, 100).tobytes() == w[5:105].tobytes()
            assert gpu_ctx.resample_range(a, sr, sr, 3, 1000).tobytes() == w[3:1003].tobytes()
            b = gpu_ctx.resample(a, sr, sr)
            try:
                assert b.n == n and gpu_ctx.audio_download(b).tobytes() == w.tobytes()
                assert not gpu_ctx.audio_download(b, -PAD, PAD).view(np.uint32).any() and not gpu_ctx.audio_download(b, n, PAD).view(np.uint32).any()
            finally:
                b.free()
    finally:
        a.free()


def test_the_export_chain_at_another_rate(mxlib, gpu_ctx, tables):
    """The levelling take of tests/test_gpu_loudness.py scaled to peak at 1.5, from 48000 to 44100 Hz at -12 LUFS under -1 dBTP:
    the gain from the measurement at 48 kHz -> mx_audio_resample -> mx_audio_limit with the defaults at 44.1 kHz and its int16,
    against tests/resample_ref.py export_chain_at: the converted and the limited samples and the int16 by bytes; no sample over the
    ceiling.  MEASURED, re-metered at 44.1 kHz (the reference chain on the CPU, and the GPU chain's wherever the bytes
    agree, which the test asserts): 114 660 samples, true peak -0.99997 dBTP (2.7e-5 dB over c), -14.2994 LUFS."""
    sr, out_rate, target = L.LEVEL_SR, 44100, -12.0
    pair = (sr, out_rate)
    w = L.levelling_take()[0]
    w = (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)
    tp_taps = mxlib.true_peak_taps()
    p, t = tables(pair)
    ref = R.export_chain_at(w, sr, out_rate, mxlib.loudness_coeffs(sr), mxlib.loudness_coeffs(out_rate), tp_taps, t, target)
    a = gpu_ctx.upload(w)
    made = []
    try:
        before = gpu_ctx.loudness_measure(a, sr)
        amp = mxlib.normalize_gain_tp(before, gpu_ctx.true_peak(a, sr)[0], target, 200.0)  # (the loudness term alone)
        assert np.float32(amp).tobytes() == ref["amp"].tobytes()
        made.append(gpu_ctx.audio_gain(a, [(0, amp)]))
        made.append(gpu_ctx.resample(made[0], sr, out_rate))
        converted = gpu_ctx.audio_download(made[1])
        b, pcm = gpu_ctx.limit(made[1], out_rate, ceiling_db=-1.0, pcm16=True)
        made.append(b)
        out = gpu_ctx.audio_download(b)
        after = gpu_ctx.loudness_measure(b, out_rate)
        tp_after = gpu_ctx.true_peak(b, out_rate)
    finally:
        for b in made:
            b.free()
        a.free()
    assert len(converted) == mxlib.resample_length(len(w), sr, out_rate) and converted.tobytes() == ref["converted"].tobytes()
    assert out.tobytes() == ref["out"].tobytes() and pcm.tobytes() == ref["pcm"].tobytes()
    assert np.abs(out).max() <= T.MINUS_1_DBTP and np.abs(pcm.astype(np.int32)).max() <= 32767 * float(T.MINUS_1_DBTP)
    assert np.abs(converted).max() > 1.0  # (the limiter had work to do)
    print(f"at {out_rate} Hz: loudness {after['integrated']:.6f} LUFS (the reference chain {ref['after']['integrated']:.6f}), true peak "
          f"{T.dbtp(tp_after[0]):+.4f} dBTP (the reference chain {T.dbtp(ref['tp_after'][0]):+.4f}), c = {T.dbtp(T.MINUS_1_DBTP):+.4f} dBTP")
    assert tp_after == ref["tp_after"] and abs(after["integrated"] - ref["after"]["integrated"]) <= 1e-9
