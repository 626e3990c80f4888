"""The dynamics compressor on the GPU (include/melonix_amd.h "Dynamics compressor"): the device's peaks, curve, f32 and int16 are
the CPU emulation's (tests/emu/compress_emu.cpp) byte for byte — and with it tests/compress_ref.py's, which
tests/test_compress_host.py holds the emulation to — through the range form, the host form, the new audio object and the _dev
forms, at the lengths, rates and settings of the host tests, f32 and int16 at shifted addresses; the same bytes whatever the
split; the laws of the definition; guard bands around every device output; every refusal before any launch; the longest take."""
import ctypes as C

import numpy as np
import pytest

import compress_ref as R
import far_take as FT
from conftest import DevBuf
from test_compress_host import LENGTHS, SETTINGS, load_emu, take_of
from far_take import far  # noqa: F401  (the module's far-take fixture)
from guarded import Guarded, pcm_dev_range

pytestmark = pytest.mark.gpu

PAD = 4096  # the stretch of either pad that is read back


@pytest.fixture(scope="module")
def emu(mxlib):
    return load_emu(mxlib)


def dev_range(ctx, audio, sr, p, first, count, shift=0, shift16=0, f32=True, i16=False):
    """The range form into guarded buffers -> (f32 | None, int16 | None); the guards must stand."""
    return pcm_dev_range(lambda f, i: (ctx.compress_dev(audio, sr, first, count, f, i, **p), ctx.synchronize()),
                         count, shift, shift16, f32, i16)


def dev_steps(ctx, audio, sr, p, first_step, nsteps, shift=4):
    """mx_compress_peaks_dev and mx_compress_gain_dev into guarded buffers -> (peaks f32, gain int32)"""
    gp, gg = Guarded(nsteps * 4, shift), Guarded(nsteps * 4, shift + 4)
    try:
        ctx.compress_peaks_dev(audio, sr, first_step, nsteps, gp.ptr)
        ctx.compress_gain_dev(audio, sr, first_step, nsteps, gg.ptr, **p)
        ctx.synchronize()
        return gp.take(np.float32), gg.take(np.int32)
    finally:
        gp.free()
        gg.free()


class Device:
    """what compress_ref.check_laws asks of an implementation, on the device through the host forms"""

    def __init__(self, mxlib, ctx, sr, p):
        self.ctx, self.sr, self.p = ctx, sr, p
        self.T, self.plan = mxlib.compress_curve(**p), mxlib.compress_plan(sr, **p)

    def run(self, x, first=0, count=None):
        a = self.ctx.upload(x)
        try:
            return self.ctx.compress_range(a, self.sr, first, count, **self.p)[0]
        finally:
            a.free()

    def gain(self, x):
        a = self.ctx.upload(x)
        try:
            return self.ctx.compress_gain(a, self.sr, **self.p)
        finally:
            a.free()


@pytest.mark.parametrize("kind", ("envelope", "clicks"))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_device_is_the_emulation_through_every_form(mxlib, gpu_ctx, emu, setting, kind):
    """Peaks, curve, f32 and int16 of every listed length at 48 kHz, and of 8, 44.1 and 384 kHz: the _dev forms into guarded
    buffers (f32 4 bytes, int16 2 bytes off a 16-byte line: launches that end in a partial step and a partial group), the host
    forms, the audio object (length, both pads zero), a range that begins and ends inside a step."""
    p = R.params(**SETTINGS[setting])
    for sr, lengths in LENGTHS.items():
        imp = emu.make(sr)(p)
        for n in lengths:
            x = take_of(kind, n, sr, seed=n % 1000 + 1)
            B = R.steps(n, sr)
            want, want16 = imp.run(x, pcm=True) if n else (np.zeros(0, np.float32), np.zeros(0, np.int16))
            wpk, wg = (imp.peaks(x), imp.gain(x)) if n else (np.zeros(0, np.float32), np.zeros(0, np.int32))
            a = gpu_ctx.upload(x)
            b = None
            try:
                if n:
                    f, i = dev_range(gpu_ctx, a, sr, p, 0, n, shift=4, shift16=2, i16=True)
                    assert f.tobytes() == want.tobytes() and i.tobytes() == want16.tobytes(), (sr, n)
                    assert dev_range(gpu_ctx, a, sr, p, 0, n, f32=False, i16=True)[1].tobytes() == want16.tobytes(), (sr, n)
                    pk, g = dev_steps(gpu_ctx, a, sr, p, 0, B)
                    assert pk.tobytes() == wpk.tobytes() and g.tobytes() == wg.tobytes(), (sr, n)
                hf, hi = gpu_ctx.compress_range(a, sr, want_i16=True, **p)
                assert hf.tobytes() == want.tobytes() and hi.tobytes() == want16.tobytes(), (sr, n)
                assert gpu_ctx.compress_gain(a, sr, **p).tobytes() == wg.tobytes(), (sr, n)
                b = gpu_ctx.compress(a, sr, **p)
                assert b.n == n == mxlib._capi.lib().mx_audio_length(b.handle)
                assert gpu_ctx.audio_download(b).tobytes() == want.tobytes(), (sr, n)
                left, right = gpu_ctx.audio_download(b, -PAD, PAD), gpu_ctx.audio_download(b, n, PAD)
                assert len(left) == PAD == len(right) and not left.view(np.uint32).any() and not right.view(np.uint32).any()
                if n > 5000:
                    lo, hi_ = n // 2 - 1234, n - 7
                    f, i = dev_range(gpu_ctx, a, sr, p, lo, hi_ - lo, shift=12, shift16=6, i16=True)
                    assert f.tobytes() == want[lo:hi_].tobytes() and i.tobytes() == want16[lo:hi_].tobytes(), (sr, n)
                    pk, g = dev_steps(gpu_ctx, a, sr, p, B // 2 - 3, 11, shift=8)
                    assert pk.tobytes() == wpk[B // 2 - 3:B // 2 + 8].tobytes() and g.tobytes() == wg[B // 2 - 3:B // 2 + 8].tobytes()
            finally:
                if b is not None:
                    b.free()
                a.free()


@pytest.mark.parametrize("setting", ("defaults", "slow", "look20"))
def test_same_bytes_whatever_the_split(gpu_ctx, emu, setting):
    """Cuts inside a step, on a step, on a group seam and one sample either side of it, single outputs, at 48 kHz and at 44.1 kHz
    (D = 44: quads that belong to two steps); the host form = the device form."""
    p = R.params(**SETTINGS[setting])
    for sr in (48000, 44100):
        D = R.step_samples(sr)
        n = 2 * R.GC * D + 777
        x = R.envelope_take(n, sr, seed=7)
        a = gpu_ctx.upload(x)
        try:
            whole, pcm = dev_range(gpu_ctx, a, sr, p, 0, n, i16=True)
            assert whole.tobytes() == emu.make(sr)(p).run(x).tobytes()
            cuts = R.cut_points(n, D)
            parts = [dev_range(gpu_ctx, a, sr, p, lo, hi - lo, shift=4, shift16=2, i16=True) for lo, hi in zip(cuts, cuts[1:])]
            assert b"".join(q[0].tobytes() for q in parts) == whole.tobytes(), (sr, cuts)
            assert b"".join(q[1].tobytes() for q in parts) == pcm.tobytes(), (sr, cuts)
            for j in (0, 1, D - 1, D, R.GC * D - 1, R.GC * D, n - 1):
                assert dev_range(gpu_ctx, a, sr, p, j, 1)[0].tobytes() == whole[j:j + 1].tobytes(), (sr, j)
            hf, hi = gpu_ctx.compress_range(a, sr, 1000, n - 1500, want_i16=True, **p)
            assert hf.tobytes() == whole[1000:n - 500].tobytes() and hi.tobytes() == pcm[1000:n - 500].tobytes()
            assert len(gpu_ctx.compress_range(a, sr, n, 0, **p)[0]) == 0
        finally:
            a.free()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_laws_on_the_device(mxlib, gpu_ctx, setting):
    R.check_laws(lambda p: Device(mxlib, gpu_ctx, 48000, p), 48000, SETTINGS[setting])


def test_refusals_happen_before_any_launch(mxlib, gpu_ctx):
    """Parameters out of range or NaN, rates out of range, ranges and steps outside the take, null pointers, misaligned outputs:
    MX_ERR_INVALID with a message, nothing written, *out untouched; then the context works on."""
    lib, INVALID, CP = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID, mxlib._capi.CompressParams
    sr, n = 48000, 5000
    B = R.steps(n, sr)
    x = R.envelope_take(n, sr, seed=1)
    a = gpu_ctx.upload(x)
    buf = DevBuf(4 * n + 64, fill=0xA5)
    host = np.full(4 * n + 64, 0xA5, dtype=np.uint8)
    ok = CP(*(R.DEFAULTS[k] for k in R.FIELDS))
    p, vp, h, au = C.byref(ok), C.c_void_p, gpu_ctx.handle, a.handle
    try:
        bad_params = []
        for k in R.FIELDS:
            lo, hi = R.RANGES[k]
            for v in (float(np.nextafter(np.float32(lo), np.float32(-1e9))), float(np.nextafter(np.float32(hi), np.float32(1e9))), float("nan")):
                bad_params.append(CP(*(float(dict(R.DEFAULTS, **{k: v})[f]) for f in R.FIELDS)))
        spans = [(-1, 1), (0, -1), (0, n + 1), (n, 1), (n + 1, 0), (2, n - 1), (1, 2 ** 62)]
        for name, out in (("mx_compress_dev", buf.ptr), ("mx_compress", host.ctypes.data)):
            fn = getattr(lib, name)
            for bp in bad_params:
                assert fn(h, au, sr, C.byref(bp), 0, 8, vp(out), None) == INVALID and lib.mx_last_error()
            for bad_sr in (7999, 384001):
                assert fn(h, au, bad_sr, p, 0, 8, vp(out), None) == INVALID
            for first, count in spans:
                assert fn(h, au, sr, p, first, count, vp(out), vp(out)) == INVALID, (name, first, count)
            assert fn(h, au, sr, p, 0, 8, None, None) == INVALID and b"null" in lib.mx_last_error()
            assert fn(None, au, sr, p, 0, 8, vp(out), None) == INVALID and fn(h, None, sr, p, 0, 8, vp(out), None) == INVALID
        assert lib.mx_compress_dev(h, au, sr, p, 0, 8, vp(buf.ptr + 2), None) == INVALID and b"aligned" in lib.mx_last_error()
        assert lib.mx_compress_dev(h, au, sr, p, 0, 8, None, vp(buf.ptr + 1)) == INVALID
        for name, out in (("mx_compress_gain_dev", buf.ptr), ("mx_compress_gain", host.ctypes.data)):
            fn = getattr(lib, name)
            for bp in bad_params:
                assert fn(h, au, sr, C.byref(bp), 0, 8, vp(out)) == INVALID
            for f0, count in ((-1, 1), (0, B + 1), (B, 1), (B + 1, 0), (0, -1)):
                assert fn(h, au, sr, p, f0, count, vp(out)) == INVALID, (name, f0, count)
            assert fn(h, au, 7999, p, 0, 1, vp(out)) == INVALID and fn(h, au, sr, p, 0, 1, None) == INVALID
            assert fn(None, au, sr, p, 0, 1, vp(out)) == INVALID and fn(h, None, sr, p, 0, 1, vp(out)) == INVALID
        assert lib.mx_compress_gain_dev(h, au, sr, p, 0, 1, vp(buf.ptr + 2)) == INVALID
        for f0, count in ((-1, 1), (0, B + 1), (B, 1), (B + 1, 0), (0, -1)):
            assert lib.mx_compress_peaks_dev(h, au, sr, f0, count, vp(buf.ptr)) == INVALID, (f0, count)
        assert lib.mx_compress_peaks_dev(h, au, sr, 0, 1, None) == INVALID and lib.mx_compress_peaks_dev(h, au, 384001, 0, 1, vp(buf.ptr)) == INVALID
        assert lib.mx_compress_peaks_dev(h, au, sr, 0, 1, vp(buf.ptr + 2)) == INVALID
        marker = 0x5A5A5A5A
        made = vp(marker)
        for bp in bad_params:
            assert lib.mx_audio_compress(h, au, sr, C.byref(bp), C.byref(made)) == INVALID
        assert lib.mx_audio_compress(h, au, 7999, p, C.byref(made)) == INVALID
        assert lib.mx_audio_compress(h, au, sr, p, None) == INVALID and made.value == marker
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5) and np.all(host == 0xA5)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.compress(a, sr, ratio=0.5)
        with pytest.raises(TypeError):
            gpu_ctx.compress(a, sr, ration=2.0)
        # the context works on: empty ranges with null outputs, NULL parameters (the defaults), an empty take
        assert lib.mx_compress_dev(h, au, sr, p, 5, 0, None, None) == 0 and lib.mx_compress(h, au, sr, p, n, 0, None, None) == 0
        assert lib.mx_compress_gain_dev(h, au, sr, p, 3, 0, None) == 0 and lib.mx_compress_peaks_dev(h, au, sr, B, 0, None) == 0
        f = np.zeros(n, np.float32)
        assert lib.mx_compress(h, au, sr, None, 0, n, f.ctypes.data, None) == 0
        assert f.tobytes() == gpu_ctx.compress_range(a, sr)[0].tobytes()
        e = gpu_ctx.upload(np.zeros(0, np.float32))
        b = gpu_ctx.compress(e, sr)
        assert b.n == 0 and len(gpu_ctx.compress_range(e, sr)[0]) == 0 and len(gpu_ctx.compress_gain(e, sr)) == 0
        b.free()
        e.free()
    finally:
        buf.free()
        a.free()


@pytest.mark.parametrize("island", ("B2G", "B4G", "END"))
def test_the_longest_take(gpu_ctx, far, island):
    """The range form and the curve over an island of the longest take the header admits equal the island uploaded as a take of
    its own, byte for byte, f32, int16, peaks and gains: the control begins on a group seam of the far take (4096 x 48 samples),
    so both cut their groups at the same samples.  Only the groups the range touches pass through work memory."""
    sr, p = 48000, R.params(**SETTINGS["look5"])
    D = R.step_samples(sr)
    q, w = FT.window(island, R.GC * D)
    lo, hi = FT.span(island)
    control = gpu_ctx.upload(w)
    try:
        first, end = lo - 1500, min(hi + 1500, FT.N_MAX)
        cf, ci = dev_range(gpu_ctx, control, sr, p, first - q, end - first, i16=True)
        ff, fi = dev_range(gpu_ctx, far.audio, sr, p, first, end - first, shift=4, shift16=2, i16=True)
        assert np.abs(cf).max() > 0.01 and ff.tobytes() == cf.tobytes() and fi.tobytes() == ci.tobytes()
        assert ff.tobytes() != w[first - q:end - q].tobytes(), "the island is loud enough to be compressed"
        s0, ns = first // D, (end - 1) // D - first // D + 1
        cp, cg = dev_steps(gpu_ctx, control, sr, p, s0 - q // D, ns)
        fp, fg = dev_steps(gpu_ctx, far.audio, sr, p, s0, ns)
        assert fp.tobytes() == cp.tobytes() and fg.tobytes() == cg.tobytes() and cg.min() < R.ONE
    finally:
        control.free()
