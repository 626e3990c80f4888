"""Noise reduction on the GPU (include/melonix_amd.h "Noise reduction"): the device within the project's yardstick of
tests/denoise_ref.py through the range form, the host form and mx_audio_denoise, on the takes and lengths of
tests/test_denoise_host.py, at output addresses shifted by 0, 4, 8, 12 bytes (f32) and 0, 2 bytes (int16); the same bytes whatever
the split or the run length; the device print against the library's host form on the same rows, byte for byte, and against the
reference; the laws of the definition; guard bands around every device output; every refusal before any launch; the longest take;
and the device's bytes beside the CPU emulation's."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import emu_build
import far_take as FT
from conftest import DevBuf
from far_take import far  # noqa: F401  (the module's far-take fixture)
from guarded import Guarded, pcm_dev_range

pytestmark = pytest.mark.gpu

PAD = 4096  # the stretch of either pad that is read back
SET = (24.0, 6.0)


def dev_range(ctx, audio, P, setting, first, count, shift=0, shift16=0, f32=True, i16=False):
    """The range form into guarded buffers -> (f32 | None, int16 | None); the guards must stand."""
    return pcm_dev_range(lambda f, i: (ctx.denoise_dev(audio, P, setting[0], setting[1], first, count, f, i), ctx.synchronize()),
                         count, shift, shift16, f32, i16)


@pytest.fixture(scope="module")
def vowel(mxlib):
    x = D.vowel_take(1e-2)
    x.setflags(write=False)
    P = D.noise_print(x, 0, 12000).astype(np.float32)
    refs = {s: D.denoise(x, P, *mxlib.denoise_factors(*s)) for s in D.SETTINGS}
    return x, P, refs


def test_the_vowel_take_through_every_form(mxlib, gpu_ctx, vowel):
    """The range form at every output alignment, the host form, the new audio object (length, both pads zero), int16 within 1 LSB
    of the reference's and exactly the conversion of the device's own f32."""
    x, P, refs = vowel
    n = len(x)
    a = gpu_ctx.upload(x)
    b = None
    try:
        for s in D.SETTINGS:
            first = None
            for shift, shift16 in ((0, 0), (4, 2), (8, 0), (12, 2)):
                got, pcm = dev_range(gpu_ctx, a, P, s, 0, n, shift, shift16, i16=True)
                w = D.assert_close(got, refs[s], (s, shift))
                first = got if first is None else first
                assert got.tobytes() == first.tobytes() and pcm.tobytes() == D.pcm16(got).tobytes(), (s, shift)
                assert np.abs(pcm.astype(np.int32) - D.pcm16(refs[s]).astype(np.int32)).max() <= 1
            print(f"{s}: worst deviation {w:.4f} of the yardstick")
            hf, hi = gpu_ctx.denoise_range(a, P, *s, want_i16=True)
            assert hf.tobytes() == first.tobytes() and hi.tobytes() == D.pcm16(first).tobytes()
            assert dev_range(gpu_ctx, a, P, s, 0, n, f32=False, i16=True)[1].tobytes() == hi.tobytes()
            b = gpu_ctx.denoise(a, P, *s)
            assert b.n == n == mxlib._capi.lib().mx_audio_length(b.handle)
            body, left, right = gpu_ctx.audio_download(b), gpu_ctx.audio_download(b, -PAD, PAD), gpu_ctx.audio_download(b, n, PAD)
            b.free()
            b = None
            assert body.tobytes() == first.tobytes()
            assert len(left) == PAD == len(right) and not left.view(np.uint32).any() and not right.view(np.uint32).any()
    finally:
        if b is not None:
            b.free()
        a.free()


@pytest.mark.parametrize("take", ("noise", "clicks"))
def test_every_length(mxlib, gpu_ctx, take):
    """Lengths 0, 1, 255 .. 1025 and 10 007 and the 10 ms file: the range form, the host form and the audio object."""
    fl, se = mxlib.denoise_factors(*SET)
    takes = [(D.noise_take(n, seed=n) if take == "noise" else D.click_take(n, seed=n), D.flat_print(3e-8 if take == "noise" else 1e-10))
             for n in D.LENGTHS]
    takes.append((D.short_take(), D.noise_print(D.noise_take(2048, seed=3), 0, 2048).astype(np.float32)))
    for x, P in takes:
        n = len(x)
        ref = D.denoise(x, P, fl, se)
        a = gpu_ctx.upload(x)
        b = None
        try:
            got = dev_range(gpu_ctx, a, P, SET, 0, n, shift=4)[0] if n else np.zeros(0, np.float32)
            D.assert_close(got, ref, (take, n))
            assert gpu_ctx.denoise_range(a, P, *SET)[0].tobytes() == got.tobytes(), n
            b = gpu_ctx.denoise(a, P, *SET)
            assert b.n == n and gpu_ctx.audio_download(b).tobytes() == got.tobytes(), n
            assert not gpu_ctx.audio_download(b, -PAD, PAD).view(np.uint32).any() and not gpu_ctx.audio_download(b, n, PAD).view(np.uint32).any()
        finally:
            if b is not None:
                b.free()
            a.free()


def test_same_bytes_whatever_the_split_and_the_run(gpu_ctx, vowel):
    """The whole range; a split at 37 and at 257; single outputs; ranges that end inside a block; 1, 5 and 32 blocks a wavefront
    (the context's pinned run length) and the default; the host form = the device form."""
    x, P, _ = vowel
    x = x[10000:20007]
    n = len(x)
    a = gpu_ctx.upload(x)
    try:
        whole, pcm = dev_range(gpu_ctx, a, P, SET, 0, n, i16=True)
        try:
            for run in (1, 5, 32):
                gpu_ctx.set_frames_per_block(run)
                assert dev_range(gpu_ctx, a, P, SET, 0, n)[0].tobytes() == whole.tobytes(), run
                for cuts in ((0, 37, n), (0, 257, n), (0, 255, 256, 1023, 1025, 8192, n)):
                    parts = [dev_range(gpu_ctx, a, P, SET, lo, hi - lo, shift=4, shift16=2, i16=True) for lo, hi in zip(cuts, cuts[1:])]
                    assert b"".join(p[0].tobytes() for p in parts) == whole.tobytes(), (run, cuts)
                    assert b"".join(p[1].tobytes() for p in parts) == pcm.tobytes(), (run, cuts)
        finally:
            gpu_ctx.set_frames_per_block(0)
        for j in (0, 1, 255, 256, 257, 1023, 1024, n - 2, n - 1):
            assert dev_range(gpu_ctx, a, P, SET, j, 1)[0].tobytes() == whole[j:j + 1].tobytes(), j
        hf, hi = gpu_ctx.denoise_range(a, P, *SET, first=1000, count=n - 1500, want_i16=True)
        assert hf.tobytes() == whole[1000:n - 500].tobytes() and hi.tobytes() == pcm[1000:n - 500].tobytes()
        assert len(gpu_ctx.denoise_range(a, P, *SET, first=n, count=0)[0]) == 0
    finally:
        a.free()


def test_the_device_print(mxlib, gpu_ctx):
    """Regions of 1, 2, 43 and 8192 frames: the device's rows (guarded) through the library's host form give the bytes of the
    device's print (guarded: 513 values and nothing beyond them) and of the host form mx_noise_print; within 2e-5 relative of the
    reference's."""
    big = 1024 + 8191 * 256
    x = D.noise_take(big + 300, level=1e-2, seed=9)
    a = gpu_ctx.upload(x)
    try:
        for begin, end in ((0, 1024), (100, 100 + 1024 + 256 + 255), (0, 12000), (256, 256 + big)):
            f0, count = D.region_frames(len(x), begin, end)
            gr, gp = Guarded(count * D.BINS * 4, 4), Guarded(D.BINS * 4, 8)
            try:
                gpu_ctx.noise_rows_dev(a, f0, count, gr.ptr)
                gpu_ctx.noise_print_dev(a, begin, end, gp.ptr)
                gpu_ctx.synchronize()
                rows = gr.take(np.float32).reshape(count, D.BINS)
                dev = gp.take(np.float32)
            finally:
                gr.free()
                gp.free()
            assert dev.tobytes() == mxlib.noise_print_rows(rows).tobytes() == gpu_ctx.noise_print(a, begin, end).tobytes(), (begin, end)
            want = D.noise_print(x[:end + 1024] if end < 20000 else x, begin, end)
            assert np.abs(dev / want - 1.0).max() <= 2e-5, (begin, end)
    finally:
        a.free()


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_the_laws_on_the_device(mxlib, gpu_ctx, setting):
    fl, se = mxlib.denoise_factors(*setting)

    def run(x, P, first=0, count=None):
        a = gpu_ctx.upload(x)
        try:
            return gpu_ctx.denoise_range(a, P, setting[0], setting[1], first, count)[0]
        finally:
            a.free()

    D.check_laws(run, fl, se)


def test_refusals_happen_before_any_launch(mxlib, gpu_ctx):
    """Parameters out of range or NaN, a bad print, bad regions, ranges outside [0, n), null pointers, misaligned outputs:
    MX_ERR_INVALID with a message, nothing written, *out untouched; then the context works on."""
    lib, INVALID, DP = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID, mxlib._capi.DenoiseParams
    n = 5000
    x = D.noise_take(n, seed=1)
    ok = D.flat_print(1e-7)
    a = gpu_ctx.upload(x)
    buf = DevBuf(4 * n + 64, fill=0xA5)
    host = np.full(4 * n + 64, 0xA5, dtype=np.uint8)
    p = C.byref(DP(12.0, 6.0))
    vp = C.c_void_p
    try:
        bad_params = [DP(-0.1, 0.0), DP(60.5, 0.0), DP(float("nan"), 0.0), DP(10.0, -12.5), DP(10.0, 24.5), DP(10.0, float("nan"))]
        bad_prints = []
        for k, v in ((0, -1e-30), (512, float("nan")), (100, float("inf"))):
            q = ok.copy()
            q[k] = v
            bad_prints.append(q)
        spans = [(-1, 1), (0, -1), (0, n + 1), (n, 1), (n + 1, 0), (2, n - 1), (1, 2 ** 62)]
        for name, out in (("mx_denoise_dev", buf.ptr), ("mx_denoise", host.ctypes.data)):
            fn = getattr(lib, name)
            for bp in bad_params:
                assert fn(gpu_ctx.handle, a.handle, ok.ctypes.data, C.byref(bp), 0, 8, vp(out), None) == INVALID and lib.mx_last_error()
            for q in bad_prints:
                assert fn(gpu_ctx.handle, a.handle, q.ctypes.data, p, 0, 8, vp(out), None) == INVALID and lib.mx_last_error()
            for first, count in spans:
                assert fn(gpu_ctx.handle, a.handle, ok.ctypes.data, p, first, count, vp(out), vp(out)) == INVALID, (name, first, count)
            assert fn(gpu_ctx.handle, a.handle, ok.ctypes.data, p, 0, 8, None, None) == INVALID and b"null" in lib.mx_last_error()
            assert fn(gpu_ctx.handle, a.handle, None, p, 0, 8, vp(out), None) == INVALID
            assert fn(gpu_ctx.handle, a.handle, ok.ctypes.data, None, 0, 8, vp(out), None) == INVALID
            assert fn(None, a.handle, ok.ctypes.data, p, 0, 8, vp(out), None) == INVALID
            assert fn(gpu_ctx.handle, None, ok.ctypes.data, p, 0, 8, vp(out), None) == INVALID
        assert lib.mx_denoise_dev(gpu_ctx.handle, a.handle, ok.ctypes.data, p, 0, 8, vp(buf.ptr + 2), None) == INVALID and b"aligned" in lib.mx_last_error()
        assert lib.mx_denoise_dev(gpu_ctx.handle, a.handle, ok.ctypes.data, p, 0, 8, None, vp(buf.ptr + 1)) == INVALID
        for name, out in (("mx_noise_print_dev", buf.ptr), ("mx_noise_print", host.ctypes.data)):
            fn = getattr(lib, name)
            for begin, end in ((0, 1023), (1, 1024), (0, 0), (-1, 2000), (0, n + 1), (3000, 2000), (4000, n)):
                assert fn(gpu_ctx.handle, a.handle, begin, end, vp(out)) == INVALID and lib.mx_last_error(), (name, begin, end)
            assert fn(gpu_ctx.handle, a.handle, 0, 2048, None) == INVALID
            assert fn(None, a.handle, 0, 2048, vp(out)) == INVALID and fn(gpu_ctx.handle, None, 0, 2048, vp(out)) == INVALID
        assert lib.mx_noise_print_dev(gpu_ctx.handle, a.handle, 0, 2048, vp(buf.ptr + 2)) == INVALID
        F = D.frames(n)
        for f0, count in ((-1, 1), (0, F + 1), (F, 1), (F + 1, 0), (0, -1)):
            assert lib.mx_noise_rows_dev(gpu_ctx.handle, a.handle, f0, count, vp(buf.ptr)) == INVALID, (f0, count)
        assert lib.mx_noise_rows_dev(gpu_ctx.handle, a.handle, 0, 1, None) == INVALID
        assert lib.mx_noise_rows_dev(gpu_ctx.handle, a.handle, 0, 1, vp(buf.ptr + 2)) == INVALID
        marker = 0x5A5A5A5A
        made = vp(marker)
        for bp in bad_params:
            assert lib.mx_audio_denoise(gpu_ctx.handle, a.handle, ok.ctypes.data, C.byref(bp), C.byref(made)) == INVALID
        for q in bad_prints:
            assert lib.mx_audio_denoise(gpu_ctx.handle, a.handle, q.ctypes.data, p, C.byref(made)) == INVALID
        assert lib.mx_audio_denoise(gpu_ctx.handle, a.handle, None, p, C.byref(made)) == INVALID
        assert lib.mx_audio_denoise(gpu_ctx.handle, a.handle, ok.ctypes.data, None, C.byref(made)) == INVALID
        assert lib.mx_audio_denoise(gpu_ctx.handle, a.handle, ok.ctypes.data, p, None) == INVALID and made.value == marker
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5) and np.all(host == 0xA5)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.denoise(a, ok, 61.0, 6.0)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.noise_print(a, 0, 1000)
        # the context works on: empty ranges with null outputs, an empty take
        assert lib.mx_denoise_dev(gpu_ctx.handle, a.handle, ok.ctypes.data, p, 5, 0, None, None) == 0
        assert lib.mx_denoise(gpu_ctx.handle, a.handle, ok.ctypes.data, p, n, 0, None, None) == 0
        assert lib.mx_noise_rows_dev(gpu_ctx.handle, a.handle, 3, 0, None) == 0
        e = gpu_ctx.upload(np.zeros(0, np.float32))
        b = gpu_ctx.denoise(e, ok)
        assert b.n == 0 and len(gpu_ctx.denoise_range(e, ok)[0]) == 0
        b.free()
        e.free()
    finally:
        buf.free()
        a.free()


@pytest.mark.parametrize("island", ("B2G", "B4G", "END"))
def test_the_longest_take(gpu_ctx, far, island):
    """The range form over an island of the longest take the header admits equals the island uploaded as a take of its own, byte
    for byte, f32 and int16; the print is learned on the control."""
    q, w = FT.window(island, D.H)
    lo, hi = FT.span(island)
    control = gpu_ctx.upload(w)
    try:
        P = gpu_ctx.noise_print(control, lo - q, lo - q + 12000)
        first, end = lo - 1500, min(hi + 1500, FT.N_MAX)
        cf, ci = dev_range(gpu_ctx, control, P, SET, first - q, end - first, i16=True)
        ff, fi = dev_range(gpu_ctx, far.audio, P, SET, first, end - first, shift=4, shift16=2, i16=True)
        assert np.abs(cf).max() > 0.01 and ff.tobytes() == cf.tobytes() and fi.tobytes() == ci.tobytes()
        assert gpu_ctx.noise_print(far.audio, lo, lo + 12000).tobytes() == P.tobytes()
    finally:
        control.free()


def test_the_device_beside_the_emulation(mxlib, gpu_ctx, vowel):
    """EXPECTED (contraction off, + - x and one correctly rounded division per bin): the device's bytes are the CPU emulation's.
    Reports the first differing values where they are not; the yardstick tests above are the requirement."""
    lib = C.CDLL(emu_build.shared_object("denoise_emu", ["denoise_emu.cpp", "denoise_logic.cpp"],
                                         ["denoise_core.h", "denoise_logic.h", "onset_core.h", "pcm16.h"]))
    ll, vp = C.c_longlong, C.c_void_p
    lib.emu_denoise.argtypes, lib.emu_denoise.restype = [vp, ll, vp, C.c_float, C.c_float, ll, ll, C.c_int, vp, vp], ll
    lib.emu_noise_rows.argtypes, lib.emu_noise_rows.restype = [vp, ll, ll, ll, C.c_int, vp], ll
    x, P, _ = vowel
    x = np.ascontiguousarray(x[10000:20007])
    n = len(x)
    fl, se = mxlib.denoise_factors(*SET)
    emu = np.zeros(n, np.float32)
    assert lib.emu_denoise(x.ctypes.data, n, P.ctypes.data, fl, se, 0, n, 32, emu.ctypes.data, None) == 0
    F = D.frames(n)
    emu_rows = np.zeros((F, D.BINS), np.float32)
    assert lib.emu_noise_rows(x.ctypes.data, n, 0, F, 1, emu_rows.ctypes.data) == 0
    a = gpu_ctx.upload(x)
    g = Guarded(F * D.BINS * 4)
    try:
        dev = gpu_ctx.denoise_range(a, P, *SET)[0]
        gpu_ctx.noise_rows_dev(a, 0, F, g.ptr)
        gpu_ctx.synchronize()
        rows = g.take(np.float32).reshape(F, D.BINS)
    finally:
        g.free()
        a.free()
    for what, d, e in (("power rows", rows.ravel(), emu_rows.ravel()), ("outputs", dev, emu)):
        diff = np.flatnonzero(d.view(np.uint32) != e.view(np.uint32))
        print(f"{what}: {len(diff)} of {len(d)} values differ from the emulation's" +
              (f"; the first at {diff[0]}: device {d[diff[0]]!r}, emulation {e[diff[0]]!r}" if len(diff) else ""))
    D.assert_close(dev, emu, "device against emulation")
    D.assert_close(rows.ravel(), emu_rows.ravel(), "device rows against the emulation's")
