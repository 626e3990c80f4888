"""Noise reduction without a GPU (include/melonix_amd.h "Noise reduction"): the kernels' arithmetic in the kernels' lane mapping
and tile walk, run on the CPU by tests/emu/denoise_emu.cpp with every staged index checked, against tests/denoise_ref.py within the
project's yardstick; the same bytes whatever the run length or the split; the print's rows and sum against the library's host
form byte for byte and against the reference; the laws of the definition; every refusal of the host side; sanitizers; the
kernels' resources; known answers measured by the reference."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import emu_build

SOURCES, HEADERS = ["denoise_emu.cpp", "denoise_logic.cpp"], ["denoise_core.h", "denoise_logic.h", "onset_core.h", "pcm16.h"]
RUNS = (1, 5, 32)  # output blocks a wavefront


@pytest.fixture(scope="module")
def emu(mxlib):
    lib = C.CDLL(emu_build.shared_object("denoise_emu", SOURCES, HEADERS))
    ll, vp = C.c_longlong, C.c_void_p
    P = C.POINTER(mxlib._capi.DenoiseParams)
    lib.emu_denoise_frames.argtypes, lib.emu_denoise_frames.restype = [ll], ll
    lib.emu_denoise_factors.argtypes = [P, vp]
    lib.emu_denoise_refuses.argtypes = [P, vp]
    lib.emu_noise_region.argtypes = [ll, ll, ll, C.POINTER(ll), C.POINTER(ll)]
    lib.emu_denoise_tiles.argtypes, lib.emu_denoise_tiles.restype = [ll, ll, C.c_int], ll
    lib.emu_denoise_tile.argtypes = [ll, ll, ll, ll, C.c_int, vp]
    lib.emu_denoise.argtypes, lib.emu_denoise.restype = [vp, ll, vp, C.c_float, C.c_float, ll, ll, C.c_int, vp, vp], ll
    lib.emu_noise_rows.argtypes, lib.emu_noise_rows.restype = [vp, ll, ll, ll, C.c_int, vp], ll
    lib.emu_noise_print.argtypes = [vp, ll, vp]

    class Emu:
        raw = lib

        @staticmethod
        def run(x, P, floor, sens, first=0, count=None, run=32, pcm=False):
            """-> outputs [first, first + count) the kernel's way (no index may leave what is staged); pcm: (f32, int16)"""
            x, P = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(P, dtype=np.float32)
            assert P.shape == (D.BINS,)
            count = len(x) - first if count is None else count
            out, i16 = np.zeros(count, np.float32), np.zeros(count, np.int16)
            bad = lib.emu_denoise(x.ctypes.data, len(x), P.ctypes.data, floor, sens, first, count, run, out.ctypes.data,
                                  i16.ctypes.data if pcm else None)
            assert bad == 0, bad
            return (out, i16) if pcm else out

        @staticmethod
        def rows(x, first_frame, count, run=1):
            x = np.ascontiguousarray(x, dtype=np.float32)
            out = np.zeros((count, D.BINS), np.float32)
            assert lib.emu_noise_rows(x.ctypes.data, len(x), first_frame, count, run, out.ctypes.data) == 0
            return out

        @staticmethod
        def print_of(rows):
            out = np.zeros(D.BINS, np.float32)
            lib.emu_noise_print(rows.ctypes.data, len(rows), out.ctypes.data)
            return out

    return Emu


@pytest.fixture(scope="module")
def factors(mxlib):
    return {s: mxlib.denoise_factors(*s) for s in D.SETTINGS}


@pytest.fixture(scope="module")
def vowel():
    """(take, its print from [0, 12000), {setting: the reference's output}) at both noise levels, computed once"""
    made = {}
    for level in (1e-2, 1e-3):
        x = D.vowel_take(level)
        x.setflags(write=False)
        made[level] = (x, D.noise_print(x, 0, 12000).astype(np.float32), {})
    return made


def test_frames_factors_and_geometry(mxlib, emu):
    for n in (0, 1, 255, 256, 257, 1024, 10007, 2 ** 31 - 65538):
        assert mxlib.denoise_frames(n) == D.frames(n) == emu.raw.emu_denoise_frames(n)
    for red, sen in D.SETTINGS + ((0.0, -12.0), (60.0, 24.0)):
        fl, se = mxlib.denoise_factors(red, sen)
        assert fl == np.float32(10.0 ** (-red / 20.0)) and se == np.float32(10.0 ** (sen / 10.0))
        mine = np.zeros(2, np.float32)
        emu.raw.emu_denoise_factors(C.byref(mxlib._capi.DenoiseParams(red, sen)), mine.ctypes.data)
        assert (mine[0], mine[1]) == (fl, se)
    # the tiles of a range cover its blocks once, in order; a tile's frames exist
    for n, first, count in ((10007, 0, 10007), (10007, 300, 9000), (257, 256, 1), (2 ** 31 - 65538, 2 ** 31 - 65538 - 5000, 5000)):
        for run in RUNS:
            tiles, nxt, t = emu.raw.emu_denoise_tiles(first, count, run), first // D.H, (C.c_longlong * 4)()
            for i in range(tiles):
                emu.raw.emu_denoise_tile(first, count, n, i, run, t)
                b0, b1, fa, F = t
                assert b0 == nxt and b0 < b1 <= b0 + run and fa == max(b0 - 1, 0) and b1 + 2 <= F - 1 == D.frames(n) - 1
                nxt = b1
            assert nxt == -(-(first + count) // D.H)
    assert emu.raw.emu_denoise_tiles(5, 0, 32) == 0


@pytest.mark.parametrize("level", (1e-2, 1e-3))
def test_emulation_is_the_reference_on_the_vowel_take(emu, factors, vowel, level):
    """One second at 48 kHz, the issue's three settings.  MEASURED here: the emulation's worst deviation from the
    reference is below 2 % of the yardstick on every take of this file."""
    x, P, refs = vowel[level]
    for s in D.SETTINGS:
        refs[s] = D.denoise(x, P, *factors[s])
        got, pcm = emu.run(x, P, *factors[s], pcm=True)
        w = D.assert_close(got, refs[s], s)
        print(f"noise {level}, {s}: worst deviation {w:.4f} of the yardstick")
        assert w <= 0.5, "DESIGN 5p says the emulation stays within half the yardstick"
        assert np.abs(pcm.astype(np.int32) - D.pcm16(refs[s]).astype(np.int32)).max() <= 1
        assert pcm.tobytes() == D.pcm16(got).tobytes()


@pytest.mark.parametrize("take", ("noise", "clicks"))
def test_emulation_is_the_reference_at_every_length_and_run(emu, factors, take):
    """Lengths 0, 1, 255 .. 1025 and 10 007 of noise and of a click train, and the 10 ms file, at 1, 5 and 32 blocks a wavefront."""
    fl, se = factors[(24.0, 6.0)]
    worst = 0.0
    for n in D.LENGTHS:
        x = D.noise_take(n, seed=n) if take == "noise" else D.click_take(n, seed=n)
        P = D.flat_print(3e-8 if take == "noise" else 1e-10)
        ref = D.denoise(x, P, fl, se)
        outs = [emu.run(x, P, fl, se, run=r) for r in RUNS]
        worst = max(worst, D.assert_close(outs[0], ref, (take, n)))
        assert all(o.tobytes() == outs[0].tobytes() for o in outs), n
    x = D.short_take()
    P = D.noise_print(np.concatenate([D.noise_take(2048, seed=3)]), 0, 2048).astype(np.float32)
    for r in RUNS:
        worst = max(worst, D.assert_close(emu.run(x, P, fl, se, run=r), D.denoise(x, P, fl, se), "10 ms"))
    print(f"{take}: worst deviation {worst:.4f} of the yardstick")
    assert worst <= 0.5


def test_same_bytes_whatever_the_run_and_the_split(emu, factors, vowel):
    x, P, _ = vowel[1e-2]
    x = x[10000:20007]
    n = len(x)
    fl, se = factors[(12.0, 6.0)]
    whole, pcm = emu.run(x, P, fl, se, pcm=True)
    for r in RUNS:
        assert emu.run(x, P, fl, se, run=r).tobytes() == whole.tobytes()
        for cuts in ((0, 37, n), (0, 257, n), (0, 1, 255, 256, 257, 8191, 8192, n)):
            parts = [emu.run(x, P, fl, se, lo, hi - lo, r, pcm=True) for lo, hi in zip(cuts, cuts[1:])]
            assert b"".join(p[0].tobytes() for p in parts) == whole.tobytes(), (r, cuts)
            assert b"".join(p[1].tobytes() for p in parts) == pcm.tobytes(), (r, cuts)


def test_the_print_is_the_librarys_and_the_references(mxlib, emu):
    """Regions of 1, 2, 43 and 8192 frames: the emulated rows and their ascending binary64 sum give the bytes of the library's host
    form on the same rows, and the reference's print within 2e-5 relative; regions of 0 and 8193 frames are refused."""
    big = 1024 + 8191 * 256
    x = D.noise_take(big + 300, level=1e-2, seed=9)
    for begin, end, frames in ((0, 1024, 1), (100, 100 + 1024 + 256 + 255, 2), (0, 12000, 43), (256, 256 + big, 8192), (5, 12005, 42)):
        f0, count = D.region_frames(len(x), begin, end)
        a, b = C.c_longlong(), C.c_longlong()
        assert emu.raw.emu_noise_region(len(x), begin, end, C.byref(a), C.byref(b)) == 1 and (a.value, b.value) == (f0, count)
        assert count == frames
        rows = emu.rows(x, f0, count, run=7)
        if count <= 43:  # (the rows do not depend on the run)
            assert rows.tobytes() == emu.rows(x, f0, count, run=1).tobytes()
        mine, lib_print = emu.print_of(rows), mxlib.noise_print_rows(rows)
        assert mine.tobytes() == lib_print.tobytes()
        want = D.noise_print(x[:end + 1024] if end < 20000 else x, begin, end)
        assert np.abs(mine / want - 1.0).max() <= 2e-5, (begin, end)
    a, b = C.c_longlong(), C.c_longlong()
    for begin, end in ((0, 1023), (1, 1024), (0, 0), (0, big + 256), (-1, 2000), (0, len(x) + 1), (3000, 2000)):
        assert D.region_frames(len(x), begin, end) is None
        assert emu.raw.emu_noise_region(len(x), begin, end, C.byref(a), C.byref(b)) == 0, (begin, end)


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_the_laws_on_the_cpu(emu, factors, setting):
    fl, se = factors[setting]
    D.check_laws(lambda x, P, first=0, count=None: emu.run(x, P, fl, se, first, count, run=5), fl, se)
    D.check_laws(lambda x, P, first=0, count=None: emu.run(x, P, fl, se, first, count, run=32), fl, se, locality_at=(3999, 1234))


def test_refusals_of_the_host_side(mxlib, emu):
    """Parameters out of range or NaN, a bad print, bad row counts, a negative length, null pointers: MX_ERR_INVALID with a message,
    outputs untouched.  (The refusals that need a context: tests/test_gpu_denoise.py.)"""
    lib, INVALID, DP = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID, mxlib._capi.DenoiseParams
    out = np.full(2, 7.0, np.float32)
    for red, sen in ((-0.1, 0.0), (60.1, 0.0), (float("nan"), 0.0), (10.0, -12.1), (10.0, 24.1), (10.0, float("nan")), (float("inf"), 0.0)):
        assert lib.mx_denoise_factors(C.byref(DP(red, sen)), out.ctypes.data) == INVALID and lib.mx_last_error(), (red, sen)
        assert emu.raw.emu_denoise_refuses(C.byref(DP(red, sen)), None) == 1
    assert lib.mx_denoise_factors(None, out.ctypes.data) == INVALID and lib.mx_denoise_factors(C.byref(DP(12.0, 6.0)), None) == INVALID
    assert np.all(out == 7.0)
    assert lib.mx_denoise_frames(-1) == INVALID
    ok = D.flat_print(1e-6)
    assert emu.raw.emu_denoise_refuses(C.byref(DP(0.0, -12.0)), ok.ctypes.data) == 0 == emu.raw.emu_denoise_refuses(C.byref(DP(60.0, 24.0)), None)
    rows, pr = np.ones((2, D.BINS), np.float32), np.full(D.BINS, 7.0, np.float32)
    for count in (0, -1, 8193):
        assert lib.mx_noise_print_rows(rows.ctypes.data, count, pr.ctypes.data) == INVALID
    assert lib.mx_noise_print_rows(None, 1, pr.ctypes.data) == INVALID and lib.mx_noise_print_rows(rows.ctypes.data, 1, None) == INVALID
    assert np.all(pr == 7.0)
    f32 = np.full(8, 7.0, np.float32)
    for k, v in ((0, -1e-30), (512, float("nan")), (100, float("inf")), (511, -float("inf"))):
        bad = ok.copy()
        bad[k] = v
        assert emu.raw.emu_denoise_refuses(None, bad.ctypes.data) == 2, (k, v)
    # null handles are refused before anything else is looked at
    p = C.byref(DP(12.0, 6.0))
    made = C.c_void_p(0x5A5A)
    assert lib.mx_denoise(None, None, ok.ctypes.data, p, 0, 8, f32.ctypes.data, None) == INVALID
    assert lib.mx_denoise_dev(None, None, ok.ctypes.data, p, 0, 8, f32.ctypes.data, None) == INVALID
    assert lib.mx_noise_print(None, None, 0, 2048, pr.ctypes.data) == INVALID and lib.mx_noise_print_dev(None, None, 0, 2048, pr.ctypes.data) == INVALID
    assert lib.mx_noise_rows_dev(None, None, 0, 1, pr.ctypes.data) == INVALID
    assert lib.mx_audio_denoise(None, None, ok.ctypes.data, p, C.byref(made)) == INVALID and made.value == 0x5A5A
    assert np.all(f32 == 7.0) and np.all(pr == 7.0)


def test_emulation_and_host_logic_under_sanitizers(tmp_path):
    assert "denoise_emu ok" in emu_build.run_sanitized(tmp_path, "denoise_emu", SOURCES, "DENOISE_EMU_MAIN")


def test_the_kernels_need_no_scratch_and_one_image_of_lds():
    """No scratch, static LDS only — the 8 x 72-point image of the two walkers —, within 256 VGPRs."""
    names, scratch, vgprs, lds = emu_build.resource_usage("denoise_kernels.hip")
    print(names, scratch, vgprs, lds)
    assert len(names) == 3 and [k for k in ("denoise_kernel", "noise_rows_kernel", "noise_print_kernel") if any(k in n for n in names)] == \
        ["denoise_kernel", "noise_rows_kernel", "noise_print_kernel"]
    assert scratch == [0, 0, 0] and max(vgprs) <= 256
    assert sorted(lds) == [0, 8 * 72 * 8, 8 * 72 * 8]


# MEASURED by the reference (tests/denoise_ref.py, this file's takes, the library's two factors), dB of the RMS over the noise-only
# stretch [2000, 10000) and over the vowel [14000, 46000): {noise level: {setting: (noise, vowel)}}
KNOWN = {1e-2: {(12.0, 6.0): (-11.96, -0.12), (24.0, 6.0): (-23.05, -0.12), (48.0, 12.0): (-48.00, -0.35)},
         1e-3: {(12.0, 6.0): (-11.96, -0.002), (24.0, 6.0): (-23.05, -0.002), (48.0, 12.0): (-48.00, -0.006)}}


def stretch_db(x, y):
    return D.db(D.rms(y[2000:10000]) / D.rms(x[2000:10000])), D.db(D.rms(y[14000:46000]) / D.rms(x[14000:46000]))


@pytest.mark.parametrize("level", (1e-2, 1e-3))
def test_known_answers(emu, factors, vowel, level):
    """At sensitivity 6 dB the noise-only stretch falls by the asked reduction (12 and 24 dB; 48 dB at sensitivity 12) and the
    vowel's RMS stays put: +-0.5 dB around the reference's recorded figure for the noise, 0.1 dB for the vowel (the margin is for
    the takes' seeds)."""
    x, P, refs = vowel[level]
    for s in D.SETTINGS:
        ref = refs[s] if s in refs else D.denoise(x, P, *factors[s])
        got = emu.run(x, P, *factors[s])
        rn, rv = stretch_db(x, ref)
        gn, gv = stretch_db(x, got)
        print(f"noise {level}, {s}: the reference {rn:.2f} dB / {rv:.3f} dB, the emulation {gn:.2f} dB / {gv:.3f} dB")
        kn, kv = KNOWN[level][s]
        assert abs(rn - kn) <= 0.5 and abs(rv - kv) <= 0.1, "the recorded figures are the reference's"
        assert abs(gn - kn) <= 0.5 and abs(gv - kv) <= 0.1
