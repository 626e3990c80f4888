"""Sample-rate conversion without a GPU (include/melonix_amd.h "Sample-rate conversion"): plan, length and refusals against
Python integers; the 64-bit index map of csrc/resample_core.h up to j = 2^40, and the tile's 32-bit map against it; the library's
table against the binary64 formula; the kernel's arithmetic run on the CPU by tests/emu/resample_emu.cpp — output by output, and
tile by tile the way the kernel walks, with every staged index checked — against tests/resample_ref.py, byte for byte; the six laws
of the definition; the binary32 sum against its binary64 self; known answers of the prototype's response and of the converted
signals, measured by the reference; sanitizers; the kernels' resources."""
import ctypes as C
import math

import numpy as np
import pytest

import bad_samples as BAD
import emu_build
import resample_ref as R

LENGTHS = lambda p: (0, 1, 2, p["M"] - 1, p["M"], p["M"] + 1, p["taps"], 10007)  # noqa: E731
REFUSED = ((384000, 44100), (44100, 48001), (7999, 48000), (48000, 7999), (384001, 48000), (48000, 384001), (0, 48000), (48000, -1))


@pytest.fixture(scope="module")
def emu(mxlib):
    lib = C.CDLL(emu_build.shared_object("resample_emu", ["resample_emu.cpp", "resample_logic.cpp"],
                                         ["resample_core.h", "resample_logic.h", "step_core.h"]))
    P = C.POINTER(mxlib._capi.ResamplePlan)
    lib.emu_resample_plan.argtypes = [C.c_int, C.c_int, P]
    lib.emu_resample_length.argtypes, lib.emu_resample_length.restype = [C.c_longlong, P], C.c_longlong
    lib.emu_resample_table.argtypes = [P, C.c_void_p]
    lib.emu_resample_i0.argtypes, lib.emu_resample_i0.restype = [C.c_double], C.c_double
    lib.emu_resample_at.argtypes = [C.c_longlong, P, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.emu_resample_at_offset_agrees.argtypes = [C.c_longlong, C.c_int, P]
    lib.emu_resample_geometry.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.emu_resample.argtypes = [C.c_void_p, C.c_longlong, P, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
    lib.emu_resample_tiled.argtypes, lib.emu_resample_tiled.restype = lib.emu_resample.argtypes, C.c_longlong

    class Emu:
        raw = lib

        @staticmethod
        def plan(p):
            return mxlib._capi.ResamplePlan(**p)

        @staticmethod
        def run(w, p, taps, first=0, count=None, tiled=False):
            """-> the outputs; tiled: the kernel's walk (no index may leave what a workgroup stages)"""
            w = np.ascontiguousarray(w, dtype=np.float32)
            count = R.length(len(w), p) - first if count is None else count
            out = np.zeros(count, dtype=np.float32)
            table = np.ascontiguousarray(taps.T if tiled else taps, dtype=np.float32)  # (tiled: a row per tap index)
            bad = (lib.emu_resample_tiled if tiled else lib.emu_resample)(w.ctypes.data, len(w), C.byref(Emu.plan(p)), table.ctypes.data,
                                                                           first, count, out.ctypes.data)
            assert not tiled or bad == 0, bad
            return out

    return Emu


@pytest.fixture(scope="module")
def tables(mxlib):
    """(in, out) -> (plan, the library's table), each built once"""
    made = {}

    def get(pair):
        if pair not in made:
            t = mxlib.resample_taps(*pair)
            t.setflags(write=False)
            made[pair] = (R.plan(*pair), t)
        return made[pair]

    return get


def test_plan_length_and_refusals(mxlib, emu):
    """The library, the core header and Python integers agree on every ratio of the issue and its reverse; the sizes to expect."""
    want = {(48000, 44100): (147, 160, 70), (44100, 48000): (160, 147, 64), (96000, 48000): (1, 2, 128), (8000, 44100): (441, 80, 64),
            (192000, 44100): (147, 640, 280)}
    pairs = set(R.PAIRS) | {(b, a) for a, b in R.PAIRS} | {(48000, 48000), (8000, 8000), (384000, 384000), (384000, 48000), (8000, 384000)}
    for pair in sorted(pairs):
        p = R.plan(*pair)
        q = mxlib._capi.ResamplePlan(9, 9, 9, 9)
        ok = emu.raw.emu_resample_plan(pair[0], pair[1], C.byref(q)) == 0
        assert ok == (p is not None), pair
        if p is None:
            with pytest.raises(mxlib.MxError):
                mxlib.resample_plan(*pair)
            continue
        assert mxlib.resample_plan(*pair) == p == mxlib._fields(q) and list(mxlib.resample_plan(*pair)) == ["L", "M", "taps", "half"], pair
        if pair in want:
            assert (p["L"], p["M"], p["taps"]) == want[pair]
        for n in (0, 1, 2, 147, 160, 10007, 172800000, 2 ** 40):
            assert mxlib.resample_length(n, *pair) == R.length(n, p) == emu.raw.emu_resample_length(n, C.byref(q)), (pair, n)
        if pair[0] == pair[1]:
            assert p == {"L": 1, "M": 1, "taps": 0, "half": 0} and mxlib.resample_taps(*pair).shape == (1, 0)
    assert R.plan(192000, 8000) is None and R.plan(8000, 192000) == {"L": 24, "M": 1, "taps": 64, "half": 32}
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    for pair in REFUSED:
        assert R.plan(*pair) is None
        q = mxlib._capi.ResamplePlan(9, 9, 9, 9)
        out = np.full(4, 7.0, np.float32)
        assert lib.mx_resample_plan_for(pair[0], pair[1], C.byref(q)) == INVALID and lib.mx_last_error(), pair
        assert lib.mx_resample_length(100, *pair) == INVALID and lib.mx_resample_taps(pair[0], pair[1], out.ctypes.data) == INVALID
        assert mxlib._fields(q) == {"L": 9, "M": 9, "taps": 9, "half": 9} and np.all(out == 7.0)
    assert lib.mx_resample_plan_for(48000, 44100, None) == INVALID and lib.mx_resample_taps(48000, 44100, None) == INVALID
    assert lib.mx_resample_length(-1, 48000, 44100) == INVALID
    assert b"phases" in (lib.mx_resample_length(1, 44100, 48001), lib.mx_last_error())[1]
    assert b"taps" in (lib.mx_resample_length(1, 384000, 44100), lib.mx_last_error())[1]


def test_index_map_in_64_bits(mxlib, emu):
    """(i_j, phi_j) of resample_core.h against Python integers at j up to 2^40 (j M passes 2^32 and, for M = 640, 2^49), and the
    tile's 32-bit map against the 64-bit one at every offset a tile can hold."""
    rng = np.random.default_rng(40)
    for pair in R.PAIRS + ((384000, 48000),):
        p = R.plan(*pair)
        q = emu.plan(p)
        js = [0, 1, p["L"] - 1, p["L"], 2 ** 31 - 1, 2 ** 31, 2 ** 32 // p["M"], 2 ** 32 // p["M"] + 1, 2 ** 32, 2 ** 40 - 1, 2 ** 40]
        js += [int(v) for v in rng.integers(0, 2 ** 40, 200)]
        for j in js:
            i, phase = C.c_longlong(), C.c_int()
            emu.raw.emu_resample_at(j, C.byref(q), C.byref(i), C.byref(phase))
            assert (i.value, phase.value) == R.index_map(j, p), (pair, j)
        for j0 in (0, p["L"] - 1, 2 ** 32 // p["M"] - 5, 2 ** 40 - 2048):
            for o in (0, 1, 255, 256, 1023, 2047):
                assert emu.raw.emu_resample_at_offset_agrees(j0, o, C.byref(q)), (pair, j0, o)


def test_the_table_is_the_formula(mxlib, emu, tables):
    """Within 2^-23 of the binary64 formula at every tap (both round nearly equal binary64 values of magnitude at most about 1);
    the unit rows exact; every row sums to 1 within T ulps of 1; the series of I0 is the reference's.  MEASURED here:
    no tap of the eight tables differs from the formula rounded to binary32."""
    for x in (0.0, 0.5, 3.0, 12.0):
        assert emu.raw.emu_resample_i0(x) == R.bessel_i0(x)
    assert abs(R.bessel_i0(12.0) / float(np.i0(12.0)) - 1.0) <= 1e-12  # (numpy's Chebyshev form: another route to the same number)
    differ = 0
    for pair in R.PAIRS:
        p, t = tables(pair)
        want = R.table64(p)
        assert t.shape == (p["L"], p["taps"]) and t.dtype == np.float32
        assert np.abs(t.astype(np.float64) - want).max() <= 2.0 ** -23, pair
        differ += int((t != want.astype(np.float32)).sum())
        if p["L"] > p["M"]:
            unit = np.zeros(p["taps"], np.float32)
            unit[p["half"] - 1] = 1.0
            assert t[0].tobytes() == unit.tobytes(), pair  # (+0 elsewhere: by bytes)
        assert np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max() <= p["taps"] * 2.0 ** -24, pair
        mine = np.zeros_like(t)
        emu.raw.emu_resample_table(C.byref(emu.plan(p)), mine.ctypes.data)
        assert mine.tobytes() == t.tobytes()
    print("taps that differ from the formula rounded to binary32:", differ)


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_emulation_is_the_reference_byte_for_byte(emu, tables, pair):
    """Both walks of the emulation at every length around the period and the window, on noise with sparse clicks and on the takes
    of bad_samples (a NaN, +Inf, -Inf mid-take and at both ends)."""
    p, t = tables(pair)
    for n in LENGTHS(p):
        takes = [R.take(n, seed=pair[0] + n)]
        if n >= 2:
            takes += [BAD.with_bad(takes[0], s, v) for v in BAD.BAD.values() for s in (0, n // 2, n - 1)]
        for w in takes if n in (p["taps"], 10007) else takes[:1]:
            want = R.resample(w, p, t)
            assert len(want) == R.length(n, p)
            for tiled in (False, True):
                got = emu.run(w, p, t, tiled=tiled)
                assert got.tobytes() == want.tobytes(), (pair, n, tiled, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])


def test_equal_rates_copy_the_bytes(emu):
    p = R.plan(44100, 44100)
    w = BAD.with_bad(R.take(1000, 1), 500, BAD.BAD["nan"])
    w[3] = -0.0
    assert emu.run(w, p, np.zeros((1, 0), np.float32)).tobytes() == w.tobytes() == R.resample(w, p, None).tobytes()
    assert emu.run(w, p, np.zeros((1, 0), np.float32), 10, 5).tobytes() == w[10:15].tobytes()


@pytest.mark.parametrize("pair", ((48000, 44100), (44100, 48000), (8000, 44100), (192000, 44100)), ids=lambda p: f"{p[0]}-{p[1]}")
def test_the_laws_on_the_cpu(emu, tables, pair):
    """Laws 1-6 of the definition on the emulation (the GPU tests repeat them on the device)."""
    R.check_laws(lambda w, first=0, count=None: emu.run(w, *tables(pair), first, count, tiled=True), *tables(pair))


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_binary32_stays_within_the_bound_of_its_binary64_self(tables, pair):
    """|y32 - y64| <= (T + 1) 2^-24 sum_k |h_k| max|x|: the bound of a recursive sum of T rounded products (Higham, Accuracy and
    Stability of Numerical Algorithms, 3.1: gamma_T < (T + 1) u while T^2 u < 1), derived, not measured."""
    p, t = tables(pair)
    w = R.take(10007, seed=7)
    y32, y64 = R.resample(w, p, t).astype(np.float64), R.resample64(w, p, t)
    phi = (np.arange(len(y32), dtype=np.int64) * p["M"]) % p["L"]
    bound = (p["taps"] + 1) * 2.0 ** -24 * np.abs(t.astype(np.float64)).sum(axis=1)[phi] * float(np.abs(w).max())
    print(f"{pair}: worst error {np.abs(y32 - y64).max():.3g}, {float((np.abs(y32 - y64) / bound).max()):.3f} of the bound")
    assert np.all(np.abs(y32 - y64) <= bound)


@pytest.mark.parametrize("pair", ((48000, 44100), (44100, 48000), (96000, 48000), (8000, 44100)), ids=lambda p: f"{p[0]}-{p[1]}")
def test_known_answers_of_the_prototypes_response(tables, pair):
    """With fmin = min(in, out): flat within +-0.01 dB up to 0.44 fmin, -6.02 dB at fmin / 2 (the half-amplitude point of a
    windowed sinc cut at fmin / 2; +-0.01 dB, the passband's own tolerance), below -100 dB from 0.57 fmin up to the prototype's
    Nyquist rate L in / 2.  MEASURED by the reference: flat to 0.4525-0.4528 fmin, -100 dB from 0.5580-0.5583 fmin, nothing above -119 dB behind it."""
    p, t = tables(pair)
    fmin = min(pair)
    hz, mag = R.response_grid(p, t, pair[0])  # from 0 to the prototype's Nyquist rate, L in / 2
    flat, stop = mag[hz <= 0.44 * fmin], mag[hz >= 0.57 * fmin]
    assert len(flat) > 200 and len(stop) > 200 and hz[1] - hz[0] <= fmin / 400.0
    half = R.response(p, t, pair[0], np.array([fmin / 2.0]))[0]
    sweep = np.linspace(0.44 * fmin, 0.57 * fmin, 521)
    r = R.response(p, t, pair[0], sweep)
    print(f"{pair}: passband within {max(abs(R.db(flat.max())), abs(R.db(flat.min()))):.5f} dB, {R.db(half):.4f} dB at fmin / 2, stopband "
          f"{R.db(stop.max()):.2f} dB; flat to {sweep[np.argmax(np.abs(20 * np.log10(r)) > 0.01)] / fmin:.4f} fmin, "
          f"-100 dB from {sweep[np.argmax(r < 1e-5)] / fmin:.4f} fmin")
    assert np.all(np.abs(20.0 * np.log10(flat)) <= 0.01)
    assert abs(R.db(half) - (-6.0206)) <= 0.01
    assert R.db(stop.max()) < -100.0


# MEASURED by the reference (tests/resample_ref.py with the library's table, this file's takes), in dB of the amplitude or the
# peak; the tests allow 3 dB more, for the takes' seeds, not for the code
SINE_DB = {(48000, 44100): -120.20, (44100, 48000): -120.36, (96000, 48000): -125.03, (48000, 96000): -121.95, (8000, 44100): -120.60,
           (192000, 44100): -117.49}
ALIAS_DB, ROUND_TRIP_DB, DC_DEVIATION = -125.39, -118.47, 1.01e-6


def interior(p, m):
    """the outputs whose windows lie inside the file"""
    edge = p["half"] * p["L"] // p["M"] + 2
    return slice(edge, m - edge)


def sine_error_db(pair, p, t):
    n, hz = 6000, 0.2 * min(pair)
    w = (0.5 * np.sin(2.0 * np.pi * hz * np.arange(n) / pair[0])).astype(np.float32)
    y = R.resample(w, p, t).astype(np.float64)
    want = 0.5 * np.sin(2.0 * np.pi * hz * np.arange(len(y)) / pair[1])
    return R.db(np.abs(y - want)[interior(p, len(y))].max() / 0.5)


@pytest.mark.parametrize("pair", sorted(SINE_DB), ids=lambda p: f"{p[0]}-{p[1]}")
def test_known_answer_a_sine_stays_a_sine(tables, pair):
    """A sine of amplitude 0.5 at 0.2 fmin against the analytic sine at the output rate: the worst interior error."""
    got = sine_error_db(pair, *tables(pair))
    print(f"{pair}: {got:.2f} dB of the amplitude (recorded {SINE_DB[pair]})")
    assert got <= SINE_DB[pair] + 3.0


def alias_db(t):
    p = R.plan(96000, 44100)
    w = (0.5 * np.sin(2.0 * np.pi * 30000.0 * np.arange(12000) / 96000.0)).astype(np.float32)
    y = R.resample(w, p, t)
    return R.db(float(np.abs(y[interior(p, len(y))]).max()) / 0.5)


def round_trip_db(t_down, t_up):
    n = 48000
    w = R.band_noise(n, 48000, 18000.0).astype(np.float32)
    down = R.resample(w, R.plan(48000, 44100), t_down)
    back = R.resample(down, R.plan(44100, 48000), t_up)[:n]
    return R.db(float(np.abs(back.astype(np.float64) - w)[200:n - 200].max()) / float(np.abs(w).max()))


def dc_deviation(p, t):
    y = R.resample(np.ones(4000, np.float32), p, t).astype(np.float64)
    return float(np.abs(y - 1.0)[interior(p, len(y))].max())


def test_known_answers_alias_round_trip_and_dc(mxlib, tables):
    """A 30 kHz tone taken 96 -> 44.1 kHz leaves its alias below ALIAS_DB; noise band-limited to 18 kHz comes back from
    48 -> 44.1 -> 48 kHz within ROUND_TRIP_DB of its peak; DC passes within DC_DEVIATION (the rows sum to 1 before they are rounded)."""
    alias = alias_db(mxlib.resample_taps(96000, 44100))
    trip = round_trip_db(tables((48000, 44100))[1], tables((44100, 48000))[1])
    dc = max(dc_deviation(*tables(pair)) for pair in R.PAIRS)
    print(f"alias {alias:.2f} dB (recorded {ALIAS_DB}), round trip {trip:.2f} dB (recorded {ROUND_TRIP_DB}), DC deviation {dc:.3g} (recorded {DC_DEVIATION})")
    assert alias <= ALIAS_DB + 3.0 and trip <= ROUND_TRIP_DB + 3.0 and dc <= DC_DEVIATION * math.sqrt(2.0)


def test_emulation_and_table_under_sanitizers(tmp_path):
    out = emu_build.run_sanitized(tmp_path, "resample_emu", ["resample_emu.cpp", "resample_logic.cpp"], "RESAMPLE_EMU_MAIN")
    assert "resample_emu ok" in out


def test_the_kernels_need_no_scratch_and_fit_their_lds(mxlib, emu):
    """No scratch, no static LDS; the dynamic LDS of every launch (the window's quads and, where it is staged, the table) stays
    within 64 KiB, the window within 32 KiB: the geometry of every plan the tests use and of the extremes."""
    names, scratch, vgprs, lds = emu_build.resource_usage("resample_kernels.hip")
    print(names, scratch, vgprs, lds)
    assert len(names) == 2 and all("resample_kernel" in n for n in names) and scratch == [0, 0] and max(vgprs) <= 128 and max(lds) <= 65536
    staged = 0
    for pair in R.PAIRS + ((384000, 48000), (8000, 384000), (8192, 8000), (8000, 8184)):
        p = R.plan(*pair)
        tile, quads, in_lds = C.c_int(), C.c_int(), C.c_int()
        emu.raw.emu_resample_geometry(C.byref(emu.plan(p)), C.byref(tile), C.byref(quads), C.byref(in_lds))
        table = 4 * p["L"] * p["taps"]
        assert 256 <= tile.value <= 2048 and tile.value % 256 == 0 and 16 * quads.value <= 32768, pair
        assert 16 * quads.value + (table if in_lds.value else 0) <= 65536 and bool(in_lds.value) == (table <= 44 * 1024), pair
        assert 4 * quads.value >= (tile.value - 1) * p["M"] // p["L"] + 1 + p["taps"] + 6, pair
        staged += in_lds.value
    assert 0 < staged < 12
