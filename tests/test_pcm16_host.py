"""The two float -> int16 conversions (melonix_amd/csrc/pcm16.h; definition: include/melonix_amd.h "PCM conversions") built for
the host: the reference form against the compiled reference arithmetic (oracle.pcm_to_i16) and the clamped form against its
numpy statement over EVERY binary32 bit pattern; the recorded table; and a program of its own under UBSan with
float-cast-overflow, where a cast of a value that does not fit ends the run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import pcm_extremes as P

CHUNK = 1 << 24  # patterns per call: 64 MiB of floats
PARTS = 16       # test cases the 2^32 patterns are split into


@pytest.fixture(scope="module")
def pcm_emu():
    L = C.CDLL(emu_build.shared_object("pcm16_emu", ["pcm16_emu.cpp"], ["pcm16.h"]))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int16)
    L.emu_pcm16_reference.argtypes = [fp, C.c_long, ip]
    L.emu_pcm16_clamped.argtypes = [fp, C.c_long, ip]
    L.emu_pcm16_patterns.argtypes = [C.c_uint32, C.c_long, fp, ip, ip]
    return L


def _convert(fn, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty(len(v), np.int16)
    fn(v.ctypes.data_as(C.POINTER(C.c_float)), len(v), out.ctypes.data_as(C.POINTER(C.c_int16)))
    return out


def test_recorded_table(pcm_emu, oracle):
    """The table recorded from the compiled reference: the oracle build still gives it, the header's reference form gives it,
    and so does the numpy statement the GPU tests use where they have no oracle."""
    v = np.array([x for x, _ in P.TABLE], np.float32)
    want = np.array([y for _, y in P.TABLE], np.int16)
    assert np.array_equal(oracle.pcm_to_i16(v), want)
    assert np.array_equal(_convert(pcm_emu.emu_pcm16_reference, v), want)
    assert np.array_equal(P.reference_i16(v), want)
    # the clamped form on the same values: saturation, and 0 for NaN
    c = _convert(pcm_emu.emu_pcm16_clamped, v)
    assert np.array_equal(c, P.clamped_i16(v))
    assert c[v > 1].tolist() == [32767] * int((v > 1).sum()) and c[v < -1].tolist() == [-32767] * int((v < -1).sum())
    assert c[np.isnan(v)].tolist() == [0]


@pytest.mark.parametrize("part", range(PARTS))
def test_every_bit_pattern(pcm_emu, oracle, part):
    """All 2^32 binary32 values, a sixteenth per case: reference form == what the compiled reference arithmetic gives, clamped form
    == its definition.  0 mismatches of either."""
    v = np.empty(CHUNK, np.float32)
    r = np.empty(CHUNK, np.int16)
    c = np.empty(CHUNK, np.int16)
    per = (1 << 32) // PARTS
    wrong_r = wrong_c = 0
    for first in range(part * per, (part + 1) * per, CHUNK):
        pcm_emu.emu_pcm16_patterns(first, CHUNK, v.ctypes.data_as(C.POINTER(C.c_float)), r.ctypes.data_as(C.POINTER(C.c_int16)),
                                   c.ctypes.data_as(C.POINTER(C.c_int16)))
        assert v.view(np.uint32)[0] == first and v.view(np.uint32)[-1] == first + CHUNK - 1
        wrong_r += int((r != oracle.pcm_to_i16(v)).sum())
        wrong_c += int((c != P.clamped_i16(v)).sum())
    print(f"patterns [{part * per:#x}, {(part + 1) * per:#x}): {wrong_r} reference-form and {wrong_c} clamped-form mismatches")
    assert wrong_r == 0 and wrong_c == 0


def test_numpy_statements_at_the_edges(oracle):
    """pcm_extremes.reference_i16 (what a test without the oracle compares with) == the oracle at the planted values and around
    every threshold."""
    edges = np.array([1.0, 65536.0, 65538.0, 2147483648.0 / 32767.0, 3.4028234663852886e38, 1.1754943508222875e-38], np.float32)
    v = [P.PLANTED]
    for e in edges:
        x = np.array([e], np.float32)
        for _ in range(3):
            v.append(x.copy()), v.append(-x)
            with np.errstate(over="ignore"):
                x = np.nextafter(x, np.float32(np.inf))
        x = np.array([e], np.float32)
        for _ in range(3):
            x = np.nextafter(x, np.float32(0))
            v.append(x.copy()), v.append(-x)
    v = np.concatenate(v + [np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)])
    assert np.array_equal(P.reference_i16(v), oracle.pcm_to_i16(v))


def test_extremes_program_under_ubsan(tmp_path):
    """tests/cpp/pcm16_extremes.cpp with -fsanitize=undefined,float-cast-overflow, no recovery: both forms on the table, the
    neighbours of every threshold, FLT_MAX, subnormals, -0, +-Inf and NaNs.  Exit status 0: nothing undefined ran, every value
    is the defined one."""
    src = os.path.join(emu_build.ROOT, "tests", "cpp", "pcm16_extremes.cpp")
    exe = str(tmp_path / "pcm16_extremes")
    for opt in ("-O0", "-O2"):
        subprocess.check_call(["g++", "-std=c++17", opt, "-g", "-Wall", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow",
                               "-fno-sanitize-recover=all", src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and " 0 wrong" in out.stdout, out.stdout + out.stderr[-3000:]


def test_resynth_arms_cover_every_planted_value():
    """The hand-made schedule tests/test_gpu_pcm_extremes.py runs on the device: in the scalar head, the packed body, the scalar tail and the long-grain loop alike every planted
    value comes out as itself (Inf included, next to NaNs of 0 * Inf), values past 65538 of both signs among them."""
    from melonix_amd import STEP_DTYPE
    w, plateaus = P.arms_audio()
    st, total = P.arms_schedule(STEP_DTYPE, plateaus)
    want, arm = P.arms_expected(w, st, total)
    finite = set(P.PLANTED[~np.isnan(P.PLANTED)].tolist())
    for a in range(4):
        here = want[arm == a]
        assert finite <= set(here[~np.isnan(here)].tolist()), a
        assert np.isnan(here).any() and (here > 65538).any() and (here < -65538).any()
    assert (st["out_offset"] & 7 != 0).any() and (st["sz"] & 7 != 0).any()
    assert not want[arm == 4].any() and (arm == 4).sum() == P.ARMS_TAIL
