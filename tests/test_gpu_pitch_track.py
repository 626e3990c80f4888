"""melonix::PitchTrack (the C++ facade of the YIN tracker) from a compiled program: its correction markers are the Python
path's, record for record."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SR
from test_gpu_f0 import melody

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mask", [0, 0xFFF & ~(1 << 2)])
def test_pitch_track_facade_matches_python(gpu_ctx, mxlib, tmp_path, mask):
    lib = os.path.join(ROOT, "melonix_amd", "lib")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "melonix_amd", "cpp"), "NO_GL=1"])
    exe = str(tmp_path / "pitch_track_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-DMELONIX_AMD_NO_GL", "-I", os.path.join(ROOT, "melonix_amd", "cpp"), "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pitch_track_driver.cpp"),
                           "-o", exe, "-L", lib, "-lmelonix_facade", "-lmelonix_amd", f"-Wl,-rpath,{lib}", "-lpthread"])
    w, _ = melody()
    src, out = tmp_path / "in.f32", tmp_path / "out.markers"
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(SR), str(mask), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=mxlib.MARKER_DTYPE)
    a = gpu_ctx.upload(w)
    tr = gpu_ctx.f0_track(a, SR, 256)
    a.free()
    ref = mxlib.correction_markers(mxlib.detect_notes(tr, SR, 256), 1.0, mask)
    assert len(got) == 12
    for f in ("sample", "note", "dTime", "pitchBend"):  # (field by field: the 4 padding bytes after `sample` are unspecified)
        assert got[f].tobytes() == ref[f].tobytes(), f
