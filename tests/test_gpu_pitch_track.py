"""melonix::PitchTrack (the C++ facade of the YIN tracker) from a compiled program: its correction markers are the Python
path's, record for record."""
import subprocess

import numpy as np
import pytest

from conftest import SR
from facade_build import build_driver
from test_gpu_f0 import melody

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mask", [0, 0xFFF & ~(1 << 2)])
def test_pitch_track_facade_matches_python(gpu_ctx, mxlib, tmp_path, mask):
    exe = build_driver(tmp_path, "pitch_track_driver")
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
