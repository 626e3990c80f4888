"""melonix::OnsetTrack::tempo / tempoWindows (the C++ facade of the tempo estimate) from a compiled program: the C-ABI's
estimate and window curve, byte for byte."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import tempo_ref as T
from facade_build import build_driver

pytestmark = pytest.mark.gpu

SR, HOP = T.SR, T.HOP


def test_tempo_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path):
    from melonix_amd import _capi

    exe = build_driver(tmp_path, "tempo_driver")
    w = T.take_wave("bpm120_exact")
    src, tb, wb = (tmp_path / k for k in ("in.f32", "tempo.bin", "windows.bin"))
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(SR), str(tb), str(wb)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    a = gpu_ctx.upload(w)
    try:
        res, win = gpu_ctx.tempo_detect(a, SR, HOP, want_windows=True)
    finally:
        a.free()
    theirs = _capi.Tempo.from_buffer_copy(tb.read_bytes()[:C.sizeof(_capi.Tempo)])
    assert {k: getattr(theirs, k) for k, _ in _capi.Tempo._fields_} == res  # (field by field: the record ends in padding)
    assert wb.read_bytes() == win.tobytes() and len(win) > 0
    assert abs(res["bpm"] - 120.0) < 0.1 and f"{len(win)} windows, {res['levels']} levels" in r.stdout
    assert np.isfinite(res["offset"]) and 0.0 <= res["offset"] < 60.0 / res["bpm"]
