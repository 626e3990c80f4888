"""melonix::SibilantTrack (the C++ facade of the sibilant detector, the protected formant curve and the sibilant balance) from
a compiled program: the C-ABI's records, curve and samples, byte for byte; empty results after every failed call."""
import subprocess

import numpy as np
import pytest

import sibilant_ref as S
from facade_build import build_driver

pytestmark = pytest.mark.gpu

SR, HOP = S.SR, S.HOP


def test_sibilant_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "sibilant_driver")
    w = S.take()[0]
    n, ramp, db = len(w), 480, -6.0
    src, ft, sb, cv, bl = (tmp_path / k for k in ("in.f32", "features.bin", "sibilants.bin", "curve.bin", "balanced.f32"))
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(SR), str(db), str(ramp), str(ft), str(sb), str(cv), str(bl)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    a = gpu_ctx.upload(w)
    try:
        feat = gpu_ctx.sib_features(a, SR, HOP)
        sibs = gpu_ctx.sibilants_detect(a, SR, HOP)
        prot = mxlib.formant_protect([(0, 4.0), (n // 2, 2.0), (n - 1, -3.0)], sibs, ramp, n)
        b = gpu_ctx.audio_gain(a, mxlib.sibilant_gain_points(sibs, db, ramp, n))
        try:
            balanced = gpu_ctx.audio_download(b)
        finally:
            b.free()
    finally:
        a.free()
    assert ft.read_bytes() == feat.tobytes() and sb.read_bytes() == sibs.tobytes() and len(sibs) == 3
    assert cv.read_bytes() == prot.tobytes() and len(prot) == 2 + 4 * 3  # (the curve's middle point lies on the "sh": dropped)
    assert bl.read_bytes() == balanced.tobytes() and balanced.tobytes() != w.tobytes()
    assert f"{len(feat)} frames, 3 sibilants, {len(prot)} curve points" in r.stdout
