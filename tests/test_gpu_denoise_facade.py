"""melonix::NoiseReduction from a compiled program: learn() + apply() on the vowel take give the C-ABI's bytes — the print of
mx_noise_print, the samples of mx_audio_denoise — and the reference chain's samples (tests/denoise_ref.py: the reference's print,
the reference's reduction) within the project's yardstick; a set print, refused regions, prints and parameters: the driver checks
them and says so by its status."""
import subprocess

import numpy as np
import pytest

import denoise_ref as D
from facade_build import build_driver

pytestmark = pytest.mark.gpu


def test_noise_reduction_facade(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "denoise_driver")
    x = D.vowel_take(1e-2)
    red, sens, begin, end = 24.0, 6.0, 0, 12000
    a = gpu_ctx.upload(x)
    b = None
    try:
        P = gpu_ctx.noise_print(a, begin, end)
        b = gpu_ctx.denoise(a, P, red, sens)
        want = gpu_ctx.audio_download(b)
    finally:
        if b is not None:
            b.free()
        a.free()
    src, pr, out = (tmp_path / k for k in ("in.f32", "print.f32", "out.f32"))
    x.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(D.SR), str(begin), str(end), str(red), str(sens), str(pr), str(out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert pr.read_bytes() == P.tobytes() and out.read_bytes() == want.tobytes()
    assert f"{len(x)} samples at {D.SR} Hz cleaned" in r.stdout
    # the reference chain: its own print, its own reduction
    ref_print = D.noise_print(x, begin, end)
    assert np.abs(P / ref_print - 1.0).max() <= 2e-5
    D.assert_close(want, D.denoise(x, ref_print, *mxlib.denoise_factors(red, sens)), "learn + apply against the reference chain")
