"""melonix::Resynth::renderPSOLA / exportWavPSOLA over a melonix::PitchTrack (the C++ facade of the PSOLA renderer) from a
compiled program: the Python path's bytes, and the WAV file saveWav makes of them.  On a decoded track the facade's default
threshold is twice the tracker's."""
import subprocess

import numpy as np
import pytest

from conftest import SR
from facade_build import build_driver
from test_gpu_psola import vowel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("decoded", [0, 1])
def test_psola_facade_matches_python(gpu_ctx, mxlib, tmp_path, decoded):
    exe = build_driver(tmp_path, "psola_driver")
    w = vowel(0.75)
    src, out, wav = tmp_path / "in.f32", tmp_path / "out.f32", tmp_path / "out.wav"
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, "plain", str(src), str(SR), "4", str(decoded), str(out), str(wav)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"threshold {0.3 if decoded else 0.15:g}" in r.stdout, r.stdout
    a = gpu_ctx.upload(w)
    try:
        tr = gpu_ctx.f0_track_decoded(a, SR, 256) if decoded else gpu_ctx.f0_track(a, SR, 256)
        mk = [(1, 0, 0.0, 4.0), (len(w) - 1, 0, 0.0, 4.0)]
        f32, i16 = gpu_ctx.psola_render(a, SR, 256, tr, mk, threshold=0.3 if decoded else 0.15)
    finally:
        a.free()
    assert np.fromfile(out, dtype="<f4").tobytes() == f32.tobytes()
    ref_wav = tmp_path / "ref.wav"
    mxlib.save_wav(str(ref_wav), i16, SR)
    assert wav.read_bytes() == ref_wav.read_bytes() and len(i16) > 30000
