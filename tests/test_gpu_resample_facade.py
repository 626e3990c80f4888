"""melonix::Mastering's export at another sample rate (finishAt, exportWavAt) from a compiled program: finishAt() equals the Python
chain's int16 byte for byte — the gain from the measurement at the take's own rate, the conversion, then the limiter with its
defaults at the output rate —, the WAV it writes carries the output rate and mx_resample_length samples, and finishAt() at the
take's own rate is finish() (the driver checks that, and the empty results of a refused rate pair, and says so by its status)."""
import subprocess

import numpy as np
import pytest

import loudness_ref as L
from facade_build import build_driver

pytestmark = pytest.mark.gpu


def test_mastering_facade_exports_at_another_rate(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "resample_driver")
    sr, out_rate, target, ceiling = L.LEVEL_SR, 44100, -12.0, -1.0
    w = L.levelling_take()[0]
    w = (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)
    a = gpu_ctx.upload(w)
    made = []
    try:
        summary = gpu_ctx.loudness_measure(a, sr)
        tp, _ = gpu_ctx.true_peak(a, sr)
        made.append(gpu_ctx.audio_gain(a, [(0, mxlib.normalize_gain_tp(summary, tp, target, 200.0))]))
        made.append(gpu_ctx.resample(made[0], sr, out_rate))
        b, pcm = gpu_ctx.limit(made[1], out_rate, ceiling_db=ceiling, pcm16=True)
        made.append(b)
        converted = gpu_ctx.audio_download(made[1])
    finally:
        for b in made:
            b.free()
        a.free()
    m = mxlib.resample_length(len(w), sr, out_rate)
    src, pc, wv = (tmp_path / k for k in ("in.f32", "pcm.i16", "out.wav"))
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(sr), str(out_rate), str(target), str(ceiling), str(pc), str(wv)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert len(pcm) == m and pc.read_bytes() == pcm.tobytes() and np.abs(pcm.astype(np.int32)).max() <= 32767 * 10 ** (ceiling / 20)
    assert np.abs(converted).max() > 1.0  # (the limiter had work to do at the output rate)
    wav_file = wv.read_bytes()
    assert wav_file[:4] == b"RIFF" and wav_file[8:12] == b"WAVE" and len(wav_file) == 44 + 2 * m
    assert int.from_bytes(wav_file[4:8], "little") == len(wav_file) - 8 and int.from_bytes(wav_file[24:28], "little") == out_rate
    assert int.from_bytes(wav_file[28:32], "little") == 2 * out_rate and int.from_bytes(wav_file[40:44], "little") == 2 * m
    assert wav_file[44:] == pcm.tobytes()
    assert f"{len(w)} samples at {sr} Hz -> {m} at {out_rate} Hz" in r.stdout
