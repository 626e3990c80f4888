"""melonix::Mastering (the C++ facade of the export chain: loudness, true peak and loudness range of a take, the gain to a target
loudness, the look-ahead limiter, the int16 and the WAV file) from a compiled program: finish() equals the Python chain's int16
byte for byte, the WAV it writes holds those samples, the measurements are the C-ABI's; empty results after every failed call,
and after a failed construction ok() is false and the accessors are empty (the driver checks both and says so by its status)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import loudness_ref as L
from facade_build import build_driver

pytestmark = pytest.mark.gpu


def test_mastering_facade_matches_the_python_chain(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "mastering_driver")
    sr, target, ceiling, ms = L.LEVEL_SR, -12.0, -1.0, 2.5
    w = L.levelling_take()[0]
    w = (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)
    a = gpu_ctx.upload(w)
    made = []
    try:
        summary = gpu_ctx.loudness_measure(a, sr)
        lra = mxlib.loudness_range(gpu_ctx.loudness_steps(a, sr), sr)
        peaks = gpu_ctx.true_peak_steps(a, sr)
        tp, sp = gpu_ctx.true_peak(a, sr)
        made.append(gpu_ctx.audio_gain(a, [(0, mxlib.normalize_gain_tp(summary, tp, target, 200.0))]))
        b, pcm = gpu_ctx.limit(made[-1], sr, ceiling_db=ceiling, lookahead=120, pcm16=True)  # 2.5 ms at 48 kHz
        made.append(b)
        gained = gpu_ctx.audio_download(made[0])
    finally:
        for b in made:
            b.free()
        a.free()
    names = ("in.f32", "pcm.i16", "out.wav", "peaks.bin", "summary.bin")
    src, pc, wv, pk, sm = (tmp_path / k for k in names)
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(sr), str(target), str(ceiling), str(ms), str(pc), str(wv), str(pk), str(sm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert pc.read_bytes() == pcm.tobytes() and np.abs(pcm).max() <= 32767 * 10 ** (ceiling / 20)
    assert np.abs(gained).max() > 1.0 and pcm.tobytes() != (np.clip(gained, -1, 1).astype(np.float64) * 32767.0).astype(np.int16).tobytes()
    wav_file = wv.read_bytes()
    assert wav_file[:4] == b"RIFF" and wav_file[8:12] == b"WAVE" and len(wav_file) == 44 + 2 * len(w)
    assert int.from_bytes(wav_file[4:8], "little") == len(wav_file) - 8 and int.from_bytes(wav_file[24:28], "little") == sr
    assert wav_file[44:] == pcm.tobytes()
    assert pk.read_bytes() == peaks.tobytes()
    raw = sm.read_bytes()
    n1, n2 = C.sizeof(mxlib._capi.Loudness), C.sizeof(mxlib._capi.LoudnessRange)
    assert len(raw) == n1 + n2 + 8
    assert mxlib._fields(mxlib._capi.Loudness.from_buffer_copy(raw[:n1])) == summary and summary["blocks"] > 0
    assert mxlib._fields(mxlib._capi.LoudnessRange.from_buffer_copy(raw[n1:n1 + n2])) == lra
    assert raw[n1 + n2:] == np.array([tp, sp], np.float32).tobytes() and tp > sp > 1.4
    assert f"{len(peaks)} steps, integrated {summary['integrated']:.4f} LUFS" in r.stdout
