"""melonix::Compressor and Mastering::finishCompressedAt / exportWavCompressedAt from a compiled program: apply() gives
mx_audio_compress's samples and reductionDb() the dB of mx_compress_gain's curve; the compressed chain — compress, measure the
compressed object again, the gain to the target, the conversion, the limiter, int16 — equals the same chain through the Python
wrappers byte for byte, at the take's rate and at 44.1 kHz, and the reference's compressor (tests/compress_ref.py) stands behind
its first step; finish() and finishAt() give the bytes of the chain without a compressor, as before; refused settings give empty
results (the driver checks them and says so by its status)."""
import subprocess

import numpy as np
import pytest

import compress_ref as R
import loudness_ref as L
from facade_build import build_driver

pytestmark = pytest.mark.gpu

SET = dict(threshold_db=-20.0, ratio=3.0, knee_db=8.0, attack_ms=3.0, release_ms=150.0, lookahead_ms=2.0)
MAKEUP_DB = 4.0


def chain(ctx, mxlib, a, sr, out_rate, target, ceiling, p=None):
    """the export chain through the Python wrappers -> (int16, the loudness of the limited take, the compressed samples | None)"""
    made = []
    try:
        src, samples = a, None
        if p is not None:
            src = ctx.compress(a, sr, **p)
            made.append(src)
            samples = ctx.audio_download(src)
        tp, _ = ctx.true_peak(src, sr)
        made.append(ctx.audio_gain(src, [(0, mxlib.normalize_gain_tp(ctx.loudness_measure(src, sr), tp, target, 200.0))]))
        if out_rate != sr:
            made.append(ctx.resample(made[-1], sr, out_rate))
        b, pcm = ctx.limit(made[-1], out_rate, ceiling_db=ceiling, pcm16=True)
        made.append(b)
        return pcm, ctx.loudness_measure(b, out_rate)["integrated"], samples
    finally:
        for b in made:
            b.free()


def test_compressor_facade_and_the_compressed_chain(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "compress_driver")
    sr, out_rate, target, ceiling = L.LEVEL_SR, 44100, -12.0, -1.0
    w = L.levelling_take()[0]
    w = (w * np.float32(1.5 / np.abs(w).max())).astype(np.float32)
    p = dict(SET, makeup_amp=float(np.float32(10.0 ** (MAKEUP_DB / 20.0))))
    a = gpu_ctx.upload(w)
    try:
        gain = gpu_ctx.compress_gain(a, sr, **p)
        pcm, lufs, samples = chain(gpu_ctx, mxlib, a, sr, sr, target, ceiling, p)
        pcm_at, lufs_at, _ = chain(gpu_ctx, mxlib, a, sr, out_rate, target, ceiling, p)
        plain, lufs_plain, _ = chain(gpu_ctx, mxlib, a, sr, sr, target, ceiling)
        plain_at = chain(gpu_ctx, mxlib, a, sr, out_rate, target, ceiling)[0]
    finally:
        a.free()
    print(f"after the limiter at {target} LUFS under {ceiling} dBTP: {lufs_plain:.2f} LUFS without the compressor, {lufs:.2f} LUFS with "
          f"{SET} and {MAKEUP_DB} dB of make-up ({lufs_at:.2f} at {out_rate} Hz)")
    names = ("in.f32", "out.f32", "red.f32", "chain.i16", "chain-at.i16", "chain.wav", "plain.i16", "plain-at.i16")
    src, out, red, ch, cha, wv, pl, pla = (tmp_path / k for k in names)
    w.astype("<f4").tofile(src)
    args = [str(v) for v in (src, sr, out_rate, target, ceiling, SET["threshold_db"], SET["ratio"], SET["knee_db"], SET["attack_ms"],
                             SET["release_ms"], SET["lookahead_ms"], MAKEUP_DB, out, red, ch, cha, wv, pl, pla)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert out.read_bytes() == samples.tobytes()
    assert red.read_bytes() == (20.0 * np.log10(gain.astype(np.float64) / R.ONE)).astype(np.float32).tobytes() and gain.min() < R.ONE
    assert ch.read_bytes() == pcm.tobytes() and cha.read_bytes() == pcm_at.tobytes()
    wav_file = wv.read_bytes()
    assert wav_file[:4] == b"RIFF" and int.from_bytes(wav_file[24:28], "little") == out_rate and wav_file[44:] == pcm_at.tobytes()
    # the methods without a compressor give the bytes of the chain without one, as before
    assert pl.read_bytes() == plain.tobytes() and pla.read_bytes() == plain_at.tobytes() and plain.tobytes() != pcm.tobytes()
    assert f"{len(w)} samples at {sr} Hz compressed, {len(gain)} steps" in r.stdout
    # the reference's compressor behind the chain's first step
    pr = R.params(**p)
    _, S, y, _ = R.compress(w, mxlib.compress_curve(**pr), mxlib.compress_plan(sr, **pr), pr["makeup_amp"])
    assert samples.tobytes() == y.tobytes() and gain.tobytes() == S[:len(gain)].tobytes()
    # the reason for the feature: the compressed take comes out of the limiter louder than the plain one
    assert lufs > lufs_plain
