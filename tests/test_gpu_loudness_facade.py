"""melonix::LoudnessTrack (the C++ facade of the loudness records, the gated loudness, note levelling and the export gain) from a
compiled program: the C-ABI's records, summary, curves and samples, byte for byte; empty results after every failed call, and
after a failed construction ok() is false and the accessors are empty (the driver checks both and says so by its status)."""
import ctypes as C
import subprocess

import pytest

import loudness_ref as L
from facade_build import build_driver

pytestmark = pytest.mark.gpu


def test_loudness_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "loudness_driver")
    sr, hop, target, ceiling = L.LEVEL_SR, 256, -14.0, -1.0
    w = L.levelling_take()[0]
    a = gpu_ctx.upload(w)
    made = []
    try:
        notes = mxlib.detect_notes(gpu_ctx.f0_track(a, sr, hop), sr, hop)
        steps = gpu_ctx.loudness_steps(a, sr)
        summary = gpu_ctx.loudness_measure(a, sr)
        lufs = mxlib.note_loudness(steps, sr, notes)
        made.append(gpu_ctx.audio_gain(a, mxlib.level_gain_points(notes, lufs)[0]))
        levelled = gpu_ctx.audio_download(made[-1])
        made.append(gpu_ctx.audio_gain(a, [(0, gpu_ctx.normalize_gain(summary, target, ceiling))]))
        normalized = gpu_ctx.audio_download(made[-1])
    finally:
        for b in made:
            b.free()
        a.free()
    names = ("in.f32", "notes.bin", "steps.bin", "summary.bin", "curves.f64", "lufs.f64", "levelled.f32", "normalized.f32")
    src, nt, st, sm, cv, lf, lv, nm = (tmp_path / k for k in names)
    w.astype("<f4").tofile(src)
    notes.tofile(nt)
    r = subprocess.run([exe, str(src), str(sr), str(nt), str(target), str(ceiling), str(st), str(sm), str(cv), str(lf), str(lv), str(nm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert len(notes) == 5 and st.read_bytes() == steps.tobytes()
    assert len(sm.read_bytes()) == C.sizeof(mxlib._capi.Loudness)  # (field by field: the record has four bytes of padding)
    assert mxlib._fields(mxlib._capi.Loudness.from_buffer_copy(sm.read_bytes())) == summary and summary["blocks"] > 0
    assert cv.read_bytes() == mxlib.loudness_curve(steps, sr, 40).tobytes() + mxlib.loudness_curve(steps, sr, 300).tobytes()
    assert lf.read_bytes() == lufs.tobytes()
    assert lv.read_bytes() == levelled.tobytes() and levelled.tobytes() != w.tobytes()
    assert nm.read_bytes() == normalized.tobytes() and normalized.tobytes() != w.tobytes()
    assert f"{len(steps)} steps, 5 notes, integrated {summary['integrated']:.4f} LUFS" in r.stdout
