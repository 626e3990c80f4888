"""melonix::KeyTrack (the C++ facade of the key, scale and tuning estimate and of the correction markers on the detected grid)
from a compiled program: the C-ABI's records, keys and markers, byte for byte; empty results after every failed call."""
import subprocess

import numpy as np
import pytest

import key_ref as K
from facade_build import build_driver

pytestmark = pytest.mark.gpu

SR = K.SR


def test_key_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "key_driver")
    w = K.takes()["c_major_446"][0]
    notes = np.zeros(len(K.C_MAJOR), dtype=mxlib.NOTE_DTYPE)
    for i, k in enumerate(K.C_MAJOR):  # the take's notes as a tracker would cut them, each a little off the 446 Hz grid
        notes[i] = (12000 * i + 600, 12000 * i + 10800, (12000 * i + 600) // 256, 40, 48 + k + 0.2345 + 0.07 * ((i * 5) % 7 - 3), 0.02, 0.05)
    src, nt, ch, ky, wn, mk = (tmp_path / k for k in ("in.f32", "notes.bin", "chroma.bin", "key.bin", "windows.bin", "markers.bin"))
    w.astype("<f4").tofile(src)
    notes.tofile(nt)
    r = subprocess.run([exe, str(src), str(SR), str(nt), "0.75", str(ch), str(ky), str(wn), str(mk)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    a = gpu_ctx.upload(w)
    try:
        rec = gpu_ctx.chroma(a, SR, 2048)
        key, wins = gpu_ctx.key_detect(a, SR, 2048, window_frames=48, window_hop=24)
    finally:
        a.free()
    markers = mxlib.correction_markers_tuned(notes, 0.75, key["scale_mask"], key["tuning_cents"])
    got_key = np.fromfile(ky, dtype=mxlib.KEY_DTYPE)
    assert ch.read_bytes() == rec.tobytes() and wn.read_bytes() == wins.tobytes() and len(wins) == 6
    assert len(got_key) == 1 and all(got_key[0][k] == v for k, v in key.items()) and (key["tonic"], key["mode"]) == (3, 0)
    got_markers = np.fromfile(mk, dtype=mxlib.MARKER_DTYPE)  # (field for field: a marker has four bytes of padding)
    assert len(got_markers) == len(markers) and all((got_markers[k] == markers[k]).all() for k in markers.dtype.names)
    assert np.abs(markers["pitchBend"]).max() > 0.1
    assert f"{len(rec)} frames, 6 windows, tonic 3 mode 0" in r.stdout
