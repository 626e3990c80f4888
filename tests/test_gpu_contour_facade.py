"""melonix::PitchContour (the C++ facade of the pitch-drift and vibrato controls) from a compiled program: the C-ABI's track,
notes, contour records, statistics, vibrato figures, bend curve and corrected PCM, byte for byte; empty results after every
failed call."""
import subprocess

import numpy as np
import pytest

from facade_build import build_driver
from test_gpu_contour_render import HOP, SR, vowel

pytestmark = pytest.mark.gpu

VOICING = 0.3  # what the facade reads a decoded track with: 2 x the tracker's threshold


def test_contour_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "contour_driver")
    w = vowel(1.0)
    names = ("in.f32", "track.bin", "notes.bin", "rec.bin", "stat.bin", "vibrato.bin", "bend.bin", "pcm.f32")
    src, tr, nt, rc, st, vb, bd, pc = (tmp_path / k for k in names)
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(SR), "1", "0.25"] + [str(p) for p in (tr, nt, rc, st, vb, bd, pc)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    a = gpu_ctx.upload(w)
    try:
        track = gpu_ctx.f0_track_decoded(a, SR, HOP)
        notes = mxlib.detect_notes(track, SR, HOP, threshold=VOICING)
        rec, stat = gpu_ctx.pitch_contour(track, SR, HOP, notes, threshold=VOICING)
        shift = np.rint(notes["note"]) - notes["note"]
        bend = mxlib.contour_bend(rec, notes, mxlib.contour_spans(notes), shift, drift_amount=1.0, vibrato_scale=0.25)
        pcm, _ = gpu_ctx.psola_render_bend(a, SR, HOP, track, [], bend, want_i16=False, threshold=VOICING)
    finally:
        a.free()
    assert len(notes) >= 1 and tr.read_bytes() == track.tobytes() and rc.read_bytes() == rec.tobytes() and st.read_bytes() == stat.tobytes()
    got_notes = np.fromfile(nt, dtype=mxlib.NOTE_DTYPE)
    assert len(got_notes) == len(notes) and all((got_notes[k] == notes[k]).all() for k in notes.dtype.names)
    want_vib = np.array([list(mxlib.contour_vibrato(s, int(n["frames"]), SR, HOP).values()) for s, n in zip(stat, notes)])
    assert vb.read_bytes() == want_vib.tobytes() and want_vib[0][1] > 25.0  # (extent_cents of the 40-cent vibrato)
    assert bd.read_bytes() == bend.tobytes() and np.abs(bend).max() > 0.2
    assert pc.read_bytes() == pcm.tobytes() and np.abs(pcm).max() > 0.1
    assert f"{len(track)} frames, {len(notes)} notes" in r.stdout
