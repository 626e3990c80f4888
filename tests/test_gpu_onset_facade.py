"""melonix::OnsetTrack (the C++ facade of the onset detector and the timing markers) from a compiled program: the C-ABI's
onsets and markers; and one end-to-end check — a take whose notes are off the grid, its timing markers, a render, and the
onsets of the render where the markers sent them."""
import subprocess

import numpy as np
import pytest

import onset_ref as R
from facade_build import build_driver

pytestmark = pytest.mark.gpu

SR, HOP = R.SR, R.HOP


@pytest.mark.parametrize("with_base", [0, 1])
def test_onset_facade_matches_the_c_abi(gpu_ctx, mxlib, tmp_path, with_base):
    exe = build_driver(tmp_path, "onset_driver")
    w = R.notes(0.005)
    src, fl, on, mk = (tmp_path / k for k in ("in.f32", "flux.f32", "onsets.bin", "markers.bin"))
    w.astype("<f4").tofile(src)
    r = subprocess.run([exe, str(src), str(SR), "100", "3", str(with_base), str(fl), str(on), str(mk)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    a = gpu_ctx.upload(w)
    try:
        flux = gpu_ctx.onset_flux(a, SR, HOP)
        onsets = gpu_ctx.onsets_detect(a, SR, HOP)
    finally:
        a.free()
    base = [(1000, 45.0, 0.0, 1.0), (len(w) - 1000, 45.0, 0.0, 1.0)] if with_base else None
    markers = mxlib.timing_markers(onsets["sample"], len(w), SR, base=base, bpm=100.0, division=3)
    assert np.fromfile(fl, dtype="<f4").tobytes() == flux.tobytes()
    assert on.read_bytes() == onsets.tobytes() and len(onsets) == 6
    theirs = np.fromfile(mk, dtype=mxlib.MARKER_DTYPE)  # (field by field: the record has four bytes of padding)
    assert len(theirs) == len(markers) == 6 + 2 * with_base
    assert all(theirs[k].tobytes() == markers[k].tobytes() for k in ("sample", "note", "dTime", "pitchBend"))
    assert np.any(markers["dTime"] != 0)
    assert f"{len(flux)} frames, 6 onsets, {len(markers)} markers" in r.stdout


def test_notes_rendered_through_their_timing_markers_land_on_the_grid(gpu_ctx, mxlib):
    """The 5 ms notes start 0.7 to 50 ms off a 120 bpm / division 4 grid.  timingMarkers -> a render -> detect again: as many
    onsets as the source has, each within +-4 frames of T_i * sr / hop (one 1024-sample window, plus +-2 frames of detector
    jitter on each side).
    Renderer: mx_psola_render with the GPU's own f0 track.  The choice was made on the CPU: tests/psola_ref.py's render of this
    take through these markers (track: tests/yin_ref.py), detected by tests/onset_ref.py, has its six onsets at frames 47, 141,
    211, 305, 375, 469 against T_i * sr / hop = 46.9, 140.6, 210.9, 304.7, 375.0, 468.8 — within one frame, so the +-4-frame
    condition holds for the definition alone and the phase vocoder was not needed."""
    w = R.notes(0.005)
    n = len(w)
    a = gpu_ctx.upload(w)
    try:
        onsets = gpu_ctx.onsets_detect(a, SR, HOP)
        assert len(onsets) == 6
        markers = mxlib.timing_markers(onsets["sample"], n, SR)
        anchors, T = R.anchor_times(onsets["sample"], SR)
        shifts = [Ti - ai / SR for ai, Ti in zip(anchors, T)]
        assert max(abs(s) for s in shifts) > 0.04  # (the take IS off the grid: the render has something to move)
        g = 60.0 / (120.0 * 4)
        assert all(abs(Ti / g - round(Ti / g)) < 1e-9 for Ti in T)
        mk = [(int(m["sample"]), float(m["note"]), float(m["dTime"]), float(m["pitchBend"])) for m in markers]
        track = gpu_ctx.f0_track(a, SR, HOP)
        f32, _ = gpu_ctx.psola_render(a, SR, HOP, track, mk, want_i16=False)
    finally:
        a.free()
    b = gpu_ctx.upload(f32)
    try:
        again = gpu_ctx.onsets_detect(b, SR, HOP)
    finally:
        b.free()
    got = [int(o["frame"]) for o in again]
    print("onsets of the render:", got, "wanted near", [round(Ti * SR / HOP, 2) for Ti in T])
    assert len(got) == len(onsets)
    for f, Ti in zip(got, T):
        assert abs(f - Ti * SR / HOP) <= 4, (f, Ti * SR / HOP)
