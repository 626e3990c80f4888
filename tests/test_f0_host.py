"""The YIN tracker's host side (no GPU): notes and correction markers against their Python restatement (tests/yin_ref.py),
marker properties, argument errors, the f64 reference itself, and the kernel's resources / hand-issued LDS reads."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import yin_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000


def _track(notes_per_frame, rng=None, ap=0.05, rms=0.1):
    """F0 records from per-frame notes (None = unvoiced): period from the note law's inverse."""
    mx = pytest.importorskip("melonix_amd")
    t = np.zeros(len(notes_per_frame), dtype=mx.F0_DTYPE)
    for i, m in enumerate(notes_per_frame):
        if m is None:
            t[i] = (0, 0.0, 1.0, 0.0)
        else:
            period = SR / (55.0 * 2 ** ((m - 24) / 12))
            a = ap if rng is None else rng.uniform(0, 0.14)
            t[i] = (int(period), period, a, rms)
    return t


def _same_notes(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (int(g["start_sample"]), int(g["end_sample"]), int(g["first_frame"]), int(g["frames"])) == r[:4]
        assert float(g["note"]) == r[4]
        assert float(g["aperiodicity"]) == r[5] and float(g["spread"]) == r[6]


HAND = {
    "silence": [None] * 40,
    "one_note": [45.3] * 20,
    "glitch": [45.3] * 10 + [57.3] + [45.3] * 10,
    "gap_glitch": [45.3] * 10 + [None] + [45.3] * 10,
    "jump": [45.2] * 12 + [47.2] * 12,
    "glide": list(np.linspace(40.0, 44.0, 60)),
    "exact_min": [50.1] * 8 + [None] + [50.1] * 7,
    "even_median": [50.0, 50.2, 50.1, 50.3, 50.4, 50.2, 50.0, 50.6, 50.2, 50.3],
    "dev_break": [50.0] * 9 + [50.4, 50.8, 51.2] + [51.2] * 9,
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_detect_notes_hand_made(mxlib, name):
    tr = _track(HAND[name])
    for first, hop in ((0, 256), (37, 200)):
        got = mxlib.detect_notes(tr, SR, hop, first)
        _same_notes(got, Y.detect_notes(tr, SR, hop, first))
    if name == "silence":
        assert len(mxlib.detect_notes(tr, SR, 256)) == 0
    if name == "exact_min":
        assert len(mxlib.detect_notes(tr, SR, 256)) == 1  # 8 frames kept, 7 dropped
    if name == "glitch":
        assert len(mxlib.detect_notes(tr, SR, 256)) == 2
    if name == "glide":
        assert len(mxlib.detect_notes(tr, SR, 256)) >= 2  # the median falls behind: a new run


def test_detect_notes_random(mxlib):
    rng = np.random.default_rng(7)
    for trial in range(40):
        F = int(rng.integers(1, 400))
        m, notes = 50.0, []
        for _ in range(F):
            r = rng.uniform()
            if r < 0.08:
                notes.append(None)
            else:
                m += rng.choice([0.0, rng.normal(0, 0.1), rng.normal(0, 2.0)], p=[0.5, 0.45, 0.05])
                notes.append(m)
        tr = _track(notes, rng)
        params = dict(min_frames=int(rng.integers(2, 12)), max_jump=float(rng.uniform(0.1, 1.0)),
                      max_dev=float(rng.uniform(0.2, 1.5)))
        got = mxlib.detect_notes(tr, SR, 256, trial, **params)
        _same_notes(got, Y.detect_notes(tr, SR, 256, trial, **params))


def test_detect_notes_hypothesis(mxlib):
    hyp = pytest.importorskip("hypothesis")
    st = hyp.strategies

    @hyp.settings(max_examples=150, deadline=None)
    @hyp.given(st.lists(st.one_of(st.none(), st.floats(24.0, 84.0)), max_size=120), st.integers(2, 10),
               st.floats(0.05, 2.0), st.floats(0.05, 2.0))
    def run(notes, min_frames, max_jump, max_dev):
        tr = _track(notes)
        got = mxlib.detect_notes(tr, SR, 256, 0, min_frames=min_frames, max_jump=max_jump, max_dev=max_dev)
        _same_notes(got, Y.detect_notes(tr, SR, 256, 0, min_frames=min_frames, max_jump=max_jump, max_dev=max_dev))

    run()


def _notes(mxlib):
    tr = _track([44.7] * 10 + [None] * 3 + [47.5] * 10 + [None] + [50.2] * 9 + [None] * 2 + [51.5] * 12)
    notes = mxlib.detect_notes(tr, SR, 256)
    assert len(notes) == 4
    return notes


@pytest.mark.parametrize("mask", [0, 0b101011010101, 1 << 3, 0xFFF, 0b000010000001])
@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0])
def test_correction_markers(mxlib, mask, strength):
    notes = _notes(mxlib)
    mk = mxlib.correction_markers(notes, strength, mask)
    ref = Y.correction_markers(notes, strength, mask)
    assert [(int(m["sample"]), float(m["note"]), float(m["dTime"]), float(m["pitchBend"])) for m in mk] == ref
    assert (np.diff(mk["sample"]) > 0).all() and (mk["dTime"] == 0).all()
    if strength == 0.0:
        assert (mk["pitchBend"] == 0).all()
    if strength == 1.0:
        tgt = mk["note"] + mk["pitchBend"]
        assert np.allclose(tgt, np.round(tgt), atol=1e-9, rtol=0)
        cls = np.round(tgt).astype(int) % 12
        allowed = mask or 0xFFF
        assert all((allowed >> c) & 1 for c in cls)
        # the nearest allowed: no allowed integer is closer
        for m, t in zip(mk["note"], np.round(tgt)):
            for k in range(int(np.floor(m)) - 12, int(np.floor(m)) + 14):
                if (allowed >> (k % 12)) & 1:
                    assert abs(k - m) >= abs(t - m) - 1e-12


def test_defaults(mxlib):
    p = mxlib.note_params_default()
    assert p["min_frames"] == 8 and p["max_jump"] == 0.5 and p["max_dev"] == 0.75
    assert np.float32(p["threshold"]) == np.float32(0.15) and np.float32(p["rms_floor"]) == np.float32(1e-3)


def test_errors_leave_outputs_untouched(mxlib):
    from melonix_amd import _capi
    L = _capi.lib()
    tr = _track([45.0] * 20)
    p = _capi.NoteParams()
    L.mx_note_params_default(C.byref(p))
    sentinel = C.cast(C.c_void_p(0x1234), C.POINTER(_capi.Note))
    cases = []
    bad = _capi.NoteParams.from_buffer_copy(bytes(p))
    bad.min_frames = 1
    cases.append((tr.ctypes.data, len(tr), SR, 256, 0, bad))
    cases.append((tr.ctypes.data, len(tr), 0, 256, 0, p))
    cases.append((tr.ctypes.data, len(tr), SR, 0, 0, p))
    cases.append((tr.ctypes.data, -1, SR, 256, 0, p))
    cases.append((None, 5, SR, 256, 0, p))
    bad2 = _capi.NoteParams.from_buffer_copy(bytes(p))
    bad2.max_dev = float("nan")
    cases.append((tr.ctypes.data, len(tr), SR, 256, 0, bad2))
    for args in cases:
        out, cnt = C.cast(sentinel, C.POINTER(_capi.Note)), C.c_int64(-77)
        rc = L.mx_detect_notes(args[0], args[1], args[2], args[3], args[4], C.byref(args[5]), C.byref(out), C.byref(cnt))
        assert rc == _capi.MX_ERR_INVALID and L.mx_last_error()
        assert C.cast(out, C.c_void_p).value == 0x1234 and cnt.value == -77
    notes = _notes(mxlib)
    buf = np.full(2 * len(notes) * 32, 0x5A, dtype=np.uint8)
    rev = np.ascontiguousarray(notes[::-1])
    for ns, strength, mask in ((notes, 1.5, 0), (notes, -0.1, 0), (notes, float("nan"), 0), (notes, 1.0, 0x1000),
                               (notes, 1.0, -1), (rev, 1.0, 0)):
        rc = L.mx_correction_markers(ns.ctypes.data, len(ns), strength, mask, buf.ctypes.data)
        assert rc == _capi.MX_ERR_INVALID and L.mx_last_error()
        assert (buf == 0x5A).all()


def test_f0_track_errors_without_touching_outputs(mxlib):
    """Argument checks come before the device: they hold on a machine without a GPU too (null context = invalid)."""
    from melonix_amd import _capi
    L = _capi.lib()
    out = np.full(64, 0x5A, dtype=np.uint8)
    for args in ((None, None, SR, 256, 0, 4, 55.0, 1760.0, 0.15),):
        assert L.mx_f0_track(*args, out.ctypes.data) == _capi.MX_ERR_INVALID
        assert L.mx_f0_track_dev(*args, out.ctypes.data) == _capi.MX_ERR_INVALID
    assert (out == 0x5A).all()


def test_reference_fft_matches_the_literal_sum():
    rng = np.random.default_rng(3)
    i = np.arange(40000)
    w = (0.4 * np.sin(2 * np.pi * 220.0 * i / SR) + 0.2 * np.sin(2 * np.pi * 331.0 * i / SR)
         + 0.05 * rng.standard_normal(len(i))).astype(np.float32)
    for first in (0, 7, 150):  # the first frames straddle the start of the file
        x = Y.frames_of(w, 256, first, 1)
        d = Y.diff_fft(x)[0]
        ref = Y.diff_direct(x[0])
        assert np.abs(d - ref).max() <= 1e-9 * ref.max()
    recs, _ = Y.track(np.zeros(10000, np.float32), SR, count=4)
    assert recs == [Y.SILENT] * 4
    recs, _ = Y.track((0.5 * np.sin(2 * np.pi * 440.0 * i / SR)).astype(np.float32), SR, first=50, count=3)
    for t, period, ap, rms in recs:
        assert abs(1200 * np.log2(SR / period / 440.0)) < 0.5 and ap < 0.01 and abs(rms - 0.5 / np.sqrt(2)) < 1e-3


def _kernel_cmd(extra):
    from melonix_amd import build

    return build.unit_command("f0_kernels.hip") + extra


def test_f0_kernel_is_scratch_free():
    out = subprocess.run(_kernel_cmd(["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", out.stderr)]
    assert any("f0_yin" in n for n in names) and len(names) == len(scratch) == len(vgprs)
    assert not [s for s in scratch if s] and max(vgprs) <= 256


def test_f0_kernel_lds_reads_are_covered_by_their_waits(tmp_path):
    asm = tmp_path / "f0.s"
    out = subprocess.run(_kernel_cmd(["--cuda-device-only", "-S", "-o", str(asm)]), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    aud = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_audit.py"), str(asm)], capture_output=True, text=True)
    assert aud.returncode == 0, aud.stdout[-3000:]
    m = re.fullmatch(r"(\d+) kernel\(s\) audited, 0 finding\(s\)", aud.stdout.splitlines()[-1])
    assert m and int(m.group(1)) >= 1, aud.stdout[-500:]


def test_reference_is_scale_invariant():
    """The scale property the GPU suite pins bit for bit belongs to the definition: 2^k x gives the same tau, period and
    aperiodicity and 2^k times the rms, for every k with 2^k x exact in f32."""
    i = np.arange(6000)
    w = Y.pcm16(0.45 * np.sin(2 * np.pi * 196.0 * i / SR) + 0.1 * np.sin(2 * np.pi * 392.0 * i / SR)
                + 1e-3 * np.random.default_rng(5).uniform(-1, 1, len(i)))
    ks = Y.exact_scales(w)
    assert ks[0] <= -130 and ks[-1] >= 120 and ks == list(range(ks[0], ks[-1] + 1))
    ref, _ = Y.track(w, SR)
    assert all(r[0] > 0 for r in ref)
    for k in ks:
        got, _ = Y.track(np.ldexp(w, k), SR)
        assert [r[0] for r in got] == [r[0] for r in ref], k
        for g, r in zip(got, ref):
            assert g[1] == r[1] and g[2] == r[2] and g[3] == math.ldexp(r[3], k), k
