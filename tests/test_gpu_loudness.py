"""The loudness records on the GPU (include/melonix_amd.h "Loudness and note levelling"): byte for byte tests/loudness_ref.py's
at the smallest shapes that can go wrong, whatever the launch split; nothing written beyond the records asked for; silence, the
power-of-two law, exactly the defined steps spoilt by a NaN or an Inf; the refusals; and the levelling chain end to end."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as L
from conftest import DevBuf

pytestmark = pytest.mark.gpu

GUARD = 4  # records of 0xA5 either side of what a launch may write


def shapes():
    """name -> (sr, n): three groups and an odd rest at 48 kHz; 70 groups + 17 samples at 44.1 kHz (odd S, group starts that are
    no multiple of 4, more groups than a wavefront); short takes at 8 kHz and at 384 kHz (W = the whole left pad)."""
    return {"48k": (48000, 3 * 10 * 480 + 1234), "441": (44100, 70 * 10 * 441 + 17), "8k": (8000, 25 * 10 * 80 + 3),
            "384k": (384000, 2 * 10 * 3840 + 777)}


@pytest.fixture(scope="module")
def cases(mxlib):
    """name -> (sr, samples, the library's coefficients, reference records): computed once, read by every test."""
    out = {}
    for name, (sr, n) in shapes().items():
        w = L.noise(n, seed=n)
        k = mxlib.loudness_coeffs(sr)
        ref = L.steps(w, sr, k)
        ref.setflags(write=False)
        out[name] = (sr, w, k, ref)
    return out


def dev_records(ctx, audio, sr, first_group, ngroups, count):
    """The device form into a 0xA5 buffer with GUARD records either side -> the `count` records; the guards must stand."""
    buf = DevBuf((count + 2 * GUARD) * 16, fill=0xA5)
    try:
        ctx.loudness_steps_dev(audio, sr, first_group, ngroups, buf.ptr + GUARD * 16)
        ctx.synchronize()
        raw = buf.read(np.uint8)
    finally:
        buf.free()
    assert np.all(raw[:GUARD * 16] == 0xA5) and np.all(raw[(GUARD + count) * 16:] == 0xA5), (first_group, ngroups)
    return np.frombuffer(raw[GUARD * 16:(GUARD + count) * 16].tobytes(), dtype=L.STEP_DTYPE)


@pytest.mark.parametrize("name", sorted(shapes()))
def test_records_are_the_references_bytes(mxlib, gpu_ctx, cases, name):
    sr, w, k, ref = cases[name]
    assert len(ref) == mxlib.loudness_step_count(len(w), sr)
    a = gpu_ctx.upload(w)
    try:
        groups = -(-len(ref) // L.G)
        dev = dev_records(gpu_ctx, a, sr, 0, groups, len(ref))
        host = gpu_ctx.loudness_steps(a, sr)
    finally:
        a.free()
    assert dev.tobytes() == ref.tobytes()
    assert host.tobytes() == dev.tobytes() and host.dtype == mxlib.LOUD_STEP_DTYPE
    assert ref["samples"][-1] == len(w) - (len(ref) - 1) * L.geometry(0, sr)[0]


@pytest.mark.parametrize("n", [1, 479, 480, 481, 4800, 4801])
def test_smallest_lengths(mxlib, gpu_ctx, n):
    sr = 48000
    w = L.noise(n, seed=n)
    ref = L.steps(w, sr, mxlib.loudness_coeffs(sr))
    a = gpu_ctx.upload(w)
    try:
        dev = dev_records(gpu_ctx, a, sr, 0, -(-len(ref) // L.G), len(ref))
    finally:
        a.free()
    assert len(ref) == -(-n // 480) and dev.tobytes() == ref.tobytes()


def test_same_bytes_whatever_the_split(gpu_ctx, cases):
    """Groups [0, 37) + [37, end) — the second range ends in the partial last group —, single groups, the host form of a range."""
    sr, w, k, ref = cases["441"]
    groups = -(-len(ref) // L.G)
    assert groups == 71 and len(ref) == 701
    a = gpu_ctx.upload(w)
    try:
        head = dev_records(gpu_ctx, a, sr, 0, 37, 370)
        tail = dev_records(gpu_ctx, a, sr, 37, groups - 37, len(ref) - 370)
        assert head.tobytes() + tail.tobytes() == ref.tobytes()
        for g in (0, 1, 41, 69):
            assert dev_records(gpu_ctx, a, sr, g, 1, 10).tobytes() == ref[10 * g:10 * g + 10].tobytes(), g
        assert dev_records(gpu_ctx, a, sr, 70, 1, 1).tobytes() == ref[700:].tobytes()
        assert gpu_ctx.loudness_steps(a, sr, 63, 8).tobytes() == ref[630:].tobytes()
        assert len(gpu_ctx.loudness_steps(a, sr, 5, 0)) == 0 and len(gpu_ctx.loudness_steps(a, sr, groups, 0)) == 0
    finally:
        a.free()


def test_silence_gives_exact_zeros(gpu_ctx):
    sr, n = 44100, 12 * 4410 + 5
    for w in (np.zeros(n, np.float32), np.full(n, -0.0, np.float32)):
        a = gpu_ctx.upload(w)
        try:
            st = gpu_ctx.loudness_steps(a, sr)
        finally:
            a.free()
        assert st["energy"].tobytes() == np.zeros(len(st)).tobytes()  # +0.0, not -0.0
        assert st["peak"].tobytes() == np.zeros(len(st), np.float32).tobytes() and st["samples"].sum() == n


def test_the_power_of_two_law(gpu_ctx, cases):
    """2^k x gives 4^k energy and 2^k peak, bit for bit, for k = +-20 (the noise take's samples stay normal binary32 numbers)."""
    sr, w, k, ref = cases["48k"]
    for p in (20, -20):
        scaled = w * np.float32(2.0 ** p)
        assert np.array_equal(scaled.astype(np.float64), w.astype(np.float64) * 2.0 ** p)  # exact in binary32
        a = gpu_ctx.upload(scaled)
        try:
            st = gpu_ctx.loudness_steps(a, sr)
        finally:
            a.free()
        assert st["energy"].tobytes() == (ref["energy"] * 4.0 ** p).tobytes(), p
        assert st["peak"].tobytes() == (ref["peak"] * np.float32(2.0 ** p)).tobytes() and np.array_equal(st["samples"], ref["samples"])


def affected_steps(p, n, sr):
    """The definition's set: the groups with g G S - W <= p < min((g + 1) G S, n), there the steps whose last sample is >= p."""
    S, W, nsteps, groups = L.geometry(n, sr)
    hit = set()
    for g in range(groups):
        if g * L.G * S - W <= p < min((g + 1) * L.G * S, n):
            for b in range(L.G * g, min(L.G * (g + 1), nsteps)):
                if min((b + 1) * S, n) - 1 >= p:
                    hit.add(b)
    return hit


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_bad_sample_spoils_exactly_the_defined_steps(gpu_ctx, cases, value):
    """Positions: late in a group, inside the next group's warm-up; in the first step of a group, outside every other group's
    warm-up; the last sample of the take."""
    sr, w, k, ref = cases["8k"]
    n, S, W = len(w), 80, 684
    late, early, last = 7 * 800 + 500, 11 * 800 + 3, n - 1
    assert late >= 8 * 800 - W and early < 12 * 800 - W
    assert affected_steps(late, n, sr) == set(range(76, 90)) and affected_steps(early, n, sr) == set(range(110, 120))
    assert affected_steps(last, n, sr) == {len(ref) - 1}
    for p in (late, early, last):
        x = w.copy()
        x[p] = value
        a = gpu_ctx.upload(x)
        try:
            st = gpu_ctx.loudness_steps(a, sr)
        finally:
            a.free()
        hit = np.zeros(len(ref), dtype=bool)
        hit[sorted(affected_steps(p, n, sr))] = True
        assert np.array_equal(~np.isfinite(st["energy"]), hit), (p, np.flatnonzero(~np.isfinite(st["energy"])))
        assert np.all(np.isnan(st["energy"][hit]) | (st["energy"][hit] == np.inf))
        assert st[~hit].tobytes() == ref[~hit].tobytes()
        own = p // S  # the bad sample's own step: its peak is over the samples that are not NaN, Inf counts
        clean = np.abs(np.delete(x[own * S:min((own + 1) * S, n)], p - own * S)).max(initial=0.0)
        assert st["peak"][own] == (clean if np.isnan(value) else np.inf)
        others = hit.copy()
        others[own] = False
        assert st["peak"][others].tobytes() == ref["peak"][others].tobytes() and np.array_equal(st["samples"], ref["samples"])


def test_bad_arguments_are_refused_before_any_launch(mxlib, gpu_ctx, cases):
    sr, w, k, ref = cases["48k"]
    lib, INVALID = mxlib._capi.lib(), mxlib._capi.MX_ERR_INVALID
    groups = -(-len(ref) // L.G)
    a = gpu_ctx.upload(w)
    buf = DevBuf((len(ref) + 2) * 16, fill=0xA5)
    host = np.full((len(ref) + 2) * 16, 0xA5, dtype=np.uint8)
    try:
        for rate, first, count in ((7999, 0, 1), (384001, 0, 1), (0, 0, 1), (sr, -1, 1), (sr, 0, -1), (sr, 0, groups + 1), (sr, groups, 1),
                                   (sr, groups + 1, 0), (sr, 2, groups - 1), (sr, 1, 2 ** 62)):
            for name, out in (("mx_loudness_steps_dev", buf.ptr), ("mx_loudness_steps", host.ctypes.data)):
                assert getattr(lib, name)(gpu_ctx.handle, a.handle, rate, first, count, C.c_void_p(out)) == INVALID, (name, rate, first, count)
        for name, out in (("mx_loudness_steps_dev", buf.ptr), ("mx_loudness_steps", host.ctypes.data)):
            assert getattr(lib, name)(None, a.handle, sr, 0, 1, C.c_void_p(out)) == INVALID
            assert getattr(lib, name)(gpu_ctx.handle, None, sr, 0, 1, C.c_void_p(out)) == INVALID
            assert getattr(lib, name)(gpu_ctx.handle, a.handle, sr, 0, 1, None) == INVALID
        assert lib.mx_loudness_steps_dev(gpu_ctx.handle, a.handle, sr, 0, 1, C.c_void_p(buf.ptr + 8)) == INVALID  # not 16-byte aligned
        assert b"aligned" in lib.mx_last_error()
        m = mxlib._capi.Loudness(integrated=7.0)
        assert lib.mx_loudness_measure(gpu_ctx.handle, a.handle, 7999, C.byref(m)) == INVALID
        assert lib.mx_loudness_measure(gpu_ctx.handle, None, sr, C.byref(m)) == INVALID and lib.mx_loudness_measure(None, a.handle, sr, C.byref(m)) == INVALID
        assert lib.mx_loudness_measure(gpu_ctx.handle, a.handle, sr, None) == INVALID and m.integrated == 7.0
        gpu_ctx.synchronize()
        assert np.all(buf.read(np.uint8) == 0xA5) and np.all(host == 0xA5)
        with pytest.raises(mxlib.MxError):
            gpu_ctx.loudness_steps(a, sr, 0, groups + 1)
        assert gpu_ctx.loudness_steps(a, sr, 0, 1).tobytes() == ref[:10].tobytes()  # the context works on
    finally:
        buf.free()
        a.free()


def test_the_whole_take_in_one_call(mxlib, gpu_ctx):
    sr = 48000
    w = L.gated_take(sr)[sr:7 * sr]
    a = gpu_ctx.upload(w)
    try:
        got = gpu_ctx.loudness_measure(a, sr)
        st = gpu_ctx.loudness_steps(a, sr)
    finally:
        a.free()
    assert got == mxlib.loudness_integrated(st, sr)
    ref = L.integrated(np.frombuffer(st.tobytes(), dtype=L.STEP_DTYPE), sr)
    assert all(got[key] == ref[key] for key in ("blocks", "passed_abs", "passed_rel", "bad_blocks")) and got["passed_rel"] < got["passed_abs"]
    assert abs(got["integrated"] - ref["integrated"]) <= 1e-9 and np.float32(got["peak"]) == np.float32(L.dbfs(-20.0))
    amp = gpu_ctx.normalize_gain(got, -14.0, -1.0)
    assert np.float32(amp).tobytes() == L.normalize_gain(ref, -14.0, -1.0).tobytes()


def test_levelling_end_to_end(mxlib, gpu_ctx):
    """track -> notes -> note_loudness -> level_gain_points -> audio_gain -> re-measure, on the levelling take (five vowels at
    0.5 / 0.06 / 0.25 / 0.12 / 0.5).  The GPU chain equals the reference chain (tests/loudness_ref.py level_chain on the same
    notes): the records before and after and the gained audio by bytes.  The spread (max - min) of the notes' loudness after
    levelling is at most twice what the REFERENCE chain leaves; the factor two is there because filter memory across the gain
    ramps is the only residue.  Measured on the CPU with the reference alone, notes from tests/yin_ref.py's tracker (they end
    in the silence behind each vowel, so every ramp lies in silence and what is left is the binary32 rounding of the gained
    samples): spread before 17.937 LU, after 3.6e-7 LU."""
    sr, hop = L.LEVEL_SR, 256
    w, truth = L.levelling_take()
    k = mxlib.loudness_coeffs(sr)
    a = gpu_ctx.upload(w)
    made = []
    try:
        notes = mxlib.detect_notes(gpu_ctx.f0_track(a, sr, hop), sr, hop)
        assert len(notes) == len(truth)
        for note, (lo, hi) in zip(notes, truth):
            assert lo <= note["start_sample"] < note["end_sample"] < hi + 2048  # (a frame reads 2048 samples back)
        spans = [(int(s), int(e)) for s, e in zip(notes["start_sample"], notes["end_sample"])]
        st = gpu_ctx.loudness_steps(a, sr)
        lufs = mxlib.note_loudness(st, sr, notes)
        points, reference = mxlib.level_gain_points(notes, lufs)
        made.append(gpu_ctx.audio_gain(a, points))
        levelled = gpu_ctx.audio_download(made[-1])
        st_after = gpu_ctx.loudness_steps(made[-1], sr)
        lufs_after = mxlib.note_loudness(st_after, sr, notes)
        chain = L.level_chain(w, sr, k, spans)
        assert st.tobytes() == chain["steps"].tobytes() and st_after.tobytes() == chain["steps_after"].tobytes()
        assert points.tobytes() == np.array(chain["points"], dtype=mxlib.GAIN_POINT_DTYPE).tobytes() and reference == chain["reference"]
        assert levelled.tobytes() == chain["levelled"].tobytes()
        assert np.all(np.abs(lufs - chain["lufs"]) <= 1e-9) and np.all(np.abs(lufs_after - chain["lufs_after"]) <= 1e-9)
        before, after, ref_after = L.spread(lufs), L.spread(lufs_after), L.spread(chain["lufs_after"])
        print(f"note loudness before {np.round(lufs, 3)} after {np.round(lufs_after, 3)}; spread before {before:.4f} LU, after {after:.4f} LU, "
              f"the reference chain leaves {ref_after:.4f} LU")
        assert before > 15.0 and after <= 2.0 * ref_after
        # raise = lower = 0: every point is 1 and the audio comes back byte for byte
        flat, _ = mxlib.level_gain_points(notes, lufs, raise_=0.0, lower=0.0)
        assert np.all(flat["amp"] == 1.0) and np.array_equal(flat["sample"], points["sample"])
        made.append(gpu_ctx.audio_gain(a, flat))
        assert gpu_ctx.audio_download(made[-1]).tobytes() == w.tobytes()
    finally:
        for b in made:
            b.free()
        a.free()
