"""mx_chroma / mx_chroma_sum / mx_key_detect on the GPU against tests/key_ref.py (include/melonix_amd.h "Key, scale and
tuning reference"): the forty columns inside the bound key_ref derives from the arithmetic (behind its guard on the peak
decisions), the same bytes whatever the launch split or the run length, the edges of n and hop, silence and bad samples, the
window sums byte for byte, guard bands, what a bad call may touch, and key, scale and tuning of the synthetic takes end to end."""
import ctypes as C

import numpy as np
import pytest

import key_ref as K
from conftest import DevBuf
from test_key_host import GUARD_SHARE, KEY_FIELDS, TAKES, Case, check_records, same_key

pytestmark = pytest.mark.gpu

SR, HOP = K.SR, 2048
REC = 160


@pytest.fixture(scope="module")
def cases():
    """name -> Case (samples and their reference, computed once, read by every test)."""
    out = {name: Case(w) for name, (w, _, _, _) in K.takes().items()}
    out["chord"] = Case(K.chord())
    out["c_major_44100"] = Case(K.melody(K.C_MAJOR[:8], sr=44100), sr=44100, fmin=200.0, fmax=4000.0)
    out["noise"] = Case(K.noise(seconds=1.0))
    return out


def _extra(case):
    return {k: v for k, v in case.params.items() if v != K.CHROMA_DEFAULTS[k]}


@pytest.fixture(scope="module")
def gpu_rec(gpu_ctx, cases):
    """name -> the GPU's records of the whole signal (host form)."""
    out = {}
    for name, case in cases.items():
        a = gpu_ctx.upload(case.w)
        try:
            out[name] = gpu_ctx.chroma(a, case.sr, case.hop, **_extra(case))
        finally:
            a.free()
    return out


def _dev_rec(ctx, a, sr, hop, first, count, **params):
    """The device form into a buffer with a record of guard band either side -> (records, guard bands untouched)."""
    buf = DevBuf((count + 2) * REC, fill=0xA5)
    try:
        ctx.chroma_dev(a, sr, hop, first, count, buf.ptr + REC, **params)
        ctx.synchronize()
        raw = buf.read(np.uint8)
        clean = raw[:REC].tobytes() == b"\xa5" * REC and raw[REC * (count + 1):].tobytes() == b"\xa5" * REC
        return raw[REC:REC * (count + 1)].view(np.float32).reshape(count, K.COLS).copy(), clean
    finally:
        buf.free()


@pytest.mark.parametrize("name", TAKES + ["chord", "c_major_44100"])
def test_records_against_the_reference(mxlib, cases, gpu_rec, name):
    assert mxlib.chroma_params_default() == K.CHROMA_DEFAULTS
    case, got = cases[name], gpu_rec[name]
    assert got.shape == case.ref.shape
    worst, left_out = check_records(got, case, name)
    print(f"{name}: {len(got)} frames, {left_out} left out by the guard, worst error / bound {worst:.4f}")
    assert left_out <= GUARD_SHARE * len(got), (name, left_out)


def test_same_bytes_whatever_the_split_or_the_run(gpu_ctx, cases, gpu_rec):
    case, whole = cases["c_major"], gpu_rec["c_major"]
    count = len(whole)
    a = gpu_ctx.upload(case.w)
    try:
        dev, clean = _dev_rec(gpu_ctx, a, SR, HOP, 0, count)
        assert clean and dev.tobytes() == whole.tobytes()  # the host form is the device form
        head, c0 = _dev_rec(gpu_ctx, a, SR, HOP, 0, 37)
        tail, c1 = _dev_rec(gpu_ctx, a, SR, HOP, 37, count - 37)
        assert c0 and c1 and np.concatenate([head, tail]).tobytes() == whole.tobytes()  # split at 37: no multiple of any run length
        one, c2 = _dev_rec(gpu_ctx, a, SR, HOP, 5, 1)
        assert c2 and one.tobytes() == whole[5:6].tobytes()
        assert gpu_ctx.chroma(a, SR, HOP, 5, 1).tobytes() == whole[5:6].tobytes()
        try:
            for run in (1, 5, 32):
                gpu_ctx.set_frames_per_block(run)
                assert gpu_ctx.chroma(a, SR, HOP).tobytes() == whole.tobytes(), run
                assert gpu_ctx.chroma(a, SR, HOP, 41, 23).tobytes() == whole[41:64].tobytes(), run
        finally:
            gpu_ctx.set_frames_per_block(0)
    finally:
        a.free()


@pytest.mark.parametrize("n,hop,first,count", [(1, 2048, 0, None), (4095, 2048, 0, None), (4096, 2048, 0, None), (4097, 2048, 0, None),
                                               (300, 1, 0, None), (9000, 1, 4000, 64), (9000, 255, 0, None), (9000, 256, 0, None),
                                               (16384 * 2 + 1, 16384, 0, None), (40000, 16384, 0, None)])
def test_short_inputs_and_hops(gpu_ctx, n, hop, first, count):
    t = np.arange(n)
    w = (0.3 * np.sin(2 * np.pi * 440.0 * t / SR) + 0.2 * np.sin(2 * np.pi * 1567.98 * t / SR) * (t > n // 3)).astype(np.float32)
    case = Case(w, hop=hop, first=first, count=count)
    a = gpu_ctx.upload(w)
    try:
        got = gpu_ctx.chroma(a, SR, hop, first, count)
        assert len(got) == len(case.ref) == (count or -(-n // hop))
        worst, left_out = check_records(got, case, f"n {n} hop {hop}", first)
        print(f"n {n} hop {hop}: {len(got)} frames, {left_out} left out by the guard, worst error / bound {worst:.4f}")
        if n == 9000:
            assert left_out <= GUARD_SHARE * len(got)
        if len(got) > 2:
            assert gpu_ctx.chroma(a, SR, hop, first + len(got) - 2, 2).tobytes() == got[-2:].tobytes()
    finally:
        a.free()


def test_silence_and_bad_samples(gpu_ctx, cases):
    z = np.zeros(20000, dtype=np.float32)
    z[100:300] = -0.0
    a = gpu_ctx.upload(z)
    try:
        got = gpu_ctx.chroma(a, SR, HOP)
        assert len(got) == 10 and got.tobytes() == bytes(REC * 10)
        key, wins = gpu_ctx.key_detect(a, SR, HOP, window_frames=4, window_hop=4)
        assert key["scale_mask"] == 0 and key["clarity"] == 0.0 and key["tuning_cents"] == 0.0 and len(wins) == 3
    finally:
        a.free()
    for bad in (np.inf, -np.inf, np.nan):
        w = cases["chord"].w[:12000].copy()
        w[5000] = bad
        case = Case(w)
        a = gpu_ctx.upload(w)
        try:
            got = gpu_ctx.chroma(a, SR, HOP)
        finally:
            a.free()
        holds = np.array([h * HOP - 2048 <= 5000 < h * HOP + 2048 for h in range(len(got))])
        assert holds.any() and got[holds].tobytes() == bytes(REC * int(holds.sum())) and got[~holds][:, 38].all()  # forty zeros
        check_records(got, case, f"sample {bad}")


def test_noise_is_finite_and_invariant(gpu_ctx, cases, gpu_rec):
    case, whole = cases["noise"], gpu_rec["noise"]
    assert np.isfinite(whole).all() and whole[:, 39].max() > 100  # a hundred peaks a frame and more
    np.testing.assert_allclose(whole[:, :36].sum(axis=1), whole[:, 38], rtol=1e-5)  # the bin window is a partition of unity
    a = gpu_ctx.upload(case.w)
    try:
        assert gpu_ctx.chroma(a, SR, HOP, 3, 11).tobytes() == whole[3:14].tobytes()
        try:
            gpu_ctx.set_frames_per_block(3)
            assert gpu_ctx.chroma(a, SR, HOP).tobytes() == whole.tobytes()
        finally:
            gpu_ctx.set_frames_per_block(0)
    finally:
        a.free()


def test_window_sums_are_the_references_bytes(mxlib, gpu_ctx, gpu_rec):
    rec = gpu_rec["c_major"].copy()
    rec[40, 3], rec[41, 36], rec[42] = np.nan, np.inf, -np.inf  # a window holding records that are not finite
    jobs = [(0, 1), (5, 2), (30, 37), (0, len(rec)), (7, 0), (len(rec), 0)]
    want = np.array([K.chroma_sum(rec, f, c) for f, c in jobs])
    got = gpu_ctx.chroma_sum(rec, jobs)
    assert got.tobytes() == want.tobytes()
    d_rec, d_jobs, d_out = DevBuf(rec.nbytes), DevBuf(16 * len(jobs)), DevBuf(320 * (len(jobs) + 2), fill=0xA5)
    try:
        d_rec.write(rec)
        d_jobs.write(np.array(jobs, dtype=np.int64))
        gpu_ctx.chroma_sum_dev(d_rec.ptr, len(rec), d_jobs.ptr, len(jobs), d_out.ptr + 320)
        gpu_ctx.synchronize()
        raw = d_out.read(np.uint8)
        assert raw[:320].tobytes() == b"\xa5" * 320 and raw[320 * (len(jobs) + 1):].tobytes() == b"\xa5" * 320
        assert raw[320:320 * (len(jobs) + 1)].tobytes() == want.tobytes()
        # the device form cannot see its jobs: one that leaves the records is clipped to them
        d_jobs.write(np.array([(-5, 10), (len(rec) - 3, 1 << 40)], dtype=np.int64))
        gpu_ctx.chroma_sum_dev(d_rec.ptr, len(rec), d_jobs.ptr, 2, d_out.ptr + 320)
        gpu_ctx.synchronize()
        clipped = d_out.read(np.float64, offset=320, count=80).reshape(2, 40)
        assert clipped.tobytes() == np.array([K.chroma_sum(rec, 0, 10), K.chroma_sum(rec, len(rec) - 3, 3)]).tobytes()
    finally:
        for b in (d_rec, d_jobs, d_out):
            b.free()
    for bad in ([(-1, 2)], [(0, len(rec) + 1)], [(len(rec) + 1, 0)], [(3, -1)]):
        with pytest.raises(mxlib.MxError) as e:
            gpu_ctx.chroma_sum(rec, bad)
        assert e.value.code == -1


def test_refusals_touch_nothing(mxlib, gpu_ctx, cases):
    L = mxlib._capi.lib()
    w = cases["chord"].w
    a = gpu_ctx.upload(w)
    frames = -(-len(w) // HOP)
    buf = DevBuf(4 * REC, fill=0xA5)
    try:
        bads = [dict(sr=0), dict(sr=-1), dict(hop=0), dict(hop=16385), dict(first=-1), dict(first=frames, count=1), dict(count=frames + 1),
                dict(fmin=0.0), dict(fmin=-1.0), dict(fmax=float("inf")), dict(fmin=float("nan")), dict(fmin=5000.0, fmax=100.0),
                dict(fmin=23990.0, fmax=24000.0), dict(fmin=1.0, fmax=10.0), dict(floor=-1.0), dict(floor=float("nan")),
                dict(rel=-0.1), dict(rel=1.5), dict(rel=float("nan"))]
        for bad in bads:
            kw = dict(sr=SR, hop=HOP, first=0, count=2)
            params = {k: bad[k] for k in bad if k not in kw}
            kw.update({k: bad[k] for k in bad if k in kw})
            with pytest.raises(mxlib.MxError) as e:
                gpu_ctx.chroma_dev(a, kw["sr"], kw["hop"], kw["first"], kw["count"], buf.ptr + REC, **params)
            assert e.value.code == -1, bad
            with pytest.raises(mxlib.MxError):
                gpu_ctx.chroma(a, kw["sr"], kw["hop"], kw["first"], kw["count"], **params)
            if "first" not in bad and "count" not in bad:  # (the whole-file call has no span to get wrong)
                with pytest.raises(mxlib.MxError):
                    gpu_ctx.key_detect(a, kw["sr"], kw["hop"], **params)
        assert L.mx_chroma_dev(gpu_ctx.handle, a.handle, SR, HOP, 0, 2, None, None) == -1
        assert L.mx_chroma_dev(None, a.handle, SR, HOP, 0, 2, None, C.c_void_p(buf.ptr)) == -1
        assert L.mx_chroma_dev(gpu_ctx.handle, None, SR, HOP, 0, 2, None, C.c_void_p(buf.ptr)) == -1
        assert L.mx_chroma_sum_dev(gpu_ctx.handle, None, 4, C.c_void_p(buf.ptr), 1, C.c_void_p(buf.ptr)) == -1
        assert L.mx_chroma_sum_dev(gpu_ctx.handle, C.c_void_p(buf.ptr), -1, C.c_void_p(buf.ptr), 1, C.c_void_p(buf.ptr)) == -1
        assert L.mx_chroma_sum_dev(gpu_ctx.handle, C.c_void_p(buf.ptr), 4, None, 1, C.c_void_p(buf.ptr)) == -1
        assert L.mx_chroma_sum_dev(None, C.c_void_p(buf.ptr), 4, C.c_void_p(buf.ptr), 1, C.c_void_p(buf.ptr)) == -1
        key = mxlib._capi.Key()
        assert L.mx_key_detect(gpu_ctx.handle, a.handle, SR, HOP, None, 0, 1, None, None, None) == -1
        out, cnt = C.c_void_p(), C.c_int64()
        assert L.mx_key_detect(gpu_ctx.handle, a.handle, SR, HOP, None, -1, 1, C.byref(key), C.byref(out), C.byref(cnt)) == -1
        assert L.mx_key_detect(gpu_ctx.handle, a.handle, SR, HOP, None, 4, 0, C.byref(key), C.byref(out), C.byref(cnt)) == -1
        assert L.mx_key_detect(gpu_ctx.handle, a.handle, SR, HOP, None, 4, 1, C.byref(key), C.byref(out), None) == -1
        gpu_ctx.synchronize()
        assert buf.read(np.uint8).tobytes() == b"\xa5" * (4 * REC)  # every bad call was refused before any launch
        assert L.mx_key_detect(gpu_ctx.handle, a.handle, SR, HOP, None, 4, 1, C.byref(key), None, None) == 0  # windows may be NULL
        assert gpu_ctx.chroma(a, SR, HOP, 0, 0).shape == (0, K.COLS)
    finally:
        buf.free()
        a.free()


def test_key_scale_and_tuning_of_the_takes(mxlib, gpu_ctx, cases, gpu_rec):
    for name, (w, tonic, mode, tuning) in K.takes().items():
        ref_key = K.key_detect(None, SR, rec=cases[name].ref.astype(np.float32))[0]
        # the guard, on the reference alone: the winner leads the other 23 candidates by far more than f32 records can move it
        assert ref_key["clarity"] > 0.1 and (ref_key["tonic"], ref_key["mode"]) == (tonic, mode), name
        a = gpu_ctx.upload(w)
        try:
            key, wins = gpu_ctx.key_detect(a, SR, HOP, window_frames=48, window_hop=24)
        finally:
            a.free()
        print(f"{name}: tonic {key['tonic']} mode {key['mode']} tuning {key['tuning_cents']:+.4f} (reference {ref_key['tuning_cents']:+.4f}, "
              f"truth {tuning:+.3f}) clarity {key['clarity']:.3f}")
        assert (key["tonic"], key["mode"], key["scale_mask"]) == (tonic, mode, K.scale_mask(tonic, mode)), name
        assert abs(key["tuning_cents"] - ref_key["tuning_cents"]) <= 0.01, name
        # the call is its parts: the host logic on the sums of the GPU's own records, field for field
        take, want = K.key_detect(None, SR, window_frames=48, window_hop=24, rec=gpu_rec[name])
        same_key(key, take, name)
        assert len(wins) == len(want) == 6
        for got_w, (first, frames, k) in zip(wins, want):
            assert (int(got_w["first_frame"]), int(got_w["frames"])) == (first, frames)
            same_key({f: got_w["key"][f].item() for f in KEY_FIELDS}, k, (name, first))


def test_the_whole_chain_lands_on_the_detected_grid(mxlib, gpu_ctx):
    """f0 track -> notes -> mx_key_detect -> mx_correction_markers_tuned at strength 1 -> mx_psola_render -> track again, on the
    a4 = 446 Hz take with every note further detuned: the notes come out on the 446 Hz C-major grid, inside the bound
    test_key_host.py establishes on psola_ref and key_ref; the plain chain (all twelve classes, A = 440 Hz) misses that grid."""
    from test_key_host import CHAIN_DETUNE, check_chain

    hop = 256
    w = K.melody(K.C_MAJOR, 446.0, detune=CHAIN_DETUNE)
    a = gpu_ctx.upload(w)
    try:
        tr = gpu_ctx.f0_track(a, SR, hop)
        notes = mxlib.detect_notes(tr, SR, hop)
        key, _ = gpu_ctx.key_detect(a, SR)
        assert (key["tonic"], key["mode"]) == (3, 0)
        out = []
        for markers in (mxlib.correction_markers_tuned(notes, 1.0, key["scale_mask"], key["tuning_cents"]), mxlib.correction_markers(notes, 1.0, 0)):
            pcm, _ = gpu_ctx.psola_render(a, SR, hop, tr, markers, want_i16=False)
            b = gpu_ctx.upload(pcm)
            try:
                out.append(mxlib.detect_notes(gpu_ctx.f0_track(b, SR, hop), SR, hop)["note"])
            finally:
                b.free()
    finally:
        a.free()
    check_chain(out[0], out[1], "GPU")
