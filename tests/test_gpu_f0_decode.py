"""The YIN candidate ladder and the Viterbi f0 decoder on the MI355X: candidates against the f64 ladder
(tests/f0_decode_ref.py), the track of the same launch against f0_track, the decode against the integer reference byte for byte
at every chunk length and at the counts where a chunked scan goes wrong, GLITCH end to end, guard bands, bad samples, and
melonix::PitchTrack's `decoded` option."""
import subprocess

import numpy as np
import pytest

import f0_decode_ref as D
import yin_ref as Y
from conftest import SR, DevBuf, accum_sweep, noisy
from facade_build import build_driver
from test_gpu_f0 import _signals

pytestmark = pytest.mark.gpu

HOP = 256
CHUNKS = (2, 7, 64, 0)  # 0: the default
ZERO = dict(unvoiced_cost=0.0, jump_cost=0.0, switch_cost=0.0, max_jump_cents=0)
STIFF = dict(unvoiced_cost=1.25, jump_cost=16.0, switch_cost=0.0, max_jump_cents=12000)


def _rung_ties(dp, picked_k, tmin, tmax, theta, eps=1e-4):
    """Near-ties of one rung: yin_ref.near_ties on the tau the reference's rung picked; where that rung found nothing under
    theta (an empty rung, or slot 0's fallback) also any d' of the range within eps of theta — the kernel may have found one."""
    ties = Y.near_ties(dp, picked_k, tmin, tmax, theta, eps_theta=eps, eps_cmp=eps)
    for i in range(len(picked_k)):
        t = int(picked_k[i])
        if (t <= 0 or not dp[i, t] < theta) and np.any(np.abs(dp[i, tmin:tmax + 1] - theta) < eps):
            ties[i] = True
    return ties


# ---- 5. candidates against the ladder reference ----
@pytest.mark.parametrize("sr", [48000, 44100])
def test_candidates_against_the_ladder_reference(gpu_ctx, sr):
    tmin, tmax = Y.tau_range(sr)
    th = D.thetas(0.15)
    frames, excused = 0, np.zeros(D.CANDS, dtype=np.int64)
    for name, w in _signals(sr).items():
        a = gpu_ctx.upload(w)
        _, got = gpu_ctx.f0_candidates(a, sr, HOP)
        a.free()
        ref, dp, picked = D.ladder(w, sr, HOP)
        assert got.shape == ref.shape
        frames += len(got)
        tie_upto = np.zeros(len(got), dtype=bool)
        for k in range(D.CANDS):
            # a rung's slot also depends on the earlier rungs (the duplicate rule): a near-tie of any rung <= k excuses slot k
            tie_upto |= _rung_ties(dp, picked[:, k], tmin, tmax, th[k])
            same = got["tau"][:, k] == ref["tau"][:, k]
            bad = ~same & ~tie_upto
            assert not bad.any(), f"sr={sr} {name} slot {k}: tau differs outside near-ties at frames {np.nonzero(bad)[0][:10]}"
            excused[k] += int((~same).sum())
            filled = same & (ref["tau"][:, k] > 0)
            empty = same & (ref["tau"][:, k] == 0)
            g, r = got[:, k], ref[:, k]
            assert (g["period"][empty] == 0).all() and (g["aperiodicity"][empty] == 1).all() and (g["cents"][empty] == 0).all()
            if filled.any():
                c = np.abs(1200 * np.log2(g["period"][filled].astype(np.float64) / r["period"][filled]))
                ap = np.abs(g["aperiodicity"][filled] - r["aperiodicity"][filled])
                note = 100.0 * (24.0 + 12.0 * np.log2(sr / g["period"][filled].astype(np.float64) / 55.0))
                ce = np.abs(g["cents"][filled] - note)
                print(f"ladder sr={sr} {name} slot {k}: {int(filled.sum())} filled, period max {c.max():.3g} cents, "
                      f"aperiodicity max err {ap.max():.2e}, cents max err {ce.max():.3f}")
                assert (c <= 1.0).all()
                assert (ap <= 1e-4 + 1e-3 * r["aperiodicity"][filled]).all()
                assert (ce <= 1.0).all()
    print(f"ladder sr={sr}: tau excused as a near-tie per rung {excused.tolist()} of {frames} frames")
    assert (excused < 0.005 * frames).all()


# ---- 6. track agreement ----
def test_track_agreement_sub_launches_and_device_form(gpu_ctx):
    w = noisy(accum_sweep(6 * SR))
    a = gpu_ctx.upload(w)
    plain = gpu_ctx.f0_track(a, SR, HOP)
    track, cands = gpu_ctx.f0_candidates(a, SR, HOP)
    F = len(plain)
    assert track.tobytes() == plain.tobytes()
    under = np.nonzero(plain["aperiodicity"] < np.float32(0.15))[0]
    assert len(under) > F // 2
    hit = cands["tau"][under] == plain["tau"][under][:, None]
    assert (hit.sum(axis=1) == 1).all()
    slot = np.argmax(hit, axis=1)
    for k in ("period", "aperiodicity"):
        assert cands[k][under, slot].tobytes() == plain[k][under].tobytes(), k
    rng = np.random.default_rng(12)
    cuts = np.unique(np.concatenate([[0, F], rng.integers(1, F, 12)]))
    parts = [gpu_ctx.f0_candidates(a, SR, HOP, int(lo), int(hi - lo)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate([p[1] for p in parts]).tobytes() == cands.tobytes()
    assert np.concatenate([p[0] for p in parts]).tobytes() == plain.tobytes()
    dt, dc = DevBuf(F * 16, fill=0x5A), DevBuf(F * 64, fill=0x5A)
    gpu_ctx.f0_candidates_dev(a, SR, HOP, 0, F, dt.ptr, dc.ptr)
    gpu_ctx.synchronize()
    assert dt.read(np.uint8).tobytes() == plain.tobytes() and dc.read(np.uint8).tobytes() == cands.tobytes()
    dc2 = DevBuf(F * 64, fill=0x5A)
    gpu_ctx.f0_candidates_dev(a, SR, HOP, 0, F, None, dc2.ptr)  # no track wanted
    gpu_ctx.synchronize()
    assert dc2.read(np.uint8).tobytes() == cands.tobytes()
    for b in (dt, dc, dc2):
        b.free()
    a.free()


# ---- 7. decode, exact ----
def _decode_all_chunks(ctx, track, cands, params, label):
    """The device decode of (track, cands) at every chunk length, host and device (aliased) forms, against the reference."""
    rs, ro = D.decode(track, cands, params)
    try:
        for c in CHUNKS:
            ctx.f0_decode_set_chunk(c)
            out, state = ctx.f0_decode(track, cands, **(params or {}))
            assert state.tobytes() == rs.tobytes(), f"{label} chunk {c}: state differs at {np.nonzero(state != rs)[0][:10]}"
            assert out.tobytes() == ro.tobytes(), f"{label} chunk {c}"
        # the device form, d_out aliasing d_track, at the last chunk length and one short one
        F = len(track)
        if F:
            for c in (7, 0):
                ctx.f0_decode_set_chunk(c)
                dt, dc, ds = DevBuf(F * 16), DevBuf(F * 64), DevBuf(F, fill=0x5A)
                dt.write(track)
                dc.write(cands)
                ctx.f0_decode_dev(dt.ptr, dc.ptr, F, dt.ptr, ds.ptr, **(params or {}))
                ctx.synchronize()
                assert dt.read(np.uint8).tobytes() == ro.tobytes() and ds.read(np.uint8).tobytes() == rs.tobytes(), (label, c)
                for b in (dt, dc, ds):
                    b.free()
    finally:
        ctx.f0_decode_set_chunk(0)
    return rs


@pytest.mark.parametrize("params", [None, ZERO, STIFF], ids=["default", "zero", "stiff"])
def test_decode_equals_the_reference_on_glitch_and_a_host_table(gpu_ctx, params):
    a = gpu_ctx.upload(D.glitch())
    track, cands = gpu_ctx.f0_candidates(a, D.GLITCH_SR, D.GLITCH_HOP)
    a.free()
    rs = _decode_all_chunks(gpu_ctx, track, cands, params, "GLITCH")
    assert len(rs) == 375
    track, cands = D.random_table(np.random.default_rng(5), 500, stretches=((5, 9), (100, 240), (499, 500)))
    rs = _decode_all_chunks(gpu_ctx, track, cands, params, "host table")
    if params is not ZERO:
        assert (rs[100:240] == D.UNVOICED).all() and (rs != D.UNVOICED).any()


def test_decode_equals_the_reference_on_the_signal_set(gpu_ctx):
    for name, w in _signals(SR).items():
        a = gpu_ctx.upload(w)
        track, cands = gpu_ctx.f0_candidates(a, SR, HOP)
        a.free()
        _decode_all_chunks(gpu_ctx, track, cands, None, name)


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 197])
def test_decode_at_the_counts_around_a_chunk(gpu_ctx, count):
    """count in {1, 2, C-1, C, C+1, 3C+5} for C = 64 (and the other chunk lengths on the way)."""
    track, cands = D.random_table(np.random.default_rng(100 + count), count, stretches=((count // 2, count // 2 + 3),))
    for params in (None, ZERO):
        _decode_all_chunks(gpu_ctx, track, cands, params, f"count {count}")


def test_decode_of_nothing_and_release(gpu_ctx, mxlib):
    out, state = gpu_ctx.f0_decode(np.zeros(0, mxlib.F0_DTYPE), np.zeros((0, 4), mxlib.F0_CAND_DTYPE))
    assert len(out) == 0 and len(state) == 0
    track, cands = D.random_table(np.random.default_rng(9), 300)
    rs, ro = D.decode(track, cands)
    out, state = gpu_ctx.f0_decode(track, cands)
    gpu_ctx.release_scratch()  # the decode's work buffers go; the next call takes new ones
    out2, state2 = gpu_ctx.f0_decode(track, cands)
    assert out.tobytes() == out2.tobytes() == ro.tobytes() and state.tobytes() == state2.tobytes() == rs.tobytes()


# ---- 8. GLITCH end to end ----
def test_glitch_end_to_end(gpu_ctx):
    a = gpu_ctx.upload(D.glitch())
    plain = gpu_ctx.f0_track(a, D.GLITCH_SR, D.GLITCH_HOP)
    decoded = gpu_ctx.f0_track_decoded(a, D.GLITCH_SR, D.GLITCH_HOP)
    track, cands = gpu_ctx.f0_candidates(a, D.GLITCH_SR, D.GLITCH_HOP)
    a.free()
    D.glitch_assertions(plain, decoded, "device")
    out, _ = gpu_ctx.f0_decode(track, cands)
    assert decoded.tobytes() == out.tobytes()  # one call or two: the same track


# ---- 9. guard bands ----
@pytest.mark.parametrize("first,count,hop", [(0, 1, 256), (3, 17, 256), (0, 100, 255), (50, 33, 1000)])
def test_guard_bands(gpu_ctx, first, count, hop):
    G, SENT = 64 * 1024, 0xA5
    w = noisy(accum_sweep(3 * SR))
    a = gpu_ctx.upload(w)
    track, cands = gpu_ctx.f0_candidates(a, SR, hop, first, count)
    out, state = gpu_ctx.f0_decode(track, cands)

    def banded(buf, lo, n, want, what):
        host = buf.read(np.uint8)
        assert (host[:lo] == SENT).all() and (host[lo + n:] == SENT).all(), what
        assert host[lo:lo + n].tobytes() == want.tobytes(), what

    try:
        for shift, chunk in ((0, 0), (4, 7)):
            gpu_ctx.f0_decode_set_chunk(chunk)
            bt, bc = DevBuf(2 * G + shift + count * 16, fill=SENT), DevBuf(2 * G + shift + count * 64, fill=SENT)
            bo, bs = DevBuf(2 * G + shift + count * 16, fill=SENT), DevBuf(2 * G + shift // 4 + count, fill=SENT)
            lo, ls = G + shift, G + shift // 4
            gpu_ctx.f0_candidates_dev(a, SR, hop, first, count, bt.ptr + lo, bc.ptr + lo)
            gpu_ctx.f0_decode_dev(bt.ptr + lo, bc.ptr + lo, count, bo.ptr + lo, bs.ptr + ls)
            gpu_ctx.synchronize()
            banded(bt, lo, count * 16, track, "d_track")
            banded(bc, lo, count * 64, cands, "d_cands")
            banded(bo, lo, count * 16, out, "d_out")
            banded(bs, ls, count, state, "d_state")
            for b in (bt, bc, bo, bs):
                b.free()
    finally:
        gpu_ctx.f0_decode_set_chunk(0)
    a.free()


# ---- 10. bad samples ----
def test_bad_samples(gpu_ctx):
    w = noisy(accum_sweep(2 * SR)).copy()
    w[[5000, 5001, 40000]] = np.inf
    w[[20000, 60001]] = np.nan
    w[70000] = -np.inf
    a = gpu_ctx.upload(w)
    track, cands = gpu_ctx.f0_candidates(a, SR, HOP)  # (check() raises on any status but MX_OK)
    decoded = gpu_ctx.f0_track_decoded(a, SR, HOP)
    plain = gpu_ctx.f0_track(a, SR, HOP)
    a.free()
    assert track.tobytes() == plain.tobytes()
    filled = cands["tau"] > 0
    assert np.isfinite(cands["aperiodicity"][filled]).all()
    e = cands[~filled]
    assert (e["tau"] == 0).all() and (e["period"] == 0).all() and (e["aperiodicity"] == 1).all() and (e["cents"] == 0).all()
    touched = np.zeros(len(track), dtype=bool)
    for s in (5000, 5001, 40000, 20000, 60001, 70000):
        touched[max(0, (s - 2048) // HOP):(s + 2048) // HOP + 1] = True
    assert filled[~touched].any(axis=1).all()  # the frames clear of the bad samples track as ever
    rs, ro = D.decode(track, cands)
    out, state = gpu_ctx.f0_decode(track, cands)
    assert state.tobytes() == rs.tobytes() and out.tobytes() == ro.tobytes() and decoded.tobytes() == ro.tobytes()


# ---- 11. the facade ----
def test_pitch_track_facade_decoded(gpu_ctx, mxlib, tmp_path):
    exe = build_driver(tmp_path, "pitch_track_decoded_driver")
    w = D.glitch()
    src = tmp_path / "in.f32"
    w.astype("<f4").tofile(src)
    a = gpu_ctx.upload(w)
    want = {0: gpu_ctx.f0_track(a, D.GLITCH_SR, HOP), 1: gpu_ctx.f0_track_decoded(a, D.GLITCH_SR, HOP)}
    a.free()
    notes = {}
    for decoded in (0, 1):
        out = tmp_path / f"frames{decoded}.f0"
        r = subprocess.run([exe, str(src), str(D.GLITCH_SR), str(decoded), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.fromfile(out, dtype=mxlib.F0_DTYPE).tobytes() == want[decoded].tobytes(), decoded
        notes[decoded] = int(r.stdout.split()[-1])
    assert notes[1] == 1 and notes[0] >= 3
