"""The kernels that WRITE audio — the reference resynthesis, PSOLA in both instantiations, the phase vocoder — on takes beyond
full scale and on takes with a sample that is Inf or NaN, and the int16 each of them stores (include/melonix_amd.h "PCM
conversions": the reference form for the resynthesis, the clamped form for the others).  The assertions are those of
tests/pcm_extremes.py; the f0 tracker, which the PSOLA renders take their records from, gets the frame walkers' rule of
tests/bad_samples.py here as well."""
import numpy as np
import pytest

import pcm_extremes as P
from conftest import SR, accum_sweep, loaded_hip, noisy
from test_gpu_guard import Guarded, _to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_ctx):
    return loaded_hip()


# ---- resynthesis: every store arm -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def arms(mxlib):
    from melonix_amd import STEP_DTYPE
    w, plateaus = P.arms_audio()
    st, total = P.arms_schedule(STEP_DTYPE, plateaus)
    want, arm = P.arms_expected(w, st, total)
    return w, st, total, want, arm


def _check_arms(f32, i16, arms, oracle, what):
    w, st, total, want, arm = arms
    if f32 is not None:
        P.same_floats(f32, want, what)
    want16 = oracle.pcm_to_i16(want)
    wrong = i16 != want16
    assert not wrong.any(), (what, [(int(k), float(want[k]), int(i16[k]), int(want16[k]), int(arm[k])) for k in np.nonzero(wrong)[0][:8]])


def test_resynth_arms_aligned_outputs(gpu_ctx, oracle, arms):
    """mx_resynth (16-byte aligned outputs: the vector kernel, its long-grain loop for grain_len > 2304): f32 == the lerp
    restated, int16 == the compiled reference's conversion of it in every arm, int16 alone the same."""
    w, st, total, want, arm = arms
    a = gpu_ctx.upload(w)
    try:
        f32, i16 = gpu_ctx.resynth(a, st, total)
        _check_arms(f32, i16, arms, oracle, "f32 and int16")
        only16 = gpu_ctx.resynth(a, st, total, want_f32=False)[1]
        _check_arms(None, only16, arms, oracle, "int16 alone")
    finally:
        a.free()


@pytest.mark.parametrize("lead", [0, 1])
def test_resynth_arms_device_outputs(gpu_ctx, hip, oracle, arms, lead):
    """mx_resynth_dev into guarded buffers: outputs at the start of the payload (vector kernel) and one element in (not 16-byte
    aligned: the scalar kernel).  The same values, and the 0xA5 bands around both outputs survive."""
    w, st, total, want, arm = arms
    a = gpu_ctx.upload(w)
    d_st = _to_device(hip, st)
    bufs = []
    try:
        for outs in ((True, True), (False, True)):
            gf = Guarded(hip, total * 4, 4 * lead) if outs[0] else None
            gi = Guarded(hip, total * 2, 2 * lead)
            bufs += [b for b in (gf, gi) if b is not None]
            gpu_ctx.resynth_dev(a, d_st.value, len(st), total, gf.ptr if gf else None, gi.ptr)
            gpu_ctx.synchronize()
            f32 = gf.fetch().view(np.float32) if gf else None
            _check_arms(f32, gi.fetch().view(np.int16), arms, oracle, ("dev", lead, outs))
    finally:
        for b in bufs:
            b.free()
        hip.hipFree(d_st)
        a.free()


# ---- resynthesis: the whole chain -------------------------------------------------------------------------------------------------

CHAIN_MARKERS = [(1000, 0, 0.0, 5.0), (30000, 0, 0.2, -7.0), (60000, 0, -0.1, 9.0), (2 * SR - 1, 0, 0, -2.0)]  # bends up and down


def _chain_take(bad):
    w = (noisy(accum_sweep(2 * SR)) * np.float32(4.0)).astype(np.float32)
    if bad:
        for s, v in ((5003, 1e9), (20011, np.inf), (40009, -np.inf), (60013, np.nan), (80021, np.inf), (90001, -1e9), (95003, np.nan)):
            w[s] = v
    return w


@pytest.mark.parametrize("bad", [False, True])
def test_resynth_chain_beyond_full_scale(gpu_ctx, oracle, mxlib, bad):
    """A take at four times full scale (int16 wraps in the reference), and the same with samples at 1e9, +-Inf and NaN: grains
    (Inf and NaN in the scan's !(x >= 0) and !(x < 0) bitmaps), schedule, f32 and int16 equal the oracle's."""
    w = _chain_take(bad)
    a = gpu_ctx.upload(w)
    try:
        s, l = gpu_ctx.grains_dev(a)
        rs, rl = oracle.grains(w)
        assert np.array_equal(s, rs) and np.array_equal(l, rl)
        steps, total = mxlib.schedule_build(w, SR, s, l, CHAIN_MARKERS)
        osteps, opcm = oracle.export_run(w, SR, CHAIN_MARKERS, memo=False)
        assert total == len(opcm) and len(steps) == len(osteps)
        for f in ("cursor", "grain_start", "grain_len", "rate", "sz", "out_offset"):
            assert np.array_equal(steps[f], osteps[f]), f
        P.same_floats(steps["next_first"], osteps["next_first"], "next_first")
        f32, i16 = gpu_ctx.resynth(a, steps, total)
        P.same_floats(f32, opcm, "pcm")
        assert np.abs(opcm[np.isfinite(opcm)]).max() > 1.5
        if bad:
            assert np.isnan(opcm).any() and (opcm == np.inf).any() and (opcm == -np.inf).any() and (np.abs(opcm[np.isfinite(opcm)]) > 1e8).any()
        assert np.array_equal(i16, oracle.pcm_to_i16(opcm))
        assert np.array_equal(gpu_ctx.resynth(a, steps, total, want_f32=False)[1], i16)
    finally:
        a.free()


# ---- PSOLA, plain and formant -----------------------------------------------------------------------------------------------------

PSOLA_KINDS = ("plain", "formant step 32768", "formant step 131072")  # the step extremes of tests/test_gpu_psola_formant.py
PSOLA_TILE = 32 * 1024  # a multiple of the kernel's 1024-output tile, mid-take


@pytest.fixture(scope="module")
def psola(gpu_ctx, mxlib):
    """The vowel of tests/test_gpu_psola.py, the CLEAN take's f0 track, and per kind the records planned from it (+4 st; the
    envelope at -12 / +12 st for the formant kinds) with the clean render: only the overlap-add ever sees a bad sample."""
    import psola_ref
    from test_gpu_psola import HOP, bend, vowel
    w = vowel()
    n = len(w)
    a = gpu_ctx.upload(w)
    try:
        tr = gpu_ctx.f0_track(a, SR, HOP)
        mk = bend(n, 4.0)
        plans = {"plain": mxlib.psola_plan(n, SR, HOP, tr, mk),
                 "formant step 32768": mxlib.psola_plan_formant(n, SR, HOP, tr, mk, [(0, -12.0)]),
                 "formant step 131072": mxlib.psola_plan_formant(n, SR, HOP, tr, mk, [(0, 12.0)])}
        assert (plans["formant step 32768"][0]["step"] == 32768).all() and (plans["formant step 131072"][0]["step"] == 131072).all()
        clean = {k: _psola_synth(gpu_ctx, a, g, L) for k, (g, L) in plans.items()}
    finally:
        a.free()
    for k, (g, L) in plans.items():
        ref = psola_ref.render(w, g, L)
        assert np.abs(clean[k][0] - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-9, k
    return w, plans, clean


def _psola_synth(gpu_ctx, a, g, L, **want):
    return (gpu_ctx.psola_synth_formant if "step" in g.dtype.names else gpu_ctx.psola_synth)(a, g, L, **want)


@pytest.mark.parametrize("kind", PSOLA_KINDS)
@pytest.mark.parametrize("k", [1, 2, 20])
def test_psola_beyond_full_scale(gpu_ctx, psola, kind, k):
    """The take times 2, 4 and 2^20: f32 within the PSOLA tolerance (2e-5 of the render's peak, so scaled by the level) of the
    f64 restatement on the scaled take, int16 == the clamped form of the f32 output, int16 alone the same.  Times 4 and 2^20 the
    int16 saturates both ways.  Times 2 it cannot: the vowel is normalised to a peak of 0.5, a render of it peaks at 1.0 (measured
    on an MI355X: the f64 restatement's peak is 1.00 to three digits in all three kinds), so that case checks the conversion up
    to full scale and the two above it the clamp."""
    import psola_ref
    w, plans, clean = psola
    g, L = plans[kind]
    ws = np.ldexp(w, k).astype(np.float32)
    a = gpu_ctx.upload(ws)
    try:
        f32, i16 = _psola_synth(gpu_ctx, a, g, L)
        only16 = _psola_synth(gpu_ctx, a, g, L, want_f32=False)[1]
    finally:
        a.free()
    ref = psola_ref.render(ws, g, L)
    err, tol = float(np.abs(f32.astype(np.float64) - ref).max()), 2e-5 * float(np.abs(ref).max()) + 1e-9
    print(f"psola {kind} x 2^{k}: max err {err:.3g} (tolerance {tol:.3g}), peak {np.abs(ref).max():.3g}")
    assert err <= tol
    P.check_clamped(i16, f32, (kind, k))
    if k > 1:
        P.saturates_both_ways(i16, (kind, k))
    assert np.array_equal(only16, i16)


def _psola_positions(n, g):
    H = int(round(1.0 / float(np.median(g["inv_half"]))))  # the grain reach of the voiced take: one period
    import psola_ref
    over = g[(g["out_lo"] < PSOLA_TILE) & (g["out_hi"] > PSOLA_TILE)][0]  # a grain with outputs in both tiles
    seam = int(psola_ref._source(over, np.array([PSOLA_TILE - 1]))[0][0]) + 1  # the second tap of the last output of a tile
    return {"first": 0, "last": n - 1, "mid": n // 2, "tile - reach": PSOLA_TILE - H, "tile": PSOLA_TILE, "tile + reach": PSOLA_TILE + H,
            "seam": seam}


@pytest.mark.parametrize("kind", PSOLA_KINDS)
@pytest.mark.parametrize("where", ["first", "last", "mid", "tile - reach", "tile", "tile + reach", "seam"])
def test_psola_one_bad_sample(gpu_ctx, psola, kind, where):
    """One sample NaN, +Inf or -Inf.  On the CPU first: the f64 restatement is non-finite exactly at the outputs whose grains
    read that source sample as either tap.  Then the device: non-finite at the same outputs sample for sample, the clean
    render's bytes everywhere else, int16 0 at NaN outputs, +-32767 at +-Inf outputs, unchanged elsewhere."""
    import psola_ref
    w, plans, clean = psola
    g, L = plans[kind]
    s = _psola_positions(len(w), g)[where]
    readers = P.psola_readers(g, L, s)
    if where in ("mid", "tile", "seam"):
        assert readers.any()
    if where == ("tile" if kind == "formant step 131072" else "seam"):
        assert readers[:PSOLA_TILE].any() and readers[PSOLA_TILE:].any()  # the readers lie in two workgroups' tiles
    for name, v in P.BAD.items():
        wb = w.copy()
        wb[s] = v
        with np.errstate(invalid="ignore"):
            ref = psola_ref.render(wb, g, L)
        a = gpu_ctx.upload(wb)
        try:
            f32, i16 = _psola_synth(gpu_ctx, a, g, L)
        finally:
            a.free()
        P.check_psola_bad(f32, i16, ref, readers, clean[kind][0], clean[kind][1], (kind, where, name))
        if name != "nan" and readers.any():
            assert np.isinf(f32[readers]).any() or np.isnan(f32[readers]).all()


# ---- phase vocoder, constant ratio and markers ------------------------------------------------------------------------------------

PV_MODES = ["+5 st", "-12 st", "markers"]
PV_CHUNK = 32  # frames per chunk of the chunked runs: the smallest


@pytest.fixture(scope="module")
def pvo():
    from oracle import pv_oracle
    return pv_oracle


def _pv_run(ctx, a, mode, **want):
    from test_gpu_pv_edges import LEVEL_MARKERS
    return ctx.pv_render(a, SR, LEVEL_MARKERS, **want) if mode == "markers" else ctx.pv_pitch_shift(a, float(mode.split()[0]), **want)


@pytest.fixture(scope="module")
def pv_take(gpu_ctx, pvo):
    """The render signal of tests/test_gpu_pv_edges.py, one second; per mode the clean render, the frames' centres and every
    output's first tap (pcm_extremes.pv_span)."""
    from test_gpu_pv_edges import LEVEL_MARKERS, _render_signal
    w = _render_signal(SR)
    a = gpu_ctx.upload(w)
    try:
        gpu_ctx.pv_set_chunk_frames(0)
        clean = {mode: _pv_run(gpu_ctx, a, mode) for mode in PV_MODES}
    finally:
        a.free()
    taps = {mode: P.pv_taps_markers(pvo, len(w), SR, LEVEL_MARKERS) if mode == "markers" else P.pv_taps_constant(pvo, len(w), float(mode.split()[0]))
            for mode in PV_MODES}
    return w, clean, taps


@pytest.mark.parametrize("mode", PV_MODES)
def test_pv_beyond_full_scale(gpu_ctx, pv_take, mode):
    """The take times 4: f32 == 4 x the base render bit for bit (the scale law), int16 == the clamped form of it, saturated both
    ways; int16 alone the same."""
    w, clean, _ = pv_take
    a = gpu_ctx.upload((w * np.float32(4.0)).astype(np.float32))
    try:
        f32, i16 = _pv_run(gpu_ctx, a, mode)
        only16 = _pv_run(gpu_ctx, a, mode, want_f32=False)[1]
    finally:
        a.free()
    assert f32.tobytes() == (clean[mode][0] * np.float32(4.0)).astype(np.float32).tobytes()
    P.check_clamped(i16, f32, mode)
    P.saturates_both_ways(i16, mode)
    assert np.array_equal(only16, i16)


def _pv_positions(n, a):
    """first, last, mid, and the centre of the frame a chunk of PV_CHUNK frames starts with: frames of both chunks hold it."""
    return {"first": 0, "last": n - 1, "mid": n // 2, "chunk": int(a[PV_CHUNK])}


@pytest.mark.parametrize("mode", PV_MODES)
@pytest.mark.parametrize("where", ["first", "last", "mid", "chunk"])
def test_pv_one_bad_sample(gpu_ctx, mxlib, pvo, pv_take, mode, where):
    """One sample NaN, +Inf or -Inf (pcm_extremes.check_pv_bad): the clean bytes before the span of the frames that hold it,
    nothing finite inside, everything finite behind; for NaN within the usual tolerance (2e-5 at a constant ratio, 5e-5 through
    markers) of the oracle behind the span; the same bytes in chunks of 32 frames; int16 as defined, alone as well; and the compact
    record pool does not overflow (the arena keeps its compact size)."""
    w, clean, taps = pv_take
    a_f, m = taps[mode]
    s = _pv_positions(len(w), a_f)[where]
    assert 0 <= s < len(w)
    hold, inside = P.pv_span(a_f, m, s)
    assert hold.any() and (where != "chunk" or (hold[PV_CHUNK - 1] and hold[PV_CHUNK]))
    tol = 5e-5 if mode == "markers" else 2e-5
    for name, v in P.BAD.items():
        wb = w.copy()
        wb[s] = v
        ref = None
        if name == "nan":
            with np.errstate(invalid="ignore"):
                from test_gpu_pv_edges import LEVEL_MARKERS
                x = wb.astype(np.float64)
                ref = pvo.render(x, SR, LEVEL_MARKERS) if mode == "markers" else pvo.pitch_shift(x, float(mode.split()[0]))
        a = gpu_ctx.upload(wb)
        try:
            gpu_ctx.pv_set_chunk_frames(0)
            gpu_ctx.release_scratch()  # (an arena sized for this call, compact records)
            f32, i16 = _pv_run(gpu_ctx, a, mode)
            assert gpu_ctx.pv_last_chunks() == 1
            assert gpu_ctx.pv_arena_bytes() < 24.0 * 1024 * (len(a_f) + 64), (mode, where, name, "the record pool overflowed")
            P.check_pv_bad(f32, i16, clean[mode][0], inside, ref, tol, (mode, where, name))
            assert np.array_equal(_pv_run(gpu_ctx, a, mode, want_f32=False)[1], i16)
            gpu_ctx.pv_set_chunk_frames(PV_CHUNK)
            g32, g16 = _pv_run(gpu_ctx, a, mode)
            assert gpu_ctx.pv_last_chunks() >= 2
            assert g32.tobytes() == f32.tobytes() and g16.tobytes() == i16.tobytes(), (mode, where, name, "chunked")
        finally:
            gpu_ctx.pv_set_chunk_frames(0)
            gpu_ctx.release_scratch()
            a.free()


@pytest.mark.parametrize("where", ["mid", "seam 2", "seam 3"])
def test_pv_bad_sample_sharded_and_device_forms(gpu_ctx, mxlib, hip, pv_take, where):
    """+5 st with the bad sample mid-file and at the centre of the first frame of rank 1 of 2 / rank 2 of 3 (frames of both ranks
    hold it: phase totals, carry and both overlap-add seams carry non-finite data): ranks 2 and 3 on one device and the _dev
    form, inside guard bands, give the resident form's bytes."""
    import melonix_amd as mx
    from melonix_amd import shard as sh
    w, clean, taps = pv_take
    st, n = 5.0, len(w)
    a_f, _ = taps["+5 st"]
    s = {"mid": n // 2, "seam 2": int(a_f[mx.pv_shard_frames(n, st, 1, 2)[0]]), "seam 3": int(a_f[mx.pv_shard_frames(n, st, 2, 3)[0]])}[where]
    for name, v in P.BAD.items():
        wb = w.copy()
        wb[s] = v
        a = gpu_ctx.upload(wb)
        try:
            whole_f, whole_i = gpu_ctx.pv_pitch_shift(a, st)
            assert not np.isfinite(whole_f).all()
            gf, gi = Guarded(hip, 4 * n, 4), Guarded(hip, 2 * n, 2)
            try:
                gpu_ctx.pv_pitch_shift_dev(a, st, gf.ptr, gi.ptr)
                gpu_ctx.synchronize()
                assert gf.fetch().tobytes() == whole_f.tobytes() and gi.fetch().tobytes() == whole_i.tobytes(), (where, name, "dev")
            finally:
                gf.free()
                gi.free()
        finally:
            a.free()
        for world in (2, 3):
            ctxs = [mx.Context(0) for _ in range(world)]
            try:
                auds = [c.upload(wb) for c in ctxs]
                tots = [c.pv_shard_analyze(x, st, r, world) for r, (c, x) in enumerate(zip(ctxs, auds))]
                all_sums, all_org = np.stack([t[0] for t in tots]), np.stack([t[1] for t in tots])
                seams = [c.pv_shard_synthesize(sh.pv_fold_carry(all_sums, all_org, r) if r else None) for r, c in enumerate(ctxs)]
                parts_f, parts_i = [], []
                for r, c in enumerate(ctxs):
                    _, _, lo, hi = mx.pv_shard_frames(n, st, r, world)
                    f, i = c.pv_shard_finish(hi - lo, seams[r - 1][1] if r else None, seams[r + 1][0] if r < world - 1 else None)
                    parts_f.append(f)
                    parts_i.append(i)
                assert np.concatenate(parts_f).tobytes() == whole_f.tobytes(), (where, name, world)
                assert np.concatenate(parts_i).tobytes() == whole_i.tobytes(), (where, name, world)
                for x in auds:
                    x.free()
            finally:
                for c in ctxs:
                    c.close()


# ---- f0 tracker: the records the PSOLA renders are planned from --------------------------------------------------------------------

@pytest.mark.parametrize("name", list(P.BAD))
def test_f0_records_with_one_bad_sample(gpu_ctx, name):
    """mx_f0_track and mx_f0_candidates with one NaN / +-Inf sample at the four positions of tests/bad_samples.py (frame h holds
    [h hop - 2048, h hop + 2048)): the frames that do not hold it keep the clean take's bytes; the whole curve is the same bytes
    at runs of 1, 5, 32 frames and the default, and across a split behind the first holding frame; in a holding frame a slot is
    empty — {0, 0, 1, 0} — unless its d' is finite, the plain record is not voiced (aperiodicity not below the threshold: the
    PSOLA plan takes such a frame as unvoiced) and it is the one the candidates' launch writes."""
    import bad_samples as B
    from melonix_amd import F0_CAND_DTYPE, F0_DTYPE
    from test_gpu_psola import HOP, vowel
    w = vowel(1.0)
    n, ctx = len(w), gpu_ctx
    both = np.dtype([("track", F0_DTYPE), ("cands", F0_CAND_DTYPE, (4,))])

    def records(a):
        def fn(first, count, run):
            ctx.set_frames_per_block(run)
            try:
                out = np.empty(count, both)
                out["track"], out["cands"] = ctx.f0_candidates(a, SR, HOP, first, count)
                assert ctx.f0_track(a, SR, HOP, first, count).tobytes() == out["track"].tobytes()
                return out
            finally:
                ctx.set_frames_per_block(0)
        return fn

    frames = B.frame_count(n, HOP)
    a = ctx.upload(w)
    try:
        clean = records(a)(0, frames, 0)
    finally:
        a.free()
    assert (clean["track"]["tau"][8:-8] > 0).all()
    for pos, s in B.positions(n, HOP, 2048, 2048).items():
        hold = B.holding(n, HOP, 2048, 2048, s)
        b = ctx.upload(B.with_bad(w, s, P.BAD[name]))
        try:
            got = B.same_whatever_the_run_or_the_split(records(b), frames, hold, (name, pos))
        finally:
            b.free()
        assert hold.any() and got[~hold].tobytes() == clean[~hold].tobytes(), (name, pos, np.nonzero(~hold & (got["track"] != clean["track"]))[0])
        c = got["cands"][hold]
        filled = c["tau"] > 0
        assert np.isfinite(c["aperiodicity"][filled]).all() and np.isfinite(c["period"][filled]).all(), (name, pos)
        assert not (got["track"]["aperiodicity"][hold] < 0.15).any(), (name, pos, got["track"][hold])  # never voiced
        e = c[~filled]
        assert (e["tau"] == 0).all() and (e["period"] == 0).all() and (e["aperiodicity"] == 1).all() and (e["cents"] == 0).all(), (name, pos)
        print(f"f0 {name} {pos}: {int(hold.sum())} holding frames, {int(filled.sum())} filled slots in them; plain records "
              f"tau {np.unique(got['track']['tau'][hold])[:6]}, aperiodicity {np.unique(got['track']['aperiodicity'][hold])[:6]}, rms {np.unique(got['track']['rms'][hold])[:4]}")
