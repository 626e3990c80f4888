"""The job-list calls (combs, chroma sums, contour spans, key detection) share one pair of job buffers of their context, and every
family's kept work memory has one form: a job buffer grown and left dirty by another family changes nothing, and every set works
again after release_scratch.  Each result is the bytes the device forms leave in fresh buffers on a fresh context.  Calls with no
jobs or no frames, in between, return what they always returned."""
import numpy as np
import pytest

from conftest import SR, DevBuf, accum_sweep, noisy

pytestmark = pytest.mark.gpu

HOP, FRAMES = 256, 32
SPLIT = dict(half_width=2, lag_min=1, lag_max=4)


def _dev(ctx, arrays, out_bytes, queue):
    """The bytes queue(*device pointers of the inputs, *device pointers of the outputs) leaves in fresh 0xA5-filled output buffers."""
    ins = [DevBuf(max(a.nbytes, 1)) for a in arrays]
    outs = [DevBuf(nb, fill=0xA5) for nb in out_bytes]
    try:
        for buf, a in zip(ins, arrays):
            if a.nbytes:
                buf.write(a)
        queue(*[b.ptr for b in ins], *[b.ptr for b in outs])
        ctx.synchronize()
        return [b.read(np.uint8).tobytes() for b in outs]
    finally:
        for b in ins + outs:
            b.free()


def test_job_lists_and_work_memory_in_sequence(mxlib):
    w = noisy(accum_sweep(FRAMES * HOP))
    assert mxlib.frame_count(len(w), HOP) == FRAMES
    one, ref = mxlib.Context(0), mxlib.Context(0)
    a, b = one.upload(w), ref.upload(w)
    try:
        # the inputs, made once on the second context
        curve = ref.tempo_smooth(ref.onset_flux(b, SR, HOP))
        chroma = ref.chroma(b, SR, HOP)
        track, cands = ref.f0_candidates(b, SR, HOP)
        cents = (1600 * 60 + 40 * np.sin(np.arange(FRAMES)) * np.arange(FRAMES)).astype(np.int32)  # (every frame voiced)
        spans = mxlib._capi.records([(0, 10), (10, 8), (20, 12)], mxlib.CONTOUR_SPAN_DTYPE)
        combs = mxlib._capi.records([(j % 8, FRAMES - j % 8 - j % 5, (2 << 16) + 1009 * j) for j in range(300)], mxlib.COMB_JOB_DTYPE)
        sums = mxlib._capi.records([(j % FRAMES, (7 * j) % (FRAMES - j % FRAMES + 1)) for j in range(300)], mxlib.CHROMA_JOB_DTYPE)
        assert len(curve) == len(chroma) == len(track) == FRAMES

        def comb_there(jobs):
            return _dev(ref, [curve, jobs], [len(jobs) * mxlib.COMB_DTYPE.itemsize],
                        lambda d_curve, d_jobs, d_out: ref.tempo_comb_dev(d_curve, FRAMES, d_jobs, len(jobs), d_out))[0]

        def sums_there(jobs):
            return _dev(ref, [chroma, jobs], [len(jobs) * mxlib.CHROMA_COLS * 8],
                        lambda d_rec, d_jobs, d_out: ref.chroma_sum_dev(d_rec, FRAMES, d_jobs, len(jobs), d_out))[0]

        def split_there():
            return _dev(ref, [cents, spans], [FRAMES * mxlib.CONTOUR_REC_DTYPE.itemsize, len(spans) * mxlib.CONTOUR_STAT_DTYPE.itemsize],
                        lambda d_cents, d_spans, d_rec, d_stat: ref.contour_split_dev(d_cents, FRAMES, d_spans, len(spans), d_rec, d_stat, **SPLIT))

        def nothing_to_do():
            """No jobs, no frames: empty results (sums over no records are zeros), every frame outside every span."""
            assert len(one.tempo_comb(curve, [])) == 0 and len(one.tempo_comb([], [])) == 0 and len(one.tempo_smooth([])) == 0
            assert one.chroma_sum(chroma, []).shape == (0, mxlib.CHROMA_COLS)
            none = one.chroma_sum(np.empty((0, mxlib.CHROMA_COLS), np.float32), [(0, 0), (0, 0)])
            assert none.shape == (2, mxlib.CHROMA_COLS) and not none.any() and not np.signbit(none).any()
            rec, stat = one.contour_split(cents, [], **SPLIT)
            assert len(stat) == 0 and (rec["smooth"] == mxlib.CONTOUR_NONE).all() and not rec["vib"].any()
            rec, stat = one.contour_split([], [], **SPLIT)
            assert len(rec) == 0 and len(stat) == 0
            out, state = one.f0_decode(track[:0], cands[:0])
            assert len(out) == 0 and len(state) == 0

        assert one.tempo_comb(curve, combs).tobytes() == comb_there(combs)
        nothing_to_do()
        assert one.chroma_sum(chroma, sums[:1]).tobytes() == sums_there(sums[:1])
        rec_there, stat_there = split_there()
        rec, stat = one.contour_split(cents, spans, want_rec=False, **SPLIT)
        assert rec is None and stat.tobytes() == stat_there
        rec, stat = one.contour_split(cents, spans, **SPLIT)
        assert rec.tobytes() == rec_there and stat.tobytes() == stat_there
        nothing_to_do()
        assert one.tempo_comb(curve, combs[:1]).tobytes() == comb_there(combs[:1])

        # key detection: the take's records and the sums of its windows through the device forms, the estimates from those sums
        key, windows = one.key_detect(a, SR, HOP, window_frames=8, window_hop=4)
        assert len(windows) > 1
        jobs = mxlib._capi.records([(int(x["first_frame"]), int(x["frames"])) for x in windows] + [(0, FRAMES)], mxlib.CHROMA_JOB_DTYPE)
        d_rec = DevBuf(chroma.nbytes, fill=0xA5)
        try:
            ref.chroma_dev(b, SR, HOP, 0, FRAMES, d_rec.ptr)
            ref.synchronize()
            assert d_rec.read(np.uint8).tobytes() == chroma.tobytes()
        finally:
            d_rec.free()
        there = np.frombuffer(sums_there(jobs), dtype=np.float64).reshape(len(jobs), mxlib.CHROMA_COLS)
        assert key == mxlib.key_from_chroma(there[-1])
        for x, s in zip(windows, there):
            want = mxlib.key_from_chroma(s)
            assert {k: x["key"][k].item() for k in want} == want

        one.release_scratch()
        assert one.chroma_sum(chroma, sums).tobytes() == sums_there(sums)
        nothing_to_do()
        out, state = one.f0_decode(track, cands)
        there = _dev(ref, [track, cands], [track.nbytes, FRAMES],
                     lambda d_track, d_cands, d_out, d_state: ref.f0_decode_dev(d_track, d_cands, FRAMES, d_out, d_state))
        assert [out.tobytes(), state.tobytes()] == there
        # ... and every family once more after another release
        one.release_scratch()
        assert one.tempo_comb(curve, combs).tobytes() == comb_there(combs)
        rec, stat = one.contour_split(cents, spans, **SPLIT)
        assert rec.tobytes() == rec_there and stat.tobytes() == stat_there
    finally:
        a.free()
        b.free()
        one.close()
        ref.close()
