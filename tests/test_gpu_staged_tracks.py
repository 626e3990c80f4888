"""The host forms of the per-frame tracks (f0, candidates, decode, onset strength) pass through the same staging buffers of
their context, one after the other: the onset strength takes the pitch records' buffer at 4 bytes per frame right after the
tracker used it at 16, and the reverse.  Each result is the bytes of the same call on a fresh context and of its device form."""
import numpy as np
import pytest

from conftest import SR, DevBuf, accum_sweep, noisy

pytestmark = pytest.mark.gpu

HOP, FRAMES = 256, 8


def _bytes(res):
    return [r.tobytes() for r in (res if isinstance(res, tuple) else (res,))]


def _dev(ctx, a, sizes, queue):
    """The bytes that queue(ctx, a, *device pointers) leaves in fresh device buffers of `sizes` bytes per frame."""
    bufs = [DevBuf(FRAMES * s, fill=0xA5) for s in sizes]
    try:
        queue(ctx, a, *[b.ptr for b in bufs])
        ctx.synchronize()
        return [b.read(np.uint8).tobytes() for b in bufs]
    finally:
        for b in bufs:
            b.free()


def test_host_forms_share_the_staging_slots_in_sequence(mxlib):
    w = noisy(accum_sweep(2000))
    assert mxlib.frame_count(len(w), HOP) == FRAMES
    first = {}  # the first call's track and candidates: what the last call decodes

    def candidates(c, a):
        return c.f0_candidates(a, SR, HOP)

    def decode(c, a):
        return c.f0_decode(*first["ladder"])

    def dev_candidates(c, a, d_track, d_cands):
        c.f0_candidates_dev(a, SR, HOP, 0, FRAMES, d_track, d_cands)

    def dev_track_decoded(c, a, d_track, d_cands):
        dev_candidates(c, a, d_track, d_cands)
        c.f0_decode_dev(d_track, d_cands, FRAMES, d_track)

    def dev_decode(c, a, d_track, d_cands, d_out, d_state):
        dev_candidates(c, a, d_track, d_cands)
        c.f0_decode_dev(d_track, d_cands, FRAMES, d_out, d_state)

    # (name, the host form, the device form's buffer sizes per frame, the device form, which of its buffers are the result)
    calls = [("f0_candidates", candidates, (16, 64), dev_candidates, (0, 1)),
             ("onset_flux", lambda c, a: c.onset_flux(a, SR, HOP), (4,), lambda c, a, d: c.onset_flux_dev(a, SR, HOP, 0, FRAMES, d), (0,)),
             ("f0_track_decoded", lambda c, a: c.f0_track_decoded(a, SR, HOP), (16, 64), dev_track_decoded, (0,)),
             ("onset_flux lag 4", lambda c, a: c.onset_flux(a, SR, HOP, lag=4), (4,),
              lambda c, a, d: c.onset_flux_dev(a, SR, HOP, 0, FRAMES, d, lag=4), (0,)),
             ("f0_track", lambda c, a: c.f0_track(a, SR, HOP), (16,), lambda c, a, d: c.f0_track_dev(a, SR, HOP, 0, FRAMES, d), (0,)),
             ("f0_decode", decode, (16, 64, 16, 1), dev_decode, (2, 3))]
    one = mxlib.Context(0)
    a = one.upload(w)
    try:
        for name, host, sizes, dev, keep in calls:
            got = host(one, a)
            if name == "f0_candidates":
                first["ladder"] = got
            assert all(len(r) == FRAMES for r in (got if isinstance(got, tuple) else (got,))), name
            fresh = mxlib.Context(0)
            b = fresh.upload(w)
            try:
                assert _bytes(host(fresh, b)) == _bytes(got), name
                there = _dev(fresh, b, sizes, dev)
                assert [there[k] for k in keep] == _bytes(got), name
            finally:
                b.free()
                fresh.close()
        whole_track, whole_flux = one.f0_track(a, SR, HOP), one.onset_flux(a, SR, HOP)
        for form, whole in ((one.f0_track, whole_track), (one.onset_flux, whole_flux)):
            assert len(form(a, SR, HOP, 0, 0)) == 0 and len(form(a, SR, HOP, 7, 0)) == 0
            last = form(a, SR, HOP, 7, 1)
            assert len(last) == 1 and last.dtype == whole.dtype
        assert one.onset_flux(a, SR, HOP, 7, 1).tobytes() == whole_flux[7:].tobytes()
    finally:
        a.free()
        one.close()
