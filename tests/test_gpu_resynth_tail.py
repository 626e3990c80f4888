"""The samples past the last step's run — the zeros of the terminating process() call — whatever the last step is: a vector
run, a run shorter than one 8-sample vector, a fallback grain too long for the LDS stage (grain_len > 2304), in the vector
kernel and in the scalar one (PCM pointers that are not 16-byte aligned).  Today a launch of its own writes them from the last
step record; a form in which the last step's workgroup writes them after its run was measured (profiles/ab_hoist_tail.log)
and is not in the tree.  The test holds for either.

k = 1, 2 and 9 consecutive steps of a real schedule, their out_offset rebased to 0: the schedule's first k; k that end in a step
cut to 5 samples; k that end in a fallback grain.  PCM pointers 0 .. 8 samples into 16-byte aligned allocations (0 and 8: the
vector kernel), int16 alone and with f32, nsamples = covered + 1500 and nsamples = covered (no tail).  The buffers start as
0x5A bytes; the PCM is the oracle's export of the same steps bit for bit, the tail is zero, and everything before the pointer
and past nsamples is still 0x5A."""
import numpy as np
import pytest

from conftest import SR, DevBuf

pytestmark = pytest.mark.gpu

GUARD = 2048  # samples watched after nsamples
FILL = 0x5A
KS = (1, 2, 9)
LDS_GRAIN = 2304


@pytest.fixture(scope="module")
def take(gpu_ctx, oracle, mxlib):
    """6 s with a second without a negative sample and a flat stretch (fallback grains among ordinary ones) at +3 st: the
    schedule, the oracle's PCM, the windows of steps per case, device buffers."""
    n = 6 * SR
    t = np.arange(n) / SR
    w = (0.3 * np.sin(2 * np.pi * 220 * t)).astype(np.float32)
    w[SR:2 * SR] = np.abs(w[SR:2 * SR]) + 0.01
    w[3 * SR:3 * SR + 9000] = 0.2
    a = gpu_ctx.upload(w)
    s, l = gpu_ctx.grains_dev(a)
    mk = [(1, 0, 0, 3.0), (n - 1, 0, 0, 3.0)]
    steps, total = mxlib.schedule_build(w, SR, s, l, mk)
    osteps, opcm = oracle.export_run(w, SR, mk)
    assert total == len(opcm) and len(steps) == len(osteps) and total == int(steps["sz"].sum()) + 1500
    for name in ("grain_start", "grain_len", "rate", "next_first", "sz", "out_offset"):
        assert np.array_equal(steps[name], osteps[name]), name
    long_ones = np.flatnonzero((steps["grain_len"] > LDS_GRAIN) & (steps["sz"] > 0))
    assert len(long_ones) and long_ones[-1] >= max(KS) and (steps["grain_len"][:max(KS)] <= LDS_GRAIN).all()
    assert (steps["sz"][:max(KS)] >= 8).all()
    cases = {}
    for k in KS:
        cases["first", k] = (0, k, None)
        cases["short", k] = (0, k, 5)                         # the last step cut to 5 samples: less than one vector
        cases["fallback", k] = (int(long_ones[-1]) - k + 1, k, None)  # the last step is a fallback grain
    most = int(steps["sz"].max()) * max(KS) + 1500 + GUARD + 16
    bufs = (DevBuf(max(KS) * steps.itemsize), DevBuf(most * 4), DevBuf(most * 2))
    yield a, steps, opcm, oracle.pcm_to_i16(opcm), cases, bufs
    for b in bufs:
        b.free()
    a.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["first", "short", "fallback"])
def test_tail_after_any_kind_of_last_step(gpu_ctx, take, kind, k):
    a, all_steps, opcm, o16, cases, (d_steps, d_f, d_i) = take
    i0, k, cut = cases[kind, k]
    steps = all_steps[i0:i0 + k].copy()
    src0 = int(steps["out_offset"][0])  # where these steps' samples lie in the oracle's export
    steps["out_offset"] -= src0
    if cut is not None:
        steps["sz"][-1] = cut
    if kind == "fallback":
        assert steps["grain_len"][-1] > LDS_GRAIN
    covered = int(steps["out_offset"][-1] + steps["sz"][-1])
    d_steps.write(steps)
    fill32, fill16 = np.uint32(0x5A5A5A5A), np.int16(0x5A5A)
    for off in range(9):
        for want_f32 in (False, True):
            for extra in (1500, 0):
                nsamples = covered + extra
                span = off + nsamples + GUARD
                for b, size in ((d_f, 4), (d_i, 2)):
                    assert b.hip.hipMemset(b.ptr, FILL, span * size) == 0
                assert d_i.hip.hipDeviceSynchronize() == 0  # the fill runs on the null stream, the kernel on the context's own
                gpu_ctx.resynth_dev(a, d_steps.ptr, k, nsamples, d_f.ptr + 4 * off if want_f32 else None, d_i.ptr + 2 * off)
                gpu_ctx.synchronize()
                what = (kind, k, off, want_f32, extra)
                i16 = d_i.read(np.int16, 0, span)
                assert np.array_equal(i16[off:off + covered], o16[src0:src0 + covered]), what
                assert not i16[off + covered:off + nsamples].any(), what
                assert (i16[:off] == fill16).all() and (i16[off + nsamples:] == fill16).all(), what
                f32 = d_f.read(np.uint32, 0, span)
                if want_f32:
                    assert np.array_equal(f32[off:off + covered], opcm[src0:src0 + covered].view(np.uint32)), what
                    assert not f32[off + covered:off + nsamples].any(), what
                    assert (f32[:off] == fill32).all() and (f32[off + nsamples:] == fill32).all(), what
                else:
                    assert (f32 == fill32).all(), what
