"""The resynthesis launch's grid, whatever maps its blocks onto the steps and whichever blocks zero the samples past the last
step's run (a block per step and a tail launch today; an XCD-contiguous map with the tail folded in was measured and
withdrawn, HISTORY.md).  Step counts around the eight XCD shares (fewer than 8 leave empty shares, 9 and 17 are no multiples
of 8) and the whole schedule of a 3 s take (about a hundred steps), both kernels (16-byte aligned PCM pointers, and PCM
pointers one sample off, which take the scalar kernel), int16 alone and int16 + f32, tails of 1 / 1 500 / 100 000 samples.
The PCM of the first k steps of a schedule is the first sum(sz) samples of the oracle's export, bit for bit; everything from
there to nsamples is zero; the bytes around the buffers stay as they were."""
import numpy as np
import pytest

from conftest import SR, DevBuf, accum_sweep

pytestmark = pytest.mark.gpu

GUARD = 4096          # samples watched after nsamples (and the one-sample offset before the pointer)
TAILS = (1, 1500, 100000)
FILL = 0x7F


@pytest.fixture(scope="module")
def take(gpu_ctx, oracle, mxlib):
    """3 s of the sweep at +3 st and -5 st: the schedules from the device grain table, the oracle's PCM, device buffers."""
    w = accum_sweep(3 * SR)
    n = len(w)
    a = gpu_ctx.upload(w)
    s, l, f = gpu_ctx.grain_table_dev(a)
    runs = {}
    for pb in (3.0, -5.0):
        mk = [(1, 0, 0, pb), (n - 1, 0, 0, pb)]
        steps, total, _ = mxlib.schedule_build_table(n, SR, s, l, f, mk)
        osteps, opcm = oracle.export_run(w, SR, mk)
        assert total == len(opcm) and len(steps) == len(osteps)
        for name in ("grain_start", "grain_len", "rate", "next_first", "sz", "out_offset"):
            assert np.array_equal(steps[name], osteps[name]), name
        runs[pb] = (steps, opcm, oracle.pcm_to_i16(opcm))
    most = max(len(r[1]) for r in runs.values()) + max(TAILS) + GUARD + 8
    bufs = (DevBuf(max(len(r[0]) for r in runs.values()) * runs[3.0][0].itemsize), DevBuf(most * 4), DevBuf(most * 2))
    yield a, runs, bufs
    for b in bufs:
        b.free()
    a.free()


def render(gpu_ctx, take, pb, k, extra, want_f32, off):
    """mx_resynth_dev of the first k steps into buffers filled with FILL bytes, the PCM pointers `off` samples into them ->
    (f32 | None, i16: everything from the buffer's start to GUARD samples past nsamples, covered, nsamples)."""
    a, runs, (d_steps, d_f, d_i) = take
    steps = runs[pb][0][:k]
    covered = int(steps["sz"].sum())
    nsamples = covered + extra
    span = off + nsamples + GUARD
    if k:
        d_steps.write(steps)
    for b, size in ((d_f, 4), (d_i, 2)):
        assert b.hip.hipMemset(b.ptr, FILL, span * size) == 0
    gpu_ctx.resynth_dev(a, d_steps.ptr, k, nsamples, d_f.ptr + 4 * off if want_f32 else None, d_i.ptr + 2 * off)
    gpu_ctx.synchronize()
    return (d_f.read(np.uint32, 0, span) if want_f32 else None), d_i.read(np.int16, 0, span), covered, nsamples


@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 17, None])
@pytest.mark.parametrize("pb", [3.0, -5.0])
def test_first_k_steps_bit_exact_tail_zero_guard_untouched(gpu_ctx, take, pb, k):
    steps, opcm, o16 = take[1][pb]
    k = len(steps) if k is None else k
    assert 17 < len(steps)
    fill32, fill16 = np.uint32(0x7F7F7F7F), np.int16(0x7F7F)
    for off in (0, 1):  # 1: the PCM pointers are not 16-byte aligned -> resynth_kernel
        for want_f32 in (False, True):
            for extra in TAILS:
                f32, i16, covered, nsamples = render(gpu_ctx, take, pb, k, extra, want_f32, off)
                what = (pb, k, off, want_f32, extra)
                assert covered == (int(steps["out_offset"][k - 1] + steps["sz"][k - 1]) if k else 0)
                assert np.array_equal(i16[off:off + covered], o16[:covered]), what
                assert not i16[off + covered:off + nsamples].any(), what
                assert (i16[:off] == fill16).all() and (i16[off + nsamples:] == fill16).all(), what
                if want_f32:
                    assert np.array_equal(f32[off:off + covered], opcm[:covered].view(np.uint32)), what
                    assert not f32[off + covered:off + nsamples].any(), what
                    assert (f32[:off] == fill32).all() and (f32[off + nsamples:] == fill32).all(), what


def test_no_steps_is_the_memset_path(gpu_ctx, take):
    """nsteps = 0: no kernel runs (there is no last step to read), the outputs are cleared by the memset."""
    for extra in TAILS:
        f32, i16, covered, nsamples = render(gpu_ctx, take, 3.0, 0, extra, True, 0)
        assert covered == 0 and nsamples == extra
        assert not f32[:extra].any() and not i16[:extra].any()
        assert (f32[extra:] == np.uint32(0x7F7F7F7F)).all() and (i16[extra:] == np.int16(0x7F7F)).all()
