"""The tempo estimator without a GPU (include/melonix_amd.h "Tempo and grid-offset estimation"): the kernels' arithmetic
(csrc/tempo_core.h) and the library's host logic (csrc/tempo_logic.cpp) run on the CPU by tests/emu/tempo_emu.cpp against
tests/tempo_ref.py byte for byte; the reference alone against the truth of the synthetic takes; the refusals; the kernels'
resources."""
import ctypes as C

import numpy as np
import pytest

import emu_build
import onset_ref as R
import tempo_ref as T
from tempo_ref import same_estimate

EMU_SOURCES = ["tempo_emu.cpp", "tempo_logic.cpp"]


class Emu:
    def __init__(self, so):
        from melonix_amd import _capi

        self.capi, self.L = _capi, C.CDLL(so)
        self.L.emu_tempo_smooth.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        self.L.emu_tempo_comb.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        self.L.emu_tempo_comb.restype = None
        self.L.emu_tempo_check_params.argtypes = [C.POINTER(_capi.TempoParams)]
        self.L.emu_tempo_check_job.argtypes = [C.POINTER(_capi.CombJob), C.c_long]
        self.L.emu_tempo_check_ladder.argtypes = [C.POINTER(_capi.TempoParams), C.c_int, C.c_int]
        self.L.emu_tempo_estimate.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_long, C.POINTER(_capi.TempoParams), C.c_int,
                                              C.POINTER(_capi.Tempo), C.c_void_p, C.c_long, C.POINTER(C.c_long)]

    def params(self, **kw):
        return self.capi.TempoParams(**dict(T.TEMPO_DEFAULTS, **kw))

    def smooth(self, flux, W):
        flux = np.ascontiguousarray(flux, dtype=np.float32)
        out = np.empty(len(flux), dtype=np.float32)
        assert self.L.emu_tempo_smooth(flux.ctypes.data, len(flux), W, out.ctypes.data) == 0
        return out

    def comb(self, curve, jobs, threads=256):
        curve = np.ascontiguousarray(curve, dtype=np.float32)
        j = np.array([tuple(x) for x in jobs], dtype=self.capi.COMB_JOB_DTYPE)
        out = np.empty(len(j), dtype=self.capi.COMB_DTYPE)
        self.L.emu_tempo_comb(curve.ctypes.data, len(curve), j.ctypes.data, len(j), threads, out.ctypes.data)
        return out

    def estimate(self, flux, sr=T.SR, hop=T.HOP, first_frame=0, threads=256, **kw):
        flux = np.ascontiguousarray(flux, dtype=np.float32)
        t, win, n = self.capi.Tempo(), np.empty(4096, dtype=self.capi.TEMPO_WINDOW_DTYPE), C.c_long()
        p = self.params(**kw) if kw else None
        rc = self.L.emu_tempo_estimate(flux.ctypes.data, len(flux), sr, hop, first_frame, C.byref(p) if p else None, threads,
                                       C.byref(t), win.ctypes.data, len(win), C.byref(n))
        if rc:
            return None
        assert n.value <= len(win)
        return {k: getattr(t, k) for k, _ in self.capi.Tempo._fields_}, win[:n.value]


@pytest.fixture(scope="module")
def tempo_emu():
    return Emu(emu_build.shared_object("tempo_emu", EMU_SOURCES, ["tempo_core.h", "tempo_logic.h"]))


def test_smoothing_equals_the_reference(tempo_emu):
    rng = np.random.default_rng(3)
    for count in (1, 63, 64, 65, 767, 769):
        o = rng.gamma(0.6, 4.0, count).astype(np.float32)
        if count >= 63:
            o[[5, 17, 40]] = [np.nan, np.inf, -np.inf]
        for W in (0, 1, 4, 32):
            want = T.smooth(o, W)
            assert tempo_emu.smooth(o, W).tobytes() == want.tobytes(), (count, W)
            assert np.isfinite(want).all()
    o = np.array([1.0, np.nan, -np.inf, 3.0], np.float32)
    assert tempo_emu.smooth(o, 0).tolist() == [1.0, 0.0, 0.0, 3.0]  # W = 0: the sanitising copy


@pytest.mark.parametrize("kind", T.COMB_CURVES)
def test_comb_equals_the_reference_whatever_the_thread_mapping(tempo_emu, kind):
    for count in T.COMB_COUNTS:
        e, jobs, want = T.comb_case(kind, count)
        want = T.records_array(want, tempo_emu.capi.COMB_DTYPE)
        for threads in (256, 7):
            assert tempo_emu.comb(e, jobs, threads).tobytes() == want.tobytes(), (kind, count, threads)
        if kind == "zeros":
            assert not want.view(np.uint8).any()  # {0, 0, 0, 0}
        if kind == "constant":
            assert (want["phase"] == 0).all() and (want["score"] == 2.0).all()  # ties: the lowest phase
        if kind == "spike" and count >= 65:
            # the whole curve at period 45.0: only phase s mod 45 meets the spike, its neighbours meet zeros
            i = jobs.index((0, count, 45 << 16))
            s = T.spike_frame(count)
            J = (count - 1 - s % 45) // 45 + 1
            r = want[i]
            assert (int(r["phase"]), float(r["prev"]), float(r["next"])) == (s % 45, 0.0, 0.0)
            assert r["score"] == np.float32(float(T.SPIKE) / J)
    # a segment shorter than its period: the phases beyond it have J = 0 and score 0
    e, _, _ = T.comb_case(kind, 257)
    s = T.comb_scores(e, 3, 10, 45 << 16)
    assert len(s) == 45 and not s[10:].any()


@pytest.mark.parametrize("name", list(T.TAKES))
def test_estimate_equals_the_reference_on_the_takes(tempo_emu, name):
    res, windows, _ = T.take_estimate(name)
    same_estimate(tempo_emu.estimate(T.take_flux(name)), (res, windows))
    same_estimate(tempo_emu.estimate(T.take_flux(name), threads=5), (res, windows))


def test_estimate_with_many_windows_a_first_frame_and_other_rates(tempo_emu):
    flux = T.take_flux("bpm100_jitter")
    kw = dict(window_frames=512, stride_frames=128)
    want = T.estimate(flux, T.SR, T.HOP, **kw)
    assert len(want[1]) == (len(flux) - 512) // 128 + 1 > 10
    same_estimate(tempo_emu.estimate(flux, **kw), want)
    # first_frame shifts the offset by first_frame * hop / sr modulo the beat, and the window curve's frames with it
    base = T.take_estimate("bpm100_jitter")[0]
    want = T.estimate(flux, T.SR, T.HOP, first_frame=1000)
    same_estimate(tempo_emu.estimate(flux, first_frame=1000), want)
    g = 60.0 / base["bpm"]
    assert want[0]["bpm"] == base["bpm"]
    d = (want[0]["offset"] - base["offset"] - 1000 * T.HOP / T.SR) % g
    assert min(d, g - d) < 1e-9
    # other parameters, a curve shorter than a window, another hop and rate
    kw = dict(bpm_min=60.0, bpm_max=200.0, per_octave=24, smooth=0, prior_bpm=90.0, prior_octaves=0.5, lock_ratio=1.0)
    same_estimate(tempo_emu.estimate(flux[:1500], 44100, 512, **kw), T.estimate(flux[:1500], 44100, 512, **kw))
    # nothing to find: the empty result, and no error
    for empty in (np.zeros(0, np.float32), np.zeros(3000, np.float32), np.full(100, np.nan, np.float32)):
        res, win = tempo_emu.estimate(empty)
        assert len(win) == 0 and res == dict(bpm=0.0, offset=0.0, score=0.0, clarity=0.0, locked_frames=0, levels=0)
        same_estimate((res, win), T.estimate(empty, T.SR, T.HOP))


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same sources with a main of their own over the smallest shapes, under AddressSanitizer and UBSan."""
    out = emu_build.run_sanitized(tmp_path, "tempo_emu_san", EMU_SOURCES, "TEMPO_EMU_MAIN")
    assert "tempo_emu ok" in out, out


@pytest.mark.parametrize("name", list(T.TAKES))
def test_the_reference_finds_the_true_grid(name):
    """The reference alone against the truth.  An onset snaps to the right line while the grid is less than half a step off; this
    asks for a quarter step at division 4, g = 60 / (bpm * 4), over the whole take:
    |offset error modulo the beat| + take length * |bpm error| / bpm < g / 4 — a bound from the use, not from a measurement."""
    res, _, details = T.take_estimate(name)
    off, rel, length = T.grid_error(name, res)
    g = 60.0 / (T.TAKES[name]["bpm"] * 4)
    print(f"{name}: {res['bpm']:.4f} bpm, offset error {off * 1e3:.2f} ms, drift {length * rel * 1e3:.2f} ms, bound {g / 4 * 1e3:.1f} ms, "
          f"clarity {float(res['clarity']):.2f}, levels {details['levels']}")
    assert off + length * rel < g / 4
    # the two best aggregated candidates are far apart: a last-place difference in the prior cannot change c*
    A = sorted(details["A"], reverse=True)
    assert (A[0] - A[1]) / A[0] > 1e-9
    assert float(res["clarity"]) > 4.0


def test_the_reference_chain_lands_on_the_true_grid():
    """What tests/test_gpu_tempo.py asks of the GPU, first of the definitions alone: the 100 bpm take -> tempo_ref.estimate ->
    onset_ref.pick -> onset_ref.timing_markers at its bpm and offset, division 4 -> psola_ref's render over yin_ref's track ->
    onset_ref again: as many onsets as before, each within +-4 frames of a line of the TRUE grid."""
    import psola_ref as P
    import yin_ref as Y

    name = "bpm100_jitter"
    w, args = T.take_wave(name), T.TAKES[name]
    res = T.take_estimate(name)[0]
    onsets = R.pick(T.take_flux(name), T.HOP)
    markers = R.timing_markers([o[0] for o in onsets], len(w), T.SR, bpm=res["bpm"], offset=res["offset"], division=4)
    recs, _ = Y.track(w, T.SR, T.HOP)
    track = np.zeros(len(recs), dtype=[("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])
    for i, r in enumerate(recs):
        track[i] = r
    grains, length = P.plan(len(w), T.SR, T.HOP, track, markers)
    y = P.render(w.astype(np.float64), grains, length).astype(np.float32)
    again = R.pick(R.flux(y, T.SR, T.HOP).astype(np.float32), T.HOP)
    g, line = 60.0 / (args["bpm"] * 4), args.get("lead", 0.0) + 0.25
    dist = [abs(((o[0] / T.SR - line + g / 2) % g) - g / 2) * T.SR / T.HOP for o in again]
    print("frames off the true grid:", np.round(dist, 2).tolist())
    assert len(again) == len(onsets) >= 15 and max(dist) <= 4


def test_the_long_take_refines_twice_from_a_later_anchor():
    res, _, details = T.take_estimate("bpm87_after_silence")
    assert details["anchor"] > 0 and res["levels"] == 2 and res["locked_frames"] == len(T.take_flux("bpm87_after_silence"))
    assert details["levels"][0][1] == 2048


def test_clarity_of_steady_noise_is_about_one():
    res, _ = T.estimate(R.flux(R.noise(), T.SR, T.HOP).astype(np.float32), T.SR, T.HOP)
    print(f"noise: clarity {float(res['clarity']):.3f}")
    assert float(res["clarity"]) < 1.5


def test_refusals(tempo_emu, mxlib):
    """Every parameter outside its range, a period outside the Q16 range, a segment outside the curve: the checks the entry
    points run before any launch (tempo_logic.cpp); and what the C-ABI refuses before it looks at its context."""
    E = tempo_emu
    assert E.L.emu_tempo_check_params(C.byref(E.params())) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(bpm_min=29.9), dict(bpm_max=250.1), dict(bpm_min=120.0, bpm_max=120.0), dict(bpm_min=200.0, bpm_max=100.0),
                dict(bpm_min=nan), dict(bpm_max=nan), dict(per_octave=7), dict(per_octave=129), dict(smooth=-1), dict(smooth=33),
                dict(window_frames=63), dict(window_frames=65537), dict(stride_frames=0), dict(stride_frames=2049),
                dict(prior_bpm=0.0), dict(prior_bpm=inf), dict(prior_bpm=nan), dict(prior_octaves=0.0), dict(prior_octaves=-1.0),
                dict(prior_octaves=inf), dict(lock_ratio=-0.01), dict(lock_ratio=1.01), dict(lock_ratio=nan)):
        assert E.L.emu_tempo_check_params(C.byref(E.params(**bad))) == -1, bad
        assert E.estimate(np.ones(100, np.float32), **bad) is None, bad
    # a candidate period outside [2, 4096] frames: 250 bpm at 4 frames per second, 30 bpm at 3000
    assert E.L.emu_tempo_check_ladder(C.byref(E.params()), 48000, 256) == 0
    for sr, hop in ((48000, 12000), (48000, 16), (0, 256), (48000, 0), (48000, 16385)):
        assert E.L.emu_tempo_check_ladder(C.byref(E.params()), sr, hop) == -1, (sr, hop)
        assert T.ladder(sr, hop) is None if sr > 0 and 0 < hop <= 16384 else True
    job = E.capi.CombJob
    for ok in ((0, 100, 2 << 16), (99, 1, 4096 << 16), (10, 90, 45 << 16)):
        assert E.L.emu_tempo_check_job(C.byref(job(*ok)), 100) == 0, ok
    for bad in ((0, 0, 45 << 16), (0, -1, 45 << 16), (-1, 10, 45 << 16), (0, 101, 45 << 16), (100, 1, 45 << 16), (50, 51, 45 << 16),
                (2 ** 31 - 1, 2 ** 31 - 1, 45 << 16), (0, 100, (2 << 16) - 1), (0, 100, (4096 << 16) + 1), (0, 100, 0)):
        assert E.L.emu_tempo_check_job(C.byref(job(*bad)), 100) == -1, bad
    assert E.L.emu_tempo_check_job(C.byref(job(0, 1, 45 << 16)), 0) == -1  # count 0: no segment fits
    # the C-ABI: null arguments are MX_ERR_INVALID, with or without a device
    L = E.capi.lib()
    t, f = E.capi.Tempo(), np.ones(8, np.float32)
    assert L.mx_tempo_smooth(None, f.ctypes.data, 8, 4, f.ctypes.data) == -1
    assert L.mx_tempo_smooth_dev(None, None, 8, 4, None) == -1
    assert L.mx_tempo_comb(None, None, 0, None, 0, None) == -1
    assert L.mx_tempo_comb_dev(None, None, 0, None, 0, None) == -1
    assert L.mx_tempo_from_flux(None, f.ctypes.data, 8, 48000, 256, 0, None, C.byref(t), None, None) == -1
    assert L.mx_tempo_detect(None, None, 48000, 256, None, None, C.byref(t), None, None) == -1
    L.mx_tempo_params_default(None)  # (nothing to write to: nothing happens)
    assert mxlib.tempo_params_default() == T.TEMPO_DEFAULTS


def test_tempo_kernels_do_not_spill():
    """Both kernels are scratch-free and inside 256 VGPRs; the comb's LDS is its row of 4096 scores and the four waves' pairs."""
    names, scratch, vgprs, lds = emu_build.resource_usage("tempo_kernels.hip")
    lds = dict(zip(names, lds))
    print(list(zip(names, scratch, vgprs)), lds)
    assert len(names) == 2
    assert any("tempo_smooth_kernel" in n for n in names) and any("tempo_comb_kernel" in n for n in names)
    assert scratch == [0, 0] and max(vgprs) <= 256
    assert [v for n, v in lds.items() if "tempo_comb_kernel" in n] == [4096 * 4 + 32]
