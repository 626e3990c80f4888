"""Sibilant detection, protection and balance without a GPU (include/melonix_amd.h "Sibilant detection, protection and
balance"): the feature kernel's per-lane arithmetic (csrc/sibilant_core.h on onset_core.h's transform) and the gain's
(csrc/gain_core.h) run on the CPU by tests/emu/sibilant_emu.cpp against tests/sibilant_ref.py; mx_sibilants,
mx_formant_protect and mx_sibilant_gain_points of the library against the reference field for field; the refusals; the
kernels' resources; the reference alone against the truth of the synthetic take."""
import ctypes as C

import numpy as np
import pytest

import bad_samples as B
import emu_build
import onset_ref as R
import sibilant_ref as S

SR, HOP = S.SR, S.HOP
FLOAT_FIELDS = ("low", "high", "centroid")


def feature_bounds(ref):
    """The project's f32-versus-f64 yardstick per field, on the field's own maximum over the take; the floor is for energies
    (1e-8 on the noise bed), not for values of order 1."""
    return {k: 2e-5 * np.abs(ref[k]).max() + 1e-12 for k in FLOAT_FIELDS}


def check_features(got, ref, what):
    assert len(got) == len(ref)
    assert np.array_equal(got["zero_crossings"], ref["zero_crossings"]), what
    worst = 0.0
    for k, bound in feature_bounds(ref).items():
        err = np.abs(got[k].astype(np.float64) - ref[k]).max() if len(ref) else 0.0
        print(f"{what}: {k} max {np.abs(ref[k]).max():.4g}  worst error {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (what, k)
        worst = max(worst, err / bound)
    return worst


@pytest.fixture(scope="module")
def takes():
    """name -> (samples, reference features): the synthetic take and onset_ref's six signals; computed once, read by every test."""
    out = {"take": S.take()[0]}
    out.update({k: v[0] for k, v in R.signals().items()})
    res = {}
    for k, w in out.items():
        ref = S.features(w, SR, HOP)
        ref.setflags(write=False)
        res[k] = (w, ref)
    return res


@pytest.fixture(scope="module")
def emu(mxlib):
    L = C.CDLL(emu_build.shared_object("sibilant_emu", ["sibilant_emu.cpp"],
                                       ["onset_walk_emu.h", "onset_core.h", "sibilant_core.h", "gain_core.h"]))
    L.emu_sib_features.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.emu_audio_gain.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]

    class Emu:
        @staticmethod
        def features(w, hop, first, count, sr=SR, split_hz=3500.0, run=8):
            w = np.ascontiguousarray(w, dtype=np.float32)
            out = np.zeros(count, dtype=mxlib.SIB_FEAT_DTYPE)
            L.emu_sib_features(w.ctypes.data, len(w), hop, first, count, S.split_bin(sr, split_hz), run, out.ctypes.data)
            return out

        @staticmethod
        def gain(x, points):
            x = np.ascontiguousarray(x, dtype=np.float32)
            pts = np.array([(int(s), np.float32(a)) for s, a in points], dtype=mxlib.GAIN_POINT_DTYPE)
            out = np.zeros(len(x), dtype=np.float32)
            L.emu_audio_gain(x.ctypes.data, len(x), pts.ctypes.data, len(pts), out.ctypes.data)
            return out

    return Emu


@pytest.mark.parametrize("name", ["take", "notes5", "notes30", "legato", "vibrato", "noise", "clicks"])
def test_the_kernels_arithmetic_on_the_cpu(emu, takes, name):
    w, ref = takes[name]
    got = emu.features(w, HOP, 0, len(ref))
    worst = check_features(got, ref, name)
    print(f"{name}: worst error / bound {worst:.4f}")
    if name in ("take", "clicks"):  # the same bytes whatever the run length or the launch split
        for run in (1, 5, 32):
            assert emu.features(w, HOP, 0, len(ref), run=run).tobytes() == got.tobytes(), run
        assert emu.features(w, HOP, 37, 50, run=7).tobytes() == got[37:87].tobytes()
        assert emu.features(w, HOP, 5, 1, run=32).tobytes() == got[5:6].tobytes()


def test_edges_of_the_split_and_of_the_frame_on_the_cpu(emu, takes):
    w = takes["take"][0][:20000]
    for sr, split in ((SR, 3500.0), (44100, 3500.0), (SR, 1.0), (SR, 24000.0), (SR, 23999.0)):
        ref = S.features(w, sr, HOP, split)
        check_features(emu.features(w, HOP, 0, len(ref), sr, split), ref, f"sr {sr} split {split}")
    assert S.split_bin(SR, 1.0) == 1 and S.split_bin(SR, 24000.0) == 512 and S.split_bin(44100, 3500.0) == 82
    assert not emu.features(w, HOP, 0, 40, split_hz=1.0)["low"].any()
    assert not emu.features(w, HOP, 0, 40, split_hz=24000.0)["high"].any()
    # silence, -0 and NaN are "not negative"; a record of silence is all zeros
    z = np.zeros(3000, np.float32)
    z[100:200] = -0.0
    assert emu.features(z, 255, 0, 12).tobytes() == bytes(16 * 12)
    x = np.tile(np.array([1.0, -1.0], np.float32), 1500)
    x[700] = np.nan
    ref = S.features(x, SR, 256)
    got = emu.features(x, 256, 0, len(ref))
    assert np.array_equal(got["zero_crossings"], ref["zero_crossings"]) and got["zero_crossings"].max() == 1023
    for n, hop in ((1, 256), (255, 256), (767, 256), (769, 256), (300, 1), (2000, 255), (40000, 16384)):
        v = takes["noise"][0][:n]
        ref = S.features(v, SR, hop)
        assert len(ref) == -(-n // hop)
        check_features(emu.features(v, hop, 0, len(ref)), ref, f"n {n} hop {hop}")


BAD_TAKE = (14000, 30000)  # the synthetic take's samples: the end of the first vowel, the "s" and the next vowel's start


@pytest.mark.parametrize("name", list(B.BAD))
def test_a_bad_sample_on_the_cpu(emu, takes, name):
    """An Inf or NaN sample leaves the frames that hold it without a finite low + high; zero_crossings (NaN is "not negative",
    Inf has its sign) equals the reference on every frame; every other record keeps the clean take's bytes; the same bytes
    whatever the run or a split inside the affected frames (tests/bad_samples.py; tests/test_gpu_bad_samples.py asks the same
    of the device)."""
    w = takes["take"][0][BAD_TAKE[0]:BAD_TAKE[1]]
    n = len(w)
    for pos, s in B.positions(n, HOP, 512, 512).items():
        v = B.with_bad(w, s, B.BAD[name])
        with np.errstate(invalid="ignore"):
            zc = S.features(v, SR, HOP)["zero_crossings"]
        B.check_features(lambda first, count, run: emu.features(v, HOP, first, count, run=run or 8),
                         lambda first, count, run: emu.features(w, HOP, first, count, run=run or 8), zc, n, HOP, s, (name, pos))


def test_levels_scale_exactly_on_the_cpu(emu, takes):
    """The take times 2^k, k in -30, -8, 8, 30: low and high are the clean bytes times 2^2k, centroid and crossings the clean
    bytes (all four k hold on the emulation; 2^-40 and 2^40 do as well)."""
    w = takes["take"][0][BAD_TAKE[0]:BAD_TAKE[1]]
    frames = B.frame_count(len(w), HOP)
    clean = emu.features(w, HOP, 0, frames)
    assert clean["low"].all() and clean["high"].all()
    for k in B.SIB_SCALES + (-40, 40):
        B.check_scaled_features(emu.features(B.scaled(w, k), HOP, 0, frames), clean, k, "emulation")


SIB_CHAIN_NAN = 120 * HOP + 7  # inside the take's second vowel, 28 frames from the nearest sibilant


def segment_survivors(clean, bad, n, what):
    """clean / bad: sibilant_ref.segments lists (or the library's records as such tuples) of the take without / with the NaN at
    SIB_CHAIN_NAN -> the clean segments whose decision window [first - merge_gap - 1, last + merge_gap + 1] (the frames that open,
    continue, close or merge it) holds no affected frame; each must be in `bad` unchanged."""
    gap = S.SEGMENT_DEFAULTS["merge_gap"]
    affected = np.nonzero(B.holding(n, HOP, 512, 512, SIB_CHAIN_NAN))[0]
    keep = [s for s in clean if not ((affected >= s[2] - gap - 1) & (affected <= s[2] + s[3] + gap)).any()]
    have = {s[2]: s for s in bad}
    for s in keep:
        assert s[2] in have and tuple(s[:4]) == tuple(have[s[2]][:4]), (what, s)
        assert np.float32(s[4]).tobytes() == np.float32(have[s[2]][4]).tobytes() and np.float32(s[5]).tobytes() == np.float32(have[s[2]][5]).tobytes(), (what, s)
    return keep


def test_the_chain_with_a_nan_on_the_cpu(mxlib, emu, takes):
    """The take with one NaN inside a vowel: mx_sibilants equals sibilant_ref.segments on the emulation's records, and every
    segment of the clean take whose decision window does not reach a frame that holds the NaN survives unchanged — all three
    (the condition on the reference alone: at least three quarters)."""
    w, ref = takes["take"]
    v = B.with_bad(w, SIB_CHAIN_NAN, np.nan)
    with np.errstate(invalid="ignore"):
        ref_bad = S.features(v, SR, HOP)
    clean = S.segments(ref, HOP)
    assert len(segment_survivors(clean, S.segments(ref_bad, HOP), len(w), "reference")) >= 0.75 * len(clean)
    rec = emu.features(v, HOP, 0, len(ref))
    _same_segments(mxlib, rec)
    segment_survivors(S.segments(emu.features(w, HOP, 0, len(ref)), HOP), S.segments(rec, HOP), len(w), "emulation")


# ---- the host logic of the library against the reference ----
def _same_segments(mx, feat, hop=HOP, first=0, **params):
    got = mx.sibilants(feat, hop, first, **params)
    want = S.segments(feat, hop, first, **params)
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert tuple(int(g[k]) for k in ("start_sample", "end_sample", "first_frame", "frames")) == w[:4], (g, w)
        assert g["share"].tobytes() == w[4].tobytes() and g["level"].tobytes() == w[5].tobytes(), (g, w)
    return got


def _records(mx, rows):
    return np.array(rows, dtype=mx.SIB_FEAT_DTYPE)


HISS, HUM, QUIET = (1e-5, 1e-3, 300.0, 300), (1e-3, 1e-5, 10.0, 20), (1e-9, 1e-8, 300.0, 300)


def test_segments_crafted(mxlib):
    assert mxlib.sibilant_params_default() == S.SEGMENT_DEFAULTS and mxlib.sib_feature_params_default() == S.FEATURE_DEFAULTS

    def frames(n, hiss):
        rows = [HUM] * n
        for i in hiss:
            rows[i] = HISS
        return _records(mxlib, rows)

    kw = dict(min_frames=2)
    # runs touching frame 0 and the last frame
    got = _same_segments(mxlib, frames(30, [0, 1, 2, 27, 28, 29]), **kw)
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(0, 3), (27, 3)]
    assert (int(got[1]["start_sample"]), int(got[1]["end_sample"])) == (27 * HOP, 29 * HOP)
    # a gap of exactly merge_gap merges, merge_gap + 1 does not
    got = _same_segments(mxlib, frames(30, [3, 4, 7, 8, 12, 13]), **kw)
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(3, 6), (12, 2)]
    # a run of min_frames - 1 is dropped, min_frames kept (after merging)
    got = _same_segments(mxlib, frames(40, list(range(5, 10)) + list(range(20, 26))))
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(20, 6)]
    # hysteresis: a frame between the shares continues a run and does not open one; too few crossings do not open one either
    mid, calm = (5e-4, 5e-4, 100.0, 300), (1e-5, 1e-3, 300.0, 63)
    got = _same_segments(mxlib, _records(mxlib, [HUM, mid, mid, HISS, mid, (5.5e-4, 4.5e-4, 90.0, 300), HUM, calm, calm, calm, HUM]), **kw)
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(3, 3)]
    # below the floor nothing opens or continues
    got = _same_segments(mxlib, _records(mxlib, [QUIET] * 10 + [HISS, HISS, QUIET, QUIET, QUIET, HISS, HISS]), min_frames=1, merge_gap=0)
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(10, 2), (15, 2)]
    # NaN and Inf records are frames without level or share
    rows = [HISS] * 12
    rows[4], rows[8] = (np.nan, 1.0, np.nan, 300), (np.inf, np.inf, np.nan, 300)
    got = _same_segments(mxlib, _records(mxlib, rows), min_frames=1, merge_gap=0)
    assert [(int(s["first_frame"]), int(s["frames"])) for s in got] == [(0, 4), (5, 3), (9, 3)]
    # counts 0 and 1, a first frame and another hop
    assert len(_same_segments(mxlib, _records(mxlib, []))) == 0
    assert len(_same_segments(mxlib, _records(mxlib, [HISS]))) == 0
    one = _same_segments(mxlib, _records(mxlib, [HISS]), hop=100, first=7, min_frames=1)
    assert (int(one[0]["start_sample"]), int(one[0]["end_sample"]), int(one[0]["first_frame"])) == (700, 700, 7)


def test_segments_random(mxlib):
    rng = np.random.default_rng(17)
    total = 0
    for count in (2, 17, 64, 500):
        for _ in range(6):
            tot = 10.0 ** rng.uniform(-8, -1, count)
            share = np.clip(np.repeat(rng.random(count // 4 + 1), 4)[:count] + 0.1 * rng.standard_normal(count), 0, 1)
            feat = np.zeros(count, dtype=mxlib.SIB_FEAT_DTYPE)
            feat["low"], feat["high"] = tot * (1 - share), tot * share
            feat["zero_crossings"] = rng.integers(0, 400, count)
            total += len(_same_segments(mxlib, feat))
            total += len(_same_segments(mxlib, feat, hop=64, first=11, share_on=0.5, share_off=0.5, level_floor=1e-4, zc_min=0, merge_gap=0,
                                        min_frames=1))
            _same_segments(mxlib, feat, share_on=0.9, share_off=0.1, level_floor=0.0, zc_min=100, merge_gap=7, min_frames=3)
    assert total > 50


def _sibs(mx, spans):
    return np.array([(a, b, a // HOP, (b - a) // HOP + 1, 0.9, 0.05) for a, b in spans], dtype=mx.SIBILANT_DTYPE)


def _same_points(got, want, value):
    assert [int(p["sample"]) for p in got] == [int(p[0]) for p in want], (got, want)
    assert all(g[value].tobytes() == np.float32(w[1]).tobytes() for g, w in zip(got, want)), (got, want)


PROTECT_CASES = [
    # (curve, sibilant spans, ramp, n)
    ([(0, 4.0), (5000, 2.0), (9000, -3.0)], [(1000, 2000)], 100, 10000),
    ([(0, 4.0), (5000, 2.0), (9000, -3.0)], [(1000, 2000), (2150, 2400), (2700, 2700)], 100, 10000),   # overlapping ramps; touching spans; one frame
    ([(0, 4.0), (5000, 2.0), (9000, -3.0)], [(0, 300), (9800, 9999)], 500, 10000),                     # clipped at 0 and at n - 1
    ([(0, 4.0), (5000, 2.0), (9000, -3.0)], [(50, 300), (9800, 9990)], 500, 10000),                    # clipped ramps that keep a sample
    ([(900, 4.0), (1000, 2.0), (1500, 1.0), (2000, -3.0), (2100, 5.0)], [(1000, 2000)], 100, 10000),   # sibilants on curve points
    ([(4000, 3.0)], [(1000, 2000)], 100, 10000),
    ([(1500, 3.0)], [(1000, 2000)], 100, 10000),
    ([(-700, 1.0), (20000, 7.0)], [(1000, 2000), (3000, 3100)], 1, 10000),
    ([], [(1000, 2000)], 100, 10000),
    ([(0, 4.0), (5000, 2.0)], [], 100, 10000),
    ([(0, 1.5)], [(0, 0)], 1, 1),
]


@pytest.mark.parametrize("case", range(len(PROTECT_CASES)))
def test_protect_and_gain_points_crafted(mxlib, case):
    curve, spans, ramp, n = PROTECT_CASES[case]
    sibs = _sibs(mxlib, spans)
    got = mxlib.formant_protect(curve, sibs, ramp, n)
    _same_points(got, S.protect(curve, [tuple(s) for s in spans], ramp, n), "semitones")
    assert np.all(np.diff(got["sample"]) > 0)
    if not curve:
        assert len(got) == 0
    if not spans:
        assert [(int(p["sample"]), float(p["semitones"])) for p in got] == curve
    pts = [(int(p["sample"]), float(p["semitones"])) for p in got]
    for a, b in spans if curve else []:  # exactly 0 st on every core, F outside the spans, linear on the ramps
        assert all(S.curve(pts, x) == 0.0 for x in (a, (a + b) // 2, b))
    for lo, a, b, hi in S.spans(spans, ramp, n) if curve else []:
        for x in (x for x in (lo - 1, lo, hi, hi + 1) if 0 <= x <= n - 1 and not a <= x <= b):  # (inside the file, off the core)
            assert abs(S.curve(pts, x) - S.curve(curve, x)) <= 1e-6 * max(1.0, abs(S.curve(curve, x))), x
        if lo < a:
            assert abs(S.curve(pts, (lo + a) / 2) - S.curve(curve, lo) / 2) <= 1e-6 * max(1.0, abs(S.curve(curve, lo)))
    gp = mxlib.sibilant_gain_points(sibs, -6.0, ramp, n)
    _same_points(gp, S.gain_points([tuple(s) for s in spans], -6.0, ramp, n), "amp")
    assert np.all(np.diff(gp["sample"]) > 0) and np.all(gp["amp"] > 0)
    assert len(gp) == 0 if not spans else np.float32(10 ** (-6.0 / 20)) in gp["amp"]


def test_protect_and_gain_points_random(mxlib):
    rng = np.random.default_rng(23)
    n = 200000
    for trial in range(40):
        k = int(rng.integers(0, 9))
        edges = np.sort(rng.choice(np.arange(0, n), 2 * k, replace=False))
        spans = [(int(edges[2 * i]), int(edges[2 * i + 1])) for i in range(k)]
        curve = [(int(s), float(np.float32(rng.uniform(-6, 6)))) for s in np.sort(rng.choice(np.arange(-100, n + 100), int(rng.integers(0, 12)), replace=False))]
        ramp = int(rng.choice([1, 50, 2400, 30000]))
        sibs = _sibs(mxlib, spans)
        got = mxlib.formant_protect(curve, sibs, ramp, n)
        _same_points(got, S.protect(curve, spans, ramp, n), "semitones")
        assert np.all(np.diff(got["sample"]) > 0)
        db = float(rng.uniform(-24, 12))
        _same_points(mxlib.sibilant_gain_points(sibs, db, ramp, n), S.gain_points(spans, db, ramp, n), "amp")


def test_protected_curves_pass_the_formant_plan(mxlib):
    """mx_psola_plan_formant takes a protected curve as it is: an unvoiced track, so the plan is the curve's check and little else."""
    n = 20000
    track = np.zeros(mxlib.frame_count(n, HOP), dtype=mxlib.F0_DTYPE)
    track["aperiodicity"] = 1.0
    for curve, spans, ramp, _ in PROTECT_CASES[:8]:
        got = mxlib.formant_protect(curve, _sibs(mxlib, spans), ramp, 10000)
        fg, ns = mxlib.psola_plan_formant(n, SR, HOP, track, [], got)
        assert len(fg) > 0 and ns > 0
        at = {int(g["centre"]): int(g["step"]) for g in fg}
        inside = [st for c, st in at.items() if any(a <= c <= b for a, b in spans)]
        assert inside and all(st == 65536 for st in inside)  # 0 st on the cores: the plain step


# What a gain must carry like numpy does: NaN, Inf, -0, subnormals, the largest normals (Inf under a gain above 1) and a small
# normal that a gain below 1 takes into the subnormals.
GAIN_EDGES = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3.4e38, -3.4e38, 1.5e-38, -1.5e-38], dtype=np.float32)


def with_gain_edges(x):
    """x with its first samples replaced by GAIN_EDGES (as many as fit)."""
    x = np.array(x, dtype=np.float32, copy=True)
    m = min(len(x), len(GAIN_EDGES))
    x[:m] = GAIN_EDGES[:m]
    return x


def test_gain_arithmetic_equals_numpy(emu):
    rng = np.random.default_rng(5)
    for n in (1, 255, 2047, 2048, 2049, 6000):
        x = with_gain_edges(rng.standard_normal(n))
        many = sorted(set(int(v) for v in rng.integers(-50, n + 50, 5000)))
        lists = [[(n // 2, 0.37)], [(n // 3, 2.5), (n // 3 + 1, 0.01)], [(-10, 0.5), (n + 10, 1.5)],
                 [(s, float(np.float32(rng.uniform(0.01, 4.0)))) for s in many]]
        for pts in lists:
            want = S.apply_gain(x, pts)
            assert emu.gain(x, pts).tobytes() == want.tobytes(), (n, len(pts))
    x = np.array([1.0, np.inf, np.nan, -0.0, 1e-45], np.float32)
    assert emu.gain(x, [(0, 0.5), (4, 2.0)]).tobytes() == S.apply_gain(x, [(0, 0.5), (4, 2.0)]).tobytes()
    assert emu.gain(np.ones(5, np.float32), [(2, 0.25)]).tolist() == [0.25] * 5


def test_refusals(mxlib):
    def refused(fn, *args, **kw):
        with pytest.raises(mxlib.MxError) as e:
            fn(*args, **kw)
        assert e.value.code == -1, e.value

    feat = _records(mxlib, [HISS] * 8)
    for bad in (dict(share_on=1.1), dict(share_on=float("nan")), dict(share_off=-0.1), dict(share_off=0.7), dict(level_floor=-1.0),
                dict(level_floor=float("inf")), dict(zc_min=-1), dict(zc_min=1024), dict(merge_gap=-1), dict(merge_gap=4097),
                dict(min_frames=0), dict(min_frames=4097)):
        refused(mxlib.sibilants, feat, HOP, **bad)
    refused(mxlib.sibilants, feat, 0)
    refused(mxlib.sibilants, feat, HOP, -1)
    refused(mxlib.sibilants, feat, 16384, 2 ** 31 // 16384)  # frame centres beyond int32 samples
    ok, curve, n = _sibs(mxlib, [(1000, 2000), (3000, 3500)]), [(0, 1.0), (500, 2.0)], 10000
    for fn, head in ((mxlib.formant_protect, (curve,)), (lambda s, r, m: mxlib.sibilant_gain_points(s, -6.0, r, m), ())):
        refused(fn, *head, ok, 0, n)                                         # no ramp
        refused(fn, *head, ok, -5, n)
        refused(fn, *head, ok, 100, 0)
        refused(fn, *head, ok, 100, 3500)                                    # a sibilant past n - 1
        refused(fn, *head, _sibs(mxlib, [(3000, 3500), (1000, 2000)]), 100, n)   # out of order
        refused(fn, *head, _sibs(mxlib, [(1000, 2000), (2000, 2500)]), 100, n)   # sharing a sample
        bad = _sibs(mxlib, [(1000, 2000)])
        bad["end_sample"] = 900
        refused(fn, *head, bad, 100, n)
        bad["start_sample"], bad["end_sample"] = -1, 900
        refused(fn, *head, bad, 100, n)
    refused(mxlib.formant_protect, [(500, 1.0), (500, 2.0)], ok, 100, n)
    refused(mxlib.formant_protect, [(500, 1.0), (400, 2.0)], ok, 100, n)
    refused(mxlib.formant_protect, [(500, float("nan"))], ok, 100, n)
    for db in (float("nan"), float("inf"), -121.0, 41.0):
        refused(mxlib.sibilant_gain_points, ok, db, 100, n)


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation and the library's host logic with a main of their own over the smallest shapes and the edges of every
    list, under AddressSanitizer and UBSan."""
    out = emu_build.run_sanitized(tmp_path, "sibilant_emu_san", ["sibilant_emu.cpp", "sibilant_logic.cpp"], "SIBILANT_EMU_MAIN")
    assert "sibilant_emu ok" in out, out


def test_sibilant_and_gain_kernels_do_not_spill():
    """Both kernels scratch-free inside 256 VGPRs; the feature kernel's LDS is the 4.5 KiB transposition image and nothing else,
    the gain kernel's the tile's first segment."""
    seen = {}
    for unit in ("sibilant_kernels.hip", "gain_kernels.hip"):
        names, scratch, vgprs, lds = emu_build.resource_usage(unit)
        assert len(names) == 1, unit
        assert scratch == [0] and vgprs[0] <= 256, (unit, scratch, vgprs)
        seen[unit] = (names[0], lds[0])
    assert "sib_features_kernel" in seen["sibilant_kernels.hip"][0] and seen["sibilant_kernels.hip"][1] == 4608
    assert "audio_gain_kernel" in seen["gain_kernels.hip"][0] and seen["gain_kernels.hip"][1] == 8


# ---- the reference alone against the truth ----
def test_the_reference_finds_the_sibilants_of_the_take(takes):
    _, truth = S.take()
    segs = S.segments(takes["take"][1], HOP)
    want = [(name, a, b) for name, a, b in truth if name in S.SIBILANT_CLASSES]
    print("segments (frames):", [(s[2], s[2] + s[3] - 1) for s in segs], " truth (frames):", [(a / HOP, b / HOP) for _, a, b in want])
    assert len(segs) == len(want) == 3  # nothing on vowels, breath, click or gaps
    for s, (name, a, b) in zip(segs, want):
        assert abs(s[0] - a) <= 3 * HOP and abs(s[1] - (b - 1)) <= 3 * HOP, (name, s, a, b)
        assert s[4] > 0.5, (name, s)
    # the click: whatever run holds its frames without min_frames is one that min_frames drops (here zc_min already keeps the
    # breath around it from opening one)
    short = S.segments(takes["take"][1], HOP, min_frames=1)
    click = [s for s in short if s[2] - 2 <= S.CLICK // HOP <= s[2] + s[3] + 1]
    print("runs at min_frames 1:", [(s[2], s[3]) for s in short])
    assert len(short) == 3 + len(click) and all(s[3] < S.SEGMENT_DEFAULTS["min_frames"] for s in click)


def test_the_reference_on_the_onset_signals(takes):
    for name in ("notes5", "notes30", "legato", "vibrato", "clicks"):
        assert S.segments(takes[name][1], HOP) == [], name
    ref = takes["noise"][1]
    segs = S.segments(ref, HOP)
    assert len(segs) == 1 and segs[0][2] <= 1 and segs[0][2] + segs[0][3] >= len(ref) - 1  # white noise is a sibilant by this definition


def decision_margins(ref, **params):
    """Per frame over the floor: the distance of share from the nearer threshold, and of level from the floor relative to the
    level -> (frames over the floor, share margins, relative level margins of every frame)."""
    p = {**S.SEGMENT_DEFAULTS, **params}
    level, share = S.views(ref)
    over = level >= p["level_floor"]
    sm = np.minimum(np.abs(share - p["share_on"]), np.abs(share - p["share_off"]))
    lm = np.abs(level - p["level_floor"]) / np.maximum(level, 1e-300)
    return over, sm, lm


def test_no_decision_of_the_take_is_near_a_threshold(takes):
    """What the GPU comparison of segments rests on, checked here on the reference alone: on the synthetic take no frame over
    the floor has its share within 100 x the f32 yardstick (2e-5 of a ratio of order 1) of a threshold, none its level within
    100 x 2e-5 of its own size of the floor, and zero_crossings is an exact integer."""
    for name, (_, ref) in takes.items():
        over, sm, lm = decision_margins(ref)
        close = (over & (sm <= 100 * 2e-5)) | (lm <= 100 * 2e-5)
        print(f"{name}: nearest share margin {sm[over].min() if over.any() else float('nan'):.4f}  nearest level margin {lm.min():.4f}"
              f"  frames excused {int(close.sum())} of {len(ref)}")
        assert close.sum() <= 0.02 * len(ref), name
        if name == "take":
            assert close.sum() == 0


def test_the_reference_chain_protects_the_s(takes):
    """What tests/test_gpu_sibilant.py asks of the GPU, first of the definitions alone: yin_ref's track and notes, the per-note
    +4 st curve of INTEGRATION.md 3c, psola_formant_ref's render with it, with its protect()ed form and with no curve.  On the
    "s" the unprotected render's centroid moves by more than 10 %, the protected one's stays within one bin of the render
    without a formant shift."""
    import psola_formant_ref as FR
    import psola_ref as P
    import yin_ref as Y

    w, ref = takes["take"]
    _, truth = S.take()
    n = len(w)
    recs, _ = Y.track(w, SR, HOP)
    track = np.zeros(len(recs), dtype=[("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])
    for i, r in enumerate(recs):
        track[i] = r
    curve = []
    for nt in Y.detect_notes(track, SR, HOP):
        if curve and nt[0] <= curve[-1][0]:
            continue
        curve.append((int(nt[0]), 4.0))
        if nt[1] > nt[0]:
            curve.append((int(nt[1]), 4.0))
    prot = S.protect(curve, S.segments(ref, HOP), int(0.01 * SR), n)
    cent = {}
    for name, pts in (("zero", []), ("plain", curve), ("prot", prot)):
        g, L = FR.plan_formant(n, SR, HOP, track, [], pts)
        cent[name] = S.features(P.render(w.astype(np.float64), g, L).astype(np.float32), SR, HOP)["centroid"]
    lo, hi = next((a, b) for name, a, b in truth if name == "s")
    fr = [h for h in range(len(cent["zero"])) if h * HOP - 512 >= lo and h * HOP + 512 <= hi]
    moved = np.abs(cent["plain"][fr] - cent["zero"][fr]) / cent["zero"][fr]
    kept = np.abs(cent["prot"][fr] - cent["zero"][fr])
    print(f"s: unprotected moves by {moved.min():.3f}..{moved.max():.3f}; protected off by {kept.max():.3f} bins")
    assert len(curve) >= 6 and len(fr) >= 10 and moved.min() > 0.10 and kept.max() <= 1.0
