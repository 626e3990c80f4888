"""The PSOLA planner (mx_psola_plan, host code: no GPU) against its f64 restatement tests/psola_ref.py, field for field —
integers equal, floats equal as binary32 —, the plan's invariants, and the argument errors of every PSOLA entry point."""
import ctypes as C

import numpy as np
import pytest

import psola_ref

HOP = 256


def _track(n, hop, period, voiced=True):
    """F0 records of every frame of an n-sample file: `period` and `voiced` scalars or per-frame arrays."""
    from melonix_amd import F0_DTYPE
    count = (n + hop - 1) // hop
    t = np.zeros(count, dtype=F0_DTYPE)
    per = np.broadcast_to(np.asarray(period, dtype=np.float32), (count,))
    v = np.broadcast_to(np.asarray(voiced, dtype=bool), (count,))
    with np.errstate(invalid="ignore"):
        t["tau"] = np.where(v, np.clip(np.nan_to_num(per, nan=100.0, posinf=100.0, neginf=100.0), 1, 4000).astype(np.int32), 0)
    t["period"] = per
    t["aperiodicity"] = np.where(v, np.float32(0.02), np.float32(1.0))
    t["rms"] = np.float32(0.1)
    return t


def _blocks(count, a, b, run=5):
    return np.where((np.arange(count) // run) % 2 == 0, a, b)


def tracks(n, hop=HOP):
    """name -> track.  Every voicing pattern the definition distinguishes."""
    count = (n + hop - 1) // hop
    half = np.arange(count) < count // 2
    rng = np.random.default_rng(1234)
    garbage = np.array([np.nan, np.inf, -np.inf, -320.0, 2048.5, 1.5, 1e9, 0.0], dtype=np.float32)[np.arange(count) % 8]
    garbage = np.where(np.arange(count) % 3 == 0, np.float32(300.25), garbage)  # a sound frame in every three
    return {
        "voiced": _track(n, hop, 320.0 + 0.37 * np.sin(np.arange(count) * 0.3)),
        "unvoiced": _track(n, hop, 0.0, False),
        "blocks": _track(n, hop, 211.7, _blocks(count, True, False)),
        "period2": _track(n, hop, 2.0),
        "period2048": _track(n, hop, 2048.0),
        "abrupt": _track(n, hop, np.where(half, 2048.0, 27.0)),
        "garbage": _track(n, hop, garbage),
        "wander": _track(n, hop, rng.uniform(200.0, 400.0, count)),  # (a new period every frame, never under half the last)
    }


def marker_sets(n, sr):
    """name -> markers (sample, note, dTime, pitchBend) for a file of n samples."""
    e = max(n - 1, 2)
    span = (e - 1) / sr
    return {
        "none": [],
        "const+4": [(1, 0, 0.0, 4.0), (e, 0, 0.0, 4.0)],
        "ramp": [(1, 0, 0.0, -3.0), (e, 0, 0.0, 5.0)],
        "warp4": [(1, 0, 0.0, 2.0), (e, 0, 3.0 * span, 2.0)],
        "warp1/4": [(1, 0, 0.0, -2.0), (e, 0, -0.75 * span, -2.0)],
        "bend+30": [(1, 0, 0.0, 30.0), (e, 0, 0.0, 30.0)],
        "bend-30": [(1, 0, 0.0, -30.0), (e, 0, 0.0, -30.0)],
    }


def _cases():
    out = []
    for sr in (48000, 44100):
        for n in (1, 255, 4096, 72000):
            for tn in ("voiced", "unvoiced", "blocks", "period2", "period2048", "abrupt", "garbage", "wander"):
                for mn in ("none", "const+4", "ramp", "warp4", "warp1/4", "bend+30", "bend-30"):
                    # (a period of 2 over 72 000 samples is 10^5 grains and more of a Python loop: the small sizes cover it,
                    # and one long run without a warp)
                    if n == 72000 and tn == "period2" and (mn != "const+4" or sr != 48000):
                        continue
                    out.append((sr, n, tn, mn))
    return out


_PLANS = {}


def both_plans(mxlib, sr, n, tn, mn, hop=HOP):
    """(library plan, reference plan) of a case, computed once for the tests that look at them."""
    key = (sr, n, tn, mn, hop)
    if key not in _PLANS:
        track, markers = tracks(n, hop)[tn], marker_sets(n, sr)[mn]
        _PLANS[key] = (mxlib.psola_plan(n, sr, hop, track, markers), psola_ref.plan(n, sr, hop, track, markers))
    return _PLANS[key]


@pytest.mark.parametrize("sr,n,tn,mn", _cases())
def test_plan_matches_reference_and_keeps_its_invariants(mxlib, sr, n, tn, mn):
    (g, L), (rg, rL) = both_plans(mxlib, sr, n, tn, mn)
    markers = marker_sets(n, sr)[mn]
    assert L == rL == mxlib._capi.lib().mx_pv_render_length(n, sr, mxlib._capi.markers_array(markers), len(markers))
    assert len(g) == len(rg)
    for f in g.dtype.names:  # integers equal, floats equal as binary32: the same bytes
        assert g[f].tobytes() == rg[f].tobytes(), (f, int(np.argmax(g[f] != rg[f])))
    if not len(g):
        assert n == 1 and L == 0  # (one sample has no duration)
        return
    key = g["centre"].astype(np.float64) + g["centre_frac"].astype(np.float64)
    assert (np.diff(key) > 0).all() and (np.diff(g["centre"]) >= 0).all()
    assert (g["out_lo"] >= 0).all() and (g["out_lo"] <= g["out_hi"]).all() and (g["out_hi"] <= L).all()
    for f in ("src_frac", "centre_frac"):
        assert (g[f] >= 0).all() and (g[f] < 1).all()
    assert (g["inv_half"] >= np.float32(1.0 / 2048)).all() and (g["inv_half"] <= 0.5).all()
    if mn == "none":
        assert not g["src_off"].any() and not g["src_frac"].any()
    if tn == "garbage":  # only the sound frames' period, or U
        assert set(np.unique(g["inv_half"])) <= {np.float32(1 / 300.25), np.float32(1 / 256.0)}
    if mn in ("bend+30", "bend-30") and tn == "voiced" and n >= 4096:  # clamped to an octave
        spacing = np.diff(key)[2:-4] * g["inv_half"][2:-5].astype(np.float64)  # (the bend ramps in at sample 1 and is 0 beyond the duration)
        assert np.allclose(spacing, 0.5 if mn == "bend+30" else 2.0, rtol=1e-6)


def test_other_hops_and_parameters(mxlib):
    n, sr = 20000, 48000
    for hop, params in ((100, {}), (1000, {"unvoiced_period": 32.0}), (16384, {"unvoiced_period": 2048.0}),
                        (256, {"threshold": 0.01}), (256, {"rms_floor": 0.5})):
        track = tracks(n, hop)["blocks"]
        markers = marker_sets(n, sr)["ramp"]
        g, L = mxlib.psola_plan(n, sr, hop, track, markers, **params)
        rg, rL = psola_ref.plan(n, sr, hop, track, markers, **params)
        assert L == rL and g.tobytes() == rg.tobytes(), (hop, params)
    # the two voicing parameters above silence every frame: U everywhere
    assert set(np.unique(g["inv_half"])) == {np.float32(1 / 256.0)}


@pytest.mark.parametrize("tn", ["voiced", "unvoiced", "blocks", "period2", "period2048", "garbage", "wander"])
@pytest.mark.parametrize("n", [255, 4096, 72000])
def test_zero_bend_reference_render_is_the_input(mxlib, n, tn):
    """No markers: every grain reads the source where it writes, and the window sum divides out.  ("abrupt" is left out by
    the definition itself: where the period falls to a small fraction from one mark to the next — 2048 to 27 — the long
    window has all but faded before the short grains begin, the window sum dips under the floor of 1/4 there, and the floor,
    not the sum, divides.  A period that halves at most keeps the sum above 0.34.)"""
    if tn == "period2" and n == 72000:
        n = 20000
    rng = np.random.default_rng(n)
    w = rng.uniform(-0.9, 0.9, n).astype(np.float32)
    g, L = mxlib.psola_plan(n, 48000, HOP, tracks(n)[tn], [])
    assert L == n - 1  # (the samples i with i / sr < duration() = (n - 1) / sr)
    y = psola_ref.render(w, g, L)
    assert np.abs(y - w[:L].astype(np.float64)).max() <= 1e-12


def test_defaults(mxlib):
    d = mxlib.psola_params_default()
    assert d == {"threshold": np.float32(0.15), "rms_floor": np.float32(1e-3), "unvoiced_period": 256.0}
    assert d == {k: float(v) for k, v in psola_ref.DEFAULTS.items()}
    # the defaults written out give the plan of "nothing given" (NULL)
    n = 4096
    t = tracks(n)["blocks"]
    a, _ = mxlib.psola_plan(n, 48000, HOP, t, [])
    b, _ = mxlib.psola_plan(n, 48000, HOP, t, [], **d)
    assert a.tobytes() == b.tobytes()
    with pytest.raises(TypeError):
        mxlib.psola_plan(n, 48000, HOP, t, [], treshold=0.1)


def test_plan_argument_errors(mxlib):
    n, sr = 4096, 48000
    t = tracks(n)["voiced"]

    def bad(**kw):
        a = dict(n=n, sr=sr, hop=HOP, track=t, markers=[], params={})
        a.update(kw)
        with pytest.raises(mxlib.MxError) as e:
            mxlib.psola_plan(a["n"], a["sr"], a["hop"], a["track"], a["markers"], **a["params"])
        assert e.value.code == -1, kw

    bad(track=t[:-1])                      # count != mx_frame_count(n, hop)
    bad(track=np.concatenate([t, t[:1]]))
    bad(hop=0, track=t[:0])
    bad(hop=16385, track=t[:1])
    bad(sr=0)
    bad(sr=-48000)
    bad(n=-1, track=t[:0])
    bad(n=2 ** 31 - 1 - 2 * 32768 + 1, hop=16384, track=t[:0])
    for u in (31.9, 2048.5, float("nan"), float("inf")):
        bad(params={"unvoiced_period": u})
    for k in ("threshold", "rms_floor"):
        for v in (float("nan"), float("inf")):
            bad(params={k: v})
    bad(markers=[(100, 0, 0.0, 1.0), (50, 0, 0.0, 1.0)])          # unsorted: mx_pv_render_length's checks
    bad(markers=[(100, 0, float("nan"), 1.0)])
    # null outputs
    L = mxlib._capi.lib()
    cnt, ns, out = C.c_int64(), C.c_int64(), C.c_void_p()
    tp = C.c_void_p(t.ctypes.data)
    assert L.mx_psola_plan(n, sr, HOP, tp, len(t), None, None, 0, None, C.byref(cnt), C.byref(ns)) == -1
    assert L.mx_psola_plan(n, sr, HOP, tp, len(t), None, None, 0, C.byref(out), None, C.byref(ns)) == -1
    assert L.mx_psola_plan(n, sr, HOP, tp, len(t), None, None, 0, C.byref(out), C.byref(cnt), None) == -1
    assert L.mx_psola_plan(n, sr, HOP, None, len(t), None, None, 0, C.byref(out), C.byref(cnt), C.byref(ns)) == -1
    assert L.mx_psola_plan(n, sr, HOP, tp, len(t), None, None, 3, C.byref(out), C.byref(cnt), C.byref(ns)) == -1
    assert out.value is None and b"marker" in L.mx_last_error()
    L.mx_psola_params_default(None)  # (nothing to fill: no fault)
    # an empty file has no grains
    g, m = mxlib.psola_plan(0, sr, HOP, t[:0], [])
    assert len(g) == 0 and m == 0


def test_device_entry_points_check_their_arguments_before_the_device(mxlib):
    """The four entry points that need a context refuse a null one (and null audio) as MX_ERR_INVALID: no GPU is touched."""
    L = mxlib._capi.lib()
    g = np.zeros(1, dtype=mxlib.PSOLA_GRAIN_DTYPE)
    t = tracks(4096)["voiced"]
    gp, tp = C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data)
    out = np.full(16, 7.0, dtype=np.float32)
    op = C.c_void_p(out.ctypes.data)
    assert L.mx_psola_synth(None, None, gp, 1, 16, op, None) == -1
    assert L.mx_psola_synth_dev(None, None, gp, 1, 16, op, None) == -1
    assert L.mx_psola_render(None, None, 48000, HOP, tp, len(t), None, None, 0, op, None) == -1
    assert L.mx_psola_render_dev(None, None, 48000, HOP, tp, len(t), None, None, 0, op, None) == -1
    assert b"null context" in L.mx_last_error() and (out == 7.0).all()
