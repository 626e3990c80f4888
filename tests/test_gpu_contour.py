"""The pitch-contour kernels on the GPU (include/melonix_amd.h "Pitch drift and vibrato inside notes"): stage B byte for byte
against numpy over the span shapes, widths and lag ranges, as spans of a 700-frame array and as one span of 70 000 frames;
stage A by the tie rule; host forms against device forms; guard bands; what a bad call or bad spans may touch.  No audio: the
tests build mx_f0 records on the host and upload them."""
import ctypes as C

import numpy as np
import pytest

import contour_ref as R
from conftest import DevBuf
from guarded import Guarded
from test_contour_host import stage_a_track

pytestmark = pytest.mark.gpu

REC, STAT = R.REC_DTYPE.itemsize, R.STAT_DTYPE.itemsize


def dev_cents(ctx, track, sr, threshold=0.15, rms_floor=1e-3):
    d_track, out = DevBuf(track.nbytes), Guarded(4 * len(track))
    try:
        d_track.write(track)
        ctx.contour_cents_dev(d_track.ptr, len(track), sr, threshold, rms_floor, out.ptr)
        ctx.synchronize()
        return out.take(np.int32)
    finally:
        d_track.free()
        out.free()


def dev_split(ctx, cents, spans, w, lag_min, lag_max, want_rec=True, want_stat=True):
    cents = np.ascontiguousarray(cents, dtype=np.int32)
    sp = np.array([tuple(s) for s in spans], dtype=R.SPAN_DTYPE)
    d_cents, d_spans = DevBuf(cents.nbytes), DevBuf(sp.nbytes)
    rec, stat = Guarded(REC * len(cents)), Guarded(STAT * len(sp))
    try:
        d_cents.write(cents)
        d_spans.write(sp)
        ctx.contour_split_dev(d_cents.ptr, len(cents), d_spans.ptr, len(sp), rec.ptr if want_rec else None,
                              stat.ptr if want_stat else None, half_width=w, lag_min=lag_min, lag_max=lag_max)
        ctx.synchronize()
        assert want_rec or rec.untouched()
        assert want_stat or stat.untouched()
        return rec.take(R.REC_DTYPE), stat.take(R.STAT_DTYPE)
    finally:
        for b in (d_cents, d_spans, rec, stat):
            b.free()


def check_stage_a(got, track, sr):
    """The CPU rule: equal wherever the reference's pre-rounding value is further than 1e-6 from a tie; nearer frames may
    differ by one unit, at most one frame in 1000 of them."""
    voiced, x = R.cents_exact(track, sr)
    near = voiced & (R.tie_distance(x) <= 1e-6)
    want = R.cents(track, sr)
    differ = got != want
    assert not (differ & ~near).any()
    assert (np.abs(got.astype(np.int64) - want)[differ] <= 1).all() and near.sum() * 1000 <= len(track)
    return int(differ.sum())


@pytest.mark.parametrize("kind", ["voice", "negative", "constant"])
def test_split_equals_numpy_over_the_span_shapes(gpu_ctx, kind):
    cents = R.case_cents(kind)
    if kind == "negative":
        # records made at sr 8000 with long periods, through stage A on the device: its int32 is the definition from here on
        voiced = cents != R.NONE
        periods = np.where(voiced, R.periods_of(np.where(voiced, cents, 0).astype(np.float64), 8000), np.float32(0))
        track = R.track_of(periods, voiced)
        got = dev_cents(gpu_ctx, track, 8000)
        check_stage_a(got, track, 8000)
        assert (got[voiced] < 0).all() and (got[~voiced] == R.NONE).all() and (track["period"][voiced] > 582).all()
        cents = got
    for w in R.CASE_WIDTHS:
        for lag_min, lag_max in R.CASE_LAGS:
            want_rec, want_stat = R.split(cents, R.CASE_SPANS, w, lag_min, lag_max)
            rec, stat = dev_split(gpu_ctx, cents, R.CASE_SPANS, w, lag_min, lag_max)
            assert rec.tobytes() == want_rec.tobytes(), (kind, w)
            assert stat.tobytes() == want_stat.tobytes(), (kind, w, lag_min, lag_max)
    assert [int(l) != 0 for l in stat["lag"]] == [F - 1 >= 200 for _, F in R.CASE_SPANS]  # (the last range: 200 .. 256)
    if kind == "constant":
        assert not rec["vib"].any() and not stat["r0"].any()


def test_one_long_span_equals_numpy(gpu_ctx):
    """The same contour as ONE span of 70 000 frames: 274 smoothing tiles and 69 statistics tiles add up to the reference's
    bytes, in the device form and in the host form (whose work memory has by now served other shapes)."""
    cents = R.case_cents("voice", 70000, [(0, 70000)])
    want_rec, want_stat = R.split(cents, [(0, 70000)], 23, 15, 62)
    rec, stat = dev_split(gpu_ctx, cents, [(0, 70000)], 23, 15, 62)
    assert rec.tobytes() == want_rec.tobytes() and stat.tobytes() == want_stat.tobytes()
    hrec, hstat = gpu_ctx.contour_split(cents, [(0, 70000)], half_width=23, lag_min=15, lag_max=62)
    assert hrec.tobytes() == want_rec.tobytes() and hstat.tobytes() == want_stat.tobytes()
    # spans that straddle the statistics tiles in every way: ending on a tile's last frame, starting on its first, inside one
    spans = [(0, 1024), (1024, 1), (1025, 2047), (3072, 500), (3600, 472), (4096, 4097), (9000, 61000)]
    want_rec, want_stat = R.split(cents, spans, 64, 1, 256)
    rec, stat = dev_split(gpu_ctx, cents, spans, 64, 1, 256)
    assert rec.tobytes() == want_rec.tobytes() and stat.tobytes() == want_stat.tobytes()


@pytest.mark.parametrize("sr", [48000, 8000])
def test_stage_a_by_the_tie_rule(gpu_ctx, sr):
    track = stage_a_track()
    track["tau"][5], track["period"][6], track["period"][7] = 0, np.nan, 0.0
    got = dev_cents(gpu_ctx, track, sr)
    differ = check_stage_a(got, track, sr)
    assert (got[5:8] == R.NONE).all()
    host = gpu_ctx.contour_cents(track, sr)
    assert host.tobytes() == got.tobytes()
    print(f"stage A at {sr} Hz: {len(track)} frames, {differ} differ from the host's log2")


def test_host_forms_equal_device_forms(gpu_ctx):
    cents = R.case_cents("voice")
    want = dev_split(gpu_ctx, cents, R.CASE_SPANS, 23, 15, 62)
    got = gpu_ctx.contour_split(cents, R.CASE_SPANS, half_width=23, lag_min=15, lag_max=62)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # either output alone
    only_rec = gpu_ctx.contour_split(cents, R.CASE_SPANS, want_stat=False, half_width=23, lag_min=15, lag_max=62)
    only_stat = gpu_ctx.contour_split(cents, R.CASE_SPANS, want_rec=False, half_width=23, lag_min=15, lag_max=62)
    assert only_rec[1] is None and only_rec[0].tobytes() == want[0].tobytes()
    assert only_stat[0] is None and only_stat[1].tobytes() == want[1].tobytes()
    assert dev_split(gpu_ctx, cents, R.CASE_SPANS, 23, 15, 62, want_rec=False)[1].tobytes() == want[1].tobytes()
    assert dev_split(gpu_ctx, cents, R.CASE_SPANS, 23, 15, 62, want_stat=False)[0].tobytes() == want[0].tobytes()
    # no spans: every record is {NONE, 0}; no frames: nothing
    rec, stat = gpu_ctx.contour_split(cents, [], half_width=23, lag_min=15, lag_max=62)
    assert (rec["smooth"] == R.NONE).all() and not rec["vib"].any() and len(stat) == 0
    rec, stat = gpu_ctx.contour_split(cents[:0], [], half_width=23, lag_min=15, lag_max=62)
    assert len(rec) == 0 and len(stat) == 0 and len(gpu_ctx.contour_cents(np.zeros(0, dtype=R.F0_DTYPE), 48000)) == 0


def test_pitch_contour_is_cents_then_split(mxlib, gpu_ctx):
    cents = R.case_cents("voice")
    voiced = cents != R.NONE
    track = R.track_of(np.where(voiced, R.periods_of(np.where(voiced, cents, 0).astype(np.float64), 48000), np.float32(0)), voiced)
    notes = np.zeros(len(R.CASE_SPANS), dtype=mxlib.NOTE_DTYPE)
    for i, (first, F) in enumerate(R.CASE_SPANS):
        notes[i] = (0, 0, first + 500, F, 45.0, 0.05, 0.1)
    dcents = dev_cents(gpu_ctx, track, 48000)
    p = mxlib.contour_params_default(48000, 256)
    want = dev_split(gpu_ctx, dcents, R.CASE_SPANS, p["half_width"], p["lag_min"], p["lag_max"])
    rec, stat = gpu_ctx.pitch_contour(track, 48000, 256, notes, first=500)
    assert rec.tobytes() == want[0].tobytes() and stat.tobytes() == want[1].tobytes()
    rec, stat = gpu_ctx.pitch_contour(track, 48000, 256, notes, first=500, half_width=5, lag_min=2, lag_max=9)
    want = dev_split(gpu_ctx, dcents, R.CASE_SPANS, 5, 2, 9)
    assert rec.tobytes() == want[0].tobytes() and stat.tobytes() == want[1].tobytes()
    # an unvoiced frame inside a note, notes that do not fit the track
    bad = track.copy()
    bad["tau"][150] = 0
    with pytest.raises(mxlib.MxError) as e:
        gpu_ctx.pitch_contour(bad, 48000, 256, notes, first=500)
    assert e.value.code == -1
    for first in (0, 499, 501):
        with pytest.raises(mxlib.MxError):
            gpu_ctx.pitch_contour(track, 48000, 256, notes, first=first)


def test_bad_spans_give_wrong_values_and_nothing_worse(gpu_ctx):
    """The device form cannot see its spans: each is clipped to the array, every index into its row.  The guard bands stay."""
    cents = R.case_cents("voice")
    cents[cents == R.NONE] = 70000
    for spans in ([(-50, 100), (650, 500)], [(100, 300), (200, 300), (50, 10)], [(0, -5), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 7)],
                  [(0, 700)] * 5):
        rec, stat = dev_split(gpu_ctx, cents, spans, 23, 15, 62)  # (take() has looked at the guard bands)
        assert len(rec) == 700 and len(stat) == len(spans)
    # spans clipped to the array are the spans of their clipped selves
    rec, stat = dev_split(gpu_ctx, cents, [(-50, 100), (650, 500)], 23, 15, 62)
    want = R.split(cents, [(0, 50), (650, 50)], 23, 15, 62)
    assert rec.tobytes() == want[0].tobytes() and stat.tobytes() == want[1].tobytes()


def test_refusals_touch_nothing(mxlib, gpu_ctx):
    L = mxlib._capi.lib()
    P = mxlib._capi.ContourParams
    h = gpu_ctx.handle
    buf = Guarded(4096)
    src = DevBuf(4096)
    host = np.zeros(512, dtype=np.int64)
    out = np.full(512, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    vp = C.c_void_p
    try:
        nan, inf = float("nan"), float("inf")
        for args in [(h, vp(src.ptr), -1, 48000, 0.15, 1e-3), (h, vp(src.ptr), 2 ** 31, 48000, 0.15, 1e-3), (h, vp(src.ptr), 4, 0, 0.15, 1e-3),
                     (h, vp(src.ptr), 4, -5, 0.15, 1e-3), (h, vp(src.ptr), 4, 48000, nan, 1e-3), (h, vp(src.ptr), 4, 48000, 0.15, inf),
                     (h, None, 4, 48000, 0.15, 1e-3), (None, vp(src.ptr), 4, 48000, 0.15, 1e-3)]:
            assert L.mx_contour_cents_dev(*args, vp(buf.ptr)) == -1, args
            hargs = (args[0], None if args[1] is None else vp(host.ctypes.data)) + args[2:]
            assert L.mx_contour_cents(*hargs, vp(out.ctypes.data)) == -1, args
        assert L.mx_contour_cents_dev(h, vp(src.ptr), 4, 48000, 0.15, 1e-3, None) == -1
        ok = P(23, 15, 62)
        for args in [(-1, vp(src.ptr), 0, ok), (2 ** 31, vp(src.ptr), 0, ok), (4, vp(src.ptr), -1, ok), (4, vp(src.ptr), 5, ok), (4, None, 1, ok),
                     (4, vp(src.ptr), 1, None), (4, vp(src.ptr), 1, P(-1, 15, 62)), (4, vp(src.ptr), 1, P(65, 15, 62)),
                     (4, vp(src.ptr), 1, P(23, 0, 62)), (4, vp(src.ptr), 1, P(23, 63, 62)), (4, vp(src.ptr), 1, P(23, 15, 257))]:
            count, spans, nspans, p = args
            pp = None if p is None else C.byref(p)
            assert L.mx_contour_split_dev(h, vp(src.ptr), count, spans, nspans, pp, vp(buf.ptr), vp(buf.ptr + 2048)) == -1, args
            hs = None if spans is None else vp(host.ctypes.data)
            assert L.mx_contour_split(h, vp(host.ctypes.data), count, hs, nspans, pp, vp(out.ctypes.data), vp(out.ctypes.data + 2048)) == -1, args
        assert L.mx_contour_split_dev(h, None, 4, vp(src.ptr), 1, C.byref(ok), vp(buf.ptr), None) == -1
        assert L.mx_contour_split_dev(None, vp(src.ptr), 4, vp(src.ptr), 1, C.byref(ok), vp(buf.ptr), None) == -1
        # the host form looks at the spans and at the frames inside them
        cents = np.full(100, 70000, dtype=np.int32)
        for bad in [[(0, 0)], [(-1, 5)], [(0, 101)], [(99, 2)], [(10, 20), (29, 5)], [(30, 5), (10, 5)]]:
            sp = np.array(bad, dtype=R.SPAN_DTYPE)
            assert L.mx_contour_split(h, vp(cents.ctypes.data), 100, vp(sp.ctypes.data), len(sp), C.byref(ok), vp(out.ctypes.data),
                                      vp(out.ctypes.data + 2048)) == -1, bad
        cents[50] = R.NONE
        sp = np.array([(40, 20)], dtype=R.SPAN_DTYPE)
        assert L.mx_contour_split(h, vp(cents.ctypes.data), 100, vp(sp.ctypes.data), 1, C.byref(ok), vp(out.ctypes.data), None) == -1
        gpu_ctx.synchronize()
        assert buf.untouched() and (out == 0x5A5A5A5A5A5A5A5A).all()  # every bad call was refused before any launch
    finally:
        buf.free()
        src.free()
