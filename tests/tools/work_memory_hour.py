#!/usr/bin/env python3
"""tests/tools/work_memory_hour.py PARENT_LIB [--seconds S] — the host forms that go through the context's work memory and job
buffers (mx_tempo_comb, mx_tempo_from_flux, mx_tempo_detect, mx_chroma_sum, mx_key_detect, mx_contour_split, mx_pitch_contour,
mx_f0_decode, mx_f0_track_decoded) over the hour of a tiled ten-second sweep (675 000 frames at hop 256): another build of the
library (PARENT_LIB, a path to its libmelonix_amd.so) and this tree's ALTERNATING call by call in one process, between HIP events
on the null stream (tests/hip_timing.py's loop): 3 warm-ups, the median (min, max) of 10.  Every result is asserted byte-equal
across the two libraries.  Prints one JSON line.  A tool, not a suite test."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, accum_sweep, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image  # noqa: E402

HOP, WARM, RUNS = 256, 3, 10
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


def P(a):
    return vp(a.ctypes.data) if a is not None else None


def main():
    parent = sys.argv[1]
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 3600.0
    n = int(seconds * SR)
    tile = accum_sweep(10 * SR)
    w = np.tile(tile, n // len(tile) + 1)[:n]
    d_img = device_image(w)
    libs = {"parent": TimedLib(parent, d_img, n), "fold": TimedLib(mx._capi.lib()._name, d_img, n)}
    assert libs["parent"].version != libs["fold"].version
    hip = loaded_hip()
    timer = EventTimer(hip)
    F = -(-n // HOP)
    L0 = libs["fold"]

    def ok(rc):
        assert rc == 0, rc

    # the inputs, made once with the fold's device forms
    d_flux, d_chroma, d_track, d_cands = DevBuf(4 * F), DevBuf(160 * F), DevBuf(16 * F), DevBuf(64 * F)
    ok(L0.so.mx_onset_flux_dev(L0.ctx, L0.audio, SR, HOP, i64(0), i64(F), None, vp(d_flux.ptr)))
    ok(L0.so.mx_chroma_dev(L0.ctx, L0.audio, SR, HOP, i64(0), i64(F), None, vp(d_chroma.ptr)))
    ok(L0.so.mx_f0_candidates_dev(L0.ctx, L0.audio, SR, HOP, i64(0), i64(F), f32(55.), f32(1760.), f32(0.15), vp(d_track.ptr), vp(d_cands.ptr)))
    flux, chroma = d_flux.read(np.float32), d_chroma.read(np.float32)
    track, cands = d_track.read(mx.F0_DTYPE), d_cands.read(mx.F0_CAND_DTYPE)
    for b in (d_flux, d_chroma, d_track, d_cands):
        b.free()
    decoded = np.empty(F, dtype=mx.F0_DTYPE)
    ok(L0.so.mx_f0_decode(L0.ctx, P(track), P(cands), i64(F), None, P(decoded), None))
    cents = np.empty(F, dtype=np.int32)
    ok(L0.so.mx_contour_cents(L0.ctx, P(decoded), i64(F), SR, f32(0.15), f32(1e-3), P(cents)))
    spans, run = [], 0
    voiced = np.append(cents != mx.CONTOUR_NONE, False)
    for f in range(F + 1):
        if voiced[f] and run < 300:
            run += 1
            continue
        if run >= 8:
            spans.append((f - run, run))
        run = 1 if voiced[f] else 0
    spans = np.array(spans, dtype=mx.CONTOUR_SPAN_DTYPE)
    notes = np.zeros(len(spans), dtype=mx.NOTE_DTYPE)
    notes["first_frame"], notes["frames"], notes["note"] = spans["first"], spans["frames"], 60.0
    notes["start_sample"], notes["end_sample"] = spans["first"] * HOP, (spans["first"] + spans["frames"] - 1) * HOP
    cp = (i32 * 3)()
    ok(L0.so.mx_contour_params_default(SR, HOP, cp))
    combs = np.array([(512 * (j // 64), 2048, (20 + j % 64 * 3) << 16) for j in range(64 * ((F - 2048) // 512))], dtype=mx.COMB_JOB_DTYPE)
    sums = np.array([(512 * j, 2048) for j in range((F - 2048) // 512)] + [(0, F)], dtype=mx.CHROMA_JOB_DTYPE)
    curve = np.empty(F, dtype=np.float32)
    ok(L0.so.mx_tempo_smooth(L0.ctx, P(flux), i64(F), 4, P(curve)))

    out = {k: {} for k in libs}  # name -> the call's result bytes, per library

    def handed(L, win, nwin, item):
        b = C.string_at(win.value, nwin.value * item) if win.value else b""
        L.so.mx_free.argtypes = [vp]
        L.so.mx_free(win)
        return b

    def tempo_from_flux(L, k):
        t, win, nwin = mx._capi.Tempo(), vp(), i64()
        ok(L.so.mx_tempo_from_flux(L.ctx, P(flux), i64(F), SR, HOP, i64(0), None, C.byref(t), C.byref(win), C.byref(nwin)))
        out[k]["tempo_from_flux"] = (t.bpm, t.offset, t.score, t.clarity, t.locked_frames, t.levels, handed(L, win, nwin, 16))

    def tempo_detect(L, k):
        t, win, nwin = mx._capi.Tempo(), vp(), i64()
        ok(L.so.mx_tempo_detect(L.ctx, L.audio, SR, HOP, None, None, C.byref(t), C.byref(win), C.byref(nwin)))
        out[k]["tempo_detect"] = (t.bpm, t.offset, t.score, t.clarity, t.locked_frames, t.levels, handed(L, win, nwin, 16))

    def tempo_comb(L, k):
        rec = np.empty(len(combs), dtype=mx.COMB_DTYPE)
        ok(L.so.mx_tempo_comb(L.ctx, P(curve), i64(F), P(combs), i64(len(combs)), P(rec)))
        out[k]["tempo_comb"] = rec.tobytes()

    def chroma_sum(L, k):
        s = np.empty((len(sums), 40), dtype=np.float64)
        ok(L.so.mx_chroma_sum(L.ctx, P(chroma), i64(F), P(sums), i64(len(sums)), P(s)))
        out[k]["chroma_sum"] = s.tobytes()

    def key_detect(L, k):
        key, win, nwin = mx._capi.Key(), vp(), i64()
        ok(L.so.mx_key_detect(L.ctx, L.audio, SR, HOP, None, i64(2048), i64(512), C.byref(key), C.byref(win), C.byref(nwin)))
        out[k]["key_detect"] = (bytes(key), handed(L, win, nwin, 56))

    def contour_split(L, k):
        rec, stat = np.empty(F, dtype=mx.CONTOUR_REC_DTYPE), np.empty(len(spans), dtype=mx.CONTOUR_STAT_DTYPE)
        ok(L.so.mx_contour_split(L.ctx, P(cents), i64(F), P(spans), i64(len(spans)), cp, P(rec), P(stat)))
        out[k]["contour_split"] = (rec.tobytes(), stat.tobytes())

    def contour_split_stat(L, k):
        stat = np.empty(len(spans), dtype=mx.CONTOUR_STAT_DTYPE)
        ok(L.so.mx_contour_split(L.ctx, P(cents), i64(F), P(spans), i64(len(spans)), cp, None, P(stat)))
        out[k]["contour_split_stat"] = stat.tobytes()

    def pitch_contour(L, k):
        rec, stat = np.empty(F, dtype=mx.CONTOUR_REC_DTYPE), np.empty(len(spans), dtype=mx.CONTOUR_STAT_DTYPE)
        ok(L.so.mx_pitch_contour(L.ctx, P(decoded), i64(F), SR, HOP, i64(0), P(notes), i64(len(notes)), f32(0.15), f32(1e-3), None, P(rec), P(stat)))
        out[k]["pitch_contour"] = (rec.tobytes(), stat.tobytes())

    def f0_decode(L, k):
        o, st = np.empty(F, dtype=mx.F0_DTYPE), np.empty(F, dtype=np.uint8)
        ok(L.so.mx_f0_decode(L.ctx, P(track), P(cands), i64(F), None, P(o), P(st)))
        out[k]["f0_decode"] = (o.tobytes(), st.tobytes())

    def f0_track_decoded(L, k):
        o = np.empty(F, dtype=mx.F0_DTYPE)
        ok(L.so.mx_f0_track_decoded(L.ctx, L.audio, SR, HOP, i64(0), i64(F), f32(55.), f32(1760.), f32(0.15), None, P(o)))
        out[k]["f0_track_decoded"] = o.tobytes()

    rows = {}
    for fn in (tempo_comb, tempo_from_flux, tempo_detect, chroma_sum, key_detect, contour_split, contour_split_stat, pitch_contour,
               f0_decode, f0_track_decoded):
        rows[fn.__name__] = timer.timed({k: (lambda L=L, k=k: fn(L, k)) for k, L in libs.items()}, WARM, RUNS)
        assert out["parent"][fn.__name__] == out["fold"][fn.__name__], fn.__name__
    print(json.dumps({"frames": F, "comb_jobs": len(combs), "sum_jobs": len(sums), "spans": len(spans), "warmups": WARM, "launches": RUNS,
                      "libs": {k: L.version for k, L in libs.items()}, "same_bytes": True, "ms": rows}))


if __name__ == "__main__":
    main()
