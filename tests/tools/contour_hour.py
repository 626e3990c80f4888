#!/usr/bin/env python3
"""tests/tools/contour_hour.py [--seconds S] [--log PATH] — the pitch-contour launches over the hour's track (675 000 frames
at hop 256, 48 kHz) with synthetic note spans, and the host side of a corrected render:
  kernels  between HIP events on the null stream, the median (min, max) of 10 launches after 3, ALTERNATING in one process:
           mx_contour_cents_dev; mx_contour_split_dev with records and statistics over notes of 60 .. 400 frames with gaps of
           0 .. 30 (the defaults: w 23, lags 15 .. 63); the same over ONE span of the whole hour; and, for scale, mx_f0_track_dev
           and mx_onset_flux_dev of the same build over the hour of audio the track stands for.
  host     on the host clock, the median of 5 calls after one: mx_contour_bend over the hour's records, mx_psola_plan_bend and
           mx_psola_plan of the same take.
The track is synthetic (a wandering contour with a 5.7 Hz vibrato): stages A and B read records, not audio; the audio under the
tracker and the flux is tests/key_ref.py's tiled "C major" take.  Prints one JSON line and, with --log, appends it to PATH.  No
counters are taken.  A tool, not a suite test."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import contour_ref as R  # noqa: E402
import key_ref as K  # noqa: E402
import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image  # noqa: E402

WARM, RUNS, HOST_RUNS = 3, 10, 5
HOP = 256


def note_spans(count, rng):
    spans, f = [], int(rng.integers(0, 30))
    while True:
        F = int(rng.integers(60, 401))
        if f + F > count:
            break
        spans.append((f, F))
        f += F + int(rng.integers(0, 31))
    return spans


def host_median(call):
    ts = []
    for it in range(HOST_RUNS + 1):
        t0 = time.perf_counter()
        out = call()
        if it:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    count = mx.frame_count(n, HOP)
    rng = np.random.default_rng(12)
    spans = note_spans(count, rng)
    cents = R.case_cents("voice", count, spans, seed=12)
    voiced = cents != R.NONE
    track = R.track_of(np.where(voiced, R.periods_of(np.where(voiced, cents, 0).astype(np.float64), SR), np.float32(0)), voiced)
    sp = np.array(spans, dtype=R.SPAN_DTYPE)
    whole = np.array([(0, count)], dtype=R.SPAN_DTYPE)
    p = mx.contour_params_default(SR, HOP)

    tile = K.takes()["c_major"][0]
    w = np.tile(tile, n // len(tile) + 1)[:n]
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(w)
    a = ctx.wrap_device(d_img.ptr, n)
    d_track, d_cents, d_all = DevBuf(track.nbytes), DevBuf(4 * count), DevBuf(4 * count)
    d_spans, d_whole = DevBuf(sp.nbytes), DevBuf(whole.nbytes)
    d_rec, d_stat, d_stat1 = DevBuf(8 * count), DevBuf(40 * len(sp)), DevBuf(40)
    d_f0, d_flux = DevBuf(16 * count), DevBuf(4 * count)
    d_track.write(track)
    d_spans.write(sp)
    d_whole.write(whole)
    d_all.write(np.where(voiced, cents, 72000).astype(np.int32))  # (the whole hour as one note: no frame without a value)
    timer = EventTimer(loaded_hip())
    rows = timer.timed({"cents": lambda: ctx.contour_cents_dev(d_track.ptr, count, SR, 0.15, 1e-3, d_cents.ptr),
                        "split_notes": lambda: ctx.contour_split_dev(d_cents.ptr, count, d_spans.ptr, len(sp), d_rec.ptr, d_stat.ptr, **p),
                        "split_notes_records_only": lambda: ctx.contour_split_dev(d_cents.ptr, count, d_spans.ptr, len(sp), d_rec.ptr, None, **p),
                        "split_one_span": lambda: ctx.contour_split_dev(d_all.ptr, count, d_whole.ptr, 1, d_rec.ptr, d_stat1.ptr, **p),
                        "f0_track": lambda: ctx.f0_track_dev(a, SR, HOP, 0, count, d_f0.ptr),
                        "onset_flux": lambda: ctx.onset_flux_dev(a, SR, HOP, 0, count, d_flux.ptr)}, WARM, RUNS)
    # the launches computed what the reference computes (its cents: the device's own)
    got_cents = d_cents.read(np.int32)
    ctx.contour_split_dev(d_cents.ptr, count, d_spans.ptr, len(sp), d_rec.ptr, d_stat.ptr, **p)
    ctx.synchronize()
    rec, stat = d_rec.read(R.REC_DTYPE), d_stat.read(R.STAT_DTYPE)
    want_rec, want_stat = R.split(got_cents, spans, **p)
    assert rec.tobytes() == want_rec.tobytes() and stat.tobytes() == want_stat.tobytes()
    assert int((got_cents != cents).sum()) * 1000 <= count  # (cents -> period -> cents: the f32 period moves a few by one unit)

    notes = np.zeros(len(sp), dtype=mx.NOTE_DTYPE)
    notes["first_frame"], notes["frames"] = sp["first"], sp["frames"]
    notes["note"] = [float(np.median(got_cents[f:f + F])) / 1600.0 for f, F in spans]
    bend_s, curve = host_median(lambda: mx.contour_bend(rec, notes, sp, None, drift_amount=1.0, vibrato_scale=0.5))
    plan_bend_s, (g, _) = host_median(lambda: mx.psola_plan_bend(n, SR, HOP, track, [], curve))
    plan_s, (g0, _) = host_median(lambda: mx.psola_plan(n, SR, HOP, track, []))
    res = {"samples": n, "sr": SR, "hop": HOP, "frames": count, "spans": len(sp), "params": p, "warmups": WARM, "launches": RUNS,
           "kernel_ms": rows, "split_over_flux": rows["split_notes"]["median"] / rows["onset_flux"]["median"],
           "contour_bend_s": bend_s, "psola_plan_bend_s": plan_bend_s, "psola_plan_s": plan_s, "grains": len(g), "grains_plain": len(g0),
           "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (d_track, d_cents, d_all, d_spans, d_whole, d_rec, d_stat, d_stat1, d_f0, d_flux):
        b.free()
    a.free()
    d_img.free()
    ctx.close()


if __name__ == "__main__":
    main()
