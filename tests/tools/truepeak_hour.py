#!/usr/bin/env python3
"""tests/tools/truepeak_hour.py [--seconds S] [--lookahead A] [--log PATH] — the true-peak record kernel and the look-ahead
limiter over the hour of 48 kHz audio (172.8 M samples, 360 000 steps) of tests/loudness_ref.py's levelling take, tiled and
scaled to peak at 1.5 (so that the limiter has work at its -1 dBTP ceiling):
  kernels   between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_true_peak_steps_dev,
            mx_audio_limit_dev without and with the int16 output (the call allocates its output: the events bracket the two pad
            clears and the kernel, not the allocation, and every output is freed after its launch), beside mx_audio_gain_dev
            (one point) and mx_loudness_steps_dev of the same build on the same samples, ALTERNATING in one process.
Prints one JSON line and, with --log, appends it to PATH.  No counters are taken and there is no threshold on the times: the
launches are new.  A tool, not a suite test; run each GPU step of a session under its own time limit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
import loudness_ref as L  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image, free_all  # noqa: E402

WARM, RUNS = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--lookahead", type=int, default=None)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = L.levelling_take()[0]
    tile = (tile * np.float32(1.5 / np.abs(tile).max())).astype(np.float32)
    w = np.tile(tile, n // len(tile) + 1)[:n]
    lookahead = mx.limit_params_default(SR)["lookahead"] if args.lookahead is None else args.lookahead
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(w)
    a = ctx.wrap_device(d_img.ptr, n)
    steps = mx.loudness_step_count(n, SR)
    groups = -(-steps // mx.LOUD_GROUP_STEPS)
    rec, loud, pcm, d_pts = DevBuf(steps * 8), DevBuf(steps * 16), DevBuf(n * 2), DevBuf(8)
    d_pts.write(np.array([(0, 0.5)], dtype=mx.GAIN_POINT_DTYPE))
    ctx.true_peak_steps_dev(a, SR, 0, steps, rec.ptr)
    records = rec.read(mx.TP_STEP_DTYPE)
    b = ctx.limit_dev(a, SR, lookahead=lookahead, d_pcm16=pcm.ptr)
    ctx.synchronize()
    limited_peak = ctx.true_peak(b, SR)
    first_pcm = pcm.read(np.int16, 0, 1 << 20)
    b.free()
    made = []
    timer = EventTimer(loaded_hip())
    calls = {"true_peak_steps": lambda: ctx.true_peak_steps_dev(a, SR, 0, steps, rec.ptr),
             "audio_limit": lambda: made.append(ctx.limit_dev(a, SR, lookahead=lookahead)),
             "audio_limit_pcm16": lambda: made.append(ctx.limit_dev(a, SR, lookahead=lookahead, d_pcm16=pcm.ptr)),
             "audio_gain": lambda: made.append(ctx.audio_gain_dev(a, d_pts.ptr, 1)),
             "loudness_steps": lambda: ctx.loudness_steps_dev(a, SR, 0, groups, loud.ptr)}
    rows = timer.timed(calls, WARM, RUNS, after=free_all(made))
    assert rec.read(mx.TP_STEP_DTYPE).tobytes() == records.tobytes()  # every launch wrote the same bytes
    assert pcm.read(np.int16, 0, 1 << 20).tobytes() == first_pcm.tobytes()
    ceiling = mx.limit_params_default(SR)["ceiling_amp"]
    res = {"samples": n, "sr": SR, "steps": steps, "lookahead": lookahead, "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "limit_over_audio_gain": rows["audio_limit"]["median"] / rows["audio_gain"]["median"],
           "limit_pcm16_over_audio_gain": rows["audio_limit_pcm16"]["median"] / rows["audio_gain"]["median"],
           "true_peak_over_loudness_steps": rows["true_peak_steps"]["median"] / rows["loudness_steps"]["median"],
           "limit_samples_per_s": n / (rows["audio_limit"]["median"] * 1e-3),
           "true_peak_samples_per_s": n / (rows["true_peak_steps"]["median"] * 1e-3),
           "true_peak": float(records["true_peak"].max()), "sample_peak": float(records["sample_peak"].max()), "ceiling_amp": ceiling,
           "limited_true_peak": float(limited_peak[0]), "limited_sample_peak": float(limited_peak[1]),
           "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for buf in (rec, loud, pcm, d_pts):
        buf.free()
    a.free()
    d_img.free()
    ctx.close()
    assert res["limited_sample_peak"] <= ceiling < res["sample_peak"], res


if __name__ == "__main__":
    main()
