#!/usr/bin/env python3
"""tests/tools/compress_hour.py [--seconds S] [--log PATH] — the dynamics compressor over the hour at 48 kHz
(tests/denoise_ref.py's vowel take, tiled: 172.8 M samples, 3.6 M control steps, 879 groups) at the defaults.
  kernels   between HIP events on the null stream, the median (min, max) of 10 launches after 3, ALTERNATING in one process:
            mx_compress_peaks_dev over every step (the peaks launch alone); mx_compress_gain_dev over every step (the table's
            copy, the peaks launch and the curve launch), at the default release and at 2 s; mx_compress_dev of the whole take
            into a buffer kept for all launches (those and the apply launch), f32 alone and f32 + int16; mx_audio_compress (the
            same with its allocation and pad clears, freed after its launch); beside mx_audio_gain_dev (one point) and
            mx_audio_limit_dev of the same build.  The curve launch and the apply launch are not entry points of their own:
            their times are the differences gain - peaks and compress - gain of the medians.
Every compress launch must write the same bytes (the first and the last 4 MiB of the kept buffers are compared).  Prints one JSON
line and, with --log, appends it to PATH.  No counters are taken and there is no threshold on the times: the launches are new.  A
tool, not a suite test; run each GPU step of a session under its own time limit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
import denoise_ref as D  # noqa: E402
from conftest import DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image, ends, free_all  # noqa: E402

WARM, RUNS = 3, 10
SR = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    tile = D.vowel_take(1e-2)
    n = int(args.seconds * SR)
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(np.tile(tile, n // len(tile) + 1)[:n])
    a = ctx.wrap_device(d_img.ptr, n)
    steps = mx.compress_steps(n, SR)
    d_f32, d_i16, d_pk, d_gain, d_pts = DevBuf(4 * n), DevBuf(2 * n), DevBuf(4 * steps), DevBuf(4 * steps), DevBuf(8)
    d_pts.write(np.array([(0, 0.5)], dtype=mx.GAIN_POINT_DTYPE))
    made = []
    calls = {
        "peaks": lambda: ctx.compress_peaks_dev(a, SR, 0, steps, d_pk.ptr),
        "gain": lambda: ctx.compress_gain_dev(a, SR, 0, steps, d_gain.ptr),
        "gain_release_2s": lambda: ctx.compress_gain_dev(a, SR, 0, steps, d_gain.ptr, release_ms=2000.0),
        "compress_f32": lambda: ctx.compress_dev(a, SR, 0, n, d_f32.ptr, None),
        "compress_f32_i16": lambda: ctx.compress_dev(a, SR, 0, n, d_f32.ptr, d_i16.ptr),
        "audio_compress": lambda: made.append(ctx.compress(a, SR)),
        "audio_gain": lambda: made.append(ctx.audio_gain_dev(a, d_pts.ptr, 1)),
        "audio_limit": lambda: made.append(ctx.limit_dev(a, SR)),
    }
    calls["compress_f32_i16"]()
    first = ends(d_f32, n, np.float32), ends(d_i16, n, np.int16)
    turned_down = int((ctx.compress_gain(a, SR, 0, min(steps, 100000)) < (1 << 30)).sum())
    timer = EventTimer(loaded_hip())
    rows = timer.timed(calls, WARM, RUNS, after=free_all(made))
    assert (ends(d_f32, n, np.float32), ends(d_i16, n, np.int16)) == first  # every launch wrote the same bytes
    med = {k: v["median"] for k, v in rows.items()}
    res = {"seconds": args.seconds, "samples": n, "steps": steps, "groups": -(-steps // 4096), "warmups": WARM, "launches": RUNS,
           "kernel_ms": rows, "curve_ms": med["gain"] - med["peaks"], "curve_release_2s_ms": med["gain_release_2s"] - med["peaks"],
           "apply_f32_ms": med["compress_f32"] - med["gain"], "apply_f32_i16_ms": med["compress_f32_i16"] - med["gain"],
           "peaks_over_audio_limit": med["peaks"] / med["audio_limit"],
           "apply_f32_over_audio_limit": (med["compress_f32"] - med["gain"]) / med["audio_limit"],
           "compress_f32_over_audio_gain": med["compress_f32"] / med["audio_gain"],
           "steps_turned_down_of_first_100000": turned_down, "samples_per_s": n / (med["compress_f32"] * 1e-3),
           "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for buf in (d_f32, d_i16, d_pk, d_gain, d_pts):
        buf.free()
    a.free()
    d_img.free()
    ctx.close()


if __name__ == "__main__":
    main()
