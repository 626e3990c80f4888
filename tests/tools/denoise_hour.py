#!/usr/bin/env python3
"""tests/tools/denoise_hour.py [--seconds S] [--log PATH] — the noise reduction over the hour at 48 kHz (tests/denoise_ref.py's
vowel take, tiled: 172.8 M samples, 675 000 output blocks).
  kernels   between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_denoise_dev of the whole take
            into buffers kept for all launches — f32 alone, and f32 + int16 — and mx_noise_print_dev over 2 s, beside
            mx_onset_flux_dev at hop 256 (one such transform a frame) and mx_audio_gain_dev (one point; the call allocates its
            output, freed after its launch) of the same build, ALTERNATING in one process.
Every denoise launch must write the same bytes (the first and the last 4 MiB of the kept buffers are compared).  Prints one JSON
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
SR, HOP = 48000, 256
SETTING = (12.0, 6.0)


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
    P = ctx.noise_print(a, 0, 12000)
    frames = mx.frame_count(n, HOP)
    d_f32, d_i16, d_flux, d_print, d_pts = DevBuf(4 * n), DevBuf(2 * n), DevBuf(4 * frames), DevBuf(4 * mx.DENOISE_BINS), DevBuf(8)
    d_pts.write(np.array([(0, 0.5)], dtype=mx.GAIN_POINT_DTYPE))
    made = []
    two_s = min(2 * SR, n)
    calls = {
        "denoise_f32": lambda: ctx.denoise_dev(a, P, SETTING[0], SETTING[1], 0, n, d_f32.ptr, None),
        "denoise_f32_i16": lambda: ctx.denoise_dev(a, P, SETTING[0], SETTING[1], 0, n, d_f32.ptr, d_i16.ptr),
        "noise_print_2s": lambda: ctx.noise_print_dev(a, 0, two_s, d_print.ptr),
        "onset_flux": lambda: ctx.onset_flux_dev(a, SR, HOP, 0, frames, d_flux.ptr),
        "audio_gain": lambda: made.append(ctx.audio_gain_dev(a, d_pts.ptr, 1)),
    }
    calls["denoise_f32_i16"]()
    first = ends(d_f32, n, np.float32), ends(d_i16, n, np.int16)
    timer = EventTimer(loaded_hip())
    rows = timer.timed(calls, WARM, RUNS, after=free_all(made))
    assert (ends(d_f32, n, np.float32), ends(d_i16, n, np.int16)) == first  # every launch wrote the same bytes
    res = {"seconds": args.seconds, "samples": n, "warmups": WARM, "launches": RUNS, "kernel_ms": rows, "setting_db": SETTING,
           "denoise_f32_over_onset_flux": rows["denoise_f32"]["median"] / rows["onset_flux"]["median"],
           "denoise_f32_i16_over_onset_flux": rows["denoise_f32_i16"]["median"] / rows["onset_flux"]["median"],
           "denoise_f32_over_audio_gain": rows["denoise_f32"]["median"] / rows["audio_gain"]["median"],
           "samples_per_s": n / (rows["denoise_f32"]["median"] * 1e-3),
           "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for buf in (d_f32, d_i16, d_flux, d_print, d_pts):
        buf.free()
    a.free()
    d_img.free()
    ctx.close()


if __name__ == "__main__":
    main()
