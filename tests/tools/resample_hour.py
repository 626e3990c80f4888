#!/usr/bin/env python3
"""tests/tools/resample_hour.py [--seconds S] [--log PATH] — the sample-rate conversion over the hour (tests/loudness_ref.py's
levelling take, tiled and scaled to peak at 1.5): the hour at 48 kHz (172.8 M samples) to 44.1 kHz (147 / 160), the hour at
44.1 kHz to 48 kHz (160 / 147) and the hour at 96 kHz to 48 kHz (1 / 2).
  kernels   between HIP events on the null stream, the median (min, max) of 10 launches after 3: per ratio mx_audio_resample (the
            call allocates its output: the events bracket the allocation, the two pad clears and the kernel, and every output is
            freed after its launch) and mx_resample_dev of the whole take into a buffer kept for all launches (the kernel alone),
            beside mx_audio_gain_dev (one point) and mx_audio_limit_dev of the same build on the 48 kHz hour, ALTERNATING in one
            process.
Every launch of a ratio must write the same bytes (the first and the last 4 MiB of the kept buffer are compared, and those of the
new audio object once).  Prints one JSON line and, with --log, appends it to PATH.  No counters are taken and there is no threshold
on the times: the launches are new.  A tool, not a suite test; run each GPU step of a session under its own time limit."""
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
from conftest import DevBuf, loaded_hip  # noqa: E402
from hip_timing import EDGE, EventTimer, device_image, ends, free_all  # noqa: E402

WARM, RUNS = 3, 10
PAIRS = ((48000, 44100), (44100, 48000), (96000, 48000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    tile = L.levelling_take()[0]
    tile = (tile * np.float32(1.5 / np.abs(tile).max())).astype(np.float32)
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    takes, made = {}, []
    for rate in sorted({p[0] for p in PAIRS}):
        n = int(args.seconds * rate)
        d_img = device_image(np.tile(tile, n // len(tile) + 1)[:n])
        takes[rate] = (d_img, ctx.wrap_device(d_img.ptr, n), n)
    d_pts = DevBuf(8)
    d_pts.write(np.array([(0, 0.5)], dtype=mx.GAIN_POINT_DTYPE))
    outs, first, calls = {}, {}, {}
    for pair in PAIRS:
        a, n = takes[pair[0]][1:]
        m = mx.resample_length(n, *pair)
        outs[pair] = (DevBuf(4 * m), m)
        ctx.resample_dev(a, pair[0], pair[1], 0, m, outs[pair][0].ptr)
        first[pair] = ends(outs[pair][0], m)
        b = ctx.resample(a, *pair)
        k = min(EDGE, m)
        assert ctx.audio_download(b, 0, k).tobytes() + ctx.audio_download(b, m - k, k).tobytes() == first[pair]
        b.free()
        name = f"{pair[0]}_{pair[1]}"
        calls["audio_resample_" + name] = lambda a=a, pair=pair: made.append(ctx.resample(a, *pair))
        calls["resample_dev_" + name] = lambda a=a, pair=pair, m=m: ctx.resample_dev(a, pair[0], pair[1], 0, m, outs[pair][0].ptr)
    a48 = takes[48000][1]
    calls["audio_gain"] = lambda: made.append(ctx.audio_gain_dev(a48, d_pts.ptr, 1))
    calls["audio_limit"] = lambda: made.append(ctx.limit_dev(a48, 48000))
    timer = EventTimer(loaded_hip())
    rows = timer.timed(calls, WARM, RUNS, after=free_all(made))
    for pair in PAIRS:
        assert ends(*outs[pair]) == first[pair], pair  # every launch wrote the same bytes
    res = {"seconds": args.seconds, "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "plans": {f"{p[0]}_{p[1]}": mx.resample_plan(*p) for p in PAIRS},
           "outputs": {f"{p[0]}_{p[1]}": outs[p][1] for p in PAIRS},
           "outputs_per_s": {f"{p[0]}_{p[1]}": outs[p][1] / (rows[f"resample_dev_{p[0]}_{p[1]}"]["median"] * 1e-3) for p in PAIRS},
           "resample_48000_44100_over_audio_gain": rows["resample_dev_48000_44100"]["median"] / rows["audio_gain"]["median"],
           "resample_48000_44100_over_audio_limit": rows["resample_dev_48000_44100"]["median"] / rows["audio_limit"]["median"],
           "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for buf, _ in outs.values():
        buf.free()
    d_pts.free()
    for d_img, a, _ in takes.values():
        a.free()
        d_img.free()
    ctx.close()


if __name__ == "__main__":
    main()
