#!/usr/bin/env python3
"""tests/tools/sibilant_hour.py [--seconds S] [--log PATH] — the sibilant-feature and source-gain kernels over the hour of
48 kHz audio (172.8 M samples, 675 000 frames at hop 256) of tests/sibilant_ref.py's synthetic take, tiled:
  features  between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_sib_features_dev and
            mx_onset_flux_dev of the same build on the same frames, ALTERNATING in one process, and their ratio.  The same
            transform without log1pf, 16 instead of 4 bytes written per frame: the ratio should be near 1.
  gain      mx_audio_gain_dev over the hour with the balance points of the hour's sibilants, alternating with the granular
            resampler's launch (mx_resynth_dev, the identity schedule of the same samples); GB/s on the gain's 8 algorithmic
            bytes per sample.  The call allocates its output: the events bracket the two pad clears and the kernel, not the
            allocation, and every output is freed after its launch.
  host      mx_sibilants over the hour's records on the host clock, and the segments it finds (three per 2 s tile).
Prints one JSON line and, with --log, appends it to PATH.  No counters are taken.  A tool, not a suite test."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
import sibilant_ref as S  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image, free_all  # noqa: E402

HOP, WARM, RUNS = 256, 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = S.take()[0]
    w = np.tile(tile, n // len(tile) + 1)[:n]
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(w)
    a = ctx.wrap_device(d_img.ptr, n)
    frames = mx.frame_count(n, HOP)
    feat, flux = DevBuf(frames * 16), DevBuf(frames * 4)
    timer = EventTimer(loaded_hip())
    rows = timer.timed({"features": lambda: ctx.sib_features_dev(a, SR, HOP, 0, frames, feat.ptr),
                        "onset_flux": lambda: ctx.onset_flux_dev(a, SR, HOP, 0, frames, flux.ptr)}, WARM, RUNS)
    records = feat.read(mx.SIB_FEAT_DTYPE)
    t0 = time.perf_counter()
    sibs = mx.sibilants(records, HOP)
    t_seg = time.perf_counter() - t0
    pts = mx.sibilant_gain_points(sibs, -6.0, SR // 100, n)
    d_pts = DevBuf(max(pts.nbytes, 8))
    d_pts.write(pts)
    starts, lens = ctx.grains_dev(a)
    steps, total = mx.schedule_build(w, SR, starts, lens, [(1, 0, 0, 0.0), (n - 1, 0, 0, 0.0)])
    d_steps, d_pcm = DevBuf(steps.nbytes), DevBuf(total * 4)
    d_steps.write(steps)
    made = []

    def gain():
        made.append(ctx.audio_gain_dev(a, d_pts.ptr, len(pts)))

    rows.update(timer.timed({"gain": gain, "granular": lambda: ctx.resynth_dev(a, d_steps.ptr, len(steps), total, d_pcm.ptr, None)},
                            WARM, RUNS, after=free_all(made)))
    tiles = n // len(tile)
    res = {"samples": n, "sr": SR, "hop": HOP, "frames": frames, "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "features_over_onset_flux": rows["features"]["median"] / rows["onset_flux"]["median"],
           "frames_per_s": frames / (rows["features"]["median"] * 1e-3),
           "gain_GBps": 8.0 * n / (rows["gain"]["median"] * 1e-3) / 1e9, "gain_over_granular": rows["gain"]["median"] / rows["granular"]["median"],
           "gain_points": len(pts), "segments_s": t_seg, "sibilants": len(sibs), "tiles": tiles, "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (feat, flux, d_pts, d_steps, d_pcm):
        b.free()
    a.free()
    d_img.free()
    ctx.close()
    assert len(sibs) >= 3 * tiles - 1, (len(sibs), tiles)


if __name__ == "__main__":
    main()
