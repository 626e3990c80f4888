#!/usr/bin/env python3
"""tests/tools/key_hour.py [--seconds S] [--log PATH] — the chroma and window-sum kernels and mx_key_detect over the hour of
48 kHz audio (172.8 M samples) of tests/key_ref.py's "C major" take, tiled:
  chroma   between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_chroma_dev at hop 256
           (675 000 frames) and at hop 2048 (84 375 frames) and mx_f0_track_dev of the same build at hop 256, ALTERNATING in one
           process.  One forward transform per frame against the tracker's three and an inverse.
  sums     mx_chroma_sum_dev over the hop-2048 records: windows of 48 frames every 24 and the whole take, in turn with the above.
  host     mx_key_detect (hop 2048, the same windows) on the host clock: the median of 5 calls after one — chroma, sums, the
           download of 320 bytes per job, the host logic; and the key it names.
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

import key_ref as K  # noqa: E402
import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image  # noqa: E402

WARM, RUNS, HOST_RUNS = 3, 10, 5
WINDOW, STRIDE = 48, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = K.takes()["c_major"][0]
    w = np.tile(tile, n // len(tile) + 1)[:n]
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(w)
    a = ctx.wrap_device(d_img.ptr, n)
    f256, f2048 = mx.frame_count(n, 256), mx.frame_count(n, 2048)
    rec256, rec2048, f0 = DevBuf(f256 * 160), DevBuf(f2048 * 160), DevBuf(f256 * 16)
    jobs = np.array(K.windows(f2048, WINDOW, STRIDE) + [(0, f2048)], dtype=np.int64)
    d_jobs, d_sums = DevBuf(jobs.nbytes), DevBuf(len(jobs) * 320)
    d_jobs.write(jobs)
    timer = EventTimer(loaded_hip())
    rows = timer.timed({"chroma_hop256": lambda: ctx.chroma_dev(a, SR, 256, 0, f256, rec256.ptr),
                        "chroma_hop2048": lambda: ctx.chroma_dev(a, SR, 2048, 0, f2048, rec2048.ptr),
                        "f0_track_hop256": lambda: ctx.f0_track_dev(a, SR, 256, 0, f256, f0.ptr),
                        "window_sums": lambda: ctx.chroma_sum_dev(rec2048.ptr, f2048, d_jobs.ptr, len(jobs), d_sums.ptr)}, WARM, RUNS)
    sums = d_sums.read(np.float64).reshape(len(jobs), 40)
    host = []
    for it in range(HOST_RUNS + 1):
        t0 = time.perf_counter()
        key, wins = ctx.key_detect(a, SR, 2048, window_frames=WINDOW, window_hop=STRIDE)
        if it:
            host.append(time.perf_counter() - t0)
    assert key == mx.key_from_chroma(sums[-1]) and len(wins) == len(jobs) - 1
    res = {"samples": n, "sr": SR, "frames_hop256": f256, "frames_hop2048": f2048, "jobs": len(jobs), "warmups": WARM, "launches": RUNS,
           "kernel_ms": rows, "chroma_over_f0_hop256": rows["chroma_hop256"]["median"] / rows["f0_track_hop256"]["median"],
           "frames_per_s_hop256": f256 / (rows["chroma_hop256"]["median"] * 1e-3), "key_detect_s": float(np.median(host)),
           "key": key, "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (rec256, rec2048, f0, d_jobs, d_sums):
        b.free()
    a.free()
    d_img.free()
    ctx.close()
    assert (key["tonic"], key["mode"]) == (3, 0), key


if __name__ == "__main__":
    main()
