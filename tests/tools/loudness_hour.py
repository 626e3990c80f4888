#!/usr/bin/env python3
"""tests/tools/loudness_hour.py [--seconds S] [--log PATH] — the loudness-record kernel over the hour of 48 kHz audio (172.8 M
samples, 360 000 steps in 36 000 groups) of tests/loudness_ref.py's levelling take, tiled:
  kernels   between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_loudness_steps_dev,
            mx_audio_gain_dev (with the levelling points of the hour's notes; the call allocates its output: the events bracket
            the two pad clears and the kernel, not the allocation, and every output is freed after its launch) and
            mx_onset_flux_dev at hop 256 of the same build on the same samples, ALTERNATING in one process.
  host      mx_loudness_integrated over the hour's records on the host clock, mx_note_loudness and mx_level_gain_points over the
            hour's notes (five per tile, from the take's truth).
Prints one JSON line and, with --log, appends it to PATH.  No counters are taken and there is no threshold on the times: the
launch is new.  A tool, not a suite test; run each GPU step of a session under its own time limit."""
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
import loudness_ref as L  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, device_image, free_all  # noqa: E402

HOP, WARM, RUNS = 256, 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile, truth = L.levelling_take()
    tiles = n // len(tile)
    w = np.tile(tile, tiles + 1)[:n]
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    d_img = device_image(w)
    a = ctx.wrap_device(d_img.ptr, n)
    steps = mx.loudness_step_count(n, SR)
    groups = -(-steps // mx.LOUD_GROUP_STEPS)
    frames = mx.frame_count(n, HOP)
    rec, flux = DevBuf(steps * 16), DevBuf(frames * 4)
    ctx.loudness_steps_dev(a, SR, 0, groups, rec.ptr)
    records = rec.read(mx.LOUD_STEP_DTYPE)
    t0 = time.perf_counter()
    measured = mx.loudness_integrated(records, SR)
    t_int = time.perf_counter() - t0
    notes = np.zeros(5 * tiles, dtype=mx.NOTE_DTYPE)
    at = np.repeat(np.arange(tiles, dtype=np.int64) * len(tile), 5)
    notes["start_sample"] = at + np.tile([lo + 480 for lo, _ in truth], tiles)
    notes["end_sample"] = at + np.tile([hi - 481 for _, hi in truth], tiles)
    t0 = time.perf_counter()
    lufs = mx.note_loudness(records, SR, notes)
    pts, reference = mx.level_gain_points(notes, lufs)
    t_level = time.perf_counter() - t0
    d_pts = DevBuf(max(pts.nbytes, 8))
    d_pts.write(pts)
    made = []
    timer = EventTimer(loaded_hip())
    calls = {"loudness_steps": lambda: ctx.loudness_steps_dev(a, SR, 0, groups, rec.ptr),
             "audio_gain": lambda: made.append(ctx.audio_gain_dev(a, d_pts.ptr, len(pts))),
             "onset_flux": lambda: ctx.onset_flux_dev(a, SR, HOP, 0, frames, flux.ptr)}
    rows = timer.timed(calls, WARM, RUNS, after=free_all(made))
    assert rec.read(mx.LOUD_STEP_DTYPE).tobytes() == records.tobytes()  # every launch wrote the same bytes
    res = {"samples": n, "sr": SR, "steps": steps, "groups": groups, "frames": frames, "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "loudness_over_onset_flux": rows["loudness_steps"]["median"] / rows["onset_flux"]["median"],
           "loudness_over_audio_gain": rows["loudness_steps"]["median"] / rows["audio_gain"]["median"],
           "samples_per_s": n / (rows["loudness_steps"]["median"] * 1e-3), "integrated_s": t_int, "integrated_lufs": measured["integrated"],
           "blocks": measured["blocks"], "passed_rel": measured["passed_rel"], "notes": len(notes), "level_points_s": t_level,
           "reference_lufs": reference, "tiles": tiles, "lib": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (rec, flux, d_pts):
        b.free()
    a.free()
    d_img.free()
    ctx.close()
    assert measured["bad_blocks"] == 0 and measured["passed_rel"] > 0 and np.all(np.isfinite(lufs)), measured


if __name__ == "__main__":
    main()
