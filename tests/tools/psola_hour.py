#!/usr/bin/env python3
"""tests/tools/psola_hour.py [--seconds S] [--semitones ST] [--log PATH] — the PSOLA renderer over the hour of 48 kHz audio
(172.8 M samples) of a synthetic voiced signal (harmonics of 150 Hz under resonances at 700 and 1200 Hz) retuned by +3 st:

  track   mx_f0_track over the whole take (hop 256), host clock around the blocking call
  plan    mx_psola_plan on the host, host clock (the copy of the records into a numpy array included)
  kernel  mx_psola_synth_dev between HIP events on the null stream, 3 warm-up launches, then the median (min, max) of 10:
          both outputs, int16 only, f32 only

and what the kernel time means against the traffic the algorithm needs (4 bytes read and 4 + 2 written per output sample).
A tool, not a suite test: there is no time bound.  Prints one JSON line and, with --log, appends it to PATH."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402

HOP, WARM, RUNS, PERIOD = 256, 3, 10, 320
_vp = C.c_void_p


def voiced_take(n):
    """One period of the vowel (150 Hz at 48 kHz: 320 samples exactly), tiled."""
    t = np.arange(PERIOD) / SR
    one = np.zeros(PERIOD)
    for k in range(1, PERIOD // 2 - 16):
        f = k * SR / PERIOD
        amp = 0.05 / k + 0.6 / (1 + ((f - 700.0) / 90.0) ** 2) + 1.0 / (1 + ((f - 1200.0) / 90.0) ** 2)
        one += amp * np.sin(2 * np.pi * f * t + 0.7 * k * k)
    one = (0.5 * one / np.abs(one).max()).astype(np.float32)
    return np.tile(one, n // PERIOD + 1)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--semitones", type=float, default=3.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    w = voiced_take(n)
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    a = ctx.upload(w)
    t0 = time.perf_counter()
    track = ctx.f0_track(a, SR, HOP)
    t_track = time.perf_counter() - t0
    markers = [(1, 0, 0.0, args.semitones), (n - 1, 0, 0.0, args.semitones)]
    t0 = time.perf_counter()
    grains, L = mx.psola_plan(n, SR, HOP, track, markers)
    t_plan = time.perf_counter() - t0

    hip = loaded_hip()
    hip.hipEventCreate.argtypes = [C.POINTER(_vp)]
    hip.hipEventRecord.argtypes = [_vp, _vp]
    hip.hipEventSynchronize.argtypes = [_vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), _vp, _vp]
    e0, e1 = _vp(), _vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    d_g = DevBuf(grains.nbytes)
    d_g.write(grains)
    d_f, d_i = DevBuf(L * 4), DevBuf(L * 2)

    def timed(f_ptr, i_ptr):
        ts = []
        for it in range(WARM + RUNS):
            assert hip.hipEventRecord(e0, None) == 0
            ctx.psola_synth_dev(a, d_g.ptr, len(grains), L, f_ptr, i_ptr)
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            if it >= WARM:
                ts.append(ms.value)
        return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))

    kernel = {"f32+i16": timed(d_f.ptr, d_i.ptr), "i16": timed(None, d_i.ptr), "f32": timed(d_f.ptr, None)}
    # a spot check that the hour is what the suite checks on seconds: the pitch moved, the level stayed
    head = d_f.read(np.float32, offset=4 * SR, count=4 * SR)
    cover = float(np.diff(grains["centre"].astype(np.float64) + grains["centre_frac"]).mean())
    res = {"samples": n, "out_samples": L, "sr": SR, "hop": HOP, "semitones": args.semitones, "frames": len(track),
           "voiced_frames": int(((track["tau"] > 0) & (track["aperiodicity"] < 0.15)).sum()), "grains": len(grains),
           "mean_grain_spacing": cover, "track_s": t_track, "plan_s": t_plan, "warmups": WARM, "launches": RUNS, "kernel_ms": kernel,
           "algorithmic_bytes": 10 * L, "GB_per_s_at_10_bytes_per_sample": 10 * L / (kernel["f32+i16"]["median"] * 1e-3) / 1e9,
           "rms_in": float(np.sqrt(np.mean(w[4 * SR:8 * SR].astype(np.float64) ** 2))),
           "rms_out": float(np.sqrt(np.mean(head.astype(np.float64) ** 2))), "version": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (d_g, d_f, d_i):
        b.free()
    a.free()
    ctx.close()


if __name__ == "__main__":
    main()
