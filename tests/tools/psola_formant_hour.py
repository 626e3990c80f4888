#!/usr/bin/env python3
"""tests/tools/psola_formant_hour.py [--seconds S] [--semitones ST] [--formant ST] [--log PATH] — the plain PSOLA launch and the
formant launch side by side over psola_hour.py's take (an hour of 48 kHz audio, a synthetic vowel on 150 Hz) retuned by +3 st,
the formant launch with the envelope moved by +3 st as well (step 77936: a wave's 64 consecutive outputs read 76 source
samples apart instead of 64):

  plans   mx_psola_plan and mx_psola_plan_formant on the host, host clock
  kernel  mx_psola_synth_dev and mx_psola_synth_formant_dev ALTERNATING in one process, each between HIP events on the null
          stream: 3 warm-up pairs, then the median (min, max) of 10 of each, both outputs written; and their ratio

A tool, not a suite test: there is no time bound.  Prints one JSON line and, with --log, appends it to PATH."""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from psola_hour import HOP, RUNS, WARM, voiced_take  # noqa: E402  (puts the repository and tests/ on the path)

import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402

_vp = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--semitones", type=float, default=3.0)
    ap.add_argument("--formant", type=float, default=3.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    w = voiced_take(n)
    ctx = mx.Context(0)
    ctx.set_stream(None)  # the null stream: the events bracket exactly the launches
    a = ctx.upload(w)
    track = ctx.f0_track(a, SR, HOP)
    markers = [(1, 0, 0.0, args.semitones), (n - 1, 0, 0.0, args.semitones)]
    t0 = time.perf_counter()
    grains, L = mx.psola_plan(n, SR, HOP, track, markers)
    t_plan = time.perf_counter() - t0
    t0 = time.perf_counter()
    fgrains, fL = mx.psola_plan_formant(n, SR, HOP, track, markers, [(0, args.formant)])
    t_fplan = time.perf_counter() - t0
    assert fL == L and len(fgrains) == len(grains)

    hip = loaded_hip()
    hip.hipEventCreate.argtypes = [C.POINTER(_vp)]
    hip.hipEventRecord.argtypes = [_vp, _vp]
    hip.hipEventSynchronize.argtypes = [_vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), _vp, _vp]
    e0, e1 = _vp(), _vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    d_g, d_fg = DevBuf(grains.nbytes), DevBuf(fgrains.nbytes)
    d_g.write(grains)
    d_fg.write(fgrains)
    d_f, d_i = DevBuf(L * 4), DevBuf(L * 2)

    def one(launch, ptr):
        assert hip.hipEventRecord(e0, None) == 0
        launch(a, ptr, len(grains), L, d_f.ptr, d_i.ptr)
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    ts = {"plain": [], "formant": []}
    for it in range(WARM + RUNS):
        for name, launch, ptr in (("plain", ctx.psola_synth_dev, d_g.ptr), ("formant", ctx.psola_synth_formant_dev, d_fg.ptr)):
            ms = one(launch, ptr)
            if it >= WARM:
                ts[name].append(ms)
    kernel = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ts.items()}
    head = d_f.read(np.float32, offset=4 * SR, count=min(4 * SR, L - SR))  # (the last launch was the formant one)
    res = {"samples": n, "out_samples": L, "sr": SR, "hop": HOP, "semitones": args.semitones, "formant": args.formant,
           "step": int(fgrains["step"][0]), "grains": len(grains), "plan_s": t_plan, "plan_formant_s": t_fplan, "warmups": WARM,
           "launches": RUNS, "kernel_ms": kernel, "formant_over_plain": kernel["formant"]["median"] / kernel["plain"]["median"],
           "algorithmic_bytes": 10 * L, "GB_per_s_at_10_bytes_per_sample": {k: 10 * L / (v["median"] * 1e-3) / 1e9 for k, v in kernel.items()},
           "rms_out_formant": float(np.sqrt(np.mean(head.astype(np.float64) ** 2))), "version": mx._capi.lib().mx_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for b in (d_g, d_fg, d_f, d_i):
        b.free()
    a.free()
    ctx.close()


if __name__ == "__main__":
    main()
