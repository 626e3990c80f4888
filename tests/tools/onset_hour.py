#!/usr/bin/env python3
"""tests/tools/onset_hour.py [--seconds S] [--runs R,R,..] [--log PATH] — the onset-strength kernel over the hour of 48 kHz
audio (172.8 M samples, 675 000 frames at hop 256) of tests/onset_ref.py's six-note take, tiled:
  kernel  between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_onset_flux_dev and
          mx_f0_track_dev on the same frames, ALTERNATING in one process, and their ratio.  The tracker's launch does three
          4096-point transforms per frame and is the yardstick: the flux launch should not take longer.
  runs    the same launch at other run lengths (frames per wavefront; the default is onset_default_run's), each row again
          alternating with the default; the values are asserted byte-equal across the run lengths.
  picks   mx_onset_pick over the hour's curve on the host clock, and the onsets it finds (six per 3 s tile).
Prints one JSON line and, with --log, appends it to PATH.  A tool, not a suite test."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
import onset_ref as R  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image  # noqa: E402

HOP, WARM, RUNS = 256, 3, 10
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


class Lib(TimedLib):
    def __init__(self, path, d_img, n):
        super().__init__(path, d_img, n)
        so = self.so
        so.mx_onset_flux_dev.argtypes = [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp]
        so.mx_f0_track_dev.argtypes = [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp]
        so.mx_ctx_set_frames_per_block.argtypes = [_vp, _i]
        so.mx_ctx_destroy.argtypes = [_vp]
        so.mx_audio_free.argtypes = [_vp, _vp]
        self.frames = -(-n // HOP)
        self.flux, self.f0 = DevBuf(self.frames * 4), DevBuf(self.frames * 16)

    def onset(self, run=0):
        assert self.so.mx_ctx_set_frames_per_block(self.ctx, run) == 0
        assert self.so.mx_onset_flux_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.flux.ptr)) == 0
        assert self.so.mx_ctx_set_frames_per_block(self.ctx, 0) == 0

    def track(self):
        assert self.so.mx_f0_track_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, 55.0, 1760.0, 0.15, _vp(self.f0.ptr)) == 0

    def close(self):
        self.flux.free()
        self.f0.free()
        self.so.mx_audio_free(self.ctx, self.audio)
        self.so.mx_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--runs", default="8,16,64")
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = R.notes(0.005)
    w = np.tile(tile, n // len(tile) + 1)[:n]
    d_img = device_image(w)
    L = Lib(mx._capi.lib()._name, d_img, n)
    timer = EventTimer(loaded_hip())
    rows = {"pair": timer.timed({"onset": L.onset, "f0": L.track}, WARM, RUNS)}
    flux = L.flux.read(np.float32)
    for run in [int(r) for r in args.runs.split(",") if r]:
        rows[f"run_{run}"] = timer.timed({"default": L.onset, "run": lambda run=run: L.onset(run)}, WARM, RUNS)
        assert L.flux.read(np.float32).tobytes() == flux.tobytes(), run  # (the last launch of the row is the run's)
    t0 = time.perf_counter()
    onsets = mx.onset_pick(flux, HOP)
    t_pick = time.perf_counter() - t0
    tiles = n // len(tile)
    res = {"samples": n, "sr": SR, "hop": HOP, "frames": L.frames, "default_run": min(32, max(1, L.frames // 4096)),
           "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "onset_over_f0": rows["pair"]["onset"]["median"] / rows["pair"]["f0"]["median"],
           "frames_per_s": L.frames / (rows["pair"]["onset"]["median"] * 1e-3),
           "pick_s": t_pick, "onsets": len(onsets), "tiles": tiles, "flux_max": float(flux.max()), "lib": L.version}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    L.close()
    d_img.free()
    assert len(onsets) >= 6 * tiles  # every note of every whole tile (a tile's end against the next one's bed may add one)


if __name__ == "__main__":
    main()
