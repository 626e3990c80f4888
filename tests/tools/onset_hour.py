#!/usr/bin/env python3
"""tests/tools/onset_hour.py [--parent-lib PATH] [--seconds S] [--runs R,R,..] [--log PATH] — the onset-strength kernel over the hour of 48 kHz
audio (172.8 M samples, 675 000 frames at hop 256) of tests/onset_ref.py's six-note take, tiled:
  kernel  between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_onset_flux_dev and
          mx_f0_track_dev on the same frames, ALTERNATING in one process, and their ratio.  The tracker's launch does three
          4096-point transforms per frame and is the yardstick: the flux launch should not take longer.  Then
          mx_sib_features_dev and mx_chroma_dev, the other two frame walkers, on the same frames with default parameters.
  runs    the same launch at other run lengths (frames per wavefront; the default is onset_default_run's), each row again
          alternating with the default; the values are asserted byte-equal across the run lengths.
  host    mx_onset_flux, the host form with its download, on the host clock: the median of 5 calls after one.
  picks   mx_onset_pick over the hour's curve on the host clock, and the onsets it finds (six per 3 s tile).
Every library goes through the same rows in turn, as in psola_hour.py: this tree's and, with --parent-lib, the parent's twice;
the curves are asserted byte-equal across the libraries.  Prints one JSON line and, with --log, appends it to PATH; then, with
--parent-lib, asserts every row's new / parent inside 1 +- 3 delta, delta the run's largest |parent_again / parent - 1| (at
least 0.001).  A tool, not a suite test."""
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
import onset_ref as R  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image, libraries, same_bytes  # noqa: E402

HOP, WARM, RUNS, HOST_RUNS = 256, 3, 10, 5
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


class Lib(TimedLib):
    def __init__(self, path, d_img, n):
        super().__init__(path, d_img, n)
        so = self.so
        so.mx_onset_flux_dev.argtypes = so.mx_onset_flux.argtypes = [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp]
        so.mx_sib_features_dev.argtypes = so.mx_chroma_dev.argtypes = so.mx_onset_flux_dev.argtypes
        so.mx_f0_track_dev.argtypes = [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp]
        so.mx_ctx_set_frames_per_block.argtypes = [_vp, _i]
        so.mx_ctx_destroy.argtypes = [_vp]
        so.mx_audio_free.argtypes = [_vp, _vp]
        self.frames = -(-n // HOP)
        self.flux, self.f0 = DevBuf(self.frames * 4), DevBuf(self.frames * 16)
        self.sib, self.chroma = DevBuf(self.frames * 16), DevBuf(self.frames * 160)
        self.host_flux, self.host_ms = np.empty(self.frames, dtype=np.float32), []

    def onset(self, run=0):
        assert self.so.mx_ctx_set_frames_per_block(self.ctx, run) == 0
        assert self.so.mx_onset_flux_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.flux.ptr)) == 0
        assert self.so.mx_ctx_set_frames_per_block(self.ctx, 0) == 0

    def host(self):
        """One call of the host form on the host clock (appended to host_ms; the first entry is the warm-up)."""
        t0 = time.perf_counter()
        assert self.so.mx_onset_flux(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.host_flux.ctypes.data)) == 0
        self.host_ms.append(1e3 * (time.perf_counter() - t0))

    def track(self):
        assert self.so.mx_f0_track_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, 55.0, 1760.0, 0.15, _vp(self.f0.ptr)) == 0

    def sibilant(self):
        assert self.so.mx_sib_features_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.sib.ptr)) == 0

    def chroma_records(self):
        assert self.so.mx_chroma_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.chroma.ptr)) == 0

    def close(self):
        for buf in (self.flux, self.f0, self.sib, self.chroma):
            buf.free()
        self.so.mx_audio_free(self.ctx, self.audio)
        self.so.mx_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--runs", default="8,16,64")
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = R.notes(0.005)
    w = np.tile(tile, n // len(tile) + 1)[:n]
    d_img = device_image(w)
    libs = libraries(Lib, args.parent_lib, d_img, n)
    new = libs["new"]
    timer = EventTimer(loaded_hip())

    def row(name, method, *a):
        """kernel_ms[name]: lib -> the timed launches of `method`; the rows of one timed() call take turns."""
        return {(name, k): (lambda L=L: getattr(L, method)(*a)) for k, L in libs.items()}

    def timed(calls):
        for (name, k), t in timer.timed(calls, WARM, RUNS).items():
            rows.setdefault(name, {})[k] = t

    rows = {}
    timed({**row("onset", "onset"), **row("f0", "track")})
    timed({**row("sibilant", "sibilant"), **row("chroma", "chroma_records")})
    flux = np.frombuffer(same_bytes(libs, "flux", "f0", "sib", "chroma")[0], dtype=np.float32)
    for run in [int(r) for r in args.runs.split(",") if r]:
        timed({**row(f"run_{run}_default", "onset"), **row(f"run_{run}", "onset", run)})
        assert same_bytes(libs, "flux")[0] == flux.tobytes(), run  # (the last launch of the row is the run's)
    for _ in range(1 + HOST_RUNS):
        for L in libs.values():
            L.host()
    for k, L in libs.items():
        assert L.host_flux.tobytes() == flux.tobytes(), k
        t = L.host_ms[1:]
        rows.setdefault("host_flux", {})[k] = dict(median=float(np.median(t)), min=min(t), max=max(t))
    t0 = time.perf_counter()
    onsets = mx.onset_pick(flux, HOP)
    t_pick = time.perf_counter() - t0
    tiles = n // len(tile)
    res = {"samples": n, "sr": SR, "hop": HOP, "frames": new.frames, "default_run": min(32, max(1, new.frames // 4096)),
           "warmups": WARM, "launches": RUNS, "host_calls": HOST_RUNS, "kernel_ms": rows,
           "onset_over_f0": rows["onset"]["new"]["median"] / rows["f0"]["new"]["median"],
           "frames_per_s": new.frames / (rows["onset"]["new"]["median"] * 1e-3),
           "pick_s": t_pick, "onsets": len(onsets), "tiles": tiles, "flux_max": float(flux.max()),
           "libs": {k: L.version for k, L in libs.items()}, "same_bytes": sorted(libs)}
    if args.parent_lib:
        res["new_vs_parent"] = nvp = {r: t["new"]["median"] / t["parent"]["median"] for r, t in rows.items()}
        res["parent_vs_parent"] = pvp = {r: t["parent_again"]["median"] / t["parent"]["median"] for r, t in rows.items()}
        res["delta"] = delta = max(0.001, max(abs(v - 1.0) for v in pvp.values()))
        res["rows_outside_1_pm_3_delta"] = missed = sorted(r for r, v in nvp.items() if abs(v - 1.0) > 3 * delta)
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for L in libs.values():
        L.close()
    d_img.free()
    assert len(onsets) >= 6 * tiles  # every note of every whole tile (a tile's end against the next one's bed may add one)
    if args.parent_lib:  # (after the line is out: a run that misses the bound is still on record)
        assert not missed, f"new / parent outside 1 +- 3 x {delta:.4f}: {missed}"


if __name__ == "__main__":
    main()
