#!/usr/bin/env python3
"""tests/tools/tempo_hour.py [--seconds S] [--other-lib PATH] [--log PATH] — the tempo estimator's launches over the hour of 48 kHz audio (172.8 M
samples, 675 000 frames at hop 256) of tests/onset_ref.py's six-note take, tiled as tests/tools/onset_hour.py tiles it, the
flux already in HBM:
  kernel  between HIP events on the null stream, the median (min, max) of 10 launches after 3, each row ALTERNATING in one
          process with mx_onset_flux_dev over the same frames, the yardstick: the smoothing launch (mx_tempo_smooth_dev), the
          coarse comb launch (mx_tempo_comb_dev: every window x every candidate) and the comb launch of each refinement level.
          The stages' job lists are the estimate's own: tests/tempo_ref.py's estimate() runs with its stages on the GPU and is
          asserted equal to mx_tempo_from_flux field for field.
  host    mx_tempo_from_flux over the hour's curve on the host clock: the median of 5 calls after one.
  other   with --other-lib (another build of the library, e.g. one compiled with -DMX_TEMPO_FETCH=1, the plain one-term-at-a-
          time loop): every comb stage of the two libraries ALTERNATING launch by launch in this one process, and the whole
          mx_tempo_from_flux of each in turn; the records are asserted byte-equal across the two.
Says which refinement levels take longer than the coarse launch (their phases sum thousands of terms on fewer than 256 lanes).
Prints one JSON line and, with --log, appends it to PATH.  No counters, nothing on recordings.  A tool, not a suite test."""
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
import tempo_ref as T  # noqa: E402
from conftest import SR, DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image  # noqa: E402

HOP, WARM, RUNS, HOST_RUNS = 256, 3, 10, 5
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64


class Lib(TimedLib):
    def __init__(self, path, d_img, n):
        super().__init__(path, d_img, n)
        so = self.so
        so.mx_onset_flux_dev.argtypes = [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp]
        so.mx_tempo_smooth_dev.argtypes = [_vp, _vp, _i64, _i, _vp]
        so.mx_tempo_comb_dev.argtypes = [_vp, _vp, _i64, _vp, _i64, _vp]
        so.mx_tempo_from_flux.argtypes = [_vp, _vp, _i64, _i, _i, _i64, _vp, _vp, _vp, _vp]
        so.mx_ctx_destroy.argtypes = [_vp]
        so.mx_audio_free.argtypes = [_vp, _vp]
        self.frames = -(-n // HOP)
        self.flux, self.scratch, self.curve = (DevBuf(self.frames * 4) for _ in range(3))
        self.stages = []  # (name, jobs DevBuf, njobs, records DevBuf)

    def onset(self):
        assert self.so.mx_onset_flux_dev(self.ctx, self.audio, SR, HOP, 0, self.frames, None, _vp(self.scratch.ptr)) == 0

    def smooth(self, W):
        assert self.so.mx_tempo_smooth_dev(self.ctx, _vp(self.flux.ptr), self.frames, W, _vp(self.curve.ptr)) == 0

    def add_stage(self, name, jobs):
        j = np.array(jobs, dtype=mx.COMB_JOB_DTYPE)
        dj, do = DevBuf(j.nbytes), DevBuf(len(j) * 16)
        dj.write(j)
        self.stages.append((name, dj, len(j), do, j))
        return len(self.stages) - 1

    def comb(self, k):
        _, dj, nj, do, _ = self.stages[k]
        assert self.so.mx_tempo_comb_dev(self.ctx, _vp(self.curve.ptr), self.frames, _vp(dj.ptr), nj, _vp(do.ptr)) == 0

    def close(self):
        for b in [self.flux, self.scratch, self.curve] + [s[1] for s in self.stages] + [s[3] for s in self.stages]:
            b.free()
        self.so.mx_audio_free(self.ctx, self.audio)
        self.so.mx_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--other-lib")
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    tile = R.notes(0.005)
    w = np.tile(tile, n // len(tile) + 1)[:n]
    d_img = device_image(w)
    L = Lib(mx._capi.lib()._name, d_img, n)
    timer = EventTimer(loaded_hip())
    hip = loaded_hip()
    p = mx.tempo_params_default()

    # the flux stays in HBM; the host copy is only what the reference estimate and mx_tempo_from_flux are handed
    assert L.so.mx_onset_flux_dev(L.ctx, L.audio, SR, HOP, 0, L.frames, None, _vp(L.flux.ptr)) == 0
    flux = L.flux.read(np.float32)

    def smooth_fn(_, W):
        L.smooth(W)
        return L.curve.read(np.float32)

    def comb_fn(_, jobs):
        k = L.add_stage("coarse" if not L.stages else f"level_{len(L.stages)}", jobs)
        L.comb(k)
        rec = L.stages[k][3].read(mx.COMB_DTYPE)
        return list(zip(rec["score"], rec["phase"].tolist(), rec["prev"], rec["next"]))

    t0 = time.perf_counter()
    want = T.estimate(flux, SR, HOP, smooth_fn=smooth_fn, comb_fn=comb_fn)
    t_python = time.perf_counter() - t0
    assert hip.hipDeviceSynchronize() == 0

    rows = {}
    for name, call in [("smooth", lambda: L.smooth(p["smooth"]))] + [(s[0], (lambda k=k: L.comb(k))) for k, s in enumerate(L.stages)]:
        t = timer.timed({name: call, "onset_flux": L.onset}, WARM, RUNS)
        rows[name] = dict(t[name], onset_flux=t["onset_flux"], over_onset_flux=t[name]["median"] / t["onset_flux"]["median"])
    libs = {"new": L}
    if args.other_lib:
        libs["other"] = O = Lib(args.other_lib, d_img, n)
        assert O.so.mx_onset_flux_dev(O.ctx, O.audio, SR, HOP, 0, O.frames, None, _vp(O.flux.ptr)) == 0
        O.smooth(p["smooth"])
        assert O.curve.read(np.uint8).tobytes() == L.curve.read(np.uint8).tobytes()
        versus = {}
        for k, st in enumerate(L.stages):
            assert O.add_stage(st[0], st[4]) == k
            t = timer.timed({"new": (lambda k=k: L.comb(k)), "other": (lambda k=k: O.comb(k))}, WARM, RUNS)
            assert O.stages[k][3].read(np.uint8).tobytes() == st[3].read(np.uint8).tobytes(), st[0]  # the same records
            versus[st[0]] = dict(t, new_over_other=t["new"]["median"] / t["other"]["median"])
    host_ms, got = {k: [] for k in libs}, None
    for _ in range(1 + HOST_RUNS):
        for name, B in libs.items():
            t, win, nwin = mx._capi.Tempo(), _vp(), _i64()
            t0 = time.perf_counter()
            assert B.so.mx_tempo_from_flux(B.ctx, _vp(flux.ctypes.data), len(flux), SR, HOP, 0, None, C.byref(t), C.byref(win), C.byref(nwin)) == 0
            host_ms[name].append(1e3 * (time.perf_counter() - t0))
            got = ({k: getattr(t, k) for k, _ in mx._capi.Tempo._fields_}, mx._take_records(win, nwin.value, mx.TEMPO_WINDOW_DTYPE))
            T.same_estimate(got, want)
    host_other = host_ms.get("other")
    host_ms = host_ms["new"]
    res = {"samples": n, "sr": SR, "hop": HOP, "frames": L.frames, "warmups": WARM, "launches": RUNS, "host_calls": HOST_RUNS,
           "jobs": {s[0]: s[2] for s in L.stages}, "kernel_ms": rows,
           "levels_slower_than_coarse": sorted(k for k in rows if k.startswith("level_") and rows[k]["median"] > rows["coarse"]["median"]),
           "host_from_flux_ms": dict(median=float(np.median(host_ms[1:])), min=min(host_ms[1:]), max=max(host_ms[1:])),
           "reference_with_gpu_stages_s": t_python, "estimate": {k: float(v) for k, v in got[0].items()}, "windows": len(got[1]),
           "lib": L.version, "same_fields_as_reference": True}
    if args.other_lib:
        res["other"] = {"lib": libs["other"].version, "kernel_ms": versus, "same_records": True,
                        "host_from_flux_ms": dict(median=float(np.median(host_other[1:])), min=min(host_other[1:]), max=max(host_other[1:]))}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for B in libs.values():
        B.close()
    d_img.free()


if __name__ == "__main__":
    main()
