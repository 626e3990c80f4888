#!/usr/bin/env python3
"""tests/tools/psola_hour.py [--parent-lib PATH] [--seconds S] [--semitones ST] [--formant ST] [--log PATH] — the PSOLA renderer
over the hour of 48 kHz audio (172.8 M samples) of a synthetic vowel on 150 Hz retuned by +3 st, plain and with the envelope
moved by +3 st as well (step 77936: a wave's 64 consecutive outputs read 76 source samples apart instead of 64):
  track   mx_f0_track over the whole take (hop 256), host clock around the blocking call
  plans   mx_psola_plan and mx_psola_plan_formant, host clock (the copy into numpy included), a warm-up and 5 runs of each
  kernel  between HIP events on the null stream, the median (min, max) of 10 launches after 3: mx_psola_synth_dev with both
          outputs, int16 only, f32 only; then it and mx_psola_synth_formant_dev ALTERNATING, both outputs, and their ratio
and the kernel time against the traffic the algorithm needs (4 bytes read and 4 + 2 written per output sample).
Every library goes through the same rows in turn, as in f0_decode_hour.py: this tree's and, with --parent-lib, the parent's
twice (new_vs_parent beside the run's noise floor parent_vs_parent); the records of the two plans and the PCM of the two renders
are asserted byte-equal across the libraries.  Prints one JSON line and, with --log, appends it to PATH; then, with
--parent-lib, asserts new_vs_parent <= parent_vs_parent + 0.01 for every launch row and, for either plan, the new median <= the
parent's slowest run.  A tool, not a suite test."""
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
from hip_timing import EventTimer, TimedLib, device_image, libraries, same_bytes  # noqa: E402

HOP, WARM, RUNS, PLAN_RUNS, PERIOD = 256, 3, 10, 5, 320
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
PLAN_ARGS = [_i64, _i, _i, _vp, _i64, _vp, _vp, _i]
PLAN_OUTS = [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64)]
KINDS = {"plain": ("", mx.PSOLA_GRAIN_DTYPE), "formant": ("_formant", mx.PSOLA_FGRAIN_DTYPE)}


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


class Lib(TimedLib):
    """One library's context, its handle on the shared device image, its plans and its own record and output buffers."""

    def __init__(self, path, d_img, n):
        super().__init__(path, d_img, n)
        so = self.so
        so.mx_psola_plan.argtypes = PLAN_ARGS + PLAN_OUTS
        so.mx_psola_plan_formant.argtypes = PLAN_ARGS + [_vp, _i] + PLAN_OUTS
        so.mx_psola_synth_dev.argtypes = so.mx_psola_synth_formant_dev.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _vp]
        so.mx_free.argtypes = so.mx_ctx_destroy.argtypes = [_vp]
        so.mx_audio_free.argtypes = [_vp, _vp]
        self.records, self.plan_s, self.d_records = {}, {}, {}

    def plan(self, kind, track, markers, points):
        """One plan of `kind` on the host clock (appended to plan_s[kind]); keeps its records."""
        sfx, dtype = KINDS[kind]
        m = mx._capi.markers_array(markers)
        extra = [_vp(points.ctypes.data), len(points)] if kind == "formant" else []
        out, cnt, L = _vp(), _i64(), _i64()
        t0 = time.perf_counter()
        assert getattr(self.so, "mx_psola_plan" + sfx)(self.n, SR, HOP, _vp(track.ctypes.data), len(track), None, m, len(markers),
                                                       *extra, C.byref(out), C.byref(cnt), C.byref(L)) == 0
        self.records[kind] = np.frombuffer(C.string_at(out, cnt.value * dtype.itemsize), dtype=dtype).copy()
        self.plan_s.setdefault(kind, []).append(time.perf_counter() - t0)
        self.so.mx_free(out)
        self.L = L.value

    def close(self):
        for b in (self.f32, self.i16, *self.d_records.values()):
            b.free()
        self.so.mx_audio_free(self.ctx, self.audio)
        self.so.mx_ctx_destroy(self.ctx)

    def synth(self, kind, f32=True, i16=True):
        assert getattr(self.so, f"mx_psola_synth{KINDS[kind][0]}_dev")(
            self.ctx, self.audio, _vp(self.d_records[kind].ptr), len(self.records[kind]), self.L, _vp(self.f32.ptr) if f32 else None,
            _vp(self.i16.ptr) if i16 else None) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--semitones", type=float, default=3.0)
    ap.add_argument("--formant", type=float, default=3.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    w = voiced_take(n)
    d_img = device_image(w)
    ctx = mx.Context(0)
    a = ctx.wrap_device(d_img.ptr, n)
    t0 = time.perf_counter()
    track = ctx.f0_track(a, SR, HOP)
    t_track = time.perf_counter() - t0
    a.free()
    ctx.close()

    libs = libraries(Lib, args.parent_lib, d_img, n)
    markers = [(1, 0, 0.0, args.semitones), (n - 1, 0, 0.0, args.semitones)]
    points = mx._formant_points([(0, args.formant)])
    new = libs["new"]
    for _ in range(1 + PLAN_RUNS):  # (the libraries in turn here too; plan_s keeps the warm-up run as its first entry)
        for L in libs.values():
            for kind in KINDS:
                L.plan(kind, track, markers, points)
    for L in libs.values():
        L.f32, L.i16 = DevBuf(L.L * 4), DevBuf(L.L * 2)
        for kind, rec in L.records.items():
            L.d_records[kind] = DevBuf(rec.nbytes)
            L.d_records[kind].write(rec)
        assert L.L == new.L and all(L.records[k].tobytes() == new.records[k].tobytes() for k in KINDS)  # the same plans ...
        assert len(L.records["formant"]) == len(L.records["plain"])  # ... a formant record per plain one
    grains, L_out = new.records["plain"], new.L

    timer = EventTimer(loaded_hip())
    rows = {}
    # the plain launch and its output selections
    for row, f32, i16 in (("f32+i16", True, True), ("i16", False, True), ("f32", True, False)):
        rows[row] = timer.timed({k: (lambda L=L: L.synth("plain", f32, i16)) for k, L in libs.items()}, WARM, RUNS)
    same_bytes(libs, "f32", "i16")
    # a spot check that the hour is what the suite checks on seconds: the pitch moved, the level stayed
    head = new.f32.read(np.float32, offset=4 * SR, count=min(4 * SR, L_out - SR))
    # the plain and the formant launch alternating, in every library in turn; the formant one comes last
    pair = timer.timed({(k, kind): (lambda L=L, kind=kind: L.synth(kind)) for k, L in libs.items() for kind in KINDS}, WARM, RUNS)
    for kind in KINDS:
        rows["pair_" + kind] = {k: pair[(k, kind)] for k in libs}
    same_bytes(libs, "f32", "i16")
    fhead = new.f32.read(np.float32, offset=4 * SR, count=min(4 * SR, L_out - SR))

    def rms(x):
        return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))

    res = {"samples": n, "out_samples": L_out, "sr": SR, "hop": HOP, "semitones": args.semitones, "formant": args.formant,
           "frames": len(track), "voiced_frames": int(((track["tau"] > 0) & (track["aperiodicity"] < 0.15)).sum()),
           "grains": len(grains), "step": int(new.records["formant"]["step"][0]),
           "mean_grain_spacing": float(np.diff(grains["centre"].astype(np.float64) + grains["centre_frac"]).mean()),
           "track_s": t_track, "plan_s": {k: L.plan_s["plain"] for k, L in libs.items()},
           "plan_formant_s": {k: L.plan_s["formant"] for k, L in libs.items()}, "warmups": WARM, "launches": RUNS, "kernel_ms": rows,
           "formant_over_plain": rows["pair_formant"]["new"]["median"] / rows["pair_plain"]["new"]["median"],
           "algorithmic_bytes": 10 * L_out, "GB_per_s_at_10_bytes_per_sample": 10 * L_out / (rows["f32+i16"]["new"]["median"] * 1e-3) / 1e9,
           "rms_in": rms(w[4 * SR:8 * SR]), "rms_out": rms(head), "rms_out_formant": rms(fhead),
           "libs": {k: L.version for k, L in libs.items()}, "same_bytes": sorted(libs)}
    if args.parent_lib:
        res["new_vs_parent"] = nvp = {r: t["new"]["median"] / t["parent"]["median"] for r, t in rows.items()}
        res["parent_vs_parent"] = pvp = {r: t["parent_again"]["median"] / t["parent"]["median"] for r, t in rows.items()}
    line = json.dumps(res)
    print(line)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    for L in libs.values():
        L.close()
    d_img.free()
    if args.parent_lib:  # (after the line is out: a run that misses a bound is still on record)
        assert all(nvp[r] <= pvp[r] + 0.01 for r in rows), "a launch row is more than 1 % over the run's own noise floor"
        for kind in KINDS:  # the new median of the timed plans against the parent's slowest one
            assert np.median(new.plan_s[kind][1:]) <= max(libs["parent"].plan_s[kind][1:]), f"{kind} plan slower than the parent's"


if __name__ == "__main__":
    main()
