#!/usr/bin/env python3
"""tests/tools/take_forms_hour.py [PARENT_LIB] [--seconds S] [--log PATH] — the call forms of the take processors (sample-rate
conversion, noise reduction, compressor) over the hour at 48 kHz (tests/denoise_ref.py's vowel take, tiled: 172.8 M samples): this
tree's library and, with PARENT_LIB (a path to another build's libmelonix_amd.so), that one twice, on one device image.
  device  the whole take: mx_resample_dev 48000 -> 44100, mx_denoise_dev (f32), mx_compress_dev (f32 + int16),
          mx_compress_gain_dev over every step, mx_noise_print_dev over the first 2 s, and mx_audio_resample, mx_audio_denoise,
          mx_audio_compress, each object freed after its launch.
  host    one second of outputs through the host forms, whose wrapper is what a change of the call forms touches: mx_resample,
          mx_denoise, mx_compress, mx_compress_gain, and mx_noise_print over the first 2 s.
  refused a fixed list of bad calls — null handles, bad span, null output, misaligned output, bad rate, bad parameters, per entry
          point, and calls wrong twice over — through each library: the status and the mx_last_error() text must be equal.
The libraries take turns call by call between HIP events on the null stream (tests/hip_timing.py's loop): 3 warm-ups, then the
median (min, max) of 10.  Every output is asserted byte-equal across the libraries: the kept buffers whole, read back once per
library before the timing, the host outputs, and the objects' samples and pads.  Prints one JSON line and, with --log, appends it
to PATH; then, with PARENT_LIB, asserts every row's new / parent inside 1 +- 3 delta, delta the run's largest |parent_again / parent
- 1| (at least 0.001): the margin is the parent's own run-to-run spread, measured in the same process.  A tool, not a suite test."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
import denoise_ref as D  # noqa: E402
from conftest import DevBuf, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image, libraries, same_bytes  # noqa: E402

WARM, RUNS = 3, 10
SR, OUT_SR = 48000, 44100
PAD = mx.MX_AUDIO_PAD
vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
DN = mx._capi.DenoiseParams(12.0, 6.0)


def P(a):
    return vp(a.ctypes.data) if a is not None else None


class Lib(TimedLib):
    def __init__(self, path, d_img, n):
        super().__init__(path, d_img, n)
        so = self.so
        so.mx_resample_dev.argtypes = so.mx_resample.argtypes = [vp, vp, i32, i32, i64, i64, vp]
        so.mx_denoise_dev.argtypes = so.mx_denoise.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp]
        so.mx_compress_dev.argtypes = so.mx_compress.argtypes = [vp, vp, i32, vp, i64, i64, vp, vp]
        so.mx_compress_gain_dev.argtypes = so.mx_compress_gain.argtypes = [vp, vp, i32, vp, i64, i64, vp]
        so.mx_compress_peaks_dev.argtypes = [vp, vp, i32, i64, i64, vp]
        so.mx_noise_print_dev.argtypes = so.mx_noise_print.argtypes = so.mx_noise_rows_dev.argtypes = [vp, vp, i64, i64, vp]
        so.mx_audio_resample.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
        so.mx_audio_denoise.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        so.mx_audio_compress.argtypes = [vp, vp, i32, vp, C.POINTER(vp)]
        so.mx_audio_download.argtypes = [vp, vp, i64, i64, vp]
        so.mx_audio_length.argtypes, so.mx_audio_length.restype = [vp], i64
        so.mx_audio_free.argtypes = [vp, vp]
        so.mx_ctx_destroy.argtypes = [vp]
        so.mx_last_error.restype = C.c_char_p
        self.m, self.steps = mx.resample_length(n, SR, OUT_SR), mx.compress_steps(n, SR)
        self.resampled, self.clean = DevBuf(4 * self.m), DevBuf(4 * n)
        self.f32, self.i16, self.gain, self.print = DevBuf(4 * n), DevBuf(2 * n), DevBuf(4 * self.steps), DevBuf(4 * mx.DENOISE_BINS)
        self.made, self.host = [], {}

    class Made:
        def __init__(self, L, handle):
            self.L, self.handle = L, handle

        def free(self):
            self.L.so.mx_audio_free(self.L.ctx, self.handle)

    def ok(self, rc):
        assert rc == 0, (rc, self.so.mx_last_error())

    # the device forms of the whole take (P0: the host print every denoise call reads)
    def resample_dev(self):
        self.ok(self.so.mx_resample_dev(self.ctx, self.audio, SR, OUT_SR, 0, self.m, vp(self.resampled.ptr)))

    def denoise_dev(self, P0):
        self.ok(self.so.mx_denoise_dev(self.ctx, self.audio, P(P0), C.byref(DN), 0, self.n, vp(self.clean.ptr), None))

    def compress_dev(self):
        self.ok(self.so.mx_compress_dev(self.ctx, self.audio, SR, None, 0, self.n, vp(self.f32.ptr), vp(self.i16.ptr)))

    def compress_gain_dev(self):
        self.ok(self.so.mx_compress_gain_dev(self.ctx, self.audio, SR, None, 0, self.steps, vp(self.gain.ptr)))

    def noise_print_dev(self):
        self.ok(self.so.mx_noise_print_dev(self.ctx, self.audio, 0, 2 * SR, vp(self.print.ptr)))

    def make(self, name, *args):
        """The object of mx_audio_<name> -> self.made, for the caller to free."""
        h = vp()
        self.ok(getattr(self.so, "mx_audio_" + name)(self.ctx, self.audio, *args, C.byref(h)))
        self.made.append(Lib.Made(self, h))

    def audio_digest(self, name, *args):
        """-> (the object's length, a digest of its samples and both pads)."""
        self.make(name, *args)
        b = self.made.pop()
        length = self.so.mx_audio_length(b.handle)
        all_ = np.empty(length + 2 * PAD, dtype=np.float32)
        self.ok(self.so.mx_audio_download(self.ctx, b.handle, -PAD, len(all_), P(all_)))
        b.free()
        return length, hashlib.sha1(all_.tobytes()).hexdigest()

    # the host forms over one second of outputs
    def resample(self):
        out = self.host["resample"] = np.empty(OUT_SR, dtype=np.float32)
        self.ok(self.so.mx_resample(self.ctx, self.audio, SR, OUT_SR, 0, len(out), P(out)))

    def denoise(self, P0):
        out = self.host["denoise"] = (np.empty(SR, dtype=np.float32), np.empty(SR, dtype=np.int16))
        self.ok(self.so.mx_denoise(self.ctx, self.audio, P(P0), C.byref(DN), 0, SR, P(out[0]), P(out[1])))

    def compress(self):
        out = self.host["compress"] = (np.empty(SR, dtype=np.float32), np.empty(SR, dtype=np.int16))
        self.ok(self.so.mx_compress(self.ctx, self.audio, SR, None, 0, SR, P(out[0]), P(out[1])))

    def compress_gain(self):
        out = self.host["compress_gain"] = np.empty(mx.compress_steps(SR, SR), dtype=np.int32)
        self.ok(self.so.mx_compress_gain(self.ctx, self.audio, SR, None, 0, len(out), P(out)))

    def noise_print(self):
        out = self.host["noise_print"] = np.empty(mx.DENOISE_BINS, dtype=np.float32)
        self.ok(self.so.mx_noise_print(self.ctx, self.audio, 0, 2 * SR, P(out)))

    def refused(self, P0):
        """The bad calls -> [(what, status, message)]; none reaches a launch (one is no refusal: an empty range asks nothing of
        the pointer of mx_resample_dev, misaligned or not)."""
        so, c, a, n = self.so, self.ctx, self.audio, self.n
        f, h = vp(self.f32.ptr), vp(self.i16.ptr)
        f_odd, h_odd, g_odd, p_odd = vp(self.f32.ptr + 2), vp(self.i16.ptr + 1), vp(self.gain.ptr + 2), vp(self.print.ptr + 2)
        host_f, host_h, host_g = np.empty(16, np.float32), np.empty(16, np.int16), np.empty(16, np.int32)
        host_p = np.empty(mx.DENOISE_BINS, np.float32)
        hf, hh, hg = P(host_f), P(host_h), P(host_g)
        pr, dn, dn_bad = P(P0), C.byref(DN), C.byref(mx._capi.DenoiseParams(99.0, 6.0))
        cp_bad = C.byref(mx._capi.CompressParams(-18.0, 0.5, 6.0, 5.0, 100.0, 0.0, 1.0))
        obj = vp()
        calls = []
        for name, out, odd in (("mx_resample", hf, None), ("mx_resample_dev", f, f_odd)):
            fn = getattr(so, name)
            calls += [(name, "null context", lambda fn=fn, out=out: fn(None, a, SR, OUT_SR, 0, 16, out)),
                      (name, "null audio", lambda fn=fn, out=out: fn(c, None, SR, OUT_SR, 0, 16, out)),
                      (name, "bad rate", lambda fn=fn, out=out: fn(c, a, 0, OUT_SR, 0, 16, out)),
                      (name, "too many phases", lambda fn=fn, out=out: fn(c, a, 8000, 383999, 0, 16, out)),
                      (name, "span before the take", lambda fn=fn, out=out: fn(c, a, SR, OUT_SR, -1, 16, out)),
                      (name, "span past the take", lambda fn=fn, out=out: fn(c, a, SR, OUT_SR, self.m - 8, 16, out)),
                      (name, "null output", lambda fn=fn: fn(c, a, SR, OUT_SR, 0, 16, None)),
                      (name, "bad rate and bad span", lambda fn=fn, out=out: fn(c, a, 0, OUT_SR, -1, 16, out))]
            if odd:
                calls += [(name, "misaligned", lambda fn=fn, odd=odd: fn(c, a, SR, OUT_SR, 0, 16, odd)),
                          (name, "misaligned, empty range", lambda fn=fn, odd=odd: fn(c, a, SR, OUT_SR, 0, 0, odd)),
                          (name, "bad span and misaligned", lambda fn=fn, odd=odd: fn(c, a, SR, OUT_SR, -1, 16, odd))]
        for name, of, oh, odd_f, odd_h in (("mx_denoise", hf, hh, None, None), ("mx_denoise_dev", f, h, f_odd, h_odd)):
            fn = getattr(so, name)
            calls += [(name, "null context", lambda fn=fn, of=of: fn(None, a, pr, dn, 0, 16, of, None)),
                      (name, "null audio", lambda fn=fn, of=of: fn(c, None, pr, dn, 0, 16, of, None)),
                      (name, "null print", lambda fn=fn, of=of: fn(c, a, None, dn, 0, 16, of, None)),
                      (name, "null parameters", lambda fn=fn, of=of: fn(c, a, pr, None, 0, 16, of, None)),
                      (name, "bad parameters", lambda fn=fn, of=of: fn(c, a, pr, dn_bad, 0, 16, of, None)),
                      (name, "span before the take", lambda fn=fn, of=of: fn(c, a, pr, dn, -1, 16, of, None)),
                      (name, "span past the take", lambda fn=fn, oh=oh: fn(c, a, pr, dn, n - 8, 16, None, oh)),
                      (name, "null outputs", lambda fn=fn: fn(c, a, pr, dn, 0, 16, None, None)),
                      (name, "bad parameters and bad span", lambda fn=fn, of=of: fn(c, a, pr, dn_bad, -1, 16, of, None))]
            if odd_f:
                calls += [(name, "misaligned f32", lambda fn=fn, odd=odd_f, oh=oh: fn(c, a, pr, dn, 0, 16, odd, oh)),
                          (name, "misaligned int16", lambda fn=fn, of=of, odd=odd_h: fn(c, a, pr, dn, 0, 16, of, odd)),
                          (name, "misaligned, empty range", lambda fn=fn, odd=odd_f: fn(c, a, pr, dn, 0, 0, odd, None)),
                          (name, "bad span and misaligned", lambda fn=fn, odd=odd_f: fn(c, a, pr, dn, -1, 16, odd, None))]
        for name, of, oh, odd_f, odd_h in (("mx_compress", hf, hh, None, None), ("mx_compress_dev", f, h, f_odd, h_odd)):
            fn = getattr(so, name)
            calls += [(name, "null context", lambda fn=fn, of=of: fn(None, a, SR, None, 0, 16, of, None)),
                      (name, "null audio", lambda fn=fn, of=of: fn(c, None, SR, None, 0, 16, of, None)),
                      (name, "bad rate", lambda fn=fn, of=of: fn(c, a, 1, None, 0, 16, of, None)),
                      (name, "bad parameters", lambda fn=fn, of=of: fn(c, a, SR, cp_bad, 0, 16, of, None)),
                      (name, "span before the take", lambda fn=fn, of=of: fn(c, a, SR, None, -1, 16, of, None)),
                      (name, "span past the take", lambda fn=fn, oh=oh: fn(c, a, SR, None, n - 8, 16, None, oh)),
                      (name, "null outputs", lambda fn=fn: fn(c, a, SR, None, 0, 16, None, None)),
                      (name, "bad rate and bad span", lambda fn=fn, of=of: fn(c, a, 1, None, -1, 16, of, None))]
            if odd_f:
                calls += [(name, "misaligned f32", lambda fn=fn, odd=odd_f, oh=oh: fn(c, a, SR, None, 0, 16, odd, oh)),
                          (name, "misaligned int16", lambda fn=fn, of=of, odd=odd_h: fn(c, a, SR, None, 0, 16, of, odd)),
                          (name, "misaligned, empty range", lambda fn=fn, odd=odd_f: fn(c, a, SR, None, 0, 0, odd, None)),
                          (name, "bad span and misaligned", lambda fn=fn, odd=odd_f: fn(c, a, SR, None, -1, 16, odd, None))]
        for name, out, odd in (("mx_compress_gain", hg, None), ("mx_compress_gain_dev", vp(self.gain.ptr), g_odd)):
            fn = getattr(so, name)
            calls += [(name, "null context", lambda fn=fn, out=out: fn(None, a, SR, None, 0, 16, out)),
                      (name, "null audio", lambda fn=fn, out=out: fn(c, None, SR, None, 0, 16, out)),
                      (name, "bad rate", lambda fn=fn, out=out: fn(c, a, 1, None, 0, 16, out)),
                      (name, "bad parameters", lambda fn=fn, out=out: fn(c, a, SR, cp_bad, 0, 16, out)),
                      (name, "span before the take", lambda fn=fn, out=out: fn(c, a, SR, None, -1, 16, out)),
                      (name, "span past the take", lambda fn=fn, out=out: fn(c, a, SR, None, self.steps - 8, 16, out)),
                      (name, "null output", lambda fn=fn: fn(c, a, SR, None, 0, 16, None))]
            if odd:
                calls += [(name, "misaligned", lambda fn=fn, odd=odd: fn(c, a, SR, None, 0, 16, odd)),
                          (name, "misaligned, empty range", lambda fn=fn, odd=odd: fn(c, a, SR, None, 0, 0, odd))]
        for name, out, odd in (("mx_noise_print", P(host_p), None), ("mx_noise_print_dev", vp(self.print.ptr), p_odd)):
            fn = getattr(so, name)
            calls += [(name, "null context", lambda fn=fn, out=out: fn(None, a, 0, 2 * SR, out)),
                      (name, "null audio", lambda fn=fn, out=out: fn(c, None, 0, 2 * SR, out)),
                      (name, "null output", lambda fn=fn: fn(c, a, 0, 2 * SR, None)),
                      (name, "a region without a frame", lambda fn=fn, out=out: fn(c, a, 0, 100, out)),
                      (name, "a region past the take", lambda fn=fn, out=out: fn(c, a, n - 8, n + 8, out))]
            if odd:
                calls += [(name, "misaligned", lambda fn=fn, odd=odd: fn(c, a, 0, 2 * SR, odd))]
        calls += [("mx_noise_rows_dev", "null context", lambda: so.mx_noise_rows_dev(None, a, 0, 4, f)),
                  ("mx_noise_rows_dev", "frames past the take", lambda: so.mx_noise_rows_dev(c, a, mx.denoise_frames(n) - 2, 4, f)),
                  ("mx_noise_rows_dev", "null output", lambda: so.mx_noise_rows_dev(c, a, 0, 4, None)),
                  ("mx_noise_rows_dev", "misaligned", lambda: so.mx_noise_rows_dev(c, a, 0, 4, f_odd)),
                  ("mx_compress_peaks_dev", "null audio", lambda: so.mx_compress_peaks_dev(c, None, SR, 0, 4, f)),
                  ("mx_compress_peaks_dev", "bad rate", lambda: so.mx_compress_peaks_dev(c, a, 1, 0, 4, f)),
                  ("mx_compress_peaks_dev", "steps past the take", lambda: so.mx_compress_peaks_dev(c, a, SR, self.steps - 2, 4, f)),
                  ("mx_compress_peaks_dev", "null output", lambda: so.mx_compress_peaks_dev(c, a, SR, 0, 4, None)),
                  ("mx_compress_peaks_dev", "misaligned", lambda: so.mx_compress_peaks_dev(c, a, SR, 0, 4, f_odd)),
                  ("mx_audio_resample", "null context", lambda: so.mx_audio_resample(None, a, SR, OUT_SR, C.byref(obj))),
                  ("mx_audio_resample", "null output", lambda: so.mx_audio_resample(c, a, SR, OUT_SR, None)),
                  ("mx_audio_resample", "bad rate", lambda: so.mx_audio_resample(c, a, SR, 0, C.byref(obj))),
                  ("mx_audio_denoise", "null audio", lambda: so.mx_audio_denoise(c, None, pr, dn, C.byref(obj))),
                  ("mx_audio_denoise", "null output", lambda: so.mx_audio_denoise(c, a, pr, dn, None)),
                  ("mx_audio_denoise", "null print", lambda: so.mx_audio_denoise(c, a, None, dn, C.byref(obj))),
                  ("mx_audio_denoise", "bad parameters", lambda: so.mx_audio_denoise(c, a, pr, dn_bad, C.byref(obj))),
                  ("mx_audio_compress", "null context", lambda: so.mx_audio_compress(None, a, SR, None, C.byref(obj))),
                  ("mx_audio_compress", "null output", lambda: so.mx_audio_compress(c, a, SR, None, None)),
                  ("mx_audio_compress", "bad rate", lambda: so.mx_audio_compress(c, a, 1, None, C.byref(obj))),
                  ("mx_audio_compress", "bad parameters", lambda: so.mx_audio_compress(c, a, SR, cp_bad, C.byref(obj)))]
        got = [(f"{name}: {what}", int(call()), so.mx_last_error().decode()) for name, what, call in calls]
        assert obj.value is None  # no refused call handed an object out
        return got

    def close(self):
        for buf in (self.resampled, self.clean, self.f32, self.i16, self.gain, self.print):
            buf.free()
        self.so.mx_audio_free(self.ctx, self.audio)
        self.so.mx_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib", nargs="?")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--log")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    assert n >= 2 * SR, "the print is learned on the first two seconds"
    tile = D.vowel_take(1e-2)
    d_img = device_image(np.tile(tile, n // len(tile) + 1)[:n])
    libs = libraries(Lib, args.parent_lib, d_img, n)
    new = libs["new"]
    new.noise_print()
    P0 = new.host["noise_print"].copy()  # the print every denoise call reads
    # every output once per library, compared whole, before anything is timed
    device = ("resample_dev", "denoise_dev", "compress_dev", "compress_gain_dev", "noise_print_dev")
    host = ("resample", "denoise", "compress", "compress_gain", "noise_print")
    objects = {"audio_resample": ("resample", SR, OUT_SR), "audio_denoise": ("denoise", P(P0), C.byref(DN)),
               "audio_compress": ("compress", SR, None)}
    takes_print = ("denoise_dev", "denoise")
    for L in libs.values():
        for name in device + host:
            getattr(L, name)(*((P0,) if name in takes_print else ()))
    kept = ("resampled", "clean", "f32", "i16", "gain", "print")
    for name in kept:  # (one at a time: an hour of float32 is 0.7 GB a library)
        same_bytes(libs, name)
    hosts = [{k: [x.tobytes() for x in (v if isinstance(v, tuple) else (v,))] for k, v in L.host.items()} for L in libs.values()]
    assert all(h == hosts[0] for h in hosts[1:]) and sorted(hosts[0]) == sorted(host)
    assert new.print.read(np.float32).tobytes() == P0.tobytes()  # the two forms of the print agree
    digests = {k: [L.audio_digest(*a) for L in libs.values()] for k, a in objects.items()}
    assert all(d == ds[0] for ds in digests.values() for d in ds[1:]), digests
    refused = [L.refused(P0) for L in libs.values()]
    assert all(r == refused[0] for r in refused[1:]), [x for r in refused[1:] for x, y in zip(r, refused[0]) if x != y]
    allowed = [w for w, rc, _ in refused[0] if rc == 0]
    assert allowed == ["mx_resample_dev: misaligned, empty range"], allowed

    timer = EventTimer(loaded_hip())
    rows = {}

    def after():
        for L in libs.values():
            while L.made:
                L.made.pop().free()

    for name in device + host:
        a = (P0,) if name in takes_print else ()
        rows[name] = timer.timed({k: (lambda L=L: getattr(L, name)(*a)) for k, L in libs.items()}, WARM, RUNS)
    for name, a in objects.items():
        rows[name] = timer.timed({k: (lambda L=L: L.make(*a)) for k, L in libs.items()}, WARM, RUNS, after=after)
    for name in kept:  # ... and the timed launches wrote them again
        same_bytes(libs, name)
    res = {"seconds": args.seconds, "samples": n, "resampled": new.m, "steps": new.steps, "warmups": WARM, "launches": RUNS,
           "ms": rows, "refused_calls": len(refused[0]), "libs": {k: L.version for k, L in libs.items()}, "same_bytes": sorted(libs)}
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
    if args.parent_lib:  # (after the line is out: a run that misses the bound is still on record)
        assert not missed, f"new / parent outside 1 +- 3 x {delta:.4f}: {missed}"


if __name__ == "__main__":
    main()
