#!/usr/bin/env python3
"""tests/tools/f0_decode_hour.py [--parent-lib PATH] [--seconds S] [--chunks 0,256] — times of the f0 unit over the hour of
48 kHz audio at hop 256 (675 000 frames; the signal of tests/test_gpu_f0.py's hour test): mx_f0_track_dev,
mx_f0_candidates_dev and mx_f0_decode_dev at each chunk length (0 = the default), each the median of 20 launches after 5
warm-ups between HIP events on the null stream.

Every library goes through the same table of calls, interleaved launch by launch in one process, on the same device image
of the samples: this tree's and, with --parent-lib (a libmelonix_amd.so built from the parent commit), the parent's and the
parent's a second time.  new/parent is the ratio asked about, parent-again/parent the noise floor of the same run; the
bytes of the track, the candidates, the decoded records and the states are asserted equal across the libraries, and the
states across the chunk lengths.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the per-kernel table
splits the decode."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import melonix_amd as mx  # noqa: E402
from conftest import SR, DevBuf, accum_sweep, loaded_hip  # noqa: E402
from hip_timing import EventTimer, TimedLib, device_image, libraries, same_bytes  # noqa: E402

HOP, WARM, RUNS = 256, 5, 20
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
TRACK_ARGS = [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f]


class Lib(TimedLib):
    """One library's context, its handle on the shared device image and its own output buffers; the table's calls."""

    def __init__(self, path, d_img, n, frames):
        super().__init__(path, d_img, n)
        so, self.frames = self.so, frames
        so.mx_f0_track_dev.argtypes = TRACK_ARGS + [_vp]
        so.mx_f0_candidates_dev.argtypes = TRACK_ARGS + [_vp, _vp]
        so.mx_f0_decode_dev.argtypes = [_vp, _vp, _vp, _i64, _vp, _vp, _vp]
        so.mx_f0_decode_set_chunk.argtypes = [_vp, _i64]
        self.track, self.cands, self.out, self.state = (DevBuf(frames * k) for k in (16, 64, 16, 1))

    def range_args(self, first, count):
        return (self.ctx, self.audio, SR, HOP, first, count, 55.0, 1760.0, 0.15)

    def f0_track(self, first=0, count=None):
        count = self.frames - first if count is None else count
        assert self.so.mx_f0_track_dev(*self.range_args(first, count), _vp(self.track.ptr + 16 * first)) == 0

    def f0_candidates(self, first=0, count=None):
        count = self.frames - first if count is None else count
        assert self.so.mx_f0_candidates_dev(*self.range_args(first, count), _vp(self.track.ptr + 16 * first),
                                            _vp(self.cands.ptr + 64 * first)) == 0

    def set_chunk(self, frames):
        assert self.so.mx_f0_decode_set_chunk(self.ctx, frames) == 0

    def f0_decode(self):
        assert self.so.mx_f0_decode_dev(self.ctx, _vp(self.track.ptr), _vp(self.cands.ptr), self.frames, None,
                                        _vp(self.out.ptr), _vp(self.state.ptr)) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunks", default="0,256")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    F = mx.frame_count(n, HOP)
    d_img = device_image(accum_sweep(n))
    libs = libraries(Lib, args.parent_lib, d_img, n, F)
    timer = EventTimer(loaded_hip())

    def timed(call):
        """{library: (median, min, max) ms} of Lib.call, the libraries in turn (interleaved) WARM + RUNS times each."""
        return timer.timed({k: (lambda L=L: call(L)) for k, L in libs.items()}, WARM, RUNS)

    # the table: (row, what to do before it, the call, the buffers whose bytes the libraries must share)
    table = [("track", None, Lib.f0_track, ("track",)), ("candidates", None, Lib.f0_candidates, ("track", "cands"))]
    for c in [int(x) for x in args.chunks.split(",")]:
        table.append(("decode_default" if c == 0 else f"decode_{c}", lambda L, c=c: L.set_chunk(c), Lib.f0_decode, ("out", "state")))
    res = {"frames": F, "hop": HOP, "sr": SR, "warmups": WARM, "launches": RUNS, "libs": {k: L.version for k, L in libs.items()},
           "ms": {}, "new_vs_parent": {}, "parent_vs_parent": {}}
    states = set()
    for row, before, call, outputs in table:
        for L in libs.values():
            if before:
                before(L)
        res["ms"][row] = t = timed(call)
        got = same_bytes(libs, *outputs)
        if "state" in outputs:
            states.add(got[-1])
        if args.parent_lib:
            res["new_vs_parent"][row] = t["new"]["median"] / t["parent"]["median"]
            res["parent_vs_parent"][row] = t["parent_again"]["median"] / t["parent"]["median"]
    assert len(states) == 1  # the path does not depend on the chunk length
    res["same_bytes"] = sorted(libs)
    res["unvoiced_frames"] = int((np.frombuffer(states.pop(), np.uint8) == 4).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
