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

HOP, WARM, RUNS = 256, 5, 20
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
TRACK_ARGS = [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f]


class Lib:
    """One library's context, its handle on the shared device image and its own output buffers; the table's calls."""

    def __init__(self, path, d_img, n, frames):
        self.so = so = C.CDLL(os.path.abspath(path))
        so.mx_ctx_create.argtypes = [_i, C.POINTER(_vp)]
        so.mx_ctx_set_stream.argtypes = [_vp, _vp]
        so.mx_audio_wrap_device.argtypes = [_vp, _vp, _i64, C.POINTER(_vp)]
        so.mx_f0_track_dev.argtypes = TRACK_ARGS + [_vp]
        so.mx_f0_candidates_dev.argtypes = TRACK_ARGS + [_vp, _vp]
        so.mx_f0_decode_dev.argtypes = [_vp, _vp, _vp, _i64, _vp, _vp, _vp]
        so.mx_f0_decode_set_chunk.argtypes = [_vp, _i64]
        so.mx_version.restype = C.c_char_p
        self.version = so.mx_version().decode()
        self.ctx, self.audio, self.frames = _vp(), _vp(), frames
        assert so.mx_ctx_create(0, C.byref(self.ctx)) == 0
        assert so.mx_ctx_set_stream(self.ctx, None) == 0  # the null stream: the events bracket exactly the launches
        assert so.mx_audio_wrap_device(self.ctx, _vp(d_img.ptr), n, C.byref(self.audio)) == 0
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


def device_image(w):
    """The padded device image of the samples that every library wraps."""
    d_img = DevBuf((len(w) + 2 * mx.MX_AUDIO_PAD) * 4)
    d_img.write(w, offset=mx.MX_AUDIO_PAD * 4)
    return d_img


def same_bytes(libs, *names):
    """Asserts the named output buffers equal, byte for byte, across the libraries; -> the first library's."""
    got = [[getattr(L, k).read(np.uint8).tobytes() for k in names] for L in libs.values()]
    assert all(g == got[0] for g in got[1:]), names
    return got[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunks", default="0,256")
    args = ap.parse_args()
    n = int(args.seconds * SR)
    F = mx.frame_count(n, HOP)
    d_img = device_image(accum_sweep(n))
    libs = {"new": Lib(mx._capi.lib()._name, d_img, n, F)}
    if args.parent_lib:
        libs["parent"] = Lib(args.parent_lib, d_img, n, F)
        libs["parent_again"] = Lib(args.parent_lib, d_img, n, F)
    hip = loaded_hip()
    hip.hipEventCreate.argtypes = [C.POINTER(_vp)]
    hip.hipEventRecord.argtypes = [_vp, _vp]
    hip.hipEventSynchronize.argtypes = [_vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), _vp, _vp]
    e0, e1 = _vp(), _vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def once(call):
        assert hip.hipEventRecord(e0, None) == 0
        call()
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    def timed(call):
        """{library: (median, min, max) ms} of Lib.call, the libraries in turn (interleaved) WARM + RUNS times each."""
        ts = {k: [] for k in libs}
        for it in range(WARM + RUNS):
            for k, L in libs.items():
                t = once(lambda: call(L))
                if it >= WARM:
                    ts[k].append(t)
        return {k: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t))) for k, t in ts.items()}

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
