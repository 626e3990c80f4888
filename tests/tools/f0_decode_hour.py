#!/usr/bin/env python3
"""tests/tools/f0_decode_hour.py [--parent-lib PATH] [--seconds S] — times of the f0 unit over the hour of 48 kHz audio at hop
256 (675 000 frames; the signal of tests/test_gpu_f0.py's hour test): mx_f0_track_dev, mx_f0_candidates_dev and
mx_f0_decode_dev (default chunk and a few set lengths), each the median of 20 launches after 5 warm-ups between HIP events
on the null stream.  --parent-lib: a libmelonix_amd.so built from the parent commit, whose mx_f0_track_dev is timed in the
same process, interleaved with this tree's (the plain instantiation is unchanged code: the two must agree within 1 %).
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the per-kernel table splits the decode."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib")
ap.add_argument("--seconds", type=float, default=3600.0)
ap.add_argument("--chunks", default="0,64,256,1024,4096")
args = ap.parse_args()
HOP, WARM, RUNS = 256, 5, 20

n = int(args.seconds * SR)
w = accum_sweep(n)
ctx = mx.Context(0)
a = ctx.upload(w)
F = mx.frame_count(n, HOP)
hip = loaded_hip()
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
e0, e1 = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
ctx.set_stream(None)  # the null stream: the events bracket exactly the launches


def once(call):
    assert hip.hipEventRecord(e0, None) == 0
    call()
    assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    return ms.value


def timed(*calls):
    """Medians of the calls, run in turn (interleaved) WARM + RUNS times each."""
    ts = [[] for _ in calls]
    for it in range(WARM + RUNS):
        for k, call in enumerate(calls):
            t = once(call)
            if it >= WARM:
                ts[k].append(t)
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


d_track, d_cands, d_out, d_state = DevBuf(F * 16), DevBuf(F * 64), DevBuf(F * 16), DevBuf(F)
res = {"frames": F, "hop": HOP, "sr": SR, "warmups": WARM, "launches": RUNS}
track_here = lambda: ctx.f0_track_dev(a, SR, HOP, 0, F, d_track.ptr)  # noqa: E731
if args.parent_lib:
    par = C.CDLL(os.path.abspath(args.parent_lib))
    par.mx_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    par.mx_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    par.mx_audio_wrap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    par.mx_f0_track_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_float,
                                    C.c_float, C.c_void_p]
    par.mx_version.restype = C.c_char_p
    pctx, paud = C.c_void_p(), C.c_void_p()
    assert par.mx_ctx_create(0, C.byref(pctx)) == 0 and par.mx_ctx_set_stream(pctx, None) == 0
    # the same samples: this tree's padded device image, wrapped
    d_img = DevBuf((n + 2 * mx.MX_AUDIO_PAD) * 4)
    d_img.write(w, offset=mx.MX_AUDIO_PAD * 4)
    assert par.mx_audio_wrap_device(pctx, C.c_void_p(d_img.ptr), n, C.byref(paud)) == 0
    a_here = ctx.wrap_device(d_img.ptr, n)
    d_ptrack = DevBuf(F * 16)

    def track_parent():
        assert par.mx_f0_track_dev(pctx, paud, SR, HOP, 0, F, 55.0, 1760.0, 0.15, C.c_void_p(d_ptrack.ptr)) == 0

    here, parent = timed(lambda: ctx.f0_track_dev(a_here, SR, HOP, 0, F, d_track.ptr), track_parent)
    assert d_track.read(np.uint8).tobytes() == d_ptrack.read(np.uint8).tobytes()
    res["parent"] = par.mx_version().decode()
    res["track_ms"] = dict(zip(("median", "min", "max"), here))
    res["parent_track_ms"] = dict(zip(("median", "min", "max"), parent))
    res["track_vs_parent"] = here[0] / parent[0]
else:
    res["track_ms"] = dict(zip(("median", "min", "max"), timed(track_here)[0]))
(cand,) = timed(lambda: ctx.f0_candidates_dev(a, SR, HOP, 0, F, d_track.ptr, d_cands.ptr))
res["candidates_ms"] = dict(zip(("median", "min", "max"), cand))
res["candidates_vs_track"] = cand[0] / res["track_ms"]["median"]
res["decode_ms"] = {}
states = set()
for c in [int(x) for x in args.chunks.split(",")]:
    ctx.f0_decode_set_chunk(c)
    (t,) = timed(lambda: ctx.f0_decode_dev(d_track.ptr, d_cands.ptr, F, d_out.ptr, d_state.ptr))
    res["decode_ms"]["default" if c == 0 else str(c)] = dict(zip(("median", "min", "max"), t))
    states.add(d_state.read(np.uint8).tobytes())
ctx.f0_decode_set_chunk(0)
assert len(states) == 1  # the path does not depend on the chunk length
st = np.frombuffer(states.pop(), np.uint8)
res["unvoiced_frames"] = int((st == 4).sum())
res["version"] = mx._capi.lib().mx_version().decode()
ctx.use_own_stream()
print(json.dumps(res))
