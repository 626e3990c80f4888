"""tests/hip_timing.py — what the hour tools (tests/tools) and the suite's timed test share: the libraries under test on one device
image of the samples, the two ends of a long output for a comparison, and the timed-launch loop: launches on the null stream
between two HIP events, the candidates in turn (interleaved launch by launch, so that drift of the clocks hits all alike), warm-ups
first, a hook behind every launch for a tool whose launches make objects it has to free."""
import ctypes as C
import os

import numpy as np

import melonix_amd as mx
from conftest import DevBuf

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64


def device_image(w):
    """The padded device image of the samples that every library wraps."""
    d_img = DevBuf((len(w) + 2 * mx.MX_AUDIO_PAD) * 4)
    d_img.write(w, offset=mx.MX_AUDIO_PAD * 4)
    return d_img


class TimedLib:
    """One library: its context on the null stream (the events bracket exactly the launches), its handle on the shared image."""

    def __init__(self, path, d_img, n):
        self.so = so = C.CDLL(os.path.abspath(path))
        so.mx_ctx_create.argtypes = [_i, C.POINTER(_vp)]
        so.mx_ctx_set_stream.argtypes = [_vp, _vp]
        so.mx_audio_wrap_device.argtypes = [_vp, _vp, _i64, C.POINTER(_vp)]
        so.mx_version.restype = C.c_char_p
        self.version = so.mx_version().decode()
        self.ctx, self.audio, self.n = _vp(), _vp(), n
        assert so.mx_ctx_create(0, C.byref(self.ctx)) == 0
        assert so.mx_ctx_set_stream(self.ctx, None) == 0
        assert so.mx_audio_wrap_device(self.ctx, _vp(d_img.ptr), n, C.byref(self.audio)) == 0


def libraries(cls, parent_lib, *args):
    """name -> cls(path, *args): this tree's library ("new") and, with parent_lib, that one twice ("parent", "parent_again")."""
    paths = {"new": mx._capi.lib()._name, **({"parent": parent_lib, "parent_again": parent_lib} if parent_lib else {})}
    return {k: cls(p, *args) for k, p in paths.items()}


def same_bytes(libs, *names):
    """Asserts the named device buffers equal, byte for byte, across the libraries; -> the first library's."""
    got = [[getattr(L, k).read(np.uint8).tobytes() for k in names] for L in libs.values()]
    assert all(g == got[0] for g in got[1:]), names
    return got[0]


EDGE = 1 << 20  # elements compared at either end of an output


def ends(buf, m, dtype=np.float32):
    """The first and the last EDGE elements of the m that a DevBuf holds, as bytes."""
    k = min(EDGE, m)
    return buf.read(dtype, 0, k).tobytes() + buf.read(dtype, np.dtype(dtype).itemsize * (m - k), k).tobytes()


def free_all(made):
    """-> an `after` hook of EventTimer.timed: frees the objects the last launch appended to `made`."""
    def after():
        while made:
            made.pop().free()
    return after


class EventTimer:
    def __init__(self, hip):
        """hip: the process's HIP runtime (conftest.loaded_hip())."""
        self.hip = hip
        hip.hipEventCreate.argtypes = [C.POINTER(_vp)]
        hip.hipEventRecord.argtypes = [_vp, _vp]
        hip.hipEventSynchronize.argtypes = [_vp]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), _vp, _vp]
        self.e0, self.e1 = _vp(), _vp()
        assert hip.hipEventCreate(C.byref(self.e0)) == 0 and hip.hipEventCreate(C.byref(self.e1)) == 0

    def once(self, call):
        """-> the milliseconds between the events around call()."""
        assert self.hip.hipEventRecord(self.e0, None) == 0
        call()
        assert self.hip.hipEventRecord(self.e1, None) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def timed(self, calls, warm, runs, after=None):
        """calls: name -> callable.  -> {name: median / min / max ms of `runs` launches after `warm`}, the calls in turn; after():
        run behind every launch, outside its events."""
        ts = {k: [] for k in calls}
        for it in range(warm + runs):
            for k, call in calls.items():
                t = self.once(call)
                if it >= warm:
                    ts[k].append(t)
                if after:
                    after()
        return {k: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t))) for k, t in ts.items()}
