"""melonix_amd — MI355X-native (gfx950) implementation of the melonix frame-parallel
DSP hot path: exponentially-windowed STFT magnitude spectrogram + pitch pick
(reference spec.cpp / spec-cache.cpp) and the marker-driven granular pitch-shift
resynthesis (reference app.cpp:153-345, 1194-1215) that feeds saveWav.

The product is libmelonix_amd.so (hand-written HIP kernels behind the C-ABI of
include/melonix_amd.h) plus the C++ drop-in facade under melonix_amd/cpp/.
This Python package is only the test/bench harness around that library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import records as _records  # tuples, or an array of the dtype -> a contiguous array of the dtype
from ._capi import (F0_CAND_DTYPE, F0_DTYPE, FORMANT_POINT_DTYPE, MARKER_DTYPE, MX_AUDIO_PAD, NOTE_DTYPE, ONSET_DTYPE, PITCH_DTYPE,  # noqa: F401
                    PSOLA_FGRAIN_DTYPE, PSOLA_GRAIN_DTYPE, STEP_DTYPE, MxError)
from ._capi import COMB_DTYPE, COMB_JOB_DTYPE, TEMPO_WINDOW_DTYPE  # noqa: F401
from ._capi import GAIN_POINT_DTYPE, SIB_FEAT_DTYPE, SIBILANT_DTYPE  # noqa: F401
from ._capi import CHROMA_COLS, CHROMA_JOB_DTYPE, KEY_DTYPE, KEY_WINDOW_DTYPE  # noqa: F401
from ._capi import CONTOUR_NONE, CONTOUR_REC_DTYPE, CONTOUR_SPAN_DTYPE, CONTOUR_STAT_DTYPE  # noqa: F401
from ._capi import LOUD_GROUP_STEPS, LOUD_STEP_DTYPE  # noqa: F401
from ._capi import TP_STEP_DTYPE  # noqa: F401

__all__ = ["Context", "Audio", "MxError", "pitch_band", "frame_count", "grains_host", "schedule_build",
           "save_wav", "column_range", "time2sample", "sample2time", "time2pitchbend", "duration",
           "F0_DTYPE", "F0_CAND_DTYPE", "f0_decode_params_default", "NOTE_DTYPE", "MARKER_DTYPE", "note_params_default", "detect_notes", "correction_markers",
           "PSOLA_GRAIN_DTYPE", "psola_params_default", "psola_plan",
           "PSOLA_FGRAIN_DTYPE", "FORMANT_POINT_DTYPE", "psola_plan_formant",
           "ONSET_DTYPE", "onset_flux_params_default", "onset_pick_params_default", "onset_pick", "timing_params_default",
           "timing_markers", "COMB_JOB_DTYPE", "COMB_DTYPE", "TEMPO_WINDOW_DTYPE", "tempo_params_default",
           "SIB_FEAT_DTYPE", "SIBILANT_DTYPE", "GAIN_POINT_DTYPE", "sib_feature_params_default", "sibilant_params_default", "sibilants",
           "formant_protect", "sibilant_gain_points",
           "CHROMA_COLS", "CHROMA_JOB_DTYPE", "KEY_DTYPE", "KEY_WINDOW_DTYPE", "chroma_params_default", "key_from_chroma",
           "key_from_notes", "correction_markers_tuned",
           "CONTOUR_NONE", "CONTOUR_SPAN_DTYPE", "CONTOUR_REC_DTYPE", "CONTOUR_STAT_DTYPE", "contour_params_default",
           "bend_params_default", "contour_spans", "contour_vibrato", "contour_bend", "psola_plan_bend", "psola_plan_formant_bend",
           "LOUD_STEP_DTYPE", "LOUD_GROUP_STEPS", "level_params_default", "loudness_step_count", "loudness_coeffs", "loudness_curve",
           "loudness_integrated", "note_loudness", "level_gain_points", "normalize_gain",
           "TP_STEP_DTYPE", "true_peak_oversampling", "true_peak_taps", "limit_params_default", "loudness_range", "normalize_gain_tp",
           "resample_plan", "resample_length", "resample_taps",
           "DENOISE_BINS", "denoise_frames", "denoise_factors", "noise_print_rows",
           "COMPRESS_CURVE", "compress_params_default", "compress_plan", "compress_curve", "compress_steps"]


# The two pointer forms of an optional argument.  New wrappers use these: _opt for a host array, _dev for a device address.
def _opt(a):
    """A host array's pointer; NULL when it is None or empty."""
    return None if a is None or not len(a) else C.c_void_p(a.ctypes.data)


def _dev(p):
    """A device address (an integer, e.g. a torch tensor's data_ptr()); NULL when it is None or 0."""
    return C.c_void_p(p or 0)


def _ptr(a):
    """An array's own pointer, even where it is empty; NULL for None only.  Kept where the library's argument checks have
    always seen it (stft ranges, resynth steps, f0_decode, upload, whole-output buffers): not for new code."""
    return None if a is None else C.c_void_p(a.ctypes.data)


_COUNT_CALLS = ("mx_pv_render_length", "mx_pv_arena_budget", "mx_resample_length", "mx_denoise_frames",
                "mx_compress_steps")  # they return a count, or a negative status


def _call(name: str, *args):
    """The entry point `name` with args, its status checked (MxError); the count of the entry points that return one."""
    rc = getattr(_capi.lib(), name)(*args)
    if name in _COUNT_CALLS:
        if rc < 0:
            _capi.check(int(rc))
        return int(rc)
    _capi.check(rc)


def _pcm_pair(n: int, want_f32: bool, want_i16: bool):
    """The host outputs of a call that writes n PCM samples -> (f32 | None, int16 | None)."""
    return np.empty(n, dtype=np.float32) if want_f32 else None, np.empty(n, dtype=np.int16) if want_i16 else None


def _take_records(p, count: int, dtype):
    """A library-allocated array of `count` records as a numpy array of its own; the allocation goes back (mx_free)."""
    out = np.frombuffer(C.string_at(p, count * dtype.itemsize), dtype=dtype).copy()
    _capi.lib().mx_free(p)
    return out


def _handed(dtype, name: str, *args, tail=()):
    """name(*args, &records, &count, *tail), where the library allocates the records -> them as a numpy array of `dtype`."""
    out, cnt = C.c_void_p(), C.c_int64()
    _call(name, *args, C.byref(out), C.byref(cnt), *tail)
    return _take_records(out, cnt.value, dtype)


def _fields(p) -> dict:
    return {k: getattr(p, k) for k, _ in p._fields_}


# the parameter blocks of the build-defined entry points: kind -> (its ctypes struct, the entry point that writes its defaults)
_PARAMS = {"decode": (_capi.F0DecodeParams, "mx_f0_decode_params_default"), "note": (_capi.NoteParams, "mx_note_params_default"),
           "psola": (_capi.PsolaParams, "mx_psola_params_default"), "flux": (_capi.OnsetFluxParams, "mx_onset_flux_params_default"),
           "pick": (_capi.OnsetPickParams, "mx_onset_pick_params_default"), "timing": (_capi.TimingParams, "mx_timing_params_default"),
           "tempo": (_capi.TempoParams, "mx_tempo_params_default"),
           "sib_feature": (_capi.SibFeatureParams, "mx_sib_feature_params_default"),
           "sibilant": (_capi.SibilantParams, "mx_sibilant_params_default"),
           "chroma": (_capi.ChromaParams, "mx_chroma_params_default"), "bend": (_capi.BendParams, "mx_bend_params_default"),
           "level": (_capi.LevelParams, "mx_level_params_default")}
# the same for the kinds whose entry point takes arguments in front of the block and returns a status: compress, the sample rate
_PARAMS_OF = {"compress": (_capi.CompressParams, "mx_compress_params_default")}


def _params_default(kind: str, *args) -> dict:
    struct, fn = _PARAMS_OF[kind] if args else _PARAMS[kind]
    p = struct()
    rc = getattr(_capi.lib(), fn)(*args, C.byref(p))
    if rc:
        _capi.check(rc)
    return _fields(p)


def _params_arg(kind: str, params: dict, never_null: bool = False, args=()):
    """The defaults (of `args`, where the kind's entry point takes any) with `params` over them, each value as its field's type
    (int or float), for the C-ABI; nothing given: NULL, the library's defaults (never_null: the defaults as a struct, for an
    entry point that refuses NULL)."""
    if not params and not never_null:
        return None
    struct = (_PARAMS_OF if args else _PARAMS)[kind][0]
    unknown = set(params) - {k for k, _ in struct._fields_}
    if unknown:
        raise TypeError(f"unknown {kind} parameters {sorted(unknown)}")
    d = {**_params_default(kind, *args), **params}
    return C.byref(struct(**{k: (float if t in (C.c_float, C.c_double) else int)(d[k]) for k, t in struct._fields_}))


def _default_fn(kind: str):
    def fn() -> dict:
        return _params_default(kind)
    fn.__name__ = fn.__qualname__ = _PARAMS[kind][1][3:]  # the entry point's name without "mx_"
    fn.__doc__ = f"The {kind} parameters as {_PARAMS[kind][1]} writes them."
    return fn


# one per kind of _PARAMS, each under its entry point's name (the check: not under a neighbour's, whatever _PARAMS' order becomes)
_DEFAULT_FNS = tuple(map(_default_fn, _PARAMS))
(f0_decode_params_default, note_params_default, psola_params_default, onset_flux_params_default, onset_pick_params_default,
 timing_params_default, tempo_params_default, sib_feature_params_default, sibilant_params_default, chroma_params_default,
 bend_params_default, level_params_default) = _DEFAULT_FNS
assert all(globals()[fn.__name__] is fn for fn in _DEFAULT_FNS)


def contour_params_default(sr: int, hop: int) -> dict:
    """The split's parameters at sr / hop frames per second: a 250 ms window, lags of 3 .. 12 Hz."""
    p = _capi.ContourParams()
    _call("mx_contour_params_default", sr, hop, C.byref(p))
    return _fields(p)


def _contour_params(params: dict):
    """half_width, lag_min, lag_max -> the struct (the split's entry points take no NULL)."""
    return C.byref(_capi.ContourParams(int(params["half_width"]), int(params["lag_min"]), int(params["lag_max"])))


def pitch_band(N: int, sr: int = 48000):
    a, b = C.c_int(), C.c_int()
    _capi.lib().mx_pitch_band(N, sr, C.byref(a), C.byref(b))
    return a.value, b.value


def bin_note(bin: int, N: int, sr: int = 48000) -> float:
    """Marker::note of a pitch record's bin (app.cpp:498-499 note law)."""
    return _capi.lib().mx_bin_note(int(bin), N, sr)


def note_bin(note: float, N: int, sr: int = 48000) -> float:
    return _capi.lib().mx_note_bin(float(note), N, sr)


def pv_plan(n: int, sr: int, markers):
    """Frame plan of the marker-driven phase vocoder -> (n_out, apos int64[F], tf f64[F], rf f64[F], i0 int64[F+1])."""
    m = _capi.markers_array(markers)
    pa, pt, pr, pi = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    F, cnt = C.c_int64(), C.c_int64()
    _call("mx_pv_plan", n, sr, m, len(markers), C.byref(pa), C.byref(pt), C.byref(pr), C.byref(pi), C.byref(F), C.byref(cnt))
    f = F.value
    out = (cnt.value,
           np.frombuffer(C.string_at(pa, f * 8), dtype=np.int64).copy(),
           np.frombuffer(C.string_at(pt, f * 8), dtype=np.float64).copy(),
           np.frombuffer(C.string_at(pr, f * 8), dtype=np.float64).copy(),
           np.frombuffer(C.string_at(pi, (f + 1) * 8), dtype=np.int64).copy())
    for q in (pa, pt, pr, pi):
        _capi.lib().mx_free(q)
    return out


def pv_shard_frames(n: int, semitones: float, rank: int, world: int):
    """-> (frame_lo, frame_hi, out_lo, out_hi) of one rank of a multi-GPU phase-vocoder run."""
    v = [C.c_int64() for _ in range(4)]
    _call("mx_pv_shard_frames", n, float(semitones), rank, world, *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def frame_count(n: int, hop: int) -> int:
    return _capi.lib().mx_frame_count(n, hop)


# the f0 wrappers' default band (Hz) and threshold
_F0_FMIN, _F0_FMAX, _F0_THRESHOLD = 55.0, 1760.0, 0.15


class Audio:
    def __init__(self, ctx: "Context", handle, n: int, keepalive=None):
        self.ctx, self.handle, self.n, self._keep = ctx, handle, n, keepalive

    def free(self):
        if self.handle:
            _capi.lib().mx_audio_free(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KeptRows:
    """Magnitude rows of one batch that stay on the device (mx_rows): fetch() / colormap() bring spans of them back
    without another transform."""

    def __init__(self, ctx, handle, N):
        self.ctx, self.handle, self.N = ctx, handle, N

    def __len__(self):
        return int(_capi.lib().mx_rows_count(self.handle)) if self.handle else 0

    def fetch(self, first: int, count: int):
        out = np.empty((count, self.N // 2), dtype=np.float32)
        _call("mx_rows_fetch", self.ctx.handle, self.handle, first, count, _ptr(out))
        return out

    def colormap(self, first: int, count: int, k: float):
        out = np.empty((count, self.N // 2, 3), dtype=np.uint8)
        _call("mx_rows_colormap", self.ctx.handle, self.handle, first, count, float(k), _ptr(out))
        return out

    def free(self):
        if self.handle:
            _capi.lib().mx_rows_free(self.ctx.handle, self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):  # the rows are a device allocation: do not leave them to the end of the process
        try:
            if self.ctx.handle:
                self.free()
        except Exception:
            pass


class Context:
    """One per GPU / rank (mx_ctx)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _call("mx_ctx_create", device, C.byref(h))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            _capi.lib().mx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int | None):
        """Launch on this hipStream_t (0/None = the HIP null stream, torch's default stream)."""
        _call("mx_ctx_set_stream", self.handle, _dev(hip_stream))

    def use_own_stream(self):
        _call("mx_ctx_use_own_stream", self.handle)

    def release_scratch(self):
        """Give back the work buffers the context keeps between calls (staging, phase-vocoder arena)."""
        _call("mx_ctx_release_scratch", self.handle)

    def set_frames_per_block(self, g: int):
        _call("mx_ctx_set_frames_per_block", self.handle, g)

    def synchronize(self):
        _call("mx_ctx_synchronize", self.handle)

    # ---- audio ----
    def _audio(self, n: int, name: str, *args, keepalive=None, tail=()) -> Audio:
        """name(ctx, *args, &handle, *tail) -> the new Audio of n samples."""
        h = C.c_void_p()
        _call(name, self.handle, *args, C.byref(h), *tail)
        return Audio(self, h, n, keepalive)

    def upload(self, wav) -> Audio:
        wav = np.ascontiguousarray(wav, dtype=np.float32)
        return self._audio(len(wav), "mx_audio_upload", _ptr(wav), len(wav))

    def wrap_device(self, d_padded_ptr: int, n: int, keepalive=None) -> Audio:
        return self._audio(n, "mx_audio_wrap_device", C.c_void_p(d_padded_ptr), n, keepalive=keepalive)

    # ---- the host form of a per-frame track ----
    def _frame_tracks(self, name: str, audio: Audio, x: int, hop: int, first: int, count: int | None, mid, *outs):
        """name(ctx, audio, x, hop, first, count, *mid, *outputs) -> the tuple of outputs.  count None: the frames from `first`
        to the end of the file; each of `outs` is (dtype, *trailing shape) of one output of max(count, 0) records, or None
        for one not wanted (NULL)."""
        count = frame_count(audio.n, hop) - first if count is None else count
        arrays = tuple(None if o is None else np.empty((max(count, 0), *o[1:]), dtype=o[0]) for o in outs)
        _call(name, self.handle, audio.handle, x, hop, first, count, *mid, *map(_ptr, arrays))
        return arrays

    # ---- STFT, host outputs ----
    def stft_hop(self, audio: Audio, N: int, hop: int, first: int = 0, count: int | None = None, band=(-1, -1),
                 want_mags: bool = True, want_pitch: bool = True):
        return self._frame_tracks("mx_stft_hop", audio, N, hop, first, count, (band[0], band[1]),
                                  (np.float32, N // 2) if want_mags else None, (PITCH_DTYPE,) if want_pitch else None)

    def stft_ranges(self, audio: Audio, N: int, ranges, band=(-1, -1), want_mags: bool = True,
                    want_pitch: bool = True):
        ranges = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        count = len(ranges)
        mags = np.empty((count, N // 2), dtype=np.float32) if want_mags else None
        pitch = np.empty(count, dtype=PITCH_DTYPE) if want_pitch else None
        _call("mx_stft_ranges", self.handle, audio.handle, N, _ptr(ranges), count, band[0], band[1], _ptr(mags), _ptr(pitch))
        return mags, pitch

    def stft_ranges_rgb(self, audio: Audio, N: int, ranges, k: float, want_mags: bool = False):
        """Texture rows (count x N/2 x 3 uint8): the spec-cache.cpp:77-96 colormap applied in the STFT
        kernel's epilogue (one launch).  want_mags: also return the magnitude rows of that launch."""
        ranges = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        rgb = np.empty((len(ranges), N // 2, 3), dtype=np.uint8)
        if not want_mags:
            _call("mx_stft_ranges_rgb", self.handle, audio.handle, N, _ptr(ranges), len(ranges), float(k), _ptr(rgb))
            return rgb
        mags = np.empty((len(ranges), N // 2), dtype=np.float32)
        _call("mx_stft_ranges_rgb_mags", self.handle, audio.handle, N, _ptr(ranges), len(ranges), float(k), _ptr(mags), _ptr(rgb))
        return rgb, mags

    def stft_ranges_keep(self, audio: Audio, N: int, ranges, k: float = 0.0, want_mags: bool = False):
        """mx_stft_ranges_keep: the batch's magnitude rows stay in HBM (returns a KeptRows handle), texel rows
        (k != 0) and / or the magnitude rows come back as well: (rows, rgb | None, mags | None)."""
        ranges = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        rgb = np.empty((len(ranges), N // 2, 3), dtype=np.uint8) if k != 0.0 else None
        mags = np.empty((len(ranges), N // 2), dtype=np.float32) if want_mags else None
        h = C.c_void_p()
        _call("mx_stft_ranges_keep", self.handle, audio.handle, N, _ptr(ranges), len(ranges), float(k), _ptr(mags), _ptr(rgb),
              C.byref(h))
        return KeptRows(self, h, N), rgb, mags

    # ---- STFT, device-resident outputs (raw device pointers, async on the ctx stream) ----
    def stft_hop_dev(self, audio: Audio, N: int, hop: int, first: int, count: int, d_mags: int | None,
                     d_pitch: int | None, band=(-1, -1)):
        _call("mx_stft_hop_dev", self.handle, audio.handle, N, hop, first, count, band[0], band[1], _dev(d_mags), _dev(d_pitch))

    def stft_ranges_dev(self, audio: Audio, N: int, d_ranges: int, count: int, d_mags: int | None,
                        d_pitch: int | None, band=(-1, -1)):
        _call("mx_stft_ranges_dev", self.handle, audio.handle, N, C.c_void_p(d_ranges), count, band[0], band[1], _dev(d_mags),
              _dev(d_pitch))

    # ---- YIN f0 tracking (build-defined; include/melonix_amd.h) ----
    def f0_track(self, audio: Audio, sr: int, hop: int = 256, first: int = 0, count: int | None = None, fmin: float = _F0_FMIN,
                 fmax: float = _F0_FMAX, threshold: float = _F0_THRESHOLD):
        """-> F0_DTYPE records of frames [first, first + count) (frame h centred on sample h*hop)."""
        return self._frame_tracks("mx_f0_track", audio, sr, hop, first, count, (fmin, fmax, threshold), (F0_DTYPE,))[0]

    def f0_track_dev(self, audio: Audio, sr: int, hop: int, first: int, count: int, d_out: int, fmin: float = _F0_FMIN,
                     fmax: float = _F0_FMAX, threshold: float = _F0_THRESHOLD):
        """The records stay in HBM at d_out (count x 16 bytes); asynchronous on the context's stream."""
        _call("mx_f0_track_dev", self.handle, audio.handle, sr, hop, first, count, fmin, fmax, threshold, _dev(d_out))

    # ---- candidate ladder and Viterbi decode (build-defined) ----
    def f0_candidates(self, audio: Audio, sr: int, hop: int = 256, first: int = 0, count: int | None = None,
                      fmin: float = _F0_FMIN, fmax: float = _F0_FMAX, threshold: float = _F0_THRESHOLD):
        """-> (track: F0_DTYPE records, exactly f0_track's; cands: count x 4 F0_CAND_DTYPE, the frames' candidate ladders)."""
        return self._frame_tracks("mx_f0_candidates", audio, sr, hop, first, count, (fmin, fmax, threshold),
                                  (F0_DTYPE,), (F0_CAND_DTYPE, _capi.F0_CANDS))

    def f0_candidates_dev(self, audio: Audio, sr: int, hop: int, first: int, count: int, d_track: int | None, d_cands: int,
                          fmin: float = _F0_FMIN, fmax: float = _F0_FMAX, threshold: float = _F0_THRESHOLD):
        """The ladders stay in HBM at d_cands (count x 64 bytes), the plain records at d_track (count x 16 bytes; None: not
        wanted); asynchronous on the context's stream."""
        _call("mx_f0_candidates_dev", self.handle, audio.handle, sr, hop, first, count, fmin, fmax, threshold, _dev(d_track),
              _dev(d_cands))

    def f0_decode(self, track, cands, **params):
        """The cheapest path through the frames' candidates and the unvoiced state -> (decoded F0_DTYPE track, uint8 state
        per frame: the slot taken, 4 = unvoiced).  params: fields of f0_decode_params_default()."""
        track = np.ascontiguousarray(track, dtype=F0_DTYPE)
        cands = np.ascontiguousarray(cands, dtype=F0_CAND_DTYPE).reshape(-1, _capi.F0_CANDS)
        if len(cands) != len(track):
            raise ValueError("one row of candidates per frame of the track")
        out = np.empty(len(track), dtype=F0_DTYPE)
        state = np.empty(len(track), dtype=np.uint8)
        _call("mx_f0_decode", self.handle, _ptr(track), _ptr(cands), len(track), _params_arg("decode", params), _ptr(out), _ptr(state))
        return out, state

    def f0_decode_dev(self, d_track: int, d_cands: int, count: int, d_out: int, d_state: int | None = None, **params):
        """Device pointers (d_out may be d_track; d_state None: not wanted); asynchronous on the context's stream."""
        _call("mx_f0_decode_dev", self.handle, _dev(d_track), _dev(d_cands), count, _params_arg("decode", params), _dev(d_out),
              _dev(d_state))

    def f0_track_decoded(self, audio: Audio, sr: int, hop: int = 256, first: int = 0, count: int | None = None,
                         fmin: float = _F0_FMIN, fmax: float = _F0_FMAX, threshold: float = _F0_THRESHOLD, **params):
        """Candidates and decode in one call -> the decoded F0_DTYPE track (tau 0: silent or unvoiced)."""
        return self._frame_tracks("mx_f0_track_decoded", audio, sr, hop, first, count,
                                  (fmin, fmax, threshold, _params_arg("decode", params)), (F0_DTYPE,))[0]

    def f0_decode_set_chunk(self, frames: int):
        """Frames per chunk of the decode's scans (0 = the default); for tests: the output does not depend on it."""
        _call("mx_f0_decode_set_chunk", self.handle, int(frames))

    # ---- onset strength and onsets (build-defined; include/melonix_amd.h) ----
    def onset_flux(self, audio: Audio, sr: int, hop: int = 256, first: int = 0, count: int | None = None, **params):
        """-> float32 onset strength of frames [first, first + count) (frame h centred on sample h*hop).  params: fields of
        onset_flux_params_default()."""
        return self._frame_tracks("mx_onset_flux", audio, sr, hop, first, count, (_params_arg("flux", params),), (np.float32,))[0]

    def onset_flux_dev(self, audio: Audio, sr: int, hop: int, first: int, count: int, d_flux: int, **params):
        """The values stay in HBM at d_flux (count x 4 bytes); asynchronous on the context's stream."""
        _call("mx_onset_flux_dev", self.handle, audio.handle, sr, hop, first, count, _params_arg("flux", params), _dev(d_flux))

    def onsets_detect(self, audio: Audio, sr: int, hop: int = 256, flux_params: dict | None = None, pick_params: dict | None = None):
        """Flux over the whole file and the picks from it -> ONSET_DTYPE array."""
        return _handed(ONSET_DTYPE, "mx_onsets_detect", self.handle, audio.handle, sr, hop, _params_arg("flux", flux_params or {}),
                       _params_arg("pick", pick_params or {}))

    # ---- sibilant features, segments, protection and balance (build-defined; include/melonix_amd.h) ----
    sib_feature_params_default = staticmethod(sib_feature_params_default)
    sibilant_params_default = staticmethod(sibilant_params_default)

    def sib_features(self, audio: Audio, sr: int, hop: int = 256, first: int = 0, count: int | None = None, **params):
        """-> SIB_FEAT_DTYPE records of frames [first, first + count) (frame h centred on sample h*hop).  params: fields of
        sib_feature_params_default()."""
        return self._frame_tracks("mx_sib_features", audio, sr, hop, first, count, (_params_arg("sib_feature", params),),
                                  (SIB_FEAT_DTYPE,))[0]

    def sib_features_dev(self, audio: Audio, sr: int, hop: int, first: int, count: int, d_feat: int, **params):
        """The records stay in HBM at d_feat (count x 16 bytes); asynchronous on the context's stream."""
        _call("mx_sib_features_dev", self.handle, audio.handle, sr, hop, first, count, _params_arg("sib_feature", params),
              _dev(d_feat))

    def sibilants_detect(self, audio: Audio, sr: int, hop: int = 256, feature_params: dict | None = None, **params):
        """Features over the whole file and the segments from them -> SIBILANT_DTYPE array.  params: fields of
        sibilant_params_default()."""
        return _handed(SIBILANT_DTYPE, "mx_sibilants_detect", self.handle, audio.handle, sr, hop,
                       _params_arg("sib_feature", feature_params or {}), _params_arg("sibilant", params))

    def sibilants(self, feat, hop: int = 256, first: int = 0, **params):
        return sibilants(feat, hop, first, **params)

    # ---- chroma records, their window sums, key / scale / tuning (build-defined; include/melonix_amd.h) ----
    chroma_params_default = staticmethod(chroma_params_default)

    def chroma(self, audio: Audio, sr: int, hop: int = 2048, first: int = 0, count: int | None = None, **params):
        """-> (count, 40) float32: the chroma records of frames [first, first + count) (frame h centred on sample h*hop).
        params: fields of chroma_params_default()."""
        return self._frame_tracks("mx_chroma", audio, sr, hop, first, count, (_params_arg("chroma", params),),
                                  (np.float32, CHROMA_COLS))[0]

    def chroma_dev(self, audio: Audio, sr: int, hop: int, first: int, count: int, d_out: int, **params):
        """The records stay in HBM at d_out (count x 160 bytes); asynchronous on the context's stream."""
        _call("mx_chroma_dev", self.handle, audio.handle, sr, hop, first, count, _params_arg("chroma", params), _dev(d_out))

    def chroma_sum(self, chroma, jobs):
        """Column sums of (count, 40) float32 records over `jobs` ((first_frame, frames) pairs) -> (njobs, 40) float64."""
        rec = np.ascontiguousarray(chroma, dtype=np.float32).reshape(-1, CHROMA_COLS)
        jobs = _records(jobs, CHROMA_JOB_DTYPE)
        out = np.empty((len(jobs), CHROMA_COLS), dtype=np.float64)
        _call("mx_chroma_sum", self.handle, _opt(rec), len(rec), _opt(jobs), len(jobs), _opt(out))
        return out

    def chroma_sum_dev(self, d_chroma: int, count: int, d_jobs: int, njobs: int, d_out: int):
        """The same with records, jobs and sums (njobs x 320 bytes) in HBM; asynchronous on the context's stream."""
        _call("mx_chroma_sum_dev", self.handle, _dev(d_chroma), count, _dev(d_jobs), njobs, _dev(d_out))

    def key_detect(self, audio: Audio, sr: int, hop: int = 2048, window_frames: int = 0, window_hop: int = 1, **params):
        """Key, scale and tuning of the whole file -> (dict of KEY_DTYPE's fields, KEY_WINDOW_DTYPE array: one key per window
        of window_frames frames every window_hop; none where window_frames is 0).  params: fields of chroma_params_default()."""
        key = _capi.Key()
        windows = _handed(KEY_WINDOW_DTYPE, "mx_key_detect", self.handle, audio.handle, sr, hop, _params_arg("chroma", params),
                          int(window_frames), int(window_hop), C.byref(key))
        return _key_dict(key), windows

    # ---- pitch drift and vibrato inside notes (build-defined; include/melonix_amd.h) ----
    def contour_cents(self, track, sr: int, threshold: float = 0.15, rms_floor: float = 1e-3):
        """-> int32[count]: the cents (1/16 cent, 1600 x the note) of F0_DTYPE records, CONTOUR_NONE where unvoiced."""
        track = np.ascontiguousarray(track, dtype=F0_DTYPE)
        out = np.empty(len(track), dtype=np.int32)
        _call("mx_contour_cents", self.handle, _opt(track), len(track), sr, threshold, rms_floor, _opt(out))
        return out

    def contour_cents_dev(self, d_track: int, count: int, sr: int, threshold: float, rms_floor: float, d_cents: int):
        """count records at d_track -> count int32 at d_cents, both in HBM; asynchronous on the context's stream."""
        _call("mx_contour_cents_dev", self.handle, _dev(d_track), count, sr, threshold, rms_floor, _dev(d_cents))

    def contour_split(self, cents, spans, want_rec: bool = True, want_stat: bool = True, **params):
        """int32 cents and (first, frames) spans -> (CONTOUR_REC_DTYPE[count] | None, CONTOUR_STAT_DTYPE[nspans] | None).
        params: half_width, lag_min, lag_max, all three (contour_params_default(sr, hop))."""
        cents = np.ascontiguousarray(cents, dtype=np.int32)
        spans = _records(spans, CONTOUR_SPAN_DTYPE)
        rec = np.empty(len(cents), dtype=CONTOUR_REC_DTYPE) if want_rec else None
        stat = np.empty(len(spans), dtype=CONTOUR_STAT_DTYPE) if want_stat else None
        _call("mx_contour_split", self.handle, _opt(cents), len(cents), _opt(spans), len(spans), _contour_params(params), _ptr(rec),
              _ptr(stat))
        return rec, stat

    def contour_split_dev(self, d_cents: int, count: int, d_spans: int, nspans: int, d_rec: int | None, d_stat: int | None,
                          **params):
        """Everything in HBM; asynchronous on the context's stream.  The spans are NOT checked (include/melonix_amd.h)."""
        _call("mx_contour_split_dev", self.handle, _dev(d_cents), count, _dev(d_spans), nspans, _contour_params(params), _dev(d_rec),
              _dev(d_stat))

    def pitch_contour(self, track, sr: int, hop: int, notes, first: int = 0, threshold: float = 0.15, rms_floor: float = 1e-3,
                      **params):
        """Cents and split of a host track over detect_notes' notes -> (CONTOUR_REC_DTYPE[count], CONTOUR_STAT_DTYPE[nnotes]).
        params: none (contour_params_default(sr, hop)) or all of half_width, lag_min, lag_max."""
        track = np.ascontiguousarray(track, dtype=F0_DTYPE)
        notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
        rec = np.empty(len(track), dtype=CONTOUR_REC_DTYPE)
        stat = np.empty(len(notes), dtype=CONTOUR_STAT_DTYPE)
        _call("mx_pitch_contour", self.handle, _opt(track), len(track), sr, hop, first, _opt(notes), len(notes), threshold, rms_floor,
              _contour_params(params) if params else None, _ptr(rec), _ptr(stat))
        return rec, stat

    def formant_protect(self, points, sibs, ramp: int, n: int):
        return formant_protect(points, sibs, ramp, n)

    def sibilant_gain_points(self, sibs, db: float, ramp: int, n: int):
        return sibilant_gain_points(sibs, db, ramp, n)

    def audio_gain(self, audio: Audio, points) -> Audio:
        """A new Audio: `audio` through the piecewise-linear gain of `points` ((sample, amp) pairs or a GAIN_POINT_DTYPE array;
        none: a copy).  Blocks."""
        pts = _records(points, GAIN_POINT_DTYPE)
        return self._audio(audio.n, "mx_audio_gain", audio.handle, _opt(pts), len(pts))

    def audio_gain_dev(self, audio: Audio, d_points: int, npts: int) -> Audio:
        """The same with the points in HBM (not validated there); asynchronous on the context's stream."""
        return self._audio(audio.n, "mx_audio_gain_dev", audio.handle, _dev(d_points), npts)

    def audio_download(self, audio: Audio, first: int = 0, count: int | None = None):
        """Samples [first, first + count) of an Audio (count None: to the end of the file; the pads are readable) -> float32."""
        count = audio.n - first if count is None else count
        out = np.empty(max(count, 0), dtype=np.float32)
        _call("mx_audio_download", self.handle, audio.handle, first, count, _ptr(out))
        return out

    # ---- loudness records, BS.1770 loudness, note levelling (build-defined; include/melonix_amd.h) ----
    level_params_default = staticmethod(level_params_default)

    def loudness_steps(self, audio: Audio, sr: int, first_group: int = 0, ngroups: int | None = None):
        """-> LOUD_STEP_DTYPE records of the steps of groups [first_group, first_group + ngroups) (ten 10 ms steps a group;
        ngroups None: to the end of the file)."""
        steps = loudness_step_count(audio.n, sr)
        ngroups = -(-steps // LOUD_GROUP_STEPS) - first_group if ngroups is None else ngroups
        count = min(LOUD_GROUP_STEPS * (first_group + ngroups), steps) - LOUD_GROUP_STEPS * first_group if ngroups > 0 else 0
        out = np.empty(max(count, 0), dtype=LOUD_STEP_DTYPE)
        _call("mx_loudness_steps", self.handle, audio.handle, sr, first_group, ngroups, _ptr(out))
        return out

    def loudness_steps_dev(self, audio: Audio, sr: int, first_group: int, ngroups: int, d_steps: int):
        """The records stay in HBM at d_steps (16 bytes a step, 16-byte aligned); asynchronous on the context's stream."""
        _call("mx_loudness_steps_dev", self.handle, audio.handle, sr, first_group, ngroups, _dev(d_steps))

    def loudness_measure(self, audio: Audio, sr: int) -> dict:
        """The whole take -> dict of mx_loudness' fields (integrated, momentary_max, shortterm_max, peak, the gate counts)."""
        m = _capi.Loudness()
        _call("mx_loudness_measure", self.handle, audio.handle, sr, C.byref(m))
        return _fields(m)

    def loudness_coeffs(self, sr: int):
        return loudness_coeffs(sr)

    def loudness_curve(self, steps, sr: int, window_steps: int = 40):
        return loudness_curve(steps, sr, window_steps)

    def loudness_integrated(self, steps, sr: int) -> dict:
        return loudness_integrated(steps, sr)

    def note_loudness(self, steps, sr: int, notes):
        return note_loudness(steps, sr, notes)

    def level_gain_points(self, notes, lufs, **params):
        return level_gain_points(notes, lufs, **params)

    def normalize_gain(self, measured: dict, target_lufs: float = -23.0, ceiling_db: float = -1.0) -> float:
        return normalize_gain(measured, target_lufs, ceiling_db)

    # ---- true peak, look-ahead limiter, loudness range (build-defined; include/melonix_amd.h) ----
    def true_peak_steps(self, audio: Audio, sr: int, first_step: int = 0, nsteps: int | None = None):
        """-> TP_STEP_DTYPE records (true peak, sample peak) of the 10 ms steps [first_step, first_step + nsteps) (nsteps None:
        to the end of the file)."""
        nsteps = loudness_step_count(audio.n, sr) - first_step if nsteps is None else nsteps
        out = np.empty(max(nsteps, 0), dtype=TP_STEP_DTYPE)
        _call("mx_true_peak_steps", self.handle, audio.handle, sr, first_step, nsteps, _ptr(out))
        return out

    def true_peak_steps_dev(self, audio: Audio, sr: int, first_step: int, nsteps: int, d_steps: int):
        """The records stay in HBM at d_steps (8 bytes a step, 8-byte aligned); asynchronous on the context's stream."""
        _call("mx_true_peak_steps_dev", self.handle, audio.handle, sr, first_step, nsteps, _dev(d_steps))

    def true_peak(self, audio: Audio, sr: int):
        """The whole take -> (true peak, sample peak), amplitudes as float32 values."""
        t, s = C.c_float(), C.c_float()
        _call("mx_true_peak_measure", self.handle, audio.handle, sr, C.byref(t), C.byref(s))
        return np.float32(t.value), np.float32(s.value)

    @staticmethod
    def _limit_params(sr: int, ceiling_db: float, lookahead, ceiling_amp):
        amp = np.float32(10.0 ** (ceiling_db / 20.0)) if ceiling_amp is None else np.float32(ceiling_amp)
        d = limit_params_default(sr)  # (raises for a sample rate out of range)
        return C.byref(_capi.LimitParams(float(amp), int(d["lookahead"] if lookahead is None else lookahead)))

    def limit(self, audio: Audio, sr: int, ceiling_db: float = -1.0, lookahead: int | None = None, pcm16: bool = False,
              ceiling_amp=None):
        """A new Audio: `audio` through the look-ahead limiter under a ceiling of ceiling_db dBTP (ceiling_amp: the amplitude
        itself, as a float32) with a look-ahead of `lookahead` samples (None: the default, 5 ms).  pcm16: -> (Audio, the int16
        samples).  Blocks."""
        out = np.empty(audio.n, dtype=np.int16) if pcm16 else None
        b = self._audio(audio.n, "mx_audio_limit", audio.handle, sr, self._limit_params(sr, ceiling_db, lookahead, ceiling_amp),
                        tail=(_ptr(out),))
        return (b, out) if pcm16 else b

    def limit_dev(self, audio: Audio, sr: int, ceiling_db: float = -1.0, lookahead: int | None = None, d_pcm16: int | None = None,
                  ceiling_amp=None) -> Audio:
        """The same with the int16 samples (d_pcm16 None: none) in HBM; asynchronous on the context's stream."""
        return self._audio(audio.n, "mx_audio_limit_dev", audio.handle, sr, self._limit_params(sr, ceiling_db, lookahead, ceiling_amp),
                           tail=(_dev(d_pcm16),))

    def loudness_range(self, steps, sr: int) -> dict:
        return loudness_range(steps, sr)

    def normalize_gain_tp(self, measured: dict, true_peak: float, target_lufs: float = -23.0, ceiling_dbtp: float = -1.0) -> float:
        return normalize_gain_tp(measured, true_peak, target_lufs, ceiling_dbtp)

    # ---- sample-rate conversion (build-defined; include/melonix_amd.h) ----
    def resample(self, audio: Audio, in_rate: int, out_rate: int) -> Audio:
        """A new Audio: `audio` converted from in_rate to out_rate, resample_length(audio.n, ...) samples (equal rates: a copy).
        Asynchronous on the context's stream."""
        return self._audio(resample_length(audio.n, in_rate, out_rate), "mx_audio_resample", audio.handle, in_rate, out_rate)

    def resample_dev(self, audio: Audio, in_rate: int, out_rate: int, first_out: int, count: int, d_out: int):
        """Outputs [first_out, first_out + count) of the converted take stay in HBM at d_out (4-byte aligned); asynchronous on the
        context's stream."""
        _call("mx_resample_dev", self.handle, audio.handle, in_rate, out_rate, first_out, count, _dev(d_out))

    def resample_range(self, audio: Audio, in_rate: int, out_rate: int, first_out: int = 0, count: int | None = None):
        """-> float32 outputs [first_out, first_out + count) of the converted take (count None: to its end).  Blocks."""
        count = resample_length(audio.n, in_rate, out_rate) - first_out if count is None else count
        out = np.empty(max(count, 0), dtype=np.float32)
        _call("mx_resample", self.handle, audio.handle, in_rate, out_rate, first_out, count, _ptr(out))
        return out

    # ---- noise reduction from a noise print (build-defined; include/melonix_amd.h) ----
    def noise_rows_dev(self, audio: Audio, first_frame: int, count: int, d_rows: int):
        """The power rows of frames [first_frame, first_frame + count) stay in HBM at d_rows (513 floats a frame); asynchronous
        on the context's stream."""
        _call("mx_noise_rows_dev", self.handle, audio.handle, first_frame, count, _dev(d_rows))

    def noise_print(self, audio: Audio, begin: int, end: int):
        """-> the noise print (513 float32) learned from samples [begin, end) of `audio`.  Blocks."""
        out = np.empty(DENOISE_BINS, dtype=np.float32)
        _call("mx_noise_print", self.handle, audio.handle, begin, end, _ptr(out))
        return out

    def noise_print_dev(self, audio: Audio, begin: int, end: int, d_print: int):
        """The same print stays in HBM at d_print; asynchronous on the context's stream."""
        _call("mx_noise_print_dev", self.handle, audio.handle, begin, end, _dev(d_print))

    def denoise(self, audio: Audio, noise_print, reduction_db: float = 12.0, sensitivity_db: float = 6.0) -> Audio:
        """A new Audio: `audio` cleaned with `noise_print` (513 float32, host).  Asynchronous on the context's stream."""
        pr = _noise_print_arg(noise_print)
        return self._audio(audio.n, "mx_audio_denoise", audio.handle, _ptr(pr), _denoise_params(reduction_db, sensitivity_db))

    def denoise_dev(self, audio: Audio, noise_print, reduction_db: float, sensitivity_db: float, first: int, count: int,
                    d_f32: int | None = None, d_i16: int | None = None):
        """Outputs [first, first + count) of the cleaned take stay in HBM: float32 at d_f32 and / or int16 at d_i16 (None: not
        wanted); asynchronous on the context's stream."""
        pr = _noise_print_arg(noise_print)
        _call("mx_denoise_dev", self.handle, audio.handle, _ptr(pr), _denoise_params(reduction_db, sensitivity_db), first, count,
              _dev(d_f32), _dev(d_i16))

    def _pcm_range(self, name: str, audio: Audio, head: tuple, first: int, count: int | None, want_f32: bool, want_i16: bool):
        """name(ctx, audio, *head, first, count, f32, i16): samples [first, first + count) of a processed take (count None: to the
        take's end) -> (float32 | None, int16 | None)."""
        count = audio.n - first if count is None else count
        f, i = _pcm_pair(max(count, 0), want_f32, want_i16)
        _call(name, self.handle, audio.handle, *head, first, count, _ptr(f), _ptr(i))
        return f, i

    def denoise_range(self, audio: Audio, noise_print, reduction_db: float = 12.0, sensitivity_db: float = 6.0, first: int = 0,
                      count: int | None = None, want_f32: bool = True, want_i16: bool = False):
        """-> (float32 | None, int16 | None) outputs [first, first + count) of the cleaned take (count None: to its end).  Blocks."""
        pr = _noise_print_arg(noise_print)
        return self._pcm_range("mx_denoise", audio, (_ptr(pr), _denoise_params(reduction_db, sensitivity_db)), first, count,
                               want_f32, want_i16)

    # ---- dynamics compressor and its gain-reduction curve (build-defined; include/melonix_amd.h).  params: fields of
    # compress_params_default() ----
    def compress(self, audio: Audio, sr: int, **params) -> Audio:
        """A new Audio: `audio` through the compressor at sr.  Asynchronous on the context's stream."""
        return self._audio(audio.n, "mx_audio_compress", audio.handle, int(sr), _params_arg("compress", params, True, (int(sr),)))

    def compress_dev(self, audio: Audio, sr: int, first: int, count: int, d_f32: int | None = None, d_i16: int | None = None, **params):
        """Outputs [first, first + count) of the compressed take stay in HBM: float32 at d_f32 and / or int16 at d_i16 (None: not
        wanted); asynchronous on the context's stream."""
        _call("mx_compress_dev", self.handle, audio.handle, int(sr), _params_arg("compress", params, True, (int(sr),)), first, count,
              _dev(d_f32), _dev(d_i16))

    def compress_range(self, audio: Audio, sr: int, first: int = 0, count: int | None = None, want_f32: bool = True,
                       want_i16: bool = False, **params):
        """-> (float32 | None, int16 | None) outputs [first, first + count) of the compressed take (count None: to its end).  Blocks."""
        return self._pcm_range("mx_compress", audio, (int(sr), _params_arg("compress", params, True, (int(sr),))), first, count,
                               want_f32, want_i16)

    def compress_gain(self, audio: Audio, sr: int, first_step: int = 0, nsteps: int | None = None, **params):
        """-> the smoothed gain s_b of steps [first_step, first_step + nsteps) as int32 Q30 (nsteps None: to the last): the
        gain-reduction meter, 20 log10(s / 2^30) dB.  Blocks."""
        nsteps = compress_steps(audio.n, sr) - first_step if nsteps is None else nsteps
        out = np.empty(max(nsteps, 0), dtype=np.int32)
        _call("mx_compress_gain", self.handle, audio.handle, int(sr), _params_arg("compress", params, True, (int(sr),)), first_step, nsteps,
              _ptr(out))
        return out

    def compress_gain_dev(self, audio: Audio, sr: int, first_step: int, nsteps: int, d_gain: int, **params):
        """The same curve stays in HBM at d_gain (int32); asynchronous on the context's stream."""
        _call("mx_compress_gain_dev", self.handle, audio.handle, int(sr), _params_arg("compress", params, True, (int(sr),)), first_step, nsteps,
              _dev(d_gain))

    def compress_peaks_dev(self, audio: Audio, sr: int, first_step: int, nsteps: int, d_peaks: int):
        """The peaks p_b of steps [first_step, first_step + nsteps) stay in HBM at d_peaks (float32); asynchronous on the
        context's stream."""
        _call("mx_compress_peaks_dev", self.handle, audio.handle, int(sr), first_step, nsteps, _dev(d_peaks))

    # ---- tempo and grid offset from the onset-strength curve (build-defined; include/melonix_amd.h) ----
    def tempo_smooth(self, flux, width: int = 4):
        """-> the smoothed float32 curve of a host flux curve (half-width `width`; 0: the sanitising copy)."""
        flux = np.ascontiguousarray(flux, dtype=np.float32)
        out = np.empty(len(flux), dtype=np.float32)
        _call("mx_tempo_smooth", self.handle, _opt(flux), len(flux), width, _opt(out))
        return out

    def tempo_smooth_dev(self, d_flux: int, count: int, width: int, d_out: int):
        """count floats at d_flux -> d_out, both in HBM; asynchronous on the context's stream."""
        _call("mx_tempo_smooth_dev", self.handle, _dev(d_flux), count, width, _dev(d_out))

    def tempo_comb(self, curve, jobs):
        """COMB_JOB_DTYPE jobs (or (first, frames, period_q16) tuples) over a host curve -> COMB_DTYPE records, one per job."""
        curve = np.ascontiguousarray(curve, dtype=np.float32)
        jobs = _records(jobs, COMB_JOB_DTYPE)
        out = np.empty(len(jobs), dtype=COMB_DTYPE)
        _call("mx_tempo_comb", self.handle, _opt(curve), len(curve), _opt(jobs), len(jobs), _opt(out))
        return out

    def tempo_comb_dev(self, d_curve: int, count: int, d_jobs: int, njobs: int, d_out: int):
        """Jobs and curve in HBM -> njobs records at d_out; asynchronous on the context's stream.  The jobs are not checked."""
        _call("mx_tempo_comb_dev", self.handle, _dev(d_curve), count, _dev(d_jobs), njobs, _dev(d_out))

    @staticmethod
    def _tempo(want_windows: bool, name: str, *args):
        """name(*args, &tempo, &windows | NULL, &count | NULL) -> dict of mx_tempo's fields, with want_windows (dict, windows)."""
        t, win, cnt = _capi.Tempo(), C.c_void_p(), C.c_int64()
        _call(name, *args, C.byref(t), C.byref(win) if want_windows else None, C.byref(cnt) if want_windows else None)
        return (_fields(t), _take_records(win, cnt.value, TEMPO_WINDOW_DTYPE)) if want_windows else _fields(t)

    def tempo_from_flux(self, flux, sr: int, hop: int = 256, first_frame: int = 0, want_windows: bool = False, **params):
        """Tempo and grid offset of a host flux curve (flux[0] = frame first_frame) -> dict of mx_tempo's fields, with
        want_windows (dict, TEMPO_WINDOW_DTYPE array).  params: fields of tempo_params_default()."""
        flux = np.ascontiguousarray(flux, dtype=np.float32)
        return self._tempo(want_windows, "mx_tempo_from_flux", self.handle, _opt(flux), len(flux), sr, hop, first_frame,
                           _params_arg("tempo", params))

    def tempo_detect(self, audio: Audio, sr: int, hop: int = 256, flux_params: dict | None = None, want_windows: bool = False,
                     **params):
        """Flux over the whole file, kept in HBM, and the estimate from it; as tempo_from_flux."""
        return self._tempo(want_windows, "mx_tempo_detect", self.handle, audio.handle, sr, hop, _params_arg("flux", flux_params or {}),
                           _params_arg("tempo", params))

    # ---- grains / resynthesis ----
    def grains_dev(self, audio: Audio):
        s, l, cnt = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64()
        _call("mx_grains_dev", self.handle, audio.handle, C.byref(s), C.byref(l), C.byref(cnt))
        return _take_array(s, cnt.value), _take_array(l, cnt.value)

    def grain_table_dev(self, audio: Audio):
        """-> (starts, lens, firsts): the grain chain built on the device, with every grain's first sample."""
        s, l, f, cnt = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int64()
        _call("mx_grain_table_dev", self.handle, audio.handle, C.byref(s), C.byref(l), C.byref(f), C.byref(cnt))
        firsts = _take_array(f, cnt.value)
        return _take_array(s, cnt.value), _take_array(l, cnt.value), firsts

    def resynth(self, audio: Audio, steps, nsamples: int, want_f32: bool = True, want_i16: bool = True):
        steps = np.ascontiguousarray(steps, dtype=STEP_DTYPE)
        f32, i16 = _pcm_pair(nsamples, want_f32, want_i16)
        _call("mx_resynth", self.handle, audio.handle, _ptr(steps), len(steps), nsamples, _ptr(f32), _ptr(i16))
        return f32, i16

    def resynth_dev(self, audio: Audio, d_steps: int, nsteps: int, nsamples: int, d_f32: int | None,
                    d_i16: int | None):
        _call("mx_resynth_dev", self.handle, audio.handle, C.c_void_p(d_steps), nsteps, nsamples, _dev(d_f32), _dev(d_i16))

    def pv_set_chunk_frames(self, frames: int):
        """Override of the phase vocoder's arena policy: two-slot chunks of exactly `frames` frames (rounded up to a multiple of
        32); 0 = back to the budget (resident when the call fits, else the longest chunks it holds)."""
        _call("mx_pv_set_chunk_frames", self.handle, int(frames))

    def pv_set_arena_budget(self, nbytes: int):
        """Bytes the phase vocoder's work arena may take; 0 = the default (MELONIX_PV_ARENA_MB, else a quarter of the free memory)."""
        _call("mx_pv_set_arena_budget", self.handle, int(nbytes))

    def pv_arena_budget(self) -> int:
        return _call("mx_pv_arena_budget", self.handle)

    def pv_last_chunks(self) -> int:
        """Chunks the last phase-vocoder run of this context took (1 = resident)."""
        return int(_capi.lib().mx_pv_last_chunks(self.handle))

    def pv_arena_bytes(self) -> int:
        """Bytes of the phase vocoder's work arena this context holds (0 before the first call)."""
        return int(_capi.lib().mx_pv_arena_bytes(self.handle))

    def pv_pitch_shift(self, audio: Audio, semitones: float, want_f32: bool = True, want_i16: bool = True):
        """Build-defined phase-vocoder pitch shift (no reference counterpart) -> (f32 | None, int16 | None)."""
        f32, i16 = _pcm_pair(audio.n, want_f32, want_i16)
        _call("mx_pv_pitch_shift", self.handle, audio.handle, float(semitones), _ptr(f32), _ptr(i16))
        return f32, i16

    def pv_pitch_shift_dev(self, audio: Audio, semitones: float, d_f32: int | None, d_i16: int | None):
        _call("mx_pv_pitch_shift_dev", self.handle, audio.handle, float(semitones), _dev(d_f32), _dev(d_i16))

    def pv_render(self, audio: Audio, sr: int, markers, want_f32: bool = True, want_i16: bool = True):
        """Marker-driven phase vocoder (build-defined) -> (f32 | None, int16 | None) over the warped duration."""
        m = _capi.markers_array(markers)
        f32, i16 = _pcm_pair(_call("mx_pv_render_length", audio.n, sr, m, len(markers)), want_f32, want_i16)
        _call("mx_pv_render", self.handle, audio.handle, sr, m, len(markers), _ptr(f32), _ptr(i16))
        return f32, i16

    # ---- formant-preserving PSOLA rendering driven by the f0 track, and the independent formant shift on it (build-defined;
    # include/melonix_amd.h).  Each call is written once over the record kind (`formant`: the "_formant" entry point, its
    # record dtype and, for a plan or a render, its points: _PSOLA_KINDS) and over `bent` (the "_bend" entry point, which takes
    # a bend curve, or NULL, after the points) ----
    def _psola_synth(self, formant: bool, audio: Audio, grains, nsamples: int, want_f32: bool, want_i16: bool):
        sfx, dtype = _PSOLA_KINDS[formant]
        grains = np.ascontiguousarray(grains, dtype=dtype)
        f32, i16 = _pcm_pair(nsamples, want_f32, want_i16)
        _call("mx_psola_synth" + sfx, self.handle, audio.handle, _opt(grains), len(grains), nsamples, _ptr(f32), _ptr(i16))
        return f32, i16

    def _psola_synth_dev(self, formant: bool, audio: Audio, d_grains, ngrains: int, nsamples: int, d_f32, d_i16):
        _call(f"mx_psola_synth{_PSOLA_KINDS[formant][0]}_dev", self.handle, audio.handle, _dev(d_grains), ngrains, nsamples,
              _dev(d_f32), _dev(d_i16))

    def _psola_render(self, formant: bool, bent: bool, audio: Audio, sr: int, hop: int, track, markers, points, bend, params: dict,
                      want=None, dev=None):
        """mx_psola_render, mx_psola_render_formant (formant) or mx_psola_render_bend (formant and bent: it takes the points
        and then the curve, or NULL).  want: (want_f32, want_i16), host outputs over the warped duration; dev: (d_f32, d_i16)
        instead, the "_dev" entry point, nothing returned."""
        track = np.ascontiguousarray(track, dtype=F0_DTYPE)
        m = _capi.markers_array(markers)
        pts = _formant_points(points) if formant else None
        b = _bend_arg(bend, len(track)) if bent else None  # (held here: it must outlive the call, like pts)
        name = "mx_psola_render" + ("_bend" if bent else _PSOLA_KINDS[formant][0]) + ("_dev" if dev else "")
        f32, i16 = (None, None) if dev else _pcm_pair(_call("mx_pv_render_length", audio.n, sr, m, len(markers)), *want)
        _call(name, self.handle, audio.handle, sr, hop, _opt(track), len(track), _params_arg("psola", params), m, len(markers),
              *_points_args(pts), *((_ptr(b),) if bent else ()), *(map(_dev, dev) if dev else (_ptr(f32), _ptr(i16))))
        return f32, i16

    def psola_synth(self, audio: Audio, grains, nsamples: int, want_f32: bool = True, want_i16: bool = True):
        """The overlap-add over PSOLA_GRAIN_DTYPE records (psola_plan) -> (f32 | None, int16 | None) of nsamples each; the
        records are checked first (MxError MX_ERR_INVALID, nothing launched)."""
        return self._psola_synth(False, audio, grains, nsamples, want_f32, want_i16)

    def psola_synth_dev(self, audio: Audio, d_grains: int, ngrains: int, nsamples: int, d_f32: int | None, d_i16: int | None):
        """Device pointers; asynchronous on the context's stream.  The records are NOT checked (include/melonix_amd.h)."""
        self._psola_synth_dev(False, audio, d_grains, ngrains, nsamples, d_f32, d_i16)

    def psola_render(self, audio: Audio, sr: int, hop: int, track, markers, want_f32: bool = True, want_i16: bool = True,
                     **params):
        """Plan and synthesis in one call -> (f32 | None, int16 | None) over the warped duration (pv_render's length).
        track: the F0_DTYPE records of every frame of the file at `hop`; params: fields of psola_params_default()."""
        return self._psola_render(False, False, audio, sr, hop, track, markers, None, None, params, want=(want_f32, want_i16))

    def psola_synth_formant(self, audio: Audio, fgrains, nsamples: int, want_f32: bool = True, want_i16: bool = True):
        """psola_synth over PSOLA_FGRAIN_DTYPE records (psola_plan_formant); the records are checked first."""
        return self._psola_synth(True, audio, fgrains, nsamples, want_f32, want_i16)

    def psola_synth_formant_dev(self, audio: Audio, d_fgrains: int, ngrains: int, nsamples: int, d_f32: int | None,
                                d_i16: int | None):
        """Device pointers; asynchronous on the context's stream.  The records are NOT checked (include/melonix_amd.h)."""
        self._psola_synth_dev(True, audio, d_fgrains, ngrains, nsamples, d_f32, d_i16)

    def psola_render_formant(self, audio: Audio, sr: int, hop: int, track, markers, points, want_f32: bool = True,
                             want_i16: bool = True, **params):
        """psola_render with the envelope moved along `points`: (source sample, semitones) pairs, samples strictly
        increasing.  No points: psola_render itself."""
        return self._psola_render(True, False, audio, sr, hop, track, markers, points, None, params,
                                  want=(want_f32, want_i16))

    def psola_render_bend(self, audio: Audio, sr: int, hop: int, track, markers, bend, points=(), want_f32: bool = True,
                          want_i16: bool = True, **params):
        """psola_render_formant following a bend curve (float32 semitones per frame of the track, contour_bend's); no points:
        the plain records and kernel."""
        return self._psola_render(True, True, audio, sr, hop, track, markers, points, bend, params,
                                  want=(want_f32, want_i16))

    def psola_render_bend_dev(self, audio: Audio, sr: int, hop: int, track, markers, bend, points, d_f32: int | None,
                              d_i16: int | None, **params):
        """The same with the PCM left in HBM (the render's length each); blocks until the records are uploaded and used."""
        self._psola_render(True, True, audio, sr, hop, track, markers, points, bend, params, dev=(d_f32, d_i16))

    # ---- one rank of a multi-GPU phase-vocoder run (melonix_amd.shard.pv_pitch_shift_rank drives these) ----
    def pv_shard_analyze(self, audio: Audio, semitones: float, rank: int, world: int):
        """Stage 1 -> (tot_sums uint32[2048], tot_org uint16[2048]): this rank's frames as one map of the phase row."""
        sums = np.empty(2048, dtype=np.uint32)
        org = np.empty(2048, dtype=np.uint16)
        _call("mx_pv_shard_analyze", self.handle, audio.handle, float(semitones), rank, world, _ptr(sums), _ptr(org))
        return sums, org

    def pv_shard_synthesize(self, carry_in):
        """Stage 2 -> (head, tail) float32[3840] raw seams; carry_in: uint32[2048] or None on rank 0."""
        head = np.empty(3840, dtype=np.float32)
        tail = np.empty(3840, dtype=np.float32)
        c = None if carry_in is None else np.ascontiguousarray(carry_in, dtype=np.uint32)
        _call("mx_pv_shard_synthesize", self.handle, _ptr(c), _ptr(head), _ptr(tail))
        return head, tail

    def pv_shard_finish(self, count: int, prev_tail, next_head, want_f32: bool = True, want_i16: bool = True):
        """Stage 3 -> (f32 | None, int16 | None) of `count` = out_hi - out_lo samples (pv_shard_frames)."""
        f32, i16 = _pcm_pair(count, want_f32, want_i16)
        pt = None if prev_tail is None else np.ascontiguousarray(prev_tail, dtype=np.float32)
        nh = None if next_head is None else np.ascontiguousarray(next_head, dtype=np.float32)
        _call("mx_pv_shard_finish", self.handle, _ptr(pt), _ptr(nh), _ptr(f32), _ptr(i16))
        return f32, i16

    # (the same stages with everything on the device: pointers are integers, e.g. torch tensors' data_ptr())
    def pv_shard_analyze_dev(self, audio: Audio, semitones: float, rank: int, world: int, d_map_out: int):
        _call("mx_pv_shard_analyze_dev", self.handle, audio.handle, float(semitones), int(rank), int(world),
              C.c_void_p(int(d_map_out)))

    def pv_shard_synthesize_dev(self, d_maps_all: int, d_f32: int | None, d_i16: int | None, d_seams_out: int):
        _call("mx_pv_shard_synthesize_dev", self.handle, C.c_void_p(int(d_maps_all)), _dev(int(d_f32 or 0)), _dev(int(d_i16 or 0)),
              C.c_void_p(int(d_seams_out)))

    def pv_shard_finish_dev(self, d_seams_all: int):
        _call("mx_pv_shard_finish_dev", self.handle, C.c_void_p(int(d_seams_all)))

    def minmax_pyramid(self, audio: Audio):
        """App::calcPicks on the GPU -> list of (count_l, 2) float32 arrays {min,max}, one per level."""
        picks = np.empty(2 * max(audio.n, 1), dtype=np.float32)
        counts = np.zeros(64, dtype=np.int64)
        nl = C.c_int()
        _call("mx_minmax_pyramid", self.handle, audio.handle, _ptr(picks), _ptr(counts), C.byref(nl))
        out, off = [], 0
        for l in range(nl.value):
            out.append(picks[off:off + 2 * counts[l]].reshape(-1, 2).copy())
            off += 2 * int(counts[l])
        return out

    def resynth_to_wav(self, audio: Audio, steps, nsamples: int, sr: int, path: str, strict: bool = True):
        """Resynthesis of a built schedule straight into a WAV file (PCM streamed off the device in pieces)."""
        steps = np.ascontiguousarray(steps)
        _call("mx_resynth_to_wav", self.handle, audio.handle, _opt(steps), len(steps), nsamples, str(path).encode(), sr,
              1 if strict else 0)

    def export_wav(self, wav, sr: int, markers, path: str, strict: bool = True):
        wav = np.ascontiguousarray(wav, dtype=np.float32)
        m = _capi.markers_array(markers)
        _call("mx_export_wav", self.handle, _ptr(wav), len(wav), sr, m, len(markers), str(path).encode(), 1 if strict else 0)


def _take_steps(p, count):
    """The library-allocated step array as a numpy structured array, without a copy: the array owns the allocation
    (mx_free runs when the last view of it goes)."""
    if not count:
        _capi.lib().mx_free(p)
        return np.zeros(0, STEP_DTYPE)
    import weakref

    addr = C.addressof(p.contents)
    buf = (C.c_char * (count * C.sizeof(_capi.Step))).from_address(addr)
    weakref.finalize(buf, _capi.lib().mx_free, C.c_void_p(addr))
    return np.frombuffer(buf, dtype=STEP_DTYPE)


def _take_array(p, cnt):
    """A library-allocated array of cnt int32 or float values (p: the typed pointer) as a numpy array of its own; mx_free."""
    out = np.ctypeslib.as_array(p, shape=(max(cnt, 1),))[:cnt].copy()
    _capi.lib().mx_free(p)
    return out


# ---- host-side entry points (no GPU needed) ----
def grains_host(wav):
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    s, l, cnt = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64()
    _call("mx_grains", _ptr(wav), len(wav), C.byref(s), C.byref(l), C.byref(cnt))
    return _take_array(s, cnt.value), _take_array(l, cnt.value)


def _schedule(name: str, head, starts, lens, firsts, markers, resume=None):
    """The schedule builder `name`(*head, starts, lens, [firsts,] count, markers, count, [cursor0, need,] &steps, &nsteps,
    &nsamples, [&cursor_end]) -> (steps, nsamples), with resume = (cursor0, need) (steps, nsamples, cursor_end)."""
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    grains = (_ptr(starts), _ptr(lens)) if firsts is None else (_ptr(starts), _ptr(lens), _ptr(firsts))
    m = _capi.markers_array(markers)
    p, ns, tot, end = C.POINTER(_capi.Step)(), C.c_int64(), C.c_int64(), C.c_double()
    outs = (C.byref(p), C.byref(ns), C.byref(tot))
    if resume is None:
        _call(name, *head, *grains, len(starts), m, len(markers), *outs)
        return _take_steps(p, ns.value), tot.value
    _call(name, *head, *grains, len(starts), m, len(markers), float(resume[0]), int(resume[1]), *outs, C.byref(end))
    return _take_steps(p, ns.value), tot.value, end.value


def schedule_build(wav, sr: int, starts, lens, markers):
    """-> (steps structured array, nsamples)"""
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    return _schedule("mx_schedule_build", (_ptr(wav), len(wav), sr), starts, lens, None, markers)


def schedule_build_table(n: int, sr: int, starts, lens, firsts, markers, cursor0: float = 0.0, need: int = -1):
    """The export / refill schedule from a grain table (Context.grain_table_dev): no host copy of the audio needed.
    -> (steps, nsamples, cursor_end)"""
    firsts = np.ascontiguousarray(firsts, dtype=np.float32)
    return _schedule("mx_schedule_build_table", (int(n), sr), starts, lens, firsts, markers, (cursor0, need))


def schedule_build_from(wav, sr: int, starts, lens, markers, cursor0: float, need: int):
    """App::playback's refill loop from warped time cursor0 -> (steps, nsamples, cursor_end)."""
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    return _schedule("mx_schedule_build_from", (_ptr(wav), len(wav), sr), starts, lens, None, markers, (cursor0, need))


def save_wav(path, pcm16, sr: int, strict: bool = True):
    pcm16 = np.ascontiguousarray(pcm16, dtype=np.int16)
    _call("mx_save_wav", str(path).encode(), _ptr(pcm16), len(pcm16), sr, 1 if strict else 0)


def minmax_range(wav, levels, start, end):
    """App::getMinMaxFromRange over a pyramid from Context.minmax_pyramid (host)."""
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    flat = np.ascontiguousarray(np.concatenate([l.reshape(-1) for l in levels]) if levels else np.zeros(2, np.float32))
    counts = np.zeros(64, dtype=np.int64)
    counts[:len(levels)] = [len(l) for l in levels]
    a, b = C.c_float(), C.c_float()
    _capi.lib().mx_minmax_range(_ptr(wav), len(wav), _ptr(flat), _ptr(counts), len(levels), int(start), int(end),
                                C.byref(a), C.byref(b))
    return a.value, b.value


def sample2time(markers, sr, val):
    return _capi.lib().mx_sample2time(_capi.markers_array(markers), len(markers), sr, int(val))


def time2sample(markers, sr, val):
    return _capi.lib().mx_time2sample(_capi.markers_array(markers), len(markers), sr, float(val))


def duration(markers, sr, n):
    return _capi.lib().mx_duration(_capi.markers_array(markers), len(markers), sr, int(n))


def time2pitchbend(markers, sr, n, val):
    return _capi.lib().mx_time2pitchbend(_capi.markers_array(markers), len(markers), sr, int(n), float(val))


def column_range(markers, sr, time, width, range_time):
    k, s, e = C.c_int(), C.c_int(), C.c_int()
    _capi.lib().mx_column_range(_capi.markers_array(markers), len(markers), sr, float(time), int(width),
                                float(range_time), C.byref(k), C.byref(s), C.byref(e))
    return k.value, s.value, e.value


# ---- notes and correction markers (host; build-defined) ----
def detect_notes(track, sr: int, hop: int, first: int = 0, **params):
    """Notes of an F0_DTYPE track (track[0] = frame `first`) -> NOTE_DTYPE array.  params: threshold, rms_floor, max_jump,
    max_dev, min_frames (defaults: note_params_default())."""
    track = np.ascontiguousarray(track, dtype=F0_DTYPE)
    out, cnt = C.POINTER(_capi.Note)(), C.c_int64()  # (a typed pointer in this entry point's signature: not _handed)
    _call("mx_detect_notes", _opt(track), len(track), sr, hop, first, _params_arg("note", params, never_null=True), C.byref(out),
          C.byref(cnt))
    return _take_records(C.cast(out, C.c_void_p), cnt.value, NOTE_DTYPE)  # (no notes: a null array)


def correction_markers(notes, strength: float = 1.0, scale_mask: int = 0):
    """Two markers per note (MARKER_DTYPE): {start, note, 0, b}, {end, note, 0, b}, b = strength * (target - note)."""
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    out = np.zeros(2 * len(notes), dtype=MARKER_DTYPE)
    _call("mx_correction_markers", _opt(notes), len(notes), float(strength), int(scale_mask), _opt(out))
    return out


def correction_markers_tuned(notes, strength: float = 1.0, scale_mask: int = 0, tuning_cents: float = 0.0):
    """correction_markers on a grid `tuning_cents` above A = 440 Hz (key_detect's or key_from_notes' tuning_cents)."""
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    out = np.zeros(2 * len(notes), dtype=MARKER_DTYPE)
    _call("mx_correction_markers_tuned", _opt(notes), len(notes), float(strength), int(scale_mask), float(tuning_cents), _opt(out))
    return out


# ---- key, scale and tuning (host; build-defined) ----
def _key_dict(key) -> dict:
    return {k: v for k, v in _fields(key).items() if k != "reserved"}


def key_from_chroma(sum40) -> dict:
    """The key estimate from a 40-value chroma sum (Context.chroma_sum) -> dict of KEY_DTYPE's fields."""
    s = np.ascontiguousarray(sum40, dtype=np.float64)
    if s.shape != (CHROMA_COLS,):
        raise ValueError("a chroma sum is 40 values")
    key = _capi.Key()
    _call("mx_key_from_chroma", _ptr(s), C.byref(key))
    return _key_dict(key)


def key_from_notes(notes) -> dict:
    """The key estimate from detect_notes' output (NOTE_DTYPE), each note weighing its frames."""
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    key = _capi.Key()
    _call("mx_key_from_notes", _opt(notes), len(notes), C.byref(key))
    return _key_dict(key)


# ---- PSOLA planning (host; build-defined) ----
def _formant_points(points):
    """(sample, semitones) pairs, or a FORMANT_POINT_DTYPE array -> a contiguous FORMANT_POINT_DTYPE array."""
    return _records(points, FORMANT_POINT_DTYPE)


# the two record kinds, by `formant`: the entry points' suffix and the record dtype
_PSOLA_KINDS = {False: ("", PSOLA_GRAIN_DTYPE), True: ("_formant", PSOLA_FGRAIN_DTYPE)}


def _points_args(pts):
    """The two extra arguments of an entry point that takes a formant curve, (points | NULL, count); () for None.  pts must
    outlive the call."""
    return () if pts is None else (_opt(pts), len(pts))


def _bend_arg(bend, count: int):
    if bend is None:
        return None
    bend = np.ascontiguousarray(bend, dtype=np.float32)
    if len(bend) != count:
        raise ValueError("a bend curve has one value per frame of the track")
    return bend


def _psola_plan(formant: bool, bent: bool, n: int, sr: int, hop: int, track, markers, points, bend, params: dict):
    """mx_psola_plan, mx_psola_plan_formant, mx_psola_plan_bend or mx_psola_plan_formant_bend.  The kind alone picks symbol,
    dtype and whether points are passed: whatever `points` is, they cannot disagree."""
    track = np.ascontiguousarray(track, dtype=F0_DTYPE)
    m = _capi.markers_array(markers)
    sfx, dtype = _PSOLA_KINDS[formant]
    pts = _formant_points(points) if formant else None
    b = _bend_arg(bend, len(track)) if bent else None  # (held here: it must outlive the call, like pts)
    ns = C.c_int64()
    grains = _handed(dtype, "mx_psola_plan" + sfx + ("_bend" if bent else ""), n, sr, hop, _opt(track), len(track),
                     _params_arg("psola", params), m, len(markers), *_points_args(pts), *((_ptr(b),) if bent else ()), tail=(C.byref(ns),))
    return grains, ns.value


def psola_plan(n: int, sr: int, hop: int, track, markers, **params):
    """Grain records of a PSOLA render -> (PSOLA_GRAIN_DTYPE array, nsamples).  track: the F0_DTYPE records of the file's
    frame_count(n, hop) frames; params: fields of psola_params_default()."""
    return _psola_plan(False, False, n, sr, hop, track, markers, None, None, params)


def psola_plan_formant(n: int, sr: int, hop: int, track, markers, points, **params):
    """psola_plan with a formant curve -> (PSOLA_FGRAIN_DTYPE array, nsamples).  points: (source sample, semitones) pairs,
    samples strictly increasing; none: every record's step is 65536."""
    return _psola_plan(True, False, n, sr, hop, track, markers, points, None, params)


def psola_plan_bend(n: int, sr: int, hop: int, track, markers, bend, **params):
    """psola_plan following a bend curve (float32 semitones, one per frame of the track; None: psola_plan itself)."""
    return _psola_plan(False, True, n, sr, hop, track, markers, None, bend, params)


def psola_plan_formant_bend(n: int, sr: int, hop: int, track, markers, points, bend, **params):
    """psola_plan_formant following a bend curve."""
    return _psola_plan(True, True, n, sr, hop, track, markers, points, bend, params)


# ---- pitch drift and vibrato inside notes (host; build-defined) ----
def contour_spans(notes, first: int = 0):
    """The spans of detect_notes' output relative to a track whose record 0 is frame `first` -> CONTOUR_SPAN_DTYPE array."""
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    out = np.zeros(len(notes), dtype=CONTOUR_SPAN_DTYPE)
    _call("mx_contour_spans", _opt(notes), len(notes), first, _opt(out))
    return out


def contour_vibrato(stat, frames: int, sr: int, hop: int) -> dict:
    """rate_hz, extent_cents, strength, drift_cents of one CONTOUR_STAT_DTYPE record of a span of `frames` frames."""
    s = np.ascontiguousarray(np.asarray(stat, dtype=CONTOUR_STAT_DTYPE).reshape(1))
    v = _capi.Vibrato()
    _call("mx_contour_vibrato", _ptr(s), int(frames), sr, hop, C.byref(v))
    return _fields(v)


def contour_bend(rec, notes, spans, shift=None, **params):
    """The bend curve (float32 semitones per frame) that corrects the notes: rec from Context.contour_split / pitch_contour,
    shift one float per note (None: 0); params: drift_amount, vibrato_scale, glide_frames (bend_params_default())."""
    rec = np.ascontiguousarray(rec, dtype=CONTOUR_REC_DTYPE)
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    spans = _records(spans, CONTOUR_SPAN_DTYPE)
    if len(spans) != len(notes):
        raise ValueError("one span per note")
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    if sh is not None and len(sh) != len(notes):
        raise ValueError("one shift per note")
    out = np.zeros(len(rec), dtype=np.float32)
    _call("mx_contour_bend", _opt(rec), len(rec), _opt(notes), _opt(spans), len(notes), _ptr(sh), _params_arg("bend", params),
          _opt(out))
    return out


# ---- onsets and timing markers (host; build-defined) ----
def onset_pick(flux, hop: int, first: int = 0, **params):
    """Onsets of an onset-strength curve (flux[0] = frame `first`) -> ONSET_DTYPE array.  params: fields of
    onset_pick_params_default()."""
    flux = np.ascontiguousarray(flux, dtype=np.float32)
    return _handed(ONSET_DTYPE, "mx_onset_pick", _opt(flux), len(flux), hop, first, _params_arg("pick", params))


def timing_markers(anchors, n: int, sr: int, base=None, **params):
    """The markers that move `anchors` (source samples) onto the tempo grid -> MARKER_DTYPE array.  base: a MARKER_DTYPE
    array (correction_markers) or (sample, note, dTime, pitchBend) tuples to merge; params: fields of timing_params_default()."""
    anchors = np.ascontiguousarray(anchors, dtype=np.int32)
    base = _records(() if base is None else base, MARKER_DTYPE)
    return _handed(MARKER_DTYPE, "mx_timing_markers", _opt(anchors), len(anchors), int(n), sr, _params_arg("timing", params),
                   _opt(base), len(base))


# ---- sibilant segments, protected formant curves, balance points (host; build-defined) ----
def sibilants(feat, hop: int = 256, first: int = 0, **params):
    """Segments of SIB_FEAT_DTYPE records (feat[0] = frame `first`) -> SIBILANT_DTYPE array.  params: fields of
    sibilant_params_default()."""
    feat = _records(feat, SIB_FEAT_DTYPE)
    return _handed(SIBILANT_DTYPE, "mx_sibilants", _opt(feat), len(feat), hop, first, _params_arg("sibilant", params))


def formant_protect(points, sibs, ramp: int, n: int):
    """A formant curve ((sample, semitones) pairs) held at 0 st across `sibs` (SIBILANT_DTYPE), `ramp` samples of linear
    return either side -> FORMANT_POINT_DTYPE array that psola_plan_formant takes as it is."""
    pts, sibs = _formant_points(points), _records(sibs, SIBILANT_DTYPE)
    return _handed(FORMANT_POINT_DTYPE, "mx_formant_protect", _opt(pts), len(pts), _opt(sibs), len(sibs), int(ramp), int(n))


def sibilant_gain_points(sibs, db: float, ramp: int, n: int):
    """The gain points of a sibilant balance of `db` decibels -> GAIN_POINT_DTYPE array for Context.audio_gain."""
    sibs = _records(sibs, SIBILANT_DTYPE)
    return _handed(GAIN_POINT_DTYPE, "mx_sibilant_gain_points", _opt(sibs), len(sibs), float(db), int(ramp), int(n))


# ---- loudness curves, gating, note loudness, levelling points, export gain (host; build-defined) ----
def loudness_step_count(n: int, sr: int) -> int:
    """ceil(n / S), S = (sr + 50) // 100 the 10 ms step; 0 for n < 1 or a sample rate outside [8000, 384000]."""
    return int(_capi.lib().mx_loudness_step_count(int(n), int(sr)))


def loudness_coeffs(sr: int):
    """The K-weighting coefficients at sr -> float64[10]: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass."""
    out = np.empty(10, dtype=np.float64)
    _call("mx_loudness_coeffs", int(sr), _ptr(out))
    return out


def loudness_curve(steps, sr: int, window_steps: int = 40):
    """Loudness over a sliding window of LOUD_STEP_DTYPE records (steps[0] = step 0) -> float64[nsteps], -inf where the window
    is not full.  window_steps 40: momentary; 300: short-term."""
    steps = _records(steps, LOUD_STEP_DTYPE)
    out = np.empty(len(steps), dtype=np.float64)
    _call("mx_loudness_curve", _opt(steps), len(steps), int(sr), int(window_steps), _opt(out))
    return out


def loudness_integrated(steps, sr: int) -> dict:
    """BS.1770-4 gated loudness of LOUD_STEP_DTYPE records -> dict of mx_loudness' fields."""
    steps = _records(steps, LOUD_STEP_DTYPE)
    m = _capi.Loudness()
    _call("mx_loudness_integrated", _opt(steps), len(steps), int(sr), C.byref(m))
    return _fields(m)


def note_loudness(steps, sr: int, notes):
    """LUFS per note (NOTE_DTYPE) from LOUD_STEP_DTYPE records -> float64[nnotes]."""
    steps, notes = _records(steps, LOUD_STEP_DTYPE), np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    out = np.empty(len(notes), dtype=np.float64)
    _call("mx_note_loudness", _opt(steps), len(steps), int(sr), _opt(notes), len(notes), _opt(out))
    return out


def level_gain_points(notes, lufs, **params):
    """The gain points that move each note towards the median loudness -> (GAIN_POINT_DTYPE[2 * nnotes] for Context.audio_gain,
    the reference in LUFS).  params: fields of level_params_default() (`raise` is a Python keyword: pass it as raise_=, or
    through a dict)."""
    notes = np.ascontiguousarray(notes, dtype=NOTE_DTYPE)
    lufs = np.ascontiguousarray(lufs, dtype=np.float64)
    if len(lufs) != len(notes):
        raise ValueError("one loudness per note")
    params = {k[:-1] if k.endswith("_") else k: v for k, v in params.items()}
    out, ref = np.zeros(2 * len(notes), dtype=GAIN_POINT_DTYPE), C.c_double()
    _call("mx_level_gain_points", _opt(notes), len(notes), _opt(lufs), _params_arg("level", params), _opt(out), C.byref(ref))
    return out, ref.value


def normalize_gain(measured: dict, target_lufs: float = -23.0, ceiling_db: float = -1.0) -> float:
    """The gain (as float32) that brings a take measured by loudness_integrated / Context.loudness_measure to target_lufs with
    its sample peak at most ceiling_db dBFS."""
    amp = C.c_float()
    _call("mx_normalize_gain", C.byref(_capi.Loudness(**measured)), float(target_lufs), float(ceiling_db), C.byref(amp))
    return amp.value


# ---- true peak, limiter parameters, loudness range, export gain under a true-peak ceiling (host; build-defined) ----
def true_peak_oversampling(sr: int) -> int:
    """L: 4 below 88.2 kHz, 2 below 176.4 kHz, else 1; 0 for a sample rate outside [8000, 384000]."""
    return int(_capi.lib().mx_true_peak_oversampling(int(sr)))


def true_peak_taps():
    """The interpolation taps -> float32[3, 12]: offsets 1/4, 1/2, 3/4, d = -5 .. 6."""
    out = np.empty((3, 12), dtype=np.float32)
    _call("mx_true_peak_taps", _ptr(out))
    return out


def limit_params_default(sr: int) -> dict:
    """The limiter's defaults at sr: a ceiling amplitude of -1 dBTP, a look-ahead of 5 ms (at most 1024 samples)."""
    p = _capi.LimitParams()
    _call("mx_limit_params_default", int(sr), C.byref(p))
    return _fields(p)


def loudness_range(steps, sr: int) -> dict:
    """EBU Tech 3342 loudness range of LOUD_STEP_DTYPE records -> dict of mx_loudness_range_result's fields."""
    steps = _records(steps, LOUD_STEP_DTYPE)
    r = _capi.LoudnessRange()
    _call("mx_loudness_range", _opt(steps), len(steps), int(sr), C.byref(r))
    return _fields(r)


def normalize_gain_tp(measured: dict, true_peak: float, target_lufs: float = -23.0, ceiling_dbtp: float = -1.0) -> float:
    """normalize_gain with a measured true peak (Context.true_peak) in place of the sample peak, the ceiling in dBTP."""
    amp = C.c_float()
    _call("mx_normalize_gain_tp", C.byref(_capi.Loudness(**measured)), float(true_peak), float(target_lufs), float(ceiling_dbtp),
          C.byref(amp))
    return amp.value


# ---- sample-rate conversion: the plan, the length and the tap table of a rate pair (host; build-defined) ----
def resample_plan(in_rate: int, out_rate: int) -> dict:
    """The plan of in_rate -> out_rate -> {L, M, taps, half}; equal rates: {1, 1, 0, 0}.  MxError for a refused pair."""
    p = _capi.ResamplePlan()
    _call("mx_resample_plan_for", int(in_rate), int(out_rate), C.byref(p))
    return _fields(p)


def resample_length(n: int, in_rate: int, out_rate: int) -> int:
    """m = ceil(n L / M): the samples of a take of n converted from in_rate to out_rate."""
    return _call("mx_resample_length", int(n), int(in_rate), int(out_rate))


def resample_taps(in_rate: int, out_rate: int):
    """The tap table -> float32[L, taps], a row per phase ([1, 0] for equal rates)."""
    p = resample_plan(in_rate, out_rate)
    out = np.empty((p["L"], p["taps"]), dtype=np.float32)
    _call("mx_resample_taps", int(in_rate), int(out_rate), _ptr(out))
    return out


# ---- noise reduction: the print and parameter arguments, the frame count, the factors, a print of rows (host; build-defined) ----
DENOISE_BINS = _capi.DENOISE_BINS


def _noise_print_arg(noise_print):
    pr = np.ascontiguousarray(noise_print, dtype=np.float32)
    if pr.shape != (DENOISE_BINS,):
        raise ValueError(f"a noise print has {DENOISE_BINS} values")
    return pr


def _denoise_params(reduction_db: float, sensitivity_db: float):
    return C.byref(_capi.DenoiseParams(float(reduction_db), float(sensitivity_db)))


def denoise_frames(n: int) -> int:
    """F = ceil(n / 256) + 3: the frames of the noise reduction over a take of n samples."""
    return _call("mx_denoise_frames", int(n))


def denoise_factors(reduction_db: float, sensitivity_db: float):
    """-> (floor, sens) as float32: the two factors the device, the emulation and numpy read."""
    out = np.empty(2, dtype=np.float32)
    _call("mx_denoise_factors", _denoise_params(reduction_db, sensitivity_db), _ptr(out))
    return out[0], out[1]


def noise_print_rows(rows):
    """The print of power rows (count x 513 float32) by the library's host form."""
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, DENOISE_BINS)
    out = np.empty(DENOISE_BINS, dtype=np.float32)
    _call("mx_noise_print_rows", _ptr(rows), len(rows), _ptr(out))
    return out


# ---- dynamics compressor: the defaults, the plan, the curve and the step count (host; build-defined) ----
COMPRESS_CURVE = _capi.COMPRESS_CURVE


def compress_params_default(sr: int = 48000) -> dict:
    """The compressor's defaults: -18 dB, 4 : 1, a 6 dB knee, 5 ms / 100 ms, no look-ahead, make-up 1."""
    return _params_default("compress", int(sr))


def compress_plan(sr: int, **params) -> dict:
    """The plan of `params` at sr -> {D, K, c_att, c_rel, W, Gc}.  MxError for a refused rate or parameter."""
    q = _capi.CompressPlan()
    _call("mx_compress_plan_for", int(sr), _params_arg("compress", params, True, (int(sr),)), C.byref(q))
    return _fields(q)


def compress_curve(**params):
    """-> the 2049 Q30 gain targets (int32) of `params`: what the device, the emulation and numpy look up."""
    out = np.empty(COMPRESS_CURVE, dtype=np.int32)
    _call("mx_compress_curve", _params_arg("compress", params, True, (48000,)), _ptr(out))
    return out


def compress_steps(n: int, sr: int) -> int:
    """B = ceil(n / D), D = (sr + 500) // 1000: the control steps of the compressor over a take of n samples."""
    return _call("mx_compress_steps", int(n), int(sr))
