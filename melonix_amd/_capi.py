"""ctypes binding of include/melonix_amd.h (the C-ABI of libmelonix_amd.so).

Thin by design: every function maps 1:1 onto a C entry point.  There is no
Python/numpy implementation of any transform here — if the shared library is
missing the import fails loudly, and every transform needs a live gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmelonix_amd.so")
_DEFAULT_LIB_PATH = LIB_PATH  # (tools that A/B another build point LIB_PATH elsewhere: no identity check there)

MX_OK = 0
MX_ERR_INVALID, MX_ERR_DEVICE, MX_ERR_NOMEM, MX_ERR_IO = -1, -2, -3, -4
MX_AUDIO_PAD = 32768


class MxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"melonix_amd error {code}: {msg}")
        self.code = code


class Pitch(C.Structure):
    _fields_ = [("bin", C.c_int32), ("mag", C.c_float)]


class Marker(C.Structure):
    _fields_ = [("sample", C.c_int32), ("note", C.c_double), ("dTime", C.c_double), ("pitchBend", C.c_double)]


class Step(C.Structure):
    _fields_ = [("cursor", C.c_double), ("grain_start", C.c_int32), ("grain_len", C.c_int32), ("rate", C.c_float),
                ("next_first", C.c_float), ("sz", C.c_int32), ("_pad", C.c_int32), ("out_offset", C.c_int64)]


class F0(C.Structure):
    _fields_ = [("tau", C.c_int32), ("period", C.c_float), ("aperiodicity", C.c_float), ("rms", C.c_float)]


class F0Cand(C.Structure):
    _fields_ = [("tau", C.c_int32), ("period", C.c_float), ("aperiodicity", C.c_float), ("cents", C.c_int32)]


class F0DecodeParams(C.Structure):
    _fields_ = [("unvoiced_cost", C.c_float), ("jump_cost", C.c_float), ("switch_cost", C.c_float),
                ("max_jump_cents", C.c_int32)]


class NoteParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("rms_floor", C.c_float), ("max_jump", C.c_double), ("max_dev", C.c_double),
                ("min_frames", C.c_int32)]


class Note(C.Structure):
    _fields_ = [("start_sample", C.c_int32), ("end_sample", C.c_int32), ("first_frame", C.c_int32), ("frames", C.c_int32),
                ("note", C.c_double), ("aperiodicity", C.c_float), ("spread", C.c_float)]


class PsolaParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("rms_floor", C.c_float), ("unvoiced_period", C.c_float)]


class PsolaGrain(C.Structure):
    _fields_ = [("out_lo", C.c_int32), ("out_hi", C.c_int32), ("src_off", C.c_int32), ("src_frac", C.c_float),
                ("centre", C.c_int32), ("centre_frac", C.c_float), ("inv_half", C.c_float), ("mark", C.c_int32)]


class FormantPoint(C.Structure):
    _fields_ = [("sample", C.c_int32), ("semitones", C.c_float)]


class PsolaFGrain(C.Structure):
    _fields_ = [("out_lo", C.c_int32), ("out_hi", C.c_int32), ("src_idx", C.c_int32), ("src_q", C.c_uint32),
                ("centre", C.c_int32), ("centre_frac", C.c_float), ("inv_half", C.c_float), ("step", C.c_uint32)]


class OnsetFluxParams(C.Structure):
    _fields_ = [("compress", C.c_float), ("lag", C.c_int32), ("fmin", C.c_float), ("fmax", C.c_float)]


class OnsetPickParams(C.Structure):
    _fields_ = [("pre_max", C.c_int32), ("post_max", C.c_int32), ("pre_avg", C.c_int32), ("post_avg", C.c_int32),
                ("wait", C.c_int32), ("ratio", C.c_double), ("delta", C.c_double)]


class Onset(C.Structure):
    _fields_ = [("sample", C.c_int32), ("frame", C.c_int32), ("strength", C.c_float), ("margin", C.c_float)]


class TimingParams(C.Structure):
    _fields_ = [("bpm", C.c_double), ("division", C.c_int32), ("offset", C.c_double), ("strength", C.c_double),
                ("max_shift", C.c_double), ("max_stretch", C.c_double)]


class CombJob(C.Structure):
    _fields_ = [("first", C.c_int32), ("frames", C.c_int32), ("period_q16", C.c_uint32)]


class Comb(C.Structure):
    _fields_ = [("score", C.c_float), ("phase", C.c_int32), ("prev", C.c_float), ("next", C.c_float)]


class TempoParams(C.Structure):
    _fields_ = [("bpm_min", C.c_double), ("bpm_max", C.c_double), ("per_octave", C.c_int32), ("smooth", C.c_int32),
                ("window_frames", C.c_int32), ("stride_frames", C.c_int32), ("prior_bpm", C.c_double),
                ("prior_octaves", C.c_double), ("lock_ratio", C.c_double)]


class Tempo(C.Structure):
    _fields_ = [("bpm", C.c_double), ("offset", C.c_double), ("score", C.c_float), ("clarity", C.c_float),
                ("locked_frames", C.c_int64), ("levels", C.c_int32)]


class TempoWindow(C.Structure):
    _fields_ = [("first_frame", C.c_int32), ("frames", C.c_int32), ("bpm", C.c_float), ("score", C.c_float)]


class SibFeat(C.Structure):
    _fields_ = [("low", C.c_float), ("high", C.c_float), ("centroid", C.c_float), ("zero_crossings", C.c_int32)]


class SibFeatureParams(C.Structure):
    _fields_ = [("split_hz", C.c_float)]


class SibilantParams(C.Structure):
    _fields_ = [("share_on", C.c_double), ("share_off", C.c_double), ("level_floor", C.c_double), ("zc_min", C.c_int32),
                ("merge_gap", C.c_int32), ("min_frames", C.c_int32)]


class Sibilant(C.Structure):
    _fields_ = [("start_sample", C.c_int32), ("end_sample", C.c_int32), ("first_frame", C.c_int32), ("frames", C.c_int32),
                ("share", C.c_float), ("level", C.c_float)]


class GainPoint(C.Structure):
    _fields_ = [("sample", C.c_int32), ("amp", C.c_float)]


class ChromaParams(C.Structure):
    _fields_ = [("fmin", C.c_float), ("fmax", C.c_float), ("floor", C.c_float), ("rel", C.c_float)]


class ChromaJob(C.Structure):
    _fields_ = [("first_frame", C.c_int64), ("frames", C.c_int64)]


class Key(C.Structure):
    _fields_ = [("tonic", C.c_int32), ("mode", C.c_int32), ("scale_mask", C.c_int32), ("reserved", C.c_int32),
                ("tuning_cents", C.c_double), ("tuning_confidence", C.c_double), ("correlation", C.c_double),
                ("clarity", C.c_double)]


class KeyWindow(C.Structure):
    _fields_ = [("first_frame", C.c_int32), ("frames", C.c_int32), ("key", Key)]


class ContourSpan(C.Structure):
    _fields_ = [("first", C.c_int32), ("frames", C.c_int32)]


class ContourParams(C.Structure):
    _fields_ = [("half_width", C.c_int32), ("lag_min", C.c_int32), ("lag_max", C.c_int32)]


class ContourRec(C.Structure):
    _fields_ = [("smooth", C.c_int32), ("vib", C.c_int32)]


class ContourStat(C.Structure):
    _fields_ = [("sum_smooth", C.c_int64), ("min_smooth", C.c_int32), ("max_smooth", C.c_int32), ("r0", C.c_int64),
                ("lag", C.c_int32), ("reserved", C.c_int32), ("r_lag", C.c_int64)]


class Vibrato(C.Structure):
    _fields_ = [("rate_hz", C.c_double), ("extent_cents", C.c_double), ("strength", C.c_double), ("drift_cents", C.c_double)]


class BendParams(C.Structure):
    _fields_ = [("drift_amount", C.c_double), ("vibrato_scale", C.c_double), ("glide_frames", C.c_int32)]


class LoudStep(C.Structure):
    _fields_ = [("energy", C.c_double), ("peak", C.c_float), ("samples", C.c_int32)]


class Loudness(C.Structure):
    _fields_ = [("integrated", C.c_double), ("momentary_max", C.c_double), ("shortterm_max", C.c_double), ("peak", C.c_float),
                ("blocks", C.c_int64), ("passed_abs", C.c_int64), ("passed_rel", C.c_int64), ("bad_blocks", C.c_int64)]


class LevelParams(C.Structure):
    _fields_ = [("raise", C.c_double), ("lower", C.c_double), ("max_db", C.c_double)]


class TpStep(C.Structure):
    _fields_ = [("true_peak", C.c_float), ("sample_peak", C.c_float)]


class LimitParams(C.Structure):
    _fields_ = [("ceiling_amp", C.c_float), ("lookahead", C.c_int32)]


class LoudnessRange(C.Structure):
    _fields_ = [("lra", C.c_double), ("low_lufs", C.c_double), ("high_lufs", C.c_double), ("values", C.c_int64),
                ("gated", C.c_int64), ("bad", C.c_int64)]


class ResamplePlan(C.Structure):
    _fields_ = [("L", C.c_int32), ("M", C.c_int32), ("taps", C.c_int32), ("half", C.c_int32)]


class DenoiseParams(C.Structure):
    _fields_ = [("reduction_db", C.c_float), ("sensitivity_db", C.c_float)]


class CompressParams(C.Structure):
    _fields_ = [("threshold_db", C.c_float), ("ratio", C.c_float), ("knee_db", C.c_float), ("attack_ms", C.c_float),
                ("release_ms", C.c_float), ("lookahead_ms", C.c_float), ("makeup_amp", C.c_float)]


class CompressPlan(C.Structure):
    _fields_ = [("D", C.c_int32), ("K", C.c_int32), ("c_att", C.c_int32), ("c_rel", C.c_int32), ("W", C.c_int32), ("Gc", C.c_int32)]


# the C type of every record class, in the order of include/melonix_amd.h.  A record is declared here once, as its class: the
# field names are the header's, the numpy dtypes below are derived from the classes, and tests/test_abi.py compares every
# class's size, field offsets and field sizes with what a C compiler makes of the header.  (mx_chroma_rec has no class: a
# chroma record is a row of CHROMA_COLS floats.)
RECORDS = {
    "mx_pitch": Pitch, "mx_marker": Marker, "mx_step": Step, "mx_f0": F0, "mx_f0_cand": F0Cand,
    "mx_f0_decode_params": F0DecodeParams, "mx_note_params": NoteParams, "mx_note": Note, "mx_psola_params": PsolaParams,
    "mx_psola_grain": PsolaGrain, "mx_formant_point": FormantPoint, "mx_psola_fgrain": PsolaFGrain,
    "mx_onset_flux_params": OnsetFluxParams, "mx_onset_pick_params": OnsetPickParams, "mx_onset": Onset,
    "mx_timing_params": TimingParams, "mx_comb_job": CombJob, "mx_comb": Comb, "mx_tempo_params": TempoParams, "mx_tempo": Tempo,
    "mx_tempo_window": TempoWindow, "mx_sib_feat": SibFeat, "mx_sib_feature_params": SibFeatureParams,
    "mx_sibilant_params": SibilantParams, "mx_sibilant": Sibilant, "mx_gain_point": GainPoint, "mx_chroma_rec": None,
    "mx_chroma_params": ChromaParams, "mx_chroma_job": ChromaJob, "mx_key": Key, "mx_key_window": KeyWindow,
    "mx_contour_span": ContourSpan, "mx_contour_params": ContourParams, "mx_contour_rec": ContourRec,
    "mx_contour_stat": ContourStat, "mx_vibrato": Vibrato, "mx_bend_params": BendParams, "mx_loud_step": LoudStep,
    "mx_loudness": Loudness, "mx_level_params": LevelParams, "mx_tp_step": TpStep, "mx_limit_params": LimitParams,
    "mx_loudness_range_result": LoudnessRange, "mx_resample_plan": ResamplePlan,
    "mx_denoise_params": DenoiseParams, "mx_compress_params": CompressParams, "mx_compress_plan": CompressPlan,
}

PITCH_DTYPE, STEP_DTYPE, MARKER_DTYPE = np.dtype(Pitch), np.dtype(Step), np.dtype(Marker)
F0_DTYPE, F0_CAND_DTYPE, NOTE_DTYPE = np.dtype(F0), np.dtype(F0Cand), np.dtype(Note)
F0_CANDS = 4
PSOLA_GRAIN_DTYPE, FORMANT_POINT_DTYPE, PSOLA_FGRAIN_DTYPE = np.dtype(PsolaGrain), np.dtype(FormantPoint), np.dtype(PsolaFGrain)
ONSET_DTYPE = np.dtype(Onset)
COMB_JOB_DTYPE, COMB_DTYPE, TEMPO_WINDOW_DTYPE = np.dtype(CombJob), np.dtype(Comb), np.dtype(TempoWindow)
SIB_FEAT_DTYPE, SIBILANT_DTYPE, GAIN_POINT_DTYPE = np.dtype(SibFeat), np.dtype(Sibilant), np.dtype(GainPoint)
CHROMA_COLS = 40  # a chroma record: 36 profile bins, the tuning phasor, the summed weight, the number of peaks
CHROMA_JOB_DTYPE, KEY_DTYPE, KEY_WINDOW_DTYPE = np.dtype(ChromaJob), np.dtype(Key), np.dtype(KeyWindow)
CONTOUR_NONE = -2 ** 31  # MX_CONTOUR_NONE: an unvoiced frame's cents, the smooth value outside every span
CONTOUR_SPAN_DTYPE, CONTOUR_REC_DTYPE, CONTOUR_STAT_DTYPE = np.dtype(ContourSpan), np.dtype(ContourRec), np.dtype(ContourStat)
LOUD_STEP_DTYPE = np.dtype(LoudStep)
LOUD_GROUP_STEPS = 10  # G: steps per group, the unit mx_loudness_steps is asked in
TP_STEP_DTYPE = np.dtype(TpStep)
DENOISE_BINS = 513  # MX_DENOISE_BINS: the values of a noise print, the floats of a power row
COMPRESS_CURVE = 2049  # MX_COMPRESS_CURVE: the Q30 targets of a compressor's curve

# name -> (restype, argtypes); kept in the order of include/melonix_amd.h
_vp, _i, _i64, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
_pi32 = C.POINTER(C.c_int32)
SIGNATURES = {
    "mx_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "mx_ctx_destroy": (None, [_vp]),
    "mx_ctx_set_stream": (_i, [_vp, _vp]),
    "mx_ctx_use_own_stream": (_i, [_vp]),
    "mx_ctx_synchronize": (_i, [_vp]),
    "mx_ctx_release_scratch": (_i, [_vp]),
    "mx_ctx_set_frames_per_block": (_i, [_vp, _i]),
    "mx_stft_run_length": (_i, [_i, _i, _i64]),
    "mx_pinned_alloc": (_i, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "mx_pinned_free": (None, [_vp, _vp]),
    "mx_last_error": (C.c_char_p, []),
    "mx_version": (C.c_char_p, []),
    "mx_audio_upload": (_i, [_vp, _vp, _i64, C.POINTER(_vp)]),
    "mx_audio_wrap_device": (_i, [_vp, _vp, _i64, C.POINTER(_vp)]),
    "mx_audio_length": (_i64, [_vp]),
    "mx_audio_free": (_i, [_vp, _vp]),
    "mx_pitch_band": (None, [_i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "mx_bin_note": (_d, [_i, _i, _i]),
    "mx_note_bin": (_d, [_d, _i, _i]),
    "mx_stft_ranges": (_i, [_vp, _vp, _i, _vp, _i64, _i, _i, _vp, _vp]),
    "mx_stft_hop": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _vp, _vp]),
    "mx_stft_hop_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _i, _vp, _vp]),
    "mx_stft_ranges_dev": (_i, [_vp, _vp, _i, _vp, _i64, _i, _i, _vp, _vp]),
    "mx_stft_ranges_rgb": (_i, [_vp, _vp, _i, _vp, _i64, _f, _vp]),
    "mx_stft_ranges_rgb_mags": (_i, [_vp, _vp, _i, _vp, _i64, _f, _vp, _vp]),
    "mx_stft_ranges_rgb_dev": (_i, [_vp, _vp, _i, _vp, _i64, _f, _vp, _vp]),
    "mx_colormap_dev": (_i, [_vp, _vp, _i64, _f, _vp]),
    "mx_stft_ranges_keep": (_i, [_vp, _vp, _i, _vp, _i64, _f, _vp, _vp, C.POINTER(_vp)]),
    "mx_rows_count": (_i64, [_vp]),
    "mx_rows_free": (None, [_vp, _vp]),
    "mx_rows_fetch": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "mx_rows_colormap": (_i, [_vp, _vp, _i64, _i64, _f, _vp]),
    "mx_frame_count": (_i64, [_i64, _i]),
    "mx_sample2time": (_d, [_vp, _i, _i, _i]),
    "mx_time2sample": (_i, [_vp, _i, _i, _d]),
    "mx_duration": (_d, [_vp, _i, _i, _i64]),
    "mx_time2pitchbend": (_f, [_vp, _i, _i, _i64, _d]),
    "mx_column_range": (None, [_vp, _i, _i, _d, _i, _d, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mx_grains": (_i, [_vp, _i64, C.POINTER(_pi32), C.POINTER(_pi32), C.POINTER(_i64)]),
    "mx_grains_dev": (_i, [_vp, _vp, C.POINTER(_pi32), C.POINTER(_pi32), C.POINTER(_i64)]),
    "mx_grain_table_dev": (_i, [_vp, _vp, C.POINTER(_pi32), C.POINTER(_pi32), C.POINTER(C.POINTER(C.c_float)), C.POINTER(_i64)]),
    "mx_schedule_build": (_i, [_vp, _i64, _i, _vp, _vp, _i64, _vp, _i, C.POINTER(C.POINTER(Step)),
                               C.POINTER(_i64), C.POINTER(_i64)]),
    "mx_schedule_build_from": (_i, [_vp, _i64, _i, _vp, _vp, _i64, _vp, _i, _d, _i64, C.POINTER(C.POINTER(Step)),
                                    C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_d)]),
    "mx_schedule_build_table": (_i, [_i64, _i, _vp, _vp, _vp, _i64, _vp, _i, _d, _i64, C.POINTER(C.POINTER(Step)),
                                     C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_d)]),
    "mx_free": (None, [_vp]),
    "mx_resynth": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_resynth_dev": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_resynth_to_wav": (_i, [_vp, _vp, _vp, _i64, _i64, C.c_char_p, _i, _i]),
    "mx_export_wav": (_i, [_vp, _vp, _i64, _i, _vp, _i, C.c_char_p, _i]),
    "mx_pv_set_chunk_frames": (_i, [_vp, _i64]),
    "mx_pv_set_arena_budget": (_i, [_vp, _i64]),
    "mx_pv_arena_budget": (_i64, [_vp]),
    "mx_pv_arena_bytes": (_i64, [_vp]),
    "mx_pv_last_chunks": (_i64, [_vp]),
    "mx_pv_pitch_shift": (_i, [_vp, _vp, _d, _vp, _vp]),
    "mx_pv_pitch_shift_dev": (_i, [_vp, _vp, _d, _vp, _vp]),
    "mx_pv_render_length": (_i64, [_i64, _i, _vp, _i]),
    "mx_pv_plan": (_i, [_i64, _i, _vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                        C.POINTER(_i64), C.POINTER(_i64)]),
    "mx_pv_render": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "mx_pv_render_dev": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "mx_pv_shard_frames": (_i, [_i64, _d, _i, _i, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "mx_pv_shard_analyze": (_i, [_vp, _vp, _d, _i, _i, _vp, _vp]),
    "mx_pv_shard_synthesize": (_i, [_vp, _vp, _vp, _vp]),
    "mx_pv_shard_finish": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mx_pv_shard_analyze_dev": (_i, [_vp, _vp, _d, _i, _i, _vp]),
    "mx_pv_shard_synthesize_dev": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mx_pv_shard_finish_dev": (_i, [_vp, _vp]),
    "mx_minmax_pyramid": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "mx_minmax_pyramid_dev": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "mx_minmax_range": (None, [_vp, _i64, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f)]),
    "mx_f0_track": (_i, [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp]),
    "mx_f0_track_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp]),
    "mx_f0_candidates_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp, _vp]),
    "mx_f0_candidates": (_i, [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, _vp, _vp]),
    "mx_f0_decode_params_default": (None, [C.POINTER(F0DecodeParams)]),
    "mx_f0_decode_dev": (_i, [_vp, _vp, _vp, _i64, C.POINTER(F0DecodeParams), _vp, _vp]),
    "mx_f0_decode": (_i, [_vp, _vp, _vp, _i64, C.POINTER(F0DecodeParams), _vp, _vp]),
    "mx_f0_track_decoded": (_i, [_vp, _vp, _i, _i, _i64, _i64, _f, _f, _f, C.POINTER(F0DecodeParams), _vp]),
    "mx_f0_decode_set_chunk": (_i, [_vp, _i64]),
    "mx_note_params_default": (None, [C.POINTER(NoteParams)]),
    "mx_detect_notes": (_i, [_vp, _i64, _i, _i, _i64, C.POINTER(NoteParams), C.POINTER(C.POINTER(Note)), C.POINTER(_i64)]),
    "mx_correction_markers": (_i, [_vp, _i64, _d, _i, _vp]),
    "mx_psola_params_default": (None, [C.POINTER(PsolaParams)]),
    "mx_psola_plan": (_i, [_i64, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, C.POINTER(_vp), C.POINTER(_i64),
                           C.POINTER(_i64)]),
    "mx_psola_synth_dev": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_psola_synth": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_psola_render": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _vp]),
    "mx_psola_render_dev": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _vp]),
    "mx_psola_plan_formant": (_i, [_i64, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, C.POINTER(_vp),
                                   C.POINTER(_i64), C.POINTER(_i64)]),
    "mx_psola_synth_formant_dev": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_psola_synth_formant": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mx_psola_render_formant": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, _vp, _vp]),
    "mx_psola_render_formant_dev": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, _vp, _vp]),
    "mx_onset_flux_params_default": (None, [C.POINTER(OnsetFluxParams)]),
    "mx_onset_flux_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(OnsetFluxParams), _vp]),
    "mx_onset_flux": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(OnsetFluxParams), _vp]),
    "mx_onset_pick_params_default": (None, [C.POINTER(OnsetPickParams)]),
    "mx_onset_pick": (_i, [_vp, _i64, _i, _i64, C.POINTER(OnsetPickParams), C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_onsets_detect": (_i, [_vp, _vp, _i, _i, C.POINTER(OnsetFluxParams), C.POINTER(OnsetPickParams), C.POINTER(_vp),
                              C.POINTER(_i64)]),
    "mx_timing_params_default": (None, [C.POINTER(TimingParams)]),
    "mx_timing_markers": (_i, [_vp, _i64, _i64, _i, C.POINTER(TimingParams), _vp, _i, C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_tempo_params_default": (None, [C.POINTER(TempoParams)]),
    "mx_tempo_smooth_dev": (_i, [_vp, _vp, _i64, _i, _vp]),
    "mx_tempo_smooth": (_i, [_vp, _vp, _i64, _i, _vp]),
    "mx_tempo_comb_dev": (_i, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "mx_tempo_comb": (_i, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "mx_tempo_from_flux": (_i, [_vp, _vp, _i64, _i, _i, _i64, C.POINTER(TempoParams), C.POINTER(Tempo), C.POINTER(_vp),
                                C.POINTER(_i64)]),
    "mx_tempo_detect": (_i, [_vp, _vp, _i, _i, C.POINTER(OnsetFluxParams), C.POINTER(TempoParams), C.POINTER(Tempo),
                             C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_sib_feature_params_default": (None, [C.POINTER(SibFeatureParams)]),
    "mx_sib_features_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(SibFeatureParams), _vp]),
    "mx_sib_features": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(SibFeatureParams), _vp]),
    "mx_sibilant_params_default": (None, [C.POINTER(SibilantParams)]),
    "mx_sibilants": (_i, [_vp, _i64, _i, _i64, C.POINTER(SibilantParams), C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_sibilants_detect": (_i, [_vp, _vp, _i, _i, C.POINTER(SibFeatureParams), C.POINTER(SibilantParams), C.POINTER(_vp),
                                 C.POINTER(_i64)]),
    "mx_formant_protect": (_i, [_vp, _i, _vp, _i64, C.c_int32, _i64, C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_audio_gain": (_i, [_vp, _vp, _vp, _i64, C.POINTER(_vp)]),
    "mx_audio_gain_dev": (_i, [_vp, _vp, _vp, _i64, C.POINTER(_vp)]),
    "mx_audio_download": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "mx_sibilant_gain_points": (_i, [_vp, _i64, _d, C.c_int32, _i64, C.POINTER(_vp), C.POINTER(_i64)]),
    "mx_chroma_params_default": (None, [C.POINTER(ChromaParams)]),
    "mx_chroma_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(ChromaParams), _vp]),
    "mx_chroma": (_i, [_vp, _vp, _i, _i, _i64, _i64, C.POINTER(ChromaParams), _vp]),
    "mx_chroma_sum_dev": (_i, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "mx_chroma_sum": (_i, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "mx_key_from_chroma": (_i, [_vp, C.POINTER(Key)]),
    "mx_key_from_notes": (_i, [_vp, _i64, C.POINTER(Key)]),
    "mx_key_detect": (_i, [_vp, _vp, _i, _i, C.POINTER(ChromaParams), _i64, _i64, C.POINTER(Key), C.POINTER(_vp),
                           C.POINTER(_i64)]),
    "mx_correction_markers_tuned": (_i, [_vp, _i64, _d, _i, _d, _vp]),
    "mx_contour_params_default": (_i, [_i, _i, C.POINTER(ContourParams)]),
    "mx_contour_cents_dev": (_i, [_vp, _vp, _i64, _i, _f, _f, _vp]),
    "mx_contour_cents": (_i, [_vp, _vp, _i64, _i, _f, _f, _vp]),
    "mx_contour_split_dev": (_i, [_vp, _vp, _i64, _vp, _i64, C.POINTER(ContourParams), _vp, _vp]),
    "mx_contour_split": (_i, [_vp, _vp, _i64, _vp, _i64, C.POINTER(ContourParams), _vp, _vp]),
    "mx_contour_spans": (_i, [_vp, _i64, _i64, _vp]),
    "mx_contour_vibrato": (_i, [_vp, C.c_int32, _i, _i, C.POINTER(Vibrato)]),
    "mx_bend_params_default": (None, [C.POINTER(BendParams)]),
    "mx_contour_bend": (_i, [_vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(BendParams), _vp]),
    "mx_pitch_contour": (_i, [_vp, _vp, _i64, _i, _i, _i64, _vp, _i64, _f, _f, C.POINTER(ContourParams), _vp, _vp]),
    "mx_psola_plan_bend": (_i, [_i64, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, C.POINTER(_vp), C.POINTER(_i64),
                                C.POINTER(_i64)]),
    "mx_psola_plan_formant_bend": (_i, [_i64, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, _vp, C.POINTER(_vp),
                                        C.POINTER(_i64), C.POINTER(_i64)]),
    "mx_psola_render_bend": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "mx_psola_render_bend_dev": (_i, [_vp, _vp, _i, _i, _vp, _i64, C.POINTER(PsolaParams), _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "mx_loudness_step_count": (_i64, [_i64, _i]),
    "mx_loudness_coeffs": (_i, [_i, _vp]),
    "mx_loudness_steps_dev": (_i, [_vp, _vp, _i, _i64, _i64, _vp]),
    "mx_loudness_steps": (_i, [_vp, _vp, _i, _i64, _i64, _vp]),
    "mx_loudness_curve": (_i, [_vp, _i64, _i, _i, _vp]),
    "mx_loudness_integrated": (_i, [_vp, _i64, _i, C.POINTER(Loudness)]),
    "mx_loudness_measure": (_i, [_vp, _vp, _i, C.POINTER(Loudness)]),
    "mx_note_loudness": (_i, [_vp, _i64, _i, _vp, _i64, _vp]),
    "mx_level_params_default": (None, [C.POINTER(LevelParams)]),
    "mx_level_gain_points": (_i, [_vp, _i64, _vp, C.POINTER(LevelParams), _vp, C.POINTER(_d)]),
    "mx_normalize_gain": (_i, [C.POINTER(Loudness), _d, _d, C.POINTER(_f)]),
    "mx_true_peak_oversampling": (_i, [_i]),
    "mx_true_peak_taps": (_i, [_vp]),
    "mx_true_peak_steps_dev": (_i, [_vp, _vp, _i, _i64, _i64, _vp]),
    "mx_true_peak_steps": (_i, [_vp, _vp, _i, _i64, _i64, _vp]),
    "mx_true_peak_measure": (_i, [_vp, _vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    "mx_limit_params_default": (_i, [_i, C.POINTER(LimitParams)]),
    "mx_audio_limit_dev": (_i, [_vp, _vp, _i, C.POINTER(LimitParams), C.POINTER(_vp), _vp]),
    "mx_audio_limit": (_i, [_vp, _vp, _i, C.POINTER(LimitParams), C.POINTER(_vp), _vp]),
    "mx_loudness_range": (_i, [_vp, _i64, _i, C.POINTER(LoudnessRange)]),
    "mx_normalize_gain_tp": (_i, [C.POINTER(Loudness), _f, _d, _d, C.POINTER(_f)]),
    "mx_resample_plan_for": (_i, [_i, _i, C.POINTER(ResamplePlan)]),
    "mx_resample_length": (_i64, [_i64, _i, _i]),
    "mx_resample_taps": (_i, [_i, _i, _vp]),
    "mx_resample_dev": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp]),
    "mx_resample": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp]),
    "mx_audio_resample": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "mx_denoise_frames": (_i64, [_i64]),
    "mx_denoise_factors": (_i, [C.POINTER(DenoiseParams), _vp]),
    "mx_noise_rows_dev": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "mx_noise_print_rows": (_i, [_vp, _i64, _vp]),
    "mx_noise_print_dev": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "mx_noise_print": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "mx_denoise_dev": (_i, [_vp, _vp, _vp, C.POINTER(DenoiseParams), _i64, _i64, _vp, _vp]),
    "mx_denoise": (_i, [_vp, _vp, _vp, C.POINTER(DenoiseParams), _i64, _i64, _vp, _vp]),
    "mx_audio_denoise": (_i, [_vp, _vp, _vp, C.POINTER(DenoiseParams), C.POINTER(_vp)]),
    "mx_compress_params_default": (_i, [_i, C.POINTER(CompressParams)]),
    "mx_compress_plan_for": (_i, [_i, C.POINTER(CompressParams), C.POINTER(CompressPlan)]),
    "mx_compress_curve": (_i, [C.POINTER(CompressParams), _vp]),
    "mx_compress_steps": (_i64, [_i64, _i]),
    "mx_compress_peaks_dev": (_i, [_vp, _vp, _i, _i64, _i64, _vp]),
    "mx_compress_gain_dev": (_i, [_vp, _vp, _i, C.POINTER(CompressParams), _i64, _i64, _vp]),
    "mx_compress_gain": (_i, [_vp, _vp, _i, C.POINTER(CompressParams), _i64, _i64, _vp]),
    "mx_compress_dev": (_i, [_vp, _vp, _i, C.POINTER(CompressParams), _i64, _i64, _vp, _vp]),
    "mx_compress": (_i, [_vp, _vp, _i, C.POINTER(CompressParams), _i64, _i64, _vp, _vp]),
    "mx_audio_compress": (_i, [_vp, _vp, _i, C.POINTER(CompressParams), C.POINTER(_vp)]),
    "mx_save_wav": (_i, [C.c_char_p, _vp, _i64, _i, _i]),
}

_LIB = None


def lib():
    """Loads libmelonix_amd.so.  Raises if it has not been built — there is no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m melonix_amd.build` (hipcc, gfx950). "
                "melonix_amd has no CPU/Python compute path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        check_identity(L.mx_version().decode(), LIB_PATH)
        _LIB = L
    return _LIB


def library_src_sha(version: str) -> str:
    """The `src:<12 hex>` digits of an mx_version() string ('' if it carries none)."""
    tail = version.rsplit("src:", 1)
    return tail[1].strip() if len(tail) == 2 else ""


def check_identity(version: str, path: str) -> None:
    """A library that was not built from the sources beside it is refused: the GPU box runs whatever .so travelled with the
    snapshot, and a kernel edit without a rebuild would otherwise be measured (and graded) as the old kernel.
    MELONIX_ALLOW_STALE=1 loads it anyway (A/B runs against an older build: tools/ab_variant.sh, MX_AB_LIB)."""
    from . import build as _build

    if os.environ.get("MELONIX_ALLOW_STALE") == "1" or os.path.abspath(path) != os.path.abspath(_DEFAULT_LIB_PATH):
        return
    have = library_src_sha(version)
    try:
        want = _build.source_sha()
    except OSError as exc:
        # a deployment that carries the library without its sources (a wheel, a box that received only the .so): nothing to compare
        # with — fall back on the digits build() left beside the library's objects, else say what is missing
        want = None
        sha_file = os.path.join(_HERE, "build", "src_sha.txt")
        if os.path.exists(sha_file):
            with open(sha_file) as fh:
                want = fh.read().strip()
        if not want:
            raise ImportError(
                f"{path}: cannot check that the library was built from this tree ({exc}); the sources under melonix_amd/csrc and "
                "include/ are needed for that — ship them with the library, or set MELONIX_ALLOW_STALE=1 to load it unchecked.") from exc
    if have != want:
        raise ImportError(
            f"{path} was built from other sources than the ones beside it (library src:{have or '?'}, tree src:{want}): "
            "rebuild with `python -m melonix_amd.build`, or set MELONIX_ALLOW_STALE=1 to load it anyway.")


def check(rc: int) -> None:
    if rc != MX_OK:
        raise MxError(rc, (lib().mx_last_error() or b"").decode(errors="replace"))


def records(items, dtype):
    """Tuples, or an array of `dtype` -> a contiguous array of `dtype`; each value is cast to its field's type.  The one
    conversion from tuples to records."""
    if isinstance(items, np.ndarray) and items.dtype == dtype:
        return np.ascontiguousarray(items)
    out = np.zeros(len(items), dtype=dtype)
    for i, it in enumerate(items):
        out[i] = tuple(it)
    return out


def markers_array(markers):
    """(sample, note, dTime, pitchBend) tuples -> a ctypes array of at least one Marker (never a null pointer), padding zero."""
    rec = records(markers, MARKER_DTYPE)
    arr = (Marker * max(1, len(rec)))()
    C.memmove(arr, rec.ctypes.data, rec.nbytes)
    return arr
