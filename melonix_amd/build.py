"""Builds melonix_amd/lib/libmelonix_amd.so (gfx950 code objects + C-ABI) in-tree.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the CPU-only
container as well as on the MI355X box.  Re-builds only when a source is newer
than the library.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libmelonix_amd.so")
OBJDIR = os.path.join(HERE, "build")

ARCH = "gfx950"
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = os.environ.get("CXX") or shutil.which("g++") or "g++"

COMMON = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
# (source, compiler, extra flags)
UNITS = [
    # the butterflies are hand-written packed arithmetic (pk_math.h: inline v_pk_fma/add/mul_f32 with op_sel / neg
    # modifiers); the SLP vectoriser's own v_pk_* forms on the remaining scalar code cost register-pairing moves, so
    # it stays off.  -ffp-contract=off: the core spells out every FMA, so all kernel instantiations round alike
    ("stft_kernels.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    # bit-exact PCM: no FMA contraction in the resampler
    ("resynth_kernels.hip", "hip", ["-ffp-contract=off"]),
    ("colormap_kernel.hip", "hip", ["-ffp-contract=off"]),
    ("grain_chain.hip", "hip", []),
    # build-defined phase vocoder, a unit per stage (pv_common.h): shares the FFT passes of stft_core.h (explicit FMAs)
    ("pv_analysis.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    ("pv_lock.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    ("pv_synthesis.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    # build-defined YIN f0 tracker: three transforms per frame on the same FFT passes
    ("f0_kernels.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    # build-defined Viterbi decode over the YIN candidate ladder: integer min-plus scans, no floating point beyond q()
    ("f0_decode.hip", "hip", ["-ffp-contract=off"]),
    # build-defined PSOLA overlap-add: the resampler's interpolation form, products rounded before the sums
    ("psola_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined onset strength: a 1024-point transform of its own on one wavefront (onset_core.h), every rounding as written
    ("onset_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined tempo estimation: f32 products rounded before a binary64 running sum (tempo_core.h), bit for bit the host's
    ("tempo_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined sibilant features: the onset transform with another tail (sibilant_core.h), every rounding as written
    ("sibilant_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined source gain: a binary64 product rounded before the sum (gain_core.h), bit for bit numpy's
    ("gain_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined chroma records: the f0 tracker's walk, one windowed transform per frame, another tail (chroma_core.h), every
    # rounding as written; and their binary64 window sums, bit for bit the host's
    ("chroma_kernels.hip", "hip", ["-fno-slp-vectorize", "-ffp-contract=off"]),
    # build-defined pitch-contour split: binary64 cents as written, integers after that (contour_core.h), bit for bit numpy's
    ("contour_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined loudness records: the K-weighting recurrence in binary64, every product rounded before its sum
    # (loudness_core.h), bit for bit numpy's
    ("loudness_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined true-peak records and look-ahead limiter: binary32 taps with every product rounded before its sum, integers
    # from the peak to the gain (truepeak_core.h), bit for bit numpy's
    ("truepeak_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined sample-rate conversion: binary32 taps with every product rounded before its sum, in ascending tap order
    # (resample_core.h), bit for bit numpy's
    ("resample_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined noise reduction: the onset transform forwards and, around conjugation, backwards (denoise_core.h), every
    # rounding as written, one correctly rounded division per bin
    ("denoise_kernels.hip", "hip", ["-ffp-contract=off"]),
    # build-defined dynamics compressor: integers from the table look-up to the gain, one binary64 product and quotient as
    # written (compress_core.h), bit for bit numpy's
    ("compress_kernels.hip", "hip", ["-ffp-contract=off"]),
    ("capi_ctx.cpp", "hip", []),
    ("capi_stft.cpp", "hip", []),
    ("capi_rows.cpp", "hip", []),
    ("capi_pv_arena.cpp", "hip", []),
    ("capi_pv.cpp", "hip", []),
    ("capi_pv_shard.cpp", "hip", []),
    ("capi_resynth.cpp", "hip", []),
    ("capi_pyramid.cpp", "hip", []),
    ("capi_f0.cpp", "hip", []),
    ("capi_psola.cpp", "hip", []),
    ("capi_onset.cpp", "hip", []),
    ("capi_tempo.cpp", "hip", []),
    ("capi_sibilant.cpp", "hip", []),
    ("capi_key.cpp", "hip", []),
    ("capi_contour.cpp", "hip", []),
    ("capi_loudness.cpp", "hip", []),
    ("capi_truepeak.cpp", "hip", []),
    ("capi_audio.cpp", "hip", []),
    ("capi_resample.cpp", "hip", []),
    ("capi_denoise.cpp", "hip", []),
    ("capi_compress.cpp", "hip", []),
    # pure host logic: plain g++, no contraction, no -march (SURVEY §7 "Bit-exact schedule")
    ("host_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("f0_notes.cpp", "cxx", ["-ffp-contract=off"]),
    ("psola_plan.cpp", "cxx", ["-ffp-contract=off"]),
    ("onset_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("tempo_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("sibilant_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("key_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("contour_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("loudness_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("resample_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("denoise_logic.cpp", "cxx", ["-ffp-contract=off"]),
    ("compress_logic.cpp", "cxx", ["-ffp-contract=off"]),
]
IDENTITY_UNIT = "capi_ctx.cpp"
PV_UNITS = [src for src, kind, _ in UNITS if kind == "hip" and src.startswith("pv_")]  # the phase vocoder's kernel units


def headers(csrc: str | None = None) -> list[str]:
    """Every header of the library, relative to `csrc`: what lies there (*.h, *.inc) and the public header."""
    names = [n for n in os.listdir(csrc or CSRC) if n.endswith((".h", ".inc"))]
    return sorted(names + [os.path.join("..", "..", "include", "melonix_amd.h")])


def unit_command(src: str) -> list[str]:
    """How unit `src` of UNITS is compiled — compiler, target, flags, source —, for the caller to append what it wants of
    the compile to: `-c -o x.o`, `-S --cuda-device-only -o x.s`, `-Rpass-analysis=...`.  build() and the tests that
    look at a unit's ISA or resource usage share it."""
    kind, extra = next((k, e) for s, k, e in UNITS if s == src)
    sp = os.path.join(CSRC, src)
    if kind == "hip":
        return [HIPCC, f"--offload-arch={ARCH}", "-x", "hip"] + COMMON + extra + [sp]
    return [CXX, "-O2", "-std=c++17", "-fPIC", "-Wall"] + extra + [sp]


def source_sha(csrc: str | None = None, extra_defines: list[str] | None = None) -> str:
    """Identity of a build: sha1 over every source and header the library is made of (names and bytes, in a fixed order)
    and the compile flags.  build() bakes the first 12 hex digits into the library (mx_version() ends in `src:<12 hex>`);
    melonix_amd._capi.lib() refuses a library whose digits differ from the tree it is loaded from."""
    csrc = csrc or CSRC
    h = hashlib.sha1()
    for name in sorted([u[0] for u in UNITS] + headers(csrc)):
        h.update(os.path.basename(name).encode() + b"\0")
        with open(os.path.join(csrc, name), "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(repr((ARCH, COMMON, [(u[0], u[1], u[2]) for u in UNITS], sorted(extra_defines or []))).encode())
    return h.hexdigest()[:12]


def _newest_header() -> float:
    return max(os.path.getmtime(os.path.join(CSRC, h)) for h in headers())


def build(force: bool = False, verbose: bool = False, extra_defines: list[str] | None = None) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(OBJDIR, exist_ok=True)
    hdr_t = _newest_header()
    sha = source_sha(extra_defines=extra_defines)
    sha_file = os.path.join(OBJDIR, "src_sha.txt")
    sha_was = open(sha_file).read().strip() if os.path.exists(sha_file) else ""
    objs, relink = [], force or not os.path.exists(LIB)
    for src, kind, extra in UNITS:
        sp = os.path.join(CSRC, src)
        op = os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")
        objs.append(op)
        stale = force or (not os.path.exists(op)) or os.path.getmtime(op) < max(os.path.getmtime(sp), hdr_t)
        ident = src == IDENTITY_UNIT  # the unit that carries the digits: rebuilt whenever they change
        if ident and sha != sha_was:
            stale = True
        if not stale:
            continue
        cmd = unit_command(src) + ["-c", "-o", op]
        if kind == "hip":
            cmd += (extra_defines or []) + ([f'-DMX_SRC_SHA="{sha}"'] if ident else [])
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        relink = True
    if relink or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs):
        cmd = [HIPCC, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    with open(sha_file, "w") as fh:
        fh.write(sha + "\n")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
