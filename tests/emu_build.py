"""The CPU emulations of tests/emu as the host tests build them, and a kernel unit's resource usage as the build compiles it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "melonix_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
FLAGS = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall"]  # as the library's host units: every product and sum rounds as written


def _paths(names):
    """emulation sources by their name in tests/emu, the library's sources and headers by their name in csrc"""
    return [os.path.join(EMU if os.path.exists(os.path.join(EMU, n)) else CSRC, n) for n in names]


def shared_object(name: str, sources, headers=()) -> str:
    """tests/emu/lib<name>.so from `sources`, rebuilt where one of them, a header of `headers` or the public header is newer;
    returns its path."""
    so = os.path.join(EMU, f"lib{name}.so")
    src = _paths(sources)
    deps = src + _paths(headers) + [os.path.join(ROOT, "include", "melonix_amd.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(FLAGS + ["-fPIC", "-shared"] + src + ["-o", so])
    return so


def run_sanitized(tmp_path, name: str, sources, define: str, opt=("-O2", "-g")) -> str:
    """`sources` with -D<define>, the stand-alone main of an emulation, under AddressSanitizer and UBSan: built into tmp_path
    (`opt`: in place of -O2 -g), run; returns its standard output (the program must end with status 0)."""
    exe = str(tmp_path / name)
    flags = [f for f in FLAGS if f != "-O2"] + list(opt)
    subprocess.check_call(flags + ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                   "-D" + define] + _paths(sources) + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    return out.stdout


def resource_usage(unit: str):
    """(kernel names, scratch bytes per lane, VGPRs, LDS bytes per block) of a unit of build.UNITS, compiled as the build compiles
    it: one entry per kernel, in the compiler's order."""
    from melonix_amd import build

    out = subprocess.run(build.unit_command(unit) + ["-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch, vgprs, lds = ([int(x) for x in re.findall(pat, out.stderr)] for pat in
                           (r"ScratchSize \[bytes/lane\]: (\d+)", r"\bVGPRs: (\d+)", r"LDS Size \[bytes/block\]: (\d+)"))
    assert len(names) == len(scratch) == len(vgprs) == len(lds), unit
    return names, scratch, vgprs, lds
