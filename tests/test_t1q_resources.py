"""The q-major T1 image in the ISA of the N = 4096 STFT kernels that take it (the unit compiled as the build compiles it): in the
frame loop the pass-1 scatter is sixteen ds_write_b64 off ONE address register with sixteen different immediates, and no
v_bitop3 / v_xor feeds a ds_write_b64 address — the XOR image's one swizzle per scattered point is gone.  Nothing else in the
assembly is looked for.  (Registers, scratch and LDS of the same kernels: tests/test_stft_resources.py.)"""
import re
import subprocess

import pytest

T1Q = re.compile(r"^(_ZN2mx11stft_kernelINS_4PlanILi4096ELi16EEELi(\d+)ELi(\d+)ELi3E\w*Lb1ELb1EEEvNS_8StftArgsE):")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
STORE = re.compile(r"^\s+ds_write_b64\s+(v\d+),\s*v\[\d+:\d+\](?:\s+offset:(\d+))?")


@pytest.fixture(scope="module")
def kernels():
    """name -> the lines of its body, for the instantiations whose last two template flags (ROWPICK, T1Q) are set"""
    from melonix_amd import build

    out = subprocess.run(build.unit_command("stft_kernels.hip") + ["-S", "--cuda-device-only", "-o", "-"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    found = {}
    for i, l in enumerate(lines):
        m = T1Q.match(l)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            found[(int(m.group(2)), int(m.group(3)))] = lines[i + 1:end]
    return found


def frame_loop(body):
    """the widest span between a label and a branch back to it"""
    at, best = {}, (0, 0, 0)
    for i, l in enumerate(body):
        m = LABEL.match(l)
        if m:
            at[m.group(1)] = i
        m = BRANCH.match(l)
        if m and m.group(1) in at and i - at[m.group(1)] > best[0]:
            best = (i - at[m.group(1)], at[m.group(1)], i)
    assert best[0] > 500, best  # a frame is several hundred instructions
    return best[1], best[2]


def test_every_row_side_pick_kernel_takes_the_q_major_image(kernels):
    # (mode, hop): the two slides, direct loads aligned and unaligned
    assert sorted(kernels) == [(0, 0), (0, 256), (0, 512), (1, 0)], sorted(kernels)


@pytest.mark.parametrize("key", [(0, 256), (0, 512), (0, 0), (1, 0)])
def test_t1_scatter_is_one_base_and_sixteen_immediates(kernels, key):
    body = kernels[key]
    lo, hi = frame_loop(body)
    stores = [(i, STORE.match(body[i])) for i in range(lo, hi + 1) if STORE.match(body[i])]
    assert len(stores) == 16, (key, len(stores))
    assert len({m.group(1) for _, m in stores}) == 1, key
    assert sorted(int(m.group(2) or 0) for _, m in stores) == [1040 * q for q in range(16)], key
    for i, m in stores:
        writes = re.compile(r"^\s+(v_\w+)\s+" + m.group(1) + r"\b")
        made = next((writes.match(body[k]).group(1) for k in range(i - 1, -1, -1) if writes.match(body[k])), None)
        assert made is not None and not made.startswith(("v_bitop3", "v_xor")), (key, made)
