"""What the compiler reports for the N = 4096 STFT kernels (-Rpass-analysis=kernel-resource-usage, the unit compiled as the build
compiles it): every instantiation built for three waves per SIMD stays within the 168 vector registers that occupancy allows,
none parks a register in scratch, and the workgroup's LDS stays 26 512 bytes (image, row region, reduction slots, pass-2 table).
The kernel hoists per-workgroup state by a per-instantiation constant (stft_kernel_impl.h: kTw3Hoist) sized against exactly
these figures; the texel instantiation is built for two waves per SIMD and has that budget (256)."""
import re

import emu_build

PLAN = re.compile(r"stft_kernelINS_4PlanILi4096ELi16EEELi(\d+)ELi(\d+)ELi(\d+)E")


def test_n4096_instantiations_keep_three_waves_no_scratch_and_their_lds():
    names, scratch, vgprs, lds = emu_build.resource_usage("stft_kernels.hip")
    seen = []
    for n, sc, vg, ld in zip(names, scratch, vgprs, lds):
        m = PLAN.search(n)
        if not m:
            continue
        mode, hop, wpe = (int(x) for x in m.groups())
        seen.append((mode, hop, wpe, n.endswith("Lb1EEEvNS_8StftArgsE")))
        assert sc == 0, (n, sc)
        assert ld == 26512, (n, ld)
        assert vg <= (168 if wpe == 3 else 256), (n, vg)
    # the two slides, direct aligned and unaligned — each with the row-side pick and without —, ranges mode and its texel kernel
    assert len(seen) == 10 and sum(1 for s in seen if s[3]) == 4 and sum(1 for s in seen if s[2] == 2) == 1, seen
    for hop in (256, 512):
        assert (0, hop, 3, True) in seen and (0, hop, 3, False) in seen, seen
