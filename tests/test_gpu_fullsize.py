"""BASELINE.json's full sizes (60 min of 48 kHz audio, 675 000 frames at N=4096/hop=256) checked
through size-independent properties — the oracle cannot cover them in seconds:
  * the pitch track of the synthetic sweep follows its known instantaneous frequency;
  * frames sampled from the bulk run equal the same (start,end) computed in ranges mode
    (bit-exact with one frame per workgroup, within 1/10 of the tolerance with the sliding window);
  * any sub-range of frames computed on its own equals the corresponding rows of the full run;
  * a handful of rows against the oracle;
  * resynthesis: identity schedule reproduces the source bit for bit over the whole grain chain;
    every step of the +3 st schedule starts on its grain's first sample; counts add up."""
import numpy as np
import pytest

from conftest import SR, mag_tol, noisy

pytestmark = pytest.mark.gpu

N, HOP = 4096, 256
MINUTES = 60


@pytest.fixture(scope="module")
def hour(oracle):
    return oracle.sweep(MINUTES * 60 * SR)  # closed-form 110 -> 1760 Hz sweep, ~3 s on the host


def test_stft_full_size_properties(gpu_ctx, oracle, hour):
    w = hour
    n = len(w)
    F = (n + HOP - 1) // HOP
    assert F == 675000
    a = gpu_ctx.upload(w)
    band = (5, 150)
    # pitch track of the whole hour (the magnitudes, 5.5 GB, stay on the device in bench.py; here
    # only slices are pulled back)
    _, pitch = gpu_ctx.stft_hop(a, N, HOP, band=band, want_mags=False)
    assert len(pitch) == F
    h = np.arange(F)
    # instantaneous frequency at the centre of gravity of the one-sided window (~the frame end)
    t_end = (h + 1) * HOP / SR
    T = n / SR
    f_inst = 110.0 + (1760.0 - 110.0) * t_end / T
    expect = f_inst * N / SR
    sel = (expect > band[0] + 3) & (expect < band[1] - 3) & (h > N // HOP)
    # the window reaches back ~4000 samples (83 ms): the sweep moves < 0.04 Hz in that time
    assert np.abs(pitch["bin"][sel] - expect[sel]).max() <= 1.5
    assert (np.diff(pitch["bin"][sel].astype(int)) >= -1).all()  # monotone sweep, up to rounding
    assert (pitch["mag"][sel] > 0.05).all()

    # sampled frames: bulk (sliding window) vs ranges mode (direct load) vs one-frame-per-workgroup bulk
    rng = np.random.default_rng(42)
    pick = np.unique(np.concatenate([[0, 1, 15, 16, 17, F - 2, F - 1], rng.integers(0, F, 40)]))
    rr = np.stack([pick * HOP, (pick + 1) * HOP], axis=1).astype(np.int32)
    m_ranges, p_ranges = gpu_ctx.stft_ranges(a, N, rr, band=band)
    sub = []
    for f in pick:
        m, p = gpu_ctx.stft_hop(a, N, HOP, first=int(f), count=1, band=band)
        sub.append(m[0])
        assert p["bin"][0] == p_ranges["bin"][list(pick).index(f)]
    sub = np.stack(sub)
    assert np.array_equal(sub, m_ranges)  # a one-frame call loads the frame directly: bit-exact indexing
    # the same frames inside a long bulk run (carried through the sliding window)
    lo = int(pick[10])
    m_run, p_run = gpu_ctx.stft_hop(a, N, HOP, first=lo - lo % 16, count=4096, band=band)
    inside = [(i, f) for i, f in enumerate(pick) if lo - lo % 16 <= f < lo - lo % 16 + 4096]
    for i, f in inside:
        row = m_run[f - (lo - lo % 16)]
        assert (np.abs(row - m_ranges[i]) <= mag_tol(m_ranges[i][None])[0] / 10).all()
    # sub-range == full-run rows (same workgroup partition when the start is a multiple of frames_per_block)
    m_a, _ = gpu_ctx.stft_hop(a, N, HOP, first=160000, count=512, band=band)
    m_b, _ = gpu_ctx.stft_hop(a, N, HOP, first=160000 + 256, count=256, band=band)
    assert np.array_equal(m_a[256:], m_b)
    # and a few rows against the oracle itself
    for i in (0, 5, 20, len(pick) - 1):
        s, e = int(rr[i, 0]), int(rr[i, 1])
        ref = oracle.spec_frame(w, N, s, e)
        assert (np.abs(m_ranges[i] - ref) <= mag_tol(ref[None])[0]).all()
    a.free()


@pytest.mark.parametrize("N2,HOP2", [(16384, 512), (32768, 375)])
def test_stft_full_size_other_plans(gpu_ctx, oracle, hour, N2, HOP2):
    """BASELINE configs[4] (N = 16384, hop 512: 337 500 frames, the sliding kernel) and the reference's own
    SpectrSize at the default view's column width (N = 32768, 375-sample columns, spec.cpp:8 / SURVEY 8a-5: 460 800
    frames, direct loads with in-kernel weights) over the whole hour, through the same size-independent properties."""
    w = hour
    n = len(w)
    F = (n + HOP2 - 1) // HOP2
    a = gpu_ctx.upload(w)
    band = oracle.pitch_band(N2, SR)
    _, pitch = gpu_ctx.stft_hop(a, N2, HOP2, band=band, want_mags=False)
    assert len(pitch) == F
    h = np.arange(F)
    f_inst = 110.0 + (1760.0 - 110.0) * ((h + 1) * HOP2 / SR) / (n / SR)
    expect = f_inst * N2 / SR
    sel = (expect > band[0] + 8) & (expect < band[1] - 8) & (h > N2 // HOP2)
    # the window is ~4000 samples long whatever N is: a bin is SR/N wide, the peak's own width ~N/4000 bins
    assert np.abs(pitch["bin"][sel] - expect[sel]).max() <= 1.5 * N2 / 4096
    assert (pitch["mag"][sel] > 0.05 * 4096 / N2).all()
    rng = np.random.default_rng(N2)
    pick = np.unique(np.concatenate([[0, 1, N2 // HOP2, F - 2, F - 1], rng.integers(0, F, 24)]))
    rr = np.stack([pick * HOP2, (pick + 1) * HOP2], axis=1).astype(np.int32)
    m_ranges, p_ranges = gpu_ctx.stft_ranges(a, N2, rr, band=band)
    # the same frames inside a bulk run (sliding window at 16384/512, derived weights at 32768/375)
    for i in (3, 9, 17):
        f = int(pick[i])
        lo = max(0, f - 40)
        m_run, p_run = gpu_ctx.stft_hop(a, N2, HOP2, first=lo, count=64, band=band)
        assert (np.abs(m_run[f - lo] - m_ranges[i]) <= mag_tol(m_ranges[i][None])[0] / 10).all()
        assert p_run["bin"][f - lo] == p_ranges["bin"][i] == pitch["bin"][f]
    for i in (0, 7, len(pick) - 1):
        ref = oracle.spec_frame(w, N2, int(rr[i, 0]), int(rr[i, 1]))
        assert (np.abs(m_ranges[i] - ref) <= mag_tol(ref[None])[0]).all()
    a.free()


def _host_threads():
    """Threads the oracle may use: the affinity mask cut to the cgroup CPU quota (as bench.py's cpu_baseline does)."""
    import os

    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, -(-int(q) // int(p)))
    except Exception:
        pass
    return max(1, n)


def _whole_config_vs_oracle(gpu_ctx, oracle, w, N2, hop, chunk, every):
    """The WHOLE configuration against the oracle (spec.cpp:44-66 restated, binary64 DFT, all host cores): every pitch
    record of the full run, and the magnitude rows of every `every`-th chunk of `chunk` frames (every = 1: all rows) plus
    both ends, each row within 2e-5 of its oracle peak.  The device rows are pulled back chunk by chunk from
    launches that start on run heads with the full run's run length pinned, i.e. they are the full run's rows bit for bit
    (test_shards_of_circular_window_kernels_equal_unsharded / the 8 h shard test establish that)."""
    import os
    import time

    from melonix_amd import shard as sh

    n = len(w)
    F = (n + hop - 1) // hop
    T = _host_threads()
    band = oracle.pitch_band(N2, SR)
    a = gpu_ctx.upload(w)
    assert chunk % sh.frame_align(N2, hop) == 0
    g = sh.pin_run_length(gpu_ctx, N2, hop, F)
    try:
        t0 = time.time()
        _, pitch = gpu_ctx.stft_hop(a, N2, hop, band=band, want_mags=False)
        _, ob, om = oracle.stft_hop(w, N2, hop, band=band, want_mags=False, nthreads=T)
        t_pitch = time.time() - t0
        assert len(pitch) == F == len(ob)
        # every record: the same bin, or a near-tie — the oracle's magnitude at the device's bin within twice the row
        # tolerance of the oracle's maximum (the rule of test_gpu_stft._check_pitch)
        diff = np.nonzero(pitch["bin"] != ob)[0]
        assert len(diff) <= 500, f"{len(diff)} of {F} pitch bins differ from the oracle's"
        for f in diff:
            ref = oracle.spec_frame(w, N2, int(f) * hop, (int(f) + 1) * hop)
            b = int(pitch["bin"][f])
            assert band[0] <= b <= band[1]
            assert ref[ob[f]] - ref[b] <= 2 * (2e-5 * ref.max() + 1e-9), (int(f), b, int(ob[f]))
        # every record's magnitude (in-band peak <= frame peak, so this is the row tolerance or tighter; the few frames
        # where it is tighter than the device manages are re-checked against the frame's real peak)
        same = pitch["bin"] == ob
        over = np.nonzero(same & (np.abs(pitch["mag"] - om) > 2e-5 * om + 1e-9))[0]
        assert len(over) <= 500, len(over)
        for f in over:
            ref = oracle.spec_frame(w, N2, int(f) * hop, (int(f) + 1) * hop)
            assert abs(float(pitch["mag"][f]) - float(ref[ob[f]])) <= 2e-5 * ref.max() + 1e-9, int(f)
        # magnitude rows
        starts = list(range(0, F, chunk))
        take = sorted(set(starts[::every]) | {starts[0], starts[-1]})
        rows, worst = 0, 0.0
        t0 = time.time()
        for c in take:
            cnt = min(chunk, F - c)
            gm, gp = gpu_ctx.stft_hop(a, N2, hop, first=c, count=cnt, band=band)
            rm, _, _ = oracle.stft_hop(w, N2, hop, first=c, count=cnt, band=band, nthreads=T)
            tol = 2e-5 * rm.max(axis=1) + 1e-9
            np.subtract(gm, rm, out=rm)
            np.abs(rm, out=rm)
            err = rm.max(axis=1)
            bad = np.nonzero(err > tol)[0]
            assert len(bad) == 0, (c + int(bad[0]), float(err[bad[0]]), float(tol[bad[0]]))
            # the chunk's pitch records are the full run's (same runs), and each is its row's own value
            assert np.array_equal(gp["bin"], pitch["bin"][c:c + cnt]) and np.array_equal(gp["mag"], pitch["mag"][c:c + cnt])
            assert np.array_equal(gp["mag"], gm[np.arange(cnt), gp["bin"]])
            worst = max(worst, float((err / tol).max()))
            rows += cnt
        t_rows = time.time() - t0
    finally:
        gpu_ctx.set_frames_per_block(0)
        a.free()
    msg = (f"whole-config vs oracle N={N2} hop={hop}: {F} of {F} pitch records ({len(diff)} near-ties, {len(over)} re-checked "
           f"magnitudes) in {t_pitch:.1f} s; {rows} of {F} magnitude rows ({len(take)} chunks of {chunk}) in {t_rows:.1f} s, "
           f"worst row error {worst:.3f} of the 2e-5*peak tolerance; run length {g}, {T} oracle threads")
    print(msg)
    log = os.environ.get("MX_PARITY_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(msg + "\n")
    return F, rows


def test_config1_whole_hour_every_record_and_row_vs_oracle(gpu_ctx, oracle, hour):
    """BASELINE configs[1] in full: all 675 000 pitch records and all 675 000 magnitude rows (5.5 GB) of the hour."""
    F, rows = _whole_config_vs_oracle(gpu_ctx, oracle, hour, N, HOP, chunk=16384, every=1)
    assert F == 675000 and rows == F


def test_config4_whole_hour_vs_oracle(gpu_ctx, oracle, hour):
    """BASELINE configs[4] (N = 16384, hop 512) in full: all 337 500 pitch records, all magnitude rows (11 GB)."""
    F, rows = _whole_config_vs_oracle(gpu_ctx, oracle, hour, 16384, 512, chunk=4096, every=1)
    assert F == 337500 and rows == F


def test_reference_size_whole_hour_vs_oracle(gpu_ctx, oracle, hour):
    """The reference's own transform (N = 32768, spec.cpp:8) at its default column width (375 samples) over the hour: all
    460 800 pitch records and all 460 800 magnitude rows (30.2 GB, pulled back in chunks of 1024 rows)."""
    F, rows = _whole_config_vs_oracle(gpu_ctx, oracle, hour, 32768, 375, chunk=1024, every=1)
    assert F == 460800 and rows == F


def test_resynth_full_size_properties(gpu_ctx, mxlib, hour):
    w = hour
    n = len(w)
    a = gpu_ctx.upload(w)
    s, l = gpu_ctx.grains_dev(a)
    assert s[0] == 0 and (s[1:] == s[:-1] + l[:-1]).all()      # the chain covers [0, lastEnd) without gaps
    assert l.min() >= 751 and int(s[-1] + l[-1]) > n - 4000      # good grains only, chain reaches the end
    # identity: no markers -> rate 1 -> PCM is the source over the chain, then 1500 zeros (app.cpp:303-309)
    st0, tot0 = mxlib.schedule_build(w, SR, s, l, [])
    assert len(st0) == len(s) and tot0 == int(l.sum()) + 1500
    f32, i16 = gpu_ctx.resynth(a, st0, tot0)
    assert np.array_equal(f32[:-1500].view(np.uint32) & 0x7FFFFFFF, w[: tot0 - 1500].view(np.uint32) & 0x7FFFFFFF)
    assert np.array_equal(f32[:-1500], w[: tot0 - 1500]) and not f32[-1500:].any()
    assert np.array_equal(i16[: tot0 - 1500], (w[: tot0 - 1500].astype(np.float64) * 32767.0).astype(np.int16))
    # +3 semitones over the whole hour (BASELINE configs[2])
    mk = [(1, 0, 0, 3.0), (n - 1, 0, 0, 3.0)]
    st, tot = mxlib.schedule_build(w, SR, s, l, mk)
    assert tot == int(st["sz"].sum()) + 1500
    assert (st["out_offset"][1:] == np.cumsum(st["sz"])[:-1]).all() and st["out_offset"][0] == 0
    rate = np.float32(2.0) ** (np.float32(3.0) / np.float32(12))
    assert (st["rate"][2:-2] == st["rate"][5]).all() and abs(float(st["rate"][5]) - float(rate)) < 1e-6
    f3, _ = gpu_ctx.resynth(a, st, tot, want_i16=False)
    # i = 0 of every step: x = 0, f = 0 -> the grain's first sample, exactly
    assert np.array_equal(f3[st["out_offset"]], w[st["grain_start"]])
    assert abs(tot / n - 1.0) < 5e-3 and not f3[-1500:].any()    # duration preserved (grains repeat/skip)
    assert np.abs(f3).max() <= np.abs(w).max() + 1e-6            # linear interpolation never overshoots
    a.free()


def test_pv_full_size_properties(gpu_ctx, oracle, hour):
    """The build-defined phase vocoder over the whole hour (BASELINE configs[2]'s size; 802 716 analysis frames at
    +3 st), through properties only: length kept, deterministic, identity at 0 semitones, level kept, and the pitch
    track of the OUTPUT — measured by this build's own STFT + pitch pick — is the sweep's track times 2^(3/12)."""
    w = hour
    n = len(w)
    a = gpu_ctx.upload(w)
    y0, _ = gpu_ctx.pv_pitch_shift(a, 0.0, want_i16=False)
    assert len(y0) == n and np.abs(y0[4096:-4096] - w[4096:-4096]).max() < 4e-6
    del y0
    y, i16 = gpu_ctx.pv_pitch_shift(a, 3.0)
    assert len(y) == n and len(i16) == n
    y2, _ = gpu_ctx.pv_pitch_shift(a, 3.0, want_i16=False)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))  # no atomics anywhere: bit-reproducible
    del y2
    assert np.array_equal(i16, (np.clip(y, -1.0, 1.0).astype(np.float64) * 32767.0).astype(np.int16))
    # Level: kept on a sweep too (identity phase locking; with independently propagating bins it came out at 0.75)
    rms_in = np.sqrt((w[n // 4: n // 2].astype(np.float64) ** 2).mean())
    rms_out = np.sqrt((y[n // 4: n // 2].astype(np.float64) ** 2).mean())
    assert abs(rms_out / rms_in - 1.0) < 0.01
    a.free()
    b = gpu_ctx.upload(y)
    band = (5, 200)
    _, pitch = gpu_ctx.stft_hop(b, N, HOP, band=band, want_mags=False)
    F = len(pitch)
    h = np.arange(F)
    f_in = 110.0 + (1760.0 - 110.0) * ((h + 1) * HOP / SR) / (n / SR)
    expect = f_in * 2.0 ** (3.0 / 12.0) * N / SR
    sel = (expect > band[0] + 3) & (expect < band[1] - 3) & (h > 64) & (h < F - 64)
    assert sel.sum() > 50000
    assert np.abs(pitch["bin"][sel] - expect[sel]).max() <= 2.0
    b.free()


def test_export_full_hour_bit_exact_vs_oracle(gpu_ctx, oracle, mxlib, hour, tmp_path):
    """BASELINE configs[2] at full size: the +3 st export of the whole 60 minutes (app.cpp:1194-1215) — grains, every
    field of every process() step, the f32 PCM bitwise, the int16 PCM, sample and step counts — against the oracle's
    restatement of the same hour (about a second of host time), and the WAV bytes through mx_resynth_to_wav."""
    w = hour
    n = len(w)
    mk = [(1, 0, 0, 3.0), (n - 1, 0, 0, 3.0)]
    ost, opcm = oracle.export_run(w, SR, mk)
    a = gpu_ctx.upload(w)
    s, l = gpu_ctx.grains_dev(a)
    rs, rl = oracle.grains(w)
    assert np.array_equal(s, rs) and np.array_equal(l, rl)
    st, total = mxlib.schedule_build(w, SR, s, l, mk)
    # (the terminating process() call — no grain left, 1500 zeros — is not a step record on either side)
    assert len(st) == len(ost) and total == len(opcm) and total == int(st["sz"].sum()) + 1500
    for field in ("cursor", "grain_start", "grain_len", "rate", "next_first", "sz", "out_offset"):
        assert np.array_equal(st[field], ost[field]), field
    f32, i16 = gpu_ctx.resynth(a, st, total)
    assert np.array_equal(f32.view(np.uint32), opcm.view(np.uint32))  # bitwise, all 172.8 M samples
    o16 = oracle.pcm_to_i16(opcm)
    assert np.array_equal(i16, o16)
    del f32
    path = tmp_path / "hour.wav"
    gpu_ctx.resynth_to_wav(a, st, total, SR, path, strict=True)
    got = path.read_bytes()
    assert len(got) == 44 + 2 * total and got == oracle.wav_bytes(o16, SR)
    a.free()


def test_eight_shards_on_one_device_equal_unsharded_8h():
    """BASELINE configs[3] played on one device (tests/tools/shard8_check.py): 8 h of the sweep cut into the 8 frame
    shards `shard_frames` gives 8 ranks, each its own padded image with the N - hop halo, run shard by shard through
    mx_stft_hop_dev; every magnitude row (the 7 seams included) and the concatenated pitch track bit-identical to the
    unsharded 8 h run, seam rows against the oracle; and configs[3] in full against the oracle: all 5.4 M pitch records of
    the 8 h signal plus 65 536 magnitude rows spread over it.  Runs in its own process: the 44 GB comparison happens on the
    device through torch, which has to initialise the HIP runtime before the C-ABI library does."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "tools", "shard8_check.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shard8_check ok" in r.stdout


@pytest.mark.parametrize("N,hop,world,hours", [(32768, 375, 2, 0.3), (16384, 375, 3, 0.25), (32768, 512, 2, 0.4),
                                               # shards too short for the unsharded run length on their own (10 min at
                                               # 4096/256: 112 500 frames -> runs of 32, a 2-rank shard alone would pick
                                               # 16; an hour at 32768/375 over 8 ranks: 32 against 16) — pinned by
                                               # shard.pin_run_length
                                               (4096, 256, 2, 1 / 6), (4096, 256, 5, 1 / 6), (32768, 375, 8, 1.0),
                                               (16384, 512, 7, 0.1)])
def test_shards_of_circular_window_kernels_equal_unsharded(N, hop, world, hours):
    """The circular-window kernels round by where a frame starts inside a slot of the device image: `shard_frames` puts
    shard boundaries on whole slots (frame_align), so shards run on their own images are still the unsharded run bit for
    bit — every row and the pitch track (same checker as the 8 h test, its own process for the same reason).  The run
    length of every shard is pinned to the whole signal's (shard.pin_run_length): shard sizes are free."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "tools", "shard8_check.py"), str(hours), str(N), str(hop), str(world)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shard8_check ok" in r.stdout


def test_pv_hour_is_bit_for_bit_what_the_single_launch_gave():
    """The hour of the bench workload at +3 st under every arena policy — the default budget (a quarter of the free memory: the
    hour is RESIDENT, one chunk, 17.9 GB), budgets of 8 and 2.4 GB (chunks of ~179 k and ~52 k frames) and an explicit chunk
    length of 8192 frames: the output's sha1s are the ones round 4's single launch over a 33 GB arena produced
    (`profiles/variants_r04_pv_steps.log`), f32 and int16.  (The vocoder is build-defined; the suite compares it with its
    oracle up to ten minutes — tests/test_pv.py — and tests/tools/pv_hour_vs_oracle.py has run the oracle over this very hour:
    the output with these sha1s is within 4.6e-7 of it, profiles/pv_hour_vs_oracle_r06.log.)"""
    import os
    import re
    import subprocess
    import sys

    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pv_ab.py")
    for var, val, chunks in (("", "", 1), ("MELONIX_PV_ARENA_MB", "8192", 5), ("MELONIX_PV_ARENA_MB", "2400", 16), ("MELONIX_PV_CHUNK_FRAMES", "8192", 98)):
        env = dict(os.environ)
        for k in ("MX_AB_LIB", "MELONIX_PV_CHUNK_FRAMES", "MELONIX_PV_ARENA_MB"):
            env.pop(k, None)
        if var:
            env[var] = val
        r = subprocess.run([sys.executable, tool, "60", "3", "sweep"], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert "sha1 f32 7d5500cef5117a15 i16 89ee573a94112bd2" in r.stdout, r.stdout[-500:]
        m = re.search(r"arena ([0-9.]+) GB of a budget of ([0-9.]+) GB, (\d+) chunk", r.stdout)
        assert m, r.stdout[-500:]
        assert float(m.group(1)) <= float(m.group(2)) + 0.05 or var == "MELONIX_PV_CHUNK_FRAMES"
        assert (int(m.group(3)) == 1) == (chunks == 1) and abs(int(m.group(3)) - chunks) <= max(2, chunks // 4), (var, val, r.stdout[-300:])


def test_pv_eight_hours_on_one_gpu_bounded_arena():
    """BASELINE configs[3]'s signal through the phase vocoder on ONE GPU (tests/tools/pv8h_check.py): rounds 1-4 needed
    ~260 GB of work buffers for it (41 KiB per frame, one allocation) and failed with MX_ERR_NOMEM; under the default budget
    (a quarter of the free memory) it is walked in a handful of long chunks, under a 2.4 GB budget in ~120 short ones.
    Properties of the output (int16 = clamped f32, level kept, deterministic, the output's pitch track = the sweep's times
    2^(3/12) by this build's own STFT) and the multi-GPU path on the same signal: eight ranks (an hour each: configs[3]) played on this device through the
    device-pointer stages — resident ranges analysed ONCE, stage times against the single call's — equal it bit for bit."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "tools", "pv8h_check.py"), "8", "8"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pv8h_check ok" in r.stdout


def test_pv_more_than_2M_frames(gpu_ctx, hour):
    """+24 semitones over the hour is 2.7 M analysis frames: the boundary fix-up kernel used to put one block row per
    32 frames on gridDim.y (capped at 65 535, i.e. 2.1 M frames) and the call failed after all the work was done."""
    w = hour
    n = len(w)
    a = gpu_ctx.upload(w)
    y, _ = gpu_ctx.pv_pitch_shift(a, 24.0, want_i16=False)
    assert len(y) == n and np.isfinite(y).all()
    # the 110..1760 Hz sweep lands two octaves up: still a tone of the input's level where it stays below Nyquist
    seg = slice(n // 8, n // 4)
    assert 0.5 < np.sqrt((y[seg].astype(np.float64) ** 2).mean()) / np.sqrt((w[seg].astype(np.float64) ** 2).mean()) < 1.1
    gpu_ctx.release_scratch()
    a.free()


def test_host_staged_paths_across_a_staging_chunk_boundary(gpu_ctx, sweep10):
    """The host-staged entry points walk a batch in staging chunks of ~1 GiB of rows: 16384 columns at N = 32768.  A
    batch of 16384 + 40 columns crosses that boundary once on every path that has one — ranges mode with magnitudes and
    pitch records, the texel rows with magnitudes, the kept rows with texels and magnitudes, and the re-colouring of
    kept rows.  Ranges-mode rows do not depend on their batch, so the one call must equal, bit for bit, two calls of
    one chunk each put end to end (the per-chunk offsets into the ranges, the rows, the texels and the kept rows)."""
    N3, C, K = 32768, 16384, 900.0
    count = C + 40
    a = gpu_ctx.upload(noisy(sweep10))
    start = np.arange(count) * ((len(sweep10) - 375) // count)
    cols = np.stack([start, start + 375], axis=1).astype(np.int32)

    def halves_equal(whole, head, tail):
        return np.array_equal(whole[:C], head) and np.array_equal(whole[C:], tail)

    # ranges mode: magnitudes + pitch records
    m, p = gpu_ctx.stft_ranges(a, N3, cols)
    assert m.shape == (count, N3 // 2) and float(m[C:].max()) > 0
    mh, ph = gpu_ctx.stft_ranges(a, N3, cols[:C])
    assert np.array_equal(m[:C], mh) and np.array_equal(p[:C], ph)
    del mh
    mt, pt = gpu_ctx.stft_ranges(a, N3, cols[C:])
    assert np.array_equal(m[C:], mt) and np.array_equal(p[C:], pt)
    del m, mt

    # texel rows with the magnitudes of the same launch
    rgb, m = gpu_ctx.stft_ranges_rgb(a, N3, cols, K, want_mags=True)
    assert int(rgb[C:].max()) > 0
    rh, mh = gpu_ctx.stft_ranges_rgb(a, N3, cols[:C], K, want_mags=True)
    rt, mt = gpu_ctx.stft_ranges_rgb(a, N3, cols[C:], K, want_mags=True)
    assert halves_equal(rgb, rh, rt) and halves_equal(m, mh, mt)
    del rgb, m, rh, mh, rt, mt

    # kept rows: the texels and magnitudes that come back, the rows that stay, and their re-colouring
    rows, rgb, m = gpu_ctx.stft_ranges_keep(a, N3, cols, k=K, want_mags=True)
    rows_h, rh, mh = gpu_ctx.stft_ranges_keep(a, N3, cols[:C], k=K, want_mags=True)
    rows_t, rt, mt = gpu_ctx.stft_ranges_keep(a, N3, cols[C:], k=K, want_mags=True)
    assert len(rows) == count
    assert halves_equal(rgb, rh, rt) and halves_equal(m, mh, mt)
    del rgb, rh, rt, mh, mt
    assert np.array_equal(rows.fetch(0, count), m)  # what stayed is what came back
    assert np.array_equal(rows.fetch(C - 20, 40), m[C - 20:C + 20])
    del m
    K2 = 400.0
    c = rows.colormap(0, count, K2)
    assert int(c[C:].max()) > 0
    assert halves_equal(c, rows_h.colormap(0, C, K2), rows_t.colormap(0, count - C, K2))
    assert np.array_equal(rows.colormap(8, C + 16, K2), c[8:C + 24])  # a span that starts inside the batch
    del c
    for r in (rows, rows_h, rows_t):
        r.free()
    gpu_ctx.release_scratch()
    a.free()
