"""bench.py's multi-rank path on real hardware with the one GPU a test box has: launched exactly as the driver
launches N > 1 (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 ...`), so RCCL initialises on the
device, every step issues the asynchronous `all_gather_into_tensor` of the pitch track on RCCL's stream with the
double-buffered waits, and the gathered-track check runs (bench.py `use_dist`).  The same workload is
then run without the launcher and the two `value`s are compared: the exchange overlaps the next step's kernels, so
one rank with it must be as fast as one rank without it."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench(args, launcher):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable]
    if launcher:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port())]
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def test_bench_under_launcher_two_minutes_rccl_world1():
    """2 minutes of audio: RCCL init on device_id, the async all-gather, works[k-2].wait(), torch.equal of the gathered
    track against the rank's own — on the hardware."""
    line, err = _bench(["--steps", "20", "--warmup", "5", "--minutes", "2", "--no-cpu-baseline", "--no-supplementary"], True)
    assert line["outputs_ok"] is True and line["n_gpus"] == 1 and line["steps"] == 20
    assert line["exchange"]["backend"] == "nccl" and line["exchange"]["collective"] == "all_gather_into_tensor"
    assert line["exchange"]["gathered_equals_local"] is True
    _check_rank_records(line, 1)
    # the PCM all-gather secondary ran through RCCL too (one rank: the exchange is a device copy, the code path is the N-rank one)
    g = line["pcm_gather_secondary"]
    assert g["backend"] == "nccl" and g["gathered_ok"] is True and g["bytes_per_rank"] >= 2 * 2 * 60 * 48000 * 0.99
    # ... and so did the sharded phase vocoder's two all-gathers (phase maps, overlap-add seams) with its three device stages
    _check_pv_shard(line, 1, "nccl")
    # `value` is the contract's own W + K region; the conditioned figure is a labelled secondary
    assert "value_no_conditioning" not in line and line["value_conditioned"]["conditioning_steps"] == 40
    log = os.environ.get("MX_RCCL_LOG")
    if log:  # kept as profiles/rccl_r04_world1.log
        with open(log, "a") as f:
            f.write(json.dumps(line) + "\n")
            f.write(err[-4000:] + "\n")


def _check_pv_shard(line, world, backend):
    """`pv_shard_secondary`: the ranks' int16 slices of a common 2-minute signal concatenate to the single call's
    output (sha1), every rank's slice of the workload equals the single call over the whole signal, resident ranges (one chunk,
    analysed once), per-rank stage and all-gather times present."""
    pv = line["pv_shard_secondary"]
    assert "error" not in pv, pv
    assert pv["world_size"] == world and pv["backend"] == backend
    c = pv["common_signal"]
    assert c["equal_on_every_rank"] is True and c["sha1_concatenated_int16"] == c["sha1_single_call_int16"]
    assert c["ranges"][0][0] == 0 and c["ranges"][-1][1] == 120 * 48000
    assert pv["slices_equal_single_call"] is True
    assert [r["rank"] for r in pv["ranks"]] == list(range(world))
    for r in pv["ranks"]:
        assert r["chunks"] == 1 and r["frames"] >= 32 and r["frames"] % 32 == 0 or r["rank"] == world - 1
        assert r["stage1_ms"] > 0 and r["stage2_ms"] > 0 and r["stage3_ms"] > 0 and r["gather_maps_ms"] > 0 and r["gather_seams_ms"] > 0
    assert pv["frames_total"] == sum(r["frames"] for r in pv["ranks"]) and 0 < pv["efficiency_vs_single_call_over_own_share"] < 1.5
    assert pv["exchanged_bytes_per_rank"] == 12288 + 30720


def _check_rank_records(line, world, single_device=False):
    """`ranks`: one record per rank with its own kernel times, package power, shader clock and PCI address (what makes a
    scaling curve attributable); distinct devices unless the ranks were told to share one."""
    rk = line["ranks"]
    assert [r["rank"] for r in rk] == list(range(world))
    for r in rk:
        assert r["kernel_ms"] > 0 and r["pci"].count(":") == 2 and r["host"]
        assert r["watts"] is None or 50 < r["watts"] < 2000
        assert r["sclk_mhz"] is None or 100 < r["sclk_mhz"] < 3000
    pcis = {(r["host"], r["pci"]) for r in rk}
    assert len(pcis) == (1 if single_device else world)


def test_bench_under_launcher_matches_plain_run_full_hour():
    """The headline workload (60 min, two launches per step) with and without the launcher: `value` within 7 % (two
    processes one after the other on a shared box; the ratio itself is logged — 0.99 on a quiet one)."""
    common = ["--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-supplementary"]
    for attempt in range(2):
        plain, _ = _bench(common, False)
        dist, err = _bench(common, True)
        assert plain["outputs_ok"] and dist["outputs_ok"] and dist["n_gpus"] == 1
        assert "exchange" in dist and "exchange" not in plain and "ranks" not in plain
        ratio = dist["value"] / plain["value"]
        if 0.93 <= ratio <= 1.07:
            break
    log = os.environ.get("MX_RCCL_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"plain": plain["value"], "under_launcher": dist["value"], "ratio": ratio,
                                "plain_ms": plain["ms_per_step"], "launcher_ms": dist["ms_per_step"]}) + "\n")
            f.write(json.dumps(dist) + "\n")
    assert dist["ranks"][0]["watts"] is not None and dist["ranks"][0]["watts"] > 600  # the sampler found THIS device under load
    assert 0.93 <= ratio <= 1.07, (plain["value"], dist["value"])


def _bench_ranks_one_device(args, world=2):
    """bench.py with several ranks as that many processes on the one GPU of the box (gloo carries the exchange: RCCL refuses two
    ranks on one device) — the rank > 0 code paths on hardware: shard generation at an offset, the N - hop halo from the
    left neighbour, the pinned run length, the gathered-track check across ranks, MAX-over-ranks timing."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--dist-backend", "gloo",
           "--single-device", "--full"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("fft,hop,per_rank,world", [(4096, 256, 8192 * 1758, 2), (32768, 375, 384000 * 45, 2),
                                                    # BASELINE configs[3] itself: 8 h over 8 ranks, 60 min each (cut to
                                                    # whole run heads: 674 976 frames per rank)
                                                    (4096, 256, 172793856, 8)])
def test_ranks_on_one_device_reproduce_the_single_rank_track(fft, hop, per_rank, world):
    """Strong scaling over ONE signal: two ranks (half the signal each, halo in the pad, the whole signal's run length
    pinned) gather a pitch track that is the single-rank run's bit for bit — at a size where a shard alone would have
    picked a shorter run length (10 min at 4096/256: the advisor's round-2 counter-example)."""
    # per_rank: samples per rank, a whole number of run heads (32 frames of 256; 1024 frames of 375: shard.frame_align)
    minutes = world * per_rank / (60.0 * 48000.0)
    common = ["--steps", "4", "--warmup", "2", "--conditioning", "0", "--fft", str(fft), "--hop", str(hop),
              "--strong-total-minutes", repr(minutes), "--no-cpu-baseline", "--no-supplementary", "--no-noise-secondary",
              "--no-limiter-probe", "--no-resynth"]
    one, _ = _bench(common, False)
    two = _bench_ranks_one_device(common, world)
    assert one["outputs_ok"] and two["outputs_ok"] and two["n_gpus"] == world and two["scaling"] == "strong"
    assert two["exchange"]["backend"] == "gloo" and two["exchange"]["gathered_equals_local"] is True
    assert two["config"]["frames_per_gpu"] == per_rank // hop and one["config"]["frames_per_gpu"] == world * per_rank // hop
    assert two["exchange"]["gathered_track_sha1"] == one["pitch_track_sha1"]
    log = os.environ.get("MX_RCCL_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({f"world{world}_one_device": {"fft": fft, "hop": hop, "minutes": minutes,
                                                      "track_sha1": one["pitch_track_sha1"],
                                                      "gathered_sha1": two["exchange"]["gathered_track_sha1"]}}) + "\n")


def test_eight_ranks_on_one_device_carry_rank_records_the_pcm_gather_and_the_pv_seams():
    """The driver's weak-scaling form at world 8 (5 min per rank to keep eight processes on one GPU short), resynthesis in
    the step: the line carries every rank's own record and the timed int16 PCM all-gather over the ranks'
    shards, each rank having checked its own shard and the others' presence in the gathered stream."""
    common = ["--steps", "4", "--warmup", "2", "--conditioning", "0", "--minutes", "5", "--no-cpu-baseline",
              "--no-supplementary", "--no-noise-secondary", "--pcm-gather-reps", "2"]
    line = _bench_ranks_one_device(common, 8)
    assert line["outputs_ok"] and line["n_gpus"] == 8 and line["scaling"] == "weak"
    _check_rank_records(line, 8, single_device=True)
    g = line["pcm_gather_secondary"]
    assert g["gathered_ok"] is True and g["world_size"] == 8 and len(g["samples_per_rank"]) == 8
    assert g["bytes_per_rank"] >= 2 * min(g["samples_per_rank"]) and g["seconds"] > 0
    assert abs(g["frac_of_xgmi_peak"] - g["recv_GBps_per_rank"] / (7 * 153.0)) < 1e-12
    # the phase vocoder sharded over the eight ranks: the collective north_star names (the overlap-add seams) in the N-rank bench
    _check_pv_shard(line, 8, "gloo")
    log = os.environ.get("MX_RCCL_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"world8_one_device_weak_5min": line}) + "\n")


def _bench_ranks_by_hand(args, world, mask_devices, timeout=600):
    """`world` bench.py processes started by hand with the launcher's environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*),
    each with its own HIP_VISIBLE_DEVICES when `mask_devices` — the layout of a launcher that hands every rank ONE device."""
    port = str(_free_port())
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port})
        if mask_devices:
            env["HIP_VISIBLE_DEVICES"] = "0"  # (the box has one GPU: every rank's "own" device is that one)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--full"] + args, cwd=ROOT, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p_ in procs:
        try:
            outs.append(p_.communicate(timeout=timeout) + (p_.returncode,))
        except subprocess.TimeoutExpired:
            p_.kill()
            outs.append(p_.communicate() + (-9,))
    return outs


def test_ranks_with_one_visible_device_each():
    """A launcher that masks the devices per rank (HIP_VISIBLE_DEVICES) leaves every rank with ONE device, ordinal 0, whatever its
    LOCAL_RANK: round 4's bench.py called set_device(LOCAL_RANK) and rank 1 died at start-up.  Two ranks here, LOCAL_RANK 0 and
    1, each seeing only device 0: both run, rank 1 on ordinal 0; the gathered track is checked as in every multi-rank run."""
    minutes = 2 * 8192 * 1758 / (60.0 * 48000.0)
    args = ["--steps", "3", "--warmup", "1", "--conditioning", "0", "--strong-total-minutes", repr(minutes), "--no-cpu-baseline",
            "--no-supplementary", "--no-noise-secondary", "--no-limiter-probe", "--no-resynth", "--dist-backend", "gloo",
            "--allow-shared-device", "--n1-value", "1e8"]
    outs = _bench_ranks_by_hand(args, 2, True)
    assert all(rc == 0 for _, _, rc in outs), [(o[-1500:], e[-3000:], rc) for o, e, rc in outs]
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not [ln for ln in outs[1][0].splitlines() if ln.startswith("{")]
    line = json.loads(lines[0])
    assert line["outputs_ok"] and line["n_gpus"] == 2 and line["exchange"]["gathered_equals_local"] is True
    rk = line["ranks"]
    assert [r["local_rank"] for r in rk] == [0, 1] and [r["device_ordinal"] for r in rk] == [0, 0]
    assert all(r["visible_devices"] == 1 for r in rk)
    eff = line["efficiency_vs_n1"]
    assert eff["n_gpus"] == 2 and abs(eff["value"] - line["value"] / 2e8) < 1e-12
    assert line["library_src_sha"] and line["library_version"].endswith("src:" + line["library_src_sha"])


def test_start_up_that_cannot_complete_ends_with_a_json_error():
    """Rank 0 of a two-rank job whose rank 1 never shows up: instead of hanging in the rendezvous (the one failure of an 8-GPU
    launch that cannot be debugged from outside) the process prints a one-line JSON error and exits 5 within the time-out."""
    import time
    port = str(_free_port())
    env = dict(os.environ)
    env.update({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port})
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--init-timeout", "8",
                        "--minutes", "1", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 5, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert time.time() - t0 < 120
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    err = json.loads(lines[0])
    assert "error" in err and err["rank"] == 0 and err["world_size"] == 2
