"""GPU: bench.py's multi-rank code path on one GPU (`--force-dist-path`: device-resident record log + the chunked stitch,
world size 1), over several timed regions -- the path the driver runs with --gpus N > 1, where every region reuses the log
and the stitch (a stale piece list made rank_logs() return the records of all regions; found in round 2)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forced_dist_path_runs_several_regions():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-dist-path", "--no-cpu-baseline", "--no-c3",
                        "--no-end-to-end", "--no-breakdown", "--config", "c1", "--steps", "16", "--warmup", "4"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stderr[-3000:]
    out = json.loads(lines[-1])
    assert out["steps"] == 16 and out["n_gpus"] == 1 and out["value"] > 0
    assert out["config"]["timed_regions"] > 1, "the short C1 regions must repeat (the case that reuses the stitch)"


def test_watchdog_prints_the_line_measured_so_far_when_the_stitch_hangs():
    """The N > 1 path has never run between two GPUs: a rank that stops progressing (here: a simulated hang where the
    stitches are created) must not leave the job without a line.  The ranks time the N = 1 code path first; the watchdog
    prints that line, marked incomplete, and the process leaves with exit code 0."""
    env = dict(os.environ, POLYCHASE_BENCH_TEST_HANG="stitch", POLYCHASE_BENCH_WATCHDOG_S="5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist-path", "--no-cpu-baseline", "--no-c3",
                        "--no-end-to-end", "--no-breakdown", "--config", "c1", "--steps", "16", "--warmup", "4"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["value"] > 0 and out["steps"] == 16 and "no progress" in out["incomplete"] and "stitch" in out["incomplete"]
    assert out["metric"] == "optical-flow frames/sec" and out["config"]["stitch"].startswith("none")


# ("peer" rides in test_c4_label_of_the_nested_4k_block_with_two_ranks and "rccl" in test_gpus_flag_launches_the_ranks_itself since
# round 6: the same assertions on jobs that are run anyway -- VERDICT r05 #7, the suite's time)
@pytest.mark.parametrize("stitch", ["peer-broken"])
def test_two_ranks_on_one_gpu_over_gloo(stitch):
    """bench.py exactly as the driver launches it for --gpus 2 (torch.distributed.run, two processes), except that both
    ranks sit on GPU 0 and the process group is gloo (POLYCHASE_BENCH_SHARE_GPU=1): the region count agreed by all-reduce,
    the stitch with two shards, the per-rank record checks and the max-over-ranks timing all run.  "peer" (the default): each
    rank maps the other's receive buffer through HIP IPC and pushes its pieces with device-to-device copies
    (distributed.PeerLogStitch; here both buffers live on GPU 0); "rccl": the chunked all-gather (gloo here);
    "peer-broken": rank 1 cannot export its buffer -- BOTH ranks must fall back to the all-gather, nobody waits."""
    env = dict(os.environ, POLYCHASE_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1", POLYCHASE_BENCH_STITCH=stitch.split("-")[0],
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    if stitch == "peer-broken":
        env["POLYCHASE_TEST_BREAK_PEER_EXPORT"] = "1"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "16",
                        "--warmup", "4", "--config", "c1", "--no-c3", "--no-breakdown"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 16 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["stitch"].startswith("xgmi peer copies" if stitch == "peer" else "rccl all_gather"), (out["config"]["stitch"], r.stderr[-2000:])
    _check_multi_gpu_keys(out, 2, peer=stitch == "peer", peer_wanted=stitch != "rccl")


def _check_multi_gpu_keys(out, n, peer, peer_wanted, arith_modes=True, top=True):
    """what ONE N-GPU run must return: both stitches and the analysis-only rate of the same job,
    per-rank step times, the exposed stitch time, bytes per second per peer link, world size and backend"""
    assert out["world_size"] == n and out["collectives_backend"] in ("nccl", "gloo")
    # the N > 1 figure is labelled analysis-only and carries the writer-bound product rate beside it
    assert out["claim"].startswith("analysis-only (no insert)")
    assert out["product_rate_with_insert"].get("value", 0) > 0, out["product_rate_with_insert"]
    assert out["gpu_busy_ms_per_step"] > 0
    assert not top or ("host" in out and "thread_placement" in out["host"])      # (the line's, not a nested block's)
    assert out["config"]["arith"] == "opencv_x86" and (not arith_modes or set(out["arith_modes"]) >= {"opencv_x86", "canonical"})
    ab = out["stitch_ab"]
    assert "rccl" in ab and ab["rccl"]["stitch"].startswith("rccl all_gather")
    if peer:
        assert ab["peer"]["stitch"].startswith("xgmi peer copies")
        assert out["value"] == ab["peer"]["value"]
    elif peer_wanted:
        assert "unavailable" in ab["peer"]
    for m in ("peer", "rccl"):
        if m in ab and "value" in ab[m]:
            d = ab[m]
            assert d["value"] > 0 and d["exposed_stitch_ms_per_region"] >= 0 and d["record_bytes_per_rank_per_region"] > 0
            assert d["per_peer_link_GBs"] > 0 and abs(d["received_GBs_per_gpu"] - (n - 1) * d["per_peer_link_GBs"]) < 1e-6
            lo, hi = d["per_rank_ms_per_step_min_max"]
            assert 0 < lo <= hi and abs(hi - d["ms_per_step"]) < 1e-9      # the slowest rank IS the step
    a = out["analysis_only"]
    assert a["value"] > 0 and len(a["per_rank_ms_per_step_min_max"]) == 2


def test_gpus_flag_launches_the_ranks_itself():
    """`python3 bench.py --gpus 2 --steps 16 --warmup 4` -- the form the driver uses (here with --full), no torchrun around it: bench.py
    re-executes itself through torch.distributed.run with two ranks (on this one-GPU box both on GPU 0 over gloo, the
    SHARE_GPU testing aid) and exactly one JSON line with n_gpus == 2 comes out (round 2 parsed --gpus and ignored it)."""
    # (POLYCHASE_BENCH_STITCH=rccl: the chunked all-gather as the headline stitch -- gloo here -- and everything ONE N-GPU run must
    # return, on the same job)
    env = dict(os.environ, POLYCHASE_BENCH_SHARE_GPU="1", POLYCHASE_BENCH_STITCH="rccl", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "16", "--warmup", "4",
                        "--config", "c1", "--no-c3", "--no-breakdown"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 16 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["parallelism"] == "frame-shard x2"
    assert out["config"]["stitch"].startswith("rccl all_gather"), (out["config"]["stitch"], r.stderr[-2000:])
    _check_multi_gpu_keys(out, 2, peer=False, peer_wanted=False)


def test_peer_stitch_selftest_three_ranks_with_logs_of_different_sizes():
    """distributed.PeerLogStitch alone, three processes on GPU 0: every rank reads back every rank's bytes, twice (the slot
    size must be agreed: each rank's log has its own length -- the first version used the local length and wrote to the
    wrong offsets of the peers' buffers)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", os.path.join(ROOT, "tools", "peer_stitch_selftest.py")],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


def test_four_ranks_push_on_three_streams():
    """The stitch of more than four ranks deals the peers onto three copy streams; here four ranks on GPU 0 are told to
    (POLYCHASE_PEER_PUSH_STREAMS=3): every rank must still end up with every rank's records (asserted inside bench.py)."""
    env = dict(os.environ, POLYCHASE_BENCH_SHARE_GPU="1", POLYCHASE_PEER_PUSH_STREAMS="3", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--steps", "16", "--warmup", "4",
                        "--config", "c1", "--no-c3", "--no-breakdown"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["config"]["stitch"].startswith("xgmi peer copies")
    _check_multi_gpu_keys(out, 4, peer=True, peer_wanted=True)


def test_gpus_flag_fails_loudly_without_enough_gpus():
    """Without the testing aid a one-GPU box must refuse --gpus 2 instead of measuring one GPU and labelling it two."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has two GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "POLYCHASE_BENCH_SHARE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "needs 2 GPUs" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_c4_label_of_the_nested_4k_block_with_two_ranks():
    """`bench.py --gpus N` carries the 4K configuration as C4's per-rank workload: the nested block must say so (frames
    per GPU, halo) and hold both stitches as well.  Two ranks on one GPU (testing aid), few steps."""
    env = dict(os.environ, POLYCHASE_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "8", "--warmup", "2",
                        "--no-breakdown", "--no-arith-modes"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    c4 = out["c3"]
    assert c4["n_gpus"] == 2 and c4["config"]["workload"].startswith("C4 3840x2160 2400-frame clip frame-sharded across 2")
    assert c4["config"]["c4_frames_per_gpu_at_8"] == 300 and c4["config"]["halo_frames_per_side"] == 8
    assert "rccl" in c4["stitch_ab"] and c4["analysis_only"]["value"] > 0
    # the default stitch -- each rank maps the other's receive buffer through HIP IPC and pushes its pieces with device-to-device
    # copies (distributed.PeerLogStitch; here both buffers live on GPU 0) -- and what ONE N-GPU run must return, headline and nested
    assert out["config"]["stitch"].startswith("xgmi peer copies"), (out["config"]["stitch"], r.stderr[-2000:])
    _check_multi_gpu_keys(out, 2, peer=True, peer_wanted=True, arith_modes=False)
    _check_multi_gpu_keys(c4, 2, peer=True, peer_wanted=True, arith_modes=False, top=False)


def test_one_gpu_line_carries_roofline_counters_arith_modes_and_c5():
    """the driver's own command on one GPU with --full: roofline = the HBM block with counters measured in the run (rocprofv3 is on the
    box), valu_roofline beside it with both ceilings, the other arithmetic mode, and the C5 end-to-end block"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "POLYCHASE_ARITH")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                        "--no-end-to-end"], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    for blk in (out, out["c3"]):
        rf = blk["roofline"]
        assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / 8000.0) < 1e-12
        assert 0.005 < rf["frac"] < 0.05
        assert blk["config"]["arith"] == "opencv_x86" and blk["arith_modes"]["canonical"]["value"] > 0
        v = blk["valu_roofline"]
        assert v["bound"] == "valu" and v["frac_of_nominal_peak"] < v["frac_of_measured_peak"] <= 1.0
        # counters: measured by the run itself where rocprofv3 works (a pass that hangs is killed and the committed profile is
        # used instead: the line then says so)
        assert rf["traffic"] > rf["algorithmic_bytes_per_launch"], rf
        assert rf["counters_measured_in_run"] in (True, False) and v["counters_measured_in_run"] == rf["counters_measured_in_run"]
        import shutil
        if not shutil.which("rocprofv3"):
            assert rf["counters_measured_in_run"] is False
    assert out["c3"]["steps"] == 20
    c5 = out["c5"]
    assert "error" not in c5, c5
    pe = c5["pose_error_vs_cpu_reference"]
    assert pe["sampled_frames"] >= 10 and pe["rotation_rad_max"] <= 1e-4 and pe["translation_rel_max"] <= 1e-4
    assert c5["tracking_fps"] > 100 and c5["refinement_seconds"] < 10


def test_plain_line_times_exactly_the_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full): one region of exactly --steps steps, the headline fields and nothing measured beside them;
    --dump-outputs writes the last timed step's records, and a second run with the same arguments writes the same arrays."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "POLYCHASE_ARITH")}
    runs = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "12", "--warmup", "3",
                            "--dump-outputs", str(d)], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
        runs.append((json.loads(lines[0]), d))
    out, d0 = runs[0]
    assert out["metric"] == "optical-flow frames/sec" and out["unit"] == "frames/s" and out["higher_is_better"] is True
    assert out["steps"] == 12 and out["config"]["timed_regions"] == 1 and out["dtype"]
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"c3", "c5", "roofline", "arith_modes", "cpu_baseline", "end_to_end", "hard_content", "host"} & set(out)
    import numpy as np
    names = sorted(p.name for p in d0.iterdir())
    assert "keypoints.npy" in names and any(n.endswith("_xy.npy") for n in names)
    assert names == sorted(p.name for p in runs[1][1].iterdir())
    for n in names:
        a, b = np.load(d0 / n), np.load(runs[1][1] / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert len(np.load(d0 / "keypoints.npy")) > 0
