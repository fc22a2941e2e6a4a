"""bench.py prints ONE JSON line with the driver's contract (metric / value / unit / n_gpus / steps / warmup / ms_per_step / dtype / config /
roofline / cpu_baseline): a small run of every workload switch, so that a change to the engine cannot silently break the line the
driver parses.  A plain run measures the headline only; --full adds the CPU baseline, the roofline, the stage table, the point-only step
and the host-to-host pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    """one bench.py run -> its JSON line (a test that needs more than the headline passes --full)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_default_workload_line():
    d = _run("--pairs", "8", "--steps", "3", "--warmup", "1", "--cpu-pairs", "2", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "pairs/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "fp16"
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["matches_mean"] > 50
    # the default workload is the reference's keyframe step: PLNet with lines and junctions (map_builder.cc:85-86)
    assert d["config"]["detector"] == "plnet" and d["config"]["lines_mean"] >= 50 and d["config"]["junctions_mean_left"] >= 50
    assert d["config"]["points_only_pairs_per_s"] > d["value"]
    assert "plnet_stage1" in d["stages"] and "plnet_s0_decode" in d["stages"]
    rf = d["roofline"]
    assert rf["bound"] in ("mfma", "hbm") and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500.0
    assert 0.0 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["traffic"] is None or rf["traffic"] > 0
    # the line audits itself: the whole step against the matrix peak, every stage against its own roof, and counter-derived numbers only
    # from profiles taken on the kernel sources this run executes
    assert 0.0 < rf["step_frac"] < rf["frac"] < 1.0 and rf["step_gflop"] > 100 * 8          # >= 112 GFLOP per pair
    for k in ("lg_gemm", "lg_attention", "conv3x3_cin64", "conv3x3_cin128"):
        assert d["stages"][k]["bound"] == "mfma" and 0.0 < d["stages"][k]["frac"] < 1.0
    assert d["stages"]["simple_nms"]["bound"] == "hbm" and 0.0 < d["stages"]["simple_nms"]["frac"] < 1.0
    from airslam_amd.build import csrc_sha
    for what, val in (("traffic", rf["traffic"]), ("mfma_util", rf["mfma_util_counters"])):
        age = rf["counters_age"][what]
        if age is None:
            assert val is None
            continue
        assert age["tree_csrc_sha"] == csrc_sha() and age["stale"] == (age["profile_csrc_sha"] != age["tree_csrc_sha"])
        assert (val is None) == age["stale"], f"{what}: a counter-derived number must be reported exactly when its profile was taken on this tree's kernels"
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "pairs/s" and cb["value"] > 0 and cb["cores"] >= 1 and "sample" in cb
    assert cb.get("parity_ok", True) is True
    # the same step host to host rides along (pinned host images in, everything the step produced back in pinned host memory, copies on their own streams)
    hh = d["host_to_host"]
    assert hh["pairs_per_s"] > 0 and hh["h2d_bytes_per_step"] == 2 * 8 * 752 * 480 and hh["d2h_bytes_per_step"] > 2 * 8 * 200 * 259 * 4 and hh["matches_mean_last_step"] > 50
    assert abs(hh["ratio_to_resident"] - hh["pairs_per_s"] / d["value"]) < 1e-9
    assert len(d["host"]["queue_ms_per_step_per_rank"]) == 1 and 0 < d["host"]["queue_ms_per_step_per_rank"][0] < d["ms_per_step"] * 1.5
    assert d["host"]["cores_per_rank"] == [None]       # one rank: nothing to share


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline alone; --dump-outputs writes what the last timed step computed, the same on every run with
    the same arguments, and what a --full run's timed steps computed too"""
    args = ("--pairs", "8", "--steps", "3", "--warmup", "1")
    d = _run(*args, "--dump-outputs", str(tmp_path / "a"))
    assert d["unit"] == "pairs/s" and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "fp16" and d["higher_is_better"] is True
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"] and d["config"]["matches_mean"] > 50
    assert d["roofline"] is None and d["cpu_baseline"] is None and "stages" not in d and "host_to_host" not in d
    assert "points_only_pairs_per_s" not in d["config"]
    _run(*args, "--dump-outputs", str(tmp_path / "b"))
    _run(*args, "--dump-outputs", str(tmp_path / "c"), "--full", "--cpu-pairs", "0", "--io-steps", "0")
    names = sorted(os.listdir(tmp_path / "a"))
    assert "features_left.npy" in names and "match_index.npy" in names and "lines.npy" in names and "junctions_left.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 * 10**6
    for f in names:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, np.load(tmp_path / "b" / f)) and np.array_equal(a, np.load(tmp_path / "c" / f)), f
    n = np.load(tmp_path / "a" / "n_matches.npy")
    assert n.shape == (8,) and abs(n.mean() - d["config"]["matches_mean"]) < 1e-6
    assert np.array_equal(np.load(tmp_path / "a" / "pair_index.npy"), np.arange(8))


def test_two_steps_in_flight_line():
    """--inflight 2: consecutive steps alternate between two contexts; the line says so, and the run itself checks that both contexts return the same matches"""
    d = _run("--pairs", "8", "--steps", "4", "--warmup", "1", "--cpu-pairs", "0", "--io-steps", "0", "--inflight", "2", "--full")
    assert d["config"]["steps_in_flight"] == 2 and "steps_in_flight_note" in d["config"] and d["steps"] == 4
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"] and d["config"]["matches_mean"] > 50
    assert d["roofline"]["launches"] == 4 and 0.0 < d["roofline"]["frac"] < 1.0


def test_io_host_line():
    """--io host: `value` = the host-to-host rate (anchor: the reference copies in and out inside every infer(), src/plnet.cpp:231,237), the resident rate beside it"""
    d = _run("--pairs", "8", "--steps", "3", "--warmup", "1", "--cpu-pairs", "0", "--io", "host", "--io-steps", "6")
    assert d["value"] == d["host_to_host"]["pairs_per_s"] and d["steps"] == 6 and d["value_resident"] > 0 and "HOST memory" in d["config"]["workload"]
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["host_to_host"]["pcie_gbs"]["h2d"] > 0 and d["host_to_host"]["pcie_gbs"]["d2h"] > 0


@pytest.mark.parametrize("args", [("--matcher", "superglue", "--pairs", "4"), ("--detector", "superpoint", "--pairs", "4"),
                                  ("--plnet-host", "--pairs", "2"), ("--workload", "loop", "--pairs", "8")],
                         ids=["superglue", "superpoint", "plnet_host", "loop"])
def test_side_workload_lines(args):
    d = _run(*args, "--steps", "2", "--warmup", "1", "--cpu-pairs", "0")
    assert d["unit"] == "pairs/s" and d["value"] > 0 and d["steps"] == 2 and "workload" in d["config"]
    if "--plnet-host" in args:
        assert d["config"]["lines_last_frame"] >= 50          # the structured synthetic line head: lines survive the reference's thresholds
    elif "superpoint" in args:
        assert d["config"]["detector"] == "superpoint" and "lines_mean" not in d["config"] and d["config"]["matches_mean"] > 50


def test_track_workload_line():
    """the normal-frame step (map_builder.cc:94-101) — by default what the shipped configs run on a normal frame: SuperPoint (use_superpoint: 1,
    feature_detector.cc:36-41) + LightGlue against the last keyframe; --detector plnet is the use_superpoint: 0 form (points + lines)"""
    d = _run("--workload", "track", "--pairs", "8", "--steps", "3", "--warmup", "1")
    assert d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["value"] > 0 and "tracked frames" in d["metric"] and "SuperPoint" in d["metric"]
    assert d["config"]["detector"] == "superpoint" and d["config"]["matches_mean"] > 50 and "lines_mean" not in d["config"]
    d = _run("--workload", "track", "--detector", "plnet", "--pairs", "8", "--steps", "3", "--warmup", "1")
    assert d["config"]["matches_mean"] > 50 and d["config"]["lines_mean"] >= 50 and "junctions_mean_left" not in d["config"] and "PLNet" in d["metric"]
    assert d["cpu_baseline"] is None if "cpu_baseline" in d else True


def test_seq_workload_line():
    """--workload seq (BASELINE configs[3]): S sequences driven as map_builder.cc:83-141 drives the front end — a short run of the batched driver and of the
    one-call driver; the schedule contains keyframes, normal frames and (scenes of 10 frames) promotions"""
    d = _run("--workload", "seq", "--sequences", "3", "--frames", "34", "--warmup", "2", "--scene-len", "10", "--cpu-pairs", "3", "--min-num-match", "100",
             "--full")
    assert d["unit"] == "frames/s" and d["steps"] == 32 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["value"] > 0
    assert abs(d["value"] - 3 * 32 / (d["ms_per_step"] * 32 * 1e-3)) <= 1e-6 * d["value"]
    sch = d["config"]["schedule"]
    # (--min-num-match 100: a normal frame whose temporal matches fall below 100 is promoted — the synthetic matcher finds 60-100 even across a scene change)
    assert sch["frames"] == 3 * 32 and sch["keyframes"] >= 6 and sch["promotions"] >= 1 and sch["normal_frames"] >= 30 and sch["temporal_matches_mean"] >= 40
    assert sch["dropped_before_init"] == 0
    # default driver: the C++ lock-step loop (include/airfe_seq.h); 3 sequences = one group
    assert d["config"]["gather_every_frames"] == 8 and d["config"]["gathers"] == 4 and "airfe_seq.h" in d["config"]["driver"] and d["config"]["groups"] == 1
    lat = d["latency_ms_per_time_step"]
    assert 0 < lat["p50"] <= lat["p99"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "frames/s" and cb["value"] > 0
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and 0.0 < rf["step_frac"] < 1.0 and 0.0 < rf["frac"] < 1.0 and rf["step_gflop"] > 50      # (frac: the bracketed pass, events included)
    ws = d["host"]["wall_split_ms_per_step"]
    assert ws["host_syncs"] >= 1.0 and ws["queue_device_work"] > 0 and ws["wait_for_device"] > 0 and ws["host_side_of_the_loop"] >= 0
    # the same frames through round 5's Python driver and through two pipelined groups of the C++ one: the same schedule
    dp = _run("--workload", "seq", "--sequences", "4", "--frames", "34", "--warmup", "2", "--scene-len", "10", "--cpu-pairs", "0", "--min-num-match", "100", "--seq-driver", "python")
    dn = _run("--workload", "seq", "--sequences", "4", "--frames", "34", "--warmup", "2", "--scene-len", "10", "--cpu-pairs", "0", "--min-num-match", "100")
    assert "BatchedSequences" in dp["config"]["driver"] and dn["config"]["groups"] == 2 and "NativePipeline" in dn["config"]["driver"]
    assert dp["config"]["schedule"] == dn["config"]["schedule"]
    assert dn["config"]["gathers"] == 2 * 4
    d1 = _run("--workload", "seq", "--sequences", "1", "--frames", "24", "--warmup", "2", "--scene-len", "10", "--cpu-pairs", "0")
    assert "SequenceFrontEnd" in d1["config"]["driver"] and d1["config"]["schedule"]["frames"] == 22 and d1["value"] > 0


def test_gpus_2_launches_two_ranks_itself(monkeypatch):
    """`python bench.py --gpus 2` without a launcher must start two ranks (torch.distributed.run underneath) and say so: here both ranks share
    GPU 0 and talk over gloo (RCCL refuses two ranks on one device); the gather of the match lists to rank 0 runs every step."""
    monkeypatch.setenv("AIRFE_DIST_BACKEND", "gloo")
    monkeypatch.setenv("AIRFE_ONE_DEVICE", "1")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    d = _run("--gpus", "2", "--pairs", "4", "--steps", "2", "--warmup", "1", "--cpu-pairs", "0", "--no-profile")
    assert d["n_gpus"] == 2 and d["collective"]["ranks"] == 2 and d["collective"]["backend"] == "gloo"
    assert abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]


def test_two_ranks_report_their_host_time_on_their_own_cores(monkeypatch):
    """Host-side readiness for the 8-rank run: one process per GPU queues a few hundred launches per step from one host thread.  Every local rank
    is given its own share of the cores (airslam_amd.dist.pin_rank_to_cores) and the line carries each rank's queueing time per step (wall and CPU), so that the
    driver's 8-GPU run explains its own efficiency.  Two ranks on this box share GPU 0 over gloo: the DEVICE is the bottleneck then — launch calls wait on a full
    queue, in wall time and (the runtime spins) in CPU time: 1.25 ms against 0.27 ms per step measured, profiles/r06_two_ranks_one_gpu.txt — so the times of the two
    runs are reported, not compared; what is asserted is that every rank reports, and that the ranks' core shares are disjoint."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = ("--pairs", "16", "--steps", "12", "--warmup", "3", "--cpu-pairs", "0", "--no-profile", "--io-steps", "0")
    one = _run("--gpus", "1", *common)
    monkeypatch.setenv("AIRFE_DIST_BACKEND", "gloo")
    monkeypatch.setenv("AIRFE_ONE_DEVICE", "1")
    two = _run("--gpus", "2", *common)
    h1, h2 = one["host"], two["host"]
    assert len(h1["queue_ms_per_step_per_rank"]) == 1 and len(h2["queue_ms_per_step_per_rank"]) == 2 and len(h2["queue_cpu_ms_per_step_per_rank"]) == 2
    assert 0 < h1["queue_cpu_ms_per_step_per_rank"][0] <= h1["queue_ms_per_step_per_rank"][0] * 1.05 + 0.05
    assert h1["queue_cpu_ms_per_step_per_rank"][0] < 0.25 * one["ms_per_step"] + 0.3          # queueing a step costs the host a fraction of what the device needs for it
    c = h2["cores_per_rank"]
    if c[0] is not None and c[1] is not None:          # pinned: disjoint shares
        assert c[0][1] < c[1][0] or c[1][1] < c[0][0], c
    from gpu_common import diag
    diag("two_ranks_one_gpu", one_rank=str(h1), two_ranks=str(h2), ms_per_step=str((one["ms_per_step"], two["ms_per_step"])))


def test_frontend_workload_line():
    """the whole per-keyframe front end, device-resident: rectify -> PLNet x2 -> LightGlue -> AssignPointsToLines x2 -> MatchLines -> BoW"""
    d = _run("--workload", "frontend", "--pairs", "8", "--steps", "3", "--warmup", "1", "--full")
    assert d["unit"] == "stereo keyframes/s" and d["n_gpus"] == 1 and d["value"] > 0 and "AssignPointsToLines" in d["metric"]
    assert d["config"]["matches_mean"] > 30 and d["config"]["lines_mean"] >= 30
    assert d["config"]["points_on_lines_mean_left"] > 50 and d["config"]["stereo_line_matches_mean"] >= 3
    for st in ("rectify", "line_assoc", "bow", "plnet_stage1", "lg_gemm"):
        assert st in d["stages"], st


def test_b1_latency_line():
    """--workload b1: one stereo keyframe at a time through the batch-1 host API, latency percentiles"""
    d = _run("--workload", "b1", "--steps", "20", "--warmup", "3")
    assert d["unit"] == "pairs/s" and d["steps"] == 20 and "latency" in d["metric"] and d["call_forms_agree"] is True
    lat = d["latency_ms"]
    assert lat["pair"]["p50"] > 0 and lat["pair"]["p99"] >= lat["pair"]["p50"] and abs(d["value"] - 1e3 / lat["pair"]["p50"]) < 1e-6 * d["value"]
    assert d["config"]["matches_mean"] > 50 and d["config"]["lines_mean_left"] >= 50
    # the one-call keyframe is the headline; the reference's two- and three-call forms of the same keyframe are beside it
    # (timing relations with slack: a test must not go red on a noisy box; the measured gaps are 20-45 %, see profiles/r04_bench_b1_latency.json)
    assert lat["three_calls"]["pair"]["p50"] * 1.1 > lat["two_calls"]["pair"]["p50"] and lat["two_calls"]["pair"]["p50"] * 1.1 > lat["pair"]["p50"] > 0
    assert lat["tracked_frame"]["two_calls"]["p50"] * 1.1 > lat["tracked_frame"]["one_call"]["p50"] > 0
    assert lat["keyframe_with_temporal_match"]["keyframe_call_plus_match_call"]["p50"] * 1.1 > lat["keyframe_with_temporal_match"]["one_call"]["p50"] > 0
