"""bench.py / __graft_entry__ contract checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"}
LINE_LIMIT = 6144  # the driver's record keeps the last 8 KB of stdout: the LAST line must fit with room to spare


def records(stdout):
    """(driver line, full record): the LAST stdout line is the driver's JSON object (<= 6 KB); everything measured is in
    the earlier line prefixed 'DETAIL ' (and in bench_detail.json)."""
    lines = stdout.splitlines()
    driver = [ln for ln in lines if ln.startswith("{")]
    detail = [ln for ln in lines if ln.startswith("DETAIL {")]
    assert len(driver) == 1 and len(detail) == 1 and lines[-1] == driver[0]
    assert len(driver[0].encode()) < LINE_LIMIT, len(driver[0])
    line, full = json.loads(driver[0]), json.loads(detail[0][len("DETAIL "):])
    assert REQUIRED <= set(line) and REQUIRED <= set(full)
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert line[k] == full[k]
    assert abs(line["value"] - full["value"]) <= 1e-4 * full["value"]  # (the line rounds to 5 significant digits)
    return line, full


def test_algorithmic_byte_formulas_match_the_survey():
    """bytes = nnzb (8 b^2 + 4) + 4 (n + 1) + 16 r b n; 100k grid: 122.7 MB ("123.1" with MB = 1e6)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.spmm_bytes(100000, 687000, 3, 5) == 687000 * 132 + 4 * 100001 + 320 * 100000 == 123084004
    assert bench.spmm_bytes(2500, 12398, 3, 5) == 2446540  # sphere2500: 2.44 MB
    assert bench.hess_bytes(100000, 687000, 3, 5) == 687000 * 132 + 4 * 100001 + 100000 * (6 * 160 + 72)
    assert bench.HBM_PEAK_GBS == 8000.0


def test_compact_line_of_a_committed_full_record_fits_the_drivers_record():
    """bench.compact_line on the largest full record committed so far (round 5's 24 KB line, which the driver could not
    parse): below 6 KB, the contract's keys present, floats rounded to 5 significant digits."""
    import glob
    sys.path.insert(0, ROOT)
    import bench
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[56]_v*_bench.json")))
    assert files
    for f in files:
        full = json.load(open(f))
        if "quality" not in full:
            continue  # (already a compact line)
        text = bench.compact_line(full)
        assert len(text.encode()) < LINE_LIMIT and "\n" not in text
        line = json.loads(text)
        assert REQUIRED <= set(line) and line["roofline"]["frac"] > 0
        assert (line["cpu_baseline"] is None) == (full["cpu_baseline"] is None)
        assert abs(line["value"] - full["value"]) <= 1e-4 * full["value"]
    # a pathological record (long strings everywhere) still fits: optional groups are dropped
    full = json.load(open(files[-1]))
    if "quality" in full:
        full["config"]["workload"] = "w" * 300
        full["also"] = {"sphere2500": {"it_per_s": 1.0, "us_per_product": 1.0, "precond_used": "x" * 3000}}
        assert len(bench.compact_line(full).encode()) < LINE_LIMIT


def test_entry_points_exist():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    assert callable(g.build) and callable(g.smoke)


def test_dump_outputs_writes_the_agents_results_within_the_size_limit(tmp_path, monkeypatch):
    """bench.dump_outputs (--dump-outputs DIR): per agent its iterate (float64 tiles in the caller's pose order) and its
    solver result; beyond the size limit a seeded, sorted sample of poses with their indices, the same rows every run."""
    import types
    import torch
    sys.path.insert(0, ROOT)
    import bench

    class Agent:
        def __init__(self, n, seed):
            self.X = torch.tensor(np.random.default_rng(seed).standard_normal((n, 4, 5)))
            self.last_result = types.SimpleNamespace(fInit=4.0, gradNormInit=3.0, fOpt=2.0, gradNormOpt=1.0, tcg_iterations=7,
                                                     rtr_iterations=3, rtr_accepted=2)

        def iterate_in_caller_order(self):
            return self.X

    agents = {0: Agent(3000, 0), 3: Agent(1000, 1)}
    bench.dump_outputs(str(tmp_path / "all"), agents, 1)
    for a, ag in agents.items():
        X = np.load(str(tmp_path / "all" / ("agent%d_X.npy" % a)))
        assert X.dtype == np.float64 and np.array_equal(X, ag.X.numpy())
        assert np.load(str(tmp_path / "all" / ("agent%d_result.npy" % a))).tolist() == [4.0, 3.0, 2.0, 1.0, 7.0, 3.0, 2.0]
    assert sorted(os.listdir(str(tmp_path / "all"))) == ["agent0_X.npy", "agent0_result.npy", "agent3_X.npy",
                                                        "agent3_result.npy"]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256 * 1024)  # (the iterates are 640 KB)
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), agents, 1)
        assert sum(f.stat().st_size for f in (tmp_path / run).iterdir()) <= 256 * 1024
    for a, ag in agents.items():
        poses = np.load(str(tmp_path / "s1" / ("agent%d_X_poses.npy" % a)))
        assert poses.dtype == np.float64 and len(poses) > 0 and np.all(np.diff(poses) > 0)
        X = np.load(str(tmp_path / "s1" / ("agent%d_X.npy" % a)))
        assert np.array_equal(X, ag.X.numpy()[poses.astype(np.int64)])
        assert np.array_equal(X, np.load(str(tmp_path / "s2" / ("agent%d_X.npy" % a))))


@pytest.mark.gpu
def test_bench_prints_one_valid_json_line(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "grid:12x10x6", "--steps", "2",
                        "--warmup", "1", "--settle", "2", "--cpu-budget-s", "3", "--spmm-reps", "20",
                        "--dump-outputs", str(tmp_path), "--full"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line, j = records(p.stdout)
    # --dump-outputs: the one agent's iterate after the last timed step (720 poses, d = 3, r = 5) and its solver result
    X, res = np.load(str(tmp_path / "agent0_X.npy")), np.load(str(tmp_path / "agent0_result.npy"))
    assert X.dtype == np.float64 and X.shape == (720, 4, 5) and np.all(np.isfinite(X))
    assert res.shape == (7,) and res[2] <= res[0] and res[4] > 0
    assert os.path.exists(os.path.join(ROOT, "bench_detail.json"))
    # ---- the driver's line: headline keys, roofline of the timed kernel, the reference-configuration pair
    assert line["metric"] == "rbcd_iterations_per_sec" and line["n_gpus"] == 1 and line["dtype"] == "f64"
    lrf, lcb = line["roofline"], line["cpu_baseline"]
    assert lrf["bound"] == "hbm" and lrf["peak"] == 8000.0 and lrf["unit"] == "GB/s" and lrf["achieved"] > 0
    assert abs(lrf["frac"] - lrf["achieved"] / lrf["peak"]) < 1e-4 and lrf["kernel"].startswith("k_rtr_persist<3,5,")
    assert lrf["frac_own_bytes"] > 0 and lrf["streamed_bytes"] > 0 and lrf["traffic"] is None
    names = [k["kernel"].split()[0] for k in lrf["kernels"]]
    assert names[:2] == ["k_tcg_update_span", "k_ml_restrict"] and names[2] in ("k_ml_coarse_prolong", "k_dense_sym_apply")
    assert names[3] in ("k_ml_post", "k_ml_post_ap") and len(names) == 4
    assert all(k["us"] > 0 and k["streamed_bytes"] > 0 and k["algorithmic_bytes_fp64"] >= k["streamed_bytes"] and
               abs(k["frac"] - k["streamed_bytes"] / k["us"] / 1e3 / 8000.0) < 1e-3 * k["frac"] for k in lrf["kernels"])
    assert lcb["kind"] == "port" and lcb["cores"] >= 1 and lcb["value"] > 0 and lcb["unit"] == "it/s" and len(lcb["sample"]) <= 200
    assert lcb["seconds_per_sweep"] > 0 and lcb["factorisation_seconds"] > 0 and lcb["tcg_iterations"] >= 0 and lcb["host_cores"] >= 1
    assert lcb["gpu_same_work"]["seconds_per_sweep"] > 0 and lcb["gpu_same_work"]["preconditioners"]
    assert "gpu_over_cpu_same_work" not in lcb
    assert "workload" in line["config"] and "model" not in line["config"] and line["products_per_step"] > 0
    assert line["time_to_tolerance_ms"] > 0 and line["hierarchy_setup_ms"] > 0 and line["us_per_product"] > 0
    # ---- the full record
    assert j["metric"] == "rbcd_iterations_per_sec" and j["unit"] == "it/s" and j["higher_is_better"] is True
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["dtype"] == "f64" and j["vs_baseline"] is None
    assert j["value"] > 0 and abs(j["value"] - 1e3 / j["ms_per_step"]) < 1e-6 * j["value"]
    assert "workload" in j["config"] and "model" not in j["config"]
    rf = j["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["achieved"] > 0
    assert rf["spmm_only"]["frac"] > 0
    # the headline describes the kernel the timed loop launched: name, time and rate belong together.  A 720-pose block is
    # in the latency regime: its solve is ONE launch of the persistent kernel, and the tCG-step kernel of the multi-launch
    # scheme (frac = rotating / HBM-only, warm beside it) is reported next to it
    assert rf["spmm_storage_selected"] == "plain" and rf["kernel"].startswith("k_rtr_persist<3,5,")
    assert abs(rf["achieved"] - rf["bytes_per_launch"] / rf["avg_launch_us"] / 1e3) < 1e-9 * rf["achieved"]
    assert rf["products_per_launch"] > 0
    assert abs(rf["us_per_product"] - rf["avg_launch_us"] / rf["products_per_launch"]) < 1e-9 * rf["us_per_product"]
    ml = rf["multi_launch_kernel"]
    assert ml["kernel"].startswith("k_tcg_hess_span<3,5,4,0>") and ml["warm"]["frac"] > 0
    assert abs(ml["achieved"] - ml["bytes_per_launch"] / ml["avg_launch_us"] / 1e3) < 1e-9 * ml["achieved"]
    assert abs(ml["warm"]["achieved"] - ml["bytes_per_launch"] / ml["warm"]["avg_launch_us"] / 1e3) < 1e-9 * ml["achieved"]
    # (one-launch solve: frac = MODELLED HBM bytes of the launch over its time -- Q and the vectors live in registers / LDS --;
    # the figure comparable with the multi-launch kernel is effective_algorithmic_*: products x the step's bytes)
    assert abs(rf["effective_algorithmic_bytes"] - rf["products_per_launch"] * ml["bytes_per_launch"]) < 1e-6 * rf["bytes_per_launch"] * 1e3
    assert abs(rf["effective_algorithmic_GBs"] - rf["effective_algorithmic_bytes"] / rf["avg_launch_us"] / 1e3) < 1e-9 * rf["effective_algorithmic_GBs"]
    assert rf["bytes_per_launch"] < ml["bytes_per_launch"] and rf["traffic"] is None
    # the TIMED kernel's own bytes are always printed, whichever storage it reads
    assert rf["stored_bytes_per_launch"] > 0 and rf["frac_own_bytes"] > 0 and "storage" in rf
    assert abs(rf["frac_own_bytes"] - rf["stored_bytes_per_launch"] / rf["avg_launch_us"] / 1e3 / 8000.0) < 1e-9
    assert rf["symmetric_storage"] is None  # (this small block cannot run the symmetric kernels: 4 lane groups per pose)
    assert j["products_per_step"] > 0 and j["time_to_tolerance_ms"] > 0 and j["products_to_tolerance"] > 0
    # ... and repeated inside `config`, which the driver's parsed record keeps
    assert j["config"]["time_to_tolerance_ms"] == j["time_to_tolerance_ms"]
    assert "time_to_tolerance_ms = %.3f" % j["time_to_tolerance_ms"] in j["config"]["local_solver"]
    assert j["config"]["products_per_step"] == j["products_per_step"]
    assert [k["kernel"].split()[0] for k in rf["kernels"]] == names
    # fp64 everywhere on this small block: the streamed bytes ARE the algorithmic bytes, up to the symmetric storage
    assert all(k["streamed_bytes"] <= k["algorithmic_bytes_fp64"] and k["frac"] <= k["frac_fp64_equivalent"] + 1e-12
               for k in rf["kernels"])
    assert all(k["avg_launch_us"] > 0 for k in rf["kernels"])
    # the once-per-Q cost of the preconditioner beside the time to tolerance (the reference factors inside its first solve)
    assert j["hierarchy_setup_ms"] > 0 and j["hierarchy_values_only_ms"] > 0
    assert abs(j["time_to_tolerance_incl_setup_ms"] - (j["time_to_tolerance_ms"] + j["hierarchy_setup_ms"])) < 1e-9
    assert j["config"]["hierarchy_setup_ms"] == j["hierarchy_setup_ms"]
    assert j["config"]["time_to_tolerance_incl_setup_ms"] == j["time_to_tolerance_incl_setup_ms"]
    assert rf["traffic_live"] is False
    cb = j["cpu_baseline"]  # reference configuration (exact factor, one core per agent) + the 1-core port beside it
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "it/s"
    # cpu_baseline.value is the pair from the SETTLED iterate every timed step restores ...
    assert "exact sparse factor" in cb["sample"] and "SETTLED" in cb["sample"] and cb["factorisation_seconds"] > 0
    same = cb["gpu_same_work"]  # the like-for-like pair: same 8 blocks, same iterate, same one sweep, on the GPU
    assert same["agents"] == 8 and same["value"] > 0 and same["gradnorm_after"] > 0 and cb["gradnorm_after"] > 0
    assert abs(cb["gpu_over_cpu_same_work"] - same["value"] / cb["value"]) < 1e-9 * cb["gpu_over_cpu_same_work"]
    assert len(same["tcg_iterations_per_agent"]) == 8 and len(cb["tcg_iterations_per_agent"]) == 8
    hs = same["hierarchy_setup_ms"]  # the GPU side's once-per-Q cost, per block
    assert len(hs["first_ms"]) == 8 and min(hs["first_ms"]) > 0 and min(hs["values_only_ms"]) > 0
    assert len(same["auto_rule"]) == 8 and all(a["state"] in ("jacobi", "trial", "additive") for a in same["auto_rule"])
    ini = cb["initial_iterate"]  # ... the pair from the benchmark's initial iterate under its own key
    assert ini["value"] > 0 and "SETTLED" not in ini["sample"] and ini["gpu_same_work"]["agents"] == 8
    assert len(ini["tcg_iterations_per_agent"]) == 8 and len(ini["gpu_same_work"]["tcg_iterations_per_agent"]) == 8
    port = cb["single_agent_port"]
    assert port["cores"] == 1 and port["value"] > 0 and port["rel_diff_fOpt_vs_device"] < 1e-6
    tt = j["quality"]["to_tolerance"]
    assert set(tt) == {"grid:12x10x6/auto", "grid:12x10x6/multilevel", "grid:12x10x6/additive", "grid:12x10x6/jacobi",
                       "grid:12x10x6/multilevel+fp32_dense_level",   # opt-in storage mode, beside the headline
                       "grid:12x10x6/multilevel+fp64_cycle_operators"}  # (the default's fp32 operator copies switched off)
    assert rf["multilevel"]["coarse_inverse_bits"] == 64  # the dense level of the headline configuration is fp64
    # the cycle's operator copies: fp32 only where the symmetric storage runs (blocks beyond the Infinity Cache), named in config
    assert rf["multilevel"]["cycle_operator_copy_bits"] == 64 and "fp64 copies" in j["config"]["cycle_storage"]
    assert "dense level (inverse, restricted residual) in fp64" in j["config"]["cycle_storage"]
    assert all("products" in v for v in tt.values())


@pytest.mark.gpu
def test_bench_plain_run_measures_the_headline_only(tmp_path):
    """Without --full a run sets up, settles, warms up, times its steps, dumps and prints: no roofline probe, CPU baseline or
    side measurement, and the steps compute bit for bit what a --full run's steps compute."""
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "grid:12x10x6", "--steps", "2", "--warmup", "1",
            "--settle", "2"]
    plain = subprocess.run(args + ["--dump-outputs", str(tmp_path / "plain")], capture_output=True, text=True, cwd=ROOT,
                           timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    line, j = records(plain.stdout)
    assert line["metric"] == "rbcd_iterations_per_sec" and line["unit"] == "it/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and j["value"] > 0 and abs(j["value"] - 1e3 / j["ms_per_step"]) < 1e-6 * j["value"]
    assert j["products_per_step"] > 0 and line["us_per_product"] > 0 and j["config"]["precond_used_in_timed_steps"]
    for k in ("roofline", "cpu_baseline", "also", "kitti_gnc", "time_to_tolerance_ms", "hierarchy_setup_ms",
              "gradnorm_before_step", "gradnorm_after_step"):
        assert j[k] is None and line.get(k) is None, k
    assert j["quality"]["to_tolerance"] is None and j["quality"]["cost_2f_trajectory"] == []
    full = subprocess.run(args + ["--dump-outputs", str(tmp_path / "full"), "--full", "--no-cpu-baseline",
                                  "--no-secondary", "--spmm-reps", "10"],
                          capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert full.returncode == 0, full.stderr[-2000:]
    _, jf = records(full.stdout)
    assert jf["roofline"] is not None and jf["gradnorm_after_step"] > 0
    assert jf["products_per_step"] == j["products_per_step"]
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full"))) and "agent0_X.npy" in names
    for f in names:
        assert np.array_equal(np.load(str(tmp_path / "plain" / f)), np.load(str(tmp_path / "full" / f))), f


@pytest.mark.gpu
def test_bench_default_invocation_fits_the_drivers_record():
    """The driver's own command with --full (python bench.py --gpus 1 --steps 20 --warmup 5 --full: the 100k-pose grid, every
    side measurement): the LAST stdout line
    is one JSON object below 6 KB carrying `roofline` (headline kernel, PMC traffic, streamed-byte fractions of every kernel
    of the iteration, the whole iteration) and `cpu_baseline`; BASELINE configs[4] (kitti_00 GNC) has its numbers; the
    default (fp32 cycle storage) and the fp64-cycle run need the same number of products to the tolerance."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--full"], capture_output=True, text=True, cwd=ROOT, timeout=1200)
    assert p.returncode == 0, p.stderr[-3000:]
    line, full = records(p.stdout)
    assert "100000 poses" in line["config"]["workload"] and line["config"]["agents"] == 1
    rf = line["roofline"]
    assert rf["kernel"].startswith("k_tcg_hess_sym<3,5,") and rf["storage"] == "symmetric" and 0.3 < rf["frac"] < 1.0
    assert rf["streamed_bytes"] < rf["bytes_per_launch"] and rf["frac_own_bytes"] < rf["frac"]
    assert rf["traffic"] > 0 and rf["traffic_live"] is False and rf["spmm"]["kernel"].startswith("k_spmm_sym<")
    assert rf["spmm"]["frac"] >= 0.30  # north_star: >= 30 % of the HBM roofline on the Q*X SpMM at 100k poses
    assert len(rf["kernels"]) == 4
    for k in rf["kernels"]:
        assert abs(k["frac"] - k["streamed_bytes"] / k["us"] / 1e3 / 8000.0) < 1e-3 * k["frac"]
        assert k["streamed_bytes"] <= k["algorithmic_bytes_fp64"] and k["traffic"] > 0
        assert abs(k["frac_traffic"] - k["traffic"] / k["us"] / 1e3 / 8000.0) < 1e-3 * k["frac_traffic"]
    it = rf["iteration"]
    assert it["launches"] == 6 and abs(it["us_per_product"] - line["us_per_product"]) < 1e-3 * it["us_per_product"]
    assert abs(it["frac"] - it["bytes"] / it["us_per_product"] / 1e3 / 8000.0) < 1e-3 * it["frac"]
    assert it["bytes"] == rf["streamed_bytes"] + sum(k["streamed_bytes"] for k in rf["kernels"])
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and len(cb["sample"]) <= 200
    assert cb["gpu_same_work"]["seconds_per_sweep"] > 0 and "gpu_over_cpu_same_work" not in cb
    kg = line["kitti_gnc"]  # BASELINE configs[4]: weight update (re-weighted Q rebuild) and GNC outer iteration, timed
    assert kg["ms_per_weight_update"] > 0 and kg["ms_per_inner_block"] > 0 and kg["updates"] >= 30
    assert abs(kg["ms_per_gnc_outer_iteration"] - (kg["ms_per_weight_update"] + kg["ms_per_inner_block"])) < 1e-3 * kg["ms_per_gnc_outer_iteration"]
    assert kg["total_ms"] > 0 and kg["cpu_seconds_per_gnc_outer_iteration"] > 0
    fk = full["kitti_gnc"]
    assert (fk["last"]["inliers"], fk["last"]["outliers"], fk["last"]["undecided"]) == (136, 25, 0)
    # the mixed-precision default against its fp64-cycle twin: same products to the tolerance
    tt = full["quality"]["to_tolerance"]
    a, b = tt["grid100k/multilevel"], tt["grid100k/multilevel+fp64_cycle_operators"]
    assert a["reached"] and b["reached"] and a["cycle_operator_copy_bits"] == 32 and b["cycle_operator_copy_bits"] == 64
    assert abs(a["products"] - b["products"]) <= 2, (a["products"], b["products"])
    assert abs(a["gradnorm"] - b["gradnorm"]) <= 1e-3 * b["gradnorm"]


@pytest.mark.gpu
def test_bench_secondary_workload_reports_per_product_cost_and_in_kernel_split():
    """`also.sphere2500` of the headline line (BASELINE's metric is quoted on sphere2500 as well): the fixed-work step rate,
    microseconds per Hessian-vector product and, for a one-launch solve, the in-kernel phase split of participant 0."""
    sys.path.insert(0, ROOT)
    import bench
    e = bench.secondary_single_agent("sphere2500", 5, "auto", 3, 1, 2)
    assert e["it_per_s"] > 0 and e["tcg_iterations_per_step"] > 0 and e["precond_used"] in ("additive", "multilevel", "jacobi")
    assert abs(e["us_per_product"] - 1e3 * e["ms_per_step"] / e["tcg_iterations_per_step"]) < 1e-6 * e["us_per_product"]
    ph = e["in_kernel_us_per_iteration"]  # sphere2500 is a one-launch solve
    assert ph is not None and ph["hessian_phase"] > 0 and ph["total"] < e["us_per_product"] * 1.5
    assert abs(ph["total"] - (ph["hessian_phase"] + ph["all_reduce_after_hessian"] + ph["update_phase"]
                              + ph["reductions_after_update"])) < 1e-9


@pytest.mark.gpu
def test_bench_loopback_runs_the_multi_agent_path_through_rccl():
    """bench.py --loopback: 4 agents on one GPU, every exchange and reduction through the library-owned 1-rank RCCL
    communicator (the N > 1 data path), same-colour agents solved concurrently, exchange time from device events."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "grid:12x10x8", "--steps", "2",
                        "--warmup", "1", "--settle", "1", "--loopback", "--agents-per-gpu", "4", "--no-cpu-baseline",
                        "--no-secondary", "--spmm-reps", "10", "--full"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line, j = records(p.stdout)
    assert line["roofline"] is not None and line["cpu_baseline"] is None and line["config"]["agents"] == j["config"]["agents"]
    assert j["config"]["agents"] == 4 and "RCCL" in j["config"]["schedule"] and "loop-back" in j["config"]["schedule"]
    assert j["quality"]["exchange_ms_per_step_rank0"] > 0 and j["value"] > 0
    assert j["quality"]["cost_2f_after_step"] < j["quality"]["cost_2f_trajectory"][0]
    # coupled blocks under `auto`: the selection is brought to its steady state before the timed steps
    assert j["config"]["selection_sweeps_before_timing"] >= 0
    assert set(j["config"]["precond_used_in_timed_steps"]) <= {"jacobi", "additive", "multilevel"}


def test_bench_default_steps_time_more_than_a_second():
    """The default --steps keeps the timed region above one second at the headline workload's ~5 ms per step (the
    driver's utilisation sampling needs that long to see the run)."""
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse_args()
    finally:
        sys.argv = old
    assert a.steps >= 200 and a.gpus == 1 and a.warmup >= 1


def test_bench_side_measurements_are_opt_in():
    """--full is off by default; the line of a run without it carries the headline keys and null in place of the side
    measurements."""
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
        assert bench.parse_args().full is False
        sys.argv += ["--full"]
        assert bench.parse_args().full is True
    finally:
        sys.argv = old
    out = {"metric": "rbcd_iterations_per_sec", "value": 250.0, "unit": "it/s", "n_gpus": 1, "steps": 3, "warmup": 1,
           "ms_per_step": 4.0, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
           "data": "synthetic", "products_per_step": 30.0, "gradnorm_before_step": None, "gradnorm_after_step": None,
           "config": {"workload": "w", "agents": 1, "precond": "auto", "precond_used_in_timed_steps": ["additive"]},
           "roofline": None, "cpu_baseline": None, "also": None, "kitti_gnc": None,
           "quality": {"us_per_tcg_iteration_rank0": 133.3, "cost_2f_trajectory": [], "to_tolerance": None}}
    line = json.loads(bench.compact_line(out))
    assert REQUIRED <= set(line) and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["value"] == 250.0 and line["ms_per_step"] == 4.0 and line["us_per_product"] == 133.3


@pytest.mark.gpu
def test_bench_multi_gpu_branch_runs_at_world_size_one():
    """The N > 1 branch of bench.py executed on ONE device exactly as the driver launches it for N > 1 (python -m
    torch.distributed.run ... bench.py --gpus 1), with --dist: init_process_group("nccl") = RCCL, the library's communicator
    taken from the process group (DeviceComm.from_torch_distributed), dist.barrier around the timed region, the
    all-reduces of work and time, 2 agents per GPU, every exchange a grouped RCCL self send / recv timed by device events."""
    port = 29500 + (os.getpid() % 400)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dist", "--workload",
           "grid:12x10x8", "--steps", "3", "--warmup", "1", "--settle", "1", "--no-cpu-baseline", "--no-secondary",
           "--spmm-reps", "10", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line, j = records(p.stdout)
    assert line["roofline"] is not None and line["cpu_baseline"] is None and line["config"]["agents"] == j["config"]["agents"]
    assert j["config"]["dist_backend"] == "nccl" and j["n_gpus"] == 1 and j["config"]["agents"] == 2
    assert j["config"]["agents_per_gpu"] == 2 and "RCCL" in j["config"]["schedule"]
    assert "torch.distributed process group" in j["config"]["schedule"]
    assert j["quality"]["exchange_ms_per_step_rank0"] > 0 and j["value"] > 0 and j["steps"] == 3
    assert j["quality"]["cost_2f_after_step"] < j["quality"]["cost_2f_trajectory"][0]


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_through_the_peer_store():
    """bench.py with TWO ranks (torch.distributed.run --nproc-per-node 2, both on device 0) and --transport ipc: gloo process
    group, 2 agents per rank, the public poses written by the senders' pack kernels straight into the receivers'
    hipIpc-mapped neighbour buffers (dpgo_amd/ipc.py), barrier + max-over-ranks timing, rank 0 prints the line."""
    port = 29500 + ((os.getpid() + 211) % 400)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--transport", "ipc",
           "--workload", "grid:12x10x8", "--steps", "3", "--warmup", "1", "--settle", "1", "--no-cpu-baseline",
           "--no-secondary", "--spmm-reps", "10", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stderr[-3000:]
    line, j = records(p.stdout)  # (one driver line: rank 0 only)
    assert line["n_gpus"] == 2 and line["config"]["transport"] == "ipc"
    assert j["n_gpus"] == 2 and j["config"]["agents"] == 4 and j["config"]["agents_per_gpu"] == 2
    assert j["config"]["dist_backend"] == "gloo" and j["config"]["transport"] == "ipc" and "peer store" in j["config"]["schedule"]
    assert j["quality"]["exchange_ms_per_step_rank0"] > 0 and j["value"] > 0 and j["scaling"] == "strong"
    assert j["quality"]["cost_2f_after_step"] < j["quality"]["cost_2f_trajectory"][0]
