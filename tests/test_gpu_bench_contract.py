"""bench.py keeps the driver's contract: ONE JSON line with the metric of BASELINE.json, whole-job value, the roofline and
cpu_baseline objects; the extra workloads print the same shape without them."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_default_workload_line():
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    d = _run("--steps", "20", "--warmup", "5", "--cpu-steps", "4", "--cpu-traj", "16", "--full")
    assert d["metric"] == base["metric"] and d["unit"] == "rollout-steps/s"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, 20, 5)
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 1024 * 20 / (d["ms_per_step"] * 20 / 1e3)) <= 1e-3 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma", "valu-issue") and r["unit"] == "TFLOP/s" and r["peak"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["kernel_ms"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and isinstance(c["sample"], str)
    assert d["q_l2_relerr_vs_oracle_max"] < 1e-8
    assert d["config"]["all_finite"] and d["config"]["not_converged_trajectories"] == 0
    # round-2 measurement contract: a utilisation (<= 1) from executed flops, traffic for ANY --steps, an issue-bound ceiling,
    # the reference-tolerance line, the tensor-free CPU baseline, Newton-count agreement and the repeated launches
    assert 0 < r["frac"] <= 1 and r["traffic"] > 0 and 0 < r["issue_bound"]["frac"] <= 1.05
    assert r["algorithmic_equiv_tflops"] > r["achieved"]
    # round 4: the lane-honest fraction (flops of the scalar algorithm, tests/flop_count.py) beside the 64-lane one
    assert 0 < r["useful_frac"] < r["frac"] and "calibration_stale" not in r
    if d["rollout_ms"]["slowest_rollout"] == 0:       # reported when the launch ends with rollout 0 (it does over 100 steps; a short --steps
        assert d["value_without_rollout_0"]["value"] > d["value"]      # window can end with another rollout)
    # round 3: the headline runs the reference's own tol; the side measurements run the reference's 100 steps whatever --steps is
    assert d["config"]["newton_tol"] == 1e-9 == d["config"]["reference_newton_tol"]
    t = d["value_plain_iterate"]
    assert t["newton_tol"] == 1e-9 and t["steps"] == 100 and t["value"] > 0 and t["all_finite"]
    assert t["newton_iters_per_step"] > r["newton_iters_per_step"] and t["not_converged_trajectories"] > 100 and t["value"] < 0.5 * d["value"]
    w = d["value_at_survey_init"]
    assert w["steps"] == 100 and w["value"] > 0 and w["all_finite"] and w["newton_iters_per_step"] > r["newton_iters_per_step"]
    assert d["value_at_tol_1e-8"]["value"] > 0 and d["value_at_tol_1e-8"]["not_converged_trajectories"] == 0
    tf = d["cpu_baseline_tensor_free"]
    assert tf["value"] > c["value"] and tf["q_l2_relerr_gpu_vs_this_max"] < 1e-8
    n = d["newton_count_agreement"]
    # per trajectory-step (>= 99 %).  The literal oracle's sample is only 16 x 4 trajectory-steps in this quick run
    # (one differing step would already be 1.6 %), so the 99 % bar is applied to the 1600-step sample and to the full-size
    # checks in tests/test_gpu_soak.py; here the small sample must not differ in more than one step
    assert n["vs_tensor_free"]["frac"] >= 0.99
    o8 = n["vs_oracle_at_tol_1e-8"]
    assert o8["trajectory_steps"] - o8["trajectory_steps_with_equal_count"] <= 1
    assert n["vs_oracle"]["gpu_iters"] <= n["vs_oracle"]["cpu_iters"]      # at the reference's tol the literal port wanders over the lattice
    assert d["repeat"]["launches"] >= 6 and d["repeat"]["kernel_ms_min"] <= d["repeat"]["kernel_ms_median"]
    assert "strong_scaling" not in d          # one rank: weak and strong coincide


def test_two_ranks_on_one_gpu_self_launch():
    """`python bench.py --gpus 2` bare (no torchrun): bench.py re-executes itself under torch.distributed.run.  On a 1-GPU box
    both ranks share device 0, where RCCL refuses duplicate GPUs, so the gather goes through gloo with host tensors - the rank
    code, shard plans, barriers and both scaling modes are the ones an 8-GPU RCCL run uses."""
    d = _run("--gpus", "2", "--steps", "10", "--warmup", "2", "--batch", "256", "--repeats", "1", "--no-side-legs", "--full")
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 512 and d["config"]["gathered_rows"] == 512
    assert d["scaling"] == "weak" and d["value"] > 0 and d["config"]["all_finite"]
    s = d["strong_scaling"]
    assert s["global_batch"] == 256 and s["batch_per_gpu"] == 128 and s["value"] > 0
    assert d["value_strong"] == s["value"] and len(d["kernel_ms_per_rank"]["weak"]) == 2 and min(d["kernel_ms_per_rank"]["strong"]) > 0


def test_plain_line_and_dump_outputs(tmp_path):
    """A plain run times the headline launch alone (the side objects need --full); --dump-outputs writes that launch's final state,
    which is the library's own result for the bench's inputs after the W warm-up and the K timed steps."""
    import bench
    import numpy as np
    d = _run("--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert (d["steps"], d["warmup"]) == (5, 2) and abs(d["value"] - 1024 * 5 / (d["ms_per_step"] * 5e-3)) <= 1e-3 * d["value"]
    assert d["config"]["all_finite"] and d["roofline"]["kernel_ms"] > 0
    for k in ("repeat", "value_plain_iterate", "value_at_survey_init", "value_at_max_valid_init", "value_at_tol_1e-8", "cpu_baseline",
              "cpu_baseline_tensor_free", "newton_count_agreement"):
        assert k not in d, k
    q, qd = np.load(tmp_path / "q.npy"), np.load(tmp_path / "qdot.npy")
    assert q.shape == qd.shape == (1024, 32) and q.dtype == qd.dtype == np.float64
    scene, h, integ, gen = bench.build_workload("chain", 32)
    st = bench.GpuStepper(scene, 1024, 0, integ)
    st.set_opts(h, 1e-9)
    st.set_state(*gen(0, 1024))
    st.warmup(2)
    st.launch(5)
    st.wait()
    qr, qdr = st.get_state()
    st.close()
    assert np.array_equal(q, qr) and np.array_equal(qd, qdr)


@pytest.mark.parametrize("wl", ["tree64", "ground"])
def test_extra_workload_lines(wl):
    d = _run("--workload", wl, "--steps", "10", "--warmup", "2", "--batch", "64")
    assert d["value"] > 0 and "cpu_baseline" not in d
    assert d["config"]["batch_per_gpu"] == 64 and d["config"]["all_finite"]
    # round 4: every workload line carries an executed-work roofline (a non-default signature uses the per-stage model or the scaled
    # totals of the calibrated launch) and the lane-honest fraction
    r = d["roofline"]
    assert r["bound"] == "valu-issue" and r["unit"] == "TFLOP/s" and "calibration_stale" not in r
    assert 0 < r["useful_frac"] <= r["frac"] <= 1 and r["kernel_ms"] > 0


def test_extra_workload_default_signature_uses_the_counter_totals():
    """At the calibrated signature the launch repeats the calibrated launch's Newton iterations exactly (deterministic workload), and the
    roofline uses the counter totals of that very launch."""
    d = _run("--workload", "tree64", "--no-side-legs", "--repeats", "0")
    r = d["roofline"]
    assert "counter totals of this very launch" in r["executed_flops_from"], r["executed_flops_from"]
    # (<=: on this branching tree the kernels execute FEWER flops than the dense scalar twin behind `useful` needs, and bench.py caps)
    assert 0 < r["useful_frac"] <= r["frac"] <= 1


def test_adjoint_workload_line():
    """BASELINE.json configs[3] at config size: 16-DOF chain, 512 rollouts, forward + backward sweep: issue-bound roofline (round 4; the
    HBM figure of rounds 1-3 stays as a side object - the path is not bound by it)."""
    d = _run("--workload", "adjoint", "--repeats", "2")
    assert d["steps"] == 20 and d["config"]["batch_per_gpu"] == 512 and d["value"] > 0
    assert d["config"]["all_finite"] and d["config"]["not_converged_trajectories"] == 0
    r = d["roofline"]
    assert r["bound"] == "valu-issue" and r["unit"] == "TFLOP/s" and 0 < r["useful_frac"] <= r["frac"] <= 1 and r["kernel_ms"] > 0
    assert "calibration_stale" not in r and 0 < r["hbm"]["frac_of_8TBps"] < 0.1


def test_rccl_code_path_at_world_size_one():
    """No multi-GPU node is available to the test environment, and at world size 1 bench.py forms no process group - so the RCCL half of the
    N > 1 path (init with device_id, barrier, all_gather_into_tensor on the device tensors rmx_get_state_device fills, device-side
    max-reduction of the elapsed time) would meet the driver's 8-GPU run untested.  RMX_BENCH_FORCE_DIST=1 forms the group at world size
    1: the same calls on a one-rank RCCL communicator."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547",
               RMX_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline",
                        "--no-side-legs", "--repeats", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "RCCL" in d["config"]["parallelism"] and d["config"]["gathered_rows"] == 1024 and d["config"]["all_finite"]
    assert d["value"] > 0 and d["n_gpus"] == 1


_RCCL_TWO_RANKS = r'''
import datetime, json, os, sys, traceback
sys.path.insert(0, sys.argv[1])
rank, port, out = int(sys.argv[2]), sys.argv[3], sys.argv[4]
import torch
import torch.distributed as dist
from redmax_amd import sharding
res = {"rank": rank, "stage": "init", "error": None}
try:
    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    os.environ["TORCH_NCCL_ASYNC_ERROR_HANDLING"] = "1"
    # exactly bench.py's rank_main call for a rank that owns a GPU: backend nccl (= RCCL), device_id given -> eager communicator
    import functools
    orig = dist.init_process_group
    dist.init_process_group = functools.partial(orig, timeout=datetime.timedelta(seconds=60))
    d = sharding.init_process_group(rank, 2, "nccl", device=0)
    res["stage"] = "collective"
    plan = sharding.plan(rank, 2, 4, "weak")
    q = torch.full((4, 3), float(rank), dtype=torch.float64, device="cuda:0")
    qa, _ = sharding.gather_states(q, q.clone(), plan)
    torch.cuda.synchronize()
    res["stage"] = "done"
    res["rows"] = int(qa.shape[0])
except BaseException as e:      # noqa: BLE001 - the text of the failure is the test's subject
    res["error"] = "%s: %s" % (type(e).__name__, e)
    res["trace"] = traceback.format_exc()[-1500:]
json.dump(res, open(out, "w"))
os._exit(0)
'''


def test_rccl_group_of_two_ranks_on_one_gpu_is_refused_as_expected(tmp_path):
    """The N = 2 RCCL path as far as a 1-GPU box allows (round-4 review): two processes build bench.py's own process group -
    sharding.init_process_group(rank, 2, "nccl", device) with device_id, then the gather of sharding.gather_states on device
    tensors - with BOTH ranks on device 0.  RCCL must refuse exactly that ("Duplicate GPU detected"): every line up to the
    communicator has then run with world size 2 (rendezvous, device_id, eager init), and a typo on that path shows up here as some
    OTHER error instead of surviving until the driver's 8-GPU run.  (bench.py itself detects shared devices and takes gloo.)"""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    script = tmp_path / "two_ranks.py"
    script.write_text(_RCCL_TWO_RANKS)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), port, str(tmp_path / ("r%d.json" % r))], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append("TIMEOUT " + p.communicate()[0])
    res = [json.load(open(tmp_path / ("r%d.json" % r))) if (tmp_path / ("r%d.json" % r)).exists() else None for r in range(2)]
    text = " ".join(logs) + " ".join((r or {}).get("error") or "" for r in res)
    print(res, logs[0][-800:], logs[1][-800:])
    out_dir = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out_dir, exist_ok=True)
    json.dump({"results": res, "logs": [lg[-3000:] for lg in logs]}, open(os.path.join(out_dir, "rccl_two_ranks_one_gpu.json"), "w"), indent=1)
    assert all(r is not None for r in res), "a rank died without reporting"
    assert any(r["error"] for r in res), "RCCL accepted two ranks on one GPU?"
    assert "uplicate GPU" in text or "invalid usage" in text, text[-1500:]
    for r in res:                         # nothing failed BEFORE the communicator: no NameError / TypeError / AttributeError on the path
        assert not (r["error"] or "").startswith(("NameError", "TypeError", "AttributeError", "ImportError", "KeyError")), r
