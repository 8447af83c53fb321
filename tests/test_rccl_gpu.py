"""GPU: the exchange step of the sharded mode over RCCL.  The GPU box has one device, so the launch is the
driver's own (`python -m torch.distributed.run --nproc-per-node 1 ... bench.py`) with SSLAM_FORCE_COLLECTIVE=1: the process
group is nccl (= RCCL), every step's packed records go through dist.gather on the device, and bench.py --full reports (config.gather_check) whether what
rank 0 receives equals its own packed results.  World sizes > 1 are covered on gloo in test_dist_cpu.py."""
import json, os, subprocess, sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_under_torchrun_with_rccl_gather():
    env = dict(os.environ, SSLAM_FORCE_COLLECTIVE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    port = 29600 + (os.getpid() % 300)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "64",
           "--full", "--no-cpu-baseline", "--no-other-workloads"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["value"] > 0
    assert out["config"]["mean_keypoints"] > 500 and out["config"]["mean_lines"] > 50
    assert out["config"]["gather_check"] is True          # rank 0 compared what RCCL delivered with its own packed records


@pytest.mark.timeout(600)
def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` with no launcher around it must start its N ranks itself (what the driver's first 8-GPU run will type).  One GPU here: the same code path
    with N = 1 forced through it (--self-launch): torch.distributed.run on 127.0.0.1, one rank, the RCCL exchange inside every step, ONE JSON line from rank 0 that
    carries n_gpus, the per-rank wall times, gather_check and the communicator's rank count, exit code 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SSLAM_FORCE_COLLECTIVE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--self-launch", "--steps", "2", "--warmup", "1", "--batch", "64", "--full", "--no-cpu-baseline", "--no-other-workloads"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["value"] > 0
    g = out["config"]["gather"]
    assert out["config"]["gather_check"] is True and g["self_launched"] is True and g["rccl_ranks"] == 1
    assert len(g["per_rank"]) == 1 and g["per_rank"][0]["wall_s"] > 0
    # BASELINE configs[4] (8 frames dealt over the GPUs, H2D + extract + match + RCCL gather inside the step) through the same launch path
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--self-launch", "--workload", "c5", "--steps", "3", "--warmup", "1", "--full"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    c5 = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert c5["n_gpus"] == 1 and c5["scaling"] == "strong" and c5["config"]["global_batch"] == 8 and c5["config"]["gather_check"] is True
    # more ranks than GPUs: a one-line refusal and a non-zero exit code, not N tracebacks
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr


_RANK_SCRIPT = r"""
import sys, os, numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import pkg
fe = pkg.frontend()
uid = np.frombuffer(bytes.fromhex(sys.argv[2]), np.uint8)
try:
    g = fe.Group(device=0, rank=int(sys.argv[3]), nranks=2, uid=uid)
    print("CREATED"); g.close()
except fe.SslamError as e:
    print("REFUSED:", e)
"""


@pytest.mark.timeout(300)
def test_two_process_ranks_on_one_device_meet_real_rccl_and_are_refused_cleanly(tmp_path):
    """What one GPU allows of N > 1 over the REAL library: two processes, both on device 0, go through ncclGetUniqueId (here) and ncclCommInitRank (there) -- the
    bootstrap runs between two real processes -- and RCCL itself refuses the communicator ("Duplicate GPU detected": this build has no switch for several ranks per
    device; `strings librccl.so`).  The library must hand that refusal back as an error with RCCL's own text from BOTH ranks, without a hang or a crash.  The 1 -> 8
    curve over xGMI remains the driver's scaling run (never measured: SCALE_r01..r04 are skip records)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pkg
    fe = pkg.frontend()
    uid = fe.Group.unique_id()
    script = tmp_path / "rank.py"; script.write_text(_RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, bytes(uid).hex(), str(r)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try: o, e = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill(); o, e = p.communicate(); o += "\nTIMEOUT"
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert "TIMEOUT" not in o, (o, e[-2000:])
        assert rc == 0, (o, e[-2000:])
        assert "REFUSED:" in o and "ncclCommInitRank failed" in o, (o, e[-2000:])
