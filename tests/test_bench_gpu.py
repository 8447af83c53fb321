"""GPU: a plain bench.py run (the headline figure only) and --dump-outputs: the result line carries the contract fields and none of the --full legs,
and the dumped arrays are what the timed step computed -- the sampled frames' keypoints, descriptors and lines equal the CPU oracle's for the same
seeded frames, and a second run writes the same bytes."""
import json, os, subprocess, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "96", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_plain_bench_and_dumped_outputs(tmp_path, oracle):
    import bench, pkg
    out = _bench(tmp_path / "a", 3)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and abs(out["value"] - 96 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"roofline", "cpu_baseline", "latency", "pcie_inclusive", "other_workloads", "latency_nfa_behind_core"} & set(out)
    d = tmp_path / "a"
    arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(arrays) == set(out["dumped_outputs"]["arrays"]) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    idx = arrays["frame_index"].astype(int)
    assert len(idx) == 96 and (arrays["keypoint_counts"] > 500).all() and arrays["orb_match_counts"].max() > 0
    fe = pkg.frontend()
    cur, _ = bench.synth_frames(640, 480, 64, 0)
    for j in (0, len(idx) - 1):
        i = idx[j]
        kp, desc = oracle.orb_extract(cur[i % 64], 1000)
        n = int(arrays["keypoint_counts"][i])
        assert n == len(kp)
        np.testing.assert_array_equal(arrays["keypoints"][j, :n], np.stack([kp[f].astype(np.float64) for f in fe.KP_DTYPE.names], -1))
        np.testing.assert_array_equal(arrays["descriptors"][j, :n], desc)
        assert not arrays["keypoints"][j, n:].any()
        kl, ld, fn, _ = oracle.lines_extract(cur[i % 64], 200)
        nl = int(arrays["line_counts"][i])
        assert nl == len(kl) > 0
        np.testing.assert_array_equal(arrays["line_descriptors"][j, :nl], ld)
        np.testing.assert_array_equal(arrays["line_functions"][j, :nl], fn)
    # the same arguments, another run (and another step count): the same inputs, so the same outputs
    _bench(tmp_path / "b", 2)
    for k, a in arrays.items():
        np.testing.assert_array_equal(np.load(tmp_path / "b" / (k + ".npy")), a, err_msg=k)
