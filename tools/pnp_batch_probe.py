"""Times PnPsolver's RANSAC for a batch of (keyframe, frame) pairs whose keypoints, map points and matches are on the device -- ONE sslam_pnp_ransac_batch_dev call (b) --
beside what a caller had before it (a): the same arithmetic on the host, one core (tests/sim/pnp_sim.cpp, the plain build: csrc/pnp_math.h under g++ -O2).

    python tools/pnp_batch_probe.py [--batches 20,64,1024,8192] [--reps 5] [--unique 4] [--out profiles/pnp_batch_probe.txt]

A pair is what SearchByBoW leaves behind between a lost frame and a candidate keyframe: 1 000 rows on each side, 150 of the frame's matched, a third of them the keyframe's
map points under one pose (0.3 px of noise), the rest anywhere.  Two calls per pair are timed with 72 inliers asked for at a probability of 1 - 1e-16 and max_iterations
300 -- no hypothesis reaches 72, so nothing returns: the first call on a fresh solver, which runs all 300 iterations (iterate's loop condition is an OR, src/PnPsolver.cc:182),
and the call after it, which runs the five iterations Tracking asks for at a time (src/Tracking.cc:2021).  Pair p of a batch is unique pair p % unique (its draw still
hashes p).
(a): wall time of the sim process over the unique pairs, per pair; it includes the program's text input and output (every hypothesis is printed).
(b): device time between two HIP events around the call on a side stream, wall time from the call to the end of a stream synchronise, and k_pnp_ransac alone through
sslam_profile_enable / sslam_profile_drain.  After a warm-up pass, `reps` passes; medians, with the lowest and highest pass.  The states and inlier rows of the first
`unique` pairs of every batch must equal the sim's bit for bit, or the probe exits non-zero.
Not measured: a call that returns early through Refine, capacities other than 1 000, and the same batch through separate single calls."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import pnp_cases as tc
import pnp_sim as sim
import host_sim
import batch_probe_common as bp
from batch_probe_common import med

N, MATCHES, SEED = 1000, 150, 2026
INTS = ("its_done", "best_inliers", "best_it", "refine_ok", "n", "min_inliers", "max_its", "found", "found_it", "n_inliers", "no_more")


def same_state(got, want):
    f = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())
    return all(int(got[k]) == int(want[k]) for k in INTS) and all(f(got[k], want[k]) for k in ("best_R", "best_t", "Tcw"))


def make(seed):
    """one pair: MATCHES correspondences, a third of them under one pose, padded to N rows on both sides"""
    c, groups, _ = tc.scene(seed, [MATCHES // 3, MATCHES - MATCHES // 3], noise=0.3)
    r = np.random.RandomState(seed)
    keep = np.where((c["assigned"] >= 0))[0]
    out = keep[groups[1]]
    c["pt"][out] = r.uniform(0, 600, (len(out), 2)).astype(np.float32)
    nf, nkf = len(c["oct"]), len(c["xw"])
    pad = lambda a, n, fill: np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])
    return dict(c, oct=pad(c["oct"], N, 0), pt=pad(c["pt"], N, 1.0), xw=pad(c["xw"], N, 1.0), valid=pad(c["valid"], N, 1), assigned=pad(c["assigned"], N, -1))


def main():
    a = bp.parse_args("--batches", "20,64,1024,8192", 5, 4, loop_lib=False)
    log = bp.Lines(); say = log.say
    fe = pkg.frontend()
    ctx = fe.Context(0)
    U = a.unique
    pairs = [make(9000 + u) for u in range(U)]
    say("pair: %d rows on each side, %d matches, two thirds of them outliers; %d unique pairs" % (N, MATCHES, U))
    host_sim.programs(sim.SRC)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)).cuda()
    kp = np.zeros((U, N), fe.KP_DTYPE)
    for u, c in enumerate(pairs):
        kp[u]["octave"] = c["oct"]; kp[u]["x"] = c["pt"][:, 0]; kp[u]["y"] = c["pt"][:, 1]
    dKP, dX, dA = up(kp), up(np.stack([c["xw"] for c in pairs])), up(np.stack([c["assigned"] for c in pairs]))
    st = torch.cuda.Stream()
    report = {}
    all_equal = True
    kw = dict(probability=1 - 1e-16, min_inliers=72, max_iterations=300, epsilon=0.05, th2=5.991, seed=SEED)
    for tag, calls in (("the first call: 300", [300]), ("iterate(5) after it", [300, 5])):
        ta = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = sim.run_plain([dict(c, pair=p, calls=calls, sets=None, **kw) for p, c in enumerate(pairs)])
            ta.append((time.perf_counter() - t0) * 1e6 / U)
        if len(calls) == 2:      # the second call alone: the difference to the first call's time
            ta = [max(t - report["the first call: 300"]["sim_us_per_pair"], 0.0) for t in ta]
        ran = [len(w["calls"][-1]["its"]) for w in want]
        say("%s | (a) the sim on one core: %.0f us per pair (min %.0f max %.0f over 3 runs of %d pairs), iterations run %s" % (tag, med(ta), min(ta), max(ta), U, ran))
        report[tag] = dict(sim_us_per_pair=med(ta), sim_all_us_per_pair=ta, iterations_run=ran)
        for B in a.sizes:
            rep = lambda d: d.repeat(-(-B // U), 1)[:B].contiguous()
            dkp, dx, asg = rep(dKP), rep(dX), rep(dA)                     # pair p is frame slot p against keyframe slot p
            n = torch.full((B,), N, dtype=torch.int32, device="cuda")
            K = torch.from_numpy(np.tile(tc.K, (B, 1))).cuda()
            state = torch.zeros(B * 192, dtype=torch.uint8, device="cuda"); inl = torch.zeros(B * N, dtype=torch.uint8, device="cuda")
            start = torch.zeros(B * 192, dtype=torch.uint8, device="cuda")
            launch = lambda its: ctx.pnp_ransac_batch_dev(dkp, n, N, B, K, dx, None, n, N, B, tc.SIGMA2, None, None, B, asg, state, inl, new_iterations=its, stream=st.cuda_stream, **kw)
            if len(calls) == 2:      # the state the first call leaves behind
                launch(300)
                st.synchronize()
                start.copy_(state)
            torch.cuda.synchronize()

            def enqueue():
                with torch.cuda.stream(st):
                    state.copy_(start)                                    # the same solver every pass
                launch(calls[-1])
            bp.timed_pass(st, enqueue)                                    # warm-up
            got = state.cpu().numpy().view(fe.PNP_STATE_DTYPE); gi = inl.cpu().numpy().reshape(B, N)
            same = all(same_state(got[p], want[p]["calls"][-1]["state"]) and np.array_equal(gi[p], want[p]["calls"][-1]["inliers"]) for p in range(min(B, U)))
            all_equal = all_equal and same
            tb = [bp.timed_pass(st, enqueue) for _ in range(a.reps)]
            kb = bp.kernel_passes(fe.lib(), ctx.h, st, enqueue, "k_pnp_ransac", a.reps)
            dev_ms, wall_ms, enq_ms = bp.b_medians(tb)
            report[tag]["B%d" % B] = dict(pairs=B, equal=same, b_device_ms=dev_ms, b_wall_ms=wall_ms, b_enqueue_ms=enq_ms, b_all_ms=tb, k_pnp_ransac_ms=med(kb), k_pnp_ransac_all_ms=kb,
                                          us_per_pair=dev_ms * 1e3 / B)
            say("%s | pairs %6d | (b) batch: %9.3f ms device (min %.3f max %.3f), %9.3f ms wall, %6.3f ms enqueue | k_pnp_ransac alone %9.3f ms (min %.3f max %.3f) | %8.2f us per pair | "
                "(a) x pairs / (b) device = %7.1f x | equal %s" % (tag, B, dev_ms, min(t[0] for t in tb), max(t[0] for t in tb), wall_ms, enq_ms, med(kb), min(kb), max(kb),
                                                                  dev_ms * 1e3 / B, med(ta) * B / (dev_ms * 1e3), same))
            del dkp, dx, asg, n, K, state, inl, start
    ctx.close()
    log.finish("pnp_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
