"""Times Sim3Solver's RANSAC for a batch of keyframe pairs whose keypoints, map points and matches are on the device -- ONE sslam_sim3_ransac_batch_dev call (b) -- beside
what a caller had before it (a): the same arithmetic on the host, one core (tests/sim/sim3_sim.cpp, the plain build: csrc/sim3_math.h under g++ -O2).

    python tools/sim3_batch_probe.py [--batches 20,64,1024,8192] [--reps 5] [--unique 4] [--out profiles/sim3_batch_probe.txt]

A pair is what SearchByBoW leaves behind between a keyframe and a loop candidate: 1 000 rows per keyframe, 150 of keyframe 1's matched, about a third of them the same map
points under one similarity (2 mm of noise), the rest anywhere.  Three calls per pair are timed, each on a fresh solver: the five iterations LoopClosing asks for at a time
(src/LoopClosing.cc:296) and find()'s 300 at once, both with 72 inliers asked for at a probability of 1 - 1e-16 -- no hypothesis reaches 72, so every iteration asked for is
run, and SetRansacParameters allows all 300 -- and five iterations under LoopClosing's own parameters (0.99, 20 inliers, 300), where a pair may return early.  Pair p of a
batch is unique pair p % unique (its draw still hashes p).
(a): wall time of the sim process over the unique pairs, per pair; it includes the program's text input and output (every hypothesis is printed).
(b): device time between two HIP events around the call on a side stream, wall time from the call to the end of a stream synchronise, and k_sim3_ransac alone through
sslam_profile_enable / sslam_profile_drain.  After a warm-up pass, `reps` passes; medians, with the lowest and highest pass.  The states and inlier rows of the first `unique`
pairs of every batch must equal the sim's bit for bit, or the probe exits non-zero."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import sim3_cases as tc
import sim3_sim as sim
import batch_probe_common as bp
from batch_probe_common import med

N, MATCHES, SEED = 1000, 150, 2026
INTS = ("its_done", "best_inliers", "best_it", "n", "max_its", "found_it", "n_inliers", "no_more")


def same_state(got, want):
    f = bp.same_floats
    return all(int(got[k]) == int(want[k]) for k in INTS) and all(f(got[k], want[k]) for k in ("s12", "R12", "t12"))


def main():
    a = bp.parse_args("--batches", "20,64,1024,8192", 5, 4, loop_lib=False)
    log = bp.Lines(); say = log.say
    fe = pkg.frontend()
    ctx = fe.Context(0)
    U = a.unique
    pairs = [tc.make("probe_%d" % u, 9000 + u, N, N, MATCHES, outliers=0.65) for u in range(U)]
    say("pair: %d rows per keyframe, %d matches, two thirds of them outliers; %d unique pairs" % (N, MATCHES, U))
    sim.programs()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)).cuda()
    kp = np.zeros((U, 2, N), fe.KP_DTYPE); x = np.zeros((U, 2, N, 3), np.float32)
    for u, c in enumerate(pairs):
        kp[u, 0]["octave"], kp[u, 1]["octave"] = c["kf1"]["oct"], c["kf2"]["oct"]
        x[u, 0], x[u, 1] = c["kf1"]["x3dc"], c["kf2"]["x3dc"]
    dKP, dX, dM = up(kp.reshape(U, -1)), up(x.reshape(U, -1)), up(np.stack([c["m12"] for c in pairs]))
    st = torch.cuda.Stream()
    report = {}
    all_equal = True
    never = dict(fix_scale=False, probability=1 - 1e-16, min_inliers=72, max_iterations=300, seed=SEED)
    for tag, new_its, kw in (("iterate(5)", 5, never), ("find(): 300", 300, never),
                             ("iterate(5), LoopClosing's 20 inliers", 5, dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, seed=SEED))):
        ta = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = sim.run_plain([dict(c, pair=p, calls=[new_its], sets=None, **kw) for p, c in enumerate(pairs)])
            ta.append((time.perf_counter() - t0) * 1e6 / U)
        ran = [len(w["calls"][0]["its"]) for w in want]
        say("%s | (a) the sim on one core: %.0f us per pair (min %.0f max %.0f over 3 runs of %d pairs), iterations run %s, returned at %s"
            % (tag, med(ta), min(ta), max(ta), U, ran, [int(w["calls"][0]["state"]["found_it"]) for w in want]))
        report[tag] = dict(sim_us_per_pair=med(ta), sim_all_us_per_pair=ta, iterations_run=ran)
        for B in a.sizes:
            rep = lambda d: d.repeat(-(-B // U), 1)[:B].contiguous()
            dkp, dx, m12 = rep(dKP), rep(dX), rep(dM)                     # pair p is slots 2p, 2p + 1 of a pool of 2B slots of N rows
            n = torch.full((2 * B,), N, dtype=torch.int32, device="cuda")
            K = torch.from_numpy(np.tile(np.stack([tc.K1, tc.K2]), (B, 1))).cuda()
            pr = torch.arange(2 * B, dtype=torch.int32, device="cuda")
            state = torch.zeros(B * 84, dtype=torch.uint8, device="cuda"); inl = torch.zeros(B * N, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def enqueue():
                with torch.cuda.stream(st):
                    state.zero_()                                         # a fresh solver every pass
                ctx.sim3_ransac_batch_dev(dkp, dx, None, n, N, 2 * B, K, tc.SIGMA2, pr, B, m12, state, inl, new_iterations=new_its, stream=st.cuda_stream, **kw)
            bp.timed_pass(st, enqueue)                                    # warm-up
            got = state.cpu().numpy().view(fe.SIM3_STATE_DTYPE); gi = inl.cpu().numpy().reshape(B, N)
            same = all(same_state(got[p], want[p]["calls"][0]["state"]) and np.array_equal(gi[p], want[p]["calls"][0]["inliers"]) for p in range(min(B, U)))
            all_equal = all_equal and same
            tb = [bp.timed_pass(st, enqueue) for _ in range(a.reps)]
            kb = bp.kernel_passes(fe.lib(), ctx.h, st, enqueue, "k_sim3_ransac", a.reps)
            dev_ms, wall_ms, enq_ms = bp.b_medians(tb)
            report[tag]["B%d" % B] = dict(pairs=B, equal=same, b_device_ms=dev_ms, b_wall_ms=wall_ms, b_enqueue_ms=enq_ms, b_all_ms=tb, k_sim3_ransac_ms=med(kb), k_sim3_ransac_all_ms=kb,
                                          us_per_pair=dev_ms * 1e3 / B)
            say("%s | pairs %6d | (b) batch: %9.3f ms device (min %.3f max %.3f), %9.3f ms wall, %6.3f ms enqueue | k_sim3_ransac alone %9.3f ms (min %.3f max %.3f) | %8.2f us per pair | "
                "(a) x pairs / (b) device = %7.1f x | equal %s" % (tag, B, dev_ms, min(t[0] for t in tb), max(t[0] for t in tb), wall_ms, enq_ms, med(kb), min(kb), max(kb),
                                                                  dev_ms * 1e3 / B, med(ta) * B / (dev_ms * 1e3), same))
            del dkp, dx, m12, n, K, pr, state, inl
    ctx.close()
    log.finish("sim3_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
