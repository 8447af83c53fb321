"""Times Initializer::Initialize's model selection for a batch of frame pairs whose keypoints and matches are on the device -- ONE sslam_two_view_ransac_batch_dev
call (b) -- beside what a caller had before it (a): the same arithmetic on the host, one core (tests/sim/two_view_sim.cpp, the plain build: csrc/two_view_math.h under g++ -O2).

    python tools/two_view_batch_probe.py [--batches 20,64,1024,12288] [--reps 5] [--unique 4] [--out profiles/two_view_batch_probe.txt]

A pair is what SearchForInitialization leaves behind: 1 000 undistorted keypoints per frame, about 300 of frame 1's matched, 70 % of them on one plane (0.5 pixels of
noise), the rest anywhere; 200 iterations, sigma 1, the library draws the sets.  Pair p of a batch is unique pair p % unique (its draw still hashes p).
(a): wall time of the sim process over the unique pairs, per pair; it includes the program's text input and output (every hypothesis is printed).
(b): device time between two HIP events around the call on a side stream, wall time from the call to the end of a stream synchronise, and k_two_view alone through
sslam_profile_enable / sslam_profile_drain.  After a warm-up pass, `reps` passes; medians, with the lowest and highest pass.  The results of the first `unique` pairs of every
batch must equal the sim's bit for bit, or the probe exits non-zero."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import two_view_cases as tc
import two_view_sim as sim
import batch_probe_common as bp
from batch_probe_common import med

N, MATCHES, ITERATIONS, SIGMA, SEED = 1000, 300, 200, 1.0, 2026


def same_result(got, want):
    f = bp.same_floats
    return all(int(got[k]) == int(want[k]) for k in ("nmatches", "model", "best_it_h", "best_it_f")) and all(f(got[k], want[k]) for k in ("score_h", "score_f", "rh", "H21", "F21"))


def main():
    a = bp.parse_args("--batches", "20,64,1024,12288", 5, 4, loop_lib=False)
    log = bp.Lines(); say = log.say
    fe = pkg.frontend()
    ctx = fe.Context(0)
    U = a.unique
    pairs = [dict(tc.make("probe_%d" % u, 9000 + u, N, N, MATCHES, noise=0.5, outliers=0.3, iterations=ITERATIONS, sigma=SIGMA), seed=SEED) for u in range(U)]
    say("pair: %d keypoints per frame, %d matches, %d iterations, sigma %.1f; %d unique pairs" % (N, MATCHES, ITERATIONS, SIGMA, U))
    sim.programs()
    ta = []
    for _ in range(3):
        t0 = time.perf_counter(); want = sim.run_plain([dict(c, pair=p) for p, c in enumerate(pairs)]); ta.append((time.perf_counter() - t0) * 1e6 / U)
    say("(a) the sim on one core: %.0f us per pair (min %.0f max %.0f over 3 runs of %d pairs), models %s" % (med(ta), min(ta), max(ta), U, [int(w["result"]["model"]) for w in want]))
    kp = np.zeros((U, 2, N), fe.KP_DTYPE)
    for u, c in enumerate(pairs):
        kp[u, 0]["x"], kp[u, 0]["y"], kp[u, 1]["x"], kp[u, 1]["y"] = c["kp1"][:, 0], c["kp1"][:, 1], c["kp2"][:, 0], c["kp2"][:, 1]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)).cuda()
    dK1, dK2, dM = up(kp[:, 0]), up(kp[:, 1]), up(np.stack([c["m12"] for c in pairs]))
    st = torch.cuda.Stream()
    report = dict(sim_us_per_pair=med(ta), sim_all_us_per_pair=ta)
    all_equal = True
    for B in a.sizes:
        rep = lambda d: d.repeat(-(-B // U), 1)[:B].contiguous()
        k1, k2, m12 = rep(dK1), rep(dK2), rep(dM)
        n = torch.full((B,), N, dtype=torch.int32, device="cuda")
        res = torch.zeros(B * fe.TWO_VIEW_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda"); inl = torch.zeros(B * N, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enqueue = lambda: ctx.two_view_ransac_batch_dev(k1, n, k2, n, N, B, m12, res, inl, iterations=ITERATIONS, sigma=SIGMA, seed=SEED, stream=st.cuda_stream)
        bp.timed_pass(st, enqueue)                                        # warm-up
        got = res.cpu().numpy().view(fe.TWO_VIEW_RESULT_DTYPE); gi = inl.cpu().numpy().reshape(B, N)
        same = all(same_result(got[p], want[p]["result"]) and np.array_equal(gi[p], want[p]["inliers"]) for p in range(min(B, U)))
        all_equal = all_equal and same
        tb = [bp.timed_pass(st, enqueue) for _ in range(a.reps)]
        kb = bp.kernel_passes(fe.lib(), ctx.h, st, enqueue, "k_two_view", a.reps)
        dev_ms, wall_ms, enq_ms = bp.b_medians(tb)
        report["B%d" % B] = dict(pairs=B, equal=same, b_device_ms=dev_ms, b_wall_ms=wall_ms, b_enqueue_ms=enq_ms, b_all_ms=tb, k_two_view_ms=med(kb), k_two_view_all_ms=kb,
                                 us_per_pair=dev_ms * 1e3 / B, models=[int((got["model"] == m).sum()) for m in (0, 1, 2)])
        say("pairs %6d | (b) batch: %9.3f ms device (min %.3f max %.3f), %9.3f ms wall, %6.3f ms enqueue | k_two_view alone %9.3f ms (min %.3f max %.3f) | %8.2f us per pair | "
            "(a) x pairs / (b) device = %7.1f x | equal %s" % (B, dev_ms, min(x[0] for x in tb), max(x[0] for x in tb), wall_ms, enq_ms, med(kb), min(kb), max(kb),
                                                              dev_ms * 1e3 / B, med(ta) * B / (dev_ms * 1e3), same))
        if B == 1024:
            # the same batch with all but the first eight matches of every pair removed: the solves, Normalize and the compaction stay, the scoring shrinks to eight rows
            few = np.stack([np.where(np.cumsum(c["m12"] >= 0) <= 8, c["m12"], -1) for c in pairs]).astype(np.int32)
            m8 = rep(up(few))
            torch.cuda.synchronize()
            enqueue8 = lambda: ctx.two_view_ransac_batch_dev(k1, n, k2, n, N, B, m8, res, inl, iterations=ITERATIONS, sigma=SIGMA, seed=SEED, stream=st.cuda_stream)
            bp.timed_pass(st, enqueue8)
            t8 = [bp.timed_pass(st, enqueue8)[0] for _ in range(a.reps)]
            report["B%d" % B]["eight_matches_device_ms"] = med(t8)
            say("pairs %6d with 8 matches each: %9.3f ms device (min %.3f max %.3f) = the solves and what does not grow with the matches, %.0f %% of the %.3f ms with %d matches; "
                "the rest is scoring" % (B, med(t8), min(t8), max(t8), 100 * med(t8) / dev_ms, dev_ms, MATCHES))
            del m8
        del k1, k2, m12, n, res, inl
    ctx.close()
    log.finish("two_view_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
