"""Times ReconstructH / ReconstructF for a batch of frame pairs whose keypoints, matches, RANSAC results and inlier bytes are on the device -- ONE
sslam_two_view_reconstruct_batch_dev call (b) -- beside what a caller had before it (a): the same arithmetic on the host, one core (tests/sim/reconstruct_sim.cpp, the plain
build: csrc/reconstruct_math.h under g++ -O2).

    python tools/reconstruct_batch_probe.py [--batches 64,1024,8192] [--reps 5] [--unique 4] [--out profiles/reconstruct_batch_probe.txt]

A pair is what the RANSAC call leaves behind: `rows` keypoints a side, `matches` of them matched and inliers of the model, an exact F21 (general scene) or, for every other
unique pair, an H21 with points beside the plane (tests/reconstruct_cases.py), and with lines 60 line pairs.  Shapes: (rows 1000, matches 150), (1000, 500), (2000, 1500),
the second one also with lines.  Pair p of a batch is unique pair p % unique.
(a): wall time of the sim process over the unique pairs, per pair; it includes the program's text input and output (every row of every hypothesis is printed).
(b): device time between two HIP events around the call on a side stream, wall time from the call to the end of a stream synchronise, and k_reconstruct alone through
sslam_profile_enable / sslam_profile_drain.  After a warm-up pass, `reps` passes; medians, with the lowest and highest pass.  The poses, points and flags of the first
`unique` pairs of every batch must equal the sim's bit for bit, or the probe exits non-zero.
Not measured: the same batch through separate single calls, capacities beyond 2000."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import reconstruct_cases as rc
import reconstruct_sim as sim
import host_sim
import batch_probe_common as bp
from batch_probe_common import med

SHAPES = ((1000, 150, 0), (1000, 500, 0), (1000, 500, 60), (2000, 1500, 0))


def make(u, rows, matches, nlp):
    if u % 2:
        c = rc._h_scene(7000 + u, matches - matches // 3, matches // 3, unmatched=rows - matches)
        if len(c["kp2"]) < rows:      # the joined scene's frame 2 has as many rows as matches: pad it
            c["kp2"] = np.concatenate([c["kp2"], np.full((rows - len(c["kp2"]), 2), 5.0, np.float32)])
    else:
        c = rc.scene(7000 + u, matches, unmatched=rows - matches, extra2=rows - matches)
    return rc.add_lines(c, 7100 + u, nlp, swap=2) if nlp else c


def same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def main():
    a = bp.parse_args("--batches", "64,1024,8192", 5, 4, loop_lib=False)
    log = bp.Lines(); say = log.say
    fe = pkg.frontend()
    ctx = fe.Context(0)
    U = a.unique
    host_sim.programs(sim.SRC)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)).cuda()
    st = torch.cuda.Stream()
    report, all_equal = {}, True
    for rows, matches, nlp in SHAPES:
        tag = "rows %d matches %d lines %d" % (rows, matches, nlp)
        pairs = [make(u, rows, matches, nlp) for u in range(U)]
        cap = max(max(len(c["kp1"]), len(c["kp2"])) for c in pairs)
        ta = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = sim.run_plain(pairs)
            ta.append((time.perf_counter() - t0) * 1e6 / U)
        say("%s | (a) the sim on one core: %.0f us per pair (min %.0f max %.0f over 3 runs of %d pairs), ok %s, models %s" %
            (tag, med(ta), min(ta), max(ta), U, [int(w["pose"]["ok"]) for w in want], [c["model"] for c in pairs]))
        report[tag] = dict(sim_us_per_pair=med(ta), sim_all_us_per_pair=ta)
        kp1 = np.zeros((U, cap), fe.KP_DTYPE); kp2 = np.zeros((U, cap), fe.KP_DTYPE); m12 = np.full((U, cap), -1, np.int32); inl = np.zeros((U, cap), np.uint8)
        res = np.zeros(U, fe.TWO_VIEW_RESULT_DTYPE); K = np.zeros((U, 4), np.float32); n1 = np.zeros((U, 1), np.int32); n2 = np.zeros((U, 1), np.int32)
        L = max(nlp + 2, 1)
        kl1 = np.zeros((U, L), fe.KL_DTYPE); f1 = np.zeros((U, L, 3)); f2 = np.zeros((U, L, 3)); lp = np.zeros((U, L, 2), np.int32); nl = np.zeros((U, 1), np.int32); nn = np.zeros((U, 1), np.int32)
        for u, c in enumerate(pairs):
            a1, a2 = len(c["kp1"]), len(c["kp2"])
            kp1[u, :a1]["x"] = c["kp1"][:, 0]; kp1[u, :a1]["y"] = c["kp1"][:, 1]; kp2[u, :a2]["x"] = c["kp2"][:, 0]; kp2[u, :a2]["y"] = c["kp2"][:, 1]
            m12[u, :a1] = c["m12"]; inl[u, :a1] = c["inliers"]; n1[u], n2[u] = a1, a2
            res[u]["model"] = c["model"]; res[u]["H21"] = c["H21"]; res[u]["F21"] = c["F21"]; K[u] = c["K"]
            if nlp:
                k = len(c["fn1"])
                kl1[u, :k]["startPointX"], kl1[u, :k]["startPointY"], kl1[u, :k]["endPointX"], kl1[u, :k]["endPointY"] = c["kl1"].T
                f1[u, :k] = c["fn1"]; f2[u, :k] = c["fn2"]; lp[u, :nlp] = c["lp"]; nl[u] = k; nn[u] = nlp
        D = [up(x) for x in (kp1, n1, kp2, n2, m12, res, inl, K)]
        DL = [up(x) for x in (kl1, nl, kl1, nl, f1, f2, lp, nn)]
        for B in a.sizes:
            rep = lambda d: d.repeat(-(-B // U), 1)[:B].contiguous()
            d = [rep(x) for x in D]
            pose = torch.zeros(B * fe.TWO_VIEW_POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            p3d = torch.zeros(B * cap * 12, dtype=torch.uint8, device="cuda"); tri = torch.zeros(B * cap, dtype=torch.uint8, device="cuda")
            lines = None
            if nlp:
                ls, le, lt = (torch.zeros(B * L * 12, dtype=torch.uint8, device="cuda"), torch.zeros(B * L * 12, dtype=torch.uint8, device="cuda"),
                              torch.zeros(B * L, dtype=torch.uint8, device="cuda"))
                lines = [rep(x) for x in DL] + [ls, le, lt]
            torch.cuda.synchronize()
            enqueue = lambda: ctx.two_view_reconstruct_batch_dev(d[0], d[1], d[2], d[3], cap, B, d[4], d[5], d[6], d[7], pose, p3d, tri, lines=lines, lcap=L if nlp else 0,
                                                                 stream=st.cuda_stream)
            bp.timed_pass(st, enqueue)                                    # warm-up
            gp = pose.cpu().numpy().view(fe.TWO_VIEW_POSE_DTYPE); g3 = p3d.cpu().numpy().view(np.float32).reshape(B, cap, 3); gt = tri.cpu().numpy().reshape(B, cap)
            ok = True
            for p in range(min(B, U)):
                w = want[p]; k = len(pairs[p]["kp1"])
                ok = ok and same(gp[p:p + 1], np.array([w["pose"]])) and same(g3[p, :k], w["p3d"]) and same(gt[p, :k], w["tri"])
                if nlp:
                    ok = ok and same(ls.cpu().numpy().view(np.float32).reshape(B, L, 3)[p, :nlp], w["line_s3d"]) and same(lt.cpu().numpy().reshape(B, L)[p, :nlp], w["line_tri"])
            all_equal = all_equal and ok
            tb = [bp.timed_pass(st, enqueue) for _ in range(a.reps)]
            kb = bp.kernel_passes(fe.lib(), ctx.h, st, enqueue, "k_reconstruct", a.reps)
            dev_ms, wall_ms, enq_ms = bp.b_medians(tb)
            report[tag]["B%d" % B] = dict(pairs=B, equal=ok, b_device_ms=dev_ms, b_wall_ms=wall_ms, b_enqueue_ms=enq_ms, b_all_ms=tb, k_reconstruct_ms=med(kb),
                                          k_reconstruct_all_ms=kb, us_per_pair=dev_ms * 1e3 / B)
            say("%s | pairs %6d | (b) batch: %9.3f ms device (min %.3f max %.3f), %9.3f ms wall, %6.3f ms enqueue | k_reconstruct alone %9.3f ms (min %.3f max %.3f) | "
                "%8.2f us per pair | (a) x pairs / (b) device = %7.1f x | equal %s" % (tag, B, dev_ms, min(t[0] for t in tb), max(t[0] for t in tb), wall_ms, enq_ms, med(kb),
                                                                                       min(kb), max(kb), dev_ms * 1e3 / B, med(ta) * B / (dev_ms * 1e3), ok))
            del d, pose, p3d, tri, lines
    ctx.close()
    log.finish("reconstruct_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
