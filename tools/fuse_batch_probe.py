"""Times the candidate search of LocalMapping::SearchInNeighbors for a batch of sessions whose keyframes are on the device -- ONE
sslam_fuse_search_batch_dev launch (b) -- against the only route a caller had before it (a): one synchronous sslam_fuse_search call per job on uploaded
frame handles.  Same keyframes, same queries, same run.

    python tools/fuse_batch_probe.py [--sessions 1,64,1024] [--reps 10] [--unique 2] [--loop-lib PATH] [--out profiles/fuse_batch_probe.txt]

A session is what SearchInNeighbors does for one new keyframe: 20 neighbour jobs -- the current keyframe's ~1000 map points (900 .. 1000 per job)
projected into each of 20 neighbours, all 20 jobs reading ONE descriptor block -- and 1 reverse job of qcap = 1024 queries, the neighbours' map points
projected into the current keyframe, with a descriptor block of its own: 21 keyframe slots of 1000 features, 21 jobs, 2 descriptor blocks.  Inputs are
synthetic (match_cases.fuse_case: features spread over 640 x 480, queries aimed at them with a pixel of noise and up to 20 flipped descriptor bits,
radius 3 x scale for keypoints, 15 / 24 px for keylines); a neighbour is the session's world with 0.5 px of noise on every feature and a few flipped
bits.  Session s of a batch is unique session s % unique.  Two modes: keypoints with the chi-square gates (kind 0, chi2 1: Fuse(KeyFrame*, MapPoints)),
keylines (kind 1: LSDmatcher::Fuse).
(b): device time between two HIP events around the call on a side stream, and wall time from the call to the end of a stream synchronise; after a
warm-up pass, the median of `reps` passes.  (a): wall time of the loop of C calls alone, queries and descriptors in host arrays as a caller of (a) has
them; above 1024 jobs the loop is timed over 1024 jobs (its cost per job does not depend on the batch).  --loop-lib: the library (a) runs on, e.g. a
build of the parent commit (default: the library under test).  Every row of every job of (b) must equal (a)'s, or the probe exits non-zero."""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import match_cases as mc
import batch_probe_common as bp
from batch_probe_common import med

NEIGH, N, QCAP = 20, 1000, 1024
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
INV_SIGMA2 = (np.float32(1) / (SCALE * SCALE)).astype(np.float32)
BOUNDS = (0.0, 640.0, 0.0, 480.0)


def session(rng, kind):
    """-> dict(kfs[21] of (feats, desc, uright), blocks[2], jobs[21] of (slot, queries, block)): slots 0 .. 19 the neighbours, slot 20 the current keyframe"""
    w = mc.fuse_case(rng, kind, N, N)
    cur = mc.fuse_case(rng, kind, N, QCAP)
    xy = ("x", "y") if kind == 0 else ("pt_x", "pt_y")
    kfs, jobs = [], []
    for k in range(NEIGH):
        f = w["feats"].copy()
        for a in xy: f[a] += rng.normal(0, 0.5, N).astype(np.float32)
        d = w["desc"] ^ np.packbits(rng.random((N, 256)) < 0.01, axis=1)
        kfs.append((f, d, w["uright"]))
        nq = int(rng.integers(900, N + 1))
        q = w["q"][:nq].copy()
        for a in ("u", "v"): q[a] += rng.normal(0, 0.5, nq).astype(np.float32)
        jobs.append((k, q, 0))
    kfs.append((cur["feats"], cur["desc"], cur["uright"]))
    jobs.append((NEIGH, cur["q"], 1))
    return dict(kfs=kfs, blocks=[w["qdesc"], cur["qdesc"]], jobs=jobs)


def main():
    a = bp.parse_args("--sessions", "1,64,1024", 10, 2)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend()
    U, K, J = a.unique, NEIGH + 1, NEIGH + 1
    ctx = fe.Context(0)
    p_ = fe._p
    say("session: %d neighbour jobs of 900..%d queries on one descriptor block + 1 reverse job of %d queries; %d keyframe slots of %d features; %d unique sessions"
        % (NEIGH, N, QCAP, K, N, U))
    LA, hA = bp.loop_library(fe, ctx, a, say)
    bounds = (C.c_float * 4)(*BOUNDS)
    st = torch.cuda.Stream()
    report = {}
    all_equal = True
    for kind, chi2, label in ((0, 1, "keypoints, chi-square gates"), (1, 0, "keylines")):
        rng = np.random.default_rng(40 + kind)
        S = [session(rng, kind) for _ in range(U)]
        fdt = fe.KP_DTYPE if kind == 0 else fe.KL_DTYPE
        # (a): handles, host queries and outputs of every unique job, untimed
        handles, argsA, outs = [], [], []
        for s in S:
            hs = []
            for f, d, ur in s["kfs"]:
                h = C.c_void_p()
                if LA.sslam_frame_upload(hA, kind, p_(np.ascontiguousarray(f)), p_(np.ascontiguousarray(d)), len(f), p_(ur) if kind == 0 else None, bounds, C.byref(h)):
                    raise RuntimeError(LA.sslam_last_error())
                hs.append(h)
            handles += hs
            for slot, q, b in s["jobs"]:
                qd = np.ascontiguousarray(s["blocks"][b][:len(q)]); q = np.ascontiguousarray(q)
                bi = np.full(len(q), -9, np.int32); bd = np.full(len(q), -9, np.int32)
                outs.append((bi, bd, q, qd))
                argsA.append((hA, hs[slot], chi2, p_(INV_SIGMA2) if chi2 else None, 8 if chi2 else 0, p_(q), p_(qd), len(q), p_(bi), p_(bd)))

        def run_a(n):
            t0 = time.perf_counter()
            for i in range(n):
                if LA.sslam_fuse_search(*argsA[i % len(argsA)]): raise RuntimeError(LA.sslam_last_error())
            return (time.perf_counter() - t0) * 1e3

        # (b)'s buffers for the unique sessions; a batch repeats them
        fU = np.zeros((U, K, N), fdt); dU = np.zeros((U, K, N, 32), np.uint8); uU = np.full((U, K, N), -1, np.float32)
        qU = np.zeros((U, J, QCAP), fe.PQ_DTYPE); qdU = np.zeros((U, N + QCAP, 32), np.uint8); nqU = np.zeros((U, J), np.int32); b0 = np.zeros((U, J), np.int32)
        for u, s in enumerate(S):
            for k, (f, d, ur) in enumerate(s["kfs"]):
                fU[u, k] = f; dU[u, k] = d
                if kind == 0: uU[u, k] = ur
            qdU[u, :N] = s["blocks"][0]; qdU[u, N:] = s["blocks"][1]
            for j, (slot, q, b) in enumerate(s["jobs"]):
                qU[u, j, :len(q)] = q; nqU[u, j] = len(q); b0[u, j] = 0 if b == 0 else N
        up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(U, -1)).cuda()
        tf, td, tu, tq, tqd = up(fU), up(dU), up(uU), up(qU), up(qdU)
        rows_mode = {}
        for B in a.sizes:
            r = -(-B // U)
            rep = lambda t: t.repeat(r, 1)[:B].contiguous()
            fB, dB, uB, qB, qdB = rep(tf), rep(td), rep(tu), rep(tq), rep(tqd)
            nB = torch.full((B * K,), N, dtype=torch.int32, device="cuda")
            jobs = np.zeros((B, J), fe.FUSE_JOB_DTYPE)
            for s in range(B):
                jobs["kf"][s] = s * K + np.arange(J); jobs["nq"][s] = nqU[s % U]; jobs["qdesc0"][s] = s * (N + QCAP) + b0[s % U]
            jB = torch.from_numpy(jobs.view(np.uint8).reshape(-1)).cuda()
            bi = torch.full((B * J, QCAP), -9, dtype=torch.int32, device="cuda"); bd = torch.full((B * J, QCAP), -9, dtype=torch.int32, device="cuda")
            nf = torch.full((B * J,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def enqueue_b():
                ctx.fuse_search_batch_dev(kind, chi2, fB, dB, nB, N, B * K, qB, QCAP, qdB, B * (N + QCAP), jB, B * J, bi, bd, nf, d_uright=uB if kind == 0 else None,
                                          inv_level_sigma2=INV_SIGMA2 if chi2 else None, bounds=BOUNDS, stream=st.cuda_stream)

            run_b = lambda: bp.timed_pass(st, enqueue_b)

            nA = min(B * J, 1024)
            run_a(len(argsA)); run_b()                               # warm-up; (a) leaves every unique job's rows in outs
            gi, gd, gn = bi.cpu().numpy(), bd.cpu().numpy(), nf.cpu().numpy()
            same = True
            for s in range(B):
                for j in range(J):
                    oi, od = outs[(s % U) * J + j][:2]
                    same = same and np.array_equal(gi[s * J + j, :len(oi)], oi) and np.array_equal(gd[s * J + j, :len(od)], od) and gn[s * J + j] == (oi >= 0).sum()
            all_equal = all_equal and same
            ta, tb = bp.alternate(a.reps, lambda: run_a(nA), run_b)
            dev_b, wall_b, enq_b = bp.b_medians(tb)
            a_us = med(ta) * 1e3 / nA
            rr = dict(kind=kind, chi2=chi2, sessions=B, jobs=B * J, equal_to_the_loop=bool(same), found_per_job=float(gn.mean()), a_jobs_timed=nA, a_us_per_job=a_us, a_all_ms=ta,
                      b_device_ms=dev_b, b_wall_ms=wall_b, b_enqueue_ms=enq_b, b_us_per_job_device=dev_b * 1e3 / (B * J), b_us_per_job_wall=wall_b * 1e3 / (B * J),
                      b_all_ms=[x[:2] for x in tb], ratio_a_over_b_wall=a_us / (wall_b * 1e3 / (B * J)))
            report["kind%d_S%d" % (kind, B)] = rr
            say("%-28s sessions %5d jobs %6d  (a) loop of single calls: %8.2f us/job wall (over %d jobs) | (b) batch: %8.3f ms device, %8.3f ms wall = %7.3f / %7.3f us/job  "
                "[enqueue %.3f ms] | (a) / (b) = %.1f x | equal %s, %.0f candidates/job"
                % (label, B, B * J, a_us, nA, dev_b, wall_b, rr["b_us_per_job_device"], rr["b_us_per_job_wall"], enq_b, rr["ratio_a_over_b_wall"], same, rr["found_per_job"]))
            del fB, dB, uB, qB, qdB, bi, bd, nf, jB
        for h in handles: LA.sslam_frame_destroy(h)
    ctx.close()
    log.finish("fuse_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
