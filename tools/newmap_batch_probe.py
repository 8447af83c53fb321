"""Times the search + triangulate chain of LocalMapping::CreateNewMapPoints / CreateNewMapLines2 for many sessions at once: per session one new keyframe and 20
neighbours on the device-resident pool, 1000 key points and 200 key lines per keyframe.

    python tools/newmap_batch_probe.py [--sessions 16,64] [--reps 5] [--unique 4] [--out profiles/newmap_batch_probe.txt]

Points: round r = one sslam_orb_search_for_triangulation_batch_dev + one sslam_new_map_points_batch_dev over all sessions (pair s = session s's keyframe against its r-th
neighbour), both on one side stream with one d_free.
  (b) stream order: the 20 rounds enqueued back to back, one synchronise at the end -- the use include/sslam_frontend.h documents
  (a) round trip:   the same launches, but after every matcher launch the stream is synchronised, d_matches12 of the round comes to the host and the keyframes' free flags
                    go back up, which is what a caller had to do between rounds before sslam_new_map_points_batch_dev existed.  The host's own triangulation of (a) is NOT
                    timed (the geometry still runs on the device), so (a) - (b) is the cost of the 20 round trips alone: a lower bound of what the call removes.
Lines: one sslam_line_match_batch_dev for all sessions x 20 pairs, then 20 sslam_new_map_lines_batch_dev with one d_lfree: (b) in stream order, (a) with a synchronise, the
round's line pairs down and the line flags up per round.
Both routes must leave the same stages, counts and flags, or the probe exits non-zero.  Device time between two HIP events and wall time to the end of the last synchronise;
after a warm-up pass the median of `reps` alternating passes.  Then an untimed pass with sslam_profile_enable for the kernels' own times, the matcher's beside the new ones.
Inputs: `unique` synthetic scenes (tests/newmap_cases.py: a cloud of points and segments seen from 21 keyframes on an arc, the middle one the new keyframe), descriptors
equal in every view, node = point id mod 100; session s is scene s mod unique in slots of its own."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import newmap_cases as nc
import tri_batch_cases as tc
import batch_probe_common as bp
from batch_probe_common import med

NKF, CUR, ROUNDS, CAP, LCAP = 21, 10, 20, 1000, 200
NEIGH = [k for k in range(NKF) if k != CUR]


def main():
    a = bp.parse_args("--sessions", "16,64", 5, 4, loop_lib=False)
    log = bp.Lines(); say = log.say
    fe = pkg.frontend()
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    U = a.unique
    rng = np.random.default_rng(51)
    kpU = np.zeros((U, NKF, CAP), fe.KP_DTYPE); dU = np.zeros((U, NKF, CAP, 32), np.uint8); ndU = np.zeros((U, NKF, CAP), np.int32); poseU = np.zeros((U, NKF, 21), np.float32)
    triU = np.zeros((U, ROUNDS), fe.TRI_PAIR_DTYPE)
    klU = np.zeros((U, NKF, LCAP), fe.KL_DTYPE); fnU = np.zeros((U, NKF, LCAP, 3), np.float64); ldU = np.zeros((U, NKF, LCAP, 32), np.uint8)
    for u in range(U):
        P = nc.point_pool(300 + u, nkf=NKF, cap=CAP, npts=CAP + 150, counts=[CAP] * NKF)
        D = rng.integers(0, 256, size=(CAP + 150, 32), dtype=np.uint8)
        for k in range(NKF):
            kpU[u, k]["x"], kpU[u, k]["y"], kpU[u, k]["octave"], kpU[u, k]["size"] = P["kp"][k][:, 0], P["kp"][k][:, 1], P["oct"][k], 31
            dU[u, k] = D[P["ids"][k]]; ndU[u, k] = P["ids"][k] % 100
        poseU[u] = P["poses"]
        for r, k in enumerate(NEIGH):
            F, ex, ey = nc.f12_of(P["poses"][CUR], P["poses"][k])
            triU[u, r]["F12"], triU[u, r]["ex"], triU[u, r]["ey"] = F.reshape(9), ex, ey
        L = nc.line_pool(400 + u, nkf=NKF, lcap=LCAP, nseg=LCAP + 30, counts=[LCAP] * NKF)
        DL = rng.integers(0, 256, size=(LCAP + 30, 32), dtype=np.uint8)
        for k in range(NKF):
            for f, c in (("startPointX", 0), ("startPointY", 1), ("endPointX", 2), ("endPointY", 3)): klU[u, k][f] = L["kl"][k][:, c]
            klU[u, k]["octave"] = L["oct"][k]; fnU[u, k] = L["fn"][k]; ldU[u, k] = DL[L["ids"][k]]
    median = 5.0
    say("scenes: %d unique, %d keyframes each (keyframe %d against %d neighbours), %d key points and %d key lines per keyframe" % (U, NKF, CUR, ROUNDS, CAP, LCAP))
    ctx = fe.Context(0)
    st = torch.cuda.Stream()
    sf, sg = tc.SCALE, tc.SIGMA2
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    report, all_equal = {}, True
    for S in a.sizes:
        assert S % U == 0
        rep = lambda x: np.concatenate([x] * (S // U))          # session s = scene s % U, slots [s * NKF, (s + 1) * NKF)
        nk = S * NKF
        d_kp, d_desc, d_node, d_pose = up(rep(kpU)), up(rep(dU)), up(rep(ndU)), up(rep(poseU))
        d_n = up(np.full(nk, CAP, np.int32))
        free0 = torch.ones(nk * CAP, dtype=torch.uint8, device="cuda"); d_free = free0.clone()
        h_free = torch.empty(nk * CAP, dtype=torch.uint8).pin_memory(); h_m12 = torch.empty(S * CAP, dtype=torch.int32).pin_memory()
        tri, nmp = [], []
        for r, k in enumerate(NEIGH):
            rows = rep(triU[:, r]).copy(); rows["kf1"] = np.arange(S) * NKF + CUR; rows["kf2"] = np.arange(S) * NKF + k
            tri.append(up(rows))
            pr = np.zeros(S, fe.NEWMAP_PAIR_DTYPE); pr["kf1"], pr["kf2"], pr["median_depth2"] = rows["kf1"], rows["kf2"], median
            nmp.append(up(pr))
        m12 = torch.full((ROUNDS, S * CAP), -9, dtype=torch.int32, device="cuda"); nm = torch.zeros((ROUNDS, S), dtype=torch.int32, device="cuda")
        x3d = torch.zeros((ROUNDS, S * CAP * 3), dtype=torch.float32, device="cuda"); nrm = torch.zeros_like(x3d); dist = torch.zeros((ROUNDS, S * CAP * 2), dtype=torch.float32, device="cuda")
        stage = torch.zeros((ROUNDS, S * CAP), dtype=torch.uint8, device="cuda"); nnew = torch.zeros((ROUNDS, S), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def points(round_trip):
            with torch.cuda.stream(st):
                d_free.copy_(free0, non_blocking=True)
            for r in range(ROUNDS):
                ctx.search_for_triangulation_batch_dev(d_kp, d_desc, d_node, d_n, CAP, nk, tri[r], S, sf, sg, m12[r], nm[r], d_free=d_free, stream=st.cuda_stream)
                if round_trip:
                    with torch.cuda.stream(st):
                        h_m12.copy_(m12[r], non_blocking=True)
                    st.synchronize()
                ctx.new_map_points_batch_dev(d_kp, d_n, CAP, nk, d_pose, nmp[r], S, m12[r], sf, sg, 1.2, x3d[r], stage[r], nrm[r], dist[r], nnew[r], d_free=d_free, stream=st.cuda_stream)
                if round_trip:
                    with torch.cuda.stream(st):
                        h_free.copy_(d_free, non_blocking=True)
                    st.synchronize()
                    with torch.cuda.stream(st):
                        d_free.copy_(h_free, non_blocking=True)

        def snapshot(*ts):
            return [t.cpu().numpy().copy() for t in ts]

        bp.timed_pass(st, lambda: points(True)); ra = snapshot(stage, nnew, d_free, m12)
        bp.timed_pass(st, lambda: points(False)); rb = snapshot(stage, nnew, d_free, m12)
        same_p = all(np.array_equal(x, y) for x, y in zip(ra, rb))
        ta, tb = bp.alternate(a.reps, lambda: bp.timed_pass(st, lambda: points(True)), lambda: bp.timed_pass(st, lambda: points(False)))
        fe.lib().sslam_profile_enable(ctx.h, 1)
        bp.timed_pass(st, lambda: points(False)); split_p = pipeline.profile_drain(fe, ctx)
        fe.lib().sslam_profile_enable(ctx.h, 0)
        created = rb[1].sum(1)
        say("S %4d points: matches per session and round %s .. %s, created %d in round 1, %d in round 2, %d in round 20; routes equal %s"
            % (S, int((rb[3] >= 0).reshape(ROUNDS, S, CAP).sum(2).min()), int((rb[3] >= 0).reshape(ROUNDS, S, CAP).sum(2).max()), created[0], created[1], created[-1], same_p))
        say("        (a) round trip per round: %8.3f ms wall | (b) stream order: %8.3f ms device, %8.3f ms wall [enqueue %.3f ms] | (a) - (b) = %.3f ms = %.1f us per round and session"
            % (med([x[1] for x in ta]), bp.b_medians(tb)[0], bp.b_medians(tb)[1], bp.b_medians(tb)[2], med([x[1] for x in ta]) - bp.b_medians(tb)[1],
               (med([x[1] for x in ta]) - bp.b_medians(tb)[1]) * 1e3 / (ROUNDS * S)))
        say("        (b) kernels: " + ", ".join("%s %.3f ms x%d = %.3f us per pair" % (k, v[0], v[1], v[0] * 1e3 / (ROUNDS * S)) for k, v in sorted(split_p.items())))

        # lines: the matcher takes descriptors by pair, round after round: pair r * S + s
        NP = ROUNDS * S
        ld = rep(ldU).reshape(S, NKF, LCAP, 32)
        d_l1 = up(np.concatenate([ld[:, CUR]] * ROUNDS)); d_l2 = up(np.concatenate([ld[:, k] for k in NEIGH]))
        d_ln = up(np.full(NP, LCAP, np.int32))
        d_kl, d_fn, d_nl = up(rep(klU)), up(rep(fnU)), up(np.full(nk, LCAP, np.int32))
        lfree0 = torch.ones(nk * LCAP, dtype=torch.uint8, device="cuda"); d_lfree = lfree0.clone(); h_lfree = torch.empty(nk * LCAP, dtype=torch.uint8).pin_memory()
        d_lp = torch.full((NP * LCAP * 2,), -9, dtype=torch.int32, device="cuda"); d_cnt = torch.zeros(NP, dtype=torch.int32, device="cuda"); h_lp = torch.empty(S * LCAP * 2, dtype=torch.int32).pin_memory()
        R = S * LCAP
        s3d = torch.zeros((ROUNDS, R * 3), dtype=torch.float32, device="cuda"); e3d = torch.zeros_like(s3d); ldist = torch.zeros((ROUNDS, R * 2), dtype=torch.float32, device="cuda")
        lnrm = torch.zeros((ROUNDS, R * 3), dtype=torch.float64, device="cuda"); lstage = torch.zeros((ROUNDS, R), dtype=torch.uint8, device="cuda"); lnew = torch.zeros((ROUNDS, S), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        vp = lambda t: C.c_void_p(t.data_ptr())

        def lines(round_trip):
            with torch.cuda.stream(st):
                d_lfree.copy_(lfree0, non_blocking=True)
            rc = fe.lib().sslam_line_match_batch_dev(ctx.h, vp(d_l1), vp(d_ln), vp(d_l2), vp(d_ln), LCAP, NP, C.c_double(0.1), 0, vp(d_lp), vp(d_cnt), C.c_void_p(st.cuda_stream))
            assert rc == 0
            for r in range(ROUNDS):
                if round_trip:
                    with torch.cuda.stream(st):
                        h_lp.copy_(d_lp[r * R * 2:(r + 1) * R * 2], non_blocking=True)
                    st.synchronize()
                ctx.new_map_lines_batch_dev(d_kl, d_fn, d_nl, LCAP, nk, d_pose, nmp[r], S, d_lp.data_ptr() + 8 * r * R, d_cnt.data_ptr() + 4 * r * S, sf, s3d[r], e3d[r], lstage[r], lnrm[r],
                                            ldist[r], lnew[r], d_lfree=d_lfree, stream=st.cuda_stream)
                if round_trip:
                    with torch.cuda.stream(st):
                        h_lfree.copy_(d_lfree, non_blocking=True)
                    st.synchronize()
                    with torch.cuda.stream(st):
                        d_lfree.copy_(h_lfree, non_blocking=True)

        bp.timed_pass(st, lambda: lines(True)); la = snapshot(lstage, lnew, d_lfree)
        bp.timed_pass(st, lambda: lines(False)); lb = snapshot(lstage, lnew, d_lfree)
        same_l = all(np.array_equal(x, y) for x, y in zip(la, lb))
        tla, tlb = bp.alternate(a.reps, lambda: bp.timed_pass(st, lambda: lines(True)), lambda: bp.timed_pass(st, lambda: lines(False)))
        fe.lib().sslam_profile_enable(ctx.h, 1)
        bp.timed_pass(st, lambda: lines(False)); split_l = pipeline.profile_drain(fe, ctx)
        fe.lib().sslam_profile_enable(ctx.h, 0)
        lcreated = lb[1].sum(1)
        say("S %4d lines:  line pairs per session and round %d .. %d, created %d in round 1, %d in round 2, %d in round 20; routes equal %s"
            % (S, int(d_cnt.min()), int(d_cnt.max()), lcreated[0], lcreated[1], lcreated[-1], same_l))
        say("        (a) round trip per round: %8.3f ms wall | (b) stream order: %8.3f ms device, %8.3f ms wall [enqueue %.3f ms] | (a) - (b) = %.3f ms = %.1f us per round and session"
            % (med([x[1] for x in tla]), bp.b_medians(tlb)[0], bp.b_medians(tlb)[1], bp.b_medians(tlb)[2], med([x[1] for x in tla]) - bp.b_medians(tlb)[1],
               (med([x[1] for x in tla]) - bp.b_medians(tlb)[1]) * 1e3 / (ROUNDS * S)))
        say("        (b) kernels: " + ", ".join("%s %.3f ms x%d = %.3f us per pair" % (k, v[0], v[1], v[0] * 1e3 / (ROUNDS * S)) for k, v in sorted(split_l.items())))
        all_equal = all_equal and same_p and same_l
        report["S%d" % S] = dict(sessions=S, points=dict(equal=same_p, created_per_round=created.tolist(), a_wall_ms=[x[1] for x in ta], b_device_ms=[x[0] for x in tb], b_wall_ms=[x[1] for x in tb],
                                                         kernels_ms={k: v[0] for k, v in split_p.items()}, launches={k: v[1] for k, v in split_p.items()}),
                                 lines=dict(equal=same_l, created_per_round=lcreated.tolist(), a_wall_ms=[x[1] for x in tla], b_device_ms=[x[0] for x in tlb], b_wall_ms=[x[1] for x in tlb],
                                            kernels_ms={k: v[0] for k, v in split_l.items()}, launches={k: v[1] for k, v in split_l.items()}))
        del d_kp, d_desc, d_node, m12, x3d, nrm, dist, stage, d_l1, d_l2, d_kl, d_fn, d_lp, s3d, e3d, lnrm
    ctx.close()
    log.finish("newmap_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
