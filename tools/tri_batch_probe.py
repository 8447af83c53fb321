"""Times the point matching of LocalMapping::CreateNewMapPoints for a batch of device-resident keyframe pairs -- two sslam_bow_transform_batch_dev
launches (the queries' slots, the candidates' slots) and one sslam_orb_search_for_triangulation_batch_dev launch (b) -- against the only route a caller
had before it (a): one synchronous sslam_orb_search_for_triangulation call per pair on uploaded frame handles.  Same keyframes, same vocabulary, same run.

    python tools/tri_batch_probe.py [--batches 64,1024,12288] [--reps 10] [--unique 16] [--loop-lib PATH] [--out profiles/tri_batch_probe.txt]

Inputs: `unique` synthetic 640x480 frames of up to 1000 ORB keypoints (the CPU oracle's extraction) as keyframe 2, the same scenes moved by
synth.warp_prev as keyframe 1, 90 % of the keypoints of either free, monocular; F12 and the epipole are match_cases.tri_F12 / TRI_EPIPOLE (the motion
of warp_prev); pair p of a batch is unique pair p % unique.  The vocabulary is tools/batch_probe_common.py's k = 10, L = 6 tree, levelsup = 4: a
feature's node is one of the 100 nodes of level 2.  only_stereo 0, check_orientation 1.
(b): device time between two HIP events around the three launches on one side stream, and wall time from the first call to the end of a stream
synchronise; after a warm-up pass, the median of `reps` passes.  (a): wall time of the loop of C calls alone -- what a caller of (a) also pays per
pair, bringing the two FeatureVectors to the host and flattening them to CSR lists, is done beforehand and NOT timed, and so are the two descents (the
handles are uploaded and the node ids known before the loop): (a) is a lower bound; above 1024 pairs the loop is timed over 1024 pairs (its cost per
pair does not depend on the batch).  --loop-lib: the library (a) runs on, e.g. a build of the parent commit (default: the library under test).  Every
pair's result of (b) must equal (a)'s, or the probe exits non-zero.  Then an untimed pass with sslam_profile_enable for the kernel split of (b)."""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg, oracle_lib
import match_cases as mc
from synth import synth_frame, warp_prev
from bow_batch_cases import csr_from_nodes
import batch_probe_common as bp
from batch_probe_common import big_vocab, med

LEVELSUP, ONLY_STEREO, ORI = 4, 0, 1


def main():
    a = bp.parse_args("--batches", "64,1024,12288", 10, 16)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend(); orc = oracle_lib.Oracle()
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    U = a.unique
    rng = np.random.default_rng(12)
    L, ptr, ch, nd, word, weight = big_vocab(rng)
    F12 = mc.tri_F12(); ex, ey = mc.TRI_EPIPOLE
    sc = orc.orb_params()[0].astype(np.float32); sg = (sc * sc).astype(np.float32)
    pairs = []
    for u in range(U):
        cur = synth_frame(3100 + u)
        k1, d1 = orc.orb_extract(warp_prev(cur), 1000); k2, d2 = orc.orb_extract(cur, 1000)
        pairs.append(dict(k1=k1, d1=d1, f1=(rng.random(len(k1)) < 0.9).astype(np.uint8), k2=k2, d2=d2, f2=(rng.random(len(k2)) < 0.9).astype(np.uint8)))
    cap = max(max(len(p["k1"]), len(p["k2"])) for p in pairs)
    say("pairs: %d unique, keyframe-1 keypoints %d..%d, keyframe-2 keypoints %d..%d, cap = %d; vocabulary k = 10, L = %d, %d nodes, levelsup %d"
        % (U, min(len(p["k1"]) for p in pairs), max(len(p["k1"]) for p in pairs), min(len(p["k2"]) for p in pairs), max(len(p["k2"]) for p in pairs), cap, L, len(ptr) - 1, LEVELSUP))
    ctx = fe.Context(0)
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    # (a)'s library and context
    LA, hA = bp.loop_library(fe, ctx, a, say)
    p_ = fe._p
    say("(a) does NOT count the caller's side of the single call: the two FeatureVectors brought to the host and flattened to CSR lists per pair, and the descents")
    # frame handles, CSR lists (what a caller flattens from the two FeatureVectors) and outputs of every unique pair, untimed
    outs, argsA, handles = [], [], []
    Fc = (C.c_float * 9)(*F12.reshape(9).tolist()); bounds = (C.c_float * 4)(0.0, 640.0, 0.0, 480.0)
    for p in pairs:
        n1, n2 = len(p["k1"]), len(p["k2"])
        p["n1"] = voc.transform(p["d1"], LEVELSUP)[2]; p["n2"] = voc.transform(p["d2"], LEVELSUP)[2]
        p["csr"] = csr_from_nodes(p["n1"], p["n2"])
        h1, h2 = C.c_void_p(), C.c_void_p()
        for h, k, d, n in ((h1, p["k1"], p["d1"], n1), (h2, p["k2"], p["d2"], n2)):
            if LA.sslam_frame_upload(hA, 0, p_(np.ascontiguousarray(k)), p_(np.ascontiguousarray(d)), n, None, bounds, C.byref(h)): raise RuntimeError(LA.sslam_last_error())
        handles += [h1, h2]
        out = np.full(n1, -2, np.int32); nm = C.c_int(); outs.append((out, nm))
        pk, pf, ik, jf = p["csr"]
        argsA.append((hA, h1, h2, p_(p["f1"]), p_(p["f2"]), p_(pk), p_(pf), len(pk) - 1, p_(ik), p_(jf), Fc, C.c_float(ex), C.c_float(ey), p_(sc), p_(sg), len(sc),
                      ONLY_STEREO, ORI, p_(out), C.byref(nm)))
    say("nodes per pair (shared by both sides): %d..%d" % (min(len(p["csr"][0]) - 1 for p in pairs), max(len(p["csr"][0]) - 1 for p in pairs)))

    def run_a(n):
        t0 = time.perf_counter()
        for i in range(n):
            if LA.sslam_orb_search_for_triangulation(*argsA[i % U]): raise RuntimeError(LA.sslam_last_error())
        return (time.perf_counter() - t0) * 1e3

    # (b)'s pool for the unique pairs: slots [0, U) keyframe 1, [U, 2U) keyframe 2; a batch repeats each half
    kpU = np.zeros((2, U, cap), fe.KP_DTYPE); dU = np.zeros((2, U, cap, 32), np.uint8); frU = np.zeros((2, U, cap), np.uint8); nU = np.zeros((2, U), np.int32)
    for u, p in enumerate(pairs):
        for s, (k, d, f) in enumerate(((p["k1"], p["d1"], p["f1"]), (p["k2"], p["d2"], p["f2"]))):
            n = len(k); nU[s, u] = n; kpU[s, u, :n] = k; dU[s, u, :n] = d; frU[s, u, :n] = f
    up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(2, U, -1)).cuda()
    tkp, td, tfr = up(kpU), up(dU), up(frU); tn = torch.from_numpy(nU).cuda()
    st = torch.cuda.Stream()
    report = {}
    all_equal = True
    for B in a.sizes:
        assert B % U == 0
        r = B // U
        half = lambda t: torch.cat([t[0].repeat(r, 1), t[1].repeat(r, 1)])          # [2B, ...]: B keyframe-1 slots, then B keyframe-2 slots
        kpB, dB, frB = half(tkp), half(td), half(tfr); nB = torch.cat([tn[0].repeat(r), tn[1].repeat(r)])
        nodeB = torch.full((2 * B, cap), -9, dtype=torch.int32, device="cuda")
        rows = np.zeros(B, fe.TRI_PAIR_DTYPE); rows["kf1"] = np.arange(B); rows["kf2"] = B + np.arange(B); rows["F12"] = F12.reshape(9); rows["ex"] = ex; rows["ey"] = ey
        prB = torch.from_numpy(rows.view(np.uint8)).cuda()
        m12 = torch.full((B, cap), -9, dtype=torch.int32, device="cuda"); nmB = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def enqueue_b():
            ctx.bow_transform_batch_dev(voc, dB, nB, cap, B, nodeB, levelsup=LEVELSUP, stream=st.cuda_stream)
            ctx.bow_transform_batch_dev(voc, dB[B:], nB[B:], cap, B, nodeB[B:], levelsup=LEVELSUP, stream=st.cuda_stream)
            ctx.search_for_triangulation_batch_dev(kpB, dB, nodeB, nB, cap, 2 * B, prB, B, sc, sg, m12, nmB, d_free=frB, only_stereo=bool(ONLY_STEREO),
                                                   check_orientation=bool(ORI), stream=st.cuda_stream)

        run_b = lambda: bp.timed_pass(st, enqueue_b)

        nA = min(B, 1024)
        run_a(max(U, 64)); run_b()                               # warm-up: code objects, the loop's arena
        got, gnm = m12.cpu().numpy(), nmB.cpu().numpy()          # EVERY pair of the batch; (a) left unique pair u's rows in outs[u]
        same = all(np.array_equal(got[p, :nU[0, p % U]], outs[p % U][0]) and gnm[p] == outs[p % U][1].value for p in range(B))
        all_equal = all_equal and same
        ta, tb = bp.alternate(a.reps, lambda: run_a(nA), run_b)
        dev_b, wall_b, enq_b = bp.b_medians(tb)
        a_us = med(ta) * 1e3 / nA
        fe.lib().sslam_profile_enable(ctx.h, 1)
        run_b(); split_b = pipeline.profile_drain(fe, ctx)
        fe.lib().sslam_profile_enable(ctx.h, 0)
        rr = dict(B=B, equal_to_the_loop=same, matches_per_pair=float(gnm.mean()), a_pairs_timed=nA, a_us_per_pair=a_us, a_all_ms=ta,
                  b_device_ms=dev_b, b_wall_ms=wall_b, b_enqueue_ms=enq_b, b_us_per_pair_device=dev_b * 1e3 / B, b_us_per_pair_wall=wall_b * 1e3 / B, b_all_ms=[x[:2] for x in tb],
                  b_kernels_ms={k: v[0] for k, v in split_b.items()}, b_launches={k: v[1] for k, v in split_b.items()},
                  ratio_a_over_b_wall=a_us / (wall_b * 1e3 / B))
        report["B%d" % B] = rr
        say("B %5d  (a) loop of single calls: %8.2f us/pair wall (over %d pairs) | (b) batch: %8.3f ms device, %8.3f ms wall = %7.3f / %7.3f us/pair  [enqueue %.3f ms] | "
            "(a) / (b) = %.1f x | equal %s, %.0f matches/pair" % (B, a_us, nA, dev_b, wall_b, rr["b_us_per_pair_device"], rr["b_us_per_pair_wall"], enq_b, rr["ratio_a_over_b_wall"], same,
                                                                 rr["matches_per_pair"]))
        say("        (b) kernels: " + ", ".join("%s %.3f ms x%d = %.3f us/pair" % (k, v[0], v[1], v[0] * 1e3 / B) for k, v in sorted(split_b.items())))
        del kpB, dB, frB, nodeB, m12, prB
    for h in handles: LA.sslam_frame_destroy(h)
    voc.close(); ctx.close()
    log.finish("tri_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
