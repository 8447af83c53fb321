"""Times the first matcher of LoopClosing::ComputeSim3 for a batch of pairs of device-resident keyframes -- one
sslam_orb_search_by_bow_keyframes_batch_dev launch (b) -- against the only route a caller had before it (a): per pair one synchronous
sslam_orb_search_by_bow_keyframes call on host arrays.  Same keyframes, same node ids, same run.

    python tools/bow_kf_batch_probe.py [--batches 20,64,1024,12288] [--reps 10] [--unique 16] [--loop-lib PATH] [--out profiles/bow_kf_batch_probe.txt]

Inputs: tools/bow_batch_probe.py's scenes and vocabulary -- `unique` synthetic 640x480 frames of up to 1000 ORB keypoints (the CPU oracle's
extraction) as keyframe 2, the same scenes moved by synth.warp_prev as keyframe 1, 90 % of the rows valid on BOTH sides; the k = 10, L = 6 tree,
levelsup = 4.  Pair p of a batch is unique pair p % unique, in slots 2p and 2p + 1 of a pool of 2 B slots (no slot is shared between pairs).  The node
ids are in the pool before the clock starts, as a keyframe's are (KeyFrame::ComputeBoW ran when it was inserted): sslam_bow_transform_batch_dev is
NOT part of (b), and sslam_compute_bow is not part of (a).  nnratio 0.75 with the rotation check (ORBmatcher matcher(0.75, true), src/LoopClosing.cc:240).
(b): device time between two HIP events around the launch on one side stream, and wall time from the call to the end of a stream synchronise; after
a warm-up pass, the median of `reps` passes.  (a): wall time of the loop of C calls alone -- flattening the two FeatureVectors to CSR lists, which a
caller also pays per pair, is done beforehand and NOT timed, and so are the downloads of the two keyframes, so (a) is a lower bound; above 1024
pairs the loop is timed over 1024 pairs (its cost per pair does not depend on the batch).  --loop-lib: the library (a) runs on, e.g. a build of the
parent commit (default: the library under test).  Then an untimed pass with sslam_profile_enable for the kernel's own time."""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg, oracle_lib
from synth import synth_frame, warp_prev
from bow_batch_cases import csr_from_nodes
import batch_probe_common as bp
from batch_probe_common import big_vocab, med

LEVELSUP, NNRATIO, ORI = 4, 0.75, 1          # LoopClosing::ComputeSim3: ORBmatcher matcher(0.75, true)


def main():
    a = bp.parse_args("--batches", "20,64,1024,12288", 10, 16)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend(); orc = oracle_lib.Oracle()
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    U = a.unique
    rng = np.random.default_rng(11)
    L, ptr, ch, nd, word, weight = big_vocab(rng)
    ctx = fe.Context(0)
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    pairs = []
    for u in range(U):
        cur = synth_frame(3000 + u)
        k1, d1 = orc.orb_extract(warp_prev(cur), 1000); k2, d2 = orc.orb_extract(cur, 1000)
        p = dict(k1=k1, d1=d1, v1=(rng.random(len(k1)) < 0.9).astype(np.uint8), k2=k2, d2=d2, v2=(rng.random(len(k2)) < 0.9).astype(np.uint8))
        p["n1"] = voc.transform(d1, LEVELSUP)[2]; p["n2"] = voc.transform(d2, LEVELSUP)[2]
        p["csr"] = csr_from_nodes(p["n1"], p["n2"])          # what a caller flattens from the two FeatureVectors, untimed
        pairs.append(p)
    cap = max(max(len(p["k1"]), len(p["k2"])) for p in pairs)
    say("pairs: %d unique, keyframe-1 keypoints %d..%d, keyframe-2 keypoints %d..%d, cap = %d, 90 %% of the rows valid on both sides; vocabulary k = 10, L = %d, %d nodes, "
        "levelsup %d; nodes per pair (shared by both sides): %d..%d"
        % (U, min(len(p["k1"]) for p in pairs), max(len(p["k1"]) for p in pairs), min(len(p["k2"]) for p in pairs), max(len(p["k2"]) for p in pairs), cap, L, len(ptr) - 1,
           LEVELSUP, min(len(p["csr"][0]) - 1 for p in pairs), max(len(p["csr"][0]) - 1 for p in pairs)))
    LA, hA = bp.loop_library(fe, ctx, a, say)
    p_ = fe._p
    outs, argsA = [], []
    for p in pairs:
        n1, n2 = len(p["k1"]), len(p["k2"])
        out = np.full(n1, -1, np.int32); outs.append(out)
        p1, p2, i1, i2 = p["csr"]
        p["nmA"] = C.c_int()
        argsA.append((hA, p_(p["k1"]), p_(p["d1"]), p_(p["v1"]), n1, p_(p["k2"]), p_(p["d2"]), p_(p["v2"]), n2, p_(p1), p_(p2), len(p1) - 1, p_(i1), p_(i2),
                      C.c_float(NNRATIO), ORI, p_(out), C.byref(p["nmA"])))

    def run_a(n):
        t0 = time.perf_counter()
        for i in range(n):
            if LA.sslam_orb_search_by_bow_keyframes(*argsA[i % U]): raise RuntimeError(LA.sslam_last_error())
        return (time.perf_counter() - t0) * 1e3

    # (b)'s pool for the unique pairs: slots 2u (keyframe 1) and 2u + 1 (keyframe 2); a batch repeats them
    kpU = np.zeros((U, 2, cap), fe.KP_DTYPE); dU = np.zeros((U, 2, cap, 32), np.uint8); nodeU = np.full((U, 2, cap), -9, np.int32); vU = np.zeros((U, 2, cap), np.uint8)
    nU = np.zeros((U, 2), np.int32)
    for u, p in enumerate(pairs):
        for s, (k, d, nn, v) in enumerate(((p["k1"], p["d1"], p["n1"], p["v1"]), (p["k2"], p["d2"], p["n2"], p["v2"]))):
            n = len(k); nU[u, s] = n
            kpU[u, s, :n] = k; dU[u, s, :n] = d; nodeU[u, s, :n] = nn; vU[u, s, :n] = v
    up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(U, -1)).cuda()
    tU = [up(x) for x in (kpU, dU, nodeU, vU, nU)]
    st = torch.cuda.Stream()
    report = {}
    equal = True
    for B in a.sizes:
        idx = torch.arange(B, device="cuda") % U
        kpB, dB, nodeB, vB, nB = [t[idx].contiguous() for t in tU]            # [B, 2 * cap * width] bytes: slots 2p, 2p + 1
        pairsB = torch.arange(2 * B, dtype=torch.int32, device="cuda")         # pair p = (2p, 2p + 1)
        m12 = torch.full((B, cap), -9, dtype=torch.int32, device="cuda"); m21 = torch.full((B, cap), -9, dtype=torch.int32, device="cuda")
        nmB = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def enqueue_b():
            ctx.search_by_bow_keyframes_batch_dev(kpB, dB, nodeB, nB, cap, 2 * B, pairsB, B, m12, m21, nmB, d_valid=vB, nnratio=NNRATIO, check_orientation=bool(ORI),
                                                  stream=st.cuda_stream)

        run_b = lambda: bp.timed_pass(st, enqueue_b)

        nA = min(B, 1024)
        run_a(max(U, 64)); run_b()                               # warm-up: code objects, the loop's arenas and pinned mirrors
        last = [(B - 1 - i) for i in range(min(U, B))]            # the LAST pairs of the batch; (a) left unique pair u's rows in outs[u]
        got, gnm = m12.cpu().numpy(), nmB.cpu().numpy()
        same = all(np.array_equal(got[p, :nU[p % U, 0]], outs[p % U]) and gnm[p] == pairs[p % U]["nmA"].value == int((outs[p % U] >= 0).sum()) for p in last)
        equal = equal and same
        ta, tb = bp.alternate(a.reps, lambda: run_a(nA), run_b)
        dev_b, wall_b, enq_b = bp.b_medians(tb)
        a_us = med(ta) * 1e3 / nA
        fe.lib().sslam_profile_enable(ctx.h, 1)
        run_b(); split_b = pipeline.profile_drain(fe, ctx)
        fe.lib().sslam_profile_enable(ctx.h, 0)
        r = dict(B=B, equal_to_the_loop=same, matches_per_pair=float(gnm.mean()), a_pairs_timed=nA, a_us_per_pair=a_us, a_all_ms=ta,
                 b_device_ms=dev_b, b_wall_ms=wall_b, b_enqueue_ms=enq_b, b_us_per_pair_device=dev_b * 1e3 / B, b_us_per_pair_wall=wall_b * 1e3 / B, b_all_ms=[x[:2] for x in tb],
                 b_kernels_ms={k: v[0] for k, v in split_b.items()}, b_launches={k: v[1] for k, v in split_b.items()},
                 ratio_a_over_b_wall=a_us / (wall_b * 1e3 / B))
        report["B%d" % B] = r
        say("B %5d  (a) loop of single calls: %8.2f us/pair wall (over %d pairs) | (b) batch: %8.3f ms device, %8.3f ms wall = %7.3f / %7.3f us/pair  [enqueue %.3f ms] | "
            "(a) / (b) = %.1f x | equal %s, %.0f matches/pair" % (B, a_us, nA, dev_b, wall_b, r["b_us_per_pair_device"], r["b_us_per_pair_wall"], enq_b, r["ratio_a_over_b_wall"], same,
                                                                 r["matches_per_pair"]))
        say("        (b) kernels: " + ", ".join("%s %.3f ms x%d = %.3f us/pair" % (k, v[0], v[1], v[0] * 1e3 / B) for k, v in sorted(split_b.items())))
        del kpB, dB, nodeB, vB, m12, m21
    say("not measured: the global-memory form (cap > 1638), pairs that share slots (one current keyframe against K candidates reads one slot K times), several streams")
    voc.close(); ctx.close()
    log.finish("bow_kf_batch_probe", report, a.out, equal)


if __name__ == "__main__":
    main()
