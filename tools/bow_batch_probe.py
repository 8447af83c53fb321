"""Times TrackReferenceKeyFrame's matching for a batch of device-resident frame pairs -- two sslam_bow_transform_batch_dev launches and one
sslam_orb_search_by_bow_batch_dev launch (b) -- against the only route a caller had before them (a): per pair two synchronous sslam_compute_bow
calls and one synchronous sslam_orb_search_by_bow call.  Same frames, same vocabulary, same run.

    python tools/bow_batch_probe.py [--batches 64,1024,12288] [--reps 10] [--unique 16] [--loop-lib PATH] [--out profiles/bow_batch_probe.txt]

Inputs: `unique` synthetic 640x480 frames of up to 1000 ORB keypoints (the CPU oracle's extraction) as the frame side, the same scenes moved by
synth.warp_prev as the keyframe side, 90 % of the keyframe keypoints valid; pair p of a batch is unique pair p % unique.  The vocabulary is a
k = 10, L = 6 tree (1 111 111 nodes, the shape of ORBvoc) of clustered random descriptors without stopped words, levelsup = 4: a feature's node is
one of the 100 nodes of level 2.
(b): device time between two HIP events around the three launches on one side stream, and wall time from the first call to the end of a stream
synchronise; after a warm-up pass, the median of `reps` passes.  (a): wall time of the loop of C calls alone -- the CSR flattening between
sslam_compute_bow and sslam_orb_search_by_bow, which a caller also pays per pair, is done beforehand and NOT timed, so (a) is a lower bound; above
1024 pairs the loop is timed over 1024 pairs (its cost per pair does not depend on the batch).  --loop-lib: the library (a) runs on, e.g. a build
of the parent commit (default: the library under test).  Then an untimed pass with sslam_profile_enable for the kernel split of (b)."""
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

LEVELSUP, NNRATIO, ORI = 4, 0.7, 1          # Tracking::TrackReferenceKeyFrame: ORBmatcher matcher(0.7, true)


def main():
    a = bp.parse_args("--batches", "64,1024,12288", 10, 16)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend(); orc = oracle_lib.Oracle()
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    U = a.unique
    rng = np.random.default_rng(11)
    L, ptr, ch, nd, word, weight = big_vocab(rng)
    pairs = []
    for u in range(U):
        cur = synth_frame(3000 + u)
        kk, kd = orc.orb_extract(warp_prev(cur), 1000); fk, fd = orc.orb_extract(cur, 1000)
        pairs.append(dict(kk=kk, kd=kd, kv=(rng.random(len(kk)) < 0.9).astype(np.uint8), fk=fk, fd=fd))
    cap = max(max(len(p["kk"]), len(p["fk"])) for p in pairs)
    say("pairs: %d unique, keyframe keypoints %d..%d, frame keypoints %d..%d, cap = %d; vocabulary k = 10, L = %d, %d nodes, levelsup %d"
        % (U, min(len(p["kk"]) for p in pairs), max(len(p["kk"]) for p in pairs), min(len(p["fk"]) for p in pairs), max(len(p["fk"]) for p in pairs), cap, L, len(ptr) - 1, LEVELSUP))
    ctx = fe.Context(0)
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    # (a)'s library, context and vocabulary
    LA, hA = bp.loop_library(fe, ctx, a, say)
    p_ = fe._p
    vA = voc.h
    if a.loop_lib:
        vA = C.c_void_p()
        assert LA.sslam_vocab_create(hA, len(ptr) - 1, L, p_(ptr), p_(ch), p_(nd), p_(word), p_(weight), C.byref(vA)) == 0, LA.sslam_last_error()
    # the CSR lists of every unique pair (what a caller flattens from the two FeatureVectors), untimed; and (a)'s outputs
    outs, argsA = [], []
    for p in pairs:
        nk, nf = len(p["kk"]), len(p["fk"])
        p["kn"] = voc.transform(p["kd"], LEVELSUP)[2]; p["fn"] = voc.transform(p["fd"], LEVELSUP)[2]
        p["csr"] = csr_from_nodes(p["kn"], p["fn"])
        m = max(nk, nf)
        p["bow"] = [np.zeros(m, np.int32), np.zeros(m, np.float64), C.c_int(), np.zeros(m, np.int32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32), C.c_int()]
        out = np.full(nf, -1, np.int32); outs.append(out)
        bw, bv, nb, fnn, fp, ff, nfv = p["bow"]
        pk, pf, ik, jf = p["csr"]
        argsA.append(((hA, vA, p_(p["kd"]), nk, LEVELSUP, p_(bw), p_(bv), C.byref(nb), p_(fnn), p_(fp), p_(ff), C.byref(nfv)),
                      (hA, vA, p_(p["fd"]), nf, LEVELSUP, p_(bw), p_(bv), C.byref(nb), p_(fnn), p_(fp), p_(ff), C.byref(nfv)),
                      (hA, p_(p["kk"]), p_(p["kd"]), p_(p["kv"]), nk, p_(p["fk"]), p_(p["fd"]), nf, p_(pk), p_(pf), len(pk) - 1, p_(ik), p_(jf), C.c_float(NNRATIO), ORI,
                       p_(out), C.byref(C.c_int()))))
    say("nodes per pair (shared by both sides): %d..%d" % (min(len(p["csr"][0]) - 1 for p in pairs), max(len(p["csr"][0]) - 1 for p in pairs)))

    def run_a(n):
        t0 = time.perf_counter()
        for i in range(n):
            b1, b2, s = argsA[i % U]
            if LA.sslam_compute_bow(*b1) or LA.sslam_compute_bow(*b2) or LA.sslam_orb_search_by_bow(*s): raise RuntimeError(LA.sslam_last_error())
        return (time.perf_counter() - t0) * 1e3

    # (b)'s buffers for the unique pairs; a batch repeats them
    kkU = np.zeros((U, cap), fe.KP_DTYPE); kdU = np.zeros((U, cap, 32), np.uint8); kvU = np.zeros((U, cap), np.uint8); nkU = np.zeros(U, np.int32)
    fkU = np.zeros((U, cap), fe.KP_DTYPE); fdU = np.zeros((U, cap, 32), np.uint8); nfU = np.zeros(U, np.int32)
    for u, p in enumerate(pairs):
        nk, nf = len(p["kk"]), len(p["fk"]); nkU[u] = nk; nfU[u] = nf
        kkU[u, :nk] = p["kk"]; kdU[u, :nk] = p["kd"]; kvU[u, :nk] = p["kv"]; fkU[u, :nf] = p["fk"]; fdU[u, :nf] = p["fd"]
    up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(U, -1)).cuda()
    tU = [up(x) for x in (kkU, kdU, kvU, fkU, fdU)] + [torch.from_numpy(nkU).cuda(), torch.from_numpy(nfU).cuda()]
    st = torch.cuda.Stream()
    report = {}
    for B in a.sizes:
        assert B % U == 0
        kkB, kdB, kvB, fkB, fdB = [t.repeat(B // U, 1) for t in tU[:5]]; nkB, nfB = tU[5].repeat(B // U), tU[6].repeat(B // U)
        knB = torch.full((B, cap), -9, dtype=torch.int32, device="cuda"); fnB = torch.full((B, cap), -9, dtype=torch.int32, device="cuda")
        assigned = torch.full((B, cap), -9, dtype=torch.int32, device="cuda"); nmB = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def enqueue_b():
            ctx.bow_transform_batch_dev(voc, kdB, nkB, cap, B, knB, levelsup=LEVELSUP, stream=st.cuda_stream)
            ctx.bow_transform_batch_dev(voc, fdB, nfB, cap, B, fnB, levelsup=LEVELSUP, stream=st.cuda_stream)
            ctx.search_by_bow_batch_dev(kkB, kdB, knB, kvB, nkB, cap, B, fkB, fdB, fnB, nfB, cap, B, B, assigned, nmB, nnratio=NNRATIO, check_orientation=bool(ORI),
                                        stream=st.cuda_stream)

        run_b = lambda: bp.timed_pass(st, enqueue_b)

        nA = min(B, 1024)
        run_a(max(U, 64)); run_b()                               # warm-up: code objects, the loop's arenas and pinned mirrors
        got, gnm = assigned[B - U:].cpu().numpy(), nmB[B - U:].cpu().numpy()      # the LAST pairs of the batch; (a) left pair u's rows in outs[u]
        same = all(np.array_equal(got[u, :nfU[u]], outs[u]) and gnm[u] == int((outs[u] >= 0).sum()) for u in range(U))
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
        del kkB, kdB, kvB, fkB, fdB, knB, fnB, assigned
    voc.close(); ctx.close()
    log.finish("bow_batch_probe", report, a.out)


if __name__ == "__main__":
    main()
