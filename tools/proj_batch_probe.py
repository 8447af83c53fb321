"""Times the projection-window matcher of a batch of device-resident frames, sslam_search_by_projection_batch_dev (b), against what a caller had
before it: a loop of one sslam_search_by_projection_frame call per frame on uploaded frame handles (a).  Same frames, same queries, same run.

    python tools/proj_batch_probe.py [--batches 1024,6144] [--reps 5] [--unique 16] [--out profiles/proj_batch_probe.txt]

Inputs: kind 0 (keypoints); mode 1 with the rotation check and mode 0.  `unique` synthetic 640x480 frames of 1000 ORB keypoints each (the CPU oracle's
extraction), one query per keypoint built from the frame's own keypoints with jitter as tests/test_match_gpu.py::_proj_queries does, query descriptors
= the keypoints' with up to 11 bits flipped, 5 % of the keypoints occupied; frame f of a batch is unique frame f % unique.
Per batch size and mode, after one untimed pass of each: `reps` alternating passes of (a) and (b), medians.  (a): wall time of the loop (every call
synchronises).  (b): device time between two HIP events on the call's stream, and wall time from the call to the end of a stream synchronise.
Then, untimed passes with sslam_profile_enable: the kernel split of (b), and the sum of (a)'s kernels.  Last, (b) with the commit layout the plan
did not choose (the single call's features in LDS, through sslam_testing_proj_batch_tuning) -- which is why the probe runs on
libsslam_frontend_testing.so, the product's sources plus the hooks of include/sslam_testing.h."""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg, oracle_lib
from synth import synth_frame
from test_match_gpu import _proj_queries
from match_cases import flip_bits
import batch_probe_common as bp
from batch_probe_common import med

PARAMS = {0: (0.8, 100, 0), 1: (0.9, 100, 1)}          # mode -> nnratio, th_dist, check_orientation


def main():
    a = bp.parse_args("--batches", "1024,6144", 5, 16, loop_lib=False)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend(); orc = oracle_lib.Oracle()
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    scales = orc.orb_params()[0].astype(np.float32)
    U = a.unique
    rng = np.random.default_rng(7)
    frames = []
    for u in range(U):
        kp, d = orc.orb_extract(synth_frame(3000 + u), 1000)
        frames.append((kp, d, (rng.random(len(kp)) < 0.05).astype(np.uint8)))
    cap = max(len(f[0]) for f in frames); qcap = cap
    say("frames: %d unique, keypoints %d..%d, cap = qcap = %d" % (U, min(len(f[0]) for f in frames), cap, cap))
    with fe.use_testing_library() as L:
        ctx = fe.Context(0)
        st = torch.cuda.Stream()
        handles = [ctx.frame_upload(0, kp, d) for kp, d, _ in frames]
        report = {}
        for mode in (1, 0):
            ratio, th, ori = PARAMS[mode]
            qs = [np.ascontiguousarray(_proj_queries(fe, rng, kp, 0, mode, scales)) for kp, _, _ in frames]
            qds = [flip_bits(rng, d, 12) for _, d, _ in frames]
            # (b)'s buffers for the unique frames; a batch repeats them
            kpU = np.zeros((U, cap), fe.KP_DTYPE); dU = np.zeros((U, cap, 32), np.uint8); occU = np.zeros((U, cap), np.uint8)
            qU = np.zeros((U, qcap), fe.PQ_DTYPE); qdU = np.zeros((U, qcap, 32), np.uint8); nU = np.zeros(U, np.int32)
            for u, (kp, d, occ) in enumerate(frames):
                n = len(kp); nU[u] = n
                kpU[u, :n] = kp; dU[u, :n] = d; occU[u, :n] = occ; qU[u, :n] = qs[u]; qdU[u, :n] = qds[u]
            up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(U, -1)).cuda()
            tU = [up(x) for x in (kpU, dU, occU, qU, qdU)] + [torch.from_numpy(nU).cuda()]
            # (a)'s arguments, ready for ctypes (no Python work inside the timed loop beyond the call)
            outs = [np.full(len(f[0]), -1, np.int32) for f in frames]; nm = C.c_int(0)
            argsA = [(ctx.h, handles[u].h, mode, fe._p(frames[u][2]), fe._p(qs[u]), fe._p(qds[u]), len(qs[u]), C.c_float(ratio), th, ori, fe._p(outs[u]), C.byref(nm))
                     for u in range(U)]
            fnA = L.sslam_search_by_projection_frame

            def run_a(B):
                t0 = time.perf_counter()
                for f in range(B):
                    rc = fnA(*argsA[f % U])
                    if rc: raise RuntimeError(L.sslam_last_error())
                return (time.perf_counter() - t0) * 1e3

            for B in a.sizes:
                assert B % U == 0
                kpB, dB, occB, qB, qdB = [t.repeat(B // U, 1) for t in tU[:5]]; nB = tU[5].repeat(B // U)
                assigned = torch.full((B, cap), -9, dtype=torch.int32, device="cuda"); nmB = torch.zeros(B, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()

                def enqueue_b():
                    ctx.search_by_projection_batch_dev(0, mode, kpB, dB, nB, cap, B, qB, qdB, nB, qcap, assigned, nmB, d_occupied=occB, nnratio=ratio, th_dist=th,
                                                       check_orientation=ori, stream=st.cuda_stream)

                run_b = lambda: bp.timed_pass(st, enqueue_b)

                run_a(B); run_b()                                   # warm-up: code objects, the arena, the pinned mirrors
                got = assigned[:U].cpu().numpy()
                same = all(np.array_equal(got[u, :nU[u]], outs[u]) for u in range(U)) and bool((nmB.cpu().numpy() >= 0).all())      # (a) left frame u's rows in outs[u]
                ta, tb = bp.alternate(a.reps, lambda: run_a(B), run_b)
                dev_b, wall_b, enq_b = bp.b_medians(tb)
                wall_a = med(ta)
                # kernel split, untimed passes
                L.sslam_profile_enable(ctx.h, 1)
                run_b(); split_b = pipeline.profile_drain(fe, ctx)
                run_a(B); split_a = pipeline.profile_drain(fe, ctx)
                L.sslam_profile_enable(ctx.h, 0)
                # the other commit layout
                assert L.sslam_testing_proj_batch_tuning(0, 1) == 0
                run_b(); tl = [run_b() for _ in range(a.reps)]
                L.sslam_profile_enable(ctx.h, 1); run_b(); split_l = pipeline.profile_drain(fe, ctx); L.sslam_profile_enable(ctx.h, 0)
                assert L.sslam_testing_proj_batch_tuning(0, 0) == 0
                same_l = all(np.array_equal(assigned[u].cpu().numpy()[:nU[u]], outs[u]) for u in range(U))
                r = dict(mode=mode, B=B, equal_to_single_calls=same, a_wall_ms=wall_a, a_us_per_frame=wall_a * 1e3 / B, a_all_ms=ta,
                         a_kernels_us_per_frame=sum(v[0] for v in split_a.values()) * 1e3 / B,
                         b_device_ms=dev_b, b_wall_ms=wall_b, b_enqueue_ms=enq_b, b_us_per_frame_device=dev_b * 1e3 / B, b_us_per_frame_wall=wall_b * 1e3 / B,
                         b_all_ms=[x[:2] for x in tb], b_kernels_ms={k: v[0] for k, v in split_b.items()}, b_launches={k: v[1] for k, v in split_b.items()},
                         lds64_device_ms=med([x[0] for x in tl]), lds64_kernels_ms={k: v[0] for k, v in split_l.items()}, lds64_equal=same_l)
                report["mode%d_B%d" % (mode, B)] = r
                say("mode %d  B %5d  (a) loop of single calls: %8.2f ms wall = %7.2f us/frame (kernels %.2f us/frame) | (b) batch: %8.2f ms device, %8.2f ms wall = %6.2f / %6.2f us/frame"
                    "  [enqueue %.2f ms] | equal %s" % (mode, B, wall_a, r["a_us_per_frame"], r["a_kernels_us_per_frame"], dev_b, wall_b, r["b_us_per_frame_device"],
                                                       r["b_us_per_frame_wall"], enq_b, same))
                say("        (b) kernels: " + ", ".join("%s %.2f ms x%d" % (k, v[0], v[1]) for k, v in sorted(split_b.items())))
                say("        commit layout: 8 B/feature (kept) %.2f ms device, kernels %s | 64 B/feature (features in LDS) %.2f ms device, kernels %s, equal %s"
                    % (dev_b, {k: round(v, 2) for k, v in r["b_kernels_ms"].items()}, r["lds64_device_ms"], {k: round(v, 2) for k, v in r["lds64_kernels_ms"].items()}, same_l))
                del kpB, dB, occB, qB, qdB, assigned
        for h in handles: h.close()
        ctx.close()
    log.finish("proj_batch_probe", report, a.out)


if __name__ == "__main__":
    main()
