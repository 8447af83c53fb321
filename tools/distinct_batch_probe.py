"""Times MapPoint / MapLine::ComputeDistinctiveDescriptors for a batch of sessions whose keyframes are on the device -- ONE
sslam_distinctive_descriptors_batch_dev call that also writes the map points' descriptor table (b) -- against the only route a caller had before it (a):
copy the pool's descriptors to the host, gather every observation's row there, one sslam_distinctive_descriptors call on the gathered rows, look the chosen
rows up and upload them as the table.  Same pool, same sets, same run.

    python tools/distinct_batch_probe.py [--sessions 1,64,1024] [--reps 10] [--unique 2] [--loop-lib PATH] [--out profiles/distinct_batch_probe.txt]

A session is what LocalMapping leaves behind for one new keyframe: 2 000 map points with 3 .. 14 observations each (the mix of tools/bench_matchers.py) in
21 keyframe slots of 1 000 features; an observation is a noisy copy of its point's descriptor and a keyframe sees a point once
(tests/distinct_batch_cases.py: workload).  Session s of a batch is unique session s % unique.
(b): device time between two HIP events around the call on a side stream, and wall time from the call to the end of a stream synchronise.  (a): wall time
from the first byte copied down to the table's upload being complete.  After a warm-up pass of each, `reps` alternating passes; medians.
Then the kernels alone, through sslam_profile_enable / sslam_profile_drain, `reps` passes each: k_distinctive of (a) on its gathered rows against
k_distinct_batch + k_distinct_large of (b) on the same sets.  THE CONDITION (64 sessions): the new kernels' median is not above k_distinctive's median by
more than the spread (max - min) of k_distinctive's own passes.
--loop-lib: the library (a) runs on, e.g. a build of the parent commit (default: the library under test).  d_best and the table of (b) must equal (a)'s
for every set, or the probe exits non-zero."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import pkg
import distinct_batch_cases as dc
import batch_probe_common as bp
from batch_probe_common import med

POINTS, K, N = 2000, 21, 1000


def main():
    a = bp.parse_args("--sessions", "1,64,1024", 10, 2)
    log = bp.Lines(); say = log.say

    fe = pkg.frontend()
    ctx = fe.Context(0)
    p_ = fe._p
    U = a.unique
    rng = np.random.default_rng(77)
    S = [dc.workload(rng, POINTS, K, N) for _ in range(U)]
    say("session: %d map points with 3..14 observations (%.1f on average) in %d keyframe slots of %d features; %d unique sessions"
        % (POINTS, np.mean([len(s[1]) for s in S]) / POINTS, K, N, U))
    LA, hA = bp.loop_library(fe, ctx, a, say)
    dU = torch.from_numpy(np.stack([s[0] for s in S]).reshape(U, -1)).cuda()
    st = torch.cuda.Stream()
    report = {}
    all_equal, condition = True, None
    for B in a.sizes:
        dB = dU.repeat(-(-B // U), 1)[:B].contiguous().view(B * K, N, 32)
        obs = np.concatenate([S[s % U][1] for s in range(B)])
        obs["kf"] += np.repeat(np.arange(B) * K, [len(S[s % U][1]) for s in range(B)]).astype(np.int32)
        sizes = np.concatenate([np.diff(S[s % U][2]) for s in range(B)])
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        ns, nobs = len(sizes), len(obs)
        flat = obs["kf"].astype(np.int64) * N + obs["row"]
        up = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda()
        d_obs, d_ptr = up(obs), up(ptr)
        d_n = torch.full((B * K,), N, dtype=torch.int32, device="cuda")
        best_b = torch.full((ns,), -9, dtype=torch.int32, device="cuda"); med_b = torch.full((ns,), -9, dtype=torch.int32, device="cuda")
        table_b = torch.zeros((ns, 32), dtype=torch.uint8, device="cuda"); table_a = torch.zeros((ns, 32), dtype=torch.uint8, device="cuda")
        best_a = np.full(ns, -9, np.int32)
        torch.cuda.synchronize()
        kept = {}

        def run_a():
            t0 = time.perf_counter()
            host = dB.cpu().numpy().reshape(-1, 32)                          # the pool's descriptors, down
            rows = host[flat]                                               # every observation's row, gathered on the host
            if LA.sslam_distinctive_descriptors(hA, p_(rows), p_(ptr), ns, p_(best_a)): raise RuntimeError(LA.sslam_last_error())
            chosen = rows[ptr[:-1] + best_a]
            table_a.copy_(torch.from_numpy(chosen)); torch.cuda.synchronize()     # the chosen rows, up again
            kept["rows"] = rows
            return (time.perf_counter() - t0) * 1e3

        def enqueue_b():
            ctx.distinctive_descriptors_batch_dev(dB, d_n, N, B * K, d_obs, nobs, d_ptr, ns, best_b, d_median=med_b, d_out_desc=table_b, nout=ns, stream=st.cuda_stream)

        run_b = lambda: bp.timed_pass(st, enqueue_b)[:2]

        run_a(); run_b()                                                    # warm-up; both leave their results behind
        same = bool(np.array_equal(best_b.cpu().numpy(), best_a) and torch.equal(table_a, table_b))
        all_equal = all_equal and same
        ta, tb = bp.alternate(a.reps, run_a, run_b)
        # the kernels alone: k_distinctive on (a)'s gathered rows, the two new kernels on the same sets
        rows = kept["rows"]
        ka, kb, kb_split = [], [], []
        LA.sslam_profile_enable(hA, 1)
        for _ in range(a.reps + 1):
            if LA.sslam_distinctive_descriptors(hA, p_(rows), p_(ptr), ns, p_(best_a)): raise RuntimeError(LA.sslam_last_error())
            ka.append(bp.drain(LA, hA)["k_distinctive"])
        LA.sslam_profile_enable(hA, 0)
        fe.lib().sslam_profile_enable(ctx.h, 1)
        for _ in range(a.reps + 1):
            enqueue_b(); st.synchronize()
            d = bp.drain(fe.lib(), ctx.h)
            kb.append(d["k_distinct_batch"] + d["k_distinct_large"]); kb_split.append((d["k_distinct_batch"], d["k_distinct_large"]))
        fe.lib().sslam_profile_enable(ctx.h, 0)
        ka, kb, kb_split = ka[1:], kb[1:], kb_split[1:]                       # the first pass of each is the warm-up
        spread = max(ka) - min(ka)
        meets = med(kb) <= med(ka) + spread
        if B == 64: condition = bool(meets)
        rr = dict(sessions=B, sets=ns, observations=nobs, equal=same, a_wall_ms=med(ta), a_all_ms=ta, b_device_ms=med([x[0] for x in tb]), b_wall_ms=med([x[1] for x in tb]),
                  b_all_ms=tb, k_distinctive_ms=med(ka), k_distinctive_all_ms=ka, k_distinctive_spread_ms=spread, new_kernels_ms=med(kb), new_kernels_all_ms=kb,
                  k_distinct_batch_ms=med([x[0] for x in kb_split]), k_distinct_large_ms=med([x[1] for x in kb_split]), new_not_above_old_plus_spread=bool(meets))
        report["S%d" % B] = rr
        say("sessions %5d sets %8d observations %9d | (a) copy down, gather, single call, upload: %10.3f ms wall | (b) batch: %8.3f ms device, %8.3f ms wall | (a) / (b) wall = %7.1f x | "
            "kernels alone: k_distinctive %8.3f ms (min %.3f max %.3f) against k_distinct_batch %8.3f + k_distinct_large %6.3f = %8.3f ms (min %.3f max %.3f): %s | equal %s"
            % (B, ns, nobs, rr["a_wall_ms"], rr["b_device_ms"], rr["b_wall_ms"], rr["a_wall_ms"] / rr["b_wall_ms"], rr["k_distinctive_ms"], min(ka), max(ka),
               rr["k_distinct_batch_ms"], rr["k_distinct_large_ms"], rr["new_kernels_ms"], min(kb), max(kb), "not above" if meets else "ABOVE", same))
        del dB, d_obs, d_ptr, d_n, best_b, med_b, table_a, table_b, rows, kept
    say("condition (64 sessions: new kernels' median <= k_distinctive's median + its spread): %s" % condition)
    ctx.close()
    log.finish("distinct_batch_probe", report, a.out, all_equal)


if __name__ == "__main__":
    main()
