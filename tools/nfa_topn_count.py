"""What the top-N form of the NFA stage (csrc/nfa_topn.h) would leave out, counted on the CPU: the oracle's candidate rectangles of the benchmark's scenes
(bench.synth_frames seeds) through the host model of the rule (tests/nfa_topn_sim.py).  Per frame: candidates validated of those emitted, refinement entries
(candidates the first evaluation does not accept) validated of all, rectangle area validated of the total, slices.  usage: nfa_topn_count.py [frames=64] [maxLines=200]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import nfa_topn_sim as sim
import bench

U = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
cur, _ = bench.synth_frames(640, 480, U, 0)
frames = [sim.oracle_frame(f) for f in cur]
res = sim.model([sim.frame_case(fr, N, 640, 480) for fr in frames], plain_only=True)
print("maxLines %d, %d scenes of 640 x 480 (bench.synth_frames, rank 0); margins %.3f / %.3f px" % (N, U, 0.125, 6.125))
print("scene  cand  valid  refine  valid   area   valid  slices  accepted  edge-margin  max|final-r0|/margin")
tot = np.zeros(6)
for i, (fr, (flags, ranked, slices, validated)) in enumerate(zip(frames, res)):
    v = flags != 2
    ref = fr["at_once"] == 0
    acc = fr["accepted"] == 1
    assert np.array_equal(sim.top_n(fr["final"], acc, N), sim.top_n(fr["final"], acc & v, N)), i
    dev = (np.abs(fr["final"] - fr["r0"]) / fr["margin"])[acc].max() if acc.any() else 0.0
    row = (len(v), v.sum(), ref.sum(), (ref & v).sum(), fr["area"].sum(), fr["area"][v].sum())
    tot += row
    print("%5d %5d %6d %7d %6d %7.0f %6.0f %7d %9d %12d %12.3f" % ((i,) + row + (slices, acc.sum(), (fr["margin"] > 1 / 640).sum(), dev)))
print("sum   %5d %6d %7d %6d %7.0f %6.0f" % tuple(tot))
print("validated: %.1f %% of the candidates, %.1f %% of the refinement entries, %.1f %% of the area" % (100 * tot[1] / tot[0], 100 * tot[3] / tot[2], 100 * tot[5] / tot[4]))
