"""Where k_fast_cells' cycles go: the phase clocks of a library built with -DSSLAM_FAST_CYCLES (tools/build_variant.sh fastcyc -DSSLAM_FAST_CYCLES orb.hip;
SSLAM_LIB=structure-slam-pointline_amd/lib/variants/fastcyc.so python tools/fast_cycles.py [copies]) over the bench's 64 scenes, ORB branch alone.  The clocks are
s_memtime reads around set-up + staging + zeroing, pass A, pass B, suppression and emission of every wave, summed over the launch: wave-cycles per frame, and the
share of each phase.  `copies` tiles the 64 scenes (default 4: 256 frames, enough waves to fill the device)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests")); sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
import bench, pkg

PHASES = ("set-up + staging + zeroing", "pass A", "pass B", "suppression", "emission")


def main():
    copies = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    fe = pkg.frontend()
    lib = C.CDLL(fe.LIB_PATH)
    if not hasattr(lib, "sslam_testing_orb_fast_cycles"):
        sys.exit("fast_cycles.py: %s was not built with -DSSLAM_FAST_CYCLES" % fe.LIB_PATH)
    ctx = fe.Context(0)
    cur, _ = bench.synth_frames(640, 480, 64, 0)
    d = torch.from_numpy(np.stack(cur)).cuda().repeat(copies, 1, 1).contiguous()
    n = d.shape[0]
    ex = fe.OrbExtractor(ctx, 1000, 1.2, 8, 20, 7)
    cap = 1000 + 64 * 8
    d_kp = torch.zeros(n * cap * 28, dtype=torch.uint8, device="cuda"); d_desc = torch.zeros(n * cap * 32, dtype=torch.uint8, device="cuda"); d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = (C.c_ulonglong * 8)()
    for rep in range(2):      # the first pass warms up; the clocks are reset behind it
        ex.extract_batch_dev(d, 640, 480, 640, 640 * 480, n, d_kp, d_desc, d_n, cap)
        torch.cuda.synchronize(); ctx.synchronize()
        assert lib.sslam_testing_orb_fast_cycles(out, 1 if rep == 0 else 0) == 0
    c = np.array(out[:5], np.float64) / n
    print("%s: %d frames, %.1f workgroups per frame, mean keypoints %.1f" % (os.path.basename(fe.LIB_PATH), n, out[5] / n, float(d_n.float().mean())))
    for name, v in zip(PHASES, c):
        print("  %-28s %12.0f wave-cycles per frame  %5.1f %%" % (name, v, 100 * v / c.sum()))
    print("  %-28s %12.0f" % ("total", c.sum()))
    ex.close(); ctx.close()


if __name__ == "__main__":
    main()
