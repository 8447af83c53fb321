"""Host-side rules of the library that need no GPU: the one CSR validator and the alignment and size rules of the device-resident
batches (csrc/match_check.h check_csr, all_aligned, rows_in_range, fits_31_bits), the parameter rules of the RANSAC entry points (sim3_params_ok,
injected_sets_ok), the bookkeeping of the buffers that
kernels use on a caller's stream after the call has returned (csrc/common.h StreamOrderedBuf), and the multi-GPU payload exchange
(csrc/group_exchange.h gather_to_root) over the RCCL stand-in with a thread per rank.  tests/sim/host_checks.cpp is a stand-alone program: plain g++ with -fsanitize=address,undefined, the HIP runtime replaced by tests/sim/hip_stub; nothing is loaded into Python."""
import os, subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_checks_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-DSSLAM_TESTING",
                           "-I" + os.path.join(HERE, "sim", "hip_stub"), os.path.join(HERE, "sim", "host_checks.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)
    assert r.stdout.splitlines() == ["check_csr ok", "argument rules ok", "ransac rules ok", "StreamOrderedBuf ok", "exchange ok", "ok"]
