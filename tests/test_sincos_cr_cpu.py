"""csrc/sincos_cr.h on the host: the double-double sin / cos that region2rect's dx and dy come from against a binary128 evaluation of its own
(tests/sim/sincos_cr_check.cpp: series, no table, no double-double), and the oracle's cr_sincos (oracle/lsd_oracle.cpp, binary128 as well, written separately) against
both.  Correctly rounded means equal: no tolerance."""
import ctypes as C
import math
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_double_double_sincos_is_correctly_rounded(tmp_path):
    """1.36 million arguments: random doubles of [0, 10], float angles in degrees turned into theta as region2rect does (with and without + pi), the neighbourhoods of the
    multiples of pi/2 (the reduction's cancellation) and of the table's points and the midpoints between them (the largest |t|)"""
    exe = str(tmp_path / "sincos_cr_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "sim", "sincos_cr_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe, "450000"], text=True).strip().split("\n")
    print("\n".join(out))
    w = out[-1].split()
    assert w[0] == "checked" and int(w[1]) > 1350000 and w[2] == "mismatches" and int(w[3]) == 0, out


def test_oracle_sincos_is_correctly_rounded_too(oracle):
    """the oracle's function against libm: they differ rarely and by one ulp only (libm is not specified to round correctly; glibc does for all but about one argument in
    750), and on an argument where the two differ the oracle's value is the one nearer to a 60-digit evaluation"""
    f = oracle.L.orc_cr_sincos
    f.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]; f.restype = None
    s, c = C.c_double(), C.c_double()
    rng = np.random.Generator(np.random.PCG64(18))
    xs = rng.uniform(0, 10, 20000); diff = 0
    for x in xs.tolist():
        f(x, C.byref(s), C.byref(c))
        for got, ref in ((s.value, math.sin(x)), (c.value, math.cos(x))):
            if got != ref:
                diff += 1
                assert got in (math.nextafter(ref, -2.0), math.nextafter(ref, 2.0)), (x, got, ref)
    assert diff <= 200, diff          # (about 50 expected of 40 000)
    # theta of a candidate of lsd_cases' spiral8 on which the device library's cos was one ulp off: cos = -0.661137970656348109849699..., 0.467 ulp from the value below
    f(8.576316142758856, C.byref(s), C.byref(c))
    assert c.value == -0.6611379706563482
