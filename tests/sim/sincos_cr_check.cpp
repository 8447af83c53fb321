// TEST INFRASTRUCTURE (not product): csrc/sincos_cr.h on the host against sin and cos evaluated in binary128 and rounded once -- a series of its own, no table, no
// double-double: another implementation.  Arguments: `n` random doubles of [0, 10], every float angle of a stride through [0, 360) as region2rect forms theta from it
// (degrees times DEG2RAD, with and without + pi), and the neighbourhoods of the multiples of pi/2 and of j/64 and the midpoints between them.  Prints "checked N mismatches M"; tests/test_sincos_cr_cpu.py asserts M == 0.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include "../../structure-slam-pointline_amd/csrc/sincos_cr.h"

typedef __float128 Q;
static const Q QPIO2 = (Q)0x1.921fb54442d18p+0 + (Q)0x1.1a62633145c07p-54 + (Q)-0x1.f1976b7ed8fbcp-110          /* pi/2 as three doubles: exact sums in binary128 down to its last bit */;

static void ref_sincos(double x, double& sn, double& cs) {
    const int k = (int)(x * 0.63661977236758134308 + 0.5);
    const Q r = (Q)x - (Q)k * QPIO2, z = r * r;          // |r| < 0.8: the constant's error times k is below 2^-110
    Q s = 0, c = 0, ts = r, tc = 1;
    for (int i = 1; i <= 40; ++i) { s += ts; c += tc; tc = -tc * z / (Q)((2 * i - 1) * (2 * i)); ts = -ts * z / (Q)((2 * i) * (2 * i + 1)); }
    const double sd = (double)s, cd = (double)c;
    switch (k & 3) {
        case 0: sn = sd; cs = cd; break;
        case 1: sn = cd; cs = -sd; break;
        case 2: sn = -sd; cs = -cd; break;
        default: sn = -cd; cs = sd; break;
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 200000;
    long checked = 0, bad = 0;
    auto check = [&](double x) {
        if (!(x >= 0 && x <= 10)) return;
        double s0, c0, s1, c1;
        sslam::crt::sincos(x, s0, c0); ref_sincos(x, s1, c1);
        ++checked;
        if (s0 != s1 || c0 != c1) { if (++bad <= 5) printf("x %.17g: sin %.17g | %.17g  cos %.17g | %.17g\n", x, s0, s1, c0, c1); }
    };
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (long i = 0; i < n; ++i) check((double)(rnd() >> 11) * (10.0 / 9007199254740992.0));
    const double DEG2RAD = 0.017453292519943295769236907684886, PI = 3.14159265358979323846;
    for (long i = 0; i < n; ++i) {
        union { uint32_t u; float f; } v; v.u = (uint32_t)(rnd() % 0x43B40000u);          // floats in [0, 360)
        const double th = (double)v.f * DEG2RAD;
        check(th); check(th + PI);
    }
    for (int k = 0; k <= 6; ++k)
        for (int d = -2000; d <= 2000; ++d) { double x = k * 1.5707963267948966; for (int q = 0; q < (d < 0 ? -d : d); ++q) x = std::nextafter(x, d < 0 ? -1.0 : 11.0); if (d % 50 == 0 || (d > -40 && d < 40)) check(x); }
    for (int j = 0; j <= 1280; ++j)
        for (int d = -6; d <= 6; ++d) { double x = j / 128.0; for (int q = 0; q < (d < 0 ? -d : d); ++q) x = std::nextafter(x, d < 0 ? -1.0 : 11.0); check(x); }
    printf("checked %ld mismatches %ld\n", checked, bad);
    return 0;
}
