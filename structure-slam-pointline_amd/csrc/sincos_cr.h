// sin and cos of a double, CORRECTLY ROUNDED, for region2rect's dx = cos(theta), dy = sin(theta) (lsd_regions.h).  The reference evaluates them with the host's libm, whose
// result is the correctly rounded one in all but about one case in 750 (glibc 2.3x, measured on random arguments of [0, 10]); the device library's cos / sin are faithful (below one ulp) and round the other way for about one
// theta in fifteen -- a last bit that no segment shows and that the NFA stage's counts depend on (tests/test_lsd_core_gpu.py compares the records bit for bit).  Two
// implementations cannot agree on every argument unless both round correctly, so that is what both sides do: the oracle in binary128 (oracle/lsd_oracle.cpp cr_sincos), the
// library here in double-double -- about 2^-100 before the final rounding, so the result is the correctly rounded one unless sin or cos lies within 2^-47 ulp of a midpoint.
// Argument range [0, 10]: theta is an angle in [0, 2 pi) plus at most pi.
//   x = k pi/2 + r (pi/2 in three parts, the products with k < 8 exact), r = j/64 + t with |t| <= 1/128 + 2^-50, sin and cos of j/64 from a table, of t by their series
//   (the two leading coefficients in double-double, the rest in double), then the addition theorems and the quadrant.
// No HIP in here: tests/sim/sincos_cr_check.cpp compiles it with a host compiler and compares it with binary128 on random and on adversarial arguments; the device runs
// the same operations (the library is built with -ffp-contract=off: an fma is one where it is written).
#pragma once
#ifdef __HIPCC__
#define SSLAM_CRT_FN __host__ __device__ __forceinline__
#else
#define SSLAM_CRT_FN inline
#endif

namespace sslam { namespace crt {

struct DD { double h, l; };
SSLAM_CRT_FN DD quick_two_sum(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }      // |a| >= |b|
SSLAM_CRT_FN DD two_sum(double a, double b) { const double s = a + b, bb = s - a; return {s, (a - (s - bb)) + (b - bb)}; }
SSLAM_CRT_FN DD two_prod(double a, double b) { const double p = a * b; return {p, __builtin_fma(a, b, -p)}; }
// (the sums below have no cancellation worth the name -- a series with falling terms, an addition theorem whose terms differ by a factor of two at least -- so the tails
// are added plainly: error about 2^-105 of the larger operand)
SSLAM_CRT_FN DD add(DD a, DD b) { DD s = two_sum(a.h, b.h); s.l += a.l + b.l; return quick_two_sum(s.h, s.l); }
SSLAM_CRT_FN DD add_ord(DD a, DD b) { DD s = quick_two_sum(a.h, b.h); s.l += a.l + b.l; return quick_two_sum(s.h, s.l); }      // |a| >= |b|: a series' coefficient and what is left of the series
SSLAM_CRT_FN DD add_big(double a, DD b) { DD s = quick_two_sum(a, b.h); s.l += b.l; return quick_two_sum(s.h, s.l); }      // |a| >= |b|
SSLAM_CRT_FN DD mul(DD a, DD b) { DD p = two_prod(a.h, b.h); p.l = __builtin_fma(a.h, b.l, __builtin_fma(a.l, b.h, p.l)); return quick_two_sum(p.h, p.l); }
// products whose consumer is a sum or another product below stay as the pair the multiplication leaves (the tail up to a few ulps of the head): those renormalise or do not care
SSLAM_CRT_FN DD mul_raw(DD a, DD b) { DD p = two_prod(a.h, b.h); p.l = __builtin_fma(a.h, b.l, __builtin_fma(a.l, b.h, p.l)); return p; }
SSLAM_CRT_FN DD mul_d_raw(DD a, double b) { DD p = two_prod(a.h, b); p.l = __builtin_fma(a.l, b, p.l); return p; }
SSLAM_CRT_FN DD neg(DD a) { return {-a.h, -a.l}; }

constexpr double PIO2_1 = 0x1.921fb54442d10p+0, PIO2_2 = 0x1.08d313198a2e0p-49, PIO2_3 = 0x1.b839a252049c1p-104;      // pi/2 in 49 + 49 + 53 bits
constexpr double TWO_OVER_PI = 0x1.45f306dc9c883p-1;
// sin(j/64), cos(j/64) as double-double, j = 0 .. 51
constexpr double TAB[52][4] = {
    {0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.fffaaaaeeeed5p-7, -0x1.2ab639a9f0776p-63, 0x1.fff000155549fp-1, 0x1.28a28a03a5ef3p-55},
    {0x1.ffeaaaeeee86fp-6, -0x1.cd406fb224ae2p-60, 0x1.ffc00155527d3p-1, -0x1.3b54492d89b5bp-55},
    {0x1.7fdc01032fba9p-5, -0x1.599bdf46e997ap-59, 0x1.ff7006bfdf99fp-1, -0x1.8b3b560648d5fp-56},
    {0x1.ffaaaeeed4edbp-5, -0x1.2d16d32684b69p-59, 0x1.ff0015549f4d3p-1, 0x1.328387b99426fp-55},
    {0x1.3facb12d1755bp-4, -0x1.921915299468bp-58, 0x1.fe7034129ef6fp-1, -0x1.cbf4337c96f97p-57},
    {0x1.7f701032550e4p-4, 0x1.afc2d1800501ap-60, 0x1.fdc06bf7e6b9bp-1, 0x1.31902b535f8dbp-55},
    {0x1.bf1b78568391dp-4, 0x1.e91841dea4cc8p-58, 0x1.fcf0c800e99b1p-1, 0x1.ea3d786d186acp-57},
    {0x1.feaaeee86ee36p-4, -0x1.afcb2bcc6f03bp-59, 0x1.fc015527d5bd3p-1, 0x1.b68f35094efb8p-55},
    {0x1.1f0d3d7afceafp-3, -0x1.6ef95099769a5p-57, 0x1.faf22263c4bd3p-1, -0x1.52ace133a2769p-58},
    {0x1.3eb312c5d66cbp-3, 0x1.47d666b66cb91p-57, 0x1.f9c340a7cc428p-1, 0x1.c5b6b063b7462p-55},
    {0x1.5e44fcfa126f3p-3, -0x1.6f443063f89b6p-57, 0x1.f874c2e1eecf6p-1, -0x1.c6514e1332b16p-55},
    {0x1.7dc102fbaf2b5p-3, 0x1.5ab50e23c97c3p-59, 0x1.f706bdf9ece1cp-1, -0x1.698c80c36dcb4p-55},
    {0x1.9d252d0cec312p-3, 0x1.9c43d80b1137dp-58, 0x1.f57948cff6797p-1, 0x1.e3a0d3e03b1d4p-57},
    {0x1.bc6f84edc6199p-3, 0x1.9c1a56a7b0cabp-57, 0x1.f3cc7c3b3d16ep-1, -0x1.21a3ad28a3494p-57},
    {0x1.db9e15fb5a5d0p-3, -0x1.32e20d6cc6fc2p-57, 0x1.f20073086649fp-1, 0x1.b940416c1984bp-56},
    {0x1.faaeed4f31577p-3, -0x1.15d88508e32b8p-57, 0x1.f01549f7deea1p-1, 0x1.d3c1e99e5cafdp-55},
    {0x1.0cd00cef36436p-2, -0x1.9fb0a0c93e2b4p-56, 0x1.ee0b1fbc0f11cp-1, -0x1.bfd2380bbc3b1p-59},
    {0x1.1c37d64c6b876p-2, 0x1.46076fe0dcff4p-56, 0x1.ebe214f76efa8p-1, -0x1.02f9f12ba543ep-55},
    {0x1.2b8ddc43eb49fp-2, 0x1.1553899f2d807p-57, 0x1.e99a4c3a7cd83p-1, -0x1.2264b1bc53ce8p-55},
    {0x1.3ad129769d3d8p-2, 0x1.03d550487839ap-63, 0x1.e733ea0193d40p-1, -0x1.6428b3546ce13p-55},
    {0x1.4a00c9b0f3d20p-2, 0x1.823ba6bb08eadp-56, 0x1.e4af14b2a449cp-1, -0x1.68ca02e8a6833p-55},
    {0x1.591bc9fa2f597p-2, 0x1.7c74bac3fe0cbp-57, 0x1.e20bf49acd6c1p-1, -0x1.660aec7ef636bp-58},
    {0x1.682138a38d7f7p-2, -0x1.d889202444aadp-56, 0x1.df4ab3ebd875ep-1, -0x1.e2d8a7e6736c4p-55},
    {0x1.7710255764214p-2, -0x1.6ead7314bb6cep-57, 0x1.dc6b7eb995912p-1, 0x1.4b364776dcd35p-58},
    {0x1.85e7a12826949p-2, 0x1.8a40e9b5face0p-56, 0x1.d96e82f71a9dcp-1, 0x1.ff61bd5d2039dp-55},
    {0x1.94a6be9f546c5p-2, -0x1.69ce13e683f58p-56, 0x1.d653f073e4040p-1, -0x1.76236434bec37p-55},
    {0x1.a34c91cc50ccap-2, -0x1.a310e3b50cecdp-58, 0x1.d31bf8d8d7c06p-1, 0x1.e60dd3089cbddp-56},
    {0x1.b1d8305321617p-2, -0x1.ae242cb99f519p-56, 0x1.cfc6cfa52ad9fp-1, 0x1.8b5b5508f2a0dp-55},
    {0x1.c048b17b140a3p-2, 0x1.19fe6757e9fa7p-57, 0x1.cc54aa2b2972ep-1, 0x1.4ee162ba83a98p-57},
    {0x1.ce9d2e3d4a51fp-2, -0x1.2fc8a12dae298p-57, 0x1.c8c5bf8ce1a84p-1, 0x1.ab3d1a1590123p-56},
    {0x1.dcd4c15329c9ap-2, 0x1.0d4c6e171fd9ap-56, 0x1.c51a48b8b175ep-1, -0x1.1bbb43b9aa880p-57},
    {0x1.eaee8744b05f0p-2, -0x1.789b43c9b027dp-58, 0x1.c1528065b7d50p-1, -0x1.892111312e828p-55},
    {0x1.f8e99e76abc97p-2, 0x1.9d950af2d00a3p-58, 0x1.bd6ea310294f5p-1, 0x1.31bbcc88c109dp-56},
    {0x1.0362939c69955p-1, -0x1.2d8cd78397b01p-55, 0x1.b96eeef58840ep-1, 0x1.45a3cc78fade0p-58},
    {0x1.0a4021e9e1001p-1, -0x1.6f643a13914f6p-55, 0x1.b553a410c104ep-1, 0x1.8ff7947027a15p-58},
    {0x1.110d0c4b69c3bp-1, 0x1.d918998809981p-55, 0x1.b11d04162a4c6p-1, 0x1.1dd561efbc0c2p-56},
    {0x1.17c8e5f2eedb0p-1, 0x1.35e57102e2488p-57, 0x1.accb526f69de5p-1, 0x1.8fb6a8dd6b6ccp-55},
    {0x1.1e7343236574cp-1, 0x1.22a3fa4f41d5ap-56, 0x1.a85ed4373e02dp-1, 0x1.9be06385ec792p-57},
    {0x1.250bb93788bbbp-1, 0x1.ea3d02457bccep-56, 0x1.a3d7d0352bdcfp-1, -0x1.68dbaeca19669p-55},
    {0x1.2b91dea88421ep-1, -0x1.fa371db216ab0p-55, 0x1.9f368ed912f85p-1, -0x1.1d200c5791606p-55},
    {0x1.32054b148bc4fp-1, 0x1.f6b42095a135bp-55, 0x1.9a7b5a36a6514p-1, 0x1.722cfcc9fa7a9p-55},
    {0x1.386597456282bp-1, -0x1.10fada93b07a8p-56, 0x1.95a67e00cb1fdp-1, -0x1.0befda21f862dp-55},
    {0x1.3eb25d36cd53ap-1, -0x1.be570e1570fc0p-58, 0x1.90b84784ddaf7p-1, -0x1.0feb10ab93b87p-56},
    {0x1.44eb381cf386bp-1, -0x1.3ed6c1e6a5505p-55, 0x1.8bb105a5dc900p-1, 0x1.863e03e9474c1p-55},
    {0x1.4b0fc46aab761p-1, 0x1.0da05738cc59cp-61, 0x1.869108d77a6c6p-1, 0x1.338ffe2bfe9ddp-56},
    {0x1.511f9fd7b351cp-1, -0x1.5c0e861c48831p-55, 0x1.8158a31916d5dp-1, -0x1.de8b90b8228dep-57},
    {0x1.571a6966d59b3p-1, 0x1.c843b4d0fb197p-58, 0x1.7c0827f09e54fp-1, -0x1.c73d6d72aee68p-57},
    {0x1.5cffc16bf8f0dp-1, 0x1.96cb370eb578ap-55, 0x1.769fec655211fp-1, -0x1.827d5cf8c68c5p-57},
    {0x1.62cf49921ac79p-1, -0x1.edd9855b6241ap-55, 0x1.712046fa77678p-1, 0x1.425b0a5029c81p-55},
    {0x1.6888a4e134b2fp-1, -0x1.6b7d37644d5e6p-55, 0x1.6b898fa9efb5dp-1, 0x1.15ac786ccf4b2p-56},
    {0x1.6e2b77c40bde1p-1, -0x1.0e729857fad53p-56, 0x1.65dc1fdeb8cbap-1, -0x1.97c1b47337c77p-58},
};
// f(u) = 1 + u (A0 + u (A1 + u (A2 + u (B0 + u (B1 + u B2))))), u = t^2 <= 2^-14: sin t = t f(u) with row 0, cos t = f(u) with row 1; A0 and A1 in double-double, the rest in
// double (the A2 term is 2^-51 of the sum, the double's own error 2^-53 of that)
constexpr double SER[2][8] = {
    {-0x1.5555555555555p-3, -0x1.5555555555555p-57, 0x1.1111111111111p-7, 0x1.1111111111111p-63, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33},
    {-0x1.0000000000000p-1, 0x0.0p+0, 0x1.5555555555555p-5, 0x1.5555555555555p-59, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29},
};

// x = k pi/2 + r: k, and r as a double-double (relative error about 2^-105)
SSLAM_CRT_FN DD reduce(double x, int& k) {
    k = (int)__builtin_fma(x, TWO_OVER_PI, 0.5);
    const double kd = (double)k;
    const double t1 = __builtin_fma(-kd, PIO2_1, x);          // exact: k PIO2_1 has 52 bits and lies within a factor of two of x
    DD r = two_sum(t1, -kd * PIO2_2);                        // exact
    r.l = __builtin_fma(-kd, PIO2_3, r.l);
    return quick_two_sum(r.h, r.l);
}

// sin(r) and cos(r) to double-double, |r| <= pi/4 + 2^-40.  The two series are independent of each other: side by side they fill each other's latencies
SSLAM_CRT_FN void kernel(DD r, DD& sn, DD& cs) {
    const double jd = __builtin_rint(r.h * 64.0);
    const int j = (int)__builtin_fabs(jd);
    const bool negr = jd < 0;
    DD t = quick_two_sum(r.h - jd * 0.015625, r.l);          // the difference is exact
    if (negr) t = neg(t);                                    // sin(-r) = -sin(r), cos(-r) = cos(r): work on |r| = j/64 + t
    const DD u = mul(t, t);
    DD f[2];
    for (int w = 0; w < 2; ++w) {
        const double* S = SER[w];
        const double tail = __builtin_fma(u.h, __builtin_fma(u.h, __builtin_fma(u.h, S[7], S[6]), S[5]), S[4]);
        DD g = add_ord(DD{S[2], S[3]}, mul_d_raw(u, tail));      // u <= 2^-14: every coefficient is far above the rest of its series
        g = add_ord(DD{S[0], S[1]}, mul_raw(u, g));
        f[w] = add_big(1.0, mul_raw(u, g));
    }
    const DD st = mul(t, f[0]), ct = f[1];
    const DD sa = {TAB[j][0], TAB[j][1]}, ca = {TAB[j][2], TAB[j][3]};
    // sa ct >= 2 |ca st| (j >= 1: sa >= 1/64.01, |st| <= 1/127; j = 0: sa = 0 and the sum is its second term, exactly) and ca ct >= 0.69 against |sa st| <= 0.006: ordered sums
    const DD s = add_ord(mul_raw(sa, ct), mul_raw(ca, st));
    sn = negr ? neg(s) : s;
    cs = add_ord(mul_raw(ca, ct), neg(mul_raw(sa, st)));
}

// both, correctly rounded, for x in [0, 10]
SSLAM_CRT_FN void sincos(double x, double& sn, double& cs) {
    int k;
    const DD r = reduce(x, k);
    DD sd, cd;
    kernel(r, sd, cd);
    const double s = sd.h, c = cd.h;
    const bool swap = k & 1;
    // quadrant k: (s, c), (c, -s), (-s, -c), (-c, s)
    const double a = swap ? c : s, b = swap ? s : c;
    sn = (k & 2) ? -a : a;
    cs = ((k + 1) & 2) ? -b : b;
}

}}  // namespace sslam::crt
