#!/usr/bin/env python3
"""Generate tests/golden/sim3_ref.npz: recorded results of the REFERENCE's own Sim3Solver functions (run where the reference tree is; the fixture is what gets committed,
never the cut source or the program).

    python tests/golden/make_sim3_ref.py [REF=/root/reference]

src/Sim3Solver.cc is cut by line range into a temporary directory -- SetRansacParameters (:114-138), iterate (:140-207), CheckInliers (:340-364), Project (:382-403),
FromCameraToImage (:405-423) as whole functions, and two statement blocks inside functions of the driver: the N11 .. N44 assignments (:251-260) and step 8 of ComputeSim3
(:319-336: mT12i and mT21i from ms12i, mR12i, mt12i) -- and compiled there, unmodified, between a stand-in class declaration and a driver (both below, this project's own
text) against oracle/ref_pin/stub_cv, with the flags of FLAGS.  The stub cv::Mat has no eye(): -Deye=zeros lets :321 and :330 compile, so the last row of mT12i / mT21i is
not the reference's; Project reads the first three rows only.  The stub's copyTo takes an lvalue: a macro behind the stub's header hands it the column and block views of
:172-173, :325-326, :334-336 as lvalues.  The driver's ComputeSim3 loads ms12i, mR12i, mt12i of tests/sim3_sim.py for that iteration (the solve is OpenCV's: decision D16) and
runs the reference's step 8 on them; its RandomInt replays the integers that make the sim's sets through the reference's own swap-with-back.  The program runs every case
of tests/sim3_cases.py but those named in LEFT_OUT, whose sets the reference's draw cannot produce, and the fixture keeps inputs and outputs: per case mRansacMaxIts and
FromCameraToImage's points; per iterate call the return's iteration, nInliers, bNoMore, vbInliers, mnIterations, mnBestInliers and the best scale, rotation and translation;
per iteration mnInliersi and mvbInliersi; and for every solved set the float M of tests/sim3_ref.py with the ten N entries the reference's lines make of it."""
import os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sim3_cases as tc      # noqa: E402
import sim3_ref as ref       # noqa: E402
import sim3_sim as sim       # noqa: E402

FUNCTIONS = ((114, 138), (140, 207), (340, 364), (382, 403), (405, 423))
N_ENTRIES = (251, 260)
STEP_8 = (319, 336)
FLAGS = ["-O2", "-std=c++11", "-ffp-contract=off", "-w", "-Deye=zeros"]
LEFT_OUT = ("count_2_drawn", "twin_set", "invalid_sets")      # fewer than three correspondences; a set that names one twice; indices out of range

HEAD = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>
#include <opencv2/core/core.hpp>
template <class T> static T& sslam_lvalue(T&& t) { return t; }
#define copyTo(x) copyTo(sslam_lvalue(x))
using namespace std;
namespace DUtils { namespace Random { int RandomInt(int lo, int hi); } }
namespace StructureSLAM {
class MapPoint;
class Sim3Solver {
public:
    void SetRansacParameters(double probability, int minInliers, int maxIterations);
    cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers);
    void ComputeSim3(cv::Mat& P1, cv::Mat& P2);
    void CheckInliers();
    void Project(const vector<cv::Mat>& vP3Dw, vector<cv::Mat>& vP2D, cv::Mat Tcw, cv::Mat K);
    void FromCameraToImage(const vector<cv::Mat>& vP3Dc, vector<cv::Mat>& vP2D, cv::Mat K);
    vector<cv::Mat> mvX3Dc1, mvX3Dc2;
    vector<MapPoint*> mvpMapPoints1;
    vector<size_t> mvnIndices1, mvnMaxError1, mvnMaxError2;
    int N, mN1;
    cv::Mat mR12i, mt12i; float ms12i; cv::Mat mT12i, mT21i;
    vector<bool> mvbInliersi; int mnInliersi;
    int mnIterations; vector<bool> mvbBestInliers; int mnBestInliers;
    cv::Mat mBestT12, mBestRotation, mBestTranslation; float mBestScale;
    vector<size_t> mvAllIndices;
    vector<cv::Mat> mvP1im1, mvP2im2;
    double mRansacProb; int mRansacMinInliers, mRansacMaxIts;
    cv::Mat mK1, mK2;
    bool pending;
    void flush();
};
"""

DRIVER_A = r"""
}
#line 1 "driver"
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float rd() { unsigned u; if (scanf("%u", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static int rdi() { int v; if (scanf("%d", &v) != 1) exit(2); return v; }
static cv::Mat rdmat(int r, int c) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r * c; ++i) m.at<float>(i / c, i % c) = rd(); return m; }
struct Iter { int randi[3]; float s; cv::Mat R, t; };
static std::deque<Iter> g_iters;
static int g_draw;
int DUtils::Random::RandomInt(int, int) { if (g_iters.empty()) exit(3); return g_iters.front().randi[g_draw++]; }
namespace StructureSLAM {
void Sim3Solver::flush() {
    if (!pending) return;
    printf("it %d", mnInliersi);
    for (int i = 0; i < N; ++i) printf(" %d", mvbInliersi[i] ? 1 : 0);
    printf("\n");
    pending = false;
}
void Sim3Solver::ComputeSim3(cv::Mat& P1, cv::Mat& P2) {
    flush();
    if (g_iters.empty() || g_draw != 3) exit(3);
    Iter it = g_iters.front(); g_iters.pop_front(); g_draw = 0;
    mR12i = it.R; mt12i = it.t; ms12i = it.s;
    pending = true;
"""

DRIVER_B = r"""
}
}
#line 100 "driver"
static void n_entries(cv::Mat& M, double* o) {
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
"""

DRIVER_C = r"""
    o[0] = N11; o[1] = N12; o[2] = N13; o[3] = N14; o[4] = N22; o[5] = N23; o[6] = N24; o[7] = N33; o[8] = N34; o[9] = N44;
}
#line 200 "driver"
static cv::Mat kmat() { cv::Mat K(3, 3, CV_32F); for (int i = 0; i < 9; ++i) K.at<float>(i / 3, i % 3) = 0; K.at<float>(0, 0) = rd(); K.at<float>(1, 1) = rd(); K.at<float>(0, 2) = rd(); K.at<float>(1, 2) = rd(); K.at<float>(2, 2) = 1; return K; }
int main() {
    int N;
    while (scanf("%d", &N) == 1) {
        StructureSLAM::Sim3Solver S;
        S.pending = false; S.mnBestInliers = 0; S.mBestScale = 0;
        S.mN1 = rdi();
        const int minInliers = rdi(), maxIterations = rdi(), ncalls = rdi(), nits = rdi(), nsolved = rdi();
        unsigned long long pb; if (scanf("%llu", &pb) != 1) return 2;
        double probability; memcpy(&probability, &pb, 8);
        S.mK1 = kmat(); S.mK2 = kmat();
        for (int i = 0; i < N; ++i) {
            S.mvnIndices1.push_back((size_t)rdi());
            S.mvX3Dc1.push_back(rdmat(3, 1)); S.mvX3Dc2.push_back(rdmat(3, 1));
            S.mvnMaxError1.push_back((size_t)rdi()); S.mvnMaxError2.push_back((size_t)rdi());
            S.mvpMapPoints1.push_back(0); S.mvAllIndices.push_back((size_t)i);
        }
        S.FromCameraToImage(S.mvX3Dc1, S.mvP1im1, S.mK1);
        S.FromCameraToImage(S.mvX3Dc2, S.mvP2im2, S.mK2);
        S.SetRansacParameters(probability, minInliers, maxIterations);
        printf("case %d", S.mRansacMaxIts);
        for (int i = 0; i < N; ++i) printf(" %u %u %u %u", bits(S.mvP1im1[i].at<float>(0)), bits(S.mvP1im1[i].at<float>(1)), bits(S.mvP2im2[i].at<float>(0)), bits(S.mvP2im2[i].at<float>(1)));
        printf("\n");
        std::vector<int> calls;
        for (int k = 0; k < ncalls; ++k) calls.push_back(rdi());
        g_iters.clear(); g_draw = 0;
        for (int k = 0; k < nits; ++k) { Iter it; for (int j = 0; j < 3; ++j) it.randi[j] = rdi(); it.s = rd(); it.R = rdmat(3, 3); it.t = rdmat(3, 1); g_iters.push_back(it); }
        for (int k = 0; k < ncalls; ++k) {
            bool bNoMore; vector<bool> vbInliers; int nInliers;
            cv::Mat T = S.iterate(calls[k], bNoMore, vbInliers, nInliers);
            S.flush();
            printf("call %d %d %d %d %d %u", T.empty() ? -1 : S.mnIterations - 1, nInliers, bNoMore ? 1 : 0, S.mnIterations, S.mnBestInliers, bits(S.mBestScale));
            for (int i = 0; i < 9; ++i) printf(" %u", S.mBestRotation.empty() ? 0u : bits(S.mBestRotation.at<float>(i / 3, i % 3)));
            for (int i = 0; i < 3; ++i) printf(" %u", S.mBestTranslation.empty() ? 0u : bits(S.mBestTranslation.at<float>(i)));
            for (size_t i = 0; i < vbInliers.size(); ++i) printf(" %d", vbInliers[i] ? 1 : 0);
            printf("\n");
        }
        if (!g_iters.empty()) return 4;
        for (int k = 0; k < nsolved; ++k) {
            cv::Mat M = rdmat(3, 3); double o[10];
            n_entries(M, o);
            printf("nent");
            for (int i = 0; i < 10; ++i) { unsigned long long u; memcpy(&u, &o[i], 8); printf(" %llu", u); }
            printf("\n");
        }
    }
    return 0;
}
"""


def randi_for(n, s):
    """the integers RandomInt has to return so that :166-177 picks the set s out of n indices"""
    avail = list(range(n)); out = []
    for idx in s:
        r = avail.index(int(idx)); out.append(r)
        avail[r] = avail[-1]; avail.pop()
    return out


def main():
    refdir = "/root/reference"
    for a in sys.argv[1:]:
        if a.startswith("REF="):
            refdir = a[4:]
    src = os.path.join(refdir, "src", "Sim3Solver.cc")
    lines = open(src, encoding="utf-8", errors="replace").read().split("\n")
    cut = lambda a, b: '#line %d "%s"\n' % (a, src) + "\n".join(lines[a - 1:b]) + "\n"
    cases = [c for c in tc.all_cases() if c["name"] not in LEFT_OUT]
    want = [w for c, w in zip(tc.all_cases(), tc.expected()) if c["name"] not in LEFT_OUT]
    with tempfile.TemporaryDirectory() as d:
        cc = os.path.join(d, "sim3_ref.cc")
        with open(cc, "w") as f:
            f.write(HEAD)
            for a, b in FUNCTIONS:
                f.write(cut(a, b))
            f.write(DRIVER_A + cut(*STEP_8) + DRIVER_B + cut(*N_ENTRIES) + DRIVER_C)
        exe = os.path.join(d, "sim3_ref")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "..", "..", "oracle", "ref_pin", "stub_cv"), cc, "-o", exe])
        text, ms = [], []
        for c, w in zip(cases, want):
            i1, i2, X1, X2, p1, p2, e1, e2 = ref.correspondences(c)
            N = len(i1)
            its = [(k, j) for k, cl in enumerate(w["calls"]) for j in range(len(cl["its"]))]
            m = []
            for k, j in its:
                s = w["calls"][k]["sets"][j]
                P1 = X1[s].T; P2 = X2[s].T
                Pr1, Pr2, _, _, _ = ref.n_entries(P1, P2)
                with np.errstate(all="ignore"):
                    m.append(ref._mul(Pr2, Pr1.T))
            ms.append(np.array(m, np.float32).reshape(len(its), 9))
            text.append("%d %d %d %d %d %d %d %d\n%s\n%s\n" % (N, len(c["m12"]), c["min_inliers"], c["max_iterations"], len(c["calls"]), len(its), len(its),
                                                           int(np.float64(c["probability"]).view(np.uint64)), sim._bits(c["kf1"]["K"]), sim._bits(c["kf2"]["K"])))
            for r in range(N):
                text.append("%d %s %s %d %d\n" % (i1[r], sim._bits(X1[r]), sim._bits(X2[r]), int(e1[r]), int(e2[r])))
            text.append(sim._ints(c["calls"]) + "\n")
            for k, j in its:
                cl = w["calls"][k]
                text.append("%s %s\n" % (sim._ints(randi_for(N, cl["sets"][j])), sim._bits(cl["mats"][j])))
            for row in ms[-1]:
                text.append(sim._bits(row) + "\n")
        out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, check=True).stdout.splitlines()
    fx = {"meta": np.array("src/Sim3Solver.cc %s (functions), :%d-%d (the N entries) and :%d-%d (step 8 of ComputeSim3) of the reference, unmodified, g++ %s against "
                           "oracle/ref_pin/stub_cv; every slice compiled as it is, none left out; inputs: tests/sim3_cases.py without %s, hypotheses: tests/sim3_sim.py "
                           "(tests/golden/make_sim3_ref.py)" % (", ".join(":%d-%d" % s for s in FUNCTIONS), N_ENTRIES[0], N_ENTRIES[1], STEP_8[0], STEP_8[1], " ".join(FLAGS),
                                                                 ", ".join(LEFT_OUT))),
          "names": np.array([c["name"] for c in cases])}
    at = 0
    for c, w, m in zip(cases, want, ms):
        n = c["name"]
        N = w["n"]
        t = out[at].split(); at += 1
        assert t[0] == "case"
        fx[n + "/max_its"] = np.int32(int(t[1]) if N >= c["min_inliers"] else -1)      # undefined below min_inliers: not recorded
        fx[n + "/img"] = sim._floats(t[2:]).reshape(N, 4)
        calls, counts, marks = [], [], []
        for cl in w["calls"]:
            for _ in cl["its"]:
                t = out[at].split(); at += 1
                assert t[0] == "it"
                counts.append(int(t[1])); marks.append([int(x) for x in t[2:]])
            t = out[at].split(); at += 1
            assert t[0] == "call"
            calls.append(dict(head=[int(x) for x in t[1:6]], best=sim._floats(t[6:19]), inl=[int(x) for x in t[19:]]))
        fx[n + "/calls"] = np.array([k["head"] for k in calls], np.int32).reshape(len(calls), 5)      # return iteration, nInliers, bNoMore, mnIterations, mnBestInliers
        fx[n + "/best"] = np.array([k["best"] for k in calls], np.float32).reshape(len(calls), 13)
        fx[n + "/inliers"] = np.array([k["inl"] for k in calls], np.uint8).reshape(len(calls), len(c["m12"]))
        fx[n + "/counts"] = np.array(counts, np.int32)
        fx[n + "/marks"] = np.array(marks, np.uint8).reshape(len(counts), N)
        fx[n + "/M"] = m
        ne = []
        for _ in range(len(m)):
            t = out[at].split(); at += 1
            assert t[0] == "nent"
            ne.append(np.array([int(x) for x in t[1:]], np.uint64).view(np.float64))
        fx[n + "/nent"] = np.array(ne, np.float64).reshape(len(m), 10)
    assert at == len(out)
    path = os.path.join(HERE, "sim3_ref.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
