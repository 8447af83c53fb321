#!/usr/bin/env python3
"""Generate tests/golden/two_view_ref.npz: recorded results of the REFERENCE's own Normalize, CheckHomography and CheckFundamental (run where the reference tree is; the
fixture is what gets committed, never the cut source or the program).

    python tests/golden/make_two_view_ref.py [REF=/root/reference]

src/Initializer.cc:334-497 and :784-830 are cut by line range into a temporary directory and compiled there, unmodified, between a stand-in class declaration and a driver
(both below, this project's own text) against oracle/ref_pin/stub_cv, with the flags of FLAGS.  The stub cv::Mat has no eye(): -Deye=zeros lets :825 compile, so the elements
of T that Normalize does not assign (the zeros and T(2, 2)) are not the reference's and are not recorded -- T(0, 0), T(1, 1), T(0, 2), T(1, 2) are.  The program runs every
case of tests/two_view_cases.py with the matrices tests/two_view_sim.py computes for every iteration (the solves and compositions are OpenCV's: decision D15), and the fixture
keeps inputs and outputs: per case the keypoints, matches, sigma and the matrices H21i, H12i, F21i that went in; vNormalizedPoints and the four T elements of both frames,
and per iteration both scores and both vbMatchesInliers that came out."""
import os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import two_view_cases as tc      # noqa: E402
import two_view_sim as sim       # noqa: E402

SLICES = ((334, 497), (784, 830))
FLAGS = ["-O2", "-std=c++11", "-ffp-contract=off", "-w", "-Deye=zeros"]

HEAD = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
using namespace std;
namespace StructureSLAM {
class Initializer {
public:
    typedef pair<int, int> Match;
    float CheckHomography(const cv::Mat& H21, const cv::Mat& H12, vector<bool>& vbMatchesInliers, float sigma);
    float CheckFundamental(const cv::Mat& F21, vector<bool>& vbMatchesInliers, float sigma);
    void Normalize(const vector<cv::KeyPoint>& vKeys, vector<cv::Point2f>& vNormalizedPoints, cv::Mat& T);
    vector<cv::KeyPoint> mvKeys1, mvKeys2;
    vector<Match> mvMatches12;
};
"""

DRIVER = r"""
}
#line 1 "driver"
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float rd() { unsigned u; if (scanf("%u", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static cv::Mat rdmat() { cv::Mat m(3, 3, CV_32F); for (int i = 0; i < 9; ++i) m.at<float>(i / 3, i % 3) = rd(); return m; }
int main() {
    int n1, n2, its;
    while (scanf("%d %d %d", &n1, &n2, &its) == 3) {
        StructureSLAM::Initializer I;
        const float sigma = rd();
        for (int i = 0; i < n1; ++i) { float x = rd(), y = rd(); I.mvKeys1.push_back(cv::KeyPoint(cv::Point2f(x, y), 31.f)); }
        for (int i = 0; i < n2; ++i) { float x = rd(), y = rd(); I.mvKeys2.push_back(cv::KeyPoint(cv::Point2f(x, y), 31.f)); }
        for (int i = 0; i < n1; ++i) { int m; if (scanf("%d", &m) != 1) return 2; if (m >= 0) I.mvMatches12.push_back(make_pair(i, m)); }      // src/Initializer.cc:67-76
        for (int f = 0; f < 2; ++f) {
            vector<cv::Point2f> pn; cv::Mat T;
            I.Normalize(f ? I.mvKeys2 : I.mvKeys1, pn, T);
            printf("norm");
            for (size_t i = 0; i < pn.size(); ++i) printf(" %u %u", bits(pn[i].x), bits(pn[i].y));
            printf(" %u %u %u %u\n", bits(T.at<float>(0, 0)), bits(T.at<float>(1, 1)), bits(T.at<float>(0, 2)), bits(T.at<float>(1, 2)));
        }
        for (int it = 0; it < its; ++it) {
            cv::Mat H21 = rdmat(), H12 = rdmat(), F21 = rdmat();
            vector<bool> ih, jf;
            const float sh = I.CheckHomography(H21, H12, ih, sigma), sf = I.CheckFundamental(F21, jf, sigma);
            printf("chk %u %u", bits(sh), bits(sf));
            for (size_t i = 0; i < ih.size(); ++i) printf(" %d", (ih[i] ? 1 : 0) | (jf[i] ? 2 : 0));
            printf("\n");
        }
    }
    return 0;
}
"""


def main():
    ref = "/root/reference"
    for a in sys.argv[1:]:
        if a.startswith("REF="):
            ref = a[4:]
    src = os.path.join(ref, "src", "Initializer.cc")
    lines = open(src, encoding="utf-8", errors="replace").read().split("\n")
    cases = tc.all_cases()
    want = sim.run(cases)
    with tempfile.TemporaryDirectory() as d:
        cc = os.path.join(d, "two_view_ref.cc")
        with open(cc, "w") as f:
            f.write(HEAD)
            for a, b in SLICES:
                f.write('#line %d "%s"\n' % (a, src) + "\n".join(lines[a - 1:b]) + "\n")
            f.write(DRIVER)
        exe = os.path.join(d, "two_view_ref")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "..", "..", "oracle", "ref_pin", "stub_cv"), cc, "-o", exe])
        text = []
        for c, w in zip(cases, want):
            assert (c["m12"] < len(c["kp2"])).all()          # the reference takes every non-negative entry: the cases hold none past frame 2
            text.append("%d %d %d %s\n%s\n%s\n%s\n" % (len(c["kp1"]), len(c["kp2"]), c["iterations"], sim._bits(np.float32(c["sigma"])), sim._bits(c["kp1"]), sim._bits(c["kp2"]),
                                                      sim._ints(c["m12"])))
            for it in range(c["iterations"]):
                text.append(sim._bits(w["mats"][it, [1, 2, 4]]) + "\n")
        out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, check=True).stdout.splitlines()
    fx = {"meta": np.array("src/Initializer.cc:%s of the reference, unmodified, g++ %s against oracle/ref_pin/stub_cv; inputs: tests/two_view_cases.py, matrices: "
                           "tests/two_view_sim.py (tests/golden/make_two_view_ref.py)" % (", ".join(":%d-%d" % s for s in SLICES), " ".join(FLAGS))),
          "names": np.array([c["name"] for c in cases])}
    at = 0
    for c, w in zip(cases, want):
        n = c["name"]
        fx[n + "/kp1"], fx[n + "/kp2"], fx[n + "/m12"], fx[n + "/sigma"] = c["kp1"], c["kp2"], c["m12"], np.float32(c["sigma"])
        fx[n + "/mats"] = w["mats"][:, [1, 2, 4]]
        for f, k in ((1, len(c["kp1"])), (2, len(c["kp2"]))):
            t = sim._floats(out[at].split()[1:]); at += 1
            fx[n + "/pn%d" % f], fx[n + "/T%d" % f] = t[:2 * k].reshape(k, 2), t[2 * k:]
            assert len(t) == 2 * k + 4
        sc, inl = [], []
        for it in range(c["iterations"]):
            t = out[at].split(); at += 1
            assert t[0] == "chk"
            sc.append(sim._floats(t[1:3])); inl.append(np.array([int(x) for x in t[3:]], np.uint8))
        fx[n + "/scores"], fx[n + "/inliers"] = np.array(sc, np.float32).reshape(-1, 2), np.array(inl, np.uint8).reshape(c["iterations"], -1)
    assert at == len(out)
    path = os.path.join(HERE, "two_view_ref.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
