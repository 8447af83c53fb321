#!/usr/bin/env python3
"""Generate tests/golden/reconstruct_ref.npz: recorded results of the REFERENCE's own ReconstructF, ReconstructH, CheckRT, DecomposeE, Triangulate, LineTriangulate,
ReconstructLine and vector_mad (run where the reference tree is; the fixture is what gets committed, never the cut source or the program).

    python tests/golden/make_reconstruct_ref.py [REF=/root/reference]

src/Initializer.cc:499-782 and :833-1171 and include/auxiliar.h:91-106 are cut by line range into a temporary directory and compiled there, unmodified, between a stand-in
class declaration and a driver (both below, this project's own text), with the flags of FLAGS.  oracle/ref_pin/stub_cv has no inv, eye, determinant, SVD or Eigen and its
`A.row(0) = expression` rebinds a header instead of writing the row, so the stand-ins are carried here: a small cv::Mat with OpenCV's reference semantics (views write
through), whose arithmetic is decision D18's conventions (products accumulated in double and rounded once, s * A and A / s through a double alpha, norm and dot in
double), and Vector3d / Vector2d.  D18's leaves are handed back to the cut code from csrc/reconstruct_math.h: cv::SVD::compute (svd3 for a 3 x 3; for a 4 x 4 svd4_last
fills vt.row(3), the only row the reference reads), cv::determinant, Mat::inv, and acos, which the cut code finds as StructureSLAM::acos.  Three names are redirected with
the preprocessor so that what the reference keeps in locals can be recorded without touching its text: inside :499-782 CheckRT is LoggedCheckRT (which records R, t, nGood,
parallax, vP3D and vbGood of every hypothesis and calls the reference's CheckRT), inside :833-1171 vector_mad is logged_mad (which records errorC1 / errorC2 and calls the
reference's vector_mad), and cout is a sink.  The driver applies the entry point's filter of line pairs ([0, nl), csrc/reconstruct.hip) before the reference's >= 0 filter.
The program runs every case of tests/reconstruct_cases.py; the fixture keeps inputs and outputs."""
import os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reconstruct_cases as rcases      # noqa: E402
import reconstruct_sim as sim           # noqa: E402

SLICES = ((499, 782), (833, 1171))
MAD = (91, 106)
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-w"]
INPUTS = ("kp1", "kp2", "m12", "inliers", "H21", "F21", "K")

HEAD = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <utility>
#include <vector>
#include "reconstruct_math.h"
using namespace std;
#define CV_32F 5
#define CV_PI 3.1415926535897932384626433832795
namespace cv {
struct Scalar { double v; Scalar(double x = 0) : v(x) {} };
struct Point2f { float x, y; Point2f(float a = 0, float b = 0) : x(a), y(b) {} };
struct Point3f { float x, y, z; Point3f(float a = 0, float b = 0, float c = 0) : x(a), y(b), z(c) {} };
struct KeyPoint { Point2f pt; };
class Mat {      // CV_32F only; a header over shared storage, views write through
public:
    shared_ptr<vector<float>> d; int off = 0, ld = 0, rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int) { create(r, c); }
    Mat(int r, int c, int, const Scalar& s) { create(r, c); for (float& f : *d) f = (float)s.v; }
    void create(int r, int c) { d = make_shared<vector<float>>((size_t)r * c, 0.f); off = 0; ld = c; rows = r; cols = c; }
    bool empty() const { return !d || rows == 0 || cols == 0; }
    float& e(int r, int c) const { return (*d)[(size_t)off + (size_t)r * ld + c]; }
    template <class T> T& at(int r, int c) const { return e(r, c); }
    template <class T> T& at(int i) const { return rows == 1 ? e(0, i) : e(i, 0); }
    static Mat eye(int r, int c, int) { Mat m(r, c, CV_32F); for (int i = 0; i < r && i < c; ++i) m.e(i, i) = 1.f; return m; }
    static Mat zeros(int r, int c, int) { return Mat(r, c, CV_32F); }
    struct View;
    View rowRange(int a, int b) const;
    View colRange(int a, int b) const;
    View row(int y) const;
    View col(int x) const;
    Mat clone() const { Mat m(rows, cols, CV_32F); for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) m.e(i, j) = e(i, j); return m; }
    void copyTo(Mat& m) const { if (empty()) { m = Mat(); return; } if (m.rows != rows || m.cols != cols || !m.d) m.create(rows, cols); write(m); }
    void copyTo(Mat&& m) const { write(m); }      // into a view
    void write(const Mat& m) const { Mat s = clone(); for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) m.e(i, j) = s.e(i, j); }
    Mat t() const { Mat m(cols, rows, CV_32F); for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) m.e(j, i) = e(i, j); return m; }
    Mat inv() const { float a[9], o[9]; get9(a); sslam::tv::inv3(a, o); return from9(o); }
    double dot(const Mat& m) const { double r = 0; for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) r += (double)e(i, j) * (double)m.e(i, j); return r; }
    Mat& operator*=(double s) { for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) e(i, j) = (float)((double)e(i, j) * s); return *this; }
    void get9(float a[9]) const { for (int i = 0; i < 9; ++i) a[i] = e(i / 3, i % 3); }
    static Mat from9(const float a[9]) { Mat m(3, 3, CV_32F); for (int i = 0; i < 9; ++i) m.e(i / 3, i % 3) = a[i]; return m; }
};
struct Mat::View : Mat {      // what row() / col() / rowRange() / colRange() return: assigning a matrix to it writes the elements
    View(const Mat& m) : Mat(m) {}
    View& operator=(const Mat& m) { m.write(*this); return *this; }
    View& operator=(const View& m) { m.write(*this); return *this; }
};
inline Mat::View Mat::rowRange(int a, int b) const { Mat m(*this); m.off = off + a * ld; m.rows = b - a; return View(m); }
inline Mat::View Mat::colRange(int a, int b) const { Mat m(*this); m.off = off + a; m.cols = b - a; return View(m); }
inline Mat::View Mat::row(int y) const { return rowRange(y, y + 1); }
inline Mat::View Mat::col(int x) const { return colRange(x, x + 1); }
inline Mat operator*(const Mat& a, const Mat& b) {      // D18 gemm
    Mat r(a.rows, b.cols, CV_32F);
    for (int i = 0; i < a.rows; ++i) for (int j = 0; j < b.cols; ++j) { double acc = 0.0; for (int k = 0; k < a.cols; ++k) acc += (double)a.e(i, k) * (double)b.e(k, j); r.e(i, j) = (float)acc; }
    return r;
}
inline Mat operator*(double s, const Mat& a) { Mat r = a.clone(); r *= s; return r; }      // D18 scale
inline Mat operator/(const Mat& a, double s) { Mat r = a.clone(); r *= 1.0 / s; return r; }
inline Mat operator-(const Mat& a) { Mat r = a.clone(); for (int i = 0; i < r.rows; ++i) for (int j = 0; j < r.cols; ++j) r.e(i, j) = -r.e(i, j); return r; }
inline Mat operator+(const Mat& a, const Mat& b) { Mat r = a.clone(); for (int i = 0; i < r.rows; ++i) for (int j = 0; j < r.cols; ++j) r.e(i, j) = a.e(i, j) + b.e(i, j); return r; }
inline Mat operator-(const Mat& a, const Mat& b) { Mat r = a.clone(); for (int i = 0; i < r.rows; ++i) for (int j = 0; j < r.cols; ++j) r.e(i, j) = a.e(i, j) - b.e(i, j); return r; }
inline double norm(const Mat& a) { return std::sqrt(a.dot(a)); }
inline double determinant(const Mat& a) { float m[9]; a.get9(m); return sslam::rc::det3(m); }
template <class T> struct Mat_ : Mat {
    Mat_(int r, int c) : Mat(r, c, CV_32F) {}
    struct Init { Mat m; int i; template <class U> Init& operator,(U v) { m.e(i / m.cols, i % m.cols) = (T)v; ++i; return *this; } operator Mat() const { return m; } };
    template <class U> Init operator<<(U v) { Init in{*this, 0}; return (in, v); }
};
struct HostWs4 { double m[sslam::rc::WS4_DOUBLES]; double& at(int k) { return m[k]; } };
struct HostWs3 { double m[sslam::rc::WS3_DOUBLES]; double& at(int k) { return m[k - sslam::pnp::WS_S]; } };
struct SVD {      // D18's leaves
    enum { MODIFY_A = 1, FULL_UV = 4 };
    static void compute(const Mat& A, Mat& w, Mat& u, Mat& vt, int = 0) {
        if (A.rows == 3) {
            float a[9], U[9], S[3], Vt[9]; A.get9(a);
            HostWs3 ws; sslam::rc::svd3(ws, a, U, S, Vt);
            u = Mat::from9(U); vt = Mat::from9(Vt); w = Mat(3, 1, CV_32F); for (int i = 0; i < 3; ++i) w.e(i, 0) = S[i];
        } else {
            float a[16], v[4]; for (int i = 0; i < 16; ++i) a[i] = A.e(i / 4, i % 4);
            HostWs4 ws; sslam::rc::svd4_last(ws, a, v);
            u = Mat(4, 4, CV_32F); w = Mat(4, 1, CV_32F); vt = Mat(4, 4, CV_32F); for (int i = 0; i < 4; ++i) vt.e(3, i) = v[i];
        }
    }
};
}
using namespace cv;
struct KeyLine { float startPointX, startPointY, endPointX, endPointY; };
struct Vector3d { double v[3]; double& operator()(int i) { return v[i]; } const double& operator()(int i) const { return v[i]; } };
struct Vector2d { double v[2]; double& operator()(int i) { return v[i]; } double norm() const { return std::sqrt(v[0] * v[0] + v[1] * v[1]); } };
struct Sink { template <class T> Sink& operator<<(const T&) { return *this; } Sink& operator<<(std::ostream& (*)(std::ostream&)) { return *this; } };
static vector<vector<double>> g_mad;      // what vector_mad was handed
"""

CLASS = r"""
inline double logged_mad(vector<double> residues) { g_mad.push_back(residues); return vector_mad(residues); }
namespace StructureSLAM {
static Sink cout;
static inline float acos(float x) { return sslam::rc::acos_f(x); }      // D18 acos
struct Call { cv::Mat R, t; int nGood; float parallax; vector<cv::Point3f> p3d; vector<bool> good; };
class Initializer {
public:
    typedef pair<int, int> Match;
    bool ReconstructF(vector<bool>& vbMatchesInliers, vector<Match>& vLineMatchesF, cv::Mat& F21, cv::Mat& K, cv::Mat& R21, cv::Mat& t21, vector<cv::Point3f>& vP3D,
                      vector<Point3f>& vLineS3D, vector<Point3f>& vLineE3D, vector<bool>& vbTriangulated, vector<bool>& vbLineTriangulated, float minParallax, int minTriangulated);
    bool ReconstructH(vector<bool>& vbMatchesInliers, vector<Match>& vLineMatchesH, cv::Mat& H21, cv::Mat& K, cv::Mat& R21, cv::Mat& t21, vector<cv::Point3f>& vP3D,
                      vector<Point3f>& vLineS3D, vector<Point3f>& vLineE3D, vector<bool>& vbTriangulated, vector<bool>& vbLineTriangulated, float minParallax, int minTriangulated);
    int CheckRT(const cv::Mat& R, const cv::Mat& t, const vector<cv::KeyPoint>& vKeys1, const vector<cv::KeyPoint>& vKeys2, const vector<Match>& vMatches12,
                vector<bool>& vbInliers, const cv::Mat& K, vector<cv::Point3f>& vP3D, float th2, vector<bool>& vbGood, float& parallax);
    int LoggedCheckRT(const cv::Mat& R, const cv::Mat& t, const vector<cv::KeyPoint>& vKeys1, const vector<cv::KeyPoint>& vKeys2, const vector<Match>& vMatches12,
                      vector<bool>& vbInliers, const cv::Mat& K, vector<cv::Point3f>& vP3D, float th2, vector<bool>& vbGood, float& parallax) {
        const int n = CheckRT(R, t, vKeys1, vKeys2, vMatches12, vbInliers, K, vP3D, th2, vbGood, parallax);
        calls.push_back(Call{R.clone(), t.clone(), n, parallax, vP3D, vbGood});
        return n;
    }
    void DecomposeE(const cv::Mat& E, cv::Mat& R1, cv::Mat& R2, cv::Mat& t);
    void Triangulate(const cv::KeyPoint& kp1, const cv::KeyPoint& kp2, const cv::Mat& P1, const cv::Mat& P2, cv::Mat& x3D);
    void LineTriangulate(const KeyLine& kl1, const KeyLine& kl2, const cv::Mat& P1, const cv::Mat& P2, const Vector3d& klf1, const Vector3d& klf2, cv::Mat& LineStart3D,
                         cv::Mat& LineEnd3D);
    void ReconstructLine(vector<Match>& vLineMatches, cv::Mat& K, cv::Mat& R21, cv::Mat& t21, vector<Vector3d>& vKeyLineFunctions1, vector<Vector3d>& vKeyLineFunctions2,
                         vector<Point3f>& vLineS3D, vector<Point3f>& vLineE3D, vector<bool>& vbLineTriangulated);
    vector<cv::KeyPoint> mvKeys1, mvKeys2;
    vector<Match> mvMatches12;
    vector<KeyLine> mvKeyLines1, mvKeyLines2;
    vector<Vector3d> mvKeyLineFunctions1, mvKeyLineFunctions2;
    cv::Mat mK; float mSigma, mSigma2;
    vector<Call> calls;
};
"""

DRIVER = r"""
}
#line 1 "driver"
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static float rd() { unsigned u; if (scanf("%u", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static double rdd() { unsigned long long u; if (scanf("%llu", &u) != 1) exit(2); double f; memcpy(&f, &u, 8); return f; }
static int rdi() { int i; if (scanf("%d", &i) != 1) exit(2); return i; }
static cv::Mat rdmat() { cv::Mat m(3, 3, CV_32F); for (int i = 0; i < 9; ++i) m.at<float>(i / 3, i % 3) = rd(); return m; }
int main() {
    int n1, n2, model;
    while (scanf("%d %d %d", &n1, &n2, &model) == 3) {
        StructureSLAM::Initializer I;
        I.mSigma = rd(); I.mSigma2 = I.mSigma * I.mSigma;
        const float minParallax = rd(); const int minTri = rdi();
        const float fx = rd(), fy = rd(), cx = rd(), cy = rd();
        const int nl1 = rdi(), nl2 = rdi(), nlp = rdi(), hasLines = rdi();
        cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
        K.at<float>(0, 0) = fx; K.at<float>(1, 1) = fy; K.at<float>(0, 2) = cx; K.at<float>(1, 2) = cy;
        I.mK = K.clone();
        for (int i = 0; i < n1; ++i) { cv::KeyPoint k; k.pt.x = rd(); k.pt.y = rd(); I.mvKeys1.push_back(k); }
        for (int i = 0; i < n2; ++i) { cv::KeyPoint k; k.pt.x = rd(); k.pt.y = rd(); I.mvKeys2.push_back(k); }
        vector<int> m12(n1), inl(n1);
        for (int& m : m12) m = rdi();
        for (int& m : inl) m = rdi();
        vector<bool> vbIn;
        for (int i = 0; i < n1; ++i) if (m12[i] >= 0) { I.mvMatches12.push_back(make_pair(i, m12[i])); vbIn.push_back((inl[i] & (model == 1 ? 1 : 2)) != 0); }      // :67-76
        cv::Mat H = rdmat(), F = rdmat();
        vector<pair<int, int>> lm; vector<int> lrow;
        if (hasLines) {
            for (int i = 0; i < nl1; ++i) { KeyLine k; k.startPointX = rd(); k.startPointY = rd(); k.endPointX = rd(); k.endPointY = rd(); I.mvKeyLines1.push_back(k); }
            I.mvKeyLines2.resize(nl2);
            for (int i = 0; i < nl1; ++i) { Vector3d v; for (int k = 0; k < 3; ++k) v(k) = rdd(); I.mvKeyLineFunctions1.push_back(v); }
            for (int i = 0; i < nl2; ++i) { Vector3d v; for (int k = 0; k < 3; ++k) v(k) = rdd(); I.mvKeyLineFunctions2.push_back(v); }
            for (int r = 0; r < nlp; ++r) {
                const int a = rdi(), b = rdi();
                if (a < nl1 && b < nl2 && a >= 0 && b >= 0) { lm.push_back(make_pair(a, b)); lrow.push_back(r); }      // the entry point's filter, then :133
            }
        }
        cv::Mat R21, t21; vector<cv::Point3f> vP3D, S3, E3; vector<bool> tri, ltri;
        bool ok = false;
        g_mad.clear();
        if (model == 1) ok = I.ReconstructH(vbIn, lm, H, K, R21, t21, vP3D, S3, E3, tri, ltri, minParallax, minTri);
        if (model == 2) ok = I.ReconstructF(vbIn, lm, F, K, R21, t21, vP3D, S3, E3, tri, ltri, minParallax, minTri);
        printf("ret %d %d", ok ? 1 : 0, (int)I.calls.size());
        for (int i = 0; i < 9; ++i) printf(" %u", R21.empty() ? 0u : bits(R21.at<float>(i / 3, i % 3)));
        for (int i = 0; i < 3; ++i) printf(" %u", t21.empty() ? 0u : bits(t21.at<float>(i)));
        printf("\np3d");
        for (int i = 0; i < n1; ++i) { const cv::Point3f p = ok && i < (int)vP3D.size() ? vP3D[i] : cv::Point3f(); printf(" %u %u %u %d", bits(p.x), bits(p.y), bits(p.z), ok && i < (int)tri.size() && tri[i] ? 1 : 0); }
        printf("\n");
        for (const StructureSLAM::Call& c : I.calls) {
            printf("call %d %u", c.nGood, bits(c.parallax));
            for (int i = 0; i < 9; ++i) printf(" %u", bits(c.R.at<float>(i / 3, i % 3)));
            for (int i = 0; i < 3; ++i) printf(" %u", bits(c.t.at<float>(i)));
            for (int i = 0; i < n1; ++i) printf(" %u %u %u %d", c.good[i] ? bits(c.p3d[i].x) : 0u, c.good[i] ? bits(c.p3d[i].y) : 0u, c.good[i] ? bits(c.p3d[i].z) : 0u, c.good[i] ? 1 : 0);
            printf("\n");
        }
        printf("lines %d %d", (int)lrow.size(), (int)g_mad.size());
        for (size_t k = 0; k < lrow.size(); ++k) {
            const bool have = ok && k < S3.size();
            const cv::Point3f s = have ? S3[k] : cv::Point3f(), e = have ? E3[k] : cv::Point3f();
            printf(" %d %u %u %u %u %u %u %d", lrow[k], bits(s.x), bits(s.y), bits(s.z), bits(e.x), bits(e.y), bits(e.z), have && ltri[k] ? 1 : 0);
        }
        printf("\n");
        for (const vector<double>& v : g_mad) { printf("mad"); for (double x : v) printf(" %llu", bits(x)); printf("\n"); }
    }
    return 0;
}
"""


def main():
    ref = "/root/reference"
    for a in sys.argv[1:]:
        if a.startswith("REF="):
            ref = a[4:]
    src = os.path.join(ref, "src", "Initializer.cc"); aux = os.path.join(ref, "include", "auxiliar.h")
    lines = open(src, encoding="utf-8", errors="replace").read().split("\n")
    auxl = open(aux, encoding="utf-8", errors="replace").read().split("\n")
    cases = rcases.all_cases()
    with tempfile.TemporaryDirectory() as d:
        cc = os.path.join(d, "reconstruct_ref.cc")
        with open(cc, "w") as f:
            f.write(HEAD)
            f.write('#line %d "%s"\n' % (MAD[0], aux) + "\n".join(auxl[MAD[0] - 1:MAD[1]]) + "\n")
            f.write(CLASS)
            f.write('#define CheckRT LoggedCheckRT\n#line %d "%s"\n' % (SLICES[0][0], src) + "\n".join(lines[SLICES[0][0] - 1:SLICES[0][1]]) + "\n#undef CheckRT\n")
            f.write('#define vector_mad logged_mad\n#line %d "%s"\n' % (SLICES[1][0], src) + "\n".join(lines[SLICES[1][0] - 1:SLICES[1][1]]) + "\n#undef vector_mad\n")
            f.write(DRIVER)
        exe = os.path.join(d, "reconstruct_ref")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "..", "..", "structure-slam-pointline_amd", "csrc"), cc, "-o", exe])
        for c in cases:
            assert (c["m12"] < len(c["kp2"])).all()          # the reference takes every non-negative entry: the cases hold none past frame 2
        out = subprocess.run([exe], input="".join(sim.encode(c) for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    f32 = lambda t: np.array([int(x) for x in t], np.uint64).astype(np.uint32).view(np.float32)
    fx = {"meta": np.array("src/Initializer.cc:%s and include/auxiliar.h:%d-%d of the reference, unmodified, g++ %s between this project's stand-ins, D18's leaves from "
                           "csrc/reconstruct_math.h; inputs: tests/reconstruct_cases.py (tests/golden/make_reconstruct_ref.py)" %
                           (", ".join(":%d-%d" % s for s in SLICES), MAD[0], MAD[1], " ".join(FLAGS))),
          "names": np.array([c["name"] for c in cases])}
    at = 0
    for c in cases:
        n, n1 = c["name"], len(c["kp1"])
        for k in INPUTS:
            fx[n + "/" + k] = np.asarray(c[k])
        fx[n + "/params"] = np.array([c["sigma"], c["min_parallax"], c["min_triangulated"], c["model"]], np.float64)
        if c.get("lp") is not None:
            for k in ("kl1", "fn1", "fn2", "lp"):
                fx[n + "/" + k] = np.asarray(c[k])
        t = out[at].split(); at += 1
        assert t[0] == "ret"
        ok, ncalls = int(t[1]), int(t[2])
        fx[n + "/ok"] = np.int32(ok); fx[n + "/R21"] = f32(t[3:12]); fx[n + "/t21"] = f32(t[12:15])
        t = out[at].split(); at += 1
        a = np.array([int(x) for x in t[1:]], np.uint64).reshape(n1, 4)
        fx[n + "/p3d"] = a[:, :3].astype(np.uint32).view(np.float32).reshape(n1, 3); fx[n + "/tri"] = a[:, 3].astype(np.uint8)
        hyp = np.zeros((8, 12), np.float32); ng = np.zeros(8, np.int32); par = np.zeros(8, np.float32); hp = np.zeros((8, n1, 3), np.float32); hg = np.zeros((8, n1), np.uint8)
        for h in range(ncalls):
            t = out[at].split(); at += 1
            assert t[0] == "call"
            ng[h] = int(t[1]); par[h] = f32(t[2:3])[0]; hyp[h] = f32(t[3:15])
            a = np.array([int(x) for x in t[15:]], np.uint64).reshape(n1, 4)
            hp[h] = a[:, :3].astype(np.uint32).view(np.float32).reshape(n1, 3); hg[h] = a[:, 3]
        fx[n + "/hyp"], fx[n + "/n_good"], fx[n + "/parallax"], fx[n + "/hyp_p3d"], fx[n + "/hyp_good"], fx[n + "/ncalls"] = hyp, ng, par, hp, hg, np.int32(ncalls)
        t = out[at].split(); at += 1
        assert t[0] == "lines"
        nv, nmad = int(t[1]), int(t[2])
        nlp = len(c["lp"]) if c.get("lp") is not None else 0
        ls, le, lt, err, valid = np.zeros((nlp, 3), np.float32), np.zeros((nlp, 3), np.float32), np.zeros(nlp, np.uint8), np.zeros((nlp, 2)), np.zeros(nlp, np.uint8)
        a = np.array([int(x) for x in t[3:]], np.uint64).reshape(nv, 8)
        rows = a[:, 0].astype(np.int64)
        if nv:
            ls[rows] = a[:, 1:4].astype(np.uint32).view(np.float32).reshape(nv, 3); le[rows] = a[:, 4:7].astype(np.uint32).view(np.float32).reshape(nv, 3)
            lt[rows] = a[:, 7]; valid[rows] = 1
        assert nmad in (0, 2)
        for k in range(nmad):
            t = out[at].split(); at += 1
            assert t[0] == "mad" and len(t) == 1 + nv
            err[rows, k] = np.array([int(x) for x in t[1:]], np.uint64).view(np.float64)
        fx[n + "/line_s3d"], fx[n + "/line_e3d"], fx[n + "/line_tri"], fx[n + "/line_err"], fx[n + "/line_valid"], fx[n + "/nmad"] = ls, le, lt, err, valid, np.int32(nmad)
    assert at == len(out)
    path = os.path.join(HERE, "reconstruct_ref.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
