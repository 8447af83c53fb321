#!/usr/bin/env python3
"""Generate tests/golden/pnp_ref.npz: recorded results of the REFERENCE's own PnPsolver functions (run where the reference tree is; the fixture is what gets committed,
never the cut source or the program).

    python tests/golden/make_pnp_ref.py [REF=/root/reference]

src/PnPsolver.cc is cut by line range into a temporary directory -- SetRansacParameters (:121-157), iterate (:165-258), Refine (:260-305), CheckInliers (:308-339) and all
of EPnP (:342-950) as whole functions -- and compiled there, unmodified, between a stand-in class declaration and a driver (both below, this project's own text) against
oracle/ref_pin/stub_cv, with the flags of FLAGS.  The stub cv::Mat has no eye() and no convertTo(): -Deye=zeros lets :221 and :298 compile (the last row of the 4 x 4 is not
the reference's; rows 0 .. 2 are recorded), and a macro turns X.convertTo(X, CV_32F) into an assignment of the float copy.  The stub's copyTo takes an lvalue: a macro hands
it the views of :222-223 and :299-300.  cv::Point3f, CvMat, cvMat, cvCreateMat, cvmGet / cvmSet and cvSetZero are a stand-in of the driver; its cvMulTransposed, cvSVD, cvInvert and
cvSolve hand back decision D17's results (the functions of csrc/pnp_math.h) for that call, so that everything between the leaves is the reference's own arithmetic.
RandomInt replays the integers that make the sim's sets through the reference's own swap-with-back.

Recorded per case: SetRansacParameters' two outputs; per iteration the host model ran, from the reference's add_correspondence / compute_pose / CheckInliers on that set:
mRi, mti (64 bits), mnInliersi and mvbInliersi -- every reference-owned function of EPnP (fill_M, compute_L_6x10, compute_rho, gauss_newton with
compute_A_and_b_gauss_newton and qr_solve, compute_ccs / compute_pcs / solve_for_sign, estimate_R_and_t, reprojection_error, the post-solve halves of find_betas_approx_*,
the choice of N) lies between the sets and these bits; per iterate call the return kind, nInliers, bNoMore, vbInliers, mnIterations, mnBestInliers and rows 0 .. 2 of the
returned matrix.  The functions' intermediate outputs are not recorded one by one.  A case runs its leading calls whose every iteration has a set the reference's draw can
produce (four distinct indices in range); LEFT_OUT names the cases without such a call."""
import os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pnp_cases as tc      # noqa: E402
import pnp_sim as sim       # noqa: E402
from host_sim import bits as _bits, ints as _ints      # noqa: E402

FUNCTIONS = ((121, 157), (165, 258), (260, 305), (308, 339), (342, 950))
FLAGS = ["-O2", "-std=c++11", "-ffp-contract=off", "-w", "-Deye=zeros"]
# sets out of range and past the caller's list in the first call; N below min_inliers (iterate returns at :173, no iteration to record); a set that names one point twice
LEFT_OUT = ("past_nsets_and_out_of_range", "n_0", "n_3", "n_min_minus_1", "repeated_point")
OUT = os.path.join(HERE, "pnp_ref.npz")

HEAD = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <vector>
#include <opencv2/core/core.hpp>
#include "pnp_math.h"
namespace cv { struct Point3f { float x, y, z; Point3f() : x(0), y(0), z(0) {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} }; }      // not in the stub
template <class T> static T& sslam_lvalue(T&& t) { return t; }
#define copyTo(x) copyTo(sslam_lvalue(x))
static cv::Mat sslam_to_float(const cv::Mat& m) { cv::Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; ++i) for (int j = 0; j < m.cols; ++j) r.at<float>(i, j) = (float)m.at<double>(i, j); return r; }
#define convertTo(dst, type) operator=(sslam_to_float(dst))
using namespace std;
struct CvMat { int rows, cols; struct { double* db; } data; };
#define CV_SVD 1
#define CV_SVD_MODIFY_A 1
#define CV_SVD_U_T 2
static CvMat cvMat(int r, int c, int, void* p) { CvMat m; m.rows = r; m.cols = c; m.data.db = (double*)p; return m; }
static CvMat* cvCreateMat(int r, int c, int) { CvMat* m = new CvMat; m->rows = r; m->cols = c; m->data.db = new double[(size_t)r * c]; return m; }
static void cvReleaseMat(CvMat** m) { delete[] (*m)->data.db; delete *m; *m = 0; }
static double cvmGet(const CvMat* m, int i, int j) { return m->data.db[i * m->cols + j]; }
static void cvmSet(CvMat* m, int i, int j, double v) { m->data.db[i * m->cols + j] = v; }
static void cvSetZero(CvMat* m) { for (int i = 0; i < m->rows * m->cols; ++i) m->data.db[i] = 0.0; }
// decision D17's leaves, from csrc/pnp_math.h
namespace d17 {
using namespace sslam::pnp;
struct Ws { double d[WS_DOUBLES]; double& at(int k) { return d[k]; } };
static Ws W;
template <int N> static void sym(const CvMat* A, CvMat* D, CvMat* Ut) {
    for (int i = 0; i < N; ++i) for (int j = i; j < N; ++j) W.at(sym_index(N, i, j)) = A->data.db[i * N + j];
    jacobi_sym<N>(W);
    for (int i = 0; i < N; ++i) {
        const int r = sym_rank<N>(W, i);
        D->data.db[r] = fabs(W.at(sym_index(N, i, i)));
        for (int k = 0; k < N; ++k) Ut->data.db[r * N + k] = W.at(78 + k * N + i);
    }
}
template <int NC> static void solve(const CvMat* A, const CvMat* b, CvMat* x) {
    for (int i = 0; i < 6; ++i) { for (int c = 0; c < NC; ++c) os_a<6, NC>(W, i, c) = A->data.db[i * NC + c]; W.at(WS_RHO + i) = b->data.db[i]; }
    double o[NC];
    solve_svd<NC>(W, o);
    for (int c = 0; c < NC; ++c) x->data.db[c] = o[c];
}
}
static void cvMulTransposed(const CvMat* A, CvMat* dst, int order) {
    if (order != 1) exit(4);
    for (int i = 0; i < A->cols; ++i) for (int j = 0; j < A->cols; ++j) { double acc = 0.0; for (int r = 0; r < A->rows; ++r) acc += A->data.db[r * A->cols + i] * A->data.db[r * A->cols + j]; dst->data.db[i * A->cols + j] = acc; }
}
static void cvSVD(CvMat* A, CvMat* D, CvMat* U, CvMat* V, int flags) {
    using namespace d17;
    if (!V) {
        if (!(flags & CV_SVD_U_T)) exit(4);
        if (A->rows == 3) sym<3>(A, D, U); else if (A->rows == 12) sym<12>(A, D, U); else exit(4);
    } else {
        if (A->rows != 3 || (flags & CV_SVD_U_T)) exit(4);
        for (int k = 0; k < 9; ++k) W.at(WS_S + k) = A->data.db[k];
        double u[9], v[9];
        svd3_uv(W, u, v);
        for (int k = 0; k < 9; ++k) { U->data.db[k] = u[k]; V->data.db[k] = v[k]; }
        for (int k = 0; k < 3; ++k) D->data.db[k] = 0.0;      // never read (:590-612)
    }
}
static void cvInvert(CvMat* A, CvMat* dst, int) {
    using namespace d17;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) os_a<3, 3>(W, i, j) = A->data.db[i * 3 + j];
    double ci[9];
    pinv3(W, ci);
    for (int k = 0; k < 9; ++k) dst->data.db[k] = ci[k];
}
static void cvSolve(const CvMat* A, const CvMat* b, CvMat* x, int) {
    if (A->rows != 6) exit(4);
    if (A->cols == 4) d17::solve<4>(A, b, x); else if (A->cols == 3) d17::solve<3>(A, b, x); else if (A->cols == 5) d17::solve<5>(A, b, x); else exit(4);
}
namespace DUtils { namespace Random { int RandomInt(int lo, int hi); } }
namespace StructureSLAM {
class MapPoint;
class Frame;
class PnPsolver {
public:
    PnPsolver() : pws(0), us(0), alphas(0), pcs(0), maximum_number_of_correspondences(0), number_of_correspondences(0), mnInliersi(0), mnIterations(0), mnBestInliers(0), N(0) {}
    void SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2);
    cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers);
    void CheckInliers();
    bool Refine();
    void set_maximum_number_of_correspondences(const int n);
    void reset_correspondences(void);
    void add_correspondence(const double X, const double Y, const double Z, const double u, const double v);
    double compute_pose(double R[3][3], double T[3]);
    void relative_error(double& rot_err, double& transl_err, const double Rtrue[3][3], const double ttrue[3], const double Rest[3][3], const double test[3]);
    void print_pose(const double R[3][3], const double t[3]);
    double reprojection_error(const double R[3][3], const double t[3]);
    void choose_control_points(void);
    void compute_barycentric_coordinates(void);
    void fill_M(CvMat* M, const int row, const double* alphas, const double u, const double v);
    void compute_ccs(const double* betas, const double* ut);
    void compute_pcs(void);
    void solve_for_sign(void);
    void find_betas_approx_1(const CvMat* L_6x10, const CvMat* Rho, double* betas);
    void find_betas_approx_2(const CvMat* L_6x10, const CvMat* Rho, double* betas);
    void find_betas_approx_3(const CvMat* L_6x10, const CvMat* Rho, double* betas);
    void qr_solve(CvMat* A, CvMat* b, CvMat* X);
    double dot(const double* v1, const double* v2);
    double dist2(const double* p1, const double* p2);
    void compute_rho(double* rho);
    void compute_L_6x10(const double* ut, double* l_6x10);
    void gauss_newton(const CvMat* L_6x10, const CvMat* Rho, double current_betas[4]);
    void compute_A_and_b_gauss_newton(const double* l_6x10, const double* rho, double cb[4], CvMat* A, CvMat* b);
    double compute_R_and_t(const double* ut, const double* betas, double R[3][3], double t[3]);
    void estimate_R_and_t(double R[3][3], double t[3]);
    void copy_R_and_t(const double R_dst[3][3], const double t_dst[3], double R_src[3][3], double t_src[3]);
    void mat_to_quat(const double R[3][3], double q[4]);
    double uc, vc, fu, fv;
    double *pws, *us, *alphas, *pcs;
    int maximum_number_of_correspondences, number_of_correspondences;
    double cws[4][3], ccs[4][3];
    vector<MapPoint*> mvpMapPointMatches;
    vector<cv::Point2f> mvP2D;
    vector<float> mvSigma2;
    vector<cv::Point3f> mvP3Dw;
    vector<size_t> mvKeyPointIndices;
    double mRi[3][3], mti[3];
    vector<bool> mvbInliersi; int mnInliersi;
    int mnIterations; vector<bool> mvbBestInliers; int mnBestInliers; cv::Mat mBestTcw;
    cv::Mat mRefinedTcw; vector<bool> mvbRefinedInliers; int mnRefinedInliers;
    int N;
    vector<size_t> mvAllIndices;
    double mRansacProb; int mRansacMinInliers, mRansacMaxIts; float mRansacEpsilon; int mRansacMinSet;
    vector<float> mvMaxError;
};
"""

TAIL = r"""
}  // namespace StructureSLAM
static std::deque<int> g_randi;
int DUtils::Random::RandomInt(int, int) { if (g_randi.empty()) exit(3); const int r = g_randi.front(); g_randi.pop_front(); return r; }
static float rdf() { unsigned u; if (scanf("%u", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static double rdd() { unsigned long long u; if (scanf("%llu", &u) != 1) exit(2); double f; memcpy(&f, &u, 8); return f; }
static int rdi() { int v; if (scanf("%d", &v) != 1) exit(2); return v; }
static unsigned long long b64(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static unsigned b32(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main() {
    int N;
    while (scanf("%d", &N) == 1) {
        StructureSLAM::PnPsolver S;
        const int nf = rdi(), minInliers = rdi(), maxIterations = rdi(), ncalls = rdi(), nits = rdi();
        const double probability = rdd(); const float epsilon = rdf(), th2 = rdf();
        S.fu = rdf(); S.fv = rdf(); S.uc = rdf(); S.vc = rdf();      // :104-107: doubles from the frame's floats
        S.mvpMapPointMatches.assign((size_t)nf, (StructureSLAM::MapPoint*)0);
        for (int i = 0; i < N; ++i) {      // what :87-96 push, from the test's correspondence list
            const int j = rdi(); const float s2 = rdf(), x = rdf(), y = rdf(), z = rdf(), u = rdf(), v = rdf();
            S.mvP2D.push_back(cv::Point2f(u, v)); S.mvSigma2.push_back(s2); S.mvP3Dw.push_back(cv::Point3f(x, y, z)); S.mvKeyPointIndices.push_back((size_t)j); S.mvAllIndices.push_back((size_t)i);
        }
        S.SetRansacParameters(probability, minInliers, maxIterations, 4, epsilon, th2);
        printf("params %d %d\n", S.mRansacMinInliers, S.mRansacMaxIts);
        std::vector<int> calls((size_t)ncalls), sets((size_t)nits * 4), randi((size_t)nits * 4);
        for (int& c : calls) c = rdi();
        for (int k = 0; k < nits; ++k) { for (int j = 0; j < 4; ++j) sets[(size_t)k * 4 + j] = rdi(); for (int j = 0; j < 4; ++j) randi[(size_t)k * 4 + j] = rdi(); }
        // every set on its own: add_correspondence, compute_pose, CheckInliers (:186-207)
        S.set_maximum_number_of_correspondences(4);
        for (int k = 0; k < nits; ++k) {
            S.reset_correspondences();
            for (int j = 0; j < 4; ++j) { const int idx = sets[(size_t)k * 4 + j]; S.add_correspondence(S.mvP3Dw[idx].x, S.mvP3Dw[idx].y, S.mvP3Dw[idx].z, S.mvP2D[idx].x, S.mvP2D[idx].y); }
            S.compute_pose(S.mRi, S.mti);
            S.CheckInliers();
            printf("hyp");
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) printf(" %llu", b64(S.mRi[i][j]));
            for (int i = 0; i < 3; ++i) printf(" %llu", b64(S.mti[i]));
            printf(" %d ", S.mnInliersi);
            for (int i = 0; i < N; ++i) putchar(S.mvbInliersi[(size_t)i] ? '1' : '0');
            printf("\n");
        }
        // the calls
        for (int r : randi) g_randi.push_back(r);
        for (int c = 0; c < ncalls; ++c) {
            bool bNoMore; std::vector<bool> vb; int nInliers;
            cv::Mat T = S.iterate(calls[(size_t)c], bNoMore, vb, nInliers);
            printf("call %d %d %d %d %d", T.empty() ? 0 : 1, nInliers, bNoMore ? 1 : 0, S.mnIterations, S.mnBestInliers);
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) printf(" %u", T.empty() ? 0u : b32(T.at<float>(i, j)));
            printf(" ");
            if (vb.empty()) putchar('-');
            for (size_t i = 0; i < vb.size(); ++i) putchar(vb[i] ? '1' : '0');
            printf("\n");
        }
        if (!g_randi.empty()) exit(5);
    }
    return 0;
}
"""


def randi_for(n, s):
    """the integers RandomInt has to return so that the swap-with-back of :188-201 takes the indices s out of n"""
    avail = list(range(n)); out = []
    for x in s:
        r = avail.index(int(x)); out.append(r)
        avail[r] = avail[-1]; avail.pop()
    return out


def plan(c, got):
    """the leading calls of a case whose every iteration has a producible set -> (number of calls, iterations)"""
    ncalls, its = 0, 0
    for cl in got["calls"]:
        ok = len(cl["its"]) > 0 and all(len(set(s.tolist())) == 4 and min(s) >= 0 and max(s) < got["n"] for s in cl["sets"])
        if not ok:
            break
        ncalls += 1; its += len(cl["its"])
    return ncalls, its


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    lines = open(os.path.join(ref, "src", "PnPsolver.cc"), encoding="utf-8", errors="replace").read().split("\n")
    B = tc.build()
    names = list(B)
    cs = [tc.public(B[n]) for n in names]
    got = sim.run(cs)
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "cut.cc"), os.path.join(d, "cut")
        with open(cc, "w") as f:
            f.write(HEAD + "\n".join("\n".join(lines[a - 1:b]) for a, b in FUNCTIONS) + TAIL)
        root = os.path.join(HERE, "..", "..")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(root, "oracle", "ref_pin", "stub_cv"), "-I" + os.path.join(root, "structure-slam-pointline_amd", "csrc"), cc, "-o", exe])
        text, used, left = [], [], []
        for name, c, g in zip(names, cs, got):
            ncalls, nits = plan(c, g)
            if ncalls == 0:
                left.append(name); continue
            used.append((name, c, g, ncalls, nits))
            N = g["n"]
            idx, oct_, pt, xw, a = g["idx"], np.asarray(c["oct"]), np.asarray(c["pt"], np.float32), np.asarray(c["xw"], np.float32), np.asarray(c["assigned"])
            head = "%d %d %d %d %d %d" % (N, len(oct_), c["min_inliers"], c["max_iterations"], ncalls, nits)
            text.append(head + " " + str(int(np.float64(c["probability"]).view(np.uint64))) + " " + _bits([c["epsilon"], c["th2"]]) + " " + _bits(c["K"]) + "\n")
            for i in range(N):
                j = int(idx[i])
                text.append("%d %s\n" % (j, _bits([np.asarray(c["sigma2"], np.float32)[oct_[j]], *xw[a[j]], *pt[j]])))
            text.append(_ints(c["calls"][:ncalls]) + "\n")
            for cl in g["calls"][:ncalls]:
                for s in cl["sets"]:
                    text.append(_ints(s) + " " + _ints(randi_for(N, s)) + "\n")
        assert tuple(left) == LEFT_OUT, (left, LEFT_OUT)
        out = subprocess.run([exe], input="".join(text), capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        out = out.stdout.splitlines()
    fx, at = {"names": np.array([u[0] for u in used]), "left_out": np.array(LEFT_OUT)}, 0
    for name, c, g, ncalls, nits in used:
        t = out[at].split(); at += 1
        assert t[0] == "params"
        fx[name + "/params"] = np.array([int(t[1]), int(t[2])], np.int32)
        fx[name + "/sets"] = np.concatenate([cl["sets"] for cl in g["calls"][:ncalls]]).astype(np.int32)
        poses, counts, marks = [], [], []
        for _ in range(nits):
            t = out[at].split(); at += 1
            assert t[0] == "hyp"
            poses.append([int(x) for x in t[1:13]]); counts.append(int(t[13])); marks.append(np.frombuffer(t[14].encode(), np.uint8) - 48)
        fx[name + "/poses"] = np.array(poses, np.uint64).view(np.float64).reshape(nits, 12)
        fx[name + "/counts"] = np.array(counts, np.int32)
        fx[name + "/marks"] = np.packbits(np.array(marks, np.uint8).reshape(nits, g["n"]), axis=1)
        calls, tcw, inl = [], [], []
        for _ in range(ncalls):
            t = out[at].split(); at += 1
            assert t[0] == "call"
            calls.append([int(x) for x in t[1:6]]); tcw.append([int(x) for x in t[6:18]])
            inl.append(np.zeros(len(c["oct"]), np.uint8) if t[18] == "-" else np.frombuffer(t[18].encode(), np.uint8) - 48)
        fx[name + "/calls"] = np.array(calls, np.int32)      # returned a matrix, nInliers, bNoMore, mnIterations, mnBestInliers
        fx[name + "/tcw"] = np.array(tcw, np.uint64).astype(np.uint32).view(np.float32).reshape(ncalls, 12)
        fx[name + "/inliers"] = np.packbits(np.array(inl, np.uint8).reshape(ncalls, len(c["oct"])), axis=1)
    assert at == len(out)
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(used), "cases, left out", LEFT_OUT)


if __name__ == "__main__":
    main()
