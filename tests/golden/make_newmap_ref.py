#!/usr/bin/env python3
"""Generate tests/golden/newmap_ref.npz: recorded results of the REFERENCE's own loop bodies of LocalMapping::CreateNewMapPoints and CreateNewMapLines2 with
MapPoint::UpdateNormalAndDepth and MapLine::UpdateAverageDir (run where the reference tree is; the fixture is what gets committed, never the cut source or the program).

    python tests/golden/make_newmap_ref.py [REF=/root/reference]

src/LocalMapping.cc:459-617 and :1007-1148, src/MapPoint.cc:353-375 and src/MapLine.cpp:343-371 are cut by line range into a temporary directory and compiled there,
unmodified, between stand-in declarations and a driver (both below, this project's own text), with the flags of FLAGS.  The cv::Mat stand-in is
make_reconstruct_ref.py's (OpenCV's reference semantics, decision D18's arithmetic, cv::SVD::compute of a 4 x 4 = rc::svd4_last filling vt.row(3)); KeyFrame, KeyLine,
Vector3d / Vector6d (plain double; norm() sums as Eigen's unrolled reduction does) and the members the two Update functions touch are carried here.  One name is
redirected with the preprocessor so that the exit a row took can be recorded without touching the reference's text: inside the two loop bodies `continue` first notes its
own line number.  The driver does what the entry points do in front of the reference's text: it drops rows without a match (stage 1) and line rows that are not free
(src/LSDmatcher.cpp:403, stage 2) and clamps octaves into [0, nlevels); the monocular fork's mvuRight is -1 everywhere.
The program runs every case of tests/newmap_cases.py; the fixture keeps inputs and outputs."""
import os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import make_reconstruct_ref as mr       # noqa: E402
import newmap_cases as ncases           # noqa: E402
import newmap_sim as sim                # noqa: E402

POINTS, LINES, MAPPOINT, MAPLINE = (459, 617), (1007, 1148), (353, 375), (343, 371)
FLAGS = mr.FLAGS
# the line of the `continue` a row left through -> the stage code of include/sslam_frontend.h
POINT_EXIT = {512: 3, 527: 2, 535: 4, 539: 5, 558: 6, 585: 7, 608: 8, 616: 9}
LINE_EXIT = {1067: 4, 1085: 5, 1090: 3, 1103: 6, 1109: 7, 1116: 8, 1126: 9, 1131: 10, 1136: 11, 1140: 12, 1144: 13, 1148: 14}
POINT_INPUTS = ("pose1", "pose2", "kp1", "oct1", "kp2", "oct2", "m12", "sf", "sigma2")
LINE_INPUTS = ("pose1", "pose2", "kl1", "loct1", "fn1", "kl2", "loct2", "fn2", "lp", "sf")

_cut = mr.HEAD.index("struct KeyLine")
_kp = "struct KeyPoint { Point2f pt; };"
assert _kp in mr.HEAD
HEAD = "#include <map>\n#include <mutex>\n" + mr.HEAD[:_cut].replace(_kp, "struct KeyPoint { Point2f pt; int octave; };") + r"""
struct KeyLine { float startPointX, startPointY, endPointX, endPointY; int octave; };
struct Vector3d {
    double v[3];
    Vector3d() { v[0] = v[1] = v[2] = 0; }
    Vector3d(double a, double b, double c) { v[0] = a; v[1] = b; v[2] = c; }
    double& operator()(int i) { return v[i]; }
    const double& operator()(int i) const { return v[i]; }
    double norm() const { return std::sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])); }      // Eigen's redux of three terms
};
inline Vector3d operator+(const Vector3d& a, const Vector3d& b) { return Vector3d(a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]); }
inline Vector3d operator-(const Vector3d& a, const Vector3d& b) { return Vector3d(a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]); }
inline Vector3d operator*(double s, const Vector3d& a) { return Vector3d(s * a.v[0], s * a.v[1], s * a.v[2]); }
inline Vector3d operator/(const Vector3d& a, double s) { return Vector3d(a.v[0] / s, a.v[1] / s, a.v[2] / s); }
struct Vector6d {
    double v[6];
    double operator()(int i) const { return v[i]; }
    Vector3d head(int) const { return Vector3d(v[0], v[1], v[2]); }
    Vector3d tail(int) const { return Vector3d(v[3], v[4], v[5]); }
};
struct KeyFrame {
    vector<cv::KeyPoint> mvKeysUn; vector<float> mvuRight, mvDepth; float mb = 0, mbf = 0;
    vector<KeyLine> mvKeyLines; vector<Vector3d> mvKeyLineFunctions;
    vector<float> mvLevelSigma2, mvScaleFactors; int mnScaleLevels = 0; float mfScaleFactor = 0;
    cv::Mat Rcw, tcw, Ow, mK; float fx, fy, cx, cy, invfx, invfy, median = 0;
    cv::Mat UnprojectStereo(int) { return cv::Mat(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    float ComputeSceneMedianDepth(int) { return median; }
};
static vector<int> g_exit;      // per match: the line of the continue it left through, 0 = created
struct PointRec { float x[3], n[3], maxd, mind; };
struct LineRec { float s[3], e[3]; double n[3]; float maxd, mind; };
static vector<PointRec> g_points; static vector<LineRec> g_lines;

struct MapPoint {
    cv::Mat mWorldPos, mNormalVector; float mfMaxDistance = 0, mfMinDistance = 0; std::mutex mMutexPos;
    void UpdateNormalAndDepth(map<KeyFrame*, size_t> observations, KeyFrame* pRefKF) {
        cv::Mat Pos = mWorldPos.clone();
"""

AFTER_MAPPOINT = r"""
    }
};
struct MapLine {
    Vector6d mWorldPos; Vector3d mNormalVector; float mfMaxDistance = 0, mfMinDistance = 0; std::mutex mMutexPos;
    void UpdateAverageDir(map<KeyFrame*, size_t> observations, KeyFrame* pRefKF) {
        Vector6d Pos = mWorldPos;
"""

BEFORE_POINTS = r"""
    }
};
struct Locals {      // what CreateNewMapPoints / CreateNewMapLines2 set up in front of their loops (:383-400, :442-454, :922-942, :990-1003)
    cv::Mat Rcw1, Rwc1, tcw1, Tcw1, Ow1, Rcw2, Rwc2, tcw2, Tcw2, Ow2;
    Locals(KeyFrame* a, KeyFrame* b) {
        Rcw1 = a->Rcw; Rwc1 = Rcw1.t(); tcw1 = a->tcw; Tcw1 = cv::Mat(3, 4, CV_32F); Rcw1.copyTo(Tcw1.colRange(0, 3)); tcw1.copyTo(Tcw1.col(3)); Ow1 = a->GetCameraCenter();
        Rcw2 = b->Rcw; Rwc2 = Rcw2.t(); tcw2 = b->tcw; Tcw2 = cv::Mat(3, 4, CV_32F); Rcw2.copyTo(Tcw2.colRange(0, 3)); tcw2.copyTo(Tcw2.col(3)); Ow2 = b->GetCameraCenter();
    }
};
static void CreateNewMapPoints(KeyFrame* mpCurrentKeyFrame, KeyFrame* pKF2, vector<pair<size_t, size_t> >& vMatchedIndices) {
    Locals L(mpCurrentKeyFrame, pKF2);
    cv::Mat &Rcw1 = L.Rcw1, &Rwc1 = L.Rwc1, &tcw1 = L.tcw1, &Tcw1 = L.Tcw1, &Ow1 = L.Ow1, &Rcw2 = L.Rcw2, &Rwc2 = L.Rwc2, &tcw2 = L.tcw2, &Tcw2 = L.Tcw2, &Ow2 = L.Ow2;
    const float &fx1 = mpCurrentKeyFrame->fx, &fy1 = mpCurrentKeyFrame->fy, &cx1 = mpCurrentKeyFrame->cx, &cy1 = mpCurrentKeyFrame->cy, &invfx1 = mpCurrentKeyFrame->invfx,
                &invfy1 = mpCurrentKeyFrame->invfy;
    const float &fx2 = pKF2->fx, &fy2 = pKF2->fy, &cx2 = pKF2->cx, &cy2 = pKF2->cy, &invfx2 = pKF2->invfx, &invfy2 = pKF2->invfy;
    const float ratioFactor = 1.5f * mpCurrentKeyFrame->mfScaleFactor;
    const int nmatches = vMatchedIndices.size();
    g_exit.assign(nmatches, -1); g_points.assign(nmatches, PointRec());
#define continue if ((g_exit[ikp] = __LINE__), true) continue
"""

AFTER_POINTS = r"""
#undef continue
#line 1 "driver"
            g_exit[ikp] = 0;
            MapPoint mp; mp.mWorldPos = x3D.clone();
            map<KeyFrame*, size_t> obs; obs[mpCurrentKeyFrame] = idx1; obs[pKF2] = idx2;
            mp.UpdateNormalAndDepth(obs, mpCurrentKeyFrame);
            PointRec& r = g_points[ikp];
            for (int k = 0; k < 3; ++k) { r.x[k] = x3D.at<float>(k); r.n[k] = mp.mNormalVector.at<float>(k); }
            r.maxd = mp.mfMaxDistance; r.mind = mp.mfMinDistance;
        }
}
static void CreateNewMapLines2(KeyFrame* mpCurrentKeyFrame, KeyFrame* pKF2, vector<pair<size_t, size_t> >& vMatchedIndices) {
    Locals L(mpCurrentKeyFrame, pKF2);
    cv::Mat &Rcw1 = L.Rcw1, &Rwc1 = L.Rwc1, &tcw1 = L.tcw1, &Tcw1 = L.Tcw1, &Ow1 = L.Ow1, &Rcw2 = L.Rcw2, &Rwc2 = L.Rwc2, &tcw2 = L.tcw2, &Tcw2 = L.Tcw2, &Ow2 = L.Ow2;
    const Mat &K1 = mpCurrentKeyFrame->mK, &K2 = pKF2->mK;
    const float &fx1 = mpCurrentKeyFrame->fx, &fy1 = mpCurrentKeyFrame->fy, &cx1 = mpCurrentKeyFrame->cx, &cy1 = mpCurrentKeyFrame->cy, &invfx1 = mpCurrentKeyFrame->invfx,
                &invfy1 = mpCurrentKeyFrame->invfy;
    const float &fx2 = pKF2->fx, &fy2 = pKF2->fy, &cx2 = pKF2->cx, &cy2 = pKF2->cy, &invfx2 = pKF2->invfx, &invfy2 = pKF2->invfy;
    const int nmatches = vMatchedIndices.size();
    g_exit.assign(nmatches, -1); g_lines.assign(nmatches, LineRec());
#define continue if ((g_exit[ikl] = __LINE__), true) continue
"""

DRIVER = r"""
#undef continue
#line 1 "driver"
            g_exit[ikl] = 0;
            MapLine ml;
            for (int k = 0; k < 3; ++k) { ml.mWorldPos.v[k] = s3D.at<float>(k); ml.mWorldPos.v[3 + k] = e3D.at<float>(k); }
            map<KeyFrame*, size_t> obs; obs[mpCurrentKeyFrame] = idx1; obs[pKF2] = idx2;
            ml.UpdateAverageDir(obs, mpCurrentKeyFrame);
            LineRec& r = g_lines[ikl];
            for (int k = 0; k < 3; ++k) { r.s[k] = s3D.at<float>(k); r.e[k] = e3D.at<float>(k); r.n[k] = ml.mNormalVector(k); }
            r.maxd = ml.mfMaxDistance; r.mind = ml.mfMinDistance;
        }
}
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static float rd() { unsigned u; if (scanf("%u", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static double rdd() { unsigned long long u; if (scanf("%llu", &u) != 1) exit(2); double f; memcpy(&f, &u, 8); return f; }
static int rdi() { int i; if (scanf("%d", &i) != 1) exit(2); return i; }
static void rdpose(KeyFrame& k) {
    k.Rcw = cv::Mat(3, 3, CV_32F); k.tcw = cv::Mat(3, 1, CV_32F); k.Ow = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 9; ++i) k.Rcw.at<float>(i / 3, i % 3) = rd();
    for (int i = 0; i < 3; ++i) k.tcw.at<float>(i) = rd();
    for (int i = 0; i < 3; ++i) k.Ow.at<float>(i) = rd();
    k.fx = rd(); k.fy = rd(); k.cx = rd(); k.cy = rd(); k.invfx = rd(); k.invfy = rd();
    k.mK = cv::Mat::eye(3, 3, CV_32F); k.mK.at<float>(0, 0) = k.fx; k.mK.at<float>(1, 1) = k.fy; k.mK.at<float>(0, 2) = k.cx; k.mK.at<float>(1, 2) = k.cy;
}
static int clampl(int o, int n) { return o < 0 ? 0 : o >= n ? n - 1 : o; }
static void levels(KeyFrame& k, int nlevels, const vector<float>& sf, const vector<float>& s2, float scaleFactor) {
    k.mnScaleLevels = nlevels; k.mvScaleFactors = sf; k.mvLevelSigma2 = s2; k.mfScaleFactor = scaleFactor;
}
int main() {
    int kind, n1;
    while (scanf("%d %d", &kind, &n1) == 2) {
        KeyFrame a, b;
        if (kind == 0) {
            const int n2 = rdi(), nlevels = rdi(); const float scaleFactor = rd();
            rdpose(a); rdpose(b);
            vector<float> sf(nlevels), s2(nlevels);
            for (float& f : sf) f = rd();
            for (float& f : s2) f = rd();
            levels(a, nlevels, sf, s2, scaleFactor); levels(b, nlevels, sf, s2, scaleFactor);
            for (int i = 0; i < n1; ++i) { cv::KeyPoint k; k.pt.x = rd(); k.pt.y = rd(); k.octave = clampl(rdi(), nlevels); a.mvKeysUn.push_back(k); }
            for (int i = 0; i < n2; ++i) { cv::KeyPoint k; k.pt.x = rd(); k.pt.y = rd(); k.octave = clampl(rdi(), nlevels); b.mvKeysUn.push_back(k); }
            a.mvuRight.assign(n1, -1.f); a.mvDepth.assign(n1, -1.f); b.mvuRight.assign(n2, -1.f); b.mvDepth.assign(n2, -1.f);
            vector<pair<size_t, size_t> > vm; vector<int> row;
            for (int i = 0; i < n1; ++i) { const int m = rdi(); if (m >= 0 && m < n2) { vm.push_back(make_pair((size_t)i, (size_t)m)); row.push_back(i); } }
            CreateNewMapPoints(&a, &b, vm);
            printf("points %d", (int)vm.size());
            for (size_t k = 0; k < vm.size(); ++k) {
                const PointRec& r = g_points[k];
                printf(" %d %d %u %u %u %u %u %u %u %u", row[k], g_exit[k], bits(r.x[0]), bits(r.x[1]), bits(r.x[2]), bits(r.n[0]), bits(r.n[1]), bits(r.n[2]), bits(r.maxd), bits(r.mind));
            }
            printf("\n");
        } else {
            const int nl1 = n1, nl2 = rdi(), nrows = rdi(), nlevels = rdi(); const float median = rd(); const int hasFree = rdi();
            rdpose(a); rdpose(b);
            vector<float> sf(nlevels);
            for (float& f : sf) f = rd();
            levels(a, nlevels, sf, sf, 0.f); levels(b, nlevels, sf, sf, 0.f);
            b.median = median;
            KeyFrame* kfs[2] = {&a, &b}; const int nl[2] = {nl1, nl2};
            for (int s = 0; s < 2; ++s) {
                for (int i = 0; i < nl[s]; ++i) { KeyLine k; k.startPointX = rd(); k.startPointY = rd(); k.endPointX = rd(); k.endPointY = rd(); k.octave = clampl(rdi(), nlevels); kfs[s]->mvKeyLines.push_back(k); }
                for (int i = 0; i < nl[s]; ++i) { Vector3d v; for (int k = 0; k < 3; ++k) v(k) = rdd(); kfs[s]->mvKeyLineFunctions.push_back(v); }
            }
            vector<int> lp(2 * nrows), f1(nl1, 1), f2(nl2, 1);
            for (int& p : lp) p = rdi();
            if (hasFree) { for (int& f : f1) f = rdi(); for (int& f : f2) f = rdi(); }
            vector<pair<size_t, size_t> > vm; vector<int> row;
            for (int r = 0; r < nrows; ++r) {
                const int i = lp[2 * r], j = lp[2 * r + 1];
                if (i < 0 || i >= nl1 || j < 0 || j >= nl2) continue;      // stage 1
                if (!f1[i] || !f2[j]) continue;                            // src/LSDmatcher.cpp:403, stage 2
                vm.push_back(make_pair((size_t)i, (size_t)j)); row.push_back(r);
            }
            CreateNewMapLines2(&a, &b, vm);
            printf("lines %d", (int)vm.size());
            for (size_t k = 0; k < vm.size(); ++k) {
                const LineRec& r = g_lines[k];
                printf(" %d %d %u %u %u %u %u %u %llu %llu %llu %u %u", row[k], g_exit[k], bits(r.s[0]), bits(r.s[1]), bits(r.s[2]), bits(r.e[0]), bits(r.e[1]), bits(r.e[2]),
                       bits(r.n[0]), bits(r.n[1]), bits(r.n[2]), bits(r.maxd), bits(r.mind));
            }
            printf("\n");
        }
    }
    return 0;
}
"""


def _slice(path, rng):
    lines = open(path, encoding="utf-8", errors="replace").read().split("\n")
    return '#line %d "%s"\n' % (rng[0], path) + "\n".join(lines[rng[0] - 1:rng[1]]) + "\n"


def main():
    ref = "/root/reference"
    for a in sys.argv[1:]:
        if a.startswith("REF="):
            ref = a[4:]
    lm, mp, ml = (os.path.join(ref, "src", f) for f in ("LocalMapping.cc", "MapPoint.cc", "MapLine.cpp"))
    cases = ncases.all_cases()
    with tempfile.TemporaryDirectory() as d:
        cc = os.path.join(d, "newmap_ref.cc")
        with open(cc, "w") as f:
            f.write(HEAD + _slice(mp, MAPPOINT) + AFTER_MAPPOINT + _slice(ml, MAPLINE) + BEFORE_POINTS + _slice(lm, POINTS) + AFTER_POINTS + _slice(lm, LINES) + DRIVER)
        exe = os.path.join(d, "newmap_ref")
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "..", "..", "structure-slam-pointline_amd", "csrc"), cc, "-o", exe])
        out = subprocess.run([exe], input="".join(sim.encode(c) for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    u32 = lambda a: np.ascontiguousarray(a.astype(np.uint32)).view(np.float32)
    fx = {"meta": np.array("src/LocalMapping.cc:%d-%d and :%d-%d, src/MapPoint.cc:%d-%d and src/MapLine.cpp:%d-%d of the reference, unmodified, g++ %s between this project's "
                           "stand-ins, D18's leaves from csrc/reconstruct_math.h; inputs: tests/newmap_cases.py (tests/golden/make_newmap_ref.py)" %
                           (POINTS + LINES + MAPPOINT + MAPLINE + (" ".join(FLAGS),))),
          "names": np.array([c["name"] for c in cases])}
    for c, ln in zip(cases, out):
        n, t = c["name"], ln.split()
        nv = int(t[1])
        if not sim.is_lines(c):
            assert t[0] == "points"
            for k in POINT_INPUTS:
                fx[n + "/" + k] = np.asarray(c[k])
            fx[n + "/scale_factor"] = np.float64(c["scale_factor"])
            n1 = len(c["oct1"])
            a = np.array([int(x) for x in t[2:]], np.uint64).reshape(nv, 10)
            rows = a[:, 0].astype(np.int64)
            stage = np.full(n1, 1, np.uint8); x3d = np.zeros((n1, 3), np.float32); normal = np.zeros((n1, 3), np.float32); dist = np.zeros((n1, 2), np.float32)
            if nv:
                stage[rows] = [0 if e == 0 else POINT_EXIT[int(e)] for e in a[:, 1]]
                x3d[rows] = u32(a[:, 2:5]); normal[rows] = u32(a[:, 5:8]); dist[rows] = u32(a[:, 8:10])
            fx[n + "/stage"], fx[n + "/x3d"], fx[n + "/normal"], fx[n + "/dist"] = stage, x3d, normal, dist
        else:
            assert t[0] == "lines"
            for k in LINE_INPUTS:
                fx[n + "/" + k] = np.asarray(c[k])
            fx[n + "/median"] = np.float64(c["median"])
            if c["free1"] is not None:
                fx[n + "/free1"], fx[n + "/free2"] = c["free1"], c["free2"]
            nr = len(c["lp"])
            a = np.array([int(x) for x in t[2:]], np.uint64).reshape(nv, 13)
            rows = a[:, 0].astype(np.int64)
            lp, nl1, nl2 = c["lp"], len(c["loct1"]), len(c["loct2"])
            inside = (lp[:, 0] >= 0) & (lp[:, 0] < nl1) & (lp[:, 1] >= 0) & (lp[:, 1] < nl2)
            stage = np.where(inside, 2, 1).astype(np.uint8)      # what the driver dropped
            s3d = np.zeros((nr, 3), np.float32); e3d = np.zeros((nr, 3), np.float32); normal = np.zeros((nr, 3), np.float64); dist = np.zeros((nr, 2), np.float32)
            if nv:
                stage[rows] = [0 if e == 0 else LINE_EXIT[int(e)] for e in a[:, 1]]
                s3d[rows] = u32(a[:, 2:5]); e3d[rows] = u32(a[:, 5:8]); normal[rows] = np.ascontiguousarray(a[:, 8:11]).view(np.float64); dist[rows] = u32(a[:, 11:13])
            fx[n + "/stage"], fx[n + "/s3d"], fx[n + "/e3d"], fx[n + "/normal"], fx[n + "/dist"] = stage, s3d, e3d, normal, dist
    path = os.path.join(HERE, "newmap_ref.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
