"""Inputs of the batch Fuse / SearchBySim3 candidate-search tests (tests/test_fuse_batch_gpu.py, tests/test_fuse_batch_cases_cpu.py).  A case is
dict(kind, chi2, pool, blocks, jobs): pool = keyframes dict(feats, desc[, uright]) in slot order, blocks = descriptor blocks [m, 32] laid end to end in
d_qdesc, jobs = dict(kf = slot, q = PQ rows, block[, off = first row inside the block]).  expect() = helper + CPU oracle (oracle.fuse_search), job by
job: the expectation of both test files.  The gate cases pick their numbers with the matcher's own float expressions (point_window_ok, chi2_ok,
line_ok), one float32 operation at a time.  Every generator is a pure function of its numpy Generator."""
import numpy as np
import match_cases as mc
import bow_batch_cases as bc
from tri_batch_cases import bisect
from oracle_lib import KP_DTYPE, KL_DTYPE

PQ_DTYPE = mc.PQ_DTYPE
JOB_DTYPE = np.dtype([("kf", "<i4"), ("nq", "<i4"), ("qdesc0", "<i4")])      # sslam_fuse_job (frontend.FUSE_JOB_DTYPE)
W = 8                                   # waves per workgroup of k_fuse_search_batch (csrc/match_plan.h BATCH_WAVES)
ROW_BYTES = 16                          # LDS bytes per keyframe row (FUSE_BATCH_ROW_BYTES)
CHUNK = 256                             # queries per workgroup (FUSE_BATCH_CHUNK)
LDS_MAX = 64 * 1024                     # BATCH_LDS_MAX
LDS_DEFAULT = 48 * 1024                 # DYNAMIC_LDS_DEFAULT_MAX
LDS_CAP = LDS_MAX // ROW_BYTES          # 4096: the last row capacity whose geometry sits in LDS
PLAIN_CAP = LDS_DEFAULT // ROW_BYTES    # 3072: the last row capacity without the dynamic-LDS opt-in
TH_LOW = 50
NLEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
INV_SIGMA2 = (np.float32(1) / (SCALE * SCALE)).astype(np.float32)         # KeyFrame::mvInvLevelSigma2
ORACLE_TABLE = np.concatenate([INV_SIGMA2, np.zeros(24, np.float32)])     # the oracle indexes its table with any admitted level: a level past the table weighs 0
BOUNDS = (0.0, 640.0, 0.0, 480.0)                                         # cells of 10 x 10 pixels: column round(x / 10), row round(y / 10)
INT_MAX = 0x7fffffff
f32 = np.float32


# ---- the matcher's gates in its own float arithmetic (csrc/match_independent.h fuse_point_window, fuse_point_chi2, fuse_line_ok)
def point_window_ok(u, v, r, x, y):
    return bool(abs(f32(f32(x) - f32(u))) < f32(r) and abs(f32(f32(y) - f32(v))) < f32(r))


def chi2_ok(u, v, qur, x, y, ur, inv):
    ex = f32(f32(u) - f32(x)); ey = f32(f32(v) - f32(y))
    e2 = f32(f32(ex * ex) + f32(ey * ey))
    if ur >= 0:
        er = f32(f32(qur) - f32(ur)); e2 = f32(e2 + f32(er * er))
        return not float(f32(e2 * f32(inv))) > 7.8
    return not float(f32(e2 * f32(inv))) > 5.99


def line_distance_ok(u, v, u2, v2, r, px, py):
    mx = 0.5 * float(f32(f32(u) + f32(u2))) - float(f32(px)); my = 0.5 * float(f32(f32(v) + f32(v2))) - float(f32(py))
    return not f32(mx * mx + my * my) > f32(f32(r) * f32(r))


def line_slope_ok(u, v, u2, v2, r, angle):
    with np.errstate(all="ignore"):
        slope = f32(f32(f32(f32(v) - f32(v2)) / f32(f32(u) - f32(u2))) - f32(angle))
    return not float(slope) > float(f32(r)) * 0.01


# ---- helper + oracle
def keyframe(feats, desc, uright=None):
    k = dict(feats=feats, desc=np.ascontiguousarray(desc, np.uint8))
    if uright is not None: k["uright"] = np.asarray(uright, np.float32)
    return k


def cut(k, n):
    return {a: v[:n].copy() for a, v in k.items()}


def job(kf, q, block, off=0):
    return dict(kf=int(kf), q=np.ascontiguousarray(q, PQ_DTYPE), block=int(block), off=int(off))


def case(kind, chi2, pool, blocks, jobs):
    return dict(kind=kind, chi2=chi2, pool=pool, blocks=[np.ascontiguousarray(b, np.uint8).reshape(-1, 32) for b in blocks], jobs=jobs)


def job_desc(c, j):
    return c["blocks"][j["block"]][j["off"]:j["off"] + len(j["q"])]


def expect_job(oracle, c, j):
    """(best_idx[nq], best_dist[nq]) of one job: the CPU oracle on the job's keyframe"""
    k = c["pool"][j["kf"]]
    nq = len(j["q"])
    if nq == 0: return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if len(k["feats"]) == 0: return np.full(nq, -1, np.int32), np.full(nq, INT_MAX, np.int32)
    return oracle.fuse_search(c["kind"], c["chi2"], k["feats"], k["desc"], j["q"], job_desc(c, j), k.get("uright"), ORACLE_TABLE, BOUNDS)


def expect(oracle, c):
    return [expect_job(oracle, c, j) for j in c["jobs"]]


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _kps(n):
    k = np.zeros(n, KP_DTYPE); k["size"] = 31; k["class_id"] = -1
    return k


def _kls(n):
    k = np.zeros(n, KL_DTYPE); k["size"] = 1; k["response"] = 0.5; k["class_id"] = np.arange(n)
    return k


def _query(u, v, r, lo, hi, u2=0.0, v2=0.0, ur=0.0, valid=1):
    q = np.zeros(1, PQ_DTYPE)
    q["u"] = u; q["v"] = v; q["u2"] = u2; q["v2"] = v2; q["radius"] = r; q["min_level"] = lo; q["max_level"] = hi; q["ur"] = ur; q["valid"] = valid; q["obs_positive"] = 1
    return q


# ---- 1. the ragged pool: slots of one capacity whose counts sit on the lane loop's edges, jobs whose counts sit on the chunk's
RAGGED_CAP, RAGGED_QCAP = 96, 300
RAGGED_COUNTS = (96, 0, 1, 63, 64, 65)
RAGGED_NQ = (0, 1, 255, 256, 257, 300)
RAGGED_MODES = ((0, 0), (0, 1), (1, 0))                  # (kind, chi2)


def ragged_pool(rng, kind, chi2):
    """six slots cut from one keyframe of 96 features, 300 queries aimed at it in ONE descriptor block; a job per (slot, query count): 36 jobs with every
    combination of an empty and a non-empty keyframe and job"""
    c = mc.fuse_case(rng, kind, RAGGED_CAP, RAGGED_QCAP)
    full = keyframe(c["feats"], c["desc"], c["uright"])
    pool = [cut(full, n) for n in RAGGED_COUNTS]
    jobs = [job(s, c["q"][:nq], 0) for s in range(len(pool)) for nq in RAGGED_NQ]
    return case(kind, chi2, pool, [c["qdesc"]], jobs)


# ---- 2. one query against chosen rows
def window_case(rng, m, pos, nfill=20):
    """a keyframe of m + nfill keypoints: m inside the query's window at ascending scattered rows, the one at position `pos` 5 bits from the query's
    descriptor, and nfill rows far outside -> (case of one job with one query, winning row)"""
    n = m + nfill
    rows = np.sort(rng.choice(n, m, replace=False))
    kp = _kps(n); kp["x"] = rng.uniform(20, 200, n); kp["y"] = rng.uniform(20, 460, n); kp["octave"] = 1
    kp["x"][rows] = 400 + rng.uniform(-6, 6, m); kp["y"][rows] = 240 + rng.uniform(-6, 6, m)
    d = mc.rand_desc(rng, n); qd = mc.rand_desc(rng, 1)
    d[rows[pos]] = bc._flip(qd[0], rng.choice(256, 5, replace=False))
    return case(0, 0, [keyframe(kp, d)], [qd], [job(0, _query(400.0, 240.0, 8.0, 0, 1), 0)]), int(rows[pos])


def lane_cases(rng):
    """name -> (case, winning row): a window of 1 / 63 / 64 / 65 / 129 admissible rows, the winner first, in the middle, last"""
    return {"lane_%d_%d" % (m, pos): window_case(rng, m, pos) for m in (1, 63, 64, 65, 129) for pos in sorted({0, m // 2, m - 1})}


def tie_cases(rng):
    """name -> (case, winning row).  Two rows at one distance from the query: GetFeaturesInArea walks the window's cells column by column (inside a cell
    in ascending index), so with the HIGHER row in the earlier column it wins; inside one cell, and for lines (GetLinesInArea walks the rows in index
    order), the lower row wins"""
    out = {}
    for name, xs in (("two_cells", {7: 101.0, 3: 107.0}), ("one_cell", {7: 101.0, 3: 102.5})):
        n = 12
        kp = _kps(n); kp["x"] = rng.uniform(300, 600, n); kp["y"] = rng.uniform(20, 460, n); kp["octave"] = 0
        d = mc.rand_desc(rng, n); qd = mc.rand_desc(rng, 1); perm = rng.permutation(256)
        for k, (row, x) in enumerate(xs.items()):
            kp["x"][row] = x; kp["y"][row] = 200.0; d[row] = bc._flip(qd[0], perm[10 * k:10 * k + 10])
        out["tie_" + name] = (case(0, 0, [keyframe(kp, d)], [qd], [job(0, _query(104.0, 200.0, 8.0, 0, 0), 0)]), 7 if name == "two_cells" else 3)
    n = 12
    kl = _kls(n); kl["pt_x"] = rng.uniform(300, 600, n); kl["pt_y"] = rng.uniform(20, 460, n)
    d = mc.rand_desc(rng, n); qd = mc.rand_desc(rng, 1); perm = rng.permutation(256)
    for k, (row, x) in enumerate({9: 101.0, 4: 107.0}.items()):
        kl["pt_x"][row] = x; kl["pt_y"][row] = 200.0; kl["angle"][row] = 0.5; d[row] = bc._flip(qd[0], perm[10 * k:10 * k + 10])
    out["tie_lines"] = (case(1, 0, [keyframe(kl, d)], [qd], [job(0, _query(94.0, 196.0, 8.0, 0, 0, u2=114.0, v2=204.0), 0)]), 4)      # midpoint (104, 200), slope 0.4
    return out


def _one_point(x, y, octave, ur, q, nfill_rng):
    """a keyframe whose row 2 is the keypoint under test, among four far rows with and without a right coordinate; its descriptor is the query's"""
    n = 5
    kp = _kps(n); kp["x"] = nfill_rng.uniform(20, 100, n); kp["y"] = nfill_rng.uniform(20, 100, n); kp["octave"] = 0
    uright = np.array([-1, 30, -1, 40, -1], np.float32)
    kp["x"][2] = x; kp["y"][2] = y; kp["octave"][2] = octave; uright[2] = ur
    d = mc.rand_desc(nfill_rng, n); qd = d[2:3].copy()
    return keyframe(kp, d, uright), qd, q


def point_gate_cases(rng):
    """name -> (keyframe, query descriptor, query, found, chi2): the keypoint under test is row 2 and carries the query's descriptor.  Each `in` / `out`
    pair differs in ONE float by one unit in the last place"""
    out = {}
    up = lambda a: np.nextafter(f32(a), f32(1e9))
    # |dx| < r, |dy| < r: strict
    u, v, r = 300.0, 200.0, 5.0
    xi, xo = bisect(lambda x: point_window_ok(u, v, r, x, v), 304.0, 306.0)
    yi, yo = bisect(lambda y: point_window_ok(u, v, r, u, y), 204.0, 206.0)
    assert up(xi) == xo and up(yi) == yo
    for name, x, y, found in (("dx_in", xi, v, True), ("dx_out", xo, v, False), ("dy_in", u, yi, True), ("dy_out", u, yo, False)):
        out["window_" + name] = _one_point(x, y, 0, -1.0, _query(u, v, r, 0, 0), rng) + (found, 0)
    # 5.99 (monocular) and 7.8 (stereo), at a weight of 1 and at a weight below 1; the stereo keypoint's right coordinate is 1 px off the query's
    for octave in (0, 2):
        inv = INV_SIGMA2[octave]
        for name, ur, qur in (("mono", -1.0, 0.0), ("stereo", 250.0, 251.0)):
            xi, xo = bisect(lambda x: chi2_ok(u, v, qur, x, v, ur, inv), u, u + 9.0)
            assert up(xi) == xo and xi > u + 2
            for side, x, found in (("in", xi, True), ("out", xo, False)):
                out["chi2_%s_oct%d_%s" % (name, octave, side)] = _one_point(x, v, octave, ur, _query(u, v, 12.0, octave, octave, ur=qur), rng) + (found, 1)
    # the level window [min_level, max_level]
    for name, octave, found in (("min-1", 1, False), ("min", 2, True), ("max", 3, True), ("max+1", 4, False)):
        out["level_" + name] = _one_point(u + 1, v, octave, -1.0, _query(u, v, r, 2, 3), rng) + (found, 0)
    # an octave outside the level table weighs 0: 9 px off passes where a level of the table (weight 1: 81 > 5.99) does not
    out["octave_past_table"] = _one_point(u + 9, v, NLEVELS + 1, -1.0, _query(u, v, 12.0, NLEVELS, NLEVELS + 1), rng) + (True, 1)
    out["octave_in_table"] = _one_point(u + 9, v, 0, -1.0, _query(u, v, 12.0, 0, 1), rng) + (False, 1)
    out["not_valid"] = _one_point(u + 1, v, 0, -1.0, _query(u, v, r, 0, 0, valid=0), rng) + (False, 0)
    out["valid"] = _one_point(u + 1, v, 0, -1.0, _query(u, v, r, 0, 0), rng) + (True, 0)
    return out


def outside_grid_case(rng):
    """-> (case, the row that wins, the row outside the grid).  x = 637 rounds to column 64 of 64: AssignFeaturesToGrid files the keypoint nowhere, so no
    window finds it although it lies inside this one and carries the query's own descriptor; the row in column 63, 12 bits away, wins"""
    n = 8
    kp = _kps(n); kp["x"] = rng.uniform(20, 300, n); kp["y"] = rng.uniform(20, 460, n)
    d = mc.rand_desc(rng, n); qd = mc.rand_desc(rng, 1)
    kp["x"][5] = 637.0; kp["y"][5] = 100.0; d[5] = qd[0]
    kp["x"][1] = 631.0; kp["y"][1] = 100.0; d[1] = bc._flip(qd[0], rng.choice(256, 12, replace=False))
    return case(0, 0, [keyframe(kp, d)], [qd], [job(0, _query(634.0, 100.0, 6.0, 0, 0), 0)]), 1, 5


def _one_line(px, py, angle, octave, q, rng):
    n = 5
    kl = _kls(n); kl["pt_x"] = rng.uniform(20, 100, n); kl["pt_y"] = rng.uniform(20, 100, n); kl["angle"] = 0.3
    kl["pt_x"][2] = px; kl["pt_y"][2] = py; kl["angle"][2] = angle; kl["octave"][2] = octave
    d = mc.rand_desc(rng, n)
    return keyframe(kl, d), d[2:3].copy(), q


def line_gate_cases(rng):
    """name -> (keyframe, query descriptor, query, found or None = whatever the oracle says).  The query runs from (280, 192) to (320, 208): midpoint
    (300, 200), slope 0.4"""
    out = {}
    u, v, u2, v2, r = 280.0, 192.0, 320.0, 208.0, 10.0
    away = lambda a, b: np.nextafter(f32(a), f32(b))
    xi, xo = bisect(lambda x: line_distance_ok(u, v, u2, v2, r, x, 200.0), 300.0, 315.0)
    assert away(xi, 1e9) == xo
    for name, x, found in (("in", xi, True), ("out", xo, False)):
        out["distance_" + name] = _one_line(x, 200.0, 0.5, 0, _query(u, v, r, 0, 0, u2=u2, v2=v2), rng) + (found,)
    ai, ao = bisect(lambda a: line_slope_ok(u, v, u2, v2, r, a), 0.5, 0.0)           # slope - angle <= 0.01 r: the angle falls until the gate closes
    assert away(ai, -1e9) == ao and 0.29 < ai < 0.31
    for name, a, found in (("in", ai, True), ("out", ao, False)):
        out["slope_" + name] = _one_line(301.0, 200.0, a, 0, _query(u, v, r, 0, 0, u2=u2, v2=v2), rng) + (found,)
    for name, octave, found in (("min-1", 0, False), ("min", 1, True), ("max", 2, True), ("max+1", 3, False)):
        out["level_" + name] = _one_line(301.0, 200.0, 0.5, octave, _query(u, v, r, 1, 2, u2=u2, v2=v2), rng) + (found,)
    # u == u2: the slope is +-inf or, with v == v2 too, NaN
    out["vertical_down"] = _one_line(301.0, 200.0, 0.5, 0, _query(300.0, 190.0, r, 0, 0, u2=300.0, v2=210.0), rng) + (None,)
    out["vertical_up"] = _one_line(301.0, 200.0, 0.5, 0, _query(300.0, 210.0, r, 0, 0, u2=300.0, v2=190.0), rng) + (None,)
    out["degenerate"] = _one_line(301.0, 200.0, 0.5, 0, _query(300.0, 200.0, r, 0, 0, u2=300.0, v2=200.0), rng) + (None,)
    out["not_valid"] = _one_line(301.0, 200.0, 0.5, 0, _query(u, v, r, 0, 0, u2=u2, v2=v2, valid=0), rng) + (False,)
    return out


def gates_as_case(G, kind, chi2):
    """the gate cases of one (kind, chi2) as ONE call: a slot, a descriptor block and a job of one query each -> (case, names)"""
    names = [k for k, g in G.items() if kind == 1 or g[4] == chi2]
    return case(kind, chi2, [G[k][0] for k in names], [G[k][1] for k in names], [job(i, G[k][2], i) for i, k in enumerate(names)]), names


# ---- 3. jobs
def neighbours_case(rng, kind=0, chi2=1, njobs=20, n=90, nq=60):
    """SearchInNeighbors seen from one slot: `njobs` jobs on ONE keyframe that share ONE descriptor block, each with windows of its own (the same map
    points projected with another pose: other centres, radii and levels), then two jobs on a second slot with descriptor blocks of their own"""
    c = mc.fuse_case(rng, kind, n, nq)
    c2 = mc.fuse_case(rng, kind, n - 20, 2 * nq)
    jobs = []
    for k in range(njobs):
        q = c["q"].copy()
        for a in ("u", "v") + (("u2", "v2") if kind == 1 else ()):
            q[a] += rng.normal(0, 1.5, nq).astype(np.float32) if kind == 0 else np.float32(rng.normal(0, 1.5))
        q["radius"] *= rng.choice([1.0, 1.2, 1.44], nq).astype(np.float32); q["valid"] = rng.random(nq) < 0.9
        jobs.append(job(0, q, 0))
    jobs += [job(1, c2["q"][:nq], 1), job(1, c2["q"][nq:], 2)]
    return case(kind, chi2, [keyframe(c["feats"], c["desc"], c["uright"]), keyframe(c2["feats"], c2["desc"], c2["uright"])],
                [c["qdesc"], c2["qdesc"][:nq], c2["qdesc"][nq:]], jobs)


# ---- 4. both forms of the kernel: a pool of full slots
def full_case(rng, kind, chi2, cap, nq=300):
    """a full slot and one of 200 rows, 300 queries each"""
    a = mc.fuse_case(rng, kind, cap, nq); b = mc.fuse_case(rng, kind, 200, nq)
    return case(kind, chi2, [keyframe(a["feats"], a["desc"], a["uright"]), keyframe(b["feats"], b["desc"], b["uright"])], [a["qdesc"], b["qdesc"]],
                [job(0, a["q"], 0), job(1, b["q"], 1), job(0, b["q"], 1), job(1, a["q"][:77], 0, off=100)])


# ---- packing: slots of `cap` rows and jobs of `qcap` rows, junk past every count
def pack_pool(rng, c, cap):
    """[S, cap] buffers of the case's keyframes, rows at or past a keyframe's count random bytes -> dict(feats, desc, uright, n); a keyframe without right
    coordinates is monocular (-1)"""
    S = len(c["pool"])
    P = dict(feats=bc.junk(rng, (S, cap), KP_DTYPE if c["kind"] == 0 else KL_DTYPE), desc=bc.junk(rng, (S, cap, 32), np.uint8), uright=bc.junk(rng, (S, cap), np.float32),
             n=np.zeros(S, np.int32))
    for i, k in enumerate(c["pool"]):
        n = len(k["feats"])
        assert n <= cap, (i, n, cap)
        P["feats"][i, :n] = k["feats"]; P["desc"][i, :n] = k["desc"]; P["n"][i] = n
        P["uright"][i, :n] = k["uright"] if "uright" in k else -1.0
    return P


def block_rows(c):
    """first row of every descriptor block in d_qdesc, and the number of rows in all"""
    sizes = [len(b) for b in c["blocks"]]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)[:-1], int(sum(sizes))


def pack_jobs(rng, c, qcap):
    """-> dict(q [J, qcap] with random bytes past every job's count, qdesc [nqdesc, 32], jobs = rows of sslam_fuse_job, nqdesc)"""
    J = len(c["jobs"])
    first, total = block_rows(c)
    Q = dict(q=bc.junk(rng, (J, qcap), PQ_DTYPE), qdesc=np.concatenate(c["blocks"]) if c["blocks"] else np.zeros((0, 32), np.uint8), jobs=np.zeros(J, JOB_DTYPE), nqdesc=total)
    for i, j in enumerate(c["jobs"]):
        nq = len(j["q"])
        assert nq <= qcap and j["off"] + nq <= len(c["blocks"][j["block"]]), i
        Q["q"][i, :nq] = j["q"]
        Q["jobs"][i] = (j["kf"], nq, first[j["block"]] + j["off"])
    return Q


# ---- 5. one family against the reference itself: map points / lines and a pose (oracle/ref_pin/compare_slices.py is the recipe)
FMP = np.dtype([("wp", "<f4", 3), ("nrm", "<f4", 3), ("minDist", "<f4"), ("maxDist", "<f4"), ("nObs", "<i4"), ("bad", "<i4"), ("inKF", "<i4")])
FQ = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("level", "<i4"), ("valid", "<i4")])
FML = np.dtype([("wp", "<f8", 6), ("nrm", "<f8", 3), ("minDist", "<f4"), ("maxDist", "<f4"), ("nObs", "<i4"), ("bad", "<i4")])
FQL = np.dtype([("u1", "<f4"), ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("radius", "<f4"), ("level", "<i4"), ("valid", "<i4")])
LOG_SF = float(np.log(f32(1.2)))


def _pose():
    ay, ax = 0.07, -0.04
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]); Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Rm = (Ry @ Rx).astype(np.float32); t = np.array([0.3, -0.2, 0.5], np.float32)
    Tcw = np.eye(4, dtype=np.float32); Tcw[:3, :3] = Rm; Tcw[:3, 3] = t
    Ow = (-(Rm.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    cam = np.array([f32(576.0), f32(576.0), f32(316.75), f32(241.5), 40.0], np.float32)
    return Rm.astype(np.float64), t.astype(np.float64), Tcw, Ow, cam


def ref_point_family(rng, n=400):
    """a keyframe of n keypoints (half with a right coordinate), its slots' map points (none / good / bad) and n map points unprojected from its own
    keypoints at random depths: some behind the camera, outside the image, bad or already in the keyframe, some descriptors past TH_LOW"""
    c = mc.fuse_case(rng, 0, n, 1)
    kp = c["feats"]; d = c["desc"]
    ur = np.where(rng.random(n) < 0.5, kp["x"] - rng.uniform(2, 40, n), -1).astype(np.float32)
    R, t, Tcw, Ow, cam = _pose()
    fx, fy, cx, cy = (float(x) for x in cam[:4])
    depth = rng.uniform(2.0, 12.0, n)
    uu = kp["x"].astype(np.float64) + rng.uniform(-2, 2, n); vv = kp["y"].astype(np.float64) + rng.uniform(-2, 2, n)
    pc = np.stack([(uu - cx) / fx * depth, (vv - cy) / fy * depth, depth], 1)
    kind = rng.choice(3, n, p=[0.86, 0.07, 0.07])
    pc[kind == 1, 2] *= -1; pc[kind == 2, 0] += 3 * depth[kind == 2]
    pw = (R.T @ (pc - t).T).T
    mp = np.zeros(n, FMP); mp["wp"] = pw.astype(np.float32)
    po = pw - Ow.astype(np.float64); dist = np.linalg.norm(po, axis=1)
    mp["nrm"] = (po / dist[:, None]).astype(np.float32)
    mp["maxDist"] = (dist * 1.2 ** kp["octave"].astype(np.int64) * rng.uniform(0.9, 1.3, n)).astype(np.float32); mp["minDist"] = (mp["maxDist"] / f32(1.2 ** 7)).astype(np.float32)
    mp["nObs"] = rng.integers(0, 4, n); mp["bad"] = rng.random(n) < 0.04; mp["inKF"] = rng.random(n) < 0.04
    mpd = d.copy()
    for i in np.nonzero(rng.random(n) < 0.5)[0]: mpd[i, rng.integers(0, 32, 6)] ^= rng.integers(1, 256, 6).astype(np.uint8)
    return dict(kp=kp, desc=d, uright=ur, Tcw=Tcw, Ow=Ow, cam=cam, mp=mp, mpd=mpd, state=rng.choice([0, 0, 1, 1, 2], n).astype(np.uint8), sobs=rng.integers(0, 4, n).astype(np.int32))


def ref_line_family(rng, n=200):
    c = mc.fuse_case(rng, 1, n, 1)
    kl = c["feats"]; d = c["desc"]
    R, t, Tcw, Ow, cam = _pose()
    fx, fy, cx, cy = (float(x) for x in cam[:4])
    z = rng.uniform(2.0, 9.0, n); dz = rng.uniform(-0.4, 0.4, n)

    def unproj(x, y, zz):
        pc = np.stack([(x.astype(np.float64) + rng.uniform(-2, 2, n) - cx) / fx * zz, (y.astype(np.float64) + rng.uniform(-2, 2, n) - cy) / fy * zz, zz], 1)
        return (R.T @ (pc - t).T).T
    kind = rng.choice(4, n, p=[0.85, 0.05, 0.05, 0.05])
    zs = z.copy(); zs[kind == 1] *= -1
    sp = unproj(kl["startPointX"], kl["startPointY"], zs); ep = unproj(kl["endPointX"], kl["endPointY"], z + dz)
    sp[kind == 2, 0] += 40.0
    ml = np.zeros(n, FML); ml["wp"] = np.concatenate([sp, ep], 1).astype(np.float32).astype(np.float64)
    mid = 0.5 * (sp + ep); om = mid - Ow.astype(np.float64); dist = np.linalg.norm(om, axis=1)
    ml["nrm"] = (om / dist[:, None]).astype(np.float32).astype(np.float64)
    lvl = rng.choice([0, 0, 0, 1, 1, 2], n); ml["maxDist"] = (dist * 1.2 ** lvl * rng.uniform(0.86, 0.99, n)).astype(np.float32)
    ml["minDist"] = (ml["maxDist"] / f32(1.2 ** 7)).astype(np.float32); ml["bad"] = kind == 3; ml["nObs"] = rng.integers(0, 4, n)
    mld = d.copy()
    for i in np.nonzero(rng.random(n) < 0.4)[0]: mld[i, rng.integers(0, 32, 4)] ^= rng.integers(1, 256, 4).astype(np.uint8)
    return dict(kl=kl, desc=d, Tcw=Tcw, Ow=Ow, cam=cam, ml=ml, mld=mld, state=rng.choice([0, 0, 1, 1, 2], n).astype(np.uint8), sobs=rng.integers(0, 4, n).astype(np.int32))


def replay_fuse(best_idx, best_dist, valid, bad, in_kf, nobs, state, sobs):
    """Fuse's bookkeeping behind the candidate search (src/ORBmatcher.cc:955-975, src/LSDmatcher.cpp:526-544), in query order, as oracle/ref_pin's harness
    records it -> (fusedIdx, action, nFused).  action: 1 new observation, 2 replaced BY the keyframe's point, 3 it replaced the keyframe's point, 4 the
    slot holds a bad point.  The harness notes `the map point the loop is at` whenever a map point of the list answers isBad() -- the slot's holder
    included, once an earlier map point of the list sits there -- and its Replace re-points the slot only where it logs action 3: restated as it is"""
    n = len(best_idx)
    bad = [bool(x) for x in bad]; nobs = [int(x) for x in nobs]
    slot = [None if s == 0 else ["occ", int(o), s == 2] for s, o in zip(state, sobs)]          # holder: [kind / pool index, observations, bad]
    idx = [-1] * n; act = [0] * n; nfused = 0
    for k in range(n):
        if bad[k] or in_kf[k]: continue
        cur = k
        if not (valid[k] == 1 and best_idx[k] >= 0 and best_dist[k] <= TH_LOW): continue
        at = int(best_idx[k]); idx[k] = at
        if not act[k]: act[k] = 4
        h = slot[at]
        if h is None:
            act[k] = 1; slot[at] = [k, nobs[k], False]
        else:
            j = h[0] if h[0] != "occ" else -1
            hbad = bad[j] if j >= 0 else h[2]
            if j >= 0: cur = j
            if not hbad:
                if h[1] > nobs[k]:
                    if cur == k: act[k] = 2
                    elif j >= 0: idx[j] = at; act[j] = 3
                    bad[k] = True
                else:
                    if j >= 0 and cur == j: idx[j] = at; act[j] = 2; bad[j] = True
                    else: act[k] = 3; slot[at] = [k, nobs[k], False]; h[2] = True
        nfused += 1
    return np.array(idx, np.int32), np.array(act, np.int32), nfused
