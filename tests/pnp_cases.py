"""The cases of the PnP RANSAC tests (tests/test_pnp_cases_cpu.py, tests/test_pnp_gpu.py): small scenes, N <= 130 and max_iterations <= 130, in the case format of
tests/pnp_sim.py.

A scene is a set of GROUPS of correspondences: group g holds sizes[g] world points and their exact projections under the group's own pose.  A four-point set taken from
one group recovers that group's pose, so its count is the group's size: the counts of a case, and with them every branch of iterate's control flow, follow from which
group each of the caller's sets comes from -- where the five Gauss-Newton steps converge, which _verified establishes per set and per model from that model's own rep_errors.  Any other four-point set
gives a pose that depends on the basis of MtM's null space: such sets appear where the library draws them (DRAWN), and those cases are compared with
tests/pnp_ref.py on what does not depend on the hypotheses' poses, and bit for bit between the host model and the GPU.  BASIS_DEPENDENT: compared with pnp_ref.py on
integers only."""
import functools
import numpy as np

K = np.array([520.0, 515.0, 320.0, 240.0], np.float32)
SIGMA2 = (1.2 ** (2 * np.arange(8))).astype(np.float32)


def _pose(r, ang):
    ax = r.randn(3); ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx, r.uniform(-0.5, 0.5, 3)


def scene(seed, sizes, junk=0, noise=0.0, planar=False):
    """-> (case fields, groups: list of index arrays into the correspondence list, poses).  Frame rows: the groups' points shuffled among `junk` rows of every filtered
    kind (unassigned, assigned >= nkf, an invalid keyframe row, an octave below 0 and one at nlevels)"""
    r = np.random.RandomState(seed)
    n = int(sum(sizes))
    nf, nkf = n + 5 * junk, n + junk + 3
    poses = [_pose(r, 0.3 + 0.25 * g) for g in range(len(sizes))]
    Xw = np.zeros((nkf, 3), np.float32); uv = r.uniform(0, 600, (nf, 2)); assigned = np.full(nf, -1, np.int32); octv = r.randint(0, 8, nf).astype(np.int32)
    valid = np.ones(nkf, np.uint8)
    frows = r.permutation(nf); krows = r.permutation(nkf)
    gid = np.full(nf, -1, np.int64)
    at = 0
    for g, (sz, (R, t)) in enumerate(zip(sizes, poses)):
        Xc = np.c_[r.uniform(-2, 2, sz), r.uniform(-1.5, 1.5, sz), r.uniform(3, 8, sz)]
        W = ((Xc - t) @ R).astype(np.float32)
        if planar:
            W[:, 2] = np.float32(W[:, 2].mean())      # one world plane, exactly: PW0's third column is zero and so are the last control-point scale and a column of CC
        Xc = W.astype(np.float64) @ R.T + t
        p = np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]] + r.randn(sz, 2) * noise
        fr, kr = frows[at:at + sz], krows[at:at + sz]
        Xw[kr] = W; uv[fr] = p; assigned[fr] = kr; gid[fr] = g
        at += sz
    spare_f, spare_k = frows[n:], krows[n:]
    Xw[spare_k] = r.uniform(-3, 3, (len(spare_k), 3))
    for q in range(junk):
        f5 = spare_f[5 * q:5 * q + 5]
        assigned[f5[0]] = -1
        assigned[f5[1]] = nkf + q
        assigned[f5[2]] = spare_k[q]; valid[spare_k[q]] = 0
        assigned[f5[3]] = spare_k[junk]; octv[f5[3]] = -1
        assigned[f5[4]] = spare_k[junk + 1]; octv[f5[4]] = len(SIGMA2)
    keep = np.where(gid >= 0)[0]      # ascending frame row: the correspondence list
    groups = [np.where(gid[keep] == g)[0] for g in range(len(sizes))]
    return dict(oct=octv, pt=uv.astype(np.float32), K=K, xw=Xw, valid=valid, assigned=assigned, sigma2=SIGMA2), groups, poses


CANDIDATES = 24      # four-point sets tried per group


CONVERGED = 1e-4     # px (the float32 pixel coordinates are rounded to about 3e-5): the smallest rep_error of a four-point set one of whose three solves arrived


def _verified(c, groups, r, exact):
    """Five Gauss-Newton steps do not bring every four-point set to a pose, and where they do not the outcome depends on the basis of the null space, in the host model
    and in tests/pnp_ref.py alike.  So the sets of a case are chosen by their conditioning: CANDIDATES random sets per group go through the host model
    (the plain build, one call that cannot return: min_inliers = N) and through pnp_ref.py, and a set is kept when in EACH model, judged by that model alone, the
    smallest of the three rep_errors -- the one compute_pose chooses by -- is below CONVERGED: four points have an exact solution, so a converged solve reprojects them
    exactly.  Whether the two models then count the same rows is not looked at here; tests/test_pnp_cases_cpu.py asserts it.  -> per group the kept sets"""
    import pnp_ref, pnp_sim
    n = int(sum(len(g) for g in groups))
    keep = [[] for _ in groups]
    for _ in range(8):      # rounds, until every group has a set
        cand = np.array([r.choice(g, 4, replace=False) for g in groups for _ in range(CANDIDATES)], np.int32).reshape(-1, 4)
        probe = dict(c, probability=0.99, min_inliers=n, max_iterations=1, epsilon=0.01, th2=c["th2"], calls=[len(cand)], sets=cand, seed=0, pair=0)
        got = pnp_sim.run_plain([probe])[0]["calls"][0]
        idx, X, uv, me = pnp_ref.correspondences(probe)
        for i, s in enumerate(cand):
            rep = got["trace"][i, :3]
            if not (np.isfinite(rep).all() and rep.min() < CONVERGED):
                continue
            rep = np.array(pnp_ref.compute_pose(X[s], uv[s], c["K"])[2]["rep"])
            if np.isfinite(rep).all() and rep.min() < CONVERGED:
                keep[i // CANDIDATES].append(s)
        if all(keep):
            break
    return keep


def _sets(r, groups, plan, good):
    """plan: per iteration a group number (the group's verified sets in turn), or a list of four indices taken as they are"""
    out, used = [], [0] * len(groups)
    for g in plan:
        if isinstance(g, (list, tuple)):
            out.append(list(g))
        elif good is None:
            out.append(list(r.choice(groups[g], 4, replace=False)))
        else:
            assert good[g], "no four-point set of group %d converges in both models" % g
            out.append(list(good[g][used[g] % len(good[g])])); used[g] += 1
    return np.array(out, np.int32).reshape(-1, 4)


def _case(seed, sizes, plan, calls, min_inliers, max_iterations, epsilon=0.05, probability=0.999999, junk=0, th2=5.991, planar=False, noise=0.0, pair=0):
    c, groups, poses = scene(seed, sizes, junk, noise, planar)
    r = np.random.RandomState(seed + 1000)
    c["th2"] = th2
    good = None if plan is None or planar else _verified(c, groups, r, noise == 0.0)
    c.update(probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, epsilon=epsilon, th2=th2, calls=list(calls), seed=seed, pair=pair,
             sets=None if plan is None else _sets(r, groups, plan, good))
    c["_groups"], c["_poses"] = groups, poses
    return c


def _gates(c):
    """Two correspondences of group 0 outside the first set get levels of their own (6 and 7; th2 is 1, so a level's sigma2 IS its gate): the gate of row A is its
    error2 under the first hypothesis exactly -- the strict < of :329 leaves it out -- and the gate of row B the next float above its error2, which lets it in.  The
    hypothesis does not depend on the gates, so one run of the host model gives the pose and tests/pnp_ref.py's restatement of :317-327 the two errors"""
    import pnp_ref, pnp_sim
    idx, X, uv, _ = pnp_ref.correspondences(c)
    A, B = [int(i) for i in c["_groups"][0] if i not in set(c["sets"][0].tolist())][:2]
    octv = c["oct"].copy()
    octv[octv > 5] -= 2
    octv[idx[A]], octv[idx[B]] = 6, 7
    c["oct"] = octv
    pose = pnp_sim.run_plain([public(c)])[0]["calls"][0]["poses"][0]
    e2 = pnp_ref.errors2(pose[:9].reshape(3, 3), pose[9:], c["K"], X, uv)
    sigma2 = SIGMA2.copy()
    sigma2[6] = e2[A]
    sigma2[7] = np.nextafter(e2[B], np.float32(np.inf))
    c["sigma2"] = sigma2
    c["_gate_rows"] = (A, B, float(e2[A]), float(e2[B]))
    return c


@functools.lru_cache(maxsize=None)
def build():
    """name -> case.  Group 0 is the large one (a success of Refine), group 1 has exactly min_inliers points where a failing Refine is wanted, group 2 is below min_inliers"""
    C = {}
    S = [30, 15, 12]      # with min_inliers 15: counts 30 (refines to 30 > 15), 15 (qualifies, Refine gives 15: fails), 12 (does not qualify)
    C["refine_at_0"] = _case(1, S, [0] + [2] * 9, [5], 15, 10)
    C["refine_at_63"] = _case(2, S, [2] * 63 + [0] + [2] * 66, [5], 15, 130)
    C["refine_at_64"] = _case(3, S, [2] * 64 + [0] + [2] * 65, [5], 15, 130)
    C["refine_fails_then_equal_then_best"] = _case(4, S, [2, 1, 1, 2, 1, 0, 2, 2], [5, 5], 15, 8, junk=2)
    C["resume_after_refined_return"] = _case(5, S, [2, 0, 2, 1, 2, 0, 1, 2, 2, 2, 2, 2], [5, 5, 5, 5], 15, 12)
    C["exhaustion_with_best"] = _case(6, S, [2, 1, 2, 1, 2, 2], [5, 5, 5], 15, 6)
    C["exhaustion_without_best"] = _case(7, S, [2] * 7, [5, 5], 15, 7)
    C["max_its_below_5"] = _case(8, S, [2, 2, 2, 1, 2, 2, 0], [5, 5], 15, 3)
    for m in (63, 64, 65, 129):
        C["max_its_%d" % m] = _case(10 + m, S, [2] * (m - 1) + [1] + [2] * 3, [5, 5], 15, m)
    C["past_nsets_and_out_of_range"] = _case(20, S, [2, [0, 1, 2, 57], [-1, 0, 1, 2], 1], [5, 5], 15, 9)
    C["n_0"] = _case(21, [0], None, [5, 5], 10, 20)
    C["n_3"] = _case(22, [3], None, [5], 4, 20, junk=1)
    C["n_4_is_min"] = _case(23, [4], None, [5, 5], 4, 20)
    C["n_min_minus_1"] = _case(24, [14], None, [5], 15, 20, junk=1)
    C["n_is_min_drawn"] = _case(25, [15], None, [5, 5, 3], 15, 20, junk=3)
    for n in (63, 64, 65):
        C["n_%d_drawn" % n] = _case(30 + n, [n], None, [5, 5], n, 20, junk=2)
    C["epsilon_above_min"] = _case(40, [40, 20], [1, 1, 0], [5], 10, 50, epsilon=0.5)       # int(60 * 0.5) = 30 > 10: group 1 (20) no longer qualifies
    C["epsilon_at_min"] = _case(41, [40, 20], [1, 0], [5], 30, 50, epsilon=0.5)
    C["epsilon_below_min"] = _case(42, [40, 20], [1, 0], [5], 20, 50, epsilon=0.25)      # int(15) < 20: group 1 qualifies with exactly min_inliers, Refine fails
    C["gate_neighbours"] = _gates(_case(43, S, [0, 2, 2], [5], 15, 3, th2=1.0))
    C["coplanar"] = _case(50, [30, 15], [1, 0, 1, 1, 0, 1], [5], 15, 6, planar=True)
    c = _case(51, S, [2, 1, 2, 0], [5], 15, 6)
    g = c["_groups"]
    c["sets"][0] = [g[0][0], g[0][0], g[0][1], g[0][2]]      # one point twice
    c["sets"][2] = [g[0][3], g[0][3], g[0][3], g[0][3]]      # one point four times
    C["repeated_point"] = c
    C["mixed_drawn"] = _case(52, [40, 25, 20], None, [5, 5, 5], 20, 130, epsilon=0.3, probability=0.99, junk=2, noise=0.3)
    return C


BASIS_DEPENDENT = ("coplanar", "repeated_point")
DRAWN = ("n_4_is_min", "n_is_min_drawn", "n_63_drawn", "n_64_drawn", "n_65_drawn", "mixed_drawn")      # the library draws: sets that need not converge


def public(c):
    """the case without the generator's own fields"""
    return {k: v for k, v in c.items() if not k.startswith("_")}
