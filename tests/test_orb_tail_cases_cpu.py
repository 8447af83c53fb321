"""The preconditions of tests/test_orb_tail_gpu.py, from the generators (tests/orb_tail_cases.py) and the oracle's trace alone: a candidate list that does not reach the
loop end, the sorted length, the tie, the node size or the staging path it is named after would pass on the device without testing anything."""
import numpy as np
import pytest
import oracle_lib as ol
import orb_tail_cases as oc


@pytest.fixture(scope="module")
def cases(oracle):
    return oc.octree_cases(oracle)


@pytest.fixture(scope="module")
def traces(oracle, cases):
    """name -> (selection, trace) of the quadtree alone; the whole tail (pyramid, orientation, descriptors) gives the same trace"""
    return {k: oracle.distribute_octtree(c["cand"], c["W"], c["H"], c["N"]) for k, c in cases.items()}


def test_geometry_matches_the_issue():
    L = oc.levels(160, 120, 1)[0]
    assert (L["W"], L["H"], L["nIni"], L["cand_cap"]) == (128, 88, 1, 2501) and len(oc.lattice(128, 88)) == 2501
    L = oc.levels(199, 151, 1)[0]
    assert (L["W"], L["H"], L["nIni"], L["cand_cap"]) == (167, 119, 1, 4617)
    L = oc.levels(400, 100, 1)[0]
    assert (L["W"], L["H"], L["nIni"]) == (368, 68, 5) and abs(L["hX"] - 73.6) < 1e-5
    assert tuple(int(np.float32(L["hX"]) * np.float32(r)) for r in range(1, 5)) == oc.STRIP_EDGES
    L = oc.levels(192, 144, 3)[0]
    assert L["pitch"] == L["w"] == 192
    assert oc.levels(199, 151, 3)[0]["pitch"] == 256 and all(L["pitch"] > L["w"] for L in oc.levels(199, 151, 3)) and all(L["pitch"] > L["w"] for L in oc.levels(192, 144, 3)[1:])
    assert oc.levels(4111, 100, 1)[0]["nIni"] == 60 and oc.levels(4111, 64, 1)[0]["nIni"] > 64 and oc.levels(64, 4111, 1)[0]["nIni"] == 0
    for name, (w, h, _) in oc.IMAGES.items():
        assert oc.image(name).shape == (h, w)


def test_level_geometry_equals_the_oracles_pyramid(oracle):
    for w, h in ((192, 144), (199, 151), (160, 120)):
        img = np.zeros((h, w), np.uint8)
        for l, L in enumerate(oc.levels(w, h, 3)):
            assert oracle.pyramid_level(img, l, nlevels=3).shape == (L["h"], L["w"])


def test_every_list_is_valid(cases):
    """inside the level, scores 1..255, Chebyshev distance >= 2, no more than the level's cells hold (octree_cases asserts it while building; here for the rest)"""
    assert len(cases) >= 35
    for c in (oc.batch_case(), oc.border_case("noise192"), oc.border_case("noise199"), oc.moments_case(), oc.cap_case()):
        h, w = c["images"].shape[1:]
        Ls = oc.levels(w, h, c["nlevels"])
        assert len(c["cands"]) == len(c["images"])
        for per in c["cands"]:
            for cand, L in zip(per, Ls):
                assert oc.check_spacing(cand, L["W"], L["H"]) and len(cand) <= L["cand_cap"]
    b = oc.big_lds_case()
    assert len(b["cand"]) >= 4000 and b["N"] == 2000


def test_loop_ends(cases, traces):
    for k in (0, 1, 2):
        t = traces["end_break_N+%d" % k][1]
        assert t["end"] == ol.END_SECOND_BREAK and t["final_nodes"] == cases["end_break_N+%d" % k]["N"] + k
    t = traces["end_round_without_break"][1]
    assert t["rounds2"] >= 2 and t["rounds2_no_break"] >= 1
    t = traces["end_first_phase_N"][1]
    assert t["end"] == ol.END_FIRST_N and t["rounds2"] == 0 and t["final_nodes"] >= cases["end_first_phase_N"]["N"]
    sel, t = traces["end_first_phase_no_growth"]
    n = len(cases["end_first_phase_no_growth"]["cand"])
    assert t["end"] == ol.END_FIRST_NO_GROWTH and t["rounds2"] == 0 and t["final_nodes"] == len(sel) == n < cases["end_first_phase_no_growth"]["N"]          # all singletons
    for name, N in (("end_N0", 0), ("end_N1", 1), ("end_N1_one_candidate", 1)):
        assert cases[name]["N"] == N and traces[name][1]["end"] == ol.END_FIRST_N and traces[name][1]["final_nodes"] >= 1
    assert traces["end_N0"][1]["final_nodes"] == 4          # N = 0 still divides the root once


def test_sorted_lengths(traces):
    seen = set()
    for name, (sel, t) in traces.items():
        assert t["n_sorted"] == len(t["sorted"]), name          # nothing cut from the record
        seen |= set(t["sorted"])
    assert set(oc.SORT_TARGETS) <= seen and max(seen) > 256, sorted(seen)
    for K in oc.SORT_TARGETS:
        assert K in traces["sort_%d" % K][1]["sorted"]
    assert max(traces["sort_300"][1]["sorted"]) == 300


def test_ties(cases, traces):
    for order in ("raster", "shuffled"):
        t = traces["tie_sizes_" + order][1]
        assert t["max_all_equal"] == 100 and 100 in t["sorted"] and t["end"] == ol.END_SECOND_BREAK and t["rounds2_no_break"] == t["rounds2"] - 1          # the break falls inside the list of equal sizes
        c = cases["tie_all_responses_" + order]
        assert len(np.unique(c["cand"][:, 2])) == 1 and traces["tie_all_responses_" + order][1]["tie_nodes"] >= 20
        assert traces["tie_max_twice_" + order][1]["tie_nodes"] >= 20
    for name in ("tie_sizes", "tie_all_responses", "tie_max_twice"):
        a, b = cases[name + "_raster"], cases[name + "_shuffled"]
        assert a["N"] == b["N"] and not np.array_equal(a["cand"], b["cand"])
        assert np.array_equal(a["cand"][np.lexsort(a["cand"].T)], b["cand"][np.lexsort(b["cand"].T)])          # the same candidates
        assert np.array_equal(a["cand"], oc.raster(a["cand"]))
    # with equal responses the survivor of a node is its first candidate in arrival order: the two orders keep different candidates
    assert not np.array_equal(traces["tie_all_responses_raster"][0], traces["tie_all_responses_shuffled"][0])


def test_node_sizes(cases, traces):
    for n in oc.NODE_SIZES:
        t = traces["node_%d" % n][1]
        assert t["div%d" % n] == 1 and t["max_divided"] == n and len(cases["node_%d" % n]["cand"]) == n
    assert traces["node_64"][1]["div_large"] == 0 and traces["node_65"][1]["div_large"] == 1          # either side of the one-pass form
    t = traces["node_chunked_empty_class"][1]
    assert t["div_large_empty_class"] >= 1 and t["max_divided"] > 2 * oc.SPLIT_ONE_PASS
    for name, n in (("node_dense_lattice", 2501), ("node_dense_lattice_199", 4617)):
        c = cases[name]
        assert len(c["cand"]) == n == oc.levels(*oc.IMAGES[c["img"]][:2], 1)[0]["cand_cap"] and traces[name][1]["div_large"] >= 20
        xy = c["cand"][:, :2]
        assert (xy % 2 == 1).all() and len(np.unique(xy, axis=0)) == n          # every second pixel of every second row


def test_root_strips(cases, traces):
    L = oc.levels(400, 100, 1)[0]
    hX = np.float32(L["hX"])
    strip = lambda c: (c[:, 0].astype(np.float32) / hX).astype(np.int32)
    for name in ("roots_strip_edges", "roots_strip_edges_only"):
        c = cases[name]["cand"]
        xs = set(c[:, 0].tolist())
        for e in oc.STRIP_EDGES: assert {e - 2, e, e + 2} <= xs
        assert {0, 2, L["W"] - 2} <= xs
        # the quirk: x == (int)(hX * r) lies in strip r - 1 by the division although that strip's box ends there
        for r, e in enumerate(oc.STRIP_EDGES, 1):
            assert int(np.float32(e) / hX) == r - 1 and int(np.float32(e + 2) / hX) == r and int(hX * np.float32(r)) == e
    cnt = lambda name: np.bincount(strip(cases[name]["cand"]), minlength=5).tolist()
    assert cnt("roots_empty_first_middle_last") == [0, 1, 0, 100, 0]
    assert cnt("roots_one_and_many") == [90, 1, 70, 0, 130]
    assert cnt("roots_N_below_strips") == [20] * 5 and traces["roots_N_below_strips"][1]["end"] == ol.END_FIRST_N
    assert traces["roots_one_and_many"][1]["max_divided"] == 130


def test_batch_case_lists_differ():
    b = oc.batch_case()
    assert b["images"].shape == (73, 120, 160) and b["nlevels"] == 3
    n = np.array([[len(c) for c in per] for per in b["cands"]])
    assert (n == 0).sum() >= 10 and (n[0] == 0).all() and any(r[0] > 0 and r[1] == 0 and r[2] > 0 for r in n)          # an empty level between full ones
    keys = {(l, c.tobytes()) for per in b["cands"] for l, c in enumerate(per) if len(c)}
    assert len(keys) == (n > 0).sum()
    assert len({im.tobytes() for im in b["images"]}) == 73


@pytest.mark.parametrize("img", ["noise192", "noise199"])
def test_border_case_reaches_both_paths_and_every_shift(oracle, img):
    c = oc.border_case(img)
    w, h = oc.IMAGES[img][:2]
    Ls = oc.levels(w, h, 3)
    q = oc.quotas(oracle, c["nfeatures"], 3)
    for l, L in enumerate(Ls):
        allc = np.concatenate([per[l] for per in c["cands"]])
        want = {(x, y) for x in range(L["W"]) for y in range(L["H"]) if x < oc.BORDER or x >= L["W"] - oc.BORDER or y < oc.BORDER or y >= L["H"] - oc.BORDER}
        assert {(int(x), int(y)) for x, y in allc[:, :2]} == want and len(allc) == len(want)          # every border position once
        paths = {(oc.interior(x + oc.MINB, y + oc.MINB, L), oc.delta(x + oc.MINB)) for x, y in allc[:, :2]}
        assert paths == {(p, d) for p in (True, False) for d in (-2, -1, 0, 1)}, (l, paths)
        for per in c["cands"]:
            assert len(per[l]) <= q[l] and len(np.unique(per[l][:, 2])) == min(len(per[l]), 255)
        only = [(x, y) for x, y in allc[:, :2] if oc.fails_only_pitch(x + oc.MINB, y + oc.MINB, L)]
        assert (len(only) > 0) == (img == "noise192" and l == 0), (l, only[:4])
    # every candidate survives: one frame's whole tail on the CPU
    kp, desc, lc, n, tr = oracle.orb_tail(c["images"][5], c["cands"][5], c["nfeatures"], nlevels=3)
    assert lc.tolist() == [len(x) for x in c["cands"][5]] and all(t["end"] in (ol.END_FIRST_NO_GROWTH, ol.END_SECOND_ROUND) for t in tr)          # no growth: all singletons


def test_moments_case_angles(oracle):
    c = oc.moments_case()
    assert len(c["images"]) == len(oc.RAMPS) == 9
    want = {"const": (0, 0), "+x": (0, 1), "-x": (0, -1), "+y": (1, 0), "-y": (-1, 0), "+x+y": (1, 1), "-x-y": (-1, -1), "+x-y": (-1, 1), "-x+y": (1, -1)}
    exact = {"const": 0.0, "+x": 0.0, "-x": 180.0, "+y": 90.0, "-y": 270.0}
    for name, img, per in zip(oc.RAMPS, c["images"], c["cands"]):
        kp, desc, lc, n, tr = oracle.orb_tail(img, per, c["nfeatures"], nlevels=1)
        assert n == len(per[0]) == 60
        m01, m10 = want[name]
        a = np.float32(oracle.fast_atan2(m01, m10))
        assert (kp["angle"] == a).all(), (name, np.unique(kp["angle"]), a)
        if name in exact: assert a == np.float32(exact[name])
        else: assert abs(float(a) - (np.degrees(np.arctan2(m01, m10)) % 360)) < 0.05
        assert {1.0, 255.0} <= set(kp["response"].tolist())


def test_cap_case_survives_whole(oracle):
    c = oc.cap_case()
    kp, desc, lc, n, tr = oracle.orb_tail(c["images"][0], c["cands"][0], c["nfeatures"], nlevels=3)
    assert lc.tolist() == [40, 50, 60] and n == 150
    kp1, desc1, lc1, n1, _ = oracle.orb_tail(c["images"][0], c["cands"][0], c["nfeatures"], nlevels=3, cap=55)
    assert n1 == 150 and len(kp1) == 55 and kp1.tobytes() == kp[:55].tobytes() and desc1.tobytes() == desc[:55].tobytes()


def test_big_lds_case_passes_64k(oracle):
    b = oc.big_lds_case()
    L = oc.levels(199, 151, 1)[0]
    lds, nc = oc.octree_lds_bytes([b["N"]], [L])
    assert lds == 16 * 2048 + 4 * (len(L["cells"]) + 1) + 20 * 2007 > 65536 and nc == 2007
    sel, t = oracle.distribute_octtree(b["cand"], b["W"], b["H"], b["N"])
    assert 2000 <= len(sel) <= 2002 and t["rounds2"] >= 1


def test_orb_extract_and_the_tail_share_one_body(oracle):
    """the oracle's own candidates fed back through orc_orb_tail give orc_orb_extract's bytes"""
    from synth import synth_frame
    img = synth_frame(31, w=320, h=240)
    kp, desc = oracle.orb_extract(img, 300, nlevels=4)
    cands = [oracle.candidates(img, l, 300, nlevels=4) for l in range(4)]
    kp2, desc2, lc, n, tr = oracle.orb_tail(img, cands, 300, nlevels=4)
    assert n == len(kp) > 100 and kp2.tobytes() == kp.tobytes() and desc2.tobytes() == desc.tobytes() and lc.sum() == n


def test_reference_distribute_octtree_equals_oracle(oracle, cases, traces, tmp_path):
    """the REFERENCE's own DistributeOctTree (oracle/ref_pin/ref_octree_stub.cpp: src/ORBextractor.cc compiled unmodified, allocator with increasing addresses) on every
    octree list of this module and on the largest-LDS list: the oracle keeps the same keypoints in the same order"""
    import os, subprocess
    import pkg
    exe = os.path.join(pkg.ROOT, "oracle", "_ref", "ref_octree_stub")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_octree_stub is not built (it needs the reference tree: `make -C oracle/ref_pin ref-build`)")
    todo = [(c, traces[k][0]) for k, c in cases.items()]
    b = oc.big_lds_case()
    todo.append((b, oracle.distribute_octtree(b["cand"], b["W"], b["H"], b["N"])[0]))
    for c, want in todo:
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        np.concatenate([np.array([c["W"], c["H"], c["N"], len(c["cand"])], np.int32), c["cand"].ravel()]).tofile(fin)
        subprocess.run([exe, fin, fout], check=True, timeout=60)
        out = np.fromfile(fout, np.int32)
        got = out[1:].reshape(-1, 3)
        assert out[0] == len(got) == len(want) and np.array_equal(got, want), (c["name"], len(got), len(want))
