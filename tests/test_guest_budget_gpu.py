"""The LDS budgets that let the LSD core's guest form and k_fast_cells share a compute unit (csrc/lsd_regions.h LSD_CORE_LDS, csrc/orb.hip FAST_LIST_CAP).

k_fast_cells keeps at most FAST_LIST_CAP survivors of its pre-test as a list; a cell with more takes the exact fallback in the same kernel.  The CPU tests here
replay the pre-test with numpy and prove which frames reach the fallback (and that the bench's scenes never do); the GPU tests compare such frames with the oracle
stage by stage.  The core's fp64 addends now lie directly behind its region queue, whose overflow slot is their first word: the GPU test runs frames with a region longer
than the queue and with regions that refine() grows again -- proved from the oracle's trace -- through the guest form on a small persistent grid."""
import functools
import numpy as np
import pytest
import lsd_cases as lc
import orb_tail_cases as otc
from synth import synth_frame, noise_frame, warp_prev

FAST_LIST_CAP = 832          # csrc/orb.hip
MIN_TH = 7
BENCH_KINDS = [(60, 40, 2.0), (35, 25, 2.0), (90, 60, 2.0), (60, 40, 3.5), (45, 70, 1.0), (75, 30, 2.5), (60, 40, 2.0), (50, 50, 2.0)]      # bench.py synth_frames


def pretest(img, t=MIN_TH):
    """pass A of k_fast_cells: a 9-arc at threshold t needs a vertical AND a horizontal compass point (distance 3) on its side of the threshold"""
    a = img.astype(np.int16)
    m = np.zeros(a.shape, bool)
    v, n, s, e, w = a[3:-3, 3:-3], a[:-6, 3:-3], a[6:, 3:-3], a[3:-3, 6:], a[3:-3, :-6]
    m[3:-3, 3:-3] = ((np.maximum(n, s) > v + t) & (np.maximum(e, w) > v + t)) | ((np.minimum(n, s) < v - t) & (np.minimum(e, w) < v - t))
    return m


def cell_survivors(oracle, img, nlevels=8):
    """survivors of the pre-test in every FAST cell of every level, in plan order"""
    out = []
    for l, L in enumerate(otc.levels(img.shape[1], img.shape[0], nlevels)):
        if not L["cells"]: continue
        m = pretest(oracle.pyramid_level(img, l, 1.2, nlevels))
        I = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int64)
        I[1:, 1:] = m.cumsum(0).cumsum(1)
        out += [int(I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]) for x0, y0, x1, y1 in L["cells"]]
    return np.array(out)


def patch_frame(k, rows=26):
    """a flat 640 x 480 frame with a checkerboard of 3 x 3 squares (every pixel of it passes the pre-test) over `rows` rows of one level-0 cell and k pixels of the next
    row: rows = 26 gives that cell 809 + k survivors (searched once with the replay above: k = 23 -> 832, k = 24 -> 833), every other cell of every level fewer"""
    x0, y0, x1, y1 = otc.levels(640, 480, 8)[0]["cells"][145]
    assert (x0, y0, x1, y1) == (174, 243, 205, 275)
    yy, xx = np.mgrid[0:480, 0:640]
    pat = np.where(((xx // 3) + (yy // 3)) % 2 == 0, 20, 235).astype(np.uint8)
    m = np.zeros((480, 640), bool)
    m[y0:y0 + rows, x0:x1] = True
    m[y0 + rows, x0:x0 + k] = True
    img = np.full((480, 640), 128, np.uint8)
    img[m] = pat[m]
    return img


FAST_FRAMES = {      # name -> (frame, busiest cell: exact count, or (">", bound) / ("<=", bound))
    "dense": (lambda: noise_frame(7), (">", FAST_LIST_CAP)),
    "plain": (lambda: synth_frame(1234), ("<=", FAST_LIST_CAP)),
    "small": (lambda: synth_frame(4321, w=97, h=83), ("<=", FAST_LIST_CAP)),
    "at_cap": (lambda: patch_frame(23), FAST_LIST_CAP),
    "cap_plus_1": (lambda: patch_frame(24), FAST_LIST_CAP + 1),
}


@functools.lru_cache(maxsize=None)
def fast_frame(name):
    img = FAST_FRAMES[name][0]()
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("name", list(FAST_FRAMES))
def test_fast_frames_reach_what_they_claim(oracle, name):
    busiest = int(cell_survivors(oracle, fast_frame(name)).max())
    want = FAST_FRAMES[name][1]
    print(name, "busiest cell:", busiest, "survivors")
    if isinstance(want, tuple): assert busiest > want[1] if want[0] == ">" else busiest <= want[1], (name, busiest)
    else: assert busiest == want, (name, busiest)


def test_small_frame_has_single_cell_levels():
    assert [len(L["cells"]) for L in otc.levels(97, 83, 8)] == [2, 1, 0, 0, 0, 0, 0, 0]


def test_no_cell_of_the_bench_scenes_exceeds_the_cap(oracle):
    """the condition FAST_LIST_CAP was chosen under: one scene of each of bench.py's eight kinds and its warped predecessor, all eight levels.  (All 64 scenes of the
    default workload and their predecessors: 104 320 cells; the busiest, 825 of 1 258 pixels at level 7, is in the predecessor of scene 30, which stands for its kind here.)"""
    worst = 0
    for i in (0, 1, 2, 3, 4, 5, 30, 7):
        ns, nst, noise = BENCH_KINDS[i % 8]
        f = synth_frame(2000 + i, 640, 480, nshapes=ns, nstrokes=nst, noise=noise)
        worst = max(worst, int(cell_survivors(oracle, f).max()), int(cell_survivors(oracle, warp_prev(f)).max()))
    print("busiest cell of 16 bench frames:", worst)
    assert worst == 825 <= FAST_LIST_CAP


# ---------------------------------------------------------------------------------------------------------------- GPU: k_fast_cells against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAST_FRAMES))
def test_fast_list_cap_against_the_oracle(fe, ctx, oracle, name):
    from test_orb_gpu import _cmp_orb
    assert _cmp_orb(fe, ctx, oracle, fast_frame(name), nfeat=300 if name == "small" else 1000) > 0


@pytest.mark.gpu
def test_fast_list_cap_mixed_batch(fe, ctx, oracle):
    """a cell over the cap and the same cell of the next frame under it, in one launch"""
    import torch
    imgs = [fast_frame("dense"), fast_frame("plain")]
    ex = fe.OrbExtractor(ctx, 1000, 1.2, 8, 20, 7)
    try:
        cap = 1000 + 64 * 8
        d = torch.from_numpy(np.stack(imgs)).cuda()
        d_kp = torch.zeros(2 * cap * 28, dtype=torch.uint8, device="cuda"); d_desc = torch.zeros(2 * cap * 32, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
        ex.extract_batch_dev(d, 640, 480, 640, 640 * 480, 2, d_kp, d_desc, d_n, cap)
        torch.cuda.synchronize(); ctx.synchronize()
        kp = d_kp.cpu().numpy().view(fe.KP_DTYPE).reshape(2, cap); desc = d_desc.cpu().numpy().reshape(2, cap, 32); n = d_n.cpu().numpy()
        for i, img in enumerate(imgs):
            for l in range(8):
                np.testing.assert_array_equal(ex.debug_candidates(i, l), oracle.candidates(img, l, 1000), err_msg="frame %d FAST candidates level %d" % (i, l))
            okp, odesc = oracle.orb_extract(img, 1000)
            assert n[i] == len(okp) > 0
            np.testing.assert_array_equal(kp[i, :n[i]].view(np.uint8), okp.view(np.uint8), err_msg="frame %d keypoints" % i)
            np.testing.assert_array_equal(desc[i, :n[i]], odesc, err_msg="frame %d descriptors" % i)
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------------------------- the core's LDS layout
CORE_FRAMES = {      # tests/lsd_cases.py CORE, 320 x 240 (the smallest size at which a region outgrows the queue): what the oracle's trace must show
    "diagonal": {"reg_max": (">=", lc.QCAP + 1)},                                  # one long straight edge: the queue's overflow slot and the global continuation
    "region769": {"reg769": 1, "reg_max": lc.QCAP + 1},                            # exactly one point beyond the queue
    "spiral8": {"refines": (">=", 10), "regrown_max": (">=", lc.QCAP + 1)},        # refine() grows regions again, beyond the queue too
    "waves": {"refines": (">=", 300), "refine_false": (">=", 1)},                  # many short re-grown regions: the fp64 addends between two growths
}


@pytest.mark.parametrize("name", list(CORE_FRAMES))
def test_core_frames_reach_what_they_claim(oracle, name):
    t = oracle.lsd_trace(lc.frame("core", name))[0]
    for k, want in CORE_FRAMES[name].items():
        assert t[k] >= want[1] if isinstance(want, tuple) else t[k] == want, (name, k, t[k])


@pytest.mark.gpu
def test_core_lds_overlay_in_the_guest_form(fe, ctx, oracle, monkeypatch):
    """1 029 frames on a persistent grid of 64 workgroups, as tests/test_lsd_forms_gpu.py runs the guest form: segments, keylines, LBD bytes and line equations of the
    first, a middle and the last copy of every frame against the oracle, and all copies of a frame equal"""
    import torch
    from test_lsd_forms_gpu import _batch, _forms, _oracle, _same_lines, _setenv, MAX_LINES, CAP
    nf = 1029
    _setenv(monkeypatch, {"SSLAM_LSD_PERSIST": "64"})
    names = list(CORE_FRAMES); U = len(names)
    frames = torch.from_numpy(np.stack([lc.frame("core", n) for n in names])).cuda().repeat((nf + U - 1) // U, 1, 1)[:nf].contiguous()
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        ev = torch.cuda.Event(); ev.record()
        ex.set_core_event(ev.cuda_event)
        kl, ld, fn, cnt = _batch(ex, frames)
        _forms(ex, lc.CORE_W, lc.CORE_H, core="guest", grid=64)
        assert ex.batch_status(CAP) == (0, 0, 0, -1)
        for i, name in enumerate(names):
            slots = np.arange(i, nf, U)
            o = _oracle(oracle, "core", name)
            n = len(o[0])
            assert (cnt[slots] == n).all(), (name, cnt[slots], n)
            for s in (int(slots[0]), int(slots[len(slots) // 2]), int(slots[-1])):
                np.testing.assert_array_equal(ex.debug_segments(s), o[3], err_msg="%s slot %d segments" % (name, s))
                _same_lines(oracle, lc.frame("core", name), kl[s, :n], ld[s, :n], fn[s, :n], o, "guest %s slot %d" % (name, s))
            for arr in (kl, ld, fn):
                assert (arr[slots, :n].view(np.uint8) == arr[int(slots[0]), :n].view(np.uint8)).all(), (name, "copies differ")
    finally:
        ex.set_core_event(None)
        ex.close()
        torch.cuda.empty_cache()
