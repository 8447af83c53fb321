"""GPU: the sequential LSD core (csrc/lsd_regions.h, csrc/lsd_cluster.h) on its own output.  sslam_testing_lines_core (include/sslam_testing.h) runs lines_prepare,
k_zero_misc, lines_prologue() and lines_core() -- the product path's functions, the launch form included -- and sslam_testing_lines_core_frame copies back what the core left
of a frame: the candidate count, every candidate's RectD record and the T plane, whose sign bits are the used map.  The other side is the oracle's core record
(oracle/lsd_oracle.cpp LsdCore, filled by the detector's own loop; tests/test_lsd_core_cases_cpu.py holds it against oracle_rects and proves what each frame reaches).

The bar is equality, with no tolerance: the core adds its fp64 sums pixel by pixel in the reference's order.  Per frame
  * Misc::nCand is the oracle's count (the first 8 192 of an over-limit frame, with SSLAM_ERR_UNSUPPORTED naming the limit),
  * all twelve doubles of every candidate, the ones the NFA stage rejects included, are bit-equal (uint64 views),
  * rows at or past nCand still hold the 0xA5 fill,
  * the used map -- T defined and its sign bit set -- is the oracle's final map, pixel for pixel,
  * |T| is the plane sslam_testing_lines_prologue returns for the frame, and T is -1024 exactly where that plane is: the core may set the sign bit and nothing else.
Which path a helper wave took -- taken, refused, regrown by the main wave -- depends on timing and is not asserted; the result must not depend on it.  Every run asserts its
launch form through sslam_testing_lines_last_forms.

What the first run of this module found: counts, used maps, the fill and |T| equal in every form, and the six forms equal to each other -- but `dx` or `dy` one ulp off the
oracle in 8 of spiral8's 119 candidates, 49 of waves' 716, 20 .. 26 of each star frame's (about one candidate in fifteen), with end points and width off by a few ulps behind
them.  region2rect took cos(theta) and sin(theta) from the device library, which is faithful but not correctly rounded; the oracle's libm nearly always is.  Both sides now
round correctly (csrc/sincos_cr.h, oracle/lsd_oracle.cpp cr_sincos; tests/test_sincos_cr_cpu.py), and a failure here reports the first differing candidate
with its seed, point count, reach, the fields and the distance in ulps."""
import numpy as np
import pytest
import torch
import lsd_cases as lc
import lsd_core_cases as cc
from test_lsd_core_cases_cpu import core as _oracle_core
from test_lsd_forms_gpu import BATCHES, _setenv, _fused_geometry

pytestmark = pytest.mark.gpu

PAD = 16          # rows asked for beyond the oracle's count: they must come back as the fill
NOTDEF_BITS = np.float32(-1024.0).view(np.uint32)
CL_KNOBS = ("SSLAM_CL_WGS", "SSLAM_CL_WINDOW", "SSLAM_CL_SMAP", "SSLAM_CL_NO_FEEDER")
_PRO = {}


def _prologue_t(fe, ctx, group, name):
    """the T plane the prologue tap leaves for a case (uint32 view), computed once"""
    if (group, name) not in _PRO:
        with fe.LinePrologue(ctx) as p:
            _PRO[group, name] = p(cc.frame(group, name)[None])[0]["T"].view(np.uint32).copy()
    return _PRO[group, name]


def _env(monkeypatch, knobs):
    for k in CL_KNOBS: monkeypatch.delenv(k, raising=False)
    _setenv(monkeypatch, knobs)


def _forms(tap, w, h, core, grid=0):
    """the tap's record: the core's and the prologue's words; behind the core nothing ran, except the consumers of the streaming form"""
    f = tap.last_forms()
    want = dict(core=core, grid=grid, fused_grad=_fused_geometry(w, h), sort_runs=True, lbd_rpi=-1)
    want.update(dict(nfa="stream", eval_waves=16, count_waves=0) if core == "cluster_stream" else dict(nfa=None, eval_waves=-1, count_waves=-1))
    assert f == want, (f, want)


FIELDS = ("x1", "y1", "x2", "y2", "width", "x", "y", "theta", "dx", "dy", "prec", "p")          # a RectD record


def _ulps(a, b):
    """distance in representable doubles between two arrays of finite doubles given as uint64 bit patterns"""
    key = lambda u: np.where(u >> 63, -(u & 0x7FFFFFFFFFFFFFFF).astype(np.int64), (u & 0x7FFFFFFFFFFFFFFF).astype(np.int64))
    return np.abs(key(a) - key(b))


def _compare(fe, ctx, oracle, tap, slot, group, name, tag):
    """every check of the module's docstring for one frame of the last run step -> the list of what differs (empty: equal).  A difference is located: the first differing
    candidate with its seed, point count and reach, the fields and by how many ulps; the first differing pixel."""
    o = _oracle_core(oracle, group, name)
    bad = []
    n = min(len(o["rects"]), lc.MAX_SEG)
    nmax = min(n + PAD, lc.MAX_SEG)
    rc, got = tap.frame_raw(slot, nmax)
    if len(o["rects"]) > lc.MAX_SEG: assert rc == fe.SSLAM_ERR_UNSUPPORTED and b"8192" in tap.T.sslam_last_error(), (tag, rc)
    else: assert rc == 0, (tag, rc, tap.T.sslam_last_error())
    assert (got["sw"], got["sh"]) == (o["sw"], o["sh"]), tag
    if got["ncand"] != n: bad.append("%s: nCand %d, oracle %d" % (tag, got["ncand"], n))
    m = min(n, max(got["ncand"], 0))
    r, want = got["rects"].view(np.uint64), o["rects"][:n].view(np.uint64)
    diff = r[:m] != want[:m]
    if diff.any():
        rows = np.flatnonzero(diff.any(1)); i = int(rows[0]); q = o["cand"][i]
        per = {FIELDS[f]: (int(diff[:, f].sum()), int(_ulps(r[:m, f], want[:m, f]).max())) for f in np.flatnonzero(diff.any(0))}
        bad.append("%s: %d of %d candidates differ, field -> (candidates, largest distance in ulps) %s; the first is candidate %d, seed (%d, %d), %d points, reach %d, regrew %d, "
                   "reduced %d: fields %s device %r oracle %r" % (tag, len(rows), m, per, i, q["x"], q["y"], q["points"], q["reach"], q["regrew"], q["reduced"],
                                                                   [FIELDS[f] for f in np.flatnonzero(diff[i])], got["rects"][i].tolist(), o["rects"][i].tolist()))
    if not (r[max(got["ncand"], 0):] == fe.LineCore.FILL).all(): bad.append("%s: rows at or past nCand were written" % tag)
    T = got["T"].view(np.uint32); P = _prologue_t(fe, ctx, group, name)
    assert T.shape == P.shape == o["used"].shape
    undef = P == NOTDEF_BITS
    if not ((T == NOTDEF_BITS) == undef).all(): bad.append("%s: T is -1024 elsewhere than the prologue left it (%d pixels)" % (tag, int(((T == NOTDEF_BITS) != undef).sum())))
    if not ((T & 0x7FFFFFFF)[~undef] == P[~undef]).all(): bad.append("%s: the core changed more than the sign bit of T" % tag)
    used = ~undef & ((T >> 31) != 0)
    if not np.array_equal(used, o["used"]):
        ys, xs = np.nonzero(used != o["used"])
        bad.append("%s: the used map differs in %d pixels, the first at (x %d, y %d): device %d, oracle %d" % (tag, len(ys), xs[0], ys[0], used[ys[0], xs[0]], o["used"][ys[0], xs[0]]))
    return bad


def _report(bad):
    for b in bad: print(b)
    assert not bad, "%d differences from the oracle, the first: %s" % (len(bad), bad[0])


SINGLE = {          # knobs -> the form a single frame takes under them
    "cluster": ({"SSLAM_NFA_STREAM": "0"}, "cluster"),
    "cluster_stream": ({}, "cluster_stream"),
    "lone": ({"SSLAM_LSD_FLAVOUR": "lat"}, "lone"),
    "per_frame": ({"SSLAM_LSD_FLAVOUR": "thr"}, "per_frame"),
}


def _run_single(fe, ctx, oracle, tap, cases, core, tag):
    bad = []
    for group, name in cases:
        img = cc.frame(group, name); h, w = img.shape
        d = torch.from_numpy(np.array(img)).cuda()
        torch.cuda.synchronize()
        tap.run(d, w, h, w, w * h, 1)
        _forms(tap, w, h, core)
        bad += _compare(fe, ctx, oracle, tap, 0, group, name, "%s %s %s" % (tag, group, name))
    _report(bad)


@pytest.mark.parametrize("form", list(SINGLE))
def test_single_frames_in_every_form(fe, ctx, oracle, form, monkeypatch):
    """the 17 core frames and 12 head sizes of tests/lsd_cases.py and the reach, list-length and contention frames of tests/lsd_core_cases.py, one frame per call; the frames
    of the bitmap boundary in the cluster form (TorusFrame | TorusGlobal) and as lone waves"""
    knobs, core = SINGLE[form]
    _env(monkeypatch, knobs)
    cases = cc.existing() + cc.new(("reach", "stg", "contention") + (("bitmap",) if form in ("cluster", "lone") else ()))
    with fe.LineCore(ctx) as tap:
        assert tap.frame_raw(0, 4)[0] == fe.SSLAM_ERR_INVALID          # (no run step yet)
        _run_single(fe, ctx, oracle, tap, cases, core, form)


@pytest.mark.parametrize("form", list(SINGLE))
def test_candidate_limit_single_frames(fe, ctx, oracle, form, monkeypatch):
    """8 192 candidates: all of them; 8 193, about 9 500 and about 17 000: the first 8 192, bit-equal, and SSLAM_ERR_UNSUPPORTED naming the limit from the copy-back"""
    knobs, core = SINGLE[form]
    _env(monkeypatch, knobs)
    with fe.LineCore(ctx) as tap:
        _run_single(fe, ctx, oracle, tap, [("limit", n) for n in lc.LIMIT], core, form)


@pytest.mark.parametrize("knobs", [{"SSLAM_CL_WINDOW": "-1"}, {"SSLAM_CL_WINDOW": "6"}, {"SSLAM_CL_WGS": "2"}, {"SSLAM_CL_WGS": "16", "SSLAM_CL_WINDOW": "1600"},
                                   {"SSLAM_CL_SMAP": "-1"}, {"SSLAM_CL_SMAP": "2", "SSLAM_CL_WGS": "3"}, {"SSLAM_CL_NO_FEEDER": "1"}],
                         ids=lambda k: "-".join("%s=%s" % (a[9:], b) for a, b in k.items()))
def test_cluster_configurations(fe, ctx, oracle, knobs, monkeypatch):
    """the knobs of tests/test_lines_gpu.py's test_lsd_cluster_configurations -- no helpers at all, helpers barely or far ahead, three or forty-five of them, no or a coarser
    shared map, no feeder wave -- on the frames where the protocol's thresholds lie: the schedule changes completely, no record and no pixel may"""
    _env(monkeypatch, {"SSLAM_NFA_STREAM": "0"})
    for k, v in knobs.items(): monkeypatch.setenv(k, v)
    with fe.LineCore(ctx) as tap:
        _run_single(fe, ctx, oracle, tap, cc.new(("contention", "reach", "stg")) + [("core", "waves")], "cluster", str(knobs))


CORE_BATCHES = ("six_wave", "guest_1029", "per_frame_1029", "cluster_20", "cluster_64", "cluster_stream_61", "lone_67")


@pytest.mark.parametrize("batch", CORE_BATCHES)
def test_forms_chosen_by_batch_size(fe, ctx, oracle, batch, monkeypatch):
    """the 320 x 240 frames tiled (slot s holds case s % U) through the forms only a batch size reaches, with the frame counts and knobs of tests/test_lsd_forms_gpu.py's test
    of the same name.  Per case its first, a middle and its last slot against the oracle, and every slot of the last n % 8 frames."""
    nf, knobs, event, calls, want = BATCHES[batch]
    nf = nf()
    _env(monkeypatch, knobs)
    cases = cc.small_320x240()[:nf]; U = len(cases)          # (cluster_20 holds the first 20 of the 25 cases)
    assert U >= 20 and (nf % 8 != 0 or batch == "cluster_64")
    frames = torch.from_numpy(np.stack([cc.frame(g, n) for g, n in cases])).cuda()
    frames = frames.repeat((nf + U - 1) // U, 1, 1)[:nf].contiguous()
    torch.cuda.synchronize()
    tap = fe.LineCore(ctx)
    ev = None
    try:
        if event:
            ev = torch.cuda.Event(); ev.record()          # (recording creates the hipEvent_t)
            tap.set_core_event(ev.cuda_event)
        for _ in range(calls):          # twice in the guest form: the frame counter of the persistent grid is reset per launch
            tap.run(frames, lc.CORE_W, lc.CORE_H, lc.CORE_W, lc.CORE_W * lc.CORE_H, nf)
        _forms(tap, lc.CORE_W, lc.CORE_H, want["core"], want["grid"])
        tail = set(range(nf - nf % 8, nf)); bad = []
        for i, (group, name) in enumerate(cases):
            slots = np.arange(i, nf, U)
            for s in sorted({int(slots[0]), int(slots[len(slots) // 2]), int(slots[-1])} | (tail & set(slots.tolist()))):
                bad += _compare(fe, ctx, oracle, tap, s, group, name, "%s %s %s slot %d" % (batch, group, name, s))
        _report(bad)
    finally:
        tap.set_core_event(None)
        tap.close()          # (the largest batch holds about 5 MB of workspace per frame)
        del frames
        torch.cuda.empty_cache()
