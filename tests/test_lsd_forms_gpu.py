"""GPU: the middle of the line branch -- the LSD prologue, the sequential core (csrc/lsd_regions.h, lsd_cluster.h) and the NFA stage (csrc/lsd_nfa.h) -- in EVERY launch form,
on the frames of tests/lsd_cases.py (whose reach tests/test_lsd_cases_cpu.py proves from the oracle's trace), against the oracle.  Which form a call took is not inferred from
its size: every run asserts it through sslam_testing_lines_last_forms (include/sslam_testing.h).  The bar is that of tests/test_lines_gpu.py: the segments before the top-N
and every output field bit for bit, `angle` within 1 ulp (libm against ocml atan2), every LBD row equal to the oracle's LBD of the keylines the device produced.

Forms asserted here: the six of the core (cluster + streaming NFA stage, cluster, lone wave, guest, one four-wave workgroup per frame, one six-wave workgroup per frame) and
the NFA stage as stream, 18 launches with 128 / 32, 64 / 16, 64 / 4 and 8 / 1 counting / evaluating waves per frame, and k_nfa_all."""
import numpy as np
import pytest
import torch
import lsd_cases as lc
import oracle_lib
from test_lines_gpu import _ulp_diff
from test_line_tail_gpu import Tail

pytestmark = pytest.mark.gpu

MAX_LINES, CAP = 200, 256
INT_MAX = 0x7FFFFFFF
_ORC = {}


def _oracle(oracle, group, name, max_lines=MAX_LINES):
    """(keylines, LBD rows, line equations, segments before the top-N) of a case, computed once"""
    if (group, name, max_lines) not in _ORC:
        _ORC[group, name, max_lines] = oracle.lines_extract(lc.frame(group, name), max_lines)
    return _ORC[group, name, max_lines]


def _same_lines(oracle, img, kl, ld, fn, want, tag):
    okl, old, ofn = want[:3]
    assert len(kl) == len(okl), (tag, len(kl), len(okl))
    for f in kl.dtype.names:
        if f == "angle": assert _ulp_diff(kl[f], okl[f]).max(initial=0) <= 1, (tag, "KeyLine.angle")
        else: np.testing.assert_array_equal(kl[f], okl[f], err_msg="%s %s" % (tag, f))
    np.testing.assert_array_equal(ld, oracle.lbd_from_keylines(img, kl), err_msg=tag + " LBD")
    np.testing.assert_array_equal(fn.view(np.uint64), ofn.view(np.uint64), err_msg=tag + " line equations")


def _fused_geometry(w, h):
    """lines_build_plan's condition for k_lsd_grad_fused"""
    sw, sh = round(w * 0.8), round(h * 0.8)
    return w % 4 == 0 and sw % 4 == 0 and sh % 4 == 0 and w == 5 * (sw // 4) and h == 5 * (sh // 4) and w >= 20 and h >= 10


def _forms(ex, w, h, **want):
    f = ex.last_forms()
    want = dict(dict(fused_grad=_fused_geometry(w, h), sort_runs=True, lbd_rpi=1), **want)
    assert {k: f[k] for k in want} == want, f
    return f


# knobs -> the forms a SINGLE frame takes under them
SINGLE = {
    "cluster_stream": ({}, dict(core="cluster_stream", nfa="stream", eval_waves=16, count_waves=0)),
    "cluster": ({"SSLAM_NFA_STREAM": "0"}, dict(core="cluster", nfa="launches", eval_waves=32, count_waves=128)),
    "cluster_launches": ({"SSLAM_NFA_STREAM": "0", "SSLAM_NFA_FUSED": "0"}, dict(core="cluster", nfa="launches", eval_waves=32, count_waves=128)),
    "cluster_nfa_all": ({"SSLAM_NFA_STREAM": "0", "SSLAM_NFA_FUSED": "2"}, dict(core="cluster", nfa="all", eval_waves=1, count_waves=1)),
    "lone": ({"SSLAM_LSD_FLAVOUR": "lat"}, dict(core="lone", nfa="launches", eval_waves=32, count_waves=128)),
    "per_frame": ({"SSLAM_LSD_FLAVOUR": "thr"}, dict(core="per_frame", nfa="launches", eval_waves=32, count_waves=128)),
}


def _setenv(monkeypatch, knobs):
    for k in ("SSLAM_NFA_STREAM", "SSLAM_NFA_FUSED", "SSLAM_LSD_FLAVOUR", "SSLAM_LSD_PERSIST", "SSLAM_LSD_CLUSTER"): monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items(): monkeypatch.setenv(k, v)


@pytest.mark.parametrize("form", list(SINGLE))
def test_single_frames_in_every_form(fe, ctx, oracle, form, monkeypatch):
    """every core case and every head size as a single frame, in each form the knobs choose"""
    knobs, want = SINGLE[form]
    _setenv(monkeypatch, knobs)
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        assert ex.last_forms()["core"] is None
        for group, name in [("core", n) for n in lc.CORE] + [("head", wh) for wh in lc.HEADS]:
            img = lc.frame(group, name); tag = "%s %s %s" % (form, group, name)
            o = _oracle(oracle, group, name)
            kl, ld, fn = ex(img)
            _forms(ex, img.shape[1], img.shape[0], grid=0, **want)
            np.testing.assert_array_equal(ex.debug_segments(0), o[3], err_msg=tag + " segments")
            _same_lines(oracle, img, kl, ld, fn, o, tag)
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------------------------- the 8 192-rectangle limit
def _kept(oracle, name):
    """the oracle's segments of a limit frame whose candidate rectangle is among the first MAX_SEG: what the device keeps"""
    t, seg, cand = oracle.lsd_trace(lc.frame("limit", name))
    return t, seg[cand < lc.MAX_SEG]


@pytest.mark.parametrize("form", ["cluster_stream", "cluster", "lone", "per_frame"])
def test_candidate_limit_single_frames(fe, ctx, oracle, form, monkeypatch):
    """8 192 candidates: everything is delivered; 8 193, about 9 500 and about 17 000: SSLAM_ERR_UNSUPPORTED naming the limit, and the segments of the first 8 192 candidates
    stand in the workspace in order (the guards `nSeg < MAX_SEG` of both cores, candFinal = 1 + min(nSeg, MAX_SEG) of the streaming hand-over)"""
    knobs, want = SINGLE[form]
    _setenv(monkeypatch, knobs)
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        img = lc.frame("limit", "squares2048"); o = _oracle(oracle, "limit", "squares2048")
        kl, ld, fn = ex(img)
        _forms(ex, lc.LIMIT_W, lc.LIMIT_H, **want)
        np.testing.assert_array_equal(ex.debug_segments(0), o[3])
        _same_lines(oracle, img, kl, ld, fn, o, form + " squares2048")
        assert ex.batch_status(MAX_LINES) == (0, 0, 0, -1)
        st = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        assert fe.lib().sslam_lines_batch_status_dev(ex.h, MAX_LINES, fe._p(st), None) == 0
        torch.cuda.synchronize(); ctx.synchronize()
        assert st.tolist() == [0, INT_MAX, 0, INT_MAX]
        for name in ("squares2048_bar", "checker16", "checker12"):
            t, kept = _kept(oracle, name)
            with pytest.raises(fe.SslamError) as e:
                ex(lc.frame("limit", name))
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and "8192" in str(e.value), e.value
            _forms(ex, lc.LIMIT_W, lc.LIMIT_H, **want)
            got = ex.debug_segments(0)
            print(form, name, "candidates", t["candidates"], "oracle segments", t["segments"], "kept", len(kept), "device", len(got))
            np.testing.assert_array_equal(got, kept, err_msg="%s %s" % (form, name))
            rc, trunc, unsup, first = ex.batch_status(MAX_LINES)
            assert (rc, unsup, first) == (fe.SSLAM_ERR_UNSUPPORTED, 1, 0)
    finally:
        ex.close()


def _batch(ex, frames, cap=CAP):
    """sslam_lines_extract_batch_dev on frames [n, h, w] (a device tensor) -> keylines [n, cap], LBD rows, line equations, counts on the host"""
    n, h, w = frames.shape
    d_kl = torch.zeros(n * cap * 68, dtype=torch.uint8, device="cuda"); d_ld = torch.zeros(n * cap * 32, dtype=torch.uint8, device="cuda")
    d_fn = torch.zeros(n * cap * 3, dtype=torch.float64, device="cuda"); d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
    ex.extract_batch_dev(frames, w, h, w, w * h, n, d_kl, d_ld, d_fn, d_n, cap)
    torch.cuda.synchronize(); ex.ctx.synchronize()
    return d_kl.cpu().numpy().view(oracle_lib.KL_DTYPE).reshape(n, cap), d_ld.cpu().numpy().reshape(n, cap, 32), d_fn.cpu().numpy().reshape(n, cap, 3), d_n.cpu().numpy()


def test_candidate_limit_in_a_device_batch(fe, ctx, oracle):
    """three frames, the overflowing one in the middle: its rows are the tail of the segments of its first 8 192 candidates, the status names it, its neighbours are exact"""
    imgs = [lc.frame("limit", "squares2048"), lc.frame("limit", "checker16"), lc.strokes(lc.LIMIT_W, lc.LIMIT_H)]
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        kl, ld, fn, cnt = _batch(ex, torch.from_numpy(np.stack(imgs)).cuda())
        _forms(ex, lc.LIMIT_W, lc.LIMIT_H, core="cluster_stream", nfa="stream")
        assert ex.batch_status(CAP) == (fe.SSLAM_ERR_UNSUPPORTED, 0, 1, 1) and b"8192" in fe.lib().sslam_last_error()
        t, kept = _kept(oracle, "checker16")
        np.testing.assert_array_equal(ex.debug_segments(1), kept)
        for i, img in enumerate(imgs):
            want = oracle.lines_tail(img, kept, MAX_LINES, cap=CAP) if i == 1 else oracle.lines_extract(img, MAX_LINES)
            if i != 1: np.testing.assert_array_equal(ex.debug_segments(i), want[3])
            assert cnt[i] == len(want[0]) > 0
            _same_lines(oracle, img, kl[i, :cnt[i]], ld[i, :cnt[i]], fn[i, :cnt[i]], want, "batch frame %d" % i)
    finally:
        ex.close()


def test_candidate_limit_in_frontend_batch(fe, ctx, oracle):
    """sslam_frontend_batch: the frame of 8 192 candidates passes, a chunk with an overflowing frame gives SSLAM_ERR_UNSUPPORTED"""
    orb = fe.OrbExtractor(ctx, 300); ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        img = lc.frame("limit", "squares2048"); o = _oracle(oracle, "limit", "squares2048")
        out = fe.frontend_batch(orb, ex, img[None])
        _same_lines(oracle, img, out[0][2], out[0][3], out[0][4], o, "frontend_batch squares2048")
        with pytest.raises(fe.SslamError) as e:
            fe.frontend_batch(orb, ex, np.stack([img, lc.frame("limit", "checker16"), lc.strokes(lc.LIMIT_W, lc.LIMIT_H)]))
        assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and "8192" in str(e.value), e.value
    finally:
        ex.close(); orb.close()


# ---------------------------------------------------------------------------------------------------------------- the forms chosen by batch size
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


BATCHES = {          # name -> (frames, knobs, core event, calls, forms)
    "six_wave": (lambda: 16 * _cus() + 5, {}, False, 1, dict(core="six_wave", grid=0, nfa="all", eval_waves=1, count_waves=1)),
    "per_frame_1029": (lambda: 1029, {}, False, 1, dict(core="per_frame", grid=0, nfa="launches", eval_waves=1, count_waves=8)),
    "guest_1029": (lambda: 1029, {"SSLAM_LSD_PERSIST": "64"}, True, 2, dict(core="guest", grid=64, nfa="launches", eval_waves=1, count_waves=8)),
    "per_frame_2053": (lambda: 2053, {}, False, 1, dict(core="per_frame", grid=0, nfa="all", eval_waves=1, count_waves=1)),
    "cluster_20": (lambda: 20, {"SSLAM_NFA_STREAM": "0"}, False, 1, dict(core="cluster", grid=0, nfa="launches", eval_waves=16, count_waves=64)),
    "cluster_64": (lambda: 64, {"SSLAM_NFA_STREAM": "0"}, False, 1, dict(core="cluster", grid=0, nfa="launches", eval_waves=4, count_waves=64)),
    "cluster_stream_61": (lambda: 61, {}, False, 1, dict(core="cluster_stream", grid=0, nfa="stream", eval_waves=16, count_waves=0)),
    "lone_67": (lambda: 67, {}, False, 1, dict(core="lone", grid=0, nfa="launches", eval_waves=4, count_waves=64)),
    "lone_130": (lambda: 130, {}, False, 1, dict(core="lone", grid=0, nfa="launches", eval_waves=4, count_waves=8)),
}


@pytest.mark.parametrize("batch", list(BATCHES))
def test_forms_chosen_by_batch_size(fe, ctx, oracle, batch, monkeypatch):
    """the core list tiled (slot s holds case s % U) through the forms only a batch size reaches.  Per case its first, a middle and its last slot against the oracle, every
    slot of the last n % 8 frames (xcd_mix_frame's identity tail, the persistent grid's last claims) as well, and all copies of a case byte-equal up to their counts."""
    nf, knobs, event, calls, want = BATCHES[batch]
    nf = nf()
    _setenv(monkeypatch, knobs)
    names = list(lc.CORE); U = len(names)
    assert nf >= U and (nf % 8 != 0 or batch == "cluster_64")          # (64: the last frame count of the cluster form)
    frames = torch.from_numpy(np.stack([lc.frame("core", n) for n in names])).cuda()
    frames = frames.repeat((nf + U - 1) // U, 1, 1)[:nf].contiguous()
    ex = fe.LineExtractor(ctx, MAX_LINES)
    ev = None
    try:
        if event:
            ev = torch.cuda.Event(); ev.record()          # (recording creates the hipEvent_t)
            ex.set_core_event(ev.cuda_event)
        for _ in range(calls):          # twice in the guest form: the frame counter of the persistent grid is reset per launch
            kl, ld, fn, cnt = _batch(ex, frames)
        _forms(ex, lc.CORE_W, lc.CORE_H, **want)
        assert ex.batch_status(CAP) == (0, 0, 0, -1)
        tail = set(range(nf - nf % 8, nf))
        for i, name in enumerate(names):
            slots = np.arange(i, nf, U)
            o = _oracle(oracle, "core", name)
            assert (cnt[slots] == len(o[0])).all(), (name, cnt[slots], len(o[0]))
            n = len(o[0])
            for s in sorted({int(slots[0]), int(slots[len(slots) // 2]), int(slots[-1])} | (tail & set(slots.tolist()))):
                np.testing.assert_array_equal(ex.debug_segments(s), o[3], err_msg="%s slot %d segments" % (name, s))
                _same_lines(oracle, lc.frame("core", name), kl[s, :n], ld[s, :n], fn[s, :n], o, "%s %s slot %d" % (batch, name, s))
            ref = int(slots[0])
            for arr in (kl, ld, fn):
                assert (arr[slots, :n].view(np.uint8) == arr[ref, :n].view(np.uint8)).all(), (name, "copies differ")
    finally:
        ex.set_core_event(None)
        ex.close()          # (the largest batch holds about 5 MB of workspace per frame)
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- frames too small for the kernels
def test_a_refused_size_leaves_the_handle_as_it_was(fe, ctx, oracle):
    """accepted size -> refused size -> the same accepted size again: the refusal must leave plan, workspace and the last batch's results alone (a plan zeroed by the refused
    size and kept under the old size's name would launch every kernel of the next call with offsets of 0), through the single-frame and the device-batch entry point; the
    status and the segments read after the refusal are the accepted call's, and the tap holds nothing of the refused call"""
    A, B = (320, 240), (641, 480)
    ex = fe.LineExtractor(ctx, MAX_LINES)
    try:
        for size in (A, B, A):
            img = lc.frame("head", size); o = _oracle(oracle, "head", size)
            for small in ((9, 9), (320, 8), (8, 400)):
                kl, ld, fn = ex(img)
                _same_lines(oracle, img, kl, ld, fn, o, "%s before %s" % (size, small))
                with pytest.raises(fe.SslamError) as e:
                    ex(lc.frame("head", small))
                assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and "%dx%d" % small in str(e.value), e.value
                assert ex.last_forms()["core"] is None and ex.last_forms()["nfa"] is None and ex.last_forms()["fused_grad"] is None
                assert ex.batch_status(MAX_LINES) == (0, 0, 0, -1)
                np.testing.assert_array_equal(ex.debug_segments(0), o[3], err_msg="%s segments after the refusal of %s" % (size, small))
                kl, ld, fn = ex(img)
                _forms(ex, size[0], size[1], core="cluster_stream", nfa="stream")
                np.testing.assert_array_equal(ex.debug_segments(0), o[3])
                _same_lines(oracle, img, kl, ld, fn, o, "%s after %s" % (size, small))
        img = lc.frame("head", A); o = _oracle(oracle, "head", A)
        d = torch.from_numpy(np.stack([img] * 3)).cuda(); tiny = torch.from_numpy(np.stack([lc.frame("head", (9, 100))] * 3)).cuda()
        for rep in range(2):
            kl, ld, fn, cnt = _batch(ex, d)
            with pytest.raises(fe.SslamError) as e:
                _batch(ex, tiny)
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and "9x100" in str(e.value), e.value
            assert ex.batch_status(CAP) == (0, 0, 0, -1)
            for i in range(3):
                np.testing.assert_array_equal(ex.debug_segments(i), o[3])
                _same_lines(oracle, img, kl[i, :cnt[i]], ld[i, :cnt[i]], fn[i, :cnt[i]], o, "batch rep %d frame %d" % (rep, i))
        ex.set_seed_order(1)          # the host sorts the seeds: the tap must not report the sort of the call before
        ex(img)
        f = ex.last_forms()
        assert f["sort_runs"] is None and f["core"] == "cluster_stream" and f["fused_grad"] is True, f
        ex.set_seed_order(0)
        kl, ld, fn = ex(img)
        _forms(ex, A[0], A[1], core="cluster_stream", nfa="stream")
        _same_lines(oracle, img, kl, ld, fn, o, "after the seed order")
    finally:
        ex.close()


def test_small_frames_are_refused_before_any_launch(fe, ctx, oracle):
    """a side below 10 pixels (a scaled side below 8: lines_build_plan) is SSLAM_ERR_UNSUPPORTED with the size in the message from every line entry point -- the plan is built
    before the first launch of each; an empty image still gives zero lines"""
    ex = fe.LineExtractor(ctx, 40); orb = fe.OrbExtractor(ctx, 100, nlevels=1)
    try:
        for w, h in lc.TOO_SMALL:
            img = lc.frame("head", (w, h)); what = "%dx%d" % (w, h)
            with pytest.raises(fe.SslamError) as e:
                ex(img)
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and what in str(e.value), (what, e.value)
            d = torch.from_numpy(np.stack([img, img])).cuda()
            with pytest.raises(fe.SslamError) as e:
                _batch(ex, d)
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and what in str(e.value), (what, e.value)
            with Tail(fe, ctx, 40) as t:
                rc, _ = t.raw(img[None], np.zeros((1, 1, 4), np.float32), [0], 40)
                assert rc == fe.SSLAM_ERR_UNSUPPORTED and what.encode() in t.T.sslam_last_error()
        for w, h in ((lc.MIN_SIDE - 1, 64), (64, lc.MIN_SIDE - 1)):          # the host batch: the point branch accepts the size, the line branch refuses it
            img = lc.strokes(w, h)
            with pytest.raises(fe.SslamError) as e:
                fe.frontend_batch(orb, ex, np.stack([img, img]))
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and "%dx%d" % (w, h) in str(e.value), e.value
        assert len(ex(np.zeros((0, 7), np.uint8))[0]) == 0 and len(ex(np.zeros((7, 0), np.uint8))[0]) == 0
        # the other side of the bound: the smallest accepted width and height against the oracle
        for w, h in ((lc.MIN_SIDE, lc.MIN_SIDE), (lc.MIN_SIDE, 40), (40, lc.MIN_SIDE)):
            img = lc.frame("head", (w, h)); o = _oracle(oracle, "head", (w, h), 40)
            kl, ld, fn = ex(img)
            np.testing.assert_array_equal(ex.debug_segments(0), o[3])
            _same_lines(oracle, img, kl, ld, fn, o, "%dx%d" % (w, h))
    finally:
        ex.close(); orb.close()
