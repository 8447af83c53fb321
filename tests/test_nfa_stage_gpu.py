"""GPU: the NFA stage (csrc/lsd_nfa.h) on injected rectangles -- sslam_testing_lines_nfa (include/sslam_testing.h) runs the product path's preparation and prologue, writes
the records of tests/nfa_stage_cases.py where the core leaves them and calls the one function that launches the stage.  Three forms per case, each asserted through
sslam_testing_lines_last_forms: the 18 launches and k_nfa_all against the CPU oracle's verdict on every record (tests/sim/nfa_topn_oracle.cpp: the oracle's own rect_nfa /
rect_improve), and k_nfa_topn against the host model of csrc/nfa_topn.h (tests/sim/nfa_topn_sim.cpp) FLAG FOR FLAG: which candidates it validates, which it leaves out,
Misc::topn.  What each case reaches -- slice counts, ties at tau, the border margin, the ranking's capacity, the 768-rectangle chunk -- is proved without a GPU by
tests/test_nfa_stage_cases_cpu.py.  No tolerance anywhere: flags and counts are integers, segments are compared by their bits, untouched rows by the 0xA5 fill.
Last, through the public path (LineExtractor.set_topn_only): the frames of lsd_cases.CORE in calls of eight, `waves` with its nine slices among them, against the oracle to
the bar of tests/test_lsd_forms_gpu.py -- which joins the model's prediction to k_keylines' handling of the flag 2."""
import numpy as np
import pytest
import torch
import lsd_cases as lc
import nfa_stage_cases as nc
from test_lsd_forms_gpu import _same_lines, _batch

pytestmark = pytest.mark.gpu

FORMS = {          # name -> (SSLAM_NFA_FUSED, whether N is handed to the stage, what last_forms must show for a call of fewer than 16 frames)
    "launches": ("0", False, dict(nfa="launches", eval_waves=32, count_waves=128)),
    "all": ("2", False, dict(nfa="all", eval_waves=1, count_waves=1)),
    "topn": ("2", True, dict(nfa="all", eval_waves=1, count_waves=1)),
}


def _segments(v):
    return np.stack([v[k].astype(np.float32) for k in ("x1", "y1", "x2", "y2")], 1) if len(v["x1"]) else np.zeros((0, 4), np.float32)


def _check_frame(tag, flags, segs, topn, n, want_flags, v, rows):
    """one frame of a call: flags [nmax], segs [nmax, 4], against the expected flags [n] and the oracle's verdicts; rows: how many rows of the arrays are specified"""
    FILL = np.uint32(0xA5A5A5A5)
    np.testing.assert_array_equal(flags[:n], want_flags, err_msg=tag + " flags")
    assert (flags[n:rows].view(np.uint32) == FILL).all(), tag + ": a flag at or past ncand was written"
    one = np.flatnonzero(want_flags == 1)
    np.testing.assert_array_equal(segs[one].view(np.uint32), _segments(v)[one].view(np.uint32), err_msg=tag + " segments of the accepted rows")
    other = np.ones(rows, bool); other[one] = False
    assert (segs[:rows][other].view(np.uint32) == FILL).all(), tag + ": the segment of a row that is not accepted was written"
    assert topn == (want_flags == 2).sum(), (tag, topn)


def _run(st, monkeypatch, form, frames, rect_lists, N, want, ver, fused_grad):
    """one call in one form; want: per frame the expected flags under the top-N form (the model's) -- the full forms expect the oracle's verdicts"""
    fused, hand_n, forms = FORMS[form]
    monkeypatch.setenv("SSLAM_NFA_FUSED", fused)
    rects, ncand = nc.pack(rect_lists)
    flags, segs, topn = st(frames, rects, ncand, N if hand_n else 0)
    got = st.last_forms()
    assert {k: got[k] for k in forms} == forms and got["core"] is None and got["fused_grad"] is fused_grad and got["sort_runs"] is True, (form, got)
    for b, r in enumerate(rect_lists):
        n = len(r)
        wf = want[b] if hand_n else (ver[b]["accepted"] == 1).astype(np.int64)
        ranked = hand_n and N < n <= nc.RANK_CAP
        rows = min(rects.shape[1], nc.RANK_BASE) if ranked else rects.shape[1]          # a ranked frame: the rows from NFA_RANK_BASE on are the kernel's copy, unspecified
        _check_frame("%s frame %d" % (form, b), flags[b], segs[b], topn[b], n, wf, ver[b], rows)


@pytest.mark.parametrize("name", nc.NAMES)
def test_every_form_on_every_case(fe, ctx, name, monkeypatch):
    c = nc.case(name); v = nc.verdicts(name); want = nc.expected(name)[0]
    with fe.LineNfaStage(ctx, c.N) as st:
        for form in FORMS:
            _run(st, monkeypatch, form, c.frame[None], [c.rects], c.N, [want], [v], fused_grad=c.frame.shape == (nc.H, nc.W))


def test_mixed_call_of_nine_frames(fe, ctx, monkeypatch):
    """no candidate, one, ranked frames of 41 .. 960, a frame of 1 000 (validated in place) and one of 1 588, whose records lie where a ranked frame's copy would, in ONE call"""
    frames, rects, ver, exp = nc.mixed()
    with fe.LineNfaStage(ctx, nc.MIXED_N) as st:
        for form in FORMS:
            _run(st, monkeypatch, form, frames, rects, nc.MIXED_N, [e[0] for e in exp], ver, fused_grad=True)


def test_workspace_reuse(fe, ctx, monkeypatch):
    """one handle: a ranked frame, then 1 588 candidates validated in place -- over the ranked copy and its NfaState --, then the ranked frame again; nothing of a call
    may show in the next"""
    frames, rects, ver, exp = nc.mixed()
    big = (frames[4][None], [rects[4]], [(ver[4]["accepted"] == 1).astype(np.int64)], [ver[4]])
    c = nc.case("waves200")
    ranked = (c.frame[None], [c.rects], [nc.expected("waves200")[0]], [nc.verdicts("waves200")])
    assert len(rects[4]) > nc.RANK_BASE + len(c.rects) - 200          # the in-place records cover most of the ranked copy
    with fe.LineNfaStage(ctx, c.N) as st:
        for k, (f, r, want, v) in enumerate((ranked, big, ranked, big, ranked)):
            _run(st, monkeypatch, "topn", f, r, c.N, want, v, fused_grad=True)


def test_records_outside_the_value_range_are_refused(fe, ctx):
    """before any launch: SSLAM_ERR_INVALID, and the handle has chosen no form"""
    c = nc.case("one_slice")
    sw, sh = round(nc.W * 0.8), round(nc.H * 0.8)
    good = c.rects[:4].copy()
    bad = []
    for col, val in ((0, np.nan), (7, np.inf), (0, -good[0, 4] - 1.0), (2, sw + good[0, 4] + 1.0), (1, sh + 50.0), (5, -0.5), (6, float(sh)), (4, 0.0), (4, max(sw, sh) + 1.0),
                     (8, good[0, 8] + (0.01 if good[0, 8] >= 0 else -0.01)), (10, good[0, 10] / 2), (11, good[0, 11] / 2)):
        r = good.copy(); r[0, col] = val; bad.append(r)
    with fe.LineNfaStage(ctx, 10) as st:
        for r in bad:
            rc, _ = st.raw(c.frame[None], r[None], [4], 10)
            assert rc == fe.SSLAM_ERR_INVALID and st.last_forms()["nfa"] is None, r[0]
        assert st.raw(c.frame[None], good[None], [5], 10)[0] == fe.SSLAM_ERR_INVALID          # more candidates than rows
        flags, segs, topn = st(c.frame[None], good[None], [4], 0)          # ... and the list they were made from passes
        np.testing.assert_array_equal(flags[0], (nc.verdicts("one_slice")["accepted"][:4] == 1).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the public path
@pytest.mark.parametrize("max_lines", [200, 5])
def test_topn_only_on_the_core_frames(fe, ctx, oracle, max_lines, monkeypatch):
    """LineExtractor.set_topn_only(1) behind the core (SSLAM_NFA_STREAM=0) as k_nfa_topn (SSLAM_NFA_FUSED=2): lsd_cases.CORE in calls of eight.  At 200 `waves` takes nine
    slices and leaves 290 candidates out; at 5 every frame of more than five candidates is ranked."""
    monkeypatch.setenv("SSLAM_NFA_STREAM", "0"); monkeypatch.setenv("SSLAM_NFA_FUSED", "2")
    names = list(lc.CORE)
    names += names[:-len(names) % 8]          # the last call is filled up with the first frames
    ex = fe.LineExtractor(ctx, max_lines)
    try:
        assert ex.set_topn_only(1) == 0
        left_out = 0
        for k in range(0, len(names), 8):
            call = names[k:k + 8]
            kl, ld, fn, cnt = _batch(ex, torch.from_numpy(np.stack([lc.frame("core", n) for n in call])).cuda(), cap=max_lines)
            f = ex.last_forms()
            assert f["nfa"] == "all" and f["fused_grad"] is True, f
            for i, name in enumerate(call):
                img = lc.frame("core", name); tag = "%s at %d" % (name, max_lines)
                want = oracle.lines_extract(img, max_lines)
                assert cnt[i] == len(want[0]), (tag, cnt[i], len(want[0]))
                _same_lines(oracle, img, kl[i, :cnt[i]], ld[i, :cnt[i]], fn[i, :cnt[i]], want, tag)
                tap = ex.debug_segments(i)
                rows = {r.tobytes(): j for j, r in enumerate(want[3])}
                idx = [rows.get(r.tobytes(), -1) for r in tap]
                assert min(idx, default=0) >= 0 and idx == sorted(set(idx)), tag + ": the tap is not a subsequence of the oracle's segments"
                left_out += len(want[3]) - len(tap)
                if name == "waves" and max_lines == 200:          # the model's multi-slice prediction: the validated accepted candidates, in emission order
                    flags = nc.expected("waves200")[0]
                    np.testing.assert_array_equal(tap, _segments(nc.verdicts("waves200"))[flags == 1])
                    assert len(tap) < len(want[3])
        assert left_out > 0
    finally:
        ex.close()
