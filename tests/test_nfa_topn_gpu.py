"""The NFA stage's top-N form (csrc/nfa_topn.h, k_nfa_topn; sslam_lines_set_topn_only) against the default and against the CPU oracle.  Calls of eight frames
reach the one-wave-per-frame form through SSLAM_NFA_FUSED=2 (behind the core: SSLAM_NFA_STREAM=0), on the smallest geometry of the fused gradient path (320 x 240) and
on an odd size off it (333 x 251): seven dense scenes, on which a small max_lines cuts, and one sparse scene on which it does not.  With the contract on, key lines, LBD
rows, line equations and counts are byte for byte those of the default, and the tap holds FEWER segments than the oracle's on the dense frames (the test is not vacuous)
and the same on the sparse one.  The reference sorts and cuts iff a frame holds MORE than max_lines lines: max_lines equal to a frame's accepted count (emission order,
no new class_id) and one below it (sorted) are both run, on a frame the oracle picks."""
import functools
import numpy as np
import pytest
import torch
from synth import synth_frame
from test_lines_gpu import _ulp_diff

pytestmark = pytest.mark.gpu

NF = 8
GEOMETRIES = {"fused_320x240": (320, 240), "odd_333x251": (333, 251)}


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    dense = [synth_frame(7100 + i, w=w, h=h, nshapes=30 + 4 * i, nstrokes=20 + 3 * i, noise=2.0) for i in range(NF - 1)]
    sparse = synth_frame(7198, w=w, h=h, nshapes=1, nstrokes=0, noise=0.0)
    return tuple(dense + [sparse])


@functools.lru_cache(maxsize=None)
def _oracle(w, h, max_lines):
    import oracle_lib
    orc = oracle_lib.Oracle()
    return tuple(orc.lines_extract(f, max_lines) for f in _frames(w, h))


def _run(fe, ctx, w, h, max_lines, on):
    """one call of NF frames -> (key lines [NF, cap], LBD rows, line equations, counts, the tap per frame, the forms the call took)"""
    frames = _frames(w, h)
    ex = fe.LineExtractor(ctx, max_lines)
    try:
        assert ex.set_topn_only(on) == 0
        dev = torch.from_numpy(np.stack(frames)).cuda()
        cap = max_lines
        rec = fe.KL_DTYPE.itemsize
        d_kl = torch.zeros(NF * cap * rec, dtype=torch.uint8, device="cuda"); d_ld = torch.zeros(NF * cap * 32, dtype=torch.uint8, device="cuda")
        d_fn = torch.zeros(NF * cap * 3, dtype=torch.float64, device="cuda"); d_n = torch.zeros(NF, dtype=torch.int32, device="cuda")
        ex.extract_batch_dev(dev, w, h, w, w * h, NF, d_kl, d_ld, d_fn, d_n, cap)
        torch.cuda.synchronize()
        forms = ex.last_forms()
        taps = [ex.debug_segments(i) for i in range(NF)]
        n = d_n.cpu().numpy()
        kl = d_kl.cpu().numpy().view(fe.KL_DTYPE).reshape(NF, cap); ld = d_ld.cpu().numpy().reshape(NF, cap, 32); fn = d_fn.cpu().numpy().reshape(NF, cap, 3)
        assert ex.set_topn_only(0) == int(bool(on))
        return kl, ld, fn, n, taps, forms
    finally:
        ex.close()


def _knobs(monkeypatch):
    monkeypatch.setenv("SSLAM_NFA_STREAM", "0")
    monkeypatch.setenv("SSLAM_NFA_FUSED", "2")


def _check_against_oracle(orc_lib, frames, want, kl, ld, fn, n):
    for i, (okl, old, ofn, oraw) in enumerate(want):
        assert n[i] == len(okl), (i, n[i], len(okl))
        k = kl[i, :n[i]]
        for f in k.dtype.names:
            if f == "angle": assert _ulp_diff(k[f], okl[f]).max(initial=0) <= 1, "KeyLine.angle of frame %d" % i
            else: np.testing.assert_array_equal(k[f], okl[f], err_msg="%s of frame %d" % (f, i))
        np.testing.assert_array_equal(ld[i, :n[i]], orc_lib.lbd_from_keylines(frames[i], k), err_msg="LBD of frame %d" % i)
        np.testing.assert_array_equal(fn[i, :n[i]], ofn, err_msg="line equations of frame %d" % i)


@pytest.mark.parametrize("max_lines", [10, 40])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_topn_only_equals_default_and_oracle(fe, ctx, oracle, geometry, max_lines, monkeypatch):
    _knobs(monkeypatch)
    w, h = GEOMETRIES[geometry]
    want = _oracle(w, h, max_lines)
    off = _run(fe, ctx, w, h, max_lines, False)
    on = _run(fe, ctx, w, h, max_lines, True)
    for r in (off, on): assert r[5]["nfa"] == "all" and r[5]["fused_grad"] == (geometry.startswith("fused")), r[5]
    for a, b, name in zip(off[:4], on[:4], ("key lines", "LBD rows", "line equations", "counts")):
        for i in range(NF):
            m = off[3][i]
            x, y = (a[i, :m], b[i, :m]) if name != "counts" else (a[i], b[i])
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), "%s of frame %d differ between topn_only on and off" % (name, i)
    _check_against_oracle(oracle, _frames(w, h), want, *on[:4])
    _check_against_oracle(oracle, _frames(w, h), want, *off[:4])
    for i, (okl, old, ofn, oraw) in enumerate(want):
        np.testing.assert_array_equal(off[4][i], oraw, err_msg="the default's tap of frame %d" % i)      # the default path's tap is unchanged: every segment
        tap = on[4][i]
        # the validated accepted segments, in emission order: a subsequence of the oracle's
        rows = {r.tobytes(): k for k, r in enumerate(oraw)}
        idx = [rows[r.tobytes()] for r in tap]
        assert idx == sorted(idx) and len(set(idx)) == len(idx), "the tap of frame %d is not a subsequence of the oracle's segments" % i
        if i < NF - 1:
            assert len(oraw) > 2 * max_lines and max_lines < len(tap) < len(oraw), (i, len(tap), len(oraw))
        else:
            assert 0 < len(oraw) <= 10 and len(tap) == len(oraw), (i, len(tap), len(oraw))


@pytest.mark.parametrize("below", [0, 1])
def test_max_lines_at_the_accepted_count(fe, ctx, oracle, below, monkeypatch):
    """max_lines == a frame's accepted count: the reference neither sorts nor renumbers, and nothing may be left out; one below: it sorts and cuts one line.  The frame: the
    dense 320 x 240 scene with the fewest segments, which has more candidates than segments (rejected rectangles), so that the ranking runs in both cases."""
    _knobs(monkeypatch)
    w, h = GEOMETRIES["fused_320x240"]
    import nfa_topn_sim as sim
    full = _oracle(w, h, 8192)
    pick = min(range(NF - 1), key=lambda i: len(full[i][3]))
    nseg = len(full[pick][3])
    assert len(sim.oracle_frame(_frames(w, h)[pick])["r0"]) > nseg > 20
    max_lines = nseg - below
    want = _oracle(w, h, max_lines)
    off = _run(fe, ctx, w, h, max_lines, False)
    on = _run(fe, ctx, w, h, max_lines, True)
    assert on[3][pick] == max_lines == off[3][pick]
    for a, b in zip(off[:4], on[:4]):
        assert np.ascontiguousarray(a[pick]).tobytes() == np.ascontiguousarray(b[pick]).tobytes()
    _check_against_oracle(oracle, _frames(w, h), want, *on[:4])
    cid = on[0][pick]["class_id"]
    resp = on[0][pick]["response"]
    if below: assert (np.diff(resp) <= 0).all() and np.array_equal(cid, np.arange(max_lines))
    else: assert len(on[4][pick]) == nseg and (np.diff(resp) > 0).any()
