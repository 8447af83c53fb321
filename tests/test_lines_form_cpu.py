"""CPU: the form plan of the line extractor (csrc/lines_form.h: LinesKnobs / lines_knobs_from, lines_forms) on both sides of every boundary.  The header holds no HIP, so
tests/sim/lines_form_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program; nothing is loaded into Python
(tests/plan_dump.py).  Every expectation is the literal that DESIGN.md section 5's table "Which call takes which form" or the code before lines_form.h existed gives
(lines_core_form, lines_guest_form, lines_core_cluster, lines_tail, lines_describe, launch_nfa_stage, lines_knobs); the rule is not restated here."""
import pytest
import plan_dump

FIELDS = ("core", "grid", "guest_fits", "sort_runs", "cl_wgs", "cl_window", "cl_smap", "big_frame", "nfa", "eval_waves", "count_waves", "topn", "stream_waves", "spin_ticks",
          "fork_blur_sobel", "lbd_rpi")
KNOBS = ("lone", "cluster", "persist", "cl_wgs", "cl_window", "cl_smap", "nfa_stream_waves", "nfa_spin_ticks", "nfa_fused")


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker(src=plan_dump.LINES_FORM)


def _row(tokens, names):
    assert len(tokens) == len(names), tokens
    return {k: (t if k in ("core", "nfa") else int(t)) for k, t in zip(names, tokens)}


def _forms(ask, n, cus=256, event=0, topn=0, size=(640, 480, 512, 384), **env):
    line = "forms %d %d %d %d %d %d %d %d" % (size + (n, cus, event, topn)) + "".join(" %s=%s" % kv for kv in env.items())
    return _row(ask([line])[0], FIELDS)


def _knobs(ask, **env):
    return _row(ask(["knobs" + "".join(" %s=%s" % kv for kv in env.items())])[0], KNOBS)


def _is(got, **want):
    assert {k: got[k] for k in want} == want, got


def test_constants(ask):
    """frames per cluster call, the cluster form's largest scaled image, the main wave's LDS bitmap, CL_MAXWG, CL_SUB, the tile-sorted runs' side, k_lbd<true>'s side, the
    waves of the streaming launch behind the core (csrc/lines.hip pins the device code's own constants to them with static_asserts)"""
    assert ask(["consts"]) == [["64", "2048", "1024", "1024", "512", "16", "4", "2048", "16384", "16"]]


# DESIGN.md section 5, "Which call takes which form", at 640 x 480: frames -> (core, NFA stage, evaluating waves, counting waves, k_blur_sobel forked beside the stage).
# 16 C and 16 C + 1 are 4 096 and 4 097 at C = 256; at C = 8 they are 128 and 129, below the 1 024 frames from which the workgroup forms start at all, and every call from
# 1 024 on is past 16 C.
STREAM = ("cluster_stream", "stream", 16, 0, 0)
TABLE = {
    256: {1: STREAM, 15: STREAM, 16: STREAM, 63: STREAM, 64: STREAM,
          65: ("lone", "launches", 4, 64, 0), 127: ("lone", "launches", 4, 64, 0), 128: ("lone", "launches", 4, 8, 0), 1023: ("lone", "launches", 4, 8, 0),
          1024: ("per_frame", "launches", 1, 8, 1), 2047: ("per_frame", "launches", 1, 8, 1), 2048: ("per_frame", "all", 1, 1, 1), 4096: ("per_frame", "all", 1, 1, 1),
          4097: ("six_wave", "all", 1, 1, 1)},
    8: {1: STREAM, 15: STREAM, 16: STREAM, 63: STREAM, 64: STREAM,
        65: ("lone", "launches", 4, 64, 0), 127: ("lone", "launches", 4, 64, 0), 128: ("lone", "launches", 4, 8, 0), 129: ("lone", "launches", 4, 8, 0),
        1023: ("lone", "launches", 4, 8, 0), 1024: ("six_wave", "launches", 1, 8, 1), 2047: ("six_wave", "launches", 1, 8, 1), 2048: ("six_wave", "all", 1, 1, 1)},
}
# the rows "1 .. 64 under SSLAM_NFA_STREAM=0"; every other row is unchanged by the knob
STREAM0 = {1: ("cluster", "launches", 32, 128, 0), 15: ("cluster", "launches", 32, 128, 0), 16: ("cluster", "launches", 16, 64, 0), 63: ("cluster", "launches", 16, 64, 0),
           64: ("cluster", "launches", 4, 64, 0)}
# the row "from 1 024, with a core event and at least two rounds of the grid": C = 8 has a grid of 20 C = 160 and two rounds of it from 320 frames; C = 256 needs 8 192 frames
# (test_guest_form) and keeps the form it had -- but a caller with a core event never has k_blur_sobel forked
GUEST8 = {1024: ("guest", 160), 2047: ("guest", 160), 2048: ("guest", 160)}


@pytest.mark.parametrize("cus", [256, 8])
@pytest.mark.parametrize("stream0", [False, True])
@pytest.mark.parametrize("event", [0, 1])
@pytest.mark.parametrize("topn", [0, 40])
def test_design_table(ask, cus, stream0, event, topn):
    env = {"SSLAM_NFA_STREAM": "0"} if stream0 else {}
    for n, want in TABLE[cus].items():
        core, nfa, ev, cnt, fork = STREAM0[n] if stream0 and n in STREAM0 else want
        grid_word = 0
        if event:
            fork = 0
            if cus == 8 and n in GUEST8: core, grid_word = GUEST8[n]
        if topn and nfa == "all": nfa = "topn"
        f = _forms(ask, n, cus, event, topn, **env)
        _is(f, core=core, nfa=nfa, eval_waves=ev, count_waves=cnt, fork_blur_sobel=fork, topn=topn if nfa == "topn" else 0, sort_runs=1, lbd_rpi=1)
        assert (f["grid"] if f["core"] == "guest" else 0) == grid_word, (n, f)
        _is(f, stream_waves=16 if nfa == "stream" else 0, spin_ticks=5000000 if nfa == "stream" else 0)
        assert f["guest_fits"] == (1 if core == "guest" else 0), (n, f)


def test_guest_form(ask):
    """two rounds of the grid: 20 C where the batch holds them, 16 C otherwise, SSLAM_LSD_PERSIST in multiples of 8 from 8; only with a core event, never below 1 024 frames"""
    _is(_forms(ask, 8191, event=1), core="six_wave", guest_fits=0, grid=4096)
    _is(_forms(ask, 8192, event=1), core="guest", guest_fits=1, grid=4096)
    _is(_forms(ask, 10239, event=1), core="guest", guest_fits=1, grid=4096)
    _is(_forms(ask, 10240, event=1), core="guest", guest_fits=1, grid=5120)
    _is(_forms(ask, 8192, event=0), core="six_wave", guest_fits=0, grid=4096)
    _is(_forms(ask, 1023, event=1), core="lone", guest_fits=0)
    _is(_forms(ask, 1023, cus=8, event=1), core="lone", guest_fits=0)
    _is(_forms(ask, 1023, event=1, SSLAM_LSD_PERSIST=64), core="lone", guest_fits=0, grid=64)
    _is(_forms(ask, 1024, event=1, SSLAM_LSD_PERSIST=64), core="guest", guest_fits=1, grid=64)
    _is(_forms(ask, 1024, event=0, SSLAM_LSD_PERSIST=64), core="per_frame", guest_fits=0, grid=64)
    _is(_forms(ask, 1024, event=1, SSLAM_LSD_PERSIST=71), core="guest", guest_fits=1, grid=64)
    _is(_forms(ask, 1024, event=1, SSLAM_LSD_PERSIST=7), core="per_frame", guest_fits=0, grid=4096)
    _is(_forms(ask, 1024, event=1, SSLAM_LSD_PERSIST=520), core="per_frame", guest_fits=0, grid=520)       # 1 040 frames are two rounds of it
    _is(_forms(ask, 1040, event=1, SSLAM_LSD_PERSIST=520), core="guest", guest_fits=1, grid=520)
    # sslam_lines_core_guest_form answers for the room, whatever the flavour makes of the core
    _is(_forms(ask, 8192, event=1, SSLAM_LSD_FLAVOUR="lat"), core="lone", guest_fits=1, grid=4096)
    _is(_forms(ask, 8192, event=1, SSLAM_LSD_FLAVOUR="thr"), core="guest", guest_fits=1, grid=4096)


def test_scaled_sizes(ask):
    """the cluster form up to 2 048 x 1 024 scaled pixels, its bitmap in LDS up to 1 024 x 512, tile-sorted runs up to 2 048 a side, k_lbd<true> up to 16 384 source pixels a side"""
    size = lambda sw, sh: (640, 480, sw, sh)
    _is(_forms(ask, 1, size=size(2048, 1024)), core="cluster_stream", big_frame=1)
    _is(_forms(ask, 1, size=size(2049, 1024)), core="lone", big_frame=0, nfa="launches", eval_waves=32, count_waves=128)
    _is(_forms(ask, 1, size=size(2048, 1025)), core="lone", big_frame=0)
    _is(_forms(ask, 1, size=size(2048, 1025), SSLAM_NFA_STREAM=0), core="lone")
    _is(_forms(ask, 1, size=size(1024, 512)), core="cluster_stream", big_frame=0)
    _is(_forms(ask, 1, size=size(1025, 512)), core="cluster_stream", big_frame=1)
    _is(_forms(ask, 1, size=size(1024, 513)), core="cluster_stream", big_frame=1)
    _is(_forms(ask, 1, size=size(1025, 8), SSLAM_NFA_STREAM=0), core="cluster", big_frame=1)
    _is(_forms(ask, 1, size=size(2048, 2048)), sort_runs=1)
    _is(_forms(ask, 1, size=size(2049, 8)), sort_runs=0)
    _is(_forms(ask, 1, size=size(8, 2049)), sort_runs=0)
    _is(_forms(ask, 4096, size=size(2049, 2049)), sort_runs=0, core="per_frame")
    _is(_forms(ask, 1, size=(16384, 16384, 13107, 13107)), lbd_rpi=1, sort_runs=0, core="lone")
    _is(_forms(ask, 1, size=(16385, 480, 13108, 384)), lbd_rpi=0)
    _is(_forms(ask, 1, size=(640, 16385, 512, 13108)), lbd_rpi=0)


@pytest.mark.parametrize("knob, want", [
    (None, {8: 10, 9: 10, 16: 10, 17: 10, 24: 10, 25: 8, 64: 4}),
    ("1", {8: 1, 9: 2, 16: 2, 17: 2, 64: 2}),
    ("40", {8: 16, 9: 16, 16: 16, 17: 10, 64: 4}),
    ("17", {8: 16, 9: 16, 16: 16, 17: 10, 64: 4}),           # CL_MAXWG + 1
])
def test_cluster_workgroups(ask, knob, want):
    """SSLAM_CL_WGS workgroups per frame, clamped to [1, CL_MAXWG]; from 9 frames on the frames of an XCD share its 32 compute units, two workgroups a frame at least"""
    env = {} if knob is None else {"SSLAM_CL_WGS": knob}
    for n, wgs in want.items():
        _is(_forms(ask, n, **env), core="cluster_stream", cl_wgs=wgs, cl_window=160, cl_smap=0)
        _is(_forms(ask, n, SSLAM_NFA_STREAM=0, **env), core="cluster", cl_wgs=wgs)
    _is(_forms(ask, 65, **env), core="lone", cl_wgs=0, cl_window=0)


DEFAULTS = dict(lone=-1, cluster=1, persist=0, cl_wgs=10, cl_window=160, cl_smap=0, nfa_stream_waves=16, nfa_spin_ticks=5000000, nfa_fused=1)


@pytest.mark.parametrize("env, want", [
    ({}, {}),
    ({"SSLAM_LSD_FLAVOUR": "cl"}, dict(lone=1, cluster=1)),
    ({"SSLAM_LSD_FLAVOUR": "lat"}, dict(lone=1, cluster=0)),
    ({"SSLAM_LSD_FLAVOUR": "thr"}, dict(lone=0, cluster=0)),
    ({"SSLAM_LSD_FLAVOUR": "x"}, dict(lone=0, cluster=0)),
    ({"SSLAM_LSD_FLAVOUR": "cl", "SSLAM_LSD_CLUSTER": "0"}, dict(lone=1, cluster=0)),
    ({"SSLAM_LSD_CLUSTER": "0"}, dict(cluster=0)),
    ({"SSLAM_LSD_CLUSTER": "5"}, {}),
    ({"SSLAM_LSD_FLAVOUR": "lat", "SSLAM_LSD_CLUSTER": "1"}, dict(lone=1, cluster=0)),           # the knob only ever turns the cluster form off
    ({"SSLAM_LSD_PERSIST": "64"}, dict(persist=64)),
    ({"SSLAM_LSD_PERSIST": "71"}, dict(persist=64)),
    ({"SSLAM_LSD_PERSIST": "8"}, dict(persist=8)),
    ({"SSLAM_LSD_PERSIST": "15"}, dict(persist=8)),
    ({"SSLAM_LSD_PERSIST": "7"}, {}),
    ({"SSLAM_LSD_PERSIST": "0"}, {}),
    ({"SSLAM_LSD_PERSIST": "-8"}, {}),
    ({"SSLAM_CL_WGS": "1"}, dict(cl_wgs=1)),
    ({"SSLAM_CL_WGS": "0"}, dict(cl_wgs=1)),
    ({"SSLAM_CL_WGS": "-3"}, dict(cl_wgs=1)),
    ({"SSLAM_CL_WGS": "16"}, dict(cl_wgs=16)),
    ({"SSLAM_CL_WGS": "17"}, dict(cl_wgs=16)),
    ({"SSLAM_CL_WGS": "40"}, dict(cl_wgs=16)),
    ({"SSLAM_CL_WINDOW": "7"}, dict(cl_window=7)),
    ({"SSLAM_CL_WINDOW": "0"}, dict(cl_window=0)),
    ({"SSLAM_CL_WINDOW": "-1"}, dict(cl_window=-1)),
    ({"SSLAM_CL_WINDOW": "-5"}, dict(cl_window=-1)),
    ({"SSLAM_CL_NO_FEEDER": "1"}, dict(cl_window=160 + (1 << 20))),
    ({"SSLAM_CL_NO_FEEDER": "0"}, dict(cl_window=160 + (1 << 20))),                              # being set is what counts
    ({"SSLAM_CL_WINDOW": "0", "SSLAM_CL_NO_FEEDER": "1"}, dict(cl_window=1 << 20)),
    ({"SSLAM_CL_WINDOW": "-1", "SSLAM_CL_NO_FEEDER": "1"}, dict(cl_window=-1)),
    ({"SSLAM_CL_SMAP": "3"}, dict(cl_smap=3)),
    ({"SSLAM_CL_SMAP": "-1"}, dict(cl_smap=-1)),
    ({"SSLAM_NFA_STREAM": "0"}, dict(nfa_stream_waves=0)),
    ({"SSLAM_NFA_STREAM": "1"}, dict(nfa_stream_waves=16)),
    ({"SSLAM_NFA_STREAM": "5"}, dict(nfa_stream_waves=5)),
    ({"SSLAM_NFA_STREAM": "64"}, dict(nfa_stream_waves=64)),
    ({"SSLAM_NFA_STREAM": "65"}, dict(nfa_stream_waves=64)),
    ({"SSLAM_NFA_STREAM": "-2"}, dict(nfa_stream_waves=0)),
    ({"SSLAM_NFA_STREAM_TICKS": "123"}, dict(nfa_spin_ticks=123)),
    ({"SSLAM_NFA_STREAM_TICKS": "0"}, dict(nfa_spin_ticks=0)),
    ({"SSLAM_NFA_STREAM_TICKS": "-5"}, dict(nfa_spin_ticks=0)),
    ({"SSLAM_NFA_STREAM_TICKS": "10000000000"}, dict(nfa_spin_ticks=10000000000)),
    ({"SSLAM_NFA_FUSED": "0"}, dict(nfa_fused=0)),
    ({"SSLAM_NFA_FUSED": "1"}, {}),
    ({"SSLAM_NFA_FUSED": "2"}, dict(nfa_fused=2)),
    ({"SSLAM_NFA_FUSED": "7"}, {}),
    ({"SSLAM_NFA_FUSED": "x"}, dict(nfa_fused=0)),
    ({"SSLAM_PROJ_STATS": "1", "SSLAM_BATCH_THREADS": "3", "LSD_FLAVOUR": "thr"}, {}),            # not the line path's
])
def test_knob_parse_and_clamp(ask, env, want):
    assert _knobs(ask, **env) == dict(DEFAULTS, **want)


def test_forms_under_knobs(ask):
    _is(_forms(ask, 1, SSLAM_LSD_FLAVOUR="cl"), core="cluster_stream", nfa="stream")
    _is(_forms(ask, 65, SSLAM_LSD_FLAVOUR="cl"), core="lone")
    _is(_forms(ask, 2048, SSLAM_LSD_FLAVOUR="cl"), core="lone", nfa="all")
    _is(_forms(ask, 1, SSLAM_LSD_FLAVOUR="cl", SSLAM_LSD_CLUSTER=0), core="lone", nfa="launches", eval_waves=32, count_waves=128, stream_waves=0)
    _is(_forms(ask, 1, SSLAM_LSD_CLUSTER=0), core="lone", nfa="launches", eval_waves=32, count_waves=128)
    _is(_forms(ask, 2048, SSLAM_LSD_CLUSTER=0), core="per_frame", nfa="all")
    _is(_forms(ask, 2048, SSLAM_LSD_FLAVOUR="lat"), core="lone", nfa="all", eval_waves=1, count_waves=1, fork_blur_sobel=1)
    _is(_forms(ask, 1, SSLAM_LSD_FLAVOUR="lat"), core="lone", nfa="launches", eval_waves=32, count_waves=128)
    _is(_forms(ask, 1, SSLAM_LSD_FLAVOUR="thr"), core="per_frame", nfa="launches", eval_waves=32, count_waves=128, fork_blur_sobel=0)
    _is(_forms(ask, 4097, SSLAM_LSD_FLAVOUR="thr"), core="six_wave")
    # SSLAM_NFA_FUSED does not reach the streaming stage
    _is(_forms(ask, 1, SSLAM_NFA_FUSED=2), core="cluster_stream", nfa="stream", eval_waves=16, count_waves=0)
    _is(_forms(ask, 1, SSLAM_NFA_FUSED=2, SSLAM_NFA_STREAM=0), core="cluster", nfa="all", eval_waves=1, count_waves=1, topn=0)
    _is(_forms(ask, 1, topn=40, SSLAM_NFA_FUSED=2, SSLAM_NFA_STREAM=0), core="cluster", nfa="topn", eval_waves=1, count_waves=1, topn=40)
    _is(_forms(ask, 1, SSLAM_NFA_FUSED=0, SSLAM_NFA_STREAM=0), core="cluster", nfa="launches", eval_waves=32, count_waves=128)
    # the 18 launches validate everything: no top-N under a forced SSLAM_NFA_FUSED=0
    _is(_forms(ask, 4096, SSLAM_NFA_FUSED=0), core="per_frame", nfa="launches", eval_waves=1, count_waves=1, topn=0)
    _is(_forms(ask, 4096, topn=40, SSLAM_NFA_FUSED=0), core="per_frame", nfa="launches", eval_waves=1, count_waves=1, topn=0)
    _is(_forms(ask, 4096, topn=40), core="per_frame", nfa="topn", eval_waves=1, count_waves=1, topn=40)
    for knob, core, nfa, ev, cnt, waves, ticks in [("0", "cluster", "launches", 32, 128, 0, 0), ("1", "cluster_stream", "stream", 16, 0, 16, 5000000),
                                                   ("5", "cluster_stream", "stream", 5, 0, 5, 5000000), ("64", "cluster_stream", "stream", 64, 0, 64, 5000000),
                                                   ("65", "cluster_stream", "stream", 64, 0, 64, 5000000)]:
        _is(_forms(ask, 1, SSLAM_NFA_STREAM=knob), core=core, nfa=nfa, eval_waves=ev, count_waves=cnt, stream_waves=waves, spin_ticks=ticks)
    _is(_forms(ask, 1, SSLAM_NFA_STREAM_TICKS=77), nfa="stream", spin_ticks=77)
    _is(_forms(ask, 3, SSLAM_CL_WINDOW=-1, SSLAM_CL_SMAP=-1, SSLAM_CL_WGS=3), core="cluster_stream", cl_wgs=3, cl_window=-1, cl_smap=-1)
    _is(_forms(ask, 3, SSLAM_CL_NO_FEEDER=1), cl_window=160 + (1 << 20))
