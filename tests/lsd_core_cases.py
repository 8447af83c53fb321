"""Frames for the sequential LSD core on its own (csrc/lsd_regions.h, csrc/lsd_cluster.h), built by numpy alone: what tests/test_lsd_core_gpu.py runs through
sslam_testing_lines_core (include/sslam_testing.h) in every launch form and compares with the oracle's core record (oracle/lsd_oracle.cpp LsdCore, Oracle.lsd_core) -- every
candidate rectangle in all twelve doubles, the used map pixel for pixel.  tests/test_lsd_core_cases_cpu.py proves from that record alone what each frame reaches.  Nothing
here is searched at import time: the parameters that hit are written down and the search is described next to them, as in tests/lsd_cases.py, whose 17 core frames and 12
head sizes are reused as they are (region sizes 767 / 768 / 769, refine / reduce beyond the LDS queue, border touches, 0 / 1 / 8 / 9 candidates).

The constants are the code's own as it stands (csrc/lines.hip pins CL_STG and the two bitmap sizes with static_asserts next to lines_forms' limits)."""
import functools
import numpy as np
import lsd_cases as lc

TORUS_REACH = 254          # csrc/lsd_regions.h TorusWide::REACH (= lsd_cluster.h ClTorus): a helper gives a region up when a point lies FURTHER than this from the seed, in x or y
CL_STG = 32                # csrc/lsd_cluster.h: list entries (nA + nB) the feeder stages per result; `stageable = cnt > 1 && cnt <= CL_STG`
LDS_SW, LDS_SH = 1024, 512          # csrc/lsd_regions.h TorusFrame / csrc/lines_form.h LINES_CLUSTER_LDS_SW, _SH: bigFrame = sw > 1024 || sh > 512
HELPER_POINTS = 600        # well below capN - 64 = 704 (csrc/lsd_regions.h region_grow_w: a helper gives up when n + 64 > capN): a region this small is given up for its reach alone
REACH_W, REACH_H = 400, 60          # scaled 320 x 48, a geometry of the fused blur + gradient kernel


def step_edge(c0, c1, row=30, lo=90, hi=170, w=REACH_W, h=REACH_H):
    """a horizontal step over the columns c0 .. c1: hi from `row` down"""
    img = np.full((h, w), lo, np.uint8); img[row:, c0:c1 + 1] = hi
    return img


def bar(length, thick):
    """one isolated bar at 320 x 240"""
    return lc.squares(0, 1, bars=[(100, 150, length, thick)])


def star(spokes, gap, soft, half_width, w=lc.CORE_W, h=lc.CORE_H, lo=70, hi=190):
    """`spokes` straight lines of half width `half_width` (anti-aliased) through the centre, and above them two parallel horizontal edges `gap` rows apart, each a logistic of
    scale `soft` rows: regions that meet at one point and regions a few pixels apart, where a later seed keeps running into pixels an earlier seed took"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64); cx, cy = w / 2 - 0.5, h / 2 - 0.5
    img = np.full((h, w), float(lo))
    for k in range(spokes):
        a = np.pi * k / spokes
        d = np.abs(-(x - cx) * np.sin(a) + (y - cy) * np.cos(a))
        img = np.maximum(img, lo + (hi - lo) * np.clip(half_width + 0.5 - d, 0, 1))
    e = lo + (hi - lo) / (1 + np.exp(-(y - 30) / soft)) - (hi - lo) / (1 + np.exp(-(y - 30 - gap) / soft))
    img[:60] = np.maximum(img[:60], e[:60])
    return np.rint(np.clip(img, 0, 255)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (generator, what Oracle.lsd_core must show).  The keys of the second dict, asserted by tests/test_lsd_core_cases_cpu.py:
#   "reach": v / (">=", v)   (with "points_max": of a candidate of at most that many points) some candidate's `reach` (largest Chebyshev distance from the seed of any point the region held, first growth and regrowth) is exactly / at least v
#   "list_len": v            some grown seed's list length (points of the first growth + points of refine()'s regrowth: MwRes nA + nB) is exactly v
#   "blocked_joins": (">=", v)
#   "size": (sw, sh), "cross_col": c / "cross_row": r / "touch_col": c / "touch_row": r   the scaled size; some candidate's points span (x0 <= c <= x1) / end at (x1 == c) that column / row
#
# The searches (run once against Oracle.lsd_core, not repeated here):
#   * reach: horizontal edges at 400 x 60 over the columns c0 .. c1, c0 0 .. 7, c1 300 .. 399, as a plain step and as logistic edges of scale 1, 1.5, 2, 3 rows.  All pixels of
#     such an edge share one gradient, so the seed is its leftmost pixel and the reach the edge's scaled length.  The plain step (90 | 170) gave 253, 254, 255 and 300 at the
#     first three c0; its regions are three pixels thick, 764 .. 901 points: beyond what a helper grows at all (it gives up when n + 64 > capN = min(QCAP, LISTCAP - 24) = 768), so
#     those frames put the main wave's own growth across the reach and the LDS queue's end (QCAP) at once.  For the torus to decide, the region must stay below capN: steps of
#     8 .. 30 gray levels and lines one pixel thick (c0 0 .. 4, c1 312 .. 329) -- the step of 10 levels (90 | 100) leaves ONE defined pixel per column, regions of 254 .. 257
#     points with the three reaches: the "thin" set.  The logistic edges reach the values too (scale 1: regions of about 1 530 points) and add nothing to the two sets.  No region
#     of the family regrows.  The 256-bit torus (reach 126) is a compile-time alternative that is not built: no cases.
#   * list length: one bar of 1 .. 39 x 1 .. 5 pixels at (100, 150).  Lengths 1 and 2 come with the bars one pixel long (1 x 1: four seeds of each); 32 first at
#     21 x 1 (two seeds), 33 at 22 x 1 and 15 x 3.  All four are first growths without a regrowth (nB = 0); min_reg_size is 14 at 320 x 240, so 32 and 33 are candidates.
#   * contention: star(spokes, gap, soft, half_width) over spokes 16 .. 48, gap 3 .. 10, soft 0.7 .. 2, half width 0.5 .. 1.5 (252 frames).  blocked_joins of lsd_cases'
#     step160 is 0 -- one region, nothing to run into -- so "ten times step160" holds for every frame; the bound stated here is what the three kept frames reach: at least
#     2 400 (5 331, 2 706, 2 490; the smallest of the family was 322; lsd_cases' `waves` has 18 305 and runs with the existing frames).
#   * the LDS / global bitmap boundary: lc.strokes() as it is.  1280 x 640 is scaled 1024 x 512, the largest frame of the LDS bitmap: no pixel lies at column 1023 or row 511
#     that could hold a gradient (the last are 1022 and 510), and its diagonal's regions end exactly there.  1285 x 640 (1028 wide) and 1280 x 645 (516 high) each have one
#     candidate whose points span column 1023 / row 511.  No extra stroke was needed.
REACH = {
    "step253": (lambda: step_edge(0, 319), {"reach": 253}),
    "step254": (lambda: step_edge(0, 320), {"reach": 254}),
    "step255": (lambda: step_edge(1, 323), {"reach": 255}),
    "step300": (lambda: step_edge(0, 376), {"reach": (">=", 300)}),
    "thin253": (lambda: step_edge(0, 318, hi=100), {"reach": 253, "points_max": HELPER_POINTS}),
    "thin254": (lambda: step_edge(0, 319, hi=100), {"reach": 254, "points_max": HELPER_POINTS}),
    "thin255": (lambda: step_edge(1, 323, hi=100), {"reach": 255, "points_max": HELPER_POINTS}),
}
STG = {
    "bar1x1": (lambda: bar(1, 1), {"list_len": [1, 2]}),
    "bar21x1": (lambda: bar(21, 1), {"list_len": [CL_STG]}),
    "bar22x1": (lambda: bar(22, 1), {"list_len": [CL_STG + 1]}),
    "bar15x3": (lambda: bar(15, 3), {"list_len": [CL_STG + 1]}),
}
CONTENTION_MIN = 2400
CONTENTION = {
    "star48a": (lambda: star(48, 10, 2.0, 0.5), {"blocked_joins": (">=", 5000)}),
    "star48b": (lambda: star(48, 10, 1.5, 0.7), {"blocked_joins": (">=", CONTENTION_MIN)}),
    "star40": (lambda: star(40, 10, 2.0, 1.0), {"blocked_joins": (">=", CONTENTION_MIN)}),
}
BITMAP = {          # single frames only, cluster and lone
    "lds_1024x512": (lambda: lc.strokes(1280, 640), {"size": (LDS_SW, LDS_SH), "touch_col": LDS_SW - 2, "touch_row": LDS_SH - 2}),
    "global_1028w": (lambda: lc.strokes(1285, 640), {"size": (LDS_SW + 4, LDS_SH), "cross_col": LDS_SW - 1}),
    "global_516h": (lambda: lc.strokes(1280, 645), {"size": (LDS_SW, LDS_SH + 4), "cross_row": LDS_SH - 1}),
}
GROUPS = {"reach": REACH, "stg": STG, "contention": CONTENTION, "bitmap": BITMAP}


@functools.lru_cache(maxsize=None)
def frame(group, name):
    """the frame of a case here, or of lsd_cases' groups "core", "head" and "limit": read-only, built once"""
    if group in ("core", "head", "limit"): return lc.frame(group, name)
    img = GROUPS[group][name][0]()
    assert img.dtype == np.uint8
    img.setflags(write=False)
    return img


def existing():
    """(group, name) of the frames of tests/lsd_cases.py reused here: its 17 core cases and 12 head sizes"""
    return [("core", n) for n in lc.CORE] + [("head", wh) for wh in lc.HEADS]


def new(groups=("reach", "stg", "contention", "bitmap")):
    return [(g, n) for g in groups for n in GROUPS[g]]


def small_320x240():
    """the 320 x 240 frames, the new ones first (a batch of fewer frames than cases takes the head of the list): what a batch tiles"""
    return [(g, n) for g, n in new(("contention", "stg")) + existing() if frame(g, n).shape == (lc.CORE_H, lc.CORE_W)]
