"""Frames for the middle of the line branch -- the LSD prologue, the sequential core (csrc/lsd_regions.h, lsd_cluster.h) and the NFA stage (csrc/lsd_nfa.h) -- built by
numpy alone.  tests/test_lsd_cases_cpu.py proves from the oracle's trace (oracle/lsd_oracle.cpp LsdTrace) what each frame reaches; tests/test_lsd_forms_gpu.py runs them
through every launch form.  Nothing here is searched at import time: where a family had to be searched, the parameters that hit are written down and the search is
described next to them."""
import functools
import numpy as np

MAX_SEG = 8192          # csrc/lsd_plan.h: candidate rectangles per frame
QCAP = 768              # csrc/lsd_regions.h: region points held in LDS; the list continues in global memory
NFA_STREAM_BLOCK = 8    # csrc/lsd_nfa.h: rectangles per claim of the streaming NFA stage
CORE_W, CORE_H = 320, 240          # every core case: scaled 256 x 192, so nXB == 1 sits at its bound
LIMIT_W, LIMIT_H = 1280, 960


def _flat(w, h, v):
    return np.full((h, w), v, np.uint8)


def logistic_edge(scale, c0, c1, row=120, lo=90, hi=170, w=CORE_W, h=CORE_H):
    """a horizontal edge over the columns c0 .. c1: lo above `row`, hi below, through a logistic of the given scale (in rows)"""
    y = np.arange(h, dtype=np.float64)[:, None]
    v = lo + (hi - lo) / (1.0 + np.exp(-(y - row) / scale))
    img = np.full((h, w), float(lo))
    img[:, c0:c1 + 1] = v
    return np.rint(img).astype(np.uint8)


def step_column(col, w=CORE_W, h=CORE_H, lo=90, hi=170):
    """a full-height step: the columns from `col` on at hi"""
    img = _flat(w, h, lo); img[:, col:] = hi
    return img


def diagonal(w=CORE_W, h=CORE_H, lo=90, hi=170):
    """a corner-to-corner edge: hi below the diagonal from (0, 0) to (w - 1, h - 1)"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(y * (w - 1) > x * (h - 1), hi, lo).astype(np.uint8)


def checkerboard(sq, w=CORE_W, h=CORE_H, lo=40, hi=210):
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // sq) + (y // sq)) % 2 == 0, lo, hi).astype(np.uint8)


def waves_noise(seed=5, w=CORE_W, h=CORE_H):
    """128 + 60 sin(x / 7) sin(y / 9) + N(0, 4) of Generator(PCG64(seed))"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    n = np.random.Generator(np.random.PCG64(seed)).normal(0, 4, (h, w))
    return np.clip(np.rint(128 + 60 * np.sin(x / 7) * np.sin(y / 9) + n), 0, 255).astype(np.uint8)


def soft_arc(radius, cx, cy, soft, lo=60, hi=200, w=CORE_W, h=CORE_H):
    """a disc of `radius` about (cx, cy) whose edge is a logistic of scale `soft` pixels: long curved regions that refine"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = np.hypot(x - cx, y - cy)
    return np.rint(lo + (hi - lo) / (1.0 + np.exp((r - radius) / soft))).astype(np.uint8)


def spiral(period, amp=90, w=CORE_W, h=CORE_H):
    """128 + amp sin(r / period + theta) about the centre"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x -= w / 2; y -= h / 2
    return np.clip(np.rint(128 + amp * np.sin(np.hypot(x, y) / period + np.arctan2(y, x))), 0, 255).astype(np.uint8)


def squares(n, per_row, side=12, pitch=22, x0=8, y0=8, lo=60, hi=200, w=CORE_W, h=CORE_H, bars=()):
    """n isolated squares (value hi on lo) in raster order, per_row to a row, the first at (x0, y0); bars: (x, y, length, thickness) rectangles at hi.  Every square
    gives 4 candidate rectangles."""
    img = _flat(w, h, lo)
    for k in range(n):
        x, y = x0 + (k % per_row) * pitch, y0 + (k // per_row) * pitch
        assert x + side < w and y + side < h
        img[y:y + side, x:x + side] = hi
    for bx, by, bl, bt in bars:
        img[by:by + bt, bx:bx + bl] = hi
    return img


def strokes(w, h):
    """the head-size frames: a diagonal edge and a few strokes, scaled to the frame"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.where(y * max(w - 1, 1) > x * max(h - 1, 1), 150, 70).astype(np.uint8)
    img[h // 5:h // 5 + max(2, h // 16), w // 8:w - w // 8] = 220
    img[h // 8:h - h // 8, w - w // 4:w - w // 4 + max(2, w // 20)] = 20
    img[h - h // 4:h - h // 4 + max(1, h // 30), w // 10:w // 2] = 240
    return img


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (generator, what the trace must show: counter -> exact value, or (">=", bound)).  tests/test_lsd_cases_cpu.py asserts every entry.
#
# The searches behind the parameters (run once against the oracle's trace, not repeated here):
#   * region sizes: at 320 x 240 a vertical edge is too short for 768 points (192 scaled rows, three points a row), so the edge lies horizontally.  Plain steps over the
#     columns c0 .. c1 (rows 120 .. 124, c0 0 .. 11, c1 300 .. 319, tilted by 0 .. 2 pixels: 3 600 frames) gave none of the three sizes; logistic edges of scale 1.0 .. 3.0 in
#     steps of 0.5, c0 20 .. 23, c1 120 .. 299 gave all three, the first hit of each is kept.
#   * refine() / reduce_region_radius() beyond the LDS queue: soft arcs of radius 100 .. 300 with the centre below the frame, softness 2 .. 4, and spirals of period 3 .. 8.
#     The period-3 spiral stops at 646 points; radius 300 / softness 3 and the period-8 spiral enter both functions with more than 768 points.
#   * exactly one candidate: bars of 3 .. 20 x 1 .. 3 pixels; 8 x 2 gives one region of min_reg_size + 1 points at 320 x 240.
#   * the smallest overflow: 2 048 squares (8 192 candidates) plus one bar.  At 1280 x 960 (min_reg_size 17) bars of 6 .. 29 x 1 .. 3 pixels were tried: 9 x 3, 10 x 2 and
#     11 x 2 give one candidate, everything longer two: 8 193 with the 10 x 2 bar.
#   * nfa()'s tail loop running to n without its break is not reachable: the last iteration (i == n) has bin_term = 1 / n < 1 and err = term * ((1 - m) / (1 - m) - 1) = 0,
#     which is below the bound unless the bound is exactly 0; no frame of any family here (nor the fuzz frames of tools/fuzz_parity.py) has shown it.
BAR1 = (100, 150, 8, 2)          # one candidate rectangle, rejected
CORE = {
    "region767": (lambda: logistic_edge(3.0, 20, 182), {"reg767": 1, "reg_max": 767, "nfa_term0_above": (">=", 1)}),
    "region768": (lambda: logistic_edge(1.5, 23, 185), {"reg768": 1, "reg_max": 768}),
    "region769": (lambda: logistic_edge(1.0, 20, 182), {"reg769": 1, "reg_max": 769}),
    "arc300": (lambda: soft_arc(300, 160, 400, 3.0), {"refines_big": (">=", 1), "reduce_iters_big": (">=", 1), "regrown_max": (">=", QCAP + 1)}),
    "spiral8": (lambda: spiral(8), {"refines_big": (">=", 10), "reduce_iters_big": (">=", 1), "regrown_max": (">=", QCAP + 1), "nfa_term0_below": (">=", 1)}),
    "arc220": (lambda: soft_arc(220, 160, 320, 2.0), {"refines_big": (">=", 1), "cols_outside": (">=", 100), "touch_col0": (">=", 1), "touch_col_last": (">=", 1)}),
    "waves": (lambda: waves_noise(5), {"refine_false": (">=", 1), "refines": (">=", 300), "rows_outside": (">=", 1), "cols_outside": (">=", 1), "improve3": (">=", 1), "improve4": (">=", 1)}),
    "checker8": (lambda: checkerboard(8), {"reg_min_m1": (">=", 100), "reg_min": (">=", 100), "improve0": (">=", 1), "improve1": (">=", 1), "improve2": (">=", 1),
                                           "improve5": (">=", 1), "nfa_all": (">=", 1), "nfa_zero": (">=", 1), "nfa_break": (">=", 1)}),
    "checker10": (lambda: checkerboard(10), {"improve3": (">=", 1), "improve4": (">=", 1), "rejected": (">=", 1)}),
    "checker12": (lambda: checkerboard(12), {"improve%d" % i: (">=", 1) for i in range(6)}),
    "diagonal": (lambda: diagonal(), {"rows_outside": (">=", 1), "nfa_term0_below": (">=", 1), "touch_row0": 1, "touch_row_last": 1, "touch_col0": 1, "touch_col_last": 1,
                                      "reg_max": (">=", QCAP + 1)}),
    "step160": (lambda: step_column(160), {"candidates": 1, "touch_row0": 1, "touch_row_last": 1, "nfa_all": (">=", 1)}),
    "constant": (lambda: _flat(CORE_W, CORE_H, 128), {"defined": 0, "seeds": 0, "candidates": 0}),
    "speck": (lambda: squares(0, 1, bars=[(100, 150, 3, 1)]), {"seeds": (">=", 1), "defined": (">=", 1), "candidates": 0}),
    "cand1": (lambda: squares(0, 1, bars=[BAR1]), {"candidates": 1, "segments": 0}),
    "cand8": (lambda: squares(2, 2), {"candidates": NFA_STREAM_BLOCK}),
    "cand9": (lambda: squares(2, 2, bars=[BAR1]), {"candidates": NFA_STREAM_BLOCK + 1}),
}

LIMIT = {
    "squares2048": (lambda: squares(2048, 58, w=LIMIT_W, h=LIMIT_H), {"candidates": MAX_SEG}),
    "squares2048_bar": (lambda: squares(2048, 58, w=LIMIT_W, h=LIMIT_H, bars=[(20, 880, 10, 2)]), {"candidates": MAX_SEG + 1}),
    "checker12": (lambda: checkerboard(12, w=LIMIT_W, h=LIMIT_H), {"candidates": (">=", 2 * MAX_SEG + 1), "segments": (">=", MAX_SEG + 1)}),
    "checker16": (lambda: checkerboard(16, w=LIMIT_W, h=LIMIT_H), {"candidates": (">=", MAX_SEG + 1)}),
}

# Head sizes (w, h): a diagonal edge and a few strokes each (strokes()).  320 | 321: scaled 256 | 257 wide, one | two 256-pixel segments a row; 640 | 641; 240 | 241 high:
# 192 | 193 scaled rows of 32-row counting-sort tiles (six full tiles | a seventh of one row); 20 x 10 the smallest geometry of the fused blur + gradient kernel, 25 x 10
# beside it; 10 the smallest side the library accepts (include/sslam_frontend.h), 12 the narrowest width of the blur kernels' uniform row loads.
HEADS = ((320, 240), (321, 240), (320, 241), (640, 480), (641, 480), (20, 10), (25, 10), (10, 10), (10, 40), (40, 10), (11, 13), (12, 12))
MIN_SIDE = 10
TOO_SMALL = ((20, 5), (320, 8), (321, 8), (8, 400), (9, 9), (9, 100), (100, 9), (1, 1), (2, 2), (3, 7))


@functools.lru_cache(maxsize=None)
def frame(group, name):
    """the frame of CORE / LIMIT[name] or of the head size name = (w, h): read-only, built once"""
    img = strokes(*name) if group == "head" else {"core": CORE, "limit": LIMIT}[group][name][0]()
    assert img.dtype == np.uint8
    img.setflags(write=False)
    return img
