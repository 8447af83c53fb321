"""Segment lists for the line tail (k_keylines, k_blur_sobel, k_lbd: csrc/lbd.h) -- what tests/test_line_tail_gpu.py injects through sslam_testing_lines_tail and
tests/test_line_tail_cases_cpu.py checks, from the oracle alone, to reach what each case is named after.  Everything is seeded; a segment is x1, y1, x2, y2 in source
pixels, a list is in emission order."""
import functools
import numpy as np
from synth import synth_frame, noise_frame

MAX_SEG = 8192          # csrc/lsd_plan.h
KL_LDS = 1024           # csrc/lbd.h: more accepted segments than this sort in global memory
LBD_TB = 8              # csrc/lbd.h: steps per block of k_lbd's walk
LSP_H = 63              # rows of LBD's line-support region

# name -> (w, h, generator).  w % 4 == 0: k_blur_sobel stores 16 bytes at a time; 199: its per-pixel stores.  16384: the largest side k_lbd<true> takes;
# 16388 wide / high: k_lbd<false> through either side of the launch's condition.
IMAGES = {
    "noise160": (160, 120, lambda: noise_frame(11, w=160, h=120)),
    "synth160": (160, 120, lambda: synth_frame(12, w=160, h=120)),
    "noise199": (199, 151, lambda: noise_frame(13, w=199, h=151)),
    "synth199": (199, 151, lambda: synth_frame(14, w=199, h=151)),
    "strip16384": (16384, 48, lambda: noise_frame(15, w=16384, h=48)),
    "strip16388": (16388, 48, lambda: noise_frame(16, w=16388, h=48)),
    "tower16388": (48, 16388, lambda: noise_frame(17, w=48, h=16388)),
}
SMALL = ("noise160", "synth160", "noise199", "synth199")
NPX = tuple(range(2, 18))       # numOfPixels of the short lines: every residue mod LBD_TB, walks shorter than one block and of two blocks and a step


@functools.lru_cache(maxsize=None)
def image(name):
    img = IMAGES[name][2]()
    assert img.shape == (IMAGES[name][1], IMAGES[name][0]) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------------------------------------------------------- directions and lengths
EXACT_DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))       # angle 0, pi/2, pi, -pi/2, pi/4, 3pi/4, -pi/4, -3pi/4


def directions():
    """(dx, dy) with max(|dx|, |dy|) == 1: every whole degree of the circle, then the exact axis and diagonal directions"""
    out = []
    for deg in range(360):
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        m = max(abs(c), abs(s))
        out.append((c / m, s / m))
    return out + [(float(a), float(b)) for a, b in EXACT_DIRS]


def long_line(name):
    """the line that spans the image: corner to corner, on the strips across the full length"""
    w, h, _ = IMAGES[name]
    if w > 1000: return (0.25, 10.25, w - 1.25, 37.75)
    if h > 1000: return (10.25, 0.25, 37.75, h - 1.25)
    return (0.25, 0.25, w - 1.25, h - 1.25)


LONG_AT = 1000          # where the long line sits in the list


def direction_case(name):
    """every direction x every numOfPixels of NPX, wholly inside the image (no endpoint clamps), + the long line: dict(img, segs, npx, max_lines, cap).  A start has the
    fraction .25 and the dominant coordinate moves by npx - 1 exactly, so the rounded endpoints are npx - 1 apart."""
    w, h, _ = IMAGES[name]
    rng = np.random.default_rng([21, w, h, sum(map(ord, name))])
    segs, npx = [], []
    for dx, dy in directions():
        for n in NPX:
            ex, ey = dx * (n - 1), dy * (n - 1)
            x1 = float(rng.integers(max(0, int(np.ceil(-ex))), min(w - 1, int(np.floor(w - 1.25 - ex))))) + 0.25
            y1 = float(rng.integers(max(0, int(np.ceil(-ey))), min(h - 1, int(np.floor(h - 1.25 - ey))))) + 0.25
            segs.append((x1, y1, x1 + ex, y1 + ey)); npx.append(n)
    segs.insert(LONG_AT, long_line(name)); npx.insert(LONG_AT, max(w, h))
    segs = np.array(segs, np.float32)
    assert segs.min() >= 0 and segs[:, [0, 2]].max() < w and segs[:, [1, 3]].max() < h and len(segs) <= MAX_SEG
    return dict(img=image(name), segs=segs, npx=np.array(npx), max_lines=len(segs), cap=len(segs))


def lgs_class(angle):
    """the gather mapping k_lbd takes for a line of this KeyLine.angle: its comment's cost rule, 2^c |sin| + (64 >> c) |cos| over c = 0 .. 3 in fp32, the first smallest.
    For counting coverage only."""
    a = np.asarray(angle, np.float32).astype(np.float64)
    c0, s0 = np.abs(np.cos(a).astype(np.float32)), np.abs(np.sin(a).astype(np.float32))
    cost = np.stack([(np.float32(1 << c) * s0).astype(np.float32) + (np.float32(64 >> c) * c0).astype(np.float32) for c in range(4)])
    return np.argmin(cost, axis=0)          # (argmin returns the first of equal minima, as the kernel's `<`)


# ---------------------------------------------------------------------------------------------------------------- borders and clamps
CLAMPS = ("x1<0", "x1>=w", "x2<0", "x2>=w", "y1<0", "y1>=h", "y2<0", "y2>=h")       # checkLineExtremes, in its order


def border_case(name):
    """lines on and along every border, into and out of every corner, and endpoints beyond the image on every side (a coordinate exactly w / h, the float just below it,
    and farther out); no segment clamps to zero length"""
    w, h, _ = IMAGES[name]
    W1, H1 = float(w - 1), float(h - 1)
    segs = []
    def both(a):
        segs.append(a); segs.append((a[2], a[3], a[0], a[1]))
    for L in (3.0, 9.5, 40.25):
        for y in (0.0, 0.4, 7.25, H1 - 7.25, H1 - 0.4, H1): both((2.25, y, 2.25 + L, y)); both((W1 - 2.25 - L, y, W1 - 2.25, y))
        for x in (0.0, 0.4, 7.25, W1 - 7.25, W1 - 0.4, W1): both((x, 2.25, x, 2.25 + L)); both((x, H1 - 2.25 - L, x, H1 - 2.25))
    both((0.0, 0.0, W1, 0.0)); both((0.0, H1, W1, H1)); both((0.0, 0.0, 0.0, H1)); both((W1, 0.0, W1, H1))       # the whole border rows and columns
    for cx, sx in ((0.0, 1.0), (W1, -1.0)):
        for cy, sy in ((0.0, 1.0), (H1, -1.0)):
            for dx, dy in ((1, 0), (0, 1), (1, 1), (2, 1), (1, 3)):
                for L in (4.0, 13.5, 30.0): both((cx + sx * dx * L, cy + sy * dy * L, cx, cy))
    wb, hb = float(np.nextafter(np.float32(w), np.float32(0))), float(np.nextafter(np.float32(h), np.float32(0)))      # just below w / h: not clamped
    for out_x, in_x in ((-3.5, 15.25), (-0.001, 22.25), (float(w), W1 - 20.25), (w + 5.5, W1 - 31.25), (wb, W1 - 12.25)):
        both((out_x, 20.25, in_x, 33.25)); both((out_x, H1 - 20.25, in_x, H1 - 33.25)); both((out_x, 40.25, in_x, 40.25))
    for out_y, in_y in ((-2.5, 18.25), (-0.001, 25.25), (float(h), H1 - 20.25), (h + 7.25, H1 - 31.25), (hb, H1 - 12.25)):
        both((20.25, out_y, 31.25, in_y)); both((W1 - 20.25, out_y, W1 - 31.25, in_y)); both((44.25, out_y, 44.25, in_y))
    both((-4.0, -6.0, 20.25, 25.25)); both((w + 3.0, h + 2.0, W1 - 30.25, H1 - 25.25)); both((-4.0, h + 2.0, 20.25, H1 - 25.25)); both((w + 3.0, -6.0, W1 - 30.25, 25.25))
    both((-5.0, -5.0, w + 5.0, h + 5.0))          # both endpoints clamped
    segs = np.array(segs, np.float32)
    return dict(img=image(name), segs=segs, max_lines=len(segs), cap=len(segs))


def clamps_fired(case, kl):
    """which of the eight checkLineExtremes conditions changed an endpoint, per segment (n x 8 bool), from the keylines of the uncapped list"""
    w, h = case["img"].shape[1], case["img"].shape[0]
    s = case["segs"]
    cols = []
    for c, f, lim in ((0, "startPointX", w), (2, "endPointX", w), (1, "startPointY", h), (3, "endPointY", h)):
        ch = kl[f] != s[:, c]
        cols += [ch & (s[:, c] < 0) & (kl[f] == 0), ch & (s[:, c] >= lim) & (kl[f] == np.float32(lim) - np.float32(1))]
    return np.stack(cols, axis=1)


def walk_extent(kl):
    """x / y range (before rounding and clamping) of the LBD walk of every keyline -> xmin, xmax, ymin, ymax (fp64, for counting coverage only)"""
    a = kl["angle"].astype(np.float64)
    c, s = np.cos(a), np.sin(a)
    hw = ((kl["numOfPixels"].astype(np.int16) - 1) // 2).astype(np.float64); hh = (LSP_H - 1) // 2
    mx = 0.5 * (kl["sPointInOctaveX"].astype(np.float64) + kl["ePointInOctaveX"]); my = 0.5 * (kl["sPointInOctaveY"].astype(np.float64) + kl["ePointInOctaveY"])
    x0 = -c * hw + s * hh + mx; y0 = -s * hw - c * hh + my
    n1 = kl["numOfPixels"].astype(np.float64) - 1
    xs = np.stack([x0, x0 + n1 * c, x0 - (LSP_H - 1) * s, x0 + n1 * c - (LSP_H - 1) * s]); ys = np.stack([y0, y0 + n1 * s, y0 + (LSP_H - 1) * c, y0 + n1 * s + (LSP_H - 1) * c])
    return xs.min(0), xs.max(0), ys.min(0), ys.max(0)


# ---------------------------------------------------------------------------------------------------------------- counts and the sort
COUNTS = (0, 1, 39, 40, 41, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8192)      # accepted segments per frame of the batch
COUNT_MAX_LINES = 40
COUNT_CAP = 64
# exact lengths 5, 10, .. 25 in several directions: the responses of a frame take five values
TIE_VECTORS = tuple((sx * a * k, sy * b * k) for k in range(1, 6) for a, b in ((5, 0), (0, 5), (3, 4), (4, 3)) for sx in (1, -1) for sy in (1, -1) if (a or sx == 1) and (b or sy == 1))


def tie_segments(rng, n, w=160, h=120):
    """n distinct segments of the tie vectors, wholly inside the image"""
    seen, out = set(), []
    while len(out) < n:
        dx, dy = TIE_VECTORS[rng.integers(len(TIE_VECTORS))]
        x1 = float(rng.integers(26, w - 27)) + (0.25, 0.75)[rng.integers(2)]; y1 = float(rng.integers(26, h - 27)) + (0.25, 0.75)[rng.integers(2)]
        s = (x1, y1, x1 + dx, y1 + dy)
        if s not in seen:
            seen.add(s); out.append(s)
    return np.array(out, np.float32)


@functools.lru_cache(maxsize=None)
def count_case():
    """the frames of ONE batch call on noise160: COUNTS[f] accepted among candidates of which about a quarter is rejected by flag (none in the frame that fills MAX_SEG; the
    frame of 0 has five candidates, all rejected); candidates 255 and 256 of every frame that has them are rejected"""
    img = image("noise160")
    nf = len(COUNTS)
    segs = np.zeros((nf, MAX_SEG, 4), np.float32); accept = np.zeros((nf, MAX_SEG), np.uint8); ncand = np.zeros(nf, np.int32)
    for f, n in enumerate(COUNTS):
        rng = np.random.default_rng([31, n])
        nc = min(MAX_SEG, n + max(n // 3, 1)) if n else 5
        fl = np.zeros(nc, np.uint8)
        forced = [i for i in (255, 256) if i < nc and nc - n >= 2]
        free = np.setdiff1d(np.arange(nc), forced)
        fl[rng.choice(free, n, replace=False)] = 1
        assert fl.sum() == n
        segs[f, :nc] = tie_segments(rng, nc); accept[f, :nc] = fl; ncand[f] = nc
    return dict(img=img, images=np.ascontiguousarray(np.broadcast_to(img, (nf,) + img.shape)), segs=segs, accept=accept, ncand=ncand, counts=np.array(COUNTS),
                max_lines=COUNT_MAX_LINES, cap=COUNT_CAP)


def accepted(case, f):
    """the accepted segments of frame f, in emission order: what the oracle's tail is given"""
    nc = int(case["ncand"][f])
    return case["segs"][f, :nc][case["accept"][f, :nc] != 0]


def full_case():
    """MAX_SEG segments under max_lines = MAX_SEG: no sort, MAX_SEG descriptors"""
    return dict(img=image("noise160"), segs=tie_segments(np.random.default_rng(41), MAX_SEG), max_lines=MAX_SEG, cap=MAX_SEG)


def small_cap_case():
    """100 segments, max_lines 40, room for 17: the count clamps to the caller's capacity"""
    return dict(img=image("noise160"), segs=tie_segments(np.random.default_rng(42), 100), max_lines=40, cap=17)


# ---------------------------------------------------------------------------------------------------------------- one whole frame of equal responses
def squares_frame():
    """320x240, value 110, 20x20 squares of value 200 at pitch 40 from (20, 20) -- 7 x 5 of them, the last row and column of the grid left empty so that no square
    touches the border --, no noise: every segment LSD finds has the same length"""
    img = np.full((240, 320), 110, np.uint8)
    for y in range(20, 200, 40):
        for x in range(20, 280, 40): img[y:y + 20, x:x + 20] = 200
    return img
