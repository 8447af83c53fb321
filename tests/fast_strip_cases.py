"""Frames for k_fast_cells' strips (csrc/orb.hip, csrc/fast_strips.h): one wave stages, pre-tests and scores up to K adjacent cells of a cell row as one rectangle
and suppresses and emits per cell.  tests/test_fast_strips_cpu.py proves from the oracle's candidates and a numpy replay of the pre-test that each frame reaches what
it is named after; tests/test_fast_strips_gpu.py runs them through OrbExtractor.  The strip table comes from the product's own header, compiled by plain g++
(tests/sim/fast_strips_dump.cpp) once as it is and once with -fsanitize=address,undefined, as a stand-alone program."""
import atexit, functools, os, shutil, subprocess, tempfile
import numpy as np
import orb_tail_cases as otc
from synth import synth_frame, noise_frame

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "fast_strips_dump.cpp")
MIN_TH, INI_TH = 7, 20
NLEVELS = 8


@functools.lru_cache(maxsize=None)
def programs():
    d = tempfile.mkdtemp(prefix="fast_strips_dump_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    plain, san = os.path.join(d, "fast_strips_dump"), os.path.join(d, "fast_strips_dump_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", san])
    return plain, san


def dump(cells):
    """(constants, strips) of the product's fast_build_strips for cells [(level, x0, y0, x1, y1)]; strips is None when the table is refused"""
    text = "".join("%d %d %d %d %d\n" % c for c in cells)
    outs = []
    for exe in programs():
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    rows = outs[0].split("\n")
    consts = dict(zip(("K", "cap", "idx_bits", "shift"), map(int, rows[0].split())))
    if rows[1] == "refused": return consts, None
    keys = ("level", "x0", "y0", "x1", "y1", "nc", "wc", "cellBeg", "magic", "gmagic", "smagic")
    return consts, [dict(zip(keys, map(int, r.split()))) for r in rows[1:] if r]


def plan_cells(w, h, nlevels=NLEVELS):
    return [(l,) + c for l, L in enumerate(otc.levels(w, h, nlevels)) for c in L["cells"]]


@functools.lru_cache(maxsize=None)
def plan(w, h, nlevels=NLEVELS):
    """(constants, strips, cells) of a frame size, cells in plan order"""
    cells = plan_cells(w, h, nlevels)
    consts, strips = dump(cells)
    assert strips is not None
    return consts, strips, cells


def consts():
    return dump([])[0]


def pretest(img, t=MIN_TH):
    """pass A of k_fast_cells: a 9-arc at threshold t needs a vertical AND a horizontal compass point (distance 3) on its side of the threshold"""
    a = img.astype(np.int16)
    m = np.zeros(a.shape, bool)
    v, n, s, e, w = a[3:-3, 3:-3], a[:-6, 3:-3], a[6:, 3:-3], a[3:-3, 6:], a[3:-3, :-6]
    m[3:-3, 3:-3] = ((np.maximum(n, s) > v + t) & (np.maximum(e, w) > v + t)) | ((np.minimum(n, s) < v - t) & (np.minimum(e, w) < v - t))
    return m


def survivors(oracle, img, nlevels=NLEVELS):
    """survivors of the pre-test per strip and per cell, in plan order"""
    _, strips, cells = plan(img.shape[1], img.shape[0], nlevels)
    I = {}
    for l in sorted({c[0] for c in cells}):
        m = pretest(oracle.pyramid_level(img, l, 1.2, nlevels))
        I[l] = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int64)
        I[l][1:, 1:] = m.cumsum(0).cumsum(1)
    box = lambda l, x0, y0, x1, y1: int(I[l][y1, x1] - I[l][y0, x1] - I[l][y1, x0] + I[l][y0, x0])
    return np.array([box(s["level"], s["x0"], s["y0"], s["x1"], s["y1"]) for s in strips]), np.array([box(*c) for c in cells])


def cell_candidates(oracle, img, level, cell, nfeat=1000):
    """the oracle's FAST candidates (x, y, score in level coordinates) inside a cell's detection rectangle"""
    c = oracle.candidates(img, level, nfeat)
    x, y = c[:, 0] + otc.MINB, c[:, 1] + otc.MINB
    _, x0, y0, x1, y1 = cell
    k = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    return np.stack([x[k], y[k], c[k, 2]], 1)


def border_pairs(oracle, img, level=0):
    """pairs of the oracle's candidates of a level in horizontally adjacent columns (rows at most one apart) with different scores: per-cell suppression lets both live
    only across a border between two cells.  Returns [(border x, inside one strip?, weaker score, stronger score)]"""
    _, strips, cells = plan(img.shape[1], img.shape[0])
    c = oracle.candidates(img, level, 1000)
    x, y, s = c[:, 0] + otc.MINB, c[:, 1] + otc.MINB, c[:, 2]
    at = {(int(a), int(b)): int(v) for a, b, v in zip(x, y, s)}
    inner = {(st["y0"], st["x0"] + k * st["wc"]) for st in strips if st["level"] == level for k in range(1, st["nc"])}
    outer = {(st["y0"], st["x0"]) for st in strips if st["level"] == level}
    rows = {(cl[2], cl[4]) for cl in cells if cl[0] == level}
    out = []
    for (a, b), v in at.items():
        for db in (-1, 0, 1):
            u = at.get((a + 1, b + db))
            if u is None or u == v: continue
            r = [y0 for y0, y1 in rows if y0 <= b < y1 and y0 <= b + db < y1]       # both in one cell row: the border between them is a column border
            if not r: continue
            if (r[0], a + 1) in inner: out.append((a + 1, True, min(u, v), max(u, v)))
            elif (r[0], a + 1) in outer: out.append((a + 1, False, min(u, v), max(u, v)))
    return out


# ---------------------------------------------------------------------------------------------------------------- frames
def _noise(seed, h, w, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w)).astype(np.uint8)


def bands_frame(seed=11, w=640, h=480, half=6):
    """flat, with noise in narrow vertical bands around every column border of level 0's cells: few survivors per strip (the list path), yet corners in adjacent
    columns on either side of the borders"""
    img = np.full((h, w), 128, np.uint8)
    nz = _noise(seed, h, w)
    for x in sorted({c[1] for c in plan_cells(w, h) if c[0] == 0}):
        img[:, x - half:x + half] = nz[:, x - half:x + half]
    return img


def ini_min_frame(seed=12, w=250, h=97):
    """level 0: one row band of seven cells; the cells alternate between noise of full contrast (corners at iniTh) and noise of +-9 grey levels (scores below 20:
    corners at minTh only)"""
    img = np.full((h, w), 128, np.uint8)
    hi_, lo_ = _noise(seed, h, w), _noise(seed + 1, h, w, 119, 138)
    cells = [c for c in plan_cells(w, h) if c[0] == 0]
    for k, (_, x0, y0, x1, y1) in enumerate(cells):
        src = lo_ if k % 2 else hi_
        img[:, x0:x1] = src[:, x0:x1]
    return img


def empty_between_frame(seed=13, w=250, h=97):
    """level 0: the second cell of every strip flat (no candidates), its neighbours noise"""
    img = _noise(seed, h, w)
    _, strips, cells = plan(w, h)
    for s in strips:
        if s["level"] == 0 and s["nc"] >= 3:
            img[:, s["x0"] + s["wc"] - 3:s["x0"] + 2 * s["wc"] + 3] = 128
    return img


CAP_W, CAP_H = 150, 151      # level 0: three rows of three cells, 40 + 40 + 32 wide: one strip of 112 pixels per cell row


def cap_frame(npix, sparse=True):
    """a flat CAP_W x CAP_H frame with a checkerboard of 3 x 3 squares (every pixel of it passes the pre-test) over the first `npix` pixels, in raster order, of the
    first two cells of level 0's middle strip; the strip's third cell holds four single pixels (four corners) when `sparse`"""
    _, strips, cells = plan(CAP_W, CAP_H)
    s = [t for t in strips if t["level"] == 0][1]
    assert s["nc"] == 3
    yy, xx = np.mgrid[0:CAP_H, 0:CAP_W]
    pat = np.where(((xx // 3) + (yy // 3)) % 2 == 0, 20, 235).astype(np.uint8)
    m = np.zeros((CAP_H, CAP_W), bool)
    wide = 2 * s["wc"]
    rows, k = divmod(npix, wide)
    m[s["y0"]:s["y0"] + rows, s["x0"]:s["x0"] + wide] = True
    m[s["y0"] + rows, s["x0"]:s["x0"] + k] = True
    img = np.full((CAP_H, CAP_W), 128, np.uint8)
    img[m] = pat[m]
    if sparse:
        x, y = s["x0"] + 2 * s["wc"] + 10, s["y0"] + 10
        for k, v in enumerate((230, 150, 40, 200)): img[y + 5 * k, x + 4 * k] = v      # single pixels: each a corner of its own
    return img


ROW_WIDTHS = {"row1": 80, "rowK": 130, "rowK1": 160, "row2K1": 250}      # level-0 rows of 1, K, K + 1 and 2K + 1 cells (K = 3): (w - 32) / 30 = 1.6, 3.3, 4.3, 7.3

FRAMES = {
    "row1": lambda: synth_frame(31, w=80, h=97),
    "rowK": lambda: synth_frame(32, w=130, h=97),
    "rowK1": lambda: synth_frame(33, w=160, h=97),
    "row2K1": lambda: noise_frame(34, w=250, h=97),
    "small": lambda: synth_frame(4321, w=97, h=83),
    "bands": bands_frame,
    "noise320": lambda: noise_frame(35, w=320, h=240),
    "ini_min": ini_min_frame,
    "empty_between": empty_between_frame,
    "at_cap": lambda: cap_frame(AT_CAP_PIXELS),
    "cap_plus_1": lambda: cap_frame(AT_CAP_PIXELS + 1),
}
AT_CAP_PIXELS = 2489         # pattern pixels that give the strip exactly FAST_LIST_CAP survivors (searched once with the replay; the CPU test holds it)


@functools.lru_cache(maxsize=None)
def frame(name):
    img = FRAMES[name]()
    img.setflags(write=False)
    return img
