"""Frames for the line PROLOGUE (csrc/lsd_front.h: k_blur7, k_lsd_grad, k_lsd_grad_fused, the gradient table, and the counting sort of the seeds in both forms), built by
numpy alone.  tests/test_lsd_head_cases_cpu.py proves from the oracle's own prologue (orc_lsd_prologue) what each frame reaches; tests/test_lsd_head_gpu.py reads the
library's planes and seed list back through sslam_testing_lines_prologue and compares them bit for bit.

Geometry the claims speak of (csrc/lsd_plan.h, lines_build_plan): the scaled image is sw x sh = round(0.8 w) x round(0.8 h); a SEGMENT is 256 pixels of one scaled row
(nXB = ceil(sw / 256) per row, one wave of the gradient kernels, one list of 256 slots); a TILE of the counting sort is tileRows = min(64, max(1, 8192 / sw)) whole rows;
the seeds are binned by int(sqrt(S / 4) * 1023 / sqrt(maxS / 4)), S = |g|^2, clamped to 1023."""
import functools
import numpy as np
import lsd_cases

N_BINS = 1024
TILE_PX = 8192          # csrc/lsd_plan.h
SEG_PX = 256
SORT_XY = 2048          # csrc/lsd_front.h SORT_XY_BITS: the tile-sorted runs pack x and y in 11 bits each; larger scaled images take k_lsd_hist + k_lsd_scatter


def geometry(w, h):
    """(sw, sh, nXB, tileRows, nTiles) as lines_build_plan computes them"""
    sw, sh = int(round(w * 0.8)), int(round(h * 0.8))
    tile_rows = min(64, max(1, TILE_PX // sw))
    return sw, sh, (sw + SEG_PX - 1) // SEG_PX, tile_rows, (sh + tile_rows - 1) // tile_rows


def fused_geometry(w, h):
    """lines_build_plan's condition for k_lsd_grad_fused (with the default blur taps and resize tables)"""
    sw, sh = int(round(w * 0.8)), int(round(h * 0.8))
    return w % 4 == 0 and sw % 4 == 0 and sh % 4 == 0 and w == 5 * (sw // 4) and h == 5 * (sh // 4) and w >= 20 and h >= 10


def _tri(n, slope=8, amp=120):
    """0, slope, 2 slope .. amp .. slope, 0, ...: a triangle wave"""
    half = amp // slope
    t = np.arange(n) % (2 * half)
    return slope * np.where(t <= half, t, 2 * half - t)


def tritri(w, h):
    """the sum of a triangle wave in x and one in y (slope 8, amplitude 120): a gradient above LSD's threshold at nearly every pixel"""
    return (_tri(w)[None, :] + _tri(h)[:, None]).astype(np.uint8)


def ramp(w, h):
    """(8 x) mod 256: one gradient value over the whole ramp and a second one at the wrap, so a handful of bins hold everything"""
    return np.broadcast_to(((8 * np.arange(w)) % 256).astype(np.uint8)[None, :], (h, w)).copy()


def noise(w, h, seed=1):
    """uniform bytes of Generator(PCG64(seed)): after the blur a smooth spread of gradient magnitudes, a few entries per bin"""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w), dtype=np.uint8)


def const(w, h, v=128):
    return np.full((h, w), v, np.uint8)


def one_square(w, h):
    """one 40 x 40 square of 200 on 60: a few hundred defined pixels on its outline, nothing elsewhere"""
    img = const(w, h, 60)
    img[h // 2 - 20:h // 2 + 20, w // 2 - 20:w // 2 + 20] = 200
    return img


def dot(w, h):
    """one 3 x 3 dot: fewer defined pixels than a wave has lanes"""
    img = const(w, h, 60)
    img[h // 2:h // 2 + 3, w // 3:w // 3 + 3] = 220
    return img


def flat_top(w, h, rows=40, seed=2):
    """noise in the lowest `rows` rows only: the leading counting-sort tiles are empty"""
    img = const(w, h, 128)
    img[h - rows:] = noise(w, rows, seed)
    return img


# name -> (generator, w, h).  What each must REACH is asserted case by case in
# tests/test_lsd_head_cases_cpu.py (the figures the oracle gave are written there next to the bounds).
CASES = {
    "tritri_640x60": (tritri, 640, 60),
    "tritri_330x40": (tritri, 330, 40),
    "tritri_645x60": (tritri, 645, 60),
    "ramp_320x240": (ramp, 320, 240),
    "noise_320x240": (noise, 320, 240),
    "noise_322x240": (noise, 322, 240),
    "noise_333x251": (noise, 333, 251),
    "noise_2570x13": (noise, 2570, 13),
    "const_320x240": (const, 320, 240),
    "one_square_320x240": (one_square, 320, 240),
    "dot_320x240": (dot, 320, 240),
    "flat_top_320x240": (flat_top, 320, 240),
}
# the head sizes of lsd_cases.HEADS at and around 10 x 10 and 20 x 10 (its strokes() frames)
SMALL = ((20, 10), (25, 10), (10, 10), (10, 40), (40, 10), (11, 13), (12, 12))
assert set(SMALL) <= set(lsd_cases.HEADS)
for _w, _h in SMALL:
    CASES["strokes_%dx%d" % (_w, _h)] = (lsd_cases.strokes, _w, _h)

# the batch of nine different 320 x 240 frames: one frame alone in the second round of sort_tile's mapping of frames to XCDs
BATCH9 = ("noise_320x240", "ramp_320x240", "const_320x240", "one_square_320x240", "flat_top_320x240", "dot_320x240", ("noise", 3), ("noise", 4), ("noise", 5))


def forms(name):
    """(fused gradient kernel, tile-sorted runs): words 2 and 3 of sslam_testing_lines_last_forms for the case in the default device layout"""
    _, w, h = CASES[name]
    sw, sh = geometry(w, h)[:2]
    return fused_geometry(w, h), sw <= SORT_XY and sh <= SORT_XY


@functools.lru_cache(maxsize=None)
def frame(name):
    """the frame of CASES[name], or of ("noise", seed) at 320 x 240: read-only, built once"""
    if isinstance(name, tuple):
        img = noise(320, 240, name[1])
    else:
        gen, w, h = CASES[name]
        img = gen(w, h)
    assert img.dtype == np.uint8
    img.setflags(write=False)
    return img


def bins(S, max_s):
    """the gradient bin of |g|^2 = S under the frame's largest defined |g|^2, in float64 as ll_angle computes it (independent of the C++)"""
    if max_s <= 0:
        return np.zeros(np.shape(S), np.int64)
    coef = 1023.0 / np.sqrt(max_s / 4.0)
    return np.minimum((np.sqrt(np.asarray(S, np.float64) / 4.0) * coef).astype(np.int64), N_BINS - 1)


def reach(p, w, h):
    """from an oracle prologue p (oracle_lib.Oracle.lsd_prologue) the figures the case claims are about -> dict"""
    sw, sh, nxb, tile_rows, ntiles = geometry(w, h)
    assert (p["sw"], p["sh"]) == (sw, sh)
    defined = p["deg"] != np.float32(-1024.0)
    seg_cnt = np.zeros((sh, nxb), np.int64)
    for k in range(nxb):
        seg_cnt[:, k] = defined[:, k * SEG_PX:(k + 1) * SEG_PX].sum(axis=1)
    tile_cnt = np.array([int(defined[t * tile_rows:(t + 1) * tile_rows].sum()) for t in range(ntiles)])
    b = bins(p["S"], p["max_s"])
    per_tile_bin_max = 0
    for t in range(ntiles):
        rows = slice(t * tile_rows, (t + 1) * tile_rows)
        bb = b[rows][defined[rows]]
        if len(bb): per_tile_bin_max = max(per_tile_bin_max, int(np.bincount(bb).max()))
    bd = b[defined]
    y = np.sqrt(p["S"][defined].astype(np.float64) / 4.0) * (1023.0 / np.sqrt(p["max_s"] / 4.0)) if p["max_s"] > 0 else np.zeros(0)
    near_int = int((np.abs(y - np.rint(y)) < 1e-3).sum())
    return dict(sw=sw, sh=sh, nxb=nxb, tile_rows=tile_rows, ntiles=ntiles, defined=int(defined.sum()), max_s=p["max_s"], seg_cnt=seg_cnt, tile_cnt=tile_cnt,
                full_segments=int((seg_cnt == SEG_PX).sum()), rows_with_full_segment=int((seg_cnt == SEG_PX).any(axis=1).sum()), distinct_bins=len(np.unique(bd)),
                per_tile_bin_max=per_tile_bin_max, clamp_bin=int((bd == N_BINS - 1).sum()), near_int=near_int)
