"""numpy restatement of the colour conversion of Tracking::GrabImageMonocularWithPL (src/Tracking.cc:146-161) for the tests: OpenCV 3.4's
8-bit RGB2Gray<uchar> in its fixed-point table form (DESIGN.md decision D14), gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 in exact integer
arithmetic -- the expression csrc/color.h writes and tests/golden/make_fixtures.py states.  The format names the byte order as stored; alpha
is ignored."""
import numpy as np

PIX_GRAY, PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA = 0, 1, 2, 3, 4
CHANNELS = {PIX_GRAY: 1, PIX_RGB: 3, PIX_BGR: 3, PIX_RGBA: 4, PIX_BGRA: 4}
COLOUR = (PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA)
NAMES = {PIX_GRAY: "gray", PIX_RGB: "rgb", PIX_BGR: "bgr", PIX_RGBA: "rgba", PIX_BGRA: "bgra"}
WR, WG, WB, SHIFT = 4899, 9617, 1868, 14


def gray_from_rgb(r, g, b):
    """integer arrays (any shape) -> uint8 gray"""
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    return ((WR * r + WG * g + WB * b + (1 << (SHIFT - 1))) >> SHIFT).astype(np.uint8)


def to_gray(img, fmt):
    """uint8 [..., h, w, cn] in fmt ([..., h, w] for PIX_GRAY) -> uint8 [..., h, w]"""
    if fmt == PIX_GRAY:
        return np.array(img, np.uint8)
    assert img.shape[-1] == CHANNELS[fmt]
    c0, c1, c2 = img[..., 0], img[..., 1], img[..., 2]
    return gray_from_rgb(c2, c1, c0) if fmt in (PIX_BGR, PIX_BGRA) else gray_from_rgb(c0, c1, c2)


def from_rgb(rgb, fmt, alpha=None):
    """uint8 [..., 3] RGB pixels -> the same pixels stored in fmt (alpha: a uint8 array / scalar for the 4-channel formats, default 255)"""
    rgb = np.asarray(rgb, np.uint8)
    if fmt in (PIX_BGR, PIX_BGRA):
        rgb = rgb[..., ::-1]
    if fmt in (PIX_RGB, PIX_BGR):
        return np.ascontiguousarray(rgb)
    a = np.broadcast_to(np.asarray(255 if alpha is None else alpha, np.uint8), rgb.shape[:-1])
    return np.ascontiguousarray(np.concatenate([rgb, a[..., None]], axis=-1))


def grey_replicated(gray, fmt):
    """R = G = B = gray in fmt: converts back to gray exactly (the coefficients sum to 1 << 14)"""
    return from_rgb(np.repeat(np.asarray(gray, np.uint8)[..., None], 3, axis=-1), fmt)


def all_triples_rgb():
    """every 24-bit RGB triple once, as one 4096 x 4096 RGB frame: pixel (y, x) = index y * 4096 + x = R << 16 | G << 8 | B"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
