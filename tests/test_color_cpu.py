"""CPU suite: the colour conversion of Tracking::GrabImageMonocularWithPL (src/Tracking.cc:146-161) -- the restatement tests/color_ref.py
(OpenCV 3.4's RGB2Gray<uchar> table form, DESIGN.md decision D14) and the declarations of the new entry points."""
import os, re
import numpy as np
import pytest
import pkg
import color_ref as cr

ROOT = pkg.ROOT
NEW_SYMBOLS = ("sslam_gray_from_color", "sslam_gray_from_color_batch_dev", "sslam_frontend_batch_color")


def test_coefficients_sum_to_one_and_grey_is_a_fixed_point():
    assert cr.WR + cr.WG + cr.WB == 1 << cr.SHIFT
    g = np.arange(256)
    np.testing.assert_array_equal(cr.gray_from_rgb(g, g, g), g.astype(np.uint8))
    for fmt in cr.COLOUR:
        np.testing.assert_array_equal(cr.to_gray(cr.grey_replicated(g[None], fmt), fmt)[0], g)


def test_rgb_and_bgr_are_mirror_images():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    np.testing.assert_array_equal(cr.to_gray(img, cr.PIX_RGB), cr.to_gray(img[..., ::-1], cr.PIX_BGR))
    np.testing.assert_array_equal(cr.to_gray(cr.from_rgb(img, cr.PIX_BGR), cr.PIX_BGR), cr.to_gray(img, cr.PIX_RGB))
    assert not np.array_equal(cr.to_gray(img, cr.PIX_RGB), cr.to_gray(img, cr.PIX_BGR))      # the order matters (R and B weigh 4899 and 1868)
    # known values: pure red, green, blue
    assert cr.gray_from_rgb(255, 0, 0) == 76 and cr.gray_from_rgb(0, 255, 0) == 150 and cr.gray_from_rgb(0, 0, 255) == 29


def test_alpha_is_ignored():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (29, 31, 3), dtype=np.uint8)
    for fmt4, fmt3 in ((cr.PIX_RGBA, cr.PIX_RGB), (cr.PIX_BGRA, cr.PIX_BGR)):
        want = cr.to_gray(cr.from_rgb(img, fmt3), fmt3)
        for alpha in (0, 255, rng.integers(0, 256, img.shape[:2], dtype=np.uint8)):
            np.testing.assert_array_equal(cr.to_gray(cr.from_rgb(img, fmt4, alpha), fmt4), want)


def test_restatement_is_the_exact_integer_formula():
    """against an independent float-free evaluation on every triple of a coarse grid, and the largest sum fits 32 bits"""
    v = np.arange(0, 256, 5)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    want = np.array([(4899 * int(x) + 9617 * int(y) + 1868 * int(z) + 8192) // 16384 for x, y, z in zip(r.ravel(), g.ravel(), b.ravel())])
    np.testing.assert_array_equal(cr.gray_from_rgb(r, g, b).ravel(), want)
    assert 255 * (cr.WR + cr.WG + cr.WB) + 8192 < 2 ** 32


def test_restatement_reproduces_the_icl_fixture():
    """icl_input_gray.npz is the ICL frame after this conversion; its colour source is not in the tree, so the grey replication stands in:
    every colour format of it converts back to the committed gray bytes"""
    gray = np.load(os.path.join(ROOT, "tests", "golden", "icl_input_gray.npz"))["gray"]
    assert gray.shape == (480, 640)
    for fmt in cr.COLOUR:
        np.testing.assert_array_equal(cr.to_gray(cr.grey_replicated(gray, fmt), fmt), gray)


def test_all_triples_frame():
    rgb = cr.all_triples_rgb()
    assert rgb.shape == (4096, 4096, 3)
    assert tuple(rgb[0, 0]) == (0, 0, 0) and tuple(rgb[-1, -1]) == (255, 255, 255) and tuple(rgb[0, 1]) == (0, 0, 1) and tuple(rgb[0, 256]) == (0, 1, 0) and tuple(rgb[16, 0]) == (1, 0, 0)


def test_new_symbols_are_declared_in_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sslam_frontend.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    for i, name in enumerate(("GRAY", "RGB", "BGR", "RGBA", "BGRA")):
        assert re.search(r"\bSSLAM_PIX_%s\s*=\s*%d\b" % (name, i), txt), name


def test_binding_constants_match_the_header():
    fe = pkg.frontend()
    assert (fe.PIX_GRAY, fe.PIX_RGB, fe.PIX_BGR, fe.PIX_RGBA, fe.PIX_BGRA) == (0, 1, 2, 3, 4)
    assert [fe.pix_format(c, rgb) for c, rgb in ((1, True), (3, True), (3, False), (4, True), (4, False))] == [0, 1, 2, 3, 4]


def test_new_entry_points_are_exported():
    import subprocess
    lib_path = pkg.builder().build(force=False, verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported
