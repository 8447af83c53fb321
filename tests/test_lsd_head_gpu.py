"""GPU: the line prologue (csrc/lsd_front.h) on its own output.  sslam_testing_lines_prologue (include/sslam_testing.h) runs lines_prepare, k_zero_misc and lines_prologue()
-- the product path's functions -- on the frames of tests/lsd_head_cases.py (whose reach tests/test_lsd_head_cases_cpu.py proves from the oracle alone) and copies back what
they leave for region growing: the T, S and Cs planes, Misc::maxS / nDefined and the ordered seed list, all of them filled with the byte 0xA5 before the launches.
sslam_testing_lines_grad_table copies back the 1021 x 1021 gradient table.  Everything is compared with the oracle's prologue (orc_lsd_prologue / orc_lsd_grad_table: the
per-pixel expressions the detector itself calls) as bit patterns: there is no tolerance here.

Per frame: T at EVERY pixel (the angle where defined, -1024.0f elsewhere, last row and column included; the sign bit -- region growing's `used` mark -- set exactly where
the pixel is undefined); S and Cs at defined pixels (elsewhere they are unspecified: the kernels write them for defined pixels only); maxS and nDefined; order[:nDefined] against
the oracle's list as x | y << 16; order[nDefined:] still the fill; words 2 and 3 of sslam_testing_lines_last_forms as the case claims."""
import numpy as np
import pytest
import lsd_cases
import lsd_head_cases as hc
from test_lsd_forms_gpu import _same_lines

pytestmark = pytest.mark.gpu

NOTDEF = np.float32(-1024.0)
FILL32 = np.uint32(0xA5A5A5A5)
_ORC = {}


def _oracle(oracle, name, resize=0, seed=0):
    """the oracle's prologue of a frame under the variants, computed once; the oracle's globals are restored whatever happens"""
    key = (name, resize, seed)
    if key not in _ORC:
        old = (oracle.set_lsd_resize(resize), oracle.set_lsd_seed_sort(seed))
        try:
            _ORC[key] = oracle.lsd_prologue(hc.frame(name))
        finally:
            oracle.set_lsd_resize(old[0]); oracle.set_lsd_seed_sort(old[1])
    return _ORC[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(got, want, tag, dense=False):
    """one frame of a tap call against the oracle's prologue.  dense: seed order 1, where S holds |g|^2 of every pixel with a gradient"""
    sw, sh = want["sw"], want["sh"]
    assert (got["sw"], got["sh"]) == (sw, sh), tag
    T, d = got["T"], want["deg"] != NOTDEF
    bad = np.argwhere(_bits(T) != _bits(want["deg"]))
    assert len(bad) == 0, (tag, "T", len(bad), [(int(y), int(x), float(T[y, x]), float(want["deg"][y, x])) for y, x in bad[:8]])
    assert (np.signbit(T) == ~d).all(), (tag, "sign bit of T")
    assert (got["max_s"], got["n_defined"]) == (want["max_s"], want["n_defined"]), (tag, "maxS, nDefined", got["max_s"], got["n_defined"], want["max_s"], want["n_defined"])
    bad = np.argwhere((got["S"] != want["S"]) & d)
    assert len(bad) == 0, (tag, "S", len(bad), [(int(y), int(x), int(got["S"][y, x]), int(want["S"][y, x])) for y, x in bad[:8]])
    bad = np.argwhere((_bits(got["Cs"]) != _bits(want["cs"])).any(axis=2) & d)
    assert len(bad) == 0, (tag, "Cs", len(bad), [(int(y), int(x), got["Cs"][y, x].tolist(), want["cs"][y, x].tolist()) for y, x in bad[:8]])
    if dense:
        np.testing.assert_array_equal(got["S"][:-1, :-1], want["S"][:-1, :-1], err_msg=tag + " S of every pixel with a gradient")
    n = want["n_defined"]
    o = want["order"].astype(np.int64)
    packed = ((o % sw) | ((o // sw) << 16)).astype(np.uint32)
    bad = np.nonzero(got["order"][:n] != packed)[0]
    assert len(bad) == 0, (tag, "order", len(bad), "first at", int(bad[0]), [(hex(int(got["order"][i])), hex(int(packed[i]))) for i in bad[:8]])
    assert (got["order"][n:] == FILL32).all(), (tag, "a seed stored at or past nDefined")


def _same_outputs(a, b, tag):
    """two tap calls left the same T plane and seed list, fill included, and the same S and Cs wherever they are specified (defined pixels)"""
    for k in ("T", "order"):
        assert (_bits(a[k]) == _bits(b[k])).all(), (tag, k)
    d = a["T"] != NOTDEF
    assert (a["S"][d] == b["S"][d]).all() and (_bits(a["Cs"])[d] == _bits(b["Cs"])[d]).all(), (tag, "S / Cs")
    assert (a["max_s"], a["n_defined"]) == (b["max_s"], b["n_defined"]), tag


@pytest.mark.parametrize("name", list(hc.CASES))
def test_case_against_the_oracle(fe, ctx, oracle, name):
    """every case in the default device layout, its forms asserted; a case whose geometry fuses once more with the first pixel one byte off a dword, which takes
    k_blur7 + k_lsd_grad: the same bytes"""
    img = hc.frame(name); want = _oracle(oracle, name)
    with fe.LinePrologue(ctx) as t:
        assert t.last_forms() == (None, None)
        got = t(img[None])[0]
        assert t.last_forms() == hc.forms(name), (name, t.last_forms())
        _check(got, want, name)
        if hc.forms(name)[0]:
            two = t(img[None], dev_offset=1)[0]
            assert t.last_forms() == (False, hc.forms(name)[1]), (name, t.last_forms())
            _check(two, want, name + " two kernels")
            _same_outputs(got, two, name + " fused against two kernels")


@pytest.mark.parametrize("name", ["noise_320x240", "tritri_640x60"])
def test_device_layouts(fe, ctx, oracle, name):
    """both gradient paths at the fused geometries 320 x 240 and 640 x 60: the default layout and rows exactly w apart fuse; a first pixel 1, 2 or 3 bytes off and a pitch
    that is no multiple of four take the two kernels; all six leave the same bytes"""
    img = hc.frame(name); want = _oracle(oracle, name); w = img.shape[1]
    with fe.LinePrologue(ctx) as t:
        base = t(img[None])[0]
        assert t.last_forms() == (True, True)
        _check(base, want, name)
        for pitch, off, fused in ((w, 0, True), (w + 3, 0, False), (0, 1, False), (0, 2, False), (0, 3, False), (w + 64, 3, False)):
            got = t(img[None], dev_pitch=pitch, dev_offset=off)[0]
            assert t.last_forms() == (fused, True), (pitch, off, t.last_forms())
            _same_outputs(base, got, "%s pitch %d offset %d" % (name, pitch, off))


VARIANTS = [          # resize variant, seed order, frame, device offsets: the template arguments 1, 2 and 3 of BOTH gradient kernels (0 is every other test)
    (1, 0, "noise_320x240", (0, 1)), (1, 0, "noise_333x251", (0,)),
    (0, 1, "noise_320x240", (0, 1)), (0, 1, "ramp_320x240", (0, 1)),
    (1, 1, "noise_320x240", (0, 1)), (1, 1, "noise_333x251", (0,)),
]


@pytest.mark.parametrize("resize,seed,name,offsets", VARIANTS, ids=["resize%d_seed%d_%s" % v[:3] for v in VARIANTS])
def test_variants(fe, ctx, oracle, resize, seed, name, offsets):
    """sslam_lines_set_resize_variant(1) (INTER_LINEAR) and sslam_lines_set_seed_order(1) (the host's std::sort over the keys the device computed: S of every pixel, word 3
    stays -1) against the oracle under the same variants, through the fused kernel and through the two kernels"""
    img = hc.frame(name); want = _oracle(oracle, name, resize, seed)
    if resize: assert (want["S"] != _oracle(oracle, name)["S"]).any()
    if seed: assert (want["order"] != _oracle(oracle, name, resize, 0)["order"]).any()
    with fe.LinePrologue(ctx) as t:
        t.set_resize_variant(resize); t.set_seed_order(seed)
        for off in offsets:
            got = t(img[None], dev_offset=off)[0]
            assert t.last_forms() == (hc.forms(name)[0] and off == 0, None if seed else hc.forms(name)[1]), (off, t.last_forms())
            _check(got, want, "%s resize %d seed order %d offset %d" % (name, resize, seed, off), dense=bool(seed))
        t.set_resize_variant(0); t.set_seed_order(0)          # and back: the plan is rebuilt, nothing of the variant stays
        _check(t(img[None])[0], _oracle(oracle, name), name + " after the variants")
        assert t.last_forms() == hc.forms(name)


def test_batch_of_nine_frames(fe, ctx, oracle):
    """ONE call, nine different 320 x 240 frames: the ninth is alone in the second round of sort_tile's mapping; every frame is binned by its own maxS and compared"""
    imgs = np.stack([hc.frame(n) for n in hc.BATCH9])
    with fe.LinePrologue(ctx) as t:
        out = t(imgs)
        assert t.last_forms() == (True, True)
        for n, got in zip(hc.BATCH9, out):
            _check(got, _oracle(oracle, n), "batch of nine, %s" % (n,))
        out = t(imgs, dev_offset=1)          # the same through k_blur7 + k_lsd_grad, whose grids walk the frames in z
        assert t.last_forms() == (False, True)
        for n, got in zip(hc.BATCH9, out):
            _check(got, _oracle(oracle, n), "batch of nine, two kernels, %s" % (n,))
    assert len({_oracle(oracle, n)["max_s"] for n in hc.BATCH9}) == 9


def test_state_between_calls_on_one_handle(fe, ctx, oracle):
    """noise, then a constant frame, then one square on ONE handle: the constant frame's maxS and nDefined are 0 (k_zero_misc), its seed list still holds the fill
    and every T pixel is -1024; the square after it is binned by its own maximum"""
    with fe.LinePrologue(ctx) as t:
        for name in ("noise_320x240", "const_320x240", "one_square_320x240", "const_320x240", "noise_320x240"):
            got = t(hc.frame(name)[None])[0]
            _check(got, _oracle(oracle, name), "sequence: " + name)
            if name == "const_320x240":
                assert (got["max_s"], got["n_defined"]) == (0, 0) and (got["T"] == NOTDEF).all()
                assert (got["order"] == FILL32).all()


def test_whole_gradient_table(fe, ctx, oracle):
    """all 1 042 441 entries of k_grad_table against orc_lsd_grad_table: angle, cos and sin bits, |g|^2, the defined test, and k_grad_smin's smallest defined |g|^2 -- read
    from a handle that has not planned a frame yet (the tap builds the table) and again after a call"""
    want, smin = oracle.lsd_grad_table()
    with fe.LinePrologue(ctx) as t:
        for when in ("fresh handle", "after a call"):
            tab, got_smin = t.grad_table()
            assert got_smin == smin, (when, got_smin, smin)
            np.testing.assert_array_equal(tab[..., 0] != NOTDEF, want[..., 0] != NOTDEF, err_msg=when + ": defined test")
            for k, what in enumerate(("angle", "cos", "sin", "|g|^2")):
                bad = np.argwhere(_bits(tab[..., k]) != _bits(want[..., k]))
                assert len(bad) == 0, (when, what, len(bad), [(int(gx) - 510, int(gy) - 510, float(tab[gy, gx, k]), float(want[gy, gx, k])) for gy, gx in bad[:8]])
            t(hc.frame("strokes_20x10")[None])


def test_extract_after_the_tap(fe, ctx, oracle):
    """the tap leaves the handle an ordinary one: sslam_lines_extract behind it, at another size and at the same size, equals the oracle"""
    img = lsd_cases.frame("head", (320, 240))
    o = oracle.lines_extract(img, 40)
    with fe.LinePrologue(ctx, 40) as t:
        for name in ("noise_333x251", "ramp_320x240"):
            _check(t(hc.frame(name)[None])[0], _oracle(oracle, name), name)
            kl, ld, fn, seg = t.extract(img)
            np.testing.assert_array_equal(seg, o[3], err_msg="segments after the tap on " + name)
            _same_lines(oracle, img, kl, ld, fn, o, "after the tap on " + name)
