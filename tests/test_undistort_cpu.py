"""CPU suite: the camera model of the C ABI (Frame::UndistortKeyPoints / Frame::ComputeImageBounds, src/Frame.cc:483-543) -- the sslam_camera
layout, the new exports, and the host-only bounds function against the fp64 restatement (tests/undistort_ref.py), bit for bit."""
import ctypes, os, subprocess
import numpy as np
import pytest
import pkg
import undistort_ref as ur

ROOT = pkg.ROOT
NEW_SYMBOLS = ("sslam_camera_image_bounds", "sslam_undistort_keypoints", "sslam_undistort_keypoints_batch_dev", "sslam_orb_set_camera",
               "sslam_frontend_batch_match_camera")


def _camera(fe, model):
    return fe.Camera(*[float(v) for v in ur.camera_params(model)])


def test_camera_struct_matches_the_header(tmp_path):
    fe = pkg.frontend()
    src = tmp_path / "cam.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "sslam_frontend.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\\n", sizeof(sslam_camera), offsetof(sslam_camera, cx), offsetof(sslam_camera, k1), offsetof(sslam_camera, p2),
           offsetof(sslam_camera, k3));
    return 0;
}
""")
    exe = tmp_path / "cam"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    Cm = fe.Camera
    assert got == [ctypes.sizeof(Cm), Cm.cx.offset, Cm.k1.offset, Cm.p2.offset, Cm.k3.offset] == [36, 8, 16, 28, 32]


def test_camera_entry_points_are_exported():
    lib_path = pkg.builder().build(force=False, verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported


@pytest.mark.parametrize("model", sorted(ur.MODELS))
def test_image_bounds_equal_the_restatement(model):
    fe = pkg.frontend()
    w, h = ur.MODELS[model][:2]
    got = fe.camera_image_bounds(_camera(fe, model), w, h)
    want = ur.image_bounds(ur.camera_params(model), w, h)
    assert np.array(got, np.float32).view(np.uint32).tolist() == np.array(want, np.float32).view(np.uint32).tolist(), (got, want)
    if model in ("zero", "k1_zero"):
        assert tuple(float(v) for v in got) == (0.0, float(w), 0.0, float(h))
    else:
        assert got != (0.0, float(w), 0.0, float(h))


def test_image_bounds_known_values():
    """the figures of the camera models quoted for this feature: TUM fr1 cuts a margin, EuRoC's barrel distortion widens the image"""
    fe = pkg.frontend()
    b = fe.camera_image_bounds(_camera(fe, "tum_fr1"), 640, 480)
    np.testing.assert_allclose(b, (10.8, 626.0, 14.7, 473.3), atol=0.1)
    b = fe.camera_image_bounds(_camera(fe, "euroc"), 752, 480)
    np.testing.assert_allclose(b, (-135.8, 895.5, -92.9, 565.6), atol=0.1)


def test_camera_arguments_are_checked():
    fe = pkg.frontend()
    with pytest.raises(fe.SslamError):
        fe.camera_image_bounds(fe.Camera(0, 500, 320, 240, 0.1), 640, 480)       # fx = 0
    with pytest.raises(fe.SslamError):
        fe.camera_image_bounds(_camera(fe, "tum_fr1"), -1, 480)


@pytest.mark.parametrize("model", ["tum_fr1", "tum_fr2", "euroc"])
def test_restatement_inverts_the_forward_model(model):
    """sanity check of the restatement itself (not of the library): redistorting the undistorted points with the forward Brown-Conrady model lands
    on the input -- within 0.3 px over the whole image (five iterations do not fully converge at the corners), 2e-3 px in its central half"""
    w, h = ur.MODELS[model][:2]
    P = ur.camera_params(model)
    gu, gv = np.meshgrid(np.linspace(0, w, 81, dtype=np.float32), np.linspace(0, h, 61, dtype=np.float32))
    u, v = gu.ravel(), gv.ravel()
    xu, yu = ur.undistort_points(P, u, v)
    xd, yd = ur.distort_points(P, xu, yu)
    err = np.hypot(xd - u, yd - v)
    assert err.max() < 0.3, err.max()
    central = (np.abs(u - w / 2) <= w / 4) & (np.abs(v - h / 2) <= h / 4)
    assert err[central].max() < 2e-3, err[central].max()
    moved = np.hypot(xu - u, yu - v)
    assert moved.max() > 5.0          # the models distort by pixels, not by rounding
