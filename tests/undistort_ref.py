"""fp64 restatement of Frame::UndistortKeyPoints / Frame::ComputeImageBounds (src/Frame.cc:483-543) for the tests: cv::undistortPoints(src, dst,
K, D, noArray(), K) as OpenCV 3.4's cvUndistortPoints computes it (DESIGN.md decision D13).  Every operation is a separate IEEE double
operation, left to right, exactly as the library's csrc/camera.h writes it; the rational / thin-prism terms k[5..13] are zero but are
written out all the same."""
import numpy as np

# (width, height, fx, fy, cx, cy, k1, k2, p1, p2, k3): the published TUM fr1 / fr2 and EuRoC models and three made-up ones
MODELS = {
    "tum_fr1": (640, 480, 517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314),
    "tum_fr2": (640, 480, 520.908620, 521.007327, 325.141442, 249.701764, 0.231222, -0.784899, -0.003257, -0.000105, 0.917205),
    "euroc": (752, 480, 458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0),
    "strong": (640, 480, 517.306408, 516.469215, 318.643040, 255.313989, 0.6, 0.0, -0.005358, 0.002628, 0.0),      # fr1's K, a stronger lens: its bounds
    # cut ~3 % of the area ORB detects in (TUM fr1's own bounds only cut the 16-pixel border FAST never reaches)
    "zero": (640, 480, 520.0, 520.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "k1_zero": (640, 480, 520.0, 520.0, 320.0, 240.0, 0.0, 0.1, 0.01, -0.02, 0.3),      # only k1 decides (src/Frame.cc:485, :517)
}


def camera_params(model):
    """the nine float32 values of sslam_camera (fx, fy, cx, cy, k1, k2, p1, p2, k3): the CV_32F K / DistCoef of src/Tracking.cc:48-72"""
    return tuple(np.float32(v) for v in MODELS[model][2:])


def undistort_points(params, u, v):
    """float32 arrays u, v -> float32 arrays u', v' (the identity rule on k1 is the caller's, as in the reference)"""
    fx, fy, cx, cy = (np.float64(p) for p in params[:4])
    k = np.zeros(14, np.float64)
    k[:5] = [np.float64(p) for p in params[4:9]]
    ifx = 1. / fx; ify = 1. / fy
    x = (np.asarray(u, np.float32).astype(np.float64) - cx) * ifx
    y = (np.asarray(v, np.float32).astype(np.float64) - cy) * ify
    x0 = x; y0 = y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - deltaX) * icdist
        y = (y0 - deltaY) * icdist
    return (fx * x + 0 * y + cx).astype(np.float32), (0 * x + fy * y + cy).astype(np.float32)


def undistort_keypoints(params, kp):
    """Frame::UndistortKeyPoints on a KP_DTYPE array: mvKeysUn"""
    out = kp.copy()
    if np.float32(params[4]) == 0:
        return out
    out["x"], out["y"] = undistort_points(params, kp["x"], kp["y"])
    return out


def image_bounds(params, w, h):
    """Frame::ComputeImageBounds: (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32"""
    if np.float32(params[4]) == 0:
        return (np.float32(0), np.float32(w), np.float32(0), np.float32(h))
    x, y = undistort_points(params, np.array([0, w, 0, w], np.float32), np.array([0, 0, h, h], np.float32))
    mn = lambda a, b: b if b < a else a          # std::min / std::max
    mx = lambda a, b: b if a < b else a
    return (mn(x[0], x[2]), mx(x[1], x[3]), mn(y[0], y[1]), mx(y[2], y[3]))


def distort_points(params, xu, yu):
    """the forward Brown-Conrady model (what undistortPoints inverts): undistorted pixels -> distorted pixels, fp64"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(p) for p in params)
    x = (np.asarray(xu, np.float64) - cx) / fx; y = (np.asarray(yu, np.float64) - cy) / fy
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd * fx + cx, yd * fy + cy
