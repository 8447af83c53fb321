"""ctypes binding of libsslam_frontend.so (include/sslam_frontend.h) for the tests
and bench.py.  The product is the C-ABI library + the C++ shim in shim/; this module
is the harness-side view of the same entry points.  It never falls back to a CPU
path: loading fails loudly if the HIP library is missing, and every call raises on
a non-zero status."""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SSLAM_LIB") or os.path.join(HERE, "lib", "libsslam_frontend.so")      # SSLAM_LIB: kernel-variant experiments (tools/build_variant.sh)

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KL_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"),
                     ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                     ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"),
                     ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"),
                     ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                     ("lineLength", "<f4"), ("numOfPixels", "<i4")])
assert KP_DTYPE.itemsize == 28 and KL_DTYPE.itemsize == 68

PQ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                     ("angle", "<f4"), ("ur", "<f4"), ("valid", "<i4"), ("obs_positive", "<i4")])
assert PQ_DTYPE.itemsize == 44

TRI_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4")])      # sslam_tri_pair
assert TRI_PAIR_DTYPE.itemsize == 52

KF_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("invfx", "<f4"),
                          ("invfy", "<f4")])      # sslam_kf_pose
NEWMAP_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("median_depth2", "<f4")])      # sslam_newmap_pair
assert KF_POSE_DTYPE.itemsize == 84 and NEWMAP_PAIR_DTYPE.itemsize == 12

FUSE_JOB_DTYPE = np.dtype([("kf", "<i4"), ("nq", "<i4"), ("qdesc0", "<i4")])      # sslam_fuse_job
assert FUSE_JOB_DTYPE.itemsize == 12

OBS_DTYPE = np.dtype([("kf", "<i4"), ("row", "<i4")])      # sslam_observation
assert OBS_DTYPE.itemsize == 8

TWO_VIEW_RESULT_DTYPE = np.dtype([("nmatches", "<i4"), ("model", "<i4"), ("best_it_h", "<i4"), ("best_it_f", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"),
                                  ("rh", "<f4"), ("H21", "<f4", (9,)), ("F21", "<f4", (9,))])      # sslam_two_view_result
assert TWO_VIEW_RESULT_DTYPE.itemsize == 100
TWO_VIEW_POSE_DTYPE = np.dtype([("ok", "<i4"), ("reason", "<i4"), ("model", "<i4"), ("hypothesis", "<i4"), ("n_inliers", "<i4"), ("n_good", "<i4", (8,)),
                                ("parallax", "<f4", (8,)), ("R21", "<f4", (9,)), ("t21", "<f4", (3,)), ("n_triangulated", "<i4"), ("n_lines", "<i4"),
                                ("n_lines_triangulated", "<i4")])      # sslam_two_view_pose
assert TWO_VIEW_POSE_DTYPE.itemsize == 144

SIM3_STATE_DTYPE = np.dtype([("its_done", "<i4"), ("best_inliers", "<i4"), ("best_it", "<i4"), ("n", "<i4"), ("max_its", "<i4"), ("found_it", "<i4"), ("n_inliers", "<i4"),
                             ("no_more", "<i4"), ("s12", "<f4"), ("R12", "<f4", (9,)), ("t12", "<f4", (3,))])      # sslam_sim3_state
assert SIM3_STATE_DTYPE.itemsize == 84
PNP_STATE_DTYPE = np.dtype([("its_done", "<i4"), ("best_inliers", "<i4"), ("best_it", "<i4"), ("refine_ok", "<i4"), ("n", "<i4"), ("min_inliers", "<i4"), ("max_its", "<i4"),
                            ("found", "<i4"), ("found_it", "<i4"), ("n_inliers", "<i4"), ("no_more", "<i4"), ("pad_", "<i4"), ("best_R", "<f8", (9,)), ("best_t", "<f8", (3,)),
                            ("Tcw", "<f4", (12,))])      # sslam_pnp_state
assert PNP_STATE_DTYPE.itemsize == 192

_lib = None

PIX_GRAY, PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA = 0, 1, 2, 3, 4      # SSLAM_PIX_* (include/sslam_frontend.h)
PIX_CHANNELS = {PIX_GRAY: 1, PIX_RGB: 3, PIX_BGR: 3, PIX_RGBA: 4, PIX_BGRA: 4}


def pix_format(channels, rgb=True):
    """the SSLAM_PIX_* format Tracking::GrabImageMonocularWithPL converts with (src/Tracking.cc:146-161): channels 1, 3 or 4, rgb = mbRGB"""
    return {1: PIX_GRAY, 3: PIX_RGB if rgb else PIX_BGR, 4: PIX_RGBA if rgb else PIX_BGRA}[int(channels)]


def _image_layout(images, fmt, batch):
    """(n, h, w, row pitch, image stride) of a uint8 numpy array [n,] h, w[, cn] in fmt whose pixels are packed (rows and frames may be padded views)"""
    cn = PIX_CHANNELS[fmt]
    a = images if batch else images[None]
    assert a.dtype == np.uint8 and a.ndim == (3 if cn == 1 else 4) and (cn == 1 or a.shape[3] == cn), (a.dtype, a.shape, fmt)
    assert a.strides[2] == cn and (cn == 1 or a.strides[3] == 1), "pixels must be packed (rows and frames may be padded)"
    return a.shape[0], a.shape[1], a.shape[2], a.strides[1], a.strides[0]


SSLAM_ERR_INVALID, SSLAM_ERR_NO_DEVICE, SSLAM_ERR_CAPACITY, SSLAM_ERR_HIP, SSLAM_ERR_UNSUPPORTED = -1, -2, -3, -4, -5      # include/sslam_frontend.h:31-35


class SslamError(RuntimeError):
    """raised for every non-zero status of the C ABI; `code` is the status (SSLAM_ERR_*)"""
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SslamError("HIP library %s not built (run __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.sslam_status_str.restype = C.c_char_p
        _lib.sslam_last_error.restype = C.c_char_p
        _lib.sslam_ctx_stream.restype = C.c_void_p
    return _lib


TESTING_LIB_PATH = os.path.join(HERE, "lib", "libsslam_frontend_testing.so")
_testing = None


def testing_lib():
    """libsslam_frontend_testing.so: the product's sources compiled with -DSSLAM_TESTING -- every product entry point plus the self-tests, probes and the RCCL stand-in of
    include/sslam_testing.h.  The self-tests take a context handle; a handle made by the product library is fine (same structs, same HIP runtime)."""
    global _testing
    if _testing is None:
        if not os.path.exists(TESTING_LIB_PATH):
            raise SslamError("testing library %s not built (run __graft_entry__.build())" % TESTING_LIB_PATH)
        _testing = C.CDLL(TESTING_LIB_PATH)
        _testing.sslam_status_str.restype = C.c_char_p
        _testing.sslam_last_error.restype = C.c_char_p
        _testing.sslam_ctx_stream.restype = C.c_void_p
    return _testing


class use_testing_library:
    """with fe.use_testing_library(): every call of this binding goes to the testing library (what the group tests need: the stand-in for RCCL is bound when a group is
    CREATED, so the groups, contexts and extractors of such a test all live in that library).  Objects made inside must be closed inside."""
    def __enter__(self):
        global _lib
        lib(); self.prev = _lib; _lib = testing_lib()
        return _lib

    def __exit__(self, *a):
        global _lib
        _lib = self.prev


def _chk(rc):
    if rc != 0:
        L = lib()
        raise SslamError("%s: %s" % (L.sslam_status_str(rc).decode(), L.sslam_last_error().decode()), rc)


def _p(a):
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):          # torch tensor (device or host)
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(lib().sslam_ctx_create(int(device), C.byref(self.h)))

    def synchronize(self):
        _chk(lib().sslam_ctx_synchronize(self.h))

    @property
    def stream(self):
        return lib().sslam_ctx_stream(self.h)

    def close(self):
        if self.h:
            lib().sslam_ctx_destroy(self.h)
            self.h = C.c_void_p()

    # ---- Hamming ------------------------------------------------------------
    def hamming_knn2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        nq, nt = q.shape[0], t.shape[0]
        idx = np.full((nq, 2), -1, np.int32); dist = np.full((nq, 2), -1, np.int32)
        _chk(lib().sslam_hamming_knn2(self.h, _p(q), nq, _p(t), nt, _p(idx), _p(dist)))
        return idx, dist

    def hamming_matrix(self, q, t):
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        D = np.zeros((q.shape[0], t.shape[0]), np.uint16)
        _chk(lib().sslam_hamming_matrix(self.h, _p(q), q.shape[0], _p(t), t.shape[0], _p(D)))
        return D

    def search_for_initialization(self, kp1, d1, kp2, d2, prev_matched, window=100, nnratio=0.9,
                                  check_orientation=True, bounds=(0.0, 640.0, 0.0, 480.0)):
        kp1 = np.ascontiguousarray(kp1); kp2 = np.ascontiguousarray(kp2)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        pm = np.ascontiguousarray(prev_matched, np.float32).copy()
        m12 = np.full(len(kp1), -1, np.int32)
        n = C.c_int(0)
        b = (C.c_float * 4)(*bounds)
        _chk(lib().sslam_orb_search_for_initialization(self.h, _p(kp1), _p(d1), len(kp1), _p(kp2), _p(d2), len(kp2),
                                                       _p(pm), _p(m12), int(window), C.c_float(nnratio),
                                                       int(bool(check_orientation)), b, C.byref(n)))
        return m12, pm, n.value

    def two_view_ransac(self, kp1, kp2, matches12, sets=None, iterations=200, sigma=1.0, seed=0):
        """Initializer::Initialize's model selection (sslam_two_view_ransac) for one pair: kp1 / kp2 the undistorted keypoints (KP_DTYPE), matches12 [n1] int32, sets None
        (the library draws) or [iterations, 8] indices into the match list.  Returns (result: a TWO_VIEW_RESULT_DTYPE record, inliers: uint8 [n1])"""
        kp1 = np.ascontiguousarray(kp1, KP_DTYPE); kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
        m12 = np.ascontiguousarray(matches12, np.int32)
        assert len(m12) == len(kp1)
        if sets is not None:
            sets = np.ascontiguousarray(sets, np.int32)
            assert sets.shape == (int(iterations), 8)
        res = np.zeros(1, TWO_VIEW_RESULT_DTYPE); inl = np.zeros(len(kp1), np.uint8)
        _chk(lib().sslam_two_view_ransac(self.h, _p(kp1), len(kp1), _p(kp2), len(kp2), _p(m12), _p(sets), int(iterations), C.c_float(sigma), C.c_uint32(seed),
                                         _p(res), _p(inl)))
        return res[0], inl

    def two_view_ransac_batch_dev(self, d_kp1, d_n1, d_kp2, d_n2, cap, npairs, d_matches12, d_result, d_inliers, d_sets=None, iterations=200, sigma=1.0, seed=0,
                                  stream=None):
        """sslam_two_view_ransac_batch_dev on device tensors / pointers laid out like search_for_initialization_batch_dev's: pair p owns rows [p*cap, (p+1)*cap) of d_kp1,
        d_kp2, d_matches12 and d_inliers (uint8); d_result receives npairs TWO_VIEW_RESULT_DTYPE records (100 bytes each), d_sets is None or [npairs, iterations, 8] int32;
        enqueues on `stream` (None: the context's) and returns without synchronising"""
        _chk(lib().sslam_two_view_ransac_batch_dev(self.h, _p(d_kp1), _p(d_n1), _p(d_kp2), _p(d_n2), int(cap), int(npairs), _p(d_matches12), _p(d_sets), int(iterations),
                                                   C.c_float(sigma), C.c_uint32(seed), _p(d_result), _p(d_inliers), C.c_void_p(stream or 0)))

    def two_view_reconstruct(self, kp1, kp2, matches12, result, inliers, K, sigma=1.0, min_parallax=1.0, min_triangulated=50, lines=None):
        """The second half of Initializer::Initialize (sslam_two_view_reconstruct) for one pair: kp1 / kp2, matches12 as two_view_ransac took them, result / inliers as it
        returned them, K = (fx, fy, cx, cy).  lines: None or (kl1, kl2, linefn1, linefn2, line_pairs) with KL_DTYPE rows, float64 [nl, 3] functions and int32 [np, 2] pairs.
        Returns (pose: a TWO_VIEW_POSE_DTYPE record, p3d float32 [n1, 3], triangulated uint8 [n1]) and, with lines, (line_s3d, line_e3d float32 [np, 3],
        line_triangulated uint8 [np]) behind them"""
        kp1 = np.ascontiguousarray(kp1, KP_DTYPE); kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
        m12 = np.ascontiguousarray(matches12, np.int32); inl = np.ascontiguousarray(inliers, np.uint8)
        res = np.ascontiguousarray(np.asarray(result, TWO_VIEW_RESULT_DTYPE).reshape(1))
        assert len(m12) == len(kp1) == len(inl)
        Kf = np.ascontiguousarray(K, np.float32); assert Kf.shape == (4,)
        pose = np.zeros(1, TWO_VIEW_POSE_DTYPE); p3d = np.zeros((len(kp1), 3), np.float32); tri = np.zeros(len(kp1), np.uint8)
        la = [None, 0, None, 0, None, None, None, 0]; lo = [None, None, None]
        if lines is not None:
            kl1, kl2, f1, f2, lp = lines
            kl1 = np.ascontiguousarray(kl1, KL_DTYPE); kl2 = np.ascontiguousarray(kl2, KL_DTYPE)
            f1 = np.ascontiguousarray(f1, np.float64).reshape(-1, 3); f2 = np.ascontiguousarray(f2, np.float64).reshape(-1, 3)
            lp = np.ascontiguousarray(lp, np.int32).reshape(-1, 2)
            assert len(f1) == len(kl1) and len(f2) == len(kl2)
            pairs = lp if len(lp) else np.zeros((1, 2), np.int32)      # line_pairs != NULL is what says "with lines", also with no pair
            la = [kl1, len(kl1), kl2, len(kl2), f1, f2, pairs, len(lp)]
            lo = [np.zeros((len(lp), 3), np.float32), np.zeros((len(lp), 3), np.float32), np.zeros(len(lp), np.uint8)]
        ptr = lambda a: _p(a if a is not None and len(a) else None)      # an empty array travels as NULL
        _chk(lib().sslam_two_view_reconstruct(self.h, _p(kp1), len(kp1), _p(kp2), len(kp2), _p(m12), _p(res), _p(inl), _p(Kf), C.c_float(sigma), C.c_float(min_parallax),
                                              int(min_triangulated), ptr(la[0]), la[1], ptr(la[2]), la[3], ptr(la[4]), ptr(la[5]), _p(la[6]), la[7], _p(pose), _p(p3d),
                                              _p(tri), ptr(lo[0]), ptr(lo[1]), ptr(lo[2])))
        if lines is None:
            return pose[0], p3d, tri
        return pose[0], p3d, tri, lo[0], lo[1], lo[2]

    def two_view_reconstruct_batch_dev(self, d_kp1, d_n1, d_kp2, d_n2, cap, npairs, d_matches12, d_result, d_inliers, d_K, d_pose, d_p3d, d_triangulated,
                                       sigma=1.0, min_parallax=1.0, min_triangulated=50, lines=None, lcap=0, stream=None):
        """sslam_two_view_reconstruct_batch_dev on device tensors / pointers in two_view_ransac_batch_dev's layout, d_result and d_inliers as that call left them; d_K
        [npairs, 4] float32; d_pose receives npairs TWO_VIEW_POSE_DTYPE records (144 bytes each), d_p3d [npairs, cap, 3] float32, d_triangulated [npairs, cap] uint8.  lines:
        None or the eleven device arrays (d_kl1, d_nl1, d_kl2, d_nl2, d_linefn1, d_linefn2, d_line_pairs, d_line_npairs, d_line_s3d, d_line_e3d, d_line_triangulated) of
        capacity lcap.  Enqueues on `stream` (None: the context's) and returns without synchronising"""
        l = [None] * 11 if lines is None else list(lines)
        assert len(l) == 11
        _chk(lib().sslam_two_view_reconstruct_batch_dev(self.h, _p(d_kp1), _p(d_n1), _p(d_kp2), _p(d_n2), int(cap), int(npairs), _p(d_matches12), _p(d_result), _p(d_inliers),
                                                        _p(d_K), C.c_float(sigma), C.c_float(min_parallax), int(min_triangulated), _p(l[0]), _p(l[1]), _p(l[2]), _p(l[3]),
                                                        _p(l[4]), _p(l[5]), int(lcap), _p(l[6]), _p(l[7]), _p(d_pose), _p(d_p3d), _p(d_triangulated), _p(l[8]), _p(l[9]),
                                                        _p(l[10]), C.c_void_p(stream or 0)))

    def sim3_ransac(self, kp1, x3dc1, valid1, K1, kp2, x3dc2, valid2, K2, level_sigma2, matches12, state=None, fix_scale=False, probability=0.99, min_inliers=20,
                    max_iterations=300, new_iterations=5, sets=None, seed=0):
        """One iterate(new_iterations, ..) of a Sim3Solver (sslam_sim3_ransac) on one pair of keyframes: kp (KP_DTYPE: mvKeysUn), x3dc float32 [n, 3] (the map points in the
        camera frame), valid uint8 [n] or None (both or neither), K = fx fy cx cy, matches12 int32 [n1], state a SIM3_STATE_DTYPE record to resume (None: a new solver), sets
        None (the library draws) or [max_iterations, 3] indices into the correspondence list.  Returns (state: a SIM3_STATE_DTYPE record, inliers: uint8 [n1])"""
        kp1 = np.ascontiguousarray(kp1, KP_DTYPE); kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
        x1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3); x2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8); v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
        m12 = np.ascontiguousarray(matches12, np.int32)
        assert len(m12) == len(kp1) == len(x1) and len(kp2) == len(x2) and (v1 is None or len(v1) == len(kp1)) and (v2 is None or len(v2) == len(kp2))
        K1 = np.ascontiguousarray(K1, np.float32).reshape(4); K2 = np.ascontiguousarray(K2, np.float32).reshape(4)
        sig = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if sets is not None:
            sets = np.ascontiguousarray(sets, np.int32)
            assert sets.shape == (int(max_iterations), 3)
        st = np.zeros(1, SIM3_STATE_DTYPE)
        if state is not None:
            st[0] = state
        inl = np.zeros(len(kp1), np.uint8)
        _chk(lib().sslam_sim3_ransac(self.h, _p(kp1), _p(x1), _p(v1), len(kp1), _p(K1), _p(kp2), _p(x2), _p(v2), len(kp2), _p(K2), _p(sig), len(sig), _p(m12), int(bool(fix_scale)),
                                     C.c_double(probability), int(min_inliers), int(max_iterations), int(new_iterations), _p(sets), C.c_uint32(seed), _p(st), _p(inl)))
        return st[0], inl

    def sim3_ransac_batch_dev(self, d_kp, d_x3dc, d_valid, d_n, cap, nkeyframes, d_K, level_sigma2, d_pairs, npairs, d_matches12, d_state, d_inliers, fix_scale=False,
                              probability=0.99, min_inliers=20, max_iterations=300, new_iterations=5, d_sets=None, seed=0, stream=None, nlevels=None):
        """sslam_sim3_ransac_batch_dev on device tensors / pointers over the keyframe pool of search_by_bow_keyframes_batch_dev: slot k owns rows [k*cap, (k+1)*cap) of d_kp,
        d_valid (None: all valid) and d_x3dc (float32, 3 per row), d_K holds fx fy cx cy per slot, level_sigma2 is a HOST float32 array, pair p owns rows [p*cap, (p+1)*cap) of
        d_matches12 and d_inliers (uint8) and the SIM3_STATE_DTYPE record p of d_state (in/out, 84 bytes each), d_sets is None or [npairs, max_iterations, 3] int32; enqueues
        on `stream` (None: the context's) and returns without synchronising"""
        sig = None if level_sigma2 is None else np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        _chk(lib().sslam_sim3_ransac_batch_dev(self.h, _p(d_kp), _p(d_x3dc), _p(d_valid), _p(d_n), int(cap), int(nkeyframes), _p(d_K), _p(sig),
                                               int((0 if sig is None else len(sig)) if nlevels is None else nlevels), _p(d_pairs), int(npairs), _p(d_matches12), int(bool(fix_scale)),
                                               C.c_double(probability), int(min_inliers), int(max_iterations), int(new_iterations), _p(d_sets), C.c_uint32(seed), _p(d_state),
                                               _p(d_inliers), C.c_void_p(stream or 0)))

    def pnp_ransac(self, f_kp, f_K, kf_xw, kf_valid, level_sigma2, assigned, state=None, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991,
                   new_iterations=5, sets=None, seed=0):
        """One iterate(new_iterations, ..) of a PnPsolver (sslam_pnp_ransac) on one (keyframe, frame) pair: f_kp (KP_DTYPE: the frame's mvKeysUn), f_K = fx fy cx cy, kf_xw
        float32 [nkf, 3] (the world positions of the keyframe's map points), kf_valid uint8 [nkf] or None, assigned int32 [nf] (what SearchByBoW wrote), state a
        PNP_STATE_DTYPE record to resume (None: a new solver), sets None (the library draws) or [nsets, 4] indices into the correspondence list.  Returns (state: a
        PNP_STATE_DTYPE record, inliers: uint8 [nf])"""
        kp = np.ascontiguousarray(f_kp, KP_DTYPE)
        xw = np.ascontiguousarray(kf_xw, np.float32).reshape(-1, 3)
        v = None if kf_valid is None else np.ascontiguousarray(kf_valid, np.uint8)
        a = np.ascontiguousarray(assigned, np.int32)
        assert len(a) == len(kp) and (v is None or len(v) == len(xw))
        K = np.ascontiguousarray(f_K, np.float32).reshape(4)
        sig = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        nsets = 0
        if sets is not None:
            sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
            nsets = len(sets)
        st = np.zeros(1, PNP_STATE_DTYPE)
        if state is not None:
            st[0] = state
        inl = np.zeros(len(kp), np.uint8)
        _chk(lib().sslam_pnp_ransac(self.h, _p(kp), len(kp), _p(K), _p(xw), _p(v), len(xw), _p(sig), len(sig), _p(a), C.c_double(probability), int(min_inliers),
                                    int(max_iterations), C.c_float(epsilon), C.c_float(th2), int(new_iterations), _p(sets), int(nsets), C.c_uint32(seed), _p(st), _p(inl)))
        return st[0], inl

    def pnp_ransac_batch_dev(self, d_f_kp, d_nf, cap, nframes, d_f_K, d_kf_xw, d_kf_valid, d_nkf, kfcap, nkeyframes, level_sigma2, d_pair_kf, d_pair_f, npairs, d_assigned,
                             d_state, d_inliers, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, new_iterations=5, d_sets=None, nsets=0, seed=0,
                             stream=None, nlevels=None):
        """sslam_pnp_ransac_batch_dev on device tensors / pointers in the layout of search_by_bow_batch_dev: frame slot f owns rows [f*cap, (f+1)*cap) of d_f_kp and
        d_f_K[4f:4f+4], keyframe slot k rows [k*kfcap, (k+1)*kfcap) of d_kf_xw (float32, 3 per row) and d_kf_valid (None: all valid), level_sigma2 is a HOST float32 array,
        pair p owns rows [p*cap, (p+1)*cap) of d_assigned and d_inliers (uint8) and the PNP_STATE_DTYPE record p of d_state (in/out, 192 bytes each), d_sets is None or
        [npairs, nsets, 4] int32; enqueues on `stream` (None: the context's) and returns without synchronising"""
        sig = None if level_sigma2 is None else np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        _chk(lib().sslam_pnp_ransac_batch_dev(self.h, _p(d_f_kp), _p(d_nf), int(cap), int(nframes), _p(d_f_K), _p(d_kf_xw), _p(d_kf_valid), _p(d_nkf), int(kfcap), int(nkeyframes),
                                              _p(sig), int((0 if sig is None else len(sig)) if nlevels is None else nlevels), _p(d_pair_kf), _p(d_pair_f), int(npairs),
                                              _p(d_assigned), C.c_double(probability), int(min_inliers), int(max_iterations), C.c_float(epsilon), C.c_float(th2),
                                              int(new_iterations), _p(d_sets), int(nsets), C.c_uint32(seed), _p(d_state), _p(d_inliers), C.c_void_p(stream or 0)))

    def search_by_projection(self, kind, mode, feats, desc, queries, qdesc, occupied=None, uright=None, nnratio=0.8, th_dist=100,
                             check_orientation=True, bounds=(0.0, 640.0, 0.0, 480.0)):
        feats = np.ascontiguousarray(feats); desc = np.ascontiguousarray(desc, np.uint8)
        queries = np.ascontiguousarray(queries, PQ_DTYPE); qdesc = np.ascontiguousarray(qdesc, np.uint8)
        n = len(feats)
        assigned = np.full(n, -1, np.int32); nm = C.c_int(0)
        b = (C.c_float * 4)(*bounds)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        _chk(lib().sslam_search_by_projection(self.h, int(kind), int(mode), _p(feats), _p(desc), n, b, _p(ur), _p(occ), _p(queries), _p(qdesc),
                                              len(queries), C.c_float(nnratio), int(th_dist), int(bool(check_orientation)), _p(assigned), C.byref(nm)))
        return assigned, nm.value

    def search_by_projection_batch_dev(self, kind, mode, d_feats, d_desc, d_n, cap, nframes, d_queries, d_qdesc, d_nq, qcap, d_assigned, d_nmatches,
                                       d_occupied=None, d_uright=None, nnratio=0.8, th_dist=100, check_orientation=True, bounds=(0.0, 640.0, 0.0, 480.0),
                                       stream=None):
        """sslam_search_by_projection_batch_dev on device tensors / pointers laid out like the batch extractors' outputs (rows f*cap .. of the
        features, f*qcap .. of the queries); enqueues on `stream` (None: the context's) and returns without synchronising"""
        b = (C.c_float * 4)(*bounds)
        _chk(lib().sslam_search_by_projection_batch_dev(self.h, int(kind), int(mode), _p(d_feats), _p(d_desc), _p(d_n), int(cap), int(nframes), b,
                                                        _p(d_uright), _p(d_occupied), _p(d_queries), _p(d_qdesc), _p(d_nq), int(qcap), C.c_float(nnratio),
                                                        int(th_dist), int(bool(check_orientation)), _p(d_assigned), _p(d_nmatches), C.c_void_p(stream or 0)))

    def search_by_bow(self, kf_kp, kf_desc, kf_valid, f_kp, f_desc, ptr_kf, ptr_f, idx_kf, idx_f, nnratio=0.9, check_orientation=True):
        kf_kp = np.ascontiguousarray(kf_kp); f_kp = np.ascontiguousarray(f_kp)
        kf_desc = np.ascontiguousarray(kf_desc, np.uint8); f_desc = np.ascontiguousarray(f_desc, np.uint8)
        kf_valid = np.ascontiguousarray(kf_valid, np.uint8)
        ptr_kf = np.ascontiguousarray(ptr_kf, np.int32); ptr_f = np.ascontiguousarray(ptr_f, np.int32)
        idx_kf = np.ascontiguousarray(idx_kf, np.int32); idx_f = np.ascontiguousarray(idx_f, np.int32)
        assigned = np.full(len(f_kp), -1, np.int32); nm = C.c_int(0)
        _chk(lib().sslam_orb_search_by_bow(self.h, _p(kf_kp), _p(kf_desc), _p(kf_valid), len(kf_kp), _p(f_kp), _p(f_desc), len(f_kp), _p(ptr_kf),
                                           _p(ptr_f), len(ptr_kf) - 1, _p(idx_kf), _p(idx_f), C.c_float(nnratio), int(bool(check_orientation)),
                                           _p(assigned), C.byref(nm)))
        return assigned, nm.value

    def bow_transform_batch_dev(self, vocab, d_desc, d_n, cap, nframes, d_node, d_word=None, d_weight=None, levelsup=4, stream=None):
        """sslam_bow_transform_batch_dev on device tensors / pointers laid out like sslam_orb_extract_batch_dev's descriptors (rows f*cap ..): per valid
        row the node at level L - levelsup into d_node (int32) and, where given, the word into d_word (int32) and its weight into d_weight (float64);
        enqueues on `stream` (None: the context's) and returns without synchronising"""
        _chk(lib().sslam_bow_transform_batch_dev(self.h, vocab.h if vocab is not None else None, _p(d_desc), _p(d_n), int(cap), int(nframes), int(levelsup),
                                                 _p(d_word), _p(d_weight), _p(d_node), C.c_void_p(stream or 0)))

    def search_by_bow_batch_dev(self, d_kf_kp, d_kf_desc, d_kf_node, d_kf_valid, d_nkf, kfcap, nkeyframes, d_f_kp, d_f_desc, d_f_node, d_nf, cap, nframes,
                                npairs, d_assigned, d_nmatches, d_pair_kf=None, d_pair_f=None, nnratio=0.9, check_orientation=True, stream=None):
        """sslam_orb_search_by_bow_batch_dev on device tensors / pointers: pair p matches keyframe slot d_pair_kf[p] (None: p) against frame slot
        d_pair_f[p] (None: p) from the per-feature node ids of bow_transform_batch_dev; d_assigned [npairs, cap] int32, d_nmatches [npairs] int32;
        enqueues on `stream` (None: the context's) and returns without synchronising"""
        _chk(lib().sslam_orb_search_by_bow_batch_dev(self.h, _p(d_kf_kp), _p(d_kf_desc), _p(d_kf_node), _p(d_kf_valid), _p(d_nkf), int(kfcap), int(nkeyframes),
                                                     _p(d_f_kp), _p(d_f_desc), _p(d_f_node), _p(d_nf), int(cap), int(nframes), _p(d_pair_kf), _p(d_pair_f),
                                                     int(npairs), C.c_float(nnratio), int(bool(check_orientation)), _p(d_assigned), _p(d_nmatches),
                                                     C.c_void_p(stream or 0)))

    def search_by_bow_keyframes_batch_dev(self, d_kp, d_desc, d_node, d_n, cap, nkeyframes, d_pairs, npairs, d_matches12, d_matches21, d_nmatches,
                                          d_valid=None, nnratio=0.75, check_orientation=True, stream=None):
        """sslam_orb_search_by_bow_keyframes_batch_dev on device tensors / pointers: pair p matches keyframe slot d_pairs[2p] (pKF1, the side the result
        is indexed by) against slot d_pairs[2p+1] (pKF2) of the one pool d_kp / d_desc / d_node / d_n [/ d_valid] from the per-feature node ids of
        bow_transform_batch_dev; d_pairs [npairs, 2] int32, d_matches12 and d_matches21 [npairs, cap] int32, d_nmatches [npairs] int32; enqueues on
        `stream` (None: the context's) and returns without synchronising"""
        _chk(lib().sslam_orb_search_by_bow_keyframes_batch_dev(self.h, _p(d_kp), _p(d_desc), _p(d_node), _p(d_valid), _p(d_n), int(cap), int(nkeyframes),
                                                               _p(d_pairs), int(npairs), C.c_float(nnratio), int(bool(check_orientation)),
                                                               _p(d_matches12), _p(d_matches21), _p(d_nmatches), C.c_void_p(stream or 0)))

    def search_for_triangulation_batch_dev(self, d_kp, d_desc, d_node, d_n, cap, nkeyframes, d_pairs, npairs, scale_factors, level_sigma2,
                                           d_matches12, d_nmatches, d_free=None, d_uright=None, only_stereo=False, check_orientation=True, nlevels=None,
                                           stream=None):
        """sslam_orb_search_for_triangulation_batch_dev on device tensors / pointers: pair p = d_pairs[p] (TRI_PAIR_DTYPE rows on the device) matches
        keyframe slot kf1 (the queries) against slot kf2 of the one pool d_kp / d_desc / d_node / d_n [/ d_free / d_uright] from the per-feature node
        ids of bow_transform_batch_dev; scale_factors / level_sigma2 are HOST arrays (nlevels: their length unless given); d_matches12 [npairs, cap]
        int32, d_nmatches [npairs] int32; enqueues on `stream` (None: the context's) and returns without synchronising"""
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        sg = None if level_sigma2 is None else np.ascontiguousarray(level_sigma2, np.float32)
        if nlevels is None: nlevels = 0 if sf is None else len(sf)
        _chk(lib().sslam_orb_search_for_triangulation_batch_dev(self.h, _p(d_kp), _p(d_desc), _p(d_node), _p(d_free), _p(d_uright), _p(d_n), int(cap),
                                                                int(nkeyframes), _p(d_pairs), int(npairs), _p(sf), _p(sg), int(nlevels),
                                                                int(bool(only_stereo)), int(bool(check_orientation)), _p(d_matches12), _p(d_nmatches),
                                                                C.c_void_p(stream or 0)))

    def new_map_points_batch_dev(self, d_kp, d_n, cap, nkeyframes, d_pose, d_pairs, npairs, d_matches12, scale_factors, level_sigma2, scale_factor,
                                 d_x3d, d_stage, d_normal, d_dist, d_nnew, d_free=None, nlevels=None, stream=None):
        """sslam_new_map_points_batch_dev on device tensors / pointers: the loop body of CreateNewMapPoints for pair p = d_pairs[p] (NEWMAP_PAIR_DTYPE rows on the
        device) of the pool d_kp / d_n with d_pose (KF_POSE_DTYPE rows) on d_matches12 [npairs, cap] as search_for_triangulation_batch_dev left it; scale_factors /
        level_sigma2 are HOST arrays (nlevels: their length unless given), scale_factor is mfScaleFactor; d_x3d / d_normal [npairs, cap, 3] float32, d_stage
        [npairs, cap] uint8, d_dist [npairs, cap, 2] float32, d_nnew [npairs] int32; d_free (uint8 [nkeyframes, cap]) is cleared for created rows; enqueues on
        `stream` (None: the context's) and returns without synchronising"""
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        sg = None if level_sigma2 is None else np.ascontiguousarray(level_sigma2, np.float32)
        if nlevels is None: nlevels = 0 if sf is None else len(sf)
        _chk(lib().sslam_new_map_points_batch_dev(self.h, _p(d_kp), _p(d_n), int(cap), int(nkeyframes), _p(d_pose), _p(d_pairs), int(npairs), _p(d_matches12), _p(sf), _p(sg),
                                                  int(nlevels), C.c_float(scale_factor), _p(d_free), _p(d_x3d), _p(d_stage), _p(d_normal), _p(d_dist), _p(d_nnew),
                                                  C.c_void_p(stream or 0)))

    def new_map_lines_batch_dev(self, d_kl, d_linefn, d_nl, lcap, nkeyframes, d_pose, d_pairs, npairs, d_line_pairs, d_line_npairs, scale_factors,
                                d_s3d, d_e3d, d_stage, d_normal, d_dist, d_nnew, d_lfree=None, nlevels=None, stream=None):
        """sslam_new_map_lines_batch_dev on device tensors / pointers: the loop body of CreateNewMapLines2 for pair p = d_pairs[p] of the line pool d_kl (KL_DTYPE) /
        d_linefn (float64 [nkeyframes, lcap, 3]) / d_nl on rows [p, r] of d_line_pairs [npairs, lcap, 2] as line_match_batch_dev left them; scale_factors is a HOST
        array; d_s3d / d_e3d [npairs, lcap, 3] float32, d_stage [npairs, lcap] uint8, d_normal [npairs, lcap, 3] float64, d_dist [npairs, lcap, 2] float32, d_nnew
        [npairs] int32; d_lfree (uint8 [nkeyframes, lcap]) filters and is cleared for created rows; enqueues on `stream` and returns without synchronising"""
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        if nlevels is None: nlevels = 0 if sf is None else len(sf)
        _chk(lib().sslam_new_map_lines_batch_dev(self.h, _p(d_kl), _p(d_linefn), _p(d_nl), int(lcap), int(nkeyframes), _p(d_pose), _p(d_pairs), int(npairs), _p(d_line_pairs),
                                                 _p(d_line_npairs), _p(sf), int(nlevels), _p(d_lfree), _p(d_s3d), _p(d_e3d), _p(d_stage), _p(d_normal), _p(d_dist), _p(d_nnew),
                                                 C.c_void_p(stream or 0)))

    def new_map_points(self, kp1, kp2, pose1, pose2, matches12, scale_factors, level_sigma2, scale_factor, tap=False):
        """sslam_new_map_points for one host pair (tap: sslam_testing_new_map_points of the testing library, which also returns what the gates consumed): kp1 / kp2
        KP_DTYPE rows (mvKeysUn), pose1 / pose2 KF_POSE_DTYPE records, matches12 int32 [n1].  Returns dict(x3d, normal float32 [n1, 3], stage uint8 [n1], dist
        float32 [n1, 2], nnew) and, with tap, cos float32 [n1] and hom float32 [n1, 4]"""
        kp1 = np.ascontiguousarray(kp1, KP_DTYPE); kp2 = np.ascontiguousarray(kp2, KP_DTYPE); m12 = np.ascontiguousarray(matches12, np.int32)
        p1 = np.ascontiguousarray(np.asarray(pose1).view(KF_POSE_DTYPE).reshape(1)); p2 = np.ascontiguousarray(np.asarray(pose2).view(KF_POSE_DTYPE).reshape(1))
        sf = np.ascontiguousarray(scale_factors, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
        n1 = len(kp1)
        assert len(m12) == n1 and len(sf) == len(sg)
        o = dict(x3d=np.zeros((n1, 3), np.float32), stage=np.zeros(n1, np.uint8), normal=np.zeros((n1, 3), np.float32), dist=np.zeros((n1, 2), np.float32))
        nnew = C.c_int(0)
        ptr = lambda a: _p(a if len(a) else None)      # an empty array travels as NULL
        args = [self.h, ptr(kp1), n1, ptr(kp2), len(kp2), _p(p1), _p(p2), ptr(m12), _p(sf), _p(sg), len(sf), C.c_float(scale_factor), ptr(o["x3d"]), ptr(o["stage"]),
                ptr(o["normal"]), ptr(o["dist"]), C.byref(nnew)]
        if tap:
            o["cos"] = np.zeros(n1, np.float32); o["hom"] = np.zeros((n1, 4), np.float32)
            _chk(testing_lib().sslam_testing_new_map_points(*args, ptr(o["cos"]), ptr(o["hom"])))
        else:
            _chk(lib().sslam_new_map_points(*args))
        o["nnew"] = nnew.value
        return o

    def new_map_lines(self, kl1, linefn1, kl2, linefn2, pose1, pose2, median_depth2, line_pairs, scale_factors, tap=False):
        """sslam_new_map_lines for one host pair (tap: sslam_testing_new_map_lines): kl1 / kl2 KL_DTYPE rows, linefn1 / linefn2 float64 [nl, 3], line_pairs int32
        [nrows, 2].  Returns dict(s3d, e3d float32 [nrows, 3], stage uint8 [nrows], normal float64 [nrows, 3], dist float32 [nrows, 2], nnew) and, with tap, cos
        float32 [nrows] and hom float32 [nrows, 8] (s3D, e3D)"""
        kl1 = np.ascontiguousarray(kl1, KL_DTYPE); kl2 = np.ascontiguousarray(kl2, KL_DTYPE)
        f1 = np.ascontiguousarray(linefn1, np.float64).reshape(-1, 3); f2 = np.ascontiguousarray(linefn2, np.float64).reshape(-1, 3)
        lp = np.ascontiguousarray(line_pairs, np.int32).reshape(-1, 2)
        p1 = np.ascontiguousarray(np.asarray(pose1).view(KF_POSE_DTYPE).reshape(1)); p2 = np.ascontiguousarray(np.asarray(pose2).view(KF_POSE_DTYPE).reshape(1))
        sf = np.ascontiguousarray(scale_factors, np.float32)
        nr = len(lp)
        assert len(f1) == len(kl1) and len(f2) == len(kl2)
        o = dict(s3d=np.zeros((nr, 3), np.float32), e3d=np.zeros((nr, 3), np.float32), stage=np.zeros(nr, np.uint8), normal=np.zeros((nr, 3), np.float64),
                 dist=np.zeros((nr, 2), np.float32))
        nnew = C.c_int(0)
        ptr = lambda a: _p(a if len(a) else None)
        args = [self.h, ptr(kl1), ptr(f1), len(kl1), ptr(kl2), ptr(f2), len(kl2), _p(p1), _p(p2), C.c_float(median_depth2), ptr(lp), nr, _p(sf), len(sf), ptr(o["s3d"]),
                ptr(o["e3d"]), ptr(o["stage"]), ptr(o["normal"]), ptr(o["dist"]), C.byref(nnew)]
        if tap:
            o["cos"] = np.zeros(nr, np.float32); o["hom"] = np.zeros((nr, 8), np.float32)
            _chk(testing_lib().sslam_testing_new_map_lines(*args, ptr(o["cos"]), ptr(o["hom"])))
        else:
            _chk(lib().sslam_new_map_lines(*args))
        o["nnew"] = nnew.value
        return o

    def fuse_search_batch_dev(self, kind, chi2_mode, d_feats, d_desc, d_n, cap, nkeyframes, d_queries, qcap, d_qdesc, nqdesc, d_jobs, njobs,
                              d_best_idx, d_best_dist, d_nfound, d_uright=None, inv_level_sigma2=None, nlevels=None, bounds=(0.0, 640.0, 0.0, 480.0),
                              stream=None):
        """sslam_fuse_search_batch_dev on device tensors / pointers: job j = d_jobs[j] (FUSE_JOB_DTYPE rows on the device) searches keyframe slot kf of
        the pool d_feats / d_desc / d_n [/ d_uright] with the queries in rows j*qcap .. of d_queries (PQ_DTYPE) and the descriptors in rows qdesc0 .. of
        d_qdesc; inv_level_sigma2 is a HOST array (chi2_mode 1; nlevels: its length unless given); d_best_idx / d_best_dist [njobs, qcap] int32,
        d_nfound [njobs] int32; enqueues on `stream` (None: the context's) and returns without synchronising"""
        sg = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        if nlevels is None: nlevels = 0 if sg is None else len(sg)
        b = None if bounds is None else (C.c_float * 4)(*bounds)
        _chk(lib().sslam_fuse_search_batch_dev(self.h, int(kind), int(chi2_mode), _p(d_feats), _p(d_desc), _p(d_uright), _p(d_n), int(cap), int(nkeyframes),
                                               b, _p(sg), int(nlevels), _p(d_queries), int(qcap), _p(d_qdesc), int(nqdesc), _p(d_jobs), int(njobs),
                                               _p(d_best_idx), _p(d_best_dist), _p(d_nfound), C.c_void_p(stream or 0)))

    def search_by_bow_keyframes(self, kp1, d1, valid1, kp2, d2, valid2, ptr1, ptr2, idx1, idx2, nnratio=0.8, check_orientation=True):
        """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (src/ORBmatcher.cc:525-658): -> (matches12, nmatches)"""
        kp1 = np.ascontiguousarray(kp1); kp2 = np.ascontiguousarray(kp2)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        valid1 = np.ascontiguousarray(valid1, np.uint8); valid2 = np.ascontiguousarray(valid2, np.uint8)
        ptr1 = np.ascontiguousarray(ptr1, np.int32); ptr2 = np.ascontiguousarray(ptr2, np.int32)
        idx1 = np.ascontiguousarray(idx1, np.int32); idx2 = np.ascontiguousarray(idx2, np.int32)
        m12 = np.full(max(len(kp1), 1), -1, np.int32); nm = C.c_int(0)
        _chk(lib().sslam_orb_search_by_bow_keyframes(self.h, _p(kp1), _p(d1), _p(valid1), len(kp1), _p(kp2), _p(d2), _p(valid2), len(kp2), _p(ptr1), _p(ptr2),
                                                     len(ptr1) - 1, _p(idx1), _p(idx2), C.c_float(nnratio), int(bool(check_orientation)), _p(m12), C.byref(nm)))
        return m12[:len(kp1)], nm.value

    def distinctive_descriptors(self, desc, ptr):
        """MapPoint/MapLine::ComputeDistinctiveDescriptors for every set ptr[s]..ptr[s+1] (src/MapPoint.cc:247-312)."""
        desc = np.ascontiguousarray(desc, np.uint8); ptr = np.ascontiguousarray(ptr, np.int32)
        best = np.full(len(ptr) - 1, -2, np.int32)
        _chk(lib().sslam_distinctive_descriptors(self.h, _p(desc), _p(ptr), len(ptr) - 1, _p(best)))
        return best

    def distinctive_descriptors_batch_dev(self, d_desc, d_n, cap, nkeyframes, d_obs, nobs, d_ptr, nsets, d_best, d_median=None, d_kf_bad=None,
                                          d_out_desc=None, d_out_row=None, nout=0, stream=None):
        """sslam_distinctive_descriptors_batch_dev on device tensors / pointers: set s owns the entries d_obs[d_ptr[s] .. d_ptr[s+1]) (OBS_DTYPE rows on the
        device: keyframe slot, feature row) of the pool d_desc / d_n [/ d_kf_bad]; d_best [nsets] int32 receives the entry position of the chosen
        descriptor (-1: no admissible entry, -2: refused), d_median [nsets] int32 its median; a set with a choice copies the 32 bytes to row
        d_out_row[s] (None: s) of d_out_desc [nout, 32]; enqueues on `stream` (None: the context's) and returns without synchronising"""
        _chk(lib().sslam_distinctive_descriptors_batch_dev(self.h, _p(d_desc), _p(d_n), int(cap), int(nkeyframes), _p(d_kf_bad), _p(d_obs), int(nobs),
                                                           _p(d_ptr), int(nsets), _p(d_best), _p(d_median), _p(d_out_desc), _p(d_out_row), int(nout),
                                                           C.c_void_p(stream or 0)))

    def frame_upload(self, kind, feats, desc, uright=None, bounds=(0.0, 640.0, 0.0, 480.0)):
        return Frame(self, kind=kind, feats=feats, desc=desc, uright=uright, bounds=bounds)

    def line_match(self, l1, l2, gate_scale=0.5, ratio_mode=False):
        l1 = np.ascontiguousarray(l1, np.uint8); l2 = np.ascontiguousarray(l2, np.uint8)
        cap = max(len(l1), 1)
        pairs = np.zeros((cap, 2), np.int32)
        n = C.c_int(0); mad = C.c_double(0); mad12 = C.c_double(0)
        _chk(lib().sslam_line_match(self.h, _p(l1), len(l1), _p(l2), len(l2), C.c_double(gate_scale), int(bool(ratio_mode)),
                                    _p(pairs), cap, C.byref(n), C.byref(mad), C.byref(mad12)))
        return pairs[:n.value].copy(), mad.value, mad12.value

    # ---- camera model ---------------------------------------------------------
    def undistort_keypoints(self, cam, kp):
        """Frame::UndistortKeyPoints (sslam_undistort_keypoints): a copy of the keypoint records with pt.x / pt.y undistorted (mvKeysUn)"""
        kp = np.ascontiguousarray(kp, KP_DTYPE)
        out = np.empty_like(kp)
        _chk(lib().sslam_undistort_keypoints(self.h, C.byref(cam), _p(kp), len(kp), _p(out)))
        return out

    def undistort_keypoints_batch_dev(self, cam, d_kp, d_counts, nframes, cap, d_kp_un, stream=None):
        """sslam_undistort_keypoints_batch_dev on device buffers laid out like sslam_orb_extract_batch_dev's (d_kp_un may be d_kp)"""
        _chk(lib().sslam_undistort_keypoints_batch_dev(self.h, C.byref(cam), _p(d_kp), _p(d_counts), int(nframes), int(cap), _p(d_kp_un), C.c_void_p(stream or 0)))

    # ---- colour frames ----------------------------------------------------------
    def gray_from_color(self, img, order="rgb", out=None):
        """the cvtColor of Tracking::GrabImageMonocularWithPL (sslam_gray_from_color) on a numpy [h, w, 3|4] array (rows may be padded; [h, w]:
        a copy) whose bytes are in `order` ("rgb": RGB / RGBA, "bgr": BGR / BGRA).  out: a uint8 [h, >= w] array (its rows may be padded) that
        receives the gray rows in out[:, :w]; only those bytes are written.  Returns the [h, w] gray image."""
        assert order in ("rgb", "bgr")
        fmt = pix_format(img.shape[2] if img.ndim == 3 else 1, order == "rgb")
        _, h, w, stride, _ = _image_layout(img, fmt, False)
        if out is None:
            out = np.empty((h, w), np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] == h and out.shape[1] >= w and out.strides[1] == 1
        _chk(lib().sslam_gray_from_color(self.h, fmt, _p(img), w, h, C.c_size_t(stride), _p(out), C.c_size_t(out.strides[0])))
        return out[:, :w]

    def gray_from_color_batch_dev(self, fmt, d_src, w, h, pitch, image_stride, nframes, d_gray, gray_pitch, gray_image_stride, stream=None):
        """sslam_gray_from_color_batch_dev on device pointers / tensors (byte pitches and strides)"""
        _chk(lib().sslam_gray_from_color_batch_dev(self.h, int(fmt), _p(d_src), int(w), int(h), C.c_size_t(pitch), C.c_size_t(image_stride), int(nframes),
                                                   _p(d_gray), C.c_size_t(gray_pitch), C.c_size_t(gray_image_stride), C.c_void_p(stream or 0)))


class Vocabulary:
    """Device-resident DBoW2 vocabulary tree (sslam_vocab_*): CSR children lists in DBoW2's node numbering."""

    def __init__(self, ctx, levels, child_ptr, children, node_desc, word_id, weight):
        self.ctx = ctx
        self.h = C.c_void_p()
        child_ptr = np.ascontiguousarray(child_ptr, np.int32); children = np.ascontiguousarray(children, np.int32)
        node_desc = np.ascontiguousarray(node_desc, np.uint8); word_id = np.ascontiguousarray(word_id, np.int32)
        weight = np.ascontiguousarray(weight, np.float64)
        _chk(lib().sslam_vocab_create(ctx.h, len(child_ptr) - 1, int(levels), _p(child_ptr), _p(children), _p(node_desc), _p(word_id), _p(weight), C.byref(self.h)))

    @classmethod
    def from_text_file(cls, ctx, path):
        """ORBVocabulary::loadFromTextFile (src/System.cc:64-73): an ORBvoc.txt-format file -> device-resident tree"""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.h = C.c_void_p()
        _chk(lib().sslam_vocab_load_text(ctx.h, str(path).encode(), C.byref(self.h)))
        return self

    def info(self):
        v = [C.c_int() for _ in range(6)]
        _chk(lib().sslam_vocab_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("k", "levels", "scoring", "weighting", "nnodes", "nwords"), (x.value for x in v)))

    def set_types(self, weighting=0, scoring=0):
        _chk(lib().sslam_vocab_set_types(self.h, int(weighting), int(scoring)))

    def compute_bow(self, desc, levelsup=4):
        """Frame::ComputeBoW (src/Frame.cc:474-481): -> (BowVector as {word: value}, FeatureVector as {node: [feature indices]}), both in key order"""
        if isinstance(desc, Frame):
            n = len(desc)
        else:
            desc = np.ascontiguousarray(desc, np.uint8); n = len(desc)
        m = max(n, 1)
        bw = np.zeros(m, np.int32); bv = np.zeros(m, np.float64); fn = np.zeros(m, np.int32); fp = np.zeros(n + 1, np.int32); ff = np.zeros(m, np.int32)
        nb, nf = C.c_int(), C.c_int()
        if isinstance(desc, Frame):
            _chk(lib().sslam_compute_bow_frame(self.ctx.h, self.h, desc.h, int(levelsup), _p(bw), _p(bv), C.byref(nb), _p(fn), _p(fp), _p(ff), C.byref(nf)))
        else:
            _chk(lib().sslam_compute_bow(self.ctx.h, self.h, _p(desc), n, int(levelsup), _p(bw), _p(bv), C.byref(nb), _p(fn), _p(fp), _p(ff), C.byref(nf)))
        bow = {int(bw[i]): float(bv[i]) for i in range(nb.value)}
        fv = {int(fn[j]): ff[fp[j]:fp[j + 1]].tolist() for j in range(nf.value)}
        return bow, fv

    def transform(self, desc, levelsup=4):
        """per feature: (word id, word weight, node at level L - levelsup) -- Frame::ComputeBoW's device part"""
        if isinstance(desc, Frame):
            n = len(desc)
            w = np.zeros(n, np.int32); v = np.zeros(n, np.float64); nd = np.zeros(n, np.int32)
            _chk(lib().sslam_bow_transform_frame(self.ctx.h, self.h, desc.h, int(levelsup), _p(w), _p(v), _p(nd)))
            return w, v, nd
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        w = np.zeros(n, np.int32); v = np.zeros(n, np.float64); nd = np.zeros(n, np.int32)
        _chk(lib().sslam_bow_transform(self.ctx.h, self.h, _p(desc), n, int(levelsup), _p(w), _p(v), _p(nd)))
        return w, v, nd

    def close(self):
        if self.h:
            lib().sslam_vocab_destroy(self.h); self.h = C.c_void_p()


class Frame:
    """Device-resident features of one Frame (sslam_frame_*): upload once, or snapshot what an extractor just produced."""

    def __init__(self, ctx, kind=0, feats=None, desc=None, uright=None, bounds=(0.0, 640.0, 0.0, 480.0), orb=None, lines=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        b = (C.c_float * 4)(*bounds)
        if orb is not None:
            _chk(lib().sslam_frame_from_orb(orb.h, b, C.byref(self.h)))
        elif lines is not None:
            _chk(lib().sslam_frame_from_lines(lines.h, b, C.byref(self.h)))
        else:
            feats = np.ascontiguousarray(feats); desc = np.ascontiguousarray(desc, np.uint8)
            ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
            _chk(lib().sslam_frame_upload(ctx.h, int(kind), _p(feats), _p(desc), len(feats), _p(ur), b, C.byref(self.h)))

    def __len__(self):
        return int(lib().sslam_frame_count(self.h))

    def search_by_projection(self, mode, queries, qdesc, occupied=None, nnratio=0.8, th_dist=100, check_orientation=True):
        queries = np.ascontiguousarray(queries, PQ_DTYPE); qdesc = np.ascontiguousarray(qdesc, np.uint8)
        n = len(self)
        assigned = np.full(n, -1, np.int32); nm = C.c_int(0)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        _chk(lib().sslam_search_by_projection_frame(self.ctx.h, self.h, int(mode), _p(occ), _p(queries), _p(qdesc), len(queries),
                                                    C.c_float(nnratio), int(th_dist), int(bool(check_orientation)), _p(assigned), C.byref(nm)))
        return assigned, nm.value

    def fuse_search(self, queries, qdesc, chi2_mode=0, inv_level_sigma2=None):
        """candidate search of ORBmatcher::Fuse / LSDmatcher::Fuse on this (key)frame: (best_idx, best_dist) per query"""
        queries = np.ascontiguousarray(queries, PQ_DTYPE); qdesc = np.ascontiguousarray(qdesc, np.uint8)
        sg = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        bi = np.zeros(len(queries), np.int32); bd = np.zeros(len(queries), np.int32)
        _chk(lib().sslam_fuse_search(self.ctx.h, self.h, int(chi2_mode), _p(sg), 0 if sg is None else len(sg), _p(queries), _p(qdesc), len(queries), _p(bi), _p(bd)))
        return bi, bd

    def search_for_triangulation(self, kf2, free1, free2, ptr1, ptr2, idx1, idx2, F12, ex, ey, scale_factors2, level_sigma2_2,
                                 only_stereo=False, check_orientation=True):
        """ORBmatcher::SearchForTriangulation(this, kf2, F12, ...) -> (vMatches12, nmatches)"""
        f1 = np.ascontiguousarray(free1, np.uint8); f2 = np.ascontiguousarray(free2, np.uint8)
        ptr1 = np.ascontiguousarray(ptr1, np.int32); ptr2 = np.ascontiguousarray(ptr2, np.int32)
        idx1 = np.ascontiguousarray(idx1, np.int32); idx2 = np.ascontiguousarray(idx2, np.int32)
        F = (C.c_float * 9)(*np.asarray(F12, np.float32).reshape(9).tolist())
        sf = np.ascontiguousarray(scale_factors2, np.float32); sg = np.ascontiguousarray(level_sigma2_2, np.float32)
        m12 = np.full(len(self), -2, np.int32); nm = C.c_int(0)
        _chk(lib().sslam_orb_search_for_triangulation(self.ctx.h, self.h, kf2.h, _p(f1), _p(f2), _p(ptr1), _p(ptr2), len(ptr1) - 1, _p(idx1), _p(idx2),
                                                      F, C.c_float(ex), C.c_float(ey), _p(sf), _p(sg), len(sf), int(bool(only_stereo)),
                                                      int(bool(check_orientation)), _p(m12), C.byref(nm)))
        return m12, nm.value

    def knn2(self, train):
        n = len(self)
        idx = np.full((n, 2), -1, np.int32); dist = np.full((n, 2), -1, np.int32)
        _chk(lib().sslam_hamming_knn2_frames(self.ctx.h, self.h, train.h, _p(idx), _p(dist)))
        return idx, dist

    def close(self):
        if self.h:
            lib().sslam_frame_destroy(self.h); self.h = C.c_void_p()


def frontend_batch_alloc(n, cap, lcap, pinned=False):
    """result arrays of sslam_frontend_batch for n frames (pinned=True: in pinned memory, so that the library copies straight into them);
    pageable arrays are touched once so that a timed call does not pay their first page faults"""
    def alloc(shape, dt):
        if not pinned:
            a = np.empty(shape, dt); a.view(np.uint8).reshape(-1)[::4096] = 0
            return a
        import torch
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True).numpy()[:nbytes].view(dt).reshape(shape)
    return (alloc((n, cap), KP_DTYPE), alloc((n, cap, 32), np.uint8), alloc((n,), np.int32),
            alloc((n, lcap), KL_DTYPE), alloc((n, lcap, 32), np.uint8), alloc((n, lcap, 3), np.float64), alloc((n,), np.int32))


def frontend_batch_raw(orb, lines, images, out, chunk=0, lcap=None):
    """sslam_frontend_batch into arrays from frontend_batch_alloc: the bare library call (what the PCIe-inclusive measurements time)"""
    n, h, w = images.shape
    kp, desc, nk, kl, ld, fn, nl = out
    lcap = int(lcap if lcap is not None else kl.shape[1])
    _chk(lib().sslam_frontend_batch(orb.h, lines.h if lines is not None else None, _p(images), n, w, h, C.c_size_t(w), C.c_size_t(w * h), int(chunk),
                                    _p(kp), _p(desc), _p(nk), orb.cap, _p(kl), _p(ld), _p(fn), _p(nl), lcap))
    return out


class BatchMatch(C.Structure):
    """sslam_batch_match (include/sslam_frontend.h)"""
    _fields_ = [("window_size", C.c_int32), ("nnratio", C.c_float), ("check_orientation", C.c_int32), ("bounds", C.c_float * 4),
                ("line_gate_scale", C.c_double), ("line_ratio_mode", C.c_int32),
                ("init_matches12", C.c_void_p), ("init_nmatches", C.c_void_p), ("knn_idx", C.c_void_p), ("knn_dist", C.c_void_p),
                ("line_pairs", C.c_void_p), ("line_npairs", C.c_void_p)]


def frontend_batch_match_alloc(n, cap, lcap, pinned=False, knn=True):
    """the match-stage arrays of sslam_frontend_batch_match: (init_matches12, init_nmatches, knn_idx, knn_dist, line_pairs, line_npairs)"""
    def alloc(shape, dt):
        if not pinned:
            a = np.empty(shape, dt); a.view(np.uint8).reshape(-1)[::4096] = 0
            return a
        import torch
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True).numpy()[:nbytes].view(dt).reshape(shape)
    return (alloc((n, cap), np.int32), alloc((n,), np.int32), alloc((n, cap, 2), np.int32) if knn else None, alloc((n, cap, 2), np.int32) if knn else None,
            alloc((n, lcap, 2), np.int32), alloc((n,), np.int32))


def frontend_batch_match_raw(orb, lines, images, out, mout, chunk=0, window=100, nnratio=0.9, check_orientation=True, bounds=None, line_gate_scale=0.5, line_ratio_mode=False):
    """sslam_frontend_batch_match into arrays from frontend_batch_alloc / frontend_batch_match_alloc: frame i is matched against frame i-1"""
    n, h, w = images.shape
    kp, desc, nk, kl, ld, fn, nl = out
    m12, nm, ki, kd, lp, nlp = mout
    M = BatchMatch()
    M.window_size = int(window); M.nnratio = float(nnratio); M.check_orientation = int(bool(check_orientation))
    M.bounds = (C.c_float * 4)(*(bounds if bounds is not None else (0.0, float(w), 0.0, float(h))))
    M.line_gate_scale = float(line_gate_scale); M.line_ratio_mode = int(bool(line_ratio_mode))
    vp = lambda a: a.ctypes.data if a is not None else None
    M.init_matches12 = vp(m12); M.init_nmatches = vp(nm); M.knn_idx = vp(ki); M.knn_dist = vp(kd); M.line_pairs = vp(lp); M.line_npairs = vp(nlp)
    _chk(lib().sslam_frontend_batch_match(orb.h, lines.h if lines is not None else None, _p(images), n, w, h, C.c_size_t(w), C.c_size_t(w * h), int(chunk),
                                          _p(kp), _p(desc), _p(nk), orb.cap, _p(kl), _p(ld), _p(fn), _p(nl), int(kl.shape[1]), C.byref(M)))
    return out, mout


class Camera(C.Structure):
    """sslam_camera (include/sslam_frontend.h): K and DistCoef as Tracking::Tracking reads them (src/Tracking.cc:48-72); k3 = 0 when absent"""
    _fields_ = [(f, C.c_float) for f in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


def camera_image_bounds(cam, w, h):
    """Frame::ComputeImageBounds (sslam_camera_image_bounds, host-only): (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32 values"""
    b = (C.c_float * 4)()
    _chk(lib().sslam_camera_image_bounds(C.byref(cam), int(w), int(h), b))
    return tuple(np.float32(v) for v in b)


def frontend_batch_camera_alloc(n, cap, lcap, pinned=False):
    """the result arrays of sslam_frontend_batch_match_camera: frontend_batch_alloc's seven plus kpun[n, cap] (mvKeysUn)"""
    if not pinned:
        kpun = np.empty((n, cap), KP_DTYPE); kpun.view(np.uint8).reshape(-1)[::4096] = 0
    else:
        import torch
        nbytes = n * cap * KP_DTYPE.itemsize
        kpun = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True).numpy()[:nbytes].view(KP_DTYPE).reshape(n, cap)
    return frontend_batch_alloc(n, cap, lcap, pinned=pinned) + (kpun,)


def frontend_batch_match_camera_raw(orb, lines, cam, images, out, mout=None, chunk=0, window=100, nnratio=0.9, check_orientation=True, bounds=None,
                                    line_gate_scale=0.5, line_ratio_mode=False):
    """sslam_frontend_batch_match_camera into arrays from frontend_batch_camera_alloc (and frontend_batch_match_alloc, or mout=None for no match
    stage); bounds default to camera_image_bounds(cam, w, h), what the frame's mnMinX .. mnMaxY are"""
    n, h, w = images.shape
    kp, desc, nk, kl, ld, fn, nl, kpun = out
    M = None
    if mout is not None:
        m12, nm, ki, kd, lp, nlp = mout
        M = BatchMatch()
        M.window_size = int(window); M.nnratio = float(nnratio); M.check_orientation = int(bool(check_orientation))
        M.bounds = (C.c_float * 4)(*(bounds if bounds is not None else camera_image_bounds(cam, w, h)))
        M.line_gate_scale = float(line_gate_scale); M.line_ratio_mode = int(bool(line_ratio_mode))
        vp = lambda a: a.ctypes.data if a is not None else None
        M.init_matches12 = vp(m12); M.init_nmatches = vp(nm); M.knn_idx = vp(ki); M.knn_dist = vp(kd); M.line_pairs = vp(lp); M.line_npairs = vp(nlp)
    _chk(lib().sslam_frontend_batch_match_camera(orb.h, lines.h if lines is not None else None, C.byref(cam), _p(images), n, w, h, C.c_size_t(w),
                                                 C.c_size_t(w * h), int(chunk), _p(kp), _p(kpun), _p(desc), _p(nk), orb.cap, _p(kl), _p(ld), _p(fn), _p(nl),
                                                 int(kl.shape[1]), C.byref(M) if M is not None else None))
    return out, mout


def frontend_batch_color_raw(orb, lines, fmt, images, out, mout=None, cam=None, chunk=0, window=100, nnratio=0.9, check_orientation=True, bounds=None,
                             line_gate_scale=0.5, line_ratio_mode=False):
    """sslam_frontend_batch_color: images = uint8 [n, h, w, cn] in fmt (SSLAM_PIX_*; [n, h, w] for PIX_GRAY) in HOST memory, rows and frames
    may be padded views.  out: frontend_batch_alloc's seven arrays, or frontend_batch_camera_alloc's eight with a Camera; mout:
    frontend_batch_match_alloc's six or None (no match stage).  bounds default to the camera's (or the whole image)."""
    n, h, w, stride, image_stride = _image_layout(images, fmt, True)
    kp, desc, nk, kl, ld, fn, nl = out[:7]
    kpun = out[7] if cam is not None else None
    M = None
    if mout is not None:
        m12, nm, ki, kd, lp, nlp = mout
        M = BatchMatch()
        M.window_size = int(window); M.nnratio = float(nnratio); M.check_orientation = int(bool(check_orientation))
        if bounds is None:
            bounds = camera_image_bounds(cam, w, h) if cam is not None else (0.0, float(w), 0.0, float(h))
        M.bounds = (C.c_float * 4)(*bounds)
        M.line_gate_scale = float(line_gate_scale); M.line_ratio_mode = int(bool(line_ratio_mode))
        vp = lambda a: a.ctypes.data if a is not None else None
        M.init_matches12 = vp(m12); M.init_nmatches = vp(nm); M.knn_idx = vp(ki); M.knn_dist = vp(kd); M.line_pairs = vp(lp); M.line_npairs = vp(nlp)
    _chk(lib().sslam_frontend_batch_color(orb.h, lines.h if lines is not None else None, C.byref(cam) if cam is not None else None, int(fmt), _p(images),
                                          n, w, h, C.c_size_t(stride), C.c_size_t(image_stride), int(chunk), _p(kp), _p(kpun), _p(desc), _p(nk), orb.cap,
                                          _p(kl), _p(ld), _p(fn), _p(nl), int(kl.shape[1]), C.byref(M) if M is not None else None))
    return out, mout


def frontend_batch(orb, lines, images, chunk=0, max_lines=None, pinned=False):
    """sslam_frontend_batch: images = uint8 array [n, h, w] in HOST memory -> per-frame (keypoints, descriptors, keylines, line descriptors,
    line functions) lists; `lines` may be None (ORB only).  pinned=True allocates the result arrays in pinned memory (torch), so that the
    library copies straight into them; pass a pinned `images` array for the same on the way in."""
    images = np.ascontiguousarray(images, np.uint8)
    n, h, w = images.shape
    cap = orb.cap
    lcap = int(max_lines if max_lines is not None else (lines.max_lines if lines is not None else 1))

    def alloc(shape, dt):
        if not pinned:
            return np.zeros(shape, dt)
        import torch
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True).numpy()[:nbytes].view(dt).reshape(shape)
    kp = alloc((n, cap), KP_DTYPE); desc = alloc((n, cap, 32), np.uint8); nk = alloc((n,), np.int32)
    kl = alloc((n, lcap), KL_DTYPE); ld = alloc((n, lcap, 32), np.uint8); fn = alloc((n, lcap, 3), np.float64); nl = alloc((n,), np.int32)
    _chk(lib().sslam_frontend_batch(orb.h, lines.h if lines is not None else None, _p(images), n, w, h, C.c_size_t(w), C.c_size_t(w * h), int(chunk),
                                    _p(kp), _p(desc), _p(nk), cap, _p(kl), _p(ld), _p(fn), _p(nl), lcap))
    if lines is None:
        nl = np.zeros(n, np.int32)
    return [(kp[i, :nk[i]], desc[i, :nk[i]], kl[i, :nl[i]], ld[i, :nl[i]], fn[i, :nl[i]]) for i in range(n)]


class OrbExtractor:
    """Harness-side mirror of StructureSLAM::ORBextractor (include/ORBextractor.h:45-111)."""

    def __init__(self, ctx, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
        self.ctx = ctx
        self.nlevels = nlevels
        self.h = C.c_void_p()
        _chk(lib().sslam_orb_create(ctx.h, int(nfeatures), C.c_float(scale_factor), int(nlevels), int(ini_th), int(min_th), C.byref(self.h)))
        self.cap = lib().sslam_orb_max_keypoints(self.h)

    def set_blur_variant(self, variant):
        """0: the bit-exact 8-bit GaussianBlur of OpenCV >= 3.4.1 (default, decision D6); 1: OpenCV 3.4.0's rounded taps (sslam_orb_set_blur_variant)"""
        _chk(lib().sslam_orb_set_blur_variant(self.h, int(variant)))

    def set_gate_event(self, hip_event):
        """hipEvent_t handle (int) every following batch call waits for between its pyramid kernels and the rest; 0 / None clears it (sslam_orb_set_gate_event)"""
        _chk(lib().sslam_orb_set_gate_event(self.h, C.c_void_p(int(hip_event or 0))))

    def set_camera(self, cam):
        """sslam_orb_set_camera: with a Camera, Frame(ctx, orb=self) holds the undistorted keypoints (mvKeysUn); None clears it"""
        _chk(lib().sslam_orb_set_camera(self.h, C.byref(cam) if cam is not None else None))

    def scales(self):
        n = self.nlevels
        s = np.zeros(n, np.float32); i = np.zeros(n, np.float32); g = np.zeros(n, np.float32); ig = np.zeros(n, np.float32)
        f = np.zeros(n, np.int32)
        _chk(lib().sslam_orb_get_scales(self.h, _p(s), _p(i), _p(g), _p(ig), _p(f)))
        return s, i, g, ig, f

    def __call__(self, gray):
        """operator()(image, mask, keypoints, descriptors) on a host image."""
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape if gray.ndim == 2 else (0, 0)
        kp = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int(0)
        _chk(lib().sslam_orb_extract(self.h, _p(gray), w, h, C.c_size_t(gray.strides[0] if gray.ndim == 2 and h else 0),
                                     _p(kp), _p(desc), self.cap, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def extract_batch_dev(self, d_images, w, h, pitch, image_stride, nframes, d_kp, d_desc, d_counts, cap, stream=None):
        _chk(lib().sslam_orb_extract_batch_dev(self.h, _p(d_images), int(w), int(h), C.c_size_t(pitch), C.c_size_t(image_stride),
                                               int(nframes), _p(d_kp), _p(d_desc), _p(d_counts), int(cap), C.c_void_p(stream or 0)))

    def debug_level(self, frame, level):
        w = C.c_int(0); h = C.c_int(0)
        _chk(lib().sslam_orb_debug_level(self.h, frame, level, C.c_void_p(0), C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _chk(lib().sslam_orb_debug_level(self.h, frame, level, _p(out), C.byref(w), C.byref(h)))
        return out

    def debug_blur_patches(self, frame=0):
        """a7 stage tap: (keypoints, blurred 37x37 windows around them) of frame `frame` of the last call, in output order."""
        kp = np.zeros(self.cap, KP_DTYPE); pat = np.zeros((self.cap, 37, 37), np.uint8); n = C.c_int(0)
        _chk(lib().sslam_orb_debug_blur_patches(self.h, frame, _p(kp), _p(pat), self.cap, C.byref(n)))
        return kp[:n.value].copy(), pat[:n.value].copy()

    def debug_candidates(self, frame, level, cap=400000):
        out = np.zeros((cap, 3), np.int32); n = C.c_int(0)
        _chk(lib().sslam_orb_debug_candidates(self.h, frame, level, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def close(self):
        if self.h:
            lib().sslam_orb_destroy(self.h)
            self.h = C.c_void_p()


class LineExtractor:
    """Harness-side mirror of LineSegment::ExtractLineSegment (src/ExtractLineSegment.cpp:18-69)."""

    def __init__(self, ctx, max_lines=40):
        self.ctx = ctx
        self.max_lines = max_lines
        self.h = C.c_void_p()
        _chk(lib().sslam_lines_create(ctx.h, int(max_lines), C.byref(self.h)))

    def __call__(self, gray, cap=None):
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        cap = cap or 8192
        kl = np.zeros(cap, KL_DTYPE); ld = np.zeros((cap, 32), np.uint8); fn = np.zeros((cap, 3), np.float64)
        n = C.c_int(0)
        _chk(lib().sslam_lines_extract(self.h, _p(gray), w, h, C.c_size_t(gray.strides[0]), _p(kl), _p(ld), _p(fn), cap, C.byref(n)))
        return kl[:n.value].copy(), ld[:n.value].copy(), fn[:n.value].copy()

    def extract_batch_dev(self, d_images, w, h, pitch, image_stride, nframes, d_kl, d_ldesc, d_linefn, d_counts, cap, stream=None):
        _chk(lib().sslam_lines_extract_batch_dev(self.h, _p(d_images), int(w), int(h), C.c_size_t(pitch), C.c_size_t(image_stride),
                                                 int(nframes), _p(d_kl), _p(d_ldesc), _p(d_linefn), _p(d_counts), int(cap),
                                                 C.c_void_p(stream or 0)))

    def set_blur_variant(self, variant):
        """0: OpenCV >= 3.4.1's bit-exact 8-bit GaussianBlur (default, decision D6); 1: OpenCV 3.4.0's rounded taps (sslam_lines_set_blur_variant)"""
        _chk(lib().sslam_lines_set_blur_variant(self.h, int(variant)))

    def set_nfa_variant(self, variant):
        """decision D11: 1 = nfa()'s first term is (double(n) + 1) (default since round 5, OpenCV as recalled); 0 = log_gamma(n + 1) (sslam_lines_set_nfa_variant)"""
        _chk(lib().sslam_lines_set_nfa_variant(self.h, int(variant)))

    def set_lbd_bit_order(self, variant):
        """decision D12: 1 = comparison i -> 0x80 >> i (default since round 5, OpenCV as recalled); 0 = comparison i -> bit i (sslam_lines_set_lbd_bit_order)"""
        _chk(lib().sslam_lines_set_lbd_bit_order(self.h, int(variant)))

    def set_resize_variant(self, variant):
        """decision D7: 0 = INTER_LINEAR_EXACT for LSD's 0.8x rescale (default); 1 = INTER_LINEAR (sslam_lines_set_resize_variant)"""
        _chk(lib().sslam_lines_set_resize_variant(self.h, int(variant)))

    def set_seed_order(self, variant):
        """decision D2: 0 = raster order inside a gradient bin (default, on the device); 1 = the host's std::sort (sslam_lines_set_seed_order)"""
        _chk(lib().sslam_lines_set_seed_order(self.h, int(variant)))

    def set_topn_only(self, on):
        """sslam_lines_set_topn_only: the caller takes nothing but the max_lines output lines (the NFA stage may then leave candidates out; debug_segments returns the
        validated ones) -> the previous value"""
        return int(lib().sslam_lines_set_topn_only(self.h, int(bool(on))))

    def set_core_event(self, hip_event):
        """hipEvent_t handle (int) recorded right before the sequential LSD core of every following batch call; 0 / None clears it"""
        _chk(lib().sslam_lines_set_core_event(self.h, C.c_void_p(int(hip_event or 0))))

    def set_core_gate(self, wait_event, done_event):
        """sslam_lines_set_core_gate: hipEvent_t handles (int; 0 / None: none) waited for right before / recorded right behind the sequential core"""
        _chk(lib().sslam_lines_set_core_gate(self.h, C.c_void_p(int(wait_event or 0)), C.c_void_p(int(done_event or 0))))

    def debug_segments(self, frame, cap=20000):
        out = np.zeros((cap, 4), np.float32); n = C.c_int(0)
        _chk(lib().sslam_lines_debug_segments(self.h, frame, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    CORE_FORMS = ("cluster_stream", "cluster", "lone", "guest", "per_frame", "six_wave")
    NFA_FORMS = ("stream", "launches", "all")

    def last_forms(self):
        """what the last batch call of this handle chose (line_last_forms).  The testing library reads the handle's plain fields, whichever of the two libraries made it."""
        return line_last_forms(self.h)

    def batch_status(self, cap, stream=None):
        """sslam_lines_batch_status -> (status code, frames over capacity, frames over the LSD limit, first such frame or -1)"""
        t, u, f = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        rc = lib().sslam_lines_batch_status(self.h, int(cap), C.c_void_p(stream or 0), C.byref(t), C.byref(u), C.byref(f))
        return rc, t.value, u.value, f.value

    def close(self):
        if self.h:
            lib().sslam_lines_destroy(self.h)
            self.h = C.c_void_p()


def line_last_forms(handle):
    """sslam_testing_lines_last_forms (include/sslam_testing.h) of a sslam_lines handle -> dict(core, grid, fused_grad, sort_runs, nfa, eval_waves, count_waves, lbd_rpi);
    core, fused_grad, sort_runs and nfa are None where the call did not get there (-1 in the other words)"""
    o = (C.c_int32 * 8)()
    rc = testing_lib().sslam_testing_lines_last_forms(handle, o)
    if rc != 0:
        raise SslamError("sslam_testing_lines_last_forms: %d" % rc, rc)
    flag = lambda v: bool(v) if v >= 0 else None
    return dict(core=LineExtractor.CORE_FORMS[o[0]] if o[0] >= 0 else None, grid=o[1], fused_grad=flag(o[2]), sort_runs=flag(o[3]),
                nfa=LineExtractor.NFA_FORMS[o[4]] if o[4] >= 0 else None, eval_waves=o[5], count_waves=o[6], lbd_rpi=o[7])


class LinePrologue:
    """A sslam_lines handle of the TESTING library (lines_prepare uploads that library's constant tables once per handle) with the two taps of the line prologue,
    sslam_testing_lines_prologue and sslam_testing_lines_grad_table (include/sslam_testing.h), and sslam_lines_extract on the same handle."""

    def __init__(self, ctx, max_lines=40):
        self.T = testing_lib()
        self.T.sslam_testing_lines_prologue.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_size_t] + [C.c_void_p] * 6
        self.T.sslam_testing_lines_grad_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.h = C.c_void_p()
        self._chk(self.T.sslam_lines_create(ctx.h, int(max_lines), C.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            raise SslamError("%s: %s" % (self.T.sslam_status_str(rc).decode(), self.T.sslam_last_error().decode()), rc)

    def __enter__(self): return self

    def __exit__(self, *a): self.close()

    def __call__(self, images, dev_pitch=0, dev_offset=0):
        """images [n, h, w] uint8 (any strides with contiguous rows) -> list of n dicts(sw, sh, T [sh, sw] float32, S [sh, sw] int32, Cs [sh, sw, 2] float32,
        order [sw * sh] uint32 as x | y << 16, max_s, n_defined): the planes and the seed list copied back WHOLE (0xA5 where no kernel wrote)"""
        images = np.asarray(images, np.uint8)
        n, h, w = images.shape
        assert images.strides[2] == 1
        sw, sh = int(round(w * 0.8)), int(round(h * 0.8))
        cap = (sw + 1) * (sh + 1)          # (the library's own rounding decides: size_out)
        size = np.zeros(2, np.int32); T = np.zeros((n, cap), np.float32); S = np.zeros((n, cap), np.int32); Cs = np.zeros((n, cap, 2), np.float32)
        order = np.zeros((n, cap), np.uint32); misc = np.zeros((n, 2), np.int32)
        self._chk(self.T.sslam_testing_lines_prologue(self.h, images.ctypes.data, w, h, images.strides[1], images.strides[0], n, int(dev_pitch), int(dev_offset), cap,
                                                      size.ctypes.data, T.ctypes.data, S.ctypes.data, Cs.ctypes.data, order.ctypes.data, misc.ctypes.data))
        assert (int(size[0]), int(size[1])) == (sw, sh), (size, sw, sh)
        npx = sw * sh          # (a frame's arrays are npx long in the library's layout: frame b starts at b * npx)
        T, S, Cs, order = (a.reshape(-1)[:n * npx * k].reshape((n, npx) + ((2,) if k == 2 else ())) for a, k in ((T, 1), (S, 1), (Cs, 2), (order, 1)))
        return [dict(sw=sw, sh=sh, T=T[b].reshape(sh, sw), S=S[b].reshape(sh, sw), Cs=Cs[b].reshape(sh, sw, 2), order=order[b], max_s=int(misc[b, 0]),
                     n_defined=int(misc[b, 1])) for b in range(n)]

    def grad_table(self):
        """-> (k_grad_table's table [1021, 1021, 4] float32 indexed [gy + 510, gx + 510], k_grad_smin's smallest defined |g|^2)"""
        tab = np.zeros((1021, 1021, 4), np.float32); smin = C.c_int32(0)
        self._chk(self.T.sslam_testing_lines_grad_table(self.h, tab.ctypes.data, C.addressof(smin)))
        return tab, smin.value

    def last_forms(self):
        """words 2 and 3 of sslam_testing_lines_last_forms as (fused_grad, sort_runs): True / False, None where the call did not get there"""
        f = line_last_forms(self.h)
        return f["fused_grad"], f["sort_runs"]

    def set_resize_variant(self, variant): self._chk(self.T.sslam_lines_set_resize_variant(self.h, int(variant)))

    def set_seed_order(self, variant): self._chk(self.T.sslam_lines_set_seed_order(self.h, int(variant)))

    def extract(self, gray, cap=8192):
        """sslam_lines_extract on this handle -> (keylines, LBD rows, line equations, the segments before the top-N)"""
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        kl = np.zeros(cap, KL_DTYPE); ld = np.zeros((cap, 32), np.uint8); fn = np.zeros((cap, 3), np.float64); n = C.c_int(0)
        self._chk(self.T.sslam_lines_extract(self.h, _p(gray), w, h, C.c_size_t(gray.strides[0]), _p(kl), _p(ld), _p(fn), cap, C.byref(n)))
        seg = np.zeros((20000, 4), np.float32); m = C.c_int(0)
        self._chk(self.T.sslam_lines_debug_segments(self.h, 0, _p(seg), len(seg), C.byref(m)))
        return kl[:n.value].copy(), ld[:n.value].copy(), fn[:n.value].copy(), seg[:m.value].copy()

    def close(self):
        if self.h:
            self.T.sslam_lines_destroy(self.h)
            self.h = C.c_void_p()


class LineNfaStage:
    """A sslam_lines handle of the TESTING library with the tap of the NFA stage, sslam_testing_lines_nfa (include/sslam_testing.h): the stage's kernels on rectangle records
    the caller supplies, over the product's own T plane of the frames."""
    FILL = 0xA5A5A5A5          # the 32 bits of a flag or a segment coordinate the stage did not write (view the arrays as uint32)

    def __init__(self, ctx, max_lines=40):
        self.T = testing_lib()
        self.T.sslam_testing_lines_nfa.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
        self.h = C.c_void_p()
        rc = self.T.sslam_lines_create(ctx.h, int(max_lines), C.byref(self.h))
        if rc != 0:
            raise SslamError("%s: %s" % (self.T.sslam_status_str(rc).decode(), self.T.sslam_last_error().decode()), rc)

    def __enter__(self): return self

    def __exit__(self, *a): self.close()

    def raw(self, images, rects, ncand, topn_max_lines):
        """images [nf, h, w] uint8, rects [nf, nmax, 12] float64, ncand [nf] -> (status, (flags [nf, nmax] int32, segs [nf, nmax, 4] float32, topn [nf] int32)): the arrays
        copied back WHOLE (FILL where the stage did not write; include/sslam_testing.h says which rows of a ranked frame are unspecified)"""
        images = np.ascontiguousarray(images, np.uint8); rects = np.ascontiguousarray(rects, np.float64); ncand = np.ascontiguousarray(ncand, np.int32)
        nf, h, w = images.shape
        assert rects.ndim == 3 and rects.shape[0] == nf and rects.shape[2] == 12 and ncand.shape == (nf,)
        nmax = rects.shape[1]
        flags = np.zeros((nf, nmax), np.int32); segs = np.zeros((nf, nmax, 4), np.float32); topn = np.full(nf, -1, np.int32)
        rc = self.T.sslam_testing_lines_nfa(self.h, images.ctypes.data, w, h, w, w * h, nf, rects.ctypes.data, ncand.ctypes.data, nmax, int(topn_max_lines),
                                            flags.ctypes.data, segs.ctypes.data, topn.ctypes.data)
        return rc, (flags, segs, topn)

    def __call__(self, images, rects, ncand, topn_max_lines=0):
        rc, out = self.raw(images, rects, ncand, topn_max_lines)
        if rc != 0:
            raise SslamError("%s: %s" % (self.T.sslam_status_str(rc).decode(), self.T.sslam_last_error().decode()), rc)
        return out

    def last_forms(self):
        """words 0 and 2 .. 6 of sslam_testing_lines_last_forms -> dict(core, fused_grad, sort_runs, nfa, eval_waves, count_waves); the tap runs no core"""
        f = line_last_forms(self.h)
        return {k: f[k] for k in ("core", "fused_grad", "sort_runs", "nfa", "eval_waves", "count_waves")}

    def close(self):
        if self.h:
            self.T.sslam_lines_destroy(self.h)
            self.h = C.c_void_p()


class LineCore:
    """A sslam_lines handle of the TESTING library with the tap of the sequential LSD core, sslam_testing_lines_core / _core_frame (include/sslam_testing.h): the product
    path's prologue and core launch on device frames, then per frame the candidate count, the first records and the T plane."""
    FILL = 0xA5A5A5A5A5A5A5A5          # the 64 bits of a record field the core did not write (view the records as uint64)

    def __init__(self, ctx, max_lines=40):
        self.T = testing_lib()
        self.T.sslam_testing_lines_core.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int]
        self.T.sslam_testing_lines_core_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t] + [C.c_void_p] * 4
        self.h = C.c_void_p()
        self._chk(self.T.sslam_lines_create(ctx.h, int(max_lines), C.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            raise SslamError("%s: %s" % (self.T.sslam_status_str(rc).decode(), self.T.sslam_last_error().decode()), rc)

    def __enter__(self): return self

    def __exit__(self, *a): self.close()

    def run(self, d_images, w, h, pitch, image_stride, nframes):
        """the run step on frames that are on the device (a torch tensor or a pointer)"""
        self._chk(self.T.sslam_testing_lines_core(self.h, _p(d_images), int(w), int(h), C.c_size_t(pitch), C.c_size_t(image_stride), int(nframes)))

    def frame_raw(self, frame, nmax, want_t=True):
        """the copy-back step -> (status, dict(sw, sh, ncand, rects [nmax, 12] float64 copied back WHOLE, T [sh, sw] float32 or None))"""
        size = np.zeros(2, np.int32); n = np.full(1, -1, np.int32); rects = np.zeros((max(nmax, 1), 12), np.float64)
        rc = self.T.sslam_testing_lines_core_frame(self.h, int(frame), int(nmax), 0, size.ctypes.data, n.ctypes.data, rects.ctypes.data, None)
        T = None
        if want_t and rc in (0, SSLAM_ERR_UNSUPPORTED):
            T = np.zeros((int(size[1]), int(size[0])), np.float32)
            rc = self.T.sslam_testing_lines_core_frame(self.h, int(frame), int(nmax), T.size, size.ctypes.data, n.ctypes.data, rects.ctypes.data, T.ctypes.data)
        return rc, dict(sw=int(size[0]), sh=int(size[1]), ncand=int(n[0]), rects=rects[:nmax], T=T)

    def frame(self, frame, nmax, want_t=True):
        rc, out = self.frame_raw(frame, nmax, want_t)
        self._chk(rc)
        return out

    def last_forms(self): return line_last_forms(self.h)

    def set_core_event(self, hip_event): self._chk(self.T.sslam_lines_set_core_event(self.h, C.c_void_p(int(hip_event or 0))))

    def close(self):
        if self.h:
            self.T.sslam_lines_destroy(self.h)
            self.h = C.c_void_p()


# ---- multi-GPU batch mode (include/sslam_frontend.h: sslam_group_*, record stream) ------------------------------------------------
class FrontendParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("ini_th_fast", C.c_int32),
                ("min_th_fast", C.c_int32), ("max_lines", C.c_int32)]


def record_bytes(nkp, nl):
    return (16 + nkp * 60 + nl * 124 + 15) & ~15


def record_stream_capacity(nframes, cap, lcap):
    lib().sslam_record_stream_capacity.restype = C.c_uint64
    return int(lib().sslam_record_stream_capacity(int(nframes), int(cap), int(lcap)))


def pack_records_dev(ctx, nframes, frame0, frame_step, d_kp, d_desc, d_nkp, cap, d_kl, d_ldesc, d_linefn, d_nl, lcap, d_out, out_capacity, d_total, stream=None):
    """device tensors / pointers in, record stream in d_out, length in the device word d_total (enqueued, not synchronised)"""
    _chk(lib().sslam_pack_records_dev(ctx.h, int(nframes), int(frame0), int(frame_step), _p(d_kp), _p(d_desc), _p(d_nkp), int(cap),
                                      _p(d_kl), _p(d_ldesc), _p(d_linefn), _p(d_nl), int(lcap), _p(d_out), C.c_uint64(out_capacity), _p(d_total),
                                      C.c_void_p(stream or 0)))


def unpack_records(stream, nframes, cap, lcap, with_lines=True):
    """host record stream (uint8 array) -> (kp[n,cap], desc, nkp, kl, ldesc, linefn, nl, nrecords) as sslam_frontend_batch lays them out"""
    stream = np.ascontiguousarray(stream, np.uint8)
    kp = np.zeros((nframes, cap), KP_DTYPE); desc = np.zeros((nframes, cap, 32), np.uint8); nk = np.full(nframes, -1, np.int32)
    kl = np.zeros((nframes, lcap), KL_DTYPE); ld = np.zeros((nframes, lcap, 32), np.uint8); fn = np.zeros((nframes, lcap, 3), np.float64); nl = np.full(nframes, -1, np.int32)
    nrec = C.c_int(0)
    _chk(lib().sslam_unpack_records(_p(stream), C.c_uint64(stream.size), int(nframes), _p(kp), _p(desc), _p(nk), int(cap),
                                    _p(kl) if with_lines else None, _p(ld), _p(fn), _p(nl), int(lcap), C.byref(nrec)))
    return kp, desc, nk, kl, ld, fn, nl, nrec.value


class Group:
    """sslam_group: Group(ngpu=G) drives G devices from this process; Group(device=, rank=, nranks=, uid=) is one rank of a
    one-process-per-GPU job (uid from Group.unique_id() on rank 0, broadcast by the launcher)."""

    def __init__(self, ngpu=None, device=0, rank=0, nranks=1, uid=None):
        self.h = C.c_void_p()
        if ngpu is not None:
            _chk(lib().sslam_group_create(int(ngpu), C.byref(self.h)))
        else:
            uid = np.ascontiguousarray(uid, np.uint8)
            assert uid.size == 128
            _chk(lib().sslam_group_create_rank(int(device), int(rank), int(nranks), _p(uid), C.byref(self.h)))
        self.size = lib().sslam_group_size(self.h); self.rank = lib().sslam_group_rank(self.h)

    @staticmethod
    def unique_id():
        uid = np.zeros(128, np.uint8)
        _chk(lib().sslam_group_unique_id(_p(uid)))
        return uid

    def gather_dev(self, d_send, d_send_bytes, d_recv=None, recv_capacity=0, stream=None):
        """the exchange step (blocking); returns the per-rank stream lengths on rank 0, None elsewhere"""
        sizes = np.zeros(self.size, np.uint64)
        _chk(lib().sslam_group_gather_dev(self.h, _p(d_send), _p(d_send_bytes), _p(d_recv), C.c_uint64(recv_capacity), _p(sizes), C.c_void_p(stream or 0)))
        return sizes if self.rank == 0 else None

    def frontend_batch_sharded(self, images, nfeatures=1000, max_lines=200, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, cap=None, lcap=None):
        images = np.ascontiguousarray(images, np.uint8)
        n, h, w = images.shape
        prm = FrontendParams(int(nfeatures), float(scale_factor), int(nlevels), int(ini_th), int(min_th), int(max_lines))
        if cap is None:
            cap = int(nfeatures) + 64 * int(nlevels)
        lcap = int(lcap if lcap is not None else max(max_lines, 1))
        kp = np.zeros((n, cap), KP_DTYPE); desc = np.zeros((n, cap, 32), np.uint8); nk = np.zeros(n, np.int32)
        kl = np.zeros((n, lcap), KL_DTYPE); ld = np.zeros((n, lcap, 32), np.uint8); fn = np.zeros((n, lcap, 3), np.float64); nl = np.zeros(n, np.int32)
        _chk(lib().sslam_frontend_batch_sharded(self.h, C.byref(prm), _p(images), n, w, h, C.c_size_t(w), C.c_size_t(w * h), _p(kp), _p(desc), _p(nk), cap,
                                                _p(kl), _p(ld), _p(fn), _p(nl), lcap))
        return [(kp[i, :nk[i]], desc[i, :nk[i]], kl[i, :nl[i]], ld[i, :nl[i]], fn[i, :nl[i]]) for i in range(n)]

    def close(self):
        if self.h:
            lib().sslam_group_destroy(self.h)
            self.h = C.c_void_p()
