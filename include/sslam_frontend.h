/* sslam_frontend.h — C ABI of the MI355X-native point+line feature front-end.
 *
 * This is the drop-in boundary beneath the reference's C++ call surface
 * (Structure-SLAM-PointLine).  Every entry point names the reference interface it
 * replaces (paths relative to the reference tree).  Plain pointers and sizes only;
 * no C++/torch/HIP types in any signature (streams travel as void*).
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, <0 = error (sslam_status_str()).
 *     Nothing throws across the boundary.
 *   - "host" entry points take host pointers and are synchronous (H2D, kernels, D2H);
 *     "_dev" entry points take DEVICE pointers, enqueue on the given HIP stream
 *     (void* = hipStream_t, NULL = the context's own stream) and return without
 *     synchronising.
 *   - The caller owns every output buffer (reference: _keypoints/_descriptors are
 *     caller containers, src/ORBextractor.cc:1064-1073).
 *   - The library fails loudly (SSLAM_ERR_NO_DEVICE) when no HIP device is usable:
 *     there is no CPU fallback.
 */
#ifndef SSLAM_FRONTEND_H
#define SSLAM_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSLAM_OK 0
#define SSLAM_ERR_INVALID (-1)     /* bad argument */
#define SSLAM_ERR_NO_DEVICE (-2)   /* no usable HIP device / HIP runtime error */
#define SSLAM_ERR_CAPACITY (-3)    /* caller buffer too small */
#define SSLAM_ERR_HIP (-4)         /* a HIP call failed; see sslam_last_error() */
#define SSLAM_ERR_UNSUPPORTED (-5)

/* cv::KeyPoint, 28 bytes (opencv2/core/types.hpp): pt.x, pt.y, size, angle,
 * response, octave, class_id.  Layout consumed verbatim by include/Frame.h:155-160. */
typedef struct sslam_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} sslam_keypoint;

/* cv::line_descriptor::KeyLine, 68 bytes (opencv2/line_descriptor/descriptor.hpp):
 * consumed by include/Frame.h:183-189. */
typedef struct sslam_keyline {
    float angle;
    int32_t class_id, octave;
    float pt_x, pt_y, response, size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength;
    int32_t numOfPixels;
} sslam_keyline;

typedef struct sslam_ctx sslam_ctx;     /* device context: HIP device, stream, scratch */
typedef struct sslam_orb sslam_orb;     /* = StructureSLAM::ORBextractor state */
typedef struct sslam_lines sslam_lines; /* = LSDDetector + BinaryDescriptor state */

const char* sslam_status_str(int status);
const char* sslam_last_error(void);      /* thread-local text of the last failure */
int sslam_abi_version(void);

/* ---- context ------------------------------------------------------------- */
int sslam_ctx_create(int device, sslam_ctx** out);
int sslam_ctx_destroy(sslam_ctx* ctx);
int sslam_ctx_synchronize(sslam_ctx* ctx);
void* sslam_ctx_stream(sslam_ctx* ctx);  /* hipStream_t of the context */

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline
 * leg; no reference counterpart).  drain() synchronises, returns the number of distinct
 * kernels and fills name / total ms / launch count per kernel. */
int sslam_profile_enable(sslam_ctx* ctx, int on);
int sslam_profile_drain(sslam_ctx* ctx, const char** names_out, double* ms_out, int* launches_out, int cap);

/* ---- ORB  (replaces StructureSLAM::ORBextractor) --------------------------- */
/* ORBextractor::ORBextractor(int nfeatures,float scaleFactor,int nlevels,int iniThFAST,
 * int minThFAST), src/ORBextractor.cc:410-470. */
int sslam_orb_create(sslam_ctx* ctx, int nfeatures, float scaleFactor, int nlevels,
                     int iniThFAST, int minThFAST, sslam_orb** out);
int sslam_orb_destroy(sslam_orb* orb);
/* Which 8-bit cv::GaussianBlur(7x7, sigma 2) the descriptors are computed on (src/ORBextractor.cc:1085-1086; the leaf is OpenCV's, and its
 * arithmetic changed inside the 3.4 series): 0 (default) = the bit-exact fixed-point filter of OpenCV >= 3.4.1, 8.8 taps 18 34 48 56 48 34 18
 * that sum to 256 (DESIGN.md decision D6); 1 = OpenCV 3.4.0 -- the version the reference's README names -- whose filter engine rounds every
 * tap of the float kernel: 18 34 49 55 49 34 18 (sum 257, result saturated).  Keypoints are the same either way; 3.7 % of the descriptor bits
 * differ between the two (oracle/ref_pin/pin_report_stub.json).  Takes effect with the next extraction. */
int sslam_orb_set_blur_variant(sslam_orb* orb, int variant);

/* GetLevels/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/
 * GetInverseScaleSigmaSquares, include/ORBextractor.h:63-83.  Each array has
 * nlevels entries; NULL pointers are skipped. */
int sslam_orb_get_scales(const sslam_orb* orb, float* scale, float* inv_scale,
                         float* sigma2, float* inv_sigma2, int32_t* features_per_level);

/* Upper bound on keypoints one frame can return (nfeatures + per-level overshoot,
 * SURVEY.md D.2 step 5); size kp/desc buffers with it. */
int sslam_orb_max_keypoints(const sslam_orb* orb);

/* ORBextractor::operator()(image, mask, keypoints, descriptors),
 * src/ORBextractor.cc:1043-1105 as called from Frame::ExtractORB (src/Frame.cc:155-161).
 * gray: host CV_8UC1, stride in bytes.  kp_out[cap], desc_out[cap*32] host.
 * Empty image (w==0||h==0) -> *n_out = 0, outputs untouched (:1046-1047). */
int sslam_orb_extract(sslam_orb* orb, const uint8_t* gray, int w, int h, size_t stride,
                      sslam_keypoint* kp_out, uint8_t* desc_out, int cap, int* n_out);

/* Batch-of-frames mode (north_star): nframes independent images of identical size
 * resident in HBM.  d_images + i*image_stride is frame i (row pitch `pitch`).
 * d_kp[nframes*cap], d_desc[nframes*cap*32], d_counts[nframes] are device buffers.
 * Level 0 of the pyramid is READ IN PLACE from d_images when base, pitch and image_stride are multiples of 4 and the frames are whole blocks
 * (pitch == w, or image_stride >= pitch * h): the kernels load aligned dwords and may touch the padding bytes [w, pitch) of a row, so with
 * padded rows every frame -- the last one included -- must be readable for pitch * h bytes.  Any other layout is copied first (one more pass).
 * A pitch below w, or frames that overlap (image_stride < pitch * (h - 1) + w, when nframes > 1), give SSLAM_ERR_INVALID; nothing is enqueued.
 * The padding bytes, the gaps between frames and the bytes around the buffer never change a result, and the images are only read.
 * The images must stay valid until the call's work on `stream` has finished (as for any asynchronous launch). */
int sslam_orb_extract_batch_dev(sslam_orb* orb, const uint8_t* d_images, int w, int h,
                                size_t pitch, size_t image_stride, int nframes,
                                sslam_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts,
                                int cap, void* stream);

/* Batch status.  The batch kernels clamp a frame's rows to `cap` (d_counts[i] <= cap) and cannot return a status from the device, so a
 * batch caller asks afterwards: frames of the LAST batch on this handle whose keypoint total exceeded `cap` -- the condition for which the
 * single-frame call returns SSLAM_ERR_CAPACITY.  The host form synchronises the stream and returns SSLAM_ERR_CAPACITY when there is one
 * (first_frame_out = its index, -1 if none); the _dev form enqueues the check and writes d_status4 = {frames over capacity, first such frame
 * (INT_MAX if none), 0, INT_MAX}.  sslam_frontend_batch performs both checks per chunk itself. */
int sslam_orb_batch_status(sslam_orb* orb, int cap, void* stream, int* truncated_frames_out, int* first_frame_out);
int sslam_orb_batch_status_dev(sslam_orb* orb, int cap, int32_t* d_status4, void* stream);

/* Stage taps for stage-by-stage parity tests (not used by the drop-in shim):
 * copy pyramid level `level` of frame `frame` of the LAST batch to host (unpadded,
 * contiguous w*h), and the FAST candidate list (x,y,score triplets relative to
 * minBorder, reference src/ORBextractor.cc:820-825) of that level.
 * Level 0 (and the blurred patches of level-0 keypoints) of a batch that was read in place come from the CALLER's image buffer of that
 * batch: it must still be alive when a tap is called (sslam_orb_extract keeps its own copy; a freed device buffer is the caller's error). */
int sslam_orb_debug_level(sslam_orb* orb, int frame, int level, uint8_t* out, int* w, int* h);
int sslam_orb_debug_candidates(sslam_orb* orb, int frame, int level, int32_t* xys_out, int cap, int* n_out);
/* Stage tap of GaussianBlur(7x7, sigma 2) on the level clones (src/ORBextractor.cc:1085-1086): the blurred levels are never stored
 * (the blur is fused into the descriptor kernel), so the tap re-runs that kernel's two blur passes over the selection of frame
 * `frame` of the LAST batch and returns, per keypoint in output order, its KeyPoint record and the blurred 37x37 window
 * (|dx|,|dy| <= 18, row-major, in level coordinates) around it: kp_out[cap], patches_out[cap*37*37]. */
int sslam_orb_debug_blur_patches(sslam_orb* orb, int frame, sslam_keypoint* kp_out, uint8_t* patches_out, int cap, int* n_out);

/* ---- Hamming matching (replaces DescriptorDistance / BFMatcher / Search*) -- */
/* cv::BFMatcher(NORM_HAMMING,false).knnMatch(q,t,matches,2) as used at
 * src/LSDmatcher.cpp:150-155,261-266,293-298,336-341,387-392 and
 * ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1650-1666).
 * idx/dist are nq x 2 (best, second); missing neighbours (nt<2) are idx=-1,dist=-1.
 * Ties resolve to the lower train index. */
int sslam_hamming_knn2(sslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                       int32_t* idx_out, int32_t* dist_out);
int sslam_hamming_knn2_dev(sslam_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                           int32_t* d_idx, int32_t* d_dist, void* stream);
/* Batch form: frame f = rows [f*cap, f*cap+nq[f]) of d_q against rows [f*cap, f*cap+nt[f]) of d_t;
 * d_idx/d_dist are nframes*cap x 2.  For cap <= 4096 the train rows are first expanded to matrix-core operands in a buffer the CONTEXT keeps
 * (256 B per train row, nframes * cap rows, never shrunk: 3 GB for 12 288 frames of 1 000 rows).  Calls on different streams of one context are
 * ordered on that buffer by an event (a later call's expansion waits for the earlier call's search), so they do not overlap; use one context per
 * stream for concurrent searches. */
int sslam_hamming_knn2_batch_dev(sslam_ctx* ctx, const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t,
                                 const int32_t* d_nt, int cap, int nframes, int32_t* d_idx, int32_t* d_dist, void* stream);
/* Dense nq x nt distance matrix (uint16), the input of the windowed Search* variants. */
int sslam_hamming_matrix(sslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* D);

/* ORBmatcher::SearchForInitialization(F1,F2,vbPrevMatched,vnMatches12,windowSize),
 * src/ORBmatcher.cc:408-523, with Frame::GetFeaturesInArea (src/Frame.cc:368-421) and
 * the 64x48 grid (src/Frame.cc:133-148,462-472) evaluated on the device.
 * kp1/desc1 (n1) = F1.mvKeysUn/mDescriptors, kp2/desc2 (n2) = F2; prev_matched[n1*2]
 * in/out (vbPrevMatched); matches12[n1] out; bounds = mnMinX,mnMaxX,mnMinY,mnMaxY. */
int sslam_orb_search_for_initialization(sslam_ctx* ctx,
        const sslam_keypoint* kp1, const uint8_t* desc1, int n1,
        const sslam_keypoint* kp2, const uint8_t* desc2, int n2,
        float* prev_matched, int32_t* matches12, int window_size,
        float nnratio, int check_orientation, const float bounds[4], int* nmatches_out);
/* Batch/device form: frame pair p uses kp1 + p*cap etc.; counts n1[p], n2[p] on device. */
int sslam_orb_search_for_initialization_batch_dev(sslam_ctx* ctx,
        const sslam_keypoint* d_kp1, const uint8_t* d_desc1, const int32_t* d_n1,
        const sslam_keypoint* d_kp2, const uint8_t* d_desc2, const int32_t* d_n2,
        int cap, int npairs, float* d_prev_matched, int32_t* d_matches12, int32_t* d_nmatches,
        int window_size, float nnratio, int check_orientation, const float bounds[4], void* stream);

/* The model selection of Initializer::Initialize (src/Initializer.cc:55-118, reached from src/Tracking.cc:366 right behind SearchForInitialization): `iterations` RANSAC
 * hypotheses, each one homography and one fundamental matrix from eight matches (FindHomography / FindFundamental :155-253, ComputeH21 / ComputeF21 :255-332 on the points of
 * Normalize :784-830), scored against every match (CheckHomography / CheckFundamental :334-497), the best of each and RH = SH / (SH + SF) (:118).  What follows in the
 * reference -- ReconstructH / ReconstructF, CheckRT, Triangulate (:499-782, :833 on) -- has its batch form on the device too (sslam_two_view_reconstruct_batch_dev below,
 * which takes H21 / F21 and the inlier bits where this call leaves them); map creation and g2o stay with the caller.  kp1 / kp2 are the UNDISTORTED keypoints (mvKeysUn: sslam_undistort_keypoints_batch_dev); matches12[i] is the keypoint of frame 2 matched to keypoint i
 * of frame 1 or negative (vnMatches12: sslam_orb_search_for_initialization_batch_dev's d_matches12); a row counts as matched when 0 <= matches12[i] < n2, and the matched rows in
 * ascending i are the match list (mvMatches12, :67-76).  sigma is mSigma (1.0 in Tracking), iterations mMaxIterations (200).
 *   sets  NULL: iteration `it` of pair p draws its eight matches as :93-108 do, with randi = hash32(seed, p, it, j) % remaining (csrc/ransac_draw.h states hash32; the
 *         reference's rand() stream is per process and not reproducible per pair).  Otherwise sets[(p * iterations + it) * 8 + j] are indices into the match list and replace
 *         the draw -- the hook for a caller that wants the reference's own rand() stream.  An iteration with an index outside [0, nmatches) gets zero matrices and the score 0:
 *         it never wins.  H and F share the sets, as in the reference.
 *   result, one per pair.  A pair with fewer than 8 matches is skipped: model 0, best_it -1, scores, rh and matrices 0, inlier bytes 0.  (Tracking only initialises from 100
 *         matches on; the library itself only refuses below 8.)  best_it_h / best_it_f: the first iteration with the highest score above 0 (:196, :246: a strict >), -1 when
 *         no score exceeded 0 (the matrix is zero then).  A NaN score (a singular H21i: its inverse is the zero matrix) never wins, as in the reference.  rh is the float the
 *         reference holds (NaN for 0 / 0); model is 1 (H) when rh > 0.40 and 2 (F) otherwise.
 *   inliers[i], by keypoint 1 like matches12: bit 0 = inlier of the winning H (vbMatchesInliersH), bit 1 = inlier of the winning F; 0 for an unmatched row.  Rows [n1, cap) are
 *         not written.
 * What the reference leaves to OpenCV here (cv::SVDecomp, the float matrix product and inverse) is restated by decision D15 of DESIGN.md; everything else is the reference's
 * arithmetic operation for operation, the score summed in match order.
 * The batch form uses the layout of sslam_orb_search_for_initialization_batch_dev: pair p owns rows [p*cap, (p+1)*cap) of d_kp1, d_kp2, d_matches12 and d_inliers, counts
 * d_n1[p], d_n2[p] on the device.  One launch on `stream` (NULL: the context's stream), no scratch, no synchronise, no host memory read or written; every output word has one
 * writer.  SSLAM_ERR_INVALID (nothing enqueued): a NULL pointer other than d_sets, cap or npairs < 1, iterations < 1, sigma <= 0 or NaN, a pointer that is not 4-byte aligned,
 * npairs * cap >= 2^31.  SSLAM_ERR_UNSUPPORTED (nothing enqueued): cap > 4096 (the match rows sit in LDS, 16 bytes each).  The single call is pair 0 of the same kernel
 * (cap = max(n1, n2)) and synchronises. */
typedef struct sslam_two_view_result {      /* 100 bytes */
    int32_t nmatches;               /* matched rows the call saw */
    int32_t model;                  /* 0 = skipped (nmatches < 8), 1 = H (RH > 0.40), 2 = F */
    int32_t best_it_h, best_it_f;   /* winning iteration, -1 when no score exceeded 0 */
    float score_h, score_f, rh;     /* SH, SF, SH / (SH + SF) */
    float H21[9], F21[9];           /* row-major; zeros when best_it is -1 */
} sslam_two_view_result;
int sslam_two_view_ransac(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2,
        const int32_t* matches12, const int32_t* sets /* NULL or [iterations*8] */, int iterations, float sigma, uint32_t seed,
        sslam_two_view_result* result, uint8_t* inliers /* [n1] */);
int sslam_two_view_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp1, const int32_t* d_n1,
        const sslam_keypoint* d_kp2, const int32_t* d_n2, int cap, int npairs, const int32_t* d_matches12,
        const int32_t* d_sets /* NULL or [npairs*iterations*8] */, int iterations, float sigma, uint32_t seed,
        sslam_two_view_result* d_result, uint8_t* d_inliers /* [npairs*cap] */, void* stream);

/* The second half of Initializer::Initialize (src/Initializer.cc:143-152): ReconstructH (:611-781, Faugeras' eight hypotheses) when the model is 1, ReconstructF (:500-608 with
 * DecomposeE :964-984, four hypotheses) when it is 2, each hypothesis checked by CheckRT (:833-961) over every inlier match with Triangulate (:987-1000), the reference's choice
 * among them, and with the winning R21 / t21 the line half of this fork: ReconstructLine (:1059-1171) with LineTriangulate (:1003-1055) and the two MADs of vector_mad
 * (include/auxiliar.h:91-106).  Together with sslam_two_view_ransac* this is all of Initialize (:55-153): (:499-782, :833-1171) are this call.
 * Pair layout and counts are sslam_two_view_ransac_batch_dev's; d_result and d_inliers are that call's outputs where they lie (model 1 reads H21 and bit 0 of the inlier
 * bytes, model 2 F21 and bit 1; any other model is a skipped pair).  d_K[p*4 .. +4) = fx fy cx cy of mK (the reference frame's); sigma is mSigma (th2 = 4 sigma^2, :527),
 * min_parallax and min_triangulated the 1.0 and 50 of :146 / :150.
 *   pose, one per pair.  ok is Initialize's return value.  reason: 0 ok, 1 skipped (model 0), 2 H: singular values not separated (:639), 3 no clear winner or too few points
 *         (:550; :763 without its parallax term), 4 parallax below min_parallax (:559-604; :763).  hypothesis: the candidate the reference settled on -- F: 0 .. 3 = (R1, t1),
 *         (R2, t1), (R1, t2), (R2, t2), the FIRST whose nGood equals maxGood, once :550 let it through; H: bestSolutionIdx 0 .. 7 -- and -1 when there is none; with reason 4
 *         it names the candidate that failed.  n_inliers is N (:504-507).  n_good / parallax: CheckRT's return and parallax per hypothesis, 0 for entries that were not run.
 *         R21 (row-major) / t21: zeros when !ok.  n_triangulated: true entries of vbTriangulated.  n_lines: line pairs that passed the index filter; n_lines_triangulated:
 *         true entries of vbLineTriangulated (0 when !ok).
 *   p3d / triangulated, by keypoint 1 (vP3D, vbTriangulated): rows [0, n1) are always written, zeros and 0 for a row that is not triangulated and for every row of a pair
 *         that fails; rows [n1, cap) are not written.
 *   lines, all NULL or none NULL: d_kl1 / d_kl2 [npairs*lcap] with counts d_nl1 / d_nl2, d_linefn1 / d_linefn2 [npairs*lcap*3] (mvKeyLineFunctions), d_line_pairs
 *         [(p*lcap + r)*2 + {0, 1}] = (line of frame 1, line of frame 2) for r < d_line_npairs[p], as sslam_frontend_batch_match leaves them.  The line outputs are indexed by
 *         that row r: rows [0, min(max(d_line_npairs[p], 0), lcap)) are always written.  A pair with an index outside [0, nl) is left out as the reference's >= 0 filter
 *         (:133) leaves it out: written as zeros and 0, not part of the MADs.  A row whose endpoints are not finite keeps zero endpoints, error 0 and stays triangulated
 *         (:1102-1106).  With !ok every line output is zero.  The line of frame 2 enters through its function alone, as in the reference (d_kl2 is not read).
 * What the reference leaves to OpenCV, Eigen and libm here (cv::SVD::compute of the 3 x 3 and 4 x 4, the float products, acos, the sorts) is restated by decision D18 of
 * DESIGN.md; everything else is the reference's arithmetic operation for operation.
 * One launch on `stream` (NULL: the context's stream), one workgroup per pair, no scratch, no synchronise, no host memory read or written; every output word has one writer.
 * SSLAM_ERR_INVALID (nothing enqueued): a NULL pointer other than the line arguments, line arguments given in part, cap or npairs < 1, lcap < 1 with lines, sigma <= 0 or
 * NaN, min_triangulated < 0, a pointer that is not 4-byte aligned (d_linefn1 / d_linefn2: 8), npairs * cap >= 2^31 or npairs * lcap >= 2^31.  SSLAM_ERR_UNSUPPORTED (nothing
 * enqueued): cap > 5120 or lcap > 1024 (a pair's rows sit in LDS).  The single call is pair 0 of the same kernel (cap = max(n1, n2), lcap = max(nl1, nl2, line_npairs)) and
 * synchronises; its line arguments are absent when line_pairs is NULL (line_npairs 0 and the other line arguments NULL then); with lines, kl2 may be NULL (it is
 * not read). */
typedef struct sslam_two_view_pose {      /* 144 bytes */
    int32_t ok;                     /* Initialize's return value */
    int32_t reason;                 /* 0 ok, 1 skipped, 2 H: singular values not separated, 3 no clear winner or too few points, 4 parallax below min */
    int32_t model, hypothesis;      /* 1 H / 2 F as in the result; the candidate hypothesis, -1 if none */
    int32_t n_inliers;              /* N */
    int32_t n_good[8]; float parallax[8];      /* CheckRT per hypothesis; unused entries 0 */
    float R21[9], t21[3];           /* zeros when !ok */
    int32_t n_triangulated, n_lines, n_lines_triangulated;
} sslam_two_view_pose;
int sslam_two_view_reconstruct_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp1, const int32_t* d_n1, const sslam_keypoint* d_kp2, const int32_t* d_n2,
        int cap, int npairs, const int32_t* d_matches12, const sslam_two_view_result* d_result, const uint8_t* d_inliers, const float* d_K /* [npairs*4] */,
        float sigma, float min_parallax, int min_triangulated,
        const sslam_keyline* d_kl1, const int32_t* d_nl1, const sslam_keyline* d_kl2, const int32_t* d_nl2, const double* d_linefn1, const double* d_linefn2, int lcap,
        const int32_t* d_line_pairs, const int32_t* d_line_npairs,
        sslam_two_view_pose* d_pose, float* d_p3d /* [npairs*cap*3] */, uint8_t* d_triangulated /* [npairs*cap] */,
        float* d_line_s3d, float* d_line_e3d /* [npairs*lcap*3] */, uint8_t* d_line_triangulated /* [npairs*lcap] */, void* stream);
int sslam_two_view_reconstruct(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
        const sslam_two_view_result* result, const uint8_t* inliers /* [n1] */, const float K[4], float sigma, float min_parallax, int min_triangulated,
        const sslam_keyline* kl1, int nl1, const sslam_keyline* kl2, int nl2, const double* linefn1, const double* linefn2,
        const int32_t* line_pairs /* NULL or [line_npairs*2] */, int line_npairs,
        sslam_two_view_pose* pose, float* p3d /* [n1*3] */, uint8_t* triangulated /* [n1] */,
        float* line_s3d, float* line_e3d /* [line_npairs*3] */, uint8_t* line_triangulated /* [line_npairs] */);

/* Sim3Solver (src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cc:279-306) between SearchByBoW (:269: sslam_orb_search_by_bow_keyframes_batch_dev) and
 * SearchBySim3 (:328: sslam_fuse_search_batch_dev, which takes the s, R, t found here): the constructor (:37-112), SetRansacParameters (:114-138) and iterate (:140-207) with
 * ComputeSim3 (:226-337, Horn's closed form on three drawn correspondences), CheckInliers (:340-364) and Project (:382-403).  What follows in the reference -- OptimizeSim3
 * (g2o), the KeyFrameDatabase, the bookkeeping of :308-347 -- stays with the caller.
 * The pool and d_pairs are those of sslam_orb_search_by_bow_keyframes_batch_dev: keyframe slot k owns rows [k*cap, k*cap + d_n[k]) of d_kp (mvKeysUn; only `octave` is read),
 * d_valid (= GetMapPoint(i) && !isBad(); NULL: every row is valid) and d_x3dc; a count below 0 is read as 0, one above cap as cap; pair p is (kf1, kf2) = (d_pairs[2p],
 * d_pairs[2p+1]); d_matches12 is that call's output, used where it lies.  d_x3dc[(k*cap + i)*3 .. +3) is the camera-frame position Rcw * Xw + tcw (:94-98) of the map point at
 * row i of slot k: the caller fills it (poses and map points stay with the tracker) and it is read only for rows that enter a correspondence.  d_K[k*4 .. +4) = fx fy cx cy of
 * slot k (mK1 / mK2, :105-106); level_sigma2 is HOST memory, mvLevelSigma2 of nlevels entries (one scale pyramid for all slots).
 *   a correspondence  keyframe-1 row i1 < n[kf1] with 0 <= m = d_matches12[p*cap + i1] < n[kf2], valid[kf1][i1], valid[kf2][m] and both octaves in [0, nlevels).  The list in
 *         ascending i1 is mvnIndices1; N is its length.  The reference's GetIndexInKeyFrame lookups (:75-79) are the rows themselves: a map point observed at row i of a keyframe
 *         has index i there.  A caller that knows otherwise (the lookup would give -1 or another row) clears d_valid for that row.
 *   gates  mvnMaxError is a vector<size_t> (include/Sim3Solver.h:78-79): a correspondence is an inlier when both squared errors are < the INTEGER part of 9.210 * sigma2[octave]
 *         (13 for sigma2 = 1.44, not 13.26).
 *   d_state, in/out, one per pair, is the solver object: zero-filled = a new Sim3Solver, and repeated calls resume exactly as repeated iterate(new_iterations, ..) calls do
 *         (mnIterations and the best hypothesis carry over; after a return best_inliers stays raised).  new_iterations is iterate's nIterations: 5 in LoopClosing (:296),
 *         max_iterations for find().  probability, min_inliers, max_iterations are SetRansacParameters' (0.99, 20, 300 at :284); max_its = mRansacMaxIts for the pair's N, from a
 *         table of cap + 1 entries the context keeps and rebuilds (on the host, with libm) only when (probability, min_inliers, max_iterations, cap) change.  iterate returns
 *         at the first iteration whose count is >= every earlier one (best_inliers included) and > min_inliers; among equal counts the later iteration becomes the best.
 *         N < min_inliers: nothing is iterated, no_more = 1, max_its = 0 and the in/out words keep their values.  Otherwise no_more = 1 when the call did not return a
 *         hypothesis and its_done >= max_its afterwards (bNoMore, :203; a return leaves it 0, as :142 does).
 *         A pair with a slot outside [0, nkeyframes) is skipped: n = 0, no_more = 1, found_it = -1, max_its = n_inliers = 0; its in/out words and d_inliers rows are not written.
 *   d_inliers[p*cap + i1], i1 < n[kf1]: 1 for an inlier of the returned hypothesis (vbInliers, :195-197), else 0; all 0 when found_it < 0.  Rows at or past the count are not
 *         touched.
 *   d_sets  NULL: iteration `it` of pair p draws as :166-177 do with randi = hash32(seed, p, it, j) % remaining (csrc/ransac_draw.h states hash32); with N < 3 nothing can
 *         be drawn and the iteration counts as one with an index out of range.  Otherwise d_sets[(p*max_iterations + it)*3 + j] are indices into the correspondence list by
 *         ABSOLUTE iteration number (equal indices are legal); a set with an index outside [0, N) makes a hypothesis that never becomes the best and never returns.
 * What the reference leaves to OpenCV and libm (cv::eigen, atan2 + cv::Rodrigues, the matrix expressions, cv::reduce, cv::pow) is restated by decision D16 of DESIGN.md;
 * everything else is the reference's arithmetic operation for operation (csrc/sim3_math.h).
 * One launch on `stream` (NULL: the context's stream) behind at most one upload of the table, no synchronise; every pointer but level_sigma2 is a device pointer; every output
 * word has one writer.  SSLAM_ERR_INVALID (nothing enqueued): a NULL ctx or pointer other than d_valid and d_sets, a typed buffer that is not 4-byte aligned, cap < 1,
 * nkeyframes < 0, npairs < 0, nlevels outside 1 .. 64, min_inliers < 1, max_iterations < 1, new_iterations < 1, probability not in (0, 1), npairs * cap or nkeyframes * cap
 * >= 2^31, with d_sets npairs * max_iterations >= 2^28.  SSLAM_ERR_UNSUPPORTED (nothing enqueued): cap > 3072 (the correspondences sit in LDS, 48 bytes each).  npairs == 0 is
 * SSLAM_OK and enqueues nothing.  The single call takes one pair from host memory (valid1 and valid2 both NULL or both given), runs it as pair 0 of the same kernel with
 * cap = max(n1, n2) and synchronises; sets holds max_iterations x 3 indices. */
typedef struct sslam_sim3_state {      /* 84 bytes, no padding; zero-filled = a new Sim3Solver */
    int32_t its_done;        /* in/out  mnIterations */
    int32_t best_inliers;    /* in/out  mnBestInliers */
    int32_t best_it;         /* in/out  iteration that holds the best, -1 none yet (read as -1 when its_done == 0) */
    int32_t n;               /* out     N: correspondences the call saw */
    int32_t max_its;         /* out     mRansacMaxIts after SetRansacParameters; 0 when n < min_inliers */
    int32_t found_it;        /* out     the iteration iterate() returned at, -1 when it returned empty */
    int32_t n_inliers;       /* out     nInliers of that return, else 0 */
    int32_t no_more;         /* out     bNoMore */
    float s12, R12[9], t12[3];  /* in/out  mBestScale / mBestRotation / mBestTranslation (row-major) */
} sslam_sim3_state;
int sslam_sim3_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp, const float* d_x3dc, const uint8_t* d_valid,
        const int32_t* d_n, int cap, int nkeyframes, const float* d_K /* [nkeyframes*4] fx fy cx cy */,
        const float* level_sigma2 /* HOST, nlevels */, int nlevels,
        const int32_t* d_pairs, int npairs, const int32_t* d_matches12,
        int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations,
        const int32_t* d_sets /* NULL or [npairs*max_iterations*3] */, uint32_t seed,
        sslam_sim3_state* d_state /* [npairs] in/out */, uint8_t* d_inliers /* [npairs*cap] */, void* stream);
int sslam_sim3_ransac(sslam_ctx* ctx, const sslam_keypoint* kp1, const float* x3dc1, const uint8_t* valid1, int n1, const float K1[4],
        const sslam_keypoint* kp2, const float* x3dc2, const uint8_t* valid2, int n2, const float K2[4],
        const float* level_sigma2, int nlevels, const int32_t* matches12,
        int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations,
        const int32_t* sets /* NULL or [max_iterations*3] */, uint32_t seed,
        sslam_sim3_state* state /* in/out */, uint8_t* inliers /* [n1] */);

/* PnPsolver (src/PnPsolver.cc), the pose RANSAC of Tracking::Relocalization (src/Tracking.cc:2004-2030) between SearchByBoW (:1996, sslam_orb_search_by_bow_batch_dev)
 * and SearchByProjection (:2071, :2085, sslam_search_by_projection_batch_dev): one iterate(new_iterations, ..) call (:165-258) for `npairs` (keyframe, frame) pairs of
 * device-resident slots, asynchronously.  The layouts and the pair arrays are those of sslam_orb_search_by_bow_batch_dev: frame slot f owns rows [f*cap, f*cap + d_nf[f])
 * of d_f_kp (mvKeysUn) and d_f_K[4f .. 4f+4) = fx fy cx cy; keyframe slot k owns rows [k*kfcap, k*kfcap + d_nkf[k]) of d_kf_xw (three floats a row: GetWorldPos of the
 * keyframe's map point, the caller fills it) and d_kf_valid (= vpMapPointsKF[i] && !isBad(); NULL: all valid).  A count below 0 is read as 0, one above its capacity as
 * the capacity.  Pair p takes keyframe slot d_pair_kf[p] and frame slot d_pair_f[p]; either array may be NULL, which means slot p and requires that side's slot count
 * to equal npairs.  A pair with a slot outside its range is skipped: its state reads n = min_inliers = max_its = found = n_inliers = 0, found_it = -1, no_more = 1 and
 * nothing else of it is written.  d_assigned[p*cap + j] is what the matcher wrote and is read where it lies.
 * The constructor (:67-110): frame row j < nf is a correspondence when 0 <= a = d_assigned[p*cap + j] < nkf, keyframe row a is valid and the keypoint's octave lies in
 * [0, nlevels); the list is in ascending j (mvKeyPointIndices) and has N entries; mvMaxError = level_sigma2[octave] * th2 in float (:156).  SetRansacParameters
 * (:121-157) with the minimal set of four: the adjusted mRansacMinInliers and mRansacMaxIts of every N come from a table that the context builds on the host with libm and
 * keeps on the device until (probability, min_inliers, max_iterations, epsilon, cap) change.  iterate's loop condition (:182) is an OR: a call runs up to iteration
 * max(max_its, its_done + new_iterations), so the first call runs all max_its iterations unless it returns.  An iteration whose count is >= min_inliers becomes the best
 * when it is strictly greater than every earlier one, then Refine (:260-305) runs on the best set and the call returns when the refined count is > min_inliers
 * (found = 1, :226-236); the call after such a return returns again at its first qualifying iteration.  A call that ends with its_done >= max_its sets no_more and, with
 * best_inliers >= min_inliers, returns the unrefined best (found = 2, :241-255).  d_inliers[p*cap + j], j < nf, = vbInliers of the return by frame row (0 without
 * one); rows at or past the frame's count are not touched.  The OpenCV leaves of EPnP (:375-950) are decision D17 of DESIGN.md.
 * The draw: DUtils::Random::RandomInt is replaced by hash32(seed, pair, iteration, j) (csrc/ransac_draw.h).  With d_sets, iteration `it` of pair p takes the four
 * indices d_sets[(p*nsets + it)*4 ..) into the correspondence list; a set for an iteration >= nsets or with an index outside [0, N) makes a hypothesis that never
 * qualifies; equal indices are legal.
 * level_sigma2 is HOST memory (nlevels floats, 1 .. 64); every other pointer is a device pointer, 4-byte aligned, d_state 8-byte.  One launch on `stream` (NULL: the
 * context's stream), no synchronise, no host memory touched but the table's upload.  SSLAM_ERR_INVALID (nothing enqueued): a NULL buffer other than d_kf_valid, the pair
 * arrays and d_sets, a misaligned one, probability outside (0, 1), min_inliers, max_iterations or new_iterations < 1, epsilon outside (0, 1], th2 <= 0 or NaN, cap or
 * kfcap < 1, npairs * cap, nframes * cap or nkeyframes * kfcap >= 2^31, with d_sets npairs * nsets >= 2^28, a NULL pair array whose side has another slot count than
 * npairs.  SSLAM_ERR_UNSUPPORTED (nothing enqueued): cap > 2048 (the correspondences sit in LDS, 24 bytes each, beside the EPnP workspace).  npairs == 0 is SSLAM_OK and
 * enqueues nothing.  The single call takes one pair from host memory, runs it as pair 0 of the same kernel with cap = nf rounded up to a multiple of 512 (one table serves candidates of different sizes) and synchronises. */
typedef struct sslam_pnp_state {       /* 192 bytes, no padding; zero-filled = a new PnPsolver */
    int32_t its_done;        /* in/out  mnIterations */
    int32_t best_inliers;    /* in/out  mnBestInliers */
    int32_t best_it;         /* in/out  iteration that holds the best, -1 none yet (read as -1 when its_done == 0) */
    int32_t refine_ok;       /* in/out  whether Refine of the best set succeeds; 0 while there is no best */
    int32_t n;               /* out     N: correspondences the call saw */
    int32_t min_inliers;     /* out     the adjusted mRansacMinInliers */
    int32_t max_its;         /* out     mRansacMaxIts; 0 when n < min_inliers */
    int32_t found;           /* out     0 none, 1 the refined pose (:226-236), 2 the best at exhaustion (:244-253) */
    int32_t found_it;        /* out     found 1: the iteration iterate() returned at; found 2: best_it; else -1 */
    int32_t n_inliers;       /* out     nInliers of that return, else 0 */
    int32_t no_more;         /* out     bNoMore */
    int32_t pad_;            /* keeps the doubles 8-byte aligned; not written */
    double  best_R[9], best_t[3];   /* in/out  mRi / mti of the best iteration (row-major) */
    float   Tcw[12];         /* out     rows 0 .. 2 of the returned 4 x 4, float as :217-223 / :294-300; zeros without a return */
} sslam_pnp_state;
int sslam_pnp_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_f_kp, const int32_t* d_nf, int cap, int nframes, const float* d_f_K /* [nframes*4] */,
        const float* d_kf_xw /* [nkeyframes*kfcap*3] */, const uint8_t* d_kf_valid, const int32_t* d_nkf, int kfcap, int nkeyframes,
        const float* level_sigma2 /* HOST, nlevels */, int nlevels,
        const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs, const int32_t* d_assigned,
        double probability, int min_inliers, int max_iterations, float epsilon, float th2, int new_iterations,
        const int32_t* d_sets /* NULL or [npairs*nsets*4] */, int nsets, uint32_t seed,
        sslam_pnp_state* d_state /* [npairs] in/out */, uint8_t* d_inliers /* [npairs*cap], by frame row */, void* stream);
int sslam_pnp_ransac(sslam_ctx* ctx, const sslam_keypoint* f_kp, int nf, const float f_K[4], const float* kf_xw, const uint8_t* kf_valid, int nkf,
        const float* level_sigma2, int nlevels, const int32_t* assigned /* [nf] */,
        double probability, int min_inliers, int max_iterations, float epsilon, float th2, int new_iterations,
        const int32_t* sets /* NULL or [nsets*4] */, int nsets, uint32_t seed,
        sslam_pnp_state* state /* in/out */, uint8_t* inliers /* [nf] */);

/* The projection-window matcher family.  The tracker keeps the projection / visibility logic (poses, map
 * points: host state) and hands over one query per map point or map line; the device replays the
 * window search, the best/second-best Hamming selection, the level-consistent ratio test, the
 * "keypoint already taken" rule and the rotation-histogram pruning of:
 *   kind 0, mode 0  ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)   src/ORBmatcher.cc:45-129
 *   kind 0, mode 1  ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)        src/ORBmatcher.cc:1331-1473
 *   kind 1, mode 0  LSDmatcher::SearchByProjection(Frame&, const vector<MapLine*>&, th)    src/LSDmatcher.cpp:185-255
 *                   LSDmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)        src/LSDmatcher.cpp:22-141
 * Mode 1 is the "best candidate only, a feature that already holds a map point is skipped" rule; three more overloads are the same
 * rule under other arguments (each checked against its own line-by-line restatement, tests/test_match_gpu.py):
 *   kind 0, mode 1  ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)  src/ORBmatcher.cc:1475-1602 (relocalisation):
 *                   occupied[i] = CurrentFrame.mvpMapPoints[i] != NULL, obs_positive = 1, uright = NULL, th_dist = ORBdist,
 *                   min/max_level = pred-1 / pred+1, angle = pKF->mvKeysUn[i].angle
 *   kind 0, mode 1  ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)        src/ORBmatcher.cc:293-406 (loop closing):
 *                   occupied[i] = vpMatched[i] != NULL, obs_positive = 1, uright = NULL, th_dist = TH_LOW, check_orientation = 0,
 *                   min/max_level = pred-1 / pred (KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:610-649, scans like Frame's)
 *   kind 1, mode 1  LSDmatcher::SearchByProjection(KeyFrame*, Scw, vpLines, vpMatched, th)         src/LSDmatcher.cpp:558-683: as the line above
 *                   with both projected endpoints (kind 1 accepts mode 1 only with check_orientation = 0)
 * feats = F.mvKeysUn (sslam_keypoint) or F.mvKeylinesUn (sslam_keyline), desc = F.mDescriptors / F.mLdesc,
 * uright = F.mvuRight or NULL (monocular), occupied[i] = F.mvpMapPoints[i] has Observations()>0 (or NULL).
 * assigned_out[i] = index of the query now owning feature i (-> F.mvpMapPoints[i] = that pMP), -1 if no query touched it (the pointer
 * keeps its value), or -2 (mode 1 with check_orientation only) if it was matched and then removed by the rotation-consistency check
 * (the reference writes NULL there, src/ORBmatcher.cc:1465, :1596). */
typedef struct sslam_proj_query {
    float u, v;            /* window centre (mTrackProjX/Y or projected u,v); lines: first projected endpoint */
    float u2, v2;          /* lines: second projected endpoint */
    float radius;          /* r * mvScaleFactors[level] resp. th * mvScaleFactors[octave] */
    int32_t min_level, max_level;   /* the GetFeaturesInArea / GetLinesInArea level arguments */
    float angle;           /* mode 1: LastFrame.mvKeysUn[i].angle (rotation histogram) */
    float ur;              /* stereo: mTrackProjXR resp. u - mbf*invzc; ignored when uright == NULL */
    int32_t valid;         /* 0: skipped (not in view, bad, outlier, behind the camera, outside the image) */
    int32_t obs_positive;  /* the map point / line has Observations() > 0 */
} sslam_proj_query;
int sslam_search_by_projection(sslam_ctx* ctx, int kind, int mode, const void* feats, const uint8_t* desc, int n,
                               const float bounds[4], const float* uright, const uint8_t* occupied,
                               const sslam_proj_query* queries, const uint8_t* qdesc, int nq,
                               float nnratio, int th_dist, int check_orientation,
                               int32_t* assigned_out, int* nmatches_out);

/* ---- device-resident frames (no single reference function: replaces the re-upload of
 * Frame::mvKeysUn / mDescriptors / mvKeylinesUn / mLdesc (include/Frame.h:155-189) around every matcher call) -------------
 * A frame handle owns device copies of one Frame's features (kind 0: sslam_keypoint rows, 1: sslam_keyline rows), their
 * 32-byte descriptors, optionally mvuRight, and the image bounds {mnMinX, mnMaxX, mnMinY, mnMaxY}. */
typedef struct sslam_frame sslam_frame;
int sslam_frame_upload(sslam_ctx* ctx, int kind, const void* feats, const uint8_t* desc, int n, const float* uright, const float bounds[4],
                       sslam_frame** out);
/* Snapshot (device to device) of what the last sslam_orb_extract / sslam_lines_extract call on this handle produced:
 * Frame::ExtractORB / ExtractLSD (src/Frame.cc:150-161) followed by the matchers without any upload. */
int sslam_frame_from_orb(sslam_orb* orb, const float bounds[4], sslam_frame** out);
int sslam_frame_from_lines(sslam_lines* lines, const float bounds[4], sslam_frame** out);
void sslam_frame_destroy(sslam_frame* frame);
int sslam_frame_count(const sslam_frame* frame);
/* sslam_search_by_projection with the frame's features taken from the handle (same kernels, same results). */
int sslam_search_by_projection_frame(sslam_ctx* ctx, const sslam_frame* frame, int mode, const uint8_t* occupied,
                                     const sslam_proj_query* queries, const uint8_t* qdesc, int nq,
                                     float nnratio, int th_dist, int check_orientation, int32_t* assigned_out, int* nmatches_out);
/* sslam_search_by_projection for `nframes` independent frames whose features are already on the device, asynchronously: the batch form of the
 * matcher a tracker runs on every frame after initialisation (TrackWithMotionModel, SearchLocalPoints and the LSDmatcher twins), for callers that
 * extract many sessions' frames in one launch.  The layout is the batch extractors': frame f owns rows [f*cap, f*cap + d_n[f]) of d_feats
 * (kind 0: sslam_keypoint, kind 1: sslam_keyline), d_desc (32 bytes per row) and, where given, d_uright and d_occupied (NULL: as in the single
 * call), so the outputs of sslam_orb_extract_batch_dev / sslam_undistort_keypoints_batch_dev / sslam_lines_extract_batch_dev are inputs here
 * without a copy; it owns rows [f*qcap, f*qcap + d_nq[f]) of d_queries and d_qdesc.  A count below 0 is read as 0, one above its capacity as
 * the capacity.  kind, mode, bounds, nnratio, th_dist and check_orientation are shared by all frames and mean what they mean in the single call.
 * d_assigned[f*cap + i], i < n[f], receives what sslam_search_by_projection writes to assigned_out[i] for that frame (query index, -1, or -2
 * after the rotation check); rows at or past a frame's count are not touched.  d_nmatches[f] = the frame's match count (0 for a frame without
 * features or without queries, whose valid rows are still set to -1).
 * Every pointer is a device pointer except bounds; d_desc and d_qdesc are 16-byte aligned.  The call enqueues on `stream` (NULL: the context's
 * stream) and returns without synchronising; it reads no host memory but bounds and writes none.  SSLAM_ERR_INVALID (nothing enqueued): the
 * single call's rules (kind / mode 0 or 1, no kind 1 with mode 1 and check_orientation, cap < 2^19), a negative cap, qcap or nframes, a NULL or
 * misaligned buffer.  nframes == 0 is SSLAM_OK and enqueues nothing.
 * Scratch: the context owns one arena for this call, apart from the synchronous matchers' (a synchronous matcher may run on the context stream
 * while a batch runs on another).  The batch runs in slices of frames, in stream order, so the arena does not grow with nframes: per frame of a
 * slice 8*(cap + qcap) + 68*qcap bytes (the per-query top-8 lists and counts, the per-frame rotation bins), at most 256 MiB (+ 768 bytes of
 * alignment) per context in all, or one frame's worth where a single frame needs more.  Calls on different streams of one context are ordered
 * on the arena by an event (the later call's kernels wait for the earlier call's); a call that needs a larger arena than the context holds
 * waits on the host for the previous call before it replaces it -- the only case in which the call blocks. */
int sslam_search_by_projection_batch_dev(sslam_ctx* ctx, int kind, int mode,
                                         const void* d_feats, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes, const float bounds[4],
                                         const float* d_uright, const uint8_t* d_occupied,
                                         const sslam_proj_query* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int qcap,
                                         float nnratio, int th_dist, int check_orientation,
                                         int32_t* d_assigned, int32_t* d_nmatches, void* stream);
/* sslam_hamming_knn2 between the descriptors of two frame handles (cv::BFMatcher::knnMatch(d1, d2, m, 2),
 * src/LSDmatcher.cpp:150,261,293,336,387). */
int sslam_hamming_knn2_frames(sslam_ctx* ctx, const sslam_frame* query, const sslam_frame* train, int32_t* idx, int32_t* dist);

/* The candidate search of the Fuse family on a device-resident keyframe:
 *   ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)            src/ORBmatcher.cc:828-960   chi2_mode 1 (stereo 7.8 / mono 5.99 gates, :913-936)
 *   ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th, vpReplacePoint) :962-1103 chi2_mode 0
 *   LSDmatcher::Fuse(KeyFrame*, const vector<MapLine*>&, th)             src/LSDmatcher.cpp:417-548  chi2_mode 0, keyline frame
 * One sslam_proj_query per projected map point / line: u,v (and u2,v2 for lines), radius = th*mvScaleFactors[pred], ur,
 * min_level = pred-1, max_level = pred, valid.  best_idx_out[q] = the feature with the smallest descriptor distance in the
 * window (first in KeyFrame::GetFeaturesInArea / GetLinesInArea order on ties, src/KeyFrame.cc:610-683), -1 if none;
 * best_dist_out[q] = that distance (INT_MAX if none).  inv_level_sigma2 = KeyFrame::mvInvLevelSigma2 (chi2_mode 1 only).
 * The `bestDist <= TH_LOW` test and the Replace / AddObservation bookkeeping stay with the caller, in query order.
 * The same inner loop (chi2_mode 0) is the candidate search of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1196-1227, :1276-1307,
 * gate TH_HIGH), LSDmatcher::SearchBySim3 (src/LSDmatcher.cpp:685-929) and LSDmatcher::Fuse(KeyFrame*, Scw, ...) (:931-1063).  The
 * loop-closing SearchByProjection(KeyFrame*, Scw, ...) overloads skip features that are already matched, which makes their queries
 * order dependent: they are sslam_search_by_projection mode 1 (above), not this function. */
int sslam_fuse_search(sslam_ctx* ctx, const sslam_frame* keyframe, int chi2_mode, const float* inv_level_sigma2, int nlevels,
                      const sslam_proj_query* queries, const uint8_t* qdesc, int nq, int32_t* best_idx_out, int32_t* best_dist_out);

/* The same candidate search for `njobs` jobs on device-resident keyframes, asynchronously: the fusion step of LocalMapping::SearchInNeighbors
 * (src/LocalMapping.cc:1178-1284, the calls at :1206, :1226, :1243, :1264) and the two directions of SearchBySim3 for callers that keep many sessions'
 * keyframes on the device.  The pool is sslam_orb_search_for_triangulation_batch_dev's: keyframe slot k owns rows [k*cap, k*cap + d_n[k]) of d_feats
 * (kind 0: sslam_keypoint, kind 1: sslam_keyline), of d_desc (32 bytes per row) and, where given, of d_uright.  A count below 0 is read as 0, one
 * above cap as cap; nothing at or past a count is read.  A NULL d_uright means monocular, as in the single call on a handle without right coordinates.
 * Job j = d_jobs[j] searches keyframe slot kf with nq queries (clamped to [0, qcap]): it owns rows [j*qcap, j*qcap + nq) of d_queries, d_best_idx and
 * d_best_dist, and its query i reads descriptor row qdesc0 + i of d_qdesc (nqdesc rows in all).  Several jobs may name one qdesc0 -- the current
 * keyframe's map points projected into 20 neighbours are 20 jobs on ONE descriptor block, each with its own windows -- and several jobs one slot.
 * For i < nq, d_best_idx[j*qcap + i] / d_best_dist[j*qcap + i] receive exactly what sslam_fuse_search returns for that query on that keyframe with the
 * same kind, chi2_mode, bounds and level table: ties go to the first in GetFeaturesInArea / GetLinesInArea order, -1 / INT_MAX for a query with
 * valid == 0 or without an admissible feature, the 5.99 / 7.8 gates under chi2_mode 1, an octave outside [0, nlevels) gated with a weight of 0.
 * Rows at or past nq are not touched.  d_nfound[j] = the number of the job's queries with a candidate.  A job whose kf is outside [0, nkeyframes),
 * whose qdesc0 is below 0 or whose qdesc0 + nq (after the clamp) is above nqdesc is skipped: d_nfound[j] = -1 and nothing else of it is written.
 * WHY ONE CALL IS EXACT: the candidate search of a query depends on nothing another query did.  The reference's inner loop (src/ORBmatcher.cc:897-952,
 * :1055-1080, src/LSDmatcher.cpp:497-523) reads the keyframe's features, their descriptors and levels, and nothing the bookkeeping behind it
 * (Replace / AddMapPoint / AddObservation, ORBmatcher.cc:955-975) writes: that bookkeeping can make LATER map points bad or IsInKeyFrame -- which
 * decides whether the reference runs their search at all -- but it never moves a window or changes a descriptor.  So every neighbour of a keyframe,
 * both directions of SearchInNeighbors and both directions of SearchBySim3 fit in one call, where the triangulation batch needs one call per round.
 * The caller replays the bookkeeping in the reference's order (job by job, query by query: `bestDist <= TH_LOW`, then Replace or AddObservation) and
 * DROPS the result of a query whose map point or line has become bad or attached to that keyframe meanwhile: the reference would have skipped it
 * (:852-853), and a skipped query changes nothing for the others.
 * inv_level_sigma2 is a HOST array of nlevels floats (1 <= nlevels <= 64, chi2_mode 1 only; ignored under chi2_mode 0), read before the call returns;
 * bounds is host memory too.  Every other pointer is a device pointer; d_desc and d_qdesc are 16-byte aligned, the typed buffers 4-byte aligned.
 * The call enqueues a clear of d_nfound and one launch on `stream` (NULL: the context's stream), uses no scratch, does not synchronise and is
 * independent of every other call on the context.  SSLAM_ERR_INVALID (nothing enqueued): kind or chi2_mode not 0 or 1, chi2_mode 1 with kind 1,
 * without a table or with nlevels outside 1..64; a NULL ctx, d_feats, d_desc, d_n, bounds, d_queries, d_qdesc, d_jobs, d_best_idx, d_best_dist or
 * d_nfound; a misaligned buffer; a negative cap, qcap, nkeyframes, njobs or nqdesc; cap >= 2^19; njobs * qcap >= 2^31; njobs * max(1, ceil(qcap /
 * 256)) >= 2^31 workgroups.  njobs == 0 is SSLAM_OK and enqueues nothing; qcap == 0 with njobs > 0 is SSLAM_OK and writes d_nfound alone (0, or -1
 * for a skipped job). */
typedef struct sslam_fuse_job {
    int32_t kf;       /* keyframe slot searched (pKF) */
    int32_t nq;       /* queries of this job */
    int32_t qdesc0;   /* first descriptor row of this job in d_qdesc */
} sslam_fuse_job;     /* 12 bytes, no padding */
int sslam_fuse_search_batch_dev(sslam_ctx* ctx, int kind, int chi2_mode,
                                const void* d_feats, const uint8_t* d_desc, const float* d_uright, const int32_t* d_n, int cap, int nkeyframes,
                                const float bounds[4], const float* inv_level_sigma2, int nlevels,
                                const sslam_proj_query* d_queries, int qcap, const uint8_t* d_qdesc, int nqdesc,
                                const sslam_fuse_job* d_jobs, int njobs,
                                int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfound, void* stream);

/* ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t,size_t>>&, bOnlyStereo),
 * src/ORBmatcher.cc:660-826 (epipolar test CheckDistEpipolarLine :140-157), on two device-resident keyframes (their
 * mvuRight are in the handles).  free1[i] / free2[i] = !GetMapPoint(i); the two FeatureVectors as CSR lists over the shared
 * vocabulary nodes in ascending node id (see sslam_orb_search_by_bow); F12 row-major (F12.at<float>(r,c) = F12[3r+c]);
 * (ex, ey) = epipole in image 2 (:667-673); scale_factors2 = pKF2->mvScaleFactors, level_sigma2_2 = pKF2->mvLevelSigma2.
 * matches12_out[i1] = matched keyframe-2 feature or -1 (the reference's vMatches12 after the rotation-histogram pruning). */
int sslam_orb_search_for_triangulation(sslam_ctx* ctx, const sslam_frame* kf1, const sslam_frame* kf2, const uint8_t* free1, const uint8_t* free2,
                                       const int32_t* node_kf1_ptr, const int32_t* node_kf2_ptr, int nnodes, const int32_t* kf1_idx, const int32_t* kf2_idx,
                                       const float F12[9], float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int nlevels,
                                       int only_stereo, int check_orientation, int32_t* matches12_out, int* nmatches_out);

/* The same matcher (src/ORBmatcher.cc:660-826) for `npairs` pairs of device-resident keyframes, asynchronously, from per-feature node ids instead of
 * CSR lists: the point half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:367-640, the call at :440) for callers that keep many sessions'
 * keyframes on the device.  Both sides of a pair are keyframes of the same maps, so there is ONE pool: keyframe slot k owns rows
 * [k*cap, k*cap + d_n[k]) of d_kp (mvKeysUn; sslam_undistort_keypoints_batch_dev), d_desc (32 bytes per row; sslam_orb_extract_batch_dev), d_node
 * (what sslam_bow_transform_batch_dev writes to d_node; a row with an id below 0 is in no node) and, where given, d_free (= !GetMapPoint(i)) and
 * d_uright (mvuRight).  A NULL d_free means every row is free; a NULL d_uright means monocular, so with only_stereo nothing matches.  A count below
 * 0 is read as 0, one above cap as cap; node ids, free flags and right coordinates at or past a count are never read.
 * Pair p = d_pairs[p]: kf1 is pKF1 (the queries), kf2 is pKF2 (the candidates), F12 row-major and (ex, ey) the epipole in image 2 as in the single
 * call.  scale_factors / level_sigma2 are HOST arrays of nlevels floats, 1 <= nlevels <= 64, shared by all pairs (pKF2's mvScaleFactors /
 * mvLevelSigma2: one extractor); they are read before the call returns, no other host memory is read and none is written.  An octave outside
 * [0, nlevels) is clamped into it, as in the single call.
 * Pair p yields exactly what sslam_orb_search_for_triangulation returns for the two FeatureVectors FeatureVector::addFeature(node[i], i) builds in
 * feature order from the two node arrays: d_matches12[p*cap + i1], i1 < n[kf1], = the matched keyframe-2 row or -1, after the rotation pruning;
 * rows at or past the count are not touched.  d_nmatches[p] = the count after the pruning.  A pair with a slot outside [0, nkeyframes) is skipped:
 * d_nmatches[p] = 0 and nothing else of the pair is written.  kf1 == kf2 is legal and computed like any other pair.
 * THE LIMIT: CreateNewMapPoints adds every newly triangulated point to the current keyframe INSIDE its neighbour loop (src/LocalMapping.cc:624), so
 * in the reference the free flags of keyframe 1 for neighbour j + 1 depend on the geometry of neighbour j; with the rotation check on a caller cannot
 * repair that afterwards by dropping matches, because the dropped matches took part in the histogram.  The exact use is therefore one pair per
 * session per round: round r matches every session's new keyframe against its r-th neighbour, and the caller updates its d_free rows between
 * rounds.  Naming one keyframe slot in many pairs of one call is allowed and well defined -- every such pair sees the same free flags -- but it is
 * NOT the reference's sequential loop.
 * Every pointer but the two level tables is a device pointer; d_desc is 16-byte aligned, the 4-byte typed buffers 4-byte aligned.  One launch on
 * `stream` (NULL: the context's stream), no scratch, no synchronise; calls on any streams of one context are independent of each other and of the
 * synchronous matchers.  SSLAM_ERR_INVALID (nothing enqueued): a NULL ctx, d_kp, d_desc, d_node, d_n, d_pairs, d_matches12, d_nmatches,
 * scale_factors or level_sigma2, a misaligned buffer, a negative cap, nkeyframes or npairs, cap >= 2^19, nlevels outside 1..64,
 * npairs * cap >= 2^31.  npairs == 0 is SSLAM_OK and enqueues nothing. */
typedef struct sslam_tri_pair {
    int32_t kf1, kf2;     /* keyframe slots: pKF1 (the queries), pKF2 (the candidates) */
    float   F12[9];       /* row-major, as in the single call */
    float   ex, ey;       /* epipole in image 2 (src/ORBmatcher.cc:667-673) */
} sslam_tri_pair;         /* 52 bytes, no padding */
int sslam_orb_search_for_triangulation_batch_dev(sslam_ctx* ctx,
                                                 const sslam_keypoint* d_kp, const uint8_t* d_desc, const int32_t* d_node,
                                                 const uint8_t* d_free, const float* d_uright, const int32_t* d_n, int cap, int nkeyframes,
                                                 const sslam_tri_pair* d_pairs, int npairs,
                                                 const float* scale_factors, const float* level_sigma2, int nlevels,
                                                 int only_stereo, int check_orientation,
                                                 int32_t* d_matches12, int32_t* d_nmatches, void* stream);

/* The geometry behind that matcher: the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:456-635) for every match of `npairs` pairs of
 * device-resident keyframes, asynchronously, with the first MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:335-376) of every new point.  It reads d_matches12 where
 * sslam_orb_search_for_triangulation_batch_dev left it and clears the free flags of the rows it turns into points, so THE LIMIT above needs no host round trip any more:
 * per round r enqueue the matcher and then this call on ONE stream with the SAME d_free (one pair per session per round), enqueue all 20 rounds back to back and
 * synchronise once.  The caller then creates the MapPoints from the rows with d_stage == 0 in row order -- ascending keypoint-1 index, the order of the reference's
 * vMatchedIndices -- and keeps AddObservation, AddMapPoint and the map as host bookkeeping; sslam_distinctive_descriptors_batch_dev takes it from there.  The baseline /
 * median-depth gate of :413-431 stays with the caller, in front of the matcher: such a pair is simply not listed.
 * The pool is the matcher's: keyframe slot k owns rows [k*cap, k*cap + d_n[k]) of d_kp (mvKeysUn) and, where given, of d_free; d_pose[k] is what KeyFrame::SetPose and
 * the constructor keep for it.  Pair p = d_pairs[p]: kf1 is mpCurrentKeyFrame, kf2 is pKF2 (median_depth2 is not read here).  scale_factors / level_sigma2 are HOST
 * arrays of nlevels floats, 1 <= nlevels <= 64 (mvScaleFactors / mvLevelSigma2: one extractor), read before the call returns; scale_factor is mfScaleFactor
 * (ratioFactor = 1.5f * scale_factor, :400).  An octave outside [0, nlevels) is clamped into it, as the matchers clamp it.  This fork is monocular (only
 * GrabImageMonocularWithPL exists), so every mvuRight is negative and the bStereo branches (:488-491, :518-525, :560-570, :587-597) do not exist here: there is no d_uright.
 * Row i1 < n[kf1] of pair p (outputs are indexed p*cap + i1; rows at or past the count are not touched):
 *   d_stage   0 created
 *             1 no match (d_matches12 < 0 or >= n[kf2])
 *             2 parallax (:497 false, the continue of :527)        3 x3D(3) == 0 (:511)
 *             4 z1 <= 0 (:534)        5 z2 <= 0 (:538)        6 reprojection in keyframe 1 (:557)        7 reprojection in keyframe 2 (:584)
 *             8 dist1 == 0 || dist2 == 0 (:607)        9 scale consistency (:615)
 *   d_x3d     x3D (:515); d_normal, d_dist = mNormalVector and (mfMaxDistance, mfMinDistance) of UpdateNormalAndDepth for the observations {kf1: i1, kf2: i2} with
 *             mpRefKF = keyframe 1 (level = kp1.octave, min = max / scale_factors[nlevels - 1]).  All of them are zero for a row that is not created.
 * d_nnew[p] = the number of created rows (nnew).  When d_free is given, a created row stores 0 to d_free[kf1*cap + i1] and d_free[kf2*cap + i2] (AddMapPoint, :624-625);
 * d_free is not read.  A NaN behaves as the reference's comparisons make it behave.  A pair with a slot outside [0, nkeyframes) or with kf1 == kf2 (the reference never
 * pairs a keyframe with itself) is skipped: d_nnew[p] = -1 and nothing else of the pair is written.
 * Every pointer but the two level tables is a device pointer, the 4-byte typed buffers 4-byte aligned.  One launch on `stream` (NULL: the context's stream), no
 * scratch, no synchronise.  SSLAM_ERR_INVALID (nothing enqueued): a NULL ctx or pointer other than d_free, a misaligned buffer, a negative cap, nkeyframes or npairs,
 * nlevels outside 1..64, npairs * cap or nkeyframes * cap >= 2^31.  npairs == 0 is SSLAM_OK and enqueues nothing. */
typedef struct sslam_kf_pose {    /* 84 bytes: what KeyFrame::SetPose and the constructor keep, per pool slot */
    float Rcw[9], tcw[3], Ow[3];  /* GetRotation (row-major), GetTranslation, GetCameraCenter */
    float fx, fy, cx, cy, invfx, invfy;
} sslam_kf_pose;
typedef struct sslam_newmap_pair {
    int32_t kf1, kf2;             /* keyframe slots: mpCurrentKeyFrame, pKF2 */
    float   median_depth2;        /* pKF2->ComputeSceneMedianDepth(2); read by the line call only */
} sslam_newmap_pair;              /* 12 bytes, no padding */
int sslam_new_map_points_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp, const int32_t* d_n, int cap, int nkeyframes, const sslam_kf_pose* d_pose,
                                   const sslam_newmap_pair* d_pairs, int npairs, const int32_t* d_matches12,
                                   const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                                   uint8_t* d_free, float* d_x3d, uint8_t* d_stage, float* d_normal, float* d_dist, int32_t* d_nnew, void* stream);
/* The same for one host pair, synchronously: pair 0 of the same kernel on a pool of two slots.  Outputs [n1] rows; *nnew = the number of created rows. */
int sslam_new_map_points(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const sslam_kf_pose* pose1, const sslam_kf_pose* pose2,
                         const int32_t* matches12, const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                         float* x3d, uint8_t* stage, float* normal, float* dist, int* nnew);

/* The loop body of LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:1005-1170) with the GetMapLine filter of LSDmatcher::SearchForTriangulation
 * (src/LSDmatcher.cpp:403) and the first MapLine::UpdateAverageDir (src/MapLine.cpp:325-372) of every new line.  SearchForTriangulation computes its MAD over all knn rows
 * and applies the filter afterwards, so the filter moves into this call with no change of result: sslam_line_match_batch_dev(gate_scale = 0.1) plus this call is the
 * whole of src/LSDmatcher.cpp:382-415 and the loop behind it.  The exact use: ONE sslam_line_match_batch_dev for all neighbours of a round set, then one of these calls per
 * round with the same d_lfree on one stream (one pair per session per round).  The gate of :955-979 stays with the caller: such a pair is not listed.
 * Keyframe slot k owns rows [k*lcap, k*lcap + d_nl[k]) of d_kl (mvKeyLines), d_linefn (mvKeyLineFunctions, 3 doubles per row) and, where given, d_lfree
 * (= !GetMapLine(i)); a NULL d_lfree means every line is free.  Pair p reads rows r < d_line_npairs[p] of d_line_pairs: (idx1, idx2) = d_line_pairs[(p*lcap + r)*2 + {0, 1}],
 * as sslam_line_match_batch_dev leaves them for a batch with cap = lcap; outputs are indexed p*lcap + r and rows at or past the count are not touched.
 * The reference's quirks stay: the endpoints of key line 2 are normalised with keyframe 1's cx, invfx, cy, invfy (:1032-1035), s3D / e3D come from line 1's endpoints and
 * both line functions, and all five ratios divide by the neighbour's median depth.
 *   d_stage   0 created        1 an index outside [0, nl)        2 not free: GetMapLine(qdx) || GetMapLine(tdx), with the flags as they stand before the pair creates anything
 *             3 parallax (:1053)        4 s3D(3) == 0 (:1066)        5 e3D(3) == 0 (:1084)
 *             6 .. 10 ratio1, ratio2, ratio3, ratio4, ratio5 (:1102-1131)        11 .. 14 SZC1, SZC2, EZC1, EZC2 (:1135-1148)
 *   d_s3d, d_e3d   the endpoints (:1070, :1088); d_normal (double) and d_dist = mNormalVector and (mfMaxDistance, mfMinDistance) of UpdateAverageDir with mpRefKF =
 *             keyframe 1 (level = keyline1.octave, clamped).  All of them are zero for a row that is not created.
 * d_nnew[p] = the number of created rows; a created row stores 0 to d_lfree[kf1*lcap + idx1] and d_lfree[kf2*lcap + idx2] (AddMapLine, :1159-1160).  In one launch two
 * pairs that share a slot may or may not see each other's creations in d_lfree; one pair per session per round never shares one.  Skipped pairs, streams, alignment (the
 * double buffers 8 bytes) and SSLAM_ERR_INVALID are as above. */
int sslam_new_map_lines_batch_dev(sslam_ctx* ctx, const sslam_keyline* d_kl, const double* d_linefn, const int32_t* d_nl, int lcap, int nkeyframes,
                                  const sslam_kf_pose* d_pose, const sslam_newmap_pair* d_pairs, int npairs, const int32_t* d_line_pairs, const int32_t* d_line_npairs,
                                  const float* scale_factors, int nlevels, uint8_t* d_lfree,
                                  float* d_s3d, float* d_e3d, uint8_t* d_stage, double* d_normal, float* d_dist, int32_t* d_nnew, void* stream);
/* The same for one host pair, synchronously (every line is free).  Outputs [line_npairs] rows. */
int sslam_new_map_lines(sslam_ctx* ctx, const sslam_keyline* kl1, const double* linefn1, int nl1, const sslam_keyline* kl2, const double* linefn2, int nl2,
                        const sslam_kf_pose* pose1, const sslam_kf_pose* pose2, float median_depth2, const int32_t* line_pairs, int line_npairs,
                        const float* scale_factors, int nlevels, float* s3d, float* e3d, uint8_t* stage, double* normal, float* dist, int* nnew);

/* ---- DBoW2 vocabulary descent: Frame::ComputeBoW, src/Frame.cc:474-481 ->
 * ORBVocabulary::transform(vCurrentDesc, mBowVec, mFeatVec, 4), whose per-feature work is
 * TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup), Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1216-1259.
 * The vocabulary is handed over as arrays in DBoW2's node numbering (node 0 = root): children of node i are
 * children[child_ptr[i] .. child_ptr[i+1]) in m_nodes[i].children order (a node without children is a leaf), node_desc =
 * 32-byte descriptor per node, word_id / weight per node (meaningful for leaves), levels = m_L (sslam_vocab_load_text below builds
 * exactly these arrays from an ORBvoc.txt-format file).  Outputs per feature: the word, its weight (0 = stopped
 * word) and the node passed at level m_L - levelsup; BowVector / FeatureVector are std::maps the caller fills from them
 * in feature order (v.addWeight(id, w); fv.addFeature(nid, i); then the L1 normalisation, TemplatedVocabulary.h:1147-1199). */
typedef struct sslam_vocab sslam_vocab;
int sslam_vocab_create(sslam_ctx* ctx, int nnodes, int levels, const int32_t* child_ptr, const int32_t* children, const uint8_t* node_desc,
                       const int32_t* word_id, const double* weight, sslam_vocab** out);
void sslam_vocab_destroy(sslam_vocab* vocab);
int sslam_bow_transform(sslam_ctx* ctx, const sslam_vocab* vocab, const uint8_t* desc, int n, int levelsup,
                        int32_t* word_out, double* weight_out, int32_t* node_out);
int sslam_bow_transform_frame(sslam_ctx* ctx, const sslam_vocab* vocab, const sslam_frame* frame, int levelsup,
                              int32_t* word_out, double* weight_out, int32_t* node_out);
/* The same descent (TemplatedVocabulary.h:1216-1259) for `nframes` frames whose descriptors are already on the device, asynchronously: what
 * Frame::ComputeBoW (src/Tracking.cc:1012, :1967) needs of every frame before SearchByBoW, for callers that extract many sessions' frames in
 * one launch.  The layout is the batch extractors': frame f owns rows [f*cap, f*cap + d_n[f]) of d_desc (32 bytes per row), so the descriptor
 * buffer of sslam_orb_extract_batch_dev is the input without a copy.  A count below 0 is read as 0, one above cap as cap.  Per valid row
 * d_word / d_weight / d_node receive what sslam_bow_transform writes for that descriptor (the first child with the smallest distance wins; the
 * node is 0 when the word lies above level m_L - levelsup); rows at or past a frame's count are not touched.  d_word and d_weight may each be
 * NULL, d_node may not: sslam_orb_search_by_bow_batch_dev below takes d_node as it is.  BowVector, its normalisation and score() are not part
 * of this call (sslam_compute_bow).
 * Every pointer but vocab is a device pointer; d_desc is 16-byte aligned.  One launch on `stream` (NULL: the context's stream), no scratch, no
 * synchronise, no host memory read or written.  SSLAM_ERR_INVALID (nothing enqueued): a NULL vocab, d_desc, d_n or d_node, a vocabulary of
 * another context, a negative cap, nframes or levelsup, nframes * cap >= 2^31, a misaligned buffer.  nframes == 0 is SSLAM_OK and enqueues
 * nothing. */
int sslam_bow_transform_batch_dev(sslam_ctx* ctx, const sslam_vocab* vocab, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes,
                                  int levelsup, int32_t* d_word, double* d_weight, int32_t* d_node, void* stream);

/* ORBVocabulary::loadFromTextFile (src/System.cc:64-73 -> TemplatedVocabulary.h:1338-1423): first line "k L scoring weighting"
 * (rejected outside 0<=k<=20, 1<=L<=10, 0<=scoring<=5, 0<=weighting<=3, as the reference does), then one line per node in id order
 * starting at 1: "parent isLeaf d0 .. d31 weight"; children keep file order, word ids count the leaves in file order.  Blank lines
 * are skipped (the reference's getline loop appends a node from uninitialised values after the final newline: undefined behaviour,
 * not reproduced).  sslam_vocab_set_types overrides what sslam_vocab_create assumes (TF_IDF = 0, L1_NORM = 0, the enums of
 * Thirdparty/DBoW2/DBoW2/BowVector.h:36-53). */
int sslam_vocab_load_text(sslam_ctx* ctx, const char* path, sslam_vocab** out);
int sslam_vocab_set_types(sslam_vocab* vocab, int weighting, int scoring);
int sslam_vocab_info(const sslam_vocab* vocab, int* k, int* levels, int* scoring, int* weighting, int* nnodes, int* nwords);

/* Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:474-481, src/KeyFrame.cc:74-84) complete:
 * TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup), TemplatedVocabulary.h:1126-1208, with
 * BowVector::addWeight / addIfNotExist / normalize (BowVector.cpp:34-85) and FeatureVector::addFeature (FeatureVector.cpp:30-44).
 * The descent runs on the device, the two std::maps are assembled on the host in feature order and returned flattened in key
 * order: BowVector = (bow_word[i], bow_value[i]) for i < *nbow; FeatureVector = node fv_node[j] owns the feature indices
 * fv_feat[fv_ptr[j] .. fv_ptr[j+1]) for j < *nfv.  Capacities: n entries each, n + 1 for fv_ptr. */
int sslam_compute_bow(sslam_ctx* ctx, const sslam_vocab* vocab, const uint8_t* desc, int n, int levelsup,
                      int32_t* bow_word, double* bow_value, int* nbow, int32_t* fv_node, int32_t* fv_ptr, int32_t* fv_feat, int* nfv);
int sslam_compute_bow_frame(sslam_ctx* ctx, const sslam_vocab* vocab, const sslam_frame* frame, int levelsup,
                            int32_t* bow_word, double* bow_value, int* nbow, int32_t* fv_node, int32_t* fv_ptr, int32_t* fv_feat, int* nfv);

/* MapPoint::ComputeDistinctiveDescriptors, src/MapPoint.cc:247-312, and MapLine::ComputeDistinctiveDescriptors,
 * src/MapLine.cpp:246-317, for nsets observation sets at once: set s owns rows ptr[s]..ptr[s+1]
 * of desc (ptr[0] = 0).  best_out[s] = index inside the set of the descriptor with the least median Hamming distance to
 * the rest (median = sorted[int(0.5*(N-1))], first row wins ties), -1 for an empty set.  Sets are limited to 1024 rows. */
int sslam_distinctive_descriptors(sslam_ctx* ctx, const uint8_t* desc, const int32_t* ptr, int nsets, int32_t* best_out);

/* The same choice (src/MapPoint.cc:247-312, src/MapLine.cpp:246-317) for `nsets` observation sets whose descriptors are rows of device-resident
 * keyframes, asynchronously: the pMP->ComputeDistinctiveDescriptors() behind every triangulated, fused or initialised map point and line
 * (src/LocalMapping.cc CreateNewMapPoints / CreateNewMapLines2 and SearchInNeighbors, Tracking::CreateInitialMapMonoWithPL) for callers that keep many
 * sessions' keyframes on the device.  The two reference functions differ only in the descriptor matrix they read (mDescriptors, mLineDescriptors);
 * ORB and LBD rows are both 32 bytes, so there is no kind argument.  The pool is sslam_orb_search_for_triangulation_batch_dev's and
 * sslam_fuse_search_batch_dev's: keyframe slot k owns rows [k*cap, k*cap + d_n[k]) of d_desc.  A count below 0 is read as 0, one above cap as cap;
 * nothing at or past a count is read.
 * Set s owns the entries d_obs[d_ptr[s] .. d_ptr[s+1]) (d_ptr: nsets + 1 ints), one (keyframe slot, feature row) per observation in the caller's
 * mObservations iteration order -- the reference walks a std::map<KeyFrame*, size_t>, i.e. in address order; what that order is, is the caller's to
 * say, and ties go to the first.  An entry is ADMISSIBLE when 0 <= kf < nkeyframes, d_kf_bad is NULL or d_kf_bad[kf] == 0 (pKF->isBad(), :270) and
 * 0 <= row < the slot's clamped count; any other entry is skipped exactly as the reference skips a bad keyframe.  N is the number of admissible
 * entries, the median of an entry is sorted[int(0.5 * (N - 1))] of its N distances to the admissible entries (itself included, :283), and the same
 * (kf, row) twice in a set is legal and counts twice.
 * d_best[s] = the position inside the set's entry list (0 .. d_ptr[s+1] - d_ptr[s] - 1, skipped entries counted) of the admissible entry with the
 * least median; the first such entry wins (`median < BestMedian`, :301).  -1 when no entry is admissible (the reference's early returns, :261 and
 * :274).  -2 when the set is refused: its range fails 0 <= d_ptr[s] <= d_ptr[s+1] <= nobs, or it has more than 1024 entries (the single call's limit;
 * the batch has no status per set beyond this).  d_median[s] (d_median may be NULL) = that least median, INT_MAX with -1 or -2.  Every set writes
 * its d_best and d_median, so the call enqueues no clear of them.
 * d_out_desc (may be NULL) is a table of nout rows of 32 bytes: a set with d_best >= 0 copies the chosen descriptor to row d_out_row[s], or to row s
 * where d_out_row is NULL; a target outside [0, nout) is not written, and a set with -1 or -2 leaves its row as it was (the reference leaves
 * mDescriptor unchanged).  When two sets name one row, one of them wins and which one is unspecified.  The table is what
 * sslam_fuse_search_batch_dev and sslam_search_by_projection_batch_dev take as d_qdesc, without a copy.
 * WHY ONE CALL IS EXACT: a set's result depends on no other set.  The function reads the observed rows and the bad flags and writes mDescriptor
 * alone (:310); no other map point's choice reads that, and the caller omits the sets of map points with mbBad (:256).
 * Every pointer is a device pointer; d_desc and d_out_desc are 16-byte aligned, the typed buffers 4-byte aligned.  The call enqueues two launches on
 * `stream` (NULL: the context's stream) -- sets of up to 64 entries, and the rare ones of 65 .. 1024 -- uses no scratch, reads and writes no host
 * memory, does not synchronise and is independent of every other call on the context.  SSLAM_ERR_INVALID (nothing enqueued): a NULL ctx, d_desc,
 * d_n, d_ptr or d_best; a NULL d_obs with nobs > 0; d_out_row without d_out_desc; a misaligned buffer; a negative cap, nkeyframes, nobs, nsets or
 * nout; cap >= 2^19; nkeyframes * cap >= 2^31.  nsets == 0 is SSLAM_OK and enqueues nothing. */
typedef struct sslam_observation {
    int32_t kf;       /* keyframe slot (mObservations' key) */
    int32_t row;      /* feature row in that keyframe (mObservations' value) */
} sslam_observation;  /* 8 bytes, no padding */
int sslam_distinctive_descriptors_batch_dev(sslam_ctx* ctx,
                                            const uint8_t* d_desc, const int32_t* d_n, int cap, int nkeyframes, const uint8_t* d_kf_bad,
                                            const sslam_observation* d_obs, int nobs, const int32_t* d_ptr, int nsets,
                                            int32_t* d_best, int32_t* d_median,
                                            uint8_t* d_out_desc, const int32_t* d_out_row, int nout, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches), src/ORBmatcher.cc:159-291.
 * The DBoW2 vocabulary transform stays on the host (the vocabulary file is not part of the reference tree); the
 * matcher takes the two FeatureVectors as CSR lists over the nodes BOTH frames contain, ascending node id:
 * node k owns keyframe features kf_idx[node_kf_ptr[k]..node_kf_ptr[k+1]) and frame features f_idx[node_f_ptr[k]..).
 * kf_valid[i] = vpMapPointsKF[i] && !isBad().  assigned_out[j] = keyframe feature matched to frame feature j, or -1. */
int sslam_orb_search_by_bow(sslam_ctx* ctx, const sslam_keypoint* kf_kp, const uint8_t* kf_desc, const uint8_t* kf_valid, int nkf,
                            const sslam_keypoint* f_kp, const uint8_t* f_desc, int nf,
                            const int32_t* node_kf_ptr, const int32_t* node_f_ptr, int nnodes,
                            const int32_t* kf_idx, const int32_t* f_idx, float nnratio, int check_orientation,
                            int32_t* assigned_out, int* nmatches_out);
/* The same matcher (src/ORBmatcher.cc:159-291, the KeyFrame -> Frame overload; sslam_orb_search_by_bow_keyframes_batch_dev is the KeyFrame -> KeyFrame one) for `npairs` pairs of device-resident frames,
 * asynchronously, from per-feature node ids instead of CSR lists: the batch form of Tracking::TrackReferenceKeyFrame (src/Tracking.cc:1009-1020,
 * one reference keyframe per session) and of Tracking::Relocalization (src/Tracking.cc:1964-1996, one frame against K candidate keyframes).
 * Keyframe slot k owns rows [k*kfcap, k*kfcap + d_nkf[k]) of d_kf_kp, d_kf_desc (32 bytes per row), d_kf_node and d_kf_valid
 * (= vpMapPointsKF[i] && !isBad()); frame slot f owns rows [f*cap, f*cap + d_nf[f]) of d_f_kp, d_f_desc and d_f_node.  A count below 0 is read
 * as 0, one above its capacity as the capacity.  The node arrays are what sslam_bow_transform_batch_dev writes to d_node.
 * Pair p matches keyframe slot d_pair_kf[p] against frame slot d_pair_f[p]; either array may be NULL, which means slot p and requires that side's
 * slot count to equal npairs.  A slot may appear in any number of pairs (Relocalization: every pair names the one frame slot).  A pair with a
 * slot index outside its range is skipped: d_nmatches[p] = 0 and nothing else of the pair is written.
 * Pair p yields what sslam_orb_search_by_bow returns for the two FeatureVectors that FeatureVector::addFeature(node[i], i) builds in feature
 * order: the nodes are the ids >= 0 present on both sides; inside a node both sides are taken in ascending index; a row with a node id below 0
 * is in no node.  d_assigned[p*cap + j], j < nf, = the keyframe feature matched to frame feature j, or -1 (also after the rotation check);
 * rows at or past the frame's count are not touched.  d_nmatches[p] = the count after the rotation pruning.
 * Every pointer is a device pointer; the descriptor buffers are 16-byte aligned.  One launch on `stream` (NULL: the context's stream), no
 * scratch, no synchronise, no host memory read or written.  SSLAM_ERR_INVALID (nothing enqueued): a NULL (other than the pair arrays) or
 * misaligned buffer, a negative size, kfcap or cap >= 2^19, a NULL pair array whose side has another slot count than npairs.  npairs == 0 is
 * SSLAM_OK and enqueues nothing. */
int sslam_orb_search_by_bow_batch_dev(sslam_ctx* ctx,
                                      const sslam_keypoint* d_kf_kp, const uint8_t* d_kf_desc, const int32_t* d_kf_node, const uint8_t* d_kf_valid,
                                      const int32_t* d_nkf, int kfcap, int nkeyframes,
                                      const sslam_keypoint* d_f_kp, const uint8_t* d_f_desc, const int32_t* d_f_node, const int32_t* d_nf, int cap, int nframes,
                                      const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs,
                                      float nnratio, int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), src/ORBmatcher.cc:525-658 (loop closing,
 * src/LoopClosing.cc:271): same node walk; kfX_valid[i] = vpMapPointsX[i] && !isBad(); a candidate of the second keyframe is skipped
 * when it is already matched or has no good map point (:576-580); the gate is `bestDist1 < TH_LOW` (strict, :600).
 * matches12_out[i] = feature of the second keyframe whose map point goes into vpMatches12[i], or -1. */
int sslam_orb_search_by_bow_keyframes(sslam_ctx* ctx, const sslam_keypoint* kf1_kp, const uint8_t* kf1_desc, const uint8_t* kf1_valid, int n1,
                                      const sslam_keypoint* kf2_kp, const uint8_t* kf2_desc, const uint8_t* kf2_valid, int n2,
                                      const int32_t* node_kf1_ptr, const int32_t* node_kf2_ptr, int nnodes,
                                      const int32_t* kf1_idx, const int32_t* kf2_idx, float nnratio, int check_orientation,
                                      int32_t* matches12_out, int* nmatches_out);
/* The same matcher (src/ORBmatcher.cc:525-658) for `npairs` pairs of device-resident keyframes, asynchronously, from per-feature node ids instead of
 * CSR lists: the first matcher of LoopClosing::ComputeSim3 (src/LoopClosing.cc:256-285: the current keyframe against every consistent candidate,
 * ORBmatcher(0.75, true), `nmatches < 20` discards the candidate), for callers that keep many sessions' keyframes on the device.  With it every
 * public matcher of ORBmatcher and LSDmatcher has a batch form: the two matchers behind this one in ComputeSim3 are sslam_fuse_search_batch_dev
 * (SearchBySim3, :328) and mode 1 of sslam_search_by_projection_batch_dev (:380).
 * The pool is sslam_orb_search_for_triangulation_batch_dev's: keyframe slot k owns rows [k*cap, k*cap + d_n[k]) of d_kp (mvKeysUn), d_desc (32 bytes
 * per row), d_node (what sslam_bow_transform_batch_dev writes to d_node; an id below 0 is in no node) and d_valid (= GetMapPoint(i) && !isBad();
 * NULL: every row is valid).  A count below 0 is read as 0, one above cap as cap; nothing at or past a count is read.
 * d_pairs holds npairs x 2 int32: pair p is (kf1, kf2) = (d_pairs[2p], d_pairs[2p+1]), kf1 is pKF1 (the side the result is indexed by), kf2 is pKF2
 * (the candidates).  kf1 == kf2 is legal and computed like any other pair; a slot may appear in any number of pairs.  A pair with a slot outside
 * [0, nkeyframes) is skipped: d_nmatches[p] = 0 and nothing else of the pair is written.
 * Pair p yields exactly what sslam_orb_search_by_bow_keyframes returns for the two FeatureVectors FeatureVector::addFeature(node[i], i) builds in
 * feature order from the two node arrays.  d_matches12[p*cap + i1], i1 < n[kf1], = the keyframe-2 row whose map point goes into vpMatches12[i1], or
 * -1, after the rotation pruning; d_nmatches[p] = the count after the pruning.  d_matches21[p*cap + i2], i2 < n[kf2], = the keyframe-1 row that
 * holds keyframe-2 row i2, or -1: the inverse of the pair's d_matches12 rows after the pruning (the reference's vbMatched2 with its owner).  It is a
 * required output, and where keyframe 2 does not fit the LDS it is also where the call keeps its live state, which is why there is no scratch.  Rows
 * at or past a count are not touched in either array.
 * Unlike the KeyFrame -> Frame batch above: the result is indexed by keyframe 1; keyframe 2 has validity flags, and an invalid or already taken
 * keyframe-2 row is skipped before its distance is looked at (:577-583), so it is neither best nor second best; the distance gate is strict,
 * bestDist1 < TH_LOW (:601); the ratio test is (float)bestDist1 < nnratio * (float)bestDist2 with bestDist2 = 256 when there is no second (:603);
 * the rotation bin is that of kp1.angle - kp2.angle (:610), one histogram entry per matched keyframe-1 row.
 * WHY ONE CALL IS EXACT for any pair list: the reference function writes nothing but its own output vector and its local vbMatched2, so the K
 * candidates of one current keyframe are K independent pairs.  (sslam_orb_search_for_triangulation_batch_dev is different: its free flags change
 * between the neighbours of one keyframe, so it needs one call per round.)
 * Every pointer is a device pointer; d_desc is 16-byte aligned, the typed buffers 4-byte aligned.  One launch on `stream` (NULL: the context's
 * stream), no scratch, no synchronise, no host memory read or written; independent of every other call on the context.  SSLAM_ERR_INVALID (nothing
 * enqueued): a NULL ctx, d_kp, d_desc, d_node, d_n, d_pairs, d_matches12, d_matches21 or d_nmatches, a misaligned buffer, a negative cap, nkeyframes
 * or npairs, cap >= 2^19, npairs * cap >= 2^31.  npairs == 0 is SSLAM_OK and enqueues nothing. */
int sslam_orb_search_by_bow_keyframes_batch_dev(sslam_ctx* ctx,
                                                const sslam_keypoint* d_kp, const uint8_t* d_desc, const int32_t* d_node, const uint8_t* d_valid,
                                                const int32_t* d_n, int cap, int nkeyframes,
                                                const int32_t* d_pairs, int npairs,
                                                float nnratio, int check_orientation,
                                                int32_t* d_matches12, int32_t* d_matches21, int32_t* d_nmatches, void* stream);

/* LSDmatcher::SerachForInitialize(InitialFrame,CurrentFrame,LineMatches),
 * src/LSDmatcher.cpp:257-284 = knn2 + Frame::lineDescriptorMAD (src/Frame.cc:190-215)
 * + the `d2-d1 > 0.5*MAD12` gate.  pairs_out[cap*2] (qdx,tdx); gate_scale = 0.5
 * (0.1 reproduces SearchForTriangulation, src/LSDmatcher.cpp:396).
 * ratio_mode != 0 uses the `d1/d2 < 1/1.5` gate of SearchByProjection(KF,F)/
 * SearchByDescriptor (src/LSDmatcher.cpp:158-169,303-314) instead. */
int sslam_line_match(sslam_ctx* ctx, const uint8_t* ldesc1, int n1, const uint8_t* ldesc2, int n2,
                     double gate_scale, int ratio_mode, int32_t* pairs_out, int cap, int* npairs_out,
                     double* nn_mad_out, double* nn12_mad_out);
/* The same for npairs_frames frame pairs on the device: pair p owns rows [p*cap, (p+1)*cap) of d_ldesc1 / d_ldesc2 and of d_pairs
 * ((qdx,tdx) per row), its counts are d_n1[p] / d_n2[p], d_npairs[p] receives its number of pairs; rows of d_pairs past that number
 * are not written.  A pair with no query rows, fewer than two train rows, or MORE THAN 1024 QUERY ROWS yields 0 pairs (the single
 * call returns SSLAM_ERR_UNSUPPORTED for n1 > 1024; the batch form has no per-pair status). */
int sslam_line_match_batch_dev(sslam_ctx* ctx, const uint8_t* d_ldesc1, const int32_t* d_n1,
                               const uint8_t* d_ldesc2, const int32_t* d_n2, int cap, int npairs_frames,
                               double gate_scale, int ratio_mode, int32_t* d_pairs, int32_t* d_npairs,
                               void* stream);

/* ---- Lines (replaces LineSegment::ExtractLineSegment) --------------------- */
/* LineSegment::ExtractLineSegment(img,keylines,ldesc,keylineFunctions,scale,numOctaves),
 * src/ExtractLineSegment.cpp:18-69 = LSDDetector::detect + top-N by response +
 * BinaryDescriptor::compute + normalised line equations.  max_lines = 40 reproduces
 * the reference's hard cap (:42); BASELINE configs use 200 / 400. */
int sslam_lines_create(sslam_ctx* ctx, int max_lines, sslam_lines** out);
int sslam_lines_destroy(sslam_lines* ln);
int sslam_lines_extract(sslam_lines* ln, const uint8_t* gray, int w, int h, size_t stride,
                        sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out /*3 per line*/,
                        int cap, int* n_out);
/* The line twin of sslam_orb_set_blur_variant: which 8-bit cv::GaussianBlur LBD's 5x5 sigma-1 pre-blur is (BinaryDescriptor::compute, called at
 * src/ExtractLineSegment.cpp:53): 0 = OpenCV >= 3.4.1 (taps 14 62 104 62 14), 1 = OpenCV 3.4.0 (14 63 103 63 14).  LSD's own 7x7 sigma-0.75 pre-blur has the
 * same taps (0 4 56 136 56 4 0) under both, so the segments do not depend on it; the LBD bytes do. */
int sslam_lines_set_blur_variant(sslam_lines* ln, int variant);
/* The other stated decisions of the line path that have a selectable alternative.  The arithmetic of LSD and LBD is OpenCV's (called at
 * src/ExtractLineSegment.cpp:38-40,53); this image holds no OpenCV, so each of these is a choice between two restatements, with the size of what it moves
 * measured in oracle/ref_pin/pin_report_stub.json.  variant is 0 or 1; the next extraction takes it.
 *   sslam_lines_set_nfa_variant    D11 -- the first term of LineSegmentDetectorImpl::nfa()'s log1term.  1 (DEFAULT since round 5) = `(double(n) + 1)` without the log_gamma,
 *                                  as imgproc/src/lsd.cpp is recalled to read (two independent recollections); 0 = log_gamma(n + 1), the binomial coefficient of von Gioi's
 *                                  lsd.c (the default of rounds 1-4).  Under 1 nearly every rectangle passes at its first rect_nfa: 2.0-2.7 x the segments of 0.
 *   sslam_lines_set_lbd_bit_order  D12 -- BinaryDescriptor::binaryConversion.  1 (DEFAULT since round 5) = comparison i sets `0x80 >> i` (as recalled); 0 = comparison i
 *                                  sets bit i (rounds 1-4).  Every byte is bit-reversed; Hamming distances, hence every matcher result, are the same.
 *   sslam_lines_set_resize_variant D7 -- LSD's 0.8x rescale: 0 (default) = INTER_LINEAR_EXACT (8.8 coefficients, one rounding); 1 = INTER_LINEAR (11-bit coefficients,
 *                                  the two-stage 8u rounding of the ORB pyramid's resize).
 *   sslam_lines_set_seed_order     D2 -- the order of LSD's seeds inside one of the 1024 gradient bins: 0 (default) = raster order (a stable counting sort, on the device);
 *                                  1 = whatever `std::sort` of this library's libstdc++ leaves, as upstream's ll_angle sorts: the bins are sorted ON THE HOST (one
 *                                  download, one std::sort of every pixel and one upload per frame: ~15 ms per 640x480 frame -- a switch for comparing with a
 *                                  maintainer's CPU build, not a production path). */
int sslam_lines_set_nfa_variant(sslam_lines* ln, int variant);
int sslam_lines_set_lbd_bit_order(sslam_lines* ln, int variant);
int sslam_lines_set_resize_variant(sslam_lines* ln, int variant);
int sslam_lines_set_seed_order(sslam_lines* ln, int variant);
/* Frame sizes of the line extractor: every line entry point (sslam_lines_extract, sslam_lines_extract_batch_dev, the host batches with lines != NULL) returns
 * SSLAM_ERR_UNSUPPORTED, before any kernel launch (sslam_lines_extract has enqueued the image's upload by then) and with the size in the message, for a frame with a side below 10 pixels (LSD's 0.8x image below 8 x 8) or whose scaled
 * side exceeds 65 535.  The stencil kernels reflect a coordinate once (BORDER_REFLECT_101 with radius 3), which is exact from 4 pixels a side on; the bound of 10 lies above
 * that and is the smallest size the suite runs against the oracle (10 x 10, 10 x 40, 40 x 10).  A refused size leaves the handle as it was: its plan, its workspace and the
 * last batch's status and segments stay those of the previous size.  An image with w == 0 or h == 0 yields zero lines and SSLAM_OK.
 * A frame whose LSD stage finds more than 8192 candidate rectangles keeps the first 8192 in seed order: sslam_lines_extract returns SSLAM_ERR_UNSUPPORTED for it, a batch
 * delivers the lines of those rectangles and reports the frame through sslam_lines_batch_status. */
/* Batch-of-frames mode over the image layout of sslam_orb_extract_batch_dev (d_images + i*image_stride is frame i, row pitch `pitch`; with padded
 * rows the last frame must be readable for pitch * h bytes): d_kl[nframes*cap], d_ldesc[nframes*cap*32], d_linefn[nframes*cap*3], d_counts[nframes].
 * The layout only chooses how the rows are loaded (aligned dwords for a dword-aligned base, pitch and image_stride; bytes otherwise), never a result.
 * A pitch below w, or frames that overlap (image_stride < pitch * (h - 1) + w, when nframes > 1), give SSLAM_ERR_INVALID; nothing is enqueued. */
int sslam_lines_extract_batch_dev(sslam_lines* ln, const uint8_t* d_images, int w, int h,
                                  size_t pitch, size_t image_stride, int nframes,
                                  sslam_keyline* d_kl, uint8_t* d_ldesc, double* d_linefn,
                                  int32_t* d_counts, int cap, void* stream);
/* Batch status of the line extractor (see sslam_orb_batch_status): frames of the last batch holding more lines than `cap`
 * (SSLAM_ERR_CAPACITY) and frames whose LSD stage overflowed its 8192 candidate rectangles (SSLAM_ERR_UNSUPPORTED, as the single-frame call
 * reports it).  d_status4 = {frames over capacity, first of them, frames over the LSD limit, first of them}. */
int sslam_lines_batch_status(sslam_lines* ln, int cap, void* stream, int* truncated_frames_out, int* unsupported_frames_out, int* first_frame_out);
int sslam_lines_batch_status_dev(sslam_lines* ln, int cap, int32_t* d_status4, void* stream);
/* Scheduling hint for a caller that keeps a second stream busy while a batch of line extractions is in flight (bench.py's two-stream mode;
 * the reference has no batch mode and no counterpart).  `hip_event` (a hipEvent_t; NULL clears it) is recorded on the stream of every
 * following sslam_lines_extract_batch_dev call immediately BEFORE the sequential core (k_lsd_regions) is launched.  The core is latency-bound
 * and leaves issue slots free, the kernels in front of it are bandwidth-bound and do not: a second stream that waits for the event overlaps
 * the core instead of the prologue.  The event stays the caller's. */
int sslam_lines_set_core_event(sslam_lines* ln, void* hip_event);
/* With a core event set, a batch of at least 32 frames per compute unit (two rounds of 16 workgroups per CU; 18 per CU from 36 frames per compute unit on) runs the sequential core in its GUEST form: a persistent grid of four-wave workgroups that
 * claim frames dynamically and leave a third of every SIMD's registers to the caller's second stream.  Returns 1 when a call of `nframes` frames
 * would take that form, 0 otherwise.  A caller in the guest form gets the most from building the ORB pyramid BEFORE the event (sslam_orb_set_gate_event: FAST and
 * what follows wait for it) -- in the other form from making its whole second branch wait for the event (bench.py / pipeline.py / sslam_frontend_batch do exactly that). */
int sslam_lines_core_guest_form(sslam_lines* ln, int nframes);
/* The counterpart on the point side: `hip_event` (a hipEvent_t; NULL clears it) is WAITED for on the stream of every following
 * sslam_orb_extract_batch_dev call after the pyramid kernels (level copy, resizes: bandwidth-bound like the line branch's prologue) and before
 * the FAST / quadtree / descriptor kernels (vector-bound: the ones that should run under the sequential core).  With the core event here the
 * point stream needs no wait of its own: the pyramid is built beside the line prologue, the rest starts with the core. */
int sslam_orb_set_gate_event(sslam_orb* orb, void* hip_event);
/* Two extractors that take turns (a batch processed as two half batches, each on its own streams): the sequential core wants every wave slot
 * of the chip, so two cores must not overlap -- but one half's kernels BEHIND its core (NFA stages, LBD: VALU-bound) overlap well with the
 * other half's kernels IN FRONT of its core (blur, gradient, counting sort: bandwidth-bound).  Every following sslam_lines_extract_batch_dev
 * of `ln` makes its stream wait for `wait_event` right before the core (NULL: no wait; an event that was never recorded does not block) and
 * records `done_event` right behind it (NULL: nothing).  The events stay the caller's. */
int sslam_lines_set_core_gate(sslam_lines* ln, void* wait_event, void* done_event);
/* Host-buffer batch (SURVEY.md §8(b) `sslam_frontend_batch`): n frames of one size in host memory through Frame::ExtractORB and, when
 * `lines` is not NULL, Frame::ExtractLSD (src/Frame.cc:150-161); frame i starts at images + i*image_stride (row pitch `stride`).
 * Per-frame results in the caller's arrays: kp_out[n*cap], desc_out[n*cap*32], nkp_out[n], kl_out[n*lcap], ldesc_out[n*lcap*32],
 * linefn_out[n*lcap*3], nl_out[n]; rows past a frame's count are unspecified.  A frame with more keypoints than `cap` / more lines than
 * `lcap` makes the call return SSLAM_ERR_CAPACITY, an LSD overflow SSLAM_ERR_UNSUPPORTED (as the single-frame entry points do; the arrays
 * then hold the truncated rows).  Frames are processed in chunks of `chunk` (0 = as many as fill every wave slot of the sequential LSD core,
 * 6144, bounded by a third of the free device memory): the upload of chunk k+1 and the download of chunk k-1 overlap the kernels of chunk
 * k (two copy streams; pinned caller memory -- hipHostMalloc / hipHostRegister -- is copied directly, pageable memory through pinned staging
 * buffers filled by a few host threads, SSLAM_BATCH_THREADS); the point branch and the line branch of a chunk run on two HIP streams, the point
 * branch released when the sequential core starts (sslam_lines_set_core_event).  Staging buffers, streams and events are kept per context
 * between calls (sslam_frontend_batch_release frees them early).  This is the PCIe-inclusive form of the batch mode; callers that already
 * hold their frames in HBM use the *_batch_dev entry points directly. */
int sslam_frontend_batch(sslam_orb* orb, sslam_lines* lines, const uint8_t* images, int n, int w, int h, size_t stride, size_t image_stride, int chunk,
                         sslam_keypoint* kp_out, uint8_t* desc_out, int32_t* nkp_out, int cap,
                         sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* nl_out, int lcap);
int sslam_frontend_batch_release(sslam_ctx* ctx);
/* sslam_frontend_batch plus the match stage of BASELINE configs[2] ("extract + Hamming match vs previous frame"): the batch is a SEQUENCE,
 * frame i is matched against frame i-1 of the same call with the three matchers the resident-frame pipeline times
 *   ORBmatcher::SearchForInitialization(F1 = frame i-1, F2 = frame i, vbPrevMatched = F1's keypoint positions, window_size)
 *                                                       src/ORBmatcher.cc:408-523 as called at src/Tracking.cc:330-345,
 *   the dense Hamming 2-NN of F1's descriptors in F2's (cv::BFMatcher::knnMatch, the reduction under every Search*; optional),
 *   LSDmatcher::SerachForInitialize(F1, F2) on the LBD descriptors (src/LSDmatcher.cpp:257-284; only with `lines`),
 * on the device, behind the chunk's extraction (point matchers on the point stream, the line matcher on the line stream).  Rows of frame i
 * describe the pair (i-1, i) and are indexed by F1's features: init_matches12[i*cap + j] = keypoint of frame i matched to keypoint j of
 * frame i-1 or -1 (j < nkp_out[i-1]), init_nmatches[i]; knn_idx / knn_dist[(i*cap + j)*2 + {0,1}]; line_pairs[(i*lcap + p)*2 + {0,1}] =
 * (line of frame i-1, line of frame i) for p < line_npairs[i].  Frame 0 has no predecessor: its counts are 0 and its rows unspecified.
 * Chunking, staging, streams and error behaviour are those of sslam_frontend_batch (chunk boundaries do not show: the last frame of a
 * chunk stays on the device as the next chunk's predecessor); the match arrays follow the same pinned-or-staged rule as the others. */
typedef struct sslam_batch_match {
    int32_t window_size; float nnratio; int32_t check_orientation; float bounds[4];      /* SearchForInitialization: windowSize (100), mfNNratio (0.9), mbCheckOrientation, mnMinX/MaxX/MinY/MaxY */
    double line_gate_scale; int32_t line_ratio_mode;                                    /* sslam_line_match arguments (0.5, 0) */
    int32_t* init_matches12;      /* [n*cap] */
    int32_t* init_nmatches;       /* [n] */
    int32_t* knn_idx;             /* [n*cap*2] or NULL (then knn_dist is NULL as well) */
    int32_t* knn_dist;            /* [n*cap*2] */
    int32_t* line_pairs;          /* [n*lcap*2]; ignored without `lines` */
    int32_t* line_npairs;         /* [n] */
} sslam_batch_match;
int sslam_frontend_batch_match(sslam_orb* orb, sslam_lines* lines, const uint8_t* images, int n, int w, int h, size_t stride, size_t image_stride, int chunk,
                               sslam_keypoint* kp_out, uint8_t* desc_out, int32_t* nkp_out, int cap,
                               sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* nl_out, int lcap, const sslam_batch_match* match);


/* ---- camera model: Frame::UndistortKeyPoints / Frame::ComputeImageBounds (src/Frame.cc:483-543) ----------------------------------------
 * The pinhole + Brown-Conrady model Tracking::Tracking reads from the settings file (src/Tracking.cc:48-72): K = fx, fy, cx, cy and
 * DistCoef = k1, k2, p1, p2 (+ k3 only when it is non-zero; k3 = 0 and a missing k3 give the same result).  The undistortion is
 * cv::undistortPoints(pts, pts, K, DistCoef, noArray(), K) restated in fp64 (DESIGN.md decision D13: five fixed iterations).  As in the
 * reference, ONLY k1 decides whether anything happens: k1 == 0 leaves every point where it is (mvKeysUn = mvKeys) and the bounds are
 * (0, w, 0, h), whatever k2, p1, p2, k3 hold.  Line features are never undistorted (the reference has no mvKeylinesUn step). */
typedef struct sslam_camera { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } sslam_camera;      /* src/Tracking.cc:48-72; k3 = 0 when absent */
/* Frame::ComputeImageBounds (src/Frame.cc:515-543): bounds_out = {mnMinX, mnMaxX, mnMinY, mnMaxY} of a w x h image, from the undistorted
 * corners (0,0), (w,0), (0,h), (w,h).  Host-only: needs no device and no context. */
int sslam_camera_image_bounds(const sslam_camera* cam, int w, int h, float bounds_out[4]);
/* Frame::UndistortKeyPoints (src/Frame.cc:483-513): kp_un[i] = kp[i] with pt.x, pt.y undistorted; size, angle, response, octave and class_id
 * are copied unchanged (:507-510).  Host pointers, synchronous; kp_un == kp is allowed. */
int sslam_undistort_keypoints(sslam_ctx* ctx, const sslam_camera* cam, const sslam_keypoint* kp, int n, sslam_keypoint* kp_un);
/* Batch/device form over the layout of sslam_orb_extract_batch_dev: frame f = rows [f*cap, f*cap + d_counts[f]) of d_kp -> the same rows of
 * d_kp_un; rows at or past a frame's count are not touched.  d_kp_un == d_kp (in place) is allowed.  With k1 == 0 it is a device copy of
 * the valid rows.  Enqueued on `stream`. */
int sslam_undistort_keypoints_batch_dev(sslam_ctx* ctx, const sslam_camera* cam, const sslam_keypoint* d_kp, const int32_t* d_counts,
                                        int nframes, int cap, sslam_keypoint* d_kp_un, void* stream);
/* The camera of the Frame an extractor feeds (NULL clears it, the default).  With a camera set, sslam_frame_from_orb snapshots the UNDISTORTED
 * keypoints of the last sslam_orb_extract -- the mvKeysUn the Frame constructor hands the matchers (src/Frame.cc:95) -- while
 * sslam_orb_extract itself keeps returning mvKeys. */
int sslam_orb_set_camera(sslam_orb* orb, const sslam_camera* cam);
/* sslam_frontend_batch_match (match may be NULL: sslam_frontend_batch) for a camera with lens distortion: kp_out stays mvKeys, byte-equal to
 * what sslam_frontend_batch_match returns, and kpun_out[n*cap] receives mvKeysUn (rows past a frame's count unspecified).  With `match`,
 * vbPrevMatched and SearchForInitialization take mvKeysUn of both frames, as src/Tracking.cc:340-342 and src/ORBmatcher.cc:408-523 do;
 * match->bounds are used as passed -- pass sslam_camera_image_bounds(cam, w, h).  The 2-NN and the line matcher are unchanged.  The
 * undistorted rows travel beside the raw ones, the predecessor carried across chunk boundaries included. */
int sslam_frontend_batch_match_camera(sslam_orb* orb, sslam_lines* lines, const sslam_camera* cam, const uint8_t* images, int n, int w, int h,
                                      size_t stride, size_t image_stride, int chunk, sslam_keypoint* kp_out, sslam_keypoint* kpun_out,
                                      uint8_t* desc_out, int32_t* nkp_out, int cap, sslam_keyline* kl_out, uint8_t* ldesc_out,
                                      double* linefn_out, int32_t* nl_out, int lcap, const sslam_batch_match* match);

/* ---- colour frames: the cvtColor of Tracking::GrabImageMonocularWithPL (src/Tracking.cc:146-161) ----------------------------------------
 *     if (mImGray.channels() == 3) cvtColor(mImGray, mImGray, mbRGB ? CV_RGB2GRAY : CV_BGR2GRAY);
 *     else if (mImGray.channels() == 4) cvtColor(mImGray, mImGray, mbRGB ? CV_RGBA2GRAY : CV_BGRA2GRAY);
 * on the device.  The format names the byte order of each pixel AS STORED (alpha is ignored): a caller that passes the bytes of its cv::Mat
 * with mbRGB's choice (RGB / RGBA when Camera.RGB is 1) gets the reference's gray bytes, whatever order the bytes really are in.  Arithmetic:
 * OpenCV 3.4's 8-bit RGB2Gray<uchar> table form, gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 (DESIGN.md decision D14).
 * Memory contract of every entry point below: the reads of a frame stay inside [frame, frame + pitch*(h-1) + w*cn) (cn = 1, 3 or 4 bytes per
 * pixel), the writes touch only bytes [0, w) of each gray row; the padding of the output rows is left alone.  An unknown format, a pitch
 * below w*cn (gray: below w) or frames that overlap (image_stride < pitch*(h-1) + w*cn, when nframes > 1) give SSLAM_ERR_INVALID. */
enum { SSLAM_PIX_GRAY = 0, SSLAM_PIX_RGB = 1, SSLAM_PIX_BGR = 2, SSLAM_PIX_RGBA = 3, SSLAM_PIX_BGRA = 4 };
/* One frame, host in, host out, through the device (synchronous): img = h rows of `stride` bytes, gray = h rows of `gray_stride` bytes.
 * SSLAM_PIX_GRAY copies the w bytes of each row. */
int sslam_gray_from_color(sslam_ctx* ctx, int format, const uint8_t* img, int w, int h, size_t stride, uint8_t* gray, size_t gray_stride);
/* Device buffers: frame f of d_src at d_src + f*image_stride (row pitch `pitch`) -> d_gray + f*gray_image_stride (row pitch `gray_pitch`),
 * one launch for the batch, enqueued on `stream` (NULL: the context stream).  SSLAM_PIX_GRAY is a pitched device copy. */
int sslam_gray_from_color_batch_dev(sslam_ctx* ctx, int format, const uint8_t* d_src, int w, int h, size_t pitch, size_t image_stride, int nframes,
                                    uint8_t* d_gray, size_t gray_pitch, size_t gray_image_stride, void* stream);
/* sslam_frontend_batch_match_camera for colour frames in host memory: frame i of `format` at images + i*image_stride (row pitch `stride`, at
 * least w*cn).  Each chunk is uploaded as it is stored (cn bytes per pixel) and converted on the device right behind its upload; both
 * extractors then read the gray plane exactly as sslam_frontend_batch hands them its frames, so every output equals what the gray entry points
 * return for the converted frames.  `cam` may be NULL (kpun_out is then not read or written: sslam_frontend_batch_match), and `match` may be
 * NULL (no match stage: sslam_frontend_batch).  SSLAM_PIX_GRAY is byte-identical to sslam_frontend_batch / _match / _match_camera.  n == 1 is
 * the single-frame colour call: one upload feeds both extractors.  The staging of pageable frames copies cn bytes per pixel; the host does
 * not convert. */
int sslam_frontend_batch_color(sslam_orb* orb, sslam_lines* lines, const sslam_camera* cam, int format, const uint8_t* images, int n, int w, int h,
                               size_t stride, size_t image_stride, int chunk, sslam_keypoint* kp_out, sslam_keypoint* kpun_out, uint8_t* desc_out,
                               int32_t* nkp_out, int cap, sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* nl_out, int lcap,
                               const sslam_batch_match* match);

/* ---- multi-GPU batch mode (SURVEY.md §8(b) "sslam_group_create + sslam_frontend_batch_sharded", §8(e)) ----------------------
 * north_star: "a batch-of-frames mode shards independent images across the 8 GPUs of one node with RCCL over xGMI only for the final
 * keypoint/line gather".  Frames are independent units: global frame i lives on GPU i % G.  Each GPU runs the single-GPU path on its
 * shard; the ONE exchange step is a gather of compacted per-frame records to the root GPU (grouped ncclSend / ncclRecv, sizes first).
 * There is no reference counterpart (the reference front-end is one thread on one CPU, src/Frame.cc:86-87); the caller-side loop this
 * replaces is the per-frame Frame::ExtractORB / ExtractLSD pair (src/Frame.cc:150-161).  RCCL is bound at run time (dlopen of
 * librccl.so.1, or the copy a host process such as PyTorch already loaded), so the library itself has no link-time RCCL dependency.
 *
 * Record stream (what travels over xGMI and what rank 0 ingests): per frame, 16-byte aligned,
 *   sslam_record_header {n_kp, n_ln, frame, bytes}  then  n_kp x sslam_keypoint (28 B), n_kp x 32 B descriptors,
 *   n_ln x sslam_keyline (68 B), n_ln x 32 B LBD descriptors, n_ln x 3 doubles (mvKeyLineFunctions, src/ExtractLineSegment.cpp:56-68)
 * -- compacted to the counts, not padded to the capacities: about 80 KB per 640x480 frame at 1000 keypoints / 165 lines. */
typedef struct sslam_group sslam_group;
#define SSLAM_GROUP_ID_BYTES 128
typedef struct sslam_record_header { int32_t n_kp, n_ln, frame, bytes; } sslam_record_header;
typedef struct sslam_frontend_params {     /* ORBextractor ctor arguments (Examples/ICL.yaml:41-54) + the line cap; max_lines 0 = no line extraction */
    int32_t nfeatures; float scale_factor; int32_t nlevels, ini_th_fast, min_th_fast, max_lines;
} sslam_frontend_params;

/* One process drives `ngpu` devices (0 .. ngpu-1): one context, extractor pair and host thread per device, communicators from
 * ncclCommInitAll.  This is the form a C++ host like the reference's (one process) uses. */
int sslam_group_create(int ngpu, sslam_group** out);
/* One process per GPU (torch.distributed / MPI style): rank 0 obtains an id, the launcher broadcasts it, every rank joins.  `device` is the
 * HIP device of this process. */
int sslam_group_unique_id(uint8_t id_out[SSLAM_GROUP_ID_BYTES]);
int sslam_group_create_rank(int device, int rank, int nranks, const uint8_t id[SSLAM_GROUP_ID_BYTES], sslam_group** out);
int sslam_group_destroy(sslam_group* group);
int sslam_group_size(const sslam_group* group);
int sslam_group_rank(const sslam_group* group);      /* 0 in the single-process form */

/* Compacts the per-frame results of a *_batch_dev call into the record stream above: frame i of the batch becomes the record with
 * header.frame = frame0 + i*frame_step.  d_kl / d_ldesc / d_linefn / d_nl may be NULL (no lines).  d_out[out_capacity]; *d_total_bytes
 * (device) receives the stream length, or UINT64_MAX when it does not fit.  Enqueued on `stream`, no synchronisation.  Calls on different streams
 * of one context are ordered on the context's buffer of per-frame offsets by an event (the later call's kernels wait for the earlier call's); a call
 * that needs a larger buffer than the context holds waits on the host for the previous call before it replaces it. */
int sslam_pack_records_dev(sslam_ctx* ctx, int nframes, int frame0, int frame_step,
                           const sslam_keypoint* d_kp, const uint8_t* d_desc, const int32_t* d_nkp, int cap,
                           const sslam_keyline* d_kl, const uint8_t* d_ldesc, const double* d_linefn, const int32_t* d_nl, int lcap,
                           uint8_t* d_out, uint64_t out_capacity, uint64_t* d_total_bytes, void* stream);
/* Upper bound of the stream length for nframes frames at the given capacities (buffer sizing). */
uint64_t sslam_record_stream_capacity(int nframes, int cap, int lcap);
/* Host side of the ingest: scatters a record stream (host memory) into per-frame arrays indexed by header.frame, laid out like the
 * outputs of sslam_frontend_batch (kp_out[nframes*cap] ...; line outputs may be NULL).  Returns SSLAM_ERR_INVALID on a malformed
 * stream, SSLAM_ERR_CAPACITY when a record exceeds cap / lcap.  *nrecords_out = records seen. */
int sslam_unpack_records(const uint8_t* stream, uint64_t bytes, int nframes,
                         sslam_keypoint* kp_out, uint8_t* desc_out, int32_t* nkp_out, int cap,
                         sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* nl_out, int lcap, int* nrecords_out);

/* The exchange step, one-process-per-GPU form: every rank hands over its device-resident record stream (length in *d_send_bytes, a
 * device word as written by sslam_pack_records_dev); rank 0 receives the streams of all ranks back to back in d_recv (rank order) and
 * gets the per-rank lengths in bytes_per_rank_out[nranks] (host).  Sizes travel first (one 8-byte ncclAllGather), then one grouped
 * ncclSend / ncclRecv per peer.  Synchronous on `stream` (NULL = an internal stream); call it from a side thread to overlap it with the
 * next batch's kernels.  d_recv / recv_capacity / bytes_per_rank_out are ignored on ranks other than 0. */
int sslam_group_gather_dev(sslam_group* group, const uint8_t* d_send, const uint64_t* d_send_bytes,
                           uint8_t* d_recv, uint64_t recv_capacity, uint64_t* bytes_per_rank_out, void* stream);

/* sslam_frontend_batch over all GPUs of a single-process group: n frames in host memory, frame i -> GPU i % G, per-GPU extraction in
 * chunks, RCCL gather of the records to GPU 0, results in the caller's arrays exactly as sslam_frontend_batch returns them (same
 * error behaviour).  The per-device extractors are created from `params` on first use and kept in the group. */
int sslam_frontend_batch_sharded(sslam_group* group, const sslam_frontend_params* params,
                                 const uint8_t* images, int n, int w, int h, size_t stride, size_t image_stride,
                                 sslam_keypoint* kp_out, uint8_t* desc_out, int32_t* nkp_out, int cap,
                                 sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* nl_out, int lcap);
/* How sslam_frontend_batch_sharded deals a batch over the GPUs (host-only bookkeeping, callable without a device): global frame i lives on
 * GPU i mod ngpu, every GPU walks its frames in chunks of *chunk_slots_out slots.  sslam_shard_frame = the global frame in slot `slot` of
 * chunk `chunk` on GPU `gpu` (-1: the slot is empty -- uneven tails); sslam_shard_chunk_count = how many leading slots of that chunk hold
 * a frame.  On any error of sslam_frontend_batch_sharded the outputs hold what arrived: nkp_out[i] (and nl_out[i]) = -1 marks a frame whose
 * records never reached the root (a HIP / RCCL failure on its GPU); truncated rows (SSLAM_ERR_CAPACITY) and LSD overflow
 * (SSLAM_ERR_UNSUPPORTED) are deferred statuses as in sslam_frontend_batch -- every frame is still delivered, clamped. */
int sslam_shard_layout(int n, int ngpu, int* chunk_slots_out, int* nchunks_out);
int sslam_shard_frame(int n, int ngpu, int chunk, int gpu, int slot);
int sslam_shard_chunk_count(int n, int ngpu, int chunk, int gpu);

/* ---- Stage taps (diagnostics).  They read back intermediate results of the LAST extraction of a handle so that a maintainer who pins this
 * library against the reference built with OpenCV 3.4 can compare stage by stage (pyramid level bytes, FAST candidates, blurred patches: sslam_orb_debug_*, declared with
 * the extractor above; LSD segments before the top-N cut: below).  Synchronous; nothing on the product path calls them. */
/* Stage tap: all LSD segments (x1,y1,x2,y2 float) of frame `frame` of the last batch, before top-N.  On a handle with sslam_lines_set_topn_only on, and a call of the
 * one-launch NFA form (2 048 frames or more), the tap returns the accepted segments among the candidates that were VALIDATED, in emission order: every segment that can
 * be among the max_lines output lines is in it, shorter ones may be missing. */
int sslam_lines_debug_segments(sslam_lines* ln, int frame, float* seg_out, int cap, int* n_out);
/* The caller's contract "only the max_lines best lines leave this handle": on != 0 states that nothing reads the segments before the top-N cut (the tap above), so the
 * NFA stage may stop validating candidate rectangles once none of the remaining ones can reach the output (a rectangle's response is known before validation up to a
 * small margin: csrc/nfa_topn.h).  Key lines, descriptors, line equations and counts are bit for bit those of the default.  Not a tuning knob: the default is 0 because the
 * tap exists.  Returns the previous value (0 for a NULL handle). */
int sslam_lines_set_topn_only(sslam_lines* ln, int on);
/* Stage clocks of the sequential LSD core for frame `frame` of the last call (grow, rect, refine, radius reduction, total, ...): zeros unless
 * the library was built with -DSSLAM_LSD_CYCLES (tools/lsd_cycles.py). */
int sslam_lines_debug_cycles(sslam_lines* ln, int frame, long long* out8);
#ifdef __cplusplus
}
#endif
#endif /* SSLAM_FRONTEND_H */
