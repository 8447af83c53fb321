/* Test-only entry points -- NOT part of the drop-in boundary (include/sslam_frontend.h is) and NOT in libsslam_frontend.so: they exist in
 * libsslam_frontend_testing.so, the same sources compiled with -DSSLAM_TESTING (structure-slam-pointline_amd/build.py builds both; the testing library exports everything the
 * product library does plus what is declared here).  tests/ and tools/ call them; a product caller has no reason to. */
#ifndef SSLAM_TESTING_H
#define SSLAM_TESTING_H
#include "sslam_frontend.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Multi-GPU group code (sslam_group_create / _create_rank, reference: the batch-of-frames mode of BASELINE configs[4]) on a box with ONE GPU:
 * while `on` is nonzero, NEW groups bind an in-process stand-in for the RCCL entry points (host-mediated device-to-device copies with NCCL's matching rules;
 * same process only) and may hold more members than GPUs are visible -- so that the group code's multi-member paths (a host thread per member, uneven tails,
 * the collective error agreement, grouped send / receive to the root) execute with real device buffers.  It says nothing about xGMI.  Process-wide; returns the
 * previous setting.  (Round 4 selected the stand-in with the environment variable SSLAM_GROUP_FAKE_RCCL; an explicit call cannot be set by accident.) */
int sslam_testing_use_rccl_standin(int on);

/* Self-test of the table-based exact integer division of the NFA binomial tail against the hardware IEEE division:
 * `pairs` random quotients a/b with 1 <= a,b < n; *mismatches_out must come back 0. */
int sslam_selftest_exact_div(sslam_ctx* ctx, int n, long long pairs, long long* mismatches_out);
/* The log-gamma / log(p) / reciprocal tables of the NFA stage as the library evaluates them on the host with the reference's own libm
 * expressions (opencv lsd.cpp log_gamma_windschitl / log_gamma_lanczos, reached from src/ExtractLineSegment.cpp:38-40): out[2n + 48].
 * Host-only; lets a test pin the table bits (a libm that rounds differently would otherwise go unnoticed until a rectangle flips). */
int sslam_debug_nfa_tables(int n, double* out);
/* Self-test of the guarded fp32 early-exit test used in the NFA tail loop (the reference's `err < tolerance * ...` test,
 * opencv lsd.cpp nfa(), reached from src/ExtractLineSegment.cpp:38-43): random inputs, half on the decision boundary.
 * disagree_out must be 0; ambiguous_out = cases that fall back to the fp64 expression. */
int sslam_selftest_tail_test(sslam_ctx* ctx, long long samples, long long* disagree_out, long long* ambiguous_out);
/* The region-growing core replaces the IEEE division inside cv::fastAtan2 by the hardware's refinement sequence without its
 * scaling / special-case steps (identity on the value range of a region's direction sums) and the quadrant compares by sign-bit
 * arithmetic: `samples` random and adversarial sums, bit-compared with the `/` operator and the straight form.
 * mismatches_out[0] = divisions that differ, mismatches_out[1] = angles that differ. */
int sslam_selftest_region_div(sslam_ctx* ctx, long long samples, long long mismatches_out[2]);

/* k_describe steers the rBRIEF pattern with (float)cos / (float)sin of the keypoint angle evaluated in double (src/ORBextractor.cc:108-147 computeOrbDescriptor) through a
 * reduction of its own for [0, 6.5] instead of the library's sincos: every float of the range, both results after the rounding to float; *mismatches_out must be 0. */
int sslam_selftest_sincos(sslam_ctx* ctx, long long* mismatches_out);
/* k_lsd_hist_sort bins a pixel's |g|^2 (LSD's 1 024 gradient bins, opencv lsd.cpp ll_angle, reached from src/ExtractLineSegment.cpp:38-40) in fp32 where fp32 decides and with
 * the reference's fp64 expression otherwise: every s in [0, max_s] (max_s = the frame's largest |g|^2, < 2^24) against the fp64 expression; *mismatches_out must be 0. */
int sslam_selftest_lsd_bin(sslam_ctx* ctx, int max_s, long long* mismatches_out);
/* k_lbd's walk rounds a coordinate with ONE conversion (v_cvt_rpi_i32_f32 = floor(x + 0.5)) where BinaryDescriptor::computeLBD has (short)round(x) under a clamp to the image
 * (OpenCV line_descriptor binary_descriptor.cpp, reached from src/ExtractLineSegment.cpp:53): every float bit pattern of the coordinate range, against the previous
 * instruction sequence under the clamps (mismatches_out[0]) and against roundf for x >= 0 (mismatches_out[1]).  Both must be 0. */
int sslam_selftest_lbd_round(sslam_ctx* ctx, long long mismatches_out[2]);

/* Profiling aid (no reference counterpart): the chip's issue rate for one kind of vector instruction (0: v_add_u32, 1: v_fma_f32,
 * 2: v_add_f64, 3: v_bcnt_u32_b32), 16 independent instructions per lane and round with 8 waves per SIMD resident: wave-instructions per
 * second in units of 1e9.  What the SQ utilisation figures of profiles/README.md are priced against. */
int sslam_selftest_valu_rate(sslam_ctx* ctx, int kind, double* ginst_per_s_out);
/* Profiling aid (no reference counterpart): reads a known number of bytes in one of the library's two dominant access
 * patterns (mode 0: 16 B/lane coalesced stream, mode 1: scattered 16-B gathers) so that rocprofv3's FETCH_SIZE can be
 * calibrated on this device (tools/fetch_probe.py, profiles/README.md). */
int sslam_selftest_fetch_probe(sslam_ctx* ctx, size_t bytes, int mode, long long* bytes_requested_out);
/* counters of the cluster form of the sequential core (one frame at a time, helper waves on several compute units) for frame `frame` of
 * the last call; meaningful in builds with -DSSLAM_CL_CYCLES only (tools/cl_probe.py). */
int sslam_lines_debug_cluster(sslam_lines* ln, int frame, long long* out8);

/* The line tail -- k_keylines (checkLineExtremes, KeyLine fill, top-N by response, line equations), k_blur_sobel and k_lbd: LSDDetector::detectImpl's KeyLine fill,
 * the cap and BinaryDescriptor::compute of src/ExtractLineSegment.cpp:42-68 -- on segments the CALLER supplies in place of the LSD detector's, so that a test can drive those
 * kernels at their own edges.  `nframes` gray images of one size on the host (row pitch `stride`, `image_stride` bytes from frame to frame); segs[nframes][nmax][4] = x1, y1,
 * x2, y2 in source pixels in emission order; accept[nframes][nmax] (NULL: all accepted) = what the NFA stage's flag would be; nsegs[nframes] <= min(nmax, 8192) candidates per
 * frame (more: SSLAM_ERR_INVALID).  The call builds plan, workspace and constants as sslam_lines_extract_batch_dev does (one shared function), zeroes the frames' scalars,
 * writes segments, flags and candidate counts where the NFA stage leaves them and runs the launches the product path runs behind that stage (one shared function).
 * Outputs on the host, `cap` (<= 8192) rows per frame: kl_out[nframes][cap], ldesc_out[nframes][cap][32], linefn_out[nframes][cap][3], counts_out[nframes] and, unless
 * NULL, lbd_dir_out[nframes][cap][2] = the (cos, sin) pairs k_keylines leaves for k_lbd.  Every device output buffer is filled with the byte 0xA5 before the launches and
 * copied back whole: rows at or past a frame's count still hold it.  The handle must have been created by THIS library (the kernels' __constant__ tables are per library and
 * uploaded once per handle); sslam_lines_debug_segments afterwards returns the accepted segments in order. */
int sslam_testing_lines_tail(sslam_lines* ln, const uint8_t* gray, int w, int h, size_t stride, size_t image_stride, int nframes, const float* segs, const uint8_t* accept,
                             const int32_t* nsegs, int nmax, int cap, sslam_keyline* kl_out, uint8_t* ldesc_out, double* linefn_out, int32_t* counts_out, float* lbd_dir_out);

/* What the last sslam_lines_extract_batch_dev of the handle (sslam_lines_extract and the host batches call it) chose among its launch forms, so that a test can assert the form
 * it means to cover instead of inferring it from the sizes: out[0] = the sequential core (0 cluster form with the NFA stage streaming beside it, 1 cluster form with the stage
 * behind it, 2 one lone wave per frame, 3 the guest form on a persistent grid, 4 one four-wave workgroup per frame, 5 one six-wave workgroup per frame), out[1] = the guest
 * form's grid (0 otherwise), out[2] = the gradient came from the fused blur + gradient kernel, out[3] = the seeds were sorted by the tile-sorted runs kernels, out[4] = the NFA
 * stage (0 streaming beside the core, 1 the 18 launches, 2 k_nfa_all), out[5] / out[6] = its evaluating / counting waves per frame (streaming: the consumer waves and 0),
 * out[7] = k_lbd's template argument.  Every call starts with -1 in all eight, so a word the call did not reach (before the first call; a call that failed early; out[3]
 * under sslam_lines_set_seed_order(1), where the host sorts) is -1 and never another call's choice; the four line taps of this header start the same way.  The handle keeps what lines_forms
 * (csrc/lines_form.h) decided for the call and how far the call got; this function alone turns that into the eight words. */
int sslam_testing_lines_last_forms(sslam_lines* ln, int32_t out[8]);

/* The line prologue -- k_blur7 + k_lsd_grad or k_lsd_grad_fused, the gradient table behind them, and the counting sort of the seeds as k_lsd_hist + k_lsd_scan +
 * k_lsd_scatter or k_lsd_hist_sort + k_lsd_scan + k_lsd_scatter_runs: LineSegmentDetectorImpl::flsd up to and including ll_angle (OpenCV imgproc lsd.cpp, reached from
 * src/ExtractLineSegment.cpp:38-40) -- ALONE, with everything it leaves for region growing copied back, so that a test can compare those kernels with the oracle pixel for
 * pixel and seed for seed instead of through the segments that come out three stages later.  `nframes` gray images of one size on the host (row pitch `stride`,
 * `image_stride` bytes from frame to frame).  They are uploaded into the handle's image buffer in the layout the caller chooses: rows `dev_pitch` bytes apart (0: the
 * 64-byte-aligned pitch sslam_lines_extract and the tail tap use; otherwise >= w), frames dev_pitch * h apart, the first pixel `dev_offset` (0 .. 3) bytes behind the
 * buffer's 256-byte-aligned start -- the fused kernel takes dword-aligned layouts of its geometry only, so an offset of 1 sends such a frame through k_blur7 + k_lsd_grad.
 * The choice itself is lines_prologue()'s, unchanged (the tile-sorted runs are lines_forms', csrc/lines_form.h).  The call sets the words of sslam_testing_lines_last_forms to -1, runs lines_prepare, k_zero_misc and lines_prologue()
 * -- the functions of sslam_lines_extract_batch_dev, nothing else -- which records words 2 (fused gradient) and 3 (tile-sorted runs; stays -1 under
 * sslam_lines_set_seed_order(1)) as on the product path.  sslam_lines_set_resize_variant / _seed_order / _blur_variant apply as they do there.
 * Outputs on the host, plane_cap pixels per frame (SSLAM_ERR_CAPACITY if the scaled image sw x sh = size_out[0] x size_out[1] holds more; size_out is valid then): with
 * npx = sw * sh, t_out[nframes][npx] = the T plane (level-line angle in degrees, -1024 where undefined), s_out[nframes][npx] = S (|g|^2), cs_out[nframes][npx][2] = Cs
 * (cos, sin), order_out[nframes][npx] = the seed list (x | y << 16), misc_out[nframes][2] = Misc::maxS, Misc::nDefined.  The T, S, Cs and seed list regions of every frame
 * are filled with the byte 0xA5 after lines_prepare and before the first launch and copied back whole: a T pixel no kernel wrote, and every seed slot at or past nDefined,
 * still hold it.  UNSPECIFIED, because the kernels write them for defined pixels only: S and Cs where T is -1024 (S is written everywhere under seed order 1, where the host
 * sorts all pixels: there it is |g|^2 for x < sw - 1, y < sh - 1).  The handle must have been created by THIS library (lines_prepare uploads the library's __constant__
 * tables once per handle); a sslam_lines_extract on it afterwards is an ordinary call. */
int sslam_testing_lines_prologue(sslam_lines* ln, const uint8_t* gray, int w, int h, size_t stride, size_t image_stride, int nframes, size_t dev_pitch, int dev_offset,
                                 size_t plane_cap, int32_t size_out[2], float* t_out, int32_t* s_out, float* cs_out, uint32_t* order_out, int32_t* misc_out);
/* The handle's gradient table as k_grad_table left it: tab_out[1021 * 1021][4], entry (gy + 510) * 1021 + (gx + 510) = {angle in degrees or -1024, cos, sin, the bits of
 * gx^2 + gy^2} for every 2 x 2 gradient of an 8-bit image, and *smin_out = k_grad_smin's smallest |g|^2 of a defined pixel.  Built first (as the first plan of the handle
 * would) if the handle has none. */
int sslam_testing_lines_grad_table(sslam_lines* ln, float* tab_out, int32_t* smin_out);

/* The NFA stage -- rect_nfa / rect_improve of LSD_REFINE_ADV (OpenCV imgproc lsd.cpp, reached from src/ExtractLineSegment.cpp:38-40) as the 18 launches, k_nfa_all or
 * k_nfa_topn (csrc/lsd_nfa.h, csrc/nfa_topn.h) -- on candidate rectangles the CALLER supplies in place of the sequential core's, so that a test can drive the stage, and
 * above all the top-N form's ranking, slices and stopping rule, at their own edges and compare every flag.  `nframes` gray images of one size on the host, passed as
 * sslam_testing_lines_tail takes them; rects[nframes][nmax][12] = the RectD records (x1, y1, x2, y2, width, x, y, theta, dx, dy, prec, p in scaled pixels) in emission order;
 * ncand[nframes] <= min(nmax, 8192); topn_max_lines = what sslam_lines_set_topn_only hands the stage (0: the full validation).  Before any launch, SSLAM_ERR_INVALID for a record
 * the core could not have emitted -- the kernels are only ever given their normal value range --: every value finite; the centre inside the scaled image
 * [0, sw - 1] x [0, sh - 1] and both end points within `width` of it (region2rect projects the region's pixels onto the axis: the core's own end points lie up to a few pixels
 * outside on ordinary frames, and the counters clip every row and column to the image); 0 < width <= max(sw, sh); |dx^2 + dy^2 - 1| <= 1e-9; prec and p equal to the plan's.  The call runs lines_prepare, k_zero_misc and
 * lines_prologue() as sslam_lines_extract_batch_dev does (the T plane is the product's own), fills every frame's flag, segment and NfaState regions with the byte 0xA5, writes
 * the records and Misc::nCand where the core leaves them and calls lines_nfa_stage (sslam::launch_nfa_stage) with topn_max_lines, nothing else: the form is chosen as on the
 * product path by lines_forms (csrc/lines_form.h) from SSLAM_NFA_FUSED and the number of frames, and recorded for sslam_testing_lines_last_forms (words 2 .. 6; the core's words stay -1).  The streaming form takes its records
 * from a cluster slot and is not reached from here.  Outputs on the host: flags_out[nframes][nmax] and segs_out[nframes][nmax][4] at EMISSION indices (flag 0 rejected,
 * 1 accepted with its segment written, 2 left out by the top-N form), topn_out[nframes] = Misc::topn.  Rows at or past ncand still hold the fill, and so does the segment
 * of every row that is not flagged 1 -- with ONE exception, documented rather than refused (a call may mix ranked frames with frames of more than 1024 rectangles): in a
 * frame that k_nfa_topn ranks (topn_max_lines < ncand <= 960) the rows from 1024 (NFA_RANK_BASE) on are the kernel's ranked copy and unspecified; only [0, 1024) is
 * meaningful there.  The handle must have been created by THIS library. */
int sslam_testing_lines_nfa(sslam_lines* ln, const uint8_t* gray, int w, int h, size_t stride, size_t image_stride, int nframes, const double* rects, const int32_t* ncand,
                            int nmax, int topn_max_lines, int32_t* flags_out, float* segs_out, int32_t* topn_out);

/* The sequential LSD core -- region growing, region2rect, refine() and reduce_region_radius() of LineSegmentDetectorImpl::flsd's seed loop (OpenCV imgproc lsd.cpp, reached from
 * src/ExtractLineSegment.cpp:38-40) as k_lsd_regions (csrc/lsd_regions.h: lone wave, guest, four- and six-wave workgroups) or k_lsd_regions_cl (csrc/lsd_cluster.h) -- ALONE, with
 * everything it leaves copied back, so that a test can compare EVERY candidate rectangle (also those the NFA stage rejects) in all twelve doubles, and the used map, with the
 * oracle instead of through the float32 segments that survive two stages later.  Two steps.
 * sslam_testing_lines_core, the run step: `nframes` gray images of one size ON THE DEVICE, the layout arguments of sslam_lines_extract_batch_dev (a batch form needs thousands
 * of frames).  It sets the words of sslam_testing_lines_last_forms to -1 and runs lines_prepare, k_zero_misc, lines_prologue() and lines_core() -- the functions of
 * sslam_lines_extract_batch_dev, the core's launch included: the form is lines_forms' (csrc/lines_form.h) from the knobs as they stand, `nframes` and the core event, and is
 * recorded as on the product path (words 0 .. 3) -- and nothing behind the core: words 4 .. 7 stay -1.  ONE exception: CoreForm::ClusterStream is coupled to its consumers, so
 * for it the step runs what the product runs, k_nfa_stream beside the core and behind it (one shared function), and words 4 .. 6 read as on the product path.  After the prologue and
 * before the core's launch every frame's candidate region (and, under the streaming form, the staged rectangles of its cluster slot) is filled with the byte 0xA5.  The step runs
 * on the context's stream and returns with it idle.
 * sslam_testing_lines_core_frame, the copy-back step, for frame `frame` of the last run step (SSLAM_ERR_INVALID if the handle's last call was anything else): size_out[2] = the
 * scaled size sw x sh, *ncand_out = Misc::nCand, rects_out[nmax][12] = the first min(nmax, 8192) RectD records in emission order, copied WHOLE from where the form leaves them
 * -- the frame's candidate region; under the streaming form the staging array of the frame's cluster slot, which the main wave alone writes (k_nfa_stream copies a record into
 * the workspace before rect_improve changes it there, so the staged records are still the core's own after the stage) -- so rows at or past nCand still hold the fill; t_out
 * (may be NULL; plane_cap pixels, SSLAM_ERR_CAPACITY if sw * sh is more) = the T plane as [sh][sw] floats: the level-line angle with the USED bit in the sign (a pixel is used
 * iff it is defined, i.e. not -1024, and its sign bit is set).  A frame of more than 8 192 candidates returns SSLAM_ERR_UNSUPPORTED naming the limit, as sslam_lines_extract
 * does, with every output filled.  The handle must have been created by THIS library. */
int sslam_testing_lines_core(sslam_lines* ln, const uint8_t* d_images, int w, int h, size_t pitch, size_t image_stride, int nframes);
int sslam_testing_lines_core_frame(sslam_lines* ln, int frame, int nmax, size_t plane_cap, int32_t size_out[2], int32_t* ncand_out, double* rects_out, float* t_out);

/* The ORB tail -- k_octree (DistributeOctTree, src/ORBextractor.cc:539-763) and k_describe (IC_Angle, the 7x7 blur, computeOrbDescriptor and the KeyPoint fill, :77-147,
 * :835-847, :1085-1101) -- on FAST candidates the CALLER supplies in place of k_fast_cells', so that a test can drive the two kernels at their own edges.  `nframes` gray
 * images of one size on the host (row pitch `stride`, `image_stride` bytes from frame to frame), uploaded the way sslam_orb_extract uploads its frame;
 * cand[nframes][nlevels][nmax][3] = x, y, score per candidate, x and y relative to the level's minBorder (16) as k_fast_cells packs them, in arrival order;
 * ncand[nframes][nlevels] <= nmax.  Before any launch: 0 <= x < W, 0 <= y < H (the level's maxBorder - minBorder extents: its width and height less 32), 1 <= score <= 255,
 * ncand <= the level's candidate capacity (the sum of its cells' ((cw + 1) / 2) * ((ch + 1) / 2); 0 for a level without cells), no two candidates of a level at one pixel
 * -- SSLAM_ERR_INVALID otherwise.  The call prepares plan, constants and workspace and runs level-0 copy, resizes and k_fast_cells as sslam_orb_extract_batch_dev does (shared
 * functions), then overwrites what k_fast_cells left: each level's list is dealt into that level's cells in order, every cell up to its capacity, and the cells' counts set to
 * match, so that k_octree's gather returns the list in the caller's order; then it runs the product path's tail (one shared function).  Outputs on the host, `cap` rows per
 * frame: kp_out[nframes][cap], desc_out[nframes][cap][32], counts_out[nframes], level_counts_out[nframes][nlevels] = what k_octree kept per level, and, unless NULL,
 * *octree_lds_bytes_out = the dynamic LDS the k_octree launch asked for.  Every device output buffer is filled with the byte 0xA5 before the launches and copied back whole:
 * rows at or past a frame's count still hold it.  The handle must have been created by THIS library (the kernels' __constant__ tables are per library and uploaded once per
 * handle); sslam_orb_debug_candidates afterwards returns the injected lists. */
int sslam_testing_orb_tail(sslam_orb* o, const uint8_t* gray, int w, int h, size_t stride, size_t image_stride, int nframes, const int32_t* cand, const int32_t* ncand,
                           int nmax, int cap, sslam_keypoint* kp_out, uint8_t* desc_out, int32_t* counts_out, int32_t* level_counts_out, size_t* octree_lds_bytes_out);

/* sslam_search_by_projection_batch_dev of THIS library: at most max_slice frames per slice (0: the plan's own size), so that a test crosses a slice
 * boundary with a handful of frames; feats_in_lds != 0: the commit keeps each frame's features in LDS as the single call does (64 bytes per feature,
 * rows of at most 2048), the layout tools/proj_batch_probe.py times against the one the plan chooses.  Process-wide; results do not depend on either. */
int sslam_testing_proj_batch_tuning(int max_slice, int feats_in_lds);

/* sslam_two_view_ransac for one host pair with EVERY hypothesis copied back, so that a wrong hypothesis that does not win is visible: the same kernel with its stores enabled,
 * run as pair `pair` of a batch (the draw of src/Initializer.cc:93-108 hashes the pair index; the single call is pair 0).  Per iteration it: sets_out[it*8 .. +8) = the eight
 * indices into the match list, mats_out[it*45 .. +45) = Hn, H21i, H12i, Fn, F21i (row-major, 9 floats each: ComputeH21, :191, :192, ComputeF21, :242), scores_out[it*2 .. +2) =
 * CheckHomography's and CheckFundamental's score.  All zero for a pair below 8 matches.  result and inliers as sslam_two_view_ransac. */
int sslam_testing_two_view_hypotheses(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12, const int32_t* sets,
                                      int iterations, float sigma, uint32_t seed, int pair, sslam_two_view_result* result, uint8_t* inliers,
                                      int32_t* sets_out, float* mats_out, float* scores_out);

/* sslam_sim3_ransac for one host pair with EVERY iteration the reference's loop ran copied back, so that a wrong hypothesis that neither becomes the best nor returns is visible:
 * the same kernel with its stores enabled, run as pair `pair` of a batch (the draw of src/Sim3Solver.cc:166-177 hashes the pair index; the single call is pair 0).  By absolute
 * iteration it < max_iterations: sets_out[it*3 .. +3) = the three indices into the correspondence list, mats_out[it*13 .. +13) = ms12i, mR12i (row-major), mt12i,
 * counts_out[it] = mnInliersi (-1 for a set with an index out of range, whose matrices are zero).  Rows of iterations this call did not run -- before its_done, past the
 * return -- are zero.  state and inliers as sslam_sim3_ransac. */
int sslam_testing_sim3_hypotheses(sslam_ctx* ctx, const sslam_keypoint* kp1, const float* x3dc1, const uint8_t* valid1, int n1, const float K1[4],
                                  const sslam_keypoint* kp2, const float* x3dc2, const uint8_t* valid2, int n2, const float K2[4], const float* level_sigma2, int nlevels,
                                  const int32_t* matches12, int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations,
                                  const int32_t* sets, uint32_t seed, int pair, sslam_sim3_state* state, uint8_t* inliers,
                                  int32_t* sets_out, float* mats_out, int32_t* counts_out);

/* sslam_pnp_ransac for one host pair with EVERY iteration the reference's loop ran copied back: the same kernel with its stores enabled, run as pair `pair` of a batch.  By
 * absolute iteration it < tap_rows (later ones are not recorded): sets_out[it*4 .. +4) = the four indices into the correspondence list, poses_out[it*12 .. +12) = mRi
 * (row-major), mti in double, counts_out[it*4 .. +4) = mnInliersi (-1 for a set that never qualifies, whose pose is zero), the N that compute_pose chose (:518-520) in the low byte with the branches the solve reached above it (bit 8: the det < 0 flip, 9: the pcs[2] < 0 sign change, 10: b4[0] < 0, 11: a dropped singular value of CC),
 * whether Refine ran at this iteration in the reference's loop (:226) and mnRefinedInliers of that run, trace_out[it*15 .. +15) = rep_errors[1 .. 3] and Betas[1 .. 3]
 * after gauss_newton.  Rows of iterations this call did not run are zero.  state and inliers as sslam_pnp_ransac. */
int sslam_testing_pnp_hypotheses(sslam_ctx* ctx, const sslam_keypoint* f_kp, int nf, const float f_K[4], const float* kf_xw, const uint8_t* kf_valid, int nkf,
                                 const float* level_sigma2, int nlevels, const int32_t* assigned, double probability, int min_inliers, int max_iterations, float epsilon,
                                 float th2, int new_iterations, const int32_t* sets, int nsets, uint32_t seed, int pair, sslam_pnp_state* state, uint8_t* inliers,
                                 int tap_rows, int32_t* sets_out, double* poses_out, int32_t* counts_out, double* trace_out);

/* sslam_two_view_reconstruct for one host pair with EVERY hypothesis copied back, so that a wrong hypothesis that does not win is visible: the same kernel with its stores
 * enabled, run as pair 0.  hyp_out[h*15 .. +15) = R (row-major), t and, for ReconstructH, the plane normal n of hypothesis h (zeros for one that was not built);
 * sel_out[h] = the cosine CheckRT selected (vCosParallax[min(50, size - 1)] after the sort; 0 when nGood is 0).  Per hypothesis and match row r (the match list in
 * ascending keypoint-1 order; rows_cap = max(n1, n2, 1) rows per hypothesis): stage_out[h*rows_cap + r] = 0 not an inlier, 1 not finite, 2 z1 <= 0, 3 z2 <= 0,
 * 4 error 1, 5 error 2, 6 good; p3d_rows_out[(h*rows_cap + r)*3 .. +3) = the triangulated point (from stage 1 on), cos_out[h*rows_cap + r] = cosParallax (from stage 2
 * on).  line_err_out[r*2 .. +2) (NULL without lines) = errorC1, errorC2 of line row r.  Rows past the match list and hypotheses that were not run are zero. */
int sslam_testing_two_view_reconstruct(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
                                       const sslam_two_view_result* result, const uint8_t* inliers, const float K[4], float sigma, float min_parallax, int min_triangulated,
                                       const sslam_keyline* kl1, int nl1, const sslam_keyline* kl2, int nl2, const double* linefn1, const double* linefn2,
                                       const int32_t* line_pairs, int line_npairs, sslam_two_view_pose* pose, float* p3d, uint8_t* triangulated,
                                       float* line_s3d, float* line_e3d, uint8_t* line_triangulated,
                                       float* hyp_out, float* sel_out, int32_t* stage_out, float* p3d_rows_out, float* cos_out, double* line_err_out);

/* sslam_new_map_points / sslam_new_map_lines for one host pair with what the gates consumed copied back: the same kernels with the stores of their tap enabled, run as
 * pair 0.  Per row: cos_out[row] = cosParallaxRays (:482, :1041; zero for a row without a match or, for a line, one that is not free) and the homogeneous vt.row(3)
 * before the division -- hom_out[row*4 .. +4) of x3D for a point (:509), hom_out[row*8 .. +4) of s3D and [row*8 + 4 .. +4) of e3D for a line (:1065, :1082) -- zeros
 * where the row ended before the decomposition. */
int sslam_testing_new_map_points(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const sslam_kf_pose* pose1, const sslam_kf_pose* pose2,
                                 const int32_t* matches12, const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                                 float* x3d, uint8_t* stage, float* normal, float* dist, int* nnew, float* cos_out, float* hom_out);
int sslam_testing_new_map_lines(sslam_ctx* ctx, const sslam_keyline* kl1, const double* linefn1, int nl1, const sslam_keyline* kl2, const double* linefn2, int nl2,
                                const sslam_kf_pose* pose1, const sslam_kf_pose* pose2, float median_depth2, const int32_t* line_pairs, int line_npairs,
                                const float* scale_factors, int nlevels, float* s3d, float* e3d, uint8_t* stage, double* normal, float* dist, int* nnew,
                                float* cos_out, float* hom_out);

#ifdef __cplusplus
}
#endif
#endif
