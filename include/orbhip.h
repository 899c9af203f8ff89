/*
 * orbhip.h -- C ABI of the MI355X-native ORB front-end + local-BA solver.
 *
 * This is the drop-in boundary: plain pointers and sizes,
 * no C++ / torch / OpenCV types.  Every entry point cites the reference interface
 * it replaces (paths relative to the reference repo root).  Status codes: 0 = ok,
 * negative = error (never throws; see ORBHIP_E_*).  All entry points are thread-safe
 * across distinct contexts; one context = one HIP stream + its own device scratch
 * (mirrors "one ORBextractor instance per thread", src/Frame.cc:109-110).
 *
 * The library REQUIRES a gfx950 device: there is no CPU fallback.  orbhip_ctx_create
 * fails with ORBHIP_E_NODEVICE when no HIP device is present.
 */
#ifndef ORBHIP_H
#define ORBHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORBHIP_OK 0
#define ORBHIP_E_BADARG (-1)
#define ORBHIP_E_NODEVICE (-2)
#define ORBHIP_E_HIP (-3)        /* a HIP runtime call failed; see orbhip_last_error() */
#define ORBHIP_E_CAPACITY (-4)   /* a device-side list overflowed its reserved capacity */
#define ORBHIP_E_ABORTED (-5)    /* BA: stop flag raised (Optimizer.cc:2041-2043) */
#define ORBHIP_E_NOTSPD (-6)     /* BA: reduced system not SPD on every LM trial */
#define ORBHIP_E_EMPTY (-7)      /* extractor: empty image (ORBextractor.cc:1072-1073 returns -1) */

/* cv::KeyPoint layout (28 B): what ORBextractor::operator() fills (ORBextractor.cc:1100). */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbhip_keypoint;

typedef struct orbhip_ctx orbhip_ctx;
typedef struct orbhip_extractor orbhip_extractor;

const char *orbhip_version(void);
const char *orbhip_last_error(void);

/* Device context.  `stream` may be NULL (the library creates its own non-blocking
 * stream) or an existing hipStream_t (e.g. torch's current stream) which is borrowed. */
int orbhip_ctx_create(int device, void *stream, orbhip_ctx **out);
void orbhip_ctx_destroy(orbhip_ctx *ctx);
int orbhip_ctx_synchronize(orbhip_ctx *ctx);
/* Stream order across two contexts of one device, without a host synchronisation: everything submitted to `other` so far completes
 * before anything submitted to `ctx` after this call starts (the reference runs its left / right extractors and its Tracking /
 * LocalMapping / LoopClosing work on separate host threads, src/Frame.cc:109-112; contexts are this library's unit of concurrency). */
int orbhip_ctx_wait_for(orbhip_ctx *ctx, orbhip_ctx *other);
/* Synchronises, then returns and clears the context's sticky device-side error word
 * (ORBHIP_E_CAPACITY when a matcher kernel met more keypoints than it can hold). */
int orbhip_ctx_check_status(orbhip_ctx *ctx);
void *orbhip_ctx_stream(orbhip_ctx *ctx);

/* ------------------------------------------------------------------ ORB extractor */
/* Replaces ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels,
 *   int iniThFAST, int minThFAST)            include/ORBextractor.h:54, src/ORBextractor.cc:408 */
int orbhip_extractor_create(orbhip_ctx *ctx, int nfeatures, float scale_factor, int nlevels,
                            int ini_th_fast, int min_th_fast, orbhip_extractor **out);
void orbhip_extractor_destroy(orbhip_extractor *ext);

/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares                 include/ORBextractor.h:61-79
 * which: 0 scale, 1 inv scale, 2 sigma2, 3 inv sigma2.  out[nlevels]. */
int orbhip_extractor_levels(const orbhip_extractor *ext);
int orbhip_extractor_table(const orbhip_extractor *ext, int which, float *out);
/* mnFeaturesPerLevel (ORBextractor.cc:434-445) and umax (ORBextractor.cc:453-468). */
int orbhip_extractor_features_per_level(const orbhip_extractor *ext, int *out);
int orbhip_extractor_umax(const orbhip_extractor *ext, int *out16);
/* out19[|dy|], |dy| = 0 .. 18: the rBRIEF samples of patch row dy lie in columns [-out19, out19] around the keypoint for every angle
 * (what the descriptor kernel fetches of a tiled blurred level).  Needs no device. */
int orbhip_blur_half_widths(int *out19);
/* The FAST stage's cell table for per-level image sizes w[l] x h[l], decoded: 12 ints per cell of a frame, in the kernel's order (level,
 * then row-major) -- level, first staged pixel x0, y0 (= iniX - 1, iniY of ORBextractor.cc:783-806), detection band dw, dh (0: the cell is
 * skipped), keypoint origin key_x0, key_y0, offset of the cell's list in a frame's lists, and the lane layout of the necessary test: tasks
 * per row, rows per trip, division magic; last the list capacity.  At most cap cells are written.  Returns the cells of a frame, or a
 * negative error.  Needs no device. */
int orbhip_fast_cell_table(int nlevels, const int *w, const int *h, int *out, int cap);

/* Reserve device memory for batches of up to max_batch frames of width x height.
 * Called implicitly by the extract calls; explicit call keeps allocation out of timed code. */
int orbhip_extractor_reserve(orbhip_extractor *ext, int width, int height, int max_batch);
/* Upper bound of keypoints per frame (row capacity of the output arrays). */
int orbhip_extractor_max_keypoints(const orbhip_extractor *ext);

/* Batched ORBextractor::operator()           include/ORBextractor.h:57-59, ORBextractor.cc:1068
 * d_images: DEVICE pointer, u8, frame f at d_images + f*frame_stride, rows at row_stride.
 * Results stay on the device (see orbhip_extractor_results).  lap0/lap1 = vLappingArea.
 * Asynchronous on the context's stream. */
int orbhip_extract_batch_device(orbhip_extractor *ext, const uint8_t *d_images, int width,
                                int height, size_t row_stride, size_t frame_stride, int batch,
                                int lap0, int lap1);
/* Device result arrays of the last batch: kp[batch][max_kp], desc[batch][max_kp][32],
 * count[batch] (nkeypoints), mono_index[batch] (operator()'s return value). */
int orbhip_extractor_results(orbhip_extractor *ext, orbhip_keypoint **d_kp, uint8_t **d_desc,
                             int32_t **d_count, int32_t **d_mono_index);
/* Host convenience == one ORBextractor::operator() call per frame: H2D, extract, D2H, sync.
 * kp_out[batch][cap], desc_out[batch][cap][32], count_out[batch], mono_out[batch].
 * Returns ORBHIP_E_EMPTY for an empty image, ORBHIP_E_CAPACITY if cap < keypoints. */
int orbhip_extract_batch_host(orbhip_extractor *ext, const uint8_t *h_images, int width, int height,
                              size_t row_stride, size_t frame_stride, int batch, int lap0, int lap1,
                              orbhip_keypoint *kp_out, uint8_t *desc_out, int cap,
                              int32_t *count_out, int32_t *mono_out);
/* The same call without the copy into caller arrays: *kp_view / *desc_view point at the extractor's page-locked mirror of the device
 * result arrays (row f at kp_view + f * row_capacity, desc_view + f * row_capacity * 32; count_view[f], mono_view[f]), valid until the
 * extractor's next extract call.  What host/ORBextractor.cc copies into the caller's vector<cv::KeyPoint> / cv::Mat. */
int orbhip_extract_batch_host_view(orbhip_extractor *ext, const uint8_t *h_images, int width, int height, size_t row_stride,
                                   size_t frame_stride, int batch, int lap0, int lap1, const orbhip_keypoint **kp_view,
                                   const uint8_t **desc_view, int *row_capacity, const int32_t **count_view, const int32_t **mono_view);
/* Which kernel blurs a batch of `batch` frames on this extractor's geometry: 0 the LDS tile kernel (small batches), 1 the row-streaming
 * kernel, 2 the matrix-core one (images of up to 320 K pixels (VGA) in batches of 128 frames or more; ORBHIP_BLUR_MFMA=0 / 1 overrides).
 * All three are bit-exact; the choice is a measured one. */
int orbhip_extractor_blur_kernel(const orbhip_extractor *ext, int batch);
/* Which instance runs the per-cell FAST stage on this extractor's geometry (after orbhip_extractor_reserve): 0 k_fast_cells for large cells,
 * 1 k_fast_cells for small cells (every level's cells at most 40 x 36), 2 / 3 k_fast_runs for cells of up to 45 / more rows
 * (ORBHIP_FAST_KERNEL=runs when the extractor reserved).  All four give the same candidate lists (tests/test_gpu_fast_cases.py). */
int orbhip_extractor_fast_kernel(const orbhip_extractor *ext);
/* 1: a call with that many frames keeps the blurred pyramid in tiles of 16 x 8 pixels (the matrix-core blur, unless ORBHIP_BLUR_TILED=0 was
 * set when the extractor reserved); 0: row-major.  orbhip_extractor_get_blurred_level returns row-major bytes either way. */
int orbhip_extractor_blur_tiled(const orbhip_extractor *ext, int batch);
/* How the descriptor kernel divides a call of `batch` frames (test hook): kp_base[l] / kp_cap[l] = the slice of level l in a frame's staging
 * slots (multiples of 4; four consecutive slots are one trip of one wave), *waves_per_xcd = the waves that share the trips of one XCD's frames
 * (frames f, f + 8, ...: wave w takes groups w, w + waves, ... of frames x slots / 4).  ORBHIP_TUNE_DESC_BLOCKS=n caps the workgroups per XCD
 * (2 waves each), so that a small batch runs waves of many trips. */
int orbhip_extractor_desc_plan(const orbhip_extractor *ext, int batch, int32_t *kp_base, int32_t *kp_cap, int32_t *waves_per_xcd);

/* Output rows per band of the row-streaming pyramid kernel at `level` (1 .. nlevels-1) on this extractor's geometry: the most whose walk
 * down the source rows fits the kernel's fixed number of steps on every band of the level.  0: the level takes the tile kernel whatever
 * the batch; -1: nothing reserved yet or no such level. */
int orbhip_extractor_resize_band_rows(const orbhip_extractor *ext, int level);

/* Frame `frame` of the extractor's latest HOST extract call as it still sits on the device (d_kp, d_desc: device pointers into the result
 * arrays) together with its page-locked host mirror and a counter that changes with every extract call.  The *_host_resident matcher
 * entry points below take d_kp / d_desc as their train side, so that Tracking's SearchByProjection(CurrentFrame, ...) right after
 * Frame::ExtractORB (src/Frame.cc:410-417 -> src/Tracking.cc:1911) uploads queries only.  ORBHIP_E_BADARG when the latest call was a
 * device call or failed (no mirror). */
int orbhip_extractor_last_frame(orbhip_extractor *ext, int frame, const orbhip_keypoint **d_kp, const uint8_t **d_desc,
                                const orbhip_keypoint **h_kp_view, const uint8_t **h_desc_view, int32_t *count, unsigned long long *generation);

/* mvImagePyramid[level] of frame `frame` (include/ORBextractor.h:83; read by
 * src/Frame.cc:809,899,913,918).  padded != 0 -> the (w+38)x(h+38) reflect-101 parent
 * buffer, else the w x h ROI.  Synchronous D2H. */
int orbhip_extractor_level_dims(const orbhip_extractor *ext, int level, int *w, int *h);
int orbhip_extractor_get_pyramid_level(orbhip_extractor *ext, int frame, int level, int padded,
                                       uint8_t *h_out, size_t out_stride);
/* All levels of frame `frame` at once, as the reference holds them after operator(): levels_out[l] receives the
 * (w_l+38) x (h_l+38) reflect-101 padded parent of level l (ORBextractor.cc:1160-1173) with row stride strides[l] >= w_l+38;
 * mvImagePyramid[l] is its ROI at (19,19).  One device-to-host pass and one synchronisation for the whole pyramid. */
int orbhip_extractor_get_pyramid_padded(orbhip_extractor *ext, int frame, uint8_t *const *levels_out, const size_t *strides);
/* Parity taps (test hooks; synchronous D2H of intermediate stages of the last batch). */
int orbhip_extractor_get_blurred_level(orbhip_extractor *ext, int frame, int level,
                                       uint8_t *h_out, size_t out_stride);
/* Pre-octree FAST candidates in reference emission order; x,y relative to (16,16). */
int orbhip_extractor_get_fast_candidates(orbhip_extractor *ext, int frame, int level,
                                         int32_t *xs, int32_t *ys, int32_t *scores, int cap,
                                         int32_t *n_out);
/* Post-octree keypoints of one level (level coords, angle set, not scaled), list order. */
int orbhip_extractor_get_level_keypoints(orbhip_extractor *ext, int frame, int level,
                                         orbhip_keypoint *out, int cap, int32_t *n_out);

/* Small batches (the per-frame real-time case, BASELINE config #1) are launch bound: 19 kernel launches per
 * extract call.  With graph mode on, the launches of one orbhip_extract_batch_device / _host call are captured once
 * per (image size, batch, lapping) and replayed as ONE hipGraph; the input is then always staged into the
 * extractor's own level-0 buffer so the captured kernels see fixed addresses.  Results are identical.
 * Ignored while stage profiling is on. */
int orbhip_extractor_set_graph_mode(orbhip_extractor *ext, int enable);

/* Per-stage device time (ms), averaged over the extract calls made since the previous query
 * (at most the 32 most recent), measured with hipEvents recorded on the context's stream
 * around each stage's launches while profiling is enabled.  Stage ids: ORBHIP_STAGE_*. */
#define ORBHIP_STAGE_PYRAMID 0      /* k_resize, nlevels-1 launches */
#define ORBHIP_STAGE_FAST_CELLS 1   /* k_fast_cells (per-cell FAST score + NMS + two-threshold retry, all levels), 1 launch */
#define ORBHIP_STAGE_BLUR 2         /* k_blur (7x7 Gaussian, all levels), 1 launch */
#define ORBHIP_STAGE_OCTREE 3       /* k_octree, 1 launch */
#define ORBHIP_STAGE_DESC 4         /* k_orient_desc, 1 launch */
#define ORBHIP_STAGE_ASSEMBLE 5     /* k_assemble, 1 launch */
#define ORBHIP_STAGE_COUNT 6
int orbhip_extractor_set_profiling(orbhip_extractor *ext, int enable);
int orbhip_extractor_stage_ms(orbhip_extractor *ext, float *ms_out /*[ORBHIP_STAGE_COUNT]*/);

/* ------------------------------------------------------------------ ORB matcher */
/* ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)
 *                                            include/ORBmatcher.h:45, src/ORBmatcher.cc:2353
 * Host-callable scalar (two 32-byte descriptors). */
int orbhip_descriptor_distance(const uint8_t *a32, const uint8_t *b32);

/* Batched all-pairs 2-NN == cv::BFMatcher(NORM_HAMMING).knnMatch(k=2), the matcher of
 * Frame::ComputeStereoFishEyeMatches          src/Frame.cc:43,1146-1153
 * (that member itself, lapping slices and triangulation included: orbhip_compute_stereo_fisheye_matches_*)
 * For pair p: queries d_descA + p*strideA (nA[p] rows), train d_descB + p*strideB (nB[p] rows).
 * Outputs per query row: idx[2], dist[2] (ascending; strict <, lowest index wins ties;
 * idx -1 / dist INT_MAX when fewer than k train rows) and ratio-test flag
 * (float)d0 < (float)d1*ratio evaluated in double as in Frame.cc:1153 (ratio there: 0.7).
 * Row q of pair p lands at [p*max_n + q].  All pointers DEVICE.  max_n <= 65535 (else ORBHIP_E_BADARG). */
int orbhip_match_bf2nn_device(orbhip_ctx *ctx, const uint8_t *d_descA, const int32_t *d_nA,
                              size_t strideA, const uint8_t *d_descB, const int32_t *d_nB,
                              size_t strideB, int pairs, int max_n, double ratio,
                              int32_t *d_idx2, int32_t *d_dist2, uint8_t *d_accept);

/* Batched ORBmatcher::SearchForInitialization(F1,F2,vbPrevMatched,vnMatches12,windowSize)
 *                                            include/ORBmatcher.h:66, src/ORBmatcher.cc:710-825
 * including Frame::AssignFeaturesToGrid / GetFeaturesInArea semantics
 *                                            src/Frame.cc:377-408,645-726
 * Pair p matches frame A_p against frame B_p.  kp arrays are the extractor's device
 * outputs (row capacity max_n).  d_prev_matched[pairs][max_n][2] (float x,y) is in/out
 * (vbPrevMatched); d_matches12[pairs][max_n] out; d_nmatches[pairs] out (return value).
 * Grid bounds = image bounds (mnMinX..mnMaxX of a distortion-free camera).  At most 8192
 * keypoints and 4096 octave-0 keypoints per frame -- the monocular-initialisation extractor runs
 * 5 x nFeatures (src/Tracking.cc:210) -- else the context's status word is set
 * (orbhip_ctx_check_status).  Scratch (LDS) is sized from max_n. */
int orbhip_search_for_initialization_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kpA, const uint8_t *d_descA, const int32_t *d_nA,
        const orbhip_keypoint *d_kpB, const uint8_t *d_descB, const int32_t *d_nB,
        int pairs, int max_n, size_t frame_stride_kp /*entries*/, float min_x, float min_y,
        float max_x, float max_y, int window_size, float nn_ratio, int check_orientation,
        float *d_prev_matched, int32_t *d_matches12, int32_t *d_nmatches);

/* vbPrevMatched[i] = mvKeysUn[i].pt for `frames` frames (src/Tracking.cc:1497-1499), on the device:
 * d_prev_matched[f][i] = (kp[f][i].x, kp[f][i].y), rows of max_n entries. */
int orbhip_prev_matched_init_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp, size_t frame_stride_kp,
                                    int frames, int max_n, float *d_prev_matched);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
 * (src/ORBmatcher.cc:1965-2181, CurrentFrame.Nleft == -1: monocular / rectified stereo) -- the matcher of
 * Tracking::TrackWithMotionModel (src/Tracking.cc:2683-2694).  The projection of the last frame's map
 * points (ORBmatcher.cc:1992-2008) stays host geometry; each surviving point arrives as one query:
 *   u, v       uv = CurrentFrame.mpCamera->project(x3Dc)                       (ORBmatcher.cc:2003)
 *   radius     th * CurrentFrame.mvScaleFactors[nLastOctave]                   (:2014)
 *   ur         uv.x - CurrentFrame.mbf * invzc                                 (:2043)
 *   angle      angle of the last frame's (undistorted) keypoint                (:2067-2073)
 *   min_level, max_level   level arguments of the GetFeaturesInArea call picked by bForward / bBackward
 *              (:2018-2023): (oct,-1) | (0,oct) | (oct-1,oct+1); -1 = open end (src/Frame.cc:676)
 *   has_obs    pMP->Observations() > 0: a keypoint claimed by such a point is no candidate for later
 *              queries (:2037-2039)
 * Train side = CurrentFrame: mvKeysUn (x, y, octave, angle of orbhip_keypoint), descriptors, optional
 * mvuRight (NULL = monocular, all -1), image bounds mnMinX..mnMaxY for the 64x48 grid (src/Frame.cc:377-408,
 * 645-726).  d_train_match [pairs][max_n] is CurrentFrame.mvpMapPoints, in/out: entry -1 = free, anything else
 * = already holds a map point with observations (returned as -2, never matched); on return a value >= 0 is the
 * index of the query that owns the keypoint.  d_nmatches[pair] = the function's return value (rotation
 * consistency, :2156-2178, applied when check_orientation).  th_high = ORBmatcher::TH_HIGH = 100 (:40).
 * At most 2048 queries and 2048 keypoints per pair (else the context status becomes ORBHIP_E_CAPACITY).
 * Pair p reads queries at d_q + p*max_q, keypoints at d_kp + p*frame_stride_kp.  All pointers DEVICE. */
typedef struct orbhip_proj_query {
    float u, v, radius, ur, angle;
    int32_t min_level, max_level, has_obs;
} orbhip_proj_query;
int orbhip_search_by_projection_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                       const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp,
                                       const uint8_t *d_desc, const float *d_u_right, const int32_t *d_n, int max_n,
                                       size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x,
                                       float max_y, int th_high, int check_orientation, int32_t *d_train_match,
                                       int32_t *d_nmatches);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:48-218, F.Nleft == -1) -- the matcher of Tracking::SearchLocalPoints (src/Tracking.cc:3096).
 * Same layout and claim rule as orbhip_search_by_projection_device; one query per map point that passes :57-67:
 * u, v = mTrackProjX/Y; radius = RadiusByViewingCos(mTrackViewCos) [* th] * F.mvScaleFactors[nPredictedLevel]
 * (:72-79); (min_level, max_level) = (nPredictedLevel-1, nPredictedLevel); ur = mTrackProjXR; angle unused.
 * A match needs best <= th_high and, when best and second best lie in the same octave, best <= nn_ratio * second
 * (mfNNratio, :131-137).  No rotation histogram. */
int orbhip_search_local_map_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                   const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp,
                                   const uint8_t *d_desc, const float *d_u_right, const int32_t *d_n, int max_n,
                                   size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x,
                                   float max_y, int th_high, float nn_ratio, int32_t *d_train_match,
                                   int32_t *d_nmatches);

/* The two searches above on frames of a two-camera rig (CurrentFrame.Nleft != -1: TUM-VI stereo-fisheye, src/Frame.cc:1034-1126) --
 * ORBmatcher.cc:2013-2016 + :2089-2153 (mode 0: SearchByProjection(CurrentFrame, LastFrame, ...)) and :113-122 + :136-214 (mode 1:
 * SearchByProjection(F, vpMapPoints, ...)).  The train side is the whole frame: keypoints [0, d_nleft[pair]) = F.mvKeys (left camera),
 * [d_nleft[pair], d_n[pair]) = F.mvKeysRight, descriptors likewise (F.mDescriptors rows, ORBmatcher.cc:176); each camera has its own
 * grid (mGrid / mGridRight, src/Frame.cc:395-405) and there is no uRight gate.  A query searches the LEFT camera's grid, or the RIGHT
 * one's when bit 1 of has_obs is set (bit 0 keeps its meaning); the caller emits a point's left query (u, v = projection in the left
 * camera) and then its right query (projection in the right camera: :2090-2092, or mTrackProjXR / YR with radius
 * RadiusByViewingCos(mTrackViewCosR) * scale[mnTrackScaleLevelR], :151-156) in the reference's order, so the claim rule sees the same
 * sequence.  d_mirror [pairs][max_n] (mode 1; may be NULL): for every keypoint the frame-wide index of the same point's keypoint in the
 * other camera -- mvLeftToRightMatch[i] + Nleft for i < Nleft, mvRightToLeftMatch[i - Nleft] otherwise -- or -1: a match also assigns
 * that keypoint and counts twice (:142-146, :203-207).  Outputs as in the single-camera calls (d_train_match indexed frame-wide). */
int orbhip_search_by_projection_rig_device(orbhip_ctx *ctx, int mode, const orbhip_proj_query *d_q, const uint8_t *d_desc_q,
                                           const int32_t *d_nq, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc,
                                           const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n,
                                           size_t frame_stride_kp, int pairs, float min_x, float min_y, float max_x, float max_y,
                                           int th_high, float nn_ratio, int check_orientation, int32_t *d_train_match,
                                           int32_t *d_nmatches);

/* DIAGNOSTIC (tests): which pairs of this context's most recent orbhip_search_by_projection_device / orbhip_search_local_map_device /
 * orbhip_search_by_projection_rig_device launch the replay form handed back to the sequential kernel (a query's truncated candidate list
 * ran dry, or a query had more than 512 candidates).  Waits for the context's stream, then copies min(cap, *pairs_out) flags (1 = handed
 * back) to the HOST array flags_out; *pairs_out = the launch's pair count, or 0 when it ran the sequential kernel alone (rig frames, rows
 * beyond 2048, ORBHIP_SBP_PARALLEL_MAX_PAIRS).  The flags live in the context's work arena: they are only meaningful until the next
 * call of any entry point on this context.  Read-only; the results of the launch do not depend on it. */
int orbhip_debug_sbp_handed_back(orbhip_ctx *ctx, int32_t *flags_out, int cap, int *pairs_out);

/* Host-pointer forms of the two calls above for ONE frame (what an ORBmatcher method with the reference's signature needs:
 * host/ORBmatcher.cc): upload into the context's arena, run the same kernel, download, synchronise.  mode 0 =
 * orbhip_search_by_projection_device (nn_ratio unused), 1 = orbhip_search_local_map_device (check_orientation unused).
 * u_right may be NULL (monocular).  train_match_inout [n] as d_train_match.  All pointers HOST. */
int orbhip_search_by_projection_host(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                     const orbhip_keypoint *kp, const uint8_t *desc, const float *u_right, int n,
                                     float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                     int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out);
/* ... and of orbhip_search_by_projection_rig_device: kp / desc are the frame's left | right keypoints, nleft = Nleft, mirror [n] or NULL. */
int orbhip_search_by_projection_rig_host(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                         const orbhip_keypoint *kp, const uint8_t *desc, int n, int nleft, const int32_t *mirror,
                                         float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                         int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out);
/* Host-pointer form of orbhip_search_for_initialization_device for one frame pair: prev_matched_inout [nA][2] is vbPrevMatched
 * (in/out), matches12_out [nA] is vnMatches12, *nmatches_out the return value.  All pointers HOST. */
int orbhip_search_for_initialization_host(orbhip_ctx *ctx, const orbhip_keypoint *kpA, const uint8_t *descA, int nA,
                                          const orbhip_keypoint *kpB, const uint8_t *descB, int nB, float min_x, float min_y,
                                          float max_x, float max_y, int window_size, float nn_ratio, int check_orientation,
                                          float *prev_matched_inout, int32_t *matches12_out, int32_t *nmatches_out);
/* The same host-pointer calls with the TRAIN side already on the device: d_kp / d_desc (d_kpB / d_descB) are DEVICE pointers to n
 * keypoints and descriptors -- the result arrays of the extraction that produced the frame (orbhip_extractor_last_frame).  This is
 * the shape of Tracking's calls: SearchByProjection(mCurrentFrame, mLastFrame, ...) (src/Tracking.cc:1911), SearchLocalPoints'
 * SearchByProjection(mCurrentFrame, vpMapPoints, ...) (:3083) and SearchForInitialization(mInitialFrame, mCurrentFrame, ...) (:1506)
 * all search the frame whose features the extractor left on the device a moment ago; only the queries (map point projections and
 * descriptors) travel.  host/frame_cache.h decides when a Frame IS that extraction (byte comparison with the page-locked mirror).
 * d_kp may be NULL while d_desc is given: the frame's descriptors are the extraction's but its keypoints are not (mvKeysUn of a camera
 * with distortion, src/Frame.cc:738-771) -- then kp_host [n] is uploaded.  Single-camera frames only.  Everything else HOST, results
 * identical to the forms above. */
int orbhip_search_by_projection_host_resident(orbhip_ctx *ctx, int mode, const orbhip_proj_query *q, const uint8_t *desc_q, int nq,
                                              const orbhip_keypoint *kp_host, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *u_right, int n,
                                              float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
                                              int check_orientation, int32_t *train_match_inout, int32_t *nmatches_out);
int orbhip_search_for_initialization_host_resident(orbhip_ctx *ctx, const orbhip_keypoint *kpA, const uint8_t *descA, int nA,
                                                   const orbhip_keypoint *kpB_host, const orbhip_keypoint *d_kpB, const uint8_t *d_descB, int nB, float min_x, float min_y,
                                                   float max_x, float max_y, int window_size, float nn_ratio, int check_orientation,
                                                   float *prev_matched_inout, int32_t *matches12_out, int32_t *nmatches_out);

/* The search part of ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th, bRight)
 * (src/ORBmatcher.cc:1403-1613, NLeft == -1; LocalMapping::SearchInNeighbors, src/LocalMapping.cc:781-860), batched over
 * (keyframe, point set) pairs.  The per-point geometry of :1430-1497 stays with the caller; each surviving point is one
 * query: u, v = uv; radius = th * pKF->mvScaleFactors[nPredictedLevel]; ur = uv.x - bf*invz; min_level / max_level =
 * nPredictedLevel-1 / nPredictedLevel (angle, has_obs unused).  Per query: the keypoint inside the window, at an allowed
 * octave, whose reprojection error passes e2 * mvInvLevelSigma2[octave] <= 5.99 (7.8 with a right coordinate,
 * mvuRight >= 0) and whose descriptor distance is smallest (first minimum in GetFeaturesInArea order, :1527-1568).
 * d_best_idx / d_best_dist [pairs][max_q] = bestIdx (-1 = none) / bestDist (256 = none); the caller applies
 * bestDist <= TH_LOW and the Replace / AddObservation bookkeeping (:1572-1595) in order.  inv_level_sigma2: HOST array
 * of nlevels floats.  At most 2900 keypoints per keyframe (they and their descriptors are LDS-resident; more sets the
 * context status to ORBHIP_E_CAPACITY).  All other pointers DEVICE. */
int orbhip_fuse_search_device(orbhip_ctx *ctx, const orbhip_proj_query *d_q, const uint8_t *d_desc_q, const int32_t *d_nq,
                              int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *d_u_right,
                              const int32_t *d_n, int max_n, size_t frame_stride_kp, int pairs,
                              const float *inv_level_sigma2, int nlevels, float min_x, float min_y, float max_x, float max_y,
                              int32_t *d_best_idx, int32_t *d_best_dist);

/* ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (src/ORBmatcher.cc:273-475,
 * F.Nleft == -1) -- the matcher of Tracking::TrackReferenceKeyFrame (src/Tracking.cc:1757) and Relocalization
 * (:3290-3300), batched over (keyframe, frame) pairs.  The DBoW2 FeatureVectors (map<NodeId, vector<feature index>>,
 * pKF->mFeatVec / F.mFeatVec) arrive flattened per pair: node ids ascending [pairs][max_nodes], node_start
 * [pairs][max_nodes+1] into feat [pairs][max_n], number of nodes [pairs] (orbhip_bow_transform_device yields the node of
 * every feature).  d_kf_valid [pairs][max_n]: the keyframe's map point at that feature exists and is not bad (:297-302).
 * Inside a shared node every valid keyframe feature, in order, takes the best still unmatched frame feature if
 * best <= TH_LOW and best < nn_ratio * second (:304-366); rotation consistency (:445-470) when check_orientation.
 * d_match_f [pairs][max_n]: per frame feature the keyframe feature whose map point it receives, or -1
 * (vpMapPointMatches[j] = vpMapPointsKF[d_match_f[j]]); d_nmatches [pairs] = the return value.  At most 4096 features per
 * frame (their descriptors are LDS-resident).  All pointers DEVICE. */
int orbhip_search_by_bow_device(orbhip_ctx *ctx,
        const int32_t *d_kf_node_ids, const int32_t *d_kf_node_start, const int32_t *d_kf_feat, const int32_t *d_kf_nnodes,
        const uint8_t *d_kf_valid, const orbhip_keypoint *d_kf_kp, const uint8_t *d_kf_desc,
        const int32_t *d_f_node_ids, const int32_t *d_f_node_start, const int32_t *d_f_feat, const int32_t *d_f_nnodes,
        const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, const int32_t *d_nF,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_match_f, int32_t *d_nmatches);

/* orbhip_search_by_bow_device for frames of a two-camera rig (F.Nleft != -1, ORBmatcher.cc:338-359, :393-425): frame features
 * [0, d_nleft[pair]) are the left camera's, the rest the right camera's (F.mDescriptors order; keypoints concatenated mvKeys | mvKeysRight,
 * on the keyframe side too).  Every keyframe feature keeps a best / second best PER CAMERA; when the left best passes TH_LOW the left
 * match needs the ratio test and the right camera's best is taken whenever it passes TH_LOW (the reference's "|| true").  Everything
 * else as orbhip_search_by_bow_device. */
int orbhip_search_by_bow_rig_device(orbhip_ctx *ctx,
        const int32_t *d_kf_node_ids, const int32_t *d_kf_node_start, const int32_t *d_kf_feat, const int32_t *d_kf_nnodes,
        const uint8_t *d_kf_valid, const orbhip_keypoint *d_kf_kp, const uint8_t *d_kf_desc,
        const int32_t *d_f_node_ids, const int32_t *d_f_node_start, const int32_t *d_f_feat, const int32_t *d_f_nnodes,
        const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, const int32_t *d_nF, const int32_t *d_nleft,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_match_f, int32_t *d_nmatches);

/* Host-pointer form for ONE (keyframe, frame) pair -- what the ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 * method of host/ORBmatcher.cc calls: flattened FeatureVectors (node ids ascending, node_start [nnodes + 1], feature indices),
 * kf_valid [nK], keypoints and descriptors of both sides; nleft < 0 for F.Nleft == -1, else the rig form.  match_f_out [nF]. */
int orbhip_search_by_bow_host(orbhip_ctx *ctx,
        const int32_t *kf_node_ids, const int32_t *kf_node_start, const int32_t *kf_feat, int kf_nnodes, const uint8_t *kf_valid,
        const orbhip_keypoint *kf_kp, const uint8_t *kf_desc, int nK,
        const int32_t *f_node_ids, const int32_t *f_node_start, const int32_t *f_feat, int f_nnodes,
        const orbhip_keypoint *f_kp, const uint8_t *f_desc, int nF, int nleft,
        float nn_ratio, int check_orientation, int32_t *match_f_out, int32_t *nmatches_out);
/* ... with the FRAME side (d_f_kp, d_f_desc: device pointers, nF entries) resident as above; single-camera frames. */
int orbhip_search_by_bow_host_resident(orbhip_ctx *ctx,
        const int32_t *kf_node_ids, const int32_t *kf_node_start, const int32_t *kf_feat, int kf_nnodes, const uint8_t *kf_valid,
        const orbhip_keypoint *kf_kp, const uint8_t *kf_desc, int nK,
        const int32_t *f_node_ids, const int32_t *f_node_start, const int32_t *f_feat, int f_nnodes,
        const orbhip_keypoint *f_kp_host, const orbhip_keypoint *d_f_kp, const uint8_t *d_f_desc, int nF,
        float nn_ratio, int check_orientation, int32_t *match_f_out, int32_t *nmatches_out);

/* ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (src/ORBmatcher.cc:827-967,
 * NLeft == -1) -- the matcher of LoopClosing's Sim3 candidates (src/LoopClosing.cc:1005, 2284), batched over keyframe
 * pairs.  Layout as orbhip_search_by_bow_device; both sides carry d_valid [pairs][max_n] (map point exists and is not
 * bad, :867-871, :887-894) and their feature counts d_n1 / d_n2 [pairs].  Inside a shared node every valid KF1 feature,
 * in order, takes the best valid, still unclaimed KF2 feature if best < TH_LOW (strict, :909) and best < nn_ratio *
 * second.  d_matches12 [pairs][max_n]: per KF1 feature the KF2 feature whose map point it receives, or -1
 * (vpMatches12[i] = vpMapPoints2[d_matches12[i]]).  At most 4096 features per keyframe.  All pointers DEVICE. */
int orbhip_search_by_bow_kf_device(orbhip_ctx *ctx,
        const int32_t *d_node_ids1, const int32_t *d_node_start1, const int32_t *d_feat1, const int32_t *d_nnodes1,
        const uint8_t *d_valid1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_valid2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const int32_t *d_n2,
        int pairs, int max_nodes, int max_n, size_t frame_stride_kp, float nn_ratio, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches);

/* Per keyframe pair of orbhip_search_for_triangulation_device: F12 = K1^-T [t12]x R12 K2^-1 (row-major; computed by the
 * caller with the reference's own matrix arithmetic, CameraModels/Pinhole.cpp:124-127), the epipole of KF1's centre in KF2
 * (ORBmatcher.cc:978-992), and the bOnlyStereo / bCoarse arguments. */
typedef struct orbhip_tri_pair { float F12[9]; float ep_x, ep_y; int32_t only_stereo, coarse; } orbhip_tri_pair;

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:969-1210;
 * Pinhole cameras, mpCamera2 == 0) -- the matcher of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:459-460),
 * batched over keyframe pairs.  d_nid1 [pairs][max_n]: vocabulary node of every KF1 feature (orbhip_bow_transform_device);
 * KF2's FeatureVector flattened as in orbhip_search_by_bow_device.  d_has_mp* [pairs][max_n]: the keypoint already has a map
 * point (:1039, :1067); d_u_right* [pairs][max_n] = mvuRight or NULL (monocular).  Per KF1 keypoint without a map point:
 * the KF2 keypoint of the same node, without a map point, with the smallest descriptor distance <= TH_LOW (a later
 * candidate at equal distance replaces an earlier one, :1073) that is not within 10*sqrt(scale) px of the epipole (both
 * monocular, :1083-1091) and passes Pinhole::epipolarConstrain (or any, if coarse); this fork never sets vbMatched2, so
 * KF1 keypoints are independent.  Rotation consistency (:1171-1189) when check_orientation.  d_matches12 [pairs][max_n] =
 * vMatches12 (idx2 or -1; vMatchedPairs is its non-negative entries in index order), d_nmatches [pairs] = the return
 * value.  scale_factors / level_sigma2: HOST arrays of nlevels floats (KF2's mvScaleFactors / mvLevelSigma2).  At most 4096
 * features per keyframe.  KannalaBrandt8 pairs (epipolarConstrain by triangulation) and rigs (mpCamera2) are not covered.
 * All other pointers DEVICE. */
int orbhip_search_for_triangulation_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const float *d_u_right1,
        const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const float *d_u_right2, const int32_t *d_n2,
        const orbhip_tri_pair *d_pair, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *scale_factors, const float *level_sigma2, int nlevels, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches);

/* ORBmatcher::SearchForTriangulation for EVERY camera combination of the reference (src/ORBmatcher.cc:969-1210): single Pinhole or
 * KannalaBrandt8 cameras and two-camera rigs (pKF->mpCamera2 != 0, NLeft != -1: TUM-VI stereo-fisheye).  Per keyframe pair: */
typedef struct orbhip_tri_pair_general {
    float R12[4][9], t12[4][3];          /* X1 = R12 X2 + t12 of the camera pair [2*bRight1 + bRight2]: ll, lr, rl, rr (:994-1008; the caller
                                            keeps the reference's cv::Mat arithmetic); a single-camera pair uses [0] (:996-997) */
    float F12[4][9];                     /* K1^-T [t12]x R12 K2^-1 of the same combinations, row-major: what Pinhole::epipolarConstrain
                                            builds (src/CameraModels/Pinhole.cpp:124-127); read only when the first camera is a Pinhole */
    float cam1[2][8], cam2[2][8];        /* mvParameters (fx fy cx cy k1..k4) of pKF1->mpCamera / mpCamera2 and of pKF2's */
    int32_t cam1_type[2], cam2_type[2];  /* 0 Pinhole, 1 KannalaBrandt8 */
    float ep_x, ep_y;                    /* pKF2->mpCamera->project(R2w Cw + t2w) (:978-984) */
    int32_t nleft1, nleft2;              /* NLeft; -1 = single camera.  Rig keyframes: keypoints and flags in mvKeys | mvKeysRight order
                                            (= descriptor rows), bRight = index >= NLeft (:1055, :1087) */
    int32_t only_stereo, coarse;
} orbhip_tri_pair_general;
/* Layout as orbhip_search_for_triangulation_device.  The candidate test is GeometricCamera::epipolarConstrain of the FIRST camera of
 * the picked pair: Pinhole -> distance to the epipolar line of F12[c] (Pinhole.cpp:129-143); KannalaBrandt8 -> TriangulateMatches
 * (src/CameraModels/KannalaBrandt8.cpp:235-238, 334-401: ray parallax < 0.9998, linear triangulation by the SVD of a 4x4 system,
 * both depths positive, reprojection errors <= 5.991 sigma^2 in both cameras, z1 > 1e-4).  Rig pairs have no stereo keypoints
 * (bStereo needs mpCamera2 == 0, :1044) and skip the epipole test (:1091).  level_sigma2_1 = pKF1->mvLevelSigma2, scale_factors2 /
 * level_sigma2_2 = pKF2's (HOST arrays of nlevels floats).  cv::SVD (one-sided Jacobi) and the float libm calls are restated as
 * DESIGN.md 2 describes: parity unpinned against an OpenCV build, bit-exact against the oracle. */
int orbhip_search_for_triangulation_general_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const float *d_u_right1,
        const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const float *d_u_right2, const int32_t *d_n2,
        const orbhip_tri_pair_general *d_pair, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2, int nlevels, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches);

/* ORBmatcher::SearchForTriangulation, the overload that also returns the triangulated points (src/ORBmatcher.cc:1212-1402, no caller
 * in the reference).  Per candidate the camera and pose of each side are picked by bRight (:1307-1321) and the test is
 * GeometricCamera::matchAndtriangulate of the FIRST camera: KannalaBrandt8 (src/CameraModels/KannalaBrandt8.cpp:240-332: ray parallax
 * < 0.9998 with the rays turned into the world frame, linear triangulation with the ABSOLUTE poses, both depths positive,
 * reprojection errors <= 5.991 sigma^2 in both cameras) or Pinhole, whose implementation is `{ return false; }`
 * (include/CameraModels/Pinhole.h:91-94): a pair whose first camera is a Pinhole matches nothing.  bOnlyStereo is not read by that
 * overload, there is no epipole gate and vbMatched2 is never set.  d_pair: cam1 / cam2 / cam*_type / nleft1 / nleft2 are read (the
 * rest ignored); d_poses: rows 0..2 of GetPose() ([0]) and GetRightPose() ([1]) of both keyframes, row-major 3x4.
 * d_points12 [pairs][max_n][3]: x3Dtriangulated (a WORLD point) of the kept match of KF1 keypoint i (zeros where matches12 < 0;
 * entries of matches the rotation histogram removed keep their point, as vMatchesPoints12 does). */
typedef struct orbhip_tri_pair_poses { float Tcw1[2][12], Tcw2[2][12]; } orbhip_tri_pair_poses;
int orbhip_match_and_triangulate_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const int32_t *d_n2,
        const orbhip_tri_pair_general *d_pair, const orbhip_tri_pair_poses *d_poses, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *level_sigma2_2, int nlevels, int check_orientation,
        int32_t *d_matches12, float *d_points12, int32_t *d_nmatches);
/* one pair, HOST pointers (as orbhip_search_for_triangulation_host below); points12_out [n1][3] */
int orbhip_match_and_triangulate_host(orbhip_ctx *ctx,
        const int32_t *nid1, const uint8_t *has_mp1, const orbhip_keypoint *kp1, const uint8_t *desc1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2,
        const uint8_t *has_mp2, const orbhip_keypoint *kp2, const uint8_t *desc2, int n2,
        const orbhip_tri_pair_general *pair, const orbhip_tri_pair_poses *poses, const float *level_sigma2_1, const float *level_sigma2_2,
        int nlevels, int check_orientation, int32_t *matches12_out, float *points12_out, int32_t *nmatches_out);

/* LocalMapping::CreateNewMapPoints, the per-match loop (src/LocalMapping.cc:479-724), on the matches SearchForTriangulation leaves on
 * the device.  Per keyframe pair (KF1 = mpCurrentKeyFrame, KF2 = the neighbour): */
typedef struct orbhip_newpoints_pair {
    float cam1[2][8], cam2[2][8];        /* as orbhip_tri_pair_general: mvParameters of mpCamera / mpCamera2; [0] also gives the keyframe's */
    int32_t cam1_type[2], cam2_type[2];  /*   fx fy cx cy (and invfx / invfy = 1.0f / fx, fy) of the stereo formulas; 0 Pinhole, 1 KannalaBrandt8 */
    int32_t nleft1, nleft2;              /* NLeft; -1 = single camera.  Both -1 or both rigs (a mixed pair is ORBHIP_E_BADARG: there the
                                            reference reuses the matrices an earlier match left behind) */
    float Tcw1[2][12], Tcw2[2][12];      /* as orbhip_tri_pair_poses: rows 0..2 of GetPose() ([0]) and GetRightPose() ([1]), row-major 3x4;
                                            Rcw / tcw / Rwc of :409-414, :465-470, :503-568 are their blocks.  Single-camera pairs use [0] */
    float Twc1[12], Twc2[12];            /* rows 0..2 of GetPoseInverse(): KeyFrame::UnprojectStereo (KeyFrame.cc:833) */
    float Ow1[2][3], Ow2[2][3];          /* GetCameraCenter() ([0]) and GetRightCameraCenter() ([1]) */
    float mb1, mb2;                      /* mb of the two keyframes (:583, :585) */
    float mbf;                           /* mpCurrentKeyFrame->mbf: read for BOTH keyframes (:656, :681) */
    float ratio_factor;                  /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:424) */
    int32_t far_points;                  /* mbFarPoints */
    float th_far_points;                 /* mThFarPoints */
} orbhip_newpoints_pair;
/* Keypoints, u_right and counts in the layout of orbhip_search_for_triangulation_general_device (d_kp* [pairs][frame_stride_kp]: mvKeysUn,
 * or mvKeys | mvKeysRight of a rig keyframe; d_u_right* [pairs][max_n] = mvuRight or NULL; d_n* [pairs]); d_depth* [pairs][max_n] =
 * mvDepth (NULL exactly when d_u_right* is); d_kp*_raw = mvKeys for UnprojectStereo (KeyFrame.cc:826-827), NULL = the same as d_kp*.
 * d_matches12 [pairs][max_n] as the search leaves it (idx2 or -1; an index >= n2 counts as -1).  `pair` is a HOST array of `pairs`
 * records: it is checked here and copied into the context's arena, and may be reused as soon as the call returns.  level_sigma2_* /
 * scale_factors_*: HOST arrays of nlevels <= 16 floats, mvLevelSigma2 / mvScaleFactors of the two keyframes.  All other pointers DEVICE.
 * Per match, exactly as the reference writes it: bStereo = (mpCamera2 == 0 && uRight >= 0), bRight = idx >= NLeft, pose and camera among
 * ll / lr / rl / rr; ray parallax against cos(2 atan2(mb/2, mvDepth)) of KF1 if it is stereo, ELSE of KF2 (:582-585); linear
 * triangulation with the absolute poses (the 4x4 SVD of orbhip_match_and_triangulate_device) or UnprojectStereo of KF1 / KF2;
 * both depths > 0; reprojection (5.991 / 7.8 sigma^2); dist != 0, mbFarPoints, the scale-ratio test.  mbInertial does not change
 * the condition at :590-591 and is no input.  Outputs per KF1 keypoint i:
 *   d_x3D [pairs][max_n][3]: the world point of a created map point, zeros elsewhere;
 *   d_outcome [pairs][max_n]: 0 no match, 1 created by triangulation, 2 created from KF1's stereo depth, 3 from KF2's, 4 low parallax
 *     and no stereo (:622), 5 w == 0 (:605), 6 empty stereo point (depth <= 0), 7 z1 <= 0, 8 z2 <= 0, 9 reprojection in KF1, 10 in KF2,
 *     11 a zero distance, 12 far point, 13 scale ratio;
 *   d_n_created [pairs]: the number of codes 1..3.
 * d_has_mp1 / d_has_mp2 [pairs][max_n] (NULL = no update): 1 is stored at idx1 and idx2 of every created point, what AddMapPoint
 * (:715-716) means to the next SearchForTriangulation (ORBmatcher.cc:1039, :1067).  Several matches may name one idx2 (this fork never
 * sets vbMatched2): each creates its own point, as in the reference.
 * Asynchronous on the context's stream; calls on one context are stream-ordered, so handing the same has_mp1 row to successive
 * (search, create) calls IS the reference's neighbour loop (:427-725) without a host visit: neighbour i + 1 is searched against the
 * flags neighbour i's points have set.  max_n <= 16384 (else ORBHIP_E_CAPACITY); bad arguments give ORBHIP_E_BADARG; both name the
 * field through orbhip_last_error().  A pair with n1 or n2 outside [0, max_n] sets the context's status word (ORBHIP_E_CAPACITY on
 * orbhip_ctx_check_status) and keeps its x3D / outcome / flag rows untouched (n_created = 0).  cv::SVD, the cv::Mat products and the
 * libm calls are restated as for orbhip_match_and_triangulate_device: parity unpinned against an OpenCV build. */
int orbhip_create_new_map_points_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kp1, const orbhip_keypoint *d_kp1_raw, const float *d_u_right1, const float *d_depth1, const int32_t *d_n1,
        const orbhip_keypoint *d_kp2, const orbhip_keypoint *d_kp2_raw, const float *d_u_right2, const float *d_depth2, const int32_t *d_n2,
        const int32_t *d_matches12, const orbhip_newpoints_pair *pair, int pairs, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors1, const float *level_sigma2_2, const float *scale_factors2, int nlevels,
        uint8_t *d_has_mp1, uint8_t *d_has_mp2, float *d_x3D, uint8_t *d_outcome, int32_t *d_n_created);

/* One keyframe of orbhip_create_new_map_points_host, HOST pointers: what SearchForTriangulation and the per-match loop read of it. */
typedef struct orbhip_newpoints_keyframe {
    const orbhip_keypoint *kp;           /* [n] mvKeysUn, or mvKeys | mvKeysRight of a rig keyframe */
    const orbhip_keypoint *kp_raw;       /* [n] mvKeys (UnprojectStereo), or NULL = kp */
    const uint8_t *desc;                 /* [n][32] */
    const float *u_right, *depth;        /* [n] mvuRight / mvDepth, or both NULL */
    const uint8_t *has_mp;               /* [n] GetMapPoint(i) != NULL when CreateNewMapPoints starts */
    int32_t n;
    const int32_t *nid;                  /* current keyframe: [n] vocabulary node of every feature (-1 = none); neighbours: NULL */
    const int32_t *node_ids, *node_start, *feat;   /* neighbours: the FeatureVector flattened as in orbhip_search_by_bow_device; current: NULL */
    int32_t nnodes;
    const float *level_sigma2, *scale_factors;     /* [nlevels] mvLevelSigma2 / mvScaleFactors */
} orbhip_newpoints_keyframe;
/* The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:427-725) for ONE current keyframe and the n_neigh
 * neighbours that survived the host-side skips, in order: per neighbour k SearchForTriangulation (the general kernel, geom[k]; its
 * only_stereo / coarse are honoured) and then the per-match loop (pair[k]) WITH the flag update, so that neighbour k + 1 is searched
 * against the flags neighbour k's points have set -- one upload (one page-locked blob), all launches on the context's stream, one
 * download, one synchronisation.  All pointers HOST.  Outputs, row k of neighbour k, rows of cur->n entries: matches12_out
 * [n_neigh][n1] (vMatches12), x3D_out [n_neigh][n1][3], outcome_out [n_neigh][n1], n_created_out [n_neigh]; has_mp1_out [n1] (or
 * NULL): KF1's flags after the last neighbour.  The caller replays :710-723 from them.  Limits and errors as the device form (a
 * keyframe of more than 16384 features: ORBHIP_E_CAPACITY). */
int orbhip_create_new_map_points_host(orbhip_ctx *ctx, const orbhip_newpoints_keyframe *cur, const orbhip_newpoints_keyframe *neigh,
        const orbhip_tri_pair_general *geom, const orbhip_newpoints_pair *pair, int n_neigh, int nlevels, int check_orientation,
        int32_t *matches12_out, float *x3D_out, uint8_t *outcome_out, int32_t *n_created_out, uint8_t *has_mp1_out);

/* Host-pointer forms for ONE keyframe (pair) -- what the ORBmatcher methods of host/ORBmatcher.cc call (upload into the context's
 * arena, the same kernels as the batched device entry points, download, synchronise).  All pointers HOST.
 *   orbhip_search_for_triangulation_host: one pair through the general kernel (nid1 [n1]: vocabulary node of every KF1 feature, -1 =
 *     in no node; KF2's FeatureVector flattened); matches12_out [n1].
 *   orbhip_fuse_search_host: orbhip_fuse_search_device for one keyframe; best_idx_out / best_dist_out [nq].
 *   orbhip_search_by_bow_kf_host: orbhip_search_by_bow_kf_device for one pair; matches12_out [n1].
 *   orbhip_pose_optimization_host: orbhip_pose_optimization_device for one frame; Xw [n][3], obs [n][3], inv_sigma2 [n] doubles,
 *     right [n] or NULL, pose_inout [7], outlier_out [n], *n_inliers_out, stats_out [4] or NULL. */
int orbhip_search_for_triangulation_host(orbhip_ctx *ctx,
        const int32_t *nid1, const uint8_t *has_mp1, const orbhip_keypoint *kp1, const uint8_t *desc1, const float *u_right1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2,
        const uint8_t *has_mp2, const orbhip_keypoint *kp2, const uint8_t *desc2, const float *u_right2, int n2,
        const orbhip_tri_pair_general *pair, const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2,
        int nlevels, int check_orientation, int32_t *matches12_out, int32_t *nmatches_out);
int orbhip_fuse_search_host(orbhip_ctx *ctx, const orbhip_proj_query *q, const uint8_t *desc_q, int nq, const orbhip_keypoint *kp,
                            const uint8_t *desc, const float *u_right, int n, const float *inv_level_sigma2, int nlevels,
                            float min_x, float min_y, float max_x, float max_y, int32_t *best_idx_out, int32_t *best_dist_out);
int orbhip_search_by_bow_kf_host(orbhip_ctx *ctx,
        const int32_t *node_ids1, const int32_t *node_start1, const int32_t *feat1, int nnodes1, const uint8_t *valid1,
        const orbhip_keypoint *kp1, const uint8_t *desc1, int n1,
        const int32_t *node_ids2, const int32_t *node_start2, const int32_t *feat2, int nnodes2, const uint8_t *valid2,
        const orbhip_keypoint *kp2, const uint8_t *desc2, int n2,
        float nn_ratio, int check_orientation, int32_t *matches12_out, int32_t *nmatches_out);

/* Frame::UndistortKeyPoints (src/Frame.cc:738-771), batched: d_kp_un = d_kp with pt replaced by
 * cv::undistortPoints(pt, K, mDistCoef, R = I, P = K) (OpenCV 3.4.1 cvUndistortPoints: 5 fixed-point iterations in double,
 * rounded to float).  dist_coef: HOST array (k1, k2, p1, p2[, k3]), n_dist 4 or 5; k1 == 0 copies (Frame.cc:740-744).
 * d_kp and d_kp_un may be the same buffer.  Other pointers DEVICE. */
int orbhip_undistort_keypoints_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp, const int32_t *d_n, int frames, int max_n,
                                      size_t frame_stride_kp, float fx, float fy, float cx, float cy, const float *dist_coef,
                                      int n_dist, orbhip_keypoint *d_kp_un);

/* Frame::AssignFeaturesToGrid (src/Frame.cc:377-408, Nleft == -1), batched, as a CSR per frame: d_cell_start
 * [frames][64*48+1], d_items [frames][max_n]; cell (ix, iy) = index ix*48+iy holds the keypoint indices
 * d_items[cell_start[c] .. cell_start[c+1]) in insertion (= index) order -- mGrid[ix][iy] of the reference
 * (PosInGrid rounds, Frame.cc:716-726).  At most 8192 keypoints per frame.  All pointers DEVICE. */
int orbhip_assign_features_to_grid_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp, const int32_t *d_n, int frames, int max_n,
                                          size_t frame_stride_kp, float min_x, float min_y, float max_x, float max_y,
                                          int32_t *d_cell_start, int32_t *d_items);

/* Frame::AssignFeaturesToGrid for frames of a two-camera rig (Nleft != -1, src/Frame.cc:395-405): keypoints [0, d_nleft[f]) fill mGrid,
 * the others mGridRight.  d_cell_start [frames][2*64*48+1]: cells 0 .. 3071 = mGrid (cell ix*48+iy), 3072 .. 6143 = mGridRight, one
 * running CSR into d_items [frames][max_n]; mGrid items are keypoint indices, mGridRight items are i - Nleft (:403). */
int orbhip_assign_features_to_grid_rig_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp, const int32_t *d_n, const int32_t *d_nleft,
                                              int frames, int max_n, size_t frame_stride_kp, float min_x, float min_y, float max_x,
                                              float max_y, int32_t *d_cell_start, int32_t *d_items);

/* Second half of Frame::ComputeBoW (src/Frame.cc:729-736): TemplatedVocabulary::transform(features, mBowVec, mFeatVec, 4)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1208, TF_IDF weighting + L1 norm as in ORBvoc) from the per-feature
 * (word id, weight, node id) of orbhip_bow_transform_device, batched over frames:
 *   mFeatVec as the CSR the SearchByBoW / SearchForTriangulation kernels read: d_node_ids [frames][max_nodes] ascending,
 *     d_node_start [frames][max_nodes+1] into d_feat [frames][max_n] (feature indices in feature order), d_nnodes [frames];
 *   mBowVec as d_bow_word / d_bow_value [frames][max_n] (ascending word ids, L1-normalised sums), d_nwords [frames].
 * Features whose word has weight <= 0 ("stopped") are in neither.  std::map order, BowVector::addWeight's accumulation order and
 * BowVector::normalize's summation order (BowVector.cpp) are reproduced, so the values are bit-identical to DBoW2's.
 * max_n <= 4096.  All pointers DEVICE. */
int orbhip_bow_vectors_device(orbhip_ctx *ctx, const int32_t *d_word_id, const double *d_weight, const int32_t *d_node_id,
                              const int32_t *d_n, int frames, int max_n, int max_nodes,
                              int32_t *d_node_ids, int32_t *d_node_start, int32_t *d_feat, int32_t *d_nnodes,
                              int32_t *d_bow_word, double *d_bow_value, int32_t *d_nwords);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:327-403), batched over map points: point p
 * has d_n[p] observing descriptors at d_desc + p*max_n*32 (the loop of :347-361 packs them, left then right index);
 * d_best_idx[p] = BestIdx: the descriptor with the least median Hamming distance to all of them (median = sorted
 * row [int(0.5*(n-1))], first minimum wins).  d_best_desc (may be NULL) receives mDescriptor, [points][32].
 * max_n <= 256.  All pointers DEVICE. */
int orbhip_distinctive_descriptors_device(orbhip_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int points, int max_n,
                                          int32_t *d_best_idx, uint8_t *d_best_desc);

/* The per-feature half of Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:729-736 -> DBoW2
 * TemplatedVocabulary::transform, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1260): for every
 * descriptor the tree descent of :1218-1260 -- at each level the child with the smallest Hamming distance, first minimum
 * wins, until a leaf -- giving its word id, the leaf's weight and the node passed at level L - levelsup (0 = root when
 * that level is <= 0; ORB-SLAM3 uses levelsup = 4).  Building BowVector (addWeight in feature order + L1 normalise,
 * :1165-1210) and FeatureVector from these triples stays on the host (std::map containers).
 * Vocabulary, resident on the device as a flat tree: node i has children d_child_ids[d_child_start[i] ..
 * d_child_start[i+1]) (none = leaf; node 0 = root), 32-byte descriptors d_node_desc[i], d_node_word[i], d_node_weight[i].
 * Frame f reads d_n[f] descriptors at d_desc + f*frame_stride*32; outputs are [frames][max_n].  All pointers DEVICE. */
int orbhip_bow_transform_device(orbhip_ctx *ctx, const uint8_t *d_desc, const int32_t *d_n, int frames, int max_n,
                                size_t frame_stride, const uint8_t *d_node_desc, const int32_t *d_child_start,
                                const int32_t *d_child_ids, const int32_t *d_node_word, const double *d_node_weight,
                                int L, int levelsup, int32_t *d_word_id, double *d_weight, int32_t *d_nid);

/* Frame::ComputeStereoMatches (src/Frame.cc:802-980), batched: rectified-stereo association
 * of the keypoints the LEFT and RIGHT extractor produced in their latest extract call (frame f with frame f;
 * both called with lapping {0,0} as the stereo constructor does, src/Frame.cc:109-110).  Per left keypoint:
 * best right keypoint by descriptor distance among those whose row band (+-2*scale[octave]) covers its row,
 * octave within +-1, disparity in [0, mbf/mb] (:833-887); if better than (TH_HIGH+TH_LOW)/2: 11x11 SAD over
 * +-5 px on the left keypoint's pyramid level (both extractors' device pyramids; columns left of the image
 * are the reflect-101 padding of mvImagePyramid), parabola fit, disparity gates (:890-963); finally matches
 * with SAD >= 1.5*1.4*median are dropped (:966-980).
 * d_u_right / d_depth [batch][max_keypoints] = mvuRight / mvDepth (-1 = no match); d_n_matches [batch] (may be
 * NULL) = matches kept.  The extractors must share image size, levels, scale factor and feature budget and may
 * live on different contexts (the right one's stream is waited for).  Runs on the LEFT context's stream.
 * max_keypoints <= 40956 (else ORBHIP_E_BADARG): the median filter ranks one 4-byte key per keypoint slot in
 * LDS, 160 KB less the kernel's static 16 bytes; above 64 KB (max_keypoints > 16384) the launch is opted in. */
int orbhip_compute_stereo_matches_device(orbhip_extractor *left, orbhip_extractor *right, float mb, float mbf,
                                         float *d_u_right, float *d_depth, int32_t *d_n_matches);

/* One stereo frame, HOST outputs: the call behind Frame::ComputeStereoMatches() of host/Frame.cc (src/Frame.cc:802-980, called by the rectified-stereo
 * constructor at :130).  u_right_out / depth_out [n] = mvuRight / mvDepth of frame 0 of the two extractors' latest extractions (n = the left
 * frame's keypoint count); *n_matches_out (may be NULL) = matches kept.  Synchronous. */
int orbhip_compute_stereo_matches_host(orbhip_extractor *left, orbhip_extractor *right, float mb, float mbf,
                                       float *u_right_out, float *depth_out, int n, int32_t *n_matches_out);

/* Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1128-1168), batched: stereo association of a KannalaBrandt8 rig's two
 * extractions (the stereo-fisheye constructor, :1056-1097).  Frame f: left keypoints d_kpL + f*strideL (d_nL[f] rows, the lapping
 * part from row d_monoL[f] = operator()'s return value), right likewise; descriptors d_descL + f*strideL*32.  Per lapping left row:
 * 2-NN over the right lapping rows (cv::BFMatcher knnMatch k=2, first index wins ties), Lowe's test d0 < d1*0.7 with two neighbours
 * required, KannalaBrandt8::TriangulateMatches(mpCamera2, kpL, kpR, Rlr, tlr, sigma2[kpL.octave], sigma2[kpR.octave]) (camera 1 /
 * camera 2: type 0 Pinhole, 1 KannalaBrandt8, and 8 mvParameters; Rlr row-major 3x3, tlr[3]; level_sigma2[nlevels]: the Frame's,
 * host arrays), kept when depth > 0.0001f.  Outputs [batch][max_n] (x3d [batch][max_n][3]), all DEVICE:
 *   d_l2r[i] = mvLeftToRightMatch (right row or -1), d_depth = mvDepth (-1), d_x3d = mvStereo3Dpoints (left camera; 0 where d_l2r is -1),
 *   d_r2l[j] = mvRightToLeftMatch: the HIGHEST left row that picked j (the reference's loop overwrites), -1 if none;
 *   d_n_matches[f] = matches kept.  mvuRight stays all -1 (:1140).  Counts must be <= max_n <= min(strideL, strideR) (a frame above it
 * keeps the reset values and raises ORBHIP_E_CAPACITY on orbhip_ctx_check_status).  Batch callers take the inputs from
 * orbhip_extractor_results of the two extractors (stride orbhip_extractor_max_keypoints).  Asynchronous on the context's stream. */
int orbhip_compute_stereo_fisheye_matches_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kpL, const uint8_t *d_descL, const int32_t *d_nL, const int32_t *d_monoL, size_t strideL,
        const orbhip_keypoint *d_kpR, const uint8_t *d_descR, const int32_t *d_nR, const int32_t *d_monoR, size_t strideR,
        int batch, int max_n, int cam1_type, const float *cam1, int cam2_type, const float *cam2, const float *Rlr, const float *tlr,
        const float *level_sigma2, int nlevels,
        int32_t *d_l2r, int32_t *d_r2l, float *d_depth, float *d_x3d, int32_t *d_n_matches);

/* One stereo-fisheye frame, HOST outputs: the call behind Frame::ComputeStereoFishEyeMatches() of host/Frame.cc.  Frame 0 of the two
 * extractors' latest host extractions (operator()); n_left / n_right must be their keypoint counts.  l2r_out / depth_out [n_left],
 * x3d_out [n_left][3], r2l_out [n_right], *n_matches_out (may be NULL) as in the batched form.  Runs on the left extractor's context
 * after the right one's stream (the right stream then waits for it); one device-to-host copy; synchronous. */
int orbhip_compute_stereo_fisheye_matches_host(orbhip_extractor *left, orbhip_extractor *right, int cam1_type, const float *cam1,
        int cam2_type, const float *cam2, const float *Rlr, const float *tlr, const float *level_sigma2, int nlevels,
        int32_t *l2r_out, float *depth_out, float *x3d_out, int n_left, int32_t *r2l_out, int n_right, int32_t *n_matches_out);

/* ------------------------------------------------------------------ local BA */
/* One keyframe-window graph in SoA form: what Optimizer::LocalBundleAdjustment builds
 * between src/Optimizer.cc:1850 and :2034.  Poses world->camera as (qx,qy,qz,qw,tx,ty,tz)
 * doubles (g2o::SE3Quat, Thirdparty/g2o/g2o/types/se3quat.h:41); points xyz doubles.
 * Edges are sorted by point (insertion order of Optimizer.cc:1940-2034 == point-major).
 * The struct MUST be zero-initialised before its fields are set (`orbhip_ba_graph g = {0};`, or designated initialisers, which zero
 * the rest): n_cameras, cameras and pose_camera are read whenever n_cameras > 0, and Trl / camera_model / edge_stereo decide which
 * code runs, so a field the caller never wrote must read as 0 / NULL. */
typedef struct {
    int32_t n_poses;            /* free + fixed keyframes */
    int32_t n_points;
    int32_t n_edges;
    const uint8_t *pose_fixed;  /* [n_poses] 1 = fixed (lFixedCameras, Optimizer.cc:1877-1903) */
    const int32_t *edge_pose;   /* [n_edges] */
    const int32_t *edge_point;  /* [n_edges] non-decreasing */
    const double *edge_obs;     /* [n_edges][3]  u,v,(ur; unused for mono) */
    const double *edge_inv_sigma2; /* [n_edges]  mvInvLevelSigma2[octave] */
    const uint8_t *edge_stereo; /* [n_edges] 0 = EdgeSE3ProjectXYZ, 1 = EdgeStereoSE3ProjectXYZ,
                                   2 = EdgeSE3ProjectXYZToBody (observation in the second camera, see Trl below) */
    double fx, fy, cx, cy, bf;  /* intrinsics (Pinhole.cpp:41-47) + stereo baseline*fx */
    int32_t camera_model;       /* 0 = Pinhole; 1 = KannalaBrandt8 for the monocular edges (src/CameraModels/
                                   KannalaBrandt8.cpp:52-69 project, :166-195 projectJac) */
    double kb[4];               /* k1..k4 (mvParameters[4..7]) when camera_model == 1 */
    /* second, rigidly attached camera for the edges of type 2 (pKFi->mpCamera2 / mTrl, src/Optimizer.cc:2001-2032;
     * include/OptimizableTypes.h:112-141, src/OptimizableTypes.cpp:192-213): */
    double Trl[7];              /* mTrl as (qx,qy,qz,qw,tx,ty,tz): left-camera frame -> right-camera frame */
    double fx2, fy2, cx2, cy2;
    int32_t camera2_model;      /* as camera_model */
    double kb2[4];
    /* Per-keyframe calibration (round 4).  The reference hands every edge its OWN keyframe's camera -- e->pCamera = pKFi->mpCamera
     * (src/Optimizer.cc:1961), e->fx ... e->bf = pKFi->fx ... pKFi->mbf (:1990-1994), e->mTrl / e->pCamera2 = pKFi->mTrl / mpCamera2
     * (:2021-2023) -- so a window of an Atlas map built from two cameras mixes calibrations.  n_cameras > 0: pose i projects through
     * cameras[pose_camera[i]] (all nine groups of fields of the entry; the single-calibration fields above are then ignored);
     * n_cameras == 0: every pose uses the fields above (cameras / pose_camera may be NULL). */
    int32_t n_cameras;
    const struct orbhip_ba_camera *cameras;   /* [n_cameras] */
    const int32_t *pose_camera;               /* [n_poses] index into cameras */
} orbhip_ba_graph;
/* one calibration of a BA graph: the same fields, with the same meaning, as the single-calibration part of orbhip_ba_graph */
typedef struct orbhip_ba_camera {
    double fx, fy, cx, cy, bf;
    int32_t camera_model;
    double kb[4];
    double Trl[7];
    double fx2, fy2, cx2, cy2;
    int32_t camera2_model;
    double kb2[4];
} orbhip_ba_camera;

typedef struct {
    int32_t iters1, iters2;     /* optimize(5) then optimize(10): Optimizer.cc:2048,2122 */
    double huber_mono2, huber_stereo2;   /* 5.991, 7.815 (Optimizer.cc:1910-1911) */
    double user_lambda_init;    /* 0 -> tau*max diag (levenberg.cpp:171-185); 100 if inertial */
    double tau;                 /* 1e-50 (levenberg.cpp:47) */
    int32_t max_trials;         /* 100 (levenberg.cpp:51) */
    /* Variant switches for the map-merge local BA, Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF,
     * pbStopFlag) (src/Optimizer.cc:6255-6800) -- all 0 in orbhip_ba_default_params: */
    int32_t stage2_exclude_outliers;  /* after optimize(5): edges with chi2 > gate or depth <= 0 get level 1 and do not
                                         take part in optimize(10) (:6554-6556, :6571-6573) */
    int32_t stage2_drop_robust;       /* after optimize(5): setRobustKernel(0) on every edge (:6560, :6577) */
    int32_t no_discard;               /* no ">= 50 % outliers" bail-out (the merge variant has none) */
    double gate_mono2, gate_stereo2;  /* outlier gates when they differ from the Huber deltas (merge: Huber sqrt(5.99),
                                         gate 5.991, :6395,6554); 0 = use huber_mono2 / huber_stereo2 */
} orbhip_ba_params;

typedef struct {
    int32_t iterations_run[2];  /* outer iterations executed in pass 1 / pass 2 */
    int32_t lm_trials;          /* total inner trials */
    int32_t n_outliers;         /* chi2 > gate or depth <= 0 (Optimizer.cc:2126-2173) */
    int32_t discarded;          /* 1 if >= 50 % outliers (Optimizer.cc:2177-2181): no write-back */
    double chi2_initial, chi2_final;
} orbhip_ba_stats;

void orbhip_ba_default_params(orbhip_ba_params *p);
/* The parameters of the map-merge variant (src/Optimizer.cc:6255): Huber 5.99 / 7.815, gates 5.991 / 7.815, outliers of
 * the first pass excluded and the robust kernel dropped for the second pass, no bail-out. */
void orbhip_ba_merge_params(orbhip_ba_params *p);

/* The numerical core of Optimizer::LocalBundleAdjustment(KeyFrame*, bool* pbStopFlag, Map*, int&)
 *                                            include/Optimizer.h:58, src/Optimizer.cc:1699-2344
 * i.e. initializeOptimization + optimize(5) + initializeOptimization(0) + optimize(10) +
 * outlier classification, on `n_graphs` independent graphs at once.  Host pointers in the
 * graph structs; poses_inout[g] = double[n_poses*7], points_inout[g] = double[n_points*3]
 * (updated in place unless discarded), edge_outlier_out[g] = uint8[n_edges] (may be NULL),
 * abort = LocalMapping::mbAbortBA (polled between iterations and LM trials; may be NULL). */
int orbhip_ba_solve_batch(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs,
                          const orbhip_ba_params *params, volatile const uint8_t *abort,
                          double *const *poses_inout, double *const *points_inout,
                          uint8_t *const *edge_outlier_out, orbhip_ba_stats *stats_out);


/* Parameters of Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:54-330; map initialisation
 * src/Tracking.cc:1603 with 20 iterations, LoopClosing::RunGlobalBundleAdjustment src/LoopClosing.cc:2437 with 10, bRobust = false):
 * the same graph and solver, ONE optimize(iterations) pass, Huber sqrt(5.99) / sqrt(7.815) when robust (else no kernel), no outlier
 * stage and no bail-out.  pose_fixed = (mnId == InitKFid) (:126).  Up to 80 free keyframes the reduced system is built on the FP64
 * matrix cores and factored inside one workgroup; larger windows (to 682 free keyframes) take a global-memory path. */
void orbhip_ba_global_params(orbhip_ba_params *p, int iterations, int robust);

/* Two-phase form of the same solver for callers that keep graphs resident in HBM (bench,
 * map-merge BA): create uploads topology + initial estimates; solve runs both LM passes and
 * the outlier gates entirely on the device (restarting from the initial estimates each call);
 * download copies estimates / outlier flags / stats back. */
typedef struct orbhip_ba_batch orbhip_ba_batch;
/* How BA batches created on this context AFTERWARDS form the Schur complement (a property of the context: two contexts may differ,
 * and orbhip_ba_solve_batch follows its context too): 0 / 1 = from per-block-pair lists, one 16-lane row per pair of free keyframes
 * (default: measured faster at every batch size), 2 = the FP64-MFMA panel GEMM (up to 80 free keyframes; always used by the
 * landmark-sharded mode).  Results agree to rounding (different summation orders); both are parity-tested against the oracle. */
int orbhip_ctx_set_ba_schur_mode(orbhip_ctx *ctx, int mode);
int orbhip_ba_batch_create(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs,
                           double *const *poses, double *const *points, orbhip_ba_batch **out);
int orbhip_ba_batch_solve(orbhip_ba_batch *b, const orbhip_ba_params *params, volatile const uint8_t *abort);
int orbhip_ba_batch_download(orbhip_ba_batch *b, double *const *poses_out, double *const *points_out,
                             uint8_t *const *edge_outlier_out, orbhip_ba_stats *stats_out);
int orbhip_ba_batch_ticks(const orbhip_ba_batch *b);   /* LM trials of the slowest graph, last solve */
void orbhip_ba_batch_destroy(orbhip_ba_batch *b);
/* Landmark-sharded solve of the same graphs by `world` ranks (one process per GPU) -- the optional single-graph mode of the
 * multi-GPU path: g2o iterates landmarks independently (Thirdparty/g2o/g2o/core/block_solver.hpp:381-432), so rank r owns points
 * [r*L/world, (r+1)*L/world) of every graph with their edges, poses are replicated, and the partial sums meet in ONE all-gather
 * per exchange: (1) Hpp, bp, chi2 and max |Hll diag| after buildSystem, (2) the shared Schur block sum_l W D^-1 W^T and W D^-1 b
 * every LM trial, (3) trial chi2, computeScale and the abort flag, (4) outlier / edge counts at the end.  Every rank reduces the
 * gathered slots in rank order, so all ranks solve the same reduced system and take the same LM decisions (deterministic).
 * create_sharded: every rank passes the SAME full graphs and initial estimates.  set_exchange_buffer: a DEVICE buffer of at least
 * world * orbhip_ba_batch_exchange_doubles(b) doubles, laid out [world][exchange_doubles].  solve_sharded: before calling
 * `exchange(user, stage, count)` the library has written `count` doubles into slot `rank` and drained its stream; the callback
 * must all-gather so that slot r of every rank's buffer holds rank r's `count` doubles (RCCL: ncclAllGather(buf + rank*stride,
 * buf, stride, ncclDouble, comm, stream) + stream sync) and return 0.  download writes this rank's points
 * and edge flags at their positions in the caller's full-size arrays (other ranks' entries untouched), all poses, and stats that
 * are identical on every rank.  The abort flag of any rank stops all of them at the same trial. */
typedef int (*orbhip_ba_exchange_fn)(void *user, int stage, size_t count);
int orbhip_ba_batch_create_sharded(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs, double *const *poses,
                                   double *const *points, int rank, int world, orbhip_ba_batch **out);
size_t orbhip_ba_batch_exchange_doubles(const orbhip_ba_batch *b);
int orbhip_ba_batch_set_exchange_buffer(orbhip_ba_batch *b, double *d_buf, size_t capacity_doubles);
int orbhip_ba_batch_solve_sharded(orbhip_ba_batch *b, const orbhip_ba_params *params, volatile const uint8_t *abort,
                                  orbhip_ba_exchange_fn exchange, void *user);
/* Measurement hooks: hipEvent timing of the Schur GEMM launches (on the context's stream), the
 * MFMA flops of the tiles that hold data (flops_per_launch), of everything issued, and a measured FP64 matrix-core peak. */
int orbhip_ba_batch_set_profiling(orbhip_ba_batch *b, int enable);
int orbhip_ba_batch_gemm_profile(const orbhip_ba_batch *b, float *total_ms, int *launches, double *flops_per_launch);
double orbhip_ba_batch_gemm_dense_flops(const orbhip_ba_batch *b);   /* same tiles without block-sparsity skipping */
double orbhip_ba_batch_gemm_issued_flops(const orbhip_ba_batch *b);  /* MFMA flops one launch issues (whole row strips a point touches) */
int orbhip_mfma_f64_peak_tflops(orbhip_ctx *ctx, double *tflops_out);

/* ------------------------------------------------------------------ inertial local BA (LocalInertialBA)
 * The numerical core of Optimizer::LocalInertialBA(KeyFrame*, bool *pbStopFlag, Map*, bool bLarge, bool bRecInit)
 *                                            include/Optimizer.h:98, src/Optimizer.cc:4574-5187
 * i.e. computeActiveErrors + activeRobustChi2, ONE optimize(opt_it) with lambda_init set (:5045-5049; the stop flag is only
 * handed to the optimizer afterwards and has no effect, :5050-5051), the outlier gates (:5056-5088) and the fail check (:5096),
 * on `n_windows` independent windows at once (one workgroup each).  Graph: per keyframe a VertexPose (ImuCamPose: body pose
 * Rwb, twb; the camera pose follows through Tcb) and, when it has IMU states, VertexVelocity / VertexGyroBias / VertexAccBias
 * (include/G2oTypes.h:131-240); EdgeMono / EdgeStereo to the landmarks (src/G2oTypes.cc:349-482), one EdgeInertial + EdgeGyroRW
 * + EdgeAccRW per pair of consecutive keyframes (src/G2oTypes.cc:693-800, include/G2oTypes.h:632-700).  The caller builds the
 * window exactly as :4588-4682 does (temporal keyframes, the fixed previous one, fixed covisible ones) and passes flat arrays.
 * Pinhole and KannalaBrandt8 cameras; keyframes of a two-camera rig (mpCamera2, mTrl) with EdgeMono(1) edges on the right camera.
 * Up to 32 keyframes with IMU states (480 unknowns; the reference caps the window at 10, 25 when bLarge).
 * Deviations from the reference's arithmetic, all far below the 1e-4 parity tolerance: the bias-corrected preintegrated deltas
 * (src/ImuTypes.cc:357-378) and ExpSO3's re-orthonormalisation (src/G2oTypes.cc:991-1008) are evaluated in double instead of
 * float cv::Mat arithmetic; dense LDL^T instead of Eigen::SimplicialLDLT.  Parity is unpinned (no reference vectors exist). */
#define ORBHIP_IBA_KF 21        /* keyframe state: Rwb[9] row-major, twb[3], velocity[3], gyro bias[3], accelerometer bias[3] */
#define ORBHIP_IBA_PREINT 67    /* IMU::Preintegrated: dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], bias bg[3], ba[3] */
typedef struct {
    int32_t n_kf;
    const uint8_t *kf_fixed;        /* setFixed(true): lFixedKeyFrames (:4757-4781) */
    const uint8_t *kf_imu;          /* pKFi->bImu (:4726-4740); keyframes without it have only the pose vertex */
    double Rcb[9], tcb[3];          /* mImuCalib.Tcb */
    double fx, fy, cx, cy, bf;      /* pKF->mpCamera, mbf */
    int32_t camera_model;           /* 0 Pinhole, 1 KannalaBrandt8 */
    double kb[4];
    int32_t has_cam2;               /* pKF->mpCamera2 != NULL: ImuCamPose carries a second camera (src/G2oTypes.cc:57-67) */
    double Trl[12];                 /* pKF->mTrl, 3x4 row-major */
    double fx2, fy2, cx2, cy2;
    int32_t camera2_model;
    double kb2[4];
    int32_t n_points;
    int32_t n_edges;                /* grouped by point: edge_point ascending, as :4914-5034 creates them */
    const int32_t *edge_kf, *edge_point;
    const double *edge_obs;         /* [3]: kpUn.pt.x, kpUn.pt.y, mvuRight */
    const uint8_t *edge_stereo;     /* 0 EdgeMono(0), 1 EdgeStereo(0), 2 EdgeMono(1): right-camera observation (:5000-5031; has_cam2);
                                       a keyframe may hold a left and a right edge to the same point */
    const double *edge_inv_sigma2;  /* mvInvLevelSigma2[octave] / uncertainty2 (:4949-4952) */
    const uint8_t *edge_close;      /* pMP->mTrackDepth < 10 (:5063); may be NULL */
    int32_t n_inertial;
    const int32_t *in_kf1, *in_kf2; /* pKFi->mPrevKF, pKFi (both with IMU states) */
    const double *in_preint;        /* [ORBHIP_IBA_PREINT] */
    const double *in_info;          /* [81] EdgeInertial information (src/G2oTypes.cc:702-714; x 1e-2 on the edge into the fixed keyframe, :4836) */
    const double *in_info_g, *in_info_a;   /* [9] each (:4845-4863) */
    const uint8_t *in_robust;       /* Huber sqrt(16.92) (:4828-4838) */
} orbhip_iba_window;
typedef struct {
    int32_t iterations;             /* 10, or 4 when bLarge */
    double lambda_init;             /* 1.0, or 1e-2 when bLarge */
    int32_t large;                  /* bLarge: no fail check */
    int32_t max_trials;             /* 100 */
} orbhip_iba_params;
typedef struct {
    int32_t iterations_run, lm_trials, n_outliers;
    int32_t failed;                 /* 2*err < err_end or NaN (:5096-5100): the estimates are NOT written back */
    double err, err_end;            /* activeRobustChi2 before / after */
} orbhip_iba_stats;
void orbhip_iba_default_params(orbhip_iba_params *p, int large);
/* Host pointers.  kf_state_inout[w] = double[n_kf * ORBHIP_IBA_KF], points_inout[w] = double[n_points * 3] (updated unless
 * failed), edge_outlier_out[w] = uint8[n_edges] = the observation goes to vToErase (may be NULL), stats_out[n_windows] (may be
 * NULL).  Synchronous. */
int orbhip_inertial_ba_solve_batch(orbhip_ctx *ctx, const orbhip_iba_window *windows, int n_windows, const orbhip_iba_params *params,
                                   double *const *kf_state_inout, double *const *points_inout, uint8_t *const *edge_outlier_out,
                                   orbhip_iba_stats *stats_out);
/* The same, as a RESIDENT batch (the inertial counterpart of orbhip_ba_batch_create): create packs the windows' constant part
 * (topology, observation and preintegration data, the kernels' task lists) and uploads it once into memory the batch owns; a solve
 * uploads only the states (n_kf x 21 + n_points x 3 doubles per window) and launches.  LocalInertialBA is called on a window whose
 * topology the caller rebuilds per call, so the reference path uses the one-shot form; the batch form is for callers that re-solve
 * the same windows (the reference's own second pass with bLarge toggled, relinearisation sweeps, benchmarks) and is what the
 * device-rate figure in bench.py times.  windows' arrays need not outlive create.  set_states replaces the initial states the next
 * solve starts from (create's kf_states/points until then); solve is synchronous and leaves the result on the device; download
 * follows the one-shot call's rules (failed windows are not written).  Not thread-safe per batch; the batch must be destroyed
 * before its context. */
typedef struct orbhip_iba_batch orbhip_iba_batch;
int orbhip_iba_batch_create(orbhip_ctx *ctx, const orbhip_iba_window *windows, int n_windows, double *const *kf_states,
                            double *const *points, orbhip_iba_batch **out);
int orbhip_iba_batch_set_states(orbhip_iba_batch *b, double *const *kf_states, double *const *points);
int orbhip_iba_batch_solve(orbhip_iba_batch *b, const orbhip_iba_params *params);
int orbhip_iba_batch_download(orbhip_iba_batch *b, double *const *kf_states_out, double *const *points_out,
                              uint8_t *const *edge_outlier_out, orbhip_iba_stats *stats_out);
void orbhip_iba_batch_destroy(orbhip_iba_batch *b);
/* Diagnostics: workgroups per window ("team size" G) of the calling thread's latest inertial solve.  Small batches give a window a
 * team of up to 16 workgroups that meet at a device-wide barrier, which needs the whole grid resident: only ONE team grid runs per
 * device at a time (in-process mutex + advisory file lock /tmp/.orbhip_team_gpu<N>.lock); a solve that finds one in flight, and
 * every batch of more than ~128 windows, runs G = 1.  Results for different G agree to rounding (summation order), identical LM
 * decisions in every tested case.  ORBHIP_IBA_TEAM=<n> caps G (tests). */
int orbhip_inertial_ba_last_team_size(void);

/* ------------------------------------------------------------------ full inertial BA
 * Optimizer::FullInertialBA (src/Optimizer.cc:420-851) from "Setup optimizer" to the end of optimize(its), batched over maps
 * (one workgroup each): the graph of a whole map, g2o Levenberg-Marquardt with setUserLambdaInit(1e-5), Huber sqrt(16.92) on
 * EVERY inertial edge, no outlier gates and no fail check: the estimates are always written.
 * An orbhip_iba_window describes a map.  Two modes:
 *   shared_bias = 1 (bInit): ONE gyro-bias and ONE accelerometer-bias vertex for the map (never fixed), shared by every
 *     EdgeInertial, with EdgePriorGyro / EdgePriorAcc on them (error 0 - b, information prior_g I / prior_a I, Jacobian +I as
 *     src/G2oTypes.cc:971-983 writes it, no robust kernel); no EdgeGyroRW / EdgeAccRW.  A free keyframe has 6 unknowns, 9 with
 *     IMU states; the 6 shared unknowns come last.  in_info_g / in_info_a are unread and may be NULL.  The shared estimate
 *     is shared_bias_inout[m] (gyro 3, accelerometer 3): the bias slots of kf_state_inout are NOT read, and on return those
 *     of every keyframe with IMU states -- fixed ones too -- hold the shared result, as :807-823 writes it back.
 *   shared_bias = 0: the 15 / 6 unknowns per keyframe and the EdgeGyroRW / EdgeAccRW of the local window.
 * In both modes edge_close and in_robust are unread (may be NULL).  g2o's activity rule is restated: an edge is active iff one
 * of its vertices is not fixed, so with shared biases an inertial edge between two FIXED keyframes still counts (chi2 and the
 * shared block), without them it does not.  A point whose edges all go to fixed keyframes is constant (bAllFixed, :751-755):
 * not an unknown, nothing in chi2, not written.  A vertex without an active edge is not updated.
 * Capacity: the reduced system is solved by the one-workgroup dense LDL^T, so a map may hold 480 reduced unknowns: 52 free
 * keyframes with IMU states in shared mode (9 x 52 + 6 = 474), 32 without it.  A larger map: ORBHIP_E_CAPACITY, the count in
 * orbhip_last_error(), nothing written.  That covers the three calls of LocalMapping::InitializeIMU and NOT the inertial
 * global BA of a long session.  Always one workgroup per map (no teams).
 * stop (may be NULL) is read ONCE before the launch: set -> ORBHIP_E_ABORTED, nothing written (:758-760).  It is not polled
 * while the kernel runs -- g2o would stop after the current iteration; RunGlobalBundleAdjustment discards a stopped result. */
typedef struct {
    int32_t iterations;             /* its */
    double lambda_init;             /* 1e-5 */
    int32_t max_trials;             /* 100 */
    int32_t shared_bias;            /* bInit */
    double prior_g, prior_a;        /* shared mode */
} orbhip_fiba_params;
#define ORBHIP_FIBA_END_ITERATIONS 0    /* all iterations run */
#define ORBHIP_FIBA_END_TRIALS 1        /* max_trials rejected steps in one iteration, or rho == 0 */
#define ORBHIP_FIBA_END_NBAD 2          /* three iterations in a row that gained less than 1e-3 of chi2 */
typedef struct {
    int32_t iterations_run, lm_trials, end_reason, n_unknowns;
    double chi2_first, chi2_last;   /* activeRobustChi2 of the initial and of the written estimate */
    double lambda;                  /* at the end */
} orbhip_fiba_stats;
void orbhip_fiba_default_params(orbhip_fiba_params *p, int its, int bInit, double priorG, double priorA);
/* Host pointers as in orbhip_inertial_ba_solve_batch; shared_bias_inout = double[n_maps * 6] (shared mode; else may be NULL).
 * A map with n_kf == 0 is skipped (zero stats).  Synchronous. */
int orbhip_full_inertial_ba_solve_batch(orbhip_ctx *ctx, const orbhip_iba_window *maps, int n_maps, const orbhip_fiba_params *params,
                                        const volatile uint8_t *stop, double *const *kf_state_inout, double *const *points_inout,
                                        double *shared_bias_inout, orbhip_fiba_stats *stats_out);

/* ------------------------------------------------------------------ pose-only BA
 * Optimizer::PoseOptimization (src/Optimizer.cc:854-1168), batched over frames: per frame one free
 * VertexSE3Expmap and n unary edges -- EdgeSE3ProjectXYZOnlyPose (include/OptimizableTypes.h:31-57) when
 * uRight < 0, g2o::EdgeStereoSE3ProjectXYZOnlyPose (Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:204-236)
 * otherwise -- solved by the same Levenberg-Marquardt as local BA with a dense 6x6 LDL^T
 * (LinearSolverDense, Thirdparty/g2o/g2o/solvers/linear_solver_dense.h:65-117): 4 rounds x 10 iterations, each
 * from the frame's initial pose, outliers (float chi2 > 5.991f / 7.815f) dropped from the next round and
 * re-tested after it, Huber kernel removed for the last round (:1043-1149).  Called by Tracking after every
 * matcher (src/Tracking.cc:1775,1934,1996-2002).  The fisheye right-camera edge (mpCamera2) is not covered.
 * Frame f reads Xw at d_Xw + f*max_edges*3 (map points, float values widened to double, :913-916),
 * d_obs [f][max_edges][3] = (kpUn.pt.x, kpUn.pt.y, mvuRight), d_inv_sigma2 [f][max_edges]
 * (mvInvLevelSigma2[octave]), d_n_edges [f].  d_pose [f][7] = (qx,qy,qz,qw,tx,ty,tz) of Tcw, in/out
 * (untouched when n < 3, :1040-1041).  d_outlier [f][max_edges] = pFrame->mvbOutlier.  d_n_inliers [f] = the
 * return value nInitialCorrespondences - nBad.  d_stats may be NULL, else [f][4] = rounds, LM iterations,
 * LM trials, nBad.  max_edges <= 8192.  kb8_k: HOST pointer to k1..k4 when pFrame->mpCamera is a KannalaBrandt8
 * (monocular edges then project through src/CameraModels/KannalaBrandt8.cpp:52-69,166-195), NULL = Pinhole.
 * cam2 (HOST pointer, may be NULL) + d_right [f][max_edges] (DEVICE, may be NULL): when pFrame->mpCamera2 exists
 * (:960-1037), d_right[e] = 1 marks an observation made in the second camera -- EdgeSE3ProjectXYZOnlyPoseToBody
 * (include/OptimizableTypes.h:59-87, src/OptimizableTypes.cpp:82-106); such rows carry uRight < 0 (2-D residual,
 * monocular gate).  All other pointers DEVICE; asynchronous on the context's stream. */
/* second camera of a rigid pair for orbhip_pose_optimization_device (pFrame->mpCamera2, pFrame->mTrl) */
typedef struct {
    double Trl[7];              /* mTrl as (qx,qy,qz,qw,tx,ty,tz) */
    double fx, fy, cx, cy;
    int32_t camera_model;       /* 0 Pinhole, 1 KannalaBrandt8 */
    double kb[4];
} orbhip_camera2;
int orbhip_pose_optimization_device(orbhip_ctx *ctx, const double *d_Xw, const double *d_obs,
                                    const double *d_inv_sigma2, const int32_t *d_n_edges, int frames, int max_edges,
                                    double fx, double fy, double cx, double cy, double bf, const double *kb8_k,
                                    const orbhip_camera2 *cam2, const uint8_t *d_right,
                                    double *d_pose, uint8_t *d_outlier, int32_t *d_n_inliers, int32_t *d_stats);
int orbhip_pose_optimization_host(orbhip_ctx *ctx, const double *Xw, const double *obs, const double *inv_sigma2, int n,
                                  double fx, double fy, double cx, double cy, double bf, const double *kb8_k,
                                  const orbhip_camera2 *cam2, const uint8_t *right,
                                  double *pose_inout, uint8_t *outlier_out, int32_t *n_inliers_out, int32_t *stats_out);

/* ------------------------------------------------------------------ inertial pose-only optimisation
 * Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:7479-7872, mode 0; include/Optimizer.h:64) and
 * Optimizer::PoseInertialOptimizationLastFrame (:7874-8299, mode 1; include/Optimizer.h:65), batched over frames; Tracking calls
 * them instead of PoseOptimization once the IMU is initialised (src/Tracking.cc:1995-2017).  Per frame: VertexPose / Velocity /
 * GyroBias / AccBias of the frame (src/G2oTypes.cc:73-118, :664-692), unary EdgeMonoOnlyPose / EdgeStereoOnlyPose edges in
 * frame-index order (:7535-7639), EdgeInertial + EdgeGyroRW + EdgeAccRW to the previous state -- the last keyframe, fixed (mode 0),
 * or the previous frame, free and held by EdgePriorPoseImu with Huber 5 (mode 1, src/G2oTypes.cc:929-969) -- solved by g2o
 * Gauss-Newton with a dense LDL^T, 4 rounds x 10 iterations, the outlier classification after each round, the recovery when
 * nInliers < 30 && !bRecInit, the new prior's Hessian (Marginalize, :5187-5267, in mode 1) cleaned as ConstraintPoseImu's
 * constructor does (include/G2oTypes.h:708-719).  tests/pose_inertial_model.py pins the arithmetic.  Deviations: the LDL^T does not
 * pivot (a pivot <= 0 or not finite is the "not positive" factorisation that stops a round); the camera poses of the first
 * iteration are computed from Rwb / twb rather than read from mTcw (they agree to the frame's float rounding).
 * Frame f reads its edges at [f][max_edges]: d_Xw [3] (map point, float widened), d_obs [3] = (kp.x, kp.y, mvuRight), d_inv_sigma2
 * (mvInvLevelSigma2[octave] / uncertainty2), d_kind (0 left mono -- mvKeysUn, or mvKeys on a rig; 1 stereo; 2 right mono, mvKeysRight),
 * d_close (mTrackDepth < 10; may be NULL), d_n_edges [f].  Kind 2 requires rig->has_cam2 (the device form does not check it; the
 * host form returns ORBHIP_E_BADARG).  d_prev [f][ORBHIP_IBA_KF]: mpLastKeyFrame (mode 0) or mpPrevFrame (mode 1;
 * never written back), d_preint [f][ORBHIP_IBA_PREINT] (mpImuPreintegrated, mode 0 / mpImuPreintegratedFrame, mode 1), d_info [f][81]
 * (EdgeInertial's information), d_info_g / d_info_a [f][9] (C(9:12,9:12)^-1, C(12:15,12:15)^-1), d_prior [f][ORBHIP_IBA_KF + 225]
 * (mode 1: pFp->mpcpi as Rwb twb vwb bg ba + H [15][15]; NULL in mode 0).  d_state [f][ORBHIP_IBA_KF] in/out.  Outputs: d_outlier
 * [f][max_edges] = mvbOutlier, d_ret [f] = nInitialCorrespondences - nBad, d_H_out [f][225] = the new mpcpi's H after
 * ConstraintPoseImu (feed it to the next frame's d_prior), d_stats [f][4] or NULL = rounds run, GN iterations, failed
 * factorisations, nBad.  All pointers DEVICE; asynchronous on the context's stream. */
typedef struct {
    double Rcb[9], tcb[3];          /* mImuCalib.Tcb */
    double fx, fy, cx, cy, bf;      /* mpCamera, mbf */
    int32_t camera_model;           /* 0 Pinhole, 1 KannalaBrandt8 */
    double kb[4];
    int32_t has_cam2;               /* mpCamera2 (right-camera edges, kind 2) */
    double Trl[12];                 /* mTrl, 3x4 row-major */
    double fx2, fy2, cx2, cy2;
    int32_t camera2_model;
    double kb2[4];
} orbhip_pim_rig;
int orbhip_pose_inertial_optimization_device(orbhip_ctx *ctx, int mode, int rec_init, const orbhip_pim_rig *rig, int frames,
        int max_edges, const double *d_Xw, const double *d_obs, const double *d_inv_sigma2, const uint8_t *d_kind, const uint8_t *d_close,
        const int32_t *d_n_edges, const double *d_prev, const double *d_preint, const double *d_info, const double *d_info_g,
        const double *d_info_a, const double *d_prior, double *d_state, uint8_t *d_outlier, int32_t *d_ret, double *d_H_out,
        int32_t *d_stats);
/* the same for ONE frame of n edges, HOST pointers (one page-locked blob up, one down; synchronous); prior NULL in mode 0,
 * stats_out [4] may be NULL */
int orbhip_pose_inertial_optimization_host(orbhip_ctx *ctx, int mode, int rec_init, const orbhip_pim_rig *rig, int n,
        const double *Xw, const double *obs, const double *inv_sigma2, const uint8_t *kind, const uint8_t *close,
        const double *prev, const double *preint, const double *info, const double *info_g, const double *info_a,
        const double *prior, double *state_inout, uint8_t *outlier_out, int32_t *ret_out, double *H_out, int32_t *stats_out);

/* ------------------------------------------------------------------ inertial initialisation (IMU init, scale refinement, inertial merge)
 * Optimizer::InertialOptimization, the four overloads of include/Optimizer.h:115-118 (src/Optimizer.cc:5303-5481 (a), :5484-5644 (b),
 * :5646-5806 (c), :5808-5908 (d)), batched over maps: one workgroup solves one map.  Per map: the keyframes in chain order with fixed
 * poses, one EdgeInertialGS (src/G2oTypes.cc:802-927) per keyframe that has a link to its predecessor, ONE gyro and ONE accelerometer
 * bias (EdgePriorGyro / EdgePriorAcc to zero with information prior_g I / prior_a I, Jacobian +I as src/G2oTypes.cc:971-983 sets it),
 * VertexGDir (Rwg <- Rwg ExpSO3(d0, d1, 0)) and VertexScale (s <- s exp(d)), include/G2oTypes.h:254-314.  No robust kernel.  g2o's
 * Levenberg-Marquardt as the fork has it (tau 1e-50, rho = dchi2 / (scale + 1e-3), up to max_trials trials per iteration, Terminate on
 * rho == 0, on max_trials failed trials or after three iterations in a row that each gained less than 1e-3 of their chi2) or, for (d),
 * Gauss-Newton.  The system is solved as an arrowhead: block elimination along the velocity chain, the border's Schur complement
 * (at most 9 x 9), back substitution; a fixed unknown is absent from it.  A block pivot that is not positive or not finite is "solver
 * failed": LM counts a failed trial, GN applies the last successful step once more (as g2o does) and stops.  Deviations from the
 * reference's arithmetic: the bias-corrected deltas are evaluated in double (as in the inertial BA above); the information is read as
 * its upper triangle.  tests/inertial_opt_model.py pins the arithmetic.
 * d_kf_off [maps + 1]: keyframe rows of map m are [d_kf_off[m], d_kf_off[m + 1]), at most 4096.  d_kf [K][ORBHIP_IBA_KF]: Rwb, twb,
 * velocity, biases.  d_link [K]: 1 = an edge joins keyframes k - 1 and k, its preintegration (d_preint [K][ORBHIP_IBA_PREINT]) and
 * information (d_info [K][81]) stored at k; the first keyframe of a map has 0, a 0 further on is a gap.  d_global [maps]
 * [ORBHIP_IO_GLOBAL]: Rwg, scale and the map's bias (the class fills it from vpKFs.front()), in/out; fixed quantities come back
 * bit-identical.  With fixed biases the two prior edges
 * have only fixed vertices and, as in g2o, add nothing to chi2.  When free_vel_bias is set every keyframe gets its velocity at [12:15] and the solved bias at [15:21] (SetNewBias),
 * otherwise d_kf is not written.  d_stats [maps][8] or NULL: iterations run, LM trials, end reason (0 ran out of iterations, 1 Terminate,
 * 2 solver failed, 3 chi2 or lambda not finite: the map keeps its last accepted state), first chi2, last chi2, final lambda, edges, 0
 * (with ORBHIP_IO_PROF=1 in the environment the last two are cycle shares instead: border solve + back substitution, chain elimination).
 * d_trace [maps][iterations][2] or NULL: chi2 and lambda after each LM iteration run (GN: chi2 at the iteration's start, 0); rows of
 * iterations not run are untouched.  The offsets are read back once (a synchronisation); the solve is asynchronous on the context's
 * stream and uses the context's work arena.  ORBHIP_E_BADARG: nothing free, maps < 0, offsets that decrease, a map of more than 4096
 * keyframes; maps == 0 succeeds and launches nothing.  Maps of up to ORBHIP_IO_LDS_KEYFRAMES keyframes keep their chain in LDS, longer
 * ones in the work arena. */
#define ORBHIP_IO_GLOBAL 16             /* Rwg[9] row-major, scale, bg[3], ba[3] */
#define ORBHIP_IO_LDS_KEYFRAMES 256     /* orbhip_inertial_opt_lds_keyframes() returns it */
typedef struct {
    int32_t free_vel_bias;              /* !bFixedVel; 0 in (d) */
    int32_t free_gdir, free_scale;
    int32_t gauss_newton;               /* (d) */
    int32_t iterations;                 /* 200; 10 in (d) */
    int32_t max_trials;                 /* 100 */
    double lambda_init;                 /* 1e3; 0 = g2o's own (tau * max diagonal) */
    double prior_g, prior_a;            /* 0 = the edge carries no information */
} orbhip_inertial_opt_params;
/* overload 0..3 = (a)..(d); mono / fixed_vel / priorG / priorA as the reference's arguments ((a): lambda_init 1e3 only when priorG != 0) */
void orbhip_inertial_opt_default_params(orbhip_inertial_opt_params *p, int overload, int mono, int fixed_vel, float priorG, float priorA);
int orbhip_inertial_opt_lds_keyframes(void);
int orbhip_inertial_optimization_device(orbhip_ctx *ctx, const orbhip_inertial_opt_params *p, int maps, const int32_t *d_kf_off,
        double *d_kf, const uint8_t *d_link, const double *d_preint, const double *d_info, double *d_global, double *d_stats,
        double *d_trace);
/* the same for ONE map of n_kf keyframes, HOST pointers (one page-locked blob up, one down; synchronous); stats_out [8] and trace_out
 * [iterations][2] may be NULL */
int orbhip_inertial_optimization_host(orbhip_ctx *ctx, const orbhip_inertial_opt_params *p, int n_kf, double *kf_inout,
        const uint8_t *link, const double *preint, const double *info, double *global_inout, double *stats_out, double *trace_out);

/* ------------------------------------------------------------------ IMU preintegration
 * IMU::Preintegrated::Initialize / IntegrateNewMeasurement (src/ImuTypes.cc:225-310, with IntegratedRotation :153-178 and
 * NormalizeRotation :30-36), batched over independent chains: what Reintegrate (:246-253), MergePrevious (:312-336) and
 * Tracking::PreintegrateIMU (src/Tracking.cc:552-666) run.  A chain is one preintegration: a bias and a list of measurements
 * (ax, ay, az, wx, wy, wz, dt), 7 floats each.  Float arithmetic throughout in the reference's update order (csrc/preint_core.h;
 * NormalizeRotation is two Newton steps of the polar iteration, sums are accumulated in float where OpenCV's gemm accumulates in
 * double; tests/preint_model.py pins the arithmetic).
 * d_meas_off [chains + 1]: the measurements of chain c are rows [d_meas_off[c], d_meas_off[c + 1]) of d_meas [total][7]; an empty
 * chain is allowed.  d_continue [chains] or NULL: 0 = the chain starts fresh (Initialize), 1 = it continues from the record, covariance
 * and averages already in the output arrays (Tracking appends each frame's measurements to mpImuPreintegratedFromLastKF); continuing
 * equals integrating the concatenated list in one go, byte for byte, within one form.  d_record [chains][ORBHIP_IBA_PREINT], in/out:
 * bg / ba at [61:67] are always read (the chain's bias) and never written, the rest is written, and read only by a continuing chain;
 * the doubles hold float values.  d_cov [chains][225]: the 15 x 15 float covariance C, row-major (C(0:9, 0:9) symmetric up to
 * rounding, as the reference's is; the blocks between it and the walk block are written as zeros).  d_avg [chains][6]: avgA, avgW.
 * A fresh chain of length 0 yields Initialize's values.  Non-finite measurements are no error: they propagate as IEEE arithmetic does,
 * inside their own chain.
 * want_info: d_info [chains][81], d_info_g [chains][9], d_info_a [chains][9] in double from the covariance just written -- the EdgeInertial
 * information as the host classes compute it (symmetrise, cyclic Jacobi, eigenvalues <= 9e-7 * the largest dropped, inverses below 1e-12
 * clamped, reassembled) and the 3 x 3 inverses of C(9:12, 9:12) and C(12:15, 12:15) rounded through float: the d_info / d_info_g /
 * d_info_a arguments of the inertial optimisers above, without a host visit.  With want_info == 0 the three may be NULL.
 * Two forms, chosen by the number of chains: fewer than ORBHIP_PREINT_WAVE_MAX_CHAINS run one wave per chain, more run one lane per chain
 * (csrc/preint_kernels.hip); force_form runs one of them at any size.  Asynchronous on the context's stream but for one read-back of
 * the offsets, which are checked first.  ORBHIP_E_BADARG (nothing written): chains < 0, an unknown force_form, a required array NULL,
 * d_meas_off[0] < 0 or offsets that decrease; chains == 0 succeeds and launches nothing. */
#define ORBHIP_PREINT_FORM_AUTO 0
#define ORBHIP_PREINT_FORM_LANE 1
#define ORBHIP_PREINT_FORM_WAVE 2
#define ORBHIP_PREINT_WAVE_MAX_CHAINS 4096  /* the measured crossing at 100 measurements per chain; orbhip_preint_wave_max_chains() returns it */
typedef struct {
    float nga[36];                      /* IMU::Calib::Cov: 6 x 6 row-major, gyro then accelerometer; symmetric */
    float nga_walk[36];                 /* IMU::Calib::CovWalk */
    int32_t force_form;                 /* ORBHIP_PREINT_FORM_* */
    int32_t want_info;
} orbhip_preint_params;
/* diag(ng^2 x 3, na^2 x 3) and diag(ngw^2 x 3, naw^2 x 3) as IMU::Calib::Set makes them (src/ImuTypes.cc:486-510), automatic form, want_info = 1 */
void orbhip_preint_default_params(orbhip_preint_params *p, float ng, float na, float ngw, float naw);
int orbhip_preint_wave_max_chains(void);
int orbhip_preintegrate_device(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *d_meas_off,
        const float *d_meas, const uint8_t *d_continue, double *d_record, float *d_cov, float *d_avg, double *d_info, double *d_info_g,
        double *d_info_a);
/* the same with HOST pointers (one page-locked blob up, one down; synchronous); cont may be NULL, the info arrays when want_info == 0 */
int orbhip_preintegrate_host(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *meas_off, const float *meas,
        const uint8_t *cont, double *record_inout, float *cov_inout, float *avg_inout, double *info_out, double *info_g_out,
        double *info_a_out);

/* ------------------------------------------------------------------ two-view reconstruction (monocular initialisation)
 * TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated)
 * (include/TwoViewReconstruction.h:36-41, src/TwoViewReconstruction.cc:39-933), batched over frame pairs -- the one consumer of
 * SearchForInitialization's vnMatches12 (mpCamera->ReconstructWithTwoViews, src/Tracking.cc:1522).  Per pair: the matches in index
 * order (:53-62), `iterations` RANSAC sets of 8 matches (:81-96), FindHomography / FindFundamental on them (Normalize over ALL
 * keypoints of each frame, ComputeH21 / ComputeF21, CheckHomography / CheckFundamental in float in the reference's operation order,
 * strictly-greater argmax: the lowest iteration among equal scores, a score of 0 never wins), RH = SH / (SH + SF) > rh_threshold ->
 * ReconstructH else ReconstructF with the reference's decision rules (:475-736), CheckRT / Triangulate for the 4 or 8 motion hypotheses.
 * The decompositions (9x9, 3x3, 4x4) are Jacobi iterations in double / float: OpenCV's SVD bits are not reproduced (for ComputeF21 they
 * cannot be: FULL_UV completes vt from a random generator), so results agree with the reference within rounding, not bit for bit, and
 * the numbering of the motion hypotheses follows this library's singular-vector signs (the set of hypotheses does not depend on them).
 * d_kp1 / d_n1 / d_kp2 / d_n2 / frame_stride_kp / d_matches12 [pairs][max_n]: exactly what orbhip_extractor_results and
 * orbhip_search_for_initialization_device leave on the device (an entry >= n2 counts as unmatched).  fx, fy, cx, cy: mK.
 * d_sets [pairs][iterations][8] (indices into the pair's match list): with draw_sets != 0 the library draws them on the device --
 * per iteration a partial Fisher-Yates over 0..N-1, 8 draws, swap-with-last as :81-96, from a counter-based generator keyed by
 * (seed, pair, iteration, draw) -- and writes them there (-1 for a pair with fewer than 8 matches); with draw_sets == 0 the caller
 * supplies them (a set with an index outside [0, N) scores 0).  Outputs: d_ok [pairs] (the return value), d_R21 [pairs][9] row-major,
 * d_t21 [pairs][3] (unit length), d_P3D [pairs][max_n][3] and d_triangulated [pairs][max_n] indexed by the FIRST keypoint index; rows
 * [0, n1) are written, on failure with the reset values (all zero) -- also for a pair with fewer than 8 matches, which the reference
 * never sees (src/Tracking.cc:1510).  d_stats, d_hyp_scores [pairs][iterations][2] (H, F) and d_hyp_mats [pairs][iterations][2][9]
 * (H21_i, F21_i) are optional (NULL).  max_n <= 8192 and iterations <= 1024, else ORBHIP_E_CAPACITY; n1 / n2 > max_n sets the
 * context's status word.  All pointers DEVICE; asynchronous on the context's stream. */
typedef struct orbhip_tvr_params {
    float sigma; int32_t iterations;                /* 1.0, 200   (include/TwoViewReconstruction.h:36) */
    float rh_threshold;                             /* 0.50       (src/TwoViewReconstruction.cc:117) */
    float min_parallax; int32_t min_triangulated;   /* 1.0, 50    (:114, :120) */
    int32_t draw_sets; uint64_t seed;
} orbhip_tvr_params;
typedef struct orbhip_tvr_stats {
    int32_t n_matches;              /* N */
    float score_h, score_f;         /* SH, SF */
    int32_t iter_h, iter_f;         /* winning iterations, -1 = no hypothesis scored above 0 */
    int32_t model;                  /* 0 none, 1 ReconstructH, 2 ReconstructF */
    int32_t n_inliers;              /* inliers of the model taken */
    int32_t n_hyp;                  /* motion hypotheses checked: 0, 4 or 8 */
    int32_t n_good[8];              /* nGood of each */
    int32_t hyp_index;              /* the hypothesis whose parallax decided, -1 = none */
    float parallax;                 /* its parallax in degrees */
} orbhip_tvr_stats;
void orbhip_tvr_default_params(orbhip_tvr_params *p);
int orbhip_two_view_reconstruct_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp1, const int32_t *d_n1, const orbhip_keypoint *d_kp2,
        const int32_t *d_n2, size_t frame_stride_kp, const int32_t *d_matches12, int pairs, int max_n, float fx, float fy, float cx, float cy,
        const orbhip_tvr_params *p, int32_t *d_sets, uint8_t *d_ok, float *d_R21, float *d_t21, float *d_P3D, uint8_t *d_triangulated,
        orbhip_tvr_stats *d_stats, float *d_hyp_scores, float *d_hyp_mats);
/* the same for ONE pair, HOST pointers (one page-locked blob up, one down; synchronous): kp1 [n1], kp2 [n2], matches12 [n1],
 * sets [iterations][8] in (draw_sets == 0) or out, P3D_out [n1][3], triangulated_out [n1]; stats_out may be NULL.  What
 * host/TwoViewReconstruction.cc calls. */
int orbhip_two_view_reconstruct_host(orbhip_ctx *ctx, const orbhip_keypoint *kp1, int n1, const orbhip_keypoint *kp2, int n2,
        const int32_t *matches12, float fx, float fy, float cx, float cy, const orbhip_tvr_params *p, int32_t *sets,
        uint8_t *ok_out, float *R21_out, float *t21_out, float *P3D_out, uint8_t *triangulated_out, orbhip_tvr_stats *stats_out);

/* ------------------------------------------------------------------ Sim3 refinement between two keyframes (loop closing / map merging)
 * Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (include/Optimizer.h:90,
 * src/Optimizer.cc:3932-4328), batched over keyframe pairs: what LoopClosing runs between its device matchers
 * (src/LoopClosing.cc:532, :742).  Per pair: one free VertexSim3Expmap (7 unknowns omega, upsilon, sigma; oplus = Sim3(update) *
 * estimate with g2o::Sim3(Vector7d)'s four branches; update[6] = 0 under fix_scale) and, per correspondence, the edge pair
 * EdgeSim3ProjectXYZ (obs1 - cam1.project(S12.map(P2c))) / EdgeInverseSim3ProjectXYZ (obs2 - cam2.project(S12^-1.map(P1c))) with
 * information inv_sigma2 * I and Huber delta (float)sqrt(th2); g2o Levenberg-Marquardt with a dense LDL^T exactly as
 * orbhip_pose_optimization_device runs it; optimize(5) with Huber, pairs dropped on the STORED chi2 of the last LM trial (either
 * edge > th2), the `nCorrespondences - nBad < 10` return of 0, optimize(nBad > 0 ? 10 : 5) without kernels, fresh errors, nIn.
 * Deviations: the Jacobians are analytic (the reference differentiates numerically with a step of 1e-9), the LDL^T does not pivot.
 * Pair p reads its correspondences at [p][max_edges]: d_P1c / d_P2c [3] = R1w * X1 + t1w / R2w * X2 + t2w (float products widened),
 * d_obs1 [2] = mvKeysUn[i].pt of KF1, d_obs2 [2] = mvKeysUn[i2].pt of KF2 or, for a point without keypoint in KF2, the NORMALISED
 * (x/z, y/z) of P2c in float (src/Optimizer.cc:4161-4181, kept), d_inv_sigma2_1 / _2 = mvInvLevelSigma2[octave] (octave 0 in
 * that case: :4178 passes mnTrackScaleLevel to cv::KeyPoint as the SIZE, the octave keeps its default), d_n [p].  The caller applies the map-point tests of :4025-4080; the `P3D2c.z < 0` test (:4082) runs on the device.
 * d_sim3 [p][8] = (qx qy qz qw tx ty tz s) of g2oS12, in/out: untouched when the call answers 0 by the `< 10` rule.
 * d_flag [p][max_edges]: 0 inlier, 1 dropped after pass 1, 2 dropped after pass 2, 3 no edge (P2c.z < 0); rows at index n and above
 * are untouched.  d_n_in [p] = the return value.  d_stats NULL or [p][4] = nCorrespondences, nBad, LM iterations, LM trials.
 * max_edges <= 8192, else ORBHIP_E_CAPACITY; a pair with n > max_edges or n < 0 sets the context's status word and writes nothing but
 * its d_n_in / d_stats entries (0).  cam1 / cam2 are HOST pointers, all others DEVICE; asynchronous on the context's stream. */
typedef struct orbhip_sim3_camera { double fx, fy, cx, cy; int32_t camera_model; double kb[4]; } orbhip_sim3_camera;
int orbhip_optimize_sim3_device(orbhip_ctx *ctx, const double *d_P1c, const double *d_P2c, const double *d_obs1, const double *d_obs2,
        const double *d_inv_sigma2_1, const double *d_inv_sigma2_2, const int32_t *d_n, int pairs, int max_edges,
        const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2, double th2, int fix_scale,
        double *d_sim3, uint8_t *d_flag, int32_t *d_n_in, int32_t *d_stats);
/* the same for ONE pair of n correspondences, HOST pointers (one page-locked blob up, one down; synchronous); stats_out [4] may be
 * NULL.  What host/Optimizer_OptimizeSim3.cc calls. */
int orbhip_optimize_sim3_host(orbhip_ctx *ctx, const double *P1c, const double *P2c, const double *obs1, const double *obs2,
        const double *inv_sigma2_1, const double *inv_sigma2_2, int n, const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2,
        double th2, int fix_scale, double *sim3_inout, uint8_t *flag_out, int32_t *n_in_out, int32_t *stats_out);

/* ------------------------------------------------------------------ Sim3 between two keyframes from 3-point sets (loop candidates)
 * Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc:35-506), batched over candidates: what LoopClosing::DetectCommonRegionsFromBoW
 * runs between SearchByBoW and SearchByProjection / OptimizeSim3 (src/LoopClosing.cc:673-684).  Per pair: the iteration budget of
 * SetRansacParameters (epsilon = (float)min_inliers / n; 1 when min_inliers == n, else ceil(log(1 - p) / log(1 - epsilon^3)) in double,
 * clamped to [1, max_iterations]; where the reference converts a quotient beyond INT_MAX to int unchecked, this saturates to
 * max_iterations); per iteration a set of 3 correspondences, ComputeSim3 on it (Horn: centroids, M, the 4x4 N, the eigenvector of its
 * largest eigenvalue by a cyclic Jacobi iteration in double, angle-axis, Rodrigues, scale or 1 under fix_scale, t12, T12, T21 -- double
 * arithmetic on the float inputs, each of T12 / T21 / R12 / t12 / s12 rounded once to float; NOT cv::eigen / cv::Rodrigues on floats) and
 * CheckInliers (both reprojections as the float small-matrix gemm then GeometricCamera::project, no z test, in the reference's
 * operation order; err1 < max1 && err2 < max2); a hypothesis with a NaN entry counts 0.  Then iterate()'s rule over the counts of
 * iterations 0 .. budget-1: the first iteration whose count is > min_inliers converges; without one the best is the LAST arg-max (the
 * reference's >= update starting from 0).  Running the reference in chunks (iterate(20, ...)) is this same scan.
 * Pair p reads its correspondences at [p][max_n]: d_X1c / d_X2c [3] float = Rcw * Xw + tcw of the two map points in their keyframes
 * (mvX3Dc1 / mvX3Dc2), d_max_err1 / d_max_err2 = the thresholds ALREADY TRUNCATED as the reference's std::vector<size_t> does
 * ((float)(size_t)(9.210 * sigma2): 9, 13, 19, ...), d_n [p].  The image points mvP1im1 / mvP2im2 are projected on the device.
 * d_sets [pairs][max_iterations][3] (indices into the pair's correspondences): with draw_sets != 0 the library draws them on the
 * device -- per iteration a partial Fisher-Yates over 0..n-1, 3 draws, the drawn slot refilled with the last one as :178-189, from the
 * counter-based generator of the two-view reconstruction keyed by (seed, pair, iteration, draw) -- and writes them there (-1 for a
 * pair with n < 3); with draw_sets == 0 the caller supplies them (a set with an index outside [0, n) is a NaN hypothesis: count 0).
 * Outputs per pair: d_converged (u8), d_R12 [9] row-major / d_t12 [3] / d_s12 (mBestRotation / mBestTranslation / mBestScale),
 * d_n_inliers, d_inlier [pairs][max_n] u8 (rows [0, n) are written: the winner's flags on convergence, else zero as vbInliers stays;
 * rows at n and above are untouched).  A pair that does not converge still reports the last arg-max hypothesis in R12 / t12 / s12 and
 * the stats, with n_inliers 0.  A pair with n < min_inliers (bNoMore at once): converged 0, n_inliers 0, R12 / t12 / s12 untouched,
 * budget 0.  d_stats NULL or [pairs][3] = iteration budget, winning iteration (-1 none), its count.  d_counts NULL or
 * [pairs][max_iterations] = inliers of every iteration (-1 beyond the budget).  max_n <= 8192 and max_iterations <= 1024, else
 * ORBHIP_E_CAPACITY; min_inliers < 1, max_iterations < 1 or probability outside (0, 1): ORBHIP_E_BADARG with the field named by
 * orbhip_last_error(); a pair with n > max_n or n < 0 sets the context's status word and writes nothing but converged = 0,
 * n_inliers = 0 and its d_stats entry (0, -1, 0).  cam1 / cam2 / p are HOST pointers (the camera parameters are narrowed to float, the
 * reference's mvParameters), all others DEVICE; asynchronous on the context's stream. */
typedef struct orbhip_sim3solver_params {
    double probability;                             /* 0.99       (include/Sim3Solver.h:40) */
    int32_t min_inliers, max_iterations;            /* 6, 300 */
    int32_t fix_scale, draw_sets; uint64_t seed;    /* 0, 1, 0 */
} orbhip_sim3solver_params;
void orbhip_sim3solver_default_params(orbhip_sim3solver_params *p);
int orbhip_sim3_solver_device(orbhip_ctx *ctx, const float *d_X1c, const float *d_X2c, const float *d_max_err1, const float *d_max_err2,
        const int32_t *d_n, int pairs, int max_n, const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2,
        const orbhip_sim3solver_params *p, int32_t *d_sets, uint8_t *d_converged, float *d_R12, float *d_t12, float *d_s12,
        int32_t *d_n_inliers, uint8_t *d_inlier, int32_t *d_stats, int32_t *d_counts);
/* the same for ONE pair of n correspondences, HOST pointers (one page-locked blob up, one down; synchronous): sets
 * [max_iterations][3] in (draw_sets == 0) or out, inlier_out [n]; stats_out [3] and counts_out [max_iterations] may be NULL.  What
 * host/Sim3Solver.cc calls. */
int orbhip_sim3_solver_host(orbhip_ctx *ctx, const float *X1c, const float *X2c, const float *max_err1, const float *max_err2, int n,
        const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2, const orbhip_sim3solver_params *p, int32_t *sets,
        uint8_t *converged_out, float *R12_out, float *t12_out, float *s12_out, int32_t *n_inliers_out, uint8_t *inlier_out,
        int32_t *stats_out, int32_t *counts_out);

/* ------------------------------------------------------------------ camera pose from 6-point sets (relocalisation candidates)
 * MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp:54-1010), batched over candidates: what Tracking::Relocalization runs between
 * SearchByBoW and PoseOptimization / SearchByProjection (src/Tracking.cc:2644-2760).  Per candidate: SetRansacParameters (:218-253) --
 * nMin = max((int)(n * epsilon), min_inliers, min_set), epsilon = max(epsilon, (float)nMin / n), the budget 1 when nMin == n, else
 * ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) (exponent 3, as written) clamped to [1, max_iterations] (a quotient beyond
 * INT_MAX saturates to max_iterations), max_err = sigma2 * th2 in float; per iteration a set of 6 matches, computePose on it (:345-651:
 * null spaces, the planar test as FullPivHouseholderQR::rank() == 2, the 12- or 9-column design matrix, the eigenvector of the smallest
 * eigenvalue of A^T A by a cyclic Jacobi iteration, scale and nearest rotation, the disambiguation on the first 6 points, at most 5
 * Gauss-Newton steps with the three exits of :738-746; double arithmetic on the float inputs, without the covariance branch) and
 * CheckInliers (:255-286: the camera point as double sums rounded to float, GeometricCamera::project in float, no z test,
 * error2 < max_err); a hypothesis with a NaN entry counts 0, and so does a set with an index outside [0, n) or with an index twice.
 * Then iterate()'s loop (:113-213) over the counts of iterations 0 .. E-1, E = max(budget, first_call_iterations) capped at
 * max_iterations: an iteration with count >= nMin and above every earlier count is a new best, and Refine() (:288-342) is called on every
 * iteration with count >= nMin.  AS WRITTEN, Refine() runs computePose on the best's inliers into a local `result` (:317-321) that is
 * never copied into mRi / mti (assigned only at :150-162), so its CheckInliers() (:324) scores the CURRENT iteration's hypothesis again
 * and mRefinedTcw (:331-337) is that hypothesis: the call returns at the first iteration k >= resume_at with count[k] > nMin, strictly
 * (outcome 1: hypothesis k rounded to float, its count and its flags); without one the best hypothesis is reported when some count
 * reached nMin (outcome 2, bNoMore), else nothing (outcome 0).  The library follows that text and does not run the N-point solve, whose
 * result nothing reads.
 * Candidate c reads its matches at [c][max_n]: d_Xw [3] float = MapPoint::GetWorldPos(), d_p2d [2] float = mvKeysUn[i].pt, d_sigma2 =
 * mvLevelSigma2[octave], d_n [c].  The bearings (unproject(pt) / z, :77-78) are computed on the device.
 * d_sets [candidates][max_iterations][6] (indices into the candidate's matches): with draw_sets != 0 the library draws them on the
 * device -- per iteration a partial Fisher-Yates over 0..n-1, 6 draws, the drawn slot refilled with the last one as :126-138, from the
 * counter-based generator of the two-view reconstruction keyed by (seed, candidate, iteration, draw) -- and writes them there (-1 for a
 * candidate with n < 6); with draw_sets == 0 the caller supplies them.
 * Outputs per candidate: d_outcome (u8: 0 nothing, 1 returned out of Refine(), 2 exhausted with the best), d_Tcw [12] float = R row-major then
 * t (mRefinedTcw / mBestTcw, rounded once from double; untouched on outcome 0), d_n_inliers, d_inlier [candidates][max_n] u8 (rows
 * [0, n) are written, zero on outcome 0; rows at n and above are untouched).  d_stats NULL or [candidates][4] = iteration budget (0 for
 * n < nMin), the returning iteration (outcome 2: the best's; -1 none), the count of that iteration's hypothesis, Refine() calls (iterations up to
 * the return whose count reached nMin).
 * d_counts NULL or [candidates][max_iterations] = inliers of every iteration (-1 for iterations the call does not run).
 * max_n <= 8192 and max_iterations <= 1024, else ORBHIP_E_CAPACITY; min_set != 6, min_inliers < 1, max_iterations < 1, probability
 * outside (0, 1), epsilon outside (0, 1], th2 <= 0, first_call_iterations < 0 or resume_at < 0: ORBHIP_E_BADARG with the field named by
 * orbhip_last_error(); a candidate with n > max_n or n < 0 sets the context's status word and writes nothing but outcome = 0,
 * n_inliers = 0 and its d_stats entry (0, -1, 0, 0).  cam / p are HOST pointers (the camera parameters are narrowed to float, the
 * reference's mvParameters), all others DEVICE; asynchronous on the context's stream. */
typedef struct orbhip_mlpnp_params {
    double probability;                             /* 0.99       (include/MLPnPsolver.h:65) */
    int32_t min_inliers, max_iterations, min_set;   /* 8, 300, 6; min_set must be 6 */
    float epsilon, th2;                             /* 0.4f, 5.991f */
    int32_t first_call_iterations;                  /* 0: the loop's `|| nCurrentIterations < nIterations` (:113); the class passes its nIterations */
    int32_t resume_at;                              /* 0: iterations below it update the best but cannot return (a resumed iterate()) */
    int32_t draw_sets; uint64_t seed;               /* 1, 0 */
} orbhip_mlpnp_params;
void orbhip_mlpnp_default_params(orbhip_mlpnp_params *p);
int orbhip_mlpnp_solver_device(orbhip_ctx *ctx, const float *d_Xw, const float *d_p2d, const float *d_sigma2, const int32_t *d_n,
        int candidates, int max_n, const orbhip_sim3_camera *cam, const orbhip_mlpnp_params *p, int32_t *d_sets, uint8_t *d_outcome,
        float *d_Tcw, int32_t *d_n_inliers, uint8_t *d_inlier, int32_t *d_stats, int32_t *d_counts);
/* the same for ONE candidate of n matches, HOST pointers (one page-locked blob up, one down; synchronous): sets [max_iterations][6]
 * in (draw_sets == 0) or out, inlier_out [n]; stats_out [4] and counts_out [max_iterations] may be NULL.  What host/MLPnPsolver.cc
 * calls. */
int orbhip_mlpnp_solver_host(orbhip_ctx *ctx, const float *Xw, const float *p2d, const float *sigma2, int n, const orbhip_sim3_camera *cam,
        const orbhip_mlpnp_params *p, int32_t *sets, uint8_t *outcome_out, float *Tcw_out, int32_t *n_inliers_out, uint8_t *inlier_out,
        int32_t *stats_out, int32_t *counts_out);

/* ------------------------------------------------------------------ Tracking::SearchLocalPoints
 * Frame::isInFrustum (src/Frame.cc:483-572) and Frame::isInFrustumChecks (:1170-1243) over a list of local map points, the query list
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) builds from their result (src/ORBmatcher.cc:54-79,
 * :149-156), and nToMatch of Tracking::SearchLocalPoints (src/Tracking.cc:2380-2401), batched over frames.
 * Per frame, HOST-built (3x3 products done once per frame, in the roundings of host/cvmath.h): */
#define ORBHIP_FRUSTUM_CHUNK 256      /* points a workgroup takes per trip (orbhip_frustum_chunk() returns it) */
#define ORBHIP_FRUSTUM_MAX_LEVELS 32
typedef struct orbhip_frustum_frame {
    float Rcw[9], tcw[3], Ow[3];      /* mRcw, mtcw, mOw (Frame::UpdatePoseMatrices, Frame.cc:456-462) */
    float Rrw[9], trw[3], Orw[3];     /* rig: Rrl*mRcw, Rrl*mtcw + trl, mRwc*mTlr.col(3) + mOw (Frame.cc:1176-1180) */
    float cam[2][8];                  /* mvParameters of mpCamera / mpCamera2: fx fy cx cy k1 k2 k3 k4 */
    int32_t cam_type[2];              /* 0 Pinhole, 1 KannalaBrandt8; [1] is read for a rig only */
    int32_t rig;                      /* Nleft != -1 */
    float mbf;
    int32_t nlevels;                  /* mnScaleLevels, 1..32 */
    float scale_factors[ORBHIP_FRUSTUM_MAX_LEVELS];      /* mvScaleFactors */
    float level_thresholds[ORBHIP_FRUSTUM_MAX_LEVELS];   /* [nlevels - 1] from orbhip_predict_scale_thresholds(mfLogScaleFactor, nlevels, ..) */
    float th;                         /* SearchByProjection's th */
    int32_t far_points;               /* bFarPoints */
    float th_far_points;              /* thFarPoints */
    float viewing_cos_limit;          /* isInFrustum's viewingCosLimit (0.5, Tracking.cc:2392) */
    int32_t n_points;                 /* points of this frame's list, 0..max_points */
} orbhip_frustum_frame;
/* Per point: what the reference would have stored in the MapPoint, and why it stopped.  code / code_r (left or only camera / right
 * camera): 0 accepted, 1 skipped (flag bit 1), 2 negative depth, 3 u outside, 4 v outside, 5 too near, 6 too far, 7 viewing angle;
 * code_r of a single-camera frame is 255.  Which fields the reference writes follows from the code:
 *   single camera (Frame.cc:485-560): mbTrackInView = in_view always (unless skipped); mTrackProjX / Y = -1 for code 2..4 and the
 *     projection for code 0 and 5..7 (:488-489, :516-517) -- proj_x / proj_y hold exactly that; proj_xr, depth, level, view_cos for
 *     code 0 only;
 *   rig (:562-570): both flags, and both levels reset to -1 (level / level_r hold -1 unless accepted); proj_x, proj_y, level, view_cos,
 *     depth for code 0; proj_xr, proj_yr, level_r, view_cos_r, depth_r for code_r 0.
 * Fields the reference leaves untouched are 0 here (all of them for a skipped point; level / level_r of a rig frame are -1 then too). */
typedef struct orbhip_track_record {
    float proj_x, proj_y, proj_xr, proj_yr, depth, depth_r, view_cos, view_cos_r;
    int32_t level, level_r;
    uint8_t in_view, in_view_r, code, code_r;
} orbhip_track_record;
/* Per-point inputs, DEVICE arrays of `frames` rows of max_points entries: d_Xw [..][3] GetWorldPos, d_normal [..][3] GetNormal,
 * d_min_dist / d_max_dist mfMinDistance / mfMaxDistance RAW (the 0.8f and 1.2f of MapPoint.cc:502-512 are applied here), d_flags: bit 0 =
 * Observations() > 0, bit 1 = skip (mnLastFrameSeen == F.mnId || isBad(), Tracking.cc:2387-2390), d_desc [..][32] GetDescriptor,
 * d_track_depth (may be NULL = 0): the point's mTrackDepth BEFORE the call -- the far-point test of ORBmatcher.cc:60 reads it, and
 * the reference leaves it stale when only the right camera of a rig sees the point.
 * Outputs, DEVICE: d_track [frames][max_points]; d_n_to_match [frames] = points for which isInFrustum returned true; d_q, d_desc_q
 * ([..][32]), d_owner [frames][max_q]: the queries in LIST order exactly as host/ORBmatcher.cc builds them (radius =
 * RadiusByViewingCos(viewCos) [* th when th != 1, left / only camera] * scale_factors[level], levels (level - 1, level), ur =
 * mTrackProjXR -- for a rig frame that is proj_xr of the record, which the rig matcher does not read --, a rig point's left query first,
 * its right query with has_obs | 2 behind it; points with far_points && mTrackDepth > th_far_points emit none), their descriptors
 * gathered into query order, and the index of the point that owns each query; d_nq [frames].  A frame with more than max_q queries
 * sets the context's status word (ORBHIP_E_CAPACITY on orbhip_ctx_check_status) and gets d_nq = 0; its track records and
 * d_n_to_match are complete.  PredictScale (MapPoint.cc:514-546) counts the level thresholds the ratio mfMaxDistance / dist reaches;
 * where the reference is undefined (dist == 0, a ratio that is not a positive finite number: it converts inf / NaN to int) the level is 0.
 * min_x .. max_y = Frame::mnMinX .. mnMaxY.  `frame` is a HOST array, checked here (more than 32 levels, a rig without a second
 * camera, n_points outside 0..max_points, max_q < 1: ORBHIP_E_BADARG, the field named by orbhip_last_error()) and copied to the
 * device; it may be reused on return.  One workgroup per frame; asynchronous on the context's stream. */
int orbhip_frustum_queries_device(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, float min_x, float min_y, float max_x, float max_y, int max_q,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq);
int orbhip_frustum_chunk(void);
/* The level thresholds of MapPoint::PredictScale for a frame with log scale factor mfLogScaleFactor: out[n], n in [0, nlevels - 2], is
 * the smallest float ratio for which ceil(logf(ratio) / log_scale_factor) exceeds n (found by bisection over float bit patterns with the
 * caller's libm; +inf if there is none), so that the number of thresholds a ratio reaches IS the clamped level.  HOST only, no device. */
int orbhip_predict_scale_thresholds(float log_scale_factor, int nlevels, float *out);
/* orbhip_frustum_queries_device and then the matcher -- orbhip_search_local_map_device, or orbhip_search_by_projection_rig_device mode 1
 * when d_nleft is given -- on the context's stream with no synchronisation in between: the first half of Tracking::TrackLocalMap
 * (Tracking::SearchLocalPoints, src/Tracking.cc:2380-2429) for `frames` frames.  Train side as in the matchers (d_u_right single camera
 * only, d_nleft / d_mirror rig only; every frame record's rig flag must agree with d_nleft); d_q / d_desc_q / d_owner / d_nq
 * [frames][max_q] are written by the first kernel and read by the second, and max_q picks the matcher's form as it does there. */
int orbhip_search_local_points_device(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, int frames, int max_points,
        const float *d_Xw, const float *d_normal, const float *d_min_dist, const float *d_max_dist, const uint8_t *d_flags,
        const uint8_t *d_desc, const float *d_track_depth, int max_q, const orbhip_keypoint *d_kp, const uint8_t *d_desc_kp,
        const float *d_u_right, const int32_t *d_n, const int32_t *d_nleft, const int32_t *d_mirror, int max_n, size_t frame_stride_kp,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio,
        orbhip_track_record *d_track, int32_t *d_n_to_match, orbhip_proj_query *d_q, uint8_t *d_desc_q, int32_t *d_owner, int32_t *d_nq,
        int32_t *d_train_match, int32_t *d_nmatches);
/* The same for ONE frame, HOST pointers: the points travel in one page-locked blob each way.  points: frame->n_points entries each;
 * train side as orbhip_search_by_projection_host (nleft = -1) or orbhip_search_by_projection_rig_host (nleft >= 0); track_out
 * [n_points], owner_out [n_points, twice that for a rig] (entries from *nq_out on are unspecified), train_match_inout [n].  The resident
 * form takes the train side as orbhip_search_by_projection_host_resident does (single camera). */
typedef struct orbhip_local_points {
    const float *Xw, *normal, *min_dist, *max_dist;
    const uint8_t *flags, *desc;
    const float *track_depth;            /* or NULL */
    int32_t n;                           /* must equal frame->n_points */
} orbhip_local_points;
int orbhip_search_local_points_host(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, const orbhip_local_points *points,
        const orbhip_keypoint *kp, const uint8_t *desc, const float *u_right, int n, int nleft, const int32_t *mirror,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio, orbhip_track_record *track_out,
        int32_t *n_to_match_out, int32_t *owner_out, int32_t *nq_out, int32_t *train_match_inout, int32_t *nmatches_out);
int orbhip_search_local_points_host_resident(orbhip_ctx *ctx, const orbhip_frustum_frame *frame, const orbhip_local_points *points,
        const orbhip_keypoint *kp_host, const orbhip_keypoint *d_kp, const uint8_t *d_desc, const float *u_right, int n,
        float min_x, float min_y, float max_x, float max_y, int th_high, float nn_ratio, orbhip_track_record *track_out,
        int32_t *n_to_match_out, int32_t *owner_out, int32_t *nq_out, int32_t *train_match_inout, int32_t *nmatches_out);

/* ------------------------------------------------------------------ KeyFrameDatabase: BoW place recognition
 * KeyFrameDatabase::add / erase / clear / clearMap (src/KeyFrameDatabase.cc:35-98), DetectNBestCandidates (:612-780) and
 * DetectRelocalizationCandidates (:783-895) with L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), batched over queries.
 * DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no caller in the reference and are not mirrored.
 * The database is a device-resident object of `capacity` keyframe SLOTS (the caller maps its keyframes to slots) holding, per slot, a
 * row of max_words (<= 4096, the limit of orbhip_bow_vectors_device) ascending word ids and L1-normalised double values -- mBowVec as
 * orbhip_bow_vectors_device leaves it --, the word count, an alive flag, the sequence number the add drew and a map id, and the state the
 * reference keeps in the KeyFrame object: (mnPlaceRecognitionQuery, mnPlaceRecognitionWords, mPlaceRecognitionScore) and (mnRelocQuery,
 * mnRelocWords, mRelocScore), all 0 at creation.  There is no inverted file: the reference's lKFsSharingWords -- query words ascending,
 * within a word the inverted list's order -- is the alive slots sharing a word, ascending by (smallest shared word id, add sequence
 * number); an erased and re-added slot draws a new number and so goes to the back of every list, as push_back does.
 * What decides bits, per query (id = pKF->mnId / F->mnId, map_id, mode):
 *   words    a slot sharing c > 0 words whose stored query id differs from id: place recognition and the slot is in the query's connected
 *            list -> words = 1, not marked, not listed (:635-645); else stored id = id, words = c, listed.  Stored id == id already (a
 *            repeated id, or id 0 on fresh state): words += c, not listed.  Relocalisation has no connected list (:798-804).
 *   scored   max_common = largest words over the LIST; listed slots with words > (int)(max_common * 0.8f) (float product, truncated,
 *            strict) are scored: double sum over the shared words ascending of fabs(vi - wi) - fabs(vi) - fabs(wi), sequentially in
 *            that order, then (float)(-sum / 2.0); the slot's stored score becomes it.
 *   acc      over the scored slots in list order: acc_score = score + the stored scores of those of its first ORBHIP_KFDB_NEIGHBOURS
 *            covisibility neighbours whose stored id == id (float, in neighbour order; a neighbour that was not scored by this query
 *            contributes what an earlier query left, :704-712); best_slot = the slot or the neighbour with the strictly largest score.
 *   NBest    (place recognition, :722-752) stable order by acc_score descending, first-seen best_slot only: same map as the query ->
 *            loop list, another map that is not in the bad list -> merge list, each up to n_candidates.  The reference's isBad() branch
 *            (:735) does not advance and would never end; a bad keyframe has left the database and every covisibility list, so here it
 *            cannot occur and the entry is simply passed over.
 *   Reloc    (:873-894) list order, acc_score > 0.75f * best acc_score and the map of best_slot == map_id, first-seen best_slot only.
 * A call with several queries is the reference's function called once per query in index order on the same state: counting and scoring
 * run in parallel over (query, slot), the state rules are applied per slot in query order. */
typedef struct orbhip_kfdb orbhip_kfdb;
#define ORBHIP_KFDB_PLACE 0           /* DetectNBestCandidates: the place-recognition state triple, connected keyframes, loop + merge lists */
#define ORBHIP_KFDB_RELOC 1           /* DetectRelocalizationCandidates: the relocalisation state triple, one list */
#define ORBHIP_KFDB_NEIGHBOURS 10     /* GetBestCovisibilityKeyFrames(10) */
#define ORBHIP_KFDB_MAX_WORDS 4096
#define ORBHIP_KFDB_MAX_LIST 4096
typedef struct orbhip_kfdb_query { uint64_t id; int32_t map_id, mode; } orbhip_kfdb_query;
typedef struct orbhip_kfdb_entry { int32_t slot, words, scored; float score; } orbhip_kfdb_entry;               /* score is 0 unless scored */
typedef struct orbhip_kfdb_candidate { int32_t slot; float score, acc_score; int32_t best_slot; } orbhip_kfdb_candidate;
typedef struct orbhip_kfdb_slot_state {
    uint64_t query[2]; int32_t words[2]; float score[2];      /* [ORBHIP_KFDB_PLACE], [ORBHIP_KFDB_RELOC] */
    int32_t n_words, alive, map_id; uint32_t sequence;
} orbhip_kfdb_slot_state;
/* capacity < 1 or max_words outside 1..4096: ORBHIP_E_BADARG naming the field.  The database lives on ctx's device and every entry below
 * is ordered on ctx's stream; destroy synchronises first. */
int orbhip_kfdb_create(orbhip_ctx *ctx, int capacity, int max_words, orbhip_kfdb **out);
void orbhip_kfdb_destroy(orbhip_kfdb *db);
/* KeyFrameDatabase::add.  _device: d_word / d_value = the keyframe's row of orbhip_bow_vectors_device's d_bow_word / d_bow_value and
 * d_nwords the address of its count, copied device to device with no host visit; a count outside 0..max_words sets the context's status
 * word and leaves the slot empty on the device (erase it before using it again).  _host: the same from host arrays (nwords > max_words:
 * ORBHIP_E_CAPACITY).  A slot outside the capacity: ORBHIP_E_CAPACITY; a slot that is alive: ORBHIP_E_BADARG.  The stored state of the
 * slot is kept, as the reference's keyframe object keeps its fields. */
int orbhip_kfdb_add_device(orbhip_kfdb *db, int slot, int map_id, const int32_t *d_word, const double *d_value, const int32_t *d_nwords);
int orbhip_kfdb_add_host(orbhip_kfdb *db, int slot, int map_id, const int32_t *word, const double *value, int nwords);
/* erase: the slot leaves every list and keeps its state (a slot that is not alive: no-op).  clear_map: erase of every slot of that map
 * (clearMap).  clear: every slot released, all state zero, the sequence restarts.  reset_slot: the two state triples of one slot to zero,
 * for a slot handed to a new keyframe. */
int orbhip_kfdb_erase(orbhip_kfdb *db, int slot);
int orbhip_kfdb_clear_map(orbhip_kfdb *db, int map_id);
int orbhip_kfdb_clear(orbhip_kfdb *db);
int orbhip_kfdb_reset_slot(orbhip_kfdb *db, int slot);
/* slots [first, first + n) as they are after everything submitted so far (synchronous; tests and the host class's checks) */
int orbhip_kfdb_get_state_host(orbhip_kfdb *db, int first, int n, orbhip_kfdb_slot_state *out);
/* The first half: the sharing list and the scores.  query: HOST records [queries] (copied; reusable on return).  Query q reads its
 * vector at d_qword / d_qvalue + q * q_stride with d_qn[q] words, and its connected keyframes (place recognition only) as
 * d_connected[q * max_connected .. + d_nconnected[q]) slots (entries outside the capacity stand for keyframes without a slot and are
 * ignored; a count above max_connected is cut to it; d_connected may be NULL with max_connected 0).
 * Outputs, DEVICE: d_counts [queries][4] = n_sharing, max_common, n_scored, n_touched; d_list [queries][max_list]: rows [0, n_sharing)
 * the sharing list in list order {slot, words, scored, score}; rows [n_sharing, n_sharing + n_touched) the slots whose words changed
 * WITHOUT being listed (connected: words 1; repeated id: the grown count), in the same order rule -- the host class needs them to leave
 * every KeyFrame field as the reference does.  Rows behind that are untouched.  The stored state of every slot is updated.
 * A query with d_qn outside 0..max_words, or with n_sharing + n_touched > max_list, sets the context's status word (ORBHIP_E_CAPACITY on
 * orbhip_ctx_check_status) and writes nothing but zero counts; in the first case it leaves the state alone as well, in the second the
 * state is updated as the reference's would be.  max_list outside 1..4096: ORBHIP_E_CAPACITY; a NULL database or output, queries < 1, a
 * mode that is neither ORBHIP_KFDB_PLACE nor ORBHIP_KFDB_RELOC: ORBHIP_E_BADARG naming the field.  Asynchronous. */
int orbhip_kfdb_score_device(orbhip_kfdb *db, const orbhip_kfdb_query *query, int queries, const int32_t *d_qword, const double *d_qvalue,
        const int32_t *d_qn, int q_stride, const int32_t *d_connected, const int32_t *d_nconnected, int max_connected, int max_list,
        int32_t *d_counts, orbhip_kfdb_entry *d_list);
/* The whole chain.  d_neighbours [capacity][ORBHIP_KFDB_NEIGHBOURS]: per slot the slots of GetBestCovisibilityKeyFrames(10) in their
 * order, -1 (or anything outside the capacity) for none / a keyframe without a slot, maintained by the caller; bad_maps: HOST list of
 * n_bad map ids for which Map::IsBad() holds.  Further outputs, DEVICE: d_scored [queries][max_list]: the n_scored scored slots in list
 * order with acc_score and best_slot; d_loop / d_merge [queries][n_candidates] slots and d_ncand [queries][2] their counts (0, 0 for a
 * relocalisation query); d_reloc [queries][max_list] and d_nreloc [queries] (0 for a place-recognition query).  n_candidates < 0:
 * ORBHIP_E_BADARG.  Rows behind the counts are untouched. */
int orbhip_kfdb_detect_device(orbhip_kfdb *db, const orbhip_kfdb_query *query, int queries, const int32_t *d_qword, const double *d_qvalue,
        const int32_t *d_qn, int q_stride, const int32_t *d_connected, const int32_t *d_nconnected, int max_connected,
        const int32_t *d_neighbours, int n_candidates, const int32_t *bad_maps, int n_bad, int max_list,
        int32_t *d_counts, orbhip_kfdb_entry *d_list, orbhip_kfdb_candidate *d_scored, int32_t *d_loop, int32_t *d_merge, int32_t *d_ncand,
        int32_t *d_reloc, int32_t *d_nreloc);
/* orbhip_kfdb_score_device for ONE query with HOST pointers (one page-locked blob up, one down; synchronous): counts_out [4], list_out
 * [max_list] (rows behind n_sharing + n_touched unspecified).  What host/KeyFrameDatabase.cc calls once per Detect... . */
int orbhip_kfdb_score_host(orbhip_kfdb *db, const orbhip_kfdb_query *query, const int32_t *word, const double *value, int nwords,
        const int32_t *connected, int n_connected, int max_list, int32_t *counts_out, orbhip_kfdb_entry *list_out);

/* ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2347-2663, the 7-argument overload LoopClosing::CorrectLoop calls at
 * src/LoopClosing.cc:1223): the Sim3 pose graph that spreads a loop's error over the map, and the correction of the map points.
 * A Sim3 is 8 doubles (qx qy qz qw tx ty tz s).
 *   vertices   one VertexSim3Expmap per keyframe (:2390-2426); fixed[v] != 0: the vertex does not move (:2418-2419, the map's first
 *              keyframe; the merge overloads fix several).  _fix_scale = params.fix_scale (:2424).
 *   edges      EdgeSim3 with identity information (:2429, :2466, ...): vertex(0) = edge_v0, vertex(1) = edge_v1, measurement edge_meas =
 *              Sji.  Their order is the caller's (the reference's: LoopConnections :2436-2474, then per keyframe the spanning-tree edge
 *              :2497-2521, older loop edges :2524-2551, covisibility edges :2554-2588, the mPrevKF edge :2591-2613); it is the
 *              summation order of every block of the system.  Several edges between one pair are allowed (they do occur); an edge from a
 *              vertex to itself is not.
 *   residual   log(Sji * S_i * S_j^-1) (types_seven_dof_expmap.h:106-114) with g2o::Sim3::log, operator* and inverse (sim3.h:148-230,
 *              :266-272, :233-236): four branches on |sigma| < 1e-5 and d > 1 - 1e-5, the small-angle omega = 1/2 deltaR(R), upsilon by
 *              a row-pivoted LU of W.
 *   Jacobians  the reference's numeric ones (base_binary_edge.hpp:136-200): central differences with delta = 1e-9 per coordinate through
 *              the vertex's own oplus, Sim3(update) * estimate with update[6] = 0 under fix_scale (types_seven_dof_expmap.h:60-69) --
 *              column 6 is then exactly zero.  A fixed vertex gets none; an edge between two fixed vertices is not active and adds
 *              nothing to chi2 (sparse_optimizer.cpp:234).
 *   solver     Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:61-169 runs it: lambda starts at lambda_init (:2364
 *              setUserLambdaInit(1e-16)), up to max_trials trials after a failure, no robust kernel, the three-bad-iterations stop of
 *              :157-166; the dense system H + lambda I is factored as L D L^T without pivoting (a zero or non-finite pivot fails the
 *              solve and leaves x as it was).  7 * n_free <= 4096 unknowns (585 free keyframes), else ORBHIP_E_CAPACITY with the count
 *              in the message, nothing written, no CPU fallback.  Up to 480 unknowns one workgroup factors; above, many.
 * Graphs of one call are solved one after the other; the LM control runs on the host (one 24-byte read-back per trial).
 * ORBHIP_E_BADARG names the field through orbhip_last_error(): a NULL pointer, n_vertices / n_edges < 0, an edge index outside the
 * vertices (edge_v0 / edge_v1), an edge from a vertex to itself, a non-finite measurement (edge_meas) or estimate (sim3_inout),
 * iterations < 1, max_trials < 1, lambda_init that is not finite and positive.  Every graph is checked before any is solved and before
 * the device is touched.  A graph without a free vertex or without an active edge: ORBHIP_OK, zero iterations, estimates untouched.
 * Reruns are byte-identical (no atomics, every sum in a fixed order). */
typedef struct orbhip_pose_graph {
    int32_t n_vertices; const uint8_t *fixed;                  /* [n_vertices] */
    int32_t n_edges; const int32_t *edge_v0, *edge_v1;         /* vertex(0), vertex(1) */
    const double *edge_meas;                                   /* [n_edges][8] = qx qy qz qw tx ty tz s of Sji */
} orbhip_pose_graph;
typedef struct orbhip_pose_graph_params {
    int32_t iterations;            /* optimizer.optimize(20), :2617 */
    double lambda_init;            /* 1e-16, :2364 */
    int32_t fix_scale;             /* bFixScale */
    int32_t max_trials;            /* _maxTrialsAfterFailure = 100 */
} orbhip_pose_graph_params;
void orbhip_pose_graph_default_params(orbhip_pose_graph_params *p);       /* 20, 1e-16, 0, 100 */
#define ORBHIP_PG_END_ITERATIONS 0   /* every iteration ran */
#define ORBHIP_PG_END_TERMINATE 1    /* max_trials trials used, or rho == 0 (levenberg.cpp:151-155) */
#define ORBHIP_PG_END_NBAD 2         /* three iterations in a row gained less than 1e-3 of chi2 (:157-166) */
#define ORBHIP_PG_END_SOLVE_FAILED 3 /* ORBHIP_PG_END_TERMINATE where no trial of the FIRST iteration could be solved: estimates untouched */
typedef struct orbhip_pose_graph_stats {
    double chi2_initial, chi2_final, lambda;
    int32_t iterations, trials, end_reason, n_free, n_unknowns;
} orbhip_pose_graph_stats;
#define ORBHIP_PG_TRACE 4            /* doubles per trial of trace_out: chi2 of the trial, rho, the lambda it was solved with, accepted (1 / 0) */
/* All pointers HOST; synchronous.  sim3_inout[g] [n_vertices][8]: the estimates (CorrectedSim3 or Sim3(Rcw, tcw, 1), :2402-2416), replaced
 * by the optimised ones.  stats_out [n_graphs] may be NULL.  trace_out: NULL, or [n_graphs][iterations * max_trials][ORBHIP_PG_TRACE],
 * the first stats.trials rows of a graph written. */
int orbhip_optimize_essential_graph_host(orbhip_ctx *ctx, const orbhip_pose_graph *graphs, int n_graphs, const orbhip_pose_graph_params *params,
        double *const *sim3_inout, orbhip_pose_graph_stats *stats_out, double *trace_out);
/* The map points' correction (:2636-2660): Xw <- corrected_Swc[ref].map(Scw[ref].map(Xw)) in double on the float position, rounded once
 * to float.  d_ref [n_points]: the point's vertex (mnCorrectedReference or the reference keyframe, :2645-2653); ref < 0 or >=
 * n_vertices: the point is copied through.  d_Scw, d_corrected_Swc [n_vertices][8].  All pointers DEVICE, d_Xw_out may be d_Xw;
 * asynchronous on the context's stream. */
int orbhip_pose_graph_correct_points_device(orbhip_ctx *ctx, const float *d_Xw, const int32_t *d_ref, int n_points,
        const double *d_Scw, const double *d_corrected_Swc, int n_vertices, float *d_Xw_out);
/* With ORBHIP_PG_PROF=1 in the environment the solve brackets every stage with two events on its stream and sums the stage's DEVICE
 * time (microseconds): out7 = linearise, assemble, fill + factor + solve, update + errors + reductions, then the trials, iterations and
 * calls counted; reset != 0 clears the sums.  Debug only: the sums are plain process-wide variables, not synchronised -- one profiled
 * caller at a time (tools/essential_graph_probe.py). */
int orbhip_debug_pose_graph_prof(double *out7, int reset);
/* Which factorisation the calling thread's last solved graph took: 0 one workgroup (<= 480 unknowns), 1 many workgroups, -1 none yet. */
int orbhip_debug_pose_graph_last_path(void);
/* The dense solve chain of one trial alone, on a system of the caller's: S x = rhs by the single-workgroup kernel for n <= 480 unless
 * force_big != 0, else by the many-workgroup factorisation (what k_ba_big_* and k_pg4_big_* run too).  All pointers HOST; synchronous.
 * x_out [n] is written when every pivot was good (*ok_out = 1) and left untouched otherwise (*ok_out = 0).  ORBHIP_E_BADARG for
 * n < 1 or a NULL pointer, ORBHIP_E_CAPACITY for n > 4096.  Debug only (tests/test_gpu_dense_ldlt.py). */
int orbhip_debug_pose_graph_dense_solve_host(orbhip_ctx *ctx, const double *S /* n*n, lower triangle read */, int n, const double *rhs, double *x_out,
        int force_big, int *ok_out);
/* One shared geometry primitive of the optimisers and matchers alone on the device, one lane per item (csrc/geom_probe_kernels.hip): row i
 * of in [n][in_width] goes through the op's function, its result to row i of out [n][out_width]; rows of `out` past n are not written.
 * All pointers HOST, all values double; synchronous.  The float ops (TRI_*) take doubles that hold float-exact values and return such.
 * Layouts: a quaternion is (x y z w), a matrix row-major, an SE3 (q t), a Sim3 (q t s), a tangent (omega upsilon [sigma]).
 *   QUAT_TO_R 4->9  R_TO_QUAT 9->4  QUAT_ROT (q v) 7->3  QUAT_MUL (a b) 8->4  QUAT_NORM_ROT 4->4  HUBER (e delta dsqr) 3->(rho rho') 2
 *   SE3_OPLUS (u pose) 13->7  SE3_MUL (a b) 14->7  SO3_EXP 3->9 (eps 1e-5, re-orthonormalised)  SO3_EXP_IMU 3->9 (eps 1e-4, not)
 *   SO3_LOG 9->3  SO3_RIGHT_JAC 3->9  SO3_INV_RIGHT_JAC 3->9  SO3_NORMALIZE 9->9  S3_EXP 7->8  S3_LOG 8->7  S3_MUL (a b) 16->8
 *   S3_INVERSE 8->8  S3_MAP (S X) 11->3  CAM_PROJECT (fx fy cx cy model k[4] P) 12->2  CAM_PROJECT_JAC (the same) 12->6
 *   TRI_PROJECT_PINHOLE / _KB8 (p[8] P) 11->2  TRI_UNPROJECT_PINHOLE / _KB8 (p[8] u v) 10->3  TRI_SVD4_NULL (At[4][4]) 16->4
 * ORBHIP_E_BADARG for an unknown op, widths that are not the op's, n < 0 or a NULL pointer with n > 0; ORBHIP_E_CAPACITY for n > 65536;
 * n == 0 launches nothing.  Debug only (tests/test_gpu_geom_probe.py). */
enum {
    ORBHIP_GEOM_QUAT_TO_R = 0, ORBHIP_GEOM_R_TO_QUAT, ORBHIP_GEOM_QUAT_ROT, ORBHIP_GEOM_QUAT_MUL, ORBHIP_GEOM_QUAT_NORM_ROT, ORBHIP_GEOM_HUBER,
    ORBHIP_GEOM_SE3_OPLUS, ORBHIP_GEOM_SE3_MUL, ORBHIP_GEOM_SO3_EXP, ORBHIP_GEOM_SO3_EXP_IMU, ORBHIP_GEOM_SO3_LOG, ORBHIP_GEOM_SO3_RIGHT_JAC,
    ORBHIP_GEOM_SO3_INV_RIGHT_JAC, ORBHIP_GEOM_SO3_NORMALIZE, ORBHIP_GEOM_S3_EXP, ORBHIP_GEOM_S3_LOG, ORBHIP_GEOM_S3_MUL, ORBHIP_GEOM_S3_INVERSE,
    ORBHIP_GEOM_S3_MAP, ORBHIP_GEOM_CAM_PROJECT, ORBHIP_GEOM_CAM_PROJECT_JAC, ORBHIP_GEOM_TRI_PROJECT_PINHOLE, ORBHIP_GEOM_TRI_PROJECT_KB8,
    ORBHIP_GEOM_TRI_UNPROJECT_PINHOLE, ORBHIP_GEOM_TRI_UNPROJECT_KB8, ORBHIP_GEOM_TRI_SVD4_NULL, ORBHIP_GEOM_N_OPS
};
int orbhip_debug_geom_probe_host(orbhip_ctx *ctx, int op, const double *in, int n, int in_width, double *out, int out_width);
/* The same with HOST pointers (one page-locked blob up, one down; synchronous): what host/Optimizer_OptimizeEssentialGraph.cc calls. */
int orbhip_pose_graph_correct_points_host(orbhip_ctx *ctx, const float *Xw, const int32_t *ref, int n_points,
        const double *Scw, const double *corrected_Swc, int n_vertices, float *Xw_out);

/* ---- Optimizer::OptimizeEssentialGraph4DoF (reference src/Optimizer.cc:8305-8610): the pose graph LoopClosing::CorrectLoop solves for an
 * inertial map whose IMU is initialised (src/LoopClosing.cc:1218) -- VertexPose4DoF / Edge4DoF (include/G2oTypes.h:152-186, :833-859).
 *   vertex     an ImuCamPose: Rwb0, DR, twb, Rcb, tcb, Rcw, tcw.  4 unknowns, yaw about the world z axis and the translation:
 *              oplus(x) is ImuCamPose::UpdateW (src/G2oTypes.cc:222-256): DR <- ExpSO3(0, 0, x0) DR, Rwb = DR Rwb0, twb += (x1, x2, x3),
 *              then Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb.  Rcw / tcw are LOADED and derived only at a vertex's first oplus:
 *              the nominal error of the first iteration is taken at the loaded ones, a fixed vertex keeps them throughout.
 *   residual   [LogSO3(Rcw_i Rcw_j^T dRij^T) ; Rcw_i (-Rcw_j^T tcw_j) + tcw_i - dtij], chi2 = e^T W e with W = diag(info_diag), no
 *              robust kernel.  The reference's W is diag(1e3, 1e3, 1, 1, 1, 1): :8378-8381 set (0,0) twice and never (2,2).
 *   Jacobians  the reference's numeric ones (base_binary_edge.hpp:136-200): central differences, delta = 1e-9, through the vertex's
 *              own oplus -- 17 error evaluations per edge.  A fixed vertex gets none; an edge between two fixed vertices is not active.
 *   solver     Levenberg-Marquardt as for orbhip_optimize_essential_graph_host, but lambda starts at tau * max |H(j, j)| over the free
 *              vertices' diagonal blocks after the first linearisation (optimization_algorithm_levenberg.cpp:171-185; tau = 1e-50 in
 *              this fork, :47) unless lambda_init > 0.  4 * n_free <= 4096 unknowns (1024 free keyframes), else ORBHIP_E_CAPACITY with
 *              the count in the message, nothing written, no CPU fallback.  Up to 480 unknowns (120 free keyframes) one workgroup
 *              factors; above, many.
 * ORBHIP_E_BADARG names the field: a NULL pointer, n_vertices / n_edges < 0, an edge index outside the vertices, an edge from a vertex
 * to itself, a non-finite edge_meas / state_inout / info_diag / lambda_init, iterations < 1, max_trials < 1, tau that is not finite and
 * positive while lambda_init <= 0.  Every graph is checked before any is solved and before the device is touched.  A graph without a
 * free vertex or without an active edge: ORBHIP_OK, zero iterations, state untouched.  Reruns are byte-identical. */
typedef struct orbhip_pose_graph4dof {
    int32_t n_vertices; const uint8_t *fixed;                  /* [n_vertices] */
    int32_t n_edges; const int32_t *edge_v0, *edge_v1;         /* vertex(0), vertex(1) */
    const double *edge_meas;                                   /* [n_edges][12] = dRij row-major, then dtij */
} orbhip_pose_graph4dof;
typedef struct orbhip_pose_graph4dof_params {
    int32_t iterations;            /* optimizer.optimize(20), :8562 */
    double lambda_init;            /* 0: computed, tau * max |H(j, j)| */
    double tau;                    /* 1e-50 */
    double info_diag[6];           /* 1e3, 1e3, 1, 1, 1, 1 */
    int32_t max_trials;            /* _maxTrialsAfterFailure = 100 */
} orbhip_pose_graph4dof_params;
void orbhip_pose_graph4dof_default_params(orbhip_pose_graph4dof_params *p);
#define ORBHIP_PG4_STATE 36          /* doubles per vertex of state_inout: Rwb 9 | twb 3 | Rcw 9 | tcw 3 | Rcb 9 | tcb 3 (matrices row-major) */
/* All pointers HOST; synchronous.  state_inout[g] [n_vertices][ORBHIP_PG4_STATE]: Rwb, twb, Rcw, tcw of a free vertex are replaced by
 * the optimised ones, a fixed vertex keeps its bytes.  stats_out, trace_out, the end reasons and the trace rows are those of
 * orbhip_optimize_essential_graph_host; stats.lambda is the lambda after the last trial. */
int orbhip_optimize_essential_graph4dof_host(orbhip_ctx *ctx, const orbhip_pose_graph4dof *graphs, int n_graphs,
        const orbhip_pose_graph4dof_params *params, double *const *state_inout, orbhip_pose_graph_stats *stats_out, double *trace_out);
/* Which factorisation the calling thread's last solved 4-DoF graph took: 0 one workgroup (<= 480 unknowns), 1 many, -1 none yet. */
int orbhip_debug_pose_graph4dof_last_path(void);

#ifdef __cplusplus
}
#endif
#endif
