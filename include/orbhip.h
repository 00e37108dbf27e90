/* orbhip.h — C ABI of liborbhip.so: the MI355X (gfx950) implementation of ORB-SLAM3's per-frame hot path.
 *
 * The reference has no FFI layer: the boundary is three C++ classes linked into libORB_SLAM3.so
 * (reference CMakeLists.txt:60-118).  Each entry point below names the reference interface it replaces;
 * the headers under include/orbslam3_hip/ hold header-only C++ adapters with the reference's class signatures that
 * forward to this ABI.
 *
 * Conventions: plain pointers and sizes only; caller-allocated outputs with explicit capacity; the library
 * owns device buffers per handle; no ownership crosses the ABI; no exceptions cross the ABI; every function
 * returns ORB_OK (0) or a negative ORB_E_* code, with a message retrievable by orb*_last_error().
 * "dev" pointers are HIP device pointers on the handle's device; `stream` is a hipStream_t (NULL = the HIP
 * default stream; the host-buffer entry points use a private stream of the handle and synchronise it).  Handles are not re-entrant; distinct handles may be used concurrently
 * (reference threading: one ORBextractor per camera, Frame.cc:111-114).
 */
#ifndef ORBHIP_H
#define ORBHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORB_OK 0
#define ORB_E_EMPTY_IMAGE (-1)   /* mirrors `return -1` of ORBextractor::operator(), ORBextractor.cc:1078-1079 */
#define ORB_E_CAPACITY (-2)      /* caller-provided output capacity too small (n_out holds the needed count) */
#define ORB_E_INVALID (-3)       /* bad argument / unsupported geometry */
#define ORB_E_HIP (-4)           /* HIP runtime error (see last_error) */
#define ORB_E_NOMEM (-5)
#define ORB_E_ABORTED (-6)       /* abort flag was raised (LBA pbStopFlag, Optimizer.cc:2197-2199) */

/* cv::KeyPoint layout (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct orb_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orb_keypoint;

/* ---------------------------------------------------------------------------------------------------------
 * Stage 1 — ORBextractor  (reference include/ORBextractor.h:49-83, src/ORBextractor.cc)
 * ------------------------------------------------------------------------------------------------------- */
typedef struct orbx_config {
    int32_t nfeatures;     /* ORBextractor.h:49 ctor arg 1 */
    float scale_factor;    /* arg 2 */
    int32_t nlevels;       /* arg 3 */
    int32_t ini_th_fast;   /* arg 4 */
    int32_t min_th_fast;   /* arg 5 */
} orbx_config;

typedef struct orbx_extractor* orbx_handle;

/* Replaces ORBextractor::ORBextractor (ORBextractor.cc:408-468) for images of one fixed size.
 * max_batch: number of frames one orbx_extract_batch_dev call may carry (device workspace is sized for it). */
int orbx_create(const orbx_config* cfg, int width, int height, int max_batch, int device, orbx_handle* out);
void orbx_destroy(orbx_handle h);
const char* orbx_last_error(orbx_handle h); /* h may be NULL: error of the last failed orbx_create */

/* Getters ORBextractor.h:61-81 (GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares) plus mnFeaturesPerLevel; arrays of nlevels entries, any may be NULL. */
int orbx_get_tables(orbx_handle h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                    int32_t* features_per_level);
/* Upper bound of keypoints one frame can return (sum over levels of N_l + 3, or the 4*nIni first-round bound). */
int orbx_max_keypoints(orbx_handle h);

/* Replaces ORBextractor::operator() (ORBextractor.cc:1074-1156) for one host image (CV_8UC1, row stride in
 * bytes).  lap0/lap1 = vLappingArea.  Writes n keypoints / n x 32 descriptor bytes in the reference's output
 * order; *mono_index = the reference's return value.  Returns ORB_E_EMPTY_IMAGE for a NULL / zero-sized image. */
int orbx_extract(orbx_handle h, const uint8_t* image, int width, int height, int stride, int lap0, int lap1,
                 orb_keypoint* kps, uint8_t* desc, int cap, int* n_out, int* mono_index);

/* The same call without the two output copies: *kps / *desc point into the handle's pinned output block ([n] records, [n][32] bytes), valid until
 * the next call on the handle.  The adapters copy from there straight into the caller's final containers (std::vector<cv::KeyPoint>, cv::Mat). */
int orbx_extract_view(orbx_handle h, const uint8_t* image, int width, int height, int stride, int lap0, int lap1,
                      const orb_keypoint** kps, const uint8_t** desc, int* n_out, int* mono_index);

/* mvImagePyramid for host consumers (public member ORBextractor.h:83; the only reader in the reference is Frame::ComputeStereoMatches,
 * Frame.cc:962,1052,1071).  keep = 1: every orbx_extract / orbx_extract_view also brings the pyramid of its image to the host in the reference's
 * layout (ORBextractor.cc:1164-1179: each level inside a 19-px BORDER_REFLECT_101 frame) — frame built on the device, ONE copy of the whole slab
 * into pinned memory on a second stream that runs under FAST / octree / describe.  keep = 0 (default): nothing is copied.
 * orbx_host_pyramid_level: pixel (0, 0) of `level` inside that slab (rows `stride` bytes apart, the 19 border pixels lie around it); the
 * storage is the handle's and is overwritten by the next call — cv::Mat headers over it need no per-call allocation. */
int orbx_set_host_pyramid(orbx_handle h, int keep);
int orbx_host_pyramid_level(orbx_handle h, int level, const uint8_t** ptr, int* w, int* hgt, int* stride);

/* Batched, device-resident form of the same call (MI355X addition; frames are independent units).
 * d_images: batch frames, frame b at d_images + b*frame_stride, rows row_stride bytes apart (4-byte aligned).
 * d_kps / d_desc: per-frame slabs of cap_per_frame entries; d_counts[2*b] = n, d_counts[2*b+1] = monoIndex
 * (n > cap_per_frame => that frame's slab holds the first cap_per_frame outputs and n reports the need; n and monoIndex are those of the whole
 * output and the slab holds its entries [0, cap_per_frame), so of a lapping split, which the reference fills from the back, the entries at the
 * front of the lapping part are the ones that are missing).  batch may be below the handle's max_batch: only the first `batch` slabs are written.
 * Asynchronous on `stream`. */
int orbx_extract_batch_dev(orbx_handle h, const uint8_t* d_images, int batch, size_t frame_stride, int row_stride,
                           int lap0, int lap1, orb_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame,
                           int32_t* d_counts, void* stream);

/* mvImagePyramid (public member, ORBextractor.h:83): device view of level `level` of frame `frame` of the last
 * call (un-bordered plane; the reference's 19-px BORDER_REFLECT_101 frame is produced by orbx_copy_level). */
int orbx_pyramid_level(orbx_handle h, int frame, int level, const uint8_t** d_ptr, int* w, int* hgt, int* stride);
/* Copies level to host; border = 0 (plane) or up to 19 (reference layout incl. reflected frame), out is tightly packed.  Waits for the stream of
 * the call that built the pyramid (never for the whole device); served from the host slab when orbx_set_host_pyramid is on. */
int orbx_copy_level(orbx_handle h, int frame, int level, int border, uint8_t* out);

/* Frame::ComputeStereoMatches (Frame.cc:955-1133) for `batch` rectified stereo pairs whose left / right images were just
 * extracted by `left` / `right` (the 11x11 SAD refinement reads their pyramids — mvImagePyramid of both extractors).
 * kps / desc / counts are the orbx_extract_batch_dev outputs of the two handles (counts = [batch][2]).
 * Outputs per left keypoint: u_right (mvuRight, -1 = no match) and depth (mvDepth, -1); d_work: cap_per_frame int32 per frame. */
int orbx_stereo_matches(orbx_handle left, orbx_handle right, const orb_keypoint* d_kps_l, const uint8_t* d_desc_l,
                        const int32_t* d_counts_l, const orb_keypoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_counts_r,
                        int cap_per_frame, int batch, float mb, float mbf, float* d_u_right, float* d_depth, int32_t* d_work,
                        void* stream);

/* Frame::ComputeStereoMatches for the pair whose images `left` and `right` each just took through orbx_extract (Frame.cc:110-114 then :132):
 * key points, descriptors and pyramids are read where those two calls left them on the device — nothing is uploaded; u_right / depth (host,
 * cap entries) receive mvuRight / mvDepth of the *n_left left key points.  Both handles: same device and configuration, last call = orbx_extract. */
int orbx_stereo_matches_last(orbx_handle left, orbx_handle right, float mb, float mbf, float* u_right, float* depth, int cap, int* n_left);

/* Stage-level taps for parity tests (valid after an extract call; host outputs):
 * FAST candidates of (frame, level) = vToDistributeKeys (ORBextractor.cc:776,845-850) as (x,y,score) int triples
 * in arbitrary order (the set is what the octree consumes); returns count via n_out. */
int orbx_debug_candidates(orbx_handle h, int frame, int level, int32_t* xys, int cap, int* n_out);
/* Octree output of (frame, level) in list order (DistributeOctTree result, ORBextractor.cc:737-761):
 * (x,y,score) int triples, coordinates relative to minBorder like the reference at that point. */
int orbx_debug_selected(orbx_handle h, int frame, int level, int32_t* xys, int cap, int* n_out);

/* Measurement facility (bench.py's per-kernel figures).  While enabled, a batch call records five HIP events on its launch stream (they cost the
 * three-stream step 0.5 %: off by default); orbx_last_timing then gives the device time of the last batch call's kernels:
 * ms[0]=pyramid ms[1]=FAST ms[2]=octree ms[3]=orient+blur+rBRIEF ms[4]=total (synchronises the stream; ORB_E_INVALID if no call was timed). */
int orbx_enable_timing(orbx_handle h, int on);
int orbx_last_timing(orbx_handle h, float* ms5);

/* How the last batch call ran FAST (a scheduling decision only: the key points do not depend on it).  two_pass: 1 = detection at iniThFAST followed by a
 * second launch on the cells that came back empty (ORBextractor.cc:812-828), 0 = one pass at min(ini, min).  listed / tiles: the tiles the handle's
 * most recent two-pass call sent to its second pass, of how many — the share that decides whether the next call takes two passes again (copied back
 * asynchronously, both words in one copy: synchronise the stream first for the figure of the call just made; the pair always belongs to ONE call).
 * A HIP graph captured from a batch call keeps the pass form it was captured with (the copy-back is not part of a capture).  Any pointer may be NULL. */
int orbx_last_fast_passes(orbx_handle h, int* two_pass, uint32_t* listed, uint32_t* tiles);

/* Two more scheduling decisions of the last batch call (never the result): frames_ordered = the (frame, tile) / (frame, level) workgroups were handed
 * out heaviest frame first, by the FAST candidate counts the handle's previous call left (a frame that costs ten times the others no longer ends the
 * launch alone); heavy_octree_pass = (frame, level) problems of 8 192 candidates or more were taken by a second k_octree launch with four times the
 * threads (chosen when the call before last had such a problem).  Any pointer may be NULL. */
int orbx_last_schedule(orbx_handle h, int* frames_ordered, int* heavy_octree_pass);

/* ---------------------------------------------------------------------------------------------------------
 * Stage 2 — ORBmatcher  (reference include/ORBmatcher.h:39-94, src/ORBmatcher.cc) + the Frame grid helpers it
 * depends on (src/Frame.cc:444-478, 755-862).  The reference functions walk pointer graphs (Frame&, KeyFrame*,
 * MapPoint*); this ABI works on the flattened records the adapters in include/orbslam3_hip/ORBmatcher.h gather,
 * batched over `batch` independent problems (frames / frame pairs) laid out as fixed-capacity slabs:
 * problem b uses kps + b*cap_k, desc + b*cap_k*32, queries + b*cap_q, ...   All pointers are device pointers.
 * ------------------------------------------------------------------------------------------------------- */
#define ORBM_TH_HIGH 100      /* ORBmatcher.cc:36 */
#define ORBM_TH_LOW 50        /* ORBmatcher.cc:37 */
#define ORBM_HISTO_LENGTH 30  /* ORBmatcher.cc:38 */
#define ORBM_GRID_COLS 64     /* FRAME_GRID_COLS, Frame.h:38 */
#define ORBM_GRID_ROWS 48     /* FRAME_GRID_ROWS, Frame.h:39 */

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:2700-2716) for every (query, train) pair:
 * out[b][i*nt + j] = Hamming(q[b][i], t[b][j]) as uint16.  nq/nt are the per-problem counts (same for all b). */
int orbm_hamming(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int batch, uint16_t* d_out, void* stream);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) as used by Frame::ComputeStereoFishEyeMatches (Frame.cc:1300):
 * per query the two nearest train descriptors, scanning train indices ascending with strict '<' (equal distances
 * keep the lower train index first).  d_nq / d_nt: per-problem counts (int32, element stride `count_stride`).
 * out_idx / out_dist: [batch][cap_q][2]; missing neighbours are idx -1, dist 256. */
int orbm_knn2(const uint8_t* d_q, const int32_t* d_nq, int cap_q, const uint8_t* d_t, const int32_t* d_nt, int cap_t,
              int count_stride, int batch, int32_t* d_out_idx, int32_t* d_out_dist, void* stream);

/* Frame bounds/grid scalars: mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv (Frame.cc:388-399) */
typedef struct orbm_grid_params {
    float min_x, min_y, grid_w_inv, grid_h_inv;
} orbm_grid_params;

/* Frame::AssignFeaturesToGrid + PosInGrid (Frame.cc:444-478, 852-862) as a CSR grid per frame:
 * cell = ix*ORBM_GRID_ROWS + iy; grid_start[b][cell..cell+1] delimit indices into grid_idx[b][], which lists keypoint
 * indices in insertion (ascending) order.  d_nkp: per-frame keypoint counts (element stride count_stride).
 * grid_start: [batch][64*48+1], grid_idx: [batch][cap_k]. */
int orbm_grid_build(const orb_keypoint* d_kps, const int32_t* d_nkp, int count_stride, int cap_k, int batch,
                    const orbm_grid_params* gp, int32_t* d_grid_start, int32_t* d_grid_idx, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Frame constructor steps between the extractor and the matcher (reference src/Frame.cc)
 * ------------------------------------------------------------------------------------------------------- */
/* Pinhole intrinsics (Pinhole::toK) + mDistCoef = (k1, k2, p1, p2, k3) (Frame.h mDistCoef; k3 = 0 for 4-coefficient files) */
typedef struct orbf_camera {
    float fx, fy, cx, cy;
    float dist[5];
} orbf_camera;

/* Frame::UndistortKeyPoints (Frame.cc:874-925): mvKeysUn = mvKeys with pt replaced by cv::undistortPoints(pt, K, mDistCoef, R = I, P = K);
 * dist[0] == 0 copies (:879-883).  In place (d_kps_un == d_kps) is allowed. */
int orbf_undistort_keypoints(const orb_keypoint* d_kps, const int32_t* d_nkp, int count_stride, int cap_k, int batch,
                             const orbf_camera* cam, orb_keypoint* d_kps_un, void* stream);
/* UndistortKeyPoints followed by AssignFeaturesToGrid (the Frame constructor's order, Frame.cc:137-167) as ONE launch, one workgroup per frame:
 * d_kps_un and the CSR grid exactly as orbf_undistort_keypoints + orbm_grid_build write them (single camera; gp from orbf_image_bounds).
 * d_kps_un == d_kps is allowed.  With orbm_enable_timing on, orbm_last_timing's ms[0] is this launch. */
int orbm_undistort_and_grid_build(const orb_keypoint* d_kps, const int32_t* d_nkp, int count_stride, int cap_k, int batch, const orbf_camera* cam,
                                  const orbm_grid_params* gp, orb_keypoint* d_kps_un, int32_t* d_grid_start, int32_t* d_grid_idx, void* stream);
/* Frame::ComputeImageBounds (Frame.cc:926-953) -> bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY} (host), and, if gp != NULL, the grid scalars
 * mfGridElementWidthInv / HeightInv of Frame.cc:394-397 ready for orbm_grid_build.  Synchronous (runs once per calibration). */
int orbf_image_bounds(const orbf_camera* cam, int width, int height, float bounds[4], orbm_grid_params* gp);
/* Frame::ComputeStereoFromRGBD (Frame.cc:1136-1157): depth image(s) float32, frame b at d_depth + b*frame_stride, rows row_stride floats
 * apart; mvDepth = d, mvuRight = kpU.x - mbf/d where d > 0, else -1.  Entries [n, cap_k) of the outputs are set to -1. */
int orbf_stereo_from_rgbd(const orb_keypoint* d_kps, const orb_keypoint* d_kps_un, const int32_t* d_nkp, int count_stride, int cap_k,
                          int batch, const float* d_depth, size_t frame_stride, int row_stride, int width, int height, float mbf,
                          float* d_u_right, float* d_depth_out, void* stream);

/* Frame::ComputeStereoFishEyeMatches (Frame.cc:1281-1325) with KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:334-400) for two fisheye
 * cameras.  Left / right keypoints and descriptors as the two extractors wrote them; d_n_* = Nleft / Nright, d_mono_* = monoLeft / monoRight (the
 * extractors' return values: keypoints [mono, N) lie in the lapping area), element stride count_stride (2 for orbx_extract_batch_dev counts:
 * pass d_counts and d_counts + 1).  Outputs: mvLeftToRightMatch [batch][cap_l], mvRightToLeftMatch [batch][cap_r] (indices into the own camera's
 * arrays, -1 = none), mvDepth [batch][cap_l] (-1), mvStereo3Dpoints [batch][cap_l][3] (left-camera frame; zeros where none), nMatches [batch]. */
typedef struct orbf_fisheye_rig {
    float k_left[8], k_right[8];   /* KannalaBrandt8 mvParameters fx fy cx cy k1..k4 of mpCamera / mpCamera2 */
    float R_lr[9], t_lr[3];        /* mRlr (row-major), mtlr = the rotation / translation of mTlr (Frame.cc:1242-1243) */
    float level_sigma2[16];        /* mvLevelSigma2 */
} orbf_fisheye_rig;
int orbf_stereo_fisheye_matches(const orb_keypoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l, const int32_t* d_mono_l,
                                const orb_keypoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, const int32_t* d_mono_r, int cap_l,
                                int cap_r, int count_stride, int batch, const orbf_fisheye_rig* rig, int32_t* d_left_to_right,
                                int32_t* d_right_to_left, float* d_depth, float* d_p3d, int32_t* d_nmatches, void* stream);

/* One projected map point = one query of a windowed search (the per-MapPoint values the reference computes before
 * calling Frame::GetFeaturesInArea: ORBmatcher.cc:88-103 for the local-map search, :2277-2309 for the motion model). */
typedef struct orbm_query {
    float u, v;          /* projection (mTrackProjX/Y, or uv) */
    float radius;        /* r * mvScaleFactors[level]  (window half-size, also the stereo gate) */
    float u_right;       /* mTrackProjXR / uv.x - mbf*invzc; only read when ORBM_Q_STEREO is set */
    float angle;         /* keypoint angle of the source observation (rotation histogram), degrees */
    int16_t min_level, max_level;   /* GetFeaturesInArea level window (its bCheckLevels rule is applied as is) */
    uint32_t flags;
} orbm_query;
#define ORBM_Q_VALID 1u      /* mbTrackInView && !isBad ... : query takes part */
#define ORBM_Q_STEREO 2u     /* apply the |u_right - mvuRight[idx]| <= radius gate where mvuRight[idx] > 0 */
#define ORBM_Q_HAS_OBS 4u    /* pMP->Observations() > 0: once matched, the keypoint is skipped by later queries */
#define ORBM_Q_RIGHT 8u      /* fisheye rig: search the right camera's grid (GetFeaturesInArea(..., bRight = true)) */
#define ORBM_Q_TWIN 16u      /* fisheye rig: right-camera query of the same map point as the previous query */

typedef struct orbm_search_params {
    int32_t mode;              /* ORBM_MODE_LOCAL_MAP, ORBM_MODE_BEST_ONLY or ORBM_MODE_INIT */
    int32_t th_dist;           /* TH_HIGH (100), or ORBdist of the relocalisation variant */
    float nn_ratio;            /* mfNNratio (LOCAL_MAP only) */
    int32_t check_orientation; /* mbCheckOrientation: rotation-histogram cull (BEST_ONLY only, as in the reference) */
    orbm_grid_params grid;
} orbm_search_params;
#define ORBM_MODE_LOCAL_MAP 0  /* SearchByProjection(Frame&, vector<MapPoint*>&, th, ...)  ORBmatcher.cc:59-255 (left camera) */
#define ORBM_MODE_BEST_ONLY 1  /* SearchByProjection(Frame&, const Frame&, th, bMono)      ORBmatcher.cc:2244-2509;
                                * SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) :2520-2652 with th_dist = ORBdist,
                                *   occupied0 = (mvpMapPoints[i] != NULL), every query ORBM_Q_HAS_OBS;
                                * SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th, ratioHamming) :593-824 with
                                *   check_orientation = 0, th_dist = floor(TH_LOW*ratioHamming), levels [L-1, L] */

#define ORBM_MODE_INIT 2       /* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)  ORBmatcher.cc:838-979:
                                *   one query per F1 keypoint (VALID iff octave == 0; u,v = vbPrevMatched[i1]; radius = windowSize;
                                *   min_level = max_level = 0; angle = F1 keypoint angle), th_dist = TH_LOW, nn_ratio, check_orientation.
                                *   A candidate is skipped while vMatchedDistance[i2] <= dist; an accepted match displaces the previous
                                *   holder of i2.  q_match = vnMatches12, kp_match = vnMatches21 (before the orientation cull).
                                *   Histogram factor HISTO_LENGTH/360 (this fork, :852).  cap_q <= 65534. */

/* Windowed projection search, results identical to the reference's serial loop (queries are resolved in index
 * order; a keypoint claimed by an earlier query with ORBM_Q_HAS_OBS is skipped by later ones).
 * Frame side: kps (x,y,octave,angle of mvKeysUn), desc, u_right (mvuRight, may be NULL = mono), occupied0 (may be NULL;
 * non-zero = mvpMapPoints[idx] already holds an observed point), CSR grid from orbm_grid_build.
 * Outputs: q_match[b][q] = matched keypoint index or -1; kp_match[b][idx] = index of the query whose map point
 * mvpMapPoints[idx] holds after the call, -1 = untouched by the call (mvpMapPoints[idx] keeps its value), -2 = claimed during the
 * call and then set to NULL by the orientation cull (ORBmatcher.cc:2499, :2637); nmatches[b] = the reference's return value.
 * d_work: scratch of orbm_search_workspace_bytes(batch, cap_q) bytes.
 * Form: the occupancy modes (LOCAL_MAP, BEST_ONLY) on single-camera frames with cap_q <= 2048 run as ONE workgroup per frame — window walk from an LDS copy of the
 * frame, the serial accept loop as parallel fixed-point rounds: the same result by construction (DESIGN.md stage-2 notes); every other call as per-query candidate
 * lists followed by a one-wave walk in query order. */
size_t orbm_search_workspace_bytes(int batch, int cap_q);
int orbm_search_by_projection(const orb_keypoint* d_kps, const uint8_t* d_desc, const float* d_u_right, const uint8_t* d_occupied0,
                              const int32_t* d_nkp, int count_stride, int cap_k,
                              const int32_t* d_grid_start, const int32_t* d_grid_idx,
                              const orbm_query* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int cap_q, int batch,
                              const orbm_search_params* params, int32_t* d_q_match, int32_t* d_kp_match, int32_t* d_nmatches,
                              void* d_work, void* stream);

/* Measurement facility (bench.py's roofline legs), the stage-2 counterpart of orbx_last_timing: while enabled, HIP events are recorded on the launch
 * stream around the kernels of orbm_grid_build and orbm_search_by_projection; orbm_last_timing synchronises on them and returns the device time of the
 * last call's kernels: ms[0] = grid build (or the fused undistort + grid launch), ms[1] = the projection search of the frames in one workgroup each (k_sbp_frame; calls it does not
 * cover — INIT mode, rigs, cap_q > 2048 —: candidate enumeration + Hamming), ms[2] = the gated launches behind it for flagged frames (those calls: the serial-order resolution).  The switch and the events are per calling thread: a thread times its own calls only, concurrent matcher
 * calls of other threads neither record into nor disturb them — so orbm_enable_timing, the timed calls and orbm_last_timing must come from the SAME thread
 * (another thread reads zeros), on one device (the events are re-made, and the last figures dropped, when the thread's current device changes). */
int orbm_enable_timing(int on);
int orbm_last_timing(float* ms3);

/* Map-point projection: the per-point loops that turn map points into orbm_query records, on the device.
 *   ORBM_PROJ_LOCAL_MAP   Tracking::SearchLocalPoints' projection loop (Tracking.cc:2874-2905) with Frame::isInFrustum (Frame.cc:571-665),
 *                         then the query loop of SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints) (ORBmatcher.cc:59-110);
 *                         search it with ORBM_MODE_LOCAL_MAP.
 *   ORBM_PROJ_LAST_FRAME  the projection of SearchByProjection(Frame&, const Frame&, th, bMono) (ORBmatcher.cc:2244-2331), bForward /
 *                         bBackward from tlc; search with ORBM_MODE_BEST_ONLY.
 *   ORBM_PROJ_RELOC       the projection of SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2520-2600), no
 *                         depth check; search with ORBM_MODE_BEST_ONLY, th_dist = ORBdist.
 * Single-camera pinhole frames only (Nleft == -1).  Each mode writes the same query fields and flags as integration/ORBmatcher_hip.cc builds
 * for that overload, with the same float / double rounding (DESIGN.md "Map-point projection"). */
typedef struct orbm_map_point {
    float pos[3];          /* GetWorldPos() */
    float normal[3];       /* GetNormal() (LOCAL_MAP) */
    float min_distance;    /* mfMinDistance: the kernel applies GetMinDistanceInvariance's 0.8f */
    float max_distance;    /* mfMaxDistance: 1.2f for GetMaxDistanceInvariance; PredictScale's ratio uses it as is */
    float angle;           /* source keypoint angle: LastFrame.mvKeysUn[i] (LAST_FRAME), pKF->mvKeysUn[i] (RELOC) */
    int32_t octave;        /* source keypoint octave, LastFrame.mvKeys[i] (LAST_FRAME); in [0, nlevels) */
    int32_t desc_row;      /* row of GetDescriptor() in the descriptor slab; rows outside [0, n_desc_rows) gather zeros */
    uint32_t flags;        /* ORBM_MP_* */
} orbm_map_point;          /* 48 B */
#define ORBM_MP_VALID 1u     /* the slot holds a point: LOCAL_MAP list entry; LAST_FRAME mvpMapPoints[i] && !mvbOutlier[i];
                              * RELOC vpMPs[i] && !sAlreadyFound.count(pMP) */
#define ORBM_MP_BAD 2u       /* isBad() (LOCAL_MAP, RELOC; the motion model does not test it) */
#define ORBM_MP_SEEN 4u      /* LOCAL_MAP: mnLastFrameSeen == the frame's mnId: isInFrustum is skipped, the track entry is read as it stands */
#define ORBM_MP_HAS_OBS 8u   /* Observations() > 0 -> ORBM_Q_HAS_OBS (LOCAL_MAP, LAST_FRAME; RELOC queries always carry it) */

/* The MapPoint members isInFrustum writes (LOCAL_MAP; in/out, one per map-point slot). */
typedef struct orbm_track {
    float proj_x, proj_y, proj_xr;   /* mTrackProjX, mTrackProjY, mTrackProjXR */
    float depth;                     /* mTrackDepth */
    float view_cos;                  /* mTrackViewCos */
    int32_t level;                   /* mnTrackScaleLevel, in [0, nlevels) */
    int32_t in_view;                 /* mbTrackInView */
    int32_t reserved;
} orbm_track;                        /* 32 B */

/* Per frame: pose of the current frame and, for LAST_FRAME, of the last frame (row-major rotations). */
typedef struct orbm_project_frame {
    float Rcw[9], tcw[3];   /* mTcw */
    float Ow[3];            /* mOw = -Rcw^T tcw (also the motion model's twc) */
    float Rlw[9], tlw[3];   /* LastFrame.mTcw (LAST_FRAME) */
    float bounds[4];        /* mnMinX, mnMaxX, mnMinY, mnMaxY */
} orbm_project_frame;       /* 124 B */

typedef struct orbm_project_params {
    int32_t mode;              /* ORBM_PROJ_* */
    int32_t camera_type;       /* ORBM_CAM_PINHOLE (KannalaBrandt8 is not supported) */
    int32_t nleft;             /* -1 (fisheye rigs are not supported) */
    float fx, fy, cx, cy;      /* Pinhole mvParameters */
    float mbf, mb;
    int32_t mono;              /* bMono (LAST_FRAME) */
    float th;                  /* the search's th */
    float view_cos_limit;      /* isInFrustum's viewingCosLimit (Tracking passes 0.5) */
    int32_t far_points;        /* bFarPoints (LOCAL_MAP) */
    float th_far_points;       /* thFarPoints */
    int32_t nlevels;           /* mnScaleLevels, 1..16 */
    int32_t n_desc_rows;       /* rows in the descriptor slab */
    float scale_factors[16];   /* mvScaleFactors */
    float level_thresholds[16];/* [0, nlevels-1): orbm_predict_scale_thresholds(mfLogScaleFactor, nlevels, .) */
} orbm_project_params;
#define ORBM_PROJ_LOCAL_MAP 0
#define ORBM_PROJ_LAST_FRAME 1
#define ORBM_PROJ_RELOC 2
#define ORBM_CAM_PINHOLE 0

/* MapPoint::PredictScale (MapPoint.cc:578-610) as a step function of the float ratio mfMaxDistance / dist: thresholds[k-1] = the smallest
 * positive float ratio whose level (ceil(std::log(ratio) / log_scale_factor) with the host's logf, clamped to [0, nlevels)) is >= k, for
 * k = 1..nlevels-1.  The kernel's level is the number of thresholds <= ratio: the host formula for every finite ratio as long as the host
 * logf is monotone (the tests sweep +-2048 ulps around every threshold).  ORB_E_INVALID unless log_scale_factor > 0 and 1 <= nlevels <= 16.
 * Host only, synchronous. */
int orbm_predict_scale_thresholds(float log_scale_factor, int nlevels, float* thresholds);

/* Projects the map-point lists of `batch` frames and writes the compacted queries straight into the buffers orbm_search_by_projection reads.
 * Frame b: records d_mp[b*cap_mp .. + min(d_nmp[b], cap_mp)), walked in list order; d_mp_desc = descriptor slab [n_desc_rows][32] shared by all
 * frames (16-byte aligned); d_frames[b]; d_track[b*cap_mp + i] (LOCAL_MAP only, in/out: a record isInFrustum does not visit keeps its entry;
 * may be NULL in the other modes).
 * Outputs, in list order (stable compaction): d_queries[b*cap_q + j], d_qdesc[(b*cap_q + j)*32] (16-byte aligned), d_q_src[b*cap_q + j] = the
 * record index of query j; d_nq[b] = min(d_n_required[b], cap_q); d_n_required[b] = the number of queries the reference hands to the search
 * (overflow is reported here, never silently); d_n_in_view[b] = nToMatch (LOCAL_MAP; other modes: the number of projected points).  LOCAL_MAP
 * with nToMatch == 0 writes nq = n_required = 0 (the reference does not call the search).  Entries past nq are unspecified.
 * Asynchronous on `stream`, no host synchronisation.  ORB_E_INVALID for null pointers, a bad mode, nlevels outside 1..16, cap_q < 1,
 * cap_mp < 1, a non-pinhole camera or a rig (nleft != -1), misaligned descriptor slabs. */
int orbm_project_map_points(const orbm_map_point* d_mp, const int32_t* d_nmp, int cap_mp, const uint8_t* d_mp_desc,
                            const orbm_project_frame* d_frames, int batch, const orbm_project_params* params, orbm_track* d_track,
                            orbm_query* d_queries, uint8_t* d_qdesc, int32_t* d_nq, int32_t* d_q_src, int32_t* d_n_required,
                            int32_t* d_n_in_view, int cap_q, void* stream);

/* Map-point refresh: the two MapPoint members the reference recomputes after every change to a point's observations or position, written
 * straight into the orbm_map_point records and the descriptor slab orbm_project_map_points reads.
 *   ORBM_REFRESH_DESCRIPTOR     MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:372-460): all pairwise Hamming distances of the observed
 *                               descriptors, the median of every row, the FIRST row with the least median wins.
 *   ORBM_REFRESH_NORMAL_DEPTH   MapPoint::UpdateNormalAndDepth (MapPoint.cc:485-558): mean unit viewing ray, mfMaxDistance, mfMinDistance.
 * The observations of all points form one CSR: point p owns d_obs[d_obs_start[p] .. d_obs_start[p+1]).  ONE record per (key frame, camera)
 * descriptor, in the iteration order of mObservations and, inside one entry, left before right (MapPoint.cc:393-410, 511-529): the order fixes
 * the tie-break of the descriptor choice and the order of the float sum of the normal. */
typedef struct orbm_observation {
    int32_t kf;            /* index of the key frame in d_kf */
    int32_t desc_row;      /* row of pKF->mDescriptors.row(leftIndex / rightIndex) in the key-frame descriptor slab d_kf_desc */
    uint32_t flags;        /* ORBM_OBS_* */
} orbm_observation;        /* 12 B */
#define ORBM_OBS_RIGHT 1u    /* the record is the entry's rightIndex: GetRightCameraCenter() instead of GetCameraCenter() (MapPoint.cc:524) */
#define ORBM_OBS_KF_BAD 2u   /* pKF->isBad(): skipped by the descriptor choice (MapPoint.cc:397), NOT by the normal (:511-529 do not test it) */

typedef struct orbm_keyframe_center {
    float left[3];         /* GetCameraCenter() */
    float right[3];        /* GetRightCameraCenter() (read only by ORBM_OBS_RIGHT records) */
} orbm_keyframe_center;    /* 24 B */

typedef struct orbm_refresh_point {
    int32_t ref_kf;        /* index of mpRefKF in d_kf */
    int32_t level;         /* octave of the reference key point, chosen by the host: the NLeft branch of MapPoint.cc:528-537, including the
                            * default (0, 0) entry std::map::operator[] makes when mpRefKF is not among the observations */
} orbm_refresh_point;      /* 8 B */

typedef struct orbm_refresh_params {
    uint32_t what;             /* ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH (the reference calls the two separately in places) */
    int32_t nlevels;           /* mnScaleLevels of the reference key frame, 1..16 */
    float scale_factors[16];   /* mvScaleFactors */
} orbm_refresh_params;         /* 72 B */
#define ORBM_REFRESH_DESCRIPTOR 1u
#define ORBM_REFRESH_NORMAL_DEPTH 2u
/* d_status bits */
#define ORBM_REFRESHED_DESCRIPTOR 1u     /* a representative descriptor was chosen (d_best_obs >= 0) */
#define ORBM_REFRESHED_NORMAL_DEPTH 2u   /* normal, min_distance and max_distance were written */
#define ORBM_REFRESH_OVERFLOW 4u         /* more than ORBM_REFRESH_MAX_OBS usable records: the point was left completely untouched */
#define ORBM_REFRESH_BAD_RECORD 8u       /* a record (or the point's ref_kf / level) was out of range and treated as absent */
/* The most usable observation records (in range, key frame not bad) one point may have. */
#define ORBM_REFRESH_MAX_OBS 1024

/* Refreshes the selected points: d_sel[0 .. n_sel) are indices into d_mp (NULL: all n_mp points, n_sel is ignored; indices outside [0, n_mp)
 * are skipped; a point listed twice is undefined).  d_best_obs and d_status have n_mp entries; only the entries of selected points are written,
 * and every other byte of d_mp / d_mp_desc stays as it is.  Per selected point p:
 *  - ORBM_MP_BAD set, ORBM_MP_VALID clear or no observation record: nothing is written, d_best_obs[p] = -1, d_status[p] = 0.
 *  - A record whose kf is outside [0, n_kf) or whose desc_row is outside [0, n_kf_desc_rows) is treated as absent in both halves (it still counts
 *    in d_best_obs indexing) and the point is flagged ORBM_REFRESH_BAD_RECORD.
 *  - More than ORBM_REFRESH_MAX_OBS usable records (in range and not ORBM_OBS_KF_BAD): the point is left untouched in both halves,
 *    d_best_obs[p] = -1, ORBM_REFRESH_OVERFLOW.  Nothing is ever truncated silently.
 *  - DESCRIPTOR: over the N usable records, Distances[i][i] = 0, median of row i = element int(0.5*(N-1)) of the sorted row (the lower median),
 *    winner = the first row with the least median.  Its 32 bytes go to d_mp_desc[d_mp[p].desc_row] (a desc_row outside [0, n_desc_rows) copies
 *    nothing) and d_best_obs[p] = its index in the point's observation list, counting every record.  N == 0: the descriptor is left alone,
 *    d_best_obs[p] = -1.  Without ORBM_REFRESH_DESCRIPTOR d_best_obs[p] = -1.
 *  - NORMAL_DEPTH: over the n in-range records (bad key frames included) in record order, normal = (sum of (pos - Ow) / cv::norm(pos - Ow)) / n;
 *    dist = cv::norm(pos - d_kf[ref_kf].left); max_distance = dist * scale_factors[level]; min_distance = max_distance / scale_factors[nlevels-1].
 *    Float rounding as in orbm_project_map_points (DESIGN.md "Map-point refresh").  ref_kf outside [0, n_kf) or level outside [0, nlevels):
 *    this half is skipped and the point flagged ORBM_REFRESH_BAD_RECORD.
 * Both descriptor slabs are 16-byte aligned.  Asynchronous on `stream`, no host synchronisation, graph-capturable.  ORB_E_INVALID for null
 * pointers (d_sel excepted), negative counts, nlevels outside 1..16, `what` zero or with unknown bits, misaligned slabs; n_mp == 0 or
 * (d_sel && n_sel == 0) is a successful no-op. */
int orbm_refresh_map_points(orbm_map_point* d_mp, int n_mp, uint8_t* d_mp_desc, int n_desc_rows, const int32_t* d_sel, int n_sel,
                            const int32_t* d_obs_start, const orbm_observation* d_obs, const orbm_refresh_point* d_ref,
                            const orbm_keyframe_center* d_kf, int n_kf, const uint8_t* d_kf_desc, int n_kf_desc_rows,
                            const orbm_refresh_params* params, int32_t* d_best_obs, uint32_t* d_status, void* stream);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:2008-2220) = orbm_fuse in both directions (each map point
 * keeps its own best candidate in [L-1, L] with bestDist <= TH_HIGH and no chi2 gate: vnMatch1 / vnMatch2, :2044-2119 and :2122-2201) followed by
 * this agreement pass (:2203-2219): out12[b][i1] = idx2 iff match12[b][i1] == idx2 and match21[b][idx2] == i1, else -1; nfound[b] = the return value. */
int orbm_mutual_matches(const int32_t* d_match12, const int32_t* d_match21, const int32_t* d_n1, const int32_t* d_n2, int cap1, int cap2,
                        int batch, int32_t* d_out12, int32_t* d_nfound, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Sim3Solver (reference src/Sim3Solver.cc, include/Sim3Solver.h): the RANSAC Horn alignment between SearchByBoW(KF, KF) and the Sim3
 * projection search of LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:640-830), for a batch of independent problems.
 * One problem = one Sim3Solver object.  Every hypothesis of a problem (one per sample triple, max_its of them) is evaluated: ComputeSim3
 * (:316-427), CheckInliers (:430-454) over all correspondences, then the reference's serial pick (:170-218).  The float cv::Mat / libm /
 * cv::eigen / cv::Rodrigues steps follow rules R4 and R5: parity against a real OpenCV build is unpinned for them.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct orbm_sim3_camera {
    int32_t model;         /* ORBM_SIM3_CAM_* */
    float p[8];            /* fx, fy, cx, cy, k0..k3 (mvParameters; a pinhole reads the first four) */
} orbm_sim3_camera;        /* 36 B */
#define ORBM_SIM3_CAM_PINHOLE 0   /* Pinhole::project(cv::Point3f): fx * x / z + cx in float */
#define ORBM_SIM3_CAM_KB8 1       /* KannalaBrandt8::project(cv::Point3f) (KannalaBrandt8.cpp:28-42, rule R4) */

/* One row per correspondence that survives the constructor's filters (:73-91), in the constructor's order. */
typedef struct orbm_sim3_corr {
    float Xw1[3];          /* pMP1->GetWorldPos() */
    float Xw2[3];          /* pMP2->GetWorldPos() */
    float max_err1;        /* (float)(size_t)(9.210 * sigmaSquare1): mvnMaxError1 is a vector<size_t>, the product is truncated (:99) */
    float max_err2;        /* the same of sigmaSquare2 (:100) */
    int32_t index1;        /* mvnIndices1[i] = i1: where vbInliers receives this correspondence */
} orbm_sim3_corr;          /* 36 B */

typedef struct orbm_sim3_problem {
    float Rcw1[9], tcw1[3];        /* pKF1->GetRotation() / GetTranslation(), row-major */
    float Rcw2[9], tcw2[3];        /* pKF2's */
    orbm_sim3_camera cam1, cam2;   /* pKF1->mpCamera, pKF2->mpCamera */
    int32_t fix_scale;             /* mbFixScale */
    int32_t min_inliers;           /* mRansacMinInliers */
    int32_t max_its;               /* mRansacMaxIts after SetRansacParameters' clamp (orbm_sim3_ransac_iterations) */
    int32_t n1;                    /* mN1 = vpMatched12.size(): the length of vbInliers */
} orbm_sim3_problem;               /* 184 B */

typedef struct orbm_sim3_hyp {
    float R12[9], t12[3], s12;     /* mR12i (row-major), mt12i, ms12i of one hypothesis */
} orbm_sim3_hyp;                   /* 52 B */

typedef struct orbm_sim3_result {
    int32_t iterations;    /* mnIterations when find() / an unbounded iterate() returns */
    int32_t converged;     /* 1: a hypothesis with more than min_inliers inliers stopped the loop (bConverge) */
    int32_t no_more;       /* bNoMore */
    int32_t best_iter;     /* the hypothesis mBest* hold at that moment (-1: none was evaluated) */
    int32_t n_inliers;     /* mnBestInliers */
    float R12[9], t12[3], s12;   /* mBestRotation, mBestTranslation, mBestScale */
    float T12[16];         /* mBestT12, row-major 4x4 */
    uint32_t status;       /* ORBM_SIM3_* bits */
} orbm_sim3_result;        /* 140 B */
#define ORBM_SIM3_BAD_SAMPLE 1u    /* a triple among the problem's max_its was out of [0, N) or not distinct: that hypothesis is NaN with 0 inliers */
#define ORBM_SIM3_ITS_CLAMPED 2u   /* max_its > cap_its: cap_its hypotheses were evaluated */
#define ORBM_SIM3_N_CLAMPED 4u     /* d_n > cap_n (or < 0): cap_n (0) correspondences were used */
#define ORBM_SIM3_BAD_INDEX 8u     /* an inlier's index1 was outside [0, min(n1, cap_n1)): not scattered */
/* The most correspondences one problem may have (they are staged in the workgroup's LDS). */
#define ORBM_SIM3_MAX_N 3392

/* SetRansacParameters' iteration count (:137-147): float epsilon = (float)min_inliers / n; min_inliers == n -> 1, else
 * ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in double converted to int as x86-64 does (NaN / out of range -> INT_MIN); the result is
 * max(1, min(that, max_its)).  Host only. */
int orbm_sim3_ransac_iterations(double probability, int min_inliers, int max_its, int n);

/* Bytes of d_work for orbm_sim3_solve (mT12i and mT21i of every hypothesis). */
size_t orbm_sim3_workspace_bytes(int batch, int cap_n, int cap_its);

/* Solves `batch` problems.  Problem b: d_problems[b]; correspondences d_corr[b*cap_n .. + d_n[b]); sample triples
 * d_samples[(b*cap_its + h)*3 .. +3) for hypothesis h < max_its: indices into the problem's correspondences, what mvAllIndices yields after
 * the three RandomInt draws with swap-with-back removal (:175-189).  The caller owns the randomness (the reference draws from the global
 * rand()).
 * Outputs: d_hyp[b*cap_its + h], d_hyp_count[b*cap_its + h] = mnInliersi, d_hyp_mask[(b*cap_its + h)*words + w] = mvbInliersi as bits
 * (correspondence i = bit i & 63 of word i >> 6, words = (cap_n + 63) / 64, bits past N are 0), all for h < max_its (entries past that are
 * left alone); d_result[b]; d_inliers[b*cap_n1 + i1] = vbInliers (bytes, all cap_n1 of them written: zero unless converged).
 * N < min_inliers (:158-162): no_more = 1, iterations = 0, best_iter = -1, the hypothesis outputs of the problem are not written.
 * Selection: running best with >= (a later tie replaces the best), stop at the first hypothesis with more than min_inliers inliers, else
 * run to max_its (then no_more).  Degenerate triples (coincident / collinear points, norm(vec) == 0, den == 0) give NaN / Inf transforms as
 * in the reference: every comparison is false, 0 inliers.
 * Asynchronous on `stream`, no host synchronisation, graph-capturable, deterministic.  ORB_E_INVALID for null pointers, cap_its < 1,
 * cap_n < 1, cap_n1 < 1, batch < 0; ORB_E_CAPACITY for cap_n > ORBM_SIM3_MAX_N.  A problem whose min_inliers < 3 is rejected on the host
 * side by the wrappers (ORB_E_INVALID); on the device it is evaluated as given. */
int orbm_sim3_solve(const orbm_sim3_problem* d_problems, const orbm_sim3_corr* d_corr, const int32_t* d_n, int cap_n,
                    const int32_t* d_samples, int cap_its, int batch, orbm_sim3_hyp* d_hyp, int32_t* d_hyp_count, uint64_t* d_hyp_mask,
                    orbm_sim3_result* d_result, uint8_t* d_inliers, int cap_n1, void* d_work, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * TwoViewReconstruction (reference src/TwoViewReconstruction.cc:51-1013): TwoViewReconstruction::Reconstruct on the Pinhole path, for a batch
 * of independent frame pairs.  Normalize, FindHomography and FindFundamental over the caller's eight-point sets, CheckHomography /
 * CheckFundamental of every hypothesis against all matches, the best of each model and the choice between them (`SH+SF == 0`, `RH > 0.50`),
 * then ReconstructH / ReconstructF: the 8 / 4 motion hypotheses, CheckRT of each over the inliers and the reference's accept logic.
 * One problem = one frame pair.  The float cv::Mat / cv::SVDecomp / Mat::inv steps follow rule R7: parity against a
 * real OpenCV build is unpinned for them.  The fisheye pre-step of KannalaBrandt8::ReconstructWithTwoViews is not part of this.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct orbm_tvr_problem {
    float fx, fy, cx, cy;      /* mK */
    float sigma;               /* mSigma (the reference constructs with 1.0) */
    int32_t max_its;           /* mMaxIterations (200) */
    int32_t n_keys1;           /* vKeys1.size() = vMatches12.size(): Normalize runs over all of them, matched or not */
    int32_t n_keys2;           /* vKeys2.size() */
    float min_parallax;        /* minParallax of ReconstructH / ReconstructF (1.0) */
    int32_t min_triangulated;  /* minTriangulated (50) */
} orbm_tvr_problem;            /* 40 B */

typedef struct orbm_tvr_result {
    float R21[9], t21[3];          /* row-major; zero unless ok (the reference leaves R21 / t21 empty) */
    float SH, SF;                  /* the best score of each model (0: no hypothesis scored above 0) */
    int32_t best_it_H, best_it_F;  /* the iteration that holds it: the first of the greatest (-1 with a score of 0) */
    int32_t n_matches;             /* N = mvMatches12.size() */
    int32_t n_inliers;             /* set bits of the chosen model's best mask (ReconstructH / ReconstructF's N) */
    int32_t model;                 /* 0: H (RH > 0.50), 1: F, -1: SH + SF == 0 (Reconstruct returns false) */
    int32_t hypothesis;            /* F: the first motion with maxGood, in the order (R1,t) (R2,t) (R1,-t) (R2,-t); H: bestSolutionIdx; -1: none */
    int32_t n_good;                /* maxGood / bestGood */
    float parallax;                /* that hypothesis's parallax in degrees (H: bestParallax, -1 while no hypothesis has a good point) */
    int32_t ok;                    /* Reconstruct's return value */
    uint32_t status;               /* ORBM_TVR_* bits */
} orbm_tvr_result;                 /* 96 B */
#define ORBM_TVR_TOO_FEW 1u        /* fewer than 8 matches (the reference would draw from an empty range): ok = 0, no hypothesis output is written */
#define ORBM_TVR_BAD_SAMPLE 2u     /* a set among the problem's max_its had an index outside [0, N) or a repeated one: NaN model, NaN score, empty mask */
#define ORBM_TVR_BAD_INDEX 4u      /* a matches12 entry >= n_keys2: treated as unmatched */
#define ORBM_TVR_ITS_CLAMPED 8u    /* max_its > cap_its: cap_its hypotheses per model were evaluated */
#define ORBM_TVR_N_CLAMPED 16u     /* n_keys1 or n_keys2 outside [0, cap_k]: clamped */
#define ORBM_TVR_NAN_PARALLAX 32u  /* a NaN cosine reached vCosParallax (the reference's sort is then undefined): ok = 0 */

/* Bytes of d_work for orbm_two_view_reconstruct (the compacted matches, the normalisation matrices, H12i of every hypothesis, the cosines). */
size_t orbm_two_view_workspace_bytes(int batch, int cap_k, int cap_its);

/* Runs `batch` problems.  Problem b: d_problems[b]; keys d_keys1[b*cap_k .. + n_keys1), d_keys2[b*cap_k .. + n_keys2) (the undistorted
 * records of orbf_undistort_keypoints; x and y are read); d_matches12[b*cap_k + i1] = i2 or a negative value (what ORBM_MODE_INIT writes);
 * d_sets[(b*cap_its + it)*8 .. +8) = mvSets[it] (:100-127), indices into the matches in their order of appearance.  The caller owns the
 * randomness (the reference draws from the global rand()).
 * Outputs, for model m (0 = H, 1 = F) and it < max_its (entries past that are left alone): d_score[(b*2 + m)*cap_its + it] = currentScore;
 * d_model[((b*2 + m)*cap_its + it)*9 .. +9) = H21i / F21i row-major; d_mask[((b*2 + m)*cap_its + it)*words + w] = vbCurrentInliers as bits
 * (match i = bit i & 63 of word i >> 6, words = (cap_k + 63) / 64, bits past N are 0); d_result[b]; d_p3d[(b*cap_k + i1)*3 .. +3) = vP3D and
 * d_triangulated[b*cap_k + i1] = vbTriangulated of the winning hypothesis (all cap_k entries written: zero unless ok and key i1 has an
 * accepted point; a point with cosParallax >= 0.99998 is written and counted but not flagged, :972-977).
 * A rank-deficient set gives whatever the arithmetic gives, NaN included: a NaN score is never picked (every comparison is false).
 * Asynchronous on `stream`, no host synchronisation, no allocation, graph-capturable, deterministic.  ORB_E_INVALID for null pointers,
 * cap_k < 1, cap_its < 1, batch < 0; ORB_E_CAPACITY for batch > 65535. */
int orbm_two_view_reconstruct(const orbm_tvr_problem* d_problems, const orb_keypoint* d_keys1, const orb_keypoint* d_keys2, int cap_k,
                              const int32_t* d_matches12, const int32_t* d_sets, int cap_its, int batch, float* d_score, float* d_model,
                              uint64_t* d_mask, orbm_tvr_result* d_result, float* d_p3d, uint8_t* d_triangulated, void* d_work, void* stream);

/* Fisheye-rig (F.Nleft != -1) variants.  Keypoints / descriptors are the concatenation [mvKeys | mvKeysRight] like the reference's
 * N-sized arrays; d_nleft[b] = Nleft.  The grid has 2 x 64 x 48 cells per frame (second half = mGridRight, entries are global indices):
 * grid_start [batch][2*64*48+1].  d_kp_link[b][i] = global index of keypoint i's stereo partner (mvLeftToRightMatch[i] + Nleft, or
 * mvRightToLeftMatch[i - Nleft]) or -1; may be NULL.  A map point seen by both cameras contributes two consecutive queries: the left
 * one, then the right one flagged ORBM_Q_RIGHT | ORBM_Q_TWIN.  Reproduced quirks:
 *   ORBM_MODE_LOCAL_MAP (ORBmatcher.cc:59-258): the `continue` of the left ratio test (:166-167) also skips the right camera; an
 *     accepted match is copied to the stereo partner and counted twice (:172-176, :239-243); u_right gating does not apply to rigs;
 *   ORBM_MODE_BEST_ONLY (:2244-2509): an empty left window (`if(vIndices2.empty()) continue;` :2332) or an invalid left query skips
 *     the right camera of that map point. */
int orbm_grid_build_rig(const orb_keypoint* d_kps, const int32_t* d_nkp, const int32_t* d_nleft, int count_stride, int cap_k, int batch,
                        const orbm_grid_params* gp, int32_t* d_grid_start, int32_t* d_grid_idx, void* stream);
int orbm_search_by_projection_rig(const orb_keypoint* d_kps, const uint8_t* d_desc, const uint8_t* d_occupied0, const int32_t* d_kp_link,
                                  const int32_t* d_nkp, int count_stride, int cap_k,
                                  const int32_t* d_grid_start, const int32_t* d_grid_idx,
                                  const orbm_query* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int cap_q, int batch,
                                  const orbm_search_params* params, int32_t* d_q_match, int32_t* d_kp_match, int32_t* d_nmatches,
                                  void* d_work, void* stream);

/* ORBmatcher::Fuse — the search half of both overloads: per projected map point the best keypoint of the key frame.
 *   chi2_gate = 1: Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight)           ORBmatcher.cc:1630-1882 (search :1770-1830)
 *   chi2_gate = 0: Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint)      ORBmatcher.cc:1884-2006 (search :1960-1985)
 * A query = what the reference computes per map point before KeyFrame::GetFeaturesInArea (KeyFrame.cc:810-854): u,v = uv,
 * u_right = uv.x - bf*invz, radius = th*mvScaleFactors[nPredictedLevel], min_level = nPredictedLevel-1, max_level = nPredictedLevel,
 * flags = ORBM_Q_VALID iff the point passed the frustum / distance / normal gates (:1700-1765).  Queries are independent (several map
 * points may select the same keypoint; the Replace / AddObservation mutations stay in the host adapter, applied in index order).
 * Outputs: q_match[b][q] = bestIdx if bestDist <= th_dist else -1; q_dist[b][q] = bestDist (256: empty window); nfused[b]. */
typedef struct orbm_fuse_params {
    int32_t th_dist;              /* TH_LOW */
    int32_t chi2_gate;
    orbm_grid_params grid;
    float inv_level_sigma2[16];   /* pKF->mvInvLevelSigma2 (chi2_gate only) */
} orbm_fuse_params;
int orbm_fuse(const orb_keypoint* d_kps, const uint8_t* d_desc, const float* d_u_right, const int32_t* d_nkp, int count_stride, int cap_k,
              const int32_t* d_grid_start, const int32_t* d_grid_idx, const orbm_query* d_queries, const uint8_t* d_qdesc,
              const int32_t* d_nq, int cap_q, int batch, const orbm_fuse_params* params, int32_t* d_q_match, int32_t* d_q_dist,
              int32_t* d_nfused, void* stream);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:1138-1428; call sites
 * LocalMapping.cc:628, Tracking.cc:3812) for pinhole key frames without a second camera.  Both FeatureVectors as CSR like
 * orbm_bow_side; has_mp[i] != 0 where pKF->GetMapPoint(i) != NULL; u_right = mvuRight (NULL = monocular).
 * Per pair: the fundamental matrix Pinhole::epipolarConstrain builds (Pinhole.cpp:157-160, row-major F12 = K1^-T [t12]x R12 K2^-1;
 * the adapter evaluates that cv::Mat expression once per pair), the epipole ep (ORBmatcher.cc:1152) and pKF2's mvLevelSigma2 /
 * mvScaleFactors.  Output match12[b][i1] = idx2 or -1 (vMatches12 after the orientation cull), nmatches[b]. */
typedef struct orbm_tri_side {
    const orb_keypoint* kps;      /* [batch][cap_f]  mvKeysUn */
    const uint8_t* desc;          /* [batch][cap_f][32] */
    const float* u_right;         /* [batch][cap_f] or NULL */
    const uint8_t* has_mp;        /* [batch][cap_f] */
    const int32_t* node_id;       /* [batch][cap_nodes] ascending */
    const int32_t* node_start;    /* [batch][cap_nodes+1] */
    const int32_t* feat_idx;      /* [batch][cap_f] */
    const int32_t* n_nodes;       /* [batch] */
    int32_t cap_f, cap_nodes;
} orbm_tri_side;
typedef struct orbm_tri_pair {
    float F12[9];
    float ep[2];
    float level_sigma2_2[16];     /* pKF2->mvLevelSigma2 */
    float scale_factors_2[16];    /* pKF2->mvScaleFactors */
    float reserved;
} orbm_tri_pair;
int orbm_search_for_triangulation(const orbm_tri_side* kf1, const orbm_tri_side* kf2, const orbm_tri_pair* d_pairs, int batch,
                                  int only_stereo, int coarse, int check_orientation, int32_t* d_match12, int32_t* d_nmatches,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * New map points: the loop of LocalMapping::CreateNewMapPoints behind SearchForTriangulation (LocalMapping.cc:651-904) for key frames with one
 * camera (NLeft == -1, no mpCamera2): parallax test, linear triangulation (cv::SVD of a 4x4) or stereo unprojection, depth-sign, reprojection
 * and scale-consistency gates, then the bookkeeping of `new MapPoint` / AddObservation / AddMapPoint as index lists.  Each side is a pinhole
 * camera (monocular, stereo, RGB-D) or a single KannalaBrandt8 camera.  bStereo of a feature is u_right[i] >= 0 as in the reference (:660, :669);
 * the reference never sets it for a KannalaBrandt8 key frame, whose side therefore passes u_right = NULL.  Fisheye rigs (mpCamera2, the four
 * pose combinations :673-743) are not supported: the wrappers refuse them with ORB_E_INVALID.  The float cv::Mat / libm / cv::SVD steps follow
 * rules R4 and R6: parity against a real OpenCV build is unpinned for them.
 * ------------------------------------------------------------------------------------------------------- */
#define ORBM_CAM_KB8 1        /* KannalaBrandt8::unproject / project(cv::Point3f) (KannalaBrandt8.cpp:101-124, 28-42, rule R4) */

/* One key frame of a pair, evaluated by the host once per pair (row-major rotation). */
typedef struct orbm_newpt_camera {
    float Rcw[9], tcw[3];      /* GetRotation(), GetTranslation(); Tcw = [Rcw | tcw], Rwc = the exact transpose of Rcw */
    float Ow[3];               /* GetCameraCenter() */
    int32_t camera_type;       /* ORBM_CAM_PINHOLE or ORBM_CAM_KB8 */
    float k[8];                /* fx, fy, cx, cy, k1..k4: mvParameters; k[0..3] are also the key frame's fx, fy, cx, cy (:554-557) */
    float invfx, invfy;        /* KeyFrame::invfx, invfy (UnprojectStereo) */
    float mb, mbf;
    float level_sigma2[16];    /* mvLevelSigma2 */
    float scale_factors[16];   /* mvScaleFactors */
} orbm_newpt_camera;           /* 240 B */

typedef struct orbm_newpt_pair {
    orbm_newpt_camera cam1, cam2;   /* mpCurrentKeyFrame, pKF2 */
    float ratio_factor;        /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:562) */
    int32_t far_points;        /* mbFarPoints */
    float th_far_points;       /* mThFarPoints */
    int32_t kf1, kf2;          /* the key frames' indices in orbm_keyframe_center order, for the observation records */
    int32_t obs_kf2_first;     /* 1: mObservations (a std::map<KeyFrame*, ...>) iterates pKF2 before pKF1; the host owns that allocator-dependent fact */
    int32_t desc_row0_1, desc_row0_2;   /* the row of feature 0 of each key frame in the key-frame descriptor slab orbm_refresh_map_points reads */
} orbm_newpt_pair;             /* 512 B */

/* The per-feature arrays of one side, [batch][cap_f] like orbm_tri_side (kps, u_right and has_mp may be the very same buffers). */
typedef struct orbm_newpt_side {
    const orb_keypoint* kps;      /* mvKeysUn */
    const orb_keypoint* kps_raw;  /* mvKeys, read by UnprojectStereo (KeyFrame.cc:866-867); NULL = the same as kps */
    const float* u_right;         /* mvuRight, or NULL = monocular */
    const float* depth;           /* mvDepth; needed when u_right is given */
    const int32_t* n;             /* [batch] the key frame's N; clamped to [0, cap_f] */
    uint8_t* has_mp;              /* in/out or NULL: set to 1 where a created point was stored */
    int32_t cap_f, reserved;
} orbm_newpt_side;

typedef struct orbm_new_point {
    float pos[3];              /* x3D */
    int32_t idx1, idx2;        /* the features of pKF1 / pKF2 */
    int32_t how;               /* ORBM_NEWPT_CREATED_* */
} orbm_new_point;              /* 24 B */

/* d_status: the reference's exit for feature i1 of KF1 */
#define ORBM_NEWPT_NO_MATCH 0              /* match12[i1] == -1 */
#define ORBM_NEWPT_CREATED_TRIANGULATED 1  /* :765-786 and every gate passed */
#define ORBM_NEWPT_CREATED_STEREO1 2       /* mpCurrentKeyFrame->UnprojectStereo(idx1) (:787-790) */
#define ORBM_NEWPT_CREATED_STEREO2 3       /* pKF2->UnprojectStereo(idx2) (:791-794) */
#define ORBM_NEWPT_LOW_PARALLAX 4          /* the final `else continue` (:795-798) */
#define ORBM_NEWPT_W_ZERO 5                /* x3D.at<float>(3) == 0 (:780) */
#define ORBM_NEWPT_EMPTY_STEREO 6          /* UnprojectStereo with z <= 0 returned an empty cv::Mat (:802) */
#define ORBM_NEWPT_BEHIND_1 7              /* z1 <= 0 (:805) */
#define ORBM_NEWPT_BEHIND_2 8              /* z2 <= 0 (:809) */
#define ORBM_NEWPT_REPROJ_1 9              /* :824 / :836 */
#define ORBM_NEWPT_REPROJ_2 10             /* :850 / :861 */
#define ORBM_NEWPT_ZERO_DIST 11            /* :872 */
#define ORBM_NEWPT_FAR 12                  /* :875 */
#define ORBM_NEWPT_SCALE 13                /* :881 */
#define ORBM_NEWPT_BAD_INDEX 14            /* match12[i1] outside [0, n2) (and not -1), i1 >= n1, or a key point octave outside [0, 16): never read through */
/* d_pair_flags bits */
#define ORBM_NEWPT_PAIR_BAD_INDEX 1u       /* a feature of the pair has ORBM_NEWPT_BAD_INDEX */
#define ORBM_NEWPT_PAIR_OVERFLOW 2u        /* d_nrequired > cap_new */
#define ORBM_NEWPT_PAIR_BAD_CAMERA 4u      /* a camera_type outside the two: nothing was read or created (every status ORBM_NEWPT_NO_MATCH) */

/* One launch for `batch` independent pairs; pair b reads d_pairs[b], the sides' rows b and d_match12[b*kf1->cap_f + i1] exactly as
 * orbm_search_for_triangulation writes it (all cap_f entries).  Outputs:
 *   d_status[b*cap_f1 + i1]      ORBM_NEWPT_* of every feature of KF1 (all cap_f1 entries are written);
 *   d_new[b*cap_new + j]         the created points in ascending idx1 (the order of vMatchedIndices, so the order the reference creates them in:
 *                                a stable compaction); entries past d_nnew[b] are unspecified;
 *   d_nnew[b] = min(d_nrequired[b], cap_new); d_nrequired[b] = the number the reference creates: overflow is reported, never silent;
 *   d_point_of_1[b*cap_f1 + i1]  the rank j of the point feature i1 created, or -1;
 *   d_point_of_2[b*cap_f2 + i2]  the rank of the LAST creator (greatest idx1) that matched i2, or -1: SearchForTriangulation never marks
 *                                vbMatched2, so two idx1 may hit one idx2 and the later pKF2->AddMapPoint wins (all cap_f2 entries are written);
 *   has_mp of both sides         set to 1 for idx1 / idx2 of every stored point, so that the next orbm_search_for_triangulation on the same
 *                                stream (the next neighbour) skips them with no host step;
 *   d_pair_flags[b]              ORBM_NEWPT_PAIR_* bits.
 * A point whose rank is >= cap_new is not stored: its status still names the exit, its d_point_of_* entries stay -1 and has_mp is not set.
 * NaN poses give NaN points through the gates exactly as the reference's comparisons do (every comparison with a NaN is false).
 * Asynchronous on `stream`, no host synchronisation, graph-capturable, deterministic (no floating-point atomics).  ORB_E_INVALID for null
 * pointers (kps_raw, u_right, depth without u_right and has_mp excepted), cap_f < 1, cap_new < 1, batch < 0; batch == 0 is a successful no-op.
 * The pair records live on the device: a camera_type outside the two is refused with ORB_E_INVALID by the wrappers that build the records;
 * on the device such a pair is flagged ORBM_NEWPT_PAIR_BAD_CAMERA. */
int orbm_create_new_map_points(const orbm_newpt_side* kf1, const orbm_newpt_side* kf2, const orbm_newpt_pair* d_pairs,
                               const int32_t* d_match12, int batch, uint8_t* d_status, orbm_new_point* d_new, int cap_new,
                               int32_t* d_nnew, int32_t* d_nrequired, int32_t* d_point_of_1, int32_t* d_point_of_2,
                               uint32_t* d_pair_flags, void* stream);

/* Appends the created points of all pairs to the device map the other kernels read, in order (b ascending, then j ascending), with no host
 * step.  *d_n_mp is the in/out cursor (the number of map points).  The point with rank r overall becomes record p = cursor + r:
 *   d_mp[p] = {pos, flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS, desc_row = p, everything else 0};
 *   its two observation records (kf1, desc_row0_1 + idx1) and (kf2, desc_row0_2 + idx2), in the order obs_kf2_first gives, at the end of the
 *   CSR: d_obs[d_obs_start[p] ..], d_obs_start[p+1] = d_obs_start[p] + 2 (d_obs_start has cap_mp + 1 entries, d_obs_start[cursor] = the end);
 *   d_ref[p] = {ref_kf = kf1, level = d_kps1[b*cap_f1 + idx1].octave} (mvKeysUn of KF1);
 *   d_sel[0 .. cap_sel) = the new indices followed by -1 padding: orbm_refresh_map_points skips indices outside [0, n_mp), so it can be
 *   called right after on the same stream with n_mp = cap_mp and n_sel = cap_sel.
 * A point that does not fit (p >= cap_mp, p >= n_desc_rows, its records past cap_obs, r >= cap_sel) is not written, and neither is any after
 * it; d_appended[0] = the number written, d_appended[1] = the shortfall; the cursor advances by d_appended[0].  Nothing else in the slabs
 * changes (the descriptor slab is not touched: ORBM_REFRESH_DESCRIPTOR fills row p).  Asynchronous on `stream`, graph-capturable.
 * ORB_E_INVALID for null pointers, cap_new / cap_f1 / cap_mp / cap_sel < 1, negative n_desc_rows / cap_obs / batch. */
int orbm_append_new_map_points(const orbm_new_point* d_new, const int32_t* d_nnew, int cap_new, const orbm_newpt_pair* d_pairs, int batch,
                               const orb_keypoint* d_kps1, int cap_f1, int32_t* d_n_mp, orbm_map_point* d_mp, int cap_mp, int n_desc_rows,
                               int32_t* d_obs_start, orbm_observation* d_obs, int cap_obs, orbm_refresh_point* d_ref, int32_t* d_sel,
                               int cap_sel, int32_t* d_appended, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Local map: Tracking::UpdateLocalMap on the device map, so that the list ORBM_PROJ_LOCAL_MAP reads is built where it is used:
 * Tracking::UpdateLocalKeyFrames (Tracking.cc:3042-3244), Tracking::UpdateLocalPoints (:2998-3036) and the marking loop at the head of
 * Tracking::SearchLocalPoints (:2852-2872).  Integer work only (votes, ordered lists, first-occurrence de-duplication): every output is the
 * reference's, bit for bit.  IncreaseVisible / mnVisible and mmProjectPoints are the caller's.
 * ------------------------------------------------------------------------------------------------------- */
/* One key frame of the map, in the index space of orbm_observation.kf and of d_kf of orbm_refresh_map_points. */
typedef struct orbm_localmap_keyframe {
    uint32_t flags;            /* ORBM_LM_KF_* */
    int32_t parent;            /* GetParent(), or -1 */
    int32_t prev;              /* mPrevKF, or -1 */
    int32_t mp_row0, n_feat;   /* d_kf_mp[mp_row0 + i] = the map-point index of GetMapPointMatches()[i], or -1 */
    int32_t covis[10];         /* GetBestCovisibilityKeyFrames(10) in order, padded with -1 */
    int32_t child_start, n_child;   /* d_children[child_start .. + n_child) = GetChilds() in the iteration order of the std::set<KeyFrame*>:
                                     * the host owns that pointer-order fact */
    int32_t reserved;
} orbm_localmap_keyframe;      /* 72 B */
#define ORBM_LM_KF_PRESENT 1u  /* the slot holds a key frame */
#define ORBM_LM_KF_BAD 2u      /* isBad() */

/* The device map (a host struct of device pointers).  d_mp, d_obs_start and d_obs are the slabs orbm_refresh_map_points and
 * orbm_append_new_map_points keep current; an array whose count is 0 may be NULL. */
typedef struct orbm_localmap_view {
    const orbm_map_point* d_mp;                 /* [n_mp], 16-byte aligned */
    const int32_t* d_obs_start;                 /* [n_mp + 1] */
    const orbm_observation* d_obs;              /* [n_obs] */
    const orbm_localmap_keyframe* d_kf;         /* [n_kf] */
    const int32_t* d_kf_mp;                     /* [n_kf_mp_rows] */
    const int32_t* d_children;                  /* [n_children] */
    const int32_t* d_kf_by_order;               /* [n_kf]: the key-frame index at each rank of KeyFrame* address order, the iteration order of
                                                 * map<KeyFrame*,int> keyframeCounter: a permutation the host supplies */
    orbm_track* d_mp_track;                     /* the persistent orbm_track of every map point (mbTrackInView outlives a frame): frame b uses
                                                 * d_mp_track + b*track_stride; 16-byte aligned */
    int32_t n_mp, n_obs, n_kf, n_kf_mp_rows, n_children;
    int32_t track_stride;                       /* in records, >= n_mp; 0 (all frames share one slab) is accepted only with batch == 1 */
} orbm_localmap_view;

typedef struct orbm_localmap_frame {
    int32_t last_kf;           /* mCurrentFrame.mpLastKeyFrame, or -1 */
    uint32_t flags;            /* ORBM_LM_INERTIAL */
} orbm_localmap_frame;         /* 8 B */
#define ORBM_LM_INERTIAL 1u    /* mSensor is IMU_MONOCULAR or IMU_STEREO: the tail :3217-3236 runs */

/* The per-frame lists of map-point indices (-1 = no point), [batch][cap_f] / [batch][cap_dropped]; counts are clamped to the capacity. */
typedef struct orbm_localmap_lists {
    int32_t* d_vote_mp;            /* in/out: the list that votes, mCurrentFrame.mvpMapPoints or mLastFrame.mvpMapPoints by the test at :3050 */
    const int32_t* d_n_vote;       /* [batch] */
    int32_t* d_frame_mp;           /* in/out: mCurrentFrame.mvpMapPoints for the marking loop; may be the very pointer d_vote_mp */
    const int32_t* d_n_frame;      /* [batch] */
    const int32_t* d_dropped_mp;   /* or NULL: the points an earlier tracking step removed as outliers, with mnLastFrameSeen = the frame's id and
                                    * mbTrackInView = false (:2234-2240, :2415) */
    const int32_t* d_n_dropped;    /* [batch]; needed when d_dropped_mp is given */
    int32_t cap_f, cap_dropped;
} orbm_localmap_lists;

typedef struct orbm_localmap_out {
    int32_t* d_local_kf;               /* [batch][cap_kf] mvpLocalKeyFrames */
    int32_t* d_n_local_kf;             /* [batch] min(required, cap_kf) */
    int32_t* d_n_local_kf_required;    /* [batch] mvpLocalKeyFrames.size() */
    int32_t* d_ref_kf;                 /* [batch] pKFmax, or -1: keep the old reference key frame */
    int32_t* d_max_votes;              /* [batch] */
    int32_t* d_local_src;              /* [batch][cap_mp] the map-point index of mvpLocalMapPoints[j] */
    int32_t* d_nmp;                    /* [batch] min(required, cap_mp) */
    int32_t* d_nmp_required;           /* [batch] mvpLocalMapPoints.size() */
    orbm_map_point* d_local_mp;        /* [batch][cap_mp] the slab records, ORBM_MP_SEEN or-ed in; 16-byte aligned */
    orbm_track* d_track;               /* [batch][cap_mp] gathered from the track slab; 16-byte aligned */
    uint32_t* d_flags;                 /* [batch] ORBM_LM_* bits */
    int32_t cap_kf, cap_mp;
} orbm_localmap_out;
/* d_flags bits */
#define ORBM_LM_KF_OVERFLOW 1u   /* d_n_local_kf_required > cap_kf: the frame has d_nmp = d_nmp_required = 0 */
#define ORBM_LM_MP_OVERFLOW 2u   /* d_nmp_required > cap_mp: the first cap_mp points were written */
#define ORBM_LM_BAD_INDEX 4u     /* an index was out of range or named an empty slot and was treated as absent */

/* Bytes of d_work for orbm_update_local_map, a multiple of 16 (0 for a negative argument); d_work is 16-byte aligned. */
size_t orbm_local_map_workspace_bytes(int n_kf, int n_mp, int batch);

/* Builds the local map of `batch` frames; frame b reads d_frames[b] and row b of every list.
 * Nulling and voting: a list entry whose point is ORBM_MP_BAD becomes -1, in both lists; an entry outside [0, n_mp) (and not -1) or whose slot
 * is not ORBM_MP_VALID becomes -1 too and sets ORBM_LM_BAD_INDEX.  Each remaining vote entry adds 1 per mObservations entry: an ORBM_OBS_RIGHT
 * record that directly follows a record of the same key frame belongs to the same entry and does not count again.  A record whose kf is
 * outside [0, n_kf), or a point whose CSR range leaves [0, n_obs], is skipped and flagged.
 * First level (:3131-3150), in d_kf_by_order order: a key frame with votes that is ORBM_LM_KF_BAD is skipped before the max test; pKFmax =
 * the first key frame with the greatest count (strict >); no cap of 80.  A voted slot without ORBM_LM_KF_PRESENT is skipped and flagged.
 * Second loop (:3155-3213) over the first-level entries only, `size() > 80` tested at the top of each iteration: the first key frame of
 * covis[] that is not bad and not listed, then the first such child, then the parent if it is not listed, bad or not; the parent branch's
 * `break` leaves the OUTER loop, so the first parent added ends the whole loop.  -1 in covis[] is padding; any other entry of covis[],
 * every entry of d_children, a parent or a prev that is out of range or not ORBM_LM_KF_PRESENT is skipped and flagged (-1 in d_children too).
 * Inertial tail (:3217-3236), with ORBM_LM_INERTIAL and size() < 80: up to 20 rounds from last_kf along prev; a key frame that is already
 * listed is NOT advanced past, so the remaining rounds do nothing.
 * UpdateLocalPoints: the local key frames in REVERSE order, each in feature order; -1 skipped, bad points never listed, the first occurrence
 * wins (two occurrences inside one key frame included).  A key frame whose rows leave [0, n_kf_mp_rows) contributes nothing and is flagged.
 * Marking (:2852-2872): record j has ORBM_MP_SEEN or-ed in where its point is in the frame list after nulling, or in the dropped list.
 * d_track[j] is the point's entry of the track slab as it stands; in_view is forced to 0 for dropped points ONLY: the marking loop clears
 * mbTrackInViewR, not mbTrackInView, so a point of the frame list keeps a stale in_view = 1 and still produces a query.
 * d_local_mp, d_nmp and d_track are directly the d_mp, d_nmp and d_track of orbm_project_map_points(ORBM_PROJ_LOCAL_MAP) with cap_mp; the
 * descriptor slab is shared (desc_row is copied as it is).  Entries past the counts are not written.
 * Overflow is reported, never silent: see ORBM_LM_KF_OVERFLOW / ORBM_LM_MP_OVERFLOW.
 * Five launches on `stream` (the first clears the workspace, so that nothing depends on an earlier call), nothing read on the host,
 * graph-capturable;
 * integer atomics only: deterministic.  ORB_E_INVALID for null pointers (d_dropped_mp and arrays of count 0 excepted), negative counts,
 * capacities below 1, a negative batch, track_stride 0 with batch > 1 or 0 < track_stride < n_mp, misaligned record slabs or workspace;
 * batch == 0 is a successful no-op. */
int orbm_update_local_map(const orbm_localmap_view* view, const orbm_localmap_frame* d_frames, const orbm_localmap_lists* lists, int batch,
                          const orbm_localmap_out* out, void* d_work, void* stream);

/* The scatter-back after the projection, so that the next frame reads the members isInFrustum left: d_mp_track[b*track_stride +
 * d_local_src[b*cap_mp + j]] = d_track[b*cap_mp + j] for j < min(d_nmp[b], cap_mp); an index outside [0, n_mp) is skipped.  Asynchronous on
 * `stream`, graph-capturable.  ORB_E_INVALID as above. */
int orbm_store_local_tracks(const orbm_track* d_track, const int32_t* d_local_src, const int32_t* d_nmp, int cap_mp, int batch,
                            orbm_track* d_mp_track, int track_stride, int n_mp, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Key-frame culling: LocalMapping::KeyFrameCulling (LocalMapping.cc:1170-1322) on the device map, with the map effects of
 * KeyFrame::SetBadFlag (KeyFrame.cc:651-688: the early returns and the EraseObservation loop), MapPoint::EraseObservation (MapPoint.cc:197-231)
 * and MapPoint::SetBadFlag (:254-277).  The loop is sequential in its effects (an erased key frame lowers Observations() of its points, a point
 * that drops to nObs <= 2 goes bad and leaves every other key frame's count, the inertial modes relink mPrevKF / mNextKF), so the candidates
 * of one problem are walked in order; `batch` problems are independent: all read the same orbm_localmap_view, start from the map as given and
 * keep their own state in the workspace.  Integer work and decisions only: every output is the reference's, bit for bit.
 * Single-camera key frames only (NLeft == -1, no mpCamera2): the rig branch of :1236-1238 is not restated; an ORBM_OBS_RIGHT record is
 * treated as absent and sets ORBM_CULL_UNSUPPORTED.  MergePrevious and the spanning-tree work of KeyFrame::SetBadFlag stay with the caller,
 * who replays the cull events in order.
 * ------------------------------------------------------------------------------------------------------- */
/* Parallel to view->d_kf: what the culling reads of a key frame beyond orbm_localmap_keyframe. */
typedef struct orbm_cull_keyframe {
    double timestamp;      /* mTimeStamp */
    uint32_t id;           /* mnId */
    int32_t prev, next;    /* mPrevKF / mNextKF as indices into d_kf, or -1 */
    int32_t desc_row0;     /* the key frame's base row in the key-frame descriptor slab: feature index = orbm_observation.desc_row - desc_row0 */
    float imu_pos[3];      /* GetImuPosition() */
    uint32_t flags;        /* ORBM_CULL_KF_* */
} orbm_cull_keyframe;      /* 40 B */
#define ORBM_CULL_KF_NOT_ERASE 1u   /* mbNotErase: KeyFrame::SetBadFlag only sets mbToBeErased */

/* Per feature, parallel to view->d_kf_mp: one byte. */
#define ORBM_CULL_FEAT_OCTAVE 0x3Fu   /* mask: mvKeysUn[i].octave */
#define ORBM_CULL_FEAT_CLOSE 0x40u    /* !(mvDepth[i] > mThDepth || mvDepth[i] < 0), evaluated by the host with that very expression */
#define ORBM_CULL_FEAT_STEREO 0x80u   /* mvuRight[i] >= 0: the observation weighs 2 in nObs (MapPoint.cc:191-194, 209-212) */

typedef struct orbm_cull_problem {
    int32_t current_kf;            /* mpCurrentKeyFrame, an index into d_kf */
    uint32_t init_kf_id;           /* GetMap()->GetInitKFid() */
    int32_t cand_start, n_cand;    /* d_candidates[cand_start .. + n_cand) = GetVectorCovisibleKeyFrames() in its order */
    int32_t n_kf_in_map;           /* mpAtlas->KeyFramesInMap() at the call */
    uint32_t flags;                /* ORBM_CULL_* mode bits */
} orbm_cull_problem;               /* 24 B */
#define ORBM_CULL_INERTIAL 1u          /* mbInertial */
#define ORBM_CULL_MONOCULAR 2u         /* mbMonocular */
#define ORBM_CULL_IMU_INITIALIZED 4u   /* mpAtlas->isImuInitialized() */
#define ORBM_CULL_INERTIAL_BA2 8u      /* GetIniertialBA2() */
#define ORBM_CULL_ABORT_BA 16u         /* mbAbortBA: a SNAPSHOT taken at the call; the reference reads the member live at the bottom of every
                                        * iteration, so a flag raised while the loop runs is seen by the reference and not here */

/* The inputs beyond the view (a host struct of device pointers). */
typedef struct orbm_cull_in {
    const orbm_cull_keyframe* d_ckf;       /* [view->n_kf] */
    const uint8_t* d_feat;                 /* [view->n_kf_mp_rows] ORBM_CULL_FEAT_* */
    const int32_t* d_mp_nobs;              /* [view->n_mp] MapPoint::nObs, or NULL: the weighted sum over the point's records.  The reference's
                                            * counter can drift from mObservations (AddObservation on an existing entry counts again): a caller
                                            * that tracks it passes it */
    const orbm_cull_problem* d_problems;   /* [batch] */
    const int32_t* d_candidates;           /* [n_candidates] shared by all problems */
    int32_t n_candidates;
    int32_t n_cand_max;                    /* the greatest n_cand of any problem, as the caller knows it: above cap_cand is refused */
} orbm_cull_in;

typedef struct orbm_cull_event {
    int32_t kf;            /* the key frame KeyFrame::SetBadFlag was called on */
    int32_t prev, next;    /* the links as they were when the inertial branch relinked them (next.prev = prev, prev.next = next); -1, -1 otherwise */
} orbm_cull_event;         /* 12 B */

typedef struct orbm_cull_out {
    uint8_t* d_code;               /* [batch][cap_cand] ORBM_CULL_CODE_* of every candidate; entries [0, n_cand) are written */
    int32_t* d_nmps;               /* [batch][cap_cand] nMPs as the reference had it at that candidate (0 where the body did not run) */
    int32_t* d_nred;               /* [batch][cap_cand] nRedundantObservations, likewise */
    orbm_cull_event* d_events;     /* [batch][cap_cand] one per SetBadFlag call, in order; entries [0, d_n_events[b]) are written */
    int32_t* d_n_events;           /* [batch] */
    uint32_t* d_flags;             /* [batch] ORBM_CULL_BAD_INDEX | ORBM_CULL_UNSUPPORTED */
    int32_t cap_cand, reserved;
} orbm_cull_out;
/* d_code: the exit of the loop body for the candidate */
#define ORBM_CULL_CODE_NOT_VISITED 0         /* the loop ended before it */
#define ORBM_CULL_CODE_SKIPPED 1             /* the init key frame or isBad() (:1212), or an index that could not be read */
#define ORBM_CULL_CODE_KEPT 2                /* not redundant (:1278 false) */
#define ORBM_CULL_CODE_KEPT_FEW_KFS 3        /* KeyFramesInMap() <= 21 (:1282), a `continue` */
#define ORBM_CULL_CODE_KEPT_RECENT 4         /* mnId > current mnId - 2 (:1285), a `continue` */
#define ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR 5   /* mPrevKF or mNextKF missing (:1288) */
#define ORBM_CULL_CODE_KEPT_INERTIAL 6       /* neither branch of :1292 / :1301 */
#define ORBM_CULL_CODE_CULLED 7              /* :1314 */
#define ORBM_CULL_CODE_CULLED_IMU1 8         /* :1292-1300 */
#define ORBM_CULL_CODE_CULLED_IMU2 9         /* :1301-1309 */
#define ORBM_CULL_CODE_DEFERRED 0x80         /* or-ed in: ORBM_CULL_KF_NOT_ERASE, SetBadFlag changed no map state (a relink still happened) */
/* d_flags bits */
#define ORBM_CULL_BAD_INDEX 1u     /* an index was out of range or named an empty slot: never read through, treated as absent */
#define ORBM_CULL_UNSUPPORTED 2u   /* the map holds an ORBM_OBS_RIGHT record (a rig): treated as absent */
/* the low two bits of a record's state word in the workspace (orbm_cull_workspace) */
#define ORBM_CULL_REC_LIVE 0u
#define ORBM_CULL_REC_ERASED_BY_KF 1u      /* mObservations.erase(pKF) of EraseObservation */
#define ORBM_CULL_REC_ERASED_BY_POINT 2u   /* mObservations.clear() of MapPoint::SetBadFlag: EraseMapPointMatch(leftIndex) ran */
#define ORBM_CULL_REC_ABSENT 3u            /* a bad index or a rig record: never live */

/* Bytes of d_work for orbm_cull_keyframes / orbm_apply_keyframe_culling, a multiple of 16 (0 for a negative argument); d_work is 16-byte
 * aligned.  Problem b owns the slice d_work + b * (bytes / batch); orbm_cull_workspace gives the sections of one slice as byte offsets. */
size_t orbm_cull_workspace_bytes(int n_kf, int n_mp, int n_obs, int batch);
typedef struct orbm_cull_workspace_layout {
    size_t stride;         /* bytes of one problem's slice */
    size_t nobs;           /* int32 [n_mp]: the final MapPoint::nObs */
    size_t rec;            /* uint32 [n_obs]: ORBM_CULL_REC_* in the low two bits (bits 8-15: the record's ORBM_CULL_FEAT_* byte) */
    size_t prev, next;     /* int32 [n_kf] each: the final links */
    size_t mp_bad;         /* uint8 [n_mp]: the point is bad */
    size_t kf_erased;      /* uint8 [n_kf]: the key frame was erased by this problem */
} orbm_cull_workspace_layout;
int orbm_cull_workspace(int n_kf, int n_mp, int n_obs, orbm_cull_workspace_layout* layout);

/* Walks LocalMapping.cc:1176-1321 for `batch` problems.  Kept literally:
 *  - `count++` comes first and the break test `(count > 20 && ABORT_BA) || count > 100` sits at the BOTTOM of the body: every `continue` (the
 *    init key frame, a bad key frame, ORBM_CULL_CODE_KEPT_FEW_KFS, ORBM_CULL_CODE_KEPT_RECENT) skips it, so a candidate past the 100th that is
 *    not skipped is still fully processed, and culled if redundant, before the loop ends.
 *  - nMPs counts the features whose point exists, is not bad NOW and, unless MONOCULAR, has ORBM_CULL_FEAT_CLOSE; a point held by two features
 *    counts twice.  A point enters the observation walk only if its live nObs > 3; the walk counts the live records of other key frames whose
 *    octave <= the feature's octave + 1; more than 3 of them make the feature redundant.  ORBM_OBS_KF_BAD is not consulted (the reference
 *    does not test pKFi->isBad()).
 *  - redundant_th is a float, 0.9f, or 0.5f with INERTIAL and not MONOCULAR; the test is (float)nRedundant > redundant_th * (float)nMPs with
 *    the product rounded to float (nMPs = 10, nRedundant = 9 is KEPT).
 *  - Not inertial: SetBadFlag.  Inertial (:1280-1310): the live KeyFramesInMap() (it drops by one per key frame erased) <= 21 -> continue;
 *    mnId > current mnId - 2 in unsigned arithmetic -> continue; both live links are needed; t = (float)(timestamp[next] - timestamp[prev]);
 *    first branch (IMU_INITIALIZED && mnId < last_ID && t < 3) || t < 0.5, with last_ID from the 21-step walk along the INITIAL prev chain
 *    from the current key frame (:1193-1203); second branch !INERTIAL_BA2 && cv::norm(imu_pos - imu_pos[prev]) < 0.02 && t < 3, the norm by
 *    the rule of the map-point refresh (float differences, sqrt of the double dot product) compared as a double.  Either branch relinks
 *    next.prev = prev, prev.next = next, clears the candidate's links, then calls SetBadFlag.
 *  - SetBadFlag: with ORBM_CULL_KF_NOT_ERASE the code gets ORBM_CULL_CODE_DEFERRED and no map state changes (the relink has happened and is
 *    in the event).  Otherwise the key frame is erased (bad from now on, KeyFramesInMap() - 1) and EraseObservation runs for every feature
 *    with a point: if the point's record of this key frame is live it dies and nObs drops by 2 with ORBM_CULL_FEAT_STEREO of the RECORD's
 *    feature, else by 1; if then nObs <= 2 the point goes bad and all its live records die "by the point".  Each record dies exactly once
 *    whatever the lane order (an integer compare-and-swap on its state word).  (The init key frame never reaches SetBadFlag: :1212 skips it.)
 *  - Bad index: the init launch checks the whole map once: a record whose kf is out of range, not ORBM_LM_KF_PRESENT, or whose feature index
 *    leaves the key frame's rows is ORBM_CULL_REC_ABSENT; a link that is out of range or names an empty slot is -1; a point whose CSR range
 *    leaves [0, n_obs] has no records; each sets ORBM_CULL_BAD_INDEX in every problem.  The walk checks what it indexes through: the current
 *    key frame and the candidate range (nothing is visited), a candidate (ORBM_CULL_CODE_SKIPPED), a key frame's rows (no features), a
 *    d_kf_mp entry outside [0, n_mp) that is not -1 or whose slot is not ORBM_MP_VALID, a point with a bad CSR range (absent).
 * Three launches on `stream`: two fill every problem's slice (kernels, not memset nodes: the flag words first, because the second ors into
 * them), then the walk, one workgroup per problem.
 * Nothing is read on the host; graph-capturable; integer atomics only: deterministic.  ORB_E_INVALID for null pointers (d_mp_nobs and arrays
 * of count 0 excepted), negative counts, cap_cand < 1, n_cand_max > cap_cand, a misaligned d_mp or workspace; batch == 0 is a no-op. */
int orbm_cull_keyframes(const orbm_localmap_view* view, const orbm_cull_in* in, int batch, const orbm_cull_out* out, void* d_work, void* stream);

/* The slabs orbm_apply_keyframe_culling folds a problem's outcome into (a host struct of device pointers; the same arrays the view and
 * orbm_cull_in name, now written). */
typedef struct orbm_cull_apply {
    orbm_map_point* d_mp;               /* [n_mp] flags: ORBM_MP_BAD or-ed in for points that went bad; ORBM_MP_HAS_OBS = final nObs > 0 (a bad
                                         * point keeps the bit: MapPoint::SetBadFlag does not reset nObs) */
    orbm_localmap_keyframe* d_kf;       /* [n_kf] ORBM_LM_KF_BAD or-ed in for erased key frames; prev = the final link */
    orbm_cull_keyframe* d_ckf;          /* [n_kf] prev / next = the final links */
    int32_t* d_kf_mp;                   /* [n_kf_mp_rows] -1 at the feature of every record erased BY THE POINT (EraseMapPointMatch); the
                                         * erased key frame's own row keeps its entries, as in the reference */
    int32_t* d_mp_nobs;                 /* [n_mp] written back, or NULL */
    orbm_refresh_point* d_ref;          /* [n_mp] a point that is not bad and whose ref_kf's record was erased gets {kf of its first remaining
                                         * record, that feature's octave} = mObservations.begin()->first after any sequence of erasures */
    int32_t* d_obs_start_out;           /* [n_mp + 1] the compacted CSR: the live records in order */
    orbm_observation* d_obs_out;        /* [cap_obs_out] */
    int32_t* d_result;                  /* [2]: the records the compacted CSR needs; 1 if that is more than cap_obs_out, else 0 */
    int32_t cap_obs_out, reserved;
} orbm_cull_apply;

/* Folds problem `problem` of the last orbm_cull_keyframes on this workspace into the device map, so that the next orbm_update_local_map /
 * orbm_refresh_map_points reads a current map with no host step (count, scan, write: three launches on `stream`, graph-capturable).  On
 * overflow (d_result[1] = 1) NOTHING is written but d_result.  A deferred key frame changes nothing but the links.  ORB_E_INVALID for null
 * pointers (d_mp_nobs excepted), negative counts, a problem outside [0, batch), a misaligned d_mp or workspace. */
int orbm_apply_keyframe_culling(const orbm_localmap_view* view, const orbm_cull_in* in, int batch, int problem, const orbm_cull_apply* apply,
                                void* d_work, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Covisibility graph: KeyFrame::UpdateConnections (KeyFrame.cc:427-550) with KeyFrame::AddConnection (:228-241) and UpdateBestCovisibles
 * (:243-265), and the connection part of KeyFrame::SetBadFlag (:675-678, 696-697) with EraseConnection (:793-807), on the device map: the
 * writers of what orbm_localmap_keyframe.covis and orbm_cull_problem's candidate list read.  Integer work only: every output is the
 * reference's, bit for bit.  The spanning-tree loop of SetBadFlag, AddChild / ChangeParent and the d_children CSR stay with the caller (who
 * replays the child events), as do bowdb_keyframe.covis (copy from the ordered rows), loop edges and rigs beyond the RIGHT-record rule.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct orbm_covis_entry {
    int32_t kf;            /* the key of mConnectedKeyFrameWeights, an index into d_kf */
    int32_t weight;
} orbm_covis_entry;        /* 8 B */

/* Parallel to view->d_kf, in/out: what UpdateConnections reads of a key frame beyond orbm_localmap_keyframe. */
typedef struct orbm_covis_keyframe {
    uint32_t id;           /* mnId */
    int32_t map_id;        /* GetMap(), as any number that tells maps apart */
    uint32_t flags;        /* ORBM_COVIS_KF_* */
    int32_t reserved;
} orbm_covis_keyframe;     /* 16 B */
#define ORBM_COVIS_KF_FIRST_CONNECTION 1u   /* mbFirstConnection: cleared when the parent is set */

/* The graph of every key frame (a host struct of device pointers; caller-owned slabs, all in/out).  Row k of d_conn is
 * mConnectedKeyFrameWeights of key frame k as an insertion-ordered map: an own update writes the whole counter in d_kf_by_order order, an
 * AddConnection on a new key appends, an overwrite keeps its place, an erase closes the gap keeping the order.  Rows k of d_ordered_kf /
 * d_ordered_w are mvpOrderedConnectedKeyFrames / mvOrderedWeights.  Entries past the counts are never written. */
typedef struct orbm_covis_store {
    orbm_covis_entry* d_conn;   /* [n_kf][cap_conn], 8-byte aligned */
    int32_t* d_n_conn;          /* [n_kf] */
    int32_t* d_ordered_kf;      /* [n_kf][cap_conn] */
    int32_t* d_ordered_w;       /* [n_kf][cap_conn] */
    int32_t* d_n_ordered;       /* [n_kf] */
    int32_t cap_conn, reserved;
} orbm_covis_store;

typedef struct orbm_covis_child_event {
    int32_t child, parent;     /* mpParent = parent; parent->AddChild(child) */
} orbm_covis_child_event;      /* 8 B */

typedef struct orbm_covis_out {
    orbm_covis_child_event* d_child_events;   /* [n_list] in list order; entries [0, d_n_child_events[0]) are written */
    int32_t* d_n_child_events;                /* [1] */
    int32_t* d_nmax;                          /* [n_list] nmax of list entry l (0 where the counter was empty) */
    int32_t* d_kfmax;                         /* [n_list] pKFmax, or -1 */
    int32_t* d_n_counter;                     /* [n_list] KFcounter.size(); 0 = the early return: nothing of the key frame changed */
    int32_t* d_overflow_kf;                   /* [1] the smallest key-frame index whose row dropped an insert, or -1 */
    uint32_t* d_flags;                        /* [1] ORBM_COVIS_* bits */
} orbm_covis_out;
#define ORBM_COVIS_BAD_INDEX 1u   /* an index was out of range or named an empty slot: never read through, treated as absent */
#define ORBM_COVIS_OVERFLOW 2u    /* a row insert did not fit cap_conn and was dropped: d_overflow_kf; every other row is exact */

/* Bytes of d_work for orbm_update_connections (and, with n_list = 0, for orbm_erase_connections), a multiple of 16 (0 for a negative
 * argument); d_work is 16-byte aligned. */
size_t orbm_covis_workspace_bytes(int n_kf, int n_list);

/* KeyFrame::UpdateConnections for the key frames d_list[0 .. n_list) IN LIST ORDER (the loop of CorrectLoop / MergeLocal; n_list = 1 is
 * ProcessNewKeyFrame; a key frame may be listed twice).  d_ckf is parallel to view->d_kf; d_kf is the writable view->d_kf (the same pointer).
 *  - Counter: for every feature of A whose point exists (ORBM_MP_VALID) and is not ORBM_MP_BAD, every mObservations entry of the point counts
 *    for its key frame, except an observer with A's mnId (ids, not slots, are compared), an observer that is ORBM_LM_KF_BAD, and one whose
 *    map_id differs.  A point held by two features counts twice; an ORBM_OBS_RIGHT record that directly follows a record of the same key
 *    frame is the same entry (the rule of orbm_update_local_map).
 *  - An empty counter is the early return: d_n_counter = 0, nothing of A changes (stale rows and ORBM_COVIS_KF_FIRST_CONNECTION included).
 *  - In d_kf_by_order order: pKFmax is the first entry with the greatest count; every entry with count >= 15 gets AddConnection(A, count);
 *    if there is none, pKFmax gets it.  A's ordered rows hold exactly those entries, weight descending, ties by pointer order DESCENDING,
 *    with no isBad() filter; A's row of d_conn becomes the WHOLE counter.
 *  - B.AddConnection(A, w): a new key is appended, another weight is overwritten in place, and B's ordered rows are rebuilt from its WHOLE
 *    row (entries below 15 included) without the entries that are ORBM_LM_KF_BAD; the same weight changes nothing and rebuilds nothing.
 *  - With ORBM_COVIS_KF_FIRST_CONNECTION and id != init_kf_id: d_kf[A].parent = the front of A's ordered row, the flag is cleared, and a
 *    child event is written.
 *  - d_kf[k].covis (padded with -1) is rewritten for every key frame whose ordered rows were rebuilt.
 * Bad index (flagged, treated as absent): a list entry, a record's kf, a d_kf_mp entry, a CSR range, a stored kf, or a key frame without a
 * rank because d_kf_by_order is not a permutation.  Four launches on `stream` (the first clears the workspace), nothing read on the host,
 * graph-capturable, integer atomics only: deterministic.  ORB_E_INVALID for null pointers (arrays of count 0 excepted), negative counts,
 * cap_conn < 1, misaligned d_mp, d_conn or workspace; n_list == 0 is a successful no-op. */
int orbm_update_connections(const orbm_localmap_view* view, const orbm_covis_store* store, orbm_covis_keyframe* d_ckf,
                            orbm_localmap_keyframe* d_kf, const int32_t* d_list, int n_list, uint32_t init_kf_id, const orbm_covis_out* out,
                            void* d_work, void* stream);

/* Folds the cull events of orbm_cull_keyframes (d_events[0 .. min(*d_n_events, cap_events)), read on the device) into the store, in event
 * order: every key frame B in the row of the erased K loses its entry of K if it has one (only then are its ordered rows rebuilt, with the
 * bad filter of that moment), then K's row and ordered rows are emptied (covis = -1).  An event whose d_kf_erased[kf] is 0 (deferred) is
 * skipped; d_kf_erased = NULL takes every event.  isBad() as a rebuild sees it: a key frame erased by an EARLIER event of this call is bad,
 * one erased by a later event is not, any other by ORBM_LM_KF_BAD; so the result is the same before and after orbm_apply_keyframe_culling.
 * Of `out` only d_flags is written (the other members may be NULL).  Two launches, graph-capturable.  ORB_E_INVALID as above and for
 * cap_events < 0. */
int orbm_erase_connections(const orbm_localmap_view* view, const orbm_covis_store* store, orbm_localmap_keyframe* d_kf,
                           const orbm_cull_event* d_events, const int32_t* d_n_events, const uint8_t* d_kf_erased, int cap_events,
                           const orbm_covis_out* out, void* d_work, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fusion in the neighbours: LocalMapping::SearchInNeighbors (LocalMapping.cc:913-1043) on the device map, with ORBmatcher::Fuse(pKF,
 * vpMapPoints) (ORBmatcher.cc:1630-1879), MapPoint::Replace (MapPoint.cc:286-338), AddObservation (:160-195) and the
 * ComputeDistinctiveDescriptors inside every Replace.  The step between orbm_append_new_map_points and the bundle adjustment: the only
 * writer of merged observation rows.  The tail (:1045-1065) is the caller's two calls right after, on the same stream:
 * orbm_refresh_map_points(DESCRIPTOR | NORMAL_DEPTH) over d_sel, then orbm_update_connections.
 * Single-camera pinhole key frames only (NLeft == -1, no mpCamera2: the second Fuse(..., true) does not exist); one camera and one extractor
 * setting per call.  An ORBM_OBS_RIGHT record is treated as absent and sets ORBM_FUSENB_UNSUPPORTED.  Everything the call decides is integer
 * work on values that orbm_fuse and orbm_refresh_map_points compute: every output is the reference's, bit for bit.
 * ------------------------------------------------------------------------------------------------------- */
/* Parallel to view->d_kf: the pose Fuse reads (row-major rotation). */
typedef struct orbm_fusenb_pose {
    float Rcw[9], tcw[3];   /* GetRotation(), GetTranslation() */
    float Ow[3];            /* GetCameraCenter() */
    int32_t reserved;
} orbm_fusenb_pose;         /* 64 B */

typedef struct orbm_fusenb_params {
    int32_t current_kf;            /* mpCurrentKeyFrame, an index into d_kf */
    uint32_t flags;                /* ORBM_FUSENB_* mode bits */
    float fx, fy, cx, cy, mbf;     /* of every key frame */
    float th;                      /* Fuse's th: 3.0f */
    float bounds[4];               /* mnMinX, mnMaxX, mnMinY, mnMaxY: IsInImage is x >= minX && x < maxX && y >= minY && y < maxY */
    orbm_grid_params grid;
    int32_t nlevels;               /* mnScaleLevels, 1..16 */
    int32_t reserved;
    float scale_factors[16];       /* mvScaleFactors */
    float inv_level_sigma2[16];    /* mvInvLevelSigma2 */
    float level_thresholds[16];    /* orbm_predict_scale_thresholds(mfLogScaleFactor, nlevels, .) */
} orbm_fusenb_params;
#define ORBM_FUSENB_MONOCULAR 1u   /* mbMonocular: nn = 20 instead of 10 */
#define ORBM_FUSENB_INERTIAL 2u    /* mbInertial: the mPrevKF walk of :968-982 */
#define ORBM_FUSENB_ABORT_BA 4u    /* mbAbortBA: a SNAPSHOT taken at the call, as ORBM_CULL_ABORT_BA is */

/* The inputs beyond the view (a host struct of device pointers).  The per-feature tables are parallel to view->d_kf_mp. */
typedef struct orbm_fusenb_in {
    const orbm_cull_keyframe* d_ckf;   /* [n_kf]: id and desc_row0 are read */
    const orbm_fusenb_pose* d_pose;    /* [n_kf] */
    const uint8_t* d_feat;             /* [n_kf_mp_rows] ORBM_CULL_FEAT_*: ORBM_CULL_FEAT_STEREO decides the nObs weight */
    const orb_keypoint* d_kps;         /* [n_kf_mp_rows] mvKeysUn */
    const float* d_u_right;            /* [n_kf_mp_rows] mvuRight */
    const uint8_t* d_kf_desc;          /* [n_kf_desc_rows][32] key-frame descriptor slab, 16-byte aligned: feature i of key frame k is row
                                        * d_ckf[k].desc_row0 + i */
    const int32_t* d_ordered_kf;       /* [n_kf][cap_conn] rows of orbm_covis_store: GetBestCovisibilityKeyFrames reads the first N */
    const int32_t* d_n_ordered;        /* [n_kf] */
    const int32_t* d_mp_nobs;          /* [n_mp] MapPoint::nObs, or NULL: the weighted record sum, exactly as in orbm_cull_in */
    int32_t n_kf_desc_rows, cap_conn;
    int32_t cap_feat;                  /* the greatest n_feat of any key frame, as the caller knows it, 1..65535: a key frame with more is
                                        * flagged ORBM_FUSENB_BAD_INDEX and neither fused into nor from */
    int32_t reserved;
} orbm_fusenb_in;

typedef struct orbm_fusenb_event {
    int32_t call;          /* the Fuse call: the target's position in d_targets, or n_targets for the stage-2 call into the current key frame */
    int32_t kf;            /* pKF of that call */
    int32_t list_index;    /* i of vpMapPoints[i] */
    int32_t point;         /* pMP */
    int32_t feature;       /* bestIdx */
    int32_t other;         /* pMPinKF, or -1 */
    int32_t kind;          /* ORBM_FUSENB_EV_* */
    int32_t reserved;
} orbm_fusenb_event;       /* 32 B */
#define ORBM_FUSENB_EV_ADD 0                   /* pMP->AddObservation(pKF, bestIdx); pKF->AddMapPoint(pMP, bestIdx) */
#define ORBM_FUSENB_EV_LIST_POINT_REPLACED 1   /* pMP->Replace(pMPinKF): nObs(pMPinKF) > nObs(pMP) */
#define ORBM_FUSENB_EV_KF_POINT_REPLACED 2     /* pMPinKF->Replace(pMP) */
#define ORBM_FUSENB_EV_NOOP_BAD 3              /* pMPinKF is bad: nothing changes, nFused still counts */
#define ORBM_FUSENB_EV_NOOP_SAME 4             /* pMPinKF == pMP without a record of pKF: Replace's id test returns */

/* What the call folds into the map (the arrays the view and orbm_fusenb_in name, now written) and what it reports. */
typedef struct orbm_fusenb_out {
    orbm_map_point* d_mp;           /* [n_mp] flags: ORBM_MP_BAD or-ed in for replaced points; ORBM_MP_HAS_OBS = final nObs > 0 (a replaced point
                                     * keeps its nObs: Replace does not reset it) */
    int32_t* d_kf_mp;               /* [n_kf_mp_rows] */
    int32_t* d_mp_nobs;             /* [n_mp] written back, or NULL */
    int32_t* d_found;               /* [n_mp] mnFound, in/out, or NULL: not tracked */
    int32_t* d_visible;             /* [n_mp] mnVisible, likewise */
    uint8_t* d_mp_desc;             /* [n_desc_rows][32] the map-point descriptor slab, 16-byte aligned: the rows of the survivors are rewritten */
    uint32_t* d_fuse_target;        /* [n_kf] mnFuseTargetForKF, in/out: a stale value equal to the current mnId skips the key frame */
    int32_t* d_targets;             /* [cap_targets] vpTargetKFs in order */
    int32_t* d_candidates;          /* [cap_candidates] vpFuseCandidates in order */
    int32_t* d_nfused;              /* [cap_targets + 1] the return value of each Fuse call: [t] for target t, [n_targets] for stage 2;
                                     * entries past that are 0 */
    orbm_fusenb_event* d_events;    /* [cap_events] one per bestDist <= TH_LOW turn that passed the gates, in order */
    int32_t* d_replaced;            /* [n_mp] mpReplaced, or -1 */
    int32_t* d_sel;                 /* [cap_feat] the current key frame's points after the fusion: not bad, first occurrence, padded with -1 */
    int32_t* d_obs_start_out;       /* [n_mp + 1] the merged CSR: every point's records in mObservations order */
    orbm_observation* d_obs_out;    /* [cap_obs_out] */
    int32_t* d_result;              /* [ORBM_FUSENB_R_WORDS] */
    int32_t n_desc_rows, cap_targets, cap_candidates, cap_events, cap_obs_out, reserved;
} orbm_fusenb_out;
/* d_result words */
#define ORBM_FUSENB_R_FLAGS 0                   /* ORBM_FUSENB_* flag bits below */
#define ORBM_FUSENB_R_N_TARGETS 1               /* min(required, cap_targets); 0 on ORBM_FUSENB_TARGET_OVERFLOW */
#define ORBM_FUSENB_R_N_TARGETS_REQUIRED 2      /* vpTargetKFs.size() */
#define ORBM_FUSENB_R_N_CANDIDATES 3            /* min(required, cap_candidates) */
#define ORBM_FUSENB_R_N_CANDIDATES_REQUIRED 4   /* vpFuseCandidates.size() (0 with ORBM_FUSENB_ABORT_BA: there is no stage 2) */
#define ORBM_FUSENB_R_N_EVENTS 5
#define ORBM_FUSENB_R_N_OBS 6                   /* the records the merged CSR needs */
#define ORBM_FUSENB_R_N_SEL 7                   /* entries of d_sel that are not padding */
#define ORBM_FUSENB_R_WORDS 8
/* flag bits */
#define ORBM_FUSENB_BAD_INDEX 1u            /* an index was out of range or named an empty slot: never read through, treated as absent */
#define ORBM_FUSENB_UNSUPPORTED 2u          /* the map holds an ORBM_OBS_RIGHT record (a rig): treated as absent */
#define ORBM_FUSENB_TARGET_OVERFLOW 4u      /* more than cap_targets targets: NOTHING is fused (no stage runs); the marks in d_fuse_target
                                             * were made for every required target all the same */
#define ORBM_FUSENB_CANDIDATE_OVERFLOW 8u   /* more than cap_candidates candidates: stage 2 fuses the first cap_candidates */
#define ORBM_FUSENB_EVENT_OVERFLOW 16u      /* the turn whose event did not fit was NOT applied and the walk ended there: the map holds exactly
                                             * the cap_events turns reported */
#define ORBM_FUSENB_OBS_OVERFLOW 32u        /* the merged CSR does not fit cap_obs_out: d_obs_start_out / d_obs_out were not written */
#define ORBM_FUSENB_REFRESH_OVERFLOW 64u    /* a survivor reached more than ORBM_REFRESH_MAX_OBS usable records: its descriptor was left alone */
#define ORBM_FUSENB_UNSORTED 128u           /* a point's input records were not in d_kf_by_order rank order: they were sorted */

/* The most targets the function can select: 20 first neighbours with 20 second neighbours each (the inertial walk stops at 20). */
#define ORBM_FUSENB_MAX_TARGETS 420

/* Bytes of d_work for orbm_search_in_neighbors, a multiple of 16 (0 for an argument out of range); d_work is 16-byte aligned. */
size_t orbm_fusenb_workspace_bytes(int n_kf, int n_mp, int n_obs, int cap_feat, int cap_candidates, int cap_events);

/* LocalMapping::SearchInNeighbors for the key frame params->current_kf.  view: d_mp, d_obs_start, d_obs, d_kf, d_kf_mp and d_kf_by_order are
 * read; a slot of d_mp without ORBM_MP_VALID has no records and its d_obs_start entry is not read, so the slabs of
 * orbm_append_new_map_points can be passed whole (n_mp = cap_mp, n_obs = cap_obs) right after it, with its d_kf_mp entries in place
 * (the point's records are mObservations, a std::map<KeyFrame*, .>: its order is ascending rank in d_kf_by_order, and that order decides
 * the descriptor tie-break of a survivor).  Kept literally:
 *  - Targets (:917-982).  nn = 10, or 20 with MONOCULAR.  A first neighbour is skipped if ORBM_LM_KF_BAD or d_fuse_target == the current mnId;
 *    each accepted one is marked.  Second neighbours come from the first 20 ordered entries of each FIRST-level target (imax is fixed before the
 *    loop): skipped if bad, marked, or carrying the current mnId (ids, not slots); the `if (mbAbortBA) break` sits at the BOTTOM, so with
 *    ABORT_BA the first target's second neighbours are still added.  INERTIAL: from d_kf[current].prev along prev while size() < 20, advancing
 *    past bad or marked key frames.
 *  - Stage 1 (:989-1008).  The current key frame's d_kf_mp row is copied ONCE as the list; then one Fuse per target in order.
 *  - Fuse.  The gates are read at the point's turn from the live state: the entry is not -1, the point is not bad, and it has no record of pKF
 *    (IsInKeyFrame is membership in mObservations, not in d_kf_mp).  Projection and gates (:1700-1761) with the arithmetic of
 *    orbm_project_map_points: R*X summed in double and rounded once, + t in float; z < 0.0f rejects (-0 passes); fx*x/z + cx; IsInImage as above;
 *    dist3D = float(sqrt(double dot)); dist3D < 0.8f*min || dist3D > 1.2f*max rejects; PO.dot(Pn) < 0.5*dist3D in double; the level is the
 *    number of thresholds <= max_distance / dist3D; radius = th * scale_factors[level]; levels [level-1, level].  The window search is
 *    orbm_fuse with chi2_gate = 1 and TH_LOW, launched on the gathered rows of pKF (its grid is built in the call with orbm_grid_build).
 *  - Apply (:1835-1862), serial in list order, pMPinKF = the live d_kf_mp entry of bestIdx: bad -> nothing; good and nObs(pMPinKF) >
 *    nObs(pMP) (strict) -> pMP->Replace(pMPinKF); good otherwise -> pMPinKF->Replace(pMP); pMPinKF == pMP -> nothing; none -> AddObservation
 *    (+2 with ORBM_CULL_FEAT_STEREO of the feature, else +1; no descriptor recomputation) and AddMapPoint.  nFused counts every such turn.
 *  - Replace(A -> B): A goes bad, d_replaced[A] = B, A's records are cleared (its nObs stays).  Each record (kf, idx) of A in order: B has no
 *    record of kf -> d_kf_mp[kf, idx] = B and B gains the record with its weight; else d_kf_mp[kf, idx] = -1.  found / visible of A are added
 *    to B's.  B's descriptor is recomputed with the rule of orbm_refresh_map_points (it IS that kernel, on the survivors' rows), once per
 *    survivor at the end of each Fuse call: a survivor has a record of pKF from then on, so nothing changes its records again inside that
 *    call but another Replace into it.  PRECONDITION of the bit-for-bit claim: d_kf_mp and the records agree for the points of a list (a
 *    point that sits in pKF's row WITHOUT a record of pKF, the NOOP_SAME state, is searched with the descriptor it had when the Fuse call
 *    began; the reference would search with the one an earlier turn of the same call recomputed, if that turn made it a survivor).
 *    The descriptor rows of points that end the call bad are unspecified.
 *  - With ABORT_BA the call ends after stage 1.  Otherwise the candidates (:1015-1038): the targets in order, each in feature order, from the
 *    live d_kf_mp, -1 and bad points skipped, first occurrence wins; then one Fuse(current, candidates).
 * A d_kf_mp entry, list entry, ordered-row entry or count, prev link, record, CSR range, key-frame row range (n_feat above cap_feat, rows or
 * descriptor rows outside their slabs) or a list point's desc_row that cannot be read sets ORBM_FUSENB_BAD_INDEX and is treated as absent;
 * a record that two CSR ranges claim belongs to one of them and is flagged.  cap_targets sizes the chain: every possible Fuse call costs 7
 * short launches whether it exists or not (an idle one a few microseconds), so size it to the targets expected (ORB-SLAM3 sees 20 to 40),
 * not to ORBM_FUSENB_MAX_TARGETS.  A fixed number of launches on `stream` (7 per possible Fuse call, cap_targets + 1 of them, and 8 around them), nothing
 * read on the host, graph-capturable, integer atomics only: deterministic.  ORB_E_INVALID for null pointers (d_mp_nobs, d_found, d_visible
 * and arrays of count 0 excepted), negative counts, capacities below 1 (cap_obs_out below 0), cap_targets above ORBM_FUSENB_MAX_TARGETS, cap_feat outside 1..65535, nlevels outside
 * 1..16, misaligned d_mp, descriptor slabs or workspace. */
int orbm_search_in_neighbors(const orbm_localmap_view* view, const orbm_fusenb_in* in, const orbm_fusenb_params* params,
                             const orbm_fusenb_out* out, void* d_work, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * New key frame: the two steps at the head of LocalMapping::Run on the device map.  LocalMapping::ProcessNewKeyFrame's association loop
 * (LocalMapping.cc:375-411) with MapPoint::AddObservation (MapPoint.cc:160-195), UpdateNormalAndDepth and ComputeDistinctiveDescriptors;
 * LocalMapping::MapPointCulling (:435-494) with the map effects of MapPoint::SetBadFlag (MapPoint.cc:254-277); and mlpRecentAddedMapPoints,
 * the list the two share with CreateNewMapPoints (:903).  With them one iteration runs from the upload of the new key frame's own rows to
 * orbm_apply_keyframe_culling with no map transfer.  The rest of ProcessNewKeyFrame is the caller's: ComputeBoW (bow_transform) before,
 * orbm_update_connections right after on the same stream (:415), and mpAtlas->AddKeyFrame.
 * Single-camera key frames only (NLeft == -1, no mpCamera2).  An ORBM_OBS_RIGHT record is treated as absent and sets ORBM_NEWKF_UNSUPPORTED.
 * Nothing here is serial in its effects: a point's turn reads that point's own state, and a point that occurs twice is settled by a
 * first-occurrence rule (an integer atomicMin).  Integer work and decisions only, apart from the one float division of the found ratio:
 * every output is the reference's, bit for bit.
 * ------------------------------------------------------------------------------------------------------- */
/* The inputs beyond the view (a host struct of device pointers). */
typedef struct orbm_newkf_in {
    const orbm_cull_keyframe* d_ckf;         /* [n_kf]: id (mnId) and desc_row0 are read */
    const uint8_t* d_feat;                   /* [n_kf_mp_rows] ORBM_CULL_FEAT_*: ORBM_CULL_FEAT_STEREO decides the nObs weight */
    const orbm_refresh_point* d_ref;         /* [n_mp] as orbm_refresh_map_points reads it (orbm_process_new_keyframe) */
    const orbm_keyframe_center* d_center;    /* [n_kf] likewise */
    const uint8_t* d_kf_desc;                /* [n_kf_desc_rows][32] key-frame descriptor slab, 16-byte aligned (orbm_process_new_keyframe) */
    const int32_t* d_found;                  /* [n_mp] mnFound (orbm_cull_map_points) */
    const int32_t* d_visible;                /* [n_mp] mnVisible (orbm_cull_map_points) */
    const uint32_t* d_first_kf_id;           /* [n_mp] mnFirstKFid (orbm_cull_map_points) */
    int32_t n_kf_desc_rows;
    int32_t cap_feat;                        /* the greatest n_feat the current key frame may have, >= 1 (orbm_process_new_keyframe) */
} orbm_newkf_in;

/* What orbm_process_new_keyframe folds into the map and what it reports. */
typedef struct orbm_newkf_out {
    orbm_map_point* d_mp;            /* [n_mp] the view's records: ORBM_MP_HAS_OBS of the points that gained a record, then the refresh */
    int32_t* d_mp_nobs;              /* [n_mp] MapPoint::nObs, in/out, or NULL: the weighted record sum, exactly as in orbm_cull_in */
    uint8_t* d_mp_desc;              /* [n_desc_rows][32] the map-point descriptor slab, 16-byte aligned */
    uint8_t* d_code;                 /* [cap_feat] ORBM_NEWKF_CODE_* of every feature; all cap_feat entries are written */
    int32_t* d_sel;                  /* [cap_feat] the points that gained a record, in feature order, padded with -1 */
    int32_t* d_obs_start_out;        /* [n_mp + 1] the merged CSR (never the view's own arrays) */
    orbm_observation* d_obs_out;     /* [cap_obs_out] */
    int32_t* d_recent;               /* [cap_recent] mlpRecentAddedMapPoints */
    int32_t* d_n_recent;             /* its in/out cursor */
    int32_t* d_result;               /* [ORBM_NEWKF_R_WORDS] */
    int32_t n_desc_rows, cap_obs_out, cap_recent, reserved;
} orbm_newkf_out;
/* d_code of a feature */
#define ORBM_NEWKF_CODE_NOT_VISITED 0   /* past the key frame's n_feat, or the key frame could not be read */
#define ORBM_NEWKF_CODE_NONE 1          /* mvpMapPoints[i] is null (:378) */
#define ORBM_NEWKF_CODE_BAD_POINT 2     /* isBad() (:380) */
#define ORBM_NEWKF_CODE_ADDED 3         /* AddObservation, UpdateNormalAndDepth, ComputeDistinctiveDescriptors (:384-400) */
#define ORBM_NEWKF_CODE_PUSHED 4        /* the point has a record of the key frame in the map as given: mlpRecentAddedMapPoints.push_back (:406) */
#define ORBM_NEWKF_CODE_PUSHED_DUP 5    /* a feature before this one added the record: the same push */
#define ORBM_NEWKF_CODE_BAD_INDEX 6     /* the entry is out of range or names an empty slot: treated as null */
/* d_result words (orbm_recent_points_push and orbm_cull_map_points write the same five) */
#define ORBM_NEWKF_R_FLAGS 0              /* ORBM_NEWKF_* flag bits below */
#define ORBM_NEWKF_R_N_ADDED 1            /* records added; orbm_cull_map_points: points culled */
#define ORBM_NEWKF_R_N_PUSHED 2           /* entries appended to the recent list; orbm_cull_map_points: entries of the surviving list */
#define ORBM_NEWKF_R_N_PUSH_REQUIRED 3    /* the pushes the reference makes; orbm_cull_map_points: the entries read */
#define ORBM_NEWKF_R_N_OBS 4              /* the records the merged CSR needs */
#define ORBM_NEWKF_R_WORDS 8
/* flag bits */
#define ORBM_NEWKF_BAD_INDEX 1u           /* an index was out of range or named an empty slot: never read through, treated as absent */
#define ORBM_NEWKF_UNSUPPORTED 2u         /* a point of the call holds an ORBM_OBS_RIGHT record (a rig): treated as absent */
#define ORBM_NEWKF_OBS_OVERFLOW 4u        /* the merged CSR does not fit cap_obs_out: d_code and d_result were written and NOTHING else */
#define ORBM_NEWKF_RECENT_OVERFLOW 8u     /* the pushes did not all fit cap_recent: the first that fit were appended */
#define ORBM_NEWKF_REFRESH_OVERFLOW 16u   /* a point reached more than ORBM_REFRESH_MAX_OBS usable records: the refresh left it alone */
#define ORBM_NEWKF_UNSORTED 32u           /* a point's input records were not in d_kf_by_order rank order: they were copied as they lie */
/* mode bits of orbm_cull_map_points */
#define ORBM_MPCULL_MONOCULAR 1u          /* mbMonocular: nThObs = 2 instead of 3 */

/* Bytes of d_work for orbm_process_new_keyframe, a multiple of 16 (0 for an argument out of range); orbm_cull_map_points needs no more
 * than that of cap_feat = 1.  d_work is 16-byte aligned. */
size_t orbm_newkf_workspace_bytes(int n_kf, int n_mp, int cap_feat);

/* The association loop of LocalMapping::ProcessNewKeyFrame for the key frame current_kf.  PRECONDITION: its slot is in the view with
 * ORBM_LM_KF_PRESENT and the caller has uploaded what Tracking made: its d_kf_mp row, d_feat, d_ckf[current_kf].{id, desc_row0},
 * d_center[current_kf] and its descriptor rows.  view: d_mp, d_obs_start, d_obs, d_kf, d_kf_mp and d_kf_by_order are read; a slot of d_mp
 * without ORBM_MP_VALID has no records and its d_obs_start entry is not read, so the slabs of orbm_append_new_map_points can be passed whole.
 * Per feature i in feature order, p = d_kf_mp[mp_row0 + i]:
 *  - p == -1, or the point is ORBM_MP_BAD: nothing (CODE_NONE, CODE_BAD_POINT).
 *  - p has a record of current_kf in the map as given (IsInKeyFrame is membership in the records, not in d_kf_mp): EVERY such feature pushes
 *    p onto the recent list (CODE_PUSHED), so a point that sits in two features of such a key frame is pushed twice.
 *  - otherwise the first feature holding p (the least i) does AddObservation(current_kf, i) (CODE_ADDED): p gains the record {kf = current_kf,
 *    desc_row = desc_row0 + i, flags = ORBM_OBS_KF_BAD iff the slot is ORBM_LM_KF_BAD}, inserted before the first usable record of p whose
 *    key frame has a greater rank in d_kf_by_order (std::map<KeyFrame*, .> order: it decides the descriptor tie-break); nObs rises by 2 with
 *    ORBM_CULL_FEAT_STEREO of the feature, else by 1, from d_mp_nobs or, with NULL, from the weighted sum of the usable records;
 *    ORBM_MP_HAS_OBS = nObs > 0.  Every later feature holding p finds it in the key frame and pushes it (CODE_PUSHED_DUP).
 * Outputs: d_code; d_sel; the merged CSR d_obs_start_out / d_obs_out, every point's rows copied as they lie (slots without ORBM_MP_VALID and
 * points whose CSR range cannot be read get zero rows, so d_obs_start_out[cursor] is the end and the result is a valid input of
 * orbm_append_new_map_points); d_mp_nobs; the recent list, the pushes appended in feature order behind *d_n_recent (a cursor outside
 * [0, cap_recent] is clamped and flagged ORBM_NEWKF_BAD_INDEX); d_result.  Then orbm_refresh_map_points(NORMAL_DEPTH | DESCRIPTOR) runs over
 * d_sel on the merged CSR (:398-400; it IS that entry point, so its lower-median, first-least-row, ORBM_OBS_KF_BAD and
 * ORBM_REFRESH_MAX_OBS rules hold; params gives nlevels and scale_factors, its `what` is not read): a point it left alone sets
 * ORBM_NEWKF_REFRESH_OVERFLOW.
 * Overflows are reported, never silent: the CSR's is decided before anything is written (ORBM_NEWKF_OBS_OVERFLOW: d_code names the
 * decisions, d_result has N_ADDED = N_PUSHED = 0, the map, d_sel and the recent list stay as given); the recent list takes the first
 * pushes that fit.  A d_kf_mp entry, record (key frame, row outside the key frame's features), CSR range, the key frame's own rows (n_feat
 * above cap_feat, rows or descriptor rows outside their slabs: then no feature is visited) that cannot be read sets ORBM_NEWKF_BAD_INDEX
 * and is treated as absent.  Eight launches on `stream` whatever the sizes (state, association, count, scan and selection, write, the two
 * of the refresh, result), nothing read on the host, integer atomics only: deterministic.  ORB_E_INVALID for null
 * pointers (d_mp_nobs, the three arrays only orbm_cull_map_points reads, and arrays of count 0 excepted), negative counts, cap_feat or
 * cap_recent below 1, cap_obs_out below 0, nlevels outside 1..16, misaligned d_mp, descriptor slabs or workspace. */
int orbm_process_new_keyframe(const orbm_localmap_view* view, const orbm_newkf_in* in, int current_kf, const orbm_refresh_params* params,
                              const orbm_newkf_out* out, void* d_work, void* stream);

/* mlpRecentAddedMapPoints.push_back (LocalMapping.cc:903) for the points orbm_append_new_map_points made: the non-negative entries of
 * d_list[0 .. n_list) (its d_sel, padded with -1) are appended to d_recent behind *d_n_recent, in order, with the cursor and overflow rule
 * above; d_result as above (N_ADDED = N_OBS = 0).  One launch, asynchronous on `stream`.  ORB_E_INVALID for null pointers, n_list < 0,
 * cap_recent < 1. */
int orbm_recent_points_push(const int32_t* d_list, int n_list, int32_t* d_recent, int32_t* d_n_recent, int cap_recent, int32_t* d_result,
                            void* stream);

/* What orbm_cull_map_points writes. */
typedef struct orbm_mpcull_out {
    orbm_map_point* d_mp;            /* [n_mp] the view's records: ORBM_MP_BAD or-ed into the culled points */
    int32_t* d_kf_mp;                /* [n_kf_mp_rows] the view's table: EraseMapPointMatch of every record of a culled point */
    uint8_t* d_code;                 /* [cap_recent] ORBM_MPCULL_CODE_* of every list entry; all cap_recent entries are written */
    int32_t* d_recent_out;           /* [cap_recent] the surviving list; never the input list */
    int32_t* d_n_recent_out;         /* its count */
    int32_t* d_culled;               /* [cap_recent] the culled points in list order (the caller replays mpMap->EraseMapPoint), padded with -1 */
    int32_t* d_n_culled;
    int32_t* d_obs_start_out;        /* [n_mp + 1] the CSR without the culled points' rows (never the view's own arrays) */
    orbm_observation* d_obs_out;     /* [cap_obs_out]: it can only shrink, n_obs is enough */
    int32_t* d_result;               /* [ORBM_NEWKF_R_WORDS] */
    int32_t cap_obs_out, cap_recent;
} orbm_mpcull_out;
/* d_code of a list entry, the reference's `else if` chain in its order */
#define ORBM_MPCULL_CODE_NOT_VISITED 0    /* past the list's count, or current_kf could not be read */
#define ORBM_MPCULL_CODE_ERASED_BAD 1     /* isBad() (:458): erased from the list; also every later occurrence of a point culled before it */
#define ORBM_MPCULL_CODE_CULLED_RATIO 2   /* GetFoundRatio() < 0.25f (:460) */
#define ORBM_MPCULL_CODE_CULLED_OBS 3     /* (int)nCurrentKFid - (int)mnFirstKFid >= 2 && Observations() <= cnThObs (:465) */
#define ORBM_MPCULL_CODE_RETIRED 4        /* the difference >= 3 (:470): erased from the list, not bad */
#define ORBM_MPCULL_CODE_KEPT 5           /* stays in the list */
#define ORBM_MPCULL_CODE_BAD_INDEX 6      /* the entry is out of range or names an empty slot: dropped from the list */

/* LocalMapping::MapPointCulling over the recent list d_recent[0 .. *d_n_recent) for the key frame current_kf (d_ckf[current_kf].id is
 * nCurrentKFid), in the order of the reference's `else if` chain: bad; float(mnFound) / mnVisible < 0.25f, the correctly rounded float
 * division of the two converted integers (mnVisible == 0 gives inf or NaN exactly as the comparison sees it); the id difference on 32-bit
 * signed casts >= 2 with nObs <= nThObs (2 with ORBM_MPCULL_MONOCULAR, else 3; nObs from d_mp_nobs or, with NULL, the weighted sum of
 * the usable records); the difference >= 3; else kept.  A point created by a later key frame gives a negative difference and is kept.
 * A point that is in the list twice: the first occurrence decides; if it was culled every later occurrence takes CODE_ERASED_BAD, otherwise
 * every occurrence takes the same exit.  Effects of a cull (SetBadFlag): ORBM_MP_BAD or-ed in; the point's rows leave the CSR;
 * d_kf_mp[mp_row0(kf) + desc_row - desc_row0(kf)] = -1 for every usable record, unconditionally (EraseMapPointMatch(idx), even where the
 * slot holds another point); nObs, found and visible stay.  ORBM_NEWKF_OBS_OVERFLOW as above: d_code and d_result only.  Bad indices and
 * rig records as above; a current_kf that cannot be read is one, and then no entry is visited and the surviving list is empty.  Five launches on `stream` whatever the sizes (state, decision, count, scan and compaction, write), nothing read on
 * the host, deterministic.  ORB_E_INVALID for null pointers (d_mp_nobs and arrays of count 0 excepted), negative counts,
 * cap_recent below 1, cap_obs_out below 0, unknown mode bits, d_recent_out == d_recent, misaligned d_mp or workspace. */
int orbm_cull_map_points(const orbm_localmap_view* view, const orbm_newkf_in* in, const int32_t* d_mp_nobs, int current_kf, uint32_t flags,
                         const int32_t* d_recent, const int32_t* d_n_recent, const orbm_mpcull_out* out, void* d_work, void* stream);

/* The same search for key frames whose cameras are KannalaBrandt8 (BASELINE configs[3]): a monocular fisheye camera
 * (n_cams = 1) or a fisheye rig with mpCamera2 (n_cams = 2; kps / desc = the concatenation [mvKeys | mvKeysRight] like a rig Frame — NOT
 * mvKeysUn, ORBmatcher.cc:1249-1251 — with d_nleft*[b] = NLeft, features >= NLeft belong to the right camera).  The gate is
 * KannalaBrandt8::epipolarConstrain = TriangulateMatches(pCamera2, kp1, kp2, R12, t12, mvLevelSigma2_1[kp1.octave], mvLevelSigma2_2[kp2.octave]) >
 * 0.0001f (KannalaBrandt8.cpp:235-238, 334-400) with the (camera, R12, t12) combination chosen per candidate from (bRight1, bRight2)
 * (ORBmatcher.cc:1280-1315).  bStereo1 / bStereo2 are false for such key frames (u_right of the sides is ignored), so only_stereo yields no
 * match; the epipole test (:1269-1277) applies only when n_cams = 1.  The float32 cv::Mat / libm / cv::SVD steps inside TriangulateMatches
 * follow rule R4, like orbf_stereo_fisheye_matches: parity vs a real OpenCV build is unpinned for them. */
typedef struct orbm_tri_kb8_pair {
    int32_t n_cams, reserved;
    float k1[2][8], k2[2][8];     /* mvParameters of pKF1->mpCamera / mpCamera2 and of pKF2->mpCamera / mpCamera2 */
    float R12[4][9], t12[4][3];   /* row-major, index bRight1*2 + bRight2: Rll, Rlr, Rrl, Rrr / tll, tlr, trl, trr (ORBmatcher.cc:1181-1193) as the adapter's
                                   * cv::Mat expressions evaluate them; n_cams = 1: entry 0 = R12, t12 (:1176-1177) */
    float ep[2];                  /* pKF2->mpCamera->project(R2w*Cw + t2w) (:1149-1152); read only when n_cams = 1 */
    float level_sigma2_1[16], level_sigma2_2[16], scale_factors_2[16];   /* pKF1->mvLevelSigma2, pKF2->mvLevelSigma2, pKF2->mvScaleFactors */
} orbm_tri_kb8_pair;
int orbm_search_for_triangulation_kb8(const orbm_tri_side* kf1, const orbm_tri_side* kf2, const int32_t* d_nleft1, const int32_t* d_nleft2,
                                      const orbm_tri_kb8_pair* d_pairs, int batch, int only_stereo, int coarse, int check_orientation,
                                      int32_t* d_match12, int32_t* d_nmatches, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:323-587, Nleft == -1 branch).
 * FeatureVector of each side as CSR: node ids ascending (std::map order), node_start[k..k+1] delimit feat_idx[] (the
 * feature indices of that node in insertion order).  kf_valid[i] != 0 where the KF feature holds a good map point.
 * Output f_match[b][j] = KF feature index matched to frame feature j or -1 (vpMapPointMatches), nmatches[b]. */
typedef struct orbm_bow_side {
    const uint8_t* desc;          /* [batch][cap_f][32] */
    const float* angle;           /* [batch][cap_f]  keypoint angles */
    const int32_t* node_id;       /* [batch][cap_nodes] ascending */
    const int32_t* node_start;    /* [batch][cap_nodes+1] */
    const int32_t* feat_idx;      /* [batch][cap_f] */
    const int32_t* n_nodes;       /* [batch] */
    int32_t cap_f, cap_nodes;
    const int32_t* n_left;        /* frame side only: [batch] F.Nleft of a fisheye rig (features >= Nleft belong to the right camera), or
                                   * NULL / -1 for a single camera.  Rig frames take the `F.Nleft != -1` branch of ORBmatcher.cc:411-436:
                                   * separate best/second for the left and the right features of a node; the right match is accepted
                                   * whenever the left best passed TH_LOW and bestDist1R <= TH_LOW (the `|| true` of :509) */
} orbm_bow_side;
int orbm_search_by_bow(const orbm_bow_side* kf, const uint8_t* d_kf_valid, const orbm_bow_side* f, int batch,
                       float nn_ratio, int check_orientation, int32_t* d_f_match, int32_t* d_nmatches, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (ORBmatcher.cc:984-1124; call site
 * LoopClosing.cc:697).  Both FeatureVectors as CSR (n_left of the sides is ignored).  valid1[i] / valid2[i] != 0 where the key frame's
 * feature i holds a map point that is not bad (:1025-1028, :1049-1053) and, for a fisheye-rig key frame (NLeft != -1), i < mvKeysUn.size()
 * (:1020-1022, :1043-1045) — the adapter folds both conditions into the flag.  Output match12[b][i1] = index of the pKF2 feature whose
 * map point vpMatches12[i1] holds, or -1 ([batch][kf1->cap_f]); nmatches[b] = the return value.  Unlike the (KeyFrame, Frame) overload the
 * acceptance is `bestDist1 < TH_LOW` (strict, :1072) and a pKF2 feature is taken at most once (vbMatched2, :1077). */
int orbm_search_by_bow_kf(const orbm_bow_side* kf1, const uint8_t* d_valid1, const orbm_bow_side* kf2, const uint8_t* d_valid2, int batch,
                          float nn_ratio, int check_orientation, int32_t* d_match12, int32_t* d_nmatches, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * SURVEY.md N2 — the DBoW2 step between the extractor and SearchByBoW: Frame::ComputeBoW (reference src/Frame.cc:865-872) =
 * TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup = 4)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1137-1206; per-descriptor tree descent :1231-1272 with FORB::distance, FORB.cpp:81-101),
 * on a vocabulary in the binary format System.cc:83 loads (loadFromBinaryFile, TemplatedVocabulary.h:1442-1480:
 * header u32 nb_nodes, u32 size_node, i32 k, i32 L, i32 scoring, i32 weighting; then nb_nodes records
 * {i32 parent, 32 B descriptor, f32 weight, u8 is_leaf}; node ids 1..nb_nodes in file order, word ids in leaf order).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct bow_vocab* bow_vocab_handle;
/* Parses the file image (host memory) and uploads the tree.  ORB_E_INVALID for a short or inconsistent file. */
int bow_vocab_load_binary(const void* file_bytes, size_t n_bytes, int device, bow_vocab_handle* out);
/* out6 = {k, L, scoring (DBoW2::ScoringType), weighting (DBoW2::WeightingType), nodes (without the root), words} */
int bow_vocab_info(bow_vocab_handle v, int32_t* out6);
void bow_vocab_destroy(bow_vocab_handle v);

/* Outputs of one transform() per frame, fixed-capacity slabs (device pointers; frame b uses x + b*cap_f, ...):
 *   per feature i (what transform(feature, id, w, &nid, levelsup) returns): word_id, node_id (NodeId at level L - levelsup), weight;
 *   FeatureVector (std::map<NodeId, vector<uint>>) as the CSR orbm_search_by_bow / orbm_search_for_triangulation consume:
 *     fv_node_id[b][cap_f] ascending, fv_node_start[b][cap_f+1], fv_feat_idx[b][cap_f] (ascending inside a node), fv_n_nodes[b];
 *   BowVector (std::map<WordId, double>) as bv_word[b][cap_f] ascending, bv_value[b][cap_f], bv_n[b] — summed / normalised in
 *     the reference's order (BowVector.cpp:34-84), so the doubles are bit-identical.
 * Features whose word weight is 0 ("stopped") appear in neither vector.  cap_f <= 4096. */
typedef struct bow_result {
    int32_t* word_id; int32_t* node_id; double* weight;
    int32_t* fv_node_id; int32_t* fv_node_start; int32_t* fv_feat_idx; int32_t* fv_n_nodes;
    int32_t* bv_word; double* bv_value; int32_t* bv_n;
} bow_result;
int bow_transform(bow_vocab_handle v, const uint8_t* d_desc, const int32_t* d_n, int count_stride, int cap_f, int batch, int levelsup,
                  const bow_result* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Place recognition — KeyFrameDatabase::DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:785-897; call site
 * Tracking.cc:3260) and KeyFrameDatabase::DetectNBestCandidates (:614-782; call site LoopClosing.cc:513) with L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), over a key-frame database whose rows live in caller-owned device slabs.
 *
 * A database is n_slots rows; slot = the caller's key-frame index.  Row s holds the key frame's BowVector exactly as bow_transform writes
 * it (bv_word + s*cap_f ascending, bv_value + s*cap_f, bv_n[s]), so bow_transform with out->bv_word = db.bv_word + s*cap_f IS the data
 * movement of KeyFrameDatabase::add.  There is no inverted file: every query streams the present rows (DESIGN.md "Place recognition").
 * erase = the caller clears BOWDB_KF_PRESENT; clear / clearMap = the same over many slots.  Precondition: a bad key frame is not present
 * (KeyFrame::SetBadFlag erases it first, KeyFrame.cc:784), and the BowVector values are finite.
 * ------------------------------------------------------------------------------------------------------- */
#define BOWDB_KF_PRESENT 1u
#define BOWDB_COVIS 10          /* GetBestCovisibilityKeyFrames(10) */
#define BOWDB_MAX_CANDIDATES 64 /* largest nNumCandidates of bowdb_detect_n_best_candidates */
#define BOWDB_L1_NORM 0         /* DBoW2::L1_NORM (BowVector.h:45-53), the scoring of ORBvoc; the only one supported */
typedef struct bowdb_keyframe {
    uint32_t flags;             /* BOWDB_KF_PRESENT */
    int32_t map_id;             /* pKF->GetMap() */
    uint32_t seq;               /* the caller's running count of add() calls when this key frame was added: its position inside every list of the
                                 * reference's inverted file (filled by push_back, so erase + add moves a key frame to the back).  Unique per slot. */
    int32_t covis[BOWDB_COVIS]; /* slots of GetBestCovisibilityKeyFrames(10) in order, -1 padded; an entry that is out of range or not present is skipped */
} bowdb_keyframe;               /* 52 B */

/* The per-slot query state is part of the contract, not scratch: the covisibility accumulation reads the score of every neighbour whose
 * last_query equals the current id, including neighbours that shared a word but were not scored in this query — their score is the one an
 * earlier query left.  Two families kept apart as the reference keeps mnRelocQuery / mRelocScore apart from mnPlaceRecognitionQuery /
 * mPlaceRecognitionScore; the caller zeroes a slot's four entries when it (re)adds the key frame.  (The reference never initialises
 * mRelocScore; here its initial value is 0.0f.) */
typedef struct bowdb_view {
    const int32_t* bv_word;     /* [n_slots][cap_f] ascending */
    const double* bv_value;     /* [n_slots][cap_f] */
    const int32_t* bv_n;        /* [n_slots] */
    const bowdb_keyframe* kf;   /* [n_slots] */
    uint64_t* reloc_query;      /* [n_slots]  mnRelocQuery */
    float* reloc_score;         /* [n_slots]  mRelocScore */
    uint64_t* place_query;      /* [n_slots]  mnPlaceRecognitionQuery */
    float* place_score;         /* [n_slots]  mPlaceRecognitionScore */
    const uint8_t* map_bad;     /* [n_maps]   Map::IsBad(); a map_id outside [0, n_maps) counts as not bad */
    int32_t n_slots, cap_f, n_maps;
    int32_t scoring;            /* BOWDB_L1_NORM */
} bowdb_view;

typedef struct bowdb_query {    /* device records, so that a captured graph can be replayed with new ids */
    uint64_t id;                /* F->mnId / pKF->mnId */
    int32_t map_id;             /* pMap / pKF->GetMap() */
    int32_t row;                /* row of the query's BowVector in the query slab; outside [0, n_rows): an empty query */
    int32_t conn_start, conn_n; /* N-best only: d_conn[conn_start .. conn_start + conn_n) = slots of pKF->GetConnectedKeyFrames() */
} bowdb_query;                  /* 24 B */

typedef struct bowdb_query_bows {   /* bow_transform output again; it may alias database rows */
    const int32_t* q_word;      /* [n_rows][cap_q] ascending */
    const double* q_value;      /* [n_rows][cap_q] */
    const int32_t* q_n;         /* [n_rows] */
    int32_t n_rows, cap_q;
} bowdb_query_bows;

typedef struct bowdb_stats {
    int32_t n_sharing;          /* lKFsSharingWords.size() */
    int32_t max_common_words;   /* maxCommonWords */
    int32_t n_scored;           /* nscores */
    float best_acc_score;       /* bestAccScore */
} bowdb_stats;                  /* 16 B */

/* Per query with id q and BowVector v, over the present slots (for N-best: those not in the query's conn list, whose state is not touched):
 *  1. A key frame is listed iff it shares at least one word with v; words = the number of common words.  List order = the order of first
 *     encounter in the reference's walk = ascending (first common word, seq).  Every listed key frame gets last_query = q.
 *  2. minCommonWords = (int)((float)maxCommonWords * 0.8f); scored iff words > minCommonWords.
 *  3. score = (float)(-s / 2.0) with s += fabs(vi - wi) - fabs(vi) - fabs(wi) in double over the common words in ascending order, one term
 *     at a time (vi the query's value, wi the key frame's).  Stored in the slot's score.
 *  4. After all scores of the query are stored, per scored key frame i in list order: best = acc = score[i], bestKF = i; for each covis entry
 *     n in order with last_query[n] == q: acc += score[n]; if (score[n] > best) { bestKF = n; best = score[n]; }.
 *     bestAccScore = the largest acc, at least 0.
 *  5. Relocalisation: in list order the entries with acc > 0.75f * bestAccScore whose bestKF has the query's map_id, first occurrence of
 *     each bestKF.  d_cand [n_queries][cap_cand] receives what fits, in order; d_n_cand[k] = entries written, d_n_required[k] = the full
 *     count (> cap_cand: overflow, nothing is truncated silently).
 *  6. N-best: the (acc, bestKF) list sorted by acc descending, equal acc in list order (std::list::sort is stable); first occurrence of each
 *     bestKF; same map -> d_loop while it holds fewer than n_candidates, other map whose map is not bad -> d_merge likewise.
 *     d_loop / d_merge are [n_queries][n_candidates], unused entries -1.
 *  7. The queries of one call behave as if run one after another in index order.
 * With ids that are not 0 and were never used before on the database in that family (Frame::mnId, the loop closer's key-frame ids) this is
 * what the reference computes; the rules hold as written for any id.  The query key frame of an N-best call is normally not present yet
 * (LoopClosing adds it after detection); if it is, list it in conn or it finds itself.
 * d_stats may be NULL.  d_workspace: bowdb_workspace_bytes(n_slots, n_queries) bytes, 16-byte aligned, contents irrelevant.
 * Asynchronous on `stream`: every launch goes to that one stream, no host synchronisation, no allocation, graph-capturable.
 * ORB_E_INVALID (nothing launched) for null pointers (d_stats excepted; d_conn may be NULL when every conn_n is 0 — it is not read then),
 * scoring != BOWDB_L1_NORM, cap_f or cap_q outside 1..4096, negative counts, cap_cand < 0, n_candidates outside 1..BOWDB_MAX_CANDIDATES.
 * n_queries == 0 is a successful no-op; n_slots == 0 gives empty results. */
size_t bowdb_workspace_bytes(int n_slots, int n_queries);
int bowdb_detect_relocalization_candidates(const bowdb_view* db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows* q,
                                           int32_t* d_cand, int cap_cand, int32_t* d_n_cand, int32_t* d_n_required, bowdb_stats* d_stats,
                                           void* d_workspace, void* stream);
int bowdb_detect_n_best_candidates(const bowdb_view* db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows* q,
                                   const int32_t* d_conn, int n_conn, int n_candidates, int32_t* d_loop, int32_t* d_n_loop, int32_t* d_merge,
                                   int32_t* d_n_merge, bowdb_stats* d_stats, void* d_workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stage 3 — Optimizer::LocalBundleAdjustment's linearisation  (reference src/Optimizer.cc:1957-2344 graph,
 * src/OptimizableTypes.{h,cpp} edges, Thirdparty/g2o core/block_solver.hpp:502-560 buildSystem,
 * core/base_binary_edge.hpp:55-120 constructQuadraticForm, core/robust_kernel_impl.cpp:78-91 Huber).
 * The adapter (include/orbslam3_hip/Optimizer.h) flattens the g2o graph into the SoA below once per optimize()
 * call (== BlockSolver::buildStructure) and then asks for one linearisation per LM iteration / trial.
 * `batch` independent windows use fixed-capacity slabs like stage 2; all pointers are device pointers, all
 * matrices are column-major doubles as in g2o's Eigen::Map blocks.
 * ------------------------------------------------------------------------------------------------------- */
#define LBA_EDGE_MONO 0    /* ORB_SLAM3::EdgeSE3ProjectXYZ        OptimizableTypes.h:102-130, .cpp:142-172 */
#define LBA_EDGE_STEREO 1  /* g2o::EdgeStereoSE3ProjectXYZ        types_six_dof_expmap.h:146-175, .cpp:190-275 */
#define LBA_EDGE_BODY 2    /* ORB_SLAM3::EdgeSE3ProjectXYZToBody  OptimizableTypes.h:132-159, .cpp:204-225 */
#define LBA_CAM_PINHOLE 0  /* CameraModels/Pinhole.cpp:43-49, 89-100 */
#define LBA_CAM_KB8 1      /* CameraModels/KannalaBrandt8.cpp:52-66, 166-196 */

typedef struct lba_camera {
    int32_t model, reserved;
    double p[8];        /* mvParameters (float values widened): fx fy cx cy [k1 k2 k3 k4] */
    double bf;          /* stereo baseline * fx (EdgeStereoSE3ProjectXYZ::bf) */
    double trl_q[4];    /* mTrl rotation as quaternion x y z w (body edges) */
    double trl_t[3];    /* mTrl translation */
} lba_camera;

typedef struct lba_edge {      /* one observation; edges are stored landmark-major (Optimizer.cc:2060-2190 insertion order) */
    int32_t pose, point;       /* indices into the window's pose / point arrays */
    int16_t kind, cam;         /* LBA_EDGE_*, index into cameras */
    float obs[3];              /* kpUn.pt.x, kpUn.pt.y, mvuRight (stereo) — float in the map, widened on use */
    float inv_sigma2;          /* mvInvLevelSigma2[octave]; information = I * inv_sigma2 */
} lba_edge;

typedef struct lba_problem {
    /* vertices */
    const double* poses;        /* [batch][cap_p][7]  SE3Quat estimate: t(x y z), q(x y z w) */
    const int32_t* pose_hidx;   /* [batch][cap_p]     Hessian block index of the pose (ascending KF id), -1 = fixed vertex */
    const double* points;       /* [batch][cap_l][3]  VertexSBAPointXYZ estimates */
    /* edges + the two CSR views built once per optimize() (BlockSolver::buildStructure, block_solver.hpp:143-295) */
    const lba_edge* edges;      /* [batch][cap_e] */
    const int32_t* lm_start;    /* [batch][cap_l+1]   edges of landmark l are [lm_start[l], lm_start[l+1]) */
    const int32_t* pose_start;  /* [batch][cap_p+1]   CSR over pose_edges */
    const int32_t* pose_edges;  /* [batch][cap_e]     edge indices of each pose, ascending */
    const lba_camera* cameras;  /* [n_cameras] shared by the batch */
    const int32_t* n_poses;     /* [batch] */
    const int32_t* n_points;    /* [batch] */
    const int32_t* n_edges;     /* [batch] */
    int32_t cap_p, cap_l, cap_e, n_cameras;
    double huber_mono, huber_stereo;   /* thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815); <= 0 disables the kernel */
} lba_problem;

typedef struct lba_system {     /* outputs; any pointer may be NULL to skip that product */
    double* Hpp;     /* [batch][cap_p][36]  6x6 block of free pose hidx (rotation first, then translation) */
    double* bp;      /* [batch][cap_p][6] */
    double* Hll;     /* [batch][cap_l][9] */
    double* bl;      /* [batch][cap_l][3] */
    double* Hpl;     /* [batch][cap_e][18]  logical 6x3 block H(pose, landmark) of each edge with a free pose (else zeros) */
    double* err;     /* [batch][cap_e][3]   _error = obs - projection */
    double* chi2;    /* [batch][cap_e]      e^T Omega e */
    double* rho;     /* [batch][cap_e][2]   Huber rho[0], rho[1] */
    double* depth;   /* [batch][cap_e]      z of the point in the (projecting) camera frame: isDepthPositive() */
    double* robust_chi2_sum;  /* [batch]    sum of rho[0] = SparseOptimizer::activeRobustChi2 (sparse_optimizer.cpp:100-114) */
} lba_system;

/* BlockSolver::buildSystem (block_solver.hpp:502-560): linearizeOplus + constructQuadraticForm over all active edges. */
int lba_build_system(const lba_problem* prob, int batch, const lba_system* out, void* stream);
/* The same with what the caller knows about the graph it flattened.  LBA_HINT_MONO_PINHOLE: EVERY edge of the batch is an EdgeSE3ProjectXYZ
 * (LBA_EDGE_MONO) on a pinhole camera — a monocular pinhole map (Optimizer.cc:2095-2127 took the `mono` branch for every observation).  The
 * kernels specialised for it give identical results with a third fewer registers; a hint that does not hold gives wrong blocks (lba_optimize
 * checks the edges itself, once per call, and needs no hint).  Unknown hint bits: ORB_E_INVALID. */
#define LBA_HINT_MONO_PINHOLE 1u
#define LBA_HINT_PINHOLE 2u        /* every edge is LBA_EDGE_MONO or LBA_EDGE_STEREO on a pinhole camera (stereo / RGB-D pinhole maps); also for pose_optimize_hint */
int lba_build_system_hint(const lba_problem* prob, int batch, const lba_system* out, unsigned hints, void* stream);
/* SparseOptimizer::computeActiveErrors (sparse_optimizer.cpp:61-75): err / chi2 / rho / depth / robust_chi2_sum only. */
int lba_compute_errors(const lba_problem* prob, int batch, const lba_system* out, void* stream);

/* SURVEY.md N4 — the rest of one SparseOptimizer::optimize(iterations) call on the LBA graph, GPU resident:
 * OptimizationAlgorithmLevenberg::solve (g2o/core/optimization_algorithm_levenberg.cpp:61-168: _tau = 1e-50, <= 100 lambda
 * trials, rho test, the "nBad" stop), BlockSolver::setLambda / Schur complement / back-substitution
 * (block_solver.hpp:564-589, 381-481) and the vertex updates (exp(dx)*T, X += dx).  The reduced camera system is solved
 * with a dense Cholesky per window (g2o: Eigen SimplicialLDLT — same solution of the SPD system).
 * prob->poses and prob->points are UPDATED IN PLACE (they must be writable device memory).  h_stats: [batch][4] host doubles =
 * {iterations run, final activeRobustChi2, final lambda, total lambda trials}.  abort_flag (may be NULL) is polled between
 * trials like pbStopFlag (Optimizer.cc:2197-2199, sparse_optimizer.cpp:376) -> ORB_E_ABORTED.  Synchronous on `stream`. */
size_t lba_lm_workspace_bytes(const lba_problem* prob, int batch);
int lba_optimize(const lba_problem* prob, int batch, int iterations, void* d_workspace, double* h_stats,
                 const volatile int* abort_flag, void* stream);
/* The same call polling the reference's own stop flag: Optimizer::LocalBundleAdjustment gets `bool* pbStopFlag` (one byte, set by LocalMapping from
 * another thread) and passes it to g2o's setForceStopFlag (Optimizer.cc:1975-1976); pb_stop_flag may be NULL. */
int lba_optimize_stopflag(const lba_problem* prob, int batch, int iterations, void* d_workspace, double* h_stats,
                          const volatile unsigned char* pb_stop_flag, void* stream);

/* lba_optimize for windows SHARDED BY LANDMARK over several processes, one per GPU (BASELINE configs[4]; the reference solves one
 * window in one process: BlockSolver::buildSystem / solve, block_solver.hpp:381-432,502-560).  Every rank passes the whole pose set of each window and the
 * points / edges of ITS landmarks only (re-indexed from 0).  Per linearisation the pose-side blocks H_pp | b_p are summed over the ranks, per lambda
 * trial the reduced camera system [np6 x np6 | np6] and three scalars per window (chi2, computeScale, failures), once the lambda start value (max):
 * all through `reduce(user, d_buf, n, op, stream)`, which must leave d_buf[0..n) = the sum (op 0) or maximum (op 1) over all ranks of their d_buf,
 * bit-identical on every rank, ordered after the work already queued on `stream` and complete (or stream-ordered) when it returns; non-zero = failure.
 * Every rank then takes the same decisions, factorises the same system and updates ALL poses; its own landmarks are back-substituted locally.
 * owner: non-zero on exactly one rank (the terms that exist once — H_pp + lambda I, b_p, the pose part of computeScale — enter the sums there).
 * h_stats as lba_optimize, identical on every rank (chi2 of the WHOLE window).  There is no stop flag: the ranks must run the same trials. */
typedef int (*lba_allreduce_fn)(void* user, double* d_buf, size_t n, int op, void* stream);
int lba_optimize_sharded(const lba_problem* prob, int batch, int iterations, void* d_workspace, double* h_stats, int owner,
                         lba_allreduce_fn reduce, void* user, void* stream);
/* lba_optimize returns ORB_E_CAPACITY when the reduced camera system (6 unknowns per FREE key frame; fixed key frames do not count) no
 * longer fits the solver's LDS budget (> ~3 300 free key frames): nothing was changed, the window stays as it was.  A host that must optimise such a map
 * keeps its own CPU solver for it (integration/Optimizer_hip.cc REPLACES the g2o body and therefore leaves the map untouched instead — GlueGuard.h). */

/* ---------------------------------------------------------------------------------------------------------
 * Local bundle adjustment on the device map: the two halves of Optimizer::LocalBundleAdjustment around the solver.
 * orbm_lba_window_build is the window selection (Optimizer.cc:1816-1945) and the graph flattening (:1978-2190) with the two guards of
 * integration/Optimizer_hip.cc; its output IS the lba_problem of lba_optimize (batch 1).  orbm_lba_window_apply is the outlier pass, the
 * erase loop and the write-back (:2293-2510).  Between them the caller runs lba_optimize(5), lba_optimize(10), lba_compute_errors.
 * One window per call.  Single-camera pinhole key frames only (NLeft == -1, no mpCamera2); one lba_camera (index 0) and one
 * inv_level_sigma2 table per call; non-inertial maps (imu_pos is never rewritten).  An ORBM_OBS_RIGHT record is treated as absent and
 * sets ORBM_LBA_UNSUPPORTED.  pMap->IncreaseChangeIndex() and mpMap->EraseMapPoint are the caller's, replayed from the lists.
 * ------------------------------------------------------------------------------------------------------- */
/* The inputs beyond the view (a host struct of device pointers); the per-feature tables are parallel to view->d_kf_mp. */
typedef struct orbm_lba_in {
    const orbm_cull_keyframe* d_ckf;      /* [n_kf]: id (mnId) and desc_row0 are read */
    const orbm_fusenb_pose* d_pose;       /* [n_kf] Rcw | tcw (build) */
    const orb_keypoint* d_kps;            /* [n_kf_mp_rows] mvKeysUn */
    const float* d_u_right;               /* [n_kf_mp_rows] mvuRight */
    const int32_t* d_ordered_kf;          /* [n_kf][cap_conn] rows of orbm_covis_store: GetVectorCovisibleKeyFrames reads the whole row */
    const int32_t* d_n_ordered;           /* [n_kf] */
    const orbm_covis_keyframe* d_map;     /* [n_kf] map_id is read, or NULL: one map */
    int32_t cap_conn;
    int32_t nlevels;                      /* 1..16 */
    float inv_level_sigma2[16];           /* mvInvLevelSigma2 */
    float scale_factors[16];              /* mvScaleFactors (apply: UpdateNormalAndDepth) */
} orbm_lba_in;

/* The window: the arrays of an lba_problem of batch 1 (caller-owned slabs of cap_p poses, cap_l points, cap_e edges) and what ties its
 * vertices and edges to the map.  orbm_lba_window_build writes all of it, lba_optimize rewrites poses and points, apply reads it. */
typedef struct orbm_lba_window {
    double* poses;           /* [cap_p][7] local and fixed key frames in ascending mnId (g2o's block order; equal ids by slot) */
    int32_t* pose_hidx;      /* [cap_p] -1 for a fixed key frame and for a local init key frame, else a running index */
    double* points;          /* [cap_l][3] lLocalMapPoints in list order */
    lba_edge* edges;         /* [cap_e] landmark-major, per point the usable records in CSR order */
    int32_t* lm_start;       /* [cap_l + 1] entries past n_points hold n_edges */
    int32_t* pose_start;     /* [cap_p + 1] likewise */
    int32_t* pose_edges;     /* [cap_e] */
    int32_t* n_poses;        /* [1] */
    int32_t* n_points;       /* [1] */
    int32_t* n_edges;        /* [1] */
    int32_t* d_pose_kf;      /* [cap_p] the key-frame slot of vertex i */
    int32_t* d_pose_local;   /* [cap_p] 1: the key frame is in lLocalKeyFrames after the num_fixedKF < 2 branch (its pose is written back) */
    int32_t* d_point_mp;     /* [cap_l] the map-point index of vertex l, padded with -1 */
    int32_t* d_edge_rec;     /* [cap_e] the index of the edge's record in view->d_obs */
    int32_t* d_result;       /* [ORBM_LBA_R_WORDS] */
    int32_t cap_p, cap_l, cap_e, reserved;
} orbm_lba_window;
/* d_result words of orbm_lba_window_build */
#define ORBM_LBA_R_FLAGS 0            /* ORBM_LBA_* flag bits below */
#define ORBM_LBA_R_N_LOCAL 1          /* lLocalKeyFrames.size() after the branch */
#define ORBM_LBA_R_N_FIXED 2          /* lFixedCameras.size() after the branch */
#define ORBM_LBA_R_NUM_FIXED_KF 3     /* num_fixedKF as the reference returns it */
#define ORBM_LBA_R_N_POINTS 4
#define ORBM_LBA_R_N_EDGES 5
#define ORBM_LBA_R_N_MONO 6
#define ORBM_LBA_R_N_STEREO 7
#define ORBM_LBA_R_N_POSES_REQUIRED 8
#define ORBM_LBA_R_N_POINTS_REQUIRED 9
#define ORBM_LBA_R_N_EDGES_REQUIRED 10
#define ORBM_LBA_R_WORDS 12
/* flag bits (both calls) */
#define ORBM_LBA_BAD_INDEX 1u         /* an index was out of range or named an empty slot: never read through, treated as absent */
#define ORBM_LBA_UNSUPPORTED 2u       /* a point of the window holds an ORBM_OBS_RIGHT record (a rig): treated as absent */
#define ORBM_LBA_OVERFLOW 4u          /* a capacity did not hold: the flag and the three required sizes were written and NOTHING else */
#define ORBM_LBA_EARLY_RETURN 8u      /* apply: (double)n_erase >= (n_mono + n_stereo) * 0.5 (:2348-2352): the map was not written */

/* Bytes of d_work for either call, a multiple of 16 (0 for an argument out of range, which includes (cap_conn + 1) * n_kf_mp_rows above
 * INT_MAX: both calls refuse such sizes with ORB_E_INVALID); d_work is 16-byte aligned. */
size_t orbm_lba_workspace_bytes(int n_kf, int n_mp, int n_obs, int n_kf_mp_rows, int cap_conn, int cap_p, int cap_l, int cap_e);

/* Builds the window of key frame current_kf, statement by statement:
 *  - lLocalKeyFrames: current_kf, then ALL d_n_ordered[current_kf] entries of its ordered row in row order.  Every entry is marked local
 *    (mnBALocalForKF); only those that are not ORBM_LM_KF_BAD and carry current_kf's map_id are listed.  (A row that names a key frame
 *    twice, or current_kf itself, lists it once, at its first place.)
 *  - lLocalMapPoints: the local key frames in list order, each key frame's features in feature order; -1, ORBM_MP_BAD points and slots
 *    without ORBM_MP_VALID are skipped; the first occurrence wins (an integer atomicMin of the position, as UpdateLocalPoints).
 *  - lFixedCameras: a key frame that owns a usable record of a local point, is not marked local, is not bad and is in the same map.
 *    num_fixedKF = their number + 1 if a listed key frame has id == init_kf_id.
 *  - num_fixedKF < 2 (:1906-1945, one lane): the local list in order without current_kf and the init key frame; ids compared as signed
 *    ints; `if (id < lowerId) .. else if (id < secondLowerId) ..`, so a new lowest id does not hand the old one down; without a candidate
 *    nothing moves; a moved key frame leaves the local list and is fixed.
 *  - poses: local and fixed key frames in ascending mnId; poses[i] = LbaLinearizer::poseFromTcw of the float Rcw | tcw, operation for
 *    operation in double.
 *  - edges: per point its usable records in CSR order whose key frame is not bad and in the same map; kind = u_right < 0 ? MONO : STEREO
 *    (-0.0f is stereo); obs = {kpUn.pt.x, kpUn.pt.y, mono ? 0 : u_right}; inv_sigma2 = inv_level_sigma2[octave]; cam = 0.  An octave
 *    outside [0, nlevels) is a bad index: the edge is dropped.
 *  - lm_start, pose_start, pose_edges (ascending per pose): the bytes of orbhip.lba.build_structure for these edges.
 * A list entry, a row, a d_kf_mp entry, a CSR range or a record that cannot be read sets ORBM_LBA_BAD_INDEX and is treated as absent; a
 * current_kf that cannot be read builds nothing (an empty window).  Overflow is decided before any slab is written.  Eight launches on
 * `stream` whatever the sizes (the first clears the workspace), nothing read on the host, graph-capturable, integer atomics only:
 * deterministic.  ORB_E_INVALID for null pointers (d_map and arrays of count 0 excepted), negative counts, capacities or cap_conn below
 * 1, nlevels outside 1..16, misaligned d_mp, poses, points or workspace. */
int orbm_lba_window_build(const orbm_localmap_view* view, const orbm_lba_in* in, int current_kf, uint32_t init_kf_id,
                          const orbm_lba_window* out, void* d_work, void* stream);

/* The slabs orbm_lba_window_apply folds the optimised window into (the arrays the view and orbm_lba_in name, now written) and its lists. */
typedef struct orbm_lba_apply {
    orbm_map_point* d_mp;              /* [n_mp] pos of every local point; ORBM_MP_BAD / ORBM_MP_HAS_OBS of the points that lost a record */
    int32_t* d_kf_mp;                  /* [n_kf_mp_rows] -1 at the feature of every record that died */
    int32_t* d_mp_nobs;                /* [n_mp] MapPoint::nObs, in/out, or NULL: the weighted record sum, exactly as in orbm_cull_in */
    orbm_refresh_point* d_ref;         /* [n_mp] the rule of orbm_cull_apply.d_ref */
    orbm_fusenb_pose* d_pose;          /* [n_kf] rewritten for every key frame still in the local list */
    orbm_keyframe_center* d_center;    /* [n_kf] .left = Ow of those; .right stays */
    int32_t* d_erased;                 /* [cap_e][2] vToErase as (key frame, point) pairs: mono outliers in edge order, then stereo */
    int32_t* d_went_bad;               /* [cap_l] the points that went bad, in list order, padded with -1 */
    int32_t* d_obs_start_out;          /* [n_mp + 1] the surviving rows (never the view's own arrays); on the early return a copy */
    orbm_observation* d_obs_out;       /* [cap_obs_out], cap_obs_out >= n_obs */
    int32_t* d_result;                 /* [ORBM_LBA_A_WORDS] */
    int32_t cap_obs_out, reserved;
} orbm_lba_apply;
/* d_result words of orbm_lba_window_apply */
#define ORBM_LBA_A_FLAGS 0
#define ORBM_LBA_A_N_ERASED 1         /* vToErase.size() */
#define ORBM_LBA_A_N_WENT_BAD 2
#define ORBM_LBA_A_N_OBS 3            /* the rows of the out-CSR */
#define ORBM_LBA_A_N_MONO 4
#define ORBM_LBA_A_N_STEREO 5
#define ORBM_LBA_A_WORDS 8

/* Optimizer.cc:2293-2510 on the window `win` that orbm_lba_window_build made of the same view (nothing of the build's workspace is
 * read: the window's slabs carry everything), whose poses and points are now the optimised ones; d_chi2 / d_depth [n_edges] are what lba_compute_errors wrote for them.
 *  - An edge is an outlier iff chi2 > 5.991 (mono) / 7.815 (stereo) or !(depth > 0.0), as doubles: a NaN chi2 keeps, a NaN depth erases.
 *  - d_erased and N_ERASED are always written.  (double)n_erase >= (n_mono + n_stereo) * 0.5, a window without edges included, is the
 *    early return: ORBM_LBA_EARLY_RETURN, and NOTHING of the map is written, poses and positions included.
 *  - The erase loop, per point in vToErase order (one lane per point): the record dies; nObs drops by 2 if the record's feature has
 *    u_right >= 0, else by 1; d_kf_mp[row of the record's feature] = -1 unconditionally; nObs <= 2 is SetBadFlag: ORBM_MP_BAD, every
 *    remaining usable record dies with its d_kf_mp entry, the point's later pairs are no-ops, nObs is not reset; ORBM_MP_HAS_OBS = nObs > 0.
 *    A bad point has no rows in the out-CSR.  d_ref: a point that is not bad and whose ref_kf record died gets {key frame of its first
 *    surviving usable record, that feature's octave}.
 *  - Every key frame with d_pose_local gets Rcw | tcw = (float) of SE3Quat::to_homogeneous_matrix in double, Ow = -Rwc * tcw as one
 *    cv::gemm with alpha = -1 (a double sum of double products in k order, times alpha, rounded once), d_center.left = Ow.
 *  - pos = (float)X for every local point; then orbm_refresh_map_points(ORBM_REFRESH_NORMAL_DEPTH) over the local points on the out-CSR
 *    with the new centres (it IS that entry point: a bad point is left alone by its own rule).
 *    Its per-point status stays in the workspace and is NOT folded into ORBM_LBA_A_FLAGS: a local point with more than
 *    ORBM_REFRESH_MAX_OBS usable records keeps its old normal and distance bounds (pos is written all the same), as after every other
 *    call of that entry point; the reference has no such cap.  A caller whose points can carry that many records checks their counts.
 * Eight launches on `stream` whatever the sizes, nothing read on the host, graph-capturable, integer atomics only: deterministic.
 * ORB_E_INVALID as above and for cap_obs_out < n_obs, out-CSR arrays that are the view's own. */
int orbm_lba_window_apply(const orbm_localmap_view* view, const orbm_lba_in* in, const orbm_lba_window* win, const double* d_chi2,
                          const double* d_depth, const orbm_lba_apply* apply, void* d_work, void* stream);

/* SURVEY.md N3 — Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:907-1273): the motion-only BA that follows
 * every matcher call in Tracking (Tracking.cc:2210,2395,2468).  One pose vertex, unary reprojection edges
 * (EdgeSE3ProjectXYZOnlyPose OptimizableTypes.h:37-63/.cpp:50-65, EdgeSE3ProjectXYZOnlyPoseToBody :65-91/.cpp:93-109,
 * g2o::EdgeStereoSE3ProjectXYZOnlyPose types_six_dof_expmap.cpp:339-404), 4 rounds x optimize(10) of g2o's Levenberg-Marquardt
 * with the dense 6x6 solver, chi2 inlier/outlier re-classification between rounds (5.991 / 7.815), Huber kernel dropped for the
 * last round, pose reset to the initial estimate at the start of every round.  One workgroup per frame runs the whole thing
 * in a single launch.  Outputs: the optimised pose, mvbOutlier per edge, and the return value nInitialCorrespondences - nBad. */
typedef struct pose_edge {
    float xw[3];        /* pMP->GetWorldPos() (float in the map) */
    float obs[3];       /* kpUn.pt.x, kpUn.pt.y, mvuRight */
    float inv_sigma2;   /* mvInvLevelSigma2[octave] */
    int16_t kind, cam;  /* LBA_EDGE_MONO / LBA_EDGE_STEREO / LBA_EDGE_BODY, camera index */
} pose_edge;
int pose_optimize(const double* d_poses_in, const pose_edge* d_edges, const int32_t* d_n_edges, int cap_e, int batch,
                  const lba_camera* d_cameras, int n_cameras, double* d_poses_out, uint8_t* d_outlier, int32_t* d_n_good,
                  void* stream);
/* The same with what the caller knows about the edges it flattened.  LBA_HINT_PINHOLE: EVERY edge is an EdgeSE3ProjectXYZOnlyPose (LBA_EDGE_MONO)
 * or an EdgeStereoSE3ProjectXYZOnlyPose (LBA_EDGE_STEREO) on a pinhole camera — the monocular, stereo and RGB-D pinhole configurations.
 * Identical results from a kernel without the fisheye model and the right-camera edge; a hint that does not hold gives wrong poses. */
int pose_optimize_hint(const double* d_poses_in, const pose_edge* d_edges, const int32_t* d_n_edges, int cap_e, int batch,
                       const lba_camera* d_cameras, int n_cameras, double* d_poses_out, uint8_t* d_outlier, int32_t* d_n_good,
                       unsigned hints, void* stream);

/* SURVEY.md N4 (tail) — Optimizer::LocalInertialBA (reference src/Optimizer.cc:4753-5365): the visual-inertial local BA of the
 * inertial modes.  Graph (include/G2oTypes.h, src/G2oTypes.cc): VertexPose (ImuCamPose, 6 dof, body-frame right perturbation
 * G2oTypes.cc:196-221), VertexVelocity / VertexGyroBias / VertexAccBias (3 dof each, additive), VertexSBAPointXYZ (marginalised);
 * EdgeInertial (9-dim, six vertices, G2oTypes.cc:706-800), EdgeGyroRW / EdgeAccRW (G2oTypes.h:633-700), EdgeMono / EdgeStereo
 * (G2oTypes.h:337-437, G2oTypes.cc:352-418; pinhole or KannalaBrandt8, camera index 0/1 of the rig).  Solver: g2o Levenberg-Marquardt
 * with setUserLambdaInit (Optimizer.cc:4884-4896), Schur complement of the landmarks, dense Cholesky of the reduced system.
 * One workgroup runs the whole optimize(iterations) of one window in a single launch; windows are batched. */
typedef struct liba_keyframe {      /* ImuCamPose + the V / G / A vertex estimates of one key frame; row-major 3x3 */
    double Rwb[9], twb[3];          /* body pose (pKF->GetImuRotation / GetImuPosition) */
    double Rcw[2][9], tcw[2][3];    /* per camera, as the ImuCamPose constructor sets them (G2oTypes.cc:43-66); rewritten by every update */
    double v[3], bg[3], ba[3];      /* VertexVelocity, VertexGyroBias, VertexAccBias estimates */
    int32_t pose_fixed;             /* VP->setFixed */
    int32_t has_imu;                /* V / G / A vertices exist (pKFi->bImu) */
    int32_t imu_fixed;              /* V / G / A fixed (the key frame just before the temporal window) */
    int32_t reserved;
} liba_keyframe;                    /* 376 bytes; key frames in ascending mnId order (= g2o's Hessian block order) */
typedef struct liba_rig {           /* calibration members of ImuCamPose (G2oTypes.h:60-72) */
    int32_t n_cams, reserved;
    double Rcb[2][9], tcb[2][3], Rbc[2][9], tbc[2][3];
    double bf;
    int32_t model[2];               /* LBA_CAM_PINHOLE / LBA_CAM_KB8 */
    double p[2][8];                 /* mvParameters widened */
} liba_rig;
typedef struct liba_imu_edge {      /* one IMU::Preintegrated between consecutive key frames: EdgeInertial + EdgeGyroRW + EdgeAccRW */
    int32_t kf1, kf2;               /* previous / current key frame (indices into the window's key frames) */
    float dR[9], dV[3], dP[3];      /* Preintegrated::dR, dV, dP (CV_32F) */
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float b[6];                     /* Preintegrated::b = bax bay baz bwx bwy bwz (the bias the measurements were integrated with) */
    float dT, pad;
    double huber;                   /* 0 = no robust kernel; sqrt(16.92) for i == N-1 or bRecInit (Optimizer.cc:5005-5012) */
    double info[81];                /* EdgeInertial::information() as the reference leaves it (constructor clean-up, x1e-2 for i == N-1) */
    double info_g[9], info_a[9];    /* EdgeGyroRW / EdgeAccRW information (Optimizer.cc:5024-5043) */
} liba_imu_edge;                    /* 1080 bytes */
#define LIBA_MAX_FREE 32            /* optimisable key frames per window (maxOpt is 10, or 25 for bLarge: Optimizer.cc:4758-4764) */
typedef struct liba_problem {
    liba_keyframe* kfs;             /* [batch][cap_kf]  UPDATED IN PLACE */
    const int32_t* n_kf;            /* [batch] */
    const liba_rig* rigs;           /* window b uses rigs[b * rig_stride] (rig_stride 0 = one shared rig) */
    double* points;                 /* [batch][cap_l][3]  UPDATED IN PLACE */
    const int32_t* n_points;        /* [batch] */
    const lba_edge* edges;          /* [batch][cap_e]  landmark-major; pose = key-frame index, kind = LBA_EDGE_MONO / LBA_EDGE_STEREO, cam = camera of the rig */
    const int32_t* n_edges;         /* [batch] */
    const liba_imu_edge* imu;       /* [batch][cap_i]  in the reference's insertion order (newest first) */
    const int32_t* n_imu;           /* [batch] */
    int32_t cap_kf, cap_l, cap_e, cap_i, rig_stride;
    int32_t max_free;               /* upper bound of optimisable key frames in any window (<= LIBA_MAX_FREE): sizes the reduced system, 15 * max_free
                                     * unknowns (6 per free pose + 9 per key frame with free IMU states).  A window with more free poses or more
                                     * unknowns is refused (stats[0] = -1) */
    double huber_mono, huber_stereo;   /* thHuberMono / thHuberStereo (Optimizer.cc:5071-5073) */
} liba_problem;
size_t liba_workspace_bytes(const liba_problem* prob, int batch);
/* optimizer.optimize(iterations) (Optimizer.cc:5225).  d_stats: [batch][5] device doubles = {iterations run (-1: invalid window), final
 * activeRobustChi2 (err_end), final lambda, lambda trials, initial activeRobustChi2 (err)}.  Asynchronous on `stream`. */
int liba_optimize(const liba_problem* prob, int batch, double lambda_init, int iterations, void* d_workspace, double* d_stats, void* stream);
/* computeActiveErrors: per visual edge chi2 and isDepthPositive (the outlier pass of Optimizer.cc:5237-5275 reads both), per preintegration
 * {EdgeInertial, EdgeGyroRW, EdgeAccRW} chi2, and activeRobustChi2 per window.  Any output may be NULL. */
int liba_compute_errors(const liba_problem* prob, int batch, double* d_vis_chi2, uint8_t* d_vis_depth_pos, double* d_imu_chi2,
                        double* d_robust_sum, void* stream);

/* Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool bRecInit) (reference src/Optimizer.cc:7665-8067): the per-frame optimisation of
 * the inertial tracking modes (Tracking.cc: after TrackLocalMap's matching when the map was updated).  Frame pose / velocity / gyro bias / acc bias free
 * (15 unknowns), the last key frame's vertices fixed; EdgeMonoOnlyPose / EdgeStereoOnlyPose (G2oTypes.h:387-421, 463-491) as pose_edge records
 * (kind = LBA_EDGE_MONO / LBA_EDGE_STEREO, cam = camera of the rig, kind |= LIBA_EDGE_CLOSE iff mTrackDepth < 10), one EdgeInertial + EdgeGyroRW +
 * EdgeAccRW (liba_imu_edge with kf1 = key frame, kf2 = frame; huber ignored).  4 rounds x optimize(10) of g2o's Gauss-Newton with the dense solver,
 * chi2 re-classification {12, 7.5, 5.991, 5.991} / {15.6, 9.8, 7.815, 7.815} with the 1.5x bClose rule, Huber dropped for the last round, the
 * < 30 inliers recovery pass.  One wave per frame, single launch.  Outputs: d_frames updated in place (SetImuPoseVelocity + mImuBias), mvbOutlier per
 * edge, the 15x15 row-major Hessian of the final state (ConstraintPoseImu::H, :8040-8062), and the return value nInitialCorrespondences - nBad. */
#define LIBA_EDGE_CLOSE 0x100
int liba_pose_inertial_kf(liba_keyframe* d_frames, const liba_keyframe* d_keyframes, const liba_rig* d_rigs, int rig_stride, const pose_edge* d_edges,
                          const int32_t* d_n_edges, int cap_e, const liba_imu_edge* d_imu, int batch, int rec_init, uint8_t* d_outlier, double* d_H,
                          int32_t* d_n_good, void* stream);

/* Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool bRecInit) (reference src/Optimizer.cc:8068-8415): as liba_pose_inertial_kf, but the previous
 * FRAME's pose / velocity / biases are free too (30 unknowns) and tied down by EdgePriorPoseImu (G2oTypes.h:737-784; Huber delta 5) built from the
 * ConstraintPoseImu the previous call left (liba_prior: its members after the constructor's eigenvalue clean-up, H row-major); the preintegration is
 * mpImuPreintegratedFrame (kf1 = previous frame, kf2 = frame); chi2Mono = 5.991 in every round.  d_prev_frames is updated in place as well.  d_H =
 * the final 30x30 Hessian marginalised over the previous frame (Optimizer::Marginalize, :5366-5450) = the 15x15 block handed to the new ConstraintPoseImu. */
typedef struct liba_prior {
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3];   /* ConstraintPoseImu linearisation point */
    double H[225];                                 /* ConstraintPoseImu::H, row-major */
} liba_prior;
int liba_pose_inertial_lastframe(liba_keyframe* d_frames, liba_keyframe* d_prev_frames, const liba_rig* d_rigs, int rig_stride, const pose_edge* d_edges,
                                 const int32_t* d_n_edges, int cap_e, const liba_imu_edge* d_imu, const liba_prior* d_priors, int batch, int rec_init,
                                 uint8_t* d_outlier, double* d_H, int32_t* d_n_good, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Device-memory helpers so that adapters written against this header need no HIP headers.
 * ------------------------------------------------------------------------------------------------------- */
int orb_device_count(void);
int orb_dev_alloc(int device, size_t bytes, void** d_ptr);
int orb_dev_free(void* d_ptr);
int orb_host_alloc(size_t bytes, void** h_ptr);   /* page-locked host memory: copies from / to it are real asynchronous DMA (a pageable copy is staged and
                                                     synchronous inside the runtime); the adapters' packed staging blocks live in it */
int orb_host_free(void* h_ptr);
int orb_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);   /* asynchronous on stream */
int orb_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);   /* asynchronous on stream */
int orb_memset(void* d_dst, int value, size_t bytes, void* stream);
int orb_stream_sync(void* stream);   /* NULL = default stream */

#ifdef __cplusplus
}
#endif
#endif /* ORBHIP_H */
