// orbm_project.hip — map-point projection on gfx950: the per-point loops that turn map points into the orbm_query records the
// projection searches read (include/orbhip.h "Map-point projection").
//
//   k_project   Frame::isInFrustum (Frame.cc:571-665) + Tracking::SearchLocalPoints (Tracking.cc:2874-2905) + the query loop of
//               SearchByProjection(Frame&, vector<MapPoint*>&, ...) (ORBmatcher.cc:59-110); the projection loops of the motion-model search
//               (:2244-2331) and of the relocalisation search (:2520-2600).  MapPoint::PredictScale (MapPoint.cc:578-610) through host-made
//               level thresholds.
//
// Form: one 256-lane workgroup per frame walks the frame's list in chunks of 256 records, one record per lane.  The kept queries are compacted
// in list order (the search's serial accept loop depends on query order): wg_scan.inc's ballot step per chunk, a running base across chunks.
// Each kept query gathers its 32-byte descriptor with two 16-byte loads and stores.
//
// Arithmetic is the reference's cv::Mat arithmetic as the glue is tested under (tests/cpp/mock_orbslam3/opencv2/core/core.hpp): R*X sums the
// products in double from 0 and rounds once, `+ t` and Pinhole::project (fx*x/z + cx) in float, cv::norm = float(sqrt(double dot)),
// PO.dot(Pn)/dist in double stored as float.  The library is built with -ffp-contract=off and correctly rounded fp32 division.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "proj_arith.inc"
#include "wg_scan.inc"

struct ProjArgs {
    const orbm_map_point* mp;
    const int32_t* nmp;
    int cap_mp;
    const uint8_t* mp_desc;
    const orbm_project_frame* frames;
    orbm_track* track;
    orbm_query* queries;
    uint8_t* qdesc;
    int32_t* nq;
    int32_t* q_src;
    int32_t* n_required;
    int32_t* n_in_view;
    int cap_q;
    orbm_project_params prm;
};

// (mat_row, dot3 and predict_scale: proj_arith.inc)
static __device__ __forceinline__ int clamp_level(int l) { return l < 0 ? 0 : (l > 15 ? 15 : l); }

static __global__ __launch_bounds__(256) void k_project(ProjArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* wtot = (int*)orb_smem;   // [2][4] kept queries per wave, by chunk parity; [8..11] in-view counts per wave
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const orbm_project_params& P = A.prm;
    int n = A.nmp[b];
    n = n < 0 ? 0 : (n > A.cap_mp ? A.cap_mp : n);
    const orbm_project_frame F = A.frames[b];
    const int mode = P.mode;
    // motion model: twc = Ow, tlc = Rlw*twc + tlw (ORBmatcher.cc:2257-2265)
    const float tlc_z = mat_row(F.Rlw + 6, F.Ow[0], F.Ow[1], F.Ow[2]) + F.tlw[2];
    const bool bForward = tlc_z > P.mb && !P.mono;
    const bool bBackward = -tlc_z > P.mb && !P.mono;
    const bool bFactor = P.th != 1.0f;
    const size_t rec0 = (size_t)b * A.cap_mp, q0 = (size_t)b * A.cap_q;
    int base = 0, in_view_w = 0;
    for (int c0 = 0, it = 0; c0 < n; c0 += 256, it++) {
        const int i = c0 + tid;
        bool keep = false, counted = false;
        orbm_query q;
        int desc_row = -1;
        if (i < n) {
            union { uint4 v[3]; orbm_map_point r; } R;
            const uint4* src = (const uint4*)(A.mp + rec0 + i);
            R.v[0] = src[0]; R.v[1] = src[1]; R.v[2] = src[2];
            const orbm_map_point& r = R.r;
            desc_row = r.desc_row;
            const uint32_t f = r.flags;
            if (f & ORBM_MP_VALID) {
                const float X = r.pos[0], Y = r.pos[1], Z = r.pos[2];
                const float xc = mat_row(F.Rcw, X, Y, Z) + F.tcw[0];
                const float yc = mat_row(F.Rcw + 3, X, Y, Z) + F.tcw[1];
                const float zc = mat_row(F.Rcw + 6, X, Y, Z) + F.tcw[2];
                if (mode == ORBM_PROJ_LOCAL_MAP) {
                    union { uint4 v[2]; orbm_track t; } T;
                    uint4* tp = (uint4*)(A.track + rec0 + i);
                    T.v[0] = tp[0]; T.v[1] = tp[1];
                    orbm_track& t = T.t;
                    if (!(f & (ORBM_MP_SEEN | ORBM_MP_BAD))) {   // Tracking.cc:2874-2877, then isInFrustum (Frame.cc:571-665)
                        t.in_view = 0;
                        t.proj_x = -1.f;
                        t.proj_y = -1.f;
                        const float Pc_dist = (float)sqrt(dot3(xc, yc, zc, xc, yc, zc));
                        const float invz = 1.0f / zc;
                        if (!(zc < 0.0f)) {
                            const float u = P.fx * xc / zc + P.cx, v = P.fy * yc / zc + P.cy;
                            if (!(u < F.bounds[0] || u > F.bounds[1]) && !(v < F.bounds[2] || v > F.bounds[3])) {
                                t.proj_x = u;
                                t.proj_y = v;
                                const float maxDistance = 1.2f * r.max_distance, minDistance = 0.8f * r.min_distance;
                                const float POx = X - F.Ow[0], POy = Y - F.Ow[1], POz = Z - F.Ow[2];
                                const float dist = (float)sqrt(dot3(POx, POy, POz, POx, POy, POz));
                                if (!(dist < minDistance || dist > maxDistance)) {
                                    const float viewCos = (float)(dot3(POx, POy, POz, r.normal[0], r.normal[1], r.normal[2]) / (double)dist);
                                    if (!(viewCos < P.view_cos_limit)) {
                                        t.in_view = 1;
                                        t.proj_xr = u - P.mbf * invz;
                                        t.depth = Pc_dist;
                                        t.level = predict_scale(r.max_distance / dist, P);
                                        t.view_cos = viewCos;
                                        counted = true;
                                    }
                                }
                            }
                        }
                        tp[0] = T.v[0]; tp[1] = T.v[1];
                    }
                    // the query loop of SearchByProjection (ORBmatcher.cc:73-110), on the track state as it now stands
                    if (t.in_view && !(P.far_points && t.depth > P.th_far_points) && !(f & ORBM_MP_BAD)) {
                        const int L = t.level;
                        float rad = ((double)t.view_cos > 0.998) ? 2.5f : 4.0f;   // RadiusByViewingCos (ORBmatcher.cc:260-266)
                        if (bFactor) rad *= P.th;
                        q.u = t.proj_x; q.v = t.proj_y; q.radius = rad * P.scale_factors[clamp_level(L)]; q.u_right = t.proj_xr; q.angle = 0.f;
                        q.min_level = (int16_t)(L - 1); q.max_level = (int16_t)L;
                        q.flags = ORBM_Q_VALID | ((f & ORBM_MP_HAS_OBS) ? ORBM_Q_HAS_OBS : 0u) | ORBM_Q_STEREO;
                        keep = true;
                    }
                } else if (mode == ORBM_PROJ_LAST_FRAME) {   // ORBmatcher.cc:2267-2331
                    const float invzc = (float)(1.0 / (double)zc);
                    if (!(invzc < 0)) {
                        const float u = P.fx * xc / zc + P.cx, v = P.fy * yc / zc + P.cy;
                        if (!(u < F.bounds[0] || u > F.bounds[1]) && !(v < F.bounds[2] || v > F.bounds[3])) {
                            const int o = r.octave;
                            q.u = u; q.v = v; q.radius = P.th * P.scale_factors[clamp_level(o)]; q.u_right = u - P.mbf * invzc; q.angle = r.angle;
                            q.min_level = (int16_t)(bForward ? o : (bBackward ? 0 : o - 1));
                            q.max_level = (int16_t)(bForward ? -1 : (bBackward ? o : o + 1));
                            q.flags = ORBM_Q_VALID | ((f & ORBM_MP_HAS_OBS) ? ORBM_Q_HAS_OBS : 0u) | ORBM_Q_STEREO;
                            keep = counted = true;
                        }
                    }
                } else if (!(f & ORBM_MP_BAD)) {   // ORBM_PROJ_RELOC, ORBmatcher.cc:2537-2600 (no depth check)
                    const float u = P.fx * xc / zc + P.cx, v = P.fy * yc / zc + P.cy;
                    if (!(u < F.bounds[0] || u > F.bounds[1]) && !(v < F.bounds[2] || v > F.bounds[3])) {
                        const float POx = X - F.Ow[0], POy = Y - F.Ow[1], POz = Z - F.Ow[2];
                        const float dist3D = (float)sqrt(dot3(POx, POy, POz, POx, POy, POz));
                        const float maxDistance = 1.2f * r.max_distance, minDistance = 0.8f * r.min_distance;
                        if (!(dist3D < minDistance || dist3D > maxDistance)) {
                            const int L = predict_scale(r.max_distance / dist3D, P);
                            q.u = u; q.v = v; q.radius = P.th * P.scale_factors[L]; q.u_right = 0.f; q.angle = r.angle;
                            q.min_level = (int16_t)(L - 1); q.max_level = (int16_t)(L + 1);
                            q.flags = ORBM_Q_VALID | ORBM_Q_HAS_OBS;
                            keep = counted = true;
                        }
                    }
                }
            }
        }
        // stable compaction (wg_scan.inc), a running base across chunks
        in_view_w += __popcll(__ballot(counted));
        int tot;
        const int pos = base + wg_scan_ballot<4>(keep, wtot, it, &tot);
        if (keep) {
            if (pos < A.cap_q) {
                A.queries[q0 + pos] = q;
                A.q_src[q0 + pos] = i;
                uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
                if (desc_row >= 0 && desc_row < P.n_desc_rows) {
                    const uint4* s = (const uint4*)(A.mp_desc + (size_t)desc_row * 32);
                    d0 = s[0]; d1 = s[1];
                }
                uint4* d = (uint4*)(A.qdesc + (q0 + pos) * 32);
                d[0] = d0; d[1] = d1;
            }
        }
        base += tot;
    }
    if (lane == 0) wtot[8 + wv] = in_view_w;
    __syncthreads();
    if (tid == 0) {
        const int nin = wtot[8] + wtot[9] + wtot[10] + wtot[11];
        const int req = (mode == ORBM_PROJ_LOCAL_MAP && nin == 0) ? 0 : base;   // nToMatch == 0: no search (Tracking.cc:2908)
        A.n_in_view[b] = nin;
        A.n_required[b] = req;
        A.nq[b] = req < A.cap_q ? req : A.cap_q;
    }
}

// the level PredictScale gives a float ratio, with the host's logf (std::log(float), as tests/cpp/mock_orbslam3 calls it); ceil compared as a
// float, so that +inf ratios need no float -> int conversion
static bool level_at_least(float ratio, float lsf, int k) { return std::ceil(std::log(ratio) / lsf) >= (float)k; }

extern "C" int orbm_predict_scale_thresholds(float log_scale_factor, int nlevels, float* thresholds) {
    if (!thresholds || !(log_scale_factor > 0.f) || std::isinf(log_scale_factor) || nlevels < 1 || nlevels > 16) return ORB_E_INVALID;
    for (int k = 1; k < nlevels; k++) {
        // smallest positive float (by bit pattern: monotone for positive floats) with level >= k; +inf always qualifies
        uint32_t lo = 0u, hi = 0x7f800000u;   // level(lo) < k (lo = +0: log = -inf), level(hi) >= k
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            float r;
            std::memcpy(&r, &mid, 4);
            if (level_at_least(r, log_scale_factor, k)) hi = mid; else lo = mid;
        }
        std::memcpy(&thresholds[k - 1], &hi, 4);
    }
    return ORB_OK;
}

extern "C" int orbm_project_map_points(const orbm_map_point* d_mp, const int32_t* d_nmp, int cap_mp, const uint8_t* d_mp_desc,
                                       const orbm_project_frame* d_frames, int batch, const orbm_project_params* params, orbm_track* d_track,
                                       orbm_query* d_queries, uint8_t* d_qdesc, int32_t* d_nq, int32_t* d_q_src, int32_t* d_n_required,
                                       int32_t* d_n_in_view, int cap_q, void* stream) {
    if (!d_mp || !d_nmp || !d_mp_desc || !d_frames || !params || !d_queries || !d_qdesc || !d_nq || !d_q_src || !d_n_required || !d_n_in_view)
        return ORB_E_INVALID;
    const int mode = params->mode;
    if (mode != ORBM_PROJ_LOCAL_MAP && mode != ORBM_PROJ_LAST_FRAME && mode != ORBM_PROJ_RELOC) return ORB_E_INVALID;
    if (mode == ORBM_PROJ_LOCAL_MAP && !d_track) return ORB_E_INVALID;
    if (params->camera_type != ORBM_CAM_PINHOLE || params->nleft != -1 || params->nlevels < 1 || params->nlevels > 16 || params->n_desc_rows < 0)
        return ORB_E_INVALID;
    if (cap_q < 1 || cap_mp < 1 || batch < 1) return ORB_E_INVALID;
    // 16-byte loads / stores of the records and descriptor rows
    if (misaligned16(d_mp) || misaligned16(d_mp_desc) || misaligned16(d_qdesc) || misaligned16(d_track)) return ORB_E_INVALID;
    ProjArgs A;
    A.mp = d_mp; A.nmp = d_nmp; A.cap_mp = cap_mp; A.mp_desc = d_mp_desc; A.frames = d_frames; A.track = mode == ORBM_PROJ_LOCAL_MAP ? d_track : nullptr;
    A.queries = d_queries; A.qdesc = d_qdesc; A.nq = d_nq; A.q_src = d_q_src; A.n_required = d_n_required; A.n_in_view = d_n_in_view;
    A.cap_q = cap_q; A.prm = *params;
    hipLaunchKernelGGL(k_project, dim3(batch), dim3(256), 12 * 4, (hipStream_t)stream, A);
    return launch_status();
}
