// orbm_newpoints.hip — the inner loop of LocalMapping::CreateNewMapPoints on gfx950 (include/orbhip.h "New map points"):
//
//   k_create_new_points   LocalMapping.cc:651-904 for one (KF1, KF2) pair per workgroup: the parallax test, the linear triangulation or the
//                         stereo unprojection, the depth-sign / reprojection / scale-consistency gates, and the ordered list of created points.
//   k_append_new_points   the created points of a batch of pairs appended to the device map (orbm_map_point records, the observation CSR,
//   k_append_finish       the orbm_refresh_point records, a selection for orbm_refresh_map_points), in order, behind a device cursor.
//
// Form of k_create_new_points: one 256-lane workgroup per pair, one lane per feature i1 of KF1, in chunks of 256.  The work per match is
// independent; only the order of the created points is serial (ascending idx1 = the order of vMatchedIndices).  The ordered compaction goes per
// chunk (wg_scan.inc's ballot step), with a running base.
// d_point_of_2 takes the LAST creator of an idx2 (pKF2->AddMapPoint overwrites): ranks ascend with idx1, so an integer atomicMax on the rank.
//
// Arithmetic: rule R6 of DESIGN.md section 2 (float expressions as written, cv::Mat products as double sums rounded once, double libm calls on
// float arguments).  The library is built with -ffp-contract=off and correctly rounded fp32 division / sqrt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/orbhip.h"
#include "kb8_geom.inc"
#include "mapview.inc"
#include "wg_scan.inc"

struct NewPtArgs {
    orbm_newpt_side s1, s2;
    const orbm_newpt_pair* pairs;
    const int32_t* match12;
    uint8_t* status;
    orbm_new_point* out;
    int cap_new;
    int32_t* nnew;
    int32_t* nrequired;
    int32_t* point_of_1;
    int32_t* point_of_2;
    uint32_t* pair_flags;
};

// one element of a cv::gemm on floats with an addend: the double sum of the double products from 0 in k order, plus c, rounded once
static __device__ __forceinline__ float gemm3(const float a0, const float a1, const float a2, const float* x, const double c) {
    double s = 0.0;
    s += (double)a0 * (double)x[0];
    s += (double)a1 * (double)x[1];
    s += (double)a2 * (double)x[2];
    return (float)(s + c);
}
static __device__ __forceinline__ double ddot3(const float* a, const float* b) {   // Mat::dot on floats: a double
    double s = 0.0;
    s += (double)a[0] * (double)b[0];
    s += (double)a[1] * (double)b[1];
    s += (double)a[2] * (double)b[2];
    return s;
}
static __device__ __forceinline__ void np_unproject(const int type, const float* k, const float u, const float v, float* xn) {
    if (type == ORBM_CAM_KB8) { kb8_unproject(k, u, v, xn); return; }
    xn[0] = (u - k[2]) / k[0]; xn[1] = (v - k[3]) / k[1]; xn[2] = 1.f;   // Pinhole.cpp:63-69
}
static __device__ __forceinline__ void np_project(const int type, const float* k, const float* X, float* uv) {
    if (type == ORBM_CAM_KB8) { kb8_project_f(k, X, uv); return; }
    uv[0] = k[0] * X[0] / X[2] + k[2]; uv[1] = k[1] * X[1] / X[2] + k[3];   // Pinhole.cpp:31-35
}
// cos(2*atan2(mb/2, depth)) with the float overloads (LocalMapping.cc:758, 760)
static __device__ __forceinline__ float stereo_cos(const float mb, const float depth) {
    const float th = (float)atan2((double)(mb / 2.f), (double)depth);
    const float a = 2.f * th;
    return (float)cos((double)a);
}
// KeyFrame::UnprojectStereo (KeyFrame.cc:861-877); false = the empty cv::Mat
static __device__ __forceinline__ bool unproject_stereo(const orbm_newpt_camera& c, const orb_keypoint& raw, const float z, float* x3D) {
    if (!(z > 0)) return false;
    float xc[3];
    xc[0] = (raw.x - c.k[2]) * z * c.invfx;
    xc[1] = (raw.y - c.k[3]) * z * c.invfy;
    xc[2] = z;
    for (int i = 0; i < 3; i++) x3D[i] = gemm3(c.Rcw[i], c.Rcw[3 + i], c.Rcw[6 + i], xc, (double)c.Ow[i]);   // Twc = [Rcw^T | Ow]
    return true;
}
// the reprojection gate of one key frame (LocalMapping.cc:812-838 / :840-863); mbf is ALWAYS KF1's (:831, :856).  true = rejected
static __device__ __forceinline__ bool reproj_rejects(const orbm_newpt_camera& c, const float mbf, const float* x3D, const float z, const orb_keypoint& kp,
                                                      const bool stereo, const float ur, const float sigma2) {
    float P[3];
    P[0] = gemm3(c.Rcw[0], c.Rcw[1], c.Rcw[2], x3D, (double)c.tcw[0]);
    P[1] = gemm3(c.Rcw[3], c.Rcw[4], c.Rcw[5], x3D, (double)c.tcw[1]);
    P[2] = z;
    const float invz = (float)(1.0 / (double)z);
    if (!stereo) {
        float uv[2];
        np_project(c.camera_type, c.k, P, uv);
        const float ex = uv[0] - kp.x, ey = uv[1] - kp.y;
        return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    }
    const float u = c.k[0] * P[0] * invz + c.k[2];
    const float u_r = u - mbf * invz;
    const float v = c.k[1] * P[1] * invz + c.k[3];
    const float ex = u - kp.x, ey = v - kp.y, er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}
static __device__ __forceinline__ float dist_to(const float* x3D, const float* Ow) {   // (float)cv::norm(x3D - Ow)
    float d[3];
    for (int i = 0; i < 3; i++) d[i] = x3D[i] - Ow[i];
    return (float)sqrt(ddot3(d, d));
}

// LocalMapping.cc:653-904 for one match (i1, idx2), both in range -> the exit's code; x3D is the new point when the code is a CREATED one
static __device__ int create_one(const NewPtArgs& A, const orbm_newpt_pair& P, const size_t o1, const size_t o2, float* x3D) {
    const orbm_newpt_camera& c1 = P.cam1;
    const orbm_newpt_camera& c2 = P.cam2;
    const orb_keypoint kp1 = A.s1.kps[o1], kp2 = A.s2.kps[o2];
    if (kp1.octave < 0 || kp1.octave >= 16 || kp2.octave < 0 || kp2.octave >= 16) return ORBM_NEWPT_BAD_INDEX;
    const float ur1 = A.s1.u_right ? A.s1.u_right[o1] : -1.f, ur2 = A.s2.u_right ? A.s2.u_right[o2] : -1.f;
    const bool bStereo1 = ur1 >= 0, bStereo2 = ur2 >= 0;
    float xn1[3], xn2[3], ray1[3], ray2[3];
    np_unproject(c1.camera_type, c1.k, kp1.x, kp1.y, xn1);
    np_unproject(c2.camera_type, c2.k, kp2.x, kp2.y, xn2);
    for (int i = 0; i < 3; i++) {   // Rwc * xn, Rwc = Rcw^T
        ray1[i] = gemm3(c1.Rcw[i], c1.Rcw[3 + i], c1.Rcw[6 + i], xn1, 0.0);
        ray2[i] = gemm3(c2.Rcw[i], c2.Rcw[3 + i], c2.Rcw[6 + i], xn2, 0.0);
    }
    const float cosParallaxRays = (float)(ddot3(ray1, ray2) / (sqrt(ddot3(ray1, ray1)) * sqrt(ddot3(ray2, ray2))));
    const float cosParallaxStereo0 = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo0, cosParallaxStereo2 = cosParallaxStereo0;
    if (bStereo1) cosParallaxStereo1 = stereo_cos(c1.mb, A.s1.depth[o1]);
    else if (bStereo2) cosParallaxStereo2 = stereo_cos(c2.mb, A.s2.depth[o2]);
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min
    int how;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float Am[16];
        for (int c = 0; c < 4; c++) {
            const float T1r0 = c < 3 ? c1.Rcw[c] : c1.tcw[0], T1r1 = c < 3 ? c1.Rcw[3 + c] : c1.tcw[1], T1r2 = c < 3 ? c1.Rcw[6 + c] : c1.tcw[2];
            const float T2r0 = c < 3 ? c2.Rcw[c] : c2.tcw[0], T2r1 = c < 3 ? c2.Rcw[3 + c] : c2.tcw[1], T2r2 = c < 3 ? c2.Rcw[6 + c] : c2.tcw[2];
            Am[c] = xn1[0] * T1r2 - T1r0;
            Am[4 + c] = xn1[1] * T1r2 - T1r1;
            Am[8 + c] = xn2[0] * T2r2 - T2r0;
            Am[12 + c] = xn2[1] * T2r2 - T2r1;
        }
        float v4[4];
        null_vector4_unrolled(Am, v4);
        if (v4[3] == 0) return ORBM_NEWPT_W_ZERO;
        for (int i = 0; i < 3; i++) x3D[i] = v4[i] / v4[3];
        how = ORBM_NEWPT_CREATED_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        if (!unproject_stereo(c1, (A.s1.kps_raw ? A.s1.kps_raw : A.s1.kps)[o1], A.s1.depth[o1], x3D)) return ORBM_NEWPT_EMPTY_STEREO;
        how = ORBM_NEWPT_CREATED_STEREO1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        if (!unproject_stereo(c2, (A.s2.kps_raw ? A.s2.kps_raw : A.s2.kps)[o2], A.s2.depth[o2], x3D)) return ORBM_NEWPT_EMPTY_STEREO;
        how = ORBM_NEWPT_CREATED_STEREO2;
    } else {
        return ORBM_NEWPT_LOW_PARALLAX;
    }
    const float z1 = gemm3(c1.Rcw[6], c1.Rcw[7], c1.Rcw[8], x3D, (double)c1.tcw[2]);
    if (z1 <= 0) return ORBM_NEWPT_BEHIND_1;
    const float z2 = gemm3(c2.Rcw[6], c2.Rcw[7], c2.Rcw[8], x3D, (double)c2.tcw[2]);
    if (z2 <= 0) return ORBM_NEWPT_BEHIND_2;
    if (reproj_rejects(c1, c1.mbf, x3D, z1, kp1, bStereo1, ur1, c1.level_sigma2[kp1.octave])) return ORBM_NEWPT_REPROJ_1;
    if (reproj_rejects(c2, c1.mbf, x3D, z2, kp2, bStereo2, ur2, c2.level_sigma2[kp2.octave])) return ORBM_NEWPT_REPROJ_2;
    const float dist1 = dist_to(x3D, c1.Ow), dist2 = dist_to(x3D, c2.Ow);
    if (dist1 == 0 || dist2 == 0) return ORBM_NEWPT_ZERO_DIST;
    if (P.far_points && (dist1 >= P.th_far_points || dist2 >= P.th_far_points)) return ORBM_NEWPT_FAR;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = c1.scale_factors[kp1.octave] / c2.scale_factors[kp2.octave];
    if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor) return ORBM_NEWPT_SCALE;
    return how;
}

static __device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static __global__ __launch_bounds__(256) void k_create_new_points(NewPtArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* wave_count = (int*)orb_smem;   // [2][4]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cap1 = A.s1.cap_f, cap2 = A.s2.cap_f;
    const orbm_newpt_pair& P = A.pairs[b];
    const int n1 = clampi(A.s1.n[b], 0, cap1), n2 = clampi(A.s2.n[b], 0, cap2);
    const int t1 = P.cam1.camera_type, t2 = P.cam2.camera_type;
    const bool bad_camera = (t1 != ORBM_CAM_PINHOLE && t1 != ORBM_CAM_KB8) || (t2 != ORBM_CAM_PINHOLE && t2 != ORBM_CAM_KB8);
    const size_t base1 = (size_t)b * cap1, base2 = (size_t)b * cap2;
    for (int i = tid; i < cap2; i += 256) A.point_of_2[base2 + i] = -1;
    __syncthreads();
    int base = 0;
    bool any_bad = false;
    for (int c0 = 0, chunk = 0; c0 < cap1; c0 += 256, chunk++) {
        const int i1 = c0 + tid;
        int code = ORBM_NEWPT_NO_MATCH, idx2 = -1;
        float x3D[3] = {0.f, 0.f, 0.f};
        if (i1 < cap1 && !bad_camera) {
            idx2 = A.match12[base1 + i1];
            if (idx2 != -1) {
                if (i1 >= n1 || idx2 < 0 || idx2 >= n2) code = ORBM_NEWPT_BAD_INDEX;
                else code = create_one(A, P, base1 + i1, base2 + idx2, x3D);
            }
        }
        const bool created = code >= ORBM_NEWPT_CREATED_TRIANGULATED && code <= ORBM_NEWPT_CREATED_STEREO2;
        any_bad |= code == ORBM_NEWPT_BAD_INDEX;
        int total;
        const int before = wg_scan_ballot<4>(created, wave_count, chunk, &total);
        if (i1 < cap1) {
            int j = -1;
            if (created) {
                j = base + before;
                if (j < A.cap_new) {
                    orbm_new_point np;
                    np.pos[0] = x3D[0]; np.pos[1] = x3D[1]; np.pos[2] = x3D[2];
                    np.idx1 = i1; np.idx2 = idx2; np.how = code;
                    A.out[(size_t)b * A.cap_new + j] = np;
                    atomicMax(&A.point_of_2[base2 + idx2], j);
                    if (A.s1.has_mp) A.s1.has_mp[base1 + i1] = 1;
                    if (A.s2.has_mp) A.s2.has_mp[base2 + idx2] = 1;
                } else {
                    j = -1;
                }
            }
            A.status[base1 + i1] = (uint8_t)code;
            A.point_of_1[base1 + i1] = j;
        }
        base += total;
    }
    // the pair's flag word: every wave votes, the waves' votes meet in LDS
    const unsigned long long bm = __ballot(any_bad);
    __syncthreads();
    if (lane == 0) wave_count[wv] = bm != 0ull;
    __syncthreads();
    if (tid == 0) {
        uint32_t f = 0;
        if (wave_count[0] | wave_count[1] | wave_count[2] | wave_count[3]) f |= ORBM_NEWPT_PAIR_BAD_INDEX;
        if (base > A.cap_new) f |= ORBM_NEWPT_PAIR_OVERFLOW;
        if (bad_camera) f |= ORBM_NEWPT_PAIR_BAD_CAMERA;
        A.pair_flags[b] = f;
        A.nrequired[b] = base;
        A.nnew[b] = base < A.cap_new ? base : A.cap_new;
    }
}

static bool side_ok(const orbm_newpt_side* s) { return s && s->kps && s->n && s->cap_f >= 1 && (!s->u_right || s->depth); }

extern "C" int orbm_create_new_map_points(const orbm_newpt_side* kf1, const orbm_newpt_side* kf2, const orbm_newpt_pair* d_pairs,
                                          const int32_t* d_match12, int batch, uint8_t* d_status, orbm_new_point* d_new, int cap_new,
                                          int32_t* d_nnew, int32_t* d_nrequired, int32_t* d_point_of_1, int32_t* d_point_of_2,
                                          uint32_t* d_pair_flags, void* stream) {
    if (!side_ok(kf1) || !side_ok(kf2) || !d_pairs || !d_match12 || !d_status || !d_new || !d_nnew || !d_nrequired || !d_point_of_1 ||
        !d_point_of_2 || !d_pair_flags || cap_new < 1 || batch < 0)
        return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    NewPtArgs A;
    A.s1 = *kf1; A.s2 = *kf2; A.pairs = d_pairs; A.match12 = d_match12; A.status = d_status; A.out = d_new; A.cap_new = cap_new; A.nnew = d_nnew;
    A.nrequired = d_nrequired; A.point_of_1 = d_point_of_1; A.point_of_2 = d_point_of_2; A.pair_flags = d_pair_flags;
    hipLaunchKernelGGL(k_create_new_points, dim3(batch), dim3(256), 8 * sizeof(int), (hipStream_t)stream, A);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
struct AppendArgs {
    const orbm_new_point* in;
    const int32_t* nnew;
    int cap_new;
    const orbm_newpt_pair* pairs;
    int batch;
    const orb_keypoint* kps1;
    int cap_f1;
    int32_t* n_mp;
    orbm_map_point* mp;
    int cap_mp, n_desc_rows;
    int32_t* obs_start;
    orbm_observation* obs;
    int cap_obs;
    orbm_refresh_point* ref;
    int32_t* sel;
    int cap_sel;
    int32_t* appended;
};

// the sum of min(max(nnew[x], 0), cap_new) over x < upto, by the whole workgroup (every lane gets it); `red` = 4 ints of LDS
static __device__ int counts_before(const AppendArgs& A, const int upto, int* red) {
    long long s = 0;
    for (int x = threadIdx.x; x < upto; x += 256) s += clampi(A.nnew[x], 0, A.cap_new);
    int v = (int)(s > 0x3fffffff ? 0x3fffffff : s);
    // wave sum by ballots of the bits (counts are < 2^30): integer, order-free
    int ws = 0;
    for (int bit = 0; bit < 30; bit++) ws += __popcll(__ballot((v >> bit) & 1)) << bit;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// how many of `total` new points fit behind the cursor; obs_base = the end of the CSR
static __device__ __forceinline__ int append_fit(const AppendArgs& A, const int cursor, const int total, int* obs_base) {
    *obs_base = 0;
    if (cursor < 0 || cursor > A.cap_mp) return 0;
    const int ob = A.obs_start[cursor];
    *obs_base = ob;
    if (ob < 0 || ob > A.cap_obs) return 0;
    int fit = total;
    if (A.cap_mp - cursor < fit) fit = A.cap_mp - cursor;
    if (A.n_desc_rows - cursor < fit) fit = A.n_desc_rows - cursor;
    if ((A.cap_obs - ob) / 2 < fit) fit = (A.cap_obs - ob) / 2;
    if (A.cap_sel < fit) fit = A.cap_sel;
    return fit < 0 ? 0 : fit;
}

// pair b's points -> records cursor + (points of the pairs before b) + j; reads the cursor, never writes it
static __global__ __launch_bounds__(256) void k_append_new_points(AppendArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* red = (int*)orb_smem;
    const int b = blockIdx.x;
    const int before = counts_before(A, b, red);
    const int total = counts_before(A, A.batch, red);
    const int cursor = *A.n_mp;
    int obs_base;
    const int fit = append_fit(A, cursor, total, &obs_base);
    const int mine = clampi(A.nnew[b], 0, A.cap_new);
    const orbm_newpt_pair& P = A.pairs[b];
    for (int j = threadIdx.x; j < mine; j += 256) {
        const int r = before + j;
        if (r >= fit) break;
        const orbm_new_point np = A.in[(size_t)b * A.cap_new + j];
        const int p = cursor + r;
        orbm_map_point mp;
        mp.pos[0] = np.pos[0]; mp.pos[1] = np.pos[1]; mp.pos[2] = np.pos[2];
        mp.normal[0] = mp.normal[1] = mp.normal[2] = 0.f;
        mp.min_distance = mp.max_distance = mp.angle = 0.f;
        mp.octave = 0; mp.desc_row = p; mp.flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS;
        A.mp[p] = mp;
        const int o = obs_base + 2 * r, first = P.obs_kf2_first ? 1 : 0;
        orbm_observation o1, o2;
        o1.kf = P.kf1; o1.desc_row = P.desc_row0_1 + np.idx1; o1.flags = 0;
        o2.kf = P.kf2; o2.desc_row = P.desc_row0_2 + np.idx2; o2.flags = 0;
        A.obs[o + first] = o1;
        A.obs[o + 1 - first] = o2;
        A.obs_start[p + 1] = o + 2;
        orbm_refresh_point rp;
        rp.ref_kf = P.kf1;
        rp.level = (np.idx1 >= 0 && np.idx1 < A.cap_f1) ? A.kps1[(size_t)b * A.cap_f1 + np.idx1].octave : 0;
        A.ref[p] = rp;
        A.sel[r] = p;
    }
}

// after every k_append_new_points workgroup: the selection's padding, the cursor, the counts
static __global__ __launch_bounds__(256) void k_append_finish(AppendArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* red = (int*)orb_smem;
    const int total = counts_before(A, A.batch, red);
    const int cursor = *A.n_mp;
    int obs_base;
    const int fit = append_fit(A, cursor, total, &obs_base);
    for (int r = fit + threadIdx.x; r < A.cap_sel; r += 256) A.sel[r] = -1;
    __syncthreads();   // every lane has read the cursor
    if (threadIdx.x == 0) {
        *A.n_mp = cursor + fit;
        A.appended[0] = fit;
        A.appended[1] = total - fit;
    }
}

extern "C" int orbm_append_new_map_points(const orbm_new_point* d_new, const int32_t* d_nnew, int cap_new, const orbm_newpt_pair* d_pairs,
                                          int batch, const orb_keypoint* d_kps1, int cap_f1, int32_t* d_n_mp, orbm_map_point* d_mp,
                                          int cap_mp, int n_desc_rows, int32_t* d_obs_start, orbm_observation* d_obs, int cap_obs,
                                          orbm_refresh_point* d_ref, int32_t* d_sel, int cap_sel, int32_t* d_appended, void* stream) {
    if (!d_new || !d_nnew || !d_pairs || !d_kps1 || !d_n_mp || !d_mp || !d_obs_start || !d_obs || !d_ref || !d_sel || !d_appended) return ORB_E_INVALID;
    if (cap_new < 1 || cap_f1 < 1 || cap_mp < 1 || cap_sel < 1 || n_desc_rows < 0 || cap_obs < 0 || batch < 0) return ORB_E_INVALID;
    AppendArgs A;
    A.in = d_new; A.nnew = d_nnew; A.cap_new = cap_new; A.pairs = d_pairs; A.batch = batch; A.kps1 = d_kps1; A.cap_f1 = cap_f1; A.n_mp = d_n_mp;
    A.mp = d_mp; A.cap_mp = cap_mp; A.n_desc_rows = n_desc_rows; A.obs_start = d_obs_start; A.obs = d_obs; A.cap_obs = cap_obs; A.ref = d_ref;
    A.sel = d_sel; A.cap_sel = cap_sel; A.appended = d_appended;
    if (batch > 0) hipLaunchKernelGGL(k_append_new_points, dim3(batch), dim3(256), 4 * sizeof(int), (hipStream_t)stream, A);
    hipLaunchKernelGGL(k_append_finish, dim3(1), dim3(256), 4 * sizeof(int), (hipStream_t)stream, A);
    return launch_status();
}
