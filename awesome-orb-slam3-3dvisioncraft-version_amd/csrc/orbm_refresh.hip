// orbm_refresh.hip — map-point refresh on gfx950: the two MapPoint members the reference recomputes after every change to a point's
// observations or position, written into the orbm_map_point records and the descriptor slab (include/orbhip.h "Map-point refresh").
//
//   refresh_point   MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:372-460) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:485-558)
//                   for one point, by one wave.
//
// Form: one wave64 per point.  The wave walks the point's records in chunks of 64, one record per lane.  Per chunk it (a) computes the unit
// viewing rays lane-parallel and adds them in record order (every lane runs the same serial float sum on v_readlane broadcasts, so the bits are
// those of the reference's loop), (b) compacts the usable records' descriptors, in order, into the wave's slice of dynamic LDS (ballot /
// popcount prefix).  Then lane j owns column j of the distance matrix (columns j + 64 c for N > 64, its descriptors in registers) and the wave
// walks the rows: the row's descriptor is an LDS broadcast read, the distances are xor + popcount, and the lower median is a 9-step MSB-first
// radix select on ballots (distances are integers in 0..256): no sort.  Rows are visited in order by the whole wave, so the first least median
// is a scalar running minimum.
//
// refresh_point<CH> holds CH columns per lane.  It is instantiated twice and launched twice per call, because the LDS slice fixes the
// occupancy: k_refresh_light (CH = 1, 2.25 KiB per wave, four points per 256-lane workgroup) takes the points with at most 64 records — all
// but a handful in a real map — and k_refresh_heavy (CH = 16, 36 KiB, one wave per workgroup) takes the rest: its waves scan the selection 64
// points at a time and visit only those with more than 64 records.  Which launch owns a point depends on its record count alone.
//
// Arithmetic is the reference's cv::Mat arithmetic as the glue is tested under (tests/cpp/mock_orbslam3/opencv2/core/core.hpp): `-` / `+`
// element-wise in float, cv::norm = sqrt of the double dot product summed from 0, Mat / scalar = the scalar converted to float and one float
// division per element.  The library is built with -ffp-contract=off and correctly rounded fp32 division.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"

#define RF_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

static constexpr int RF_LIGHT_MAX = 64;          // records a point of the light launch may have
static constexpr int RF_HEAVY_CH = ORBM_REFRESH_MAX_OBS / 64;
static constexpr int RF_HEAVY_GRID = 1024;       // waves of the heavy launch (each scans 64 points at a time)
static_assert(ORBM_REFRESH_MAX_OBS % 64 == 0, "whole chunks");

struct RefreshArgs {
    orbm_map_point* mp;
    int n_mp;
    uint8_t* mp_desc;
    int n_desc_rows;
    const int32_t* sel;
    int n_sel;
    const int32_t* obs_start;
    const orbm_observation* obs;
    const orbm_refresh_point* ref;
    const orbm_keyframe_center* kf;
    int n_kf;
    const uint8_t* kf_desc;
    int n_kf_desc_rows;
    int32_t* best_obs;
    uint32_t* status;
    orbm_refresh_params prm;
};

// cv::norm of a 3-vector as `Mat / cv::norm(.)` and `float dist = cv::norm(.)` use it: sqrt of the double dot product, converted to float
static __device__ __forceinline__ float norm3f(float x, float y, float z) {
    double s = 0.0;
    s += (double)x * (double)x;
    s += (double)y * (double)y;
    s += (double)z * (double)z;
    return (float)sqrt(s);
}
static __device__ __forceinline__ float lane_bcast(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
static __device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// the selection entry s -> point index, or -1
static __device__ __forceinline__ int selected_point(const RefreshArgs& A, int s) {
    if (s >= A.n_sel) return -1;
    const int p = A.sel ? A.sel[s] : s;
    return (p >= 0 && p < A.n_mp) ? p : -1;
}

// One point by one wave; `lds` is the wave's slice: descriptors [CH*64][32] then observation indices [CH*64] int32.  Every lane of the wave
// takes the same branches (all conditions below are wave-uniform).
template <int CH>
static __device__ __forceinline__ void refresh_point(const RefreshArgs& A, const int p, unsigned char* lds, const int lane) {
    constexpr int CAP = CH * 64;
    uint4* sdesc = (uint4*)lds;
    int32_t* sidx = (int32_t*)(lds + (size_t)CAP * 32);
    const uint32_t what = A.prm.what;
    const int o0 = A.obs_start[p], cnt = A.obs_start[p + 1] - o0;
    orbm_map_point* mp = A.mp + p;
    const uint32_t f = mp->flags;
    uint32_t status = 0;
    int best_obs = -1;
    if ((f & ORBM_MP_VALID) && !(f & ORBM_MP_BAD) && cnt > 0) {
        const float X = mp->pos[0], Y = mp->pos[1], Z = mp->pos[2];
        float nx = 0.f, ny = 0.f, nz = 0.f;   // cv::Mat::zeros(3,1,CV_32F)
        int n = 0, N = 0;
        bool bad_record = false;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int i = c0 + lane;
            bool valid = false, usable = false;
            int row = 0;
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if (i < cnt) {
                const orbm_observation ob = A.obs[(size_t)o0 + i];
                valid = ob.kf >= 0 && ob.kf < A.n_kf && ob.desc_row >= 0 && ob.desc_row < A.n_kf_desc_rows;
                usable = valid && !(ob.flags & ORBM_OBS_KF_BAD);   // MapPoint.cc:397
                row = ob.desc_row;
                if (valid && (what & ORBM_REFRESH_NORMAL_DEPTH)) {   // normali / cv::norm(normali), MapPoint.cc:516-527
                    const float* Ow = (ob.flags & ORBM_OBS_RIGHT) ? A.kf[ob.kf].right : A.kf[ob.kf].left;
                    const float dx = X - Ow[0], dy = Y - Ow[1], dz = Z - Ow[2];
                    const float nr = norm3f(dx, dy, dz);
                    ux = dx / nr; uy = dy / nr; uz = dz / nr;
                }
            }
            const unsigned long long in_range = __ballot(i < cnt), vm = __ballot(valid), um = __ballot(usable);
            bad_record |= vm != in_range;
            if (what & ORBM_REFRESH_NORMAL_DEPTH)
                for (unsigned long long m = vm; m; m &= m - 1ull) {   // normal = normal + ..., in record order
                    const int j = __ffsll((long long)m) - 1;
                    nx += lane_bcast(ux, j);
                    ny += lane_bcast(uy, j);
                    nz += lane_bcast(uz, j);
                }
            n += __popcll(vm);
            if (what & ORBM_REFRESH_DESCRIPTOR) {
                const int pos = N + __popcll(um & ((1ull << lane) - 1ull));
                if (usable && pos < CAP) {
                    const uint4* s = (const uint4*)(A.kf_desc + (size_t)row * 32);
                    sdesc[2 * pos] = s[0];
                    sdesc[2 * pos + 1] = s[1];
                    sidx[pos] = i;
                }
            }
            N += __popcll(um);
        }
        if (bad_record) status |= ORBM_REFRESH_BAD_RECORD;
        if (N > ORBM_REFRESH_MAX_OBS) {
            status |= ORBM_REFRESH_OVERFLOW;
        } else {
            if ((what & ORBM_REFRESH_DESCRIPTOR) && N > 0) {
                RF_WAVE_SYNC();
                const int nch = (N + 63) >> 6;
                uint4 own[CH][2];
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    const int col = lane + 64 * c;
                    own[c][0] = own[c][1] = make_uint4(0, 0, 0, 0);
                    if (c < nch && col < N) { own[c][0] = sdesc[2 * col]; own[c][1] = sdesc[2 * col + 1]; }
                }
                const int k = (N - 1) >> 1;   // vDists[0.5*(N-1)]
                int best_median = 0x7fffffff, best_idx = 0;
                for (int i = 0; i < N; i++) {
                    const uint4 r0 = sdesc[2 * i], r1 = sdesc[2 * i + 1];
                    int d[CH];
#pragma unroll
                    for (int c = 0; c < CH; c++) d[c] = (c < nch && lane + 64 * c < N) ? hamming256(own[c][0], own[c][1], r0, r1) : 0xFFFF;
                    // the k-th smallest of the row, MSB first: the candidates are the entries that agree with `median` above bit b
                    int median = 0, kk = k;
#pragma unroll
                    for (int b = 8; b >= 0; b--) {
                        int zeros = 0;
#pragma unroll
                        for (int c = 0; c < CH; c++)
                            if (c < nch) zeros += __popcll(__ballot((d[c] >> b) == (median >> b)));
                        if (kk >= zeros) { kk -= zeros; median |= 1 << b; }
                    }
                    if (median < best_median) { best_median = median; best_idx = i; }   // strict: the first least median
                }
                best_obs = sidx[best_idx];
                const int drow = mp->desc_row;
                if (drow >= 0 && drow < A.n_desc_rows && lane < 2) ((uint4*)(A.mp_desc + (size_t)drow * 32))[lane] = sdesc[2 * best_idx + lane];
                status |= ORBM_REFRESHED_DESCRIPTOR;
            }
            if ((what & ORBM_REFRESH_NORMAL_DEPTH) && n > 0) {
                const orbm_refresh_point rp = A.ref[p];
                if (rp.ref_kf >= 0 && rp.ref_kf < A.n_kf && rp.level >= 0 && rp.level < A.prm.nlevels) {
                    const float* Or = A.kf[rp.ref_kf].left;
                    const float dist = norm3f(X - Or[0], Y - Or[1], Z - Or[2]);
                    const float max_distance = dist * A.prm.scale_factors[rp.level];
                    const float min_distance = max_distance / A.prm.scale_factors[A.prm.nlevels - 1];
                    const float fn = (float)n;
                    if (lane == 0) {
                        mp->normal[0] = nx / fn;
                        mp->normal[1] = ny / fn;
                        mp->normal[2] = nz / fn;
                        mp->min_distance = min_distance;
                        mp->max_distance = max_distance;
                    }
                    status |= ORBM_REFRESHED_NORMAL_DEPTH;
                } else {
                    status |= ORBM_REFRESH_BAD_RECORD;
                }
            }
        }
    }
    if (lane == 0) {
        A.best_obs[p] = best_obs;
        A.status[p] = status;
    }
    RF_WAVE_SYNC();   // the wave's next point rewrites the slice
}

static constexpr size_t rf_slice_bytes(int ch) { return (size_t)ch * 64 * 36; }

// points with at most RF_LIGHT_MAX records: one wave each, four per workgroup
static __global__ __launch_bounds__(256) void k_refresh_light(RefreshArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = selected_point(A, blockIdx.x * 4 + wv);
    if (p < 0) return;
    if (A.obs_start[p + 1] - A.obs_start[p] > RF_LIGHT_MAX) return;   // k_refresh_heavy's
    refresh_point<1>(A, p, orb_smem + wv * rf_slice_bytes(1), lane);
}

// points with more records: each single-wave workgroup scans the selection 64 entries at a time and visits the heavy ones
static __global__ __launch_bounds__(64) void k_refresh_heavy(RefreshArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const int lane = threadIdx.x;
    for (int s0 = blockIdx.x * 64; s0 < A.n_sel; s0 += gridDim.x * 64) {
        const int p = selected_point(A, s0 + lane);
        const bool heavy = p >= 0 && A.obs_start[p + 1] - A.obs_start[p] > RF_LIGHT_MAX;
        for (unsigned long long m = __ballot(heavy); m; m &= m - 1ull)
            refresh_point<RF_HEAVY_CH>(A, __builtin_amdgcn_readlane(p, __ffsll((long long)m) - 1), orb_smem, lane);
    }
}

extern "C" int orbm_refresh_map_points(orbm_map_point* d_mp, int n_mp, uint8_t* d_mp_desc, int n_desc_rows, const int32_t* d_sel, int n_sel,
                                       const int32_t* d_obs_start, const orbm_observation* d_obs, const orbm_refresh_point* d_ref,
                                       const orbm_keyframe_center* d_kf, int n_kf, const uint8_t* d_kf_desc, int n_kf_desc_rows,
                                       const orbm_refresh_params* params, int32_t* d_best_obs, uint32_t* d_status, void* stream) {
    if (!d_mp || !d_mp_desc || !d_obs_start || !d_obs || !d_ref || !d_kf || !d_kf_desc || !params || !d_best_obs || !d_status) return ORB_E_INVALID;
    if (n_mp < 0 || n_desc_rows < 0 || n_kf < 0 || n_kf_desc_rows < 0 || (d_sel && n_sel < 0)) return ORB_E_INVALID;
    if (params->nlevels < 1 || params->nlevels > 16) return ORB_E_INVALID;
    if (params->what == 0u || (params->what & ~(ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH)) != 0u) return ORB_E_INVALID;
    if (misaligned16(d_mp_desc) || misaligned16(d_kf_desc)) return ORB_E_INVALID;   // 16-byte loads / stores of the descriptor rows
    const int n = d_sel ? n_sel : n_mp;
    if (n == 0 || n_mp == 0) return ORB_OK;
    RefreshArgs A;
    A.mp = d_mp; A.n_mp = n_mp; A.mp_desc = d_mp_desc; A.n_desc_rows = n_desc_rows; A.sel = d_sel; A.n_sel = n; A.obs_start = d_obs_start;
    A.obs = d_obs; A.ref = d_ref; A.kf = d_kf; A.n_kf = n_kf; A.kf_desc = d_kf_desc; A.n_kf_desc_rows = n_kf_desc_rows; A.best_obs = d_best_obs;
    A.status = d_status; A.prm = *params;
    hipLaunchKernelGGL(k_refresh_light, dim3((n + 3) / 4), dim3(256), 4 * rf_slice_bytes(1), (hipStream_t)stream, A);
    const int chunks = (n + 63) / 64;
    hipLaunchKernelGGL(k_refresh_heavy, dim3(chunks < RF_HEAVY_GRID ? chunks : RF_HEAVY_GRID), dim3(64), rf_slice_bytes(RF_HEAVY_CH), (hipStream_t)stream, A);
    return launch_status();
}
