// two_view.hip — TwoViewReconstruction::Reconstruct on gfx950, the Pinhole path (reference src/TwoViewReconstruction.cc:51-1013;
// include/orbhip.h "TwoViewReconstruction"), for a batch of independent frame pairs.
//
//   k_tvr_prepare      one workgroup per problem: Normalize of both frames (four serial float chains over ALL keys of a frame, one lane each,
//                      the keys staged through LDS 256 at a time), T1 / T2 / T2.inv() / T2.t(), then the ordered compaction of matches12 into
//                      the workspace as eight planes (pixel and normalised u1 v1 u2 v2): match order is the score's summation order.
//   k_tvr_models       one lane per (problem, model, iteration): the eight-point DLT.  A^T A and the Jacobi eigenvectors live in dynamic LDS
//                      as [element][lane] planes (162 doubles per lane, 81 KB per wave: lane i touches word pair i of a plane, no bank
//                      conflict); F's rank-2 step (svd3) runs in registers; then the denormalisation and H21i.inv().
//   k_tvr_score        one lane per hypothesis, the matches walked serially: every lane runs the reference's own in-order float sum.  The
//                      match coordinates are wave-uniform loads; the flags accumulate in a register, one 64-bit word stored per 64 matches;
//                      the two thresholds are selects.  H and F hypotheses are different waves.
//   k_tvr_reconstruct  one 512-lane workgroup per problem.  Wave 0 picks the first strictly greatest score of each model (the reference's
//                      `currentScore>score` from 0), then `SH+SF == 0` and `RH > 0.50`.  One lane per motion hypothesis (4 for F, 8 for H)
//                      builds R, t, P2 and O2; CheckRT runs one wave per hypothesis, one match per lane in chunks of 64: nGood is a popcount,
//                      the idx-th cosine a bitwise radix select over the ordered bit patterns.  Lane 0 runs the accept logic; the winner's
//                      CheckRT runs once more over all waves to write vP3D / vbTriangulated.
// Nothing couples two hypotheses before the pick, and the pick compares keys: results do not depend on any execution order.
//
// Arithmetic: rule R7 of DESIGN.md section 2.  The library is built with -ffp-contract=off and correctly rounded fp32 division / sqrt; every
// operation below but the acos of the parallax is IEEE + - * / sqrt, so x86 and gfx950 agree bit for bit on everything else.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/orbhip.h"
#include "lds_optin.inc"
#include "kb8_geom.inc"
#include "wg_scan.inc"
#include "workspace.inc"

static constexpr int TV_PREP_WG = 256, TV_PREP_NW = TV_PREP_WG / 64;
static constexpr int TV_SWEEPS9 = 12;   // cyclic Jacobi sweeps of the 9x9 Gram matrix (R7: the off-diagonal norm stops falling after 8)
static constexpr int TV_SWEEPS3 = 10;   // one-sided Jacobi sweeps of svd3 (R7: orthogonal to 1e-15 after 5)
static constexpr int TV_LANES = 64;     // hypotheses of a workgroup of k_tvr_models / k_tvr_score: one wave
static constexpr size_t TV_MODEL_LDS = (size_t)2 * 81 * TV_LANES * sizeof(double);
static constexpr int TV_PLANES = 8;     // u1 v1 u2 v2 in pixels, then normalised
static constexpr int TV_T_FLOATS = 36;  // T1, T2, T2inv, T2t
static constexpr int TV_REC_WG = 512;   // k_tvr_reconstruct: 8 waves = the 8 motion hypotheses of ReconstructH
static constexpr int TV_MOTION = 27;    // R[9] t[3] P2[12] O2[3] of a motion hypothesis

// The workspace, listed once (workspace.inc): sizing walks it from a null base.
struct TvWork {
    int32_t* n;         // [batch] N = mvMatches12.size()
    uint32_t* status;   // [batch]
    float* T;           // [batch][TV_T_FLOATS]
    float* planes;      // [batch][TV_PLANES][cap_k]
    float* inv;         // [batch][cap_its][9] H12i
    int32_t* i1;        // [batch][cap_k] mvMatches12[i].first
    float* cosv;        // [batch][8][cap_k] vCosParallax of each motion hypothesis
};
static __host__ __device__ TvWork tv_layout(void* base, int batch, int cap_k, int cap_its, size_t* bytes) {
    WsCursor c{(unsigned char*)base, 256, 0};
    TvWork w;
    w.n = c.take<int32_t>((size_t)batch);
    w.status = c.take<uint32_t>((size_t)batch);
    w.T = c.take<float>((size_t)batch * TV_T_FLOATS);
    w.planes = c.take<float>((size_t)batch * TV_PLANES * (size_t)cap_k);
    w.inv = c.take<float>((size_t)batch * (size_t)cap_its * 9);
    w.i1 = c.take<int32_t>((size_t)batch * (size_t)cap_k);
    w.cosv = c.take<float>((size_t)batch * 8 * (size_t)cap_k);
    *bytes = c.off;
    return w;
}

struct TvArgs {
    const orbm_tvr_problem* prob;
    const orb_keypoint* keys1;
    const orb_keypoint* keys2;
    int cap_k;
    const int32_t* matches12;
    const int32_t* sets;
    int cap_its;
    float* score;
    float* model;
    unsigned long long* mask;
    int words;
    orbm_tvr_result* result;
    float* p3d;
    uint8_t* triangulated;
    TvWork w;
};

static __device__ __forceinline__ int tv_its(const orbm_tvr_problem* P, int cap_its) {
    const int its = P->max_its < 0 ? 0 : P->max_its;
    return its > cap_its ? cap_its : its;
}

// a set is usable when its eight indices lie in [0, N) and are distinct
static __device__ __forceinline__ bool tv_set_ok(const int32_t* set, int N) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        ok = ok && set[j] >= 0 && set[j] < N;
#pragma unroll
        for (int k = 0; k < j; k++) ok = ok && set[j] != set[k];
    }
    return ok;
}

// a float cv::Mat product of two 3x3 (cv::gemm): the double sum of the double products from 0 in k order, rounded once
static __device__ __forceinline__ void tv_gemm3(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += (double)A[i * 3 + k] * (double)B[k * 3 + j];
            C[i * 3 + j] = (float)acc;
        }
}

// Mat::inv() of a 3x3 CV_32F (R7): determinant and cofactors in double, scaled by the double 1 / det, rounded once; det == 0 -> the zero matrix
static __device__ __forceinline__ void tv_inv3(const float* S, float* t) {
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
    double d = s00 * (s11 * s22 - s12 * s21) - s01 * (s10 * s22 - s12 * s20) + s02 * (s10 * s21 - s11 * s20);
    if (d != 0.0) {
        d = 1.0 / d;
        t[0] = (float)((s11 * s22 - s12 * s21) * d);
        t[1] = (float)((s02 * s21 - s01 * s22) * d);
        t[2] = (float)((s01 * s12 - s02 * s11) * d);
        t[3] = (float)((s12 * s20 - s10 * s22) * d);
        t[4] = (float)((s00 * s22 - s02 * s20) * d);
        t[5] = (float)((s02 * s10 - s00 * s12) * d);
        t[6] = (float)((s10 * s21 - s11 * s20) * d);
        t[7] = (float)((s01 * s20 - s00 * s21) * d);
        t[8] = (float)((s00 * s11 - s01 * s10) * d);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) t[i] = 0.f;
    }
}

// ---- the null vector of a float system with nine columns (the last row of cv::SVDecomp's vt, R7): cyclic Jacobi on A^T A in double, the rotation
// of jacobi4_rotate (kb8_geom.inc) at n = 9.  M and V are this lane's planes: element e at M[e * TV_LANES].
#define TVM(X, i, j) X[((i) * 9 + (j)) * TV_LANES]
static __device__ __forceinline__ void tv_null9_init(double* M, double* V) {
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) { TVM(M, i, j) = 0.0; TVM(V, i, j) = i == j ? 1.0 : 0.0; }
}
// one row of A: M += a^T a (the sums of A^T A grow in row order from 0)
static __device__ __forceinline__ void tv_null9_row(double* M, const float* a) {
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) TVM(M, i, j) += (double)a[i] * (double)a[j];
}
static __device__ __forceinline__ void tv_null9_rotate(double* M, double* V, const int p, const int q) {
    const double apq = TVM(M, p, q);
    if (apq == 0.0) return;
    const double th = (TVM(M, q, q) - TVM(M, p, p)) / (2.0 * apq);
    const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
    for (int k = 0; k < 9; k++) { const double a = TVM(M, k, p), b = TVM(M, k, q); TVM(M, k, p) = c * a - sn * b; TVM(M, k, q) = sn * a + c * b; }
    for (int k = 0; k < 9; k++) { const double a = TVM(M, p, k), b = TVM(M, q, k); TVM(M, p, k) = c * a - sn * b; TVM(M, q, k) = sn * a + c * b; }
    for (int k = 0; k < 9; k++) { const double a = TVM(V, k, p), b = TVM(V, k, q); TVM(V, k, p) = c * a - sn * b; TVM(V, k, q) = sn * a + c * b; }
}
static __device__ __forceinline__ void tv_null9_solve(double* M, double* V, float* v9) {
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS9; sweep++)
#pragma unroll 1
        for (int p = 0; p < 8; p++)
#pragma unroll 1
            for (int q = p + 1; q < 9; q++) tv_null9_rotate(M, V, p, q);
    int m = 0;
    double least = TVM(M, 0, 0);
    for (int i = 1; i < 9; i++) { const double d = TVM(M, i, i); if (d < least) { least = d; m = i; } }
#pragma unroll
    for (int k = 0; k < 9; k++) v9[k] = (float)TVM(V, k, m);
}

// ---- svd3 (R7): the full SVD of a 3x3 float matrix in double by one-sided Jacobi on its columns.  w descending, U (row-major, column i = u_i)
// and Vt.  Only + - * / sqrt and comparisons.
template <int P, int Q> static __device__ __forceinline__ void tv_svd3_rotate(double* G, double* V) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { alpha += G[k * 3 + P] * G[k * 3 + P]; beta += G[k * 3 + Q] * G[k * 3 + Q]; gamma += G[k * 3 + P] * G[k * 3 + Q]; }
    if (gamma == 0.0) return;
    const double th = (beta - alpha) / (2.0 * gamma);
    const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
    for (int k = 0; k < 3; k++) { const double a = G[k * 3 + P], b = G[k * 3 + Q]; G[k * 3 + P] = c * a - sn * b; G[k * 3 + Q] = sn * a + c * b; }
#pragma unroll
    for (int k = 0; k < 3; k++) { const double a = V[k * 3 + P], b = V[k * 3 + Q]; V[k * 3 + P] = c * a - sn * b; V[k * 3 + Q] = sn * a + c * b; }
}
template <int A, int B> static __device__ __forceinline__ void tv_svd3_swap(double* w, double* G, double* V) {
    double x = w[A]; w[A] = w[B]; w[B] = x;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        x = G[k * 3 + A]; G[k * 3 + A] = G[k * 3 + B]; G[k * 3 + B] = x;
        x = V[k * 3 + A]; V[k * 3 + A] = V[k * 3 + B]; V[k * 3 + B] = x;
    }
}
// the normalised cross product a x b into column `col` of U
static __device__ __forceinline__ void tv_svd3_cross(const double* a, const double* b, double* U, int col) {
    const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    const double n = sqrt(x * x + y * y + z * z);
    U[col] = x / n; U[3 + col] = y / n; U[6 + col] = z / n;
}
static __device__ __forceinline__ void tv_svd3(const float* A, double* w, double* U, double* Vt) {
    double G[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { G[i] = (double)A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS3; sweep++) {
        tv_svd3_rotate<0, 1>(G, V);
        tv_svd3_rotate<0, 2>(G, V);
        tv_svd3_rotate<1, 2>(G, V);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = sqrt(G[i] * G[i] + G[3 + i] * G[3 + i] + G[6 + i] * G[6 + i]);
    // selection sort, descending, the first of equals
    if (w[0] < w[1]) { if (w[1] < w[2]) tv_svd3_swap<0, 2>(w, G, V); else tv_svd3_swap<0, 1>(w, G, V); }
    else if (w[0] < w[2]) tv_svd3_swap<0, 2>(w, G, V);
    if (w[1] < w[2]) tv_svd3_swap<1, 2>(w, G, V);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) Vt[i * 3 + k] = V[k * 3 + i];
    if (w[0] == 0.0) {   // the zero matrix: U = I
#pragma unroll
        for (int i = 0; i < 9; i++) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double tiny = w[0] * 0x1p-40;
    double u0[3], u1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { u0[k] = G[k * 3] / w[0]; U[k * 3] = u0[k]; }
    if (w[1] < tiny) {   // rank one: u1 = u0 x (the axis u0 is least along, the first of equals)
        int ax = 0;
        double least = fabs(u0[0]);
        if (fabs(u0[1]) < least) { least = fabs(u0[1]); ax = 1; }
        if (fabs(u0[2]) < least) ax = 2;
        const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        tv_svd3_cross(u0, e, U, 1);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) U[k * 3 + 1] = G[k * 3 + 1] / w[1];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) u1[k] = U[k * 3 + 1];
    if (w[2] < tiny) {
        tv_svd3_cross(u0, u1, U, 2);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) U[k * 3 + 2] = G[k * 3 + 2] / w[2];
    }
}

// ComputeF21's tail (:376-380): SVDecomp of Fpre, w(2) = 0, u * diag(w) * vt (two gemms, left to right)
static __device__ __forceinline__ void tv_rank2(const float* Fpre, float* Fn) {
    double w[3], U[9], Vt[9];
    tv_svd3(Fpre, w, U, Vt);
    float uf[9], vtf[9], D[9], tmp[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { uf[i] = (float)U[i]; vtf[i] = (float)Vt[i]; D[i] = 0.f; }
    D[0] = (float)w[0]; D[4] = (float)w[1];   // D[8] = w.at<float>(2) = 0
    tv_gemm3(uf, D, tmp);
    tv_gemm3(tmp, vtf, Fn);
}

// ------------------------------------------------------------------------------------------------------------------------------ k_tvr_prepare
static __global__ __launch_bounds__(TV_PREP_WG) void k_tvr_prepare(TvArgs A) {
    __shared__ float s_xy[4][TV_PREP_WG];   // a chunk of keys: x1 y1 x2 y2
    __shared__ float s_mean[4], s_scale[4];
    __shared__ int s_scan[2 * TV_PREP_NW];
    __shared__ unsigned s_status;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cap_k = A.cap_k;
    const orbm_tvr_problem* P = A.prob + b;
    unsigned status = 0;
    int n1 = P->n_keys1, n2 = P->n_keys2;
    if (n1 < 0 || n1 > cap_k) { n1 = n1 < 0 ? 0 : cap_k; status |= ORBM_TVR_N_CLAMPED; }
    if (n2 < 0 || n2 > cap_k) { n2 = n2 < 0 ? 0 : cap_k; status |= ORBM_TVR_N_CLAMPED; }
    if (P->max_its > A.cap_its) status |= ORBM_TVR_ITS_CLAMPED;
    const orb_keypoint* k1 = A.keys1 + (size_t)b * cap_k;
    const orb_keypoint* k2 = A.keys2 + (size_t)b * cap_k;
    if (tid == 0) s_status = status;
    // ---- Normalize (:833-879): chain wv (lane 0 of wave wv) sums plane wv over ALL keys of its frame in index order
    const int nmax = n1 > n2 ? n1 : n2, nmine = wv < 2 ? n1 : n2;
    float acc = 0.f, mean = 0.f;
    for (int pass = 0; pass < 2; pass++) {
        acc = 0.f;
        for (int c0 = 0; c0 < nmax; c0 += TV_PREP_WG) {
            const int i = c0 + tid;
            if (i < n1) { s_xy[0][tid] = k1[i].x; s_xy[1][tid] = k1[i].y; }
            if (i < n2) { s_xy[2][tid] = k2[i].x; s_xy[3][tid] = k2[i].y; }
            __syncthreads();
            if (lane == 0) {
                const int cnt = nmine - c0 < TV_PREP_WG ? nmine - c0 : TV_PREP_WG;
                if (pass == 0) for (int k = 0; k < cnt; k++) acc += s_xy[wv][k];
                else for (int k = 0; k < cnt; k++) acc += fabsf(s_xy[wv][k] - mean);
            }
            __syncthreads();
        }
        acc = acc / nmine;   // meanX = meanX/N: a float division
        if (pass == 0) mean = acc;
    }
    if (lane == 0) { s_mean[wv] = mean; s_scale[wv] = (float)(1.0 / (double)acc); }   // sX = 1.0/meanDevX
    __syncthreads();
    float* T = A.w.T + (size_t)b * TV_T_FLOATS;
    if (tid == 0) {
        float Tm[2][9];
        for (int f = 0; f < 2; f++) {
            const float sX = s_scale[2 * f], sY = s_scale[2 * f + 1];
            const float t[9] = {sX, 0.f, -s_mean[2 * f] * sX, 0.f, sY, -s_mean[2 * f + 1] * sY, 0.f, 0.f, 1.f};
            for (int i = 0; i < 9; i++) { Tm[f][i] = t[i]; T[f * 9 + i] = t[i]; }
        }
        float inv[9];
        tv_inv3(Tm[1], inv);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { T[18 + i * 3 + j] = inv[i * 3 + j]; T[27 + i * 3 + j] = Tm[1][j * 3 + i]; }
    }
    // ---- mvMatches12 (:67-79): the ordered compaction; an entry outside [0, n_keys2) counts as unmatched
    const int32_t* m12 = A.matches12 + (size_t)b * cap_k;
    float* pl = A.w.planes + (size_t)b * TV_PLANES * cap_k;
    int base = 0, chunk = 0;
    for (int c0 = 0; c0 < n1; c0 += TV_PREP_WG, chunk++) {
        const int i = c0 + tid;
        const int m = i < n1 ? m12[i] : -1;
        const bool keep = m >= 0 && m < n2;
        if (m >= n2) atomicOr(&s_status, (unsigned)ORBM_TVR_BAD_INDEX);   // a flag: the order of the ORs cannot show
        int total;
        const int pos = base + wg_scan_ballot<TV_PREP_NW>(keep, s_scan, chunk, &total);
        if (keep) {
            const float u1 = k1[i].x, v1 = k1[i].y, u2 = k2[m].x, v2 = k2[m].y;
            A.w.i1[(size_t)b * cap_k + pos] = i;
            pl[pos] = u1; pl[(size_t)cap_k + pos] = v1; pl[(size_t)2 * cap_k + pos] = u2; pl[(size_t)3 * cap_k + pos] = v2;
            pl[(size_t)4 * cap_k + pos] = (u1 - s_mean[0]) * s_scale[0];
            pl[(size_t)5 * cap_k + pos] = (v1 - s_mean[1]) * s_scale[1];
            pl[(size_t)6 * cap_k + pos] = (u2 - s_mean[2]) * s_scale[2];
            pl[(size_t)7 * cap_k + pos] = (v2 - s_mean[3]) * s_scale[3];
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        A.w.n[b] = base;
        A.w.status[b] = s_status | (base < 8 ? (unsigned)ORBM_TVR_TOO_FEW : 0u);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------- k_tvr_models
static __global__ __launch_bounds__(TV_LANES) void k_tvr_models(TvArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const int b = blockIdx.z, model = blockIdx.y, lane = threadIdx.x, it = blockIdx.x * TV_LANES + lane, cap_k = A.cap_k;
    const int N = A.w.n[b];
    if (N < 8 || it >= tv_its(A.prob + b, A.cap_its)) return;
    const size_t h = (size_t)b * A.cap_its + it;
    const int32_t* set = A.sets + h * 8;
    float* out = A.model + (((size_t)b * 2 + model) * A.cap_its + it) * 9;
    if (!tv_set_ok(set, N)) {
        const float nan = __int_as_float(0x7fc00000);
        for (int k = 0; k < 9; k++) out[k] = nan;
        if (model == 0) for (int k = 0; k < 9; k++) A.w.inv[h * 9 + k] = nan;
        atomicOr(A.w.status + b, (unsigned)ORBM_TVR_BAD_SAMPLE);
        return;
    }
    double* M = (double*)orb_smem + lane;
    double* V = M + 81 * TV_LANES;
    const float* pl = A.w.planes + (size_t)b * TV_PLANES * cap_k;
    const float* T = A.w.T + (size_t)b * TV_T_FLOATS;
    tv_null9_init(M, V);
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
        const int idx = set[j];
        const float u1 = pl[(size_t)4 * cap_k + idx], v1 = pl[(size_t)5 * cap_k + idx], u2 = pl[(size_t)6 * cap_k + idx], v2 = pl[(size_t)7 * cap_k + idx];
        if (model == 0) {   // ComputeH21 (:310-337)
            const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
            tv_null9_row(M, r0);
            tv_null9_row(M, r1);
        } else {            // ComputeF21 (:352-368)
            const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
            tv_null9_row(M, r);
        }
    }
    float v9[9], tmp[9], res[9];
    tv_null9_solve(M, V, v9);
    if (model == 0) {
        float inv[9];
        tv_gemm3(T + 18, v9, tmp);   // H21i = T2inv*Hn*T1
        tv_gemm3(tmp, T, res);
        tv_inv3(res, inv);           // H12i = H21i.inv()
        for (int k = 0; k < 9; k++) A.w.inv[h * 9 + k] = inv[k];
    } else {
        float Fn[9];
        tv_rank2(v9, Fn);
        tv_gemm3(T + 27, Fn, tmp);   // F21i = T2t*Fn*T1
        tv_gemm3(tmp, T, res);
    }
    for (int k = 0; k < 9; k++) out[k] = res[k];
}

// -------------------------------------------------------------------------------------------------------------------------------- k_tvr_score
static __global__ __launch_bounds__(TV_LANES) void k_tvr_score(TvArgs A) {
    const int b = blockIdx.z, model = blockIdx.y, lane = threadIdx.x, it = blockIdx.x * TV_LANES + lane, cap_k = A.cap_k;
    const int N = A.w.n[b];
    const orbm_tvr_problem* P = A.prob + b;
    if (N < 8 || it >= tv_its(P, A.cap_its)) return;
    const size_t h = (size_t)b * A.cap_its + it, hm = ((size_t)b * 2 + model) * A.cap_its + it;
    unsigned long long* mask = A.mask + hm * A.words;
    if (!tv_set_ok(A.sets + h * 8, N)) {   // BAD_SAMPLE: a NaN score and an empty mask
        A.score[hm] = __int_as_float(0x7fc00000);
        for (int w = 0; w < A.words; w++) mask[w] = 0ull;
        return;
    }
    const float* pl = A.w.planes + (size_t)b * TV_PLANES * cap_k;
    const float* pu1 = pl, *pv1 = pl + cap_k, *pu2 = pl + (size_t)2 * cap_k, *pv2 = pl + (size_t)3 * cap_k;
    const float sigma = P->sigma;
    const float invSigmaSquare = (float)(1.0 / (double)(sigma * sigma));
    float m[9], mi[9];
    for (int k = 0; k < 9; k++) { m[k] = A.model[hm * 9 + k]; mi[k] = model == 0 ? A.w.inv[h * 9 + k] : 0.f; }
    float score = 0.f;
    unsigned long long bitsw = 0ull;
    if (model == 0) {   // CheckHomography (:383-468)
        const float th = 5.991f;
        for (int i = 0; i < N; i++) {
            const float u1 = pu1[i], v1 = pv1[i], u2 = pu2[i], v2 = pv2[i];
            const float w2in1inv = (float)(1.0 / (double)(mi[6] * u2 + mi[7] * v2 + mi[8]));
            const float u2in1 = (mi[0] * u2 + mi[1] * v2 + mi[2]) * w2in1inv;
            const float v2in1 = (mi[3] * u2 + mi[4] * v2 + mi[5]) * w2in1inv;
            const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
            const float chiSquare1 = squareDist1 * invSigmaSquare;
            const bool out1 = chiSquare1 > th;
            const float s1 = score + (th - chiSquare1);
            score = out1 ? score : s1;
            const float w1in2inv = (float)(1.0 / (double)(m[6] * u1 + m[7] * v1 + m[8]));
            const float u1in2 = (m[0] * u1 + m[1] * v1 + m[2]) * w1in2inv;
            const float v1in2 = (m[3] * u1 + m[4] * v1 + m[5]) * w1in2inv;
            const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
            const float chiSquare2 = squareDist2 * invSigmaSquare;
            const bool out2 = chiSquare2 > th;
            const float s2 = score + (th - chiSquare2);
            score = out2 ? score : s2;
            bitsw |= (unsigned long long)(!out1 && !out2) << (i & 63);
            if ((i & 63) == 63) { mask[i >> 6] = bitsw; bitsw = 0ull; }
        }
    } else {            // CheckFundamental (:470-548)
        const float th = 3.841f, thScore = 5.991f;
        for (int i = 0; i < N; i++) {
            const float u1 = pu1[i], v1 = pv1[i], u2 = pu2[i], v2 = pv2[i];
            const float a2 = m[0] * u1 + m[1] * v1 + m[2];
            const float b2 = m[3] * u1 + m[4] * v1 + m[5];
            const float c2 = m[6] * u1 + m[7] * v1 + m[8];
            const float num2 = a2 * u2 + b2 * v2 + c2;
            const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
            const float chiSquare1 = squareDist1 * invSigmaSquare;
            const bool out1 = chiSquare1 > th;
            const float s1 = score + (thScore - chiSquare1);
            score = out1 ? score : s1;
            const float a1 = m[0] * u2 + m[3] * v2 + m[6];
            const float b1 = m[1] * u2 + m[4] * v2 + m[7];
            const float c1 = m[2] * u2 + m[5] * v2 + m[8];
            const float num1 = a1 * u1 + b1 * v1 + c1;
            const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
            const float chiSquare2 = squareDist2 * invSigmaSquare;
            const bool out2 = chiSquare2 > th;
            const float s2 = score + (thScore - chiSquare2);
            score = out2 ? score : s2;
            bitsw |= (unsigned long long)(!out1 && !out2) << (i & 63);
            if ((i & 63) == 63) { mask[i >> 6] = bitsw; bitsw = 0ull; }
        }
    }
    if (N & 63) mask[N >> 6] = bitsw;
    for (int w = (N + 63) >> 6; w < A.words; w++) mask[w] = 0ull;
    A.score[hm] = score;
}

// -------------------------------------------------------------------------------------------------------------------------- k_tvr_reconstruct
static __device__ __forceinline__ double tv_det3(const float* S) {   // cv::determinant of a 3x3 CV_32F: in double
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
    return s00 * (s11 * s22 - s12 * s21) - s01 * (s10 * s22 - s12 * s20) + s02 * (s10 * s21 - s11 * s20);
}
static __device__ __forceinline__ bool tv_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// t / cv::norm(t): the norm in double, every element times the double 1 / norm, rounded once
static __device__ __forceinline__ void tv_unit3(float* t) {
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) n2 += (double)t[i] * (double)t[i];
    const double alpha = 1.0 / sqrt(n2);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = (float)((double)t[i] * alpha);
}
static __device__ __forceinline__ void tv_svd3f(const float* A, float* w, float* U, float* Vt) {   // cv::SVD::compute of a CV_32F matrix: narrowed
    double wd[3], Ud[9], Vtd[9];
    tv_svd3(A, wd, Ud, Vtd);
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = (float)Ud[i]; Vt[i] = (float)Vtd[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = (float)wd[i];
}

// ReconstructF's motions (:563-572, DecomposeE :993-1013): hypothesis h = (R1,t) (R2,t) (R1,-t) (R2,-t)
static __device__ void tv_motion_F(const float* K, const float* F21, int h, float* R, float* t) {
    const float Kt[9] = {K[0], K[3], K[6], K[1], K[4], K[7], K[2], K[5], K[8]};
    float tmp[9], E[9], w[3], U[9], Vt[9];
    tv_gemm3(Kt, F21, tmp);   // E21 = K.t()*F21*K
    tv_gemm3(tmp, K, E);
    tv_svd3f(E, w, U, Vt);
    t[0] = U[2]; t[1] = U[5]; t[2] = U[8];   // u.col(2)
    tv_unit3(t);
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    tv_gemm3(U, (h & 1) ? Wt : W, tmp);
    tv_gemm3(tmp, Vt, R);
    if (tv_det3(R) < 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = -R[i];
    }
    if (h & 2) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
}

// ReconstructH's motions (:668-770, Faugeras): false = the early return of :681
static __device__ bool tv_motion_H(const float* K, const float* H21, int h, float* R, float* t) {
    float invK[9], tmp[9], A[9], w[3], U[9], Vt[9];
    tv_inv3(K, invK);
    tv_gemm3(invK, H21, tmp);   // A = invK*H21*K
    tv_gemm3(tmp, K, A);
    tv_svd3f(A, w, U, Vt);
    const float s = (float)(tv_det3(U) * tv_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const int i = h & 3;
    const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
    const bool plus = i == 0 || i == 3;   // stheta[] / sphi[] = {a, -a, -a, a}
    float Rp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, tp[3], scale;
    if (h < 4) {   // case d' = d2
        const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        const float st = plus ? aux_stheta : -aux_stheta;
        Rp[0] = ctheta; Rp[2] = -st; Rp[4] = 1.f; Rp[6] = st; Rp[8] = ctheta;
        tp[0] = x1; tp[1] = 0.f; tp[2] = -x3;
        scale = d1 - d3;
    } else {       // case d' = -d2
        const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        const float sp = plus ? aux_sphi : -aux_sphi;
        Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.f; Rp[6] = sp; Rp[8] = -cphi;
        tp[0] = x1; tp[1] = 0.f; tp[2] = x3;
        scale = d1 + d3;
    }
    // R = s*U*Rp*Vt: s*U*Rp is one gemm with alpha = s, then the product with Vt
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += (double)U[r * 3 + k] * (double)Rp[k * 3 + c];
            tmp[r * 3 + c] = (float)((double)s * acc);
        }
    tv_gemm3(tmp, Vt, R);
#pragma unroll
    for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * (double)scale);   // tp*=d1-d3
#pragma unroll
    for (int r = 0; r < 3; r++) {   // t = U*tp
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) acc += (double)U[r * 3 + k] * (double)tp[k];
        t[r] = (float)acc;
    }
    tv_unit3(t);
    return true;
}

// The body of CheckRT's loop for one inlier match (:919-977).  M = R[9] t[3] P2[12] O2[3].  0: rejected, 1: counted and written, 3: and flagged.
static __device__ __forceinline__ int tv_check_point(const float fx, const float fy, const float cx, const float cy, const float* M, const float th2,
                                                     const float u1, const float v1, const float u2, const float v2, float* X, float* cosOut) {
    const float* R = M;
    const float* t = M + 9;
    const float* P2 = M + 12;
    const float* O2 = M + 24;
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};   // K[I|0]
    float A[16], v4[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {   // Triangulate (:818-831)
        A[c] = u1 * P1[8 + c] - P1[c];
        A[4 + c] = v1 * P1[8 + c] - P1[4 + c];
        A[8 + c] = u2 * P2[8 + c] - P2[c];
        A[12 + c] = v2 * P2[8 + c] - P2[4 + c];
    }
    null_vector4_unrolled(A, v4);
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = v4[i] / v4[3];
    if (!tv_finite(X[0]) || !tv_finite(X[1]) || !tv_finite(X[2])) return 0;
    float n2[3];
    double q1 = 0.0, q2 = 0.0, dot = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) { n2[i] = X[i] - O2[i]; q1 += (double)X[i] * (double)X[i]; q2 += (double)n2[i] * (double)n2[i]; dot += (double)X[i] * (double)n2[i]; }
    const float dist1 = (float)sqrt(q1), dist2 = (float)sqrt(q2);
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    const bool low = (double)cosParallax < 0.99998;
    if (X[2] <= 0 && low) return 0;
    float X2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {   // R*p3dC1+t: one gemm
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) acc += (double)R[r * 3 + k] * (double)X[k];
        X2[r] = (float)(acc + (double)t[r]);
    }
    if (X2[2] <= 0 && low) return 0;
    const float invZ1 = (float)(1.0 / (double)X[2]);
    const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;
    const float invZ2 = (float)(1.0 / (double)X2[2]);
    const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;
    *cosOut = cosParallax;
    return low ? 3 : 1;
}

static __device__ __forceinline__ unsigned tv_ordered(float f) {   // float bits -> integers in the floats' order
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

static __global__ __launch_bounds__(TV_REC_WG) void k_tvr_reconstruct(TvArgs A) {
    __shared__ float s_S[2];
    __shared__ int s_best[2], s_model, s_ninl, s_valid, s_win;
    __shared__ float s_M[8][TV_MOTION];
    __shared__ int s_ngood[8], s_nan[8];
    __shared__ float s_par[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cap_k = A.cap_k;
    const orbm_tvr_problem* P = A.prob + b;
    const int N = A.w.n[b];
    const int its = N < 8 ? 0 : tv_its(P, A.cap_its);
    float* p3d = A.p3d + (size_t)b * cap_k * 3;
    uint8_t* tri = A.triangulated + (size_t)b * cap_k;
    for (int i = tid; i < cap_k; i += TV_REC_WG) { p3d[i * 3] = 0.f; p3d[i * 3 + 1] = 0.f; p3d[i * 3 + 2] = 0.f; tri[i] = 0; }
    // ---- the pick (:221-249, :277-299, :154-161), by wave 0
    if (wv == 0) {
        float S[2];
        int best[2];
        for (int model = 0; model < 2; model++) {
            // `currentScore>score` from score = 0 in iteration order keeps the first strictly greatest positive score: the greatest
            // (score bits, -index) key; a NaN score compares false and never enters
            const float* sc = A.score + ((size_t)b * 2 + model) * A.cap_its;
            unsigned long long key = 0ull;
            for (int h = lane; h < its; h += 64) {
                const float s = sc[h];
                if (s > 0.f) {
                    const unsigned long long k = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
                    if (k > key) key = k;
                }
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long o = __shfl_xor(key, d, 64);
                if (o > key) key = o;
            }
            S[model] = __uint_as_float((unsigned)(key >> 32));
            best[model] = key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : -1;
        }
        int model = -1;
        if (!(S[0] + S[1] == 0.f)) {   // :154
            const float RH = S[0] / (S[0] + S[1]);
            model = RH > 0.50 ? 0 : 1;
        }
        int count = 0;
        if (model >= 0 && best[model] >= 0) {
            const unsigned long long* mask = A.mask + (((size_t)b * 2 + model) * A.cap_its + best[model]) * A.words;
            for (int w = lane; w < (N + 63) >> 6; w += 64) count += __popcll(mask[w]);
        }
        for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d, 64);
        if (lane == 0) { s_S[0] = S[0]; s_S[1] = S[1]; s_best[0] = best[0]; s_best[1] = best[1]; s_model = model; s_ninl = count; s_valid = 1; s_win = -1; }
    }
    __syncthreads();
    const int model = s_model;
    orbm_tvr_result r = {};
    r.SH = s_S[0]; r.SF = s_S[1]; r.best_it_H = s_best[0]; r.best_it_F = s_best[1];
    r.n_matches = N; r.n_inliers = s_ninl; r.model = model; r.hypothesis = -1;
    r.status = A.w.status[b];
    if (model < 0 || s_best[model] < 0) {   // Reconstruct returns false at :154 (uniform in the workgroup)
        if (tid == 0) A.result[b] = r;
        return;
    }
    const size_t hm = ((size_t)b * 2 + model) * A.cap_its + s_best[model];
    const unsigned long long* mask = A.mask + hm * A.words;
    const float fx = P->fx, fy = P->fy, cx = P->cx, cy = P->cy;
    const int nh = model == 0 ? 8 : 4;
    // ---- the motion hypotheses, one lane each
    if (tid < nh) {
        const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
        float Mx[9], R[9], t[3];
        for (int k = 0; k < 9; k++) Mx[k] = A.model[hm * 9 + k];
        bool valid = true;
        if (model == 0) valid = tv_motion_H(K, Mx, tid, R, t);
        else tv_motion_F(K, Mx, tid, R, t);
        if (!valid) { if (tid == 0) s_valid = 0; }   // (the same test in every lane)
        else {
            float* M = s_M[tid];
            for (int k = 0; k < 9; k++) M[k] = R[k];
            for (int k = 0; k < 3; k++) M[9 + k] = t[k];
            for (int i = 0; i < 3; i++) {
                for (int c = 0; c < 4; c++) {   // P2 = K*[R|t]
                    double acc = 0.0;
                    for (int k = 0; k < 3; k++) acc += (double)K[i * 3 + k] * (double)(c < 3 ? R[k * 3 + c] : t[k]);
                    M[12 + i * 4 + c] = (float)acc;
                }
                double acc = 0.0;   // O2 = -R.t()*t: alpha = -1
                for (int k = 0; k < 3; k++) acc += (double)R[k * 3 + i] * (double)t[k];
                M[24 + i] = (float)(-1.0 * acc);
            }
        }
    }
    __syncthreads();
    if (!s_valid) {   // ReconstructH's early return (:681)
        if (tid == 0) A.result[b] = r;
        return;
    }
    const float* pl = A.w.planes + (size_t)b * TV_PLANES * cap_k;
    const float sigma = P->sigma;
    const float th2 = (float)(4.0 * (double)(sigma * sigma));   // 4.0*mSigma2
    // ---- CheckRT of every hypothesis (:882-991): wave = hypothesis, one match per lane in chunks of 64
    float* cosv = A.w.cosv + ((size_t)b * 8 + wv) * cap_k;
    int nGood = 0, ncos = 0, sawNan = 0;
    if (wv < nh) {
        float M[TV_MOTION];
        for (int k = 0; k < TV_MOTION; k++) M[k] = s_M[wv][k];
        for (int c0 = 0; c0 < N; c0 += 64) {
            const int i = c0 + lane;
            int res = 0;
            float X[3], c = 0.f;
            if (i < N && ((mask[i >> 6] >> lane) & 1ull)) res = tv_check_point(fx, fy, cx, cy, M, th2, pl[i], pl[cap_k + i], pl[(size_t)2 * cap_k + i], pl[(size_t)3 * cap_k + i], X, &c);
            const bool num = res != 0 && c == c;   // a NaN cosine is counted, not listed
            const unsigned long long mA = __ballot(res != 0), mV = __ballot(num);
            if (num) cosv[ncos + __popcll(mV & ((1ull << lane) - 1ull))] = c;
            nGood += __popcll(mA);
            ncos += __popcll(mV);
            sawNan |= mA != mV;
        }
    }
    __syncthreads();   // the cosines a wave wrote are read back by its other lanes
    if (wv < nh) {
        float par = 0.f;
        if (nGood > 0 && ncos > 0) {
            // sort(vCosParallax); idx = min(50, size - 1): the idx-th smallest by a bitwise radix select over the ordered bit patterns
            const int k = ncos - 1 < 50 ? ncos - 1 : 50;
            unsigned ans = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const unsigned cand = ans | (1u << bit);
                int cnt = 0;
                for (int c0 = 0; c0 < ncos; c0 += 64) cnt += __popcll(__ballot(c0 + lane < ncos && tv_ordered(cosv[c0 + lane]) < cand));
                if (cnt <= k) ans = cand;
            }
            const float c = __uint_as_float((ans & 0x80000000u) ? (ans & 0x7fffffffu) : ~ans);
            par = (float)(acos((double)c) * 180.0 / 3.1415926535897932384626433832795);   // acos(.)*180/CV_PI
        }
        if (lane == 0) { s_ngood[wv] = nGood; s_par[wv] = par; s_nan[wv] = sawNan; }
    }
    __syncthreads();
    // ---- the accept logic (:584-654, :773-815)
    if (tid == 0) {
        const int Ninl = s_ninl;
        int nan = 0;
        for (int h = 0; h < nh; h++) nan |= s_nan[h];
        if (nan) r.status |= ORBM_TVR_NAN_PARALLAX;
        int ok = 0, win = -1;
        if (model == 1) {
            int maxGood = s_ngood[0];
            for (int h = 1; h < 4; h++) maxGood = s_ngood[h] > maxGood ? s_ngood[h] : maxGood;
            const int n09 = (int)(0.9 * Ninl);
            const int nMinGood = n09 > P->min_triangulated ? n09 : P->min_triangulated;
            int nsimilar = 0;
            for (int h = 0; h < 4; h++) nsimilar += (double)s_ngood[h] > 0.7 * maxGood;
            for (int h = 3; h >= 0; h--) if (s_ngood[h] == maxGood) win = h;   // the if / else-if chain takes the first
            ok = !(maxGood < nMinGood || nsimilar > 1) && s_par[win] > P->min_parallax;
            r.n_good = maxGood; r.parallax = s_par[win];
        } else {
            int bestGood = 0, secondBestGood = 0;
            float bestParallax = -1.f;
            for (int h = 0; h < 8; h++) {
                const int g = s_ngood[h];
                if (g > bestGood) { secondBestGood = bestGood; bestGood = g; win = h; bestParallax = s_par[h]; }
                else if (g > secondBestGood) secondBestGood = g;
            }
            ok = (double)secondBestGood < 0.75 * bestGood && bestParallax >= P->min_parallax && bestGood > P->min_triangulated && (double)bestGood > 0.9 * Ninl;
            r.n_good = bestGood; r.parallax = bestParallax;
        }
        if (nan) ok = 0;
        r.hypothesis = win; r.ok = ok;
        if (ok) {
            for (int k = 0; k < 9; k++) r.R21[k] = s_M[win][k];
            for (int k = 0; k < 3; k++) r.t21[k] = s_M[win][9 + k];
            s_win = win;
        }
        A.result[b] = r;
    }
    __syncthreads();
    const int win = s_win;
    if (win < 0) return;
    // ---- vP3D / vbTriangulated of the winner: its CheckRT once more, the chunks spread over the waves
    {
        float M[TV_MOTION];
        for (int k = 0; k < TV_MOTION; k++) M[k] = s_M[win][k];
        const int32_t* i1 = A.w.i1 + (size_t)b * cap_k;
        for (int i = tid; i < N; i += TV_REC_WG) {
            if (!((mask[i >> 6] >> (i & 63)) & 1ull)) continue;
            float X[3], c;
            const int res = tv_check_point(fx, fy, cx, cy, M, th2, pl[i], pl[cap_k + i], pl[(size_t)2 * cap_k + i], pl[(size_t)3 * cap_k + i], X, &c);
            if (res) {
                const int k1 = i1[i];
                p3d[k1 * 3] = X[0]; p3d[k1 * 3 + 1] = X[1]; p3d[k1 * 3 + 2] = X[2];
                tri[k1] = res == 3;
            }
        }
    }
}

extern "C" size_t orbm_two_view_workspace_bytes(int batch, int cap_k, int cap_its) {
    if (batch < 0 || cap_k < 0 || cap_its < 0) return 0;
    size_t bytes = 0;
    tv_layout(nullptr, batch, cap_k, cap_its, &bytes);
    return bytes ? bytes : 256;
}

extern "C" int orbm_two_view_reconstruct(const orbm_tvr_problem* d_problems, const orb_keypoint* d_keys1, const orb_keypoint* d_keys2, int cap_k,
                                         const int32_t* d_matches12, const int32_t* d_sets, int cap_its, int batch, float* d_score, float* d_model,
                                         uint64_t* d_mask, orbm_tvr_result* d_result, float* d_p3d, uint8_t* d_triangulated, void* d_work,
                                         void* stream) {
    if (!d_problems || !d_keys1 || !d_keys2 || !d_matches12 || !d_sets || !d_score || !d_model || !d_mask || !d_result || !d_p3d || !d_triangulated ||
        !d_work)
        return ORB_E_INVALID;
    if (cap_k < 1 || cap_its < 1 || batch < 0) return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    if (batch > 65535) return ORB_E_CAPACITY;   // the problems are the grid's z
    const int rc = orb_lds_optin((const void*)k_tvr_models, TV_MODEL_LDS);
    if (rc != ORB_OK) return rc;
    TvArgs A;
    size_t bytes = 0;
    A.prob = d_problems; A.keys1 = d_keys1; A.keys2 = d_keys2; A.cap_k = cap_k; A.matches12 = d_matches12; A.sets = d_sets; A.cap_its = cap_its;
    A.score = d_score; A.model = d_model; A.mask = (unsigned long long*)d_mask; A.words = (cap_k + 63) / 64; A.result = d_result;
    A.p3d = d_p3d; A.triangulated = d_triangulated;
    A.w = tv_layout(d_work, batch, cap_k, cap_its, &bytes);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((cap_its + TV_LANES - 1) / TV_LANES, 2, batch);
    hipLaunchKernelGGL(k_tvr_prepare, dim3(batch), dim3(TV_PREP_WG), 0, s, A);
    hipLaunchKernelGGL(k_tvr_models, grid, dim3(TV_LANES), TV_MODEL_LDS, s, A);
    hipLaunchKernelGGL(k_tvr_score, grid, dim3(TV_LANES), 0, s, A);
    hipLaunchKernelGGL(k_tvr_reconstruct, dim3(batch), dim3(TV_REC_WG), 0, s, A);
    return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP;
}

// ---- debug exports for the tests of svd3 and the 9-column null vector (not part of the ABI): one lane, device pointers
static __global__ void k_tvr_debug_svd3(const float* A, double* out) {   // out: w[3], U[9], Vt[9]
    if (threadIdx.x == 0) tv_svd3(A, out, out + 3, out + 12);
}
static __global__ __launch_bounds__(TV_LANES) void k_tvr_debug_null9(const float* A, int rows, float* v9) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    double* M = (double*)orb_smem + threadIdx.x;
    double* V = M + 81 * TV_LANES;
    if (threadIdx.x != 0) return;
    tv_null9_init(M, V);
    for (int r = 0; r < rows; r++) tv_null9_row(M, A + r * 9);
    float v[9];
    tv_null9_solve(M, V, v);
    for (int k = 0; k < 9; k++) v9[k] = v[k];
}
extern "C" int tvr_debug_svd3(const float* d_A, double* d_out, void* stream) {
    hipLaunchKernelGGL(k_tvr_debug_svd3, dim3(1), dim3(64), 0, (hipStream_t)stream, d_A, d_out);
    return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP;
}
extern "C" int tvr_debug_null9(const float* d_A, int rows, float* d_v9, void* stream) {
    const int rc = orb_lds_optin((const void*)k_tvr_debug_null9, TV_MODEL_LDS);
    if (rc != ORB_OK) return rc;
    hipLaunchKernelGGL(k_tvr_debug_null9, dim3(1), dim3(TV_LANES), TV_MODEL_LDS, (hipStream_t)stream, d_A, rows, d_v9);
    return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP;
}
