// sim3_solver.hip — Sim3Solver on gfx950: the RANSAC Horn alignment of the loop / merge chain (reference src/Sim3Solver.cc; include/orbhip.h
// "Sim3Solver"), for a batch of independent problems.
//
//   k_sim3_solve   one workgroup per problem, four phases separated by workgroup barriers:
//     0  the constructor (:106-121): every correspondence's camera points mvX3Dc1 / mvX3Dc2 and their images mvP1im1 / mvP2im2, one thread
//        per correspondence, staged once in dynamic LDS as twelve planes of cap_n floats (lane i reads word i of a plane: no bank conflict);
//     1  ComputeSim3 (:316-427), one thread per hypothesis: mR12i / mt12i / ms12i to d_hyp, mT12i / mT21i to the workspace;
//     2  CheckInliers (:430-454), one wave per hypothesis, one correspondence per lane: the flags are a ballot (= the mask word), the count
//        its popcount;
//     3  the reference's serial pick (:170-218) by wave 0: the stop is the first count above min_inliers (ballot + ffs per 64 counts), the
//        best of the iterations before it the greatest (count, index) key, i.e. the LAST of the hypotheses tied at the best count, as the
//        reference's `>=` leaves it; then vbInliers is scattered through index1.
// Nothing couples two hypotheses before phase 3, and phase 3 is integer work: results do not depend on any execution order.
//
// Arithmetic: rules R4 and R5 of DESIGN.md section 2.  A float cv::Mat product is the double sum of the double products, from 0 in k order, times
// alpha, plus beta * C, rounded to float once (cv::gemm; `A * B + C` and `C - s * A * B` are ONE gemm); Mat * scalar and Mat / scalar multiply each
// element by the double alpha (1 / s for a division) and round once; Mat::dot and cv::norm accumulate in double; cv::reduce(SUM) of three floats is
// (a0 + a2) + a1 in float; cv::eigen is JacobiImpl_<float>; cv::Rodrigues works in double.  Expressions on M.at<float>() are float expressions.
// The library is built with -ffp-contract=off and correctly rounded fp32 division / sqrt.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/orbhip.h"
#include "lds_optin.inc"
#include "kb8_geom.inc"

static constexpr int S3_THREADS = 512;   // 8 waves: 512 hypotheses of phase 1 at once, 8 hypotheses of phase 2 at a time
static constexpr int S3_PLANES = 12;     // X3Dc1 xyz, X3Dc2 xyz, P1im1 uv, P2im2 uv, max_err1, max_err2
static_assert((size_t)ORBM_SIM3_MAX_N * S3_PLANES * 4 + 64 <= ORB_LDS_CU_BYTES, "the staged correspondences fit the CU's LDS");

constexpr int S3_WORK_FLOATS = 24;   // the workspace row of a hypothesis: the 24 floats of T (ComputeSim3 below)

struct Sim3Args {
    const orbm_sim3_problem* prob;
    const orbm_sim3_corr* corr;
    const int32_t* n;
    int cap_n;
    const int32_t* samples;
    int cap_its;
    orbm_sim3_hyp* hyp;
    int32_t* hyp_count;
    unsigned long long* hyp_mask;
    int words;
    orbm_sim3_result* result;
    uint8_t* inliers;
    int cap_n1;
    float* work;   // [batch][cap_its][S3_WORK_FLOATS]: mT12i rows 0-2 (sR | t12), mT21i rows 0-2 (sRinv | tinv)
};

// cv::gemm row: (float)(alpha * sum_k a[k] * b[k] + c), everything in double
static __device__ __forceinline__ double s3_dot3(const float* a, int sa, const float* b, int sb) {
    double acc = 0.0;
    acc += (double)a[0] * (double)b[0];
    acc += (double)a[sa] * (double)b[sb];
    acc += (double)a[2 * sa] * (double)b[2 * sb];
    return acc;
}

static __device__ void s3_project(const orbm_sim3_camera& cam, const float* X, float* uv) {
    if (cam.model == ORBM_SIM3_CAM_KB8) {
        kb8_project_f(cam.p, X, uv);
    } else {   // Pinhole.cpp:27-33
        uv[0] = cam.p[0] * X[0] / X[2] + cam.p[2];
        uv[1] = cam.p[1] * X[1] / X[2] + cam.p[3];
    }
}

// cv::hypot of OpenCV's Jacobi (lapack.cpp)
static __device__ __forceinline__ float s3_hypot(float a, float b) {
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}

// cv::eigen of a symmetric 4x4 CV_32F matrix = JacobiImpl_<float> (rule R5): A is destroyed, W = eigenvalues descending, row k of V the k-th
// eigenvector.  At most n*n*30 rotations; NaN input ends there (every comparison is false, the indices stay in range).
static __device__ void s3_jacobi4(float* A, float* W, float* V) {
    const int n = 4;
    const float eps = FLT_EPSILON;
    int indR[4], indC[4];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.f : 0.f;
    auto row_max = [&](int k) {
        int m = k + 1;
        float mv = fabsf(A[n * k + m]);
        for (int i = k + 2; i < n; i++) { const float val = fabsf(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
        indR[k] = m;
    };
    auto col_max = [&](int k) {
        int m = 0;
        float mv = fabsf(A[k]);
        for (int i = 1; i < k; i++) { const float val = fabsf(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
        indC[k] = m;
    };
    for (int k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) row_max(k);
        if (k > 0) col_max(k);
    }
    for (int iters = 0; iters < n * n * 30; iters++) {
        int k = 0;
        float mv = fabsf(A[indR[0]]);
        for (int i = 1; i < n - 1; i++) { const float val = fabsf(A[n * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
        int l = indR[k];
        for (int i = 1; i < n; i++) { const float val = fabsf(A[n * indC[i] + i]); if (mv < val) { mv = val; k = indC[i]; l = i; } }
        const float p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        const float y = (W[l] - W[k]) * 0.5f;
        float t = fabsf(y) + s3_hypot(p, y);
        float s = s3_hypot(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        A[n * k + l] = 0;
        W[k] -= t;
        W[l] += t;
#define S3_ROTATE(v0, v1) do { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; } while (0)
        for (int i = 0; i < k; i++) S3_ROTATE(A[n * i + k], A[n * i + l]);
        for (int i = k + 1; i < l; i++) S3_ROTATE(A[n * k + i], A[n * i + l]);
        for (int i = l + 1; i < n; i++) S3_ROTATE(A[n * k + i], A[n * l + i]);
        for (int i = 0; i < n; i++) S3_ROTATE(V[n * k + i], V[n * l + i]);
#undef S3_ROTATE
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) row_max(idx);
            if (idx > 0) col_max(idx);
        }
    }
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            const float w = W[m]; W[m] = W[k]; W[k] = w;
            for (int i = 0; i < n; i++) { const float v = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = v; }
        }
    }
}

// cv::Rodrigues, vector -> matrix (rule R5): in double, narrowed to float
static __device__ void s3_rodrigues(const float* rv, float* R) {
    double r[3] = {(double)rv[0], (double)rv[1], (double)rv[2]};
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
    r[0] *= itheta; r[1] *= itheta; r[2] *= itheta;
    const double rx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i * 3 + j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + s * rx[i * 3 + j]);
}

// ComputeCentroid (:305-314): P is 3 x 3 row-major, column i = point i
static __device__ void s3_centroid(const float* P, float* Pr, float* C) {
    for (int r = 0; r < 3; r++) {
        const float sum = (P[r * 3] + P[r * 3 + 2]) + P[r * 3 + 1];   // cv::reduce(SUM) over a row of three
        C[r] = (float)((double)sum * (1.0 / 3.0));                      // C / P.cols
        for (int i = 0; i < 3; i++) Pr[r * 3 + i] = P[r * 3 + i] - C[r];
    }
}

// ComputeSim3 (:316-427).  T[0..12) = rows 0-2 of mT12i, T[12..24) = rows 0-2 of mT21i.
static __device__ void s3_compute(const float* P1, const float* P2, const int fix_scale, orbm_sim3_hyp& H, float* T) {
    float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i * 3 + j] = (float)s3_dot3(Pr2 + i * 3, 1, Pr1 + j * 3, 1);   // Pr2 * Pr1.t()
    const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3], N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3],
                N24 = M[6] + M[2], N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
    float A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44}, W[4], V[16];
    s3_jacobi4(A, W, V);
    double nrm2 = 0.0;
    for (int i = 1; i < 4; i++) nrm2 += (double)V[i] * (double)V[i];
    const double nrm = sqrt(nrm2);                              // norm(vec)
    const double ang = atan2(nrm, (double)V[0]);
    const double alpha = (2.0 * ang) * (1.0 / nrm);             // vec = 2*ang*vec/norm(vec)
    float rv[3];
    for (int i = 0; i < 3; i++) rv[i] = (float)((double)V[1 + i] * alpha);
    s3_rodrigues(rv, H.R12);
    const float* R = H.R12;
    float s;
    if (!fix_scale) {
        float P3[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) P3[i * 3 + j] = (float)s3_dot3(R + i * 3, 1, Pr2 + j, 3);   // mR12i * Pr2
        double nom = 0.0, den = 0.0;
        for (int i = 0; i < 9; i++) nom += (double)Pr1[i] * (double)P3[i];   // Pr1.dot(P3)
        for (int i = 0; i < 9; i++) den += (double)(P3[i] * P3[i]);          // cv::pow(P3, 2, .) in float, summed in double
        s = (float)(nom / den);
    } else {
        s = 1.0f;
    }
    H.s12 = s;
    for (int i = 0; i < 3; i++) H.t12[i] = (float)(s3_dot3(R + i * 3, 1, O2, 1) * (-(double)s) + (double)O1[i]);   // O1 - ms12i*mR12i*O2: one gemm
    const double inv = 1.0 / (double)s;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            T[i * 4 + j] = (float)((double)R[i * 3 + j] * (double)s);          // sR
            T[12 + i * 4 + j] = (float)((double)R[j * 3 + i] * inv);           // sRinv = (1.0/ms12i)*mR12i.t()
        }
        T[i * 4 + 3] = H.t12[i];
    }
    for (int i = 0; i < 3; i++) T[12 + i * 4 + 3] = (float)(s3_dot3(T + 12 + i * 4, 1, H.t12, 1) * -1.0);   // tinv = -sRinv*mt12i
}

static __global__ __launch_bounds__(S3_THREADS) void k_sim3_solve(Sim3Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    __shared__ unsigned s_status;
    float* pl = (float*)orb_smem;   // plane k of correspondence i: pl[k * cap_n + i]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwaves = blockDim.x >> 6;
    const orbm_sim3_problem* P = A.prob + b;
    const int cap_n = A.cap_n;
    unsigned status = 0;
    int N = A.n[b];
    if (N < 0) { N = 0; status |= ORBM_SIM3_N_CLAMPED; }
    if (N > cap_n) { N = cap_n; status |= ORBM_SIM3_N_CLAMPED; }
    int its = P->max_its < 0 ? 0 : P->max_its;
    if (its > A.cap_its) { its = A.cap_its; status |= ORBM_SIM3_ITS_CLAMPED; }
    const int min_inliers = P->min_inliers;
    const int n1 = P->n1 < A.cap_n1 ? P->n1 : A.cap_n1;
    const size_t h0 = (size_t)b * A.cap_its;
    if (tid == 0) s_status = 0;
    for (int i = tid; i < A.cap_n1; i += blockDim.x) A.inliers[(size_t)b * A.cap_n1 + i] = 0;   // vbInliers = vector<bool>(mN1, false)
    if (N < min_inliers) {   // :158-162 (uniform in the workgroup)
        if (tid == 0) {
            orbm_sim3_result r = {};
            r.no_more = 1;
            r.best_iter = -1;
            r.status = status;
            A.result[b] = r;
        }
        return;
    }
    // ---- phase 0: the constructor's per-correspondence work
    for (int i = tid; i < N; i += blockDim.x) {
        const orbm_sim3_corr c = A.corr[(size_t)b * cap_n + i];
        float X1[3], X2[3], uv1[2], uv2[2];
        for (int r = 0; r < 3; r++) {
            X1[r] = (float)(s3_dot3(P->Rcw1 + r * 3, 1, c.Xw1, 1) + (double)P->tcw1[r]);   // Rcw1*X3D1w+tcw1
            X2[r] = (float)(s3_dot3(P->Rcw2 + r * 3, 1, c.Xw2, 1) + (double)P->tcw2[r]);
        }
        s3_project(P->cam1, X1, uv1);
        s3_project(P->cam2, X2, uv2);
        const float v[S3_PLANES] = {X1[0], X1[1], X1[2], X2[0], X2[1], X2[2], uv1[0], uv1[1], uv2[0], uv2[1], c.max_err1, c.max_err2};
        for (int k = 0; k < S3_PLANES; k++) pl[(size_t)k * cap_n + i] = v[k];
    }
    __syncthreads();
    // ---- phase 1: one hypothesis per thread
    for (int h = tid; h < its; h += blockDim.x) {
        const int32_t* tr = A.samples + (h0 + h) * 3;
        const int i0 = tr[0], i1 = tr[1], i2 = tr[2];
        orbm_sim3_hyp H;
        float T[24];
        if (i0 < 0 || i0 >= N || i1 < 0 || i1 >= N || i2 < 0 || i2 >= N || i0 == i1 || i0 == i2 || i1 == i2) {
            const float nan = __int_as_float(0x7fc00000);
            for (int k = 0; k < 9; k++) H.R12[k] = nan;
            for (int k = 0; k < 3; k++) H.t12[k] = nan;
            H.s12 = nan;
            for (int k = 0; k < 24; k++) T[k] = nan;
            atomicOr(&s_status, ORBM_SIM3_BAD_SAMPLE);   // a flag: the order of the ORs cannot show
        } else {
            const int idx[3] = {i0, i1, i2};
            float P1[9], P2[9];
            for (int c = 0; c < 3; c++)
                for (int r = 0; r < 3; r++) {
                    P1[r * 3 + c] = pl[(size_t)r * cap_n + idx[c]];          // mvX3Dc1[idx].copyTo(P3Dc1i.col(i))
                    P2[r * 3 + c] = pl[(size_t)(3 + r) * cap_n + idx[c]];
                }
            s3_compute(P1, P2, P->fix_scale, H, T);
        }
        A.hyp[h0 + h] = H;
        float* w = A.work + (h0 + h) * S3_WORK_FLOATS;
        for (int k = 0; k < 24; k++) w[k] = T[k];
    }
    __syncthreads();
    // ---- phase 2: one hypothesis per wave, one correspondence per lane
    for (int h = wv; h < its; h += nwaves) {
        float T[24];
        const float* w = A.work + (h0 + h) * S3_WORK_FLOATS;
        for (int k = 0; k < 24; k++) T[k] = w[k];
        int count = 0;
        for (int wd = 0; wd < A.words; wd++) {
            const int i = wd * 64 + lane;
            bool ok = false;
            if (i < N) {
                float X1[3], X2[3], Y[3], uv[2];
                for (int r = 0; r < 3; r++) { X1[r] = pl[(size_t)r * cap_n + i]; X2[r] = pl[(size_t)(3 + r) * cap_n + i]; }
                for (int r = 0; r < 3; r++) Y[r] = (float)(s3_dot3(T + r * 4, 1, X2, 1) + (double)T[r * 4 + 3]);        // Project(mvX3Dc2, ., mT12i, pCamera1)
                s3_project(P->cam1, Y, uv);
                const float d1x = pl[(size_t)6 * cap_n + i] - uv[0], d1y = pl[(size_t)7 * cap_n + i] - uv[1];       // mvP1im1[i]-vP2im1[i]
                for (int r = 0; r < 3; r++) Y[r] = (float)(s3_dot3(T + 12 + r * 4, 1, X1, 1) + (double)T[12 + r * 4 + 3]);   // Project(mvX3Dc1, ., mT21i, pCamera2)
                s3_project(P->cam2, Y, uv);
                const float d2x = uv[0] - pl[(size_t)8 * cap_n + i], d2y = uv[1] - pl[(size_t)9 * cap_n + i];       // vP1im2[i]-mvP2im2[i]
                double e1 = 0.0, e2 = 0.0;
                e1 += (double)d1x * (double)d1x; e1 += (double)d1y * (double)d1y;
                e2 += (double)d2x * (double)d2x; e2 += (double)d2y * (double)d2y;
                const float err1 = (float)e1, err2 = (float)e2;
                ok = err1 < pl[(size_t)10 * cap_n + i] && err2 < pl[(size_t)11 * cap_n + i];
            }
            const unsigned long long m = __ballot(ok);
            if (lane == 0) A.hyp_mask[(h0 + h) * A.words + wd] = m;
            count += __popcll(m);
        }
        if (lane == 0) A.hyp_count[h0 + h] = count;
    }
    __syncthreads();
    // ---- phase 3: the serial pick, by wave 0
    if (wv != 0) return;
    int stop = -1;
    for (int c0 = 0; c0 < its && stop < 0; c0 += 64) {
        const int h = c0 + lane;
        const unsigned long long m = __ballot(h < its && A.hyp_count[h0 + h] > min_inliers);
        if (m) stop = c0 + __ffsll((long long)m) - 1;
    }
    const int iterations = stop >= 0 ? stop + 1 : its;
    long long key = -1;   // (count << 32) | index: the greatest key is the last of the hypotheses tied at the best count
    for (int h = lane; h < iterations; h += 64) {
        const long long k = ((long long)A.hyp_count[h0 + h] << 32) | (long long)h;
        if (k > key) key = k;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(key, d, 64);
        if (o > key) key = o;
    }
    const int best = key < 0 ? -1 : (int)(key & 0x7fffffff);
    const int converged = stop >= 0;
    if (converged) {   // vbInliers[mvnIndices1[i]] = true
        bool bad = false;
        for (int i = lane; i < N; i += 64)
            if ((A.hyp_mask[(h0 + best) * A.words + (i >> 6)] >> (i & 63)) & 1ull) {
                const int i1 = A.corr[(size_t)b * cap_n + i].index1;
                if (i1 >= 0 && i1 < n1) A.inliers[(size_t)b * A.cap_n1 + i1] = 1;
                else bad = true;
            }
        if (__ballot(bad)) status |= ORBM_SIM3_BAD_INDEX;
    }
    if (lane == 0) {
        orbm_sim3_result r = {};
        r.iterations = iterations;
        r.converged = converged;
        r.no_more = (!converged && iterations >= P->max_its) ? 1 : 0;
        r.best_iter = best;
        if (best >= 0) {
            const orbm_sim3_hyp H = A.hyp[h0 + best];
            const float* w = A.work + (h0 + best) * S3_WORK_FLOATS;
            r.n_inliers = A.hyp_count[h0 + best];
            for (int k = 0; k < 9; k++) r.R12[k] = H.R12[k];
            for (int k = 0; k < 3; k++) r.t12[k] = H.t12[k];
            r.s12 = H.s12;
            for (int k = 0; k < 12; k++) r.T12[k] = w[k];
            r.T12[15] = 1.f;
        }
        r.status = status | s_status;
        A.result[b] = r;
    }
}

extern "C" int orbm_sim3_ransac_iterations(double probability, int min_inliers, int max_its, int n) {
    const float epsilon = (float)min_inliers / n;
    int nIterations;
    if (min_inliers == n) {
        nIterations = 1;
    } else {
        const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;   // cvttsd2si's answer for NaN and out of range
    }
    const int m = nIterations < max_its ? nIterations : max_its;
    return m > 1 ? m : 1;
}

extern "C" size_t orbm_sim3_workspace_bytes(int batch, int cap_n, int cap_its) {
    (void)cap_n;
    if (batch < 0 || cap_its < 0) return 0;
    const size_t bytes = (size_t)batch * (size_t)cap_its * S3_WORK_FLOATS * sizeof(float);
    return bytes ? bytes : 256;
}

extern "C" int orbm_sim3_solve(const orbm_sim3_problem* d_problems, const orbm_sim3_corr* d_corr, const int32_t* d_n, int cap_n,
                               const int32_t* d_samples, int cap_its, int batch, orbm_sim3_hyp* d_hyp, int32_t* d_hyp_count, uint64_t* d_hyp_mask,
                               orbm_sim3_result* d_result, uint8_t* d_inliers, int cap_n1, void* d_work, void* stream) {
    if (!d_problems || !d_corr || !d_n || !d_samples || !d_hyp || !d_hyp_count || !d_hyp_mask || !d_result || !d_inliers || !d_work) return ORB_E_INVALID;
    if (cap_its < 1 || cap_n < 1 || cap_n1 < 1 || batch < 0) return ORB_E_INVALID;
    if (cap_n > ORBM_SIM3_MAX_N) return ORB_E_CAPACITY;
    if (batch == 0) return ORB_OK;
    const size_t lds = (size_t)cap_n * S3_PLANES * sizeof(float);
    const int rc = orb_lds_optin((const void*)k_sim3_solve, lds);
    if (rc != ORB_OK) return rc;
    Sim3Args A;
    A.prob = d_problems; A.corr = d_corr; A.n = d_n; A.cap_n = cap_n; A.samples = d_samples; A.cap_its = cap_its; A.hyp = d_hyp;
    A.hyp_count = d_hyp_count; A.hyp_mask = (unsigned long long*)d_hyp_mask; A.words = (cap_n + 63) / 64; A.result = d_result;
    A.inliers = d_inliers; A.cap_n1 = cap_n1; A.work = (float*)d_work;
    hipLaunchKernelGGL(k_sim3_solve, dim3(batch), dim3(S3_THREADS), lds, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP;
}
