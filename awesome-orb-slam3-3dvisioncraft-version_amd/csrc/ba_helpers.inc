// ba_helpers.inc — what the two bundle adjustments (lba_build.hip, liba_inertial.hip) share: the camera models and the fixed-order workgroup sum.

// ---- cameras: GeometricCamera::project / projectJac on (model, parameters p[8]) ----
static __device__ __forceinline__ void cam_project(const int model, const double* p, const double* v, double* res) {
    if (model == LBA_CAM_PINHOLE) {  // Pinhole.cpp:43-49
        res[0] = p[0] * v[0] / v[2] + p[2];
        res[1] = p[1] * v[1] / v[2] + p[3];
    } else {
        // KannalaBrandt8.cpp:52-66 rounds theta and psi through atan2f/sqrtf; reproduced as float(atan2(double)) — a
        // correctly rounded float result, which is what glibc's atan2f returns in all but rare double-rounding cases
        // (within 1 float ulp of it: DESIGN.md section 2).
        const double x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
        const float rf = sqrtf((float)x2_plus_y2);
        const double theta = (double)(float)atan2((double)rf, (double)(float)v[2]);
        const double psi = (double)(float)atan2((double)(float)v[1], (double)(float)v[0]);
        const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2,
                     theta9 = theta7 * theta2;
        const double r = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
        res[0] = p[0] * r * cos(psi) + p[2];
        res[1] = p[1] * r * sin(psi) + p[3];
    }
}
static __device__ __forceinline__ void cam_project_jac(const int model, const double* p, const double* v, double* J) {
    if (model == LBA_CAM_PINHOLE) {  // Pinhole.cpp:89-100
        J[0] = p[0] / v[2]; J[1] = 0; J[2] = -p[0] * v[0] / (v[2] * v[2]);
        J[3] = 0; J[4] = p[1] / v[2]; J[5] = -p[1] * v[1] / (v[2] * v[2]);
    } else {  // KannalaBrandt8.cpp:166-196
        const double x2 = v[0] * v[0], y2 = v[1] * v[1], z2 = v[2] * v[2];
        const double r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
        const double theta = atan2(r, v[2]);
        const double theta2 = theta * theta, theta3 = theta2 * theta, theta4 = theta2 * theta2, theta5 = theta4 * theta,
                     theta6 = theta2 * theta4, theta7 = theta6 * theta, theta8 = theta4 * theta4, theta9 = theta8 * theta;
        const double f = theta + theta3 * p[4] + theta5 * p[5] + theta7 * p[6] + theta9 * p[7];
        const double fd = 1 + 3 * p[4] * theta2 + 5 * p[5] * theta4 + 7 * p[6] * theta6 + 9 * p[7] * theta8;
        J[0] = p[0] * (fd * v[2] * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
        J[3] = p[1] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
        J[1] = p[0] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
        J[4] = p[1] * (fd * v[2] * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
        J[2] = -p[0] * fd * v[0] / (r2 + z2);
        J[5] = -p[1] * fd * v[1] / (r2 + z2);
    }
}

// sum of NV doubles per thread over a workgroup of T threads, result broadcast to every thread; fixed order (butterfly inside a wave, then the
// waves 0 .. T / 64 - 1 through scratch[T / 64][NV])
template <int NV, int T>
static __device__ __forceinline__ void block_sum(double (&v)[NV], double* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if (T > 64) {
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NV; k++) scratch[wave * NV + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NV; k++) {
            double t = scratch[k];
#pragma unroll
            for (int w = 1; w < T / 64; w++) t += scratch[w * NV + k];
            v[k] = t;
        }
    }
}
