// proj_arith.inc — the cv::Mat arithmetic of a map-point projection as the map-point projection (orbm_project.hip) and the fusion in the
// neighbours (orbm_fuse_neighbors.hip) share it (DESIGN.md "Map-point projection"): written once, so that both round alike.
#ifndef ORB_PROJ_ARITH_INC
#define ORB_PROJ_ARITH_INC

// one row of cv::Mat R*X (3x3 float times 3x1 float): products summed in double from 0, rounded to float once
static __device__ __forceinline__ float mat_row(const float* R, float x, float y, float z) {
    double s = 0.0;
    s += (double)R[0] * (double)x;
    s += (double)R[1] * (double)y;
    s += (double)R[2] * (double)z;
    return (float)s;
}
// cv::Mat::dot of two 3-vectors: double sum from 0
static __device__ __forceinline__ double dot3(float ax, float ay, float az, float bx, float by, float bz) {
    double s = 0.0;
    s += (double)ax * (double)bx;
    s += (double)ay * (double)by;
    s += (double)az * (double)bz;
    return s;
}

// MapPoint::PredictScale: the number of level thresholds <= ratio.  NaN, non-positive and +inf ratios give 0, as the reference's int conversion
// of ceil(log(ratio) / mfLogScaleFactor) does on x86 (NaN / -inf / +inf -> INT_MIN, clamped to 0).  P: a params struct with nlevels and
// level_thresholds[16] (orbm_project_params, orbm_fusenb_params).
template <class Params> static __device__ __forceinline__ int predict_scale(float ratio, const Params& P) {
    if (!(ratio <= 3.40282347e38f)) return 0;
    int l = 0;
    for (int k = 0; k < 15; k++)
        if (k < P.nlevels - 1 && ratio >= P.level_thresholds[k]) l++;
    return l;
}
#endif
