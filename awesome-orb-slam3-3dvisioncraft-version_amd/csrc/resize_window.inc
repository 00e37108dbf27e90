// resize_window.inc — the source window of one k_resize2 lane (orbx_extractor.hip), written once so that the host can check what the kernel takes
// on trust (tests/cpp/resize_window_test.cpp sweeps it over image sizes, scale factors and level counts).
//
// A lane owns four adjacent destination columns.  Their eight taps (source columns c[j] and c[j] + 1) lie, for scale factors <= 1.3, inside the
// eight bytes that start at c[0]: c[3] - c[0] <= 4.  Those bytes are cut out of three aligned dwords of the source row — dwords (c[0] >> 2) + 0, 1, 2 —
// by two v_alignbyte with the byte phase c[0] & 3; column j's byte pair is then picked by v_perm with selector sel[j].
// A load may touch only dwords that hold at least one pixel of the row (level 0 is the caller's buffer: its last row may end the allocation, and a
// pyramid plane whose width is a multiple of 64 has no padding either), so the three indices are clamped to the row's last dword, (sw - 1) >> 2.  A
// byte that comes from a clamped dword lies past column sw - 1, and only a tap of weight 0 names such a column (cv::resize clamps the index and
// forces the fraction to 0 there: resize_coef).
#ifndef ORB_RESIZE_WINDOW_INC
#define ORB_RESIZE_WINDOW_INC
#include <cmath>
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define __forceinline__ inline
#endif

// cv::resize coefficient of one destination coordinate (SURVEY.md Appendix B2), with the same IEEE double/float operations as OpenCV's table
// setup: source index + the two 11-bit weights.  k_resize evaluates it in the kernel, orbx_create tabulates it per level for k_resize2.
static __host__ __device__ __forceinline__ void resize_coef(int d, double scale, int slen, bool clampIndex, int& s0, int& w0, int& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int si = (int)floorf(f);
    f -= (float)si;
    if (clampIndex) {   // x: OpenCV clamps index and weight (resize.cpp alpha table); y keeps the weight and clips rows later
        if (si < 0) { f = 0.f; si = 0; }
        if (si >= slen - 1) { f = 0.f; si = slen - 1; }
    }
    s0 = si;
    w0 = (int)rintf((1.f - f) * 2048.f);   // cvRound: round half to even (default rounding mode)
    w1 = (int)rintf(f * 2048.f);
    w0 = w0 < -32768 ? -32768 : (w0 > 32767 ? 32767 : w0);
    w1 = w1 < -32768 ? -32768 : (w1 > 32767 ? 32767 : w1);
}

struct Resize2Window {
    uint32_t dword[3];   // aligned dword indices into the source row, each <= (sw - 1) >> 2
    uint32_t phase;      // c[0] & 3: the byte shift of both v_alignbyte
    uint32_t sel[4];     // v_perm selectors: bytes (c[j] - c[0], c[j] - c[0] + 1) of the window -> the low bytes of the two 16-bit halves
};
// c: the clamped source columns (resize_coef, clampIndex) of the lane's four destination columns, 0 <= c[0] <= ... <= c[3] <= sw - 1
static __host__ __device__ __forceinline__ Resize2Window resize2_window(const int c[4], const int sw) {
    Resize2Window w;
    const uint32_t first = (uint32_t)c[0] >> 2, last = (uint32_t)(sw - 1) >> 2;
    for (int k = 0; k < 3; k++) w.dword[k] = first + (uint32_t)k < last ? first + (uint32_t)k : last;
    w.phase = (uint32_t)c[0] & 3u;
    for (int j = 0; j < 4; j++) {
        const uint32_t off = (uint32_t)(c[j] - c[0]);   // 0..4 for scale <= 1.3
        w.sel[j] = off | ((off + 1u) << 16) | 0x0c000c00u;
    }
    return w;
}
#endif
