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

// ---- the wave-uniform values of k_resize2, tabulated once per level (orbx_create) ---------------------------------------------------------------------
// Everything a k_resize2 wave derived from (level, destination row) or (level, strip) with scalar instructions — clips, weight shifts, the strip's
// division into (row, column), its first and last source row — is the same for every frame of every call.  The host writes it down; the kernel reads
// one strip record at its head and one row record per destination row (tests/cpp/resize_rows_test.cpp checks both against resize_coef).
struct Resize2Row {      // 16 bytes, one scalar load
    int e1;              // the row's second source row, clipped to [0, sh - 1]: it is emitted when that row has been filtered (-1: the strip's end mark)
    int flags;           // bit 0: the clipped first source row is the same row (the level's first / last rows) — its H result is used twice;
                         // bit 1: the strip's next row has the same e1 (it is emitted behind this one, without another look at a record)
    uint32_t b0, b1;     // the two 11-bit weights << 12 (the V pass multiplies by them with v_mul_hi_u32_u24)
};
struct Resize2Strip {    // 32 bytes, one scalar load
    int y0, y1;          // destination rows [y0, y1)
    int rlo, rhi;        // source rows [rlo, rhi], every one of them read by some row of the strip: a wave loads no other row
    int col;             // strip column: destination columns [256 * col, 256 * col + 256)
    int rounds;          // rounds of `depth` source rows whose prefetched successors (the rows `depth` further on) all lie inside the strip
    int rec;             // index of the strip's first row record: the records of a strip row are stripRows + 1 consecutive entries, end mark last
    int last;            // 1: the level's last strip column (the only one that can hold lanes past dw or a lane with fewer than four columns)
};
// ys / yw: the level's row tables (resize_coef without clampIndex, yw = w0 & 0xFFFF | w1 << 16); rows: stripsY * (stripRows + 1) records, strips:
// stripsY * stripsX records (x fastest, the order of the kernel's strip numbers).  depth: the kernel's rows in flight (R2_D).
template <class RowVec, class StripVec>
static inline void resize2_records(const int* ys, const int* yw, const int dh, const int sh, const int stripsX, const int stripRows, const int depth,
                                   RowVec& rows, StripVec& strips) {
    auto clip = [&](const int r) { return r < 0 ? 0 : (r < sh ? r : sh - 1); };   // rows are clipped after the weights are fixed (resize.cpp)
    const int stripsY = (dh + stripRows - 1) / stripRows;
    for (int s = 0; s < stripsY; s++) {
        const int y0 = s * stripRows, y1 = y0 + stripRows < dh ? y0 + stripRows : dh;
        const int rec = (int)rows.size();
        for (int y = y0; y < y0 + stripRows + 1; y++) {
            Resize2Row r = {-1, 0, 0u, 0u};
            if (y < y1) {
                r.e1 = clip(ys[y] + 1);
                r.flags = (clip(ys[y]) == r.e1 ? 1 : 0) | (y + 1 < y1 && clip(ys[y + 1] + 1) == r.e1 ? 2 : 0);
                r.b0 = ((uint32_t)yw[y] & 0xFFFFu) << 12;
                r.b1 = ((uint32_t)yw[y] >> 16) << 12;
            }
            rows.push_back(r);
        }
        const int rlo = clip(ys[y0]), rhi = clip(ys[y1 - 1] + 1), n = rhi - rlo + 1;
        for (int c = 0; c < stripsX; c++) {
            const Resize2Strip t = {y0, y1, rlo, rhi, c, n >= depth ? n / depth - 1 : 0, rec, c == stripsX - 1 ? 1 : 0};
            strips.push_back(t);
        }
    }
}
#endif
