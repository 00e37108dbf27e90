// resize_window_test.cpp — host check of the source window a k_resize2 lane loads (csrc/resize_window.inc: resize2_window, shared with the kernel).
// Stand-alone: links no library.  For 3 000 random (width, height, scale factor <= 1.3, levels) configurations — the sweep of
// test_edge_cases.py::test_emu_resize_staging_footprints_cover_their_tiles restricted to the scale factors the kernel serves — plus widths that are
// multiples of 64 (a pyramid plane without padding: the right-edge window must clamp), every level the kernel would build and every lane of it:
//   * the three dword indices lie in [0, (sw - 1) >> 2]: a load touches only dwords that hold a pixel of the row;
//   * both taps of all four columns lie inside the 8 bytes the lane cuts out of its three dwords, and the byte v_perm picks is the tap's pixel —
//     except taps of weight 0 past the row's end, which may be any byte;
// on a row whose bytes are their own column numbers, so a wrong byte is a wrong value.  The level sizes and scales are orbx_create's.
#include "../../awesome-orb-slam3-3dvisioncraft-version_amd/csrc/resize_window.inc"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static long g_bad = 0, g_lanes = 0, g_clamped = 0;

static void fail(const char* what, int W, int H, double sf, int l, int x) {
    if (g_bad++ < 10) std::fprintf(stderr, "FAIL %s: %dx%d scale factor %.6f level %d lane column %d\n", what, W, H, sf, l, x);
}

// one axis of one level: dw destination columns from sw source columns
static void check_level(int sw, int dw, int W, int H, double sf, int l) {
    const double scale = 1. / ((double)dw / sw);
    std::vector<int> xs(dw), xw(dw);
    for (int x = 0; x < dw; x++) { int s0, w0, w1; resize_coef(x, scale, sw, true, s0, w0, w1); xs[x] = s0; xw[x] = (w0 & 0xFFFF) | (w1 << 16); }
    // the row as the kernel sees it: exactly ((sw - 1) >> 2) + 1 dwords (a heap block of that size: AddressSanitizer sees a read past the last one)
    const int ndw = ((sw - 1) >> 2) + 1;
    std::vector<uint32_t> row(ndw);
    uint8_t* bytes = (uint8_t*)row.data();
    for (int i = 0; i < 4 * ndw; i++) bytes[i] = (uint8_t)(i * 7 + 3);
    const int lanes = ((dw + 255) / 256) * 64;   // every lane of every strip column, the ones past dw included
    for (int lane = 0; lane < lanes; lane++) {
        int c[4], a[4];
        for (int j = 0; j < 4; j++) { const int x = std::min(lane * 4 + j, dw - 1); c[j] = xs[x]; a[j] = xw[x]; }
        const Resize2Window w = resize2_window(c, sw);
        g_lanes++;
        uint32_t d[3];
        for (int k = 0; k < 3; k++) {
            if (w.dword[k] > (uint32_t)((sw - 1) >> 2)) { fail("dword index past the row", W, H, sf, l, lane * 4); return; }
            d[k] = row[w.dword[k]];
        }
        g_clamped += w.dword[2] != w.dword[0] + 2;
        // v_alignbyte x 2: the 8 bytes that start at byte `phase` of the three dwords
        uint8_t win[8];
        for (int i = 0; i < 8; i++) { const int b = (int)w.phase + i; win[i] = (uint8_t)(d[b >> 2] >> (8 * (b & 3))); }
        for (int j = 0; j < 4; j++) {
            const int off = c[j] - c[0];
            if (off < 0 || off + 1 > 7) { fail("tap outside the 8-byte window", W, H, sf, l, lane * 4 + j); return; }
            if (w.sel[j] != ((uint32_t)off | ((uint32_t)(off + 1) << 16) | 0x0c000c00u)) { fail("selector", W, H, sf, l, lane * 4 + j); return; }
            const int a0 = (int)(short)(a[j] & 0xFFFF), a1 = a[j] >> 16;
            if (win[off] != bytes[c[j]]) { fail("first tap's byte", W, H, sf, l, lane * 4 + j); return; }
            if (c[j] + 1 <= sw - 1) {
                if (win[off + 1] != bytes[c[j] + 1]) { fail("second tap's byte", W, H, sf, l, lane * 4 + j); return; }
            } else if (a1 != 0 || a0 != 2048) {
                fail("a tap past the row's end has a weight", W, H, sf, l, lane * 4 + j); return;
            }
        }
    }
}

static int check_config(int W, int H, double sfIn, int nl) {
    // orbx_create: scale[i] = (float)(scale[i - 1] * scaleFactor), sizes cvRound(size * (1 / scale[i])); k_resize2 serves a level if both axes scale by <= 1.3
    const double sf = (double)(float)sfIn;
    float scale = 1.0f;
    int pw = W, ph = H, served = 0;
    for (int l = 1; l < nl; l++) {
        scale = (float)(scale * sf);
        const float inv = 1.0f / scale;
        const int w = (int)lrintf((float)W * inv), h = (int)lrintf((float)H * inv);
        if (w - 32 < 30 || h - 32 < 30) break;   // (the extractor refuses levels without a FAST cell)
        if (1. / ((double)w / pw) <= 1.3 && 1. / ((double)h / ph) <= 1.3) {
            check_level(pw, w, W, H, sfIn, l);
            check_level(ph, h, W, H, sfIn, l);   // the same window arithmetic on the other axis' sizes: more widths for free
            served++;
        }
        pw = w; ph = h;
    }
    return served;
}

int main() {
    std::mt19937_64 rng(2024);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo)); };
    const double fixed[4] = {1.1, 1.2, 1.25, 1.3};
    long served = 0;
    for (int i = 0; i < 3000; i++) {
        const int W = uni(80, 2600), H = uni(80, 1700);
        const double sf = i % 2 == 0 ? 1.01 + 0.29 * (double)(rng() % 1000000) / 1e6 : fixed[rng() % 4];
        served += check_config(W, H, sf, uni(2, 11));
    }
    for (int W = 64; W <= 4096; W += 64)         // level 0 without padding; every fixed factor also makes some pyramid widths multiples of 64
        for (int f = 0; f < 4; f++) served += check_config(W, 480, fixed[f], 8);
    for (int w1 = 64; w1 <= 1024; w1 += 64)      // level 1 a multiple of 64 wide (plane stride == width): W = the widths that round to it at 1.2
        for (int W = (int)(w1 * 1.2) - 2; W <= (int)(w1 * 1.2) + 2; W++) served += check_config(W, 480, 1.2, 4);
    std::printf("%ld levels, %ld lanes, %ld with a clamped window, %ld failures\n", served, g_lanes, g_clamped, g_bad);
    if (g_bad || served < 5000 || g_clamped == 0) return 1;
    std::printf("resize_window_test OK\n");
    return 0;
}
