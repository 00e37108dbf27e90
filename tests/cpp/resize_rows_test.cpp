// resize_rows_test.cpp — host check of the records a k_resize2 wave reads in place of computing them (csrc/resize_window.inc: resize2_records, the
// builder orbx_create calls).  Stand-alone: links no library.  For random (width, height, scale factor 1.01 ... 1.3, 2 ... 8 levels) configurations
// with sizes 64 ... 1 300, every level the kernel would build, and the strip heights / prefetch depths the shipped and the test builds use:
//   * every row record against its definition from resize_coef: e1 and the "same row" flag against the two clips, the weights against yw, the
//     "next row shares the second tap" flag against the next record, end marks behind a strip row's last record;
//   * every strip record: y0 / y1, rlo / rhi against the first and last row of the strip, column, last-column flag, index of its row records;
//   * every source row a strip names lies inside the level and inside [rlo, rhi];
//   * the walk the kernel makes of a strip from these records alone (prologue of `depth` loads, `rounds` rounds that load without a test, the rows
//     behind them): it asks only for rows of [rlo, rhi], each exactly once but for a strip shorter than the depth, has a row in its slot when it
//     filters it, and emits rows y0 ... y1 - 1 in order, each behind its second tap with its first tap one row back (or the same row).
// The level sizes and scales are orbx_create's.
#include "../../awesome-orb-slam3-3dvisioncraft-version_amd/csrc/resize_window.inc"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static long g_bad = 0, g_rows = 0, g_strips = 0, g_same = 0, g_short = 0, g_shared = 0;

static void fail(const char* what, int sh, int dh, int stripRows, int depth, int at) {
    if (g_bad++ < 10) std::fprintf(stderr, "FAIL %s: %d -> %d rows, strips of %d rows, depth %d, at %d\n", what, sh, dh, stripRows, depth, at);
}

// one level: dh destination rows from sh source rows, dw destination columns
static void check_level(int sh, int dh, int dw, int stripRows, int depth) {
    const double scale = 1. / ((double)dh / sh);
    std::vector<int> ys(dh), yw(dh);
    for (int y = 0; y < dh; y++) { int s0, w0, w1; resize_coef(y, scale, sh, false, s0, w0, w1); ys[y] = s0; yw[y] = (w0 & 0xFFFF) | (w1 << 16); }
    auto clip = [&](int r) { return std::min(std::max(r, 0), sh - 1); };
    const int stripsX = (dw + 255) / 256, stripsY = (dh + stripRows - 1) / stripRows;
    std::vector<Resize2Row> rows;
    std::vector<Resize2Strip> strips;
    resize2_records(ys.data(), yw.data(), dh, sh, stripsX, stripRows, depth, rows, strips);
#define CHECK(cond, what, at) do { if (!(cond)) { fail(what, sh, dh, stripRows, depth, at); return; } } while (0)
    CHECK((int)rows.size() == stripsY * (stripRows + 1) && (int)strips.size() == stripsY * stripsX, "record counts", 0);
    for (int i = 0; i < (int)strips.size(); i++) {
        const Resize2Strip& t = strips[i];
        const int s = i / stripsX, c = i % stripsX, y0 = s * stripRows, y1 = std::min(y0 + stripRows, dh);
        g_strips++;
        CHECK(t.y0 == y0 && t.y1 == y1 && t.col == c && t.last == (c == stripsX - 1 ? 1 : 0) && t.rec == s * (stripRows + 1), "strip record", i);
        CHECK(t.rlo == clip(ys[y0]) && t.rhi == clip(ys[y1 - 1] + 1), "rlo / rhi", i);
        CHECK(0 <= t.rlo && t.rlo <= t.rhi && t.rhi <= sh - 1, "a strip's rows outside the level", i);
        const int n = t.rhi - t.rlo + 1;
        CHECK(t.rounds >= 0 && (t.rounds == 0 || (t.rounds + 1) * depth <= n) && (t.rounds + 2) * depth > n, "rounds", i);
        g_short += n < depth;
        // the row records of the strip
        for (int y = y0; y < y0 + stripRows + 1; y++) {
            const Resize2Row& r = rows[t.rec + (y - y0)];
            if (y >= y1) { CHECK(r.e1 == -1 && r.flags == 0, "end mark", y); continue; }
            if (c == 0) g_rows++;
            const int e0 = clip(ys[y]), e1 = clip(ys[y] + 1);
            CHECK(r.e1 == e1 && (r.flags & 1) == (e0 == e1 ? 1 : 0), "e1 / same", y);
            CHECK(t.rlo <= e0 && e1 <= t.rhi, "a row's taps outside [rlo, rhi]", y);
            const int b0 = (int)(short)(yw[y] & 0xFFFF), b1 = yw[y] >> 16;   // as k_resize reads them
            CHECK(b0 >= 0 && b1 >= 0 && r.b0 == (uint32_t)b0 << 12 && r.b1 == (uint32_t)b1 << 12 && r.b0 < (1u << 24) && r.b1 < (1u << 24), "weights", y);
            CHECK(((r.flags >> 1) & 1) == (rows[t.rec + (y - y0) + 1].e1 == e1 ? 1 : 0) && (r.flags & ~3) == 0, "shared second tap flag", y);
            if (c == 0) { g_same += r.flags & 1; g_shared += (r.flags >> 1) & 1; }
        }
        if (c) continue;   // (the walk is the same for every column of a strip row)
        // the kernel's walk, from the records alone
        std::vector<int> slot(depth, -1), asked(n, 0);
        auto load = [&](int k, int rowIdx) -> bool { if (rowIdx < 0 || rowIdx >= n) return false; slot[k] = rowIdx; asked[rowIdx]++; return true; };
        int rp = t.rec, emitted = 0;
        auto step = [&](int rowIdx) -> bool {   // strip row rowIdx has been filtered: emit what it completes
            const int row = t.rlo + rowIdx;
            if (rows[rp].e1 == row) {
                bool more;
                do {
                    const Resize2Row& r = rows[rp];
                    const int y = y0 + emitted;
                    if (y >= y1 || r.e1 != row || clip(ys[y] + 1) != row) return false;
                    if (!(r.flags & 1) && (rowIdx == 0 || clip(ys[y]) != row - 1)) return false;   // its first tap is the row filtered before this one
                    emitted++;
                    more = (r.flags & 2) != 0;
                    rp++;
                } while (more);
            }
            return true;
        };
        for (int k = 0; k < depth; k++) CHECK(load(k, std::min(k, n - 1)), "prologue load outside the strip", i);
        int next = depth, row = 0;
        for (int r = 0; r < t.rounds; r++, row += depth)
            for (int k = 0; k < depth; k++) {
                CHECK(slot[k] == row + k, "a round's slot", i);
                CHECK(load(k, next++), "a round's load outside the strip", i);
                CHECK(step(row + k), "a round's step", i);
            }
        const int m = n - row;
        CHECK(m >= 1 && m <= 2 * depth - 1, "rows behind the rounds", i);
        for (int k = 0; k < depth; k++)
            if (k < m) {
                CHECK(slot[k] == row + k, "a tail slot", i);
                if (k + depth < m) CHECK(load(k, next++), "a tail load outside the strip", i);
                CHECK(step(row + k), "a tail step", i);
            }
        for (int k = 0; k < depth - 1; k++)
            if (k + depth < m) { CHECK(slot[k] == row + depth + k, "a last slot", i); CHECK(step(row + depth + k), "a last step", i); }
        CHECK(emitted == y1 - y0 && rows[rp].e1 == -1, "rows emitted", i);
        for (int j = 0; j < n; j++) CHECK(asked[j] == 1 || (n < depth && j == n - 1 && asked[j] == depth - n + 1), "a row asked for other than once", j);
    }
#undef CHECK
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
            check_level(ph, h, w, 16, 4);        // the shipped constants
            check_level(ph, h, w, 8, 2);         // the test builds'
            check_level(pw, w, h, 8, 4);         // the same arithmetic on the other axis' sizes: more heights for free
            check_level(pw, w, h, 5, 6);
            served++;
        }
        pw = w; ph = h;
    }
    return served;
}

int main() {
    std::mt19937_64 rng(2025);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo)); };
    const double fixed[5] = {1.01, 1.1, 1.2, 1.25, 1.3};
    long served = 0;
    for (int i = 0; i < 1500; i++) {
        const int W = uni(64, 1301), H = uni(64, 1301);
        const double sf = i % 2 == 0 ? 1.01 + 0.29 * (double)(rng() % 1000000) / 1e6 : fixed[rng() % 5];
        served += check_config(W, H, sf, uni(2, 9));
    }
    for (int H = 64; H <= 1300; H += 7)          // every fixed factor on a regular sweep of heights
        for (int f = 0; f < 5; f++) served += check_config(H + 40, H, fixed[f], 8);
    std::printf("%ld levels, %ld strips, %ld rows, %ld with one tap row, %ld sharing a second tap, %ld strips shorter than the depth, %ld failures\n",
                served, g_strips, g_rows, g_same, g_shared, g_short, g_bad);
    if (g_bad || served < 3000 || g_same == 0) return 1;
    std::printf("resize_rows_test OK\n");
    return 0;
}
