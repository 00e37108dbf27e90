// two_view_host_timing.cpp — the plain C++ host loop of TwoViewReconstruction::Reconstruct under rule R7 (tests/cpp/two_view_host.h) on one
// CPU thread, on scenes of the shapes tools/two_view_timing.py times on the GPU: N matches out of n keys, 20 % wrong matches, 0.1 px noise,
// 200 iterations.  The reference runs FindHomography and FindFundamental on two threads; this is the one-thread figure.
//   g++ -std=c++17 -O2 -ffp-contract=off -I tests/cpp tools/two_view_host_timing.cpp -o tools/bin/two_view_host_timing
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "two_view_host.h"

static double urand(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; }
static double nrand(unsigned& s) { double a = 0; for (int i = 0; i < 12; i++) a += urand(s); return a - 6.0; }

int main() {
    const int shapes[2][2] = {{300, 2000}, {1000, 5000}};
    const int its = 200, repeats = 10;
    for (const auto& sh : shapes) {
        const int N = sh[0], n = sh[1];
        unsigned seed = 1u;
        std::vector<float> x1(n), y1(n), x2(n), y2(n);
        std::vector<int> m12(n, -1);
        for (int i = 0; i < n; i++) { x1[i] = (float)(640 * urand(seed)); y1[i] = (float)(480 * urand(seed)); x2[i] = (float)(640 * urand(seed)); y2[i] = (float)(480 * urand(seed)); }
        const double a = 4.0 * 3.14159265358979323846 / 180.0;
        for (int j = 0; j < N; j++) {
            const double x = -2 + 4 * urand(seed), y = -1.5 + 3 * urand(seed), z = 4 + 4 * urand(seed);
            const double X2 = std::cos(a) * x + std::sin(a) * z + 0.6, Y2 = y + 0.05, Z2 = -std::sin(a) * x + std::cos(a) * z + 0.1;
            const int i1 = (int)((long long)j * n / N), i2 = (int)(((long long)j * 7) % n);
            x1[i1] = (float)(500 * x / z + 320 + 0.1 * nrand(seed)); y1[i1] = (float)(500 * y / z + 240 + 0.1 * nrand(seed));
            if (j % 5 != 4) { x2[i2] = (float)(500 * X2 / Z2 + 320 + 0.1 * nrand(seed)); y2[i2] = (float)(500 * Y2 / Z2 + 240 + 0.1 * nrand(seed)); }
            m12[i1] = i2;
        }
        std::vector<int32_t> sets((size_t)its * 8), avail;
        std::srand(0);
        for (int it = 0; it < its; it++) {
            avail.resize(N);
            for (int i = 0; i < N; i++) avail[i] = i;
            for (int j = 0; j < 8; j++) {
                const int randi = int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * (int)avail.size());
                sets[(size_t)it * 8 + j] = avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
        }
        const float K4[4] = {500.f, 500.f, 320.f, 240.f};
        std::vector<double> us;
        tvhost::Result R;
        for (int r = 0; r < repeats + 2; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            R = tvhost::Reconstruct(K4, 1.0f, its, x1, y1, x2, y2, m12, sets);
            const auto t1 = std::chrono::steady_clock::now();
            if (r >= 2) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("{\"host_loop\": true, \"matches\": %d, \"keys\": %d, \"iterations\": %d, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"ok\": %d, \"model\": %d, \"n_inliers\": %d, \"n_good\": %d}\n",
                    N, n, its, us[us.size() / 2], us.front(), us.back(), (int)R.ok, R.model, R.nInliers, R.nGood);
    }
    return 0;
}
