// covisibility_host_test.cpp — the host restatement of the covisibility graph (tests/cpp/covisibility_host.h) on hand-made maps whose answers
// are worked out in the comments.  Links no library; also built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "covisibility_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

typedef std::vector<int> Ints;

static Ints keys(const std::vector<orbm_covis_entry>& row) { Ints k; for (const auto& e : row) k.push_back(e.kf); return k; }
static Ints weights(const std::vector<orbm_covis_entry>& row) { Ints w; for (const auto& e : row) w.push_back(e.weight); return w; }

int main() {
    {   // A = 0 shares 14, 15, 16 and 3 points with key frames 1..4; pointer order 3, 0, 4, 1, 2.  The own map holds all four in pointer order;
        // 15 is connected, 14 is not; the list is weight descending; the parent is its front
        covis_synth::World W = covis_synth::star({14, 15, 16, 3}, {3, 0, 4, 1, 2});
        covis_host::Graph G(W.map(), W.ckf);
        const covis_host::Update U = covis_host::update_connections(W.map(), G, 0, 99u);
        CHECK(U.n_counter == 4 && U.nmax == 16 && U.kfmax == 3 && U.event && U.parent == 3);
        CHECK(keys(G.conn[0]) == Ints({3, 4, 1, 2}) && weights(G.conn[0]) == Ints({16, 3, 14, 15}));
        CHECK(G.okf[0] == Ints({3, 2}) && G.ow[0] == Ints({16, 15}) && G.parent[0] == 3 && !(G.ckf[0].flags & ORBM_COVIS_KF_FIRST_CONNECTION));
        CHECK(G.conn[1].empty() && G.conn[4].empty() && keys(G.conn[2]) == Ints({0}) && weights(G.conn[3]) == Ints({16}) && G.okf[3] == Ints({0}));
        // a second update changes nothing (the same weights: no AddConnection rebuilds) and raises no event
        const covis_host::Update U2 = covis_host::update_connections(W.map(), G, 0, 99u);
        CHECK(U2.n_counter == 4 && !U2.event && G.okf[0] == Ints({3, 2}));
    }
    {   // nobody reaches 15: counts 7, 9, 9: the first maximum in pointer order (0, 3, 2, 1) is key frame 3; it alone is connected
        covis_synth::World W = covis_synth::star({7, 9, 9}, {0, 3, 2, 1});
        covis_host::Graph G(W.map(), W.ckf);
        const covis_host::Update U = covis_host::update_connections(W.map(), G, 0, 0u);   // the init key frame: no parent, the flag stays
        CHECK(U.nmax == 9 && U.kfmax == 3 && !U.event && (G.ckf[0].flags & ORBM_COVIS_KF_FIRST_CONNECTION) && G.parent[0] == -1);
        CHECK(G.okf[0] == Ints({3}) && G.ow[0] == Ints({9}) && keys(G.conn[0]) == Ints({3, 2, 1}));
        CHECK(keys(G.conn[3]) == Ints({0}) && G.conn[2].empty() && G.conn[1].empty());
    }
    {   // equal weights: ties by pointer order descending (order 2, 0, 1, 3: key frame 3 has the highest rank); a bad observer is not counted
        covis_synth::World W = covis_synth::star({17, 17, 17}, {2, 0, 1, 3});
        covis_host::Graph G(W.map(), W.ckf);
        covis_host::update_connections(W.map(), G, 0, 99u);
        CHECK(G.okf[0] == Ints({3, 1, 2}));
        covis_host::Graph H(W.map(), W.ckf);
        H.bad[1] = 1;
        const covis_host::Update U = covis_host::update_connections(W.map(), H, 0, 99u);
        CHECK(U.n_counter == 2 && H.okf[0] == Ints({3, 2}) && H.conn[1].empty());
    }
    {   // the rebuild of a neighbour lists its whole map: B = 1 holds {2: 3} below the threshold; A's AddConnection(0, 20) surfaces it
        covis_synth::World W = covis_synth::star({20, 0}, {0, 1, 2});
        covis_host::Graph G(W.map(), W.ckf);
        G.conn[1].push_back(orbm_covis_entry{2, 3});
        covis_host::update_connections(W.map(), G, 0, 99u);
        CHECK(keys(G.conn[1]) == Ints({2, 0}) && G.okf[1] == Ints({0, 2}) && G.ow[1] == Ints({20, 3}));
        // the erase: key frame 0 goes; 1 loses its entry and is rebuilt, 0's map and list are emptied
        covis_host::erase_connections(G, 0);
        CHECK(keys(G.conn[1]) == Ints({2}) && G.okf[1] == Ints({2}) && G.conn[0].empty() && G.okf[0].empty() && G.bad[0]);
        // 2's map never held 1: erasing 2 changes nothing of 1 (its list keeps the bad key frame)
        covis_host::erase_connections(G, 2);
        CHECK(keys(G.conn[1]) == Ints({2}) && G.okf[1] == Ints({2}));
    }
    std::printf("covisibility_host_test OK\n");
    return 0;
}
