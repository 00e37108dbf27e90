// covisibility_test.cpp — the header-only adapter orbslam3_hip::CovisibilityGraph (include/orbslam3_hip/KeyFrame.h) against the host
// restatement (tests/cpp/covisibility_host.h): a list of updates in order, the store left on the device row by row, the child events, the
// getters, the erase of cull events, the culling adapter's device map plugged in, exceptions.
#include <cstdio>
#include <cstdlib>

#include "covisibility_synth.h"
#include "orbslam3_hip/KeyFrame.h"
#include "orbslam3_hip/LocalMapping.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using orbslam3_hip::CovisibilityGraph;
using orbslam3_hip::KeyFrameCulling;
typedef std::vector<int> Ints;

static KeyFrameCulling::MapView view_of(const covis_synth::World& W) {
    const cull_synth::World& B = W.base;
    KeyFrameCulling::MapView MV;
    MV.mapPoints = B.mp.data(); MV.nMapPoints = (int)B.mp.size(); MV.obsStart = B.obs_start.data(); MV.observations = B.obs.data();
    MV.nObservations = (int)B.obs.size(); MV.keyFrames = B.kf.data(); MV.nKeyFrames = (int)B.kf.size(); MV.keyFrameMapPoints = B.kf_mp.data();
    MV.nKeyFrameMapPointRows = (int)B.kf_mp.size(); MV.cullKeyFrames = B.ckf.data(); MV.features = B.feat.data();
    return MV;
}

// a strip of key frames: key frame k holds the points [step * k, step * k + width), so neighbours share many points and far ones none
static covis_synth::World strip(int n_kf, int width, int step, const Ints& order) {
    std::vector<Ints> points(n_kf);
    for (int k = 0; k < n_kf; k++)
        for (int i = 0; i < width; i++) points[k].push_back(step * k + i);
    return covis_synth::make(points, step * (n_kf - 1) + width, order);
}

// every row of the device store against the restatement
static void compare_store(CovisibilityGraph& C, const covis_host::Graph& G, int cap) {
    const int n = (int)G.conn.size();
    std::vector<int32_t> n_conn(n), n_ord(n), okf((size_t)n * cap), ow((size_t)n * cap);
    std::vector<orbm_covis_entry> conn((size_t)n * cap);
    std::vector<orbm_covis_keyframe> ckf(n);
    const orbm_covis_store& S = C.deviceStore();
    using orbslam3_hip::detail::download;
    download(n_conn.data(), S.d_n_conn, n * 4, nullptr);
    download(n_ord.data(), S.d_n_ordered, n * 4, nullptr);
    download(conn.data(), S.d_conn, conn.size() * sizeof(orbm_covis_entry), nullptr);
    download(okf.data(), S.d_ordered_kf, okf.size() * 4, nullptr);
    download(ow.data(), S.d_ordered_w, ow.size() * 4, nullptr);
    download(ckf.data(), C.deviceKeyFrames(), ckf.size() * sizeof(orbm_covis_keyframe), nullptr);
    orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
    for (int k = 0; k < n; k++) {
        CHECK(n_conn[k] == (int)G.conn[k].size() && n_ord[k] == (int)G.okf[k].size() && ckf[k].flags == G.ckf[k].flags);
        for (int j = 0; j < n_conn[k]; j++)
            CHECK(conn[(size_t)k * cap + j].kf == G.conn[k][j].kf && conn[(size_t)k * cap + j].weight == G.conn[k][j].weight);
        for (int j = 0; j < n_ord[k]; j++) CHECK(okf[(size_t)k * cap + j] == G.okf[k][j] && ow[(size_t)k * cap + j] == G.ow[k][j]);
        CHECK(C.GetVectorCovisibleKeyFrames(k) == G.okf[k]);
    }
}

int main() {
    const int n_kf = 12, cap = 12;
    const Ints order = {7, 2, 9, 0, 11, 4, 1, 6, 10, 3, 8, 5};
    const covis_synth::World W = strip(n_kf, 40, 6, order);   // neighbours at distance d share 40 - 6 d points: 34, 28, 22, 16, 10, 4
    KeyFrameCulling K;   // the device map of the culling adapter is the graph's map
    K.SetMap(view_of(W));
    {
        CovisibilityGraph C;
        bool threw = false;
        CovisibilityGraph::UpdateResult R;
        try { C.UpdateConnections({0}, 0u, R); } catch (const std::logic_error&) { threw = true; }
        CHECK(threw);
        CovisibilityGraph::GraphView GV;
        GV.keyFrames = W.ckf.data(); GV.nKeyFrames = n_kf; GV.capConnections = cap;
        C.SetGraph(GV);
        C.UseDeviceMap(K.deviceMap(), const_cast<orbm_localmap_keyframe*>(K.deviceMap().d_kf));
        C.SetPointerOrder(order);
        covis_host::Graph G(W.map(), W.ckf);
        // ProcessNewKeyFrame: one key frame; then the loop of CorrectLoop over several, one of them twice
        const std::vector<Ints> lists = {{5}, {0, 11, 5, 3, 6, 5}, {}, {1, 2, 4, 7, 8, 9, 10}};
        for (const Ints& list : lists) {
            C.UpdateConnections(list, 0u, R);
            CHECK(R.flags == 0 && R.overflowKeyFrame == -1 && R.nmax.size() == list.size());
            size_t ev = 0;
            for (size_t i = 0; i < list.size(); i++) {
                const covis_host::Update U = covis_host::update_connections(W.map(), G, list[i], 0u);
                CHECK(R.counterSize[i] == U.n_counter && R.nmax[i] == U.nmax && R.pKFmax[i] == U.kfmax);
                if (U.event) { CHECK(ev < R.childEvents.size() && R.childEvents[ev].child == list[i] && R.childEvents[ev].parent == U.parent); ev++; }
            }
            CHECK(ev == R.childEvents.size());
            compare_store(C, G, cap);
        }
        CHECK(G.okf[5].size() == 8 && G.ow[5][0] == 34 && G.ow[5][7] == 16 && G.conn[5].size() == 11);   // distance <= 4 on both sides
        // the getters (KeyFrame.cc:275-330)
        CHECK(C.GetBestCovisibilityKeyFrames(5, 3) == Ints(G.okf[5].begin(), G.okf[5].begin() + 3) && C.GetBestCovisibilityKeyFrames(5, 20) == G.okf[5]);
        CHECK(C.GetCovisiblesByWeight(5, 28).size() == 4 && C.GetCovisiblesByWeight(5, 35).empty() && C.GetCovisiblesByWeight(5, 1) == G.okf[5]);
        CHECK(C.GetWeight(5, 4) == 34 && C.GetWeight(5, 0) == 10 && C.GetWeight(5, 5) == 0 && C.GetWeight(0, 11) == 0);
        // the parent went into the culling adapter's key-frame slab, where orbm_update_local_map reads it
        std::vector<orbm_localmap_keyframe> kf(n_kf);
        orbslam3_hip::detail::download(kf.data(), K.deviceMap().d_kf, kf.size() * sizeof(orbm_localmap_keyframe), nullptr);
        orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
        for (int k = 0; k < n_kf; k++) {
            CHECK(kf[k].parent == G.parent[k]);
            for (int j = 0; j < 10; j++) CHECK(kf[k].covis[j] == (j < (int)G.okf[k].size() ? G.okf[k][j] : -1));
        }
        // cull events in order, one deferred
        CHECK(C.EraseConnections({{4, true}, {6, false}, {5, true}}) == 0);
        covis_host::erase_connections(G, 4);
        covis_host::erase_connections(G, 5);
        for (int k = 0; k < n_kf; k++) G.bad[k] = 0;   // (the bad flags are the apply's to write; the next update reads the map's)
        compare_store(C, G, cap);
        CHECK(C.GetWeight(6, 5) == 0 && C.GetWeight(6, 7) == 34 && C.GetVectorCovisibleKeyFrames(5).empty());
        // a second adapter on the same device store
        CovisibilityGraph C2;
        C2.UseDeviceStore(C.deviceStore(), C.deviceKeyFrames());
        C2.UseDeviceMap(C.deviceMap(), const_cast<orbm_localmap_keyframe*>(C.deviceMap().d_kf));
        CHECK(C2.GetVectorCovisibleKeyFrames(7) == G.okf[7]);
        // exceptions: a list entry out of range (the result is filled in before), a getter's index, a row that does not fit
        threw = false;
        try { C.UpdateConnections({3, 99}, 0u, R); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && (R.flags & ORBM_COVIS_BAD_INDEX) && R.counterSize.size() == 2 && R.counterSize[1] == 0);
        threw = false;
        try { C.GetWeight(n_kf, 0); } catch (const std::out_of_range&) { threw = true; }
        CHECK(threw);
    }
    {
        CovisibilityGraph C;
        CovisibilityGraph::GraphView GV;
        GV.keyFrames = W.ckf.data(); GV.nKeyFrames = n_kf; GV.capConnections = 3;
        C.SetGraph(GV);
        C.UseDeviceMap(K.deviceMap(), const_cast<orbm_localmap_keyframe*>(K.deviceMap().d_kf));
        C.SetPointerOrder(order);
        CovisibilityGraph::UpdateResult R;
        bool threw = false;
        try { C.UpdateConnections({5}, 0u, R); } catch (const std::length_error&) { threw = true; }
        CHECK(threw && R.flags == ORBM_COVIS_OVERFLOW && R.overflowKeyFrame == 5);
        GV.capConnections = 0;
        threw = false;
        try { C.SetGraph(GV); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
    }
    std::printf("covisibility_test OK\n");
    return 0;
}
