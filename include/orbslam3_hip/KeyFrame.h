// orbslam3_hip/KeyFrame.h — adapter for the covisibility graph of ORB_SLAM3::KeyFrame over liborbhip.so (include/orbhip.h "Covisibility
// graph"): KeyFrame::UpdateConnections (KeyFrame.cc:427-550) for a list of key frames in order, the connection part of KeyFrame::SetBadFlag
// (:675-678, 696-697) for cull events in order, and the getters of :275-330, on a store that lives next to the device map.  What stays with
// the caller: the spanning tree (AddChild for every child event, ChangeParent, the loop of SetBadFlag :699-778), loop edges, and the pointer
// order of the key frames (SetPointerOrder).  The gather loop and the replay loop are shown in INTEGRATION.md "KeyFrame::UpdateConnections".
#ifndef ORBSLAM3_HIP_KEYFRAME_H
#define ORBSLAM3_HIP_KEYFRAME_H
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class CovisibilityGraph {
public:
    // The graph as the host holds it, flattened (rows of capConnections entries; any array may be nullptr: an empty graph).
    struct GraphView {
        const orbm_covis_keyframe* keyFrames = nullptr; int nKeyFrames = 0;   // mnId, the map, mbFirstConnection
        int capConnections = 0;
        const orbm_covis_entry* connections = nullptr; const int32_t* nConnections = nullptr;   // mConnectedKeyFrameWeights, insertion order
        const int32_t* orderedKeyFrames = nullptr; const int32_t* orderedWeights = nullptr; const int32_t* nOrdered = nullptr;
    };
    struct ChildEvent { int child, parent; };       // mpParent = parent; parent->AddChild(child)
    struct UpdateResult {
        std::vector<int> nmax, pKFmax, counterSize;  // per list entry; counterSize 0 = the early return (nothing of the key frame changed)
        std::vector<ChildEvent> childEvents;         // in list order
        int overflowKeyFrame = -1;
        uint32_t flags = 0;                          // ORBM_COVIS_*
    };
    struct CullEvent { int keyFrame; bool erased; };   // erased false: mbNotErase deferred it (ORBM_CULL_CODE_DEFERRED)

    // Uploads the graph: for callers whose graph lives on the host.  Synchronous.
    void SetGraph(const GraphView& G) {
        if (G.nKeyFrames < 0 || G.capConnections < 1 || (G.nKeyFrames && !G.keyFrames)) throw std::invalid_argument("CovisibilityGraph: bad graph view");
        const size_t n = (size_t)G.nKeyFrames, rows = n * (size_t)G.capConnections;
        const std::vector<orbm_covis_entry> noRows(rows, orbm_covis_entry{-1, 0});
        const std::vector<int32_t> zeros(rows > n ? rows : n, 0);
        store_.d_conn = conn_.upload(G.connections ? G.connections : noRows.data(), rows);
        store_.d_n_conn = nConn_.upload(G.nConnections ? G.nConnections : zeros.data(), n);
        store_.d_ordered_kf = okf_.upload(G.orderedKeyFrames ? G.orderedKeyFrames : zeros.data(), rows);
        store_.d_ordered_w = ow_.upload(G.orderedWeights ? G.orderedWeights : zeros.data(), rows);
        store_.d_n_ordered = nOrd_.upload(G.nOrdered ? G.nOrdered : zeros.data(), n);
        store_.cap_conn = G.capConnections; store_.reserved = 0;
        d_ckf_ = ckf_.upload(G.keyFrames, n);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        haveStore_ = true;
    }
    // For callers whose store is on the device already.
    void UseDeviceStore(const orbm_covis_store& store, orbm_covis_keyframe* d_ckf) { store_ = store; d_ckf_ = d_ckf; haveStore_ = true; }
    // The device map: KeyFrameCulling::deviceMap() or LocalMap's view; d_kf is its key-frame slab, written (covis, parent).
    void UseDeviceMap(const orbm_localmap_view& view, orbm_localmap_keyframe* d_kf) { view_ = view; d_kf_ = d_kf; haveMap_ = true; }
    // d_kf_by_order for a view that lacks it: the key-frame index at each rank of KeyFrame* address order.  Synchronous.
    void SetPointerOrder(const std::vector<int>& order) {
        const std::vector<int32_t> o(order.begin(), order.end());
        view_.d_kf_by_order = order_.upload(o.data(), o.size());
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
    }
    // The erased bytes of one problem in KeyFrameCulling::deviceWorkspace(), for EraseConnectionsOnDevice.
    static const uint8_t* ErasedBytes(const orbm_localmap_view& view, const void* cullWorkspace, int problem = 0) {
        orbm_cull_workspace_layout Y;
        detail::check(orbm_cull_workspace(view.n_kf, view.n_mp, view.n_obs, &Y), "orbm_cull_workspace");
        return (const uint8_t*)cullWorkspace + (size_t)problem * Y.stride + Y.kf_erased;
    }

    // KeyFrame::UpdateConnections of every key frame of `list`, in order (one entry: ProcessNewKeyFrame; many: CorrectLoop / MergeLocal).
    // One upload, the launches, one download, one synchronisation.  Throws std::runtime_error on ORBM_COVIS_BAD_INDEX and std::length_error
    // on ORBM_COVIS_OVERFLOW; the result is filled in before.
    void UpdateConnections(const std::vector<int>& list, uint32_t initKeyFrameId, UpdateResult& R, void* stream = nullptr) {
        using namespace detail;
        ready();
        const int n = (int)list.size();
        R = UpdateResult();
        if (n == 0) return;
        Layout out;
        const auto sHead = out.add<int32_t>(3);   // n_child_events, overflow_kf, flags
        const auto sNmax = out.add<int32_t>(n);
        const auto sKfmax = out.add<int32_t>(n);
        const auto sCounter = out.add<int32_t>(n);
        const auto sEvents = out.add<orbm_covis_child_event>(n);
        const std::vector<int32_t> l32(list.begin(), list.end());
        const int32_t* d_list = list_.upload(l32.data(), (size_t)n);
        outBuf_.ensure(out.size() + 16);
        work_.ensure(orbm_covis_workspace_bytes(view_.n_kf, n) + 16);
        int32_t* dh = at(outBuf_, sHead);
        orbm_covis_out O;
        O.d_child_events = at(outBuf_, sEvents); O.d_n_child_events = dh; O.d_overflow_kf = dh + 1; O.d_flags = (uint32_t*)(dh + 2);
        O.d_nmax = at(outBuf_, sNmax); O.d_kfmax = at(outBuf_, sKfmax); O.d_n_counter = at(outBuf_, sCounter);
        check(orbm_update_connections(&view_, &store_, d_ckf_, d_kf_, d_list, n, initKeyFrameId, &O, work_.p, stream), "orbm_update_connections");
        download(back_.ensure(out.size()), outBuf_.p, out.size(), stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sHead, 0);
        R.flags = (uint32_t)h[2]; R.overflowKeyFrame = h[1];
        R.nmax.assign(downloaded(back_, sNmax, 0), downloaded(back_, sNmax, 0) + n);
        R.pKFmax.assign(downloaded(back_, sKfmax, 0), downloaded(back_, sKfmax, 0) + n);
        R.counterSize.assign(downloaded(back_, sCounter, 0), downloaded(back_, sCounter, 0) + n);
        const orbm_covis_child_event* ev = downloaded(back_, sEvents, 0);
        for (int i = 0; i < h[0] && i < n; i++) R.childEvents.push_back(ChildEvent{ev[i].child, ev[i].parent});
        throwOn(R.flags);
    }

    // The connection part of KeyFrame::SetBadFlag for the events of KeyFrameCulling::Run, in order (replayed from the host's copy).
    uint32_t EraseConnections(const std::vector<CullEvent>& events, void* stream = nullptr) {
        ready();
        std::vector<orbm_cull_event> ev(events.size());
        std::vector<uint8_t> erased((size_t)view_.n_kf + 1, 0);
        for (size_t i = 0; i < events.size(); i++) {
            ev[i] = orbm_cull_event{events[i].keyFrame, -1, -1};
            if (events[i].erased && events[i].keyFrame >= 0 && events[i].keyFrame < view_.n_kf) erased[(size_t)events[i].keyFrame] = 1;
        }
        const int32_t n = (int32_t)events.size();
        const orbm_cull_event* d_ev = events_.upload(ev.data(), ev.size());
        const int32_t* d_n = nEvents_.upload(&n, 1);
        const uint8_t* d_er = erased_.upload(erased.data(), erased.size());
        return EraseConnectionsOnDevice(d_ev, d_n, d_er, (int)n, stream);
    }
    // The same on events that are on the device (orbm_cull_out.d_events / d_n_events of one problem, ErasedBytes() or nullptr).
    uint32_t EraseConnectionsOnDevice(const orbm_cull_event* d_events, const int32_t* d_n_events, const uint8_t* d_kf_erased, int capEvents,
                                      void* stream = nullptr) {
        using namespace detail;
        ready();
        outBuf_.ensure(256);
        work_.ensure(orbm_covis_workspace_bytes(view_.n_kf, 0) + 16);
        orbm_covis_out O;
        std::memset(&O, 0, sizeof O);
        O.d_flags = (uint32_t*)outBuf_.p;
        check(orbm_erase_connections(&view_, &store_, d_kf_, d_events, d_n_events, d_kf_erased, capEvents, &O, work_.p, stream),
              "orbm_erase_connections");
        uint32_t flags = 0;
        download(&flags, outBuf_.p, 4, stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        throwOn(flags);
        return flags;
    }

    // ---- the getters (each downloads the key frame's rows; synchronous)
    std::vector<int> GetVectorCovisibleKeyFrames(int kf) { std::vector<int> k, w; ordered(kf, k, w); return k; }
    std::vector<int> GetBestCovisibilityKeyFrames(int kf, int N) {
        std::vector<int> k, w;
        ordered(kf, k, w);
        if ((int)k.size() >= N) k.resize((size_t)std::max(N, 0));
        return k;
    }
    std::vector<int> GetCovisiblesByWeight(int kf, int w) {   // KeyFrame.cc:293-314: upper_bound on the descending weights
        std::vector<int> k, ws;
        ordered(kf, k, ws);
        if (k.empty()) return k;
        const auto it = std::upper_bound(ws.begin(), ws.end(), w, [](int a, int b) { return a > b; });
        if (it == ws.end() && ws.back() < w) return std::vector<int>();
        k.resize((size_t)(it - ws.begin()));
        return k;
    }
    int GetWeight(int kf, int other) {
        ready();
        inRange(kf);
        int32_t n = 0;
        detail::download(&n, store_.d_n_conn + kf, 4, nullptr);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        n = std::min(std::max(n, 0), store_.cap_conn);
        std::vector<orbm_covis_entry> row((size_t)n + 1);
        if (n) detail::download(row.data(), store_.d_conn + (size_t)kf * store_.cap_conn, (size_t)n * sizeof(orbm_covis_entry), nullptr);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        for (int i = 0; i < n; i++)
            if (row[(size_t)i].kf == other) return row[(size_t)i].weight;
        return 0;
    }

    const orbm_covis_store& deviceStore() const { return store_; }
    orbm_covis_keyframe* deviceKeyFrames() const { return d_ckf_; }
    const orbm_localmap_view& deviceMap() const { return view_; }

private:
    void ready() const { if (!haveStore_ || !haveMap_) throw std::logic_error("CovisibilityGraph: no store or no map"); }
    void inRange(int kf) const { if (kf < 0 || kf >= view_.n_kf) throw std::out_of_range("CovisibilityGraph: key frame index"); }
    static void throwOn(uint32_t flags) {
        if (flags & ORBM_COVIS_BAD_INDEX) throw std::runtime_error("CovisibilityGraph: an index was out of range");
        if (flags & ORBM_COVIS_OVERFLOW) throw std::length_error("CovisibilityGraph: a row does not fit cap_conn");
    }
    void ordered(int kf, std::vector<int>& k, std::vector<int>& w) {
        ready();
        inRange(kf);
        int32_t n = 0;
        detail::download(&n, store_.d_n_ordered + kf, 4, nullptr);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        n = std::min(std::max(n, 0), store_.cap_conn);
        std::vector<int32_t> a((size_t)n + 1), b((size_t)n + 1);
        if (n) {
            detail::download(a.data(), store_.d_ordered_kf + (size_t)kf * store_.cap_conn, (size_t)n * 4, nullptr);
            detail::download(b.data(), store_.d_ordered_w + (size_t)kf * store_.cap_conn, (size_t)n * 4, nullptr);
        }
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        k.assign(a.begin(), a.begin() + n);
        w.assign(b.begin(), b.begin() + n);
    }

    orbm_localmap_view view_{};
    orbm_covis_store store_{};
    orbm_covis_keyframe* d_ckf_ = nullptr;
    orbm_localmap_keyframe* d_kf_ = nullptr;
    bool haveStore_ = false, haveMap_ = false;
    detail::DevBuf conn_, nConn_, okf_, ow_, nOrd_, ckf_, order_, list_, events_, nEvents_, erased_, outBuf_, work_;
    detail::HostBuf back_;
};

}  // namespace orbslam3_hip
#endif
