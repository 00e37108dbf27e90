// orbslam3_hip/KeyFrameDatabase.h — adapter for ORB_SLAM3::KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) over
// liborbhip.so (include/orbhip.h "Place recognition"): add / erase / clear / clearMap and the two queries the reference calls,
// DetectRelocalizationCandidates (:785-897) and DetectNBestCandidates (:614-782).
//
// The reference keeps KeyFrame* in an inverted file; here a key frame is a slot of fixed-capacity device slabs.  The integration maps
// KeyFrame* <-> slot and gathers the flattened records (INTEGRATION.md "Place recognition" shows the loop): the BowVector as ascending words +
// values, the map id, GetBestCovisibilityKeyFrames(10) and GetConnectedKeyFrames() as slots.  Candidates come back as slots, in the
// reference's order.  The static overloads on device pointers serve a caller whose database already lives on the GPU: they move nothing.
#ifndef ORBSLAM3_HIP_KEYFRAMEDATABASE_H
#define ORBSLAM3_HIP_KEYFRAMEDATABASE_H
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class KeyFrameDatabase {
public:
    KeyFrameDatabase(int nSlots, int capF, int nMaps, int device = 0) : n_(nSlots), cap_(capF), nMaps_(nMaps), stride_(nSlots > BOWDB_MAX_CANDIDATES ? nSlots : BOWDB_MAX_CANDIDATES), kf_((size_t)nSlots), mapBad_((size_t)(nMaps > 0 ? nMaps : 1), 0) {
        if (nSlots < 1 || capF < 1 || capF > 4096 || nMaps < 1) throw std::invalid_argument("KeyFrameDatabase: nSlots, nMaps >= 1, capF in 1..4096");
        for (auto& k : kf_) { std::memset(&k, 0, sizeof(k)); for (int& c : k.covis) c = -1; }
        using namespace detail;
        const size_t N = (size_t)n_;
        Layout slab;
        W_ = slab.add<int32_t>(N * cap_); V_ = slab.add<double>(N * cap_); N_ = slab.add<int32_t>(N); K_ = slab.add<bowdb_keyframe>(N);
        RQ_ = slab.add<uint64_t>(N); RS_ = slab.add<float>(N); PQ_ = slab.add<uint64_t>(N); PS_ = slab.add<float>(N); MB_ = slab.add<uint8_t>(mapBad_.size());
        QW_ = slab.add<int32_t>(cap_); QV_ = slab.add<double>(cap_); QN_ = slab.add<int32_t>(1); Q_ = slab.add<bowdb_query>(1); C_ = slab.add<int32_t>(N);
        Out_ = slab.add<int32_t>(2 * (size_t)stride_ + 4 + sizeof(bowdb_stats) / 4); Work_ = slab.add<uint8_t>(bowdb_workspace_bytes(n_, 1));
        slab_.device = device;
        slab_.ensure(slab.size());
        detail::check(orb_memset(slab_.p, 0, slab.size(), nullptr), "orb_memset");
        detail::check(orb_stream_sync(nullptr), "orb_memset");
        // the page-locked staging block: a BowVector (words, values, count), the query record and its connected slots, the key-frame records
        Layout st;
        sW_ = st.add<int32_t>(cap_); sV_ = st.add<double>(cap_); sN_ = st.add<int32_t>(1); sQ_ = st.add<bowdb_query>(1); sC_ = st.add<int32_t>(N);
        sK_ = st.add<bowdb_keyframe>(N); sMB_ = st.add<uint8_t>(mapBad_.size());
        stage_.ensure(st.size());
    }

    // Device rows of a slot: bow_transform with out->bv_word = rowWords(slot), ... writes the BowVector in place (no copy); then add(slot, mapId).
    int32_t* rowWords(int slot) { return detail::at(slab_, W_) + (size_t)check(slot) * cap_; }
    double* rowValues(int slot) { return detail::at(slab_, V_) + (size_t)check(slot) * cap_; }
    int32_t* rowCount(int slot) { return detail::at(slab_, N_) + check(slot); }

    // KeyFrameDatabase::add (:41-49) of a key frame whose row is already on the device
    void add(int slot, int mapId, void* stream = nullptr) {
        bowdb_keyframe& k = kf_[(size_t)check(slot)];
        k.flags |= BOWDB_KF_PRESENT; k.map_id = mapId; k.seq = ++seq_;
        detail::check(orb_memset(detail::at(slab_, RQ_) + slot, 0, 8, stream), "orb_memset");
        detail::check(orb_memset(detail::at(slab_, RS_) + slot, 0, 4, stream), "orb_memset");
        detail::check(orb_memset(detail::at(slab_, PQ_) + slot, 0, 8, stream), "orb_memset");
        detail::check(orb_memset(detail::at(slab_, PS_) + slot, 0, 4, stream), "orb_memset");
        dirty_ = true;
    }
    // the same from a host BowVector (ascending words, their values)
    void add(int slot, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values, void* stream = nullptr) {
        const int32_t n = (int32_t)words.size();
        if (words.size() != values.size() || n > cap_) throw std::invalid_argument("KeyFrameDatabase::add: BowVector larger than capF");
        send(rowWords(slot), sW_, words.data(), n, stream);
        send(rowValues(slot), sV_, values.data(), n, stream);
        send(rowCount(slot), sN_, &n, 1, stream);
        detail::check(orb_stream_sync(stream), "orb_memcpy_h2d");
        add(slot, mapId, stream);
    }
    void erase(int slot) { kf_[(size_t)check(slot)].flags &= ~BOWDB_KF_PRESENT; dirty_ = true; }                       // :51-72
    void clear() { for (auto& k : kf_) k.flags &= ~BOWDB_KF_PRESENT; dirty_ = true; }                                   // :74-78
    void clearMap(int mapId) { for (auto& k : kf_) if (k.map_id == mapId) k.flags &= ~BOWDB_KF_PRESENT; dirty_ = true; }  // :80-102
    void setMap(int slot, int mapId) { kf_[(size_t)check(slot)].map_id = mapId; dirty_ = true; }                        // KeyFrame::UpdateMap
    void setMapBad(int mapId, bool bad) {
        if (mapId < 0 || mapId >= nMaps_) throw std::invalid_argument("KeyFrameDatabase: map id");
        mapBad_[(size_t)mapId] = bad; dirty_ = true;
    }
    // GetBestCovisibilityKeyFrames(10) of the slot's key frame, as slots in order
    void setCovisibles(int slot, const std::vector<int>& covis) {
        if (covis.size() > BOWDB_COVIS) throw std::invalid_argument("KeyFrameDatabase: more than 10 covisibles");
        bowdb_keyframe& k = kf_[(size_t)check(slot)];
        for (int c = 0; c < BOWDB_COVIS; c++) k.covis[c] = c < (int)covis.size() ? covis[(size_t)c] : -1;
        dirty_ = true;
    }

    // DetectRelocalizationCandidates(F, pMap): id = F->mnId (non-zero, greater than every id used before), the frame's BowVector.  Returns the
    // candidate slots in the reference's order; synchronises `stream`.
    std::vector<int> DetectRelocalizationCandidates(uint64_t id, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values,
                                                    bowdb_stats* stats = nullptr, void* stream = nullptr) {
        if (id == 0 || id <= lastReloc_) throw std::invalid_argument("KeyFrameDatabase: relocalisation ids are non-zero and increasing");
        lastReloc_ = id;
        const bowdb_view v = view(stream);
        upload(id, mapId, words, values, nullptr, stream);
        const bowdb_query_bows qb = bows();
        int32_t* out = detail::at(slab_, Out_);
        DetectRelocalizationCandidates(v, detail::at(slab_, Q_), 1, qb, out + 4, stride_, out, out + 1, (bowdb_stats*)(out + 4 + 2 * (size_t)stride_), detail::at(slab_, Work_), stream);
        const std::vector<int32_t> h = download(stream, stats);
        return std::vector<int>(h.begin() + 4, h.begin() + 4 + h[0]);
    }

    // DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates): id = pKF->mnId, connected = GetConnectedKeyFrames() as slots
    void DetectNBestCandidates(uint64_t id, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values, const std::vector<int>& connected,
                               std::vector<int>& loopCand, std::vector<int>& mergeCand, int nNumCandidates, bowdb_stats* stats = nullptr, void* stream = nullptr) {
        if (id == 0 || id <= lastPlace_) throw std::invalid_argument("KeyFrameDatabase: place-recognition ids are non-zero and increasing");
        if (nNumCandidates < 1 || nNumCandidates > BOWDB_MAX_CANDIDATES || (int)connected.size() > n_) throw std::invalid_argument("KeyFrameDatabase: nNumCandidates / connected");
        lastPlace_ = id;
        const bowdb_view v = view(stream);
        upload(id, mapId, words, values, &connected, stream);
        const bowdb_query_bows qb = bows();
        int32_t* out = detail::at(slab_, Out_);
        DetectNBestCandidates(v, detail::at(slab_, Q_), 1, qb, detail::at(slab_, C_), (int)connected.size(), nNumCandidates, out + 4, out, out + 4 + stride_, out + 1,
                              (bowdb_stats*)(out + 4 + 2 * (size_t)stride_), detail::at(slab_, Work_), stream);
        const std::vector<int32_t> h = download(stream, stats);
        loopCand.assign(h.begin() + 4, h.begin() + 4 + h[0]);
        mergeCand.assign(h.begin() + 4 + stride_, h.begin() + 4 + stride_ + h[1]);
    }

    // Device records (the arguments of the C entry points): launch on `stream` and return; nothing is copied or synchronised.
    static void DetectRelocalizationCandidates(const bowdb_view& db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows& q, int32_t* d_cand,
                                               int cap_cand, int32_t* d_n_cand, int32_t* d_n_required, bowdb_stats* d_stats, void* d_workspace, void* stream) {
        detail::check(bowdb_detect_relocalization_candidates(&db, d_queries, n_queries, &q, d_cand, cap_cand, d_n_cand, d_n_required, d_stats, d_workspace, stream), "bowdb_detect_relocalization_candidates");
    }
    static void DetectNBestCandidates(const bowdb_view& db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows& q, const int32_t* d_conn, int n_conn,
                                      int n_candidates, int32_t* d_loop, int32_t* d_n_loop, int32_t* d_merge, int32_t* d_n_merge, bowdb_stats* d_stats,
                                      void* d_workspace, void* stream) {
        detail::check(bowdb_detect_n_best_candidates(&db, d_queries, n_queries, &q, d_conn, n_conn, n_candidates, d_loop, d_n_loop, d_merge, d_n_merge, d_stats,
                                                     d_workspace, stream), "bowdb_detect_n_best_candidates");
    }

    // the database as the C entry points take it (records uploaded if they changed)
    bowdb_view view(void* stream = nullptr) {
        using namespace detail;
        if (dirty_) {
            send(at(slab_, K_), sK_, kf_.data(), kf_.size(), stream);
            send(at(slab_, MB_), sMB_, mapBad_.data(), mapBad_.size(), stream);
            detail::check(orb_stream_sync(stream), "orb_memcpy_h2d");
            dirty_ = false;
        }
        bowdb_view v;
        v.bv_word = at(slab_, W_); v.bv_value = at(slab_, V_); v.bv_n = at(slab_, N_); v.kf = at(slab_, K_);
        v.reloc_query = at(slab_, RQ_); v.reloc_score = at(slab_, RS_); v.place_query = at(slab_, PQ_); v.place_score = at(slab_, PS_);
        v.map_bad = at(slab_, MB_); v.n_slots = n_; v.cap_f = cap_; v.n_maps = nMaps_; v.scoring = BOWDB_L1_NORM;
        return v;
    }

private:
    int check(int slot) const { if (slot < 0 || slot >= n_) throw std::out_of_range("KeyFrameDatabase: slot"); return slot; }
    bowdb_query_bows bows() const {
        bowdb_query_bows b;
        b.q_word = detail::at(slab_, QW_); b.q_value = detail::at(slab_, QV_); b.q_n = detail::at(slab_, QN_); b.n_rows = 1; b.cap_q = cap_;
        return b;
    }
    void upload(uint64_t id, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values, const std::vector<int>* conn, void* stream) {
        const int32_t n = (int32_t)words.size();
        if (words.size() != values.size() || n > cap_) throw std::invalid_argument("KeyFrameDatabase: query BowVector larger than capF");
        const size_t nc = conn ? conn->size() : 0;
        bowdb_query q;
        q.id = id; q.map_id = mapId; q.row = 0; q.conn_start = 0; q.conn_n = (int32_t)nc;
        send(detail::at(slab_, QW_), sW_, words.data(), n, stream);
        send(detail::at(slab_, QV_), sV_, values.data(), n, stream);
        send(detail::at(slab_, QN_), sN_, &n, 1, stream);
        send(detail::at(slab_, Q_), sQ_, &q, 1, stream);
        if (nc) send(detail::at(slab_, C_), sC_, conn->data(), nc, stream);
    }
    // host data -> its section of the staging block -> the device, one copy on `stream`
    template <class T> void send(T* d, detail::Section<T> s, const T* h, size_t count, void* stream) {
        detail::put(stage_, s, h, count);
        detail::check(orb_memcpy_h2d(d, stage_.p + s.offset, count * sizeof(T), stream), "orb_memcpy_h2d");
    }
    // [n_a, n_b, -, -, list a [stride_], list b [stride_], stats]
    std::vector<int32_t> download(void* stream, bowdb_stats* stats) {
        detail::download(back_.ensure(Out_.bytes), detail::at(slab_, Out_), Out_.bytes, stream);
        detail::check(orb_stream_sync(stream), "orb_memcpy_d2h");
        const int32_t* out = detail::downloaded(back_, Out_, Out_.offset);
        if (stats) std::memcpy(stats, out + 4 + 2 * (size_t)stride_, sizeof(bowdb_stats));
        return std::vector<int32_t>(out, out + Out_.bytes / 4);
    }

    int n_, cap_, nMaps_, stride_;   // stride_: room of each candidate list in the output block
    std::vector<bowdb_keyframe> kf_;
    std::vector<uint8_t> mapBad_;
    uint32_t seq_ = 0;
    uint64_t lastReloc_ = 0, lastPlace_ = 0;
    bool dirty_ = true;
    // sections of the device slab (BowVector rows, key-frame records, score tables, the query, the output block, the workspace) and, s*, of the
    // staging block
    detail::Section<int32_t> W_, N_, QW_, QN_, C_, Out_, sW_, sN_, sC_;
    detail::Section<double> V_, QV_, sV_;
    detail::Section<uint64_t> RQ_, PQ_;
    detail::Section<float> RS_, PS_;
    detail::Section<uint8_t> MB_, Work_, sMB_;
    detail::Section<bowdb_keyframe> K_, sK_;
    detail::Section<bowdb_query> Q_, sQ_;
    detail::DevBuf slab_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
