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

#include "ORBmatcher.h"

namespace orbslam3_hip {

class KeyFrameDatabase {
public:
    KeyFrameDatabase(int nSlots, int capF, int nMaps, int device = 0) : n_(nSlots), cap_(capF), nMaps_(nMaps), stride_(nSlots > BOWDB_MAX_CANDIDATES ? nSlots : BOWDB_MAX_CANDIDATES), kf_((size_t)nSlots), mapBad_((size_t)(nMaps > 0 ? nMaps : 1), 0) {
        if (nSlots < 1 || capF < 1 || capF > 4096 || nMaps < 1) throw std::invalid_argument("KeyFrameDatabase: nSlots, nMaps >= 1, capF in 1..4096");
        for (auto& k : kf_) { std::memset(&k, 0, sizeof(k)); for (int& c : k.covis) c = -1; }
        size_t off = 0;
        auto sec = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
        const size_t N = (size_t)n_;
        oW_ = sec(N * cap_ * 4); oV_ = sec(N * cap_ * 8); oN_ = sec(N * 4); oK_ = sec(N * sizeof(bowdb_keyframe)); oRQ_ = sec(N * 8); oRS_ = sec(N * 4);
        oPQ_ = sec(N * 8); oPS_ = sec(N * 4); oMB_ = sec(mapBad_.size()); oQW_ = sec((size_t)cap_ * 4); oQV_ = sec((size_t)cap_ * 8); oQN_ = sec(4);
        oQ_ = sec(sizeof(bowdb_query)); oC_ = sec(N * 4); oOut_ = sec((2 * (size_t)stride_ + 4) * 4 + sizeof(bowdb_stats)); oWork_ = sec(bowdb_workspace_bytes(n_, 1));
        slab_.device = device;
        d_ = (uint8_t*)slab_.ensure(off);
        if (orb_memset(d_, 0, off, nullptr) != ORB_OK || orb_stream_sync(nullptr) != ORB_OK) throw std::runtime_error("orb_memset");
    }

    // Device rows of a slot: bow_transform with out->bv_word = rowWords(slot), ... writes the BowVector in place (no copy); then add(slot, mapId).
    int32_t* rowWords(int slot) { return (int32_t*)(d_ + oW_) + (size_t)check(slot) * cap_; }
    double* rowValues(int slot) { return (double*)(d_ + oV_) + (size_t)check(slot) * cap_; }
    int32_t* rowCount(int slot) { return (int32_t*)(d_ + oN_) + check(slot); }

    // KeyFrameDatabase::add (:41-49) of a key frame whose row is already on the device
    void add(int slot, int mapId, void* stream = nullptr) {
        bowdb_keyframe& k = kf_[(size_t)check(slot)];
        k.flags |= BOWDB_KF_PRESENT; k.map_id = mapId; k.seq = ++seq_;
        if (orb_memset(d_ + oRQ_ + (size_t)slot * 8, 0, 8, stream) != ORB_OK || orb_memset(d_ + oRS_ + (size_t)slot * 4, 0, 4, stream) != ORB_OK ||
            orb_memset(d_ + oPQ_ + (size_t)slot * 8, 0, 8, stream) != ORB_OK || orb_memset(d_ + oPS_ + (size_t)slot * 4, 0, 4, stream) != ORB_OK)
            throw std::runtime_error("orb_memset");
        dirty_ = true;
    }
    // the same from a host BowVector (ascending words, their values)
    void add(int slot, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values, void* stream = nullptr) {
        const int32_t n = (int32_t)words.size();
        if (words.size() != values.size() || n > cap_) throw std::invalid_argument("KeyFrameDatabase::add: BowVector larger than capF");
        uint8_t* st = stage_.ensure((size_t)cap_ * 12 + 16);
        std::memcpy(st, words.data(), (size_t)n * 4); std::memcpy(st + (size_t)cap_ * 4, values.data(), (size_t)n * 8); std::memcpy(st + (size_t)cap_ * 12, &n, 4);
        if (orb_memcpy_h2d(rowWords(slot), st, (size_t)n * 4, stream) != ORB_OK || orb_memcpy_h2d(rowValues(slot), st + (size_t)cap_ * 4, (size_t)n * 8, stream) != ORB_OK ||
            orb_memcpy_h2d(rowCount(slot), st + (size_t)cap_ * 12, 4, stream) != ORB_OK || orb_stream_sync(stream) != ORB_OK)
            throw std::runtime_error("orb_memcpy_h2d");
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
        const bowdb_view v = view(stream);   // before upload(): both go through the staging block
        upload(id, mapId, words, values, nullptr, stream);
        const bowdb_query_bows qb = bows();
        int32_t* out = (int32_t*)(d_ + oOut_);
        DetectRelocalizationCandidates(v, (const bowdb_query*)(d_ + oQ_), 1, qb, out + 4, stride_, out, out + 1, (bowdb_stats*)(out + 4 + 2 * (size_t)stride_), d_ + oWork_, stream);
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
        int32_t* out = (int32_t*)(d_ + oOut_);
        DetectNBestCandidates(v, (const bowdb_query*)(d_ + oQ_), 1, qb, (const int32_t*)(d_ + oC_), (int)connected.size(), nNumCandidates, out + 4, out, out + 4 + stride_, out + 1,
                              (bowdb_stats*)(out + 4 + 2 * (size_t)stride_), d_ + oWork_, stream);
        const std::vector<int32_t> h = download(stream, stats);
        loopCand.assign(h.begin() + 4, h.begin() + 4 + h[0]);
        mergeCand.assign(h.begin() + 4 + stride_, h.begin() + 4 + stride_ + h[1]);
    }

    // Device records (the arguments of the C entry points): launch on `stream` and return; nothing is copied or synchronised.
    static void DetectRelocalizationCandidates(const bowdb_view& db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows& q, int32_t* d_cand,
                                               int cap_cand, int32_t* d_n_cand, int32_t* d_n_required, bowdb_stats* d_stats, void* d_workspace, void* stream) {
        if (bowdb_detect_relocalization_candidates(&db, d_queries, n_queries, &q, d_cand, cap_cand, d_n_cand, d_n_required, d_stats, d_workspace, stream) != ORB_OK)
            throw std::runtime_error("bowdb_detect_relocalization_candidates");
    }
    static void DetectNBestCandidates(const bowdb_view& db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows& q, const int32_t* d_conn, int n_conn,
                                      int n_candidates, int32_t* d_loop, int32_t* d_n_loop, int32_t* d_merge, int32_t* d_n_merge, bowdb_stats* d_stats,
                                      void* d_workspace, void* stream) {
        if (bowdb_detect_n_best_candidates(&db, d_queries, n_queries, &q, d_conn, n_conn, n_candidates, d_loop, d_n_loop, d_merge, d_n_merge, d_stats, d_workspace,
                                           stream) != ORB_OK)
            throw std::runtime_error("bowdb_detect_n_best_candidates");
    }

    // the database as the C entry points take it (records uploaded if they changed)
    bowdb_view view(void* stream = nullptr) {
        if (dirty_) {
            uint8_t* st = stage_.ensure(kf_.size() * sizeof(bowdb_keyframe) + mapBad_.size());
            std::memcpy(st, kf_.data(), kf_.size() * sizeof(bowdb_keyframe));
            std::memcpy(st + kf_.size() * sizeof(bowdb_keyframe), mapBad_.data(), mapBad_.size());
            if (orb_memcpy_h2d(d_ + oK_, st, kf_.size() * sizeof(bowdb_keyframe), stream) != ORB_OK ||
                orb_memcpy_h2d(d_ + oMB_, st + kf_.size() * sizeof(bowdb_keyframe), mapBad_.size(), stream) != ORB_OK || orb_stream_sync(stream) != ORB_OK)
                throw std::runtime_error("orb_memcpy_h2d");
            dirty_ = false;
        }
        bowdb_view v;
        v.bv_word = (const int32_t*)(d_ + oW_); v.bv_value = (const double*)(d_ + oV_); v.bv_n = (const int32_t*)(d_ + oN_); v.kf = (const bowdb_keyframe*)(d_ + oK_);
        v.reloc_query = (uint64_t*)(d_ + oRQ_); v.reloc_score = (float*)(d_ + oRS_); v.place_query = (uint64_t*)(d_ + oPQ_); v.place_score = (float*)(d_ + oPS_);
        v.map_bad = d_ + oMB_; v.n_slots = n_; v.cap_f = cap_; v.n_maps = nMaps_; v.scoring = BOWDB_L1_NORM;
        return v;
    }

private:
    int check(int slot) const { if (slot < 0 || slot >= n_) throw std::out_of_range("KeyFrameDatabase: slot"); return slot; }
    bowdb_query_bows bows() const {
        bowdb_query_bows b;
        b.q_word = (const int32_t*)(d_ + oQW_); b.q_value = (const double*)(d_ + oQV_); b.q_n = (const int32_t*)(d_ + oQN_); b.n_rows = 1; b.cap_q = cap_;
        return b;
    }
    void upload(uint64_t id, int mapId, const std::vector<int32_t>& words, const std::vector<double>& values, const std::vector<int>* conn, void* stream) {
        const int32_t n = (int32_t)words.size();
        if (words.size() != values.size() || n > cap_) throw std::invalid_argument("KeyFrameDatabase: query BowVector larger than capF");
        const size_t nc = conn ? conn->size() : 0;
        uint8_t* st = stage_.ensure((size_t)cap_ * 12 + 64 + nc * 4);
        bowdb_query q;
        q.id = id; q.map_id = mapId; q.row = 0; q.conn_start = 0; q.conn_n = (int32_t)nc;
        std::memcpy(st, words.data(), (size_t)n * 4); std::memcpy(st + (size_t)cap_ * 4, values.data(), (size_t)n * 8); std::memcpy(st + (size_t)cap_ * 12, &n, 4);
        std::memcpy(st + (size_t)cap_ * 12 + 8, &q, sizeof(q));
        for (size_t i = 0; i < nc; i++) { const int32_t c = (*conn)[i]; std::memcpy(st + (size_t)cap_ * 12 + 64 + i * 4, &c, 4); }
        bool ok = orb_memcpy_h2d(d_ + oQW_, st, (size_t)n * 4, stream) == ORB_OK && orb_memcpy_h2d(d_ + oQV_, st + (size_t)cap_ * 4, (size_t)n * 8, stream) == ORB_OK &&
                  orb_memcpy_h2d(d_ + oQN_, st + (size_t)cap_ * 12, 4, stream) == ORB_OK && orb_memcpy_h2d(d_ + oQ_, st + (size_t)cap_ * 12 + 8, sizeof(q), stream) == ORB_OK;
        if (ok && nc) ok = orb_memcpy_h2d(d_ + oC_, st + (size_t)cap_ * 12 + 64, nc * 4, stream) == ORB_OK;
        if (!ok) throw std::runtime_error("orb_memcpy_h2d");
    }
    // [n_a, n_b, -, -, list a [stride_], list b [stride_], stats]
    std::vector<int32_t> download(void* stream, bowdb_stats* stats) {
        const size_t words = 4 + 2 * (size_t)stride_ + sizeof(bowdb_stats) / 4;
        uint8_t* back = back_.ensure(words * 4);
        if (orb_memcpy_d2h(back, d_ + oOut_, words * 4, stream) != ORB_OK || orb_stream_sync(stream) != ORB_OK) throw std::runtime_error("orb_memcpy_d2h");
        std::vector<int32_t> h(words);
        std::memcpy(h.data(), back, words * 4);
        if (stats) std::memcpy(stats, back + (4 + 2 * (size_t)stride_) * 4, sizeof(bowdb_stats));
        return h;
    }

    int n_, cap_, nMaps_, stride_;   // stride_: room of each candidate list in the output block
    std::vector<bowdb_keyframe> kf_;
    std::vector<uint8_t> mapBad_;
    uint32_t seq_ = 0;
    uint64_t lastReloc_ = 0, lastPlace_ = 0;
    bool dirty_ = true;
    size_t oW_, oV_, oN_, oK_, oRQ_, oRS_, oPQ_, oPS_, oMB_, oQW_, oQV_, oQN_, oQ_, oC_, oOut_, oWork_;
    uint8_t* d_ = nullptr;
    detail::DevBuf slab_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
