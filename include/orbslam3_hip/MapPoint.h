// orbslam3_hip/MapPoint.h — adapter for the two ORB_SLAM3::MapPoint members the reference recomputes in loops over hundreds to thousands of
// points: ComputeDistinctiveDescriptors (MapPoint.cc:372-460) and UpdateNormalAndDepth (MapPoint.cc:485-558), over liborbhip.so
// (include/orbhip.h "Map-point refresh").
//
// The reference walks mObservations (a std::map<KeyFrame*, tuple<int,int>>) per point; `MapPointRefresh::Refresh` takes the flattened records an
// integration gathers from those maps (the gather loop is shown in INTEGRATION.md "Map-point refresh") for a whole batch of points and runs
// one call.  The overload on device pointers serves a caller whose map already lives on the GPU: it moves nothing.
#ifndef ORBSLAM3_HIP_MAPPOINT_H
#define ORBSLAM3_HIP_MAPPOINT_H
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "ORBmatcher.h"

namespace orbslam3_hip {

class MapPointRefresh {
public:
    // Host records.  mapPoints[p] (in/out: normal, min_distance, max_distance are rewritten), mpDesc = the map points' descriptor slab
    // (nDescRows x 32, in/out: row mapPoints[p].desc_row receives the representative descriptor unless downloadDescriptors is false), the
    // observation CSR obsStart [n + 1] / obs, ref [n], the key-frame centres kf, kfDesc = the key frames' descriptor rows (nKfDescRows x 32).
    // sel: the points to refresh, or nullptr for all.  bestObs[p] = the index of the chosen descriptor in point p's observation list (-1: none;
    // the host sets mDescriptor = that observation's row), status[p] = ORBM_REFRESH* bits (unselected points: -1 / 0).
    // One packed upload, the kernel, one packed download, all on `stream`; returns after the download has completed.
    // Returns the number of points flagged ORBM_REFRESH_OVERFLOW (more than ORBM_REFRESH_MAX_OBS usable observations: left untouched, the
    // caller refreshes them on the host).
    int Refresh(std::vector<orbm_map_point>& mapPoints, uint8_t* mpDesc, int nDescRows, const std::vector<int32_t>& obsStart,
                const std::vector<orbm_observation>& obs, const std::vector<orbm_refresh_point>& ref, const std::vector<orbm_keyframe_center>& kf,
                const uint8_t* kfDesc, int nKfDescRows, const orbm_refresh_params& prm, std::vector<int>& bestObs, std::vector<uint32_t>& status,
                const std::vector<int32_t>* sel = nullptr, void* stream = nullptr, bool downloadDescriptors = true) {
        const int n = (int)mapPoints.size(), nKf = (int)kf.size();
        bestObs.assign(n, -1);
        status.assign(n, 0u);
        if ((int)obsStart.size() != n + 1 || (int)ref.size() != n) throw std::invalid_argument("MapPointRefresh: obsStart needs n + 1 entries and ref n");
        if (n && (obsStart[0] != 0 || obsStart[n] != (int)obs.size())) throw std::invalid_argument("MapPointRefresh: obsStart does not cover obs");
        if (n == 0 || (sel && sel->empty())) return 0;
        // one device block: [inputs | mpDesc | mapPoints | bestObs | status]; upload [0, oB), download [oMD or oMP, end)
        size_t off = 0;
        auto sec = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
        const size_t oS = sec((size_t)(n + 1) * 4), oO = sec((obs.size() + 1) * sizeof(orbm_observation)), oR = sec((size_t)n * sizeof(orbm_refresh_point)),
                     oK = sec((size_t)(nKf + 1) * sizeof(orbm_keyframe_center)), oKD = sec((size_t)(nKfDescRows + 1) * 32),
                     oL = sec(sel ? sel->size() * 4 : 0), oMD = sec((size_t)(nDescRows + 1) * 32), oMP = sec((size_t)n * sizeof(orbm_map_point)),
                     oB = sec((size_t)n * 4), oST = sec((size_t)n * 4);
        uint8_t* stage = stage_.ensure(oB);
        std::memcpy(stage + oS, obsStart.data(), (size_t)(n + 1) * 4);
        if (!obs.empty()) std::memcpy(stage + oO, obs.data(), obs.size() * sizeof(orbm_observation));
        std::memcpy(stage + oR, ref.data(), (size_t)n * sizeof(orbm_refresh_point));
        if (nKf) std::memcpy(stage + oK, kf.data(), (size_t)nKf * sizeof(orbm_keyframe_center));
        if (nKfDescRows > 0) std::memcpy(stage + oKD, kfDesc, (size_t)nKfDescRows * 32);
        if (sel) std::memcpy(stage + oL, sel->data(), sel->size() * 4);
        if (nDescRows > 0) std::memcpy(stage + oMD, mpDesc, (size_t)nDescRows * 32);
        std::memcpy(stage + oMP, mapPoints.data(), (size_t)n * sizeof(orbm_map_point));
        uint8_t* d = (uint8_t*)io_.ensure(off);
        if (orb_memcpy_h2d(d, stage, oB, stream) != ORB_OK) throw std::runtime_error("orb_memcpy_h2d");
        if (sel && (orb_memset(d + oB, 0xFF, (size_t)n * 4, stream) != ORB_OK || orb_memset(d + oST, 0, (size_t)n * 4, stream) != ORB_OK))
            throw std::runtime_error("orb_memset");   // unselected points: bestObs -1, status 0
        Refresh((orbm_map_point*)(d + oMP), n, d + oMD, nDescRows, sel ? (const int32_t*)(d + oL) : nullptr, sel ? (int)sel->size() : 0,
                (const int32_t*)(d + oS), (const orbm_observation*)(d + oO), (const orbm_refresh_point*)(d + oR), (const orbm_keyframe_center*)(d + oK),
                nKf, d + oKD, nKfDescRows, prm, (int32_t*)(d + oB), (uint32_t*)(d + oST), stream);
        const size_t from = (downloadDescriptors && nDescRows > 0) ? oMD : oMP, len = oST + (size_t)n * 4 - from;
        uint8_t* back = back_.ensure(len);
        if (orb_memcpy_d2h(back, d + from, len, stream) != ORB_OK || orb_stream_sync(stream) != ORB_OK) throw std::runtime_error("orb_memcpy_d2h");
        if (from == oMD) std::memcpy(mpDesc, back, (size_t)nDescRows * 32);
        std::memcpy(mapPoints.data(), back + (oMP - from), (size_t)n * sizeof(orbm_map_point));
        std::memcpy(bestObs.data(), back + (oB - from), (size_t)n * 4);
        std::memcpy(status.data(), back + (oST - from), (size_t)n * 4);
        int overflow = 0;
        for (int p = 0; p < n; p++) overflow += (status[p] & ORBM_REFRESH_OVERFLOW) != 0;
        return overflow;
    }

    // Device records (the arguments of orbm_refresh_map_points): launches on `stream` and returns; nothing is copied or synchronised.
    static void Refresh(orbm_map_point* d_mp, int n_mp, uint8_t* d_mp_desc, int n_desc_rows, const int32_t* d_sel, int n_sel, const int32_t* d_obs_start,
                        const orbm_observation* d_obs, const orbm_refresh_point* d_ref, const orbm_keyframe_center* d_kf, int n_kf,
                        const uint8_t* d_kf_desc, int n_kf_desc_rows, const orbm_refresh_params& prm, int32_t* d_best_obs, uint32_t* d_status,
                        void* stream) {
        if (orbm_refresh_map_points(d_mp, n_mp, d_mp_desc, n_desc_rows, d_sel, n_sel, d_obs_start, d_obs, d_ref, d_kf, n_kf, d_kf_desc,
                                    n_kf_desc_rows, &prm, d_best_obs, d_status, stream) != ORB_OK)
            throw std::runtime_error("orbm_refresh_map_points");
    }

private:
    detail::DevBuf io_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
