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

#include "detail/DeviceIO.h"

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
        // one device block: [inputs | mpDesc | mapPoints | bestObs | status]; upload [0, B), download [MD or MP, end of ST)
        using namespace detail;
        Layout io;
        const auto S = io.add<int32_t>(n + 1); const auto O = io.add<orbm_observation>(obs.size() + 1); const auto R = io.add<orbm_refresh_point>(n);
        const auto K = io.add<orbm_keyframe_center>(nKf + 1); const auto KD = io.add<uint8_t>((size_t)(nKfDescRows + 1) * 32); const auto L = io.add<int32_t>(sel ? sel->size() : 0);
        const auto MD = io.add<uint8_t>((size_t)(nDescRows + 1) * 32); const auto MP = io.add<orbm_map_point>(n);
        const auto B = io.add<int32_t>(n); const auto ST = io.add<uint32_t>(n);
        stage_.ensure(B.offset);
        put(stage_, S, obsStart.data(), n + 1);
        if (!obs.empty()) put(stage_, O, obs.data(), obs.size());
        put(stage_, R, ref.data(), n);
        if (nKf) put(stage_, K, kf.data(), nKf);
        if (nKfDescRows > 0) put(stage_, KD, kfDesc, (size_t)nKfDescRows * 32);
        if (sel) put(stage_, L, sel->data(), sel->size());
        if (nDescRows > 0) put(stage_, MD, mpDesc, (size_t)nDescRows * 32);
        put(stage_, MP, mapPoints.data(), n);
        io_.ensure(io.size());
        check(orb_memcpy_h2d(io_.p, stage_.p, B.offset, stream), "orb_memcpy_h2d");
        if (sel) {   // unselected points: bestObs -1, status 0
            check(orb_memset(at(io_, B), 0xFF, B.bytes, stream), "orb_memset");
            check(orb_memset(at(io_, ST), 0, ST.bytes, stream), "orb_memset");
        }
        Refresh(at(io_, MP), n, at(io_, MD), nDescRows, sel ? at(io_, L) : nullptr, sel ? (int)sel->size() : 0, at(io_, S), at(io_, O), at(io_, R), at(io_, K),
                nKf, at(io_, KD), nKfDescRows, prm, at(io_, B), at(io_, ST), stream);
        const bool withDesc = downloadDescriptors && nDescRows > 0;
        const size_t from = withDesc ? MD.offset : MP.offset, len = ST.offset + ST.bytes - from;
        download(back_.ensure(len), (const uint8_t*)io_.p + from, len, stream);
        check(orb_stream_sync(stream), "orb_memcpy_d2h");
        if (withDesc) std::memcpy(mpDesc, downloaded(back_, MD, from), (size_t)nDescRows * 32);
        std::memcpy(mapPoints.data(), downloaded(back_, MP, from), MP.bytes);
        std::memcpy(bestObs.data(), downloaded(back_, B, from), B.bytes);
        std::memcpy(status.data(), downloaded(back_, ST, from), ST.bytes);
        int overflow = 0;
        for (int p = 0; p < n; p++) overflow += (status[p] & ORBM_REFRESH_OVERFLOW) != 0;
        return overflow;
    }

    // Device records (the arguments of orbm_refresh_map_points): launches on `stream` and returns; nothing is copied or synchronised.
    static void Refresh(orbm_map_point* d_mp, int n_mp, uint8_t* d_mp_desc, int n_desc_rows, const int32_t* d_sel, int n_sel, const int32_t* d_obs_start,
                        const orbm_observation* d_obs, const orbm_refresh_point* d_ref, const orbm_keyframe_center* d_kf, int n_kf,
                        const uint8_t* d_kf_desc, int n_kf_desc_rows, const orbm_refresh_params& prm, int32_t* d_best_obs, uint32_t* d_status,
                        void* stream) {
        detail::check(orbm_refresh_map_points(d_mp, n_mp, d_mp_desc, n_desc_rows, d_sel, n_sel, d_obs_start, d_obs, d_ref, d_kf, n_kf, d_kf_desc,
                                              n_kf_desc_rows, &prm, d_best_obs, d_status, stream), "orbm_refresh_map_points");
    }

private:
    detail::DevBuf io_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
