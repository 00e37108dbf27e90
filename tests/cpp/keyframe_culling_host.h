// keyframe_culling_host.h — LocalMapping::KeyFrameCulling (LocalMapping.cc:1176-1321) with the map effects of KeyFrame::SetBadFlag
// (KeyFrame.cc:651-688), MapPoint::EraseObservation (MapPoint.cc:197-231) and MapPoint::SetBadFlag (:254-277), restated on the host over the
// flattened map of include/orbhip.h "Key-frame culling": what a caller runs today on its pointer graph.  A point's mObservations is its slice
// of the CSR with a state per record; everything else is the reference's loop, one candidate after the other.
// Test and timing infrastructure; the product never includes it.
#ifndef KEYFRAME_CULLING_HOST_H
#define KEYFRAME_CULLING_HOST_H
#include <cmath>
#include <cstdint>
#include <vector>

#include "orbhip.h"

namespace cull_host {

struct Map {
    const orbm_map_point* mp = nullptr; int n_mp = 0;
    const int32_t* obs_start = nullptr; const orbm_observation* obs = nullptr; int n_obs = 0;
    const orbm_localmap_keyframe* kf = nullptr; int n_kf = 0;
    const int32_t* kf_mp = nullptr; int n_kf_mp_rows = 0;
    const orbm_cull_keyframe* ckf = nullptr;
    const uint8_t* feat = nullptr;
    const int32_t* mp_nobs = nullptr;   // or nullptr: the weighted sum over the records
};

struct Result {
    std::vector<uint8_t> code;
    std::vector<int32_t> nmps, nred;
    std::vector<orbm_cull_event> events;
    uint32_t flags = 0;
    // the state after the loop
    std::vector<int32_t> nobs, prev, next;
    std::vector<uint8_t> rec, rec_feat, mp_bad, kf_erased;
    int kf_in_map = 0;
};

inline bool kf_present(const Map& M, int v) { return v >= 0 && v < M.n_kf && (M.kf[v].flags & ORBM_LM_KF_PRESENT); }
inline bool rows(const Map& M, int k, int* row0, int* nf) {
    const int r = M.kf[k].mp_row0, n = M.kf[k].n_feat;
    const bool ok = r >= 0 && n >= 0 && n <= M.n_kf_mp_rows - r;
    *row0 = ok ? r : 0; *nf = ok ? n : 0;
    return ok;
}
inline bool range(const Map& M, int p, int* s, int* e) {
    *s = M.obs_start[p]; *e = M.obs_start[p + 1];
    return *s >= 0 && *e >= *s && *e <= M.n_obs;
}

// the state every problem starts from (the device's init launch)
inline void init(const Map& M, Result& R) {
    R.flags = 0;
    R.rec.assign(M.n_obs, ORBM_CULL_REC_ABSENT); R.rec_feat.assign(M.n_obs, 0);
    for (int o = 0; o < M.n_obs; o++) {
        const orbm_observation& r = M.obs[o];
        if (r.flags & ORBM_OBS_RIGHT) { R.flags |= ORBM_CULL_UNSUPPORTED; continue; }
        int row0, nf;
        if (!kf_present(M, r.kf) || !rows(M, r.kf, &row0, &nf)) { R.flags |= ORBM_CULL_BAD_INDEX; continue; }
        const long long idx = (long long)r.desc_row - (long long)M.ckf[r.kf].desc_row0;
        if (idx < 0 || idx >= nf) { R.flags |= ORBM_CULL_BAD_INDEX; continue; }
        R.rec[o] = ORBM_CULL_REC_LIVE; R.rec_feat[o] = M.feat[row0 + (int)idx];
    }
    R.prev.assign(M.n_kf, -1); R.next.assign(M.n_kf, -1); R.kf_erased.assign(M.n_kf, 0);
    for (int k = 0; k < M.n_kf; k++) {
        if (!(M.kf[k].flags & ORBM_LM_KF_PRESENT)) continue;
        const int v[2] = {M.ckf[k].prev, M.ckf[k].next};
        for (int j = 0; j < 2; j++) {
            int x = v[j];
            if (x != -1 && !kf_present(M, x)) { R.flags |= ORBM_CULL_BAD_INDEX; x = -1; }
            (j ? R.next : R.prev)[k] = x;
        }
    }
    R.nobs.assign(M.n_mp, 0); R.mp_bad.assign(M.n_mp, 0);
    for (int p = 0; p < M.n_mp; p++) {
        int s, e, sum = 0;
        if (!range(M, p, &s, &e)) R.flags |= ORBM_CULL_BAD_INDEX;
        else if (!M.mp_nobs)
            for (int o = s; o < e; o++)
                if (R.rec[o] == ORBM_CULL_REC_LIVE) sum += (R.rec_feat[o] & ORBM_CULL_FEAT_STEREO) ? 2 : 1;
        R.nobs[p] = M.mp_nobs ? M.mp_nobs[p] : sum;
        R.mp_bad[p] = (M.mp[p].flags & ORBM_MP_BAD) ? 1 : 0;
    }
}

inline int point_of(const Map& M, Result& R, int row0, int i, int* s, int* e) {
    const int p = M.kf_mp[row0 + i];
    if (p == -1) return -1;
    if (p < 0 || p >= M.n_mp || !(M.mp[p].flags & ORBM_MP_VALID) || !range(M, p, s, e)) { R.flags |= ORBM_CULL_BAD_INDEX; return -1; }
    return p;
}

// MapPoint::EraseObservation(pKF) and, where nObs drops to 2 or less, MapPoint::SetBadFlag
inline void erase_observation(const Map& M, Result& R, int p, int s, int e, int k) {
    int o = s;
    while (o < e && !(M.obs[o].kf == k && R.rec[o] != ORBM_CULL_REC_ABSENT)) o++;
    if (o == e || R.rec[o] != ORBM_CULL_REC_LIVE) return;   // !mObservations.count(pKF)
    R.rec[o] = ORBM_CULL_REC_ERASED_BY_KF;
    R.nobs[p] -= (R.rec_feat[o] & ORBM_CULL_FEAT_STEREO) ? 2 : 1;
    if (R.nobs[p] <= 2) {
        R.mp_bad[p] = 1;
        for (int q = s; q < e; q++)
            if (R.rec[q] == ORBM_CULL_REC_LIVE) R.rec[q] = ORBM_CULL_REC_ERASED_BY_POINT;
    }
}

inline void cull(const Map& M, const orbm_cull_problem& P, const int32_t* candidates, int n_candidates, Result& R) {
    init(M, R);
    R.events.clear();
    R.kf_in_map = P.n_kf_in_map;
    int n_cand = P.n_cand;
    if (P.cand_start < 0 || n_cand < 0 || n_cand > n_candidates - P.cand_start) { R.flags |= ORBM_CULL_BAD_INDEX; n_cand = 0; }
    R.code.assign(n_cand, ORBM_CULL_CODE_NOT_VISITED); R.nmps.assign(n_cand, 0); R.nred.assign(n_cand, 0);
    if (!kf_present(M, P.current_kf)) { R.flags |= ORBM_CULL_BAD_INDEX; return; }
    const int32_t* cand = candidates + (n_cand ? P.cand_start : 0);
    const int Nd = 21;
    const bool inertial = P.flags & ORBM_CULL_INERTIAL, mono = P.flags & ORBM_CULL_MONOCULAR;
    float redundant_th;
    if (!inertial) redundant_th = 0.9;
    else if (mono) redundant_th = 0.9;
    else redundant_th = 0.5;
    const uint32_t cur_id = M.ckf[P.current_kf].id;
    unsigned int last_ID = 0;
    {
        int count = 0, aux = P.current_kf;
        while (count < Nd && R.prev[aux] != -1) { aux = R.prev[aux]; count++; }
        last_ID = M.ckf[aux].id;
    }
    int count = 0;
    for (int c = 0; c < n_cand; c++) {
        count++;
        const int k = cand[c];
        if (!kf_present(M, k)) { R.flags |= ORBM_CULL_BAD_INDEX; R.code[c] = ORBM_CULL_CODE_SKIPPED; continue; }
        if (M.ckf[k].id == P.init_kf_id || (M.kf[k].flags & ORBM_LM_KF_BAD) || R.kf_erased[k]) { R.code[c] = ORBM_CULL_CODE_SKIPPED; continue; }
        int row0, nf;
        if (!rows(M, k, &row0, &nf)) R.flags |= ORBM_CULL_BAD_INDEX;
        const int thObs = 3;
        int nRedundantObservations = 0, nMPs = 0;
        for (int i = 0; i < nf; i++) {
            int s, e;
            const int p = point_of(M, R, row0, i, &s, &e);
            if (p < 0 || R.mp_bad[p]) continue;
            const uint8_t fb = M.feat[row0 + i];
            if (!mono && !(fb & ORBM_CULL_FEAT_CLOSE)) continue;
            nMPs++;
            if (R.nobs[p] > thObs) {
                const int scaleLevel = fb & ORBM_CULL_FEAT_OCTAVE;
                int nObs = 0;
                for (int o = s; o < e; o++) {
                    if (R.rec[o] != ORBM_CULL_REC_LIVE || M.obs[o].kf == k) continue;
                    if ((int)(R.rec_feat[o] & ORBM_CULL_FEAT_OCTAVE) <= scaleLevel + 1) {
                        nObs++;
                        if (nObs > thObs) break;
                    }
                }
                if (nObs > thObs) nRedundantObservations++;
            }
        }
        R.nmps[c] = nMPs; R.nred[c] = nRedundantObservations;
        int code = ORBM_CULL_CODE_KEPT;
        bool set_bad = false;
        orbm_cull_event ev{k, -1, -1};
        if (nRedundantObservations > redundant_th * nMPs) {
            if (inertial) {
                if (R.kf_in_map <= Nd) { R.code[c] = ORBM_CULL_CODE_KEPT_FEW_KFS; continue; }
                if (M.ckf[k].id > (cur_id - 2)) { R.code[c] = ORBM_CULL_CODE_KEPT_RECENT; continue; }
                const int pv = R.prev[k], nx = R.next[k];
                if (pv != -1 && nx != -1) {
                    const float t = M.ckf[nx].timestamp - M.ckf[pv].timestamp;
                    const float* a = M.ckf[k].imu_pos;
                    const float* b = M.ckf[pv].imu_pos;
                    const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
                    double n2 = 0.0;
                    for (int j = 0; j < 3; j++) n2 += (double)d[j] * (double)d[j];
                    if (((P.flags & ORBM_CULL_IMU_INITIALIZED) && (M.ckf[k].id < last_ID) && t < 3.) || (t < 0.5)) code = ORBM_CULL_CODE_CULLED_IMU1;
                    else if (!(P.flags & ORBM_CULL_INERTIAL_BA2) && (std::sqrt(n2) < 0.02) && (t < 3)) code = ORBM_CULL_CODE_CULLED_IMU2;
                    else code = ORBM_CULL_CODE_KEPT_INERTIAL;
                    if (code != ORBM_CULL_CODE_KEPT_INERTIAL) {
                        R.prev[nx] = pv; R.next[pv] = nx; R.next[k] = -1; R.prev[k] = -1;
                        ev.prev = pv; ev.next = nx;
                        set_bad = true;
                    }
                } else code = ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR;
            } else { code = ORBM_CULL_CODE_CULLED; set_bad = true; }
        }
        if (set_bad) {   // KeyFrame::SetBadFlag
            R.events.push_back(ev);
            if (M.ckf[k].flags & ORBM_CULL_KF_NOT_ERASE) code |= ORBM_CULL_CODE_DEFERRED;
            else {
                for (int i = 0; i < nf; i++) {
                    int s, e;
                    const int p = point_of(M, R, row0, i, &s, &e);
                    if (p >= 0) erase_observation(M, R, p, s, e, k);
                }
                R.kf_erased[k] = 1;
                R.kf_in_map--;
            }
        }
        R.code[c] = (uint8_t)code;
        if ((count > 20 && (P.flags & ORBM_CULL_ABORT_BA)) || count > 100) break;
    }
}

}  // namespace cull_host
#endif
