// orbm_newkeyframe.hip — the head of LocalMapping::Run on the device map for gfx950 (include/orbhip.h "New key frame"): the association loop
// of LocalMapping::ProcessNewKeyFrame, LocalMapping::MapPointCulling with the map effects of MapPoint::SetBadFlag, and the recent-points
// list the two share with CreateNewMapPoints.
//
// Form (DESIGN.md "New key frame").  Nothing here is serial in its effects: a feature's (a list entry's) turn reads its own point's state as
// the map gives it, and the one exception, a point that occurs twice, is settled by an integer atomicMin of the position per point.  So both
// functions are lane-per-item kernels, stable compactions by one workgroup (wg_scan.inc), and the merged CSR by obs_csr.inc's three launches
// over the points (the scan runs at the head of k_nk_select / k_mc_compact, which go on compacting on the same scratch; an overflow writes
// nothing).  A lane walks the records of ITS point, never the items of the call.  The record check, the point test, the rows a call can use
// and the stereo weight are mapview.inc's.
//   orbm_process_new_keyframe, 8 launches:
//     k_nk_state<0>   first[p] = none, the header, the rank of every key frame
//     k_nk_assoc      a lane per feature: :378-392 -> the code; atomicMin(first[p], i) where the point has no record of the key frame
//     k_nk_count<0>   a lane per point: its rows (+1 where it gains the record), summed per block
//     k_nk_select     one workgroup: the block sums scanned, the overflow decided; the features in chunks of 256: who added (first[p] == i)
//                     -> d_sel, who pushed -> the recent list, both in feature order
//     k_nk_write<0>   a lane per point: its rows copied as they lie, the new record at its rank, nObs, ORBM_MP_HAS_OBS
//     orbm_refresh_map_points (two launches, orbm_refresh.hip unchanged) over the selection on the merged CSR
//     k_nk_result     what the refresh said of the selection, the result words
//   orbm_cull_map_points, 5 launches:
//     k_nk_state<1>, k_mc_decide (a lane per list entry: the `else if` chain :463-491, atomicMin(first[p], j), mark[p] where culled),
//     k_nk_count<1>, k_mc_compact (the scan; the surviving list and the culled list in list order; the result words), k_nk_write<1>
//     (the rows of the points that stay; ORBM_MP_BAD and EraseMapPointMatch of every record for the culled)
//   orbm_recent_points_push, 1 launch: k_rp_push.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "obs_csr.inc"
#include "workspace.inc"

enum { NK_H_FLAGS = 0, NK_H_NADD, NK_H_NPUSHED, NK_H_NPUSH_REQ, NK_H_NOBS, NK_H_WORDS = 8 };

struct NkWork {
    int32_t *hdr, *rank;
    int32_t *first, *mark;   // per point: the least position that claims it (INT_MAX: none); culled
    int32_t* blk;            // per block of 256 points: its rows, then the rows before it; [nblk] = the total
    int32_t* best;           // what orbm_refresh_map_points reports per point
    uint32_t* status;
    int32_t* sel;            // the selection the refresh reads: d_sel, or all -1 where the CSR overflowed
};

// The workspace, listed once.  -> its bytes (a multiple of 16)
static __host__ __device__ __forceinline__ size_t nk_work_layout(int n_kf, int n_mp, int cap_feat, unsigned char* base, NkWork& W) {
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp;
    WsCursor c{base, 16, 0};
    W.hdr = c.take<int32_t>(NK_H_WORDS);
    W.rank = c.take<int32_t>(nk);
    W.first = c.take<int32_t>(nm);
    W.mark = c.take<int32_t>(nm);
    W.blk = c.take<int32_t>(csr_blk_words(n_mp));
    W.best = c.take<int32_t>(nm);
    W.status = c.take<uint32_t>(nm);
    W.sel = c.take<int32_t>((size_t)cap_feat);
    return c.off;
}

struct NkArgs {
    orbm_localmap_view V;
    orbm_newkf_in I;
    orbm_newkf_out P;          // orbm_process_new_keyframe
    orbm_mpcull_out C;         // orbm_cull_map_points
    const int32_t *nobs_in, *recent_in, *n_recent_in;
    unsigned char* work;
    int cur;
    uint32_t mode;
};

static __device__ __forceinline__ NkWork nk_work(const NkArgs& A) {
    NkWork W;
    nk_work_layout(A.V.n_kf, A.V.n_mp, A.I.cap_feat, A.work, W);
    return W;
}

static __device__ __forceinline__ void nk_flag(const NkWork& W, uint32_t bad) { flag_or(&W.hdr[NK_H_FLAGS], bad); }

// the point of a d_kf_mp / list entry (not -1: the caller has handled "none") if it can be used, else -1: out of range or an empty slot is flagged
static __device__ __forceinline__ int nk_point(const NkArgs& A, int p, uint32_t* bad) {
    if (!view_point_ok(A.V, p)) { *bad |= ORBM_NEWKF_BAD_INDEX; return -1; }
    return p;
}

// the d_kf_mp row of a record's feature if the record can be used, else negative and flagged
static __device__ __forceinline__ int nk_record_row(const NkArgs& A, const orbm_observation& r, uint32_t* bad) {
    int idx;
    const int row = view_record_row(A.V, A.I.d_ckf, r, &idx);
    *bad |= view_record_flag(row, ORBM_NEWKF_UNSUPPORTED, ORBM_NEWKF_BAD_INDEX);
    return row;
}

static __device__ __forceinline__ int nk_weight(const NkArgs& A, int row) { return view_feat_weight(A.I.d_feat[row]); }

// the rows of the current key frame that the association can use (none where it cannot be read)
static __device__ __forceinline__ bool nk_current_rows(const NkArgs& A, int* row0, int* nf, int* drow0) {
    *row0 = *nf = *drow0 = 0;
    return view_present(A.V, A.cur) && view_call_rows(A.V, A.I.d_ckf, A.cur, A.I.cap_feat, A.I.n_kf_desc_rows, row0, nf, drow0);
}

// the recent list's cursor as it can be used
static __device__ __forceinline__ int nk_cursor(const int32_t* d_n, int cap, uint32_t* bad) {
    const int n = *d_n;
    if (n < 0 || n > cap) { *bad |= ORBM_NEWKF_BAD_INDEX; return n < 0 ? 0 : cap; }
    return n;
}

// the rows point g has in the out-CSR, and its range in the view's
template <bool CULL> static __device__ __forceinline__ int nk_rows(const NkArgs& A, const NkWork& W, int g, int* s, int* e, uint32_t* bad) {
    *s = *e = 0;
    if (!view_point_ok(A.V, g)) return 0;   // (past n_mp, or an empty slot: behind the cursor of orbm_append_new_map_points d_obs_start is not written yet)
    if (!view_obs_range(A.V, g, s, e)) { *bad |= ORBM_NEWKF_BAD_INDEX; *s = *e = 0; }
    if (CULL) return W.mark[g] ? 0 : *e - *s;
    return *e - *s + (W.first[g] != INT_MAX ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------ the kernels both functions launch
// grid x over the blocks of 256 points; block 0 also clears the header and, for the association, ranks the key frames
template <bool CULL> static __global__ __launch_bounds__(256) void k_nk_state(NkArgs A) {
    const NkWork W = nk_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < A.V.n_mp) { W.first[g] = INT_MAX; W.mark[g] = 0; }
    if (blockIdx.x != 0) return;
    if (threadIdx.x < NK_H_WORDS) W.hdr[threadIdx.x] = 0;
    __syncthreads();   // (the flag word is cleared before any lane ors into it)
    if (!CULL && view_build_ranks(A.V, W.rank)) nk_flag(W, ORBM_NEWKF_BAD_INDEX);
}

// (the CSR kernels are obs_csr.inc's count / scan / place; orb_smem = its scratch, int[2][4])
template <bool CULL> static __global__ __launch_bounds__(256) void k_nk_count(NkArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const NkWork W = nk_work(A);
    uint32_t bad = 0;
    int s, e;
    csr_count(nk_rows<CULL>(A, W, blockIdx.x * 256 + threadIdx.x, &s, &e, &bad), W.blk, (int*)orb_smem);
    nk_flag(W, bad);
}

// the result words, by one lane after a barrier behind every flag of the launch
static __device__ __forceinline__ void nk_result(const NkWork& W, int32_t* R) {
    R[ORBM_NEWKF_R_FLAGS] = (int32_t)ld_relaxed((uint32_t*)&W.hdr[NK_H_FLAGS]);
    R[ORBM_NEWKF_R_N_ADDED] = W.hdr[NK_H_NADD];
    R[ORBM_NEWKF_R_N_PUSHED] = W.hdr[NK_H_NPUSHED];
    R[ORBM_NEWKF_R_N_PUSH_REQUIRED] = W.hdr[NK_H_NPUSH_REQ];
    R[ORBM_NEWKF_R_N_OBS] = W.hdr[NK_H_NOBS];
    for (int i = ORBM_NEWKF_R_N_OBS + 1; i < ORBM_NEWKF_R_WORDS; i++) R[i] = 0;
}

// grid x over the blocks of 256 points: the out-CSR unless it overflows, and what the call does to the points it changed
template <bool CULL> static __global__ __launch_bounds__(256) void k_nk_write(NkArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const NkWork W = nk_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x, n_mp = A.V.n_mp;
    orbm_observation* out = CULL ? A.C.d_obs_out : A.P.d_obs_out;
    const bool fits = csr_total(W.blk, nblk) <= (CULL ? A.C.cap_obs_out : A.P.cap_obs_out);
    uint32_t ignore = 0;   // (the count launch and the lane of the feature / list entry flagged what cannot be read)
    int s, e;
    int at = csr_place(nk_rows<CULL>(A, W, g, &s, &e, &ignore), W.blk, n_mp, fits, CULL ? A.C.d_obs_start_out : A.P.d_obs_start_out, (int*)orb_smem);
    if (g >= n_mp || !fits) return;
    if (!(A.V.d_mp[g].flags & ORBM_MP_VALID)) return;   // (an empty slot has its start and no rows)
    if (CULL) {
        if (!W.mark[g]) {
            for (int o = s; o < e; o++) out[at++] = A.V.d_obs[o];
            return;
        }
        A.C.d_mp[g].flags |= ORBM_MP_BAD;   // MapPoint::SetBadFlag: mbBad, mObservations.clear(), EraseMapPointMatch(leftIndex) of every entry
        for (int o = s; o < e; o++) {
            const int row = nk_record_row(A, A.V.d_obs[o], &ignore);
            if (row >= 0) A.C.d_kf_mp[row] = -1;
        }
        return;
    }
    const int i = W.first[g];
    if (i == INT_MAX) {
        for (int o = s; o < e; o++) out[at++] = A.V.d_obs[o];
        return;
    }
    // AddObservation(current, i): the record goes before the first usable record of a greater rank; nObs from the array or the usable rows
    int row0, nf, drow0, sum = 0;
    nk_current_rows(A, &row0, &nf, &drow0);   // (the association ran: the rows can be read)
    orbm_observation rec;
    rec.kf = A.cur;
    rec.desc_row = drow0 + i;
    rec.flags = (A.V.d_kf[A.cur].flags & ORBM_LM_KF_BAD) ? ORBM_OBS_KF_BAD : 0u;
    const int rk = W.rank[A.cur];
    bool placed = false;
    for (int o = s; o < e; o++) {
        const orbm_observation r = A.V.d_obs[o];
        const int row = nk_record_row(A, r, &ignore);
        if (row >= 0) {
            sum += nk_weight(A, row);
            if (!placed && W.rank[r.kf] > rk) { out[at++] = rec; placed = true; }
        }
        out[at++] = r;
    }
    if (!placed) out[at++] = rec;
    const int nobs = (A.P.d_mp_nobs ? A.P.d_mp_nobs[g] : sum) + nk_weight(A, row0 + i);
    if (A.P.d_mp_nobs) A.P.d_mp_nobs[g] = nobs;
    const uint32_t f = A.P.d_mp[g].flags;
    A.P.d_mp[g].flags = (f & ~ORBM_MP_HAS_OBS) | (nobs > 0 ? ORBM_MP_HAS_OBS : 0u);
}

// ------------------------------------------------------------------------------------------------ LocalMapping.cc:375-411
// grid x over cap_feat: feature i of the current key frame
static __global__ __launch_bounds__(256) void k_nk_assoc(NkArgs A) {
    const NkWork W = nk_work(A);
    const int i = blockIdx.x * 256 + threadIdx.x;
    int row0, nf, drow0;
    uint32_t bad = 0;
    if (!nk_current_rows(A, &row0, &nf, &drow0) && i == 0) bad |= ORBM_NEWKF_BAD_INDEX;
    if (i >= A.I.cap_feat) return;
    int code = ORBM_NEWKF_CODE_NOT_VISITED;
    if (i < nf) {
        const int e0 = A.V.d_kf_mp[row0 + i];
        const int p = e0 == -1 ? -1 : nk_point(A, e0, &bad);
        if (e0 == -1) code = ORBM_NEWKF_CODE_NONE;
        else if (p < 0) code = ORBM_NEWKF_CODE_BAD_INDEX;
        else if (A.V.d_mp[p].flags & ORBM_MP_BAD) code = ORBM_NEWKF_CODE_BAD_POINT;
        else {
            // MapPoint::IsInKeyFrame: mObservations.count(pKF), over the usable records as they lie
            int s, e, last = INT_MIN;
            if (!view_obs_range(A.V, p, &s, &e)) { bad |= ORBM_NEWKF_BAD_INDEX; s = e = 0; }
            bool in_kf = false;
            for (int o = s; o < e; o++) {
                const orbm_observation r = A.V.d_obs[o];
                if (nk_record_row(A, r, &bad) < 0) continue;
                const int rk = W.rank[r.kf];
                if (rk < last) bad |= ORBM_NEWKF_UNSORTED;
                last = rk;
                in_kf |= r.kf == A.cur;
            }
            if (in_kf) code = ORBM_NEWKF_CODE_PUSHED;
            else {
                code = ORBM_NEWKF_CODE_ADDED;   // (if this is the first feature holding p: the selection settles it)
                atomicMin(&W.first[p], i);
            }
        }
    }
    A.P.d_code[i] = (uint8_t)code;
    nk_flag(W, bad);
}

// one workgroup of 256.  orb_smem = int[8]: wg_scan.inc's two sets of wave totals
static __global__ __launch_bounds__(256) void k_nk_select(NkArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const NkWork W = nk_work(A);
    const int tid = threadIdx.x, cap = A.P.cap_recent;
    int it = 0;
    const int run = csr_scan_blocks(W.blk, nblk, scan, &it);
    const bool fits = run <= A.P.cap_obs_out;   // decided before anything is written
    uint32_t bad = 0;
    const int n0 = nk_cursor(A.P.d_n_recent, cap, &bad);
    int row0, nf, drow0, n_add = 0, n_push = 0;
    nk_current_rows(A, &row0, &nf, &drow0);
    for (int c0 = 0; c0 < nf; c0 += 256) {
        const int i = c0 + tid;
        const int code = i < nf ? A.P.d_code[i] : ORBM_NEWKF_CODE_NOT_VISITED;
        const int p = (code == ORBM_NEWKF_CODE_ADDED || code == ORBM_NEWKF_CODE_PUSHED) ? A.V.d_kf_mp[row0 + i] : -1;
        const bool add = code == ORBM_NEWKF_CODE_ADDED && W.first[p] == i;
        const bool push = p >= 0 && !add;
        if (code == ORBM_NEWKF_CODE_ADDED && !add) A.P.d_code[i] = ORBM_NEWKF_CODE_PUSHED_DUP;
        int tot_a, tot_p;
        const int at_a = n_add + wg_scan_ballot<4>(add, scan, it++, &tot_a);
        const int at_p = n0 + n_push + wg_scan_ballot<4>(push, scan, it++, &tot_p);
        if (add) {
            W.sel[at_a] = fits ? p : -1;
            if (fits) A.P.d_sel[at_a] = p;
        }
        if (push && fits && at_p < cap) A.P.d_recent[at_p] = p;
        n_add += tot_a;
        n_push += tot_p;
    }
    for (int i = n_add + tid; i < A.I.cap_feat; i += 256) {
        W.sel[i] = -1;
        if (fits) A.P.d_sel[i] = -1;
    }
    const int room = cap - n0, pushed = n_push < room ? n_push : room;
    if (tid == 0) {
        if (!fits) bad |= ORBM_NEWKF_OBS_OVERFLOW;
        if (n_push > room) bad |= ORBM_NEWKF_RECENT_OVERFLOW;
        W.blk[nblk] = run;
        W.hdr[NK_H_NADD] = fits ? n_add : 0;
        W.hdr[NK_H_NPUSHED] = fits ? pushed : 0;
        W.hdr[NK_H_NPUSH_REQ] = n_push;
        W.hdr[NK_H_NOBS] = run;
        if (fits) *A.P.d_n_recent = n0 + pushed;
    }
    nk_flag(W, bad);
}

// one workgroup of 256: ORBM_REFRESH_OVERFLOW of the selection, then the result words
static __global__ __launch_bounds__(256) void k_nk_result(NkArgs A) {
    const NkWork W = nk_work(A);
    uint32_t bad = 0;
    for (int j = threadIdx.x; j < A.I.cap_feat; j += 256) {
        const int p = W.sel[j];
        if (p >= 0 && (W.status[p] & ORBM_REFRESH_OVERFLOW)) bad |= ORBM_NEWKF_REFRESH_OVERFLOW;
    }
    nk_flag(W, bad);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) nk_result(W, A.P.d_result);
}

// ------------------------------------------------------------------------------------------------ LocalMapping.cc:903
// one workgroup of 256: the entries >= 0 of the list, in order, behind the cursor
static __global__ __launch_bounds__(256) void k_rp_push(const int32_t* list, int n_list, int32_t* recent, int32_t* n_recent, int cap, int32_t* R) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    uint32_t bad = 0;
    const int n0 = nk_cursor(n_recent, cap, &bad);
    int n_push = 0;
    for (int c0 = 0, it = 0; c0 < n_list; c0 += 256, it++) {
        const int j = c0 + threadIdx.x;
        const int p = j < n_list ? list[j] : -1;
        int tot;
        const int at = n0 + n_push + wg_scan_ballot<4>(p >= 0, (int*)orb_smem, it, &tot);
        if (p >= 0 && at < cap) recent[at] = p;
        n_push += tot;
    }
    if (threadIdx.x != 0) return;
    const int room = cap - n0, pushed = n_push < room ? n_push : room;
    if (n_push > room) bad |= ORBM_NEWKF_RECENT_OVERFLOW;
    for (int i = 0; i < ORBM_NEWKF_R_WORDS; i++) R[i] = 0;
    R[ORBM_NEWKF_R_FLAGS] = (int32_t)bad;
    R[ORBM_NEWKF_R_N_PUSHED] = pushed;
    R[ORBM_NEWKF_R_N_PUSH_REQUIRED] = n_push;
    *n_recent = n0 + pushed;
}

// ------------------------------------------------------------------------------------------------ LocalMapping.cc:435-494
// grid x over cap_recent: list entry j.  Every occurrence of a point reads the same state and takes the same exit; which one is the first
// (the one that culls) the compaction reads from first[p]
static __global__ __launch_bounds__(256) void k_mc_decide(NkArgs A) {
    const NkWork W = nk_work(A);
    const int j = blockIdx.x * 256 + threadIdx.x;
    uint32_t bad = 0;
    const int n = nk_cursor(A.n_recent_in, A.C.cap_recent, &bad);
    const bool cur_ok = view_present(A.V, A.cur);
    if (!cur_ok) bad |= ORBM_NEWKF_BAD_INDEX;
    if (j != 0) bad = 0;   // (what every lane sees, one lane flags)
    if (j >= A.C.cap_recent) return;
    int code = ORBM_MPCULL_CODE_NOT_VISITED;
    if (cur_ok && j < n) {
        const int p = nk_point(A, A.recent_in[j], &bad);
        if (p < 0) code = ORBM_MPCULL_CODE_BAD_INDEX;
        else {
            atomicMin(&W.first[p], j);
            if (A.V.d_mp[p].flags & ORBM_MP_BAD) code = ORBM_MPCULL_CODE_ERASED_BAD;
            else {
                int s, e, sum = 0;
                if (!view_obs_range(A.V, p, &s, &e)) { bad |= ORBM_NEWKF_BAD_INDEX; s = e = 0; }
                for (int o = s; o < e; o++) {
                    const int row = nk_record_row(A, A.V.d_obs[o], &bad);
                    if (row >= 0) sum += nk_weight(A, row);
                }
                const int nobs = A.nobs_in ? A.nobs_in[p] : sum;
                const int th = (A.mode & ORBM_MPCULL_MONOCULAR) ? 2 : 3;
                // (int)nCurrentKFid - (int)pMP->mnFirstKFid, on the 32-bit casts (the subtraction wraps where the reference's would overflow)
                const int diff = (int)(A.I.d_ckf[A.cur].id - A.I.d_first_kf_id[p]);
                const float ratio = (float)A.I.d_found[p] / (float)A.I.d_visible[p];   // static_cast<float>(mnFound) / mnVisible
                if (ratio < 0.25f) code = ORBM_MPCULL_CODE_CULLED_RATIO;
                else if (diff >= 2 && nobs <= th) code = ORBM_MPCULL_CODE_CULLED_OBS;
                else if (diff >= 3) code = ORBM_MPCULL_CODE_RETIRED;
                else code = ORBM_MPCULL_CODE_KEPT;
                if (code == ORBM_MPCULL_CODE_CULLED_RATIO || code == ORBM_MPCULL_CODE_CULLED_OBS) W.mark[p] = 1;
            }
        }
    }
    A.C.d_code[j] = (uint8_t)code;
    nk_flag(W, bad);
}

// one workgroup of 256.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_mc_compact(NkArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const NkWork W = nk_work(A);
    const int tid = threadIdx.x, cap = A.C.cap_recent;
    int it = 0;
    const int run = csr_scan_blocks(W.blk, nblk, scan, &it);
    const bool fits = run <= A.C.cap_obs_out;
    uint32_t ignore = 0;
    const int n = view_present(A.V, A.cur) ? nk_cursor(A.n_recent_in, cap, &ignore) : 0;
    int n_keep = 0, n_cull = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int j = c0 + tid;
        int code = j < n ? A.C.d_code[j] : ORBM_MPCULL_CODE_NOT_VISITED;
        const bool culled = code == ORBM_MPCULL_CODE_CULLED_RATIO || code == ORBM_MPCULL_CODE_CULLED_OBS;
        const int p = (culled || code == ORBM_MPCULL_CODE_KEPT) ? A.recent_in[j] : -1;
        const bool cull = culled && W.first[p] == j;
        if (culled && !cull) A.C.d_code[j] = ORBM_MPCULL_CODE_ERASED_BAD;   // the first occurrence made it bad
        const bool keep = code == ORBM_MPCULL_CODE_KEPT;
        int tot_k, tot_c;
        const int at_k = n_keep + wg_scan_ballot<4>(keep, scan, it++, &tot_k);
        const int at_c = n_cull + wg_scan_ballot<4>(cull, scan, it++, &tot_c);
        if (fits && keep) A.C.d_recent_out[at_k] = p;
        if (fits && cull) A.C.d_culled[at_c] = p;
        n_keep += tot_k;
        n_cull += tot_c;
    }
    if (fits)
        for (int j = n_cull + tid; j < cap; j += 256) A.C.d_culled[j] = -1;
    __threadfence();
    __syncthreads();
    if (tid != 0) return;
    W.blk[nblk] = run;
    W.hdr[NK_H_NADD] = fits ? n_cull : 0;
    W.hdr[NK_H_NPUSHED] = fits ? n_keep : 0;
    W.hdr[NK_H_NPUSH_REQ] = n;
    W.hdr[NK_H_NOBS] = run;
    if (!fits) nk_flag(W, ORBM_NEWKF_OBS_OVERFLOW);
    else { *A.C.d_n_recent_out = n_keep; *A.C.d_n_culled = n_cull; }
    nk_result(W, A.C.d_result);
}

// ------------------------------------------------------------------------------------------------ host
static bool nk_sizes_ok(int n_kf, int n_mp, int cap_feat) { return n_kf >= 0 && n_mp >= 0 && cap_feat >= 1; }

extern "C" size_t orbm_newkf_workspace_bytes(int n_kf, int n_mp, int cap_feat) {
    if (!nk_sizes_ok(n_kf, n_mp, cap_feat)) return 0;
    NkWork W;
    return nk_work_layout(n_kf, n_mp, cap_feat, nullptr, W);
}

extern "C" int orbm_process_new_keyframe(const orbm_localmap_view* view, const orbm_newkf_in* in, int current_kf,
                                         const orbm_refresh_params* params, const orbm_newkf_out* out, void* d_work, void* stream) {
    if (!view || !in || !params || !out || !d_work) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    const orbm_newkf_in& I = *in;
    const orbm_newkf_out& O = *out;
    if (view_invalid(V, VIEW_ALL) || (!V.d_kf_by_order && V.n_kf) || misaligned16(d_work)) return ORB_E_INVALID;
    if (!nk_sizes_ok(V.n_kf, V.n_mp, I.cap_feat) || I.n_kf_desc_rows < 0 || O.n_desc_rows < 0 || O.cap_obs_out < 0 || O.cap_recent < 1)
        return ORB_E_INVALID;
    if (params->nlevels < 1 || params->nlevels > 16) return ORB_E_INVALID;
    if ((V.n_kf && (!I.d_ckf || !I.d_center)) || (V.n_kf_mp_rows && !I.d_feat) || (V.n_mp && (!I.d_ref || !O.d_mp)) ||
        (I.n_kf_desc_rows && !I.d_kf_desc) || (O.n_desc_rows && !O.d_mp_desc))
        return ORB_E_INVALID;
    if (!O.d_code || !O.d_sel || !O.d_obs_start_out || (!O.d_obs_out && O.cap_obs_out) || !O.d_recent || !O.d_n_recent || !O.d_result)
        return ORB_E_INVALID;
    if (O.d_obs_start_out == V.d_obs_start || (O.d_obs_out && O.d_obs_out == V.d_obs)) return ORB_E_INVALID;
    if (misaligned16(O.d_mp) || misaligned16(I.d_kf_desc) || misaligned16(O.d_mp_desc)) return ORB_E_INVALID;

    NkArgs A = {};
    A.V = V; A.I = I; A.P = O; A.work = (unsigned char*)d_work; A.cur = current_kf;
    NkWork W;
    nk_work_layout(V.n_kf, V.n_mp, I.cap_feat, A.work, W);
    orbm_refresh_params rp = *params;
    rp.what = ORBM_REFRESH_NORMAL_DEPTH | ORBM_REFRESH_DESCRIPTOR;

    hipStream_t st = (hipStream_t)stream;
    const int nblk = csr_blocks(V.n_mp), gp = nblk < 1 ? 1 : nblk;
    hipLaunchKernelGGL((k_nk_state<false>), dim3(gp), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_nk_assoc, dim3((I.cap_feat + 255) / 256), dim3(256), 0, st, A);
    hipLaunchKernelGGL((k_nk_count<false>), dim3(gp), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_nk_select, dim3(1), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL((k_nk_write<false>), dim3(gp), dim3(256), 32, st, A, nblk);
    // (orbm_refresh_map_points refuses a null array even where its count is 0 and nothing reads it: the workspace stands in.  With n_mp == 0
    //  it launches nothing)
    const void* w = d_work;
    const int rc = orbm_refresh_map_points(O.d_mp ? O.d_mp : (orbm_map_point*)d_work, V.n_mp, O.d_mp_desc ? O.d_mp_desc : (uint8_t*)d_work,
                                           O.n_desc_rows, W.sel, I.cap_feat, O.d_obs_start_out,
                                           O.d_obs_out ? O.d_obs_out : (const orbm_observation*)w, I.d_ref ? I.d_ref : (const orbm_refresh_point*)w,
                                           I.d_center ? I.d_center : (const orbm_keyframe_center*)w, V.n_kf,
                                           I.d_kf_desc ? I.d_kf_desc : (const uint8_t*)w, I.n_kf_desc_rows, &rp, W.best, W.status, stream);
    if (rc != ORB_OK) return rc;
    hipLaunchKernelGGL(k_nk_result, dim3(1), dim3(256), 0, st, A);
    return launch_status();
}

extern "C" int orbm_recent_points_push(const int32_t* d_list, int n_list, int32_t* d_recent, int32_t* d_n_recent, int cap_recent,
                                       int32_t* d_result, void* stream) {
    if (!d_list || !d_recent || !d_n_recent || !d_result || n_list < 0 || cap_recent < 1) return ORB_E_INVALID;
    hipLaunchKernelGGL(k_rp_push, dim3(1), dim3(256), 32, (hipStream_t)stream, d_list, n_list, d_recent, d_n_recent, cap_recent, d_result);
    return launch_status();
}

extern "C" int orbm_cull_map_points(const orbm_localmap_view* view, const orbm_newkf_in* in, const int32_t* d_mp_nobs, int current_kf,
                                    uint32_t flags, const int32_t* d_recent, const int32_t* d_n_recent, const orbm_mpcull_out* out,
                                    void* d_work, void* stream) {
    if (!view || !in || !out || !d_work || !d_recent || !d_n_recent) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    const orbm_newkf_in& I = *in;
    const orbm_mpcull_out& O = *out;
    if (view_invalid(V, VIEW_ALL) || misaligned16(d_work) || (flags & ~ORBM_MPCULL_MONOCULAR)) return ORB_E_INVALID;
    if (O.cap_obs_out < 0 || O.cap_recent < 1) return ORB_E_INVALID;
    if ((V.n_kf && !I.d_ckf) || (V.n_kf_mp_rows && (!I.d_feat || !O.d_kf_mp)) ||
        (V.n_mp && (!I.d_found || !I.d_visible || !I.d_first_kf_id || !O.d_mp)))
        return ORB_E_INVALID;
    if (!O.d_code || !O.d_recent_out || !O.d_n_recent_out || !O.d_culled || !O.d_n_culled || !O.d_obs_start_out ||
        (!O.d_obs_out && O.cap_obs_out) || !O.d_result)
        return ORB_E_INVALID;
    if (O.d_recent_out == d_recent || O.d_obs_start_out == V.d_obs_start || (O.d_obs_out && O.d_obs_out == V.d_obs) || misaligned16(O.d_mp))
        return ORB_E_INVALID;

    NkArgs A = {};
    A.V = V; A.I = I; A.C = O; A.work = (unsigned char*)d_work; A.cur = current_kf; A.mode = flags;
    A.I.cap_feat = 1;   // (the selection of the association is not part of this call's workspace)
    A.nobs_in = d_mp_nobs; A.recent_in = d_recent; A.n_recent_in = d_n_recent;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = csr_blocks(V.n_mp), gp = nblk < 1 ? 1 : nblk;
    hipLaunchKernelGGL((k_nk_state<true>), dim3(gp), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_mc_decide, dim3((O.cap_recent + 255) / 256), dim3(256), 0, st, A);
    hipLaunchKernelGGL((k_nk_count<true>), dim3(gp), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_mc_compact, dim3(1), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL((k_nk_write<true>), dim3(gp), dim3(256), 32, st, A, nblk);
    return launch_status();
}
