// orbm_fuse_neighbors.hip — LocalMapping::SearchInNeighbors on the device map for gfx950 (include/orbhip.h "Fusion in the neighbours"): the
// last step of LocalMapping::Run that had to fuse on host objects.
//
// Form (DESIGN.md "Fusion in the neighbours").  The observations of every point live in the workspace as a linked list per point, sorted by the
// key frame's rank in d_kf_by_order (std::map<KeyFrame*, .> order): Replace moves records from list to list, AddObservation takes a record
// from the spare end of the pool.  A Fuse call is seven launches, the same for every target and for the stage-2 call into the current key
// frame; a call that does not exist (past n_targets, after an abort or an overflow) runs them on empty counts:
//   k_fn_gather       the rows of pKF (key points, descriptors, mvuRight) copied to one staging frame
//   orbm_grid_build   its grid (orbm_matcher.hip, unchanged)
//   k_fn_project      a lane per list point: ORBmatcher.cc:1677-1761 -> an orbm_query and the point's descriptor as it stands NOW
//   orbm_fuse         the window search, k_fuse itself with chi2_gate = 1 (orbm_matcher.hip, unchanged)
//   k_fn_apply        one workgroup: the matched turns compacted in list order, then ONE lane walks them (:1835-1862 is serial in its effects:
//                     every turn reads the gates and pMPinKF as the turns before it left them), then the survivors' rows are laid out as a
//                     small CSR of their own
//   orbm_refresh_map_points (two launches)   ComputeDistinctiveDescriptors of the survivors on that CSR (orbm_refresh.hip, unchanged)
// Around them: k_fn_clear, k_fn_init (the lists, nObs, bad bytes; what is wrong in the map is flagged), k_fn_targets (:917-982 on one lane,
// and the copy of the list), k_fn_candidates (:1015-1038 before the last call), k_fn_sel, and the merged CSR by obs_csr.inc's three launches
// (k_fn_count / _scan / _write: a lane's rows are its point's list; an overflow skips the CSR only).  The record check, the point test, the
// rows a call can use and the stereo weight are mapview.inc's.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "obs_csr.inc"
#include "proj_arith.inc"
#include "workspace.inc"

#define FN_GRID_CELLS (ORBM_GRID_COLS * ORBM_GRID_ROWS)
#define FN_UNOWNED INT_MIN   // p_next of a record of the map that no point has linked yet

enum { FN_H_FLAGS = 0, FN_H_NT, FN_H_NT_REQ, FN_H_NLIST, FN_H_NCAND, FN_H_NCAND_REQ, FN_H_NEV, FN_H_STOP, FN_H_POOL, FN_H_NSEL, FN_H_NSURV,
       FN_H_WORDS = 16 };
enum { FN_C_NKP = 0, FN_C_NQ = 1, FN_C_NF = 2, FN_C_WORDS = 4 };

struct FnWork {
    int32_t *hdr, *rank;
    int32_t *nobs, *head, *mark, *surv_step;
    uint8_t* bad;
    orbm_observation* p_obs;   // the record pool: [0, n_obs) the map's records where they lie, then the records AddObservation made
    int32_t *p_next, *p_idx;   // the next record of the same point (-1: the last); the record's feature index in its key frame
    int32_t *list1, *surv, *blk;
    // the staging frame of one Fuse call
    orb_keypoint* s_kps;
    uint8_t* s_desc;
    float* s_ur;
    int32_t *s_cnt, *s_gstart, *s_gidx;
    orbm_query* s_q;
    uint8_t* s_qdesc;
    int32_t *s_match, *s_dist;
    // the survivors as orbm_refresh_map_points reads them
    orbm_map_point* r_mp;
    int32_t* r_start;
    orbm_observation* r_obs;
    int32_t* r_best;
    uint32_t* r_status;
};

// The workspace, listed once.  -> its bytes (a multiple of 16)
static __host__ __device__ __forceinline__ size_t fn_work_layout(int n_kf, int n_mp, int pool_n, int cap_feat, int cap_q, unsigned char* base,
                                                                 FnWork& W) {
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp, np = (size_t)pool_n, cf = (size_t)cap_feat, cq = (size_t)cap_q;
    WsCursor c{base, 16, 0};
    W.hdr = c.take<int32_t>(FN_H_WORDS);
    W.rank = c.take<int32_t>(nk);
    W.nobs = c.take<int32_t>(nm);
    W.head = c.take<int32_t>(nm);
    W.mark = c.take<int32_t>(nm);
    W.surv_step = c.take<int32_t>(nm);
    W.bad = c.take<uint8_t>(nm);
    W.p_obs = c.take<orbm_observation>(np);
    W.p_next = c.take<int32_t>(np);
    W.p_idx = c.take<int32_t>(np);
    W.list1 = c.take<int32_t>(cf);
    W.surv = c.take<int32_t>(cq);
    W.blk = c.take<int32_t>(csr_blk_words(n_mp));
    W.s_kps = c.take<orb_keypoint>(cf);
    W.s_desc = c.take<uint8_t>(cf * 32);
    W.s_ur = c.take<float>(cf);
    W.s_cnt = c.take<int32_t>(FN_C_WORDS);
    W.s_gstart = c.take<int32_t>(FN_GRID_CELLS + 1);
    W.s_gidx = c.take<int32_t>(cf);
    W.s_q = c.take<orbm_query>(cq);
    W.s_qdesc = c.take<uint8_t>(cq * 32);
    W.s_match = c.take<int32_t>(cq);
    W.s_dist = c.take<int32_t>(cq);
    W.r_mp = c.take<orbm_map_point>(cq);
    W.r_start = c.take<int32_t>(cq + 1);
    W.r_obs = c.take<orbm_observation>(np);
    W.r_best = c.take<int32_t>(cq);
    W.r_status = c.take<uint32_t>(cq);
    return c.off;
}

struct FnArgs {
    orbm_localmap_view V;
    orbm_fusenb_in I;
    orbm_fusenb_params P;
    orbm_fusenb_out O;
    unsigned char* work;
    int cap_q, pool_n;
};

static __device__ __forceinline__ FnWork fn_work(const FnArgs& A) {
    FnWork W;
    fn_work_layout(A.V.n_kf, A.V.n_mp, A.pool_n, A.I.cap_feat, A.cap_q, A.work, W);
    return W;
}

// the rows of a readable key frame that a Fuse call can use
static __device__ __forceinline__ bool fn_kf_rows(const FnArgs& A, int kf, int* row0, int* nf, int* drow0) {
    return view_call_rows(A.V, A.I.d_ckf, kf, A.I.cap_feat, A.I.n_kf_desc_rows, row0, nf, drow0);
}

// the point of a d_kf_mp / list entry if it can be used: -1 for none; out of range or an empty slot is flagged and none
static __device__ __forceinline__ int fn_point(const FnArgs& A, int p, uint32_t* bad) {
    if (p == -1) return -1;
    if (!view_point_ok(A.V, p)) { *bad |= ORBM_FUSENB_BAD_INDEX; return -1; }
    return p;
}

static __device__ __forceinline__ int fn_weight(const FnArgs& A, int row) { return view_feat_weight(A.I.d_feat[row]); }

// MapPoint::IsInKeyFrame: mObservations.count(pKF)
static __device__ __forceinline__ bool fn_in_kf(const FnWork& W, int p, int kf) {
    for (int r = ld_relaxed(&W.head[p]); r != -1; r = ld_relaxed(&W.p_next[r]))
        if (ld_relaxed(&W.p_obs[r].kf) == kf) return true;
    return false;
}

// mObservations[pKF] = ...: record r enters the list of point p at its key frame's rank (behind an equal rank).  -> it became the last
static __device__ __forceinline__ bool fn_insert(const FnWork& W, int p, int r) {
    const int rk = W.rank[W.p_obs[r].kf];
    int prev = -1, cur = W.head[p];
    while (cur != -1 && W.rank[W.p_obs[cur].kf] <= rk) { prev = cur; cur = W.p_next[cur]; }
    W.p_next[r] = cur;
    if (prev < 0) W.head[p] = r;
    else W.p_next[prev] = r;
    return cur == -1;
}

// The key frame of Fuse call `step` and its list: steps [0, cap_targets) are the targets, step cap_targets is the call into the current key
// frame.  -> the key frame, or -1: the call does not exist
static __device__ __forceinline__ int fn_step(const FnArgs& A, const FnWork& W, int step, const int32_t** list, int* n_list, int* call) {
    *list = W.list1;
    *n_list = 0;
    *call = step;
    if (W.hdr[FN_H_STOP]) return -1;
    const int nt = W.hdr[FN_H_NT];
    if (step < A.O.cap_targets) {
        if (step >= nt) return -1;
        *n_list = W.hdr[FN_H_NLIST];
        return A.O.d_targets[step];
    }
    if (A.P.flags & ORBM_FUSENB_ABORT_BA) return -1;
    *list = A.O.d_candidates;
    *n_list = W.hdr[FN_H_NCAND];
    *call = nt;
    return A.P.current_kf;
}

// ------------------------------------------------------------------------------------------------ the state
// one workgroup: the header, the counts of the outputs, the rank of every key frame
static __global__ __launch_bounds__(256) void k_fn_clear(FnArgs A) {
    const FnWork W = fn_work(A);
    const int tid = threadIdx.x;
    if (tid < FN_H_WORDS) W.hdr[tid] = tid == FN_H_POOL ? A.V.n_obs : 0;
    if (tid < FN_C_WORDS) W.s_cnt[tid] = 0;
    if (tid < ORBM_FUSENB_R_WORDS) A.O.d_result[tid] = 0;
    for (int i = tid; i <= A.O.cap_targets; i += 256) A.O.d_nfused[i] = 0;
    for (int o = tid; o < A.V.n_obs; o += 256) W.p_next[o] = FN_UNOWNED;
    __syncthreads();   // (the header word below is cleared before any lane ors into it)
    if (view_build_ranks(A.V, W.rank)) atomicOr((uint32_t*)&W.hdr[FN_H_FLAGS], (uint32_t)ORBM_FUSENB_BAD_INDEX);
}

// a lane per point: its records checked once and linked in rank order, nObs, the bad byte
static __global__ __launch_bounds__(256) void k_fn_init(FnArgs A) {
    const FnWork W = fn_work(A);
    uint32_t bad = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < A.V.n_mp; p += gridDim.x * 256) {
        W.mark[p] = INT_MAX;
        W.surv_step[p] = 0;
        W.bad[p] = (A.V.d_mp[p].flags & ORBM_MP_BAD) ? 1 : 0;
        A.O.d_replaced[p] = -1;
        W.head[p] = -1;
        int s = 0, e = 0, sum = 0, tail = -1;
        // (a slot without a point has no records and its CSR entry is not read: behind the cursor of orbm_append_new_map_points it is not written yet)
        if ((A.V.d_mp[p].flags & ORBM_MP_VALID) && !view_obs_range(A.V, p, &s, &e)) { bad |= ORBM_FUSENB_BAD_INDEX; s = e = 0; }
        for (int o = s; o < e; o++) {
            const orbm_observation r = A.V.d_obs[o];
            // Ranges that overlap (a d_obs_start that is not monotone) would link one record into two lists: a record belongs to the first
            // point that claims it, so the lists stay disjoint and every walk ends
            if (atomicCAS(&W.p_next[o], FN_UNOWNED, -1) != FN_UNOWNED) { bad |= ORBM_FUSENB_BAD_INDEX; continue; }
            int idx;
            const int row = view_record_row(A.V, A.I.d_ckf, r, &idx);
            if (row < 0) { bad |= view_record_flag(row, ORBM_FUSENB_UNSUPPORTED, ORBM_FUSENB_BAD_INDEX); continue; }
            W.p_obs[o] = r;
            W.p_idx[o] = idx;
            if (tail >= 0 && W.rank[W.p_obs[tail].kf] <= W.rank[r.kf]) {   // in order: behind the last
                W.p_next[o] = -1;
                W.p_next[tail] = o;
                tail = o;
            } else if (fn_insert(W, p, o)) tail = o;
            else bad |= ORBM_FUSENB_UNSORTED;
            sum += fn_weight(A, row);
        }
        W.nobs[p] = A.I.d_mp_nobs ? A.I.d_mp_nobs[p] : sum;
    }
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

// ------------------------------------------------------------------------------------------------ LocalMapping.cc:917-989
// the first min(n, d_n_ordered) entries of a key frame's ordered row
static __device__ __forceinline__ int fn_best_covisibles(const FnArgs& A, int kf, int n, const int32_t** row, uint32_t* bad) {
    int cnt = A.I.d_n_ordered[kf];
    if (cnt < 0 || cnt > A.I.cap_conn) { *bad |= ORBM_FUSENB_BAD_INDEX; cnt = cnt < 0 ? 0 : A.I.cap_conn; }
    *row = A.I.d_ordered_kf + (size_t)kf * A.I.cap_conn;
    return cnt < n ? cnt : n;
}

static __global__ __launch_bounds__(256) void k_fn_targets(FnArgs A) {
    const FnWork W = fn_work(A);
    const int tid = threadIdx.x, cur = A.P.current_kf;
    uint32_t bad = 0;
    int row0 = 0, nf = 0, drow0;
    const bool cur_ok = view_present(A.V, cur) && fn_kf_rows(A, cur, &row0, &nf, &drow0);
    for (int i = tid; i < nf; i += 256) W.list1[i] = A.V.d_kf_mp[row0 + i];   // vpMapPointMatches = GetMapPointMatches(), once
    if (tid != 0) return;
    if (!cur_ok) {
        W.hdr[FN_H_STOP] = 1;
        atomicOr((uint32_t*)&W.hdr[FN_H_FLAGS], (uint32_t)ORBM_FUSENB_BAD_INDEX);
        return;
    }
    const uint32_t cur_id = A.I.d_ckf[cur].id;
    const int cap = A.O.cap_targets;
    int first[20], n = 0;
    auto push = [&](int k) {
        if (n < cap) A.O.d_targets[n] = k;
        n++;
        A.O.d_fuse_target[k] = cur_id;
    };
    const int32_t* row;
    const int nn = fn_best_covisibles(A, cur, (A.P.flags & ORBM_FUSENB_MONOCULAR) ? 20 : 10, &row, &bad);
    for (int j = 0; j < nn; j++) {
        const int k = row[j];
        if (!view_present(A.V, k)) { bad |= ORBM_FUSENB_BAD_INDEX; continue; }
        if ((A.V.d_kf[k].flags & ORBM_LM_KF_BAD) || A.O.d_fuse_target[k] == cur_id) continue;
        first[n] = k;
        push(k);
    }
    const int imax = n;
    for (int i = 0; i < imax; i++) {
        const int n2 = fn_best_covisibles(A, first[i], 20, &row, &bad);
        for (int j = 0; j < n2; j++) {
            const int k = row[j];
            if (!view_present(A.V, k)) { bad |= ORBM_FUSENB_BAD_INDEX; continue; }
            if ((A.V.d_kf[k].flags & ORBM_LM_KF_BAD) || A.O.d_fuse_target[k] == cur_id || A.I.d_ckf[k].id == cur_id) continue;
            push(k);
        }
        if (A.P.flags & ORBM_FUSENB_ABORT_BA) break;
    }
    if (A.P.flags & ORBM_FUSENB_INERTIAL) {
        int k = A.V.d_kf[cur].prev;
        for (int guard = 0; n < 20 && k != -1 && guard <= A.V.n_kf; guard++) {   // (a chain has no more links than key frames)
            if (!view_present(A.V, k)) { bad |= ORBM_FUSENB_BAD_INDEX; break; }
            if (!((A.V.d_kf[k].flags & ORBM_LM_KF_BAD) || A.O.d_fuse_target[k] == cur_id)) push(k);
            k = A.V.d_kf[k].prev;
        }
    }
    W.hdr[FN_H_NT_REQ] = n;
    W.hdr[FN_H_NLIST] = nf;
    if (n > cap) { bad |= ORBM_FUSENB_TARGET_OVERFLOW; W.hdr[FN_H_STOP] = 1; }   // nothing is fused
    else W.hdr[FN_H_NT] = n;
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

// ------------------------------------------------------------------------------------------------ one Fuse call
// grid x over cap_feat: the rows of pKF as one frame of orbm_grid_build / orbm_fuse
static __global__ __launch_bounds__(256) void k_fn_gather(FnArgs A, int step) {
    const FnWork W = fn_work(A);
    const int32_t* list;
    int n_list, call, row0 = 0, nf = 0, drow0 = 0;
    const int kf = fn_step(A, W, step, &list, &n_list, &call);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (kf >= 0 && !fn_kf_rows(A, kf, &row0, &nf, &drow0) && i == 0) atomicOr((uint32_t*)&W.hdr[FN_H_FLAGS], (uint32_t)ORBM_FUSENB_BAD_INDEX);
    if (i == 0) W.s_cnt[FN_C_NKP] = nf;
    if (i < nf) {
        W.s_kps[i] = A.I.d_kps[row0 + i];
        W.s_ur[i] = A.I.d_u_right[row0 + i];
        const uint4* src = (const uint4*)(A.I.d_kf_desc + (size_t)(drow0 + i) * 32);
        uint4* dst = (uint4*)(W.s_desc + (size_t)i * 32);
        dst[0] = src[0];
        dst[1] = src[1];
    }
}

// grid x over cap_q: ORBmatcher.cc:1677-1761 for list entry i.  isBad() and IsInKeyFrame() only ever turn true for a point inside a Fuse
// call, so a point they stop now is stopped at its turn as well: the apply reads them again there, this is the early out.
static __global__ __launch_bounds__(256) void k_fn_project(FnArgs A, int step) {
    const FnWork W = fn_work(A);
    const int32_t* list;
    int n_list, call;
    const int kf = fn_step(A, W, step, &list, &n_list, &call);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) W.s_cnt[FN_C_NQ] = kf >= 0 ? n_list : 0;
    if (kf < 0 || i >= n_list) return;
    uint32_t bad = 0;
    orbm_query Q;
    Q.u = Q.v = Q.radius = Q.u_right = Q.angle = 0.f;
    Q.min_level = Q.max_level = 0;
    Q.flags = 0;
    const int p = fn_point(A, list[i], &bad);
    if (p >= 0 && !W.bad[p] && !fn_in_kf(W, p, kf) && (A.V.d_mp[p].desc_row < 0 || A.V.d_mp[p].desc_row >= A.O.n_desc_rows))
        bad |= ORBM_FUSENB_BAD_INDEX;   // no descriptor to search with: the point is absent from this call
    else if (p >= 0 && !W.bad[p] && !fn_in_kf(W, p, kf)) {
        const orbm_map_point r = A.V.d_mp[p];
        const orbm_fusenb_pose F = A.I.d_pose[kf];
        const orbm_fusenb_params& P = A.P;
        const float X = r.pos[0], Y = r.pos[1], Z = r.pos[2];
        const float xc = mat_row(F.Rcw, X, Y, Z) + F.tcw[0];
        const float yc = mat_row(F.Rcw + 3, X, Y, Z) + F.tcw[1];
        const float zc = mat_row(F.Rcw + 6, X, Y, Z) + F.tcw[2];
        if (!(zc < 0.0f)) {
            const float invz = 1.0f / zc;
            const float u = P.fx * xc / zc + P.cx, v = P.fy * yc / zc + P.cy;
            if (u >= P.bounds[0] && u < P.bounds[1] && v >= P.bounds[2] && v < P.bounds[3]) {   // KeyFrame::IsInImage
                const float maxDistance = 1.2f * r.max_distance, minDistance = 0.8f * r.min_distance;
                const float POx = X - F.Ow[0], POy = Y - F.Ow[1], POz = Z - F.Ow[2];
                const float dist3D = (float)sqrt(dot3(POx, POy, POz, POx, POy, POz));
                if (!(dist3D < minDistance || dist3D > maxDistance) &&
                    !(dot3(POx, POy, POz, r.normal[0], r.normal[1], r.normal[2]) < 0.5 * (double)dist3D)) {
                    const int L = predict_scale(r.max_distance / dist3D, P);
                    Q.u = u; Q.v = v; Q.u_right = u - P.mbf * invz;
                    Q.radius = P.th * P.scale_factors[L];
                    Q.min_level = (int16_t)(L - 1); Q.max_level = (int16_t)L;
                    Q.flags = ORBM_Q_VALID;
                    const uint4* src = (const uint4*)(A.O.d_mp_desc + (size_t)r.desc_row * 32);
                    uint4* dst = (uint4*)(W.s_qdesc + (size_t)i * 32);
                    dst[0] = src[0];
                    dst[1] = src[1];
                }
            }
        }
    }
    W.s_q[i] = Q;
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

// MapPoint::Replace(A -> B) without its ComputeDistinctiveDescriptors (MapPoint.cc:286-334), on one lane
static __device__ void fn_replace(const FnArgs& A, const FnWork& W, int a, int b) {
    W.bad[a] = 1;
    A.O.d_replaced[a] = b;
    int r = W.head[a];
    W.head[a] = -1;
    while (r != -1) {
        const int nx = W.p_next[r], kf = W.p_obs[r].kf;
        const int row = A.V.d_kf[kf].mp_row0 + W.p_idx[r];   // (the init launch checked the record)
        if (fn_in_kf(W, b, kf)) A.O.d_kf_mp[row] = -1;       // EraseMapPointMatch
        else {
            A.O.d_kf_mp[row] = b;                            // ReplaceMapPointMatch, AddObservation
            fn_insert(W, b, r);
            W.nobs[b] += fn_weight(A, row);
        }
        r = nx;
    }
    if (A.O.d_found) A.O.d_found[b] += A.O.d_found[a];
    if (A.O.d_visible) A.O.d_visible[b] += A.O.d_visible[a];
}

// one workgroup of 256.  orb_smem = int[8]: wg_scan.inc's two sets of wave totals
static __global__ __launch_bounds__(256) void k_fn_apply(FnArgs A, int step) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const FnWork W = fn_work(A);
    const int tid = threadIdx.x;
    const int32_t* list;
    int n_list, call;
    const int kf = fn_step(A, W, step, &list, &n_list, &call);
    uint32_t bad = 0;
    int it = 0;
    // the survivors of the call before this one: what the refresh said of them
    if (step > 0)
        for (int j = tid; j < A.cap_q; j += 256)
            if (W.r_status[j] & ORBM_REFRESH_OVERFLOW) bad |= ORBM_FUSENB_REFRESH_OVERFLOW;
    // the turns with bestDist <= TH_LOW, in list order -> s_dist[0 .. n_turn)
    int n_turn = 0;
    if (kf >= 0)
        for (int c0 = 0; c0 < n_list; c0 += 256, it++) {
            const int i = c0 + tid;
            const bool keep = i < n_list && W.s_match[i] >= 0;
            int tot;
            const int at = n_turn + wg_scan_ballot<4>(keep, scan, it, &tot);
            if (keep) W.s_dist[at] = i;
            n_turn += tot;
        }
    __threadfence();
    __syncthreads();

    if (tid == 0) {
        int n_surv = 0;
        if (kf >= 0) {
            int row0, nf, drow0, n_events = W.hdr[FN_H_NEV], n_fused = 0;
            fn_kf_rows(A, kf, &row0, &nf, &drow0);   // (the gather flagged a key frame whose rows cannot be used: then nothing matched)
            auto survivor = [&](int p) {
                if (W.surv_step[p] != step + 1) { W.surv_step[p] = step + 1; W.surv[n_surv++] = p; }
            };
            for (int t = 0; t < n_turn; t++) {
                const int i = ld_relaxed(&W.s_dist[t]), m = W.s_match[i];
                const int p = fn_point(A, list[i], &bad);
                if (p < 0 || m >= nf || W.bad[p] || fn_in_kf(W, p, kf)) continue;   // :1677-1696 at the point's turn
                if (n_events >= A.O.cap_events) {   // the turn is not applied and the walk ends
                    bad |= ORBM_FUSENB_EVENT_OVERFLOW;
                    W.hdr[FN_H_STOP] = 1;
                    break;
                }
                const int q = fn_point(A, A.O.d_kf_mp[row0 + m], &bad);   // pKF->GetMapPoint(bestIdx), live
                int kind;
                if (q >= 0) {
                    if (W.bad[q]) kind = ORBM_FUSENB_EV_NOOP_BAD;
                    else if (q == p) kind = ORBM_FUSENB_EV_NOOP_SAME;
                    else if (W.nobs[q] > W.nobs[p]) { kind = ORBM_FUSENB_EV_LIST_POINT_REPLACED; fn_replace(A, W, p, q); survivor(q); }
                    else { kind = ORBM_FUSENB_EV_KF_POINT_REPLACED; fn_replace(A, W, q, p); survivor(p); }
                } else {
                    kind = ORBM_FUSENB_EV_ADD;
                    const int r = W.hdr[FN_H_POOL]++;   // (one record per event at the most: the pool has cap_events spare records)
                    orbm_observation o;
                    o.kf = kf; o.desc_row = drow0 + m; o.flags = 0;
                    W.p_obs[r] = o;
                    W.p_idx[r] = m;
                    fn_insert(W, p, r);
                    W.nobs[p] += fn_weight(A, row0 + m);
                    A.O.d_kf_mp[row0 + m] = p;
                }
                orbm_fusenb_event ev;
                ev.call = call; ev.kf = kf; ev.list_index = i; ev.point = p; ev.feature = m; ev.other = q; ev.kind = kind; ev.reserved = 0;
                A.O.d_events[n_events++] = ev;
                n_fused++;
            }
            W.hdr[FN_H_NEV] = n_events;
            A.O.d_nfused[call] = n_fused;
        }
        W.hdr[FN_H_NSURV] = n_surv;
    }
    __threadfence();
    __syncthreads();

    // the survivors that are still good, as a CSR of their own: a count per survivor, a scan, the rows in list (= rank) order
    const int n_surv = ld_relaxed(&W.hdr[FN_H_NSURV]);
    int run = 0;
    for (int c0 = 0; c0 < A.cap_q; c0 += 256, it++) {
        const int j = c0 + tid;
        int p = -1, cnt = 0;
        if (j < n_surv) {
            p = ld_relaxed(&W.surv[j]);
            if (W.bad[p]) p = -1;   // replaced again later in the call: ComputeDistinctiveDescriptors returns at once
            else for (int r = ld_relaxed(&W.head[p]); r != -1; r = ld_relaxed(&W.p_next[r])) cnt++;
        }
        int tot;
        int at = run + wg_scan_value<4>(cnt, scan, it, &tot);
        run += tot;
        if (j < A.cap_q) {
            W.r_start[j] = at;
            if (j == A.cap_q - 1) W.r_start[A.cap_q] = run;
            if (p >= 0) {
                orbm_map_point mp = A.V.d_mp[p];
                mp.flags = ORBM_MP_VALID;
                W.r_mp[j] = mp;
                for (int r = ld_relaxed(&W.head[p]); r != -1; r = ld_relaxed(&W.p_next[r])) {
                    orbm_observation o;
                    o.kf = ld_relaxed(&W.p_obs[r].kf);
                    o.desc_row = ld_relaxed(&W.p_obs[r].desc_row);
                    o.flags = ld_relaxed(&W.p_obs[r].flags);
                    W.r_obs[at++] = o;
                }
            } else W.r_mp[j].flags = 0;
        }
    }
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

// ------------------------------------------------------------------------------------------------ LocalMapping.cc:1015-1038
// one workgroup of 256: the first occurrence of every good point over the targets' rows (the least position wins an integer atomicMin), then
// the stable compaction in (target, feature) order
static __global__ __launch_bounds__(256) void k_fn_candidates(FnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const FnWork W = fn_work(A);
    const int tid = threadIdx.x;
    if (W.hdr[FN_H_STOP] || (A.P.flags & ORBM_FUSENB_ABORT_BA)) return;   // (the counts are zero)
    const int nt = W.hdr[FN_H_NT], cf = A.I.cap_feat;
    uint32_t bad = 0;
    for (int t = 0; t < nt; t++) {
        int row0, nf, drow0;
        fn_kf_rows(A, A.O.d_targets[t], &row0, &nf, &drow0);
        for (int i = tid; i < nf; i += 256) {
            const int q = fn_point(A, A.O.d_kf_mp[row0 + i], &bad);
            if (q >= 0 && !W.bad[q]) atomicMin(&W.mark[q], t * cf + i);
        }
    }
    __threadfence();
    __syncthreads();
    int run = 0, it = 0;
    for (int t = 0; t < nt; t++) {
        int row0, nf, drow0;
        fn_kf_rows(A, A.O.d_targets[t], &row0, &nf, &drow0);
        for (int c0 = 0; c0 < nf; c0 += 256, it++) {
            const int i = c0 + tid;
            uint32_t ignore = 0;
            const int q = i < nf ? fn_point(A, A.O.d_kf_mp[row0 + i], &ignore) : -1;
            const bool keep = q >= 0 && !W.bad[q] && ld_relaxed(&W.mark[q]) == t * cf + i;
            int tot;
            const int at = run + wg_scan_ballot<4>(keep, scan, it, &tot);
            if (keep && at < A.O.cap_candidates) A.O.d_candidates[at] = q;
            run += tot;
        }
    }
    if (run > A.O.cap_candidates) bad |= ORBM_FUSENB_CANDIDATE_OVERFLOW;
    if (tid == 0) {
        W.hdr[FN_H_NCAND_REQ] = run;
        W.hdr[FN_H_NCAND] = run < A.O.cap_candidates ? run : A.O.cap_candidates;
    }
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

// ------------------------------------------------------------------------------------------------ the outputs
// one workgroup of 256: d_sel = the current key frame's points as they now stand, not bad, first occurrence, padded with -1
static __global__ __launch_bounds__(256) void k_fn_sel(FnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const FnWork W = fn_work(A);
    const int tid = threadIdx.x, cur = A.P.current_kf;
    int row0 = 0, nf = 0, drow0;
    if (view_present(A.V, cur)) fn_kf_rows(A, cur, &row0, &nf, &drow0);
    uint32_t bad = 0;
    for (int i = tid; i < nf; i += 256) {
        const int q = fn_point(A, A.O.d_kf_mp[row0 + i], &bad);
        if (q >= 0) W.mark[q] = INT_MAX;
    }
    __threadfence();
    __syncthreads();
    for (int i = tid; i < nf; i += 256) {
        const int q = fn_point(A, A.O.d_kf_mp[row0 + i], &bad);
        if (q >= 0 && !W.bad[q]) atomicMin(&W.mark[q], i);
    }
    __threadfence();
    __syncthreads();
    int run = 0;
    for (int c0 = 0, it = 0; c0 < nf; c0 += 256, it++) {
        const int i = c0 + tid;
        uint32_t ignore = 0;
        const int q = i < nf ? fn_point(A, A.O.d_kf_mp[row0 + i], &ignore) : -1;
        const bool keep = q >= 0 && !W.bad[q] && ld_relaxed(&W.mark[q]) == i;
        int tot;
        const int at = run + wg_scan_ballot<4>(keep, scan, it, &tot);
        if (keep) A.O.d_sel[at] = q;
        run += tot;
    }
    for (int i = run + tid; i < A.I.cap_feat; i += 256) A.O.d_sel[i] = -1;
    if (tid == 0) W.hdr[FN_H_NSEL] = run;
    flag_or(&W.hdr[FN_H_FLAGS], bad);
}

static __device__ __forceinline__ int fn_live(const FnArgs& A, const FnWork& W, int p) {
    int n = 0;
    if (p < A.V.n_mp)
        for (int r = W.head[p]; r != -1; r = W.p_next[r]) n++;
    return n;
}

// (the three CSR kernels are obs_csr.inc's count / scan / place; orb_smem = its scratch, int[2][4])
static __global__ __launch_bounds__(256) void k_fn_count(FnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const FnWork W = fn_work(A);
    csr_count(fn_live(A, W, blockIdx.x * 256 + threadIdx.x), W.blk, (int*)orb_smem);
}

// one workgroup: the block totals scanned; the result words, overflow decided before anything is written
static __global__ __launch_bounds__(256) void k_fn_scan(FnArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const FnWork W = fn_work(A);
    int it = 0;
    const int run = csr_scan_blocks(W.blk, nblk, (int*)orb_smem, &it);
    uint32_t bad = 0;
    for (int j = threadIdx.x; j < A.cap_q; j += 256)   // the survivors of the last call
        if (W.r_status[j] & ORBM_REFRESH_OVERFLOW) bad |= ORBM_FUSENB_REFRESH_OVERFLOW;
    flag_or(&W.hdr[FN_H_FLAGS], bad);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        W.blk[nblk] = run;
        int32_t* R = A.O.d_result;
        R[ORBM_FUSENB_R_FLAGS] = (int32_t)(ld_relaxed((uint32_t*)&W.hdr[FN_H_FLAGS]) | (run > A.O.cap_obs_out ? ORBM_FUSENB_OBS_OVERFLOW : 0u));
        R[ORBM_FUSENB_R_N_TARGETS] = W.hdr[FN_H_NT];
        R[ORBM_FUSENB_R_N_TARGETS_REQUIRED] = W.hdr[FN_H_NT_REQ];
        R[ORBM_FUSENB_R_N_CANDIDATES] = W.hdr[FN_H_NCAND];
        R[ORBM_FUSENB_R_N_CANDIDATES_REQUIRED] = W.hdr[FN_H_NCAND_REQ];
        R[ORBM_FUSENB_R_N_EVENTS] = W.hdr[FN_H_NEV];
        R[ORBM_FUSENB_R_N_OBS] = run;
        R[ORBM_FUSENB_R_N_SEL] = W.hdr[FN_H_NSEL];
    }
}

// grid x over the blocks of 256 points: the flags and nObs of every point; the merged CSR unless it overflows
static __global__ __launch_bounds__(256) void k_fn_write(FnArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const FnWork W = fn_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x, n_mp = A.V.n_mp;
    const bool fits = csr_total(W.blk, nblk) <= A.O.cap_obs_out;
    int at = csr_place(fn_live(A, W, g), W.blk, n_mp, fits, A.O.d_obs_start_out, (int*)orb_smem);
    if (g >= n_mp) return;
    const int nobs = W.nobs[g];
    uint32_t f = A.O.d_mp[g].flags;
    f = (f & ~ORBM_MP_HAS_OBS) | (nobs > 0 ? ORBM_MP_HAS_OBS : 0u) | (W.bad[g] ? ORBM_MP_BAD : 0u);
    A.O.d_mp[g].flags = f;
    if (A.O.d_mp_nobs) A.O.d_mp_nobs[g] = nobs;
    if (!fits) return;
    for (int r = W.head[g]; r != -1; r = W.p_next[r]) A.O.d_obs_out[at++] = W.p_obs[r];
}

// ------------------------------------------------------------------------------------------------ host
static bool fn_sizes_ok(int n_kf, int n_mp, int n_obs, int cap_feat, int cap_candidates, int cap_events) {
    return n_kf >= 0 && n_mp >= 0 && n_obs >= 0 && cap_feat >= 1 && cap_feat <= 65535 && cap_candidates >= 1 && cap_events >= 1 &&
           (long long)n_obs + cap_events <= INT_MAX;
}

extern "C" size_t orbm_fusenb_workspace_bytes(int n_kf, int n_mp, int n_obs, int cap_feat, int cap_candidates, int cap_events) {
    if (!fn_sizes_ok(n_kf, n_mp, n_obs, cap_feat, cap_candidates, cap_events)) return 0;
    FnWork W;
    return fn_work_layout(n_kf, n_mp, n_obs + cap_events, cap_feat, cap_feat > cap_candidates ? cap_feat : cap_candidates, nullptr, W);
}

extern "C" int orbm_search_in_neighbors(const orbm_localmap_view* view, const orbm_fusenb_in* in, const orbm_fusenb_params* params,
                                        const orbm_fusenb_out* out, void* d_work, void* stream) {
    if (!view || !in || !params || !out || !d_work) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    const orbm_fusenb_in& I = *in;
    const orbm_fusenb_out& O = *out;
    if (view_invalid(V, VIEW_ALL) || (!V.d_kf_by_order && V.n_kf) || misaligned16(d_work)) return ORB_E_INVALID;
    if (O.cap_targets < 1 || O.cap_targets > ORBM_FUSENB_MAX_TARGETS || O.cap_obs_out < 0 || O.n_desc_rows < 0 || I.n_kf_desc_rows < 0 || I.cap_conn < 1 ||
        !fn_sizes_ok(V.n_kf, V.n_mp, V.n_obs, I.cap_feat, O.cap_candidates, O.cap_events))
        return ORB_E_INVALID;
    if (params->nlevels < 1 || params->nlevels > 16) return ORB_E_INVALID;
    if ((V.n_kf && (!I.d_ckf || !I.d_pose || !I.d_ordered_kf || !I.d_n_ordered || !O.d_fuse_target)) ||
        (V.n_kf_mp_rows && (!I.d_feat || !I.d_kps || !I.d_u_right || !O.d_kf_mp)) || (I.n_kf_desc_rows && !I.d_kf_desc) ||
        (V.n_mp && (!O.d_mp || !O.d_replaced)) || (O.n_desc_rows && !O.d_mp_desc))
        return ORB_E_INVALID;
    if (!O.d_targets || !O.d_candidates || !O.d_nfused || !O.d_events || !O.d_sel || !O.d_obs_start_out || (!O.d_obs_out && O.cap_obs_out) ||
        !O.d_result)
        return ORB_E_INVALID;
    if (misaligned16(O.d_mp) || misaligned16(I.d_kf_desc) || misaligned16(O.d_mp_desc)) return ORB_E_INVALID;
    // orbm_refresh_map_points refuses null slabs: a map without descriptor rows has nothing to fuse with
    if (!I.d_kf_desc || !O.d_mp_desc) return ORB_E_INVALID;

    FnArgs A;
    A.V = V; A.I = I; A.P = *params; A.O = O; A.work = (unsigned char*)d_work;
    A.cap_q = I.cap_feat > O.cap_candidates ? I.cap_feat : O.cap_candidates;
    A.pool_n = V.n_obs + O.cap_events;
    FnWork W;
    fn_work_layout(V.n_kf, V.n_mp, A.pool_n, I.cap_feat, A.cap_q, A.work, W);
    orbm_fuse_params fp;
    fp.th_dist = ORBM_TH_LOW;
    fp.chi2_gate = 1;
    fp.grid = params->grid;
    orbm_refresh_params rp;
    rp.what = ORBM_REFRESH_DESCRIPTOR;
    rp.nlevels = params->nlevels;
    for (int i = 0; i < 16; i++) { fp.inv_level_sigma2[i] = params->inv_level_sigma2[i]; rp.scale_factors[i] = params->scale_factors[i]; }

    // (orbm_grid_build, orbm_fuse and orbm_refresh_map_points below test null pointers, cap_feat in 1..65535, cap_q >= 1, nlevels and the
    //  slabs' alignment: all of it is tested above or holds by the layout, so none of them refuses a call that got this far)
    hipStream_t st = (hipStream_t)stream;
    const int nblk = csr_blocks(V.n_mp);
    const int gp = nblk < 1 ? 1 : (nblk < 1024 ? nblk : 1024);
    hipLaunchKernelGGL(k_fn_clear, dim3(1), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_fn_init, dim3(gp), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_fn_targets, dim3(1), dim3(256), 0, st, A);
    for (int step = 0; step <= O.cap_targets; step++) {
        if (step == O.cap_targets) hipLaunchKernelGGL(k_fn_candidates, dim3(1), dim3(256), 32, st, A);
        hipLaunchKernelGGL(k_fn_gather, dim3((I.cap_feat + 255) / 256), dim3(256), 0, st, A, step);
        int rc = orbm_grid_build(W.s_kps, W.s_cnt + FN_C_NKP, 1, I.cap_feat, 1, &params->grid, W.s_gstart, W.s_gidx, stream);
        if (rc != ORB_OK) return rc;
        hipLaunchKernelGGL(k_fn_project, dim3((A.cap_q + 255) / 256), dim3(256), 0, st, A, step);
        rc = orbm_fuse(W.s_kps, W.s_desc, W.s_ur, W.s_cnt + FN_C_NKP, 1, I.cap_feat, W.s_gstart, W.s_gidx, W.s_q, W.s_qdesc, W.s_cnt + FN_C_NQ,
                       A.cap_q, 1, &fp, W.s_match, W.s_dist, W.s_cnt + FN_C_NF, stream);
        if (rc != ORB_OK) return rc;
        hipLaunchKernelGGL(k_fn_apply, dim3(1), dim3(256), 32, st, A, step);
        // (DESCRIPTOR alone reads neither the reference key frames nor the camera centres: any non-null pointer serves)
        rc = orbm_refresh_map_points(W.r_mp, A.cap_q, O.d_mp_desc, O.n_desc_rows, nullptr, 0, W.r_start, W.r_obs,
                                     (const orbm_refresh_point*)W.r_best, (const orbm_keyframe_center*)W.r_mp, V.n_kf, I.d_kf_desc,
                                     I.n_kf_desc_rows, &rp, W.r_best, W.r_status, stream);
        if (rc != ORB_OK) return rc;
    }
    hipLaunchKernelGGL(k_fn_sel, dim3(1), dim3(256), 32, st, A);
    if (nblk) hipLaunchKernelGGL(k_fn_count, dim3(nblk), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_fn_scan, dim3(1), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL(k_fn_write, dim3(nblk < 1 ? 1 : nblk), dim3(256), 32, st, A, nblk);
    return launch_status();
}
