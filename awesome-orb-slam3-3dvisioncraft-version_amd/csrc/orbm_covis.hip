// orbm_covis.hip — the covisibility graph on the device map for gfx950 (include/orbhip.h "Covisibility graph"): KeyFrame::UpdateConnections
// with AddConnection / UpdateBestCovisibles, and the connection part of KeyFrame::SetBadFlag with EraseConnection.
//
//   k_covis_clear       grid-wide, zeroes the counters, the modes and the flag word (a kernel rather than a memset node: DESIGN.md "Local map").
//   k_covis_count       one workgroup per (list entry, chunk of 256 features): a lane walks its point's records and adds 1 to the observer's
//                       word of the entry's counter row.  The counts depend on the observation graph only, which the call does not change, so
//                       every list entry is counted before any is applied.
//   k_covis_apply       one workgroup, serial over the list (every update changes the rows the next one reads).  Per entry: the counter over the
//                       pointer ranks (size, pKFmax as an LDS atomicMax of count << 32 | ~rank, the front of the ordered list as count << 32 |
//                       rank over the entries >= 15), the own row as an ordered compaction in rank order (wg_scan.inc), then one wave per
//                       AddConnection target: it scans the target's row for the key and overwrites or appends.  No list is rebuilt here: a touched key frame gets a
//                       mode (own / full) and the rebuild runs once at the end, which is exact because only a key frame's last rebuild is
//                       visible and an AddConnection that does not rebuild does not change the map either.
//   k_covis_erase       one workgroup, serial over the cull events, one wave per key frame in the erased row: it loses its entry of the erased
//                       key frame (the entries behind move up) and is stamped with the event's index, the bad filter of that moment.
//   k_covis_rebuild     one workgroup per touched key frame: ranks its row by counting on the unique key (weight, pointer rank) and writes the
//                       two ordered rows and covis[10].
//
// Workspace (each section padded to 16 bytes): hdr int32[8] | cnt int32[n_list][n_kf] | mode uint32[n_kf] | stamp int32[n_kf] |
// erased_at int32[n_kf] | rank_of int32[n_kf].
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "wg_scan.inc"
#include "workspace.inc"

#define COVIS_WG 256
constexpr int COVIS_NW = COVIS_WG / 64;
constexpr int COVIS_TH = 15;   // KeyFrame.cc:470

struct CovisWork {
    int32_t *hdr, *cnt;
    uint32_t* mode;
    int32_t *stamp, *erased_at, *rank_of;
};
enum { COVIS_HDR_WORDS = 8, COVIS_HDR_FLAGS = 0 };
enum : uint32_t { COVIS_MODE_NONE = 0, COVIS_MODE_OWN = 1, COVIS_MODE_FULL = 2, COVIS_MODE_CLEARED = 3 };

// The workspace, listed once.  -> its bytes (a multiple of 16)
static __host__ __device__ __forceinline__ size_t covis_work_layout(int n_kf, int n_list, unsigned char* base, CovisWork& W) {
    const size_t nk = (size_t)n_kf;
    WsCursor c{base, 16, 0};
    W.hdr = c.take<int32_t>(COVIS_HDR_WORDS);
    W.cnt = c.take<int32_t>((size_t)n_list * nk);
    W.mode = c.take<uint32_t>(nk);
    W.stamp = c.take<int32_t>(nk);
    W.erased_at = c.take<int32_t>(nk);
    W.rank_of = c.take<int32_t>(nk);
    return c.off;
}

struct CovisArgs {
    orbm_localmap_view V;
    orbm_covis_store S;
    orbm_covis_out O;
    orbm_covis_keyframe* ckf;
    orbm_localmap_keyframe* kf;   // the writable view.d_kf
    const int32_t* list;
    const orbm_cull_event* events;
    const int32_t* n_events;
    const uint8_t* kf_erased;
    unsigned char* work;
    int n_list, cap_events, erase;
    uint32_t init_kf_id;
};

static __device__ __forceinline__ CovisWork covis_work(const CovisArgs& A) {
    CovisWork W;
    covis_work_layout(A.V.n_kf, A.n_list, A.work, W);
    return W;
}

// the usable length of row k: a stored count outside [0, cap_conn] is a bad index (ld_relaxed: an apply kernel changed it earlier in its launch)
static __device__ __forceinline__ int covis_row_len(const CovisArgs& A, int k, uint32_t* bad) {
    const int n = ld_relaxed(&A.S.d_n_conn[k]);
    if (n < 0 || n > A.S.cap_conn) { *bad |= ORBM_COVIS_BAD_INDEX; return n < 0 ? 0 : A.S.cap_conn; }
    return n;
}

static __global__ __launch_bounds__(256) void k_covis_clear(CovisArgs A) {
    const CovisWork W = covis_work(A);
    const size_t n_cnt = (size_t)A.n_list * (size_t)A.V.n_kf, n_kf = (size_t)A.V.n_kf;
    const size_t n = n_cnt > COVIS_HDR_WORDS ? n_cnt : COVIS_HDR_WORDS;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (i < COVIS_HDR_WORDS) W.hdr[i] = 0;
        if (i < n_cnt) W.cnt[i] = 0;
        if (i < n_kf) { W.mode[i] = COVIS_MODE_NONE; W.stamp[i] = 0; }
    }
}

// grid (chunks of 256 features, n_list)
static __global__ __launch_bounds__(256) void k_covis_count(CovisArgs A) {
    const CovisWork W = covis_work(A);
    const orbm_localmap_view& V = A.V;
    const int l = blockIdx.y;
    const int a = A.list[l];
    uint32_t bad = 0;
    if (!view_present(A.V, a)) return;   // (the apply kernel flags it)
    int row0, nf;
    if (!view_rows(V, a, &row0, &nf)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((uint32_t*)&W.hdr[COVIS_HDR_FLAGS], (uint32_t)ORBM_COVIS_BAD_INDEX);
        return;
    }
    const uint32_t id = A.ckf[a].id;
    const int32_t map_id = A.ckf[a].map_id;
    int32_t* cnt = W.cnt + (size_t)l * (size_t)V.n_kf;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nf; i += gridDim.x * 256) {
        const int p = V.d_kf_mp[row0 + i];
        if (p == -1) continue;
        if (!view_point_ok(V, p)) { bad |= ORBM_COVIS_BAD_INDEX; continue; }
        if (V.d_mp[p].flags & ORBM_MP_BAD) continue;
        int s, e;
        if (!view_obs_range(V, p, &s, &e)) { bad |= ORBM_COVIS_BAD_INDEX; continue; }
        int before = -1;
        for (int o = s; o < e; o++) {
            const orbm_observation r = V.d_obs[o];
            const bool same_entry = (r.flags & ORBM_OBS_RIGHT) && o > s && before == r.kf;
            before = r.kf;
            if (same_entry) continue;
            if (!view_present(A.V, r.kf)) { bad |= ORBM_COVIS_BAD_INDEX; continue; }
            if (A.ckf[r.kf].id == id || (V.d_kf[r.kf].flags & ORBM_LM_KF_BAD) || A.ckf[r.kf].map_id != map_id) continue;   // KeyFrame.cc:455
            atomicAdd(&cnt[r.kf], 1);
        }
    }
    if (bad) atomicOr((uint32_t*)&W.hdr[COVIS_HDR_FLAGS], bad);
}

// LDS of the two one-workgroup kernels: best uint64[2] | words
enum { COVIS_S_N = 0, COVIS_S_NGE = 1, COVIS_S_FLAGS = 2, COVIS_S_OVER = 3, COVIS_S_WT = 4, COVIS_S_WORDS = 4 + 2 * COVIS_NW };
constexpr size_t COVIS_LDS = 16 + COVIS_S_WORDS * 4;

// rank_of[k] = the rank of key frame k in d_kf_by_order (the least, where it is listed twice), INT_MAX where it has none; the caller's launch is
// one workgroup.  Also clears the erase's stamps.
static __device__ __forceinline__ void covis_ranks(const CovisArgs& A, const CovisWork& W, uint32_t* bad) {
    const int n_kf = A.V.n_kf;
    for (int i = threadIdx.x; i < n_kf; i += COVIS_WG) {
        W.rank_of[i] = INT_MAX;
        W.erased_at[i] = INT_MAX;
        if (A.erase) { W.mode[i] = COVIS_MODE_NONE; W.stamp[i] = 0; }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_kf; r += COVIS_WG) {
        const int k = A.V.d_kf_by_order[r];
        if (k < 0 || k >= n_kf) { *bad |= ORBM_COVIS_BAD_INDEX; continue; }
        atomicMin(&W.rank_of[k], r);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_kf; i += COVIS_WG)
        if (ld_relaxed(&W.rank_of[i]) == INT_MAX && (A.V.d_kf[i].flags & ORBM_LM_KF_PRESENT)) *bad |= ORBM_COVIS_BAD_INDEX;
}

// the key frame at rank r and its count in `cnt`: 0 where the rank names nothing usable (out of range, or a second listing of a key frame)
static __device__ __forceinline__ int covis_count_at(const CovisArgs& A, const CovisWork& W, const int32_t* cnt, int r, int* k) {
    *k = -1;
    if (r >= A.V.n_kf) return 0;
    const int v = A.V.d_kf_by_order[r];
    if (v < 0 || v >= A.V.n_kf || ld_relaxed(&W.rank_of[v]) != r) return 0;
    *k = v;
    return cnt[v];
}

// the position of key `key` in row b (wave-uniform), or -1; all 64 lanes call
static __device__ __forceinline__ int covis_find(const CovisArgs& A, int b, int nb, int key) {
    const orbm_covis_entry* row = A.S.d_conn + (size_t)b * A.S.cap_conn;
    const int lane = threadIdx.x & 63;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long m = __ballot(j < nb && ld_relaxed(&row[j].kf) == key);
        if (m) return j0 + __ffsll((long long)m) - 1;
    }
    return -1;
}

static __global__ __launch_bounds__(COVIS_WG) void k_covis_apply(CovisArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    unsigned long long* best = (unsigned long long*)orb_smem;   // [2]
    int* sh = (int*)(orb_smem + 16);                             // [COVIS_S_WORDS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CovisWork W = covis_work(A);
    const int n_kf = A.V.n_kf, cap = A.S.cap_conn;
    uint32_t bad = 0;
    if (tid == 0) { sh[COVIS_S_FLAGS] = 0; sh[COVIS_S_OVER] = INT_MAX; }
    covis_ranks(A, W, &bad);
    int n_child = 0;   // lane 0's

    for (int l = 0; l < A.n_list; l++) {
        const int a = A.list[l];
        if (!view_present(A.V, a)) {
            bad |= ORBM_COVIS_BAD_INDEX;
            if (tid == 0) { A.O.d_nmax[l] = 0; A.O.d_kfmax[l] = -1; A.O.d_n_counter[l] = 0; }
            continue;
        }
        const int32_t* cnt = W.cnt + (size_t)l * (size_t)n_kf;
        if (tid == 0) { best[0] = 0; best[1] = 0; sh[COVIS_S_N] = 0; sh[COVIS_S_NGE] = 0; }
        __syncthreads();
        // ---- KeyFrame.cc:466-486: the counter in pointer order: its size, pKFmax (the first greatest), the entries >= th
        for (int r0 = 0; r0 < n_kf; r0 += COVIS_WG) {
            int k;
            const int r = r0 + tid, c = covis_count_at(A, W, cnt, r, &k);
            const unsigned long long bh = __ballot(c > 0), bg = __ballot(c >= COVIS_TH);
            if (c > 0) atomicMax(&best[0], ((unsigned long long)c << 32) | (uint32_t)~r);
            if (c >= COVIS_TH) atomicMax(&best[1], ((unsigned long long)c << 32) | (uint32_t)r);   // the front: ties by rank DESCENDING
            if (lane == 0 && bh) { atomicAdd(&sh[COVIS_S_N], __popcll(bh)); atomicAdd(&sh[COVIS_S_NGE], __popcll(bg)); }
        }
        __syncthreads();
        const int n_counter = sh[COVIS_S_N], n_ge = sh[COVIS_S_NGE];
        const unsigned long long b0 = best[0], b1 = best[1];
        const int nmax = (int)(b0 >> 32), rmax = n_counter ? (int)~(uint32_t)b0 : 0;
        const int kfmax = n_counter ? A.V.d_kf_by_order[rmax] : -1;
        const int front = n_ge ? A.V.d_kf_by_order[(int)(uint32_t)b1] : kfmax;
        if (tid == 0) { A.O.d_nmax[l] = nmax; A.O.d_kfmax[l] = kfmax; A.O.d_n_counter[l] = n_counter; }
        if (n_counter == 0) { __syncthreads(); continue; }   // :462: nothing changes

        // ---- :534: mConnectedKeyFrameWeights = KFcounter, the whole counter in pointer order
        orbm_covis_entry* row = A.S.d_conn + (size_t)a * cap;
        int base = 0;
        for (int r0 = 0, it = 0; r0 < n_kf; r0 += COVIS_WG, it++) {
            int k;
            const int r = r0 + tid, c = covis_count_at(A, W, cnt, r, &k);
            int tot;
            const int pos = base + wg_scan_ballot<COVIS_NW>(c > 0, sh + COVIS_S_WT, it, &tot);
            if (c > 0 && pos < cap) { orbm_covis_entry en; en.kf = k; en.weight = c; row[pos] = en; }
            base += tot;
        }
        if (tid == 0) {
            A.S.d_n_conn[a] = n_counter < cap ? n_counter : cap;
            W.mode[a] = COVIS_MODE_OWN;
            W.stamp[a] = l;
            if (n_counter > cap) { atomicOr((uint32_t*)&sh[COVIS_S_FLAGS], (uint32_t)ORBM_COVIS_OVERFLOW); atomicMin(&sh[COVIS_S_OVER], a); }
            // ---- :537-545
            if ((A.ckf[a].flags & ORBM_COVIS_KF_FIRST_CONNECTION) && A.ckf[a].id != A.init_kf_id) {
                A.kf[a].parent = front;
                A.ckf[a].flags &= ~ORBM_COVIS_KF_FIRST_CONNECTION;
                orbm_covis_child_event ev; ev.child = a; ev.parent = front;
                A.O.d_child_events[n_child++] = ev;
            }
        }
        // ---- :480-493: AddConnection(this, count) of every entry >= th, or of pKFmax alone: one wave per target
        for (int r0 = wv * 64; r0 < n_kf; r0 += COVIS_WG) {
            int k;
            const int r = r0 + lane, c = covis_count_at(A, W, cnt, r, &k);
            unsigned long long m = __ballot(n_ge ? c >= COVIS_TH : (c > 0 && r == rmax));
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int b = __shfl(k, j, 64), w = __shfl(c, j, 64);
                const int nb = covis_row_len(A, b, &bad);
                const int at = covis_find(A, b, nb, a);
                __builtin_amdgcn_wave_barrier();   // every lane has read the row's length before lane 0 changes it
                if (lane == 0) {
                    orbm_covis_entry* rb = A.S.d_conn + (size_t)b * cap;
                    if (at >= 0) {
                        if (rb[at].weight != w) { rb[at].weight = w; W.mode[b] = COVIS_MODE_FULL; }   // the same weight: no rebuild (:236)
                    } else if (nb < cap) {
                        orbm_covis_entry en; en.kf = a; en.weight = w;
                        rb[nb] = en;
                        A.S.d_n_conn[b] = nb + 1;
                        W.mode[b] = COVIS_MODE_FULL;
                    } else {
                        atomicOr((uint32_t*)&sh[COVIS_S_FLAGS], (uint32_t)ORBM_COVIS_OVERFLOW);
                        atomicMin(&sh[COVIS_S_OVER], b);
                    }
                }
            }
        }
        __syncthreads();   // the next entry reads these rows, and lane 0 rewrites the LDS words
    }

    if (bad) atomicOr((uint32_t*)&sh[COVIS_S_FLAGS], bad);
    __syncthreads();
    if (tid == 0) {
        A.O.d_n_child_events[0] = n_child;
        A.O.d_overflow_kf[0] = sh[COVIS_S_OVER] == INT_MAX ? -1 : sh[COVIS_S_OVER];
        A.O.d_flags[0] = (uint32_t)sh[COVIS_S_FLAGS] | (uint32_t)W.hdr[COVIS_HDR_FLAGS];
    }
}

static __global__ __launch_bounds__(COVIS_WG) void k_covis_erase(CovisArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* sh = (int*)(orb_smem + 16);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CovisWork W = covis_work(A);
    const int cap = A.S.cap_conn;
    uint32_t bad = 0;
    if (tid == 0) sh[COVIS_S_FLAGS] = 0;
    covis_ranks(A, W, &bad);
    int ne = A.n_events[0];
    if (ne < 0 || ne > A.cap_events) { bad |= ORBM_COVIS_BAD_INDEX; ne = ne < 0 ? 0 : A.cap_events; }
    // when each key frame goes bad: the first event that erases it
    for (int e = tid; e < ne; e += COVIS_WG) {
        const int k = A.events[e].kf;
        if (view_present(A.V, k) && (!A.kf_erased || A.kf_erased[k])) atomicMin(&W.erased_at[k], e);
    }
    __syncthreads();
    for (int e = 0; e < ne; e++) {
        const int k = A.events[e].kf;
        if (!view_present(A.V, k)) { bad |= ORBM_COVIS_BAD_INDEX; continue; }
        if (A.kf_erased && !A.kf_erased[k]) continue;   // deferred: SetBadFlag returned before the loop
        const int nk = covis_row_len(A, k, &bad);
        const orbm_covis_entry* rk = A.S.d_conn + (size_t)k * cap;
        // ---- KeyFrame.cc:675-678: EraseConnection(this) of every key frame in the map, one wave per target
        for (int j = wv; j < nk; j += COVIS_NW) {
            const int b = ld_relaxed(&rk[j].kf);
            if (b == k) continue;
            if (b < 0 || b >= A.V.n_kf) { bad |= ORBM_COVIS_BAD_INDEX; continue; }
            const int nb = covis_row_len(A, b, &bad);
            const int at = covis_find(A, b, nb, k);
            if (at < 0) continue;   // :799: nothing erased, nothing rebuilt
            orbm_covis_entry* rb = A.S.d_conn + (size_t)b * cap;
            for (int j0 = at; j0 < nb - 1; j0 += 64) {   // mConnectedKeyFrameWeights.erase: the entries behind move up, in order
                const int j = j0 + lane;
                orbm_covis_entry en; en.kf = 0; en.weight = 0;
                if (j < nb - 1) { en.kf = ld_relaxed(&rb[j + 1].kf); en.weight = ld_relaxed(&rb[j + 1].weight); }
                __builtin_amdgcn_wave_barrier();   // every lane has read its successor before any is overwritten
                if (j < nb - 1) rb[j] = en;
                __builtin_amdgcn_wave_barrier();
            }
            __builtin_amdgcn_wave_barrier();   // every lane has read the row's length before lane 0 changes it
            if (lane == 0) {
                A.S.d_n_conn[b] = nb - 1;
                W.mode[b] = COVIS_MODE_FULL;
                W.stamp[b] = e;
            }
        }
        __syncthreads();
        if (tid == 0) {   // :696-697
            A.S.d_n_conn[k] = 0;
            W.mode[k] = COVIS_MODE_CLEARED;
        }
        __syncthreads();
    }
    if (bad) atomicOr((uint32_t*)&sh[COVIS_S_FLAGS], bad);
    __syncthreads();
    if (tid == 0) A.O.d_flags[0] = (uint32_t)sh[COVIS_S_FLAGS];
}

// isBad() of key frame x as the rebuild of key frame k sees it
static __device__ __forceinline__ bool covis_is_bad(const CovisArgs& A, const CovisWork& W, int x, int k) {
    if (A.erase) {
        const int ea = W.erased_at[x];
        if (ea != INT_MAX) return ea < W.stamp[k];
    }
    return (A.V.d_kf[x].flags & ORBM_LM_KF_BAD) != 0;
}

// one workgroup per key frame
static __global__ __launch_bounds__(COVIS_WG) void k_covis_rebuild(CovisArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* sh = (int*)(orb_smem + 16);
    const int tid = threadIdx.x, lane = tid & 63;
    const CovisWork W = covis_work(A);
    const int k = blockIdx.x, cap = A.S.cap_conn;
    const uint32_t mode = W.mode[k];
    if (mode == COVIS_MODE_NONE) return;
    if (mode == COVIS_MODE_CLEARED) {
        if (tid == 0) A.S.d_n_ordered[k] = 0;
        if (tid < 10) A.kf[k].covis[tid] = -1;
        return;
    }
    uint32_t bad = 0;
    const orbm_covis_entry* row = A.S.d_conn + (size_t)k * cap;
    int n = A.S.d_n_conn[k];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    if (tid == 0) { sh[COVIS_S_N] = 0; sh[COVIS_S_FLAGS] = 0; }
    __syncthreads();
    // ---- the ordered rows: an entry's place is the number of listed entries with a greater (weight, pointer rank)
    int own_nmax = 0, own_kfmax = -1;
    if (mode == COVIS_MODE_OWN) { const int l = W.stamp[k]; own_nmax = A.O.d_nmax[l]; own_kfmax = A.O.d_kfmax[l]; }
    const size_t o0 = (size_t)k * cap;
    for (int i0 = 0; i0 < n; i0 += COVIS_WG) {
        const int i = i0 + tid;
        bool listed = false;
        orbm_covis_entry en; en.kf = -1; en.weight = 0;
        long long key = 0;
        if (i < n) {
            en = row[i];
            if (!view_present(A.V, en.kf) || W.rank_of[en.kf] == INT_MAX) bad |= ORBM_COVIS_BAD_INDEX;
            else {
                listed = mode == COVIS_MODE_OWN ? (own_nmax >= COVIS_TH ? en.weight >= COVIS_TH : en.kf == own_kfmax)   // :480-493, no isBad()
                                                : !covis_is_bad(A, W, en.kf, k);                                       // :254
                key = ((long long)en.weight << 32) | (long long)W.rank_of[en.kf];
            }
        }
        if (listed) {
            int place = 0;
            for (int j = 0; j < n; j++) {
                const orbm_covis_entry ej = row[j];
                if (!view_present(A.V, ej.kf) || W.rank_of[ej.kf] == INT_MAX) continue;
                const bool lj = mode == COVIS_MODE_OWN ? (own_nmax >= COVIS_TH ? ej.weight >= COVIS_TH : ej.kf == own_kfmax)
                                                       : !covis_is_bad(A, W, ej.kf, k);
                place += lj && (((long long)ej.weight << 32) | (long long)W.rank_of[ej.kf]) > key ? 1 : 0;
            }
            A.S.d_ordered_kf[o0 + place] = en.kf;
            A.S.d_ordered_w[o0 + place] = en.weight;
            if (place < 10) A.kf[k].covis[place] = en.kf;
        }
        const unsigned long long bl = __ballot(listed);
        if (lane == 0 && bl) atomicAdd(&sh[COVIS_S_N], __popcll(bl));
    }
    if (bad) atomicOr((uint32_t*)&sh[COVIS_S_FLAGS], bad);
    __syncthreads();
    const int n_listed = sh[COVIS_S_N];
    if (tid == 0) {
        A.S.d_n_ordered[k] = n_listed;
        if (sh[COVIS_S_FLAGS]) atomicOr(A.O.d_flags, (uint32_t)sh[COVIS_S_FLAGS]);
    }
    if (tid < 10 && tid >= n_listed) A.kf[k].covis[tid] = -1;
}

// ------------------------------------------------------------------------------------------------ host
extern "C" size_t orbm_covis_workspace_bytes(int n_kf, int n_list) {
    if (n_kf < 0 || n_list < 0) return 0;
    CovisWork W;
    return covis_work_layout(n_kf, n_list, nullptr, W);
}

// `need`: the view's tables the entry point reads (the erase reads the key frames only)
static bool covis_invalid(const orbm_localmap_view& V, unsigned need, const orbm_covis_store& S, const void* d_kf, const void* d_work) {
    if (view_invalid(V, need) || S.cap_conn < 1) return true;
    if (V.n_kf && (!d_kf || !V.d_kf_by_order || !S.d_conn || !S.d_n_conn || !S.d_ordered_kf || !S.d_ordered_w || !S.d_n_ordered)) return true;
    return ((uintptr_t)S.d_conn & 7u) != 0 || misaligned16(d_work);   // d_conn: 8-byte entries
}

extern "C" int orbm_update_connections(const orbm_localmap_view* view, const orbm_covis_store* store, orbm_covis_keyframe* d_ckf,
                                       orbm_localmap_keyframe* d_kf, const int32_t* d_list, int n_list, uint32_t init_kf_id,
                                       const orbm_covis_out* out, void* d_work, void* stream) {
    if (!view || !store || !out || !d_work || n_list < 0) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    if (covis_invalid(V, VIEW_ALL, *store, d_kf, d_work) || (!d_ckf && V.n_kf)) return ORB_E_INVALID;
    if ((!d_list && n_list) || !out->d_n_child_events || !out->d_overflow_kf || !out->d_flags) return ORB_E_INVALID;
    if (n_list && (!out->d_child_events || !out->d_nmax || !out->d_kfmax || !out->d_n_counter)) return ORB_E_INVALID;
    if (n_list == 0) return ORB_OK;
    CovisArgs A{};
    A.V = V; A.S = *store; A.O = *out; A.ckf = d_ckf; A.kf = d_kf; A.list = d_list; A.n_list = n_list; A.init_kf_id = init_kf_id;
    A.work = (unsigned char*)d_work; A.erase = 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t n_cnt = (size_t)n_list * (size_t)V.n_kf;
    const int gc = (int)((n_cnt + 255) / 256 < 1024 ? (n_cnt + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_covis_clear, dim3(gc > 0 ? gc : 1), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_covis_count, dim3(8, n_list), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_covis_apply, dim3(1), dim3(COVIS_WG), COVIS_LDS, st, A);
    if (V.n_kf) hipLaunchKernelGGL(k_covis_rebuild, dim3(V.n_kf), dim3(COVIS_WG), COVIS_LDS, st, A);
    return launch_status();
}

extern "C" int orbm_erase_connections(const orbm_localmap_view* view, const orbm_covis_store* store, orbm_localmap_keyframe* d_kf,
                                      const orbm_cull_event* d_events, const int32_t* d_n_events, const uint8_t* d_kf_erased, int cap_events,
                                      const orbm_covis_out* out, void* d_work, void* stream) {
    if (!view || !store || !out || !d_work || cap_events < 0) return ORB_E_INVALID;
    if (covis_invalid(*view, VIEW_KF, *store, d_kf, d_work) || !d_n_events || (!d_events && cap_events) || !out->d_flags) return ORB_E_INVALID;
    CovisArgs A{};
    A.V = *view; A.S = *store; A.O = *out; A.kf = d_kf; A.events = d_events; A.n_events = d_n_events; A.kf_erased = d_kf_erased;
    A.cap_events = cap_events; A.n_list = 0; A.work = (unsigned char*)d_work; A.erase = 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_covis_erase, dim3(1), dim3(COVIS_WG), COVIS_LDS, st, A);
    if (view->n_kf) hipLaunchKernelGGL(k_covis_rebuild, dim3(view->n_kf), dim3(COVIS_WG), COVIS_LDS, st, A);
    return launch_status();
}
