// bowdb_query.hip — place recognition on gfx950: KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:785-897) and
// KeyFrameDatabase::DetectNBestCandidates (:614-782) with L1Scoring::score (DBoW2 ScoringObject.cpp:23-68), over the device-resident key-frame
// database of include/orbhip.h "Place recognition".
//
// Form: dense.  The reference's inverted file exists so that a CPU never touches key frames that share nothing; here every query streams the
// sorted BowVector rows of all slots, which is deterministic and keeps add / erase a plain row write.  Per query, on the one stream:
//
//   k_mark   (N-best) stamps the slots of the query's conn list.
//   k_share  one wave per row, lanes stride the row, the query's words in LDS (binary search): words, first common word; last_query = id for
//            the listed slots; per-wave partial maxCommonWords / list size go to the query's scalars with integer atomics.
//   k_score  one wave per row with words > minCommonWords: the common-word terms are computed lane-parallel per 64 row entries and added in
//            ascending word order on broadcasts, every lane running the same serial double sum (the price of bit-identity); score written, the
//            slot appended to the scored list (the list's order is arbitrary, nothing below depends on it).
//   k_acc    one thread per scored key frame: the ten covisibility gathers; bestAccScore by atomicMax on the float's bits (acc > 0 only, for
//            which the integer order is the float order).
//   k_rank   one thread per scored key frame counts the entries whose key precedes its own — (first word, seq, slot) for the relocalisation
//            list order, (acc descending, first word, seq, slot) for N-best, which makes the stable sort a plain one — and scatters (bestKF)
//            to that rank; the earliest rank electing each bestKF is kept by a 64-bit atomicMax of (query stamp, ~rank).
//   k_emit   one workgroup walks the ranks in order and compacts the candidates (ballot / popcount prefix).
//
// Stamps (query index + 1 in the call; the stamped arrays are zeroed once per call) stand in for per-query clears.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "workspace.inc"

static constexpr int BQ_MAX_CAP = 4096;       // cap_f / cap_q limit of bow_transform
static constexpr int BQ_ROW_GRID = 1024;      // most workgroups of the two row passes; a wave takes at least BQ_ROWS_PER_WAVE rows
static constexpr int BQ_ROWS_PER_WAVE = 4;

struct BqScalars {            // one per query, zeroed per call
    int32_t n_sharing, max_common, n_scored, best_acc_bits;
};

struct BqWork {
    BqScalars* scal;          // [n_queries]
    uint32_t* mark;           // [n_slots]  stamp of the query whose conn list holds the slot
    unsigned long long* first;// [n_slots]  (stamp << 32) | ~rank of the earliest entry electing the slot
    int32_t* words;           // [n_slots]  common words of the listed slots, 0 for the others
    int32_t* first_word;      // [n_slots]
    int32_t* list;            // [n_slots]  scored slots, arbitrary order
    float* e_acc;             // [n_slots]  per list entry
    int32_t* e_best;          // [n_slots]
    int32_t* sorted;          // [n_slots]  per rank: bestKF, or -1 where the entry is no candidate
};

struct BqArgs {
    bowdb_view db;
    bowdb_query_bows qb;
    const bowdb_query* queries;
    const int32_t* conn;
    int n_conn;
    uint64_t* last_query;     // the family's state
    float* score;
    BqWork w;
    int k;                    // query index
    int nbest;                // 0 relocalisation, 1 N-best
    int n_candidates, cap_cand;
    int32_t *out_a, *n_a, *out_b, *n_b;   // reloc: cand, n_cand, -, n_required; N-best: loop, n_loop, merge, n_merge
    bowdb_stats* stats;
};

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the query's row and length (0 for a row outside the slab)
static __device__ __forceinline__ int query_row(const BqArgs& A, const bowdb_query& q, int* row) {
    if (q.row < 0 || q.row >= A.qb.n_rows) { *row = 0; return 0; }
    *row = q.row;
    return clampi(A.qb.q_n[q.row], 0, A.qb.cap_q);
}

// index of w in the ascending sq[0 .. n), or -1
static __device__ __forceinline__ int find_word(const int32_t* sq, int n, int32_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sq[mid] < w) lo = mid + 1; else hi = mid;
    }
    return (lo < n && sq[lo] == w) ? lo : -1;
}

static __device__ __forceinline__ int min_common(int max_common) { return (int)((float)max_common * 0.8f); }   // int minCommonWords = maxCommonWords*0.8f

static __global__ __launch_bounds__(256) void k_mark(BqArgs A) {
    const bowdb_query q = A.queries[A.k];
    const int start = q.conn_start, n = q.conn_n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const long long at = (long long)start + i;
        if (at < 0 || at >= A.n_conn) continue;
        const int s = A.conn[at];
        if (s >= 0 && s < A.db.n_slots) A.w.mark[s] = (uint32_t)A.k + 1u;
    }
}

static __device__ __forceinline__ int stage_query(const BqArgs& A, const bowdb_query& q, int32_t* sq, int* row) {
    const int qn = query_row(A, q, row);
    const int32_t* src = A.qb.q_word + (size_t)(*row) * A.qb.cap_q;
    for (int i = threadIdx.x; i < qn; i += blockDim.x) sq[i] = src[i];
    __syncthreads();
    return qn;
}

static __global__ __launch_bounds__(256) void k_share(BqArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int32_t* sq = (int32_t*)orb_smem;
    const bowdb_query q = A.queries[A.k];
    int qrow;
    const int qn = stage_query(A, q, sq, &qrow);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int wave_max = 0, wave_listed = 0;
    for (int s = blockIdx.x * 4 + wv; s < A.db.n_slots; s += gridDim.x * 4) {
        int cnt = 0, first = 0x7fffffff;
        const bool open = (A.db.kf[s].flags & BOWDB_KF_PRESENT) && !(A.nbest && A.w.mark[s] == (uint32_t)A.k + 1u);
        if (open && qn > 0) {
            const int n = clampi(A.db.bv_n[s], 0, A.db.cap_f);
            const int32_t* row = A.db.bv_word + (size_t)s * A.db.cap_f;
            for (int i = lane; i < n; i += 64) {
                const int32_t w = row[i];
                if (find_word(sq, qn, w) >= 0) { cnt++; first = w < first ? w : first; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {   // both reductions on one exchange: count in the high half, first word in the low half
            const unsigned long long o = __shfl_xor(((unsigned long long)(uint32_t)cnt << 32) | (uint32_t)first, m, 64);
            cnt += (int)(o >> 32);
            first = (int)(uint32_t)o < first ? (int)(uint32_t)o : first;
        }
        if (lane == 0) {
            A.w.words[s] = cnt;
            A.w.first_word[s] = first;
            if (cnt > 0) A.last_query[s] = q.id;
        }
        if (cnt > 0) { wave_listed++; wave_max = cnt > wave_max ? cnt : wave_max; }
    }
    if (lane == 0 && wave_listed > 0) {
        atomicAdd(&A.w.scal[A.k].n_sharing, wave_listed);
        atomicMax(&A.w.scal[A.k].max_common, wave_max);
    }
}

static __global__ __launch_bounds__(256) void k_score(BqArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int32_t* sq = (int32_t*)orb_smem;
    const bowdb_query q = A.queries[A.k];
    int qrow;
    const int qn = stage_query(A, q, sq, &qrow);
    const double* qv = A.qb.q_value + (size_t)qrow * A.qb.cap_q;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int min_words = min_common(A.w.scal[A.k].max_common);
    for (int s = blockIdx.x * 4 + wv; s < A.db.n_slots; s += gridDim.x * 4) {
        const int words = A.w.words[s];
        if (words <= 0 || words <= min_words) continue;   // wave-uniform
        const int n = clampi(A.db.bv_n[s], 0, A.db.cap_f);
        const int32_t* row = A.db.bv_word + (size_t)s * A.db.cap_f;
        const double* val = A.db.bv_value + (size_t)s * A.db.cap_f;
        double sum = 0.0;
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int i = c0 + lane;
            double term = 0.0;
            bool hit = false;
            if (i < n) {
                const int at = find_word(sq, qn, row[i]);
                if (at >= 0) {
                    const double vi = qv[at], wi = val[i];
                    term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                    hit = true;
                }
            }
            for (unsigned long long m = __ballot(hit); m; m &= m - 1ull) sum += __shfl(term, __ffsll((long long)m) - 1, 64);   // score += ..., ascending words
        }
        if (lane == 0) {
            A.score[s] = (float)(-sum / 2.0);
            A.w.list[atomicAdd(&A.w.scal[A.k].n_scored, 1)] = s;
        }
    }
}

static __global__ __launch_bounds__(256) void k_acc(BqArgs A) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.w.scal[A.k].n_scored) return;
    const uint64_t id = A.queries[A.k].id;
    const int s = A.w.list[e];
    float best = A.score[s], acc = best;
    int best_kf = s;
    const bowdb_keyframe* kf = A.db.kf + s;
    for (int c = 0; c < BOWDB_COVIS; c++) {
        const int n = kf->covis[c];
        if (n < 0 || n >= A.db.n_slots) continue;
        if (!(A.db.kf[n].flags & BOWDB_KF_PRESENT) || A.last_query[n] != id) continue;
        const float sn = A.score[n];
        acc += sn;
        if (sn > best) { best_kf = n; best = sn; }
    }
    A.w.e_acc[e] = acc;
    A.w.e_best[e] = best_kf;
    if (acc > 0.f) atomicMax(&A.w.scal[A.k].best_acc_bits, __float_as_int(acc));   // if(accScore>bestAccScore) from 0
}

static __global__ __launch_bounds__(256) void k_rank(BqArgs A) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int S = A.w.scal[A.k].n_scored;
    if (e >= S) return;
    const int s = A.w.list[e];
    const float acc = A.w.e_acc[e];
    const int fw = A.w.first_word[s];
    const uint32_t seq = A.db.kf[s].seq;
    int rank = 0;
    for (int j = 0; j < S; j++) {
        const int sj = A.w.list[j];
        bool before;
        const float aj = A.w.e_acc[j];
        if (A.nbest && aj != acc) before = aj > acc;
        else {
            const int fj = A.w.first_word[sj];
            const uint32_t qj = A.db.kf[sj].seq;
            before = fj != fw ? fj < fw : (qj != seq ? qj < seq : sj < s);
        }
        rank += before;
    }
    const int b = A.w.e_best[e];
    bool cand = true;
    if (!A.nbest) {   // si > minScoreToRetain, pKFi->GetMap() == pMap
        const float retain = 0.75f * __int_as_float(A.w.scal[A.k].best_acc_bits);
        cand = acc > retain && A.db.kf[b].map_id == A.queries[A.k].map_id;
    }
    A.w.sorted[rank] = cand ? b : -1;
    if (cand) atomicMax(&A.w.first[b], ((unsigned long long)((uint32_t)A.k + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)rank));
}

static __global__ __launch_bounds__(256) void k_emit(BqArgs A) {
    __shared__ int s_cnt[2][4];
    const bowdb_query q = A.queries[A.k];
    const BqScalars sc = A.w.scal[A.k];
    const int S = sc.n_scored, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cap = A.nbest ? A.n_candidates : A.cap_cand;
    int32_t* out_a = A.out_a + (size_t)A.k * cap;
    int32_t* out_b = A.nbest ? A.out_b + (size_t)A.k * cap : nullptr;
    if (A.nbest)
        for (int i = threadIdx.x; i < cap; i += blockDim.x) { out_a[i] = -1; out_b[i] = -1; }
    __syncthreads();
    int na = 0, nb = 0;   // block-uniform running counts
    for (int r0 = 0; r0 < S; r0 += 256) {
        if (A.nbest && na >= cap && nb >= cap) break;
        const int r = r0 + threadIdx.x;
        bool fa = false, fb = false;
        int b = -1;
        if (r < S) {
            b = A.w.sorted[r];
            if (b >= 0 && A.w.first[b] == (((unsigned long long)((uint32_t)A.k + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)r))) {
                if (!A.nbest) fa = true;
                else {
                    const int m = A.db.kf[b].map_id;
                    if (m == q.map_id) fa = true;
                    else fb = !(m >= 0 && m < A.db.n_maps && A.db.map_bad[m]);
                }
            }
        }
        const unsigned long long ma = __ballot(fa), mb = __ballot(fb), below = (1ull << lane) - 1ull;
        if (lane == 0) { s_cnt[0][wv] = __popcll(ma); s_cnt[1][wv] = __popcll(mb); }
        __syncthreads();
        int pa = na + __popcll(ma & below), pb = nb + __popcll(mb & below);
        for (int w = 0; w < 4; w++) {
            if (w < wv) { pa += s_cnt[0][w]; pb += s_cnt[1][w]; }
            na += s_cnt[0][w]; nb += s_cnt[1][w];
        }
        if (fa && pa < cap) out_a[pa] = b;
        if (fb && pb < cap) out_b[pb] = b;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        A.n_a[A.k] = na < cap ? na : cap;
        if (A.nbest) A.n_b[A.k] = nb < cap ? nb : cap;
        else A.n_b[A.k] = na;   // d_n_required
        if (A.stats) {
            bowdb_stats st;
            st.n_sharing = sc.n_sharing; st.max_common_words = sc.max_common; st.n_scored = S; st.best_acc_score = __int_as_float(sc.best_acc_bits);
            A.stats[A.k] = st;
        }
    }
}

// The workspace, listed once: its sections (16-byte aligned) into w.  -> bytes; *zeroed: the bytes of the leading
// sections a call clears (the per-query scalars and the two stamped arrays)
static size_t bq_layout(int n_slots, int n_queries, void* base, BqWork& w, size_t* zeroed) {
    const size_t n = (size_t)n_slots;
    WsCursor c{(unsigned char*)base, 16, 0};
    w.scal = c.take<BqScalars>((size_t)n_queries);
    w.mark = c.take<uint32_t>(n);
    w.first = c.take<unsigned long long>(n);
    *zeroed = c.off;
    w.words = c.take<int32_t>(n);
    w.first_word = c.take<int32_t>(n);
    w.list = c.take<int32_t>(n);
    w.e_acc = c.take<float>(n);
    w.e_best = c.take<int32_t>(n);
    w.sorted = c.take<int32_t>(n);
    return c.off + 16;
}

extern "C" size_t bowdb_workspace_bytes(int n_slots, int n_queries) {
    if (n_slots < 0 || n_queries < 0) return 0;
    BqWork w;
    size_t zeroed;
    return bq_layout(n_slots, n_queries, nullptr, w, &zeroed);
}

static int bq_run(const bowdb_view* db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows* q, const int32_t* d_conn, int n_conn,
                  int nbest, int cap, int32_t* out_a, int32_t* n_a, int32_t* out_b, int32_t* n_b, bowdb_stats* d_stats, void* d_workspace, void* stream) {
    if (!db || !d_queries || !q || !out_a || !n_a || !n_b || (nbest && !out_b) || !d_workspace) return ORB_E_INVALID;
    if (!db->bv_word || !db->bv_value || !db->bv_n || !db->kf || !db->reloc_query || !db->reloc_score || !db->place_query || !db->place_score ||
        !db->map_bad || !q->q_word || !q->q_value || !q->q_n)
        return ORB_E_INVALID;
    if (db->scoring != BOWDB_L1_NORM) return ORB_E_INVALID;
    if (db->cap_f < 1 || db->cap_f > BQ_MAX_CAP || q->cap_q < 1 || q->cap_q > BQ_MAX_CAP) return ORB_E_INVALID;
    if (db->n_slots < 0 || db->n_maps < 0 || q->n_rows < 0 || n_queries < 0 || n_conn < 0 || (n_conn > 0 && !d_conn)) return ORB_E_INVALID;
    if (nbest ? (cap < 1 || cap > BOWDB_MAX_CANDIDATES) : cap < 0) return ORB_E_INVALID;
    if (misaligned16(d_workspace)) return ORB_E_INVALID;
    if (n_queries == 0) return ORB_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int n = db->n_slots;
    BqArgs A;
    A.db = *db; A.qb = *q; A.queries = d_queries; A.conn = d_conn; A.n_conn = n_conn;
    A.last_query = nbest ? db->place_query : db->reloc_query;
    A.score = nbest ? db->place_score : db->reloc_score;
    A.nbest = nbest; A.n_candidates = nbest ? cap : 0; A.cap_cand = nbest ? 0 : cap;
    A.out_a = out_a; A.n_a = n_a; A.out_b = out_b; A.n_b = n_b; A.stats = d_stats;
    size_t zeroed;
    bq_layout(n, n_queries, d_workspace, A.w, &zeroed);
    if (hipMemsetAsync(d_workspace, 0, zeroed, st) != hipSuccess) return ORB_E_HIP;
    const int row_wgs = (n + 4 * BQ_ROWS_PER_WAVE - 1) / (4 * BQ_ROWS_PER_WAVE), row_grid = row_wgs < BQ_ROW_GRID ? row_wgs : BQ_ROW_GRID;
    const int ent_grid = (n + 255) / 256;
    const size_t lds = (size_t)q->cap_q * 4;
    for (int k = 0; k < n_queries; k++) {
        A.k = k;
        if (n > 0) {
            if (nbest && n_conn > 0) hipLaunchKernelGGL(k_mark, dim3((n_conn + 255) / 256 < 64 ? (n_conn + 255) / 256 : 64), dim3(256), 0, st, A);
            hipLaunchKernelGGL(k_share, dim3(row_grid), dim3(256), lds, st, A);
            hipLaunchKernelGGL(k_score, dim3(row_grid), dim3(256), lds, st, A);
            hipLaunchKernelGGL(k_acc, dim3(ent_grid), dim3(256), 0, st, A);
            hipLaunchKernelGGL(k_rank, dim3(ent_grid), dim3(256), 0, st, A);
        }
        hipLaunchKernelGGL(k_emit, dim3(1), dim3(256), 0, st, A);
    }
    return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP;
}

extern "C" int bowdb_detect_relocalization_candidates(const bowdb_view* db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows* q,
                                                      int32_t* d_cand, int cap_cand, int32_t* d_n_cand, int32_t* d_n_required, bowdb_stats* d_stats,
                                                      void* d_workspace, void* stream) {
    return bq_run(db, d_queries, n_queries, q, nullptr, 0, 0, cap_cand, d_cand, d_n_cand, nullptr, d_n_required, d_stats, d_workspace, stream);
}

extern "C" int bowdb_detect_n_best_candidates(const bowdb_view* db, const bowdb_query* d_queries, int n_queries, const bowdb_query_bows* q,
                                              const int32_t* d_conn, int n_conn, int n_candidates, int32_t* d_loop, int32_t* d_n_loop, int32_t* d_merge,
                                              int32_t* d_n_merge, bowdb_stats* d_stats, void* d_workspace, void* stream) {
    if (!d_n_loop || !d_n_merge) return ORB_E_INVALID;
    return bq_run(db, d_queries, n_queries, q, d_conn, n_conn, 1, n_candidates, d_loop, d_n_loop, d_merge, d_n_merge, d_stats, d_workspace, stream);
}
