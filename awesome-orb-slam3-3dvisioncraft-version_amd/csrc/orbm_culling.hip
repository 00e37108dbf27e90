// orbm_culling.hip — LocalMapping::KeyFrameCulling on the device map for gfx950 (include/orbhip.h "Key-frame culling"): the last step of
// LocalMapping::Run that had to walk the whole local map on the host.
//
//   k_cull_init         grid-wide, fills every problem's slice of the workspace (a kernel rather than a memset node, so that a captured graph
//                       holds kernels only): the record state words (live / absent, with the record's feature byte so that the walk reads no
//                       key-frame record per observation), MapPoint::nObs (given, or the weighted sum over the point's records), the bad
//                       bytes, the checked link copies, zeros.  What it finds wrong in the map is flagged in every problem.
//   k_cull_walk         one CULL_WG-lane workgroup per problem.  Candidates are serial (LocalMapping.cc:1207-1321: every cull changes what the
//                       next candidate sees).  Per candidate: the lanes stride over its features and each walks its point's records; nMPs and
//                       nRedundantObservations are ballot / popcount sums per wave and one LDS add; lane 0 takes the decision (the float test
//                       of :1278 and the inertial tests :1280-1310) and publishes it through LDS; the erase pass (KeyFrame::SetBadFlag's
//                       EraseObservation loop) runs over the features again.  A record dies by an integer compare-and-swap on its state word:
//                       exactly once whatever the lane order, and only the lane that killed a point's record of the key frame lowers nObs.
//   k_cull_apply_count / _scan / _write   orbm_apply_keyframe_culling: the CSR of the live records by obs_csr.inc's three launches (the scan
//                       decides overflow: then the write launch writes nothing), and with it the map's flags, rows and reference key frames.
// The record check, the point test and the stereo weight are mapview.inc's.
//
// Workspace of problem b (each section padded to 16 bytes): hdr int32[8] | nobs int32[n_mp] | rec uint32[n_obs] | prev int32[n_kf] |
// next int32[n_kf] | blk int32[csr_blk_words(n_mp)] | mp_bad uint8[n_mp] | kf_erased uint8[n_kf].
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "obs_csr.inc"
#include "workspace.inc"

#ifndef CULL_WG
#define CULL_WG 1024   // the fastest of 64 / 128 / 256 / 512 / 1024 for one problem (and of 256 / 1024 for 64): DESIGN.md "Key-frame culling"
#endif
static_assert(CULL_WG % 64 == 0 && CULL_WG >= 64 && CULL_WG <= 1024, "whole waves");

struct CullWork {
    int32_t *hdr, *nobs;
    uint32_t* rec;
    int32_t *prev, *next, *blk;
    uint8_t *mp_bad, *kf_erased;
};
enum { CULL_HDR_WORDS = 8, CULL_HDR_FLAGS = 0 };
constexpr int CULL_ND = 21;   // LocalMapping.cc:1176

// One problem's slice, listed once.  -> bytes of the slice (a multiple of 16)
static __host__ __device__ __forceinline__ size_t cull_work_layout(int n_kf, int n_mp, int n_obs, unsigned char* base, CullWork& W) {
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp;
    WsCursor c{base, 16, 0};
    W.hdr = c.take<int32_t>(CULL_HDR_WORDS);
    W.nobs = c.take<int32_t>(nm);
    W.rec = c.take<uint32_t>((size_t)n_obs);
    W.prev = c.take<int32_t>(nk);
    W.next = c.take<int32_t>(nk);
    W.blk = c.take<int32_t>(csr_blk_words(n_mp));
    W.mp_bad = c.take<uint8_t>(nm);
    W.kf_erased = c.take<uint8_t>(nk);
    return c.off;
}

struct CullArgs {
    orbm_localmap_view V;
    orbm_cull_in I;
    orbm_cull_out O;
    unsigned char* work;
    size_t stride;   // bytes per problem
    int batch;
};

static __device__ __forceinline__ CullWork cull_work(const CullArgs& A, int b) {
    CullWork W;
    cull_work_layout(A.V.n_kf, A.V.n_mp, A.V.n_obs, A.work + (size_t)b * A.stride, W);
    return W;
}

// The state word of record o as the map gives it: LIVE | feature byte << 8, or ABSENT.  -> flag bits
static __device__ __forceinline__ uint32_t cull_record(const CullArgs& A, int o, uint32_t* word) {
    int idx;
    const int row = view_record_row(A.V, A.I.d_ckf, A.V.d_obs[o], &idx);
    *word = row < 0 ? ORBM_CULL_REC_ABSENT : ORBM_CULL_REC_LIVE | ((uint32_t)A.I.d_feat[row] << 8);
    return view_record_flag(row, ORBM_CULL_UNSUPPORTED, ORBM_CULL_BAD_INDEX);
}

static __device__ __forceinline__ int cull_link(const CullArgs& A, int v, uint32_t* bad) {
    if (v == -1) return -1;
    if (!view_present(A.V, v)) { *bad |= ORBM_CULL_BAD_INDEX; return -1; }
    return v;
}

// grid (x, batch): x strides over max(n_obs, n_mp, n_kf)
static __global__ __launch_bounds__(256) void k_cull_init(CullArgs A) {
    const int b = blockIdx.y;
    const CullWork W = cull_work(A, b);
    const int n_mp = A.V.n_mp, n_kf = A.V.n_kf, n_obs = A.V.n_obs;
    const int n = max(max(n_obs, n_mp), max(n_kf, (int)CULL_HDR_WORDS));
    uint32_t bad = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (i < CULL_HDR_WORDS && i != CULL_HDR_FLAGS) W.hdr[i] = 0;
        if (i < n_obs) {
            uint32_t w;
            bad |= cull_record(A, i, &w);
            W.rec[i] = w;
        }
        if (i < n_kf) {
            int pv = -1, nx = -1;
            if (A.V.d_kf[i].flags & ORBM_LM_KF_PRESENT) {
                pv = cull_link(A, A.I.d_ckf[i].prev, &bad);
                nx = cull_link(A, A.I.d_ckf[i].next, &bad);
            }
            W.prev[i] = pv;
            W.next[i] = nx;
            W.kf_erased[i] = 0;
        }
        if (i < n_mp) {
            int s, e, sum = 0;
            if (!view_obs_range(A.V, i, &s, &e)) bad |= ORBM_CULL_BAD_INDEX;
            else if (!A.I.d_mp_nobs)
                for (int o = s; o < e; o++) {   // AddObservation's weights (MapPoint.cc:191-194) over the records that can be read
                    uint32_t w;
                    cull_record(A, o, &w);
                    if ((w & 3u) == ORBM_CULL_REC_LIVE) sum += view_feat_weight(w >> 8);
                }
            W.nobs[i] = A.I.d_mp_nobs ? A.I.d_mp_nobs[i] : sum;
            W.mp_bad[i] = (A.V.d_mp[i].flags & ORBM_MP_BAD) ? 1 : 0;
        }
    }
    // hdr[FLAGS] is the one word several lanes write: k_cull_flags_clear zeroed it before this launch
    flag_or(&W.hdr[CULL_HDR_FLAGS], bad);
}

static __global__ __launch_bounds__(64) void k_cull_flags_clear(CullArgs A) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < A.batch) cull_work(A, b).hdr[CULL_HDR_FLAGS] = 0;
}

// the point of feature i of a key frame whose rows start at row0, if it can be used: in range, a valid slot, a CSR range inside the records
static __device__ __forceinline__ int cull_point(const CullArgs& A, int row0, int i, int* s, int* e, uint32_t* bad) {
    const int p = A.V.d_kf_mp[row0 + i];
    if (p == -1) return -1;
    if (!view_point_ok(A.V, p)) { *bad |= ORBM_CULL_BAD_INDEX; return -1; }
    if (!view_obs_range(A.V, p, s, e)) { *bad |= ORBM_CULL_BAD_INDEX; return -1; }
    return p;
}

// cv::norm of a float 3-vector difference as the reference's `cv::norm(a - b) < 0.02` sees it: the differences in float, sqrt of the double dot
// product summed from 0 (DESIGN.md "Map-point refresh"), not rounded to float: the comparison is in double
static __device__ __forceinline__ double cull_norm3(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    double s = 0.0;
    s += (double)dx * (double)dx;
    s += (double)dy * (double)dy;
    s += (double)dz * (double)dz;
    return sqrt(s);
}

enum { CULL_S_NMP = 0, CULL_S_NRED = 1, CULL_S_ERASE = 2, CULL_S_STOP = 3, CULL_S_FLAGS = 4, CULL_S_WORDS = 8 };

static __global__ __launch_bounds__(CULL_WG) void k_cull_walk(CullArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* sh = (int*)orb_smem;   // [CULL_S_WORDS]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const CullWork W = cull_work(A, b);
    const orbm_cull_problem P = A.I.d_problems[b];
    const size_t o0 = (size_t)b * A.O.cap_cand;
    uint32_t bad = 0;

    // what cannot be read ends the problem before the loop: nothing is visited
    int n_cand = P.n_cand;
    const bool range_ok = P.cand_start >= 0 && n_cand >= 0 && n_cand <= A.I.n_candidates - P.cand_start && n_cand <= A.I.n_cand_max &&
                          n_cand <= A.O.cap_cand;
    if (!range_ok) { bad |= ORBM_CULL_BAD_INDEX; n_cand = 0; }
    const bool cur_ok = view_present(A.V, P.current_kf);
    if (!cur_ok) bad |= ORBM_CULL_BAD_INDEX;
    const int32_t* cand = A.I.d_candidates + (range_ok ? P.cand_start : 0);
    for (int c = tid; c < n_cand; c += CULL_WG) {
        A.O.d_code[o0 + c] = ORBM_CULL_CODE_NOT_VISITED;
        A.O.d_nmps[o0 + c] = 0;
        A.O.d_nred[o0 + c] = 0;
    }
    if (tid == 0) { sh[CULL_S_FLAGS] = 0; sh[CULL_S_NMP] = 0; sh[CULL_S_NRED] = 0; }
    __syncthreads();

    const bool inertial = P.flags & ORBM_CULL_INERTIAL, mono = P.flags & ORBM_CULL_MONOCULAR;
    const float redundant_th = (!inertial || mono) ? 0.9f : 0.5f;   // :1180-1186
    // lane 0's serial state
    uint32_t cur_id = 0, last_id = 0;
    int kf_in_map = P.n_kf_in_map, n_events = 0;
    if (tid == 0 && cur_ok) {
        cur_id = A.I.d_ckf[P.current_kf].id;
        int aux = P.current_kf;   // :1193-1203 on the links as given (nothing has been relinked yet)
        for (int k = 0; k < CULL_ND && W.prev[aux] != -1; k++) aux = W.prev[aux];
        last_id = A.I.d_ckf[aux].id;
    }

    int count = 0;
    for (int c = 0; c < n_cand && cur_ok; c++) {
        count++;
        const int k = cand[c];
        const bool present = view_present(A.V, k);
        if (!present) bad |= ORBM_CULL_BAD_INDEX;
        if (!present || A.I.d_ckf[k].id == P.init_kf_id || (A.V.d_kf[k].flags & ORBM_LM_KF_BAD) || W.kf_erased[k]) {   // :1212
            if (tid == 0) A.O.d_code[o0 + c] = ORBM_CULL_CODE_SKIPPED;
            continue;
        }
        int row0, nf;
        if (!view_rows(A.V, k, &row0, &nf)) bad |= ORBM_CULL_BAD_INDEX;

        // ---- :1216-1276: nMPs and nRedundantObservations
        int w_nmp = 0, w_red = 0;
        for (int c0 = 0; c0 < nf; c0 += CULL_WG) {
            const int i = c0 + tid;
            bool is_mp = false, is_red = false;
            int s = 0, e = 0;
            const int p = i < nf ? cull_point(A, row0, i, &s, &e, &bad) : -1;
            if (p >= 0 && !W.mp_bad[p]) {
                const uint32_t fb = A.I.d_feat[row0 + i];
                if (mono || (fb & ORBM_CULL_FEAT_CLOSE)) {
                    is_mp = true;
                    if (ld_relaxed(&W.nobs[p]) > 3) {   // Observations() > thObs
                        const int level = (int)(fb & ORBM_CULL_FEAT_OCTAVE) + 1;
                        int n = 0;
                        for (int o = s; o < e; o++) {
                            const uint32_t w = ld_relaxed(&W.rec[o]);
                            if ((w & 3u) != ORBM_CULL_REC_LIVE || A.V.d_obs[o].kf == k) continue;
                            n += (int)((w >> 8) & ORBM_CULL_FEAT_OCTAVE) <= level ? 1 : 0;
                        }
                        is_red = n > 3;
                    }
                }
            }
            w_nmp += __popcll(__ballot(is_mp));
            w_red += __popcll(__ballot(is_red));
        }
        if (lane == 0 && (w_nmp | w_red)) { atomicAdd(&sh[CULL_S_NMP], w_nmp); atomicAdd(&sh[CULL_S_NRED], w_red); }
        __syncthreads();

        // ---- :1278-1320: the decision, on one lane
        if (tid == 0) {
            const int nmp = sh[CULL_S_NMP], nred = sh[CULL_S_NRED];
            sh[CULL_S_NMP] = 0;
            sh[CULL_S_NRED] = 0;
            A.O.d_nmps[o0 + c] = nmp;
            A.O.d_nred[o0 + c] = nred;
            int code = ORBM_CULL_CODE_KEPT, ev_prev = -1, ev_next = -1;
            bool set_bad = false, skip_break = false;
            if ((float)nred > redundant_th * (float)nmp) {
                if (!inertial) { code = ORBM_CULL_CODE_CULLED; set_bad = true; }
                else if (kf_in_map <= CULL_ND) { code = ORBM_CULL_CODE_KEPT_FEW_KFS; skip_break = true; }
                else if (A.I.d_ckf[k].id > cur_id - 2u) { code = ORBM_CULL_CODE_KEPT_RECENT; skip_break = true; }
                else {
                    const int pv = W.prev[k], nx = W.next[k];
                    if (pv == -1 || nx == -1) code = ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR;
                    else {
                        const float t = (float)(A.I.d_ckf[nx].timestamp - A.I.d_ckf[pv].timestamp);
                        if (((P.flags & ORBM_CULL_IMU_INITIALIZED) && A.I.d_ckf[k].id < last_id && t < 3.f) || t < 0.5f)
                            code = ORBM_CULL_CODE_CULLED_IMU1;
                        else if (!(P.flags & ORBM_CULL_INERTIAL_BA2) && cull_norm3(A.I.d_ckf[k].imu_pos, A.I.d_ckf[pv].imu_pos) < 0.02 && t < 3.f)
                            code = ORBM_CULL_CODE_CULLED_IMU2;
                        else code = ORBM_CULL_CODE_KEPT_INERTIAL;
                        if (code != ORBM_CULL_CODE_KEPT_INERTIAL) {
                            W.prev[nx] = pv;
                            W.next[pv] = nx;
                            W.next[k] = -1;
                            W.prev[k] = -1;
                            ev_prev = pv; ev_next = nx;
                            set_bad = true;
                        }
                    }
                }
            }
            bool erase = false;
            if (set_bad) {   // KeyFrame::SetBadFlag
                if (n_events < A.O.cap_cand) {
                    orbm_cull_event ev;
                    ev.kf = k; ev.prev = ev_prev; ev.next = ev_next;
                    A.O.d_events[o0 + n_events] = ev;
                }
                n_events++;
                if (A.I.d_ckf[k].flags & ORBM_CULL_KF_NOT_ERASE) code |= ORBM_CULL_CODE_DEFERRED;
                else { erase = true; kf_in_map--; W.kf_erased[k] = 1; }
            }
            A.O.d_code[o0 + c] = (uint8_t)code;
            sh[CULL_S_ERASE] = erase ? 1 : 0;
            sh[CULL_S_STOP] = (!skip_break && ((count > 20 && (P.flags & ORBM_CULL_ABORT_BA)) || count > 100)) ? 1 : 0;   // :1317
        }
        __syncthreads();
        const bool erase = sh[CULL_S_ERASE], stop = sh[CULL_S_STOP];

        // ---- KeyFrame.cc:681-688: EraseObservation for every feature with a point
        if (erase)
            for (int i = tid; i < nf; i += CULL_WG) {
                int s, e;
                const int p = cull_point(A, row0, i, &s, &e, &bad);
                if (p < 0) continue;
                int o = s;
                while (o < e && !(A.V.d_obs[o].kf == k && (W.rec[o] & 3u) != ORBM_CULL_REC_ABSENT)) o++;   // mObservations.count(pKF)
                if (o == e) continue;
                const uint32_t w = ld_relaxed(&W.rec[o]);
                if ((w & 3u) != ORBM_CULL_REC_LIVE || atomicCAS(&W.rec[o], w, w | ORBM_CULL_REC_ERASED_BY_KF) != w) continue;
                const int dec = view_feat_weight(w >> 8);
                const int left = atomicSub(&W.nobs[p], dec) - dec;
                if (left <= 2) {   // MapPoint::SetBadFlag: this lane alone owns the point now
                    W.mp_bad[p] = 1;
                    for (int q = s; q < e; q++) {
                        const uint32_t x = ld_relaxed(&W.rec[q]);
                        if ((x & 3u) == ORBM_CULL_REC_LIVE) atomicCAS(&W.rec[q], x, x | ORBM_CULL_REC_ERASED_BY_POINT);
                    }
                }
            }
        __syncthreads();   // the next candidate reads the states, and lane 0 rewrites the LDS words
        if (stop) break;
    }

    flag_or(&sh[CULL_S_FLAGS], bad);
    __syncthreads();
    if (tid == 0) {
        A.O.d_n_events[b] = n_events;
        A.O.d_flags[b] = (uint32_t)sh[CULL_S_FLAGS] | (uint32_t)W.hdr[CULL_HDR_FLAGS];
    }
}

// ------------------------------------------------------------------------------------------------ apply
struct CullApplyArgs {
    orbm_localmap_view V;
    orbm_cull_in I;
    orbm_cull_apply Y;
    unsigned char* work;   // the problem's slice
};

static __device__ __forceinline__ CullWork cull_apply_work(const CullApplyArgs& A) {
    CullWork W;
    cull_work_layout(A.V.n_kf, A.V.n_mp, A.V.n_obs, A.work, W);
    return W;
}

// the live records of point p (0 for a range that leaves the records)
static __device__ __forceinline__ int cull_live(const CullApplyArgs& A, const CullWork& W, int p, int* s, int* e) {
    int n = 0;
    if (p >= A.V.n_mp || !view_obs_range(A.V, p, s, e)) { *s = *e = 0; return 0; }
    for (int o = *s; o < *e; o++) n += (W.rec[o] & 3u) == ORBM_CULL_REC_LIVE ? 1 : 0;
    return n;
}

// (the three apply kernels are obs_csr.inc's count / scan / place; orb_smem = its scratch, int[2][4])
static __global__ __launch_bounds__(256) void k_cull_apply_count(CullApplyArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const CullWork W = cull_apply_work(A);
    int s, e;
    csr_count(cull_live(A, W, blockIdx.x * 256 + threadIdx.x, &s, &e), W.blk, (int*)orb_smem);
}

// one workgroup: the block totals scanned; overflow is decided here, before anything is written
static __global__ __launch_bounds__(256) void k_cull_apply_scan(CullApplyArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const CullWork W = cull_apply_work(A);
    int it = 0;
    const int run = csr_scan_blocks(W.blk, nblk, (int*)orb_smem, &it);
    if (threadIdx.x == 0) {
        W.blk[nblk] = run;
        A.Y.d_result[0] = run;
        A.Y.d_result[1] = run > A.Y.cap_obs_out ? 1 : 0;
    }
}

// grid x strides over max(n_mp blocks, records, key frames) in blocks of 256: block j < nblk also compacts its 256 points (and block 0 a map
// without points: its CSR is one zero)
static __global__ __launch_bounds__(256) void k_cull_apply_write(CullApplyArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const CullWork W = cull_apply_work(A);
    if (csr_total(W.blk, nblk) > A.Y.cap_obs_out) return;   // overflow: nothing is written
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int n_mp = A.V.n_mp, n_kf = A.V.n_kf, n_obs = A.V.n_obs;
    if (blockIdx.x < nblk || blockIdx.x == 0) {   // (uniform: csr_place holds a barrier)
        int s, e;
        int at = csr_place(cull_live(A, W, g, &s, &e), W.blk, n_mp, true, A.Y.d_obs_start_out, (int*)orb_smem);
        if (g < n_mp) {
            const bool is_bad = W.mp_bad[g];
            const int ref = A.Y.d_ref[g].ref_kf;
            bool ref_erased = false;
            int first = -1;
            for (int o = s; o < e; o++) {
                const uint32_t w = W.rec[o];
                const orbm_observation r = A.V.d_obs[o];
                if ((w & 3u) == ORBM_CULL_REC_LIVE) {
                    if (first < 0) first = o;
                    A.Y.d_obs_out[at++] = r;
                } else if ((w & 3u) == ORBM_CULL_REC_ERASED_BY_KF && r.kf == ref) ref_erased = true;
            }
            if (!is_bad && ref_erased && first >= 0) {   // mpRefKF = mObservations.begin()->first (MapPoint.cc:220-221)
                orbm_refresh_point rp;
                rp.ref_kf = A.V.d_obs[first].kf;
                rp.level = (int)((W.rec[first] >> 8) & ORBM_CULL_FEAT_OCTAVE);
                A.Y.d_ref[g] = rp;
            }
            const int nobs = W.nobs[g];
            uint32_t f = A.Y.d_mp[g].flags;
            f = (f & ~ORBM_MP_HAS_OBS) | (nobs > 0 ? ORBM_MP_HAS_OBS : 0u) | (is_bad ? ORBM_MP_BAD : 0u);
            A.Y.d_mp[g].flags = f;
            if (A.Y.d_mp_nobs) A.Y.d_mp_nobs[g] = nobs;
        }
    }
    if (g < n_obs && (W.rec[g] & 3u) == ORBM_CULL_REC_ERASED_BY_POINT) {   // EraseMapPointMatch(leftIndex)
        int idx;
        const int row = view_record_row(A.V, A.I.d_ckf, A.V.d_obs[g], &idx);   // (a row: the init launch gave a state to checked records only)
        if (row >= 0) A.Y.d_kf_mp[row] = -1;
    }
    if (g < n_kf) {
        if (W.kf_erased[g]) A.Y.d_kf[g].flags |= ORBM_LM_KF_BAD;
        if (A.Y.d_kf[g].flags & ORBM_LM_KF_PRESENT) {
            A.Y.d_kf[g].prev = W.prev[g];
            A.Y.d_ckf[g].prev = W.prev[g];
            A.Y.d_ckf[g].next = W.next[g];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
static size_t cull_work_bytes(int n_kf, int n_mp, int n_obs) { CullWork W; return cull_work_layout(n_kf, n_mp, n_obs, nullptr, W); }

extern "C" size_t orbm_cull_workspace_bytes(int n_kf, int n_mp, int n_obs, int batch) {
    if (n_kf < 0 || n_mp < 0 || n_obs < 0 || batch < 0) return 0;
    return (size_t)batch * cull_work_bytes(n_kf, n_mp, n_obs);
}

extern "C" int orbm_cull_workspace(int n_kf, int n_mp, int n_obs, orbm_cull_workspace_layout* layout) {
    if (!layout || n_kf < 0 || n_mp < 0 || n_obs < 0) return ORB_E_INVALID;
    CullWork W;
    layout->stride = cull_work_layout(n_kf, n_mp, n_obs, nullptr, W);
    layout->nobs = (size_t)W.nobs;   // from a null base the pointers are the offsets
    layout->rec = (size_t)W.rec;
    layout->prev = (size_t)W.prev;
    layout->next = (size_t)W.next;
    layout->mp_bad = (size_t)W.mp_bad;
    layout->kf_erased = (size_t)W.kf_erased;
    return ORB_OK;
}

static bool cull_view_invalid(const orbm_localmap_view& V, const orbm_cull_in& I) {
    if (view_invalid(V, VIEW_ALL) || I.n_candidates < 0 || I.n_cand_max < 0) return true;
    return (!I.d_ckf && V.n_kf) || (!I.d_feat && V.n_kf_mp_rows) || (!I.d_candidates && I.n_candidates);
}

extern "C" int orbm_cull_keyframes(const orbm_localmap_view* view, const orbm_cull_in* in, int batch, const orbm_cull_out* out, void* d_work,
                                   void* stream) {
    if (!view || !in || !out || !d_work || batch < 0) return ORB_E_INVALID;
    const orbm_cull_out& O = *out;
    if (cull_view_invalid(*view, *in) || !in->d_problems || misaligned16(d_work)) return ORB_E_INVALID;
    if (!O.d_code || !O.d_nmps || !O.d_nred || !O.d_events || !O.d_n_events || !O.d_flags || O.cap_cand < 1) return ORB_E_INVALID;
    if (in->n_cand_max > O.cap_cand) return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    CullArgs A;
    A.V = *view; A.I = *in; A.O = O; A.work = (unsigned char*)d_work; A.batch = batch;
    A.stride = cull_work_bytes(view->n_kf, view->n_mp, view->n_obs);
    hipStream_t st = (hipStream_t)stream;
    int n = view->n_obs > view->n_mp ? view->n_obs : view->n_mp;
    if (view->n_kf > n) n = view->n_kf;
    const int gx = n + 255 < 256 * 256 ? (n + 255) / 256 : 256;
    hipLaunchKernelGGL(k_cull_flags_clear, dim3((batch + 63) / 64), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_cull_init, dim3(gx > 0 ? gx : 1, batch), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_cull_walk, dim3(batch), dim3(CULL_WG), CULL_S_WORDS * 4, st, A);
    return launch_status();
}

extern "C" int orbm_apply_keyframe_culling(const orbm_localmap_view* view, const orbm_cull_in* in, int batch, int problem,
                                           const orbm_cull_apply* apply, void* d_work, void* stream) {
    if (!view || !in || !apply || !d_work || batch < 0 || problem < 0 || problem >= batch) return ORB_E_INVALID;
    const orbm_cull_apply& Y = *apply;
    if (cull_view_invalid(*view, *in) || misaligned16(d_work) || misaligned16(Y.d_mp)) return ORB_E_INVALID;
    if ((!Y.d_mp && view->n_mp) || (!Y.d_kf && view->n_kf) || (!Y.d_ckf && view->n_kf) || (!Y.d_kf_mp && view->n_kf_mp_rows) ||
        (!Y.d_ref && view->n_mp) || !Y.d_obs_start_out || (!Y.d_obs_out && Y.cap_obs_out) || !Y.d_result || Y.cap_obs_out < 0)
        return ORB_E_INVALID;
    CullApplyArgs A;
    A.V = *view; A.I = *in; A.Y = Y;
    A.work = (unsigned char*)d_work + (size_t)problem * cull_work_bytes(view->n_kf, view->n_mp, view->n_obs);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = csr_blocks(view->n_mp);
    int n = view->n_obs > view->n_mp ? view->n_obs : view->n_mp;
    if (view->n_kf > n) n = view->n_kf;
    const int gx = n > 0 ? (n + 255) / 256 : 1;
    if (nblk) hipLaunchKernelGGL(k_cull_apply_count, dim3(nblk), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_cull_apply_scan, dim3(1), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL(k_cull_apply_write, dim3(gx), dim3(256), 32, st, A, nblk);
    return launch_status();
}
