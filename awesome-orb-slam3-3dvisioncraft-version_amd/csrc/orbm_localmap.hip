// orbm_localmap.hip — Tracking::UpdateLocalMap on the device map for gfx950 (include/orbhip.h "Local map"): the list of local map points
// that orbm_project_map_points(ORBM_PROJ_LOCAL_MAP) reads is built on the device, between the two pose optimisations, with no host step.
//
//   k_lm_keyframes      Tracking::UpdateLocalKeyFrames (Tracking.cc:3042-3244) and the marking loop of SearchLocalPoints (:2852-2872): one
//                       256-lane workgroup per frame.  Votes are integer atomics on a [n_kf] counter; the first level is an ordered
//                       compaction over the pointer-order ranks (wg_scan.inc's ballot step); the second loop and the inertial tail are serial
//                       by nature (every push changes what the next test sees) and run on one lane; the segment offsets of UpdateLocalPoints'
//                       walk are a workgroup scan (its value step).
//   k_lm_points_first   UpdateLocalPoints (:2998-3036), pass 1: one workgroup per local key frame; every usable occurrence of a point offers
//                       its position in the walk (reverse key-frame order, feature order) to a [n_mp] table with an integer atomicMax of
//                       ~position: the first occurrence wins whatever the order the lanes run in.
//   k_lm_points_count   pass 2: the winners of each key frame are counted.
//   k_lm_points_write   pass 3: the counts before a key frame are summed, its winners are compacted in feature order and the records, track
//                       entries and indices are gathered.
//   k_lm_store_tracks   orbm_store_local_tracks.
//
//   k_lm_clear          zeroes the workspace (a kernel of its own rather than a memset node, so that a captured graph holds kernels only).
//
// Workspace of frame b (int32 words, cleared on the stream in every call): header[8] | votes[n_kf] | listed[n_kf] | list[n_kf] |
// seg_off[n_kf] | seg_cnt[n_kf] | first[n_mp] | mark[n_mp].
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "wg_scan.inc"
#include "workspace.inc"

struct LmArgs {
    orbm_localmap_view V;
    const orbm_localmap_frame* frames;
    orbm_localmap_lists L;
    orbm_localmap_out O;
    int32_t* work;
    size_t work_stride;   // words per frame
};

struct LmWork {
    int32_t *hdr, *votes, *listed, *list, *seg_off, *seg_cnt;
    uint32_t *first, *mark;
};
enum { LM_HDR_WORDS = 8, LM_HDR_NSEG = 0 };
constexpr uint32_t LM_MARK_FRAME = 1u, LM_MARK_DROPPED = 2u;
// k_lm_points_write patches the two members in the 16-byte words it moves
static_assert(sizeof(orbm_map_point) == 48 && offsetof(orbm_map_point, flags) == 44, "orbm_map_point.flags is word 3 of the third uint4");
static_assert(sizeof(orbm_track) == 32 && offsetof(orbm_track, in_view) == 24, "orbm_track.in_view is word 2 of the second uint4");

// One frame's slice of the workspace, listed once: its sections into W.  -> words of the slice, the stride between
// frames: a multiple of 4 so that the workspace is cleared in 16-byte words
static __host__ __device__ __forceinline__ size_t lm_work_layout(int n_kf, int n_mp, int32_t* base, LmWork& W) {
    const size_t nk = (size_t)n_kf, nm = (size_t)n_mp;
    WsCursor c{(unsigned char*)base, 4, 0};
    W.hdr = c.take<int32_t>(LM_HDR_WORDS);
    W.votes = c.take<int32_t>(nk);
    W.listed = c.take<int32_t>(nk);
    W.list = c.take<int32_t>(nk);
    W.seg_off = c.take<int32_t>(nk);
    W.seg_cnt = c.take<int32_t>(nk);
    W.first = c.take<uint32_t>(nm);
    W.mark = c.take<uint32_t>(nm);
    return (c.off / 4 + 3) & ~(size_t)3;
}
static __device__ __forceinline__ LmWork lm_work(const LmArgs& A, int b) {
    LmWork W;
    lm_work_layout(A.V.n_kf, A.V.n_mp, A.work + (size_t)b * A.work_stride, W);
    return W;
}

static __device__ __forceinline__ int lm_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the position of an occurrence in UpdateLocalPoints' walk as the atomicMax key: a smaller position is a greater key, 0 = no occurrence
static __device__ __forceinline__ uint32_t lm_key(uint32_t pos) { return 0xFFFFFFFFu - pos; }

// Nulls one list of map-point indices and, per remaining entry, votes and / or marks.  Lane tid owns entries tid, tid + 256, ...: the two
// visits of an aliased list never meet in different lanes.
static __device__ __forceinline__ uint32_t lm_visit(const LmArgs& A, const LmWork& W, int32_t* lst, int n, bool vote, uint32_t mark, int tid) {
    uint32_t bad = 0;
    for (int i = tid; i < n; i += 256) {
        const int p = lst[i];
        if (p == -1) continue;
        if (!view_point_ok(A.V, p)) { lst[i] = -1; bad = ORBM_LM_BAD_INDEX; continue; }
        if (A.V.d_mp[p].flags & ORBM_MP_BAD) { lst[i] = -1; continue; }   // Tracking.cc:3079 / :3108 / :2860
        if (mark) atomicOr(&W.mark[p], mark);
        if (!vote) continue;
        int s, e;
        if (!view_obs_range(A.V, p, &s, &e)) { bad = ORBM_LM_BAD_INDEX; continue; }
        for (int o = s; o < e; o++) {   // keyframeCounter[it->first]++ per mObservations entry (:3065-3075)
            const int kf = A.V.d_obs[o].kf;
            if ((A.V.d_obs[o].flags & ORBM_OBS_RIGHT) && o > s && A.V.d_obs[o - 1].kf == kf) continue;   // the entry's rightIndex
            if (kf < 0 || kf >= A.V.n_kf) { bad = ORBM_LM_BAD_INDEX; continue; }
            atomicAdd(&W.votes[kf], 1);
        }
    }
    return bad;
}

static __global__ __launch_bounds__(256) void k_lm_keyframes(LmArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* wtot = (int*)orb_smem;                                        // [2][4] per-wave totals by chunk parity
    unsigned long long* sbest = (unsigned long long*)(orb_smem + 32);  // (votes << 32) | ~rank of pKFmax
    uint32_t* sflags = (uint32_t*)(orb_smem + 40);
    int* sn = (int*)(orb_smem + 44);                                   // [0] list size, [1] segments
    const int b = blockIdx.x, tid = threadIdx.x;
    const LmWork W = lm_work(A, b);
    const int n_kf = A.V.n_kf;
    if (tid == 0) { *sbest = 0ull; *sflags = 0u; }
    __syncthreads();

    // the vote list (:3050-3112), the frame list (:2852-2872), the dropped points
    uint32_t bad = 0;
    const size_t l0 = (size_t)b * A.L.cap_f;
    bad |= lm_visit(A, W, A.L.d_vote_mp + l0, lm_clamp(A.L.d_n_vote[b], A.L.cap_f), true, 0u, tid);
    bad |= lm_visit(A, W, A.L.d_frame_mp + l0, lm_clamp(A.L.d_n_frame[b], A.L.cap_f), false, LM_MARK_FRAME, tid);
    if (A.L.d_dropped_mp) {
        const int32_t* dl = A.L.d_dropped_mp + (size_t)b * A.L.cap_dropped;
        const int nd = lm_clamp(A.L.d_n_dropped[b], A.L.cap_dropped);
        for (int i = tid; i < nd; i += 256) {
            const int p = dl[i];
            if (p == -1) continue;
            if (!view_point_ok(A.V, p)) { bad = ORBM_LM_BAD_INDEX; continue; }
            atomicOr(&W.mark[p], LM_MARK_DROPPED);
        }
    }
    __syncthreads();

    // first level (:3131-3150): keyframeCounter in pointer order = the ranks of d_kf_by_order, compacted in rank order
    int base = 0;
    for (int c0 = 0, it = 0; c0 < n_kf; c0 += 256, it++) {
        const int r = c0 + tid;
        bool keep = false;
        int k = -1;
        if (r < n_kf) {
            k = A.V.d_kf_by_order[r];
            if (k < 0 || k >= n_kf) bad = ORBM_LM_BAD_INDEX;
            else {
                const int votes = W.votes[k];
                if (votes > 0) {
                    const uint32_t f = A.V.d_kf[k].flags;
                    if (!(f & ORBM_LM_KF_PRESENT)) bad = ORBM_LM_BAD_INDEX;
                    else if (!(f & ORBM_LM_KF_BAD)) {   // isBad() is tested before the max (:3136)
                        keep = true;
                        atomicMax(sbest, ((unsigned long long)(uint32_t)votes << 32) | (unsigned long long)lm_key((uint32_t)r));
                    }
                }
            }
        }
        int tot;
        const int pos = base + wg_scan_ballot<4>(keep, wtot, it, &tot);
        if (keep) {
            if (pos < n_kf) W.list[pos] = k;   // a permutation lists a key frame once, so the list fits n_kf
            W.listed[k] = 1;                   // mnTrackReferenceForFrame = mCurrentFrame.mnId
        }
        base += tot;
    }
    if (bad) atomicOr(sflags, bad);
    __syncthreads();

    if (tid == 0) {
        uint32_t fl = *sflags;
        const int n1 = base < n_kf ? base : n_kf;
        int n = n1;
        auto push = [&](int v) {
            if (n < n_kf) W.list[n] = v;
            W.listed[v] = 1;
            n++;
        };
        // second loop (:3155-3213): over the first-level entries only (itEndKF is taken before any push)
        for (int i = 0; i < n1; i++) {
            if (n > 80) break;
            const orbm_localmap_keyframe& K = A.V.d_kf[W.list[i]];
            for (int c = 0; c < 10; c++) {   // GetBestCovisibilityKeyFrames(10)
                const int v = K.covis[c];
                if (v == -1) continue;
                if (!view_present(A.V, v)) { fl |= ORBM_LM_BAD_INDEX; continue; }
                if ((A.V.d_kf[v].flags & ORBM_LM_KF_BAD) || W.listed[v]) continue;
                push(v);
                break;
            }
            if (K.n_child < 0 || K.child_start < 0 || K.n_child > A.V.n_children - K.child_start) fl |= ORBM_LM_BAD_INDEX;
            else
                for (int c = 0; c < K.n_child; c++) {   // GetChilds()
                    const int v = A.V.d_children[K.child_start + c];
                    if (!view_present(A.V, v)) { fl |= ORBM_LM_BAD_INDEX; continue; }
                    if ((A.V.d_kf[v].flags & ORBM_LM_KF_BAD) || W.listed[v]) continue;
                    push(v);
                    break;
                }
            const int par = K.parent;   // GetParent(): not tested for isBad(), and its break leaves this loop (:3203-3212)
            if (par != -1) {
                if (!view_present(A.V, par)) fl |= ORBM_LM_BAD_INDEX;
                else if (!W.listed[par]) { push(par); break; }
            }
        }
        // inertial tail (:3217-3236): a listed tempKeyFrame is not advanced, so the rounds after it do nothing
        const orbm_localmap_frame F = A.frames[b];
        if ((F.flags & ORBM_LM_INERTIAL) && n < 80) {
            int t = F.last_kf;
            for (int i = 0; i < 20 && t != -1; i++) {
                if (!view_present(A.V, t)) { fl |= ORBM_LM_BAD_INDEX; break; }
                if (W.listed[t]) break;
                push(t);
                t = A.V.d_kf[t].prev;
            }
        }
        const unsigned long long best = *sbest;
        const bool over = n > A.O.cap_kf;
        if (over) fl |= ORBM_LM_KF_OVERFLOW;
        A.O.d_n_local_kf_required[b] = n;
        A.O.d_n_local_kf[b] = over ? A.O.cap_kf : n;
        A.O.d_ref_kf[b] = best ? A.V.d_kf_by_order[0xFFFFFFFFu - (uint32_t)best] : -1;   // pKFmax (:3239)
        A.O.d_max_votes[b] = (int)(best >> 32);
        A.O.d_nmp[b] = 0;              // k_lm_points_write overwrites both where the frame has segments
        A.O.d_nmp_required[b] = 0;
        *sflags = fl;
        sn[0] = n < n_kf ? n : n_kf;
        sn[1] = over ? 0 : sn[0];
        W.hdr[LM_HDR_NSEG] = sn[1];
    }
    __syncthreads();

    const int n = sn[0], nseg = sn[1];
    for (int s = tid; s < n && s < A.O.cap_kf; s += 256) A.O.d_local_kf[(size_t)b * A.O.cap_kf + s] = W.list[s];
    // UpdateLocalPoints walks the list in reverse: segment s = list[nseg - 1 - s]; seg_off = the exclusive scan of the feature counts
    bad = 0;
    uint32_t run = 0;
    for (int c0 = 0, it = 0; c0 < nseg; c0 += 256, it++) {
        const int s = c0 + tid;
        int row0, nf = 0;
        if (s < nseg && !view_rows(A.V, W.list[nseg - 1 - s], &row0, &nf)) bad = ORBM_LM_BAD_INDEX;
        uint32_t tot;   // (the offsets are keys of an unsigned atomicMax: the sum is in uint32_t)
        const uint32_t pre = wg_scan_value<4>((uint32_t)nf, wtot, it, &tot);
        if (s < nseg) W.seg_off[s] = (int32_t)(run + pre);
        run += tot;
    }
    if (bad) atomicOr(sflags, bad);
    __syncthreads();
    if (tid == 0) A.O.d_flags[b] = *sflags;
}

// one workgroup per (segment, frame)
struct LmSegment { int row0, nf; uint32_t off; bool live; };
static __device__ __forceinline__ LmSegment lm_segment(const LmArgs& A, const LmWork& W, int s) {
    LmSegment S;
    S.row0 = S.nf = 0;
    S.off = 0;
    const int nseg = W.hdr[LM_HDR_NSEG];
    S.live = s < nseg;
    if (S.live) {
        view_rows(A.V, W.list[nseg - 1 - s], &S.row0, &S.nf);
        S.off = (uint32_t)W.seg_off[s];
    }
    return S;
}

static __global__ __launch_bounds__(256) void k_lm_points_first(LmArgs A) {
    const int s = blockIdx.x, b = blockIdx.y;
    const LmWork W = lm_work(A, b);
    const LmSegment S = lm_segment(A, W, s);
    if (!S.live) return;
    uint32_t bad = 0;
    for (int i = threadIdx.x; i < S.nf; i += 256) {
        const int p = A.V.d_kf_mp[S.row0 + i];
        if (p == -1) continue;
        if (!view_point_ok(A.V, p)) { bad = ORBM_LM_BAD_INDEX; continue; }
        if (A.V.d_mp[p].flags & ORBM_MP_BAD) continue;   // !pMP->isBad() (:3028)
        atomicMax(&W.first[p], lm_key(S.off + (uint32_t)i));
    }
    if (bad) atomicOr(&A.O.d_flags[b], bad);
}

// the point of occurrence i of segment S where UpdateLocalPoints lists it there, else -1 (only usable occurrences wrote a key)
static __device__ __forceinline__ int lm_winner(const LmArgs& A, const LmWork& W, const LmSegment& S, int i) {
    if (i >= S.nf) return -1;
    const int p = A.V.d_kf_mp[S.row0 + i];
    return (p >= 0 && p < A.V.n_mp && W.first[p] == lm_key(S.off + (uint32_t)i)) ? p : -1;
}

static __global__ __launch_bounds__(256) void k_lm_points_count(LmArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* red = (int*)orb_smem;
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const LmWork W = lm_work(A, b);
    const LmSegment S = lm_segment(A, W, s);
    if (!S.live) return;
    int mine = 0;
    for (int i = tid; i < S.nf; i += 256) mine += lm_winner(A, W, S, i) >= 0 ? 1 : 0;
    if (tid == 0) red[0] = 0;
    __syncthreads();
    if (mine) atomicAdd(red, mine);
    __syncthreads();
    if (tid == 0) W.seg_cnt[s] = red[0];
}

static __global__ __launch_bounds__(256) void k_lm_points_write(LmArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* wtot = (int*)orb_smem;   // [2][4] per-wave totals by chunk parity; [8] points before this segment, [9] points of the frame
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const LmWork W = lm_work(A, b);
    const LmSegment S = lm_segment(A, W, s);
    if (!S.live) return;
    const int nseg = W.hdr[LM_HDR_NSEG], cap_mp = A.O.cap_mp;
    if (tid == 0) wtot[8] = wtot[9] = 0;
    __syncthreads();
    int before = 0, all = 0;
    for (int j = tid; j < nseg; j += 256) { const int c = W.seg_cnt[j]; all += c; before += j < s ? c : 0; }
    if (before) atomicAdd(&wtot[8], before);
    if (all) atomicAdd(&wtot[9], all);
    __syncthreads();
    int base = wtot[8];
    const int total = wtot[9];
    if (s == 0 && tid == 0) {
        A.O.d_nmp_required[b] = total;
        A.O.d_nmp[b] = total < cap_mp ? total : cap_mp;
        if (total > cap_mp) atomicOr(&A.O.d_flags[b], ORBM_LM_MP_OVERFLOW);
    }
    const size_t o0 = (size_t)b * cap_mp;
    const orbm_track* slab = A.V.d_mp_track + (size_t)b * (size_t)A.V.track_stride;
    for (int c0 = 0, it = 0; c0 < S.nf && base < cap_mp; c0 += 256, it++) {
        const int p = lm_winner(A, W, S, c0 + tid);
        const bool keep = p >= 0;
        int tot;
        const int j = base + wg_scan_ballot<4>(keep, wtot, it, &tot);
        if (keep && j >= 0 && j < cap_mp) {
            const uint32_t mk = W.mark[p];
            const uint4* src = (const uint4*)(A.V.d_mp + p);
            const uint4 r0 = src[0], r1 = src[1], r2s = src[2];
            const uint4 r2 = make_uint4(r2s.x, r2s.y, r2s.z, r2s.w | (mk ? ORBM_MP_SEEN : 0u));   // flags: mnLastFrameSeen == mCurrentFrame.mnId
            uint4* dst = (uint4*)(A.O.d_local_mp + o0 + j);
            dst[0] = r0; dst[1] = r1; dst[2] = r2;
            const uint4* ts = (const uint4*)(slab + p);
            const uint4 t0 = ts[0], t1s = ts[1];
            // a dropped point has mbTrackInView = false; the marking loop clears mbTrackInViewR, NOT mbTrackInView (:2869), so a point of the
            // frame list keeps the in_view an earlier frame left
            const uint4 t1 = make_uint4(t1s.x, t1s.y, (mk & LM_MARK_DROPPED) ? 0u : t1s.z, t1s.w);   // in_view
            uint4* td = (uint4*)(A.O.d_track + o0 + j);
            td[0] = t0; td[1] = t1;
            A.O.d_local_src[o0 + j] = p;
        }
        base += tot;
    }
}

struct LmStoreArgs {
    const orbm_track* track;
    const int32_t* src;
    const int32_t* nmp;
    int cap_mp;
    orbm_track* slab;
    int track_stride, n_mp;
};

static __global__ __launch_bounds__(256) void k_lm_store_tracks(LmStoreArgs A) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= lm_clamp(A.nmp[b], A.cap_mp)) return;
    const size_t o = (size_t)b * A.cap_mp + j;
    const int p = A.src[o];
    if (p < 0 || p >= A.n_mp) return;
    const uint4* s = (const uint4*)(A.track + o);
    uint4* d = (uint4*)(A.slab + (size_t)b * (size_t)A.track_stride + p);
    const uint4 a = s[0], c = s[1];
    d[0] = a; d[1] = c;
}

static __global__ __launch_bounds__(256) void k_lm_clear(uint4* p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

static size_t lm_work_words(int n_kf, int n_mp) { LmWork W; return lm_work_layout(n_kf, n_mp, nullptr, W); }

extern "C" size_t orbm_local_map_workspace_bytes(int n_kf, int n_mp, int batch) {
    if (n_kf < 0 || n_mp < 0 || batch < 0) return 0;
    return (size_t)batch * lm_work_words(n_kf, n_mp) * sizeof(int32_t);
}

extern "C" int orbm_update_local_map(const orbm_localmap_view* view, const orbm_localmap_frame* d_frames, const orbm_localmap_lists* lists,
                                     int batch, const orbm_localmap_out* out, void* d_work, void* stream) {
    if (!view || !d_frames || !lists || !out || !d_work || batch < 0) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    const orbm_localmap_lists& L = *lists;
    const orbm_localmap_out& O = *out;
    if (view_invalid(V, VIEW_ALL) || V.n_children < 0 || V.track_stride < 0) return ORB_E_INVALID;
    if ((!V.d_mp_track && V.n_mp) || (!V.d_kf_by_order && V.n_kf) || (!V.d_children && V.n_children)) return ORB_E_INVALID;
    if ((V.track_stride == 0 && batch > 1) || (V.track_stride != 0 && V.track_stride < V.n_mp)) return ORB_E_INVALID;
    if (!L.d_vote_mp || !L.d_n_vote || !L.d_frame_mp || !L.d_n_frame || L.cap_f < 1) return ORB_E_INVALID;
    if (L.d_dropped_mp && (!L.d_n_dropped || L.cap_dropped < 1)) return ORB_E_INVALID;
    if (!O.d_local_kf || !O.d_n_local_kf || !O.d_n_local_kf_required || !O.d_ref_kf || !O.d_max_votes || !O.d_local_src || !O.d_nmp ||
        !O.d_nmp_required || !O.d_local_mp || !O.d_track || !O.d_flags || O.cap_kf < 1 || O.cap_mp < 1)
        return ORB_E_INVALID;
    if (misaligned16(V.d_mp_track) || misaligned16(O.d_local_mp) || misaligned16(O.d_track) || misaligned16(d_work))
        return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    LmArgs A;
    A.V = V; A.frames = d_frames; A.L = L; A.O = O; A.work = (int32_t*)d_work; A.work_stride = lm_work_words(V.n_kf, V.n_mp);
    hipStream_t st = (hipStream_t)stream;
    const size_t n16 = orbm_local_map_workspace_bytes(V.n_kf, V.n_mp, batch) / 16;
    hipLaunchKernelGGL(k_lm_clear, dim3((unsigned)(n16 + 255 < 1024 * 256 ? (n16 + 255) / 256 : 1024)), dim3(256), 0, st, (uint4*)d_work, n16);
    hipLaunchKernelGGL(k_lm_keyframes, dim3(batch), dim3(256), 64, st, A);
    const int segs = O.cap_kf < V.n_kf ? O.cap_kf : V.n_kf;   // a frame whose list does not fit cap_kf has no segments
    if (segs > 0) {
        hipLaunchKernelGGL(k_lm_points_first, dim3(segs, batch), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_lm_points_count, dim3(segs, batch), dim3(256), 4, st, A);
        hipLaunchKernelGGL(k_lm_points_write, dim3(segs, batch), dim3(256), 10 * 4, st, A);
    }
    return launch_status();
}

extern "C" int orbm_store_local_tracks(const orbm_track* d_track, const int32_t* d_local_src, const int32_t* d_nmp, int cap_mp, int batch,
                                       orbm_track* d_mp_track, int track_stride, int n_mp, void* stream) {
    if (!d_track || !d_local_src || !d_nmp || !d_mp_track || cap_mp < 1 || batch < 0 || n_mp < 0 || track_stride < 0) return ORB_E_INVALID;
    if ((track_stride == 0 && batch > 1) || (track_stride != 0 && track_stride < n_mp)) return ORB_E_INVALID;
    if (misaligned16(d_track) || misaligned16(d_mp_track)) return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    LmStoreArgs A;
    A.track = d_track; A.src = d_local_src; A.nmp = d_nmp; A.cap_mp = cap_mp; A.slab = d_mp_track; A.track_stride = track_stride; A.n_mp = n_mp;
    hipLaunchKernelGGL(k_lm_store_tracks, dim3((cap_mp + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, A);
    return launch_status();
}
