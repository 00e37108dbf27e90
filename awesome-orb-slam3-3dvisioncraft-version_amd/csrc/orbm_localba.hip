// orbm_localba.hip — the two halves of Optimizer::LocalBundleAdjustment around the solver, on the device map for gfx950 (include/orbhip.h
// "Local bundle adjustment on the device map"): the window selection and graph flattening (Optimizer.cc:1816-1945, :1978-2190) before
// lba_optimize, and the outlier pass, erase loop and write-back (:2293-2510) after it.
//
// Form (DESIGN.md "Local bundle adjustment").  Lane-per-item kernels, stable compactions by one workgroup (wg_scan.inc), the out-CSR by
// obs_csr.inc's three launches.  A lane walks the records of ITS point.  What is serial in the reference is either order-free here (a mark
// per key frame, a first occurrence per point by an integer atomicMin of the position) or short and run by one lane (the num_fixedKF < 2
// branch).  The record check and the point test are mapview.inc's.
//   orbm_lba_window_build, 8 launches:
//     k_lb_init        first[p] = none, the marks, the header
//     k_lb_local       one workgroup: lLocalKeyFrames from the ordered row (first place of a key frame by atomicMin), the feature offsets
//     k_lb_feat        a lane per feature of the local key frames in list order: atomicMin(first[p], position)
//     k_lb_points      one workgroup: lLocalMapPoints = the features that are their point's first, in order
//     k_lb_fixed       a lane per local point: the fixed marks, the edges it will have
//     k_lb_poses       one workgroup: num_fixedKF and its branch, the vertices ranked by id, the edge starts, the overflow decision, the poses
//     k_lb_edges       a lane per local point: its vertex and its edges, the per-pose counts
//     k_lb_pose_edges  a workgroup per pose: its edge list ascending (a ballot scan over the edge chunks); the result words
//   orbm_lba_window_apply, 8 launches:
//     k_la_init, k_la_outliers (one workgroup: vToErase, mono then stereo, the majority rule), k_la_erase (a lane per local point: its
//     pairs in order, SetBadFlag, d_ref, pos), k_la_count (the rows per point; a lane per pose: Rcw | tcw | Ow), k_la_scan (the block sums,
//     the points that went bad, the result words), k_la_write (the out-CSR), orbm_refresh_map_points (two launches, orbm_refresh.hip
//     unchanged) over the local points on the out-CSR.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/orbhip.h"
#include "mapview.inc"
#include "obs_csr.inc"
#include "workspace.inc"

enum {
    LB_H_FLAGS = 0, LB_H_NLOCAL, LB_H_NFEAT, LB_H_NPOINTS, LB_H_NEDGES, LB_H_NMONO, LB_H_NSTEREO, LB_H_NFIXED, LB_H_NUMFIXED, LB_H_NPOSES,
    LB_H_OVERFLOW, LB_H_NLOCAL_FINAL,
    LA_H_NERASE, LA_H_EARLY, LA_H_NMONO, LA_H_NSTEREO, LA_H_NBAD, LA_H_NOBS,
    LB_H_WORDS = 32
};
enum : int32_t { LB_M_LOCAL = 1, LB_M_LISTED = 2, LB_M_FIXED = 4 };   // mnBALocalForKF; in lLocalKeyFrames; in lFixedCameras

struct LbWork {
    int32_t* hdr;
    int32_t *kfmark, *kfpos;   // per key frame: LB_M_*; the least row position that names it, later its vertex rank
    int32_t *llist, *foff;     // lLocalKeyFrames before the branch; the features before list entry j
    int32_t *first, *featp;    // per point: the least feature position holding it; per feature position: its point or -1
    int32_t *plist, *ecount;   // lLocalMapPoints; per list entry: its edges, later its first edge
    int32_t *vlist, *pcount;   // the vertices by slot; per rank: its edges
    uint8_t *eout, *recdead;   // apply: the edge is an outlier; the record died
    int32_t *ndead, *blk;      // apply: per point the records that died (-1: all, the point went bad); obs_csr.inc's block sums
    int32_t* best;
    uint32_t* status;
    int32_t* sel;              // apply: the local points the refresh reads, all -1 on the early return
};

struct LbSizes { int n_kf, n_mp, n_obs, n_rows, cap_conn, cap_p, cap_l, cap_e; };

// The workspace, listed once.  -> its bytes (a multiple of 16)
static __host__ __device__ __forceinline__ size_t lb_work_layout(const LbSizes& S, unsigned char* base, LbWork& W) {
    const size_t nk = (size_t)S.n_kf, nm = (size_t)S.n_mp;
    WsCursor c{base, 16, 0};
    W.hdr = c.take<int32_t>(LB_H_WORDS);
    W.kfmark = c.take<int32_t>(nk);
    W.kfpos = c.take<int32_t>(nk);
    W.llist = c.take<int32_t>((size_t)S.cap_conn + 1);
    W.foff = c.take<int32_t>((size_t)S.cap_conn + 2);
    W.first = c.take<int32_t>(nm);
    W.featp = c.take<int32_t>((size_t)S.n_rows);
    W.plist = c.take<int32_t>(nm);
    W.ecount = c.take<int32_t>(nm);
    W.vlist = c.take<int32_t>(nk);
    W.pcount = c.take<int32_t>(nk);
    W.eout = c.take<uint8_t>((size_t)S.cap_e);
    W.recdead = c.take<uint8_t>((size_t)S.n_obs);
    W.ndead = c.take<int32_t>(nm);
    W.blk = c.take<int32_t>(csr_blk_words(S.n_mp));
    W.best = c.take<int32_t>(nm);
    W.status = c.take<uint32_t>(nm);
    W.sel = c.take<int32_t>((size_t)S.cap_l);
    return c.off;
}

struct LbArgs {
    orbm_localmap_view V;
    orbm_lba_in I;
    orbm_lba_window O;
    orbm_lba_apply P;
    const double *chi2, *depth;
    unsigned char* work;
    int cur;
    uint32_t init_id;
};

static __host__ __device__ __forceinline__ LbSizes lb_sizes(const LbArgs& A) {
    return LbSizes{A.V.n_kf, A.V.n_mp, A.V.n_obs, A.V.n_kf_mp_rows, A.I.cap_conn, A.O.cap_p, A.O.cap_l, A.O.cap_e};
}
static __device__ __forceinline__ LbWork lb_work(const LbArgs& A) {
    LbWork W;
    lb_work_layout(lb_sizes(A), A.work, W);
    return W;
}
static __device__ __forceinline__ void lb_flag(const LbWork& W, uint32_t bad) { flag_or(&W.hdr[LB_H_FLAGS], bad); }
static __device__ __forceinline__ int lb_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the d_kf_mp row of a record's feature if the record can be used, else negative and flagged
static __device__ __forceinline__ int lb_record_row(const LbArgs& A, const orbm_observation& r, uint32_t* bad) {
    int idx;
    const int row = view_record_row(A.V, A.I.d_ckf, r, &idx);
    *bad |= view_record_flag(row, ORBM_LBA_UNSUPPORTED, ORBM_LBA_BAD_INDEX);
    return row;
}
static __device__ __forceinline__ bool lb_same_map(const LbArgs& A, int k) { return !A.I.d_map || A.I.d_map[k].map_id == A.I.d_map[A.cur].map_id; }
// the key frame of a usable record takes an edge: !pKFi->isBad() && pKFi->GetMap() == pCurrentMap
static __device__ __forceinline__ bool lb_kf_in_graph(const LbArgs& A, int k) { return !(A.V.d_kf[k].flags & ORBM_LM_KF_BAD) && lb_same_map(A, k); }
static __device__ __forceinline__ int lb_weight(const LbArgs& A, int row) { return A.I.d_u_right[row] >= 0.f ? 2 : 1; }

// ------------------------------------------------------------------------------------------------ the build
static __global__ __launch_bounds__(256) void k_lb_init(LbArgs A) {
    const LbWork W = lb_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < A.V.n_mp) W.first[g] = INT_MAX;
    if (g < A.V.n_kf) { W.kfmark[g] = 0; W.kfpos[g] = INT_MAX; W.pcount[g] = 0; }
    if (blockIdx.x == 0 && threadIdx.x < LB_H_WORDS) W.hdr[threadIdx.x] = 0;
}

// one workgroup of 256: Optimizer.cc:1816-1829.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_lb_local(LbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const LbWork W = lb_work(A);
    const int tid = threadIdx.x, cur = A.cur;
    int row0, nf_cur;
    if (!view_present(A.V, cur) || !view_rows(A.V, cur, &row0, &nf_cur)) {   // (uniform) nothing is built
        if (tid == 0) lb_flag(W, ORBM_LBA_BAD_INDEX);
        return;
    }
    uint32_t bad = 0;
    const int n_raw = A.I.d_n_ordered[cur], n_ord = lb_clamp(n_raw, A.I.cap_conn);
    if (n_raw != n_ord && tid == 0) bad |= ORBM_LBA_BAD_INDEX;
    const int32_t* row = A.I.d_ordered_kf + (size_t)cur * A.I.cap_conn;
    if (tid == 0) { W.kfpos[cur] = -1; W.kfmark[cur] = LB_M_LOCAL | LB_M_LISTED; W.llist[0] = cur; W.foff[0] = 0; }
    __threadfence();   // (the -1 is in place before a row that names current_kf takes its atomicMin)
    __syncthreads();
    for (int r = tid; r < n_ord; r += 256) {
        const int k = row[r];
        if (view_present(A.V, k)) atomicMin(&W.kfpos[k], r);
        else bad |= ORBM_LBA_BAD_INDEX;
    }
    __threadfence();
    __syncthreads();
    int n = 1, nfeat = nf_cur, it = 0;
    for (int c0 = 0; c0 < n_ord; c0 += 256) {
        const int r = c0 + tid, k = r < n_ord ? row[r] : -1;
        bool listed = false;
        int nf = 0;
        if (k >= 0 && view_present(A.V, k) && ld_relaxed(&W.kfpos[k]) == r) {
            listed = lb_kf_in_graph(A, k);
            W.kfmark[k] = LB_M_LOCAL | (listed ? LB_M_LISTED : 0);
            int r0;
            if (listed && !view_rows(A.V, k, &r0, &nf)) bad |= ORBM_LBA_BAD_INDEX;
        }
        int tot, totf;
        const int at = n + wg_scan_ballot<4>(listed, scan, it++, &tot);
        const int fo = nfeat + wg_scan_value<4>(nf, scan, it++, &totf);
        if (listed) { W.llist[at] = k; W.foff[at] = fo; }
        n += tot;
        nfeat += totf;
    }
    if (tid == 0) {
        W.foff[n] = nfeat;
        // (key frames whose rows overlap could name more features than the table has rows: the positions past it are dropped)
        if (nfeat > A.V.n_kf_mp_rows) { bad |= ORBM_LBA_BAD_INDEX; nfeat = A.V.n_kf_mp_rows; }
        W.hdr[LB_H_NLOCAL] = n;
        W.hdr[LB_H_NFEAT] = nfeat;
    }
    lb_flag(W, bad);
}

// grid x over the rows of d_kf_mp: feature position g of the local key frames in list order (:1835-1862)
static __global__ __launch_bounds__(256) void k_lb_feat(LbArgs A) {
    const LbWork W = lb_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= W.hdr[LB_H_NFEAT]) return;
    int lo = 0, hi = W.hdr[LB_H_NLOCAL];   // the last list entry whose offset is <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (W.foff[mid] <= g) lo = mid; else hi = mid;
    }
    const int kf = W.llist[lo];
    int row0, nf;
    view_rows(A.V, kf, &row0, &nf);   // (k_lb_local checked them)
    const int p = A.V.d_kf_mp[row0 + (g - W.foff[lo])];
    int keep = -1;
    if (p != -1) {
        if (!view_point_ok(A.V, p)) lb_flag(W, ORBM_LBA_BAD_INDEX);
        else if (!(A.V.d_mp[p].flags & ORBM_MP_BAD)) { keep = p; atomicMin(&W.first[p], g); }
    }
    W.featp[g] = keep;
}

// one workgroup of 256.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_lb_points(LbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const LbWork W = lb_work(A);
    const int nfeat = W.hdr[LB_H_NFEAT];
    int n = 0;
    for (int c0 = 0, it = 0; c0 < nfeat; c0 += 256, it++) {
        const int g = c0 + threadIdx.x, p = g < nfeat ? W.featp[g] : -1;
        const bool keep = p >= 0 && W.first[p] == g;
        int tot;
        const int at = n + wg_scan_ballot<4>(keep, (int*)orb_smem, it, &tot);
        if (keep) W.plist[at] = p;
        n += tot;
    }
    if (threadIdx.x == 0) W.hdr[LB_H_NPOINTS] = n;
}

// The records of local point p that become edges, in CSR order: f(o, row, k, stereo, octave) per edge.  FIXED: also mark the key frames that
// are fixed (:1864-1882).  -> the edges
template <bool FIXED, typename F> static __device__ __forceinline__ int lb_walk_edges(const LbArgs& A, const LbWork& W, int p, uint32_t* bad, F f) {
    int s, e, cnt = 0;
    if (!view_obs_range(A.V, p, &s, &e)) { *bad |= ORBM_LBA_BAD_INDEX; return 0; }
    for (int o = s; o < e; o++) {
        const orbm_observation r = A.V.d_obs[o];
        const int row = lb_record_row(A, r, bad);
        if (row < 0 || !lb_kf_in_graph(A, r.kf)) continue;
        if (FIXED && !(W.kfmark[r.kf] & (LB_M_LOCAL | LB_M_FIXED))) atomicOr(&W.kfmark[r.kf], (int32_t)LB_M_FIXED);
        const int octave = A.I.d_kps[row].octave;
        if (octave < 0 || octave >= A.I.nlevels) { *bad |= ORBM_LBA_BAD_INDEX; continue; }
        f(o, row, r.kf, octave);
        cnt++;
    }
    return cnt;
}

// grid x over the blocks of 256 points: local point l
static __global__ __launch_bounds__(256) void k_lb_fixed(LbArgs A) {
    const LbWork W = lb_work(A);
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= W.hdr[LB_H_NPOINTS]) return;
    uint32_t bad = 0;
    W.ecount[l] = lb_walk_edges<true>(A, W, W.plist[l], &bad, [](int, int, int, int) {});
    lb_flag(W, bad);
}

// LbaLinearizer::poseFromTcw (Converter::toSE3Quat: Eigen Quaterniond(Matrix3d) + SE3Quat::normalizeRotation), operation for operation
static __device__ __forceinline__ void lb_pose_from_tcw(const orbm_fusenb_pose& T, double* out7) {
    double m[9], q[4];
    for (int i = 0; i < 9; i++) m[i] = (double)T.Rcw[i];
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        double qi = 0.5 * t;
        t = 0.5 / t;
        const double qw = (m[k * 3 + j] - m[j * 3 + k]) * t, qj = (m[j * 3 + i] + m[i * 3 + j]) * t, qk = (m[k * 3 + i] + m[i * 3 + k]) * t;
        q[0] = i == 0 ? qi : j == 0 ? qj : qk;
        q[1] = i == 1 ? qi : j == 1 ? qj : qk;
        q[2] = i == 2 ? qi : j == 2 ? qj : qk;
        q[3] = qw;
    }
    if (q[3] < 0) for (int c = 0; c < 4; c++) q[c] = -q[c];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int r = 0; r < 3; r++) out7[r] = (double)T.tcw[r];
    for (int c = 0; c < 4; c++) out7[3 + c] = q[c] / n;
}

// one workgroup of 256.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_lb_poses(LbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const LbWork W = lb_work(A);
    const int tid = threadIdx.x, n_kf = A.V.n_kf, n_local = W.hdr[LB_H_NLOCAL], n_points = W.hdr[LB_H_NPOINTS];
    int it = 0, n_fixed = 0, init_local = 0;
    for (int c0 = 0; c0 < n_kf; c0 += 256) {
        const int k = c0 + tid;
        int tot;
        wg_scan_ballot<4>(k < n_kf && (W.kfmark[k] & LB_M_FIXED), scan, it++, &tot);
        n_fixed += tot;
    }
    for (int c0 = 0; c0 < n_local; c0 += 256) {
        const int j = c0 + tid;
        int tot;
        wg_scan_ballot<4>(j < n_local && A.I.d_ckf[W.llist[j]].id == A.init_id, scan, it++, &tot);
        init_local |= tot > 0;
    }
    int num_fixed = n_fixed + init_local, n_moved = 0;
    if (num_fixed < 2 && n_local > 0) {   // :1906-1945, kept literally; every lane walks, lane 0 writes
        int lower = (int)A.I.d_ckf[A.cur].id, second = lower, k_lower = -1, k_second = -1;
        for (int j = 0; j < n_local; j++) {
            const int k = W.llist[j], id = (int)A.I.d_ckf[k].id;
            if (k == A.cur || A.I.d_ckf[k].id == A.init_id) continue;
            if (id < lower) { lower = id; k_lower = k; }
            else if (id < second) { second = id; k_second = k; }
        }
        if (k_lower >= 0) {
            if (tid == 0) W.kfmark[k_lower] = LB_M_LOCAL | LB_M_FIXED;
            num_fixed++; n_moved++;
            if (num_fixed < 2 && k_second >= 0) {
                if (tid == 0) W.kfmark[k_second] = LB_M_LOCAL | LB_M_FIXED;
                num_fixed++; n_moved++;
            }
        }
    }
    __threadfence();
    __syncthreads();
    int nv = 0;   // the vertices by slot
    for (int c0 = 0; c0 < n_kf; c0 += 256) {
        const int k = c0 + tid;
        const bool v = k < n_kf && (ld_relaxed(&W.kfmark[k]) & (LB_M_LISTED | LB_M_FIXED));
        int tot;
        const int at = nv + wg_scan_ballot<4>(v, scan, it++, &tot);
        if (v) W.vlist[at] = k;
        nv += tot;
    }
    int n_edges = 0;   // the first edge of every point
    for (int c0 = 0; c0 < n_points; c0 += 256) {
        const int l = c0 + tid, c = l < n_points ? W.ecount[l] : 0;
        int tot;
        const int pre = wg_scan_value<4>(c, scan, it++, &tot);
        if (l < n_points) W.ecount[l] = n_edges + pre;
        n_edges += tot;
    }
    const bool overflow = nv > A.O.cap_p || n_points > A.O.cap_l || n_edges > A.O.cap_e;   // decided before anything is written
    if (tid == 0) {
        W.hdr[LB_H_NFIXED] = n_fixed + n_moved;
        W.hdr[LB_H_NUMFIXED] = num_fixed;
        W.hdr[LB_H_NLOCAL_FINAL] = n_local - n_moved;
        W.hdr[LB_H_NPOSES] = nv;
        W.hdr[LB_H_NEDGES] = n_edges;
        W.hdr[LB_H_OVERFLOW] = overflow;
        if (overflow) lb_flag(W, ORBM_LBA_OVERFLOW);
    }
    if (overflow) return;
    __threadfence();
    __syncthreads();
    // the rank of every vertex by (mnId, slot): g2o's block order, kfById of the glue
    for (int v = tid; v < nv; v += 256) {
        const int k = ld_relaxed(&W.vlist[v]);
        const uint32_t id = A.I.d_ckf[k].id;
        int rank = 0;
        for (int u = 0; u < nv; u++) {
            const uint32_t idu = A.I.d_ckf[ld_relaxed(&W.vlist[u])].id;
            rank += idu < id || (idu == id && u < v);
        }
        W.kfpos[k] = rank;
        A.O.d_pose_kf[rank] = k;
        A.O.d_pose_local[rank] = (ld_relaxed(&W.kfmark[k]) & LB_M_LISTED) ? 1 : 0;
        lb_pose_from_tcw(A.I.d_pose[k], A.O.poses + (size_t)rank * 7);
    }
    __threadfence();
    __syncthreads();
    int n_free = 0;   // pose_hidx: a running index over the free vertices in rank order
    for (int c0 = 0; c0 < nv; c0 += 256) {
        const int i = c0 + tid;
        bool fr = false;
        if (i < nv) {
            const int k = ld_relaxed(&A.O.d_pose_kf[i]);
            fr = (ld_relaxed(&W.kfmark[k]) & LB_M_LISTED) && A.I.d_ckf[k].id != A.init_id;
        }
        int tot;
        const int at = n_free + wg_scan_ballot<4>(fr, scan, it++, &tot);
        if (i < nv) A.O.pose_hidx[i] = fr ? at : -1;
        n_free += tot;
    }
    for (int i = nv + tid; i < A.O.cap_p; i += 256) { A.O.pose_hidx[i] = -1; A.O.d_pose_kf[i] = -1; A.O.d_pose_local[i] = 0; }
}

// grid x over max(n_mp, cap_l + 1): local point l, its vertex and its edges (:2060-2190); the tails of lm_start and d_point_mp
static __global__ __launch_bounds__(256) void k_lb_edges(LbArgs A) {
    const LbWork W = lb_work(A);
    if (W.hdr[LB_H_OVERFLOW]) return;
    const int l = blockIdx.x * 256 + threadIdx.x, n_points = W.hdr[LB_H_NPOINTS], n_edges = W.hdr[LB_H_NEDGES];
    if (l >= n_points) {
        if (l <= A.O.cap_l) A.O.lm_start[l] = n_edges;
        if (l < A.O.cap_l) A.O.d_point_mp[l] = -1;
        return;
    }
    const int p = W.plist[l];
    int e = W.ecount[l], n_mono = 0, n_stereo = 0;
    A.O.lm_start[l] = e;
    A.O.d_point_mp[l] = p;
    for (int i = 0; i < 3; i++) A.O.points[(size_t)l * 3 + i] = (double)A.V.d_mp[p].pos[i];
    uint32_t ignore = 0;   // (k_lb_fixed flagged what cannot be read)
    lb_walk_edges<false>(A, W, p, &ignore, [&](int o, int row, int k, int octave) {
        const float ur = A.I.d_u_right[row];
        const bool mono = ur < 0.f;
        const int rank = W.kfpos[k];
        lba_edge ed;
        ed.pose = rank; ed.point = l;
        ed.kind = mono ? LBA_EDGE_MONO : LBA_EDGE_STEREO; ed.cam = 0;
        ed.obs[0] = A.I.d_kps[row].x; ed.obs[1] = A.I.d_kps[row].y; ed.obs[2] = mono ? 0.f : ur;
        ed.inv_sigma2 = A.I.inv_level_sigma2[octave];
        A.O.edges[e] = ed;
        A.O.d_edge_rec[e] = o;
        e++;
        atomicAdd(&W.pcount[rank], 1);
        if (mono) n_mono++; else n_stereo++;
    });
    if (n_mono) atomicAdd(&W.hdr[LB_H_NMONO], n_mono);
    if (n_stereo) atomicAdd(&W.hdr[LB_H_NSTEREO], n_stereo);
}

// grid x over cap_p + 1: pose blockIdx.x, its edges ascending; block 0 also writes the counts and the result words.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_lb_pose_edges(LbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const LbWork W = lb_work(A);
    const int i = blockIdx.x, tid = threadIdx.x;
    const bool overflow = W.hdr[LB_H_OVERFLOW] != 0;
    if (i == 0 && tid == 0) {
        int32_t* R = A.O.d_result;
        for (int w = 0; w < ORBM_LBA_R_WORDS; w++) R[w] = 0;
        R[ORBM_LBA_R_FLAGS] = W.hdr[LB_H_FLAGS];
        R[ORBM_LBA_R_N_POSES_REQUIRED] = W.hdr[LB_H_NPOSES];
        R[ORBM_LBA_R_N_POINTS_REQUIRED] = W.hdr[LB_H_NPOINTS];
        R[ORBM_LBA_R_N_EDGES_REQUIRED] = W.hdr[LB_H_NEDGES];
        if (!overflow) {
            R[ORBM_LBA_R_N_LOCAL] = W.hdr[LB_H_NLOCAL_FINAL];
            R[ORBM_LBA_R_N_FIXED] = W.hdr[LB_H_NFIXED];
            R[ORBM_LBA_R_NUM_FIXED_KF] = W.hdr[LB_H_NUMFIXED];
            R[ORBM_LBA_R_N_POINTS] = W.hdr[LB_H_NPOINTS];
            R[ORBM_LBA_R_N_EDGES] = W.hdr[LB_H_NEDGES];
            R[ORBM_LBA_R_N_MONO] = W.hdr[LB_H_NMONO];
            R[ORBM_LBA_R_N_STEREO] = W.hdr[LB_H_NSTEREO];
            *A.O.n_poses = W.hdr[LB_H_NPOSES];
            *A.O.n_points = W.hdr[LB_H_NPOINTS];
            *A.O.n_edges = W.hdr[LB_H_NEDGES];
        }
    }
    if (overflow) return;
    const int n_poses = W.hdr[LB_H_NPOSES], n_edges = W.hdr[LB_H_NEDGES];
    if (i >= n_poses) {
        if (tid == 0) A.O.pose_start[i] = n_edges;
        return;
    }
    int mine = 0, start;
    for (int j = tid; j < i; j += 256) mine += W.pcount[j];
    wg_scan_value<4>(mine, scan, 0, &start);
    if (tid == 0) A.O.pose_start[i] = start;
    int run = 0;
    for (int c0 = 0, it = 1; c0 < n_edges; c0 += 256, it++) {
        const int e = c0 + tid;
        const bool keep = e < n_edges && A.O.edges[e].pose == i;
        int tot;
        const int at = start + run + wg_scan_ballot<4>(keep, scan, it, &tot);
        if (keep) A.O.pose_edges[at] = e;
        run += tot;
    }
}

// ------------------------------------------------------------------------------------------------ the apply
struct LaWin { int n_poses, n_points, n_edges; };
static __device__ __forceinline__ LaWin la_win(const LbArgs& A) {
    return LaWin{lb_clamp(*A.O.n_poses, A.O.cap_p), lb_clamp(*A.O.n_points, A.O.cap_l), lb_clamp(*A.O.n_edges, A.O.cap_e)};
}

static __global__ __launch_bounds__(256) void k_la_init(LbArgs A) {
    const LbWork W = lb_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < A.V.n_mp) W.ndead[g] = 0;
    if (g < A.V.n_obs) W.recdead[g] = 0;
    if (g < A.O.cap_e) W.eout[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x < LB_H_WORDS) W.hdr[threadIdx.x] = 0;
}

// one workgroup of 256: :2293-2352.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_la_outliers(LbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const LbWork W = lb_work(A);
    const LaWin N = la_win(A);
    const int tid = threadIdx.x;
    int it = 0, n_erase = 0, n_mono = 0;
    uint32_t bad = 0;
    for (int pass = 0; pass < 2; pass++)   // vpEdgesMono, then vpEdgesStereo
        for (int c0 = 0; c0 < N.n_edges; c0 += 256) {
            const int e = c0 + tid;
            bool mine = false, out = false;
            int kf = -1, mp = -1;
            if (e < N.n_edges) {
                const lba_edge ed = A.O.edges[e];
                const bool mono = ed.kind == LBA_EDGE_MONO;
                mine = mono == (pass == 0);
                if (ed.pose < 0 || ed.pose >= N.n_poses || ed.point < 0 || ed.point >= N.n_points) { if (mine) bad |= ORBM_LBA_BAD_INDEX; }
                else if (mine) {
                    out = A.chi2[e] > (mono ? 5.991 : 7.815) || !(A.depth[e] > 0.0);
                    kf = A.O.d_pose_kf[ed.pose];
                    mp = A.O.d_point_mp[ed.point];
                    if (out) W.eout[e] = 1;
                }
            }
            int tot, totm;
            const int at = n_erase + wg_scan_ballot<4>(out, scan, it++, &tot);
            wg_scan_ballot<4>(mine && pass == 0, scan, it++, &totm);
            if (out) { A.P.d_erased[2 * (size_t)at] = kf; A.P.d_erased[2 * (size_t)at + 1] = mp; }
            n_erase += tot;
            n_mono += totm;
        }
    if (tid == 0) {
        const int n_stereo = N.n_edges - n_mono;
        W.hdr[LA_H_NERASE] = n_erase;
        W.hdr[LA_H_NMONO] = n_mono;
        W.hdr[LA_H_NSTEREO] = n_stereo;
        // if (vToErase.size() >= (vpMapPointEdgeMono.size() + vpMapPointEdgeStereo.size()) * 0.5) return;
        W.hdr[LA_H_EARLY] = (double)n_erase >= (double)(n_mono + n_stereo) * 0.5;
    }
    lb_flag(W, bad);
}

// grid x over cap_l: local point l (:2375-2401 for its own pairs, :2499-2506)
static __global__ __launch_bounds__(256) void k_la_erase(LbArgs A) {
    const LbWork W = lb_work(A);
    const LaWin N = la_win(A);
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= A.O.cap_l) return;
    W.sel[l] = -1;
    if (W.hdr[LA_H_EARLY] || l >= N.n_points) return;
    const int p = A.O.d_point_mp[l];
    uint32_t bad = 0;
    int s, e;
    if (!view_point_ok(A.V, p) || !view_obs_range(A.V, p, &s, &e)) { lb_flag(W, ORBM_LBA_BAD_INDEX); return; }
    W.sel[l] = p;
    int nobs = 0;
    if (A.P.d_mp_nobs) nobs = A.P.d_mp_nobs[p];
    else
        for (int o = s; o < e; o++) {
            const int row = lb_record_row(A, A.V.d_obs[o], &bad);
            if (row >= 0) nobs += lb_weight(A, row);
        }
    const int e0 = lb_clamp(A.O.lm_start[l], N.n_edges), e1 = lb_clamp(A.O.lm_start[l + 1], N.n_edges), ref = A.P.d_ref[p].ref_kf;
    bool went_bad = false, ref_died = false;
    int nd = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int ei = e0; ei < e1; ei++) {
            if (!W.eout[ei] || (A.O.edges[ei].kind == LBA_EDGE_MONO) != (pass == 0) || went_bad) continue;   // (a bad point: GetIndexInKeyFrame is -1)
            const int o = A.O.d_edge_rec[ei];
            if (o < s || o >= e) { bad |= ORBM_LBA_BAD_INDEX; continue; }
            const orbm_observation r = A.V.d_obs[o];
            const int row = lb_record_row(A, r, &bad);
            if (row < 0 || W.recdead[o]) continue;
            A.P.d_kf_mp[row] = -1;    // pKFi->EraseMapPointMatch(pMPi)
            W.recdead[o] = 1;         // pMPi->EraseObservation(pKFi)
            nd++;
            nobs -= lb_weight(A, row);
            ref_died |= r.kf == ref;
            if (nobs <= 2) {          // SetBadFlag
                went_bad = true;
                for (int o2 = s; o2 < e; o2++) {
                    if (W.recdead[o2]) continue;
                    const int row2 = lb_record_row(A, A.V.d_obs[o2], &bad);
                    if (row2 >= 0) A.P.d_kf_mp[row2] = -1;
                }
            }
        }
    if (nd) {
        W.ndead[p] = went_bad ? -1 : nd;
        if (A.P.d_mp_nobs) A.P.d_mp_nobs[p] = nobs;
        const uint32_t f = A.P.d_mp[p].flags;
        A.P.d_mp[p].flags = (f & ~ORBM_MP_HAS_OBS) | (nobs > 0 ? ORBM_MP_HAS_OBS : 0u) | (went_bad ? ORBM_MP_BAD : 0u);
        if (!went_bad && ref_died)
            for (int o = s; o < e; o++) {
                if (W.recdead[o]) continue;
                const orbm_observation r = A.V.d_obs[o];
                const int row = lb_record_row(A, r, &bad);
                if (row < 0) continue;
                A.P.d_ref[p].ref_kf = r.kf;
                A.P.d_ref[p].level = A.I.d_kps[row].octave;
                break;
            }
    }
    for (int i = 0; i < 3; i++) A.P.d_mp[p].pos[i] = (float)A.O.points[(size_t)l * 3 + i];   // Converter::toCvMat(Eigen::Vector3d)
    lb_flag(W, bad);
}

// the rows point g has in the out-CSR, and its range in the view's
static __device__ __forceinline__ int la_rows(const LbArgs& A, const LbWork& W, int g, int* s, int* e, uint32_t* bad) {
    *s = *e = 0;
    if (!view_point_ok(A.V, g)) return 0;
    if (!view_obs_range(A.V, g, s, e)) { *bad |= ORBM_LBA_BAD_INDEX; *s = *e = 0; return 0; }
    const int nd = W.ndead[g];
    return nd < 0 ? 0 : *e - *s - nd;
}

// Converter::toCvMat(SE3Quat) -> KeyFrame::SetPose: Rcw | tcw as floats of to_homogeneous_matrix in double; Ow = -Rwc * tcw by one cv::gemm
static __device__ __forceinline__ void la_write_pose(const double* p7, orbm_fusenb_pose* T, orbm_keyframe_center* C) {
    const double x = p7[3], y = p7[4], z = p7[5], w = p7[6];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    float Rf[9], tf[3];
    for (int i = 0; i < 9; i++) Rf[i] = (float)R[i];
    for (int i = 0; i < 3; i++) tf[i] = (float)p7[i];
    for (int i = 0; i < 9; i++) T->Rcw[i] = Rf[i];
    for (int i = 0; i < 3; i++) T->tcw[i] = tf[i];
    for (int r = 0; r < 3; r++) {   // Rwc(r, k) = Rcw(k, r)
        double sum = (double)Rf[r] * (double)tf[0];
        sum += (double)Rf[3 + r] * (double)tf[1];
        sum += (double)Rf[6 + r] * (double)tf[2];
        const float ow = (float)(sum * -1.0);
        T->Ow[r] = ow;
        C->left[r] = ow;
    }
}

// grid x over max(the blocks of 256 points, the blocks of cap_p): the rows of point g; pose g (:2425-2433).  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_la_count(LbArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const LbWork W = lb_work(A);
    const LaWin N = la_win(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    uint32_t bad = 0;
    if ((int)blockIdx.x < nblk) {   // (uniform)
        int s, e;
        csr_count(la_rows(A, W, g, &s, &e, &bad), W.blk, (int*)orb_smem);
    }
    if (g < N.n_poses && !W.hdr[LA_H_EARLY] && A.O.d_pose_local[g]) {
        const int k = A.O.d_pose_kf[g];
        if (!view_present(A.V, k)) bad |= ORBM_LBA_BAD_INDEX;
        else la_write_pose(A.O.poses + (size_t)g * 7, &A.P.d_pose[k], &A.P.d_center[k]);
    }
    lb_flag(W, bad);
}

// one workgroup of 256.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_la_scan(LbArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    int* scan = (int*)orb_smem;
    const LbWork W = lb_work(A);
    const int tid = threadIdx.x, cap_l = A.O.cap_l;
    int it = 0, n_bad = 0;
    const int run = csr_scan_blocks(W.blk, nblk, scan, &it);
    for (int c0 = 0; c0 < cap_l; c0 += 256) {
        const int l = c0 + tid, p = l < cap_l ? W.sel[l] : -1;
        const bool wb = p >= 0 && W.ndead[p] < 0;
        int tot;
        const int at = n_bad + wg_scan_ballot<4>(wb, scan, it++, &tot);
        if (wb) A.P.d_went_bad[at] = p;
        n_bad += tot;
    }
    for (int l = n_bad + tid; l < cap_l; l += 256) A.P.d_went_bad[l] = -1;
    if (tid != 0) return;
    W.blk[nblk] = run;
    int32_t* R = A.P.d_result;
    for (int w = 0; w < ORBM_LBA_A_WORDS; w++) R[w] = 0;
    R[ORBM_LBA_A_FLAGS] = (int32_t)(ld_relaxed((uint32_t*)&W.hdr[LB_H_FLAGS]) | (W.hdr[LA_H_EARLY] ? ORBM_LBA_EARLY_RETURN : 0u));
    R[ORBM_LBA_A_N_ERASED] = W.hdr[LA_H_NERASE];
    R[ORBM_LBA_A_N_WENT_BAD] = n_bad;
    R[ORBM_LBA_A_N_OBS] = run;
    R[ORBM_LBA_A_N_MONO] = W.hdr[LA_H_NMONO];
    R[ORBM_LBA_A_N_STEREO] = W.hdr[LA_H_NSTEREO];
}

// grid x over the blocks of 256 points: the out-CSR.  orb_smem = int[8]
static __global__ __launch_bounds__(256) void k_la_write(LbArgs A, int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orb_smem[];
    const LbWork W = lb_work(A);
    const int g = blockIdx.x * 256 + threadIdx.x;
    uint32_t ignore = 0;
    int s, e;
    const int n = la_rows(A, W, g, &s, &e, &ignore);
    int at = csr_place(n, W.blk, A.V.n_mp, true, A.P.d_obs_start_out, (int*)orb_smem);
    if (g >= A.V.n_mp || n == 0) return;
    const bool some_dead = W.ndead[g] > 0;
    for (int o = s; o < e; o++)
        if (!some_dead || !W.recdead[o]) A.P.d_obs_out[at++] = A.V.d_obs[o];
}

// ------------------------------------------------------------------------------------------------ host
// (k_lb_local sums the feature counts of up to cap_conn + 1 key frames in an int, each at most n_rows even where damaged rows overlap:
//  sizes whose product leaves an int are refused)
static bool lb_sizes_ok(const LbSizes& S) {
    return S.n_kf >= 0 && S.n_mp >= 0 && S.n_obs >= 0 && S.n_rows >= 0 && S.cap_conn >= 1 && S.cap_p >= 1 && S.cap_l >= 1 && S.cap_e >= 1 &&
           ((long long)S.cap_conn + 1) * (long long)S.n_rows <= (long long)INT_MAX;
}

extern "C" size_t orbm_lba_workspace_bytes(int n_kf, int n_mp, int n_obs, int n_kf_mp_rows, int cap_conn, int cap_p, int cap_l, int cap_e) {
    const LbSizes S{n_kf, n_mp, n_obs, n_kf_mp_rows, cap_conn, cap_p, cap_l, cap_e};
    if (!lb_sizes_ok(S)) return 0;
    LbWork W;
    return lb_work_layout(S, nullptr, W);
}

static int lb_blocks(int n) { return n < 1 ? 1 : (n + 255) / 256; }
static int lb_max(int a, int b) { return a > b ? a : b; }

static bool lb_common_invalid(const orbm_localmap_view& V, const orbm_lba_in& I, const orbm_lba_window& O, const void* d_work) {
    if (view_invalid(V, VIEW_ALL) || misaligned16(d_work)) return true;
    const LbSizes S{V.n_kf, V.n_mp, V.n_obs, V.n_kf_mp_rows, I.cap_conn, O.cap_p, O.cap_l, O.cap_e};
    if (!lb_sizes_ok(S) || I.nlevels < 1 || I.nlevels > 16) return true;
    if ((V.n_kf && (!I.d_ckf || !I.d_pose || !I.d_ordered_kf || !I.d_n_ordered)) || (V.n_kf_mp_rows && (!I.d_kps || !I.d_u_right))) return true;
    if (!O.poses || !O.pose_hidx || !O.points || !O.edges || !O.lm_start || !O.pose_start || !O.pose_edges || !O.n_poses || !O.n_points ||
        !O.n_edges || !O.d_pose_kf || !O.d_pose_local || !O.d_point_mp || !O.d_edge_rec || !O.d_result)
        return true;
    return misaligned16(O.poses) || misaligned16(O.points);
}

extern "C" int orbm_lba_window_build(const orbm_localmap_view* view, const orbm_lba_in* in, int current_kf, uint32_t init_kf_id,
                                     const orbm_lba_window* out, void* d_work, void* stream) {
    if (!view || !in || !out || !d_work) return ORB_E_INVALID;
    if (lb_common_invalid(*view, *in, *out, d_work)) return ORB_E_INVALID;
    LbArgs A = {};
    A.V = *view; A.I = *in; A.O = *out; A.work = (unsigned char*)d_work; A.cur = current_kf; A.init_id = init_kf_id;
    const orbm_localmap_view& V = A.V;
    hipStream_t st = (hipStream_t)stream;
    const int gp = lb_blocks(V.n_mp);
    hipLaunchKernelGGL(k_lb_init, dim3(lb_blocks(lb_max(V.n_mp, V.n_kf))), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_lb_local, dim3(1), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_lb_feat, dim3(lb_blocks(V.n_kf_mp_rows)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_lb_points, dim3(1), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_lb_fixed, dim3(gp), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_lb_poses, dim3(1), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_lb_edges, dim3(lb_blocks(lb_max(V.n_mp, A.O.cap_l + 1))), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_lb_pose_edges, dim3(A.O.cap_p + 1), dim3(256), 32, st, A);
    return launch_status();
}

extern "C" int orbm_lba_window_apply(const orbm_localmap_view* view, const orbm_lba_in* in, const orbm_lba_window* win, const double* d_chi2,
                                     const double* d_depth, const orbm_lba_apply* apply, void* d_work, void* stream) {
    if (!view || !in || !win || !d_chi2 || !d_depth || !apply || !d_work) return ORB_E_INVALID;
    if (lb_common_invalid(*view, *in, *win, d_work)) return ORB_E_INVALID;
    const orbm_localmap_view& V = *view;
    const orbm_lba_apply& P = *apply;
    if (P.cap_obs_out < V.n_obs || !P.d_erased || !P.d_went_bad || !P.d_obs_start_out || (!P.d_obs_out && P.cap_obs_out) || !P.d_result)
        return ORB_E_INVALID;
    if ((V.n_mp && (!P.d_mp || !P.d_ref)) || (V.n_kf_mp_rows && !P.d_kf_mp) || (V.n_kf && (!P.d_pose || !P.d_center))) return ORB_E_INVALID;
    if (P.d_obs_start_out == V.d_obs_start || (P.d_obs_out && P.d_obs_out == V.d_obs) || misaligned16(P.d_mp)) return ORB_E_INVALID;
    LbArgs A = {};
    A.V = V; A.I = *in; A.O = *win; A.P = P; A.chi2 = d_chi2; A.depth = d_depth; A.work = (unsigned char*)d_work;
    LbWork W;
    lb_work_layout(lb_sizes(A), A.work, W);
    orbm_refresh_params rp = {};
    rp.what = ORBM_REFRESH_NORMAL_DEPTH;
    rp.nlevels = A.I.nlevels;
    for (int i = 0; i < 16; i++) rp.scale_factors[i] = A.I.scale_factors[i];

    hipStream_t st = (hipStream_t)stream;
    const int nblk = csr_blocks(V.n_mp), gp = nblk < 1 ? 1 : nblk;
    hipLaunchKernelGGL(k_la_init, dim3(lb_blocks(lb_max(lb_max(V.n_mp, V.n_obs), A.O.cap_e))), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_la_outliers, dim3(1), dim3(256), 32, st, A);
    hipLaunchKernelGGL(k_la_erase, dim3(lb_blocks(A.O.cap_l)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_la_count, dim3(lb_max(gp, lb_blocks(A.O.cap_p))), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL(k_la_scan, dim3(1), dim3(256), 32, st, A, nblk);
    hipLaunchKernelGGL(k_la_write, dim3(gp), dim3(256), 32, st, A, nblk);
    // (orbm_refresh_map_points refuses a null array even where nothing reads it: the workspace stands in.  Without ORBM_REFRESH_DESCRIPTOR
    //  no descriptor row is read or written, and the row bound only has to admit every record the view admits.  With n_mp == 0 it launches
    //  nothing)
    const void* w = d_work;
    const int rc = orbm_refresh_map_points(P.d_mp ? P.d_mp : (orbm_map_point*)d_work, V.n_mp, (uint8_t*)d_work, 0, W.sel, A.O.cap_l,
                                           P.d_obs_start_out, P.d_obs_out ? P.d_obs_out : (const orbm_observation*)w,
                                           P.d_ref ? P.d_ref : (const orbm_refresh_point*)w,
                                           P.d_center ? P.d_center : (const orbm_keyframe_center*)w, V.n_kf, (const uint8_t*)w, INT_MAX, &rp,
                                           W.best, W.status, stream);
    if (rc != ORB_OK) return rc;
    return launch_status();
}
