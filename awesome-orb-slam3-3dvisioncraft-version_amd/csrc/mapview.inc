// mapview.inc — the checked reads of an orbm_localmap_view (include/orbhip.h "Local map") that the map-side kernels (orbm_localmap, _covis,
// _culling, _fuse_neighbors, _newkeyframe) share, and the host-side tests their entry points open with.  These are the checks that decide
// which indices raise a kernel's *_BAD_INDEX / *_UNSUPPORTED flag rather than fault: a key frame, its rows, a point, a point's CSR range, an
// observation record, the rows a call can use.  A caller adds the flag of its own, the test is written here once.  Beside them the two
// smallest shared pieces: the nObs weight of a feature byte and the or into a flag word.  (Included after orbhip.h.)
#ifndef ORB_MAPVIEW_INC
#define ORB_MAPVIEW_INC
#include <climits>

// key frame v can be read: in range and present
static __device__ __forceinline__ bool view_present(const orbm_localmap_view& V, int v) {
    return v >= 0 && v < V.n_kf && (V.d_kf[v].flags & ORBM_LM_KF_PRESENT);
}

// the usable rows of a (readable) key frame in d_kf_mp and the tables beside it: false (and no rows) where they leave the table
static __device__ __forceinline__ bool view_rows(const orbm_localmap_view& V, int kf, int* row0, int* nf) {
    const int r = V.d_kf[kf].mp_row0, n = V.d_kf[kf].n_feat;
    const bool ok = r >= 0 && n >= 0 && n <= V.n_kf_mp_rows - r;
    *row0 = ok ? r : 0;
    *nf = ok ? n : 0;
    return ok;
}

// the CSR range of point p (in range): false where it leaves [0, n_obs]
static __device__ __forceinline__ bool view_obs_range(const orbm_localmap_view& V, int p, int* s, int* e) {
    *s = V.d_obs_start[p];
    *e = V.d_obs_start[p + 1];
    return *s >= 0 && *e >= *s && *e <= V.n_obs;
}

// point p can be read: in range and a filled slot (the caller decides what -1, "none", means to it before it asks)
static __device__ __forceinline__ bool view_point_ok(const orbm_localmap_view& V, int p) {
    return p >= 0 && p < V.n_mp && (V.d_mp[p].flags & ORBM_MP_VALID);
}

// The check of an observation record before anything reads through it: a rig record is unsupported; its key frame must be present and keep
// its rows inside d_kf_mp; its descriptor row must be one of that key frame's features (d_ckf is parallel to d_kf).
// -> the d_kf_mp row of the record's feature and *idx = the feature's index in its key frame, or a negative reason
enum { VIEW_REC_RIG = -1, VIEW_REC_BAD_INDEX = -2 };
static __device__ __forceinline__ int view_record_row(const orbm_localmap_view& V, const orbm_cull_keyframe* d_ckf, const orbm_observation& r,
                                                      int* idx) {
    if (r.flags & ORBM_OBS_RIGHT) return VIEW_REC_RIG;
    int row0, nf;
    if (!view_present(V, r.kf) || !view_rows(V, r.kf, &row0, &nf)) return VIEW_REC_BAD_INDEX;
    const long long i = (long long)r.desc_row - (long long)d_ckf[r.kf].desc_row0;
    if (i < 0 || i >= nf) return VIEW_REC_BAD_INDEX;
    *idx = (int)i;
    return row0 + (int)i;
}

// what view_record_row returned as the caller's own flag bits (0 for a row)
static __device__ __forceinline__ uint32_t view_record_flag(int row, uint32_t unsupported, uint32_t bad_index) {
    return row >= 0 ? 0u : row == VIEW_REC_RIG ? unsupported : bad_index;
}

// the rows of a (readable) key frame that a call with room for cap_feat features can use: its d_kf_mp rows, no more than cap_feat of them,
// and its descriptor rows from *drow0 inside the n_kf_desc_rows of the slab: false (and *nf = 0) otherwise
static __device__ __forceinline__ bool view_call_rows(const orbm_localmap_view& V, const orbm_cull_keyframe* d_ckf, int kf, int cap_feat,
                                                      int n_kf_desc_rows, int* row0, int* nf, int* drow0) {
    *drow0 = d_ckf[kf].desc_row0;
    if (!view_rows(V, kf, row0, nf) || *nf > cap_feat || *drow0 < 0 || *nf > n_kf_desc_rows - *drow0) { *nf = 0; return false; }
    return true;
}

// AddObservation's weight of a feature in nObs (MapPoint.cc:191-194), from its ORBM_CULL_FEAT_* byte
static __device__ __forceinline__ int view_feat_weight(uint32_t feat) { return (feat & ORBM_CULL_FEAT_STEREO) ? 2 : 1; }

// what a lane found wrong, or-ed into a flag word that several lanes write
static __device__ __forceinline__ void flag_or(int32_t* word, uint32_t bad) {
    if (bad) atomicOr((uint32_t*)word, bad);
}

// A word that the launch itself changed earlier (with atomics, which are performed in L2, or from another wave) and reads again: a relaxed
// atomic load is not served by a line the CU's L1 still holds from before the change, a plain load may be
static __device__ __forceinline__ uint32_t ld_relaxed(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
static __device__ __forceinline__ int32_t ld_relaxed(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// rank[k] = the rank of key frame k in d_kf_by_order (std::map<KeyFrame*, .> order), by ONE workgroup of 256 whose every lane calls under
// uniform control flow (two barriers inside).  A key frame without a rank (d_kf_by_order is not a permutation) goes behind every ranked one,
// by slot.  -> this lane met an entry out of range or a present key frame without a rank
static __device__ __forceinline__ bool view_build_ranks(const orbm_localmap_view& V, int32_t* rank) {
    const int tid = threadIdx.x, n_kf = V.n_kf;
    bool bad = false;
    for (int k = tid; k < n_kf; k += 256) rank[k] = INT_MAX;
    __syncthreads();
    for (int r = tid; r < n_kf; r += 256) {
        const int k = V.d_kf_by_order[r];
        if (k < 0 || k >= n_kf) bad = true;
        else atomicMin(&rank[k], r);
    }
    __syncthreads();
    for (int k = tid; k < n_kf; k += 256)
        if (ld_relaxed(&rank[k]) == INT_MAX) {
            rank[k] = n_kf + k;
            if (V.d_kf[k].flags & ORBM_LM_KF_PRESENT) bad = true;
        }
    return bad;
}

// ------------------------------------------------------------------------------------------------ host
// the kernels move records and descriptor rows with 16-byte loads / stores
static bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// what an entry point returns after its launches
static int launch_status() { return hipGetLastError() == hipSuccess ? ORB_OK : ORB_E_HIP; }

// The view's common members: a negative count, a null table in `need` with a count above zero (d_obs_start has n_mp + 1 entries: never null),
// or a d_mp off 16 bytes.  What only one entry point reads (d_kf_by_order, d_children, d_mp_track, ...) it tests itself.
enum : unsigned { VIEW_OBS_START = 1u, VIEW_MP = 2u, VIEW_OBS = 4u, VIEW_KF = 8u, VIEW_KF_MP = 16u, VIEW_ALL = 31u };
static bool view_invalid(const orbm_localmap_view& V, unsigned need) {
    if (V.n_mp < 0 || V.n_obs < 0 || V.n_kf < 0 || V.n_kf_mp_rows < 0) return true;
    if ((need & VIEW_OBS_START) && !V.d_obs_start) return true;
    if ((need & VIEW_MP) && !V.d_mp && V.n_mp) return true;
    if ((need & VIEW_OBS) && !V.d_obs && V.n_obs) return true;
    if ((need & VIEW_KF) && !V.d_kf && V.n_kf) return true;
    if ((need & VIEW_KF_MP) && !V.d_kf_mp && V.n_kf_mp_rows) return true;
    return misaligned16(V.d_mp);
}
#endif
