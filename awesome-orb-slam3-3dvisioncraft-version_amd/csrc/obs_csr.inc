// obs_csr.inc — the rebuild of the observation CSR (d_obs_start_out / d_obs_out) that closes every map-side step (orbm_culling.hip,
// orbm_fuse_neighbors.hip, orbm_newkeyframe.hip), in three launches of 256-lane workgroups over `blk`, csr_blk_words(n_mp) words of workspace:
//   count   a workgroup per block of 256 points: csr_count(rows of this lane's point)             -> blk[b] = the rows of block b
//   scan    ONE workgroup: csr_scan_blocks -> blk[j] = the rows before block j, and the total, which the caller stores to blk[nblk] and
//           holds against its capacity: overflow is decided here, before anything is written
//   place   a workgroup per block again: csr_place(the same row count) -> where this lane's rows go; it writes d_obs_start_out
// The caller owns how many rows its point has (0 for a lane past n_mp), how it emits them from the returned position, and what an overflow
// suppresses: it passes `fits` to csr_place and may read the total back with csr_total.
//
// The contract (wg_scan.inc's, at NW = 4):
//   * EVERY lane of the 256 calls, under workgroup-uniform control flow: each helper holds exactly one __syncthreads per chunk
//     (csr_count and csr_place take one chunk; csr_scan_blocks one per 256 blocks).  A call inside `if (blockIdx.x < n)` is legal: the
//     condition is uniform.  k_cull_apply_write does that, its grid has other duties beyond the point blocks.
//   * `scratch` is wg_scan.inc's 2 * 4 words of LDS.  csr_count and csr_place use set 0 and must be the kernel's only scan; csr_scan_blocks
//     threads the caller's chunk counter through, so the caller can keep scanning on the same scratch behind it (k_nk_select, k_mc_compact).
#ifndef ORB_OBS_CSR_INC
#define ORB_OBS_CSR_INC
#include "wg_scan.inc"

static __host__ __device__ __forceinline__ int csr_blocks(int n_mp) { return n_mp / 256 + (n_mp % 256 ? 1 : 0); }
static __host__ __device__ __forceinline__ size_t csr_blk_words(int n_mp) { return (size_t)csr_blocks(n_mp) + 1; }

// count: n = the rows of point blockIdx.x * 256 + threadIdx.x
static __device__ __forceinline__ void csr_count(int n, int32_t* blk, int* scratch) {
    int tot;
    wg_scan_value<4>(n, scratch, 0, &tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// scan, by one workgroup: blk[j] becomes the rows before block j.  -> the total.  `chunk` is the caller's chunk counter of wg_scan.inc
static __device__ __forceinline__ int csr_scan_blocks(int32_t* blk, int nblk, int* scratch, int* chunk) {
    int run = 0;
    for (int c0 = 0; c0 < nblk; c0 += 256, (*chunk)++) {
        const int j = c0 + threadIdx.x;
        const int v = j < nblk ? blk[j] : 0;
        int tot;
        const int pre = wg_scan_value<4>(v, scratch, *chunk, &tot);
        if (j < nblk) blk[j] = run + pre;
        run += tot;
    }
    return run;
}

// the total the scan launch's caller stored
static __device__ __forceinline__ int csr_total(const int32_t* blk, int nblk) { return blk[nblk]; }

// place: n as in the count launch.  -> the position of the point's first row.  Where the CSR fits: start_out[g], the closing start_out[n_mp]
// from the last point, and the single zero of a map without points
static __device__ __forceinline__ int csr_place(int n, const int32_t* blk, int n_mp, bool fits, int32_t* start_out, int* scratch) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    int tot;
    const int at = blk[blockIdx.x] + wg_scan_value<4>(n, scratch, 0, &tot);
    if (fits && g < n_mp) {
        start_out[g] = at;
        if (g == n_mp - 1) start_out[n_mp] = at + n;
    }
    if (fits && n_mp == 0 && g == 0) start_out[0] = 0;
    return at;
}
#endif
