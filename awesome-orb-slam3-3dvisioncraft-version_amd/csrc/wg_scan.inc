// wg_scan.inc — the ordered scan / compaction step of a workgroup of NW waves, as the map-side kernels (orbm_*.hip) take it once per chunk of
// 64 * NW items: the exclusive position of this lane's item among the chunk's items, in lane order, and the chunk's total.  The caller keeps
// its own running base across chunks, its capacity test and its writes.
//
// The contract, for both forms:
//   * EVERY lane of the workgroup calls, under workgroup-uniform control flow: there is exactly one __syncthreads inside.
//   * `scratch` is 2 * NW words of LDS that nothing else touches while a chunk loop runs: two sets of NW per-wave totals.
//   * `chunk` is the loop's chunk counter: consecutive calls without another workgroup barrier between them alternate its parity, and the call
//     takes the set `chunk & 1`.
//   * Why one barrier is enough.  Call k writes its set before its barrier B(k) and reads it after B(k).  The next writer of that set is call
//     k + 2, and a wave gets there only through B(k + 1), which no wave passes before every wave has arrived at it, its reads of call k behind
//     it in program order.  So a third call may overwrite the first call's totals with no second barrier.  With ONE set, call k + 1's write
//     would race the reads a slower wave still owes call k: the parity double-buffer is what buys the single barrier.
#ifndef ORB_WG_SCAN_INC
#define ORB_WG_SCAN_INC

// the per-wave totals of set `t` -> those of the waves before wave `wv`, and their sum
template <int NW, typename T> static __device__ __forceinline__ T wg_scan_waves(const T* t, int wv, T* total) {
    T off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { const T c = t[w]; off += w < wv ? c : (T)0; tot += c; }
    *total = tot;
    return off;
}

// Ballot step: a flag per lane -> the kept lanes of the chunk before this one (in-wave prefix = popcount of the ballot below the lane)
template <int NW> static __device__ __forceinline__ int wg_scan_ballot(bool keep, int* scratch, int chunk, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    int* t = scratch + (chunk & 1) * NW;
    if (lane == 0) t[wv] = __popcll(m);
    __syncthreads();
    return wg_scan_waves<NW>(t, wv, total) + __popcll(m & ((1ull << lane) - 1ull));
}

// Value step: an integer per lane (int32_t, or uint32_t where the sum is meant to wrap) -> the sum of the values of the lanes before this one
template <int NW, typename T> static __device__ __forceinline__ T wg_scan_value(T v, int* scratch, int chunk, T* total) {
    static_assert(sizeof(T) == sizeof(int), "the scratch is 2 * NW 32-bit words");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    T* t = (T*)scratch + (chunk & 1) * NW;
    if (lane == 63) t[wv] = inc;
    __syncthreads();
    return wg_scan_waves<NW>(t, wv, total) + inc - v;
}
#endif
