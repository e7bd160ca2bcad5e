// wv_graph_grow.hip -- what an existing graph needs before the batched insert
// (wv_hnsw.hip, "GPU graph construction") can continue from it
// (wv_index_extend_graph):
//
//   wv_list_counts_kernel   the link kernel appends to a neighbour's list at
//                           its count (connectNeighborAtLevel,
//                           neighbor_connections.go:151-157); a graph that was
//                           uploaded, or whose buffers moved, has no counts, so
//                           they are read off the lists: a list is a dense
//                           prefix padded with 0xFFFFFFFF, its count the
//                           entries before the first pad.
//   wv_upper_relay_kernel   `upper` is [n_upper][upper_levels][M]; a new node
//                           above the old top widens the level stride, so every
//                           old (row, level) list moves to its place in the new
//                           array (padded beforehand), and its count with it.
//
// One wave per list in both; plain loads and vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wv_launch.h"

namespace wv {

constexpr uint32_t GG_NIL = 0xFFFFFFFFu;
constexpr int GG_WAVES = 4;   // lists per workgroup

__global__ __launch_bounds__(64 * GG_WAVES) void wv_list_counts_kernel(const uint32_t* __restrict__ lists,
                                                                       uint64_t n_lists, int deg,
                                                                       uint32_t* __restrict__ counts) {
    const uint64_t l = (uint64_t)blockIdx.x * GG_WAVES + (threadIdx.x >> 6);
    if (l >= n_lists) return;   // (whole waves leave: l is wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t* row = lists + l * (uint64_t)deg;
    int first = deg;   // the lowest pad this lane saw
    for (int i = lane; i < deg; i += 64)
        if (row[i] == GG_NIL) { first = i; break; }
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (lane == 0) counts[l] = (uint32_t)first;
}

__global__ __launch_bounds__(64 * GG_WAVES) void wv_upper_relay_kernel(const uint32_t* __restrict__ old_upper,
                                                                       const uint32_t* __restrict__ old_counts,
                                                                       uint64_t n_rows, int old_levels, int new_levels,
                                                                       int deg, uint32_t* __restrict__ new_upper,
                                                                       uint32_t* __restrict__ new_counts) {
    const uint64_t l = (uint64_t)blockIdx.x * GG_WAVES + (threadIdx.x >> 6);
    if (l >= n_rows * (uint64_t)old_levels) return;
    const int lane = threadIdx.x & 63;
    const uint64_t r = l / (uint64_t)old_levels;
    const int level = (int)(l % (uint64_t)old_levels);
    if (level >= new_levels) return;   // (the stride never shrinks; kept for the bound)
    const uint64_t d = r * (uint64_t)new_levels + level;
    const uint32_t* src = old_upper + l * (uint64_t)deg;
    uint32_t* dst = new_upper + d * (uint64_t)deg;
    for (int i = lane; i < deg; i += 64) dst[i] = src[i];
    if (lane == 0) new_counts[d] = old_counts[l];
}

}  // namespace wv

extern "C" {

// counts[l] = entries of lists[l][0..deg) before the first 0xFFFFFFFF
hipError_t wv_launch_list_counts(const uint32_t* lists, uint64_t n_lists, int deg, uint32_t* counts, hipStream_t s) {
    if (n_lists == 0) return hipSuccess;
    const uint64_t blocks = (n_lists + wv::GG_WAVES - 1) / wv::GG_WAVES;
    if (deg < 1 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_list_counts_kernel, dim3((unsigned)blocks), dim3(64 * wv::GG_WAVES), 0, s, lists, n_lists,
                       deg, counts);
    return hipGetLastError();
}

// [n_rows][old_levels][deg] -> [..][new_levels][deg] (new_levels >= old_levels,
// the new arrays padded by the caller), the per-list counts the same way
hipError_t wv_launch_upper_relay(const uint32_t* old_upper, const uint32_t* old_counts, uint64_t n_rows, int old_levels,
                                 int new_levels, int deg, uint32_t* new_upper, uint32_t* new_counts, hipStream_t s) {
    const uint64_t n_lists = n_rows * (uint64_t)old_levels;
    if (n_lists == 0) return hipSuccess;
    const uint64_t blocks = (n_lists + wv::GG_WAVES - 1) / wv::GG_WAVES;
    if (deg < 1 || old_levels < 1 || new_levels < old_levels || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_upper_relay_kernel, dim3((unsigned)blocks), dim3(64 * wv::GG_WAVES), 0, s, old_upper,
                       old_counts, n_rows, old_levels, new_levels, deg, new_upper, new_counts);
    return hipGetLastError();
}

}  // extern "C"
