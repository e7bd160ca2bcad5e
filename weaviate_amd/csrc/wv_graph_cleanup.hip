// wv_graph_cleanup.hip -- removing deleted nodes from the resident graph
// (wv_index_cleanup_tombstones; CleanUpTombstonedNodes, delete.go:177-224).
// D is the set of tombstoned ids below the graph's n, as a bitmap.  The
// passes outside the searches (the re-link search and the list replacement sit
// with search_layer and heuristic_select in wv_hnsw.hip):
//
//   wv_cleanup_flag_kernel      connectionsPointTo (delete.go:378-388): one wave
//                               per 64 consecutive nodes; for each live one the
//                               lanes read its layer-0 list, then the strip of
//                               its upper lists, coalesced, test D's bitmap, and
//                               a ballot gives the node's flag.  The wave stores
//                               its 64 flags as one word and their count.
//   wv_cleanup_scatter_kernel   after an exclusive scan of the counts: every
//                               wave writes its flagged ids at its offset, lane
//                               order = id order, so the list is ascending with
//                               no atomic deciding a position.
//   wv_cleanup_strike_kernel    one wave per member whose search overflowed:
//                               D's ids leave each of its lists, the rest moves
//                               up in stored order (ballot + prefix count), the
//                               tail is padded.
//   wv_cleanup_ep_kernel        findNewGlobalEntrypoint's outcome
//                               (delete.go:422-478): the minimum over the live
//                               nodes of (top - level, id), per block and then
//                               over the blocks' keys.
//   wv_cleanup_remove_kernel    one wave per bitmap word of D: the nodes become
//                               nil (level -1, lists padded) and their
//                               tombstone bits are cleared.
//
// Plain loads and vector stores; every order is fixed by position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wv_device.h"
#include "wv_launch.h"

namespace wv {

constexpr int GC_WAVES = 4;   // waves per workgroup
constexpr uint64_t GC_NO_KEY = ~0ull;

__device__ __forceinline__ void gc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// any of list[0..len) in D (wave-uniform result)
__device__ __forceinline__ bool gc_points_to_dead(const CleanupParams& c, const uint32_t* list, int len, int lane) {
    bool hit = false;
    for (int i = lane; i < len; i += 64) {
        const uint32_t v = list[i];
        hit = hit || (v != WV_NIL && bit_test(c.dead, c.n, v));
    }
    return __any(hit);
}

// the upper lists a node of this level owns inside the level stride
__device__ __forceinline__ int gc_upper_lists(const CleanupParams& c, int level) {
    return level < c.upper_levels ? level : c.upper_levels;
}

__global__ __launch_bounds__(64 * GC_WAVES) void wv_cleanup_flag_kernel(CleanupParams c) {
    const uint64_t w = (uint64_t)blockIdx.x * GC_WAVES + (threadIdx.x >> 6);
    if (w * 64 >= c.n) return;   // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint64_t mine = w * 64 + lane;
    int lvl = -1;
    if (mine < c.n && !bit_test(c.dead, c.n, mine)) lvl = c.levels[mine];
    uint64_t todo = __ballot(lvl >= 0);   // the live nodes of this wave
    uint64_t flags = 0;
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint64_t node = w * 64 + j;
        const int level = __shfl(lvl, j, 64);
        bool hit = gc_points_to_dead(c, c.layer0 + node * (uint64_t)c.deg0, c.deg0, lane);
        if (!hit && level > 0) {
            const uint32_t row = c.upper_row[node];
            if (row != WV_NIL)
                hit = gc_points_to_dead(c, c.upper + (uint64_t)row * c.upper_levels * c.degU,
                                        gc_upper_lists(c, level) * c.degU, lane);
        }
        if (hit) flags |= 1ull << j;
    }
    if (lane == 0) {
        c.wave_mask[w] = flags;
        c.wave_cnt[w] = (uint32_t)__popcll(flags);
    }
}

__global__ __launch_bounds__(64 * GC_WAVES) void wv_cleanup_scatter_kernel(CleanupParams c) {
    const uint64_t w = (uint64_t)blockIdx.x * GC_WAVES + (threadIdx.x >> 6);
    if (w * 64 >= c.n) return;
    const int lane = threadIdx.x & 63;
    const uint64_t flags = c.wave_mask[w];
    if ((flags >> lane) & 1ull) c.flagged[c.wave_off[w] + mbcnt64(flags)] = (uint32_t)(w * 64 + lane);
}

// D's ids leave list[0..deg), deg <= 256: the kept ids move up in stored order
__device__ __forceinline__ void gc_strike_list(const CleanupParams& c, uint32_t* list, int deg, int lane) {
    uint32_t v[4];
    bool keep[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = q * 64 + lane;
        v[q] = i < deg ? list[i] : WV_NIL;
        keep[q] = v[q] != WV_NIL && !bit_test(c.dead, c.n, v[q]);
    }
    gc_wave_sync();   // the whole list is in registers before any of it is overwritten
    int out = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t m = __ballot(keep[q]);
        if (keep[q]) list[out + mbcnt64(m)] = v[q];   // out + rank <= q * 64 + lane < deg
        out += __popcll(m);
    }
    for (int i = out + lane; i < deg; i += 64) list[i] = WV_NIL;
}

__global__ __launch_bounds__(64 * GC_WAVES) void wv_cleanup_strike_kernel(CleanupParams c) {
    const uint64_t f = (uint64_t)blockIdx.x * GC_WAVES + (threadIdx.x >> 6);
    if (f >= c.n_flagged || c.status[f] == 0) return;
    const int lane = threadIdx.x & 63;
    const uint64_t node = c.flagged[f];
    const int level = c.levels[node];
    gc_strike_list(c, c.layer0 + node * (uint64_t)c.deg0, c.deg0, lane);
    const uint32_t row = c.upper_row[node];
    if (level < 1 || row == WV_NIL) return;
    const int lists = gc_upper_lists(c, level);
    for (int l = 0; l < lists; ++l)
        gc_strike_list(c, c.upper + ((uint64_t)row * c.upper_levels + l) * c.degU, c.degU, lane);
}

// (level descending, id ascending) as one ascending key; levels above the
// searched top count as the top
__device__ __forceinline__ uint64_t gc_ep_key(const CleanupParams& c, uint64_t node) {
    if (bit_test(c.dead, c.n, node)) return GC_NO_KEY;
    const int level = c.levels[node];
    if (level < 0) return GC_NO_KEY;
    const int below = c.max_level - (level < c.max_level ? level : c.max_level);
    return ((uint64_t)below << 32) | node;
}

__device__ __forceinline__ uint64_t gc_block_min(uint64_t key, uint64_t* lds) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor((unsigned long long)key, o, 64);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = key;
    __syncthreads();
    key = lds[0];
    for (int i = 1; i < GC_WAVES; ++i) key = lds[i] < key ? lds[i] : key;
    return key;
}

// stage 0: block b's minimum over its nodes -> ep_part[1 + b]; stage 1 (one
// block): the minimum of those -> ep_part[0]
__global__ __launch_bounds__(64 * GC_WAVES) void wv_cleanup_ep_kernel(CleanupParams c, int stage) {
    __shared__ uint64_t lds[GC_WAVES];
    uint64_t key = GC_NO_KEY;
    if (stage == 0) {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gridDim.x * blockDim.x) {
            const uint64_t k = gc_ep_key(c, i);
            key = k < key ? k : key;
        }
    } else {
        for (int i = threadIdx.x; i < c.ep_blocks; i += blockDim.x) {
            const uint64_t k = c.ep_part[1 + i];
            key = k < key ? k : key;
        }
    }
    key = gc_block_min(key, lds);
    if (threadIdx.x == 0) c.ep_part[stage == 0 ? 1 + blockIdx.x : 0] = key;
}

__global__ __launch_bounds__(64 * GC_WAVES) void wv_cleanup_remove_kernel(CleanupParams c) {
    const uint64_t w = (uint64_t)blockIdx.x * GC_WAVES + (threadIdx.x >> 6);
    if (w * 64 >= c.n) return;
    const int lane = threadIdx.x & 63;
    const uint64_t word = c.dead[w];
    uint64_t todo = word;
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint64_t node = w * 64 + j;   // (< n: D holds no bit at or above n)
        const int level = c.levels[node];
        uint32_t* l0 = c.layer0 + node * (uint64_t)c.deg0;
        for (int i = lane; i < c.deg0; i += 64) l0[i] = WV_NIL;
        const uint32_t row = level >= 1 ? c.upper_row[node] : WV_NIL;
        if (row != WV_NIL) {
            uint32_t* up = c.upper + (uint64_t)row * c.upper_levels * c.degU;
            for (int i = lane; i < c.upper_levels * c.degU; i += 64) up[i] = WV_NIL;
        }
        gc_wave_sync();   // the level was read by every lane before it goes
        if (lane == 0) c.levels[node] = -1;
    }
    if (lane == 0 && word) c.tomb[w] &= ~word;
}

}  // namespace wv

extern "C" {

static bool gc_shape_ok(const wv::CleanupParams* c) {
    return c->n > 0 && c->deg0 >= 1 && c->deg0 <= 256 && c->degU >= 1 && c->degU <= 256 && c->upper_levels >= 1 &&
           (c->n + 63) / 64 / wv::GC_WAVES < 0x7FFFFFFFull;
}
static unsigned gc_word_blocks(const wv::CleanupParams* c) {
    return (unsigned)(((c->n + 63) / 64 + wv::GC_WAVES - 1) / wv::GC_WAVES);
}

// wave_mask / wave_cnt[w] for the (n + 63) / 64 waves of 64 nodes
hipError_t wv_launch_cleanup_flag(const wv::CleanupParams* c, hipStream_t s) {
    if (!gc_shape_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_cleanup_flag_kernel, dim3(gc_word_blocks(c)), dim3(64 * wv::GC_WAVES), 0, s, *c);
    return hipGetLastError();
}

// flagged[] from wave_mask and wave_off (the exclusive scan of wave_cnt)
hipError_t wv_launch_cleanup_scatter(const wv::CleanupParams* c, hipStream_t s) {
    if (!gc_shape_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_cleanup_scatter_kernel, dim3(gc_word_blocks(c)), dim3(64 * wv::GC_WAVES), 0, s, *c);
    return hipGetLastError();
}

hipError_t wv_launch_cleanup_strike(const wv::CleanupParams* c, hipStream_t s) {
    if (c->n_flagged == 0) return hipSuccess;
    if (!gc_shape_ok(c)) return hipErrorInvalidValue;
    const unsigned blocks = (c->n_flagged + wv::GC_WAVES - 1) / wv::GC_WAVES;
    hipLaunchKernelGGL(wv::wv_cleanup_strike_kernel, dim3(blocks), dim3(64 * wv::GC_WAVES), 0, s, *c);
    return hipGetLastError();
}

int wv_cleanup_entrypoint_blocks(uint64_t n) {
    const uint64_t per_block = 64 * wv::GC_WAVES * 16;
    return (int)std::min<uint64_t>(1024, std::max<uint64_t>(1, (n + per_block - 1) / per_block));
}

// ep_part[0] = (max_level - level) << 32 | id of the new entrypoint, ~0: no live node
hipError_t wv_launch_cleanup_entrypoint(const wv::CleanupParams* c, hipStream_t s) {
    if (!gc_shape_ok(c) || c->ep_blocks != wv_cleanup_entrypoint_blocks(c->n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_cleanup_ep_kernel, dim3(c->ep_blocks), dim3(64 * wv::GC_WAVES), 0, s, *c, 0);
    hipLaunchKernelGGL(wv::wv_cleanup_ep_kernel, dim3(1), dim3(64 * wv::GC_WAVES), 0, s, *c, 1);
    return hipGetLastError();
}

hipError_t wv_launch_cleanup_remove(const wv::CleanupParams* c, hipStream_t s) {
    if (!gc_shape_ok(c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::wv_cleanup_remove_kernel, dim3(gc_word_blocks(c)), dim3(64 * wv::GC_WAVES), 0, s, *c);
    return hipGetLastError();
}

}  // extern "C"
