// wv_bigk_dev.h -- what the bound passes of the large-k route share
// (wv_bigk.hip, wv_bigk_kinds.hip): the orderable key of a sampled distance,
// the merge of a workgroup's four lists, and the sample walk of the kernels
// whose lanes own whole rows.
#pragma once
#include "wv_device.h"
#include "wv_params.h"
#include "wv_topk.h"

namespace wv {

constexpr uint32_t BIGK_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t BIGK_KEY_INF = 0xFF800000u;   // bigk_key(+inf)

// the distance's half of sbd_key: unsigned order = float order, -0 and +0 one key
__device__ __forceinline__ uint32_t bigk_key(float d) { return (uint32_t)(sbd_key(d, 0u) >> 32); }
__device__ __forceinline__ float bigk_unkey(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// the workgroup's four sorted lists into wave 0's (wl: [4][64]); the other
// waves' return value is their own list
__device__ __forceinline__ uint32_t bigk_merge_waves(uint32_t top, uint32_t (*wl)[64], int wave, int lane) {
    wl[wave][lane] = top;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) top = wave_min64_of(top, wl[w][lane], lane);
    }
    return top;
}

__device__ __forceinline__ void bigk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// A workgroup's walk over its segment of the sample when a lane owns whole
// rows (a serial chain per row: the PQ table sum, the manhattan and hamming
// sums).  A wave takes 64 samples a step, tests their bits and appends the
// survivors' rows to its queue in LDS (sid: 64 (R + 1) slots of the wave);
// once the queue holds 64 R rows, dist(sid, n, d) evaluates them -- d[r] the
// distance of slot lane + 64 r, slots < n -- so every evaluation but a
// segment's last runs with all lanes busy whatever share of the sample the
// allow list keeps.  The keys go into the wave's list as in bigk_bound_kernel
// and the segment writes its 64 smallest.
template <int R, class Dist>
__device__ __forceinline__ void bigk_walk(const BigkParams& p, uint32_t* sid, uint32_t (*wl)[64], Dist&& dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x, seg = blockIdx.y;
    const uint64_t* allow = p.allow ? p.allow + (p.allow_stride ? (uint64_t)q * p.allow_stride : 0) : nullptr;
    const uint64_t j_begin = (uint64_t)seg * p.samples_per_seg;
    uint64_t j_end = j_begin + p.samples_per_seg;
    if (j_end > p.n_samples) j_end = p.n_samples;
    uint32_t top = BIGK_EMPTY;
    auto drain = [&](int n) {
        float d[R];
        dist(sid, n, d);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t key = lane + 64 * r < n ? bigk_key(d[r]) : BIGK_EMPTY;
            const uint32_t last = (uint32_t)__shfl((int)top, 63, 64);
            if (wave_any(key < last)) top = wave_min64_of(top, bitonic64_sort(key, lane), lane);
        }
    };
    int cnt = 0;   // queued rows (the wave agrees), < 64 R between steps
    for (uint64_t j0 = j_begin + 64 * (uint64_t)wave; j0 < j_end; j0 += 256) {
        const uint64_t r = (j0 + lane) * p.step;
        bool ok = j0 + lane < j_end && r < p.N && !bit_test(p.excl, p.excl_nbits, r);
        if (ok && allow) ok = bit_test(allow, p.allow_nbits, r);
        const uint64_t m = __ballot(ok);
        if (ok) sid[cnt + mbcnt64(m)] = (uint32_t)r;
        cnt += __popcll(m);
        bigk_wave_sync();
        if (cnt < 64 * R) continue;
        drain(64 * R);
        bigk_wave_sync();
        // the rows past the batch (fewer than 64) move to the queue's head
        cnt -= 64 * R;
        const uint32_t rest = lane < cnt ? sid[64 * R + lane] : 0u;
        bigk_wave_sync();
        if (lane < cnt) sid[lane] = rest;
        bigk_wave_sync();
    }
    if (cnt) drain(cnt);
    top = bigk_merge_waves(top, wl, wave, lane);
    if (wave == 0) p.seg_keys[((uint64_t)q * p.n_seg + seg) * 64 + lane] = top;
}

}  // namespace wv
