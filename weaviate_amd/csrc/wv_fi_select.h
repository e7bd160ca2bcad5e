// wv_fi_select.h -- the (dist, id) selection the flat kernels that walk rows
// one per lane share (wv_flat_ids.hip, wv_pq_scan.hip, wv_l1_ids.hip).  Keys are fin_key
// keys: a wave holds its 256 smallest sorted in registers (element 64 j + lane
// in register j); a new key is staged only if it is below the wave's k-th, and
// a full stage is sorted and merged in (the element-wise minimum of an
// ascending and a descending run is bitonic and holds the 256 smallest of
// both).
#pragma once
#include "wv_device.h"
#include "wv_params.h"
#include "wv_topk.h"

namespace wv {

constexpr uint64_t FI_EMPTY = ~0ull;
constexpr int FI_STAGE = 256;   // staged keys per wave
constexpr int FI_STEP = 64;     // ids per wave step

__device__ __forceinline__ void fi_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t fi_shfl(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The last phase of bitonic256_wave: a bitonic run of 256 keys, ascending after.
__device__ __forceinline__ void bitonic_merge256_wave(uint64_t (&kk)[4], int lane) {
    auto cas = [&](auto jc, auto pc) {   // (literal register indices, as in bitonic256_wave)
        constexpr int j = decltype(jc)::value, pj = decltype(pc)::value;
        const bool sw = kk[pj] < kk[j];
        const uint64_t t = kk[j];
        kk[j] = sw ? kk[pj] : kk[j];
        kk[pj] = sw ? t : kk[pj];
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    cas(I0{}, I2{}); cas(I1{}, I3{});
    cas(I0{}, I1{}); cas(I2{}, I3{});
#pragma unroll
    for (int jj = 32; jj > 0; jj >>= 1) {
        const bool lower = (lane & jj) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t plo = (uint32_t)__shfl_xor((int)(uint32_t)kk[j], jj, 64);
            const uint32_t phi = (uint32_t)__shfl_xor((int)(uint32_t)(kk[j] >> 32), jj, 64);
            const uint64_t pk = ((uint64_t)phi << 32) | plo;
            // the lower lane keeps the min
            const uint64_t a = lower ? pk : kk[j], b = lower ? kk[j] : pk;
            kk[j] = a < b ? pk : kk[j];
        }
    }
}

// top (ascending) <- the 256 smallest of top and desc (descending)
__device__ __forceinline__ void fi_merge(uint64_t (&top)[4], const uint64_t (&desc)[4], int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) top[j] = desc[j] < top[j] ? desc[j] : top[j];
    bitonic_merge256_wave(top, lane);
}

// the wave's cnt staged keys into top
__device__ __forceinline__ void fi_flush(uint64_t (&top)[4], const uint64_t* stage, int cnt, int lane) {
    uint64_t st[4];
    // sorted ascending as complements = descending as keys (an empty slot's complement is 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = 64 * j + lane < cnt ? ~stage[64 * j + lane] : 0ull;
    bitonic256_wave(st, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = ~st[j];
    fi_merge(top, st, lane);
}

// element k - 1 of top, in every lane
__device__ __forceinline__ uint64_t fi_kth(const uint64_t (&top)[4], int k) {
    const int j = (k - 1) >> 6;
    const uint64_t v = j == 0 ? top[0] : j == 1 ? top[1] : j == 2 ? top[2] : top[3];
    return fi_shfl(v, (k - 1) & 63);
}

// (P: FlatIdsParams or FlatIdsPqParams -- the same output fields)
template <int METRIC, class P>
__device__ __forceinline__ void fi_write(const P& p, const uint64_t (&top)[4], int q, int lane) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 64 * j + lane;
        const bool has = i < p.k && top[j] != FI_EMPTY;
        if (has) {
            float d;
            uint32_t id;
            fin_unkey(top[j], d, id);
            // fin_key folds -0 into +0; a dot product of exactly 0 is the
            // distance -0 (the sums themselves are never -0)
            if (METRIC == WV_METRIC_DOT && d == 0.f) d = -0.0f;
            p.out_ids[(size_t)q * p.k + i] = p.id_base + id;
            p.out_d[(size_t)q * p.k + i] = d;
        }
        n += __popcll(__ballot(has));
    }
    if (lane == 0) p.out_n[q] = n;
}

// The end of a workgroup's walk: each wave's last staged keys flushed, the
// waves merged through their stages, and wave 0 writes the query's output rows
// (one chunk) or the chunk's sorted keys for flat_ids_merge_kernel.
template <int METRIC, class P>
__device__ __forceinline__ void fi_finish(const P& p, uint64_t (&top)[4], uint64_t* stage_all, uint64_t* stage, int cnt,
                                          int s, int chunk, int q, int lane, int wave) {
    if (cnt) fi_flush(top, stage, cnt, lane);
    fi_wave_sync();
    // the waves of the workgroup: each leaves its sorted keys in its stage
#pragma unroll
    for (int j = 0; j < 4; ++j) stage[64 * j + lane] = top[j];
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) {
        uint64_t od[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) od[j] = stage_all[w * FI_STAGE + 255 - (64 * j + lane)];
        fi_merge(top, od, lane);
    }
    if (p.n_chunks == 1) {
        fi_write<METRIC>(p, top, q, lane);
    } else {
        unsigned long long* out = p.part + ((size_t)s * p.n_chunks + chunk) * p.k;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (64 * j + lane < p.k) out[64 * j + lane] = top[j];
    }
}
}  // namespace wv
