// wv_l1_ring.h -- the serial manhattan / hamming chains of a wave's gathered
// rows, transposed through the wave's LDS ring (wv_l1_ids.hip's data movement,
// shared with the large-k bound pass of wv_bigk_kinds.hip).
#pragma once
#include "wv_device.h"
#include "wv_fi_select.h"
#include "wv_l1_dev.h"
#include "wv_params.h"

namespace wv {

constexpr int L1I_RING = 2 * L1_BK * L1I_LD;   // floats of a wave's ring

__host__ __device__ constexpr int l1i_dq(int D) { return (D + L1_BK - 1) / L1_BK * L1_BK; }

// acc[r] <- the chain of the wave's survivor lane + 64 r (r < L1I_R, slots < n)
// against the query in qv; xs: the wave's ring
template <int METRIC>
__device__ __forceinline__ void l1i_dists(const float* __restrict__ X, int ldx, int D, const uint32_t* sid, int n,
                                          const float* qv, float* xs, int lane, float (&acc)[L1I_R]) {
    const int nk = (D + L1_BK - 1) / L1_BK;
#pragma unroll
    for (int r = 0; r < L1I_R; ++r) acc[r] = 0.f;
    constexpr int NL = 4 * L1I_R;   // a lane's float4 loads a chunk: piece (lane & 3) of the rows 16 it + lane / 4
    const int lr = lane >> 2, k4 = (lane & 3) * 4;
    const float* row[NL];
#pragma unroll
    for (int it = 0; it < NL; ++it)
        row[it] = 16 * it + lr < n ? X + (uint64_t)sid[16 * it + lr] * (uint64_t)ldx : nullptr;
    float4 xr[NL];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int it = 0; it < NL; ++it) xr[it] = l1_load4(row[it], kc * L1_BK + k4, ldx, D);
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int it = 0; it < NL; ++it) {
            float* d = xs + (b * L1_BK + k4) * L1I_LD + 16 * it + lr;
            d[0] = xr[it].x;
            d[L1I_LD] = xr[it].y;
            d[2 * L1I_LD] = xr[it].z;
            d[3 * L1I_LD] = xr[it].w;
        }
    };
    fetch(0);
    stash(0);
    fi_wave_sync();
    for (int kc = 0; kc < nk; ++kc) {
        const int b = kc & 1;
        if (kc + 1 < nk) fetch(kc + 1);
        const float* xb = xs + b * L1_BK * L1I_LD + lane;
        const float* qk = qv + kc * L1_BK;
#pragma unroll
        for (int k = 0; k < L1_BK; ++k) {
            const float qx = qk[k];
#pragma unroll
            for (int r = 0; r < L1I_R; ++r) l1_step<METRIC>(acc[r], qx, xb[k * L1I_LD + 64 * r]);
        }
        if (kc + 1 < nk) stash(b ^ 1);
        fi_wave_sync();
    }
}

}  // namespace wv
