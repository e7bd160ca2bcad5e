// wv_l1_dev.h -- what the manhattan / hamming kernels share (wv_l1.hip,
// wv_l1_ids.hip): one step of a pair's serial fp32 chain and the row loads.
#pragma once
#include "wv_device.h"

namespace wv {

template <int METRIC>
__device__ __forceinline__ void l1_step(float& acc, float q, float x) {
    if (METRIC == WV_METRIC_MANHATTAN) acc += fabsf(q - x);
    else acc += q != x ? 1.f : 0.f;
}

// float4 at column kk of a row of ld floats (null row: zeros), columns >= D zeroed
__device__ __forceinline__ float4 l1_load4(const float* __restrict__ row, int kk, int ld, int D) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row && kk < ld) v = *reinterpret_cast<const float4*>(row + kk);
    if (kk + 0 >= D) v.x = 0.f;
    if (kk + 1 >= D) v.y = 0.f;
    if (kk + 2 >= D) v.z = 0.f;
    if (kk + 3 >= D) v.w = 0.f;
    return v;
}

}  // namespace wv
