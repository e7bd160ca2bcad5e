// wv_pq_lut.h -- the per-query PQ lookup table shared by the kernels that walk
// rows of a compressed index one row per lane (wv_sbd_pq.hip, wv_flat_ids.hip).
//
// The reference's table (ssdhelpers/product_quantization.go:56-75): lut[i][c] =
// segment i's Step value of the query against centroid c, every entry computed
// by pq_dist_row's inner loop (pq_step), m * ks floats of LDS built by the
// workgroup.  A row's distance is then its m entries added in segment order
// from 0.f with __fadd_rn, then Wrap -- the sum pq_dist_row (wv_device.h)
// forms, bit for bit.  All lanes of a wave read the same segment's row of the
// table at once, at addresses that differ by their codes: conflicts are those
// of random codes, equal codes broadcast, and no two segments are read by one
// instruction.
#pragma once
#include "wv_device.h"
#include "wv_params.h"

namespace wv {

// one segment's Step value: the inner loop of pq_dist_row, product rounded
// before the add
template <int METRIC>
__device__ __forceinline__ float pq_step(const float* __restrict__ qs, const float* __restrict__ cp, int ds) {
    float s = 0.f;
    for (int j = 0; j < ds; ++j) {
        if (METRIC == WV_METRIC_L2) {
            const float d = __fsub_rn(qs[j], cp[j]);
            s = __fadd_rn(s, __fmul_rn(d, d));
        } else {
            s = __fadd_rn(s, __fmul_rn(qs[j], cp[j]));
        }
    }
    return s;
}

// the workgroup's table for the query row q (global memory: every thread of a
// segment reads the same ds floats); ends with a barrier
template <int METRIC>
__device__ __forceinline__ void pq_lut_build(float* lut, const float* __restrict__ q, const PqParams& pq) {
    const int n = pq.m * pq.ks;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int i = e / pq.ks;   // e = i * ks + c: centroid c of segment i starts at cent + e * ds
        lut[e] = pq_step<METRIC>(q + i * pq.ds, pq.cent + (uint64_t)e * pq.ds, pq.ds);
    }
    __syncthreads();
}

// the m table entries of one row summed in segment order; the row's codes are
// loaded NW dwords at a time (NW * 4 bytes divide the row stride)
template <int NW, bool WIDE>
__device__ __forceinline__ float pq_lut_sum(const float* lut, const uint8_t* __restrict__ cr, int m, int ks) {
    constexpr int CPD = WIDE ? 2 : 4;   // codes per dword
    float dist = 0.f;
    for (int i0 = 0; i0 < m; i0 += NW * CPD) {
        uint32_t w[NW];
        const uint8_t* src = cr + (WIDE ? 2 * i0 : i0);
        if constexpr (NW == 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(src);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if constexpr (NW == 2) {
            const uint2 v = *reinterpret_cast<const uint2*>(src);
            w[0] = v.x; w[1] = v.y;
        } else {
            w[0] = *reinterpret_cast<const uint32_t*>(src);
        }
#pragma unroll
        for (int t = 0; t < NW * CPD; ++t) {
            if (i0 + t >= m) break;   // (m need not fill the last load)
            const uint32_t c = WIDE ? (w[t >> 1] >> (16 * (t & 1))) & 0xFFFFu : (w[t >> 2] >> (8 * (t & 3))) & 0xFFu;
            dist = __fadd_rn(dist, lut[(i0 + t) * ks + (int)c]);
        }
    }
    return dist;
}

// a row's distance from the table: the widest aligned loads its stride allows
template <int METRIC>
__device__ __forceinline__ float pq_lut_dist(const float* lut, const PqParams& pq, uint32_t row) {
    const uint8_t* cr = pq.codes + (uint64_t)row * pq.stride;
    float dist;
    if (pq.wide) {
        if (pq.stride % 16 == 0) dist = pq_lut_sum<4, true>(lut, cr, pq.m, pq.ks);
        else if (pq.stride % 8 == 0) dist = pq_lut_sum<2, true>(lut, cr, pq.m, pq.ks);
        else dist = pq_lut_sum<1, true>(lut, cr, pq.m, pq.ks);
    } else {
        if (pq.stride % 16 == 0) dist = pq_lut_sum<4, false>(lut, cr, pq.m, pq.ks);
        else if (pq.stride % 8 == 0) dist = pq_lut_sum<2, false>(lut, cr, pq.m, pq.ks);
        else dist = pq_lut_sum<1, false>(lut, cr, pq.m, pq.ks);
    }
    if (METRIC == WV_METRIC_L2) return dist;
    if (METRIC == WV_METRIC_DOT) return -dist;
    return __fsub_rn(1.0f, dist);
}

// ---- host side: what the launchers of these kernels check and plan ----------

inline bool pq_ok(const wv::PqParams& pq) {
    return pq.codes && pq.cent && pq.m > 0 && pq.ks > 0 && pq.ds > 0 && pq.stride % 4 == 0 &&
           pq.stride >= (uint64_t)pq.m * (pq.wide ? 2 : 1) && (pq.wide || pq.ks <= 256) && pq.ks <= 65536;
}

// the table's LDS for a launch (0: every workgroup evaluates directly) and the
// share of rows from which a workgroup builds it
inline size_t lut_plan(const wv::PqParams& pq, int lut, uint64_t* min_rows) {
    const uint64_t bytes = (uint64_t)pq.m * (uint64_t)pq.ks * 4;
    if (lut == 0 || bytes > (uint64_t)wv::SBD_PQ_LUT_BYTES_MAX) {
        *min_rows = ~0ull;
        return 0;
    }
    *min_rows = lut > 0 ? 0 : (uint64_t)pq.ks;
    return (size_t)bytes;
}

}  // namespace wv
