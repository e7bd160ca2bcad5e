// wv_pq_scan.hip -- flatSearch on a compressed index with the selection fused
// into the scan (hnsw/flat_search.go:19-74, where distBetweenNodeAndVec is the
// PQ distance, hnsw/index.go:493-511): no [nq][rows] arrays, no library sort.
//
// Grid (query groups, row slabs), 256 threads.  A workgroup serves G queries
// of the batch (4, 2 or 1) over its slab of consecutive rows -- or consecutive
// entries of a row list -- from G lookup tables interleaved by query: entry
// (segment i, centroid c, query g) at lut[(i * ks + c) * G + g], every entry
// pq_step's value.  A wave takes 64 rows a step, one row per lane: the lane
// tests the exclusion bit once, loads its row's codes once (pq_lut_sum's
// loads) and reads, per code, the G queries' entries with one LDS read of
// 4 G bytes.  Each query's distance is its m entries added in segment order
// from 0.f with __fadd_rn, then the metric's wrap: pq_dist_row's sum, bit for
// bit.  A per-query allow bit masks that query's result only.  Where no table
// fits (G = 0 in the parameters) the workgroup serves one query and every
// lane evaluates pq_dist_row.
//
// Selection is wv_fi_select.h's, once per (wave, query): 256 sorted keys in
// registers, a stage of PQ_KNN_STAGE keys in LDS that is flushed once a
// further 64-key step could overflow it.  At the end of the slab the tables
// are dead: the waves leave their sorted keys in LDS and wave g merges query
// g's four runs, then writes the output rows (one slab) or the slab's sorted
// k keys for flat_ids_merge_kernel.
#include "wv_device.h"
#include "wv_fi_select.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_pq_lut.h"
#include "wv_topk.h"

namespace wv {

// the G tables of queries q0 .. q0 + G - 1 (zeros for the slots past the
// batch: nothing of theirs is written); ends with a barrier
template <int METRIC, int G>
__device__ __forceinline__ void pq_knn_build(float* lut, const PqKnnParams& p, int q0) {
    const int n = p.pq.m * p.pq.ks;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int i = e / p.pq.ks;   // e = i * ks + c
        const float* cp = p.pq.cent + (uint64_t)e * p.pq.ds;
#pragma unroll
        for (int g = 0; g < G; ++g)
            lut[e * G + g] = q0 + g < p.nq
                                 ? pq_step<METRIC>(p.Q + (uint64_t)(q0 + g) * p.ldq + i * p.pq.ds, cp, p.pq.ds)
                                 : 0.f;
    }
    __syncthreads();
}

// pq_lut_sum for G queries at once: the row's codes loaded NW dwords at a
// time, per code one read of the G interleaved entries
template <int G, int NW, bool WIDE>
__device__ __forceinline__ void pq_knn_sum(const float* lut, const uint8_t* __restrict__ cr, int m, int ks,
                                           float (&dist)[G]) {
    constexpr int CPD = WIDE ? 2 : 4;   // codes per dword
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
            const float* e = lut + ((i0 + t) * ks + (int)c) * G;
            if constexpr (G == 4) {
                const float4 v = *reinterpret_cast<const float4*>(e);
                dist[0] = __fadd_rn(dist[0], v.x);
                dist[1] = __fadd_rn(dist[1], v.y);
                dist[2] = __fadd_rn(dist[2], v.z);
                dist[3] = __fadd_rn(dist[3], v.w);
            } else if constexpr (G == 2) {
                const float2 v = *reinterpret_cast<const float2*>(e);
                dist[0] = __fadd_rn(dist[0], v.x);
                dist[1] = __fadd_rn(dist[1], v.y);
            } else {
                dist[0] = __fadd_rn(dist[0], e[0]);
            }
        }
    }
}

// a row's G distances from the tables: the widest aligned loads its stride allows
template <int METRIC, int G>
__device__ __forceinline__ void pq_knn_dists(const float* lut, const PqParams& pq, uint32_t row, float (&dist)[G]) {
    const uint8_t* cr = pq.codes + (uint64_t)row * pq.stride;
#pragma unroll
    for (int g = 0; g < G; ++g) dist[g] = 0.f;
    if (pq.wide) {
        if (pq.stride % 16 == 0) pq_knn_sum<G, 4, true>(lut, cr, pq.m, pq.ks, dist);
        else if (pq.stride % 8 == 0) pq_knn_sum<G, 2, true>(lut, cr, pq.m, pq.ks, dist);
        else pq_knn_sum<G, 1, true>(lut, cr, pq.m, pq.ks, dist);
    } else {
        if (pq.stride % 16 == 0) pq_knn_sum<G, 4, false>(lut, cr, pq.m, pq.ks, dist);
        else if (pq.stride % 8 == 0) pq_knn_sum<G, 2, false>(lut, cr, pq.m, pq.ks, dist);
        else pq_knn_sum<G, 1, false>(lut, cr, pq.m, pq.ks, dist);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (METRIC == WV_METRIC_DOT) dist[g] = -dist[g];
        else if (METRIC == WV_METRIC_COSINE) dist[g] = __fsub_rn(1.0f, dist[g]);
    }
}

// grid (ceil(nq / G), n_slabs), 256 threads; dynamic LDS (pq_knn_lds):
// stages [4][G][PQ_KNN_STAGE] | tables [m * ks][G]; LUT false: G = 1, no table
template <int METRIC, int G, bool LUT>
__global__ __launch_bounds__(256) void pq_knn_kernel(PqKnnParams p) {
    extern __shared__ __attribute__((aligned(16))) char pqk_smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(pqk_smem);
    float* lut = reinterpret_cast<float*>(pqk_smem + 4 * G * PQ_KNN_STAGE * 8);
    const int q0 = blockIdx.x * G, slab = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t beg = (uint64_t)slab * p.slab_rows;
    const uint64_t end = p.nr - beg > p.slab_rows ? beg + p.slab_rows : p.nr;   // (beg < nr: the launcher's n_slabs)
    if (LUT) pq_knn_build<METRIC, G>(lut, p, q0);
    uint64_t* stage = keys + wave * G * PQ_KNN_STAGE;   // query g's at stage + g * PQ_KNN_STAGE

    uint64_t top[G][4], kth[G];
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = 0; j < 4; ++j) top[g][j] = FI_EMPTY;
        kth[g] = FI_EMPTY;
        cnt[g] = 0;
    }
    for (uint64_t i0 = beg + (uint64_t)FI_STEP * wave; i0 < end; i0 += 4 * FI_STEP) {
        const uint64_t i = i0 + lane;
        uint32_t row = 0;
        bool ok = false;
        if (i < end) {
            row = p.rows ? p.rows[i] : (uint32_t)i;
            ok = !bit_test(p.excl, p.excl_nbits, row);
        }
        if (__ballot(ok) == 0) continue;
        float d[G];
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = 0.f;
        if (ok) {
            if (LUT) pq_knn_dists<METRIC, G>(lut, p.pq, row, d);
            else d[0] = pq_dist_row<METRIC>(p.Q + (uint64_t)q0 * p.ldq, p.pq, row);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            // (a dead slot of the last group, a row query g's list leaves out,
            // a distance of +inf: absent)
            bool okg = ok && q0 + g < p.nq && d[g] != __builtin_inff();
            if (okg && p.allow) okg = bit_test(p.allow + (uint64_t)(q0 + g) * p.allow_stride, p.allow_nbits, row);
            const uint64_t key = okg ? fin_key(d[g], row) : FI_EMPTY;
            const bool adm = key < kth[g];
            const uint64_t am = __ballot(adm);
            if (adm) stage[g * PQ_KNN_STAGE + cnt[g] + mbcnt64(am)] = key;
            cnt[g] += __popcll(am);
            if (cnt[g] > PQ_KNN_STAGE - FI_STEP) {
                fi_wave_sync();
                fi_flush(top[g], stage + g * PQ_KNN_STAGE, cnt[g], lane);
                cnt[g] = 0;
                kth[g] = fi_kth(top[g], p.k);
                fi_wave_sync();
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (cnt[g] == 0) continue;
        fi_wave_sync();
        fi_flush(top[g], stage + g * PQ_KNN_STAGE, cnt[g], lane);
    }
    // the tables and stages are dead: every wave's sorted keys, [4][G][256]
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) keys[(wave * G + g) * 256 + 64 * j + lane] = top[g][j];
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (wave != g || q0 + g >= p.nq) continue;   // wave g merges query g (G <= 4 waves)
        for (int w = 0; w < 4; ++w) {
            if (w == wave) continue;
            uint64_t od[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) od[j] = keys[(w * G + g) * 256 + 255 - (64 * j + lane)];
            fi_merge(top[g], od, lane);
        }
        if (p.n_slabs == 1) {
            fi_write<METRIC>(p, top[g], q0 + g, lane);
        } else {
            unsigned long long* out = p.part + ((size_t)(q0 + g) * p.n_slabs + slab) * p.k;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (64 * j + lane < p.k) out[64 * j + lane] = top[g][j];
        }
    }
}

template <int METRIC>
static hipError_t pq_knn_launch(const PqKnnParams& p, size_t lds, hipStream_t s) {
    const int g = p.group ? p.group : 1;
    const dim3 grid((unsigned)((p.nq + g - 1) / g), (unsigned)p.n_slabs);
    if (p.group == 4) hipLaunchKernelGGL((pq_knn_kernel<METRIC, 4, true>), grid, dim3(256), lds, s, p);
    else if (p.group == 2) hipLaunchKernelGGL((pq_knn_kernel<METRIC, 2, true>), grid, dim3(256), lds, s, p);
    else if (p.group == 1) hipLaunchKernelGGL((pq_knn_kernel<METRIC, 1, true>), grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL((pq_knn_kernel<METRIC, 1, false>), grid, dim3(256), lds, s, p);
    return hipGetLastError();
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_pq_knn(const wv::PqKnnParams* p, hipStream_t s) {
    if (p->nq == 0 || p->nr == 0) return hipSuccess;
    if (p->metric > WV_METRIC_COSINE) return hipErrorInvalidValue;   // (no branch for it: never the cosine one)
    // the group is the one the plan gives for it, the slabs cover the rows exactly
    if (p->k < 1 || p->k > 256 || !wv::pq_ok(p->pq) || p->group != wv::pq_knn_group(p->pq, p->group) ||
        p->slab_rows == 0 || p->slab_rows % 256 || p->n_slabs < 1 || p->n_slabs > 65535 ||
        (uint64_t)p->n_slabs != (p->nr + p->slab_rows - 1) / p->slab_rows || (p->n_slabs > 1 && !p->part) ||
        (p->allow && !p->allow_stride))
        return hipErrorInvalidValue;
    const size_t lds = wv::pq_knn_lds(p->pq, p->group);
    hipError_t e;
    if (p->metric == WV_METRIC_L2) e = wv::pq_knn_launch<WV_METRIC_L2>(*p, lds, s);
    else if (p->metric == WV_METRIC_DOT) e = wv::pq_knn_launch<WV_METRIC_DOT>(*p, lds, s);
    else e = wv::pq_knn_launch<WV_METRIC_COSINE>(*p, lds, s);
    if (e != hipSuccess || p->n_slabs == 1) return e;
    // the slabs' keys merge as the list kernels' chunks do
    wv::FlatIdsParams mp{};
    mp.id_base = p->id_base;
    mp.part = p->part;
    mp.ns = p->nq;
    mp.n_chunks = p->n_slabs;
    mp.metric = p->metric;
    mp.k = p->k;
    mp.out_ids = p->out_ids;
    mp.out_d = p->out_d;
    mp.out_n = p->out_n;
    return wv_launch_flat_ids_merge(&mp, s);
}

}  // extern "C"
