// wv_sbd_pq.hip -- SearchByVectorDistance's threshold passes on a compressed
// index (the counterparts of wv_sbd.hip's sbd_scan_kernel and sbd_ids_kernel).
//
// Same outputs into the same buffers -- keys sbd_key(d, row), cnt[q][0..2] =
// |Q|, A, n -- and the same inclusion tests; the distance is the PQ distance,
// bit for bit pq_dist_row<METRIC> (wv_device.h): round 1 of an HNSW query
// comes from the HNSW kernel, which ranks by pq_dist_row, and the host merges
// the two, so one ulp apart would duplicate or drop rows.
//
// The hot path is the reference's per-query lookup table (wv_pq_lut.h: built by
// the workgroup in LDS, a row's distance its m entries added in segment order,
// one row per lane).
//
// A workgroup uses the table when it fits (SBD_PQ_LUT_BYTES_MAX) and its share
// of rows is at least ks: building costs ks * D multiply-adds, evaluating its
// rows directly costs rows * D.  Otherwise (ks 65536, many segments, a list
// chunk shorter than ks) each lane calls pq_dist_row.
#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_pq_lut.h"

namespace wv {

// one wave step's rows (ok: this lane has one, at distance d) appended to the
// query's list as sbd_scan_kernel does; returns the lanes with d <= target
__device__ __forceinline__ unsigned int sbd_pq_append(bool ok, float d, uint32_t row, float tf, double t,
                                                      unsigned int* cnt_q, unsigned long long* keys,
                                                      unsigned int seg_cap, int lane) {
    const bool in = ok && (double)d - t <= 1e-6;
    const bool below = ok && d <= tf;
    const uint64_t im = __ballot(in);
    const int ni = __popcll(im);
    if (ni) {
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(cnt_q, (unsigned int)ni);
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned int pos = base + (unsigned int)mbcnt64(im);
        if (in && pos < seg_cap) keys[pos] = sbd_key(d, row);
    }
    return (unsigned int)__popcll(__ballot(below));
}

// grid (nq, row blocks), 256 threads, dynamic LDS: the table.  Each wave takes
// 64 consecutive rows a step, one row per lane, so a wave's code loads are
// contiguous.
template <int METRIC>
__global__ __launch_bounds__(256) void sbd_pq_scan_kernel(SbdPqParams pp) {
    extern __shared__ __attribute__((aligned(16))) char sbd_pq_smem[];
    float* lut = reinterpret_cast<float*>(sbd_pq_smem);
    const SbdParams& p = pp.s;
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (q >= p.nq) return;
    const uint64_t r_begin = (uint64_t)blockIdx.y * p.rows_per_block;
    uint64_t r_end = r_begin + p.rows_per_block;
    if (r_end > p.N) r_end = p.N;
    if (r_begin >= r_end) return;
    const float* qrow = p.Q + (uint64_t)q * p.dpad;
    const bool use_lut = r_end - r_begin >= pp.lut_min_rows;   // (the whole workgroup agrees)
    if (use_lut) pq_lut_build<METRIC>(lut, qrow, pp.pq);
    const float tf = p.target[q];
    const double t = (double)tf;
    const uint64_t* allow = p.allow ? p.allow + (p.allow_stride ? (uint64_t)q * p.allow_stride : 0) : nullptr;
    unsigned long long* keys = p.keys + (uint64_t)q * p.cap;
    unsigned int n_a = 0, n_ok = 0;   // (lane 0's running counts)
    for (uint64_t r0 = r_begin + 64 * (uint64_t)wave; r0 < r_end; r0 += 256) {
        const uint64_t r = r0 + lane;
        bool ok = r < r_end && !bit_test(p.excl, p.excl_nbits, r);
        if (ok && allow) ok = bit_test(allow, p.allow_nbits, r);
        const uint64_t m = __ballot(ok);
        if (m == 0) continue;
        float d = 0.f;
        if (ok) d = use_lut ? pq_lut_dist<METRIC>(lut, pp.pq, (uint32_t)r) : pq_dist_row<METRIC>(qrow, pp.pq, (uint32_t)r);
        n_a += sbd_pq_append(ok, d, (uint32_t)r, tf, t, p.cnt + 3 * q, keys, (unsigned int)p.cap, lane);
        n_ok += (unsigned int)__popcll(m);
    }
    if (lane == 0 && n_a) atomicAdd(p.cnt + 3 * q + 1, n_a);
    if (lane == 0 && n_ok) atomicAdd(p.cnt + 3 * q + 2, n_ok);
}

// The same pass over allow lists given as ids: grid (queries of the chunk,
// chunks of a list), 256 threads, dynamic LDS: the table.  A wave walks its
// chunk 64 ids a step, one id per lane (ids past the rows and excluded rows
// dropped), and appends into the query's own segment of seg_cap keys.
template <int METRIC>
__global__ __launch_bounds__(256) void sbd_pq_ids_kernel(SbdPqIdsParams pp) {
    extern __shared__ __attribute__((aligned(16))) char sbd_pq_smem[];
    float* lut = reinterpret_cast<float*>(sbd_pq_smem);
    const SbdIdsParams& p = pp.s;
    const int qi = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (qi >= p.nq) return;
    const int q = p.q0 + qi;
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)blockIdx.y * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;
    if (beg >= end) return;
    const float* qrow = p.Q + (uint64_t)q * p.dpad;
    const bool use_lut = end - beg >= pp.lut_min_rows;   // (the whole workgroup agrees)
    if (use_lut) pq_lut_build<METRIC>(lut, qrow, pp.pq);
    const float tf = p.target[q];
    const double t = (double)tf;
    const unsigned int seg_cap = (unsigned int)p.seg_cap[qi];
    unsigned long long* keys = p.keys + p.seg_beg[qi];
    unsigned int n_a = 0, n_ok = 0;   // (lane 0's running counts)
    for (uint64_t i0 = beg + 64 * (uint64_t)wave; i0 < end; i0 += 256) {
        const uint64_t i = i0 + lane;
        uint32_t r = 0;
        bool ok = false;
        if (i < end) {
            r = p.ids[i];
            ok = r < p.n_rows && !bit_test(p.excl, p.excl_nbits, r);
        }
        const uint64_t m = __ballot(ok);
        if (m == 0) continue;
        float d = 0.f;
        if (ok) d = use_lut ? pq_lut_dist<METRIC>(lut, pp.pq, r) : pq_dist_row<METRIC>(qrow, pp.pq, r);
        n_a += sbd_pq_append(ok, d, r, tf, t, p.cnt + 3 * q, keys, seg_cap, lane);
        n_ok += (unsigned int)__popcll(m);
    }
    if (lane == 0 && n_a) atomicAdd(p.cnt + 3 * q + 1, n_a);
    if (lane == 0 && n_ok) atomicAdd(p.cnt + 3 * q + 2, n_ok);
}

}  // namespace wv

using wv::lut_plan;
using wv::pq_ok;

extern "C" {

hipError_t wv_launch_sbd_pq_scan(const wv::SbdPqParams* p, hipStream_t s) {
    if (p->s.nq == 0 || p->s.N == 0) return hipSuccess;
    if (!pq_ok(p->pq) || p->s.rows_per_block == 0 || p->s.N > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t blocks_y = (p->s.N + p->s.rows_per_block - 1) / p->s.rows_per_block;
    if (blocks_y > 65535) return hipErrorInvalidValue;
    wv::SbdPqParams pp = *p;
    const size_t lds = lut_plan(pp.pq, pp.lut, &pp.lut_min_rows);
    const dim3 grid((unsigned)pp.s.nq, (unsigned)blocks_y);
    if (pp.s.metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::sbd_pq_scan_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, pp);
    else if (pp.s.metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::sbd_pq_scan_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, pp);
    else hipLaunchKernelGGL(wv::sbd_pq_scan_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, pp);
    return hipGetLastError();
}

hipError_t wv_launch_sbd_pq_ids(const wv::SbdPqIdsParams* p, hipStream_t s) {
    if (p->s.nq == 0 || p->s.n_chunks == 0) return hipSuccess;
    if (!pq_ok(p->pq) || p->s.n_chunks < 0 || p->s.n_chunks > 65535 || p->s.chunk_len == 0 || p->s.chunk_len % 256)
        return hipErrorInvalidValue;
    wv::SbdPqIdsParams pp = *p;
    const size_t lds = lut_plan(pp.pq, pp.lut, &pp.lut_min_rows);
    const dim3 grid((unsigned)pp.s.nq, (unsigned)pp.s.n_chunks);
    if (pp.s.metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::sbd_pq_ids_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, pp);
    else if (pp.s.metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::sbd_pq_ids_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, pp);
    else hipLaunchKernelGGL(wv::sbd_pq_ids_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, pp);
    return hipGetLastError();
}

}  // extern "C"
