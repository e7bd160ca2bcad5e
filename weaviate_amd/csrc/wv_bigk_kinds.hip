// wv_bigk_kinds.hip -- the large-k route's bound pass on the index kinds whose
// distance is one serial chain per row: PQ-compressed (the table sum in
// segment order) and manhattan / hamming (the fp32 chain in dimension order).
// The counterparts of wv_bigk.hip's bigk_bound_kernel, which spreads a row
// over 8 lanes for the reference's 32 FMA chains and so fits neither.
//
// Both kernels: grid (query, sample segment) x 256 threads, sample j is row
// j step with the scan's tombstone and allow-list bit tests, and the selection
// is bigk_bound_kernel's -- a wave keeps its 64 smallest orderable keys, one
// per lane, the four waves merge through LDS, bigk_tau_kernel merges the
// segments (bigk_walk, wv_bigk_dev.h).  A chain cannot be split over lanes
// without changing its bits, so a lane owns whole rows, and since idle lanes
// are then idle for a whole chain the walk queues the surviving rows in LDS
// and evaluates them a full wave at a time: under a per-query bitmap that
// keeps half the corpus -- the route's filtered searches -- no evaluation but
// a segment's last runs half empty.
//
// PQ (bigk_bound_pq_kernel).  One query per workgroup, its lookup table
// (wv_pq_lut.h: m ks floats, pq_step's values) built once in LDS where
// lut_plan lets it -- the table fits SBD_PQ_LUT_BYTES_MAX and the segment holds
// at least ks samples (WV_SBD_PQ_LUT=0|1 as for the threshold pass) -- else
// every lane calls pq_dist_row.  Either way the value is pq_dist_row's, bit
// for bit, which is what the threshold pass (wv_sbd_pq.hip) computes for the
// same row: tau and the lists agree.
//   The sampled read: whole rows per lane (pq_lut_dist's loads, up to 16 code
// bytes each).  Sampled rows lie step x stride bytes apart, so no two lanes
// share a cache line from step >= 2 at 64-byte rows whoever loads them;
// spreading a row's bytes over lanes would save load instructions but the
// sum needs the m entries in segment order in one lane, i.e. a serial chain of
// m cross-lane moves in place of m adds.  With one row per lane every table
// read of a wave is within one segment's ks entries (the addresses differ by
// the lanes' codes: random codes' bank conflicts, equal codes broadcast), as
// in the scan kernels; the tables are not interleaved by query as the fused
// scan's are, because the queue's rows differ per query under the per-query
// bitmaps this route mostly serves.
//
// Manhattan, hamming (bigk_bound_l1_kernel).  wv_l1_ids.hip's data movement
// (wv_l1_ring.h): the query in LDS, columns >= D zeroed; a batch of 64 L1I_R
// queued rows goes global -> LDS in 16-float chunks transposed through the
// wave's double-buffered ring, and lane l runs the whole chains of rows l,
// l + 64, ...: the bits of wv_l1.hip and wv_l1_ids.hip.  dpad up to
// FLAT_IDS_DPAD_MAX, as there.  LDS: queues 4 x 64 (L1I_R + 1) x 4 + query +
// rings 67,584 B at L1I_R = 2: 71 KiB at D = 128 (two workgroups a CU),
// 102 KiB at D = 8192.
//
// Built as wv_l1.hip is: no contraction, no packed fp32 forms.
#include "wv_bigk_dev.h"
#include "wv_device.h"
#include "wv_l1_dev.h"
#include "wv_l1_ring.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_pq_lut.h"
#include "wv_topk.h"

namespace wv {

// dynamic LDS: the table (none where every workgroup evaluates directly)
template <int METRIC>
__global__ __launch_bounds__(256) void bigk_bound_pq_kernel(BigkPqParams pp) {
    extern __shared__ __attribute__((aligned(16))) char bigk_smem[];
    __shared__ uint32_t sid[4][128];
    __shared__ uint32_t wl[4][64];
    float* lut = reinterpret_cast<float*>(bigk_smem);
    const BigkParams& p = pp.b;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x, seg = blockIdx.y;
    if (q >= p.nq || seg >= p.n_seg) return;
    const uint64_t j_begin = (uint64_t)seg * p.samples_per_seg;
    const uint64_t n_seg_samples = p.n_samples > j_begin ? min(p.samples_per_seg, p.n_samples - j_begin) : 0;
    const float* qrow = p.Q + (uint64_t)q * p.dpad;
    const bool use_lut = n_seg_samples >= pp.lut_min_rows;   // (the whole workgroup agrees)
    if (use_lut) pq_lut_build<METRIC>(lut, qrow, pp.pq);
    bigk_walk<1>(p, sid[wave], wl, [&](const uint32_t* rows, int n, float (&d)[1]) {
        d[0] = 0.f;
        if (lane < n)
            d[0] = use_lut ? pq_lut_dist<METRIC>(lut, pp.pq, rows[lane]) : pq_dist_row<METRIC>(qrow, pp.pq, rows[lane]);
    });
}

// dynamic LDS: queues [4][64 (L1I_R + 1)] | query [l1i_dq(D)] | rings [4][L1I_RING]
constexpr int BIGK_L1_QUEUE = 64 * (L1I_R + 1);
__host__ __device__ constexpr size_t bigk_l1_lds(int D) {
    return (size_t)4 * BIGK_L1_QUEUE * 4 + (size_t)l1i_dq(D) * 4 + (size_t)4 * L1I_RING * 4;
}

template <int METRIC>
__global__ __launch_bounds__(256) void bigk_bound_l1_kernel(BigkParams p) {
    extern __shared__ __attribute__((aligned(16))) char bigk_smem[];
    __shared__ uint32_t wl[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x, seg = blockIdx.y;
    if (q >= p.nq || seg >= p.n_seg) return;
    uint32_t* sid = reinterpret_cast<uint32_t*>(bigk_smem) + wave * BIGK_L1_QUEUE;
    float* qv = reinterpret_cast<float*>(bigk_smem + 4 * BIGK_L1_QUEUE * 4);
    const int dq = l1i_dq(p.D);
    float* xs = qv + dq + wave * L1I_RING;
    const float* qrow = p.Q + (uint64_t)q * p.dpad;
    for (int i = threadIdx.x; i < dq; i += 256) qv[i] = i < p.D ? qrow[i] : 0.f;
    __syncthreads();
    bigk_walk<L1I_R>(p, sid, wl, [&](const uint32_t* rows, int n, float (&d)[L1I_R]) {
        l1i_dists<METRIC>(p.X, p.ldx, p.D, rows, n, qv, xs, lane, d);
    });
}

}  // namespace wv

namespace {

// what both launchers ask of the sample and its segments (wv_launch_bigk_bound's tests)
bool bigk_sample_ok(const wv::BigkParams* p) {
    return p->nq > 0 && p->Q && p->excl && p->N != 0 && p->N <= 0xFFFFFFFFull && p->step >= 1 && p->n_samples >= 1 &&
           p->n_seg >= 1 && p->n_seg <= 65535 && p->samples_per_seg != 0 && p->samples_per_seg % 256 == 0 &&
           (uint64_t)p->n_seg * p->samples_per_seg >= p->n_samples && (p->n_samples - 1) * p->step < p->N &&
           p->seg_keys && p->tau;
}

}  // namespace

extern "C" {

hipError_t wv_launch_bigk_bound_pq(const wv::BigkPqParams* p, hipStream_t s) {
    if (p->b.nq == 0) return hipSuccess;
    if (!bigk_sample_ok(&p->b) || p->b.metric > WV_METRIC_COSINE || !wv::pq_ok(p->pq) ||
        p->b.dpad < p->pq.m * p->pq.ds)
        return hipErrorInvalidValue;
    wv::BigkPqParams pp = *p;
    const size_t lds = wv::lut_plan(pp.pq, pp.lut, &pp.lut_min_rows);
    const dim3 grid((unsigned)pp.b.nq, (unsigned)pp.b.n_seg);
    if (pp.b.metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::bigk_bound_pq_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, pp);
    else if (pp.b.metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::bigk_bound_pq_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, pp);
    else hipLaunchKernelGGL(wv::bigk_bound_pq_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return wv_launch_bigk_tau(&p->b, s);
}

hipError_t wv_launch_bigk_bound_l1(const wv::BigkParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (!bigk_sample_ok(p) || (p->metric != WV_METRIC_MANHATTAN && p->metric != WV_METRIC_HAMMING) || !p->X ||
        p->D < 1 || p->ldx < p->D || p->dpad < p->D || p->ldx % 4 || ((uintptr_t)p->X & 15) ||
        p->dpad > wv::FLAT_IDS_DPAD_MAX)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq, (unsigned)p->n_seg);
    const size_t lds = wv::bigk_l1_lds(p->D);
    if (p->metric == WV_METRIC_MANHATTAN)
        hipLaunchKernelGGL(wv::bigk_bound_l1_kernel<WV_METRIC_MANHATTAN>, grid, dim3(256), lds, s, *p);
    else
        hipLaunchKernelGGL(wv::bigk_bound_l1_kernel<WV_METRIC_HAMMING>, grid, dim3(256), lds, s, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return wv_launch_bigk_tau(p, s);
}

}  // extern "C"
