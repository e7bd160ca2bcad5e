// wv_bigk.hip -- exact k-NN for k past every key pass, batched: the bound pass
// and the emit of the large-k route (wv_search_bigk.hip).
//
// The route answers a chunk of queries in three stages.  The bound pass here
// gives every query a distance tau that, with overwhelming probability, at
// least k eligible rows lie within and at most a few k do (BigkParams in
// wv_params.h derives the constants).  The threshold passes of the distance
// search (wv_sbd.hip, wv_sbd_h16*.hip) then list every eligible row within
// tau and the segmented sort orders each list by (dist, id).  The emit kernel
// checks the counts: a query whose list is whole and holds k rows within tau
// has its k nearest as the list's first k entries -- the reference-order
// distances of exact_dist_rows, so the answer has the per-query route's bits
// -- and any other query is flagged for that route.
//
// Bound pass, grid (query, corpus segment) x 256 threads.  Sample j is row
// j step.  A wave takes 64 samples a step, drops the tombstoned and the
// disallowed ones with the scan's bit tests, compacts the survivors into its
// LDS slots and computes their distances 32 at a time, as sbd_scan_kernel
// does.  It keeps the 64 smallest distances it has seen as orderable u32 keys,
// one per lane, ascending: a step whose keys all lie past the list's last
// entry costs one vote; otherwise the step's keys are sorted in registers and
// merged in (wave_min64_of, wv_topk.h).  The four waves' lists merge through
// LDS at the segment's end and the segment writes its 64 keys.
// bigk_tau_kernel, one workgroup per query, merges the segments the same way
// and writes the BIGK_RANK-th smallest as tau, +inf where the sample holds
// fewer finite distances -- then every eligible row is listed.
//
// The bound pass here is the uncompressed l2 / dot / cosine one; compressed,
// manhattan and hamming indexes have theirs in wv_bigk_kinds.hip, and share
// the keys, the wave merge (wv_bigk_dev.h), bigk_tau_kernel and the emit.
#include "wv_bigk_dev.h"
#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_topk.h"

namespace wv {

template <int METRIC>
__global__ __launch_bounds__(256) void bigk_bound_kernel(BigkParams p) {
    __shared__ float qv[1024];
    __shared__ uint32_t ids[4][64];
    __shared__ float ds[4][64];
    __shared__ uint32_t wl[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x, seg = blockIdx.y;
    if (q >= p.nq || seg >= p.n_seg || p.dpad > 1024) return;
    for (int i = threadIdx.x; i < p.dpad; i += 256) qv[i] = p.Q[(uint64_t)q * p.dpad + i];
    __syncthreads();
    const uint64_t* allow = p.allow ? p.allow + (p.allow_stride ? (uint64_t)q * p.allow_stride : 0) : nullptr;
    const uint64_t j_begin = (uint64_t)seg * p.samples_per_seg;
    uint64_t j_end = j_begin + p.samples_per_seg;
    if (j_end > p.n_samples) j_end = p.n_samples;
    uint32_t top = BIGK_EMPTY;
    for (uint64_t j0 = j_begin + 64 * (uint64_t)wave; j0 < j_end; j0 += 256) {
        const uint64_t r = (j0 + lane) * p.step;
        bool ok = j0 + lane < j_end && r < p.N && !bit_test(p.excl, p.excl_nbits, r);
        if (ok && allow) ok = bit_test(allow, p.allow_nbits, r);
        const uint64_t m = __ballot(ok);
        const int n = __popcll(m);
        if (ok) ids[wave][mbcnt64(m)] = (uint32_t)r;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (n == 0) continue;
        exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, ids[wave], min(n, 32), ds[wave], lane);
        if (n > 32) exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, ids[wave] + 32, n - 32, ds[wave] + 32, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t key = lane < n ? bigk_key(ds[wave][lane]) : BIGK_EMPTY;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t last = (uint32_t)__shfl((int)top, 63, 64);
        if (wave_any(key < last)) top = wave_min64_of(top, bitonic64_sort(key, lane), lane);
    }
    top = bigk_merge_waves(top, wl, wave, lane);
    if (wave == 0) p.seg_keys[((uint64_t)q * p.n_seg + seg) * 64 + lane] = top;
}

// a query's segments -> tau: wave w merges segments w, w + 4, ...
__global__ __launch_bounds__(256) void bigk_tau_kernel(BigkParams p) {
    __shared__ uint32_t wl[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x;
    if (q >= p.nq) return;
    uint32_t top = BIGK_EMPTY;
    for (int seg = wave; seg < p.n_seg; seg += 4)
        top = wave_min64_of(top, p.seg_keys[((uint64_t)q * p.n_seg + seg) * 64 + lane], lane);
    top = bigk_merge_waves(top, wl, wave, lane);
    if (wave == 0 && lane == BIGK_RANK - 1) p.tau[q] = top >= BIGK_KEY_INF ? __builtin_inff() : bigk_unkey(top);
}

// One workgroup per query over the threshold pass's counts and sorted list.
// Answered: the list is whole (|Q| <= cap; the f16 filter's candidates fitted
// theirs) and either k rows lie within tau -- the list's first k are then the
// k nearest -- or tau is +inf and the list holds every eligible row at a
// finite distance, as the per-query route's answer does.
template <int METRIC>
__global__ __launch_bounds__(256) void bigk_emit_kernel(BigkParams p) {
    const int q = blockIdx.x;
    if (q >= p.nq) return;
    const unsigned int n_list = p.cnt[3 * q], n_within = p.cnt[3 * q + 1];
    bool ok = n_list <= (unsigned int)p.cap && (n_within >= (unsigned int)p.k || p.tau[q] == __builtin_inff());
    if (p.ccnt && p.ccnt[q] > (unsigned int)p.ccap) ok = false;
    if (!ok) {
        if (threadIdx.x == 0) p.flag[q] = 1;
        return;
    }
    const int m = (int)min(n_list, (unsigned int)p.k);
    for (int i = threadIdx.x; i < m; i += 256) {
        const unsigned long long key = p.sorted[(uint64_t)q * p.cap + i];
        float d = bigk_unkey((uint32_t)(key >> 32));
        // sbd_key folds -0 into +0; a dot product of exactly 0 is the distance
        // -0 (the sums themselves are never -0)
        if (METRIC == WV_METRIC_DOT && d == 0.f) d = -0.0f;
        p.out_ids[(uint64_t)q * p.k + i] = p.id_base + (uint32_t)key;
        p.out_d[(uint64_t)q * p.k + i] = d;
    }
    if (threadIdx.x == 0) {
        p.out_n[q] = m;
        p.flag[q] = 0;
    }
}

}  // namespace wv

extern "C" {

// the bound pass: every query's tau into p->tau
hipError_t wv_launch_bigk_bound(const wv::BigkParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (p->metric > WV_METRIC_COSINE || p->dpad > 1024 || p->N == 0 || p->N > 0xFFFFFFFFull || p->step < 1 ||
        p->n_seg < 1 || p->n_seg > 65535 || p->samples_per_seg == 0 || p->samples_per_seg % 256 ||
        (uint64_t)p->n_seg * p->samples_per_seg < p->n_samples || (p->n_samples - 1) * p->step >= p->N || !p->seg_keys ||
        !p->tau)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq, (unsigned)p->n_seg);
    if (p->metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::bigk_bound_kernel<WV_METRIC_L2>, grid, dim3(256), 0, s, *p);
    else if (p->metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::bigk_bound_kernel<WV_METRIC_DOT>, grid, dim3(256), 0, s, *p);
    else hipLaunchKernelGGL(wv::bigk_bound_kernel<WV_METRIC_COSINE>, grid, dim3(256), 0, s, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return wv_launch_bigk_tau(p, s);
}

// every query's tau from its segments' keys (any bound pass's second half)
hipError_t wv_launch_bigk_tau(const wv::BigkParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (p->n_seg < 1 || !p->seg_keys || !p->tau) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::bigk_tau_kernel, dim3((unsigned)p->nq), dim3(256), 0, s, *p);
    return hipGetLastError();
}

// (a zero distance is -0 only under the dot metrics' wrap, raw or PQ; the
// manhattan and hamming sums are never negative)
hipError_t wv_launch_bigk_emit(const wv::BigkParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (p->metric > WV_METRIC_HAMMING || p->k < 1 || p->cap < 1 || !p->sorted || !p->cnt || !p->tau || !p->flag)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq);
    if (p->metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::bigk_emit_kernel<WV_METRIC_DOT>, grid, dim3(256), 0, s, *p);
    else hipLaunchKernelGGL(wv::bigk_emit_kernel<WV_METRIC_L2>, grid, dim3(256), 0, s, *p);
    return hipGetLastError();
}

}  // extern "C"
