// wv_sbd.hip -- SearchByVectorDistance on the device, batched
// (adapters/repos/db/vector/hnsw/search.go:90-158 with searchByDistParams,
// :552-619).
//
// The reference deepens: SearchByVector(limit 100), then 1100, 11100, ...,
// each round appending the entries [offset, total) that are within the target
// distance (or InDelta 1e-6 of it) and continuing while the round's last entry
// is <= target.  Every round past the first asks a limit whose ef exceeds the
// beam (1100 > HNSW_EF_MAX): on the GPU those rounds are exact, and an exact
// search's ranks [offset, total) are the ranks of the sorted set of rows within
// the target.  So one threshold pass answers every round past the first at
// once: per query, the allowed rows with d - target <= 1e-6 (float64, as
// floatcomp.InDelta) are appended to a per-query list with their sort keys,
// counted (|Q|, and A = those with d <= target), and the rows the search
// could return are counted too (n); a segmented sort orders the lists by
// (d, id).  The host then applies the rounds' arithmetic to |Q|, A and n.
// Distances are the reference-order exact ones (exact_dist_rows, bit-identical
// to the asm distancer).
//
// Two threshold passes: sbd_scan_kernel tests every row of the corpus against
// a bitmap (or no filter); sbd_ids_kernel walks per-query allow lists given as
// ids and reads only the listed rows, each query appending into a segment of
// its own length.
#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"

#include <hipcub/hipcub.hpp>

namespace wv {

// SbdParams: wv_params.h; sbd_key: wv_device.h

// grid (nq, row blocks), 256 threads: each wave takes 64 candidate rows a
// step, keeps the allowed ones, computes their distances 32 at a time and
// appends the ones within the target
template <int METRIC>
__global__ __launch_bounds__(256) void sbd_scan_kernel(SbdParams p) {
    __shared__ float qv[1024];
    __shared__ uint32_t ids[4][64];
    __shared__ float ds[4][64];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (q >= p.nq || p.dpad > 1024) return;
    for (int i = threadIdx.x; i < p.dpad; i += 256) qv[i] = p.Q[(uint64_t)q * p.dpad + i];
    __syncthreads();
    const double t = (double)p.target[q];
    const uint64_t* allow = p.allow ? p.allow + (p.allow_stride ? (uint64_t)q * p.allow_stride : 0) : nullptr;
    const uint64_t r_begin = (uint64_t)blockIdx.y * p.rows_per_block;
    uint64_t r_end = r_begin + p.rows_per_block;
    if (r_end > p.N) r_end = p.N;
    unsigned int n_a = 0, n_ok = 0;   // (lane 0's running counts)
    for (uint64_t r0 = r_begin + 64 * (uint64_t)wave; r0 < r_end; r0 += 256) {
        const uint64_t r = r0 + lane;
        bool ok = r < r_end && !bit_test(p.excl, p.excl_nbits, r);
        if (ok && allow) ok = bit_test(allow, p.allow_nbits, r);
        const uint64_t m = __ballot(ok);
        const int n = __popcll(m);
        if (ok) ids[wave][mbcnt64(m)] = (uint32_t)r;
        __builtin_amdgcn_wave_barrier();
        if (n == 0) continue;
        exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, ids[wave], n, ds[wave], lane);
        if (n > 32) exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, ids[wave] + 32, n - 32, ds[wave] + 32, lane);
        __builtin_amdgcn_wave_barrier();
        const float d = lane < n ? ds[wave][lane] : 0.f;
        const uint32_t id = lane < n ? ids[wave][lane] : 0u;
        const bool in = lane < n && (double)d - t <= 1e-6;
        const bool below = lane < n && d <= p.target[q];
        const uint64_t im = __ballot(in);
        const int ni = __popcll(im);
        unsigned int base = 0;
        if (ni) {
            if (lane == 0) base = atomicAdd(p.cnt + 3 * q, (unsigned int)ni);
            base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
            const unsigned int pos = base + (unsigned int)mbcnt64(im);
            if (in && pos < (unsigned int)p.cap) p.keys[(uint64_t)q * p.cap + pos] = sbd_key(d, id);
        }
        n_a += (unsigned int)__popcll(__ballot(below));
        n_ok += (unsigned int)n;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0 && n_a) atomicAdd(p.cnt + 3 * q + 1, n_a);
    if (lane == 0 && n_ok) atomicAdd(p.cnt + 3 * q + 2, n_ok);
}

// segment bounds of the sort: [q cap, q cap + min(|Q|, cap))
__global__ void sbd_offsets_kernel(const unsigned int* cnt, int nq, int cap, int* beg, int* end) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    beg[q] = q * cap;
    end[q] = q * cap + (int)min(cnt[3 * q], (unsigned int)cap);
}

// The same pass over allow lists given as ids: grid (queries of the chunk,
// chunks of a list), 256 threads; dynamic LDS: ids | dists | query.  A wave
// walks its chunk 64 ids a step as flat_ids_kernel does (ids past the rows and
// excluded rows dropped, survivors compacted into its LDS slots) and appends
// as sbd_scan_kernel does, into the query's own segment of seg_cap keys.
template <int METRIC>
__global__ __launch_bounds__(256) void sbd_ids_kernel(SbdIdsParams p) {
    extern __shared__ __attribute__((aligned(16))) char sbd_smem[];
    uint32_t* sid = reinterpret_cast<uint32_t*>(sbd_smem);        // [4][64]
    float* sds = reinterpret_cast<float*>(sbd_smem + 4 * 64 * 4); // [4][64]
    float* qv = reinterpret_cast<float*>(sbd_smem + 8 * 64 * 4);  // [dpad]
    const int qi = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (qi >= p.nq) return;
    const int q = p.q0 + qi;
    for (int i = threadIdx.x; i < p.dpad; i += 256) qv[i] = p.Q[(uint64_t)q * p.dpad + i];
    __syncthreads();
    sid += 64 * wave;
    sds += 64 * wave;
    const float tf = p.target[q];
    const double t = (double)tf;
    const unsigned int seg_cap = (unsigned int)p.seg_cap[qi];
    unsigned long long* keys = p.keys + p.seg_beg[qi];
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)blockIdx.y * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;
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
        const int n = __popcll(m);
        if (ok) sid[mbcnt64(m)] = r;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (n == 0) continue;
        exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, sid, min(n, 32), sds, lane);
        if (n > 32) exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, sid + 32, n - 32, sds + 32, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const float d = lane < n ? sds[lane] : 0.f;
        const uint32_t id = lane < n ? sid[lane] : 0u;
        const bool in = lane < n && (double)d - t <= 1e-6;
        const bool below = lane < n && d <= tf;
        const uint64_t im = __ballot(in);
        const int ni = __popcll(im);
        unsigned int base = 0;
        if (ni) {
            if (lane == 0) base = atomicAdd(p.cnt + 3 * q, (unsigned int)ni);
            base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
            const unsigned int pos = base + (unsigned int)mbcnt64(im);
            if (in && pos < seg_cap) keys[pos] = sbd_key(d, id);
        }
        n_a += (unsigned int)__popcll(__ballot(below));
        n_ok += (unsigned int)n;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0 && n_a) atomicAdd(p.cnt + 3 * q + 1, n_a);
    if (lane == 0 && n_ok) atomicAdd(p.cnt + 3 * q + 2, n_ok);
}

// segment ends of the list route's sort: seg_beg[i] + min(|Q|, seg_cap[i])
__global__ void sbd_ids_ends_kernel(const unsigned int* cnt, int q0, int nq, const int* seg_beg, const int* seg_cap,
                                    int* end) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    end[i] = seg_beg[i] + (int)min(cnt[3 * (q0 + i)], (unsigned int)seg_cap[i]);
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_sbd_ids(const wv::SbdIdsParams* p, hipStream_t s) {
    if (p->nq == 0 || p->n_chunks == 0) return hipSuccess;
    if (p->dpad > wv::FLAT_IDS_DPAD_MAX || p->n_chunks < 0 || p->n_chunks > 65535 || p->chunk_len == 0 ||
        p->chunk_len % 256)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq, (unsigned)p->n_chunks);
    const size_t lds = 8 * 64 * 4 + (size_t)p->dpad * 4;
    if (p->metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::sbd_ids_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, *p);
    else if (p->metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::sbd_ids_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, *p);
    else hipLaunchKernelGGL(wv::sbd_ids_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, *p);
    return hipGetLastError();
}

// sort the nq segments of the list route by (d, id): keys -> tmp (n_keys each,
// the sum of the segments); ends: [nq] scratch for the segment ends
hipError_t wv_sbd_ids_sort(unsigned long long* keys, unsigned long long* tmp, int n_keys, const unsigned int* cnt,
                           int q0, int nq, const int* seg_beg, const int* seg_cap, int* ends, void** scratch,
                           size_t* scratch_cap, hipStream_t s) {
    if (nq == 0 || n_keys == 0) return hipSuccess;
    hipLaunchKernelGGL(wv::sbd_ids_ends_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, cnt, q0, nq, seg_beg, seg_cap,
                       ends);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t need = 0;
    e = hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, need, keys, tmp, n_keys, nq, seg_beg, (const int*)ends, 0, 64, s);
    if (e != hipSuccess) return e;
    if (need > *scratch_cap) {
        if (*scratch) (void)hipFree(*scratch);
        *scratch = nullptr;
        *scratch_cap = 0;
        e = hipMalloc(scratch, need);
        if (e != hipSuccess) return e;
        *scratch_cap = need;
    }
    return hipcub::DeviceSegmentedRadixSort::SortKeys(*scratch, need, keys, tmp, n_keys, nq, seg_beg, (const int*)ends, 0, 64, s);
}

hipError_t wv_launch_sbd_scan(const wv::SbdParams* p, hipStream_t s) {
    if (p->nq == 0 || p->N == 0) return hipSuccess;
    if (p->dpad > 1024) return hipErrorInvalidValue;
    const uint64_t blocks_y = (p->N + p->rows_per_block - 1) / p->rows_per_block;
    if (blocks_y > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq, (unsigned)blocks_y);
    if (p->metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::sbd_scan_kernel<WV_METRIC_L2>, grid, dim3(256), 0, s, *p);
    else if (p->metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::sbd_scan_kernel<WV_METRIC_DOT>, grid, dim3(256), 0, s, *p);
    else hipLaunchKernelGGL(wv::sbd_scan_kernel<WV_METRIC_COSINE>, grid, dim3(256), 0, s, *p);
    return hipGetLastError();
}

// sort every query's list by (d, id): keys in place via tmp (same size)
hipError_t wv_sbd_sort(unsigned long long* keys, unsigned long long* tmp, const unsigned int* cnt, int nq, int cap,
                       int* offsets, void** scratch, size_t* scratch_cap, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(wv::sbd_offsets_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, cnt, nq, cap, offsets,
                       offsets + nq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t need = 0;
    e = hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, need, keys, tmp, nq * cap, nq, offsets, offsets + nq, 0,
                                                   64, s);
    if (e != hipSuccess) return e;
    if (need > *scratch_cap) {
        if (*scratch) (void)hipFree(*scratch);
        *scratch = nullptr;
        *scratch_cap = 0;
        e = hipMalloc(scratch, need);
        if (e != hipSuccess) return e;
        *scratch_cap = need;
    }
    return hipcub::DeviceSegmentedRadixSort::SortKeys(*scratch, need, keys, tmp, nq * cap, nq, offsets, offsets + nq,
                                                      0, 64, s);
}

}  // extern "C"
