// wv_search.hip -- the device pipelines behind every search of the C ABI, and
// its batch entry points (wv_search_batch, _ids, _device, wv_search_by_vector).
// search_core dispatches SearchByVector the way the reference does
// (search.go:64-79) and runs the pipelines of wv_bf.hip / wv_h16.hip /
// wv_pq.hip / wv_hnsw.hip.  No CPU search code: every distance and every
// selection happens on the GPU.
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <cstring>
#include <thread>

#include "wv_index.h"
#include "wv_launch.h"

using namespace wv_host;

namespace {

__global__ void gather_rows_kernel(const float* src, int ld_src, const int32_t* idx, int n, int D, float* dst,
                                   int ld_dst) {
    const int r = blockIdx.x;
    if (r >= n) return;
    const float* s = src + (size_t)idx[r] * ld_src;
    float* d = dst + (size_t)r * ld_dst;
    for (int i = threadIdx.x; i < ld_dst; i += blockDim.x) d[i] = i < D ? s[i] : 0.f;
}

__global__ void gather_words_kernel(const uint64_t* src, uint64_t stride, const int32_t* idx, int n, uint64_t* dst) {
    const int r = blockIdx.x;
    if (r >= n) return;
    for (uint64_t i = threadIdx.x; i < stride; i += blockDim.x) dst[r * stride + i] = src[(uint64_t)idx[r] * stride + i];
}

__global__ void scatter_results_kernel(const uint64_t* ids, const float* ds, const int32_t* ns, const int32_t* idx,
                                       int n, int k, uint64_t* out_ids, float* out_d, int32_t* out_n) {
    const int r = blockIdx.x;
    if (r >= n) return;
    const int q = idx[r];
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        out_ids[(size_t)q * k + i] = ids[(size_t)r * k + i];
        out_d[(size_t)q * k + i] = ds[(size_t)r * k + i];
    }
    if (threadIdx.x == 0) out_n[q] = ns[r];
}

__global__ void copy_topk_kernel(const float* sd, const uint32_t* si, uint64_t n_eligible_cap, int k, uint64_t id_base,
                                 uint64_t* out_ids, float* out_d, int32_t* out_n) {
    // first k of a sorted (dist, id) array; +inf marks ineligible rows
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        if ((uint64_t)i < n_eligible_cap && sd[i] != __builtin_inff()) {
            out_ids[i] = id_base + si[i];
            out_d[i] = sd[i];
            atomicAdd(&cnt, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *out_n = cnt;
}

// queries whose search reported an overflow (status != 0) into *acc
__global__ void count_nonzero_kernel(const int32_t* st, int n, unsigned long long* acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool nz = i < n && st[i] != 0;
    const unsigned long long c = __popcll(__ballot(nz));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(acc, c);
}

__global__ void popcount_rows_kernel(const uint64_t* bits, uint64_t words, uint64_t stride, int nrows,
                                     unsigned long long* out) {
    const int r = blockIdx.x;
    if (r >= nrows) return;
    unsigned long long c = 0;
    for (uint64_t i = threadIdx.x; i < words; i += blockDim.x) c += __popcll(bits[r * stride + i]);
    atomicAdd(&out[r], c);
}

// Exact scan + stable radix sort, one query at a time (large k and certificate
// fallbacks).  q: device query (normalized if cosine).
int exact_full(wv_index* ix, const float* d_q, int k, const uint64_t* d_allow, uint64_t allow_nbits,
               uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s) {
    const uint64_t N = ix->n_rows;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t), s));
        return WV_OK;
    }
    HIP_TRY(ix->scan_d.ensure(N * 4));
    HIP_TRY(ix->scan_i.ensure(N * 4));
    HIP_TRY(ix->sort_d.ensure(N * 4));
    HIP_TRY(ix->sort_i.ensure(N * 4));
    wv::ScanParams sp{};
    sp.X = ix->vecs.as<float>();
    sp.q = d_q;
    sp.tomb = ix->excl.as<uint64_t>();
    sp.tomb_nbits = ix->capacity;
    sp.allow = d_allow;
    sp.allow_nbits = allow_nbits;
    sp.N = N;
    sp.D = ix->dim;
    sp.ldx = ix->ldx;
    sp.metric = ix->metric;
    sp.dist = ix->scan_d.as<float>();
    sp.ids = ix->scan_i.as<uint32_t>();
    HIP_TRY(wv_launch_exact_scan(&sp, s));
    size_t tmp = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, ix->scan_d.as<float>(), ix->sort_d.as<float>(),
                                               ix->scan_i.as<uint32_t>(), ix->sort_i.as<uint32_t>(), (int)N, 0, 32,
                                               s));
    HIP_TRY(ix->sort_tmp.ensure(tmp));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ix->sort_tmp.p, tmp, ix->scan_d.as<float>(), ix->sort_d.as<float>(),
                                               ix->scan_i.as<uint32_t>(), ix->sort_i.as<uint32_t>(), (int)N, 0, 32,
                                               s));
    hipLaunchKernelGGL(copy_topk_kernel, dim3(1), dim3(256), 0, s, ix->sort_d.as<float>(), ix->sort_i.as<uint32_t>(),
                       N, k, ix->cfg.id_base, d_out_ids, d_out_d, d_out_n);
    HIP_TRY(hipGetLastError());
    return WV_OK;
}

__global__ void allowed_count_kernel(const uint64_t* allow, uint64_t allow_words, const uint64_t* excl, uint64_t N,
                                     uint32_t* cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t words = (N + 63) / 64;
    if (w >= words) return;
    uint64_t b = w < allow_words ? allow[w] & ~excl[w] : 0ull;
    if (w == words - 1 && (N & 63)) b &= (1ull << (N & 63)) - 1;
    cnt[w] = (uint32_t)__popcll(b);
}

__global__ void allowed_scatter_kernel(const uint64_t* allow, uint64_t allow_words, const uint64_t* excl, uint64_t N,
                                       const uint32_t* off, uint32_t* rowidx) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t words = (N + 63) / 64;
    if (w >= words) return;
    uint64_t b = w < allow_words ? allow[w] & ~excl[w] : 0ull;
    if (w == words - 1 && (N & 63)) b &= (1ull << (N & 63)) - 1;
    uint32_t o = off[w];
    while (b) {
        rowidx[o++] = (uint32_t)(w * 64 + __builtin_ctzll(b));
        b &= b - 1;
    }
}

__global__ void pad_rowidx_kernel(uint32_t* rowidx, uint64_t from, uint64_t to, const uint32_t* n_dev) {
    if (n_dev) {   // (the device's count: pad it to a whole tile)
        from = *n_dev;
        to = (from + wv::HW_BN - 1) / wv::HW_BN * wv::HW_BN;
    }
    const uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) rowidx[i] = 0;   // padded tile rows read row 0 and are masked by the row count
}

// Ascending list of the rows a shared allow list keeps (allowed, not excluded,
// < N) into ix->rowidx, padded to whole tiles; *n_ok = its length.
// The f16 pass runs over a shared allow list's gathered rows when gathering
// costs less than masking the rest of the corpus: a gathered row moves ~6 D
// bytes once, a masked row costs the pass ~nq x D of MFMA work (measured at
// 10M x 768: 0.9 ns per gathered row, 1.6 ns per scanned row per 1000
// queries) and at least one read of its 2 D-byte image, so compacting pays
// below n_ok / N = max(1/3, nq / (nq + 560)) -- 64 % at configs[3]'s 1000
// queries (round 4's fixed rule, 50 %, left the 50 % leg a coin flip).
static bool worth_compacting(uint64_t n_ok, uint64_t N, int nq) {
    const double f = std::max(1.0 / 3.0, (double)nq / ((double)nq + 560.0));
    return (double)n_ok < (double)N * f;
}

// The prefix both compactions share: the allowed rows counted per 64-row word
// into ix->ac_cnt and their exclusive scan into ix->ac_off, whose entry
// `words` = (N + 63) / 64 is then the list's length (on the device).
static int count_allowed(wv_index* ix, const uint64_t* d_allow, uint64_t allow_words, uint64_t N, hipStream_t s) {
    const uint64_t words = (N + 63) / 64;
    HIP_TRY(ix->ac_cnt.ensure((words + 1) * 4));
    HIP_TRY(ix->ac_off.ensure((words + 1) * 4));
    hipLaunchKernelGGL(allowed_count_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_allow,
                       allow_words, ix->excl.as<uint64_t>(), N, ix->ac_cnt.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(ix->ac_cnt.as<uint32_t>() + words, 0, 4, s));
    size_t tmp = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, ix->ac_cnt.as<uint32_t>(), ix->ac_off.as<uint32_t>(),
                                             (int)(words + 1), s));
    HIP_TRY(ix->sort_tmp.ensure(tmp));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(ix->sort_tmp.p, tmp, ix->ac_cnt.as<uint32_t>(), ix->ac_off.as<uint32_t>(),
                                             (int)(words + 1), s));
    return WV_OK;
}

int compact_allowed(wv_index* ix, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N, uint64_t* n_ok,
                    hipStream_t s, bool always = false, int nq = 1) {
    const uint64_t words = (N + 63) / 64;
    const uint64_t allow_words = (allow_nbits + 63) / 64;
    const unsigned blocks = (unsigned)((words + 255) / 256);
    if (int rc = count_allowed(ix, d_allow, allow_words, N, s)) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, ix->ac_off.as<uint32_t>() + words, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_ok = total;
    // (the row list also serves the fp32 pass, which compacts below 1/2)
    if (total == 0 || (!worth_compacting(total, N, nq) && 2 * (uint64_t)total >= N && !always)) return WV_OK;
    // (whole 256-row tiles: the wide-D pass reads the list per tile)
    const uint64_t padded = (total + wv::HW_BN - 1) / wv::HW_BN * wv::HW_BN;
    HIP_TRY(ix->rowidx.ensure(padded * 4));
    hipLaunchKernelGGL(allowed_scatter_kernel, dim3(blocks), dim3(256), 0, s, d_allow, allow_words,
                       ix->excl.as<uint64_t>(), N, ix->ac_off.as<uint32_t>(), ix->rowidx.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (padded > total)
        hipLaunchKernelGGL(pad_rowidx_kernel, dim3(1), dim3(256), 0, s, ix->rowidx.as<uint32_t>(), (uint64_t)total,
                           padded, nullptr);
    HIP_TRY(hipGetLastError());
    return WV_OK;
}

// The same list without reading its length back: ix->rowidx holds it, padded
// to whole tiles, and *n_dev (device memory) its length, which the compacted
// f16 wide-D pass reads itself (H16Params.n_dev) -- no host round trip
// between the allow list and the scan.
int compact_allowed_dev(wv_index* ix, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N, const uint32_t** n_dev,
                        hipStream_t s) {
    const uint64_t words = (N + 63) / 64;
    const uint64_t allow_words = (allow_nbits + 63) / 64;
    const unsigned blocks = (unsigned)((words + 255) / 256);
    if (int rc = count_allowed(ix, d_allow, allow_words, N, s)) return rc;
    const uint64_t padded = (N + wv::HW_BN - 1) / wv::HW_BN * wv::HW_BN;
    HIP_TRY(ix->rowidx.ensure(padded * 4));
    hipLaunchKernelGGL(allowed_scatter_kernel, dim3(blocks), dim3(256), 0, s, d_allow, allow_words,
                       ix->excl.as<uint64_t>(), N, ix->ac_off.as<uint32_t>(), ix->rowidx.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    *n_dev = ix->ac_off.as<uint32_t>() + words;
    hipLaunchKernelGGL(pad_rowidx_kernel, dim3(1), dim3(256), 0, s, ix->rowidx.as<uint32_t>(), 0ull, 0ull, *n_dev);
    HIP_TRY(hipGetLastError());
    return WV_OK;
}

__global__ void iota_stride_kernel(int32_t* off, int n, int64_t stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) off[i] = (int32_t)(i * stride);
}

// flatSearch over PQ codes: the rows a shared allow list (or the delta mask)
// keeps are compacted, every (query, row) distance is computed from the codes
// and a stable segmented radix sort orders each query's row list by
// (dist, id); queries go in chunks of at most 2^26 (query, row) pairs.
int run_pq_flat(wv_index* ix, const float* d_q, int nq, int k, const uint64_t* d_allow, uint64_t allow_nbits,
                uint64_t allow_stride, uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s,
                const uint64_t* d_rowmask, uint64_t rowmask_nbits) {
    const uint64_t N = ix->n_rows;
    if (N == 0 || nq == 0) {
        if (nq) HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t) * nq, s));
        return WV_OK;
    }
    const uint64_t* cmask = d_allow && !allow_stride ? d_allow : d_rowmask;
    const uint64_t cbits = d_allow && !allow_stride ? allow_nbits : rowmask_nbits;
    uint64_t nr = N;
    const uint32_t* rows = nullptr;
    if (cmask) {
        int rc = compact_allowed(ix, cmask, cbits, N, &nr, s, true);
        if (rc) return rc;
        if (nr == 0) {
            HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t) * nq, s));
            return WV_OK;
        }
        rows = ix->rowidx.as<uint32_t>();
    }
    const uint64_t cap = 1ull << 26;
    const int qc = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)nq, cap / nr));
    const uint64_t items = (uint64_t)qc * nr;
    if (items > (uint64_t)INT32_MAX) return fail(WV_EINVAL, "flat PQ search: too many rows per query");
    HIP_TRY(ix->pk_key.ensure(items * 4));
    HIP_TRY(ix->pk_dist.ensure(items * 4));
    HIP_TRY(ix->pk_val.ensure(items * 4));
    HIP_TRY(ix->pk_skey.ensure(items * 4));
    HIP_TRY(ix->pk_sval.ensure(items * 4));
    HIP_TRY(ix->pk_off.ensure(((size_t)qc + 1) * 4));
    wv::PqScanParams sp{};
    sp.pq = pq_params(ix);
    sp.Q = d_q;
    sp.rows = rows;
    sp.excl = ix->excl.as<uint64_t>();
    sp.excl_nbits = ix->capacity;
    sp.allow = allow_stride ? d_allow : nullptr;   // a shared list is compacted already
    sp.allow_nbits = allow_nbits;
    sp.allow_stride = allow_stride;
    sp.nr = nr;
    sp.ldq = ix->dpad;
    sp.metric = ix->metric;
    sp.key = ix->pk_key.as<float>();
    sp.dist = ix->pk_dist.as<float>();
    sp.val = ix->pk_val.as<uint32_t>();
    for (int q0 = 0; q0 < nq; q0 += qc) {
        const int nqc = std::min(qc, nq - q0);
        sp.q0 = q0;
        sp.nqc = nqc;
        HIP_TRY(wv_launch_pq_scan(&sp, s));
        hipLaunchKernelGGL(iota_stride_kernel, dim3((nqc + 256) / 256), dim3(256), 0, s, ix->pk_off.as<int32_t>(), nqc,
                           (int64_t)nr);
        HIP_TRY(hipGetLastError());
        const int n_items = (int)((uint64_t)nqc * nr);
        size_t tmp = 0;
        HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(
            nullptr, tmp, ix->pk_key.as<float>(), ix->pk_skey.as<float>(), ix->pk_val.as<uint32_t>(),
            ix->pk_sval.as<uint32_t>(), n_items, nqc, ix->pk_off.as<int32_t>(), ix->pk_off.as<int32_t>() + 1, 0, 32, s));
        HIP_TRY(ix->sort_tmp.ensure(tmp));
        HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(
            ix->sort_tmp.p, tmp, ix->pk_key.as<float>(), ix->pk_skey.as<float>(), ix->pk_val.as<uint32_t>(),
            ix->pk_sval.as<uint32_t>(), n_items, nqc, ix->pk_off.as<int32_t>(), ix->pk_off.as<int32_t>() + 1, 0, 32, s));
        HIP_TRY(wv_launch_pq_topk(ix->pk_skey.as<float>(), ix->pk_sval.as<uint32_t>(), ix->pk_dist.as<float>(), rows,
                                  nr, q0, nqc, k, ix->cfg.id_base, d_out_ids, d_out_d, d_out_n, s));
    }
    return WV_OK;
}

// Block order of an f16 pass: the blocks sorted by the corpus offset of their
// first tile, read by the kernels at their XCD-contiguous position (locality
// bit 1), so that each XCD runs the blocks of every query block over the same
// part of the corpus at the same time -- a tile then comes into that XCD's L2
// once per pass instead of once per query block.  nullptr: the identity
// (a single query block).
// rotated: the tiles of query block qb are rotated by qb ntiles mod U (the
// D <= 128 pass's locality bit 2), so a block's first tile is (slot U) mod ntiles.
int block_order(wv_index* ix, uint64_t nqb, const wv::BfSchedule& sch, hipStream_t s, const int** out,
                bool rotated = false) {
    *out = nullptr;
    if (nqb < 2 || sch.n_blocks < 16) return WV_OK;
    const uint64_t key[4] = {nqb, sch.ntiles, sch.units_per_block, rotated ? 1u : 0u};
    if (!std::equal(key, key + 4, ix->blk_key)) {
        const int nb = sch.n_blocks;
        const uint64_t U = sch.units_per_block, nt = sch.ntiles;
        auto first_tile = [&](int lb) -> uint64_t {
            if (!rotated) return (uint64_t)lb * U % nt;
            const uint64_t qb = (uint64_t)lb * U / nt;
            return ((uint64_t)lb - (uint64_t)wv::bf_first_block(qb, nt, U)) * U % nt;
        };
        std::vector<int>& ord = ix->blk_order_host;
        ord.resize(nb);
        for (int i = 0; i < nb; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return first_tile(a) < first_tile(b); });
        HIP_TRY(ix->blk_order.ensure((size_t)nb * 4));
        HIP_TRY(hipMemcpyAsync(ix->blk_order.p, ord.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));   // (pageable source; a later schedule rewrites it)
        std::copy(key, key + 4, ix->blk_key);
    }
    *out = ix->blk_order.as<int>();
    return WV_OK;
}

// f16 key pass (wv_h16.hip) over the whole corpus, optionally masked by a
// shared allow list: query image + scale, an optional seed pre-pass over every
// H_SAMPLE-th tile (its finalize yields per-query thresholds), the main pass
// seeded with them, and the certifying finalize, which flags uncertified
// queries in ix->fail for the device-resolved fallback (queue_fbd).
// rowidx (nullable): the ascending row list of a compacted shared allow list
// (compact_allowed) -- the pass then runs over an f16 image of just those N
// rows (gathered here) and the candidate ids are mapped back to rows before
// the finalize; d_allow is then already applied
int run_h16(wv_index* ix, const float* d_q, int nq, int k, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N,
            uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s,
            const uint32_t* rowidx = nullptr, const uint32_t* n_dev = nullptr) {
    const int ns = ix->h16_ns;
    const bool wd = ix->h16_wide;   // D > 128: the wide-D kernel
    // D <= 128: 8-wave (512-query) workgroups, one per CU; D > 128: 256-row
    // tiles x 256-query blocks, one workgroup per CU
    const int tile_rows = wd ? wv::HW_BN : wv::H_BN, bq = wd ? wv::HW_BQ : 512;
    // lists (and seed minima) per query and slot, entries per list
    const int prod = wd ? wv::HW_PROD : wv::H_PROD;
    const int kp = wv::BF_KP;
    const uint64_t ntl = (N + tile_rows - 1) / tile_rows;
    const uint64_t words = ntl * (uint64_t)(tile_rows / 64);   // allow words the kernel reads
    const uint64_t* allow = d_allow;
    if (d_allow && (allow_nbits + 63) / 64 < words) {
        HIP_TRY(ix->allow_pad.ensure(words * 8));
        HIP_TRY(hipMemsetAsync(ix->allow_pad.p, 0, words * 8, s));
        if (allow_nbits)
            HIP_TRY(hipMemcpyAsync(ix->allow_pad.p, d_allow, (allow_nbits + 63) / 64 * 8, hipMemcpyDeviceToDevice, s));
        allow = ix->allow_pad.as<uint64_t>();
    }
    const int nqb = (nq + bq - 1) / bq;
    const size_t qbytes = (size_t)nqb * bq * ns * 16 * 2;
    HIP_TRY(ix->qimg16.ensure(qbytes));
    HIP_TRY(ix->qres.ensure((size_t)nq * 4));
    HIP_TRY(ix->tau.ensure((size_t)nq * 4));
    HIP_TRY(ix->gtau.ensure((size_t)nq * 4));
    HIP_TRY(ix->q_nrm2.ensure((size_t)nq * 4));
    HIP_TRY(ix->fail.ensure((size_t)nq * 4));
    HIP_TRY(ix->fail_thr.ensure((size_t)nq * 4));
    // |q|^2 and, in the same pass, the batch's max |q_i|; B = f16(s_q b),
    // b = -2q (L2) or -q, s_q from max |b|
    const float bsign = ix->metric == WV_L2_SQUARED ? -2.f : -1.f;
    HIP_TRY(ix->qmax_part.ensure((size_t)((nq + 3) / 4) * 4));
    HIP_TRY(wv_launch_qnorm(d_q, nq, ix->dim, ix->dpad, ix->metric, ix->q_nrm2.as<float>(), ix->qmax_part.as<float>(),
                            s));
    HIP_TRY(hipMemsetAsync(ix->qimg16.p, 0, qbytes, s));
    HIP_TRY(wv_launch_h16_qscale(ix->qmax_part.as<float>(), (nq + 3) / 4, ix->qmax.as<unsigned int>(), bsign,
                                 ix->qscale.as<float>(), s));
    HIP_TRY(wv_launch_h16_rows(d_q, ix->dpad, nullptr, nq, ix->dim, ns, bsign, 1.f, ix->qmax.as<unsigned int>(),
                               ix->qimg16.p, 0, nullptr, ix->qres.as<float>(), 0, s));
    const void* ximg = ix->ximg16.p;
    const float* xnorm = ix->xnorm.as<float>();
    const uint64_t* excl = ix->excl.as<uint64_t>();
    if (rowidx) {
        // the allowed rows' image in list order (whole tiles, zero padded),
        // their |x|^2, and exclusion bits set only past N
        const uint64_t rows = ntl * tile_rows, ew = rows / 64 + 2;
        HIP_TRY(ix->cxnorm.ensure(rows * 4));
        HIP_TRY(ix->cexcl.ensure(ew * 8));
        HIP_TRY(hipMemsetAsync(ix->cxnorm.p, 0, rows * 4, s));
        if (!wd) {   // (D > 128: the pass reads the row-major image through the list itself)
            const size_t ib = rows * (size_t)ns * 16 * 2;
            HIP_TRY(ix->cimg16.ensure(ib));
            HIP_TRY(wv_launch_h16_rows_gather(ix->vecs.as<float>(), ix->ldx, rowidx, N, rows, ix->dim, ns, ix->h16_sx,
                                              ix->cimg16.p, s));
            ximg = ix->cimg16.p;
        }
        HIP_TRY(wv_launch_h16_compact_aux(ix->xnorm.as<float>(), rowidx, N, n_dev, ix->cxnorm.as<float>(),
                                          ix->cexcl.as<uint64_t>(), ew, s));
        xnorm = ix->cxnorm.as<float>();
        excl = ix->cexcl.as<uint64_t>();
        allow = nullptr;
    }
    if (ix->metric == WV_L2_SQUARED)
        HIP_TRY(wv_launch_h16_xns(xnorm, ntl * tile_rows, ix->h16_sx, ix->qscale.as<float>(), ix->xns.as<float>(), s));
    wv::H16Params hp{};
    hp.X = ximg;
    hp.rowidx = wd ? rowidx : nullptr;
    hp.Q = ix->qimg16.p;
    hp.xns = ix->xns.as<float>();
    hp.excl = excl;
    hp.allow = allow;
    hp.N = N;
    hp.nq = nq;
    hp.metric = ix->metric;
    hp.n_qblocks = nqb;
    // 64-row tiles the pass need not mask: every row present and eligible
    // (no allow list; a compacted scan: the rows below N)
    hp.clean_tiles = wd ? 0 : rowidx ? N / wv::H_BN : allow ? 0 : std::min<uint64_t>(ix->clean_words, N / wv::H_BN);
    hp.locality = 1;   // XCD-contiguous workgroup ids
    wv::BfFinParams fp{};
    fp.X = ix->vecs.as<float>();
    fp.Q = d_q;
    fp.qnorm = ix->q_nrm2.as<float>();
    fp.xnorm_max = ix->maxnorm_host;
    fp.nq = nq;
    fp.D = ix->dim;
    fp.ldx = ix->ldx;
    fp.ldq = ix->dpad;
    fp.metric = ix->metric;
    fp.k = k;
    fp.id_base = ix->cfg.id_base;
    fp.out_ids = d_out_ids;
    fp.out_d = d_out_d;
    fp.out_n = d_out_n;
    fp.fail = ix->fail.as<int32_t>();
    fp.fail_thr = ix->fail_thr.as<float>();
    fp.bq = bq;
    fp.prod = prod;
    fp.kp = kp;
    fp.h16 = 1;
    hp.ns = ns;
    fp.qscale = ix->qscale.as<float>();
    fp.sx = ix->h16_sx;
    fp.ex_max = ix->h16_ex;
    fp.qres = ix->qres.as<float>();
    // seed pre-pass: the k-th exact distance over every H_SAMPLE-th tile bounds
    // each query's true k-th distance, hence the keys worth keeping
    // k > FIN_KF (the wide finalize): at least k slots per query block, i.e.
    // >= 2k lists of BF_KP per query, so that no list is likely to hold more
    // than BF_KP of the top k (which would leave its tail below the k-th key
    // and fail the certificate); the seed pass needs >= k minima likewise
    const bool wide = k > wv::FIN_KF;
    auto target = [&](uint64_t tiles) {
        uint64_t t = (uint64_t)ix->n_cus;
        if (wide) t = std::max<uint64_t>(t, (uint64_t)nqb * std::min<uint64_t>(tiles, (uint64_t)k + 2));
        return (int)std::min<uint64_t>(t, 1u << 30);
    };
    // cross-slot threshold (32x32x16 pass, <= 32 list heads per query; on
    // unless WV_H16_XSLOT=0): 2.87-2.91 vs 2.98-3.00 ms per 1M x 10k key pass
    const char* xe = std::getenv("WV_H16_XSLOT");
    const bool xs_on = !xe || std::atoi(xe) != 0;
    auto xs_fits = [&](const wv::BfSchedule& sc) { return xs_on && !wd && 2 * sc.n_slots <= 32 && k <= 2 * sc.n_slots; };
    // The seed's tile stride (WV_H16_SAMPLE: for measurements).  Where the
    // main pass will run the cross-slot exchange, its bounds overtake the
    // seed's within the first eighth of a segment, so a sparser seed costs
    // fewer insertion events than its pre-pass saves (H_SAMPLE_XS; the main
    // pass's schedule does not depend on the stride).
    int sample = wv::H_SAMPLE;
    if (!wd && !n_dev && xs_fits(wv::bf_schedule(nq, N, target(ntl), bq, tile_rows))) sample = wv::H_SAMPLE_XS;
    if (const char* e = std::getenv("WV_H16_SAMPLE")) sample = std::max(1, std::atoi(e));
    // (seeded from H_SEED_MIN_TILES tiles on, whatever the stride)
    const bool seed = !wd && ntl >= (uint64_t)wv::H_SEED_MIN_TILES && !std::getenv("WV_H16_NO_SEED");
    // the wide pass: query blocks cut at the same tile offsets where that
    // costs no work (bf_schedule_aligned)
    wv::BfSchedule sch{};
    if (n_dev) {
        // a device-counted list (N its bound): S slots per query block, the
        // kernel sizes their runs (H16Params.n_dev); finalize and remap see
        // S one-tile slots, which index the lists the same way
        if (!wd || wide) return fail(WV_ESTATE, "run_h16: device-counted rows need the wide-D pass");
        const int S = std::max(1, target(ntl) / nqb);
        sch.bq = bq;
        sch.ntiles = (uint64_t)S;
        sch.units_per_block = 1;
        sch.n_blocks = nqb * S;
        sch.n_slots = S + 1;
    }
    if (wd && !wide && sch.n_blocks == 0) sch = wv::bf_schedule_aligned(nq, N, target(ntl), bq, tile_rows, false);
    if (sch.n_blocks == 0)
        sch = wv::bf_schedule(nq, N, target(ntl), bq, tile_rows);
    if (wide && (uint64_t)sch.n_slots * prod * kp > (uint64_t)wv::FINW_NE)
        return fail(WV_ESTATE, "run_h16: too many lists for the wide finalize");
    HIP_TRY(ix->cand_d.ensure((size_t)nq * sch.n_slots * prod * kp * 4));
    HIP_TRY(ix->cand_id.ensure((size_t)nq * sch.n_slots * prod * kp * 4));
    // the seed pre-pass: minima over every sample-th tile -> thresholds (tau, gtau)
    auto seed_minima = [&]() -> int {
        const uint64_t nt = (ntl + sample - 1) / sample;
        const wv::BfSchedule ms = wv::bf_schedule(nq, nt * wv::H_BN, target(nt), bq, wv::H_BN);
        HIP_TRY(ix->cand_d.ensure((size_t)nq * std::max(ms.n_slots * prod, sch.n_slots * prod * kp) * 4));
        hp.ntiles = ms.ntiles;
        hp.ntiles_real = ms.ntiles;
        hp.units_per_block = ms.units_per_block;
        hp.n_slots = ms.n_slots;
        hp.tile_stride = sample;
        hp.out_d = ix->cand_d.as<float>();
        hp.out_id = nullptr;
        HIP_TRY(wv_launch_bf_h16(&hp, ns, 1, s));
        wv::H16SeedParams sp{};
        sp.minima = ix->cand_d.as<float>();
        sp.n_slots = ms.n_slots;
        sp.ntiles = ms.ntiles;
        sp.units_per_block = ms.units_per_block;
        sp.nq = nq;
        sp.k = k;
        sp.metric = ix->metric;
        sp.D = ix->dim;
        sp.qscale = ix->qscale.as<float>();
        sp.sx = ix->h16_sx;
        sp.qnorm = ix->q_nrm2.as<float>();
        sp.xnorm_max = ix->maxnorm_host;
        sp.ex_max = ix->h16_ex;
        sp.qres = ix->qres.as<float>();
        sp.tau = ix->tau.as<float>();
        sp.gtau = ix->gtau.as<unsigned int>();
        sp.bq = bq;
        HIP_TRY(wv_launch_h16_seed(&sp, s));
        return WV_OK;
    };
    if (seed) {
        TREC(6);
        if (int rc = seed_minima()) return rc;
        TREC(7);
    }
    hp.ntiles = sch.ntiles;
    hp.ntiles_real = ntl;
    hp.units_per_block = sch.units_per_block;
    hp.n_slots = sch.n_slots;
    hp.n_dev = n_dev;
    hp.tile_stride = 1;
    // the running threshold (k <= 2 BF_KP), started at the seed's
    if (!seed) HIP_TRY(hipMemsetAsync(ix->gtau.p, 0xFF, (size_t)nq * 4, s));
    hp.gtau = ix->gtau.as<unsigned int>();
    // (with the seed's threshold the running one only adds work: measured
    // 3.048 vs 3.092 ms per 1M x 10k key pass; without a seed -- corpora below
    // 64 * H_SAMPLE tiles -- it cuts the pass 4.13 -> 3.43 ms at 1M)
    // (the wide-D pass publishes from a lane pair's two lists: k <= 2 BF_KP)
    hp.kth = k <= (wd ? 2 * kp : prod * kp) && !seed && !std::getenv("WV_H16_NO_RUNNING")
                 ? k
                 : 0;
    // cross-slot threshold (xs_fits above)
    if (xs_fits(sch)) {
        const size_t gb = (size_t)nq * 2 * sch.n_slots * 4;
        HIP_TRY(ix->gslot.ensure(gb));
        HIP_TRY(hipMemsetAsync(ix->gslot.p, 0x7F, gb, s));   // 3.4e38: no head yet
        hp.gslot = ix->gslot.as<float>();
        hp.xslot = 1;
        hp.kth = k;
    }
    if (hp.kth) {
        HIP_TRY(ix->marg.ensure((size_t)nq * 4));
        HIP_TRY(wv_launch_h16_margin(ix->metric, ix->dim, ix->q_nrm2.as<float>(), ix->qres.as<float>(),
                                     ix->maxnorm_host, ix->h16_ex, ix->h16_sx, ix->qscale.as<float>(), nq,
                                     ix->marg.as<float>(), s));
        hp.marg = ix->marg.as<float>();
    }
    hp.out_d = ix->cand_d.as<float>();
    hp.out_id = ix->cand_id.as<uint32_t>();
    // the 8-wave D <= 128 pass on the flat schedule: tiles rotated per query
    // block (locality bit 2): 2.73-2.75 -> 2.66-2.68 ms per 1M x 10k pass,
    // L2-miss bytes 5.23 -> 0.66 GB
    const bool rotate = !wd && nqb >= 2 && sch.ntiles == ntl;
    if (rotate) hp.locality |= 2;
    if (int rc = block_order(ix, (uint64_t)nqb, sch, s, &hp.block_order, rotate)) return rc;
    TREC(0);
    HIP_TRY(wd ? wv_launch_bf_h16w(&hp, s) : wv_launch_bf_h16(&hp, ns, 0, s));
    TREC(1);
    // compacted scan: the candidate positions map to rows -- inside the
    // finalize for its FIN_KF selected entries, or (the wide finalize) all
    // of them first
    if (rowidx && wide)
        HIP_TRY(wv_launch_remap_ids(ix->cand_id.as<uint32_t>(), nq, sch.n_slots, prod * kp, bq, sch.ntiles,
                                    sch.units_per_block, rowidx, N, n_dev, s));
    if (rowidx && !wide) {
        fp.rowidx = rowidx;
        fp.rowidx_n = N;
        fp.rowidx_ndev = n_dev;
    }
    fp.cand_d = ix->cand_d.as<float>();
    fp.cand_id = ix->cand_id.as<uint32_t>();
    fp.n_slots = sch.n_slots;
    fp.ntiles = sch.ntiles;
    fp.units_per_block = sch.units_per_block;
    HIP_TRY(wv_launch_h16_gtau(ix->gtau.as<unsigned int>(), nq, ix->h16_sx, ix->qscale.as<float>(), ix->tau.as<float>(),
                               s));
    fp.tau_in = ix->tau.as<float>();
    TREC(2);
    HIP_TRY(wide ? wv_launch_bf_finalize_wide(&fp, s) : wv_launch_bf_finalize(&fp, s));
    TREC(3);
    return WV_OK;
}

// Queue the device-resolved fallback for the queries whose flag in ix->fail
// is set (threshold ix->fail_thr): no host round trip (wv_bf.hip, fbd kernels).
int queue_fbd(wv_index* ix, const float* d_q, int nq, int k, const uint64_t* d_allow, uint64_t allow_nbits,
              uint64_t allow_stride, uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s) {
    const uint64_t N = ix->n_rows;
    HIP_TRY(ix->fbd_list.ensure((size_t)nq * 4));
    HIP_TRY(ix->fbd_nf.ensure(16));
    HIP_TRY(ix->fbd_over.ensure((size_t)nq * 4));
    HIP_TRY(ix->fbd_cd.ensure((size_t)nq * wv::FB_CAP * 4));
    HIP_TRY(ix->fbd_ci.ensure((size_t)nq * wv::FB_CAP * 4));
    HIP_TRY(ix->fbd_cn.ensure((size_t)nq * 4));
    HIP_TRY(ix->fbd_scr.ensure((size_t)wv::FBD_SCR * std::max<uint64_t>(N, 1) * 4));
    HIP_TRY(ix->stat_acc.ensure(48));
    wv::FbParams bp{};
    bp.X = ix->vecs.as<float>();
    bp.Q = d_q;
    bp.qidx = ix->fbd_list.as<int32_t>();
    bp.thr = ix->fail_thr.as<float>();
    bp.tomb = ix->excl.as<uint64_t>();
    bp.tomb_nbits = ix->capacity;
    bp.allow = d_allow;
    bp.allow_nbits = allow_nbits;
    bp.allow_stride = allow_stride;
    bp.N = N;
    bp.nf = nq;
    bp.D = ix->dim;
    bp.ldx = ix->ldx;
    bp.ldq = ix->dpad;
    bp.metric = ix->metric;
    bp.k = k;
    bp.id_base = ix->cfg.id_base;
    bp.cand_d = ix->fbd_cd.as<float>();
    bp.cand_id = ix->fbd_ci.as<uint32_t>();
    bp.cand_n = ix->fbd_cn.as<uint32_t>();
    bp.out_ids = d_out_ids;
    bp.out_d = d_out_d;
    bp.out_n = d_out_n;
    bp.overflow = ix->fbd_over.as<int32_t>();
    bp.d_nf = ix->fbd_nf.as<int32_t>();
    bp.scratch = ix->fbd_scr.as<float>();
    bp.n_scr = wv::FBD_SCR;
    bp.fb_total = ix->stat_acc.as<unsigned long long>() + 2;
#ifdef WV_ABLATION_BUILD
    if (std::getenv("WV_ABLATE_NO_FALLBACK")) return WV_OK;   // kernel ablations only (tools/h16_ablate.sh)
#endif
    HIP_TRY(wv_launch_fbd(ix->fail.as<int32_t>(), nq, &bp, s));
    return WV_OK;
}

// Brute force (flatSearch semantics) over a device batch of prepared queries.
// d_rowmask (nullable, with per-query allow lists only): a shared bitmap that
// contains every row any query may return (the delta set of wv_index_add);
// its rows are compacted and each query's own list is tested per row.
int run_exact(wv_index* ix, const float* d_q, int nq, int k, const uint64_t* d_allow, uint64_t allow_nbits,
              uint64_t allow_stride, uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s,
              const uint64_t* d_rowmask = nullptr, uint64_t rowmask_nbits = 0) {
    if (ix->pq_on)   // flatSearch on a compressed index ranks by PQ distance (index.go:493-511)
        return run_pq_flat(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s,
                           d_rowmask, rowmask_nbits);
    const uint64_t N = ix->n_rows;
    if (N == 0 || nq == 0) {
        if (nq) HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t) * nq, s));
        return WV_OK;
    }
    // the f16 pass (whole corpus or a shared allow list) serves k up to
    // BF_WIDE_KMAX; the other key passes k up to BF_FAST_KMAX
    const bool h16_ok = ix->use_h16 && !allow_stride && !d_rowmask;
    // the key pass + finalize ran: fail_thr holds each failed query's bound
    const bool keyed = k <= wv::BF_FAST_KMAX || (h16_ok && k <= wv::BF_WIDE_KMAX);
    if (keyed) {
        // A shared allow list that keeps under half the corpus is compacted
        // into a row list first: the contraction then runs over |allow| rows
        // (the reference's flatSearch also walks only the allow list,
        // flat_search.go:25-58) instead of masking N.
        uint64_t n_scan = N;
        const uint32_t* d_rowidx = nullptr;
        const uint64_t* cmask = d_allow && !allow_stride ? d_allow : d_rowmask;
        const uint64_t cbits = d_allow && !allow_stride ? allow_nbits : rowmask_nbits;
        // The wide-D f16 pass (k <= FIN_KF) compacts every shared list with
        // no host round trip: its per-lane fill reads a compacted tile at the
        // cost of a contiguous one, so the list's length need not steer the
        // scan (WV_BF_SYNC_COMPACT=1: the read-back rule below, measurements)
        if (cmask && !d_rowmask && h16_ok && ix->h16_wide && k <= wv::FIN_KF && !std::getenv("WV_BF_SYNC_COMPACT") &&
            !std::getenv("WV_BF_NO_COMPACT")) {
            const uint32_t* n_dev = nullptr;
            const uint64_t n_bound = std::min<uint64_t>(N, cbits);
            if (n_bound == 0) {
                HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t) * nq, s));
                return WV_OK;
            }
            if (int rc = compact_allowed_dev(ix, cmask, cbits, N, &n_dev, s)) return rc;
            if (int rc = run_h16(ix, d_q, nq, k, nullptr, 0, n_bound, d_out_ids, d_out_d, d_out_n, s,
                                 ix->rowidx.as<uint32_t>(), n_dev))
                return rc;
            return queue_fbd(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
        }
        if (cmask) {
            uint64_t n_ok = 0;
            int rc = compact_allowed(ix, cmask, cbits, N, &n_ok, s, d_rowmask != nullptr, nq);
            if (rc) return rc;
            if (n_ok == 0) {
                HIP_TRY(hipMemsetAsync(d_out_n, 0, sizeof(int32_t) * nq, s));
                return WV_OK;
            }
            // a list worth compacting (worth_compacting): the scan runs over
            // its rows -- on the f16 pass over their gathered image (h16_ok),
            // else (below 1/2 or 1/8) on the fp32 pass over the row list
            const bool compact = (worth_compacting(n_ok, N, nq) && !std::getenv("WV_BF_NO_COMPACT")) || d_rowmask;
            if (compact && h16_ok) {
                int rc2 = run_h16(ix, d_q, nq, k, nullptr, 0, n_ok, d_out_ids, d_out_d, d_out_n, s,
                                  ix->rowidx.as<uint32_t>());
                if (rc2) return rc2;
                return queue_fbd(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
            }
            // (no gathered f16 pass: the f16 pass masks the whole corpus
            // unless the list keeps under 1/8 of it)
            const uint64_t frac = ix->use_h16 && !allow_stride ? 8 : 2;
            if (((frac * n_ok < N && !std::getenv("WV_BF_NO_COMPACT")) || d_rowmask) && k <= wv::BF_FAST_KMAX) {
                n_scan = n_ok;
                d_rowidx = ix->rowidx.as<uint32_t>();
            }
        }
        if (ix->use_h16 && !d_rowidx && !allow_stride) {
            const uint64_t* sh = d_allow && !allow_stride ? d_allow : nullptr;
            int rc = run_h16(ix, d_q, nq, k, sh, allow_nbits, N, d_out_ids, d_out_d, d_out_n, s);
            if (rc) return rc;
            return queue_fbd(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
        }
        // bf16x3 key pass on native images (whole-corpus or shared allow list
        // scans, opt-in WV_BF_SPLIT=1): 256-query blocks, one 512-thread
        // workgroup per CU, two waves per SIMD (wv_bf_split_kernel)
        const bool split = ix->use_split && !d_rowidx && !allow_stride;
        const int bq = split ? 2 * wv::BF_BQ : wv::BF_BQ;
        const int prod = wv::BF_PROD;
        const int n_qblocks = (nq + bq - 1) / bq;
        const wv::BfSchedule sch =
            wv::bf_schedule(nq, n_scan, bq == wv::BF_BQ ? ix->bf_blocks : ix->bf_blocks / 2, bq);
        const size_t n_lists = (size_t)sch.n_slots * prod;
        HIP_TRY(ix->cand_d.ensure((size_t)nq * n_lists * wv::BF_KP * 4));
        HIP_TRY(ix->cand_id.ensure((size_t)nq * n_lists * wv::BF_KP * 4));
        HIP_TRY(ix->q_nrm2.ensure((size_t)nq * 4));
        HIP_TRY(ix->fail.ensure((size_t)nq * 4));
        HIP_TRY(wv_launch_qnorm(d_q, nq, ix->dim, ix->dpad, ix->metric, ix->q_nrm2.as<float>(), nullptr, s));
        // B operand in whole bq-row query blocks, zero rows past nq: -2q
        // (L2) or -q, as fp32 rows or (split key pass: whole-corpus or shared
        // allow list scans) as the native bf16 hi/lo image
        const size_t nq_pad = (size_t)n_qblocks * bq;
        const int ldb = split ? ix->ldx : ix->dpad;
        const float bscale = ix->metric == WV_L2_SQUARED ? -2.f : -1.f;
        HIP_TRY(ix->q_scaled.ensure(nq_pad * ldb * 4));
        if (split) {
            HIP_TRY(wv_launch_split_rows(d_q, ix->dpad, nullptr, nq_pad, nq, ix->dim, bscale, ix->q_scaled.p, ldb, 0, s));
        } else {
            if (nq_pad > (size_t)nq)
                HIP_TRY(hipMemsetAsync(ix->q_scaled.as<float>() + (size_t)nq * ldb, 0, (nq_pad - nq) * ldb * 4, s));
            HIP_TRY(wv_launch_scale(d_q, ix->q_scaled.as<float>(), (uint64_t)nq * ix->dpad, bscale, s));
        }
        wv::BfParams bp{};
        bp.split = split ? 1 : 0;
        bp.bq = bq;
        bp.prod = prod;
        bp.locality = 3;   // XCD-contiguous workgroups, aligned tile rotation
        bp.X = split ? ix->xsplit.as<float>() : ix->vecs.as<float>();
        bp.Q = ix->q_scaled.as<float>();
        bp.xnorm = ix->xnorm.as<float>();
        bp.tomb = d_rowidx ? nullptr : ix->excl.as<uint64_t>();
        bp.tomb_nbits = ix->capacity;
        // compacted rows carry the shared list already; per-query lists are
        // still tested (per gathered row)
        bp.allow = d_rowidx && !allow_stride ? nullptr : d_allow;
        bp.allow_nbits = allow_nbits;
        bp.allow_stride = allow_stride;
        bp.rowidx = d_rowidx;
        bp.N = n_scan;
        bp.nq = nq;
        bp.D = ix->dim;
        bp.ldx = ix->ldx;
        bp.ldq = ldb;
        bp.metric = ix->metric;
        bp.n_qblocks = n_qblocks;
        bp.n_slots = sch.n_slots;
        bp.ntiles = sch.ntiles;
        bp.units_per_block = sch.units_per_block;
        bp.out_d = ix->cand_d.as<float>();
        bp.out_id = ix->cand_id.as<uint32_t>();
        TREC(0);
        HIP_TRY(wv_launch_bf_mfma(&bp, s));
        TREC(1);
        const float maxn = ix->maxnorm_host;   // cached at every row write
        wv::BfFinParams fp{};
        fp.X = ix->vecs.as<float>();
        fp.Q = d_q;
        fp.cand_d = ix->cand_d.as<float>();
        fp.cand_id = ix->cand_id.as<uint32_t>();
        fp.qnorm = ix->q_nrm2.as<float>();
        fp.xnorm_max = maxn;
        fp.n_slots = sch.n_slots;
        fp.ntiles = sch.ntiles;
        fp.units_per_block = sch.units_per_block;
        fp.nq = nq;
        fp.D = ix->dim;
        fp.ldx = ix->ldx;
        fp.ldq = ix->dpad;
        fp.metric = ix->metric;
        fp.k = k;
        fp.id_base = ix->cfg.id_base;
        fp.out_ids = d_out_ids;
        fp.out_d = d_out_d;
        fp.out_n = d_out_n;
        fp.fail = ix->fail.as<int32_t>();
        HIP_TRY(ix->fail_thr.ensure((size_t)nq * 4));
        fp.fail_thr = ix->fail_thr.as<float>();
        fp.split = bp.split;
        fp.bq = bq;
        fp.prod = prod;
        TREC(2);
        HIP_TRY(wv_launch_bf_finalize(&fp, s));
        TREC(3);
        return queue_fbd(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    }
    // k past every key pass: each query by a full scan and sort
    ix->last_fallbacks += (uint64_t)nq;
    for (int q = 0; q < nq; ++q) {
        const uint64_t* al = d_allow ? d_allow + (allow_stride ? (uint64_t)q * allow_stride : 0) : nullptr;
        int rc = ix->pq_on ? run_pq_flat(ix, d_q + (size_t)q * ix->dpad, 1, k, al, allow_nbits, 0,
                                         d_out_ids + (size_t)q * k, d_out_d + (size_t)q * k, d_out_n + q, s, nullptr, 0)
                           : exact_full(ix, d_q + (size_t)q * ix->dpad, k, al, allow_nbits, d_out_ids + (size_t)q * k,
                                        d_out_d + (size_t)q * k, d_out_n + q, s);
        if (rc) return rc;
    }
    return WV_OK;
}

int run_hnsw(wv_index* ix, const float* d_q, int nq, int k, int ef, const uint64_t* d_allow, uint64_t allow_nbits,
             uint64_t allow_stride, uint64_t* d_out_ids, float* d_out_d, int32_t* d_out_n, hipStream_t s) {
    if (!ix->has_graph || ix->gn == 0) return fail(WV_ESTATE, "no graph uploaded");
    const int efc = std::max(64, (ef + 63) / 64 * 64);
    // Side candidates S (traversed but ineligible: search.go:282-298) and the
    // exact set of expanded side candidates exist only under a filter,
    // tombstones or nil nodes.  Without them the wave state shrinks and more
    // queries are in flight (the search is latency-bound on its gathers).  A
    // stray ineligible node still ends in the exact fallback (status bit 0),
    // never in a wrong answer.
    const bool filtered = d_allow != nullptr || ix->any_tomb || ix->any_nil;
    const int sc = filtered ? 256 : 0;
    const int xs_log2 = filtered ? 9 : 0;
    // register results (unfiltered, ef <= 256): the wave's LDS is the query,
    // the batch and the visited cache only
    const bool reg = !filtered && efc <= 256;
    const int fixed = reg ? wv_hnsw_reg_per_wave_words(ix->dpad, 0) - 1
                          : wv_hnsw_per_wave_words(ix->dpad, efc, sc, 0, xs_log2) - 1;
    // per-wave LDS budget: 20 KiB filtered (8 waves per CU), 12 KiB otherwise
    int wave_kb = filtered ? 20 : 12;
    if (const char* e = std::getenv("WV_HNSW_WAVE_KB")) wave_kb = std::max(4, std::atoi(e));
    const int budget = wave_kb * 1024 / 4;
    int vc_tbits = 0;
    const int vc_log2 = choose_vc_log2(budget, fixed, ix->gn, &vc_tbits);
    int per_wave = reg ? wv_hnsw_reg_per_wave_words(ix->dpad, vc_log2)
                       : wv_hnsw_per_wave_words(ix->dpad, efc, sc, vc_log2, xs_log2);
    per_wave = (per_wave + 3) & ~3;
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * per_wave * 4 > 160 * 1024) --wpb;
    if ((size_t)per_wave * 4 > 160 * 1024) return fail(WV_EINVAL, "hnsw LDS footprint too large");
    HIP_TRY(ix->status.ensure((size_t)nq * 4));
    HIP_TRY(ix->counters.ensure((size_t)nq * 8));
    wv::HnswParams hp{};
    hp.X = ix->vecs.as<float>();
    hp.levels = ix->levels.as<int8_t>();
    hp.layer0 = ix->layer0.as<uint32_t>();
    hp.upper_row = ix->upper_row.as<uint32_t>();
    hp.upper = ix->upper.as<uint32_t>();
    hp.tomb = ix->any_tomb ? ix->tomb.as<uint64_t>() : nullptr;
    hp.tomb_nbits = ix->capacity;
    hp.allow = d_allow;
    hp.allow_nbits = allow_nbits;
    hp.allow_stride = allow_stride;
    hp.Q = d_q;
    hp.N = ix->gn;
    hp.id_base = ix->cfg.id_base;
    hp.entrypoint = (uint32_t)ix->entrypoint;
    hp.D = ix->dim;
    hp.ldx = ix->ldx;
    hp.ldq = ix->dpad;
    hp.metric = ix->metric;
    hp.deg0 = ix->deg0;
    hp.degU = ix->degU;
    hp.max_level = ix->max_level;
    hp.upper_levels = ix->max_level;
    hp.nq = nq;
    hp.k = k;
    hp.ef = ef;
    hp.efc = efc;
    hp.sc = sc;
    hp.vc_log2 = vc_log2;
    hp.vc_tbits = vc_tbits;
    hp.xs_log2 = xs_log2;
    hp.dpad = ix->dpad;
    hp.per_wave_words = per_wave;
    hp.out_ids = d_out_ids;
    hp.out_d = d_out_d;
    hp.out_n = d_out_n;
    hp.status = ix->status.as<int32_t>();
    hp.counters = ix->counters.as<uint32_t>();
    if (ix->pq_on) hp.pq = pq_params(ix);   // compressed: PQ distances (search.go:171-199)
    // diagnostic: exact per-query visited bitmaps for the evaluation counts
    // (a bounded sample: nq x N bits of scratch, freed after the launch)
    void* uniq = nullptr;
    // (bounded by bytes too: a 100M-node graph would take 51 GB at nq 4096)
    if (std::getenv("WV_HNSW_UNIQUE_COUNTS") && nq <= 4096 && (size_t)nq * ((ix->gn + 63) / 64) * 8 <= ((size_t)1 << 30)) {
        hp.uniq_words = (ix->gn + 63) / 64;
        HIP_TRY(hipMallocAsync(&uniq, (size_t)nq * hp.uniq_words * 8, s));
        HIP_TRY(hipMemsetAsync(uniq, 0, (size_t)nq * hp.uniq_words * 8, s));
        hp.uniq = static_cast<unsigned long long*>(uniq);
    }
    TREC(4);
    // Filtered / tombstoned / nil-node searches with ef <= 128 (round 6):
    // the side-register path.  Layer 0 has an exact visited bitmap per query
    // in HBM (nothing evaluated or queued twice) and a side set whose smallest
    // keys sit in LDS, sized from the eligible fraction p (the live side set
    // peaks near 1.4 ef (1-p)/p: oracle side diagnostics), the
    // rest spilled to HBM.  Only a spill past its capacity takes the exact
    // fallback.  WV_HNSW_NO_SIDE=1 keeps the LDS path.
    const bool side = filtered && !ix->pq_on && efc <= 128 && !std::getenv("WV_HNSW_NO_SIDE");
    if (side) {
        double p_el = 1.0;
        if (d_allow) {
            const int rows = allow_stride ? nq : 1;
            const uint64_t words = std::min<uint64_t>((allow_nbits + 63) / 64, (ix->gn + 63) / 64);
            HIP_TRY(ix->g_cnt.ensure((size_t)rows * 8));
            HIP_TRY(hipMemsetAsync(ix->g_cnt.p, 0, (size_t)rows * 8, s));
            hipLaunchKernelGGL(popcount_rows_kernel, dim3(rows), dim3(256), 0, s, d_allow, words,
                               allow_stride ? allow_stride : words, rows, ix->g_cnt.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
            std::vector<unsigned long long> cnt(rows);
            HIP_TRY(hipMemcpyAsync(cnt.data(), ix->g_cnt.p, 8 * (size_t)rows, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const unsigned long long mn = *std::min_element(cnt.begin(), cnt.end());
            p_el = (double)mn / (double)std::max<uint64_t>(1, ix->gn);
        }
        p_el *= 1.0 - std::min(1.0, (double)ix->n_tomb / (double)std::max<uint64_t>(1, ix->gn));
        p_el = std::max(p_el, 1e-5);
        const double side_need = 1.4 * ef * (1.0 - p_el) / p_el;
        // per-wave LDS: 13 KiB (12 waves per CU); the side array takes what a
        // 2K-slot visited cache leaves, up to the live-set estimate
        int side_kb = 13;
        if (const char* e = std::getenv("WV_HNSW_SIDE_KB")) side_kb = std::max(4, std::atoi(e));
        const int xl = 8;   // the upper levels' expanded set
        const int budget_words = side_kb * 256;
        const int base_words = wv_hnsw_side_per_wave_words(ix->dpad, 0, 11, xl);
        const int max_rows = std::max(4, (budget_words - base_words) / 128);
        int side_rows = std::min(max_rows, std::max(4, (int)std::ceil((side_need + 64.0) / 64.0)));
        if (const char* e = std::getenv("WV_HNSW_SIDE_ROWS")) side_rows = std::max(4, std::atoi(e));
        wv::HnswParams hs = hp;
        hs.sc = 0;
        hs.side_rows = side_rows;
        hs.xs_log2 = xl;
        const int fixed = wv_hnsw_side_per_wave_words(ix->dpad, side_rows, 0, xl) - 1;
        hs.vc_log2 = std::max(10, choose_vc_log2(std::max(budget_words, fixed + 512), fixed, ix->gn, &hs.vc_tbits));
        int pw = (wv_hnsw_side_per_wave_words(ix->dpad, side_rows, hs.vc_log2, xl) + 3) & ~3;
        while (pw * 4 > 160 * 1024 && hs.vc_log2 > 8) {
            --hs.vc_log2;
            pw = (wv_hnsw_side_per_wave_words(ix->dpad, side_rows, hs.vc_log2, xl) + 3) & ~3;
        }
        if (pw * 4 > 160 * 1024) return fail(WV_EINVAL, "hnsw side state too large");
        hs.per_wave_words = pw;
        int wpb = 4;
        while (wpb > 1 && (size_t)wpb * pw * 4 > 160 * 1024) --wpb;
        // HBM scratch per query: the visited bitmap and the spill, in chunks
        // of at most WV_HNSW_SIDE_SCRATCH_MB (4 GiB) -- a 10M-row graph takes
        // 1.25 MB of bitmap a query
        hs.vwords = (ix->gn + 31) / 32;
        double cap = std::ceil(8.0 * side_need) + 4096.0;
        if (const char* e = std::getenv("WV_HNSW_SPILL_CAP")) cap = std::max(64, std::atoi(e));
        hs.spill_cap = (int)std::min(cap, (double)(1 << 22));
        const size_t per_q = hs.vwords * 4 + (size_t)hs.spill_cap * 8;
        size_t budget_b = (size_t)4 << 30;
        if (const char* e = std::getenv("WV_HNSW_SIDE_SCRATCH_MB")) budget_b = (size_t)std::max(1, std::atoi(e)) << 20;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, budget_b / per_q));
        HIP_TRY(ix->side_vb.ensure((size_t)chunk * hs.vwords * 4));
        HIP_TRY(ix->side_sp.ensure((size_t)chunk * hs.spill_cap * 8));
        hs.vbits = ix->side_vb.as<uint32_t>();
        hs.spill = ix->side_sp.as<uint32_t>();
        ix->last_side_rows = side_rows;
        ix->last_side_xs = hs.spill_cap;
        // Layer 0 with the exact bitmap below WV_HNSW_EV_BELOW (0.4) of the
        // rows eligible; above it (light filters, a few tombstones) the lossy
        // cache + expanded set, whose rare overflow re-runs exactly (redo).
        // Small batches (<= WV_HNSW_WG_MAX, 512): a workgroup per query.
        double ev_below = 0.4;
        if (const char* e = std::getenv("WV_HNSW_EV_BELOW")) ev_below = std::atof(e);
        const bool ev_first = p_el < ev_below;
        int wg_max = 512;
        if (const char* e = std::getenv("WV_HNSW_WG_MAX")) wg_max = std::atoi(e);
        hs.wg_helpers = nq <= wg_max ? 3 : 0;
        HIP_TRY(ix->stat_acc.ensure(48));
        hs.side_acc = ix->stat_acc.as<unsigned long long>();
        hs.ev_spec = std::getenv("WV_HNSW_EV_SPEC") ? 1 : 0;
        const int passes = ev_first ? 1 : 2;
        for (int pass = 0; pass < passes; ++pass) {
            for (int c0 = 0; c0 < nq; c0 += chunk) {
                const int cn = std::min(chunk, nq - c0);
                wv::HnswParams hc = hs;
                hc.nq = cn;
                hc.Q = d_q + (size_t)c0 * hp.ldq;
                if (hc.allow && allow_stride) hc.allow = d_allow + (size_t)c0 * allow_stride;
                hc.out_ids = d_out_ids + (size_t)c0 * k;
                hc.out_d = d_out_d + (size_t)c0 * k;
                hc.out_n = d_out_n + c0;
                hc.status = hp.status + c0;
                hc.counters = hp.counters + 2 * (size_t)c0;
                hc.redo = pass ? hc.status : nullptr;
                hc.vb_host_clear = std::getenv("WV_HNSW_VB_MEMSET") ? 1 : 0;
                if (hc.vb_host_clear && (ev_first || pass))
                    HIP_TRY(hipMemsetAsync(hs.vbits, 0, (size_t)cn * hs.vwords * 4, s));
                HIP_TRY(wv_launch_hnsw_side(&hc, wpb, ev_first || pass, s));
            }
        }
    } else {
    // small unfiltered batches (the batcher's callers): a workgroup per
    // query, whose three helper waves take the distance batches' other rows
    // -- while every workgroup is resident (up to 3 per CU at 158 VGPRs; a
    // 256-query batch 898 -> 705 us p50, profiles/r05/wg_latency.log).
    // WV_HNSW_WG_MAX: the largest such batch; 0 turns it off.
    int wg_max = 512;
    if (const char* e = std::getenv("WV_HNSW_WG_MAX")) wg_max = std::atoi(e);
    const bool wg = !filtered && !ix->pq_on && reg && nq <= wg_max;
    if (wg) {
        hp.wg_helpers = 3;
        HIP_TRY(wv_launch_hnsw_wg(&hp, s));
    } else {
        HIP_TRY(wv_launch_hnsw(&hp, wpb, s));
    }
    if (filtered && !std::getenv("WV_HNSW_NO_WIDE_SIDE")) {
        // second pass for the queries whose side set or expanded-set table
        // overflowed (status != 0; the others' waves exit at once): the same
        // search with a 2048-entry side set and a 2048-slot expanded set --
        // selective filters traverse many ineligible nodes (search.go:282-298:
        // at 10 % of the rows the reference's candidate heap reaches ~1.8k).
        // Only what still overflows here takes the exact fallback.
        wv::HnswParams h2 = hp;
        h2.redo = ix->status.as<int32_t>();
        h2.sc = 2048;
        h2.xs_log2 = 11;
        const int fixed2 = wv_hnsw_per_wave_words(ix->dpad, efc, h2.sc, 0, h2.xs_log2) - 1;
        h2.vc_log2 = choose_vc_log2(fixed2 + 1024, fixed2, ix->gn, &h2.vc_tbits);
        int pw2 = (wv_hnsw_per_wave_words(ix->dpad, efc, h2.sc, h2.vc_log2, h2.xs_log2) + 3) & ~3;
        h2.per_wave_words = pw2;
        int wpb2 = 4;
        while (wpb2 > 1 && (size_t)wpb2 * pw2 * 4 > 160 * 1024) --wpb2;
        if ((size_t)pw2 * 4 <= 160 * 1024) HIP_TRY(wv_launch_hnsw(&h2, wpb2, s));
    }
    }
    TREC(5);
    if (uniq) HIP_TRY(hipFreeAsync(uniq, s));
    HIP_TRY(ix->stat_acc.ensure(48));
    HIP_TRY(wv_launch_hnsw_stats(ix->counters.as<uint32_t>(), nq, ix->stat_acc.as<unsigned long long>(), s));
    if (!ix->pq_on) {
        // queries whose side state outgrew LDS: exact answer on the device
        HIP_TRY(ix->fail.ensure((size_t)nq * 4));
        HIP_TRY(ix->fail_thr.ensure((size_t)nq * 4));
        HIP_TRY(wv_launch_fbd_mark(ix->status.as<int32_t>(), nq, ix->fail.as<int32_t>(), ix->fail_thr.as<float>(),
                                   d_out_d, d_out_n, k, s));
        return queue_fbd(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    }
    std::vector<int32_t> st(nq);
    HIP_TRY(hipMemcpyAsync(st.data(), ix->status.p, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // Queries whose side-candidate set outgrew LDS are answered exactly
    // (flatSearch over the same allow list: a superset in quality).
    for (int q = 0; q < nq; ++q) {
        if (!st[q]) continue;
        ix->last_fallbacks++;
        const uint64_t* al = d_allow ? d_allow + (allow_stride ? (uint64_t)q * allow_stride : 0) : nullptr;
        int rc = ix->pq_on ? run_pq_flat(ix, d_q + (size_t)q * ix->dpad, 1, k, al, allow_nbits, 0,
                                         d_out_ids + (size_t)q * k, d_out_d + (size_t)q * k, d_out_n + q, s, nullptr, 0)
                           : exact_full(ix, d_q + (size_t)q * ix->dpad, k, al, allow_nbits, d_out_ids + (size_t)q * k,
                                        d_out_d + (size_t)q * k, d_out_n + q, s);
        if (rc) return rc;
    }
    return WV_OK;
}

// out[r][w] = a[r or 0][w] & b[w]  (rows x words; a_stride 0 = one shared row)
__global__ void and_bits_kernel(const uint64_t* a, uint64_t a_words, uint64_t a_stride, const uint64_t* b,
                                uint64_t words, int rows, uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words * (uint64_t)rows) return;
    const uint64_t r = i / words, w = i % words;
    const uint64_t av = a ? (w < a_words ? a[r * a_stride + w] : 0ull) : ~0ull;
    out[i] = av & b[w];
}

// knnSearchByVector over the uploaded graph, plus an exact pass over the
// delta set (rows added since the graph snapshot), merged by
// (dist, id): added rows are findable at once, as in the reference where
// Add inserts into the live graph (insert.go:43-65).  Exact over the delta is
// a superset in quality of a graph search.
int run_hnsw_delta(wv_index* ix, const float* d_q, int nq, int k, int ef, const uint64_t* d_allow,
                   uint64_t allow_nbits, uint64_t allow_stride, uint64_t* d_out_ids, float* d_out_d,
                   int32_t* d_out_n, hipStream_t s) {
    if (ix->delta_count == 0 || nq == 0)
        return run_hnsw(ix, d_q, nq, k, ef, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    const size_t nk = (size_t)nq * k;
    HIP_TRY(ix->dl_ids.ensure(2 * nk * 8));
    HIP_TRY(ix->dl_d.ensure(2 * nk * 4));
    HIP_TRY(ix->dl_n.ensure(2 * (size_t)nq * 4));
    uint64_t* ids = ix->dl_ids.as<uint64_t>();
    float* ds = ix->dl_d.as<float>();
    int32_t* ns = ix->dl_n.as<int32_t>();
    int rc = run_hnsw(ix, d_q, nq, k, ef, d_allow, allow_nbits, allow_stride, ids, ds, ns, s);
    if (rc) return rc;
    const uint64_t words = ix->bm_words;
    const int rows = d_allow && allow_stride ? nq : 1;
    HIP_TRY(ix->dmask.ensure((size_t)rows * words * 8));
    hipLaunchKernelGGL(and_bits_kernel, dim3((unsigned)((rows * words + 255) / 256)), dim3(256), 0, s, d_allow,
                       (allow_nbits + 63) / 64, allow_stride ? allow_stride : 0, ix->delta.as<uint64_t>(), words, rows,
                       ix->dmask.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    const uint64_t st = d_allow && allow_stride ? words : 0;
    const uint64_t e = ix->last_dist, x = ix->last_exp, f = ix->last_fallbacks;
    rc = run_exact(ix, d_q, nq, k, ix->dmask.as<uint64_t>(), ix->capacity, st, ids + nk, ds + nk, ns + nq, s,
                   st ? ix->delta.as<uint64_t>() : nullptr, ix->capacity);
    if (rc) return rc;
    ix->last_dist = e;
    ix->last_exp = x;
    ix->last_fallbacks += f;
    HIP_TRY(launch_merge_shards(ds, ids, ns, 2, nq, k, d_out_d, d_out_ids, d_out_n, s));
    return WV_OK;
}

}  // namespace

namespace wv_host {

// Visited-cache size (2^vc_log2 16-bit slots) for a per-wave LDS budget, and
// the tag width that makes slot + tag identify ids below n_nodes exactly
// (HnswParams.vc_tbits <= 15; a graph past 2^(vc_log2 + 15) nodes gets more
// slots than the budget would give).
int choose_vc_log2(int per_wave_budget_words, int fixed_words, uint64_t n_nodes, int* tbits) {
    int l = 13;
    while (l > 8 && fixed_words + ((1 << l) + 1) / 2 > per_wave_budget_words) --l;
    int hb = 1;
    while (hb < 32 && (1ull << hb) < n_nodes) ++hb;
    if (hb - l > 15) l = hb - 15;
    *tbits = hb > l ? hb - l : 0;
    return l;
}

hipError_t launch_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int D, float* dst, int ld_dst,
                              hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(128), 0, s, src, ld_src, idx, n, D, dst, ld_dst);
    return hipGetLastError();
}

// Core: device queries already padded to dpad and normalized (cosine).
int search_core(wv_index* ix, const float* d_q, int nq, int k, int ef, const uint64_t* d_allow,
                uint64_t allow_nbits, uint64_t allow_stride, int mode, uint64_t* d_out_ids, float* d_out_d,
                int32_t* d_out_n, hipStream_t s) {
    int rc = refresh_bitmaps(ix);
    if (rc) return rc;
    ix->last_dist = ix->last_exp = ix->last_fallbacks = 0;
    ix->last_side_rows = ix->last_side_xs = 0;
    HIP_TRY(ix->stat_acc.ensure(48));
    HIP_TRY(hipMemsetAsync(ix->stat_acc.p, 0, 48, s));
    ix->stat_stream = s;
    if (ix->timing) {
        if (ix->ev_used == ix->ev_pool.size()) {
            std::array<hipEvent_t, 8> e{};
            for (auto& x : e) HIP_TRY(hipEventCreate(&x));
            ix->ev_pool.push_back(e);
            ix->ev_mask.push_back(0);
        }
        ix->ev = ix->ev_pool[ix->ev_used].data();
        ix->ev_mask[ix->ev_used] = 0;
        ix->ev_used++;
    }
    if (ef <= 0) ef = search_time_ef(ix->cfg, k);
    if (mode == WV_MODE_EXACT)
        return run_exact(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    if (mode == WV_MODE_HNSW) {
        if (ef > wv::HNSW_EF_MAX)
            return run_exact(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
        return run_hnsw_delta(ix, d_q, nq, k, ef, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    }
    // AUTO: search.go:74-78
    const bool can_hnsw = ix->has_graph && ef <= wv::HNSW_EF_MAX;
    if (!d_allow || ix->cfg.forbid_flat) {
        if (can_hnsw)
            return run_hnsw_delta(ix, d_q, nq, k, ef, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
        return run_exact(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    }
    // allowList.Len() < flatSearchCutoff decides per query
    const int rows = allow_stride ? nq : 1;
    const uint64_t words = (allow_nbits + 63) / 64;
    HIP_TRY(ix->g_cnt.ensure((size_t)rows * 8));
    HIP_TRY(hipMemsetAsync(ix->g_cnt.p, 0, (size_t)rows * 8, s));
    hipLaunchKernelGGL(popcount_rows_kernel, dim3(rows), dim3(256), 0, s, d_allow, words,
                       allow_stride ? allow_stride : words, rows, ix->g_cnt.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> cnt(rows);
    HIP_TRY(hipMemcpyAsync(cnt.data(), ix->g_cnt.p, 8 * (size_t)rows, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> flat, knn;
    for (int q = 0; q < nq; ++q) {
        const unsigned long long c = cnt[allow_stride ? q : 0];
        if ((int64_t)c < ix->cfg.flat_search_cutoff || !can_hnsw) flat.push_back(q);
        else knn.push_back(q);
    }
    if (knn.empty())
        return run_exact(ix, d_q, nq, k, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    if (flat.empty())
        return run_hnsw_delta(ix, d_q, nq, k, ef, d_allow, allow_nbits, allow_stride, d_out_ids, d_out_d, d_out_n, s);
    // split the batch: gather each group, run, scatter back
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<int32_t>& sel = pass == 0 ? flat : knn;
        const int n = (int)sel.size();
        HIP_TRY(ix->g_idx.ensure((size_t)n * 4));
        HIP_TRY(ix->g_q.ensure((size_t)n * ix->dpad * 4));
        HIP_TRY(ix->g_ids.ensure((size_t)n * k * 8));
        HIP_TRY(ix->g_d.ensure((size_t)n * k * 4));
        HIP_TRY(ix->g_n.ensure((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(ix->g_idx.p, sel.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_gather_rows(d_q, ix->dpad, ix->g_idx.as<int32_t>(), n, ix->dpad, ix->g_q.as<float>(), ix->dpad, s));
        const uint64_t* al = d_allow;
        uint64_t ast = 0;
        if (allow_stride) {
            HIP_TRY(ix->g_allow.ensure((size_t)n * allow_stride * 8));
            hipLaunchKernelGGL(gather_words_kernel, dim3(n), dim3(256), 0, s, d_allow, allow_stride,
                               ix->g_idx.as<int32_t>(), n, ix->g_allow.as<uint64_t>());
            al = ix->g_allow.as<uint64_t>();
            ast = allow_stride;
        }
        HIP_TRY(hipGetLastError());
        int rc2 = pass == 0 ? run_exact(ix, ix->g_q.as<float>(), n, k, al, allow_nbits, ast, ix->g_ids.as<uint64_t>(),
                                        ix->g_d.as<float>(), ix->g_n.as<int32_t>(), s)
                            : run_hnsw_delta(ix, ix->g_q.as<float>(), n, k, ef, al, allow_nbits, ast,
                                       ix->g_ids.as<uint64_t>(), ix->g_d.as<float>(), ix->g_n.as<int32_t>(), s);
        if (rc2) return rc2;
        hipLaunchKernelGGL(scatter_results_kernel, dim3(n), dim3(64), 0, s, ix->g_ids.as<uint64_t>(),
                           ix->g_d.as<float>(), ix->g_n.as<int32_t>(), ix->g_idx.as<int32_t>(), n, k, d_out_ids,
                           d_out_d, d_out_n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return WV_OK;
}

// host queries -> device, padded, normalized for cosine (search.go:68-72)
int stage_queries(wv_index* ix, const float* q, int nq, const float** d_out, hipStream_t s) {
    HIP_TRY(ix->q_in.ensure((size_t)nq * ix->dpad * 4));
    if (ix->dpad == ix->dim) {
        HIP_TRY(hipMemcpyAsync(ix->q_in.p, q, (size_t)nq * ix->dim * 4, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(ix->stage.ensure((size_t)nq * ix->dim * 4));
        HIP_TRY(hipMemcpyAsync(ix->stage.p, q, (size_t)nq * ix->dim * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_pad_rows(ix->stage.as<float>(), ix->dim, nq, ix->dim, ix->q_in.as<float>(), ix->dpad, s));
    }
    if (ix->metric == WV_COSINE_DOT)
        HIP_TRY(wv_launch_normalize(ix->q_in.as<float>(), ix->q_in.as<float>(), nq, ix->dim, ix->dpad, s));
    *d_out = ix->q_in.as<float>();
    return WV_OK;
}

// the pinned slot grown to `need` bytes, with its event
int slot_reserve(wv_index::HostSlot& sl, size_t need) {
    if (sl.cap < need) {
        if (sl.pin) HIP_TRY(hipHostFree(sl.pin));
        sl.pin = nullptr;
        sl.cap = 0;
        const size_t want = std::max<size_t>(need + need / 4, 1 << 20);
        HIP_TRY(hipHostMalloc(&sl.pin, want, hipHostMallocDefault));
        sl.cap = want;
    }
    if (!sl.done) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    return WV_OK;
}

// Per-query allow lists given as ids (wv_search_batch_ids and
// wv_search_by_vector_distance_batch_ids; fn: the caller's name for the
// messages).  The offsets' checks, before any device call:
int ids_check_offsets(const std::string& fn, const uint64_t* allow_ids, const uint64_t* allow_offsets, int nq) {
    if (allow_offsets[0] != 0) return fail(WV_EINVAL, fn + ": allow_offsets[0] must be 0");
    for (int q = 0; q < nq; ++q)
        if (allow_offsets[q + 1] < allow_offsets[q]) return fail(WV_EINVAL, fn + ": allow_offsets must not decrease");
    if (allow_offsets[nq] && !allow_ids) return fail(WV_EINVAL, fn + ": null allow_ids");
    return WV_OK;
}

// ... and the lists into the pinned slot: ids narrowed to u32 (capacity <
// 2^31; larger ids name no row) at ids32, the kept lists' offsets at off
// [nq + 1]; a list that does not strictly ascend is refused.
int ids_stage(const std::string& fn, const uint64_t* allow_ids, const uint64_t* allow_offsets, int nq, uint32_t* ids32,
              uint64_t* off) {
    const uint64_t total = allow_offsets[nq];
    // In an ascending list the ids >= 2^31 are a suffix: each list's kept
    // length first (a list out of order is refused below, whatever was kept)
    uint64_t pos = 0;
    for (int q = 0; q < nq; ++q) {
        off[q] = pos;
        uint64_t m = allow_offsets[q + 1] - allow_offsets[q];
        while (m && allow_ids[allow_offsets[q] + m - 1] >= (1ull << 31)) --m;
        pos += m;
    }
    off[nq] = pos;
    // one pass over the lists: the ascending check and the narrowing, in
    // threads over equal shares of the ids when the batch is large (a 256 x
    // 40,000 batch reads 80 MB: one core's pass cost more than the search)
    auto narrow = [&](int q0, int q1) {
        uint64_t bad = 0;
        for (int q = q0; q < q1; ++q) {
            const uint64_t* a = allow_ids + allow_offsets[q];
            const uint64_t n = allow_offsets[q + 1] - allow_offsets[q], m = off[q + 1] - off[q];
            uint32_t* o = ids32 + off[q];
            for (uint64_t i = 0; i < m; ++i) o[i] = (uint32_t)a[i];
            for (uint64_t i = 1; i < n; ++i) bad |= (uint64_t)(a[i] <= a[i - 1]);
        }
        return bad != 0;
    };
    bool bad = false;
    const int nth = (int)std::min<uint64_t>(std::min(8, nq), total >> 18);
    if (nth <= 1) {
        bad = narrow(0, nq);
    } else {
        std::vector<std::thread> th;
        std::vector<char> tb((size_t)nth, 0);
        int q0 = 0;
        for (int t = 0; t < nth; ++t) {
            int q1 = q0;
            const uint64_t until = t == nth - 1 ? total : total / nth * (t + 1);
            while (q1 < nq && (allow_offsets[q1 + 1] <= until || t == nth - 1)) ++q1;
            th.emplace_back([&, t, q0, q1] { tb[t] = narrow(q0, q1); });
            q0 = q1;
        }
        for (auto& x : th) x.join();
        for (char c : tb) bad |= c != 0;
    }
    if (bad) return fail(WV_EINVAL, fn + ": allow ids must be strictly ascending within a query");
    return WV_OK;
}

// the staged lists and their offsets to the device (fi_ids, fi_off)
int ids_upload(wv_index* ix, const uint32_t* ids32, const uint64_t* off, int nq, hipStream_t s) {
    const uint64_t kept = off[nq];
    const size_t fb = ((size_t)nq + 1) * 8;
    HIP_TRY(ix->fi_ids.ensure(std::max<size_t>(kept * 4, 4)));
    HIP_TRY(ix->fi_off.ensure(fb));
    if (kept) HIP_TRY(hipMemcpyAsync(ix->fi_ids.p, ids32, kept * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ix->fi_off.p, off, fb, hipMemcpyHostToDevice, s));
    return WV_OK;
}

// chunks of a list for a grid of (ns queries, chunks): enough workgroups to
// fill the machine, at least 512 ids each; whole wave rounds (256 ids)
void ids_chunks(const wv_index* ix, int ns, uint64_t max_len, uint64_t* chunk_len, uint64_t* n_chunks) {
    uint64_t nc = std::max<uint64_t>(1, (2 * (uint64_t)ix->n_cus + ns - 1) / ns);
    nc = std::max<uint64_t>(1, std::min(nc, (max_len + 511) / 512));
    *chunk_len = std::max<uint64_t>(256, ((max_len + nc - 1) / nc + 255) / 256 * 256);
    *n_chunks = std::max<uint64_t>(1, (max_len + *chunk_len - 1) / *chunk_len);
}

// Switches of the list kernel on a compressed index, read per call.
// WV_FLAT_IDS_PQ_LUT=0|1: every workgroup evaluates rows directly / from the
// lookup table wherever it fits; unset: the table where the workgroup's chunk
// holds at least ks ids (as WV_SBD_PQ_LUT).
static int flat_ids_pq_lut() {
    const char* e = std::getenv("WV_FLAT_IDS_PQ_LUT");
    return e && *e ? (std::atoi(e) ? 1 : 0) : -1;
}
// ids_chunks cuts a long list into chunks as short as 256 ids when few queries
// are in flight, below the ks ids from which a workgroup builds the table.
// Where the table may be used, a chunk is at least 4 ks ids (whole wave
// rounds): a build costs what ks direct rows cost, so it is spread over four
// times that.  Measured against no floor, ks, 16 ks and the scan pass's
// 4 ks ds (profiles/flat_ids_pq/README.md): up to 1.8 x faster than no floor
// on long lists of small batches; slower only for 1-8 queries with lists of a
// few 4 ks on a 64 KiB table.  WV_FLAT_IDS_PQ_CHUNK=<ids> overrides the floor
// (0: none; A/B runs).
static void flat_ids_pq_chunk_floor(const wv::PqParams& pq, int lut, uint64_t max_len, uint64_t* chunk_len,
                                    uint64_t* n_chunks) {
    if (lut == 0 || (uint64_t)pq.m * pq.ks * 4 > (uint64_t)wv::SBD_PQ_LUT_BYTES_MAX) return;
    uint64_t floor = 4 * (uint64_t)pq.ks;
    if (const char* e = std::getenv("WV_FLAT_IDS_PQ_CHUNK")) floor = (uint64_t)std::max(0ll, std::atoll(e));
    floor = (floor + 255) / 256 * 256;
    if (*chunk_len >= floor) return;
    *chunk_len = floor;
    *n_chunks = std::max<uint64_t>(1, (max_len + floor - 1) / floor);
}
// A batch's results from the pinned staging copy to the caller's arrays: the
// counts, and of every row the first out_n[q] slots only.  The slots past a
// count stay as the caller left them: the device buffers behind the staging
// copy still hold earlier batches' results there (ids another batch's allow
// list admitted).
static void copy_results(const char* ids, const char* dists, const char* counts, int nq, int k, uint64_t* out_ids,
                         float* out_dists, int32_t* out_n) {
    std::memcpy(out_n, counts, (size_t)nq * 4);
    bool full = true;
    for (int q = 0; q < nq && full; ++q) full = out_n[q] == k;
    if (full) {
        std::memcpy(out_ids, ids, (size_t)nq * k * 8);
        std::memcpy(out_dists, dists, (size_t)nq * k * 4);
        return;
    }
    for (int q = 0; q < nq; ++q) {
        const size_t n = (size_t)std::min(std::max(out_n[q], 0), k), o = (size_t)q * k;
        std::memcpy(out_ids + o, ids + o * 8, n * 8);
        std::memcpy(out_dists + o, dists + o * 4, n * 4);
    }
}
}  // namespace wv_host

extern "C" {

int wv_search_batch(wv_index* ix, const float* queries, int nq, int k, int ef, const uint64_t* allow_bits,
                    uint64_t allow_nbits, uint64_t allow_stride_words, int mode, uint64_t* out_ids, float* out_dists,
                    int32_t* out_n) {
    if (check(ix) || nq < 0 || k <= 0 || (nq && (!queries || !out_ids || !out_dists || !out_n)))
        return fail(WV_EINVAL, "wv_search_batch: bad argument");
    if (nq == 0) return WV_OK;
    const uint64_t words = (allow_nbits + 63) / 64;
    const uint64_t arows = allow_bits ? (allow_stride_words ? (uint64_t)nq : 1) : 0;
    const uint64_t astride = allow_stride_words ? allow_stride_words : words;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * 4, ab = arows * astride * 8, ib = (size_t)nq * k * 8,
                 db = (size_t)nq * k * 4, nb = (size_t)nq * 4;
    const size_t o_a = al(qb), o_i = o_a + al(ab), o_d = o_i + al(ib), o_n = o_d + al(db), need = o_n + al(nb);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    SlotLease lease(ix);
    wv_index::HostSlot& sl = *lease.sl;
    if (int rc = slot_reserve(sl, need)) return rc;
    char* pin = static_cast<char*>(sl.pin);
    std::memcpy(pin, queries, qb);
    if (ab) std::memcpy(pin + o_a, allow_bits, ab);
    {
        std::lock_guard<std::mutex> g(ix->mu);
        HIP_TRY(hipSetDevice(ix->cfg.device));
        hipStream_t s = ix->stream;
        const float* dq = nullptr;
        int rc = stage_queries(ix, reinterpret_cast<const float*>(pin), nq, &dq, s);
        if (rc) return rc;
        const uint64_t* dallow = nullptr;
        if (ab) {
            // an AUTO batch with per-query allow lists gathers into g_allow:
            // keep the caller's bitmaps in their own buffer then
            DevBuf& dst = allow_stride_words && mode == WV_MODE_AUTO ? ix->allow_keep : ix->g_allow;
            HIP_TRY(dst.ensure(ab));
            HIP_TRY(hipMemcpyAsync(dst.p, pin + o_a, ab, hipMemcpyHostToDevice, s));
            dallow = dst.as<uint64_t>();
        }
        HIP_TRY(ix->out_ids.ensure(ib));
        HIP_TRY(ix->out_d.ensure(db));
        HIP_TRY(ix->out_n.ensure(nb));
        rc = search_core(ix, dq, nq, k, ef, dallow, allow_nbits, allow_stride_words, mode, ix->out_ids.as<uint64_t>(),
                         ix->out_d.as<float>(), ix->out_n.as<int32_t>(), s);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(pin + o_i, ix->out_ids.p, ib, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(pin + o_d, ix->out_d.p, db, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(pin + o_n, ix->out_n.p, nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(sl.done, s));
    }
    // the index is free for the next batch while this one finishes
    HIP_TRY(hipEventSynchronize(sl.done));
    copy_results(pin + o_i, pin + o_d, pin + o_n, nq, k, out_ids, out_dists, out_n);
    return WV_OK;
}

// wv_search_batch with one allow list per query, as ids.  The flat-versus-HNSW
// rule of search.go:64-79 is applied on the host from each list's length; a
// flat query whose list is short goes to the sparse kernel (wv_flat_ids.hip;
// on a compressed index its PQ variant, where wv_index_set_pq_list_search is
// on), every other query to search_core over bitmap rows scattered on the device.
int wv_search_batch_ids(wv_index* ix, const float* queries, int nq, int k, int ef, const uint64_t* allow_ids,
                        const uint64_t* allow_offsets, int mode, uint64_t* out_ids, float* out_dists, int32_t* out_n) {
    if (nq < 0) return fail(WV_EINVAL, "wv_search_batch_ids: nq < 0");
    if (k <= 0) return fail(WV_EINVAL, "wv_search_batch_ids: k <= 0");
    if (!allow_offsets) return fail(WV_EINVAL, "wv_search_batch_ids: null allow_offsets");
    if (check(ix)) return fail(WV_EINVAL, "wv_search_batch_ids: null index");
    if (nq && (!queries || !out_ids || !out_dists || !out_n))
        return fail(WV_EINVAL, "wv_search_batch_ids: null queries or outputs");
    if (int rc = ids_check_offsets("wv_search_batch_ids", allow_ids, allow_offsets, nq)) return rc;
    const uint64_t total = allow_offsets[nq];
    if (nq == 0) return WV_OK;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * 4, lb = (size_t)total * 4, fb = ((size_t)nq + 1) * 8,
                 ib = (size_t)nq * k * 8, db = (size_t)nq * k * 4, nb = (size_t)nq * 4;
    const size_t o_l = al(qb), o_f = o_l + al(lb), o_i = o_f + al(fb), o_d = o_i + al(ib), o_n = o_d + al(db),
                 need = o_n + al(nb);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    SlotLease lease(ix);
    wv_index::HostSlot& sl = *lease.sl;
    if (int rc = slot_reserve(sl, need)) return rc;
    char* pin = static_cast<char*>(sl.pin);
    std::memcpy(pin, queries, qb);
    uint32_t* ids32 = reinterpret_cast<uint32_t*>(pin + o_l);
    uint64_t* off = reinterpret_cast<uint64_t*>(pin + o_f);
    if (int rc = ids_stage("wv_search_batch_ids", allow_ids, allow_offsets, nq, ids32, off)) return rc;
    {
        std::lock_guard<std::mutex> g(ix->mu);
        HIP_TRY(hipSetDevice(ix->cfg.device));
        hipStream_t s = ix->stream;
        const float* dq = nullptr;
        int rc = stage_queries(ix, reinterpret_cast<const float*>(pin), nq, &dq, s);
        if (rc) return rc;
        rc = ids_upload(ix, ids32, off, nq, s);
        if (rc) return rc;
        HIP_TRY(ix->out_ids.ensure(ib));
        HIP_TRY(ix->out_d.ensure(db));
        HIP_TRY(ix->out_n.ensure(nb));
        rc = refresh_bitmaps(ix);
        if (rc) return rc;
        // the route of every query, from its list's length
        const uint64_t N = ix->n_rows;
        const int ef_eff = ef <= 0 ? search_time_ef(ix->cfg, k) : ef;
        const bool can_hnsw = ix->has_graph && ef_eff <= wv::HNSW_EF_MAX;
        // (compressed: the list kernel over the codes, where the index asks
        // for it -- its query row stays in memory, so any dimension)
        const bool sparse_ok = k <= wv::BF_WIDE_KMAX &&
                               (ix->pq_on ? ix->pq_list_search : ix->dpad <= wv::FLAT_IDS_DPAD_MAX);
        std::vector<int32_t> sel[3];   // sparse, bitmap rows searched flat, bitmap rows searched by HNSW
        uint64_t sp_ids = 0, sp_max = 0;
        for (int q = 0; q < nq; ++q) {
            const uint64_t L = allow_offsets[q + 1] - allow_offsets[q];
            bool flat;
            if (mode == WV_MODE_EXACT) flat = true;
            else if (mode == WV_MODE_HNSW) flat = false;
            else flat = !can_hnsw || (!ix->cfg.forbid_flat && (int64_t)L < ix->cfg.flat_search_cutoff);
            // (EXACT: the 1/8 rule of run_exact's compacted scans)
            const bool sparse = flat && sparse_ok && (mode != WV_MODE_EXACT || 8 * L < N);
            sel[sparse ? 0 : flat ? 1 : 2].push_back(q);
            if (sparse) {
                sp_ids += L;
                sp_max = std::max(sp_max, off[q + 1] - off[q]);
            }
        }
        std::vector<int32_t> order;
        for (auto& v : sel) order.insert(order.end(), v.begin(), v.end());
        HIP_TRY(ix->fi_sel.ensure(nb));
        HIP_TRY(hipMemcpyAsync(ix->fi_sel.p, order.data(), nb, hipMemcpyHostToDevice, s));
        ix->fi_sparse_q = sel[0].size();
        ix->fi_sparse_ids = sp_ids;
        ix->fi_bitmap_q = sel[1].size() + sel[2].size();
        ix->fi_timed = false;
        if (!sel[0].empty()) {
            const int ns = (int)sel[0].size();
            uint64_t chunk_len = 0, nc = 0;
            ids_chunks(ix, ns, sp_max, &chunk_len, &nc);
            wv::PqParams pq{};
            int lut = -1;
            if (ix->pq_on) {
                pq = pq_params(ix);
                lut = flat_ids_pq_lut();
                flat_ids_pq_chunk_floor(pq, lut, sp_max, &chunk_len, &nc);
            }
            if (nc > 1) HIP_TRY(ix->fi_part.ensure((size_t)ns * nc * k * 8));
            // what both list kernels read: the lists, the selection, the outputs
            auto fill = [&](auto& fp) {
                fp.Q = dq;
                fp.excl = ix->excl.as<uint64_t>();
                fp.excl_nbits = ix->capacity;
                fp.ids = ix->fi_ids.as<uint32_t>();
                fp.off = ix->fi_off.as<uint64_t>();
                fp.sel = ix->fi_sel.as<int32_t>();
                fp.n_rows = N;
                fp.id_base = ix->cfg.id_base;
                fp.chunk_len = chunk_len;
                fp.ns = ns;
                fp.n_chunks = (int)nc;
                if (nc > 1) fp.part = ix->fi_part.as<unsigned long long>();
                fp.dpad = ix->dpad;
                fp.metric = ix->metric;
                fp.k = k;
                fp.out_ids = ix->out_ids.as<uint64_t>();
                fp.out_d = ix->out_d.as<float>();
                fp.out_n = ix->out_n.as<int32_t>();
            };
            if (ix->timing) {
                for (auto& e : ix->fi_ev)
                    if (!e) HIP_TRY(hipEventCreate(&e));
                HIP_TRY(hipEventRecord(ix->fi_ev[0], s));
            }
            if (ix->pq_on) {
                wv::FlatIdsPqParams fp{};
                fill(fp);
                fp.pq = pq;
                fp.lut = lut;
                HIP_TRY(wv_launch_flat_ids_pq(&fp, s));
            } else {
                wv::FlatIdsParams fp{};
                fill(fp);
                fp.X = ix->vecs.as<float>();
                fp.D = ix->dim;
                fp.ldx = ix->ldx;
                HIP_TRY(wv_launch_flat_ids(&fp, s));
            }
            if (ix->timing) {
                HIP_TRY(hipEventRecord(ix->fi_ev[1], s));
                ix->fi_timed = true;
            }
        }
        // the bitmap route: rows scattered from the ids into bounded scratch,
        // then today's kernels (search_core) and each row back to its query
        const uint64_t words = std::max<uint64_t>(1, (N + 63) / 64);
        const size_t rows_cap = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(65535, (1ull << 30) / (words * 8)));
        size_t base = sel[0].size();
        for (int grp = 1; grp <= 2; ++grp) {
            const std::vector<int32_t>& v = sel[grp];
            for (size_t c0 = 0; c0 < v.size(); c0 += rows_cap) {
                const int n = (int)std::min(rows_cap, v.size() - c0);
                const int32_t* d_sel = ix->fi_sel.as<int32_t>() + base + c0;
                uint64_t max_len = 0;
                for (int i = 0; i < n; ++i) max_len = std::max(max_len, off[v[c0 + i] + 1] - off[v[c0 + i]]);
                HIP_TRY(ix->fi_q.ensure((size_t)n * ix->dpad * 4));
                HIP_TRY(ix->fi_bits.ensure((size_t)n * words * 8));
                HIP_TRY(ix->fi_oid.ensure((size_t)n * k * 8));
                HIP_TRY(ix->fi_od.ensure((size_t)n * k * 4));
                HIP_TRY(ix->fi_on.ensure((size_t)n * 4));
                HIP_TRY(launch_gather_rows(dq, ix->dpad, d_sel, n, ix->dpad, ix->fi_q.as<float>(), ix->dpad, s));
                HIP_TRY(hipMemsetAsync(ix->fi_bits.p, 0, (size_t)n * words * 8, s));
                HIP_TRY(wv_launch_ids_to_bits(ix->fi_ids.as<uint32_t>(), ix->fi_off.as<uint64_t>(), d_sel, n, max_len, N,
                                              words, ix->fi_bits.as<uint64_t>(), s));
                rc = search_core(ix, ix->fi_q.as<float>(), n, k, ef, ix->fi_bits.as<uint64_t>(), std::max<uint64_t>(N, 1),
                                 words, grp == 1 ? WV_MODE_EXACT : WV_MODE_HNSW, ix->fi_oid.as<uint64_t>(),
                                 ix->fi_od.as<float>(), ix->fi_on.as<int32_t>(), s);
                if (rc) return rc;
                hipLaunchKernelGGL(scatter_results_kernel, dim3(n), dim3(64), 0, s, ix->fi_oid.as<uint64_t>(),
                                   ix->fi_od.as<float>(), ix->fi_on.as<int32_t>(), d_sel, n, k,
                                   ix->out_ids.as<uint64_t>(), ix->out_d.as<float>(), ix->out_n.as<int32_t>());
                HIP_TRY(hipGetLastError());
            }
            base += v.size();
        }
        HIP_TRY(hipMemcpyAsync(pin + o_i, ix->out_ids.p, ib, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(pin + o_d, ix->out_d.p, db, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(pin + o_n, ix->out_n.p, nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(sl.done, s));
    }
    HIP_TRY(hipEventSynchronize(sl.done));
    copy_results(pin + o_i, pin + o_d, pin + o_n, nq, k, out_ids, out_dists, out_n);
    return WV_OK;
}

int wv_last_sparse_stats(wv_index* ix, uint64_t* sparse_queries, uint64_t* sparse_ids, uint64_t* bitmap_queries) {
    if (check(ix)) return fail(WV_EINVAL, "wv_last_sparse_stats: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    if (sparse_queries) *sparse_queries = ix->fi_sparse_q;
    if (sparse_ids) *sparse_ids = ix->fi_sparse_ids;
    if (bitmap_queries) *bitmap_queries = ix->fi_bitmap_q;
    return WV_OK;
}

int wv_last_sparse_time(wv_index* ix, float* kernel_ms) {
    if (check(ix) || !kernel_ms) return fail(WV_EINVAL, "wv_last_sparse_time: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    *kernel_ms = 0.f;
    if (!ix->fi_timed) return WV_OK;
    HIP_TRY(hipEventSynchronize(ix->fi_ev[1]));
    HIP_TRY(hipEventElapsedTime(kernel_ms, ix->fi_ev[0], ix->fi_ev[1]));
    return WV_OK;
}

int wv_search_batch_device(wv_index* ix, const float* d_queries, int nq, int k, int ef, const uint64_t* d_allow_bits,
                           uint64_t allow_nbits, uint64_t allow_stride_words, int mode, uint64_t* d_out_ids,
                           float* d_out_dists, int32_t* d_out_n, void* stream) {
    if (check(ix) || nq < 0 || k <= 0 || (nq && (!d_queries || !d_out_ids || !d_out_dists || !d_out_n)))
        return fail(WV_EINVAL, "wv_search_batch_device: bad argument");
    if (nq == 0) return WV_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : ix->stream;
    const bool foreign = s != ix->stream;
    if (foreign) {
        if (!ix->ev_in) {
            HIP_TRY(hipEventCreateWithFlags(&ix->ev_in, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&ix->ev_out, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(ix->ev_in, ix->stream));
        HIP_TRY(hipStreamWaitEvent(s, ix->ev_in, 0));
    } else {
        // NULL: the index's own (non-blocking) stream, which would not wait
        // for work the caller queued on the legacy default stream -- e.g. a
        // torch kernel that just wrote d_queries: order after it explicitly
        if (!ix->ev_null) HIP_TRY(hipEventCreateWithFlags(&ix->ev_null, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ix->ev_null, nullptr));
        HIP_TRY(hipStreamWaitEvent(s, ix->ev_null, 0));
    }
    const float* dq = d_queries;
    int rc = WV_OK;
    if (ix->metric == WV_COSINE_DOT) {
        // the caller's rows are [nq][dpad]; normalize a padded copy
        HIP_TRY(ix->q_norm.ensure((size_t)nq * ix->dpad * 4));
        HIP_TRY(launch_pad_rows(d_queries, ix->dpad, nq, ix->dim, ix->q_norm.as<float>(), ix->dpad, s));
        HIP_TRY(wv_launch_normalize(ix->q_norm.as<float>(), ix->q_norm.as<float>(), nq, ix->dim, ix->dpad, s));
        dq = ix->q_norm.as<float>();
    }
    rc = search_core(ix, dq, nq, k, ef, d_allow_bits, allow_nbits, allow_stride_words, mode, d_out_ids, d_out_dists,
                     d_out_n, s);
    if (foreign) {
        HIP_TRY(hipEventRecord(ix->ev_out, s));
        HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ev_out, 0));
    }
    return rc;
}

int wv_index_query_ld(const wv_index* ix) { return ix ? ix->dpad : -1; }

int wv_index_synchronize(wv_index* ix) {
    if (check(ix)) return fail(WV_EINVAL, "wv_index_synchronize: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return WV_OK;
}

int wv_search_by_vector(wv_index* ix, const float* vector, int k, const uint64_t* allow_bits, uint64_t allow_nbits,
                        uint64_t* out_ids, float* out_dists, int32_t* out_n) {
    return wv_search_batch(ix, vector, 1, k, 0, allow_bits, allow_nbits, 0, WV_MODE_AUTO, out_ids, out_dists, out_n);
}

}  // extern "C"
