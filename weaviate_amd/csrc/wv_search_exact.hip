// wv_search_exact.hip -- flatSearch on the device: the key passes of wv_bf.hip
// and wv_h16.hip with allow-list compaction and the device-resolved fallback,
// the scan over PQ codes (wv_pq.hip), and the per-query full scan and sort.
#include <hipcub/hipcub.hpp>

#include "wv_search.h"

using namespace wv_host;

// hipcub's two-call pattern over ix->sort_tmp: the size query, the scratch,
// the run.  A macro, so that a failure's message still names the hipcub call
// (HIP_TRY prints its expression).
#define CUB_TRY(ix, fn, ...)                                    \
    do {                                                        \
        size_t tmp = 0;                                         \
        HIP_TRY(fn(nullptr, tmp, __VA_ARGS__));                 \
        HIP_TRY((ix)->sort_tmp.ensure(tmp));                    \
        HIP_TRY(fn((ix)->sort_tmp.p, tmp, __VA_ARGS__));        \
    } while (0)

namespace {

// nothing to search: every query's count is 0
int no_rows(const Batch& b) {
    if (b.nq) HIP_TRY(b.zero_counts());
    return WV_OK;
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

// Exact scan + stable radix sort, one query at a time (large k and certificate
// fallbacks).  b: one query, its allow row shared (Batch::one).
int exact_full(wv_index* ix, const Batch& b) {
    const uint64_t N = ix->n_rows;
    hipStream_t s = b.s;
    if (N == 0) return no_rows(b);
    HIP_TRY(ix->scan_d.ensure(N * 4));
    HIP_TRY(ix->scan_i.ensure(N * 4));
    HIP_TRY(ix->sort_d.ensure(N * 4));
    HIP_TRY(ix->sort_i.ensure(N * 4));
    wv::ScanParams sp{};
    sp.X = ix->vecs.as<float>();
    sp.q = b.q;
    sp.tomb = ix->excl.as<uint64_t>();
    sp.tomb_nbits = ix->capacity;
    sp.allow = b.allow;
    sp.allow_nbits = b.allow_nbits;
    sp.N = N;
    sp.D = ix->dim;
    sp.ldx = ix->ldx;
    sp.metric = ix->metric;
    sp.dist = ix->scan_d.as<float>();
    sp.ids = ix->scan_i.as<uint32_t>();
    HIP_TRY(wv_launch_exact_scan(&sp, s));
    CUB_TRY(ix, hipcub::DeviceRadixSort::SortPairs, ix->scan_d.as<float>(), ix->sort_d.as<float>(),
            ix->scan_i.as<uint32_t>(), ix->sort_i.as<uint32_t>(), (int)N, 0, 32, s);
    hipLaunchKernelGGL(copy_topk_kernel, dim3(1), dim3(256), 0, s, ix->sort_d.as<float>(), ix->sort_i.as<uint32_t>(),
                       N, b.k, ix->cfg.id_base, b.out_ids, b.out_d, b.out_n);
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
static int count_allowed(wv_index* ix, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N, hipStream_t s) {
    const uint64_t words = (N + 63) / 64, allow_words = (allow_nbits + 63) / 64;
    HIP_TRY(ix->ac_cnt.ensure((words + 1) * 4));
    HIP_TRY(ix->ac_off.ensure((words + 1) * 4));
    hipLaunchKernelGGL(allowed_count_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_allow,
                       allow_words, ix->excl.as<uint64_t>(), N, ix->ac_cnt.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(ix->ac_cnt.as<uint32_t>() + words, 0, 4, s));
    CUB_TRY(ix, hipcub::DeviceScan::ExclusiveSum, ix->ac_cnt.as<uint32_t>(), ix->ac_off.as<uint32_t>(),
            (int)(words + 1), s);
    return WV_OK;
}

// ... and the rows written at those offsets into ix->rowidx
static int scatter_allowed(wv_index* ix, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N, hipStream_t s) {
    const uint64_t words = (N + 63) / 64;
    hipLaunchKernelGGL(allowed_scatter_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_allow,
                       (allow_nbits + 63) / 64, ix->excl.as<uint64_t>(), N, ix->ac_off.as<uint32_t>(),
                       ix->rowidx.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    return WV_OK;
}

int compact_allowed(wv_index* ix, const uint64_t* d_allow, uint64_t allow_nbits, uint64_t N, uint64_t* n_ok,
                    hipStream_t s, bool always = false, int nq = 1) {
    const uint64_t words = (N + 63) / 64;
    if (int rc = count_allowed(ix, d_allow, allow_nbits, N, s)) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, ix->ac_off.as<uint32_t>() + words, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_ok = total;
    // (the row list also serves the fp32 pass, which compacts below 1/2)
    if (total == 0 || (!worth_compacting(total, N, nq) && 2 * (uint64_t)total >= N && !always)) return WV_OK;
    // (whole 256-row tiles: the wide-D pass reads the list per tile)
    const uint64_t padded = (total + wv::HW_BN - 1) / wv::HW_BN * wv::HW_BN;
    HIP_TRY(ix->rowidx.ensure(padded * 4));
    if (int rc = scatter_allowed(ix, d_allow, allow_nbits, N, s)) return rc;
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
    if (int rc = count_allowed(ix, d_allow, allow_nbits, N, s)) return rc;
    const uint64_t padded = (N + wv::HW_BN - 1) / wv::HW_BN * wv::HW_BN;
    HIP_TRY(ix->rowidx.ensure(padded * 4));
    if (int rc = scatter_allowed(ix, d_allow, allow_nbits, N, s)) return rc;
    *n_dev = ix->ac_off.as<uint32_t>() + (N + 63) / 64;
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
int run_pq_flat(wv_index* ix, const Batch& b, const uint64_t* d_rowmask, uint64_t rowmask_nbits) {
    const uint64_t N = ix->n_rows;
    const int nq = b.nq;
    hipStream_t s = b.s;
    if (N == 0 || nq == 0) return no_rows(b);
    const bool shared = b.allow && !b.allow_stride;
    const uint64_t* cmask = shared ? b.allow : d_rowmask;
    const uint64_t cbits = shared ? b.allow_nbits : rowmask_nbits;
    uint64_t nr = N;
    const uint32_t* rows = nullptr;
    if (cmask) {
        int rc = compact_allowed(ix, cmask, cbits, N, &nr, s, true);
        if (rc) return rc;
        if (nr == 0) return no_rows(b);
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
    sp.Q = b.q;
    sp.rows = rows;
    sp.excl = ix->excl.as<uint64_t>();
    sp.excl_nbits = ix->capacity;
    sp.allow = b.allow_stride ? b.allow : nullptr;   // a shared list is compacted already
    sp.allow_nbits = b.allow_nbits;
    sp.allow_stride = b.allow_stride;
    sp.nr = nr;
    sp.ldq = b.ldq;
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
        CUB_TRY(ix, hipcub::DeviceSegmentedRadixSort::SortPairs, ix->pk_key.as<float>(), ix->pk_skey.as<float>(),
                ix->pk_val.as<uint32_t>(), ix->pk_sval.as<uint32_t>(), n_items, nqc, ix->pk_off.as<int32_t>(),
                ix->pk_off.as<int32_t>() + 1, 0, 32, s);
        HIP_TRY(wv_launch_pq_topk(ix->pk_skey.as<float>(), ix->pk_sval.as<uint32_t>(), ix->pk_dist.as<float>(), rows,
                                  nr, q0, nqc, b.k, ix->cfg.id_base, b.out_ids, b.out_d, b.out_n, s));
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

// what every finalize reads of the index and the batch (the ix buffers ensured
// by the caller); the key pass's lists and schedule are the caller's to set
wv::BfFinParams fin_params(const wv_index* ix, const Batch& b) {
    wv::BfFinParams fp{};
    fp.X = ix->vecs.as<float>();
    fp.Q = b.q;
    fp.qnorm = ix->q_nrm2.as<float>();
    fp.xnorm_max = ix->maxnorm_host;   // cached at every row write
    fp.nq = b.nq;
    fp.D = ix->dim;
    fp.ldx = ix->ldx;
    fp.ldq = b.ldq;
    fp.metric = ix->metric;
    fp.k = b.k;
    fp.id_base = ix->cfg.id_base;
    fp.out_ids = b.out_ids;
    fp.out_d = b.out_d;
    fp.out_n = b.out_n;
    fp.fail = ix->fail.as<int32_t>();
    fp.fail_thr = ix->fail_thr.as<float>();
    return fp;
}

// f16 key pass (wv_h16.hip) over the whole corpus, optionally masked by a
// shared allow list: query image + scale, an optional seed pre-pass over every
// H_SAMPLE-th tile (its finalize yields per-query thresholds), the main pass
// seeded with them, and the certifying finalize, which flags uncertified
// queries in ix->fail for the device-resolved fallback (queue_fbd).
// rowidx (nullable): the ascending row list of a compacted shared allow list
// (compact_allowed) -- the pass then runs over an f16 image of just those N
// rows (gathered here) and the candidate ids are mapped back to rows before
// the finalize; the batch's (shared) allow list is then already applied.
// Ends by queueing the fallback for the queries the finalize flagged.
int run_h16(wv_index* ix, const Batch& b, uint64_t N, const uint32_t* rowidx = nullptr,
            const uint32_t* n_dev = nullptr) {
    const float* d_q = b.q;
    const int nq = b.nq, k = b.k;
    const uint64_t* d_allow = rowidx ? nullptr : b.allow;
    const uint64_t allow_nbits = b.allow_nbits;
    hipStream_t s = b.s;
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
    wv::BfFinParams fp = fin_params(ix, b);
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
    const bool xs_on = env_int("WV_H16_XSLOT", 1) != 0;
    auto xs_fits = [&](const wv::BfSchedule& sc) { return xs_on && !wd && 2 * sc.n_slots <= 32 && k <= 2 * sc.n_slots; };
    // The seed's tile stride (WV_H16_SAMPLE: for measurements).  Where the
    // main pass will run the cross-slot exchange, its bounds overtake the
    // seed's within the first eighth of a segment, so a sparser seed costs
    // fewer insertion events than its pre-pass saves (H_SAMPLE_XS; the main
    // pass's schedule does not depend on the stride).
    int sample = wv::H_SAMPLE;
    if (!wd && !n_dev && xs_fits(wv::bf_schedule(nq, N, target(ntl), bq, tile_rows))) sample = wv::H_SAMPLE_XS;
    if (const int v = env_int("WV_H16_SAMPLE", 0, 1)) sample = v;
    // (seeded from H_SEED_MIN_TILES tiles on, whatever the stride)
    const bool seed = !wd && ntl >= (uint64_t)wv::H_SEED_MIN_TILES && !env_on("WV_H16_NO_SEED");
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
    hp.kth = k <= (wd ? 2 * kp : prod * kp) && !seed && !env_on("WV_H16_NO_RUNNING")
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
    return queue_fbd(ix, b);
}

}  // namespace

namespace wv_host {

// Queue the device-resolved fallback for the queries whose flag in ix->fail
// is set (threshold ix->fail_thr): no host round trip (wv_bf.hip, fbd kernels).
int queue_fbd(wv_index* ix, const Batch& b) {
    const uint64_t N = ix->n_rows;
    const int nq = b.nq;
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
    bp.Q = b.q;
    bp.qidx = ix->fbd_list.as<int32_t>();
    bp.thr = ix->fail_thr.as<float>();
    bp.tomb = ix->excl.as<uint64_t>();
    bp.tomb_nbits = ix->capacity;
    bp.allow = b.allow;
    bp.allow_nbits = b.allow_nbits;
    bp.allow_stride = b.allow_stride;
    bp.N = N;
    bp.nf = nq;
    bp.D = ix->dim;
    bp.ldx = ix->ldx;
    bp.ldq = b.ldq;
    bp.metric = ix->metric;
    bp.k = b.k;
    bp.id_base = ix->cfg.id_base;
    bp.cand_d = ix->fbd_cd.as<float>();
    bp.cand_id = ix->fbd_ci.as<uint32_t>();
    bp.cand_n = ix->fbd_cn.as<uint32_t>();
    bp.out_ids = b.out_ids;
    bp.out_d = b.out_d;
    bp.out_n = b.out_n;
    bp.overflow = ix->fbd_over.as<int32_t>();
    bp.d_nf = ix->fbd_nf.as<int32_t>();
    bp.scratch = ix->fbd_scr.as<float>();
    bp.n_scr = wv::FBD_SCR;
    bp.fb_total = ix->stat_acc.as<unsigned long long>() + 2;
#ifdef WV_ABLATION_BUILD
    if (env_on("WV_ABLATE_NO_FALLBACK")) return WV_OK;   // kernel ablations only (tools/h16_ablate.sh)
#endif
    HIP_TRY(wv_launch_fbd(ix->fail.as<int32_t>(), nq, &bp, b.s));
    return WV_OK;
}

// Brute force (flatSearch semantics) over a device batch of prepared queries.
// d_rowmask (nullable, with per-query allow lists only): a shared bitmap that
// contains every row any query may return (the delta set of wv_index_add);
// its rows are compacted and each query's own list is tested per row.
int run_exact(wv_index* ix, const Batch& b, const uint64_t* d_rowmask, uint64_t rowmask_nbits) {
    if (ix->pq_on)   // flatSearch on a compressed index ranks by PQ distance (index.go:493-511)
        return run_pq_flat(ix, b, d_rowmask, rowmask_nbits);
    const uint64_t N = ix->n_rows;
    const float* d_q = b.q;
    const int nq = b.nq, k = b.k;
    const uint64_t* d_allow = b.allow;
    const uint64_t allow_nbits = b.allow_nbits, allow_stride = b.allow_stride;
    hipStream_t s = b.s;
    if (N == 0 || nq == 0) return no_rows(b);
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
        const bool no_compact = env_on("WV_BF_NO_COMPACT");
        if (cmask && !d_rowmask && h16_ok && ix->h16_wide && k <= wv::FIN_KF && !env_on("WV_BF_SYNC_COMPACT") &&
            !no_compact) {
            const uint32_t* n_dev = nullptr;
            const uint64_t n_bound = std::min<uint64_t>(N, cbits);
            if (n_bound == 0) return no_rows(b);
            if (int rc = compact_allowed_dev(ix, cmask, cbits, N, &n_dev, s)) return rc;
            return run_h16(ix, b, n_bound, ix->rowidx.as<uint32_t>(), n_dev);
        }
        if (cmask) {
            uint64_t n_ok = 0;
            int rc = compact_allowed(ix, cmask, cbits, N, &n_ok, s, d_rowmask != nullptr, nq);
            if (rc) return rc;
            if (n_ok == 0) return no_rows(b);
            // a list worth compacting (worth_compacting): the scan runs over
            // its rows -- on the f16 pass over their gathered image (h16_ok),
            // else (below 1/2 or 1/8) on the fp32 pass over the row list
            const bool compact = (worth_compacting(n_ok, N, nq) && !no_compact) || d_rowmask;
            if (compact && h16_ok) return run_h16(ix, b, n_ok, ix->rowidx.as<uint32_t>());
            // (no gathered f16 pass: the f16 pass masks the whole corpus
            // unless the list keeps under 1/8 of it)
            const uint64_t frac = ix->use_h16 && !allow_stride ? 8 : 2;
            if (((frac * n_ok < N && !no_compact) || d_rowmask) && k <= wv::BF_FAST_KMAX) {
                n_scan = n_ok;
                d_rowidx = ix->rowidx.as<uint32_t>();
            }
        }
        if (ix->use_h16 && !d_rowidx && !allow_stride) return run_h16(ix, b, N);   // (masked by the shared list, if any)
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
        HIP_TRY(ix->fail_thr.ensure((size_t)nq * 4));
        wv::BfFinParams fp = fin_params(ix, b);
        fp.cand_d = ix->cand_d.as<float>();
        fp.cand_id = ix->cand_id.as<uint32_t>();
        fp.n_slots = sch.n_slots;
        fp.ntiles = sch.ntiles;
        fp.units_per_block = sch.units_per_block;
        fp.split = bp.split;
        fp.bq = bq;
        fp.prod = prod;
        TREC(2);
        HIP_TRY(wv_launch_bf_finalize(&fp, s));
        TREC(3);
        return queue_fbd(ix, b);
    }
    // k past every key pass: each query by a full scan and sort
    return exact_each(ix, b, nullptr);
}

int exact_each(wv_index* ix, const Batch& b, const int32_t* pick) {
    if (!pick) ix->last_fallbacks += (uint64_t)b.nq;
    for (int q = 0; q < b.nq; ++q) {
        if (pick && !pick[q]) continue;
        if (pick) ix->last_fallbacks++;
        const Batch one = b.one(q);
        int rc = ix->pq_on ? run_pq_flat(ix, one, nullptr, 0) : exact_full(ix, one);
        if (rc) return rc;
    }
    return WV_OK;
}

}  // namespace wv_host
