// wv_search_bigk.hip -- flatSearch for k past every key pass, batched: the
// large-k route (wv_index_set_large_k) in place of a scan and a sort per query.
//
// Per chunk of queries, all on the batch's stream: the bound pass
// (wv_bigk.hip; wv_bigk_kinds.hip on a compressed, manhattan or hamming index)
// writes each query's tau into the targets of the distance search's threshold
// pass; that pass (the index kind's own -- over the codes, or the tiled
// manhattan / hamming kernel's epilogue -- else the f16 filter where the index
// runs it, else the scan) lists every eligible row within tau; the segmented sort
// orders the lists by (dist, id); the emit kernel writes the first k of every
// list that is whole and holds k rows within tau, and flags the other queries.
// One sync per chunk reads the flags, and exact_each answers the flagged
// queries.  The answers are exact_each's bits either way: on a compressed
// index the PQ distance ranks, as in run_pq_flat, which is also what answers a
// flagged query there.
//
// Which k come here (run_exact): past the key passes on an uncompressed l2,
// dot or cosine index; past L1_KMAX on a manhattan or hamming one; on a
// compressed index every k past BF_FAST_KMAX that the fused scan does not
// serve -- k > 256 with wv_index_set_pq_scan on, k > 32 with it off, the edge
// uncompressed per-query bitmaps have, since the alternative is the same
// nq x N sort at every such k.
//
// A chunk holds at most WV_BIGK_MAX_ENTRIES (2^26, read per call) list entries
// at WV_SBD_CAP each, which also keeps the sort's int offsets in range.
#include <cmath>
#include <cstdlib>

#include "wv_pq_lut.h"
#include "wv_search.h"

namespace wv_host {

// k up to BIGK_KMAX (less for the smallest batches, which the per-query route
// answers sooner), the distance search's buffers free, and what the index
// kind's passes ask: uncompressed l2 / dot / cosine rows that the scan's query
// buffer holds; codes the PQ kernels read (pq_ok; any dimension: the table or
// direct rule is the kernels'); manhattan and hamming rows that the bound
// pass's LDS query holds and the tiled kernel counts
bool bigk_ok(const wv_index* ix, const Batch& b) {
    // (the small-batch cut-offs per index kind: wv_params.h)
    const int kmax = ix->pq_on                  ? wv::BIGK_KMAX
                     : b.nq == 1               ? (ix->metric == WV_HAMMING ? wv::BIGK_ONE_QUERY_KMAX_HAMMING : wv::BIGK_ONE_QUERY_KMAX)
                     : b.nq <= wv::BIGK_FEW_NQ ? wv::BIGK_FEW_QUERIES_KMAX
                                               : wv::BIGK_KMAX;
    const bool kind_ok = ix->pq_on                   ? wv::pq_ok(pq_params(ix))
                         : metric_is_l1(ix->metric) ? ix->dpad <= wv::FLAT_IDS_DPAD_MAX && ix->n_rows < (1ull << 31)
                                                    : ix->dpad <= 1024;
    return ix->large_k && kind_ok && b.k <= kmax && b.ldq == ix->dpad && !ix->sbd_busy && ix->n_rows < (1ull << 32);
}

int run_bigk(wv_index* ix, const Batch& b) {
    const uint64_t N = ix->n_rows;
    const int nq = b.nq, k = b.k;
    hipStream_t s = b.s;
    const int cap = sbd_cap();
    uint64_t max_entries = 1ull << 26;   // (64-bit: its own parse)
    if (const char* e = std::getenv("WV_BIGK_MAX_ENTRIES")) max_entries = std::strtoull(e, nullptr, 10);
    max_entries = std::min<uint64_t>(std::max<uint64_t>(max_entries, 1), 0x7FFFFFFFull);
    const int qc = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)nq, max_entries / (uint64_t)cap));
    const bool own_pass = sbd_kind_has_pass(ix);     // compressed, manhattan, hamming
    const bool keyed = !own_pass && sbd_h16_ok(ix);   // the f16 filter in place of the scan
    const int ccap = keyed ? sbd_h16_cand(cap) : 0;

    wv::BigkParams kp{};
    kp.X = ix->vecs.as<float>();
    kp.excl = ix->excl.as<uint64_t>();
    kp.excl_nbits = ix->capacity;
    kp.allow_nbits = b.allow_nbits;
    kp.allow_stride = b.allow_stride;
    kp.N = N;
    kp.D = ix->dim;
    kp.ldx = ix->ldx;
    kp.dpad = ix->dpad;
    kp.metric = ix->metric;
    kp.k = k;
    kp.step = (uint32_t)std::max(1, k / wv::BIGK_SAMPLE);
    kp.n_samples = (N + kp.step - 1) / kp.step;
    // segments as the scan's rows per workgroup: ~4 workgroups per CU over the
    // chunk, whole 4-wave steps, at least BIGK_SEG_MIN samples each
    const uint64_t target = std::max<uint64_t>(1, (uint64_t)ix->n_cus * 4 / (uint64_t)qc);
    kp.samples_per_seg = std::max<uint64_t>(wv::BIGK_SEG_MIN, (kp.n_samples + target - 1) / target);
    // over codes: a segment that builds the query's table holds the samples
    // that pay for it, the threshold pass's floor (sbd_kind_pass)
    wv::BigkPqParams kq{};
    if (ix->pq_on) {
        kq.pq = pq_params(ix);
        kq.lut = sbd_pq_lut();
        if (kq.lut != 0 && (uint64_t)kq.pq.m * kq.pq.ks * 4 <= (uint64_t)wv::SBD_PQ_LUT_BYTES_MAX)
            kp.samples_per_seg = std::max<uint64_t>(kp.samples_per_seg, 4 * (uint64_t)kq.pq.ks * (uint64_t)kq.pq.ds);
    }
    kp.samples_per_seg = (kp.samples_per_seg + 255) / 256 * 256;
    kp.n_seg = (int)((kp.n_samples + kp.samples_per_seg - 1) / kp.samples_per_seg);
    kp.cap = cap;
    kp.ccap = ccap;
    kp.id_base = ix->cfg.id_base;

    HIP_TRY(ix->sbd_q.ensure((size_t)qc * ix->dpad * 4));
    HIP_TRY(ix->sbd_t.ensure((size_t)qc * 4));
    HIP_TRY(ix->sbd_keys.ensure((size_t)qc * cap * 8));
    HIP_TRY(ix->sbd_tmp.ensure((size_t)qc * cap * 8));
    HIP_TRY(ix->sbd_cnt.ensure((size_t)qc * 12));
    HIP_TRY(ix->sbd_off.ensure((size_t)qc * 8));
    HIP_TRY(ix->bigk_seg.ensure((size_t)qc * kp.n_seg * 64 * 4));
    HIP_TRY(ix->bigk_flag.ensure((size_t)qc * 4));
    std::vector<int32_t> flags((size_t)qc);
    for (int q0 = 0; q0 < nq; q0 += qc) {
        const Batch c = b.slice(q0, std::min(qc, nq - q0));
        HIP_TRY(hipMemcpyAsync(ix->sbd_q.p, c.q, (size_t)c.nq * ix->dpad * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemsetAsync(ix->sbd_cnt.p, 0, (size_t)c.nq * 12, s));
        kp.Q = ix->sbd_q.as<float>();
        kp.allow = c.allow;
        kp.nq = c.nq;
        kp.seg_keys = ix->bigk_seg.as<uint32_t>();
        kp.tau = ix->sbd_t.as<float>();
        TREC(6);
        if (ix->pq_on) {
            kq.b = kp;
            HIP_TRY(wv_launch_bigk_bound_pq(&kq, s));
        } else if (metric_is_l1(ix->metric)) {
            HIP_TRY(wv_launch_bigk_bound_l1(&kp, s));
        } else {
            HIP_TRY(wv_launch_bigk_bound(&kp, s));
        }
        TREC(7);
        wv::SbdParams sp{};
        sp.X = kp.X;
        sp.Q = kp.Q;
        sp.target = kp.tau;
        sp.excl = kp.excl;
        sp.allow = c.allow;
        sp.excl_nbits = kp.excl_nbits;
        sp.allow_nbits = c.allow_nbits;
        sp.allow_stride = c.allow_stride;
        sp.N = N;
        sp.D = kp.D;
        sp.ldx = kp.ldx;
        sp.dpad = kp.dpad;
        sp.metric = kp.metric;
        sp.nq = c.nq;
        sp.rows_per_block = sbd_scan_rows(ix, N, c.nq);
        sp.cap = cap;
        sp.keys = ix->sbd_keys.as<unsigned long long>();
        sp.cnt = ix->sbd_cnt.as<unsigned int>();
        TREC(0);
        if (own_pass) {
            if (int rc = sbd_kind_pass(ix, sp, s)) return rc;
        } else if (keyed) {
            if (int rc = sbd_h16_pass(ix, sp, ccap, s)) return rc;
        } else {
            HIP_TRY(wv_launch_sbd_scan(&sp, s));
        }
        TREC(1);
        TREC(2);   // (sort and emit: the finalize pair)
        HIP_TRY(wv_sbd_sort(sp.keys, ix->sbd_tmp.as<unsigned long long>(), sp.cnt, c.nq, cap, ix->sbd_off.as<int>(),
                            &ix->sbd_scr, &ix->sbd_scr_cap, s));
        kp.sorted = ix->sbd_tmp.as<unsigned long long>();
        kp.cnt = sp.cnt;
        kp.ccnt = keyed ? ix->sbd_ccnt.as<unsigned int>() : nullptr;
        kp.out_ids = c.out_ids;
        kp.out_d = c.out_d;
        kp.out_n = c.out_n;
        kp.flag = ix->bigk_flag.as<int32_t>();
        HIP_TRY(wv_launch_bigk_emit(&kp, s));
        TREC(3);
        HIP_TRY(hipMemcpyAsync(flags.data(), ix->bigk_flag.p, (size_t)c.nq * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint64_t n_legacy = (uint64_t)std::count_if(flags.begin(), flags.begin() + c.nq, [](int32_t f) { return f != 0; });
        ix->bigk_batched_q += (uint64_t)c.nq - n_legacy;
        ix->bigk_legacy_q += n_legacy;
        if (n_legacy)
            if (int rc = exact_each(ix, c, flags.data())) return rc;
    }
    return WV_OK;
}

}  // namespace wv_host

using namespace wv_host;

extern "C" {

int wv_index_set_large_k(wv_index* ix, int on) {
    if (!ix) return fail(WV_EINVAL, "wv_index_set_large_k: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->large_k = on != 0;
    return WV_OK;
}

int wv_last_large_k_stats(wv_index* ix, uint64_t* batched_queries, uint64_t* legacy_queries) {
    if (!ix) return fail(WV_EINVAL, "wv_last_large_k_stats: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    if (batched_queries) *batched_queries = ix->bigk_batched_q;
    if (legacy_queries) *legacy_queries = ix->bigk_legacy_q;
    return WV_OK;
}

}  // extern "C"
