// wv_search_hnsw.hip -- knnSearchByVector on the device: the launches of
// wv_hnsw.hip (register / LDS path, side-register path) with their LDS sizing
// and fallback, and the exact pass over the delta set beside the graph.
#include <cmath>

#include "wv_search.h"

using namespace wv_host;

namespace {

// waves per workgroup: up to 4, as many as fit 160 KiB of LDS
int waves_per_block(int per_wave_words) {
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * per_wave_words * 4 > 160 * 1024) --wpb;
    return wpb;
}

// what every launch of a batch reads of the index and the batch; the wave's
// LDS layout (sc, xs_log2, vc_log2, vc_tbits, per_wave_words) is the caller's
wv::HnswParams hnsw_params(wv_index* ix, const Batch& b, int ef, int efc) {
    wv::HnswParams hp{};
    hp.X = ix->vecs.as<float>();
    hp.levels = ix->levels.as<int8_t>();
    hp.layer0 = ix->layer0.as<uint32_t>();
    hp.upper_row = ix->upper_row.as<uint32_t>();
    hp.upper = ix->upper.as<uint32_t>();
    hp.tomb = ix->any_tomb ? ix->tomb.as<uint64_t>() : nullptr;
    hp.tomb_nbits = ix->capacity;
    hp.allow = b.allow;
    hp.allow_nbits = b.allow_nbits;
    hp.allow_stride = b.allow_stride;
    hp.Q = b.q;
    hp.N = ix->gn;
    hp.id_base = ix->cfg.id_base;
    hp.entrypoint = (uint32_t)ix->entrypoint;
    hp.D = ix->dim;
    hp.ldx = ix->ldx;
    hp.ldq = b.ldq;
    hp.metric = ix->metric;
    hp.deg0 = ix->deg0;
    hp.degU = ix->degU;
    hp.max_level = ix->max_level;
    hp.upper_levels = ix->max_level;
    hp.nq = b.nq;
    hp.k = b.k;
    hp.ef = ef;
    hp.efc = efc;
    hp.dpad = ix->dpad;
    hp.out_ids = b.out_ids;
    hp.out_d = b.out_d;
    hp.out_n = b.out_n;
    hp.status = ix->status.as<int32_t>();
    hp.counters = ix->counters.as<uint32_t>();
    if (ix->pq_on) hp.pq = pq_params(ix);   // compressed: PQ distances (search.go:171-199)
    return hp;
}

// Filtered / tombstoned / nil-node searches with ef <= 128 (round 6):
// the side-register path.  Layer 0 has an exact visited bitmap per query
// in HBM (nothing evaluated or queued twice) and a side set whose smallest
// keys sit in LDS, sized from the eligible fraction p (the live side set
// peaks near 1.4 ef (1-p)/p: oracle side diagnostics), the
// rest spilled to HBM.  Only a spill past its capacity takes the exact
// fallback.
int hnsw_side(wv_index* ix, const Batch& b, int ef, const wv::HnswParams& hp, int wg_max) {
    const int nq = b.nq;
    hipStream_t s = b.s;
    double p_el = 1.0;
    if (b.allow) {
        // (the graph's words only)
        const uint64_t words = std::min<uint64_t>((b.allow_nbits + 63) / 64, (ix->gn + 63) / 64);
        std::vector<unsigned long long> cnt;
        if (int rc = count_allow_rows(ix, b, words, &cnt)) return rc;
        const unsigned long long mn = *std::min_element(cnt.begin(), cnt.end());
        p_el = (double)mn / (double)std::max<uint64_t>(1, ix->gn);
    }
    p_el *= 1.0 - std::min(1.0, (double)ix->n_tomb / (double)std::max<uint64_t>(1, ix->gn));
    p_el = std::max(p_el, 1e-5);
    const double side_need = 1.4 * ef * (1.0 - p_el) / p_el;
    // per-wave LDS: 13 KiB (12 waves per CU); the side array takes what a
    // 2K-slot visited cache leaves, up to the live-set estimate
    const int side_kb = env_int("WV_HNSW_SIDE_KB", 13, 4);
    const int xl = 8;   // the upper levels' expanded set
    const int budget_words = side_kb * 256;
    const int base_words = wv_hnsw_side_per_wave_words(ix->dpad, 0, 11, xl);
    const int max_rows = std::max(4, (budget_words - base_words) / 128);
    int side_rows = std::min(max_rows, std::max(4, (int)std::ceil((side_need + 64.0) / 64.0)));
    if (const int r = env_int("WV_HNSW_SIDE_ROWS", 0, 4)) side_rows = r;
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
    const int wpb = waves_per_block(pw);
    // HBM scratch per query: the visited bitmap and the spill, in chunks
    // of at most WV_HNSW_SIDE_SCRATCH_MB (4 GiB) -- a 10M-row graph takes
    // 1.25 MB of bitmap a query
    hs.vwords = (ix->gn + 31) / 32;
    double cap = std::ceil(8.0 * side_need) + 4096.0;
    if (const int c = env_int("WV_HNSW_SPILL_CAP", 0, 64)) cap = c;
    hs.spill_cap = (int)std::min(cap, (double)(1 << 22));
    const size_t per_q = hs.vwords * 4 + (size_t)hs.spill_cap * 8;
    const size_t budget_b = (size_t)env_int("WV_HNSW_SIDE_SCRATCH_MB", 4096, 1) << 20;
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
    const bool ev_first = p_el < env_double("WV_HNSW_EV_BELOW", 0.4);
    hs.wg_helpers = nq <= wg_max ? 3 : 0;
    HIP_TRY(ix->stat_acc.ensure(48));
    hs.side_acc = ix->stat_acc.as<unsigned long long>();
    hs.ev_spec = env_on("WV_HNSW_EV_SPEC") ? 1 : 0;
    hs.vb_host_clear = env_on("WV_HNSW_VB_MEMSET") ? 1 : 0;
    const int passes = ev_first ? 1 : 2;
    for (int pass = 0; pass < passes; ++pass) {
        for (int c0 = 0; c0 < nq; c0 += chunk) {
            const Batch c = b.slice(c0, std::min(chunk, nq - c0));
            wv::HnswParams hc = hs;
            hc.nq = c.nq;
            hc.Q = c.q;
            hc.allow = c.allow;
            hc.out_ids = c.out_ids;
            hc.out_d = c.out_d;
            hc.out_n = c.out_n;
            hc.status = hp.status + c0;
            hc.counters = hp.counters + 2 * (size_t)c0;
            hc.redo = pass ? hc.status : nullptr;
            if (hc.vb_host_clear && (ev_first || pass))
                HIP_TRY(hipMemsetAsync(hs.vbits, 0, (size_t)c.nq * hs.vwords * 4, s));
            HIP_TRY(wv_launch_hnsw_side(&hc, wpb, ev_first || pass, s));
        }
    }
    return WV_OK;
}

// The register / LDS launch (hp laid out by run_hnsw, wpb waves a workgroup)
// and, under a filter, its wide second pass.
int hnsw_lds(wv_index* ix, const Batch& b, wv::HnswParams hp, bool filtered, bool reg, int wpb, int wg_max) {
    hipStream_t s = b.s;
    // small unfiltered batches (the batcher's callers): a workgroup per
    // query, whose three helper waves take the distance batches' other rows
    // -- while every workgroup is resident (up to 3 per CU at 158 VGPRs; a
    // 256-query batch 898 -> 705 us p50, profiles/r05/wg_latency.log).
    // WV_HNSW_WG_MAX: the largest such batch; 0 turns it off.
    const bool wg = !filtered && !ix->pq_on && reg && b.nq <= wg_max;
    if (wg) {
        hp.wg_helpers = 3;
        HIP_TRY(wv_launch_hnsw_wg(&hp, s));
    } else {
        HIP_TRY(wv_launch_hnsw(&hp, wpb, s));
    }
    if (!filtered) return WV_OK;
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
    const int fixed2 = wv_hnsw_per_wave_words(ix->dpad, hp.efc, h2.sc, 0, h2.xs_log2) - 1;
    h2.vc_log2 = choose_vc_log2(fixed2 + 1024, fixed2, ix->gn, &h2.vc_tbits);
    h2.per_wave_words = (wv_hnsw_per_wave_words(ix->dpad, hp.efc, h2.sc, h2.vc_log2, h2.xs_log2) + 3) & ~3;
    if ((size_t)h2.per_wave_words * 4 <= 160 * 1024)
        HIP_TRY(wv_launch_hnsw(&h2, waves_per_block(h2.per_wave_words), s));
    return WV_OK;
}

int run_hnsw(wv_index* ix, const Batch& b, int ef) {
    if (!ix->has_graph || ix->gn == 0) return fail(WV_ESTATE, "no graph uploaded");
    const int nq = b.nq;
    hipStream_t s = b.s;
    const int efc = std::max(64, (ef + 63) / 64 * 64);
    // Side candidates S (traversed but ineligible: search.go:282-298) and the
    // exact set of expanded side candidates exist only under a filter,
    // tombstones or nil nodes.  Without them the wave state shrinks and more
    // queries are in flight (the search is latency-bound on its gathers).  A
    // stray ineligible node still ends in the exact fallback (status bit 0),
    // never in a wrong answer.
    const bool filtered = b.allow != nullptr || ix->any_tomb || ix->any_nil;
    const int sc = filtered ? 256 : 0;
    const int xs_log2 = filtered ? 9 : 0;
    // register results (unfiltered, ef <= 256): the wave's LDS is the query,
    // the batch and the visited cache only
    const bool reg = !filtered && efc <= 256;
    const int fixed = reg ? wv_hnsw_reg_per_wave_words(ix->dpad, 0) - 1
                          : wv_hnsw_per_wave_words(ix->dpad, efc, sc, 0, xs_log2) - 1;
    // per-wave LDS budget: 20 KiB filtered (8 waves per CU), 12 KiB otherwise
    const int wave_kb = env_int("WV_HNSW_WAVE_KB", filtered ? 20 : 12, 4);
    const int budget = wave_kb * 1024 / 4;
    int vc_tbits = 0;
    const int vc_log2 = choose_vc_log2(budget, fixed, ix->gn, &vc_tbits);
    int per_wave = reg ? wv_hnsw_reg_per_wave_words(ix->dpad, vc_log2)
                       : wv_hnsw_per_wave_words(ix->dpad, efc, sc, vc_log2, xs_log2);
    per_wave = (per_wave + 3) & ~3;
    if ((size_t)per_wave * 4 > 160 * 1024) return fail(WV_EINVAL, "hnsw LDS footprint too large");
    HIP_TRY(ix->status.ensure((size_t)nq * 4));
    HIP_TRY(ix->counters.ensure((size_t)nq * 8));
    wv::HnswParams hp = hnsw_params(ix, b, ef, efc);
    hp.sc = sc;
    hp.vc_log2 = vc_log2;
    hp.vc_tbits = vc_tbits;
    hp.xs_log2 = xs_log2;
    hp.per_wave_words = per_wave;
    // diagnostic: exact per-query visited bitmaps for the evaluation counts
    // (a bounded sample: nq x N bits of scratch, freed after the launch)
    void* uniq = nullptr;
    // (bounded by bytes too: a 100M-node graph would take 51 GB at nq 4096)
    if (env_on("WV_HNSW_UNIQUE_COUNTS") && nq <= 4096 && (size_t)nq * ((ix->gn + 63) / 64) * 8 <= ((size_t)1 << 30)) {
        hp.uniq_words = (ix->gn + 63) / 64;
        HIP_TRY(hipMallocAsync(&uniq, (size_t)nq * hp.uniq_words * 8, s));
        HIP_TRY(hipMemsetAsync(uniq, 0, (size_t)nq * hp.uniq_words * 8, s));
        hp.uniq = static_cast<unsigned long long*>(uniq);
    }
    TREC(4);
    // the largest batch that gets a workgroup per query (512; both paths)
    const int wg_max = env_int("WV_HNSW_WG_MAX", 512);
    // the side-register path (filtered ef <= 128, uncompressed), else the
    // register / LDS path and its wide second pass
    const bool side = filtered && !ix->pq_on && efc <= 128;
    if (int rc = side ? hnsw_side(ix, b, ef, hp, wg_max)
                      : hnsw_lds(ix, b, hp, filtered, reg, waves_per_block(per_wave), wg_max))
        return rc;
    TREC(5);
    if (uniq) HIP_TRY(hipFreeAsync(uniq, s));
    HIP_TRY(ix->stat_acc.ensure(48));
    HIP_TRY(wv_launch_hnsw_stats(ix->counters.as<uint32_t>(), nq, ix->stat_acc.as<unsigned long long>(), s));
    if (!ix->pq_on) {
        // queries whose side state outgrew LDS: exact answer on the device
        HIP_TRY(ix->fail.ensure((size_t)nq * 4));
        HIP_TRY(ix->fail_thr.ensure((size_t)nq * 4));
        HIP_TRY(wv_launch_fbd_mark(ix->status.as<int32_t>(), nq, ix->fail.as<int32_t>(), ix->fail_thr.as<float>(),
                                   b.out_d, b.out_n, b.k, s));
        return queue_fbd(ix, b);
    }
    std::vector<int32_t> st(nq);
    HIP_TRY(hipMemcpyAsync(st.data(), ix->status.p, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // Queries whose side-candidate set outgrew LDS are answered exactly
    // (flatSearch over the same allow list: a superset in quality).
    return exact_each(ix, b, st.data());
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

}  // namespace

namespace wv_host {

// knnSearchByVector over the uploaded graph, plus an exact pass over the
// delta set (rows added since the graph snapshot), merged by
// (dist, id): added rows are findable at once, as in the reference where
// Add inserts into the live graph (insert.go:43-65).  Exact over the delta is
// a superset in quality of a graph search.
int run_hnsw_delta(wv_index* ix, const Batch& b, int ef) {
    if (ix->delta_count == 0 || b.nq == 0) return run_hnsw(ix, b, ef);
    const int nq = b.nq, k = b.k;
    hipStream_t s = b.s;
    const size_t nk = (size_t)nq * k;
    HIP_TRY(ix->dl_ids.ensure(2 * nk * 8));
    HIP_TRY(ix->dl_d.ensure(2 * nk * 4));
    HIP_TRY(ix->dl_n.ensure(2 * (size_t)nq * 4));
    uint64_t* ids = ix->dl_ids.as<uint64_t>();
    float* ds = ix->dl_d.as<float>();
    int32_t* ns = ix->dl_n.as<int32_t>();
    int rc = run_hnsw(ix, b.with_outputs(ids, ds, ns), ef);
    if (rc) return rc;
    const uint64_t words = ix->bm_words;
    const int rows = b.allow_rows();
    HIP_TRY(ix->dmask.ensure((size_t)rows * words * 8));
    hipLaunchKernelGGL(and_bits_kernel, dim3((unsigned)((rows * words + 255) / 256)), dim3(256), 0, s, b.allow,
                       (b.allow_nbits + 63) / 64, b.allow_stride, ix->delta.as<uint64_t>(), words, rows,
                       ix->dmask.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    // (per-query lists: the delta set is the shared bitmap run_exact compacts)
    const uint64_t st = b.allow && b.allow_stride ? words : 0;
    const uint64_t e = ix->last_dist, x = ix->last_exp, f = ix->last_fallbacks;
    rc = run_exact(ix, b.with_allow(ix->dmask.as<uint64_t>(), ix->capacity, st).with_outputs(ids + nk, ds + nk, ns + nq),
                   st ? ix->delta.as<uint64_t>() : nullptr, ix->capacity);
    if (rc) return rc;
    ix->last_dist = e;
    ix->last_exp = x;
    ix->last_fallbacks += f;
    HIP_TRY(launch_merge_shards(ds, ids, ns, 2, nq, k, b.out_d, b.out_ids, b.out_n, s));
    return WV_OK;
}

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

}  // namespace wv_host
