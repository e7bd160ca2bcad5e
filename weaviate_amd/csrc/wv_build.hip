// wv_build.hip -- the index's HNSW graph: built on the device from the
// uploaded rows (wv_index_build_graph), extended in place with the rows added
// since (wv_index_extend_graph), uploaded from or downloaded to the host.
// Kernels: wv_hnsw.hip ("GPU graph construction"), wv_graph_grow.hip.
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "wv_device.h"
#include "wv_search.h"

using namespace wv_host;

extern "C" {

// level draw of the restatement (oracle/wv_oracle.c insert_node): a
// counter-based U(0,1) per id, targetLevel = floor(-ln(U) * 1/ln(M))
// (insert.go:132, index.go:226) -- identical levels on the CPU and the GPU
static int draw_level(uint64_t seed, uint64_t id, double normalizer) {
    auto mix = [](uint64_t x) {
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 27; x *= 0x94D049BB133111EBull;
        x ^= x >> 31;
        return x;
    };
    const uint64_t r = mix(seed * 0xD1B54A32D192ED03ull + id * 0x9E3779B97F4A7C15ull + 1);
    const double u = ((double)(r >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const int t = (int)std::floor(-std::log(u) * normalizer);
    return t > 126 ? 126 : t;
}

// insert.go:103-217 in batches (wv_hnsw.hip, "GPU graph construction"): the
// rows [done, n) join the graph of the `done` nodes before them, whose top
// level is `top` and entrypoint `ep`; both are updated.  The graph arrays hold
// n nodes (the part from `done` on padded), `upper` and the upper counts have
// the level stride ul, and the counts describe the lists.  lv: the levels of
// the new ids only, lv[i - done].
static int insert_batches(wv_index* ix, int ef_construction, int batch_div, uint64_t done, uint64_t n, const int8_t* lv,
                          int ul, int& top, uint64_t& ep) {
    hipStream_t s = ix->stream;
    const int M = ix->cfg.max_connections, M0 = 2 * M;
    const uint64_t lv0 = done;
    // per-wave search state as in run_hnsw (unfiltered layout)
    const int efc = std::max(64, (ef_construction + 63) / 64 * 64);
    const int fixed = wv_hnsw_per_wave_words(ix->dpad, efc, 0, 0, 0) - 1;
    int vc_tbits = 0;
    const int vc_log2 = choose_vc_log2(12 * 1024 / 4, fixed, n, &vc_tbits);
    int per_wave = (wv_hnsw_per_wave_words(ix->dpad, efc, 0, vc_log2, 0) + 3) & ~3;
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * per_wave * 4 > 160 * 1024) --wpb;
    const int bmax = 16384;
    // WV_BUILD_TRACE=1 (diagnostic): per-phase device times (events) summed
    // over intervals of 64 batches, printed to stderr with the host time
    const bool trace = std::getenv("WV_BUILD_TRACE") != nullptr;
    hipEvent_t tev[5] = {};
    double tph[4] = {0, 0, 0, 0};
    uint64_t tbatches = 0, treq = 0, truns = 0;
    auto thost = std::chrono::steady_clock::now();
    if (trace)
        for (auto& e : tev) HIP_TRY(hipEventCreate(&e));
    while (done < n) {
        const int nb = (int)std::min<uint64_t>(n - done, std::max<uint64_t>(1, std::min<uint64_t>(bmax, done / batch_div)));
        int lb = 1;
        const int8_t* blv = lv + (done - lv0);   // the batch's levels
        for (int i = 0; i < nb; ++i) lb = std::max(lb, blv[i] + 1);
        HIP_TRY(ix->b_tgt.ensure(nb));
        HIP_TRY(ix->b_ci.ensure((size_t)nb * lb * ef_construction * 4));
        HIP_TRY(ix->b_cd.ensure((size_t)nb * lb * ef_construction * 4));
        HIP_TRY(ix->b_cn.ensure((size_t)nb * lb * 4));
        const size_t nreq = (size_t)nb * lb * M;
        HIP_TRY(ix->b_rk.ensure(nreq * 8));
        HIP_TRY(ix->b_rn.ensure(nreq * 4));
        HIP_TRY(ix->b_rk2.ensure(nreq * 8));
        HIP_TRY(ix->b_rn2.ensure(nreq * 4));
        HIP_TRY(ix->b_uk.ensure(nreq * 8));
        HIP_TRY(ix->b_ul.ensure(nreq * 4));
        HIP_TRY(ix->b_uo.ensure(nreq * 4));
        HIP_TRY(ix->b_nr.ensure(8));
        HIP_TRY(hipMemcpyAsync(ix->b_tgt.p, blv, nb, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(ix->b_cn.p, 0, (size_t)nb * lb * 4, s));
        wv::BuildParams b{};
        wv::HnswParams& h = b.h;
        h.X = ix->vecs.as<float>();
        h.levels = ix->levels.as<int8_t>();
        h.layer0 = ix->layer0.as<uint32_t>();
        h.upper_row = ix->upper_row.as<uint32_t>();
        h.upper = ix->upper.as<uint32_t>();
        h.N = done;
        h.entrypoint = (uint32_t)ep;
        h.D = ix->dim;
        h.ldx = ix->ldx;
        h.ldq = ix->dpad;
        h.metric = ix->metric;
        h.deg0 = M0;
        h.degU = M;
        h.max_level = top;
        h.upper_levels = ul;
        h.nq = nb;
        h.ef = ef_construction;
        h.efc = efc;
        h.sc = 0;
        h.vc_log2 = vc_log2;
        h.vc_tbits = vc_tbits;
        h.xs_log2 = 0;
        h.dpad = ix->dpad;
        h.per_wave_words = per_wave;
        b.first = done;
        b.nb = nb;
        b.lb = lb;
        b.M = M;
        b.M0 = M0;
        b.target = ix->b_tgt.as<int8_t>();
        b.cand_i = ix->b_ci.as<uint32_t>();
        b.cand_d = ix->b_cd.as<float>();
        b.cand_n = ix->b_cn.as<int32_t>();
        b.counts0 = ix->b_cnt0.as<uint32_t>();
        b.countsU = ix->b_cntu.as<uint32_t>();
        b.req_key = ix->b_rk.as<uint64_t>();
        b.req_node = ix->b_rn.as<uint32_t>();
        if (trace) HIP_TRY(hipEventRecord(tev[0], s));
        HIP_TRY(wv_launch_build_search(&b, wpb, s));
        if (trace) HIP_TRY(hipEventRecord(tev[1], s));
        HIP_TRY(wv_launch_build_select(&b, s));
        if (trace) HIP_TRY(hipEventRecord(tev[2], s));
        // reverse links grouped by (level, neighbour), batch order kept (stable)
        size_t tb = 0, tb2 = 0, tb3 = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ix->b_rk.as<uint64_t>(), ix->b_rk2.as<uint64_t>(),
                                                   ix->b_rn.as<uint32_t>(), ix->b_rn2.as<uint32_t>(), (int)nreq, 0, 64,
                                                   s));
        HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, tb2, ix->b_rk2.as<uint64_t>(), ix->b_uk.as<uint64_t>(),
                                                      ix->b_ul.as<uint32_t>(), ix->b_nr.as<uint32_t>(), (int)nreq, s));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb3, ix->b_ul.as<uint32_t>(), ix->b_uo.as<uint32_t>(),
                                                 (int)nreq, s));
        HIP_TRY(ix->b_tmp.ensure(std::max(tb, std::max(tb2, tb3))));
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ix->b_tmp.p, tb, ix->b_rk.as<uint64_t>(), ix->b_rk2.as<uint64_t>(),
                                                   ix->b_rn.as<uint32_t>(), ix->b_rn2.as<uint32_t>(), (int)nreq, 0, 64,
                                                   s));
        HIP_TRY(hipMemsetAsync(ix->b_ul.p, 0, nreq * 4, s));
        HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(ix->b_tmp.p, tb2, ix->b_rk2.as<uint64_t>(),
                                                      ix->b_uk.as<uint64_t>(), ix->b_ul.as<uint32_t>(),
                                                      ix->b_nr.as<uint32_t>(), (int)nreq, s));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(ix->b_tmp.p, tb3, ix->b_ul.as<uint32_t>(), ix->b_uo.as<uint32_t>(),
                                                 (int)nreq, s));
        uint32_t n_runs = 0;
        if (trace) HIP_TRY(hipEventRecord(tev[3], s));
        HIP_TRY(hipMemcpyAsync(&n_runs, ix->b_nr.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        b.run_key = ix->b_uk.as<uint64_t>();
        b.run_off = ix->b_uo.as<uint32_t>();
        b.run_len = ix->b_ul.as<uint32_t>();
        b.sorted_node = ix->b_rn2.as<uint32_t>();
        b.n_runs = (int)n_runs;
        HIP_TRY(wv_launch_build_link(&b, s));
        if (trace) {
            HIP_TRY(hipEventRecord(tev[4], s));
            HIP_TRY(hipEventSynchronize(tev[4]));
            for (int i = 0; i < 4; ++i) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, tev[i], tev[i + 1]));
                tph[i] += ms;
            }
            ++tbatches;
            treq += nreq;
            truns += n_runs;
            if (tbatches % 64 == 0 || done + nb >= n) {
                const auto now = std::chrono::steady_clock::now();
                std::fprintf(stderr,
                             "[build] done %llu nb %d lb %d | %llu batches: host %.1f ms, search %.1f select %.1f "
                             "sort %.1f link %.1f ms, req %.2fM runs %.2fM\n",
                             (unsigned long long)(done + nb), nb, lb, (unsigned long long)tbatches,
                             std::chrono::duration<double, std::milli>(now - thost).count(), tph[0], tph[1], tph[2],
                             tph[3], treq / 1e6, truns / 1e6);
                thost = now;
                tph[0] = tph[1] = tph[2] = tph[3] = 0;
                tbatches = treq = truns = 0;
            }
        }
        // the batch is in the graph: its levels make it reachable for the next one
        HIP_TRY(hipMemcpyAsync(ix->levels.as<int8_t>() + done, blv, nb, hipMemcpyHostToDevice, s));
        for (int i = 0; i < nb; ++i)   // insert.go:202-213: a higher node becomes the entrypoint
            if (blv[i] > top) { top = blv[i]; ep = done + i; }
        done += nb;
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (trace)
        for (auto& e : tev) HIP_TRY(hipEventDestroy(e));
    return WV_OK;
}

int wv_index_build_graph(wv_index* ix, int ef_construction, uint64_t seed, int batch_div) {
    if (check(ix) || ef_construction < 1 || ef_construction > wv::HNSW_EF_MAX || batch_div < 1)
        return fail(WV_EINVAL, "wv_index_build_graph: bad argument");
    std::lock_guard<std::mutex> guard(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    const uint64_t n = ix->n_rows;
    if (n == 0) return fail(WV_ESTATE, "wv_index_build_graph: no vectors");
    for (uint64_t i = 0; i < n; ++i)
        if (!(ix->has_vec[i >> 6] & (1ull << (i & 63)))) return fail(WV_ESTATE, "wv_index_build_graph: a row has no vector");
    const int M = ix->cfg.max_connections, M0 = 2 * M;
    if (M < 2 || M0 > 256) return fail(WV_EINVAL, "wv_index_build_graph: maxConnections out of range");
    // levels: the first node is insertInitialElement's level 0 (insert.go:67-101)
    std::vector<int8_t> lv(n);
    const double norm = 1.0 / std::log((double)M);
    int maxL = 0;
    uint64_t n_upper = 0;
    std::vector<uint32_t> urow(n, WV_NIL);
    for (uint64_t i = 0; i < n; ++i) {
        lv[i] = (int8_t)(i == 0 ? 0 : draw_level(seed, i, norm));
        maxL = std::max<int>(maxL, lv[i]);
        if (lv[i] >= 1) urow[i] = (uint32_t)n_upper++;
    }
    const int ul = std::max(1, maxL);
    HIP_TRY(ix->levels.ensure(n));
    HIP_TRY(ix->layer0.ensure(n * (size_t)M0 * 4));
    HIP_TRY(ix->upper_row.ensure(n * 4));
    HIP_TRY(ix->upper.ensure(std::max<uint64_t>(1, n_upper) * ul * (size_t)M * 4));
    HIP_TRY(ix->b_cnt0.ensure(n * 4));
    HIP_TRY(ix->b_cntu.ensure(std::max<uint64_t>(1, n_upper) * ul * 4));
    HIP_TRY(hipMemsetAsync(ix->levels.p, 0xFF, n, s));   // -1: not inserted yet
    HIP_TRY(hipMemsetAsync(ix->layer0.p, 0xFF, n * (size_t)M0 * 4, s));
    HIP_TRY(hipMemsetAsync(ix->upper.p, 0xFF, std::max<uint64_t>(1, n_upper) * ul * (size_t)M * 4, s));
    HIP_TRY(hipMemsetAsync(ix->b_cnt0.p, 0, n * 4, s));
    HIP_TRY(hipMemsetAsync(ix->b_cntu.p, 0, std::max<uint64_t>(1, n_upper) * ul * 4, s));
    HIP_TRY(hipMemcpyAsync(ix->upper_row.p, urow.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ix->levels.p, lv.data(), 1, hipMemcpyHostToDevice, s));   // node 0
    uint64_t ep = 0;
    int top = 0;
    int rc = insert_batches(ix, ef_construction, batch_div, 1, n, lv.data() + 1, ul, top, ep);
    if (rc) return rc;
    ix->nil_host.assign(ix->bm_words, ~0ull);
    for (uint64_t i = 0; i < lv.size(); ++i)
        if (lv[i] >= 0) ix->nil_host[i >> 6] &= ~(1ull << (i & 63));
    ix->gn = n;
    ix->deg0 = M0;
    ix->degU = M;
    ix->max_level = top;
    ix->n_upper = n_upper;
    ix->entrypoint = ep;
    ix->has_graph = true;
    ix->any_nil = false;
    for (uint64_t i = 0; i < n; ++i) ix->pending_host[i >> 6] &= ~(1ull << (i & 63));
    ix->bitmaps_dirty = true;
    return WV_OK;
}

// A graph array at new_bytes: the first old_bytes kept, the rest filled with
// `pad` (regrow zero-fills and skips unallocated buffers; the graph's arrays
// pad with 0xFF).  A buffer that moves is freed once the device is idle: a
// search queued on a caller's stream may still read it.
static hipError_t grow_padded(DevBuf& b, size_t old_bytes, size_t new_bytes, int pad, hipStream_t s) {
    if (new_bytes <= old_bytes) return hipSuccess;
    if (new_bytes <= b.cap) return hipMemsetAsync(static_cast<char*>(b.p) + old_bytes, pad, new_bytes - old_bytes, s);
    size_t want = std::max<size_t>(new_bytes, 256);
    if (b.cap) want = std::max(want, std::min(b.cap + b.cap / 2, new_bytes + ((size_t)256 << 20)));
    void* np = nullptr;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess) return e;
    old_bytes = std::min(old_bytes, b.cap);
    if (old_bytes) e = hipMemcpyAsync(np, b.p, old_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<char*>(np) + old_bytes, pad, new_bytes - old_bytes, s);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(np); return e; }
    if (b.p) (void)hipFree(b.p);
    b.p = np;
    b.cap = want;
    return hipSuccess;
}

int wv_index_extend_graph(wv_index* ix, int ef_construction, uint64_t seed, int batch_div, uint64_t* inserted) {
    if (inserted) *inserted = 0;
    if (ef_construction < 1 || ef_construction > wv::HNSW_EF_MAX)
        return fail(WV_EINVAL, "wv_index_extend_graph: ef_construction outside 1.." + std::to_string(wv::HNSW_EF_MAX));
    if (batch_div < 1) return fail(WV_EINVAL, "wv_index_extend_graph: batch_div < 1");
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> guard(ix->mu);
    if (!ix->has_graph || ix->gn == 0) return fail(WV_ESTATE, "wv_index_extend_graph: the index has no graph");
    const uint64_t gn = ix->gn, n = ix->n_rows;
    if (n <= gn) return WV_OK;   // nothing to add
    const int M = ix->cfg.max_connections, M0 = 2 * M;
    if (M < 2 || M0 > 256) return fail(WV_ESTATE, "wv_index_extend_graph: maxConnections out of range");
    if (ix->deg0 != M0 || ix->degU != M)
        return fail(WV_ESTATE, "wv_index_extend_graph: the graph's degrees (" + std::to_string(ix->deg0) + ", " +
                                   std::to_string(ix->degU) + ") are not 2 x maxConnections and maxConnections (" +
                                   std::to_string(M0) + ", " + std::to_string(M) + ")");
    // The build search passes no tombstone set, and insert.go keeps deleted
    // nodes out of its results (search.go:294, neighbor_connections.go:217):
    // over a graph that holds nil or tombstoned nodes the caller rebuilds.
    for (uint64_t i = 0; i < gn; ++i) {
        const uint64_t bit = 1ull << (i & 63);
        if (ix->nil_host[i >> 6] & bit)
            return fail(WV_ESTATE, "wv_index_extend_graph: graph node " + std::to_string(i) + " is nil");
        if (ix->tomb_host[i >> 6] & bit)
            return fail(WV_ESTATE, "wv_index_extend_graph: graph node " + std::to_string(i) + " has a tombstone");
    }
    for (uint64_t i = gn; i < n; ++i)
        if (!(ix->has_vec[i >> 6] & (1ull << (i & 63))))
            return fail(WV_ESTATE, "wv_index_extend_graph: row " + std::to_string(i) + " has no vector");
    // levels and `upper` rows of the new ids (the draw of wv_index_build_graph)
    const uint64_t k = n - gn;
    std::vector<int8_t> lv(k);
    std::vector<uint32_t> urow(k, WV_NIL);
    const double norm = 1.0 / std::log((double)M);
    int maxL = ix->max_level;
    uint64_t n_upper = ix->n_upper;
    for (uint64_t i = 0; i < k; ++i) {
        lv[i] = (int8_t)draw_level(seed, gn + i, norm);
        maxL = std::max<int>(maxL, lv[i]);
        if (lv[i] >= 1) urow[i] = (uint32_t)n_upper++;
    }
    const int ul_old = std::max(1, ix->max_level), ul = std::max(1, maxL);
    const uint64_t nu_old = ix->n_upper;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    HIP_TRY(hipStreamSynchronize(s));
    // WV_BUILD_TRACE=1 (diagnostic): the preparation's steps, each waited for
    const bool trace = std::getenv("WV_BUILD_TRACE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    double t_step[3] = {0, 0, 0};   // growth, counts, re-layout
    auto step_done = [&](int i) -> hipError_t {
        if (!trace) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        t_step[i] += std::chrono::duration<double, std::milli>(now - t0).count();
        t0 = now;
        return e;
    };
    // the per-node arrays at n nodes: the new part not inserted yet (-1), empty
    HIP_TRY(grow_padded(ix->levels, gn, n, 0xFF, s));
    HIP_TRY(grow_padded(ix->layer0, gn * (size_t)M0 * 4, n * (size_t)M0 * 4, 0xFF, s));
    HIP_TRY(grow_padded(ix->upper_row, gn * 4, n * 4, 0xFF, s));
    HIP_TRY(hipMemcpyAsync(ix->upper_row.as<uint32_t>() + gn, urow.data(), k * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(step_done(0));
    // neighbour counts, read off the lists (none are kept between calls)
    HIP_TRY(ix->b_cnt0.ensure(n * 4));
    HIP_TRY(hipMemsetAsync(ix->b_cnt0.p, 0, n * 4, s));
    HIP_TRY(wv_launch_list_counts(ix->layer0.as<uint32_t>(), gn, M0, ix->b_cnt0.as<uint32_t>(), s));
    const size_t cu_words = std::max<uint64_t>(1, n_upper) * (size_t)ul;
    if (ul != ul_old || n_upper != nu_old) {
        // `upper` re-laid at [n_upper][ul][M], its counts with it
        HIP_TRY(ix->b_tmp.ensure(std::max<uint64_t>(1, nu_old) * (size_t)ul_old * 4));
        HIP_TRY(wv_launch_list_counts(ix->upper.as<uint32_t>(), nu_old * (uint64_t)ul_old, M, ix->b_tmp.as<uint32_t>(),
                                      s));
        HIP_TRY(step_done(1));
        DevBuf up;
        HIP_TRY(up.ensure(cu_words * M * 4));
        hipError_t e = ix->b_cntu.ensure(cu_words * 4);
        if (e == hipSuccess) e = hipMemsetAsync(up.p, 0xFF, cu_words * M * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(ix->b_cntu.p, 0, cu_words * 4, s);
        if (e == hipSuccess)
            e = wv_launch_upper_relay(ix->upper.as<uint32_t>(), ix->b_tmp.as<uint32_t>(), nu_old, ul_old, ul, M,
                                      up.as<uint32_t>(), ix->b_cntu.as<uint32_t>(), s);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            up.release();
            HIP_TRY(e);
        }
        std::swap(ix->upper, up);
        up.release();
        HIP_TRY(step_done(2));
    } else {
        HIP_TRY(ix->b_cntu.ensure(cu_words * 4));
        HIP_TRY(hipMemsetAsync(ix->b_cntu.p, 0, cu_words * 4, s));
        HIP_TRY(wv_launch_list_counts(ix->upper.as<uint32_t>(), nu_old * (uint64_t)ul, M, ix->b_cntu.as<uint32_t>(), s));
        HIP_TRY(step_done(1));
    }
    if (trace)
        std::fprintf(stderr,
                     "[extend] %llu nodes + %llu rows, upper %llu x %d -> %llu x %d: grow %.2f ms, counts %.2f ms, "
                     "re-layout %.2f ms\n",
                     (unsigned long long)gn, (unsigned long long)k, (unsigned long long)nu_old, ul_old,
                     (unsigned long long)n_upper, ul, t_step[0], t_step[1], t_step[2]);
    // from here on `upper` has the stride of the graph to come: a failure
    // below leaves the index without a graph (its rows are still served exactly)
    int top = ix->max_level;
    uint64_t ep = ix->entrypoint;
    int rc = insert_batches(ix, ef_construction, batch_div, gn, n, lv.data(), ul, top, ep);
    if (rc) {
        ix->has_graph = false;
        ix->bitmaps_dirty = true;
        return rc;
    }
    for (uint64_t i = gn; i < n; ++i) {
        ix->nil_host[i >> 6] &= ~(1ull << (i & 63));
        ix->pending_host[i >> 6] &= ~(1ull << (i & 63));
    }
    ix->gn = n;
    ix->max_level = top;
    ix->n_upper = n_upper;
    ix->entrypoint = ep;
    ix->bitmaps_dirty = true;
    if (inserted) *inserted = k;
    return WV_OK;
}

int wv_index_download_graph(wv_index* ix, int8_t* levels, uint32_t* layer0, uint32_t* upper_row, uint32_t* upper) {
    if (check(ix) || !ix->has_graph) return fail(WV_ESTATE, "wv_index_download_graph: no graph");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    const uint64_t n = ix->gn;
    if (levels) HIP_TRY(hipMemcpyAsync(levels, ix->levels.p, n, hipMemcpyDeviceToHost, s));
    if (layer0) HIP_TRY(hipMemcpyAsync(layer0, ix->layer0.p, n * (size_t)ix->deg0 * 4, hipMemcpyDeviceToHost, s));
    if (upper_row) HIP_TRY(hipMemcpyAsync(upper_row, ix->upper_row.p, n * 4, hipMemcpyDeviceToHost, s));
    if (upper && ix->max_level > 0)
        HIP_TRY(hipMemcpyAsync(upper, ix->upper.p, ix->n_upper * (size_t)ix->max_level * ix->degU * 4,
                               hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return WV_OK;
}

int wv_index_graph_info(wv_index* ix, uint64_t* n, int* deg0, int* degU, int* max_level, uint64_t* n_upper,
                        uint64_t* entrypoint) {
    if (check(ix) || !ix->has_graph) return fail(WV_ESTATE, "wv_index_graph_info: no graph");
    if (n) *n = ix->gn;
    if (deg0) *deg0 = ix->deg0;
    if (degU) *degU = ix->degU;
    if (max_level) *max_level = ix->max_level;
    if (n_upper) *n_upper = ix->n_upper;
    if (entrypoint) *entrypoint = ix->entrypoint;
    return WV_OK;
}

int wv_index_upload_graph(wv_index* ix, uint64_t n, const int8_t* levels, const uint32_t* layer0, int deg0,
                          const uint32_t* upper_row, const uint32_t* upper, uint64_t n_upper, int degU, int max_level,
                          uint64_t entrypoint) {
    if (check(ix)) return WV_EINVAL;
    if (n == 0 || n > ix->capacity || !levels || !layer0 || deg0 <= 0 || deg0 > 256 || max_level < 0 ||
        entrypoint >= n || (max_level > 0 && (!upper_row || !upper || degU <= 0 || degU > 256)))
        return fail(WV_EINVAL, "wv_index_upload_graph: bad argument");
    // A nil entrypoint is the reference's "entrypoint was deleted"
    // (search.go:473-476).  An entrypoint below max_level is legal: the
    // descent skips a node whose level is below the layer (search.go:226-233),
    // as after deleteEntrypoint wrote the lower level first (delete.go:405-414).
    // Checked before any loop reads `upper`, whose size is n_upper * max_level
    // * degU: the caller's array must have exactly that level stride.
    if (levels[entrypoint] < 0) return fail(WV_EDELETED, "wv_index_upload_graph: entrypoint is a nil node");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    // validate neighbour ids on the host once (a bad id would fault the kernel)
    for (uint64_t i = 0; i < n * (uint64_t)deg0; ++i)
        if (layer0[i] != WV_NIL && layer0[i] >= n) return fail(WV_EINVAL, "layer0 neighbour out of range");
    if (max_level > 0) {
        for (uint64_t i = 0; i < n; ++i) {
            if (levels[i] >= 1 && (upper_row[i] == WV_NIL || upper_row[i] >= n_upper))
                return fail(WV_EINVAL, "upper_row out of range");
        }
        for (uint64_t i = 0; i < n_upper * (uint64_t)max_level * degU; ++i)
            if (upper[i] != WV_NIL && upper[i] >= n) return fail(WV_EINVAL, "upper neighbour out of range");
    }
    HIP_TRY(ix->levels.ensure(n));
    HIP_TRY(ix->layer0.ensure(n * (size_t)deg0 * 4));
    HIP_TRY(ix->upper_row.ensure(n * 4));
    HIP_TRY(ix->upper.ensure(std::max<uint64_t>(1, n_upper * (uint64_t)std::max(1, max_level) * std::max(1, degU)) * 4));
    HIP_TRY(hipMemcpyAsync(ix->levels.p, levels, n, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->layer0.p, layer0, n * (size_t)deg0 * 4, hipMemcpyHostToDevice, ix->stream));
    if (max_level > 0) {
        HIP_TRY(hipMemcpyAsync(ix->upper_row.p, upper_row, n * 4, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipMemcpyAsync(ix->upper.p, upper, n_upper * (size_t)max_level * degU * 4, hipMemcpyHostToDevice,
                               ix->stream));
    }
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->nil_host.assign(ix->bm_words, ~0ull);
    for (uint64_t i = 0; i < n; ++i)
        if (levels[i] >= 0) ix->nil_host[i >> 6] &= ~(1ull << (i & 63));
    ix->any_nil = std::any_of(levels, levels + n, [](int8_t l) { return l < 0; });
    for (uint64_t i = 0; i < n; ++i)   // the new snapshot holds these added rows
        if (levels[i] >= 0) ix->pending_host[i >> 6] &= ~(1ull << (i & 63));
    ix->gn = n;
    ix->deg0 = deg0;
    ix->degU = max_level > 0 ? degU : 1;
    ix->max_level = max_level;
    ix->n_upper = n_upper;
    ix->entrypoint = entrypoint;
    ix->has_graph = true;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

}  // extern "C"
