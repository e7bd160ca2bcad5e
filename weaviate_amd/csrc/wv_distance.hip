// wv_distance.hip -- SearchByVectorDistance of the C ABI: the two batches
// (allow lists as bitmaps or as ids), their host arithmetic over the
// threshold passes of wv_sbd.hip / wv_sbd_pq.hip, and the per-query path.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "wv_search.h"

using namespace wv_host;

// SearchByVectorDistance (search.go:90-158) for a batch of queries, on the
// device: round 1 (limit 100) is the batch's SearchByVector where it would
// run HNSW; every exact round -- round 1 of a flat search, and all rounds
// past the first (limit 1100, 11100, ...: their ef exceeds the beam) -- is
// answered by one threshold pass + segmented sort (wv_sbd.hip), launched
// beside round 1 so the batch syncs once.  The rounds' arithmetic
// (searchByDistParams, :552-619) then runs on the host over the counts.  A
// compressed index runs the same flow with the PQ distance (wv_sbd_pq.hip):
// its exact rounds are flat searches over the codes, ordered by (dist, row).
// A query whose within-target set outgrows its list (WV_SBD_CAP, 16384) takes
// the per-query path.
namespace {
// Switches of the compressed threshold passes, read per call.  WV_SBD_PQ=0: a
// compressed index takes the per-query path (A/B runs).  WV_SBD_PQ_LUT=0|1:
// every workgroup evaluates rows directly / from the lookup table wherever it
// fits; unset: the table where the workgroup's share of rows is at least ks.
bool sbd_pq_enabled() {
    const char* e = std::getenv("WV_SBD_PQ");
    return !(e && e[0] == '0' && !e[1]);
}
int sbd_pq_lut() { return env_tri("WV_SBD_PQ_LUT"); }
// entries of a query's list (WV_SBD_CAP, read per call)
int sbd_cap() { return env_int("WV_SBD_CAP", 16384, 128); }

// Round 1 (limit 100) of the queries that search by HNSW, on the host: slot[q]
// is query q's row of ids / d ([nh][100]) and n ([nh]), -1 where round 1 is
// exact too -- the accessors then return nulls
struct SbdRound1 {
    std::vector<uint64_t> ids;
    std::vector<float> d;
    std::vector<int32_t> n;
    std::vector<int> slot;
    explicit SbdRound1(int nq) : slot(nq, -1) {}
    void resize(int nh) {
        ids.resize((size_t)std::max(nh, 1) * 100);
        d.resize((size_t)std::max(nh, 1) * 100);
        n.resize(std::max(nh, 1));
    }
    const uint64_t* ids_of(int q) const { return slot[q] >= 0 ? ids.data() + (size_t)slot[q] * 100 : nullptr; }
    const float* d_of(int q) const { return slot[q] >= 0 ? d.data() + (size_t)slot[q] * 100 : nullptr; }
    int32_t n_of(int q) const { return slot[q] >= 0 ? n[slot[q]] : 0; }
};

// the fields SbdParams and SbdIdsParams share, from the staged batch
template <class P>
void sbd_fill(const wv_index* ix, P& sp) {
    sp.X = ix->vecs.as<float>();
    sp.Q = ix->sbd_q.as<float>();
    sp.target = ix->sbd_t.as<float>();
    sp.excl = ix->excl.as<uint64_t>();
    sp.excl_nbits = ix->capacity;
    sp.D = ix->dim;
    sp.dpad = ix->dpad;
    sp.ldx = ix->ldx;
    sp.metric = ix->metric;
    sp.keys = ix->sbd_keys.as<unsigned long long>();
    sp.cnt = ix->sbd_cnt.as<unsigned int>();
}

// the search.go:90-158 loop over an exact sorted list (from round r0: 1 when
// round 1 is exact too, 2 after an HNSW round 1): the end of the kept prefix
int64_t sbd_exact_rounds(int r0, int64_t Qn, int64_t A, int64_t n, int64_t max_limit) {
    int64_t prev = 0, total = 100, limit = 100, kept = r0 == 1 ? 0 : 100;
    for (int r = 1;; ++r) {
        if (r > 1) {
            prev = total;
            limit *= 10;
            total = prev + limit;
            if (max_limit >= 0 && total > max_limit) break;   // maxLimitReached
        }
        if (total > (int64_t)1 << 40) break;
        if (r < r0) continue;
        const int64_t lo = std::min(prev, n), hi = std::min(total, n);
        if (hi - lo <= 0) break;
        kept = std::max(lo, std::min(hi, Qn));   // (appending stops at the first entry past the target)
        if (!(hi <= A)) break;                   // lastFound <= target
    }
    return kept;
}

// whether an HNSW round 1 (its hi distances, ascending) lets the deepening go on
bool sbd_r1_continues(const float* r1_d, int64_t hi, float t, int64_t max_limit) {
    return hi > 0 && r1_d[hi - 1] <= t && (max_limit < 0 || 1100 <= max_limit);
}

// entries of a query's sorted list that the rounds keep, from its counts
// cnt3 = {|Q|, A, n}; r1_d / r1_n: its HNSW round 1 (r1_d null: round 1 is
// exact too).  (An HNSW round 1 that ends the deepening needs no list.)
int64_t sbd_list_need(const float* r1_d, int32_t r1_n, float t, int64_t max_limit, const unsigned int* cnt3) {
    if (r1_d && !sbd_r1_continues(r1_d, std::min<int64_t>(100, r1_n), t, max_limit)) return 0;
    const int64_t kept = sbd_exact_rounds(r1_d ? 2 : 1, cnt3[0], cnt3[1], cnt3[2], max_limit);
    return std::min<int64_t>(kept, cnt3[0]);
}

// a query's answer: the qualifying prefix of its HNSW round 1 (r1_d non-null),
// then the kept entries of its sorted list, decoded; returns the count
int64_t sbd_emit(const uint64_t* r1_ids, const float* r1_d, int32_t r1_n, float t, int64_t max_limit,
                 const std::vector<unsigned long long>& list, uint64_t id_base, uint64_t* out_ids, float* out_dists,
                 int64_t out_cap) {
    int64_t m = 0;
    auto put = [&](uint64_t id, float d) {
        if (m < out_cap) { out_ids[m] = id; out_dists[m] = d; }
        m++;
    };
    auto qual = [&](float d) { return d <= t || std::fabs((double)d - (double)t) <= 1e-6; };
    bool exact_more = true;
    if (r1_d) {
        // round 1 from the HNSW search: its qualifying prefix, and whether
        // the deepening continues
        const int64_t hi = std::min<int64_t>(100, r1_n);
        for (int64_t j = 0; j < hi; ++j) {
            const float d = r1_d[j];
            if (!qual(d)) break;
            put(r1_ids[j], d);
        }
        exact_more = sbd_r1_continues(r1_d, hi, t, max_limit);
    }
    if (exact_more) {
        for (int64_t j = r1_d ? 100 : 0; j < (int64_t)list.size(); ++j) {
            const unsigned long long key = list[j];
            uint32_t u = (uint32_t)(key >> 32);
            u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
            float d;
            std::memcpy(&d, &u, 4);
            put(id_base + (uint32_t)key, d);
        }
    }
    return m;
}

// the answers of a batch's queries, but for those the per-query path takes
void sbd_emit_all(int nq, const std::vector<int>& legacy, const SbdRound1& r1, const float* targets, int64_t max_limit,
                  const std::vector<std::vector<unsigned long long>>& lists, uint64_t id_base, uint64_t* out_ids,
                  float* out_dists, int64_t out_cap, int64_t* out_n) {
    std::vector<char> is_legacy(nq, 0);
    for (int q : legacy) is_legacy[q] = 1;
    for (int q = 0; q < nq; ++q) {
        if (is_legacy[q]) continue;
        out_n[q] = sbd_emit(r1.ids_of(q), r1.d_of(q), r1.n_of(q), targets[q], max_limit, lists[q], id_base,
                            out_ids + (size_t)q * out_cap, out_dists + (size_t)q * out_cap, out_cap);
    }
}
}  // namespace

extern "C" {

int wv_search_by_vector_distance_batch(wv_index* ix, const float* queries, int nq, const float* targets,
                                       int64_t max_limit, const uint64_t* allow_bits, uint64_t allow_nbits,
                                       uint64_t allow_stride_words, uint64_t* out_ids, float* out_dists,
                                       int64_t out_cap, int64_t* out_n) {
    if (check(ix) || nq < 0 || out_cap < 0 || (nq && (!queries || !targets || !out_n)) ||
        (out_cap && nq && (!out_ids || !out_dists)))
        return fail(WV_EINVAL, "wv_search_by_vector_distance_batch: bad argument");
    if (nq == 0) return WV_OK;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    const uint64_t words = (allow_nbits + 63) / 64;
    const uint64_t astride = allow_stride_words ? allow_stride_words : words;
    auto allow_of = [&](int q) { return allow_row(allow_bits, allow_stride_words, q); };
    std::vector<int> legacy;   // queries for the per-query path
    std::vector<int> hnsw_q;   // queries whose round 1 is an HNSW search
    SbdRound1 r1(nq);
    {
        std::lock_guard<std::mutex> g(ix->mu);
        ix->sbd_pass_q = ix->sbd_hnsw_q = 0;
        ix->sbd_legacy_q = (uint64_t)nq;
        if (ix->pq_on && !sbd_pq_enabled()) {
            for (int q = 0; q < nq; ++q) legacy.push_back(q);
        } else {
            const int ef = search_time_ef(ix->cfg, 100);
            const bool can_hnsw = ix->has_graph && ef <= wv::HNSW_EF_MAX;
            for (int q = 0; q < nq; ++q) {
                // allowList.Len() < flatSearchCutoff (search.go:74-78); no
                // list: a length never below the cutoff (and none counted
                // where the rule does not read it)
                uint64_t c = INT64_MAX;
                if (can_hnsw && allow_bits && !ix->cfg.forbid_flat) {
                    const uint64_t* a = allow_of(q);
                    c = 0;
                    for (uint64_t w = 0; w < words; ++w) c += (uint64_t)__builtin_popcountll(a[w]);
                }
                if (!flat_by_len(ix, can_hnsw, c)) {
                    r1.slot[q] = (int)hnsw_q.size();
                    hnsw_q.push_back(q);
                }
            }
        }
    }
    if ((int)legacy.size() < nq) {
        const int cap = sbd_cap();
        const int nh = (int)hnsw_q.size();
        std::vector<float> hq((size_t)std::max(nh, 1) * ix->dim);
        std::vector<uint64_t> hallow;
        for (int i = 0; i < nh; ++i)
            std::memcpy(hq.data() + (size_t)i * ix->dim, queries + (size_t)hnsw_q[i] * ix->dim, 4 * (size_t)ix->dim);
        if (allow_bits && allow_stride_words && nh) {
            hallow.resize((size_t)nh * astride);
            for (int i = 0; i < nh; ++i)
                std::memcpy(hallow.data() + (size_t)i * astride, allow_of(hnsw_q[i]), 8 * astride);
        }
        r1.resize(nh);
        std::vector<unsigned int> cnt(3 * (size_t)nq);
        std::vector<std::vector<unsigned long long>> lists(nq);
        {
            std::lock_guard<std::mutex> g(ix->mu);
            hipStream_t s = ix->stream;
            int rc = refresh_bitmaps(ix);
            if (rc) return rc;
            const uint64_t* dallow = nullptr;
            if (allow_bits) {
                const size_t ab = (allow_stride_words ? (size_t)nq : 1) * astride * 8;
                HIP_TRY(ix->allow_keep.ensure(ab));
                HIP_TRY(hipMemcpyAsync(ix->allow_keep.p, allow_bits, ab, hipMemcpyHostToDevice, s));
                dallow = ix->allow_keep.as<uint64_t>();
            }
            // every query's threshold pass (its queries staged first: round
            // 1's search restages q_in)
            const float* dq = nullptr;
            bool passed = false;
            auto launch_pass = [&]() -> int {
                int rc = stage_queries(ix, queries, nq, &dq, s);
                if (rc) return rc;
                HIP_TRY(ix->sbd_q.ensure((size_t)nq * ix->dpad * 4));
                HIP_TRY(hipMemcpyAsync(ix->sbd_q.p, dq, (size_t)nq * ix->dpad * 4, hipMemcpyDeviceToDevice, s));
                HIP_TRY(ix->sbd_t.ensure((size_t)nq * 4));
                HIP_TRY(hipMemcpyAsync(ix->sbd_t.p, targets, (size_t)nq * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(ix->sbd_keys.ensure((size_t)nq * cap * 8));
                HIP_TRY(ix->sbd_tmp.ensure((size_t)nq * cap * 8));
                HIP_TRY(ix->sbd_cnt.ensure((size_t)nq * 12));
                HIP_TRY(ix->sbd_off.ensure((size_t)nq * 8));
                HIP_TRY(hipMemsetAsync(ix->sbd_cnt.p, 0, (size_t)nq * 12, s));
                wv::SbdParams sp{};
                sbd_fill(ix, sp);
                sp.allow = dallow;
                sp.allow_nbits = allow_nbits;
                sp.allow_stride = allow_stride_words;
                sp.N = ix->n_rows;
                sp.nq = nq;
                // ~4 blocks per CU over the batch, whole 4-wave steps of 256 rows
                const uint64_t target_blocks = std::max<uint64_t>(1, (uint64_t)ix->n_cus * 4 / (uint64_t)nq);
                sp.rows_per_block = std::max<uint64_t>(4096, (sp.N + target_blocks - 1) / target_blocks);
                sp.rows_per_block = (sp.rows_per_block + 255) / 256 * 256;
                while ((sp.N + sp.rows_per_block - 1) / sp.rows_per_block > 65535) sp.rows_per_block *= 2;
                sp.cap = cap;
                if (ix->pq_on) {
                    wv::SbdPqParams pp{};
                    pp.pq = pq_params(ix);
                    pp.lut = sbd_pq_lut();
                    // A workgroup that builds the table reads ks * D centroid
                    // floats, 4 ks ds bytes a segment, against the m code bytes of
                    // each row: from 4 ks ds rows a block the table's traffic is at
                    // most the block's code traffic (and its ks * D multiply-adds
                    // at most a quarter of its rows' m gathers), so that is the
                    // floor where it exceeds 4096 (ks 256, ds 4: the same 4096).
                    const uint64_t lut_floor = 4 * (uint64_t)pp.pq.ks * (uint64_t)pp.pq.ds;
                    if (pp.lut != 0 && (uint64_t)pp.pq.m * pp.pq.ks * 4 <= (uint64_t)wv::SBD_PQ_LUT_BYTES_MAX &&
                        sp.rows_per_block < lut_floor) {
                        sp.rows_per_block = (lut_floor + 255) / 256 * 256;
                        while ((sp.N + sp.rows_per_block - 1) / sp.rows_per_block > 65535) sp.rows_per_block *= 2;
                    }
                    pp.s = sp;
                    HIP_TRY(wv_launch_sbd_pq_scan(&pp, s));
                } else {
                    HIP_TRY(wv_launch_sbd_scan(&sp, s));
                }
                HIP_TRY(wv_sbd_sort(ix->sbd_keys.as<unsigned long long>(), ix->sbd_tmp.as<unsigned long long>(),
                                    ix->sbd_cnt.as<unsigned int>(), nq, cap, ix->sbd_off.as<int>(), &ix->sbd_scr,
                                    &ix->sbd_scr_cap, s));
                passed = true;
                return WV_OK;
            };
            // round 1 of the HNSW queries: their SearchByVector(limit 100)
            auto launch_r1 = [&]() -> int {
                if (!nh) return WV_OK;
                int rc = stage_queries(ix, hq.data(), nh, &dq, s);
                if (rc) return rc;
                const uint64_t* dal = dallow;
                if (allow_bits && allow_stride_words) {
                    HIP_TRY(ix->g_allow.ensure(hallow.size() * 8));
                    HIP_TRY(hipMemcpyAsync(ix->g_allow.p, hallow.data(), hallow.size() * 8, hipMemcpyHostToDevice, s));
                    dal = ix->g_allow.as<uint64_t>();
                }
                HIP_TRY(ix->out_ids.ensure((size_t)nh * 100 * 8));
                HIP_TRY(ix->out_d.ensure((size_t)nh * 100 * 4));
                HIP_TRY(ix->out_n.ensure((size_t)nh * 4));
                const Batch b{dq, ix->dpad, nh, 100, dal, allow_nbits, allow_stride_words, ix->out_ids.as<uint64_t>(),
                              ix->out_d.as<float>(), ix->out_n.as<int32_t>(), s};
                rc = search_core(ix, b, 0, WV_MODE_AUTO);
                if (rc) return rc;
                HIP_TRY(hipMemcpyAsync(r1.ids.data(), ix->out_ids.p, (size_t)nh * 100 * 8, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(r1.d.data(), ix->out_d.p, (size_t)nh * 100 * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(r1.n.data(), ix->out_n.p, (size_t)nh * 4, hipMemcpyDeviceToHost, s));
                return WV_OK;
            };
            if (ix->pq_on && nq == 1 && nh == 1) {
                // One HNSW query on a compressed index: nothing to launch the
                // pass beside, so round 1 runs first and the pass only when
                // round 1 lets the deepening go on (cnt stays 0 otherwise).
                // Launched before it, the pass cost a call whose round 1 ends
                // the deepening 0.26 ms of 10 (profiles/sbd_pq/README.md).
                rc = launch_r1();
                if (rc) return rc;
                HIP_TRY(hipStreamSynchronize(s));
                if (sbd_r1_continues(r1.d.data(), std::min<int64_t>(100, r1.n[0]), targets[0], max_limit)) {
                    rc = launch_pass();
                    if (rc) return rc;
                }
            } else {
                rc = launch_pass();
                if (rc) return rc;
                rc = launch_r1();
                if (rc) return rc;
            }
            if (passed)
                HIP_TRY(hipMemcpyAsync(cnt.data(), ix->sbd_cnt.p, (size_t)nq * 12, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            // the sorted lists, as far as the rounds keep them (and the caller
            // takes them)
            std::vector<int64_t> need(nq, 0);
            for (int q = 0; q < nq; ++q) {
                need[q] = sbd_list_need(r1.d_of(q), r1.n_of(q), targets[q], max_limit, cnt.data() + 3 * (size_t)q);
                if ((int64_t)cnt[3 * q] > cap && need[q] > 0) { legacy.push_back(q); need[q] = 0; continue; }
                if (need[q] > 0) {
                    lists[q].resize(need[q]);
                    HIP_TRY(hipMemcpyAsync(lists[q].data(), ix->sbd_tmp.as<unsigned long long>() + (size_t)q * cap,
                                           8 * need[q], hipMemcpyDeviceToHost, s));
                }
            }
            HIP_TRY(hipStreamSynchronize(s));
            ix->sbd_legacy_q = legacy.size();
            ix->sbd_pass_q = (uint64_t)nq - legacy.size();
            ix->sbd_hnsw_q = (uint64_t)nh;
        }
        sbd_emit_all(nq, legacy, r1, targets, max_limit, lists, ix->cfg.id_base, out_ids, out_dists, out_cap, out_n);
    }
    for (int q : legacy) {
        int rc = wv_search_by_vector_distance(ix, queries + (size_t)q * ix->dim, targets[q], max_limit, allow_of(q),
                                              allow_nbits, out_cap ? out_ids + (size_t)q * out_cap : nullptr,
                                              out_cap ? out_dists + (size_t)q * out_cap : nullptr, out_cap, out_n + q);
        if (rc) return rc;
    }
    return WV_OK;
}

// wv_search_by_vector_distance_batch with one allow list per query, as ids.
// Every query's threshold pass walks its list (sbd_ids_kernel) into a segment
// of min(list length, WV_SBD_CAP) keys; the segments of a chunk of queries lie
// back to back and are sorted by one segmented sort, and a batch whose
// segments sum past WV_SBD_IDS_MAX_ENTRIES (2^26) runs in consecutive chunks
// of queries.  Flat or HNSW round 1 is decided from the list's length; the
// HNSW queries' bitmap rows are scattered on the device.  The host arithmetic
// is that of the bitmap route.
int wv_search_by_vector_distance_batch_ids(wv_index* ix, const float* queries, int nq, const float* targets,
                                           int64_t max_limit, const uint64_t* allow_ids,
                                           const uint64_t* allow_offsets, uint64_t* out_ids, float* out_dists,
                                           int64_t out_cap, int64_t* out_n) {
    const std::string fn = "wv_search_by_vector_distance_batch_ids";
    if (nq < 0) return fail(WV_EINVAL, fn + ": nq < 0");
    if (out_cap < 0) return fail(WV_EINVAL, fn + ": out_cap < 0");
    if (!allow_offsets) return fail(WV_EINVAL, fn + ": null allow_offsets");
    if (check(ix)) return fail(WV_EINVAL, fn + ": null index");
    if (nq && (!queries || !targets || !out_n)) return fail(WV_EINVAL, fn + ": null queries, targets or out_n");
    if (nq && out_cap && (!out_ids || !out_dists)) return fail(WV_EINVAL, fn + ": null outputs");
    if (int rc = ids_check_offsets(fn, allow_ids, allow_offsets, nq)) return rc;
    if (nq == 0) return WV_OK;
    const uint64_t total = allow_offsets[nq];
    const int cap = sbd_cap();
    uint64_t max_entries = 1ull << 26;   // (64-bit: its own parse)
    if (const char* e = std::getenv("WV_SBD_IDS_MAX_ENTRIES")) max_entries = std::strtoull(e, nullptr, 10);
    max_entries = std::min<uint64_t>(std::max<uint64_t>(max_entries, 1), 0x7FFFFFFFull);
    std::vector<int> legacy;   // queries for the per-query path
    std::vector<int> hnsw_q;   // queries whose round 1 is an HNSW search
    SbdRound1 r1(nq);
    std::vector<std::vector<unsigned long long>> lists(nq);
    uint64_t N = 0;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    {
        const size_t qb = (size_t)nq * ix->dim * 4, lb = (size_t)total * 4, fb = ((size_t)nq + 1) * 8,
                     tb = (size_t)nq * 4;
        PinLayout lay;
        lay.add(qb);   // (the queries, at 0)
        const size_t o_l = lay.add(lb), o_f = lay.add(fb), o_t = lay.add(tb);
        SlotLease lease(ix);
        wv_index::HostSlot& sl = *lease.sl;
        if (int rc = slot_reserve(sl, lay.need())) return rc;
        char* pin = static_cast<char*>(sl.pin);
        std::memcpy(pin, queries, qb);
        std::memcpy(pin + o_t, targets, tb);
        uint32_t* ids32 = reinterpret_cast<uint32_t*>(pin + o_l);
        uint64_t* off = reinterpret_cast<uint64_t*>(pin + o_f);
        if (int rc = ids_stage(fn, allow_ids, allow_offsets, nq, ids32, off)) return rc;
        std::lock_guard<std::mutex> g(ix->mu);
        HIP_TRY(hipSetDevice(ix->cfg.device));
        hipStream_t s = ix->stream;
        N = ix->n_rows;
        ix->sbd_ids_list_q = ix->sbd_ids_list_ids = ix->sbd_ids_hnsw_q = ix->sbd_ids_legacy_q = 0;
        if (ix->pq_on ? !sbd_pq_enabled() : ix->dpad > wv::FLAT_IDS_DPAD_MAX) {
            // the uncompressed kernel keeps the query row in LDS (the
            // compressed ones read it from memory): the per-query path
            for (int q = 0; q < nq; ++q) legacy.push_back(q);
        } else {
            int rc = refresh_bitmaps(ix);
            if (rc) return rc;
            // the queries staged, and kept beside round 1's searches
            const float* dq = nullptr;
            rc = stage_queries(ix, reinterpret_cast<const float*>(pin), nq, &dq, s);
            if (rc) return rc;
            HIP_TRY(ix->sbd_q.ensure((size_t)nq * ix->dpad * 4));
            HIP_TRY(hipMemcpyAsync(ix->sbd_q.p, dq, (size_t)nq * ix->dpad * 4, hipMemcpyDeviceToDevice, s));
            rc = ids_upload(ix, ids32, off, nq, s);
            if (rc) return rc;
            HIP_TRY(ix->sbd_t.ensure(tb));
            HIP_TRY(hipMemcpyAsync(ix->sbd_t.p, pin + o_t, tb, hipMemcpyHostToDevice, s));
            HIP_TRY(ix->sbd_cnt.ensure((size_t)nq * 12));
            HIP_TRY(hipMemsetAsync(ix->sbd_cnt.p, 0, (size_t)nq * 12, s));
            // flat or HNSW round 1, from the list's length (search.go:64-79)
            const bool can_hnsw = ix->has_graph && search_time_ef(ix->cfg, 100) <= wv::HNSW_EF_MAX;
            for (int q = 0; q < nq; ++q) {
                const uint64_t L = allow_offsets[q + 1] - allow_offsets[q];
                if (!flat_by_len(ix, can_hnsw, L)) {
                    r1.slot[q] = (int)hnsw_q.size();
                    hnsw_q.push_back(q);
                }
            }
            const int nh = (int)hnsw_q.size();
            r1.resize(nh);
            std::vector<unsigned int> cnt(3 * (size_t)nq);
            std::vector<int> segs;   // a chunk's segment starts, then their lengths
            std::vector<unsigned long long> sorted;   // a chunk's sorted keys, when one copy fetches them
            for (int q0 = 0; q0 < nq;) {
                // the chunk [q0, q1): segments back to back, at most max_entries keys
                segs.clear();
                uint64_t sum = 0, max_len = 0;
                int q1 = q0;
                for (; q1 < nq; ++q1) {
                    const uint64_t len = off[q1 + 1] - off[q1], seg = std::min<uint64_t>(len, (uint64_t)cap);
                    if (q1 > q0 && sum + seg > max_entries) break;
                    segs.push_back((int)sum);
                    sum += seg;
                    max_len = std::max(max_len, len);
                }
                const int nqc = q1 - q0, n_keys = (int)sum;
                for (int q = q0; q < q1; ++q) segs.push_back((int)std::min<uint64_t>(off[q + 1] - off[q], (uint64_t)cap));
                if (n_keys > 0) {
                    HIP_TRY(ix->sbd_seg.ensure((size_t)nqc * 12));
                    HIP_TRY(hipMemcpyAsync(ix->sbd_seg.p, segs.data(), (size_t)nqc * 8, hipMemcpyHostToDevice, s));
                    HIP_TRY(ix->sbd_keys.ensure((size_t)n_keys * 8));
                    HIP_TRY(ix->sbd_tmp.ensure((size_t)n_keys * 8));
                    uint64_t chunk_len = 0, nc = 0;
                    ids_chunks(ix, nqc, max_len, &chunk_len, &nc);
                    while (nc > 65535) {
                        chunk_len *= 2;
                        nc = (max_len + chunk_len - 1) / chunk_len;
                    }
                    wv::SbdIdsParams sp{};
                    sbd_fill(ix, sp);
                    sp.ids = ix->fi_ids.as<uint32_t>();
                    sp.off = ix->fi_off.as<uint64_t>();
                    sp.seg_beg = ix->sbd_seg.as<int>();
                    sp.seg_cap = ix->sbd_seg.as<int>() + nqc;
                    sp.n_rows = N;
                    sp.chunk_len = chunk_len;
                    sp.q0 = q0;
                    sp.nq = nqc;
                    sp.n_chunks = (int)nc;
                    if (ix->pq_on) {
                        wv::SbdPqIdsParams pp{};
                        pp.s = sp;
                        pp.pq = pq_params(ix);
                        pp.lut = sbd_pq_lut();
                        HIP_TRY(wv_launch_sbd_pq_ids(&pp, s));
                    } else {
                        HIP_TRY(wv_launch_sbd_ids(&sp, s));
                    }
                    HIP_TRY(wv_sbd_ids_sort(sp.keys, ix->sbd_tmp.as<unsigned long long>(), n_keys, sp.cnt, q0, nqc,
                                            sp.seg_beg, sp.seg_cap, ix->sbd_seg.as<int>() + 2 * nqc, &ix->sbd_scr,
                                            &ix->sbd_scr_cap, s));
                }
                if (q0 == 0 && nh) {
                    // round 1 of the HNSW queries, beside the first chunk's
                    // pass: their bitmap rows scattered from the ids into
                    // bounded scratch, then SearchByVector(limit 100)
                    HIP_TRY(ix->fi_sel.ensure((size_t)nh * 4));
                    HIP_TRY(hipMemcpyAsync(ix->fi_sel.p, hnsw_q.data(), (size_t)nh * 4, hipMemcpyHostToDevice, s));
                    auto keep_r1 = [&](size_t c0, int n, const int32_t*) -> int {
                        HIP_TRY(hipMemcpyAsync(r1.ids.data() + c0 * 100, ix->fi_oid.p, (size_t)n * 100 * 8,
                                               hipMemcpyDeviceToHost, s));
                        HIP_TRY(hipMemcpyAsync(r1.d.data() + c0 * 100, ix->fi_od.p, (size_t)n * 100 * 4,
                                               hipMemcpyDeviceToHost, s));
                        HIP_TRY(hipMemcpyAsync(r1.n.data() + c0, ix->fi_on.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
                        return WV_OK;
                    };
                    rc = ids_bitmap_route(ix, ix->sbd_q.as<float>(), hnsw_q.data(), ix->fi_sel.as<int32_t>(), (size_t)nh,
                                          100, 0, WV_MODE_HNSW, off, s, keep_r1);
                    if (rc) return rc;
                }
                HIP_TRY(hipMemcpyAsync(cnt.data() + 3 * (size_t)q0, ix->sbd_cnt.as<unsigned int>() + 3 * (size_t)q0,
                                       (size_t)nqc * 12, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                // the sorted lists, as far as the rounds keep them: the
                // segments lie back to back, so a chunk of short segments
                // comes over in one copy (a copy per query cost more than the
                // pass at 1024 queries), long ones each on its own
                int64_t span = 0;   // keys up to the last kept entry
                for (int q = q0; q < q1; ++q) {
                    const int64_t need =
                        sbd_list_need(r1.d_of(q), r1.n_of(q), targets[q], max_limit, cnt.data() + 3 * (size_t)q);
                    if (need <= 0) continue;
                    if ((int64_t)cnt[3 * (size_t)q] > segs[nqc + q - q0]) {
                        legacy.push_back(q);
                        continue;
                    }
                    lists[q].resize(need);
                    span = std::max<int64_t>(span, segs[q - q0] + need);
                }
                const bool one_copy = span * 8 <= (int64_t)(8 << 20);
                if (one_copy && span) {
                    sorted.resize(span);
                    HIP_TRY(hipMemcpyAsync(sorted.data(), ix->sbd_tmp.p, 8 * (size_t)span, hipMemcpyDeviceToHost, s));
                } else {
                    for (int q = q0; q < q1; ++q)
                        if (!lists[q].empty())
                            HIP_TRY(hipMemcpyAsync(lists[q].data(),
                                                   ix->sbd_tmp.as<unsigned long long>() + segs[q - q0],
                                                   8 * lists[q].size(), hipMemcpyDeviceToHost, s));
                }
                HIP_TRY(hipStreamSynchronize(s));
                if (one_copy)
                    for (int q = q0; q < q1; ++q)
                        if (!lists[q].empty())
                            std::memcpy(lists[q].data(), sorted.data() + segs[q - q0], 8 * lists[q].size());
                q0 = q1;
            }
            ix->sbd_ids_list_ids = total;
            ix->sbd_ids_hnsw_q = (uint64_t)nh;
        }
        ix->sbd_ids_legacy_q = legacy.size();
        ix->sbd_ids_list_q = (uint64_t)nq - legacy.size();
    }
    sbd_emit_all(nq, legacy, r1, targets, max_limit, lists, ix->cfg.id_base, out_ids, out_dists, out_cap, out_n);
    // the per-query path, over a bitmap row built for the query alone
    const uint64_t nbits = std::max<uint64_t>(N, 1);
    std::vector<uint64_t> row;
    for (int q : legacy) {
        row.assign((nbits + 63) / 64, 0);
        for (uint64_t i = allow_offsets[q]; i < allow_offsets[q + 1] && allow_ids[i] < N; ++i)
            row[allow_ids[i] >> 6] |= 1ull << (allow_ids[i] & 63);
        int rc = wv_search_by_vector_distance(ix, queries + (size_t)q * ix->dim, targets[q], max_limit, row.data(), nbits,
                                              out_cap ? out_ids + (size_t)q * out_cap : nullptr,
                                              out_cap ? out_dists + (size_t)q * out_cap : nullptr, out_cap, out_n + q);
        if (rc) return rc;
    }
    return WV_OK;
}

int wv_last_sbd_ids_stats(wv_index* ix, uint64_t* list_queries, uint64_t* list_ids, uint64_t* hnsw_round1_queries,
                          uint64_t* legacy_queries) {
    if (check(ix)) return fail(WV_EINVAL, "wv_last_sbd_ids_stats: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    if (list_queries) *list_queries = ix->sbd_ids_list_q;
    if (list_ids) *list_ids = ix->sbd_ids_list_ids;
    if (hnsw_round1_queries) *hnsw_round1_queries = ix->sbd_ids_hnsw_q;
    if (legacy_queries) *legacy_queries = ix->sbd_ids_legacy_q;
    return WV_OK;
}

int wv_last_sbd_stats(wv_index* ix, uint64_t* pass_queries, uint64_t* hnsw_round1_queries, uint64_t* legacy_queries) {
    if (check(ix)) return fail(WV_EINVAL, "wv_last_sbd_stats: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    if (pass_queries) *pass_queries = ix->sbd_pass_q;
    if (hnsw_round1_queries) *hnsw_round1_queries = ix->sbd_hnsw_q;
    if (legacy_queries) *legacy_queries = ix->sbd_legacy_q;
    return WV_OK;
}

int wv_search_by_vector_distance(wv_index* ix, const float* vector, float target, int64_t max_limit,
                                 const uint64_t* allow_bits, uint64_t allow_nbits, uint64_t* out_ids,
                                 float* out_dists, int64_t out_cap, int64_t* out_n) {
    if (check(ix) || !vector || !out_n) return fail(WV_EINVAL, "bad argument");
    // search.go:90-158 with searchByDistParams (:552-619)
    int64_t offset = 0, limit = 100, total = 100, n_out = 0;
    std::vector<uint64_t> ids;
    std::vector<float> ds;
    std::vector<int32_t> nn(1);
    for (bool first = true;; first = false) {
        if (!first) {
            offset = total;
            limit *= 10;
            total = offset + limit;
            if (max_limit >= 0 && total > max_limit) break;
        }
        if (total > (int64_t)0x7FFFFFFF) break;
        ids.assign(total, 0);
        ds.assign(total, 0.f);
        int rc = wv_search_by_vector(ix, vector, (int)total, allow_bits, allow_nbits, ids.data(), ds.data(), nn.data());
        if (rc) return rc;
        const int64_t n = nn[0];
        const int64_t lo = std::min(offset, n), hi = std::min(total, n);
        if (hi - lo <= 0) break;
        const bool cont = ds[hi - 1] <= target;
        for (int64_t i = lo; i < hi; ++i) {
            if (ds[i] <= target || std::fabs((double)ds[i] - (double)target) <= 1e-6) {
                if (n_out < out_cap) { out_ids[n_out] = ids[i]; out_dists[n_out] = ds[i]; }
                n_out++;
            } else {
                break;
            }
        }
        if (!cont) break;
    }
    *out_n = n_out;
    return WV_OK;
}

}  // extern "C"
