// wv_search.h -- what the search host files share (wv_search.hip,
// wv_search_exact.hip, wv_search_hnsw.hip, wv_distance.hip): the batch
// descriptor every pipeline takes and the declarations that cross files.
// Internal, like wv_index.h: hidden visibility.
#pragma once
#include "wv_index.h"
#include "wv_launch.h"

#pragma GCC visibility push(hidden)

namespace wv_host {

// row q of an allow list: one shared row where stride is 0, else a row of
// stride words per query; null without a list (device or host memory)
inline const uint64_t* allow_row(const uint64_t* allow, uint64_t stride, int q) {
    return allow ? allow + (stride ? (uint64_t)q * stride : 0) : nullptr;
}

// One batch of prepared queries on the device: rows of ldq floats (padded,
// normalized for cosine), an optional allow list (one shared row, or one row
// of allow_stride words per query), the outputs ([nq][k], [nq][k], [nq]) and
// the stream.  An aggregate: a sub-batch is asked for, not computed.
struct Batch {
    const float* q;
    int ldq, nq, k;
    const uint64_t* allow;
    uint64_t allow_nbits, allow_stride;
    uint64_t* out_ids;
    float* out_d;
    int32_t* out_n;
    hipStream_t s;

    const uint64_t* allow_row(int i) const { return wv_host::allow_row(allow, allow_stride, i); }
    int allow_rows() const { return allow && allow_stride ? nq : 1; }
    // queries [c0, c0 + n) with their allow rows and output rows
    Batch slice(int c0, int n) const {
        return Batch{q + (size_t)c0 * ldq, ldq, n, k, allow_row(c0), allow_nbits, allow_stride,
                     out_ids + (size_t)c0 * k, out_d + (size_t)c0 * k, out_n + c0, s};
    }
    // query i alone, its allow row as a shared list
    Batch one(int i) const { return slice(i, 1).with_allow(allow_row(i), allow_nbits, 0); }
    Batch with_allow(const uint64_t* a, uint64_t nbits, uint64_t stride) const {
        return Batch{q, ldq, nq, k, a, nbits, stride, out_ids, out_d, out_n, s};
    }
    Batch with_outputs(uint64_t* ids, float* d, int32_t* n) const {
        return Batch{q, ldq, nq, k, allow, allow_nbits, allow_stride, ids, d, n, s};
    }
    // no rows to search: every query's count is 0
    hipError_t zero_counts() const { return hipMemsetAsync(out_n, 0, sizeof(int32_t) * nq, s); }
};

// The flat-or-HNSW rule of search.go:64-79 for an allow list of len ids.  One
// form covers every caller: where forbid_flat is set the length is not read,
// so a caller that has dealt with forbid_flat before counting (search_core)
// gets `len < cutoff || !can_hnsw`, which is this with forbid_flat false.
inline bool flat_by_len(const wv_index* ix, bool can_hnsw, uint64_t len) {
    return !can_hnsw || (!ix->cfg.forbid_flat && (int64_t)len < ix->cfg.flat_search_cutoff);
}

// offsets into a pinned slot: each part starts on a 256-byte boundary
struct PinLayout {
    size_t end = 0;
    size_t add(size_t bytes) { const size_t o = end; end += (bytes + 255) & ~(size_t)255; return o; }
    size_t need() const { return end; }
};

// wv_search_exact.hip: flatSearch -- the key passes, their fallback, the PQ scan
int run_exact(wv_index* ix, const Batch& b, const uint64_t* d_rowmask = nullptr, uint64_t rowmask_nbits = 0);
int queue_fbd(wv_index* ix, const Batch& b);
// each query (pick null) or each query with pick[q] != 0 by a full scan and
// sort of its own; counted in ix->last_fallbacks
int exact_each(wv_index* ix, const Batch& b, const int32_t* pick);

// wv_search_hnsw.hip: the graph search, beside an exact pass over the delta set
int choose_vc_log2(int per_wave_budget_words, int fixed_words, uint64_t n_nodes, int* tbits);
int run_hnsw_delta(wv_index* ix, const Batch& b, int ef);

// wv_search.hip: the dispatch, the pinned slots, per-query allow lists given as ids
int search_core(wv_index* ix, const Batch& b, int ef, int mode);
// out[r] = set bits in the first `words` words of allow row r (allow_rows() of them), read back
int count_allow_rows(wv_index* ix, const Batch& b, uint64_t words, std::vector<unsigned long long>* out);
int stage_queries(wv_index* ix, const float* q, int nq, const float** d_out, hipStream_t s);
// dst[r] = src[idx[r]] for n rows (zero past D), one 128-thread workgroup per row
hipError_t launch_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int D, float* dst, int ld_dst,
                              hipStream_t s);
int slot_reserve(wv_index::HostSlot& sl, size_t need);
// a batch's results (ix->out_*) into the slot at the offsets o = {ids, dists, counts}: queued, then the
// slot's event ...
int results_to_host(wv_index* ix, wv_index::HostSlot& sl, const size_t* o, int nq, int k, hipStream_t s);
// ... and, once the event has passed, from the slot to the caller's arrays
int results_deliver(wv_index::HostSlot& sl, const size_t* o, int nq, int k, uint64_t* out_ids, float* out_dists,
                    int32_t* out_n);
int ids_check_offsets(const std::string& fn, const uint64_t* allow_ids, const uint64_t* allow_offsets, int nq);
int ids_stage(const std::string& fn, const uint64_t* allow_ids, const uint64_t* allow_offsets, int nq, uint32_t* ids32,
              uint64_t* off);
int ids_upload(wv_index* ix, const uint32_t* ids32, const uint64_t* off, int nq, hipStream_t s);
void ids_chunks(const wv_index* ix, int ns, uint64_t max_len, uint64_t* chunk_len, uint64_t* n_chunks);
// The id lists' bitmap route for the n_sel queries sel (host; d_sel: the same
// on the device) of d_src: in chunks of bounded scratch, the queries gathered,
// their bitmap rows scattered from the uploaded lists (off: the host offsets),
// search_core over them, then after(c0, n, d_sel + c0) -> int takes the
// chunk's results from fi_oid / fi_od / fi_on
template <class After>
int ids_bitmap_route(wv_index* ix, const float* d_src, const int32_t* sel, const int32_t* d_sel, size_t n_sel, int k,
                     int ef, int mode, const uint64_t* off, hipStream_t s, After&& after) {
    const uint64_t N = ix->n_rows;
    const uint64_t words = std::max<uint64_t>(1, (N + 63) / 64);
    const size_t rows_cap = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(65535, (1ull << 30) / (words * 8)));
    for (size_t c0 = 0; c0 < n_sel; c0 += rows_cap) {
        const int n = (int)std::min(rows_cap, n_sel - c0);
        uint64_t max_len = 0;
        for (int i = 0; i < n; ++i) max_len = std::max(max_len, off[sel[c0 + i] + 1] - off[sel[c0 + i]]);
        HIP_TRY(ix->fi_q.ensure((size_t)n * ix->dpad * 4));
        HIP_TRY(ix->fi_bits.ensure((size_t)n * words * 8));
        HIP_TRY(ix->fi_oid.ensure((size_t)n * k * 8));
        HIP_TRY(ix->fi_od.ensure((size_t)n * k * 4));
        HIP_TRY(ix->fi_on.ensure((size_t)n * 4));
        HIP_TRY(launch_gather_rows(d_src, ix->dpad, d_sel + c0, n, ix->dpad, ix->fi_q.as<float>(), ix->dpad, s));
        HIP_TRY(hipMemsetAsync(ix->fi_bits.p, 0, (size_t)n * words * 8, s));
        HIP_TRY(wv_launch_ids_to_bits(ix->fi_ids.as<uint32_t>(), ix->fi_off.as<uint64_t>(), d_sel + c0, n, max_len, N,
                                      words, ix->fi_bits.as<uint64_t>(), s));
        const Batch b{ix->fi_q.as<float>(), ix->dpad, n, k, ix->fi_bits.as<uint64_t>(), std::max<uint64_t>(N, 1), words,
                      ix->fi_oid.as<uint64_t>(), ix->fi_od.as<float>(), ix->fi_on.as<int32_t>(), s};
        if (int rc = search_core(ix, b, ef, mode)) return rc;
        if (int rc = after(c0, n, d_sel + c0)) return rc;
    }
    return WV_OK;
}

}  // namespace wv_host

#pragma GCC visibility pop
