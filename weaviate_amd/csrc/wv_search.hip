// wv_search.hip -- the dispatch behind every search of the C ABI and its batch
// entry points (wv_search_batch, _ids, _device, wv_search_by_vector).
// search_core dispatches SearchByVector the way the reference does
// (search.go:64-79) to the pipelines of wv_search_exact.hip (flatSearch) and
// wv_search_hnsw.hip (the graph).  No CPU search code: every distance and
// every selection happens on the GPU.
#include <cstring>
#include <thread>

#include "wv_search.h"

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

}  // namespace

namespace wv_host {

hipError_t launch_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int D, float* dst, int ld_dst,
                              hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(128), 0, s, src, ld_src, idx, n, D, dst, ld_dst);
    return hipGetLastError();
}

int count_allow_rows(wv_index* ix, const Batch& b, uint64_t words, std::vector<unsigned long long>* out) {
    const int rows = b.allow_rows();
    HIP_TRY(ix->g_cnt.ensure((size_t)rows * 8));
    HIP_TRY(hipMemsetAsync(ix->g_cnt.p, 0, (size_t)rows * 8, b.s));
    hipLaunchKernelGGL(popcount_rows_kernel, dim3(rows), dim3(256), 0, b.s, b.allow, words,
                       b.allow_stride ? b.allow_stride : words, rows, ix->g_cnt.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    out->resize(rows);
    HIP_TRY(hipMemcpyAsync(out->data(), ix->g_cnt.p, 8 * (size_t)rows, hipMemcpyDeviceToHost, b.s));
    HIP_TRY(hipStreamSynchronize(b.s));
    return WV_OK;
}

// Core: device queries already padded to dpad and normalized (cosine).
int search_core(wv_index* ix, const Batch& b, int ef, int mode) {
    int rc = refresh_bitmaps(ix);
    if (rc) return rc;
    hipStream_t s = b.s;
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
    if (ef <= 0) ef = search_time_ef(ix->cfg, b.k);
    if (mode == WV_MODE_EXACT) return run_exact(ix, b);
    if (mode == WV_MODE_HNSW) return ef > wv::HNSW_EF_MAX ? run_exact(ix, b) : run_hnsw_delta(ix, b, ef);
    // AUTO: search.go:74-78
    const bool can_hnsw = ix->has_graph && ef <= wv::HNSW_EF_MAX;
    if (!b.allow || ix->cfg.forbid_flat) return can_hnsw ? run_hnsw_delta(ix, b, ef) : run_exact(ix, b);
    // allowList.Len() < flatSearchCutoff decides per query
    std::vector<unsigned long long> cnt;
    if (int rc2 = count_allow_rows(ix, b, (b.allow_nbits + 63) / 64, &cnt)) return rc2;
    std::vector<int32_t> flat, knn;
    for (int q = 0; q < b.nq; ++q) (flat_by_len(ix, can_hnsw, cnt[b.allow_stride ? q : 0]) ? flat : knn).push_back(q);
    if (knn.empty()) return run_exact(ix, b);
    if (flat.empty()) return run_hnsw_delta(ix, b, ef);
    // split the batch: gather each group, run, scatter back
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<int32_t>& sel = pass == 0 ? flat : knn;
        const int n = (int)sel.size();
        HIP_TRY(ix->g_idx.ensure((size_t)n * 4));
        HIP_TRY(ix->g_q.ensure((size_t)n * b.ldq * 4));
        HIP_TRY(ix->g_ids.ensure((size_t)n * b.k * 8));
        HIP_TRY(ix->g_d.ensure((size_t)n * b.k * 4));
        HIP_TRY(ix->g_n.ensure((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(ix->g_idx.p, sel.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_gather_rows(b.q, b.ldq, ix->g_idx.as<int32_t>(), n, b.ldq, ix->g_q.as<float>(), b.ldq, s));
        Batch g = b.with_outputs(ix->g_ids.as<uint64_t>(), ix->g_d.as<float>(), ix->g_n.as<int32_t>());
        g.q = ix->g_q.as<float>();
        g.nq = n;
        if (b.allow_stride) {
            HIP_TRY(ix->g_allow.ensure((size_t)n * b.allow_stride * 8));
            hipLaunchKernelGGL(gather_words_kernel, dim3(n), dim3(256), 0, s, b.allow, b.allow_stride,
                               ix->g_idx.as<int32_t>(), n, ix->g_allow.as<uint64_t>());
            g.allow = ix->g_allow.as<uint64_t>();
        }
        HIP_TRY(hipGetLastError());
        if (int rc2 = pass == 0 ? run_exact(ix, g) : run_hnsw_delta(ix, g, ef)) return rc2;
        hipLaunchKernelGGL(scatter_results_kernel, dim3(n), dim3(64), 0, s, g.out_ids, g.out_d, g.out_n,
                           ix->g_idx.as<int32_t>(), n, b.k, b.out_ids, b.out_d, b.out_n);
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
static int flat_ids_pq_lut() { return env_tri("WV_FLAT_IDS_PQ_LUT"); }
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
    if (const char* e = std::getenv("WV_FLAT_IDS_PQ_CHUNK")) floor = (uint64_t)std::max(0ll, std::atoll(e));   // (64-bit: its own parse)
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

int results_to_host(wv_index* ix, wv_index::HostSlot& sl, const size_t* o, int nq, int k, hipStream_t s) {
    char* pin = static_cast<char*>(sl.pin);
    HIP_TRY(hipMemcpyAsync(pin + o[0], ix->out_ids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(pin + o[1], ix->out_d.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(pin + o[2], ix->out_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(sl.done, s));
    return WV_OK;
}

int results_deliver(wv_index::HostSlot& sl, const size_t* o, int nq, int k, uint64_t* out_ids, float* out_dists,
                    int32_t* out_n) {
    const char* pin = static_cast<const char*>(sl.pin);
    HIP_TRY(hipEventSynchronize(sl.done));
    copy_results(pin + o[0], pin + o[1], pin + o[2], nq, k, out_ids, out_dists, out_n);
    return WV_OK;
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
    const size_t qb = (size_t)nq * ix->dim * 4, ab = arows * astride * 8, ib = (size_t)nq * k * 8,
                 db = (size_t)nq * k * 4, nb = (size_t)nq * 4;
    PinLayout lay;
    lay.add(qb);   // (the queries, at 0)
    const size_t o_a = lay.add(ab), o_res[3] = {lay.add(ib), lay.add(db), lay.add(nb)};
    HIP_TRY(hipSetDevice(ix->cfg.device));
    SlotLease lease(ix);
    wv_index::HostSlot& sl = *lease.sl;
    if (int rc = slot_reserve(sl, lay.need())) return rc;
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
        const Batch b{dq, ix->dpad, nq, k, dallow, allow_nbits, allow_stride_words, ix->out_ids.as<uint64_t>(),
                      ix->out_d.as<float>(), ix->out_n.as<int32_t>(), s};
        rc = search_core(ix, b, ef, mode);
        if (rc) return rc;
        rc = results_to_host(ix, sl, o_res, nq, k, s);
        if (rc) return rc;
    }
    // the index is free for the next batch while this one finishes
    return results_deliver(sl, o_res, nq, k, out_ids, out_dists, out_n);
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
    const size_t qb = (size_t)nq * ix->dim * 4, lb = (size_t)total * 4, fb = ((size_t)nq + 1) * 8,
                 ib = (size_t)nq * k * 8, db = (size_t)nq * k * 4, nb = (size_t)nq * 4;
    PinLayout lay;
    lay.add(qb);   // (the queries, at 0)
    const size_t o_l = lay.add(lb), o_f = lay.add(fb), o_res[3] = {lay.add(ib), lay.add(db), lay.add(nb)};
    HIP_TRY(hipSetDevice(ix->cfg.device));
    SlotLease lease(ix);
    wv_index::HostSlot& sl = *lease.sl;
    if (int rc = slot_reserve(sl, lay.need())) return rc;
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
            else flat = flat_by_len(ix, can_hnsw, L);
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
        auto scatter = [&](size_t, int n, const int32_t* d_sel) -> int {
            hipLaunchKernelGGL(scatter_results_kernel, dim3(n), dim3(64), 0, s, ix->fi_oid.as<uint64_t>(),
                               ix->fi_od.as<float>(), ix->fi_on.as<int32_t>(), d_sel, n, k,
                               ix->out_ids.as<uint64_t>(), ix->out_d.as<float>(), ix->out_n.as<int32_t>());
            HIP_TRY(hipGetLastError());
            return WV_OK;
        };
        size_t base = sel[0].size();
        for (int grp = 1; grp <= 2; ++grp) {
            rc = ids_bitmap_route(ix, dq, sel[grp].data(), ix->fi_sel.as<int32_t>() + base, sel[grp].size(), k, ef,
                                  grp == 1 ? WV_MODE_EXACT : WV_MODE_HNSW, off, s, scatter);
            if (rc) return rc;
            base += sel[grp].size();
        }
        rc = results_to_host(ix, sl, o_res, nq, k, s);
        if (rc) return rc;
    }
    return results_deliver(sl, o_res, nq, k, out_ids, out_dists, out_n);
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
    const Batch b{dq, ix->dpad, nq, k, d_allow_bits, allow_nbits, allow_stride_words, d_out_ids, d_out_dists, d_out_n, s};
    rc = search_core(ix, b, ef, mode);
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
