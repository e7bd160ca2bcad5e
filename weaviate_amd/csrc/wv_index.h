// wv_index.h -- what the host files of the C ABI share (wv_api.hip,
// wv_search*.hip, wv_distance.hip, wv_build.hip): the index itself and the
// helpers that more than one of them calls (the search files' own: wv_search.h).
// Internal: all of it has hidden visibility, the library exports
// include/wvgpu.h only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wvgpu.h"
#include "wv_params.h"

#pragma GCC visibility push(hidden)

namespace wv_host {
// sets the calling thread's wv_last_error() message; returns code
int fail(int code, const std::string& msg);
}  // namespace wv_host

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return wv_host::fail(_e == hipErrorOutOfMemory ? WV_EOOM : WV_EDEVICE,             \
                                 std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)
// record timing event i of the current batch's set (wv_index::ev)
#define TREC(i)                                                                     \
    do {                                                                            \
        if (ix->timing && ix->ev) {                                                 \
            HIP_TRY(hipEventRecord(ix->ev[i], s));                                  \
            ix->ev_mask[ix->ev_used - 1] |= (uint8_t)(1u << (i));                   \
        }                                                                           \
    } while (0)

namespace wv_host {

// growable device scratch buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        // batches may still be queued that read the old buffer (several in
        // flight on the index's stream, wv_search_batch): drain the device
        // before it goes
        size_t want = std::max<size_t>(bytes, 256);
        // scratch that grows with the batch: geometric steps (bounded), so a
        // stream of growing batches does not reallocate -- and drain -- each time
        if (cap) want = std::max(want, std::min(cap + cap / 2, bytes + ((size_t)256 << 20)));
        if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); }
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// rows of the corpus buffers: whole 128-row tiles of the brute-force passes
// and whole 256-row tiles of the wide f16 pass (wv_bf_h16w_kernel<.., 128>)
inline uint64_t align_rows(uint64_t n) { return (n + 255) / 256 * 256; }

// Environment switches.  Read per call: tests flip them between calls of one
// process.  env_on: set at all (NAME=0 counts as set); env_int: atoi of the
// value, at least min, or, when unset, dflt as given -- min is not applied to
// it, so a dflt of 0 under a min >= 1 tells "unset" apart (WV_H16_SAMPLE,
// WV_HNSW_SIDE_ROWS, WV_HNSW_SPILL_CAP); env_tri: 0 / 1, or -1 when unset or
// empty.
inline bool env_on(const char* name) { return std::getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt, int min = INT_MIN) {
    const char* e = std::getenv(name);
    return e ? std::max(min, std::atoi(e)) : dflt;
}
inline double env_double(const char* name, double dflt) {
    const char* e = std::getenv(name);
    return e ? std::atof(e) : dflt;
}
inline int env_tri(const char* name) {
    const char* e = std::getenv(name);
    return e && *e ? (std::atoi(e) ? 1 : 0) : -1;
}

}  // namespace wv_host

using wv_host::DevBuf;

struct wv_index {
    int dim = 0, dpad = 0, metric = 0;
    int ldx = 0;            // corpus row stride: D rounded up to 32 floats (whole 128-B lines, whole MFMA k-chunks) when D >= 32
    wv_config cfg{};
    uint64_t capacity = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // corpus
    DevBuf vecs;            // [capacity rounded to 128][ldx]
    // bf16 hi/lo image of vecs for the brute-force key pass (same bytes, in
    // the MFMA-native layout of split_hi_index), kept in step with every row write
    DevBuf xsplit;
    bool use_split = false;
    // f16 image of vecs for the f16 key pass (wv_h16.hip, the default for
    // D <= 128): f16(s_x x) in the layout of h16_index; h16_ex = max residual
    // norm |x - f16(s_x x) / s_x| over the rows (rounded up), both host-cached
    bool use_h16 = false;
    bool h16_wide = false;  // D > 128: wv_bf_h16w_kernel (both operands through LDS, 256-row tiles)
    int h16_ns = 0;
    float h16_sx = 0.f, h16_ex = 0.f;
    DevBuf ximg16, xns, qimg16, qres, qmax, qscale, tau, gtau, marg, allow_pad, ex_bits, gslot;
    // the f16 pass's block order (block_order), cached for its schedule
    DevBuf blk_order;
    std::vector<int> blk_order_host;
    uint64_t blk_key[4] = {0, 0, 0, 0};
    DevBuf qmax_part;       // per-block max |q_i| of the query-norm pass
    float maxnorm_host = 0.f;   // max |x| (rounded up), cached after every row write
    DevBuf xnorm;           // [capacity]
    DevBuf maxnorm;         // unsigned bits of max |x|
    std::vector<uint64_t> has_vec;   // host copy of uploaded rows
    uint64_t n_rows = 0;    // highest uploaded id + 1
    // graph
    bool has_graph = false;
    uint64_t gn = 0;
    int deg0 = 0, degU = 0, max_level = 0;
    uint64_t n_upper = 0, entrypoint = 0;
    std::vector<uint64_t> nil_host;   // graph nil nodes and ids >= gn, one bit per id
    DevBuf levels, layer0, upper_row, upper;
    // bitmaps
    std::vector<uint64_t> tomb_host;
    bool any_tomb = false, any_nil = false;   // any tombstone / nil node below gn
    uint64_t n_tomb = 0;                      // tombstones (sizes the side-register path's state)
    int last_side_rows = 0, last_side_xs = 0;  // the last side-register launch's LDS rows / spill capacity
    DevBuf side_vb, side_sp;                   // its visited bitmaps and spills (HBM scratch)
    DevBuf tomb;            // tombstones (HNSW eligibility)
    DevBuf excl;            // tombstone | nil node | no vector (flatSearch skips)
    uint64_t bm_words = 0;
    uint64_t clean_words = 0;   // leading exclusion words that are zero (refresh_bitmaps)
    bool bitmaps_dirty = true;
    // scratch
    DevBuf stage;           // contiguous host->device staging
    DevBuf q_in, q_norm, q_nrm2, q_scaled, cand_d, cand_id, fail, status, counters;
    // SearchByVectorDistance batches (wv_sbd.hip): targets, lists, counts, sort scratch
    DevBuf sbd_t, sbd_keys, sbd_tmp, sbd_cnt, sbd_off, sbd_q;
    DevBuf sbd_seg;         // (the id-list route) a chunk's segment starts, lengths and ends
    uint64_t sbd_ids_list_q = 0, sbd_ids_list_ids = 0, sbd_ids_hnsw_q = 0, sbd_ids_legacy_q = 0;   // the last call's routes
    uint64_t sbd_pass_q = 0, sbd_hnsw_q = 0, sbd_legacy_q = 0;   // the same of the last bitmap-route batch
    void* sbd_scr = nullptr;
    size_t sbd_scr_cap = 0;
    DevBuf scan_d, scan_i, sort_d, sort_i, sort_tmp;
    DevBuf g_idx, g_q, g_allow, g_ids, g_d, g_n, g_cnt;
    DevBuf out_ids, out_d, out_n;
    DevBuf fail_thr;
    DevBuf ac_cnt, ac_off, rowidx;   // allow-list compaction
    // mutable-index sync: rows added since the last graph
    // upload are "pending"; those the graph does not hold are the delta set,
    // searched exactly beside the graph
    std::vector<uint64_t> pending_host;
    uint64_t delta_count = 0;
    DevBuf delta, dmask, dl_ids, dl_d, dl_n, dq_tmp;
    // graph construction scratch
    DevBuf b_tgt, b_ci, b_cd, b_cn, b_cnt0, b_cntu, b_rk, b_rn, b_rk2, b_rn2, b_uk, b_ul, b_uo, b_nr, b_tmp;
    // product quantization: h.pq / h.compressed
    // (compress.go:39-89).  Codes live on the device as u8 (ks <= 256) or u16
    // per segment, rows padded to whole words; has_code marks rows encoded.
    int pq_m = 0, pq_ks = 0, pq_ds = 0, pq_encoder = 0;
    bool pq_set = false, pq_on = false, pq_use_bits = false;
    bool pq_list_search = false;   // wv_index_set_pq_list_search: flat queries of wv_search_batch_ids walk their lists
    uint64_t pq_stride = 0;
    std::vector<uint64_t> has_code;
    DevBuf pq_cent, pq_codes;
    DevBuf pk_key, pk_dist, pk_val, pk_skey, pk_sval, pk_off;
    // stats of the last batch: host-side counts plus device accumulators
    // (stat_acc: distance evaluations, expansions, device-resolved
    // fallbacks), read -- after a sync -- only when the stats are asked for
    uint64_t last_dist = 0, last_exp = 0, last_fallbacks = 0;
    DevBuf stat_acc;
    hipStream_t stat_stream = nullptr;
    // device-resolved certificate fallback (wv_launch_fbd): failed-query list
    // and count, survivors, overflow flags, full-scan slots
    DevBuf fbd_list, fbd_nf, fbd_over, fbd_cd, fbd_ci, fbd_cn, fbd_scr;
    // ordering of work on a caller's stream (wv_search_batch_device) against
    // the index's own stream: the call waits for ix->stream, and ix->stream
    // then waits for the call, so the scratch and state buffers the call reads
    // are never rewritten by a later call while it is still queued
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipEvent_t ev_null = nullptr;   // a NULL-stream call: the legacy default stream's work so far
    // optional kernel timing (hipEvents on the launch stream): each batch
    // records into its own event set (pairs 0-1 key pass, 2-3 finalize, 4-5
    // HNSW, 6-7 seed pass); the sets are read -- after a sync -- only when the
    // times are asked for, so timing adds no host round trip per batch
    bool timing = false;
    hipEvent_t* ev = nullptr;                    // the current batch's set
    std::vector<std::array<hipEvent_t, 8>> ev_pool;
    std::vector<uint8_t> ev_mask;                // pairs recorded per set
    size_t ev_used = 0;                          // sets recorded since the last read
    float t_mfma = 0.f, t_fin = 0.f, t_hnsw = 0.f, t_pre = 0.f;
    int n_cus = 256;
    // brute-force workgroups per launch: a whole number of resident waves of
    // workgroups (CUs x 2 per CU x WV_BF_ROUNDS)
    int bf_blocks = 512;
    // host staging of wv_search_batch: pinned slots, so a batch's copies are
    // asynchronous and the index mutex is released before the caller waits --
    // the next batch (another batcher worker) is staged and queued while this
    // one runs, and the GPU does not idle between batches
    struct HostSlot {
        void* pin = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    std::mutex slot_mu;
    std::condition_variable slot_cv;
    std::array<HostSlot, 3> slots;
    DevBuf allow_keep;   // per-query allow lists of an AUTO batch (the dispatch gathers into g_allow)
    // f16 key pass over a compacted shared allow list: the rows' image,
    // their |x|^2 and the scan's exclusion bits (the last tile's padding)
    DevBuf cimg16, cxnorm, cexcl;
    // wv_search_batch_ids: the lists (u32 ids, offsets), the rows of each
    // route, the sparse kernel's per-chunk keys, and the bitmap route's
    // gathered queries, bitmap rows and results
    DevBuf fi_ids, fi_off, fi_sel, fi_part, fi_q, fi_bits, fi_oid, fi_od, fi_on;
    uint64_t fi_sparse_q = 0, fi_sparse_ids = 0, fi_bitmap_q = 0;   // the last call's routes
    hipEvent_t fi_ev[2] = {nullptr, nullptr};                       // the sparse kernel (timing on)
    bool fi_timed = false;
};

namespace wv_host {

// one pinned staging slot of wv_search_batch, returned when the call ends
struct SlotLease {
    wv_index* ix;
    wv_index::HostSlot* sl = nullptr;
    explicit SlotLease(wv_index* x) : ix(x) {
        std::unique_lock<std::mutex> l(ix->slot_mu);
        ix->slot_cv.wait(l, [&] {
            for (auto& c : ix->slots)
                if (!c.busy) return true;
            return false;
        });
        for (auto& c : ix->slots)
            if (!c.busy) { sl = &c; break; }
        sl->busy = true;
    }
    ~SlotLease() {
        std::lock_guard<std::mutex> l(ix->slot_mu);
        sl->busy = false;
        ix->slot_cv.notify_one();
    }
};

// wv_api.hip: state, configuration and row buffers
int check(wv_index* ix);
int refresh_bitmaps(wv_index* ix);
int search_time_ef(const wv_config& c, int k);
wv::PqParams pq_params(const wv_index* ix);
hipError_t launch_pad_rows(const float* src, uint64_t ld_src, uint64_t n, int D, float* dst, int ld_dst, hipStream_t s);
// out[q] = the first k of n_shards sorted lists merged by (dist, id); 128 queries per workgroup
hipError_t launch_merge_shards(const float* in_d, const uint64_t* in_ids, const int32_t* in_n, int n_shards, int nq,
                               int k, float* out_d, uint64_t* out_ids, int32_t* out_n, hipStream_t s);

}  // namespace wv_host

#pragma GCC visibility pop
