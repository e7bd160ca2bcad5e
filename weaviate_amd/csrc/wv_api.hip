// wv_api.hip -- host side of the C ABI declared in include/wvgpu.h: one index
// and its device memory (vectors, norms, CSR graph, bitmaps).  Error state,
// configuration, create/destroy, row upload and add, tombstones and the delta
// set, capacity growth, product-quantizer setup, timing and stats.  Searches:
// wv_search.hip (with wv_search_exact.hip, wv_search_hnsw.hip),
// wv_distance.hip; graph construction: wv_build.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "wv_index.h"
#include "wv_launch.h"

using namespace wv_host;

namespace {

thread_local std::string g_err;

// copy rows [n][ld_src] into the padded layout [n][ld_dst], zero-filling D..ld_dst
__global__ void pad_rows_kernel(const float* src, uint64_t ld_src, uint64_t n, int D, float* dst, int ld_dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t r = i / ld_dst;
    const int c = (int)(i % ld_dst);
    if (r >= n) return;
    dst[r * ld_dst + c] = c < D ? src[r * ld_src + c] : 0.f;
}

__global__ void merge_shards_kernel(const float* in_d, const uint64_t* in_ids, const int32_t* in_n, int n_shards,
                                    int nq, int k, float* out_d, uint64_t* out_ids, int32_t* out_n) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int head[16];
    for (int s = 0; s < n_shards; ++s) head[s] = 0;
    int n = 0;
    for (; n < k; ++n) {
        int best = -1;
        float bd = 0.f;
        uint64_t bi = 0;
        for (int s = 0; s < n_shards; ++s) {
            const int cnt = in_n[(size_t)s * nq + q];
            if (head[s] >= cnt) continue;
            const size_t off = ((size_t)s * nq + q) * k + head[s];
            const float d = in_d[off];
            const uint64_t id = in_ids[off];
            if (best < 0 || d < bd || (d == bd && id < bi)) { best = s; bd = d; bi = id; }
        }
        if (best < 0) break;
        head[best]++;
        out_d[(size_t)q * k + n] = bd;
        out_ids[(size_t)q * k + n] = bi;
    }
    out_n[q] = n;
}

}  // namespace

namespace wv_host {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int check(wv_index* ix) {
    if (!ix) return fail(WV_EINVAL, "null index");
    return WV_OK;
}

hipError_t launch_pad_rows(const float* src, uint64_t ld_src, uint64_t n, int D, float* dst, int ld_dst, hipStream_t s) {
    const uint64_t total = n * (uint64_t)ld_dst;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, ld_src, n, D, dst,
                       ld_dst);
    return hipGetLastError();
}

hipError_t launch_merge_shards(const float* in_d, const uint64_t* in_ids, const int32_t* in_n, int n_shards, int nq,
                               int k, float* out_d, uint64_t* out_ids, int32_t* out_n, hipStream_t s) {
    hipLaunchKernelGGL(merge_shards_kernel, dim3((nq + 127) / 128), dim3(128), 0, s, in_d, in_ids, in_n, n_shards, nq, k,
                       out_d, out_ids, out_n);
    return hipGetLastError();
}

int refresh_bitmaps(wv_index* ix) {
    if (!ix->bitmaps_dirty) return WV_OK;
    const uint64_t words = ix->bm_words;
    std::vector<uint64_t> ex(words, 0);
    for (uint64_t w = 0; w < words; ++w) {
        uint64_t v = ~ix->has_vec[w];
        // compressed: a node whose code is missing is skipped like a deleted
        // one (distanceToByteNode, search.go:403-418)
        if (ix->pq_on) v |= ~ix->has_code[w];
        if (w < ix->tomb_host.size()) v |= ix->tomb_host[w];
        ex[w] = v;
    }
    std::vector<uint64_t> dl(words, 0);
    uint64_t dcount = 0;
    if (ix->has_graph) {
        // a nil node is skipped by flatSearch (flat_search.go:29-40) unless
        // it was added after the graph snapshot: then it is live (delta)
        for (uint64_t w = 0; w < words; ++w) {
            const uint64_t nil = ix->nil_host[w], pend = ix->pending_host[w];
            dl[w] = nil & pend & ix->has_vec[w] & ~ex[w];
            ex[w] |= nil & ~pend;
            dcount += (uint64_t)__builtin_popcountll(dl[w]);
        }
    }
    ix->delta_count = dcount;
    // the clean prefix: words (64-row tiles of the f16 pass) before the first
    // excluded row, which the key pass need not test
    ix->clean_words = 0;
    while (ix->clean_words < words && ex[ix->clean_words] == 0) ix->clean_words++;
    if (dcount) {
        HIP_TRY(ix->delta.ensure(words * 8));
        HIP_TRY(hipMemcpyAsync(ix->delta.p, dl.data(), words * 8, hipMemcpyHostToDevice, ix->stream));
    }
    std::vector<uint64_t> tb(words, 0);
    for (uint64_t w = 0; w < words && w < ix->tomb_host.size(); ++w) tb[w] = ix->tomb_host[w];
    HIP_TRY(hipMemcpyAsync(ix->excl.p, ex.data(), words * 8, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->tomb.p, tb.data(), words * 8, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->bitmaps_dirty = false;
    return WV_OK;
}

int search_time_ef(const wv_config& c, int k) {
    int ef = (int)c.ef;
    if (ef < 1) {
        ef = k * (int)c.dynamic_ef_factor;
        if (ef > (int)c.dynamic_ef_max) ef = (int)c.dynamic_ef_max;
        else if (ef < (int)c.dynamic_ef_min) ef = (int)c.dynamic_ef_min;
        if (k > ef) ef = k;
        return ef;
    }
    if (ef < k) ef = k;
    return ef;
}

wv::PqParams pq_params(const wv_index* ix) {
    wv::PqParams pq{};
    pq.codes = ix->pq_codes.as<uint8_t>();
    pq.cent = ix->pq_cent.as<float>();
    pq.stride = ix->pq_stride;
    pq.m = ix->pq_m;
    pq.ks = ix->pq_ks;
    pq.ds = ix->pq_ds;
    pq.wide = ix->pq_ks > 256;
    return pq;
}

// Re-home a capacity-sized device buffer at new_bytes: the first old_bytes
// copied, the rest zeroed (an unused buffer stays unallocated).
static hipError_t regrow(DevBuf& b, size_t old_bytes, size_t new_bytes, hipStream_t s) {
    if (!b.p || new_bytes <= b.cap) return hipSuccess;
    void* np = nullptr;
    hipError_t e = hipMalloc(&np, new_bytes);
    if (e != hipSuccess) return e;
    old_bytes = std::min(old_bytes, b.cap);
    if (old_bytes) e = hipMemcpyAsync(np, b.p, old_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<char*>(np) + old_bytes, 0, new_bytes - old_bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(np); return e; }
    (void)hipFree(b.p);
    b.p = np;
    b.cap = new_bytes;
    return hipSuccess;
}

}  // namespace wv_host

extern "C" {

void wv_config_default(wv_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->device = 0;
    c->max_connections = 64;
    c->ef = -1;
    c->dynamic_ef_min = 100;
    c->dynamic_ef_max = 500;
    c->dynamic_ef_factor = 8;
    c->flat_search_cutoff = 40000;
    c->forbid_flat = 0;
    c->id_base = 0;
}

const char* wv_last_error(void) { return g_err.c_str(); }
// for wv_batcher.cpp: a request's error is reported on its caller's thread
void wv_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }
const char* wv_version(void) { return "wvgpu 0.1 (gfx950)"; }

int wv_index_create(int dim, int metric, const wv_config* cfg, uint64_t capacity, wv_index** out) {
    if (!out || dim <= 0 || metric < 0 || metric > 2 || capacity == 0 || capacity >= (1ull << 31))
        return fail(WV_EINVAL, "wv_index_create: bad argument");
    auto* ix = new wv_index();
    ix->dim = dim;
    ix->dpad = (dim + 3) & ~3;
    ix->ldx = dim >= 32 ? (dim + 31) & ~31 : ix->dpad;
    ix->metric = metric;
    if (cfg) ix->cfg = *cfg; else wv_config_default(&ix->cfg);
    ix->capacity = capacity;
    hipError_t e = hipSetDevice(ix->cfg.device);
    if (e != hipSuccess) { delete ix; return fail(WV_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e)); }
    e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ix; return fail(WV_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->cfg.device) != hipSuccess || cus <= 0)
            cus = 256;
        ix->bf_blocks = cus * 2;
        ix->n_cus = cus;
    }
    ix->bm_words = (capacity + 63) / 64;
    // whole brute-force tiles (wv_bf.hip layout contract) and whole 256-row
    // tiles of the wide f16 pass: zero rows past capacity
    const uint64_t cap_rows = align_rows(capacity);
    const size_t vbytes = cap_rows * (size_t)ix->ldx * 4;
    if (ix->vecs.ensure(vbytes) != hipSuccess || ix->xnorm.ensure(cap_rows * 4) != hipSuccess ||
        ix->maxnorm.ensure(4) != hipSuccess || ix->tomb.ensure(ix->bm_words * 8) != hipSuccess ||
        ix->excl.ensure((ix->bm_words + 4) * 8) != hipSuccess) {   // + the words of a last 256-row tile
        wv_index_destroy(ix);
        return fail(WV_EOOM, "wv_index_create: device allocation failed");
    }
    // bf16x3 key pass (wv_bf_split_kernel): whole 32-float chunks, stride <= 128
    // (the query block image stays resident in LDS); WV_BF_FP32=1 keeps the
    // fp32 MFMA pass for every scan
    // f16 key pass (wv_bf_h16_kernel) for D <= 128 unless an ablation switch
    // asks for the bf16x3 (WV_BF_SPLIT=1) or the fp32 (WV_BF_FP32=1) pass
    ix->use_h16 = dim <= 16 * wv::HW_NS_MAX && !std::getenv("WV_BF_FP32") && !std::getenv("WV_BF_SPLIT");
    if (ix->use_h16) {
        // D > 128: the wide-D kernel, whose chunks are HW_KC 16-k steps
        ix->h16_wide = dim > 16 * wv::H_NS_MAX;
        ix->h16_ns = ix->h16_wide ? (dim + 16 * wv::HW_KC - 1) / (16 * wv::HW_KC) * wv::HW_KC : (dim + 15) / 16;
        const size_t ibytes = cap_rows * (size_t)ix->h16_ns * 16 * 2;
        if (ix->ximg16.ensure(ibytes) != hipSuccess || ix->xns.ensure(cap_rows * 4) != hipSuccess ||
            ix->ex_bits.ensure(4) != hipSuccess || ix->qmax.ensure(4) != hipSuccess ||
            ix->qscale.ensure(4) != hipSuccess) {
            wv_index_destroy(ix);
            return fail(WV_EOOM, "wv_index_create: device allocation failed");
        }
        (void)hipMemsetAsync(ix->ximg16.p, 0, ibytes, ix->stream);
        (void)hipMemsetAsync(ix->xns.p, 0, cap_rows * 4, ix->stream);
        (void)hipMemsetAsync(ix->ex_bits.p, 0, 4, ix->stream);
    }
    ix->use_split = !ix->use_h16 && ix->ldx % wv::BF_BK == 0 && ix->ldx <= 128 && !std::getenv("WV_BF_FP32");
    if (ix->use_split && ix->xsplit.ensure(vbytes) != hipSuccess) {
        wv_index_destroy(ix);
        return fail(WV_EOOM, "wv_index_create: device allocation failed");
    }
    if (ix->use_split) (void)hipMemsetAsync(ix->xsplit.p, 0, vbytes, ix->stream);
    (void)hipMemsetAsync(ix->vecs.p, 0, vbytes, ix->stream);
    (void)hipMemsetAsync(ix->xnorm.p, 0, cap_rows * 4, ix->stream);
    (void)hipMemsetAsync(ix->maxnorm.p, 0, 4, ix->stream);
    (void)hipStreamSynchronize(ix->stream);
    ix->has_vec.assign(ix->bm_words, 0);
    ix->tomb_host.assign(ix->bm_words, 0);
    ix->pending_host.assign(ix->bm_words, 0);
    *out = ix;
    return WV_OK;
}

int wv_index_destroy(wv_index* ix) {
    if (!ix) return WV_OK;
    (void)hipSetDevice(ix->cfg.device);
    for (DevBuf* b : {&ix->vecs, &ix->xsplit, &ix->xnorm, &ix->maxnorm, &ix->levels, &ix->layer0, &ix->upper_row, &ix->upper,
                      &ix->tomb, &ix->excl, &ix->q_in, &ix->q_norm, &ix->q_nrm2, &ix->q_scaled, &ix->cand_d, &ix->cand_id,
                      &ix->fail, &ix->status, &ix->counters, &ix->scan_d, &ix->scan_i, &ix->sort_d, &ix->sort_i,
                      &ix->sort_tmp, &ix->g_idx, &ix->g_q, &ix->g_allow, &ix->g_ids, &ix->g_d, &ix->g_n, &ix->g_cnt,
                      &ix->out_ids, &ix->out_d, &ix->out_n, &ix->stage, &ix->fail_thr,
                      &ix->ac_cnt, &ix->ac_off, &ix->rowidx, &ix->pq_cent, &ix->pq_codes, &ix->pk_key,
                      &ix->pk_dist, &ix->pk_val, &ix->pk_skey, &ix->pk_sval, &ix->pk_off, &ix->ximg16, &ix->qmax_part, &ix->xns,
                      &ix->qimg16, &ix->qres, &ix->qmax, &ix->qscale, &ix->tau, &ix->gtau, &ix->marg, &ix->allow_pad, &ix->ex_bits, &ix->gslot, &ix->blk_order,
                      &ix->delta, &ix->dmask, &ix->dl_ids, &ix->dl_d, &ix->dl_n, &ix->dq_tmp, &ix->b_tgt, &ix->b_ci,
                      &ix->b_cd, &ix->b_cn, &ix->b_cnt0, &ix->b_cntu, &ix->b_rk, &ix->b_rn, &ix->b_rk2, &ix->b_rn2,
                      &ix->b_uk, &ix->b_ul, &ix->b_uo, &ix->b_nr, &ix->b_tmp, &ix->stat_acc, &ix->fbd_list,
                      &ix->fbd_nf, &ix->fbd_over, &ix->fbd_cd, &ix->fbd_ci, &ix->fbd_cn, &ix->fbd_scr})
        b->release();
    if (ix->stream) (void)hipStreamSynchronize(ix->stream);
    ix->allow_keep.release();
    for (DevBuf* b : {&ix->sbd_t, &ix->sbd_keys, &ix->sbd_tmp, &ix->sbd_cnt, &ix->sbd_off, &ix->sbd_q, &ix->sbd_seg})
        b->release();
    if (ix->sbd_scr) (void)hipFree(ix->sbd_scr);
    ix->sbd_scr = nullptr;
    ix->cimg16.release();
    ix->cxnorm.release();
    ix->cexcl.release();
    for (DevBuf* b : {&ix->fi_ids, &ix->fi_off, &ix->fi_sel, &ix->fi_part, &ix->fi_q, &ix->fi_bits, &ix->fi_oid,
                      &ix->fi_od, &ix->fi_on})
        b->release();
    for (auto e : ix->fi_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& sl : ix->slots) {
        if (sl.pin) (void)hipHostFree(sl.pin);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (auto& set : ix->ev_pool)
        for (auto e : set)
            if (e) (void)hipEventDestroy(e);
    if (ix->ev_in) (void)hipEventDestroy(ix->ev_in);
    if (ix->ev_out) (void)hipEventDestroy(ix->ev_out);
    if (ix->ev_null) (void)hipEventDestroy(ix->ev_null);
    if (ix->stream) (void)hipStreamDestroy(ix->stream);
    delete ix;
    return WV_OK;
}

int wv_index_update_config(wv_index* ix, const wv_config* cfg) {
    if (check(ix) || !cfg) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    const int dev = ix->cfg.device;
    const uint64_t base = ix->cfg.id_base;
    ix->cfg = *cfg;
    ix->cfg.device = dev;   // the device and id base are fixed at creation
    ix->cfg.id_base = base;
    return WV_OK;
}

// After rows were written to vecs (rownorm updated maxnorm; the stream is
// synchronised): cache max |x| on the host (the finalize's eps needs it, and
// reading it per batch would cost a host round trip), and keep the f16 image
// in step.  s_x is fixed by the first write and only ever lowered (then the
// whole image is rebuilt) so that no element overflows f16.
static int rows_written(wv_index* ix, const uint64_t* d_ids, uint64_t n, uint64_t first_id) {
    unsigned int mb = 0;
    HIP_TRY(hipMemcpyAsync(&mb, ix->maxnorm.p, 4, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    std::memcpy(&ix->maxnorm_host, &mb, 4);
    if (!ix->use_h16 || n == 0) return WV_OK;
    const float sx = wv_h16_pow2_scale(ix->maxnorm_host);
    const bool rebuild = ix->h16_sx != 0.f && sx < ix->h16_sx;
    if (ix->h16_sx == 0.f || rebuild) ix->h16_sx = sx;
    unsigned int* exb = ix->ex_bits.as<unsigned int>();
    if (rebuild) HIP_TRY(hipMemsetAsync(exb, 0, 4, ix->stream));
    {
        void* img = ix->ximg16.p;
        const int wide_layout = ix->h16_wide ? 1 : 0;   // (the wide-D kernel's h16w_index image)
        if (rebuild) {
            HIP_TRY(wv_launch_h16_rows(ix->vecs.as<float>(), ix->ldx, nullptr, ix->n_rows, ix->dim, ix->h16_ns, 1.f,
                                       ix->h16_sx, nullptr, img, 0, exb, nullptr, wide_layout, ix->stream));
        } else if (d_ids) {
            HIP_TRY(wv_launch_h16_rows(ix->vecs.as<float>(), ix->ldx, d_ids, n, ix->dim, ix->h16_ns, 1.f, ix->h16_sx,
                                       nullptr, img, 0, exb, nullptr, wide_layout, ix->stream));
        } else {
            HIP_TRY(wv_launch_h16_rows(ix->vecs.as<float>() + first_id * ix->ldx, ix->ldx, nullptr, n, ix->dim,
                                       ix->h16_ns, 1.f, ix->h16_sx, nullptr, img, first_id, exb, nullptr, wide_layout,
                                       ix->stream));
        }
    }
    unsigned int eb = 0;
    HIP_TRY(hipMemcpyAsync(&eb, exb, 4, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    std::memcpy(&ix->h16_ex, &eb, 4);
    return WV_OK;
}

// Rows written while a quantizer is set: with KMeans encoders the device
// encodes them as hnsw.Add does on a compressed index (insert.go:91-95,
// 166-170); codes of other encoders come from the host, so the rows are
// unsearchable on a compressed index until wv_index_upload_pq_codes.
static int pq_rows_written(wv_index* ix, const uint64_t* d_ids, const uint64_t* ids, uint64_t n, uint64_t first_id) {
    if (!ix->pq_set || n == 0) return WV_OK;
    if (ix->pq_encoder == WV_PQ_KMEANS) {
        wv::PqParams pq = pq_params(ix);
        if (d_ids) {
            HIP_TRY(wv_launch_pq_encode(ix->vecs.as<float>(), ix->ldx, d_ids, n, &pq, ix->pq_codes.as<uint8_t>(),
                                        ix->stream));
        } else {
            HIP_TRY(wv_launch_pq_encode(ix->vecs.as<float>() + first_id * ix->ldx, ix->ldx, nullptr, n, &pq,
                                        ix->pq_codes.as<uint8_t>() + first_id * ix->pq_stride, ix->stream));
        }
        HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t id = ids ? ids[i] : first_id + i;
        if (ix->pq_encoder == WV_PQ_KMEANS) ix->has_code[id >> 6] |= 1ull << (id & 63);
        else ix->has_code[id >> 6] &= ~(1ull << (id & 63));
    }
    ix->bitmaps_dirty = true;
    return WV_OK;
}

static int upload_rows(wv_index* ix, const float* src, bool device_src, int ld, uint64_t n, uint64_t first_id) {
    if (first_id + n > ix->capacity) return fail(WV_EINVAL, "upload beyond capacity");
    if (n == 0) return WV_OK;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    float* dst = ix->vecs.as<float>() + first_id * ix->ldx;
    const float* dsrc = src;
    if (!device_src) {
        HIP_TRY(ix->stage.ensure(n * (size_t)ix->dim * 4));
        HIP_TRY(hipMemcpyAsync(ix->stage.p, src, n * (size_t)ix->dim * 4, hipMemcpyHostToDevice, ix->stream));
        dsrc = ix->stage.as<float>();
        ld = ix->dim;
    }
    HIP_TRY(launch_pad_rows(dsrc, ld, n, ix->dim, dst, ix->ldx, ix->stream));
    if (ix->metric == WV_COSINE_DOT)  // normalize on write (insert.go:56-60, vector_cache.go:110-112)
        HIP_TRY(wv_launch_normalize(dst, dst, n, ix->dim, ix->ldx, ix->stream));
    HIP_TRY(wv_launch_rownorm(dst, n, ix->dim, ix->ldx, ix->xnorm.as<float>() + first_id,
                              ix->maxnorm.as<unsigned int>(), ix->stream));
    if (ix->use_split)
        HIP_TRY(wv_launch_split_rows(dst, ix->ldx, nullptr, n, n, ix->dim, 1.f, ix->xsplit.p, ix->ldx, first_id,
                                     ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (uint64_t i = first_id; i < first_id + n; ++i) ix->has_vec[i >> 6] |= 1ull << (i & 63);
    ix->n_rows = std::max(ix->n_rows, first_id + n);
    ix->bitmaps_dirty = true;
    int rc = rows_written(ix, nullptr, n, first_id);
    if (rc) return rc;
    return pq_rows_written(ix, nullptr, nullptr, n, first_id);
}

int wv_index_upload_vectors(wv_index* ix, const float* rows, uint64_t n, uint64_t first_id) {
    if (check(ix) || (!rows && n)) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    return upload_rows(ix, rows, false, ix->dim, n, first_id);
}

int wv_index_upload_vectors_device(wv_index* ix, const float* d_rows, uint64_t n, uint64_t first_id, int ld) {
    if (check(ix) || (!d_rows && n) || ld < ix->dim) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    return upload_rows(ix, d_rows, true, ld, n, first_id);
}

int wv_index_set_tombstones(wv_index* ix, const uint64_t* bits, uint64_t nbits) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    std::fill(ix->tomb_host.begin(), ix->tomb_host.end(), 0);
    const uint64_t w = std::min<uint64_t>((nbits + 63) / 64, ix->bm_words);
    for (uint64_t i = 0; i < w; ++i) ix->tomb_host[i] = bits ? bits[i] : 0;
    if (nbits & 63 && w == (nbits + 63) / 64 && w > 0) ix->tomb_host[w - 1] &= (1ull << (nbits & 63)) - 1;
    ix->n_tomb = 0;
    for (uint64_t i = 0; i < ix->bm_words; ++i) ix->n_tomb += (uint64_t)__builtin_popcountll(ix->tomb_host[i]);
    ix->any_tomb = ix->n_tomb > 0;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

__global__ void scatter_rows_kernel(const float* src, int ld_src, const uint64_t* ids, uint64_t n, int ldx,
                                    float* X, const float* norms, float* xnorm) {
    const uint64_t r = blockIdx.x;
    if (r >= n) return;
    const uint64_t id = ids[r];
    for (int i = threadIdx.x; i < ldx; i += blockDim.x) X[id * ldx + i] = src[r * (uint64_t)ld_src + i];
    if (threadIdx.x == 0) xnorm[id] = norms[r];
}

int wv_index_add(wv_index* ix, const uint64_t* ids_in, const float* rows_in, uint64_t n_in) {
    if (check(ix) || (n_in && (!ids_in || !rows_in))) return fail(WV_EINVAL, "wv_index_add: bad argument");
    if (n_in == 0) return WV_OK;
    for (uint64_t i = 0; i < n_in; ++i)
        if (ids_in[i] >= ix->capacity) return fail(WV_EINVAL, "wv_index_add: id beyond capacity");
    // The reference applies Adds one after another, so the last write of a
    // repeated id wins (insert.go:43-65).  One scatter block per distinct id:
    // two blocks writing one row would leave a mix of both rows, and its |x|^2
    // (which the finalize certificate relies on) from either.
    std::vector<uint64_t> ids_v;
    std::vector<float> rows_v;
    const uint64_t* ids = ids_in;
    const float* rows = rows_in;
    uint64_t n = n_in;
    {
        std::vector<uint64_t> sorted(ids_in, ids_in + n_in);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            std::vector<uint64_t> last_pos;   // positions of the last occurrence, in input order
            std::vector<uint8_t> seen(ix->bm_words * 64, 0);
            for (uint64_t i = n_in; i-- > 0;)
                if (!seen[ids_in[i]]) { seen[ids_in[i]] = 1; last_pos.push_back(i); }
            std::reverse(last_pos.begin(), last_pos.end());
            ids_v.resize(last_pos.size());
            rows_v.resize(last_pos.size() * (size_t)ix->dim);
            for (size_t j = 0; j < last_pos.size(); ++j) {
                ids_v[j] = ids_in[last_pos[j]];
                std::memcpy(rows_v.data() + j * ix->dim, rows_in + last_pos[j] * ix->dim, ix->dim * sizeof(float));
            }
            ids = ids_v.data();
            rows = rows_v.data();
            n = ids_v.size();
        }
    }
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    // rows -> [n][ldx] padded (normalized for cosine, insert.go:56-60), their
    // |x|^2, then scattered to their ids
    HIP_TRY(ix->stage.ensure(n * (size_t)ix->dim * 4));
    HIP_TRY(ix->dq_tmp.ensure(n * (size_t)ix->ldx * 4 + (n + (n & 1)) * 4 + n * 8));   // (the ids start 8-aligned)
    float* tmp = ix->dq_tmp.as<float>();
    float* nrm = tmp + n * (size_t)ix->ldx;
    uint64_t* d_ids = reinterpret_cast<uint64_t*>(nrm + n + (n & 1));
    HIP_TRY(hipMemcpyAsync(ix->stage.p, rows, n * (size_t)ix->dim * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_ids, ids, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_pad_rows(ix->stage.as<float>(), ix->dim, n, ix->dim, tmp, ix->ldx, s));
    if (ix->metric == WV_COSINE_DOT) HIP_TRY(wv_launch_normalize(tmp, tmp, n, ix->dim, ix->ldx, s));
    HIP_TRY(wv_launch_rownorm(tmp, n, ix->dim, ix->ldx, nrm, ix->maxnorm.as<unsigned int>(), s));
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)n), dim3(128), 0, s, tmp, ix->ldx, d_ids, n, ix->ldx,
                       ix->vecs.as<float>(), nrm, ix->xnorm.as<float>());
    HIP_TRY(hipGetLastError());
    if (ix->use_split)
        HIP_TRY(wv_launch_split_rows(ix->vecs.as<float>(), ix->ldx, d_ids, n, n, ix->dim, 1.f, ix->xsplit.p, ix->ldx, 0,
                                     s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t id = ids[i];
        ix->has_vec[id >> 6] |= 1ull << (id & 63);
        ix->pending_host[id >> 6] |= 1ull << (id & 63);
        ix->n_rows = std::max(ix->n_rows, id + 1);
    }
    ix->bitmaps_dirty = true;
    int rc = rows_written(ix, d_ids, n, 0);
    if (rc) return rc;
    return pq_rows_written(ix, d_ids, ids, n, 0);
}

static int edit_tombstones(wv_index* ix, const uint64_t* ids, uint64_t n, bool add) {
    if (check(ix) || (n && !ids)) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    for (uint64_t i = 0; i < n; ++i) {
        if (ids[i] >= ix->capacity) return fail(WV_EINVAL, "tombstone id beyond capacity");
        const uint64_t bit = 1ull << (ids[i] & 63);
        uint64_t& w = ix->tomb_host[ids[i] >> 6];
        if (add && !(w & bit)) { w |= bit; ix->n_tomb++; }
        else if (!add && (w & bit)) { w &= ~bit; ix->n_tomb--; }
    }
    ix->any_tomb = ix->n_tomb > 0;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_add_tombstones(wv_index* ix, const uint64_t* ids, uint64_t n) { return edit_tombstones(ix, ids, n, true); }
int wv_index_remove_tombstones(wv_index* ix, const uint64_t* ids, uint64_t n) {
    return edit_tombstones(ix, ids, n, false);
}

int wv_index_delta_size(wv_index* ix, uint64_t* n) {
    if (check(ix) || !n) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    int rc = refresh_bitmaps(ix);
    if (rc) return rc;
    *n = ix->delta_count;
    return WV_OK;
}

// Capacity growth in place (the mirror of a shard that outgrew its
// allocation; hnsw grows its node array the same way,
// maintainance.go:31-100 growIndexToAccomodateNode): every row, image, norm, code, tombstone and the
// graph stay; the queued work is drained first.
int wv_index_reserve(wv_index* ix, uint64_t capacity) {
    if (check(ix) || capacity >= (1ull << 31)) return fail(WV_EINVAL, "wv_index_reserve: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (capacity <= ix->capacity) return WV_OK;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t old_rows = align_rows(ix->capacity);
    const uint64_t cap_rows = align_rows(capacity);
    const size_t ld4 = (size_t)ix->ldx * 4, img = (size_t)ix->h16_ns * 16 * 2;
    const uint64_t words = (capacity + 63) / 64;
    HIP_TRY(regrow(ix->vecs, old_rows * ld4, cap_rows * ld4, s));
    HIP_TRY(regrow(ix->xsplit, old_rows * ld4, cap_rows * ld4, s));
    HIP_TRY(regrow(ix->xnorm, old_rows * 4, cap_rows * 4, s));
    HIP_TRY(regrow(ix->xns, old_rows * 4, cap_rows * 4, s));
    HIP_TRY(regrow(ix->ximg16, old_rows * img, cap_rows * img, s));
    HIP_TRY(regrow(ix->pq_codes, ix->capacity * ix->pq_stride, capacity * ix->pq_stride, s));
    // bitmaps are rewritten from the host copies by the next refresh
    HIP_TRY(ix->tomb.ensure(words * 8));
    HIP_TRY(ix->excl.ensure((words + 4) * 8));
    ix->has_vec.resize(words, 0);
    ix->tomb_host.resize(words, 0);
    ix->pending_host.resize(words, 0);
    if (!ix->has_code.empty()) ix->has_code.resize(words, 0);
    if (!ix->nil_host.empty()) ix->nil_host.resize(words, ~0ull);
    ix->capacity = capacity;
    ix->bm_words = words;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_capacity(const wv_index* ix, uint64_t* capacity, uint64_t* n_rows) {
    if (!ix) return fail(WV_EINVAL, "null index");
    if (capacity) *capacity = ix->capacity;
    if (n_rows) *n_rows = ix->n_rows;
    return WV_OK;
}

// ---- product quantization ---------------------------------
namespace {
// NewProductQuantizer (ssdhelpers/product_quantization.go:116-179) and
// ExtractCode (:191-237), read on the host: bits = int(log2 ks), bytes =
// int(log2(ks-1))/8 + 1; whole-byte codes are big-endian `bytes`-wide fields,
// bit-packed ones (useBitsEncoding, bits < 8*bytes) are cut from the
// (bytes+1)-byte big-endian word at index*bits/8.
struct CodeLayout {
    int bits = 0, bytes = 0;
    bool packed = false;
    bool init(int ks, bool use_bits) {
        if (ks < 2 || ks > 65536) return false;
        bits = (int)std::floor(std::log2((double)ks));
        bytes = (int)std::floor(std::log2((double)(ks - 1))) / 8 + 1;
        packed = use_bits && bits != 8 * bytes;
        return true;
    }
    static uint64_t be(const uint8_t* p, int nb) {
        uint64_t v = 0;
        for (int i = 0; i < nb; ++i) v = (v << 8) | p[i];
        return v;
    }
    uint64_t get(const uint8_t* enc, int index) const {
        if (!packed) return be(enc + (size_t)index * bytes, bytes);
        uint64_t code = be(enc + (size_t)index * bits / 8, bytes + 1);
        const int rest = (index + 1) * bits % 8, from_start = index * bits % 8;
        code >>= from_start < rest ? 16 - rest : 8 - rest;
        return code & ((1ull << bits) - 1);
    }
};
}  // namespace

int wv_pq_code_len(int segments, int centroids, int use_bits_encoding) {
    CodeLayout L;
    if (segments <= 0 || !L.init(centroids, use_bits_encoding != 0)) return -1;
    return segments * L.bytes;   // ProductQuantizer.Encode allocates m * bytes (:348-354)
}

int wv_index_set_pq(wv_index* ix, int segments, int centroids, int use_bits_encoding, int encoder,
                    const float* centroid_table) {
    CodeLayout L;
    if (check(ix) || !centroid_table || segments <= 0 || ix->dim % segments || !L.init(centroids, use_bits_encoding) ||
        (encoder != WV_PQ_TILE && encoder != WV_PQ_KMEANS))
        return fail(WV_EINVAL, "wv_index_set_pq: bad argument (segments must divide dims, 2 <= centroids <= 65536)");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    ix->pq_m = segments;
    ix->pq_ks = centroids;
    ix->pq_ds = ix->dim / segments;
    ix->pq_encoder = encoder;
    ix->pq_use_bits = use_bits_encoding != 0;
    ix->pq_stride = centroids > 256 ? ((2 * (uint64_t)segments + 7) & ~7ull) : (((uint64_t)segments + 3) & ~3ull);
    const size_t tbytes = (size_t)segments * centroids * ix->pq_ds * 4;
    HIP_TRY(ix->pq_cent.ensure(tbytes));
    HIP_TRY(ix->pq_codes.ensure(ix->capacity * ix->pq_stride));
    HIP_TRY(hipMemcpyAsync(ix->pq_cent.p, centroid_table, tbytes, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemsetAsync(ix->pq_codes.p, 0, ix->capacity * ix->pq_stride, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->has_code.assign(ix->bm_words, 0);
    ix->pq_set = true;
    ix->pq_on = false;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

namespace {
// scratch of one wv_index_fit_pq call, returned when it ends
struct FitScratch {
    DevBuf rowmap, active, points, changes, key, val, skey, sval, start, donor, reseeded, sort;
    ~FitScratch() {
        for (DevBuf* b : {&rowmap, &active, &points, &changes, &key, &val, &skey, &sval, &start, &donor, &reseeded, &sort})
            b->release();
    }
};
// bytes per (row, segment) of a group: points, the pairs in and out, and the
// radix sort's own copy of both
constexpr uint64_t FIT_PAIR_BYTES = 28;
constexpr uint64_t FIT_GROUP_BYTES = 1ull << 30;
}  // namespace

int wv_index_fit_pq(wv_index* ix, int segments, int centroids, int use_bits_encoding, const float* init_table,
                    uint64_t seed, float* out_table, int32_t* out_iterations, uint64_t* out_reseeded) {
    if (!ix) return fail(WV_EINVAL, "wv_index_fit_pq: null index");
    if (segments <= 0) segments = ix->dim;   // compress.go:54-56
    CodeLayout L;
    if (ix->dim % segments || !L.init(centroids, use_bits_encoding != 0))
        return fail(WV_EINVAL, "wv_index_fit_pq: bad argument (segments must divide dims, 2 <= centroids <= 65536)");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->pq_on) return fail(WV_ESTATE, "wv_index_fit_pq: the index is compressed (wv_index_set_compressed(ix, 0) first)");
    // cleanData (compress.go:62-69): the rows that hold a vector, in id order
    uint64_t n = 0;
    for (uint64_t w = 0; w < ix->bm_words; ++w) n += (uint64_t)__builtin_popcountll(ix->has_vec[w]);
    if (n < (uint64_t)centroids) return fail(WV_ESTATE, "wv_index_fit_pq: too few data to fit KMeans (rows < centroids)");
    if (n > 0x7FFFFFFFull) return fail(WV_ESTATE, "wv_index_fit_pq: more than 2^31 - 1 rows");
    HIP_TRY(hipSetDevice(ix->cfg.device));
    hipStream_t s = ix->stream;
    const int ds = ix->dim / segments;
    ix->pq_set = false;   // until the fit is complete
    ix->pq_m = segments;
    ix->pq_ks = centroids;
    ix->pq_ds = ds;
    ix->pq_encoder = WV_PQ_KMEANS;
    ix->pq_use_bits = use_bits_encoding != 0;
    ix->pq_stride = centroids > 256 ? ((2 * (uint64_t)segments + 7) & ~7ull) : (((uint64_t)segments + 3) & ~3ull);
    const size_t tbytes = (size_t)segments * centroids * ds * 4;
    HIP_TRY(ix->pq_cent.ensure(tbytes));
    HIP_TRY(ix->pq_codes.ensure(ix->capacity * ix->pq_stride));

    FitScratch sc;
    wv::PqFitParams p{};
    p.X = ix->vecs.as<float>();
    p.ldx = ix->ldx;
    p.n = n;
    p.ks = centroids;
    p.ds = ds;
    p.cc = wv_pq_fit_chunk_centres(centroids, ds);
    p.seed = seed;
    p.cent = ix->pq_cent.as<float>();
    if (n != ix->n_rows) {   // holes: position -> row
        std::vector<uint32_t> rows;
        rows.reserve(n);
        for (uint64_t i = 0; i < ix->n_rows; ++i)
            if (ix->has_vec[i >> 6] & (1ull << (i & 63))) rows.push_back((uint32_t)i);
        HIP_TRY(sc.rowmap.ensure(n * 4));
        HIP_TRY(hipMemcpyAsync(sc.rowmap.p, rows.data(), n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        p.rowmap = sc.rowmap.as<uint32_t>();
    }
    if (init_table) HIP_TRY(hipMemcpyAsync(p.cent, init_table, tbytes, hipMemcpyHostToDevice, s));
    else HIP_TRY(wv_launch_pq_fit_init(&p, segments, s));

    // segments per group: the sort buffers stay within FIT_GROUP_BYTES (one
    // segment's where n alone outgrows that), the pair count within an int
    const int group = (int)std::max<uint64_t>(
        1, std::min<uint64_t>({(uint64_t)segments, FIT_GROUP_BYTES / (FIT_PAIR_BYTES * n), 0x7FFFFFFFull / n}));
    HIP_TRY(sc.active.ensure((size_t)group * 4));
    HIP_TRY(sc.changes.ensure((size_t)group * 4));
    HIP_TRY(sc.reseeded.ensure(8));
    for (DevBuf* b : {&sc.points, &sc.key, &sc.val, &sc.skey, &sc.sval}) HIP_TRY(b->ensure((size_t)group * n * 4));
    HIP_TRY(sc.start.ensure(((size_t)group * centroids + 1) * 4));
    HIP_TRY(sc.donor.ensure((size_t)group * centroids * 4));
    p.active = sc.active.as<int32_t>();
    p.points = sc.points.as<uint32_t>();
    p.changes = sc.changes.as<uint32_t>();
    p.key = sc.key.as<uint32_t>();
    p.val = sc.val.as<uint32_t>();
    p.skey = sc.skey.as<uint32_t>();
    p.sval = sc.sval.as<uint32_t>();
    p.start = sc.start.as<uint32_t>();
    p.donor = sc.donor.as<uint32_t>();
    p.reseeded = sc.reseeded.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(p.reseeded, 0, 8, s));

    // stopCondition (kmeans.go:191-194): an fp32 product, truncated
    const float delta = (float)n * 0.01f;
    const int64_t min_changes = (int64_t)delta;
    std::vector<int32_t> iters((size_t)segments, 0), act;
    std::vector<uint32_t> chg;
    for (int s0 = 0; s0 < segments; s0 += group) {
        p.s0 = s0;
        p.ng = std::min(group, segments - s0);
        act.assign((size_t)p.ng, 1);
        chg.assign((size_t)p.ng, 0);
        size_t sort_bytes = 0;
        HIP_TRY(wv_pq_fit_sort(&p, nullptr, &sort_bytes, s));
        HIP_TRY(sc.sort.ensure(sort_bytes));
        sort_bytes = sc.sort.cap;
        HIP_TRY(hipMemsetAsync(p.points, 0, (size_t)p.ng * n * 4, s));   // m.data.points = make([]uint64, dataSize)
        HIP_TRY(wv_launch_pq_fit_iota(&p, s));
        for (int i = 0;; ++i) {
            p.iter = i;
            HIP_TRY(hipMemcpyAsync(sc.active.p, act.data(), (size_t)p.ng * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(p.changes, 0, (size_t)p.ng * 4, s));
            HIP_TRY(wv_launch_pq_fit_assign(&p, s));
            HIP_TRY(wv_pq_fit_sort(&p, sc.sort.p, &sort_bytes, s));
            HIP_TRY(wv_launch_pq_fit_empty(&p, s));
            HIP_TRY(wv_launch_pq_fit_centres(&p, s));
            HIP_TRY(hipMemcpyAsync(chg.data(), p.changes, (size_t)p.ng * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            bool any = false;
            for (int sl = 0; sl < p.ng; ++sl) {
                if (!act[sl]) continue;
                iters[s0 + sl] = i + 1;
                if (i >= 10 || (int64_t)chg[sl] < min_changes || chg[sl] == 0) act[sl] = 0;
                else any = true;
            }
            if (!any) break;
        }
    }
    unsigned long long reseeded = 0;
    HIP_TRY(hipMemcpyAsync(&reseeded, p.reseeded, 8, hipMemcpyDeviceToHost, s));
    if (out_table) HIP_TRY(hipMemcpyAsync(out_table, p.cent, tbytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(ix->pq_codes.p, 0, ix->capacity * ix->pq_stride, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_iterations) std::copy(iters.begin(), iters.end(), out_iterations);
    if (out_reseeded) *out_reseeded = reseeded;
    ix->has_code.assign(ix->bm_words, 0);
    ix->pq_set = true;
    ix->pq_on = false;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_upload_pq_codes(wv_index* ix, const uint8_t* encoded, uint64_t n, uint64_t first_id) {
    if (check(ix) || (n && !encoded)) return fail(WV_EINVAL, "wv_index_upload_pq_codes: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->pq_set) return fail(WV_ESTATE, "wv_index_upload_pq_codes: no quantizer (wv_index_set_pq)");
    if (first_id + n > ix->capacity) return fail(WV_EINVAL, "wv_index_upload_pq_codes: beyond capacity");
    if (n == 0) return WV_OK;
    HIP_TRY(hipSetDevice(ix->cfg.device));
    CodeLayout L;
    L.init(ix->pq_ks, ix->pq_use_bits);
    const size_t len = (size_t)ix->pq_m * L.bytes;
    std::vector<uint8_t> row(len + 8, 0), out(n * ix->pq_stride, 0);
    for (uint64_t r = 0; r < n; ++r) {
        std::memcpy(row.data(), encoded + r * len, len);   // zero tail: the packed reader looks one byte ahead
        uint8_t* dst = out.data() + r * ix->pq_stride;
        for (int i = 0; i < ix->pq_m; ++i) {
            const uint64_t c = L.get(row.data(), i);
            if (c >= (uint64_t)ix->pq_ks) return fail(WV_EINVAL, "wv_index_upload_pq_codes: code out of range");
            if (ix->pq_ks > 256) reinterpret_cast<uint16_t*>(dst)[i] = (uint16_t)c;
            else dst[i] = (uint8_t)c;
        }
    }
    HIP_TRY(hipMemcpyAsync(ix->pq_codes.as<uint8_t>() + first_id * ix->pq_stride, out.data(), out.size(),
                           hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (uint64_t i = first_id; i < first_id + n; ++i) ix->has_code[i >> 6] |= 1ull << (i & 63);
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_pq_encode(wv_index* ix) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->pq_set || ix->pq_encoder != WV_PQ_KMEANS)
        return fail(WV_ESTATE, "wv_index_pq_encode: needs a KMeans quantizer (wv_index_set_pq)");
    HIP_TRY(hipSetDevice(ix->cfg.device));
    wv::PqParams pq = pq_params(ix);
    HIP_TRY(wv_launch_pq_encode(ix->vecs.as<float>(), ix->ldx, nullptr, ix->n_rows, &pq, ix->pq_codes.as<uint8_t>(),
                                ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (uint64_t w = 0; w < ix->bm_words; ++w) ix->has_code[w] |= ix->has_vec[w];
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_download_pq_codes(wv_index* ix, uint16_t* out, uint64_t first_id, uint64_t n) {
    if (check(ix) || (n && !out)) return fail(WV_EINVAL, "wv_index_download_pq_codes: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->pq_set) return fail(WV_ESTATE, "wv_index_download_pq_codes: no quantizer");
    if (first_id + n > ix->capacity) return fail(WV_EINVAL, "wv_index_download_pq_codes: beyond capacity");
    HIP_TRY(hipSetDevice(ix->cfg.device));
    std::vector<uint8_t> raw(n * ix->pq_stride);
    HIP_TRY(hipMemcpyAsync(raw.data(), ix->pq_codes.as<uint8_t>() + first_id * ix->pq_stride, raw.size(),
                           hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (uint64_t r = 0; r < n; ++r)
        for (int i = 0; i < ix->pq_m; ++i) {
            const uint8_t* src = raw.data() + r * ix->pq_stride;
            out[r * ix->pq_m + i] = ix->pq_ks > 256 ? reinterpret_cast<const uint16_t*>(src)[i] : src[i];
        }
    return WV_OK;
}

int wv_index_set_compressed(wv_index* ix, int on) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    if (on) {
        if (!ix->pq_set) return fail(WV_ESTATE, "wv_index_set_compressed: no quantizer (wv_index_set_pq)");
        for (uint64_t w = 0; w < ix->bm_words; ++w)
            if (ix->has_vec[w] & ~ix->has_code[w])
                return fail(WV_ESTATE, "wv_index_set_compressed: a row with a vector has no code");
    }
    ix->pq_on = on != 0;
    ix->bitmaps_dirty = true;
    return WV_OK;
}

int wv_index_set_pq_list_search(wv_index* ix, int on) {
    if (!ix) return fail(WV_EINVAL, "wv_index_set_pq_list_search: null index");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->pq_list_search = on != 0;
    return WV_OK;
}

int wv_search_time_ef(const wv_index* ix, int k) { return ix ? search_time_ef(ix->cfg, k) : -1; }
int wv_config_search_time_ef(const wv_config* cfg, int k) { return cfg ? search_time_ef(*cfg, k) : -1; }

int wv_merge_shards_device(const float* d_in_dists, const uint64_t* d_in_ids, const int32_t* d_in_n, int n_shards,
                           int nq, int k, float* d_out_dists, uint64_t* d_out_ids, int32_t* d_out_n, void* stream) {
    if (n_shards <= 0 || n_shards > 16 || nq < 0 || k <= 0) return fail(WV_EINVAL, "wv_merge_shards_device: bad argument");
    if (nq == 0) return WV_OK;
    HIP_TRY(launch_merge_shards(d_in_dists, d_in_ids, d_in_n, n_shards, nq, k, d_out_dists, d_out_ids, d_out_n,
                                (hipStream_t)stream));
    return WV_OK;
}

int wv_index_set_timing(wv_index* ix, int enable) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    ix->timing = enable != 0;
    ix->ev_used = 0;
    return WV_OK;
}

// the recorded event sets -> per-batch averages (one sync, on request)
static int read_timing(wv_index* ix) {
    if (ix->ev_used == 0) return WV_OK;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t b = 0; b < ix->ev_used; ++b) {
        const auto& e = ix->ev_pool[b];
        const uint8_t m = ix->ev_mask[b];
        for (int pr = 0; pr < 4; ++pr) {
            if ((m & (3u << (2 * pr))) != (3u << (2 * pr))) continue;
            HIP_TRY(hipEventSynchronize(e[2 * pr + 1]));
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, e[2 * pr], e[2 * pr + 1]));
            a[pr] += t;
        }
    }
    const float inv = 1.0f / (float)ix->ev_used;
    ix->t_mfma = a[0] * inv;
    ix->t_fin = a[1] * inv;
    ix->t_hnsw = a[2] * inv;
    ix->t_pre = a[3] * inv;
    ix->ev_used = 0;
    return WV_OK;
}

int wv_last_kernel_times(wv_index* ix, float* bf_mfma_ms, float* bf_finalize_ms, float* hnsw_ms) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    int rc = read_timing(ix);
    if (rc) return rc;
    if (bf_mfma_ms) *bf_mfma_ms = ix->t_mfma;
    if (bf_finalize_ms) *bf_finalize_ms = ix->t_fin;
    if (hnsw_ms) *hnsw_ms = ix->t_hnsw;
    return WV_OK;
}

int wv_last_seed_time(wv_index* ix, float* seed_ms) {
    if (check(ix) || !seed_ms) return fail(WV_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    int rc = read_timing(ix);
    if (rc) return rc;
    *seed_ms = ix->t_pre;
    return WV_OK;
}

int wv_last_batch_stats(wv_index* ix, uint64_t* dist_evals, uint64_t* expansions, uint64_t* fallbacks) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    unsigned long long acc[3] = {0, 0, 0};
    if (ix->stat_acc.p) {
        HIP_TRY(hipMemcpyAsync(acc, ix->stat_acc.p, 24, hipMemcpyDeviceToHost, ix->stat_stream));
        HIP_TRY(hipStreamSynchronize(ix->stat_stream));
    }
    if (dist_evals) *dist_evals = ix->last_dist + acc[0];
    if (expansions) *expansions = ix->last_exp + acc[1];
    if (fallbacks) *fallbacks = ix->last_fallbacks + acc[2];
    return WV_OK;
}

int wv_last_side_stats(wv_index* ix, uint64_t* overflowed, uint64_t* redone, uint64_t* claims, int* side_rows,
                       int* spill_cap) {
    if (check(ix)) return WV_EINVAL;
    std::lock_guard<std::mutex> g(ix->mu);
    HIP_TRY(hipSetDevice(ix->cfg.device));
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    if (ix->stat_acc.p) {
        HIP_TRY(hipMemcpyAsync(acc, ix->stat_acc.p, 48, hipMemcpyDeviceToHost, ix->stat_stream));
        HIP_TRY(hipStreamSynchronize(ix->stat_stream));
    }
    if (overflowed) *overflowed = acc[3];
    if (redone) *redone = acc[4];
    if (claims) *claims = acc[5];
    if (side_rows) *side_rows = ix->last_side_rows;
    if (spill_cap) *spill_cap = ix->last_side_xs;
    return WV_OK;
}

}  // extern "C"
