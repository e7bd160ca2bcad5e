// wv_flat_ids.hip -- flatSearch over per-query allow lists given as ids
// (adapters/repos/db/vector/hnsw/flat_search.go:24-58): only the listed rows
// are read.
//
// One workgroup (4 waves) per (query, chunk of its list).  A wave takes 64 ids
// a step, drops the ids past the corpus and the excluded rows (tombstone, nil
// node, no vector), compacts the survivors into its LDS slots and computes
// their reference-order distances 32 rows at a time (exact_dist_rows: all row
// loads of a slab in flight before any FMA).  Selection keeps (dist, id) as
// fin_key keys: a wave holds its 256 smallest sorted in registers (element
// 64 j + lane in register j); a new key is staged only if it is below the
// wave's k-th, and a full stage is sorted and merged in (the element-wise
// minimum of an ascending and a descending run is bitonic and holds the 256
// smallest of both).  The waves merge through LDS, the chunks of a query in
// flat_ids_merge_kernel.  The path is exact from the start: no key pass, no
// certificate.
//
// On a compressed index (flat_ids_pq_kernel) the walk, the selection and the
// merges are the same; the distance is the PQ distance of the id's codes, one
// row per lane, from the query's lookup table in LDS (wv_pq_lut.h) or from
// pq_dist_row -- the same bits.
#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_pq_lut.h"
#include "wv_topk.h"

namespace wv {

constexpr uint64_t FI_EMPTY = ~0ull;
constexpr int FI_STAGE = 256;   // staged keys per wave
constexpr int FI_STEP = 64;     // ids per wave step

__device__ __forceinline__ void fi_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t fi_shfl(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The last phase of bitonic256_wave: a bitonic run of 256 keys, ascending after.
__device__ __forceinline__ void bitonic_merge256_wave(uint64_t (&kk)[4], int lane) {
    auto cas = [&](auto jc, auto pc) {   // (literal register indices, as in bitonic256_wave)
        constexpr int j = decltype(jc)::value, pj = decltype(pc)::value;
        const bool sw = kk[pj] < kk[j];
        const uint64_t t = kk[j];
        kk[j] = sw ? kk[pj] : kk[j];
        kk[pj] = sw ? t : kk[pj];
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    cas(I0{}, I2{}); cas(I1{}, I3{});
    cas(I0{}, I1{}); cas(I2{}, I3{});
#pragma unroll
    for (int jj = 32; jj > 0; jj >>= 1) {
        const bool lower = (lane & jj) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t plo = (uint32_t)__shfl_xor((int)(uint32_t)kk[j], jj, 64);
            const uint32_t phi = (uint32_t)__shfl_xor((int)(uint32_t)(kk[j] >> 32), jj, 64);
            const uint64_t pk = ((uint64_t)phi << 32) | plo;
            // the lower lane keeps the min
            const uint64_t a = lower ? pk : kk[j], b = lower ? kk[j] : pk;
            kk[j] = a < b ? pk : kk[j];
        }
    }
}

// top (ascending) <- the 256 smallest of top and desc (descending)
__device__ __forceinline__ void fi_merge(uint64_t (&top)[4], const uint64_t (&desc)[4], int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) top[j] = desc[j] < top[j] ? desc[j] : top[j];
    bitonic_merge256_wave(top, lane);
}

// the wave's cnt staged keys into top
__device__ __forceinline__ void fi_flush(uint64_t (&top)[4], const uint64_t* stage, int cnt, int lane) {
    uint64_t st[4];
    // sorted ascending as complements = descending as keys (an empty slot's complement is 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = 64 * j + lane < cnt ? ~stage[64 * j + lane] : 0ull;
    bitonic256_wave(st, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = ~st[j];
    fi_merge(top, st, lane);
}

// element k - 1 of top, in every lane
__device__ __forceinline__ uint64_t fi_kth(const uint64_t (&top)[4], int k) {
    const int j = (k - 1) >> 6;
    const uint64_t v = j == 0 ? top[0] : j == 1 ? top[1] : j == 2 ? top[2] : top[3];
    return fi_shfl(v, (k - 1) & 63);
}

// (P: FlatIdsParams or FlatIdsPqParams -- the same output fields)
template <int METRIC, class P>
__device__ __forceinline__ void fi_write(const P& p, const uint64_t (&top)[4], int q, int lane) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 64 * j + lane;
        const bool has = i < p.k && top[j] != FI_EMPTY;
        if (has) {
            float d;
            uint32_t id;
            fin_unkey(top[j], d, id);
            // fin_key folds -0 into +0; a dot product of exactly 0 is the
            // distance -0 (the sums themselves are never -0)
            if (METRIC == WV_METRIC_DOT && d == 0.f) d = -0.0f;
            p.out_ids[(size_t)q * p.k + i] = p.id_base + id;
            p.out_d[(size_t)q * p.k + i] = d;
        }
        n += __popcll(__ballot(has));
    }
    if (lane == 0) p.out_n[q] = n;
}

// The end of a workgroup's walk: each wave's last staged keys flushed, the
// waves merged through their stages, and wave 0 writes the query's output rows
// (one chunk) or the chunk's sorted keys for flat_ids_merge_kernel.
template <int METRIC, class P>
__device__ __forceinline__ void fi_finish(const P& p, uint64_t (&top)[4], uint64_t* stage_all, uint64_t* stage, int cnt,
                                          int s, int chunk, int q, int lane, int wave) {
    if (cnt) fi_flush(top, stage, cnt, lane);
    fi_wave_sync();
    // the waves of the workgroup: each leaves its sorted keys in its stage
#pragma unroll
    for (int j = 0; j < 4; ++j) stage[64 * j + lane] = top[j];
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) {
        uint64_t od[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) od[j] = stage_all[w * FI_STAGE + 255 - (64 * j + lane)];
        fi_merge(top, od, lane);
    }
    if (p.n_chunks == 1) {
        fi_write<METRIC>(p, top, q, lane);
    } else {
        unsigned long long* out = p.part + ((size_t)s * p.n_chunks + chunk) * p.k;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (64 * j + lane < p.k) out[64 * j + lane] = top[j];
    }
}

// grid (ns, n_chunks), 256 threads; dynamic LDS: stage | ids | dists | query
template <int METRIC>
__global__ __launch_bounds__(256) void flat_ids_kernel(FlatIdsParams p) {
    extern __shared__ __attribute__((aligned(16))) char fi_smem[];
    uint64_t* stage_all = reinterpret_cast<uint64_t*>(fi_smem);                              // [4][FI_STAGE]
    uint32_t* sid_all = reinterpret_cast<uint32_t*>(fi_smem + 4 * FI_STAGE * 8);             // [4][FI_STEP]
    float* sds_all = reinterpret_cast<float*>(fi_smem + 4 * FI_STAGE * 8 + 4 * FI_STEP * 4); // [4][FI_STEP]
    float* qv = reinterpret_cast<float*>(fi_smem + 4 * FI_STAGE * 8 + 8 * FI_STEP * 4);      // [dpad]
    const int s = blockIdx.x, chunk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = p.sel[s];
    for (int i = threadIdx.x; i < p.dpad; i += 256) qv[i] = p.Q[(uint64_t)q * p.dpad + i];
    __syncthreads();
    uint64_t* stage = stage_all + wave * FI_STAGE;
    uint32_t* sid = sid_all + wave * FI_STEP;
    float* sds = sds_all + wave * FI_STEP;
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)chunk * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;

    uint64_t top[4] = {FI_EMPTY, FI_EMPTY, FI_EMPTY, FI_EMPTY};
    uint64_t kth = FI_EMPTY;
    int cnt = 0;
    for (uint64_t i0 = beg + (uint64_t)FI_STEP * wave; i0 < end; i0 += 4 * FI_STEP) {
        const uint64_t i = i0 + lane;
        uint32_t id = 0;
        bool ok = false;
        if (i < end) {
            id = p.ids[i];
            ok = id < p.n_rows && !bit_test(p.excl, p.excl_nbits, id);
        }
        const uint64_t m = __ballot(ok);
        const int n = __popcll(m);
        if (ok) sid[mbcnt64(m)] = id;
        fi_wave_sync();
        if (n == 0) continue;
        exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, sid, min(n, 32), sds, lane);
        if (n > 32) exact_dist_rows<METRIC, 4, true>(qv, p.X, p.ldx, p.D, sid + 32, n - 32, sds + 32, lane);
        fi_wave_sync();
        const uint64_t key = lane < n ? fin_key(sds[lane], sid[lane]) : FI_EMPTY;
        const bool adm = key < kth;
        const uint64_t am = __ballot(adm);
        if (adm) stage[cnt + mbcnt64(am)] = key;
        cnt += __popcll(am);
        fi_wave_sync();
        if (cnt > FI_STAGE - FI_STEP) {
            fi_flush(top, stage, cnt, lane);
            cnt = 0;
            kth = fi_kth(top, p.k);
            fi_wave_sync();
        }
    }
    fi_finish<METRIC>(p, top, stage_all, stage, cnt, s, chunk, q, lane, wave);
}

// The same walk on a compressed index: grid (ns, n_chunks), 256 threads;
// dynamic LDS: stage | lookup table.  Each lane evaluates its own id's row from
// the codes -- no compaction into slots -- by the workgroup's table where the
// chunk holds at least lut_min_rows ids (the whole workgroup agrees), else by
// pq_dist_row on the query row in memory: the same bits either way.
template <int METRIC>
__global__ __launch_bounds__(256) void flat_ids_pq_kernel(FlatIdsPqParams p) {
    extern __shared__ __attribute__((aligned(16))) char fi_smem[];
    uint64_t* stage_all = reinterpret_cast<uint64_t*>(fi_smem);          // [4][FI_STAGE]
    float* lut = reinterpret_cast<float*>(fi_smem + 4 * FI_STAGE * 8);   // [m][ks] (when built)
    const int s = blockIdx.x, chunk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = p.sel[s];
    uint64_t* stage = stage_all + wave * FI_STAGE;
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)chunk * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;
    const float* qrow = p.Q + (uint64_t)q * p.dpad;
    const bool use_lut = end > beg && end - beg >= p.lut_min_rows;
    if (use_lut) pq_lut_build<METRIC>(lut, qrow, p.pq);

    uint64_t top[4] = {FI_EMPTY, FI_EMPTY, FI_EMPTY, FI_EMPTY};
    uint64_t kth = FI_EMPTY;
    int cnt = 0;
    for (uint64_t i0 = beg + (uint64_t)FI_STEP * wave; i0 < end; i0 += 4 * FI_STEP) {
        const uint64_t i = i0 + lane;
        uint32_t id = 0;
        bool ok = false;
        if (i < end) {
            id = p.ids[i];
            ok = id < p.n_rows && !bit_test(p.excl, p.excl_nbits, id);
        }
        if (__ballot(ok) == 0) continue;
        float d = 0.f;
        if (ok) d = use_lut ? pq_lut_dist<METRIC>(lut, p.pq, id) : pq_dist_row<METRIC>(qrow, p.pq, id);
        const uint64_t key = ok ? fin_key(d, id) : FI_EMPTY;
        const bool adm = key < kth;
        const uint64_t am = __ballot(adm);
        if (adm) stage[cnt + mbcnt64(am)] = key;
        cnt += __popcll(am);
        fi_wave_sync();
        if (cnt > FI_STAGE - FI_STEP) {
            fi_flush(top, stage, cnt, lane);
            cnt = 0;
            kth = fi_kth(top, p.k);
            fi_wave_sync();
        }
    }
    fi_finish<METRIC>(p, top, stage_all, stage, cnt, s, chunk, q, lane, wave);
}

// one wave per query: its chunks' sorted keys merged, then the output rows
template <int METRIC>
__global__ __launch_bounds__(64) void flat_ids_merge_kernel(FlatIdsParams p) {
    const int s = blockIdx.x, lane = threadIdx.x;
    uint64_t top[4] = {FI_EMPTY, FI_EMPTY, FI_EMPTY, FI_EMPTY};
    for (int c = 0; c < p.n_chunks; ++c) {
        const unsigned long long* in = p.part + ((size_t)s * p.n_chunks + c) * p.k;
        uint64_t od[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 255 - (64 * j + lane);
            od[j] = r < p.k ? in[r] : FI_EMPTY;
        }
        fi_merge(top, od, lane);
    }
    fi_write<METRIC>(p, top, p.sel[s], lane);
}

// bitmap rows of the queries sel[0 .. nsel) from their id lists (rows zeroed
// by the caller): one id per thread, grid (id blocks, nsel)
__global__ __launch_bounds__(256) void ids_to_bits_kernel(const uint32_t* ids, const uint64_t* off, const int32_t* sel,
                                                          uint64_t n_rows, uint64_t words, unsigned long long* bits) {
    const int r = blockIdx.y;
    const int q = sel[r];
    const uint64_t i = off[q] + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= off[q + 1]) return;
    const uint64_t id = ids[i];
    if (id >= n_rows || (id >> 6) >= words) return;
    atomicOr(bits + (uint64_t)r * words + (id >> 6), 1ull << (id & 63));
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_flat_ids(const wv::FlatIdsParams* p, hipStream_t s) {
    if (p->ns == 0) return hipSuccess;
    if (p->k < 1 || p->k > 256 || p->n_chunks < 1 || p->n_chunks > 65535 || p->dpad > wv::FLAT_IDS_DPAD_MAX ||
        p->chunk_len == 0 || (p->n_chunks > 1 && !p->part))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->ns, (unsigned)p->n_chunks);
    const size_t lds = 4 * wv::FI_STAGE * 8 + 8 * wv::FI_STEP * 4 + (size_t)p->dpad * 4;
    if (p->metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::flat_ids_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, *p);
    else if (p->metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::flat_ids_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, *p);
    else hipLaunchKernelGGL(wv::flat_ids_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p->n_chunks == 1) return e;
    // (the metric only decides how a zero distance is written)
    if (p->metric == WV_METRIC_DOT)
        hipLaunchKernelGGL(wv::flat_ids_merge_kernel<WV_METRIC_DOT>, dim3(p->ns), dim3(64), 0, s, *p);
    else
        hipLaunchKernelGGL(wv::flat_ids_merge_kernel<WV_METRIC_L2>, dim3(p->ns), dim3(64), 0, s, *p);
    return hipGetLastError();
}

hipError_t wv_launch_flat_ids_pq(const wv::FlatIdsPqParams* p, hipStream_t s) {
    if (p->ns == 0) return hipSuccess;
    if (p->k < 1 || p->k > 256 || p->n_chunks < 1 || p->n_chunks > 65535 || p->chunk_len == 0 ||
        p->chunk_len % 256 || (p->n_chunks > 1 && !p->part) || !wv::pq_ok(p->pq))
        return hipErrorInvalidValue;
    wv::FlatIdsPqParams pp = *p;
    // stage 8 KiB + a table of at most 64 KiB: two workgroups in a CU's 160 KiB
    const size_t lds = 4 * wv::FI_STAGE * 8 + wv::lut_plan(pp.pq, pp.lut, &pp.lut_min_rows);
    const dim3 grid((unsigned)pp.ns, (unsigned)pp.n_chunks);
    if (pp.metric == WV_METRIC_L2) hipLaunchKernelGGL(wv::flat_ids_pq_kernel<WV_METRIC_L2>, grid, dim3(256), lds, s, pp);
    else if (pp.metric == WV_METRIC_DOT) hipLaunchKernelGGL(wv::flat_ids_pq_kernel<WV_METRIC_DOT>, grid, dim3(256), lds, s, pp);
    else hipLaunchKernelGGL(wv::flat_ids_pq_kernel<WV_METRIC_COSINE>, grid, dim3(256), lds, s, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pp.n_chunks == 1) return e;
    // the chunks' keys merge as the raw kernel's do: the fields flat_ids_merge_kernel reads
    wv::FlatIdsParams mp{};
    mp.sel = pp.sel;
    mp.id_base = pp.id_base;
    mp.part = pp.part;
    mp.ns = pp.ns;
    mp.n_chunks = pp.n_chunks;
    mp.metric = pp.metric;
    mp.k = pp.k;
    mp.out_ids = pp.out_ids;
    mp.out_d = pp.out_d;
    mp.out_n = pp.out_n;
    if (mp.metric == WV_METRIC_DOT)
        hipLaunchKernelGGL(wv::flat_ids_merge_kernel<WV_METRIC_DOT>, dim3(mp.ns), dim3(64), 0, s, mp);
    else
        hipLaunchKernelGGL(wv::flat_ids_merge_kernel<WV_METRIC_L2>, dim3(mp.ns), dim3(64), 0, s, mp);
    return hipGetLastError();
}

hipError_t wv_launch_ids_to_bits(const uint32_t* ids, const uint64_t* off, const int32_t* sel, int nsel,
                                 uint64_t max_len, uint64_t n_rows, uint64_t words, uint64_t* bits, hipStream_t s) {
    if (nsel == 0 || max_len == 0) return hipSuccess;
    if (nsel > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((max_len + 255) / 256), (unsigned)nsel);
    hipLaunchKernelGGL(wv::ids_to_bits_kernel, grid, dim3(256), 0, s, ids, off, sel, n_rows, words,
                       reinterpret_cast<unsigned long long*>(bits));
    return hipGetLastError();
}

}  // extern "C"
