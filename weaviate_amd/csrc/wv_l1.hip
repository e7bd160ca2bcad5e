// wv_l1.hip -- manhattan and hamming distances (distancer/manhattan.go,
// distancer/hamming.go) over the resident fp32 rows: exact k-NN search and the
// threshold pass of SearchByVectorDistance.
//
// Neither metric is a contraction, so there is no MFMA key pass and nothing to
// certify.  The reference accumulates one serial fp32 chain per (query, row)
// in dimension order,
//     manhattan: sum += |a[i] - b[i]|        hamming: sum += 1 when a[i] != b[i]
// (float compare: -0 == +0, a NaN differs from everything), and a thread that
// owns a (query, row) pair for the whole k loop produces exactly that chain.
// The kernel's distances are therefore the reference's bits: no re-rank.
//
// Work split.  Grid (corpus segment, query block); a segment is a run of
// whole 128-row tiles, and the host sizes the segments from the CU count so
// that every CU holds its share of workgroups.  A 256-thread workgroup
// computes a BQ-query x 128-row tile; each thread holds TQ x TR accumulators:
//     wide   BQ = 64, 4 x 8 per thread (16 query groups x 16 row groups)
//     narrow BQ =  8, 1 x 4 per thread ( 8 query groups x 32 row groups)
// The k loop streams both operands through LDS in 16-float chunks, double
// buffered: a thread loads float4s along the row (4 lanes cover a row's 64
// bytes), and stores them k-major, xs[k][row] with a row of 128 + 4 floats and
// qs[k][query] with BQ + 4 -- 4 x LD = 16 mod 64 words, so the four k-quarters
// of a wave's transposing store fall in four disjoint sets of 16 banks.  Per k
// a thread reads its operands as TQ/4 + TR/4 128-bit LDS reads (a row group's
// 4 rows, then the 4 rows 4 RG further: a wave's 16 or 32 row groups read
// consecutive 16-byte words) and does TQ x TR subtracts and TQ x TR adds with
// the |.| source modifier (hamming: compare, select, add).  Columns past D
// are zeroed in LDS for both operands (the caller's query padding is not
// trusted); they add +0 to a non-negative sum, which changes no bit.
//
// The narrow block serves small batches: at one query the wide block spends
// 64 x the useful VALU work, where the pass should be bound by reading the
// corpus.  The host takes the narrow block for nq <= L1_NARROW_NQ (128),
// from the measured crossover at 1M x 128 (profiles/l1/README.md): hamming's
// lies between 128 queries (2.87 against 3.00 ms) and 192 (4.26 against
// 4.14 ms), manhattan's above 256 (3.32 against 3.71 ms), so up to 128 the
// narrow block is ahead for both.  Three resident narrow workgroups hide
// each other's LDS and barrier stalls; the single wide one cannot.
//
// k-NN epilogue.  A query's candidates live in an LDS pool of 256 fin_key
// (dist, id) keys, with its bound (the k-th key once k are known, else
// L1_EMPTY) and its count.  After a tile's k loop a thread tests its rows
// against the tile's eligibility words (exclusion bitmap, shared or per-query
// allow bitmap and the row count, staged once per tile) and appends the keys
// below the bound -- the whole 64-bit key, so a lower id wins a tie.  A pool
// that the next tile could overflow (count > 256 - 128) is sorted by one wave
// (bitonic256_wave), cut to k, and its bound set to key k - 1; hence
// L1_KMAX = 128.  At the segment's end every pool is sorted and its first k
// keys go to part[q][segment][k]; l1_merge_kernel merges a query's segments
// (four waves over quarters of them, 256 - k new keys a sort) and writes the
// (dist, id) rows.
//
// LDS, wide k-NN block, against the CU's 160 KiB (163,840 B):
//     operand rings 2 x 16 x 132 x 4 + 2 x 16 x 68 x 4   =  25,600
//     pools         64 x 256 x 8                          = 131,072
//     eligibility 64 x 2 x 8, bounds 64 x 8, counts 64 x 4 =   1,792
//     the threshold epilogue's bases and totals 3 x 64 x 4 =     768
//                                                   total = 159,232
// (158,976 allocated: the k-NN instantiation drops the unused bases) so one
// wide workgroup per CU;
// the narrow block takes 35 KiB and, at 159 VGPRs (manhattan), three fit a CU.
//
// Threshold epilogue (SearchByVectorDistance).  Same loop.  A row is kept when
// (double) d - target <= 1e-6, exactly sbd_scan_kernel's test; its sbd_key
// goes to the query's LDS list of the tile, whose range in the query's segment
// of `cap` keys is reserved with one memory atomic per (query, tile); stores
// are guarded by cap.  cnt[3q], cnt[3q + 1] (d <= target) and cnt[3q + 2]
// (eligible rows) are kept as the scan keeps them, so the segmented sort and
// the host arithmetic of wv_distance.hip apply unchanged.
//
// Built without the packed fp32 forms, as wv_sbd_h16.hip is.
#include "wv_device.h"
#include "wv_l1_dev.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_topk.h"

namespace wv {

constexpr int L1_LDX = L1_BN + 4;          // LDS row of the corpus ring
constexpr int L1_POOL = 256;               // keys of a query's pool: one bitonic256_wave
constexpr uint64_t L1_EMPTY = ~0ull;       // above every fin_key
enum { L1_KNN = 0, L1_THRESH = 1 };

static_assert(L1_KMAX + L1_BN <= L1_POOL, "a pruned pool takes one more tile");

// l1_step, l1_load4: wv_l1_dev.h

// word w of a bitmap of nbits bits: bits past nbits (and words past it) read 0
__device__ __forceinline__ uint64_t l1_word(const uint64_t* __restrict__ bits, uint64_t nbits, uint64_t w) {
    const uint64_t words = (nbits + 63) >> 6;
    if (w >= words) return 0;
    uint64_t v = bits[w];
    if (w == words - 1 && (nbits & 63)) v &= (1ull << (nbits & 63)) - 1;
    return v;
}

// one wave: the pool's first c keys sorted (the rest L1_EMPTY), written back whole
__device__ __forceinline__ void l1_sort_pool(uint64_t* pool, int c, int lane) {
    uint64_t kk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kk[j] = 64 * j + lane < c ? pool[64 * j + lane] : L1_EMPTY;
    bitonic256_wave(kk, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) pool[64 * j + lane] = kk[j];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int METRIC, int BQ, int TQ, int EPI>
__global__ __launch_bounds__(256) void l1_kernel(L1Params p) {
    constexpr int QG = BQ / TQ, RG = 256 / QG, TR = L1_BN / RG, LDQ = BQ + 4;
    constexpr int NPOOL = EPI == L1_KNN ? L1_POOL : L1_BN;
    static_assert(TQ == 1 || TQ == 4, "query operands: a scalar or one 128-bit read");
    static_assert(TR % 4 == 0 && QG * RG == 256 && RG * TR == L1_BN, "tile shape");
    __shared__ __attribute__((aligned(16))) float xs[2][L1_BK][L1_LDX];
    __shared__ __attribute__((aligned(16))) float qs[2][L1_BK][LDQ];
    __shared__ uint64_t pool[BQ][NPOOL];
    __shared__ uint64_t elig[BQ][2];
    __shared__ uint64_t bound[BQ];      // (k-NN) the k-th key, L1_EMPTY until k are known
    __shared__ int cnt[BQ];             // keys in the pool / in the tile's list
    __shared__ unsigned int base[BQ];   // (threshold) the tile's range in the query's segment
    __shared__ unsigned int tot_a[BQ], tot_ok[BQ];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tr = tid % RG, tq = tid / RG;
    const int seg = blockIdx.x, q0 = (int)blockIdx.y * BQ;
    const uint32_t t_beg = (uint32_t)seg * p.tiles_per_seg;
    const uint32_t t_end = min(p.ntiles, t_beg + p.tiles_per_seg);
    const int nk = (p.D + L1_BK - 1) / L1_BK;
    const bool per_query = p.allow && p.allow_stride;

    if (tid < BQ) {
        bound[tid] = L1_EMPTY;
        cnt[tid] = 0;
        tot_a[tid] = tot_ok[tid] = 0;
    }
    float tf[TQ];
    unsigned int n_a[TQ], n_ok[TQ];
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
        const int q = q0 + tq * TQ + i;
        tf[i] = EPI == L1_THRESH && q < p.nq ? p.target[q] : 0.f;
        n_a[i] = n_ok[i] = 0;
    }
    // the operand a thread fetches: corpus float4s f = tid, tid + 256 (row f / 4,
    // k-quarter f % 4), query float4 f = tid < 4 BQ
    const int lq = tid >> 2, k4 = (tid & 3) * 4;
    const float* qrow = tid < 4 * BQ && q0 + lq < p.nq ? p.Q + (uint64_t)(q0 + lq) * p.ldq : nullptr;

    for (uint32_t tile = t_beg; tile < t_end; ++tile) {
        const uint64_t row0 = (uint64_t)tile * L1_BN;
        // the tile's eligibility words: not excluded, allowed, below N
        if (tid < 2 * BQ && (per_query || tid < 2)) {
            const int ql = tid >> 1, h = tid & 1;
            const uint64_t w = (uint64_t)tile * 2 + h, r = w * 64;
            uint64_t e = ~l1_word(p.excl, p.excl_nbits, w);
            if (p.allow) {
                const int q = min(q0 + ql, p.nq - 1);
                e &= l1_word(p.allow + (per_query ? (uint64_t)q * p.allow_stride : 0), p.allow_nbits, w);
            }
            if (r >= p.N) e = 0;
            else if (p.N - r < 64) e &= (1ull << (p.N - r)) - 1;
            elig[ql][h] = e;
        }
        const float* xrow[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const uint64_t r = row0 + (uint64_t)(lq + 64 * it);
            xrow[it] = r < p.N ? p.X + r * (uint64_t)p.ldx : nullptr;
        }
        float acc[TQ][TR];
#pragma unroll
        for (int i = 0; i < TQ; ++i)
#pragma unroll
            for (int j = 0; j < TR; ++j) acc[i][j] = 0.f;

        float4 xr[2], qr;
        auto fetch = [&](int kc) {
            const int kk = kc * L1_BK + k4;
            xr[0] = l1_load4(xrow[0], kk, p.ldx, p.D);
            xr[1] = l1_load4(xrow[1], kk, p.ldx, p.D);
            if (tid < 4 * BQ) qr = l1_load4(qrow, kk, p.ldq, p.D);
        };
        auto stash = [&](int b) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                float* d = &xs[b][k4][lq + 64 * it];
                d[0] = xr[it].x;
                d[L1_LDX] = xr[it].y;
                d[2 * L1_LDX] = xr[it].z;
                d[3 * L1_LDX] = xr[it].w;
            }
            if (tid < 4 * BQ) {
                float* d = &qs[b][k4][lq];
                d[0] = qr.x;
                d[LDQ] = qr.y;
                d[2 * LDQ] = qr.z;
                d[3 * LDQ] = qr.w;
            }
        };
        fetch(0);
        stash(0);
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const int b = kc & 1;
            if (kc + 1 < nk) fetch(kc + 1);
#pragma unroll
            for (int k = 0; k < L1_BK; ++k) {
                float qv[TQ], xv[TR];
                if constexpr (TQ == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(&qs[b][k][tq * 4]);
                    qv[0] = v.x;
                    qv[1 % TQ] = v.y;
                    qv[2 % TQ] = v.z;
                    qv[3 % TQ] = v.w;
                } else {
                    qv[0] = qs[b][k][tq];
                }
#pragma unroll
                for (int g = 0; g < TR / 4; ++g) {
                    const float4 v = *reinterpret_cast<const float4*>(&xs[b][k][tr * 4 + g * RG * 4]);
                    xv[4 * g] = v.x;
                    xv[4 * g + 1] = v.y;
                    xv[4 * g + 2] = v.z;
                    xv[4 * g + 3] = v.w;
                }
#pragma unroll
                for (int i = 0; i < TQ; ++i)
#pragma unroll
                    for (int j = 0; j < TR; ++j) l1_step<METRIC>(acc[i][j], qv[i], xv[j]);
            }
            if (kc + 1 < nk) stash(b ^ 1);
            __syncthreads();
        }

        // ---- epilogue: this thread's TQ x TR (query, row) pairs ----
#pragma unroll
        for (int i = 0; i < TQ; ++i) {
            const int ql = tq * TQ + i;
            const bool qvalid = q0 + ql < p.nq;
            const int ai = per_query ? ql : 0;
            const uint64_t e0 = elig[ai][0], e1 = elig[ai][1];
            const uint64_t bnd = EPI == L1_KNN ? bound[ql] : 0;
            const double t = (double)tf[i];
#pragma unroll
            for (int j = 0; j < TR; ++j) {
                const int r = tr * 4 + (j & 3) + RG * 4 * (j >> 2);
                const bool ok = qvalid && (((r < 64 ? e0 >> r : e1 >> (r - 64)) & 1ull) != 0);
                const float d = acc[i][j];
                const uint32_t row = (uint32_t)(row0 + (uint64_t)r);
                if constexpr (EPI == L1_KNN) {
                    const uint64_t key = fin_key(d, row);
                    if (ok && key < bnd) pool[ql][atomicAdd(&cnt[ql], 1)] = key;
                } else {
                    n_ok[i] += ok ? 1u : 0u;
                    n_a[i] += ok && d <= tf[i] ? 1u : 0u;
                    if (ok && (double)d - t <= 1e-6) pool[ql][atomicAdd(&cnt[ql], 1)] = sbd_key(d, row);
                }
            }
        }
        __syncthreads();
        if constexpr (EPI == L1_KNN) {
            // a pool the next tile could overflow, and every pool at the end:
            // sorted by one wave, cut to k
            const bool last = tile + 1 == t_end;
            for (int ql = wave; ql < BQ; ql += 4) {
                const int c = cnt[ql];
                if (c > L1_POOL - L1_BN || last) {
                    l1_sort_pool(pool[ql], c, lane);
                    if (lane == 0) {
                        cnt[ql] = min(c, p.k);
                        bound[ql] = c >= p.k ? pool[ql][p.k - 1] : L1_EMPTY;
                    }
                    if (last && q0 + ql < p.nq) {
                        unsigned long long* out = p.part + ((uint64_t)(q0 + ql) * p.n_seg + seg) * p.k;
                        for (int i = lane; i < p.k; i += 64) out[i] = pool[ql][i];
                    }
                }
            }
            __syncthreads();
        } else {
            if (tid < BQ) {
                const int c = cnt[tid];
                if (c) base[tid] = atomicAdd(p.cnt + 3 * (uint64_t)(q0 + tid), (unsigned int)c);
            }
            __syncthreads();
            for (int idx = tid; idx < BQ * L1_BN; idx += 256) {
                const int ql = idx / L1_BN, s = idx % L1_BN;
                if (s < cnt[ql]) {
                    const unsigned int pos = base[ql] + (unsigned int)s;
                    if (pos < (unsigned int)p.cap) p.keys[(uint64_t)(q0 + ql) * p.cap + pos] = pool[ql][s];
                }
            }
            __syncthreads();
            if (tid < BQ) cnt[tid] = 0;
        }
    }
    if (EPI == L1_THRESH) {
#pragma unroll
        for (int i = 0; i < TQ; ++i) {
            if (n_a[i]) atomicAdd(&tot_a[tq * TQ + i], n_a[i]);
            if (n_ok[i]) atomicAdd(&tot_ok[tq * TQ + i], n_ok[i]);
        }
        __syncthreads();
        if (tid < BQ && q0 + tid < p.nq) {
            if (tot_a[tid]) atomicAdd(p.cnt + 3 * (uint64_t)(q0 + tid) + 1, tot_a[tid]);
            if (tot_ok[tid]) atomicAdd(p.cnt + 3 * (uint64_t)(q0 + tid) + 2, tot_ok[tid]);
        }
    }
}

// One workgroup per query: wave w folds quarter w of the query's n_seg x k
// segment keys into its best k (kept in best[w], 256 - k new keys a sort),
// then wave 0 folds the four and writes the rows.
__global__ __launch_bounds__(256) void l1_merge_kernel(L1Params p) {
    __shared__ uint64_t best[4][L1_POOL];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = p.k, step = L1_POOL - k;
    const unsigned long long* in = p.part + (uint64_t)q * p.n_seg * k;
    const int64_t total = (int64_t)p.n_seg * k, per = (total + 3) / 4;
    const int64_t beg = wave * per < total ? wave * per : total, end = beg + per < total ? beg + per : total;
    uint64_t* mine = best[wave];
    for (int j = 0; j < 4; ++j) mine[64 * j + lane] = L1_EMPTY;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t pos = beg; pos < end; pos += step) {
        for (int i = lane; i < step; i += 64) mine[k + i] = pos + i < end ? in[pos + i] : L1_EMPTY;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        l1_sort_pool(mine, L1_POOL, lane);
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) {
        for (int i = lane; i < L1_POOL - k; i += 64) mine[k + i] = i < k ? best[w][i] : L1_EMPTY;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        l1_sort_pool(mine, L1_POOL, lane);
    }
    int n = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        const bool have = i < k && mine[i] != L1_EMPTY;
        if (have) {
            float d;
            uint32_t id;
            fin_unkey(mine[i], d, id);
            p.out_ids[(uint64_t)q * k + i] = p.id_base + id;
            p.out_d[(uint64_t)q * k + i] = d;
        }
        n += __popcll(__ballot(have));
    }
    if (lane == 0) p.out_n[q] = n;
}

}  // namespace wv

namespace {

// what both launchers ask of the operands and the schedule
bool l1_params_ok(const wv::L1Params* p) {
    return (p->metric == WV_METRIC_MANHATTAN || p->metric == WV_METRIC_HAMMING) && p->X && p->Q && p->excl &&
           p->D >= 1 && p->ldx >= p->D && p->ldq >= p->D && p->ldx % 4 == 0 && p->ldq % 4 == 0 &&
           ((uintptr_t)p->X & 15) == 0 && ((uintptr_t)p->Q & 15) == 0 && p->N < (1ull << 31) &&
           p->excl_nbits >= p->N && (uint64_t)p->ntiles * wv::L1_BN >= p->N &&
           (uint64_t)(p->ntiles - 1) * wv::L1_BN < p->N && p->tiles_per_seg >= 1 && p->n_seg >= 1 &&
           (uint64_t)p->n_seg * p->tiles_per_seg >= p->ntiles &&
           (uint64_t)(p->n_seg - 1) * p->tiles_per_seg < p->ntiles;
}

template <int EPI>
hipError_t l1_launch(const wv::L1Params* p, hipStream_t s) {
    const int bq = p->narrow ? wv::L1_BQ_NARROW : wv::L1_BQ_WIDE;
    const int nqb = (p->nq + bq - 1) / bq;
    if (nqb > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->n_seg, (unsigned)nqb);
    const bool man = p->metric == WV_METRIC_MANHATTAN;
    if (p->narrow) {
        if (man) hipLaunchKernelGGL((wv::l1_kernel<WV_METRIC_MANHATTAN, wv::L1_BQ_NARROW, 1, EPI>), grid, dim3(256), 0, s, *p);
        else hipLaunchKernelGGL((wv::l1_kernel<WV_METRIC_HAMMING, wv::L1_BQ_NARROW, 1, EPI>), grid, dim3(256), 0, s, *p);
    } else {
        if (man) hipLaunchKernelGGL((wv::l1_kernel<WV_METRIC_MANHATTAN, wv::L1_BQ_WIDE, 4, EPI>), grid, dim3(256), 0, s, *p);
        else hipLaunchKernelGGL((wv::l1_kernel<WV_METRIC_HAMMING, wv::L1_BQ_WIDE, 4, EPI>), grid, dim3(256), 0, s, *p);
    }
    return hipGetLastError();
}

}  // namespace

extern "C" {

hipError_t wv_launch_l1_knn(const wv::L1Params* p, hipStream_t s) {
    if (p->nq == 0 || p->N == 0) return hipSuccess;
    if (!l1_params_ok(p) || p->nq < 0 || p->k < 1 || p->k > wv::L1_KMAX || !p->part || !p->out_ids || !p->out_d ||
        !p->out_n)
        return hipErrorInvalidValue;
    hipError_t e = l1_launch<wv::L1_KNN>(p, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wv::l1_merge_kernel, dim3((unsigned)p->nq), dim3(256), 0, s, *p);
    return hipGetLastError();
}

hipError_t wv_launch_l1_thresh(const wv::L1Params* p, hipStream_t s) {
    if (p->nq == 0 || p->N == 0) return hipSuccess;
    if (!l1_params_ok(p) || p->nq < 0 || !p->target || !p->keys || !p->cnt || p->cap < 1) return hipErrorInvalidValue;
    return l1_launch<wv::L1_THRESH>(p, s);
}

}  // extern "C"
