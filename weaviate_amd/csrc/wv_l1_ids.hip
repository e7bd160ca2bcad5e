// wv_l1_ids.hip -- manhattan and hamming distances over per-query allow lists
// given as ids (flat_search.go:24-58 with distancer/manhattan.go and
// distancer/hamming.go): only the listed rows are read.  The k-NN search of
// wv_search_batch_ids and the threshold pass of
// wv_search_by_vector_distance_batch_ids on such an index.
//
// Both distances are one serial fp32 chain per (query, row) in dimension order
// (wv_l1.hip), so one lane owns a pair from the first column to the last: no
// cross-lane reduction, hence not exact_dist_rows' 8 lanes a row.
//
// Work split.  Grid (selected query, chunk of its list), 256 threads, as
// flat_ids_kernel and sbd_ids_kernel: the query row sits in LDS (columns >= D
// zeroed, the caller's padding is not trusted).  A wave takes L1I_STEP =
// 64 L1I_R consecutive list entries a step, drops the ids past the corpus and
// the excluded rows and compacts the survivors into its LDS slots; lane l then
// owns the survivors l, l + 64, ...: L1I_R independent chains, since a single
// dependent chain of adds leaves the VALU idle between them.
//
// Data movement.  A survivor's row is one contiguous segment of memory but the
// chains want it k-major, so rows go global -> LDS in 16-float chunks,
// transposed: four adjacent lanes load the four float4s of one row's 64-byte
// piece (a wave's load covers 16 whole pieces, 4 L1I_R loads a chunk) and
// store them into the wave's ring xs[2][16][L1I_LD], a row of 64 L1I_R + 4
// floats: 4 x L1I_LD = 16 mod 64 words, so the four k-quarters of a
// transposing store fall in four disjoint sets of 16 banks.  The ring is
// double buffered: chunk c + 1's loads are issued before chunk c's adds.  Per
// k a lane reads its L1I_R row values (stride 1 across the wave) and the query
// value (one address: a broadcast).  Columns >= D are zeroed on the way in;
// +0 changes no bit of these non-negative sums.  The ring belongs to one wave,
// so the loop needs wave barriers only.
//
// k-NN epilogue: wv_fi_select.h as flat_ids_kernel uses it -- fin_key keys, a
// key staged only when below the wave's k-th, the waves merged through their
// stages, then fi_write (one chunk) or part + flat_ids_merge_kernel.  k <= 256;
// the whole key is compared, so hamming's ties go to the lower id.  Threshold
// epilogue: sbd_ids_kernel's -- a row is kept when (double) d - target <= 1e-6,
// its sbd_key appended to the query's segment under seg_cap, and cnt[3q],
// cnt[3q + 1] (d <= target) and cnt[3q + 2] (eligible rows) kept as there.
//
// LDS per workgroup: stages 8 KiB (k-NN only) + slots 4 x L1I_STEP x 4 + the
// query 4 x D rounded up to 16 columns + rings 4 x 2 x 16 x L1I_LD x 4; at
// L1I_R = 2 and D = 128 that is 8,192 + 2,048 + 512 + 67,584 = 78,336 B: two
// workgroups in a CU's 160 KiB.
//
// Built as wv_l1.hip is: no contraction, no packed fp32 forms.
#include "wv_device.h"
#include "wv_fi_select.h"
#include "wv_l1_dev.h"
#include "wv_l1_ring.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_topk.h"

namespace wv {

// dynamic LDS past the stages: slots | query | rings
__host__ __device__ constexpr size_t l1i_lds(int D) {
    return (size_t)4 * L1I_STEP * 4 + (size_t)l1i_dq(D) * 4 + (size_t)4 * L1I_RING * 4;
}

// A workgroup's walk over the list entries [beg, end): the query row staged,
// then wave by wave, step by step, the survivors' distances handed to
// emit(acc, sid, n) -- acc[r] and sid[lane + 64 r] belong together, slots < n.
// lds: the dynamic LDS past the stages (l1i_lds bytes).
template <int METRIC, class Emit>
__device__ __forceinline__ void l1i_walk(const float* __restrict__ X, const float* __restrict__ qrow,
                                         const uint64_t* __restrict__ excl, uint64_t excl_nbits,
                                         const uint32_t* __restrict__ ids, uint64_t beg, uint64_t end, uint64_t n_rows,
                                         int D, int ldx, char* lds, Emit&& emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* sid = reinterpret_cast<uint32_t*>(lds) + wave * L1I_STEP;   // [4][L1I_STEP]
    float* qv = reinterpret_cast<float*>(lds + 4 * L1I_STEP * 4);        // [l1i_dq(D)]
    const int dq = l1i_dq(D);
    float* xs = qv + dq + wave * L1I_RING;                               // [4][2][L1_BK][L1I_LD]
    for (int i = threadIdx.x; i < dq; i += 256) qv[i] = i < D ? qrow[i] : 0.f;
    __syncthreads();
    for (uint64_t i0 = beg + (uint64_t)L1I_STEP * wave; i0 < end; i0 += 4 * L1I_STEP) {
        int n = 0;
#pragma unroll
        for (int r = 0; r < L1I_R; ++r) {
            const uint64_t i = i0 + 64 * r + lane;
            uint32_t id = 0;
            bool ok = false;
            if (i < end) {
                id = ids[i];
                ok = id < n_rows && !bit_test(excl, excl_nbits, id);
            }
            const uint64_t m = __ballot(ok);
            if (ok) sid[n + mbcnt64(m)] = id;
            n += __popcll(m);
        }
        fi_wave_sync();
        if (n == 0) continue;
        float acc[L1I_R];
        l1i_dists<METRIC>(X, ldx, D, sid, n, qv, xs, lane, acc);
        emit(acc, sid, n);
        fi_wave_sync();
    }
}

// grid (ns, n_chunks), 256 threads; dynamic LDS: stage | slots | query | rings
template <int METRIC>
__global__ __launch_bounds__(256) void l1_ids_kernel(FlatIdsParams p) {
    extern __shared__ __attribute__((aligned(16))) char l1i_smem[];
    uint64_t* stage_all = reinterpret_cast<uint64_t*>(l1i_smem);   // [4][FI_STAGE]
    const int s = blockIdx.x, chunk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = p.sel[s];
    uint64_t* stage = stage_all + wave * FI_STAGE;
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)chunk * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;

    uint64_t top[4] = {FI_EMPTY, FI_EMPTY, FI_EMPTY, FI_EMPTY};
    uint64_t kth = FI_EMPTY;
    int cnt = 0;
    l1i_walk<METRIC>(p.X, p.Q + (uint64_t)q * p.dpad, p.excl, p.excl_nbits, p.ids, beg, end, p.n_rows, p.D, p.ldx,
                     l1i_smem + 4 * FI_STAGE * 8, [&](const float (&acc)[L1I_R], const uint32_t* sid, int n) {
#pragma unroll
                         for (int r = 0; r < L1I_R; ++r) {
                             const int slot = lane + 64 * r;
                             const uint64_t key = slot < n ? fin_key(acc[r], sid[slot]) : FI_EMPTY;
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
                     });
    fi_finish<METRIC>(p, top, stage_all, stage, cnt, s, chunk, q, lane, wave);
}

// grid (queries of the chunk, chunks of a list), 256 threads; dynamic LDS:
// slots | query | rings
template <int METRIC>
__global__ __launch_bounds__(256) void l1_sbd_ids_kernel(SbdIdsParams p) {
    extern __shared__ __attribute__((aligned(16))) char l1i_smem[];
    const int qi = blockIdx.x, lane = threadIdx.x & 63;
    if (qi >= p.nq) return;
    const int q = p.q0 + qi;
    const unsigned int seg_cap = (unsigned int)p.seg_cap[qi];
    unsigned long long* keys = p.keys + p.seg_beg[qi];
    const uint64_t l_end = p.off[q + 1];
    uint64_t beg = p.off[q] + (uint64_t)blockIdx.y * p.chunk_len;
    if (beg > l_end) beg = l_end;
    const uint64_t end = l_end - beg > p.chunk_len ? beg + p.chunk_len : l_end;
    const float tf = p.target[q];
    const double t = (double)tf;
    unsigned int n_a = 0, n_ok = 0;   // (lane 0's running counts)
    l1i_walk<METRIC>(p.X, p.Q + (uint64_t)q * p.dpad, p.excl, p.excl_nbits, p.ids, beg, end, p.n_rows, p.D, p.ldx,
                     l1i_smem, [&](const float (&acc)[L1I_R], const uint32_t* sid, int n) {
#pragma unroll
                         for (int r = 0; r < L1I_R; ++r) {
                             const int slot = lane + 64 * r;
                             const float d = acc[r];
                             const uint32_t id = slot < n ? sid[slot] : 0u;
                             const bool in = slot < n && (double)d - t <= 1e-6;
                             const bool below = slot < n && d <= tf;
                             const uint64_t im = __ballot(in);
                             const int ni = __popcll(im);
                             unsigned int base = 0;
                             if (ni) {
                                 if (lane == 0) base = atomicAdd(p.cnt + 3 * q, (unsigned int)ni);
                                 base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
                                 const unsigned int pos = base + (unsigned int)mbcnt64(im);
                                 if (in && pos < seg_cap) keys[pos] = sbd_key(d, id);
                             }
                             n_a += (unsigned int)__popcll(__ballot(below));
                         }
                         n_ok += (unsigned int)n;
                     });
    if (lane == 0 && n_a) atomicAdd(p.cnt + 3 * q + 1, n_a);
    if (lane == 0 && n_ok) atomicAdd(p.cnt + 3 * q + 2, n_ok);
}

}  // namespace wv

namespace {

// what both launchers ask of the operands and the schedule
template <class P>
bool l1_ids_params_ok(const P* p) {
    return (p->metric == WV_METRIC_MANHATTAN || p->metric == WV_METRIC_HAMMING) && ((p->X && p->excl) || p->n_rows == 0) && p->Q &&
           p->ids && p->off && p->D >= 1 && p->ldx >= p->D && p->dpad >= p->D && p->ldx % 4 == 0 &&
           ((uintptr_t)p->X & 15) == 0 && p->dpad <= wv::FLAT_IDS_DPAD_MAX && p->n_chunks >= 1 &&
           p->n_chunks <= 65535 && p->chunk_len != 0 && p->chunk_len % wv::L1I_STEP == 0;
}

}  // namespace

extern "C" {

hipError_t wv_launch_l1_ids(const wv::FlatIdsParams* p, hipStream_t s) {
    if (p->ns == 0) return hipSuccess;
    if (!l1_ids_params_ok(p) || p->ns < 0 || p->k < 1 || p->k > 256 || !p->sel || (p->n_chunks > 1 && !p->part) ||
        !p->out_ids || !p->out_d || !p->out_n)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->ns, (unsigned)p->n_chunks);
    const size_t lds = 4 * wv::FI_STAGE * 8 + wv::l1i_lds(p->D);
    if (p->metric == WV_METRIC_MANHATTAN)
        hipLaunchKernelGGL(wv::l1_ids_kernel<WV_METRIC_MANHATTAN>, grid, dim3(256), lds, s, *p);
    else
        hipLaunchKernelGGL(wv::l1_ids_kernel<WV_METRIC_HAMMING>, grid, dim3(256), lds, s, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p->n_chunks == 1) return e;
    return wv_launch_flat_ids_merge(p, s);   // (never the dot branch: a zero distance is +0)
}

hipError_t wv_launch_l1_sbd_ids(const wv::SbdIdsParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (!l1_ids_params_ok(p) || p->nq < 0 || p->cand_cnt || !p->target || !p->seg_beg || !p->seg_cap || !p->keys ||
        !p->cnt)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->nq, (unsigned)p->n_chunks);
    const size_t lds = wv::l1i_lds(p->D);
    if (p->metric == WV_METRIC_MANHATTAN)
        hipLaunchKernelGGL(wv::l1_sbd_ids_kernel<WV_METRIC_MANHATTAN>, grid, dim3(256), lds, s, *p);
    else
        hipLaunchKernelGGL(wv::l1_sbd_ids_kernel<WV_METRIC_HAMMING>, grid, dim3(256), lds, s, *p);
    return hipGetLastError();
}

}  // extern "C"
