// wv_sbd_h16.hip -- the f16 MFMA threshold filter of SearchByVectorDistance
// (wv_search_by_vector_distance_batch on an uncompressed index, D <= 128).
//
// The exact rounds of a distance search ask, per query, for the rows with
// (double)d - (double)target <= 1e-6, d the reference-order fp32 distance.
// sbd_scan_kernel (wv_sbd.hip) answers by computing every d of every query on
// the VALU, one sweep of the fp32 corpus per query.  This pass answers the
// same question in two stages: a filter over the resident f16 image that
// shares one read of a corpus tile among all the queries of a block and
// computes on the matrix cores, and an exact stage over the few rows the
// filter lets through (sbd_ids_kernel's candidate form).  The filter is
// certified: with key the f16 MFMA key of a (query, row) pair (the k-NN key
// pass's operands: B = f16(s_q b), b = -2q or -q, the L2 accumulator started
// at s |x|^2), h16_eps bounds |key + offset - d| for every row, offset = |q|^2
// (L2), 0 (dot) or 1 (cosine).  So every row of the answer has
//     key <= target + 1e-6 - offset + eps,
// and the prologue kernel writes that bound per query, in the kernel's scaled
// key units (times s = s_x s_q, a power of two) and rounded upward.  What the
// filter passes is a superset; the exact stage decides, so the answers are the
// scan's bits.
//
// Work split (one 512-thread workgroup of 8 waves):
//  * grid = corpus segments x query blocks; a workgroup keeps its query
//    block's B operands in registers for its whole run (a wave holds 64
//    queries: 2 column blocks x NS k-steps of v_mfma_f32_32x32x16_f16) and
//    walks its segment of 64-row tiles;
//  * the tiles stream global -> registers -> LDS in stages, double buffered:
//    the loads of stage i + 1 are issued before the MFMAs of stage i and
//    stored after them, one barrier per stage.  The image is MFMA-native
//    (h16_index), so a stage is one contiguous run of it and an A fragment is
//    one 16-byte LDS read per lane;
//  * QW, the waves across the queries, is the template parameter that sets
//    the query-block width.  QW = 1 (64 queries: batches of up to 64): the 8
//    waves split the rows of a 4-tile stage, a 32-row half tile each, so one
//    query still spreads the corpus over every CU and the pass is a single
//    read of the f16 image.  QW = 8 (512 queries): each wave computes the
//    stage's rows against its own 64 queries, so a tile is read once per 512
//    queries instead of once per query.
//
// Hit path: after a half tile's MFMAs a lane holds 16 keys of one query per
// accumulator; their minimum is compared with the query's bound and a
// wave-wide "any" decides whether anything else happens -- the miss path is
// that compare and a branch.  On a hit the lane finds the keys under the
// bound, and only then tests the row: below N and the segment's end, not
// excluded, allowed (no list, a shared bitmap, or the query's own bitmap row;
// no tile masks anywhere).  An eligible row is appended to the query's
// candidate list at the position a returning atomic on the query's count
// gives; the store is guarded by the capacity, the count keeps counting, and
// a query that outgrows its list is answered by sbd_scan_kernel instead
// (wv_distance.hip).  Padding columns of a partial block carry a bound of
// -inf, like a NaN or -inf target: nothing passes.
//
// The third count of the host arithmetic, n (the rows the search could
// return), is counted from the bitmaps alone (sbd_h16_count_kernel), once for
// a shared or absent list.
//
// D > 128 (the wide image layout) has a filter of its own: wv_sbd_h16w.hip.
// Follow-ups, out of scope here: the Go binding, and making the switch
// (wv_index_set_sbd_key_pass) the default.
// Measured at 1M x 128 (profiles/sbd_h16/README.md): 3.3x / 1.5x the scan's
// speed at 64 queries and 4.5x / 3.9x at 1024 with about 100 / 5,000 rows
// within the target; a single query is 10 % faster with 100 rows within and
// 5 % slower with 5,000 (0.43 against 0.41 ms), where the launches around the
// filter outweigh the halved read.  No batch-size floor is applied.
#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"
#include "wv_topk.h"

#include <float.h>

namespace wv {

typedef _Float16 sbdh_half8 __attribute__((ext_vector_type(8)));

template <int NS, int QW>
struct SbdH16Stage {
    static constexpr int TPS = QW == 1 ? 4 : 2;      // 64-row tiles per stage
    static constexpr int NG = 2 * TPS;               // 32-row groups per stage
    static constexpr int IMG_U4 = NG * NS * 64;      // image words of a stage
    static constexpr int ROWS = 64 * TPS;
    static constexpr int U4 = IMG_U4 + ROWS / 4;     // + the rows' s |x|^2
};

template <int NS, bool L2, int QW>
__global__ __launch_bounds__(512) void sbd_h16_kernel(SbdH16Params p) {
    using St = SbdH16Stage<NS, QW>;
    constexpr int RW = SBDH_WAVES / QW;              // waves across a stage's rows
    constexpr int LPT = (St::IMG_U4 + 511) / 512;    // image words a thread moves per stage
    constexpr int TILE_U4 = 2 * NS * 64;
    extern __shared__ uint4 lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave % QW, wr = wave / QW;
    const int qb = blockIdx.y;
    const uint32_t t_begin = blockIdx.x * p.tiles_per_seg;
    if (t_begin >= p.ntiles) return;
    const uint32_t t_end = min(t_begin + p.tiles_per_seg, p.ntiles);
    const uint32_t r_end = (uint32_t)min((uint64_t)t_end * 64, p.N);   // rows this workgroup answers for

    // the wave's 64 queries: B operands and bounds, for the whole segment
    const uint4* __restrict__ Qg = reinterpret_cast<const uint4*>(p.Q);
    uint4 bq0[NS], bq1[NS];
    const uint64_t cb = (uint64_t)qb * (2 * QW) + 2 * wq;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        bq0[k] = Qg[(cb * NS + k) * 64 + lane];
        bq1[k] = Qg[((cb + 1) * NS + k) * 64 + lane];
    }
    const int jq0 = (int)cb * 32 + l31, jq1 = jq0 + 32;
    const float NINF = -__builtin_inff();
    const float b0 = jq0 < p.nq ? p.bound[jq0] : NINF;
    const float b1 = jq1 < p.nq ? p.bound[jq1] : NINF;

    const uint4* __restrict__ X = reinterpret_cast<const uint4*>(p.X);
    uint4 st_img[LPT];
    float st_xn = 0.f;
    // a stage's tiles past the segment's end are not read (the image ends
    // with the corpus's last tile) and their rows never pass r_end
    auto fetch = [&](uint32_t t0) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + 512 * i;
            st_img[i] = make_uint4(0, 0, 0, 0);
            if (idx < St::IMG_U4 && t0 + (uint32_t)(idx / TILE_U4) < t_end) st_img[i] = X[(uint64_t)t0 * TILE_U4 + idx];
        }
        if (L2 && tid < St::ROWS) st_xn = t0 + (uint32_t)(tid >> 6) < t_end ? p.xns[(uint64_t)t0 * 64 + tid] : 0.f;
    };
    auto stash = [&](int buf) {
        uint4* img = lds + buf * St::U4;
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + 512 * i;
            if (idx < St::IMG_U4) img[idx] = st_img[i];
        }
        if (L2 && tid < St::ROWS) reinterpret_cast<float*>(img + St::IMG_U4)[tid] = st_xn;
    };
    // the keys of one accumulator under the bound: eligibility, then the append
    auto append = [&](const floatx16& acc, float b, int jq, uint32_t row0) {
        if (jq >= p.nq) return;   // (a padding column's bound is -inf; never a store past the lists)
        const uint64_t* allow = p.allow ? p.allow + (p.allow_stride ? (uint64_t)jq * p.allow_stride : 0) : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!(acc[r] <= b)) continue;
            const uint32_t row = row0 + (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * khalf);
            if (row >= r_end || bit_test(p.excl, p.excl_nbits, row)) continue;
            if (allow && !bit_test(allow, p.allow_nbits, row)) continue;
            const unsigned int pos = atomicAdd(p.ccnt + jq, 1u);
            if (pos < (unsigned int)p.ccap) p.cand[(uint64_t)jq * p.ccap + pos] = row;
        }
    };
    auto min16 = [](const floatx16& a) {
        float m0 = fminf(fminf(a[0], a[1]), a[2]), m1 = fminf(fminf(a[3], a[4]), a[5]);
        float m2 = fminf(fminf(a[6], a[7]), a[8]), m3 = fminf(fminf(a[9], a[10]), a[11]);
        m0 = fminf(fminf(m0, a[12]), a[13]);
        m1 = fminf(fminf(m1, a[14]), a[15]);
        return fminf(fminf(m0, m1), fminf(m2, m3));
    };

    fetch(t_begin);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t t0 = t_begin; t0 < t_end; t0 += St::TPS, buf ^= 1) {
        const bool more = t0 + St::TPS < t_end;
        if (more) fetch(t0 + St::TPS);
        const uint4* img = lds + buf * St::U4;
        const float* xn = reinterpret_cast<const float*>(img + St::IMG_U4);
#pragma unroll
        for (int g = wr; g < St::NG; g += RW) {
            const uint32_t row0 = t0 * 64 + (uint32_t)g * 32;
            if (row0 >= r_end) break;   // (wave-uniform)
            floatx16 acc0, acc1;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (L2) v = *reinterpret_cast<const float4*>(xn + 32 * g + 4 * khalf + 8 * g4);
                acc0[4 * g4] = v.x; acc0[4 * g4 + 1] = v.y; acc0[4 * g4 + 2] = v.z; acc0[4 * g4 + 3] = v.w;
            }
            acc1 = acc0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const sbdh_half8 a = __builtin_bit_cast(sbdh_half8, img[(g * NS + k) * 64 + lane]);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(sbdh_half8, bq0[k]), acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(sbdh_half8, bq1[k]), acc1, 0, 0, 0);
            }
            const bool hit = min16(acc0) <= b0 || min16(acc1) <= b1;
            if (__builtin_expect(wave_any(hit), 0)) {
                append(acc0, b0, jq0, row0);
                append(acc1, b1, jq1, row0);
            }
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
    }
}

// One bound per query, in scaled key units: (target + 1e-6 - offset + eps) s,
// the sum in float64 (every term is exact there; its own rounding, 2^-53 of
// the largest term, is added back a thousandfold), one part in 10^6 on top as
// h16_eps adds its 1.0001, then rounded up to a float.  ccnt starts at 0.  A
// target of NaN or -inf admits nothing: bound -inf.  A query the filter cannot
// bound -- a target of +inf, or a certificate or scale that is not finite --
// starts past its capacity instead, which sends it to the scan.
__global__ void sbd_h16_bound_kernel(SbdH16BoundParams p) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.nq) return;
    const float INF = __builtin_inff();
    const float t = p.target[q], s = p.sx * p.qscale[0];
    const float eps = h16_eps(p.metric, p.D, p.qnorm[q], p.xnorm_max, p.ex_max, p.qres[q]);
    const float off = p.metric == WV_METRIC_L2 ? p.qnorm[q] : (p.metric == WV_METRIC_DOT ? 0.f : 1.f);
    float b = -INF;
    bool scan = false;
    if (!(eps < INF) || !(s > 0.f && s < INF) || !(fabsf(off) < INF)) scan = true;
    else if (!(t > -INF)) b = -INF;
    else if (!(t < INF)) scan = true;
    else {
        const double mag = fabs((double)t) + fabs((double)off) + (double)eps + 1e-6;
        double bt = ((double)t + 1e-6 - (double)off + (double)eps + mag * 1e-12) * (double)s;
        bt += fabs(bt) * 1e-6;
        b = (float)bt;
        if ((double)b < bt) b = nextafterf(b, INF);
        if (!(b < INF)) { b = -INF; scan = true; }
    }
    p.bound[q] = b;
    p.ccnt[q] = scan ? (unsigned int)p.ccap + 1u : 0u;
}

// n of the host arithmetic from the bitmaps alone: the rows below N that are
// not excluded and that the list allows -- grid (words / 256, lists): one list
// row for a shared or absent list, else one per query.  n_elig is zeroed by
// the caller.
__global__ __launch_bounds__(256) void sbd_h16_count_kernel(const uint64_t* excl, const uint64_t* allow,
                                                            uint64_t allow_nbits, uint64_t allow_stride, uint64_t N,
                                                            unsigned int* n_elig) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x, words = (N + 63) / 64;
    uint64_t b = 0;
    if (w < words) {
        b = ~excl[w];
        if (w == words - 1 && (N & 63)) b &= (1ull << (N & 63)) - 1;
        if (allow) {
            const uint64_t aw = (allow_nbits + 63) / 64;
            uint64_t a = w < aw ? allow[(uint64_t)blockIdx.y * allow_stride + w] : 0ull;
            if (w + 1 == aw && (allow_nbits & 63)) a &= (1ull << (allow_nbits & 63)) - 1;
            b &= a;
        }
    }
    unsigned int c = (unsigned int)__popcll(b);
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_elig + blockIdx.y, c);
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_sbd_h16_bound(const wv::SbdH16BoundParams* p, hipStream_t s) {
    if (p->nq == 0) return hipSuccess;
    if (p->ccap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::sbd_h16_bound_kernel, dim3((p->nq + 255) / 256), dim3(256), 0, s, *p);
    return hipGetLastError();
}

hipError_t wv_launch_sbd_h16_count(const uint64_t* excl, const uint64_t* allow, uint64_t allow_nbits,
                                   uint64_t allow_stride, uint64_t N, int nq, unsigned int* n_elig, hipStream_t s) {
    if (N == 0 || nq == 0) return hipSuccess;
    const uint64_t blocks = ((N + 63) / 64 + 255) / 256;
    const int lists = allow && allow_stride ? nq : 1;
    if (blocks > 0x7FFFFFFFull || lists > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wv::sbd_h16_count_kernel, dim3((unsigned)blocks, (unsigned)lists), dim3(256), 0, s, excl, allow,
                       allow_nbits, allow_stride, N, n_elig);
    return hipGetLastError();
}

hipError_t wv_launch_sbd_h16(const wv::SbdH16Params* p, hipStream_t s) {
    if (p->nq == 0 || p->ntiles == 0) return hipSuccess;
    const int qw = p->qwaves;
    if (p->ns < 1 || p->ns > wv::H_NS_MAX || (qw != 1 && qw != wv::SBDH_WAVES) || !p->X || !p->Q || !p->bound ||
        !p->excl || !p->cand || !p->ccnt || p->ccap < 1 || p->tiles_per_seg < 1 || p->n_seg < 1 || p->n_qblocks < 1 ||
        p->n_qblocks > 65535 || (uint64_t)p->n_qblocks * 64 * qw < (uint64_t)p->nq ||
        (uint64_t)p->n_seg * p->tiles_per_seg < p->ntiles || (uint64_t)p->ntiles * 64 < p->N ||
        (uint64_t)(p->ntiles - 1) * 64 >= p->N || p->N > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const bool l2 = p->metric == WV_METRIC_L2;
    if (l2 && !p->xns) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->n_seg, (unsigned)p->n_qblocks);
#define WV_SBDH_GO(NS, L, QW)                                                   \
    {                                                                           \
        const size_t lds = (size_t)2 * wv::SbdH16Stage<NS, QW>::U4 * 16;        \
        hipLaunchKernelGGL((wv::sbd_h16_kernel<NS, L, QW>), grid, dim3(512), lds, s, *p); \
    }
#define WV_SBDH_LAUNCH(NS)                                                          \
    if (qw == 1) { if (l2) { WV_SBDH_GO(NS, true, 1) } else { WV_SBDH_GO(NS, false, 1) } } \
    else { if (l2) { WV_SBDH_GO(NS, true, wv::SBDH_WAVES) } else { WV_SBDH_GO(NS, false, wv::SBDH_WAVES) } }
    switch (p->ns) {
        case 1: WV_SBDH_LAUNCH(1) break;
        case 2: WV_SBDH_LAUNCH(2) break;
        case 3: WV_SBDH_LAUNCH(3) break;
        case 4: WV_SBDH_LAUNCH(4) break;
        case 5: WV_SBDH_LAUNCH(5) break;
        case 6: WV_SBDH_LAUNCH(6) break;
        case 7: WV_SBDH_LAUNCH(7) break;
        default: WV_SBDH_LAUNCH(8) break;
    }
#undef WV_SBDH_LAUNCH
#undef WV_SBDH_GO
    return hipGetLastError();
}

}  // extern "C"
