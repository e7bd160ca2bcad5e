// wv_sbd_h16w.hip -- the f16 MFMA threshold filter of SearchByVectorDistance
// for 128 < D <= 1024 (wv_search_by_vector_distance_batch on an uncompressed
// index whose f16 image has the wide layout, h16w_index).
//
// The contract is sbd_h16_kernel's (wv_sbd_h16.hip): per query, every eligible
// row whose scaled f16 key is at most bound[q] is appended to cand[q], counted
// by a returning atomic on ccnt[q], the store guarded by ccap.  The bounds and
// the counts' start come from sbd_h16_bound_kernel, n from
// sbd_h16_count_kernel, and sbd_ids_kernel's candidate form decides among the
// candidates: the answers are the scan's bits.
//
// The D <= 128 design does not carry over: at up to 64 k-steps a wave cannot
// keep its 64 queries' B operands in registers, and the accumulators live
// across D / 32 chunks.  So both operands stream through LDS:
//  * workgroup = 512 threads, 8 waves; grid = corpus segments x query blocks;
//    a workgroup walks its segment's 256-row tiles (HW_BN) against its query
//    block;
//  * a chunk is 32 k (2 sixteen-k steps).  Its A side is the tile's 256 rows x
//    64 B = 16 KiB straight from the image: a 16-row piece's panel is one
//    contiguous 1 KiB run, wave w moves pieces w and w + 8 by LDS-DMA, 16 B a
//    lane, into slot (i % 4) ^ ((row >> 2) & 3) of its row, so the MFMA's
//    ds_read_b128 lane groups hit distinct banks (wv_bf_h16w_kernel's
//    swizzle).  Its B side is the block's QB / 32 query groups x 2 steps x
//    1 KiB of the h16_index query image, as is;
//  * chunks go through a ring of 3 stages: wait for chunk g (a counted vmcnt:
//    chunk g + 1 stays in flight), barrier, issue chunk g + 2 between the
//    chunk's two k-steps, compute g.  The sources are running wave-uniform
//    pointers (SGPR base + a fixed per-lane offset): no per-chunk index math;
//  * nothing else goes through LDS but, for L2, the tile's 256 s |x|^2 values
//    (a 2-slot ring, issued by wave 7 with the tile's first chunk): no row
//    list, no tile mask words, no running thresholds.
//
// Query-block shapes (QB, chosen by the host):
//  * QB = 256 (batches above 64): wave w computes rows 128 (w & 1).. x queries
//    64 (w >> 1)..: 4 row groups x 2 column blocks = 8 accumulators of
//    v_mfma_f32_32x32x16_f16.  A tile is read once per 256 queries; 3 x 32 KiB
//    of LDS, one workgroup per CU;
//  * QB = 64 (batches of up to 64): the 8 waves split the tile's rows, 32 rows
//    x 64 queries each (2 accumulators); the B chunk is 4 KiB, filled by waves
//    0-3; 3 x 20 KiB of LDS, two workgroups per CU.  One query still spreads
//    the corpus over every CU and the pass is a single read of the f16 image.
//
// Epilogue, once per tile: the minimum of each accumulator against the
// query's bound and one wave-wide "any" -- the miss path is those compares and
// a branch.  On a hit the lane takes, per accumulator, the half words of the
// exclusion bitmap and of its allow list (none, shared, or the query's own
// row) that cover the group's 32 rows, clipped to the segment's end and N, and
// appends the rows whose key is under the bound and whose bit is set.  Padding
// columns of a partial block carry a bound of -inf; tiles past the segment's
// end are never read (the image ends with the corpus's last tile).
//
// Measured at 1M x 768 dot (profiles/sbd_h16w/README.md): whole calls 1.5x /
// 1.3x the scan's speed at one query, 14x / 6.9x at 64 and 24x / 20x at 1024
// with about 100 / 5,000 rows within the target; the kernel takes 0.25 ms at
// one query (the 1.5 GB image at 6.2 TB/s) and 1.67 ms at 1024 (0.96 Pflop/s).
// Follow-ups, out of scope here: the Go binding, and the switch
// (wv_index_set_sbd_wide_key_pass) as the default.
#include "wv_h16_dev.h"
#include "wv_launch.h"

namespace wv {

template <int QB>
struct SbdH16WStage {
    static constexpr int KC = HW_KC / 2;             // 16-k steps per chunk
    static constexpr int QG = QB / 32;               // 32-query groups per block
    static constexpr int A_U4 = HW_BN * KC * 2;      // 256 rows x 32 KC bytes (16 KiB)
    static constexpr int B_U4 = QG * KC * 64;        // QG groups x KC steps x 64 lanes
    static constexpr int U4 = A_U4 + B_U4;
};
constexpr int SBDW_STAGES = 3;
constexpr int SBDW_XN_BYTES = 2 * HW_BN * 4;         // the 2-slot ring of s |x|^2 (L2)

template <bool L2, int QB>
__global__ __launch_bounds__(512, QB == 64 ? 4 : 2) void sbd_h16w_kernel(SbdH16WParams p) {
    using St = SbdH16WStage<QB>;
    constexpr int KC = St::KC, BN = HW_BN;
    static_assert(KC == 2, "a chunk is one 64 B panel per row");
    constexpr int RG = QB == 256 ? 4 : 1;            // 32-row groups per wave
    constexpr int BJ = QB == 256 ? KC : 1;           // query blocks a filling wave moves per chunk
    extern __shared__ uint4 lds[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg0 = QB == 256 ? RG * (wave & 1) : wave;   // the wave's first row group of a tile
    const int qq = QB == 256 ? wave >> 1 : 0;             // its 64-query column of the block
    const int qb = blockIdx.y;
    const uint32_t t_begin = blockIdx.x * p.tiles_per_seg;
    if (t_begin >= p.ntiles) return;
    const uint32_t t_end = min(t_begin + p.tiles_per_seg, p.ntiles);
    const uint32_t r_end = (uint32_t)min((uint64_t)t_end * BN, p.N);   // rows this workgroup answers for
    const int ns = p.ns, nch = ns / KC;
    const int nchunks = (int)(t_end - t_begin) * nch;

    const int jq0 = qb * QB + qq * 64 + l31, jq1 = jq0 + 32;
    const float NINF = -__builtin_inff();
    float b0 = jq0 < p.nq ? p.bound[jq0] : NINF;
    float b1 = jq1 < p.nq ? p.bound[jq1] : NINF;
    // (landed before the first LDS-DMA: a wait for them inside the tile loop
    // would drain the chunk stream at every epilogue)
    asm volatile("" : "+v"(b0), "+v"(b1));

    const uint32_t lds0 = lds_addr(lds);
    const uint32_t xn0 = lds0 + (uint32_t)(SBDW_STAGES * St::U4 * 16);
    const float* xn_lds = reinterpret_cast<const float*>(lds + SBDW_STAGES * St::U4);

    // The chunk stream.  A side: pieces wave and wave + 8 of the tile (16-row
    // groups 16 tile + piece of the image, ns * 512 B each, the chunk's panel
    // at + 1 KiB per chunk); lane i moves 16 B of row i / 4, the source slot
    // swizzled.  B side: block b = wave + 8 j of the chunk's QG * KC (group
    // b / KC, step b % KC).  A wave's ops per chunk are fixed, so the counted
    // wait is `ops` (the extras of a tile's first chunk only make it wait for
    // more).
    const bool bfill = QB == 256 || wave < St::QG * KC;
    const int ops = 2 + (bfill ? BJ : 0);
    const uint64_t gsb = (uint64_t)ns * 512;   // bytes per 16-row group (= nch chunks of 1 KiB)
    const uint32_t a_voff = (uint32_t)((lane >> 2) * 64 + 16 * ((lane & 3) ^ ((lane >> 4) & 3)));
    const uint32_t b_voff = (uint32_t)(lane * 16);
    const char* a_cur = reinterpret_cast<const char*>(p.X) + ((uint64_t)t_begin * 16 + (uint64_t)wave) * gsb;
    const uint4* b_src0 =
        reinterpret_cast<const uint4*>(p.Q) + (((uint64_t)qb * St::QG + (uint64_t)(wave / KC)) * ns + (wave % KC)) * 64;
    const uint64_t b_gstride = (uint64_t)(8 / KC) * ns * 64;   // 8 / KC groups, in uint4
    const uint4* b_cur = b_src0;
    int ft = 0, fc = 0;   // the next chunk to fill: (tile, chunk)
    auto fill_next = [&](int stage) {
        ft = __builtin_amdgcn_readfirstlane(ft);
        fc = __builtin_amdgcn_readfirstlane(fc);
        stage = __builtin_amdgcn_readfirstlane(stage);
        const uint32_t dst = lds0 + (uint32_t)(stage * St::U4 * 16) + (uint32_t)(wave * 1024);
        const char* a = uniform_ptr(a_cur);
        const uint4* b = uniform_ptr(b_cur);
        glds16s(a, a_voff, dst);
        glds16s(uniform_ptr(a + 8 * gsb), a_voff, dst + 8 * 1024);
        if (bfill) {
#pragma unroll
            for (int j = 0; j < BJ; ++j)
                glds16s(uniform_ptr(b + j * b_gstride), b_voff, dst + (uint32_t)(St::A_U4 * 16 + 8 * j * 1024));
        }
        if (L2 && fc == 0 && wave == 7) {
            const float* xs = p.xns + (uint64_t)(t_begin + (uint32_t)ft) * BN + lane;
#pragma unroll
            for (int j = 0; j < BN / 64; ++j) glds4(xs + 64 * j, xn0 + (uint32_t)((ft & 1) * BN * 4 + 256 * j));
        }
        a_cur = a + KC * 512;
        b_cur = b + KC * 64;
        if (++fc == nch) {   // the next tile's groups: 16 on; the queries start over
            fc = 0;
            ++ft;
            a_cur = a + KC * 512 + 15 * gsb;
            b_cur = b_src0;
        }
    };

    // the keys of one accumulator under the bound: eligibility, then the append
    auto append = [&](const floatx16& acc, float b, int jq, uint32_t row0) {
        if (jq >= p.nq) return;   // (a padding column's bound is -inf; never a store past the lists)
        // The group's 32 rows start at a multiple of 32: their exclusion and
        // allow bits are one 32-bit half word each (bit_test's answers: a row
        // at or past a bitmap's length is not excluded / not allowed), clipped
        // to the rows this workgroup answers for (row0 < r_end).
        auto word = [&](const uint64_t* bits, uint64_t nbits) -> uint32_t {
            if ((uint64_t)row0 >= nbits) return 0u;
            const uint32_t w = reinterpret_cast<const uint32_t*>(bits)[row0 >> 5];
            return nbits - row0 < 32 ? w & ((1u << (uint32_t)(nbits - row0)) - 1u) : w;
        };
        uint32_t ok = ~word(p.excl, p.excl_nbits);
        if (p.allow) ok &= word(p.allow + (p.allow_stride ? (uint64_t)jq * p.allow_stride : 0), p.allow_nbits);
        if (r_end - row0 < 32) ok &= (1u << (r_end - row0)) - 1u;
        ok >>= 4 * khalf;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int bit = (r & 3) + 8 * (r >> 2);   // (the 32x32 accumulator's row order, + 4 khalf)
            if (!(acc[r] <= b) || !((ok >> bit) & 1u)) continue;
            const unsigned int pos = atomicAdd(p.ccnt + jq, 1u);
            if (pos < (unsigned int)p.ccap) p.cand[(uint64_t)jq * p.ccap + pos] = row0 + (uint32_t)(bit + 4 * khalf);
        }
    };
    auto min16 = [](const floatx16& a) {
        float m0 = fminf(fminf(a[0], a[1]), a[2]), m1 = fminf(fminf(a[3], a[4]), a[5]);
        float m2 = fminf(fminf(a[6], a[7]), a[8]), m3 = fminf(fminf(a[9], a[10]), a[11]);
        m0 = fminf(fminf(m0, a[12]), a[13]);
        m1 = fminf(fminf(m1, a[14]), a[15]);
        return fminf(fminf(m0, m1), fminf(m2, m3));
    };

    floatx16 acc[RG][2];
    fill_next(0);
    if (nchunks > 1) fill_next(1);
    int t = 0, c = 0, stg = 0;   // the chunk computed: (tile, chunk), its stage
    for (int g = 0; g < nchunks; ++g) {
        // chunk g landed, for every wave; chunk g + 1 (its first `ops` ops) may stay in flight
        if (g + 1 < nchunks) vm_wait(ops);
        else vm_wait(0);
        block_barrier();
        const uint4* st = lds + stg * St::U4;
        if (c == 0) {
            // C-in: s |x|^2 of the wave's rows in the accumulator's row order (L2) or zero
#pragma unroll
            for (int i = 0; i < RG; ++i) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (L2) v = *reinterpret_cast<const float4*>(xn_lds + (t & 1) * BN + 32 * (rg0 + i) + 4 * khalf + 8 * g4);
                    acc[i][0][4 * g4] = v.x; acc[i][0][4 * g4 + 1] = v.y;
                    acc[i][0][4 * g4 + 2] = v.z; acc[i][0][4 * g4 + 3] = v.w;
                }
                acc[i][1] = acc[i][0];
            }
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const half8 q0 = __builtin_bit_cast(half8, st[St::A_U4 + ((2 * qq) * KC + k) * 64 + lane]);
            const half8 q1 = __builtin_bit_cast(half8, st[St::A_U4 + ((2 * qq + 1) * KC + k) * 64 + lane]);
            // row 32 G + l31's 16 B unit 2 k + khalf of the chunk (swizzled slot)
            const int aslot = 4 * l31 + ((2 * k + khalf) ^ ((l31 >> 2) & 3));
            half8 a[RG];
#pragma unroll
            for (int i = 0; i < RG; ++i) a[i] = __builtin_bit_cast(half8, st[128 * (rg0 + i) + aslot]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < RG; ++i) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], q0, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], q1, acc[i][1], 0, 0, 0);
            }
            if (k == 0) {
                // the stage chunk g - 1 was computed from, free since this chunk's barrier
                __builtin_amdgcn_sched_barrier(0);
                if (g + 2 < nchunks) fill_next(stg == 0 ? 2 : stg - 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        stg = stg == 2 ? 0 : stg + 1;
        if (++c != nch) continue;
        c = 0;
        // ---- tile epilogue ----
        const uint32_t row0 = (t_begin + (uint32_t)t) * BN + 32u * (uint32_t)rg0;
        ++t;
        if (row0 >= r_end) continue;   // (wave-uniform)
        bool hit = false;
#pragma unroll
        for (int i = 0; i < RG; ++i) hit = hit || min16(acc[i][0]) <= b0 || min16(acc[i][1]) <= b1;
        if (__builtin_expect(wave_any(hit), 0)) {
#pragma unroll
            for (int i = 0; i < RG; ++i) {
                append(acc[i][0], b0, jq0, row0 + 32u * i);
                append(acc[i][1], b1, jq1, row0 + 32u * i);
            }
        }
    }
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_sbd_h16w(const wv::SbdH16WParams* p, hipStream_t s) {
    if (p->nq == 0 || p->ntiles == 0) return hipSuccess;
    const int qb = p->qblock;
    if (p->ns < wv::HW_KC || p->ns > wv::HW_NS_MAX || p->ns % wv::HW_KC || (qb != 64 && qb != wv::HW_BQ) || !p->X ||
        !p->Q || !p->bound || !p->excl || !p->cand || !p->ccnt || p->ccap < 1 || p->tiles_per_seg < 1 || p->n_seg < 1 ||
        p->n_qblocks < 1 || p->n_qblocks > 65535 || (uint64_t)p->n_qblocks * qb < (uint64_t)p->nq ||
        (uint64_t)p->n_seg * p->tiles_per_seg < p->ntiles || (uint64_t)p->ntiles * wv::HW_BN < p->N ||
        (uint64_t)(p->ntiles - 1) * wv::HW_BN >= p->N || p->N > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const bool l2 = p->metric == WV_METRIC_L2;
    if (l2 && !p->xns) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->n_seg, (unsigned)p->n_qblocks);
#define WV_SBDW_GO(L, QB)                                                                                     \
    {                                                                                                         \
        const size_t lds = (size_t)wv::SBDW_STAGES * wv::SbdH16WStage<QB>::U4 * 16 + (L ? wv::SBDW_XN_BYTES : 0); \
        hipLaunchKernelGGL((wv::sbd_h16w_kernel<L, QB>), grid, dim3(512), lds, s, *p);                         \
    }
    if (qb == 64) { if (l2) WV_SBDW_GO(true, 64) else WV_SBDW_GO(false, 64) }
    else { if (l2) WV_SBDW_GO(true, 256) else WV_SBDW_GO(false, 256) }
#undef WV_SBDW_GO
    return hipGetLastError();
}

}  // extern "C"
