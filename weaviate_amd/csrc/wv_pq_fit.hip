// wv_pq_fit.hip -- ProductQuantizer.Fit with KMeans encoders on the device.
//
// adapters/repos/db/vector/ssdhelpers/product_quantization.go:312-336 runs one
// KMeans.Fit (kmeans.go:118-226) per segment; the segments are independent, so
// a group of them runs side by side here, one round of the reference's loop
// per pass over the rows:
//   * pq_fit_assign_kernel: recluster (:134-148).  Nearest is
//     wv_pq_encode_kernel's rule -- asm_l2_serial, centres ascending, the LAST
//     of equal distances wins -- with the segment's centres staged in LDS.
//   * wv_pq_fit_sort: the member lists m.data.cc in ascending j, as a stable
//     radix sort of (segment, cluster) -> j plus the clusters' bounds.
//   * pq_fit_empty_kernel: resortOnEmptySets (:150-170), sequential per
//     segment, the two rand.Intn draws replaced by a counter-based generator.
//   * pq_fit_centre_kernel: recalcCenters (:172-189): fp32 sums in list
//     order, one add per member, then one correctly rounded division.
// The host loop (wv_index_fit_pq, wv_api.hip) reads `changes` back once per
// round and applies stopCondition (:191-194) per segment.
#include <hipcub/hipcub.hpp>

#include "wv_device.h"
#include "wv_launch.h"
#include "wv_params.h"

namespace wv {

namespace {

constexpr uint32_t FIT_NIL = 0xFFFFFFFFu;

// draw_level's mixer (wv_build.hip)
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// the position in [0, n) drawn for (segment, round, centre, attempt)
__device__ __forceinline__ uint64_t fit_draw(uint64_t seed, uint64_t seg, uint64_t round, uint64_t ci, uint64_t a,
                                             uint64_t n) {
    const uint64_t ctr = seg << 40 | round << 32 | ci << 8 | a;
    return mix64(seed * 0xD1B54A32D192ED03ull + ctr * 0x9E3779B97F4A7C15ull + 1) % n;
}

__device__ __forceinline__ uint64_t fit_row(const PqFitParams& p, uint64_t j) { return p.rowmap ? p.rowmap[j] : j; }

}  // namespace

// initCenters (:118-132): centre i of segment s = the slice of the row drawn
// with round 15, with replacement.  One thread per table element.
__global__ __launch_bounds__(256) void pq_fit_init_kernel(PqFitParams p, int m) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_seg = (uint64_t)p.ks * p.ds;
    if (t >= per_seg * m) return;
    const uint64_t s = t / per_seg, c = (t % per_seg) / p.ds;
    const int d = (int)(t % p.ds);
    const uint64_t j = fit_draw(p.seed, s, 15, c, 0, p.n);
    p.cent[t] = p.X[fit_row(p, j) * p.ldx + s * p.ds + d];
}

// val[sl][j] = j: the sort's payload, written once per group
__global__ __launch_bounds__(256) void pq_fit_iota_kernel(PqFitParams p) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.n) return;
    p.val[(uint64_t)blockIdx.y * p.n + j] = (uint32_t)j;
}

// grid: x over 256-row tiles, y over the group's segments.  DS > 0: the row
// slice lives in registers (ds == DS); DS == 0: any ds, the slice read where
// it lies.  Centres come from LDS in chunks of p.cc (p.cc == 0: a single
// centre outgrows the chunk, they are read from the table).
template <int DS>
__global__ __launch_bounds__(256) void pq_fit_assign_kernel(PqFitParams p) {
    extern __shared__ float fit_lds[];
    const int sl = blockIdx.y;
    if (!p.active[sl]) return;   // this segment has stopped (uniform per workgroup)
    const int ds = DS ? DS : p.ds;
    const int s = p.s0 + sl;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = j < p.n;
    const float* xg = p.X + (valid ? fit_row(p, j) : 0) * p.ldx + (uint64_t)s * ds;
    float xr[DS ? DS : 1];
    if (DS) {
#pragma unroll
        for (int i = 0; i < (DS ? DS : 1); ++i) xr[i] = valid ? xg[i] : 0.f;
    }
    const float* x = DS ? xr : xg;
    const float* cs = p.cent + (uint64_t)s * p.ks * ds;
    uint32_t best = 0;
    float bd = 3.40282346638528859812e+38f;   // math.MaxFloat32
    if (p.cc == 0) {
        if (valid)
            for (int c = 0; c < p.ks; ++c) {
                const float d = asm_l2_serial(x, cs + (uint64_t)c * ds, ds);
                if (!(bd < d)) { bd = d; best = (uint32_t)c; }
            }
    } else {
        for (int c0 = 0; c0 < p.ks; c0 += p.cc) {
            const int cn = min(p.cc, p.ks - c0);
            __syncthreads();   // the previous chunk has been read
            for (int i = threadIdx.x; i < cn * ds; i += blockDim.x) fit_lds[i] = cs[(uint64_t)c0 * ds + i];
            __syncthreads();
            if (valid)
                for (int c = 0; c < cn; ++c) {
                    const float d = asm_l2_serial(x, fit_lds + c * ds, ds);
                    if (!(bd < d)) { bd = d; best = (uint32_t)(c0 + c); }   // the running best crosses chunks
                }
        }
    }
    bool changed = false;
    if (valid) {
        const uint64_t o = (uint64_t)sl * p.n + j;
        changed = p.points[o] != best;
        p.points[o] = best;
        p.key[o] = (uint32_t)sl * (uint32_t)p.ks + best;
    }
    const unsigned long long b = __ballot(changed);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(p.changes + sl, (uint32_t)__popcll(b));
}

// start[q] = the first sorted position whose key is >= q, for q in [0, nkeys]
__global__ __launch_bounds__(256) void pq_fit_bounds_kernel(const uint32_t* __restrict__ skey, uint64_t total,
                                                            uint32_t nkeys, uint32_t* __restrict__ start) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t k = skey[t];
    const uint32_t lo = t ? skey[t - 1] + 1 : 0;
    for (uint32_t q = lo; q <= k; ++q) start[q] = (uint32_t)t;
    if (t == total - 1)
        for (uint32_t q = k + 1; q <= nkeys; ++q) start[q] = (uint32_t)total;
}

// One wave per segment.  The lanes look for empty clusters 64 at a time; lane
// 0 alone finds their donors, in ascending ci.  A cluster's length is its
// sorted run's, which a donation does not change: the donor stays in its old
// list, and a cluster filled here (run length 0, one member) never donates.
__global__ __launch_bounds__(64) void pq_fit_empty_kernel(PqFitParams p) {
    const int sl = blockIdx.x;
    if (!p.active[sl]) return;
    const int lane = threadIdx.x;
    const uint32_t* st = p.start + (uint64_t)sl * p.ks;
    uint32_t* pts = p.points + (uint64_t)sl * p.n;
    const uint64_t s = (uint64_t)(p.s0 + sl);
    unsigned long long filled = 0;
    for (int base = 0; base < p.ks; base += 64) {
        const int c = base + lane;
        const bool empty = c < p.ks && st[c + 1] == st[c];
        unsigned long long mask = __ballot(empty);
        uint32_t mine = FIT_NIL;
        while (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            const uint32_t ci = (uint32_t)(base + b);
            uint32_t j = 0;
            if (lane == 0) {
                bool found = false;
                for (int a = 0; a < 64 && !found; ++a) {
                    j = (uint32_t)fit_draw(p.seed, s, (uint64_t)p.iter, ci, (uint64_t)a, p.n);
                    const uint32_t cl = pts[j];
                    found = st[cl + 1] - st[cl] > 1;
                }
                // n >= ks: some cluster holds two points that have not been given away
                for (uint64_t t = 0; t < p.n && !found; ++t) {
                    j = (uint64_t)j + 1 == p.n ? 0 : j + 1;
                    const uint32_t cl = pts[j];
                    found = st[cl + 1] - st[cl] > 1;
                }
                pts[j] = ci;
                ++filled;
            }
            j = __shfl(j, 0, 64);
            if (lane == b) mine = j;
        }
        if (c < p.ks) p.donor[(uint64_t)sl * p.ks + c] = mine;
    }
    if (lane == 0 && filled) {
        p.changes[sl] = (uint32_t)p.n;   // m.data.changes = dataSize
        atomicAdd(p.reseeded, filled);
    }
}

// one thread per (segment, cluster, dimension): the ds threads of a cluster
// read adjacent floats of every member row.  One wave per workgroup: there are
// only segments * ks * ds threads, and they should reach every CU.
__global__ __launch_bounds__(64) void pq_fit_centre_kernel(PqFitParams p) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_seg = (uint64_t)p.ks * p.ds;
    if (t >= per_seg * p.ng) return;
    const int sl = (int)(t / per_seg);
    if (!p.active[sl] || p.changes[sl] == 0) return;
    const uint64_t c = (t % per_seg) / p.ds;
    const int d = (int)(t % p.ds);
    const int s = p.s0 + sl;
    const float* xs = p.X + (uint64_t)s * p.ds + d;
    const uint64_t kc = (uint64_t)sl * p.ks + c;
    const uint32_t dn = p.donor[kc];
    float sum = 0.f;
    uint32_t len;
    if (dn != FIT_NIL) {
        len = 1;
        sum = __fadd_rn(sum, xs[fit_row(p, dn) * p.ldx]);
    } else {
        const uint32_t beg = p.start[kc], end = p.start[kc + 1];
        len = end - beg;
        // the loads of 16 members are in flight together; the adds keep list order
        uint32_t q = beg;
        for (; end - q >= 16; q += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = xs[fit_row(p, p.sval[q + u]) * p.ldx];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum = __fadd_rn(sum, v[u]);
        }
        for (; q < end; ++q) sum = __fadd_rn(sum, xs[fit_row(p, p.sval[q]) * p.ldx]);
    }
    p.cent[(uint64_t)s * per_seg + c * p.ds + d] = __fdiv_rn(sum, (float)len);
}

}  // namespace wv

extern "C" {

hipError_t wv_launch_pq_fit_init(const wv::PqFitParams* p, int segments, hipStream_t s) {
    const uint64_t total = (uint64_t)segments * p->ks * p->ds;
    hipLaunchKernelGGL(wv::pq_fit_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *p, segments);
    return hipGetLastError();
}

hipError_t wv_launch_pq_fit_iota(const wv::PqFitParams* p, hipStream_t s) {
    hipLaunchKernelGGL(wv::pq_fit_iota_kernel, dim3((unsigned)((p->n + 255) / 256), (unsigned)p->ng), dim3(256), 0, s,
                       *p);
    return hipGetLastError();
}

int wv_pq_fit_chunk_centres(int ks, int ds) {
    const int fit = wv::SBD_PQ_LUT_BYTES_MAX / (ds * 4);
    return fit < ks ? fit : ks;
}

hipError_t wv_launch_pq_fit_assign(const wv::PqFitParams* p, hipStream_t s) {
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)p->ng), block(256);
    const size_t lds = (size_t)p->cc * p->ds * 4;
    switch (p->ds) {
#define WV_FIT_CASE(DS)                                                                           \
    case DS:                                                                                      \
        hipLaunchKernelGGL(wv::pq_fit_assign_kernel<DS>, grid, block, lds, s, *p);                \
        break;
        WV_FIT_CASE(1)
        WV_FIT_CASE(2)
        WV_FIT_CASE(4)
        WV_FIT_CASE(8)
        WV_FIT_CASE(16)
        WV_FIT_CASE(32)
#undef WV_FIT_CASE
    default:
        hipLaunchKernelGGL(wv::pq_fit_assign_kernel<0>, grid, block, lds, s, *p);
    }
    return hipGetLastError();
}

// The group's (segment, cluster) -> j pairs sorted stably (equal keys keep
// ascending j) into skey / sval, then the clusters' bounds.  scratch ==
// nullptr: only *scratch_bytes is set.
hipError_t wv_pq_fit_sort(const wv::PqFitParams* p, void* scratch, size_t* scratch_bytes, hipStream_t s) {
    const uint64_t total = (uint64_t)p->ng * p->n;
    const uint32_t nkeys = (uint32_t)p->ng * (uint32_t)p->ks;
    int bits = 1;
    while (bits < 32 && (1ull << bits) < nkeys) ++bits;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(scratch, *scratch_bytes, p->key, p->skey, p->val, p->sval,
                                                      (int)total, 0, bits, s);
    if (e != hipSuccess || !scratch) return e;
    hipLaunchKernelGGL(wv::pq_fit_bounds_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p->skey, total,
                       nkeys, p->start);
    return hipGetLastError();
}

hipError_t wv_launch_pq_fit_empty(const wv::PqFitParams* p, hipStream_t s) {
    hipLaunchKernelGGL(wv::pq_fit_empty_kernel, dim3((unsigned)p->ng), dim3(64), 0, s, *p);
    return hipGetLastError();
}

hipError_t wv_launch_pq_fit_centres(const wv::PqFitParams* p, hipStream_t s) {
    const uint64_t total = (uint64_t)p->ng * p->ks * p->ds;
    hipLaunchKernelGGL(wv::pq_fit_centre_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, *p);
    return hipGetLastError();
}

}  // extern "C"
