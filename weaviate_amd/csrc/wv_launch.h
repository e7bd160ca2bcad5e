// wv_launch.h -- the host launchers of the kernel files, declared once.
//
// Included by the file that defines a launcher and by every caller (the host
// files, tools/, tests/native): extern "C" names carry no types, so only a
// shared prototype makes the compiler refuse a definition that disagrees.
#pragma once
#include <hip/hip_runtime.h>

#include "wv_params.h"

extern "C" {
hipError_t wv_launch_bf_mfma(const wv::BfParams* p, hipStream_t s);
hipError_t wv_launch_bf_finalize(const wv::BfFinParams* p, hipStream_t s);
hipError_t wv_launch_bf_finalize_wide(const wv::BfFinParams* p, hipStream_t s);
hipError_t wv_launch_exact_scan(const wv::ScanParams* p, hipStream_t s);
hipError_t wv_launch_fbd(const int32_t* flags, int nq, const wv::FbParams* fb, hipStream_t s);
hipError_t wv_launch_fbd_mark(const int32_t* status, int nq, int32_t* flags, float* thr, const float* out_d,
                              const int32_t* out_n, int k, hipStream_t s);
hipError_t wv_launch_hnsw_stats(const uint32_t* counters, int nq, unsigned long long* acc, hipStream_t s);
hipError_t wv_launch_rownorm(const float* X, uint64_t N, int D, int ldx, float* norm2, unsigned int* maxbits,
                             hipStream_t s);
hipError_t wv_launch_normalize(const float* in, float* out, uint64_t n, int D, int ld, hipStream_t s);
hipError_t wv_launch_scale(const float* in, float* out, uint64_t n, float scale, hipStream_t s);
hipError_t wv_launch_qnorm(const float* Q, int nq, int D, int ldq, int metric, float* out, float* absmax_part,
                           hipStream_t s);
hipError_t wv_launch_hnsw(const wv::HnswParams* p, int waves_per_block, hipStream_t s);
hipError_t wv_launch_hnsw_wg(const wv::HnswParams* p, hipStream_t s);
hipError_t wv_launch_build_search(const wv::BuildParams* b, int waves_per_block, hipStream_t s);
hipError_t wv_launch_build_select(const wv::BuildParams* b, hipStream_t s);
hipError_t wv_launch_build_link(const wv::BuildParams* b, hipStream_t s);
hipError_t wv_launch_list_counts(const uint32_t* lists, uint64_t n_lists, int deg, uint32_t* counts, hipStream_t s);
hipError_t wv_launch_upper_relay(const uint32_t* old_upper, const uint32_t* old_counts, uint64_t n_rows, int old_levels,
                                 int new_levels, int deg, uint32_t* new_upper, uint32_t* new_counts, hipStream_t s);
int wv_hnsw_per_wave_words(int dpad, int efc, int sc, int vc_log2, int xs_log2);
int wv_hnsw_side_per_wave_words(int dpad, int side_rows, int vc_log2, int xs_log2);
int wv_hnsw_reg_per_wave_words(int dpad, int vc_log2);
hipError_t wv_launch_hnsw_side(const wv::HnswParams* p, int waves_per_block, int ev, hipStream_t s);
hipError_t wv_launch_sbd_scan(const wv::SbdParams* p, hipStream_t s);
hipError_t wv_sbd_sort(unsigned long long* keys, unsigned long long* tmp, const unsigned int* cnt, int nq, int cap,
                       int* offsets, void** scratch, size_t* scratch_cap, hipStream_t s);
hipError_t wv_launch_sbd_ids(const wv::SbdIdsParams* p, hipStream_t s);
hipError_t wv_sbd_ids_sort(unsigned long long* keys, unsigned long long* tmp, int n_keys, const unsigned int* cnt,
                           int q0, int nq, const int* seg_beg, const int* seg_cap, int* ends, void** scratch,
                           size_t* scratch_cap, hipStream_t s);
hipError_t wv_launch_sbd_pq_scan(const wv::SbdPqParams* p, hipStream_t s);
hipError_t wv_launch_sbd_pq_ids(const wv::SbdPqIdsParams* p, hipStream_t s);
hipError_t wv_launch_pq_encode(const float* X, int ldx, const uint64_t* ids, uint64_t n_rows, const wv::PqParams* pq,
                               uint8_t* codes, hipStream_t s);
hipError_t wv_launch_pq_scan(const wv::PqScanParams* p, hipStream_t s);
hipError_t wv_launch_pq_fit_init(const wv::PqFitParams* p, int segments, hipStream_t s);
hipError_t wv_launch_pq_fit_iota(const wv::PqFitParams* p, hipStream_t s);
int wv_pq_fit_chunk_centres(int ks, int ds);
hipError_t wv_launch_pq_fit_assign(const wv::PqFitParams* p, hipStream_t s);
hipError_t wv_pq_fit_sort(const wv::PqFitParams* p, void* scratch, size_t* scratch_bytes, hipStream_t s);
hipError_t wv_launch_pq_fit_empty(const wv::PqFitParams* p, hipStream_t s);
hipError_t wv_launch_pq_fit_centres(const wv::PqFitParams* p, hipStream_t s);
hipError_t wv_launch_split_rows(const float* in, int ld_in, const uint64_t* ids, uint64_t n, uint64_t n_valid, int D,
                                float scale, void* out, int ld_out, uint64_t out_row0, hipStream_t s);
hipError_t wv_launch_h16_rows(const float* in, int ld_in, const uint64_t* ids, uint64_t n, int D, int ns, float sign,
                              float scale, const unsigned int* scale_from_max, void* out, uint64_t out_row0,
                              unsigned int* res_max_bits, float* res_out, int wide_layout, hipStream_t s);
hipError_t wv_launch_h16_rows_gather(const float* in, int ld_in, const uint32_t* gather, uint64_t n, uint64_t n_pad,
                                     int D, int ns, float scale, void* out, hipStream_t s);
hipError_t wv_launch_h16_compact_aux(const float* xnorm, const uint32_t* rowidx, uint64_t n, const uint32_t* n_dev,
                                     float* cxnorm, uint64_t* excl, uint64_t excl_words, hipStream_t s);
hipError_t wv_launch_remap_ids(uint32_t* ids, int nq, int n_slots, int per_slot, int bq, uint64_t ntiles,
                               uint64_t units_per_block, const uint32_t* rowidx, uint64_t n_rows, const uint32_t* n_dev,
                               hipStream_t s);
hipError_t wv_launch_absmax(const float* in, int ld, uint64_t n, int D, unsigned int* max_bits, hipStream_t s);
hipError_t wv_launch_h16_qscale(const float* part, int nparts, unsigned int* max_bits, float bsign, float* qscale,
                                hipStream_t s);
hipError_t wv_launch_h16_xns(const float* xnorm, uint64_t n, float sx, const float* qscale, float* xns, hipStream_t s);
hipError_t wv_launch_bf_h16(const wv::H16Params* p, int ns, int seed, hipStream_t s);
hipError_t wv_launch_bf_h16w(const wv::H16Params* p, hipStream_t s);
hipError_t wv_launch_h16_seed(const wv::H16SeedParams* p, hipStream_t s);
hipError_t wv_launch_h16_margin(int metric, int D, const float* qnorm, const float* qres, float xnorm_max,
                                float ex_max, float sx, const float* qscale, int nq, float* marg, hipStream_t s);
hipError_t wv_launch_h16_gtau(const unsigned int* gtau, int nq, float sx, const float* qscale, float* tau,
                              hipStream_t s);
float wv_h16_pow2_scale(float maxabs);
hipError_t wv_launch_flat_ids(const wv::FlatIdsParams* p, hipStream_t s);
hipError_t wv_launch_flat_ids_pq(const wv::FlatIdsPqParams* p, hipStream_t s);
hipError_t wv_launch_ids_to_bits(const uint32_t* ids, const uint64_t* off, const int32_t* sel, int nsel,
                                 uint64_t max_len, uint64_t n_rows, uint64_t words, uint64_t* bits, hipStream_t s);
hipError_t wv_launch_pq_topk(const float* skey, const uint32_t* sval, const float* dist, const uint32_t* rows,
                             uint64_t nr, int q0, int nqc, int k, uint64_t id_base, uint64_t* out_ids, float* out_d,
                             int32_t* out_n, hipStream_t s);
}
