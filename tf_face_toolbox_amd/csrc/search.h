// search.h -- evaluation kernels (search.hip): row normalisation, listed-pair scores, fused similarity + top-k, fused
// similarity + score histograms, template pooling, set-to-set softmax score fusion and the MegaFace rank / impostor scan.  fp32 throughout (v_mfma_f32_32x32x2_f32,
// v_mfma_f32_16x16x4_f32); fte_set_mfma_dtype does not apply.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

hipError_t s_normalize_rows(const float* x, float* y, float* norms, int n, int d, hipStream_t st);
hipError_t s_pair_scores(const float* x, const int32_t* ia, const int32_t* ib, float* out, int n, int d, int npairs, hipStream_t st);
int s_topk_slices(int m, int n, int k);                  // gallery slices of the partial pass (from the CU count)
size_t s_topk_ws_bytes(int m, int n, int k);
hipError_t s_topk_search(const float* probes, const float* gallery, int m, int n, int d, int k, int gallery_base, int exclude_self,
                         int probe_base, float* scores, int32_t* index, void* ws, hipStream_t st);
hipError_t s_topk_merge(const float* in_scores, const int32_t* in_index, int m, int lists, int k, float* scores, int32_t* index,
                        hipStream_t st);
hipError_t s_score_histograms(const float* a, const int32_t* la, int na, const float* b, const int32_t* lb, int nb, int d, int same,
                              int nbins, unsigned long long* hg, unsigned long long* hi, hipStream_t st);
hipError_t s_template_pool(const float* x, const float* w, int n, int d, const int32_t* members, int n_members, const int32_t* media_off,
                           int n_media, const int32_t* tmpl_off, int n_templates, float* out, hipStream_t st);
// betas: host array of nbetas (1..32) values
hipError_t s_set_pair_scores(const float* x, int n, int d, const int32_t* members, int n_members, const int32_t* media_off, int n_media,
                             const int32_t* tmpl_off, int n_templates, const int32_t* ta, const int32_t* tb, int npairs,
                             const float* betas, int nbetas, float* out, hipStream_t st);
hipError_t s_mf_pair_scores(const float* probes, int m, const float* rows, int n, int d, const int32_t* ip, const int32_t* ig, int npairs,
                            float* out, hipStream_t st);
size_t s_mf_scan_ws_bytes(int nthr);
hipError_t s_mf_scan(const float* probes, int m, const float* rows, int n, int d, const int32_t* thr_off, const float* thr, int nthr,
                     int nbins, unsigned long long* counts, unsigned long long* hist, void* ws, hipStream_t st);
