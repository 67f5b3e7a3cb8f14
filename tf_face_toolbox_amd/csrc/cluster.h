// cluster.h -- clustering kernels (cluster.hip) behind include/fte.h "Clustering": link rules over the kNN lists of a leave-one-out
// fte_topk_search (cosine threshold with an optional mutual test; approximate rank-order distance) and connected components by a
// lock-free union-find.  Integer logic on int32 lists; no matrix cores, no workspace beyond the caller's parent array.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

hipError_t c_links_threshold(const float* scores, const int32_t* index, int n, int k, float min_score, int mutual, uint8_t* keep,
                             hipStream_t st);
hipError_t c_links_rank_order(const float* scores, const int32_t* index, int n, int k, float theta, float min_score, uint8_t* keep,
                              hipStream_t st);
hipError_t c_components(const int32_t* index, const uint8_t* keep, int n, int k, int32_t* parent, int32_t* label, hipStream_t st);
