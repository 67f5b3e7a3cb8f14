// partial_fc.h -- sampled-class (Partial FC) head kernels (partial_fc.hip): the per-step class sample, the column gather of the
// classifier weights, the one-pass column scatter of their gradient, and the optimizer updates that take the compact gradient
// straight into the classifier.  include/fte.h "Partial FC" states the contract.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

size_t p_sample_ws_bytes(int C);
hipError_t p_sample(const int32_t* labels, int n, int C, int S, uint32_t seed, uint32_t step, int32_t* index, int32_t* inverse,
                    int32_t* labels_out, void* ws, hipStream_t st);
hipError_t p_gather_cols(const float* W, const int32_t* index, float* Ws, int D, int C, int cpad, int S, int Spad, hipStream_t st);
hipError_t p_scatter_cols(const float* dWs, const int32_t* inverse, float* dW, int D, int C, int cpad, int S, int Spad, hipStream_t st);
hipError_t p_momentum_update_cols(float* W, float* acc, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S, int Spad,
                                  float lr, float mom, float wd, float gs, hipStream_t st);
hipError_t p_adam_update_cols(float* W, float* m, float* v, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S,
                              int Spad, float lr_t, float b1, float b2, float eps, float wd, float gs, hipStream_t st);
