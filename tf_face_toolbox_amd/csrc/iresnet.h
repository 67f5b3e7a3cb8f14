// iresnet.h -- host launchers of the fused batch-norm + PReLU kernels (iresnet.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// floats of workspace the backward needs: [BN_MAX_SPLITS][3][C] partial sums (sum g, sum g * xhat, sum_{u <= 0} dy * u) and the
// three coefficient rows of dz = A g + B z + C0
size_t l_bn_prelu_ws_floats(int C);
// y = u > 0 ? u : alpha[c] * u with u = fma(z, scale[c], shift[c]);  C % 4 == 0
hipError_t l_bn_prelu_apply(const float* z, const float* scale, const float* shift, const float* alpha, float* y, long rows, int C,
                            hipStream_t st);
// split reduce (three sums per channel) -> ordered merge (dgamma, dbeta, dalpha, coef) -> dz = A g + B z + C0, g = dy * (u > 0 ? 1 : alpha)
hipError_t l_bn_prelu_bwd(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd, const float* scale,
                          const float* shift, const float* alpha, float* dz, float* dgamma, float* dbeta, float* dalpha, long rows, int C,
                          float* ws, hipStream_t st);
