// iresnet.h -- host launchers of the fused batch-norm + PReLU kernels and of the SE-IResNet block tail (iresnet.hip).
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

// BN + SE + shortcut, no activation (fte.h): tensors [n, hw, c] fp32, c % 4 == 0; sq / xm / gate / s1 / s2 / dgate [n, c].
// floats of workspace of the two split reductions: [S][2][n][c] partial sums, S from the device's CU count
size_t l_se_lin_ws_floats(int n, int hw, int c);
hipError_t l_se_lin_squeeze(const float* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq,
                            float* xm, int n, int hw, int c, float* ws, hipStream_t st);
hipError_t l_se_lin_apply(const float* z, const float* scale, const float* shift, const float* gate, const float* shortcut, float* out,
                          int n, int hw, int c, hipStream_t st);
hipError_t l_se_lin_bwd_sums(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd,
                             const float* gate, float* s1, float* s2, float* dgate, int n, int hw, int c, float* ws, hipStream_t st);
