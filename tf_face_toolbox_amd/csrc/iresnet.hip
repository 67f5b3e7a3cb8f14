// iresnet.hip -- batch norm fused with a per-channel PReLU for gfx950 (the IResNet block: BN -> conv -> BN -> PReLU -> conv -> BN,
// nets/iresnet.py).  Tensors are [rows, C] fp32 with C % 4 == 0; a lane moves 16 bytes along C.  With u = fma(z, scale[c], shift[c]),
// the expression bn_apply_kernel (layers.hip) evaluates:
//   forward   y = u > 0 ? u : alpha[c] * u
//   backward  g = dy * (u > 0 ? 1 : alpha[c]),  dalpha[c] = sum_{u <= 0} dy * u,  dgamma = sum g * xhat,  dbeta = sum g,
//             dz = gamma * rstd * (g - dbeta / rows - xhat * dgamma / rows) = A g + B z + C0
// The backward recomputes u from z with the forward's expression (the idea of fte_bn_train_bwd_zmask): the activated tensor is not read.
// Two passes over (dy, z): a split reduce carrying three sums per channel, a small ordered merge, the apply.  Every sum is fp32 and
// merged in a fixed order (lanes of a wave by an xor butterfly, the four waves of a block and the row splits in index order): no float
// atomics, two calls write identical bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "iresnet.h"
#include "igemm.h"
#include "layers.h"

#define SE_LIN_MAX_SPLITS 64

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ f32x4 ldq4(const float* p, long off) { return *reinterpret_cast<const f32x4*>(p + off); }
__device__ __forceinline__ void stq4(float* p, long off, const f32x4 v) { *reinterpret_cast<f32x4*>(p + off) = v; }

// scale * z + shift as ONE fused multiply-add per element: bn_affine of layers.hip, so that the forward's sign is the sign that
// fte_bn_apply would see and the backward's recomputed one
__device__ __forceinline__ f32x4 affine4(const f32x4 z, const f32x4 sc, const f32x4 sf) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(z[e], sc[e], sf[e]);
    return v;
}
// the PReLU of the igemm.hip epilogues: v > 0 ? v : alpha * v.  No contraction around the select: the product is rounded on its own,
// so alpha = 1 returns u's bits
__device__ __forceinline__ f32x4 prelu4(const f32x4 u, const f32x4 al) {
#pragma clang fp contract(off)
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = u[e] > 0.f ? u[e] : al[e] * u[e];
    return v;
}
// g = dy * (u > 0 ? 1 : alpha): evaluated by the reduce AND the apply pass, which must agree bit for bit
__device__ __forceinline__ f32x4 prelu_grad4(const f32x4 dy, const f32x4 u, const f32x4 al) {
#pragma clang fp contract(off)
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = u[e] > 0.f ? dy[e] : dy[e] * al[e];
    return g;
}

// A thread stays on ONE channel quad when the grid stride is a multiple of C / 4 (the launcher sizes the grid so: `inv`), and walks
// four 16-byte pieces at a time with all loads in flight -- the shape of bn_apply_kernel.
__global__ __launch_bounds__(256) void bn_prelu_apply_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ alpha,
                                                             float* __restrict__ y, long n4, int C) {
    const unsigned q = (unsigned)C >> 2;
    const long step = (long)gridDim.x * 256;
    const bool inv = step % q == 0;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    int c = (int)((unsigned)(i % q) << 2);
    f32x4 sc = ldq4(scale, c), sf = ldq4(shift, c), al = ldq4(alpha, c);
    if (inv) {
        for (; i + 3 * step < n4; i += 4 * step) {
            f32x4 zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) zv[u] = ldq4(z, (i + u * step) * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) stq4(y, (i + u * step) * 4, prelu4(affine4(zv[u], sc, sf), al));
        }
    }
    for (; i < n4; i += step) {
        if (!inv) {
            c = (int)((unsigned)(i % q) << 2);
            sc = ldq4(scale, c); sf = ldq4(shift, c); al = ldq4(alpha, c);
        }
        stq4(y, i * 4, prelu4(affine4(ldq4(z, i * 4), sc, sf), al));
    }
}

// sum over the lanes of a wave that hold the same channel quad (lanes Q apart), as an xor butterfly: every lane ends with the sum
template <int Q>
__device__ __forceinline__ f32x4 wave_rows_sum(f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = v[e];
#pragma unroll
        for (int m = Q; m < 64; m <<= 1) x += __shfl_xor(x, m);
        v[e] = x;
    }
    return v;
}

// Partial sums of one row split: part[(split * 3 + {0: sum g, 1: sum g * xhat, 2: sum_{u <= 0} dy * u}) * C + c].
// grid = (ceil(C / 4 / Q), splits), block = Q channel quads x 256 / Q row lanes, four rows in flight per lane (bn_bwd_reduce_v4_kernel).
template <int Q>
__global__ __launch_bounds__(256) void bn_prelu_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const float* __restrict__ alpha, float* __restrict__ part,
                                                                  long rows, int C, long rows_per_split) {
    constexpr int RL = 256 / Q;
    __shared__ f32x4 sh[3][4][Q];
    const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
    const int ch = (blockIdx.x * Q + q) * 4;
    const long r0 = (long)blockIdx.y * rows_per_split, r1 = min(rows, r0 + rows_per_split);
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = sg, sa = sg;
    const bool ok = ch < C;
    if (ok) {
        const f32x4 mu = ldq4(mean, ch), rs = ldq4(rstd, ch), sc = ldq4(scale, ch), sf = ldq4(shift, ch), al = ldq4(alpha, ch);
        auto one = [&](const f32x4 d, const f32x4 zz) {
            const f32x4 u = affine4(zz, sc, sf);
            const f32x4 g = prelu_grad4(d, u, al);
#pragma unroll
            for (int e = 0; e < 4; ++e) sa[e] += u[e] > 0.f ? 0.f : d[e] * u[e];
            sg += g;
            sgx += g * ((zz - mu) * rs);
        };
        long r = r0 + rl;
        for (; r + 3 * RL < r1; r += 4 * RL) {
            f32x4 d4[4], z4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                d4[u] = ldq4(dy, (r + u * RL) * C + ch);
                z4[u] = ldq4(z, (r + u * RL) * C + ch);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) one(d4[u], z4[u]);
        }
        for (; r < r1; r += RL) one(ldq4(dy, r * C + ch), ldq4(z, r * C + ch));
    }
    sg = wave_rows_sum<Q>(sg); sgx = wave_rows_sum<Q>(sgx); sa = wave_rows_sum<Q>(sa);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < Q) { sh[0][wave][q] = sg; sh[1][wave][q] = sgx; sh[2][wave][q] = sa; }
    __syncthreads();
    if (threadIdx.x < Q && ok) {
        f32x4 a = sh[0][0][q], b = sh[1][0][q], d = sh[2][0][q];
#pragma unroll
        for (int w = 1; w < 4; ++w) { a += sh[0][w][q]; b += sh[1][w][q]; d += sh[2][w][q]; }
        float* pp = part + (long)blockIdx.y * 3 * C;
        stq4(pp, ch, a); stq4(pp, C + ch, b); stq4(pp, 2 * C + ch, d);
    }
}

// merge the splits in index order -> dbeta, dgamma, dalpha and the coefficients of dz = A g + B z + C0 (bn_bwd_finalize_kernel's).
// Block = 16 channels x 16 split lanes: a wave holds 4 split lanes of its 16 channels (butterfly over lanes 16 and 32 apart), the four
// waves meet in LDS.
__global__ __launch_bounds__(256) void bn_prelu_bwd_finalize_kernel(const float* __restrict__ part, int splits, int C, float count,
                                                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta, float* __restrict__ dalpha,
                                                                    float* __restrict__ coef) {
    __shared__ float sh[3][4][16];
    const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int ch = blockIdx.x * 16 + cl;
    float sg = 0.f, sgx = 0.f, sa = 0.f;
    if (ch < C) {
#pragma unroll 4
        for (int s = lane; s < splits; s += 16) {
            const float* pp = part + (long)s * 3 * C;
            sg += pp[ch];
            sgx += pp[C + ch];
            sa += pp[2 * C + ch];
        }
    }
#pragma unroll
    for (int m = 16; m < 64; m <<= 1) { sg += __shfl_xor(sg, m); sgx += __shfl_xor(sgx, m); sa += __shfl_xor(sa, m); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < 16) { sh[0][wave][cl] = sg; sh[1][wave][cl] = sgx; sh[2][wave][cl] = sa; }
    __syncthreads();
    if (threadIdx.x >= 16 || ch >= C) return;
    sg = sh[0][0][cl]; sgx = sh[1][0][cl]; sa = sh[2][0][cl];
#pragma unroll
    for (int w = 1; w < 4; ++w) { sg += sh[0][w][cl]; sgx += sh[1][w][cl]; sa += sh[2][w][cl]; }
    dbeta[ch] = sg;
    dgamma[ch] = sgx;
    dalpha[ch] = sa;
    const float gr = gamma[ch] * rstd[ch];
    const float b = -gr * rstd[ch] * sgx / count;
    coef[ch] = gr;
    coef[C + ch] = b;
    coef[2 * C + ch] = -gr * sg / count - b * mean[ch];
}

// dz = A g + B z + C0 with g recomputed from (dy, z) as the reduce pass did
__global__ __launch_bounds__(256) void bn_prelu_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                                 const float* __restrict__ coef, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ alpha,
                                                                 float* __restrict__ dz, long n4, int C) {
    const unsigned q = (unsigned)C >> 2;
    const long step = (long)gridDim.x * 256;
    const bool inv = step % q == 0;                            // one channel quad per thread (see bn_prelu_apply_kernel)
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    f32x4 A, B, C0, sc, sf, al;
    auto coefs = [&](long ii) {
        const int c = (int)((unsigned)(ii % q) << 2);
        A = ldq4(coef, c); B = ldq4(coef, C + c); C0 = ldq4(coef, 2 * C + c);
        sc = ldq4(scale, c); sf = ldq4(shift, c); al = ldq4(alpha, c);
    };
    coefs(i);
    if (inv) {
        for (; i + 3 * step < n4; i += 4 * step) {
            f32x4 gv[4], zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gv[u] = ldq4(dy, (i + u * step) * 4);
                zv[u] = ldq4(z, (i + u * step) * 4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 g = prelu_grad4(gv[u], affine4(zv[u], sc, sf), al);
                stq4(dz, (i + u * step) * 4, A * g + B * zv[u] + C0);
            }
        }
    }
    for (; i < n4; i += step) {
        if (!inv) coefs(i);
        const f32x4 zz = ldq4(z, i * 4);
        const f32x4 g = prelu_grad4(ldq4(dy, i * 4), affine4(zz, sc, sf), al);
        stq4(dz, i * 4, A * g + B * zz + C0);
    }
}

// ---------------------------------------------------------------------------------------------------
// BN + SE + shortcut, no activation (the SE-IResNet block tail: z -> u = BN(z) -> u * gate(mean_hw u) + shortcut; fte.h).  The SE
// kernels of layers.hip give one block a whole image of 64 channels: at 128 x 56^2 x 64 that is 128 blocks.  Here the pixels of an
// image are split over S blocks when the unsplit grid cannot fill the device (se_lin_split); the partial sums of a split go to the
// workspace as part[split][sum][n][c] and a small launch adds them in split order.  S == 1 writes the results from the one kernel.
// Block = Q channel quads x 256 / Q pixel lanes (Q = 16; 8 below 32 channels, with idle lanes where c / 4 is no multiple of Q), four
// pixels in flight per lane, lanes of a wave by wave_rows_sum, the four waves in LDS in index order.
// ---------------------------------------------------------------------------------------------------
// NS sums per (image, channel) over the pixels [blockIdx.y * pps, ...) of image blockIdx.z: `load` walks a lane's pixels into acc[NS],
// `finish` takes the block's sums of one channel quad
template <int Q, int NS, class Load, class Finish>
__device__ __forceinline__ void se_lin_block_sums(int hw, int c, int pps, Load load, Finish finish) {
    constexpr int RL = 256 / Q;
    __shared__ f32x4 sh[NS][4][Q];
    const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
    const int ch = (blockIdx.x * Q + q) * 4;
    const int r0 = blockIdx.y * pps, r1 = min(hw, r0 + pps);
    f32x4 acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool ok = ch < c;
    if (ok) load(ch, (long)blockIdx.z * hw * c + ch, r0 + rl, r1, RL, acc);
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = wave_rows_sum<Q>(acc[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < Q) {
#pragma unroll
        for (int k = 0; k < NS; ++k) sh[k][wave][q] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < Q && ok) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            acc[k] = sh[k][0][q];
#pragma unroll
            for (int w = 1; w < 4; ++w) acc[k] += sh[k][w][q];
        }
        finish(ch, acc);
    }
}

// sq = scale * mean_hw(z) + shift, xm = (mean_hw(z) - mean) * rstd from the pixel sum of one image and channel quad
__device__ __forceinline__ void se_lin_squeeze_finish(const f32x4 s, int hw, long o, int ch, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, float* __restrict__ sq, float* __restrict__ xm) {
    const f32x4 zm = s / (float)hw;
    stq4(sq, o, affine4(zm, ldq4(scale, ch), ldq4(shift, ch)));
    if (xm) stq4(xm, o, (zm - ldq4(mean, ch)) * ldq4(rstd, ch));
}
// s1, s2 -> dgate = (gamma * s2 + beta * s1) * gate * (1 - gate)      (sum_hw dy * u with u = gamma * xhat + beta)
__device__ __forceinline__ void se_lin_sums_finish(const f32x4 t1, const f32x4 t2, long o, int ch, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ gate,
                                                   float* __restrict__ s1, float* __restrict__ s2, float* __restrict__ dgate) {
    stq4(s1, o, t1);
    stq4(s2, o, t2);
    const f32x4 gt = ldq4(gate, o);
    const f32x4 gy = ldq4(gamma, ch) * t2 + ldq4(beta, ch) * t1;
    stq4(dgate, o, gy * gt * (1.f - gt));
}

// grid = (channel blocks, S, n).  part == nullptr (S == 1): sq / xm written here; else part[split][n][c]
template <int Q>
__global__ __launch_bounds__(256) void se_lin_squeeze_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ sq,
                                                             float* __restrict__ xm, float* __restrict__ part, int hw, int c, int pps) {
    const long img_c = (long)blockIdx.z * c, slab = (long)gridDim.z * c;
    se_lin_block_sums<Q, 1>(hw, c, pps,
        [&](int, long px, int r, int r1, int RL, f32x4* acc) {
            f32x4 s0 = acc[0], s1 = acc[0];
            for (; r + 3 * RL < r1; r += 4 * RL) {
                f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = ldq4(z, px + (long)(r + u * RL) * c);
                s0 += v[0] + v[2]; s1 += v[1] + v[3];
            }
            for (; r < r1; r += RL) s0 += ldq4(z, px + (long)r * c);
            acc[0] = s0 + s1;
        },
        [&](int ch, const f32x4* acc) {
            if (part) stq4(part, blockIdx.y * slab + img_c + ch, acc[0]);
            else se_lin_squeeze_finish(acc[0], hw, img_c + ch, ch, scale, shift, mean, rstd, sq, xm);
        });
}
// one thread per (image, channel quad): the splits in index order, then the direct kernel's last step
__global__ __launch_bounds__(256) void se_lin_squeeze_merge_kernel(const float* __restrict__ part, int splits, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, float* __restrict__ sq,
                                                                   float* __restrict__ xm, int n, int hw, int c) {
    const int cq = c >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * cq) return;
    const long o = i * 4, slab = (long)n * c;
    f32x4 s = ldq4(part, o);
    for (int k = 1; k < splits; ++k) s += ldq4(part, k * slab + o);
    se_lin_squeeze_finish(s, hw, o, (int)(i % cq) * 4, scale, shift, mean, rstd, sq, xm);
}

// s1 = sum_hw dy, s2 = sum_hw dy * xhat.  part == nullptr (S == 1): s1 / s2 / dgate written here; else part[split][2][n][c]
template <int Q>
__global__ __launch_bounds__(256) void se_lin_bwd_sums_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gate, float* __restrict__ s1,
                                                              float* __restrict__ s2, float* __restrict__ dgate, float* __restrict__ part,
                                                              int hw, int c, int pps) {
    const long img_c = (long)blockIdx.z * c, slab = (long)gridDim.z * c;
    se_lin_block_sums<Q, 2>(hw, c, pps,
        [&](int ch, long px, int r, int r1, int RL, f32x4* acc) {
            const f32x4 mu = ldq4(mean, ch), rs = ldq4(rstd, ch);
            f32x4 a = acc[0], b = acc[1];
            for (; r + 3 * RL < r1; r += 4 * RL) {
                f32x4 d4[4], z4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    d4[u] = ldq4(dy, px + (long)(r + u * RL) * c);
                    z4[u] = ldq4(z, px + (long)(r + u * RL) * c);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { a += d4[u]; b += d4[u] * ((z4[u] - mu) * rs); }
            }
            for (; r < r1; r += RL) {
                const f32x4 d = ldq4(dy, px + (long)r * c);
                a += d; b += d * ((ldq4(z, px + (long)r * c) - mu) * rs);
            }
            acc[0] = a; acc[1] = b;
        },
        [&](int ch, const f32x4* acc) {
            if (part) {
                float* pp = part + (long)blockIdx.y * 2 * slab + img_c + ch;
                stq4(pp, 0, acc[0]); stq4(pp, slab, acc[1]);
            } else {
                se_lin_sums_finish(acc[0], acc[1], img_c + ch, ch, gamma, beta, gate, s1, s2, dgate);
            }
        });
}
__global__ __launch_bounds__(256) void se_lin_bwd_sums_merge_kernel(const float* __restrict__ part, int splits, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ gate,
                                                                    float* __restrict__ s1, float* __restrict__ s2, float* __restrict__ dgate,
                                                                    int n, int c) {
    const int cq = c >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * cq) return;
    const long o = i * 4, slab = (long)n * c;
    f32x4 t1 = ldq4(part, o), t2 = ldq4(part, slab + o);
    for (int k = 1; k < splits; ++k) { t1 += ldq4(part, 2 * k * slab + o); t2 += ldq4(part, (2 * k + 1) * slab + o); }
    se_lin_sums_finish(t1, t2, o, (int)(i % cq) * 4, gamma, beta, gate, s1, s2, dgate);
}

// out = u * gate[n, c] + shortcut, u = fma(z, scale, shift); product and sum rounded on their own, so gate = 1 gives the bytes of
// fte_bn_apply(res = shortcut, relu = 0).  grid = (blocks over one image's hw * c / 4 quads, image), the stride a multiple of c / 4
// (se_lin_apply_grid): a thread keeps its channel quad -- the walk of se_apply_kernel (layers.hip)
__global__ __launch_bounds__(256) void se_lin_apply_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ gate,
                                                           const float* __restrict__ res, float* __restrict__ out, int hwq, int cq) {
    const int step = (int)gridDim.x * 256;
    const long base = (long)blockIdx.y * hwq;
    int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= hwq) return;
    const int cqi = i % cq;
    const f32x4 g = ldq4(gate, ((long)blockIdx.y * cq + cqi) * 4);
    const f32x4 sc = ldq4(scale, cqi * 4), sf = ldq4(shift, cqi * 4);
    auto f = [&](const f32x4 zz, const f32x4 rr) {
#pragma clang fp contract(off)
        const f32x4 u = affine4(zz, sc, sf);
        const f32x4 p = u * g;
        return p + rr;
    };
    for (; i + 3 * step < hwq; i += 4 * step) {
        f32x4 zv[4], rv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { zv[u] = ldq4(z, (base + i + u * step) * 4); rv[u] = ldq4(res, (base + i + u * step) * 4); }
#pragma unroll
        for (int u = 0; u < 4; ++u) stq4(out, (base + i + u * step) * 4, f(zv[u], rv[u]));
    }
    for (; i < hwq; i += step) stq4(out, (base + i) * 4, f(ldq4(z, (base + i) * 4), ldq4(res, (base + i) * 4)));
}

// grid_for_c of layers.hip for fp32 tensors: the grid stride (blocks * 256 threads) is a multiple of C / 4, about two resident blocks
// per CU once every thread has four pieces to walk (FTE_BN_APPLY_BLOCKS: the same tuning hook)
inline int apply_grid(long n4, int C) {
    long q = C / 4, a = q, b = 256;
    while (b) { const long t = a % b; a = b; b = t; }
    const long m = q / a;
    long blocks = (n4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
    static const long cap_env = getenv("FTE_BN_APPLY_BLOCKS") ? atol(getenv("FTE_BN_APPLY_BLOCKS")) : 0;
    const long cap = cap_env > 0 ? cap_env : 512;
    if (blocks > cap && n4 >= 4 * cap * 256) blocks = cap;
    blocks = (blocks + m - 1) / m * m;
    return (int)blocks;
}

// channel quads per block of the reduce: quads_per_block of layers.hip, with the 8-quad form also taking C < 32
inline int reduce_quads(int C) { return C >= 256 ? 64 : (C >= 128 ? 32 : (C >= 64 ? 16 : 8)); }

// stat_split of layers.hip (the plan of the statistics and backward-reduce kernels there): about FTE_BN_SPLIT_BLOCKS = 2048 blocks per
// pass, at least 8 rows per row lane, at most BN_MAX_SPLITS splits
inline void prelu_split(long rows, int C, int* splits, long* rps) {
    const int Q = reduce_quads(C);
    const long cb = (C / 4 + Q - 1) / Q;
    const long lanes = 256 / Q;
    static const long target = getenv("FTE_BN_SPLIT_BLOCKS") ? atol(getenv("FTE_BN_SPLIT_BLOCKS")) : 2048;
    long rs = target / cb;
    if (rs > rows / (lanes * 8)) rs = rows / (lanes * 8);
    if (rs > BN_MAX_SPLITS) rs = BN_MAX_SPLITS;
    if (rs < 1) rs = 1;
    *rps = (rows + rs - 1) / rs;
    *splits = (int)((rows + *rps - 1) / *rps);
}


// chscale_grid of layers.hip: blocks.x a multiple of (c / 4) / gcd(c / 4, 256), four pieces per thread, about 1024 blocks in all
inline dim3 se_lin_apply_grid(int n, int hw, int c) {
    const long hwq = (long)hw * (c / 4), cq = c / 4;
    long a = cq, b = 256;
    while (b) { const long t = a % b; a = b; b = t; }
    const long m = cq / a;
    long gx = (hwq + 1023) / 1024;
    const long want = (1024 + n - 1) / n;
    if (gx > want) gx = want;
    if (gx < 1) gx = 1;
    gx = (gx + m - 1) / m * m;
    return dim3((unsigned)gx, (unsigned)n);
}

inline int se_lin_quads(int c) { return c < 32 ? 8 : 16; }

// Pixel splits of an image.  None when the unsplit grid (channel blocks x images) has a block for every CU (a quarter of the target
// FTE_SE_LIN_BLOCKS, default 4 blocks per CU; 0: never split -- the A/B hook) or the image has fewer than 64 pixels; else enough
// for the target, every pixel lane of a split with a pixel, at most SE_LIN_MAX_SPLITS.  -> S and the pixels per split; the last
// split may be short.
inline void se_lin_split(int n, int hw, int c, int* splits, int* pps) {
    const int Q = se_lin_quads(c);
    const long base = (long)((c / 4 + Q - 1) / Q) * n;
    static const long env = getenv("FTE_SE_LIN_BLOCKS") ? atol(getenv("FTE_SE_LIN_BLOCKS")) : -1;
    const long target = env >= 0 ? env : 4L * igemm_num_cus();
    long s = (4 * base >= target || hw < 64) ? 1 : (target + base - 1) / base;
    if (s > hw / (256 / Q)) s = hw / (256 / Q);
    if (s > SE_LIN_MAX_SPLITS) s = SE_LIN_MAX_SPLITS;
    if (s < 1) s = 1;
    *pps = (int)((hw + s - 1) / s);
    *splits = (hw + *pps - 1) / *pps;
}

}  // namespace

size_t l_bn_prelu_ws_floats(int C) { return (size_t)BN_MAX_SPLITS * 3 * C + 3 * (size_t)C; }

hipError_t l_bn_prelu_apply(const float* z, const float* scale, const float* shift, const float* alpha, float* y, long rows, int C,
                            hipStream_t st) {
    if (C < 4 || C % 4 || rows < 1) return hipErrorInvalidValue;
    const long n4 = rows * C / 4;
    hipLaunchKernelGGL(bn_prelu_apply_kernel, dim3(apply_grid(n4, C)), dim3(256), 0, st, z, scale, shift, alpha, y, n4, C);
    return hipGetLastError();
}

hipError_t l_bn_prelu_bwd(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd, const float* scale,
                          const float* shift, const float* alpha, float* dz, float* dgamma, float* dbeta, float* dalpha, long rows, int C,
                          float* ws, hipStream_t st) {
    if (C < 4 || C % 4 || rows < 1) return hipErrorInvalidValue;
    int splits; long rps;
    prelu_split(rows, C, &splits, &rps);
    float* part = ws;
    float* coef = ws + (size_t)BN_MAX_SPLITS * 3 * C;
#define FTE_PR(Q_) hipLaunchKernelGGL((bn_prelu_bwd_reduce_kernel<Q_>), dim3((C / 4 + Q_ - 1) / Q_, splits), dim3(256), 0, st, \
                                      dy, z, mean, rstd, scale, shift, alpha, part, rows, C, rps)
    switch (reduce_quads(C)) {
        case 64: FTE_PR(64); break;
        case 32: FTE_PR(32); break;
        case 16: FTE_PR(16); break;
        default: FTE_PR(8);
    }
#undef FTE_PR
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bn_prelu_bwd_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, part, splits, C, (float)rows, gamma, mean, rstd,
                       dgamma, dbeta, dalpha, coef);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long n4 = rows * C / 4;
    hipLaunchKernelGGL(bn_prelu_bwd_apply_kernel, dim3(apply_grid(n4, C)), dim3(256), 0, st, dy, z, coef, scale, shift, alpha, dz, n4, C);
    return hipGetLastError();
}

// ---- BN + SE + shortcut, no activation -------------------------------------------------------------
size_t l_se_lin_ws_floats(int n, int hw, int c) {
    int splits, pps;
    se_lin_split(n, hw, c, &splits, &pps);
    return (size_t)2 * splits * n * c;                     // (the squeeze uses half; S == 1 uses none of it)
}

static bool se_lin_shape_ok(int n, int hw, int c) {
    return n >= 1 && hw >= 1 && c >= 4 && c % 4 == 0 && n <= 65535 && (long)hw * c / 4 < (1L << 30);
}

hipError_t l_se_lin_squeeze(const float* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq,
                            float* xm, int n, int hw, int c, float* ws, hipStream_t st) {
    if (!se_lin_shape_ok(n, hw, c)) return hipErrorInvalidValue;
    int splits, pps;
    se_lin_split(n, hw, c, &splits, &pps);
    float* part = splits > 1 ? ws : nullptr;
    const int Q = se_lin_quads(c);
    const dim3 grid((c / 4 + Q - 1) / Q, splits, n);
    if (Q == 16) hipLaunchKernelGGL(se_lin_squeeze_kernel<16>, grid, dim3(256), 0, st, z, scale, shift, mean, rstd, sq, xm, part, hw, c, pps);
    else hipLaunchKernelGGL(se_lin_squeeze_kernel<8>, grid, dim3(256), 0, st, z, scale, shift, mean, rstd, sq, xm, part, hw, c, pps);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || splits == 1) return e;
    const long nq = (long)n * (c / 4);
    hipLaunchKernelGGL(se_lin_squeeze_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, part, splits, scale, shift, mean, rstd,
                       sq, xm, n, hw, c);
    return hipGetLastError();
}

hipError_t l_se_lin_apply(const float* z, const float* scale, const float* shift, const float* gate, const float* shortcut, float* out,
                          int n, int hw, int c, hipStream_t st) {
    if (!se_lin_shape_ok(n, hw, c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(se_lin_apply_kernel, se_lin_apply_grid(n, hw, c), dim3(256), 0, st, z, scale, shift, gate, shortcut, out, hw * (c / 4), c / 4);
    return hipGetLastError();
}

hipError_t l_se_lin_bwd_sums(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd,
                             const float* gate, float* s1, float* s2, float* dgate, int n, int hw, int c, float* ws, hipStream_t st) {
    if (!se_lin_shape_ok(n, hw, c)) return hipErrorInvalidValue;
    int splits, pps;
    se_lin_split(n, hw, c, &splits, &pps);
    float* part = splits > 1 ? ws : nullptr;
    const int Q = se_lin_quads(c);
    const dim3 grid((c / 4 + Q - 1) / Q, splits, n);
    if (Q == 16) hipLaunchKernelGGL(se_lin_bwd_sums_kernel<16>, grid, dim3(256), 0, st, dy, z, gamma, beta, mean, rstd, gate, s1, s2, dgate, part, hw, c, pps);
    else hipLaunchKernelGGL(se_lin_bwd_sums_kernel<8>, grid, dim3(256), 0, st, dy, z, gamma, beta, mean, rstd, gate, s1, s2, dgate, part, hw, c, pps);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || splits == 1) return e;
    const long nq = (long)n * (c / 4);
    hipLaunchKernelGGL(se_lin_bwd_sums_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, part, splits, gamma, beta, gate,
                       s1, s2, dgate, n, c);
    return hipGetLastError();
}
