// partial_fc.hip -- sampled-class (Partial FC) head: the kernels around the classifier products (include/fte.h "Partial FC",
// DESIGN.md 4.13).
//
// Sampler.  Class j gets the hash h_j = fmix32(j + base); the sample is every class of the batch plus the S - P other classes with
// the smallest hashes (P = distinct classes of the batch).  fmix32 is a bijection of uint32, so the h_j are distinct and the
// (S - P)-th smallest hash of the other classes is one threshold T: the sample is {positive} u {h_j <= T}.  T comes from a radix
// select, four passes of 8 bits from the top, each an integer histogram (LDS per block, then integer atomic adds: sums of integers,
// the same whatever the order).  Every kernel of a later pass re-derives the digits chosen so far from the finished histograms
// (256 bins each, one block scan), so nothing is read back to the host.  The compaction is in class order (per-block counts, one
// scan block, then the write), so `index` comes out sorted with no sort; the same pass writes the inverse map class -> position.
//
// Gather / scatter.  Both move whole columns of a [D, ld] row-major matrix.  The thread map is a thread per four adjacent columns of
// the COMPACT side for the gather and of the DENSE side for the scatter, 16 rows per block: the wide side of each kernel is one
// float4 per lane (fully coalesced), the other side reads sorted columns of one row, so every 128-byte line of that row is fetched
// once.  The scatter writes every element of dW exactly once (value or 0.0): no clear pass before it.
//
// Fused classifier update.  k_momentum_cols / k_adam_cols are the scatter's thread map with the optimizer in place of the store: the
// gradient of a lane's four columns is picked from the compact dWs (or is 0.0) and goes straight into W and its slots, so the dense
// dW is neither written nor read back.  The arithmetic is momentum_kernel's / adam_kernel's (kernels.hip) with the FMA contraction
// those kernels compile to written out (momentum_elem / adam_elem), so the bytes of W and the slots equal scatter + dense update.
#include <hip/hip_runtime.h>

#include "partial_fc.h"

namespace {

constexpr int TPB = 256;
constexpr int PER_THREAD = 8;                       // classes per thread in the compaction kernels
constexpr int CHUNK = TPB * PER_THREAD;             // classes per block
constexpr int ROWS = 16;                            // matrix rows per gather / scatter block
// workspace, in uint32 words: hist[4][256] | P | pad to 1088 | block counts [nblk rounded to 64] | flags (a byte per class)
constexpr int WS_P = 1024;
constexpr int WS_BLK = 1088;

__host__ __device__ inline int nblk_of(int C) { return (C + CHUNK - 1) / CHUNK; }
__host__ __device__ inline size_t flags_word(int C) { return WS_BLK + (size_t)(nblk_of(C) + 63) / 64 * 64; }

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// inclusive scan of one value per thread over the block (TPB threads); buf holds 2 * TPB words
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* buf) {
    const int tid = threadIdx.x;
    int cur = 0;
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < TPB; off <<= 1) {
        uint32_t x = buf[cur * TPB + tid];
        if (tid >= off) x += buf[cur * TPB + tid - off];
        cur ^= 1;
        buf[cur * TPB + tid] = x;
        __syncthreads();
    }
    const uint32_t r = buf[cur * TPB + tid];
    __syncthreads();
    return r;
}

// The digits the first `npass` finished passes select for rank K (1-based) among the other classes' hashes: prefix holds them in
// its top 8 * npass bits, krem is the rank left inside that prefix.  K == 0 (the batch's classes fill the sample): nothing to select.
__device__ __forceinline__ void derive(const uint32_t* hist, int npass, uint32_t K, uint32_t* buf, uint32_t* sel, uint32_t& prefix,
                                       uint32_t& krem) {
    prefix = 0;
    krem = K;
    if (K == 0) return;
    const int tid = threadIdx.x;
    for (int q = 0; q < npass; ++q) {
        const uint32_t v = hist[q * 256 + tid];
        const uint32_t inc = block_scan_incl(v, buf);
        const uint32_t exc = inc - v;
        if (tid == 0) { sel[0] = 255; sel[1] = 1; }             // (unreachable with K <= the number of other classes)
        __syncthreads();
        if (exc < krem && krem <= inc) { sel[0] = tid; sel[1] = krem - exc; }
        __syncthreads();
        prefix |= sel[0] << (24 - 8 * q);
        krem = sel[1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TPB) k_mark(const int32_t* __restrict__ labels, int n, int C, unsigned char* __restrict__ flags) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int y = labels[i];
    if ((unsigned)y < (unsigned)C) flags[y] = 1;               // several rows of one class store the same byte
}

__global__ void __launch_bounds__(TPB) k_hist(const unsigned char* __restrict__ flags, int C, uint32_t base, int S, int pass,
                                              uint32_t* __restrict__ ws) {
    __shared__ uint32_t lh[256];
    __shared__ uint32_t buf[2 * TPB];
    __shared__ uint32_t sel[2];
    __shared__ uint32_t npos;
    const int tid = threadIdx.x;
    uint32_t* hist = ws;
    lh[tid] = 0;
    if (tid == 0) npos = 0;
    uint32_t prefix = 0, krem = 1;
    if (pass > 0) {
        const uint32_t P = ws[WS_P];
        derive(hist, pass, (uint32_t)S - P, buf, sel, prefix, krem);
        if ((uint32_t)S == P) return;                           // uniform: no other class is sampled
    }
    __syncthreads();
    const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (32 - 8 * pass);
    const int shift = 24 - 8 * pass;
    uint32_t pos = 0;
    for (long j = (long)blockIdx.x * TPB + tid; j < C; j += (long)gridDim.x * TPB) {
        if (flags[j]) {
            ++pos;
            continue;
        }
        const uint32_t h = fmix32((uint32_t)j + base);
        if ((h & mask) == prefix) atomicAdd(&lh[(h >> shift) & 255], 1u);
    }
    if (pass == 0 && pos) atomicAdd(&npos, pos);
    __syncthreads();
    if (lh[tid]) atomicAdd(&hist[pass * 256 + tid], lh[tid]);
    if (pass == 0 && tid == 0 && npos) atomicAdd(&ws[WS_P], npos);
}

// which of the thread's PER_THREAD classes (from j0) are in the sample: bit i of the result
__device__ __forceinline__ uint32_t selected(const unsigned char* flags, int C, long j0, uint32_t base, bool any_neg, uint32_t T) {
    if (j0 >= C) return 0;
    const unsigned long long f8 = *(const unsigned long long*)(flags + j0);      // the flag array is padded past C and cleared
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const long j = j0 + i;
        const bool posv = (f8 >> (8 * i)) & 0xff;
        const bool in = j < C && (posv || (any_neg && fmix32((uint32_t)j + base) <= T));
        bits |= (uint32_t)in << i;
    }
    return bits;
}

__global__ void __launch_bounds__(TPB) k_count(const unsigned char* __restrict__ flags, int C, uint32_t base, int S,
                                               uint32_t* __restrict__ ws) {
    __shared__ uint32_t buf[2 * TPB];
    __shared__ uint32_t sel[2];
    uint32_t T, krem;
    const uint32_t K = (uint32_t)S - ws[WS_P];
    derive(ws, 4, K, buf, sel, T, krem);
    const long j0 = ((long)blockIdx.x * TPB + threadIdx.x) * PER_THREAD;
    const uint32_t cnt = __popc(selected(flags, C, j0, base, K != 0, T));
    const uint32_t inc = block_scan_incl(cnt, buf);
    if (threadIdx.x == TPB - 1) ws[WS_BLK + blockIdx.x] = inc;
}

// exclusive scan of the block counts, in place, by one block
__global__ void __launch_bounds__(TPB) k_scan(uint32_t* __restrict__ cnt, int nblk) {
    __shared__ uint32_t buf[2 * TPB];
    __shared__ uint32_t total;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += TPB) {
        const int b = b0 + threadIdx.x;
        const uint32_t v = b < nblk ? cnt[b] : 0;
        const uint32_t inc = block_scan_incl(v, buf);
        if (b < nblk) cnt[b] = carry + inc - v;
        if (threadIdx.x == TPB - 1) total = inc;
        __syncthreads();
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TPB) k_write(const unsigned char* __restrict__ flags, int C, uint32_t base, int S, int Spad,
                                               const uint32_t* __restrict__ ws, int32_t* __restrict__ index,
                                               int32_t* __restrict__ inverse) {
    __shared__ uint32_t buf[2 * TPB];
    __shared__ uint32_t sel[2];
    uint32_t T, krem;
    const uint32_t K = (uint32_t)S - ws[WS_P];
    derive(ws, 4, K, buf, sel, T, krem);
    const long j0 = ((long)blockIdx.x * TPB + threadIdx.x) * PER_THREAD;
    const uint32_t bits = selected(flags, C, j0, base, K != 0, T);
    const uint32_t cnt = __popc(bits);
    const uint32_t inc = block_scan_incl(cnt, buf);
    uint32_t pos = ws[WS_BLK + blockIdx.x] + inc - cnt;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const long j = j0 + i;
        if (j >= C) break;
        int32_t where = -1;
        if ((bits >> i) & 1) {
            if (pos < (uint32_t)S) {                            // always, by the select; never write past the sample
                index[pos] = (int32_t)j;
                where = (int32_t)pos;
            }
            ++pos;
        }
        inverse[j] = where;
    }
    if (blockIdx.x == 0)
        for (int k = S + threadIdx.x; k < Spad; k += TPB) index[k] = -1;
}

__global__ void __launch_bounds__(TPB) k_labels(const int32_t* __restrict__ labels, int n, int C, const int32_t* __restrict__ inverse,
                                                int32_t* __restrict__ out) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int y = labels[i];
    out[i] = (unsigned)y < (unsigned)C ? inverse[y] : -1;       // -1: the head's out-of-range label (a NaN row)
}

__global__ void __launch_bounds__(TPB) k_gather(const float* __restrict__ W, const int32_t* __restrict__ index, float* __restrict__ Ws,
                                                int D, int C, int cpad, int S, int Spad) {
    const int k4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (k4 >= Spad) return;
    const int4 id = *(const int4*)(index + k4);
    const int ids[4] = {id.x, id.y, id.z, id.w};
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ok[i] = k4 + i < S && (unsigned)ids[i] < (unsigned)C;
    const int d0 = blockIdx.y * ROWS;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int d = d0 + r;
        if (d >= D) break;
        const float* row = W + (size_t)d * cpad;
        float4 v;
        v.x = ok[0] ? row[ids[0]] : 0.f;
        v.y = ok[1] ? row[ids[1]] : 0.f;
        v.z = ok[2] ? row[ids[2]] : 0.f;
        v.w = ok[3] ? row[ids[3]] : 0.f;
        *(float4*)(Ws + (size_t)d * Spad + k4) = v;
    }
}

__global__ void __launch_bounds__(TPB) k_scatter(const float* __restrict__ dWs, const int32_t* __restrict__ inverse,
                                                 float* __restrict__ dW, int D, int C, int cpad, int S, int Spad) {
    const int j4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (j4 >= cpad) return;
    int ks[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ks[i] = j4 + i < C ? inverse[j4 + i] : -1;
        ok[i] = (unsigned)ks[i] < (unsigned)S;
    }
    const int d0 = blockIdx.y * ROWS;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int d = d0 + r;
        if (d >= D) break;
        const float* row = dWs + (size_t)d * Spad;
        float4 v;
        v.x = ok[0] ? row[ks[0]] : 0.f;
        v.y = ok[1] ? row[ks[1]] : 0.f;
        v.z = ok[2] ? row[ks[2]] : 0.f;
        v.w = ok[3] ? row[ks[3]] : 0.f;
        *(float4*)(dW + (size_t)d * cpad + j4) = v;
    }
}

// the four compact positions of the dense columns j4 .. j4 + 3 (k_scatter's rule): ok[i] <=> column j4 + i is in the sample
__device__ __forceinline__ void cols_of(const int32_t* __restrict__ inverse, int j4, int C, int S, int (&ks)[4], bool (&ok)[4]) {
    if (j4 + 3 < C) {
        const int4 iv = *(const int4*)(inverse + j4);           // inverse is 16-byte aligned and j4 a multiple of 4
        ks[0] = iv.x; ks[1] = iv.y; ks[2] = iv.z; ks[3] = iv.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) ks[i] = j4 + i < C ? inverse[j4 + i] : -1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ok[i] = (unsigned)ks[i] < (unsigned)S;
        if (!ok[i]) ks[i] = 0;                                  // a valid position: picked() loads without a branch, then drops it
    }
}

// dWs[d, k] of a sampled column, 0.0 otherwise (whatever the row holds at position 0, a NaN included, is dropped)
__device__ __forceinline__ float picked(const float* __restrict__ row, int k, bool ok) {
    const float g = row[k];
    return ok ? g : 0.f;
}

// One element of momentum_kernel (kernels.hip) as the compiler contracts `av = mom * av + (gs * gv + wd * wv); wv = wv - lr * av`
// there (read off its gfx950 code): the product gs * g is rounded, the other three multiplies are fused.  Spelt out, with
// contraction off, so that this kernel cannot drift from the dense one.
__device__ __forceinline__ void momentum_elem(float& w, float& a, float g, float lr, float mom, float wd, float gs) {
#pragma clang fp contract(off)
    float t = gs * g;
    t = __builtin_fmaf(wd, w, t);
    a = __builtin_fmaf(mom, a, t);
    w = __builtin_fmaf(-lr, a, w);
}

// One element of adam_kernel (kernels.hip), likewise: only gs * g + wd * w is fused there (onto the rounded wd * w); the moment
// updates and the step are separate multiplies and adds, the division and the square root the correctly rounded ones.
__device__ __forceinline__ void adam_elem(float& w, float& m, float& v, float g, float lr_t, float b1, float b2, float eps, float wd,
                                          float gs) {
#pragma clang fp contract(off)
    const float gv = __builtin_fmaf(gs, g, wd * w);
    const float mv = b1 * m + (1.f - b1) * gv;
    const float vv = b2 * v + (1.f - b2) * gv * gv;
    m = mv;
    v = vv;
    w = w - lr_t * mv / (sqrtf(vv) + eps);
}

// momentum_kernel with g[d, j] = dWs[d, inverse[j]] or 0.0: W, acc [D, cpad], one float4 of each per lane and row
__global__ void __launch_bounds__(TPB) k_momentum_cols(float* __restrict__ W, float* __restrict__ acc, const float* __restrict__ dWs,
                                                       const int32_t* __restrict__ inverse, int D, int C, int cpad, int S, int Spad,
                                                       float lr, float mom, float wd, float gs) {
    const int j4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (j4 >= cpad) return;
    int ks[4];
    bool ok[4];
    cols_of(inverse, j4, C, S, ks, ok);
    const int d0 = blockIdx.y * ROWS;
#pragma unroll 4
    for (int r = 0; r < ROWS; ++r) {
        const int d = d0 + r;
        if (d >= D) break;
        const float* row = dWs + (size_t)d * Spad;
        const size_t at = (size_t)d * cpad + j4;
        const float4 w4 = *(const float4*)(W + at), a4 = *(const float4*)(acc + at);
        float w[4] = {w4.x, w4.y, w4.z, w4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) momentum_elem(w[i], a[i], picked(row, ks[i], ok[i]), lr, mom, wd, gs);
        *(float4*)(acc + at) = make_float4(a[0], a[1], a[2], a[3]);
        *(float4*)(W + at) = make_float4(w[0], w[1], w[2], w[3]);
    }
}

// adam_kernel on the same thread map
__global__ void __launch_bounds__(TPB) k_adam_cols(float* __restrict__ W, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ dWs, const int32_t* __restrict__ inverse, int D, int C,
                                                   int cpad, int S, int Spad, float lr_t, float b1, float b2, float eps, float wd,
                                                   float gs) {
    const int j4 = (blockIdx.x * TPB + threadIdx.x) * 4;
    if (j4 >= cpad) return;
    int ks[4];
    bool ok[4];
    cols_of(inverse, j4, C, S, ks, ok);
    const int d0 = blockIdx.y * ROWS;
#pragma unroll 2
    for (int r = 0; r < ROWS; ++r) {
        const int d = d0 + r;
        if (d >= D) break;
        const float* row = dWs + (size_t)d * Spad;
        const size_t at = (size_t)d * cpad + j4;
        const float4 w4 = *(const float4*)(W + at), m4 = *(const float4*)(m + at), v4 = *(const float4*)(v + at);
        float w[4] = {w4.x, w4.y, w4.z, w4.w}, mo[4] = {m4.x, m4.y, m4.z, m4.w}, vo[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) adam_elem(w[i], mo[i], vo[i], picked(row, ks[i], ok[i]), lr_t, b1, b2, eps, wd, gs);
        *(float4*)(m + at) = make_float4(mo[0], mo[1], mo[2], mo[3]);
        *(float4*)(v + at) = make_float4(vo[0], vo[1], vo[2], vo[3]);
        *(float4*)(W + at) = make_float4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

size_t p_sample_ws_bytes(int C) { return flags_word(C) * 4 + ((size_t)C + 15) / 16 * 16 + 16; }

hipError_t p_sample(const int32_t* labels, int n, int C, int S, uint32_t seed, uint32_t step, int32_t* index, int32_t* inverse,
                    int32_t* labels_out, void* ws, hipStream_t st) {
    uint32_t hs = seed;                                         // fmix32 on the host: base = fmix32(fmix32(seed) + step)
    for (int i = 0; i < 2; ++i) {
        hs ^= hs >> 16;
        hs *= 0x85ebca6bu;
        hs ^= hs >> 13;
        hs *= 0xc2b2ae35u;
        hs ^= hs >> 16;
        if (i == 0) hs += step;
    }
    const uint32_t base = hs;
    uint32_t* w32 = (uint32_t*)ws;
    unsigned char* flags = (unsigned char*)(w32 + flags_word(C));
    const int Spad = (S + 63) / 64 * 64;
    const int nblk = nblk_of(C);
    hipError_t e = hipMemsetAsync(ws, 0, p_sample_ws_bytes(C), st);
    if (e != hipSuccess) return e;
    k_mark<<<(n + TPB - 1) / TPB, TPB, 0, st>>>(labels, n, C, flags);
    const int hblocks = nblk < 1024 ? nblk : 1024;
    for (int pass = 0; pass < 4; ++pass) k_hist<<<hblocks, TPB, 0, st>>>(flags, C, base, S, pass, w32);
    k_count<<<nblk, TPB, 0, st>>>(flags, C, base, S, w32);
    k_scan<<<1, TPB, 0, st>>>(w32 + WS_BLK, nblk);
    k_write<<<nblk, TPB, 0, st>>>(flags, C, base, S, Spad, w32, index, inverse);
    k_labels<<<(n + TPB - 1) / TPB, TPB, 0, st>>>(labels, n, C, inverse, labels_out);
    return hipGetLastError();
}

hipError_t p_gather_cols(const float* W, const int32_t* index, float* Ws, int D, int C, int cpad, int S, int Spad, hipStream_t st) {
    dim3 grid((Spad / 4 + TPB - 1) / TPB, (D + ROWS - 1) / ROWS);
    k_gather<<<grid, TPB, 0, st>>>(W, index, Ws, D, C, cpad, S, Spad);
    return hipGetLastError();
}

hipError_t p_scatter_cols(const float* dWs, const int32_t* inverse, float* dW, int D, int C, int cpad, int S, int Spad, hipStream_t st) {
    dim3 grid((cpad / 4 + TPB - 1) / TPB, (D + ROWS - 1) / ROWS);
    k_scatter<<<grid, TPB, 0, st>>>(dWs, inverse, dW, D, C, cpad, S, Spad);
    return hipGetLastError();
}

hipError_t p_momentum_update_cols(float* W, float* acc, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S, int Spad,
                                  float lr, float mom, float wd, float gs, hipStream_t st) {
    dim3 grid((cpad / 4 + TPB - 1) / TPB, (D + ROWS - 1) / ROWS);
    k_momentum_cols<<<grid, TPB, 0, st>>>(W, acc, dWs, inverse, D, C, cpad, S, Spad, lr, mom, wd, gs);
    return hipGetLastError();
}

hipError_t p_adam_update_cols(float* W, float* m, float* v, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S,
                              int Spad, float lr_t, float b1, float b2, float eps, float wd, float gs, hipStream_t st) {
    dim3 grid((cpad / 4 + TPB - 1) / TPB, (D + ROWS - 1) / ROWS);
    k_adam_cols<<<grid, TPB, 0, st>>>(W, m, v, dWs, inverse, D, C, cpad, S, Spad, lr_t, b1, b2, eps, wd, gs);
    return hipGetLastError();
}
