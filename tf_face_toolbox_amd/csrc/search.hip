// search.hip -- evaluation kernels behind include/fte.h "Evaluation: similarity search and score statistics".
// Row normalisation, listed-pair scores, fused similarity + top-k (partial pass + merge) and fused similarity + score histograms.
// All arithmetic is fp32; the products run on v_mfma_f32_32x32x2_f32 (an exact k-ordered fp32 fma chain), whatever
// fte_set_mfma_dtype says.
//
// The products are oriented S^T = G . P^T: a 32-row block of the lane-side set ("probes", b) sits on the 32 lanes of a wave
// (lane l holds column l & 31 of the accumulator tile), and 32-row tiles of the register-side set (gallery, a) run through the 16
// accumulator registers (row (i & 3) + 8 (i >> 2) + 4 (l >> 5) of register i).  Each wave takes TG = 2 register-side tiles per step,
// so one probe operand feeds two MFMAs.  Operands come straight from global memory: over a 32-wide k block, lane (r, h) loads
// float4s at k = 32q + 16h + 4u (u = 0..3) of its row, and MFMA t = 4u + e of the block takes element e, i.e. sums k = 32q + t and
// 32q + 16 + t.  That k order is fixed by d alone, so a score never depends on the tile, slice or chunk that computed it.
#include <hip/hip_runtime.h>
#include <math.h>

#include "igemm.h"
#include "search.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TG = 2;                  // register-side tiles per wave step (64 rows)
constexpr int SLACK = 32;              // top-k: room above k kept per probe before a compaction

__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// acc[t][i] = dot(lane-side row, register-side row of tile t) over d (d % 32 == 0); bp / ap[t] already point at column 16h.
__device__ __forceinline__ void dot_tiles(const float* bp, const float* const (&ap)[TG], int d, f32x16 (&acc)[TG]) {
#pragma unroll
    for (int t = 0; t < TG; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float4 B[4], A[TG][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        B[u] = *(const float4*)(bp + 4 * u);
#pragma unroll
        for (int t = 0; t < TG; ++t) A[t][u] = *(const float4*)(ap[t] + 4 * u);
    }
    for (int q = 0; q < d; q += 32) {
        float4 Bc[4], Ac[TG][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            Bc[u] = B[u];
#pragma unroll
            for (int t = 0; t < TG; ++t) Ac[t][u] = A[t][u];
        }
        if (q + 32 < d) {                    // next k block in flight while this one multiplies
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                B[u] = *(const float4*)(bp + q + 32 + 4 * u);
#pragma unroll
                for (int t = 0; t < TG; ++t) A[t][u] = *(const float4*)(ap[t] + q + 32 + 4 * u);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float b4[4] = {Bc[u].x, Bc[u].y, Bc[u].z, Bc[u].w};
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                const float a4[4] = {Ac[t][u].x, Ac[t][u].y, Ac[t][u].z, Ac[t][u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[t], 0, 0, 0);
            }
        }
    }
}

// (score, index) order of every result: score descending, then index ascending; index < 0 marks an empty slot, last of all
__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    return s1 > s2 || (s1 == s2 && i1 < i2);
}

__device__ __forceinline__ void wave_lds_sync() {        // LDS written by other lanes of this wave becomes visible
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---------------------------------------------------------------- row normalisation, listed pairs (one wave per row / pair)
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* x, float* y, float* norms, int n, int d) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* xr = x + (long)row * d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) ss = fmaf(xr[c], xr[c], ss);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);     // every lane ends with the same sum
    const float nrm = sqrtf(ss), den = fmaxf(nrm, 1e-12f);
    if (norms && lane == 0) norms[row] = nrm;
    float* yr = y + (long)row * d;                                         // y may alias x: each lane rewrites what it read
    for (int c = lane; c < d; c += 64) yr[c] = xr[c] / den;
}

__global__ __launch_bounds__(256) void pair_scores_kernel(const float* x, const int32_t* ia, const int32_t* ib, float* out, int n, int d,
                                                          int np) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= np) return;
    const int a = ia[p], b = ib[p];
    if (a < 0 || a >= n || b < 0 || b >= n) {
        if (lane == 0) out[p] = __builtin_nanf("");
        return;
    }
    const float* xa = x + (long)a * d;
    const float* xb = x + (long)b * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s = fmaf(xa[c], xb[c], s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[p] = s;
}

// ---------------------------------------------------------------- top-k, partial pass
// One wave per (32-probe block, gallery slice).  Each probe keeps a candidate list in LDS (sc / ix, [slot][probe]: conflict-free
// for a common slot) shared by its two lanes, and one running threshold: the k-th best kept score once k are kept.  Gallery rows
// reach a lane in increasing index order, so a later row with a score equal to the threshold loses the tie and `s > thr` admits
// exactly the rows that can still enter.  When some probe's list passes k + SLACK, the wave compacts every list to its exact top k.
__device__ void compact(float* sc, int* ix, int r, int h, int& cnt, float& thr, int k) {
    wave_lds_sync();
    if (h == 0) {
        const int keep = min(cnt, k);
        for (int t = 0; t < keep; ++t) {          // selection: slots 0..keep-1 end sorted
            float bs = sc[t * 32 + r];
            int bi = ix[t * 32 + r], bj = t;
            for (int j = t + 1; j < cnt; ++j) {
                const float s = sc[j * 32 + r];
                const int i = ix[j * 32 + r];
                if (s > bs || (s == bs && i < bi)) { bs = s; bi = i; bj = j; }
            }
            if (bj != t) {
                sc[bj * 32 + r] = sc[t * 32 + r];
                ix[bj * 32 + r] = ix[t * 32 + r];
                sc[t * 32 + r] = bs;
                ix[t * 32 + r] = bi;
            }
        }
        cnt = keep;
        thr = keep == k ? sc[(k - 1) * 32 + r] : -INFINITY;
    }
    wave_lds_sync();
    cnt = __shfl(cnt, r);
    thr = __shfl(thr, r);
}

__global__ __launch_bounds__(64) void topk_partial_kernel(const float* __restrict__ P, const float* __restrict__ G, int m, int n, int d,
                                                          int k, int steps_per_slice, int gbase, int excl, int pbase,
                                                          float* __restrict__ ws_s, int* __restrict__ ws_i) {
    extern __shared__ float lds[];
    const int cap = k + SLACK + 32 * TG;
    float* sc = lds;
    int* ix = (int*)(lds + cap * 32);
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int probe = blockIdx.x * 32 + r, S = gridDim.y, slice = blockIdx.y;
    const bool pvalid = probe < m;
    const int nsteps = (n + 63) / 64;
    const int s0 = slice * steps_per_slice, s1 = min(nsteps, s0 + steps_per_slice);
    const long self = excl ? (long)pbase + probe - gbase : -1;             // the gallery row this probe skips (local index)
    const float* bp = P + (long)min(probe, m - 1) * d + 16 * h;
    float thr = -INFINITY;
    int cnt = 0;
    for (int st = s0; st < s1; ++st) {
        const int g = st * 64;
        const float* ap[TG];
#pragma unroll
        for (int t = 0; t < TG; ++t) ap[t] = G + (long)min(g + 32 * t + r, n - 1) * d + 16 * h;
        f32x16 acc[TG];
        dot_tiles(bp, ap, d, acc);
        unsigned cm = 0;
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = g + 32 * t + acc_row(i, h);
                const bool ok = pvalid && acc[t][i] > thr && row < n && row != self;
                cm |= (unsigned)ok << (16 * t + i);
            }
        if (__any(cm != 0)) {
            const unsigned pm = (unsigned)__shfl_xor((int)cm, 32);          // the probe's other lane: it fills the slots after ours
            int off = cnt + (h ? __popc(pm) : 0);
#pragma unroll
            for (int t = 0; t < TG; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((cm >> (16 * t + i)) & 1u) {
                        sc[off * 32 + r] = acc[t][i];
                        ix[off * 32 + r] = gbase + g + 32 * t + acc_row(i, h);
                        ++off;
                    }
            cnt += __popc(cm) + __popc(pm);
            if (__any(cnt > k + SLACK)) compact(sc, ix, r, h, cnt, thr, k);
        }
    }
    compact(sc, ix, r, h, cnt, thr, k);
    if (h == 0 && pvalid) {
        float* os = ws_s + ((long)probe * S + slice) * k;
        int* oi = ws_i + ((long)probe * S + slice) * k;
        for (int t = 0; t < k; ++t) {
            os[t] = t < cnt ? sc[t * 32 + r] : -INFINITY;
            oi[t] = t < cnt ? ix[t * 32 + r] : -1;
        }
    }
}

// ---------------------------------------------------------------- top-k merge: L sorted lists of k per row -> one (one wave per row)
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ in_s, const int32_t* __restrict__ in_i, int L, int k,
                                                        float* __restrict__ out_s, int32_t* __restrict__ out_i) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* ls = in_s + ((long)row * L + lane) * k;
    const int32_t* li = in_i + ((long)row * L + lane) * k;
    int p = 0;
    float s = -INFINITY;
    int ix = -1;
    if (lane < L) { s = ls[0]; ix = li[0]; }
    for (int t = 0; t < k; ++t) {
        float bs = s;
        int bi = ix, bl = lane;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {       // (key, lane) is a total order: every lane ends with the same winner
            const float os = __shfl_xor(bs, off);
            const int oi = __shfl_xor(bi, off), ol = __shfl_xor(bl, off);
            if (better(os, oi, bs, bi) || (!better(bs, bi, os, oi) && ol < bl)) { bs = os; bi = oi; bl = ol; }
        }
        if (lane == 0) {
            out_s[(long)row * k + t] = bs;
            out_i[(long)row * k + t] = bi;
        }
        if (lane == bl) {
            ++p;
            if (lane < L && p < k) { s = ls[p]; ix = li[p]; }
            else { s = -INFINITY; ix = -1; }
        }
    }
}

// ---------------------------------------------------------------- score histograms
// Four waves per block share two LDS uint32 histograms (genuine, impostor); waves stride over (32-row b tile, 64-row a step) pairs;
// in the triangle (same) a tile with no pair i < j is skipped before its product.  The block adds its non-zero bins to the uint64
// outputs with global atomics at the end; integer adds keep the counts independent of order.
__global__ __launch_bounds__(256) void score_hist_kernel(const float* __restrict__ A, const int32_t* __restrict__ la, int na,
                                                         const float* __restrict__ B, const int32_t* __restrict__ lb, int nb, int d,
                                                         int same, int nbins, long ntiles, int nbt, unsigned long long* hg,
                                                         unsigned long long* hi) {
    extern __shared__ unsigned hl[];
    for (int i = threadIdx.x; i < 2 * nbins; i += 256) hl[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const float half = 0.5f * nbins;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long)gridDim.x * 4) {
        const int b0 = (int)(tile % nbt) * 32, a0 = (int)(tile / nbt) * 64;
        if (same && a0 >= b0 + 31) continue;                // every pair of the tile has i >= j
        const int j = b0 + r, jc = min(j, nb - 1);
        const int lj = lb[jc];
        const float* bp = B + (long)jc * d + 16 * h;
        const float* ap[TG];
#pragma unroll
        for (int t = 0; t < TG; ++t) ap[t] = A + (long)min(a0 + 32 * t + r, na - 1) * d + 16 * h;
        f32x16 acc[TG];
        dot_tiles(bp, ap, d, acc);
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = a0 + 32 * t + acc_row(i, h);
                if (row < na && j < nb && (!same || row < j)) {
                    const int bin = min(max((int)((acc[t][i] + 1.0f) * half), 0), nbins - 1);
                    atomicAdd(&hl[(la[row] == lj ? 0 : nbins) + bin], 1u);
                }
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * nbins; i += 256) {
        const unsigned v = hl[i];
        if (v) atomicAdd(i < nbins ? &hg[i] : &hi[i - nbins], (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- template pooling (one wave per template)
// Lane l owns columns c = c0 + l + 64 j (j < PC) of a 64 * PC column chunk and walks the template's media and members in listed
// order, so every column's sum is a fixed sequential chain; the norm is the normalize_rows_kernel reduction (same lane/column map,
// same butterfly), so a pooled row is bit-identical to normalising the unnormalised pooled sum with fte_l2_normalize_rows.
constexpr int PC = 8;                  // columns per lane per chunk: d <= 512 stays in registers
constexpr int PU = 4;                  // member rows in flight per wave

__global__ __launch_bounds__(256) void template_pool_kernel(const float* __restrict__ x, const float* __restrict__ w, int n, int d,
                                                            const int32_t* __restrict__ members, int nmem,
                                                            const int32_t* __restrict__ media_off, int nmedia,
                                                            const int32_t* __restrict__ tmpl_off, int nt, float* __restrict__ out) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= nt) return;
    const int m0 = tmpl_off[t], m1 = tmpl_off[t + 1];
    bool bad = !(0 <= m0 && m0 <= m1 && m1 <= nmedia);          // every test below reads wave-uniform values
    float* o = out + (long)t * d;
    const bool regs = d <= 64 * PC;
    float acc[PC], ss = 0.f;
    for (int c0 = 0; c0 < d && !bad; c0 += 64 * PC) {
#pragma unroll
        for (int j = 0; j < PC; ++j) acc[j] = 0.f;
        for (int m = m0; m < m1 && !bad; ++m) {
            const int i0 = media_off[m], i1 = media_off[m + 1];
            if (!(0 <= i0 && i0 <= i1 && i1 <= nmem)) { bad = true; break; }
            float sm[PC], ws = 0.f;
#pragma unroll
            for (int j = 0; j < PC; ++j) sm[j] = 0.f;
            for (int i = i0; i < i1 && !bad; i += PU) {
                const int cnt = min(PU, i1 - i);
                int r[PU];
                float v[PU][PC], wu[PU];
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    r[u] = u < cnt ? members[i + u] : 0;
                    if (r[u] < 0 || r[u] >= n) bad = true;
                }
                if (bad) break;
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const float* xr = x + (long)r[u] * d;
                    wu[u] = u < cnt ? (w ? w[r[u]] : 1.f) : 0.f;
#pragma unroll
                    for (int j = 0; j < PC; ++j) {
                        const int c = c0 + lane + 64 * j;
                        v[u][j] = (u < cnt && c < d) ? xr[c] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < PU; ++u)
                    if (u < cnt) {
                        ws += wu[u];
#pragma unroll
                        for (int j = 0; j < PC; ++j) sm[j] = fmaf(wu[u], v[u][j], sm[j]);
                    }
            }
            if (!bad && ws != 0.f)
#pragma unroll
                for (int j = 0; j < PC; ++j) acc[j] += sm[j] / ws;
        }
#pragma unroll
        for (int j = 0; j < PC; ++j) {
            const int c = c0 + lane + 64 * j;
            if (c < d) {
                ss = fmaf(acc[j], acc[j], ss);
                if (!regs) o[c] = acc[j];                           // re-read and scaled below by the lane that wrote it
            }
        }
    }
    if (bad) {
        for (int c = lane; c < d; c += 64) o[c] = __builtin_nanf("");
        return;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    const float den = fmaxf(sqrtf(ss), 1e-12f);
    if (regs) {
#pragma unroll
        for (int j = 0; j < PC; ++j) {
            const int c = lane + 64 * j;
            if (c < d) o[c] = acc[j] / den;
        }
    } else {
        for (int c = lane; c < d; c += 64) o[c] = o[c] / den;
    }
}

// ---------------------------------------------------------------- set-to-set softmax score fusion (one wave per pair)
// The pair's |A| x |B| scores come in 16 x 16 tiles of v_mfma_f32_16x16x4_f32 (A rows on (lane & 15, register rows), B rows on
// lane & 15 of the columns), A tiles outer, B tiles inner, two B tiles per step while two remain (one A operand feeds both).
// Operands come straight from global memory: over a 32-wide k block, lane (r, g = lane >> 4) loads float4s at k = 32q + 8g + 4u
// (u = 0, 1) of its row, and MFMA t = 4u + e of the block takes element e, i.e. sums k = 32q + 8g' + 4u + e over g'.  That k order
// is fixed by d alone.  The epilogue keeps per-lane running sums num[b] += s e, den[b] += e with e = exp2(c_b (s - 1)),
// c_b = beta_b log2(e); the tile order, the lane butterfly and the beta order are fixed by (|A|, |B|, nbetas) alone.
constexpr int MAXB = 32;
struct BetaC { float c[MAXB]; };

template <int NT>
__device__ __forceinline__ void dot16(const float* ap, const float* const (&bp)[NT], int d, f32x4 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 A[2], B[NT][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        A[u] = *(const float4*)(ap + 4 * u);
#pragma unroll
        for (int t = 0; t < NT; ++t) B[t][u] = *(const float4*)(bp[t] + 4 * u);
    }
    for (int q = 0; q < d; q += 32) {
        float4 Ac[2], Bc[NT][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            Ac[u] = A[u];
#pragma unroll
            for (int t = 0; t < NT; ++t) Bc[t][u] = B[t][u];
        }
        if (q + 32 < d) {                    // next k block in flight while this one multiplies
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                A[u] = *(const float4*)(ap + q + 32 + 4 * u);
#pragma unroll
                for (int t = 0; t < NT; ++t) B[t][u] = *(const float4*)(bp[t] + q + 32 + 4 * u);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float a4[4] = {Ac[u].x, Ac[u].y, Ac[u].z, Ac[u].w};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float b4[4] = {Bc[t][u].x, Bc[t][u].y, Bc[t][u].z, Bc[t][u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], b4[e], acc[t], 0, 0, 0);
            }
        }
    }
}

// members of template t: [s, e) of `members`; false for a bad id, bad offsets or an empty template
__device__ __forceinline__ bool template_range(int t, int nt, const int32_t* media_off, int nmedia, const int32_t* tmpl_off, int nmem,
                                               int& s, int& e) {
    if (t < 0 || t >= nt) return false;
    const int m0 = tmpl_off[t], m1 = tmpl_off[t + 1];
    if (!(0 <= m0 && m0 < m1 && m1 <= nmedia)) return false;
    s = media_off[m0];
    e = media_off[m1];
    return 0 <= s && s < e && e <= nmem;
}

__device__ __forceinline__ void softmax_acc(float s, const BetaC& bc, int nb, float (&num)[MAXB], float (&den)[MAXB]) {
#pragma unroll
    for (int k = 0; k < MAXB; ++k)
        if (k < nb) {
            const float e = __builtin_amdgcn_exp2f(fmaf(bc.c[k], s, -bc.c[k]));     // in (2^-116, 1]: a normal float
            num[k] = fmaf(s, e, num[k]);
            den[k] += e;
        }
}

template <int NT>
__device__ __forceinline__ void pair_step(const float* x, const int32_t* members, int d, int a0, int na, int ti, int b0, int nbm, int tj,
                                          int r, int g, const BetaC& bc, int nb, float (&num)[MAXB], float (&den)[MAXB]) {
    const float* ap = x + (long)members[a0 + min(16 * ti + r, na - 1)] * d + 8 * g;
    const float* bp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bp[t] = x + (long)members[b0 + min(16 * (tj + t) + r, nbm - 1)] * d + 8 * g;
    f32x4 acc[NT];
    dot16<NT>(ap, bp, d, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (16 * ti + 4 * g + q < na && 16 * (tj + t) + r < nbm) softmax_acc(acc[t][q], bc, nb, num, den);
}

__global__ __launch_bounds__(256) void set_pair_scores_kernel(const float* __restrict__ x, int n, int d, const int32_t* __restrict__ members,
                                                              int nmem, const int32_t* __restrict__ media_off, int nmedia,
                                                              const int32_t* __restrict__ tmpl_off, int nt, const int32_t* __restrict__ ta,
                                                              const int32_t* __restrict__ tb, int np, BetaC bc, int nb,
                                                              float* __restrict__ out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= np) return;
    int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    bool ok = template_range(ta[p], nt, media_off, nmedia, tmpl_off, nmem, a0, a1) &&
              template_range(tb[p], nt, media_off, nmedia, tmpl_off, nmem, b0, b1);
    if (ok) {
        bool badrow = false;
        for (int i = a0 + lane; i < a1; i += 64) badrow |= members[i] < 0 || members[i] >= n;
        for (int i = b0 + lane; i < b1; i += 64) badrow |= members[i] < 0 || members[i] >= n;
        ok = !__any(badrow);
    }
    if (!ok) {
        if (lane == 0) out[p] = __builtin_nanf("");
        return;
    }
    const int na = a1 - a0, nbm = b1 - b0, TA = (na + 15) / 16, TB = (nbm + 15) / 16;
    const int r = lane & 15, g = lane >> 4;
    float num[MAXB], den[MAXB];
#pragma unroll
    for (int k = 0; k < MAXB; ++k) num[k] = den[k] = 0.f;
    for (int ti = 0; ti < TA; ++ti) {
        int tj = 0;
        for (; tj + 2 <= TB; tj += 2) pair_step<2>(x, members, d, a0, na, ti, b0, nbm, tj, r, g, bc, nb, num, den);
        if (tj < TB) pair_step<1>(x, members, d, a0, na, ti, b0, nbm, tj, r, g, bc, nb, num, den);
    }
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < MAXB; ++k)
        if (k < nb) {
            float nu = num[k], de = den[k];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                nu += __shfl_xor(nu, off);
                de += __shfl_xor(de, off);
            }
            tot += nu / de;
        }
    if (lane == 0) out[p] = tot / (float)nb;
}

// ---------------------------------------------------------------- MegaFace: genuine scores, fused rank count + impostor histogram
// Both kernels use dot_tiles' operand orientation and k order (probes on the lanes, the other rows through the registers, lane
// (r, h) at k = 32q + 16h + 4u, MFMA t = 4u + e), for NP lane-side blocks and NT register-side tiles at once: every accumulator
// is the same MFMA chain over the same operands, so a genuine score s(p, g) is bitwise the scan's s(p, d) for a copy d of g.
template <int NP, int NT>
__device__ __forceinline__ void dot_blocks(const float* const (&bp)[NP], const float* const (&ap)[NT], int d, f32x16 (&acc)[NP][NT]) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[p][t][i] = 0.f;
    float4 B[NP][4], A[NT][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int p = 0; p < NP; ++p) B[p][u] = *(const float4*)(bp[p] + 4 * u);
#pragma unroll
        for (int t = 0; t < NT; ++t) A[t][u] = *(const float4*)(ap[t] + 4 * u);
    }
    for (int q = 0; q < d; q += 32) {
        float4 Bc[NP][4], Ac[NT][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int p = 0; p < NP; ++p) Bc[p][u] = B[p][u];
#pragma unroll
            for (int t = 0; t < NT; ++t) Ac[t][u] = A[t][u];
        }
        if (q + 32 < d) {                    // next k block in flight while this one multiplies
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int p = 0; p < NP; ++p) B[p][u] = *(const float4*)(bp[p] + q + 32 + 4 * u);
#pragma unroll
                for (int t = 0; t < NT; ++t) A[t][u] = *(const float4*)(ap[t] + q + 32 + 4 * u);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float b4[4] = {Bc[p][u].x, Bc[p][u].y, Bc[p][u].z, Bc[p][u].w};
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float a4[4] = {Ac[t][u].x, Ac[t][u].y, Ac[t][u].z, Ac[t][u].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[p][t], 0, 0, 0);
                }
            }
        }
    }
}

// One wave per 32 listed pairs: pair j's probe row on lane column j, its target row on register row j, the score on the diagonal
// (row j sits in lane (j, (j >> 2) & 1), register (j & 3) + 4 (j >> 3)).  A row index outside its set gives NaN.
__global__ __launch_bounds__(256) void mf_pair_scores_kernel(const float* __restrict__ P, int m, const float* __restrict__ G, int n, int d,
                                                             const int32_t* __restrict__ ip, const int32_t* __restrict__ ig, int np,
                                                             float* __restrict__ out) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    if (w * 32 >= np) return;
    const int pair = min(w * 32 + r, np - 1);
    const int a = ip[pair], b = ig[pair];
    const bool ok = a >= 0 && a < m && b >= 0 && b < n;
    const float* bp[1] = {P + (long)(ok ? a : 0) * d + 16 * h};
    const float* ap[1] = {G + (long)(ok ? b : 0) * d + 16 * h};
    f32x16 acc[1][1];
    dot_blocks<1, 1>(bp, ap, d, acc);
    if (h != ((r >> 2) & 1) || w * 32 + r >= np) return;
    const int want = (r & 3) + 4 * (r >> 3);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i == want) s = acc[0][0][i];
    out[pair] = ok ? s : __builtin_nanf("");
}

// The scan.  Four waves per block share one LDS uint32 impostor histogram; waves stride over (MP-probe block, 64-row step) tiles,
// probe block fastest, so a 64-row step of the distractors is read from HBM once and met by every probe block while it is in L2.
// A wave holds MF_PB 32-probe blocks sharing each distractor operand.  Per probe a lane keeps its smallest genuine score (the CSR
// list is sorted descending): a score below it counts nowhere, which is nearly every score of a trained model.  A survivor
// binary-searches the probe's list for the first threshold it reaches and adds 1 there (ws, uint64); mf_prefix_kernel turns those
// into the counts.  Integer adds only: the results do not depend on the order.
constexpr int MF_PB = 2;               // 32-probe blocks per wave
constexpr int MF_MP = 32 * MF_PB;      // probes per tile

__global__ __launch_bounds__(256) void mf_scan_kernel(const float* __restrict__ P, int m, const float* __restrict__ G, int n, int d,
                                                      const int32_t* __restrict__ thr_off, const float* __restrict__ thr, int T,
                                                      int nbins, long ntiles, int npb, unsigned long long* __restrict__ first,
                                                      unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned hl[];
    for (int i = threadIdx.x; i < nbins; i += 256) hl[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const float half = 0.5f * nbins;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long)gridDim.x * 4) {
        const int p0 = (int)(tile % npb) * MF_MP, g0 = (int)(tile / npb) * 64;
        const float* bp[MF_PB];
        int o0[MF_PB], o1[MF_PB];
        float tmin[MF_PB];
        bool pv[MF_PB];
#pragma unroll
        for (int p = 0; p < MF_PB; ++p) {
            const int probe = p0 + 32 * p + r;
            pv[p] = probe < m;
            const int pc = min(probe, m - 1);
            bp[p] = P + (long)pc * d + 16 * h;
            o0[p] = thr_off[pc];
            o1[p] = thr_off[pc + 1];
            const bool ok = pv[p] && 0 <= o0[p] && o0[p] < o1[p] && o1[p] <= T;    // bad or empty list: counts nowhere
            if (!ok) o0[p] = o1[p] = 0;
            tmin[p] = ok ? thr[o1[p] - 1] : 0.f;
        }
        const float* ap[TG];
#pragma unroll
        for (int t = 0; t < TG; ++t) ap[t] = G + (long)min(g0 + 32 * t + r, n - 1) * d + 16 * h;
        f32x16 acc[MF_PB][TG];
        dot_blocks<MF_PB, TG>(bp, ap, d, acc);
#pragma unroll
        for (int p = 0; p < MF_PB; ++p)
#pragma unroll
            for (int t = 0; t < TG; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = g0 + 32 * t + acc_row(i, h);
                    if (!pv[p] || row >= n) continue;
                    const float s = acc[p][t][i];
                    atomicAdd(&hl[min(max((int)((s + 1.0f) * half), 0), nbins - 1)], 1u);
                    if (o1[p] > o0[p] && s >= tmin[p]) {
                        int lo = o0[p], hi = o1[p];              // first j in [o0, o1) with thr[j] <= s
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (thr[mid] <= s) hi = mid;
                            else lo = mid + 1;
                        }
                        if (lo < o1[p]) atomicAdd(&first[lo], 1ull);
                    }
                }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += 256) {
        const unsigned v = hl[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// counts[j] += sum of first[o0 .. j] over each probe's list (one thread per probe, in list order); a bad list is skipped
__global__ __launch_bounds__(256) void mf_prefix_kernel(const int32_t* __restrict__ thr_off, int m, int T,
                                                        const unsigned long long* __restrict__ first, unsigned long long* __restrict__ counts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const int o0 = thr_off[p], o1 = thr_off[p + 1];
    if (!(0 <= o0 && o0 < o1 && o1 <= T)) return;
    unsigned long long run = 0;
    for (int j = o0; j < o1; ++j) {
        run += first[j];
        counts[j] += run;
    }
}

}  // namespace

hipError_t s_normalize_rows(const float* x, float* y, float* norms, int n, int d, hipStream_t st) {
    normalize_rows_kernel<<<(n + 3) / 4, 256, 0, st>>>(x, y, norms, n, d);
    return hipGetLastError();
}

hipError_t s_pair_scores(const float* x, const int32_t* ia, const int32_t* ib, float* out, int n, int d, int npairs, hipStream_t st) {
    pair_scores_kernel<<<(npairs + 3) / 4, 256, 0, st>>>(x, ia, ib, out, n, d, npairs);
    return hipGetLastError();
}

int s_topk_slices(int m, int n, int k) {
    (void)k;
    const long ptiles = (m + 31) / 32, nsteps = (n + 63) / 64;
    const long want = 8L * igemm_num_cus();                 // one-wave blocks: about two rounds of four per CU
    long S = (want + ptiles - 1) / ptiles;
    if (S > 64) S = 64;                                     // the merge takes at most 64 lists
    if (S > nsteps) S = nsteps;
    return (int)(S < 1 ? 1 : S);
}

size_t s_topk_ws_bytes(int m, int n, int k) {
    return (size_t)m * s_topk_slices(m, n, k) * k * (sizeof(float) + sizeof(int32_t));
}

hipError_t s_topk_search(const float* probes, const float* gallery, int m, int n, int d, int k, int gallery_base, int exclude_self,
                         int probe_base, float* scores, int32_t* index, void* ws, hipStream_t st) {
    const int S = s_topk_slices(m, n, k), nsteps = (n + 63) / 64;
    float* ws_s = (float*)ws;
    int32_t* ws_i = (int32_t*)(ws_s + (size_t)m * S * k);
    const size_t lds = (size_t)(k + SLACK + 32 * TG) * 32 * (sizeof(float) + sizeof(int));
    topk_partial_kernel<<<dim3((m + 31) / 32, S), 64, lds, st>>>(probes, gallery, m, n, d, k, (nsteps + S - 1) / S, gallery_base,
                                                                 exclude_self, probe_base, ws_s, ws_i);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return s_topk_merge(ws_s, ws_i, m, S, k, scores, index, st);
}

hipError_t s_topk_merge(const float* in_scores, const int32_t* in_index, int m, int lists, int k, float* scores, int32_t* index,
                        hipStream_t st) {
    topk_merge_kernel<<<m, 64, 0, st>>>(in_scores, in_index, lists, k, scores, index);
    return hipGetLastError();
}

hipError_t s_score_histograms(const float* a, const int32_t* la, int na, const float* b, const int32_t* lb, int nb, int d, int same,
                              int nbins, unsigned long long* hg, unsigned long long* hi, hipStream_t st) {
    const int nbt = (nb + 31) / 32;
    const long ntiles = (long)nbt * ((na + 63) / 64);
    long blocks = 2L * igemm_num_cus();
    const long per_block_cap = 1L << 20;                    // tiles per block: its uint32 bins see at most 2^20 * 2048 = 2^31 pairs
    if (blocks < (ntiles + per_block_cap - 1) / per_block_cap) blocks = (ntiles + per_block_cap - 1) / per_block_cap;
    if (blocks > (ntiles + 3) / 4) blocks = (ntiles + 3) / 4;
    score_hist_kernel<<<(unsigned)blocks, 256, (size_t)2 * nbins * sizeof(unsigned), st>>>(a, la, na, b, lb, nb, d, same, nbins, ntiles,
                                                                                           nbt, hg, hi);
    return hipGetLastError();
}

hipError_t s_template_pool(const float* x, const float* w, int n, int d, const int32_t* members, int n_members, const int32_t* media_off,
                           int n_media, const int32_t* tmpl_off, int n_templates, float* out, hipStream_t st) {
    template_pool_kernel<<<(n_templates + 3) / 4, 256, 0, st>>>(x, w, n, d, members, n_members, media_off, n_media, tmpl_off, n_templates,
                                                                out);
    return hipGetLastError();
}

hipError_t s_set_pair_scores(const float* x, int n, int d, const int32_t* members, int n_members, const int32_t* media_off, int n_media,
                             const int32_t* tmpl_off, int n_templates, const int32_t* ta, const int32_t* tb, int npairs,
                             const float* betas, int nbetas, float* out, hipStream_t st) {
    BetaC bc = {};
    for (int k = 0; k < nbetas && k < MAXB; ++k) bc.c[k] = betas[k] * 1.44269504088896340736f;     // beta * log2(e), rounded once
    set_pair_scores_kernel<<<(npairs + 3) / 4, 256, 0, st>>>(x, n, d, members, n_members, media_off, n_media, tmpl_off, n_templates, ta, tb,
                                                             npairs, bc, nbetas, out);
    return hipGetLastError();
}

hipError_t s_mf_pair_scores(const float* probes, int m, const float* rows, int n, int d, const int32_t* ip, const int32_t* ig, int npairs,
                            float* out, hipStream_t st) {
    const int waves = (npairs + 31) / 32;
    mf_pair_scores_kernel<<<(waves + 3) / 4, 256, 0, st>>>(probes, m, rows, n, d, ip, ig, npairs, out);
    return hipGetLastError();
}

size_t s_mf_scan_ws_bytes(int nthr) { return (size_t)nthr * sizeof(unsigned long long); }

hipError_t s_mf_scan(const float* probes, int m, const float* rows, int n, int d, const int32_t* thr_off, const float* thr, int nthr,
                     int nbins, unsigned long long* counts, unsigned long long* hist, void* ws, hipStream_t st) {
    unsigned long long* first = (unsigned long long*)ws;
    hipError_t e = hipMemsetAsync(first, 0, s_mf_scan_ws_bytes(nthr), st);
    if (e != hipSuccess) return e;
    const int npb = (m + MF_MP - 1) / MF_MP;
    const long ntiles = (long)npb * ((n + 63) / 64);
    long blocks = 2L * igemm_num_cus();
    const long per_block_cap = (1L << 31) / (64L * MF_MP);  // tiles per block: its uint32 bins see at most 2^31 scores
    if (blocks < (ntiles + per_block_cap - 1) / per_block_cap) blocks = (ntiles + per_block_cap - 1) / per_block_cap;
    if (blocks > (ntiles + 3) / 4) blocks = (ntiles + 3) / 4;
    mf_scan_kernel<<<(unsigned)blocks, 256, (size_t)nbins * sizeof(unsigned), st>>>(probes, m, rows, n, d, thr_off, thr, nthr, nbins, ntiles,
                                                                                    npb, first, hist);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    mf_prefix_kernel<<<(m + 255) / 256, 256, 0, st>>>(thr_off, m, nthr, first, counts);
    return hipGetLastError();
}
