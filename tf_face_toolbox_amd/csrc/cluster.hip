// cluster.hip -- clustering kernels behind include/fte.h "Clustering" (DESIGN.md 4.17).
// Input: the kNN lists of a leave-one-out fte_topk_search of a set against itself, scores / index [n, k], k <= 64.  A slot (a, t)
// is VALID iff 0 <= index[a,t] < n and index[a,t] != a; everything else (the (-inf, -1) tails, garbage, self) is a hole that
// never links and is never a member of a list, so no index is followed before it has been range-checked.
//
// Link kernels: one wave per row a, lane l holding slot l of the row (k <= 64 = the wave).  For every slot that passes its own
// tests the wave fetches row b = index[a,t] in one coalesced load (the next row's load is issued before this one's arithmetic)
// and answers set questions about the two lists by broadcast-compare: a wave-uniform loop u < k reads slot u of one list into a
// scalar and every lane compares its slot of the other list with it; counts are popcounts of ballots.  Integer logic throughout:
// the only fp32 operations are the `>=` against the score floor and one product in the rank-order test.
//
// Components: a lock-free union-find over parent [n] in three launches (init, link, flatten).  Links hook the LARGER root under
// the SMALLER with a compare-and-swap, so parent[x] <= x always, every chain descends strictly (finds terminate, whatever they
// race with), and the root of a tree is its smallest member: the labels depend on the edge set alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "cluster.h"

namespace {

__device__ __forceinline__ int lane_value(int v, int l) { return __builtin_amdgcn_readlane(v, l); }     // l is wave-uniform
__device__ __forceinline__ int first_lane(unsigned long long m) { return __ffsll((long long)m) - 1; }

// ---------------------------------------------------------------- threshold links
__global__ __launch_bounds__(256) void links_threshold_kernel(const float* __restrict__ scores, const int32_t* __restrict__ index, int n,
                                                              int k, float min_score, uint8_t* __restrict__ keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const int a = i / k, b = index[i];
    keep[i] = (b >= 0 && b < n && b != a && scores[i] >= min_score) ? 1 : 0;
}

// keep[a,t] additionally needs a slot of row b = index[a,t] that lists a with a score at or above the floor
__global__ __launch_bounds__(256) void links_mutual_kernel(const float* __restrict__ scores, const int32_t* __restrict__ index, int n, int k,
                                                           float min_score, uint8_t* __restrict__ keep) {
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n) return;
    const bool in = lane < k;
    const long base = (long)a * k;
    const int ea = in ? index[base + lane] : -1;
    const float sa = in ? scores[base + lane] : 0.f;
    const bool valid = in && ea >= 0 && ea < n && ea != a;
    const int eav = valid ? ea : -1;
    unsigned long long todo = __ballot(valid && sa >= min_score);
    bool kept = false;
    int t = todo ? first_lane(todo) : -1;
    int eb = -1;
    float sb = 0.f;
    if (t >= 0) {
        const long rb = (long)lane_value(eav, t) * k;
        if (in) { eb = index[rb + lane]; sb = scores[rb + lane]; }
    }
    while (t >= 0) {
        const int tc = t, ebc = eb;
        const float sbc = sb;
        todo &= todo - 1;
        t = todo ? first_lane(todo) : -1;
        if (t >= 0) {                                        // the next row is in flight during this one's test
            const long rb = (long)lane_value(eav, t) * k;
            if (in) { eb = index[rb + lane]; sb = scores[rb + lane]; }
        }
        const bool back = __ballot(in && ebc == a && sbc >= min_score) != 0ull;
        if (lane == tc) kept = back;
    }
    if (in) keep[base + lane] = kept ? 1 : 0;
}

// ---------------------------------------------------------------- approximate rank-order links (Otto, Wang, Jain, TPAMI 2018)
// L_a = (a, index[a,0..k)) at positions 0..k; its members are a and its valid entries, a repeated entry counting at its first
// position only.  r(a,b) = 1 + the first t with index[a,t] == b (k + 1 if none); m(a,b) = the positions p <= min(r(a,b), k) of L_a
// whose entry is a member of L_a and not of L_b.  keep[a,t] = valid, score >= floor, and
//     (float)(m(a,b) + m(b,a)) < theta * (float)min(r(a,b), r(b,a))        (one fp32 product, one compare)
__global__ __launch_bounds__(256) void links_rank_order_kernel(const float* __restrict__ scores, const int32_t* __restrict__ index, int n,
                                                               int k, float theta, float min_score, uint8_t* __restrict__ keep) {
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n) return;
    const bool in = lane < k;
    const long base = (long)a * k;
    const int ea = in ? index[base + lane] : -1;
    const float sa = in ? scores[base + lane] : 0.f;
    const bool valid = in && ea >= 0 && ea < n && ea != a;
    const int eav = valid ? ea : -1;                         // -1 equals no row number
    bool dupa = false;
    for (int u = 0; u < k; ++u) {
        const int xa = lane_value(eav, u);
        dupa |= u < lane && xa == eav;
    }
    const bool livea = valid && !dupa;
    unsigned long long todo = __ballot(valid && sa >= min_score);
    bool kept = false;
    int t = todo ? first_lane(todo) : -1;
    int b = t >= 0 ? lane_value(eav, t) : 0;
    int eb = (t >= 0 && in) ? index[(long)b * k + lane] : -1;
    while (t >= 0) {
        const int tc = t, bc = b, ebc = eb;
        todo &= todo - 1;
        t = todo ? first_lane(todo) : -1;
        if (t >= 0) {                                        // the next row is in flight during this one's counts
            b = lane_value(eav, t);
            eb = in ? index[(long)b * k + lane] : -1;
        }
        const bool vb = in && ebc >= 0 && ebc < n && ebc != bc;
        const int ebv = vb ? ebc : -1;
        bool a_in_b = false, b_in_a = false, dupb = false;   // this lane's entry of L_a is in L_b / of L_b is in L_a / repeats
        for (int u = 0; u < k; ++u) {
            const int xa = lane_value(eav, u), xb = lane_value(ebv, u);
            a_in_b |= eav == xb;
            b_in_a |= ebv == xa;
            dupb |= u < lane && xb == ebv;
        }
        const int r_ab = first_lane(__ballot(eav == bc)) + 1;            // lane tc matches: never empty
        const unsigned long long hit = __ballot(ebv == a);
        const int r_ba = hit ? first_lane(hit) + 1 : k + 1;
        const int m_ab = (hit ? 0 : 1) + __popcll(__ballot(livea && lane < min(r_ab, k) && eav != bc && !a_in_b));
        const int m_ba = __popcll(__ballot(vb && !dupb && lane < min(r_ba, k) && ebv != a && !b_in_a));      // position 0 is b, a member of L_a
        const float bound = theta * (float)min(r_ab, r_ba);
        if (lane == tc) kept = (float)(m_ab + m_ba) < bound;
    }
    if (in) keep[base + lane] = kept ? 1 : 0;
}

// ---------------------------------------------------------------- connected components: lock-free union-find
// Every access to parent inside the link launch is an agent-scope atomic (the per-XCD L2s are not coherent for plain accesses).
// A value read late is still an ancestor of the node it was read for (a node's parent is only ever replaced by one of its
// ancestors), and a hook is a compare-and-swap on a node that must still be its own parent, so a late value costs a retry at most.
__device__ __forceinline__ int uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(int32_t* parent, int x) {        // path halving; every step moves to a smaller index
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        const int g = uf_load(parent + p);
        if (g == p) return p;
        uf_store(parent + x, g);             // x is not a root and never becomes one again: no hook can be overwritten here
        x = g;
    }
}

__global__ __launch_bounds__(256) void uf_init_kernel(int32_t* parent, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(256) void uf_link_kernel(const int32_t* __restrict__ index, const uint8_t* __restrict__ keep, int n, int k,
                                                      int32_t* parent) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k || !keep[i]) return;
    const int a = i / k, b = index[i];
    if (b < 0 || b >= n || b == a) return;
    int lo = uf_find(parent, a), hi = uf_find(parent, b);
    while (lo != hi) {
        if (lo > hi) { const int s = lo; lo = hi; hi = s; }
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) break;
        hi = uf_find(parent, old);           // lost: hi was hooked under old < hi meanwhile; max(lo, hi) has dropped, so this ends
    }
}

__global__ __launch_bounds__(256) void uf_flatten_kernel(const int32_t* __restrict__ parent, int n, int32_t* __restrict__ label) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x = i, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    label[i] = x;
}

}  // namespace

hipError_t c_links_threshold(const float* scores, const int32_t* index, int n, int k, float min_score, int mutual, uint8_t* keep,
                             hipStream_t st) {
    if (mutual) links_mutual_kernel<<<(n + 3) / 4, 256, 0, st>>>(scores, index, n, k, min_score, keep);
    else links_threshold_kernel<<<(n * k + 255) / 256, 256, 0, st>>>(scores, index, n, k, min_score, keep);
    return hipGetLastError();
}

hipError_t c_links_rank_order(const float* scores, const int32_t* index, int n, int k, float theta, float min_score, uint8_t* keep,
                              hipStream_t st) {
    links_rank_order_kernel<<<(n + 3) / 4, 256, 0, st>>>(scores, index, n, k, theta, min_score, keep);
    return hipGetLastError();
}

hipError_t c_components(const int32_t* index, const uint8_t* keep, int n, int k, int32_t* parent, int32_t* label, hipStream_t st) {
    uf_init_kernel<<<(n + 255) / 256, 256, 0, st>>>(parent, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uf_link_kernel<<<(n * k + 255) / 256, 256, 0, st>>>(index, keep, n, k, parent);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    uf_flatten_kernel<<<(n + 255) / 256, 256, 0, st>>>(parent, n, label);
    return hipGetLastError();
}
