// api.hip -- extern "C" entry points of libfte.so (declared in include/fte.h).
// Host-side only: shape checks, operand-gather descriptors for the igemm kernel
// family, tile / split-K selection, ordered reductions.  Never allocates, never
// synchronises; every launch goes to the caller's stream.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../include/fte.h"
#include "conv_plan.h"
#include "igemm.h"
#include "wgrad16.h"
#include "pw16.h"
#include "kernels.h"
#include "loader.h"
#include "layers.h"
#include "wino.h"
#include "search.h"
#include "partial_fc.h"
#include "cluster.h"
#include "iresnet.h"

namespace {

inline int rc(hipError_t e) { return e == hipSuccess ? FTE_OK : (int)e; }

// The planner (conv_plan.h) is pure; its three inputs are made here.  The switches and the device figures are read ONCE, by the first call
// that plans -- function-local statics, not load-time constructors: Python may set os.environ between dlopen and that call.
const PlanKnobs& knobs() {
    static const PlanKnobs k = plan_knobs_from_env();
    return k;
}
// The device is asked (CU count, occupancy of a stream-K symbol) only for what a plan can consult: by a context that reaches the stream-K rule
// (fp32 operands, no BN fusion), for the one tile of its epilogue (sk_tile; with its 128x64 fallback).  Every symbol asked about costs
// the host time of ALL later launches of the process (measured on the BN nets, profiles/conv_plan_refactor.md), so none is asked in advance.
const Planner& planner(PlanCtx c, int epi) {
    if (c.bf16 || c.bn) {
        static const Planner host = {knobs(), {}};
        return host;
    }
    auto with_device = [](int e) {
        Planner p = {knobs(), {}};
        p.d.cus = igemm_num_cus();
        const int tile = sk_tile(p.k, e);
        for (int t : {tile, tile == TILE_128x128 ? (int)TILE_128x64 : tile})
            if (t >= 0 && t < 5) p.d.sk_bpc[t][e] = igemm_sk_blocks_per_cu(t, e);
        return p;
    };
    if (epi == EPI_FWD) {
        static const Planner fwd = with_device(EPI_FWD);
        return fwd;
    }
    static const Planner dgrad = with_device(EPI_DGRAD);
    return dgrad;
}
// context of an fp32-tensor entry point (operands follow fte_set_mfma_dtype) / of a bf16-source (fte_*16) one
inline PlanCtx ctx32(bool bn = false) { return {igemm_get_bf16(), false, bn, wino_get_algo()}; }
inline PlanCtx ctx16(bool s16, bool bn = false) { return {true, s16, bn, wino_get_algo()}; }
// the tile plan depends on the operand mode (fte_set_mfma_dtype, the *16 and the bf16-STORAGE *_s16 entry points): workspace queries
// answer for ALL of them, so that a buffer sized once stays valid when the mode is switched
template <class F>
size_t max_over_modes(bool bn, F total) {
    size_t need = 0;
    const int algo = wino_get_algo();
    for (const PlanCtx& c : {PlanCtx{false, false, bn, algo}, PlanCtx{true, false, bn, algo}, PlanCtx{true, true, bn, algo}}) {
        const size_t v = total(c);
        if (v > need) need = v;
    }
    return need;
}

inline void zero_params(IgemmParams* p) { memset(p, 0, sizeof(*p)); }

inline void plain_a(IgemmParams* p, const float* a, int ld, int kc) {
    p->A = a; p->a_OH = 1; p->a_OW = 1; p->a_IH = 1; p->a_IW = 1; p->a_stride = 1;
    p->a_ld = ld; p->a_KC = kc; p->a_NT = 1;
}
// taps of a SAME conv on the A operand: source pixel = grid * stride + (r - pad, s - pad)
inline void conv_taps(IgemmParams* p, int ksize, const Pads& ph, const Pads& pw) {
    p->a_NT = ksize * ksize;
    for (int r = 0; r < ksize; ++r)
        for (int s = 0; s < ksize; ++s) { p->a_dh[r * ksize + s] = r - ph.before; p->a_dw[r * ksize + s] = s - pw.before; }
}

// operand sizes for the buffer-load range check; tensors must stay below 2 GiB (offsets are 32-bit,
// 0x80000000 is the out-of-range marker)
inline bool set_bytes(IgemmParams* p, size_t a_elems, size_t b_elems, size_t esize = 4) {
    const size_t lim = (size_t)1 << 31;
    if (a_elems * esize >= lim || b_elems * esize >= lim) return false;
    p->a_bytes = (unsigned)(a_elems * esize);
    p->b_bytes = (unsigned)(b_elems * esize);
    return true;
}

// main (+ tail) launches of one row-tiled op; PA/PB partial rows are numbered main first, then tail
inline hipError_t launch_rows(IgemmParams p, const RowPlan& rp, int al, int bl, int epi, long prow0, float* pw, hipStream_t st) {
    const int M = p.M;
    hipError_t e = hipSuccess;
    if (rp.tail_mode == 3) {                      // stream-K: slabs first, the flag words behind them
        int bm, bn;
        igemm_tile_dims(rp.main_tile, &bm, &bn);
        const long T = rp.main_mtiles * (p.N / bn), iters = T * (p.K / 32);
        p.m_base = 0; p.prow0 = (int)prow0;
        p.sk_workers = rp.sk_workers; p.sk_base = (int)(iters / rp.sk_workers); p.sk_rem = (int)(iters % rp.sk_workers);
        p.SKW = pw; p.SKF = reinterpret_cast<unsigned*>(pw + (size_t)rp.sk_workers * bm * bn);
        return igemm_launch(p, al, bl, epi, rp.main_tile, 1, st);
    }
    if (rp.main_rows > 0) {
        p.m_base = 0; p.M = (int)rp.main_rows; p.prow0 = (int)prow0;
        e = igemm_launch(p, al, bl, epi, rp.main_tile, 1, st);
        if (e != hipSuccess) return e;
    }
    if (rp.tail_mode == 0) return e;
    p.m_base = (int)rp.main_rows; p.M = M; p.prow0 = (int)(prow0 + rp.main_mtiles);
    if (rp.tail_mode == 1) return igemm_launch(p, al, bl, epi, rp.tail_tile, 1, st);
    p.PW = pw; p.kchunk = rp.tail_kchunk;
    e = igemm_launch(p, al, bl, epi, rp.tail_tile, rp.tail_splits, st);
    if (e != hipSuccess) return e;
    return igemm_fixup(p, epi, rp.tail_tile, rp.tail_splits, st);
}

// a dense product (params complete but for Y) by its plan: split-K into workspace slabs, then the ordered reduction into `out` with bias
// and activation in its epilogue -- or one launch straight into `out`
inline int launch_dense(IgemmParams p, const DensePlan& d, int al, int bl, int tile, float* out, const float* bias, int bmod, int act,
                        void* ws, size_t ws_bytes, hipStream_t st) {
    p.kchunk = d.kchunk;
    p.slab = (long)p.M * p.N;
    if (d.splits > 1) {
        if (!ws || ws_bytes < d.slab_bytes) return FTE_EWORKSPACE;
        p.Y = (float*)ws;
        hipError_t e = igemm_launch(p, al, bl, EPI_FWD, tile, d.splits, st);
        if (e != hipSuccess) return (int)e;
        return rc(k_reduce_rows((const float*)ws, out, bias, bmod, d.splits, p.slab, 1, 1.f, nullptr, st, act));
    }
    p.Y = out; p.bias = bias;
    return rc(igemm_launch(p, al, bl, EPI_FWD, tile, 1, st));
}

// every tensor the Winograd kernels touch moves 16 bytes per lane, like the direct path's (igemm_launch): 16-byte aligned or an error code
inline bool aligned16(std::initializer_list<const void*> ptrs) {
    uintptr_t v = 0;
    for (const void* q : ptrs) v |= (uintptr_t)q;
    return (v & 15) == 0;
}
// the first conv's kernels exist for SAME padding at stride 1 and 2 (same_pads divides by the stride)
inline bool first_conv_shape_ok(int n, int h, int wd, int stride) { return n >= 1 && h >= 1 && wd >= 1 && (stride == 1 || stride == 2); }
}  // namespace

extern "C" {

#ifndef FTE_SRC_SHA
#define FTE_SRC_SHA "unstamped"
#endif
// "... src:<hash of csrc/*.hip, *.h at build time>" (csrc/build.sh): bench.py and __graft_entry__.build() compare it with the sources'
const char* fte_version(void) { return "fte 0.2 gfx950 fp32-mfma src:" FTE_SRC_SHA; }

int fte_to_bf16(const float* x, uint16_t* y, long n, void* stream) {
    if (!x || !y || n <= 0 || n % 4) return FTE_EINVAL;
    return rc(k_to_bf16(x, y, n, (hipStream_t)stream));
}
int fte_pack_weights_bf16(const float* w, uint16_t* w16, uint16_t* w16t, int ksize, int cin, int cout, void* stream) {
    if (!w || (!w16 && !w16t) || ksize <= 0 || cin <= 0 || cout <= 0) return FTE_EINVAL;
    return rc(k_pack_weights_bf16(w, w16, w16t, ksize * ksize, cin, cout, (hipStream_t)stream));
}

int fte_pack_weights_bf16_table(const float* params, uint16_t* dst, const int32_t* table, int nconv, long total, int transposed, void* stream) {
    if (!params || !dst || !table || nconv <= 0 || nconv > 64 || total <= 0 || total % 4) return FTE_EINVAL;
    return rc(k_pack_weights_table(params, dst, table, nconv, total, transposed, (hipStream_t)stream));
}

int fte_set_mfma_dtype(int dtype) {
    if (dtype != FTE_MFMA_F32 && dtype != FTE_MFMA_BF16) return FTE_EINVAL;
    igemm_set_bf16(dtype == FTE_MFMA_BF16);
    return FTE_OK;
}
int fte_get_mfma_dtype(void) { return igemm_get_bf16() ? FTE_MFMA_BF16 : FTE_MFMA_F32; }

int fte_set_conv_algo(int algo) {
    if (algo < FTE_CONV_DIRECT || algo > FTE_CONV_AUTO) return FTE_EINVAL;
    wino_set_algo(algo);
    return FTE_OK;
}
int fte_get_conv_algo(void) { return wino_get_algo(); }

int fte_prof_enable(int on) { igemm_prof_enable(on != 0, on == 1); return FTE_OK; }
int fte_prof_count(void) { return igemm_prof_count(); }
int fte_prof_get_shape(int i, int* mnk, double* bytes) {
    if (!mnk || !bytes) return FTE_EINVAL;
    return rc(igemm_prof_get_shape(i, mnk, bytes));
}
int fte_prof_get_name(int i, char* buf, int buflen) {
    if (!buf || buflen <= 0) return FTE_EINVAL;
    return rc(igemm_prof_get_name(i, buf, buflen));
}
int fte_prof_get(int i, int* sig, double* flops, float* ms) {
    if (!sig || !flops || !ms) return FTE_EINVAL;
    return rc(igemm_prof_get(i, sig, flops, ms));
}

// ------------------------------------------------------------------------------------------------
size_t fte_conv2d_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride) {
    if (n <= 0 || cin <= 0 || cin % 32 || cout <= 0 || cout % 64) return 0;
    const ConvShape s = {n, h, wd, cin, cout, ksize, stride};
    return max_over_modes(false, [&](PlanCtx c) { return fwd_layout(planner(c, EPI_FWD), c, s).total; });
}

// Arguments of the forward launch, named as they were as parameters: context, shape, workspace and stream lead, everything else starts zero
// and is set by name.  x / w are bf16 copies (x16 [n,h,wd,cin]; w16t [k*k][cout][cin], fte_pack_weights_bf16) when `src16`
struct FwdArgs {
    PlanCtx ctx; ConvShape s; void* ws; size_t ws_bytes; void* stream;
    const void* x; const void* w; bool src16; const float* bias; const float* alpha; const float* res; float* z; float* y; uint16_t* y16;
    const uint16_t* res16; uint16_t* z16; float* stat_part; int* stat_rows; float* vpack; const float* xalpha; bool z_only_ok;
    int run() const;
};
int FwdArgs::run() const {
    const int n = s.n, h = s.h, wd = s.wd, cin = s.cin, cout = s.cout, ksize = s.ksize, stride = s.stride;
    // xalpha / z_only_ok (fte_conv3x3_fwd_keep_act): x is the producing layer's z, activated in the tile transform; y may be absent.  Both
    // exist on the Winograd path with a kept V only -- every other path below needs x as it is and writes y
    const bool z_only = z_only_ok && !y && z && vpack;
    if ((xalpha || z_only_ok) && !vpack) return FTE_EINVAL;
    if (!x || !w || (!y && !(src16 && y16) && !z_only) || n <= 0 || cin % 32 || cout % 64 || (stride != 1 && stride != 2) || (ksize != 1 && ksize != 3))
        return FTE_EINVAL;
    const Pads ph = same_pads(h, ksize, stride), pw = same_pads(wd, ksize, stride);
    IgemmParams p;
    zero_params(&p);
    p.M = n * ph.out * pw.out; p.N = cout; p.K = ksize * ksize * cin; p.kchunk = p.K;
    p.a_OH = ph.out; p.a_OW = pw.out; p.a_IH = h; p.a_IW = wd; p.a_stride = stride;
    p.a_ld = cin; p.a_KC = cin;
    conv_taps(&p, ksize, ph, pw);
    p.A = (const float*)x;
    p.B = (const float*)w;
    p.c_ld = cout;
    p.Y = y; p.Z = z; p.R = res; p.bias = bias; p.alpha = alpha; p.Y16 = y16;
    p.R16 = res16; p.Z16 = z16;
    int bl = BL_KN;
    if (src16) {                                     // transposed pack: rows = output channels, k-contiguous per tap
        p.src16 = 1; p.b_ld = cin; bl = BL_NK;
        for (int t = 0; t < ksize * ksize; ++t) p.b_tapoff[t] = t * cout * cin;
    } else {
        p.b_ld = cout;
    }
    if (!set_bytes(&p, (size_t)n * h * wd * cin, (size_t)ksize * ksize * cin * cout, src16 ? 2 : 4)) return FTE_EINVAL;
    const FwdLayout lay = fwd_layout(planner(ctx, EPI_FWD), ctx, s);
    if (lay.wino && !stat_part && (y || z_only)) {
        const WinoWs& wl = vpack ? lay.w_kept : lay.w;      // the caller keeps V (fte_conv3x3_fwd_keep): ws holds the filters only
        if (ws && ws_bytes >= wl.total) {          // Winograd F(2x2,3x3): filter transform, tile transform, 16 products + output transform + epilogue
            if (!aligned16({x, w, bias, alpha, res, z, y, ws, vpack, xalpha})) return FTE_EINVAL;
            float* V = vpack ? vpack : (float*)((char*)ws + wl.v_off);
            float* U = (float*)((char*)ws + wl.u_off);
            hipError_t e = wino_transform_filter((const float*)w, U, cin, cout, 0, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            e = wino_transform_tiles((const float*)x, V, n, h, wd, cin, 0, (hipStream_t)stream, wino_fwd_small_tiles(knobs()), xalpha);
            if (e != hipSuccess) return (int)e;
            WinoMMParams q;
            memset(&q, 0, sizeof(q));
            q.V = V; q.U = U; q.K = cin; q.N = cout; q.g = wino_geom(n, h, wd);
            q.Y = y; q.Z = z; q.R = res; q.bias = bias; q.alpha = alpha;
            return rc(wino_mm(q, EPI_FWD, (hipStream_t)stream));
        }
    }
    if (vpack) return FTE_EWORKSPACE;              // a kept V was asked for and the Winograd path did not run: never silently
    RowPlan rp = lay.rp;
    if (rp.tail_mode >= 2 && (!ws || ws_bytes < rp.pw_bytes)) rp = plan_rows(planner(ctx, EPI_FWD), ctx, p.M, p.N, p.K, false);   // no room: small-tile tail
    if (stat_part) {                                 // "BN fusion": one statistics partial row per tile row of the launch(es)
        if (rp.tail_mode == 2) return FTE_EINVAL;    // (plan_rows never splits in a bn context)
        p.SP = stat_part;
        *stat_rows = (int)(rp.main_mtiles + rp.tail_mtiles);
    }
    return rc(launch_rows(p, rp, AL_MK, bl, EPI_FWD, 0, (float*)ws, (hipStream_t)stream));
}
int fte_conv2d_fwd(const float* x, const float* w, const float* bias, const float* alpha, const float* res,
                   float* z, float* y, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                   void* ws, size_t ws_bytes, void* stream) {
    FwdArgs a = {ctx32(), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.x = x; a.w = w;
    a.bias = bias; a.alpha = alpha; a.res = res; a.z = z; a.y = y;
    return a.run();
}
int fte_conv2d_fwd16(const uint16_t* x16, const uint16_t* w16t, const float* bias, const float* alpha, const float* res,
                     float* z, float* y, uint16_t* y16, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                     void* ws, size_t ws_bytes, void* stream) {
    FwdArgs a = {ctx16(false), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.x = x16; a.w = w16t; a.src16 = true;
    a.bias = bias; a.alpha = alpha; a.res = res; a.z = z; a.y = y; a.y16 = y16;
    return a.run();
}

int fte_conv2d_fwd_s16(const uint16_t* x16, const uint16_t* w16t, const float* bias, const float* alpha, const uint16_t* res16,
                       uint16_t* z16, uint16_t* y16, float* z32, float* y32, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!y16 || (res16 && ((uintptr_t)res16 & 15))) return FTE_EINVAL;
    FwdArgs a = {ctx16(!z32 && !y32), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.x = x16; a.w = w16t; a.src16 = true;
    a.bias = bias; a.alpha = alpha; a.z = z32; a.y = y32; a.y16 = y16; a.res16 = res16; a.z16 = z16;
    return a.run();
}

size_t fte_conv3x3_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int stride) {
    return fte_conv2d_fwd_ws_bytes(n, h, wd, cin, cout, 3, stride);
}
int fte_conv3x3_fwd(const float* x, const float* w, const float* bias, const float* alpha, const float* res,
                    float* z, float* y, int n, int h, int wd, int cin, int cout, int stride,
                    void* ws, size_t ws_bytes, void* stream) {
    return fte_conv2d_fwd(x, w, bias, alpha, res, z, y, n, h, wd, cin, cout, 3, stride, ws, ws_bytes, stream);
}
int fte_conv3x3_fwd_keep(const float* x, const float* w, const float* bias, const float* alpha, const float* res,
                         float* z, float* y, int n, int h, int wd, int cin, int cout, int stride, float* vpack,
                         void* ws, size_t ws_bytes, void* stream) {
    if (vpack && ((uintptr_t)vpack & 15)) return FTE_EINVAL;
    FwdArgs a = {ctx32(), {n, h, wd, cin, cout, 3, stride}, ws, ws_bytes, stream};
    a.x = x; a.w = w; a.bias = bias; a.alpha = alpha; a.res = res; a.z = z; a.y = y; a.vpack = vpack;
    return a.run();
}
int fte_conv3x3_fwd_keep_act(const float* x, const float* xalpha, const float* w, const float* bias, const float* alpha, const float* res,
                             float* z, float* y, int n, int h, int wd, int cin, int cout, int stride, float* vpack,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!vpack || ((uintptr_t)vpack & 15) || (!y && !z)) return FTE_EINVAL;
    FwdArgs a = {ctx32(), {n, h, wd, cin, cout, 3, stride}, ws, ws_bytes, stream};
    a.x = x; a.w = w; a.bias = bias; a.alpha = alpha; a.res = res; a.z = z; a.y = y;
    a.vpack = vpack; a.xalpha = xalpha; a.z_only_ok = true;
    return a.run();
}
int fte_conv3x3_algo(int n, int h, int wd, int cin, int cout, int stride, int op) {
    if (op < 0 || op > 2) return FTE_EINVAL;
    return wino_wanted(knobs(), ctx32(), {n, h, wd, cin, cout, 3, stride}, op) ? FTE_CONV_WINOGRAD : FTE_CONV_DIRECT;
}
size_t fte_wino_pack_bytes(int n, int h, int wd, int c) {
    if (n <= 0 || h < 2 || wd < 2 || c <= 0 || c % 64) return 0;
    return wino_pack_floats(wino_geom(n, h, wd).M, c) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
static size_t dgrad_ws_bytes(const ConvShape& s, bool bn) {
    if (s.n <= 0 || s.cin <= 0 || s.cin % 64 || s.cout % 32) return 0;      // shapes fte_conv2d_dgrad rejects need no workspace
    return max_over_modes(bn, [&](PlanCtx c) { return dgrad_layout(planner(c, EPI_DGRAD), c, s).total; });
}
size_t fte_conv2d_dgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride) {
    return dgrad_ws_bytes({n, h, wd, cin, cout, ksize, stride}, false);
}

// the BN layer a "BN fusion" data gradient lands on (fte_conv2d_dgrad_bn): see igemm.h
struct DgradBn {
    const void* zbn; const void* ybn;                 // the BN's input z; its (add + ReLU'd) output when the mask comes from there
    const float* gamma; const float* mean; const float* rstd; const float* scale; const float* shift;
    float* dgamma; float* dbeta; float* coef;
};
// arguments of the data-gradient launch, as FwdArgs.  dz / w are bf16 copies (dz16 [n,ho,wo,cout]; w16 [k*k][cin][cout], the HWIO layout) when `src16`
struct DgradArgs {
    PlanCtx ctx; ConvShape s; void* ws; size_t ws_bytes; void* stream;
    const void* dz; const void* w; bool src16; const float* addin; const float* zprev; const float* alpha_prev;
    float* raw; float* dzprev; uint16_t* dzprev16; float* dalpha_prev; float* dbias_prev;
    const uint16_t* addin16; const uint16_t* zprev16; uint16_t* raw16; const DgradBn* bn;
    int run();      // (on the caller's own copy: a BN layer's tensors are moved into the PReLU slots)
};
int DgradArgs::run() {
    const int n = s.n, h = s.h, wd = s.wd, cin = s.cin, cout = s.cout, ksize = s.ksize, stride = s.stride;
    const float* zx = nullptr;
    const uint16_t* zx16 = nullptr;
    if (bn) {          // mask tensor -> the Zin slot, the BN input -> Zx when the mask comes from the output
        const void* msk = (!bn->scale && bn->ybn) ? bn->ybn : bn->zbn;
        const void* zb = (!bn->scale && bn->ybn) ? bn->zbn : nullptr;
        if (src16) { zprev16 = (const uint16_t*)msk; zx16 = (const uint16_t*)zb; }
        else { zprev = (const float*)msk; zx = (const float*)zb; }
        alpha_prev = bn->gamma;                       // (never read by the BN epilogue; keeps the PReLU argument check below quiet)
        dalpha_prev = bn->dgamma; dbias_prev = bn->dbeta;
    }
    if (zprev16 && !zprev) zprev = reinterpret_cast<const float*>(zprev16);      // "has a PReLU mask" below; the kernels read p.Zin16
    const bool z16only = zprev16 != nullptr;
    if (!dz || !w || (!dzprev && !(src16 && dzprev16)) || n <= 0 || cout % 32 || cin % 64 || (stride != 1 && stride != 2) || (ksize != 1 && ksize != 3)) return FTE_EINVAL;
    if (zprev && !alpha_prev) return FTE_EINVAL;
    const Pads pho = same_pads(h, ksize, stride), pwo = same_pads(wd, ksize, stride);
    const DgradLayout lay = dgrad_layout(planner(ctx, EPI_DGRAD), ctx, s);
    if (lay.wino && dzprev && !dzprev16 && !addin16 && !zprev16 && !raw16) {
        // Winograd: the forward algorithm on dz with the rotated, channel-swapped filters; one partial row of dalpha / dbias per row block
        const WinoGeom g = wino_geom(n, h, wd);
        const size_t half_w = lay.wino_half;
        const WinoWs& wl = lay.w;
        if (ws && ws_bytes >= wl.total) {
            if (!aligned16({dz, w, addin, zprev, alpha_prev, raw, dzprev, ws})) return FTE_EINVAL;
            const bool part = zprev && (dalpha_prev || dbias_prev);
            float* V = (float*)((char*)ws + wl.v_off);
            float* U = (float*)((char*)ws + wl.u_off);
            hipError_t e = wino_transform_filter((const float*)w, U, cin, cout, 1, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            e = wino_transform_tiles((const float*)dz, V, n, h, wd, cout, 0, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            WinoMMParams q;
            memset(&q, 0, sizeof(q));
            q.V = V; q.U = U; q.K = cout; q.N = cin; q.g = g;
            q.ADD = addin; q.RAW = raw; q.Zin = zprev; q.alpha = alpha_prev; q.amod = cin; q.DZ = dzprev;
            q.PA = part ? (float*)ws : nullptr; q.PB = part ? (float*)((char*)ws + half_w) : nullptr;
            e = wino_mm(q, EPI_DGRAD, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            if (part) {
                float* scratch = (float*)((char*)ws + 2 * half_w);
                if (dalpha_prev && dbias_prev) return rc(k_reduce_rows2(q.PA, dalpha_prev, q.PB, dbias_prev, nullptr, 1, g.MB, cin, 1, 1.f, scratch, (hipStream_t)stream));
                if (dalpha_prev) return rc(k_reduce_rows(q.PA, dalpha_prev, nullptr, 1, g.MB, cin, 1, 1.f, scratch, (hipStream_t)stream));
                return rc(k_reduce_rows(q.PB, dbias_prev, nullptr, 1, g.MB, cin, 1, 1.f, scratch, (hipStream_t)stream));
            }
            return FTE_OK;
        }
    }
    const DgradClass* cls = lay.cls;
    const int nc = lay.nc;
    const bool merged = lay.merged;
    const long rows = lay.rows;
    const bool want_part = zprev && (dalpha_prev || dbias_prev);
    const size_t half = lay.half, pw_need = lay.pw_bytes;
    if ((want_part || pw_need) && (!ws || ws_bytes < lay.need)) return FTE_EWORKSPACE;
    float* scratch = want_part ? (float*)((char*)ws + lay.scratch_off) : nullptr;
    float* pwbuf = pw_need ? (float*)((char*)ws + lay.pw_off) : nullptr;
    float* PA = want_part ? (float*)ws : nullptr;
    float* PB = want_part ? (float*)((char*)ws + half) : nullptr;
    if (merged) {
        // one launch for all parity classes (each had its own until now: at 36-60 % of the rate of a stride-1 layer,
        // the 1-tap class being a K = cout GEMM that cannot fill the chip on its own)
        const int* order = lay.order;
        const int tile = lay.merged_tile;
        IgemmParams p;
        zero_params(&p);
        const DgradClass& c0 = cls[0];
        p.M = n * c0.hq * c0.wq; p.N = cin; p.a_KC = cout;
        p.A = (const float*)dz; p.a_OH = c0.hq; p.a_OW = c0.wq; p.a_IH = pho.out; p.a_IW = pwo.out; p.a_stride = 1; p.a_ld = cout;
        p.ncls = nc;
        int t = 0;
        for (int k = 0; k < nc; ++k) {
            const DgradClass& c = cls[order[k]];
            p.cls_tap0[k] = t; p.cls_ph[k] = c.ph; p.cls_pw[k] = c.pw;
            for (int j = 0; j < c.ntap; ++j, ++t) { p.a_dh[t] = c.dh[j]; p.a_dw[t] = c.dw[j]; p.b_tapoff[t] = c.wt[j] * cin * cout; }
        }
        p.cls_tap0[nc] = t;
        p.a_NT = t; p.K = t * cout; p.kchunk = p.K;
        p.B = (const float*)w; p.b_ld = cout;
        p.c_OH = c0.hq; p.c_OW = c0.wq; p.c_FH = h; p.c_FW = wd; p.c_step = stride; p.c_ld = cin;
        p.ADD = addin; p.RAW = raw; p.Zin = z16only ? nullptr : zprev; p.alpha = alpha_prev; p.amod = cin; p.DZ = dzprev;
        p.ADD16 = addin16; p.Zin16 = zprev16; p.RAW16 = raw16;
        p.PA = PA; p.PB = PB; p.prow0 = 0;
        if (bn) { p.bn_mu = bn->mean; p.bn_rs = bn->rstd; p.bn_sc = bn->scale; p.bn_sh = bn->shift; p.Zx = zx; p.Zx16 = zx16; }
        p.src16 = src16 ? 1 : 0; p.DZ16 = dzprev16;
        if (!set_bytes(&p, (size_t)n * pho.out * pwo.out * cout, (size_t)ksize * ksize * cin * cout, src16 ? 2 : 4)) return FTE_EINVAL;
        hipError_t e = igemm_launch(p, AL_MK, BL_NK, EPI_DGRAD, tile, 1, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    } else {
    long prow = 0;
    for (int i = 0; i < nc; ++i) {
        const DgradClass& c = cls[i];
        IgemmParams p;
        zero_params(&p);
        p.M = n * c.hq * c.wq; p.N = cin; p.K = c.ntap * cout; p.kchunk = p.K;
        p.A = (const float*)dz; p.a_OH = c.hq; p.a_OW = c.wq; p.a_IH = pho.out; p.a_IW = pwo.out; p.a_stride = 1;
        p.a_ld = cout; p.a_KC = cout; p.a_NT = c.ntap;
        for (int t = 0; t < c.ntap; ++t) {
            p.a_dh[t] = c.dh[t]; p.a_dw[t] = c.dw[t];
            p.b_tapoff[t] = c.wt[t] * cin * cout;
        }
        p.B = (const float*)w; p.b_ld = cout;
        p.src16 = src16 ? 1 : 0; p.DZ16 = dzprev16;
        if (stride == 1) { p.c_OH = 0; }
        else { p.c_OH = c.hq; p.c_OW = c.wq; p.c_FH = h; p.c_FW = wd; p.c_step = stride; p.c_ph = c.ph; p.c_pw = c.pw; }
        p.c_ld = cin;
        p.ADD = addin; p.RAW = raw; p.Zin = z16only ? nullptr : zprev; p.alpha = alpha_prev; p.amod = cin; p.DZ = dzprev;
        p.ADD16 = addin16; p.Zin16 = zprev16; p.RAW16 = raw16;
        p.PA = PA; p.PB = PB;
        if (bn) { p.bn_mu = bn->mean; p.bn_rs = bn->rstd; p.bn_sc = bn->scale; p.bn_sh = bn->shift; p.Zx = zx; p.Zx16 = zx16; }
        if (!set_bytes(&p, (size_t)n * pho.out * pwo.out * cout, (size_t)ksize * ksize * cin * cout, src16 ? 2 : 4)) return FTE_EINVAL;
        hipError_t e = launch_rows(p, c.rp, AL_MK, BL_NK, EPI_DGRAD, prow, pwbuf, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
        prow += c.mtiles;
    }
    }
    if (bn)            // PA = sum g * xhat, PB = sum g per partial row -> dgamma, dbeta, the coefficients of dz = A g + B z + C0
        return rc(l_bn_bwd_finalize(PB, PA, cin, (int)rows, (long)n * h * wd, cin, bn->gamma, bn->mean, bn->rstd, bn->dgamma, bn->dbeta,
                                    bn->coef, (hipStream_t)stream));
    if (want_part) {
        if (dalpha_prev && dbias_prev) {
            hipError_t e = k_reduce_rows2(PA, dalpha_prev, PB, dbias_prev, nullptr, 1, rows, cin, 1, 1.f, scratch, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
        } else {
            if (dalpha_prev) { hipError_t e = k_reduce_rows(PA, dalpha_prev, nullptr, 1, rows, cin, 1, 1.f, scratch, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
            if (dbias_prev) { hipError_t e = k_reduce_rows(PB, dbias_prev, nullptr, 1, rows, cin, 1, 1.f, scratch, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
        }
    }
    return FTE_OK;
}

int fte_conv2d_dgrad(const float* dz, const float* w, const float* addin, const float* zprev,
                     const float* alpha_prev, float* raw, float* dzprev, float* dalpha_prev, float* dbias_prev,
                     int n, int h, int wd, int cin, int cout, int ksize, int stride, void* ws, size_t ws_bytes, void* stream) {
    DgradArgs a = {ctx32(), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.dz = dz; a.w = w;
    a.addin = addin; a.zprev = zprev; a.alpha_prev = alpha_prev; a.raw = raw; a.dzprev = dzprev; a.dalpha_prev = dalpha_prev; a.dbias_prev = dbias_prev;
    return a.run();
}
int fte_conv2d_dgrad16(const uint16_t* dz16, const uint16_t* w16, const float* addin, const float* zprev,
                       const float* alpha_prev, float* raw, float* dzprev, uint16_t* dzprev16, float* dalpha_prev, float* dbias_prev,
                       int n, int h, int wd, int cin, int cout, int ksize, int stride, void* ws, size_t ws_bytes, void* stream) {
    DgradArgs a = {ctx16(false), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.dz = dz16; a.w = w16; a.src16 = true;
    a.addin = addin; a.zprev = zprev; a.alpha_prev = alpha_prev; a.raw = raw; a.dzprev = dzprev; a.dzprev16 = dzprev16;
    a.dalpha_prev = dalpha_prev; a.dbias_prev = dbias_prev;
    return a.run();
}

int fte_conv2d_dgrad_s16(const uint16_t* dz16, const uint16_t* w16, const uint16_t* addin16, const uint16_t* zprev16,
                         const float* alpha_prev, uint16_t* raw16, uint16_t* dzprev16, float* dalpha_prev, float* dbias_prev,
                         int n, int h, int wd, int cin, int cout, int ksize, int stride, void* ws, size_t ws_bytes, void* stream) {
    if (!dzprev16) return FTE_EINVAL;
    DgradArgs a = {ctx16(true), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.dz = dz16; a.w = w16; a.src16 = true;
    a.alpha_prev = alpha_prev; a.dzprev16 = dzprev16; a.dalpha_prev = dalpha_prev; a.dbias_prev = dbias_prev;
    a.addin16 = addin16; a.zprev16 = zprev16; a.raw16 = raw16;
    return a.run();
}

size_t fte_conv3x3_dgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride) {
    return fte_conv2d_dgrad_ws_bytes(n, h, wd, cin, cout, 3, stride);
}
int fte_conv3x3_dgrad(const float* dz, const float* w, const float* addin, const float* zprev,
                      const float* alpha_prev, float* raw, float* dzprev, float* dalpha_prev, float* dbias_prev,
                      int n, int h, int wd, int cin, int cout, int stride, void* ws, size_t ws_bytes, void* stream) {
    return fte_conv2d_dgrad(dz, w, addin, zprev, alpha_prev, raw, dzprev, dalpha_prev, dbias_prev,
                            n, h, wd, cin, cout, 3, stride, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
namespace {
// The two resident bf16 kernels (wgrad16.hip): all nine taps per block, LDS-DMA, slot-range splits (3x3 / stride 1), and the pointwise one
// (1x1 / stride 1, pixel-range splits).  wgrad16.hip owns their plans; the slabs of a split reduction sit at offset 0 of the workspace.
struct Resident16 {
    int ksize;
    bool (*plan)(int, int, int, int, int, Wgrad16Params*, int*);
    hipError_t (*launch)(const Wgrad16Params&, int, hipStream_t);
    const char* sym[7];      // kernel symbol per plan cfg
};
const Resident16 RESIDENT3 = {3, wgrad16_plan, wgrad16_launch, {"wgrad16_kernel<32,256,3,128>", "wgrad16_kernel<64,128,3,128>", "wgrad16_kernel<64,64,3,192>"}};
const Resident16 RESIDENT1 = {1, wgrad16p_plan, wgrad16p_launch,
                              {"wgrad16p_kernel<128,256,2,4>", "wgrad16p_kernel<256,128,4,2>", "wgrad16p_kernel<128,128,2,4>", "wgrad16p_kernel<64,256,1,8>",
                               "wgrad16p_kernel<256,64,8,1>", "wgrad16p_kernel<64,128,2,4>", "wgrad16p_kernel<128,64,4,2>"}};
inline bool resident_takes(const Resident16& k, const ConvShape& s, Wgrad16Params* g, int* cfg) {
    return s.ksize == k.ksize && s.stride == 1 && k.plan(s.n, s.h, s.wd, s.cin, s.cout, g, cfg);
}
inline size_t resident_slab_bytes(const Wgrad16Params& g) { return g.S > 1 ? (size_t)g.S * g.slab * sizeof(float) : 0; }
inline size_t resident_ws_bytes(const Resident16& k, const ConvShape& s) {
    Wgrad16Params g;
    int cfg = 0;
    return resident_takes(k, s, &g, &cfg) ? resident_slab_bytes(g) : 0;
}
// -1: the kernel does not take the layer, or the workspace cannot hold its slabs -- the caller goes on to the tile kernels
int wgrad_resident(const Resident16& k, const ConvShape& s, int K, const void* x, const void* dz, float* dw, void* ws, size_t ws_bytes, hipStream_t st) {
    Wgrad16Params g;
    int cfg = 0;
    if (!resident_takes(k, s, &g, &cfg)) return -1;
    const size_t gneed = resident_slab_bytes(g);
    const size_t xb = (size_t)s.n * s.h * s.wd * s.cin * 2, db = (size_t)s.n * s.h * s.wd * s.cout * 2;
    if ((gneed && (!ws || ws_bytes < gneed)) || xb >= (1ull << 31) || db >= (1ull << 31)) return -1;
    g.x = (const unsigned short*)x; g.dz = (const unsigned short*)dz;
    g.out = g.S > 1 ? (float*)ws : dw;
    g.x_bytes = (unsigned)xb; g.dz_bytes = (unsigned)db;
    if (k.ksize == 3)
        for (int r = 0; r < 3; ++r)
            for (int s2 = 0; s2 < 3; ++s2) { g.dh[r * 3 + s2] = r - 1; g.dw[r * 3 + s2] = s2 - 1; }
    const int sig[5] = {AL_KM, BL_KN, EPI_FWD, 7, g.S};              // tile id 7: the resident kernels (bench.py TILES)
    const double rows = (double)k.ksize * k.ksize * s.cin;
    const int h = igemm_prof_begin(sig, (int)rows, s.cout, K, 2.0 * rows * s.cout * (double)K, (double)xb + (double)db + (double)g.S * g.slab * 4.0, st);
    hipError_t e = k.launch(g, cfg, st);
    igemm_prof_end(h, k.sym[cfg], st);
    if (e != hipSuccess) return (int)e;
    if (g.S > 1) return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, g.S, g.slab, 1, 1.f, nullptr, st));
    return FTE_OK;
}
}  // namespace

size_t fte_conv2d_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride) {
    if (n <= 0 || cin <= 0 || cin % 4 || cout <= 0 || cout % 64) return 0;
    const ConvShape s = {n, h, wd, cin, cout, ksize, stride};
    return wgrad_layout(knobs(), ctx32(), s, resident_ws_bytes(RESIDENT3, s), resident_ws_bytes(RESIDENT1, s)).total;
}
size_t fte_conv3x3_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride) {
    return fte_conv2d_wgrad_ws_bytes(n, h, wd, cin, cout, 3, stride);
}

static int conv2d_wgrad_impl(PlanCtx ctx, const void* x, const void* dz, bool src16, float* dw, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                             void* ws, size_t ws_bytes, void* stream, const float* vpack = nullptr) {
    if (src16 && (cin % 8 || cout % 8)) return FTE_EINVAL;
    // (x may be absent beside a kept V: that call reads the pack or fails below, it never reaches a path that reads x)
    if ((!x && !vpack) || !dz || !dw || n <= 0 || cin % 4 || cout % 64 || (stride != 1 && stride != 2) || (ksize != 1 && ksize != 3)) return FTE_EINVAL;
    const Pads ph = same_pads(h, ksize, stride), pw = same_pads(wd, ksize, stride);
    {       // tensors of 2 GiB or more (32-bit buffer offsets): an argument error, reported before any workspace question
        const size_t lim = (size_t)1 << 31, es = src16 ? 2 : 4;
        if ((size_t)n * h * wd * cin * es >= lim || (size_t)n * ph.out * pw.out * cout * es >= lim) return FTE_EINVAL;
    }
    const ConvShape s = {n, h, wd, cin, cout, ksize, stride};
    const WgradLayout lay = wgrad_layout(knobs(), ctx, s);
    const int tile = lay.tile, splits = lay.splits, kchunk = lay.kchunk, K = lay.K;
    if (lay.wino) {
        // Winograd F(3x3, 2x2): V = B^T d B of x, 16 products over the tiles with U' = G' e G'^T of dz formed in the kernel, A'^T . A' of the sums
        const WinoWs& wl = vpack ? lay.w_kept : lay.w;      // V = B^T d B of x kept by the forward pass (fte_conv3x3_fwd_keep): ws holds the slabs only
        if (ws && ws_bytes >= wl.total) {
            if (!aligned16({x, dz, dw, ws, vpack})) return FTE_EINVAL;
            const float* V = vpack ? vpack : (float*)((char*)ws + wl.v_off);
            float* slabs = (float*)((char*)ws + wl.slab_off);
            hipError_t e = hipSuccess;
            if (!vpack) e = wino_transform_tiles((const float*)x, (float*)((char*)ws + wl.v_off), n, h, wd, cin, 0, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            return rc(wino_wgrad(V, (const float*)dz, slabs, dw, wino_geom(n, h, wd), cin, cout, (hipStream_t)stream));
        }
    }
    if (vpack) return FTE_EWORKSPACE;              // a kept V was handed over and the Winograd path did not run: never silently
    if (src16)
        for (const Resident16* k : {&RESIDENT3, &RESIDENT1}) {
            const int r = wgrad_resident(*k, s, K, x, dz, dw, ws, ws_bytes, (hipStream_t)stream);
            if (r >= 0) return r;
        }
    const size_t need = lay.slab_bytes;
    if (need && (!ws || ws_bytes < need)) return FTE_EWORKSPACE;
    IgemmParams p;
    zero_params(&p);
    p.M = ksize * ksize * cin; p.N = cout; p.K = K; p.kchunk = kchunk;
    p.A = (const float*)x; p.a_OH = ph.out; p.a_OW = pw.out; p.a_IH = h; p.a_IW = wd; p.a_stride = stride;
    p.a_ld = cin; p.a_KC = cin;
    conv_taps(&p, ksize, ph, pw);
    p.B = (const float*)dz; p.b_ld = cout;
    p.c_ld = cout;
    p.slab = (long)p.M * p.N;
    p.Y = splits > 1 ? (float*)ws : dw;
    p.split_major = (knobs().wgrad_split_major && splits > 1) ? splits : 0;
    p.src16 = src16 ? 1 : 0;
    if (!set_bytes(&p, (size_t)n * h * wd * cin, (size_t)K * cout, src16 ? 2 : 4)) return FTE_EINVAL;
    hipError_t e = igemm_launch(p, AL_KM, BL_KN, EPI_FWD, tile, splits, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (splits > 1) return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, splits, p.slab, 1, 1.f, nullptr, (hipStream_t)stream));
    return FTE_OK;
}
int fte_conv2d_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                     void* ws, size_t ws_bytes, void* stream) {
    return conv2d_wgrad_impl(ctx32(), x, dz, false, dw, n, h, wd, cin, cout, ksize, stride, ws, ws_bytes, stream);
}
int fte_conv2d_wgrad16(const uint16_t* x16, const uint16_t* dz16, float* dw, int n, int h, int wd, int cin, int cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream) {
    return conv2d_wgrad_impl(ctx16(false), x16, dz16, true, dw, n, h, wd, cin, cout, ksize, stride, ws, ws_bytes, stream);
}
int fte_conv3x3_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                      void* ws, size_t ws_bytes, void* stream) {
    return fte_conv2d_wgrad(x, dz, dw, n, h, wd, cin, cout, 3, stride, ws, ws_bytes, stream);
}
int fte_conv3x3_wgrad_kept(const float* x, const float* dz, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                           const float* vpack, void* ws, size_t ws_bytes, void* stream) {
    if (vpack && ((uintptr_t)vpack & 15)) return FTE_EINVAL;
    return conv2d_wgrad_impl(ctx32(), x, dz, false, dw, n, h, wd, cin, cout, 3, stride, ws, ws_bytes, stream, vpack);
}

// ------------------------------------------------------------------------------------------------
int fte_conv3x3_first_fwd(const float* x, const float* w, const float* bias, const float* alpha, float* z, float* y,
                          int n, int h, int wd, int cin, int cout, int stride, void* stream) {
    if (!x || !w || !y || (cout != 64 && cout != 32) || (cin != 1 && cin != 3) || !first_conv_shape_ok(n, h, wd, stride)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(k_conv_first_fwd(x, w, bias, alpha, z, y, nullptr, nullptr, n, h, wd, cin, cout, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}
int fte_conv3x3_first_fwd_s16(const float* x, const float* w, const float* bias, const float* alpha, uint16_t* z16, uint16_t* y16,
                              int n, int h, int wd, int cin, int cout, int stride, void* stream) {
    if (!x || !w || !y16 || (cout != 64 && cout != 32) || (cin != 1 && cin != 3) || !first_conv_shape_ok(n, h, wd, stride)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(k_conv_first_fwd(x, w, bias, alpha, nullptr, nullptr, z16, y16, n, h, wd, cin, cout, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}

size_t fte_conv3x3_first_wgrad_ws_bytes(int n, int h, int wd, int cin, int cout, int stride) {
    if ((cout != 64 && cout != 32) || (cin != 1 && cin != 3) || !first_conv_shape_ok(n, h, wd, stride)) return 0;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return align_up((size_t)k_conv_first_wgrad_blocks((long)n * ph.out * pw.out) * 9 * cin * cout * sizeof(float)) + SCRATCH_BYTES;
}

static int conv_first_wgrad_impl(const float* x, const float* dz, const uint16_t* dz16, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (!x || (!dz && !dz16) || !dw || (cout != 64 && cout != 32) || (cin != 1 && cin != 3) || !first_conv_shape_ok(n, h, wd, stride)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int blocks = k_conv_first_wgrad_blocks((long)n * ph.out * pw.out);
    const size_t need = align_up((size_t)blocks * 9 * cin * cout * sizeof(float));
    if (!ws || ws_bytes < need + SCRATCH_BYTES) return FTE_EWORKSPACE;
    hipError_t e = k_conv_first_wgrad(x, dz, dz16, (float*)ws, n, h, wd, cin, cout, ph.out, pw.out, stride, ph.before, pw.before, blocks, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, blocks, 9L * cin * cout, 1, 1.f, (float*)((char*)ws + need), (hipStream_t)stream));
}
int fte_conv3x3_first_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                            void* ws, size_t ws_bytes, void* stream) {
    return conv_first_wgrad_impl(x, dz, nullptr, dw, n, h, wd, cin, cout, stride, ws, ws_bytes, stream);
}
int fte_conv3x3_first_wgrad_s16(const float* x, const uint16_t* dz16, float* dw, int n, int h, int wd, int cin, int cout, int stride,
                                void* ws, size_t ws_bytes, void* stream) {
    return conv_first_wgrad_impl(x, nullptr, dz16, dw, n, h, wd, cin, cout, stride, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// dense
size_t fte_gemm_ws_bytes(int m, int n, int k) {
    // max over nn (m x n, red k), nt (m x k, red n; or its dalpha partials), tn (k x n, red m)
    if (m <= 0 || n <= 0 || k <= 0) return 0;         // no product takes these (and dense_plan divides by the tile count)
    const PlanKnobs& kn = knobs();
    const bool b16 = igemm_get_bf16();
    size_t need = 0, v;
    if (n % 64 == 0) { v = dense_plan(kn, pick_tile(kn, b16, m, n), m, n, k).slab_bytes; if (v > need) need = v; }
    if (k % 64 == 0) {
        v = dense_plan(kn, pick_tile(kn, b16, m, k), m, k, n).slab_bytes; if (v > need) need = v;
        v = align_up((size_t)((m + 63) / 64) * k * sizeof(float)) + SCRATCH_BYTES; if (v > need) need = v;
    }
    if (n % 64 == 0) { v = dense_plan(kn, tn_tile(k, n), k, n, m).slab_bytes; if (v > need) need = v; }
    return need;
}

static int gemm_nn_impl(const float* x, const float* w, const float* bias, float* y, int m, int n, int k, int act,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!x || !w || !y || m <= 0 || n <= 0 || k <= 0 || n % 64 || k % 32 || act < 0 || act > 2) return FTE_EINVAL;
    IgemmParams p;
    zero_params(&p);
    p.M = m; p.N = n; p.K = k;
    plain_a(&p, x, k, k);
    p.B = w; p.b_ld = n; p.c_ld = n;
    if (!set_bytes(&p, (size_t)m * k, (size_t)k * n)) return FTE_EINVAL;
    const int tile = pick_tile(knobs(), igemm_get_bf16(), m, n);
    const DensePlan d = dense_plan(knobs(), tile, m, n, k);
    // (split: the activation rides in the slab reduction's epilogue, no separate pass over y)
    const int r = launch_dense(p, d, AL_MK, BL_KN, tile, y, bias, n, act, ws, ws_bytes, (hipStream_t)stream);
    if (r != FTE_OK || d.splits > 1 || !act) return r;
    return rc(l_act_fwd(y, y, (long)m * n, act - 1, (hipStream_t)stream));
}
int fte_gemm_nn(const float* x, const float* w, const float* bias, float* y, int m, int n, int k,
                void* ws, size_t ws_bytes, void* stream) {
    return gemm_nn_impl(x, w, bias, y, m, n, k, 0, ws, ws_bytes, stream);
}
int fte_gemm_nn_act(const float* x, const float* w, const float* bias, float* y, int m, int n, int k, int act,
                    void* ws, size_t ws_bytes, void* stream) {
    return gemm_nn_impl(x, w, bias, y, m, n, k, act, ws, ws_bytes, stream);
}

int fte_dense_small(const float* a, const float* w, const float* bias, const float* mask, float* out, int m, int n, int k,
                    int trans_w, int act, void* stream) {
    if (!a || !w || !out || m <= 0 || n <= 0 || n % 32 || k <= 0 || k % 128 || act < 0 || act > 2 || (trans_w & ~1)) return FTE_EINVAL;
    return rc(k_dense_small(a, w, bias, mask, out, m, n, k, trans_w != 0, act, igemm_get_bf16(), (hipStream_t)stream));
}

int fte_gemm_nt(const float* dy, const float* w, const float* zprev, const float* alpha_prev, int amod,
                float* raw, float* dx, float* dalpha_prev, int m, int n, int k, void* ws, size_t ws_bytes, void* stream) {
    // dx[m,k] = dy[m,n] @ w[k,n]^T : GEMM with rows m, cols k, reduction n
    if (!dy || !w || !dx || m <= 0 || n <= 0 || k <= 0 || k % 64 || n % 32) return FTE_EINVAL;
    if (zprev && (!alpha_prev || amod <= 0 || k % amod)) return FTE_EINVAL;
    IgemmParams p;
    zero_params(&p);
    p.M = m; p.N = k; p.K = n;
    plain_a(&p, dy, n, n);
    p.B = w; p.b_ld = n; p.c_ld = k;
    if (!set_bytes(&p, (size_t)m * n, (size_t)k * n)) return FTE_EINVAL;
    const int tile = pick_tile(knobs(), igemm_get_bf16(), m, k);
    if (!zprev && !raw)       // plain product, split-K allowed
        return launch_dense(p, dense_plan(knobs(), tile, m, k, n), AL_MK, BL_NK, tile, dx, nullptr, 1, 0, ws, ws_bytes, (hipStream_t)stream);
    p.kchunk = n;
    int bm, bn;
    igemm_tile_dims(tile, &bm, &bn);
    const long mtiles = ((long)m + bm - 1) / bm;
    const bool want_part = zprev && dalpha_prev;
    const size_t part_bytes = align_up((size_t)mtiles * k * sizeof(float));
    if (want_part && (!ws || ws_bytes < part_bytes + SCRATCH_BYTES)) return FTE_EWORKSPACE;
    p.RAW = raw; p.Zin = zprev; p.alpha = alpha_prev; p.amod = zprev ? amod : 1; p.DZ = dx;
    p.PA = want_part ? (float*)ws : nullptr;
    hipError_t e = igemm_launch(p, AL_MK, BL_NK, EPI_DGRAD, tile, 1, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (want_part) return rc(k_reduce_rows((const float*)ws, dalpha_prev, nullptr, 1, mtiles, k, k / amod, 1.f,
                                           (float*)((char*)ws + part_bytes), (hipStream_t)stream));
    return FTE_OK;
}

int fte_gemm_tn(const float* x, const float* dy, float* dw, int m, int n, int k, void* ws, size_t ws_bytes, void* stream) {
    // dw[k,n] = x[m,k]^T @ dy[m,n] : GEMM with rows k, cols n, reduction m
    if (!x || !dy || !dw || m <= 0 || n <= 0 || k <= 0 || n % 64 || k % 4) return FTE_EINVAL;
    IgemmParams p;
    zero_params(&p);
    p.M = k; p.N = n; p.K = m;
    plain_a(&p, x, k, k);
    p.B = dy; p.b_ld = n; p.c_ld = n;
    if (!set_bytes(&p, (size_t)m * k, (size_t)m * n)) return FTE_EINVAL;
    const int tile = tn_tile(k, n);
    return launch_dense(p, dense_plan(knobs(), tile, k, n, m), AL_KM, BL_KN, tile, dw, nullptr, 1, 0, ws, ws_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// loss heads
int fte_softmax_ce_fwd_bwd(const float* logits, const int32_t* labels, float* loss_rows, float* dlogits,
                           int n, int c, int ld, float grad_scale, void* stream) {
    if (!logits || !labels || !loss_rows || !dlogits || n <= 0 || c <= 0 || ld < c) return FTE_EINVAL;
    return rc(k_softmax_ce(logits, labels, loss_rows, dlogits, n, c, ld, grad_scale, (hipStream_t)stream));
}
int fte_focal_loss_fwd_bwd(const float* logits, const int32_t* labels, float* loss_rows, float* dlogits,
                           int n, int c, int ld, float gamma, float alpha, float grad_scale, void* stream) {
    if (!logits || !labels || !loss_rows || !dlogits || n <= 0 || c <= 0 || ld < c || alpha < 1.f) return FTE_EINVAL;
    return rc(k_focal_loss(logits, labels, loss_rows, dlogits, n, c, ld, gamma, alpha, grad_scale, (hipStream_t)stream));
}
int fte_asoftmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float lambda,
                         float* f, float* loss_rows, float* G, float* rowcoef, int n, int c, int ld,
                         float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !loss_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c) return FTE_EINVAL;
    return rc(k_asoftmax(s, xn, wn, labels, lambda, f, loss_rows, G, rowcoef, n, c, ld, grad_scale, (hipStream_t)stream));
}
int fte_margin_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale, float m, float m3,
                               float* f, float* loss_rows, float* G, float* rowcoef, int n, int c, int ld, float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !loss_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c || !(scale > 0.f) || !(m >= 0.f))
        return FTE_EINVAL;
    return rc(k_margin_softmax(s, xn, wn, labels, scale, m, m3, f, loss_rows, G, rowcoef, n, c, ld, grad_scale, (hipStream_t)stream));
}
// the shard [class_lo, class_lo + c) must lie inside [0, num_classes) (the sum in 64 bits: class_lo + c may not wrap)
static bool shard_ok(int class_lo, int num_classes, int c) { return class_lo >= 0 && (long long)class_lo + c <= (long long)num_classes; }
int fte_margin_shard_stats(const float* s, const float* xn, const float* wn, const int32_t* labels, int class_lo, int num_classes, float scale,
                           float m, float m3, float* stats, int n, int c, int ld, void* stream) {
    if (!s || !xn || !wn || !labels || !stats || n <= 0 || c <= 0 || ld < c || !(scale > 0.f) || !(m >= 0.f) || !shard_ok(class_lo, num_classes, c))
        return FTE_EINVAL;
    return rc(k_margin_shard_stats(s, xn, wn, labels, class_lo, num_classes, scale, m, m3, stats, n, c, ld, (hipStream_t)stream));
}
int fte_margin_shard_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, int class_lo, int num_classes, float scale,
                             float m, float m3, const float* all_stats, int R, float* f, float* loss_rows, float* G, float* rowcoef_part,
                             int n, int c, int ld, float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !all_stats || !loss_rows || !G || !rowcoef_part || n <= 0 || c <= 0 || ld < c || !(scale > 0.f) ||
        !(m >= 0.f) || R < 1 || !shard_ok(class_lo, num_classes, c))
        return FTE_EINVAL;
    return rc(k_margin_shard_fwd_bwd(s, xn, wn, labels, class_lo, num_classes, scale, m, m3, all_stats, R, f, loss_rows, G, rowcoef_part,
                                     n, c, ld, grad_scale, (hipStream_t)stream));
}
int fte_margin_softmax_rows_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale,
                                    const float* a_rows, const float* b_rows, float* f, float* loss_rows, float* G, float* rowcoef,
                                    int n, int c, int ld, float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !a_rows || !b_rows || !loss_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c || !(scale > 0.f))
        return FTE_EINVAL;
    return rc(k_margin_softmax_rows(s, xn, wn, labels, scale, a_rows, b_rows, f, loss_rows, G, rowcoef, n, c, ld, grad_scale,
                                    (hipStream_t)stream));
}
int fte_adaface_margins(const float* xn, int n, float m, float h, float t_alpha, int update, float* stats, float* a_rows, float* b_rows,
                        void* stream) {
    if (!xn || !stats || !a_rows || !b_rows || n < 2 || !(m >= 0.f) || !(h > 0.f) || !(t_alpha >= 0.f && t_alpha <= 1.f)) return FTE_EINVAL;
    return rc(k_adaface_margins(xn, n, m, h, t_alpha, update, stats, a_rows, b_rows, (hipStream_t)stream));
}
// S > 0, 0 <= m < pi/2, 0 <= alpha <= 1; a NaN fails every compare
static bool curricular_ok(float scale, float m, float alpha) {
    return scale > 0.f && m >= 0.f && m < 1.57079632679489661923f && alpha >= 0.f && alpha <= 1.f;
}
int fte_curricular_t(const float* s, const float* xn, const float* wn, const int32_t* labels, float alpha, int update, float* t_state,
                     float* t_used, int n, int c, int ld, void* stream) {
    if (!s || !xn || !wn || !labels || !t_state || !t_used || n <= 0 || c <= 0 || ld < c || !curricular_ok(1.f, 0.f, alpha)) return FTE_EINVAL;
    return rc(k_curricular_t(s, xn, wn, labels, alpha, update, t_state, t_used, n, c, ld, (hipStream_t)stream));
}
int fte_curricular_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale, float m,
                                   const float* t_used, float* f, float* loss_rows, float* G, float* rowcoef, int n, int c, int ld,
                                   float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !t_used || !loss_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c || !curricular_ok(scale, m, 0.f))
        return FTE_EINVAL;
    return rc(k_curricular_softmax(s, xn, wn, labels, scale, m, t_used, f, loss_rows, G, rowcoef, n, c, ld, grad_scale, (hipStream_t)stream));
}
int fte_magface_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, float scale, float l_a, float u_a,
                                float l_m, float u_m, float lambda_g, float* f, float* loss_rows, float* reg_rows, float* G, float* rowcoef,
                                int n, int c, int ld, float grad_scale, void* stream) {
    // S > 0, 0 < l_a < u_a, 0 <= l_m <= u_m < pi/2, lambda_g >= 0; a NaN fails every compare
    const bool ok = scale > 0.f && l_a > 0.f && u_a > l_a && l_m >= 0.f && u_m >= l_m && u_m < 1.57079632679489661923f && lambda_g >= 0.f;
    if (!s || !xn || !wn || !labels || !loss_rows || !reg_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c || !ok) return FTE_EINVAL;
    return rc(k_magface_softmax(s, xn, wn, labels, scale, l_a, u_a, l_m, u_m, lambda_g, f, loss_rows, reg_rows, G, rowcoef, n, c, ld, grad_scale,
                                (hipStream_t)stream));
}
int fte_asoftmax_colcoef(const float* G, const float* s, const float* wn, float* colcoef, int n, int c, int ld, void* stream) {
    if (!G || !s || !wn || !colcoef || n <= 0 || c <= 0 || ld < c) return FTE_EINVAL;
    return rc(k_asoftmax_colcoef(G, s, wn, colcoef, n, c, ld, (hipStream_t)stream));
}
int fte_subcenter_margin_softmax_fwd_bwd(const float* s, const float* xn, const float* wn, const int32_t* labels, int K, float scale, float m,
                                         float m3, float* f, float* loss_rows, float* G, float* rowcoef, int n, int c, int ld,
                                         float grad_scale, void* stream) {
    if (!s || !xn || !wn || !labels || !loss_rows || !G || !rowcoef || n <= 0 || c <= 0 || ld < c || !(scale > 0.f) || !(m >= 0.f) ||
        K < 1 || K > 8)
        return FTE_EINVAL;
    return rc(k_subcenter_margin_softmax(s, xn, wn, labels, K, scale, m, m3, f, loss_rows, G, rowcoef, n, c, ld, grad_scale,
                                         (hipStream_t)stream));
}
int fte_subcenter_colcoef(const float* G, const float* s, const float* wn, float* colcoef, int K, int n, int c, int ld, void* stream) {
    if (!G || !s || !wn || !colcoef || n <= 0 || c <= 0 || ld < c || K < 1 || K > 8) return FTE_EINVAL;
    return rc(k_subcenter_colcoef(G, s, wn, colcoef, K, n, c, ld, (hipStream_t)stream));
}
int fte_subcenter_assign(const float* x, const float* wt, const int32_t* labels, int K, int32_t* sel, float* cosv, int n, int d, int c,
                         void* stream) {
    if (!x || !wt || !labels || !sel || !cosv || n <= 0 || d <= 0 || c <= 0 || K < 1 || K > 8) return FTE_EINVAL;
    return rc(k_subcenter_assign(x, wt, labels, K, sel, cosv, n, d, c, (hipStream_t)stream));
}
int fte_row_norms(const float* a, float* out, int rows, int cols, int ld, void* stream) {
    if (!a || !out || rows <= 0 || cols <= 0 || ld < cols) return FTE_EINVAL;
    return rc(k_row_norms(a, out, rows, cols, ld, (hipStream_t)stream));
}
int fte_col_norms(const float* a, float* out, int rows, int cols, int ld, void* stream) {
    if (!a || !out || rows <= 0 || cols <= 0 || ld < cols) return FTE_EINVAL;
    return rc(k_col_norms(a, out, rows, cols, ld, (hipStream_t)stream));
}
int fte_flip_width(const float* x, float* y, int n, int h, int wd, int c, void* stream) {
    if (!x || !y || x == y || n <= 0 || h <= 0 || wd <= 0 || c <= 0) return FTE_EINVAL;
    if ((c % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15)) return FTE_EINVAL;
    return rc(k_flip_w(x, y, (long)n * h, wd, c, (hipStream_t)stream));
}
int fte_axpby(float a, const float* x, float b, const float* y, float* out, long n, void* stream) {
    if (!x || !y || !out || n <= 0) return FTE_EINVAL;
    return rc(k_axpby(a, x, b, y, out, n, (hipStream_t)stream));
}
int fte_add_scaled_rows_cols(float* a, const float* b, const float* rcf, const float* cc, int rows, int cols, int ld, void* stream) {
    if (!a || !b || rows <= 0 || cols <= 0 || ld < cols) return FTE_EINVAL;
    return rc(k_add_scaled(a, b, rcf, cc, rows, cols, ld, (hipStream_t)stream));
}
int fte_center_loss_fwd_bwd_update(const float* feat, const int32_t* labels, float* centers, float* loss_rows, float* dfeat,
                                   int n, int d, int num_classes, float alpha, float grad_scale, void* ws, size_t ws_bytes, void* stream) {
    if (!feat || !labels || !centers || !loss_rows || !dfeat || n <= 0 || d <= 0 || num_classes <= 0) return FTE_EINVAL;
    if (!ws || ws_bytes < (size_t)n * d * sizeof(float)) return FTE_EWORKSPACE;
    return rc(k_center_loss(feat, labels, centers, loss_rows, dfeat, n, d, num_classes, alpha, grad_scale, (float*)ws, (hipStream_t)stream));
}
int fte_center_scatter_update(const float* diff, const int32_t* labels, float* centers, int n, int d, int num_classes, float alpha, void* stream) {
    if (!diff || !labels || !centers || n <= 0 || d <= 0 || num_classes <= 0) return FTE_EINVAL;
    return rc(k_center_update(diff, labels, centers, n, d, num_classes, alpha, (hipStream_t)stream));
}
int fte_batch_hard_triplet_fwd_bwd(const float* feat, const int32_t* labels, float margin, int soft_margin, float loss_weight,
                                   float* loss_rows, float* dfeat, int n, int d, void* ws, size_t ws_bytes, void* stream) {
    // n <= 8192: triplet_grad_kernel keeps a coefficient row of n floats in LDS (and 2*n*n floats of workspace stay below 2 GiB)
    if (!feat || !labels || !loss_rows || !dfeat || n <= 0 || n > 8192 || d <= 0) return FTE_EINVAL;
    if (!ws || ws_bytes < (size_t)2 * n * n * sizeof(float)) return FTE_EWORKSPACE;
    return rc(k_triplet(feat, labels, margin, soft_margin != 0, loss_weight, loss_rows, dfeat, n, d, (float*)ws, (hipStream_t)stream));
}

// ------------------------------------------------------------------------------------------------
// reductions / optimizers
int fte_reduce_rows(const float* in, float* out, const float* bias, int bmod, long rows, long cols, int fold, float scale, void* stream) {
    if (!in || !out || rows <= 0 || cols <= 0 || fold <= 0 || cols % fold) return FTE_EINVAL;
    return rc(k_reduce_rows(in, out, bias, bmod > 0 ? bmod : 1, rows, cols, fold, scale, nullptr, (hipStream_t)stream));
}
int fte_sumsq(const float* a, long n, float scale, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !out || n <= 0 || ((uintptr_t)a & 15)) return FTE_EINVAL;
    if (!ws || ws_bytes < 1024 * sizeof(float)) return FTE_EWORKSPACE;
    return rc(k_sum(a, n, scale, out, (float*)ws, true, (hipStream_t)stream));
}
int fte_sum(const float* a, long n, float scale, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !out || n <= 0 || ((uintptr_t)a & 15)) return FTE_EINVAL;
    if (!ws || ws_bytes < 1024 * sizeof(float)) return FTE_EWORKSPACE;
    return rc(k_sum(a, n, scale, out, (float*)ws, false, (hipStream_t)stream));
}
int fte_momentum_update(float* w, float* acc, const float* g, long n, float lr, float mom, float wd, float gscale, void* stream) {
    if (!w || !acc || !g || n <= 0 || (((uintptr_t)w | (uintptr_t)acc | (uintptr_t)g) & 15)) return FTE_EINVAL;
    return rc(k_momentum(w, acc, g, n, lr, mom, wd, gscale, (hipStream_t)stream));
}
int fte_adam_update(float* w, float* m, float* v, const float* g, long n, float lr, float b1, float b2, float eps,
                    float wd, float gscale, int t, void* stream) {
    if (!w || !m || !v || !g || n <= 0 || t < 1) return FTE_EINVAL;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t));
    return rc(k_adam(w, m, v, g, n, (float)lr_t, b1, b2, eps, wd, gscale, (hipStream_t)stream));
}

// ------------------------------------------------------------------------------------------------
// layers of the BN / pooling nets
// split partials (3 per channel: n, mean, M2) + the group partials of the in-launch finalize (one per 16 splits) + the backward coefficients
size_t fte_bn_ws_bytes(int c) { return ((size_t)BN_MAX_SPLITS * 3 * c + (size_t)(BN_MAX_SPLITS / 16) * 3 * c + 3 * (size_t)c) * sizeof(float); }

int fte_bn_train_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y,
                     float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                     long rows, int c, float eps, float decay, int relu, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !gamma || !beta || !y || !mean || !rstd || !scale || !shift || rows <= 0 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    hipError_t e = l_bn_train_stats(z, gamma, beta, rows, c, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                                    (float*)ws, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_apply(z, scale, shift, res, y, rows, c, relu, (hipStream_t)stream));
}
int fte_bn_infer_fwd(const float* z, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                     const float* res, float* y, float* scale, float* shift, long rows, int c, float eps, int relu, void* stream) {
    if (!z || !gamma || !beta || !moving_mean || !moving_var || !y || !scale || !shift || rows <= 0 || c % 4) return FTE_EINVAL;
    hipError_t e = l_bn_infer_coef(gamma, beta, moving_mean, moving_var, eps, c, scale, shift, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_apply(z, scale, shift, res, y, rows, c, relu, (hipStream_t)stream));
}
int fte_bn_train_bwd(const float* dy, const float* ymask, const float* z, const float* gamma, const float* mean,
                     const float* rstd, float* dz, float* dgamma, float* dbeta, long rows, int c,
                     void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !z || !gamma || !mean || !rstd || !dz || !dgamma || !dbeta || rows <= 0 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_bwd(dy, ymask, z, gamma, mean, rstd, nullptr, nullptr, nullptr, dz, dgamma, dbeta, rows, c, (float*)ws, (hipStream_t)stream));
}
int fte_bn_train_bwd_res(const float* dy, const float* y, const float* z, const float* gamma, const float* mean, const float* rstd,
                         float* g_out, float* dz, float* dgamma, float* dbeta, long rows, int c,
                         void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !y || !z || !gamma || !mean || !rstd || !g_out || !dz || !dgamma || !dbeta || rows <= 0 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_bwd(dy, y, z, gamma, mean, rstd, nullptr, nullptr, g_out, dz, dgamma, dbeta, rows, c, (float*)ws, (hipStream_t)stream));
}
int fte_bn_train_bwd_zmask(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd,
                           const float* scale, const float* shift, float* dz, float* dgamma, float* dbeta, long rows, int c,
                           void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !z || !gamma || !mean || !rstd || !scale || !shift || !dz || !dgamma || !dbeta || rows <= 0 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_bwd(dy, nullptr, z, gamma, mean, rstd, scale, shift, nullptr, dz, dgamma, dbeta, rows, c, (float*)ws, (hipStream_t)stream));
}
int fte_bn_train_stats(const float* z, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift,
                       float* moving_mean, float* moving_var, long rows, int c, float eps, float decay,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!z || !gamma || !beta || !mean || !rstd || !scale || !shift || rows <= 0 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_train_stats(z, gamma, beta, rows, c, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                               (float*)ws, (hipStream_t)stream));
}
int fte_bn_infer_coef(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                      float* scale, float* shift, int c, float eps, void* stream) {
    if (!gamma || !beta || !moving_mean || !moving_var || !scale || !shift || c <= 0) return FTE_EINVAL;
    return rc(l_bn_infer_coef(gamma, beta, moving_mean, moving_var, eps, c, scale, shift, (hipStream_t)stream));
}
// BN + PReLU (iresnet.hip)
size_t fte_bn_prelu_ws_bytes(int c) { return c > 0 ? l_bn_prelu_ws_floats(c) * sizeof(float) : 0; }
int fte_bn_prelu_apply(const float* z, const float* scale, const float* shift, const float* alpha, float* y, long rows, int c,
                       void* stream) {
    if (!z || !scale || !shift || !alpha || !y || rows <= 0 || c < 4 || c % 4) return FTE_EINVAL;
    return rc(l_bn_prelu_apply(z, scale, shift, alpha, y, rows, c, (hipStream_t)stream));
}
int fte_bn_prelu_infer_fwd(const float* z, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                           const float* alpha, float* y, float* scale, float* shift, long rows, int c, float eps, void* stream) {
    if (!z || !gamma || !beta || !moving_mean || !moving_var || !alpha || !y || !scale || !shift || rows <= 0 || c < 4 || c % 4) return FTE_EINVAL;
    hipError_t e = l_bn_infer_coef(gamma, beta, moving_mean, moving_var, eps, c, scale, shift, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_prelu_apply(z, scale, shift, alpha, y, rows, c, (hipStream_t)stream));
}
int fte_bn_prelu_train_bwd(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd,
                           const float* scale, const float* shift, const float* alpha, float* dz, float* dgamma, float* dbeta,
                           float* dalpha, long rows, int c, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !z || !gamma || !mean || !rstd || !scale || !shift || !alpha || !dz || !dgamma || !dbeta || !dalpha || rows <= 0 ||
        c < 4 || c % 4) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_prelu_ws_bytes(c)) return FTE_EINVAL;      // (fte.h: one refusal code for this block)
    return rc(l_bn_prelu_bwd(dy, z, gamma, mean, rstd, scale, shift, alpha, dz, dgamma, dbeta, dalpha, rows, c, (float*)ws, (hipStream_t)stream));
}
// BN + SE + shortcut, no activation (iresnet.hip)
static bool se_lin_args_ok(int n, int hw, int c) { return n >= 1 && hw >= 1 && c >= 4 && c % 4 == 0; }
size_t fte_se_lin_ws_bytes(int n, int hw, int c) { return se_lin_args_ok(n, hw, c) ? l_se_lin_ws_floats(n, hw, c) * sizeof(float) : 0; }
int fte_se_lin_squeeze(const float* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq, float* xm,
                       int n, int hw, int c, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !scale || !shift || !sq || (xm && (!mean || !rstd)) || !se_lin_args_ok(n, hw, c)) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_se_lin_ws_bytes(n, hw, c)) return FTE_EINVAL;      // (fte.h: one refusal code for this block)
    return rc(l_se_lin_squeeze(z, scale, shift, mean, rstd, sq, xm, n, hw, c, (float*)ws, (hipStream_t)stream));
}
int fte_se_lin_apply_fwd(const float* z, const float* scale, const float* shift, const float* gate, const float* shortcut, float* out,
                         int n, int hw, int c, void* stream) {
    if (!z || !scale || !shift || !gate || !shortcut || !out || !se_lin_args_ok(n, hw, c)) return FTE_EINVAL;
    return rc(l_se_lin_apply(z, scale, shift, gate, shortcut, out, n, hw, c, (hipStream_t)stream));
}
int fte_se_lin_bwd_sums(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        const float* gate, float* s1, float* s2, float* dgate, int n, int hw, int c, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !z || !gamma || !beta || !mean || !rstd || !gate || !s1 || !s2 || !dgate || !se_lin_args_ok(n, hw, c)) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_se_lin_ws_bytes(n, hw, c)) return FTE_EINVAL;
    return rc(l_se_lin_bwd_sums(dy, z, gamma, beta, mean, rstd, gate, s1, s2, dgate, n, hw, c, (float*)ws, (hipStream_t)stream));
}
int fte_relu_bwd(const float* dy, const float* y, float* g, long n, void* stream) {
    if (!dy || !y || !g || n <= 0 || n % 4) return FTE_EINVAL;
    return rc(l_relu_bwd(dy, y, g, n, (hipStream_t)stream));
}
int fte_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int wd, int c, void* stream) {
    if (!x || !y || !idx || n <= 0 || c % 4) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, 2), pw = same_pads(wd, 3, 2);
    return rc(l_maxpool_fwd(x, y, idx, n, h, wd, c, ph.out, pw.out, ph.before, pw.before, (hipStream_t)stream));
}
int fte_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int wd, int c, void* stream) {
    if (!dy || !idx || !dx || n <= 0 || c % 4) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, 2), pw = same_pads(wd, 3, 2);
    return rc(l_maxpool_bwd(dy, idx, dx, n, h, wd, c, ph.out, pw.out, ph.before, pw.before, (hipStream_t)stream));
}
int fte_gap_fwd(const float* x, float* y, int n, int hw, int c, void* stream) {
    if (!x || !y || n <= 0 || hw <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_gap_fwd(x, y, n, hw, c, (hipStream_t)stream));
}
int fte_gap_bwd(const float* dy, float* dx, int n, int hw, int c, void* stream) {
    if (!dy || !dx || n <= 0 || hw <= 0 || c <= 0) return FTE_EINVAL;
    return rc(l_gap_bwd(dy, dx, n, hw, c, (hipStream_t)stream));
}
// ---- bf16 STORAGE twins of the BN-net layers (fte.h): flags bit 0 (FTE_S16_Z) = z / dz are bf16, bit 1 (FTE_S16_A) = y / shortcut /
// dy / masked gradient are bf16; channel counts of the float4 layouts only (c % 4 == 0, c >= 32)
static inline const float* f32p(const void* p) { return reinterpret_cast<const float*>(p); }
static inline float* f32p(void* p) { return reinterpret_cast<float*>(p); }
int fte_bn_train_fwd_s16(const void* z, const float* gamma, const float* beta, const void* res, void* y,
                         float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                         long rows, int c, float eps, float decay, int relu, int flags, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !gamma || !beta || !y || !mean || !rstd || !scale || !shift || rows <= 0 || c % 4 || c < 32 || (flags & ~3)) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    hipError_t e = l_bn_train_stats(f32p(z), gamma, beta, rows, c, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                                    (float*)ws, (hipStream_t)stream, flags);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_apply(f32p(z), scale, shift, f32p(res), f32p(y), rows, c, relu, (hipStream_t)stream, flags));
}
int fte_bn_infer_fwd_s16(const void* z, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                         const void* res, void* y, float* scale, float* shift, long rows, int c, float eps, int relu, int flags, void* stream) {
    if (!z || !gamma || !beta || !moving_mean || !moving_var || !y || !scale || !shift || rows <= 0 || c % 4 || (flags & ~3)) return FTE_EINVAL;
    hipError_t e = l_bn_infer_coef(gamma, beta, moving_mean, moving_var, eps, c, scale, shift, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_apply(f32p(z), scale, shift, f32p(res), f32p(y), rows, c, relu, (hipStream_t)stream, flags));
}
int fte_bn_train_bwd_s16(const void* dy, const void* y, const void* z, const float* gamma, const float* mean, const float* rstd,
                         const float* scale, const float* shift, void* g_out, void* dz, float* dgamma, float* dbeta,
                         long rows, int c, int flags, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !z || !gamma || !mean || !rstd || !dz || !dgamma || !dbeta || rows <= 0 || c % 4 || c < 32 || (flags & ~3)) return FTE_EINVAL;
    if ((g_out && !y) || ((scale == nullptr) != (shift == nullptr)) || (scale && (g_out || y))) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_bwd(f32p(dy), f32p(y), f32p(z), gamma, mean, rstd, scale, shift, f32p(g_out), f32p(dz), dgamma, dbeta, rows, c,
                       (float*)ws, (hipStream_t)stream, flags));
}
// ---- "BN fusion": conv -> BN pairs of the graph nets (fte.h) -----------------------------------------------------------------------
size_t fte_conv2d_bn_fwd_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride) {
    if (n <= 0 || cin <= 0 || cout <= 0 || (stride != 1 && stride != 2)) return 0;
    const Pads ph = same_pads(h, ksize, stride), pw = same_pads(wd, ksize, stride);
    const size_t rows = ((size_t)n * ph.out * pw.out + 63) / 64 + 2;      // at most one partial row per 64 output rows
    return align_up(rows * 3 * cout * sizeof(float));
}
int fte_conv2d_bn_fwd_folds(int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16) {
    Pw16Params pw;
    return s16 == 1 && ksize == 1 && stride == 1 && n > 0 && h > 0 && wd > 0 && pw16_plan((long)n * h * wd, cin, cout, PW_EPI_STATS, &pw) ? 1 : 0;
}
int fte_conv2d_bn_fwd(const void* x, const void* w, void* z, const float* gamma, const float* beta, float* mean, float* rstd,
                      float* scale, float* shift, float* moving_mean, float* moving_var, float eps, float decay,
                      const float* in_scale, const float* in_shift, void* y_side,
                      int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !w || !z || !gamma || !beta || !mean || !rstd || !scale || !shift || (s16 & ~1) || ((moving_mean == nullptr) != (moving_var == nullptr)))
        return FTE_EINVAL;      // (x / w here: the streaming pointwise path below does not go through FwdArgs::run's checks)
    if (((in_scale == nullptr) != (in_shift == nullptr)) || (in_scale && !y_side) ||
        (in_scale && !fte_conv2d_bn_fwd_folds(n, h, wd, cin, cout, ksize, stride, s16))) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_conv2d_bn_fwd_ws_bytes(n, h, wd, cin, cout, ksize, stride)) return FTE_EWORKSPACE;
    int rows = 0;
    Pw16Params pw;
    memset(&pw, 0, sizeof(pw));
    if (s16 && ksize == 1 && stride == 1 && pw16_plan((long)n * h * wd, cin, cout, PW_EPI_STATS, &pw)) {
        // the streaming pointwise kernel (pw16.hip): filter slice resident in LDS, statistics of the stored rows from its epilogue
        pw.A = (const unsigned short*)x; pw.W = (const unsigned short*)w; pw.OUT = (unsigned short*)z; pw.part = (float*)ws;
        pw.c0 = in_scale; pw.c1 = in_shift; pw.SIDE = (unsigned short*)y_side;
        const long M = (long)n * h * wd;
        const int sig[5] = {AL_MK, BL_NK, EPI_FWD, 8, 1};                         // tile id 8: the streaming pointwise kernel
        const int hr = igemm_prof_begin(sig, (int)M, cout, cin, 2.0 * M * cout * (double)cin, 2.0 * M * (cin + cout) + 2.0 * cin * cout, (hipStream_t)stream);
        hipError_t he = pw16_launch(pw, in_scale ? PW_PRO_FWD : PW_PRO_NONE, PW_EPI_STATS, (hipStream_t)stream);
        char sym[64];
        snprintf(sym, sizeof(sym), "pw16_kernel<%d,%d,%d,%d,%d>", cin, cout / pw.nct, pw16_waves(pw, in_scale ? PW_PRO_FWD : PW_PRO_NONE, PW_EPI_STATS), in_scale ? PW_PRO_FWD : PW_PRO_NONE, PW_EPI_STATS);
        igemm_prof_end(hr, sym, (hipStream_t)stream);
        if (he != hipSuccess) return (int)he;
        return rc(l_bn_finalize((const float*)ws, pw.nrb, gamma, beta, cout, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                                (hipStream_t)stream));
    }
    FwdArgs a = {s16 ? ctx16(true, true) : ctx32(true), {n, h, wd, cin, cout, ksize, stride}, nullptr, 0, stream};      // (a bn context never splits: ws holds the statistics rows only)
    a.x = x; a.w = w; a.src16 = s16 != 0; a.stat_part = (float*)ws; a.stat_rows = &rows;
    if (s16) a.y16 = (uint16_t*)z; else a.y = (float*)z;
    const int e = a.run();
    if (e != FTE_OK) return e;
    return rc(l_bn_finalize((const float*)ws, rows, gamma, beta, cout, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                            (hipStream_t)stream));
}
size_t fte_conv2d_dgrad_bn_ws_bytes(int n, int h, int wd, int cin, int cout, int ksize, int stride) {
    return dgrad_ws_bytes({n, h, wd, cin, cout, ksize, stride}, true);
}
int fte_conv2d_dgrad_bn(const void* dz, const void* w, const void* addin, const void* zbn, const void* ybn,
                        const float* gamma, const float* mean, const float* rstd, const float* bn_scale, const float* bn_shift,
                        void* g, float* dgamma, float* dbeta, float* coef,
                        int n, int h, int wd, int cin, int cout, int ksize, int stride, int s16, void* ws, size_t ws_bytes, void* stream) {
    if (!dz || !w || !zbn || !gamma || !mean || !rstd || !g || !dgamma || !dbeta || !coef || (s16 & ~1) || ((bn_scale == nullptr) != (bn_shift == nullptr)) ||
        (bn_scale && ybn))
        return FTE_EINVAL;
    const DgradBn bn = {zbn, ybn, gamma, mean, rstd, bn_scale, bn_shift, dgamma, dbeta, coef};
    Pw16Params pw;
    memset(&pw, 0, sizeof(pw));
    // (opt-in, FTE_PW16_DGRAD=1: measured SLOWER than the tile kernel's BN epilogue at 128 images -- 28x28 128<-256 69 vs 46 us, 14x14
    // 512<-256 87 vs 58: the K = 256 form runs four waves per CU, too few to hide the row pass's three input loads)
    static const bool pw_dgrad = getenv("FTE_PW16_DGRAD") && atoi(getenv("FTE_PW16_DGRAD")) == 1;
    if (pw_dgrad && s16 && ksize == 1 && stride == 1 && n > 0 && pw16_plan((long)n * h * wd, cout, cin, PW_EPI_BN, &pw)) {
        // the streaming pointwise kernel (pw16.hip): OUT[M, cin] = dz[M, cout] * W[cin, cout]^T (the HWIO pack's rows are its k-contiguous
        // filter rows), mask and sums in its row-coalesced epilogue, one partial row per block
        const size_t need = 2 * (size_t)pw.nrb * cin * sizeof(float);
        if (!ws || ws_bytes < need) return FTE_EWORKSPACE;
        pw.A = (const unsigned short*)dz; pw.W = (const unsigned short*)w; pw.OUT = (unsigned short*)g;
        pw.ADD = (const unsigned short*)addin;
        pw.Zm = (const unsigned short*)((!bn_scale && ybn) ? ybn : zbn);
        pw.Zx = (const unsigned short*)((!bn_scale && ybn) ? zbn : nullptr);
        pw.mu = mean; pw.rs = rstd; pw.sc = bn_scale; pw.sh = bn_shift;
        pw.part = (float*)ws; pw.pgx = (float*)ws + (size_t)pw.nrb * cin;
        hipError_t he = pw16_launch(pw, PW_PRO_NONE, PW_EPI_BN, (hipStream_t)stream);
        if (he != hipSuccess) return (int)he;
        return rc(l_bn_bwd_finalize(pw.part, pw.pgx, cin, pw.nrb, (long)n * h * wd, cin, gamma, mean, rstd, dgamma, dbeta, coef, (hipStream_t)stream));
    }
    DgradArgs a = {s16 ? ctx16(true, true) : ctx32(true), {n, h, wd, cin, cout, ksize, stride}, ws, ws_bytes, stream};
    a.dz = dz; a.w = w; a.src16 = s16 != 0; a.bn = &bn;
    if (s16) { a.addin16 = (const uint16_t*)addin; a.dzprev16 = (uint16_t*)g; }
    else { a.addin = (const float*)addin; a.dzprev = (float*)g; }
    return a.run();
}
int fte_bn_apply(const void* z, const float* scale, const float* shift, const void* res, void* y, long rows, int c, int relu, int flags, void* stream) {
    if (!z || !scale || !shift || !y || rows <= 0 || c % 4 || (flags & ~3) || (flags && c < 32)) return FTE_EINVAL;
    return rc(l_bn_apply(f32p(z), scale, shift, f32p(res), f32p(y), rows, c, relu, (hipStream_t)stream, flags));
}
int fte_bn_bwd_apply(const void* g, const void* z, const float* coef, void* dz, long rows, int c, int flags, void* stream) {
    if (!g || !z || !coef || !dz || rows <= 0 || c % 4 || (flags & ~3) || (flags && c < 32)) return FTE_EINVAL;
    return rc(l_bn_bwd_apply(f32p(g), f32p(z), coef, f32p(dz), rows, c, (hipStream_t)stream, flags));
}
size_t fte_gconv3x3_bn_ws_bytes(int n, int h, int wd, int c, int stride) {
    if (n <= 0 || h <= 0 || wd <= 0 || c <= 0 || c % 32 || (stride != 1 && stride != 2)) return 0;
    return align_up((size_t)l_gconv_bn_rows(n, h, wd, c) * 3 * c * sizeof(float));      // (h, wd: the input's side -- the larger grid)
}
int fte_gconv3x3_bn_fwd_bf16_s16(const uint16_t* x16, const uint16_t* wpk, uint16_t* z16, const float* gamma, const float* beta,
                                 float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var,
                                 float eps, float decay, const float* in_scale, const float* in_shift, uint16_t* y_side,
                                 int n, int h, int wd, int c, int stride, void* ws, size_t ws_bytes, void* stream) {
    if (!x16 || !wpk || !z16 || !gamma || !beta || !mean || !rstd || !scale || !shift || n <= 0 || h <= 0 || wd <= 0 || c <= 0 || c % 32 ||
        (stride != 1 && stride != 2) || (long)n * h * wd >= ((long)1 << 31) || ((moving_mean == nullptr) != (moving_var == nullptr)))
        return FTE_EINVAL;
    if (((in_scale == nullptr) != (in_shift == nullptr)) || (in_scale && (!y_side || stride != 1))) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_gconv3x3_bn_ws_bytes(n, h, wd, c, stride)) return FTE_EWORKSPACE;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    hipError_t e;
    int rows;
    if (stride == 1) {
        rows = l_gconv_bn_rows(n, h, wd, c);
        e = l_gconv_mfma16_bn(f32p(x16), wpk, f32p(z16), n, h, wd, c, h, wd, 0, 1, 1, 1, (float*)ws, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream,
                              in_scale, in_shift, y_side);
    } else {
        rows = l_gconv_bn_rows(n, ph.out, pw.out, c);
        e = l_gconv_mfma16_bn(f32p(x16), wpk, f32p(z16), n, ph.out, pw.out, c, h, wd, 1, ph.before, pw.before, 1, (float*)ws, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              (hipStream_t)stream);
    }
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_finalize((const float*)ws, rows, gamma, beta, c, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var, (hipStream_t)stream));
}
int fte_gconv3x3_dgrad_bn_bf16_s16(const uint16_t* dz16, const uint16_t* wpk_dgrad, const uint16_t* zbn16, const float* gamma, const float* mean,
                                   const float* rstd, const float* bn_scale, const float* bn_shift, uint16_t* g16, float* dgamma, float* dbeta,
                                   float* coef, int n, int h, int wd, int c, int stride, void* ws, size_t ws_bytes, void* stream) {
    if (!dz16 || !wpk_dgrad || !zbn16 || !gamma || !mean || !rstd || !g16 || !dgamma || !dbeta || !coef || n <= 0 || h <= 0 || wd <= 0 || c <= 0 ||
        c % 32 || (stride != 1 && stride != 2) || (long)n * h * wd >= ((long)1 << 31) || ((bn_scale == nullptr) != (bn_shift == nullptr)))
        return FTE_EINVAL;
    if (!ws || ws_bytes < fte_gconv3x3_bn_ws_bytes(n, h, wd, c, stride)) return FTE_EWORKSPACE;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int rows = l_gconv_bn_rows(n, h, wd, c);
    float* pg = (float*)ws;
    float* pgx = pg + (size_t)rows * c;
    hipError_t e;
    if (stride == 1)
        e = l_gconv_mfma16_bn(f32p(dz16), wpk_dgrad, f32p(g16), n, h, wd, c, h, wd, 0, 1, 1, 2, pg, pgx, zbn16, mean, rstd, bn_scale, bn_shift, (hipStream_t)stream);
    else
        e = l_gconv_mfma16_bn(f32p(dz16), wpk_dgrad, f32p(g16), n, h, wd, c, ph.out, pw.out, 2, ph.before, pw.before, 2, pg, pgx, zbn16, mean, rstd, bn_scale, bn_shift,
                              (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(l_bn_bwd_finalize(pg, pgx, c, rows, (long)n * h * wd, c, gamma, mean, rstd, dgamma, dbeta, coef, (hipStream_t)stream));
}

int fte_relu_bwd_s16(const uint16_t* dy16, const uint16_t* y16, uint16_t* g16, long n, void* stream) {
    if (!dy16 || !y16 || !g16 || n <= 0 || n % 4) return FTE_EINVAL;
    return rc(l_relu_bwd(f32p(dy16), f32p(y16), f32p(g16), n, (hipStream_t)stream, 2));
}
int fte_maxpool3x3s2_fwd_s16(const uint16_t* x16, uint16_t* y16, uint8_t* idx, int n, int h, int wd, int c, void* stream) {
    if (!x16 || !y16 || !idx || n <= 0 || c % 4) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, 2), pw = same_pads(wd, 3, 2);
    return rc(l_maxpool_fwd(f32p(x16), f32p(y16), idx, n, h, wd, c, ph.out, pw.out, ph.before, pw.before, (hipStream_t)stream, 2));
}
int fte_maxpool3x3s2_bwd_s16(const uint16_t* dy16, const uint8_t* idx, uint16_t* dx16, int n, int h, int wd, int c, void* stream) {
    if (!dy16 || !idx || !dx16 || n <= 0 || c % 4) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, 2), pw = same_pads(wd, 3, 2);
    return rc(l_maxpool_bwd(f32p(dy16), idx, f32p(dx16), n, h, wd, c, ph.out, pw.out, ph.before, pw.before, (hipStream_t)stream, 2));
}
int fte_gap_fwd_s16(const uint16_t* x16, float* y, int n, int hw, int c, void* stream) {
    if (!x16 || !y || n <= 0 || hw <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_gap_fwd(f32p(x16), y, n, hw, c, (hipStream_t)stream, 2));
}
int fte_gap_bwd_s16(const float* dy, uint16_t* dx16, int n, int hw, int c, void* stream) {
    if (!dy || !dx16 || n <= 0 || hw <= 0 || c <= 0) return FTE_EINVAL;
    return rc(l_gap_bwd(dy, f32p(dx16), n, hw, c, (hipStream_t)stream, 2));
}
int fte_dropout_fwd(const float* x, float* mask, float* y, long n, float keep_prob, uint64_t seed, void* stream) {
    if (!x || !mask || !y || n <= 0 || !(keep_prob > 0.f)) return FTE_EINVAL;
    return rc(l_dropout_fwd(x, mask, y, n, keep_prob, seed, (hipStream_t)stream));
}
int fte_dropout_bwd(const float* dy, const float* mask, float* dx, long n, float keep_prob, void* stream) {
    if (!dy || !mask || !dx || n <= 0 || !(keep_prob > 0.f)) return FTE_EINVAL;
    return rc(l_scale_mask(dy, mask, dx, n, 1.f / keep_prob, (hipStream_t)stream));
}
int fte_im2col_first(const float* x, float* cols, int n, int h, int wd, int cin, int ksize, int stride, int kpad, void* stream) {
    if (!x || !cols || n <= 0 || kpad % 32 || kpad < ksize * ksize * cin) return FTE_EINVAL;
    const Pads ph = same_pads(h, ksize, stride), pw = same_pads(wd, ksize, stride);
    return rc(l_im2col_first(x, cols, n, h, wd, cin, ksize, stride, ph.out, pw.out, ph.before, pw.before, kpad, (hipStream_t)stream));
}

int fte_im2col_first_s16(const float* x, uint16_t* cols16, int n, int h, int wd, int cin, int ksize, int stride, int kpad, void* stream) {
    if (!x || !cols16 || n <= 0 || kpad % 32 || kpad < ksize * ksize * cin) return FTE_EINVAL;
    const Pads ph = same_pads(h, ksize, stride), pw = same_pads(wd, ksize, stride);
    return rc(l_im2col_first(x, f32p(cols16), n, h, wd, cin, ksize, stride, ph.out, pw.out, ph.before, pw.before, kpad, (hipStream_t)stream, 1));
}

// the refusals the four transform entries share; min_stride: the header a slot must at least hold (64, aligned slots 128)
static bool preprocess_args_ok(const uint8_t* slots, const float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h,
                               int crop_w, long min_stride) {
    return slots && out && n > 0 && (channels == 1 || channels == 3) && in_h > 0 && in_w > 0 && crop_h > 0 && crop_w > 0 &&
           crop_h <= in_h && crop_w <= in_w && slot_stride >= min_stride && slot_stride % 64 == 0 && n <= 65535;
}

int fte_preprocess_u8(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h, int crop_w,
                      void* stream) {
    if (!preprocess_args_ok(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, 64)) return FTE_EINVAL;
    return rc(k_preprocess_u8(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, (hipStream_t)stream));
}

int fte_preprocess_u8_aug(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h, int crop_w,
                          void* stream) {
    if (!preprocess_args_ok(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, 64)) return FTE_EINVAL;
    return rc(k_preprocess_u8_aug(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, (hipStream_t)stream));
}

size_t fte_preprocess_u8_geo_ws_bytes(int n, int channels, int crop_h, int crop_w) {
    if (n <= 0 || (channels != 1 && channels != 3) || crop_h <= 0 || crop_w <= 0) return 0;
    return k_preprocess_u8_geo_ws_bytes(n, channels, crop_h, crop_w);
}

int fte_preprocess_u8_geo(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h, int crop_w,
                          const float* affine_table, void* ws, size_t ws_bytes, void* stream) {
    if (!preprocess_args_ok(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, 64) || !affine_table ||
        (long)crop_h * crop_w * channels >= ((long)1 << 28)) return FTE_EINVAL;       // plane offsets are ints
    const size_t need = k_preprocess_u8_geo_ws_bytes(n, channels, crop_h, crop_w);
    if (need && (!ws || ws_bytes < need)) return FTE_EWORKSPACE;
    return rc(k_preprocess_u8_geo(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, affine_table, ws, (hipStream_t)stream));
}

int fte_preprocess_u8_align(const uint8_t* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w, int crop_h, int crop_w,
                            void* stream) {
    if (!preprocess_args_ok(slots, out, n, slot_stride, channels, in_h, in_w, crop_h, crop_w, 128)) return FTE_EINVAL;
    return rc(k_preprocess_u8_align(slots, out, n, slot_stride, channels, crop_h, crop_w, (hipStream_t)stream));
}

int fte_pack_gather_slots(const uint8_t* rows, long num_rows, long row_stride, const int64_t* index, const uint8_t* headers, uint8_t* slots,
                          int n, long slot_stride, void* stream) {
    if (!rows || !index || !headers || !slots || n < 1 || num_rows < 1 || row_stride < 64 || row_stride % 64 || slot_stride % 64 ||
        slot_stride < 64 + row_stride || ((uintptr_t)rows | (uintptr_t)headers | (uintptr_t)slots) % 16 || (uintptr_t)index % 8) return FTE_EINVAL;
    return rc(k_pack_gather_slots(rows, num_rows, row_stride, index, headers, slots, n, slot_stride, igemm_num_cus(), (hipStream_t)stream));
}

// ------------------------------------------------------------------------------------------------
// grouped 3x3 conv, SE-gate pieces
// fte.h: c / groups in {4, 8, 16, 32}; any other width is refused here, before a launcher sees it
static inline bool gconv_width_ok(int gw) { return gw == 4 || gw == 8 || gw == 16 || gw == 32; }
int fte_gconv3x3_fwd(const float* x, const float* w, float* y, int n, int h, int wd, int c, int groups, int stride, void* stream) {
    if (!x || !w || !y || n <= 0 || groups <= 0 || c % groups || (stride != 1 && stride != 2) || !gconv_width_ok(c / groups)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_gconv_fwd(x, w, y, n, h, wd, c, groups, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}
int fte_gconv3x3_pack_bf16(const float* w, uint16_t* wpk_fwd, uint16_t* wpk_dgrad, int c, int groups, void* stream) {
    if (!w || !wpk_fwd || !wpk_dgrad || groups <= 0 || c % groups || c % 32) return FTE_EINVAL;
    const int gw = c / groups;
    if (gw != 4 && gw != 8 && gw != 16 && gw != 32) return FTE_EINVAL;
    return rc(l_gconv_pack16(w, wpk_fwd, wpk_dgrad, c, groups, (hipStream_t)stream));
}
int fte_gconv3x3_bf16(const float* x, const uint16_t* wpk, float* y, int n, int h, int wd, int c, int stride, int dgrad, void* stream) {
    if (!x || !wpk || !y || n <= 0 || h <= 0 || wd <= 0 || c <= 0 || c % 32 || (stride != 1 && stride != 2) ||
        (long)n * h * wd >= ((long)1 << 31)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    if (stride == 1) return rc(l_gconv_mfma16(x, wpk, y, n, h, wd, c, h, wd, 0, 1, 1, (hipStream_t)stream));
    if (!dgrad) return rc(l_gconv_mfma16(x, wpk, y, n, ph.out, pw.out, c, h, wd, 1, ph.before, pw.before, (hipStream_t)stream));
    return rc(l_gconv_mfma16(x, wpk, y, n, h, wd, c, ph.out, pw.out, 2, ph.before, pw.before, (hipStream_t)stream));
}
int fte_gconv3x3_bf16_s16(const uint16_t* x16, const uint16_t* wpk, uint16_t* y16, int n, int h, int wd, int c, int stride, int dgrad, void* stream) {
    if (!x16 || !wpk || !y16 || n <= 0 || h <= 0 || wd <= 0 || c <= 0 || c % 32 || (stride != 1 && stride != 2) ||
        (long)n * h * wd >= ((long)1 << 31)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const float* x = f32p(x16);
    float* y = f32p(y16);
    if (stride == 1) return rc(l_gconv_mfma16(x, wpk, y, n, h, wd, c, h, wd, 0, 1, 1, (hipStream_t)stream, 1));
    if (!dgrad) return rc(l_gconv_mfma16(x, wpk, y, n, ph.out, pw.out, c, h, wd, 1, ph.before, pw.before, (hipStream_t)stream, 1));
    return rc(l_gconv_mfma16(x, wpk, y, n, h, wd, c, ph.out, pw.out, 2, ph.before, pw.before, (hipStream_t)stream, 1));
}
size_t fte_gconv3x3_wgrad_bf16_ws_bytes(int n, int h, int wd, int c, int groups, int stride) {
    if (n <= 0 || h <= 0 || wd <= 0 || c <= 0 || groups <= 0 || c % groups || c % 32 || (stride != 1 && stride != 2)) return 0;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return align_up((size_t)l_gconv_wgrad16_chunks((long)n * ph.out * pw.out, c) * c * 9 * (c / groups) * sizeof(float));
}
int fte_gconv3x3_wgrad_bf16(const float* x, const float* dz, float* dw, int n, int h, int wd, int c, int groups, int stride,
                            void* ws, size_t ws_bytes, void* stream) {
    if (!x || !dz || !dw || n <= 0 || h <= 0 || wd <= 0 || groups <= 0 || c % groups || c % 32 || (stride != 1 && stride != 2) ||
        (long)n * h * wd >= ((long)1 << 31)) return FTE_EINVAL;
    const int gw = c / groups;
    if (gw != 4 && gw != 8 && gw != 16 && gw != 32) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_gconv3x3_wgrad_bf16_ws_bytes(n, h, wd, c, groups, stride)) return FTE_EWORKSPACE;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_gconv_wgrad16(x, dz, (float*)ws, dw, n, h, wd, c, groups, ph.out, pw.out, stride, ph.before, pw.before,
                              l_gconv_wgrad16_chunks((long)n * ph.out * pw.out, c), (hipStream_t)stream));
}
int fte_gconv3x3_wgrad_bf16_s16(const uint16_t* x16, const uint16_t* dz16, float* dw, int n, int h, int wd, int c, int groups, int stride,
                                void* ws, size_t ws_bytes, void* stream) {
    if (!x16 || !dz16 || !dw || n <= 0 || h <= 0 || wd <= 0 || groups <= 0 || c % groups || c % 32 || (stride != 1 && stride != 2) ||
        (long)n * h * wd >= ((long)1 << 31)) return FTE_EINVAL;
    const int gw = c / groups;
    if (gw != 4 && gw != 8 && gw != 16 && gw != 32) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_gconv3x3_wgrad_bf16_ws_bytes(n, h, wd, c, groups, stride)) return FTE_EWORKSPACE;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_gconv_wgrad16(f32p(x16), f32p(dz16), (float*)ws, dw, n, h, wd, c, groups, ph.out, pw.out, stride, ph.before, pw.before,
                              l_gconv_wgrad16_chunks((long)n * ph.out * pw.out, c), (hipStream_t)stream, 1));
}
int fte_gconv3x3_dgrad(const float* dz, const float* w, float* dx, int n, int h, int wd, int c, int groups, int stride, void* stream) {
    if (!dz || !w || !dx || n <= 0 || groups <= 0 || c % groups || (stride != 1 && stride != 2) || !gconv_width_ok(c / groups)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_gconv_dgrad(dz, w, dx, n, h, wd, c, groups, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}
size_t fte_gconv3x3_wgrad_ws_bytes(int n, int h, int wd, int c, int groups, int stride) {
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int gw = c / groups;
    return align_up((size_t)l_gconv_wgrad_chunks((long)n * ph.out * pw.out, c, gw) * 9 * c * gw * sizeof(float)) + SCRATCH_BYTES;
}
int fte_gconv3x3_wgrad(const float* x, const float* dz, float* dw, int n, int h, int wd, int c, int groups, int stride,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!x || !dz || !dw || n <= 0 || groups <= 0 || c % groups || (stride != 1 && stride != 2) || !gconv_width_ok(c / groups)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int gw = c / groups;
    const int chunks = l_gconv_wgrad_chunks((long)n * ph.out * pw.out, c, gw);
    const size_t need = align_up((size_t)chunks * 9 * c * gw * sizeof(float));
    if (!ws || ws_bytes < need + SCRATCH_BYTES) return FTE_EWORKSPACE;
    hipError_t e = l_gconv_wgrad(x, dz, (float*)ws, n, h, wd, c, groups, ph.out, pw.out, stride, ph.before, pw.before, chunks, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, chunks, 9L * c * gw, 1, 1.f, (float*)((char*)ws + need), (hipStream_t)stream));
}
int fte_bcast_add(float* dx, const float* v, int n, int hw, int c, float scale, void* stream) {
    if (!dx || !v || n <= 0 || hw <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_bcast_add(dx, v, n, hw, c, scale, (hipStream_t)stream));
}
int fte_act_fwd(const float* x, float* y, long n, int kind, void* stream) {
    if (!x || !y || n <= 0 || (kind != 0 && kind != 1)) return FTE_EINVAL;
    return rc(l_act_fwd(x, y, n, kind, (hipStream_t)stream));
}
int fte_act_bwd(const float* dy, const float* y, float* dx, long n, int kind, void* stream) {
    if (!dy || !y || !dx || n <= 0 || (kind != 0 && kind != 1)) return FTE_EINVAL;
    return rc(l_act_bwd(dy, y, dx, n, kind, (hipStream_t)stream));
}
int fte_channel_scale_fwd(const float* x, const float* gate, float* y, int n, int hw, int c, void* stream) {
    if (!x || !gate || !y || n <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_chscale_fwd(x, gate, y, n, hw, c, (hipStream_t)stream));
}
int fte_channel_scale_bwd(const float* dy, const float* x, const float* gate, float* dx, float* dgate, int n, int hw, int c,
                          int pre_sigmoid, void* stream) {
    if (!dy || !x || !gate || !dx || !dgate || n <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_chscale_bwd(dy, x, gate, dx, dgate, n, hw, c, pre_sigmoid ? 1 : 0, (hipStream_t)stream));
}

// SE gate on bf16 tensors (fte.h, bf16 STORAGE): scale, the gate-gradient reduction (no dx), and the one-pass input gradient
int fte_channel_scale_fwd_s16(const uint16_t* x16, const float* gate, uint16_t* y16, int n, int hw, int c, void* stream) {
    if (!x16 || !gate || !y16 || n <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_chscale_fwd(f32p(x16), gate, f32p(y16), n, hw, c, (hipStream_t)stream, 1));
}
int fte_channel_scale_bwd_s16(const uint16_t* dy16, const uint16_t* x16, const float* gate, float* dgate, int n, int hw, int c,
                              int pre_sigmoid, void* stream) {
    if (!dy16 || !x16 || !gate || !dgate || n <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_chscale_bwd(f32p(dy16), f32p(x16), gate, nullptr, dgate, n, hw, c, pre_sigmoid ? 1 : 0, (hipStream_t)stream, 1));
}
int fte_channel_scale_bwd_apply_s16(const uint16_t* dy16, const float* gate, const float* dsq, uint16_t* dx16, int n, int hw, int c,
                                    float scale, void* stream) {
    if (!dy16 || !gate || !dsq || !dx16 || n <= 0 || c <= 0 || c % 4) return FTE_EINVAL;
    return rc(l_chscale_bwd_apply(f32p(dy16), gate, dsq, f32p(dx16), n, hw, c, scale, (hipStream_t)stream, 1));
}

// the SE residual block, fused (layers.hip "SE residual block")
static bool se_args_ok(int n, int hw, int c, int flags) { return n > 0 && hw > 0 && c > 0 && c % 4 == 0 && !(flags & ~3) && (!flags || c >= 32); }
int fte_se_squeeze(const void* z, const float* scale, const float* shift, const float* mean, const float* rstd, float* sq, float* xm,
                   int n, int hw, int c, int flags, void* stream) {
    if (!z || !scale || !shift || !sq || (xm && (!mean || !rstd)) || !se_args_ok(n, hw, c, flags)) return FTE_EINVAL;
    return rc(l_se_squeeze(f32p(z), scale, shift, mean, rstd, sq, xm, n, hw, c, (hipStream_t)stream, flags));
}
int fte_se_apply_fwd(const void* z, const float* scale, const float* shift, const float* gate, const void* shortcut, void* out,
                     int n, int hw, int c, int flags, void* stream) {
    if (!z || !scale || !shift || !gate || !shortcut || !out || !se_args_ok(n, hw, c, flags)) return FTE_EINVAL;
    return rc(l_se_apply(f32p(z), scale, shift, gate, f32p(shortcut), f32p(out), n, hw, c, (hipStream_t)stream, flags));
}
int fte_se_bwd_gate(const void* dy, const void* out, const void* z, const float* gamma, const float* beta, const float* mean,
                    const float* rstd, const float* gate, void* g, float* s1, float* s2, float* dgate, int n, int hw, int c, int flags, void* stream) {
    if (!dy || !out || !z || !gamma || !beta || !mean || !rstd || !gate || !g || !s1 || !s2 || !dgate || !se_args_ok(n, hw, c, flags)) return FTE_EINVAL;
    return rc(l_se_bwd_gate(f32p(dy), f32p(out), f32p(z), gamma, beta, mean, rstd, gate, f32p(g), s1, s2, dgate, n, hw, c, (hipStream_t)stream, flags));
}
int fte_se_bn_bwd_coef(const float* s1, const float* s2, const float* gate, const float* dsq, const float* xm, const float* gamma,
                       const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef, int n, int hw, int c, void* stream) {
    if (!s1 || !s2 || !gate || !dsq || !xm || !gamma || !mean || !rstd || !dgamma || !dbeta || !coef || !se_args_ok(n, hw, c, 0)) return FTE_EINVAL;
    return rc(l_se_bn_coef(s1, s2, gate, dsq, xm, gamma, mean, rstd, dgamma, dbeta, coef, n, hw, c, (hipStream_t)stream));
}
int fte_se_bn_bwd_apply(const void* g, const void* z, const float* coef, const float* gate, const float* dsq, void* dz,
                        int n, int hw, int c, int flags, void* stream) {
    if (!g || !z || !coef || !gate || !dsq || !dz || !se_args_ok(n, hw, c, flags)) return FTE_EINVAL;
    return rc(l_se_bn_apply(f32p(g), f32p(z), coef, gate, dsq, f32p(dz), n, hw, c, (hipStream_t)stream, flags));
}

// ------------------------------------------------------------------------------------------------
// ShuffleNet-v2: depthwise 3x3, channel gather
int fte_dwconv3x3_fwd(const float* x, const float* w, float* y, int n, int h, int wd, int c, int stride, void* stream) {
    if (!x || !w || !y || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_dwconv_fwd(x, w, y, n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}
int fte_dwconv3x3_dgrad(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int stride, void* stream) {
    if (!dy || !w || !dx || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_dwconv_dgrad(dy, w, dx, n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream));
}
size_t fte_dwconv3x3_wgrad_ws_bytes(int n, int h, int wd, int c, int stride) {
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return align_up((size_t)l_dwconv_wgrad_splits((long)n * ph.out * pw.out, c) * 9 * c * sizeof(float)) + SCRATCH_BYTES;
}
int fte_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int n, int h, int wd, int c, int stride,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!x || !dy || !dw || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int splits = l_dwconv_wgrad_splits((long)n * ph.out * pw.out, c);
    const size_t need = align_up((size_t)splits * 9 * c * sizeof(float));
    if (!ws || ws_bytes < need + SCRATCH_BYTES) return FTE_EWORKSPACE;
    hipError_t e = l_dwconv_wgrad(x, dy, (float*)ws, n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, splits, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, splits, 9L * c, 1, 1.f, (float*)((char*)ws + need), (hipStream_t)stream));
}
int fte_channel_gather(const float* a, const float* b, float* out, const int32_t* table, long rows, int ca, int cb, int co, void* stream) {
    if (!a || !out || !table || rows <= 0 || co <= 0 || co % 4) return FTE_EINVAL;      // the table is read 4 entries at a time
    return rc(l_channel_gather(a, b ? b : a, out, table, rows, ca, cb, co, (hipStream_t)stream));
}
int fte_channel_gather_affine(const float* a, const float* b, float* out, const int32_t* table, int co,
                              float* out1, const int32_t* table1, int co1, long rows, int ca, int cb,
                              const float* scale_a, const float* shift_a, int relu_a,
                              const float* scale_b, const float* shift_b, int relu_b, void* stream) {
    if (!a || !out || !table || rows <= 0 || co <= 0 || co % 4 || (scale_a && !shift_a) || (scale_b && (!shift_b || !b))) return FTE_EINVAL;
    if (out1 ? (!table1 || co1 <= 0 || co1 % 4) : co1 != 0) return FTE_EINVAL;
    return rc(l_channel_gather_affine(a, b ? b : a, out, table, co, out1, table1, co1, rows, ca, cb, scale_a, shift_a, relu_a,
                                      scale_b, shift_b, relu_b, (hipStream_t)stream));
}

// ---- bf16 STORAGE twins of ShuffleNet-v2's layers: every activation-side tensor bf16, filters / tables / per-channel vectors unchanged
int fte_dwconv3x3_fwd_s16(const uint16_t* x16, const float* w, uint16_t* y16, int n, int h, int wd, int c, int stride, void* stream) {
    if (!x16 || !w || !y16 || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_dwconv_fwd(f32p(x16), w, f32p(y16), n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream, 1));
}
int fte_dwconv3x3_dgrad_s16(const uint16_t* dy16, const float* w, uint16_t* dx16, int n, int h, int wd, int c, int stride, void* stream) {
    if (!dy16 || !w || !dx16 || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    return rc(l_dwconv_dgrad(f32p(dy16), w, f32p(dx16), n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, (hipStream_t)stream, 1));
}
int fte_dwconv3x3_wgrad_s16(const uint16_t* x16, const uint16_t* dy16, float* dw, int n, int h, int wd, int c, int stride,
                            void* ws, size_t ws_bytes, void* stream) {
    if (!x16 || !dy16 || !dw || n <= 0 || c % 4 || (stride != 1 && stride != 2)) return FTE_EINVAL;
    const Pads ph = same_pads(h, 3, stride), pw = same_pads(wd, 3, stride);
    const int splits = l_dwconv_wgrad_splits((long)n * ph.out * pw.out, c);
    const size_t need = align_up((size_t)splits * 9 * c * sizeof(float));
    if (!ws || ws_bytes < need + SCRATCH_BYTES) return FTE_EWORKSPACE;
    hipError_t e = l_dwconv_wgrad(f32p(x16), f32p(dy16), (float*)ws, n, h, wd, c, ph.out, pw.out, stride, ph.before, pw.before, splits, (hipStream_t)stream, 1);
    if (e != hipSuccess) return (int)e;
    return rc(k_reduce_rows((const float*)ws, dw, nullptr, 1, splits, 9L * c, 1, 1.f, (float*)((char*)ws + need), (hipStream_t)stream));
}
int fte_channel_gather_s16(const uint16_t* a, const uint16_t* b, uint16_t* out, const int32_t* table, long rows, int ca, int cb, int co, void* stream) {
    if (!a || !out || !table || rows <= 0 || co <= 0 || co % 4) return FTE_EINVAL;
    return rc(l_channel_gather(f32p(a), f32p(b ? b : a), f32p(out), table, rows, ca, cb, co, (hipStream_t)stream, 1));
}
int fte_channel_gather_affine_s16(const uint16_t* a, const uint16_t* b, uint16_t* out, const int32_t* table, int co,
                                  uint16_t* out1, const int32_t* table1, int co1, long rows, int ca, int cb,
                                  const float* scale_a, const float* shift_a, int relu_a,
                                  const float* scale_b, const float* shift_b, int relu_b, void* stream) {
    if (!a || !out || !table || rows <= 0 || co <= 0 || co % 4 || (scale_a && !shift_a) || (scale_b && (!shift_b || !b))) return FTE_EINVAL;
    if (out1 ? (!table1 || co1 <= 0 || co1 % 4) : co1 != 0) return FTE_EINVAL;
    return rc(l_channel_gather_affine(f32p(a), f32p(b ? b : a), f32p(out), table, co, f32p(out1), table1, co1, rows, ca, cb, scale_a, shift_a, relu_a,
                                      scale_b, shift_b, relu_b, (hipStream_t)stream, 1));
}
int fte_bn_train_stats_s16(const void* z, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift,
                           float* moving_mean, float* moving_var, long rows, int c, float eps, float decay, int flags,
                           void* ws, size_t ws_bytes, void* stream) {
    if (!z || !gamma || !beta || !mean || !rstd || !scale || !shift || rows <= 0 || c % 4 || c < 32 || (flags & ~3)) return FTE_EINVAL;
    if (!ws || ws_bytes < fte_bn_ws_bytes(c)) return FTE_EWORKSPACE;
    return rc(l_bn_train_stats(f32p(z), gamma, beta, rows, c, eps, decay, mean, rstd, scale, shift, moving_mean, moving_var,
                               (float*)ws, (hipStream_t)stream, flags));
}

// ---------------------------------------------------------------- evaluation (search.hip)
static inline bool below_2g(long rows, long cols, long elem = 4) { return rows * cols * elem < (1L << 31); }
int fte_l2_normalize_rows(const float* x, float* y, float* norms, int n, int d, void* stream) {
    if (!x || !y || n < 1 || d < 1 || !below_2g(n, d)) return FTE_EINVAL;
    return rc(s_normalize_rows(x, y, norms, n, d, (hipStream_t)stream));
}
int fte_pair_scores(const float* x, const int32_t* ia, const int32_t* ib, float* out, int n, int d, int npairs, void* stream) {
    if (!x || !ia || !ib || !out || n < 1 || d < 1 || npairs < 1 || !below_2g(n, d)) return FTE_EINVAL;
    return rc(s_pair_scores(x, ia, ib, out, n, d, npairs, (hipStream_t)stream));
}
size_t fte_topk_search_ws_bytes(int m, int n, int d, int k) {
    (void)d;
    if (m < 1 || n < 1 || k < 1 || k > 64) return 0;
    return s_topk_ws_bytes(m, n, k);
}
int fte_topk_search(const float* probes, const float* gallery, int m, int n, int d, int k, int gallery_base, int exclude_self,
                    int probe_base, float* scores, int32_t* index, void* ws, size_t ws_bytes, void* stream) {
    if (!probes || !gallery || !scores || !index || m < 1 || n < 1 || d < 32 || d % 32 || k < 1 || k > 64 || k > n || gallery_base < 0 ||
        probe_base < 0 || !below_2g(m, d) || !below_2g(n, d) || !below_2g(m, k) || (long)gallery_base + n > 0x7fffffffL)
        return FTE_EINVAL;
    if (!ws || ws_bytes < s_topk_ws_bytes(m, n, k)) return FTE_EWORKSPACE;
    return rc(s_topk_search(probes, gallery, m, n, d, k, gallery_base, exclude_self != 0, probe_base, scores, index, ws, (hipStream_t)stream));
}
int fte_topk_merge(const float* in_scores, const int32_t* in_index, int m, int lists, int k, float* scores, int32_t* index, void* stream) {
    if (!in_scores || !in_index || !scores || !index || m < 1 || lists < 1 || lists > 64 || k < 1 || k > 64 || !below_2g((long)m * lists, k))
        return FTE_EINVAL;
    return rc(s_topk_merge(in_scores, in_index, m, lists, k, scores, index, (hipStream_t)stream));
}
int fte_score_histograms(const float* a, const int32_t* la, int na, const float* b, const int32_t* lb, int nb, int d, int same,
                         int nbins, uint64_t* hist_genuine, uint64_t* hist_impostor, void* stream) {
    if (!a || !la || !b || !lb || !hist_genuine || !hist_impostor || na < 1 || nb < 1 || d < 32 || d % 32 || nbins < 256 || nbins > 8192 ||
        (nbins & (nbins - 1)) || (same && na != nb) || !below_2g(na, d) || !below_2g(nb, d))
        return FTE_EINVAL;
    return rc(s_score_histograms(a, la, na, b, lb, nb, d, same != 0, nbins, (unsigned long long*)hist_genuine,
                                 (unsigned long long*)hist_impostor, (hipStream_t)stream));
}

int fte_template_pool(const float* x, const float* w, int n, int d, const int32_t* members, int n_members, const int32_t* media_off,
                      int n_media, const int32_t* tmpl_off, int n_templates, float* out, void* stream) {
    if (!x || !members || !media_off || !tmpl_off || !out || n < 1 || d < 1 || n_members < 1 || n_media < 1 || n_templates < 1 ||
        !below_2g(n, d) || !below_2g(n_templates, d) || !below_2g(n_members, 1) || !below_2g(n_media + 1L, 1) || !below_2g(n_templates + 1L, 1))
        return FTE_EINVAL;
    return rc(s_template_pool(x, w, n, d, members, n_members, media_off, n_media, tmpl_off, n_templates, out, (hipStream_t)stream));
}
int fte_set_pair_scores(const float* x, int n, int d, const int32_t* members, int n_members, const int32_t* media_off, int n_media,
                        const int32_t* tmpl_off, int n_templates, const int32_t* ta, const int32_t* tb, int npairs, const float* betas,
                        int nbetas, float* out, void* stream) {
    if (!x || !members || !media_off || !tmpl_off || !ta || !tb || !betas || !out || n < 1 || d < 32 || d % 32 || n_members < 1 ||
        n_media < 1 || n_templates < 1 || npairs < 1 || nbetas < 1 || nbetas > 32 || !below_2g(n, d) ||
        !below_2g(n_members, 1) || !below_2g(n_media + 1L, 1) || !below_2g(n_templates + 1L, 1) || !below_2g(npairs, 1))
        return FTE_EINVAL;
    for (int k = 0; k < nbetas; ++k)
        if (!(betas[k] >= 0.f && betas[k] <= 40.f)) return FTE_EINVAL;          // NaN fails too
    return rc(s_set_pair_scores(x, n, d, members, n_members, media_off, n_media, tmpl_off, n_templates, ta, tb, npairs, betas, nbetas, out,
                                (hipStream_t)stream));
}

int fte_megaface_pair_scores(const float* probes, int m, const float* rows, int n, int d, const int32_t* ip, const int32_t* ig, int npairs,
                             float* out, void* stream) {
    if (!probes || !rows || !ip || !ig || !out || m < 1 || n < 1 || d < 32 || d % 32 || npairs < 1 || !below_2g(m, d) || !below_2g(n, d) ||
        !below_2g(npairs, 1))
        return FTE_EINVAL;
    return rc(s_mf_pair_scores(probes, m, rows, n, d, ip, ig, npairs, out, (hipStream_t)stream));
}
size_t fte_megaface_scan_ws_bytes(int m, int nthr) {
    if (m < 1 || nthr < 1) return 0;
    return s_mf_scan_ws_bytes(nthr);
}
int fte_megaface_scan(const float* probes, int m, const float* rows, int n, int d, const int32_t* thr_off, const float* thr, int nthr,
                      int nbins, uint64_t* counts, uint64_t* hist, void* ws, size_t ws_bytes, void* stream) {
    if (!probes || !rows || !thr_off || !thr || !counts || !hist || m < 1 || n < 1 || d < 32 || d % 32 || nthr < 1 || nbins < 256 ||
        nbins > 8192 || (nbins & (nbins - 1)) || !below_2g(m, d) || !below_2g(n, d) || !below_2g(m + 1L, 1) || !below_2g(nthr, 2))
        return FTE_EINVAL;
    if (!ws || ws_bytes < s_mf_scan_ws_bytes(nthr)) return FTE_EWORKSPACE;
    return rc(s_mf_scan(probes, m, rows, n, d, thr_off, thr, nthr, nbins, (unsigned long long*)counts, (unsigned long long*)hist, ws,
                        (hipStream_t)stream));
}

// ---- Partial FC (partial_fc.hip) ----
size_t fte_pfc_sample_ws_bytes(int C) { return C < 1 ? 0 : p_sample_ws_bytes(C); }
int fte_pfc_sample(const int32_t* labels, int n, int C, int S, uint32_t seed, uint32_t step, int32_t* index, int32_t* inverse,
                   int32_t* labels_out, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !index || !inverse || !labels_out || n < 1 || C < 1 || S < n || S > C ||
        (((uintptr_t)index | (uintptr_t)inverse | (uintptr_t)labels_out) & 15))
        return FTE_EINVAL;
    if (!ws || ws_bytes < p_sample_ws_bytes(C)) return FTE_EWORKSPACE;
    if ((uintptr_t)ws & 15) return FTE_EINVAL;
    return rc(p_sample(labels, n, C, S, seed, step, index, inverse, labels_out, ws, (hipStream_t)stream));
}
int fte_pfc_gather_cols(const float* W, const int32_t* index, float* Ws, int D, int C, int cpad, int S, int Spad, void* stream) {
    if (!W || !index || !Ws || D < 1 || C < 1 || cpad < C || S < 1 || Spad < S || Spad % 4 || (((uintptr_t)index | (uintptr_t)Ws) & 15))
        return FTE_EINVAL;
    return rc(p_gather_cols(W, index, Ws, D, C, cpad, S, Spad, (hipStream_t)stream));
}
int fte_pfc_scatter_cols(const float* dWs, const int32_t* inverse, float* dW, int D, int C, int cpad, int S, int Spad, void* stream) {
    if (!dWs || !inverse || !dW || D < 1 || C < 1 || cpad < C || cpad % 4 || S < 1 || Spad < S || ((uintptr_t)dW & 15)) return FTE_EINVAL;
    return rc(p_scatter_cols(dWs, inverse, dW, D, C, cpad, S, Spad, (hipStream_t)stream));
}
int fte_pfc_momentum_update_cols(float* W, float* acc, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S, int Spad,
                                 float lr, float mom, float wd, float gscale, void* stream) {
    if (!W || !acc || !dWs || !inverse || D < 1 || C < 1 || cpad < C || cpad % 4 || S < 1 || Spad < S ||
        (((uintptr_t)W | (uintptr_t)acc | (uintptr_t)inverse) & 15))
        return FTE_EINVAL;
    return rc(p_momentum_update_cols(W, acc, dWs, inverse, D, C, cpad, S, Spad, lr, mom, wd, gscale, (hipStream_t)stream));
}
int fte_pfc_adam_update_cols(float* W, float* m, float* v, const float* dWs, const int32_t* inverse, int D, int C, int cpad, int S,
                             int Spad, float lr, float b1, float b2, float eps, float wd, float gscale, int t, void* stream) {
    if (!W || !m || !v || !dWs || !inverse || D < 1 || C < 1 || cpad < C || cpad % 4 || S < 1 || Spad < S || t < 1 ||
        (((uintptr_t)W | (uintptr_t)m | (uintptr_t)v | (uintptr_t)inverse) & 15))
        return FTE_EINVAL;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t));      // fte_adam_update's
    return rc(p_adam_update_cols(W, m, v, dWs, inverse, D, C, cpad, S, Spad, (float)lr_t, b1, b2, eps, wd, gscale, (hipStream_t)stream));
}

// ---- Clustering (cluster.hip) ----
static inline bool knn_lists_ok(int n, int k) { return n >= 1 && k >= 1 && k <= 64 && (long)n * k < (1L << 29); }
int fte_knn_links_threshold(const float* scores, const int32_t* index, int n, int k, float min_score, int mutual, uint8_t* keep,
                            void* stream) {
    if (!scores || !index || !keep || !knn_lists_ok(n, k)) return FTE_EINVAL;
    return rc(c_links_threshold(scores, index, n, k, min_score, mutual != 0, keep, (hipStream_t)stream));
}
int fte_knn_links_rank_order(const float* scores, const int32_t* index, int n, int k, float theta, float min_score, uint8_t* keep,
                             void* stream) {
    if (!scores || !index || !keep || !knn_lists_ok(n, k) || !(theta > 0.f && theta <= 3.402823466e38f))
        return FTE_EINVAL;                                   // (a NaN or infinite theta fails the comparison too)
    return rc(c_links_rank_order(scores, index, n, k, theta, min_score, keep, (hipStream_t)stream));
}
int fte_components(const int32_t* index, const uint8_t* keep, int n, int k, int32_t* parent, int32_t* label, void* stream) {
    if (!index || !keep || !parent || !label || !knn_lists_ok(n, k)) return FTE_EINVAL;
    return rc(c_components(index, keep, n, k, parent, label, (hipStream_t)stream));
}
}  // extern "C"
