// conv_plan.h -- the launch planner of the conv / dense entry points (api.hip): tile and split-K / stream-K selection, the parity classes
// of the data gradient, the Winograd rule, and the workspace layout of every op.  HOST-ONLY and pure: plain C++17, no HIP header, no
// pointer, no stream -- it compiles with g++ alone and tests/test_conv_plan_host.py runs it on a machine without a GPU.
// Everything a plan depends on is an argument:
//   PlanKnobs   the FTE_* tuning switches, read from the environment ONCE (plan_knobs_from_env; api.hip keeps the one copy)
//   PlanDevice  what the planner asks of the device: CU count, resident stream-K blocks per CU of every (tile, epilogue)
//   PlanCtx     operand / storage mode of THIS call: bf16 operands, bf16 storage only, BN fusion, the conv algorithm switch
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

// ---- ids shared with the kernel launchers (igemm.h, kernels.h, wino.h include this header) ------------------------------------------
enum { EPI_FWD = 0, EPI_DGRAD = 1 };
enum { TILE_128x128 = 0, TILE_256x64 = 1, TILE_128x64 = 2, TILE_64x64 = 3, TILE_192x64 = 4,      // 192x64: M = 576 = 9 taps x 64 channels in three whole tiles
       TILE_64x64_W1 = 5, TILE_64x64_W2 = 6 };  // 64x64 tile computed by ONE wave (64 threads, no barrier) / by two waves (128 threads)
// the fix-up splits every tile into this many row chunks (one block each); a dgrad fix-up therefore writes
// FIXUP_CHUNKS partial rows (PA/PB) per tile row, numbered prow0 + mt*FIXUP_CHUNKS + chunk
constexpr int FIXUP_CHUNKS = 4;
constexpr long REDUCE_SCRATCH_FLOATS = 1 << 18;      // 1 MiB of scratch for the tall-and-narrow case of k_reduce_rows

inline void igemm_tile_dims(int tile, int* bm, int* bn) {
    switch (tile) {
        case TILE_128x128: *bm = 128; *bn = 128; break;
        case TILE_256x64:  *bm = 256; *bn = 64; break;
        case TILE_128x64:  *bm = 128; *bn = 64; break;
        case TILE_192x64:  *bm = 192; *bn = 64; break;
        default:           *bm = 64;  *bn = 64; break;
    }
}
// workspace (slabs + flag words) a stream-K launch of `workers` blocks needs
inline size_t igemm_sk_ws_bytes(int tile, int workers) {
    int bm, bn;
    igemm_tile_dims(tile, &bm, &bn);
    return (size_t)workers * bm * bn * sizeof(float) + (((size_t)workers * 4 + 255) & ~(size_t)255);
}

// Geometry of one stride-1 SAME 3x3 layer over [n, h, w, c]: 2x2 output tiles, TH x TW of them per image (odd sizes: the last
// tile row / column is half outside the image), M tiles in all, MB = row blocks of 64 tiles.
struct WinoGeom {
    int n, h, w, th, tw;
    long M;
    int MB;
};
inline WinoGeom wino_geom(int n, int h, int w) {
    WinoGeom g;
    g.n = n; g.h = h; g.w = w; g.th = (h + 1) / 2; g.tw = (w + 1) / 2;
    g.M = (long)n * g.th * g.tw;
    g.MB = (int)((g.M + 63) / 64);
    return g;
}
// floats of a "pack" (wino.h) of R rows and C channels
inline size_t wino_pack_floats(long rows, int c) { return (size_t)((rows + 63) / 64) * 64 * (size_t)c * 16; }
// slabs of the Winograd filter gradient (0: shape not supported)
inline int wino_wgrad_splits(int cin, int cout) {
    if (cin % 64 || cout % 64) return 0;
    const int P = (cin / 64) * (cout / 64);
    if (P > 256 || 256 % P) return 0;
    return 256 / P;
}

// ---- the three inputs ---------------------------------------------------------------------------------------------------------------
struct PlanCtx {
    bool bf16;      // bf16 MFMA operands: the bf16-operand mode (fte_set_mfma_dtype) or a bf16-source (fte_*16) entry point
    bool s16;       // ... and a storage-only launch (bf16 tensors in the epilogue, no fp32 outputs): the persistent kernels of igemm16.hip take it
    bool bn;        // a "BN fusion" launch (fte_conv2d_bn_fwd, fte_conv2d_dgrad_bn): no split-K (the statistics / BN sums come from the
                    // epilogue of the launch that holds the whole reduction) and the per-tile kernels, whose shared epilogue carries them
    int algo;       // fte_set_conv_algo: 0 = direct, 1 = Winograd wherever the kernels exist, 2 = auto (wino_sized's rule)
};

struct PlanDevice {
    int cus;                 // compute units (MI355X: 256)
    int sk_bpc[5][2];        // [tile][epi]: resident stream-K blocks per CU of the tiles the planner asks about (sk_tile); 0: no stream-K there
};

// One field per switch, named after it; `*_set`: the switch is present, where a rule asks that.  The rule a switch tunes -- and the
// measurement behind its default -- is where the field is read.
struct PlanKnobs {
    long pick_want, pick_want16, fills16;
    int narrow_tile, wide_tile; bool narrow_tile_set, wide_tile_set;
    int sk, sk_tile, sk_tile_dgrad, sk_ops; double sk_max_per_cu; long sk_min_steps;
    bool plan_unsplit16, plan16_nosplit, tail_split_set;
    int min_splitp, split_minsteps, split_mink, split_rounds, split_minrounds;
    int wino_min_c, wino_fwd_tpb, wino_ops, wino_ops64;
    bool dgrad_cls_big, dgrad_merged16, dgrad_classes_set; char dgrad_classes;      // first letter of "split" | "merged"
    bool wgrad_split_major; int wgrad_tile;
};
inline PlanKnobs plan_knobs_from_env() {
    auto num = [](const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; };
    auto flag = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    PlanKnobs k;
    memset(&k, 0, sizeof(k));
    k.pick_want = num("FTE_PICK_WANT", 384); k.pick_want16 = num("FTE_PICK_WANT16", 120); k.fills16 = num("FTE_FILLS16", 384);
    k.narrow_tile = flag("FTE_NARROW_TILE", TILE_64x64); k.narrow_tile_set = getenv("FTE_NARROW_TILE") != nullptr;
    k.wide_tile = flag("FTE_WIDE_TILE", TILE_64x64); k.wide_tile_set = getenv("FTE_WIDE_TILE") != nullptr;
    k.sk = flag("FTE_SK", 1);                                 // 0: off; 1: plan_sk's rule; 2: every eligible launch (tests, A/B)
    k.sk_tile = flag("FTE_SK_TILE", -1); k.sk_tile_dgrad = flag("FTE_SK_TILE_DGRAD", k.sk_tile);
    k.sk_ops = flag("FTE_SK_OPS", 3);                         // A/B hook: 1 = forward only, 2 = data gradient only
    k.sk_max_per_cu = getenv("FTE_SK_MAX_PER_CU") ? atof(getenv("FTE_SK_MAX_PER_CU")) : 4.0;
    k.sk_min_steps = num("FTE_SK_MIN_STEPS", 12);             // K-steps per worker
    k.plan_unsplit16 = flag("FTE_PLAN_UNSPLIT16", 1) != 0; k.plan16_nosplit = flag("FTE_PLAN16_NOSPLIT", 1) != 0;
    k.tail_split_set = getenv("FTE_TAIL_SPLIT") != nullptr;
    k.min_splitp = flag("FTE_MIN_SPLITP", 2); k.split_minsteps = flag("FTE_SPLIT_MINSTEPS", 0);
    k.split_mink = flag("FTE_SPLIT_MINK", 256);               // shortest K range per split
    k.split_rounds = flag("FTE_SPLIT_ROUNDS", 3); k.split_minrounds = flag("FTE_SPLIT_MINROUNDS", 1);
    k.wino_min_c = flag("FTE_WINO_MIN_C", 128); k.wino_fwd_tpb = flag("FTE_WINO_FWD_TPB", 256);
    k.wino_ops = flag("FTE_WINO_OPS", 7); k.wino_ops64 = flag("FTE_WINO_OPS64", 5);      // A/B hooks: bit per op
    k.dgrad_cls_big = flag("FTE_DGRAD_CLS_BIG", 0) == 1; k.dgrad_merged16 = flag("FTE_DGRAD_MERGED16", 0) == 1;
    k.dgrad_classes_set = getenv("FTE_DGRAD_CLASSES") != nullptr; k.dgrad_classes = k.dgrad_classes_set ? getenv("FTE_DGRAD_CLASSES")[0] : 0;
    k.wgrad_split_major = flag("FTE_WGRAD_SPLIT_MAJOR", 1) != 0;      // 0 = 2-D grid
    k.wgrad_tile = flag("FTE_WGRAD_TILE", -1);
    return k;
}
struct Planner { PlanKnobs k; PlanDevice d; };

// ---- tiles --------------------------------------------------------------------------------------------------------------------------
struct Pads { int out, before; };
inline Pads same_pads(int in, int k, int stride) {
    const int out = (in + stride - 1) / stride;
    int total = (out - 1) * stride + k - in;
    if (total < 0) total = 0;
    return {out, total / 2};
}
struct ConvShape { int n, h, wd, cin, cout, ksize, stride; };

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr size_t SCRATCH_BYTES = (size_t)REDUCE_SCRATCH_FLOATS * sizeof(float);

inline long tiles_of(int tile, long M, long N) {
    int bm, bn;
    igemm_tile_dims(tile, &bm, &bn);
    return ((M + bm - 1) / bm) * (N / bn);
}

// Largest tile that still gives the chip >= 1.5 blocks per CU; else the smallest legal one.
inline int pick_tile(const PlanKnobs& k, bool bf16, long M, long N) {
    // pick_want: (measured again in round 2 on the BN nets: 384 / 800 / 1200 / always-smallest are within 0.5 %)
    // bf16 operands: the 128-row tiles run on the LDS-DMA kernels (igemm16.hip), the 64 x 64 tile on the register-staged one, which is
    // the slower kernel by more than the half-empty chip costs the larger tiles (FTE_PICK_WANT16 sweep in DESIGN.md)
    const long want = bf16 ? k.pick_want16 : k.pick_want;
    const int cands[3] = {N % 128 == 0 ? TILE_128x128 : TILE_256x64, TILE_128x64, TILE_64x64};
    for (int i = 0; i < 3; ++i)
        if (tiles_of(cands[i], M, N) >= want) return cands[i];
    return cands[2];
}

// Resident blocks the planner assumes: 256 CUs x 6 blocks of the 64x64 tile (16 KiB of LDS, <= 80 VGPRs).
// fp32 MFMAs are 64 cycles each, so operand reuse is not what limits these kernels -- latency hiding is: on
// MI355X at batch 512 the conv time per step is 60.7 ms with 128x128 tiles at 2 blocks/CU, 56.2 ms at 3 blocks/CU
// (single LDS stage) and 53.4 ms with 64x64 tiles at 6 blocks/CU.
constexpr long SLOTS_BIG = 768;       // 128x128 / 128x64 tiles (wgrad, dense split-K): 3 blocks per CU
constexpr long SLOTS = 1536;

// Row plan of an M x N output with reduction length K.  T big tiles on SLOTS resident blocks run in
// ceil(T/SLOTS) rounds, so a launch of 1568 tiles pays for 4 rounds while doing 3.06 rounds of work.  The
// plan keeps whole rounds in a big-tile MAIN launch (epilogue fused in the kernel) and runs the leftover
// tiles -- or ALL tiles when there is less than one round of them (small per-GPU shards) -- as a TAIL:
//   mode 2 (needs workspace): the same big tiles with split-K, P = SLOTS / tiles splits, raw partial
//          tiles to the workspace, then igemm_fixup sums them and applies the epilogue;
//   mode 1 (no workspace / P < 2): 64x64 tiles (4x the blocks, 1/4 of the work each).
//   mode 3 (needs workspace): STREAM-K -- one launch of resident workers that share the (tile, K-step) space equally (igemm.hip
//          "stream-K"); main_tile / main_mtiles describe its tile grid (the partial rows of dalpha / dbias are per tile row as ever).
struct RowPlan {
    int main_tile; long main_rows, main_mtiles;
    int tail_mode, tail_tile; long tail_mtiles; int tail_splits, tail_kchunk; size_t pw_bytes;
    int sk_workers;
};

// Stream-K plan of an fp32 forward / data-gradient launch, or false.  The one-block-per-tile schedule finishes a launch of T tiles on
// S = CUs x blocks-per-CU slots in ceil-ish rounds: what the chip loses is (rounds up - rounds) of the LAST round, which matters when
// there are only one or two (the 64- and 128-image shards of SphereNet: 14x14x256 at 64 images is 1.53 tiles of 128x64 per CU).
// measured on MI355X (profiles/r5_notes.md): forward -- 64x64 tiles, six workers per CU; data gradient (more registers: the
// PReLU / partial-sum epilogue) -- 128x64 tiles, four per CU.  (A 128x128 tile falls back to 128x64 where N % 128.)
inline int sk_tile(const PlanKnobs& k, int epi) {
    const int want = epi == EPI_FWD ? k.sk_tile : k.sk_tile_dgrad;
    return want >= 0 ? want : (epi == EPI_FWD ? TILE_64x64 : TILE_128x64);
}
inline bool plan_sk(const Planner& pl, long M, long N, long K, int epi, RowPlan* out) {
    const PlanKnobs& k = pl.k;
    if (!k.sk || K % 32 || N % 64 || !(k.sk_ops & (epi == EPI_FWD ? 1 : 2))) return false;
    const long ksteps = K / 32;
    int tile = sk_tile(k, epi);
    if (tile == TILE_128x128 && N % 128) tile = TILE_128x64;
    const int bpc = tile < 5 ? pl.d.sk_bpc[tile][epi] : 0;
    if (bpc <= 0) return false;
    int bm, bn;
    igemm_tile_dims(tile, &bm, &bn);
    const long MT = (M + bm - 1) / bm, T = MT * (N / bn), iters = T * ksteps;
    long W = (long)pl.d.cus * bpc;
    if (iters >= (1L << 31)) return false;
    if (k.sk == 1) {
        // The rule, in units of 128x64 tiles per CU (the one-block-per-tile plans' tile at these sizes): stream-K wins up to ~3 tiles
        // per CU (14x14x256 at 64 images, 1.53 per CU: forward 152 -> 127 us, data gradient 160 -> 138; at 128 images, 3.06: 248 ->
        // 228 / 255 -> 245), is even at ~6 (28x28x128 at 128 images) and loses at 12 (56x56x64: 304 -> 321); and every worker should
        // have a few K-steps of its own.
        const double per_cu = (double)(((M + 127) / 128) * (N / 64)) / pl.d.cus;
        if (per_cu > k.sk_max_per_cu) return false;
        if (iters / W < k.sk_min_steps) return false;
    }
    if (W > iters) W = iters;
    memset(out, 0, sizeof(*out));
    out->main_tile = tile; out->main_rows = M; out->main_mtiles = MT;
    out->tail_mode = 3; out->sk_workers = (int)W;
    out->pw_bytes = igemm_sk_ws_bytes(tile, (int)W);
    return true;
}

inline RowPlan plan_rows(const Planner& pl, PlanCtx c, long M, long N, long K, bool allow_pw, bool small_only = false, int epi = -1) {
    const PlanKnobs& k = pl.k;
    RowPlan r;
    memset(&r, 0, sizeof(r));
    if (c.bn) allow_pw = false;
    if (epi >= 0 && allow_pw && !small_only && !c.bf16 && plan_sk(pl, M, N, K, epi, &r)) return r;
    // narrow_tile (N = 64), default 64x64: measured on MI355X
    // 64x64 beats 128x64 beats 256x64 (fwd 83 / 82 / 75 TF, dgrad 80 / 76 / 65): with only 18 K-steps per tile the
    // layer lives on co-resident blocks hiding each other's prologue / epilogue, not on operand reuse.
    // bf16-operand mode: the loop is instruction-issue bound (17 VALU + 20 SALU per MFMA on the 64x64 tile), so the tile
    // with 4x the MFMAs per staged operand wins where N allows it and the launch still fills the chip (batch 512: forward
    // 6.8 -> 5.8 ms, dgrad 8.1 -> 7.5 ms per step; at batch 64 the big tile loses: 3.7 -> 4.7 ms);
    // the short-K stride-2 dgrad classes stay on 64x64 (`small_only`)
    // fills16: half a round: measured 768 / 384 / 190 / 120 on the bf16s nets
    const bool fills = ((M + 127) / 128) * (N / 128) >= k.fills16;        // at least one round of the big tile's slots
    const int wide = (!k.wide_tile_set && c.bf16 && !small_only && fills) ? TILE_128x128 : k.wide_tile;
    const bool fills_n = ((M + 127) / 128) * (N / 64) >= k.fills16;
    const int narrow = (!k.narrow_tile_set && c.bf16 && !small_only && fills_n) ? TILE_128x64 : k.narrow_tile;   // N = 64 layers: +3 %
    // fp32, very tall outputs (>= 4096 tiles of 128 x 64: the 56x56 and 28x28 layers at batch 512): 128 x 64 tiles -- two
    // accumulator blocks per wave, 32 MFMAs per barrier instead of 16 -- measured after the K-order / priority work of round 2:
    // 28x28x128->128 forward 123.5 -> 130.1, dgrad 120.3 -> 127.3 TFLOP/s, 56x56x64->64 91.2 -> 93.3 / 94.8 -> 97.1; at 14x14 and
    // below (fewer tiles than ~4 rounds of the big tile's slots) the 64 x 64 tile stays ahead
    // (not for K < 576: with two K-steps per tile the bigger tile only lengthens the epilogue -- 28x28x64->256 dgrad 122 vs 92 us)
    const bool tall = !k.wide_tile_set && !k.narrow_tile_set && !c.bf16 && !small_only && K >= 576 && ((M + 127) / 128) * (N / 64) >= 4096;
    const int big = tall ? TILE_128x64 : ((N % 128 == 0) ? wide : narrow);
    int bm, bn;
    igemm_tile_dims(big, &bm, &bn);
    const long ntn = N / bn, MT = (M + bm - 1) / bm, T = MT * ntn, ksteps = (K + 31) / 32;
    r.main_tile = big;
    long tail_rows = 0;
    // bf16-STORAGE launches (fte_conv2d_{fwd,dgrad}_s16 without fp32 outputs) with at least a round of the window kernel's 256-row
    // tiles stay ONE unsplit launch: resident loader / consumer blocks (igemm16rw) beat split-K + fix-up there -- 7x7x512 at batch 512:
    // forward 0.186 -> 0.134 ms, data gradient 0.214 -> 0.148.  FTE_PLAN_UNSPLIT16=0 restores the split plan.
    if (k.plan_unsplit16 && c.s16 && !small_only) {
        const int t16 = N % 128 == 0 ? TILE_128x128 : TILE_128x64;
        const long m16 = (M + 127) / 128, n16 = (M + 127) / 128 * (N / (N % 128 == 0 ? 128 : 64));
        if (n16 >= 512 && n16 < SLOTS) { r.main_tile = t16; r.main_rows = M; r.main_mtiles = m16; return r; }
    }
    if (T >= SLOTS) {
        const long full = T / SLOTS * SLOTS;
        // A leftover fraction of a round used to go to a separate small-tile TAIL launch (mode 1 below).  Measured again at the end of
        // round 2 it no longer pays: blocks of a many-round launch drift apart, the last partial round is absorbed, and the tail
        // launch's own ramp costs more -- SphereNet step 49.30 -> 49.16 ms fp32, 17.15 -> 16.78 ms in the bf16 mode (whose main
        // launches are 4x shorter).  FTE_TAIL_SPLIT=1 brings the tail back (A/B hook).
        if ((bm == 64 && bn == 64) || T - full == 0 || T - full >= SLOTS * 4 / 5 || !k.tail_split_set) {
            r.main_rows = M; r.main_mtiles = MT;
            return r;
        }
        r.main_mtiles = full / ntn;
        r.main_rows = r.main_mtiles * bm;
        tail_rows = M - r.main_rows;
    } else {
        tail_rows = M;                                            // less than one round in total
    }
    const long tmt = (tail_rows + bm - 1) / bm, R = tmt * ntn;
    long P = (SLOTS + R / 2) / R;
    // every split keeps >= 32 K-steps (K = 1024): the 4x4x512->512 1x1 convs of ShuffleNet's last stage (1024 tiles, P = 2) ran
    // 58 us split + fixed up against 43 us in one launch, and with 16..32 K-steps per split the 1x1 convs of the ResNet family
    // lose too (SE-ResNet-50 at 128 per GPU +1.1 % without those splits); the 3x3 layers of SphereNet at 64 images per GPU
    // (K = 2304 / 4608, 36 K-steps per split) kept theirs while the step ran on one stream (48 cost them 1.4 %).  With the filter
    // gradients on a second stream (nets/sphere.py) a half-filled launch is no longer alone on the chip and the 2-way splits of the
    // K = 2304 layers stop paying once the unsplit launch has a block for every CU: 48 steps per split there, one GPU, images/s:
    // 32 per GPU 6.99 k -> 7.15 k, 64: 8.40 k -> 8.50 k (bf16 mode 16.2 k -> 17.5 k), 128 / 256 and the BN nets unchanged.
    const int min_steps = k.split_minsteps > 0 ? k.split_minsteps : (R >= 256 ? 48 : 32);
    if (P > ksteps / min_steps) P = ksteps / min_steps;
    // Split-K pays only when there is NO whole round (small per-GPU shards): measured on MI355X at batch
    // 512 a 32-tile tail split 16 ways is slower than the 64x64 tail (which costs ~3 % of the kernel).
    // P = 2 (min_splitp) already pays (batch 64, 14x14x256: 96 -> 101 TFLOP/s forward, 89 -> 95
    // dgrad; batch 128, 7x7x512: 100 -> 111); P = 1 means the tiles fill the chip on their own.
    // bf16 plans: an unsplit launch on the LDS-DMA kernels (three-stage ring below 768 tiles) instead of split-K + fix-up on the
    // register-staged 64x64 kernel, whenever the 128-row tiles give pick_tile's minimum.  FTE_PLAN16_NOSPLIT=0: the split plan.
    if (k.plan16_nosplit && c.bf16 && !small_only && T < SLOTS) {
        const int t16 = pick_tile(k, c.bf16, M, N);
        if (t16 == TILE_128x128 || t16 == TILE_128x64) {
            int tbm, tbn;
            igemm_tile_dims(t16, &tbm, &tbn);
            r.main_tile = t16; r.main_rows = M; r.main_mtiles = (M + tbm - 1) / tbm;
            return r;
        }
    }
    if (allow_pw && P >= k.min_splitp && T < SLOTS) {
        r.tail_mode = 2; r.tail_tile = big; r.tail_mtiles = tmt * FIXUP_CHUNKS;   // partial rows: one per (tile row, chunk)
        r.tail_kchunk = (int)((ksteps + P - 1) / P * 32);
        r.tail_splits = (int)((K + r.tail_kchunk - 1) / r.tail_kchunk);
        r.pw_bytes = (size_t)r.tail_splits * R * bm * bn * sizeof(float);
        return r;
    }
    if (T >= SLOTS) {
        r.tail_mode = 1; r.tail_tile = TILE_64x64; r.tail_mtiles = (tail_rows + 63) / 64;
        return r;
    }
    r.main_tile = pick_tile(k, c.bf16, M, N);                     // single launch with a smaller tile
    igemm_tile_dims(r.main_tile, &bm, &bn);
    r.main_rows = M; r.main_mtiles = (M + bm - 1) / bm;
    return r;
}

// split-K plan: pick the split count whose tiles*splits fills whole rounds of SLOTS_BIG best
// (>= split_mink of K per split; ties go to fewer splits = less slab traffic)
inline void plan_splits(const PlanKnobs& k, long tiles, int K, int* splits, int* kchunk, bool prefer8 = false) {
    const int maxs = K / k.split_mink > 0 ? K / k.split_mink : 1;
    long lo = (k.split_minrounds * SLOTS_BIG + tiles - 1) / tiles, hi = (k.split_rounds * SLOTS_BIG + tiles - 1) / tiles;
    if (lo < 1) lo = 1;
    if (hi > maxs) hi = maxs;
    if (lo > hi) lo = hi;
    double best = -1.0;
    int bs = 1;
    for (long sI = lo; sI <= hi; ++sI) {
        const int kc = (int)(((K + sI - 1) / sI + 31) / 32 * 32);
        const long sp = (K + kc - 1) / kc;
        const double rounds = (double)(tiles * sp) / SLOTS_BIG;
        double eff = rounds / (double)(long)(rounds + 0.999999);
        if (prefer8 && sp % 8 == 0) eff += 0.05;     // split-major placement: one K range per XCD
        if (eff > best + 0.02) { best = eff; bs = (int)sI; }
    }
    const int kc = ((K + bs - 1) / bs + 31) / 32 * 32;
    *kchunk = kc;
    *splits = (K + kc - 1) / kc;
}

// ---- dense products -----------------------------------------------------------------------------------------------------------------
// split-K plan of a dense product with `rows` x `cols` outputs and reduction length `red`: fewer than 256 tiles -> plan_splits
struct DensePlan { int splits, kchunk; size_t slab_bytes; };
inline DensePlan dense_plan(const PlanKnobs& k, int tile, long rows, long cols, int red) {
    DensePlan d = {1, (red + 31) / 32 * 32, 0};
    if (tiles_of(tile, rows, cols) < 256) plan_splits(k, tiles_of(tile, rows, cols), red, &d.splits, &d.kchunk);
    d.slab_bytes = d.splits > 1 ? (size_t)d.splits * rows * cols * sizeof(float) : 0;
    return d;
}
inline int tn_tile(long k, long n) {
    return (n % 128 == 0) ? (tiles_of(TILE_128x128, k, n) >= 384 ? TILE_128x128 : TILE_128x64) : TILE_128x64;
}

// ---- Winograd F(2x2, 3x3) plan (wino.hip) ---------------------------------------------------------------------------------------
// The stride-1 3x3 layers of the BN-free fp32 path (nets/sphere.py:41-42) may run as 16 products of 1/2.25 of the MACs.  FTE_CONV_ALGO /
// fte_set_conv_algo: direct = never, winograd = wherever the kernels exist (channels % 64, fp32 operands), auto = the measured rule:
// layers of >= FTE_WINO_MIN_C channels (default 128: SphereNet's stages 2-4) take it for all three products; 64-channel layers per FTE_WINO_OPS64 -- below that the transform traffic (16 floats per tile and channel, in
// and out of HBM) outweighs the saved MFMA time.
// forward-side tile transforms in 256-thread blocks (wino.h; the default: 72 registers per SIMD fit beside a resident block of the forward
// product, so one half shard's transform runs under the other's product -- nets/sphere.py backbone; alone 34.72 -> 34.58 ms per step at 512
// images, with the half shards 34.36 -> 34.21).  FTE_WINO_FWD_TPB=512: the 512-thread blocks of the data-gradient side.
inline bool wino_fwd_small_tiles(const PlanKnobs& k) { return k.wino_fwd_tpb != 512; }
inline bool wino_shape_ok(const ConvShape& s) {
    if (s.ksize != 3 || s.stride != 1 || s.cin % 64 || s.cout % 64 || s.n <= 0 || s.h < 2 || s.wd < 2) return false;
    const size_t lim = (size_t)1 << 31;
    return (size_t)s.n * s.h * s.wd * s.cin * 4 < lim && (size_t)s.n * s.h * s.wd * s.cout * 4 < lim;
}
// op: 0 forward, 1 data gradient, 2 filter gradient.  wino_sized: the switch `algo` would pick the algorithm for this layer in the
// fp32 mode (what the workspace queries size for); wino_wanted: ... and this launch is an fp32, BN-free one
inline bool wino_sized(const PlanKnobs& k, int algo, const ConvShape& s, int op) {
    if (algo == 0 || !wino_shape_ok(s)) return false;
    if (op == 2 && !wino_wgrad_splits(s.cin, s.cout)) return false;
    if (algo == 1) return true;
    // 64-channel layers (SphereNet's stage 1, 56x56): the tile packs are 16 floats per tile and channel -- 1.6 GB at 512 images, 0.4 ms of
    // HBM time per transform against ~0.5 ms saved in a product.  Measured (one box, same call): forward + filter gradient (they share
    // one transform) 35.60 -> 34.96 ms per step, the data gradient on top 34.98: it stays direct.  FTE_WINO_OPS64: bit per op for that class
    const int cmin = s.cin < s.cout ? s.cin : s.cout;
    if (cmin < k.wino_min_c) return cmin >= 64 && (k.wino_ops64 & (1 << op)) != 0;
    return (k.wino_ops & (1 << op)) != 0;
}
inline bool wino_wanted(const PlanKnobs& k, PlanCtx c, const ConvShape& s, int op) {
    return !c.bf16 && !c.bn && wino_sized(k, c.algo, s, op);
}
struct WinoWs { size_t v_off, u_off, slab_off, total; };
// workspace layout behind `head` bytes the caller keeps for itself: [V pack | U pack (| slabs)]
inline WinoWs wino_ws(const ConvShape& s, int op, size_t head) {
    const WinoGeom g = wino_geom(s.n, s.h, s.wd);
    WinoWs w;
    w.v_off = align_up(head);
    if (op == 0) {            // V(x): cin channels; U: filters
        w.u_off = w.v_off + align_up(wino_pack_floats(g.M, s.cin) * 4);
        w.slab_off = w.total = w.u_off + align_up((size_t)16 * s.cin * s.cout * 4);
    } else if (op == 1) {     // V(dz): cout channels; U: rotated filters
        w.u_off = w.v_off + align_up(wino_pack_floats(g.M, s.cout) * 4);
        w.slab_off = w.total = w.u_off + align_up((size_t)16 * s.cin * s.cout * 4);
    } else {                  // V(x), slabs (U' of dz is computed inside the kernel)
        w.u_off = w.v_off + align_up(wino_pack_floats(g.M, s.cin) * 4);
        w.slab_off = w.u_off;
        w.total = w.slab_off + align_up((size_t)wino_wgrad_splits(s.cin, s.cout) * 16 * s.cin * s.cout * 4);
    }
    return w;
}

// ---- one layout per op: the plan and the byte offset of everything the op places in its workspace.  The *_ws_bytes query returns the
// largest `total` over the contexts a buffer must serve; the launch reads the offsets -- the arithmetic exists once.
// `total` counts the Winograd layout wherever the switch picks the algorithm for the shape (wino_sized), whatever the context: a buffer
// sized in one mode stays valid in every other.

// forward: [split-K partial tiles | stream-K slabs + flags] at offset 0, or the Winograd packs
struct FwdLayout {
    long M, N, K;
    RowPlan rp;                // with a workspace; without room for rp.pw_bytes the launch re-plans with allow_pw = false
    bool wino;                 // this context runs Winograd when the workspace holds `w` (`w_kept`: the caller keeps V, ws holds the filters only)
    WinoWs w, w_kept;
    size_t total;
};
inline FwdLayout fwd_layout(const Planner& pl, PlanCtx c, const ConvShape& s) {
    const Pads ph = same_pads(s.h, s.ksize, s.stride), pw = same_pads(s.wd, s.ksize, s.stride);
    FwdLayout l;
    memset(&l, 0, sizeof(l));
    l.M = (long)s.n * ph.out * pw.out; l.N = s.cout; l.K = (long)s.ksize * s.ksize * s.cin;
    l.wino = wino_wanted(pl.k, c, s, 0);
    l.rp = plan_rows(pl, c, l.M, l.N, l.K, true, false, EPI_FWD);
    l.total = l.rp.pw_bytes;
    if (wino_sized(pl.k, c.algo, s, 0)) {
        l.w = l.w_kept = wino_ws(s, 0, 0);
        l.w_kept.u_off = 0; l.w_kept.total = align_up((size_t)16 * s.cin * s.cout * 4);
        if (l.w.total > l.total) l.total = l.w.total;
    }
    return l;
}

// data gradient.  One GEMM per output-parity class of the stride (1 or 4 of them), or one merged launch of all four.
struct DgradClass { int ph, pw, hq, wq, ntap, dh[9], dw[9], wt[9]; RowPlan rp; long mtiles; };
inline int dgrad_classes(const Planner& pl, PlanCtx ctx, const ConvShape& s, DgradClass* cls) {
    const Pads ph = same_pads(s.h, s.ksize, s.stride), pw = same_pads(s.wd, s.ksize, s.stride);
    int nc = 0;
    for (int a = 0; a < s.stride; ++a)
        for (int b = 0; b < s.stride; ++b) {
            DgradClass& c = cls[nc];
            c.ph = a; c.pw = b;
            c.hq = (s.h - a + s.stride - 1) / s.stride;
            c.wq = (s.wd - b + s.stride - 1) / s.stride;
            c.ntap = 0;
            if (c.hq <= 0 || c.wq <= 0) continue;
            for (int r = 0; r < s.ksize; ++r) {
                if ((a + ph.before - r) % s.stride) continue;
                for (int t = 0; t < s.ksize; ++t) {
                    if ((b + pw.before - t) % s.stride) continue;
                    // hi = ho*stride + r - pt  with hi = hq*stride + a  ->  ho = hq + (a + pt - r)/stride
                    c.dh[c.ntap] = (a + ph.before - r) / s.stride;
                    c.dw[c.ntap] = (b + pw.before - t) / s.stride;
                    c.wt[c.ntap] = r * s.ksize + t;
                    ++c.ntap;
                }
            }
            // FTE_DGRAD_CLS_BIG=1 (A/B hook): let the bf16 plans give the parity classes the 128-row tiles of the LDS-DMA kernels
            c.rp = plan_rows(pl, ctx, (long)s.n * c.hq * c.wq, s.cin, (long)c.ntap * s.cout, true, s.stride != 1 && !pl.k.dgrad_cls_big, EPI_DGRAD);
            c.mtiles = c.rp.main_mtiles + c.rp.tail_mtiles;
            ++nc;
        }
    return nc;
}
// stride-2 3x3 with even image sides: the four classes have identical row grids and 4 / 2 / 2 / 1 taps
// ... and only while one class alone cannot fill the chip (fewer 64x64 tiles than resident slots: the small per-GPU
// shards).  Measured on MI355X, 28x28x128 <- 256 at batch 512: four launches 0.55 ms, the merged one 0.75 ms with the SAME
// instruction counts but half the resident waves (PMC); at batch 64 the merged launch is the faster one (36 -> 50 TFLOP/s).
// FTE_DGRAD_MERGED16=1 (A/B hook): in the bf16 plans the four classes always share ONE launch on the LDS-DMA kernels' 128-row tiles
// FTE_DGRAD_CLASSES (tuning hook): "split" | "merged"
inline bool dgrad_mergeable(const PlanKnobs& k, PlanCtx c, const DgradClass* cls, int nc, int n, int cin) {
    if (nc != 4 || k.dgrad_classes == 's') return false;
    for (int i = 0; i < nc; ++i)
        if (cls[i].hq != cls[0].hq || cls[i].wq != cls[0].wq || cls[i].ntap < 1) return false;
    if (k.dgrad_classes == 'm' || (k.dgrad_merged16 && c.bf16)) return true;
    const long tiles = (((long)n * cls[0].hq * cls[0].wq + 63) / 64) * (cin / 64);
    return tiles < SLOTS;
}
inline int dgrad_merged_tile(const PlanKnobs& k, PlanCtx c, int cin) {
    if (!(k.dgrad_merged16 && c.bf16)) return TILE_64x64;
    return cin % 128 == 0 ? TILE_128x128 : TILE_128x64;
}
// partial rows (one per tile row and class) the merged launch writes for dalpha / dbias
inline long dgrad_merged_rows(const PlanKnobs& k, PlanCtx c, const DgradClass* cls, int nc, int n, int cin) {
    if (!dgrad_mergeable(k, c, cls, nc, n, cin)) return 0;
    int bm, bn;
    igemm_tile_dims(dgrad_merged_tile(k, c, cin), &bm, &bn);
    return (long)nc * (((long)n * cls[0].hq * cls[0].wq + bm - 1) / bm);
}
// tile of the merged launch and the class order (most taps first)
inline int dgrad_merged_plan(const PlanKnobs& k, PlanCtx c, const DgradClass* cls, int nc, int cin, int* order) {
    for (int i = 0; i < nc; ++i) order[i] = i;
    for (int i = 0; i < nc; ++i)
        for (int j = i + 1; j < nc; ++j)
            if (cls[order[j]].ntap > cls[order[i]].ntap) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    return dgrad_merged_tile(k, c, cin);
}
// direct: [PA rows | PB rows | reduction scratch | split-K tiles / stream-K slabs of the class in flight]
// Winograd: [PA | PB (one row per row block) | scratch | V | U]
struct DgradLayout {
    int nc; DgradClass cls[4];
    bool merged; int merged_tile, order[4];
    long rows;                 // partial rows of dalpha / dbias the launch(es) write
    size_t half, scratch_off, pw_off, pw_bytes, need;      // PA at 0, PB at half; need: bytes this context's direct launch touches
    bool wino; size_t wino_half; WinoWs w;      // (wino_half: PB offset of the Winograd form, its scratch at 2 * wino_half)
    size_t total;              // sized for the per-class and the merged form alike (64-row tiles give the most partial rows)
};
inline DgradLayout dgrad_layout(const Planner& pl, PlanCtx c, const ConvShape& s) {
    DgradLayout l;
    memset(&l, 0, sizeof(l));
    l.nc = dgrad_classes(pl, c, s, l.cls);
    l.merged = dgrad_mergeable(pl.k, c, l.cls, l.nc, s.n, s.cin);
    long rows = 0;
    size_t pw = 0;
    for (int i = 0; i < l.nc; ++i) { rows += l.cls[i].mtiles; if (l.cls[i].rp.pw_bytes > pw) pw = l.cls[i].rp.pw_bytes; }
    const long merged_rows = dgrad_merged_rows(pl.k, c, l.cls, l.nc, s.n, s.cin);
    if (l.merged) l.merged_tile = dgrad_merged_plan(pl.k, c, l.cls, l.nc, s.cin, l.order);
    l.rows = l.merged ? merged_rows : rows;
    l.half = align_up((size_t)l.rows * s.cin * sizeof(float));
    l.scratch_off = 2 * l.half; l.pw_off = l.scratch_off + SCRATCH_BYTES;
    l.pw_bytes = l.merged ? 0 : pw;
    l.need = l.pw_off + l.pw_bytes;
    l.total = 2 * align_up((size_t)(merged_rows > rows ? merged_rows : rows) * s.cin * sizeof(float)) + SCRATCH_BYTES + pw;
    l.wino = wino_wanted(pl.k, c, s, 1);
    if (wino_sized(pl.k, c.algo, s, 1)) {
        l.wino_half = align_up((size_t)wino_geom(s.n, s.h, s.wd).MB * s.cin * sizeof(float));
        l.w = wino_ws(s, 1, 2 * l.wino_half + SCRATCH_BYTES);
        if (l.w.total > l.total) l.total = l.w.total;
    }
    return l;
}

// filter gradient
inline void wgrad_plan(const PlanKnobs& k, const ConvShape& s, int* tile, int* splits, int* kchunk, int* K) {
    const Pads ph = same_pads(s.h, s.ksize, s.stride), pw = same_pads(s.wd, s.ksize, s.stride);
    *K = s.n * ph.out * pw.out;
    const long M = (long)s.ksize * s.ksize * s.cin;
    // N = 64 layers: M = 9 * 64 = 576 is 4.5 tiles of 128 rows (a tenth of the MFMAs multiply zero padding: the stage-1
    // filter gradient ran at 68 % of peak with its MFMA pipe 76 % busy) but exactly 3 tiles of 192
    const int narrow = (M % 192 == 0 && M % 128 != 0) ? TILE_192x64 : TILE_128x64;
    // a filter gradient of at most 256 x 256 (the 1x1 convs of the ShuffleNet stages) is 1-4 tiles of 128 x 128: every block is
    // then one of ~400 K ranges of 256 pixels -- 64 x 64 tiles give 4x the blocks over K ranges 4x as long for the same
    // slab bytes (14x14x128->128 at batch 512: 65 -> 51 us, 7x7x256->256: 52 -> 44 us with the slab reduction)
    const bool tiny = s.ksize == 1 && M * s.cout <= 256L * 256;
    *tile = k.wgrad_tile >= 0 ? k.wgrad_tile : (tiny ? TILE_64x64 : (s.cout % 128 == 0) ? TILE_128x128 : narrow);
    // Block placement: split-major (k.wgrad_split_major, ON by default since round 2; FTE_WGRAD_SPLIT_MAJOR=0 gives the 2-D grid
    // back): the tiles of one pixel range sit 8 block ids apart -- same XCD, same L2 -- so x / dz leave HBM once per pixel range
    // instead of once per tile (stage-1 symbol 2844 -> 904 MB per launch, 128x128 symbol 1923 -> 523 MB) at unchanged kernel
    // time.  `prefer8` (split counts that are multiples of 8) stays off in plan_splits: the kernels are MFMA-bound and the
    // rounder split count cost more than the L2 locality gave (18.4 -> 18.9 ms per step when first measured).
    plan_splits(k, tiles_of(*tile, M, s.cout), *K, splits, kchunk, false);
    // Small per-GPU shards: when filling the chip with big tiles leaves every block fewer than 1024 pixels of K (32 K-steps), take
    // 64 x 64 tiles instead -- 4x the tiles, a quarter of the splits, K ranges 4x as long and a quarter of the slab traffic.
    // SphereNet step, one GPU: batch 32 +5.9 %, 64 +3.2 %, 128 +1.3 %, 256 +-0, 512 -1.1 % (where this rule does not fire).
    if (k.wgrad_tile < 0 && *tile != TILE_64x64 && *splits > 1 && *kchunk < 1024) {
        *tile = TILE_64x64;
        plan_splits(k, tiles_of(*tile, M, s.cout), *K, splits, kchunk, false);
    }
}
// direct: [split-K slabs] at offset 0; the resident bf16 kernels (wgrad16.hip) put THEIR slabs there (`resident3` / `resident1`: bytes
// of the 3x3 and the pointwise kernel's plan, 0 where it does not apply -- wgrad16.hip owns those plans); Winograd: [V | slabs]
struct WgradLayout {
    int tile, splits, kchunk, K;
    size_t slab_bytes;
    bool wino; WinoWs w, w_kept;      // w_kept: V kept by the forward pass, ws holds the slabs only
    size_t total;
};
inline WgradLayout wgrad_layout(const PlanKnobs& k, PlanCtx c, const ConvShape& s, size_t resident3 = 0, size_t resident1 = 0) {
    WgradLayout l;
    memset(&l, 0, sizeof(l));
    wgrad_plan(k, s, &l.tile, &l.splits, &l.kchunk, &l.K);
    l.slab_bytes = l.splits > 1 ? (size_t)l.splits * s.ksize * s.ksize * s.cin * s.cout * sizeof(float) : 0;
    l.total = l.slab_bytes;
    if (resident3 > l.total) l.total = resident3;
    if (resident1 > l.total) l.total = resident1;
    l.wino = wino_wanted(k, c, s, 2);
    if (wino_sized(k, c.algo, s, 2)) {
        l.w = l.w_kept = wino_ws(s, 2, 0);
        const size_t vsz = l.w.u_off - l.w.v_off;
        l.w_kept.u_off -= vsz; l.w_kept.slab_off -= vsz; l.w_kept.total -= vsz;
        if (l.w.total > l.total) l.total = l.w.total;
    }
    l.total += SCRATCH_BYTES;
    return l;
}
