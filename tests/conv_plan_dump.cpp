// conv_plan_dump.cpp -- stand-alone driver of csrc/conv_plan.h for tests/test_conv_plan_host.py (no GPU, no HIP):
//     conv_plan_dump CASEFILE CUS B64F B64D B128x64F B128x64D B128F B128D [--layouts]
// PlanKnobs come from the environment, PlanDevice from the arguments (CU count; resident stream-K blocks per CU of the 64x64, 128x64 and
// 128x128 tiles, forward and data gradient).  CASEFILE holds one case per line (tests/conv_plan_cases.py):
//     conv n h w cin cout ksize stride | rows M N K allow_pw small_only epi | splits tiles K | dense m n k
// One JSON line per case goes to stdout.  --layouts adds every context's layout totals and the query totals (the invariants' input).
#include <stdio.h>

#include "../tf_face_toolbox_amd/csrc/conv_plan.h"

static const char* const CTX_NAME[5] = {"f32", "bf16", "s16", "f32bn", "s16bn"};
static PlanCtx ctx_of(int i, int algo) {
    const PlanCtx c[5] = {{false, false, false, algo}, {true, false, false, algo}, {true, true, false, algo},
                          {false, false, true, algo}, {true, true, true, algo}};
    return c[i];
}
static void put_rows(const RowPlan& r) {
    printf("[%d,%ld,%ld,%d,%d,%ld,%d,%d,%zu,%d]", r.main_tile, r.main_rows, r.main_mtiles, r.tail_mode, r.tail_tile, r.tail_mtiles,
           r.tail_splits, r.tail_kchunk, r.pw_bytes, r.sk_workers);
}
static void put_ws(const WinoWs& w) { printf("[%zu,%zu,%zu,%zu]", w.v_off, w.u_off, w.slab_off, w.total); }

static void dump_conv(const Planner& pl, const ConvShape& s, bool layouts) {
    const PlanKnobs& k = pl.k;
    const bool fwd_ok = s.cin % 32 == 0 && s.cout % 64 == 0, dg_ok = s.cin % 64 == 0 && s.cout % 32 == 0, wg_ok = s.cin % 4 == 0 && s.cout % 64 == 0;
    printf("{\"case\":[\"conv\",%d,%d,%d,%d,%d,%d,%d],\"ctx\":{", s.n, s.h, s.wd, s.cin, s.cout, s.ksize, s.stride);
    for (int ci = 0; ci < 5; ++ci) {
        const PlanCtx c = ctx_of(ci, 2);
        printf("%s\"%s\":{", ci ? "," : "", CTX_NAME[ci]);
        printf("\"wanted\":[%d,%d,%d]", wino_wanted(k, c, s, 0), wino_wanted(k, c, s, 1), wino_wanted(k, c, s, 2));
        if (fwd_ok) {
            const FwdLayout l = fwd_layout(pl, c, s);
            printf(",\"fwd\":"); put_rows(l.rp);
            printf(",\"fwd_nows\":"); put_rows(plan_rows(pl, c, l.M, l.N, l.K, false));
            printf(",\"pick\":%d", pick_tile(k, c.bf16, l.M, l.N));
            if (layouts) printf(",\"fwd_total\":%zu", l.total);
        }
        if (dg_ok) {
            const DgradLayout l = dgrad_layout(pl, c, s);
            printf(",\"cls\":[");
            for (int i = 0; i < l.nc; ++i) {
                printf("%s[%d,%d,%d,%ld,", i ? "," : "", l.cls[i].ntap, l.cls[i].hq, l.cls[i].wq, l.cls[i].mtiles);
                put_rows(l.cls[i].rp);
                printf("]");
            }
            int order[4] = {0, 1, 2, 3};
            const int mtile = dgrad_merged_plan(k, c, l.cls, l.nc, s.cin, order);
            printf("],\"merged\":[%d,%ld,%d,[", l.merged, dgrad_merged_rows(k, c, l.cls, l.nc, s.n, s.cin), mtile);
            for (int i = 0; i < l.nc; ++i) printf("%s%d", i ? "," : "", order[i]);
            printf("]]");
            if (layouts) printf(",\"dgrad_total\":%zu,\"dgrad_need\":%zu,\"dgrad_rows\":%ld", l.total, l.need, l.rows);
        }
        printf("}");
    }
    printf("}");
    if (wg_ok) {
        const WgradLayout l = wgrad_layout(k, ctx_of(0, 2), s);
        printf(",\"wgrad\":[%d,%d,%d,%d,%d]", l.tile, l.splits, l.kchunk, l.K, (k.wgrad_split_major && l.splits > 1) ? l.splits : 0);
    }
    printf(",\"sized\":[");
    for (int algo = 0; algo < 3; ++algo)
        printf("%s[%d,%d,%d]", algo ? "," : "", wino_sized(k, algo, s, 0), wino_sized(k, algo, s, 1), wino_sized(k, algo, s, 2));
    printf("]");
    if (wino_shape_ok(s)) {
        const size_t head1 = 2 * align_up((size_t)wino_geom(s.n, s.h, s.wd).MB * s.cin * sizeof(float)) + SCRATCH_BYTES;
        printf(",\"wino_ws\":["); put_ws(wino_ws(s, 0, 0)); printf(","); put_ws(wino_ws(s, 1, head1));
        if (wino_wgrad_splits(s.cin, s.cout)) { printf(","); put_ws(wino_ws(s, 2, 0)); }
        printf("]");
    }
    if (layouts) {          // what the *_ws_bytes queries answer per algorithm switch (the filter gradient without wgrad16.hip's slabs)
        printf(",\"query\":[");
        for (int algo = 0; algo < 3; ++algo) {
            size_t q[3] = {0, 0, 0};
            for (int ci = 0; ci < 3; ++ci) {
                const PlanCtx c = ctx_of(ci, algo);
                size_t t = fwd_ok ? fwd_layout(pl, c, s).total : 0; if (t > q[0]) q[0] = t;
                t = dg_ok ? dgrad_layout(pl, c, s).total : 0; if (t > q[1]) q[1] = t;
                t = wg_ok ? wgrad_layout(k, c, s).total : 0; if (t > q[2]) q[2] = t;
            }
            printf("%s[%zu,%zu,%zu]", algo ? "," : "", q[0], q[1], q[2]);
        }
        printf("]");
    }
    printf("}\n");
}

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s CASEFILE CUS B64F B64D B128x64F B128x64D B128F B128D [--layouts]\n", argv[0]); return 2; }
    Planner pl;
    memset(&pl, 0, sizeof(pl));
    pl.k = plan_knobs_from_env();
    pl.d.cus = atoi(argv[2]);
    const int tiles[3] = {TILE_64x64, TILE_128x64, TILE_128x128};
    for (int i = 0; i < 3; ++i)
        for (int e = 0; e < 2; ++e) pl.d.sk_bpc[tiles[i]][e] = atoi(argv[3 + 2 * i + e]);
    const bool layouts = argc > 9 && !strcmp(argv[9], "--layouts");
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char kind[16];
    while (fscanf(f, "%15s", kind) == 1) {
        long v[7] = {0, 0, 0, 0, 0, 0, 0};
        const int want = !strcmp(kind, "conv") ? 7 : !strcmp(kind, "rows") ? 6 : !strcmp(kind, "splits") ? 2 : !strcmp(kind, "dense") ? 3 : -1;
        if (want < 0) { fprintf(stderr, "unknown case kind %s\n", kind); return 2; }
        for (int i = 0; i < want; ++i)
            if (fscanf(f, "%ld", &v[i]) != 1) { fprintf(stderr, "short case line (%s)\n", kind); return 2; }
        if (want == 7) {
            const ConvShape s = {(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6]};
            dump_conv(pl, s, layouts);
        } else if (want == 6) {
            printf("{\"case\":[\"rows\",%ld,%ld,%ld,%ld,%ld,%ld],\"ctx\":{", v[0], v[1], v[2], v[3], v[4], v[5]);
            for (int ci = 0; ci < 5; ++ci) {
                printf("%s\"%s\":", ci ? "," : "", CTX_NAME[ci]);
                put_rows(plan_rows(pl, ctx_of(ci, 2), v[0], v[1], v[2], v[3] != 0, v[4] != 0, (int)v[5]));
            }
            printf("}}\n");
        } else if (want == 2) {
            int sp, kc;
            plan_splits(pl.k, v[0], (int)v[1], &sp, &kc);
            printf("{\"case\":[\"splits\",%ld,%ld],\"splits\":[%d,%d]}\n", v[0], v[1], sp, kc);
        } else {            // the three products of a dense layer, fp32 / bf16 operand mode: [tile, splits, kchunk, slab bytes]
            const long m = v[0], n = v[1], kk = v[2];
            printf("{\"case\":[\"dense\",%ld,%ld,%ld]", m, n, kk);
            for (int b = 0; b < 2; ++b) {
                const int t[3] = {pick_tile(pl.k, b != 0, m, n), pick_tile(pl.k, b != 0, m, kk), tn_tile(kk, n)};
                const DensePlan d[3] = {dense_plan(pl.k, t[0], m, n, (int)kk), dense_plan(pl.k, t[1], m, kk, (int)n), dense_plan(pl.k, t[2], kk, n, (int)m)};
                printf(",\"%s\":[", b ? "bf16" : "f32");
                for (int i = 0; i < 3; ++i) printf("%s[%d,%d,%d,%zu]", i ? "," : "", t[i], d[i].splits, d[i].kchunk, d[i].slab_bytes);
                printf("]");
            }
            printf("}\n");
        }
    }
    fclose(f);
    return 0;
}
