"""The case table of tests/test_conv_plan_host.py: inputs of the planner in csrc/conv_plan.h, each with the branches (TAGS) it is in the
table for.  tests/golden/conv_plans.json holds what the planner answered for every case before it became a header (recorded per
environment: the switches are read once per process); the host test compares the header's answers with it and proves, from the recorded
plans, that every tag is hit by a case that names it.

Case kinds (one line each for tests/conv_plan_dump.cpp):
    ('conv', n, h, w, cin, cout, ksize, stride)      every plan of a conv layer in the five contexts f32 / bf16 / s16 / f32bn / s16bn
    ('rows', M, N, K, allow_pw, small_only, epi)     plan_rows alone (epi -1: no stream-K)
    ('splits', tiles, K)                             plan_splits alone
    ('dense', m, n, k)                               the three products of a dense layer
The recording's device: 256 CUs; resident stream-K blocks per CU 6 / 5 (64x64 forward / data gradient), 4 (128x64), 3 (128x128)."""

T128, T256x64, T128x64, T64, T192 = 0, 1, 2, 3, 4
# RowPlan as the dump prints it
MAIN_TILE, MAIN_ROWS, MAIN_MT, TAIL_MODE, TAIL_TILE, TAIL_MT, TAIL_SPLITS, TAIL_KCHUNK, PW_BYTES, SK_WORKERS = range(10)
SLOTS = 1536


def _up(a, b):
    return (a + b - 1) // b


# ---- the layers the benchmarks run -------------------------------------------------------------------------------------------------
def sphere20(n):
    """SphereNet-20 at 112 x 112: the stride-2 conv of stages 2-4 and the residual convs of all four (the 3-channel stem has its own kernel)"""
    out = []
    for side, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        if c > 64:
            out.append(('conv', n, side * 2, side * 2, c // 2, c, 3, 2))
        out.append(('conv', n, side, side, c, c, 3, 1))
    return out


def resnet50(n):
    """ResNet-50 at 112 x 112 (28 x 28 behind the stem and the pool): shortcut, 1x1, 3x3, 1x1 of the first and the later blocks per stage"""
    out, cin, side = [], 64, 28
    for si, cout in enumerate((256, 512, 1024, 2048)):
        s = 2 if si else 1
        so = side // s if side % s == 0 else side // s + 1
        out += [('conv', n, side, side, cin, cout, 1, s), ('conv', n, side, side, cin, cout // 4, 1, 1), ('conv', n, side, side, cout // 4, cout // 4, 3, s),
                ('conv', n, so, so, cout // 4, cout, 1, 1), ('conv', n, so, so, cout, cout // 4, 1, 1), ('conv', n, so, so, cout // 4, cout // 4, 3, 1)]
        cin, side = cout, so
    return out


def shufflenet_v2(n):
    """ShuffleNet-v2 x2 at 112 x 112, channels stored rounded up to 64: every conv the matrix cores see is 1x1 / stride 1"""
    out, cin, side = [], 64, 28
    for c in (128, 256, 512):
        so = side // 2
        out += [('conv', n, side, side, cin, c, 1, 1), ('conv', n, so, so, cin, c, 1, 1), ('conv', n, so, so, c, c, 1, 1)]
        cin, side = c, so
    out.append(('conv', n, 4, 4, 1024, 2048, 1, 1))
    return out


# ---- tags: name -> predicate(case, record) ---------------------------------------------------------------------------------------------
def _mnk_fwd(c):
    _, n, h, w, cin, cout, k, s = c
    return n * _up(h, s) * _up(w, s), cout, k * k * cin


def _rows_of(c, r, ctx, field='fwd'):
    """(M, N, K, RowPlan) of a 'rows' case or of a conv case's forward"""
    if c[0] == 'rows':
        return c[1], c[2], c[3], r['ctx'][ctx]
    return _mnk_fwd(c) + (r['ctx'][ctx][field],)


def _per_cu(M, N):
    return _up(M, 128) * (N // 64) / 256.0


def _sk_refused(c, r, why):
    M, N, K, rp = _rows_of(c, r, 'f32')
    iters = _up(M, 64) * (N // 64) * (K // 32)
    ok = {'per_cu': _per_cu(M, N) > 4.0, 'steps': _per_cu(M, N) <= 4.0 and K % 32 == 0 and iters // 1536 < 12, 'k32': K % 32 != 0}[why]
    return ok and rp[TAIL_MODE] != 3


def _pick(bf16, n128, cand):
    def pred(c, r):
        _, N, _ = _mnk_fwd(c)
        cands = [T128, T128x64, T64] if N % 128 == 0 else [T256x64, T128x64, T64]
        return (N % 128 == 0) == n128 and r['ctx']['bf16' if bf16 else 'f32']['pick'] == cands[cand]
    return pred


def _n16(c):
    return _up(c[1], 128) * (c[2] // (128 if c[2] % 128 == 0 else 64))


def _splits_mirror(tiles, K, mink=256, rmax=3, rmin=1):
    """plan_splits of csrc/conv_plan.h -> (splits, kchunk, [(candidate, efficiency)], clamped)"""
    maxs = max(K // mink, 1)
    lo, hi = max(_up(rmin * 768, tiles), 1), min(_up(rmax * 768, tiles), maxs)
    clamped = lo > hi
    lo = min(lo, hi)
    best, bs, effs = -1.0, 1, []
    for s in range(lo, hi + 1):
        kc = _up(_up(K, s), 32) * 32
        rounds = tiles * _up(K, kc) / 768.0
        eff = rounds / int(rounds + 0.999999)
        effs.append((s, eff))
        if eff > best + 0.02:
            best, bs = eff, s
    kc = _up(_up(K, bs), 32) * 32
    return _up(K, kc), kc, effs, clamped, bs


def _tie(c, r):
    sp, kc, effs, _, bs = _splits_mirror(c[1], c[2])
    top = max(e for _, e in effs)
    return [sp, kc] == r['splits'] and any(s > bs and e == top for s, e in effs) and dict(effs)[bs] < top


def _cls(r, ctx='f32'):
    return r['ctx'][ctx]['cls']


TAGS = {
    # plan_sk
    'sk_fwd': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] == 3 and r['ctx']['f32']['fwd'][MAIN_TILE] == T64,
    'sk_dgrad': lambda c, r: _cls(r)[0][4][TAIL_MODE] == 3 and _cls(r)[0][4][MAIN_TILE] == T128x64,
    'sk_refuse_per_cu': lambda c, r: _sk_refused(c, r, 'per_cu'),
    'sk_refuse_steps': lambda c, r: _sk_refused(c, r, 'steps'),
    'sk_refuse_k32': lambda c, r: _sk_refused(c, r, 'k32'),
    'sk_refuse_ops': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] == 3 and _cls(r)[0][4][TAIL_MODE] != 3,      # FTE_SK_OPS=1
    'sk_w_clipped': lambda c, r: r['ctx']['f32'][TAIL_MODE] == 3 and r['ctx']['f32'][SK_WORKERS] == _up(c[1], 64) * (c[2] // 64) * (c[3] // 32) < 1536,
    # plan_rows
    'tall': lambda c, r: _mnk_fwd(c)[2] >= 576 and r['ctx']['f32']['fwd'][MAIN_TILE] == T128x64 and r['ctx']['f32']['fwd'][TAIL_MODE] == 0,
    'tall_refused_k': lambda c, r: _mnk_fwd(c)[2] < 576 and _up(_mnk_fwd(c)[0], 128) * (_mnk_fwd(c)[1] // 64) >= 4096 and r['ctx']['f32']['fwd'][MAIN_TILE] == T64,
    'bf16_wide_fills': lambda c, r: c[2] % 128 == 0 and _up(c[1], 128) * (c[2] // 128) == 384 and r['ctx']['bf16'][TAIL_TILE] == T128,      # FTE_PLAN16_NOSPLIT=0
    'bf16_wide_below': lambda c, r: c[2] % 128 == 0 and _up(c[1], 128) * (c[2] // 128) == 380 and r['ctx']['bf16'][TAIL_MODE] == 0,      # (no split-K on 128x128 tiles)
    'bf16_narrow_fills': lambda c, r: c[2] == 64 and _up(c[1], 128) == 384 and r['ctx']['bf16'][TAIL_TILE] == T128x64,
    'bf16_narrow_below': lambda c, r: c[2] == 64 and _up(c[1], 128) == 383 and r['ctx']['bf16'][TAIL_MODE] == 2 and r['ctx']['bf16'][TAIL_TILE] == T64,
    'unsplit16_511': lambda c, r: _n16(c) == 511 and r['ctx']['s16'][TAIL_MODE] == 2,      # FTE_PLAN16_NOSPLIT=0: the split plan shows
    'unsplit16_512': lambda c, r: _n16(c) == 512 and r['ctx']['s16'][:4] == [T128, c[1], 512, 0] and r['ctx']['bf16'][TAIL_MODE] == 2,
    'unsplit16_1535': lambda c, r: _n16(c) == 1535 and r['ctx']['s16'][:4] == [T128, c[1], 1535, 0],
    'unsplit16_1536': lambda c, r: _n16(c) == 1536 and r['ctx']['s16'][:4] == [T128, c[1], 1536, 0],
    'one_launch': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] == 0 and r['ctx']['f32']['fwd'][MAIN_TILE] == T64 and r['ctx']['f32']['fwd'][MAIN_MT] * (c[5] // 64) >= SLOTS,
    'tail_split_mode1': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] == 1 and r['ctx']['f32']['fwd'][MAIN_ROWS] < _mnk_fwd(c)[0],      # FTE_TAIL_SPLIT=1
    'nosplit16_taken': lambda c, r: r['ctx']['bf16']['fwd'][TAIL_MODE] == 0 and r['ctx']['bf16']['fwd'][MAIN_TILE] in (T128, T128x64) and r['ctx']['bf16']['fwd'][MAIN_MT] * (c[5] // 64) < SLOTS,
    'nosplit16_not_taken': lambda c, r: r['ctx']['bf16']['pick'] == T64 and r['ctx']['bf16']['fwd'][TAIL_MODE] == 2,
    'split_r_lt256': lambda c, r: _rows_of(c, r, 'f32')[3][TAIL_MODE] == 2 and _rows_of(c, r, 'f32')[3][TAIL_MT] // 4 * (_rows_of(c, r, 'f32')[1] // 64) < 256 and
        _rows_of(c, r, 'f32')[3][TAIL_KCHUNK] < 48 * 32,
    'split_r_ge256': lambda c, r: r['ctx']['f32'][TAIL_MODE] == 2 and r['ctx']['f32'][TAIL_MT] // 4 * (c[2] // 64) >= 256 and r['ctx']['f32'][TAIL_KCHUNK] >= 48 * 32,
    'min_steps_48_vs_32': lambda c, r: c[2] == 64 and ((_up(c[1], 64) == 256 and r['ctx']['f32'][TAIL_MODE] == 0) or (_up(c[1], 64) == 255 and r['ctx']['f32'][TAIL_MODE] == 2)),
    'p_lt2_pick': lambda c, r: c[0] == 'rows' and _up(c[1], 64) * (c[2] // 64) < SLOTS and r['ctx']['f32'][TAIL_MODE] == 0 and r['ctx']['f32'][MAIN_ROWS] == c[1],
    'no_ws': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] >= 2 and r['ctx']['f32']['fwd_nows'][TAIL_MODE] == 0 and r['ctx']['f32']['fwd_nows'][PW_BYTES] == 0,
    'bn_no_split': lambda c, r: r['ctx']['f32']['fwd'][TAIL_MODE] >= 2 and r['ctx']['f32bn']['fwd'][TAIL_MODE] == 0 and r['ctx']['s16bn']['fwd'][TAIL_MODE] == 0,
    'small_only': lambda c, r: c[7] == 2 and all(k[4][MAIN_TILE] == T64 for k in _cls(r, 'bf16')) and r['ctx']['bf16']['pick'] != T64,
    'cls_big': lambda c, r: c[7] == 2 and all(k[4][MAIN_TILE] == T128x64 for k in _cls(r, 'bf16')),      # FTE_DGRAD_CLS_BIG=1
    # pick_tile: candidate 0 / 1 / 2, N % 128 == 0 or not, fp32 / bf16
    'pick_f32_n128_c0': _pick(False, True, 0), 'pick_f32_n128_c1': _pick(False, True, 1), 'pick_f32_n128_c2': _pick(False, True, 2),
    'pick_f32_n64_c0': _pick(False, False, 0), 'pick_f32_n64_c1': _pick(False, False, 1), 'pick_f32_n64_c2': _pick(False, False, 2),
    'pick_bf16_n128_c0': _pick(True, True, 0), 'pick_bf16_n128_c1': _pick(True, True, 1), 'pick_bf16_n128_c2': _pick(True, True, 2),
    'pick_bf16_n64_c0': _pick(True, False, 0), 'pick_bf16_n64_c1': _pick(True, False, 1), 'pick_bf16_n64_c2': _pick(True, False, 2),
    # plan_splits
    'splits_clamped': lambda c, r: _splits_mirror(c[1], c[2])[3] and _splits_mirror(c[1], c[2])[:2] == tuple(r['splits']),
    'splits_tie_fewer': _tie,
    'splits_maxs1': lambda c, r: c[2] // 256 <= 1 and r['splits'][0] == 1,
    # dgrad_classes
    'dg_s1': lambda c, r: c[7] == 1 and [k[0] for k in _cls(r)] == [9],
    'dg_s2_even': lambda c, r: c[7] == 2 and [k[0] for k in _cls(r)] == [4, 2, 2, 1] and len({(k[1], k[2]) for k in _cls(r)}) == 1,
    'dg_s2_odd': lambda c, r: c[7] == 2 and len(_cls(r)) == 4 and len({(k[1], k[2]) for k in _cls(r)}) > 1 and r['ctx']['f32']['merged'][0] == 0,
    'dg_hq0': lambda c, r: c[7] == 2 and len(_cls(r)) < 4,
    'dg_1x1_s2': lambda c, r: c[6] == 1 and c[7] == 2 and [k[0] for k in _cls(r)] == [1, 0, 0, 0] and r['ctx']['f32']['merged'][0] == 0,
    'dg_merge_tiles': lambda c, r: r['ctx']['f32']['merged'][0] == 1 and r['ctx']['f32']['merged'][2] == T64 and r['ctx']['f32']['merged'][3] == [0, 1, 2, 3],
    'dg_split_tiles': lambda c, r: [k[0] for k in _cls(r)] == [4, 2, 2, 1] and r['ctx']['f32']['merged'][:2] == [0, 0],
    'dg_env_merged': lambda c, r: _up(c[1] * _cls(r)[0][1] * _cls(r)[0][2], 64) * (c[4] // 64) >= SLOTS and r['ctx']['f32']['merged'][0] == 1,
    'dg_env_split': lambda c, r: _up(c[1] * _cls(r)[0][1] * _cls(r)[0][2], 64) * (c[4] // 64) < SLOTS and r['ctx']['f32']['merged'][0] == 0,
    'dg_merged16': lambda c, r: r['ctx']['bf16']['merged'][0] == 1 and r['ctx']['bf16']['merged'][2] in (T128, T128x64) and r['ctx']['f32']['merged'][2] == T64,
    # wgrad_plan
    'wg_192': lambda c, r: r['wgrad'][0] == T192,
    'wg_128x128': lambda c, r: r['wgrad'][0] == T128,
    'wg_128x64': lambda c, r: r['wgrad'][0] == T128x64,
    'wg_tiny': lambda c, r: c[6] == 1 and c[4] * c[5] <= 65536 and r['wgrad'][0] == T64,
    'wg_small_shard': lambda c, r: not (c[6] == 1 and c[4] * c[5] <= 65536) and r['wgrad'][0] == T64 and r['wgrad'][1] > 1,
    'wg_big_shard': lambda c, r: r['wgrad'][0] != T64 and r['wgrad'][1] > 1 and r['wgrad'][2] >= 1024,
    'wg_env_tile': lambda c, r: r['wgrad'][0] == T256x64,      # FTE_WGRAD_TILE=1
    'wg_2d_grid': lambda c, r: r['wgrad'][1] > 1 and r['wgrad'][4] == 0,      # FTE_WGRAD_SPLIT_MAJOR=0
    # wino_sized / wino_wanted
    'wino_algo0': lambda c, r: r['sized'][0] == [0, 0, 0] and r['sized'][1] == [1, 1, 1],
    'wino_algo1': lambda c, r: r['sized'][1] == [1, 1, 1] and r['sized'][2] != [1, 1, 1],
    'wino_algo2': lambda c, r: min(c[4], c[5]) >= 128 and r['sized'][2] == [1, 1, 1],
    'wino_c64_ops': lambda c, r: min(c[4], c[5]) == 64 and r['sized'][2] == [1, 0, 1],
    'wino_wgrad_splits0': lambda c, r: r['sized'][1] == [1, 1, 0],
    'wino_refuse_stride': lambda c, r: c[6] == 3 and c[7] == 2 and c[4] % 64 == 0 and r['sized'][1] == [0, 0, 0],
    'wino_refuse_1x1': lambda c, r: c[6] == 1 and c[4] % 64 == 0 and r['sized'][1] == [0, 0, 0],
    'wino_refuse_channels': lambda c, r: c[6] == 3 and c[7] == 1 and c[4] % 64 != 0 and r['sized'][1] == [0, 0, 0],
    'wino_refuse_side': lambda c, r: c[6] == 3 and c[7] == 1 and c[2] < 2 and c[4] % 64 == 0 and r['sized'][1] == [0, 0, 0],
    'wino_ctx_refused': lambda c, r: r['ctx']['f32']['wanted'] == [1, 1, 1] and all(r['ctx'][k]['wanted'] == [0, 0, 0] for k in ('bf16', 's16', 'f32bn', 's16bn')),
    'wino_env_min_c': lambda c, r: min(c[4], c[5]) == 128 and r['sized'][2] == [1, 0, 1],      # FTE_WINO_MIN_C=256
    # the benchmarks' layers
    'net_sphere20': lambda c, r: c[6] == 3, 'net_resnet50': lambda c, r: True, 'net_shufflenet_v2': lambda c, r: c[6] == 1 and c[7] == 1,
}

NOSPLIT0 = {'FTE_PLAN16_NOSPLIT': '0'}
# (case, environment, tags)
CASES = [
    # stream-K: SphereNet's 14x14x256 at 64 images (1.53 tiles per CU) takes it, forward and data gradient
    (('conv', 64, 14, 14, 256, 256, 3, 1), {}, ['sk_fwd', 'sk_dgrad', 'dg_s1', 'wino_algo0', 'wino_algo2', 'wino_ctx_refused', 'no_ws', 'bn_no_split']),
    (('conv', 64, 56, 56, 64, 64, 3, 1), {}, ['sk_refuse_per_cu', 'wino_algo1', 'wino_c64_ops', 'one_launch']),
    (('conv', 64, 14, 14, 128, 128, 1, 1), {}, ['sk_refuse_steps', 'wino_refuse_1x1', 'wg_tiny']),
    (('rows', 12544, 256, 2320, 1, 0, 0), {}, ['sk_refuse_k32']),
    (('conv', 64, 14, 14, 256, 256, 3, 1), {'FTE_SK_OPS': '1'}, ['sk_refuse_ops']),
    (('rows', 64, 64, 64, 1, 0, 0), {'FTE_SK': '2'}, ['sk_w_clipped']),
    # tiles of the row plan
    (('conv', 512, 56, 56, 64, 64, 3, 1), {}, ['tall', 'wg_192']),
    (('conv', 512, 14, 14, 256, 256, 3, 1), {}, ['wg_128x128', 'wg_big_shard']),
    (('conv', 512, 56, 56, 64, 64, 1, 1), {}, ['tall_refused_k']),
    (('rows', 12288, 512, 4608, 1, 0, -1), NOSPLIT0, ['bf16_wide_fills']),
    (('rows', 12160, 512, 4608, 1, 0, -1), NOSPLIT0, ['bf16_wide_below']),
    (('rows', 49152, 64, 4608, 1, 0, -1), NOSPLIT0, ['bf16_narrow_fills']),
    (('rows', 49024, 64, 4608, 1, 0, -1), NOSPLIT0, ['bf16_narrow_below']),
    (('rows', 65408, 128, 4608, 1, 0, -1), NOSPLIT0, ['unsplit16_511']),
    (('rows', 65536, 128, 4608, 1, 0, -1), NOSPLIT0, ['unsplit16_512']),
    (('rows', 196480, 128, 4608, 1, 0, -1), NOSPLIT0, ['unsplit16_1535']),
    (('rows', 196608, 128, 4608, 1, 0, -1), NOSPLIT0, ['unsplit16_1536']),
    (('rows', 65408, 128, 4608, 1, 0, -1), {}, []), (('rows', 65536, 128, 4608, 1, 0, -1), {}, []),
    (('rows', 196480, 128, 4608, 1, 0, -1), {}, []), (('rows', 196608, 128, 4608, 1, 0, -1), {}, []),
    (('rows', 65536, 128, 4608, 1, 0, -1), {'FTE_PLAN_UNSPLIT16': '0'}, []),
    (('conv', 512, 56, 56, 64, 64, 3, 1), {'FTE_TAIL_SPLIT': '1'}, ['tail_split_mode1']),
    (('conv', 64, 7, 7, 512, 512, 3, 1), {}, ['nosplit16_taken']),
    (('conv', 16, 7, 7, 512, 512, 3, 1), {}, ['nosplit16_not_taken', 'split_r_lt256']),
    (('rows', 3136, 512, 4608, 1, 0, -1), {}, ['split_r_ge256']),
    (('rows', 16384, 64, 2048, 1, 0, -1), {}, ['min_steps_48_vs_32', 'p_lt2_pick']),
    (('rows', 16320, 64, 2048, 1, 0, -1), {}, ['min_steps_48_vs_32']),
    (('rows', 3136, 512, 4608, 0, 0, -1), {}, []), (('rows', 3136, 512, 4608, 1, 1, 1), {}, []),
    (('rows', 3136, 512, 4608, 1, 0, -1), {'FTE_MIN_SPLITP': '4'}, []), (('rows', 3136, 512, 4608, 1, 0, -1), {'FTE_SPLIT_MINSTEPS': '16'}, []),
    (('rows', 49152, 128, 1152, 1, 0, 0), {'FTE_WIDE_TILE': '0', 'FTE_NARROW_TILE': '2', 'FTE_FILLS16': '100', 'FTE_PICK_WANT': '100', 'FTE_PICK_WANT16': '500'}, []),
    (('rows', 49152, 64, 1152, 1, 0, 0), {'FTE_WIDE_TILE': '0', 'FTE_NARROW_TILE': '2', 'FTE_FILLS16': '100', 'FTE_PICK_WANT': '100', 'FTE_PICK_WANT16': '500'}, []),
    (('conv', 64, 14, 14, 256, 256, 3, 1), {'FTE_SK_TILE': '0', 'FTE_SK_TILE_DGRAD': '3', 'FTE_SK_MAX_PER_CU': '1.0', 'FTE_SK_MIN_STEPS': '2'}, []),
    (('conv', 32, 14, 14, 256, 256, 3, 1), {'FTE_SK_TILE': '0', 'FTE_SK_TILE_DGRAD': '3', 'FTE_SK_MAX_PER_CU': '1.0', 'FTE_SK_MIN_STEPS': '2'}, []),
    (('conv', 64, 14, 14, 256, 256, 3, 1), {'FTE_SK': '0'}, []),
    (('conv', 512, 56, 56, 64, 128, 3, 2), {}, ['small_only', 'dg_s2_even', 'dg_split_tiles', 'wino_refuse_stride']),
    (('conv', 512, 56, 56, 64, 128, 3, 2), {'FTE_DGRAD_CLS_BIG': '1'}, ['cls_big']),
    # pick_tile: M = n, N = cout
    (('conv', 49152, 1, 1, 64, 128, 1, 1), {}, ['pick_f32_n128_c0']), (('conv', 24576, 1, 1, 64, 128, 1, 1), {}, ['pick_f32_n128_c1']),
    (('conv', 1024, 1, 1, 64, 128, 1, 1), {}, ['pick_f32_n128_c2', 'pick_bf16_n128_c2']),
    (('conv', 98304, 1, 1, 64, 64, 1, 1), {}, ['pick_f32_n64_c0']), (('conv', 49152, 1, 1, 64, 64, 1, 1), {}, ['pick_f32_n64_c1']),
    (('conv', 1024, 1, 1, 64, 64, 1, 1), {}, ['pick_f32_n64_c2', 'pick_bf16_n64_c2']),
    (('conv', 15360, 1, 1, 64, 128, 1, 1), {}, ['pick_bf16_n128_c0']), (('conv', 7680, 1, 1, 64, 128, 1, 1), {}, ['pick_bf16_n128_c1']),
    (('conv', 30720, 1, 1, 64, 64, 1, 1), {}, ['pick_bf16_n64_c0']), (('conv', 15360, 1, 1, 64, 64, 1, 1), {}, ['pick_bf16_n64_c1']),
    # plan_splits
    (('splits', 4, 1024), {}, ['splits_clamped']),
    (('splits', 36, 100352), {}, ['splits_tie_fewer']),
    (('splits', 8, 300), {}, ['splits_maxs1']),
    (('splits', 96, 8192), {'FTE_SPLIT_MINK': '512', 'FTE_SPLIT_ROUNDS': '2', 'FTE_SPLIT_MINROUNDS': '2'}, []),
    (('dense', 512, 512, 25088), {}, []), (('dense', 64, 10624, 512), {}, []), (('dense', 512, 85184, 512), {}, []), (('dense', 8, 64, 64), {}, []),
    # data-gradient classes
    (('conv', 8, 7, 7, 64, 128, 3, 2), {}, ['dg_s2_odd']),
    (('conv', 8, 1, 8, 64, 64, 3, 2), {}, ['dg_hq0']),
    (('conv', 8, 28, 28, 256, 512, 1, 2), {}, ['dg_1x1_s2']),
    (('conv', 8, 28, 28, 128, 256, 3, 2), {}, ['dg_merge_tiles']),
    (('conv', 512, 56, 56, 64, 128, 3, 2), {'FTE_DGRAD_CLASSES': 'merged'}, ['dg_env_merged']),
    (('conv', 8, 28, 28, 128, 256, 3, 2), {'FTE_DGRAD_CLASSES': 'split'}, ['dg_env_split']),
    (('conv', 512, 28, 28, 128, 256, 3, 2), {'FTE_DGRAD_MERGED16': '1'}, ['dg_merged16']),
    (('conv', 512, 56, 56, 64, 128, 3, 2), {'FTE_DGRAD_MERGED16': '1'}, []),
    # filter gradient
    (('conv', 512, 28, 28, 128, 64, 3, 1), {}, ['wg_128x64']),
    (('conv', 8, 14, 14, 256, 256, 3, 1), {}, ['wg_small_shard']),
    (('conv', 64, 14, 14, 256, 256, 3, 1), {'FTE_WGRAD_TILE': '1'}, ['wg_env_tile']),
    (('conv', 64, 14, 14, 256, 256, 3, 1), {'FTE_WGRAD_SPLIT_MAJOR': '0'}, ['wg_2d_grid']),
    # Winograd rule
    (('conv', 8, 14, 14, 192, 64, 3, 1), {}, ['wino_wgrad_splits0']),
    (('conv', 8, 14, 14, 96, 64, 3, 1), {}, ['wino_refuse_channels']),
    (('conv', 8, 1, 14, 64, 64, 3, 1), {}, ['wino_refuse_side']),
    (('conv', 8, 15, 13, 128, 128, 3, 1), {}, []),
    (('conv', 64, 28, 28, 128, 128, 3, 1), {'FTE_WINO_MIN_C': '256'}, ['wino_env_min_c']),
    (('conv', 64, 28, 28, 128, 128, 3, 1), {'FTE_WINO_OPS': '3', 'FTE_WINO_OPS64': '2'}, []),
    (('conv', 64, 56, 56, 64, 64, 3, 1), {'FTE_WINO_OPS': '3', 'FTE_WINO_OPS64': '2'}, []),
]
for _n in (64, 128, 512):
    CASES += [(c, {}, ['net_sphere20']) for c in sphere20(_n)] + [(c, {}, ['net_resnet50']) for c in resnet50(_n)] + \
             [(c, {}, ['net_shufflenet_v2']) for c in shufflenet_v2(_n)]


def env_key(env):
    return ' '.join('%s=%s' % kv for kv in sorted(env.items()))


def by_environment():
    """{environment key: (environment, [cases in table order, each once])}"""
    out = {}
    for case, env, _ in CASES:
        cases = out.setdefault(env_key(env), (env, []))[1]
        if case not in cases:
            cases.append(case)
    return out


def case_line(case):
    return ' '.join(str(v) for v in case)
