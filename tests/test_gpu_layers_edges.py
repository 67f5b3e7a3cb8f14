"""-m gpu: the BN-net layer kernels of csrc/layers.hip (batch norm, pooling, dropout, stem im2col, grouped 3x3, depthwise 3x3,
channel scale, channel gather) through the C ABI at the shapes their host launchers branch on.  References are float64 numpy
(oracle.ops) on the float32-rounded (for bf16 storage: bf16-exact) inputs; the *_s16 twins are held to the convention of
test_gpu_bf16_storage.py: on bf16-exact inputs a stored bf16 tensor is the rounding of the fp32 entry point's result bit for bit
and an fp32 result is bit-identical.  Tolerances are the project's (util_gpu.TOL_MAXABS / TOL_RELL2, 1e-6 mean, 2e-6 rstd, half a
bf16 step where a value is stored as bf16); where a bound is this file's own the reasoning stands next to it.  Every output buffer
is poisoned with NaN and followed by a canary that must come back bit for bit; inputs must come back unchanged.  The launch
profiler does not record these kernels: each case relies on the launcher condition as written in layers.hip and asserts, with a
host mirror of that condition, which side it is on.

Launcher conditions (layers.hip) -> case below / case above, or what the 64 MB per-tensor limit leaves out:

  stat_split: splits = min(2048 / cb, rows / (lanes * 8), BN_MAX_SPLITS = 512), >= 1
                                         BN_PLAN rows with 1 split / with 16, 17, 33 and 512 splits, every quads_per_block class
  quads_per_block 0 / 8 / 16 / 32 / 64   C = 8, 28 / 32, 48 / 64, 116 / 128, 244 / 256, 488 (second of each: ragged last block)
  rows % rps != 0 (short last split)     the 17- and 33-split rows
  TAIL_GROUP = 16 (FTE_BN_TAIL=1)        16 splits (one full group), 17 (a group of one), 33 (two full groups and one)
  l_bn_finalize / l_bn_bwd_finalize: splits > fin_wide_from() (512) -> the wide kernels
                                         NOT reachable from the BN entry points by default: stat_split never gives more than
                                         BN_MAX_SPLITS = 512 splits and the comparison is strict.  The child run with
                                         FTE_BN_FIN_WIDE=16 puts the 17-, 33- and 512-split cases on the wide kernels and the 1-
                                         and 16-split cases on the narrow ones.  With at most 512 splits the wide kernels' rows u = 2, 3
                                         of a trip (splits 512 ..) and their second `s0 += 1024` trip never run: only the conv
                                         epilogues of the BN-fusion path leave that many partial rows
  grid_for_c cap 512 (fp32) / 1024 (bf16), from n4 >= 4 * cap * 256
                                         test_bn_apply_second_grid_trip: n4 just below / at the threshold, m = 1 and m = 29
  l_relu_bwd cap 512 / 1024, same rule   test_relu_bwd_second_grid_trip: n / 4 = 4 * cap * 256 - 1 / = 4 * cap * 256
  l_act_* cap 4096 blocks                n = 4096 * 256 / 4096 * 256 + 3
  grid_for cap 8192: gap_bwd             2 x 4095 x 256 / 2 x 4099 x 256
                     maxpool fwd         4090 x 1 x 3 x 1024 / 4100 x 1 x 3 x 1024
                     maxpool bwd general 2700 x 1 x 3 x 1024 / 4100 x 1 x 3 x 1024
                     maxpool bwd even    2 x 8 x 6 x 8 / left out: above the cap the input has 33.6 M elements, 134 MB (67 MB as bf16)
                     dropout fwd / bwd   test_dropout: n = 8192 * 256 + 259 (above); test_gpu_layers.py is below
                     im2col generic      test_stem_im2col_forms / test_stem_im2col_generic_second_grid_trip: 50 176 rows x 48 quads
  gconv_launch gw 4 / 8 / 16 / 32, GPBK = 1 when groups % 32 / % 16 / % 4 != 0
                                         (c, groups) = (32, 8), (64, 8), (32, 2), (64, 2) / (128, 32), (128, 16), (64, 4)
  gconv_launch 8192-block cap            left out: needs n * h * ceil(w / 4) > 8192 * 256 / ((gw / 4) * GPBK) units, >= 134 MB at c = 128
  l_gconv_wgrad groups < gpb             (32, 8): used = 24 threads, (64, 8), (32, 2), (128, 32): 96, (128, 16), (64, 4): 192 / (64, 2): groups >= gpb
  l_gconv_wgrad_chunks 96 MiB cap        left out: the partial buffer itself is 96 MiB
  gconv16_blocks cap 512 / (c / 32), per launch (forward: n h w at stride 1, the output grid at stride 2; data gradient: n h w)
                     forward stride 1    (2, 56, 56, 128), (4, 7, 7, 1024) / (6, 56, 56, 128), (48, 7, 7, 1024)
                     forward stride 2    the same and (6, 56, 56, 128), (48, 7, 7, 1024) / (24, 56, 56, 128), (48, 14, 14, 1024)
                     data gradient       (2, 56, 56, 128), (4, 7, 7, 1024) / (6, 56, 56, 128), (48, 7, 7, 1024), both strides
  l_gconv_wgrad16_chunks                 (1, 9, 7, 128), (4, 7, 7, 1024): 1 chunk / the others: several
  dw_quads 16 / 32 / 64                  c = 64, 116 / 244 / 488, 1024
  l_dwconv_wgrad_splits clamps           < 1 -> 1: the small sizes; npix clamp: (3, 7, 9); 1024: (5, 128, 128, 64); 2048 / cb: (2, 80, 64, 1024)
  dwconv dgrad stride 2 quads            (1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 7, 9), (2, 8, 6)
  dwconv dgrad stride 2 grid_for_c cap 1024, from total >= 4 * 1024 * 256 units (a thread keeps its weight quad across trips)
                                         (17189, 1, 3, 244) / (17190, 1, 3, 244), m = 61
  depthwise / gather 16 384-block caps   left out: need 16384 * 256 quads = 67 MB per tensor
  chscale_grid gx rounded up to m        c = 256 (m = 1) / c = 244 (m = 61), 116 (m = 29); want = 1 at n = 1030; 1 and several pieces
  gather_lds (six conditions)            test_channel_gather_lds_conditions: one LDS-form shape and five variants failing one each
  gather_lds groups > cap (2048)         rows = 2048 * rg + 5
  l_im2col_first rows form               (7, 3, kpad 160), w = 9, 13 and 1024 (several PX = 14 trips, 86 KB of LDS) / kpad 192, w = 1030,
                                         cin = 1, ks = 5"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ops

from test_gpu_arena_edges import CANARY, _f32, _guarded, _intact

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, host, stream, ws, check_maxabs, check_rell2, TOL_MAXABS, TOL_RELL2

EINVAL = -1
CANARY16 = CANARY.view(np.int16)
BF16_HALF_STEP = 2.0 ** -8          # half a bf16 step relative to the value (8 significant bits)
ULP = 2.0 ** -23


def _source_constant(name, pattern):
    """a constant as csrc/ states it today: the host mirrors below follow the sources, they do not copy them"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tf_face_toolbox_amd', 'csrc')
    m = re.search(pattern, open(os.path.join(csrc, name)).read())
    assert m, (name, pattern)
    return int(m.group(1))


BN_MAX_SPLITS = _source_constant('layers.h', r'constexpr int BN_MAX_SPLITS = (\d+);')
TAIL_GROUP = _source_constant('layers.hip', r'constexpr int TAIL_GROUP = (\d+);')
FIN_WIDE_FROM = _source_constant('layers.hip', r'getenv\("FTE_BN_FIN_WIDE"\)\) : (\d+);')         # fin_wide_from()'s default


# ------------------------------------------------------------------------------------------------------------------------
# buffers: NaN-poisoned outputs with a canary behind them
# ------------------------------------------------------------------------------------------------------------------------
def _out(n):
    return _guarded(np.full(int(n), np.nan, np.float32))


def _out16(n):
    """int16 (bf16) output of n elements, poisoned with a bf16 NaN, followed by the canary's 16 half-words"""
    return torch.tensor(np.concatenate([np.full(int(n), 0x7FC1, np.int16), CANARY16]), device='cuda')


def _in16(a):
    """bf16-exact float array -> guarded device int16"""
    b = (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16).ravel()
    return torch.tensor(np.concatenate([b, CANARY16]), device='cuda')


def _intact16(t, n):
    return np.array_equal(t[n:].cpu().numpy(), CANARY16)


def _u8out(n):
    return torch.tensor(np.concatenate([np.full(int(n), 0xEE, np.uint8), CANARY.view(np.uint8)]), device='cuda')


def _intact8(t, n):
    return np.array_equal(t[n:].cpu().numpy(), CANARY.view(np.uint8))


def _bits16(t32):
    """device fp32 -> its bf16 rounding as int16 (torch: round to nearest even)"""
    return t32.bfloat16().view(torch.int16)


def _f16(t16):
    return t16.view(torch.bfloat16).float()


def _b16(a):
    return ops.bf16_round(_f32(a))


def _unchanged(t, a):
    n = a.size
    return np.array_equal(t[:n].cpu().numpy().view(np.uint32), np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)) and _intact(t, n)


def _unchanged16(t, n, before):
    return torch.equal(t, before) and _intact16(t, n)


def _stored16(got16, ref, what):
    """a value stored as bf16: within half a bf16 step of the float64 reference, plus the fp32 path's own TOL_MAXABS"""
    got = host(_f16(got16)).reshape(ref.shape)
    assert np.isfinite(got).all(), what
    lim = np.abs(ref) * BF16_HALF_STEP + TOL_MAXABS * max(np.abs(ref).max(), 1e-30)
    assert (np.abs(got - ref) <= lim).all(), (what, float((np.abs(got - ref) / lim).max()))


# ------------------------------------------------------------------------------------------------------------------------
# 1. BN forward / backward split plan
# ------------------------------------------------------------------------------------------------------------------------
def _quads_per_block(c):
    return 0 if c % 4 else (64 if c >= 256 else 32 if c >= 128 else 16 if c >= 64 else 8 if c >= 32 else 0)


def _stat_split(rows, c):
    """host mirror of stat_split (layers.hip): (splits, rows per split)"""
    q = _quads_per_block(c)
    cb = (c // 4 + q - 1) // q if q else (c + 63) // 64
    lanes = 256 // q if q else 4
    rs = max(1, min(2048 // cb, rows // (lanes * 8), BN_MAX_SPLITS))
    rps = (rows + rs - 1) // rs
    return (rows + rps - 1) // rps, rps


# (rows, C, splits): every quads_per_block class with 1 split; 16 / 17 / 33 splits (TAIL_GROUP: a full group, a group of one, two full
# groups and one; the 17- and 33-split rows leave the last split short) in the scalar layout, a full vector class and a ragged one;
# BN_MAX_SPLITS = 512 splits exactly -- at the clamp (520 * 256 rows would give more without it) -- in both layouts and ragged
BN_PLAN = [(37, 8, 1), (50, 28, 1), (100, 32, 1), (77, 64, 1), (60, 128, 1), (31, 256, 1),
           (100, 48, 1), (77, 116, 1), (60, 244, 1), (31, 488, 1),
           (512, 28, 16), (547, 28, 17), (1061, 28, 33),
           (4096, 32, 16), (4357, 32, 17), (8455, 32, 33),
           (1024, 244, 16), (1091, 244, 17), (2117, 244, 33),
           (2179, 116, 17), (547, 488, 17), (2183, 64, 17), (1061, 256, 33),
           (16384, 8, 512), (512 * 256, 32, 512), (520 * 256, 32, 512), (16384, 256, 512), (16384, 488, 512)]


def _last_block_channels(c):
    q = _quads_per_block(c)
    w = 4 * q if q else 64
    return slice((c - 1) // w * w, c)


def _per_channel(got, ref, terms, maxterm, what, sl):
    """the last channel block on its own.  A sum of `terms` fp32 terms in any order: ulp * sqrt(terms) * max|term| of accumulated
    rounding (each partial sum is of the order sqrt(terms) * |term|), next to the project's relative tolerance on the value itself"""
    err = np.abs(np.asarray(got, np.float64)[sl] - ref[sl])
    bound = TOL_RELL2 * np.abs(ref[sl]) + ULP * math.sqrt(terms) * maxterm
    assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize('rows,c,splits', BN_PLAN)
def test_bn_split_plan(rows, c, splits):
    """stat_split / quads_per_block: see BN_PLAN.  fte_bn_train_fwd (residual + ReLU, moving statistics), fte_bn_train_stats,
    fte_bn_train_bwd, _bwd_res, _bwd_zmask against float64; the _s16 twins with flags 1, 2, 3 against the fp32 entry points."""
    assert _stat_split(rows, c)[0] == splits
    assert splits <= BN_MAX_SPLITS <= FIN_WIDE_FROM, 'the wide finalize kernels (splits > fin_wide_from()) are now reachable by default: add cases'
    assert (TAIL_GROUP, BN_MAX_SPLITS) == (16, 512), 'BN_PLAN was laid out for groups of 16 splits and at most 512 of them'
    rps = _stat_split(rows, c)[1]
    r = np.random.default_rng(rows * 1000 + c)
    s16 = c >= 32
    rd = _b16 if s16 else _f32                              # bf16-exact inputs where the twins run: both paths read the same values
    z = rd(r.standard_normal((rows, c)) * 2.0 + 3.0); res = rd(r.standard_normal((rows, c))); dy = rd(r.standard_normal((rows, c)))
    gamma = _f32(1 + 0.2 * r.standard_normal(c)); beta = _f32(0.3 * r.standard_normal(c))
    mm = _f32(r.standard_normal(c) * 0.1); mv = _f32(1 + 0.1 * r.random(c))
    z64, res64, dy64, g64, b64 = [a.astype(np.float64) for a in (z, res, dy, gamma, beta)]
    bn_ref, cache = ops.bn_train_fwd(z64, g64, b64)
    y_ref = np.maximum(bn_ref + res64, 0)
    mm_ref, mv_ref = ops.bn_moving_update(mm.astype(np.float64), mv.astype(np.float64), cache['mean'], cache['var'], rows)
    n = rows * c
    zd, resd, dyd, gd, bd = _guarded(z), _guarded(res), _guarded(dy), _guarded(gamma), _guarded(beta)
    y = _out(n); mean, rstd, scale, shift = _out(c), _out(c), _out(c), _out(c)
    mmd, mvd = _guarded(mm), _guarded(mv)
    wsb, nb = ws(query('fte_bn_ws_bytes', c))
    st = stream()
    call('fte_bn_train_fwd', zd, gd, bd, resd, y, mean, rstd, scale, shift, mmd, mvd, rows, c, 1e-3, 0.999, 1, wsb, nb, st)
    torch.cuda.synchronize()
    last = _last_block_channels(c)
    tail_rows = slice((splits - 1) * rps, rows)               # the last (possibly short) split
    check_maxabs(host(mean)[:c], cache['mean'], 1e-6, 'mean'); check_maxabs(host(rstd)[:c], cache['rstd'], 2e-6, 'rstd')
    check_maxabs(host(mean)[:c][last], cache['mean'][last], 1e-6, 'mean, last block'); check_maxabs(host(rstd)[:c][last], cache['rstd'][last], 2e-6, 'rstd, last block')
    sc_ref = g64 * cache['rstd']
    check_maxabs(host(scale)[:c], sc_ref, 2e-6, 'scale'); check_maxabs(host(shift)[:c], b64 - cache['mean'] * sc_ref, TOL_MAXABS, 'shift')
    check_maxabs(host(mmd)[:c], mm_ref, 1e-6, 'moving mean'); check_maxabs(host(mvd)[:c], mv_ref, 1e-6, 'moving var')
    yh = host(y)[:n].reshape(rows, c)
    check_maxabs(yh, y_ref, TOL_MAXABS, 'y'); check_maxabs(yh[tail_rows], y_ref[tail_rows], TOL_MAXABS, 'y, last split')
    check_maxabs(yh[:, last], y_ref[:, last], TOL_MAXABS, 'y, last block')
    # statistics alone: the same launches, the same bits
    m2, r2, s2, f2 = _out(c), _out(c), _out(c), _out(c)
    call('fte_bn_train_stats', zd, gd, bd, m2, r2, s2, f2, None, None, rows, c, 1e-3, 0.999, wsb, nb, st)
    assert torch.equal(m2, mean) and torch.equal(r2, rstd) and torch.equal(s2, scale) and torch.equal(f2, shift)
    # backward through relu(bn + res)
    g_ref = dy64 * (y_ref > 0)
    dz_ref, dg_ref, db_ref = ops.bn_train_bwd(g_ref, g64, cache)
    dz, dg, db = _out(n), _out(c), _out(c)
    call('fte_bn_train_bwd', dyd, y, zd, gd, mean, rstd, dz, dg, db, rows, c, wsb, nb, st)
    torch.cuda.synchronize()
    dzh = host(dz)[:n].reshape(rows, c)
    check_maxabs(dzh, dz_ref, TOL_MAXABS, 'dz'); check_maxabs(dzh[tail_rows], dz_ref[tail_rows], TOL_MAXABS, 'dz, last split')
    check_maxabs(dzh[:, last], dz_ref[:, last], TOL_MAXABS, 'dz, last block')
    check_rell2(host(dg)[:c], dg_ref, TOL_RELL2, 'dgamma'); check_rell2(host(db)[:c], db_ref, TOL_RELL2, 'dbeta')
    _per_channel(host(dg)[:c], dg_ref, rows, np.abs(g_ref * cache['xhat']).max(), 'dgamma, last block', last)
    _per_channel(host(db)[:c], db_ref, rows, np.abs(g_ref).max(), 'dbeta, last block', last)
    g1, dz1, dg1, db1 = _out(n), _out(n), _out(c), _out(c)
    call('fte_bn_train_bwd_res', dyd, y, zd, gd, mean, rstd, g1, dz1, dg1, db1, rows, c, wsb, nb, st)
    assert torch.equal(dz1, dz) and torch.equal(dg1, dg) and torch.equal(db1, db)
    assert np.array_equal(g1[:n].cpu().numpy().reshape(rows, c), (dy * (yh > 0)).astype(np.float32))
    # the mask recomputed from z is the forward's bit for bit (fte.h): forward without a residual, then both backward forms
    y2 = _out(n)
    call('fte_bn_train_fwd', zd, gd, bd, None, y2, mean, rstd, scale, shift, None, None, rows, c, 1e-3, 0.999, 1, wsb, nb, st)
    assert torch.equal(m2, mean) and torch.equal(f2, shift)
    check_maxabs(host(y2)[:n].reshape(rows, c), np.maximum(bn_ref, 0), TOL_MAXABS, 'relu(bn)')
    dz2, dg2, db2 = _out(n), _out(c), _out(c); dz3, dg3, db3 = _out(n), _out(c), _out(c)
    call('fte_bn_train_bwd', dyd, y2, zd, gd, mean, rstd, dz2, dg2, db2, rows, c, wsb, nb, st)
    call('fte_bn_train_bwd_zmask', dyd, zd, gd, mean, rstd, scale, shift, dz3, dg3, db3, rows, c, wsb, nb, st)
    assert torch.equal(dz3, dz2) and torch.equal(dg3, dg2) and torch.equal(db3, db2)
    bufs = [(y, n), (y2, n), (dz, n), (dz1, n), (dz2, n), (dz3, n), (g1, n)] + [(t, c) for t in (mean, rstd, scale, shift, mmd, mvd, m2, r2, s2, f2, dg, db, dg1, db1, dg2, db2, dg3, db3)]
    assert all(_intact(t, k) for t, k in bufs)
    assert _unchanged(zd, z) and _unchanged(resd, res) and _unchanged(dyd, dy) and _unchanged(gd, gamma) and _unchanged(bd, beta)
    if not s16:
        return
    # bf16 storage twins: flags bit 0 = z / dz, bit 1 = y / res / dy / g.  Same kernels, same arithmetic: the statistics and sums are
    # bit-identical to the fp32 entry points', a stored tensor is their result's rounding
    z16, res16, dy16 = _in16(z), _in16(res), _in16(dy)
    z16_0, res16_0, dy16_0 = z16.clone(), res16.clone(), dy16.clone()
    call('fte_bn_train_fwd', zd, gd, bd, resd, y, mean, rstd, scale, shift, None, None, rows, c, 1e-3, 0.999, 1, wsb, nb, st)
    for flags in (1, 2, 3):
        zh, ah = flags & 1, flags & 2
        zin = z16 if zh else zd
        ys = _out16(n) if ah else _out(n)
        ms, rs_, ss, fs = _out(c), _out(c), _out(c), _out(c)
        mm1, mv1 = _guarded(mm), _guarded(mv)
        call('fte_bn_train_fwd_s16', zin, gd, bd, res16 if ah else resd, ys, ms, rs_, ss, fs, mm1, mv1, rows, c, 1e-3, 0.999, 1, flags, wsb, nb, st)
        assert torch.equal(ms, mean) and torch.equal(rs_, rstd) and torch.equal(ss, scale) and torch.equal(fs, shift), flags
        assert torch.equal(mm1, mmd) and torch.equal(mv1, mvd), flags
        assert torch.equal(ys[:n], _bits16(y[:n])) if ah else torch.equal(ys, y), flags
        m3, r3, s3, f3 = _out(c), _out(c), _out(c), _out(c)
        call('fte_bn_train_stats_s16', zin, gd, bd, m3, r3, s3, f3, None, None, rows, c, 1e-3, 0.999, flags & 1, wsb, nb, st)
        assert torch.equal(m3, mean) and torch.equal(r3, rstd) and torch.equal(s3, scale) and torch.equal(f3, shift), flags
        # residual backward on the STORED y (for flags & 2 its rounding: the same mask, rounding keeps the sign and zero)
        gs = _out16(n) if ah else _out(n); dzs = _out16(n) if zh else _out(n); dgs, dbs = _out(c), _out(c)
        call('fte_bn_train_bwd_s16', dy16 if ah else dyd, ys, zin, gd, mean, rstd, None, None, gs, dzs, dgs, dbs, rows, c, flags, wsb, nb, st)
        assert torch.equal(dgs, dg) and torch.equal(dbs, db), flags
        assert torch.equal(gs[:n], _bits16(g1[:n])) if ah else torch.equal(gs, g1), flags
        assert torch.equal(dzs[:n], _bits16(dz[:n])) if zh else torch.equal(dzs, dz), flags
        dzs2 = _out16(n) if zh else _out(n)
        call('fte_bn_train_bwd_s16', dy16 if ah else dyd, None, zin, gd, mean, rstd, s2, f2, None, dzs2, dgs, dbs, rows, c, flags, wsb, nb, st)
        assert torch.equal(dgs, dg3) and torch.equal(dbs, db3), flags
        assert torch.equal(dzs2[:n], _bits16(dz3[:n])) if zh else torch.equal(dzs2, dz3), flags
        for t, half in ((ys, ah), (gs, ah), (dzs, zh), (dzs2, zh)):
            assert _intact16(t, n) if half else _intact(t, n), flags
        assert all(_intact(t, c) for t in (ms, rs_, ss, fs, mm1, mv1, m3, r3, s3, f3, dgs, dbs))
    assert _unchanged16(z16, n, z16_0) and _unchanged16(res16, n, res16_0) and _unchanged16(dy16, n, dy16_0)


@pytest.mark.parametrize('env', [{'FTE_BN_TAIL': '1'}, {'FTE_BN_FIN_WIDE': '16'}], ids=['in_launch_finalize', 'wide_finalize_from_17_splits'])
def test_bn_split_plan_with_the_other_finalize_paths(env):
    """FTE_BN_TAIL=1: the splits are merged inside the producing launch in groups of TAIL_GROUP = 16 (16 / 17 / 33 splits: a full
    group, a group of one, two full groups and one; the scalar layouts keep the second launch).  FTE_BN_FIN_WIDE=16:
    bn_finalize_wide_kernel / bn_bwd_finalize_wide_kernel from 17 splits on -- with the default threshold (splits > 512) the BN entry
    points never reach them, stat_split stops at BN_MAX_SPLITS = 512.  Both hooks are read once per process: the cases of
    test_bn_split_plan re-run in a fresh child, same oracle, same tolerances."""
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-k', 'test_bn_split_plan and not other_finalize',
                        '-p', 'no:cacheprovider'], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and '%d passed' % len(BN_PLAN) in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------------
# 2. second grid trip
# ------------------------------------------------------------------------------------------------------------------------
def _grid_for(n):
    return max(1, min(8192, (n + 255) // 256))


def _grid_for_c(n4, c, wide):
    q = c // 4
    m = q // math.gcd(q, 256)
    blocks, cap = _grid_for(n4), 512 if wide else 1024
    if blocks > cap and n4 >= 4 * cap * 256:
        blocks = cap
    return (blocks + m - 1) // m * m


@pytest.mark.parametrize('above', [False, True])
@pytest.mark.parametrize('c,flags', [(64, 0), (116, 0), (64, 3), (116, 3)])
def test_bn_apply_second_grid_trip(c, flags, above):
    """grid_for_c (fte_bn_apply, fte_bn_bwd_apply): the grid is capped at 512 (fp32) / 1024 (bf16) blocks once n4 = rows * c / 4 >=
    4 * cap * 256 and each thread then walks at least four 16-byte pieces; one piece below that.  c = 116: blocks rounded up to a
    multiple of m = 29.  The pieces past the first trip are checked on their own."""
    cap = 1024 if flags else 512
    rows = -(-4 * cap * 256 * 4 // c) - (0 if above else 1)
    n4 = rows * c // 4
    blocks = _grid_for_c(n4, c, not flags)
    assert (n4 >= 4 * cap * 256) == above and (blocks * 256 < n4) == above and blocks % (c // 4 // math.gcd(c // 4, 256)) == 0
    first = blocks * 256 * 4 // c if above else rows - 1      # rows wholly past the first trip (below the cap: the last row)
    first = min(first + 1, rows - 1)
    r = np.random.default_rng(c + flags + above)
    rd = _b16 if flags else _f32
    z = rd(r.standard_normal((rows, c))); res = rd(r.standard_normal((rows, c))); g = rd(r.standard_normal((rows, c)))
    scale = _f32(1 + 0.2 * r.standard_normal(c)); shift = _f32(0.3 * r.standard_normal(c)); coef = _f32(r.standard_normal(3 * c))
    z64, res64, g64, c64 = z.astype(np.float64), res.astype(np.float64), g.astype(np.float64), coef.astype(np.float64)
    y_ref = np.maximum(z64 * scale.astype(np.float64) + shift.astype(np.float64) + res64, 0)
    dz_ref = c64[:c] * g64 + c64[c:2 * c] * z64 + c64[2 * c:]
    n = rows * c
    sd, fd, cd = _guarded(scale), _guarded(shift), _guarded(coef)
    st = stream()
    if flags:
        zd, rsd, gd_ = _in16(z), _in16(res), _in16(g)
        before = [t.clone() for t in (zd, rsd, gd_)]
        y, dz = _out16(n), _out16(n)
    else:
        zd, rsd, gd_ = _guarded(z), _guarded(res), _guarded(g)
        y, dz = _out(n), _out(n)
    call('fte_bn_apply', zd, sd, fd, rsd, y, rows, c, 1, flags, st)
    call('fte_bn_bwd_apply', gd_, zd, cd, dz, rows, c, flags, st)
    torch.cuda.synchronize()
    if flags:
        _stored16(y[:n], y_ref, 'y'); _stored16(y[:n].view(rows, c)[first:], y_ref[first:], 'y, second trip')
        _stored16(dz[:n], dz_ref, 'dz'); _stored16(dz[:n].view(rows, c)[first:], dz_ref[first:], 'dz, second trip')
        assert _intact16(y, n) and _intact16(dz, n) and all(_unchanged16(t, n, b) for t, b in zip((zd, rsd, gd_), before))
    else:
        yh, dzh = host(y)[:n].reshape(rows, c), host(dz)[:n].reshape(rows, c)
        check_maxabs(yh, y_ref, TOL_MAXABS, 'y'); check_maxabs(yh[first:], y_ref[first:], TOL_MAXABS, 'y, second trip')
        check_maxabs(dzh, dz_ref, TOL_MAXABS, 'dz'); check_maxabs(dzh[first:], dz_ref[first:], TOL_MAXABS, 'dz, second trip')
        assert _intact(y, n) and _intact(dz, n) and _unchanged(zd, z) and _unchanged(rsd, res) and _unchanged(gd_, g)
    assert _unchanged(sd, scale) and _unchanged(fd, shift) and _unchanged(cd, coef)


@pytest.mark.parametrize('above', [False, True])
@pytest.mark.parametrize('half', [False, True])
def test_relu_bwd_second_grid_trip(half, above):
    """l_relu_bwd: 512 (fp32) / 1024 (bf16) blocks once n / 4 >= 4 * cap * 256 (the rule is on 16-byte pieces: n = 16 * cap * 256
    elements); four elements fewer and every thread takes one piece.  g = dy * (y > 0) is exact."""
    cap = 1024 if half else 512
    n = 16 * cap * 256 - (0 if above else 4)
    r = np.random.default_rng(n)
    dy = _b16(r.standard_normal(n)); y = _b16(np.maximum(r.standard_normal(n), 0))
    y[-4:] = [0.0, 1.5, 0.0, 2.0]
    ref = np.where(y > 0, dy, np.float32(0)).astype(np.float32)
    trip = cap * 256 * 4 if above else n - 4
    assert (y[trip:] > 0).any() and (y[trip:] == 0).any()
    if half:
        dyd, yd, g = _in16(dy), _in16(y), _out16(n)
        b0, b1 = dyd.clone(), yd.clone()
        call('fte_relu_bwd_s16', dyd, yd, g, n, stream())
        got = g[:n].cpu().numpy()
        want = _in16(ref)[:n].cpu().numpy()
        assert np.array_equal(got[trip:], want[trip:]), 'second trip'
        assert np.array_equal(got, want) and _intact16(g, n) and _unchanged16(dyd, n, b0) and _unchanged16(yd, n, b1)
    else:
        dyd, yd, g = _guarded(dy), _guarded(y), _out(n)
        call('fte_relu_bwd', dyd, yd, g, n, stream())
        got = g[:n].cpu().numpy()
        assert np.array_equal(got[trip:].view(np.uint32), ref[trip:].view(np.uint32)), 'second trip'
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and _intact(g, n) and _unchanged(dyd, dy) and _unchanged(yd, y)


@pytest.mark.parametrize('n', [4096 * 256, 4096 * 256 + 3])
@pytest.mark.parametrize('kind', [0, 1])
def test_act_second_grid_trip(n, kind):
    """l_act_fwd / l_act_bwd: at most 4096 blocks of 256 threads, one element per thread and trip: n = 4096 * 256 fills the first trip
    exactly, three more elements take the second.  The tolerances of test_se_gate_pieces."""
    r = np.random.default_rng(n + kind)
    v = _f32(r.standard_normal(n) * 3); d = _f32(r.standard_normal(n))
    v64, d64 = v.astype(np.float64), d.astype(np.float64)
    f = np.maximum(v64, 0) if kind == 0 else 1 / (1 + np.exp(-v64))
    vd, dd = _guarded(v), _guarded(d)
    o, dx = _out(n), _out(n)
    call('fte_act_fwd', vd, o, n, kind, stream())
    call('fte_act_bwd', dd, o, dx, n, kind, stream())
    torch.cuda.synchronize()
    oh = host(o)[:n]
    df = (oh > 0).astype(np.float64) if kind == 0 else oh * (1 - oh)        # the derivative from the OUTPUT, as the entry point takes it
    check_maxabs(oh, f, 1e-6, 'act fwd'); check_maxabs(host(dx)[:n], d64 * df, 1e-5, 'act bwd')
    t = slice(n - 3, n)
    check_maxabs(oh[t], f[t], 1e-6, 'act fwd, last three'); check_maxabs(host(dx)[:n][t], (d64 * df)[t], 1e-5, 'act bwd, last three')
    assert _intact(o, n) and _intact(dx, n) and _unchanged(vd, v) and _unchanged(dd, d)


@pytest.mark.parametrize('hw', [4095, 4099])
def test_gap_bwd_second_grid_trip(hw):
    """l_gap_bwd: grid_for(n * hw * c) -- 8192 blocks x 256 elements per trip: 2 x 4095 x 256 is below, 2 x 4099 x 256 above.  1e-6 as in
    test_maxpool_gap_dropout; the bf16 twin stores the rounding of the same quotient."""
    nimg, c = 2, 256
    total = nimg * hw * c
    assert (total > 8192 * 256) == (hw == 4099)
    r = np.random.default_rng(hw)
    dg = _f32(r.standard_normal((nimg, c)))
    ref = ops.gap_bwd(dg.astype(np.float64), (nimg, hw, 1, c)).reshape(-1)
    dgd, dx, dx16 = _guarded(dg), _out(total), _out16(total)
    call('fte_gap_bwd', dgd, dx, nimg, hw, c, stream())
    call('fte_gap_bwd_s16', dgd, dx16, nimg, hw, c, stream())
    torch.cuda.synchronize()
    trip = min(8192 * 256, total - 256)
    check_maxabs(host(dx)[:total], ref, 1e-6, 'gap bwd'); check_maxabs(host(dx)[trip:total], ref[trip:], 1e-6, 'gap bwd, second trip')
    assert torch.equal(dx16[:total], _bits16(dx[:total])) and _intact(dx, total) and _intact16(dx16, total) and _unchanged(dgd, dg)


@pytest.mark.parametrize('n,h,w,c,what', [(4090, 1, 3, 1024, 'fwd below'), (4100, 1, 3, 1024, 'fwd above, general bwd above'),
                                          (2700, 1, 3, 1024, 'general bwd below'), (2, 8, 6, 8, 'even bwd below')])
def test_maxpool_second_grid_trip(n, h, w, c, what):
    """l_maxpool_fwd walks grid_for(n * ho * wo * c / 4) output quads, the general backward kernel grid_for(n * h * w * c / 4) input
    quads, the even kernel (no padding, even h and w) output quads again; 8192 x 256 quads per trip.  A 1 x 3 map keeps the input
    within 64 MB above the cap (the even kernel's input would be four times its output: left out).  Values with ties; the maximum
    and its index are exact, the gradient 1e-6 as in test_maxpool_gap_dropout."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    uq, iq = n * ho * wo * (c // 4), n * h * w * (c // 4)
    even = h % 2 == 0 and w % 2 == 0
    assert {'fwd below': uq < 8192 * 256, 'fwd above, general bwd above': uq > 8192 * 256 and iq > 8192 * 256 and not even,
            'general bwd below': iq < 8192 * 256 and not even, 'even bwd below': even and uq < 8192 * 256}[what]
    r = np.random.default_rng(n)
    x = (r.integers(0, 4, (n, h, w, c)) + 0.25 * r.integers(0, 2, (n, h, w, c))).astype(np.float32)
    y_ref, cache = ops.maxpool3x3s2_fwd(x)
    m, mi = y_ref.size, x.size
    xd = _guarded(x); y = _out(m); idx = _u8out(m)
    call('fte_maxpool3x3s2_fwd', xd, y, idx, n, h, w, c, stream())
    torch.cuda.synchronize()
    yh, ih = y[:m].cpu().numpy().reshape(y_ref.shape), idx[:m].cpu().numpy().reshape(y_ref.shape)
    t = max(0, min(8192 * 256 * 4, m - 1024)) // (ho * wo * c)         # images from the first one the second trip touches (or the last)
    assert np.array_equal(yh[t:], y_ref[t:]) and np.array_equal(ih[t:].astype(np.int64), cache['arg'][t:]), 'second trip'
    assert np.array_equal(yh, y_ref) and np.array_equal(ih.astype(np.int64), cache['arg'])
    dy = _f32(r.standard_normal(y_ref.shape))
    dx_ref = ops.maxpool3x3s2_bwd(dy.astype(np.float64), cache)
    dyd, dx = _guarded(dy), _out(mi)
    call('fte_maxpool3x3s2_bwd', dyd, idx, dx, n, h, w, c, stream())
    torch.cuda.synchronize()
    dxh = host(dx)[:mi].reshape(x.shape)
    ti = max(0, min(8192 * 256 * 4, mi - 1024)) // (h * w * c)
    check_maxabs(dxh, dx_ref, 1e-6, 'maxpool bwd'); check_maxabs(dxh[ti:], dx_ref[ti:], 1e-6, 'maxpool bwd, second trip')
    # bf16 twins: the inputs here are bf16-exact (multiples of 1/4 below 4)
    x16 = _in16(x); y16 = _out16(m); idx2 = _u8out(m); dy16 = _in16(_b16(dy)); dx16 = _out16(mi); dx32 = _out(mi)
    call('fte_maxpool3x3s2_fwd_s16', x16, y16, idx2, n, h, w, c, stream())
    call('fte_maxpool3x3s2_bwd_s16', dy16, idx2, dx16, n, h, w, c, stream())
    call('fte_maxpool3x3s2_bwd', _f16(dy16[:m]).contiguous(), idx, dx32, n, h, w, c, stream())
    assert torch.equal(y16[:m], _bits16(y[:m])) and torch.equal(idx2, idx) and torch.equal(dx16[:mi], _bits16(dx32[:mi]))
    assert _intact(y, m) and _intact8(idx, m) and _intact(dx, mi) and _intact16(y16, m) and _intact8(idx2, m) and _intact16(dx16, mi)
    assert _unchanged(xd, x) and _unchanged(dyd, dy)


# ------------------------------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keep', [0.1, 0.5, 0.9, 1.0])
def test_dropout_mask_is_keyed_by_element_across_the_grid_stride(keep):
    """l_dropout_fwd / l_scale_mask through grid_for: 8192 blocks x 256 elements per trip, n = 8192 * 256 + 259 leaves 259 elements to
    the second trip.  The mask is a function of (seed, element index): a mask keyed by thread would repeat mask[:259] there."""
    trip = 8192 * 256
    n = trip + 259
    assert _grid_for(n) * 256 == trip
    r = np.random.default_rng(int(keep * 10))
    x = _f32(r.standard_normal(n) + 3.0); dy = _f32(r.standard_normal(n))
    xd, dyd = _guarded(x), _guarded(dy)
    m, y, m2, y2, dx = _out(n), _out(n), _out(n), _out(n), _out(n)
    call('fte_dropout_fwd', xd, m, y, n, keep, 1234, stream())
    call('fte_dropout_fwd', xd, m2, y2, n, keep, 1234, stream())
    call('fte_dropout_bwd', dyd, m, dx, n, keep, stream())
    torch.cuda.synchronize()
    mh = m[:n].cpu().numpy()
    assert set(np.unique(mh)) <= {0.0, 1.0}
    k32 = float(np.float32(keep))                                   # the probability the kernel was handed
    sd = math.sqrt(k32 * (1 - k32) / n)                             # binomial: the mean of n independent draws
    assert abs(mh.mean() - k32) <= 5 * sd, (mh.mean(), k32, sd)
    assert abs(mh[trip:].mean() - k32) <= 5 * math.sqrt(k32 * (1 - k32) / 259), 'second trip'
    assert torch.equal(m, m2) and torch.equal(y, y2), 'same seed, same mask'
    yh, dxh = y[:n].cpu().numpy(), dx[:n].cpu().numpy()
    if keep == 1.0:
        assert (mh == 1.0).all() and np.array_equal(yh.view(np.uint32), x.view(np.uint32)) and np.array_equal(dxh.view(np.uint32), dy.view(np.uint32))
    else:
        assert not np.array_equal(mh[:259], mh[trip:]), 'the second trip repeats the first: the mask is keyed by thread'
        m3 = _out(n)
        call('fte_dropout_fwd', xd, m3, y2, n, keep, 1235, stream())
        assert not torch.equal(m, m3)
    y_ref = ops.dropout_fwd(x.astype(np.float64), mh.astype(np.float64), k32); dx_ref = dy.astype(np.float64) * mh / k32
    assert (np.abs(yh - y_ref) <= 1e-7 * np.abs(y_ref)).all() and (np.abs(dxh - dx_ref) <= 1e-7 * np.abs(dx_ref)).all()
    assert (np.abs(yh[trip:] - y_ref[trip:]) <= 1e-7 * np.abs(y_ref[trip:])).all() and np.isfinite(yh).all() and np.isfinite(dxh).all()
    assert all(_intact(t, n) for t in (m, y, m2, y2, dx)) and _unchanged(xd, x) and _unchanged(dyd, dy)


# ------------------------------------------------------------------------------------------------------------------------
# 4. grouped 3x3, fp32
# ------------------------------------------------------------------------------------------------------------------------
def _gconv_ref(x, wt, dz, stride):
    groups, gw = wt.shape[0], wt.shape[3]
    ys, dx, dw = [], np.zeros_like(x), np.zeros_like(wt)
    for g in range(groups):
        s = slice(g * gw, (g + 1) * gw)
        ys.append(ops.conv2d_fwd(x[..., s], wt[g], stride))
        if dz is not None:
            dx[..., s], dw[g] = ops.conv2d_bwd(x[..., s], wt[g], dz[..., s], stride)
    return np.concatenate(ys, axis=-1), dx, dw


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c,groups', [(32, 8), (64, 8), (32, 2), (64, 2), (128, 32), (128, 16), (64, 4)])
def test_grouped_conv3x3_group_packing_branches(c, groups, stride):
    """gconv_launch: gw = 4 with groups % 32 != 0 -> GPBK = 1 (32, 8), gw = 8 with groups % 16 != 0 (64, 8), gw = 16 with groups % 4 != 0
    (32, 2), gw = 32 with two groups (64, 2); the packed forms with the fewest groups they take: (128, 32), (128, 16), (64, 4).
    l_gconv_wgrad cuts the block to `used` threads in whole waves when groups < gpb = 256 / (3 (gw / 4)^2) -- every case but (64, 2),
    where gpb = 1: 24 of 64 threads at (32, 8), 96 of 128 at (64, 8), (32, 2) and (128, 32), 192 (whole waves) at (128, 16) and (64, 4).
    Odd, non-square 7 x 9 maps (a ragged 4-pixel unit), three images."""
    n, h, w = 3, 7, 9
    gw = c // groups
    tpg = 3 * (gw // 4) ** 2
    gpb = max(256 // tpg, 1)
    used = min(groups, gpb) * tpg
    assert (groups < gpb) == ((c, groups) != (64, 2)) and used == {(32, 8): 24, (64, 8): 96, (32, 2): 96, (64, 2): 192, (128, 32): 96, (128, 16): 192, (64, 4): 192}[(c, groups)]
    r = np.random.default_rng(c * groups + stride)
    x = _f32(r.standard_normal((n, h, w, c))); wt = _f32(r.standard_normal((groups, 3, 3, gw, gw)) * 0.2)
    ho, wo = -(-h // stride), -(-w // stride)
    dz = _f32(r.standard_normal((n, ho, wo, c)))
    y_ref, dx_ref, dw_ref = _gconv_ref(x.astype(np.float64), wt.astype(np.float64), dz.astype(np.float64), stride)
    xd, wd_, dzd = _guarded(x), _guarded(wt), _guarded(dz)
    y, dx, dw = _out(dz.size), _out(x.size), _out(wt.size)
    call('fte_gconv3x3_fwd', xd, wd_, y, n, h, w, c, groups, stride, stream())
    call('fte_gconv3x3_dgrad', dzd, wd_, dx, n, h, w, c, groups, stride, stream())
    wsb, nb = ws(query('fte_gconv3x3_wgrad_ws_bytes', n, h, w, c, groups, stride))
    call('fte_gconv3x3_wgrad', xd, dzd, dw, n, h, w, c, groups, stride, wsb, nb, stream())
    torch.cuda.synchronize()
    yh, dxh, dwh = host(y)[:dz.size].reshape(dz.shape), host(dx)[:x.size].reshape(x.shape), host(dw)[:wt.size].reshape(wt.shape)
    check_maxabs(yh, y_ref, TOL_MAXABS, 'fwd'); check_maxabs(dxh, dx_ref, TOL_MAXABS, 'dgrad'); check_maxabs(dwh, dw_ref, TOL_MAXABS, 'wgrad')
    # the tails on their own: the last group, the last pixel column (the ragged unit of four), the last image
    check_maxabs(yh[..., -gw:], y_ref[..., -gw:], TOL_MAXABS, 'fwd, last group'); check_maxabs(yh[:, :, -1], y_ref[:, :, -1], TOL_MAXABS, 'fwd, last column')
    check_maxabs(dxh[..., -gw:], dx_ref[..., -gw:], TOL_MAXABS, 'dgrad, last group'); check_maxabs(dxh[:, :, -1], dx_ref[:, :, -1], TOL_MAXABS, 'dgrad, last column')
    check_maxabs(yh[-1], y_ref[-1], TOL_MAXABS, 'fwd, last image'); check_maxabs(dxh[-1], dx_ref[-1], TOL_MAXABS, 'dgrad, last image')
    check_maxabs(dwh[-1], dw_ref[-1], TOL_MAXABS, 'wgrad, last group'); check_maxabs(dwh[0], dw_ref[0], TOL_MAXABS, 'wgrad, first group')
    assert _intact(y, dz.size) and _intact(dx, x.size) and _intact(dw, wt.size) and _unchanged(xd, x) and _unchanged(wd_, wt) and _unchanged(dzd, dz)


# ------------------------------------------------------------------------------------------------------------------------
# 5. grouped 3x3, bf16
# ------------------------------------------------------------------------------------------------------------------------
def _gconv16_blocks(npix, c):
    return min((((npix + 31) // 32) + 3) // 4, max(512 // (c // 32), 1))


def _wgrad16_chunks(npix, c):
    return max(1, min(1024 // (c // 32), ((npix + 15) // 16) // 8))


@pytest.mark.parametrize('n,h,w,c,groups,stride,fwd_above,dgrad_above', [
    (1, 9, 7, 128, 32, 1, False, False), (1, 9, 7, 128, 32, 2, False, False), (2, 56, 56, 128, 32, 1, False, False), (2, 56, 56, 128, 32, 2, False, False),
    (6, 56, 56, 128, 32, 1, True, True), (6, 56, 56, 128, 32, 2, False, True), (24, 56, 56, 128, 32, 2, True, True),
    (4, 7, 7, 1024, 32, 1, False, False), (4, 7, 7, 1024, 32, 2, False, False), (48, 7, 7, 1024, 32, 1, True, True), (48, 7, 7, 1024, 32, 2, False, True),
    (48, 14, 14, 1024, 32, 2, True, True)])
def test_grouped_conv3x3_bf16_tiles_per_wave(n, h, w, c, groups, stride, fwd_above, dgrad_above):
    """gconv16_blocks: at most 512 / (c / 32) blocks of four 32-pixel tiles along x, so a wave walks several tiles above 16 384 walked
    pixels at c = 128 and above 2 048 at c = 1024.  Which grid is walked depends on the launch: forward and data gradient walk n h w
    at stride 1 (gconv3x3_mfma16_win_kernel / _kernel<0>); at stride 2 the forward (_kernel<1>) walks the output grid and the data
    gradient (_kernel<2>) the input grid -- the side of the cap is asserted per launch.  l_gconv_wgrad16_chunks: one chunk at
    (1, 9, 7, 128) and (4, 7, 7, 1024), several elsewhere.  bf16-exact operands, fp32 accumulation: TOL_MAXABS against float64."""
    gw = c // groups
    ho, wo = -(-h // stride), -(-w // stride)
    npix_in, npix_out = n * h * w, n * ho * wo
    npix_fwd = npix_in if stride == 1 else npix_out
    assert (_gconv16_blocks(npix_fwd, c) * 128 < npix_fwd) == fwd_above and (_gconv16_blocks(npix_in, c) * 128 < npix_in) == dgrad_above
    assert (_wgrad16_chunks(npix_out, c) == 1) == ((n, h, w) in ((1, 9, 7), (4, 7, 7)))
    r = np.random.default_rng(n * c + stride)
    x = _b16(r.standard_normal((n, h, w, c))); wt = _b16(r.standard_normal((groups, 3, 3, gw, gw)) * 0.2); dz = _b16(r.standard_normal((n, ho, wo, c)))
    y_ref, dx_ref, dw_ref = _gconv_ref(x.astype(np.float64), wt.astype(np.float64), dz.astype(np.float64), stride)
    words = (c // 32) * 9 * 1024
    pf = torch.empty(words, dtype=torch.int16, device='cuda'); pd = torch.empty_like(pf)
    xd, wd_, dzd = _guarded(x), _guarded(wt), _guarded(dz)
    st = stream()
    call('fte_gconv3x3_pack_bf16', wd_, pf, pd, c, groups, st)
    y, dx, dw = _out(dz.size), _out(x.size), _out(wt.size)
    call('fte_gconv3x3_bf16', xd, pf, y, n, h, w, c, stride, 0, st)
    call('fte_gconv3x3_bf16', dzd, pd, dx, n, h, w, c, stride, 1, st)
    wsb, nb = ws(query('fte_gconv3x3_wgrad_bf16_ws_bytes', n, h, w, c, groups, stride))
    call('fte_gconv3x3_wgrad_bf16', xd, dzd, dw, n, h, w, c, groups, stride, wsb, nb, st)
    torch.cuda.synchronize()
    yh, dxh, dwh = host(y)[:dz.size].reshape(dz.shape), host(dx)[:x.size].reshape(x.shape), host(dw)[:wt.size].reshape(wt.shape)
    check_maxabs(yh, y_ref, TOL_MAXABS, 'fwd'); check_maxabs(dxh, dx_ref, TOL_MAXABS, 'dgrad'); check_maxabs(dwh, dw_ref, TOL_MAXABS, 'wgrad')
    # past the first trip of the capped grid (below the cap: the last image): pixels from blocks * 128 on, flat over [n, h, w]
    t_in = min(_gconv16_blocks(npix_in, c) * 128, npix_in - h * w)
    t_out = min(_gconv16_blocks(npix_fwd, c) * 128, npix_out - ho * wo)
    check_maxabs(yh.reshape(-1, c)[t_out:], y_ref.reshape(-1, c)[t_out:], TOL_MAXABS, 'fwd, later tiles')
    check_maxabs(dxh.reshape(-1, c)[t_in:], dx_ref.reshape(-1, c)[t_in:], TOL_MAXABS, 'dgrad, later tiles')
    check_maxabs(dwh[-1], dw_ref[-1], TOL_MAXABS, 'wgrad, last group')
    # bf16 storage twins
    x16, dz16 = _in16(x), _in16(dz)
    b0, b1 = x16.clone(), dz16.clone()
    y16, dx16, dw1 = _out16(dz.size), _out16(x.size), _out(wt.size)
    call('fte_gconv3x3_bf16_s16', x16, pf, y16, n, h, w, c, stride, 0, st)
    call('fte_gconv3x3_bf16_s16', dz16, pd, dx16, n, h, w, c, stride, 1, st)
    call('fte_gconv3x3_wgrad_bf16_s16', x16, dz16, dw1, n, h, w, c, groups, stride, wsb, nb, st)
    assert torch.equal(y16[:dz.size], _bits16(y[:dz.size])) and torch.equal(dx16[:x.size], _bits16(dx[:x.size])) and torch.equal(dw1, dw)
    assert _intact(y, dz.size) and _intact(dx, x.size) and _intact(dw, wt.size) and _intact16(y16, dz.size) and _intact16(dx16, x.size) and _intact(dw1, wt.size)
    assert _unchanged(xd, x) and _unchanged(wd_, wt) and _unchanged(dzd, dz) and _unchanged16(x16, x.size, b0) and _unchanged16(dz16, dz.size, b1)


# ------------------------------------------------------------------------------------------------------------------------
# 6. depthwise 3x3
# ------------------------------------------------------------------------------------------------------------------------
def _dw_quads(c):
    return 64 if c >= 256 else 32 if c >= 128 else 16


def _dw_splits(npix, c):
    q = _dw_quads(c)
    cb = (c // 4 + q - 1) // q
    return max(1, min(2048 // cb, npix // (256 // q * 4), 1024))


DW_SIZES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 7, 9), (2, 8, 6)]


def _depthwise_case(n, h, w, c, stride):
    r = np.random.default_rng(n * h * w + c + stride)
    ho, wo = -(-h // stride), -(-w // stride)
    x = _b16(r.standard_normal((n, h, w, c))); wt = _f32(r.standard_normal((3, 3, c)) * 0.3); dy = _b16(r.standard_normal((n, ho, wo, c)))
    x64, w64, dy64 = x.astype(np.float64), wt.astype(np.float64)[..., None], dy.astype(np.float64)
    y_ref = ops.dwconv3x3_fwd(x64, w64, stride)
    dx_ref, dw_ref = ops.dwconv3x3_bwd(x64, w64, dy64, stride)
    dw_ref = dw_ref[..., 0]
    xd, wd_, dyd = _guarded(x), _guarded(wt), _guarded(dy)
    y, dx, dw = _out(dy.size), _out(x.size), _out(wt.size)
    st = stream()
    call('fte_dwconv3x3_fwd', xd, wd_, y, n, h, w, c, stride, st)
    call('fte_dwconv3x3_dgrad', dyd, wd_, dx, n, h, w, c, stride, st)
    wsb, nb = ws(query('fte_dwconv3x3_wgrad_ws_bytes', n, h, w, c, stride))
    call('fte_dwconv3x3_wgrad', xd, dyd, dw, n, h, w, c, stride, wsb, nb, st)
    torch.cuda.synchronize()
    yh, dxh, dwh = host(y)[:dy.size].reshape(dy.shape), host(dx)[:x.size].reshape(x.shape), host(dw)[:wt.size].reshape(wt.shape)
    check_maxabs(yh, y_ref, TOL_MAXABS, 'fwd'); check_maxabs(dxh, dx_ref, TOL_MAXABS, 'dgrad'); check_maxabs(dwh, dw_ref, TOL_MAXABS, 'wgrad')
    last = slice((c // 4 - 1) // _dw_quads(c) * _dw_quads(c) * 4, c)           # the last (ragged) channel block
    check_maxabs(yh[..., last], y_ref[..., last], TOL_MAXABS, 'fwd, last block'); check_maxabs(dxh[..., last], dx_ref[..., last], TOL_MAXABS, 'dgrad, last block')
    check_maxabs(dwh[..., last], dw_ref[..., last], TOL_MAXABS, 'wgrad, last block')
    check_maxabs(yh[-1, -1, -1], y_ref[-1, -1, -1], TOL_MAXABS, 'fwd, last pixel'); check_maxabs(dxh[-1, -1, -1], dx_ref[-1, -1, -1], TOL_MAXABS, 'dgrad, last pixel')
    check_maxabs(dxh[:, -1], dx_ref[:, -1], TOL_MAXABS, 'dgrad, last row'); check_maxabs(dxh[:, :, -1], dx_ref[:, :, -1], TOL_MAXABS, 'dgrad, last column')
    x16, dy16 = _in16(x), _in16(dy)
    b0, b1 = x16.clone(), dy16.clone()
    y16, dx16, dw1 = _out16(dy.size), _out16(x.size), _out(wt.size)
    call('fte_dwconv3x3_fwd_s16', x16, wd_, y16, n, h, w, c, stride, st)
    call('fte_dwconv3x3_dgrad_s16', dy16, wd_, dx16, n, h, w, c, stride, st)
    call('fte_dwconv3x3_wgrad_s16', x16, dy16, dw1, n, h, w, c, stride, wsb, nb, st)
    assert torch.equal(y16[:dy.size], _bits16(y[:dy.size])) and torch.equal(dx16[:x.size], _bits16(dx[:x.size])) and torch.equal(dw1, dw)
    assert _intact(y, dy.size) and _intact(dx, x.size) and _intact(dw, wt.size) and _intact16(y16, dy.size) and _intact16(dx16, x.size) and _intact(dw1, wt.size)
    assert _unchanged(xd, x) and _unchanged(wd_, wt) and _unchanged(dyd, dy) and _unchanged16(x16, x.size, b0) and _unchanged16(dy16, dy.size, b1)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c', [64, 116, 244, 488])
def test_depthwise3x3_channel_blocks_and_small_maps(c, stride):
    """dw_quads: Q = 16 at c = 64 (one full block) and 116 (29 quads: a ragged second block), 32 at 244 (61 quads), 64 at 488 (122 quads).
    dwconv3x3_dgrad_s2_kernel covers 2 x 2 input pixels per output quad: one pixel, a one-pixel row, a one-pixel column, odd and even
    sizes.  l_dwconv_wgrad_splits: below 1 (-> 1) at the small sizes, the npix clamp at (3, 7, 9) with c = 64."""
    assert _dw_quads(c) == {64: 16, 116: 16, 244: 32, 488: 64}[c] and (c // 4) % _dw_quads(c) == {64: 0, 116: 13, 244: 29, 488: 58}[c]
    assert _dw_splits(1, c) == 1 and (c != 64 or stride != 1 or _dw_splits(3 * 7 * 9, c) == 2)
    for n, h, w in DW_SIZES:
        _depthwise_case(n, h, w, c, stride)


@pytest.mark.parametrize('n,h,w,c,splits', [(5, 128, 128, 64, 1024), (2, 80, 64, 1024, 512), (3, 31, 29, 244, 84)])
def test_depthwise3x3_wgrad_split_clamps(n, h, w, c, splits):
    """l_dwconv_wgrad_splits = min(2048 / cb, npix / (256 / Q * 4), 1024): the 1024 clamp at (5, 128, 128, 64) (npix / 64 = 1280), the 2048 / cb clamp at
    (2, 80, 64, 1024) (cb = 4: 512 < npix / 16 = 640), the npix clamp with a ragged channel block at (3, 31, 29, 244) (2697 / 32 = 84)."""
    assert _dw_splits(n * h * w, c) == splits
    _depthwise_case(n, h, w, c, 1)


@pytest.mark.parametrize('n', [17189, 17190])
def test_depthwise3x3_dgrad_stride2_second_grid_trip(n):
    """l_dwconv_dgrad, stride 2: dwconv3x3_dgrad_s2_kernel on grid_for_c(total, c), total = n * ceil(h / 2) * ceil(ceil(w / 2) / 2) * c / 4
    units -- capped at 1024 blocks (rounded up to a multiple of m) once total >= 4 * 1024 * 256, and only then does a thread take a
    second trip with the weight quad it loaded once (`inv`: the stride is a multiple of c / 4, which is what the rounding to m is
    for).  c = 244: m = 61; a 1 x 3 map is 61 units per image, so 17 190 images are at the threshold and 17 189 just below it.  The
    images past the first trip are checked on their own."""
    h, w, c = 1, 3, 244
    ho, wo = 1, 2
    total = n * 1 * 1 * (c // 4)
    blocks = _grid_for_c(total, c, False)
    above = n == 17190
    assert (total >= 4 * 1024 * 256) == above and (blocks * 256 < total) == above and blocks % 61 == 0
    first = blocks * 256 // (c // 4) + 1 if above else n - 1            # images wholly past the first trip (below: the last one)
    r = np.random.default_rng(n)
    wt = _f32(r.standard_normal((3, 3, c)) * 0.3); dy = _b16(r.standard_normal((n, ho, wo, c)))
    dy64, w64 = dy.astype(np.float64), wt.astype(np.float64)
    pl = ops.same_pads(w, 3, 2)[1]; pt = ops.same_pads(h, 3, 2)[1]
    dxp = np.zeros((n, h + 2, w + 2, c))                                 # the transpose of ops.dwconv3x3_fwd, tap by tap
    for rr in range(3):
        for q in range(3):
            dxp[:, rr:rr + (ho - 1) * 2 + 1:2, q:q + (wo - 1) * 2 + 1:2, :] += dy64 * w64[rr, q]
    dx_ref = dxp[:, pt:pt + h, pl:pl + w, :]
    assert np.allclose(dx_ref[:3], ops.dwconv3x3_bwd(np.zeros((3, h, w, c)), w64[..., None], dy64[:3], 2)[0], rtol=1e-12, atol=0)
    dyd, wd_ = _guarded(dy), _guarded(wt)
    dx = _out(n * h * w * c)
    call('fte_dwconv3x3_dgrad', dyd, wd_, dx, n, h, w, c, 2, stream())
    torch.cuda.synchronize()
    dxh = host(dx)[:n * h * w * c].reshape(n, h, w, c)
    check_maxabs(dxh, dx_ref, TOL_MAXABS, 'dgrad'); check_maxabs(dxh[first:], dx_ref[first:], TOL_MAXABS, 'dgrad, second trip')
    check_maxabs(dxh[first:, ..., -4:], dx_ref[first:, ..., -4:], TOL_MAXABS, 'dgrad, second trip, last quad')
    dy16 = _in16(dy); b0 = dy16.clone(); dx16 = _out16(n * h * w * c)
    call('fte_dwconv3x3_dgrad_s16', dy16, wd_, dx16, n, h, w, c, 2, stream())
    assert torch.equal(dx16[:n * h * w * c], _bits16(dx[:n * h * w * c]))
    assert _intact(dx, n * h * w * c) and _intact16(dx16, n * h * w * c) and _unchanged(dyd, dy) and _unchanged(wd_, wt) and _unchanged16(dy16, dy.size, b0)


# ------------------------------------------------------------------------------------------------------------------------
# 7. channel scale
# ------------------------------------------------------------------------------------------------------------------------
def _chscale_gx(n, hw, c):
    cq = c // 4
    m = cq // math.gcd(cq, 256)
    gx = max(1, min((hw * cq + 1023) // 1024, (1024 + n - 1) // n))
    return gx, (gx + m - 1) // m * m, m


@pytest.mark.parametrize('n,hw,c,gx_plain,gx_rounded', [(1, 5, 256, 1, 1), (1, 5, 244, 1, 61), (1, 5, 116, 1, 29), (1, 400, 244, 24, 61),
                                                        (3, 400, 116, 12, 29), (5, 49, 256, 4, 4), (1030, 9, 244, 1, 61), (1030, 9, 256, 1, 1),
                                                        (1, 1, 244, 1, 61)])
def test_channel_scale_grid_rounding(n, hw, c, gx_plain, gx_rounded):
    """chscale_grid: gx = min(ceil(hw * c / 4 / 1024), ceil(1024 / n)) rounded UP to a multiple of m = (c / 4) / gcd(c / 4, 256) so that a
    thread keeps its gate quad: m = 1 at c = 256, 61 at 244, 29 at 116.  hw = 5: gx 1 -> m, at most one piece per thread; hw = 400:
    raised by the rounding (24 -> 61, 12 -> 29) and several pieces per thread; n = 1030: want = 1.  The tolerances of
    test_se_gate_pieces; dx = dy * gate + dsq * scale stored as bf16: half a bf16 step."""
    gx0, gx, m = _chscale_gx(n, hw, c)
    assert m == {256: 1, 244: 61, 116: 29}[c] and (gx0, gx) == (gx_plain, gx_rounded)
    r = np.random.default_rng(n * hw + c)
    x = _b16(r.standard_normal((n, hw, c))); dy = _b16(r.standard_normal((n, hw, c)))
    gate = _f32(1 / (1 + np.exp(-r.standard_normal((n, c))))); dsq = _f32(r.standard_normal((n, c)))
    x64, dy64, gt64, dsq64 = x.astype(np.float64), dy.astype(np.float64), gate.astype(np.float64), dsq.astype(np.float64)
    t = n * hw * c
    xd, dyd, gd, dsd = _guarded(x), _guarded(dy), _guarded(gate), _guarded(dsq)
    y, dx, dg0, dg1 = _out(t), _out(t), _out(n * c), _out(n * c)
    st = stream()
    call('fte_channel_scale_fwd', xd, gd, y, n, hw, c, st)
    call('fte_channel_scale_bwd', dyd, xd, gd, dx, dg0, n, hw, c, 0, st)
    torch.cuda.synchronize()
    yh, dxh = host(y)[:t].reshape(x.shape), host(dx)[:t].reshape(x.shape)
    check_maxabs(yh, x64 * gt64[:, None, :], 1e-6, 'scale fwd'); check_maxabs(dxh, dy64 * gt64[:, None, :], 1e-6, 'scale dx')
    check_maxabs(yh[-1, -1], (x64 * gt64[:, None, :])[-1, -1], 1e-6, 'scale fwd, last pixel'); check_maxabs(yh[..., -4:], (x64 * gt64[:, None, :])[..., -4:], 1e-6, 'scale fwd, last quad')
    check_maxabs(host(dg0)[:n * c].reshape(n, c), (dy64 * x64).sum(1), 1e-5, 'scale dgate')
    call('fte_channel_scale_bwd', dyd, xd, gd, dx, dg1, n, hw, c, 1, st)
    dg_ref = (dy64 * x64).sum(1) * gt64 * (1 - gt64)
    check_maxabs(host(dg1)[:n * c].reshape(n, c), dg_ref, 1e-5, 'scale d(pre-sigmoid)')
    # the last quad of the last image on its own: a sum of hw fp32 terms, ulp * sqrt(terms) * max|term|, next to 1e-5 of the value
    err = np.abs(host(dg1)[:n * c].reshape(n, c)[-1, -4:] - dg_ref[-1, -4:])
    assert (err <= 1e-5 * np.abs(dg_ref[-1, -4:]) + ULP * math.sqrt(hw) * np.abs(dy64 * x64)[-1, :, -4:].max()).all(), 'd(pre-sigmoid), last quad'
    x16, dy16 = _in16(x), _in16(dy)
    b0, b1 = x16.clone(), dy16.clone()
    y16, dx16, dg2 = _out16(t), _out16(t), _out(n * c)
    call('fte_channel_scale_fwd_s16', x16, gd, y16, n, hw, c, st)
    call('fte_channel_scale_bwd_s16', dy16, x16, gd, dg2, n, hw, c, 1, st)
    call('fte_channel_scale_bwd_apply_s16', dy16, gd, dsd, dx16, n, hw, c, 1.0 / hw, st)
    assert torch.equal(y16[:t], _bits16(y[:t])) and torch.equal(dg2, dg1)
    ref = dy64 * gt64[:, None, :] + dsq64[:, None, :] * float(np.float32(1.0 / hw))
    _stored16(dx16[:t], ref, 'bwd_apply'); _stored16(dx16[:t].view(n, hw, c)[-1, -1], ref[-1, -1], 'bwd_apply, last pixel')
    assert _intact(y, t) and _intact(dx, t) and _intact(dg0, n * c) and _intact(dg1, n * c) and _intact(dg2, n * c) and _intact16(y16, t) and _intact16(dx16, t)
    assert _unchanged(xd, x) and _unchanged(dyd, dy) and _unchanged(gd, gate) and _unchanged(dsd, dsq) and _unchanged16(x16, t, b0) and _unchanged16(dy16, t, b1)


# ------------------------------------------------------------------------------------------------------------------------
# 8. channel gather
# ------------------------------------------------------------------------------------------------------------------------
def _gather_lds(ca, cb, co0, co1, aligned=True):
    """host mirror of gather_lds' six conditions (layers.hip): the failing ones"""
    qin, qout = (ca + cb) // 4, (co0 + co1) // 4
    bad = []
    if (ca & 3) or (cb & 3) or (co0 & 3) or (co1 & 3):
        bad.append('width & 3')
    if not aligned:
        bad.append('pointer & 15')
    if qin < 1 or qin > 256 or (qin & (qin - 1)):
        bad.append('qin')
    if qout < 1 or qout > 256 or (qout & (qout - 1)):
        bad.append('qout')
    if not bad or bad == ['pointer & 15']:
        rg = 4 * max(256 // qin, 256 // qout)
        if rg * qin * 16 > 65536:
            bad.append('staging')
    return bad


GATHER = {'lds': (64, 64, 128, 0), 'width & 3': (62, 66, 128, 0), 'pointer & 15': (64, 64, 128, 1), 'qin': (64, 32, 128, 0),
          'qout': (64, 64, 2048, 0), 'staging': (512, 512, 4, 0)}


@pytest.mark.parametrize('rows', [1, 31, 33, 2048 * 32 + 5])
@pytest.mark.parametrize('variant', list(GATHER))
def test_channel_gather_lds_conditions(variant, rows):
    """gather_lds: the LDS form needs widths in whole quads, 16-byte aligned pointers, qin = (ca + cb) / 4 and qout = co / 4 powers of two
    up to 256, and at most 64 KB of staging (rg * qin * 16 bytes, rg = 4 * max(256 / qin, 256 / qout) rows).  'lds' (64 + 64 -> 128: rg = 32)
    passes all of them; every other variant fails exactly the one it is named after and takes the element kernels.  Rows: 1, rg - 1,
    rg + 1 and more than 2048 * rg (the block cap of the LDS form; the variants with wider rows take a tenth of it).  A gather
    copies: every result equals the concat / shuffle / split of the inputs element for element; the affine form with a scale is held
    to TOL_MAXABS."""
    ca, cb, co, off = GATHER[variant]
    assert _gather_lds(ca, cb, co, 0, not off) == ([] if variant == 'lds' else [variant])
    if rows > 33 and variant in ('qout', 'staging'):
        rows = 6559
    r = np.random.default_rng(rows + co)
    a = _b16(r.standard_normal((rows, ca))); b = _b16(r.standard_normal((rows, cb)))
    src = r.integers(0, ca + cb, co)
    src[:min(co, ca + cb)] = r.permutation(ca + cb)[:min(co, ca + cb)]
    if co >= 8:
        src[co // 2] = -1; src[-1] = -1                              # empty slots: zeros
    tab = np.where(src < 0, -1, np.where(src < ca, src, (1 << 16) | (src - ca))).astype(np.int32)
    cat = np.concatenate([a, b], 1)
    ref = np.where(src[None, :] < 0, np.float32(0), cat[:, np.maximum(src, 0)])
    td = torch.tensor(tab, device='cuda')
    abuf = _guarded(np.concatenate([np.zeros(off, np.float32), a.ravel()]))
    ad = abuf[off:]
    bd = _guarded(b)
    out = _out(rows * co)
    st = stream()
    call('fte_channel_gather', ad, bd, out, td, rows, ca, cb, co, st)
    torch.cuda.synchronize()
    got = out[:rows * co].cpu().numpy().reshape(rows, co)
    assert np.array_equal(got[-1].view(np.uint32), ref[-1].view(np.uint32)), 'last row'
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and _intact(out, rows * co)
    # two outputs in one launch (the split halves), no scale: still a copy
    if co % 8 == 0:
        h0 = co // 2
        t0, t1 = torch.tensor(tab[:h0], device='cuda'), torch.tensor(tab[h0:], device='cuda')
        o0, o1 = _out(rows * h0), _out(rows * h0)
        call('fte_channel_gather_affine', ad, bd, o0, t0, h0, o1, t1, h0, rows, ca, cb, None, None, 0, None, None, 0, st)
        assert np.array_equal(o0[:rows * h0].cpu().numpy().reshape(rows, h0).view(np.uint32), ref[:, :h0].view(np.uint32))
        assert np.array_equal(o1[:rows * h0].cpu().numpy().reshape(rows, h0).view(np.uint32), ref[:, h0:].view(np.uint32))
        assert _intact(o0, rows * h0) and _intact(o1, rows * h0)
    # batch norm folded into source a (+ ReLU), source b as it is
    sca = _f32(1 + 0.2 * r.standard_normal(ca)); sfa = _f32(0.3 * r.standard_normal(ca))
    scd, sfd = _guarded(sca), _guarded(sfa)
    o2 = _out(rows * co)
    call('fte_channel_gather_affine', ad, bd, o2, td, co, None, None, 0, rows, ca, cb, scd, sfd, 1, None, None, 0, st)
    torch.cuda.synchronize()
    cat64 = np.concatenate([np.maximum(a.astype(np.float64) * sca.astype(np.float64) + sfa.astype(np.float64), 0), b.astype(np.float64)], 1)
    ref2 = np.where(src[None, :] < 0, 0.0, cat64[:, np.maximum(src, 0)])
    check_maxabs(host(o2)[:rows * co].reshape(rows, co), ref2, TOL_MAXABS, 'affine'); check_maxabs(host(o2)[:rows * co].reshape(rows, co)[-1], ref2[-1], TOL_MAXABS, 'affine, last row')
    assert _intact(o2, rows * co) and _unchanged(scd, sca) and _unchanged(sfd, sfa)
    if not off:                                                      # bf16 storage (no 4-byte offset there: 2-byte elements)
        a16, b16 = _in16(a), _in16(b)
        c0, c1 = a16.clone(), b16.clone()
        o16, p16 = _out16(rows * co), _out16(rows * co)
        call('fte_channel_gather_s16', a16, b16, o16, td, rows, ca, cb, co, st)
        call('fte_channel_gather_affine_s16', a16, b16, p16, td, co, None, None, 0, rows, ca, cb, scd, sfd, 1, None, None, 0, st)
        assert torch.equal(o16[:rows * co], _bits16(out[:rows * co])) and torch.equal(p16[:rows * co], _bits16(o2[:rows * co]))
        assert _intact16(o16, rows * co) and _intact16(p16, rows * co) and _unchanged16(a16, rows * ca, c0) and _unchanged16(b16, rows * cb, c1)
    assert np.array_equal(abuf[off:off + rows * ca].cpu().numpy().view(np.uint32), a.ravel().view(np.uint32)) and _intact(abuf, off + rows * ca) and _unchanged(bd, b)
    assert np.array_equal(td.cpu().numpy(), tab)


# ------------------------------------------------------------------------------------------------------------------------
# 9. stem im2col
# ------------------------------------------------------------------------------------------------------------------------
def _im2col_ref(x, ks, stride, kpad):
    n, h, w, cin = x.shape
    ho, pt, pb = ops.same_pads(h, ks, stride)
    wo, pl, pr = ops.same_pads(w, ks, stride)
    cols = ops._im2col(np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0))), ks, ks, stride, ho, wo)
    out = np.zeros((n * ho * wo, kpad), np.float32)
    out[:, :ks * ks * cin] = cols
    return out


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('n,h,w,cin,ks,kpad', [(2, 13, 9, 3, 7, 160), (2, 13, 9, 3, 7, 192), (1, 7, 11, 1, 7, 64), (2, 9, 13, 3, 5, 96),
                                               (1, 5, 1030, 3, 7, 160), (1, 5, 1024, 3, 7, 160)])
def test_stem_im2col_forms(n, h, w, cin, ks, kpad, stride):
    """l_im2col_first: the rows form needs ks == 7, cin == 3, kpad == 160 and w <= 1024 (w = 1024: the widest it takes, 86 KB of dynamic
    LDS, 74 / 37 trips of its PX = 14 output-column loop and several of its staging loop); kpad = 192 or w = 1030 on the same kind of image
    takes the generic kernel's <7, 3> instance, cin = 1 its <7, 1> instance, ks = 5 the run-time <0, 0> one.  im2col copies: the columns
    equal the padded image's windows bit for bit (k ordered (r, s, c)), the pad columns are exactly zero, and the two forms agree on
    their first 147 columns.  The bf16 form stores the rounding."""
    r = np.random.default_rng(h * w + cin + ks + stride)
    x = _f32(r.uniform(-1, 1, (n, h, w, cin)))
    ref = _im2col_ref(x, ks, stride, kpad)
    m = ref.shape[0]
    k = ks * ks * cin
    xd = _guarded(x)
    cols, cols16 = _out(m * kpad), _out16(m * kpad)
    call('fte_im2col_first', xd, cols, n, h, w, cin, ks, stride, kpad, stream())
    call('fte_im2col_first_s16', xd, cols16, n, h, w, cin, ks, stride, kpad, stream())
    torch.cuda.synchronize()
    got = cols[:m * kpad].cpu().numpy().reshape(m, kpad)
    assert np.array_equal(got[:, k:].view(np.uint32), np.zeros((m, kpad - k), np.uint32)), 'pad columns'
    assert np.array_equal(got[-1].view(np.uint32), ref[-1].view(np.uint32)), 'last row'
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert torch.equal(cols16[:m * kpad], _bits16(cols[:m * kpad])) and _intact(cols, m * kpad) and _intact16(cols16, m * kpad) and _unchanged(xd, x)
    if kpad == 160 and w <= 1024:                                    # the rows form against the generic form on the same image
        wide = _out(m * 192)
        call('fte_im2col_first', xd, wide, n, h, w, cin, ks, stride, 192, stream())
        other = wide[:m * 192].cpu().numpy().reshape(m, 192)
        assert np.array_equal(other[:, :147].view(np.uint32), got[:, :147].view(np.uint32)) and (other[:, 147:].view(np.uint32) == 0).all() and _intact(wide, m * 192)


def test_stem_im2col_generic_second_grid_trip():
    """im2col_first_kernel walks grid_for(n * ho * wo * kpad / 4) quads, 8192 x 256 per trip: (4, 224, 224, 3) at stride 2 with kpad =
    192 (the generic <7, 3> instance) is 50 176 rows of 48 quads, 2.4 M quads, so rows from 43 691 on belong to the second trip."""
    n, h, w, cin, ks, stride, kpad = 4, 224, 224, 3, 7, 2, 192
    r = np.random.default_rng(224)
    x = _f32(r.uniform(-1, 1, (n, h, w, cin)))
    ref = _im2col_ref(x, ks, stride, kpad)
    m = ref.shape[0]
    assert m * (kpad // 4) > 8192 * 256
    trip = 8192 * 256 // (kpad // 4) + 1
    xd = _guarded(x)
    cols, cols16 = _out(m * kpad), _out16(m * kpad)
    call('fte_im2col_first', xd, cols, n, h, w, cin, ks, stride, kpad, stream())
    call('fte_im2col_first_s16', xd, cols16, n, h, w, cin, ks, stride, kpad, stream())
    torch.cuda.synchronize()
    got = cols[:m * kpad].cpu().numpy().reshape(m, kpad)
    assert np.array_equal(got[trip:].view(np.uint32), ref[trip:].view(np.uint32)), 'second trip'
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and (got[:, 147:].view(np.uint32) == 0).all()
    assert torch.equal(cols16[:m * kpad], _bits16(cols[:m * kpad])) and _intact(cols, m * kpad) and _intact16(cols16, m * kpad) and _unchanged(xd, x)


# ------------------------------------------------------------------------------------------------------------------------
# 10. rejections
# ------------------------------------------------------------------------------------------------------------------------
def test_layer_entry_points_refuse_what_fte_h_excludes_and_launch_nothing():
    """FTE_EINVAL before any launch: c % 4 where the float4 layouts need it, c < 32 with a bf16 flag, n % 4 for fte_relu_bwd, a stride of
    3, a group width outside {4, 8, 16, 32}, and for fte_gap_bwd what fte.h states for every entry point (a null pointer, a
    non-positive size).  Every buffer is a poisoned, canaried one and must come back as it was."""
    bufs = [_out(4096) for _ in range(8)]
    b16 = [_out16(4096) for _ in range(3)]
    u8 = _u8out(4096)
    wsb, nb = ws(query('fte_bn_ws_bytes', 64))
    p = [t.data_ptr() for t in bufs]
    h = [t.data_ptr() for t in b16]
    w_, st = wsb.data_ptr(), stream()
    tab = torch.zeros(64, dtype=torch.int32, device='cuda').data_ptr()
    q = query
    # c % 4
    assert q('fte_bn_train_fwd', p[0], p[1], p[2], None, p[3], p[4], p[5], p[6], p[7], None, None, 8, 6, 1e-3, 0.9, 0, w_, nb, st) == EINVAL
    assert q('fte_bn_train_bwd', p[0], None, p[1], p[2], p[3], p[4], p[5], p[6], p[7], 8, 6, w_, nb, st) == EINVAL
    assert q('fte_bn_train_stats', p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, None, 8, 6, 1e-3, 0.9, w_, nb, st) == EINVAL
    assert q('fte_bn_apply', p[0], p[1], p[2], None, p[3], 8, 6, 0, 0, st) == EINVAL
    assert q('fte_bn_bwd_apply', p[0], p[1], p[2], p[3], 8, 6, 0, st) == EINVAL
    assert q('fte_maxpool3x3s2_fwd', p[0], p[1], u8.data_ptr(), 1, 4, 4, 6, st) == EINVAL
    assert q('fte_maxpool3x3s2_bwd', p[0], u8.data_ptr(), p[1], 1, 4, 4, 6, st) == EINVAL
    assert q('fte_gap_fwd', p[0], p[1], 1, 4, 6, st) == EINVAL
    assert q('fte_channel_scale_fwd', p[0], p[1], p[2], 1, 4, 6, st) == EINVAL
    assert q('fte_channel_scale_bwd', p[0], p[1], p[2], p[3], p[4], 1, 4, 6, 0, st) == EINVAL
    assert q('fte_channel_scale_bwd_apply_s16', h[0], p[1], p[2], h[1], 1, 4, 6, 1.0, st) == EINVAL
    assert q('fte_dwconv3x3_fwd', p[0], p[1], p[2], 1, 4, 4, 6, 1, st) == EINVAL
    assert q('fte_dwconv3x3_dgrad', p[0], p[1], p[2], 1, 4, 4, 6, 1, st) == EINVAL
    assert q('fte_dwconv3x3_wgrad', p[0], p[1], p[2], 1, 4, 4, 6, 1, w_, nb, st) == EINVAL
    assert q('fte_channel_gather', p[0], p[1], p[2], tab, 4, 8, 8, 6, st) == EINVAL
    # c < 32 (or a flag outside bits 0 and 1) with bf16 storage
    assert q('fte_bn_train_fwd_s16', h[0], p[1], p[2], None, h[1], p[4], p[5], p[6], p[7], None, None, 8, 28, 1e-3, 0.9, 0, 3, w_, nb, st) == EINVAL
    assert q('fte_bn_train_bwd_s16', h[0], None, h[1], p[2], p[3], p[4], None, None, None, h[2], p[6], p[7], 8, 28, 3, w_, nb, st) == EINVAL
    assert q('fte_bn_train_stats_s16', h[0], p[1], p[2], p[3], p[4], p[5], p[6], None, None, 8, 28, 1e-3, 0.9, 1, w_, nb, st) == EINVAL
    assert q('fte_bn_apply', h[0], p[1], p[2], None, h[1], 8, 28, 0, 3, st) == EINVAL
    assert q('fte_bn_bwd_apply', h[0], h[1], p[2], h[2], 8, 28, 1, st) == EINVAL
    assert q('fte_bn_apply', p[0], p[1], p[2], None, p[3], 8, 32, 0, 4, st) == EINVAL
    # n % 4
    assert q('fte_relu_bwd', p[0], p[1], p[2], 1022, st) == EINVAL and q('fte_relu_bwd_s16', h[0], h[1], h[2], 1022, st) == EINVAL
    # a stride of 3
    assert q('fte_gconv3x3_fwd', p[0], p[1], p[2], 1, 4, 4, 32, 8, 3, st) == EINVAL
    assert q('fte_gconv3x3_dgrad', p[0], p[1], p[2], 1, 4, 4, 32, 8, 3, st) == EINVAL
    assert q('fte_gconv3x3_wgrad', p[0], p[1], p[2], 1, 4, 4, 32, 8, 3, w_, nb, st) == EINVAL
    assert q('fte_gconv3x3_bf16', p[0], h[0], p[2], 1, 4, 4, 32, 3, 0, st) == EINVAL
    assert q('fte_dwconv3x3_fwd', p[0], p[1], p[2], 1, 4, 4, 8, 3, st) == EINVAL
    assert q('fte_dwconv3x3_dgrad_s16', h[0], p[1], h[1], 1, 4, 4, 8, 3, st) == EINVAL
    # a group width outside 4 / 8 / 16 / 32: 2, 64 and 12
    for c, groups in ((32, 16), (64, 1), (24, 2)):
        assert q('fte_gconv3x3_fwd', p[0], p[1], p[2], 1, 4, 4, c, groups, 1, st) == EINVAL, (c, groups)
        assert q('fte_gconv3x3_dgrad', p[0], p[1], p[2], 1, 4, 4, c, groups, 1, st) == EINVAL, (c, groups)
        assert q('fte_gconv3x3_wgrad', p[0], p[1], p[2], 1, 4, 4, c, groups, 1, w_, nb, st) == EINVAL, (c, groups)
    assert q('fte_gconv3x3_pack_bf16', p[0], h[0], h[1], 64, 1, st) == EINVAL
    assert q('fte_gconv3x3_wgrad_bf16', p[0], p[1], p[2], 1, 4, 4, 64, 1, 1, w_, nb, st) == EINVAL
    # fte_gap_bwd: null pointers and non-positive sizes
    for name, dx in (('fte_gap_bwd', p[1]), ('fte_gap_bwd_s16', h[0])):
        assert q(name, None, dx, 1, 4, 8, st) == EINVAL and q(name, p[0], None, 1, 4, 8, st) == EINVAL
        assert q(name, p[0], dx, 0, 4, 8, st) == EINVAL and q(name, p[0], dx, 1, 0, 8, st) == EINVAL and q(name, p[0], dx, 1, 4, 0, st) == EINVAL
        assert q(name, p[0], dx, 1, 4, -8, st) == EINVAL
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.isnan(t[:4096]).all() and _intact(t, 4096)
    for t in b16:
        assert (t[:4096] == 0x7FC1).all() and _intact16(t, 4096)
    assert (u8[:4096] == 0xEE).all() and _intact8(u8, 4096)
