"""-m gpu: the fused BN + PReLU kernels of csrc/iresnet.hip through the C ABI (fte.h "BN + PReLU") against float64 on the float32
inputs (tests/iresnet_ref.py).  Every output buffer is poisoned with NaN and followed by a canary that must come back bit for bit;
inputs must come back unchanged (the convention of test_gpu_layers_edges.py, whose tolerances for fte_bn_train_bwd_zmask are the
ones used here: TOL_MAXABS on dz, TOL_RELL2 on the per-channel sums, and per channel TOL_RELL2 * |ref| + ulp * sqrt(rows) * max|term|).

Launcher conditions (iresnet.hip) -> the case on each side, asserted with a host mirror (iresnet_ref.split_plan / _apply_grid):
  prelu_split: splits = min(2048 / cb, rows / (lanes * 8), BN_MAX_SPLITS), >= 1
        one split: (1, 64), (37, 64), (77, 116), (50, 28); several with a short last split: (784, 128) 12, (98, 512) 3,
        (1061, 256) 33, (8200, 256) 249 -- more than the 16 split lanes of the merge kernel, so a lane sums several
  reduce_quads 8 / 16 / 32 / 64: c = 28 (below 32 channels: 7 of the block's 8 quads) / 64, 116 (ragged second block) / 128 / 256, 512
  apply grid capped at 512 blocks from n4 >= 4 * 512 * 256: (8200, 256) is above (four pieces per thread and a remainder), the rest below

The kink: fma rounds to nearest, so the sign of u = fma(z, scale, shift) IS the sign of the exact z * scale + shift the float64
reference evaluates on the same float32 scale / shift -- no element should differ.  The band of the issue is applied all the same:
an element with |u| < 1e-5 * rms(u) is left out of the dz comparison only (at most 0.1 % of a case, checked for the reference alone in
test_iresnet_host.py); the planted u == 0 are never left out."""
import math

import numpy as np
import pytest
import torch

import iresnet_ref as ir
from test_gpu_arena_edges import _guarded, _intact
from test_gpu_layers_edges import BN_MAX_SPLITS, ULP, _out, _unchanged

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, host, stream, ws, check_maxabs, check_rell2, TOL_MAXABS, TOL_RELL2

EINVAL = -1
INPUTS = ('z', 'dy', 'gamma', 'mean', 'rstd', 'scale', 'shift', 'alpha')


def _apply_grid(n4, c):
    """host mirror of apply_grid (iresnet.hip; grid_for_c of layers.hip for fp32 tensors): (blocks, capped)"""
    q = c // 4
    m = q // math.gcd(q, 256)
    blocks = max(1, min(8192, (n4 + 255) // 256))
    capped = blocks > 512 and n4 >= 4 * 512 * 256
    if capped:
        blocks = 512
    return (blocks + m - 1) // m * m, capped


def _device(case):
    return {k: _guarded(case[k]) for k in INPUTS}


def _inputs_unchanged(d, case):
    return all(_unchanged(d[k], case[k]) for k in INPUTS)


def _per_channel(got, ref, terms, maxterm, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = TOL_RELL2 * np.abs(ref) + ULP * math.sqrt(terms) * maxterm
    assert (err <= bound).all(), (what, float((err / bound).max()))


def _backward(d, rows, c, alpha=None):
    n = rows * c
    dz, dg, db, da = _out(n), _out(c), _out(c), _out(c)
    wsb, nb = ws(query('fte_bn_prelu_ws_bytes', c))
    call('fte_bn_prelu_train_bwd', d['dy'], d['z'], d['gamma'], d['mean'], d['rstd'], d['scale'], d['shift'], d['alpha'] if alpha is None else alpha,
         dz, dg, db, da, rows, c, wsb, nb, stream())
    torch.cuda.synchronize()
    assert _intact(dz, n) and _intact(dg, c) and _intact(db, c) and _intact(da, c)
    return dz, dg, db, da


@pytest.mark.parametrize('rows,c,splits', ir.KERNEL_CASES)
def test_forward(rows, c, splits):
    """fte_bn_prelu_apply against float64 at TOL_MAXABS; the planted u == 0 give 0; alpha = 1 is fte_bn_apply(relu = 0) bit for bit,
    alpha = 0 equals fte_bn_apply(relu = 1) in value; fte_bn_prelu_infer_fwd = fte_bn_infer_coef + the apply, same bits"""
    n = rows * c
    assert _apply_grid(n // 4, c)[1] == (rows == 8200)
    case = ir.kernel_case(rows, c)
    ref = ir.kernel_ref(case)
    d = _device(case)
    st = stream()
    y = _out(n)
    call('fte_bn_prelu_apply', d['z'], d['scale'], d['shift'], d['alpha'], y, rows, c, st)
    torch.cuda.synchronize()
    yh = host(y)[:n].reshape(rows, c)
    check_maxabs(yh, ref['y'], TOL_MAXABS, 'y')
    for rr in case['planted']:
        assert ref['u'][rr, 0] == 0 and ref['u'][rr, 3] == 0 and yh[rr, 0] == 0 and yh[rr, 3] == 0
    one, zero = _guarded(np.ones(c, np.float32)), _guarded(np.zeros(c, np.float32))
    y1, y1r, y0, y0r = _out(n), _out(n), _out(n), _out(n)
    call('fte_bn_prelu_apply', d['z'], d['scale'], d['shift'], one, y1, rows, c, st)
    call('fte_bn_apply', d['z'], d['scale'], d['shift'], None, y1r, rows, c, 0, 0, st)
    call('fte_bn_prelu_apply', d['z'], d['scale'], d['shift'], zero, y0, rows, c, st)
    call('fte_bn_apply', d['z'], d['scale'], d['shift'], None, y0r, rows, c, 1, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y1r.view(torch.int32)), 'alpha = 1 differs from fte_bn_apply(relu = 0) in some bit'
    assert bool((y0[:n] == y0r[:n]).all()), 'alpha = 0 differs from fte_bn_apply(relu = 1) in value'
    # inference form: coefficients from the moving statistics, then the same apply
    r = np.random.default_rng(c)
    gam, bet = case['gamma'], (0.3 * r.standard_normal(c)).astype(np.float32)
    mm, mv = (0.1 * r.standard_normal(c) + 3).astype(np.float32), (4 + r.random(c)).astype(np.float32)
    gd, bd, mmd, mvd = _guarded(gam), _guarded(bet), _guarded(mm), _guarded(mv)
    yi, sc, sf, sc2, sf2, yi2 = _out(n), _out(c), _out(c), _out(c), _out(c), _out(n)
    call('fte_bn_prelu_infer_fwd', d['z'], gd, bd, mmd, mvd, d['alpha'], yi, sc, sf, rows, c, ir.BN_EPS, st)
    call('fte_bn_infer_coef', gd, bd, mmd, mvd, sc2, sf2, c, ir.BN_EPS, st)
    call('fte_bn_prelu_apply', d['z'], sc2, sf2, d['alpha'], yi2, rows, c, st)
    torch.cuda.synchronize()
    assert torch.equal(sc, sc2) and torch.equal(sf, sf2) and torch.equal(yi.view(torch.int32), yi2.view(torch.int32))
    f = lambda a: a.astype(np.float64)
    ui = f(gam) * (f(case['z']) - f(mm)) / np.sqrt(f(mv) + ir.BN_EPS) + f(bet)
    check_maxabs(host(yi)[:n].reshape(rows, c), np.where(ui > 0, ui, f(case['alpha']) * ui), TOL_MAXABS, 'inference y')
    assert all(_intact(t, n) for t in (y, y1, y1r, y0, y0r, yi, yi2)) and all(_intact(t, c) for t in (sc, sf, sc2, sf2))
    assert _inputs_unchanged(d, case) and _unchanged(gd, gam) and _unchanged(bd, bet) and _unchanged(mmd, mm) and _unchanged(mvd, mv)
    assert _unchanged(one, np.ones(c, np.float32)) and _unchanged(zero, np.zeros(c, np.float32))


@pytest.mark.parametrize('rows,c,splits', ir.KERNEL_CASES)
def test_backward(rows, c, splits):
    """fte_bn_prelu_train_bwd: dz, dgamma, dbeta, dalpha against float64; every sum against its terms' magnitudes; two calls give the
    same bytes; alpha = 1 agrees with fte_bn_train_bwd without a mask"""
    got_splits, rps = ir.split_plan(rows, c, BN_MAX_SPLITS)
    assert got_splits == splits
    if splits > 1:
        assert rows % rps != 0, 'the several-split cases leave the last split short'
    n = rows * c
    case = ir.kernel_case(rows, c)
    ref = ir.kernel_ref(case)
    assert ref['band'].sum() <= ir.KINK_CAP * n
    d = _device(case)
    dz, dg, db, da = _backward(d, rows, c)
    dzh = host(dz)[:n].reshape(rows, c)
    assert np.isfinite(dzh).all()
    keep = ~ref['band']                                  # (the planted zeros are never in the band)
    for rr in case['planted']:
        assert keep[rr, 0] and keep[rr, 3]
    check_maxabs(np.where(keep, dzh, ref['dz']), ref['dz'], TOL_MAXABS, 'dz')
    dzp, refp = dzh[case['planted']][:, [0, 3]], ref['dz'][case['planted']][:, [0, 3]]
    assert (np.abs(dzp - refp) <= TOL_MAXABS * np.abs(ref['dz']).max()).all(), 'dz at u == 0: slope alpha, as the forward'
    check_rell2(host(dg)[:c], ref['dgamma'], TOL_RELL2, 'dgamma')
    check_rell2(host(db)[:c], ref['dbeta'], TOL_RELL2, 'dbeta')
    check_rell2(host(da)[:c], ref['dalpha'], TOL_RELL2, 'dalpha')
    _per_channel(host(dg)[:c], ref['dgamma'], rows, ref['max_gamma'], 'dgamma per channel')
    _per_channel(host(db)[:c], ref['dbeta'], rows, ref['max_beta'], 'dbeta per channel')
    _per_channel(host(da)[:c], ref['dalpha'], rows, ref['max_alpha'], 'dalpha per channel')
    # against the sum of the terms' magnitudes: rows fp32 terms, each with at most three roundings of its own (u, the product with
    # alpha, the product with dy or xhat), summed in some order: |err| <= (rows + 3) * 2^-24 * sum |term| whatever the order
    for nm, got in (('alpha', da), ('gamma', dg), ('beta', db)):
        err = np.abs(host(got)[:c] - ref['d' + nm])
        assert (err <= (rows + 3) * 2.0 ** -24 * ref['mag_' + nm] + 1e-30).all(), ('d' + nm, float(err.max()))
    # deterministic: same bytes twice
    dz2, dg2, db2, da2 = _backward(d, rows, c)
    for a, b in ((dz, dz2), (dg, dg2), (db, db2), (da, da2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # alpha = 1: the BN backward without a mask
    one = _guarded(np.ones(c, np.float32))
    dz1, dg1, db1, da1 = _backward(d, rows, c, alpha=one)
    dzr, dgr, dbr = _out(n), _out(c), _out(c)
    wsb, nb = ws(query('fte_bn_ws_bytes', c))
    call('fte_bn_train_bwd', d['dy'], None, d['z'], d['gamma'], d['mean'], d['rstd'], dzr, dgr, dbr, rows, c, wsb, nb, stream())
    torch.cuda.synchronize()
    check_maxabs(host(dz1)[:n], host(dzr)[:n], TOL_MAXABS, 'dz, alpha = 1, against fte_bn_train_bwd')
    check_rell2(host(dg1)[:c], host(dgr)[:c], TOL_RELL2, 'dgamma, alpha = 1'); check_rell2(host(db1)[:c], host(dbr)[:c], TOL_RELL2, 'dbeta, alpha = 1')
    assert _intact(dzr, n) and _intact(dgr, c) and _intact(dbr, c)
    assert _inputs_unchanged(d, case) and _unchanged(one, np.ones(c, np.float32))


def test_bad_arguments_launch_nothing():
    """c % 4 != 0 and a short workspace: FTE_EINVAL, every buffer as it was"""
    bufs = [_out(4096) for _ in range(12)]
    p = [t.data_ptr() for t in bufs]
    before = [t.clone() for t in bufs]
    c = 64
    wsb, nb = ws(query('fte_bn_prelu_ws_bytes', c))
    need = query('fte_bn_prelu_ws_bytes', c)
    assert need == (BN_MAX_SPLITS * 3 * c + 3 * c) * 4 and nb >= need
    w_, st = wsb.data_ptr(), stream()
    wsb.fill_(7.0)
    q = query
    assert q('fte_bn_prelu_apply', p[0], p[1], p[2], p[3], p[4], 8, 6, st) == EINVAL
    assert q('fte_bn_prelu_infer_fwd', p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], 8, 6, 1e-5, st) == EINVAL
    assert q('fte_bn_prelu_train_bwd', *p[:12], 8, 6, w_, nb, st) == EINVAL
    assert q('fte_bn_prelu_train_bwd', *p[:12], 8, c, w_, need - 4, st) == EINVAL
    assert q('fte_bn_prelu_train_bwd', *p[:12], 8, c, None, need, st) == EINVAL
    assert q('fte_bn_prelu_train_bwd', *p[:12], 0, c, w_, nb, st) == EINVAL
    assert q('fte_bn_prelu_apply', p[0], p[1], p[2], None, p[4], 8, c, st) == EINVAL
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    assert bool((wsb == 7.0).all())
