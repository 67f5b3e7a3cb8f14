"""-m gpu: the kernels of csrc/iresnet.hip behind fte.h "BN + SE + shortcut, no activation" through the C ABI against float64 on the
float32 inputs (tests/se_iresnet_ref.py).  Every output buffer is poisoned with NaN and followed by a canary that must come back bit
for bit; inputs must come back unchanged (the conventions of test_gpu_iresnet_kernels.py).

Tolerances.  Tensors: TOL_MAXABS of the largest reference value.  A sum over the pixels of an image, per [n, c] entry:
TOL_RELL2 * |ref| + ulp * sqrt(hw) * max|term|.  The squeeze's sum is sum_hw z; sq and xm are that sum through an affine map, so
their bound is the sum's bound times |scale| / hw (|rstd| / hw) plus one ulp of each of the map's two terms (the division and the
final multiply-add round once each).  dgate = (gamma s2 + beta s1) gate (1 - gate): the bounds of s1 and s2 through the same map,
plus two ulp of its terms.

Launcher branches -> cases: se_iresnet_ref.KERNEL_CASES states the branch beside every case; the split count the device plans
(fte_se_lin_ws_bytes / (2 n c 4)) must be the host mirror's for the device's CU count, and on a 256-CU device the stated one."""
import numpy as np
import pytest
import torch

import se_iresnet_ref as sr
from test_gpu_arena_edges import _guarded, _intact
from test_gpu_layers_edges import ULP, _out, _unchanged

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, host, stream, ws, check_maxabs, TOL_MAXABS, TOL_RELL2

EINVAL = -1
INPUTS = ('z', 'dy', 'shortcut', 'gamma', 'beta', 'mean', 'rstd', 'scale', 'shift', 'gate')
_DEV = {}


def _device(case):
    """guarded device copies of a case's inputs: uploaded once per shape, checked for changes by every test that used them"""
    key = (case['n'], case['hw'], case['c'])
    if key not in _DEV:
        _DEV.clear()                                      # (one shape resident at a time: the parametrised tests run shape by shape)
        _DEV[key] = {k: _guarded(case[k]) for k in INPUTS}
    return _DEV[key]


def _inputs_unchanged(d, case):
    return all(_unchanged(d[k], case[k]) for k in INPUTS)


def _splits(n, hw, c, stated):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nbytes = query('fte_se_lin_ws_bytes', n, hw, c)
    assert nbytes % (2 * n * c * 4) == 0
    s = nbytes // (2 * n * c * 4)
    assert s == sr.split_plan(n, hw, c, cus)[0], (s, cus)
    if cus == 256:
        assert s == stated
    return s


def _sum_bound(ref, hw, maxterm):
    return TOL_RELL2 * np.abs(ref) + ULP * np.sqrt(hw) * maxterm


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()))


def _squeeze(d, n, hw, c, with_xm=True):
    sq, xm = _out(n * c), _out(n * c)
    wsb, nb = ws(query('fte_se_lin_ws_bytes', n, hw, c))
    call('fte_se_lin_squeeze', d['z'], d['scale'], d['shift'], d['mean'], d['rstd'], sq, xm if with_xm else None, n, hw, c, wsb, nb, stream())
    torch.cuda.synchronize()
    assert _intact(sq, n * c) and _intact(xm, n * c)
    return sq, xm


def _sums(d, n, hw, c):
    s1, s2, dg = _out(n * c), _out(n * c), _out(n * c)
    wsb, nb = ws(query('fte_se_lin_ws_bytes', n, hw, c))
    call('fte_se_lin_bwd_sums', d['dy'], d['z'], d['gamma'], d['beta'], d['mean'], d['rstd'], d['gate'], s1, s2, dg, n, hw, c, wsb, nb, stream())
    torch.cuda.synchronize()
    assert _intact(s1, n * c) and _intact(s2, n * c) and _intact(dg, n * c)
    return s1, s2, dg


@pytest.mark.parametrize('n,hw,c,splits', sr.KERNEL_CASES)
def test_squeeze(n, hw, c, splits):
    """fte_se_lin_squeeze: sq, xm against float64; without xm nothing is written there; against fte_se_squeeze on the same inputs
    (within the two bounds: the walk order differs -- lanes of a wave by an xor butterfly, the sibling adds 16 LDS rows in order -- so no
    bit identity is claimed, at S = 1 either); two calls give the same bytes"""
    s = _splits(n, hw, c, splits)
    case = sr.kernel_case(n, hw, c)
    ref = sr.kernel_ref(case)
    d = _device(case)
    f = lambda k: case[k].astype(np.float64)
    bsum = _sum_bound(f('z').sum(1), hw, ref['max_z'])
    b_sq = bsum * np.abs(f('scale')) / hw + ULP * (np.abs(ref['sq']) + np.abs(f('shift')))
    b_xm = bsum * np.abs(f('rstd')) / hw + ULP * (np.abs(ref['xm']) + np.abs(f('mean') * f('rstd')))
    sq, xm = _squeeze(d, n, hw, c)
    _within(host(sq)[:n * c].reshape(n, c), ref['sq'], b_sq, 'sq')
    _within(host(xm)[:n * c].reshape(n, c), ref['xm'], b_xm, 'xm')
    sq2, xm2 = _squeeze(d, n, hw, c)
    assert torch.equal(sq.view(torch.int32), sq2.view(torch.int32)) and torch.equal(xm.view(torch.int32), xm2.view(torch.int32)), s
    sq3, xm3 = _squeeze(d, n, hw, c, with_xm=False)
    assert torch.equal(sq.view(torch.int32), sq3.view(torch.int32)) and bool(torch.isnan(xm3[:n * c]).all())
    sqs, xms = _out(n * c), _out(n * c)
    call('fte_se_squeeze', d['z'], d['scale'], d['shift'], d['mean'], d['rstd'], sqs, xms, n, hw, c, 0, stream())
    torch.cuda.synchronize()
    assert _intact(sqs, n * c) and _intact(xms, n * c)
    _within(host(sq)[:n * c].reshape(n, c), host(sqs)[:n * c].reshape(n, c), 2 * b_sq, 'sq against fte_se_squeeze')
    _within(host(xm)[:n * c].reshape(n, c), host(xms)[:n * c].reshape(n, c), 2 * b_xm, 'xm against fte_se_squeeze')
    assert _inputs_unchanged(d, case)


@pytest.mark.parametrize('n,hw,c,splits', sr.KERNEL_CASES)
def test_apply_forward(n, hw, c, splits):
    """fte_se_lin_apply_fwd: out = u * gate + shortcut, negative values kept; gate = 1 gives the bytes of fte_bn_apply(res, relu = 0)"""
    case = sr.kernel_case(n, hw, c)
    ref = sr.kernel_ref(case)
    d = _device(case)
    m = n * hw * c
    out = _out(m)
    call('fte_se_lin_apply_fwd', d['z'], d['scale'], d['shift'], d['gate'], d['shortcut'], out, n, hw, c, stream())
    torch.cuda.synchronize()
    got = host(out)[:m].reshape(n, hw, c)
    check_maxabs(got, ref['out'], TOL_MAXABS, 'out')
    assert (ref['out'] < 0).any() and ((got < 0) == (ref['out'] < 0))[np.abs(ref['out']) > TOL_MAXABS * np.abs(ref['out']).max()].all(), 'no clamp'
    one = _guarded(np.ones(n * c, np.float32))
    o1, o1r = _out(m), _out(m)
    call('fte_se_lin_apply_fwd', d['z'], d['scale'], d['shift'], one, d['shortcut'], o1, n, hw, c, stream())
    call('fte_bn_apply', d['z'], d['scale'], d['shift'], d['shortcut'], o1r, n * hw, c, 0, 0, stream())
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int32), o1r.view(torch.int32)), 'gate = 1 differs from fte_bn_apply(res = shortcut, relu = 0) in some bit'
    check_maxabs(host(o1)[:m].reshape(n, hw, c), ref['bn_res'], TOL_MAXABS, 'gate = 1')
    assert _intact(out, m) and _intact(o1, m) and _intact(o1r, m)
    assert _inputs_unchanged(d, case) and _unchanged(one, np.ones(n * c, np.float32))


@pytest.mark.parametrize('n,hw,c,splits', sr.KERNEL_CASES)
def test_backward_sums(n, hw, c, splits):
    """fte_se_lin_bwd_sums: s1, s2, dgate against float64 per [n, c] entry; two calls give the same bytes; against fte_se_bwd_gate fed
    an all-positive `out` (its mask passes everything, its g is dy) within the two bounds"""
    s = _splits(n, hw, c, splits)
    case = sr.kernel_case(n, hw, c)
    ref = sr.kernel_ref(case)
    d = _device(case)
    f = lambda k: case[k].astype(np.float64)
    b1, b2 = _sum_bound(ref['s1'], hw, ref['max_s1']), _sum_bound(ref['s2'], hw, ref['max_s2'])
    gg = f('gate') * (1 - f('gate'))
    bd = (np.abs(f('gamma')) * b2 + np.abs(f('beta')) * b1) * gg + 2 * ULP * (np.abs(f('gamma') * ref['s2']) + np.abs(f('beta') * ref['s1'])) * gg
    s1, s2, dg = _sums(d, n, hw, c)
    h = lambda t: host(t)[:n * c].reshape(n, c)
    _within(h(s1), ref['s1'], b1, 's1')
    _within(h(s2), ref['s2'], b2, 's2')
    _within(h(dg), ref['dgate'], bd, 'dgate')
    t1, t2, tg = _sums(d, n, hw, c)
    for a, b in ((s1, t1), (s2, t2), (dg, tg)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s
    m = n * hw * c
    pos = _guarded(np.ones(m, np.float32))
    g, r1, r2, rg = _out(m), _out(n * c), _out(n * c), _out(n * c)
    call('fte_se_bwd_gate', d['dy'], pos, d['z'], d['gamma'], d['beta'], d['mean'], d['rstd'], d['gate'], g, r1, r2, rg, n, hw, c, 0, stream())
    torch.cuda.synchronize()
    assert torch.equal(g[:m].view(torch.int32), d['dy'][:m].view(torch.int32)) and _intact(g, m)
    _within(h(s1), h(r1), 2 * b1, 's1 against fte_se_bwd_gate')
    _within(h(s2), h(r2), 2 * b2, 's2 against fte_se_bwd_gate')
    _within(h(dg), h(rg), 2 * bd, 'dgate against fte_se_bwd_gate')
    assert _inputs_unchanged(d, case)


def test_bad_arguments_launch_nothing():
    """a null pointer, n < 1, hw < 1, c < 4, c % 4, a null or short workspace: FTE_EINVAL, every buffer as it was"""
    bufs = [_out(4096) for _ in range(10)]
    p = [t.data_ptr() for t in bufs]
    before = [t.clone() for t in bufs]
    n, hw, c = 2, 16, 64
    need = query('fte_se_lin_ws_bytes', n, hw, c)
    assert need >= 2 * n * c * 4
    wsb, nb = ws(need)
    w_, st = wsb.data_ptr(), stream()
    wsb.fill_(7.0)
    q = query
    sq = lambda *a: q('fte_se_lin_squeeze', *a)
    assert sq(*p[:7], n, hw, c, w_, nb, st) == 0                     # (the argument list itself is good: this one runs)
    torch.cuda.synchronize()
    for t in bufs[5:7]:
        t.copy_(before[5])
    wsb.fill_(7.0)
    for dims in ((0, hw, c), (n, 0, c), (n, hw, 0), (n, hw, 2), (n, hw, 6), (n, hw, 62)):
        assert sq(*p[:7], *dims, w_, nb, st) == EINVAL
        assert q('fte_se_lin_apply_fwd', *p[:6], *dims, st) == EINVAL
        assert q('fte_se_lin_bwd_sums', *p[:10], *dims, w_, nb, st) == EINVAL
    assert sq(*p[:7], n, hw, c, None, nb, st) == EINVAL and sq(*p[:7], n, hw, c, w_, need - 4, st) == EINVAL
    assert q('fte_se_lin_bwd_sums', *p[:10], n, hw, c, None, nb, st) == EINVAL
    assert q('fte_se_lin_bwd_sums', *p[:10], n, hw, c, w_, need - 4, st) == EINVAL
    for k in (0, 1, 2, 5):                                            # z, scale, shift, sq (mean / rstd / xm are optional together)
        a = list(p[:7]); a[k] = None
        assert sq(*a, n, hw, c, w_, nb, st) == EINVAL
    a = list(p[:7]); a[3] = None                                      # xm wanted without mean
    assert sq(*a, n, hw, c, w_, nb, st) == EINVAL
    for k in range(6):
        a = list(p[:6]); a[k] = None
        assert q('fte_se_lin_apply_fwd', *a, n, hw, c, st) == EINVAL
    for k in range(10):
        a = list(p[:10]); a[k] = None
        assert q('fte_se_lin_bwd_sums', *a, n, hw, c, w_, nb, st) == EINVAL
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    assert bool((wsb == 7.0).all())
