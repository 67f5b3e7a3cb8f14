"""-m gpu: the first conv (fte_conv3x3_first_fwd, _fwd_s16, _wgrad, _wgrad_s16 and the workspace query) through the C ABI at the shapes
its two kernels and the reduction of its partial rows branch on.  The cases are tests/dense_ref.py's; tests/test_dense_cases_host.py
proves on the CPU which branch each one takes (32-pixel groups per row and their last group, the pads, blocks, rows per block, trips
per wave, blocks and waves without a row, the k_reduce_rows2 plan of the partial rows).  The launch profiler does not record these
kernels.  References are the float64 oracle.ops.conv2d_fwd / conv2d_bwd on the float32 inputs; outputs are NaN-poisoned and canaried,
inputs must come back bit for bit, the workspace is exactly the query's size plus a canary, two calls must give the same bytes."""
import time

import numpy as np
import pytest
import torch

from oracle import ops

import dense_ref as D
from test_gpu_arena_edges import _guarded, _intact
from test_gpu_layers_edges import _out, _out16, _in16, _intact16, _stored16, _unchanged

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, host, stream, check_maxabs, TOL_MAXABS

EINVAL, EWORKSPACE = -1, -2


def _same_bytes(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _ws_exact(nbytes):
    assert nbytes % 4 == 0
    return _guarded(np.full(nbytes // 4, np.nan, np.float32))


def _ids(c):
    return 'x'.join(str(v) for v in c)


def _fwd_refs(case, inp, bias, alpha):
    stride = case[5]
    z = ops.conv2d_fwd(inp['x'].astype(np.float64), inp['w'].astype(np.float64), stride, inp['b'].astype(np.float64) if bias else None)
    return z, (ops.prelu_fwd(z, inp['al'].astype(np.float64)) if alpha else z)


def _prelu_of_stored_z(zg, al):
    """what the kernel's y must be BIT FOR BIT given the z it stored: one fp32 comparison and one fp32 multiplication per element
    (z == +0 with a negative slope gives -0: the z > 0 test is strict)"""
    return np.where(zg > 0, zg, al[None, None, None, :] * zg).astype(np.float32)


def _fwd_call(case, inp, bias, alpha, want_z=True):
    n, h, w, cin, cout, stride = case
    g = D.first_fwd_geometry(case)
    cnt = n * g['ho'] * g['wo'] * cout
    xd, wd, bd, ald = _guarded(inp['x']), _guarded(inp['w']), _guarded(inp['b']), _guarded(inp['al'])
    outs = []
    for rep in range(2):
        z, y = (_out(cnt) if want_z else None), _out(cnt)
        call('fte_conv3x3_first_fwd', xd, wd, bd if bias else None, ald if alpha else None, z, y, n, h, w, cin, cout, stride, stream())
        torch.cuda.synchronize()
        assert _intact(y, cnt) and (z is None or _intact(z, cnt))
        outs.append((z, y))
    assert _same_bytes(outs[0][1], outs[1][1]) and (not want_z or _same_bytes(outs[0][0], outs[1][0]))
    assert _unchanged(xd, inp['x']) and _unchanged(wd, inp['w']) and _unchanged(bd, inp['b']) and _unchanged(ald, inp['al'])
    shape = (n, g['ho'], g['wo'], cout)
    z, y = outs[0]
    return (None if z is None else z[:cnt].cpu().numpy().reshape(shape)), y[:cnt].cpu().numpy().reshape(shape)


@pytest.mark.parametrize('case', D.FIRST_FWD_CASES, ids=_ids)
def test_first_conv_forward(case):
    inp = D.first_inputs(case)
    z_ref, y_ref = _fwd_refs(case, inp, True, True)
    zg, yg = _fwd_call(case, inp, True, True)
    check_maxabs(zg, z_ref, TOL_MAXABS, 'z'); check_maxabs(yg, y_ref, TOL_MAXABS, 'y')
    np.testing.assert_array_equal(yg.view(np.uint32), _prelu_of_stored_z(zg, inp['al']).view(np.uint32))


def test_first_conv_forward_optional_bias_alpha_and_z():
    """the four bias / alpha presence combinations, and z absent.  Without a bias output pixel (0, 0) of image 0 is exactly +0 (its window
    is zero): y there must be alpha * 0, i.e. -0 under a negative slope -- the strict side of the PReLU's comparison."""
    case = D.FIRST_COMBO_CASE
    inp = D.first_inputs(case)
    assert (inp['al'] < 0).sum() >= 8 and (inp['al'] > 0).sum() >= 8
    for bias in (True, False):
        for alpha in (True, False):
            z_ref, y_ref = _fwd_refs(case, inp, bias, alpha)
            zg, yg = _fwd_call(case, inp, bias, alpha)
            what = 'bias %d alpha %d' % (bias, alpha)
            check_maxabs(zg, z_ref, TOL_MAXABS, what + ': z'); check_maxabs(yg, y_ref, TOL_MAXABS, what + ': y')
            want = _prelu_of_stored_z(zg, inp['al']) if alpha else zg
            np.testing.assert_array_equal(yg.view(np.uint32), want.view(np.uint32), err_msg=what)
            if not bias:
                assert (zg[0, 0, 0].view(np.uint32) == 0).all(), what
                if alpha:
                    assert (np.signbit(yg[0, 0, 0]) == (inp['al'] < 0)).all(), what
    z_ref, y_ref = _fwd_refs(case, inp, True, True)
    _, yg = _fwd_call(case, inp, True, True, want_z=False)
    check_maxabs(yg, y_ref, TOL_MAXABS, 'y without z')


@pytest.mark.parametrize('case', D.FIRST_S16_FWD, ids=_ids)
def test_first_conv_forward_bf16_storage(case):
    n, h, w, cin, cout, stride = case
    inp = D.first_inputs(case)
    z_ref, y_ref = _fwd_refs(case, inp, True, True)
    cnt = z_ref.size
    xd, wd, bd, ald = _guarded(inp['x']), _guarded(inp['w']), _guarded(inp['b']), _guarded(inp['al'])
    outs = []
    for rep in range(2):
        z16, y16 = _out16(cnt), _out16(cnt)
        call('fte_conv3x3_first_fwd_s16', xd, wd, bd, ald, z16, y16, n, h, w, cin, cout, stride, stream())
        torch.cuda.synchronize()
        assert _intact16(z16, cnt) and _intact16(y16, cnt)
        _stored16(z16[:cnt], z_ref, 'z16'); _stored16(y16[:cnt], y_ref, 'y16')
        outs.append((z16, y16))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    y16 = _out16(cnt)
    call('fte_conv3x3_first_fwd_s16', xd, wd, bd, ald, None, y16, n, h, w, cin, cout, stride, stream())          # z16 absent
    torch.cuda.synchronize()
    assert torch.equal(y16, outs[0][1])
    assert _unchanged(xd, inp['x']) and _unchanged(wd, inp['w']) and _unchanged(bd, inp['b']) and _unchanged(ald, inp['al'])


def _wgrad(case, x, dz, entry='fte_conv3x3_first_wgrad'):
    """two calls with exact, NaN-poisoned workspaces -> (dw float32 [3, 3, cin, cout] of the first, its device buffer, its workspace)"""
    n, h, w, cin, cout, stride = case
    nb = query('fte_conv3x3_first_wgrad_ws_bytes', n, h, w, cin, cout, stride)
    assert nb == D.first_wgrad_ws_bytes(case)
    cnt = 9 * cin * cout
    xd = _guarded(x)
    dzd = _in16(dz) if entry.endswith('_s16') else _guarded(dz)
    outs = []
    for rep in range(2):
        dw, wsb = _out(cnt), _ws_exact(nb)
        call(entry, xd, dzd, dw, n, h, w, cin, cout, stride, wsb, nb, stream())
        torch.cuda.synchronize()
        assert _intact(dw, cnt) and _intact(wsb, nb // 4)
        outs.append((dw, wsb))
    assert _same_bytes(outs[0][0], outs[1][0])
    assert _unchanged(xd, x) and (_intact16(dzd, dz.size) if entry.endswith('_s16') else _unchanged(dzd, dz))
    return outs[0][0][:cnt].cpu().numpy().reshape(3, 3, cin, cout), outs[0][0], outs[0][1]


def _check_wgrad(case, got, x, dz, what):
    n, h, w, cin, cout, stride = case
    g = D.first_wgrad_geometry(case)
    ref, sabs = D.first_wgrad_ref(x, dz, stride)
    check_maxabs(got, ref, TOL_MAXABS, what)
    bound = D.sum_bound(n * g['ho'] * g['wo'], sabs)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), (what, 'beyond the order-free bound', float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize('case', D.FIRST_FWD_CASES + D.FIRST_WGRAD_BIG, ids=_ids)
def test_first_conv_filter_gradient(case):
    n, h, w, cin, cout, stride = case
    g = D.first_wgrad_geometry(case)
    x, dz = D.first_inputs(case)['x'], D.first_dz(case)
    got, _, wsb = _wgrad(case, x, dz)
    _check_wgrad(case, got, x, dz, 'dw')
    # the partial rows: every block writes its own, the blocks without an output row write zeros
    part = wsb[:g['blocks'] * g['cols']].cpu().numpy().reshape(g['blocks'], g['cols'])
    assert np.isfinite(part).all()
    used = g['blocks'] - g['empty_blocks']
    assert (part[used:] == 0).all() and (g['empty_blocks'] == 0 or np.abs(part[used - 1]).max() > 0)


def test_first_conv_filter_gradient_block_cap():
    """1.05 M output pixels: 2048 partial rows (the cap of every headline step), 480 of them zeros, summed by the two-pass
    reduce_rows_q_kernel plan.  The one large case: dz is 135 MB."""
    case = D.FIRST_WGRAD_CAP
    g = D.first_wgrad_geometry(case)
    assert g['blocks'] == D.FIRST_WGRAD_BLOCK_CAP
    x, dz = D.first_inputs(case)['x'], D.first_dz(case)
    t0 = time.perf_counter()
    got, _, wsb = _wgrad(case, x, dz)
    print('block cap case: upload + two calls + checks of the buffers %.2f s' % (time.perf_counter() - t0))
    _check_wgrad(case, got, x, dz, 'dw at the block cap')
    part = wsb[:g['blocks'] * g['cols']].cpu().numpy().reshape(g['blocks'], g['cols'])
    used = g['blocks'] - g['empty_blocks']
    assert np.isfinite(part).all() and (part[used:] == 0).all() and np.abs(part[used - 1]).max() > 0


@pytest.mark.parametrize('case', D.FIRST_S16_WGRAD, ids=_ids)
def test_first_conv_filter_gradient_from_bf16_dz(case):
    """on a bf16-exact dz the bf16-source entry point equals the fp32 one bit for bit"""
    x, dz = D.first_inputs(case)['x'], D.first_dz(case, bf16_exact=True)
    got16, buf16, _ = _wgrad(case, x, dz, 'fte_conv3x3_first_wgrad_s16')
    got32, buf32, _ = _wgrad(case, x, dz)
    assert _same_bytes(buf16, buf32)
    _check_wgrad(case, got16, x, dz, 'dw from bf16 dz')


def test_bad_arguments_launch_nothing():
    """stride 0 (same_pads divides by it) and 3, n = 0, h = 0, w = 0, cin = 2, cout = 48: FTE_EINVAL and a query of 0; a workspace four
    bytes short or absent: the workspace error; every buffer as it was"""
    bufs = [_out(8192) for _ in range(6)]
    p = [t.data_ptr() for t in bufs]
    before = [t.clone() for t in bufs]
    good = (1, 8, 8, 3, 64, 1)
    need = query('fte_conv3x3_first_wgrad_ws_bytes', *good)
    assert need == D.first_wgrad_ws_bytes(good)
    wsb = _guarded(np.full(need // 4, 7.0, np.float32))
    w0 = wsb.clone()
    w_, st, q = wsb.data_ptr(), stream(), query
    for dims in ((1, 8, 8, 3, 64, 0), (1, 8, 8, 3, 64, 3), (1, 8, 8, 3, 64, -2), (0, 8, 8, 3, 64, 1), (1, 0, 8, 3, 64, 1), (1, 8, 0, 3, 64, 2),
                 (-1, 8, 8, 3, 64, 1), (1, 8, 8, 2, 64, 1), (1, 8, 8, 3, 48, 1)):
        assert q('fte_conv3x3_first_fwd', p[0], p[1], p[2], p[3], p[4], p[5], *dims, st) == EINVAL, dims
        assert q('fte_conv3x3_first_fwd_s16', p[0], p[1], p[2], p[3], p[4], p[5], *dims, st) == EINVAL, dims
        assert q('fte_conv3x3_first_wgrad', p[0], p[1], p[2], *dims, w_, need, st) == EINVAL, dims
        assert q('fte_conv3x3_first_wgrad_s16', p[0], p[1], p[2], *dims, w_, need, st) == EINVAL, dims
        assert q('fte_conv3x3_first_wgrad_ws_bytes', *dims) == 0, dims
    for entry in ('fte_conv3x3_first_wgrad', 'fte_conv3x3_first_wgrad_s16'):
        assert q(entry, p[0], p[1], p[2], *good, w_, need - 4, st) == EWORKSPACE
        assert q(entry, p[0], p[1], p[2], *good, None, need, st) == EWORKSPACE
        assert q(entry, p[0], None, p[2], *good, w_, need, st) == EINVAL
    assert q('fte_conv3x3_first_fwd', p[0], p[1], p[2], p[3], p[4], None, *good, st) == EINVAL          # y is not optional
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert _same_bytes(t, b)
    assert _same_bytes(wsb, w0)
