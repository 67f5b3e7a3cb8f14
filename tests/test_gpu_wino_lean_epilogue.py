"""-m gpu: the lean epilogues of the Winograd products (csrc/wino.hip wino_mm_kernel<.., .., LEAN>) and the residual-block walk that
uses them (fte_conv3x3_fwd_keep_act, nets/sphere.py).

A residual block's first conv writes z only and the second conv's tile transform applies the PReLU to that z; the data gradient of a
block's second conv has neither ADD nor RAW.  Both must give what the generic path gives -- `==` on every tensor, which lets only the
sign of a zero differ (the generic epilogue adds the absent tensor's 0.0) -- and both paths are held to the float64 oracle at the 2e-5
of tests/test_gpu_wino.py.  FTE_WINO_LEAN=0 (read by the library at every call, and by the net when it is constructed) is the old path."""
import os

import numpy as np
import pytest
import torch

from oracle import ops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, dev, host, stream, ws, check_maxabs, check_rell2
    from tf_face_toolbox_amd import _lib, net_select, Singular

WINOGRAD = 1

# n, h, w, c (cin = cout): at 128 channels there are two column blocks
CASES = [
    (3, 7, 7, 128),       # 48 tiles: one partly filled row block; odd size: the out-of-range offsets are used
    (5, 7, 7, 128),       # 80 tiles: the second row block partly filled
    (2, 6, 6, 128),       # even size, 18 tiles
    (2, 8, 8, 64),        # the 64-channel class: one column block (the planner takes ops 0 and 2 of it: _algo below)
]
# every case above is less than half a round of tiles on 256 CUs: the half-tile kernels <e,1,1>.  This one is 131 row blocks x 2 column
# blocks = 262 whole tiles <e,2,1>: resident blocks with a second tile (the wait that leaves the epilogue's 8 stores in flight) at an odd
# size.  Against the generic kernels only: they are held to the oracle at whole tiles by tests/test_gpu_wino.py, and `==` passes it on.
WHOLE = (524, 7, 7, 128)


class _env(object):
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = os.environ.get('FTE_WINO_LEAN')
        os.environ['FTE_WINO_LEAN'] = self.value

    def __exit__(self, *a):
        if self.prev is None:
            del os.environ['FTE_WINO_LEAN']
        else:
            os.environ['FTE_WINO_LEAN'] = self.prev


def _symbols(fn):
    call('fte_prof_enable', 1)
    fn()
    torch.cuda.synchronize()
    call('fte_prof_enable', 0)
    return [r[5] for r in _lib.prof_records(shapes=True)]


def _algo(n, h, w, c, ops_):
    """the planner (auto) must take the Winograd algorithm for these ops of the shape: a direct plan fails the test, it does not skip it"""
    assert query('fte_get_conv_algo') == 2, 'the tests run under FTE_CONV_AUTO'
    for op in ops_:
        assert query('fte_conv3x3_algo', n, h, w, c, c, 1, op) == WINOGRAD, 'the planner reports direct for op %d of %s' % (op, (n, h, w, c))


def _block_inputs(n, h, w, c, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, h, w, c))                                  # the block's input: the shortcut of its second conv
    w1 = r.standard_normal((3, 3, c, c)) * 0.05; w2 = r.standard_normal((3, 3, c, c)) * 0.05
    a1 = 0.25 + 0.1 * r.standard_normal(c); a2 = 0.25 + 0.1 * r.standard_normal(c)
    a1[1] = -0.3; a1[2] = 0.0                                            # slopes whose products change sign / vanish
    return x, w1, w2, a1, a2


def _run_block(n, h, w, c, t, new):
    """conv1 -> conv2 of a residual block (nets/sphere.py:38-45: no biases) by the new calls or by fte_conv3x3_fwd_keep"""
    x, w1, w2, a1, a2 = t
    shape = (n, h, w, c)
    z1, z2, y2 = (torch.full(shape, 7.0, device='cuda') for _ in range(3))
    nv = query('fte_wino_pack_bytes', n, h, w, c) // 4
    v1, v2 = torch.full((nv,), 7.0, device='cuda'), torch.full((nv,), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_fwd_ws_bytes', n, h, w, c, c, 1))
    dims = (n, h, w, c, c, 1)
    s1 = s2 = []
    if new:
        s1 = _symbols(lambda: call('fte_conv3x3_fwd_keep_act', x, None, w1, None, a1, None, z1, None, *dims, v1, wsb, nb, stream()))
        s2 = _symbols(lambda: call('fte_conv3x3_fwd_keep_act', z1, a1, w2, None, a2, x, z2, y2, *dims, v2, wsb, nb, stream()))
        assert s1 and all(s.startswith('wino_mm_kernel<0,') and s.endswith(',1>') and s.count(',') == 2 for s in s1), s1      # lean
        assert s2 and all(s.startswith('wino_mm_kernel<0,') and s.count(',') == 1 for s in s2), s2                            # generic
    else:
        y1 = torch.full(shape, 7.0, device='cuda')
        call('fte_conv3x3_fwd_keep', x, w1, None, a1, None, z1, y1, *dims, v1, wsb, nb, stream())
        call('fte_conv3x3_fwd_keep', y1, w2, None, a2, x, z2, y2, *dims, v2, wsb, nb, stream())
    torch.cuda.synchronize()
    return z1, z2, y2, v2, s1 + s2


def _same(a, b, what):
    assert bool((a == b).all()), '%s differs: %d elements, max |diff| %.3e' % (what, int((a != b).sum()), float((a - b).abs().max()))


@pytest.mark.parametrize('n,h,w,c', CASES + [WHOLE])
def test_block_forward_equals_the_walk_that_writes_y(n, h, w, c):
    _algo(n, h, w, c, (0, 2))
    t = tuple(dev(a) for a in _block_inputs(n, h, w, c, 31))
    new = _run_block(n, h, w, c, t, True)
    old = _run_block(n, h, w, c, t, False)
    for a, b, what in zip(new, old, ('z of the first conv', 'z of the second conv', 'y of the second conv', 'V pack of the second conv')):
        _same(a, b, what)
    if (n, h, w, c) == WHOLE:
        assert new[4] == ['wino_mm_kernel<0,2,1>', 'wino_mm_kernel<0,2>'], new[4]


@pytest.mark.parametrize('n,h,w,c', CASES)
def test_block_forward_against_the_oracle(n, h, w, c):
    _algo(n, h, w, c, (0, 2))
    x, w1, w2, a1, a2 = _block_inputs(n, h, w, c, 31)
    z1_ref = ops.conv2d_fwd(x, w1, 1)
    # the second conv sees the fp32 z of the first: its kink (sign of z) is the device's, as in __graft_entry__.smoke
    for new in (True, False):
        z1, z2, y2, _, _ = _run_block(n, h, w, c, tuple(dev(a) for a in (x, w1, w2, a1, a2)), new)
        check_maxabs(host(z1), z1_ref, what='z1 (new=%s)' % new)
        y1 = ops.prelu_fwd(host(z1), a1)
        z2_ref = ops.conv2d_fwd(y1, w2, 1)
        check_maxabs(host(z2), z2_ref, what='z2 (new=%s)' % new)
        check_maxabs(host(y2), ops.prelu_fwd(host(z2), a2) + x, what='y2 (new=%s)' % new)


def _dgrad_inputs(n, h, w, c, seed):
    r = np.random.default_rng(seed)
    dz = r.standard_normal((n, h, w, c)); wt = r.standard_normal((3, 3, c, c)) * 0.05
    zprev = r.standard_normal((n, h, w, c)); alp = 0.25 + 0.1 * r.standard_normal(c)
    zprev[0, 0, 0, :4] = 0.0
    return dz, wt, zprev, alp


def _run_dgrad(n, h, w, c, t, lean):
    """the data gradient of a block's second conv (nets/sphere.py _body_walk: no addin, no raw; dalpha of the first conv, no bias)"""
    dz, wt, zprev, alp = t
    dzp = torch.full((n, h, w, c), 7.0, device='cuda')
    da, db = torch.full((c,), 7.0, device='cuda'), torch.full((c,), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_dgrad_ws_bytes', n, h, w, c, c, 1))
    with _env('1' if lean else '0'):
        syms = _symbols(lambda: call('fte_conv3x3_dgrad', dz, wt, None, zprev, alp, None, dzp, da, db, n, h, w, c, c, 1, wsb, nb, stream()))
    assert syms and all(s.startswith('wino_mm_kernel<1,') and s.count(',') == (2 if lean else 1) for s in syms), (lean, syms)
    return dzp, da, db, syms


@pytest.fixture
def winograd():
    prev = query('fte_get_conv_algo')
    call('fte_set_conv_algo', WINOGRAD)
    yield
    call('fte_set_conv_algo', prev)


def _dgrad_case(n, h, w, c, oracle):
    t = _dgrad_inputs(n, h, w, c, 32)
    td = tuple(dev(a) for a in t)
    lean = _run_dgrad(n, h, w, c, td, True)
    gen = _run_dgrad(n, h, w, c, td, False)
    for a, b, what in zip(lean, gen, ('dz', 'dalpha row', 'dbias row')):
        _same(a, b, what)
    if oracle:
        dz, wt, zprev, alp = t
        g_ref, _ = ops.conv2d_bwd(np.zeros((n, h, w, c)), wt, dz, 1, need_dw=False)
        dzp_ref, da_ref = ops.prelu_bwd(zprev, alp, g_ref)
        for dzp, da, db, _ in (lean, gen):
            check_maxabs(host(dzp), dzp_ref, what='dzprev')
            check_rell2(host(da), da_ref, what='dalpha'); check_rell2(host(db), dzp_ref.sum(axis=(0, 1, 2)), what='dbias')
    return lean[3]


@pytest.mark.parametrize('n,h,w,c', CASES[:3] + [WHOLE])
def test_lean_data_gradient_equals_the_generic_one(n, h, w, c):
    _algo(n, h, w, c, (1,))
    syms = _dgrad_case(n, h, w, c, oracle=(n, h, w, c) != WHOLE)
    if (n, h, w, c) == WHOLE:
        assert syms == ['wino_mm_kernel<1,2,1>'], syms


def test_lean_data_gradient_at_64_channels(winograd):
    """the planner keeps the 64-channel data gradient direct; the kernel takes the shape under FTE_CONV_WINOGRAD (one column block)"""
    n, h, w, c = CASES[3]
    assert query('fte_conv3x3_algo', n, h, w, c, c, 1, 1) == WINOGRAD
    _dgrad_case(n, h, w, c, oracle=True)


def test_new_entry_point_fails_rather_than_falling_back():
    """no kept pack, no result, or an algorithm that is not Winograd: an error code and no launch -- the direct and the bf16 paths need y"""
    n, h, w, c = CASES[0]
    t = lambda *s: torch.full(s, 7.0, device='cuda')
    x, wt, al, z, y = t(n, h, w, c), t(3, 3, c, c), t(c), t(n, h, w, c), t(n, h, w, c)
    v = t(query('fte_wino_pack_bytes', n, h, w, c) // 4)
    wsb, nb = ws(query('fte_conv3x3_fwd_ws_bytes', n, h, w, c, c, 1))
    dims = (n, h, w, c, c, 1)
    P = lambda q: q.data_ptr() if q is not None else 0
    fwd = lambda x_, xa, z_, y_, v_, nb_: query('fte_conv3x3_fwd_keep_act', P(x_), P(xa), P(wt), 0, P(al), 0, P(z_), P(y_), *dims, P(v_), P(wsb), nb_, 0)
    EINVAL, EWORKSPACE = -1, -2
    syms = _symbols(lambda: [
        _expect(fwd(x, al, z, y, None, nb), EINVAL, 'no pack'),
        _expect(fwd(x, al, None, None, v, nb), EINVAL, 'neither z nor y'),
        _expect(fwd(x, al, z, None, v, 4096), EWORKSPACE, 'workspace too small for the filters'),
    ])
    prev = query('fte_get_conv_algo')
    try:
        call('fte_set_conv_algo', 0)
        syms += _symbols(lambda: _expect(fwd(x, al, z, None, v, nb), EWORKSPACE, 'direct plan'))
        call('fte_set_conv_algo', prev)
        call('fte_set_mfma_dtype', 1)
        syms += _symbols(lambda: _expect(fwd(x, al, z, None, v, nb), EWORKSPACE, 'bf16 operands'))
    finally:
        call('fte_set_mfma_dtype', 0)
        call('fte_set_conv_algo', prev)
    assert syms == [], syms
    assert all(bool((o == 7.0).all()) for o in (z, y, v)), 'a refused call wrote'


def _expect(got, want, what):
    assert got == want, '%s: return code %d, expected %d' % (what, got, want)


def _train(lean, steps=3):
    n, h, w, ch, ncls = 8, 40, 24, 3, 10              # stages of 20x12, 10x6, 5x3 (odd), 3x2
    from oracle import spherenet as osn
    p = osn.perturb_params(osn.init_params(11, ch, ncls, h, w), 12)
    r = np.random.default_rng(5)
    devc = torch.device('cuda:0')
    with _env('1' if lean else '0'):
        net = net_select('SphereNet-ASoftmax', 'NCHW', 5e-4)
        net.build(h, w, ch, ncls, devc)
        net.load_params(p)
        inputs = {'images': torch.tensor(r.uniform(-1, 1, (n, h, w, ch)), dtype=torch.float32, device=devc),
                  'labels': torch.tensor(r.integers(0, ncls, n), dtype=torch.int32, device=devc), 'num_classes': ncls, 'num_examples': n}
        step, losses, names, others = Singular(net, 0.1, 'Momentum')(inputs)
        hist = []
        for _ in range(steps):
            step()
            torch.cuda.synchronize()
            hist.append([float(t) for t in losses])
        # the walk that ran: every block of the net is lean, and its first conv's y exists only on the old walk
        assert sum(net.lean) == 8, net.lean
        firsts = [l - 1 for l, f in enumerate(net.lean) if f]
        assert all((net.y[l] is None) == lean for l in firsts), [net.y[l] is None for l in firsts]
        return hist, {k: net.get_variable(k).clone() for k in net.variables}


def test_whole_net_three_steps_equal_the_old_walk():
    new_l, new_v = _train(True)
    old_l, old_v = _train(False)
    assert new_l == old_l, (new_l, old_l)
    assert all(np.isfinite(v) for s_ in new_l for v in s_), new_l
    for k in new_v:
        _same(new_v[k], old_v[k], k)
