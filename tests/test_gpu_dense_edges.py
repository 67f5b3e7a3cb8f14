"""-m gpu: the dense products (fte_gemm_nn, fte_gemm_nn_act, fte_gemm_nt plain and with the fused PReLU backward, fte_gemm_tn) through
the C ABI at the shapes their plans branch on.  The cases, their plan columns and the branch each one is in the table for are
tests/dense_ref.py's; tests/test_dense_cases_host.py proves on the CPU that the table hits those branches.  Here every call runs with
NaN-poisoned outputs followed by a canary, inputs that must come back bit for bit, a workspace of exactly fte_gemm_ws_bytes(m, n, k)
bytes followed by a canary, twice (the sums are ordered: the same bytes both times), and with the launch records on: the kernel symbol's
tile, the split count and the GEMM dimensions of the record are asserted, so that a change of plan cannot silently move a case off its
branch.  References are float64 numpy on the float32 inputs, held to util_gpu.TOL_MAXABS / TOL_RELL2, and for every element of a tn
product and of dalpha also to the order-free bound dense_ref.sum_bound (derived there, not measured)."""
import numpy as np
import pytest
import torch

from oracle import ops

import dense_ref as D
from test_gpu_arena_edges import CANARY, _guarded, _intact
from test_gpu_layers_edges import _out, _unchanged

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, host, stream, check_maxabs, check_rell2, TOL_MAXABS, TOL_RELL2
    from tf_face_toolbox_amd import _lib

EINVAL, EWORKSPACE = -1, -2
AL_MK, AL_KM, BL_KN, BL_NK, EPI_FWD, EPI_DGRAD = 0, 1, 0, 1, 0, 1          # csrc/igemm.h, csrc/conv_plan.h
OPERANDS = {'nn': (AL_MK, BL_KN), 'nt': (AL_MK, BL_NK), 'tn': (AL_KM, BL_KN)}
BF16_TOL = 2e-5          # test_dense_small_one_launch_layers' limit against float64 on the bf16-rounded operands


def _ws_exact(nbytes):
    """a NaN workspace of exactly `nbytes` bytes with the canary behind it"""
    assert nbytes % 4 == 0
    return _guarded(np.full(nbytes // 4, np.nan, np.float32))


def _recorded(fn):
    query('fte_prof_enable', 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        query('fte_prof_enable', 0)
    return _lib.prof_records(shapes=True)


def _same_bytes(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_record(recs, c, tile, splits, epi=EPI_FWD, bf16=False):
    """one launch of the igemm family: operand layouts, epilogue, tile, split count, the GEMM's dimensions, the symbol's tile"""
    assert len(recs) == 1, recs
    sig, _, _, mnk, _, sym = recs[0]
    rows, cols, red = D.gemm_dims(c)
    assert tuple(sig) == OPERANDS[c.product] + (epi, tile, splits), (c.name, sig, sym)
    assert tuple(mnk) == (rows, cols, red), (c.name, mnk)
    assert sym, (c.name, 'no kernel symbol recorded')
    if sym.startswith('igemm_kernel<'):
        targs = [int(v) for v in sym[len('igemm_kernel<'):-1].split(',')]
        assert tuple(targs[:2]) == D.TILE_DIMS[tile] and targs[4:7] == list(OPERANDS[c.product]) + [epi] and targs[7] == (1 if bf16 else 0), sym
    else:
        assert bf16, sym            # the fp32 products have one kernel family


def _operands(inp, bf16):
    """float64 views of the float32 inputs, rounded to bf16 where the MFMA operands are"""
    rd = (lambda a: ops.bf16_round(a).astype(np.float64)) if bf16 else (lambda a: a.astype(np.float64))
    return {k: rd(v) for k, v in inp.items()}


def _run_nn(c, inp, bias, act, entry, tile, splits, bf16=False):
    m, n, k = c.m, c.n, c.k
    o = _operands(inp, bf16)
    lin = o['x'] @ o['w'] + (inp['b'].astype(np.float64) if bias else 0.0)
    ref = D.act_ref(lin, act)
    nb = query('fte_gemm_ws_bytes', m, n, k)
    assert nb >= D.dense_need_bytes(c)
    xd, wd = _guarded(inp['x']), _guarded(inp['w'])
    bd = _guarded(inp['b']) if bias else None
    outs = []
    for rep in range(2):
        y, wsb = _out(m * n), _ws_exact(nb)
        if entry == 'fte_gemm_nn':
            recs = _recorded(lambda: call(entry, xd, wd, bd, y, m, n, k, wsb, nb, stream()))
        else:
            recs = _recorded(lambda: call(entry, xd, wd, bd, y, m, n, k, act, wsb, nb, stream()))
        _check_record(recs, c, tile, splits, bf16=bf16)
        what = '%s %s bias %d act %d%s' % (c.name, entry, bias, act, ' bf16' if bf16 else '')
        check_maxabs(host(y)[:m * n].reshape(m, n), ref, BF16_TOL if bf16 else TOL_MAXABS, what)
        assert _intact(y, m * n) and _intact(wsb, nb // 4), what
        outs.append(y)
    assert _same_bytes(outs[0], outs[1]), (c.name, 'two calls differ')
    assert _unchanged(xd, inp['x']) and _unchanged(wd, inp['w']) and (not bias or _unchanged(bd, inp['b']))
    return xd, wd, bd


@pytest.mark.parametrize('c', D.NN_CASES, ids=lambda c: c.name)
def test_nn_at_the_plan_branches(c):
    inp = D.dense_inputs(c)
    _run_nn(c, inp, False, 0, 'fte_gemm_nn', c.tile, c.splits)
    xd, wd, bd = _run_nn(c, inp, True, 0, 'fte_gemm_nn', c.tile, c.splits)
    if c.name in ('nn_split4_bias_act', 'nn_unsplit_act'):
        for act in (0, 1, 2):
            _run_nn(c, inp, True, act, 'fte_gemm_nn_act', c.tile, c.splits)
    need = D.dense_need_bytes(c)
    if need:            # a workspace four bytes short of the slabs: the workspace error, nothing written
        y, wsb = _out(c.m * c.n), _ws_exact(need)
        y0, w0 = y.clone(), wsb.clone()
        for ptr, nb in ((wsb.data_ptr(), need - 4), (None, need)):
            assert query('fte_gemm_nn', xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), c.m, c.n, c.k, ptr, nb, stream()) == EWORKSPACE
            assert query('fte_gemm_nn_act', xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), c.m, c.n, c.k, 1, ptr, nb, stream()) == EWORKSPACE
        torch.cuda.synchronize()
        assert _same_bytes(y, y0) and _same_bytes(wsb, w0)


def _nt_call(c, dyd, wd, zpd, ald, amod, raw, dx, da, wsb, nb):
    return _recorded(lambda: call('fte_gemm_nt', dyd, wd, zpd, ald, amod, raw, dx, da, c.m, c.n, c.k, wsb, nb, stream()))


@pytest.mark.parametrize('c', D.NT_CASES, ids=lambda c: c.name)
def test_nt_plain(c):
    inp = D.dense_inputs(c)
    m, n, k = c.m, c.n, c.k
    ref = inp['dy'].astype(np.float64) @ inp['w'].astype(np.float64).T
    nb = query('fte_gemm_ws_bytes', m, n, k)
    dyd, wd = _guarded(inp['dy']), _guarded(inp['w'])
    outs = []
    for rep in range(2):
        dx, wsb = _out(m * k), _ws_exact(nb)
        recs = _nt_call(c, dyd, wd, None, None, 0, None, dx, None, wsb, nb)
        _check_record(recs, c, c.tile, c.splits)
        check_maxabs(host(dx)[:m * k].reshape(m, k), ref, TOL_MAXABS, c.name)
        assert _intact(dx, m * k) and _intact(wsb, nb // 4)
        outs.append(dx)
    assert _same_bytes(outs[0], outs[1])
    assert _unchanged(dyd, inp['dy']) and _unchanged(wd, inp['w'])
    need = D.dense_need_bytes(c)
    if need:
        dx, wsb = _out(m * k), _ws_exact(need)
        d0, w0 = dx.clone(), wsb.clone()
        assert query('fte_gemm_nt', dyd.data_ptr(), wd.data_ptr(), None, None, 0, None, dx.data_ptr(), None, m, n, k, wsb.data_ptr(), need - 4, stream()) == EWORKSPACE
        torch.cuda.synchronize()
        assert _same_bytes(dx, d0) and _same_bytes(wsb, w0)


@pytest.mark.parametrize('c', D.NT_CASES, ids=lambda c: c.name)
def test_nt_fused_prelu_backward_pointer_sets(c):
    """the four pointer sets the API allows -- raw only; zprev + alpha; zprev + alpha + raw; all with dalpha_prev -- at amod = 64 and
    amod = k.  The reference is ops.prelu_bwd on dy @ w^T with zprev == 0 planted in the first and in the last row tile."""
    inp = D.dense_inputs(c)
    m, n, k = c.m, c.n, c.k
    tile, part_rows = D.NT_FUSED[c.name]
    g_ref = inp['dy'].astype(np.float64) @ inp['w'].astype(np.float64).T
    zp64 = inp['zp'].astype(np.float64)
    assert (inp['zp'] == 0).sum() >= 5
    nb = query('fte_gemm_ws_bytes', m, n, k)
    need = D.nt_fused_need_bytes(c)
    assert nb >= need
    dyd, wd, zpd = _guarded(inp['dy']), _guarded(inp['w']), _guarded(inp['zp'])
    for amod in sorted({64, k}):
        al = inp['al'][:amod]
        ald = _guarded(al)
        dz_ref, dal_full = ops.prelu_bwd(zp64, np.tile(al.astype(np.float64), k // amod), g_ref)
        dal_ref = dal_full.reshape(-1, amod).sum(0)
        dal_bound = D.dalpha_bound(inp['dy'], inp['w'], inp['zp'], amod)
        sets = {'raw only': (False, True, False), 'zprev': (True, False, False), 'zprev + raw': (True, True, False), 'all': (True, True, True)}
        for name, (use_z, use_raw, use_da) in sets.items():
            if not use_z and amod != 64:
                continue                     # no alpha in this set: nothing depends on amod
            what = '%s amod %d %s' % (c.name, amod, name)
            outs = []
            for rep in range(2):
                dx, wsb = _out(m * k), _ws_exact(nb)
                raw = _out(m * k) if use_raw else None
                da = _out(amod) if use_da else None
                recs = _nt_call(c, dyd, wd, zpd if use_z else None, ald if use_z else None, amod if use_z else 0, raw, dx, da, wsb, nb)
                _check_record(recs, c, tile, 1, epi=EPI_DGRAD)
                check_maxabs(host(dx)[:m * k].reshape(m, k), dz_ref if use_z else g_ref, TOL_MAXABS, what + ': dx')
                assert _intact(dx, m * k) and _intact(wsb, nb // 4), what
                if use_raw:
                    check_maxabs(host(raw)[:m * k].reshape(m, k), g_ref, TOL_MAXABS, what + ': raw')
                    assert _intact(raw, m * k), what
                if use_da:
                    got = host(da)[:amod]
                    check_rell2(got, dal_ref, TOL_RELL2, what + ': dalpha')
                    err = np.abs(got - dal_ref)
                    assert (err <= dal_bound).all(), (what, 'dalpha beyond the order-free bound', float((err / dal_bound).max()))
                    assert _intact(da, amod), what
                else:
                    assert bool(torch.isnan(wsb[:nb // 4]).all()), (what, 'workspace written without dalpha_prev')
                outs.append((dx, raw, da))
            for a, b in zip(*outs):
                assert a is None or _same_bytes(a, b), (what, 'two calls differ')
        # the partial rows' workspace at its exact size: four bytes short (or absent) is the workspace error and writes nothing
        bufs = [_out(m * k), _out(m * k), _out(amod), _ws_exact(need)]
        before = [t.clone() for t in bufs]
        dx, raw, da, wsb = bufs
        args = (dyd.data_ptr(), wd.data_ptr(), zpd.data_ptr(), ald.data_ptr(), amod, raw.data_ptr(), dx.data_ptr(), da.data_ptr(), m, n, k)
        assert query('fte_gemm_nt', *args, wsb.data_ptr(), need - 4, stream()) == EWORKSPACE
        assert query('fte_gemm_nt', *args, None, need, stream()) == EWORKSPACE
        torch.cuda.synchronize()
        assert all(_same_bytes(t, b) for t, b in zip(bufs, before))
        call('fte_gemm_nt', dyd, wd, zpd, ald, amod, raw, dx, da, m, n, k, wsb, need, stream())          # exactly what the launch needs: runs
        torch.cuda.synchronize()
        check_rell2(host(da)[:amod], dal_ref, TOL_RELL2, 'dalpha, exact workspace')
        assert _intact(wsb, need // 4) and _intact(da, amod) and _unchanged(ald, al)
    assert _unchanged(dyd, inp['dy']) and _unchanged(wd, inp['w']) and _unchanged(zpd, inp['zp'])


def _run_tn(c, inp, tile, splits, bf16=False):
    m, n, k = c.m, c.n, c.k
    o = _operands(inp, bf16)
    ref = o['x'].T @ o['dy']
    bound = D.sum_bound(m, np.abs(o['x']).T @ np.abs(o['dy']))
    nb = query('fte_gemm_ws_bytes', m, n, k)
    assert nb >= D.dense_need_bytes(c)
    xd, dyd = _guarded(inp['x']), _guarded(inp['dy'])
    outs = []
    for rep in range(2):
        dw, wsb = _out(k * n), _ws_exact(nb)
        recs = _recorded(lambda: call('fte_gemm_tn', xd, dyd, dw, m, n, k, wsb, nb, stream()))
        _check_record(recs, c, tile, splits, bf16=bf16)
        got = host(dw)[:k * n].reshape(k, n)
        check_maxabs(got, ref, BF16_TOL if bf16 else TOL_MAXABS, c.name)
        err = np.abs(got - ref)
        assert (err <= bound).all(), (c.name, 'beyond the order-free bound', float((err / bound).max()))
        assert _intact(dw, k * n) and _intact(wsb, nb // 4)
        outs.append(dw)
    assert _same_bytes(outs[0], outs[1])
    assert _unchanged(xd, inp['x']) and _unchanged(dyd, inp['dy'])
    return xd, dyd


@pytest.mark.parametrize('c', D.TN_CASES, ids=lambda c: c.name)
def test_tn_slow_gather_ragged_splits_and_rows(c):
    inp = D.dense_inputs(c)
    xd, dyd = _run_tn(c, inp, c.tile, c.splits)
    need = D.dense_need_bytes(c)
    if need:
        dw, wsb = _out(c.k * c.n), _ws_exact(need)
        d0, w0 = dw.clone(), wsb.clone()
        assert query('fte_gemm_tn', xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), c.m, c.n, c.k, wsb.data_ptr(), need - 4, stream()) == EWORKSPACE
        torch.cuda.synchronize()
        assert _same_bytes(dw, d0) and _same_bytes(wsb, w0)


@pytest.mark.parametrize('name', D.BF16_CASES)
def test_bf16_operand_mode(name):
    """bf16 MFMA operands, fp32 accumulation: against float64 on the bf16-rounded operands; tile and split count as the bf16 plan
    of the planner states them (dense_ref.BF16_PLANS, checked on the CPU), read back from the launch record"""
    c = next(v for v in D.DENSE_CASES if v.name == name)
    tile, splits = D.BF16_PLANS[name]
    inp = D.dense_inputs(c)
    prev = _lib.precision_mode()
    _lib.set_mfma_dtype('bf16')
    try:
        if c.product == 'nn':
            _run_nn(c, inp, True, 0, 'fte_gemm_nn', tile, splits, bf16=True)
            if name == 'nn_split4_bias_act':
                for act in (1, 2):
                    _run_nn(c, inp, True, act, 'fte_gemm_nn_act', tile, splits, bf16=True)
        elif c.product == 'tn':
            _run_tn(c, inp, tile, splits, bf16=True)
        else:
            m, n, k = c.m, c.n, c.k
            o = _operands({'dy': inp['dy'], 'w': inp['w']}, True)
            nb = query('fte_gemm_ws_bytes', m, n, k)
            dyd, wd = _guarded(inp['dy']), _guarded(inp['w'])
            dx, wsb = _out(m * k), _ws_exact(nb)
            recs = _nt_call(c, dyd, wd, None, None, 0, None, dx, None, wsb, nb)
            _check_record(recs, c, tile, splits, bf16=True)
            check_maxabs(host(dx)[:m * k].reshape(m, k), o['dy'] @ o['w'].T, BF16_TOL, name + ' bf16')
            assert _intact(dx, m * k) and _intact(wsb, nb // 4) and _unchanged(dyd, inp['dy']) and _unchanged(wd, inp['w'])
    finally:
        _lib.set_mfma_dtype(prev)


def test_bad_arguments_launch_nothing():
    """n = 0, k = 0, negative multiples of 64 (they pass the divisibility rules), m = 0, amod not dividing k, zprev without alpha:
    FTE_EINVAL, every buffer and the workspace as they were; the query answers 0 for the sizes no product takes"""
    bufs = [_out(4096) for _ in range(8)]
    p = [t.data_ptr() for t in bufs]
    before = [t.clone() for t in bufs]
    wsb = _guarded(np.full(1 << 19, 7.0, np.float32))
    w0 = wsb.clone()
    w_, nb, st = wsb.data_ptr(), (1 << 19) * 4, stream()
    q = query
    assert q('fte_gemm_nn', p[0], p[1], p[2], p[3], 8, 64, 64, w_, nb, st) == 0          # (the argument list itself is good)
    torch.cuda.synchronize()
    bufs[3].copy_(before[3])
    for m, n, k in ((8, 0, 64), (8, 64, 0), (8, -64, 64), (8, 64, -64), (0, 64, 64), (-8, 64, 64), (8, 0, 0)):
        assert q('fte_gemm_nn', p[0], p[1], p[2], p[3], m, n, k, w_, nb, st) == EINVAL, (m, n, k)
        assert q('fte_gemm_nn_act', p[0], p[1], p[2], p[3], m, n, k, 1, w_, nb, st) == EINVAL, (m, n, k)
        assert q('fte_gemm_nt', p[0], p[1], None, None, 0, None, p[3], None, m, n, k, w_, nb, st) == EINVAL, (m, n, k)
        assert q('fte_gemm_nt', p[0], p[1], p[2], p[4], 64, p[5], p[3], p[6], m, n, k, w_, nb, st) == EINVAL, (m, n, k)
        assert q('fte_gemm_tn', p[0], p[1], p[3], m, n, k, w_, nb, st) == EINVAL, (m, n, k)
        assert q('fte_gemm_ws_bytes', m, n, k) == 0, (m, n, k)
    assert q('fte_gemm_nt', p[0], p[1], p[2], p[4], 48, p[5], p[3], p[6], 8, 64, 64, w_, nb, st) == EINVAL          # amod does not divide k
    assert q('fte_gemm_nt', p[0], p[1], p[2], p[4], 0, p[5], p[3], p[6], 8, 64, 64, w_, nb, st) == EINVAL
    assert q('fte_gemm_nt', p[0], p[1], p[2], None, 64, p[5], p[3], p[6], 8, 64, 64, w_, nb, st) == EINVAL         # zprev without alpha
    assert q('fte_gemm_nn', p[0], p[1], p[2], p[3], 8, 96, 64, w_, nb, st) == EINVAL and q('fte_gemm_tn', p[0], p[1], p[3], 8, 64, 6, w_, nb, st) == EINVAL
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert _same_bytes(t, b)
    assert _same_bytes(wsb, w0)
