"""Child process of tests/test_gpu_tiles.py: runs fte_conv3x3_{fwd,dgrad,wgrad} through the C ABI on one case list and compares
every result with the float64 oracle (oracle/ops.py), image block by image block so that the production sizes of the headline run
(hundreds of 56x56 / 28x28 images) fit the host.  The tile / split-K hooks of csrc/conv_plan.h are read ONCE per process
(FTE_WGRAD_TILE, FTE_WGRAD_SPLIT_MAJOR, ...), hence a process per environment.

    python tests/tile_worker.py '[["wgrad", n, h, w, cin, cout, stride], ["fwd", ...], ["dgrad", ...]]'

The case kinds 'bnfwd1' / 'bnfold1' run fte_conv2d_bn_fwd of a 1x1 conv under bf16 storage, plain / with the BN in front folded in (the
FTE_PW16_* hooks of csrc/pw16.hip are read once per process too); their checks are the functions tests/test_gpu_pw16_edges.py calls
in-process for the default environment.

The bf16-storage kinds ('s16fwd', 's16dgrad', 's16fwd1', 's16dgrad1', 's16wgrad', 's16wgrad1') poison what they hand to the library: every bf16
output holds CANARY16 and carries GUARD rows behind row M, dalpha / dbias / dw hold NaN, the workspace is NaN with 4 KB behind the granted
bytes -- a guard row that changed, a canary left inside or a changed workspace tail fails the case.  's16fwdx' / 's16dgradx' are the
EXACT-PLACEMENT kinds of a 3x3 conv (tests/win16_map.py: position-coded input, one power of two per output channel): the stored tensor must
equal the tap-shifted input bit for bit.

Prints one JSON line: {"cases": [{"case": [...], "symbols": [...kernel symbols the launch records name...], "splits": [...],
"errors": {...}}], "ok": true|false}.  Tolerances are tests/util_gpu.py's (2e-5 max-abs / rel-L2 against float64)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import win16_map                                           # noqa: E402
from oracle import ops                                     # noqa: E402
from tf_face_toolbox_amd import _lib                       # noqa: E402
from util_gpu import call, query, stream, ws, TOL_MAXABS, TOL_RELL2      # noqa: E402

BLOCK = 8           # images per oracle block


def _maxabs(got, ref):
    return float(np.abs(got - ref).max()), float(np.abs(ref).max())


def _records():
    torch.cuda.synchronize()
    recs = _lib.prof_records(shapes=True)
    return sorted({r[5] for r in recs}), [r[0][4] for r in recs]


def run_fwd(n, h, w, cin, cout, stride, r):
    x = r.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (r.standard_normal((3, 3, cin, cout), dtype=np.float32) * 0.05).astype(np.float32)
    b = r.standard_normal(cout, dtype=np.float32)
    al = (0.25 + 0.1 * r.standard_normal(cout, dtype=np.float32)).astype(np.float32)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    res = r.standard_normal((n, ho, wo, cout), dtype=np.float32)
    z = torch.empty(n, ho, wo, cout, device='cuda'); y = torch.empty_like(z)
    wsb, nb = ws(query('fte_conv3x3_fwd_ws_bytes', n, h, w, cin, cout, stride))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv3x3_fwd', torch.from_numpy(x).cuda(), torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(al).cuda(),
         torch.from_numpy(res).cuda(), z, y, n, h, w, cin, cout, stride, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    zg, yg = z.cpu().numpy(), y.cpu().numpy()
    ez = ey = sz = sy = 0.0
    w64, b64, al64 = wt.astype(np.float64), b.astype(np.float64), al.astype(np.float64)
    for i in range(0, n, BLOCK):
        zr = ops.conv2d_fwd(x[i:i + BLOCK].astype(np.float64), w64, stride, b64)
        yr = ops.prelu_fwd(zr, al64) + res[i:i + BLOCK]
        e, s = _maxabs(zg[i:i + BLOCK], zr); ez = max(ez, e); sz = max(sz, s)
        e, s = _maxabs(yg[i:i + BLOCK], yr); ey = max(ey, e); sy = max(sy, s)
    errs = {'z_maxabs_rel': ez / sz, 'y_maxabs_rel': ey / sy}
    return syms, splits, errs, all(v <= TOL_MAXABS for v in errs.values())


def run_dgrad(n, h, w, cin, cout, stride, r):
    wt = (r.standard_normal((3, 3, cin, cout), dtype=np.float32) * 0.05).astype(np.float32)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    dz = r.standard_normal((n, ho, wo, cout), dtype=np.float32)
    addin = r.standard_normal((n, h, w, cin), dtype=np.float32)
    zprev = r.standard_normal((n, h, w, cin), dtype=np.float32)
    zprev[0, 0, 0, :4] = 0.0                                  # the z == 0 sub-gradient (slope alpha / 2)
    alp = (0.25 + 0.1 * r.standard_normal(cin, dtype=np.float32)).astype(np.float32)
    raw = torch.empty(n, h, w, cin, device='cuda'); dzp = torch.empty_like(raw)
    da = torch.empty(cin, device='cuda'); db = torch.empty(cin, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_dgrad_ws_bytes', n, h, w, cin, cout, stride))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv3x3_dgrad', torch.from_numpy(dz).cuda(), torch.from_numpy(wt).cuda(), torch.from_numpy(addin).cuda(),
         torch.from_numpy(zprev).cuda(), torch.from_numpy(alp).cuda(), raw, dzp, da, db, n, h, w, cin, cout, stride, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    rawg, dzpg = raw.cpu().numpy(), dzp.cpu().numpy()
    w64, al64 = wt.astype(np.float64), alp.astype(np.float64)
    er = ed = sr = sd = 0.0
    da_ref = np.zeros(cin); db_ref = np.zeros(cin)
    xshape = np.zeros((1, h, w, cin))
    for i in range(0, n, BLOCK):
        m = min(BLOCK, n - i)
        dx, _ = ops.conv2d_bwd(np.broadcast_to(xshape, (m, h, w, cin)), w64, dz[i:i + m].astype(np.float64), stride, need_dw=False)
        g = dx + addin[i:i + m]
        dzr, dar = ops.prelu_bwd(zprev[i:i + m].astype(np.float64), al64, g)
        da_ref += dar; db_ref += dzr.sum(axis=(0, 1, 2))
        e, s = _maxabs(rawg[i:i + m], g); er = max(er, e); sr = max(sr, s)
        e, s = _maxabs(dzpg[i:i + m], dzr); ed = max(ed, e); sd = max(sd, s)

    def rl2(got, ref):
        return float(np.sqrt(((got - ref) ** 2).sum() / (ref ** 2).sum()))
    errs = {'raw_maxabs_rel': er / sr, 'dzprev_maxabs_rel': ed / sd,
            'dalpha_rell2': rl2(da.cpu().numpy().astype(np.float64), da_ref), 'dbias_rell2': rl2(db.cpu().numpy().astype(np.float64), db_ref)}
    ok = errs['raw_maxabs_rel'] <= TOL_MAXABS and errs['dzprev_maxabs_rel'] <= TOL_MAXABS and \
        errs['dalpha_rell2'] <= TOL_RELL2 and errs['dbias_rell2'] <= TOL_RELL2
    return syms, splits, errs, ok


def run_wgrad(n, h, w, cin, cout, stride, r):
    x = r.standard_normal((n, h, w, cin), dtype=np.float32)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    dz = r.standard_normal((n, ho, wo, cout), dtype=np.float32)
    dw = torch.empty(3, 3, cin, cout, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, stride))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv3x3_wgrad', torch.from_numpy(x).cuda(), torch.from_numpy(dz).cuda(), dw, n, h, w, cin, cout, stride, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    ref = np.zeros((3, 3, cin, cout))
    wz = np.zeros((3, 3, cin, cout))
    for i in range(0, n, BLOCK):
        _, d = ops.conv2d_bwd(x[i:i + BLOCK].astype(np.float64), wz, dz[i:i + BLOCK].astype(np.float64), stride, need_dx=False)
        ref += d
    e, s = _maxabs(dw.cpu().numpy().astype(np.float64), ref)
    errs = {'dw_maxabs_rel': e / s}
    return syms, splits, errs, e / s <= TOL_MAXABS


def _bf(a):
    """float32 array -> (bf16-exact float32 values, their int16 bit patterns on the GPU)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda().bfloat16()
    return t.float().cpu().numpy(), t.view(torch.int16)


def _stored_ok(got16, ref64, scale):
    """a bf16-STORED result against the float64 value it rounds: within one bf16 step of the reference (fp32 accumulation may tip a
    value across a rounding boundary) -- |got - ref| <= 2^-8 |ref| + 2e-5 scale; returns (worst excess ratio, ok)"""
    got = got16.view(torch.bfloat16).float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref64)
    lim = np.abs(ref64) * 2.0 ** -8 + TOL_MAXABS * scale
    return float((err / lim).max()), bool((err <= lim).all())


CANARY16 = 0x7fc1       # a bf16 NaN no kernel stores: an element still holding it was never written
GUARD = 8               # rows behind row M of a bf16 output that must keep the canary


def _out16(n, h, w, c):
    """a poisoned bf16 output: (the [n, h, w, c] view the library writes, the whole buffer with GUARD rows behind row M)"""
    M = n * h * w
    buf = torch.full((M + GUARD, c), CANARY16, dtype=torch.int16, device='cuda')
    return buf[:M].view(n, h, w, c), buf


def _nan32(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _ws_nan(nbytes):
    """a NaN workspace of exactly the granted bytes (what the library is told) with 4 KB of NaN behind them"""
    nbytes = int(nbytes)
    return torch.full(((nbytes + 3) // 4 + 1024,), float('nan'), device='cuda'), nbytes


def _canary_fails(outs, wsb=None, nbytes=0, finite=()):
    """outs: {name: whole buffer of _out16}; finite: {name: fp32 tensor that must be written everywhere} -> failure messages"""
    fails = []
    for name, buf in outs.items():
        M = buf.shape[0] - GUARD
        if not bool((buf[M:] == CANARY16).all()):
            fails.append('%s: a guard row behind row M = %d was written' % (name, M))
        left = int((buf[:M] == CANARY16).sum())
        if left:
            fails.append('%s: %d elements never written' % (name, left))
    if wsb is not None and not bool(torch.isnan(wsb[(nbytes + 3) // 4:]).all()):
        fails.append('workspace: written behind the granted %d bytes' % nbytes)
    for name, t in dict(finite).items():
        bad = int((~torch.isfinite(t)).sum())
        if bad:
            fails.append('%s: %d elements not finite (never written?)' % (name, bad))
    return fails


def run_s16fwd(n, h, w, cin, cout, stride, r, k=3):
    """fte_conv2d_fwd_s16 (bf16 x / shortcut in, bf16 z / y out): the persistent bf16 kernels at the sizes that select them"""
    assert stride == 1
    x, x16 = _bf(r.standard_normal((n, h, w, cin), dtype=np.float32))
    wt = (r.standard_normal((k, k, cin, cout), dtype=np.float32) * 0.05).astype(np.float32)
    wd = torch.from_numpy(wt).cuda()
    w16 = torch.empty(k, k, cin, cout, dtype=torch.int16, device='cuda'); w16t = torch.empty(k, k, cout, cin, dtype=torch.int16, device='cuda')
    call('fte_pack_weights_bf16', wd, w16, w16t, k, cin, cout, stream())
    wb = wd.bfloat16().float().cpu().numpy().astype(np.float64)
    b = r.standard_normal(cout, dtype=np.float32)
    al = (0.25 + 0.1 * r.standard_normal(cout, dtype=np.float32)).astype(np.float32)
    res, res16 = _bf(r.standard_normal((n, h, w, cout), dtype=np.float32))
    (z16, zbuf), (y16, ybuf) = _out16(n, h, w, cout), _out16(n, h, w, cout)
    wsb, nb = _ws_nan(query('fte_conv2d_fwd_ws_bytes', n, h, w, cin, cout, k, 1))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_fwd_s16', x16, w16t, torch.from_numpy(b).cuda(), torch.from_numpy(al).cuda(), res16, z16, y16, None, None,
         n, h, w, cin, cout, k, 1, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({'z16': zbuf, 'y16': ybuf}, wsb, nb)
    b64, al64 = b.astype(np.float64), al.astype(np.float64)
    wz = wy = 0.0
    ok = True
    for i in range(0, n, BLOCK):
        zr = ops.conv2d_fwd(x[i:i + BLOCK].astype(np.float64), wb, 1, b64)
        yr = ops.prelu_fwd(zr, al64) + res[i:i + BLOCK]
        e, o = _stored_ok(z16[i:i + BLOCK], zr, np.abs(zr).max()); wz = max(wz, e); ok = ok and o
        e, o = _stored_ok(y16[i:i + BLOCK], yr, np.abs(yr).max()); wy = max(wy, e); ok = ok and o
    return syms, splits, {'z_worst_over_limit': wz, 'y_worst_over_limit': wy, 'fails': fails}, ok and not fails


def run_s16dgrad(n, h, w, cin, cout, stride, r, k=3):
    """fte_conv2d_dgrad_s16 (bf16 dz / skip gradient / previous z in, bf16 raw / dz out, fp32 dalpha / dbias sums)"""
    assert stride == 1
    wt = (r.standard_normal((k, k, cin, cout), dtype=np.float32) * 0.05).astype(np.float32)
    wd = torch.from_numpy(wt).cuda()
    w16 = torch.empty(k, k, cin, cout, dtype=torch.int16, device='cuda'); w16t = torch.empty(k, k, cout, cin, dtype=torch.int16, device='cuda')
    call('fte_pack_weights_bf16', wd, w16, w16t, k, cin, cout, stream())
    wb = wd.bfloat16().float().cpu().numpy().astype(np.float64)
    dz, dz16 = _bf(r.standard_normal((n, h, w, cout), dtype=np.float32))
    addin, add16 = _bf(r.standard_normal((n, h, w, cin), dtype=np.float32))
    zp = r.standard_normal((n, h, w, cin), dtype=np.float32)
    zp[0, 0, 0, :4] = 0.0
    zprev, zp16 = _bf(zp)
    alp = (0.25 + 0.1 * r.standard_normal(cin, dtype=np.float32)).astype(np.float32)
    (raw16, rawbuf), (dzp16, dzpbuf) = _out16(n, h, w, cin), _out16(n, h, w, cin)
    da = _nan32(cin); db = _nan32(cin)
    wsb, nb = _ws_nan(query('fte_conv2d_dgrad_ws_bytes', n, h, w, cin, cout, k, 1))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_dgrad_s16', dz16, w16, add16, zp16, torch.from_numpy(alp).cuda(), raw16, dzp16, da, db, n, h, w, cin, cout, k, 1, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({'raw16': rawbuf, 'dz16': dzpbuf}, wsb, nb, {'dalpha': da, 'dbias': db})
    al64 = alp.astype(np.float64)
    da_ref = np.zeros(cin); db_ref = np.zeros(cin)
    xshape = np.zeros((1, h, w, cin))
    wr = wd_ = 0.0
    ok = True
    for i in range(0, n, BLOCK):
        m = min(BLOCK, n - i)
        dx, _ = ops.conv2d_bwd(np.broadcast_to(xshape, (m, h, w, cin)), wb, dz[i:i + m].astype(np.float64), 1, need_dw=False)
        g = dx + addin[i:i + m]
        dzr, dar = ops.prelu_bwd(zprev[i:i + m].astype(np.float64), al64, g)
        da_ref += dar; db_ref += dzr.sum(axis=(0, 1, 2))
        e, o = _stored_ok(raw16[i:i + m], g, np.abs(g).max()); wr = max(wr, e); ok = ok and o
        e, o = _stored_ok(dzp16[i:i + m], dzr, np.abs(dzr).max()); wd_ = max(wd_, e); ok = ok and o

    def rl2(got, ref):
        return float(np.sqrt(((got - ref) ** 2).sum() / (ref ** 2).sum()))
    errs = {'raw_worst_over_limit': wr, 'dz_worst_over_limit': wd_,
            'dalpha_rell2': rl2(da.cpu().numpy().astype(np.float64), da_ref), 'dbias_rell2': rl2(db.cpu().numpy().astype(np.float64), db_ref)}
    errs['fails'] = fails
    ok = ok and errs['dalpha_rell2'] <= TOL_RELL2 and errs['dbias_rell2'] <= TOL_RELL2 and not fails
    return syms, splits, errs, ok


def _bits(t16):
    return t16.cpu().numpy()


def _placement_errs(name, got16, want, errs, fails, bitwise=True):
    """got16: int16 [n, h, w, N] device tensor; want: float64 (bf16-exact) -- bit for bit, or by value (+0 == -0)"""
    if bitwise:
        cnt, first = win16_map.placement_check(_bits(got16), _bits(_dev16(want)))
    else:
        cnt, first = win16_map.placement_check(_host16(got16), want)
    errs[name + '_wrong_elements'] = cnt
    if cnt:
        fails.append('exact: %s differs from the tap-shifted input, first at (image, y, x, channel) = %s, %d in all' % (name, first, cnt))


def run_s16fwdx(n, h, w, cin, cout, stride, r):
    """EXACT placement, forward 3x3: position-coded x, one power of two per output channel at tap n mod 9 (tests/win16_map.py), zero bias,
    no shortcut, alpha = 1/4 -- every product and sum is exact, so the stored z must equal the tap-shifted input element times its power of
    two BIT FOR BIT, exact zero where the tap leaves the image; y = z or z / 4 by value"""
    assert stride == 1
    M = n * h * w
    x = coded_input(M, cin).reshape(n, h, w, cin)
    wd = torch.tensor(win16_map.hwio_filter('fwd', cin, cout), dtype=torch.float32, device='cuda')
    w16 = torch.empty(3, 3, cin, cout, dtype=torch.int16, device='cuda'); w16t = torch.empty(3, 3, cout, cin, dtype=torch.int16, device='cuda')
    call('fte_pack_weights_bf16', wd, w16, w16t, 3, cin, cout, stream())
    (z16, zbuf), (y16, ybuf) = _out16(n, h, w, cout), _out16(n, h, w, cout)
    wsb, nb = _ws_nan(query('fte_conv2d_fwd_ws_bytes', n, h, w, cin, cout, 3, 1))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_fwd_s16', _dev16(x), w16t, torch.zeros(cout, device='cuda'), torch.full((cout,), 0.25, device='cuda'), None, z16, y16, None, None,
         n, h, w, cin, cout, 3, 1, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({'z16': zbuf, 'y16': ybuf}, wsb, nb)
    want = win16_map.placement_expected('fwd', x, cout)
    errs = {}
    _placement_errs('z16', z16, want, errs, fails)
    _placement_errs('y16', y16, np.where(want > 0, want, 0.25 * want), errs, fails, bitwise=False)
    errs['fails'] = fails
    return syms, splits, errs, not fails


def run_s16dgradx(n, h, w, cin, cout, stride, r):
    """EXACT placement, data gradient 3x3 in its plain form (no skip gradient, no previous z, no alpha, no dalpha / dbias): position-coded
    dz, one power of two per INPUT channel -- the stored dx (and the raw copy) must equal the tap-shifted dz element times its power of two"""
    assert stride == 1
    M = n * h * w
    dz = coded_input(M, cout).reshape(n, h, w, cout)
    wd = torch.tensor(win16_map.hwio_filter('dgrad', cin, cout), dtype=torch.float32, device='cuda')
    w16 = torch.empty(3, 3, cin, cout, dtype=torch.int16, device='cuda'); w16t = torch.empty(3, 3, cout, cin, dtype=torch.int16, device='cuda')
    call('fte_pack_weights_bf16', wd, w16, w16t, 3, cin, cout, stream())
    (raw16, rawbuf), (dx16, dxbuf) = _out16(n, h, w, cin), _out16(n, h, w, cin)
    wsb, nb = _ws_nan(query('fte_conv2d_dgrad_ws_bytes', n, h, w, cin, cout, 3, 1))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_dgrad_s16', _dev16(dz), w16, None, None, None, raw16, dx16, None, None, n, h, w, cin, cout, 3, 1, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({'raw16': rawbuf, 'dx16': dxbuf}, wsb, nb)
    want = win16_map.placement_expected('dgrad', dz, cin)
    errs = {}
    _placement_errs('dx16', dx16, want, errs, fails)
    _placement_errs('raw16', raw16, want, errs, fails, bitwise=False)
    errs['fails'] = fails
    return syms, splits, errs, not fails


def run_s16wgrad1(n, h, w, cin, cout, stride, r):
    """fte_conv2d_wgrad16 of a 1x1 conv: the pointwise resident kernel (wgrad16p_kernel) against the float64 product of the same bf16 inputs"""
    x, x16 = _bf(r.standard_normal((n, h, w, cin), dtype=np.float32))
    dz, dz16 = _bf(r.standard_normal((n, h, w, cout), dtype=np.float32))
    dw = _nan32(1, 1, cin, cout)
    wsb, nb = _ws_nan(query('fte_conv2d_wgrad_ws_bytes', n, h, w, cin, cout, 1, stride))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_wgrad16', x16, dz16, dw, n, h, w, cin, cout, 1, stride, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({}, wsb, nb, {'dw': dw})
    ref = x.reshape(-1, cin).astype(np.float64).T @ dz.reshape(-1, cout).astype(np.float64)
    e, s = _maxabs(dw.cpu().numpy().astype(np.float64).reshape(cin, cout), ref)
    return syms, splits, {'dw_maxabs_rel': e / s, 'fails': fails}, e / s <= TOL_MAXABS and not fails


def run_s16wgrad(n, h, w, cin, cout, stride, r):
    """fte_conv2d_wgrad16 (bf16 x and dz in, fp32 dw out): the resident kernel of wgrad16.hip at the sizes that select it"""
    x, x16 = _bf(r.standard_normal((n, h, w, cin), dtype=np.float32))
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    dz, dz16 = _bf(r.standard_normal((n, ho, wo, cout), dtype=np.float32))
    dw = _nan32(3, 3, cin, cout)
    wsb, nb = _ws_nan(query('fte_conv2d_wgrad_ws_bytes', n, h, w, cin, cout, 3, stride))
    _lib.query('fte_prof_enable', 1)
    call('fte_conv2d_wgrad16', x16, dz16, dw, n, h, w, cin, cout, 3, stride, wsb, nb, stream())
    _lib.query('fte_prof_enable', 0)
    syms, splits = _records()
    fails = _canary_fails({}, wsb, nb, {'dw': dw})
    ref = np.zeros((3, 3, cin, cout))
    wz = np.zeros((3, 3, cin, cout))
    for i in range(0, n, BLOCK):
        _, d = ops.conv2d_bwd(x[i:i + BLOCK].astype(np.float64), wz, dz[i:i + BLOCK].astype(np.float64), stride, need_dx=False)
        ref += d
    e, s = _maxabs(dw.cpu().numpy().astype(np.float64), ref)
    return syms, splits, {'dw_maxabs_rel': e / s, 'fails': fails}, e / s <= TOL_MAXABS and not fails


# ---- fte_conv2d_bn_fwd under bf16 storage (tests/test_gpu_pw16_edges.py, tests/test_gpu_bn_fusion.py): conv, rounded z, the batch
# statistics of the stored values; folded: the BN in front of the conv in the loader, y side-stored.  Called in-process by those modules
# for the default environment and through main() ('bnfwd1' / 'bnfold1') where a hook of csrc/pw16.hip is set.
BN_EPS, BN_DECAY = 1e-3, 0.999
# (CANARY16 / GUARD above: z and y_side carry GUARD rows behind row M that must keep the canary)
# the limits of tests/test_gpu_bn_fusion.py on the statistics of the stored z (max-abs over the channels, relative to the largest reference)
BN_LIMITS = {'mean': 2e-6, 'rstd': 4e-6, 'scale': 4e-6, 'shift': 1e-5, 'moving_mean': 2e-6, 'moving_var': 2e-6}


def _bf64(a):
    return ops.bf16_round(np.asarray(a, np.float64))


def _dev16(a):
    """float64 array of bf16-exact values -> int16 device tensor holding the bf16 bits"""
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).to(torch.bfloat16).view(torch.int16).cuda()


def _host16(t):
    return t.view(torch.bfloat16).float().cpu().numpy().astype(np.float64)


def selection_filter(K, N, a=5, b=3, unit=False):
    """HWIO [1, 1, K, N] filter with ONE non-zero per output channel: W[n][k] = 2^e at k = (a n + b) mod K (a odd), e = n mod 5 - 2 (0 with
    `unit`).  Returns (filter, the selected input channel per n, the power of two per n)."""
    n = np.arange(N)
    k, g = (a * n + b) % K, 2.0 ** (((n % 5) - 2) * (0 if unit else 1))
    wt = np.zeros((1, 1, K, N))
    wt[0, 0, k, n] = g
    return wt, k, g


def coded_input(M, K):
    """x[m][k] = (((7 m + 13 k) mod 251) - 125) / 64: every value bf16-exact (|numerator| < 2^7), no two neighbours alike"""
    m, k = np.arange(M, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return (((7 * m + 13 * k) % 251) - 125) / 64.0


def stats64(zs, gamma, beta, mm, mv):
    """float64 statistics of the stored rows [M, C] and what bn_finalize derives from them"""
    mean, var = zs.mean(axis=0), zs.var(axis=0)
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    scale = gamma * rstd
    mmr, mvr = ops.bn_moving_update(mm, mv, mean, var, zs.shape[0])
    return {'mean': mean, 'rstd': rstd, 'scale': scale, 'shift': beta - mean * scale, 'moving_mean': mmr, 'moving_var': mvr}


def bn_fwd_call(x16, wt, dims, gamma, beta, mm, mv, fold=None, nrb=None):
    """One fte_conv2d_bn_fwd call (s16 = 1) on x16 [M, cin] bf16 bits with every output poisoned first: z and y_side hold CANARY16 and carry
    GUARD rows behind row M, the statistics and the WHOLE workspace hold NaN.  fold = (in_scale, in_shift) device tensors or None.  nrb: the
    partial rows the streaming kernel must write (rows [nrb, granted) must stay NaN), or None for the tile kernels.
    -> dict(z16 [M, cout], y16 [M, cin] | None, stats {name: float64 [cout]}, symbols, fails [messages])"""
    n, h, w, cin, cout, ks, stride = dims
    M = n * h * w
    assert stride == 1
    wd = torch.tensor(np.ascontiguousarray(wt), dtype=torch.float32, device='cuda')
    w16 = torch.empty(ks * ks * cin * cout, dtype=torch.int16, device='cuda'); w16t = torch.empty_like(w16)
    call('fte_pack_weights_bf16', wd, w16, w16t, ks, cin, cout, stream())
    z16 = torch.full((M + GUARD, cout), CANARY16, dtype=torch.int16, device='cuda')
    ys = torch.full((M + GUARD, cin), CANARY16, dtype=torch.int16, device='cuda') if fold else None
    st = [torch.full((cout,), float('nan'), device='cuda') for _ in range(4)]
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda')
    mmd, mvd = f32(mm), f32(mv)
    nbytes = query('fte_conv2d_bn_fwd_ws_bytes', n, h, w, cin, cout, ks, stride)
    wsb = torch.full((nbytes // 4 + 1024,), float('nan'), device='cuda')       # 4 KB behind the grant: must stay NaN too
    prev = _lib.precision_mode()
    _lib.set_mfma_dtype('bf16s')
    try:
        _lib.query('fte_prof_enable', 1)
        call('fte_conv2d_bn_fwd', x16, w16t, z16, f32(gamma), f32(beta), st[0], st[1], st[2], st[3], mmd, mvd, BN_EPS, BN_DECAY,
             fold[0] if fold else None, fold[1] if fold else None, ys, n, h, w, cin, cout, ks, stride, 1, wsb, nbytes, stream())
        torch.cuda.synchronize()
        _lib.query('fte_prof_enable', 0)
    finally:
        _lib.set_mfma_dtype(prev)
    syms = [r[5] for r in _lib.prof_records(shapes=True)]
    fails = []
    if not bool((z16[M:] == CANARY16).all()):
        fails.append('z: a guard row behind row M was written')
    if bool((z16[:M] == CANARY16).any()):
        fails.append('z: %d elements never written' % int((z16[:M] == CANARY16).sum()))
    if fold:
        if not bool((ys[M:] == CANARY16).all()):
            fails.append('y_side: a guard row behind row M was written')
        if bool((ys[:M] == CANARY16).any()):
            fails.append('y_side: %d elements never written' % int((ys[:M] == CANARY16).sum()))
    if not bool(torch.isnan(wsb[nbytes // 4:]).all()):
        fails.append('workspace: written behind the granted bytes')
    if nrb is not None:
        used = nrb * 3 * cout
        if not bool(torch.isfinite(wsb[:used]).all()):
            fails.append('workspace: %d words of the %d partial rows never written' % (int((~torch.isfinite(wsb[:used])).sum()), nrb))
        if not bool(torch.isnan(wsb[used:]).all()):
            fails.append('workspace: a partial row >= nrb = %d was written' % nrb)
    names = ['mean', 'rstd', 'scale', 'shift']
    stats = {k: st[i].cpu().numpy().astype(np.float64) for i, k in enumerate(names)}
    stats['moving_mean'] = mmd.cpu().numpy().astype(np.float64); stats['moving_var'] = mvd.cpu().numpy().astype(np.float64)
    for k, v in stats.items():
        if not np.isfinite(v).all():
            fails.append('%s: %d channels not finite' % (k, int((~np.isfinite(v)).sum())))
    return dict(z16=z16[:M], y16=ys[:M] if fold else None, stats=stats, symbols=syms, fails=fails)


def _fold_coef(r, cin):
    """scale / shift of the BN in front: in_shift > 0 on EVERY channel, so that a row the loader fetched as zeros (beyond row M) becomes a
    non-zero operand -- the statistics must still count M rows only"""
    isc = (1 + 0.2 * r.standard_normal(cin)).astype(np.float32)
    ish = (0.1 + 0.3 * np.abs(r.standard_normal(cin))).astype(np.float32)
    return isc, ish


def _bn_apply_ref(x16, isc, ish, M, cin):
    y = torch.empty((M, cin), dtype=torch.int16, device='cuda')
    call('fte_bn_apply', x16, torch.tensor(isc, device='cuda'), torch.tensor(ish, device='cuda'), None, y, M, cin, 1, 3, stream())
    return y


def _where2(mask, cout):
    i = int(np.flatnonzero(mask.reshape(-1))[0])
    return 'first at (row, channel) = (%d, %d), %d in all' % (i // cout, i % cout, int(mask.sum()))


def bn_exact(dims, fold, nrb=None, seed=31):
    """EXACT placement (1x1 only): selection filter x position-coded input -- every product and sum exact, so z must equal the expected
    tensor bit for bit; folded: y_side bit-equal to fte_bn_apply, z bit-equal to the selection of that y.  -> (symbols, errors, fails)"""
    n, h, w, cin, cout, ks, stride = dims
    M = n * h * w
    assert ks == 1
    r = np.random.default_rng(seed)
    wt, sel, g = selection_filter(cin, cout)
    x16 = _dev16(coded_input(M, cin))
    gamma = 1 + 0.2 * r.standard_normal(cout); beta = 0.3 * r.standard_normal(cout)
    mm = r.standard_normal(cout) * 0.1; mv = 1 + 0.1 * r.random(cout)
    coef = None
    if fold:
        isc, ish = _fold_coef(r, cin)
        coef = (torch.tensor(isc, device='cuda'), torch.tensor(ish, device='cuda'))
    o = bn_fwd_call(x16, wt, dims, gamma, beta, mm, mv, coef, nrb)
    fails = list(o['fails'])
    src16 = x16
    if fold:
        src16 = _bn_apply_ref(x16, isc, ish, M, cin)
        if not torch.equal(o['y16'], src16):
            fails.append('exact: y_side differs from fte_bn_apply, ' + _where2((o['y16'] != src16).cpu().numpy(), cin))
    want = _dev16(_host16(src16)[:, sel] * g)          # one input element times a power of two: exact, bf16-exact
    bad = (o['z16'] != want).cpu().numpy()
    if bad.any():
        fails.append('exact: z differs from the selected input, ' + _where2(bad, cout))
    return o['symbols'], {'exact_wrong_elements': int(bad.sum())}, fails


def bn_random(dims, fold, nrb=None, seed=32):
    """the generator of tests/test_gpu_bn_fusion.py: z element by element against the float64 product (_stored_ok), the statistics against
    float64 statistics of the STORED z with that module's limits.  -> (symbols, errors, fails)"""
    n, h, w, cin, cout, ks, stride = dims
    M = n * h * w
    r = np.random.default_rng(seed)
    wt = _bf64(r.standard_normal((ks, ks, cin, cout)) * 0.05)
    gamma = 1 + 0.2 * r.standard_normal(cout); beta = 0.3 * r.standard_normal(cout)
    mm = r.standard_normal(cout) * 0.1; mv = 1 + 0.1 * r.random(cout)
    coef = None
    if fold:
        x = _bf64(r.standard_normal((M, cin)) * 1.5 + 0.3)
        isc, ish = _fold_coef(r, cin)
        coef = (torch.tensor(isc, device='cuda'), torch.tensor(ish, device='cuda'))
    else:
        x = _bf64(r.standard_normal((M, cin)) + 0.7)
    x16 = _dev16(x)
    o = bn_fwd_call(x16, wt, dims, gamma, beta, mm, mv, coef, nrb)
    fails = list(o['fails'])
    src = x
    if fold:
        y_ref = _bn_apply_ref(x16, isc, ish, M, cin)
        if not torch.equal(o['y16'], y_ref):
            fails.append('random: y_side differs from fte_bn_apply, ' + _where2((o['y16'] != y_ref).cpu().numpy(), cin))
        src = _host16(y_ref)
        y64 = _bf64(np.maximum(x * isc.astype(np.float64) + ish.astype(np.float64), 0))
        e = float(np.sqrt(((src - y64) ** 2).sum() / (y64 ** 2).sum()))
        if e > 2e-3:
            fails.append('random: y vs the oracle rel-L2 %.3e > 2e-3' % e)
    if ks == 1:
        z_ref = src @ wt.reshape(cin, cout)
    else:
        z_ref = ops.conv2d_fwd(src.reshape(n, h, w, cin), wt, 1).reshape(M, cout)
    worst, ok = _stored_ok(o['z16'], z_ref, np.abs(z_ref).max())
    errs = {'z_worst_over_limit': worst}
    if not ok:
        fails.append('random: z beyond 2^-8 |ref| + 2e-5 max|ref| (worst / limit = %.3f)' % worst)
    ref = stats64(_host16(o['z16']), gamma, beta, mm, mv)
    for k, lim in BN_LIMITS.items():
        e = float(np.abs(o['stats'][k] - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30))
        errs[k + '_maxabs_rel'] = e
        if not e <= lim:
            fails.append('random: %s of the stored z off by %.3e > %.1e (relative to the largest)' % (k, e, lim))
    return o['symbols'], errs, fails


def _run_bn1(n, h, w, cin, cout, stride, r, fold):
    """worker form of the two checks for a hooked 1x1 case: the partial-row count from tests/pw16_map.py under THIS process's hooks"""
    import pw16_cases
    import pw16_map
    dims = (n, h, w, cin, cout, 1, stride)
    p = pw16_map.plan(n * h * w, cin, cout, **pw16_cases.hooks(os.environ))
    nrb = p['nrb'] if p else None
    s1, e1, f1 = bn_exact(dims, fold, nrb)
    s2, e2, f2 = bn_random(dims, fold, nrb)
    errs = dict(e1, **e2)
    errs['fails'] = f1 + f2
    errs['symbols_per_call'] = [s1, s2]
    return sorted(set(s1 + s2)), [], errs, not (f1 + f2)


def main():
    cases = json.loads(sys.argv[1])
    out, ok_all = [], True
    for ci, c in enumerate(cases):
        op, dims = c[0], [int(v) for v in c[1:]]
        r = np.random.default_rng(100 + ci)
        syms, splits, errs, ok = {'fwd': run_fwd, 'dgrad': run_dgrad, 'wgrad': run_wgrad, 's16fwd': run_s16fwd, 's16dgrad': run_s16dgrad,
                                  's16fwd1': lambda *a: run_s16fwd(*a, k=1), 's16dgrad1': lambda *a: run_s16dgrad(*a, k=1),
                                  's16wgrad': run_s16wgrad, 's16wgrad1': run_s16wgrad1, 's16fwdx': run_s16fwdx, 's16dgradx': run_s16dgradx,
                                  'bnfwd1': lambda *a: _run_bn1(*a, fold=False), 'bnfold1': lambda *a: _run_bn1(*a, fold=True)}[op](*dims, r)
        out.append({'case': c, 'symbols': syms, 'splits': splits, 'errors': errs, 'ok': bool(ok)})
        ok_all = ok_all and ok
        torch.cuda.empty_cache()
    print(json.dumps({'cases': out, 'ok': bool(ok_all)}))
    sys.exit(0 if ok_all else 1)


if __name__ == '__main__':
    main()
