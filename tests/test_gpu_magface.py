"""-m gpu: the MagFace head (include/fte.h fte_magface_softmax_fwd_bwd) -- the kernel against the float64 restatement
(tests/magface_ref.py) at the shapes its code branches on, the public loss function, SphereNet-MagFace against the oracle backbone
composed with the restatement (every gradient, training steps), the graph nets' head, determinism, checkpoints, the command line,
two data-parallel ranks and verify.py --weight_by_norm.  Shapes, tolerances and the way G and rowcoef are judged are
tests/test_gpu_adaface.py's for the same quantities; reg_rows: 1e-6 relative (one division and one fma on an fp32 norm).

THE JUMPS.  The target logit jumps where c_iy crosses -cos mu_i, and the norm gradient where xn_i crosses l_a or u_a.  The kernel
tests BUILD their inputs clear of both and assert, in float64 on the device's s / xn / wn before any comparison, that every row has
|c_iy + cos mu_i| > 1e-4, |xn_i - l_a| > 1e-3 l_a and |xn_i - u_a| > 1e-3 u_a: conditions on the inputs, nothing is excluded.

rowcoef is a sum of terms of both signs -- sum_j G_ij s_ij over the row and, inside [l_a, u_a], the two shares of dL/da -- and is
judged against 2e-5 of the sum of their magnitudes, as test_gpu_adaface.py judges the first sum."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import magface_ref as gr
import template_ref as tr
from oracle import spherenet as osn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2, kink_of, ws, call, stream
    from tf_face_toolbox_amd import net_select, Singular, _lib, saver
    from tf_face_toolbox_amd.loss import magface_loss

D = 512
NAME = 'SphereNet-MagFace'
PRESET = (64.0, 10.0, 110.0, 0.45, 0.8, 35.0)
OTHER = (30.0, 10.0, 110.0, 0.35, 1.2, 5.0)                        # same norm range (the inputs' zones), another S / margin range / lambda_g
HYPERS = (PRESET, OTHER)


# ------------------------------------------------------------------------------------------------ inputs
def _zone_norms(rng, zone, l_a=10.0, u_a=110.0):
    """norms below l_a (zone 0), inside (1) and above u_a (2), at least 5 % away from the bounds"""
    n = len(zone)
    return np.where(zone == 0, rng.uniform(0.05 * l_a, 0.95 * l_a, n),
                    np.where(zone == 1, rng.uniform(1.05 * l_a, 0.95 * u_a, n), rng.uniform(1.05 * u_a, 2 * u_a, n)))


def _mu(norms, hyper):
    return gr.margins(norms, *hyper[1:5])[1]


def _features(rng, W, y, n, zone, a=None):
    """rows whose target cosine spreads over [-0.97, 0.97] (tests/test_gpu_adaface.py) with norms in the zones given; a cosine
    within 2e-3 of -cos mu_i under either parameter set is moved 5e-3 away from it, so no row sits at the fallback's jump"""
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    if a is None:
        a = rng.uniform(-0.97, 0.97, n)
        a[:min(n, 2)] = [-0.95, 0.9][:min(n, 2)]
        if n > 4:
            a[4] = -0.93                                            # zone 1 (inside the norm range) on the fallback side
    norms = _zone_norms(rng, zone)
    for _ in range(4):
        for hyper in HYPERS:
            near = np.abs(a + np.cos(_mu(norms, hyper))) < 2e-3
            a = np.where(near, a + 5e-3, a)
    e = rng.standard_normal((D, n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    x = (a * wy + np.sqrt(1 - a * a) * e) * norms
    return x.T.astype(np.float32)


def _products(x, W, c):
    """(s [n, ldp], xn [n], wn [ldp]) on the GPU: s = x @ W by the library's product, the norms by its kernels"""
    n, ldp = x.shape[0], W.shape[1]
    xd, Wd = dev(x), dev(W)
    s = torch.empty(n, ldp, dtype=torch.float32, device='cuda')
    xn = torch.empty(n, dtype=torch.float32, device='cuda')
    wn = torch.empty(ldp, dtype=torch.float32, device='cuda')
    w_, wb = ws(_lib.query('fte_gemm_ws_bytes', n, ldp, D))
    call('fte_gemm_nn', xd, Wd, None, s, n, ldp, D, w_, wb, stream())
    call('fte_row_norms', xd, xn, n, D, D, stream())
    call('fte_col_norms', Wd, wn, D, c, ldp, stream())
    return s, xn, wn


_RAW = {}
# one row cannot be below, inside and above the norm range at once: the n = 1 shapes run four single rows, (zone, target cosine).
# A batch of ONE row has only its own gradient as the scale G is judged against (tests/test_gpu_adaface.py _raw), so its target
# cosine must not saturate the softmax: at c_iy = 0.9 and S = 64 the target logit leads the others by 25, 1 - p_iy = 3e-12 is below
# what fp32 holds beside 1 and the whole row of G is rounding.  0.5 keeps p_iy between 1e-4 and 0.9 at every c and S used here.
SINGLE = ((0, 0.5), (1, -0.95), (1, 0.5), (2, -0.95))


def _raw(n, c, seed, single=None):
    """made once per (n, c, seed, single) and shared: the tests only read it.  Row i is in zone i % 3 (n = 1: the zone of `single`)."""
    key = (n, c, seed, single)
    if key not in _RAW:
        rng = np.random.default_rng(seed)
        ldp = (c + 127) // 128 * 128
        W = np.zeros((D, ldp), np.float32)
        W[:, :c] = rng.standard_normal((D, c), dtype=np.float32)
        y = rng.integers(0, c, n)
        y[0] = 0
        y[-1] = c - 1
        zone = np.arange(n) % 3 if single is None else np.full(n, single[0])
        a = None if single is None else np.full(n, single[1])
        s, xn, wn = _products(_features(rng, W, y, n, zone, a), W, c)
        if len(_RAW) > 3:
            _RAW.clear()                                            # a few cases at a time stay on the device
        _RAW[key] = (s, xn, wn, dev(y, torch.int32))
    return _RAW[key]


def _cases(n, c, seed):
    return [_raw(n, c, seed)] if n > 1 else [_raw(n, c, seed, single) for single in SINGLE]


# ------------------------------------------------------------------------------------------------ fte_magface_softmax_fwd_bwd
def _kernel(s, xn, wn, labels, c, hyper, gs, with_f=True):
    n, ld = s.shape
    f = torch.full((n, ld), 7.0, device='cuda') if with_f else None
    G = torch.full((n, ld), 7.0, device='cuda')
    rows, reg, rc = (torch.full((n,), 7.0, device='cuda') for _ in range(3))
    call('fte_magface_softmax_fwd_bwd', s, xn, wn, labels, *hyper, f, rows, reg, G, rc, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, reg, G, rc


def _check_inputs(sh, xnh, wnh, y, c, hyper, what):
    """the conditions on the inputs, in float64, before any comparison"""
    gap_c, gap_l, gap_u = gr.gaps(sh, xnh, wnh, y, *hyper[1:5], c=c)
    print(what, 'min |c_y + cos mu| %.2e, min |xn - l_a| / l_a %.2e, min |xn - u_a| / u_a %.2e' % (gap_c, gap_l, gap_u))
    assert gap_c > 1e-4 and gap_l > 1e-3 and gap_u > 1e-3, (what, gap_c, gap_l, gap_u)


def _check_head(got, s, xn, wn, labels, c, hyper, gs, what):
    """the kernel's (f, loss_rows, reg_rows, G, rowcoef) against the restatement on the same s / xn / wn"""
    f, rows, reg, G, rc = got
    sh, xnh, wnh = host(s), host(xn), host(wn)
    y = host(labels).astype(int)
    ld = sh.shape[1]
    _check_inputs(sh, xnh, wnh, y, c, hyper, what)
    fr, lr, regr, Gr, rcr, arc_part, norm_part, mag = gr.kernel_ref(sh, xnh, wnh, y, *hyper, gs, c=c, parts=True)
    ok = np.isfinite(lr)
    if f is not None:
        print(what, 'f err', np.abs(host(f)[ok] - fr[ok]).max(), 'of', np.abs(fr[ok]).max())
        check_maxabs(host(f)[ok], fr[ok], what=what + ' f')
        assert (host(f)[:, c:] == 0).all(), what
    print(what, 'G err', np.abs(host(G)[ok] - Gr[ok]).max(), 'of', np.abs(Gr[ok]).max(), 'loss err', np.abs(host(rows)[ok] - lr[ok]).max())
    check_maxabs(host(G)[ok], Gr[ok], what=what + ' G')
    check_rell2(host(G)[ok], Gr[ok], what=what + ' G')
    assert (host(G)[:, c:ld] == 0).all(), what + ': padding columns'
    lg = host(rows)[ok]
    assert np.all(np.abs(lg - lr[ok]) <= 2e-5 * np.maximum(1.0, np.abs(lr[ok]))), (what, np.abs(lg - lr[ok]).max())
    rg = host(reg)[ok]
    print(what, 'reg_rows rel err', (np.abs(rg - regr[ok]) / regr[ok]).max())
    assert np.all(np.abs(rg - regr[ok]) <= 1e-6 * regr[ok]), (what, 'reg_rows', (np.abs(rg - regr[ok]) / regr[ok]).max())
    err = np.abs(host(rc)[ok] - rcr[ok]) / mag[ok]
    print(what, 'rowcoef err / sum of term magnitudes', err.max())
    assert np.all(err <= 2e-5), (what, 'rowcoef', err)
    return ok, arc_part, norm_part


def _coverage(xnh, sh, wnh, y, c, hyper):
    """rows below l_a, inside, above u_a; target cosines on both sides of the fallback"""
    _, mu, _, inside, _ = gr.margins(xnh, *hyper[1:5])
    cy = sh[np.arange(len(y)), y] / (xnh.astype(np.float64) * wnh[y])
    return (xnh < hyper[1]).any(), inside.any(), (xnh > hyper[2]).any(), (cy > -np.cos(mu)).any(), (cy < -np.cos(mu)).any()


@pytest.mark.parametrize('n,c', [(1, 10), (7, 1000), (64, 1001), (512, 1000), (64, 4100), (512, 10575), (1, 10575), (64, 85742)])
def test_kernel_against_the_restatement(n, c):
    """ld % 4 == 0 throughout (the vector path); c = 1001 / 10575 / 85742 not a multiple of 4 under an aligned ld; c < 1024 one trip
    of the unrolled loop, c > 4096 several; n = 1 and n = 512"""
    seen = np.zeros(5, bool)
    for s, xn, wn, labels in _cases(n, c, seed=n * 7 + c):
        assert s.shape[1] % 4 == 0
        for hyper in HYPERS:
            ok, arc_part, norm_part = _check_head(_kernel(s, xn, wn, labels, c, hyper, 1.0 / n), s, xn, wn, labels, c, hyper, 1.0 / n,
                                                  'n=%d c=%d S=%g' % (n, c, hyper[0]))
            # OUTSIDE the norm range a row gets no norm gradient: rowcoef is the ArcFace-form value (checked above against
            # arc_part + norm_part with norm_part = 0 there, by the restatement's construction; asserted here)
            xnh = host(xn)
            out = (xnh < hyper[1]) | (xnh > hyper[2])
            assert (norm_part[out] == 0).all() and (np.abs(norm_part[~out]) > 0).all()
        seen |= np.array(_coverage(host(xn), host(s), host(wn), host(labels).astype(int), c, PRESET))
    assert seen.all(), seen                                         # every case: all three zones, both sides of the fallback


@pytest.mark.parametrize('n', [1, 7, 512])
def test_unaligned_ld_takes_the_scalar_path(n):
    c = 1000
    ld = c + 3
    seen = np.zeros(5, bool)
    for s, xn, wn, labels in _cases(n, c, seed=100 + n):
        su = torch.zeros(n, ld, device='cuda')
        su[:, :c] = s[:, :c]
        for hyper in HYPERS:
            _check_head(_kernel(su, xn, wn, labels, c, hyper, 1.0 / n), su, xn, wn, labels, c, hyper, 1.0 / n, 'ld=%d n=%d S=%g' % (ld, n, hyper[0]))
        seen |= np.array(_coverage(host(xn), host(su), host(wn), host(labels).astype(int), c, PRESET))
    assert seen.all(), seen


def _arcface(s, xn, wn, labels, c, S, m, gs):
    n, ld = s.shape
    f, G = torch.empty_like(s), torch.empty_like(s)
    rows, rc = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, S, m, 0.0, f, rows, G, rc, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, G, rc


def _same_as_arcface(got, ref, s, xn, sel, what):
    f, rows, _, G, rc = got
    check_maxabs(host(f)[sel], host(ref[0])[sel], what=what + ' f')
    check_maxabs(host(G)[sel], host(ref[2])[sel], what=what + ' G')
    lg, lr = host(rows)[sel], host(ref[1])[sel]
    assert np.all(np.abs(lg - lr) <= 2e-5 * np.maximum(1.0, np.abs(lr))), what
    mag = (np.abs(host(ref[2]) * host(s)).sum(1) / host(xn) ** 2)[sel]      # rowcoef: against the sum of its terms' magnitudes
    assert np.all(np.abs(host(rc)[sel] - host(ref[3])[sel]) <= 2e-5 * mag), what


def test_rows_outside_the_norm_range_get_the_arcface_rowcoef():
    """below l_a the row is ArcFace's at m = l_m, above u_a at m = u_m -- f, loss, G and rowcoef, no norm term -- against
    fte_margin_softmax_fwd_bwd on the same data"""
    n, c = 64, 4100
    s, xn, wn, labels = _raw(n, c, seed=n * 7 + c)
    got = _kernel(s, xn, wn, labels, c, PRESET, 1.0 / n)
    xnh = host(xn)
    for sel, m in ((xnh < PRESET[1], PRESET[3]), (xnh > PRESET[2], PRESET[4])):
        assert sel.sum() >= n // 4
        _same_as_arcface(got, _arcface(s, xn, wn, labels, c, 64.0, m, 1.0 / n), s, xn, sel, 'm=%g' % m)


def test_constant_margin_reproduces_the_arcface_kernel():
    """l_m = u_m = 0.5, lambda_g = 0: fte_margin_softmax_fwd_bwd(m = 0.5) on every row, whatever its norm"""
    n, c = 64, 10575
    s, xn, wn, labels = _raw(n, c, seed=15)
    got = _kernel(s, xn, wn, labels, c, (64.0, 10.0, 110.0, 0.5, 0.5, 0.0), 1.0 / n)
    _same_as_arcface(got, _arcface(s, xn, wn, labels, c, 64.0, 0.5, 1.0 / n), s, xn, np.ones(n, bool), 'constant margin')
    a = np.clip(host(xn).astype(np.float64), 10.0, 110.0)
    assert np.all(np.abs(host(got[2]) - (a / 110.0 ** 2 + 1 / a)) <= 1e-6 * (a / 110.0 ** 2 + 1 / a))      # reg_rows is still g


def test_f_null_gives_the_same_G_and_repeats_bit_for_bit():
    n, c = 64, 10575
    s, xn, wn, labels = _raw(n, c, seed=15)
    r1 = _kernel(s, xn, wn, labels, c, PRESET, 1.0 / n, with_f=True)
    r2 = _kernel(s, xn, wn, labels, c, PRESET, 1.0 / n, with_f=False)
    r3 = _kernel(s, xn, wn, labels, c, PRESET, 1.0 / n, with_f=False)
    for i in (1, 2, 3, 4):
        assert torch.equal(r1[i], r2[i]) and torch.equal(r2[i], r3[i])
    ld = c + 3                                                      # the scalar path too
    su = torch.zeros(n, ld, device='cuda')
    su[:, :c] = s[:, :c]
    q1 = _kernel(su, xn, wn, labels, c, PRESET, 1.0 / n, with_f=True)
    q2 = _kernel(su, xn, wn, labels, c, PRESET, 1.0 / n, with_f=False)
    for i in (1, 2, 3, 4):
        assert torch.equal(q1[i], q2[i])


def test_bad_labels_give_nan_rows_and_leave_their_neighbours_alone():
    n, c = 7, 1000
    s, xn, wn, labels = _raw(n, c, seed=100 + n)
    want = _kernel(s, xn, wn, labels, c, PRESET, 1.0 / n)
    bad = labels.clone()
    bad[3] = c
    bad[5] = -1
    f, rows, reg, G, rc = _kernel(s, xn, wn, bad, c, PRESET, 1.0 / n)
    for i in (3, 5):
        assert np.isnan(float(rows[i])) and np.isnan(float(rc[i])) and np.isnan(float(reg[i])), i
        assert torch.isnan(G[i, :c]).all() and torch.isnan(f[i, :c]).all(), i
    assert (G[:, c:] == 0).all() and (f[:, c:] == 0).all()                  # padding: 0, on the NaN rows too
    good = [0, 1, 2, 4, 6]
    for u, v in zip((f, rows, reg, G, rc), want):
        assert torch.equal(u[good], v[good])                                # bit for bit


def test_invalid_arguments_write_nothing():
    s, xn, wn, labels = _raw(7, 1000, seed=107)
    n, c, ld = 7, 1000, s.shape[1]
    G = torch.full_like(s, 7.0)
    rows, reg, rc = (torch.full((n,), 7.0, device='cuda') for _ in range(3))
    nan = float('nan')
    ok = dict(S=64.0, l_a=10.0, u_a=110.0, l_m=0.45, u_m=0.8, lg=35.0, n=n, c=c, ld=ld)
    for bad in (dict(S=0.0), dict(S=-1.0), dict(S=nan), dict(l_a=0.0), dict(l_a=-1.0), dict(l_a=nan), dict(u_a=10.0), dict(u_a=5.0),
                dict(u_a=nan), dict(l_m=-0.1), dict(l_m=nan), dict(u_m=0.4), dict(u_m=1.5708), dict(u_m=nan), dict(lg=-1.0), dict(lg=nan),
                dict(n=0), dict(n=-1), dict(c=0), dict(ld=999)):
        k = dict(ok, **bad)
        with pytest.raises(_lib.FteError):
            call('fte_magface_softmax_fwd_bwd', s, xn, wn, labels, k['S'], k['l_a'], k['u_a'], k['l_m'], k['u_m'], k['lg'], None, rows, reg, G,
                 rc, k['n'], k['c'], k['ld'], 0.25, stream())
    for miss in range(8):
        ptrs = [s, xn, wn, labels, rows, reg, G, rc]
        ptrs[miss] = None
        with pytest.raises(_lib.FteError):
            call('fte_magface_softmax_fwd_bwd', ptrs[0], ptrs[1], ptrs[2], ptrs[3], *PRESET, None, ptrs[4], ptrs[5], ptrs[6], ptrs[7],
                 n, c, ld, 0.25, stream())
    torch.cuda.synchronize()
    assert (G == 7.0).all() and (rows == 7.0).all() and (reg == 7.0).all() and (rc == 7.0).all()      # nothing written
    call('fte_magface_softmax_fwd_bwd', s, xn, wn, labels, 64.0, 10.0, 110.0, 0.0, 0.0, 0.0, None, rows, reg, G, rc, n, c, ld, 0.25,
         stream())                                                  # l_m = u_m = 0 and lambda_g = 0 are valid
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all() and torch.isfinite(rc).all()


# ------------------------------------------------------------------------------------------------ loss.magface_loss
@pytest.mark.parametrize('hyper', HYPERS)
def test_public_loss_function(hyper):
    rng = np.random.default_rng(17)
    n, c, ld = 64, 1000, 1024
    W = np.zeros((D, ld), np.float32)
    W[:, :c] = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    x = _features(rng, W, y, n, np.arange(n) % 3)
    x64, W64 = x.astype(np.float64), W[:, :c].astype(np.float64)
    gap_c, gap_l, gap_u = gr.head_gaps(x64, W64, y, *hyper[1:5])
    assert gap_c > 1e-4 and gap_l > 1e-3 and gap_u > 1e-3
    loss, dx, dW, mag = magface_loss(dev(x), dev(W), dev(y, torch.int32), *hyper, num_classes=c)
    torch.cuda.synchronize()
    ce_r, mag_r, _, dxr, dWr = gr.head_fwd_bwd(x64, W64, y, *hyper)
    # reg_rows to 1e-6 each, an fp32 sum of n = 64 positive terms (at most n * 2^-24 = 3.8e-6) and the rounding of lambda_g / n
    assert abs(float(mag) - mag_r) <= 5e-6 * mag_r, (float(mag), mag_r)
    assert abs(float(loss) - (ce_r + mag_r)) <= 2e-5 * max(1.0, abs(ce_r + mag_r)), (float(loss), ce_r + mag_r)
    check_rell2(host(dx), dxr, what='dfeatures')
    check_rell2(host(dW)[:, :c], dWr, what='dweights')
    assert (host(dW)[:, c:] == 0).all()
    # the norm term is a visible part of dfeatures: without it the comparison above fails
    s, xn, wn = x64 @ W64, np.linalg.norm(x64, axis=1), np.linalg.norm(W64, axis=0)
    norm_part = gr.kernel_ref(s, xn, wn, y, *hyper, 1.0 / n, parts=True)[6]
    missing = np.sqrt(((norm_part[:, None] * x64) ** 2).sum()) / np.sqrt((dxr ** 2).sum())
    print('share of the norm term in |dfeatures|: %.3e' % missing)
    assert missing > 1e-3
    with pytest.raises(ValueError, match='MagFace head needs'):
        magface_loss(dev(x), dev(W), dev(y, torch.int32), u_m=1.6)


# ------------------------------------------------------------------------------------------------ SphereNet-MagFace
def _setup(n, h, w, ch, ncls, seed=21, name=NAME):
    """images of different contrast (tests/test_gpu_adaface.py: equally scaled random images give norms within 1 % of each other);
    l_a and u_a are then put BETWEEN the oracle's embedding norms: the smallest below l_a, the largest above u_a (n >= 3; n = 2:
    one below, one inside)"""
    p = osn.perturb_params(osn.init_params(seed, ch, ncls, h, w), seed + 1)
    rng = np.random.default_rng(seed + 2)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    x = x * np.linspace(0.1, 4.0, n)[:, None, None, None]
    net = net_select(name, 'NCHW', 5e-4)
    net.build(h, w, ch, ncls, 'cuda')
    net.load_params(p)
    emb, _ = osn.backbone_fwd(p, x, 'NCHW')
    q = np.sort(np.sqrt((emb * emb).sum(1)))
    l_a = float(np.float32(0.5 * (q[0] + q[1])))
    u_a = float(np.float32(0.5 * (q[-2] + q[-1]) if n >= 3 else 2.0 * q[-1]))
    net.set_magface(l_a=l_a, u_a=u_a)
    return net, p, x, y


def _hyper(net):
    return (net.margin_scale,) + tuple(net.magface)


def _gaps_ok(g):
    return g[0] > 1e-4 and g[1] > 1e-3 and g[2] > 1e-3


@pytest.mark.parametrize('n,h,w,ch,ncls', [(4, 32, 32, 3, 10), (2, 112, 112, 1, 10575)])
def test_spherenet_forward_loss_and_every_gradient(n, h, w, ch, ncls):
    net, p, x, y = _setup(n, h, w, ch, ncls)
    xd, yd = dev(x), dev(y, torch.int32)
    net.tower_scale = 1.0
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    losses, names, others = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    hyper = _hyper(net)
    losses_ref, g_ref, ex = gr.loss_and_grads(p, x, y, hyper, 5e-4, 'NCHW', kink=kink_of(net))
    print('gaps', ex['gaps'], 'norms', ex['norms'], 'l_a, u_a', hyper[1:3])
    assert _gaps_ok(ex['gaps'])                                     # nothing near a jump: nothing excluded
    inside = (ex['norms'] >= hyper[1]) & (ex['norms'] <= hyper[2])
    assert inside.any() and (~inside).any()
    assert names == ['cross_entropy', 'magnitude_loss', 'reg_loss'] and not others
    check_maxabs(host(net.emb), ex['embedding'], what='embedding')
    check_maxabs(host(logits['logits']), ex['logits'], what='logits')
    for got, ref in zip(losses, losses_ref):
        assert abs(float(got) - ref) <= 1e-5 * max(1, abs(ref)), (float(got), ref, names)
    for k in p:
        data_grad = g_ref[k] - (5e-4 * p[k] if k.endswith('/weights') else 0)
        check_rell2(host(net.get_variable(k, net.grads)), data_grad, what='grad ' + k)


def test_three_training_steps_match_oracle():
    n, h, w, ch, ncls = 4, 32, 32, 3, 10
    net, p, x, y = _setup(n, h, w, ch, ncls, seed=31)
    inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
    step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
    torch.cuda.synchronize()
    assert names == ['cross_entropy', 'magnitude_loss', 'reg_loss']
    slots = osn.zero_slots(p)
    for i in range(3):
        step()
        p, slots, l_ref, gaps = gr.train_step(p, slots, x, y, 0.05, _hyper(net), kink=kink_of(net))
        assert _gaps_ok(gaps), (i, gaps)
        for got, ref in zip(losses, l_ref):
            assert abs(float(got) - ref) <= 1e-5 * max(1, abs(ref)), (i, float(got), ref)
    for k in p:
        check_maxabs(host(net.get_variable(k)), p[k], 2e-5, what='weights after 3 steps ' + k)


def test_two_identical_runs_are_bit_identical():
    outs = []
    for _ in range(2):
        net, p, x, y = _setup(16, 112, 112, 3, 1000, seed=41)
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': 1000, 'num_examples': 16}
        step, losses, _, _ = Singular(net, 0.05, 'Momentum')(inputs)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        outs.append((net.params.clone(), net.grads.clone()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    assert float(outs[0][1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ graph nets
def test_graph_net_head_parity():
    """the MagFace head of the BN nets on the classifier's own input (the dropped-out pooled features) and weights: the three
    losses, the classifier-weight gradient and the gradient into the features (tests/test_gpu_adaface.py)"""
    n, h, w, ncls = 8, 64, 64, 10
    net = net_select('ResNet-50-magface', 'NCHW', 5e-4)
    assert net.head == 'magface' and _hyper(net) == PRESET
    rng = np.random.default_rng(51)
    x = rng.uniform(-1, 1, (n, h, w, 3)) * np.linspace(0.3, 3.0, n)[:, None, None, None]
    xd, yd = dev(x), dev(rng.integers(0, ncls, n), torch.int32)
    net.build(h, w, 3, ncls, 'cuda')
    wname = 'classifier/fc_classifier/weights'
    net.set_variable(wname, torch.tensor(rng.standard_normal((2048, ncls)) * 0.05, dtype=torch.float32))
    net.tower_scale = 1.0
    # a construction-style pass first: it shows the feature norms; l_a and u_a go between them
    net.update_moving_stats = False
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    net.loss_function('TOWER', yd, **logits)
    torch.cuda.synchronize()
    net.update_moving_stats = True
    q = np.sort(np.linalg.norm(host(net.t['features_drop']).astype(np.float64), axis=1))
    net.set_magface(l_a=float(np.float32(0.5 * (q[1] + q[2]))), u_a=float(np.float32(0.5 * (q[-3] + q[-2]))))
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **logits)
    stages = net.backward_stages()
    stages[0]()                                               # the classifier bucket
    torch.cuda.synchronize()
    feat = host(net.t['features_drop'])
    gin = host(net._grad['features_drop'])
    gw = host(net.get_variable(wname, net.grads))
    W = host(net.get_variable(wname))
    y = host(yd).astype(int)
    hyper = _hyper(net)
    gaps = gr.head_gaps(feat, W, y, *hyper[1:5])
    fn = np.linalg.norm(feat.astype(np.float64), axis=1)
    print('gaps', gaps, 'norms', fn, 'l_a, u_a', hyper[1:3])
    assert _gaps_ok(gaps)
    assert (fn < hyper[1]).any() and (fn > hyper[2]).any() and ((fn > hyper[1]) & (fn < hyper[2])).any()
    ce_r, mag_r, fr, dxr, dWr = gr.head_fwd_bwd(feat, W, y, *hyper)
    assert names == ['cross_entropy', 'magnitude_loss', 'reg_loss']
    assert abs(float(losses[0]) - ce_r) <= 2e-5 * max(1.0, abs(ce_r)), (float(losses[0]), ce_r)
    assert abs(float(losses[1]) - mag_r) <= 2e-5 * max(1.0, abs(mag_r)), (float(losses[1]), mag_r)
    check_rell2(gw, dWr, what='classifier weight gradient')
    check_rell2(gin, dxr, what='gradient into the features')
    for st in stages[1:]:
        st()
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads).all()


def test_iresnet18_magface_one_step():
    from tf_face_toolbox_amd.nets.iresnet import IResNet
    n, h, w, ncls = 4, 32, 32, 10
    net = IResNet(num_layers=18, data_format='NCHW', weight_decay=5e-4, head='magface', blocks=[1, 1, 1, 1])
    assert net.head == 'magface' and _hyper(net) == PRESET
    rng = np.random.default_rng(53)
    inputs = {'images': dev(rng.uniform(-1, 1, (n, h, w, 3))), 'labels': dev(rng.integers(0, ncls, n), torch.int32),
              'num_classes': ncls, 'num_examples': n}
    step, losses, names, _ = Singular(net, 0.05, 'Momentum')(inputs)
    before = net.params.clone()
    step()
    torch.cuda.synchronize()
    assert names == ['cross_entropy', 'magnitude_loss', 'reg_loss']
    vals = [float(v) for v in losses]
    assert all(np.isfinite(v) for v in vals), vals
    # magnitude_loss is lambda_g * mean g of the classifier's input
    a = np.clip(np.linalg.norm(host(net.t[net.plan[-1].inp]).astype(np.float64), axis=1), 10.0, 110.0)
    want = 35.0 * (a / 110.0 ** 2 + 1 / a).mean()
    assert abs(vals[1] - want) <= 1e-5 * want, (vals[1], want)
    assert torch.isfinite(net.params).all() and not torch.equal(net.params, before)


# ------------------------------------------------------------------------------------------------ checkpoints, CLI, two ranks
def test_checkpoint_round_trip_resumes_bit_for_bit(tmp_path):
    n, h, w, ch, ncls = 4, 32, 32, 3, 10

    def start(name=NAME):
        net, p, x, y = _setup(n, h, w, ch, ncls, seed=61, name=NAME)
        if name != NAME:                                            # the same inputs and parameters under another head
            net = net_select(name, 'NCHW', 5e-4)
            net.build(h, w, ch, ncls, 'cuda')
            net.load_params(p)
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
        model = Singular(net, 0.05, 'Momentum')
        step, losses, _, _ = model(inputs)
        return net, model, step, losses
    net, model, step, losses = start()
    step(); step()
    torch.cuda.synchronize()
    path = saver.save(net, model._opt.slots, model.global_step, str(tmp_path / 'c' / 'c.ckpt'))
    saved_params = net.params.clone()
    step()
    torch.cuda.synchronize()
    want = (net.params.clone(), [float(v) for v in losses])
    net2, model2, step2, losses2 = start()
    model2.global_step = saver.restore(net2, path, optimizer=model2._opt)
    assert model2.global_step == 2
    step2()
    torch.cuda.synchronize()
    assert torch.equal(net2.params, want[0]) and [float(v) for v in losses2] == want[1]
    # the head has no state and the ArcFace net's variable names: checkpoints cross between the two heads, both ways
    arc, amodel, astep, alosses = start('SphereNet-ArcFace')
    amodel.global_step = saver.restore(arc, path, optimizer=amodel._opt)
    assert amodel.global_step == 2
    assert list(arc.variables) == list(net.variables) and torch.equal(arc.params, saved_params)
    astep()
    torch.cuda.synchronize()
    apath = saver.save(arc, amodel._opt.slots, amodel.global_step, str(tmp_path / 'a' / 'a.ckpt'))
    net3, model3, step3, losses3 = start()
    model3.global_step = saver.restore(net3, apath, optimizer=model3._opt)
    assert model3.global_step == 3
    assert torch.equal(net3.params, arc.params)
    step3()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in losses3)


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_train_synthetic_save_evaluate(tmp_path):
    from PIL import Image
    from scipy.io import loadmat
    from tf_face_toolbox_amd import verification as V
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        path = str(tmp_path / ('im%d.png' % i))
        Image.fromarray(rng.integers(0, 255, (32, 32, 3), dtype=np.uint8)).save(path)
        lines.append('%s %d' % (path, i % 3))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', NAME, '--model_name', 'm', '--synthetic', '1',
                '--synthetic_classes', '10', '--input_height', '32', '--input_width', '32', '--batch_size', '8', '--num_gpus', '1',
                '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
                '--save_interval', '1000', '--max_steps', '2', '--magface', '2,30,0.3,0.7,1', '--margin_scale', '32'], str(tmp_path))
    assert 'Loss #0: cross_entropy' in out and 'Loss #1: magnitude_loss' in out and 'Loss #2: reg_loss' in out
    assert 'lambda_g = 1 is below' in out and out.count('is below') == 1          # the notice, once
    assert 'Model has been saved in Iteration 1' in out
    ckpt = str(tmp_path / 'models' / (NAME + '_m') / (NAME + '_m.ckpt-2'))
    saved = torch.load(ckpt, map_location='cpu')['variables']
    assert not any(k.startswith('classifier/magface') for k in saved)             # no state variable
    out = _run([os.path.join(ROOT, 'evaluate.py'), '--net_name', NAME, '--model_name', 'm', '--fea_name', 'f',
                '--data_list_path', str(tmp_path / 'list.txt'), '--input_height', '32', '--input_width', '32', '--batch_size', '4'],
               str(tmp_path))
    assert 'Totally extracted 6 features.' in out
    m = loadmat(str(tmp_path / 'features' / (NAME + '_m') / 'f_2.mat'))
    fea = np.asarray(m['wfea'], np.float32)
    assert fea.shape == (6, 512) and np.isfinite(fea).all() and np.abs(fea).max() > 0
    # the features are saved raw: their norms are the quality scores
    qual = host(V.feature_quality(fea))
    want = np.linalg.norm(fea.astype(np.float64), axis=1)
    assert qual.shape == (6,) and np.all(np.abs(qual - want) <= 1e-6 * want) and want.std() > 0
    assert torch.equal(V.feature_quality(dev(fea)), V.normalize(dev(fea), return_norms=True)[1])
    # a preset run on the deep net of the issue's example logs the third loss too
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', 'IResNet-50-magface', '--model_name', 'i', '--synthetic', '1',
                '--synthetic_classes', '10', '--input_height', '32', '--input_width', '32', '--batch_size', '4', '--num_gpus', '1',
                '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
                '--save_interval', '1000', '--max_steps', '1'], str(tmp_path))
    assert 'Loss #1: magnitude_loss' in out and 'is below' not in out
    # refused on the command line
    for extra, word in ((['--margin', '0.3'], '--magface'),):       # (the other refusals: tests/test_magface_host.py)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--net_name', NAME, '--model_name', 'r', '--synthetic', '1', '--batch_size', '8'] + extra,
                           cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=600)
        assert r.returncode != 0 and word in r.stdout, (extra, r.stdout[-1000:])


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_keep_the_trainable_variables_identical(tmp_path):
    """two DataParallel_margin ranks (tests/dp_worker.py; one GPU: both on it over gloo): the all-reduced gradients keep every
    trainable variable bit-identical across the ranks, the three losses travel with the gradient arena and are finite"""
    n, h, w, ch, ncls, steps = 8, 32, 32, 3, 20, 2
    p = osn.perturb_params(osn.init_params(71, ch, ncls, h, w), 72)
    rng = np.random.default_rng(73)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    fix = str(tmp_path / 'fix.npz')
    np.savez(fix, x=x, y=y, ncls=ncls, **{'p:' + k: v for k, v in p.items()})
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
                        os.path.join(ROOT, 'tests', 'dp_worker.py'), fix, out, NAME, str(steps)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    r0, r1 = np.load(out + '.rank0.npz'), np.load(out + '.rank1.npz')
    nw = 0
    for k in r0.files:
        if k.startswith('w:'):
            np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
            nw += 1
    assert nw > 0 and not any(k.startswith('s:classifier/magface') for k in r0.files)
    assert np.isfinite(r0['losses']).all() and np.isfinite(r1['losses']).all() and r0['losses'].shape == (steps, 3)
    np.testing.assert_array_equal(r0['losses'], r1['losses'])      # the all-reduced loss slots: the same on both ranks
    assert (r0['losses'][:, 1] > 0).all()                           # magnitude_loss = lambda_g * mean g > 0


# ------------------------------------------------------------------------------------------------ verify.py --weight_by_norm
def _toy_templates(tmp):
    """a toy template set whose feature norms spread over two decades: the norm weights matter"""
    from scipy.io import savemat
    rng = np.random.default_rng(5)
    centers = rng.standard_normal((6, 64))
    rows, feats = [], []
    for t in range(24):
        sub = t % 6
        for med in range(1 + t % 3):
            for j in range(1 + (t + med) % 4):
                rows.append((t + 1, sub, 'frames/%d_%d_%d.jpg' % (t, med, j), '%d_%d' % (t, med)))
                feats.append((centers[sub] + 3.0 * rng.standard_normal(64)) * 10.0 ** rng.uniform(-1, 1))
    x = np.asarray(feats, np.float32)
    savemat(str(tmp / 'set.mat'), {'wfea': x})
    with open(str(tmp / 'set.csv'), 'w') as f:
        f.write('TEMPLATE_ID,SUBJECT_ID,FILE,MEDIA_ID,Q\n')
        for t, s, fn, m in rows:
            f.write('%d,%d,%s,%s,1.0\n' % (t, s, fn, m))
    with open(str(tmp / 'set.txt'), 'w') as f:
        for t, s, fn, m in rows:
            f.write('/data/ijb/%s %d\n' % (fn, s))
    return x, rows


def test_verify_weight_by_norm(tmp_path):
    import json
    import verify
    from tf_face_toolbox_amd import verification as V
    x, rows = _toy_templates(tmp_path)
    meta = V.read_template_metadata(str(tmp_path / 'set.csv'))
    tpl = V.build_templates(meta)
    x64 = x.astype(np.float64)
    nrm = np.linalg.norm(x64, axis=1)
    want = tr.pool(x64 / nrm[:, None], tpl['members'], tpl['media_off'], tpl['tmpl_off'], nrm)
    plain = tr.pool(x64 / nrm[:, None], tpl['members'], tpl['media_off'], tpl['tmpl_off'])
    got = host(verify._pooled(x, tpl, meta, True))[:, :64]
    assert np.abs(got - want).max() <= 2e-6 and np.abs(want - plain).max() > 1e-2          # weighted, and the weights matter
    assert np.abs(host(verify._pooled(x, tpl, meta, False))[:, :64] - plain).max() <= 2e-6
    # the command line: scores of all template pairs against the numpy pooling
    tids = tpl['template_ids'].tolist()
    ia, ib = np.triu_indices(len(tids), 1)
    with open(str(tmp_path / 'pairs.txt'), 'w') as f:
        for a, b in zip(ia, ib):
            f.write('%d %d\n' % (tids[a], tids[b]))
    subj = np.asarray(tpl['subjects'])
    genuine = subj[ia] == subj[ib]
    base = ['--protocol', 'templates', '--feature_path', str(tmp_path / 'set.mat'), '--data_list_path', str(tmp_path / 'set.txt'),
            '--template_metadata', str(tmp_path / 'set.csv'), '--template_pairs', str(tmp_path / 'pairs.txt')]
    res = {}
    for tag, extra in (('norm', ['--weight_by_norm', '1']), ('plain', [])):
        out = str(tmp_path / (tag + '.json'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py')] + base + extra + ['--output_json', out], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        res[tag] = json.load(open(out))
    fars = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
    for tag, P in (('norm', want), ('plain', plain)):
        ref = tr.tar_at_far((P[ia] * P[ib]).sum(1), genuine, fars)
        for row, r_ in zip(res[tag]['tar_at_far'], ref):
            assert (r_ is None) == (row['tar'] == 'n/a'), (tag, row, r_)
            if r_ is not None:
                assert abs(row['tar'] - r_[0]) <= 1.01 / genuine.sum() and abs(row['threshold'] - r_[2]) <= 1e-5, (tag, row, r_)
    thr = [(a['threshold'], b['threshold']) for a, b in zip(res['norm']['tar_at_far'], res['plain']['tar_at_far']) if a['tar'] != 'n/a']
    assert thr and any(abs(a - b) > 1e-4 for a, b in thr)          # the flag changed the scores
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py')] + base + ['--weight_by_norm', '1', '--weight_column', 'Q'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--weight_column' in (r.stdout + r.stderr)
