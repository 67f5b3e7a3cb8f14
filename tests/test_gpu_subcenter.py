"""-m gpu: the sub-center ArcFace head (include/fte.h fte_subcenter_margin_softmax_fwd_bwd / fte_subcenter_colcoef) against the float64
restatement (tests/subcenter_ref.py) fed the GPU's own s / xn / wn, bit-identity with the one-centre head at K = 1, exact ties, the
zeros, both paths, the public loss, both net families, the assignment kernel, the cleaning pass and the command lines.

The winner of the pool is discontinuous: a (row, class) pair whose top two cosines lie within 1e-5 of each other in the restatement is
left out of the G comparison (and its class's columns out of the colcoef comparison) -- nothing else is.  At most 0.5 % of a case's pairs
may be left out and never a target pair; both are asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as mr
import subcenter_ref as sr
from oracle import spherenet as osn
from test_subcenter_host import cleaning_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2, kink_of, ws, call, stream
    from tf_face_toolbox_amd import net_select, saver, subcenter, _lib
    from tf_face_toolbox_amd.loss import additive_margin_loss, subcenter_margin_loss
    from test_gpu_margin import _features

ARC, COS, MIX = (64.0, 0.5, 0.0), (64.0, 0.0, 0.35), (30.0, 0.3, 0.2)
D = 512
NEAR = 1e-5
CLS = 'classifier/fc_classifier/weights'


def _raw(n, c, K, seed):
    """tests/test_gpu_margin.py::_raw per plane: (s [n, K * ldp], xn [n], wn [K * ldp], labels, ldp) computed on the GPU"""
    rng = np.random.default_rng(seed)
    ldp = (c + 127) // 128 * 128
    W = np.zeros((D, K, ldp), np.float32)
    W[:, :, :c] = rng.standard_normal((D, K, c), dtype=np.float32)
    y = rng.integers(0, c, n)
    y[0] = 0
    y[-1] = c - 1
    x = _features(rng, W[:, 0], y, n)
    xd, Wd = dev(x), dev(W.reshape(D, K * ldp))
    s = torch.empty(n, K * ldp, dtype=torch.float32, device='cuda')
    xn = torch.empty(n, dtype=torch.float32, device='cuda')
    wn = torch.empty(K * ldp, dtype=torch.float32, device='cuda')
    w_, wb = ws(_lib.query('fte_gemm_ws_bytes', n, K * ldp, D))
    call('fte_gemm_nn', xd, Wd, None, s, n, K * ldp, D, w_, wb, stream())
    call('fte_row_norms', xd, xn, n, D, D, stream())
    call('fte_col_norms', Wd, wn, D, K * ldp, K * ldp, stream())
    return s, xn, wn, dev(y, torch.int32), ldp


def _kernel(s, xn, wn, labels, K, c, ld, S, m, m3, gs, with_f=True):
    n = s.shape[0]
    f = torch.full((n, ld), 7.0, device='cuda') if with_f else None
    G = torch.full((n, K * ld), 7.0, device='cuda')
    rows, rc = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    call('fte_subcenter_margin_softmax_fwd_bwd', s, xn, wn, labels, K, S, m, m3, f, rows, G, rc, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, G, rc


def _colcoef(G, s, wn, K, c, ld):
    cc = torch.full((K * ld,), 7.0, device='cuda')
    call('fte_subcenter_colcoef', G, s, wn, cc, K, s.shape[0], c, ld, stream())
    torch.cuda.synchronize()
    return cc


def _check_head(got, s, xn, wn, labels, K, c, ld, S, m, m3, gs, what, cc=None):
    """test_gpu_margin.py::_check_head's bounds on the same quantities, for K planes; `cc`: the kernel's colcoef, checked too"""
    f, rows, G, rc = got
    sh, xh, wh, yh = host(s), host(xn), host(wn), host(labels).astype(int)
    n = sh.shape[0]
    fr, lr, Gr, rcr = sr.kernel_ref(sh, xh, wh, yh, K, S, m, m3, gs, c, ld)
    ok = np.isfinite(lr)
    cos, _ = sr.plane_cos(sh, xh, wh, K, c, ld)
    near = sr.gaps(cos) < NEAR                                    # [n, c]: pairs whose winner fp32 may legitimately call otherwise
    print('%s: %d of %d pairs within %g' % (what, near.sum(), near.size, NEAR))
    assert near.mean() <= 0.005, (what, near.mean())
    idx, yc = np.arange(n), np.clip(yh, 0, c - 1)
    assert not near[idx[ok], yc[ok]].any(), what + ': a target pair is near a tie'
    if f is not None:
        check_maxabs(host(f)[ok], fr[ok], what=what + ' f')
        assert (host(f)[:, c:] == 0).all(), what
    Gg, Grr = host(G).reshape(n, K, ld), Gr.reshape(n, K, ld).copy()
    assert (Gg[:, :, c:] == 0).all(), what + ': padding columns of every plane'
    cmax, kst = sr.pool(cos)
    loser = (np.arange(K)[None, :, None] != kst[:, None, :]) & ~near[:, None, :] & ok[:, None, None]
    assert (Gg[:, :, :c][loser] == 0).all(), what + ': a centre that did not win has a gradient'
    skip = np.zeros((n, K, ld), bool)
    skip[:, :, :c] = near[:, None, :]
    Gc = np.where(skip, 0.0, Gg)
    Grr[skip] = 0.0
    check_maxabs(Gc[ok], Grr[ok], what=what + ' G')
    check_rell2(Gc[ok], Grr[ok], what=what + ' G')
    lg = host(rows)[ok]
    assert np.all(np.abs(lg - lr[ok]) <= 2e-5 * np.maximum(1.0, np.abs(lr[ok]))), (what, np.abs(lg - lr[ok]).max())
    # rowcoef: as in test_gpu_margin.py, against the sum of the magnitudes of its terms (on the pooled cosines)
    xv = np.maximum(xh, 1e-12)
    z = np.where(np.isfinite(fr[:, :c]), fr[:, :c], 0)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    _, tp = mr.target(cmax[idx, yc], m, m3)
    wgt = p.copy()
    wgt[idx, yc] = (p[idx, yc] + 1) * tp
    mag = abs(gs) * S * (wgt * np.abs(cmax)).sum(1) / xv ** 2
    assert np.all(np.abs(host(rc)[ok] - rcr[ok]) <= 2e-5 * mag[ok]), (what, 'rowcoef', np.abs(host(rc)[ok] - rcr[ok]) / mag[ok])
    if cc is not None:
        # colcoef likewise: G s = dL/dc * c, so column (k, j) is -sum over the rows that chose centre k of dL/dc_ij c_ij / wn^2; its
        # magnitude is the same sum of |terms|, the target's weight again (p_y + 1) t' (p_y - 1 cancels where p_y is 1 to fp32)
        assert ok.all()
        ccr = sr.colcoef_ref(Gr, sh, wh, K, c, ld).reshape(K, ld)
        ccg = host(cc).reshape(K, ld)
        assert (ccg[:, c:] == 0).all(), what + ': colcoef pads'
        cmag = np.zeros((K, ld))
        for k in range(K):
            cmag[k, :c] = (abs(gs) * S * wgt * np.abs(cmax) * (kst == k)).sum(0) / wh.reshape(K, ld)[k, :c] ** 2
        live = np.zeros((K, ld), bool)
        live[:, :c] = ~near.any(0)[None, :]
        assert np.all(np.abs(ccg - ccr)[live] <= 2e-5 * cmag[live] + 1e-30), (what, 'colcoef')
    return fr, Gr


# K = 5 and 8 hold one chunk per trip: c = 1030 is their smallest shape with a second trip, its last chunk partly filled
@pytest.mark.parametrize('n,c,K', [(n, c, K) for K in (2, 3, 4) for c in (10, 1000, 4100) for n in (1, 7, 64)] +
                         [(n, c, K) for K in (5, 8) for n, c in ((1, 10), (7, 1030))])
def test_kernel_against_the_restatement(n, c, K):
    s, xn, wn, labels, ld = _raw(n, c, K, seed=n * 7 + c + 100 * K)
    for S, m, m3 in (ARC, COS, MIX):
        got = _kernel(s, xn, wn, labels, K, c, ld, S, m, m3, 1.0 / n)
        _check_head(got, s, xn, wn, labels, K, c, ld, S, m, m3, 1.0 / n, 'n=%d c=%d K=%d S=%g m=%g m3=%g' % (n, c, K, S, m, m3),
                    cc=_colcoef(got[2], s, wn, K, c, ld))


@pytest.mark.parametrize('n,c', [(7, 1000), (64, 4100)])
def test_one_centre_is_bit_identical_to_the_margin_head(n, c):
    s, xn, wn, labels, ld = _raw(n, c, 1, seed=3 + n)
    for S, m, m3 in (ARC, COS, MIX):
        f0, G0 = torch.full((n, ld), 7.0, device='cuda'), torch.full((n, ld), 7.0, device='cuda')
        r0, rc0, cc0 = torch.empty(n, device='cuda'), torch.empty(n, device='cuda'), torch.empty(ld, device='cuda')
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, S, m, m3, f0, r0, G0, rc0, n, c, ld, 1.0 / n, stream())
        call('fte_asoftmax_colcoef', G0, s, wn, cc0, n, c, ld, stream())
        f, rows, G, rc = _kernel(s, xn, wn, labels, 1, c, ld, S, m, m3, 1.0 / n)
        assert torch.equal(f, f0) and torch.equal(rows, r0) and torch.equal(G, G0) and torch.equal(rc, rc0)
        assert torch.equal(_colcoef(G, s, wn, 1, c, ld), cc0)
        # and on the scalar path (an ld that is no multiple of 4)
        su = torch.zeros(n, c + 3, device='cuda')
        su[:, :c] = s[:, :c]
        f0, G0 = torch.empty(n, c + 3, device='cuda'), torch.empty(n, c + 3, device='cuda')
        call('fte_margin_softmax_fwd_bwd', su, xn, wn, labels, S, m, m3, f0, r0, G0, rc0, n, c, c + 3, 1.0 / n, stream())
        f, rows, G, rc = _kernel(su, xn, wn, labels, 1, c, c + 3, S, m, m3, 1.0 / n)
        assert torch.equal(f, f0) and torch.equal(rows, r0) and torch.equal(G, G0) and torch.equal(rc, rc0)


@pytest.mark.parametrize('n,c', [(7, 1000), (5, 10)])
def test_exact_ties_go_to_the_lowest_centre(n, c):
    """s and wn written so that centres are bitwise equal: planes 0 and 2 tie above plane 1 (two-way), or all three tie; the target
    classes of rows 0, 1 and n - 1 among them"""
    K = 3
    s, xn, wn, labels, ld = _raw(n, c, K, seed=17)
    labels[1] = 1
    two, three = [0, 5, c - 1], [1, 7]
    sp, wp = s.reshape(n, K, ld), wn.reshape(K, ld)
    for j in two + three:
        sp[:, 2, j] = sp[:, 0, j]
        wp[2, j] = wp[0, j]
    for j in three:
        sp[:, 1, j] = sp[:, 0, j]
        wp[1, j] = wp[0, j]
    for j in two:
        sp[:, 1, j] = -2.0 * xn * wp[1, j]                      # cosine -1: below the tie
    for S, m, m3 in (ARC, COS):
        f, rows, G, rc = _kernel(s, xn, wn, labels, K, c, ld, S, m, m3, 1.0 / n)
        Gg = host(G).reshape(n, K, ld)
        fr, lr, Gr, rcr = sr.kernel_ref(host(s), host(xn), host(wn), host(labels).astype(int), K, S, m, m3, 1.0 / n, c, ld)
        Gr = Gr.reshape(n, K, ld)
        tie = two + three
        assert (Gg[:, 1:, tie] == 0).all()
        assert (Gg[:, 0, tie] != 0).mean() >= 0.9              # (a target whose p_y is 1.0f has the gradient 0.0 in plane 0 as well)
        assert (Gr[:, 1:, tie] == 0).all()                      # the restatement's rule is the same one
        check_maxabs(Gg[:, 0, tie], Gr[:, 0, tie], what='G of the tied classes')
        check_maxabs(host(f), fr, what='f')
        assert np.all(np.abs(host(rows) - lr) <= 2e-5 * np.maximum(1.0, np.abs(lr)))
        cc = host(_colcoef(G, s, wn, K, c, ld)).reshape(K, ld)
        assert (cc[1:, tie] == 0).all() and (cc[:, c:] == 0).all()


def test_unaligned_ld_takes_the_scalar_path():
    n, c, K = 7, 1000, 3
    s, xn, wn, labels, ldp = _raw(n, c, K, seed=9)
    ld = c + 3
    su, wu = torch.zeros(n, K, ld, device='cuda'), torch.zeros(K, ld, device='cuda')
    su[:, :, :c] = s.reshape(n, K, ldp)[:, :, :c]
    wu[:, :c] = wn.reshape(K, ldp)[:, :c]
    su, wu = su.reshape(n, K * ld), wu.reshape(K * ld)
    for p in (ARC, COS):
        got = _kernel(su, xn, wu, labels, K, c, ld, *p, 1.0 / n)
        _check_head(got, su, xn, wu, labels, K, c, ld, *p, 1.0 / n, 'ld=%d' % ld, cc=_colcoef(got[2], su, wu, K, c, ld))
        vec = _kernel(s, xn, wn, labels, K, c, ldp, *p, 1.0 / n)                         # the vector path on the same planes
        check_maxabs(host(got[2]).reshape(n, K, ld)[:, :, :c], host(vec[2]).reshape(n, K, ldp)[:, :, :c], what='scalar vs vector G')


def test_out_of_range_label_gives_a_nan_row_in_every_plane():
    n, c, K = 7, 1000, 3
    s, xn, wn, labels, ld = _raw(n, c, K, seed=11)
    clean = _kernel(s, xn, wn, labels, K, c, ld, *ARC, 1.0 / n)
    labels[3] = c
    labels[5] = -1
    labels[1] = c + 5                                           # a pad column
    f, rows, G, rc = _kernel(s, xn, wn, labels, K, c, ld, *ARC, 1.0 / n)
    Gp = G.reshape(n, K, ld)
    for i in (1, 3, 5):
        assert np.isnan(float(rows[i])) and np.isnan(float(rc[i]))
        assert torch.isnan(Gp[i, :, :c]).all() and torch.isnan(f[i, :c]).all()
    assert (Gp[:, :, c:] == 0).all() and (f[:, c:] == 0).all()                          # padding: 0, on the NaN rows too
    good = [0, 2, 4, 6]
    for a, b in zip(clean, (f, rows, G, rc)):
        assert torch.equal(a[good], b[good])                   # the other rows: bitwise what they are without the bad rows


def test_f_null_gives_the_same_G_and_repeats_bit_for_bit():
    n, c, K = 64, 4100, 3
    s, xn, wn, labels, ld = _raw(n, c, K, seed=13)
    a = _kernel(s, xn, wn, labels, K, c, ld, *ARC, 1.0 / n, with_f=True)
    b = _kernel(s, xn, wn, labels, K, c, ld, *ARC, 1.0 / n, with_f=False)
    c2 = _kernel(s, xn, wn, labels, K, c, ld, *ARC, 1.0 / n, with_f=False)
    for i in (1, 2, 3):
        assert torch.equal(a[i], b[i]) and torch.equal(b[i], c2[i])


def test_invalid_arguments():
    K = 2
    s, xn, wn, labels, ld = _raw(4, 10, K, seed=1)
    G, rows, rc, cc = torch.empty_like(s), torch.empty(4, device='cuda'), torch.empty(4, device='cuda'), torch.empty(K * ld, device='cuda')
    name = 'fte_subcenter_margin_softmax_fwd_bwd'
    for k_, S, m, m3, c, ld_ in ((0, 64.0, 0.5, 0.0, 10, ld), (9, 64.0, 0.5, 0.0, 10, ld), (-1, 64.0, 0.5, 0.0, 10, ld),
                                 (2, 0.0, 0.5, 0.0, 10, ld), (2, 64.0, -0.1, 0.0, 10, ld), (2, 64.0, 0.5, 0.0, 0, ld),
                                 (2, 64.0, 0.5, 0.0, 10, 9), (2, float('nan'), 0.5, 0.0, 10, ld)):
        with pytest.raises(_lib.FteError):
            call(name, s, xn, wn, labels, k_, S, m, m3, None, rows, G, rc, 4, c, ld_, 0.25, stream())
    with pytest.raises(_lib.FteError):
        call(name, s, xn, wn, labels, 2, 64.0, 0.5, 0.0, None, rows, None, rc, 4, 10, ld, 0.25, stream())
    for k_ in (0, 9):
        with pytest.raises(_lib.FteError):
            call('fte_subcenter_colcoef', G, s, wn, cc, k_, 4, 10, ld, stream())
        with pytest.raises(_lib.FteError):
            call('fte_subcenter_assign', s, s, labels, k_, labels, rc, 4, 8, 10, stream())
    call(name, s, xn, wn, labels, 8, 64.0, 0.5, 0.0, None, rows, G, rc, 4, 10, ld // 4, 0.25, stream())      # K = 8 is in range
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ public loss, nets
@pytest.mark.parametrize('preset', [ARC, COS])
def test_public_loss_function(preset):
    rng = np.random.default_rng(17)
    n, c, ld, K = 16, 200, 256, 3
    W = np.zeros((D, K, ld), np.float32)
    W[:, :, :c] = rng.standard_normal((D, K, c))
    y = rng.integers(0, c, n)
    x = _features(rng, W[:, 0], y, n)
    Wp = W.reshape(D, K * ld)
    loss, dx, dW = subcenter_margin_loss(dev(x), dev(Wp), dev(y, torch.int32), K, *preset, num_classes=c)
    torch.cuda.synchronize()
    packed = W[:, :, :c].reshape(D, K * c).astype(np.float64)
    cos, _ = sr.plane_cos(x.astype(np.float64) @ packed, np.linalg.norm(x.astype(np.float64), axis=1), np.linalg.norm(packed, axis=0), K, c, c)
    assert sr.gaps(cos).min() >= NEAR
    lr, _, dxr, dWr = sr.head_fwd_bwd(x.astype(np.float64), packed, y, K, *preset)
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    check_rell2(host(dx), dxr, what='dfeatures')
    dWg = host(dW).reshape(D, K, ld)
    check_rell2(dWg[:, :, :c].reshape(D, K * c), dWr, what='dweights')
    assert (dWg[:, :, c:] == 0).all()
    # K = 1 is additive_margin_loss, bit for bit
    a = subcenter_margin_loss(dev(x), dev(W[:, 0]), dev(y, torch.int32), 1, *preset, num_classes=c)
    b = additive_margin_loss(dev(x), dev(W[:, 0]), dev(y, torch.int32), *preset, num_classes=c)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _setup(name, n, h, w, ch, ncls, K, seed=21):
    p = osn.perturb_params(osn.init_params(seed, ch, K * ncls, h, w), seed + 1)      # the classifier [512, K * C]: planes packed
    rng = np.random.default_rng(seed + 2)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    net = net_select(name, 'NCHW', 5e-4, sub_centers=K)
    net.build(h, w, ch, ncls, 'cuda')
    net.load_params(p)
    return net, p, x, y


def _preset(net):
    return net.margin_scale, net.margin, net.margin_cos


def test_spherenet_forward_loss_and_every_gradient():
    n, h, w, ch, ncls, K = 4, 32, 32, 3, 10, 3
    net, p, x, y = _setup('SphereNet-ArcFace', n, h, w, ch, ncls, K)
    xd, yd = dev(x), dev(y, torch.int32)
    net.tower_scale = 1.0
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    losses, names, others = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    losses_ref, g_ref, ex = sr.loss_and_grads(p, x, y, K, *_preset(net), 5e-4, 'NCHW', kink=kink_of(net))
    emb = ex['embedding']
    cos, _ = sr.plane_cos(emb @ p[CLS], np.linalg.norm(emb, axis=1), np.linalg.norm(p[CLS], axis=0), K, ncls, ncls)
    assert sr.gaps(cos).min() >= NEAR
    assert names == ['cross_entropy', 'reg_loss'] and not others
    check_maxabs(host(net.emb), ex['embedding'], what='embedding')
    check_maxabs(host(logits['logits']), ex['logits'], what='logits')
    assert abs(float(losses[0]) - losses_ref[0]) <= 1e-5 * max(1, abs(losses_ref[0])), (float(losses[0]), losses_ref[0])
    assert abs(float(losses[1]) - losses_ref[1]) <= 1e-5 * max(1, abs(losses_ref[1]))
    for k in p:
        data_grad = g_ref[k] - (5e-4 * p[k] if k.endswith('/weights') else 0)
        check_rell2(host(net.get_variable(k, net.grads)), data_grad, what='grad ' + k)


def test_graph_net_head_parity():
    n, h, w, ncls, K = 8, 64, 64, 10, 3
    net = net_select('ResNet-50-arcface', 'NCHW', 5e-4, sub_centers=K)
    rng = np.random.default_rng(51)
    xd, yd = dev(rng.uniform(-1, 1, (n, h, w, 3))), dev(rng.integers(0, ncls, n), torch.int32)
    net.build(h, w, 3, ncls, 'cuda')
    net.set_variable(CLS, torch.tensor(rng.standard_normal((2048, K * ncls)) * 0.05, dtype=torch.float32))
    net.tower_scale = 1.0
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **logits)
    stages = net.backward_stages()
    stages[0]()                                               # the classifier bucket
    torch.cuda.synchronize()
    feat, gin = host(net.t['features_drop']), host(net._grad['features_drop'])
    gw, W = host(net.get_variable(CLS, net.grads)), host(net.get_variable(CLS))
    assert W.shape == (2048, K * ncls)
    cos, _ = sr.plane_cos(feat @ W, np.linalg.norm(feat, axis=1), np.linalg.norm(W, axis=0), K, ncls, ncls)
    assert sr.gaps(cos).min() >= NEAR
    lr, fr, dxr, dWr = sr.head_fwd_bwd(feat, W, host(yd).astype(int), K, *_preset(net))
    assert names[0] == 'cross_entropy' and abs(float(losses[0]) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(losses[0]), lr)
    check_rell2(gw, dWr, what='classifier weight gradient')
    check_rell2(gin, dxr, what='gradient into the features')
    for st in stages[1:]:
        st()
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads).all()


def test_two_identical_steps_are_bit_identical():
    net, p, x, y = _setup('SphereNet-ArcFace', 8, 32, 32, 3, 100, 3, seed=41)
    xd, yd = dev(x), dev(y, torch.int32)
    arenas = []
    for _ in range(2):
        logits = net.forward(xd, yd, num_classes=100, is_training=True)
        net.loss_function('TOWER', yd, **logits)
        net.backward()
        torch.cuda.synchronize()
        arenas.append(net.grads.clone())
    assert torch.equal(arenas[0], arenas[1]) and float(arenas[0].abs().max()) > 0


def test_one_centre_makes_the_calls_it_always_made(monkeypatch):
    """the launch list of a step with sub_centers = 1: the head's four launches with the parent's arguments, none of the new symbols"""
    n, ncls = 4, 10
    net, p, x, y = _setup('SphereNet-ArcFace', n, 32, 32, 3, ncls, 1)
    xd, yd = dev(x), dev(y, torch.int32)
    seen = []
    real = _lib.call

    def rec(name, *args):
        seen.append((name,) + tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool) and abs(a) < 1 << 20))
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'call', real)
    names = [s[0] for s in seen]
    assert not [s for s in names if 'subcenter' in s]
    i = names.index('fte_row_norms')
    head = [q[:4] for q in seen]                                 # the name and the first three sizes (a stream or a byte count may follow)
    assert head[i:i + 4] == [('fte_row_norms', n, D, D), ('fte_col_norms', D, ncls, 128), ('fte_margin_softmax_fwd_bwd', n, ncls, 128),
                             ('fte_asoftmax_colcoef', n, ncls, 128)], head[i:i + 4]
    assert head[i - 1] == ('fte_gemm_nn', n, 128, D)
    assert ('fte_gemm_tn', n, 128, D) in head and ('fte_add_scaled_rows_cols', D, 128, 128) in head
    # and K = 3: the same places, the K-plane symbols, every width 3 * 128
    net3, _, _, _ = _setup('SphereNet-ArcFace', n, 32, 32, 3, ncls, 3)
    seen3 = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (seen3.append(name), real(name, *a))[1])
    logits = net3.forward(xd, yd, num_classes=ncls, is_training=True)
    net3.loss_function('TOWER', yd, **logits)
    net3.backward()
    torch.cuda.synchronize()
    swap = {'fte_margin_softmax_fwd_bwd': 'fte_subcenter_margin_softmax_fwd_bwd', 'fte_asoftmax_colcoef': 'fte_subcenter_colcoef'}
    assert seen3 == [swap.get(s, s) for s in names]


# ------------------------------------------------------------------------------------------------ assignment kernel
def _assign_case(n, d, K, c=37, seed=0):
    rng = np.random.default_rng(seed + n + d + K)
    Wt = rng.standard_normal((K * c, d)).astype(np.float32) * rng.uniform(0.5, 2.0, (K * c, 1)).astype(np.float32)
    y = rng.integers(0, c, n)
    x = (rng.standard_normal((n, d)) + 0.5 * Wt[rng.integers(0, K, n) * c + y]).astype(np.float32)
    return x, Wt, y, c


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('d', [128, 512])
@pytest.mark.parametrize('n', [1, 65])
def test_assignment_kernel(n, d, K):
    x, Wt, y, c = _assign_case(n, d, K)
    sel, cosv = subcenter.assign(dev(x), dev(Wt), dev(y, torch.int32), K, c)
    torch.cuda.synchronize()
    rs, rc, gap = sr.assign_ref(x, Wt, y, K, c)
    assert np.abs(host(cosv) - rc).max() <= 2e-6, np.abs(host(cosv) - rc).max()
    far = gap >= NEAR
    assert (~far).mean() <= 0.005
    assert np.array_equal(host(sel).astype(int)[far], rs[far])


def test_assignment_does_not_depend_on_position_or_batch():
    n, d, K = 65, 512, 3
    x, Wt, y, c = _assign_case(n, d, K)
    Wd = dev(Wt)
    sel, cosv = subcenter.assign(dev(x), Wd, dev(y, torch.int32), K, c)
    perm = np.random.default_rng(1).permutation(n)
    sel2, cosv2 = subcenter.assign(dev(x[perm]), Wd, dev(y[perm], torch.int32), K, c)
    assert torch.equal(sel[perm], sel2) and torch.equal(cosv[:, perm], cosv2)
    for i in (0, 3, 64):
        s1, c1 = subcenter.assign(dev(x[i:i + 1]), Wd, dev(y[i:i + 1], torch.int32), K, c)
        assert torch.equal(s1, sel[i:i + 1]) and torch.equal(c1, cosv[:, i:i + 1])


def test_assignment_bad_label_and_exact_tie():
    n, d, K = 9, 128, 3
    x, Wt, y, c = _assign_case(n, d, K)
    Wt[2 * c + y[0]] = Wt[1 * c + y[0]]                         # centres 1 and 2 of row 0's class: the same bits
    x[0] = Wt[1 * c + y[0]] * 3.0
    y2 = y.copy()
    y2[4], y2[7] = c, -1
    sel, cosv = subcenter.assign(dev(x), dev(Wt), dev(y2, torch.int32), K, c)
    torch.cuda.synchronize()
    sel, cosv = host(sel).astype(int), host(cosv)
    assert sel[4] == -1 and sel[7] == -1 and np.isnan(cosv[:, [4, 7]]).all()
    good = [i for i in range(n) if i not in (4, 7)]
    assert np.isfinite(cosv[:, good]).all()
    assert sel[0] == 1 and cosv[1, 0] == cosv[2, 0]


# ------------------------------------------------------------------------------------------------ cleaning pass
@pytest.mark.parametrize('d', [128, 512])
def test_cleaning_pass(d, tmp_path, capsys):
    """The hand-built case of test_subcenter_host.py (C = 5, K = 3, mutually orthogonal centres, --angle 50) through subcenter_clean.py.
    d = 128 runs on a checkpoint that holds the classifier alone; SphereNet's embedding is 512 wide, so the restore into a K = 1
    SphereNet-ArcFace is checked with the same construction at d = 512, on a checkpoint a K = 3 SphereNet-ArcFace saved."""
    import subcenter_clean
    C, K = 5, 3
    x, Wt, labels, lines, keep, dominant = cleaning_case(d, C, K)
    W = torch.tensor(Wt.T.copy())                               # [d, K * C], column k * C + j
    if d == 512:
        net = net_select('SphereNet-ArcFace', sub_centers=K).build(32, 32, 3, C, 'cuda')
        net.set_variable(CLS, W)
        model = saver.save(net, [torch.ones_like(net.params)], 11, str(tmp_path / 'k3' / 'k3.ckpt'))
    else:
        model = str(tmp_path / 'k3.ckpt-11')
        torch.save({'global_step': 11, 'variables': {CLS: W}, 'slots': []}, model)
    (tmp_path / 'list.txt').write_text(''.join(lines[:3]) + '\n' + ''.join(lines[3:]))      # a blank line: skipped, as the readers do
    np.save(str(tmp_path / 'fea.npy'), x)
    out_list, out_model = str(tmp_path / 'clean.txt'), str(tmp_path / 'k1' / 'k1.ckpt-11')
    subcenter_clean.main(['--feature_path', str(tmp_path / 'fea.npy'), '--data_list_path', str(tmp_path / 'list.txt'), '--model_path', model,
                          '--sub_centers', '3', '--angle', '50', '--out_list', out_list, '--out_model', out_model, '--chunk', '5'])
    out = capsys.readouterr().out
    assert open(out_list).read() == ''.join(l for l, k in zip(lines, keep) if k)
    for j, (kp, dr) in enumerate(zip([3, 2, 2, 2, 0], [2, 1, 2, 2, 0])):
        assert 'class %d: dominant centre %d, kept %d, dropped %d\n' % (j, dominant[j], kp, dr) in out
    assert 'total: kept 9, dropped 7 of 16 samples' in out and 'samples on non-dominant centres: 3 of 16 (18.7500%)' in out
    state = torch.load(out_model, map_location='cpu')
    want = torch.stack([W[:, dominant[j] * C + j] for j in range(C)], 1)
    assert state['variables'][CLS].dtype == torch.float32 and torch.equal(state['variables'][CLS], want)
    if d == 512:
        assert torch.equal(state['slots'][0][CLS], torch.zeros(512, C)) and state['global_step'] == 11
        k1 = net_select('SphereNet-ArcFace').build(32, 32, 3, C, 'cuda')
        assert saver.restore(k1, out_model) == 11
        assert torch.equal(k1.get_variable(CLS).cpu(), want)
        for name in net.variables:
            if name != CLS:
                assert torch.equal(k1.get_variable(name), net.get_variable(name))


# ------------------------------------------------------------------------------------------------ command lines
def _run(args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-3000:]
    return r.stdout


def test_train_with_sub_centers_saves_and_restores(tmp_path):
    images = os.path.join(ROOT, 'tests', 'golden', 'images')
    common = ['--net_name', 'SphereNet-ArcFace', '--model_name', 's', '--train_list_path', os.path.join(images, 'list.txt'),
              '--input_height', '36', '--input_width', '36', '--crop_height', '32', '--crop_width', '32', '--batch_size', '4',
              '--num_gpus', '1', '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
              '--save_interval', '1000', '--margin', '0.3', '--train_dir', str(tmp_path / 'train'), '--model_dir', str(tmp_path / 'models')]
    out = _run([os.path.join(ROOT, 'train.py')] + common + ['--sub_centers', '3', '--max_steps', '3'], images)
    assert 'Loss #0: cross_entropy' in out and 'Model has been saved in Iteration 2' in out
    ck = torch.load(str(tmp_path / 'models' / 'SphereNet-ArcFace_s' / 'SphereNet-ArcFace_s.ckpt-3'), map_location='cpu')
    assert ck['variables'][CLS].shape == (512, 3 * 4)
    out = _run([os.path.join(ROOT, 'train.py')] + common + ['--sub_centers', '3', '--max_steps', '5'], images)
    assert 'Model restored from' in out and 'Epoch/Step 2/3' in out            # resumed at global_step 3 (8 images / 4: 3 batches per epoch)
    out = _run([os.path.join(ROOT, 'train.py')] + common + ['--max_steps', '5'], images, ok=False)      # the file is K = 3: not a K = 1 net's
    assert '12 columns' in out and '1 * 4 = 4' in out
    out = _run([os.path.join(ROOT, 'train.py')] + common + ['--sub_centers', '3', '--sample_rate', '0.1'], images, ok=False)
    assert '--sub_centers 3' in out and 'class sampler' in out
