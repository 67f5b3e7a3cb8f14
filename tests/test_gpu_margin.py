"""-m gpu: the additive-margin softmax heads (ArcFace / CosFace, include/fte.h fte_margin_softmax_fwd_bwd) -- the kernel against
the float64 restatement (tests/margin_ref.py) fed the GPU's own s / xn / wn, the public loss function, SphereNet-ArcFace /
-CosFace against the oracle backbone composed with the restatement, the graph nets' margin head, determinism, the mixed
precision modes, convergence and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as mr
from oracle import spherenet as osn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2, kink_of, ws, call, stream
    from tf_face_toolbox_amd import net_select, Singular, _lib
    from tf_face_toolbox_amd.loss import additive_margin_loss

ARC, COS = (64.0, 0.5, 0.0), (64.0, 0.0, 0.35)
D = 512


def _features(rng, W, y, n):
    """rows whose target cosine spreads over [-0.97, 0.97] (the ArcFace fallback branch below cos(pi - m) included) plus noise"""
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    a = rng.uniform(-0.97, 0.97, n)
    a[:min(n, 2)] = [-0.95, 0.9][:min(n, 2)]
    e = rng.standard_normal((D, n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    x = (a * wy + np.sqrt(1 - a * a) * e) * rng.uniform(0.5, 20.0, n)
    return x.T.astype(np.float32)


def _raw(n, c, seed):
    """(s [n, ldp], xn [n], wn [ldp], labels) computed on the GPU: s = x @ W by the library's product, the norms by its kernels"""
    rng = np.random.default_rng(seed)
    ldp = (c + 127) // 128 * 128
    W = np.zeros((D, ldp), np.float32)
    W[:, :c] = rng.standard_normal((D, c), dtype=np.float32)
    y = rng.integers(0, c, n)
    y[0] = 0
    y[-1] = c - 1
    x = _features(rng, W, y, n)
    xd, Wd = dev(x), dev(W)
    s = torch.empty(n, ldp, dtype=torch.float32, device='cuda')
    xn = torch.empty(n, dtype=torch.float32, device='cuda')
    wn = torch.empty(ldp, dtype=torch.float32, device='cuda')
    w_, wb = ws(_lib.query('fte_gemm_ws_bytes', n, ldp, D))
    call('fte_gemm_nn', xd, Wd, None, s, n, ldp, D, w_, wb, stream())
    call('fte_row_norms', xd, xn, n, D, D, stream())
    call('fte_col_norms', Wd, wn, D, c, ldp, stream())
    return s, xn, wn, dev(y, torch.int32)


def _kernel(s, xn, wn, labels, c, S, m, m3, gs, with_f=True):
    n, ld = s.shape
    f = torch.full((n, ld), 7.0, device='cuda') if with_f else None
    G = torch.full((n, ld), 7.0, device='cuda')
    rows = torch.empty(n, device='cuda')
    rc = torch.empty(n, device='cuda')
    call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, S, m, m3, f, rows, G, rc, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, G, rc


def _check_head(got, s, xn, wn, labels, c, S, m, m3, gs, what):
    """the kernel's (f, loss_rows, G, rowcoef) against the restatement on the same s / xn / wn"""
    f, rows, G, rc = got
    sh = host(s)
    fr, lr, Gr, rcr = mr.kernel_ref(sh, host(xn), host(wn), host(labels).astype(int), S, m, m3, gs, c=c)
    ok = np.isfinite(lr)
    ld = sh.shape[1]
    if f is not None:
        check_maxabs(host(f)[ok], fr[ok], what=what + ' f')
        assert (host(f)[:, c:] == 0).all(), what
    check_maxabs(host(G)[ok], Gr[ok], what=what + ' G')
    check_rell2(host(G)[ok], Gr[ok], what=what + ' G')
    assert (host(G)[:, c:ld] == 0).all(), what + ': padding columns'
    lg = host(rows)[ok]
    assert np.all(np.abs(lg - lr[ok]) <= 2e-5 * np.maximum(1.0, np.abs(lr[ok]))), (what, np.abs(lg - lr[ok]).max())
    # rowcoef = -(S gs / xn^2) (sum_j p_j c_j t'_j - t' c_y): a sum of terms of both signs that cancel on a row whose p_y is 1 to
    # within fp32's resolution -- judge its error against the sum of the terms' magnitudes
    xv = np.maximum(host(xn), 1e-12)
    idx, y = np.arange(sh.shape[0]), np.clip(host(labels).astype(int), 0, c - 1)
    cos = np.clip(sh[:, :c] / (xv[:, None] * host(wn)[None, :c]), -1, 1)
    z = np.where(np.isfinite(fr[:, :c]), fr[:, :c], 0)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    _, tp = mr.target(cos[idx, y], m, m3)
    wgt = p.copy()
    wgt[idx, y] = (p[idx, y] + 1) * tp
    mag = abs(gs) * S * (wgt * np.abs(cos)).sum(1) / xv ** 2
    assert np.all(np.abs(host(rc)[ok] - rcr[ok]) <= 2e-5 * mag[ok]), (what, 'rowcoef', np.abs(host(rc)[ok] - rcr[ok]) / mag[ok])
    return fr, Gr


@pytest.mark.parametrize('c', [10, 1000, 10575, 85742])
@pytest.mark.parametrize('n', [1, 7, 64, 512])
def test_kernel_against_the_restatement(n, c):
    s, xn, wn, labels = _raw(n, c, seed=n * 7 + c)
    for S, m, m3 in (ARC, COS, (30.0, 0.3, 0.2)):
        _check_head(_kernel(s, xn, wn, labels, c, S, m, m3, 1.0 / n), s, xn, wn, labels, c, S, m, m3, 1.0 / n,
                    'n=%d c=%d S=%g m=%g m3=%g' % (n, c, S, m, m3))


def test_fallback_branch_is_taken():
    """every target cosine below cos(pi - m): t = c - m sin m (the easy_margin = False fallback), t' = 1"""
    n, c = 64, 1000
    s, xn, wn, labels = _raw(n, c, seed=5)
    sh = host(s)
    rows, y = np.arange(n), host(labels).astype(int)
    den = host(xn) * host(wn)[y]
    sh[rows, y] = -0.99 * den                                   # target cosine -0.99 on every row
    s = dev(sh)
    cy = host(s)[rows, y] / den
    assert (cy < np.cos(np.pi - ARC[1])).all()
    _check_head(_kernel(s, xn, wn, labels, c, *ARC, 1.0 / n), s, xn, wn, labels, c, *ARC, 1.0 / n, 'fallback')


def test_unaligned_ld_takes_the_scalar_path():
    n, c = 7, 1000
    s, xn, wn, labels = _raw(n, c, seed=9)
    ld = c + 3
    su = torch.zeros(n, ld, device='cuda')
    su[:, :c] = s[:, :c]
    for p in (ARC, COS):
        _check_head(_kernel(su, xn, wn, labels, c, *p, 1.0 / n), su, xn, wn, labels, c, *p, 1.0 / n, 'ld=%d' % ld)


def test_out_of_range_label_gives_a_nan_row():
    n, c = 7, 1000
    s, xn, wn, labels = _raw(n, c, seed=11)
    labels[3] = c
    labels[5] = -1
    f, rows, G, rc = _kernel(s, xn, wn, labels, c, *ARC, 1.0 / n)
    for i in (3, 5):
        assert np.isnan(float(rows[i])) and np.isnan(float(rc[i]))
        assert torch.isnan(G[i, :c]).all() and torch.isnan(f[i, :c]).all()
    assert (G[:, c:] == 0).all() and (f[:, c:] == 0).all()                  # padding: 0, on the NaN rows too
    good = [0, 1, 2, 4, 6]
    _check_head((f[good], rows[good], G[good], rc[good]), s[good], xn[good], wn, labels[good], c, *ARC, 1.0 / n, 'other rows')


def test_f_null_gives_the_same_G_and_repeats_bit_for_bit():
    n, c = 64, 10575
    s, xn, wn, labels = _raw(n, c, seed=13)
    a = _kernel(s, xn, wn, labels, c, *ARC, 1.0 / n, with_f=True)
    b = _kernel(s, xn, wn, labels, c, *ARC, 1.0 / n, with_f=False)
    c2 = _kernel(s, xn, wn, labels, c, *ARC, 1.0 / n, with_f=False)
    for i in (1, 2, 3):
        assert torch.equal(a[i], b[i]) and torch.equal(b[i], c2[i])


def test_invalid_arguments():
    s, xn, wn, labels = _raw(4, 10, seed=1)
    G, rows, rc = torch.empty_like(s), torch.empty(4, device='cuda'), torch.empty(4, device='cuda')
    ld = s.shape[1]
    for args in ((0.0, 0.5, 0.0, 10, ld), (64.0, -0.1, 0.0, 10, ld), (64.0, 0.5, 0.0, 0, ld), (64.0, 0.5, 0.0, 10, 9),
                 (float('nan'), 0.5, 0.0, 10, ld)):
        S, m, m3, c, ld_ = args
        with pytest.raises(_lib.FteError):
            call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, S, m, m3, None, rows, G, rc, 4, c, ld_, 0.25, stream())
    with pytest.raises(_lib.FteError):
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, 64.0, 0.5, 0.0, None, rows, None, rc, 4, 10, ld, 0.25, stream())


@pytest.mark.parametrize('preset', [ARC, COS])
def test_public_loss_function(preset):
    rng = np.random.default_rng(17)
    n, c, ld = 64, 1000, 1024
    W = np.zeros((D, ld), np.float32)
    W[:, :c] = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    x = _features(rng, W, y, n)
    loss, dx, dW = additive_margin_loss(dev(x), dev(W), dev(y, torch.int32), *preset, num_classes=c)
    torch.cuda.synchronize()
    lr, _, dxr, dWr = mr.head_fwd_bwd(x.astype(np.float64), W[:, :c].astype(np.float64), y, *preset)
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    check_rell2(host(dx), dxr, what='dfeatures')
    check_rell2(host(dW)[:, :c], dWr, what='dweights')
    assert (host(dW)[:, c:] == 0).all()


# ------------------------------------------------------------------------------------------------ SphereNet
def _setup(name, n, h, w, ch, ncls, seed=21):
    p = osn.perturb_params(osn.init_params(seed, ch, ncls, h, w), seed + 1)
    rng = np.random.default_rng(seed + 2)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    net = net_select(name, 'NCHW', 5e-4)
    net.build(h, w, ch, ncls, 'cuda')
    net.load_params(p)
    return net, p, x, y


def _preset(net):
    return net.margin_scale, net.margin, net.margin_cos


@pytest.mark.parametrize('name,n,h,w,ch,ncls', [
    ('SphereNet-ArcFace', 4, 32, 32, 3, 10),
    ('SphereNet-CosFace', 4, 32, 32, 3, 10),
    ('SphereNet-ArcFace', 2, 112, 112, 1, 10575),
    ('SphereNet-CosFace', 2, 112, 112, 1, 10575),
])
def test_spherenet_forward_loss_and_every_gradient(name, n, h, w, ch, ncls):
    net, p, x, y = _setup(name, n, h, w, ch, ncls)
    xd, yd = dev(x), dev(y, torch.int32)
    net.tower_scale = 1.0
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    losses, names, others = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    losses_ref, g_ref, ex = mr.loss_and_grads(p, x, y, *_preset(net), 5e-4, 'NCHW', kink=kink_of(net))
    assert names == ['cross_entropy', 'reg_loss'] and not others
    check_maxabs(host(net.emb), ex['embedding'], what='embedding')
    check_maxabs(host(logits['logits']), ex['logits'], what='logits')
    assert abs(float(losses[0]) - losses_ref[0]) <= 1e-5 * max(1, abs(losses_ref[0])), (float(losses[0]), losses_ref[0])
    assert abs(float(losses[1]) - losses_ref[1]) <= 1e-5 * max(1, abs(losses_ref[1]))
    for k in p:
        data_grad = g_ref[k] - (5e-4 * p[k] if k.endswith('/weights') else 0)
        check_rell2(host(net.get_variable(k, net.grads)), data_grad, what='grad ' + k)


@pytest.mark.parametrize('name', ['SphereNet-ArcFace', 'SphereNet-CosFace'])
def test_three_training_steps_match_oracle(name):
    n, h, w, ch, ncls = 4, 32, 32, 3, 10
    net, p, x, y = _setup(name, n, h, w, ch, ncls, seed=31)
    inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
    step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
    slots = osn.zero_slots(p)
    for t in range(3):
        step()
        p, slots, l_ref = mr.train_step(p, slots, x, y, 0.05, *_preset(net), kink=kink_of(net))
        assert abs(float(losses[0]) - l_ref[0]) <= 1e-5 * max(1, abs(l_ref[0])), (t, float(losses[0]), l_ref)
    for k in p:
        check_maxabs(host(net.get_variable(k)), p[k], 2e-5, what='weights after 3 steps ' + k)


def test_two_identical_steps_are_bit_identical():
    net, p, x, y = _setup('SphereNet-ArcFace', 16, 112, 112, 3, 1000, seed=41)
    xd, yd = dev(x), dev(y, torch.int32)
    arenas = []
    for _ in range(2):
        logits = net.forward(xd, yd, num_classes=1000, is_training=True)
        net.loss_function('TOWER', yd, **logits)
        net.backward()
        torch.cuda.synchronize()
        arenas.append(net.grads.clone())
    assert torch.equal(arenas[0], arenas[1]) and float(arenas[0].abs().max()) > 0


@pytest.mark.parametrize('mode', ['bf16', 'bf16s'])
def test_precision_modes_head_parity(mode):
    """in the mixed-precision modes the head still runs in fp32: parity of the head on the GPU's own s / xn / wn, and a finite step"""
    _lib.set_mfma_dtype(mode)
    try:
        n, ncls = 8, 1000
        net, p, x, y = _setup('SphereNet-ArcFace', n, 112, 112, 3, ncls, seed=43)
        xd, yd = dev(x), dev(y, torch.int32)
        logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
        net.loss_function('TOWER', yd, **logits)
        net.backward()
        torch.cuda.synchronize()
        got = (net.logits_buf, net.loss_rows, net.G, net.rowcoef)
        _, Gr = _check_head(got, net.s_raw, net.xn, net.wn, yd, ncls, *_preset(net), 1.0 / n, mode)
        check_maxabs(host(net.colcoef)[:ncls], mr.colcoef_ref(Gr, host(net.s_raw), host(net.wn), ncls)[:ncls], 1e-4, what='colcoef')
        assert torch.isfinite(net.grads).all()
    finally:
        _lib.set_mfma_dtype('f32')


# ------------------------------------------------------------------------------------------------ graph nets
@pytest.mark.parametrize('name', ['ResNet-50-arcface', 'ResNet-50-cosface'])
def test_graph_net_head_parity(name):
    """the margin head of the BN nets on the classifier's own input (the dropped-out pooled features) and weights: loss, the
    classifier-weight gradient (norm term added on the product's stream before the bucket is reduced) and the gradient into the
    features (norm term on the main stream)"""
    n, h, w, ncls = 8, 64, 64, 10
    net = net_select(name, 'NCHW', 5e-4)
    rng = np.random.default_rng(51)
    xd, yd = dev(rng.uniform(-1, 1, (n, h, w, 3))), dev(rng.integers(0, ncls, n), torch.int32)
    net.build(h, w, 3, ncls, 'cuda')
    wname = 'classifier/fc_classifier/weights'
    net.set_variable(wname, torch.tensor(rng.standard_normal((2048, ncls)) * 0.05, dtype=torch.float32))
    net.tower_scale = 1.0
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **logits)
    stages = net.backward_stages()
    stages[0]()                                               # the classifier bucket
    torch.cuda.synchronize()
    feat = host(net.t['features_drop'])
    gin = host(net._grad['features_drop'])
    gw = host(net.get_variable(wname, net.grads))
    W = host(net.get_variable(wname))
    lr, fr, dxr, dWr = mr.head_fwd_bwd(feat, W, host(yd).astype(int), *_preset(net))
    assert names[0] == 'cross_entropy' and abs(float(losses[0]) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(losses[0]), lr)
    check_rell2(gw, dWr, what='classifier weight gradient')
    check_rell2(gin, dxr, what='gradient into the features')
    for st in stages[1:]:
        st()
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads).all()


def test_graph_net_trains():
    net = net_select('ResNet-50-cosface', 'NCHW', 5e-4)
    rng = np.random.default_rng(1)
    n, ncls = 8, 10
    x = dev(rng.uniform(-1, 1, (n, 64, 64, 3))); y = dev(rng.integers(0, ncls, n), torch.int32)
    step, losses, names, _ = Singular(net, 0.01, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
    hist = []
    for _ in range(30):
        step()
        hist.append(float(losses[0]))
    assert all(np.isfinite(hist)) and np.mean(hist[-6:]) < np.mean(hist[:6]), hist


# ------------------------------------------------------------------------------------------------ convergence, CLI
def _samples(templates, labels, rng, sigma=0.3):
    x = templates[labels] + sigma * rng.standard_normal((len(labels),) + templates.shape[1:])
    return torch.tensor(np.clip(x, -1, 1), dtype=torch.float32, device='cuda')


@pytest.mark.parametrize('name,margin', [('SphereNet-CosFace', None), ('SphereNet-ArcFace', 0.1)])
def test_identities_become_separable(name, margin):
    """test_gpu_convergence.py's ten-identity task under the margin heads (S = 64): the loss falls and nearest-centroid accuracy on
    fresh samples reaches 0.95.  CosFace runs its preset m3 = 0.35.  ArcFace runs m = 0.1, not its preset 0.5: from scratch, at this
    budget and learning rate, m = 0.5 / 0.3 / 0.2 stall on a plateau at loss 33.2 / 21.2 / 15.1 = S sin m + log 10, the net with every
    cosine near 0 (the untrained net's theta ~ 90 degrees, where the target logit is S cos(90 deg + m) = -S sin m); m = 0.1 reaches
    loss 0 by step 60.  Large-margin ArcFace is usually started from a softmax-trained net or with m ramped up."""
    rng = np.random.default_rng(0)
    ncls, h, w, bs = 10, 32, 32, 64
    templates = rng.uniform(-0.7, 0.7, (ncls, h, w, 3))
    net = net_select(name, 'NCHW', 5e-4)
    net.set_margin(margin=margin)
    state = {}

    def images():
        state['y'] = rng.integers(0, ncls, bs)
        return _samples(templates, state['y'], rng)

    def labels():
        return torch.tensor(state['y'], dtype=torch.int32, device='cuda')
    step, losses, names, _ = Singular(net, 0.01, 'Momentum')({'images': images, 'labels': labels, 'num_classes': ncls, 'num_examples': 10000})
    first = None
    for i in range(120):
        step()
        if i == 4:
            first = float(losses[0])
    last = float(losses[0])
    assert np.isfinite(last) and last < 0.5 * first, (first, last)

    def embed(y):
        e = net.forward(_samples(templates, y, rng), is_training=False)
        return e / e.norm(dim=1, keepdim=True)
    ya = np.repeat(np.arange(ncls), 20)
    cent = torch.stack([embed(ya)[torch.tensor(ya, device='cuda') == c].mean(0) for c in range(ncls)])
    cent = cent / cent.norm(dim=1, keepdim=True)
    yt = rng.integers(0, ncls, 200)
    acc = float(((embed(yt) @ cent.t()).argmax(1).cpu().numpy() == yt).mean())
    print('%s: loss %.3f -> %.3f, nearest-centroid accuracy %.3f' % (name, first, last, acc))
    assert acc >= 0.95, acc


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_train_synthetic_save_evaluate(tmp_path):
    from PIL import Image
    from scipy.io import loadmat
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        path = str(tmp_path / ('im%d.png' % i))
        Image.fromarray(rng.integers(0, 255, (32, 32, 3), dtype=np.uint8)).save(path)
        lines.append('%s %d' % (path, i % 3))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--synthetic', '1',
                '--synthetic_classes', '10', '--input_height', '32', '--input_width', '32', '--batch_size', '8', '--num_gpus', '1',
                '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
                '--save_interval', '1000', '--max_steps', '3', '--margin', '0.3'], str(tmp_path))
    assert 'Loss #0: cross_entropy' in out and 'Model has been saved in Iteration 2' in out
    out = _run([os.path.join(ROOT, 'evaluate.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--fea_name', 'f',
                '--data_list_path', str(tmp_path / 'list.txt'), '--input_height', '32', '--input_width', '32', '--batch_size', '4'],
               str(tmp_path))
    assert 'Totally extracted 6 features.' in out
    m = loadmat(str(tmp_path / 'features' / 'SphereNet-ArcFace_m' / 'f_3.mat'))
    assert m['wfea'].shape == (6, 512) and np.isfinite(m['wfea']).all() and np.abs(m['wfea']).max() > 0
