"""-m gpu: the sampled-class (Partial FC) margin head, include/fte.h "Partial FC" -- the sampler against the integer restatement
(tests/partial_fc_ref.py) exactly, gather / scatter against numpy indexing exactly, the public loss function and SphereNet-ArcFace
with a sample rate against the float64 restatement, the dense path at rate 1 bit for bit, the million-class case, the refusals and
the command line.

Exclusions: tests/test_gpu_margin.py drops from its comparisons only the rows whose float64 reference loss is not finite (none of
its cases has one; the margin head has no kink band of its own); the same rule is applied here, decided from the reference alone,
and the count (0) is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as mr
import partial_fc_ref as pr
from oracle import spherenet as osn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    import test_gpu_margin as tgm
    from util_gpu import dev, host, check_maxabs, check_rell2, kink_of, call, stream
    from tf_face_toolbox_amd import net_select, Singular, DataParallel, DataParallel_margin, _lib
    from tf_face_toolbox_amd.loss import additive_margin_loss, partial_fc_margin_loss, sample_size

ARC, COS = (64.0, 0.5, 0.0), (64.0, 0.0, 0.35)
D = 512


def _i32(n, fill=None):
    t = torch.empty(n, dtype=torch.int32, device='cuda')
    if fill is not None:
        t.fill_(fill)
    return t


def _sample(y, C, S, seed, step):
    n = len(y)
    spad = (S + 63) // 64 * 64
    index, inverse, ys = _i32(spad, 12345), _i32(C, 12345), _i32(n, 12345)
    nb = _lib.query('fte_pfc_sample_ws_bytes', C)
    ws = torch.full((nb // 4 + 16,), float('nan'), device='cuda')              # the call clears what it uses
    call('fte_pfc_sample', dev(y, torch.int32), n, C, S, seed, step, index, inverse, ys, ws, ws.numel() * 4, stream())
    torch.cuda.synchronize()
    return index.cpu().numpy(), inverse.cpu().numpy(), ys.cpu().numpy()


def _check_sample(y, C, S, seed, step):
    got = _sample(y, C, S, seed, step)
    index, inverse, ys = pr.sample(y, C, S, seed, step)
    assert np.array_equal(got[0][:S], index), (C, S, len(y))
    assert (got[0][S:] == -1).all()
    assert np.array_equal(got[1], inverse) and np.array_equal(got[2], ys)
    again = _sample(y, C, S, seed, step)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    return got


@pytest.mark.parametrize('C', [1000, 10575, 85742, 1000000])
@pytest.mark.parametrize('r', [0.05, 0.1, 0.5])
@pytest.mark.parametrize('n', [1, 64, 512])
def test_sampler_equals_the_restatement_exactly(n, r, C):
    rng = np.random.default_rng(n + C)
    y = rng.integers(0, C, n)
    y[0], y[-1] = 0, C - 1
    S = pr.sample_size(C, r)
    if S < n:                                                  # refused: a batch's classes must always fit
        idx, inv, ys = _i32(64), _i32(C), _i32(n)
        ws = torch.empty(_lib.query('fte_pfc_sample_ws_bytes', C) // 4 + 16, device='cuda')
        with pytest.raises(_lib.FteError):
            call('fte_pfc_sample', dev(y, torch.int32), n, C, S, 1, 0, idx, inv, ys, ws, ws.numel() * 4, stream())
        return
    _check_sample(y, C, S, seed=3, step=n)
    _check_sample(y, C, S, seed=0xfffffff1, step=0xffffffff)   # uint32 wrap-around of seed, step and j + base


def test_sampler_edge_batches():
    C = 85742
    _check_sample(np.full(512, 4711), C, pr.sample_size(C, 0.1), 5, 2)         # one class in the whole batch
    y = np.random.default_rng(0).permutation(C)[:512]
    got = _check_sample(y, C, 512, 5, 2)                                        # n distinct classes and S = n: the batch alone
    assert np.array_equal(got[0], np.sort(y))
    y = np.random.default_rng(1).integers(0, 1000, 64)
    y[3], y[9] = -1, 1000                                                       # outside [0, C): no part in the sample, label -1
    got = _check_sample(y, 1000, 100, 5, 2)
    assert got[2][3] == -1 and got[2][9] == -1
    _check_sample(y, 1000, 1000, 5, 2)                                          # S = C
    steps = [_sample(y, 1000, 100, 5, t)[0] for t in range(3)]
    assert not np.array_equal(steps[0], steps[1]) and not np.array_equal(steps[1], steps[2])


@pytest.mark.parametrize('C,S,d', [(1000, 100, 512), (10575, 529, 64), (85742, 8575, 512), (1000, 1000, 48), (333, 65, 7)])
def test_gather_and_scatter_equal_numpy_indexing(C, S, d):
    rng = np.random.default_rng(C + S)
    cpad, spad = (C + 127) // 128 * 128, (S + 63) // 64 * 64
    y = rng.integers(0, C, min(S, 64))
    index, inverse, _ = pr.sample(y, C, S, 9, 1)
    W = rng.standard_normal((d, cpad)).astype(np.float32)
    idx = np.full(spad, -1, np.int32)
    idx[:S] = index
    Ws = torch.full((d, spad), float('nan'), device='cuda')
    call('fte_pfc_gather_cols', dev(W), dev(idx, torch.int32), Ws, d, C, cpad, S, spad, stream())
    want = np.zeros((d, spad), np.float32)
    want[:, :S] = W[:, index]
    assert np.array_equal(Ws.cpu().numpy(), want)
    dWs = rng.standard_normal((d, spad)).astype(np.float32)
    for before in (0.0, float('nan')):
        dW = torch.full((d, cpad), before, device='cuda')
        call('fte_pfc_scatter_cols', dev(dWs), dev(inverse, torch.int32), dW, d, C, cpad, S, spad, stream())
        want = np.zeros((d, cpad), np.float32)
        want[:, index] = dWs[:, :S]
        got = dW.cpu().numpy()
        assert np.array_equal(got, want)
        unsampled = np.setdiff1d(np.arange(cpad), index)
        assert (got[:, unsampled].view(np.uint32) == 0).all()                   # +0.0 bit for bit


def test_invalid_arguments():
    C, S, n = 1000, 100, 8
    idx, inv, ys, y = _i32(128), _i32(C), _i32(n), _i32(n, 1)
    ws = torch.empty(_lib.query('fte_pfc_sample_ws_bytes', C) // 4 + 16, device='cuda')
    wsb = ws.numel() * 4
    for args in ((0, C, S, wsb), (n, 0, S, wsb), (n, C, n - 1, wsb), (n, C, C + 1, wsb), (n, C, S, 64)):
        with pytest.raises(_lib.FteError):
            call('fte_pfc_sample', y, args[0], args[1], args[2], 0, 0, idx, inv, ys, ws, args[3], stream())
    with pytest.raises(_lib.FteError):
        call('fte_pfc_sample', y, n, C, S, 0, 0, idx, None, ys, ws, wsb, stream())
    W, Ws = torch.zeros(64, 1024, device='cuda'), torch.zeros(64, 128, device='cuda')
    for args in ((0, C, 1024, S, 128), (64, C, 999, S, 128), (64, C, 1024, S, 64), (64, 0, 1024, S, 128), (64, C, 1024, 0, 128)):
        with pytest.raises(_lib.FteError):
            call('fte_pfc_gather_cols', W, idx, Ws, *args, stream())
        with pytest.raises(_lib.FteError):
            call('fte_pfc_scatter_cols', Ws, inv, W, *args, stream())
    with pytest.raises(_lib.FteError):
        call('fte_pfc_gather_cols', W, idx, Ws, 64, C, 1024, S, 126, stream())      # Spad % 4


# ------------------------------------------------------------------------------------------------ the public loss function
def _head_case(seed, n, c, ld):
    rng = np.random.default_rng(seed)
    W = np.zeros((D, ld), np.float32)
    W[:, :c] = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    return tgm._features(rng, W, y, n), W, y


@pytest.mark.parametrize('preset', [ARC, COS])
@pytest.mark.parametrize('n,c,ld,rate', [(64, 1000, 1024, 0.25), (512, 10575, 10624, 0.1)])
def test_public_loss_function(preset, n, c, ld, rate):
    x, W, y = _head_case(17, n, c, ld)
    S = sample_size(c, rate)
    loss, dx, dW, index = partial_fc_margin_loss(dev(x), dev(W), dev(y, torch.int32), rate, 5, 3, *preset, num_classes=c)
    torch.cuda.synchronize()
    lr, _, dxr, dWr, ir = pr.head_fwd_bwd(x.astype(np.float64), W[:, :c].astype(np.float64), y, S, 5, 3, *preset)
    rows = mr.kernel_ref((x.astype(np.float64) @ W[:, ir].astype(np.float64)), np.linalg.norm(x.astype(np.float64), axis=1),
                         np.linalg.norm(W[:, ir].astype(np.float64), axis=0), pr.sample(y, c, S, 5, 3)[2], *preset, 1.0 / n)[1]
    assert int((~np.isfinite(rows)).sum()) == 0                # rows the reference excludes: none, as in test_gpu_margin.py
    assert np.array_equal(index.cpu().numpy(), ir)
    print('loss %.8f ref %.8f' % (float(loss), lr))
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    check_rell2(host(dx), dxr, what='dfeatures')
    check_rell2(host(dW)[:, :c], dWr, what='dweights')
    unsampled = np.setdiff1d(np.arange(ld), ir)
    assert (dW.cpu().numpy()[:, unsampled].view(np.uint32) == 0).all()


def test_sample_smaller_than_the_batch_is_refused():
    x, W, y = _head_case(1, 64, 1000, 1024)
    with pytest.raises(ValueError, match='smaller than the batch'):
        partial_fc_margin_loss(dev(x), dev(W), dev(y, torch.int32), 0.05, 0, 0, num_classes=1000)
    with pytest.raises(ValueError):
        partial_fc_margin_loss(dev(x), dev(W), dev(y, torch.int32), 0.0, 0, 0, num_classes=1000)


@pytest.mark.parametrize('rate', [1, 1.0, None])
def test_rate_one_is_the_dense_function_bit_for_bit(rate):
    x, W, y = _head_case(19, 64, 1000, 1024)
    a = additive_margin_loss(dev(x), dev(W), dev(y, torch.int32), *ARC, num_classes=1000)
    b = partial_fc_margin_loss(dev(x), dev(W), dev(y, torch.int32), rate, 5, 3, *ARC, num_classes=1000)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b[:3]))
    assert np.array_equal(b[3].cpu().numpy(), np.arange(1000))


# ------------------------------------------------------------------------------------------------ SphereNet
def _setup(name, n, h, w, ch, ncls, seed=21, rate=None, sample_seed=0):
    net, p, x, y = tgm._setup(name, n, h, w, ch, ncls, seed)
    if rate is not None:
        net.set_sample_rate(rate, sample_seed)
    return net, p, x, y


def test_net_rate_one_is_the_dense_net_bit_for_bit():
    n, ncls = 4, 10
    arenas = []
    for rate in (None, 1.0):
        net, p, x, y = _setup('SphereNet-ArcFace', n, 32, 32, 3, ncls, seed=31, rate=rate)
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
        step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
        seen = []
        for t in range(3):
            step()
            seen.append((float(losses[0]), net.grads.clone()))
        torch.cuda.synchronize()
        arenas.append((seen, net.params.clone()))
    for (la, ga), (lb, gb) in zip(arenas[0][0], arenas[1][0]):
        assert la == lb and torch.equal(ga, gb)
    assert torch.equal(arenas[0][1], arenas[1][1])


@pytest.mark.parametrize('name', ['SphereNet-ArcFace', 'SphereNet-CosFace'])
def test_spherenet_sampled_forward_loss_and_every_gradient(name):
    n, h, w, ch, ncls, rate, seed = 4, 32, 32, 3, 1000, 0.25, 11
    net, p, x, y = _setup(name, n, h, w, ch, ncls, rate=rate, sample_seed=seed)
    S = sample_size(ncls, rate)
    xd, yd = dev(x), dev(y, torch.int32)
    net.tower_scale = 1.0
    net.global_step = 6
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    losses, names, others = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    losses_ref, g_ref, ex = pr.loss_and_grads(p, x, y, S, seed, 6, *tgm._preset(net), 5e-4, 'NCHW', kink=kink_of(net))
    assert names == ['cross_entropy', 'reg_loss'] and not others
    assert net.sample_size == S == 250 and logits['logits'].shape == (n, S) and net.s_raw.shape == (n, 256)
    assert np.array_equal(logits['class_index'].cpu().numpy(), ex['index'])
    check_maxabs(host(net.emb), ex['embedding'], what='embedding')
    check_maxabs(host(logits['logits']), ex['logits'], what='logits')
    assert abs(float(losses[0]) - losses_ref[0]) <= 1e-5 * max(1, abs(losses_ref[0])), (float(losses[0]), losses_ref[0])
    assert abs(float(losses[1]) - losses_ref[1]) <= 1e-5 * max(1, abs(losses_ref[1]))
    for k in p:
        data_grad = g_ref[k] - (5e-4 * p[k] if k.endswith('/weights') else 0)
        check_rell2(host(net.get_variable(k, net.grads)), data_grad, what='grad ' + k)
    gw = net.get_variable('classifier/fc_classifier/weights', net.grads).cpu().numpy()
    unsampled = np.setdiff1d(np.arange(ncls), ex['index'])
    assert (gw[:, unsampled].view(np.uint32) == 0).all()
    assert net.forward(xd, is_training=False).shape == (n, 512)                 # features only, as before


def test_three_sampled_training_steps_match_the_restatement():
    n, h, w, ch, ncls, rate, seed = 4, 32, 32, 3, 1000, 0.25, 13
    net, p, x, y = _setup('SphereNet-ArcFace', n, h, w, ch, ncls, seed=31, rate=rate, sample_seed=seed)
    S = sample_size(ncls, rate)
    inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
    step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
    slots = osn.zero_slots(p)
    samples = []
    for t in range(3):
        step()
        samples.append(net.class_index[:S].cpu().numpy().copy())
        p, slots, l_ref = pr.train_step(p, slots, x, y, 0.05, S, seed, t, *tgm._preset(net), kink=kink_of(net))
        assert abs(float(losses[0]) - l_ref[0]) <= 1e-5 * max(1, abs(l_ref[0])), (t, float(losses[0]), l_ref)
    for k in p:
        check_maxabs(host(net.get_variable(k)), p[k], 2e-5, what='weights after 3 steps ' + k)
    assert not np.array_equal(samples[0], samples[1]) and not np.array_equal(samples[1], samples[2])
    assert all(np.isin(y, s).all() for s in samples)


def test_two_identical_sampled_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        net, p, x, y = _setup('SphereNet-ArcFace', 16, 112, 112, 3, 1000, seed=41, rate=0.25, sample_seed=2)
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': 1000, 'num_examples': 16}
        step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
        for t in range(2):
            step()
        torch.cuda.synchronize()
        runs.append((net.params.clone(), net.grads.clone(), net.class_index.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and float(runs[0][1].abs().max()) > 0


def test_bf16_mode_head_parity():
    """test_gpu_margin.py's test_precision_modes_head_parity on the sampled buffers: the head runs in fp32 on the GPU's own s / xn / wn"""
    _lib.set_mfma_dtype('bf16')
    try:
        n, ncls, rate = 8, 1000, 0.25
        net, p, x, y = _setup('SphereNet-ArcFace', n, 112, 112, 3, ncls, seed=43, rate=rate, sample_seed=1)
        S = sample_size(ncls, rate)
        xd, yd = dev(x), dev(y, torch.int32)
        logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
        net.loss_function('TOWER', yd, **logits)
        net.backward()
        torch.cuda.synchronize()
        got = (net.logits_buf, net.loss_rows, net.G, net.rowcoef)
        assert np.array_equal(net.sampled_labels.cpu().numpy(), pr.sample(y, ncls, S, 1, 0)[2])
        _, Gr = tgm._check_head(got, net.s_raw, net.xn, net.wn, net.sampled_labels, S, *tgm._preset(net), 1.0 / n, 'bf16')
        check_maxabs(host(net.colcoef)[:S], mr.colcoef_ref(Gr, host(net.s_raw), host(net.wn), S)[:S], 1e-4, what='colcoef')
        assert torch.isfinite(net.grads).all()
    finally:
        _lib.set_mfma_dtype('f32')


# ------------------------------------------------------------------------------------------------ scale
def test_million_classes():
    n, c, rate = 512, 1000000, 0.1
    ld = (c + 127) // 128 * 128
    S = sample_size(c, rate)
    g = torch.Generator(device='cuda').manual_seed(3)
    W = torch.randn(D, ld, generator=g, device='cuda')
    W[:, c:] = 0
    rng = np.random.default_rng(5)
    y = rng.integers(0, c, n)
    x = (rng.standard_normal((n, D)) * rng.uniform(0.5, 20.0, (n, 1))).astype(np.float32)
    xd, yd = dev(x), dev(y, torch.int32)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, dx, dW, index = partial_fc_margin_loss(xd, W, yd, rate, 7, 1, *ARC, num_classes=c)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    dense_three = 3 * n * ld * 4
    print('peak of the sampled call %.2f GB, the dense head\'s three [n, cpad] tensors alone %.2f GB' % (peak / 1e9, dense_three / 1e9))
    assert peak < dense_three, (peak, dense_three)
    ir, _, ys = pr.sample(y, c, S, 7, 1)
    assert np.array_equal(index.cpu().numpy(), ir)
    Wg = W[:, torch.as_tensor(ir, device='cuda')].cpu().numpy().astype(np.float64)
    lr = mr.loss_only(x.astype(np.float64), Wg, ys, *ARC)
    print('loss %.8f ref %.8f' % (float(loss), lr))
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    assert torch.isfinite(dx).all()
    nz = (dW != 0).any(0)
    assert int(nz.sum()) <= S and not bool(nz[torch.as_tensor(np.setdiff1d(np.arange(ld), ir)[:100000], device='cuda')].any())


# ------------------------------------------------------------------------------------------------ refusals, CLI
def test_refusals():
    net = net_select('SphereNet-ArcFace', 'NCHW', 5e-4)
    net.set_sample_rate(0.1, 0)
    for wrapper in (DataParallel, DataParallel_margin):
        with pytest.raises(ValueError, match='one GPU only'):
            wrapper(net, 0.1, 'Momentum', num_gpus=2)
    DataParallel_margin(net_select('SphereNet-ArcFace', 'NCHW', 5e-4), 0.1, 'Momentum', num_gpus=2)      # the dense head: accepted
    for name in ('ResNet-50-arcface', 'ResNet-50-cosface', 'SphereNet-ASoftmax', 'SphereNet'):
        with pytest.raises(ValueError, match='sampled-class head'):
            net_select(name, 'NCHW', 5e-4).set_sample_rate(0.1, 0)
    # S < n is refused when the head is built
    net, p, x, y = _setup('SphereNet-ArcFace', 64, 32, 32, 3, 1000, rate=0.05)
    with pytest.raises(ValueError, match='smaller than the batch'):
        Singular(net, 0.1, 'Momentum')({'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': 1000, 'num_examples': 64})


def test_train_sampled_save_evaluate(tmp_path):
    from PIL import Image
    from scipy.io import loadmat
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        path = str(tmp_path / ('im%d.png' % i))
        Image.fromarray(rng.integers(0, 255, (32, 32, 3), dtype=np.uint8)).save(path)
        lines.append('%s %d' % (path, i % 3))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    out = tgm._run([os.path.join(ROOT, 'train.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--synthetic', '1',
                    '--synthetic_classes', '1000', '--input_height', '32', '--input_width', '32', '--batch_size', '8', '--num_gpus', '1',
                    '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
                    '--save_interval', '1000', '--max_steps', '3', '--margin', '0.3', '--sample_rate', '0.1', '--sample_seed', '4'],
                   str(tmp_path))
    assert 'Sampled-class head: sample_rate = 0.1, sample_seed = 4, S = 100 of 1000 classes per step' in out
    assert 'Loss #0: cross_entropy' in out and 'Model has been saved in Iteration 2' in out
    out = tgm._run([os.path.join(ROOT, 'evaluate.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--fea_name', 'f',
                    '--data_list_path', str(tmp_path / 'list.txt'), '--input_height', '32', '--input_width', '32', '--batch_size', '4'],
                   str(tmp_path))
    assert 'Totally extracted 6 features.' in out
    m = loadmat(str(tmp_path / 'features' / 'SphereNet-ArcFace_m' / 'f_3.mat'))
    assert m['wfea'].shape == (6, 512) and np.isfinite(m['wfea']).all() and np.abs(m['wfea']).max() > 0
