"""-m gpu: IResNet on the graph engine against the float64 restatement (tests/iresnet_ref.py), by the procedure and tolerances of
test_gpu_resnet.py: every tensor is held to max(base, 2 x the restatement's own float32-vs-float64 error on this input); inside the
kink band of a PReLU -- max(1e-5 rms(u), 16 x the restatement's own fp32 noise on u), computed from the reference alone -- the side the
engine took is adopted, as for the ReLU nets.  The net under test has one block per stage on 6 images of 32 x 24 x 3: the final map is
2 x 2, so a wrong flatten order fails; 7 classes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import iresnet_ref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from util_gpu import dev, host, check_rell2
    from tf_face_toolbox_amd import _lib, net_select, Singular
    from tf_face_toolbox_amd.nets.iresnet import IResNet

BLOCKS, N, H, W, NCLS = [1, 1, 1, 1], 6, 32, 24, 7
WD, LR = 5e-4, 0.05
_CASE = {}


def _case():
    """graph, parameters, moving statistics, images, labels: made once, never modified"""
    if not _CASE:
        g, spec, _ = ir.iresnet_graph(18, 3, NCLS, H, W, BLOCKS)
        p, state = ir.init_params(spec, 71)
        p = ir.perturb(p, 72)
        rng = np.random.default_rng(73)
        _CASE.update(g=g, spec=spec, p=p, state=state, x=rng.uniform(-1, 1, (N, H, W, 3)), y=rng.integers(0, NCLS, N))
    c = _CASE
    return c['g'], c['spec'], c['p'], c['state'], c['x'], c['y']


def _net(head, p, fmt='NCHW'):
    net = IResNet(18, weight_decay=WD, data_format=fmt, head=head, blocks=BLOCKS)
    net.build(H, W, 3, NCLS, 'cuda')
    net.load_params(p)
    return net


def _kink(net):
    """prelu output -> u = scale * z + shift with the engine's z, scale, shift: products of fp32 values are exact in float64 and the
    sum keeps the sign, so this is the sign fma(z, scale, shift) had on the device"""
    return {op[1]: host(net.t[op[2]]) * host(net.bn[op[1]]['scale']) + host(net.bn[op[1]]['shift']) for op in net.plan if op[0] == 'bnprelu'}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-30))


def _f32(d):
    return {k: v.astype(np.float32) for k, v in d.items()}


def _audit(net, head, p, state, x, y, fmt='NCHW'):
    """one training-mode pass of `net` (forward, loss, backward done by the caller) against the restatement"""
    g = _case()[0]
    kink = _kink(net)
    bands = ir.noise_bands(g, p, x, state, fmt)
    kw = dict(head=head, weight_decay=WD, kink=kink, bands=bands, data_format=fmt)
    l_ref, g_ref, env, new_state = ir.loss_and_grads(g, p, x, y, state=state, **kw)
    _, g32, env32, _ = ir.loss_and_grads(g, _f32(p), x.astype(np.float32), y, state=_f32(state), **kw)
    names = ['stem', 's1b0', 's2b0/c1', 's3b0/sc/bn', 's4b0', 'out/bn', 'embed', 'features'] + (['logits'] if head == 'softmax' else [])
    for name in names:
        got = host(net.t[name])
        if name == 'logits':
            got = got[:, :NCLS]
        r, r32 = _rel(got, env[name]), _rel(env32[name], env[name])
        print('%-12s rel %.2e (float32 restatement %.2e)' % (name, r, r32))
        assert r <= max(2e-5, 2 * r32), name
    return l_ref, g_ref, g32, new_state


def _check_grads(net, p, g_ref, g32):
    for k in p:
        got = host(net.get_variable(k, net.grads)) + (WD * p[k] if k.endswith('weights') else 0)      # + wd * w (folded into the optimizer)
        r, r32 = _rel(got, g_ref[k]), _rel(g32[k], g_ref[k])
        print('grad %-60s rel %.2e (float32 restatement %.2e)' % (k, r, r32))
        assert float(np.abs(got).max()) > 0, k
        assert r <= max(1e-4, 2 * r32), ('grad ' + k, r, r32)


@pytest.mark.parametrize('head,fmt,fuse', [('softmax', 'NCHW', '1'), ('arcface', 'NHWC', '1'), ('softmax', 'NCHW', '0')],
                         ids=['softmax', 'arcface_nhwc', 'softmax_stats_stand_alone'])
def test_training_forward_loss_every_gradient_moving_statistics(head, fmt, fuse, monkeypatch):
    """fuse = '0': FTE_BN_FUSE=0, the statistics of every BN from the stand-alone pass instead of the producing conv's epilogue.  The
    existing nets claim no bit identity between the two (the partial sums are merged in another order), so both are held to the same
    audit."""
    g, spec, p, state, x, y = _case()
    monkeypatch.setenv('FTE_BN_FUSE', fuse)
    net = _net(head, p, fmt)
    n_prelu = sum(1 for op in net.plan if op[0] == 'bnprelu')
    assert net.graph == g and sorted(net.variables) == sorted(p) and n_prelu == 5
    fused_prelu = [j for j in net.fuse_fwd.values() if net.plan[j][0] == 'bnprelu']
    assert len(fused_prelu) == (5 if fuse == '1' else 0)          # planned for every BN + PReLU behind a conv (the stem's direct conv declines when it runs)
    xd, yd = dev(x), dev(y, torch.int32)
    out = net.forward(xd, num_classes=NCLS, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **out)
    net.backward()
    torch.cuda.synchronize()
    assert names == ['cross_entropy', 'reg_loss']
    l_ref, g_ref, g32, new_state = _audit(net, head, p, state, x, y, fmt)
    assert abs(float(losses[0]) - l_ref[0]) <= 1e-4 * max(1, l_ref[0]) and abs(float(losses[1]) - l_ref[1]) <= 1e-5 * max(1, l_ref[1]), (losses, l_ref)
    _check_grads(net, p, g_ref, g32)
    for k in new_state:                                          # moving statistics: decay 0.9, unbiased variance
        got = host(net.get_variable(k))
        assert np.abs(got - new_state[k]).max() <= 3e-5 * np.abs(new_state[k]).max() + 1e-9, k


@pytest.mark.parametrize('head', ['softmax', 'arcface'])
def test_three_momentum_steps(head):
    """three Momentum steps through Singular on one batch; the restatement takes the same steps, resolving each step's kinks with
    that step's pre-activations.  Every variable's total update is held to max(1e-4, 2 x the float32 restatement's error) of itself."""
    g, spec, p, state, x, y = _case()
    net = _net(head, p)
    step, losses, names, _ = Singular(net, LR, 'Momentum', weight_decay=WD)(
        {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': NCLS, 'num_examples': N})
    for k in state:                                               # the construction-time pass moved nothing
        assert np.array_equal(host(net.get_variable(k)), state[k]), k
    from oracle import ops
    refs = {}
    for dt in (np.float64, np.float32):
        refs[dt] = dict(p={k: v.astype(dt) for k, v in p.items()}, s={k: v.astype(dt) for k, v in state.items()},
                        slots={k: np.zeros_like(v, dtype=dt) for k, v in p.items()})
    for i in range(3):
        step()
        torch.cuda.synchronize()
        kink = _kink(net)
        bands = ir.noise_bands(g, refs[np.float64]['p'], x, refs[np.float64]['s'])
        for dt, r in refs.items():
            ls, gr, _, r['s'] = ir.loss_and_grads(g, r['p'], x.astype(dt), y, head=head, weight_decay=WD, state=r['s'], kink=kink, bands=bands)
            if dt is np.float64:
                assert abs(float(losses[0]) - ls[0]) <= 1e-4 * max(1, ls[0]), (i, float(losses[0]), ls)
            newp = {}
            for k in r['p']:
                newp[k], r['slots'][k] = ops.momentum_step(r['p'][k], r['slots'][k], gr[k], dt(LR))
            r['p'] = newp
    for k in p:
        d_ref = refs[np.float64]['p'][k] - p[k]
        d_32 = refs[np.float32]['p'][k].astype(np.float64) - p[k]
        d_got = host(net.get_variable(k)) - p[k]
        assert _rel(d_got, d_ref) <= max(1e-4, 2 * _rel(d_32, d_ref)), (k, _rel(d_got, d_ref), _rel(d_32, d_ref))
    for k in state:
        ref = refs[np.float64]['s'][k]
        assert np.abs(host(net.get_variable(k)) - ref).max() <= 3e-5 * np.abs(ref).max() + 1e-9, k


@pytest.mark.parametrize('fmt', ['NCHW', 'NHWC'])
def test_inference_mode(fmt):
    """eval_features (moving statistics, fte_bn_prelu_infer_fwd) against the restatement's inference mode"""
    g, spec, p, state, x, y = _case()
    rng = np.random.default_rng(9)
    st = {k: (v + 0.2 * rng.random(v.shape)) for k, v in state.items()}
    net = _net('arcface', p, fmt)
    for k, v in st.items():
        net.set_variable(k, torch.tensor(v, dtype=torch.float32))
    feat = host(net.eval_features(dev(x)))
    env, _, _ = ir.forward(g, p, x, False, st, fmt)
    env32, _, _ = ir.forward(g, _f32(p), x.astype(np.float32), False, _f32(st), fmt)
    assert feat.shape == (N, 512)
    assert _rel(feat, env['features']) <= max(2e-5, 2 * _rel(env32['features'], env['features']))
    for k, v in st.items():                                       # inference moves no statistics
        assert np.array_equal(host(net.get_variable(k)), v.astype(np.float32).astype(np.float64)), k


def test_bf16_operand_mode():
    """the rules of test_gpu_bf16.py for a whole step in the bf16-operand mode: against the UNROUNDED restatement, rel-L2 1e-2 on
    features / logits, 1e-2 on the loss, 3e-2 on every gradient; the kink band is 4 x the restatement's own bf16 noise; and the step
    is measurably not the fp32 one"""
    g, spec, p, state, x, y = _case()
    _lib.set_mfma_dtype('bf16')
    try:
        net = _net('softmax', p)
        out = net.forward(dev(x), num_classes=NCLS, is_training=True)
        losses, _, _ = net.loss_function('TOWER', dev(y, torch.int32), **out)
        net.backward()
        torch.cuda.synchronize()
        assert not net._act_s16
        bands = ir.noise_bands16(g, p, x, state)
        l_ref, g_ref, env, _ = ir.loss_and_grads(g, p, x, y, weight_decay=WD, state=state, kink=_kink(net), bands=bands, kink_mode='bf16')
        check_rell2(host(net.t['features']), env['features'], 1e-2, 'features (bf16 operands)')
        check_rell2(host(net.t['logits'])[:, :NCLS], env['logits'], 1e-2, 'logits (bf16 operands)')
        assert abs(float(losses[0]) - l_ref[0]) <= 1e-2 * l_ref[0]
        worst, zero = 0.0, []
        bn_out = {op[3]: op[1] for op in g if op[0] == 'bn'}
        for k in p:
            got = host(net.get_variable(k, net.grads)) + (WD * p[k] if k.endswith('weights') else 0)
            if k.endswith('/beta'):
                # dbeta = sum of g over the rows.  Where every consumer of the BN's output normalises per channel again (the block's
                # last BN and its shortcut's BN, whose sum feeds the next block's leading BN and 1x1 shortcut -> BN), a shift of beta
                # changes nothing: the sum cancels to 0 (1e-17 in float64) and a RELATIVE error has no meaning.  The rule's 3e-2 on
                # the terms then bounds the sum: terms with independent errors of 3e-2 |g_i| add up to 3e-2 * sqrt(sum g_i^2)
                gt = env['tensor_grads'][bn_out[k[:-len('/beta')]]]
                gnorm = float(np.sqrt((gt * gt).sum()))
                if np.sqrt((g_ref[k] ** 2).sum()) <= 1e-9 * gnorm:
                    zero.append(k)
                    assert np.sqrt((got * got).sum()) <= 3e-2 * gnorm, (k, float(np.sqrt((got * got).sum())), gnorm)
                    continue
            worst = max(worst, check_rell2(got, g_ref[k], 3e-2, 'grad ' + k))
        assert worst > 1e-5
        assert set(zero) == set(['IResNet-18/stage%d/block_0/%s/BatchNorm/beta' % (s, c) for s in (1, 2, 3, 4) for c in ('conv2_3x3', 'conv_shortcut_1x1')]
                                + ['IResNet-18/output/BatchNorm/beta']), zero          # (the output BN's shift reaches the last BN as a per-feature constant)
    finally:
        _lib.set_mfma_dtype('f32')


def test_real_topology_one_step_and_determinism():
    """IResNet-18-arcface as the factory builds it, 4 images of 112 x 96: names and shapes from the block table, one Momentum step with
    everything finite and every gradient non-zero, and a second net taking the same step ends with the same bytes"""
    n, h, w, ncls = 4, 112, 96, 10
    rng = np.random.default_rng(4)
    x, y = dev(rng.uniform(-1, 1, (n, h, w, 3))), dev(rng.integers(0, ncls, n), torch.int32)
    arenas = []
    for _ in range(2):
        net = net_select('IResNet-18-arcface', 'NCHW', WD)
        step, losses, names, _ = Singular(net, 0.01, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
        w0 = net.params.clone()
        step()
        torch.cuda.synchronize()
        tv, st = ir.expected_variables(18, 3, ncls, h, w)
        assert sorted(net.variables) == sorted(k for k, _ in tv)
        for k, shape in tv:
            assert tuple(net.get_variable(k).shape) == shape, k
            gk = net.get_variable(k, net.grads)
            assert torch.isfinite(gk).all(), k
            # (the betas of a block's last BN, of its shortcut's BN and of the output BN feed nothing but another per-channel
            # normalisation: their gradient is 0 by construction and what the engine holds there is rounding noise)
            if not k.endswith(('conv2_3x3/BatchNorm/beta', 'conv_shortcut_1x1/BatchNorm/beta', 'output/BatchNorm/beta')):
                assert float(gk.abs().max()) > 0, k
        for k, shape in st:
            assert tuple(net.get_variable(k).shape) == shape and torch.isfinite(net.get_variable(k)).all(), k
        assert names == ['cross_entropy', 'reg_loss'] and all(np.isfinite(float(v)) for v in losses)
        assert torch.isfinite(net.params).all() and not torch.equal(net.params, w0)
        assert net.t['out/bn'].shape == (n, 7, 6, 512) and net.t['features'].shape == (n, 512)
        arenas.append((net.params.clone(), net.grads.clone(), [net.state[k].clone() for k in sorted(net.state)]))
    a, b = arenas
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(a[2], b[2]))


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_cli_train_checkpoint_evaluate(tmp_path):
    """train.py --net_name IResNet-18-arcface for two steps on a JPEG list, checkpoint, then evaluate.py restores it: the features it
    writes are eval_features of a net holding the checkpoint's variables and moving statistics"""
    from PIL import Image
    from scipy.io import loadmat
    rng = np.random.default_rng(3)
    lines, imgs = [], []
    for c in range(4):
        for i in range(3):
            path = str(tmp_path / ('id%d_%d.jpg' % (c, i)))
            Image.fromarray(rng.integers(0, 255, (32, 24, 3), dtype=np.uint8)).save(path, quality=95)
            lines.append('%s %d' % (path, c))
            imgs.append(np.asarray(Image.open(path).convert('RGB')))
    (tmp_path / 'train.txt').write_text('\n'.join(lines) + '\n')
    name, tag = 'IResNet-18-arcface', 'IResNet-18-arcface_g'
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', name, '--model_name', 'g', '--train_list_path', str(tmp_path / 'train.txt'),
                '--input_height', '32', '--input_width', '24', '--num_gpus', '1', '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50',
                '--display_interval', '1', '--save_interval', '1000', '--max_steps', '2', '--batch_size', '8'], str(tmp_path))
    assert 'Model has been saved in Iteration 1' in out
    out = _run([os.path.join(ROOT, 'evaluate.py'), '--net_name', name, '--model_name', 'g', '--fea_name', 'f', '--data_list_path', str(tmp_path / 'train.txt'),
                '--input_height', '32', '--input_width', '24', '--batch_size', '8'], str(tmp_path))
    assert 'Totally extracted 12 features.' in out
    wfea = loadmat(str(tmp_path / 'features' / tag / 'f_2.mat'))['wfea']
    assert wfea.shape == (12, 512) and np.isfinite(wfea).all()
    ck = torch.load(str(tmp_path / 'models' / tag / (tag + '.ckpt-2')), map_location='cpu')
    v = ck['variables']
    tv, st = ir.expected_variables(18, 3, 4, 32, 24)
    assert set(k for k, _ in tv + st) <= set(v)
    assert any(float(v[k].abs().max()) > 0 for k, _ in st if k.endswith('moving_mean'))          # two training steps moved the statistics
    net = net_select(name, 'NCHW', WD)
    net.build(32, 24, 3, 4, 'cuda')
    for k, _ in tv + st:
        net.set_variable(k, v[k])
    x = (np.stack(imgs).astype(np.float64) / 255.0 - 0.5) / 0.5
    ref = np.concatenate([host(net.eval_features(dev(x[i:i + 8]))) for i in (0, 8)])
    err = np.abs(wfea - ref).max()
    assert err <= 2e-5 * np.abs(ref).max(), (err, np.abs(ref).max())
    # ... and the restatement's inference mode on the checkpoint
    g, _, _ = ir.iresnet_graph(18, 3, 4, 32, 24)
    p64 = {k: v[k].numpy().astype(np.float64) for k, _ in tv}
    s64 = {k: v[k].numpy().astype(np.float64) for k, _ in st}
    env, _, _ = ir.forward(g, p64, x, False, s64, 'NCHW')
    assert np.abs(wfea - env['features']).max() <= 1e-4 * np.abs(env['features']).max()
