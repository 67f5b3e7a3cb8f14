"""-m gpu: SE-IResNet on the graph engine against the float64 restatement (tests/se_iresnet_ref.py), under the audit of
test_gpu_iresnet.py: every tensor is held to max(2e-5, 2 x the restatement's own float32-vs-float64 error on this input), every
gradient to max(1e-4, 2 x ...); inside a kink band -- max(1e-5 rms(u), 16 x the restatement's own fp32 noise on u), computed from
the reference alone -- the side the engine took is adopted.  The kinks are the PReLUs and the hidden ReLU of every block's gate (the
engine's side there: its stored hidden activations).  The net under test has one block per stage on 6 images of 32 x 24 x 3 (final
map 2 x 2, so a wrong flatten order fails) and 7 classes; its inputs are se_iresnet_ref.audit_case(), whose bands
test_se_iresnet_host.py keeps nearly empty."""
import numpy as np
import pytest
import torch

import se_iresnet_ref as sr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import dev, host, check_rell2
    from tf_face_toolbox_amd import _lib, net_select, Singular
    from tf_face_toolbox_amd.nets.iresnet import IResNet

BLOCKS = (1, 1, 1, 1)
N, H, W, NCLS = sr.AUDIT['n'], sr.AUDIT['h'], sr.AUDIT['w'], sr.AUDIT['ncls']
WD, LR = 5e-4, 0.05
GATE_VARS = ('fc1/weights', 'fc1/biases', 'fc2/weights', 'fc2/biases')


def _net(head, p, fmt='NCHW', blocks=BLOCKS):
    net = IResNet(18, weight_decay=WD, data_format=fmt, head=head, blocks=list(blocks), se=True)
    net.build(H, W, 3, NCLS, 'cuda')
    net.load_params(p)
    return net


def _kink(net):
    """prelu output -> u = scale * z + shift with the engine's z, scale, shift (exact in float64: the sign fma had on the device);
    gate output -> the engine's hidden activations (> 0 where its ReLU passed), without the zero padding of the stored width"""
    k = {op[1]: host(net.t[op[2]]) * host(net.bn[op[1]]['scale']) + host(net.bn[op[1]]['shift']) for op in net.plan if op[0] == 'bnprelu'}
    for op in net.plan:
        if op[0] == 'selin':
            hd = net.spec[op.se.w1][0][1]
            hid = host(net.t[op.out + '/hid'])
            assert hid.shape[1] == op.se.hidden and not hid[:, hd:].any(), 'the padding of the hidden layer is not zero'
            k[op.s] = hid[:, :hd]
    return k


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-30))


def _f32(d):
    return {k: v.astype(np.float32) for k, v in d.items()}


def _audit(net, g, head, p, state, x, y, fmt='NCHW'):
    """one training-mode pass of `net` (forward, loss, backward done by the caller) against the restatement"""
    kink = _kink(net)
    bands = sr.noise_bands(g, p, x, state, fmt)
    kw = dict(head=head, weight_decay=WD, kink=kink, bands=bands, data_format=fmt)
    l_ref, g_ref, env, new_state = sr.loss_and_grads(g, p, x, y, state=state, **kw)
    _, g32, env32, _ = sr.loss_and_grads(g, _f32(p), x.astype(np.float32), y, state=_f32(state), **kw)
    names = ['stem', 's1b0', 's1b0/c2/bn', 's2b0/c1', 's2b0/se', 's3b0/sc/bn', 's3b0', 's4b0', 'out/bn', 'embed', 'features'] + \
        (['logits'] if head == 'softmax' else [])            # (s1b0/c2/bn, s2b0/se: never stored, recomputed from z, scale, shift, gate)
    for name in names:
        got = host(net.t[name])
        if name == 'logits':
            got = got[:, :NCLS]
        r, r32 = _rel(got, env[name]), _rel(env32[name], env[name])
        print('%-12s rel %.2e (float32 restatement %.2e)' % (name, r, r32))
        assert r <= max(2e-5, 2 * r32), name
    for op in net.plan:
        if op[0] == 'selin':
            for what, key in (('sq', 'sq'), ('gate', 'gate')):
                got, ref, r32 = host(net.t[op.out + '/' + what]), env['cache'][op.s][key], env32['cache'][op.s][key]
                r, rr = _rel(got, ref), _rel(r32, ref)
                print('%-12s rel %.2e (float32 restatement %.2e)' % (op.out + '/' + what, r, rr))
                assert r <= max(2e-5, 2 * rr), (op.out, what)
    return l_ref, g_ref, g32, new_state


def _check_grads(net, p, g_ref, g32):
    for k in p:
        got = host(net.get_variable(k, net.grads)) + (WD * p[k] if k.endswith('weights') else 0)      # + wd * w (folded into the optimizer)
        r, r32 = _rel(got, g_ref[k]), _rel(g32[k], g_ref[k])
        print('grad %-60s rel %.2e (float32 restatement %.2e)' % (k, r, r32))
        assert float(np.abs(got).max()) > 0, k
        assert r <= max(1e-4, 2 * r32), ('grad ' + k, r, r32)


def _one_pass(head, fmt, blocks=BLOCKS):
    g, spec, p, state, x, y = sr.audit_case(blocks)
    net = _net(head, p, fmt, blocks)
    assert net.graph == g and sorted(net.variables) == sorted(p)
    assert sum(1 for op in net.plan if op[0] == 'selin') == sum(blocks) and not any(op[0] in ('se', 'seblock', 'add') for op in net.plan)
    assert sum(1 for k in p if k.endswith(GATE_VARS)) == 4 * sum(blocks)
    out = net.forward(dev(x), num_classes=NCLS, is_training=True)
    losses, names, _ = net.loss_function('TOWER', dev(y, torch.int32), **out)
    net.backward()
    torch.cuda.synchronize()
    assert names == ['cross_entropy', 'reg_loss']
    l_ref, g_ref, g32, new_state = _audit(net, g, head, p, state, x, y, fmt)
    assert abs(float(losses[0]) - l_ref[0]) <= 1e-4 * max(1, l_ref[0]) and abs(float(losses[1]) - l_ref[1]) <= 1e-5 * max(1, l_ref[1]), (losses, l_ref)
    _check_grads(net, p, g_ref, g32)
    for k in new_state:                                          # moving statistics: decay 0.9, unbiased variance
        got = host(net.get_variable(k))
        assert np.abs(got - new_state[k]).max() <= 3e-5 * np.abs(new_state[k]).max() + 1e-9, k
    return net


@pytest.mark.parametrize('head,fmt,fuse', [('softmax', 'NCHW', '1'), ('arcface', 'NHWC', '1'), ('softmax', 'NCHW', '0')],
                         ids=['softmax', 'arcface_nhwc', 'softmax_stats_stand_alone'])
def test_training_forward_loss_every_gradient_moving_statistics(head, fmt, fuse, monkeypatch):
    """fuse = '0': FTE_BN_FUSE=0, the statistics of every BN (the selin ops' too) from the stand-alone pass instead of the producing
    conv's epilogue"""
    monkeypatch.setenv('FTE_BN_FUSE', fuse)
    net = _one_pass(head, fmt)
    fused = [j for j in net.fuse_fwd.values() if net.plan[j][0] == 'selin']
    assert len(fused) == (4 if fuse == '1' else 0)


def test_identity_block_sums_the_two_gradients_of_its_input():
    """blocks = [2, 1, 1, 1]: s1b1 reads s1b0 through its leading BN and as its shortcut -- _add of the shortcut's dy and the BN's dz"""
    blocks = (2, 1, 1, 1)
    net = _one_pass('softmax', 'NCHW', blocks)
    assert 's1b0' in net.shortcut_shared and [op.shortcut for op in net.plan if op[0] == 'selin'][1] == 's1b0'


@pytest.mark.parametrize('head', ['softmax', 'arcface'])
def test_three_momentum_steps(head):
    """three Momentum steps through Singular on one batch; the restatement takes the same steps, resolving each step's kinks with
    that step's pre-activations.  Every variable's total update is held to max(1e-4, 2 x the float32 restatement's error) of itself."""
    g, spec, p, state, x, y = sr.audit_case()
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
        bands = sr.noise_bands(g, refs[np.float64]['p'], x, refs[np.float64]['s'])
        for dt, r in refs.items():
            ls, gr, _, r['s'] = sr.loss_and_grads(g, r['p'], x.astype(dt), y, head=head, weight_decay=WD, state=r['s'], kink=kink, bands=bands)
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
    for op in net.plan:                                           # the zero padding of the gate's stored width took three steps and stayed zero
        if op[0] == 'selin':
            hd = net.spec[op.se.w1][0][1]
            assert not net.view(op.se.w1).reshape(-1, op.se.hidden)[:, hd:].any() and not net.view(op.se.w2).reshape(op.se.hidden, -1)[hd:].any()
            assert not net.view(op.se.b1)[hd:].any()


@pytest.mark.parametrize('fmt', ['NCHW', 'NHWC'])
def test_inference_mode(fmt):
    """eval_features (moving statistics: fte_bn_infer_coef, then the squeeze, the gate and the apply) against the restatement's
    inference mode"""
    g, spec, p, state, x, y = sr.audit_case()
    rng = np.random.default_rng(9)
    st = {k: (v + 0.2 * rng.random(v.shape)) for k, v in state.items()}
    net = _net('arcface', p, fmt)
    for k, v in st.items():
        net.set_variable(k, torch.tensor(v, dtype=torch.float32))
    feat = host(net.eval_features(dev(x)))
    env, _, _ = sr.forward(g, p, x, False, st, fmt)
    env32, _, _ = sr.forward(g, _f32(p), x.astype(np.float32), False, _f32(st), fmt)
    assert feat.shape == (N, 512)
    assert _rel(feat, env['features']) <= max(2e-5, 2 * _rel(env32['features'], env['features']))
    for k, v in st.items():                                       # inference moves no statistics
        assert np.array_equal(host(net.get_variable(k)), v.astype(np.float32).astype(np.float64)), k


def test_bf16_operand_mode():
    """the procedure of test_gpu_iresnet.py::test_bf16_operand_mode: against the UNROUNDED restatement, rel-L2 1e-2 on features /
    logits, 1e-2 on the loss, 3e-2 on every gradient; the kink band is 4 x the restatement's own bf16 noise; the step is measurably
    not the fp32 one.  With the gate a shift of the block's last BN changes the squeeze, so only the betas of the shortcuts' BNs and
    of the output BN still have a gradient that cancels to zero."""
    g, spec, p, state, x, y = sr.audit_case()
    _lib.set_mfma_dtype('bf16')
    try:
        net = _net('softmax', p)
        out = net.forward(dev(x), num_classes=NCLS, is_training=True)
        losses, _, _ = net.loss_function('TOWER', dev(y, torch.int32), **out)
        net.backward()
        torch.cuda.synchronize()
        assert not net._act_s16
        bands = sr.noise_bands16(g, p, x, state)
        l_ref, g_ref, env, _ = sr.loss_and_grads(g, p, x, y, weight_decay=WD, state=state, kink=_kink(net), bands=bands, kink_mode='bf16')
        check_rell2(host(net.t['features']), env['features'], 1e-2, 'features (bf16 operands)')
        check_rell2(host(net.t['logits'])[:, :NCLS], env['logits'], 1e-2, 'logits (bf16 operands)')
        assert abs(float(losses[0]) - l_ref[0]) <= 1e-2 * l_ref[0]
        worst, zero = 0.0, []
        bn_out = {op[3]: op[1] for op in g if op[0] == 'bn'}
        for k in p:
            got = host(net.get_variable(k, net.grads)) + (WD * p[k] if k.endswith('weights') else 0)
            if k.endswith('/beta'):
                gt = env['tensor_grads'][bn_out[k[:-len('/beta')]]]
                gnorm = float(np.sqrt((gt * gt).sum()))
                if np.sqrt((g_ref[k] ** 2).sum()) <= 1e-9 * gnorm:
                    zero.append(k)
                    assert np.sqrt((got * got).sum()) <= 3e-2 * gnorm, (k, float(np.sqrt((got * got).sum())), gnorm)
                    continue
            worst = max(worst, check_rell2(got, g_ref[k], 3e-2, 'grad ' + k))
        assert worst > 1e-5
        assert set(zero) == set(['SE-IResNet-18/stage%d/block_0/conv_shortcut_1x1/BatchNorm/beta' % s for s in (1, 2, 3, 4)]
                                + ['SE-IResNet-18/output/BatchNorm/beta']), zero
    finally:
        _lib.set_mfma_dtype('f32')


def test_real_topology_one_step_and_determinism():
    """SE-IResNet-18-arcface as the factory builds it, 2 images of 112 x 96: names and shapes from the block table, one Momentum step
    with everything finite and every gradient non-zero, and a second net taking the same step ends with the same bytes.  The 56 x 48
    stage is split over several blocks per image here (2 images cannot fill the device)."""
    n, h, w, ncls = 2, 112, 96, 10
    assert sr.split_plan(n, 56 * 48, 64)[0] > 1
    rng = np.random.default_rng(4)
    x, y = dev(rng.uniform(-1, 1, (n, h, w, 3))), dev(rng.integers(0, ncls, n), torch.int32)
    arenas = []
    for _ in range(2):
        net = net_select('SE-IResNet-18-arcface', 'NCHW', WD)
        step, losses, names, _ = Singular(net, 0.01, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
        w0 = net.params.clone()
        step()
        torch.cuda.synchronize()
        tv, st = sr.expected_variables(18, 3, ncls, h, w)
        assert sorted(net.variables) == sorted(k for k, _ in tv)
        for k, shape in tv:
            assert tuple(net.get_variable(k).shape) == shape, k
            gk = net.get_variable(k, net.grads)
            assert torch.isfinite(gk).all(), k
            if not k.endswith(('conv_shortcut_1x1/BatchNorm/beta', 'output/BatchNorm/beta')):      # (zero by construction: rounding noise)
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


def test_the_50_layer_net_builds():
    net = net_select('SE-IResNet-50-arcface')
    net.build(112, 112, 3, 100, 'cuda')
    assert net.name == 'SE-IResNet-50' and net.head == 'arcface' and sum(1 for op in net.plan if op[0] == 'selin') == 24
    assert net.params.is_cuda and len(net.variables) == len(sr.expected_variables(50, 3, 100, 112, 112)[0])
