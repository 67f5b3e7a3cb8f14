"""-m gpu: ShuffleNet-v2 (depthwise 3x3, channel split / concat / shuffle, 64-padded channel storage) through the
reference-shaped API and the C ABI against the float64 graph oracle."""
import numpy as np
import pytest
import torch

from oracle import graphnet as og, ops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import dev, host, stream, ws, check_maxabs, check_rell2
    from tf_face_toolbox_amd import net_select, Singular, _lib
    from tf_face_toolbox_amd.nets.shufflenet_v2 import ShuffleNet_v2_small, ShuffleNet_v2_middle, ShuffleNet_v2_large
    from test_gpu_resnet import _kink


@pytest.mark.parametrize('n,h,w,c,stride', [(3, 14, 14, 128, 1), (2, 28, 28, 64, 2), (2, 7, 9, 256, 2), (1, 4, 4, 512, 1),
                                            (5, 13, 8, 192, 1), (64, 14, 14, 128, 2),
                                            (2, 13, 8, 64, 2), (3, 28, 27, 128, 2), (2, 5, 5, 64, 2)])       # stride 2 with SAME pads (1,0) / (0,1) / (1,1): the parity-patch dgrad
def test_depthwise_conv_kernels(n, h, w, c, stride):
    rng = np.random.default_rng(n * 100 + c + stride)
    x = rng.standard_normal((n, h, w, c)); wt = rng.standard_normal((3, 3, c, 1)) * 0.3
    y = ops.dwconv3x3_fwd(x, wt, stride)
    dy = rng.standard_normal(y.shape)
    dx, dw = ops.dwconv3x3_bwd(x, wt, dy, stride)
    xd, wd_, dyd = dev(x), dev(wt.reshape(3, 3, c)), dev(dy)
    yd = torch.empty(y.shape, device='cuda'); dxd = torch.empty(x.shape, device='cuda'); dwd = torch.empty(3, 3, c, device='cuda')
    _lib.call('fte_dwconv3x3_fwd', xd, wd_, yd, n, h, w, c, stride, stream())
    _lib.call('fte_dwconv3x3_dgrad', dyd, wd_, dxd, n, h, w, c, stride, stream())
    buf, nb = ws(_lib.query('fte_dwconv3x3_wgrad_ws_bytes', n, h, w, c, stride))
    _lib.call('fte_dwconv3x3_wgrad', xd, dyd, dwd, n, h, w, c, stride, buf, nb, stream())
    check_maxabs(host(yd), y, 2e-6, 'dw fwd')
    check_maxabs(host(dxd), dx, 2e-6, 'dw dgrad')
    check_rell2(host(dwd), dw.reshape(3, 3, c), 2e-6, 'dw wgrad')


@pytest.mark.parametrize('fmt', ['NCHW', 'NHWC'])
@pytest.mark.parametrize('ca', [12, 122, 58])
def test_channel_gather_is_concat_shuffle_split(ca, fmt):
    """The engine's tables against the literal reference sequence: bit-exact (pure data movement)."""
    net = ShuffleNet_v2_small(alpha=2.0, data_format=fmt)
    net.device = torch.device('cuda')
    pc = net._pc
    n, h, w = 3, 5, 4
    rng = np.random.default_rng(ca)
    a, b = rng.standard_normal((n, h, w, ca)).astype(np.float32), rng.standard_normal((n, h, w, ca)).astype(np.float32)
    s_ref, x_ref = ops.channel_split(ops.channel_shuffle(np.concatenate([a, b], -1), fmt))
    net.real_c = {'a': ca, 'b': ca}
    net.shapes = {k: (h, w, pc(ca)) for k in ('a', 'b', 's', 'x')}
    net.shapes['cat'] = (h, w, pc(2 * ca))
    net.real_c['cat'] = 2 * ca

    def padded(v):
        out = np.zeros(v.shape[:-1] + (pc(v.shape[-1]),), np.float32)
        out[..., :v.shape[-1]] = v
        return dev(out)
    ad, bd = padded(a), padded(b)
    rows = n * h * w

    def run(table, s0, s1, co):
        out = torch.full((n, h, w, co), 7.0, device='cuda')
        _lib.call('fte_channel_gather', s0, s1, out, table, rows, s0.shape[-1], s1.shape[-1] if s1 is not None else 0, co, stream())
        return out
    tb = net._gather_tables(('shufsplit', 's', 'a', 'b', 'x', fmt))
    sd = run(tb['outs'][0][1], ad, bd, pc(ca)); xd = run(tb['outs'][1][1], ad, bd, pc(ca))
    np.testing.assert_array_equal(sd.cpu().numpy()[..., :ca], s_ref); np.testing.assert_array_equal(xd.cpu().numpy()[..., :ca], x_ref)
    assert float(sd[..., ca:].abs().max()) == 0 and float(xd[..., ca:].abs().max()) == 0          # padding stays zero
    # backward tables = the inverse permutation: gather(s, x) must give back a and b
    a2 = run(tb['bwd'][0][1], sd, xd, pc(ca)); b2 = run(tb['bwd'][1][1], sd, xd, pc(ca))
    assert torch.equal(a2, ad) and torch.equal(b2, bd)
    tc = net._gather_tables(('shufcat', 'cat', 'a', 'b', fmt))
    cd = run(tc['outs'][0][1], ad, bd, pc(2 * ca))
    np.testing.assert_array_equal(cd.cpu().numpy()[..., :2 * ca], ops.channel_shuffle(np.concatenate([a, b], -1), fmt))
    assert torch.equal(run(tc['bwd'][0][1], cd, None, pc(ca)), ad) and torch.equal(run(tc['bwd'][1][1], cd, None, pc(ca)), bd)
    net.real_c['in'] = 2 * ca; net.shapes['in'] = (h, w, pc(2 * ca))
    ts = net._gather_tables(('split', 's', 'in', 'x'))
    h0 = run(ts['outs'][0][1], cd, None, pc(ca)); h1 = run(ts['outs'][1][1], cd, None, pc(ca))
    r0, r1 = ops.channel_split(cd.cpu().numpy()[..., :2 * ca])
    np.testing.assert_array_equal(h0.cpu().numpy()[..., :ca], r0); np.testing.assert_array_equal(h1.cpu().numpy()[..., :ca], r1)
    assert torch.equal(run(ts['bwd'][0][1], h0, h1, pc(2 * ca)), cd)


@pytest.mark.parametrize('s16', [0, 1])
@pytest.mark.parametrize('rows,ca,cb,co0,co1', [(256 * 28 * 28 // 8 + 3, 128, 128, 128, 128), (9001, 256, 256, 256, 256), (777, 512, 512, 512, 512),
                                             (5003, 256, 0, 128, 128), (4099, 128, 128, 256, 0), (1234, 32, 32, 32, 0), (3001, 64, 192, 64, 64),
                                             (2050, 40, 24, 32, 32), (2051, 40, 32, 40, 32)])
def test_channel_gather_row_groups_through_lds(rows, ca, cb, co0, co1, s16):
    """The LDS form of the gather (power-of-two quads per row; csrc/layers.hip channel_gather_lds_kernel) and the element form
    (the last case: 10 + 8 quads) against plain indexing: random tables with zero entries, row counts that end inside a row
    group, one and two sources / outputs; bit-exact without the affine, and the affine = fma + max of the source's scale / shift."""
    g = torch.Generator(device='cuda').manual_seed(rows + ca)
    a = torch.randn(rows, ca, device='cuda', generator=g)
    b = torch.randn(rows, cb, device='cuda', generator=g) if cb else None
    if s16:
        a = a.bfloat16().float(); b = b.bfloat16().float() if cb else None
    perm = torch.randperm(ca + cb, generator=torch.Generator().manual_seed(ca + co0)).tolist()
    ent = [(-1 if k % 11 == 3 else k) for k in (perm * 2)[:co0 + co1]]
    enc = lambda ks: torch.tensor([(-1 if k < 0 else ((0 << 16) | k if k < ca else (1 << 16) | (k - ca))) for k in ks], dtype=torch.int32, device='cuda')
    t0, t1 = enc(ent[:co0]), (enc(ent[co0:]) if co1 else None)
    cat = torch.cat([a, b], 1) if cb else a

    def ref(src, ks):
        idx = torch.tensor([max(k, 0) for k in ks], device='cuda')
        out = src[:, idx]
        out[:, torch.tensor([k < 0 for k in ks], device='cuda')] = 0
        return out
    bits = lambda x: x.bfloat16().view(torch.int16)
    dt = dict(dtype=torch.int16 if s16 else torch.float32, device='cuda')
    arg = (lambda x: None if x is None else bits(x)) if s16 else (lambda x: x)
    sfx = '_s16' if s16 else ''
    o0 = torch.empty(rows, co0, **dt); o1 = torch.empty(rows, co1, **dt) if co1 else None
    _lib.call('fte_channel_gather' + sfx, arg(a), arg(b), o0, t0, rows, ca, cb, co0, stream())
    want = ref(cat, ent[:co0])
    assert torch.equal(o0, bits(want) if s16 else want)
    _lib.call('fte_channel_gather_affine' + sfx, arg(a), arg(b), o0, t0, co0, o1, t1, co1, rows, ca, cb, None, None, 0, None, None, 0, stream())
    assert torch.equal(o0, bits(want) if s16 else want)
    if co1:
        w1 = ref(cat, ent[co0:])
        assert torch.equal(o1, bits(w1) if s16 else w1)
    sca = torch.rand(ca, device='cuda', generator=g) + 0.5; sfa = torch.randn(ca, device='cuda', generator=g) * 0.2
    scb = torch.rand(max(cb, 1), device='cuda', generator=g) + 0.5; sfb = torch.randn(max(cb, 1), device='cuda', generator=g) * 0.2
    _lib.call('fte_channel_gather_affine' + sfx, arg(a), arg(b), o0, t0, co0, o1, t1, co1, rows, ca, cb, sca, sfa, 1,
              scb if cb else None, sfb if cb else None, 0, stream())
    ya = torch.relu(a.double() * sca.double() + sfa.double())
    ycat = torch.cat([ya, b.double() * scb.double() + sfb.double()], 1) if cb else ya
    for o, ks in ((o0, ent[:co0]), (o1, ent[co0:])):
        if o is None:
            continue
        got = o.view(torch.bfloat16).double() if s16 else o.double()
        err = (got - ref(ycat, ks)).abs().max().item()
        assert err <= (2e-2 if s16 else 2e-6), err


@pytest.mark.parametrize('rows,c', [(3 * 14 * 14, 128), (512 * 7 * 7, 256), (40, 64)])
def test_bn_folded_into_the_gather_is_the_unfused_sequence_bit_for_bit(rows, c):
    """fte_bn_train_stats + fte_channel_gather_affine == fte_bn_train_fwd + fte_channel_gather, and the backward pass with
    the mask recomputed from z == the one reading the stored output: both bit-exact (same fma, same reduction order)."""
    g = torch.Generator(device='cuda').manual_seed(rows + c)
    rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=g)
    z, s_in, dy = rnd(rows, c), rnd(rows, c), rnd(rows, c)
    gamma, beta = rnd(c) * 0.5 + 1.0, rnd(c) * 0.3
    buf, nb = ws(_lib.query('fte_bn_ws_bytes', c))
    new = lambda: [torch.empty(c, device='cuda') for _ in range(4)]
    y = torch.empty_like(z)
    m0 = new(); m1 = new()
    _lib.call('fte_bn_train_fwd', z, gamma, beta, None, y, m0[0], m0[1], m0[2], m0[3], None, None, rows, c, 1e-5, 0.9, 1, buf, nb, stream())
    _lib.call('fte_bn_train_stats', z, gamma, beta, m1[0], m1[1], m1[2], m1[3], None, None, rows, c, 1e-5, 0.9, buf, nb, stream())
    for a, b in zip(m0, m1):
        assert torch.equal(a, b)
    perm = torch.randperm(2 * c, generator=torch.Generator().manual_seed(c)).tolist()
    table = torch.tensor([((j // c) << 16) | (j % c) for j in perm[:c]], dtype=torch.int32, device='cuda')
    o0 = torch.empty(rows, c, device='cuda'); o1 = torch.empty(rows, c, device='cuda'); o2 = torch.empty(rows, c, device='cuda')
    _lib.call('fte_channel_gather', s_in, y, o0, table, rows, c, c, c, stream())
    _lib.call('fte_channel_gather_affine', s_in, z, o1, table, c, None, None, 0, rows, c, c, None, None, 0, m1[2], m1[3], 1, stream())
    assert torch.equal(o0, o1)
    _lib.call('fte_channel_gather', y, s_in, o0, table, rows, c, c, c, stream())
    _lib.call('fte_channel_gather_affine', z, s_in, o2, table, c, None, None, 0, rows, c, c, m1[2], m1[3], 1, None, None, 0, stream())
    assert torch.equal(o0, o2)
    # two outputs in one launch == two launches
    table_b = torch.tensor([((j // c) << 16) | (j % c) for j in perm[c:]], dtype=torch.int32, device='cuda')
    o3 = torch.empty(rows, c, device='cuda'); o4 = torch.empty(rows, c, device='cuda'); o5 = torch.empty(rows, c, device='cuda')
    _lib.call('fte_channel_gather', y, s_in, o3, table_b, rows, c, c, c, stream())
    _lib.call('fte_channel_gather_affine', z, s_in, o4, table, c, o5, table_b, c, rows, c, c, m1[2], m1[3], 1, None, None, 0, stream())
    assert torch.equal(o4, o0) and torch.equal(o5, o3)
    outs = []
    for zmask in (False, True):
        dz = torch.empty_like(z); dg = torch.empty(c, device='cuda'); db = torch.empty(c, device='cuda')
        if zmask:
            _lib.call('fte_bn_train_bwd_zmask', dy, z, gamma, m1[0], m1[1], m1[2], m1[3], dz, dg, db, rows, c, buf, nb, stream())
        else:
            _lib.call('fte_bn_train_bwd', dy, y, z, gamma, m0[0], m0[1], dz, dg, db, rows, c, buf, nb, stream())
        outs.append((dz, dg, db))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # inference coefficients: the ones fte_bn_infer_fwd derives
    mm, mv = rnd(c) * 0.1, rnd(c).abs() + 0.5
    sc0, sf0, sc1, sf1 = new()
    _lib.call('fte_bn_infer_fwd', z, gamma, beta, mm, mv, None, y, sc0, sf0, rows, c, 1e-5, 1, stream())
    _lib.call('fte_bn_infer_coef', gamma, beta, mm, mv, sc1, sf1, c, 1e-5, stream())
    assert torch.equal(sc0, sc1) and torch.equal(sf0, sf1)


def test_shufflenet_folds_every_gather_only_bn():
    """conv3_1x1's and the stride-2 shortcut's BN + ReLU outputs feed only the concat / shuffle / split: 16 + 3 folded BNs in the
    x2 net, none of them stored; asking for one recomputes it."""
    net = ShuffleNet_v2_small(alpha=2.0)
    net.build(64, 64, 3, 10, 'cuda')
    kinds = [op[0] for op in net.plan]
    assert kinds.count('bnstats') == 19 and len(net.folded) == 19
    x = torch.rand(4, 64, 64, 3, device='cuda') * 2 - 1
    net.forward(x, num_classes=10, is_training=True)
    name = 'conv3b1/c3'
    assert name in net.folded and name not in dict.keys(net.t)
    y = net.t[name]
    zname, relu = net.folded[name]
    assert relu == 1 and y.shape == net.t[zname].shape and float(y.min()) == 0.0


def _check_net(net, variant, blocks, fmt, n, h, w, ncls, seed):
    graph, spec = og.shufflenet_train_graph(variant, 3, ncls, fmt, blocks_override=blocks)
    p, state = og.init_params(spec, seed)
    p = og.perturb(p, seed + 1)
    rng = np.random.default_rng(seed + 2)
    x = rng.uniform(-1, 1, (n, h, w, 3)); y = rng.integers(0, ncls, n)
    if blocks is not None:
        net.num_block = list(blocks)
    net.build(h, w, 3, ncls, 'cuda')
    assert net.graph == graph and sorted(net.variables) == sorted(p)          # same op list, same variable names and shapes
    assert all(tuple(net.variables[k].ref_shape) == p[k].shape for k in p)
    net.load_params(p)
    net.dropout_seed = 5
    xd, yd = dev(x), dev(y, torch.int32)
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    mask = host(net.t['features_drop/mask'])
    kink = {}
    for op in net.graph:                                      # the HIP path's ReLU outputs / pool arg-max, unpadded
        if op[0] == 'relu':
            kink[op[1]] = host(net.t[op[1]])[..., :net.real_c[op[1]]]
        elif op[0] == 'maxpool':
            kink[op[1] + '/idx'] = net.t[op[1] + '/idx'].cpu().numpy()[..., :net.real_c[op[1]]]
            kink[op[1]] = host(net.t[op[1]])[..., :net.real_c[op[1]]]
    bands = og.noise_bands(graph, p, x, {'features_drop': mask}, state)
    l_ref, g_ref, env, new_state = og.loss_and_grads(graph, p, x, y, 5e-4, masks={'features_drop': mask}, state=state, kink=kink, bands=bands)
    p32 = {k: v.astype(np.float32) for k, v in p.items()}
    s32 = {k: v.astype(np.float32) for k, v in state.items()}
    _, g32, env32, _ = og.loss_and_grads(graph, p32, x.astype(np.float32), y, np.float32(5e-4),
                                         masks={'features_drop': mask.astype(np.float32)}, state=s32, kink=kink, bands=bands)

    def rel(a, b):
        return float(np.sqrt(((np.asarray(a, np.float64) - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), 1e-30))
    # every activation the engine stores: real channels match the oracle, padding channels are exactly zero
    worst = 0.0
    for name, t in net.t.items():
        if name in env and name != 'images' and t.dtype == torch.float32:
            rc = net.real_c[name]
            got = host(t)
            if name != 'logits':
                assert np.abs(got[..., rc:]).max(initial=0.0) == 0.0, 'padding of %s is not zero' % name
            e = rel(got[..., :rc], env[name])
            assert e <= max(2e-5, 2 * rel(env32[name], env[name])), (name, e, rel(env32[name], env[name]))
            worst = max(worst, e)
    assert abs(float(losses[0]) - l_ref[0]) <= 1e-4 * max(1, l_ref[0]) and abs(float(losses[1]) - l_ref[1]) <= 1e-5 * max(1, l_ref[1])
    for k in p:
        got = host(net.get_variable(k, net.grads)) + (5e-4 * p[k] if k.endswith('weights') else 0)     # + wd*w (folded into the optimizer)
        ref = g_ref.get(k, np.zeros_like(p[k]))               # large net: the dead stem BN variables get no gradient
        if not np.any(ref):
            assert not np.any(got), k
            continue
        # a BN beta (or a bias) that feeds conv -> BN has a true gradient of exactly zero (the next BN removes any
        # per-channel constant); the oracle gives 1e-18, fp32 gives 1e-9: judge those against an absolute noise floor
        err = np.sqrt(((got - ref) ** 2).sum())
        floor = 1e-7 * np.sqrt(ref.size)
        assert err <= max(1e-4 * np.sqrt((ref * ref).sum()), 2 * np.sqrt(((g32[k] - ref) ** 2).sum()), floor), ('grad ' + k, err, floor)
    # gradient arena outside the real entries (the padding rows / columns) must be exactly zero
    real = torch.zeros_like(net.grads[:net.arena_size])
    ones = {k: np.ones(p[k].shape) for k in p}
    for k in p:
        net.set_variable(k, ones[k], arena=real)
    assert float(net.grads[:net.arena_size][real == 0].abs().max()) == 0.0
    for k in new_state:
        got = host(net.get_variable(k))
        assert np.abs(got - new_state[k]).max() <= 3e-5 * np.abs(new_state[k]).max() + 1e-9, k
    return worst


@pytest.mark.parametrize('n,h,w,fmt', [(8, 64, 64, 'NCHW'), (4, 112, 112, 'NCHW'), (6, 64, 48, 'NHWC')])
def test_shufflenet_small_x2_forward_loss_and_every_gradient(n, h, w, fmt):
    """net_base.py:37-42's net: alpha = 2.0 (122 / 244 / 488 / 2048), all 16 blocks."""
    _check_net(ShuffleNet_v2_small(alpha=2.0, data_format=fmt), 'small', None, fmt, n, h, w, 10, 31)


def test_shufflenet_other_widths_and_variants():
    _check_net(ShuffleNet_v2_small(alpha=1.0), 'small_x1', [2, 2, 2], 'NCHW', 6, 64, 64, 7, 41)
    _check_net(ShuffleNet_v2_middle(), 'middle', [2, 2, 2, 2], 'NCHW', 6, 64, 64, 7, 51)
    _check_net(ShuffleNet_v2_large(), 'large', [2, 1, 1, 2], 'NCHW', 4, 32, 32, 7, 61)          # SE gate + stride-1 stem + dead stem convs


def test_shufflenet_training_steps_and_eval_mode():
    ncls, n, h, w = 10, 16, 64, 64
    net = net_select('ShuffleNet-v2-small', 'NCHW', 5e-4)
    assert net.name == 'ShuffleNet_v2_small_x2'
    rng = np.random.default_rng(1)
    x = dev(rng.uniform(-1, 1, (n, h, w, 3))); y = dev(rng.integers(0, ncls, n), torch.int32)
    step, losses, names, _ = Singular(net, 0.05, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
    w0 = net.params.clone()
    real = torch.zeros_like(net.params)
    for k, v in net.variables.items():
        net.set_variable(k, torch.ones(v.ref_shape), arena=real)
    hist = []
    for i in range(40):
        step()
        hist.append(float(losses[0]))
    assert all(np.isfinite(hist)) and not torch.equal(w0, net.params)
    assert np.mean(hist[-8:]) < np.mean(hist[:8])
    assert float(net.params[real == 0].abs().max()) == 0.0          # 40 optimizer steps later the padding is still exactly zero
    assert names == ['cross_entropy', 'reg_loss']
    out = net.forward(x, num_classes=ncls, is_training=False)['logits']
    assert out.shape == (n, ncls) and torch.isfinite(out).all()
    assert net.get_variable('ShuffleNet_v2_small_x2/conv2/resBlock_1/conv1_1x1/BatchNorm/moving_mean').shape == (122,)
    assert net.get_variable('ShuffleNet_v2_small_x2/conv2/resBlock_0/separable_conv_shortcut_3x3/depthwise_weights').shape == (3, 3, 12, 1)


@pytest.mark.parametrize('name,n', [('ShuffleNet-v2-small', 8), ('ResNet-26', 6), ('ResNeXt-26', 4), ('SENet-50', 4)])
def test_second_stream_and_folded_gather_change_no_bit(name, n, monkeypatch):
    """The filter gradients run on a second HIP stream, BN is folded into the channel gather and the 3x3 stem runs on the direct
    conv: every kernel is deterministic and the folds evaluate the same fused multiply-adds, so after five optimizer steps the
    parameter arena is BIT-IDENTICAL to a run with the side stream and the gather fold switched off -- and to one that keeps the side
    stream for the filter gradients but takes the shortcut branches, the classifier's filter gradient and the weight-decay sum off it."""
    ncls, h, w = 10, 64, 64
    rng = np.random.default_rng(3)
    x = dev(rng.uniform(-1, 1, (n, h, w, 3))); y = dev(rng.integers(0, ncls, n), torch.int32)

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        net = net_select(name, 'NCHW', 5e-4)
        net.dropout_seed = 11
        step, losses, _, _ = Singular(net, 0.05, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        return net.params.clone(), float(losses[0]), net
    moves = ('FTE_SHORTCUT_SIDE', 'FTE_HEAD_SIDE', 'FTE_REG_SIDE')          # these only choose the stream a launch goes to
    p1, l1, net1 = run(dict({'FTE_SIDE_STREAM': '1', 'FTE_BN_GATHER': '1'}, **{k: '1' for k in moves}))
    p2, l2, net2 = run(dict({'FTE_SIDE_STREAM': '1', 'FTE_BN_GATHER': '1'}, **{k: '0' for k in moves}))
    p0, l0, net0 = run(dict({'FTE_SIDE_STREAM': '0', 'FTE_BN_GATHER': '0'}, **{k: '0' for k in moves}))
    assert net1.side is not None and net2.side is not None and net0.side is None
    assert (len(net1.folded) > 0) == name.startswith('Shuffle') and len(net0.folded) == 0
    assert (len(net1.shortcut_fwd) > 0) == (not name.startswith('Shuffle')) and len(net2.shortcut_fwd) == 0 and len(net0.shortcut_fwd) == 0
    assert np.isfinite(l1) and l1 == l0 and l1 == l2
    assert torch.equal(p1, p0) and torch.equal(p1, p2)


def test_config5_per_gpu_workload_properties():
    """BASELINE config 5 at its per-GPU size (ShuffleNet-v2 + softmax, 2048 images on 8 GPUs = 256 x 112 x 112 per GPU, 10575
    classes), through size-independent properties -- the float64 oracle needs hours at this size:
      * determinism: the same three optimizer steps from the same weights give a bit-identical parameter arena and losses
        (ordered reductions everywhere, second stream included);
      * the channel padding (and the 27..31 unused rows of the 32-wide stem filter) is exactly zero in the gradient and stays zero
        in the parameters;
      * eval mode (moving statistics) of image 0..7 alone == the same images inside the 256-batch (inference BN has no batch
        coupling) to 2e-5 of the largest feature, across different tile plans and split-K factors."""
    ncls, n, h, w = 10575, 256, 112, 112
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(n, h, w, 3, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, ncls, (n,), generator=g, dtype=torch.int32).cuda()

    def run():
        net = net_select('ShuffleNet-v2-small', 'NCHW', 5e-4)
        net.seed = 9
        net.dropout_seed = 3
        step, losses, names, _ = Singular(net, 0.05, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': n})
        hist = []
        for _ in range(3):
            step()
            hist.append([float(v) for v in losses])
        torch.cuda.synchronize()
        return net, hist
    net_a, hist_a = run()
    net_b, hist_b = run()
    assert hist_a == hist_b and all(np.isfinite(v) for row in hist_a for v in row)
    assert torch.equal(net_a.params, net_b.params) and torch.equal(net_a.grads, net_b.grads)
    real = torch.zeros_like(net_a.params)
    for k, v in net_a.variables.items():
        net_a.set_variable(k, torch.ones(v.ref_shape), arena=real)
    assert float(net_a.params[real == 0].abs().max()) == 0.0 and float(net_a.grads[:net_a.arena_size][real == 0].abs().max()) == 0.0
    net_a.forward(x, num_classes=ncls, is_training=False)
    full = net_a.t['features'][:8].clone()
    net_a.forward(x[:8].contiguous(), num_classes=ncls, is_training=False)
    alone = net_a.t['features'].clone()
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    check_maxabs(host(alone), host(full).astype(np.float64), 2e-5, 'eval features: 8 images alone vs inside the 256-batch')
