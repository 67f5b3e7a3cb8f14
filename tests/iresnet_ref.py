"""float64 restatement of IResNet (Deng et al., CVPR 2019, section 3.2) and of the fused BN + PReLU kernels, composed from
oracle.ops.  TEST INFRASTRUCTURE: the block table, the variable names and the op list below are written from the paper and the
issue that introduced the nets, not derived from tf_face_toolbox_amd/nets/iresnet.py -- the tests compare the two.

  block   BN -> conv 3x3 -> BN -> PReLU -> conv 3x3 (stride) -> BN, plus the shortcut (identity, or conv 1x1 (stride) -> BN in the
          first block of every stage)
  stem    conv 3x3 stride 1, in -> 64 -> BN -> PReLU, no pooling
  output  BN -> flatten -> FC to 512 (no bias) -> BN = features

PReLU convention (fte.h "BN + PReLU"): y = u > 0 ? u : alpha * u, slope alpha AT u == 0 (oracle.ops.prelu_bwd puts alpha / 2 there:
TF's relu / abs composition, which SphereNet mirrors; the fused kernels do not)."""
from collections import OrderedDict

import numpy as np

from oracle import ops

BLOCKS = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 14, 3], 100: [3, 13, 30, 3]}
WIDTHS = [64, 128, 256, 512]
EMBED = 512
BN_EPS, BN_DECAY = 1e-5, 0.9
KINK_BAND = 1e-5          # oracle.graphnet.KINK_BAND: |u| < KINK_BAND * rms(u) cannot be placed by an fp32 evaluation
NOISE_MULT = 16           # oracle.graphnet.NOISE_MULT: ... nor |u| < 16 x the restatement's own fp32 noise on that tensor
CLS = 'classifier/fc_classifier/weights'


def _out_hw(h, w):
    for _ in range(4):                     # one stride-2 conv per stage, TF 'SAME'
        h, w = -(-h // 2), -(-w // 2)
    return h, w


def iresnet_graph(depth, in_ch, num_classes, h, w, blocks=None):
    """-> (graph, spec, name).  spec = [(variable, reference shape, kind)]; the op list is what nets/graph.py executes."""
    blocks = BLOCKS[depth] if blocks is None else list(blocks)
    name = 'IResNet-%d' % depth
    g, spec = [], []

    def bn(scope, out, inp, c):
        spec.append((scope + '/BatchNorm/gamma', (c,), 'gamma'))
        spec.append((scope + '/BatchNorm/beta', (c,), 'beta'))
        g.append(('bn', out, inp, scope + '/BatchNorm'))

    def conv(scope, out, inp, k, cin, cout, stride):
        spec.append((scope + '/weights', (k, k, cin, cout), 'conv_w'))
        g.append(('conv', out, inp, scope + '/weights', stride))

    def prelu(scope, out, inp, c):
        spec.append((scope + '/prelu/alpha', (c,), 'alpha'))
        g.append(('prelu', out, inp, scope + '/prelu/alpha'))
    s = name + '/stem/conv_3x3'
    conv(s, 'stem/z', 'images', 3, in_ch, 64, 1)
    bn(s, 'stem/bn', 'stem/z', 64)
    prelu(s, 'stem', 'stem/bn', 64)
    x, cin = 'stem', 64
    for si, (nb, cout) in enumerate(zip(blocks, WIDTHS)):
        for bi in range(nb):
            sc = '%s/stage%d/block_%d' % (name, si + 1, bi)
            t = 's%db%d' % (si + 1, bi)
            stride = 2 if bi == 0 else 1
            shortcut = x
            if bi == 0:
                conv(sc + '/conv_shortcut_1x1', t + '/sc/z', x, 1, cin, cout, stride)
                bn(sc + '/conv_shortcut_1x1', t + '/sc/bn', t + '/sc/z', cout)
                shortcut = t + '/sc/bn'
            bn(sc + '/bn1', t + '/bn1', x, cin)
            conv(sc + '/conv1_3x3', t + '/c1/z', t + '/bn1', 3, cin, cout, 1)
            bn(sc + '/conv1_3x3', t + '/c1/bn', t + '/c1/z', cout)
            prelu(sc + '/conv1_3x3', t + '/c1', t + '/c1/bn', cout)
            conv(sc + '/conv2_3x3', t + '/c2/z', t + '/c1', 3, cout, cout, stride)
            bn(sc + '/conv2_3x3', t + '/c2/bn', t + '/c2/z', cout)
            g.append(('add', t, t + '/c2/bn', shortcut))
            x, cin = t, cout
    bn(name + '/output', 'out/bn', x, cin)
    oh, ow = _out_hw(h, w)
    spec.append((name + '/output/fc/weights', (oh * ow * cin, EMBED), 'embed_w'))
    g.append(('fc', 'embed', 'out/bn', name + '/output/fc/weights', None))
    bn(name + '/output/fc', 'features', 'embed', EMBED)
    spec.append((CLS, (EMBED, num_classes), 'cls_w'))
    g.append(('fc', 'logits', 'features', CLS, None))
    return g, spec, name


def init_params(spec, seed, dtype=np.float64):
    """Xavier-uniform filters, gamma 1, beta 0, alpha 0.25, classifier N(0, 1e-3); moving statistics (0, 1)"""
    rng = np.random.default_rng(seed)
    p, state = OrderedDict(), OrderedDict()
    for name, shape, kind in spec:
        if kind == 'conv_w':
            k, _, cin, cout = shape
            lim = np.sqrt(6.0 / (k * k * cin + k * k * cout))
            p[name] = rng.uniform(-lim, lim, shape).astype(dtype)
        elif kind == 'embed_w':
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            p[name] = rng.uniform(-lim, lim, shape).astype(dtype)
        elif kind == 'cls_w':
            p[name] = (0.001 * rng.standard_normal(shape)).astype(dtype)
        elif kind == 'alpha':
            p[name] = np.full(shape, 0.25, dtype)
        elif kind == 'gamma':
            p[name] = np.ones(shape, dtype)
            pre = name[:-len('/gamma')]
            state[pre + '/moving_mean'] = np.zeros(shape, dtype)
            state[pre + '/moving_variance'] = np.ones(shape, dtype)
        elif kind == 'beta':
            p[name] = np.zeros(shape, dtype)
        else:
            raise ValueError(kind)
    return p, state


def perturb(p, seed, scale=0.1):
    """gamma / beta / alpha away from their initial constants (alpha of both signs), the classifier to a useful size"""
    rng = np.random.default_rng(seed)
    q = OrderedDict()
    for k, v in p.items():
        if k.endswith(('/gamma', '/beta')):
            q[k] = (v + scale * rng.standard_normal(v.shape)).astype(v.dtype)
        elif k.endswith('/alpha'):
            q[k] = (v + 0.3 * rng.standard_normal(v.shape)).astype(v.dtype)
        elif k == CLS:
            q[k] = (0.05 * rng.standard_normal(v.shape)).astype(v.dtype)
        else:
            q[k] = v
    return q


def _flat(x, data_format):
    """[n, h, w, c] -> [n, h w c] in the flatten order of `data_format` (the checkpoint layout of the FC rows, as SphereNet's fc)"""
    if x.ndim == 2:
        return x
    if data_format == 'NCHW':
        x = x.transpose(0, 3, 1, 2)
    return x.reshape(x.shape[0], -1)


def _unflat(d, shape, data_format):
    if len(shape) == 2:
        return d
    n, h, w, c = shape
    if data_format == 'NCHW':
        return d.reshape(n, c, h, w).transpose(0, 2, 3, 1)
    return d.reshape(n, h, w, c)


def forward(graph, p, images, train=True, state=None, data_format='NCHW', eps=BN_EPS, decay=BN_DECAY):
    """-> (env, cache, new moving statistics).  Works in the dtype of its inputs (float32 gives the restatement's own fp32 noise)."""
    env, cache, new_state = {'images': images}, {}, OrderedDict()
    for op in graph:
        kind, out = op[0], op[1]
        if kind == 'conv':
            env[out] = ops.conv2d_fwd(env[op[2]], p[op[3]], op[4])
        elif kind == 'bn':
            x, pre = env[op[2]], op[3]
            gam, bet = p[pre + '/gamma'], p[pre + '/beta']
            if train:
                env[out], cache[out] = ops.bn_train_fwd(x, gam, bet, x.dtype.type(eps))
                if state is not None:
                    cnt = float(np.prod(x.shape[:-1]))
                    new_state[pre + '/moving_mean'], new_state[pre + '/moving_variance'] = ops.bn_moving_update(
                        state[pre + '/moving_mean'], state[pre + '/moving_variance'], cache[out]['mean'], cache[out]['var'], cnt, decay)
            else:
                env[out] = ops.bn_infer(x, gam, bet, state[pre + '/moving_mean'], state[pre + '/moving_variance'], x.dtype.type(eps))
        elif kind == 'prelu':
            u = env[op[2]]
            env[out] = np.where(u > 0, u, p[op[3]] * u)
        elif kind == 'add':
            env[out] = env[op[2]] + env[op[3]]
        elif kind == 'fc':
            env[out] = ops.fc_fwd(_flat(env[op[2]], data_format), p[op[3]])
        else:
            raise ValueError(kind)
    return env, cache, new_state


def noise_bands(graph, p, images, state=None, data_format='NCHW'):
    """rms(float32 restatement - float64 restatement) of every PReLU's input on THIS input (oracle.graphnet.noise_bands for the
    ReLU nets): the decision band of the kink, from the reference alone"""
    f = lambda d, t: None if d is None else OrderedDict((k, np.asarray(v, t)) for k, v in d.items())
    e64, _, _ = forward(graph, f(p, np.float64), np.asarray(images, np.float64), True, f(state, np.float64), data_format)
    e32, _, _ = forward(graph, f(p, np.float32), np.asarray(images, np.float32), True, f(state, np.float32), data_format)
    return {op[1]: float(np.sqrt(((e32[op[2]].astype(np.float64) - e64[op[2]]) ** 2).mean())) for op in graph if op[0] == 'prelu'}


def noise_bands16(graph, p, images, state=None, data_format='NCHW'):
    """rms(restatement with bf16-rounded MFMA operands - exact restatement) of every PReLU's input: the bf16 mode's decision band
    (oracle.graphnet.noise_bands16)"""
    with ops.operand_rounding('bf16'):
        ea, _, _ = forward(graph, p, images, True, state, data_format)
    with ops.no_rounding():
        eb, _, _ = forward(graph, p, images, True, state, data_format)
    return {op[1]: float(np.sqrt(((ea[op[2]] - eb[op[2]]) ** 2).mean())) for op in graph if op[0] == 'prelu'}


BF16_NOISE_MULT = 4       # oracle.graphnet.BF16_NOISE_MULT


def backward(graph, p, env, cache, dout, kink=None, bands=None, data_format='NCHW', kink_mode='fp32'):
    """dout: {tensor: gradient} -> (parameter gradients, tensor gradients).  kink[prelu out] = the pre-activation u as the
    implementation under test evaluated it: inside max(KINK_BAND * rms(u), NOISE_MULT * bands[out]) -- never a function of the
    implementation's tensors -- the side it took is adopted (u == 0 exactly is not a band element: the convention decides).
    kink_mode 'bf16' (mixed-precision checks): BF16_NOISE_MULT x noise_bands16() instead."""
    mult = {'fp32': NOISE_MULT, 'bf16': BF16_NOISE_MULT}[kink_mode]
    gt, gp = dict(dout), OrderedDict()

    def acc(d, k, v):
        d[k] = v if k not in d else d[k] + v
    for op in reversed(graph):
        kind, out = op[0], op[1]
        if out not in gt:
            continue
        dy = gt[out]
        if kind == 'conv':
            dx, dw = ops.conv2d_bwd(env[op[2]], p[op[3]], dy, op[4], need_dx=op[2] != 'images')
            acc(gp, op[3], dw)
            if dx is not None:
                acc(gt, op[2], dx)
        elif kind == 'bn':
            pre = op[3]
            dx, dg, db = ops.bn_train_bwd(dy, p[pre + '/gamma'], cache[out])
            acc(gp, pre + '/gamma', dg)
            acc(gp, pre + '/beta', db)
            acc(gt, op[2], dx)
        elif kind == 'prelu':
            u, a = env[op[2]], p[op[3]]
            pos = u > 0
            if kink is not None and out in kink:
                thr = max(KINK_BAND * np.sqrt((u * u).mean()), mult * (bands or {}).get(out, 0.0))
                band = (np.abs(u) < thr) & (u != 0)
                pos = np.where(band, kink[out] > 0, pos)
            acc(gt, op[2], dy * np.where(pos, u.dtype.type(1), a * np.ones_like(u)))
            acc(gp, op[3], (dy * np.where(pos, 0, u)).sum(axis=tuple(range(u.ndim - 1))))
        elif kind == 'add':
            acc(gt, op[2], dy)
            acc(gt, op[3], dy)
        elif kind == 'fc':
            x = env[op[2]]
            dx, dw, _ = ops.fc_bwd(_flat(x, data_format), p[op[3]], dy, False)
            acc(gp, op[3], dw)
            acc(gt, op[2], _unflat(dx, x.shape, data_format))
    return gp, gt


def loss_and_grads(graph, p, images, labels, head='softmax', margin=(64.0, 0.5, 0.0), weight_decay=5e-4, state=None, kink=None,
                   bands=None, data_format='NCHW', kink_mode='fp32'):
    """-> ([cross-entropy, reg], gradients incl. wd * w on the filters, env, new moving statistics).  head 'softmax': CE on the
    classifier; 'arcface' / 'cosface': tests/margin_ref.py's additive-margin head (S, m, m3) on the features and the classifier."""
    env, cache, new_state = forward(graph, p, images, True, state, data_format)
    if head == 'softmax':
        ce, dlogits = ops.softmax_ce(env['logits'], labels)
        gp, gt = backward(graph, p, env, cache, {'logits': dlogits}, kink, bands, data_format, kink_mode)
    else:
        import margin_ref as mr
        ce, f, dx, dw = mr.head_fwd_bwd(env['features'], p[CLS], labels, *margin)
        env['logits'] = f
        gp, gt = backward(graph[:-1], p, env, cache, {'features': dx.astype(images.dtype)}, kink, bands, data_format, kink_mode)
        gp[CLS] = dw.astype(images.dtype)
    reg_names = [k for k in p if k.endswith('weights')]
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        gp[k] = gp[k] + weight_decay * p[k]
    env['tensor_grads'] = gt                              # gradient of the loss with respect to every tensor, by tensor name
    return [float(ce), reg], gp, env, new_state


def loss_only(graph, p, images, labels, head='softmax', margin=(64.0, 0.5, 0.0), weight_decay=5e-4, data_format='NCHW'):
    """the total loss straight from the forward pass (for central differences)"""
    env, _, _ = forward(graph, p, images, True, None, data_format)
    if head == 'softmax':
        ce, _ = ops.softmax_ce(env['logits'], labels)
    else:
        import margin_ref as mr
        ce = mr.loss_only(env['features'], p[CLS], labels, *margin)
    return float(ce) + ops.l2_reg([p[k] for k in p if k.endswith('weights')], weight_decay)


# ------------------------------------------------------------------------------------------------------------------------
# the fused BN + PReLU kernels (fte.h "BN + PReLU") on [rows, c]
# ------------------------------------------------------------------------------------------------------------------------
# (rows, c, splits of the launcher's plan): the four shapes of the issue -- (1, 64) and (37, 64): one split; (784, 128) and (98, 512):
# several, the last one short -- then several splits with a short last one at c = 256, a ragged last channel block (116 = 29 quads on
# blocks of 16), the 8-quad layout below 32 channels, and a tensor past the apply grid's cap (n4 >= 4 * 512 * 256: four pieces per thread)
KERNEL_CASES = [(1, 64, 1), (37, 64, 1), (784, 128, 12), (98, 512, 3), (1061, 256, 33), (77, 116, 1), (50, 28, 1), (8200, 256, 249)]
ALPHAS = (0.25, 0.0, 1.0, -0.5)
KINK_CAP = 1e-3           # at most 0.1 % of a case's elements may sit in the kink band


def kernel_case(rows, c, alpha=None):
    """float32 inputs of one kernel case.  Channel k has alpha ALPHAS[k % 4] (or the constant `alpha`).  Channels 0 and 3 carry
    scale / shift pairs (0.5, -1) and (0.25, -0.5), exact in fp32, and z = 2 is planted in a few rows there: u == 0 exactly."""
    r = np.random.default_rng(rows * 1000 + c)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    z = f32(r.standard_normal((rows, c)) * 2.0 + 3.0)
    dy = f32(r.standard_normal((rows, c)))
    gamma = f32(1 + 0.2 * r.standard_normal(c))
    beta = f32(0.3 * r.standard_normal(c))
    z64 = z.astype(np.float64)
    mean = f32(z64.mean(0) + (0.1 * r.standard_normal(c) if rows == 1 else 0))      # (one row: z - mean would be 0 everywhere)
    rstd = f32(1.0 / np.sqrt(z64.var(0) + (1.0 if rows == 1 else BN_EPS)))
    scale = f32(gamma.astype(np.float64) * rstd)
    shift = f32(beta.astype(np.float64) - mean.astype(np.float64) * scale)
    scale[0], shift[0] = 0.5, -1.0
    scale[3], shift[3] = 0.25, -0.5
    planted = sorted(set([0, rows // 2, rows - 1]))
    for rr in planted:
        z[rr, 0] = 2.0
        z[rr, 3] = 2.0
    al = f32(np.full(c, alpha)) if alpha is not None else f32([ALPHAS[k % 4] for k in range(c)])
    return dict(rows=rows, c=c, z=z, dy=dy, gamma=gamma, mean=mean, rstd=rstd, scale=scale, shift=shift, alpha=al, planted=planted)


def kernel_ref(case):
    """float64 results on the float32 inputs: y, dz, dgamma, dbeta, dalpha, the sums of the terms' magnitudes, and the kink band mask
    (|u| < KINK_BAND * rms(u), exact zeros not in it)"""
    d = {k: np.asarray(v, np.float64) for k, v in case.items() if isinstance(v, np.ndarray)}
    rows = case['rows']
    u = d['z'] * d['scale'] + d['shift']
    pos = u > 0
    y = np.where(pos, u, d['alpha'] * u)
    g = d['dy'] * np.where(pos, 1.0, d['alpha'])
    xhat = (d['z'] - d['mean']) * d['rstd']
    da_terms = d['dy'] * np.where(pos, 0.0, u)
    dbeta, dgamma, dalpha = g.sum(0), (g * xhat).sum(0), da_terms.sum(0)
    dz = d['gamma'] * d['rstd'] * (g - dbeta / rows - xhat * dgamma / rows)
    band = (np.abs(u) < KINK_BAND * np.sqrt((u * u).mean())) & (u != 0)
    return dict(u=u, y=y, g=g, xhat=xhat, dz=dz, dgamma=dgamma, dbeta=dbeta, dalpha=dalpha, band=band,
                mag_gamma=np.abs(g * xhat).sum(0), mag_beta=np.abs(g).sum(0), mag_alpha=np.abs(da_terms).sum(0),
                max_gamma=np.abs(g * xhat).max(), max_beta=np.abs(g).max(), max_alpha=np.abs(da_terms).max())


def reduce_quads(c):
    """channel quads per block of the backward reduce (csrc/iresnet.hip reduce_quads)"""
    return 64 if c >= 256 else 32 if c >= 128 else 16 if c >= 64 else 8


def split_plan(rows, c, max_splits=512):
    """host mirror of prelu_split (csrc/iresnet.hip; stat_split of layers.hip): (splits, rows per split)"""
    q = reduce_quads(c)
    cb = (c // 4 + q - 1) // q
    lanes = 256 // q
    rs = max(1, min(2048 // cb, rows // (lanes * 8), max_splits))
    rps = (rows + rs - 1) // rs
    return (rows + rps - 1) // rps, rps


def expected_variables(depth, in_ch, num_classes, h, w, blocks=None):
    """[(name, shape)] of the trainable variables and [(name, shape)] of the moving statistics, from the block table alone"""
    blocks = BLOCKS[depth] if blocks is None else list(blocks)
    name = 'IResNet-%d' % depth
    tv, st = [], []

    def bn(scope, c):
        tv.extend([(scope + '/BatchNorm/gamma', (c,)), (scope + '/BatchNorm/beta', (c,))])
        st.extend([(scope + '/BatchNorm/moving_mean', (c,)), (scope + '/BatchNorm/moving_variance', (c,))])
    s = name + '/stem/conv_3x3'
    tv.append((s + '/weights', (3, 3, in_ch, 64)))
    bn(s, 64)
    tv.append((s + '/prelu/alpha', (64,)))
    cin = 64
    for si, (nb, cout) in enumerate(zip(blocks, WIDTHS)):
        for bi in range(nb):
            sc = '%s/stage%d/block_%d' % (name, si + 1, bi)
            if bi == 0:
                tv.append((sc + '/conv_shortcut_1x1/weights', (1, 1, cin, cout)))
                bn(sc + '/conv_shortcut_1x1', cout)
            bn(sc + '/bn1', cin)
            tv.append((sc + '/conv1_3x3/weights', (3, 3, cin, cout)))
            bn(sc + '/conv1_3x3', cout)
            tv.append((sc + '/conv1_3x3/prelu/alpha', (cout,)))
            tv.append((sc + '/conv2_3x3/weights', (3, 3, cout, cout)))
            bn(sc + '/conv2_3x3', cout)
            cin = cout
    bn(name + '/output', 512)
    oh, ow = _out_hw(h, w)
    tv.append((name + '/output/fc/weights', (oh * ow * 512, EMBED)))
    bn(name + '/output/fc', EMBED)
    tv.append((CLS, (EMBED, num_classes)))
    return tv, st
