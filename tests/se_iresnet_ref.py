"""float64 restatement of SE-IResNet ("IR-SE": the IResNet block of tests/iresnet_ref.py with a squeeze-and-excitation gate between the
block's last BN and the shortcut add, no activation behind the add) and of the kernels of fte.h "BN + SE + shortcut, no activation",
composed from oracle.ops.  TEST INFRASTRUCTURE: the block table, the variable names and the op list are written from the issue that
introduced the nets, not derived from tf_face_toolbox_amd/nets/iresnet.py -- the tests compare the two.

  block   BN -> conv 3x3 -> BN -> PReLU -> conv 3x3 (stride) -> BN -> SE gate, plus the shortcut (identity, or conv 1x1 (stride) -> BN)
  gate    g = sigmoid(fc2(relu(fc1(mean_hw(y))))), fc1 [c, c / 16] + bias, fc2 [c / 16, c] + bias; the gated tensor is y * g[n, c]

Two kinks: the PReLUs (convention and band of iresnet_ref) and the gate's hidden ReLU, whose band is the same rule applied to its
pre-activation fc1(sq) + b1."""
from collections import OrderedDict

import numpy as np

import iresnet_ref as ir
from iresnet_ref import BLOCKS, WIDTHS, EMBED, BN_EPS, BN_DECAY, KINK_BAND, NOISE_MULT, BF16_NOISE_MULT, CLS, KINK_CAP, _flat, _unflat, _out_hw
from oracle import ops

SE_REDUCTION = 16


def se_iresnet_graph(depth, in_ch, num_classes, h, w, blocks=None):
    """-> (graph, spec, name): iresnet_ref.iresnet_graph with ('se', t/se, t/c2/bn, scope/se) before every block's add"""
    blocks = BLOCKS[depth] if blocks is None else list(blocks)
    name = 'SE-IResNet-%d' % depth
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
            hid = cout // SE_REDUCTION
            spec.extend([(sc + '/se/fc1/weights', (cout, hid), 'fc_w'), (sc + '/se/fc1/biases', (hid,), 'bias'),
                         (sc + '/se/fc2/weights', (hid, cout), 'fc_w'), (sc + '/se/fc2/biases', (cout,), 'bias')])
            g.append(('se', t + '/se', t + '/c2/bn', sc + '/se'))
            g.append(('add', t, t + '/se', shortcut))
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
    """iresnet_ref.init_params; the gate's weights Xavier-uniform, its biases 0"""
    p, state = ir.init_params([e for e in spec if e[2] not in ('fc_w', 'bias')], seed, dtype)
    rng = np.random.default_rng(seed + 1000)
    for name, shape, kind in spec:
        if kind == 'fc_w':
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            p[name] = rng.uniform(-lim, lim, shape).astype(dtype)
        elif kind == 'bias':
            p[name] = np.zeros(shape, dtype)
    return OrderedDict((n, p[n]) for n, _, _ in spec), state


def perturb(p, seed, scale=0.1):
    """iresnet_ref.perturb, and the gate's biases away from 0 (hidden units on both sides of their ReLU)"""
    q = ir.perturb(p, seed, scale)
    rng = np.random.default_rng(seed + 1000)
    for k, v in p.items():
        if k.endswith('/biases'):
            q[k] = (v + 0.3 * rng.standard_normal(v.shape)).astype(v.dtype)
    return q


def forward(graph, p, images, train=True, state=None, data_format='NCHW', eps=BN_EPS, decay=BN_DECAY):
    """-> (env, cache, new moving statistics), in the dtype of its inputs.  cache[se out] = sq, pre (the hidden pre-activation), hid, gate"""
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
        elif kind == 'se':
            x, pre = env[op[2]], op[3]
            sq = x.mean(axis=(1, 2))
            pre1 = ops.mfma_matmul(sq, p[pre + '/fc1/weights']) + p[pre + '/fc1/biases']
            hid = np.maximum(pre1, 0)
            gate = 1 / (1 + np.exp(-(ops.mfma_matmul(hid, p[pre + '/fc2/weights']) + p[pre + '/fc2/biases'])))
            env[out] = x * gate[:, None, None, :]
            cache[out] = dict(sq=sq, pre=pre1, hid=hid, gate=gate)
        elif kind == 'add':
            env[out] = env[op[2]] + env[op[3]]
        elif kind == 'fc':
            env[out] = ops.fc_fwd(_flat(env[op[2]], data_format), p[op[3]])
        else:
            raise ValueError(kind)
    return env, cache, new_state


def _kink_inputs(graph, env, cache):
    """tensor with a kink -> its pre-activation: the PReLUs' inputs and the gates' hidden pre-activations"""
    d = {op[1]: env[op[2]] for op in graph if op[0] == 'prelu'}
    d.update({op[1]: cache[op[1]]['pre'] for op in graph if op[0] == 'se'})
    return d


def noise_bands(graph, p, images, state=None, data_format='NCHW'):
    """rms(float32 restatement - float64 restatement) of every pre-activation with a kink on THIS input"""
    f = lambda d, t: None if d is None else OrderedDict((k, np.asarray(v, t)) for k, v in d.items())
    e64, c64, _ = forward(graph, f(p, np.float64), np.asarray(images, np.float64), True, f(state, np.float64), data_format)
    e32, c32, _ = forward(graph, f(p, np.float32), np.asarray(images, np.float32), True, f(state, np.float32), data_format)
    a, b = _kink_inputs(graph, e32, c32), _kink_inputs(graph, e64, c64)
    return {k: float(np.sqrt(((a[k].astype(np.float64) - b[k]) ** 2).mean())) for k in b}


def noise_bands16(graph, p, images, state=None, data_format='NCHW'):
    """rms(restatement with bf16-rounded MFMA operands - exact restatement): the bf16 operand mode's decision band"""
    with ops.operand_rounding('bf16'):
        ea, ca, _ = forward(graph, p, images, True, state, data_format)
    with ops.no_rounding():
        eb, cb, _ = forward(graph, p, images, True, state, data_format)
    a, b = _kink_inputs(graph, ea, ca), _kink_inputs(graph, eb, cb)
    return {k: float(np.sqrt(((a[k] - b[k]) ** 2).mean())) for k in b}


def kink_band(u, out, bands=None, mult=NOISE_MULT):
    """the elements of pre-activation u an fp32 evaluation cannot place: |u| < max(KINK_BAND * rms(u), mult * bands[out]), u != 0"""
    thr = max(KINK_BAND * np.sqrt((u * u).mean()), mult * (bands or {}).get(out, 0.0))
    return (np.abs(u) < thr) & (u != 0)


def backward(graph, p, env, cache, dout, kink=None, bands=None, data_format='NCHW', kink_mode='fp32'):
    """iresnet_ref.backward plus the gate.  kink[prelu out] = the engine's pre-activation u, kink[se out] = the engine's hidden
    activations (> 0 where its ReLU passed): inside the band the engine's side is adopted."""
    mult = {'fp32': NOISE_MULT, 'bf16': BF16_NOISE_MULT}[kink_mode]
    gt, gp = dict(dout), OrderedDict()

    def acc(d, k, v):
        d[k] = v if k not in d else d[k] + v

    def side(u, out):
        pos = u > 0
        if kink is not None and out in kink:
            pos = np.where(kink_band(u, out, bands, mult), kink[out] > 0, pos)
        return pos
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
            pos = side(u, out)
            acc(gt, op[2], dy * np.where(pos, u.dtype.type(1), a * np.ones_like(u)))
            acc(gp, op[3], (dy * np.where(pos, 0, u)).sum(axis=tuple(range(u.ndim - 1))))
        elif kind == 'se':
            x, pre, c = env[op[2]], op[3], cache[out]
            hw = x.shape[1] * x.shape[2]
            dpre2 = (dy * x).sum(axis=(1, 2)) * c['gate'] * (1 - c['gate'])
            acc(gp, pre + '/fc2/weights', ops.mfma_matmul(c['hid'].T, dpre2))
            acc(gp, pre + '/fc2/biases', dpre2.sum(0))
            dpre1 = ops.mfma_matmul(dpre2, p[pre + '/fc2/weights'].T) * side(c['pre'], out)
            acc(gp, pre + '/fc1/weights', ops.mfma_matmul(c['sq'].T, dpre1))
            acc(gp, pre + '/fc1/biases', dpre1.sum(0))
            dsq = ops.mfma_matmul(dpre1, p[pre + '/fc1/weights'].T)
            acc(gt, op[2], dy * c['gate'][:, None, None, :] + dsq[:, None, None, :] / hw)
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
    """iresnet_ref.loss_and_grads on this module's forward / backward; env['cache'] holds the gates' intermediates"""
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
    env['tensor_grads'] = gt
    env['cache'] = cache
    return [float(ce), reg], gp, env, new_state


def loss_only(graph, p, images, labels, head='softmax', margin=(64.0, 0.5, 0.0), weight_decay=5e-4, data_format='NCHW'):
    env, _, _ = forward(graph, p, images, True, None, data_format)
    if head == 'softmax':
        ce, _ = ops.softmax_ce(env['logits'], labels)
    else:
        import margin_ref as mr
        ce = mr.loss_only(env['features'], p[CLS], labels, *margin)
    return float(ce) + ops.l2_reg([p[k] for k in p if k.endswith('weights')], weight_decay)


def expected_variables(depth, in_ch, num_classes, h, w, blocks=None):
    """iresnet_ref.expected_variables under the SE- name, plus the four gate variables of every block"""
    blocks = BLOCKS[depth] if blocks is None else list(blocks)
    name = 'SE-IResNet-%d' % depth
    tv, st = ir.expected_variables(depth, in_ch, num_classes, h, w, blocks)
    ren = lambda k: 'SE-' + k if k.startswith('IResNet-') else k
    tv, st = [(ren(k), s) for k, s in tv], [(ren(k), s) for k, s in st]
    for si, (nb, c) in enumerate(zip(blocks, WIDTHS)):
        for bi in range(nb):
            pre = '%s/stage%d/block_%d/se' % (name, si + 1, bi)
            tv.extend([(pre + '/fc1/weights', (c, c // 16)), (pre + '/fc1/biases', (c // 16,)),
                       (pre + '/fc2/weights', (c // 16, c)), (pre + '/fc2/biases', (c,))])
    return tv, st


# ------------------------------------------------------------------------------------------------------------------------
# the kernels of fte.h "BN + SE + shortcut, no activation" on [n, hw, c]
# ------------------------------------------------------------------------------------------------------------------------
MAX_SPLITS = 64


def quads(c):
    """channel quads per block of the two reductions (csrc/iresnet.hip se_lin_quads): the 8-quad layout below 32 channels"""
    return 8 if c < 32 else 16


def split_plan(n, hw, c, cus=256, target=None):
    """host mirror of se_lin_split (csrc/iresnet.hip) -> (S, pixels per split).  cus: compute units of the device; target: blocks wanted
    (FTE_SE_LIN_BLOCKS; default 4 per CU)"""
    q = quads(c)
    base = ((c // 4 + q - 1) // q) * n
    target = 4 * cus if target is None else target
    s = 1 if (4 * base >= target or hw < 64) else (target + base - 1) // base
    s = max(1, min(s, hw // (256 // q), MAX_SPLITS))
    pps = (hw + s - 1) // s
    return (hw + pps - 1) // pps, pps


# (n, hw, c, S on a 256-CU device) -> the launcher branch the case is on (se_lin_split, se_lin_quads, the kernels' walks):
#   S = 1   (2, 1, 4)      one pixel, one quad: 7 of the 8 quads and 31 of the 32 pixel lanes idle
#           (3, 49, 512)   fewer than 64 pixels: never split; eight channel blocks per image
#           (300, 4, 64)   enough images that no split is taken (300 * 4 >= 1024), and fewer than 64 pixels
#           (300, 65, 8)   enough images ALONE: 65 pixels would be split
#           (256, 80, 64)  enough images; 80 pixels = one four-in-flight trip of the 16 pixel lanes and a tail
#           (2, 50, 116)   a ragged second channel block (29 quads on blocks of 16), not split (50 pixels)
#   S > 1   (2, 3136, 64)  capped at MAX_SPLITS = 64: 49 pixels per split, hw < 64 * S (no four-in-flight trip: the tail loop alone), last split full
#           (1, 785, 128)  capped by the pixel lanes (785 / 16 = 49 -> 17 pixels per split -> 47 splits), the last split short: 3 pixels
#           (2, 197, 28)   the 8-quad layout (32 pixel lanes): 6 splits of 33, the last short: 32
#           (2, 130, 116)  ragged second channel block AND split: 8 splits of 17, the last short: 11
#           (64, 1100, 64) 16 splits of 69 pixels: a four-in-flight trip and a tail inside a split; the last split short: 65
# The merge kernels have no lanes over the splits (one thread per image and channel quad adds them in order), so there is no
# "more splits than lanes" branch.
KERNEL_CASES = [(2, 1, 4, 1), (3, 49, 512, 1), (300, 4, 64, 1), (300, 65, 8, 1), (256, 80, 64, 1), (2, 50, 116, 1),
                (2, 3136, 64, 64), (1, 785, 128, 47), (2, 197, 28, 6), (2, 130, 116, 8), (64, 1100, 64, 16)]
_CASES = {}


def kernel_case(n, hw, c):
    """float32 inputs of one kernel case (made once per shape, never modified)"""
    key = (n, hw, c)
    if key not in _CASES:
        r = np.random.default_rng(n * 1000003 + hw * 1009 + c)
        f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
        z = f32(r.standard_normal((n, hw, c)) * 2.0 + 3.0)
        dy = f32(r.standard_normal((n, hw, c)))
        shortcut = f32(r.standard_normal((n, hw, c)))
        gamma = f32(1 + 0.2 * r.standard_normal(c))
        beta = f32(0.3 * r.standard_normal(c))
        z64 = z.astype(np.float64).reshape(-1, c)
        one = z64.shape[0] == 1
        mean = f32(z64.mean(0) + (0.1 * r.standard_normal(c) if one else 0))
        rstd = f32(1.0 / np.sqrt(z64.var(0) + (1.0 if one else BN_EPS)))
        scale = f32(gamma.astype(np.float64) * rstd)
        shift = f32(beta.astype(np.float64) - mean.astype(np.float64) * scale)
        gate = f32(1 / (1 + np.exp(-r.standard_normal((n, c)))))
        _CASES[key] = dict(n=n, hw=hw, c=c, z=z, dy=dy, shortcut=shortcut, gamma=gamma, beta=beta, mean=mean, rstd=rstd, scale=scale,
                           shift=shift, gate=gate)
    return _CASES[key]


def kernel_ref(case):
    """float64 results on the float32 inputs, and the largest term of every [n, c] sum"""
    if 'ref' not in case:
        d = {k: np.asarray(v, np.float64) for k, v in case.items() if isinstance(v, np.ndarray)}
        zm = d['z'].mean(1)
        u = d['z'] * d['scale'] + d['shift']
        xhat = (d['z'] - d['mean']) * d['rstd']
        s1, s2 = d['dy'].sum(1), (d['dy'] * xhat).sum(1)
        case['ref'] = dict(sq=d['scale'] * zm + d['shift'], xm=(zm - d['mean']) * d['rstd'], out=u * d['gate'][:, None, :] + d['shortcut'],
                           bn_res=u + d['shortcut'], s1=s1, s2=s2, dgate=(d['gamma'] * s2 + d['beta'] * s1) * d['gate'] * (1 - d['gate']),
                           max_z=np.abs(d['z']).max(), max_s1=np.abs(d['dy']).max(), max_s2=np.abs(d['dy'] * xhat).max(),
                           max_u=np.abs(d['dy'] * (d['gamma'] * xhat + d['beta'])).max())
    return case['ref']


def block_tail_composed(z, gamma, beta, fc, shortcut, dout, eps=BN_EPS):
    """the block tail BN -> gate -> + shortcut op by op (oracle.ops and this module's 'se'): out and every gradient"""
    g = [('bn', 'y', 'z', 'B'), ('se', 's', 'y', 'S'), ('add', 'out', 's', 'sc')]
    p = {'B/gamma': gamma, 'B/beta': beta, 'S/fc1/weights': fc[0], 'S/fc1/biases': fc[1], 'S/fc2/weights': fc[2], 'S/fc2/biases': fc[3]}
    env, cache = {'z': z, 'sc': shortcut}, {}
    env['y'], cache['y'] = ops.bn_train_fwd(z, gamma, beta, eps)
    x = env['y']
    sq = x.mean(axis=(1, 2))
    pre1 = sq @ fc[0] + fc[1]
    hid = np.maximum(pre1, 0)
    gate = 1 / (1 + np.exp(-(hid @ fc[2] + fc[3])))
    env['s'] = x * gate[:, None, None, :]
    cache['s'] = dict(sq=sq, pre=pre1, hid=hid, gate=gate)
    env['out'] = env['s'] + shortcut
    gp, gt = backward(g, p, env, cache, {'out': dout})
    return env['out'], gp, gt, cache


def block_tail_fused(z, gamma, beta, fc, shortcut, dout, eps=BN_EPS):
    """the same block tail in the arithmetic of the fused plan op: squeeze from z, out = u * gate + shortcut; backward from the
    per-image sums s1 = sum dy, s2 = sum dy * xhat: dgate -> dense layers -> dsq; the BN backward's two sums WITHOUT a pass over the
    tensor, sum dy_bn = sum_n (gate * s1 + dsq), sum dy_bn * xhat = sum_n (gate * s2 + dsq * xm); dz = A dy_bn + B z + C0 with
    dy_bn = dy * gate + dsq / hw (fte_se_bn_bwd_coef / _apply with g = dy)"""
    n, h, w, c = z.shape
    hw, rows = h * w, n * h * w
    mean, var = z.mean(axis=(0, 1, 2)), z.var(axis=(0, 1, 2))
    rstd = 1 / np.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    zm = z.mean(axis=(1, 2))
    sq, xm = scale * zm + shift, (zm - mean) * rstd
    hid = np.maximum(sq @ fc[0] + fc[1], 0)
    gate = 1 / (1 + np.exp(-(hid @ fc[2] + fc[3])))
    out = (z * scale + shift) * gate[:, None, None, :] + shortcut
    xhat = (z - mean) * rstd
    s1, s2 = dout.sum(axis=(1, 2)), (dout * xhat).sum(axis=(1, 2))
    dgate = (gamma * s2 + beta * s1) * gate * (1 - gate)
    dhid = (dgate @ fc[2].T) * (hid > 0)
    dsq = dhid @ fc[0].T
    dbeta, dgamma = (gate * s1 + dsq).sum(0), (gate * s2 + dsq * xm).sum(0)
    A = gamma * rstd
    B = -A * rstd * dgamma / rows
    C0 = -A * dbeta / rows - B * mean
    dz = A * (dout * gate[:, None, None, :] + dsq[:, None, None, :] / hw) + B * z + C0
    gp = {'B/gamma': dgamma, 'B/beta': dbeta, 'S/fc2/weights': hid.T @ dgate, 'S/fc2/biases': dgate.sum(0),
          'S/fc1/weights': sq.T @ dhid, 'S/fc1/biases': dhid.sum(0)}
    return out, gp, {'z': dz, 'sc': dout}


# ------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU audit (tests/test_gpu_se_iresnet.py), shared with the CPU check of their kink bands
# ------------------------------------------------------------------------------------------------------------------------
AUDIT = dict(n=6, h=32, w=24, ncls=7)
AUDIT_SEEDS = (71, 72, 73)        # parameters, perturbation, images / labels: chosen so that the kink bands stay nearly empty (test_se_iresnet_host.py)
_AUDIT = {}


def audit_case(blocks=(1, 1, 1, 1)):
    """graph, spec, parameters, moving statistics, images, labels of the audited net: made once per block table, never modified"""
    key = tuple(blocks)
    if key not in _AUDIT:
        a = AUDIT
        g, spec, _ = se_iresnet_graph(18, 3, a['ncls'], a['h'], a['w'], list(blocks))
        p, state = init_params(spec, AUDIT_SEEDS[0])
        p = perturb(p, AUDIT_SEEDS[1])
        rng = np.random.default_rng(AUDIT_SEEDS[2])
        _AUDIT[key] = (g, spec, p, state, rng.uniform(-1, 1, (a['n'], a['h'], a['w'], 3)), rng.integers(0, a['ncls'], a['n']))
    return _AUDIT[key]


def kink_shares(graph, p, x, state, data_format='NCHW', mode='fp32'):
    """tensor with a kink -> (elements in the audit's band, elements), from the reference alone"""
    bands = (noise_bands if mode == 'fp32' else noise_bands16)(graph, p, x, state, data_format)
    mult = NOISE_MULT if mode == 'fp32' else BF16_NOISE_MULT
    env, cache, _ = forward(graph, p, x, True, state, data_format)
    return {k: (int(kink_band(u, k, bands, mult).sum()), u.size) for k, u in _kink_inputs(graph, env, cache).items()}
