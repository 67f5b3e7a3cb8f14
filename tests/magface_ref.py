"""Float64 numpy restatement of the MagFace head (Meng et al., CVPR 2021; include/fte.h fte_magface_softmax_fwd_bwd): ArcFace's
target column with the margin of each row a linear function of its clamped norm, the regulariser g per row, the gradient G and
rowcoef WITH the derivative through the norm (the margin is not a constant of the gradient), and its composition with the SphereNet
oracle's backbone (oracle.spherenet.backbone_fwd / backbone_bwd), in the style of tests/margin_ref.py.

The target logit JUMPS where c_iy crosses -cos mu_i (ArcFace's fallback), and the norm gradient jumps where xn_i crosses l_a or
u_a (the clamp's derivative).  gaps() measures the distance of a batch from both in float64: the tests assert it on their inputs."""
from collections import OrderedDict

import numpy as np

from margin_ref import EPS, colcoef_ref
from oracle import ops, spherenet as osn

PRESET = (64.0, 10.0, 110.0, 0.45, 0.8, 35.0)      # S, l_a, u_a, l_m, u_m, lambda_g


def margins(xn, l_a, u_a, l_m, u_m):
    """(a, mu, g, inside, k_m) from the norms xn [n]: the clamped norm, the row's margin, the regulariser, [l_a <= xn <= u_a]"""
    xn = np.asarray(xn, np.float64)
    k_m = (u_m - l_m) / (u_a - l_a)
    a = np.minimum(np.maximum(xn, l_a), u_a)
    return a, l_m + k_m * (a - l_a), a / u_a ** 2 + 1.0 / a, (xn >= l_a) & (xn <= u_a), k_m


def target(c, mu):
    """t, t' = dt/dc and dt/dmu of the target logit, elementwise"""
    c, mu = np.asarray(c, np.float64), np.asarray(mu, np.float64)
    sin_t = np.sqrt(np.maximum((1 - c) * (1 + c), 0))
    cm, sm = np.cos(mu), np.sin(mu)
    arc = c > -cm
    t = np.where(arc, c * cm - sin_t * sm, c - mu * sm)
    tp = np.where(arc, cm + sm * c / np.maximum(sin_t, 1e-6), 1.0)
    tmu = np.where(arc, -(sin_t * cm + c * sm), -(sm + mu * cm))
    return t, tp, tmu


def kernel_ref(s, xn, wn, labels, S, l_a, u_a, l_m, u_m, lambda_g, grad_scale, c=None, parts=False):
    """What the kernel computes from s [n, ld], xn [n], wn [>= c]: (f [n, ld], loss_rows [n], reg_rows [n], G [n, ld], rowcoef [n]).
    Rows with an out-of-range label are NaN (below c).  parts=True: also (the ArcFace-form share of rowcoef, the norm share,
    the sum of the magnitudes of rowcoef's terms)."""
    s = np.asarray(s, np.float64)
    n, ld = s.shape
    c = ld if c is None else c
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)[:c]
    labels = np.asarray(labels)
    a, mu, g, inside, k_m = margins(xn, l_a, u_a, l_m, u_m)
    f, G = np.zeros((n, ld)), np.zeros((n, ld))
    loss, reg, rowcoef = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    arc_part, norm_part, mag = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c:
            f[i, :c] = G[i, :c] = np.nan
            continue
        den = max(xn[i], EPS) * wn
        cos = np.clip(s[i, :c] / den, -1, 1)
        t, tp, tmu = target(cos[y], mu[i])
        z = S * cos
        z[y] = S * t
        zm = z.max()
        e = np.exp(z - zm)
        lse = zm + np.log(e.sum())
        p = e / e.sum()
        dc = p.copy()
        dc[y] = (p[y] - 1) * tp
        dc *= grad_scale * S
        G[i, :c] = dc / den
        f[i, :c] = z
        loss[i] = lse - z[y]
        reg[i] = g[i]
        da = grad_scale * (S * (p[y] - 1) * tmu * k_m + lambda_g * (1 / u_a ** 2 - 1 / a[i] ** 2)) if inside[i] else 0.0
        live = xn[i] > EPS
        arc_part[i] = -(G[i, :c] * s[i, :c]).sum() / xn[i] ** 2 if live else 0.0
        norm_part[i] = da / xn[i] if live else 0.0
        rowcoef[i] = arc_part[i] + norm_part[i]
        if live:
            wgt = p.copy()
            wgt[y] = (p[y] + 1) * abs(tp)
            mag[i] = abs(grad_scale) * S * (wgt * np.abs(cos)).sum() / xn[i] ** 2
            if inside[i]:
                mag[i] += abs(grad_scale) * (S * (p[y] + 1) * abs(tmu) * k_m + lambda_g * (1 / u_a ** 2 + 1 / a[i] ** 2)) / xn[i]
    if parts:
        return f, loss, reg, G, rowcoef, arc_part, norm_part, mag
    return f, loss, reg, G, rowcoef


def gaps(s, xn, wn, labels, l_a, u_a, l_m, u_m, c=None):
    """(min |c_iy + cos mu_i|, min |xn_i - l_a| / l_a, min |xn_i - u_a| / u_a) over the rows with a label in range, float64"""
    s = np.asarray(s, np.float64)
    c = s.shape[1] if c is None else c
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)
    y = np.asarray(labels).astype(int)
    ok = (y >= 0) & (y < c)
    yc = np.clip(y, 0, c - 1)
    idx = np.arange(s.shape[0])
    cy = np.clip(s[idx, yc] / (np.maximum(xn, EPS) * wn[yc]), -1, 1)
    _, mu, _, _, _ = margins(xn, l_a, u_a, l_m, u_m)
    return (np.abs(cy + np.cos(mu))[ok].min(), (np.abs(xn - l_a) / l_a)[ok].min(), (np.abs(xn - u_a) / u_a)[ok].min())


def head_fwd_bwd(x, W, labels, S=PRESET[0], l_a=PRESET[1], u_a=PRESET[2], l_m=PRESET[3], u_m=PRESET[4], lambda_g=PRESET[5],
                 grad_scale=None):
    """the whole head on x [N, D], W [D, C] -> (mean CE, lambda_g * mean g, logits f [N, C], dx, dW of their sum)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n = x.shape[0]
    gs = 1.0 / n if grad_scale is None else grad_scale
    s = x @ W
    xn = np.sqrt((x * x).sum(1))
    wn = np.sqrt((W * W).sum(0))
    f, rows, reg, G, rc = kernel_ref(s, xn, wn, labels, S, l_a, u_a, l_m, u_m, lambda_g, gs)
    cc = colcoef_ref(G, s, wn)
    dx = G @ W.T + rc[:, None] * x
    dW = x.T @ G + cc[None, :] * W
    return rows.mean(), lambda_g * reg.mean(), f, dx, dW


def head_gaps(x, W, labels, l_a, u_a, l_m, u_m):
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    return gaps(x @ W, np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0)), labels, l_a, u_a, l_m, u_m)


def loss_only(x, W, labels, S, l_a, u_a, l_m, u_m, lambda_g):
    """mean CE + lambda_g * mean g, straight from the definition (for finite differences)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    xn = np.sqrt((x * x).sum(1))
    cos = np.clip((x @ W) / np.maximum(xn, EPS)[:, None] / np.sqrt((W * W).sum(0))[None, :], -1, 1)
    _, mu, g, _, _ = margins(xn, l_a, u_a, l_m, u_m)
    idx = np.arange(x.shape[0])
    t, _, _ = target(cos[idx, labels], mu)
    z = S * cos
    z[idx, labels] = S * t
    zm = z.max(1, keepdims=True)
    lse = zm[:, 0] + np.log(np.exp(z - zm).sum(1))
    return (lse - z[idx, labels]).mean() + lambda_g * g.mean()


def loss_and_grads(p, images, labels, hyper=PRESET, weight_decay=5e-4, data_format='NCHW', kink=None, kink_mode='fp32'):
    """oracle.spherenet.loss_and_grads with this head: ([ce, magnitude_loss, reg], grads incl. the L2 term, extras with the gaps)."""
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, mag, logits, demb, dwc = head_fwd_bwd(emb, wc, labels, *hyper)
    noise = osn.bf16_noise(p, images, data_format) if (kink is not None and kink_mode == 'bf16') else None
    g = osn.backbone_bwd(p, cache, demb, None, kink, kink_mode, noise)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, mag, reg], g, dict(embedding=emb, logits=logits, gaps=head_gaps(emb, wc, labels, *hyper[1:5]),
                                   norms=np.sqrt((emb * emb).sum(1)))


def train_step(p, slots, images, labels, lr, hyper=PRESET, weight_decay=5e-4, data_format='NCHW', kink=None):
    """one Momentum step of one tower -> (params, slots, losses, the gaps of the step's batch)"""
    losses, g, ex = loss_and_grads(p, images, labels, hyper, weight_decay, data_format, kink)
    newp, news = OrderedDict(), OrderedDict()
    for k in p:
        newp[k], news[k] = ops.momentum_step(p[k], slots[k], g[k], lr)
    return newp, news, losses, ex['gaps']
