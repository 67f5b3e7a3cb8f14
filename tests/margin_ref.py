"""Float64 numpy restatement of the additive-margin softmax head (ArcFace / CosFace, include/fte.h
fte_margin_softmax_fwd_bwd), head only, and its composition with the SphereNet oracle's backbone
(oracle.spherenet.backbone_fwd / backbone_bwd) for the whole-net checks."""
from collections import OrderedDict

import numpy as np

from oracle import ops, spherenet as osn

EPS = 1e-12


def target(c, m, m3):
    """t(c) and t'(c) of the target logit, elementwise"""
    c = np.asarray(c, np.float64)
    if m == 0:
        return c - m3, np.ones_like(c)
    sin_t = np.sqrt(np.maximum((1 - c) * (1 + c), 0))
    arc = c > np.cos(np.pi - m)
    t = np.where(arc, c * np.cos(m) - sin_t * np.sin(m) - m3, c - m * np.sin(m) - m3)
    tp = np.where(arc, np.cos(m) + np.sin(m) * c / np.maximum(sin_t, 1e-6), 1.0)
    return t, tp


def kernel_ref(s, xn, wn, labels, scale, m, m3, grad_scale, c=None):
    """What the kernel computes from s [n, ld], xn [n], wn [>= c]: (f [n, ld], loss_rows [n], G [n, ld], rowcoef [n]).
    Rows with an out-of-range label are NaN (below c)."""
    s = np.asarray(s, np.float64)
    n, ld = s.shape
    c = ld if c is None else c
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)[:c]
    labels = np.asarray(labels)
    f, G = np.zeros((n, ld)), np.zeros((n, ld))
    loss, rowcoef = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c:
            f[i, :c] = G[i, :c] = np.nan
            continue
        den = max(xn[i], EPS) * wn
        cos = np.clip(s[i, :c] / den, -1, 1)
        t, tp = target(cos[y], m, m3)
        z = scale * cos
        z[y] = scale * t
        zm = z.max()
        e = np.exp(z - zm)
        lse = zm + np.log(e.sum())
        p = e / e.sum()
        dc = p.copy()
        dc[y] = (p[y] - 1) * tp
        dc *= grad_scale * scale
        G[i, :c] = dc / den
        f[i, :c] = z
        loss[i] = lse - z[y]
        rowcoef[i] = -(G[i, :c] * s[i, :c]).sum() / xn[i] ** 2 if xn[i] > EPS else 0.0
    return f, loss, G, rowcoef


def colcoef_ref(G, s, wn, c=None):
    G, s = np.asarray(G, np.float64), np.asarray(s, np.float64)
    c = s.shape[1] if c is None else c
    out = np.zeros(s.shape[1])
    out[:c] = -(G[:, :c] * s[:, :c]).sum(0) / np.asarray(wn, np.float64)[:c] ** 2
    return out


def head_fwd_bwd(x, W, labels, scale, m, m3, grad_scale=None):
    """x [N, D], W [D, C] -> (mean loss, logits f [N, C], dx, dW) of the mean loss (grad_scale default 1/N)."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n = x.shape[0]
    gs = 1.0 / n if grad_scale is None else grad_scale
    s = x @ W
    xn = np.sqrt((x * x).sum(1))
    wn = np.sqrt((W * W).sum(0))
    f, rows, G, rc = kernel_ref(s, xn, wn, labels, scale, m, m3, gs)
    cc = colcoef_ref(G, s, wn)
    dx = G @ W.T + rc[:, None] * x
    dW = x.T @ G + cc[None, :] * W
    return rows.mean(), f, dx, dW


def loss_only(x, W, labels, scale, m, m3):
    """the mean loss alone, straight from the definition (for finite differences)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    xn = np.maximum(np.sqrt((x * x).sum(1)), EPS)
    cos = np.clip((x @ W) / xn[:, None] / np.sqrt((W * W).sum(0))[None, :], -1, 1)
    z = scale * cos
    idx = np.arange(x.shape[0])
    t, _ = target(cos[idx, labels], m, m3)
    z[idx, labels] = scale * t
    zm = z.max(1, keepdims=True)
    lse = zm[:, 0] + np.log(np.exp(z - zm).sum(1))
    return (lse - z[idx, labels]).mean()


def loss_and_grads(p, images, labels, scale, m, m3, weight_decay=5e-4, data_format='NCHW', kink=None, kink_mode='fp32'):
    """oracle.spherenet.loss_and_grads with this head: ([ce, reg], grads incl. the L2 term, extras)."""
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, logits, demb, dwc = head_fwd_bwd(emb, wc, labels, scale, m, m3)
    noise = osn.bf16_noise(p, images, data_format) if (kink is not None and kink_mode == 'bf16') else None
    g = osn.backbone_bwd(p, cache, demb, None, kink, kink_mode, noise)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, reg], g, dict(embedding=emb, logits=logits)


def train_step(p, slots, images, labels, lr, scale, m, m3, weight_decay=5e-4, data_format='NCHW', kink=None):
    """one Momentum step of one tower (oracle.spherenet.train_step with this head)"""
    losses, g, _ = loss_and_grads(p, images, labels, scale, m, m3, weight_decay, data_format, kink)
    newp, news = OrderedDict(), OrderedDict()
    for k in p:
        newp[k], news[k] = ops.momentum_step(p[k], slots[k], g[k], lr)
    return newp, news, losses
