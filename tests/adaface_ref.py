"""Float64 numpy restatement of the AdaFace head (Kim et al., CVPR 2022; include/fte.h fte_adaface_margins and
fte_margin_softmax_rows_fwd_bwd): the margins from the norms with their running statistics, the per-row-margin softmax head with
its exact gradient through both normalisations, and its composition with the SphereNet oracle's backbone
(oracle.spherenet.backbone_fwd / backbone_bwd) for the whole-net checks, in the style of tests/margin_ref.py."""
from collections import OrderedDict

import numpy as np

from margin_ref import EPS, colcoef_ref
from oracle import ops, spherenet as osn

CLIP = 1e-3                      # E: theta' is clipped to [E, pi - E]
STATS_INIT = (20.0, 100.0)       # the running (mean, std) of the norms before the first step
PRESET = (64.0, 0.4, 0.333, 0.01)      # S, m, h, t_alpha


def margins(xn, stats, m, h, t_alpha):
    """-> (a [n], b [n], (mu, sd)): the per-row margins and the blended statistics they were computed with (what an updating call
    leaves in `stats`)"""
    q = np.clip(np.asarray(xn, np.float64), 1e-3, 100.0)
    n = q.shape[0]
    mean_b = q.sum() / n
    std_b = np.sqrt(((q - mean_b) ** 2).sum() / (n - 1))
    mu = t_alpha * mean_b + (1 - t_alpha) * float(stats[0])
    sd = t_alpha * std_b + (1 - t_alpha) * float(stats[1])
    k = np.clip((q - mu) / (sd + 1e-3) * h, -1.0, 1.0)
    return -m * k, m + m * k, (mu, sd)


def target(c, a, b):
    """t(c) and t'(c) of the target logit for margins a, b (elementwise); t' = 0 where the clip of theta' binds"""
    c, a, b = np.asarray(c, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    th = np.arccos(c) + a
    thc = np.clip(th, CLIP, np.pi - CLIP)
    inside = (th >= CLIP) & (th <= np.pi - CLIP)
    sin_t = np.sqrt(np.maximum((1 - c) * (1 + c), 0))
    t = np.cos(thc) - b
    tp = np.where(inside, np.sin(thc) / np.maximum(sin_t, 1e-6), 0.0)
    return t, tp


def kernel_ref(s, xn, wn, labels, scale, a_rows, b_rows, grad_scale, c=None):
    """What the kernel computes from s [n, ld], xn [n], wn [>= c] and the margins: (f [n, ld], loss_rows [n], G [n, ld],
    rowcoef [n]).  Rows with an out-of-range label or a non-finite margin are NaN (below c)."""
    s = np.asarray(s, np.float64)
    n, ld = s.shape
    c = ld if c is None else c
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)[:c]
    labels = np.asarray(labels)
    f, G = np.zeros((n, ld)), np.zeros((n, ld))
    loss, rowcoef = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c or not (np.isfinite(a_rows[i]) and np.isfinite(b_rows[i])):
            f[i, :c] = G[i, :c] = np.nan
            continue
        den = max(xn[i], EPS) * wn
        cos = np.clip(s[i, :c] / den, -1, 1)
        t, tp = target(cos[y], a_rows[i], b_rows[i])
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


def rows_head_fwd_bwd(x, W, labels, a_rows, b_rows, scale, grad_scale=None):
    """x [N, D], W [D, C] and given margins -> (mean loss, logits f [N, C], dx, dW) of the mean loss (grad_scale default 1/N)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n = x.shape[0]
    gs = 1.0 / n if grad_scale is None else grad_scale
    s = x @ W
    xn = np.sqrt((x * x).sum(1))
    wn = np.sqrt((W * W).sum(0))
    f, rows, G, rc = kernel_ref(s, xn, wn, labels, scale, a_rows, b_rows, gs)
    cc = colcoef_ref(G, s, wn)
    dx = G @ W.T + rc[:, None] * x
    dW = x.T @ G + cc[None, :] * W
    return rows.mean(), f, dx, dW


def head_fwd_bwd(x, W, labels, stats, scale=PRESET[0], m=PRESET[1], h=PRESET[2], t_alpha=PRESET[3], grad_scale=None):
    """the whole head: margins from the norms of x and `stats`, then rows_head_fwd_bwd.  -> (mean loss, f, dx, dW, (mu, sd)); the
    norms enter the margins as constants (no gradient through k_i)"""
    x = np.asarray(x, np.float64)
    a, b, new = margins(np.sqrt((x * x).sum(1)), stats, m, h, t_alpha)
    return rows_head_fwd_bwd(x, W, labels, a, b, scale, grad_scale) + (new,)


def loss_and_grads(p, images, labels, stats, scale=PRESET[0], m=PRESET[1], h=PRESET[2], t_alpha=PRESET[3], weight_decay=5e-4,
                   data_format='NCHW', kink=None, kink_mode='fp32'):
    """oracle.spherenet.loss_and_grads with this head: ([ce, reg], grads incl. the L2 term, extras with the new statistics)."""
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, logits, demb, dwc, new = head_fwd_bwd(emb, wc, labels, stats, scale, m, h, t_alpha)
    noise = osn.bf16_noise(p, images, data_format) if (kink is not None and kink_mode == 'bf16') else None
    g = osn.backbone_bwd(p, cache, demb, None, kink, kink_mode, noise)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, reg], g, dict(embedding=emb, logits=logits, stats=new)


def train_step(p, slots, stats, images, labels, lr, scale=PRESET[0], m=PRESET[1], h=PRESET[2], t_alpha=PRESET[3], weight_decay=5e-4,
               data_format='NCHW', kink=None):
    """one Momentum step of one tower -> (params, slots, stats, losses)"""
    losses, g, ex = loss_and_grads(p, images, labels, stats, scale, m, h, t_alpha, weight_decay, data_format, kink)
    newp, news = OrderedDict(), OrderedDict()
    for k in p:
        newp[k], news[k] = ops.momentum_step(p[k], slots[k], g[k], lr)
    return newp, news, ex['stats'], losses
