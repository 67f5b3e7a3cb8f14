"""Float64 numpy restatement of the CurricularFace head (Huang et al., CVPR 2020; include/fte.h fte_curricular_t and
fte_curricular_softmax_fwd_bwd): the running mean t of the target cosines, the softmax head with ArcFace's target column and the
hard negatives re-weighted by t, its exact gradient through both normalisations (t and the mask are constants), and its composition
with the SphereNet oracle's backbone (oracle.spherenet.backbone_fwd / backbone_bwd), in the style of tests/margin_ref.py.

The logit JUMPS at the mask boundary c_ij = u_i by S c (t + c - 1).  kernel_ref therefore takes an optional explicit mask `hard`
[n, c] (bool): the tests pass the device's side for the few pairs whose float64 distance to the boundary is below what fp32 resolves."""
from collections import OrderedDict

import numpy as np

from margin_ref import EPS, colcoef_ref, target
from oracle import ops, spherenet as osn

T_INIT = 0.0
PRESET = (64.0, 0.5, 0.01)       # S, m, alpha
STATE = ('classifier/curricularface/t',)


def cosines(s, xn, wn, c=None):
    """c_ij [n, c] of the contract from s [n, ld], xn [n], wn [>= c]"""
    s = np.asarray(s, np.float64)
    c = s.shape[1] if c is None else c
    den = np.maximum(np.asarray(xn, np.float64), EPS)[:, None] * np.asarray(wn, np.float64)[None, :c]
    return np.clip(s[:, :c] / den, -1, 1)


def threshold(cy, m):
    """u = cos(theta_y + m) from the target cosine, on both sides of ArcFace's fallback"""
    cy = np.asarray(cy, np.float64)
    return cy * np.cos(m) - np.sqrt(np.maximum((1 - cy) * (1 + cy), 0)) * np.sin(m)


def t_update(t, cy, alpha, valid=None):
    """t after one training forward: alpha * mean(c_iy over the valid rows) + (1 - alpha) * t; unchanged when no row is valid"""
    cy = np.asarray(cy, np.float64)
    valid = np.ones(cy.shape, bool) if valid is None else np.asarray(valid, bool)
    if not valid.any():
        return float(t)
    return alpha * cy[valid].sum() / valid.sum() + (1 - alpha) * float(t)


def kernel_ref(s, xn, wn, labels, S, m, t, grad_scale, c=None, hard=None):
    """What the kernel computes from s [n, ld], xn [n], wn [>= c] and the scalar t: (f [n, ld], loss_rows [n], G [n, ld],
    rowcoef [n]).  `hard` [n, c] bool replaces the mask c_ij > u_i (its target column is ignored).  Rows with an out-of-range label
    are NaN (below c)."""
    s = np.asarray(s, np.float64)
    n, ld = s.shape
    c = ld if c is None else c
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)[:c]
    labels = np.asarray(labels)
    t = float(t)
    f, G = np.zeros((n, ld)), np.zeros((n, ld))
    loss, rowcoef = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c:
            f[i, :c] = G[i, :c] = np.nan
            continue
        den = max(xn[i], EPS) * wn
        cos = np.clip(s[i, :c] / den, -1, 1)
        ty, tp = target(cos[y], m, 0.0)
        mask = cos > threshold(cos[y], m) if hard is None else np.asarray(hard[i], bool).copy()
        mask[y] = False
        z = S * np.where(mask, cos * (t + cos), cos)
        dz = np.where(mask, t + 2 * cos, 1.0)                       # (dz/dc) / S
        z[y] = S * ty
        dz[y] = tp
        zm = z.max()
        e = np.exp(z - zm)
        lse = zm + np.log(e.sum())
        p = e / e.sum()
        dc = p.copy()
        dc[y] = p[y] - 1
        dc *= grad_scale * S * dz
        G[i, :c] = dc / den
        f[i, :c] = z
        loss[i] = lse - z[y]
        rowcoef[i] = -(G[i, :c] * s[i, :c]).sum() / xn[i] ** 2 if xn[i] > EPS else 0.0
    return f, loss, G, rowcoef


def boundary_gap(s, xn, wn, labels, m, c=None):
    """|c_ij - u_i| [n, c] in float64, +inf on the target column and on rows with an out-of-range label"""
    cos = cosines(s, xn, wn, c)
    n, c = cos.shape
    y = np.asarray(labels).astype(int)
    ok = (y >= 0) & (y < c)
    yc = np.clip(y, 0, c - 1)
    gap = np.abs(cos - threshold(cos[np.arange(n), yc], m)[:, None])
    gap[np.arange(n), yc] = np.inf
    gap[~ok] = np.inf
    return gap


def head_fwd_bwd(x, W, labels, t, S=PRESET[0], m=PRESET[1], alpha=PRESET[2], update=True, grad_scale=None, hard=None):
    """the whole head on x [N, D], W [D, C]: t moved by the batch's target cosines first (update), then the softmax with it.
    -> (mean loss, logits f [N, C], dx, dW, t used)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n = x.shape[0]
    gs = 1.0 / n if grad_scale is None else grad_scale
    s = x @ W
    xn = np.sqrt((x * x).sum(1))
    wn = np.sqrt((W * W).sum(0))
    y = np.asarray(labels).astype(int)
    valid = (y >= 0) & (y < W.shape[1])
    cy = cosines(s, xn, wn)[np.arange(n), np.clip(y, 0, W.shape[1] - 1)]
    t = t_update(t, cy, alpha, valid) if update else float(t)
    f, rows, G, rc = kernel_ref(s, xn, wn, labels, S, m, t, gs, hard=hard)
    cc = colcoef_ref(G, s, wn)
    dx = G @ W.T + rc[:, None] * x
    dW = x.T @ G + cc[None, :] * W
    return rows.mean(), f, dx, dW, t


def head_gap(x, W, labels, m):
    """min |c_ij - u_i| of the head on (x, W): the whole-net tests assert it is far above what fp32 resolves"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    return boundary_gap(x @ W, np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0)), labels, m).min()


def loss_and_grads(p, images, labels, t, S=PRESET[0], m=PRESET[1], alpha=PRESET[2], weight_decay=5e-4, data_format='NCHW',
                   kink=None, kink_mode='fp32', update=True):
    """oracle.spherenet.loss_and_grads with this head: ([ce, reg], grads incl. the L2 term, extras with t and the boundary gap)."""
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, logits, demb, dwc, new = head_fwd_bwd(emb, wc, labels, t, S, m, alpha, update)
    noise = osn.bf16_noise(p, images, data_format) if (kink is not None and kink_mode == 'bf16') else None
    g = osn.backbone_bwd(p, cache, demb, None, kink, kink_mode, noise)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, reg], g, dict(embedding=emb, logits=logits, t=new, gap=head_gap(emb, wc, labels, m))


def train_step(p, slots, t, images, labels, lr, S=PRESET[0], m=PRESET[1], alpha=PRESET[2], weight_decay=5e-4, data_format='NCHW',
               kink=None):
    """one Momentum step of one tower -> (params, slots, t, losses, boundary gap of the step)"""
    losses, g, ex = loss_and_grads(p, images, labels, t, S, m, alpha, weight_decay, data_format, kink)
    newp, news = OrderedDict(), OrderedDict()
    for k in p:
        newp[k], news[k] = ops.momentum_step(p[k], slots[k], g[k], lr)
    return newp, news, ex['t'], losses, ex['gap']
