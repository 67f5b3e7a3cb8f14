"""Float64 numpy restatement of the sub-center ArcFace head (include/fte.h fte_subcenter_margin_softmax_fwd_bwd /
fte_subcenter_colcoef: the pool over K centres with the lowest-k tie rule, margin, loss, G, rowcoef, colcoef), of the assignment
(fte_subcenter_assign) and of the cleaning decision (tf_face_toolbox_amd/subcenter.py), and the head's composition with the
SphereNet oracle's backbone.  Planar layout: centre k of class j at column k * ld + j."""
import numpy as np

import margin_ref as mr
from oracle import ops, spherenet as osn

EPS = 1e-12


def plane_cos(s, xn, wn, K, c, ld):
    """cos [n, K, c] and den [n, K, c] = max(xn, eps) * wn of the live columns of every plane"""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    sp = s.reshape(n, K, ld)[:, :, :c]
    den = np.maximum(np.asarray(xn, np.float64), EPS)[:, None, None] * np.asarray(wn, np.float64).reshape(K, ld)[None, :, :c]
    return np.clip(sp / den, -1, 1), den


def pool(cos):
    """cos [..., K, c] -> (max over K, the LOWEST k attaining it): numpy's argmax returns the first maximal index"""
    return cos.max(-2), cos.argmax(-2)


def gaps(cos):
    """top-two gap of every (row, class) pair [n, c]; +inf for K = 1"""
    if cos.shape[-2] == 1:
        return np.full(cos.shape[:-2] + cos.shape[-1:], np.inf)
    top = np.sort(cos, axis=-2)
    return top[..., -1, :] - top[..., -2, :]


def kernel_ref(s, xn, wn, labels, K, scale, m, m3, grad_scale, c, ld):
    """s [n, K * ld], xn [n], wn [K * ld] -> (f [n, ld], loss_rows [n], G [n, K * ld], rowcoef [n]); rows with an out-of-range label
    are NaN below c in every plane"""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    xn = np.asarray(xn, np.float64)
    labels = np.asarray(labels)
    cos, den = plane_cos(s, xn, wn, K, c, ld)
    sp = s.reshape(n, K, ld)
    f, G = np.zeros((n, ld)), np.zeros((n, K, ld))
    loss, rowcoef = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c:
            f[i, :c] = np.nan
            G[i, :, :c] = np.nan
            continue
        cmax, kst = pool(cos[i])
        t, tp = mr.target(cmax[y], m, m3)
        z = scale * cmax
        z[y] = scale * t
        zm = z.max()
        e = np.exp(z - zm)
        lse = zm + np.log(e.sum())
        p = e / e.sum()
        dc = p.copy()
        dc[y] = (p[y] - 1) * tp
        dc *= grad_scale * scale
        for k in range(K):
            G[i, k, :c] = np.where(kst == k, dc / den[i, k], 0.0)
        f[i, :c] = z
        loss[i] = lse - z[y]
        rowcoef[i] = -(G[i, :, :c] * sp[i, :, :c]).reshape(-1).sum() / xn[i] ** 2 if xn[i] > EPS else 0.0
    return f, loss, G.reshape(n, K * ld), rowcoef


def colcoef_ref(G, s, wn, K, c, ld):
    """[K * ld]: -sum_i G s / wn^2 in the live columns of every plane, 0 in every plane's pads"""
    G, s = np.asarray(G, np.float64), np.asarray(s, np.float64)
    n = s.shape[0]
    G, s, wn = G.reshape(n, K, ld), s.reshape(n, K, ld), np.asarray(wn, np.float64).reshape(K, ld)
    out = np.zeros((K, ld))
    for k in range(K):
        out[k, :c] = -(G[:, k, :c] * s[:, k, :c]).sum(0) / wn[k, :c] ** 2
    return out.reshape(-1)


def head_fwd_bwd(x, W, labels, K, scale, m, m3, grad_scale=None):
    """x [N, D], W [D, K * C] (planes packed: ld = C) -> (mean loss, f [N, C], dx, dW) of the mean loss, through both normalisations"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n, C = x.shape[0], W.shape[1] // K
    gs = 1.0 / n if grad_scale is None else grad_scale
    s = x @ W
    xn = np.sqrt((x * x).sum(1))
    wn = np.sqrt((W * W).sum(0))
    f, rows, G, rc = kernel_ref(s, xn, wn, labels, K, scale, m, m3, gs, C, C)
    cc = colcoef_ref(G, s, wn, K, C, C)
    return rows.mean(), f, G @ W.T + rc[:, None] * x, x.T @ G + cc[None, :] * W


def loss_only(x, W, labels, K, scale, m, m3):
    """the mean loss alone, straight from the definition (for finite differences)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n, C = x.shape[0], W.shape[1] // K
    xn = np.maximum(np.sqrt((x * x).sum(1)), EPS)
    cos = np.clip((x @ W) / xn[:, None] / np.sqrt((W * W).sum(0))[None, :], -1, 1).reshape(n, K, C).max(1)
    z = scale * cos
    idx = np.arange(n)
    t, _ = mr.target(cos[idx, labels], m, m3)
    z[idx, labels] = scale * t
    zm = z.max(1, keepdims=True)
    return ((zm[:, 0] + np.log(np.exp(z - zm).sum(1))) - z[idx, labels]).mean()


def loss_and_grads(p, images, labels, K, scale, m, m3, weight_decay=5e-4, data_format='NCHW', kink=None):
    """margin_ref.loss_and_grads with K centres per class; p's classifier is [D, K * C], planes packed"""
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, logits, demb, dwc = head_fwd_bwd(emb, wc, labels, K, scale, m, m3)
    g = osn.backbone_bwd(p, cache, demb, None, kink, 'fp32', None)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, reg], g, dict(embedding=emb, logits=logits)


# ---- the cleaning pass ----------------------------------------------------------------------------------------------------------------
def assign_ref(x, Wt, labels, K, c):
    """x [n, d], Wt [K * c, d] -> (sel [n], cosv [K, n], gap [n]): the cosines to the K centres of the sample's own class, the arg-max
    (lowest k on a tie), the top-two gap; a bad label gives -1 / NaN"""
    x, Wt = np.asarray(x, np.float64), np.asarray(Wt, np.float64)
    n = x.shape[0]
    sel, cosv, gap = np.full(n, -1), np.full((K, n), np.nan), np.full(n, np.inf)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < c:
            continue
        w = Wt[np.arange(K) * c + y]
        cosv[:, i] = np.clip((w @ x[i]) / (max(np.sqrt((x[i] * x[i]).sum()), EPS) * np.maximum(np.sqrt((w * w).sum(1)), EPS)), -1, 1)
        sel[i] = cosv[:, i].argmax()
        if K > 1:
            top = np.sort(cosv[:, i])
            gap[i] = top[-1] - top[-2]
    return sel, cosv, gap


def clean_ref(sel, cosv, labels, K, C, angle_deg):
    """-> (dominant [C], keep [n] bool, kept [C], dropped [C], non_dominant): the dominant centre is the one most samples of the class
    select (lowest k on a tie, 0 for an empty class); kept iff cos to it >= fp32(cos(angle))"""
    sel, labels = np.asarray(sel), np.asarray(labels)
    counts = np.zeros((C, K), np.int64)
    ok = sel >= 0
    np.add.at(counts, (labels[ok], sel[ok]), 1)
    dominant = counts.argmax(1)
    thr = np.float32(np.cos(np.deg2rad(np.float64(angle_deg))))
    keep = np.zeros(len(sel), bool)
    idx = np.nonzero(ok)[0]
    keep[idx] = np.asarray(cosv, np.float32)[dominant[labels[idx]], idx] >= thr
    kept = np.bincount(labels[keep], minlength=C)
    dropped = np.bincount(labels[ok], minlength=C) - kept
    return dominant, keep, kept, dropped, int((sel[idx] != dominant[labels[idx]]).sum())


def packed_to_planar(W, K, ld):
    """[D, K * C] planes packed -> [D, K * ld] planar with zero pads"""
    W = np.asarray(W)
    d, C = W.shape[0], W.shape[1] // K
    out = np.zeros((d, K, ld), W.dtype)
    out[:, :, :C] = W.reshape(d, K, C)
    return out.reshape(d, K * ld)

