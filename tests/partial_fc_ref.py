"""Numpy restatement of the sampled-class (Partial FC) head, include/fte.h "Partial FC": the sampler in uint32 / uint64 integer
arithmetic, and the head = tests/margin_ref.head_fwd_bwd on the gathered float64 columns, scattered back into the dense gradient."""
import math

import numpy as np

import margin_ref as mr

M32 = np.uint64(0xffffffff)


def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 values held in uint64 (so the products wrap explicitly)"""
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def sample_size(num_classes, rate):
    return min(int(num_classes), int(math.ceil(float(rate) * int(num_classes))))


def sample(labels, num_classes, S, seed, step):
    """-> (index [S] sorted class ids, inverse [C] position or -1, labels_out [n]): the first S classes of the order
    (not in the batch, h_j, j).  A label outside [0, C) takes no part and maps to -1."""
    C = int(num_classes)
    labels = np.asarray(labels, np.int64)
    base = fmix32((fmix32(np.uint64(seed & 0xffffffff)) + np.uint64(step & 0xffffffff)) & M32)
    j = np.arange(C, dtype=np.uint64)
    h = fmix32((j + base) & M32)
    negative = np.ones(C, bool)
    good = labels[(labels >= 0) & (labels < C)]
    negative[good] = False
    order = np.lexsort((j, h, negative))                      # last key first: (negative, h, j)
    index = np.sort(order[:S]).astype(np.int64)
    inverse = np.full(C, -1, np.int64)
    inverse[index] = np.arange(S)
    out = np.full(len(labels), -1, np.int64)
    ok = (labels >= 0) & (labels < C)
    out[ok] = inverse[labels[ok]]
    return index, inverse, out


def head_fwd_bwd(x, W, labels, S, seed, step, scale, m, m3, grad_scale=None):
    """x [N, D], W [D, C] -> (mean loss, logits over the sampled columns [N, S], dx, dense dW [D, C], index)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    index, _, ys = sample(labels, W.shape[1], S, seed, step)
    loss, f, dx, dWs = mr.head_fwd_bwd(x, W[:, index], ys, scale, m, m3, grad_scale)
    dW = np.zeros_like(W)
    dW[:, index] = dWs
    return loss, f, dx, dW, index


def loss_only(x, W, labels, S, seed, step, scale, m, m3):
    index, _, ys = sample(labels, np.asarray(W).shape[1], S, seed, step)
    return mr.loss_only(x, np.asarray(W, np.float64)[:, index], ys, scale, m, m3)


def loss_and_grads(p, images, labels, S, seed, step, scale, m, m3, weight_decay=5e-4, data_format='NCHW', kink=None):
    """margin_ref.loss_and_grads with the head swapped for the sampled one: ([ce, reg], grads incl. the L2 term, extras)"""
    from oracle import ops, spherenet as osn
    emb, cache = osn.backbone_fwd(p, images, data_format)
    wc = p['classifier/fc_classifier/weights']
    ce, logits, demb, dwc, index = head_fwd_bwd(emb, wc, labels, S, seed, step, scale, m, m3)
    g = osn.backbone_bwd(p, cache, demb, None, kink, 'fp32', None)
    g['classifier/fc_classifier/weights'] = dwc
    reg_names = osn.regularized_names(p)
    reg = ops.l2_reg([p[k] for k in reg_names], weight_decay)
    for k in reg_names:
        g[k] = g[k] + weight_decay * p[k]
    return [ce, reg], g, dict(embedding=emb, logits=logits, index=index)


def train_step(p, slots, images, labels, lr, S, seed, step, scale, m, m3, weight_decay=5e-4, data_format='NCHW', kink=None):
    """one Momentum step of one tower; the dense optimizer treats the zero-gradient columns like any other parameter"""
    from collections import OrderedDict
    from oracle import ops
    losses, g, _ = loss_and_grads(p, images, labels, S, seed, step, scale, m, m3, weight_decay, data_format, kink)
    newp, news = OrderedDict(), OrderedDict()
    for k in p:
        newp[k], news[k] = ops.momentum_step(p[k], slots[k], g[k], lr)
    return newp, news, losses
