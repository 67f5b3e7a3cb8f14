"""Host-side mirror of the reference's loss.py: focal_loss (:18-27), center_loss (:29-45), batch_hard_triplet_loss
(:47-78) on libfte.so, plus additive_margin_loss (ArcFace / CosFace; not in the reference), its K-centre form subcenter_margin_loss, its sampled-class form partial_fc_margin_loss and adaface_loss (the margin per row from the feature norms), curricularface_loss and magface_loss (the margin a function of the feature norm AND part of the gradient).  Same names, argument meaning and defaults.  There is no autograd here, so every function
also returns the gradient of ITS OWN loss value with respect to its first argument (what tf.gradients would have
produced for that term); the graph nets wire them as heads (nets/graph.py), a caller can combine them freely.

All tensors are float32 / int32 CUDA tensors; logits may carry padding columns (ld = logits.shape[1] >= num_classes)."""
import math
from types import SimpleNamespace

import torch

from . import _lib, heads


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(t, dtype, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
        raise TypeError('%s must be a %s CUDA tensor' % (what, dtype))
    return t.contiguous()


def _scaled_sum(rows, scale):
    """0-d tensor scale * sum(rows) on the library's ordered two-stage reduction (no ATen kernel on the step)"""
    out = torch.empty(1, dtype=torch.float32, device=rows.device)
    ws = torch.empty(2048, dtype=torch.float32, device=rows.device)
    _lib.call('fte_sum', rows, rows.numel(), float(scale), out, ws, ws.numel() * 4, _stream())
    return out[0]


def focal_loss(logits, labels, gamma=1.0, alpha=2.0, num_classes=None):
    """mean_i gamma * (1 - p_y)^alpha * CE_i (loss.py:18-27; the reference's parameter names are kept as written).
    -> (loss [0-d], dlogits [N, ld])"""
    logits, labels = _check(logits, torch.float32, 'logits'), _check(labels, torch.int32, 'labels')
    n, ld = logits.shape
    c = ld if num_classes is None else int(num_classes)
    rows = torch.empty(n, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits)
    _lib.call('fte_focal_loss_fwd_bwd', logits, labels, rows, d, n, c, ld, float(gamma), float(alpha), 1.0 / n, _stream())
    return _scaled_sum(rows, 1.0 / n), d


def center_loss(features, labels, num_classes, alpha=0.99, weight=1.0, centers=None):
    """loss.py:29-45.  `centers` [num_classes, D] is the non-trainable variable the reference creates with zeros
    (:34-35); pass the tensor to keep state across calls, it is updated in place (scatter_sub of (1-alpha)(c_y - f),
    duplicates accumulate, no count normalisation).  -> (center_loss_mean, centers, dfeatures) where dfeatures is the
    gradient of weight * center_loss_mean (the term the reference adds to the 'losses' collection, :43)."""
    features, labels = _check(features, torch.float32, 'features'), _check(labels, torch.int32, 'labels')
    n, d = features.shape
    if centers is None:
        centers = torch.zeros(int(num_classes), d, dtype=torch.float32, device=features.device)
    rows = torch.empty(n, dtype=torch.float32, device=features.device)
    df = torch.empty_like(features)
    ws = torch.empty(max(n * d, 1024) + 1024, dtype=torch.float32, device=features.device)
    _lib.call('fte_center_loss_fwd_bwd_update', features, labels, centers, rows, df, n, d, int(centers.shape[0]), float(alpha),
              float(weight) / (n * d), ws, ws.numel() * 4, _stream())
    return _scaled_sum(rows, 1.0 / (n * d)), centers, df


def batch_hard_triplet_loss(features, labels, margin=None, metric='euclidean'):
    """loss.py:47-78: per-sample batch-hard triplet loss (UNREDUCED, as the reference returns it): softplus(pos - neg)
    for margin None, else max(0, pos - neg + margin).  -> (diff [N], dfeatures of mean(diff)).
    `metric` is accepted and IGNORED, as in the reference: loss.py:65 calls `cdist(features, features)` without forwarding it, so
    every value gives the euclidean distance sqrt(sum d^2 + 1e-12) of loss.py:57."""
    features, labels = _check(features, torch.float32, 'features'), _check(labels, torch.int32, 'labels')
    n, d = features.shape
    rows = torch.empty(n, dtype=torch.float32, device=features.device)
    df = torch.empty_like(features)
    ws = torch.empty(max(4 * n * n, 1024) + 1024, dtype=torch.float32, device=features.device)
    _lib.call('fte_batch_hard_triplet_fwd_bwd', features, labels, 0.0 if margin is None else float(margin), int(margin is None), 1.0 / n,
              rows, df, n, d, ws, ws.numel() * 4, _stream())
    return rows, df


def _head_args(features, weights, labels, num_classes):
    """the checked arguments of a margin head and its sizes -> (features, weights, labels, n, d, ld, c)"""
    features, labels = _check(features, torch.float32, 'features'), _check(labels, torch.int32, 'labels')
    weights = _check(weights, torch.float32, 'weights')
    n, d = features.shape
    ld = weights.shape[1]
    if weights.shape[0] != d or labels.shape != (n,):
        raise ValueError('features [N, D], weights [D, ld] and labels [N] do not fit: %s %s %s'
                         % (tuple(features.shape), tuple(weights.shape), tuple(labels.shape)))
    return features, weights, labels, n, d, ld, ld if num_classes is None else int(num_classes)


def _head_scratch(features, n, d, ld, ws_bytes=0, **more):
    """workspace, stream and the scratch buffers of one head call over ld columns, under the names heads.py reads"""
    f32 = dict(dtype=torch.float32, device=features.device)
    ws = torch.empty(max(_lib.query('fte_gemm_ws_bytes', n, ld, d), ws_bytes, 4096) // 4 + 1024, **f32)
    return SimpleNamespace(st=_stream(), ws=ws, wsb=ws.numel() * 4, s=torch.empty(n, ld, **f32), G=torch.empty(n, ld, **f32),
                           xn=torch.empty(n, **f32), rowcoef=torch.empty(n, **f32), loss_rows=torch.empty(n, **f32),
                           wn=torch.empty(ld, **f32), colcoef=torch.empty(ld, **f32), dx=torch.empty_like(features), **more)


def _head_run(b, features, W, dW, labels, head, n, d, c, ld, after_dw=None):
    """the head `head` (heads.margin_forward) on the columns W [d, ld] and both classifier gradients -> (mean loss, dfeatures)"""
    _lib.call('fte_gemm_nn', features, W, None, b.s, n, ld, d, b.ws, b.wsb, b.st)
    heads.margin_forward(b, features, W, b.s, labels, None, head, n, d, c, ld, 1.0 / n, b.st)
    heads.classifier_dw(b, features, W, dW, n, d, ld, b.ws, b.wsb, b.st)
    if after_dw is not None:
        after_dw()
    heads.classifier_dx(b, features, W, b.dx, n, d, ld, b.ws, b.wsb, b.st)
    return _scaled_sum(b.loss_rows, 1.0 / n), b.dx


def additive_margin_loss(features, weights, labels, scale=64.0, margin=0.5, margin_cos=0.0, num_classes=None):
    """Additive-margin softmax on the normalised features and weight columns: ArcFace (angular margin `margin`, cos(theta + m))
    and CosFace (cosine margin `margin_cos`, cos(theta) - m3), scale S = `scale`; the contract is fte.h's
    fte_margin_softmax_fwd_bwd.  ArcFace: scale=64, margin=0.5, margin_cos=0; CosFace: scale=64, margin=0, margin_cos=0.35.
    features [N, D], weights [D, ld] (columns num_classes..ld-1 are padding, default num_classes = ld), labels [N] int32;
    D % 64 == 0 and ld % 64 == 0 (the classifier products' tiling: pad with zero columns).
    -> (loss [0-d] = mean over the rows, dfeatures [N, D], dweights [D, ld]): the exact gradient of the mean through both
    normalisations; padding columns get 0."""
    features, weights, labels, n, d, ld, c = _head_args(features, weights, labels, num_classes)
    dw = torch.empty_like(weights)
    head = ('arcface', float(scale), float(margin), float(margin_cos))
    return _head_run(_head_scratch(features, n, d, ld), features, weights, dw, labels, head, n, d, c, ld) + (dw,)


def sharded_margin_loss(features, weights_shard, labels, class_lo, num_classes, comm, scale=64.0, margin=0.5, margin_cos=0.0):
    """additive_margin_loss with the classifier split by class over the ranks of `comm` (fte.h "Sharded margin head"): this rank
    holds weights_shard [D, ld], the columns of classes class_lo .. (heads.shard_range gives the range of a rank; columns past the
    range's length are padding), features [n, D] and labels [n] are this rank's rows of the global batch and the labels are GLOBAL
    class ids.  Does the all-gathers and the reduce-scatter itself: `comm` has world_size / rank / all_gather / reduce_scatter_sum
    (data_parallel._HostComm).  Every rank must call it.
    -> (loss [0-d] = the mean over the GLOBAL batch, the same on every rank, dfeatures [n, D], dweights_shard [D, ld]): the exact
    gradient of that mean; dweights_shard is final on this rank, it is not to be all-reduced."""
    features, labels = _check(features, torch.float32, 'features'), _check(labels, torch.int32, 'labels')
    W = _check(weights_shard, torch.float32, 'weights_shard')
    n, d = features.shape
    ld = W.shape[1]
    R, C = comm.world_size(), int(num_classes)
    lo, hi = heads.shard_range(C, R, comm.rank())
    if int(class_lo) != lo:
        raise ValueError('rank %d of %d owns classes [%d, %d) of %d, not a shard that starts at %d' % (comm.rank(), R, lo, hi, C, class_lo))
    c = hi - lo
    if W.shape[0] != d or labels.shape != (n,) or ld < c:
        raise ValueError('features [n, D], weights_shard [D, ld >= %d] and labels [n] do not fit: %s %s %s'
                         % (c, tuple(features.shape), tuple(W.shape), tuple(labels.shape)))
    N = R * n
    b = _head_scratch(features, N, d, ld)
    heads.shard_buffers(b, n, d, R, features.device)
    dW, dx = torch.empty_like(W), torch.empty_like(features)
    head = ('arcface', float(scale), float(margin), float(margin_cos))
    heads.sharded_margin_forward(b, features, W, b.s, labels, None, head, n, d, lo, c, ld, C, comm, 1.0 / N, b.ws, b.wsb, b.st)
    heads.sharded_classifier_dw(b, W, dW, n, d, ld, b.ws, b.wsb, b.st)
    heads.sharded_classifier_dx(b, W, dx, n, d, ld, comm, b.ws, b.wsb, b.st)
    return _scaled_sum(b.loss_rows, 1.0 / N), dx, dW


def subcenter_margin_loss(features, weights, labels, K, scale=64.0, margin=0.5, margin_cos=0.0, num_classes=None):
    """additive_margin_loss with K centres per class (sub-center ArcFace, Deng et al. 2020): the class cosine is the max over its K
    centres, the lowest k on a tie, and only the winning centre of a (row, class) pair takes its gradient; the contract is fte.h's
    fte_subcenter_margin_softmax_fwd_bwd.  weights [D, K * ld] is planar: centre k of class j is column k * ld + j, columns
    num_classes..ld-1 of every plane are padding (default num_classes = ld); D % 64 == 0 and ld % 64 == 0.  K in 1..8; K = 1 is
    additive_margin_loss itself (the same calls, bit-identical).  The other arguments and the result (loss, dfeatures [N, D],
    dweights [D, K * ld]) are additive_margin_loss's."""
    K = heads.check_sub_centers(K)
    if K == 1:
        return additive_margin_loss(features, weights, labels, scale, margin, margin_cos, num_classes)
    features, weights, labels, n, d, wide, c = _head_args(features, weights, labels, None)
    if wide % K:
        raise ValueError('weights [D, K * ld] with K = %d: %d columns do not divide' % (K, wide))
    ld = wide // K
    c = ld if num_classes is None else int(num_classes)
    dw = torch.empty_like(weights)
    b = _head_scratch(features, n, d, wide)
    head = ('arcface', float(scale), float(margin), float(margin_cos), K)
    _lib.call('fte_gemm_nn', features, weights, None, b.s, n, wide, d, b.ws, b.wsb, b.st)
    heads.margin_forward(b, features, weights, b.s, labels, None, head, n, d, c, ld, 1.0 / n, b.st)
    heads.classifier_dw(b, features, weights, dw, n, d, wide, b.ws, b.wsb, b.st)
    heads.classifier_dx(b, features, weights, b.dx, n, d, wide, b.ws, b.wsb, b.st)
    return _scaled_sum(b.loss_rows, 1.0 / n), b.dx, dw


def adaface_loss(features, weights, labels, stats, scale=64.0, margin=0.4, h=0.333, t_alpha=0.01, update=True, num_classes=None):
    """AdaFace (Kim et al., CVPR 2022): additive_margin_loss with the margin of each row set from the norm of its feature vector against
    running statistics of the norms; the contract is fte.h's fte_adaface_margins / fte_margin_softmax_rows_fwd_bwd.  `stats` is the
    float32 CUDA tensor [mean, std] (the paper's code starts it at [20, 100]); with `update` it is moved in place by the batch's
    statistics (weight t_alpha), otherwise left alone -- the margins use the blended values either way.  The other arguments, the
    shapes and the result (loss, dfeatures, dweights) are additive_margin_loss's; the norm enters the margins as a constant."""
    if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2):
        raise TypeError('stats must be a contiguous float32 CUDA tensor of 2 elements [mean, std]')
    features, weights, labels, n, d, ld, c = _head_args(features, weights, labels, num_classes)
    rows = dict(dtype=torch.float32, device=features.device)
    b = _head_scratch(features, n, d, ld, adaface_stats=stats, a_rows=torch.empty(n, **rows), b_rows=torch.empty(n, **rows))
    dw = torch.empty_like(weights)
    head = ('adaface', float(scale), float(margin), float(h), float(t_alpha), int(bool(update)))
    return _head_run(b, features, weights, dw, labels, head, n, d, c, ld) + (dw,)


def curricularface_loss(features, weights, labels, t, scale=64.0, margin=0.5, alpha=0.01, update=True, num_classes=None):
    """CurricularFace (Huang et al., CVPR 2020): ArcFace's target logit, and every negative column whose cosine exceeds the margined
    target cosine re-weighted by t + cos; the contract is fte.h's fte_curricular_t / fte_curricular_softmax_fwd_bwd.  `t` is the
    float32 CUDA tensor [1] (the paper's code starts it at 0); with `update` it is moved in place towards the mean target cosine of
    the batch (weight alpha) BEFORE the logits are formed, otherwise it is used as it stands and left alone.  The other arguments,
    the shapes and the result (loss, dfeatures, dweights) are additive_margin_loss's; t and the mask enter the gradient as constants."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 1):
        raise TypeError('t must be a contiguous float32 CUDA tensor of 1 element')
    features, weights, labels, n, d, ld, c = _head_args(features, weights, labels, num_classes)
    b = _head_scratch(features, n, d, ld, cf_state=t, cf_t=torch.empty(1, dtype=torch.float32, device=features.device))
    dw = torch.empty_like(weights)
    head = ('curricularface', float(scale), float(margin), float(alpha), int(bool(update)))
    return _head_run(b, features, weights, dw, labels, head, n, d, c, ld) + (dw,)


def magface_loss(features, weights, labels, scale=64.0, l_a=10.0, u_a=110.0, l_m=0.45, u_m=0.8, lambda_g=35.0, num_classes=None):
    """MagFace (Meng et al., CVPR 2021): ArcFace's target logit with the margin of each row a linear function of the clamped norm a
    of its feature vector, mu = l_m + (u_m - l_m) (a - l_a) / (u_a - l_a), plus the regulariser g(a) = a / u_a^2 + 1 / a with weight
    lambda_g; the contract is fte.h's fte_magface_softmax_fwd_bwd.  The margin and g are part of the gradient: dfeatures carries the
    derivative through the norm.  The other arguments and the shapes are additive_margin_loss's.
    -> (loss [0-d] = mean CE + lambda_g * mean g, dfeatures [N, D], dweights [D, ld], magnitude_loss [0-d] = lambda_g * mean g)."""
    from .nets.net_base import magface_params
    head = ('magface',) + magface_params(scale, l_a, u_a, l_m, u_m, lambda_g)
    features, weights, labels, n, d, ld, c = _head_args(features, weights, labels, num_classes)
    b = _head_scratch(features, n, d, ld, reg_rows=torch.empty(n, dtype=torch.float32, device=features.device))
    dw = torch.empty_like(weights)
    ce, dx = _head_run(b, features, weights, dw, labels, head, n, d, c, ld)
    mag = _scaled_sum(b.reg_rows, head[6] / n)
    return ce + mag, dx, dw, mag


def sample_size(num_classes, sample_rate):
    """S = ceil(sample_rate * num_classes) of the sampled-class head (fte.h "Partial FC"); None or a rate of 1 = every class."""
    c = int(num_classes)
    if sample_rate is None:
        return c
    r = float(sample_rate)
    if not 0.0 < r <= 1.0:
        raise ValueError('sample_rate must lie in (0, 1] (got %r)' % (sample_rate,))
    return min(c, int(math.ceil(r * c)))


def partial_fc_margin_loss(features, weights, labels, sample_rate, seed, step, scale=64.0, margin=0.5, margin_cos=0.0, num_classes=None):
    """additive_margin_loss over a per-step sample of the classes (Partial FC): the batch's own classes plus the other classes with
    the smallest hashes under (seed, step), S = ceil(sample_rate * num_classes) in all; the contract is fte.h's "Partial FC".
    Arguments as additive_margin_loss; `seed` / `step` are taken modulo 2^32.
    -> (loss, dfeatures [N, D], dweights [D, ld], index [S] int32): the sampled classes in ascending order; dweights is the dense
    gradient, exactly 0.0 in every column outside `index`.  sample_rate None or 1 is additive_margin_loss itself (the same calls,
    bit-identical; index = every class).  S < N raises ValueError: with S >= N all of a batch's classes always fit."""
    ld = weights.shape[1]
    c = ld if num_classes is None else int(num_classes)
    S = sample_size(c, sample_rate)
    if S >= c:
        loss, dx, dw = additive_margin_loss(features, weights, labels, scale, margin, margin_cos, num_classes)
        return loss, dx, dw, torch.arange(c, dtype=torch.int32, device=weights.device)
    features, weights, labels, n, d, ld, c = _head_args(features, weights, labels, num_classes)
    if S < n:
        raise ValueError('the sample of %d classes (sample_rate %g of %d) is smaller than the batch of %d rows' % (S, sample_rate, c, n))
    spad = (S + 63) // 64 * 64
    f32, i32 = dict(dtype=torch.float32, device=features.device), dict(dtype=torch.int32, device=features.device)
    b = _head_scratch(features, n, d, spad, _lib.query('fte_pfc_sample_ws_bytes', c), class_index=torch.empty(spad, **i32),
                      class_inverse=torch.empty(c, **i32), sampled_labels=torch.empty(n, **i32), Ws=torch.empty(d, spad, **f32))
    dWs, dw = torch.empty(d, spad, **f32), torch.empty_like(weights)
    heads.sample_classes(b, labels, weights, n, d, c, ld, S, spad, seed, step, b.ws, b.wsb, b.st)
    loss, dx = _head_run(b, features, b.Ws, dWs, b.sampled_labels, ('arcface', float(scale), float(margin), float(margin_cos)), n, d, S, spad,
                         lambda: _lib.call('fte_pfc_scatter_cols', dWs, b.class_inverse, dw, d, c, ld, S, spad, b.st))
    return loss, dx, dw, b.class_index[:S]
