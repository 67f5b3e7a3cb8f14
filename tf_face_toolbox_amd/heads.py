"""The launch sequence of the heads on the normalised features and classifier columns (A-softmax, ArcFace / CosFace, AdaFace, the
sampled-class form and the K-centre form), written once: loss.py, nets/sphere.py and nets/graph.py (loss_function, backward_head) call it.

Plain functions over buffers the CALLER owns.  `b` is any object that carries them under the nets' attribute names -- a net itself, or
the scratch namespace loss.py allocates per call: xn [n], wn [ld], rowcoef [n], colcoef [ld], G [n, ld], loss_rows [n]; for AdaFace
also adaface_stats [2], a_rows [n], b_rows [n]; for the class sampler class_index [spad], class_inverse [c], sampled_labels [n],
Ws [d, spad]; with K > 1 centres per class (planar layout, fte.h "Sub-center ArcFace") wn, colcoef and the columns of G are K * ld.
Nothing here allocates on a step (the sampler's all-gather pair is made once per batch size).  Every launch goes
through `_lib.call`, looked up when it is made: the launch recorder and tests/step_audit.py swap it.

The gradient contract (fte.h): G = dLoss/ds feeds the classifier's two products, and the two normalisations add
dW += colcoef (.) W and dx += rowcoef (.) x, so the gradient is exact through both; the margin is not applied under no_grad."""
import torch

from . import _lib


def check_labels(labels):
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32):
        raise TypeError('labels must be an int32 CUDA tensor (data.py:259)')
    return labels.contiguous()


def describe(net):
    """The head description margin_forward takes, from a margin net's attributes: ('adaface', S, m, h, t_alpha, update) -- the running
    statistics move under the net's update_moving_stats -- or (head, S, m, m3) for 'arcface' / 'cosface'."""
    if net.head == 'adaface':
        return ('adaface', net.margin_scale, net.margin, net.adaface_h, net.adaface_t_alpha, int(net.update_moving_stats))
    K = int(getattr(net, 'sub_centers', 1))
    if K > 1:                            # K centres per class: the count rides behind (S, m, m3); K = 1 is today's tuple
        return (net.head, net.margin_scale, net.margin, net.margin_cos, K)
    return (net.head, net.margin_scale, net.margin, net.margin_cos)


SUB_CENTERS_MAX = 8


def check_sub_centers(K, head='arcface', sample_rate=None, what='the head'):
    """The centre count of a net or a loss call -> int K.  ValueError for K outside 1..8 and, with K > 1, for every head but ArcFace /
    CosFace and for the class sampler (the per-plane gather / scatter the planar layout prepares is not built: DESIGN.md 9)."""
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= SUB_CENTERS_MAX:
        raise ValueError('sub_centers must be an integer in 1..%d (got %r)' % (SUB_CENTERS_MAX, K))
    K = int(K)
    if K > 1 and head not in ('arcface', 'cosface'):
        raise ValueError('sub_centers = %d needs an ArcFace / CosFace head: %s has %r' % (K, what, head))
    if K > 1 and sample_rate is not None and float(sample_rate) < 1.0:
        raise ValueError('sub_centers = %d does not compose with the class sampler (sample_rate %g < 1): not built yet' % (K, sample_rate))
    return K


def margin_forward(b, x, W, s, labels, logits, head, n, d, c, ld, grad_scale, st):
    """From the features x [n, d], the classifier columns in use W [d, ld] (c live ones) and their raw product s [n, ld]: the norms,
    the margin kernel of `head` -- ('asoftmax', lambda), describe()'s tuples -- and colcoef.  A describe() tuple that ends in K > 1:
    W, s, b.G are K * ld wide, b.wn / b.colcoef K * ld long, c and ld describe ONE plane and `logits` is [n, ld].  Leaves the margin logits in `logits`
    (None: not wanted), the loss per row in b.loss_rows, G = grad_scale * dLoss/ds in b.G, and rowcoef / colcoef for the backward."""
    call = _lib.call
    if head[0] in ('arcface', 'cosface') and len(head) == 5:      # K centres per class
        S, m, m3, K = head[1:]
        call('fte_row_norms', x, b.xn, n, d, d, st)
        call('fte_col_norms', W, b.wn, d, K * ld, K * ld, st)       # the pads of every plane are zero columns: wn = 0, never read
        call('fte_subcenter_margin_softmax_fwd_bwd', s, b.xn, b.wn, labels, K, S, m, m3, logits, b.loss_rows, b.G, b.rowcoef, n, c, ld,
             grad_scale, st)
        call('fte_subcenter_colcoef', b.G, s, b.wn, b.colcoef, K, n, c, ld, st)
        return
    call('fte_row_norms', x, b.xn, n, d, d, st)
    call('fte_col_norms', W, b.wn, d, c, ld, st)
    out = (logits, b.loss_rows, b.G, b.rowcoef, n, c, ld, grad_scale, st)
    if head[0] == 'asoftmax':
        call('fte_asoftmax_fwd_bwd', s, b.xn, b.wn, labels, head[1], *out)
    elif head[0] == 'adaface':           # per-row margins from the norms, then the additive-margin softmax with a margin pair per row
        S, m, h, t_alpha, update = head[1:]
        call('fte_adaface_margins', b.xn, n, m, h, t_alpha, update, b.adaface_stats, b.a_rows, b.b_rows, st)
        call('fte_margin_softmax_rows_fwd_bwd', s, b.xn, b.wn, labels, S, b.a_rows, b.b_rows, *out)
    else:                                # (S, m, m3): ArcFace / CosFace
        call('fte_margin_softmax_fwd_bwd', s, b.xn, b.wn, labels, *(head[1:] + out))
    call('fte_asoftmax_colcoef', b.G, s, b.wn, b.colcoef, n, c, ld, st)


def sample_classes(b, labels, W, n, d, c, ld, S, spad, seed, step, ws, wsb, st, comm=None):
    """The sampled-class head's step before the dense one (fte.h "Partial FC"): S of the c classes under (seed, step) into
    b.class_index / b.class_inverse, the remapped labels into b.sampled_labels, the sampled columns of W [d, ld] into b.Ws [d, spad].
    After it the head is the dense head on (b.Ws, S, spad, b.sampled_labels).  With `comm` the ranks sample as one: the labels of the
    global batch, in rank order, go through the unchanged sampler, and a rank's own remapped labels are its rows of the result."""
    call = _lib.call
    world, every, mine = 1, labels, b.sampled_labels
    if comm is not None:
        world = comm.world_size()
        if getattr(b, '_all_labels', None) is None or b._all_labels.numel() != world * n:
            b._all_labels = torch.empty(world * n, dtype=torch.int32, device=labels.device)
            b._all_sampled = torch.empty(world * n, dtype=torch.int32, device=labels.device)
        comm.all_gather(b._all_labels, labels)
        every, mine = b._all_labels, b._all_sampled
    call('fte_pfc_sample', every, world * n, c, S, int(seed) & 0xffffffff, int(step) & 0xffffffff, b.class_index, b.class_inverse, mine,
         ws, wsb, st)
    if comm is not None:
        r = comm.rank()
        b.sampled_labels = mine[r * n:(r + 1) * n]
    call('fte_pfc_gather_cols', W, b.class_index, b.Ws, d, c, ld, S, spad, st)


def classifier_dw(b, x, W, dW, n, d, ld, ws, wsb, st, norm=True):
    """dW [d, ld] = x^T G (+ colcoef (.) W on the same stream; norm=False: the plain softmax / focal heads, which share the product)"""
    _lib.call('fte_gemm_tn', x, b.G, dW, n, ld, d, ws, wsb, st)
    if norm:
        _lib.call('fte_add_scaled_rows_cols', dW, W, None, b.colcoef, d, ld, ld, st)


def classifier_dx(b, x, W, dx, n, d, ld, ws, wsb, st, norm=True):
    """dx [n, d] = G W^T (+ rowcoef (.) x); a workspace and stream of its own: the graph nets run classifier_dw beside it"""
    _lib.call('fte_gemm_nt', b.G, W, None, None, 0, None, dx, None, n, ld, d, ws, wsb, st)
    if norm:
        _lib.call('fte_add_scaled_rows_cols', dx, x, b.rowcoef, None, n, d, d, st)
