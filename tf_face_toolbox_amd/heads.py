"""The launch sequence of the heads on the normalised features and classifier columns (A-softmax, ArcFace / CosFace, AdaFace, CurricularFace,
MagFace, the sampled-class form and the K-centre form), written once: loss.py, nets/sphere.py and nets/graph.py (loss_function, backward_head) call it.

Plain functions over buffers the CALLER owns.  `b` is any object that carries them under the nets' attribute names -- a net itself, or
the scratch namespace loss.py allocates per call: xn [n], wn [ld], rowcoef [n], colcoef [ld], G [n, ld], loss_rows [n]; for AdaFace
also adaface_stats [2], a_rows [n], b_rows [n]; for CurricularFace cf_state [1], cf_t [1]; for MagFace reg_rows [n]; for the class sampler class_index [spad],
class_inverse [c], sampled_labels [n],
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
    statistics move under the net's update_moving_stats --, ('curricularface', S, m, alpha, update) -- t moves the same way --,
    ('magface', S, l_a, u_a, l_m, u_m, lambda_g) -- no state -- or (head, S, m, m3) for 'arcface' / 'cosface'."""
    if net.head == 'magface':
        return ('magface', net.margin_scale) + tuple(net.magface)
    if net.head == 'curricularface':
        return ('curricularface', net.margin_scale, net.margin, net.curricular_alpha, int(net.update_moving_stats))
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
    elif head[0] == 'curricularface':    # t from the batch's target cosines, before the logits; then the softmax that re-weights by it
        S, m, alpha, update = head[1:]
        call('fte_curricular_t', s, b.xn, b.wn, labels, alpha, update, b.cf_state, b.cf_t, n, c, ld, st)
        call('fte_curricular_softmax_fwd_bwd', s, b.xn, b.wn, labels, S, m, b.cf_t, *out)
    elif head[0] == 'magface':           # the margin from the row's norm inside the kernel: one launch; the regulariser per row beside the loss
        S, l_a, u_a, l_m, u_m, lambda_g = head[1:]
        call('fte_magface_softmax_fwd_bwd', s, b.xn, b.wn, labels, S, l_a, u_a, l_m, u_m, lambda_g, logits, b.loss_rows, b.reg_rows,
             *out[2:])
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


# ---- the classifier split by class over the ranks (fte.h "Sharded margin head") ----------------------------------------
def shard_range(num_classes, world, rank):
    """Rank `rank` of `world` owns classes [lo, hi): Cs = ceil(C / R) per rank, the last one short.  ValueError for a split that
    would leave a rank without a class (R = 8 over C = 9: Cs = 2, ranks 5..7 would be empty)."""
    C, R, r = int(num_classes), int(world), int(rank)
    if C < 1 or R < 1 or not 0 <= r < R:
        raise ValueError('shard_range: num_classes %d, %d ranks, rank %d' % (C, R, r))
    cs = (C + R - 1) // R
    if (R - 1) * cs >= C:
        raise ValueError('%d classes over %d ranks is %d per rank, which leaves rank %d without a class' % (C, R, cs, (C + cs - 1) // cs))
    return r * cs, min(C, (r + 1) * cs)


def shard_ld(num_classes, world):
    """columns every rank stores: Cs rounded up to 128 (cpad's rule), the same on all ranks"""
    cs = (int(num_classes) + int(world) - 1) // int(world)
    return (cs + 127) // 128 * 128


def check_sharding(head, sample_rate=None, sync_sample=False, sub_centers=1, what='the head'):
    """what the sharded classifier composes with: the dense K = 1 ArcFace / CosFace head.  ValueError names the reason."""
    if head not in ('arcface', 'cosface'):
        raise ValueError('shard_classes needs an ArcFace / CosFace head: %s has %r' % (what, head))
    if sample_rate is not None and float(sample_rate) < 1.0:
        raise ValueError('shard_classes does not compose with the class sampler (sample_rate %g < 1): sampling inside each shard is '
                         'not built yet' % float(sample_rate))
    if sync_sample:
        raise ValueError('shard_classes does not compose with sync_sample: the shared sample is the data-parallel form of the head')
    if int(sub_centers) > 1:
        raise ValueError('shard_classes does not compose with sub_centers = %d > 1: not built yet' % int(sub_centers))


def shard_buffers(b, n, d, world, device):
    """The gather buffers of the sharded head for a local batch of n rows, made once per batch size: b.X [N, d] and b.Y [N] (the
    global batch in rank order), b.shard_stats [3, N], b.all_stats [R, 3, N], b.dX_part [N, d]."""
    N = world * n
    if getattr(b, 'X', None) is not None and b.X.shape == (N, d) and b.all_stats.shape[0] == world:
        return
    f32 = dict(dtype=torch.float32, device=device)
    b.X, b.Y = torch.empty(N, d, **f32), torch.empty(N, dtype=torch.int32, device=device)
    b.shard_stats, b.all_stats = torch.empty(3, N, **f32), torch.empty(world, 3, N, **f32)
    b.dX_part = torch.empty(N, d, **f32)


def sharded_margin_forward(b, x, W, s, labels, logits, head, n, d, class_lo, c, ld, num_classes, comm, grad_scale, ws, wsb, st):
    """The head of one rank that owns classes class_lo .. class_lo + c as the columns W [d, ld]: x [n, d] and the GLOBAL labels [n]
    of this rank's rows are all-gathered into b.X / b.Y (shard_buffers), s [N, ld] = X W, the per-shard statistics, ONE all-gather
    of the [3, N] block, then the gradient kernel and colcoef.  `head` is describe()'s (name, S, m, m3).  Leaves the shard's margin
    logits in `logits` [N, ld] (None: not wanted), the loss of every row of the global batch in b.loss_rows [N] (the same bits on
    every rank), G [N, ld] in b.G, b.rowcoef [N] = this shard's share and b.colcoef [ld], complete.  b.xn / b.loss_rows / b.rowcoef
    are N long, b.wn / b.colcoef ld."""
    call = _lib.call
    R = comm.world_size()
    N = R * n
    S, m, m3 = head[1:4]
    comm.all_gather(b.X, x)
    comm.all_gather(b.Y, labels)
    call('fte_row_norms', b.X, b.xn, N, d, d, st)
    call('fte_col_norms', W, b.wn, d, c, ld, st)
    call('fte_gemm_nn', b.X, W, None, s, N, ld, d, ws, wsb, st)
    call('fte_margin_shard_stats', s, b.xn, b.wn, b.Y, class_lo, num_classes, S, m, m3, b.shard_stats, N, c, ld, st)
    comm.all_gather(b.all_stats, b.shard_stats)
    call('fte_margin_shard_fwd_bwd', s, b.xn, b.wn, b.Y, class_lo, num_classes, S, m, m3, b.all_stats, R, logits, b.loss_rows, b.G,
         b.rowcoef, N, c, ld, grad_scale, st)
    call('fte_asoftmax_colcoef', b.G, s, b.wn, b.colcoef, N, c, ld, st)


def sharded_classifier_dw(b, W, dW, n, d, ld, ws, wsb, st):
    """dW_r [d, ld] = X^T G + colcoef (.) W_r over the N = R n gathered rows: final on the owning rank, never all-reduced"""
    classifier_dw(b, b.X, W, dW, b.X.shape[0], d, ld, ws, wsb, st)


def sharded_classifier_dx(b, W, dx, n, d, ld, comm, ws, wsb, st):
    """dx [n, d] of this rank's rows: dX_part = G W_r^T + rowcoef_part (.) X over all N rows, then a sum reduce-scatter"""
    classifier_dx(b, b.X, W, b.dX_part, b.X.shape[0], d, ld, ws, wsb, st)
    comm.reduce_scatter_sum(dx, b.dX_part)


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
