"""Parallel training-step builders: host-side mirror of the reference's data_parallel.py.

Reference: data_parallel.py:24-79 (Singular), :81-166 (DataParallel), :168-256
(DataParallel_margin).  Same constructor arguments and the same call protocol

    train_ops, losses, losses_name, others = wrapper(inputs)

with inputs = {'images', 'labels', 'num_classes', 'num_examples'} (data.py:275-279).
`train_ops` is a callable: one call = one `sess.run(train_ops)` of the reference
(train.py:228) = forward + loss + backward + gradient all-reduce + optimizer + global_step++.
`losses` are 0-d device tensors that hold the last step's values (reading one synchronises).

MI355X-first differences, all deliberate:
  * one PROCESS per GPU (torch.distributed, backend 'nccl' == RCCL over xGMI) instead of
    in-graph towers: `num_gpus` must equal the world size; rank r takes rows
    [r*B/n, (r+1)*B/n) of the global batch (tf.split, data_parallel.py:206-207);
  * gradients live in one flat arena and are summed by ONE bucketed all-reduce per step
    (head bucket first, launched while the conv backward still runs) instead of one
    nccl.all_sum per variable (data_parallel.py:179); the 1/num_gpus factor of :37 is
    folded into the loss-head gradient; the two displayed losses ride on the last bucket
    (data_parallel.py:248);
  * the initial replica sync of train.py:101-120 is one broadcast of the parameter arena;
  * one fused optimizer launch per decay group on the arena (data_parallel.py:186-196).
"""
from collections import OrderedDict

import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _DeviceOptimizer(object):
    """tf.train.MomentumOptimizer(lr, 0.9) / AdamOptimizer(lr, beta1=0.5, beta2=0.999)
    (data_parallel.py:65-69,191-196) as fused launches over the arena."""

    def __init__(self, model, optimizer):
        if optimizer not in ('Momentum', 'Adam'):
            raise ValueError('Unsupported optimizer.')
        self.kind = optimizer
        self.model = model
        self.slots = None

    def _ensure(self):
        if self.slots is None:
            n = self.model.arena_size
            dev = self.model.params.device
            self.slots = [torch.zeros(n, dtype=torch.float32, device=dev)
                          for _ in range(1 if self.kind == 'Momentum' else 2)]

    supports_ranges = True

    def apply(self, lr, step_1based, mult_lr_list, lo=None, hi=None):
        """Update the arena (or only its [lo, hi) part: one all-reduce bucket at a time)."""
        self._ensure()
        m = self.model
        st = _stream()
        for a, b, decayed, grp in m.arena_groups():
            if lo is not None:
                a, b = max(a, lo), min(b, hi)
                if a >= b:
                    continue
            wd = m.weight_decay if decayed else 0.0
            gs = float(mult_lr_list[grp])
            if self.kind == 'Momentum':
                _lib.call('fte_momentum_update', m.params[a:b], self.slots[0][a:b], m.grads[a:b], b - a,
                          float(lr), 0.9, wd * gs, gs, st)
            else:
                _lib.call('fte_adam_update', m.params[a:b], self.slots[0][a:b], self.slots[1][a:b], m.grads[a:b],
                          b - a, float(lr), 0.5, 0.999, 1e-8, wd * gs, gs, int(step_1based), st)


class _HostComm(object):
    """The collective layer the wrappers talk to: torch.distributed (RCCL on GPUs, gloo in the
    CPU tests).  Kept tiny so that tests can drive the bucket logic without a GPU."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group

    def world_size(self):
        return self.dist.get_world_size(self.group)

    def rank(self):
        return self.dist.get_rank(self.group)

    def all_reduce_async(self, t):
        return self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)

    def broadcast(self, t, src=0):
        self.dist.broadcast(t, src=src, group=self.group)

    def all_gather(self, out, t):
        """out [world * len(t)] <- every rank's t, in rank order (the center loss's opt-in reconciliation).  Tensors of more
        dimensions go as their flat views (out is contiguous, [world, *t.shape] or the rows of the ranks one after another): gloo
        takes no stacked output shape."""
        self.dist.all_gather_into_tensor(out.view(-1), t.contiguous().view(-1), group=self.group)

    def reduce_scatter_sum(self, out, inp):
        """out [len(inp) / world] <- this rank's rows of the sum of every rank's inp (the sharded head's dx, heads.py).  RCCL has the
        collective; gloo has none, so there it is an all-reduce of inp IN PLACE followed by a copy of the rank's rows."""
        if self.dist.get_backend(self.group) == 'nccl':
            self.dist.reduce_scatter_tensor(out, inp, op=self.dist.ReduceOp.SUM, group=self.group)
            return
        self.dist.all_reduce(inp, op=self.dist.ReduceOp.SUM, group=self.group)
        rows = out.shape[0]
        out.copy_(inp[self.rank() * rows:(self.rank() + 1) * rows])


def check_shard_classes(model, sync_sample=False):
    """ValueError, with the reason, for every net and head option the sharded classifier does not compose with -- before anything is
    built or communicated."""
    from . import heads
    name = getattr(model, 'name', type(model).__name__)
    if not hasattr(model, 'shard_comm'):
        raise ValueError('shard_classes: %s (%s, head %r) has no sharded classifier: only SphereNet-ArcFace / SphereNet-CosFace do (not the '
                         'A-softmax and AdaFace nets, not the graph nets)' % (name, type(model).__name__, getattr(model, 'head', None)))
    heads.check_sharding(model.head, model.sample_rate, sync_sample, model.sub_centers, name)
    if getattr(model, 'built', False) and getattr(model, 'shard', None) is None:
        raise ValueError('shard_classes: %s was already built with the dense classifier; pass a net that has not been built' % name)


class Singular(object):
    """data_parallel.py:24-79."""

    def __init__(self, model, lr, optimizer, weight_decay=5e-4):
        self.model = model
        self.lr = lr                    # float, or callable(global_step) -> float  (train.py:122-144)
        self.optimizer = optimizer
        self.weight_decay = weight_decay
        self.num_gpus = 1
        self.global_step = 0
        self.pretrained_param = []
        self._opt = None
        self.learning_rate = None

    # -- pieces shared with the multi-GPU wrappers ------------------------------------------------
    def _fetch(self, inputs):
        images, labels = inputs['images'], inputs['labels']
        if callable(images):
            images = images()
        if callable(labels):
            labels = labels()
        return images, labels

    @staticmethod
    def _validate_labels(inputs):
        """Labels index rows of the centers table and columns of the logits inside the loss kernels: a label outside
        [0, num_classes) (list / num_classes mismatch, a hand-built inputs dict) must fail HERE, at graph-construction
        time, like TF's range error -- not as an out-of-bounds device access.  Resident label tensors are checked once
        (one host sync at setup); batches from data.train_inputs are checked per batch in the loader thread."""
        labels = inputs.get('labels')
        if callable(labels) or not isinstance(labels, torch.Tensor) or labels.numel() == 0 or 'num_classes' not in inputs:
            return
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= int(inputs['num_classes']):
            raise ValueError('labels must lie in [0, num_classes): got [%d, %d] with num_classes = %d'
                             % (lo, hi, int(inputs['num_classes'])))

    def _compact(self):
        """the sampled-class head's compact classifier update (nets/sphere.py apply_compact_update) is on for this model"""
        active = getattr(self.model, 'compact_active', None)
        return active is not None and active()

    def _lr_value(self):
        return float(self.lr(self.global_step)) if callable(self.lr) else float(self.lr)

    def _forward_loss(self, images, labels, num_classes, scope):
        m = self.model
        m.tower_scale = 1.0 / self.num_gpus          # data_parallel.py:37
        m.global_step = self.global_step
        if m.needs_labels:                            # data_parallel.py:220 (margin nets)
            logits = m.forward(images, labels, num_classes=num_classes, is_training=True)
        else:                                         # data_parallel.py:51,133
            logits = m.forward(images, num_classes=num_classes, is_training=True)
        return m.loss_function(scope, labels, **logits)

    class _Construction(object):
        """The reference builds its graph here and runs NOTHING: variables get their initial values, the non-trainable
        state (BatchNorm moving statistics -- UPDATE_OPS --, the center loss's scatter_sub on `centers`) only moves when
        train_ops runs.  This engine is eager, so the construction-time forward / loss pass (it creates the variables and the
        loss handles) runs with those side effects switched off."""

        def __init__(self, model):
            self.m = model

        def __enter__(self):
            m = self.m
            self.prev = (getattr(m, 'update_moving_stats', None), getattr(m, 'update_centers', None))
            if self.prev[0] is not None:
                m.update_moving_stats = False
            if self.prev[1] is not None:
                m.update_centers = False

        def __exit__(self, *exc):
            m = self.m
            if self.prev[0] is not None:
                m.update_moving_stats = self.prev[0]
            if self.prev[1] is not None:
                m.update_centers = self.prev[1]

    def _setup(self, inputs):
        m = self.model
        self._validate_labels(inputs)
        m.weight_decay = self.weight_decay
        make = getattr(m, 'make_optimizer', None)
        self._opt = make(self.optimizer) if make is not None else _DeviceOptimizer(m, self.optimizer)

    def __call__(self, inputs):
        self._setup(inputs)
        num_classes = inputs['num_classes']
        state = {}

        def train_ops():
            images, labels = self._fetch(inputs)
            losses, names, others = self._forward_loss(images, labels, num_classes, 'TOWER')
            if not self.pretrained_param:
                self.pretrained_param = self.model.pretrained_param()
            self.model.backward()
            self.learning_rate = self._lr_value()
            self._opt.apply(self.learning_rate, self.global_step + 1, self.model.mult_lr_list())
            if self._compact():                       # model.compact_head_update: arena_groups() left the classifier out
                self.model.apply_compact_update(self._opt, self.learning_rate, self.global_step + 1, self.model.mult_lr_list())
            self.global_step += 1                     # data_parallel.py:75-77
            state['losses'], state['others'] = losses, others
            return losses, others

        # Build the variables and the loss handles now (graph construction time in the reference).
        images, labels = self._fetch(inputs)
        with self._Construction(self.model):
            losses, losses_name, others = self._forward_loss(images, labels, num_classes, 'TOWER')
        self.pretrained_param = self.model.pretrained_param()
        return train_ops, losses, losses_name, others


class DataParallel(Singular):
    """data_parallel.py:81-166: synchronous data parallelism, one replica per GPU."""

    def __init__(self, model, lr, optimizer, num_gpus=4, weight_decay=5e-4, comm=None, sync_centers=False, sync_sample=False,
                 shard_classes=False):
        """`sync_centers` (not in the reference; default off = the reference's behaviour): the center loss's `centers` table
        is per-tower state there (loss.py:34-39) and the towers' tables drift apart; True all-gathers every step's scatter rows
        so that all replicas keep ONE table, equal to the single-tower update of the global batch (nets/graph.py _reconcile_centers).
        `sync_sample` (default off): a sampled-class head (sample_rate) under data parallelism.  The ranks all-gather their labels
        and draw ONE class sample from the global batch, the compact [D, Spad] classifier gradient is all-reduced instead of the
        dense one and goes straight into the classifier; without it such a net is refused.  No effect on a dense
        head.
        `shard_classes` (default off): the margin classifier split by class over the ranks (model parallelism for the head, DESIGN.md
        4.20; SphereNet-ArcFace / -CosFace, dense head, one centre per class).  Rank r holds C / R columns, their optimizer slots
        and their gradient; the features of the global batch are all-gathered, the classifier gradient is final on its rank and is
        never all-reduced, dx comes back through a reduce-scatter.  The net must not have been built yet."""
        assert num_gpus > 1, 'DataParallel objects are only used for multi-gpu training tasks.'
        self.shard_classes = bool(shard_classes)
        if self.shard_classes:
            check_shard_classes(model, sync_sample)
        if getattr(model, 'sample_rate', None) is not None and not sync_sample:
            # each rank sees other labels, so the ranks' samples would differ and the all-reduce would average gradients of
            # different column sets
            raise ValueError('a sampled-class head (sample_rate %g) runs on one GPU only: num_gpus = %d' % (model.sample_rate, num_gpus))
        super(DataParallel, self).__init__(model, lr, optimizer, weight_decay)
        self.num_gpus = num_gpus
        self.pretrained_param = []
        self.comm = comm
        self.sync_centers = bool(sync_centers)
        self.sync_sample = bool(sync_sample)
        self._global_batch = None

    def _shard(self, t):
        """tf.split(axis=0, num_or_size_splits=num_gpus) (data_parallel.py:206-207): this rank's rows.
        With inputs['batch_size'] given, a tensor that already has batch_size/num_gpus rows is taken
        as this rank's shard (each rank's loader reads only its own rows)."""
        n = t.shape[0]
        if self._global_batch is not None and n * self.num_gpus == self._global_batch:
            return t
        assert n % self.num_gpus == 0, 'batch size must be divisible by num_gpus (train.py:98)'
        sh = n // self.num_gpus
        r = self.comm.rank()
        return t[r * sh:(r + 1) * sh]

    def _reduced_opt(self):
        """data_parallel.py:88-113 / :175-200.  Backward runs bucket by bucket; as soon as a bucket of
        the gradient arena is final its sum-all-reduce is enqueued (RCCL's own stream), so the head
        bucket (classifier + FC, 73 MB of the 120 MB) crosses xGMI under the conv backward.  Then every
        replica applies the same summed gradient to its own copy with its own slots."""
        m = self.model
        works = []
        buckets = m.grad_buckets()
        compact = None
        sharded = self.shard_classes                    # until the head stage has run
        for stage, (a, b) in zip(m.backward_stages(), buckets):
            stage()
            if sharded:
                # behind backward_head the classifier gradient of this rank's columns is final (no rank holds another part of it): the
                # update follows on the kernel stream, behind the products that read W, with no collective to wait for; the head bucket
                # is the FC range and the loss slots get the 16-byte all-reduce of their own
                sharded = False
                if not getattr(self._opt, 'supports_ranges', False):
                    raise ValueError('shard_classes needs an optimizer that updates a range of the arena')
                self.learning_rate = self._lr_value()
                self._opt.apply(self.learning_rate, self.global_step + 1, m.mult_lr_list(), m.cls_start, m.arena_size)
                compact = (None, self.comm.all_reduce_async(m.loss_slots))
            if self._compact() and compact is None:
                # the sampled-class head with one shared sample: behind backward_head the classifier gradient is the compact
                # [D, Spad] buffer, the same columns on every rank, so its sum is the dense sum (the zeros of the other columns add
                # exactly); the head bucket is the FC range alone, and the four loss slots behind the arena, no longer next to it,
                # get a 16-byte all-reduce of their own
                compact = (self.comm.all_reduce_async(m.compact_grad()), self.comm.all_reduce_async(m.loss_slots))
            works.append(self.comm.all_reduce_async(m.grads[a:b]))
        self.learning_rate = self._lr_value()
        if compact is not None:
            if compact[0] is not None:
                compact[0].wait()
                m.apply_compact_update(self._opt, self.learning_rate, self.global_step + 1, m.mult_lr_list())
            compact[1].wait()
        if getattr(self._opt, 'supports_ranges', False):
            # bucket by bucket, in completion order: the head bucket (73 of the 120 MB) is updated while the later, smaller
            # all-reduces are still crossing xGMI -- the kernel stream only ever waits for the bucket it is about to update
            for w, (a, b) in zip(works, buckets):
                w.wait()
                self._opt.apply(self.learning_rate, self.global_step + 1, m.mult_lr_list(), a, min(b, m.arena_size))
        else:
            for w in works:
                w.wait()
            self._opt.apply(self.learning_rate, self.global_step + 1, m.mult_lr_list())

    def __call__(self, inputs):
        if self.comm is None:
            self.comm = _HostComm()
        assert self.comm.world_size() == self.num_gpus, \
            'one process per GPU: launch with torch.distributed.run --nproc-per-node %d' % self.num_gpus
        self._setup(inputs)
        if hasattr(self.model, 'center_comm'):
            self.model.center_comm = self.comm if self.sync_centers else None
        if self.sync_sample and getattr(self.model, 'sample_rate', None) is not None:
            self.model.sample_comm = self.comm
            self.model.compact_head_update = True
        num_classes = inputs['num_classes']
        if self.shard_classes:
            from . import heads
            check_shard_classes(self.model, self.sync_sample)
            heads.shard_range(num_classes, self.num_gpus, self.comm.rank())      # a rank without a class: refused before the build
            self.model.shard_comm = self.comm                 # before the construction pass: build() lays out this rank's columns
        self._global_batch = inputs.get('batch_size')
        scope = 'TOWER_%d' % self.comm.rank()
        # the reference's towers draw independent dropout masks (one layers.dropout op per tower); a shared seed would
        # give every replica the same mask for its shard
        if hasattr(self.model, 'dropout_seed'):
            base = getattr(self.model, '_dropout_seed_base', None)
            if base is None:
                base = self.model._dropout_seed_base = int(self.model.dropout_seed)
            self.model.dropout_seed = base * self.num_gpus + self.comm.rank()

        def tower():
            images, labels = self._fetch(inputs)
            return self._forward_loss(self._shard(images), self._shard(labels), num_classes, scope)

        def train_ops():
            losses, names, others = tower()
            self._reduced_opt()
            self.global_step += 1                     # data_parallel.py:160-161
            return losses, others

        with self._Construction(self.model):
            losses, losses_name, others = tower()
        # train.py:101-120: every replica starts from replica 0's values
        self.comm.broadcast(self.replicated_params(), src=0)
        self.pretrained_param = self.model.pretrained_param()
        return train_ops, losses, losses_name, others

    def replicated_params(self):
        """the part of the parameter arena every rank holds a copy of: all of it, or what lies before a sharded classifier"""
        return self.model.params[:self.model.cls_start] if self.shard_classes else self.model.params


class DataParallel_margin(DataParallel):
    """data_parallel.py:168-256: identical to DataParallel except that labels go into
    model.forward (:220) and `others` are collected per tower (:225-228).  Both behaviours are
    selected by the model (`needs_labels`) here, so the subclass only keeps the name."""
    pass
