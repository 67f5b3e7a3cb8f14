"""Static-graph engine for the BN / pooling nets (ResNet family) on libfte.so.

A net is a list of ops over named NHWC tensors (the same description the oracle executes,
oracle/graphnet.py).  `GraphNet` compiles it once -- shapes, one flat parameter arena
[gamma+beta | conv W | classifier W], a state arena for the BN moving statistics, BN+add+ReLU
fusion -- and then forward / backward are fixed sequences of kernel launches on the current stream.
It replaces the TF graph that nets/resnet.py builds and `tf.gradients` differentiates
(data_parallel.py:33); every FLOP runs in libfte.so.
"""
from collections import OrderedDict

import torch

from .. import _lib, heads
from . import plan
from .net_base import (MARGIN_PRESETS, NORMALISED_HEADS, Network, adaface_params, adaface_state, curricular_params, curricular_state,
                       magface_params, margin_params, side_stream)
from .plan import shuffle_perm, stem_kpad          # noqa: F401 (shuffle_perm: the tests import it from here)
from .sphere import Variable

BN_EPS = 1e-3          # nets/resnet.py:97-99 via layers.batch_norm defaults
BN_DECAY = 0.999


def _stream():
    return torch.cuda.current_stream().cuda_stream



class _Activations(dict):
    """name -> stored activation.  A BN output that was folded into the channel gather that consumes it is never stored;
    asking for it (tests, debugging) recomputes it from z and the kept scale / shift."""

    def __init__(self, net):
        super(_Activations, self).__init__()
        self.net = net

    def __missing__(self, name):
        net = self.net
        if name in getattr(net, 'se_fused', {}):         # the BN output / gated tensor of a fused SE block (never stored)
            which, out, z = net.se_fused[name]
            b = net.bn[out]
            zz = self[z]
            if zz.dtype == torch.int16:
                zz = zz.view(torch.bfloat16).float()
            y = torch.addcmul(b['shift'], zz, b['scale'])
            return y if which == 'y' else y * self[out + '/gate'][:, None, None, :]
        if name not in net.folded:
            raise KeyError(name)
        z, relu = net.folded[name]
        b = net.bn[name]
        zz = self[z]
        if zz.dtype == torch.int16:                      # bf16 storage
            zz = zz.view(torch.bfloat16).float()
        y = torch.addcmul(b['shift'], zz, b['scale'])
        return torch.relu(y) if relu else y


class _Walk(object):
    """What the handlers of one walk over the plan share beside the net's buffers.  forward: batch size, _lib.call as found when the
    walk started, training / storage mode, the main and side streams, the stream and workspace of the op at hand, the BN ops whose
    statistics a conv epilogue left, the folds taken, the events of the shortcut branches and of the filter packs.  backward: the
    side stream's handle and workspace, the queued filter gradients, the BN outputs reduced by a fused data gradient, the gradients
    in flight.  _alloc: batch size, storage mode and the workspace bytes needed so far."""
    __slots__ = ('call', 'n', 'is_training', 's16', 'sfx', 'upd', 'main', 'side', 'st', 'ws', 'on_side', 'pack_ev', 'packs_pending',
                 'stats_done', 'folded_in', 'sc_ev', 'wst', 'wws', 'pending', 'reduced', 'G', 'need')


class GraphNet(Network):
    """Network whose body is an op list: ('conv', out, inp, wname, stride) | ('bn', out, inp, prefix) |
    ('relu', out, inp) | ('add', out, a, b) | ('maxpool', out, inp) | ('gap', out, inp) |
    ('dropout', out, inp, keep) | ('fc', out, inp, wname, None) | ('gconv', out, inp, wname, stride, groups) |
    ('se', out, inp, prefix[, scope1, scope2]) | ('dwconv', out, inp, wname, stride) | ('split', out_a, inp, out_b) |
    ('shufsplit', out_s, a, b, out_x, fmt) | ('shufcat', out, a, b, fmt).
    `channel_pad` > 1 (ShuffleNet: 64) stores every activation and weight with its channel count rounded up to that
    multiple; the padding channels are exactly zero in the forward and backward pass (zero weight rows / columns, BN of
    a constant-zero channel with beta 0 stays 0, and every gradient flowing into them is 0), so results equal the
    unpadded net's while all kernels keep their float4 / MFMA-tile granularity.  Heads: 'softmax' (CE on the classifier), 'focal' (loss.py:18-27 instead of CE), 'softmax+center' (CE + weight * center loss
    on the pooled features, loss.py:29-45), 'triplet' (batch-hard triplet on the pooled features, loss.py:47-78, no
    classifier) and 'arcface' / 'cosface' (additive-margin softmax on the normalised classifier input and columns, fte.h
    fte_margin_softmax_fwd_bwd; (S, m, m3) in margin_scale / margin / margin_cos) and 'adaface' (the same head with the margin of
    each row set from the norm of the classifier's input against two running scalars, fte.h fte_adaface_margins /
    fte_margin_softmax_rows_fwd_bwd; (S, m) in margin_scale / margin, h / t_alpha in adaface_h / adaface_t_alpha; the scalars are
    state like the BN moving statistics and move under the same switch, update_moving_stats) and 'curricularface' (ArcFace's target
    logit with the hard negatives re-weighted by the running scalar t, fte.h fte_curricular_t / fte_curricular_softmax_fwd_bwd; (S, m)
    in margin_scale / margin, alpha in curricular_alpha; t is state under the same switch) and 'magface' (ArcFace's target logit with
    the margin a function of the norm of the classifier's input and a regulariser on that norm, both part of the gradient, fte.h
    fte_magface_softmax_fwd_bwd; S in margin_scale, (l_a, u_a, l_m, u_m, lambda_g) in magface; no state; a third loss, magnitude_loss)."""

    head = 'softmax'
    channel_pad = 1
    bn_eps, bn_decay = BN_EPS, BN_DECAY      # per net: IResNet sets 1e-5 / 0.9; they reach every BN call of the walk
    se_hidden_pad = None                     # multiple the SE gates' dense layers are stored at (None: channel_pad); SE-IResNet: 64

    def _pc(self, c):
        p = self.channel_pad
        return (c + p - 1) // p * p

    def __init__(self, weight_decay, data_format, name, seed=0):
        super(GraphNet, self).__init__(weight_decay, data_format, name)
        self.seed = seed
        self.built = False
        self._views = {}
        self._gpacks = {}
        self.tower_scale = 1.0
        self.global_step = 0
        self.update_moving_stats = True      # data_parallel.py:242-243: UPDATE_OPS of tower 0 only
        self.dropout_seed = 0
        self._act_n = None
        self.center_weight = 0.0          # 'softmax+center': total loss = CE + center_weight * center_loss
        self.center_alpha = 0.99          # loss.py:29 default
        self.update_centers = True        # False: the loss is evaluated without running centers_update_op (loss.py:39,43 returns it to the caller)
        self.center_comm = None           # set by DataParallel(sync_centers=True): all-gather the scatter rows, one table for all replicas
        self.triplet_margin = None        # 'triplet': None = soft-margin (softplus), loss.py:47
        self.focal_gamma, self.focal_alpha = 1.0, 2.0     # 'focal': loss.py:18 defaults (names as in the reference)
        self.margin_scale = self.margin = self.margin_cos = None      # 'arcface' / 'cosface': S, m, m3 (_set_head)
        self.sub_centers = 1              # 'arcface' / 'cosface': K centres per class in K planes of cpad columns (set_sub_centers)

    def _set_head(self, head, scale=None, margin=None, margin_cos=None):
        """the subclasses' head= argument; a margin head resolves (S, m, m3) against its preset (nets/net_base.py MARGIN_PRESETS)"""
        self.head = head
        if head in MARGIN_PRESETS:
            self.margin_scale, self.margin, self.margin_cos = margin_params(head, scale, margin, margin_cos)
        elif head == 'adaface':
            if margin_cos is not None:
                raise ValueError('the adaface head has no margin_cos')
            self.margin_scale, self.margin, self.adaface_h, self.adaface_t_alpha = adaface_params(scale, margin)
            self.margin_cos = 0.0
        elif head == 'curricularface':
            if margin_cos is not None:
                raise ValueError('the curricularface head has no margin_cos')
            self.margin_scale, self.margin, self.curricular_alpha = curricular_params(scale, margin)
            self.margin_cos = 0.0
        elif head == 'magface':
            if margin is not None or margin_cos is not None:
                raise ValueError('the magface head has no margin / margin_cos (set_magface sets its margin range)')
            vals = magface_params(scale)
            self.margin_scale, self.magface = vals[0], vals[1:]
            self.margin, self.margin_cos = 0.0, 0.0
        elif (scale, margin, margin_cos) != (None, None, None):
            raise ValueError('scale / margin / margin_cos belong to the arcface / cosface heads, not %r' % head)

    def set_sub_centers(self, K):
        """K centres per class (fte.h "Sub-center ArcFace"), before build(): the classifier becomes [D, K * cpad], centre k of class j at
        column k * cpad + j, and [D, K * C] in the reference layout (planes packed)."""
        assert not self.built, 'sub_centers is fixed when the variables are created'
        self.sub_centers = heads.check_sub_centers(K, self.head, None, self.name)

    # ---- to be provided by the subclass ----------------------------------------------------------
    def build_graph(self, in_ch, num_classes):
        """-> (graph, spec) with spec = [(variable name, reference shape, kind)], kind in
        {'conv_w', 'gamma', 'beta', 'cls_w'}."""
        raise NotImplementedError

    # ---- construction -----------------------------------------------------------------------------
    def build(self, height, width, channels, num_classes, device='cuda'):
        _lib.load()
        self.device = torch.device(device)
        self.in_hwc = (height, width, channels)
        self.num_classes = int(num_classes)
        self.cpad = (self.num_classes + 127) // 128 * 128
        self.opt = plan.read_options()                   # every FTE_* switch of the engine, as set now
        self.fuse_3x3, self.fuse_bwd_conv, self.fuse_bwd_gconv = self.opt.bn_fuse_3x3, self.opt.bn_fuse_bwd, self.opt.bn_fuse_gbwd
        self.graph, spec = self.build_graph(channels, num_classes)
        if self.sub_centers > 1:
            spec = [(n, (s[0], self.sub_centers * s[1]) if k == 'cls_w' else s, k) for n, s, k in spec]
        self.spec = OrderedDict((n, (s, k)) for n, s, k in spec)
        # shapes, typed plan ops and fusion tables (nets/plan.py); the gather tables become device tensors here
        compiled = plan.compile_net(self.graph, self.spec, self.in_hwc, self.channel_pad, self.feature_name, self.opt,
                                    self.num_classes, self.sub_centers * self.cpad, self.name, self.se_hidden_pad)
        for field, value in compiled._asdict().items():
            setattr(self, field, value)
        self.plan = [self._device_tables(op) if op[0] == 'gather' else op for op in compiled.plan]
        self._alloc_ops, self._fwd_ops, self._bwd_ops = (self._dispatch(phase) for phase in ('alloc', 'fwd', 'bwd'))
        small = [(n, s, k) for n, s, k in spec if k in ('gamma', 'beta', 'bias', 'alpha')]
        convs = [(n, s, k) for n, s, k in spec if k in ('conv_w', 'gconv_w', 'fc_w', 'dw_w', 'embed_w')]
        cls = [(n, s, k) for n, s, k in spec if k == 'cls_w']
        self.variables = OrderedDict()
        off = 0
        self.ishape = {}
        for n, s, k in small + convs + cls:
            self.ishape[n] = self._internal_shape(s, k, n)
            size = 1
            for d in self.ishape[n]:
                size *= d
            self.variables[n] = Variable(n, k, s, off, size)
            off += (size + 3) // 4 * 4
        self.small_end = self.variables[convs[0][0]].offset
        self.cls_start = self.variables[cls[0][0]].offset if cls else off
        self.arena_size = off
        dev = self.device
        self.params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(off + 4, dtype=torch.float32, device=dev)
        self.loss_slots = self.grads[off:off + 4]
        # BN moving statistics: non-trainable state, never all-reduced (each replica keeps its own; only
        # tower 0's are saved: saver.py:36-40)
        self.state = OrderedDict()
        self.state_ref = {}
        for n, s, k in small:
            if k == 'gamma':
                pre = n[:-len('/gamma')]
                cp = self.ishape[n][0]
                self.state[pre + '/moving_mean'] = torch.zeros(cp, dtype=torch.float32, device=dev)
                self.state[pre + '/moving_variance'] = torch.ones(cp, dtype=torch.float32, device=dev)
                self.state_ref[pre + '/moving_mean'] = self.state_ref[pre + '/moving_variance'] = s[0]
        if self.head == 'adaface':                        # the head's running norm statistics: two more non-trainable variables
            self.adaface_stats, extra = adaface_state(dev)
            self.state.update(extra)
        if self.head == 'curricularface':                 # t, the running mean of the target cosines: one more non-trainable variable
            self.cf_state, extra = curricular_state(dev)
            self.state.update(extra)
        self._init_params()
        self.built = True
        return self

    def _internal_shape(self, shape, kind, name=None):
        """arena layout of a variable whose reference shape is `shape`"""
        pc = (lambda c: (c + 31) // 32 * 32) if name in self.narrow else self._pc
        if self.se_hidden_pad and kind in ('fc_w', 'bias'):      # an SE gate's dense layers: zero rows / columns up to the GEMMs' granularity
            pc = lambda c: (c + self.se_hidden_pad - 1) // self.se_hidden_pad * self.se_hidden_pad
        if kind == 'cls_w':
            assert pc(shape[0]) == shape[0]
            return (shape[0], self.sub_centers * self.cpad)
        if kind == 'conv_w':
            k, _, cin, cout = shape
            if cin <= 4:                                       # the stem (image channels): [k*k*cin -> kpad, cout]
                return (stem_kpad(k, cin), pc(cout))
            return (k, k, pc(cin), pc(cout))
        if kind == 'dw_w':
            return (3, 3, pc(shape[2]))
        if kind == 'fc_w':
            return (pc(shape[-2]), pc(shape[-1]))
        if kind in ('gamma', 'beta', 'bias', 'alpha'):
            return (pc(shape[0]),)
        assert self.channel_pad == 1 or kind not in ('gconv_w', 'embed_w')
        return tuple(shape)

    def view(self, name, arena=None):
        """flat view of a variable in the parameter arena (or in `arena`, e.g. the gradient arena).  Views of the two arenas that
        live as long as the net are cached: the step makes ~1000 of these lookups and is host-bound at small shards."""
        a = self.params if arena is None else arena
        if a is self.params or a is self.grads:
            key = (name, a is self.grads)
            t = self._views.get(key)
            if t is None or t.data_ptr() != a.data_ptr() + self.variables[name].offset * 4:
                v = self.variables[name]
                t = self._views[key] = a[v.offset:v.offset + v.size]
            return t
        v = self.variables[name]
        return a[v.offset:v.offset + v.size]

    def _init_params(self):
        """layers.conv2d default Xavier-uniform; BN gamma 1 / beta 0; classifier N(0, 1e-3) (nets/resnet.py:153-157)."""
        g = torch.Generator().manual_seed(self.seed)
        for n, v in self.variables.items():
            if v.kind == 'conv_w':
                k, _, cin, cout = v.ref_shape
                lim = (6.0 / (k * k * cin + k * k * cout)) ** 0.5
                self.set_variable(n, (torch.rand(v.ref_shape, generator=g) * 2 - 1) * lim)
            elif v.kind == 'gconv_w':
                gw = v.ref_shape[3]
                lim = (6.0 / (18 * gw)) ** 0.5
                self.set_variable(n, (torch.rand(v.ref_shape, generator=g) * 2 - 1) * lim)
            elif v.kind == 'fc_w':
                lim = (6.0 / (v.ref_shape[-2] + v.ref_shape[-1])) ** 0.5
                self.set_variable(n, (torch.rand(v.ref_shape, generator=g) * 2 - 1) * lim)
            elif v.kind == 'dw_w':
                lim = (6.0 / (9 * v.ref_shape[2] + 9)) ** 0.5          # Xavier on [3,3,C,1]: fan_in 9C, fan_out 9
                self.set_variable(n, (torch.rand(v.ref_shape, generator=g) * 2 - 1) * lim)
            elif v.kind == 'cls_w':
                self.set_variable(n, torch.randn(v.ref_shape, generator=g) * 0.001)
            elif v.kind == 'embed_w':
                lim = (6.0 / (v.ref_shape[0] + v.ref_shape[1])) ** 0.5
                self.set_variable(n, (torch.rand(v.ref_shape, generator=g) * 2 - 1) * lim)
            elif v.kind == 'gamma':
                self.set_variable(n, torch.ones(v.ref_shape))
            elif v.kind == 'alpha':                      # nets/sphere.py:34
                self.set_variable(n, torch.full(v.ref_shape, 0.25))

    def get_variable(self, name, arena=None):
        if name in self.state:
            t = self.state[name]
            return t[:self.state_ref[name]].clone() if name in self.state_ref else t.clone()
        v = self.variables[name]
        t = self.view(name, arena).reshape(self.ishape[name])
        ref = v.ref_shape
        if v.kind == 'cls_w':
            return t.reshape(ref[0], self.sub_centers, self.cpad)[:, :, :self.num_classes].reshape(ref).clone()
        if v.kind == 'conv_w':
            k, _, cin, cout = ref
            if cin <= 4:
                return t[:k * k * cin, :cout].reshape(ref).clone()
            return t[:, :, :cin, :cout].clone()
        if v.kind == 'dw_w':
            return t[:, :, :ref[2]].reshape(ref).clone()
        if v.kind == 'fc_w':
            return t[:ref[-2], :ref[-1]].reshape(ref).clone()
        if v.kind in ('gamma', 'beta', 'bias', 'alpha'):
            return t[:ref[0]].clone()
        if v.kind == 'embed_w':
            return self._embed_perm(name, t, False).contiguous()
        return t.reshape(ref).clone()

    def set_variable(self, name, value, arena=None):
        if name in self.state:
            t = torch.as_tensor(value, dtype=torch.float32)
            if name in self.state_ref:
                self.state[name][:self.state_ref[name]].copy_(t)
            else:
                self.state[name].copy_(t)
            return
        v = self.variables[name]
        t = torch.as_tensor(value, dtype=torch.float32).to(self.device)
        ref = v.ref_shape
        assert tuple(t.shape) == ref, (name, tuple(t.shape), ref)
        buf = torch.zeros(self.ishape[name], device=self.device)
        if v.kind == 'cls_w':
            buf.view(ref[0], self.sub_centers, self.cpad)[:, :, :self.num_classes] = t.reshape(ref[0], self.sub_centers, self.num_classes)
        elif v.kind == 'conv_w':
            k, _, cin, cout = ref
            if cin <= 4:
                buf[:k * k * cin, :cout] = t.reshape(k * k * cin, cout)
            else:
                buf[:, :, :cin, :cout] = t
        elif v.kind == 'dw_w':
            buf[:, :, :ref[2]] = t.reshape(3, 3, ref[2])
        elif v.kind == 'fc_w':
            buf[:ref[-2], :ref[-1]] = t.reshape(ref[-2], ref[-1])
        elif v.kind in ('gamma', 'beta', 'bias', 'alpha'):
            buf[:ref[0]] = t
        elif v.kind == 'embed_w':
            buf = self._embed_perm(name, t, True)
        else:
            buf = t
        self.view(name, arena).copy_(buf.reshape(-1))

    def load_params(self, params):
        for k, val in params.items():
            self.set_variable(k, val)

    def _embed_perm(self, name, t, to_internal):
        """Rows of an FC that flattens a feature map: the reference order is the flatten order of data_format (SphereNet's fc,
        nets/sphere.py _fc_perm); the arena keeps NHWC order, the order the activations are stored in."""
        h, w, c = self.embed_in[name]
        d = t.shape[-1]
        if self.data_format == 'NHWC':
            return t.reshape(h * w * c, d)
        if to_internal:
            return t.reshape(c, h, w, d).permute(1, 2, 0, 3).reshape(h * w * c, d)
        return t.reshape(h, w, c, d).permute(2, 0, 1, 3).reshape(h * w * c, d)

    def _device_tables(self, op):
        """a 'gather' plan op with its int32 tables (plan.gather_tables) as device tensors"""
        dev = lambda pairs: [(name, torch.tensor(t, dtype=torch.int32, device=self.device)) for name, t in pairs]
        return op._replace(outs=dev(op.outs), bwd=dev(op.bwd))

    def _gather_tables(self, op):
        """the fields of the 'gather' plan op of a split / shufsplit / shufcat graph op (plan.gather_tables), tables on the device"""
        return self._device_tables(plan.gather_tables(op, self.shapes, self.real_c))._asdict()

    _op_weight_names = staticmethod(plan.op_weight_names)

    # ---- buffers --------------------------------------------------------------------------------------
    S16_OPS = ('conv', 'bn', 'bnstats', 'gconv', 'dwconv', 'gather', 'se', 'seblock', 'maxpool', 'addrelu', 'gap', 'dropout', 'fc')

    def _storage16(self):
        """bf16 STORAGE ('bf16s', fte.h): the tensors between the layers live in HBM as bf16 -- implemented for the op sets of the ResNet
        family (conv / BN / grouped 3x3 on the bf16 MFMA / max-pool / add+ReLU / GAP; BASELINE.json configs[2]) and of ShuffleNet-v2
        (depthwise 3x3, channel gathers with folded BN) and SE gates.  A grouped 3x3 that cannot run on the bf16 MFMA (channels per
        group not 4 / 8 / 16 / 32) makes the net fall back to the 'bf16' operand mode: same MFMA precision, fp32 tensors."""
        if not _lib.bf16_storage():
            return False
        ok = all(op[0] in self.S16_OPS for op in self.plan) and \
            all(self._gconv_pack(op) is not None for op in self.plan if op[0] == 'gconv')
        if not ok and not getattr(self, '_s16_note', False):
            self._s16_note = True
            print('%s: bf16 storage is not implemented for one of its ops; this net runs bf16 MFMA operands with fp32 tensors' % self.name)
        return ok

    def _dispatch(self, phase):
        """the handler of every plan op for one phase ('alloc' / 'fwd' / 'bwd'), in plan order; None: the kind has no work there"""
        return [getattr(self, '_%s_%s' % (phase, op[0]), None) for op in self.plan]

    def _alloc(self, n):
        s16 = self._storage16()
        if self._act_n == n and getattr(self, '_act_s16', False) == s16:
            return
        self._act_s16 = s16
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # h16: names of the tensors stored as bf16 (each kind's _alloc_ handler says whether its output is); the pooled features and
        # everything after them stay fp32
        self.h16 = set()
        self._pack_entries = []
        self.t = _Activations(self)
        self.bn = {}
        self.ident = {}
        w = _Walk()
        w.n, w.s16, w.need = n, s16, 1 << 20
        for op, handler in zip(self.plan, self._alloc_ops):
            if handler is None:                          # (a kind no walk knows: the forward walk raises on it)
                self._alloc_out(w, op, False, op[1])
            else:
                handler(w, op)
        # tensors whose GRADIENT is stored as bf16: the stored ones, the BN outputs folded into a gather (never stored themselves) and the
        # gated tensor of a fused SE block: its gradient g = dy * (out > 0) is stored (the shortcut's gradient too)
        self.g16 = set(self.h16)
        if s16:
            self.g16.update(self.folded)
            self.g16.update(op.s for op in self.plan if op[0] == 'seblock')
            from ._packs import FilterPacks
            self.packs = FilterPacks(self._pack_entries, dev, head=self.opt.pack_head)
            self.w16, self.w16t = self.packs.w16, self.packs.w16t
        self.G = torch.empty(n, self.sub_centers * self.cpad, **f32)
        self.loss_rows = torch.empty(n, **f32)
        fdim = self.shapes[self.feature_name][0]
        self.dfeat = torch.empty(n, fdim, **f32)
        self.ones_n = torch.ones(n, **f32)
        if self.head in NORMALISED_HEADS:
            self.xn, self.rowcoef = torch.empty(n, **f32), torch.empty(n, **f32)
            self.wn, self.colcoef = (torch.empty(self.sub_centers * self.cpad, **f32) for _ in range(2))
        if self.head == 'adaface':
            self.a_rows, self.b_rows = torch.empty(n, **f32), torch.empty(n, **f32)
        if self.head == 'curricularface':
            self.cf_t = torch.empty(1, **f32)
        if self.head == 'magface':
            self.reg_rows = torch.empty(n, **f32)
        need = max(w.need, 4 * n * fdim, 12 * n * n)
        self.ws = torch.empty((need + 3) // 4 + 1024, **f32)
        self.ws_bytes = self.ws.numel() * 4
        # filter gradients run on a second HIP stream beside the data-gradient chain (backward_body): their own workspace
        self.side = side_stream(dev, self.opt.side_prio) if self.opt.side_stream else None
        self.ws_side = torch.empty_like(self.ws) if self.side is not None else self.ws
        self.side_batch = self.opt.side_batch
        self._act_n = n

    def _alloc_out(self, w, op, stored16, name=None):
        """the output tensor of a plan op; `stored16`: as bf16 under bf16 storage -> its shape with the batch dimension"""
        name = op.out if name is None else name
        shape = (w.n,) + self.shapes[name]
        if stored16 and w.s16:
            self.h16.add(name)
        self.t[name] = torch.empty(shape, dtype=torch.int16 if name in self.h16 else torch.float32, device=self.device)
        return shape

    def _alloc_bn(self, w, op, stored=True):
        """scale / shift / statistics of a BN layer (and its output: bf16 unless it lies behind the pooling, where the features stay fp32)"""
        out = op.out
        c = self.shapes[out][-1]
        if stored:
            self._alloc_out(w, op, len(self.shapes[out]) == 3)
        self.bn[out] = dict((k, self._f32(c)) for k in ('mean', 'rstd', 'scale', 'shift'))
        self.bn[out]['coef'] = self._f32(3 * c)
        w.need = max(w.need, _lib.query('fte_bn_ws_bytes', c))

    def _f32(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _reads16(self, w, op, *names):
        """every bf16-storage entry point reads its tensor input as bf16: an fp32 input would be misread silently"""
        if w.s16:
            for x in names:
                assert x in self.h16, 'bf16 storage: %s reads %s, which is stored as fp32' % (op[0] + ' ' + op.out, x)

    # ---- the pieces several kinds share -----------------------------------------------------------------
    def _bn_args(self, op, upd):
        """(gamma, beta, mean, rstd, scale, shift, moving_mean, moving_variance, eps, decay) of a BN plan op; the moving statistics
        are None when they are not to move (`upd` False)"""
        b, pre = self.bn[op.out], op.pre
        return (self.view(pre + '/gamma'), self.view(pre + '/beta'), b['mean'], b['rstd'], b['scale'], b['shift'],
                self.state[pre + '/moving_mean'] if upd else None, self.state[pre + '/moving_variance'] if upd else None, self.bn_eps, self.bn_decay)

    def _bn_stats(self, w, op, x, x16):
        """The statistics-only pass of BN plan op `op` over its input x: batch statistics -> mean / rstd / scale / shift (training), or
        scale / shift from the moving statistics.  `x16`: x is stored as bf16."""
        c = self.shapes[op.out][-1]
        if not w.is_training:
            ba = self._bn_args(op, True)
            w.call('fte_bn_infer_coef', ba[0], ba[1], ba[6], ba[7], ba[4], ba[5], c, self.bn_eps, w.st)
            return
        ba = self._bn_args(op, w.upd)
        rows = x.numel() // c
        if w.s16:
            w.call('fte_bn_train_stats_s16', x, *ba[:8], rows, c, ba[8], ba[9], 1 if x16 else 0, self.ws, self.ws_bytes, w.st)
        else:
            w.call('fte_bn_train_stats', x, *ba[:8], rows, c, ba[8], ba[9], self.ws, self.ws_bytes, w.st)

    def _sflag(self, w, inp):
        """the storage word of the BN / SE entry points: bit 0 = the input is bf16, bit 1 = the output is; 0 outside bf16 storage"""
        return ((1 if inp in self.h16 else 0) | 2) if w.s16 else 0

    def _se_buffers(self, out):
        T = self.t
        return T[out + '/sq'], T[out + '/hid'], T[out + '/gate']

    def _alloc_se_gate(self, w, out, se, c):
        n, hd = w.n, se.hidden
        self.t[out + '/sq'] = self._f32(n, c)
        self.t[out + '/hid'] = self._f32(n, hd)
        self.t[out + '/gate'] = self._f32(n, c)
        w.need = max(w.need, _lib.query('fte_gemm_ws_bytes', n, c, hd), _lib.query('fte_gemm_ws_bytes', n, hd, c))
        # backward scratch: dsq is shared by all SE blocks of a width; dgate / dhid are per block -- the gate's weight gradients
        # read them on the side stream while the walk has moved on to the next block
        if ('se', 'dsq', c) not in self.ident:
            self.ident[('se', 'dsq', c)] = self._f32(n, c)
        self.ident[('se', out, 'dgate')] = self._f32(n, c)
        self.ident[('se', out, 'dhid')] = self._f32(n, hd)

    def _se_gate_fwd(self, w, out, se, c, how):
        """squeeze -> hidden -> gate: the SE gate's two dense layers with ReLU / sigmoid.  `how`: 'small' (fte_dense_small, one launch
        each), 'act' (the GEMM with the activation in the same pass over the output) or 'plain' (activations as launches of their own)"""
        call, st, n, hd = w.call, w.st, w.n, se.hidden
        sq, hid, gate = self._se_buffers(out)
        w1, b1, w2, b2 = self.view(se.w1), self.view(se.b1), self.view(se.w2), self.view(se.b2)
        if how == 'small':
            call('fte_dense_small', sq, w1, b1, None, hid, n, hd, c, 0, 1, st)
            call('fte_dense_small', hid, w2, b2, None, gate, n, c, hd, 0, 2, st)
        elif how == 'act':
            call('fte_gemm_nn_act', sq, w1, b1, hid, n, hd, c, 1, self.ws, self.ws_bytes, st)
            call('fte_gemm_nn_act', hid, w2, b2, gate, n, c, hd, 2, self.ws, self.ws_bytes, st)
        else:
            call('fte_gemm_nn', sq, w1, b1, hid, n, hd, c, self.ws, self.ws_bytes, st)
            call('fte_act_fwd', hid, hid, hid.numel(), 0, st)
            call('fte_gemm_nn', hid, w2, b2, gate, n, c, hd, self.ws, self.ws_bytes, st)
            call('fte_act_fwd', gate, gate, gate.numel(), 1, st)

    def _se_gate_bwd(self, w, out, se, c, small):
        """dgate = d(pre-sigmoid) -> dsq, the gradient of the squeeze, through the gate's two dense layers.  The four parameter
        gradients feed nothing but the optimizer: side stream, like every filter gradient.  `small`: fte_dense_small, which takes
        the ReLU mask in the same launch.  -> dsq"""
        call, st, n, hd = w.call, w.st, w.n, se.hidden
        sq, hid, _ = self._se_buffers(out)
        # scratch preallocated in _alloc (three allocator calls per SE block and step otherwise)
        dgate, dhid, dsq = self.ident[('se', out, 'dgate')], self.ident[('se', out, 'dhid')], self.ident[('se', 'dsq', c)]
        self._wgrad(w, 'fte_gemm_tn', dgate, hid, dgate, self.view(se.w2, self.grads), n, c, hd, w.wws, self.ws_bytes, w.wst)
        self._wgrad(w, 'fte_reduce_rows', dgate, dgate, self.view(se.b2, self.grads), None, 1, n, c, 1, 1.0, w.wst)
        if small:                                      # d(pre-ReLU) = (dgate W2^T) * (hid > 0) in one launch
            call('fte_dense_small', dgate, self.view(se.w2), None, hid, dhid, n, hd, c, 1, 0, st)
        else:
            call('fte_gemm_nt', dgate, self.view(se.w2), None, None, 0, None, dhid, None, n, c, hd, self.ws, self.ws_bytes, st)
            call('fte_act_bwd', dhid, hid, dhid, dhid.numel(), 0, st)                        # -> d(pre-ReLU)
        self._wgrad(w, 'fte_gemm_tn', dhid, sq, dhid, self.view(se.w1, self.grads), n, hd, c, w.wws, self.ws_bytes, w.wst)
        self._wgrad(w, 'fte_reduce_rows', dhid, dhid, self.view(se.b1, self.grads), None, 1, n, hd, 1, 1.0, w.wst)
        if small:
            call('fte_dense_small', dhid, self.view(se.w1), None, None, dsq, n, c, hd, 1, 0, st)
        else:
            call('fte_gemm_nt', dhid, self.view(se.w1), None, None, 0, None, dsq, None, n, hd, c, self.ws, self.ws_bytes, st)
        return dsq

    def _wait_shortcut(self, w, *names):
        """the shortcut branch (side stream) has written these tensors"""
        for nm in names:
            if nm in w.sc_ev:
                w.main.wait_event(w.sc_ev.pop(nm))

    def _wgrad(self, w, name, dy, *args):
        """a filter-gradient launch: queued for the side stream (released by _flush), or issued at once without one"""
        if w.side is None:
            w.call(name, *args)
        else:
            w.pending.append((name, dy, args))

    def _flush(self, w, limit=0):
        if len(w.pending) > limit:
            w.side.wait_event(w.main.record_event())
            for name, dy, args in w.pending:
                dy.record_stream(w.side)
                w.call(name, *args)
            del w.pending[:]

    def _bn_below(self, w, name):
        """arguments of the BN layer whose output `name` a fused data gradient lands on, or None"""
        bj = self.fuse_bwd.get(name)
        if bj is None:
            return None
        bop = self.plan[bj]
        T = self.t
        if w.s16 and not (bop.inp in self.h16 and bop.out in self.h16):
            return None
        b, pre = self.bn[bop.out], bop.pre
        zmask = bop.relu and bop.res is None
        return (T[bop.inp], T[bop.out] if bop.res is not None else None, self.view(pre + '/gamma'), b['mean'], b['rstd'],
                b['scale'] if zmask else None, b['shift'] if zmask else None), \
               (self.view(pre + '/gamma', self.grads), self.view(pre + '/beta', self.grads), b['coef'])

    def _folds(self, w, bj):
        """does the consumer of BN plan op bj take the normalise pass into its loader? (bf16 storage, training, statistics fused)"""
        cj = self.fold_apply.get(bj)
        if cj is None or not (w.s16 and w.is_training and bj in w.stats_done):
            return False
        cop = self.plan[cj]
        ih, iw, cin = self.shapes[cop.inp]
        if cop[0] == 'gconv':                       # (its fused launch carries the fold: FTE_BN_FUSE_3X3=0 takes both away)
            return cop.stride == 1 and self._gconv_pack(cop) is not None and self.fuse_3x3
        return bool(_lib.query('fte_conv2d_bn_fwd_folds', w.n, ih, iw, cin, self.shapes[cop.out][-1], self.spec[cop.wname][0][0], cop.stride, 1))

    def _fold_args(self, w, j):
        """(x, in_scale, in_shift, y_side) of consumer plan op j"""
        bj = w.folded_in.get(j)
        if bj is None:
            return self.t[self.plan[j].inp], None, None, None
        bop = self.plan[bj]
        b = self.bn[bop.out]
        return self.t[bop.inp], b['scale'], b['shift'], self.t[bop.out]

    def _gconv_pack(self, op):
        """(forward, dgrad) packed bf16 filters of a grouped 3x3 that runs on the matrix cores -- bf16 MFMA mode,
        4 / 8 / 16 / 32 channels per group -- else None (fp32 vector kernels)."""
        c = self.shapes[op.inp][-1]
        if c % 32 or (c // op.groups) not in (4, 8, 16, 32) or _lib.get_mfma_dtype() != 'bf16' or not self.opt.gconv_mfma:
            return None
        pk = self._gpacks.get(op.wname)
        if pk is None:
            words = (c // 32) * 9 * 1024
            pk = self._gpacks[op.wname] = (torch.empty(words, dtype=torch.int16, device=self.device),
                                           torch.empty(words, dtype=torch.int16, device=self.device))
        return pk

    def _direct_stem(self, k, cin, cout):
        return plan.direct_stem(k, cin, cout, self.opt)

    def _se_small(self, c, hd):
        """the SE gate's dense layers through fte_dense_small (one launch each)?  FTE_SE_DENSE=0: fte_gemm_* (A/B hook)"""
        return c % 128 == 0 and hd % 128 == 0 and self.opt.se_dense

    def _scr(self, c, i):
        key = ('scr', c, i)
        if key not in self.ident:
            self.ident[key] = torch.empty(c, dtype=torch.float32, device=self.device)
        return self.ident[key]

    def _new(self, name):
        """a gradient buffer for tensor `name`: bf16 where the tensor (or, for a BN output folded into a gather, its gradient) is"""
        if name in self.folded:                  # never stored: no tensor to take the layout from
            z = self.t[self.folded[name][0]]
            return torch.empty(z.shape, dtype=torch.int16 if name in self.g16 else torch.float32, device=self.device)
        return torch.empty_like(self.t[name])

    # ---- forward ----------------------------------------------------------------------------------------
    def _check_images(self, images):
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32):
            raise TypeError('images must be a float32 CUDA tensor in NHWC (data.py:275-279 layout)')
        return images.contiguous()

    def _run_forward(self, images, is_training):
        x = self._check_images(images)
        n, h, wd, ch = x.shape
        assert (h, wd, ch) == self.in_hwc, ((h, wd, ch), self.in_hwc)
        self._alloc(n)
        self.t['images'] = x
        w = _Walk()
        w.call, w.n, w.is_training, w.s16, w.sfx = _lib.call, n, is_training, self._act_s16, '_s16' if self._act_s16 else ''
        w.upd = self.update_moving_stats
        w.main, w.side = torch.cuda.current_stream(), self.side
        w.st, w.ws, w.on_side = w.main.cuda_stream, self.ws, False
        w.pack_ev, w.packs_pending = None, False
        w.stats_done = set()                             # BN plan ops whose statistics came out of the producing conv's epilogue
        w.folded_in = {}                                 # consumer plan op -> BN plan op whose normalise pass its loader applies
        w.sc_ev = {}                                     # shortcut tensor -> event of the side stream that completes it
        self._start_regularizer(w)
        if w.s16:
            self._start_packs(w)
        st_main = w.st
        side_ops = self.shortcut_fwd if (self.side is not None and is_training) else ()
        sst = self.side.cuda_stream if side_ops else None
        for j, (op, handler) in enumerate(zip(self.plan, self._fwd_ops)):
            if handler is None:
                raise RuntimeError('op %s must have been fused away' % op[0])
            if j in side_ops:
                w.on_side, w.st, w.ws = True, sst, self.ws_side
            else:
                w.on_side, w.st, w.ws = False, st_main, self.ws
            handler(w, j, op)

    def _start_regularizer(self, w):
        self._reg_ev = None
        if w.is_training and self.side is not None and self.opt.reg_side:
            # Network._regularize's sum over the decayed weights (one pass over the arena: 25-40 us) depends on nothing the walk computes:
            # it runs on the side stream under the first layers instead of between the loss head's launches; loss_function waits for it
            self.side.wait_stream(w.main)
            nreg = self.arena_size - self.small_end
            # (into a scratch scalar of its own, not the displayed slot: the previous step's reg_loss stays readable until this step's
            # loss_function copies the new value in; the scale used is remembered -- a tower_scale / weight_decay changed between
            # forward() and loss_function() makes loss_function recompute)
            if getattr(self, '_reg_scratch', None) is None:
                self._reg_scratch = torch.zeros(4, dtype=torch.float32, device=self.params.device)
            self._reg_scale = 0.5 * self.weight_decay * self.tower_scale
            w.call('fte_sumsq', self.params[self.small_end:], nreg, self._reg_scale,
                   self._reg_scratch[0:1], self.ws_side, self.ws_bytes, self.side.cuda_stream)
            self._reg_ev = self.side.record_event()

    def _start_packs(self, w):
        """Every filter's bf16 packs, refreshed once per step.  The walk's first layers need only THEIR forward packs: those are
        made here; the rest -- the other layers' forward packs, every HWIO pack (read by the backward pass only) and the
        grouped convs' packs -- are made on the side stream under the first layers, and the first conv outside the head
        waits for them (0.27 ms of launches off the ResNeXt-50 step's critical path at 128 images)."""
        if self.side is None or self.packs.head_names == set(self.w16t):
            self.packs.refresh(self.params, w.st)
            return
        self.packs.refresh_head(self.params, w.st)
        # A 7x7 stem's im2col (150-200 MB of strided traffic) and the packs (the same again) choke each other when they run
        # side by side: im2col 74 -> 240-260 us beside ResNet-50's 47 MB of packs (profiles/r5_resnet50_*).  The packs start
        # behind the im2col instead, under the stem's GEMM (FTE_PACK_AFTER_STEM=0: at the start of the walk, as before).
        first = self.plan[0]
        stem_cols = first[0] == 'conv' and self.shapes[first.inp][-1] < 32 and \
            not self._direct_stem(self.spec[first.wname][0][0], self.shapes[first.inp][-1], self.shapes[first.out][-1])
        if stem_cols and self.opt.pack_after_stem:
            w.packs_pending = True
        else:
            w.pack_ev = self._side_packs(w)

    def _side_packs(self, w):
        """the packs the head of the walk does not need, on the side stream -> the event that completes them"""
        side = self.side
        side.wait_stream(w.main)
        sst = side.cuda_stream
        self.packs.refresh_rest(self.params, sst)
        for op in self.plan:
            if op[0] == 'gconv':
                pk = self._gconv_pack(op)
                if pk is not None:
                    w.call('fte_gconv3x3_pack_bf16', self.view(op.wname), pk[0], pk[1], self.shapes[op.inp][-1], op.groups, sst)
        w.packs_pending = False
        return side.record_event()

    def _wait_packs(self, w):
        """the side stream's packs (once: every later layer is behind this wait)"""
        torch.cuda.current_stream().wait_event(w.pack_ev)
        w.pack_ev = None

    # ---- backward ---------------------------------------------------------------------------------------
    def backward_body(self, lo=0, hi=None):
        """The backward walk over plan ops [lo, hi) (default: the whole body), last op first.  Segments are walked from the end of
        the plan: the gradients in flight between two calls stay in self._grad; when a call returns its filter gradients are final."""
        nops = len(self.plan) - (1 if self.has_classifier else 0)
        hi = nops if hi is None else hi
        if hi == nops and not self.has_classifier:
            self._grad = {self.feature_name: self._dfeat}
            self._dfeat = None
        if hi == nops:
            self._reduced = set()
        w = _Walk()
        w.call, w.n, w.s16, w.sfx = _lib.call, self._act_n, self._act_s16, '_s16' if self._act_s16 else ''
        # Filter gradients (conv / depthwise / grouped wgrad + their slab reductions) depend only on the layer's dz and its
        # stored input, and nothing but the optimizer reads them: they go to a second stream and overlap the dgrad -> BN
        # backward chain (these nets' kernels are 5-60 us long and leave CUs idle at their ramps and tails).  An event on
        # the main stream costs it a ~7 us bubble, so the launches are queued and released a few layers at a time.
        w.main, w.side = torch.cuda.current_stream(), self.side
        w.st = w.main.cuda_stream
        w.wst, w.wws = (w.side.cuda_stream, self.ws_side) if w.side is not None else (w.st, self.ws)
        w.pending = []
        w.reduced = self._reduced  # BN outputs whose mask / reduction pass ran in the epilogue of the data gradient that produced G[name]
        G = w.G = self._grad
        plan_ops, handlers, feat = self.plan, self._bwd_ops, self.feature_name
        for j in range(hi - 1, lo - 1, -1):
            op = plan_ops[j]
            out = op[1]
            if out == feat and self._dfeat is not None and out in G:
                # the pooled features also feed the center loss: add its gradient to the classifier path's
                d = G[out].shape[1]
                w.call('fte_add_scaled_rows_cols', G[out], self._dfeat, self.ones_n, None, w.n, d, d, w.st)
                self._dfeat = None
            if out not in G:                             # (a gather: the first of its outputs)
                continue
            if handlers[j] is None:
                raise RuntimeError(op[0])
            handlers[j](w, op, G.pop(out))
        if w.side is not None:
            self._flush(w)
            w.main.wait_stream(w.side)
        if lo == 0:
            self._grad = {}

    # ---- the plan kinds: buffers, forward, backward of each ----------------------------------------------
    def _alloc_conv(self, w, op):
        # every conv writes bf16 under bf16 storage: the MFMA convs, the direct 3x3 stem, and the im2col stem (a 1x1 conv of `kpad` bf16
        # columns on the bf16-source kernels)
        n, q, s16 = w.n, _lib.query, w.s16
        shape = self._alloc_out(w, op, True)
        ih, iw, cin = self.shapes[op.inp]
        k, stride, cout = self.spec[op.wname][0][0], op.stride, shape[-1]
        if cin >= 32:
            self._reads16(w, op, op.inp)
            w.need = max(w.need, *[q('fte_conv2d_%s_ws_bytes' % what, n, ih, iw, cin, cout, k, stride)
                                   for what in ('fwd', 'dgrad', 'wgrad', 'bn_fwd', 'dgrad_bn')])
            if s16:          # bf16 packs of the filter: HWIO (data gradient) and [tap][cout][cin] (forward), refreshed every step
                self._pack_entries.append((op.wname, self.variables[op.wname].offset, k, cin, cout))
        elif self._direct_stem(k, cin, cout):
            w.need = max(w.need, q('fte_conv3x3_first_wgrad_ws_bytes', n, ih, iw, cin, cout, stride))
        else:
            oh, ow, _ = self.shapes[op.out]
            kpad = stem_kpad(k, cin)
            self.cols = torch.empty(n * oh * ow, kpad, dtype=torch.int16 if s16 else torch.float32, device=self.device)
            w.need = max(w.need, q('fte_gemm_ws_bytes', n * oh * ow, cout, kpad))
            if s16:          # the stem as a 1x1 conv of kpad bf16 columns: packs like any other conv's, [1, 1, kpad, cout]
                self._pack_entries.append((op.wname, self.variables[op.wname].offset, 1, kpad, cout))
                w.need = max(w.need, q('fte_conv2d_fwd_ws_bytes', n, oh, ow, kpad, cout, 1, 1), q('fte_conv2d_bn_fwd_ws_bytes', n, oh, ow, kpad, cout, 1, 1),
                             q('fte_conv2d_wgrad_ws_bytes', n, oh, ow, kpad, cout, 1, 1))

    def _fwd_conv(self, w, j, op):
        call, T, s16, n, st = w.call, self.t, w.s16, w.n, w.st
        out, inp, wname, stride = op.out, op.inp, op.wname, op.stride
        ih, iw, cin = self.shapes[inp]
        k = self.spec[wname][0][0]
        cout = self.shapes[out][-1]
        if w.on_side:
            w.side.wait_event(w.main.record_event())          # the block's input is complete (the packs were made on this stream)
        if cin < 32:
            self._fwd_stem(w, j, op, k, cin, cout)
            return
        if not w.on_side and w.pack_ev is not None and wname not in self.packs.head_names:
            self._wait_packs(w)
        bj = self.fuse_fwd.get(j) if w.is_training else None
        if bj is not None and (k == 1 or not s16 or self.fuse_3x3):          # conv + the batch statistics of its output ("BN fusion")
            xin, isc, ish, yside = self._fold_args(w, j)
            call('fte_conv2d_bn_fwd', xin, self.w16t[wname] if s16 else self.view(wname), T[out], *self._bn_args(self.plan[bj], w.upd),
                 isc, ish, yside, n, ih, iw, cin, cout, k, stride, 1 if s16 else 0, w.ws, self.ws_bytes, st)
            w.stats_done.add(bj)
        elif s16:          # bf16 storage: bf16 x in, bf16 z out, filters packed once per step
            call('fte_conv2d_fwd_s16', T[inp], self.w16t[wname], None, None, None, None, T[out], None, None,
                 n, ih, iw, cin, cout, k, stride, w.ws, self.ws_bytes, st)
        else:
            call('fte_conv2d_fwd', T[inp], self.view(wname), None, None, None, None, T[out],
                 n, ih, iw, cin, cout, k, stride, w.ws, self.ws_bytes, st)

    def _fwd_stem(self, w, j, op, k, cin, cout):
        """the first conv (image channels)"""
        call, T, s16, n, st = w.call, self.t, w.s16, w.n, w.st
        out, inp, wname, stride = op.out, op.inp, op.wname, op.stride
        ih, iw, _ = self.shapes[inp]
        if self._direct_stem(k, cin, cout):          # 3x3 stem of 32 / 64 stored filters: the direct MFMA kernel
            call('fte_conv3x3_first_fwd' + w.sfx, T[inp], self.view(wname), None, None, None, T[out], n, ih, iw, cin, cout, stride, st)
            return
        oh, ow, _ = self.shapes[out]
        kpad = stem_kpad(k, cin)
        if not s16:                                    # other stems (7x7): im2col + dense MFMA GEMM
            call('fte_im2col_first', T[inp], self.cols, n, ih, iw, cin, k, stride, kpad, st)
            call('fte_gemm_nn', self.cols, self.view(wname), None, T[out], n * oh * ow, cout, kpad, self.ws, self.ws_bytes, st)
            return
        # ... under bf16 storage: bf16 columns, then a 1x1 conv of kpad channels
        call('fte_im2col_first_s16', T[inp], self.cols, n, ih, iw, cin, k, stride, kpad, st)
        if w.packs_pending:                            # the rest of the filter packs, from here on (_start_packs)
            w.pack_ev = self._side_packs(w)
        if w.is_training and j in self.fuse_fwd:
            bj = self.fuse_fwd[j]
            call('fte_conv2d_bn_fwd', self.cols, self.w16t[wname], T[out], *self._bn_args(self.plan[bj], w.upd), None, None, None,
                 n, oh, ow, kpad, cout, 1, 1, 1, self.ws, self.ws_bytes, st)
            w.stats_done.add(bj)
        else:
            call('fte_conv2d_fwd_s16', self.cols, self.w16t[wname], None, None, None, None, T[out], None, None,
                 n, oh, ow, kpad, cout, 1, 1, self.ws, self.ws_bytes, st)

    def _bwd_conv(self, w, op, dy):
        call, T, s16, n, st, G = w.call, self.t, w.s16, w.n, w.st, w.G
        out, inp, wname, stride = op.out, op.inp, op.wname, op.stride
        ih, iw, cin = self.shapes[inp]
        k = self.spec[wname][0][0]
        cout = self.shapes[out][-1]
        gw = self.view(wname, self.grads)
        if cin < 32 and self._direct_stem(k, cin, cout):
            call('fte_conv3x3_first_wgrad' + w.sfx, T[inp], dy, gw, n, ih, iw, cin, cout, stride, self.ws, self.ws_bytes, st)
            return
        if cin < 32:                             # stem: filter gradient only
            oh, ow, _ = self.shapes[out]
            if s16:
                call('fte_conv2d_wgrad16', self.cols, dy, gw, n, oh, ow, stem_kpad(k, cin), cout, 1, 1, self.ws, self.ws_bytes, st)
            else:
                call('fte_gemm_tn', self.cols, dy, gw, n * oh * ow, cout, stem_kpad(k, cin), self.ws, self.ws_bytes, st)
            return
        self._wgrad(w, 'fte_conv2d_wgrad16' if s16 else 'fte_conv2d_wgrad', dy, T[inp], dy, gw, n, ih, iw, cin, cout, k, stride, w.wws, self.ws_bytes, w.wst)
        self._flush(w, self.side_batch)
        prev = G.pop(inp, None)                  # accumulate into an existing contribution through `addin`
        dx = self._new(inp)
        bnb = self._bn_below(w, inp) if self.fuse_bwd_conv else None
        if bnb is not None:          # the last contribution to the gradient of a BN output: mask + BN sums in the epilogue
            ins, outs = bnb
            call('fte_conv2d_dgrad_bn', dy, self.w16[wname] if s16 else self.view(wname), prev, *ins, dx, *outs,
                 n, ih, iw, cin, cout, k, stride, 1 if s16 else 0, self.ws, self.ws_bytes, st)
            w.reduced.add(inp)
        else:          # bf16 storage: bf16 dz in, bf16 dx out (+ the bf16 contribution already there); the HWIO pack is this step's
            call('fte_conv2d_dgrad' + w.sfx, dy, self.w16[wname] if s16 else self.view(wname), prev, None, None, None, dx, None, None,
                 n, ih, iw, cin, cout, k, stride, self.ws, self.ws_bytes, st)
        G[inp] = dx

    def _alloc_gconv(self, w, op):
        n, q = w.n, _lib.query
        self._alloc_out(w, op, True)
        self._reads16(w, op, op.inp)
        ih, iw, cc = self.shapes[op.inp]
        w.need = max(w.need, q('fte_gconv3x3_wgrad_ws_bytes', n, ih, iw, cc, op.groups, op.stride))
        if cc % 32 == 0 and cc // op.groups in (4, 8, 16, 32):
            w.need = max(w.need, q('fte_gconv3x3_wgrad_bf16_ws_bytes', n, ih, iw, cc, op.groups, op.stride),
                         q('fte_gconv3x3_bn_ws_bytes', n, ih, iw, cc, op.stride))

    def _fwd_gconv(self, w, j, op):
        call, T, s16, n, st = w.call, self.t, w.s16, w.n, w.st
        out, inp, wname, stride, groups = op.out, op.inp, op.wname, op.stride, op.groups
        ih, iw, c = self.shapes[inp]
        pk = self._gconv_pack(op)
        if pk is None:
            call('fte_gconv3x3_fwd', T[inp], self.view(wname), T[out], n, ih, iw, c, groups, stride, st)
            return
        # bf16 MFMA mode: block-diagonal slices on the matrix cores
        if not s16 or self.side is None or self.packs.head_names == set(self.w16t):
            call('fte_gconv3x3_pack_bf16', self.view(wname), pk[0], pk[1], c, groups, st)
        elif w.pack_ev is not None:                  # (packed on the side stream at the start of the walk)
            self._wait_packs(w)
        if s16 and w.is_training and j in self.fuse_fwd and self.fuse_3x3:
            bj = self.fuse_fwd[j]
            xin, isc, ish, yside = self._fold_args(w, j)
            call('fte_gconv3x3_bn_fwd_bf16_s16', xin, pk[0], T[out], *self._bn_args(self.plan[bj], w.upd), isc, ish, yside, n, ih, iw, c, stride,
                 self.ws, self.ws_bytes, st)
            w.stats_done.add(bj)
        else:
            call('fte_gconv3x3_bf16' + w.sfx, T[inp], pk[0], T[out], n, ih, iw, c, stride, 0, st)

    def _bwd_gconv(self, w, op, dy):
        call, T, s16, n, st = w.call, self.t, w.s16, w.n, w.st
        inp, wname, stride, groups = op.inp, op.wname, op.stride, op.groups
        ih, iw, c = self.shapes[inp]
        pk = self._gconv_pack(op)
        self._wgrad(w, ('fte_gconv3x3_wgrad_bf16' + w.sfx) if pk is not None else 'fte_gconv3x3_wgrad',      # (bf16 MFMA mode, or the vector kernel)
                    dy, T[inp], dy, self.view(wname, self.grads), n, ih, iw, c, groups, stride, w.wws, self.ws_bytes, w.wst)
        dx = self._new(inp)
        bnb = self._bn_below(w, inp) if (pk is not None and s16 and self.fuse_bwd_gconv) else None
        if bnb is not None:                      # ... with the mask / sums of the BN layer below in the epilogue
            (zbn, _, gam, mean, rstd, sc, sh), outs = bnb
            call('fte_gconv3x3_dgrad_bn_bf16_s16', dy, pk[1], zbn, gam, mean, rstd, sc, sh, dx, *outs, n, ih, iw, c, stride,
                 self.ws, self.ws_bytes, st)
            w.reduced.add(inp)
        elif pk is not None:                     # packed by this step's forward pass (the weights have not changed since)
            call('fte_gconv3x3_bf16' + w.sfx, dy, pk[1], dx, n, ih, iw, c, stride, 1, st)
        else:
            call('fte_gconv3x3_dgrad', dy, self.view(wname), dx, n, ih, iw, c, groups, stride, st)
        self._put(inp, dx)

    def _alloc_dwconv(self, w, op):
        self._alloc_out(w, op, True)
        self._reads16(w, op, op.inp)
        ih, iw, cc = self.shapes[op.inp]
        w.need = max(w.need, _lib.query('fte_dwconv3x3_wgrad_ws_bytes', w.n, ih, iw, cc, op.stride))

    def _fwd_dwconv(self, w, j, op):
        ih, iw, c = self.shapes[op.inp]
        w.call('fte_dwconv3x3_fwd' + w.sfx, self.t[op.inp], self.view(op.wname), self.t[op.out], w.n, ih, iw, c, op.stride, w.st)

    def _bwd_dwconv(self, w, op, dy):
        inp, wname, n = op.inp, op.wname, w.n
        ih, iw, c = self.shapes[inp]
        self._wgrad(w, 'fte_dwconv3x3_wgrad' + w.sfx, dy, self.t[inp], dy, self.view(wname, self.grads), n, ih, iw, c, op.stride, w.wws, self.ws_bytes, w.wst)
        dx = self._new(inp)
        w.call('fte_dwconv3x3_dgrad' + w.sfx, dy, self.view(wname), dx, n, ih, iw, c, op.stride, w.st)
        self._put(inp, dx)

    def _alloc_gather(self, w, op):
        for name, _ in op.outs:
            self._alloc_out(w, op, True, name)

    def _fwd_gather(self, w, j, op):
        call, T, st = w.call, self.t, w.st
        a, b = op.ins
        fa, fb = self.folded.get(a), self.folded.get(b)
        outs = op.outs
        if fa is None and fb is None and len(outs) == 1:
            name, table = outs[0]
            co = self.shapes[name][-1]
            call('fte_channel_gather' + w.sfx, T[a], T[b] if b else None, T[name], table, T[name].numel() // co,
                 self.shapes[a][-1], self.shapes[b][-1] if b else 0, co, st)
        else:                                          # both halves in one launch, BN applied to a folded source
            sa = (T[fa[0]], self.bn[a]['scale'], self.bn[a]['shift'], fa[1]) if fa else (T[a], None, None, 0)
            sb = (T[fb[0]], self.bn[b]['scale'], self.bn[b]['shift'], fb[1]) if fb else (T[b] if b else None, None, None, 0)
            (n0, t0), (n1, t1) = outs[0], (outs[1] if len(outs) > 1 else (None, None))
            co0 = self.shapes[n0][-1]
            call('fte_channel_gather_affine' + w.sfx, sa[0], sb[0], T[n0], t0, co0, T[n1] if n1 else None, t1,
                 self.shapes[n1][-1] if n1 else 0, T[n0].numel() // co0, self.shapes[a][-1],
                 self.shapes[b][-1] if b else 0, sa[1], sa[2], sa[3], sb[1], sb[2], sb[3], st)

    def _bwd_gather(self, w, op, da):
        call, st, G = w.call, w.st, w.G
        gb = op.gouts[1]
        db = G.pop(gb) if gb else None
        gs = [(name, table, torch.empty((w.n,) + self.shapes[name], dtype=torch.int16 if w.s16 else torch.float32, device=self.device))
              for name, table in op.bwd]
        (n0, t0, g0), (n1, t1, g1) = gs[0], (gs[1] if len(gs) > 1 else (None, None, None))
        co0 = self.shapes[n0][-1]
        if g1 is None:
            call('fte_channel_gather' + w.sfx, da, db, g0, t0, g0.numel() // co0, da.shape[-1],
                 db.shape[-1] if db is not None else 0, co0, st)
        else:                                    # the gradients of both sources in one launch
            call('fte_channel_gather_affine' + w.sfx, da, db, g0, t0, co0, g1, t1, self.shapes[n1][-1], g0.numel() // co0,
                 da.shape[-1], db.shape[-1] if db is not None else 0, None, None, 0, None, None, 0, st)
        for name, _, g in gs:
            self._put(name, g)

    def _alloc_bnstats(self, w, op):
        self._alloc_bn(w, op, stored=False)              # (applied inside the gather that consumes it: the output is never stored)

    def _fwd_bnstats(self, w, j, op):
        if j not in w.stats_done:
            self._bn_stats(w, op, self.t[op.inp], op.inp in self.h16)

    def _fwd_bn(self, w, j, op):
        call, T, s16, st = w.call, self.t, w.s16, w.st
        out, inp, res, relu = op.out, op.inp, op.res, op.relu
        b = self.bn[out]
        c = self.shapes[out][-1]
        rows = T[out].numel() // c
        resbuf = T[res] if res is not None else None
        if res is not None:
            self._wait_shortcut(w, res)
            assert not s16 or res in self.h16, 'bf16 storage: the shortcut of %s is an fp32 tensor' % out
        if j in w.stats_done and self._folds(w, j):  # ... which the consumer's operand loader takes over (it also writes T[out])
            w.folded_in[self.fold_apply[j]] = j
        elif j in w.stats_done:            # scale / shift are there already: the normalise pass alone
            call('fte_bn_apply', T[inp], b['scale'], b['shift'], resbuf, T[out], rows, c, relu, self._sflag(w, inp), st)
        elif w.is_training:
            ba = self._bn_args(op, w.upd)
            args = (T[inp], ba[0], ba[1], resbuf, T[out]) + ba[2:8] + (rows, c, ba[8], ba[9], relu)
            if s16:
                call('fte_bn_train_fwd_s16', *args, self._sflag(w, inp), w.ws, self.ws_bytes, st)
            else:
                call('fte_bn_train_fwd', *args, w.ws, self.ws_bytes, st)
        else:
            ba = self._bn_args(op, True)
            args = (T[inp], ba[0], ba[1], ba[6], ba[7], resbuf, T[out], b['scale'], b['shift'], rows, c, self.bn_eps, relu)
            if s16:
                call('fte_bn_infer_fwd_s16', *args, self._sflag(w, inp), st)
            else:
                call('fte_bn_infer_fwd', *args, st)
        if w.on_side:
            w.sc_ev[out] = w.side.record_event()

    def _bwd_bn(self, w, op, dy):
        call, T, st = w.call, self.t, w.st
        out, inp, pre, res, relu = op.out, op.inp, op.pre, op.res, op.relu
        b = self.bn[out]
        c = self.shapes[out][-1]
        rows = dy.numel() // c
        dz = torch.empty_like(T[inp])
        gam, dgam, dbet = self.view(pre + '/gamma'), self.view(pre + '/gamma', self.grads), self.view(pre + '/beta', self.grads)
        tail = (rows, c, self.ws, self.ws_bytes, st)
        if out in w.reduced:             # dy is the masked gradient already, dgamma / dbeta / coef are there: the apply pass alone
            call('fte_bn_bwd_apply', dy, T[inp], b['coef'], dz, rows, c, 3 if w.s16 else 0, st)
            if res is not None:
                self._put(res, dy)               # the shortcut sees the same (read-only) masked gradient
        elif w.s16:                      # one entry point: y (the mask of a residual BN), scale / shift (the mask recomputed from z) or neither
            g = self._new(out) if res is not None else None
            zmask = relu and res is None
            call('fte_bn_train_bwd_s16', dy, T[out] if res is not None else None, T[inp], gam, b['mean'], b['rstd'],
                 b['scale'] if zmask else None, b['shift'] if zmask else None, g, dz, dgam, dbet, rows, c, self._sflag(w, inp), self.ws, self.ws_bytes, st)
            if res is not None:
                self._put(res, g)
        elif res is not None and not relu:         # BN + shortcut, no activation: dy goes unmasked into the BN backward and
            call('fte_bn_train_bwd', dy, None, T[inp], gam, b['mean'], b['rstd'], dz, dgam, dbet, *tail)      # unchanged (no copy) to the shortcut
            self._add(res, dy)
        elif res is not None:                      # the shortcut gets g = dy * (out > 0): a by-product of the reduce pass
            g = self._new(out)
            call('fte_bn_train_bwd_res', dy, T[out], T[inp], gam, b['mean'], b['rstd'], g, dz, dgam, dbet, *tail)
            self._put(res, g)
        elif relu:                                 # ReLU mask recomputed from z: the output is not read
            call('fte_bn_train_bwd_zmask', dy, T[inp], gam, b['mean'], b['rstd'], b['scale'], b['shift'], dz, dgam, dbet, *tail)
        else:
            call('fte_bn_train_bwd', dy, None, T[inp], gam, b['mean'], b['rstd'], dz, dgam, dbet, *tail)
        if inp in self.shortcut_shared:
            self._add(inp, dz)               # ... plus the gradient the shortcut passed on
        else:
            self._put(inp, dz)

    _bwd_bnstats = _bwd_bn

    def _alloc_bnprelu(self, w, op):
        w.need = max(w.need, _lib.query('fte_bn_prelu_ws_bytes', self.shapes[op.out][-1]))
        self._alloc_bn(w, op)

    def _fwd_bnprelu(self, w, j, op):
        T = self.t
        x, y = T[op.inp], T[op.out]
        b = self.bn[op.out]
        c = self.shapes[op.out][-1]
        rows = y.numel() // c
        if not w.is_training:                            # moving statistics -> scale / shift, then the apply (fte.h)
            ba = self._bn_args(op, True)
            w.call('fte_bn_prelu_infer_fwd', x, ba[0], ba[1], ba[6], ba[7], self.view(op.alpha), y, b['scale'], b['shift'], rows, c, self.bn_eps, w.st)
            return
        if j not in w.stats_done:                    # (else the producing conv's epilogue left the batch statistics)
            self._bn_stats(w, op, x, False)
        w.call('fte_bn_prelu_apply', x, b['scale'], b['shift'], self.view(op.alpha), y, rows, c, w.st)

    def _bwd_bnprelu(self, w, op, dy):
        inp, pre, alpha = op.inp, op.pre, op.alpha
        b = self.bn[op.out]
        c = self.shapes[op.out][-1]
        dz = torch.empty_like(self.t[inp])
        w.call('fte_bn_prelu_train_bwd', dy, self.t[inp], self.view(pre + '/gamma'), b['mean'], b['rstd'], b['scale'], b['shift'], self.view(alpha),
               dz, self.view(pre + '/gamma', self.grads), self.view(pre + '/beta', self.grads), self.view(alpha, self.grads), dy.numel() // c, c,
               self.ws, self.ws_bytes, w.st)
        self._put(inp, dz)

    def _alloc_seblock(self, w, op):
        self._alloc_out(w, op, True)
        self._reads16(w, op, op.inp, op.shortcut)
        self._alloc_bn(w, op, stored=False)
        c = self.shapes[op.out][-1]
        for nm in ('xm', 's1', 's2'):                  # per-image sums of the backward pass, the squeeze in xhat units
            self.t[op.out + '/' + nm] = self._f32(w.n, c)
        self._alloc_se_gate(w, op.out, op.se, c)

    def _fwd_seblock(self, w, j, op):
        call, T, n, st = w.call, self.t, w.n, w.st
        out, zin, scn, se = op.out, op.inp, op.shortcut, op.se
        ih, iw, c = self.shapes[out]
        hw = ih * iw
        b = self.bn[out]
        fl = self._sflag(w, zin)
        if j not in w.stats_done:                      # (else the producing conv's epilogue left the batch statistics)
            self._bn_stats(w, op, T[zin], zin in self.h16)
        sq, _, gate = self._se_buffers(out)
        call('fte_se_squeeze', T[zin], b['scale'], b['shift'], b['mean'], b['rstd'], sq, T[out + '/xm'] if w.is_training else None,
             n, hw, c, fl & 1, st)
        self._se_gate_fwd(w, out, se, c, 'small' if self._se_small(c, se.hidden) else 'act')
        self._wait_shortcut(w, scn)
        call('fte_se_apply_fwd', T[zin], b['scale'], b['shift'], gate, T[scn], T[out], n, hw, c, fl, st)

    def _bwd_seblock(self, w, op, dy):
        call, T, n, st = w.call, self.t, w.n, w.st
        out, zin, pre, se = op.out, op.inp, op.pre, op.se
        ih, iw, c = self.shapes[out]
        hw = ih * iw
        b = self.bn[out]
        fl = self._sflag(w, zin)
        gate = T[out + '/gate']
        s1, s2, xm = T[out + '/s1'], T[out + '/s2'], T[out + '/xm']
        gam, bet = self.view(pre + '/gamma'), self.view(pre + '/beta')
        g = self._new(out)                             # dy * (out > 0): the shortcut's gradient, and the gate path's input
        call('fte_se_bwd_gate', dy, T[out], T[zin], gam, bet, b['mean'], b['rstd'], gate, g, s1, s2, self.ident[('se', out, 'dgate')], n, hw, c, fl, st)
        dsq = self._se_gate_bwd(w, out, se, c, self._se_small(c, se.hidden))
        call('fte_se_bn_bwd_coef', s1, s2, gate, dsq, xm, gam, b['mean'], b['rstd'], self.view(pre + '/gamma', self.grads),
             self.view(pre + '/beta', self.grads), b['coef'], n, hw, c, st)
        dz = torch.empty_like(T[zin])
        call('fte_se_bn_bwd_apply', g, T[zin], b['coef'], gate, dsq, dz, n, hw, c, fl, st)
        self._put(op.shortcut, g)
        self._put(zin, dz)

    def _alloc_selin(self, w, op):
        assert not w.s16, 'selin: fp32 tensors only (the nets that plan it refuse bf16 storage)'
        self._alloc_out(w, op, False)
        self._alloc_bn(w, op, stored=False)
        ih, iw, c = self.shapes[op.out]
        for nm in ('xm', 's1', 's2'):                  # per-image sums of the backward pass, the squeeze in xhat units
            self.t[op.out + '/' + nm] = self._f32(w.n, c)
        self._alloc_se_gate(w, op.out, op.se, c)
        w.need = max(w.need, _lib.query('fte_se_lin_ws_bytes', w.n, ih * iw, c))

    def _fwd_selin(self, w, j, op):
        """BN -> SE gate -> + shortcut, no activation: statistics, squeeze, the gate's dense layers, out = u * gate + shortcut"""
        call, T, n, st = w.call, self.t, w.n, w.st
        out, zin, scn, se = op.out, op.inp, op.shortcut, op.se
        ih, iw, c = self.shapes[out]
        hw = ih * iw
        b = self.bn[out]
        if j not in w.stats_done:                      # (else the producing conv's epilogue left the batch statistics)
            self._bn_stats(w, op, T[zin], False)
        sq, _, gate = self._se_buffers(out)
        call('fte_se_lin_squeeze', T[zin], b['scale'], b['shift'], b['mean'], b['rstd'], sq, T[out + '/xm'] if w.is_training else None,
             n, hw, c, w.ws, self.ws_bytes, st)
        self._se_gate_fwd(w, out, se, c, 'small' if self._se_small(c, se.hidden) else 'act')
        self._wait_shortcut(w, scn)
        call('fte_se_lin_apply_fwd', T[zin], b['scale'], b['shift'], gate, T[scn], T[out], n, hw, c, st)

    def _bwd_selin(self, w, op, dy):
        """dy is the gated tensor's gradient AND the shortcut's (passed on uncopied, as the activation-free bn op does)"""
        call, T, n, st = w.call, self.t, w.n, w.st
        out, zin, pre, se = op.out, op.inp, op.pre, op.se
        ih, iw, c = self.shapes[out]
        hw = ih * iw
        b = self.bn[out]
        gate = T[out + '/gate']
        s1, s2, xm = T[out + '/s1'], T[out + '/s2'], T[out + '/xm']
        gam, bet = self.view(pre + '/gamma'), self.view(pre + '/beta')
        call('fte_se_lin_bwd_sums', dy, T[zin], gam, bet, b['mean'], b['rstd'], gate, s1, s2, self.ident[('se', out, 'dgate')], n, hw, c,
             self.ws, self.ws_bytes, st)
        dsq = self._se_gate_bwd(w, out, se, c, self._se_small(c, se.hidden))
        call('fte_se_bn_bwd_coef', s1, s2, gate, dsq, xm, gam, b['mean'], b['rstd'], self.view(pre + '/gamma', self.grads),
             self.view(pre + '/beta', self.grads), b['coef'], n, hw, c, st)
        dz = torch.empty_like(T[zin])
        call('fte_se_bn_bwd_apply', dy, T[zin], b['coef'], gate, dsq, dz, n, hw, c, 0, st)
        self._add(op.shortcut, dy)
        self._put(zin, dz)

    def _alloc_se(self, w, op):
        self._alloc_out(w, op, True)
        self._reads16(w, op, op.inp)
        self._alloc_se_gate(w, op.out, op, self.shapes[op.out][-1])

    def _fwd_se(self, w, j, op):
        call, T, n, st = w.call, self.t, w.n, w.st
        out, inp = op.out, op.inp
        ih, iw, c = self.shapes[inp]
        sq, _, gate = self._se_buffers(out)
        call('fte_gap_fwd' + w.sfx, T[inp], sq, n, ih * iw, c, st)
        self._se_gate_fwd(w, out, op, c, 'act' if self.opt.se_act_fuse else 'plain')      # ('plain': A/B hook)
        call('fte_channel_scale_fwd' + w.sfx, T[inp], gate, T[out], n, ih * iw, c, st)

    def _bwd_se(self, w, op, dy):
        call, T, n, st = w.call, self.t, w.n, w.st
        out, inp = op.out, op.inp
        ih, iw, c = self.shapes[inp]
        hw = ih * iw
        gate = T[out + '/gate']
        dgate = self.ident[('se', out, 'dgate')]
        dx = self._new(inp)
        if w.s16:          # reduction only; dx is written once by the apply pass below
            call('fte_channel_scale_bwd_s16', dy, T[inp], gate, dgate, n, hw, c, 1, st)
        else:
            call('fte_channel_scale_bwd', dy, T[inp], gate, dx, dgate, n, hw, c, 1, st)         # dgate = d(pre-sigmoid)
        dsq = self._se_gate_bwd(w, out, op, c, False)
        if w.s16:
            call('fte_channel_scale_bwd_apply_s16', dy, gate, dsq, dx, n, hw, c, 1.0 / hw, st)
        else:
            call('fte_bcast_add', dx, dsq, n, hw, c, 1.0 / hw, st)
        self._put(inp, dx)

    def _alloc_addrelu(self, w, op):
        self._alloc_out(w, op, True)
        c = self.shapes[op.out][-1]
        if c not in self.ident:
            self.ident[c] = (torch.ones(c, dtype=torch.float32, device=self.device), torch.zeros(c, dtype=torch.float32, device=self.device))

    def _fwd_addrelu(self, w, j, op):
        T, out, a, b = self.t, op.out, op.a, op.b
        c = self.shapes[out][-1]
        one, zero = self.ident[c]
        self._wait_shortcut(w, a, b)
        args = (T[a], one, zero, zero, one, T[b], T[out], self._scr(c, 0), self._scr(c, 1), T[out].numel() // c, c, 0.0, 1)
        if w.s16:
            assert a in self.h16 and b in self.h16
            w.call('fte_bn_infer_fwd_s16', *args, 3, w.st)
        else:
            w.call('fte_bn_infer_fwd', *args, w.st)

    def _bwd_addrelu(self, w, op, dy):
        g = self._new(op.out)
        w.call('fte_relu_bwd' + w.sfx, dy, self.t[op.out], g, dy.numel(), w.st)
        self._put(op.a, g)
        self._put(op.b, g)                      # both addends see the same (read-only) gradient

    def _alloc_maxpool(self, w, op):
        shape = self._alloc_out(w, op, True)
        self._reads16(w, op, op.inp)
        self.t[op.out + '/idx'] = torch.empty(shape, dtype=torch.uint8, device=self.device)

    def _fwd_maxpool(self, w, j, op):
        T = self.t
        ih, iw, c = self.shapes[op.inp]
        w.call('fte_maxpool3x3s2_fwd' + w.sfx, T[op.inp], T[op.out], T[op.out + '/idx'], w.n, ih, iw, c, w.st)

    def _bwd_maxpool(self, w, op, dy):
        ih, iw, c = self.shapes[op.inp]
        g = self._new(op.inp)
        w.call('fte_maxpool3x3s2_bwd' + w.sfx, dy, self.t[op.out + '/idx'], g, w.n, ih, iw, c, w.st)
        self._put(op.inp, g)

    def _alloc_gap(self, w, op):
        self._alloc_out(w, op, False)

    def _fwd_gap(self, w, j, op):
        ih, iw, c = self.shapes[op.inp]
        w.call('fte_gap_fwd_s16' if op.inp in self.h16 else 'fte_gap_fwd', self.t[op.inp], self.t[op.out], w.n, ih * iw, c, w.st)

    def _bwd_gap(self, w, op, dy):
        ih, iw, c = self.shapes[op.inp]
        g = self._new(op.inp)
        w.call('fte_gap_bwd_s16' if op.inp in self.h16 else 'fte_gap_bwd', dy, g, w.n, ih * iw, c, w.st)
        self._put(op.inp, g)

    def _alloc_dropout(self, w, op):
        shape = self._alloc_out(w, op, False)
        self.t[op.out + '/mask'] = self._f32(shape)

    def _fwd_dropout(self, w, j, op):
        T = self.t
        if w.is_training:
            seed = (self.dropout_seed * 1000003 + self.global_step) & 0x7FFFFFFFFFFFFFFF
            w.call('fte_dropout_fwd', T[op.inp], T[op.out + '/mask'], T[op.out], T[op.out].numel(), op.keep, seed, w.st)
        else:
            T[op.out].copy_(T[op.inp])

    def _bwd_dropout(self, w, op, dy):
        g = self._new(op.inp)
        w.call('fte_dropout_bwd', dy, self.t[op.out + '/mask'], g, dy.numel(), op.keep, w.st)
        self._put(op.inp, g)

    def _fc_dims(self, op):
        """(inputs, outputs) of a dense layer: an 'embed_w' FC reads [n, h, w, c] as one row-major [n, h w c] operand (no bias); the
        classifier writes the padded class columns"""
        if op.embed:
            return self.spec[op.wname][0]
        return self.shapes[op.inp][0], self.sub_centers * self.cpad

    def _alloc_fc(self, w, op):
        self._alloc_out(w, op, False)
        fin, d = self._fc_dims(op)
        w.need = max(w.need, _lib.query('fte_gemm_ws_bytes', w.n, d, fin))

    def _fwd_fc(self, w, j, op):
        fin, d = self._fc_dims(op)
        w.call('fte_gemm_nn', self.t[op.inp], self.view(op.wname), None, self.t[op.out], w.n, d, fin, self.ws, self.ws_bytes, w.st)

    def _bwd_fc(self, w, op, dy):
        """a dense layer inside the body (the classifier is backward_head's)"""
        fin, d = self.spec[op.wname][0]
        x = self.t[op.inp]
        self._wgrad(w, 'fte_gemm_tn', dy, x, dy, self.view(op.wname, self.grads), w.n, d, fin, w.wws, self.ws_bytes, w.wst)
        dx = self._new(op.inp)
        w.call('fte_gemm_nt', dy, self.view(op.wname), None, None, 0, None, dx, None, w.n, d, fin, self.ws, self.ws_bytes, w.st)
        self._put(op.inp, dx)

    def _ensure_built(self, images, num_classes):
        if not self.built:
            n, h, w, ch = images.shape
            self.build(h, w, ch, num_classes, images.device)
        else:
            assert num_classes == self.num_classes, 'num_classes changed after the variables were created'

    def backbone(self, inputs, is_training=False, reuse=None):
        self._run_forward(inputs, is_training)
        return self.t[self.feature_name]

    def eval_features(self, images):
        """The extractor's output for these nets (evaluate.py): the pooled backbone features in inference mode (BN on the
        moving statistics, no dropout).  The reference's ResNet.forward asserts num_classes even for is_training=False
        (nets/resnet.py:147), so its evaluate.py:63 only ever worked for SphereNet; this is what that call was after."""
        assert self.built, 'build() / restore the variables first'
        return self.backbone(images, is_training=False)

    def forward(self, images, num_classes=None, is_training=True):
        assert num_classes is not None, 'num_classes must be given when is_training=True'   # nets/resnet.py:147
        self._ensure_built(images, num_classes)
        self._run_forward(images, is_training)
        out = {'features': self.t[self.feature_name]}
        if self.has_classifier:
            out['logits'] = self.t['logits'][:, :self.num_classes]
        return out

    # ---- loss -------------------------------------------------------------------------------------------
    def _centers(self):
        if 'centers' not in self.state:          # loss.py:34-35: zeros, non-trainable
            d = self.shapes[self.feature_name][0]
            self.state['centers'] = torch.zeros(self.num_classes, d, dtype=torch.float32, device=self.device)
        return self.state['centers']

    def _reconcile_centers(self, comm, labels, n, d):
        """Opt-in (DataParallel(sync_centers=True)): one `centers` table for all replicas.  The reference creates the table inside
        every tower's variable scope and each tower scatter_subs only ITS shard (loss.py:34-39), so its replicas drift apart
        silently (SURVEY.md 8e caveat).  Here every rank has evaluated loss and gradient against the OLD table without touching it;
        the ranks all-gather their (labels, f - c_y) rows -- n x (d + 1) words per rank, the sparse rows only, never the table --
        and each applies ALL rows in rank order with the deterministic scatter kernel: tables stay bit-identical across replicas and
        equal the single-tower update of the GLOBAL batch."""
        world = comm.world_size()
        diff = self.ws[:n * d]
        all_diff = torch.empty(world * n * d, dtype=torch.float32, device=self.device)
        all_lab = torch.empty(world * n, dtype=torch.int32, device=self.device)
        comm.all_gather(all_diff, diff)
        comm.all_gather(all_lab, labels)
        _lib.call('fte_center_scatter_update', all_diff, all_lab, self._centers(), world * n, d, self.num_classes,
                  self.center_alpha, _stream())

    def loss_function(self, scope, labels, **logits):
        """nets/resnet.py:163-176 + Network._regularize; the center / triplet terms are loss.py's functions wired to
        the pooled features (the reference leaves that wiring to the caller)."""
        labels = heads.check_labels(labels)
        n = labels.shape[0]
        st = _stream()
        call = _lib.call
        slots = self.loss_slots
        feat = self.t[self.feature_name]
        d = feat.shape[1]
        losses, names = [], []
        self._dfeat = None
        if self.head == 'triplet':
            soft = self.triplet_margin is None                                  # loss.py:74-77: None -> softplus, any number -> hinge
            call('fte_batch_hard_triplet_fwd_bwd', feat, labels, 0.0 if soft else float(self.triplet_margin), int(soft), self.tower_scale / n, self.loss_rows, self.dfeat,
                 n, d, self.ws, self.ws_bytes, st)
            call('fte_sum', self.loss_rows, n, self.tower_scale / n, slots[0:1], self.ws, self.ws_bytes, st)
            self._dfeat = self.dfeat
            losses.append(slots[0]); names.append('triplet_loss')
        else:
            if self.head == 'focal':                         # loss.py:18-27 on the classifier logits
                call('fte_focal_loss_fwd_bwd', self.t['logits'], labels, self.loss_rows, self.G, n,
                     self.num_classes, self.cpad, self.focal_gamma, self.focal_alpha, self.tower_scale / n, st)
            elif self.head in NORMALISED_HEADS:              # the margin on the raw classifier output; backward_head adds the norm terms
                op = self.plan[-1]                           # (the running statistics of AdaFace and CurricularFace's t move with BN's: heads.describe)
                heads.margin_forward(self, self.t[op.inp], self.view(op.wname), self.t['logits'], labels, None, heads.describe(self), n,
                                     self.shapes[op.inp][0], self.num_classes, self.cpad, self.tower_scale / n, st)
            else:
                call('fte_softmax_ce_fwd_bwd', self.t['logits'], labels, self.loss_rows, self.G, n,
                     self.num_classes, self.cpad, self.tower_scale / n, st)
            call('fte_sum', self.loss_rows, n, self.tower_scale / n, slots[0:1], self.ws, self.ws_bytes, st)
            losses.append(slots[0]); names.append('focal_entropy' if self.head == 'focal' else 'cross_entropy')
            if self.head == 'magface':                       # lambda_g * mean g; cross_entropy above stays the pure CE
                call('fte_sum', self.reg_rows, n, self.magface[4] * self.tower_scale / n, slots[2:3], self.ws, self.ws_bytes, st)
                losses.append(slots[2]); names.append('magnitude_loss')
            if self.head == 'softmax+center':
                comm = self.center_comm if self.update_centers else None
                call('fte_center_loss_fwd_bwd_update', feat, labels, self._centers(), self.loss_rows, self.dfeat, n, d, self.num_classes,
                     self.center_alpha if (self.update_centers and comm is None) else 1.0,      # alpha = 1: loss + gradient only
                     self.center_weight * self.tower_scale / (n * d), self.ws, self.ws_bytes, st)
                if comm is not None:
                    self._reconcile_centers(comm, labels, n, d)
                call('fte_sum', self.loss_rows, n, self.tower_scale / (n * d), slots[2:3], self.ws, self.ws_bytes, st)
                self._dfeat = self.dfeat
                losses.append(slots[2]); names.append('center_loss')
        if getattr(self, '_reg_ev', None) is not None and self._reg_scale == 0.5 * self.weight_decay * self.tower_scale:
            torch.cuda.current_stream().wait_event(self._reg_ev)           # taken on the side stream at the start of this forward pass
            self._reg_ev = None
            call('fte_axpby', 1.0, self._reg_scratch[0:1], 0.0, self._reg_scratch[0:1], slots[1:2], 1, st)
        else:
            self._reg_ev = None
            nreg = self.arena_size - self.small_end
            call('fte_sumsq', self.params[self.small_end:], nreg, 0.5 * self.weight_decay * self.tower_scale,
                 slots[1:2], self.ws, self.ws_bytes, st)
        losses.append(slots[1]); names.append('reg_loss')
        return losses, names, OrderedDict()

    # ---- backward ---------------------------------------------------------------------------------------
    def backward(self):
        if self.has_classifier:
            self.backward_head(join=False)               # (backward_body joins the side stream when it returns)
        self.backward_body()

    def backward_stages(self):
        """One callable per all-reduce bucket of grad_buckets(), in the order the backward walk completes them: the classifier, then
        the body in segments from the last layers to the first (data_parallel.py:88-113 issues one nccl.all_sum per variable, which TF
        schedules as each gradient becomes ready; here every segment's filter gradients are final -- side stream joined -- when its
        callable returns, and DataParallel enqueues that bucket's all-reduce while the next segment still runs)."""
        segs = self._segments()
        body = [(lambda lo=lo, hi=hi: self.backward_body(lo, hi)) for lo, hi, _, _ in reversed(segs)]
        return ([self.backward_head] if self.has_classifier else []) + body

    def _segments(self):
        """[(plan lo, plan hi, arena a, arena b)] in forward order: the body's all-reduce buckets (plan.segments)"""
        if getattr(self, '_segs', None) is None:
            self._segs = plan.segments(self.plan, self.variables, self.small_end, self.cls_start, self.has_classifier, self.opt.grad_buckets)
        return self._segs

    def backward_head(self, join=True):
        """Classifier gradient (first all-reduce bucket) and the gradient wrt its input.  The filter gradient goes to the side stream
        like every other one (nothing but the optimizer / the bucket's all-reduce reads it); `join`: the main stream waits for it before
        this returns (backward_stages: the bucket is reduced next)."""
        n = self._act_n
        st = _stream()
        op = self.plan[-1]
        k = self.shapes[op.inp][0]
        self._grad = {}
        gin = torch.empty(n, k, dtype=torch.float32, device=self.device)
        side = self.side if self.opt.head_side else None
        norm = self.head in NORMALISED_HEADS             # their norm corrections ride on the stream of the product they correct
        x, W = self.t[op.inp], self.view(op.wname)
        wst, wws = st, self.ws
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_event(main.record_event())         # G (the loss head's gradient) and the features are complete
            wst, wws = side.cuda_stream, self.ws_side
        heads.classifier_dw(self, x, W, self.view(op.wname, self.grads), n, k, self.sub_centers * self.cpad, wws, self.ws_bytes, wst, norm)      # (before the bucket is reduced)
        heads.classifier_dx(self, x, W, gin, n, k, self.sub_centers * self.cpad, self.ws, self.ws_bytes, st, norm)
        if side is not None and join:
            torch.cuda.current_stream().wait_stream(side)
        self._grad[op.inp] = gin


    def _put(self, name, g):
        if name in self._grad:
            raise RuntimeError('gradient of %s already has a contribution that cannot be accumulated in place' % name)
        self._grad[name] = g

    def _add(self, name, g):
        """_put, or -- a tensor read by a BN and by a shortcut (the IResNet block's input) -- the sum of the two contributions.  The
        one already there may be shared with another tensor's gradient (a shortcut passes its gradient on without a copy), so the
        sum goes to whichever buffer is the walk's own: `g` when it is a fresh BN dz, else a new one."""
        assert name in self.shortcut_shared, name
        prev = self._grad.get(name)
        if prev is None:
            self._grad[name] = g
            return
        assert prev.dtype == torch.float32 and g.dtype == torch.float32 and prev.shape == g.shape, name
        out = g if self._own(g) else torch.empty_like(g)
        _lib.call('fte_axpby', 1.0, g, 1.0, prev, out, g.numel(), _stream())
        self._grad[name] = out

    def _own(self, g):
        """is `g` referenced by no other entry of the gradients in flight?"""
        return not any(v is g for v in self._grad.values())

    # ---- bookkeeping the wrappers use ---------------------------------------------------------------------
    def param_list(self, is_training, trainable, scope=None):
        """nets/resnet.py:178-184: trainable=True -> tf.trainable_variables(scope), trainable=False ->
        tf.global_variables(scope), which also holds the scope's BatchNorm moving statistics (what the fine-tune
        saver of train.py:191-193 restores through pretrained_param)."""
        bb = [v for k, v in self.variables.items() if k.startswith(self.name + '/')]
        if not trainable:
            bb = bb + [Variable(k, 'state', (self.state_ref.get(k, t.shape[0]),), -1, self.state_ref.get(k, t.shape[0]))
                       for k, t in self.state.items() if k.startswith(self.name + '/')]
        if is_training:
            return [bb, [v for k, v in self.variables.items() if k.startswith('classifier/')]]
        return [bb]

    def pretrained_param(self, scope=None):
        return [v for grp in self.param_list(is_training=False, trainable=False, scope=scope) for v in grp if self.name in v.name]

    def arena_groups(self):
        groups = [(0, self.small_end, False, 0), (self.small_end, self.cls_start, True, 0)]
        if self.has_classifier:
            groups.append((self.cls_start, self.arena_size, True, 1))
        return groups

    def grad_buckets(self):
        """arena ranges of backward_stages()'s callables, in the same order; the four loss slots behind the arena ride on the bucket
        that ends at the arena's end"""
        segs = self._segments()
        body = [(a, b) for _, _, a, b in reversed(segs)]
        if self.has_classifier:
            return [(self.cls_start, self.arena_size + 4)] + body
        body[0] = (body[0][0], self.arena_size + 4)          # (cls_start == arena_size: the last segment ends the arena)
        return body
