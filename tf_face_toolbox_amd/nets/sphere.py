"""SphereNet-20 ("SphereFaceNet-20") on libfte.so -- host-side mirror of nets/sphere.py.

Reference: nets/sphere.py:23-134 (class SphereNet: prelu :29-36, resBlock :38-45, backbone
:47-76, forward :78-101, loss_function :103-118, param_list :120-126, pretrained_param
:128-134).  Same constructor / method names and argument meaning; the bodies enqueue HIP
kernels instead of building TF graph nodes.

MI355X-first layout decisions (engine-internal; the boundary keeps the reference layouts):
  * activations are NHWC fp32 end to end -- the NHWC->NCHW transpose of nets/sphere.py:53-54
    disappears; with data_format='NCHW' only the ROW ORDER of the 25088x512 FC weight differs
    (flatten order C,H,W vs H,W,C, nets/sphere.py:72) and that is permuted on import/export;
  * all parameters live in ONE flat fp32 arena  [biases+alphas | conv W (HWIO) | FC W | classifier W],
    gradients and optimizer slots in arenas of the same layout: one fused optimizer launch per
    decay group and one (bucketed) RCCL all-reduce instead of 47 (data_parallel.py:179);
  * the classifier is padded to a multiple of 128 columns (zero weights, masked in the loss);
  * every conv keeps z (pre-activation) and y = PReLU(z) (+shortcut): backward needs sign(z)
    and min(z,0) exactly, for any alpha.
"""
import os
from collections import OrderedDict, namedtuple

import torch

from .. import _lib, heads
from ..loss import sample_size
from .net_base import (NORMALISED_HEADS, Network, adaface_params, adaface_state, curricular_params, curricular_state, magface_params,
                       margin_params, side_stream)
from .sphere_plan import StageRing, split_point, wino_plan

NUM_BLOCKS = (1, 2, 4, 1)     # nets/sphere.py:58,62,66,70
EMBED = 512                   # nets/sphere.py:73

Options = namedtuple('Options', [
    'bf16_copies',      # FTE_BF16_COPIES (1): in the bf16 MFMA mode the convs read bf16 copies of their operands (net.bf16_copies starts here)
    'wino_keep',        # FTE_WINO_KEEP (1): a Winograd layer's forward leaves the V pack of its input for its filter gradient
    'wino_lean',        # FTE_WINO_LEAN (1): the first conv of a block whose two convs keep a pack writes no y (the library reads it too)
    'side_stream',      # FTE_SIDE_STREAM (unset: 'size'): filter gradients on a second stream: 0 'off', 1 'forced', else where it pays
    'fwd_halves',       # FTE_FWD_HALVES (unset: 'auto'): forward walk as two part shards: 0 'off', 1 'forced', else from fwd_halves_min
    'fwd_split',        # FTE_FWD_SPLIT (unset: None): images in the first part shard instead of the planned split point
    'fwd_halves_min',   # FTE_FWD_HALVES_MIN (128): smallest shard the 'auto' part-shard walk takes
    'dz_buffers',       # FTE_DZ_BUFFERS (3, at least 2): dz buffers per stage: with 3, wgrad(l) may still read its dz while dgrad(l - 1) writes
])

# what one pass may use, resolved by the forward walk for the backward walk of the same pass: the activations were kept (training);
# bf16 storage; the convs read bf16 copies (storage included); the Winograd layers kept their V packs; ... and the lean blocks wrote no y
Mode = namedtuple('Mode', 'keep s16 copies vpack lean')

LayerViews = namedtuple('LayerViews', 'w b a')       # a conv's filter, bias (or None) and alpha in one of the arenas, made once in build()

PLAIN, KEEP, LEAN_FIRST, LEAN_SECOND = range(4)      # a layer's forward launch in the fp32 training walk (_wino_tables)


def read_options(env=None):
    """SphereNet's switches as one immutable record.  SphereNet.__init__ calls this, so a switch acts on the nets constructed after
    it is set (the precision mode and fte_set_conv_algo are not among them: they are asked of _lib at every step)."""
    env = os.environ if env is None else env
    three = lambda k, other: {'0': 'off', '1': 'forced'}.get(env.get(k), other)
    return Options(
        bf16_copies=env.get('FTE_BF16_COPIES', '1') != '0', wino_keep=env.get('FTE_WINO_KEEP', '1') != '0',
        wino_lean=env.get('FTE_WINO_LEAN', '1') != '0', side_stream=three('FTE_SIDE_STREAM', 'size'),
        fwd_halves=three('FTE_FWD_HALVES', 'auto'), fwd_split=int(env['FTE_FWD_SPLIT']) if 'FTE_FWD_SPLIT' in env else None,
        fwd_halves_min=int(env.get('FTE_FWD_HALVES_MIN', '128')), dz_buffers=max(2, int(env.get('FTE_DZ_BUFFERS', '3'))))


def same_pads(in_size, k, stride):
    out = -(-in_size // stride)
    total = max((out - 1) * stride + k - in_size, 0)
    return out, total // 2, total - total // 2


class _Conv(object):
    __slots__ = ('name', 'stage', 'stride', 'has_bias', 'second', 'cin', 'cout', 'hin', 'win', 'hout', 'wout')

    @property
    def tiles(self):
        """2x2-output Winograd tiles per image of the layer's input"""
        return ((self.hin + 1) // 2) * ((self.win + 1) // 2)


class Variable(object):
    """A named view of the parameter arena, addressed by the reference's TF variable name."""

    def __init__(self, name, kind, ref_shape, offset, size):
        self.name, self.kind, self.ref_shape, self.offset, self.size = name, kind, tuple(ref_shape), offset, size

    def __repr__(self):
        return '<Variable %s %s>' % (self.name, self.ref_shape)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class SphereNet(Network):
    head = 'softmax'

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0):
        super(SphereNet, self).__init__(weight_decay, data_format, name)
        self.num_outputs = [64, 128, 256, 512]
        self.seed = seed
        self.built = False
        # in the bf16 MFMA mode the convs read bf16 COPIES of their operands (written by the producing epilogue / packed
        # once per step) through fte_conv2d_*16: bit-identical to the operand mode, half the bytes through the load path
        self.options = read_options()
        self.bf16_copies = self.options.bf16_copies
        self.tower_scale = 1.0        # 1/num_gpus, set by the parallel wrapper (data_parallel.py:37)
        self.global_step = 0          # A-softmax lambda annealing reads it
        self.sub_centers = 1          # K centres per class (SphereNetAdditiveMargin only; fte.h "Sub-center ArcFace")
        self.one_stream = False       # True: one chain, forward and backward (bench.py's launch-record steps: a launch's duration is its own)
        self._trace_dz = None         # a dict: the backward walk leaves a copy of every layer's dz in it (scripts/trace_dz.py)
        self._act_n = self._act_key = None
        self._split_key, self._split = None, 0
        self._mode = Mode(False, False, False, False, False)
        self.packs = self.side = self._images = None

    # ------------------------------------------------------------------ construction
    def _conv_specs(self, h, w, cin):
        specs = []
        for si, nb in enumerate(NUM_BLOCKS):
            stage = '%s/conv%d' % (self.name, si + 1)
            lst = [(stage + '/Conv', 2, True, None)]
            for b in range(nb):
                blk = stage + ('/resBlock' if nb == 1 else '/Repeat/resBlock_%d' % (b + 1))
                lst += [(blk + '/Conv', 1, False, 0), (blk + '/Conv_1', 1, False, 1)]
            for nm, stride, has_bias, second in lst:
                c = _Conv()
                c.name, c.stage, c.stride, c.has_bias, c.second = nm, si, stride, has_bias, second
                c.cin, c.cout, c.hin, c.win = cin, self.num_outputs[si], h, w
                c.hout, c.wout = same_pads(h, 3, stride)[0], same_pads(w, 3, stride)[0]
                specs.append(c)
                h, w, cin = c.hout, c.wout, c.cout
        return specs

    def build(self, height, width, channels, num_classes, device='cuda'):
        """Create the variables (TF does this lazily inside the first forward())."""
        _lib.load()
        self.device = torch.device(device)
        self.in_hwc = (height, width, channels)
        self.num_classes = int(num_classes)
        self.cpad = (self.num_classes + 127) // 128 * 128
        self.convs = self._conv_specs(height, width, channels)
        self.cls_w, self.fc_w = 'classifier/fc_classifier/weights', self.name + '/fully_connected/weights'
        last = self.convs[-1]
        self.feat_hwc = (last.hout, last.wout, last.cout)
        self.fin = last.hout * last.wout * last.cout
        # ---- arena layout: [small | conv W | FC W | classifier W(padded)] ----------------
        small, big = [], []
        for c in self.convs:
            if c.has_bias:
                small.append((c.name + '/biases', 'bias', (c.cout,), c.cout))
            small.append((c.name + '/alpha', 'alpha', (c.cout,), c.cout))
            big.append((c.name + '/weights', 'conv_w', (3, 3, c.cin, c.cout), 9 * c.cin * c.cout))
        small.append((self.name + '/fully_connected/biases', 'fc_b', (EMBED,), EMBED))
        big.append((self.fc_w, 'fc_w', (self.fin, EMBED), self.fin * EMBED))
        # K centres per class: K planes of cpad columns, centre k of class j at column k * cpad + j; the reference layout packs them
        K = self.sub_centers
        big.append((self.cls_w, 'cls_w', (EMBED, K * self.num_classes), EMBED * self._head_width_stored()))
        self.variables = OrderedDict()
        off = 0
        for nm, kind, shape, size in small + big:
            self.variables[nm] = Variable(nm, kind, shape, off, size)
            off += (size + 3) // 4 * 4
        self.small_end = self.variables[big[0][0]].offset
        self.cls_start = self.variables[self.cls_w].offset
        self.fc_start = self.variables[self.fc_w].offset
        self._stage_first = [min(self.variables[c.name + '/weights'].offset for c in self.convs if c.stage == st_)
                             for st_ in sorted(set(c.stage for c in self.convs))]
        self.arena_size = off
        dev = self.device
        self.params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(off + 4, dtype=torch.float32, device=dev)      # +4: [ce, reg, -, -] loss slots
        self.loss_slots = self.grads[off:off + 4]
        views = lambda arena: [LayerViews(self.view(c.name + '/weights', arena), self.view(c.name + '/biases', arena) if c.has_bias else None,
                                          self.view(c.name + '/alpha', arena)) for c in self.convs]
        self._pv, self._gv = views(self.params), views(self.grads)      # per layer: parameters, gradients
        self.state = self._make_state()                   # non-trainable variables: outside the arena, never all-reduced
        self._init_params()
        self.built = True
        return self

    def _make_state(self):
        """name -> tensor of the head's non-trainable variables (saver.py writes them beside the weights); none for most heads"""
        return OrderedDict()

    def view(self, name, arena=None):
        v = self.variables[name]
        a = self.params if arena is None else arena
        return a[v.offset:v.offset + v.size]

    def _init_params(self):
        """Reference initialisers: nets/sphere.py:34 (alpha 0.25), :41-42 (N(0,0.01) resBlock convs),
        :87 (N(0,1e-3) classifier); layers.conv2d / fully_connected defaults = Xavier-uniform, zero bias."""
        g = torch.Generator().manual_seed(self.seed)
        for c in self.convs:
            if c.has_bias:
                lim = (6.0 / (9 * c.cin + 9 * c.cout)) ** 0.5
                w = (torch.rand(3, 3, c.cin, c.cout, generator=g) * 2 - 1) * lim
            else:
                w = torch.randn(3, 3, c.cin, c.cout, generator=g) * 0.01
            self.view(c.name + '/weights').copy_(w.reshape(-1))
            self.view(c.name + '/alpha').fill_(0.25)
        lim = (6.0 / (self.fin + EMBED)) ** 0.5
        w = (torch.rand(self.fin, EMBED, generator=g) * 2 - 1) * lim
        self.view(self.fc_w).copy_(w.reshape(-1))
        K = self.sub_centers                              # every plane drawn on its own: identical planes would tie on every sample
        wc = torch.zeros(EMBED, K, self.cpad)
        wc[:, :, :self.num_classes] = (torch.randn(EMBED, K * self.num_classes, generator=g) * 0.001).reshape(EMBED, K, self.num_classes)
        self.view(self.cls_w).copy_(self._stored_columns(wc).reshape(-1))

    def _head_width_stored(self):
        """columns of the classifier the arena holds: every plane, padded"""
        return self.sub_centers * self.cpad

    def _stored_columns(self, wc):
        """what the arena keeps of the dense classifier wc [EMBED, K, cpad]: all of it"""
        return wc

    def _head_rows(self, n):
        """rows of the head's buffers for a batch of n images: its own rows"""
        return n

    # ---- reference-layout import / export ----------------------------------------------
    def _fc_perm(self, t, to_internal):
        """FC weight rows: reference order is the flatten order of data_format (nets/sphere.py:72)."""
        if self.data_format == 'NHWC':
            return t
        h, w, c = self.feat_hwc
        if to_internal:
            return t.reshape(c, h, w, EMBED).permute(1, 2, 0, 3).reshape(self.fin, EMBED)
        return t.reshape(h, w, c, EMBED).permute(2, 0, 1, 3).reshape(self.fin, EMBED)

    def get_variable(self, name, arena=None):
        """Value of a variable (or of its gradient / slot when `arena` is given) in the REFERENCE layout."""
        if name in self.state:
            return self.state[name].clone()
        v = self.variables[name]
        t = self.view(name, arena)
        if v.kind == 'cls_w':
            return t.reshape(EMBED, self.sub_centers, self.cpad)[:, :, :self.num_classes].reshape(v.ref_shape).clone()
        if v.kind == 'fc_w':
            return self._fc_perm(t.reshape(self.fin, EMBED), False).contiguous()
        return t.reshape(v.ref_shape).clone()

    def set_variable(self, name, value, arena=None):
        """Write a reference-layout value into the variable (or into its slot of another arena)."""
        if name in self.state:
            self.state[name].copy_(torch.as_tensor(value, dtype=torch.float32).reshape(self.state[name].shape))
            return
        v = self.variables[name]
        t = torch.as_tensor(value, dtype=torch.float32).to(self.device)
        assert tuple(t.shape) == v.ref_shape, (name, tuple(t.shape), v.ref_shape)
        if v.kind == 'cls_w':
            buf = torch.zeros(EMBED, self.sub_centers, self.cpad, device=self.device)
            buf[:, :, :self.num_classes] = t.reshape(EMBED, self.sub_centers, self.num_classes)
            t = buf
        elif v.kind == 'fc_w':
            t = self._fc_perm(t, True)
        self.view(name, arena).copy_(t.reshape(-1))

    def load_params(self, params):
        for k, val in params.items():
            self.set_variable(k, val)

    # ---- buffers that depend on the batch size -----------------------------------------
    def _storage16(self):
        """bf16 STORAGE ('bf16s', fte.h): z, y, dz and the skip-path gradient live in HBM as bf16 only; the last conv layer's z / y
        (the dense layer's operands, 25088 values per image) are kept in fp32 as well."""
        return _lib.bf16_storage()

    def _alloc_acts(self, n):
        s16 = self._storage16()
        key = (s16, _lib.get_mfma_dtype(), _lib.query('fte_get_conv_algo'))      # what the workspace / V-pack sizes depend on
        if self._act_n == n and self._act_key == key:
            return
        self._act_key, self._act_s16 = key, s16
        self._alloc_forward(n, s16)
        self._alloc_backward(n, s16)
        self._wino_tables(n, s16)
        self._alloc_workspace(n)
        self._alloc_head(n)
        self._act_n = n

    def _alloc_forward(self, n, s16):
        """z / y of every layer (bf16 storage: as bf16, and in fp32 for the last layer only) and the head's buffers"""
        f32 = dict(dtype=torch.float32, device=self.device)
        last = len(self.convs) - 1
        act = lambda c, dtype: torch.empty(n, c.hout, c.wout, c.cout, dtype=dtype, device=self.device)
        self.z = [act(c, torch.float32) if not s16 or l == last else None for l, c in enumerate(self.convs)]
        self.y = [act(c, torch.float32) if not s16 or l == last else None for l, c in enumerate(self.convs)]
        self.z16 = [act(c, torch.int16) for c in self.convs] if s16 else None
        self.y16 = None                                   # allocated on first use (_alloc_copies)
        self.emb = torch.empty(n, EMBED, **f32)
        hw = self._head_width()                           # cpad; the sampled-class head: its Spad columns
        hn = self._head_rows(n)                           # n; the sharded head: the global batch
        self.s_raw, self.G = torch.empty(hn, hw, **f32), torch.empty(hn, hw, **f32)
        self.logits_buf = torch.empty(hn, hw // self.sub_centers, **f32) if self.head == 'asoftmax' or self.head in NORMALISED_HEADS else self.s_raw
        self.loss_rows, self.xn, self.rowcoef = torch.empty(hn, **f32), torch.empty(hn, **f32), torch.empty(hn, **f32)
        self.wn, self.colcoef = torch.empty(hw, **f32), torch.empty(hw, **f32)
        self.demb = torch.empty(n, EMBED, **f32)

    def _alloc_backward(self, n, s16):
        """one StageRing per stage; bf16 storage: bf16 only, the last stage keeps one fp32 dz / raw for the dense layer's backward epilogue"""
        self.bwd = []
        for si in range(len(NUM_BLOCKS)):
            c = [q for q in self.convs if q.stage == si][0]
            new = lambda k, dtype: [torch.empty(n, c.hout, c.wout, c.cout, dtype=dtype, device=self.device) for _ in range(k)]
            if s16:
                dz16 = new(self.options.dz_buffers, torch.int16)
                self.bwd.append(StageRing(dz16, new(2, torch.int16), dz16, new(2, torch.float32) if si == len(NUM_BLOCKS) - 1 else None))
            else:
                self.bwd.append(StageRing(new(self.options.dz_buffers, torch.float32), new(2, torch.float32)))

    def _algo(self, *shape_op):
        return _lib.query('fte_conv3x3_algo', *shape_op)

    def _wino_tables(self, n, s16):
        """Winograd layers (fte.h FTE_CONV_*; the reference's train.py:260): the forward pass leaves V = B^T d B of its input for the
        layer's filter gradient (fte_conv3x3_fwd_keep / fte_conv3x3_wgrad_kept) -- one tile transform instead of two.
        Residual blocks whose two convs both keep a V pack (lean[l], l = the block's second conv): the training forward does not
        write the first conv's y = prelu(z).  Its readers are the second conv's tile transform, which takes z and alpha instead
        (fte_conv3x3_fwd_keep_act), and that conv's filter gradient, which reads the kept pack; the data gradient reads z.  Those
        y buffers (1.3 GB of writes per step at 512 images) are allocated only when another walk asks for them (_y_buf).
        FTE_WINO_LEAN=0: the walk that writes every y (A/B hook; the library reads the same variable for its epilogues).
        -> vpack, lean, and form[l]: the forward launch of layer l in the fp32 training walk."""
        keep, self.lean = wino_plan(self.convs, n, self._algo, self.options, s16)
        self.vpack = [torch.empty(_lib.query('fte_wino_pack_bytes', n, c.hin, c.win, c.cin) // 4, dtype=torch.float32, device=self.device)
                      if k else None for c, k in zip(self.convs, keep)]
        lean = [f and self.options.wino_lean for f in self.lean] + [False]
        self.form = [LEAN_SECOND if lean[l] else LEAN_FIRST if lean[l + 1] else KEEP if keep[l] else PLAIN for l in range(len(keep))]
        for l, f in enumerate(self.lean):
            if f:
                self.y[l - 1] = None

    def _alloc_workspace(self, n):
        q = _lib.query
        need = 4096
        for c in self.convs[1:]:
            need = max(need, q('fte_conv3x3_fwd_ws_bytes', n, c.hin, c.win, c.cin, c.cout, c.stride),
                       q('fte_conv3x3_wgrad_ws_bytes', n, c.hin, c.win, c.cin, c.cout, c.stride),
                       q('fte_conv3x3_dgrad_ws_bytes', n, c.hin, c.win, c.cin, c.cout, c.stride))
        c0 = self.convs[0]
        need = max(need, q('fte_conv3x3_first_wgrad_ws_bytes', n, c0.hin, c0.win, c0.cin, c0.cout, c0.stride),
                   q('fte_gemm_ws_bytes', n, EMBED, self.fin), q('fte_gemm_ws_bytes', self._head_rows(n), self._head_width(), EMBED))
        self.ws = torch.empty((need + 3) // 4 + 1024, dtype=torch.float32, device=self.device)
        self.ws_bytes = self.ws.numel() * 4
        self._alloc_side()

    def _alloc_side(self):
        # filter gradients run on a second stream beside the data gradient of the same layer (_body_walk); their split-K slabs
        # need a workspace of their own
        self.side = side_stream(self.device) if self.options.side_stream != 'off' else None
        self.ws_side = torch.empty_like(self.ws) if self.side is not None else self.ws

    def _y_buf(self, l):
        """y of layer l; the first conv of a lean block (_alloc_acts) gets its buffer on the first walk that writes it"""
        if self.y[l] is None and not self._storage16():
            c = self.convs[l]
            self.y[l] = torch.empty(self._act_n, c.hout, c.wout, c.cout, dtype=torch.float32, device=self.device)
        return self.y[l]

    def _head_width(self):
        """columns of the head's [n, .] buffers (s_raw, G, logits_buf)"""
        return self.sub_centers * self.cpad

    def _alloc_head(self, n):
        """further head buffers of a subclass, sized with the activations"""

    def _use_copies(self):
        return self.bf16_copies and _lib.get_mfma_dtype() == 'bf16'

    def _alloc_copies(self):
        """bf16 copies of what the conv MFMAs read: y16[l] (written by layer l's forward epilogue), dz16 per stage
        (written by the dgrad epilogue), the weight packs w16 (HWIO, dgrad) and w16t ([tap][cout][cin], forward)."""
        if self.y16 is not None and self.y16[0].shape[0] == self._act_n:
            return
        i16 = dict(dtype=torch.int16, device=self.device)
        self.y16 = [torch.empty(self._act_n, c.hout, c.wout, c.cout, **i16) for c in self.convs]
        for ring in self.bwd:
            if ring.dz16 is None:
                ring.dz16 = [torch.empty(d.shape, **i16) for d in ring.dz]
        if self.packs is None:
            from ._packs import FilterPacks
            self.packs = FilterPacks([(c.name, self.variables[c.name + '/weights'].offset, 3, c.cin, c.cout) for c in self.convs[1:]], self.device)
            self.w16, self.w16t = self.packs.w16, self.packs.w16t

    def _pack_weights(self, st):
        self.packs.refresh(self.params, st)          # all 19 filters, one launch per layout

    # ------------------------------------------------------------------ forward
    def prelu(self, x, name='prelu'):
        raise RuntimeError('PReLU is fused into the conv epilogue (fte_conv3x3_fwd); it is not a separate op here.')

    def _check_images(self, images):
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32):
            raise TypeError('images must be a float32 CUDA tensor in NHWC (data.py:275-279 layout)')
        if not images.is_contiguous():
            images = images.contiguous()
        return images

    def _fwd_split(self, n, copies):
        """Forward walk as two part shards on two streams: the size of the first part, or 0 (one chain).  fp32 Winograd plan only (the
        direct kernels fill the chip by themselves and have no HBM-bound companion); sphere_plan.split_point has the rule."""
        if copies or self.side is None or self.one_stream:      # (one_stream: bench.py's launch-record steps)
            return 0
        key = (n, self._act_key)
        if self._split_key != key:
            self._split_key, self._split = key, split_point(self.convs, [v is not None for v in self.vpack], n, self._algo, self.options)
        return self._split

    def _fwd_halves(self, n, copies):
        return self._fwd_split(n, copies) > 0

    def _part_pack(self, l, lo, hi):
        """the V pack of layer l for images [lo, hi): a part shard's is its part of the shard's (whole row blocks: split_point)"""
        vp, n = self.vpack[l], self._act_n
        if hi - lo != n:
            per = self.convs[l].tiles * self.convs[l].cin * 16      # floats per image
            vp = vp[lo * per:hi * per] if hi < n else vp[lo * per:]      # (the last part keeps the shard's padding rows)
        return vp

    def _layer_views(self, l, lo, hi):
        """(conv spec, filter, bias, alpha, fp32 z to keep) of layer l; bf16 storage keeps fp32 z / y for the last layer only"""
        return (self.convs[l],) + self._pv[l] + (self.z[l][lo:hi] if self._mode.keep and self.z[l] is not None else None,)

    # layer l over images [lo, hi) on stream st (every forward kernel is per image: no statistics, nets/sphere.py:38-45): the stem,
    # then one launch body per mode
    def _fwd_stem(self, l, lo, hi, ws, st):
        c, wv, bv, av, zz = self._layer_views(0, lo, hi)
        x, m, call = self._images[lo:hi], self._mode, _lib.call
        if m.s16:
            call('fte_conv3x3_first_fwd_s16', x, wv, bv, av, self.z16[0][lo:hi] if m.keep else None, self.y16[0][lo:hi],
                 hi - lo, c.hin, c.win, c.cin, c.cout, c.stride, st)
            return
        call('fte_conv3x3_first_fwd', x, wv, bv, av, zz, self.y[0][lo:hi], hi - lo, c.hin, c.win, c.cin, c.cout, c.stride, st)
        if m.copies:
            call('fte_to_bf16', self.y[0][lo:hi], self.y16[0][lo:hi], self.y[0][lo:hi].numel(), st)

    def _fwd_s16(self, l, lo, hi, ws, st):
        """bf16 storage: every layer writes bf16 z / y only (+ the unrounded fp32 pair for the last layer: the dense layer reads it)"""
        c, _, bv, av, zz = self._layer_views(l, lo, hi)
        _lib.call('fte_conv2d_fwd_s16', self.y16[l - 1][lo:hi], self.w16t[c.name], bv, av, self.y16[l - 2][lo:hi] if c.second == 1 else None,
                  self.z16[l][lo:hi] if self._mode.keep else None, self.y16[l][lo:hi], zz, self.y[l][lo:hi] if self.y[l] is not None else None,
                  hi - lo, c.hin, c.win, c.cin, c.cout, 3, c.stride, ws, self.ws_bytes, st)

    def _fwd_copies(self, l, lo, hi, ws, st):
        """bf16 operands read as copies: the epilogue writes fp32 y and its bf16 copy"""
        c, _, bv, av, zz = self._layer_views(l, lo, hi)
        _lib.call('fte_conv2d_fwd16', self.y16[l - 1][lo:hi], self.w16t[c.name], bv, av, self.y[l - 2][lo:hi] if c.second == 1 else None, zz,
                  self.y[l][lo:hi], self.y16[l][lo:hi], hi - lo, c.hin, c.win, c.cin, c.cout, 3, c.stride, ws, self.ws_bytes, st)

    def _fwd_f32(self, l, lo, hi, ws, st):
        """fp32 storage, operands as the library's mode has them: the layer's Winograd form of _wino_tables while the packs are kept"""
        c, wv, bv, av, zz = self._layer_views(l, lo, hi)
        form, call = self.form[l] if self._mode.vpack else PLAIN, _lib.call
        shape = (hi - lo, c.hin, c.win, c.cin, c.cout, c.stride)
        if form == LEAN_SECOND:      # the input is prelu(z) of the block's first conv, formed in the tile transform
            call('fte_conv3x3_fwd_keep_act', self.z[l - 1][lo:hi], self._pv[l - 1].a, wv, bv, av, self.y[l - 2][lo:hi], zz,
                 self.y[l][lo:hi], *shape, self._part_pack(l, lo, hi), ws, self.ws_bytes, st)
        elif form == LEAN_FIRST:     # z only
            call('fte_conv3x3_fwd_keep_act', self.y[l - 1][lo:hi], None, wv, bv, av, None, zz, None, *shape, self._part_pack(l, lo, hi), ws, self.ws_bytes, st)
        else:
            res = self.y[l - 2][lo:hi] if c.second == 1 else None
            if form == KEEP:
                call('fte_conv3x3_fwd_keep', self.y[l - 1][lo:hi], wv, bv, av, res, zz, self.y[l][lo:hi], *shape, self._part_pack(l, lo, hi), ws, self.ws_bytes, st)
            else:
                call('fte_conv3x3_fwd', self.y[l - 1][lo:hi], wv, bv, av, res, zz, self.y[l][lo:hi], *shape, ws, self.ws_bytes, st)

    def backbone(self, inputs, is_training=False, reuse=None):
        """nets/sphere.py:47-76: [N,H,W,C] NHWC -> embedding [N,512] (a view of an internal buffer)."""
        x = self._check_images(inputs)
        n, h, w, ch = x.shape
        if not self.built:
            raise RuntimeError('call build() or forward(..., num_classes=) with is_training=True first')
        assert (h, w, ch) == self.in_hwc, ((h, w, ch), self.in_hwc)
        self._alloc_acts(n)
        st = _stream()
        self._images = x
        s16 = self._storage16()
        copies = self._use_copies() or s16
        vpack = is_training and not copies
        m = self._mode = Mode(is_training, s16, copies, vpack, vpack and self.options.wino_lean)
        nl = len(self.convs)
        if not m.lean:                                   # (before any stream forks: the part shards write them from two streams)
            for l in range(nl):
                self._y_buf(l)
        if copies:
            self._alloc_copies()
            self._pack_weights(st)
        launch = [self._fwd_stem] + [self._fwd_s16 if s16 else self._fwd_copies if copies else self._fwd_f32] * (nl - 1)
        split = self._fwd_split(n, copies)
        if split:
            # Two part shards (halves), one per stream: layer l of one part runs beside the tile transform of the other (an HBM-bound
            # kernel of 68 registers under an MFMA-bound resident one), and the CUs a launch's last, partly filled round leaves idle go
            # to the other part's launch.  No forward kernel of this net looks across images: each part comes out bit for bit as the
            # net computes it for those images as a shard of their own (against ONE launch over the whole shard the direct kernels of
            # the stride-2 layers may split their K sums differently: ~1e-7 relative; tests/test_gpu_stress.py).
            main, side = torch.cuda.current_stream(), self.side
            side.wait_stream(main)
            for l in range(nl):
                launch[l](l, 0, split, self.ws, st)
                launch[l](l, split, n, self.ws_side, side.cuda_stream)
            main.wait_stream(side)
        else:
            for l in range(nl):
                launch[l](l, 0, n, self.ws, st)
        _lib.call('fte_gemm_nn', self.y[-1], self.view(self.fc_w), self.view(self.name + '/fully_connected/biases'), self.emb,
                  n, EMBED, self.fin, self.ws, self.ws_bytes, st)
        return self.emb

    def _head_cols(self):
        """(W, dW, live columns, leading dimension) of the classifier columns the head runs on: here all of them, in the arenas"""
        return self.view(self.cls_w), self.view(self.cls_w, self.grads), self.num_classes, self.cpad

    def _classifier_raw(self, n):
        W, _, _, ld = self._head_cols()
        _lib.call('fte_gemm_nn', self.emb, W, None, self.s_raw, n, self.sub_centers * ld, EMBED, self.ws, self.ws_bytes, _stream())

    def _ensure_built(self, images, num_classes):
        if not self.built:
            n, h, w, ch = images.shape
            self.build(h, w, ch, num_classes, images.device)
        else:
            assert num_classes == self.num_classes, 'num_classes changed after the variables were created'

    def forward(self, images, num_classes=None, is_training=True):
        """nets/sphere.py:78-101."""
        if is_training:
            assert num_classes is not None, 'num_classes must be given when is_training=True'
            self._ensure_built(images, num_classes)
            self.backbone(images, is_training=True)
            self._classifier_raw(images.shape[0])
            return {'logits': self.s_raw[:, :self.num_classes]}
        return self._eval_features(images)

    def _eval_features(self, images):
        # nets/sphere.py:97-101: mean of the embeddings of x and of its horizontal flip (axis 2 of NHWC)
        # (flip and mean run in libfte.so like everything else of the path: fte_flip_width, fte_axpby)
        images = self._check_images(images)
        n, h, w, ch = images.shape
        st = _stream()
        out = torch.empty(n, EMBED, dtype=torch.float32, device=images.device)
        f1 = self.backbone(images, is_training=False)
        _lib.call('fte_axpby', 0.5, f1, 0.0, f1, out, n * EMBED, st)
        flipped = torch.empty_like(images)
        _lib.call('fte_flip_width', images, flipped, n, h, w, ch, st)
        f2 = self.backbone(flipped, is_training=False)
        _lib.call('fte_axpby', 1.0, out, 0.5, f2, out, n * EMBED, st)
        return out

    # ------------------------------------------------------------------ loss
    def _grad_scale(self, n):
        # mean over the shard (tf.losses.sparse_softmax_cross_entropy) times the 1/num_gpus of
        # data_parallel.py:37 -- applied at the head so that it propagates through backward for free.
        return self.tower_scale / n

    def _finish_losses(self, n):
        st = _stream()
        # slots: [ce * tower_scale, reg * tower_scale]  (sum over towers == data_parallel.py:248 mean)
        _lib.call('fte_sum', self.loss_rows, n, self.tower_scale / n, self.loss_slots[0:1], self.ws, self.ws_bytes, st)
        nreg = self.arena_size - self.small_end
        _lib.call('fte_sumsq', self.params[self.small_end:], nreg, 0.5 * self.weight_decay * self.tower_scale,
                  self.loss_slots[1:2], self.ws, self.ws_bytes, st)

    def loss_function(self, scope, labels, **logits):
        """nets/sphere.py:103-118 + Network._regularize (nets/net_base.py:103-116).
        Returns ([cross_entropy, reg_loss], names, others): the losses are 0-d device tensors
        (views of the loss slots that ride on the gradient arena); read them after the step."""
        n = labels.shape[0]
        labels = heads.check_labels(labels)
        self._labels = labels
        _lib.call('fte_softmax_ce_fwd_bwd', self.s_raw, labels, self.loss_rows, self.G, n, self.num_classes, self.cpad,
                  self._grad_scale(n), _stream())
        self._finish_losses(n)
        return [self.loss_slots[0], self.loss_slots[1]], ['cross_entropy', 'reg_loss'], OrderedDict()

    # ------------------------------------------------------------------ backward (replaces tf.gradients)
    def _head_backward(self, n, st):
        """the classifier's two products on the columns of _head_cols; the margin heads add the norm corrections (heads.py)"""
        W, dW, _, ld = self._head_cols()
        ld *= self.sub_centers                            # the products run over every plane
        norm = self.head != 'softmax'
        heads.classifier_dw(self, self.emb, W, dW, n, EMBED, ld, self.ws, self.ws_bytes, st, norm)
        self._scatter_dw(st)
        heads.classifier_dx(self, self.emb, W, self.demb, n, EMBED, ld, self.ws, self.ws_bytes, st, norm)

    def _scatter_dw(self, st):
        """what a head on a subset of the columns does with its dW before the input side runs; nothing for all columns"""

    def backward_head(self):
        """Classifier + FC gradients: the first (and largest) all-reduce bucket."""
        n = self._act_n
        st = _stream()
        call = _lib.call
        g = self.grads
        self._head_backward(n, st)
        call('fte_reduce_rows', self.demb, self.view(self.name + '/fully_connected/biases', g), None, 1, n, EMBED, 1, 1.0, st)
        call('fte_gemm_tn', self.y[-1], self.demb, self.view(self.fc_w, g), n, EMBED, self.fin, self.ws, self.ws_bytes, st)

    def backward(self):
        for stage in self.backward_stages():
            stage()

    def backward_stages(self):
        """One callable per all-reduce bucket of grad_buckets(), in the order backward completes them: the head, then the
        conv stack stage by stage from the last one (its filter gradients are final as soon as the walk leaves the
        stage -- 23.6 MB for stage 4, 21 MB for stage 3 -- so they cross xGMI under the remaining backward; only the
        stage-1 bucket with the biases / alphas is reduced after the last kernel)."""
        it = self._body_walk()
        return [self.backward_head] + [lambda it=it: next(it) for _ in range(len(self._stage_first))]

    def _side_stream(self, n):
        """The stream of the filter gradients, or None for the one-stream walk.  Measured on MI355X (fp32, images/s, one stream ->
        two): 64 per GPU 7.95 k -> 8.30 k, 128: 9.08 k -> 9.44 k, 256: 9.79 k -> 9.96 k, 512: 10.44 k -> 10.30 k -- at 512 every
        kernel is many rounds of blocks, nothing is left to cover and two MFMA-bound kernels sharing the chip cost 1.3 %; in the
        bf16 mode (launches 3x shorter) 512 gains too: 16.63 -> 16.13 ms.  FTE_SIDE_STREAM=0 / 1 forces one / two streams."""
        if self.side is None or self.one_stream:         # one_stream: bench.py's launch-record steps (a launch's duration is its own)
            return None
        if self.options.side_stream == 'forced':
            return self.side
        # ... and with the Winograd layers (round 6) at every size: the data gradient's tile transform (HBM-bound, 68 registers) shares the
        # CUs with the resident filter-gradient kernel of the other stream (MFMA-bound): 34.5 -> 33.4 ms per step at 512 images
        return self.side if (n <= 256 or _lib.get_mfma_dtype() == 'bf16' or _lib.query('fte_get_conv_algo') != 0) else None

    def backward_body(self):
        for _ in self._body_walk():
            pass

    def _dense_backward(self, ring, s16, copies, st):
        """the dense layer's data gradient with the last conv's PReLU backward in its epilogue -> (dz, skip gradient, bf16 dz) of the last
        layer in the mode's precision; bf16 storage: written in fp32 (ring.f32) and rounded, the skip gradient too"""
        c, call = self.convs[-1], _lib.call
        dz, raw = ring.reset()
        dz32, raw32 = ring.f32 if s16 else (dz, raw)
        call('fte_gemm_nt', self.demb, self.view(self.fc_w), self.z[-1], self._pv[-1].a, c.cout, raw32, dz32,
             self._gv[-1].a, self._act_n, EMBED, self.fin, self.ws, self.ws_bytes, st)
        if copies:
            call('fte_to_bf16', dz32, ring.dz16[0], dz32.numel(), st)
        if s16:
            call('fte_to_bf16', raw32, raw, raw32.numel(), st)
        return dz, raw, ring.dz16[0] if copies else None

    # filter gradient of layer l from its dz (dz16: the bf16 one where the mode has it), one launch body per mode ...
    def _wgrad_stem(self, dz, s16, st):
        c = self.convs[0]
        _lib.call('fte_conv3x3_first_wgrad_s16' if s16 else 'fte_conv3x3_first_wgrad', self._images, dz, self._gv[0].w,
                  self._act_n, c.hin, c.win, c.cin, c.cout, c.stride, self.ws, self.ws_bytes, st)

    def _wgrad16(self, l, dz, dz16, ws, st):
        c = self.convs[l]
        _lib.call('fte_conv2d_wgrad16', self.y16[l - 1], dz16, self._gv[l].w, self._act_n, c.hin, c.win, c.cin, c.cout,
                  3, c.stride, ws, self.ws_bytes, st)

    def _wgrad_f32(self, l, dz, dz16, ws, st):
        c, m = self.convs[l], self._mode
        gw, shape = self._gv[l].w, (self._act_n, c.hin, c.win, c.cin, c.cout, c.stride)
        if m.vpack and self.vpack[l] is not None:
            # (x is never read beside a kept pack -- fte.h -- and in a lean block y[l - 1] was not written)
            _lib.call('fte_conv3x3_wgrad_kept', None if m.lean and self.lean[l] else self.y[l - 1], dz, gw, *shape, self.vpack[l], ws, self.ws_bytes, st)
        else:
            _lib.call('fte_conv3x3_wgrad', self.y[l - 1], dz, gw, *shape, ws, self.ws_bytes, st)

    # ... and its data gradient: dz (+ addin) -> dz_prev (+ its bf16 copy), raw: the skip gradient it leaves for the block's shortcut
    def _dgrad_tail(self, l):
        """the arguments every data gradient ends on: dalpha and dbias of the layer below, the shard and the layer's shape"""
        c, g = self.convs[l], self._gv[l - 1]
        return g.a, g.b, self._act_n, c.hin, c.win, c.cin, c.cout

    def _dgrad_s16(self, l, dz, dz16, addin, raw, dz_prev, dz16_prev, st):
        c = self.convs[l]
        _lib.call('fte_conv2d_dgrad_s16', dz, self.w16[c.name], addin, self.z16[l - 1], self._pv[l - 1].a, raw, dz_prev,
                  *self._dgrad_tail(l), 3, c.stride, self.ws, self.ws_bytes, st)

    def _dgrad_copies(self, l, dz, dz16, addin, raw, dz_prev, dz16_prev, st):
        c = self.convs[l]
        _lib.call('fte_conv2d_dgrad16', dz16, self.w16[c.name], addin, self.z[l - 1], self._pv[l - 1].a, raw, dz_prev, dz16_prev,
                  *self._dgrad_tail(l), 3, c.stride, self.ws, self.ws_bytes, st)

    def _dgrad_f32(self, l, dz, dz16, addin, raw, dz_prev, dz16_prev, st):
        c = self.convs[l]
        _lib.call('fte_conv3x3_dgrad', dz, self._pv[l].w, addin, self.z[l - 1], self._pv[l - 1].a, raw, dz_prev,
                  *self._dgrad_tail(l), c.stride, self.ws, self.ws_bytes, st)

    def _body_walk(self):
        """Generator over the conv stack's backward pass; yields each time every filter gradient of one stage is final.
        Second stream: wgrad(l) and dgrad(l) both consume dz(l) and are independent of each other (and of every other layer's
        wgrad), so the filter gradients are queued on `side` and share the chip with the dgrad chain -- at small per-GPU shards a
        launch is one round of blocks whose prologue, epilogue and stragglers (~25 us of 130) are covered by the other stream's
        MFMAs.  dz rotates through the stage's three buffers (StageRing): before dgrad(l) overwrites one, the main stream waits for
        the wgrad that read it (two layers earlier).
        Same kernels, same operands, same order of every reduction: bit-identical to the one-stream walk."""
        m, L, st = self._mode, self.convs, _stream()
        s16, copies = m.keep and m.s16, m.keep and m.copies
        wgrad = self._wgrad16 if copies else self._wgrad_f32
        dgrad = self._dgrad_s16 if s16 else self._dgrad_copies if copies else self._dgrad_f32
        dz, d_out, dz16 = self._dense_backward(self.bwd[L[-1].stage], s16, copies, st)
        main, side = torch.cuda.current_stream(), self._side_stream(self._act_n)
        wst, wws = (side.cuda_stream, self.ws_side) if side is not None else (st, self.ws)
        readers = {}                                    # dz buffer -> event: the filter gradient that reads it has finished
        last_w = None
        for l in range(len(L) - 1, 0, -1):
            c, p = L[l], L[l - 1]
            if self._trace_dz is not None:
                self._trace_dz[c.name] = dz.clone()
            if side is not None:
                side.wait_event(main.record_event())    # dz(l) is complete
            wgrad(l, dz, dz16, wws, wst)
            if side is not None:
                last_w = readers[dz.data_ptr()] = side.record_event()
            ring, boundary = self.bwd[p.stage], p.stage != c.stage
            dz_prev, raw = ring.reset() if boundary else ring.advance()
            raw = raw if p.second == 1 else None
            ev = readers.pop(dz_prev.data_ptr(), None)
            if ev is not None:
                main.wait_event(ev)                     # an earlier layer's wgrad still reads the buffer dgrad(l) is about to overwrite
            dz16_prev = ring.copy16() if copies else None
            dgrad(l, dz, dz16, d_out if c.second == 0 else None, raw, dz_prev, dz16_prev, st)
            if raw is not None:
                d_out = raw
                ring.take_raw()
            dz, dz16 = dz_prev, dz16_prev
            if boundary:
                if last_w is not None:
                    main.wait_event(last_w)             # the stage's filter gradients are final for whoever follows on this stream
                    last_w = None
                    readers.clear()
                yield                                   # stage c.stage is done: its filter gradients are final
        if self._trace_dz is not None:
            self._trace_dz[L[0].name] = dz.clone()
        if last_w is not None:
            main.wait_event(last_w)
        self._wgrad_stem(dz, s16, st)
        yield

    # ------------------------------------------------------------------ bookkeeping the wrappers use
    def param_list(self, is_training, trainable, scope=None):
        """nets/sphere.py:120-126: [backbone vars, classifier vars] (lists of Variable)."""
        bb = [v for k, v in self.variables.items() if k.startswith(self.name + '/')]
        if is_training:
            return [bb, [self.variables[self.cls_w]]]
        return [bb]

    def pretrained_param(self, scope=None):
        """nets/sphere.py:128-134: backbone variables only."""
        return [v for grp in self.param_list(is_training=False, trainable=False, scope=scope) for v in grp
                if self.name in v.name]

    def arena_groups(self):
        """(start, end, decayed, param_group_index) ranges of the flat arena, in arena order."""
        return [(0, self.small_end, False, 0), (self.small_end, self.cls_start, True, 0),
                (self.cls_start, self.arena_size, True, 1)]

    def grad_buckets(self):
        """All-reduce buckets in the order backward completes them: head (classifier + FC, produced first, with the 4 loss
        slots that follow the arena riding along), then the conv filters stage by stage from the last; the first stage's
        bucket also carries the biases and alphas at the front of the arena (final only after the last dgrad)."""
        firsts = self._stage_first                       # arena offset of each stage's first conv filter, ascending
        ends = firsts[1:] + [self.fc_start]
        buckets = [(self.fc_start, self.arena_size + 4)]
        for i in range(len(firsts) - 1, 0, -1):
            buckets.append((firsts[i], ends[i]))
        buckets.append((0, ends[0]))
        return buckets


class SphereNetMargin(SphereNet):
    """SphereNet-20 + A-softmax (SphereFace, m = 4): the margin net DataParallel_margin drives
    (data_parallel.py:220: forward(images, labels, num_classes=..., is_training=True)).  The head's
    code is absent from the reference snapshot; spec = SURVEY.md Appendix A.9."""
    head = 'asoftmax'
    needs_labels = True

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0,
                 lambda_base=1000.0, gamma=0.12, power=1.0, lambda_min=5.0):
        super(SphereNetMargin, self).__init__(weight_decay, data_format, name, seed)
        self.lambda_base, self.gamma, self.power, self.lambda_min = lambda_base, gamma, power, lambda_min

    def current_lambda(self):
        return max(self.lambda_min, self.lambda_base * (1.0 + self.gamma * self.global_step) ** (-self.power))

    def forward(self, images, labels=None, num_classes=None, is_training=True):
        """backbone, then the head on the columns of _head_cols (heads.margin_forward); a sampled-class head picks them first"""
        if not is_training:
            return self._eval_features(images)
        assert num_classes is not None, 'num_classes must be given when is_training=True'
        assert labels is not None, 'margin nets take labels in forward (data_parallel.py:220)'
        self._ensure_built(images, num_classes)
        n = images.shape[0]
        self._check_sample(n)
        labels = heads.check_labels(labels)
        self._labels = labels
        st = _stream()
        self.backbone(images, is_training=True)
        labels, extra = self._sample_classes(labels, n, st)
        self._classifier_raw(n)
        W, _, c, ld = self._head_cols()
        heads.margin_forward(self, self.emb, W, self.s_raw, labels, self.logits_buf, self._head_spec(), n, EMBED, c, ld,
                             self._grad_scale(n), st)
        return dict({'logits': self.logits_buf[:, :c]}, **extra)

    def _check_sample(self, n):
        """a sampled-class head refuses a batch its sample cannot hold"""

    def _sample_classes(self, labels, n, st):
        """-> (the labels the head sees, further entries of forward's result); a sampled-class head draws its columns here"""
        return labels, {}

    def _head_spec(self):
        """the head description of heads.margin_forward"""
        self.lam = self.current_lambda()
        return ('asoftmax', self.lam)

    def _others(self):
        others = OrderedDict()
        others['lambda'] = self.lam
        return others

    def loss_function(self, scope, labels, **logits):
        n = labels.shape[0]
        self._finish_losses(n)
        return [self.loss_slots[0], self.loss_slots[1]], ['cross_entropy', 'reg_loss'], self._others()


class SphereNetAdditiveMargin(SphereNetMargin):
    """SphereNet-20 + an additive-margin softmax head on the normalised embedding and classifier columns: ArcFace
    (head='arcface', cos(theta + m)) or CosFace (head='cosface', cos(theta) - m3), scale S; fte.h fte_margin_softmax_fwd_bwd
    states the contract.  `scale` / `margin` / `margin_cos` = S / m / m3, None = the head's preset (nets/net_base.py
    MARGIN_PRESETS).  A margin net like SphereNetMargin (labels enter forward, DataParallel_margin drives it) with the same
    norm-correction backward (rowcoef (.) x, colcoef (.) W): the gradient is exact through both normalisations, the margin is
    not applied under no_grad.  The variables and their names are SphereNet's."""

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0, head='arcface',
                 scale=None, margin=None, margin_cos=None, sample_rate=None, sample_seed=0, sub_centers=1):
        super(SphereNetAdditiveMargin, self).__init__(weight_decay, data_format, name, seed)
        self.sub_centers = heads.check_sub_centers(sub_centers, head, sample_rate, name)
        self.margin_scale, self.margin, self.margin_cos = margin_params(head, scale, margin, margin_cos)
        self.head = head
        # the sampled-class head under data parallelism and its compact classifier update; the dense head ignores both
        self.sample_comm = None           # set by DataParallel(sync_sample=True): the ranks all-gather their labels, one sample for all
        self.compact_head_update = False  # True: no dense classifier gradient; the wrapper ends the step with apply_compact_update
        # the classifier split by class over the ranks (fte.h "Sharded margin head"): set by
        # DataParallel(shard_classes=True) BEFORE build(); this rank then holds only its own [D, ld_r] columns
        self.shard_comm = None
        self.set_sample_rate(sample_rate, sample_seed)

    def _head_spec(self):
        return heads.describe(self)

    # ---- the sharded classifier --------------------------------------------------------------------------------------------------
    def build(self, height, width, channels, num_classes, device='cuda'):
        self.shard = None                                 # (lo, hi): the classes this rank owns
        if self.shard_comm is not None:
            heads.check_sharding(self.head, self.sample_rate, self.sample_comm is not None, self.sub_centers, self.name)
            R = self.shard_comm.world_size()
            self.shard = heads.shard_range(num_classes, R, self.shard_comm.rank())
            self.shard_cols = heads.shard_ld(num_classes, R)      # from Cs: the arena has the same size on every rank
        return super(SphereNetAdditiveMargin, self).build(height, width, channels, num_classes, device)

    def _sharded(self):
        if self.shard_comm is not None and getattr(self, 'shard', None) is None:
            raise ValueError('%s was already built with the dense classifier: shard_comm must be set before build()' % self.name)
        return self.shard_comm is not None

    def _head_width_stored(self):
        return self.shard_cols if self.shard is not None else super(SphereNetAdditiveMargin, self)._head_width_stored()

    def _stored_columns(self, wc):
        # the dense classifier is drawn from the seed on every rank and the rank keeps its own columns: a sharded net starts from the
        # dense net's values
        if self.shard is None:
            return wc
        lo, hi = self.shard
        own = torch.zeros(EMBED, self.shard_cols)
        own[:, :hi - lo] = wc[:, 0, lo:hi]
        return own

    def _head_rows(self, n):
        return n * self.shard_comm.world_size() if self.shard is not None else n

    def get_variable(self, name, arena=None):
        """The classifier (or its gradient / slot) of a sharded net comes back DENSE, [512, C], the shards side by side bit for bit: a
        COLLECTIVE (one all-gather) that every rank must enter."""
        if self.shard is None or name != self.cls_w:
            return super(SphereNetAdditiveMargin, self).get_variable(name, arena)
        R, ld = self.shard_comm.world_size(), self.shard_cols
        every = torch.empty(R, EMBED, ld, dtype=torch.float32, device=self.device)
        self.shard_comm.all_gather(every, self.view(name, arena).reshape(EMBED, ld))
        ranges = [heads.shard_range(self.num_classes, R, r) for r in range(R)]
        return torch.cat([every[r, :, :hi - lo] for r, (lo, hi) in enumerate(ranges)], dim=1)

    def set_variable(self, name, value, arena=None):
        """a dense [512, C] classifier value: the rank keeps its own columns (no collective)"""
        if self.shard is None or name != self.cls_w:
            return super(SphereNetAdditiveMargin, self).set_variable(name, value, arena)
        t = torch.as_tensor(value, dtype=torch.float32).to(self.device)
        assert tuple(t.shape) == self.variables[name].ref_shape, (name, tuple(t.shape), self.variables[name].ref_shape)
        lo, hi = self.shard
        buf = torch.zeros(EMBED, self.shard_cols, device=self.device)
        buf[:, :hi - lo] = t[:, lo:hi]
        self.view(name, arena).copy_(buf.reshape(-1))

    def _alloc_head(self, n):
        if self.shard is not None:
            heads.shard_buffers(self, n, EMBED, self.shard_comm.world_size(), self.device)
            return
        self._alloc_sampler(n)

    def forward(self, images, labels=None, num_classes=None, is_training=True):
        if not is_training or self.shard_comm is None:
            return super(SphereNetAdditiveMargin, self).forward(images, labels, num_classes, is_training)
        assert num_classes is not None, 'num_classes must be given when is_training=True'
        assert labels is not None, 'margin nets take labels in forward (data_parallel.py:220)'
        self._ensure_built(images, num_classes)
        self._sharded()
        n = images.shape[0]
        labels = heads.check_labels(labels)
        self._labels = labels
        st = _stream()
        self.backbone(images, is_training=True)
        W, _, c, ld = self._head_cols()
        N = self._head_rows(n)
        # grad_scale = 1 / N: what tower_scale / n summed over the ranks gives the dense head
        heads.sharded_margin_forward(self, self.emb, W, self.s_raw, labels, self.logits_buf, self._head_spec(), n, EMBED, self.shard[0], c, ld,
                                     self.num_classes, self.shard_comm, 1.0 / N, self.ws, self.ws_bytes, st)
        return {'logits': self.logits_buf[:, :c]}           # this rank's [N, c_r] block

    def _finish_losses(self, n):
        if self.shard is None:
            return super(SphereNetAdditiveMargin, self)._finish_losses(n)
        # the slots are summed over the ranks: cross_entropy is the mean over the GLOBAL batch, the same bits on every rank, times
        # tower_scale = 1 / R; reg_loss counts the backbone once (its share times tower_scale) and this rank's classifier columns whole
        st, N, call = _stream(), self._head_rows(n), _lib.call
        call('fte_sum', self.loss_rows, N, self.tower_scale / N, self.loss_slots[0:1], self.ws, self.ws_bytes, st)
        half = 0.5 * self.weight_decay
        call('fte_sumsq', self.params[self.small_end:self.cls_start], self.cls_start - self.small_end, half * self.tower_scale,
             self.loss_slots[1:2], self.ws, self.ws_bytes, st)
        call('fte_sumsq', self.params[self.cls_start:], self.arena_size - self.cls_start, half, self.loss_slots[2:3], self.ws, self.ws_bytes, st)
        call('fte_axpby', 1.0, self.loss_slots[1:2], 1.0, self.loss_slots[2:3], self.loss_slots[1:2], 1, st)

    def _head_backward(self, n, st):
        if self.shard is None:
            return super(SphereNetAdditiveMargin, self)._head_backward(n, st)
        W, dW, _, ld = self._head_cols()
        heads.sharded_classifier_dw(self, W, dW, n, EMBED, ld, self.ws, self.ws_bytes, st)       # final: never all-reduced
        heads.sharded_classifier_dx(self, W, self.demb, n, EMBED, ld, self.shard_comm, self.ws, self.ws_bytes, st)

    # ---- the sampled-class head (Partial FC; fte.h "Partial FC") -----------------------------------------------
    def set_sample_rate(self, rate, seed=0):
        """rate in (0, 1): every training step runs the head over S = ceil(rate * num_classes) classes, the batch's own plus the
        other classes with the smallest hashes under (seed, global_step); None or 1: the dense head.  The variables, the dense
        [D, cpad] classifier gradient (0.0 in the unsampled columns), the optimizer and the checkpoints stay as they are."""
        sample_size(1, rate)                              # validates the rate
        heads.check_sub_centers(self.sub_centers, self.head, rate, self.name)
        self.sample_rate = None if rate is None or float(rate) >= 1.0 else float(rate)
        self.sample_seed = int(seed)
        self._act_n = None                                # the head buffers change width

    @property
    def sample_size(self):
        """S, the classes per step (num_classes for the dense head)"""
        return sample_size(self.num_classes, self.sample_rate)

    def _head_width(self):
        if getattr(self, 'shard', None) is not None:
            return self.shard_cols
        return self.sub_centers * self.cpad if self.sample_rate is None else (self.sample_size + 63) // 64 * 64

    def _alloc_sampler(self, n):
        if self.sample_rate is None:
            return
        S, spad = self.sample_size, self._head_width()
        f32, i32 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.int32, device=self.device)
        self.class_index = torch.empty(spad, **i32)
        self.class_inverse = torch.empty(self.num_classes, **i32)
        self.sampled_labels = torch.empty(n, **i32)
        self.Ws = torch.empty(EMBED, spad, **f32)
        self.dWs = torch.empty(EMBED, spad, **f32)
        self.pfc_ws = torch.empty(_lib.query('fte_pfc_sample_ws_bytes', self.num_classes) // 4 + 16, **f32)

    def _check_sample(self, n):
        if self.sample_rate is None:
            return
        S = self.sample_size
        comm = self.sample_comm
        world = 1 if comm is None else comm.world_size()
        if S < world * n:
            if comm is None:
                raise ValueError('the sample of %d classes (sample_rate %g of %d) is smaller than the batch of %d rows'
                                 % (S, self.sample_rate, self.num_classes, n))
            raise ValueError('the sample of %d classes (sample_rate %g of %d) is smaller than the batch of %d rows (the global batch: '
                             '%d ranks of %d rows)' % (S, self.sample_rate, self.num_classes, world * n, world, n))

    def _sample_classes(self, labels, n, st):
        if self.sample_rate is None:
            return labels, {}
        S = self.sample_size
        heads.sample_classes(self, labels, self.view(self.cls_w), n, EMBED, self.num_classes, self.cpad, S,
                             self._head_width(), self.sample_seed, self.global_step, self.pfc_ws, self.pfc_ws.numel() * 4, st,
                             self.sample_comm)
        return self.sampled_labels, {'class_index': self.class_index[:S]}

    def _head_cols(self):
        """the sampled head is the dense head on its S gathered columns and their compact gradient"""
        if getattr(self, 'shard', None) is not None:        # the rank's own columns, in the arenas
            return self.view(self.cls_w), self.view(self.cls_w, self.grads), self.shard[1] - self.shard[0], self.shard_cols
        if self.sample_rate is None:
            return super(SphereNetAdditiveMargin, self)._head_cols()
        return self.Ws, self.dWs, self.sample_size, self._head_width()

    def _scatter_dw(self, st):
        # under compact_head_update the classifier range of `grads` is NOT written (it holds whatever an earlier step or mode left there);
        # the gradient is compact_grad(), and apply_compact_update takes it into the classifier
        if self.sample_rate is not None and not self.compact_head_update:
            _lib.call('fte_pfc_scatter_cols', self.dWs, self.class_inverse, self.view(self.cls_w, self.grads), EMBED,
                      self.num_classes, self.cpad, self.sample_size, self._head_width(), st)

    # ---- the compact classifier update (fte.h fte_pfc_momentum_update_cols / fte_pfc_adam_update_cols) -------------------------------
    def compact_active(self):
        """True when the step ends with apply_compact_update instead of a dense classifier gradient: the sampled head, switched on"""
        return self.sample_rate is not None and bool(self.compact_head_update)

    def compact_grad(self):
        """The [D, Spad] gradient of the sampled classifier columns, as backward_head leaves it (columns in class_index order).  Under
        data parallelism every rank holds the same columns (one shared sample), so its sum over the ranks is the dense gradient's sum:
        this buffer is what crosses the wire."""
        return self.dWs

    def arena_groups(self):
        groups = super(SphereNetAdditiveMargin, self).arena_groups()
        return groups[:-1] if self.compact_active() else groups      # the classifier is updated by apply_compact_update

    def grad_buckets(self):
        buckets = super(SphereNetAdditiveMargin, self).grad_buckets()
        if getattr(self, 'shard', None) is not None:
            # the classifier gradient is final on its rank: the head bucket is the FC range, the four loss slots travel on their own
            buckets[0] = (self.fc_start, self.cls_start)
        if self.compact_active():
            # the head bucket shrinks to the FC range: the classifier gradient travels as compact_grad(), the four loss slots behind the
            # arena in an all-reduce of their own (data_parallel.py)
            buckets[0] = (self.fc_start, self.cls_start)
        return buckets

    def apply_compact_update(self, opt, lr, step_1based, mult_lr_list):
        """The classifier's share of _DeviceOptimizer.apply -- group 1 of the dense arena_groups(), with the same lr, wd * gs, gs and t
        and the optimizer's own slots for the range -- taken straight from compact_grad(): the same bytes as the scatter followed by the
        dense update, without the dense gradient."""
        opt._ensure()
        a, b = self.cls_start, self.arena_size
        gs = float(mult_lr_list[1])
        wd = self.weight_decay
        S, spad = self.sample_size, self._head_width()
        shape = (EMBED, self.num_classes, self.cpad, S, spad)
        if opt.kind == 'Momentum':
            _lib.call('fte_pfc_momentum_update_cols', self.params[a:b], opt.slots[0][a:b], self.dWs, self.class_inverse, *shape,
                      float(lr), 0.9, wd * gs, gs, _stream())
        else:
            _lib.call('fte_pfc_adam_update_cols', self.params[a:b], opt.slots[0][a:b], opt.slots[1][a:b], self.dWs, self.class_inverse,
                      *shape, float(lr), 0.5, 0.999, 1e-8, wd * gs, gs, int(step_1based), _stream())

    def _others(self):
        return OrderedDict()


class SphereNetAdaFace(SphereNetMargin):
    """SphereNet-20 + the AdaFace head (Kim et al., CVPR 2022): the additive-margin softmax with the margin of each image set from
    the norm of its embedding against running statistics of the norms -- low-norm (unrecognisable) images get a positive angular
    margin and a small additive one, high-norm ones the reverse; fte.h fte_adaface_margins / fte_margin_softmax_rows_fwd_bwd state the contract.  `scale` /
    `margin` / `h` / `t_alpha` = S / m / h / t_alpha, None = the preset (nets/net_base.py ADAFACE_PRESET).  The call order and the
    norm-correction backward are SphereNetAdditiveMargin's; the norm enters the margins as a constant.  State: the two running
    scalars `classifier/adaface/batch_mean` / `batch_std` (net.state; saved and restored by saver.py, not in the arena, not
    all-reduced: per-tower state like the BN moving statistics); they move on every training forward unless `update_moving_stats`
    is False (the parallel wrappers' construction pass)."""
    head = 'adaface'

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0, scale=None, margin=None, h=None, t_alpha=None):
        super(SphereNetAdaFace, self).__init__(weight_decay, data_format, name, seed)
        self.margin_scale, self.margin, self.adaface_h, self.adaface_t_alpha = adaface_params(scale, margin, h, t_alpha)
        self.margin_cos = 0.0
        self.update_moving_stats = True

    def _make_state(self):
        self.adaface_stats, state = adaface_state(self.device)
        return state

    def _alloc_head(self, n):
        self.a_rows = torch.empty(n, dtype=torch.float32, device=self.device)
        self.b_rows = torch.empty(n, dtype=torch.float32, device=self.device)

    def _head_spec(self):
        return heads.describe(self)

    def _others(self):
        return OrderedDict()


class SphereNetCurricularFace(SphereNetMargin):
    """SphereNet-20 + the CurricularFace head (Huang et al., CVPR 2020): ArcFace's target logit, and every negative column whose
    cosine exceeds the margined target cosine (a hard negative) re-weighted by t + cos, t a running mean of the batch's target
    cosines -- the emphasis on hard negatives grows as training converges; fte.h fte_curricular_t / fte_curricular_softmax_fwd_bwd
    state the contract.  `scale` / `margin` / `alpha` = S / m / alpha, None = the preset (nets/net_base.py CURRICULAR_PRESET).  The
    call order and the norm-correction backward are SphereNetAdditiveMargin's; t and the mask enter the gradient as constants.
    State: the scalar `classifier/curricularface/t` (net.state; saved and restored by saver.py, not in the arena, not all-reduced:
    per-tower state like the BN moving statistics); it moves on every training forward, before the logits are formed, unless
    `update_moving_stats` is False (the parallel wrappers' construction pass)."""
    head = 'curricularface'

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0, scale=None, margin=None, alpha=None):
        super(SphereNetCurricularFace, self).__init__(weight_decay, data_format, name, seed)
        self.margin_scale, self.margin, self.curricular_alpha = curricular_params(scale, margin, alpha)
        self.margin_cos = 0.0
        self.update_moving_stats = True

    def _make_state(self):
        self.cf_state, state = curricular_state(self.device)
        return state

    def _alloc_head(self, n):
        self.cf_t = torch.empty(1, dtype=torch.float32, device=self.device)

    def _head_spec(self):
        return heads.describe(self)

    def _others(self):
        return OrderedDict()


class SphereNetMagFace(SphereNetMargin):
    """SphereNet-20 + the MagFace head (Meng et al., CVPR 2021): ArcFace's target logit with the margin of each image a linear
    function of the clamped norm of its embedding, mu = l_m + (u_m - l_m) (a - l_a) / (u_a - l_a), and the regulariser
    g(a) = a / u_a^2 + 1 / a, weight lambda_g, which rewards large norms; fte.h fte_magface_softmax_fwd_bwd states the contract.
    The margin is part of the gradient (the opposite of AdaFace): the norms are trained, and after training the norm of the raw
    embedding is a quality score of the image (verification.feature_quality).  `scale` = S and `l_a` .. `lambda_g`, None = the
    preset (nets/net_base.py MAGFACE_PRESET).  The call order and the norm-correction backward are SphereNetAdditiveMargin's; the
    head's whole norm gradient is in rowcoef.  No state: the variable names are SphereNet-ArcFace's.  Three losses: cross_entropy
    (the pure CE, comparable with ArcFace's), magnitude_loss = lambda_g * mean g, reg_loss."""
    head = 'magface'

    def __init__(self, weight_decay=0.0005, data_format='NCHW', name='SphereNet', seed=0, scale=None, l_a=None, u_a=None, l_m=None,
                 u_m=None, lambda_g=None):
        super(SphereNetMagFace, self).__init__(weight_decay, data_format, name, seed)
        vals = magface_params(scale, l_a, u_a, l_m, u_m, lambda_g)
        self.margin_scale, self.magface = vals[0], vals[1:]
        self.margin, self.margin_cos = 0.0, 0.0

    def _alloc_head(self, n):
        self.reg_rows = torch.empty(n, dtype=torch.float32, device=self.device)

    def _head_spec(self):
        return heads.describe(self)

    def _finish_losses(self, n):
        super(SphereNetMagFace, self)._finish_losses(n)
        # slot 2: lambda_g * mean g * tower_scale (the term G's rowcoef already carries the gradient of)
        _lib.call('fte_sum', self.reg_rows, n, self.magface[4] * self.tower_scale / n, self.loss_slots[2:3], self.ws, self.ws_bytes, _stream())

    def loss_function(self, scope, labels, **logits):
        n = labels.shape[0]
        self._finish_losses(n)
        return ([self.loss_slots[0], self.loss_slots[2], self.loss_slots[1]], ['cross_entropy', 'magnitude_loss', 'reg_loss'],
                OrderedDict())
