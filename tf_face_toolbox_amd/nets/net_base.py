"""Net factory + Network ABC: the host-side mirror of the reference's nets/net_base.py.

Same names, arguments and error behaviour as nets/net_base.py:22-63 (`net_select`) and
:65-101 (`Network`).  What was graph construction in TF1 is eager here: `forward` /
`loss_function` enqueue HIP kernels, and because there is no `tf.gradients`
(data_parallel.py:33) a Network also implements `backward()`, which fills the flat
gradient arena the parallel wrappers all-reduce.
"""
import abc

# (S, m, m3) of the additive-margin heads: ArcFace (Deng et al. 2019: s = 64, m = 0.5) and CosFace (Wang et al. 2018: s = 64,
# m = 0.35, here the cosine margin m3)
MARGIN_PRESETS = {'arcface': (64.0, 0.5, 0.0), 'cosface': (64.0, 0.0, 0.35)}


def margin_params(head, scale=None, margin=None, margin_cos=None):
    """(S, m, m3) of the additive-margin head `head`: the given values, the head's preset where an argument is None."""
    if head not in MARGIN_PRESETS:
        raise ValueError('%r is not an additive-margin head (%s)' % (head, ', '.join(sorted(MARGIN_PRESETS))))
    ps, pm, pm3 = MARGIN_PRESETS[head]
    S = float(ps if scale is None else scale)
    m = float(pm if margin is None else margin)
    m3 = float(pm3 if margin_cos is None else margin_cos)
    if not (S > 0.0 and 0.0 <= m < 3.141592653589793 and abs(m3) < 1.0):
        raise ValueError('margin head needs scale > 0, 0 <= margin < pi and |margin_cos| < 1 (got %r, %r, %r)' % (S, m, m3))
    return S, m, m3


# AdaFace (Kim et al. 2022: s = 64, m = 0.4, h = 0.333, t_alpha = 0.01): the margin of each image follows the norm of its embedding,
# measured against running statistics of the norms -- two non-trainable variables, initialised to mean 20 and std 100
ADAFACE_PRESET = (64.0, 0.4, 0.333, 0.01)
ADAFACE_STATS_INIT = (20.0, 100.0)
ADAFACE_STATE = ('classifier/adaface/batch_mean', 'classifier/adaface/batch_std')
# heads on the normalised embedding and classifier columns: xn / wn / rowcoef / colcoef buffers and the norm-correction backward
NORMALISED_HEADS = tuple(MARGIN_PRESETS) + ('adaface', 'curricularface', 'magface')
# CurricularFace (Huang et al. 2020: s = 64, m = 0.5, alpha = 0.01): ArcFace's target logit, and the negative columns above the
# margined target cosine re-weighted by t, a running mean of the batch's target cosines -- one non-trainable variable, initially 0
CURRICULAR_PRESET = (64.0, 0.5, 0.01)
CURRICULAR_STATE = ('classifier/curricularface/t',)
# MagFace (Meng et al. 2021, the MS1M-V2 values: s = 64, l_a = 10, u_a = 110, l_m = 0.45, u_m = 0.8, lambda_g = 35): the margin of each
# image grows linearly with the clamped norm of its embedding and a regulariser rewards large norms; the margin is part of the
# gradient, so the norms are trained.  No state variable: a MagFace net has the variable names of the ArcFace net of its backbone
MAGFACE_PRESET = (64.0, 10.0, 110.0, 0.45, 0.8, 35.0)


def adaface_params(scale=None, margin=None, h=None, t_alpha=None):
    """(S, m, h, t_alpha) of the AdaFace head: the given values, the preset where an argument is None."""
    vals = [float(p if v is None else v) for p, v in zip(ADAFACE_PRESET, (scale, margin, h, t_alpha))]
    S, m, h_, ta = vals
    if not (S > 0.0 and 0.0 <= m < 1.5707963267948966 and h_ > 0.0 and 0.0 <= ta <= 1.0):
        raise ValueError('AdaFace head needs scale > 0, 0 <= margin < pi/2, h > 0 and 0 <= t_alpha <= 1 (got %r, %r, %r, %r)' % tuple(vals))
    return S, m, h_, ta


def adaface_state(device):
    """-> (stats, state): the [mean, std] pair the kernel updates in place and its two one-element views under their variable names"""
    import torch
    from collections import OrderedDict
    stats = torch.tensor(ADAFACE_STATS_INIT, dtype=torch.float32, device=device)
    return stats, OrderedDict((name, stats[i:i + 1]) for i, name in enumerate(ADAFACE_STATE))


def curricular_params(scale=None, margin=None, alpha=None):
    """(S, m, alpha) of the CurricularFace head: the given values, the preset where an argument is None."""
    vals = [float(p if v is None else v) for p, v in zip(CURRICULAR_PRESET, (scale, margin, alpha))]
    S, m, a = vals
    if not (S > 0.0 and 0.0 <= m < 1.5707963267948966 and 0.0 <= a <= 1.0):
        raise ValueError('CurricularFace head needs scale > 0, 0 <= margin < pi/2 and 0 <= alpha <= 1 (got %r, %r, %r)' % tuple(vals))
    return S, m, a


def curricular_state(device):
    """-> (t, state): the one-element t the kernel updates in place (initially 0) and the same tensor under its variable name"""
    import torch
    from collections import OrderedDict
    t = torch.zeros(1, dtype=torch.float32, device=device)
    return t, OrderedDict(((CURRICULAR_STATE[0], t),))


def magface_params(scale=None, l_a=None, u_a=None, l_m=None, u_m=None, lambda_g=None):
    """(S, l_a, u_a, l_m, u_m, lambda_g) of the MagFace head: the given values, the preset where an argument is None.  The ranges are
    fte.h's fte_magface_softmax_fwd_bwd (a NaN fails every compare)."""
    vals = [float(p if v is None else v) for p, v in zip(MAGFACE_PRESET, (scale, l_a, u_a, l_m, u_m, lambda_g))]
    S, la, ua, lm, um, lg = vals
    if not (S > 0.0 and la > 0.0 and ua > la and lm >= 0.0 and um >= lm and um < 1.5707963267948966 and lg >= 0.0):
        raise ValueError('MagFace head needs scale > 0, 0 < l_a < u_a, 0 <= l_m <= u_m < pi/2 and lambda_g >= 0 '
                         '(got %r, %r, %r, %r, %r, %r)' % tuple(vals))
    return tuple(vals)


def magface_lambda_bound(scale, l_a, u_a, l_m, u_m):
    """S k_m u_a^2 l_a^2 / (u_a^2 - l_a^2): below it lambda_g does not give the loss a unique optimum in the norm (the paper's
    condition; 22.6 for the preset)"""
    k_m = (u_m - l_m) / (u_a - l_a)
    return scale * k_m * u_a * u_a * l_a * l_a / (u_a * u_a - l_a * l_a)


IRESNET_NAMES = tuple('IResNet-%d%s' % (d, h) for d in (18, 34, 50, 100) for h in ('', '-arcface', '-cosface', '-adaface', '-curricularface', '-magface'))
SE_IRESNET_NAMES = tuple('SE-' + n for n in IRESNET_NAMES)      # "IR-SE": an SE gate behind every block's last BN
SUB_CENTER_NETS = ('SphereNet-ArcFace', 'SphereNet-CosFace', 'ResNet-50-arcface', 'ResNet-50-cosface')


def sub_centers_check(name, sub_centers, sample_rate=None):
    """sub_centers of net_select / train.py --sub_centers -> int K; ValueError for what the K-centre head does not do (K outside 1..8;
    with K > 1: a net outside SUB_CENTER_NETS -- the A-softmax and AdaFace heads among them -- and the class sampler)."""
    from ..heads import check_sub_centers
    K = check_sub_centers(sub_centers)
    if K > 1 and name not in SUB_CENTER_NETS:
        raise ValueError('sub_centers = %d: only %s have a K-centre head, not %s' % (K, ' / '.join(SUB_CENTER_NETS), name))
    return check_sub_centers(K, 'arcface', sample_rate, name)


def net_select(name, data_format='NCHW', weight_decay=5e-4, sub_centers=1):
    """nets/net_base.py:22-63.  Names kept verbatim; `SphereNet-ASoftmax` is the margin net the
    reference's `DataParallel_margin` (data_parallel.py:220) expects but whose code is missing
    from the snapshot (README.md:14,19).  `sub_centers` = K centres per class (sub-center ArcFace, fte.h; SUB_CENTER_NETS only;
    1 = one column per class, the nets as they always were)."""
    sub_centers = sub_centers_check(name, sub_centers)
    if name == 'SphereNet':
        from .sphere import SphereNet
        network = SphereNet(data_format=data_format, weight_decay=weight_decay)
    elif name == 'SphereNet-ASoftmax':
        from .sphere import SphereNetMargin
        network = SphereNetMargin(data_format=data_format, weight_decay=weight_decay)
    elif name in ('SphereNet-ArcFace', 'SphereNet-CosFace'):      # additive-margin heads (fte.h fte_margin_softmax_fwd_bwd)
        from .sphere import SphereNetAdditiveMargin
        network = SphereNetAdditiveMargin(data_format=data_format, weight_decay=weight_decay, head=name.split('-')[1].lower(),
                                          sub_centers=sub_centers)
    elif name == 'SphereNet-AdaFace':                             # quality-adaptive margin head (fte.h fte_adaface_margins)
        from .sphere import SphereNetAdaFace
        network = SphereNetAdaFace(data_format=data_format, weight_decay=weight_decay)
    elif name == 'SphereNet-CurricularFace':                      # hard-negative re-weighting head (fte.h fte_curricular_softmax_fwd_bwd)
        from .sphere import SphereNetCurricularFace
        network = SphereNetCurricularFace(data_format=data_format, weight_decay=weight_decay)
    elif name == 'SphereNet-MagFace':                             # magnitude-aware margin head (fte.h fte_magface_softmax_fwd_bwd)
        from .sphere import SphereNetMagFace
        network = SphereNetMagFace(data_format=data_format, weight_decay=weight_decay)
    elif name == 'ResNet-50':
        from .resnet import ResNet
        network = ResNet(num_layers=50, data_format=data_format, weight_decay=weight_decay)
    elif name in ('ResNet-50-arcface', 'ResNet-50-cosface', 'ResNet-50-adaface', 'ResNet-50-curricularface', 'ResNet-50-magface'):
        from .resnet import ResNet
        network = ResNet(num_layers=50, data_format=data_format, weight_decay=weight_decay, head=name.split('-')[2])
        network.set_sub_centers(sub_centers)
    elif name in IRESNET_NAMES + SE_IRESNET_NAMES:      # the ArcFace papers' backbone (nets/iresnet.py): [SE-]IResNet-<depth>[-<margin head>]
        from .iresnet import IResNet
        se = name.startswith('SE-')
        parts = name[3 if se else 0:].split('-')
        network = IResNet(num_layers=int(parts[1]), data_format=data_format, weight_decay=weight_decay,
                          head=parts[2] if len(parts) > 2 else 'softmax', se=se)
    elif name == 'ResNet-26':                    # not a reference factory name; the class accepts 26 (nets/resnet.py:39-40)
        from .resnet import ResNet
        network = ResNet(num_layers=26, data_format=data_format, weight_decay=weight_decay)
    elif name in ('ResNeXt-26', 'ResNeXt-50'):   # nets/net_base.py:27-31 exposes -26; -50 is BASELINE config 3
        from .resnet import ResNeXt
        network = ResNeXt(num_layers=int(name.split('-')[1]), num_card=32, data_format=data_format, weight_decay=weight_decay)
    elif name in ('ResNeXt-50-center', 'ResNeXt-26-center'):      # config 3: + center loss on the pooled features (loss.py:29-45)
        from .resnet import ResNeXt
        network = ResNeXt(num_layers=int(name.split('-')[1]), num_card=32, data_format=data_format, weight_decay=weight_decay,
                          head='softmax+center', center_weight=0.008)
    elif name == 'SENet-50':
        from .resnet import SENet
        network = SENet(num_layers=50, data_format=data_format, weight_decay=weight_decay)
    elif name == 'SENet-50-triplet':             # config 4: batch-hard triplet (loss.py:47-78), no classifier
        from .resnet import SENet
        network = SENet(num_layers=50, data_format=data_format, weight_decay=weight_decay, head='triplet')
    elif name == 'ShuffleNet-v2-small':                                  # nets/net_base.py:37-42
        from .shufflenet_v2 import ShuffleNet_v2_small
        network = ShuffleNet_v2_small(alpha=2.0, se=False, residual=False, data_format=data_format, weight_decay=weight_decay)
    elif name == 'ShuffleNet-v2-middle':                                 # :43-47
        from .shufflenet_v2 import ShuffleNet_v2_middle
        network = ShuffleNet_v2_middle(se=False, residual=False, data_format=data_format, weight_decay=weight_decay)
    elif name == 'ShuffleNet-v2-large':                                  # :48-51
        from .shufflenet_v2 import ShuffleNet_v2_large
        network = ShuffleNet_v2_large(data_format=data_format, weight_decay=weight_decay)
    elif name in ('MobileNet-v2', 'Inception-v4', 'VGG16', 'AlexNet'):
        # nets/net_base.py:52-59 `pass` branches: the reference dies with UnboundLocalError here
        raise UnboundLocalError("local variable 'network' referenced before assignment")
    else:
        raise ValueError('Unsupport network architecture.')
    return network


class Network(abc.ABC):
    """nets/net_base.py:65-101."""

    needs_labels = False       # True for margin nets: forward(images, labels, num_classes=...)

    def __init__(self, weight_decay, data_format, name=None):
        assert data_format in ['NCHW', 'NHWC'], 'Unknown data format.'
        self.data_format = data_format
        self.channel_axis = 1 if self.data_format == 'NCHW' else 3
        self.spatial_axis = [2, 3] if self.data_format == 'NCHW' else [1, 2]
        self.weight_decay = weight_decay
        self.name = name

    @abc.abstractmethod
    def backbone(self, inputs, is_training, reuse):
        pass

    @abc.abstractmethod
    def forward(self, images, num_classes, is_training):
        pass

    @abc.abstractmethod
    def loss_function(self, scope, labels, **logits):
        pass

    @abc.abstractmethod
    def backward(self):
        """Replaces tf.gradients(total_loss, params): fill the gradient arena for the
        batch that the last forward()/loss_function() saw."""

    def param_list(self, is_training, trainable, scope=None):
        raise NotImplementedError

    def set_margin(self, scale=None, margin=None, margin_cos=None):
        """Margin nets only: replace the head's (S, m, m3) -- train.py --margin_scale / --margin / --margin_cos; None keeps a
        value.  Takes effect from the next forward / loss_function."""
        head = getattr(self, 'head', None)
        if head == 'adaface':                            # S and m; the head has no cosine margin of its own (b_i follows the norm)
            if margin_cos is not None:
                raise ValueError('%s: the AdaFace head has no margin_cos' % self.name)
            self.margin_scale, self.margin, _, _ = adaface_params(self.margin_scale if scale is None else scale,
                                                                  self.margin if margin is None else margin, self.adaface_h, self.adaface_t_alpha)
            return
        if head == 'curricularface':                     # S and m; the head has no cosine margin
            if margin_cos is not None:
                raise ValueError('%s: the CurricularFace head has no margin_cos' % self.name)
            self.margin_scale, self.margin, _ = curricular_params(self.margin_scale if scale is None else scale,
                                                                  self.margin if margin is None else margin, self.curricular_alpha)
            return
        if head == 'magface':                            # S alone; the margin is (l_a, u_a, l_m, u_m) of set_magface
            if margin is not None or margin_cos is not None:
                raise ValueError('%s: the MagFace head has no margin / margin_cos; its margin range is set by --magface '
                                 '(set_magface)' % self.name)
            self.margin_scale = magface_params(self.margin_scale if scale is None else scale, *self.magface)[0]
            return
        if head not in MARGIN_PRESETS:
            raise ValueError('%s has no additive-margin head' % self.name)
        self.margin_scale, self.margin, self.margin_cos = margin_params(
            head, self.margin_scale if scale is None else scale, self.margin if margin is None else margin,
            self.margin_cos if margin_cos is None else margin_cos)

    def set_magface(self, l_a=None, u_a=None, l_m=None, u_m=None, lambda_g=None):
        """MagFace nets only: replace (l_a, u_a, l_m, u_m, lambda_g) -- train.py --magface; None keeps a value.  Takes effect from
        the next forward / loss_function."""
        if getattr(self, 'head', None) != 'magface':
            raise ValueError('%s has no MagFace head (--magface: SphereNet-MagFace, ResNet-50-magface, [SE-]IResNet-*-magface only)' % self.name)
        given = (l_a, u_a, l_m, u_m, lambda_g)
        self.magface = magface_params(self.margin_scale, *(old if v is None else v for old, v in zip(self.magface, given)))[1:]

    def set_sample_rate(self, rate, seed=0):
        """Nets with a sampled-class (Partial FC) head only -- SphereNet-ArcFace / -CosFace; train.py --sample_rate / --sample_seed.
        Every other net (the graph nets and the A-softmax head included) refuses."""
        raise ValueError('%s has no sampled-class head (--sample_rate: SphereNet-ArcFace / SphereNet-CosFace only)' % self.name)

    def mult_lr_list(self, scope=None):
        return [1.0 for _ in self.param_list(is_training=True, trainable=True, scope=scope)]


_SIDE_STREAMS = {}


def side_stream(device, priority=0):
    """The process's second stream on `device` (filter gradients beside the data-gradient chain, the forward walk's second half shard, the
    BN nets' side work): ONE per (device, priority), shared by every net of the process.  A stream per net made the walk's overlap a
    matter of luck: the runtime maps streams onto a few hardware queues round-robin, and the n-th stream created can share its queue
    with the current stream -- the 64-image SphereNet step then read 6.5 ms instead of 5.9 in bench.py's `other_configs` leg, depending
    on which nets had been built before it."""
    import torch
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(priority))
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev, priority=int(priority))
    return s
