"""IResNet-18 / 34 / 50 / 100 on the graph engine: the "improved residual" backbone of ArcFace (Deng et al., CVPR 2019, section 3.2),
the net the margin-head papers (ArcFace, sub-center ArcFace, Partial FC, AdaFace) train.

  stem    conv 3x3 stride 1, 3 -> 64 -> BN -> PReLU; no pooling
  block   BN -> conv 3x3 -> BN -> PReLU -> conv 3x3 (stride) -> BN, plus the shortcut: the block's input, or conv 1x1 (stride) -> BN in
          the first block of every stage (stride 2, stage 1 included)
  stages  64 / 128 / 256 / 512 channels; 112 x 112 input: 112 (stem) -> 56 / 28 / 14 / 7
  output  BN -> flatten -> FC to 512 (no bias: the BN that follows cancels it exactly) -> BN = `features`

Variable names follow the ResNet scheme: `IResNet-50/stage2/block_0/conv1_3x3/weights`, `.../BatchNorm/{gamma,beta,moving_mean,
moving_variance}`, `.../prelu/alpha`, `classifier/fc_classifier/weights`.  BN + PReLU pairs run fused (csrc/iresnet.hip); batch norm uses
epsilon 1e-5 and momentum 0.9, the published code's values.  Differences from that code are listed in DESIGN.md section 8.

se=True gives SE-IResNet ("IR-SE"): the block's last BN is followed by a squeeze-and-excitation gate before the shortcut is added,
  gate = sigmoid(fc2(relu(fc1(mean_hw(BN output))))), fc1 [c, c / 16] + bias, fc2 [c / 16, c] + bias, variables `.../se/fc1/weights`,
  `.../se/fc1/biases`, `.../se/fc2/...` as nets/resnet.py names them.  BN -> gate -> + shortcut runs as one plan op ('selin', fte.h
  "BN + SE + shortcut, no activation").  The gate's dense layers are stored 64 hidden units wide (zero columns / rows, which stay
  zero): the granularity of the GEMM entry points."""
from .. import _lib
from .graph import GraphNet

BLOCKS = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 14, 3], 100: [3, 13, 30, 3]}
WIDTHS = [64, 128, 256, 512]
EMBED = 512
SE_REDUCTION = 16


def _refuse_bf16s(name):
    if _lib.bf16_storage():
        raise ValueError("%s: the 'bf16s' storage mode is not implemented for the IResNet nets (their BN + PReLU kernels take fp32 tensors "
                         "only); bf16 storage for them is the follow-up -- use 'f32' or 'bf16' (bf16 MFMA operands, fp32 tensors)" % name)


class IResNet(GraphNet):
    bn_eps, bn_decay = 1e-5, 0.9

    def __init__(self, num_layers, weight_decay=0.0005, data_format='NCHW', name='IResNet', seed=0, head='softmax',
                 scale=None, margin=None, margin_cos=None, blocks=None, se=False):
        if num_layers not in BLOCKS:
            raise ValueError('Unsupported num_layers.')
        self.num_layers = num_layers
        self.num_block = list(BLOCKS[num_layers] if blocks is None else blocks)          # blocks=: test-only override of the block counts
        assert len(self.num_block) == 4 and all(b >= 1 for b in self.num_block), self.num_block
        self.se = bool(se)
        if self.se:
            self.se_hidden_pad = 64
        super(IResNet, self).__init__(weight_decay, data_format, ('SE-' if self.se else '') + name + '-' + str(num_layers), seed)
        _refuse_bf16s(self.name)
        self.feature_name = 'features'
        self._set_head(head, scale, margin, margin_cos)

    def _storage16(self):
        _refuse_bf16s(self.name)              # (the mode can be switched after construction)
        return False

    def _segments(self):
        """Four body segments cut at stage boundaries, in forward order: stem + stages 1 and 2, stage 3, stage 4, the output layers.
        The equal-bytes rule of the base class cannot cut behind the flatten FC -- the last and by far the largest filter (a quarter
        to a half of the body) -- so it is a segment of its own here: its bucket, final right after the head's, is reduced under the
        whole of stage 4's backward."""
        if getattr(self, '_segs', None) is None:
            nops = len(self.plan) - (1 if self.has_classifier else 0)
            if self.opt.grad_buckets <= 1:
                self._segs = [(0, nops, 0, self.cls_start)]
            else:
                at = {op[1]: j for j, op in enumerate(self.plan)}
                cuts = [(at['s3b0/sc/z'], self.name + '/stage3/block_0/conv_shortcut_1x1/weights'),
                        (at['s4b0/sc/z'], self.name + '/stage4/block_0/conv_shortcut_1x1/weights'),
                        (at['out/bn'], self.name + '/output/fc/weights')]
                segs, lo, a0 = [], 0, 0
                for j, w in cuts:
                    a = self.variables[w].offset
                    segs.append((lo, j, a0, a))
                    lo, a0 = j, a
                segs.append((lo, nops, a0, self.cls_start))
                self._segs = segs
        return self._segs

    # -- graph construction -------------------------------------------------------------------------
    @staticmethod
    def _bn(g, spec, scope, out, inp, c):
        spec.append((scope + '/BatchNorm/gamma', (c,), 'gamma'))
        spec.append((scope + '/BatchNorm/beta', (c,), 'beta'))
        g.append(('bn', out, inp, scope + '/BatchNorm'))

    @staticmethod
    def _conv(g, spec, scope, out, inp, k, cin, cout, stride):
        spec.append((scope + '/weights', (k, k, cin, cout), 'conv_w'))
        g.append(('conv', out, inp, scope + '/weights', stride))

    @staticmethod
    def _prelu(g, spec, scope, out, inp, c):
        spec.append((scope + '/prelu/alpha', (c,), 'alpha'))
        g.append(('prelu', out, inp, scope + '/prelu/alpha'))

    def block(self, g, spec, scope, t, x, cin, cout, stride, project):
        shortcut = x
        if project:                              # first in plan order: its data gradient runs last and takes the other contribution in
            self._conv(g, spec, scope + '/conv_shortcut_1x1', t + '/sc/z', x, 1, cin, cout, stride)
            self._bn(g, spec, scope + '/conv_shortcut_1x1', t + '/sc/bn', t + '/sc/z', cout)
            shortcut = t + '/sc/bn'
        self._bn(g, spec, scope + '/bn1', t + '/bn1', x, cin)
        self._conv(g, spec, scope + '/conv1_3x3', t + '/c1/z', t + '/bn1', 3, cin, cout, 1)
        self._bn(g, spec, scope + '/conv1_3x3', t + '/c1/bn', t + '/c1/z', cout)
        self._prelu(g, spec, scope + '/conv1_3x3', t + '/c1', t + '/c1/bn', cout)
        self._conv(g, spec, scope + '/conv2_3x3', t + '/c2/z', t + '/c1', 3, cout, cout, stride)
        self._bn(g, spec, scope + '/conv2_3x3', t + '/c2/bn', t + '/c2/z', cout)
        last = t + '/c2/bn'
        if self.se:
            pre, hid = scope + '/se', cout // SE_REDUCTION
            spec.extend([(pre + '/fc1/weights', (cout, hid), 'fc_w'), (pre + '/fc1/biases', (hid,), 'bias'),
                         (pre + '/fc2/weights', (hid, cout), 'fc_w'), (pre + '/fc2/biases', (cout,), 'bias')])
            g.append(('se', t + '/se', last, pre))
            last = t + '/se'
        g.append(('add', t, last, shortcut))
        return t

    def build_graph(self, in_ch, num_classes):
        g, spec = [], []
        s = self.name + '/stem/conv_3x3'
        self._conv(g, spec, s, 'stem/z', 'images', 3, in_ch, 64, 1)
        self._bn(g, spec, s, 'stem/bn', 'stem/z', 64)
        self._prelu(g, spec, s, 'stem', 'stem/bn', 64)
        x, cin = 'stem', 64
        for si, (nb, cout) in enumerate(zip(self.num_block, WIDTHS)):
            for idx in range(nb):
                x = self.block(g, spec, '%s/stage%d/block_%d' % (self.name, si + 1, idx), 's%db%d' % (si + 1, idx), x, cin, cout,
                               2 if idx == 0 else 1, idx == 0)
                cin = cout
        self._bn(g, spec, self.name + '/output', 'out/bn', x, cin)
        h, w, _ = self.in_hwc
        for _ in range(4):
            h, w = (h + 1) // 2, (w + 1) // 2
        spec.append((self.name + '/output/fc/weights', (h * w * cin, EMBED), 'embed_w'))
        g.append(('fc', 'embed', 'out/bn', self.name + '/output/fc/weights', None))
        self._bn(g, spec, self.name + '/output/fc', 'features', 'embed', EMBED)
        spec.append(('classifier/fc_classifier/weights', (EMBED, num_classes), 'cls_w'))
        g.append(('fc', 'logits', 'features', 'classifier/fc_classifier/weights', None))
        return g, spec
