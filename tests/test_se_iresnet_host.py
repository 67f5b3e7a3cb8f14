"""CPU: the SE-IResNet nets -- the float64 restatement (tests/se_iresnet_ref.py) against central differences and against the fused
plan op's arithmetic, the factory names against the block table, the plan (one 'selin' op per block), the refusals, the host mirror
of the kernels' split rule on the GPU kernel cases, and the kink bands of the GPU audit's inputs."""
import numpy as np
import pytest

import se_iresnet_ref as sr

from tf_face_toolbox_amd import _lib, net_select
from tf_face_toolbox_amd.nets import plan as planmod
from tf_face_toolbox_amd.nets.iresnet import IResNet


GROUPS = [('conv filters', lambda k: k.endswith('_3x3/weights') or k.endswith('_1x1/weights')),
          ('gamma', lambda k: k.endswith('/gamma') and '/output/fc/' not in k),
          ('beta', lambda k: k.endswith('/beta') and '/output/fc/' not in k),
          ('alpha', lambda k: k.endswith('/prelu/alpha')),
          ('gate fc1 weights', lambda k: k.endswith('/se/fc1/weights')), ('gate fc1 biases', lambda k: k.endswith('/se/fc1/biases')),
          ('gate fc2 weights', lambda k: k.endswith('/se/fc2/weights')), ('gate fc2 biases', lambda k: k.endswith('/se/fc2/biases')),
          ('flatten FC', lambda k: k.endswith('/output/fc/weights')),
          ('last BN', lambda k: '/output/fc/BatchNorm/' in k),
          ('classifier', lambda k: k == sr.CLS)]


@pytest.mark.parametrize('head,fmt', [('softmax', 'NCHW'), ('arcface', 'NHWC')])
def test_restatement_gradients_against_central_differences(head, fmt):
    """d(loss + reg) along a random unit direction inside every variable group (the filters one variable at a time), the four gate
    variables of every block in groups of their own, and single entries of a gate weight and a gate bias.  Step and bound of
    test_iresnet_host.py (h = 1e-6, 2e-6 relative + 1e-8 absolute): the gate adds a sigmoid (smooth) and a hidden ReLU, whose 4 - 32
    units per image move across their kink with probability O(h)."""
    g, spec, p, state, x, y = sr.audit_case()
    kw = dict(head=head, data_format=fmt)
    losses, grads, env, _ = sr.loss_and_grads(g, p, x, y, **kw)
    assert abs(sum(losses) - sr.loss_only(g, p, x, y, **kw)) <= 1e-12 * max(1.0, sum(losses))
    assert sorted(grads) == sorted(p)
    rng = np.random.default_rng(5)
    h = 1e-6

    def fd(direction):
        lp = sr.loss_only(g, {k: v + h * direction.get(k, 0.0) for k, v in p.items()}, x, y, **kw)
        lm = sr.loss_only(g, {k: v - h * direction.get(k, 0.0) for k, v in p.items()}, x, y, **kw)
        return (lp - lm) / (2 * h)
    groups = []
    for what, sel in GROUPS:
        names = [k for k in p if sel(k)]
        assert names, what
        groups.extend([(k, [k]) for k in names] if what == 'conv filters' else [(what, names)])
    assert sorted(k for _, names in groups for k in names) == sorted(p)          # every variable is in exactly one group
    for what, names in groups:
        d = {k: rng.standard_normal(p[k].shape) for k in names}
        norm = np.sqrt(sum(float((v * v).sum()) for v in d.values()))
        d = {k: v / norm for k, v in d.items()}
        ana = sum(float((grads[k] * d[k]).sum()) for k in names)
        num = fd(d)
        assert abs(ana - num) <= 2e-6 * abs(num) + 1e-8, (what, ana, num)
    for k, idx in (('SE-IResNet-18/stage2/block_0/se/fc1/weights', (17, 3)), ('SE-IResNet-18/stage3/block_0/se/fc2/biases', (40,)),
                   ('SE-IResNet-18/stage1/block_0/conv2_3x3/BatchNorm/gamma', (9,))):
        e = np.zeros_like(p[k]); e[idx] = 1.0
        num = fd({k: e})
        assert abs(grads[k][idx] - num) <= 2e-6 * abs(num) + 1e-8, (k, grads[k][idx], num)


@pytest.mark.parametrize('n,h,w,c', [(3, 5, 4, 32), (1, 2, 2, 16)])
def test_fused_block_tail_arithmetic_is_the_composed_block(n, h, w, c):
    """what the plan op 'selin' computes (squeeze from z, per-image sums s1 / s2, the BN backward's sums assembled from them without a
    pass over the tensor) against BN -> gate -> add differentiated op by op, both in float64: 1e-11 relative"""
    r = np.random.default_rng(c + n)
    z, sc, dout = r.standard_normal((n, h, w, c)) * 2 + 1, r.standard_normal((n, h, w, c)), r.standard_normal((n, h, w, c))
    gamma, beta = 1 + 0.2 * r.standard_normal(c), 0.3 * r.standard_normal(c)
    hd = c // 4                                           # (more hidden units than the nets' c / 16: both sides of their ReLU occur)
    fc = (r.standard_normal((c, hd)), r.standard_normal(hd), r.standard_normal((hd, c)) * 0.5, 0.3 * r.standard_normal(c))
    out_a, gp_a, gt_a, cache = sr.block_tail_composed(z, gamma, beta, fc, sc, dout)
    out_b, gp_b, gt_b = sr.block_tail_fused(z, gamma, beta, fc, sc, dout)
    assert (cache['s']['hid'] > 0).any() and (cache['s']['hid'] == 0).any()
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert rel(out_b, out_a) <= 1e-11
    assert rel(gt_b['z'], gt_a['z']) <= 1e-11 and rel(gt_b['sc'], gt_a['sc']) == 0
    for k in gp_a:
        assert rel(gp_b[k], gp_a[k]) <= 1e-11, k


@pytest.mark.parametrize('depth', [18, 34, 50, 100])
@pytest.mark.parametrize('head', ['', '-arcface', '-cosface', '-adaface'])
def test_factory_names_follow_the_block_table(depth, head):
    net = net_select('SE-IResNet-%d%s' % (depth, head), 'NHWC', 1e-4)
    assert isinstance(net, IResNet) and net.se and net.name == 'SE-IResNet-%d' % depth and net.head == (head[1:] or 'softmax')
    assert net.num_block == sr.BLOCKS[depth] and (net.bn_eps, net.bn_decay) == (1e-5, 0.9) and net.weight_decay == 1e-4
    if head not in ('', '-arcface') or depth in (34, 100) or (depth == 50 and head):
        return                                            # (18 with two heads, 50 once: the variables do not depend on the head)
    net.build(112, 96, 3, 100, 'cpu')
    tv, st = sr.expected_variables(depth, 3, 100, 112, 96)
    assert sorted(net.variables) == sorted(k for k, _ in tv)
    for k, shape in tv:
        assert tuple(net.get_variable(k).shape) == shape, k
    assert sorted(net.state) == sorted(k for k, _ in st)
    graph, spec, _ = sr.se_iresnet_graph(depth, 3, 100, 112, 96)
    assert net.graph == graph and [(k, s, kd) for k, (s, kd) in net.spec.items()] == spec
    # the gate's variables as nets/resnet.py types them; stored 64 hidden units wide, the padding exactly zero
    w1 = 'SE-IResNet-%d/stage1/block_0/se/fc1/weights' % depth
    assert net.variables[w1].kind == 'fc_w' and net.variables[w1[:-7] + 'biases'].kind == 'bias'
    assert net.ishape[w1] == (64, 64) and float(net.view(w1).reshape(64, 64)[:, 4:].abs().max()) == 0
    assert float(net.get_variable(w1).abs().max()) > 0 and float(net.get_variable(w1[:-7] + 'biases').abs().max()) == 0


def test_plan_one_selin_per_block_and_nothing_else_changes(monkeypatch):
    net = net_select('SE-IResNet-50')
    net.build(112, 112, 3, 100, 'cpu')
    kinds = [op[0] for op in net.plan]
    assert kinds.count('selin') == 24 and 'se' not in kinds and 'seblock' not in kinds and 'add' not in kinds and 'addrelu' not in kinds
    assert not any(op[0] == 'bn' and op.res is not None for op in net.plan)
    assert set(kinds) == {'conv', 'bn', 'bnprelu', 'selin', 'fc'}
    for j, op in enumerate(net.plan):
        if op[0] != 'selin':
            continue
        assert op._fields == planmod.SeBlock._fields and op.se.hidden == 64 and op.inp.endswith('/c2/z') and op.y.endswith('/c2/bn')
        assert planmod.plan_inputs(op) == [op.inp, op.shortcut] and planmod.op_weight_names(op) == [op.se.w1, op.se.w2]
        assert net.fuse_fwd[j - 1] == j and net.plan[j - 1][0] == 'conv'          # statistics from the producing conv's epilogue
        assert op.shortcut in net.shortcut_shared
        assert net.se_fused[op.y] == ('y', op.out, op.inp) and net.se_fused[op.s] == ('s', op.out, op.inp)
    ident = sum(net.num_block) - 4
    assert len([t for t in net.shortcut_shared if '/' not in t]) == ident and len(net.shortcut_shared) == ident + 4
    assert sum(1 for j in net.shortcut_fwd if net.plan[j][0] == 'bn') == 4          # the four projection shortcuts run on the side stream
    segs = net._segments()
    assert len(segs) == 4 and net.plan[segs[1][0]][1] == 's3b0/sc/z' and net.plan[segs[3][0]][1] == 'out/bn'
    for lo, hi, a, e in segs:                                 # the gate's filters lie in their block's bucket
        for j in range(lo, hi):
            for w in net._op_weight_names(net.plan[j]):
                assert a <= net.variables[w].offset and net.variables[w].offset + net.variables[w].size <= e, w
    # the nets that were there: the same kinds as before
    want = {'IResNet-50': {'conv', 'bn', 'bnprelu', 'fc'},
            'ResNet-50': {'conv', 'bn', 'maxpool', 'gap', 'dropout', 'fc'},
            'SENet-50': {'conv', 'bn', 'seblock', 'maxpool', 'gap', 'dropout', 'fc'},
            'ResNeXt-50': {'conv', 'gconv', 'bn', 'maxpool', 'gap', 'dropout', 'fc'},
            'ShuffleNet-v2-small': None}
    for name, kinds in want.items():
        other = net_select(name)
        other.build(112, 112, 3, 100, 'cpu')
        got = {op[0] for op in other.plan}
        assert 'selin' not in got and 'add' not in got
        if kinds is None:
            assert got == {'conv', 'bn', 'bnstats', 'dwconv', 'gather', 'maxpool', 'gap', 'dropout', 'fc'}, got
        else:
            assert got == kinds, (name, got)
        if name != 'IResNet-50':
            assert other.shortcut_shared == set()
    # FTE_SE_FUSE=0: there is no unfused path
    monkeypatch.setenv('FTE_SE_FUSE', '0')
    with pytest.raises(ValueError, match="SE-IResNet-18: BN -> SE gate -> add without an activation .* 'selin'.*no unfused path"):
        net_select('SE-IResNet-18').build(112, 112, 3, 100, 'cpu')
    net_select('IResNet-18').build(112, 112, 3, 100, 'cpu')              # (the plain net does not care)


def test_a_bare_add_behind_anything_else_still_asserts():
    from tf_face_toolbox_amd.nets.graph import GraphNet

    class Stray(GraphNet):
        feature_name = 'features'

        def build_graph(self, in_ch, num_classes):
            g = [('conv', 'a', 'images', 'S/a/weights', 1), ('conv', 'b', 'images', 'S/b/weights', 1), ('add', 'c', 'a', 'b'), ('gap', 'features', 'c')]
            return g, [('S/a/weights', (3, 3, in_ch, 64), 'conv_w'), ('S/b/weights', (3, 3, in_ch, 64), 'conv_w')]
    with pytest.raises(AssertionError, match='a bare add is always followed by a ReLU'):
        Stray(5e-4, 'NHWC', 'S').build(16, 16, 3, 4, 'cpu')


def test_refusals_inherited_from_iresnet(monkeypatch):
    for name in ('SE-IResNet-26', 'SE-IResNet-50-triplet', 'SE-IResNet', 'SE-IResNet-50-asoftmax', 'SE-ResNet-50'):
        with pytest.raises(ValueError, match='Unsupport network architecture'):
            net_select(name)
    with pytest.raises(ValueError, match='only .* have a K-centre head, not SE-IResNet-50-arcface'):
        net_select('SE-IResNet-50-arcface', sub_centers=2)
    net = net_select('SE-IResNet-18-arcface')
    with pytest.raises(ValueError, match='SE-IResNet-18 has no sampled-class head'):
        net.set_sample_rate(0.1)
    import train as cli
    with pytest.raises(SystemExit, match='--sample_rate 0.1: only .* have a sampled-class head, not SE-IResNet-50-arcface'):
        cli.sample_flags_check(cli.build_parser().parse_args(['--net_name', 'SE-IResNet-50-arcface', '--model_name', 'm', '--sample_rate', '0.1']))
    with pytest.raises(SystemExit, match='--sub_centers 2'):
        cli.sub_centers_flags_check(cli.build_parser().parse_args(['--net_name', 'SE-IResNet-50-arcface', '--model_name', 'm', '--sub_centers', '2']))
    monkeypatch.setattr(_lib, 'bf16_storage', lambda: True)
    with pytest.raises(ValueError, match="SE-IResNet-50: the 'bf16s' storage mode is not implemented for the IResNet nets .* follow-up"):
        net_select('SE-IResNet-50')
    with pytest.raises(ValueError, match="'bf16s' storage mode is not implemented"):
        net._storage16()


@pytest.mark.parametrize('n,hw,c,splits', sr.KERNEL_CASES)
def test_split_rule_on_the_kernel_cases(n, hw, c, splits):
    """the host mirror of se_lin_split gives the splits the GPU test states (256 compute units), the properties stated beside the
    cases hold, and the library's workspace query -- without a device it plans for 256 compute units -- is the mirror's"""
    s, pps = sr.split_plan(n, hw, c)
    assert s == splits and (s - 1) * pps < hw <= s * pps
    if s > 1:
        assert hw >= 64 and pps * sr.quads(c) * 4 >= 256 or pps >= 256 // sr.quads(c)          # every pixel lane of a full split has a pixel
    short = hw - (s - 1) * pps
    facts = {(2, 3136, 64): s == sr.MAX_SPLITS and short == pps and hw < 64 * s,
             (1, 785, 128): short == 3 and hw < 64 * s, (2, 197, 28): short == 32 and sr.quads(c) == 8,
             (2, 130, 116): short == 11 and (c // 4) % 16 != 0, (64, 1100, 64): pps == 69 and short == 65 and pps >= 64,
             (300, 65, 8): sr.split_plan(2, hw, c)[0] > 1, (256, 80, 64): sr.split_plan(2, hw, c)[0] > 1,
             (2, 50, 116): (c // 4) % 16 != 0 and hw < 64, (3, 49, 512): hw < 64, (300, 4, 64): 4 * n >= 1024, (2, 1, 4): True}
    assert facts[(n, hw, c)]
    assert sr.split_plan(n, hw, c, target=0)[0] == 1                              # FTE_SE_LIN_BLOCKS=0: never split
    import torch
    if not torch.cuda.is_available():
        assert _lib.query('fte_se_lin_ws_bytes', n, hw, c) == 2 * s * n * c * 4
    for bad in ((0, hw, c), (n, 0, c), (n, hw, 0), (n, hw, c + 2)):
        assert _lib.query('fte_se_lin_ws_bytes', *bad) == 0


def test_split_rule_at_the_training_shapes():
    """128 images: only the 56 x 56 x 64 stage cannot give every compute unit a block without a split"""
    assert [sr.split_plan(128, hw, c)[0] for hw, c in ((3136, 64), (784, 128), (196, 256), (49, 512))] == [8, 1, 1, 1]
    assert sr.split_plan(128, 3136, 64) == (8, 392)


@pytest.mark.parametrize('blocks', [(1, 1, 1, 1), (2, 1, 1, 1)])
@pytest.mark.parametrize('fmt', ['NCHW', 'NHWC'])
def test_audit_inputs_keep_the_kink_bands_nearly_empty(blocks, fmt):
    """the bands of the GPU audit (max(1e-5 rms(u), 16 x the restatement's own fp32 noise on u)), from the reference alone on the audit's
    inputs: at most 0.1 % of a tensor's elements -- none at all for a gate's hidden layer, which has 24 to 192 of them -- and both
    sides of the hidden ReLU are populated.  (The bf16 operand mode's band, 4 x the restatement's bf16 noise, holds 0.7 - 2 % of a
    tensor by construction -- bf16 rounding against the spread of u -- and is not capped, as for IResNet.)"""
    g, spec, p, state, x, y = sr.audit_case(blocks)
    shares = sr.kink_shares(g, p, x, state, fmt)
    assert sum(1 for k in shares if k.endswith('/se')) == sum(blocks) and len(shares) == 2 * sum(blocks) + 1
    for k, (inside, size) in shares.items():
        assert inside <= sr.KINK_CAP * size, (k, inside, size)
    env, cache, _ = sr.forward(g, p, x, True, state, fmt)
    hid = np.concatenate([cache[op[1]]['pre'].ravel() for op in g if op[0] == 'se'])
    assert (hid > 0).mean() > 0.2 and (hid < 0).mean() > 0.2
