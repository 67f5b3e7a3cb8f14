"""CPU: the float64 restatement of the MagFace head (tests/magface_ref.py) against torch autograd of the paper's published
MagLinear / MagLoss written out literally, against finite differences, its reduction to the ArcFace restatement
(tests/margin_ref.py) when the margin is constant and the regulariser off, and the host surface: parameter validation, symbols,
factory names, refusals, the command line, the lambda_g notice, the loss names, --weight_by_norm.

The target logit jumps at c_iy = -cos mu_i and the norm gradient at xn_i = l_a / u_a, so every comparison runs on inputs whose
float64 distance from both exceeds 1e-4 / 1e-3 relative (asserted): both sides take the same branch and nothing is excluded."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import magface_ref as gr
import margin_ref as mr
import template_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (('SphereNet-MagFace', 'ResNet-50-magface')
         + tuple('%sIResNet-%d-magface' % (se, d) for se in ('', 'SE-') for d in (18, 34, 50, 100)))
PRESET = (64.0, 10.0, 110.0, 0.45, 0.8, 35.0)
D = 512


# ------------------------------------------------------------------------------------------------ the paper's code under autograd
def _paper(x, W, y, S, l_a, u_a, l_m, u_m, lambda_g):
    """MagLinear.forward (easy_margin = False) and MagLoss.forward of the paper's repository in float64, statement for statement,
    and the trainer's total loss = loss + lambda_g * loss_g -> (ce, lambda_g * loss_g, dx, dW, logits)"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    weight = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    target = torch.tensor(y, dtype=torch.long)

    def m(x_norm):                                                  # the trainer's margin function
        return (u_m - l_m) / (u_a - l_a) * (x_norm - l_a) + l_m
    # MagLinear.forward
    x_norm = torch.norm(xt, dim=1, keepdim=True).clamp(l_a, u_a)
    ada_margin = m(x_norm)
    cos_m, sin_m = torch.cos(ada_margin), torch.sin(ada_margin)
    weight_norm = torch.nn.functional.normalize(weight, dim=0)
    cos_theta = torch.mm(torch.nn.functional.normalize(xt), weight_norm)
    cos_theta = cos_theta.clamp(-1, 1)
    sin_theta = torch.sqrt(1.0 - torch.pow(cos_theta, 2))
    cos_theta_m = cos_theta * cos_m - sin_theta * sin_m
    mm = torch.sin(math.pi - ada_margin) * ada_margin
    threshold = torch.cos(math.pi - ada_margin)
    cos_theta_m = torch.where(cos_theta > threshold, cos_theta_m, cos_theta - mm)
    cos_theta_m = S * cos_theta_m
    cos_theta = S * cos_theta
    # MagLoss.forward
    g = 1 / (u_a ** 2) * x_norm + 1 / x_norm
    loss_g = torch.mean(g)
    one_hot = torch.zeros_like(cos_theta)
    one_hot.scatter_(1, target.view(-1, 1), 1.0)
    output = one_hot * cos_theta_m + (1.0 - one_hot) * cos_theta
    loss = torch.nn.functional.cross_entropy(output, target, reduction='mean')
    total = loss + lambda_g * loss_g
    total.backward()
    return float(loss.detach()), float(lambda_g * loss_g.detach()), xt.grad.numpy(), weight.grad.numpy(), output.detach().numpy()


def _features(rng, W, y, cosines, norms):
    """rows with the given target cosines (plus an orthogonal remainder) and the given norms"""
    n = len(cosines)
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    e = rng.standard_normal((W.shape[0], n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    return ((cosines * wy + np.sqrt(1 - cosines ** 2) * e) * norms).T


def _spread(seed, l_a, u_a, n=48, c=37):
    """target cosines over [-0.97, 0.97] -- rows on both sides of the fallback -- and norms below l_a, inside and above u_a in
    turn (row i: zone i % 3), each at least 5 % away from the bounds"""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    cosines = rng.uniform(-0.97, 0.97, n)
    cosines[:6] = [-0.95, 0.9, -0.93, 0.8, -0.96, 0.5]
    zone = np.arange(n) % 3
    norms = np.where(zone == 0, rng.uniform(0.2 * l_a, 0.95 * l_a, n),
                     np.where(zone == 1, rng.uniform(1.05 * l_a, 0.95 * u_a, n), rng.uniform(1.05 * u_a, 2 * u_a, n)))
    return _features(rng, W, y, cosines, norms), W, y, cosines, zone


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


HYPERS = [PRESET, (30.0, 4.0, 40.0, 0.35, 1.2, 5.0), (64.0, 10.0, 110.0, 0.4, 0.8, 0.0)]


@pytest.mark.parametrize('hyper', HYPERS)
def test_restatement_equals_autograd_of_the_papers_code(hyper):
    S, l_a, u_a, l_m, u_m, lg = hyper
    x, W, y, cosines, zone = _spread(2, l_a, u_a)
    gap_c, gap_l, gap_u = gr.head_gaps(x, W, y, l_a, u_a, l_m, u_m)
    assert gap_c > 1e-4 and gap_l > 1e-3 and gap_u > 1e-3           # no row near a jump: both sides take the same branch
    xn = np.linalg.norm(x, axis=1)
    _, mu, _, inside, _ = gr.margins(xn, l_a, u_a, l_m, u_m)
    fallback = cosines < -np.cos(mu)
    for z in range(3):                                              # both target branches in every zone of the norm
        assert (fallback & (zone == z)).any() and (~fallback & (zone == z)).any(), z
    assert (xn < l_a).any() and (xn > u_a).any() and inside.any()
    ce_a, mag_a, dxa, dWa, out = _paper(x, W, y, *hyper)
    ce_r, mag_r, f, dxr, dWr = gr.head_fwd_bwd(x, W, y, *hyper)
    assert np.abs(f - out).max() <= 1e-9 * np.abs(out).max()
    assert abs(ce_r - ce_a) <= 1e-9 * abs(ce_a) and abs(mag_r - mag_a) <= 1e-9 * max(abs(mag_a), 1e-300)
    assert _rel(dxr, dxa) <= 1e-9 and _rel(dWr, dWa) <= 1e-9, (_rel(dxr, dxa), _rel(dWr, dWa))


def test_the_norm_term_is_not_negligible_and_matches_finite_differences():
    """the gradient through the norm is a visible part of dx (dropping it fails this test), and dx is the derivative of
    loss_only along random directions"""
    x, W, y, _, zone = _spread(3, 10.0, 110.0, n=12, c=9)
    _, _, _, dx, dW = gr.head_fwd_bwd(x, W, y, *PRESET)
    s, xn, wn = x @ W, np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    parts = gr.kernel_ref(s, xn, wn, y, *PRESET, 1.0 / len(y), parts=True)
    norm_part = parts[6]
    assert (norm_part[zone != 1] == 0).all() and (np.abs(norm_part[zone == 1]) > 0).all()
    rng = np.random.default_rng(0)
    for _ in range(3):
        d = rng.standard_normal(x.shape) * xn[:, None] / np.sqrt(D)
        h = 1e-6
        fd = (gr.loss_only(x + h * d, W, y, *PRESET) - gr.loss_only(x - h * d, W, y, *PRESET)) / (2 * h)
        assert abs(fd - (dx * d).sum()) <= 1e-6 * max(1.0, abs(fd)), (fd, (dx * d).sum())
        dw = rng.standard_normal(W.shape)
        fd = (gr.loss_only(x, W + h * dw, y, *PRESET) - gr.loss_only(x, W - h * dw, y, *PRESET)) / (2 * h)
        assert abs(fd - (dW * dw).sum()) <= 1e-6 * max(1.0, abs(fd)), (fd, (dW * dw).sum())


@pytest.mark.parametrize('m', [0.5, 0.3])
def test_constant_margin_without_regulariser_is_arcface_exactly(m):
    x, W, y, _, _ = _spread(4, 10.0, 110.0)
    ce, mag, f, dx, dW = gr.head_fwd_bwd(x, W, y, 64.0, 10.0, 110.0, m, m, 0.0)
    ce_a, f_a, dx_a, dW_a = mr.head_fwd_bwd(x, W, y, 64.0, m, 0.0)
    assert mag == 0.0 and ce == ce_a
    assert np.array_equal(f, f_a) and np.array_equal(dx, dx_a) and np.array_equal(dW, dW_a)


def test_rows_outside_the_norm_range_carry_no_norm_gradient():
    x, W, y, _, zone = _spread(5, 10.0, 110.0)
    s, xn, wn = x @ W, np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    n = len(y)
    f, rows, reg, G, rc = gr.kernel_ref(s, xn, wn, y, *PRESET, 1.0 / n)
    for z, m in ((0, 0.45), (2, 0.8)):                              # below l_a the margin is l_m, above u_a it is u_m
        sel = zone == z
        fa, la, Ga, rca = mr.kernel_ref(s[sel], xn[sel], wn, y[sel], 64.0, m, 0.0, 1.0 / n)
        assert np.allclose(f[sel], fa, rtol=0, atol=1e-12) and np.allclose(rows[sel], la, rtol=0, atol=1e-12)
        assert np.allclose(G[sel], Ga, rtol=1e-12, atol=0) and np.allclose(rc[sel], rca, rtol=1e-12, atol=0)
    a = np.clip(xn, 10.0, 110.0)
    assert np.allclose(reg, a / 110.0 ** 2 + 1 / a, rtol=1e-15)


def test_bad_label_rows_are_nan_and_leave_the_rest_alone():
    x, W, y, _, _ = _spread(6, 10.0, 110.0, n=9)
    s, xn, wn = x @ W, np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    want = gr.kernel_ref(s, xn, wn, y, *PRESET, 1.0 / 9)
    bad = y.copy()
    bad[3], bad[5] = W.shape[1], -1
    got = gr.kernel_ref(s, xn, wn, bad, *PRESET, 1.0 / 9)
    good = [0, 1, 2, 4, 6, 7, 8]
    for u, v in zip(got, want):
        assert np.isnan(u[3]).all() and np.isnan(u[5]).all() and np.array_equal(u[good], v[good])


# ------------------------------------------------------------------------------------------------ host surface
def test_parameter_validation():
    from tf_face_toolbox_amd.nets.net_base import MAGFACE_PRESET, magface_params, magface_lambda_bound
    assert MAGFACE_PRESET == PRESET and magface_params() == PRESET
    assert magface_params(32, 5, 50, 0.1, 0.1, 0) == (32.0, 5.0, 50.0, 0.1, 0.1, 0.0)          # u_m = l_m and lambda_g = 0 are valid
    nan = float('nan')
    for bad in (dict(scale=0), dict(scale=-1), dict(scale=nan), dict(l_a=0), dict(l_a=-1), dict(l_a=nan), dict(u_a=10), dict(u_a=5),
                dict(u_a=nan), dict(l_m=-0.1), dict(l_m=nan), dict(u_m=0.4), dict(u_m=math.pi / 2), dict(u_m=1.6), dict(u_m=nan),
                dict(lambda_g=-1), dict(lambda_g=nan)):
        with pytest.raises(ValueError, match='MagFace head needs'):
            magface_params(**bad)
    assert abs(magface_lambda_bound(*PRESET[:5]) - 22.59) < 0.01    # the paper's condition: 22.6 for the preset


def test_symbol_is_declared_bound_and_documented():
    from tf_face_toolbox_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fte.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    name = 'fte_magface_softmax_fwd_bwd'
    assert re.search(r'\b%s\s*\(' % name, hdr) and name in doc
    assert len(_lib._SIGS[name][1]) == 20


def test_factory_builds_the_new_names():
    from tf_face_toolbox_amd import net_select, heads
    from tf_face_toolbox_amd.nets import net_base
    assert 'magface' in net_base.NORMALISED_HEADS and 'magface' not in net_base.MARGIN_PRESETS
    for name in NAMES:
        net = net_select(name, 'NCHW', 5e-4)
        assert net.head == 'magface', name
        assert heads.describe(net) == ('magface',) + PRESET
    for name in NAMES[:3]:
        net = net_select(name, 'NCHW', 5e-4)
        net.set_margin(scale=32.0)                                  # train.py --margin_scale sets S
        assert heads.describe(net) == ('magface', 32.0) + PRESET[1:]
        net.set_magface(5, 50, 0.2, 0.6, 10)                        # train.py --magface
        assert heads.describe(net) == ('magface', 32.0, 5.0, 50.0, 0.2, 0.6, 10.0)
        net.set_magface(lambda_g=0)
        assert heads.describe(net)[-1] == 0.0 and heads.describe(net)[2] == 5.0
        with pytest.raises(ValueError, match='--magface'):
            net.set_margin(margin=0.3)
        with pytest.raises(ValueError, match='--magface'):
            net.set_margin(margin_cos=0.2)
        with pytest.raises(ValueError, match='MagFace head needs'):
            net.set_magface(u_m=1.6)
        with pytest.raises(ValueError, match='sampled-class head'):
            net.set_sample_rate(0.1, 0)
    assert net_select('SphereNet-MagFace').needs_labels is True
    for other in ('SphereNet-ArcFace', 'SphereNet-AdaFace', 'ResNet-50-arcface', 'ResNet-50'):
        with pytest.raises(ValueError, match='no MagFace head'):
            net_select(other).set_magface(lambda_g=1)


def test_a_magface_net_has_the_variable_names_of_the_arcface_net():
    from tf_face_toolbox_amd import net_select
    for mag, arc, size in (('SphereNet-MagFace', 'SphereNet-ArcFace', 16), ('ResNet-50-magface', 'ResNet-50-arcface', 32)):
        a, b = net_select(mag), net_select(arc)
        a.build(size, size, 3, 7, 'cpu'); b.build(size, size, 3, 7, 'cpu')
        assert list(a.variables) == list(b.variables)
        assert list(a.state) == list(b.state)                       # no state variable of the head


def test_refusals_through_net_select_and_the_flag_checks():
    from tf_face_toolbox_amd import net_select
    from tf_face_toolbox_amd.data_parallel import check_shard_classes
    import train as cli
    for name in NAMES[:3]:
        with pytest.raises(ValueError, match='K-centre head'):
            net_select(name, sub_centers=2)
        base = ['--net_name', name, '--model_name', 'm']
        F = cli.build_parser().parse_args(base + ['--sample_rate', '0.1'])
        with pytest.raises(SystemExit, match='only SphereNet-ArcFace / SphereNet-CosFace have a sampled-class head'):
            cli.sample_flags_check(F)
        F = cli.build_parser().parse_args(base + ['--sub_centers', '2'])
        with pytest.raises(SystemExit, match='--sub_centers 2'):
            cli.sub_centers_flags_check(F)
        F = cli.build_parser().parse_args(base + ['--shard_classes', '1', '--num_gpus', '2'])
        with pytest.raises(SystemExit, match='only SphereNet-ArcFace / SphereNet-CosFace have a sharded classifier'):
            cli.shard_flags_check(F)
        with pytest.raises(ValueError, match='no sharded classifier'):
            check_shard_classes(net_select(name))
        for flag in ('--margin', '--margin_cos'):
            F = cli.build_parser().parse_args(base + [flag, '0.3'])
            with pytest.raises(SystemExit, match='--magface'):
                cli.magface_flags_check(F)
        F = cli.build_parser().parse_args(base)                    # the plain command line passes all four; the preset
        cli.sample_flags_check(F); cli.sub_centers_flags_check(F); cli.shard_flags_check(F); cli.magface_flags_check(F)
        assert F.magface_values == PRESET[1:]
        F = cli.build_parser().parse_args(base + ['--magface', '5,50,0.2,0.6,10', '--margin_scale', '32'])
        cli.magface_flags_check(F)
        assert F.magface_values == (5.0, 50.0, 0.2, 0.6, 10.0) and F.margin_scale == 32.0
        for bad in ('5,50,0.2,0.6', '5,50,0.2,0.6,10,1', 'a,b,c,d,e', '50,5,0.2,0.6,10', '5,50,0.2,1.6,10', '5,50,0.2,0.6,-1'):
            F = cli.build_parser().parse_args(base + ['--magface', bad])
            with pytest.raises(SystemExit, match='--magface'):
                cli.magface_flags_check(F)
    for other in ('SphereNet-ArcFace', 'SphereNet-AdaFace', 'ResNet-50-curricularface', 'IResNet-50', 'SphereNet'):
        F = cli.build_parser().parse_args(['--net_name', other, '--model_name', 'm', '--magface', '10,110,0.45,0.8,35'])
        with pytest.raises(SystemExit, match='only the MagFace nets'):
            cli.magface_flags_check(F)
        F = cli.build_parser().parse_args(['--net_name', other, '--model_name', 'm', '--margin', '0.3'])
        cli.magface_flags_check(F)                                  # the other nets keep --margin
        assert F.magface_values is None


def test_the_lambda_g_notice():
    import train as cli
    assert cli.magface_notice(*PRESET) is None                      # 35 > 22.6
    assert cli.magface_notice(64.0, 10.0, 110.0, 0.45, 0.8, 22.6) is None
    text = cli.magface_notice(64.0, 10.0, 110.0, 0.45, 0.8, 22.5)
    assert text and 'lambda_g = 22.5' in text and '22.59' in text
    assert cli.magface_notice(64.0, 10.0, 110.0, 0.5, 0.5, 0.0) is None          # a constant margin needs no regulariser


def test_loss_names_and_their_order(monkeypatch):
    """SphereNet-MagFace reports [cross_entropy, magnitude_loss, reg_loss]; magnitude_loss is fte_sum of reg_rows with the factor
    lambda_g * tower_scale / n into loss slot 2 (the launches are recorded, nothing runs)"""
    from tf_face_toolbox_amd import net_select, _lib
    from tf_face_toolbox_amd.nets import sphere
    net = net_select('SphereNet-MagFace')
    net.build(16, 16, 3, 7, 'cpu')
    net.reg_rows = torch.zeros(4)
    net.loss_rows = torch.zeros(4)
    net.ws, net.ws_bytes = torch.zeros(8), 32
    net.tower_scale = 0.5
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(sphere, '_stream', lambda: 0)
    losses, names, others = net.loss_function('TOWER', torch.zeros(4, dtype=torch.int32))
    assert names == ['cross_entropy', 'magnitude_loss', 'reg_loss'] and not others
    slots = net.loss_slots
    assert [l.data_ptr() for l in losses] == [slots[0].data_ptr(), slots[2].data_ptr(), slots[1].data_ptr()]
    sums = [c for c in calls if c[0] == 'fte_sum']
    assert len(sums) == 2
    assert sums[0][1] is net.loss_rows and sums[0][3] == 0.5 / 4 and sums[0][4].data_ptr() == slots[0].data_ptr()
    assert sums[1][1] is net.reg_rows and sums[1][3] == 35.0 * 0.5 / 4 and sums[1][4].data_ptr() == slots[2].data_ptr()


def test_margin_forward_launches_one_margin_kernel(monkeypatch):
    """ArcFace's launch count: norms, ONE margin kernel, colcoef"""
    from tf_face_toolbox_amd import heads, _lib
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name,) + a))
    b = SimpleNamespace(xn='xn', wn='wn', rowcoef='rc', colcoef='cc', G='G', loss_rows='rows', reg_rows='reg')
    heads.margin_forward(b, 'x', 'W', 's', 'y', 'f', ('magface',) + PRESET, 4, 512, 10, 128, 0.25, 0)
    assert [c[0] for c in calls] == ['fte_row_norms', 'fte_col_norms', 'fte_magface_softmax_fwd_bwd', 'fte_asoftmax_colcoef']
    assert calls[2][1:] == ('s', 'xn', 'wn', 'y') + PRESET + ('f', 'rows', 'reg', 'G', 'rc', 4, 10, 128, 0.25, 0)


def test_train_help_names_the_flag():
    import train as cli
    text = cli.build_parser().format_help()
    assert '--magface' in text and 'l_a,u_a,l_m,u_m,lambda_g' in text


# ------------------------------------------------------------------------------------------------ --weight_by_norm
def test_weight_by_norm_pools_with_the_norms_as_weights(monkeypatch):
    """verify.py's pooling with --weight_by_norm: the unit rows and their norms go to template_pool (stood in for by numpy here; the
    GPU test runs the library); without the flag the metadata column does"""
    import verify
    from tf_face_toolbox_amd import verification as V
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((11, 64)) * rng.uniform(0.1, 10, (11, 1))).astype(np.float32)
    members, media_off, tmpl_off = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [0, 3, 4, 8, 11], [0, 2, 3, 4]
    tpl = dict(members=members, media_off=media_off, tmpl_off=tmpl_off)

    def normalize(t, return_norms=False):
        a = t.numpy().astype(np.float64)
        nrm = np.linalg.norm(a, axis=1)
        return (a / nrm[:, None], nrm) if return_norms else a / nrm[:, None]
    seen = {}

    def template_pool(rows, mem, mo, to, weights=None):
        seen['w'] = weights
        return tr.pool(rows, mem, mo, to, weights)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    monkeypatch.setattr(V, 'normalize', normalize)
    monkeypatch.setattr(V, 'template_pool', template_pool)
    x64 = x.astype(np.float64)
    nrm = np.linalg.norm(x64, axis=1)
    got = verify._pooled(x, tpl, {'weight': None}, True)
    assert np.allclose(got, tr.pool(x64 / nrm[:, None], members, media_off, tmpl_off, nrm), rtol=0, atol=1e-12)
    assert np.allclose(seen['w'], nrm)
    plain = verify._pooled(x, tpl, {'weight': None}, False)
    assert seen['w'] is None and np.abs(plain - got).max() > 1e-3  # the weights matter on this set
    col = rng.uniform(0.5, 2, 11)
    verify._pooled(x, tpl, {'weight': col}, False)
    assert seen['w'] is col


def test_weight_by_norm_flag_checks():
    import verify
    base = ['--feature_path', 'f', '--data_list_path', 'l']
    P = verify.build_parser()
    verify.weight_flags_check(P.parse_args(['--protocol', 'templates', '--weight_by_norm', '1'] + base))
    verify.weight_flags_check(P.parse_args(['--protocol', 'template_search', '--weight_by_norm', '1'] + base))
    verify.weight_flags_check(P.parse_args(['--protocol', 'pairs', '--weight_column', 'Q'] + base))
    with pytest.raises(SystemExit, match='--weight_column'):
        verify.weight_flags_check(P.parse_args(['--protocol', 'templates', '--weight_by_norm', '1', '--weight_column', 'Q'] + base))
    with pytest.raises(SystemExit, match='--weight_by_norm'):
        verify.weight_flags_check(P.parse_args(['--protocol', 'pairs', '--weight_by_norm', '1'] + base))
    with pytest.raises(SystemExit, match='--weight_by_norm'):
        verify.weight_flags_check(P.parse_args(['--protocol', 'templates', '--fusion', 'softmax', '--weight_by_norm', '1'] + base))
