"""CPU: the float64 restatement of the CurricularFace head (tests/curricular_ref.py) against torch autograd of the paper's code
written out literally, its reduction to the ArcFace restatement (tests/margin_ref.py) on the rows without a hard negative, the
recursion of t, and the host surface: symbols, factory names, refusals, command line, the state through saver.py and the
construction-pass switch.

The logit jumps at the mask boundary c_ij = u_i, so every comparison here runs on inputs whose float64 distance to the boundary
exceeds 1e-4 (asserted): both sides then take the same branch on every pair and nothing is excluded."""
import math
import os
import re

import numpy as np
import pytest
import torch

import curricular_ref as cr
import margin_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('fte_curricular_t', 'fte_curricular_softmax_fwd_bwd')
STATE = ('classifier/curricularface/t',)
NAMES = (('SphereNet-CurricularFace', 'ResNet-50-curricularface')
         + tuple('%sIResNet-%d-curricularface' % (se, d) for se in ('', 'SE-') for d in (18, 34, 50, 100)))
D = 512


# ------------------------------------------------------------------------------------------------ the paper's code under autograd
def _paper(x, W, y, S, m, t, alpha=0.01):
    """CurricularFace.forward of the paper's repository in float64, statement for statement -> (loss, dx, dW, t after, mask)"""
    embbedings = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    kernel = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    label = torch.tensor(y, dtype=torch.long)
    t = torch.tensor([t], dtype=torch.float64)
    cos_m, sin_m = math.cos(m), math.sin(m)
    threshold = math.cos(math.pi - m)
    mm = math.sin(math.pi - m) * m
    emb_n = embbedings / embbedings.norm(dim=1, keepdim=True)
    kernel_norm = kernel / kernel.norm(dim=0, keepdim=True)
    cos_theta = torch.mm(emb_n, kernel_norm)
    cos_theta = cos_theta.clamp(-1, 1)
    target_logit = cos_theta[torch.arange(0, emb_n.size(0)), label].view(-1, 1)
    sin_theta = torch.sqrt(1.0 - torch.pow(target_logit, 2))
    cos_theta_m = target_logit * cos_m - sin_theta * sin_m
    mask = cos_theta > cos_theta_m
    final_target_logit = torch.where(target_logit > threshold, cos_theta_m, target_logit - mm)
    hard_example = cos_theta[mask]
    with torch.no_grad():
        t = target_logit.mean() * alpha + (1 - alpha) * t
    cos_theta[mask] = hard_example * (t + hard_example)
    cos_theta.scatter_(1, label.view(-1, 1).long(), final_target_logit)
    output = cos_theta * S
    loss = torch.nn.functional.cross_entropy(output, label)
    loss.backward()
    return float(loss.detach()), embbedings.grad.numpy(), kernel.grad.numpy(), float(t), mask.numpy(), output.detach().numpy()


def _features(rng, W, y, cosines):
    """rows with the given target cosines (plus an orthogonal remainder), norms in [0.5, 20] (tests/test_adaface_host.py)"""
    n = len(cosines)
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    e = rng.standard_normal((W.shape[0], n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    return ((cosines * wy + np.sqrt(1 - cosines ** 2) * e) * rng.uniform(0.5, 20.0, n)).T


def _spread(seed, n=48, c=37):
    """target cosines over [-0.97, 0.97]: rows on both sides of the easy-margin fallback (c_y = -0.95 < -cos m), rows with many hard
    negatives (u below the negatives' cosines) and rows with none (c_y = 0.9: u = 0.58)"""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    cosines = rng.uniform(-0.97, 0.97, n)
    cosines[:4] = [-0.95, 0.9, -0.9, 0.8]
    return _features(rng, W, y, cosines), W, y, cosines


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize('t0', [0.0, 0.35])
@pytest.mark.parametrize('S,m', [(64.0, 0.5), (30.0, 0.4)])
def test_restatement_equals_autograd_of_the_papers_code(t0, S, m):
    x, W, y, cosines = _spread(2)
    assert cr.head_gap(x, W, y, m) > 1e-4                          # no pair near the jump: both sides take the same branch
    assert (cosines < -math.cos(m)).any() and (cosines > -math.cos(m)).any()      # both sides of the fallback
    la, dxa, dWa, ta, mask, out = _paper(x, W, y, S, m, t0)
    lr, f, dxr, dWr, tr = cr.head_fwd_bwd(x, W, y, t0, S, m, 0.01)
    neg = mask.copy()
    neg[np.arange(len(y)), y] = False
    assert 0 < neg.sum() < neg.size and (neg.sum(1) == 0).any() and (neg.sum(1) > 0).any()
    assert abs(tr - ta) <= 1e-12 and tr != t0
    assert np.abs(f - out).max() <= 1e-9 * np.abs(out).max()
    assert abs(lr - la) <= 1e-9 * abs(la)
    assert _rel(dxr, dxa) <= 1e-9 and _rel(dWr, dWa) <= 1e-9, (_rel(dxr, dxa), _rel(dWr, dWa))


def test_update_off_uses_the_stored_t():
    x, W, y, _ = _spread(2)
    on = cr.head_fwd_bwd(x, W, y, 0.35, update=True)
    off = cr.head_fwd_bwd(x, W, y, 0.35, update=False)
    assert off[4] == 0.35 and on[4] != 0.35 and off[0] != on[0]
    again = cr.head_fwd_bwd(x, W, y, on[4], alpha=0.0)             # alpha = 0: t stays, so this is the updated head once more
    assert again[4] == on[4] and again[0] == on[0]


# ------------------------------------------------------------------------------------------------ reduction to ArcFace
def test_rows_without_a_hard_column_are_arcface():
    x, W, y, _ = _spread(4)
    n = len(y)
    S, m = 64.0, 0.5
    s = x @ W
    xn, wn = np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    assert cr.boundary_gap(s, xn, wn, y, m).min() > 1e-4
    cos = cr.cosines(s, xn, wn)
    hard = cos > cr.threshold(cos[np.arange(n), y], m)[:, None]
    hard[np.arange(n), y] = False
    rows = hard.sum(1) == 0
    assert 0 < rows.sum() < n                                      # both kinds of row are present
    for t in (0.0, 0.35):
        fc, lc, Gc, rc = cr.kernel_ref(s, xn, wn, y, S, m, t, 1.0 / n)
        fm, lm, Gm, rm = mr.kernel_ref(s, xn, wn, y, S, m, 0.0, 1.0 / n)
        for g, r in ((fc, fm), (Gc, Gm), (lc, lm), (rc, rm)):
            assert _rel(g[rows], r[rows]) <= 1e-12
        assert _rel(fc[~rows], fm[~rows]) > 1e-3                   # the re-weighting is CurricularFace's alone
    # the target column is ArcFace's on EVERY row, fallback rows included
    idx = np.arange(n)
    np.testing.assert_array_equal(fc[idx, y], fm[idx, y])
    # an explicit mask overrides the compare; all-false is ArcFace everywhere
    f0, l0, G0, r0 = cr.kernel_ref(s, xn, wn, y, S, m, 0.35, 1.0 / n, hard=np.zeros_like(hard))
    assert _rel(f0, fm) <= 1e-12 and _rel(G0, Gm) <= 1e-12
    f1, _, _, _ = cr.kernel_ref(s, xn, wn, y, S, m, 0.35, 1.0 / n, hard=hard)
    np.testing.assert_array_equal(f1, cr.kernel_ref(s, xn, wn, y, S, m, 0.35, 1.0 / n)[0])


def test_bad_label_rows_are_nan_and_leave_the_rest_alone():
    x, W, y, _ = _spread(4, n=6, c=11)
    s, xn, wn = x @ W, np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    yb = y.copy()
    yb[2], yb[4] = 11, -1
    f, l, G, r = cr.kernel_ref(s, xn, wn, yb, 64.0, 0.5, 0.2, 1.0 / 6)
    f2, l2, G2, r2 = cr.kernel_ref(s, xn, wn, y, 64.0, 0.5, 0.2, 1.0 / 6)
    good = [0, 1, 3, 5]
    assert np.isnan(l[[2, 4]]).all() and np.isnan(G[[2, 4]]).all() and np.isnan(r[[2, 4]]).all()
    np.testing.assert_array_equal(G[good], G2[good])
    np.testing.assert_array_equal(l[good], l2[good])


# ------------------------------------------------------------------------------------------------ t
def test_t_recursion_over_three_steps():
    rng = np.random.default_rng(7)
    t, alpha = 0.0, 0.25
    means = []
    for _ in range(3):
        cy = rng.uniform(-0.5, 0.9, 32)
        means.append(cy.mean())
        t = cr.t_update(t, cy, alpha)
    want = alpha * means[2] + (1 - alpha) * (alpha * means[1] + (1 - alpha) * alpha * means[0])
    assert abs(t - want) <= 1e-14
    cy = rng.uniform(-0.5, 0.9, 8)
    valid = np.array([1, 1, 0, 1, 1, 1, 0, 1], bool)
    assert abs(cr.t_update(0.3, cy, 0.01, valid) - (0.01 * cy[valid].mean() + 0.99 * 0.3)) <= 1e-15      # bad labels are left out
    assert cr.t_update(0.3, cy, 0.01, np.zeros(8, bool)) == 0.3                                           # no valid row: unchanged
    assert cr.t_update(0.3, cy, 0.0) == 0.3 and abs(cr.t_update(0.3, cy, 1.0) - cy.mean()) <= 1e-15
    # the head moves t BEFORE it forms the logits: the t it returns is the one the logits were made with
    x, W, y, cosines = _spread(2)
    _, f, _, _, t1 = cr.head_fwd_bwd(x, W, y, 0.0, alpha=0.5)
    cos = cr.cosines(x @ W, np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0))
    assert abs(t1 - 0.5 * cos[np.arange(len(y)), y].mean()) <= 1e-14 and abs(t1) > 1e-3
    i, j = np.argwhere((cos > cr.threshold(cos[np.arange(len(y)), y], 0.5)[:, None]) & (np.arange(cos.shape[1])[None, :] != y[:, None]))[0]
    assert abs(f[i, j] - 64.0 * cos[i, j] * (t1 + cos[i, j])) <= 1e-12


def test_construction_pass_switches_t_off():
    """Singular / DataParallel run their construction-time forward inside _Construction: the nets' update_moving_stats switch is off
    there and back on afterwards; heads.describe passes it to fte_curricular_t as `update`"""
    from tf_face_toolbox_amd import net_select, Singular, heads
    for name in ('SphereNet-CurricularFace', 'ResNet-50-curricularface', 'IResNet-18-curricularface'):
        net = net_select(name)
        assert heads.describe(net) == ('curricularface', 64.0, 0.5, 0.01, 1)
        with Singular._Construction(net):
            assert net.update_moving_stats is False and heads.describe(net)[-1] == 0
        assert net.update_moving_stats is True


# ------------------------------------------------------------------------------------------------ host surface
def test_symbols_are_declared_and_bound():
    from tf_face_toolbox_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fte.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in doc, name
    assert len(_lib._SIGS['fte_curricular_t'][1]) == 12 and len(_lib._SIGS['fte_curricular_softmax_fwd_bwd'][1]) == 16


def test_factory_builds_the_new_names():
    from tf_face_toolbox_amd import net_select
    from tf_face_toolbox_amd.nets import net_base
    assert net_base.CURRICULAR_PRESET == (64.0, 0.5, 0.01) and net_base.CURRICULAR_STATE == STATE
    assert 'curricularface' in net_base.NORMALISED_HEADS and 'curricularface' not in net_base.MARGIN_PRESETS
    for name in NAMES:
        net = net_select(name, 'NCHW', 5e-4)
        assert net.head == 'curricularface', name
        assert (net.margin_scale, net.margin, net.curricular_alpha) == (64.0, 0.5, 0.01)
    for name in NAMES[:3]:
        net = net_select(name, 'NCHW', 5e-4)
        net.set_margin(margin=0.3)                                 # train.py --margin sets m
        assert (net.margin_scale, net.margin) == (64.0, 0.3)
        net.set_margin(scale=32.0)                                 # --margin_scale sets S
        assert (net.margin_scale, net.margin) == (32.0, 0.3)
        with pytest.raises(ValueError, match='no margin_cos'):
            net.set_margin(margin_cos=0.2)
        with pytest.raises(ValueError):
            net.set_margin(margin=-0.1)
        with pytest.raises(ValueError):
            net.set_margin(margin=1.6)                             # m < pi / 2
        with pytest.raises(ValueError, match='sampled-class head'):
            net.set_sample_rate(0.1, 0)
    assert net_select('SphereNet-CurricularFace').needs_labels is True
    with pytest.raises(ValueError):
        net_base.curricular_params(alpha=1.5)


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
        F = cli.build_parser().parse_args(base)                    # the plain command line passes all three
        cli.sample_flags_check(F); cli.sub_centers_flags_check(F); cli.shard_flags_check(F)
        with pytest.raises(ValueError, match='no sharded classifier'):
            check_shard_classes(net_select(name))
    F = cli.build_parser().parse_args(['--net_name', NAMES[0], '--model_name', 'm', '--margin', '0.3', '--margin_scale', '32'])
    assert (F.margin, F.margin_scale, F.margin_cos) == (0.3, 32.0, None)


@pytest.mark.parametrize('name,size,ncls', [('SphereNet-CurricularFace', 16, 7), ('ResNet-50-curricularface', 32, 11)])
def test_state_travels_through_saver(tmp_path, name, size, ncls):
    from tf_face_toolbox_amd import net_select, saver
    net = net_select(name, 'NCHW'); net.seed = 3
    net.build(size, size, 3, ncls, 'cpu')
    assert [k for k in net.state if k.startswith('classifier/curricularface/')] == list(STATE)
    assert STATE[0] not in net.variables                           # not in the arena
    assert tuple(net.get_variable(STATE[0]).shape) == (1,) and float(net.get_variable(STATE[0])) == 0.0
    net.cf_state.fill_(0.4375)                                     # the scalar the kernel updates is what the name shows
    assert float(net.get_variable(STATE[0])) == 0.4375
    path = saver.save(net, None, 5, str(tmp_path / 'a' / 'a.ckpt'))
    saved = torch.load(path, map_location='cpu')['variables']
    assert STATE[0] in saved and tuple(saved[STATE[0]].shape) == (1,)
    other = net_select(name, 'NHWC'); other.seed = 4
    other.build(size, size, 3, ncls, 'cpu')
    assert saver.restore(other, path) == 5
    assert other.cf_state.tolist() == [0.4375]
    for k in list(net.variables) + list(net.state):
        assert torch.equal(other.get_variable(k), net.get_variable(k)), k
    # fine-tuning restores the backbone only: t stays at its initial value
    ft = net_select(name, 'NCHW'); ft.seed = 5
    ft.build(size, size, 3, ncls, 'cpu')
    assert not any(v.name in STATE for v in ft.pretrained_param())
    saver.restore(ft, path, only=ft.pretrained_param())
    assert ft.cf_state.tolist() == [0.0]
