"""-m gpu: the margin classifier split by class over the ranks (DataParallel(shard_classes=True), include/fte.h "Sharded margin head",
DESIGN.md 4.20) -- 2 and 4 ranks against the float64 restatement of the GLOBAL batch (tests/margin_ref.py), the construction pass, the
collectives a step makes, dense checkpoints both ways, the refusals and the command line.  The multi-rank runs are real processes
(tests/shard_dp_worker.py under torch.distributed.run): RCCL with a GPU per rank, gloo on one shared GPU; the result files record
which ran."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as mr
import pfc_dp_case as case
import sharded_head_ref as shr
import test_gpu_margin as tgm
from oracle import ops, spherenet as osn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS = 'classifier/fc_classifier/weights'
D = 512

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2
    from tf_face_toolbox_amd import net_select, DataParallel, DataParallel_margin, saver


def _case(world, per_rank, ncls):
    """pfc_dp_case's fixed case; at 1001 classes (4 ranks: shards of 251, 251, 251 and 248) the same seeds with the wider classifier
    and the last label on class 1000, in the short last shard"""
    if ncls == case.NCLS:
        return case.case(world, per_rank)
    seed = 91
    p = osn.perturb_params(osn.init_params(seed, case.CH, ncls, case.H, case.W), seed + 1)
    x = np.random.default_rng(seed + 2).uniform(-1, 1, (world * per_rank, case.H, case.W, case.CH))
    y = case.labels_for(world, per_rank)
    y[-1] = ncls - 1
    return p, x, y


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(tmp_path, mode, world, name, steps, tag='out', timeout=600, **fix):
    path = str(tmp_path / (tag + '.fix.npz'))
    p = fix.pop('p', {})
    np.savez(path, **dict(fix, **{'p:' + k: v for k, v in p.items()}))
    out = str(tmp_path / tag)
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='2')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
                        '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
                        os.path.join(ROOT, 'tests', 'shard_dp_worker.py'), mode, path, out, name, str(steps)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:]
    res = [np.load(out + '.rank%d.npz' % k) for k in range(world)]
    rccl = torch.cuda.device_count() >= world and os.environ.get('FTE_TEST_FORCE_GLOO') != '1'
    for k, rk in enumerate(res):
        assert str(rk['backend']) == ('nccl' if rccl else 'gloo')
        assert int(rk['device']) == (k if rccl else 0)
    print('transport: %s, %d ranks' % ('nccl' if rccl else 'gloo', world))
    return res


def _steps(tmp_path, world, name, steps, p, x, y, ncls, tag='out', opt='Momentum', lr=0.05, save_at=-1, restore=''):
    return _launch(tmp_path, 'steps', world, name, steps, tag=tag, x=x, y=y, ncls=ncls, p=p, opt=opt, lr=lr, save_at=save_at,
                   ckpt=str(tmp_path / 'ckpt' / 'm.ckpt'), restore=restore)


def _side_by_side(res, key, ncls):
    """the ranks' [512, ld] shards cut to their live columns, in rank order"""
    cols = [rk[key][:, :int(rk['range'][1] - rk['range'][0])] for rk in res]
    out = np.concatenate(cols, axis=1)
    assert out.shape == (D, ncls)
    return out


def _check_run(res, world, ncls, per_rank, steps):
    """what every sharded run must show, whatever it is compared with afterwards"""
    N = world * per_rank
    ranges = shr.shard_ranges(ncls, world)
    for k, rk in enumerate(res):
        lo, hi, ld, arena, cls_start = (int(v) for v in rk['range'])
        assert (lo, hi) == ranges[k] and ld == (ranges[0][1] + 127) // 128 * 128 and arena == cls_start + D * ld      # equal on all ranks
        assert tuple(rk['logits_shape']) == (N, hi - lo)
        # the construction pass: the ranks started different; now every backbone is rank 0's and the shard is the rank's columns of
        # the dense initial value, its pads zero
        assert str(rk['init_backbone_sha']) == str(res[0]['init_backbone_sha']) == str(res[0]['init_dense_backbone_sha'])
        assert k == 0 or str(rk['init_dense_backbone_sha']) != str(res[0]['init_dense_backbone_sha'])
        np.testing.assert_array_equal(rk['init_shard'][:, :hi - lo], rk['init_dense_cols'])
        assert (rk['init_shard'][:, hi - lo:] == 0).all() and (rk['shard'][:, hi - lo:] == 0).all()
        assert [c.split(':')[0] for c in rk['setup_calls']].count('broadcast') == 1
        assert [c for c in rk['setup_calls'] if c.startswith('broadcast')] == ['broadcast:%d:0' % cls_start]      # params[0:cls_start) only
        # the backbone bytes are equal on all ranks after every step, the losses too
        assert list(rk['backbone_sha']) == list(res[0]['backbone_sha']) and len(set(rk['backbone_sha'])) == steps
        np.testing.assert_array_equal(rk['losses'], res[0]['losses'])
        # a step's collectives: the features, the labels and the statistics are gathered, dx is reduce-scattered, and what is
        # all-reduced is the backbone's gradient and the four loss slots -- nothing touches the classifier's range
        for line in rk['calls']:
            calls = [c.split(':') for c in line.split('|')]
            assert [c[1] for c in calls if c[0] == 'all_gather'] == [str(N * D), str(N), str(world * 3 * N)], line
            assert [c[1] for c in calls if c[0] == 'reduce_scatter'] == [str(N * D)], line
            assert not any(c[0] == 'broadcast' for c in calls)
            reduced = [c for c in calls if c[0] == 'all_reduce']
            assert all(c[2] == '0' for c in reduced), 'an all-reduce touches the classifier gradient: ' + line
            assert sorted(int(c[1]) for c in reduced)[0] == 4 and sum(int(c[1]) for c in reduced) == cls_start + 4, line
        # get_variable's dense classifier is the shards side by side, bit for bit, on every rank
        np.testing.assert_array_equal(rk['w:' + CLS], _side_by_side(res, 'shard', ncls))


def _against_the_global_batch(tmp_path, name, world, per_rank, ncls, steps=3, **kw):
    preset = case.PRESETS[name]
    p, x, y = _case(world, per_rank, ncls)
    owners = [sum(lo <= v < hi for v in y) for lo, hi in shr.shard_ranges(ncls, world)]
    assert all(owners), owners                                 # every shard owns a label of the batch
    res = _steps(tmp_path, world, name, steps, p, x, y, ncls, **kw)
    _check_run(res, world, ncls, per_rank, steps)
    slots = osn.zero_slots(p)
    ref_losses = []
    for t in range(steps):
        gap = case.arc_gap(p, x, y, preset[1])
        assert gap >= case.ARC_GAP, (t, gap)                   # the oracle's own cosines, away from the ArcFace threshold
        kink = {c: np.concatenate([rk['z:%d:%s' % (t, c)] for rk in res]).astype(np.float64)
                for c in (key.split(':', 2)[2] for key in res[0].files if key.startswith('z:0:'))}
        p, slots, ls = mr.train_step(p, slots, x, y, 0.05, *preset, kink=kink)
        ref_losses.append(ls)
    print('losses', res[0]['losses'].tolist(), 'ref', np.array(ref_losses).tolist())
    worst = max((np.sqrt(((res[0]['w:' + k].astype(np.float64) - p[k]) ** 2).sum()) / max(np.sqrt((p[k] * p[k]).sum()), 1e-30), k) for k in p)
    print('worst relative L2 %.3e (%s)' % worst)
    np.testing.assert_allclose(res[0]['losses'], np.array(ref_losses), rtol=2e-5)
    assert worst[0] <= 2e-5, worst
    return res


@pytest.mark.parametrize('name', ['SphereNet-ArcFace', 'SphereNet-CosFace'])
def test_two_ranks_equal_the_global_batch_oracle(tmp_path, name):
    _against_the_global_batch(tmp_path, name, 2, 4, case.NCLS)


def test_four_ranks_with_a_short_last_shard_equal_the_global_batch_oracle(tmp_path):
    _against_the_global_batch(tmp_path, 'SphereNet-ArcFace', 4, 2, 1001)


def test_one_adam_step_on_two_ranks(tmp_path):
    """against oracle.ops.adam_step on the restatement's gradient g of the global batch.  Adam's first step is
    u(g) = lr_t (1 - b1) g / (sqrt(1 - b2) |g| + eps), ~lr sign(g): an element whose |g| is below fp32's resolution of the tensor moves
    by anything in [-lr, lr], and among the classifier's 512,000 elements some always are (a bound of 2e-3 max |w|, which holds for the
    5,120 elements of tests/test_gpu_spherenet.py's classifier, does not: first written so here, 1.6e-5 against 1.1e-5 on one
    element).  So the step is held elementwise to the image under u of the band the gradient itself is allowed: u is monotonic, a
    gradient within delta = 2e-5 max |g| of g (util_gpu's max-abs bound, applied to the gradient tensor) gives a step within
    [u(g - delta), u(g + delta)], plus 2e-5 max |w| for the weights' own fp32 rounding."""
    name, world, per_rank, lr = 'SphereNet-ArcFace', 2, 4, 1e-3
    p, x, y = _case(world, per_rank, case.NCLS)
    res = _steps(tmp_path, world, name, 1, p, x, y, case.NCLS, opt='Adam', lr=lr)
    _check_run(res, world, case.NCLS, per_rank, 1)
    kink = {c: np.concatenate([rk['z:0:%s' % c] for rk in res]).astype(np.float64)
            for c in (key.split(':', 2)[2] for key in res[0].files if key.startswith('z:0:'))}
    losses, g, _ = mr.loss_and_grads(p, x, y, *case.PRESETS[name], kink=kink)
    np.testing.assert_allclose(res[0]['losses'][0], np.array(losses), rtol=2e-5)
    assert len(res[0]['slots_sha']) == 2
    b1, b2, eps = 0.5, 0.999, 1e-8
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    u = lambda v: lr_t * (1 - b1) * v / (np.sqrt(1 - b2) * np.abs(v) + eps)
    for k in p:
        ref = ops.adam_step(p[k], np.zeros_like(p[k]), np.zeros_like(p[k]), g[k], lr, 1)[0]
        np.testing.assert_allclose(p[k] - u(g[k]), ref, rtol=0, atol=1e-12)      # u restates oracle.ops.adam_step at t = 1
        delta = 2e-5 * np.abs(g[k]).max()
        lo_, hi_ = p[k] - u(g[k] + delta), p[k] - u(g[k] - delta)
        slack = 2e-5 * np.abs(ref).max()
        got = res[0]['w:' + k].astype(np.float64)
        assert np.all(got >= lo_ - slack) and np.all(got <= hi_ + slack), \
            ('after one Adam step ' + k, float(np.maximum(lo_ - got, got - hi_).max()), slack)
        assert np.abs(got - p[k]).max() > 0.5 * lr
        inside = np.abs(g[k]) > 100 * delta                    # where the band is narrow the step is the oracle's to 2 % of lr
        assert np.all(np.abs(got - ref)[inside] <= 0.02 * lr + slack), k


def test_save_restore_and_a_dense_net_reads_the_checkpoint(tmp_path):
    """3 uninterrupted steps with a save after the second; fresh nets restore it and take 1 step: the same bytes.  The checkpoint is
    dense: a fresh dense one-GPU net restores it and holds the shards side by side bit for bit, and the sharded ranks restore a
    checkpoint a dense net wrote."""
    name, world, per_rank, ncls = 'SphereNet-ArcFace', 2, 4, case.NCLS
    p, x, y = _case(world, per_rank, ncls)
    full = _steps(tmp_path, world, name, 3, p, x, y, ncls, tag='full', save_at=2)
    path = saver.latest_checkpoint(str(tmp_path / 'ckpt'))
    assert path and path.endswith('m.ckpt-2')
    for rk in full:                                            # the save is one all-gather per classifier tensor (weights + 1 slot), on every rank
        assert [c.split(':')[0] for c in rk['save_calls']] == ['all_gather', 'all_gather'], list(rk['save_calls'])
    state = torch.load(path, map_location='cpu')
    assert tuple(state['variables'][CLS].shape) == (D, ncls) and tuple(state['slots'][0][CLS].shape) == (D, ncls)
    resumed = _steps(tmp_path, world, name, 1, p, x, y, ncls, tag='resumed', restore=path)
    for a, b in zip(full, resumed):
        assert int(b['global_step']) == 3 == int(a['global_step'])
        assert str(a['arena_sha']) == str(b['arena_sha']) and list(a['slots_sha']) == list(b['slots_sha'])
        np.testing.assert_array_equal(a['losses'][2], b['losses'][0])
    # a fresh DENSE net on one GPU restores the sharded checkpoint
    net = net_select(name, 'NCHW', 5e-4)
    net.build(case.H, case.W, case.CH, ncls, 'cuda')
    assert saver.restore(net, path) == 2
    np.testing.assert_array_equal(net.get_variable(CLS).cpu().numpy(), _side_by_side(full, 'saved_shard', ncls))
    np.testing.assert_array_equal(state['slots'][0][CLS].numpy(), _side_by_side(full, 'saved_slot_shard', ncls))
    assert float(np.abs(_side_by_side(full, 'saved_slot_shard', ncls)).max()) > 0
    # ... and the other way round: the dense net writes a checkpoint, sharded ranks start from it
    dense_path = saver.save(net, None, 2, str(tmp_path / 'dense' / 'd.ckpt'))
    again = _steps(tmp_path, world, name, 1, p, x, y, ncls, tag='again', restore=dense_path)
    for a, b in zip(full, again):
        np.testing.assert_array_equal(a['losses'][2], b['losses'][0])      # (no slots in that file: the loss of the step is what must agree)


# ------------------------------------------------------------------------------------------------ loss.sharded_margin_loss
@pytest.mark.parametrize('preset', [tgm.ARC, tgm.COS], ids=['arcface', 'cosface'])
def test_public_loss_function_on_two_ranks(tmp_path, preset):
    rng = np.random.default_rng(19)
    world, n, c = 2, 8, 1001
    W = rng.standard_normal((D, c)).astype(np.float32)
    y = rng.integers(0, c, world * n)
    y[0], y[-1] = 0, c - 1
    x = tgm._features(rng, W, y, world * n)
    res = _launch(tmp_path, 'loss', world, '-', 0, x=x, w=W, y=y, ncls=c, preset=np.array(preset))
    lr, _, dxr, dWr = mr.head_fwd_bwd(x.astype(np.float64), W.astype(np.float64), y, *preset)
    for rk in res:
        assert abs(float(rk['loss']) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(rk['loss']), lr)
    assert float(res[0]['loss']) == float(res[1]['loss'])
    check_rell2(np.concatenate([rk['dx'] for rk in res]), dxr, what='dfeatures')
    check_rell2(_side_by_side(res, 'dw', c), dWr, what='dweights')
    for rk in res:
        assert (rk['dw'][:, int(rk['range'][1] - rk['range'][0]):] == 0).all()


# ------------------------------------------------------------------------------------------------ refusals, CLI
class _Ranks(object):
    """a collective layer that only answers who is there: the refusals come before anything is communicated"""

    def __init__(self, world, rank=0):
        self.world, self.r = world, rank

    def world_size(self):
        return self.world

    def rank(self):
        return self.r

    def __getattr__(self, name):
        raise AssertionError('the refusal came after a collective: ' + name)


def test_refusals():
    arc = lambda **kw: net_select('SphereNet-ArcFace', 'NCHW', 5e-4, **kw)
    for wrapper in (DataParallel, DataParallel_margin):
        net = arc()
        net.set_sample_rate(0.1, 0)
        with pytest.raises(ValueError, match='does not compose with the class sampler'):
            wrapper(net, 0.1, 'Momentum', num_gpus=2, shard_classes=True)
        with pytest.raises(ValueError, match='does not compose with the class sampler'):
            wrapper(net, 0.1, 'Momentum', num_gpus=2, shard_classes=True, sync_sample=True)
        with pytest.raises(ValueError, match='does not compose with sync_sample'):
            wrapper(arc(), 0.1, 'Momentum', num_gpus=2, shard_classes=True, sync_sample=True)
        with pytest.raises(ValueError, match=r'does not compose with sub_centers = 3'):
            wrapper(arc(sub_centers=3), 0.1, 'Momentum', num_gpus=2, shard_classes=True)
        for other in ('SphereNet-ASoftmax', 'SphereNet-AdaFace', 'SphereNet', 'ResNet-50-arcface', 'IResNet-18'):
            with pytest.raises(ValueError, match='shard_classes'):
                wrapper(net_select(other, 'NCHW', 5e-4), 0.1, 'Momentum', num_gpus=2, shard_classes=True)
        built = arc()
        built.build(case.H, case.W, case.CH, 10, 'cuda')
        with pytest.raises(ValueError, match='already built with the dense classifier'):
            wrapper(built, 0.1, 'Momentum', num_gpus=2, shard_classes=True)
    # a split that leaves a rank without a class: 9 classes over 8 ranks is 2 per rank, ranks 5..7 would be empty -- refused on every
    # rank before the net is built and before anything is communicated
    x, y = dev(np.zeros((2, case.H, case.W, case.CH))), dev(np.array([0, 8]), torch.int32)
    for rank in (0, 7):
        net = arc()
        model = DataParallel_margin(net, 0.1, 'Momentum', num_gpus=8, comm=_Ranks(8, rank), shard_classes=True)
        with pytest.raises(ValueError, match='leaves rank 5 without a class'):
            model({'images': x, 'labels': y, 'num_classes': 9, 'num_examples': 16, 'batch_size': 16})
        assert not net.built
    # shard_classes off: the argument changes nothing
    model = DataParallel_margin(arc(), 0.1, 'Momentum', num_gpus=2)
    assert model.shard_classes is False


def _train(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='2', FTE_BENCH_SHARED_GPU='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm',
                           '--synthetic', '1', '--synthetic_classes', '1001', '--input_height', '32', '--input_width', '32',
                           '--batch_size', '8', '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50',
                           '--display_interval', '1', '--save_interval', '1000', '--max_steps', '2'] + args,
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=cwd)


def test_train_cli(tmp_path):
    r = _train(['--num_gpus', '2', '--shard_classes', '1'], str(tmp_path))
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'classifier: 2 shards of 501 classes' in r.stdout, r.stdout[-4000:]
    lines = [l for l in r.stdout.splitlines() if 'Loss #0: cross_entropy' in l]
    assert len(lines) == 2 and all(np.isfinite(float(l.rsplit('=', 1)[1])) for l in lines), r.stdout[-4000:]
    assert 'Model has been saved in Iteration 1' in r.stdout
    path = tmp_path / 'models' / 'SphereNet-ArcFace_m' / 'SphereNet-ArcFace_m.ckpt-2'      # (the index names it relative to the run's cwd)
    assert path.exists(), r.stdout[-2000:]
    state = torch.load(str(path), map_location='cpu')
    assert tuple(state['variables'][CLS].shape) == (D, 1001) and tuple(state['slots'][0][CLS].shape) == (D, 1001)
    assert torch.isfinite(state['variables'][CLS]).all() and float(state['slots'][0][CLS].abs().max()) > 0
