"""-m gpu: the sampled-class (Partial FC) head under data parallelism and its compact classifier update (include/fte.h "Partial FC",
DESIGN.md 4.13) -- the fused update kernels against scatter + dense update bit for bit, 2 and 4 ranks with one shared class sample
against the float64 restatement of the GLOBAL batch (tests/partial_fc_ref.py), Singular with and without the compact update bit for
bit, the refusals and the command line.  The multi-rank runs are real processes (tests/pfc_dp_worker.py under torch.distributed.run):
RCCL with a GPU per rank, gloo on one shared GPU; the result files record which ran."""
import glob
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import partial_fc_ref as pr
import pfc_dp_case as case
from oracle import spherenet as osn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 512

if torch.cuda.is_available():
    from util_gpu import dev, call, stream
    from tf_face_toolbox_amd import net_select, Singular, DataParallel, DataParallel_margin, _lib
    from tf_face_toolbox_amd.loss import sample_size


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _inverse(C, S, kind, rng):
    if kind == 'none':
        return np.full(C, -1, np.int64)
    if kind == 'all':
        assert S == C
        return np.arange(C)
    inv = np.full(C, -1, np.int64)
    inv[np.sort(rng.permutation(C)[:S])] = np.arange(S)
    return inv


def _pair(opt, W, slots, dWs, inv, d, C, cpad, S, spad, scal, t):
    """(fused, scatter + dense) results as lists of numpy arrays [W, slot...]"""
    outs = []
    for fused in (True, False):
        Wd = dev(W)
        sl = [dev(s) for s in slots]
        dWsd, invd = dev(dWs), dev(inv, torch.int32)
        if fused:
            if opt == 'Momentum':
                call('fte_pfc_momentum_update_cols', Wd, sl[0], dWsd, invd, d, C, cpad, S, spad, *scal, stream())
            else:
                call('fte_pfc_adam_update_cols', Wd, sl[0], sl[1], dWsd, invd, d, C, cpad, S, spad, *scal, t, stream())
        else:
            dW = torch.full((d, cpad), float('nan'), device='cuda')
            call('fte_pfc_scatter_cols', dWsd, invd, dW, d, C, cpad, S, spad, stream())
            if opt == 'Momentum':
                call('fte_momentum_update', Wd, sl[0], dW, d * cpad, *scal, stream())
            else:
                call('fte_adam_update', Wd, sl[0], sl[1], dW, d * cpad, *scal, t, stream())
        torch.cuda.synchronize()
        outs.append([Wd.cpu().numpy()] + [s.cpu().numpy() for s in sl])
    return outs


# C not a multiple of 4 with cpad > C; S just below and at a multiple of 64; D not a multiple of 16; no class / every class sampled
SHAPES = [(1001, 1024, 127, 512, 'some'), (1001, 1024, 128, 16, 'some'), (333, 384, 65, 7, 'some'), (85742, 85760, 8575, 37, 'some'),
          (1001, 1024, 100, 20, 'none'), (1001, 1024, 1001, 20, 'all'), (1000, 1000, 64, 33, 'some')]


@pytest.mark.parametrize('opt,t', [('Momentum', 0), ('Adam', 1), ('Adam', 100000)])
@pytest.mark.parametrize('C,cpad,S,d,kind', SHAPES)
def test_fused_update_equals_scatter_plus_dense_update_bit_for_bit(C, cpad, S, d, kind, opt, t):
    rng = np.random.default_rng(C + S + d + t)
    spad = (S + 63) // 64 * 64
    inv = _inverse(C, S, kind, rng)
    W = rng.standard_normal((d, cpad)).astype(np.float32)
    W[:, C:] = 0
    W[0, 1] = -0.0
    slots = [rng.standard_normal((d, cpad)).astype(np.float32) * 0.1]
    if opt == 'Adam':
        slots.append((rng.standard_normal((d, cpad)) ** 2).astype(np.float32) * 0.01)
        slots[1][1, :8] = 0.0                                  # sqrt(0) + eps in the step
    slots[0][0, :4] = [0.0, -0.0, 0.0, -0.0]
    dWs = rng.standard_normal((d, spad)).astype(np.float32)
    sampled = np.flatnonzero(inv >= 0)
    if len(sampled):
        dWs[d // 2, inv[sampled[len(sampled) // 2]]] = np.nan  # a NaN in a sampled column: must reach W and the slots
    if spad > S:
        dWs[:, S:] = np.nan                                    # NaNs in the padding of dWs: dropped
    scal = (0.05, 0.9, 5e-4, 1.0) if opt == 'Momentum' else (0.01, 0.5, 0.999, 1e-8, 5e-4 * 0.5, 0.5)
    fused, dense = _pair(opt, W, slots, dWs, inv, d, C, cpad, S, spad, scal, t)
    for a, b, what in zip(fused, dense, ('W', 'slot 0', 'slot 1')):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)      # NaN and +-0 patterns included
    nan_w = np.isnan(fused[0])
    if len(sampled):
        j = sampled[len(sampled) // 2]
        assert nan_w[d // 2, j] and nan_w.sum() == 1, nan_w.sum()
    else:
        assert not nan_w.any()
    assert not np.array_equal(fused[0], W)                     # the update moved the weights


def test_fused_update_invalid_arguments():
    d, C, cpad, S, spad = 16, 1000, 1024, 100, 128
    W, a, v = (torch.zeros(d * cpad + 4, device='cuda') for _ in range(3))
    dWs = torch.zeros(d, spad, device='cuda')
    inv = torch.full((C + 4,), -1, dtype=torch.int32, device='cuda')
    mom, adam = (0.05, 0.9, 0.0, 1.0), (0.01, 0.5, 0.999, 1e-8, 0.0, 1.0)
    call('fte_pfc_momentum_update_cols', W, a, dWs, inv, d, C, cpad, S, spad, *mom, stream())           # the valid call
    call('fte_pfc_adam_update_cols', W, a, v, dWs, inv, d, C, cpad, S, spad, *adam, 1, stream())
    bad = [(0, C, cpad, S, spad), (d, 0, cpad, S, spad), (d, C, 999, S, spad), (d, C, 1022, S, spad), (d, C, cpad, 0, spad),
           (d, C, cpad, S, S - 1)]
    for shp in bad:
        with pytest.raises(_lib.FteError):
            call('fte_pfc_momentum_update_cols', W, a, dWs, inv, *shp, *mom, stream())
        with pytest.raises(_lib.FteError):
            call('fte_pfc_adam_update_cols', W, a, v, dWs, inv, *shp, *adam, 1, stream())
    shp = (d, C, cpad, S, spad)
    for args in ((None, a, dWs, inv), (W, None, dWs, inv), (W, a, None, inv), (W, a, dWs, None),
                 (W[1:], a, dWs, inv), (W, a[1:], dWs, inv), (W, a, dWs, inv[1:])):                     # NULL, misaligned
        with pytest.raises(_lib.FteError):
            call('fte_pfc_momentum_update_cols', *args, *shp, *mom, stream())
    for args in ((W, a, None, dWs, inv), (W, a, v[1:], dWs, inv), (W[1:], a, v, dWs, inv)):
        with pytest.raises(_lib.FteError):
            call('fte_pfc_adam_update_cols', *args, *shp, *adam, 1, stream())
    with pytest.raises(_lib.FteError):
        call('fte_pfc_adam_update_cols', W, a, v, dWs, inv, *shp, *adam, 0, stream())                   # t < 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. / 4. ranks against the oracle
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(tmp_path, mode, world, name, steps, p, x, y, rate=case.RATE, timeout=900):
    fix = str(tmp_path / 'fix.npz')
    np.savez(fix, x=x, y=y, ncls=case.NCLS, rate=rate, sample_seed=case.SAMPLE_SEED, **{'p:' + k: v for k, v in p.items()})
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='2')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
                        '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
                        os.path.join(ROOT, 'tests', 'pfc_dp_worker.py'), mode, fix, out, name, str(steps)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:]
    res = [np.load(out + '.rank%d.npz' % k) for k in range(world)]
    rccl = torch.cuda.device_count() >= world and os.environ.get('FTE_TEST_FORCE_GLOO') != '1'
    for k, rk in enumerate(res):
        assert str(rk['backend']) == ('nccl' if rccl else 'gloo')
        assert int(rk['device']) == (k if rccl else 0)
    print('transport: %s, %d ranks' % ('nccl' if rccl else 'gloo', world))
    return res


def _ranks_against_the_global_batch(tmp_path, name, world, per_rank):
    steps = 2
    preset = case.PRESETS[name]
    p, x, y = case.case(world, per_rank)
    n = world * per_rank
    S = pr.sample_size(case.NCLS, case.RATE)
    assert S == 100 and S >= n
    shards = [set(y[r * per_rank:(r + 1) * per_rank]) for r in range(world)]
    assert shards[0] != shards[1] and 120 in shards[0] & shards[1]      # different classes, one of them in both
    res = _launch(tmp_path, 'dp', world, name, steps, p, x, y)
    for k, rk in enumerate(res):                               # replicas bit-identical after every step: every variable, the losses
        assert list(rk['compact']) == [True, True]
        for key in res[0].files:
            if key[:2] in ('w:', 'lo', 'ar', 'in'):
                np.testing.assert_array_equal(res[0][key], rk[key], err_msg='rank %d %s' % (k, key))
    slots = osn.zero_slots(p)
    ref_losses = []
    for t in range(steps):
        gap = case.arc_gap(p, x, y, preset[1])
        assert gap >= case.ARC_GAP, (t, gap)                   # the oracle's own cosines, away from the ArcFace threshold
        index = pr.sample(y, case.NCLS, S, case.SAMPLE_SEED, t)[0]
        for k, rk in enumerate(res):
            assert np.array_equal(rk['index:%d' % t], index), (t, k)
        kink = {c: np.concatenate([rk['z:%d:%s' % (t, c)] for rk in res]).astype(np.float64)
                for c in (key.split(':', 2)[2] for key in res[0].files if key.startswith('z:0:'))}
        p, slots, ls = pr.train_step(p, slots, x, y, 0.05, S, case.SAMPLE_SEED, t, *preset, kink=kink)
        ref_losses.append(ls)
    print('losses', res[0]['losses'].tolist(), 'ref', np.array(ref_losses).tolist())
    worst = max((np.sqrt(((res[0]['w:' + k].astype(np.float64) - p[k]) ** 2).sum()) / max(np.sqrt((p[k] * p[k]).sum()), 1e-30), k) for k in p)
    print('worst relative L2 %.3e (%s)' % worst)
    np.testing.assert_allclose(res[0]['losses'], np.array(ref_losses), rtol=2e-5)
    assert worst[0] <= 2e-5, worst


@pytest.mark.parametrize('name', ['SphereNet-ArcFace', 'SphereNet-CosFace'])
def test_two_ranks_one_sample_equal_the_global_batch_oracle(tmp_path, name):
    _ranks_against_the_global_batch(tmp_path, name, 2, 4)


def test_four_ranks_one_sample_equal_the_global_batch_oracle(tmp_path):
    _ranks_against_the_global_batch(tmp_path, 'SphereNet-CosFace', 4, 2)


# ------------------------------------------------------------------------------------------------ 3. one GPU
@pytest.mark.parametrize('opt', ['Momentum', 'Adam'])
def test_singular_compact_update_is_the_default_path_bit_for_bit(opt):
    p, x, y = case.case(1, 8)
    runs = []
    for compact in (False, True):
        net = net_select('SphereNet-ArcFace', 'NCHW', 5e-4)
        net.build(case.H, case.W, case.CH, case.NCLS, 'cuda')
        net.load_params(p)
        net.set_sample_rate(case.RATE, case.SAMPLE_SEED)
        net.compact_head_update = compact
        model = Singular(net, 0.05 if opt == 'Momentum' else 0.001, opt)
        step, losses, _, _ = model({'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': case.NCLS, 'num_examples': 8})
        assert net.compact_active() == compact and len(net.arena_groups()) == (2 if compact else 3)
        seen = []
        for t in range(3):
            step()
            seen.append(float(losses[0]))
        torch.cuda.synchronize()
        runs.append((seen, net.params.clone(), [s.clone() for s in model._opt.slots]))
    (la, pa, sa), (lb, pb, sb) = runs
    assert la == lb and torch.equal(pa, pb) and len(sa) == len(sb) == (1 if opt == 'Momentum' else 2)
    assert all(torch.equal(a, b) for a, b in zip(sa, sb))
    assert float(sa[0][net.cls_start:].abs().max()) > 0


def test_compact_step_launches_no_scatter(tmp_path):
    """the kernel trace of a compact Singular run: the fused update is there, k_scatter is not"""
    rocprof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    p, x, y = case.case(1, 8)
    fix = str(tmp_path / 'fix.npz')
    np.savez(fix, x=x, y=y, ncls=case.NCLS, rate=case.RATE, sample_seed=case.SAMPLE_SEED)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([rocprof, '--kernel-trace', '--output-format', 'csv', '-d', str(tmp_path / 'trace'), '-o', 'run', '--',
                        sys.executable, os.path.join(ROOT, 'tests', 'pfc_dp_worker.py'), 'single', fix, str(tmp_path / 'out'),
                        'SphereNet-ArcFace', '2'], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    files = glob.glob(str(tmp_path / 'trace' / '**' / '*kernel_trace.csv'), recursive=True)
    assert files, r.stdout[-2000:]
    text = ''.join(open(f).read() for f in files)
    assert text.count('k_momentum_cols') >= 2 and 'k_gather' in text
    assert 'k_scatter' not in text


# ------------------------------------------------------------------------------------------------ 5. refusals, CLI
def test_sync_sample_lifts_the_refusal():
    net = net_select('SphereNet-ArcFace', 'NCHW', 5e-4)
    net.set_sample_rate(0.1, 0)
    for wrapper in (DataParallel, DataParallel_margin):
        with pytest.raises(ValueError, match='one GPU only'):
            wrapper(net, 0.1, 'Momentum', num_gpus=2)
        with pytest.raises(ValueError, match='one GPU only'):
            wrapper(net, 0.1, 'Momentum', num_gpus=2, sync_sample=False)
        model = wrapper(net, 0.1, 'Momentum', num_gpus=2, sync_sample=True)
        assert model.sync_sample
    assert net.sample_comm is None and net.compact_head_update is False          # set when the wrapper is called, not before
    DataParallel_margin(net_select('SphereNet-ArcFace', 'NCHW', 5e-4), 0.1, 'Momentum', num_gpus=2, sync_sample=True)      # dense: no effect


def test_sample_smaller_than_the_global_batch_is_refused(tmp_path):
    p, x, y = case.case(2, 4)
    rate = 0.005                                               # S = 5: a rank's 4 rows fit, the global batch of 8 does not
    assert 4 <= sample_size(case.NCLS, rate) < 8
    res = _launch(tmp_path, 'refuse', 2, 'SphereNet-ArcFace', 0, p, x, y, rate=rate)
    for rk in res:
        msg = str(rk['error'])
        assert 'smaller than the batch of 8 rows' in msg and 'global batch' in msg and '2 ranks of 4 rows' in msg, msg


def _train(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='2')
    if torch.cuda.device_count() < 2:
        env['FTE_BENCH_SHARED_GPU'] = '1'
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--net_name', 'SphereNet-ArcFace', '--model_name', 'm',
                           '--synthetic', '1', '--synthetic_classes', '1000', '--input_height', '32', '--input_width', '32',
                           '--batch_size', '8', '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50',
                           '--display_interval', '1', '--save_interval', '1000', '--max_steps', '3'] + args,
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, cwd=cwd)


def test_train_cli(tmp_path):
    r = _train(['--num_gpus', '2', '--sample_rate', '0.1', '--sync_sample', '1'], str(tmp_path))
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.count('Loss #0: cross_entropy') == 3, r.stdout[-4000:]
    assert 'Sampled-class head: sample_rate = 0.1, sample_seed = 0, S = 100 of 1000 classes per step' in r.stdout
    assert 'Sampled-class head mode: one shared sample over 2 ranks, compact classifier update' in r.stdout
    r = _train(['--num_gpus', '2', '--sample_rate', '0.1'], str(tmp_path))
    assert r.returncode != 0 and 'one GPU only' in r.stdout and 'Loss #0' not in r.stdout
    r = _train(['--num_gpus', '1', '--sample_rate', '0.1', '--compact_head_update', '1', '--model_name', 'c'], str(tmp_path))
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'Sampled-class head mode: one GPU, compact classifier update' in r.stdout and r.stdout.count('Loss #0: cross_entropy') == 3
