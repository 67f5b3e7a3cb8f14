"""CPU: the host surface of the sampled-class head under data parallelism -- train.py's flags and its unchanged
refusal, the shared sample of a union of shards, the fixed case of the GPU test against the ArcFace threshold (oracle alone), and
the new symbols in fte.h, the ctypes table and INTEGRATION.md."""
import os
import re

import numpy as np
import pytest

import partial_fc_ref as pr
import pfc_dp_case as case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('fte_pfc_momentum_update_cols', 'fte_pfc_adam_update_cols')


def test_flags():
    import train as cli
    base = ['--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--batch_size', '8', '--max_epoches', '1']
    F = cli.build_parser().parse_args(base)
    assert F.sync_sample == 0 and F.compact_head_update == 0
    two = base + ['--num_gpus', '2', '--sample_rate', '0.1']
    with pytest.raises(SystemExit) as e:
        cli.sample_flags_check(cli.build_parser().parse_args(two))
    assert str(e.value) == '--sample_rate 0.1: the sampled-class head runs on one GPU only (--num_gpus 2)'      # the text as it was
    F = cli.build_parser().parse_args(two + ['--sync_sample', '1'])
    assert F.sync_sample == 1
    cli.sample_flags_check(F)
    cli.sample_flags_check(cli.build_parser().parse_args(base + ['--num_gpus', '1', '--sample_rate', '0.1', '--compact_head_update', '1']))
    with pytest.raises(SystemExit, match='only SphereNet-ArcFace'):                # the other refusals do not move
        cli.sample_flags_check(cli.build_parser().parse_args(['--net_name', 'SphereNet', '--model_name', 'm', '--num_gpus', '2',
                                                              '--sample_rate', '0.1', '--sync_sample', '1']))
    help_text = cli.build_parser().format_help()
    assert '--sync_sample' in help_text and '--compact_head_update' in help_text


def test_wrapper_refusal_text_is_unchanged():
    from tf_face_toolbox_amd import net_select, DataParallel, DataParallel_margin
    net = net_select('SphereNet-ArcFace')
    net.set_sample_rate(0.1, 0)
    for wrapper in (DataParallel, DataParallel_margin):
        with pytest.raises(ValueError) as e:
            wrapper(net, 0.1, 'Momentum', num_gpus=2)
        assert str(e.value) == 'a sampled-class head (sample_rate 0.1) runs on one GPU only: num_gpus = 2'
        assert wrapper(net, 0.1, 'Momentum', num_gpus=2, sync_sample=True).sync_sample is True
    assert net.sample_comm is None and net.compact_head_update is False and not net.compact_active()
    net.compact_head_update = True
    assert net.compact_active()
    net.set_sample_rate(1.0)
    assert not net.compact_active()                            # the dense head ignores the switch


def test_sample_of_the_union_holds_every_shards_classes():
    C, S, world, n = 20000, 2000, 4, 64
    rng = np.random.default_rng(3)
    for t in range(20):
        shards = [rng.integers(0, C, n) for _ in range(world)]
        index, inverse, ys = pr.sample(np.concatenate(shards), C, S, 7, t)
        for r, y in enumerate(shards):
            assert np.isin(y, index).all()
            assert (index[ys[r * n:(r + 1) * n]] == y).all()  # a rank's rows of labels_out are its own remapped labels
        own = pr.sample(shards[0], C, S, 7, t)[0]
        assert not np.array_equal(own, index)                  # per-rank samples would differ: why the labels are gathered


def test_compact_buckets_and_groups():
    from tf_face_toolbox_amd import net_select
    net = net_select('SphereNet-ArcFace')
    net.build(32, 32, 3, 1000, 'cpu')
    dense_groups, dense_buckets = net.arena_groups(), net.grad_buckets()
    net.set_sample_rate(0.1, 0)
    assert net.arena_groups() == dense_groups and net.grad_buckets() == dense_buckets      # the default: nothing moves
    net.compact_head_update = True
    assert net.arena_groups() == dense_groups[:2]
    buckets = net.grad_buckets()
    assert buckets[0] == (net.fc_start, net.cls_start) and buckets[1:] == dense_buckets[1:]
    covered = sorted(buckets)
    assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][1] == net.cls_start


@pytest.mark.parametrize('name', sorted(case.PRESETS))
@pytest.mark.parametrize('world,per_rank', [(2, 4), (4, 2)])
def test_the_gpu_case_is_away_from_the_arcface_threshold(name, world, per_rank):
    """from the oracle alone, before any GPU run: the initial target cosines of the fixed case lie far from cos(pi - m)"""
    p, x, y = case.case(world, per_rank)
    gap = case.arc_gap(p, x, y, case.PRESETS[name][1])
    assert gap >= case.ARC_GAP, gap
    shards = [set(y[r * per_rank:(r + 1) * per_rank]) for r in range(world)]
    assert 120 in shards[0] & shards[1] and shards[0] != shards[1]
    assert pr.sample_size(case.NCLS, case.RATE) >= world * per_rank


def test_symbols_are_declared_and_bound():
    from tf_face_toolbox_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fte.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in doc, name
