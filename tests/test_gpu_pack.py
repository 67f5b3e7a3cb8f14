"""-m gpu: image packs on the device.  fte_pack_gather_slots (include/fte.h) against a torch index-gather, byte for byte, with
guarded outputs, untrusted indices, every refusal and a pack beyond 4 GiB; the host-pack and resident-pack loaders against the
list loader, bit for bit; train.py / evaluate.py from a pack against the same run from the list."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FILL = 0xA5
GUARD = 4096


def _gather(rows, num_rows, row_stride, index, headers, out, n, slot_stride):
    from tf_face_toolbox_amd._lib import query
    r = query('fte_pack_gather_slots', rows.data_ptr(), num_rows, row_stride, index.data_ptr(), headers.data_ptr(), out.data_ptr(), n,
              slot_stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return r


def _check(row_stride, n, num_rows, extra, index):
    g = torch.Generator().manual_seed(row_stride + n)
    rows = torch.randint(0, 256, (num_rows, row_stride), dtype=torch.uint8, generator=g).cuda()
    headers = torch.randint(0, 256, (n, 64), dtype=torch.uint8, generator=g).cuda()
    index = torch.tensor(index, dtype=torch.int64).cuda()
    assert index.numel() == n
    slot_stride = 64 + row_stride + extra
    out = torch.full((n * slot_stride + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    assert _gather(rows, num_rows, row_stride, index, headers, out, n, slot_stride) == 0
    want = torch.full((n, slot_stride), FILL, dtype=torch.uint8, device='cuda')
    want[:, :64] = headers
    want[:, 64:64 + row_stride] = rows[index.clamp(0, num_rows - 1)]                # the torch index-gather
    got = out[:n * slot_stride].view(n, slot_stride)
    assert torch.equal(got[:, :64], headers)
    assert torch.equal(got, want)                                                   # rows right, slot tails untouched
    assert bool((out[n * slot_stride:] == FILL).all())                              # guard untouched
    again = torch.full_like(out, FILL)
    assert _gather(rows, num_rows, row_stride, index, headers, again, n, slot_stride) == 0
    assert torch.equal(again, out)


@pytest.mark.parametrize('extra', [0, 64])
@pytest.mark.parametrize('row_stride,n', [(64, 1), (1088, 5), (32256, 130), (187520, 3)])
def test_gather_equals_an_index_gather(row_stride, n, extra):
    """64: one 16-byte chunk of row per lane of the first wave only; 1088: 72 chunks, a partly filled block; 32256 (112 x 96 x 3):
    8 blocks per slot and 130 images, more than the grid's rows hold at once on a small device cap, with repeats, the first and
    the last row; 187520 (250 x 250 x 3 padded): 46 blocks per slot.  Out-of-range indices read the first / the last row."""
    num_rows = {64: 3, 1088: 9, 32256: 40, 187520: 4}[row_stride]
    rng = np.random.default_rng(n)
    index = rng.integers(0, num_rows, n).tolist()
    if n >= 3:
        index[0], index[1], index[2] = 0, num_rows - 1, num_rows - 1
    if n >= 5:
        index[3], index[4] = -1, num_rows
    if n >= 130:
        index[100:110] = [7] * 10
        index[129] = -(2 ** 40)
        index[128] = 2 ** 40
    _check(row_stride, n, num_rows, extra, index)


def test_untrusted_indices_are_clamped():
    _check(1088, 4, 6, 0, [-1, 6, -(2 ** 62), 2 ** 62])


def test_refusals_leave_the_output_untouched():
    rs, n, nr = 1088, 3, 4
    rows = torch.zeros((nr, rs), dtype=torch.uint8, device='cuda')
    headers = torch.zeros((n, 64), dtype=torch.uint8, device='cuda')
    index = torch.zeros(n, dtype=torch.int64, device='cuda')
    ss = 64 + rs
    out = torch.full((n * (ss + 64) + GUARD,), FILL, dtype=torch.uint8, device='cuda')

    class Null(object):
        @staticmethod
        def data_ptr():
            return None
    ok = dict(rows=rows, num_rows=nr, row_stride=rs, index=index, headers=headers, out=out, n=n, slot_stride=ss)
    bad = [dict(rows=Null), dict(index=Null), dict(headers=Null), dict(out=Null), dict(n=0), dict(n=-1), dict(num_rows=0),
           dict(row_stride=0), dict(row_stride=32), dict(row_stride=1024 + 32), dict(slot_stride=ss + 32), dict(slot_stride=ss - 64),
           dict(slot_stride=rs), dict(slot_stride=0)]
    for case in bad:
        assert _gather(**dict(ok, **case)) == EINVAL, case
        assert bool((out == FILL).all()), case
    assert _gather(**ok) == 0 and not bool((out[:ss] == FILL).all())


def test_offsets_are_64_bit():
    """1,200,000 rows of 4096 bytes = 4.9 GB, uninitialised; row 1,048,576 starts at byte 2^32 exactly"""
    rs, nr = 4096, 1200000
    free, _ = torch.cuda.mem_get_info()
    assert free > rs * nr + (1 << 30), 'this test needs 6 GB of free device memory'
    rows = torch.empty(rs * nr, dtype=torch.uint8, device='cuda')
    picks = [0, 1048576, nr - 1]
    g = torch.Generator().manual_seed(1)
    known = torch.randint(0, 256, (3, rs), dtype=torch.uint8, generator=g).cuda()
    for k, r in enumerate(picks):
        rows[r * rs:(r + 1) * rs] = known[k]
    headers = torch.randint(0, 256, (3, 64), dtype=torch.uint8, generator=g).cuda()
    out = torch.full((3 * (64 + rs) + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    assert _gather(rows, nr, rs, torch.tensor(picks, dtype=torch.int64).cuda(), headers, out, 3, 64 + rs) == 0
    got = out[:3 * (64 + rs)].view(3, 64 + rs)
    assert torch.equal(got[:, 64:], known) and torch.equal(got[:, :64], headers)
    assert bool((out[3 * (64 + rs):] == FILL).all())
    del rows
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the loaders
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """64 PNGs of 40 x 36 in 8 classes, their list and their lossless pack"""
    from PIL import Image
    from tf_face_toolbox_amd import packs, _decode_worker as dw
    d = tmp_path_factory.mktemp('gpu_pack')
    rng = np.random.default_rng(2)
    paths, labels = [], []
    for k in range(64):
        p = str(d / ('im%02d.png' % k))
        Image.fromarray(rng.integers(0, 256, (40, 36, 3), dtype=np.uint8)).save(p)
        paths.append(p)
        labels.append(k % 8)
    lst = str(d / 'list.txt')
    open(lst, 'w').write(''.join('%s %d\n' % (p, lab) for p, lab in zip(paths, labels)))
    pack = str(d / 'set.fpk')
    packs.write_pack(pack, (dw._load(p, 3) for p in paths), labels, paths)
    return {'list': lst, 'pack': pack, 'dir': str(d)}


def _two_batches(inp):
    try:
        out = []
        for _ in range(2):
            x = inp['images']()
            out.append((x.cpu().numpy(), inp['labels']().cpu().numpy()))
        return out
    finally:
        inp['close']()


@pytest.mark.parametrize('augmentation', [0, 1, 3])
def test_pack_loaders_equal_the_list_loader(dataset, augmentation):
    from tf_face_toolbox_amd import data
    kw = dict(crop_height=28, crop_width=24, is_color=1, augmentation=augmentation, batch_size=16, device='cuda', seed=9, num_workers=2)
    a = data.train_inputs(dataset['list'], 32, 28, **kw)
    assert a['gpu_transform'] and a['packed'] is None
    want = _two_batches(a)
    for on_gpu in (False, True):
        b = data.train_inputs(None, 32, 28, packed_data_path=dataset['pack'], pack_on_gpu=on_gpu, **kw)
        assert b['gpu_transform'] and b['packed'] == ('gpu' if on_gpu else 'host')
        got = _two_batches(b)
        for (xa, ya), (xb, yb) in zip(want, got):
            assert xb.shape == (16, 28, 24, 3) and xb.dtype == np.float32
            assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32)), on_gpu
            assert np.array_equal(ya, yb)
    assert not np.array_equal(want[0][0], want[1][0])


def test_resident_pack_without_workers_equals_the_list_loader(dataset):
    """num_workers 0: the headers are written by the loader's own process"""
    from tf_face_toolbox_amd import data
    kw = dict(crop_height=28, crop_width=24, is_color=1, augmentation=1, batch_size=16, device='cuda', seed=4)
    want = _two_batches(data.train_inputs(dataset['list'], 32, 28, num_workers=2, **kw))
    got = _two_batches(data.train_inputs(None, 32, 28, num_workers=0, packed_data_path=dataset['pack'], pack_on_gpu=True, **kw))
    for (xa, ya), (xb, yb) in zip(want, got):
        assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32)) and np.array_equal(ya, yb)


def test_resident_eval_equals_the_lists_and_starts_no_worker(dataset, monkeypatch):
    """64 images in batches of 24: the third batch wraps"""
    from tf_face_toolbox_amd import data
    na, ca = data.eval_inputs(dataset['list'], 24, 1, 32, 28, device='cuda', num_workers=2)
    try:
        want = [na().cpu().numpy() for _ in range(3)]
    finally:
        na.close()
    started = []
    real = subprocess.Popen

    def counting(*a, **kw):
        started.append(a)
        return real(*a, **kw)
    monkeypatch.setattr(subprocess, 'Popen', counting)
    monkeypatch.setattr(data, '_WorkerPool', lambda *a, **kw: started.append(a))
    nb, cb = data.eval_inputs(None, 24, 1, 32, 28, device='cuda', num_workers=2, packed_data_path=dataset['pack'], pack_on_gpu=True)
    try:
        got = [nb().cpu().numpy() for _ in range(3)]
    finally:
        assert nb.close()
    assert ca == cb == 64 and nb.packed == 'gpu' and not started
    for xa, xb in zip(want, got):
        assert xb.shape == (24, 32, 28, 3) and np.array_equal(xa.view(np.uint32), xb.view(np.uint32))


def test_a_pack_larger_than_free_memory_is_refused(dataset, monkeypatch):
    from tf_face_toolbox_amd import data, packs
    need = packs.ImagePack(dataset['pack']).row_stride * 64
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (12345, 67890))
    before = torch.cuda.memory_allocated()
    for build in (lambda: data.train_inputs(None, 32, 28, batch_size=16, device='cuda', num_workers=0, packed_data_path=dataset['pack'],
                                            pack_on_gpu=True),
                  lambda: data.eval_inputs(None, 16, 1, 32, 28, device='cuda', packed_data_path=dataset['pack'], pack_on_gpu=True)):
        with pytest.raises(ValueError) as e:
            build()
        assert str(need) in str(e.value) and '12345' in str(e.value)
    assert torch.cuda.memory_allocated() <= before + (1 << 20)


# ------------------------------------------------------------------ the CLIs
def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, FTE_LOADER_WORKERS='2')
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _train(dataset, name, source):
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', 'SphereNet', '--model_name', name, '--input_height', '32', '--input_width', '28',
                '--crop_height', '28', '--crop_width', '24', '--batch_size', '16', '--num_gpus', '1', '--init_lr', '0.01', '--lr_decay_epoch', '2',
                '--max_epoches', '50', '--display_interval', '1', '--save_interval', '1000', '--augmentation', '1', '--max_steps', '4'] + source,
               dataset['dir'])
    assert '64 images loaded, totally 8 classes' in out
    ck = torch.load(os.path.join(dataset['dir'], 'models', 'SphereNet_' + name, 'SphereNet_%s.ckpt-4' % name), map_location='cpu')
    return out, ck['variables']


@pytest.fixture(scope='module')
def trained_from_the_list(dataset):
    return _train(dataset, 'list', ['--train_list_path', dataset['list']])[1]


@pytest.mark.parametrize('on_gpu', [0, 1])
def test_train_from_the_pack_saves_the_lists_checkpoint(dataset, trained_from_the_list, on_gpu):
    out, got = _train(dataset, 'pack%d' % on_gpu, ['--packed_data_path', dataset['pack'], '--pack_on_gpu', str(on_gpu)])
    assert 'image pack %s' % dataset['pack'] in out and '40 x 36 x 3' in out
    assert ('resident in device memory' in out) == bool(on_gpu)
    assert sorted(got) == sorted(trained_from_the_list)
    for k, v in trained_from_the_list.items():
        assert torch.equal(v, got[k]), k


@pytest.mark.parametrize('on_gpu', [0, 1])
def test_evaluate_from_the_pack_extracts_the_lists_features(dataset, trained_from_the_list, on_gpu):
    from scipy.io import loadmat
    common = [os.path.join(ROOT, 'evaluate.py'), '--net_name', 'SphereNet', '--model_name', 'list', '--input_height', '32', '--input_width', '28',
              '--batch_size', '24']
    want_path = os.path.join(dataset['dir'], 'features', 'SphereNet_list', 'a_4.mat')
    if not os.path.exists(want_path):
        _run(common + ['--fea_name', 'a', '--data_list_path', dataset['list']], dataset['dir'])
    out = _run(common + ['--fea_name', 'b%d' % on_gpu, '--packed_data_path', dataset['pack'], '--pack_on_gpu', str(on_gpu)], dataset['dir'])
    assert 'Totally extracted 64 features.' in out
    a = loadmat(want_path)['wfea']
    b = loadmat(os.path.join(dataset['dir'], 'features', 'SphereNet_list', 'b%d_4.mat' % on_gpu))['wfea']
    assert a.shape == (64, 512) and np.abs(a).max() > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
