"""Image packs on the host (tf_face_toolbox_amd/packs.py, pack_list.py, data.train_inputs / eval_inputs with packed_data_path): the
file format round-trips and refuses what is not a pack, pack_list.py stores the bytes the decode workers produce, and a loader fed
from a pack delivers the batches of the list the pack was made from, bit for bit.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 36


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def make_list(d, n=24, shape=(H, W), labels=True, gray=False, prefix='im'):
    """n PNGs of one shape under d and a list of them; label k % 5, except that class 4 gets ONE image (k == 4): the PxK sampler
    with num_per_class 2 drops it and keeps 0..3, and with the classes 1, 2, 3, 0 .. the renumbering has work to do"""
    from PIL import Image
    rng = np.random.default_rng(len(str(d)) + n)
    paths, labs = [], []
    for k in range(n):
        a = rng.integers(0, 256, shape + ((3,) if not gray else ()), dtype=np.uint8)
        p = os.path.join(str(d), '%s%03d.png' % (prefix, k))
        Image.fromarray(a).save(p)
        paths.append(p)
        labs.append(5 if k == 4 else (k % 4) + (1 if k % 4 >= 2 else 0))          # classes 0, 1, 3, 4 full; 5 has one image; 2 is empty
    lst = os.path.join(str(d), prefix + '_list.txt')
    with open(lst, 'w') as f:
        for p, lab in zip(paths, labs):
            f.write('%s %d\n' % (p, lab) if labels else p + '\n')
    return lst, paths, labs


def pack_cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'pack_list.py')] + [str(a) for a in args], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, cwd=ROOT)


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    """a colour list of 24 PNGs of 40 x 36 and its lossless pack, made once by the CLI (two decode processes)"""
    d = tmp_path_factory.mktemp('packed')
    lst, paths, labs = make_list(d)
    out = os.path.join(str(d), 'colour.fpk')
    r = pack_cli('--data_list_path', lst, '--out', out, '--is_color', 1, '--workers', 2)
    assert r.returncode == 0, r.stdout
    assert 'lossless' in r.stdout
    return {'list': lst, 'paths': paths, 'labels': labs, 'pack': out, 'dir': str(d)}


# ------------------------------------------------------------------ the file
@pytest.mark.parametrize('shape', [(112, 96, 3), (20, 18, 3), (20, 18, 1), (8, 8, 1)])
def test_round_trip(tmp_path, shape):
    """112 x 96 x 3 = 32256 and 8 x 8 x 1 = 64 are multiples of 64 already (no padding); 20 x 18 x 3 = 1080 -> 1088 and
    20 x 18 x 1 = 360 -> 384 are padded with zeros"""
    from tf_face_toolbox_amd import packs
    rng = np.random.default_rng(sum(shape))
    n = 5
    rows = rng.integers(1, 256, (n,) + shape, dtype=np.uint8)                      # no zero byte: the padding is told apart
    labels = [3, 0, 2, 2, 7]
    paths = ['a/b.jpg', 'c d.png', 'é/ü.jpg', 'x', 'y/z/w.jpeg']
    p = str(tmp_path / 'p.fpk')
    assert packs.write_pack(p, iter(rows), labels, paths) == (n,) + shape + (packs.row_stride_of(*shape),)
    assert not [f for f in os.listdir(str(tmp_path)) if f != 'p.fpk']              # the temporary name is gone
    pk = packs.ImagePack(p)
    size = shape[0] * shape[1] * shape[2]
    assert pk.shape == shape and pk.num_rows == n == len(pk) and pk.paths == paths
    assert pk.labels.dtype == np.int32 and pk.labels.tolist() == labels and pk.has_labels
    assert pk.row_stride % 64 == 0 and size <= pk.row_stride < size + 64
    assert pk.data_offset % 4096 == 0
    assert pk.rows.shape == (n, pk.row_stride) and pk.rows.dtype == np.uint8 and not pk.rows.flags.writeable
    assert np.array_equal(pk.rows[:, :size].reshape((n,) + shape), rows)
    assert not pk.rows[:, size:].any()
    for k in range(n):
        assert np.array_equal(pk.image(k), rows[k])
    assert os.path.getsize(p) == 4096 + n * pk.row_stride + 4 * n + len('\n'.join(paths).encode('utf-8'))
    # without labels: -1 everywhere
    packs.write_pack(p, rows, None, paths)
    pk = packs.ImagePack(p)
    assert pk.labels.tolist() == [-1] * n and not pk.has_labels


def test_reader_refusals(tmp_path):
    from tf_face_toolbox_amd import packs
    good = str(tmp_path / 'good.fpk')
    packs.write_pack(good, np.full((3, 20, 18, 3), 7, dtype=np.uint8), [0, 1, 2], ['a', 'b', 'c'])
    blob = open(good, 'rb').read()
    cases = {'magic': b'FTEPACX\0' + blob[8:], 'version': blob[:8] + (2).to_bytes(4, 'little') + blob[12:],
             'truncated': blob[:-1], 'trailing': blob + b'\0',
             'stride': blob[:32] + (1080).to_bytes(8, 'little') + blob[40:], 'empty': b''}
    for name, data in cases.items():
        bad = str(tmp_path / (name + '.fpk'))
        open(bad, 'wb').write(data)
        with pytest.raises(ValueError) as e:
            packs.ImagePack(bad)
        assert bad in str(e.value), (name, str(e.value))
    assert 'version' in str(pytest.raises(ValueError, packs.ImagePack, str(tmp_path / 'version.fpk')).value)
    assert 'multiple of 64' in str(pytest.raises(ValueError, packs.ImagePack, str(tmp_path / 'stride.fpk')).value)
    packs.ImagePack(good)


def test_writer_refuses_a_second_shape_and_leaves_nothing(tmp_path):
    from tf_face_toolbox_amd import packs
    p = str(tmp_path / 'p.fpk')
    imgs = [np.zeros((20, 18, 3), np.uint8), np.zeros((20, 18, 3), np.uint8), np.zeros((18, 20, 3), np.uint8)]
    with pytest.raises(ValueError) as e:
        packs.write_pack(p, imgs, None, ['one', 'two', 'three'])
    assert 'three' in str(e.value)
    assert os.listdir(str(tmp_path)) == []


# ------------------------------------------------------------------ pack_list.py
def test_pack_list_rows_are_the_workers_bytes(packed, tmp_path):
    from tf_face_toolbox_amd import packs, _decode_worker as dw
    pk = packs.ImagePack(packed['pack'])
    assert pk.shape == (H, W, 3) and pk.paths == packed['paths'] and pk.labels.tolist() == packed['labels']
    for k, p in enumerate(packed['paths']):
        assert np.array_equal(pk.image(k), dw._load(p, 3))
    # the same list read as gray, no labels column kept apart: a list of paths only
    lst, paths, _ = make_list(tmp_path, n=5, gray=True, labels=False, prefix='g')
    out = str(tmp_path / 'gray.fpk')
    r = pack_cli('--data_list_path', lst, '--out', out, '--is_color', 0, '--workers', 0)
    assert r.returncode == 0, r.stdout
    pk = packs.ImagePack(out)
    assert pk.shape == (H, W, 1) and pk.labels.tolist() == [-1] * 5
    for k, p in enumerate(paths):
        assert np.array_equal(pk.image(k), dw._load(p, 1))


def test_pack_list_with_landmarks_stores_the_aligned_crops(packed, tmp_path):
    import align
    from tf_face_toolbox_amd import packs
    from tf_face_toolbox_amd.preprocessing import ALIGN_TEMPLATE_112, read_landmarks
    lml = str(tmp_path / 'lm.txt')
    centred = (ALIGN_TEMPLATE_112 - 55.5) * (0.7 * W / 112.0)
    with open(lml, 'w') as f:
        for i, p in enumerate(packed['paths']):
            t = np.deg2rad((i * 7) % 41 - 20)
            pts = centred @ np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]]) + ((W - 1) / 2.0, (H - 1) / 2.0)
            f.write('%s %s\n' % (p, ' '.join('%.2f' % v for v in pts.reshape(-1))))
    out = str(tmp_path / 'aligned.fpk')
    r = pack_cli('--data_list_path', packed['list'], '--out', out, '--landmark_list_path', lml, '--input_height', 28, '--input_width', 24,
                 '--workers', 2)
    assert r.returncode == 0, r.stdout
    pk = packs.ImagePack(out)
    assert pk.shape == (28, 24, 3) and pk.labels.tolist() == packed['labels']
    lms = read_landmarks(lml, packed['paths'])
    for k, p in enumerate(packed['paths']):
        want = align.aligned_u8(p, lms[k], 3, 28, 24)
        assert want.any() and np.array_equal(pk.image(k), want)


def test_pack_list_mixed_shapes(packed, tmp_path):
    """two shapes: refused by the name of the first image that differs; with --resize_* the rows are the rounded resize"""
    from tf_face_toolbox_amd import packs, _decode_worker as dw
    _, other, _ = make_list(tmp_path, n=2, shape=(30, 44), prefix='o')
    lst = str(tmp_path / 'mixed.txt')
    paths = packed['paths'][:3] + other + packed['paths'][3:5]
    open(lst, 'w').write(''.join('%s %d\n' % (p, k) for k, p in enumerate(paths)))
    out = str(tmp_path / 'mixed.fpk')
    r = pack_cli('--data_list_path', lst, '--out', out, '--workers', 2)
    assert r.returncode != 0 and other[0] in r.stdout and other[1] not in r.stdout, r.stdout
    assert not os.path.exists(out) and not [f for f in os.listdir(str(tmp_path)) if '.fpk' in f]
    r = pack_cli('--data_list_path', lst, '--out', out, '--resize_height', 32, '--resize_width', 28, '--workers', 2)
    assert r.returncode == 0 and 'QUANTISED' in r.stdout, r.stdout
    pk = packs.ImagePack(out)
    assert pk.shape == (32, 28, 3) and pk.labels.tolist() == list(range(7))
    for k, p in enumerate(paths):
        x = dw.resize_window(dw._load(p, 3), 32, 28)
        assert np.array_equal(pk.image(k), np.rint(x.astype(np.float64) * 255.0).astype(np.uint8))
    assert 'quantis' in pack_cli('--help').stdout.lower()


# ------------------------------------------------------------------ the loader
def _three_batches(inp):
    try:
        out = []
        for _ in range(3):
            x = inp['images']()
            out.append((x.numpy().copy(), inp['labels']().numpy().copy()))
        return out
    finally:
        inp['close']()


def _assert_same_batches(a, b):
    assert len(a) == len(b) == 3
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xa.dtype == np.float32 and _same_bits(xa, xb) and _same_bits(ya, yb)
    assert not _same_bits(a[0][0], a[1][0])


@pytest.mark.parametrize('augmentation', [0, 1, 3])
@pytest.mark.parametrize('crop', [(-1, -1), (28, 24)])
@pytest.mark.parametrize('num_workers', [0, 2])
def test_train_batches_from_the_pack_equal_the_lists(packed, augmentation, crop, num_workers):
    from tf_face_toolbox_amd import data
    kw = dict(crop_height=crop[0], crop_width=crop[1], is_color=1, augmentation=augmentation, batch_size=8, device='cpu', seed=11,
              num_workers=num_workers)
    a = data.train_inputs(packed['list'], 32, 28, **kw)
    b = data.train_inputs(None, 32, 28, packed_data_path=packed['pack'], **kw)
    assert a['packed'] is None and b['packed'] == 'host'
    assert (a['num_examples'], a['num_classes'], a['batch_size']) == (b['num_examples'], b['num_classes'], b['batch_size'])
    _assert_same_batches(_three_batches(a), _three_batches(b))


@pytest.mark.parametrize('num_workers', [0, 2])
def test_pxk_sampler_from_the_pack(packed, num_workers):
    """batch_size -1: class 5 (one image) and the empty class 2 are dropped, the others renumbered 0..3"""
    from tf_face_toolbox_amd import data
    kw = dict(crop_height=28, crop_width=24, is_color=1, augmentation=1, batch_size=-1, num_classes=3, num_per_class=2, device='cpu',
              seed=3, num_workers=num_workers)
    a = data.train_inputs(packed['list'], 32, 28, **kw)
    b = data.train_inputs(None, 32, 28, packed_data_path=packed['pack'], **kw)
    assert a['num_classes'] == b['num_classes'] == 4 and a['num_examples'] == b['num_examples'] == 23
    ba, bb = _three_batches(a), _three_batches(b)
    _assert_same_batches(ba, bb)
    assert all(y.max() <= 3 for _, y in bb)


@pytest.mark.parametrize('rank', [0, 1])
def test_two_ranks_from_the_pack(packed, rank):
    from tf_face_toolbox_amd import data
    kw = dict(crop_height=28, crop_width=24, is_color=1, augmentation=0, batch_size=8, device='cpu', seed=5, num_workers=0, rank=rank,
              world_size=2)
    a = _three_batches(data.train_inputs(packed['list'], 32, 28, **kw))
    b = _three_batches(data.train_inputs(None, 32, 28, packed_data_path=packed['pack'], **kw))
    _assert_same_batches(a, b)
    assert a[0][0].shape == (4, 28, 24, 3)


@pytest.mark.parametrize('num_workers', [0, 2])
def test_eval_batches_from_the_pack_equal_the_lists(packed, num_workers):
    """24 images in batches of 10: the third batch wraps to the start of the list"""
    from tf_face_toolbox_amd import data
    na, ca = data.eval_inputs(packed['list'], 10, 1, 32, 28, device='cpu', num_workers=num_workers)
    nb, cb = data.eval_inputs(None, 10, 1, 32, 28, device='cpu', num_workers=num_workers, packed_data_path=packed['pack'])
    try:
        assert ca == cb == 24 and na.packed is None and nb.packed == 'host'
        got = [(na().numpy().copy(), nb().numpy().copy()) for _ in range(3)]
    finally:
        na.close(); nb.close()
    for xa, xb in got:
        assert xa.shape == (10, 32, 28, 3) and _same_bits(xa, xb)
    assert _same_bits(got[2][1][4:], got[0][1][:6])                                 # rows 20..23, then 0..5


def test_header_only_slots_carry_the_draws_of_a_full_slot(packed):
    """the resident mode's 64-byte slots: the header a full slot of the same seed gets, from the same code"""
    from tf_face_toolbox_amd import packs, _decode_worker as dw
    pk = packs.ImagePack(packed['pack'])
    for aug in (0, 1, 3):
        for seed in (1, 2, 3, 4):
            full = np.zeros(64 + pk.row_stride, np.uint8)
            file_slot = np.zeros(64 + pk.row_stride, np.uint8)
            head = np.full(64, 255, np.uint8)
            dw.raw_example(full, 7, 3, 44, 40, 40, 36, np.random.default_rng(seed), aug, pack=packed['pack'])
            dw.raw_example(head, 7, 3, 44, 40, 40, 36, np.random.default_rng(seed), aug, pack=pk, header_only=True)
            dw.raw_example(file_slot, packed['paths'][7], 3, 44, 40, 40, 36, np.random.default_rng(seed), aug)
            assert np.array_equal(full[:64], head) and np.array_equal(full, file_slot)
            assert full[:12].view(np.int32).tolist() == [0, H, W]
            assert np.array_equal(full[64:], pk.rows[7])
    with pytest.raises(ValueError):
        dw.raw_example(np.zeros(64, np.uint8), 24, 3, 44, 40, 40, 36, None, 0, pack=pk, header_only=True)


# ------------------------------------------------------------------ refusals
def test_loader_refusals(packed, tmp_path):
    from tf_face_toolbox_amd import data, packs
    with pytest.raises(ValueError, match='not both'):
        data.train_inputs(packed['list'], 32, 28, batch_size=8, device='cpu', packed_data_path=packed['pack'])
    with pytest.raises(ValueError, match='aligned when it is made'):
        data.train_inputs(None, 32, 28, batch_size=8, device='cpu', packed_data_path=packed['pack'], landmark_list_path=packed['list'])
    with pytest.raises(ValueError, match='aligned when it is made'):
        data.eval_inputs(None, 8, 1, 32, 28, device='cpu', packed_data_path=packed['pack'], landmark_list_path=packed['list'])
    with pytest.raises(ValueError, match='pack_on_gpu'):
        data.train_inputs(None, 32, 28, batch_size=8, device='cpu', packed_data_path=packed['pack'], pack_on_gpu=True)
    with pytest.raises(ValueError, match='pack_on_gpu'):
        data.eval_inputs(None, 8, 1, 32, 28, device='cpu', packed_data_path=packed['pack'], pack_on_gpu=True)
    with pytest.raises(ValueError, match='data_list_path or packed_data_path'):
        data.train_inputs(None, 32, 28, batch_size=8, device='cpu')
    with pytest.raises(ValueError, match='channel'):
        data.eval_inputs(None, 8, 0, 32, 28, device='cpu', packed_data_path=packed['pack'])
    bare = str(tmp_path / 'bare.fpk')
    packs.write_pack(bare, np.zeros((4, H, W, 3), np.uint8), None, list('abcd'))
    with pytest.raises(ValueError, match='no labels'):
        data.train_inputs(None, 32, 28, batch_size=4, device='cpu', packed_data_path=bare)
    nb, n = data.eval_inputs(None, 4, 1, 32, 28, device='cpu', num_workers=0, packed_data_path=bare)      # evaluation needs none
    try:
        assert n == 4 and nb().shape == (4, 32, 28, 3)
    finally:
        nb.close()


def test_cli_flag_refusals(packed, tmp_path):
    import evaluate
    import train
    from tf_face_toolbox_amd import packs
    base = ['--net_name', 'SphereNet', '--model_name', 'm', '--batch_size', '8', '--num_gpus', '1']

    def refused(argv, check=train.pack_flags_check, parser=train.build_parser, **kw):
        with pytest.raises(SystemExit) as e:
            check(parser().parse_args(argv), **kw)
        return str(e.value.code)
    pk = ['--packed_data_path', packed['pack']]
    assert 'train_list_path' in refused(base + pk + ['--train_list_path', packed['list']])
    assert 'synthetic' in refused(base + pk + ['--synthetic', '1'])
    assert 'aligned when it is made' in refused(base + pk + ['--landmark_list_path', packed['list']])
    assert 'packed_data_path' in refused(base + ['--pack_on_gpu', '1', '--train_list_path', packed['list']])
    bare = str(tmp_path / 'bare.fpk')
    packs.write_pack(bare, np.zeros((4, H, W, 3), np.uint8), None, list('abcd'))
    assert 'no labels' in refused(base + ['--packed_data_path', bare])
    assert str(tmp_path / 'none.fpk') in refused(base + ['--packed_data_path', str(tmp_path / 'none.fpk')])
    for ok in (base + pk, base + pk + ['--pack_on_gpu', '1'], base + ['--train_list_path', packed['list']]):
        FLAGS = train.build_parser().parse_args(ok)
        train.pack_flags_check(FLAGS)
        assert FLAGS.pack_on_gpu in (0, 1)
    ev = dict(parser=evaluate.build_parser, list_flag='data_list_path')
    assert 'data_list_path' in refused(pk + ['--data_list_path', packed['list']], **ev)
    assert 'aligned when it is made' in refused(pk + ['--landmark_list_path', packed['list']], **ev)
    train.pack_flags_check(evaluate.build_parser().parse_args(['--packed_data_path', bare, '--pack_on_gpu', '1']), 'data_list_path')
