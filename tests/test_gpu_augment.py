"""The loader's GPU transform with the colour augmentation (fte_preprocess_u8_aug, include/fte.h): decoded uint8 images + the
workers' seeded draws in, the float32 NHWC batch of train_inputs(..., augmentation=1) out -- BIT-EQUAL to the host transform
(tf_face_toolbox_amd/_decode_worker.py + preprocessing.py, themselves held to the per-pixel restatement tests/augment_ref.py
by tests/test_augment_host.py).  Mirrors tests/test_gpu_loader.py."""
import os

import numpy as np
import pytest

import augment_ref as ar

pytestmark = pytest.mark.gpu

IMG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'images')
NAMES = ['a.png', 'b.png', 'c.png', 'd.png', 'e.jpg', 'f.jpg', 'g.jpg', 'h.jpg']


def _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes, augmentation=1):
    from tf_face_toolbox_amd import _decode_worker as dw
    buf = np.zeros((len(seeds), nbytes), dtype=np.uint8)
    for i, seed in enumerate(seeds):
        dw.raw_example(buf[i], os.path.join(IMG, NAMES[i % len(NAMES)]), ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed),
                       augmentation)
    return buf


def _gpu(buf, ch, in_h, in_w, out_h, out_w, entry='fte_preprocess_u8_aug'):
    import torch
    from tf_face_toolbox_amd._lib import call
    raw = torch.from_numpy(buf).cuda()
    out = torch.empty((buf.shape[0], out_h, out_w, ch), dtype=torch.float32, device='cuda')
    call(entry, raw.data_ptr(), out.data_ptr(), buf.shape[0], buf.shape[1], ch, in_h, in_w, out_h, out_w,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('geom', ar.GEOMS)
def test_augmenting_transform_is_bit_equal_to_the_host(ch, geom):
    """resize + crop + flip + brightness / hue / saturation + normalise for the 64 seeded examples per geometry; slots large
    enough for every image, and slots that force the larger ones through the finished-crop path.  Flips and every flag bit (for
    colour: every combination) occur."""
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = geom
    out_h, out_w = (crop_h, crop_w) if crop_h != -1 else (in_h, in_w)
    seeds = ar.SEEDS
    want = np.stack([dw.train_example(os.path.join(IMG, NAMES[i % len(NAMES)]), ch, in_h, in_w, crop_h, crop_w, 1, np.random.default_rng(s))
                     for i, s in enumerate(seeds)])
    for side in (256, 64):
        nbytes = (dw.HEADER_BYTES + max(side * side * ch, out_h * out_w * ch * 4) + 63) // 64 * 64
        buf = _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes)
        hd = buf[:, :dw.HEADER_BYTES].view(np.int32)
        if side == 256:
            assert (hd[:, 0] == 0).all() and 0 < hd[:, 5].sum() < len(seeds)
            assert set(hd[:, 6].tolist()) == (set(range(8)) if ch == 3 else {0, 1})
        else:                                           # d.png, the largest image, is 250 x 250: finished by the worker when it does not fit
            assert (hd[:, 0] == 1).any() == (250 * 250 * ch > nbytes - dw.HEADER_BYTES)
        got = _gpu(buf, ch, in_h, in_w, out_h, out_w)
        bad = [s for i, s in enumerate(seeds) if not _same_bits(got[i], want[i])]
        assert not bad, 'slot side %d: seeds %s differ' % (side, bad)


@pytest.mark.parametrize('ch', [3, 1])
def test_edge_image_is_bit_equal_to_the_per_pixel_recipe(ch):
    """the hand-built edge image (black, white, gray, primaries, secondaries, equal maxima, values brightness pushes below 0)
    under hand-set headers: the 8 flag combinations x hue deltas at, just above and just below a pixel's hue (the floor-mod
    wrap to exactly 1.0)"""
    buf = ar.edge_slots(ch)
    s = ar.EDGE_SIDE
    got = _gpu(buf, ch, s, s, s, s)
    for i, slot in enumerate(buf):
        want = ar.restate_slot(slot, ch, s, s, s, s)
        assert _same_bits(got[i], want), ar.header(slot)
    assert got[1].min() < -1.0                       # brightness alone: negative values pass unclipped


@pytest.mark.parametrize('ch', [3, 1])
def test_no_flag_bits_is_the_plain_transform_and_the_plain_transform_ignores_the_draws(ch):
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = 120, 116, 112, 112
    nbytes = dw.HEADER_BYTES + 256 * 256 * ch
    seeds = ar.SEEDS[:16]
    buf = _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes)
    hd = buf[:, :dw.HEADER_BYTES].view(np.int32)
    assert hd[:, 6].any() and hd[:, 7:(10 if ch == 3 else 8)].all()
    plain = _gpu(buf, ch, in_h, in_w, crop_h, crop_w, 'fte_preprocess_u8')          # words 6..9 set: the old entry ignores them
    zeroed = buf.copy()
    zeroed[:, :dw.HEADER_BYTES].view(np.int32)[:, 6:10] = 0
    assert _same_bits(plain, _gpu(zeroed, ch, in_h, in_w, crop_h, crop_w, 'fte_preprocess_u8'))
    noflags = buf.copy()
    noflags[:, :dw.HEADER_BYTES].view(np.int32)[:, 6] = 0                            # draws present, none applied
    assert _same_bits(plain, _gpu(noflags, ch, in_h, in_w, crop_h, crop_w))
    assert _same_bits(plain, _gpu(zeroed, ch, in_h, in_w, crop_h, crop_w))
    assert not _same_bits(plain, _gpu(buf, ch, in_h, in_w, crop_h, crop_w))


def test_bad_arguments_are_refused():
    import torch
    from tf_face_toolbox_amd._lib import query
    x = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    o = torch.zeros(4096, dtype=torch.float32, device='cuda')
    for args in [(1, 100, 3, 8, 8, 8, 8), (1, 4096, 2, 8, 8, 8, 8), (1, 4096, 3, 8, 8, 9, 8), (0, 4096, 3, 8, 8, 8, 8)]:
        assert query('fte_preprocess_u8_aug', x.data_ptr(), o.data_ptr(), *args, 0) != 0


def test_train_inputs_with_augmentation_on_the_gpu_equal_the_host_pipeline(tmp_path, monkeypatch):
    """train_inputs(augmentation=1) end to end on the GPU box: worker processes + raw slots + fte_preprocess_u8_aug deliver the
    batches the all-host pipeline delivers for the same seed, labels included."""
    from tf_face_toolbox_amd import data
    lst = tmp_path / 'list.txt'
    lst.write_text(''.join('%s %d\n' % (os.path.join(IMG, n), i % 4) for i, n in enumerate(NAMES * 4)))
    monkeypatch.setenv('FTE_LOADER_GPU', '0')
    a = data.train_inputs(str(lst), 120, 116, 112, 112, is_color=1, augmentation=1, batch_size=16, device='cuda', seed=5, num_workers=3)
    monkeypatch.setenv('FTE_LOADER_GPU', '1')
    b = data.train_inputs(str(lst), 120, 116, 112, 112, is_color=1, augmentation=1, batch_size=16, device='cuda', seed=5, num_workers=3)
    try:
        assert not a['gpu_transform'] and b['gpu_transform']
        for _ in range(6):
            xa, xb = a['images'](), b['images']()
            assert xb.shape == (16, 112, 112, 3) and xb.dtype == xa.dtype
            assert np.array_equal(xa.cpu().numpy().view(np.uint32), xb.cpu().numpy().view(np.uint32))
            assert np.array_equal(a['labels']().cpu().numpy(), b['labels']().cpu().numpy())
    finally:
        a['close'](); b['close']()
