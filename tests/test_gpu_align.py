"""The loader's GPU transform with five-point alignment (fte_preprocess_u8_align, include/fte.h): a window of the decoded image, the
worker's draws and the inverse similarity in, the float32 NHWC batch out -- BIT-EQUAL to the host aligned transform
(tf_face_toolbox_amd/preprocessing.py: align_warp, apply_augmentation; held to independent restatements by
tests/test_align_host.py).  Hand-built slots first, then the loader end to end.  Mirrors tests/test_gpu_augment.py."""
import numpy as np
import pytest

import align_ref as ar

pytestmark = pytest.mark.gpu

IN_H, IN_W = 112, 96
HEADER = 128
COLOUR = (0.07, 0.13, 0.8)                       # brightness delta, hue delta, saturation factor


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _slot_bytes(ch, wh, ww, out_h, out_w):
    return (HEADER + max(wh * ww * ch, out_h * out_w * ch * 4) + 63) // 64 * 64


def _slot(nbytes, window, m6, y0=0, x0=0, flip=0, flags=0, colour=(0.0, 0.0, 0.0)):
    slot = np.zeros(nbytes, dtype=np.uint8)
    hd = slot[:HEADER].view(np.int32)
    hd[:7] = (0, window.shape[0], window.shape[1], y0, x0, flip, flags)
    hd[7:10].view(np.float32)[:] = colour
    hd[16:22].view(np.float32)[:] = m6
    slot[HEADER:HEADER + window.size] = window.reshape(-1)
    return slot


def _host(slot, ch, out_h, out_w):
    """the host aligned transform of one mode-0 slot, from the slot's own words"""
    from tf_face_toolbox_amd import preprocessing as pp
    hd = slot[:HEADER].view(np.int32)
    _, wh, ww, y0, x0, flip, flags = hd[:7].tolist()
    window = slot[HEADER:HEADER + wh * ww * ch].reshape(wh, ww, ch).astype(np.float32) * np.float32(1.0 / 255.0)
    image = pp.align_warp(window, hd[16:22].view(np.float32), IN_H, IN_W, y0, out_h, x0, out_w)
    image = pp.apply_augmentation(image, flip, flags, *hd[7:10].view(np.float32))
    return (image - np.float32(0.5)) / np.float32(0.5)


def _gpu(buf, ch, out_h, out_w, in_h=IN_H, in_w=IN_W):
    import torch
    from tf_face_toolbox_amd._lib import call
    raw = torch.from_numpy(buf).cuda()
    out = torch.empty((buf.shape[0], out_h, out_w, ch), dtype=torch.float32, device='cuda')
    call('fte_preprocess_u8_align', raw.data_ptr(), out.data_ptr(), buf.shape[0], buf.shape[1], ch, in_h, in_w, out_h, out_w,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _matrices(wh, ww):
    """inverse similarities (and two plain affine maps: the kernel takes any six numbers) from the 112 x 96 aligned image into a
    wh x ww window: name -> (a0, a1, a2, b0, b1, b2)"""
    f = ww / float(IN_W)
    c, s = np.cos(np.deg2rad(30.0)) * f, np.sin(np.deg2rad(30.0)) * f
    cx, cy = (IN_W - 1) / 2.0, (IN_H - 1) / 2.0
    return {
        'identity': (1, 0, 0, 0, 1, 0),
        'rotation 30': (c, -s, (ww - 1) / 2.0 - (c * cx - s * cy), s, c, (wh - 1) / 2.0 - (s * cx + c * cy)),
        'scale 0.5': (0.5, 0, 0.25, 0, 0.5, 0.25),
        'scale 2.3': (2.3, 0, -3.7, 0, 2.3, -1.2),
        'half outside': (f, 0, -0.5 * ww, 0, wh / float(IN_H), 0.3),
        'all outside': (1, 0, 1e4, 0, 1, 1e4),
    }


OUTPUTS = {'full': (IN_H, IN_W, 0, 0), 'crop at (12, 8)': (100, 88, 12, 8), 'crop at (0, 0)': (100, 88, 0, 0)}


@pytest.mark.parametrize('output', sorted(OUTPUTS))
@pytest.mark.parametrize('window', [(1, 1), (37, 29), (250, 250)])
@pytest.mark.parametrize('ch', [3, 1])
def test_aligning_transform_is_bit_equal_to_the_host(ch, window, output):
    """one launch of 24 slots: the six matrices x flip 0 / 1 x colour flags 0 / all three bits (gray ignores hue and
    saturation).  100 x 88 = 34.4 blocks of 256 pixels: the last block of every image is partly filled."""
    wh, ww = window
    out_h, out_w, y0, x0 = OUTPUTS[output]
    rng = np.random.default_rng(wh * 1000 + ww + ch)
    nbytes = _slot_bytes(ch, wh, ww, out_h, out_w)
    names, slots = [], []
    for name, m6 in sorted(_matrices(wh, ww).items()):
        for flip in (0, 1):
            for flags in (0, 7):
                names.append((name, flip, flags))
                slots.append(_slot(nbytes, rng.integers(0, 256, (wh, ww, ch), dtype=np.uint8), m6, y0, x0, flip, flags,
                                   COLOUR if flags else (0.0, 0.0, 0.0)))
    buf = np.stack(slots)
    got = _gpu(buf, ch, out_h, out_w)
    assert np.isfinite(got).all()
    for i, name in enumerate(names):
        want = _host(buf[i], ch, out_h, out_w)
        assert _same_bits(got[i], want), name
        if name[0] == 'all outside' and name[2] == 0:
            assert (got[i] == -1.0).all()
        if name[0] == 'half outside' and name[2] == 0 and output == 'full' and window == (250, 250):      # zero fill left, image right
            left = got[i][:, IN_W // 2 + 2:] if name[1] else got[i][:, :IN_W // 2 - 2]
            assert (left == -1.0).all() and (got[i] != -1.0).any()
    if window != (1, 1):
        assert len({got[i].tobytes() for i in range(len(names))}) >= 20                  # the slots really differ


@pytest.mark.parametrize('n', [1, 5])
def test_batch_sizes(n):
    rng = np.random.default_rng(n)
    nbytes = _slot_bytes(3, 37, 29, 100, 88)
    m = _matrices(37, 29)
    buf = np.stack([_slot(nbytes, rng.integers(0, 256, (37, 29, 3), dtype=np.uint8), m[k], 3 + i, 2 * i, i & 1, 7 * (i & 1), COLOUR)
                    for i, k in enumerate(['rotation 30', 'scale 0.5', 'half outside', 'identity', 'rotation 30'][:n])])
    got = _gpu(buf, 3, 100, 88)
    for i in range(n):
        assert _same_bits(got[i], _host(buf[i], 3, 100, 88)), i


@pytest.mark.parametrize('ch', [3, 1])
def test_finished_slots_are_copied(ch):
    """mode 1: the float32 crop behind the 128-byte header, bit for bit, whatever the other words say; next to a mode-0 slot"""
    rng = np.random.default_rng(8)
    nbytes = _slot_bytes(ch, 37, 29, 100, 88)
    done = np.zeros(nbytes, dtype=np.uint8)
    crop = rng.standard_normal((100, 88, ch)).astype(np.float32)
    done[HEADER:HEADER + crop.size * 4] = crop.reshape(-1).view(np.uint8)
    hd = done[:HEADER].view(np.int32)
    hd[:7] = (1, 100, 88, 5, 6, 1, 7)
    hd[16:22].view(np.float32)[:] = np.nan
    raw = _slot(nbytes, rng.integers(0, 256, (37, 29, ch), dtype=np.uint8), _matrices(37, 29)['rotation 30'], 1, 2, 1)
    got = _gpu(np.stack([done, raw, done]), ch, 100, 88)
    assert _same_bits(got[0], crop) and _same_bits(got[2], crop) and _same_bits(got[1], _host(raw, ch, 100, 88))


UNTRUSTED = {
    'NaN in m6': dict(m6=(np.nan, 0, 0, 0, 1, 0)),
    'NaN translation': dict(m6=(1, 0, 0, 0, 1, np.nan)),
    '+inf in m6': dict(m6=(1, 0, np.inf, 0, 1, 0)),
    '+inf factor': dict(m6=(np.inf, 0, 0, 0, 1, 0)),
    'translation 1e9': dict(m6=(1, 0, 1e9, 0, 1, 1e9)),
    'translation -1e9': dict(m6=(1, 0, -1e9, 0, 1, 2.0)),
    'window larger than the slot': dict(h0=30000, w0=30000),
    'window of 2^31 - 1 squared': dict(h0=2 ** 31 - 1, w0=2 ** 31 - 1),
    'one row too many': dict(grow=1),
    'h0 = 0': dict(h0=0),
    'w0 = -5': dict(w0=-5),
}


@pytest.mark.parametrize('what', sorted(UNTRUSTED))
@pytest.mark.parametrize('ch', [3, 1])
def test_untrusted_words_read_zeros(ch, what):
    """words 16..21 and h0 / w0 steer addresses: a NaN, an infinity, a coordinate far outside or a window that does not fit the
    slot reads the zero fill -- the host rule -- whatever bytes the slot holds: -1.0 everywhere after the normalisation"""
    case = UNTRUSTED[what]
    wh, ww = 37, 29
    nbytes = _slot_bytes(ch, wh, ww, IN_H, IN_W)
    slot = _slot(nbytes, np.full((wh, ww, ch), 200, dtype=np.uint8), case.get('m6', (0.3, 0, 0, 0, 0.3, 0)))
    slot[HEADER + wh * ww * ch:] = 200
    hd = slot[:HEADER].view(np.int32)
    if case.get('grow'):                             # the largest window that fits, then one more row: h0 * w0 * ch > stride - 128
        hd[1:3] = ((nbytes - HEADER) // (ch * ww), ww)
        assert (_gpu(slot[None], ch, IN_H, IN_W) != -1.0).any()
        hd[1] += 1
    hd[1] = case.get('h0', hd[1])
    hd[2] = case.get('w0', hd[2])
    got = _gpu(slot[None], ch, IN_H, IN_W)
    assert (got == -1.0).all()
    if 'm6' in case:                                 # the host definition says the same
        assert _same_bits(got[0], _host(slot, ch, IN_H, IN_W))


def test_bad_arguments_are_refused():
    import torch
    from tf_face_toolbox_amd._lib import query
    x = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    o = torch.zeros(4096, dtype=torch.float32, device='cuda')
    for args in [(1, 100, 3, 8, 8, 8, 8), (1, 64, 3, 8, 8, 8, 8), (1, 4096, 2, 8, 8, 8, 8), (1, 4096, 3, 8, 8, 9, 8), (1, 4096, 3, 8, 8, 8, 9),
                 (0, 4096, 3, 8, 8, 8, 8)]:
        assert query('fte_preprocess_u8_align', x.data_ptr(), o.data_ptr(), *args, 0) != 0
    assert query('fte_preprocess_u8_align', None, o.data_ptr(), 1, 4096, 3, 8, 8, 8, 8, 0) != 0


def test_train_inputs_aligned_on_the_gpu_equal_the_host_pipeline(tmp_path, monkeypatch):
    """train_inputs(landmark_list_path=...) end to end: 2 worker processes + aligned raw slots + fte_preprocess_u8_align deliver
    the batches the all-host pipeline (FTE_LOADER_GPU=0) delivers for the same seed, labels included"""
    from tf_face_toolbox_amd import data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    kw = dict(is_color=1, augmentation=1, batch_size=8, device='cuda', seed=5, num_workers=2, landmark_list_path=lml)
    monkeypatch.setenv('FTE_LOADER_GPU', '0')
    a = data.train_inputs(lst, 112, 96, 100, 88, **kw)
    monkeypatch.setenv('FTE_LOADER_GPU', '1')
    b = data.train_inputs(lst, 112, 96, 100, 88, **kw)
    try:
        assert not a['gpu_transform'] and b['gpu_transform']
        for _ in range(4):
            xa, xb = a['images'](), b['images']()
            assert xb.shape == (8, 100, 88, 3) and xb.dtype == xa.dtype
            assert np.array_equal(xa.cpu().numpy().view(np.uint32), xb.cpu().numpy().view(np.uint32))
            assert np.array_equal(a['labels']().cpu().numpy(), b['labels']().cpu().numpy())
    finally:
        a['close'](); b['close']()


def test_eval_inputs_aligned_on_the_gpu_equal_the_host_pipeline(tmp_path, monkeypatch):
    from tf_face_toolbox_amd import data, preprocessing as pp, _decode_worker as dw
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    monkeypatch.setenv('FTE_LOADER_GPU', '0')
    a, n = data.eval_inputs(lst, 8, 1, 112, 112, device='cuda', num_workers=2, landmark_list_path=lml)
    monkeypatch.setenv('FTE_LOADER_GPU', '1')
    b, _ = data.eval_inputs(lst, 8, 1, 112, 112, device='cuda', num_workers=2, landmark_list_path=lml)
    try:
        assert n == 8
        for _ in range(2):
            xa, xb = a().cpu().numpy(), b().cpu().numpy()
            assert xb.shape == (8, 112, 112, 3) and _same_bits(xa, xb)
        first = (pp.aligned_image(dw._load(paths[0], 3), lm[0], 112, 112) - np.float32(0.5)) / np.float32(0.5)
        assert _same_bits(xb[0], first)
    finally:
        a.close(); b.close()
