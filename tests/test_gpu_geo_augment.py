"""The loader's GPU transform with the geometric augmentation (fte_preprocess_u8_geo, include/fte.h): decoded uint8 images + the
workers' seeded draws in, the float32 NHWC batch of train_inputs(..., augmentation=2 | 3) out -- BIT-EQUAL to the host transform
(tf_face_toolbox_amd/_decode_worker.py + preprocessing.py, themselves held to the per-pixel restatement tests/geo_ref.py by
tests/test_geo_augment_host.py).  Mirrors tests/test_gpu_augment.py."""
import os

import numpy as np
import pytest

import augment_ref as ar
import geo_ref as gr

pytestmark = pytest.mark.gpu

IMG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'images')
NAMES = ['a.png', 'b.png', 'c.png', 'd.png', 'e.jpg', 'f.jpg', 'g.jpg', 'h.jpg']
# every geometry of augment_ref.GEOMS is a multiple of 256 pixels; (37, 29, 31, 23) and (37, 29, -1, -1) give 713 and 1073: a last
# trip of the workgroup's pixel loops that is partly filled
GEOMS = ar.GEOMS + [(37, 29, 31, 23), (37, 29, -1, -1)]
S = ar.EDGE_SIDE


def _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes, augmentation):
    from tf_face_toolbox_amd import _decode_worker as dw
    buf = np.zeros((len(seeds), nbytes), dtype=np.uint8)
    for i, seed in enumerate(seeds):
        dw.raw_example(buf[i], os.path.join(IMG, NAMES[i % len(NAMES)]), ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed),
                       augmentation)
    return buf


def _table():
    import torch
    from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE
    return torch.from_numpy(AFFINE_TABLE).cuda()


def _gpu(buf, ch, in_h, in_w, out_h, out_w, entry='fte_preprocess_u8_geo'):
    import torch
    from tf_face_toolbox_amd._lib import call, query
    raw = torch.from_numpy(buf).cuda()
    out = torch.empty((buf.shape[0], out_h, out_w, ch), dtype=torch.float32, device='cuda')
    extra = ()
    if entry == 'fte_preprocess_u8_geo':
        ws_bytes = query('fte_preprocess_u8_geo_ws_bytes', buf.shape[0], ch, out_h, out_w)
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device='cuda')
        extra = (_table(), ws, ws_bytes)
    call(entry, raw.data_ptr(), out.data_ptr(), buf.shape[0], buf.shape[1], ch, in_h, in_w, out_h, out_w, *extra,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('geom', GEOMS)
@pytest.mark.parametrize('augmentation', [2, 3])
def test_geometric_transform_is_bit_equal_to_the_host(augmentation, geom, ch):
    """resize + crop + zoom + affine + flip (+ colour) + normalise for the seeded examples of each geometry (64; 16 for the
    224 x 224 crop, whose planes go through the workspace even for gray); slots large enough for every image, and slots that
    force the larger ones through the finished-crop path.  Zoomed and unzoomed images, flips and many affine rows occur."""
    import torch  # noqa: F401  (before the library is loaded, as everywhere: libfte.so then binds to the HIP runtime torch brought)
    from tf_face_toolbox_amd import _decode_worker as dw
    from tf_face_toolbox_amd._lib import query
    in_h, in_w, crop_h, crop_w = geom
    out_h, out_w = (crop_h, crop_w) if crop_h != -1 else (in_h, in_w)
    seeds = ar.SEEDS[:16] if out_h == 224 else ar.SEEDS
    ws_bytes = query('fte_preprocess_u8_geo_ws_bytes', len(seeds), ch, out_h, out_w)
    planes = 2 * out_h * out_w * ch * 4
    assert ws_bytes == (0 if planes <= 160 * 1024 else planes * len(seeds))
    if out_h == 224:
        assert ws_bytes > 0
    if (out_h, out_w, ch) == (112, 112, 1):
        assert ws_bytes == 0                            # gray 112 x 112: both planes in LDS
    if (out_h, out_w, ch) == (112, 112, 3):
        assert ws_bytes > 0
    want = np.stack([dw.train_example(os.path.join(IMG, NAMES[i % len(NAMES)]), ch, in_h, in_w, crop_h, crop_w, augmentation,
                                      np.random.default_rng(s)) for i, s in enumerate(seeds)])
    for side in (256, 64):
        nbytes = (dw.HEADER_BYTES + max(side * side * ch, out_h * out_w * ch * 4) + 63) // 64 * 64
        buf = _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes, augmentation)
        hd = buf[:, :dw.HEADER_BYTES].view(np.int32)
        if side == 256:
            assert (hd[:, 0] == 0).all() and 0 < hd[:, 5].sum() < len(seeds)
            assert (hd[:, 6] & gr.AFFINE).all() and 0 < (hd[:, 6] & gr.ZOOM).astype(bool).sum() < len(seeds)
            assert len(set(hd[:, 12].tolist())) >= (20 if len(seeds) == 64 else 10)
            if augmentation == 3 and len(seeds) == 64:
                assert set((hd[:, 6] & 7).tolist()) == (set(range(8)) if ch == 3 else {0, 1})
        else:                                           # d.png, the largest image, is 250 x 250: finished by the worker when it does not fit
            assert (hd[:, 0] == 1).any() == (250 * 250 * ch > nbytes - dw.HEADER_BYTES)
        got = _gpu(buf, ch, in_h, in_w, out_h, out_w)
        bad = [s for i, s in enumerate(seeds) if not _same_bits(got[i], want[i])]
        assert not bad, 'slot side %d: seeds %s differ' % (side, bad)


def _edge_cases():
    from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE as t
    rnds = [0, 364, 728, int(np.abs(t[:, 1]).argmax()), int(np.abs(t[:, 3]).argmax())]
    assert len(set(rnds)) == 5
    cases = [(gr.ZOOM | gr.AFFINE, th, tw, rnd, colour, flip)
             for th, tw in ((1, 1), (1, 16), (8, 8), (15, 16), (16, 16)) for rnd in rnds for colour in (0, 7) for flip in (0, 1)]
    cases += [(gr.ZOOM, 8, 8, rnds[3], 7, 1), (gr.AFFINE, 8, 8, rnds[3], 7, 1), (gr.ZOOM, 5, 11, 0, 0, 0), (gr.AFFINE, 0, 0, rnds[4], 0, 0)]
    return cases


@pytest.mark.parametrize('ch', [3, 1])
def test_edge_image_under_hand_set_headers_is_bit_equal_to_the_per_pixel_recipe(ch):
    """the 16 x 16 edge image, no resize: zoom shapes (1, 1), (1, 16), (8, 8), (15, 16) and (16, 16) with bit 8 set x the table's
    rows 0, 364, 728 and the two with the largest |a1| and |b0| x colour flags {0, 7} x both flips, and one bit at a time"""
    cases = _edge_cases()
    buf = gr.edge_slots(ch, cases)
    got = _gpu(buf, ch, S, S, S, S)
    for i, slot in enumerate(buf):
        assert _same_bits(got[i], gr.restate_slot(slot, ch, S, S, S, S)), cases[i]
    assert cases[40][1:4] == (8, 8, 0) and cases[44][1:4] == (8, 8, 364)
    assert not _same_bits(got[40], got[44])              # the same zoom, rows 0 and 364: the warp changes the image


@pytest.mark.parametrize('ch', [3, 1])
def test_out_of_range_header_words_clear_their_bit(ch):
    """words 10..12 steer addresses: th = 0, th = out_h + 1, tw = -1 give the output of the same slot without bit 8, rnd = 729
    and rnd = -1 the output without bit 16 -- defined inputs with a defined result"""
    from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE as t
    row = int(np.abs(t[:, 1]).argmax())
    both = gr.ZOOM | gr.AFFINE
    bad = [(both, 0, 8, row, 7, 1), (both, S + 1, 8, row, 7, 0), (both, 8, -1, row, 0, 1), (both, 8, 8, 729, 7, 1), (both, 8, 8, -1, 0, 0),
           (both, 2 ** 31 - 1, 8, row, 7, 0), (both, 8, 8, 2 ** 31 - 1, 7, 0), (both, 8, 8, -2 ** 31, 7, 0)]
    cleared = [(gr.AFFINE,) + c[1:] for c in bad[:3]] + [(gr.ZOOM,) + c[1:] for c in bad[3:5]] + \
              [(gr.AFFINE,) + bad[5][1:], (gr.ZOOM,) + bad[6][1:], (gr.ZOOM,) + bad[7][1:]]
    got = _gpu(gr.edge_slots(ch, bad), ch, S, S, S, S)
    want = _gpu(gr.edge_slots(ch, cleared), ch, S, S, S, S)
    valid = _gpu(gr.edge_slots(ch, [(both, 8, 8, row, 7, 1)]), ch, S, S, S, S)[0]
    for i, case in enumerate(bad):
        assert _same_bits(got[i], want[i]), case
        assert _same_bits(got[i], gr.restate_slot(gr.edge_slots(ch, [case])[0], ch, S, S, S, S)), case
        assert not _same_bits(got[i], valid)


@pytest.mark.parametrize('ch', [3, 1])
def test_no_geometric_bit_is_the_colour_transform_and_the_older_entries_ignore_the_new_words(ch):
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = 120, 116, 112, 112
    nbytes = dw.HEADER_BYTES + 256 * 256 * ch
    seeds = ar.SEEDS[:16]
    buf = _slots(ch, in_h, in_w, crop_h, crop_w, seeds, nbytes, 3)
    hd = buf[:, :dw.HEADER_BYTES].view(np.int32)
    assert (hd[:, 6] & 24).all() and hd[:, 10:13].any(0).all()
    nogeo = buf.copy()
    nogeo[:, :dw.HEADER_BYTES].view(np.int32)[:, 6] &= 7                                 # words 10..12 still set
    zeroed = nogeo.copy()
    zeroed[:, :dw.HEADER_BYTES].view(np.int32)[:, 10:13] = 0
    for entry in ('fte_preprocess_u8_aug', 'fte_preprocess_u8'):                         # bits 8, 16 and words 10..12 are ignored
        base = _gpu(zeroed, ch, in_h, in_w, crop_h, crop_w, entry)
        assert _same_bits(base, _gpu(buf, ch, in_h, in_w, crop_h, crop_w, entry))
        assert _same_bits(base, _gpu(nogeo, ch, in_h, in_w, crop_h, crop_w, entry))
    aug = _gpu(zeroed, ch, in_h, in_w, crop_h, crop_w, 'fte_preprocess_u8_aug')
    assert _same_bits(aug, _gpu(nogeo, ch, in_h, in_w, crop_h, crop_w))
    assert _same_bits(aug, _gpu(zeroed, ch, in_h, in_w, crop_h, crop_w))
    assert not _same_bits(aug, _gpu(buf, ch, in_h, in_w, crop_h, crop_w))


def test_bad_arguments_are_refused():
    import torch
    from tf_face_toolbox_amd._lib import query
    x = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    o = torch.zeros(4096, dtype=torch.float32, device='cuda')
    t = _table()
    for args in [(1, 100, 3, 8, 8, 8, 8), (1, 4096, 2, 8, 8, 8, 8), (1, 4096, 3, 8, 8, 9, 8), (0, 4096, 3, 8, 8, 8, 8)]:
        assert query('fte_preprocess_u8_geo', x.data_ptr(), o.data_ptr(), *args, t.data_ptr(), None, 0, 0) != 0
    assert query('fte_preprocess_u8_geo', x.data_ptr(), o.data_ptr(), 1, 4096, 3, 8, 8, 8, 8, None, None, 0, 0) != 0      # no table
    assert query('fte_preprocess_u8_geo_ws_bytes', 1, 3, 8, 8) == 0
    need = query('fte_preprocess_u8_geo_ws_bytes', 2, 3, 224, 224)                       # planes too large for LDS
    assert need == 2 * 2 * 224 * 224 * 3 * 4
    big = torch.zeros((2, 64 + 16 * 16 * 3 + 48), dtype=torch.uint8, device='cuda')      # zero headers: never read past them
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.zeros((2, 224, 224, 3), dtype=torch.float32, device='cuda')
    args = (big.data_ptr(), out.data_ptr(), 2, big.shape[1], 3, 224, 224, 224, 224, t.data_ptr())
    assert query('fte_preprocess_u8_geo', *args, ws.data_ptr(), need - 1, 0) != 0
    assert query('fte_preprocess_u8_geo', *args, None, need, 0) != 0


def test_train_inputs_with_geometric_augmentation_on_the_gpu_equal_the_host_pipeline(tmp_path, monkeypatch):
    """train_inputs(augmentation=3) end to end on the GPU box: worker processes + raw slots + fte_preprocess_u8_geo deliver the
    batches the all-host pipeline delivers for the same seed, labels included."""
    from tf_face_toolbox_amd import data
    lst = tmp_path / 'list.txt'
    lst.write_text(''.join('%s %d\n' % (os.path.join(IMG, n), i % 4) for i, n in enumerate(NAMES * 4)))
    monkeypatch.setenv('FTE_LOADER_GPU', '0')
    a = data.train_inputs(str(lst), 120, 116, 112, 112, is_color=1, augmentation=3, batch_size=16, device='cuda', seed=5, num_workers=3)
    monkeypatch.setenv('FTE_LOADER_GPU', '1')
    b = data.train_inputs(str(lst), 120, 116, 112, 112, is_color=1, augmentation=3, batch_size=16, device='cuda', seed=5, num_workers=3)
    try:
        assert not a['gpu_transform'] and b['gpu_transform']
        for _ in range(6):
            xa, xb = a['images'](), b['images']()
            assert xb.shape == (16, 112, 112, 3) and xb.dtype == xa.dtype
            assert np.array_equal(xa.cpu().numpy().view(np.uint32), xb.cpu().numpy().view(np.uint32))
            assert np.array_equal(a['labels']().cpu().numpy(), b['labels']().cpu().numpy())
    finally:
        a['close'](); b['close']()
