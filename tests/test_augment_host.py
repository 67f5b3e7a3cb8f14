"""The colour augmentation's way to the GPU transform, host side (no GPU needed): the draws raw_example() writes into a slot header
reproduce train_example(..., augmentation=1, ...) bit for bit through the plain per-pixel restatement of the kernel's contract
(tests/augment_ref.py); the refactored data_augmentation equals its frozen former self; fill_rows hands over raw slots with
the augmentation on and leaves the augmentation-0 slots byte for byte what they were."""
import os

import numpy as np
import pytest

import augment_ref as ar

IMG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'images')
NAMES = ['a.png', 'b.png', 'c.png', 'd.png', 'e.jpg', 'f.jpg', 'g.jpg', 'h.jpg']
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('geom', [(120, 116, 112, 112), (112, 96, -1, -1), (37, 29, 32, 24)])
def test_slot_draws_and_the_per_pixel_recipe_reproduce_train_example(ch, geom):
    """64 seeds per geometry and channel count: header draws + restatement == train_example(augmentation=1), as uint32; every
    flag combination occurs (8 for colour, 2 for gray), flips too; slots too small for the larger images hold the finished
    example (mode 1)."""
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = geom
    out_h, out_w = (crop_h, crop_w) if crop_h != -1 else (in_h, in_w)
    big = dw.HEADER_BYTES + 256 * 256 * ch
    small = (dw.HEADER_BYTES + max(64 * 64 * ch, out_h * out_w * ch * 4) + 63) // 64 * 64
    combos, flips, modes = set(), set(), set()
    for i, seed in enumerate(ar.SEEDS):
        path = os.path.join(IMG, NAMES[i % len(NAMES)])
        want = dw.train_example(path, ch, in_h, in_w, crop_h, crop_w, 1, np.random.default_rng(seed))
        slot = np.zeros(big, dtype=np.uint8)
        dw.raw_example(slot, path, ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed), augmentation=1)
        hd = ar.header(slot)
        assert hd[0] == 0
        combos.add(hd[6]); flips.add(hd[5])
        got = ar.restate_slot(slot, ch, in_h, in_w, out_h, out_w)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (seed, hd)
        slot = np.zeros(small, dtype=np.uint8)
        dw.raw_example(slot, path, ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed), augmentation=1)
        modes.add(ar.header(slot)[0])
        assert np.array_equal(_bits(ar.restate_slot(slot, ch, in_h, in_w, out_h, out_w)), _bits(want)), (seed, 'small slot')
    assert combos == (set(range(8)) if ch == 3 else {0, 1}), combos
    assert flips == {0, 1} and 1 in modes


@pytest.mark.parametrize('geom', ar.GEOMS)
def test_the_seed_list_reaches_every_flag_combination(geom):
    """the condition on the seed list the GPU test relies on, for all five geometries (the crop's draws come first, so the flags of a
    seed depend on whether the geometry crops)"""
    from tf_face_toolbox_amd.preprocessing import augmentation_draws
    in_h, in_w, crop_h, crop_w = geom
    for ch, want in ((3, set(range(8))), (1, {0, 1})):
        combos = set()
        for seed in ar.SEEDS:
            rng = np.random.default_rng(seed)
            if crop_h != -1:
                rng.integers(0, in_h - crop_h + 1); rng.integers(0, in_w - crop_w + 1)
            combos.add(augmentation_draws(rng, ch)[1])
        assert combos == want


def test_edge_image_holds_the_cases_it_is_meant_to():
    img = ar.edge_image().reshape(-1, 3).astype(int)
    have = {tuple(p) for p in img}
    for p in [(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
              (255, 0, 255)]:
        assert p in have
    assert any(r == g > b for r, g, b in img) and any(g == b > r for r, g, b in img)
    buf = ar.edge_slots()
    assert sorted(ar.header(s)[6] for s in buf) == sorted(list(range(8)) * 3)
    for flags in (2, 3, 6, 7):                                         # the floor-mod wrap, both sides of h == delta
        h = ar.hue_pixel_hue(flags)
        deltas = [ar.header(buf[flags + 8 * k])[8] for k in range(3)]
        assert deltas[0] == h and deltas[1] > h > deltas[2] and abs(float(deltas[1]) - float(deltas[2])) <= 2 * float(np.spacing(h))
        assert ar.hue_after_shift(h, deltas[0]) == 0
        assert ar.hue_after_shift(h, deltas[1]) == F(1)                # a tiny negative sum rounds up to exactly 1.0: sextant 6 % 6
        assert 0 < ar.hue_after_shift(h, deltas[2]) < 1e-6
    assert (img.min(1).astype(np.float32) * F(1.0 / 255.0) < ar.EDGE_BRIGHTNESS).any()      # brightness pushes values below 0


@pytest.mark.parametrize('ch', [3, 1])
def test_edge_image_recipe_equals_the_host_augmentation(ch):
    """the hand-set headers through the restatement against preprocessing.apply_augmentation on the same values: all 8 flag
    combinations, hue deltas at the wrap; brightness alone lets negative values through unclipped"""
    from tf_face_toolbox_amd import preprocessing as pp
    buf = ar.edge_slots(ch)
    lowest = {}
    for slot in buf:
        _, h0, w0, _, _, flip, flags, brightness, hue, saturation = ar.header(slot)
        img = slot[64:64 + h0 * w0 * ch].reshape(h0, w0, ch).astype(np.float32) * F(1.0 / 255.0)
        want = (pp.apply_augmentation(img, flip, flags, float(brightness), float(hue), float(saturation)) - F(0.5)) / F(0.5)
        got = ar.restate_slot(slot, ch, h0, w0, h0, w0)
        assert want.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), flags
        lowest[flags] = min(lowest.get(flags, 0), float(got.min()))
    assert lowest[1] < -1.0 and lowest[0] == -1.0
    if ch == 3:
        assert all(lowest[f] >= -1.0 for f in (2, 3, 4, 5, 6, 7))       # hue / saturation clip first


def _rgb_to_hsv_frozen(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(-1), rgb.min(-1)
    d = mx - mn
    s = np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0)
    dz = np.where(d > 0, d, 1)
    h = np.where(mx == r, (g - b) / dz % 6, np.where(mx == g, (b - r) / dz + 2, (r - g) / dz + 4)) / 6.0
    h = np.where(d > 0, h, 0)
    return np.stack([h, s, mx], -1)


def _hsv_to_rgb_frozen(hsv):
    h, s, v = hsv[..., 0] * 6.0, hsv[..., 1], hsv[..., 2]
    c = v * s
    x = c * (1 - np.abs(h % 2 - 1))
    z = np.zeros_like(c)
    i = np.floor(h).astype(int) % 6
    r = np.choose(i, [c, x, z, z, x, c])
    g = np.choose(i, [x, c, c, x, z, z])
    b = np.choose(i, [z, z, x, c, c, x])
    m = v - c
    return np.stack([r + m, g + m, b + m], -1)


def _data_augmentation_frozen(image, rng):
    """preprocessing.data_augmentation as it was before augmentation_draws was split off it"""
    if rng.random() < 0.5:
        image = image[:, ::-1, :]
    delta = rng.uniform(0, 0.2)
    if delta < 0.1:
        image = image - delta
    if image.shape[-1] == 3:
        delta = rng.uniform(0, 0.4)
        if delta < 0.2:
            hsv = _rgb_to_hsv_frozen(np.clip(image, 0, 1))
            hsv[..., 0] = (hsv[..., 0] + -delta) % 1.0
            image = _hsv_to_rgb_frozen(hsv)
        delta = rng.uniform(0.6, 1.4)
        if delta < 1.0:
            hsv = _rgb_to_hsv_frozen(np.clip(image, 0, 1))
            hsv[..., 1] = np.clip(hsv[..., 1] * delta, 0, 1)
            image = _hsv_to_rgb_frozen(hsv)
    return np.ascontiguousarray(image, dtype=np.float32)


@pytest.mark.parametrize('ch', [3, 1])
def test_data_augmentation_kept_its_bits_and_its_draws(ch):
    """240 seeds: the same output bits as the frozen copy, and the generator left in the same state (every draw consumed in the
    same order, applied or not)"""
    from tf_face_toolbox_amd import _decode_worker as dw
    from tf_face_toolbox_amd.preprocessing import data_augmentation
    images = [dw.decode(os.path.join(IMG, n), ch, 40, 36) for n in NAMES]
    for seed in range(240):
        img = images[seed % len(images)]
        if seed % 5 == 0:
            img = np.random.default_rng(1000 + seed).random((9, 11, ch), dtype=np.float32)
        ra, rb = np.random.default_rng(seed), np.random.default_rng(seed)
        want, got = _data_augmentation_frozen(img, ra), data_augmentation(img, rb)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), seed
        assert ra.random() == rb.random()


def test_fill_rows_hands_over_raw_slots_with_the_augmentation_on(tmp_path):
    """fill_rows(raw = 1, augmentation = 1) fills slots whose draws give train_example's bits; augmentation = 0 writes the bytes a
    call without the new parameter writes"""
    from tf_face_toolbox_amd import _decode_worker as dw
    slot = dw.HEADER_BYTES + 256 * 256 * 3
    rows = [(i, os.path.join(IMG, NAMES[i % len(NAMES)]), 300 + i) for i in range(8)]
    bufs = {}
    for aug in (0, 1):
        name = str(tmp_path / ('slots%d.bin' % aug))
        np.zeros((8, slot), dtype=np.uint8).tofile(name)
        assert dw.fill_rows((name, (8, slot), rows, 3, 37, 29, 32, 24, aug, 1)) == 8
        bufs[aug] = np.fromfile(name, dtype=np.uint8).reshape(8, slot)
    for i, (row, path, seed) in enumerate(rows):
        want = dw.train_example(path, 3, 37, 29, 32, 24, 1, np.random.default_rng(seed))
        assert np.array_equal(_bits(ar.restate_slot(bufs[1][i], 3, 37, 29, 32, 24)), _bits(want))
        old = np.zeros(slot, dtype=np.uint8)
        dw.raw_example(old, path, 3, 37, 29, 32, 24, np.random.default_rng(seed))              # the new parameter omitted
        assert np.array_equal(bufs[0][i], old)
        new = np.zeros(slot, dtype=np.uint8)
        dw.raw_example(new, path, 3, 37, 29, 32, 24, np.random.default_rng(seed), augmentation=0)
        assert np.array_equal(new, old)
    assert {ar.header(s)[6] for s in bufs[1]} != {0}
