"""The geometric augmentation's way to the GPU transform, host side (no GPU needed): augmentation 0 and 1 keep the bits and the
draws of the former _finish; for augmentation 2 and 3 the draws raw_example() writes into a slot header reproduce
train_example() bit for bit through the per-pixel restatement of the kernel's contract (tests/geo_ref.py); AFFINE_TABLE holds
what the reference's solve gives; fill_rows hands over raw slots with the geometric pair on."""
import os

import numpy as np
import pytest

import augment_ref as ar
import geo_ref as gr

IMG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'images')
NAMES = ['a.png', 'b.png', 'c.png', 'd.png', 'e.jpg', 'f.jpg', 'g.jpg', 'h.jpg']
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('geom', [(120, 116, 112, 112), (112, 96, -1, -1), (37, 29, 32, 24)])
@pytest.mark.parametrize('augmentation', [0, 1])
def test_augmentation_0_and_1_keep_the_bits_the_draws_and_the_headers(augmentation, geom, ch):
    """train_example == the frozen former _finish as uint32 with the generator left in the same state; the headers
    raw_example writes have words 10..15 zero and no geometric bit in word 6"""
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = geom
    for i, seed in enumerate(ar.SEEDS):
        path = os.path.join(IMG, NAMES[i % len(NAMES)])
        ra, rb = np.random.default_rng(seed), np.random.default_rng(seed)
        want = gr.finish_frozen(dw._load(path, ch), in_h, in_w, crop_h, crop_w, augmentation, ra)
        got = dw.train_example(path, ch, in_h, in_w, crop_h, crop_w, augmentation, rb)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), seed
        assert ra.random() == rb.random()
        slot = np.zeros(dw.HEADER_BYTES + 256 * 256 * ch, dtype=np.uint8)
        dw.raw_example(slot, path, ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed), augmentation)
        hd = slot[:64].view(np.int32)
        assert hd[0] == 0 and not hd[10:16].any() and 0 <= hd[6] < 8, (seed, hd)


def _check_seeds(ch, geom, augmentation, seeds, seen):
    from tf_face_toolbox_amd import _decode_worker as dw
    in_h, in_w, crop_h, crop_w = geom
    out_h, out_w = (crop_h, crop_w) if crop_h != -1 else (in_h, in_w)
    big = dw.HEADER_BYTES + 256 * 256 * ch
    for i, seed in enumerate(seeds):
        path = os.path.join(IMG, NAMES[i % len(NAMES)])
        want = dw.train_example(path, ch, in_h, in_w, crop_h, crop_w, augmentation, np.random.default_rng(seed))
        slot = np.zeros(big, dtype=np.uint8)
        dw.raw_example(slot, path, ch, in_h, in_w, crop_h, crop_w, np.random.default_rng(seed), augmentation)
        hd = gr.header(slot)
        assert hd[0] == 0 and hd[6] & gr.AFFINE and not slot[:64].view(np.int32)[13:16].any()
        assert bool(hd[6] & gr.ZOOM) == ((hd[10], hd[11]) != (out_h, out_w))
        if not augmentation & 1:
            assert hd[6] & 7 == 0
        seen.append((hd[6], hd[5], hd[10] / out_h, hd[12]))
        got = gr.restate_slot(slot, ch, in_h, in_w, out_h, out_w)
        assert got.shape == want.shape and want.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (seed, hd)
    return seen


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('geom', gr.SMALL_GEOMS)
@pytest.mark.parametrize('augmentation', [2, 3])
def test_slot_draws_and_the_per_pixel_recipe_reproduce_train_example(augmentation, geom, ch):
    """64 seeds per small geometry, channel count and augmentation value: header draws + restatement == train_example as
    uint32.  The seed list reaches: zoom applied and not applied, a zoom to 0.6 of the side or less, at least 20 distinct affine
    indices, both flips (the GPU test relies on the same list)."""
    seen = _check_seeds(ch, geom, augmentation, ar.SEEDS, [])
    assert {bool(s[0] & gr.ZOOM) for s in seen} == {False, True}
    assert any(s[0] & gr.ZOOM and s[2] <= 0.6 for s in seen)
    assert len({s[3] for s in seen}) >= 20 and all(0 <= s[3] <= 728 for s in seen)
    assert {s[1] for s in seen} == {0, 1}
    if augmentation == 3:
        assert {s[0] & 7 for s in seen} == (set(range(8)) if ch == 3 else {0, 1})


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('augmentation', [2, 3])
def test_the_training_geometry_reproduces_train_example(augmentation, ch):
    """(120, 116) -> crop 112 x 112, the first seeds of the list (geo_ref.BIG_SEEDS: the Python restatement of 12544 pixels takes
    seconds); zoomed and unzoomed images both occur among them"""
    seen = _check_seeds(ch, gr.BIG_GEOM, augmentation, gr.BIG_SEEDS, [])
    assert {bool(s[0] & gr.ZOOM) for s in seen} == {False, True}


def test_mode_1_slots_hold_the_finished_example_with_the_geometric_steps():
    from tf_face_toolbox_amd import _decode_worker as dw
    small = (dw.HEADER_BYTES + max(64 * 64 * 3, 32 * 24 * 3 * 4) + 63) // 64 * 64
    modes = set()
    for i, seed in enumerate(ar.SEEDS[:16]):
        path = os.path.join(IMG, NAMES[i % len(NAMES)])
        want = dw.train_example(path, 3, 37, 29, 32, 24, 3, np.random.default_rng(seed))
        slot = np.zeros(small, dtype=np.uint8)
        dw.raw_example(slot, path, 3, 37, 29, 32, 24, np.random.default_rng(seed), augmentation=3)
        modes.add(gr.header(slot)[0])
        assert np.array_equal(_bits(gr.restate_slot(slot, 3, 37, 29, 32, 24)), _bits(want)), seed
    assert modes == {0, 1}


def test_evaluation_slots_carry_no_geometric_draws():
    from tf_face_toolbox_amd import _decode_worker as dw
    slot = np.zeros(dw.HEADER_BYTES + 256 * 256 * 3, dtype=np.uint8)
    dw.raw_example(slot, os.path.join(IMG, NAMES[0]), 3, 37, 29, 32, 24, None, augmentation=3)
    assert not slot[:64].view(np.int32)[3:16].any()


def _solve(rnd):
    """the reference's arithmetic for one index, float64 (Python-2 `/` on ints is floor division)"""
    sx, sy = np.array([38, 89, 64]), np.array([55, 55, 105])
    tx = np.array([sx[0] + rnd // 243 - 1, sx[1] + rnd % 81 // 27 - 1, sx[2] + rnd % 9 // 3 - 1])
    ty = np.array([sy[0] + rnd % 243 // 81 - 1, sy[1] + rnd % 27 // 9 - 1, sy[2] + rnd % 3 - 1])
    a = np.transpose(np.vstack((sx, sy, np.ones(3))))
    return np.concatenate([np.linalg.solve(a, tx), np.linalg.solve(a, ty)]), (sx, sy, tx, ty)


def test_affine_table():
    """rows 0, 364 and 728 are the translation by -1, the identity and the translation by +1; every row is the float32 rounding
    of the solve (atol 1e-5: the values are O(1) and the solve is well conditioned)"""
    from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE as t
    assert t.shape == (729, 6) and t.dtype == np.float32
    for rnd, want in ((0, (1, 0, -1, 0, 1, -1)), (728, (1, 0, 1, 0, 1, 1)), (364, (1, 0, 0, 0, 1, 0))):
        assert np.allclose(t[rnd], np.asarray(want, dtype=np.float32), rtol=0, atol=1e-5), (rnd, t[rnd])
        assert np.allclose(t[rnd], _solve(rnd)[0].astype(np.float32), rtol=0, atol=1e-5)
    for rnd in range(729):
        assert np.allclose(t[rnd], _solve(rnd)[0].astype(np.float32), rtol=0, atol=1e-5), rnd
    assert len({r.tobytes() for r in t}) == 729


def test_a_one_landmark_row_moves_that_landmark_only():
    """rnd = 364 + 243: only the first landmark's x moves (by +1).  The coefficients take the source landmarks to the targets,
    and the inverse map takes the targets back to the source landmarks, within 1e-4."""
    from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE as t
    rnd = 364 + 243
    _, (sx, sy, tx, ty) = _solve(rnd)
    assert (tx - sx).tolist() == [1, 0, 0] and (ty - sy).tolist() == [0, 0, 0]
    m = np.vstack([t[rnd].astype(np.float64).reshape(2, 3), [0, 0, 1]])
    src, tgt = np.vstack([sx, sy, np.ones(3)]), np.vstack([tx, ty, np.ones(3)])
    assert np.abs(m @ src - tgt).max() <= 1e-4
    assert np.abs(np.linalg.inv(m) @ tgt - src).max() <= 1e-4


def test_the_array_code_equals_the_restatement_on_hand_set_cases():
    """zoom_in_out and affine_warp against geo_ref on the edge image: degenerate zoom shapes and the table's extreme rows"""
    from tf_face_toolbox_amd import preprocessing as pp
    img = ar.edge_image().astype(np.float32) * F(1.0 / 255.0)
    for th, tw in ((1, 1), (1, 16), (8, 8), (15, 16), (16, 1)):
        assert np.array_equal(_bits(pp.zoom_in_out(img, th, tw)), _bits(gr.zoom(img, th, tw))), (th, tw)
    assert pp.zoom_in_out(img, 16, 16) is not None and np.array_equal(_bits(pp.zoom_in_out(img, 16, 16)), _bits(img))
    t = pp.AFFINE_TABLE
    for rnd in (0, 364, 728, int(np.abs(t[:, 1]).argmax()), int(np.abs(t[:, 3]).argmax())):
        assert np.array_equal(_bits(pp.affine_warp(img, t[rnd])), _bits(gr.warp(img, t[rnd]))), rnd
    # the identity row is the solve's, residues of 1e-16 included (as the reference has it): the image to rounding, not to the bit
    assert np.allclose(pp.affine_warp(img, t[364]), img, rtol=0, atol=1e-6)
    assert (pp.affine_warp(img, t[0])[0] == 0).all() and (pp.affine_warp(img, t[0])[:, 0] == 0).all()      # zero fill


def test_fill_rows_hands_over_raw_slots_with_the_geometric_pair_on(tmp_path):
    """fill_rows(raw = 1, augmentation = 3) fills slots whose restatement equals the rows the float path writes"""
    from tf_face_toolbox_amd import _decode_worker as dw
    slot = dw.HEADER_BYTES + 256 * 256 * 3
    rows = [(i, os.path.join(IMG, NAMES[i % len(NAMES)]), 300 + i) for i in range(8)]
    raw_name, float_name = str(tmp_path / 'slots.bin'), str(tmp_path / 'rows.bin')
    np.zeros((8, slot), dtype=np.uint8).tofile(raw_name)
    np.zeros((8, 32, 24, 3), dtype=np.float32).tofile(float_name)
    assert dw.fill_rows((raw_name, (8, slot), rows, 3, 37, 29, 32, 24, 3, 1)) == 8
    assert dw.fill_rows((float_name, (8, 32, 24, 3), rows, 3, 37, 29, 32, 24, 3)) == 8
    slots = np.fromfile(raw_name, dtype=np.uint8).reshape(8, slot)
    want = np.fromfile(float_name, dtype=np.float32).reshape(8, 32, 24, 3)
    for i in range(8):
        assert gr.header(slots[i])[6] & gr.AFFINE
        assert np.array_equal(_bits(gr.restate_slot(slots[i], 3, 37, 29, 32, 24)), _bits(want[i])), i
    assert want.any()
