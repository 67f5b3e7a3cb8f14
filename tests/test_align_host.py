"""Five-point alignment on the host (tf_face_toolbox_amd/preprocessing.py: align_template, similarity_from_landmarks, align_window,
align_warp; _decode_worker.py / data.py: the aligned transform, aligned raw slots, --landmark_list_path) against the independent
restatements of tests/align_ref.py.  CPU only; the GPU transform is held to this host definition by tests/test_gpu_align.py."""
import os

import numpy as np
import pytest

import align_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pp():
    from tf_face_toolbox_amd import preprocessing
    return preprocessing


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ estimate
def _point_sets():
    """200 (src, dst) sets: dst = a random similarity (rotation over the full circle, scale 0.2 .. 5) of src plus noise of up to
    2 % of the spread; every fourth set comes from the MIRRORED template (x -> 112 - x), which no rotation fits -- the residual is
    large there and the determinant correction of the SVD solution is in play."""
    rng = np.random.default_rng(20)
    sets = []
    while len(sets) < 200:
        k = len(sets)
        if k % 4 == 3:
            src = ar.TEMPLATE_112 * np.array([-1.0, 1.0]) + np.array([112.0, 0.0]) + rng.uniform(-1, 1, (5, 2))
        else:
            src = rng.uniform(0, 250, (5, 2))
        if src.std(0).min() < 10:
            continue
        m = ar.similarity(rng.uniform(-180, 180), rng.uniform(0.2, 5), rng.uniform(-100, 100), rng.uniform(-100, 100))
        base = ar.TEMPLATE_112 if k % 4 == 3 else src
        dst = ar.apply(m, base)
        dst = dst + rng.uniform(-0.02, 0.02, (5, 2)) * dst.std(0)
        sets.append((src, dst))
    return sets


def test_closed_form_similarity_equals_the_svd_umeyama():
    """every one of the six entries to 1e-9 RELATIVE TO THAT ENTRY, |got - want| <= 1e-9 |want|, both in float64.  All 200 sets
    agree, the 50 mirrored ones (det of the covariance < 0) included: checked when this test was written, worst per-entry
    difference 4.9e-13 of the entry.  Printed as well, not asserted: the difference relative to the similarity's scale (2 x 2
    part) and to max(|t|, scale * |mean of src|) (translation), worst 2e-15."""
    pp = _pp()
    worst = worst_scaled = 0.0
    mirrored = 0
    for src, dst in _point_sets():
        got, want = pp.similarity_from_landmarks(src, dst), ar.umeyama(src, dst)
        assert got.shape == (2, 3) and got.dtype == np.float64
        p, q = src - src.mean(0), dst - dst.mean(0)
        mirrored += np.linalg.det(q.T @ p) < 0
        err = np.abs(got - want) / np.abs(want)
        worst = max(worst, err.max())
        assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all(), (src, dst, got, want)
        scale = np.hypot(want[0, 0], want[1, 0])
        tref = max(np.abs(want[:, 2]).max(), scale * np.abs(src.mean(0)).max())
        worst_scaled = max(worst_scaled, np.abs(got[:, :2] - want[:, :2]).max() / scale, np.abs(got[:, 2] - want[:, 2]).max() / tref)
        assert got[0, 0] == got[1, 1] and got[0, 1] == -got[1, 0]                    # a similarity, not a general affine map
    assert mirrored == 50
    print('worst difference relative to the entry %.3g, relative to the scale of its part %.3g' % (worst, worst_scaled))


def test_coincident_points_are_refused():
    pp = _pp()
    with pytest.raises(ValueError):
        pp.similarity_from_landmarks(np.tile([[120.0, 77.0]], (5, 1)), pp.ALIGN_TEMPLATE_112)
    with pytest.raises(ValueError):
        pp.align_window(np.tile([120.0, 77.0], 5), 250, 250, 112, 112)
    with pytest.raises(ValueError):
        pp.similarity_from_landmarks(np.full((5, 2), np.nan), pp.ALIGN_TEMPLATE_112)


# ------------------------------------------------------------------ template
def test_templates():
    pp = _pp()
    assert np.array_equal(pp.ALIGN_TEMPLATE_112, ar.TEMPLATE_112)
    assert np.array_equal(pp.align_template(112, 112), ar.TEMPLATE_112)
    assert np.allclose(pp.align_template(112, 96), ar.TEMPLATE_112 - np.array([8.0, 0.0]), rtol=0, atol=1e-12)
    assert np.allclose(pp.align_template(224, 224), 2 * ar.TEMPLATE_112, rtol=0, atol=1e-12)
    assert np.array_equal(pp.ALIGN_TEMPLATE_112, ar.TEMPLATE_112)                    # align_template hands out copies


# ------------------------------------------------------------------ geometry
GEOMETRY = [(25.0, 1.7), (-40.0, 0.6)]


@pytest.mark.parametrize('in_h,in_w', [(112, 112), (112, 96)])
@pytest.mark.parametrize('angle,scale', GEOMETRY)
def test_blobs_at_the_landmarks_land_on_the_template(angle, scale, in_h, in_w):
    """a 250 x 250 image with five 5 x 5 blobs at landmarks that are the 112 template under a known similarity: after alignment
    the intensity centroid in the 7 x 7 window around each template point lies within 1.0 px of it in both axes.  Observed on
    the host definition: worst offset 0.36 px in each of the four cases (the blobs sit on whole source pixels, up to half a
    source pixel from the landmark)."""
    pp = _pp()
    m = ar.similarity(angle, scale)
    marks = ar.apply(m, ar.TEMPLATE_112 - ar.TEMPLATE_112.mean(0)) + np.array([127.3, 121.6])
    assert marks.min() > 10 and marks.max() < 240
    img = ar.dot_image(250, 250, marks)
    out = pp.aligned_image(img, marks.reshape(-1), in_h, in_w)
    assert out.shape == (in_h, in_w, 3) and out.dtype == np.float32
    worst = 0.0
    for tx, ty in pp.align_template(in_h, in_w):
        gx, gy = ar.centroid(out[:, :, 0], tx, ty)
        worst = max(worst, abs(gx - tx), abs(gy - ty))
    print('worst centroid offset %.3f px' % worst)
    assert worst <= 1.0


def test_aligned_image_is_the_float64_warp_by_the_inverse_umeyama():
    """the float32 host definition against the direct float64 warp of align_ref with the SVD similarity: equal to float32
    accuracy (coordinates below 256 carry 2^-16 px of rounding, an 8-bit step across one pixel is at most 1: 1e-4 of the range)"""
    pp = _pp()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)
    marks = ar.apply(ar.similarity(-17.0, 0.45, 12.0, 30.0), ar.TEMPLATE_112)
    got = pp.aligned_image(img, marks.reshape(-1), 28, 24)
    inv = ar.invert(ar.umeyama(marks, ar.TEMPLATE_112 * 0.25 + np.array([(24 - 28) / 2.0, 0.0])))
    want = ar.warp64(img / 255.0, inv, 28, 24)
    assert np.abs(got - want).max() <= 1e-4


# ------------------------------------------------------------------ window
def _warp_at_origin(image01, m6, wy0, wx0, in_h, in_w):
    """align_warp's formula with the SAME float32 m6 (translation relative to the window's corner, subtracted in float64 before
    the rounding), reading the WHOLE image at (fy + wy0, fx + wx0): zero outside the image, not outside the window"""
    h, w, _ = image01.shape
    a0, a1, a2, b0, b1, b2 = (np.float32(v) for v in m6)
    x = np.arange(in_w, dtype=np.float32)[None, :]
    y = np.arange(in_h, dtype=np.float32)[:, None]
    sx = (a0 * x + a1 * y) + a2
    sy = (b0 * x + b1 * y) + b2
    fx, fy = np.floor(sx), np.floor(sy)
    cx, cy = fx + np.float32(1), fy + np.float32(1)

    def read(yy, xx):
        yi, xi = yy.astype(np.int64) + wy0, xx.astype(np.int64) + wx0
        ok = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
        return np.where(ok[:, :, None], image01[np.where(ok, yi, 0), np.where(ok, xi, 0)], np.float32(0))
    wl, wr = (cx - sx)[:, :, None], (sx - fx)[:, :, None]
    top = wl * read(fy, fx) + wr * read(fy, cx)
    bot = wl * read(cy, fx) + wr * read(cy, cx)
    return (cy - sy)[:, :, None] * top + (sy - fy)[:, :, None] * bot


def test_windowed_warp_equals_the_warp_of_the_whole_image():
    """50 random similarities (faces from a seventh of the frame to larger than it, any rotation, partly outside): warping the
    window is warping the image -- the window holds every tap that lies inside the image"""
    pp = _pp()
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (180, 220, 3), dtype=np.uint8)
    img01 = img.astype(np.float32) * np.float32(1.0 / 255.0)
    small = clamped = 0
    for k in range(50):
        in_h, in_w = ((112, 112), (112, 96), (56, 48))[k % 3]
        m = ar.similarity(rng.uniform(-180, 180), rng.uniform(0.15, 2.5), rng.uniform(-20, 200), rng.uniform(-20, 160))
        marks = ar.apply(m, ar.TEMPLATE_112 - ar.TEMPLATE_112.mean(0)).reshape(-1)
        wy0, wx0, wh, ww, m6 = pp.align_window(marks, 180, 220, in_h, in_w)
        assert 0 <= wy0 and wy0 + wh <= 180 and 0 <= wx0 and wx0 + ww <= 220 and wh >= 1 and ww >= 1 and m6.dtype == np.float32
        small += wh * ww < 180 * 220 // 4
        clamped += wy0 == 0 or wx0 == 0 or wy0 + wh == 180 or wx0 + ww == 220
        got = pp.align_warp(img01[wy0:wy0 + wh, wx0:wx0 + ww], m6, in_h, in_w)
        assert _same_bits(got, _warp_at_origin(img01, m6, wy0, wx0, in_h, in_w)), k
        assert _same_bits(got, pp.aligned_image(img, marks, in_h, in_w))
        y0, x0 = in_h // 7, in_w // 5                                                 # a sub-window is that part of the whole
        part = pp.align_warp(img01[wy0:wy0 + wh, wx0:wx0 + ww], m6, in_h, in_w, y0, in_h - y0 - 3, x0, in_w - x0 - 1)
        assert _same_bits(part, np.ascontiguousarray(got[y0:in_h - 3, x0:in_w - 1]))
    assert small >= 10 and clamped >= 10


def test_window_clamped_at_the_border_reads_zeros_outside():
    pp = _pp()
    img = np.full((100, 120, 3), 255, dtype=np.uint8)
    # a face of the image's own size centred on the top left corner: three quarters of the aligned crop lie outside the image
    marks = (ar.TEMPLATE_112 - np.array([56.0, 56.0])).reshape(-1)
    wy0, wx0, wh, ww, m6 = pp.align_window(marks, 100, 120, 112, 112)
    assert (wy0, wx0) == (0, 0) and wh in (58, 59) and ww in (58, 59)                  # rows / columns 0 .. 55 (+ rounding) + 2 of padding
    out = pp.aligned_image(img, marks, 112, 112)
    assert (out[:55, :, :] == 0).all() and (out[:, :55, :] == 0).all()
    assert np.allclose(out[57:, 57:, :], 1.0, rtol=0, atol=1e-6)
    # a face far outside the image: the 1 x 1 window at (0, 0), zeros everywhere
    far = (ar.TEMPLATE_112 + np.array([5000.0, 300.0])).reshape(-1)
    assert pp.align_window(far, 100, 120, 112, 112)[:4] == (0, 0, 1, 1)
    assert (pp.aligned_image(img, far, 112, 112) == 0).all()
    # coordinates no window holds: every tap outside, the value is 0 and not NaN
    win = np.ones((4, 5, 3), dtype=np.float32)
    for m6 in ([np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 1e9, 0, 1, 1e9], [1, 0, 0, 0, 1, -np.inf]):
        assert (pp.align_warp(win, np.asarray(m6, dtype=np.float32), 6, 7) == 0).all()


# ------------------------------------------------------------------ loader, threads
def _host_example(path, lm, ch, in_h, in_w, crop_h, crop_w, augmentation, seed):
    """the host aligned transform from its parts, with the draws of one example taken here in the loader's order"""
    from tf_face_toolbox_amd import _decode_worker as dw
    pp = _pp()
    raw = dw._load(path, ch)
    if seed is None:
        return (pp.aligned_image(raw, lm, in_h, in_w) - np.float32(0.5)) / np.float32(0.5)
    rng = np.random.default_rng(seed)
    if crop_h != -1:
        y0 = int(rng.integers(0, in_h - crop_h + 1))
        x0 = int(rng.integers(0, in_w - crop_w + 1))
        image = pp.aligned_image(raw, lm, in_h, in_w, y0, crop_h, x0, crop_w)
    else:
        image = pp.aligned_image(raw, lm, in_h, in_w)
    if augmentation & 1:
        image = pp.apply_augmentation(image, *pp.augmentation_draws(rng, ch))
    elif rng.random() < 0.5:
        image = image[:, ::-1, :]
    return (np.ascontiguousarray(image, dtype=np.float32) - np.float32(0.5)) / np.float32(0.5)


@pytest.mark.parametrize('augmentation,crop', [(0, (-1, -1)), (1, (100, 88))])
def test_train_inputs_on_threads_equal_the_host_transform_image_by_image(tmp_path, augmentation, crop):
    from tf_face_toolbox_amd import data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    inputs = data.train_inputs(lst, 112, 96, crop[0], crop[1], is_color=1, augmentation=augmentation, batch_size=4, device='cpu', seed=7,
                               num_workers=0, landmark_list_path=lml)
    try:
        rng = np.random.default_rng(7)
        order = []
        for _ in range(3):
            if not order:
                order = list(rng.permutation(len(paths)))
            idx, order = order[:4], order[4:]
            seeds = rng.integers(0, 2 ** 31, size=4)
            x, y = inputs['images']().numpy(), inputs['labels']().numpy()
            assert list(y) == [labels[i] for i in idx]
            for row, (i, sd) in enumerate(zip(idx, seeds)):
                assert _same_bits(x[row], _host_example(paths[i], lm[i], 3, 112, 96, crop[0], crop[1], augmentation, int(sd))), (i, sd)
    finally:
        inputs['close']()


def test_train_inputs_class_balanced_and_sharded_carry_the_right_landmarks(tmp_path):
    """the PxK generator and world_size = 2: every delivered image is the aligned transform of ITS OWN landmarks (an image aligned
    with another image's landmarks differs) and comes with ITS OWN label as the generator renumbers it (class 1 keeps one image
    and is dropped: labels 0, 2, 3 become 0, 1, 2), and the two ranks together deliver the batch one rank delivers"""
    from tf_face_toolbox_amd import data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    keep = [i for i in range(len(paths)) if not paths[i].endswith('f.jpg')]             # f.jpg: the second image of class 1
    lst = str(tmp_path / 'list_pxk.txt')
    with open(lst, 'w') as f:
        f.write(''.join('%s %d\n' % (paths[i], labels[i]) for i in keep))
    renumbered = {0: 0, 2: 1, 3: 2}
    kw = dict(is_color=0, augmentation=0, num_classes=2, num_per_class=2, device='cpu', seed=3, num_workers=0, landmark_list_path=lml)
    whole = data.train_inputs(lst, 56, 48, **kw)
    halves = [data.train_inputs(lst, 56, 48, rank=r, world_size=2, **kw) for r in (0, 1)]
    try:
        table = {}
        for i in keep:
            for flip in (0, 1):
                v = _host_example(paths[i], lm[i], 1, 56, 48, -1, -1, 0, None)
                table[(v[:, ::-1] if flip else v).tobytes()] = labels[i]
        assert len(table) == 2 * len(keep)
        seen = set()
        for _ in range(4):
            x, y = whole['images']().numpy(), whole['labels']().numpy()
            for row in range(4):
                assert renumbered[table[x[row].tobytes()]] == y[row]
            seen.update(y.tolist())
            assert _same_bits(x, np.concatenate([h['images']().numpy() for h in halves]))
            assert np.array_equal(y, np.concatenate([h['labels']().numpy() for h in halves]))
        assert seen == {0, 1, 2}
    finally:
        for inp in [whole] + halves:
            inp['close']()


def test_eval_inputs_on_threads_equal_the_host_transform_image_by_image(tmp_path):
    from tf_face_toolbox_amd import data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    next_batch, n = data.eval_inputs(lst, 3, 1, 112, 112, device='cpu', num_workers=0, landmark_list_path=lml)
    try:
        assert n == len(paths)
        for b in range(4):                                                             # 12 images: the list wraps round
            x = next_batch().numpy()
            for row in range(3):
                i = (3 * b + row) % n
                assert _same_bits(x[row], _host_example(paths[i], lm[i], 3, 112, 112, -1, -1, 0, None)), i
    finally:
        next_batch.close()


def test_landmark_list_errors(tmp_path):
    from tf_face_toolbox_amd import data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    lines = open(lml).read().splitlines()
    short = tmp_path / 'short.txt'
    short.write_text('\n'.join(lines[:2] + lines[4:]) + '\n')                           # c.png and d.png have no landmarks
    for call in (lambda p: data.train_inputs(lst, 112, 96, batch_size=4, device='cpu', seed=1, num_workers=0, landmark_list_path=p),
                 lambda p: data.eval_inputs(lst, 4, 1, 112, 96, device='cpu', num_workers=0, landmark_list_path=p)):
        with pytest.raises(ValueError) as e:
            call(str(short))
        assert paths[2] in str(e.value) and '2 of the 8' in str(e.value)
        for bad in (lines[5].rsplit(' ', 1)[0], lines[5] + ' 1.0', lines[5].replace(lines[5].split()[3], 'x'), lines[5].split()[0] + ' nan' * 10):
            broken = tmp_path / 'broken.txt'
            broken.write_text('\n'.join(lines[:5] + [bad] + lines[6:]) + '\n')
            with pytest.raises(ValueError) as e:
                call(str(broken))
            assert 'line 6' in str(e.value)


def test_geometric_augmentation_with_landmarks_is_refused(tmp_path):
    from tf_face_toolbox_amd import _decode_worker as dw, data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    for aug in (2, 3):
        with pytest.raises(ValueError, match='geometric'):
            data.train_inputs(lst, 112, 96, augmentation=aug, batch_size=4, device='cpu', seed=1, num_workers=0, landmark_list_path=lml)
        with pytest.raises(ValueError, match='geometric'):
            dw.train_example(paths[0], 3, 112, 96, -1, -1, aug, np.random.default_rng(0), landmarks=lm[0])
        with pytest.raises(ValueError, match='geometric'):
            dw.raw_example(np.zeros(1 << 18, dtype=np.uint8), paths[0], 3, 112, 96, -1, -1, np.random.default_rng(0), aug, landmarks=lm[0])


def test_coincident_landmarks_name_the_image(tmp_path):
    from tf_face_toolbox_amd import _decode_worker as dw
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    with pytest.raises(ValueError) as e:
        dw.decode(paths[1], 3, 112, 96, landmarks=np.tile([40.0, 50.0], 5))
    assert paths[1] in str(e.value)


# ------------------------------------------------------------------ slots
@pytest.mark.parametrize('ch', [3, 1])
def test_raw_example_writes_the_aligned_header(tmp_path, ch):
    from tf_face_toolbox_amd import _decode_worker as dw, data
    pp = _pp()
    assert dw.HEADER_BYTES == 64 and dw.ALIGN_HEADER_BYTES == 128
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    nbytes = data.raw_slot_bytes(dw.ALIGN_HEADER_BYTES, ch, 100, 88)
    assert nbytes % 64 == 0 and nbytes >= 128 + 256 * 256 * ch
    for i, path in enumerate(paths):
        for aug, seed in ((0, 5 + i), (1, 40 + i), (0, None)):
            slot = np.full(nbytes, 0xAB, dtype=np.uint8)                                # stale bytes of an earlier batch
            crop = (-1, -1) if seed is None else (100, 88)
            dw.raw_example(slot, path, ch, 112, 96, crop[0], crop[1], None if seed is None else np.random.default_rng(seed), aug, landmarks=lm[i])
            raw = dw._load(path, ch)
            wy0, wx0, wh, ww, m6 = pp.align_window(lm[i], raw.shape[0], raw.shape[1], 112, 96)
            hd = slot[:128].view(np.int32)
            y0 = x0 = flip = flags = 0
            colour = (0.0, 0.0, 0.0)
            if seed is not None:
                rng = np.random.default_rng(seed)
                y0, x0 = int(rng.integers(0, 13)), int(rng.integers(0, 9))
                if aug:
                    flip, flags, *colour = pp.augmentation_draws(rng, ch)
                else:
                    flip = int(rng.random() < 0.5)
            assert hd[:7].tolist() == [0, wh, ww, y0, x0, flip, flags]
            assert _same_bits(hd[7:10].view(np.float32), np.asarray(colour, dtype=np.float32))
            assert not hd[10:16].any() and not hd[22:32].any()
            assert _same_bits(hd[16:22].view(np.float32), m6)
            assert np.array_equal(slot[128:128 + wh * ww * ch], raw[wy0:wy0 + wh, wx0:wx0 + ww].reshape(-1))


def test_small_slots_hold_the_finished_host_transform(tmp_path, monkeypatch):
    """FTE_LOADER_RAW_SIDE=16: the slot is as large as the finished crop needs and no larger; a window that does not fit is
    transformed by the worker and stored finished (mode 1) behind the 128-byte header"""
    from tf_face_toolbox_amd import _decode_worker as dw, data
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    monkeypatch.setenv('FTE_LOADER_RAW_SIDE', '16')
    nbytes = data.raw_slot_bytes(dw.ALIGN_HEADER_BYTES, 3, 32, 28)
    assert nbytes == (128 + 32 * 28 * 3 * 4 + 63) // 64 * 64
    modes = []
    for i, path in enumerate(paths):
        for aug, seed, crop in ((1, 9 + i, (32, 28)), (0, None, (-1, -1))):
            in_h, in_w = (36, 30) if seed is not None else (32, 28)
            slot = np.zeros(nbytes, dtype=np.uint8)
            dw.raw_example(slot, path, 3, in_h, in_w, crop[0], crop[1], None if seed is None else np.random.default_rng(seed), aug, landmarks=lm[i])
            hd = slot[:128].view(np.int32)
            modes.append(int(hd[0]))
            if hd[0] == 1:
                assert hd[:6].tolist() == [1, 32, 28, 0, 0, 0] and not hd[6:32].any()
                want = _host_example(path, lm[i], 3, in_h, in_w, crop[0], crop[1], aug, seed)
                assert _same_bits(slot[128:128 + want.size * 4].view(np.float32).reshape(want.shape), want)
    assert modes.count(1) >= 6 and modes.count(0) >= 2                                  # a.png's face is a few pixels wide: it fits


# ------------------------------------------------------------------ CLI
def test_both_parsers_take_the_flag_and_the_geometric_pair_is_refused():
    import evaluate
    import train
    base = ['--net_name', 'SphereNet-ArcFace', '--model_name', 'm']
    assert train.build_parser().parse_args(base).landmark_list_path is None
    assert evaluate.build_parser().parse_args(base).landmark_list_path is None
    assert evaluate.build_parser().parse_args(base + ['--landmark_list_path', 'lm.txt']).landmark_list_path == 'lm.txt'
    for aug in ('0', '1'):
        F = train.build_parser().parse_args(base + ['--landmark_list_path', 'lm.txt', '--augmentation', aug])
        assert F.landmark_list_path == 'lm.txt'
        train.landmark_flags_check(F)
    train.landmark_flags_check(train.build_parser().parse_args(base + ['--augmentation', '3']))      # no landmarks: nothing to refuse
    with pytest.raises(SystemExit, match='synthetic'):                                  # a resident random batch reads no images
        train.landmark_flags_check(train.build_parser().parse_args(base + ['--landmark_list_path', 'lm.txt', '--synthetic', '1']))
    for aug in ('2', '3'):
        with pytest.raises(SystemExit) as e:
            train.landmark_flags_check(train.build_parser().parse_args(base + ['--landmark_list_path', 'lm.txt', '--augmentation', aug]))
        assert 'geometric' in str(e.value)


# ------------------------------------------------------------------ align.py
def test_align_tool_writes_the_host_aligned_images(tmp_path):
    from PIL import Image
    import align
    from tf_face_toolbox_amd import _decode_worker as dw
    pp = _pp()
    lst, lml, paths, labels, lm = ar.golden_lists(tmp_path)
    out = tmp_path / 'crops'
    assert align.main(['--data_list_path', lst, '--landmark_list_path', lml, '--input_height', '112', '--input_width', '96',
                       '--out_dir', str(out)]) == 0
    lines = [ln.split() for ln in open(str(out / 'list.txt'))]
    assert [int(p[1]) for p in lines] == labels
    for (dst, _), path, marks in zip(lines, paths, lm):
        assert dst.startswith(str(out)) and dst.endswith(os.path.splitext(path)[0].lstrip(os.sep) + '.png')
        got = np.asarray(Image.open(dst))
        want = np.rint(pp.aligned_image(dw._load(path, 3), marks, 112, 96).astype(np.float64) * 255.0).astype(np.uint8)
        assert got.shape == (112, 96, 3) and np.array_equal(got, want)
    gray = tmp_path / 'gray'
    align.main(['--data_list_path', lst, '--landmark_list_path', lml, '--input_height', '56', '--input_width', '56', '--is_color', '0',
                '--out_dir', str(gray), '--out_list', str(tmp_path / 'gray.txt')])
    first = open(str(tmp_path / 'gray.txt')).readline().split()[0]
    want = np.rint(pp.aligned_image(dw._load(paths[0], 1), lm[0], 56, 56).astype(np.float64) * 255.0).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(first)), want[:, :, 0])
