"""Plain per-pixel restatement of the loader's geometric augmentation (fte_preprocess_u8_geo, include/fte.h): the zoom (TF-1.x
bilinear down to th x tw and back up) and the affine warp (tf.contrib.image.transform, 'BILINEAR', zero outside), written from
the contract with np.float32 scalars -- one rounding per operation -- independently of the array code in
tf_face_toolbox_amd/preprocessing.py and of the kernel, as tests/augment_ref.py is for the colour part, whose pixel() finishes
every pixel here.  Also the frozen former _decode_worker._finish (augmentation 0 and 1 must keep its bits and its draws).
Shared by tests/test_geo_augment_host.py and tests/test_gpu_geo_augment.py."""
import numpy as np

import augment_ref as ar

F = np.float32
ZOOM, AFFINE = 8, 16
SMALL_GEOMS = [(37, 29, 32, 24), (37, 29, 31, 23), (37, 29, -1, -1)]       # 768, 713 and 1073 pixels: the last two are no multiple of 256
BIG_GEOM = (120, 116, 112, 112)
BIG_SEEDS = ar.SEEDS[:6]          # the per-pixel Python restatement of a 112 x 112 image takes seconds: six seeds of it per case


def finish_frozen(raw, input_height, input_width, crop_height, crop_width, augmentation, rng):
    """_decode_worker._finish as it was before the geometric pair: `augmentation` is a truth value"""
    from tf_face_toolbox_amd import _decode_worker as dw
    from tf_face_toolbox_amd.preprocessing import data_augmentation
    if crop_height != -1 and crop_width != -1:
        y0 = rng.integers(0, input_height - crop_height + 1)
        x0 = rng.integers(0, input_width - crop_width + 1)
        image = dw.resize_window(raw, input_height, input_width, y0, crop_height, x0, crop_width)
    else:
        image = dw.resize_window(raw, input_height, input_width)
    if augmentation:
        image = data_augmentation(image, rng)
    elif rng.random() < 0.5:
        image = image[:, ::-1, :]
    return (np.ascontiguousarray(image, dtype=np.float32) - 0.5) / 0.5


def _tap(n_in, n_out, i):
    """in = out * (n_in / n_out); low = floor(in); high = min(low + 1, n_in - 1); weight of high = in - low"""
    pos = F(i) * (F(n_in) / F(n_out))
    lo = int(np.floor(pos))
    assert 0 <= lo <= n_in - 1
    return lo, min(lo + 1, n_in - 1), pos - F(lo)


def resize(img, dh, dw):
    """TF-1.x ResizeBilinear (align_corners=False) of a float32 HWC image, one pixel at a time: along x, then along y"""
    sh, sw, ch = img.shape
    out = np.empty((dh, dw, ch), dtype=np.float32)
    xs = [_tap(sw, dw, x) for x in range(dw)]
    for y in range(dh):
        ylo, yhi, yw = _tap(sh, dh, y)
        for x in range(dw):
            xlo, xhi, xw = xs[x]
            for c in range(ch):
                a, b, d, e = img[ylo, xlo, c], img[ylo, xhi, c], img[yhi, xlo, c], img[yhi, xhi, c]
                top = (b - a) * xw + a
                bot = (e - d) * xw + d
                v = (bot - top) * yw + top
                assert type(v) is np.float32
                out[y, x, c] = v
    return out


def zoom(img, th, tw):
    return resize(resize(img, th, tw), img.shape[0], img.shape[1])


def warp(img, coef):
    """out(x, y) = bilinear read of img at ((a0 x + a1 y) + a2, (b0 x + b1 y) + b2), 0 outside the image"""
    h, w, ch = img.shape
    a0, a1, a2, b0, b1, b2 = (F(v) for v in coef)
    out = np.empty((h, w, ch), dtype=np.float32)

    def read(yy, xx, c):
        if 0 <= yy <= h - 1 and 0 <= xx <= w - 1:
            return img[int(yy), int(xx), c]
        return F(0)
    for y in range(h):
        for x in range(w):
            sx = (a0 * F(x) + a1 * F(y)) + a2
            sy = (b0 * F(x) + b1 * F(y)) + b2
            fx, fy = np.floor(sx), np.floor(sy)
            cx, cy = fx + F(1), fy + F(1)
            for c in range(ch):
                top = (cx - sx) * read(fy, fx, c) + (sx - fx) * read(fy, cx, c)
                bot = (cx - sx) * read(cy, fx, c) + (sx - fx) * read(cy, cx, c)
                v = (cy - sy) * top + (sy - fy) * bot
                assert type(v) is np.float32
                out[y, x, c] = v
    return out


def header(slot):
    """augment_ref.header's ten fields + (th, tw, rnd)"""
    return ar.header(slot) + tuple(int(x) for x in slot[:64].view(np.int32)[10:13])


def geometry_of(flags, th, tw, rnd, out_h, out_w):
    """(zoom applied, affine applied) as the contract decides them: a word out of its range clears its bit"""
    return (bool(flags & ZOOM) and 1 <= th <= out_h and 1 <= tw <= out_w, bool(flags & AFFINE) and 0 <= rnd <= 728)


def restate_slot(slot, ch, in_h, in_w, out_h, out_w, table=None):
    """what fte_preprocess_u8_geo computes from one slot: the host's resize of the window, then zoom, warp, flip and
    augment_ref.pixel() one pixel at a time"""
    from tf_face_toolbox_amd import _decode_worker as dw
    if table is None:
        from tf_face_toolbox_amd.preprocessing import AFFINE_TABLE as table
    mode, h0, w0, y0, x0, flip, flags, brightness, hue, saturation, th, tw, rnd = header(slot)
    if mode == 1:
        return slot[64:64 + out_h * out_w * ch * 4].view(np.float32).reshape(out_h, out_w, ch).copy()
    raw = slot[64:64 + h0 * w0 * ch].reshape(h0, w0, ch)
    img = np.ascontiguousarray(dw.resize_window(raw, in_h, in_w, y0, out_h, x0, out_w))
    assert img.dtype == np.float32
    zoomed, warped = geometry_of(flags, th, tw, rnd, out_h, out_w)
    if zoomed:
        img = zoom(img, th, tw)
    if warped:
        img = warp(img, table[rnd])
    if flip:
        img = img[:, ::-1, :]
    out = np.empty((out_h, out_w, ch), dtype=np.float32)
    for y in range(out_h):
        for x in range(out_w):
            out[y, x] = ar.pixel(img[y, x], flags, brightness, hue, saturation)
    return out


def edge_slots(ch, cases):
    """slots of augment_ref.edge_image() passed straight through (16 x 16, no resize, no crop) under hand-set headers:
    cases = [(geometry flags, th, tw, rnd, colour flags, flip), ...]"""
    img = ar.edge_image() if ch == 3 else ar.edge_image()[:, :, 1:2]
    s = ar.EDGE_SIDE
    buf = np.zeros((len(cases), 64 + s * s * 4), dtype=np.uint8)
    for i, (geo, th, tw, rnd, colour, flip) in enumerate(cases):
        hd = buf[i, :64].view(np.int32)
        hd[:7] = (0, s, s, 0, 0, flip, geo | colour)
        hd[7:10].view(np.float32)[:] = (ar.EDGE_BRIGHTNESS, F(0.125), ar.EDGE_SATURATION)
        hd[10:13] = (th, tw, rnd)
        buf[i, 64:64 + img.size] = img.reshape(-1)
    return buf
