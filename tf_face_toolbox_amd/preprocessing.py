"""Host-side image augmentation: mirror of the reference's preprocessing.py.  Lines 22-38 (the only function the reference's
train_inputs calls): numpy restatements of tf.image.{random_flip_left_right, adjust_brightness, adjust_hue, adjust_saturation}.
Lines 41-71 (_random_zoom_in_out, _random_affine_distort, which the reference defines and never calls): the geometric pair
below, `augmentation & 2`.  The array code here is the bit-exact specification of the loader's GPU transforms
(fte_preprocess_u8_aug, fte_preprocess_u8_geo; include/fte.h)."""
import colorsys  # noqa: F401  (documented reference for the HSV convention below)

import numpy as np


def _rgb_to_hsv(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(-1), rgb.min(-1)
    d = mx - mn
    s = np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0)
    dz = np.where(d > 0, d, 1)
    h = np.where(mx == r, (g - b) / dz % 6, np.where(mx == g, (b - r) / dz + 2, (r - g) / dz + 4)) / 6.0
    h = np.where(d > 0, h, 0)
    return np.stack([h, s, mx], -1)


def _hsv_to_rgb(hsv):
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


def adjust_hue(image, delta):
    hsv = _rgb_to_hsv(image)
    hsv[..., 0] = (hsv[..., 0] + delta) % 1.0
    return _hsv_to_rgb(hsv)


def adjust_saturation(image, factor):
    hsv = _rgb_to_hsv(image)
    hsv[..., 1] = np.clip(hsv[..., 1] * factor, 0, 1)
    return _hsv_to_rgb(hsv)


BRIGHTNESS, HUE, SATURATION = 1, 2, 4        # flag bits of augmentation_draws (and of the slot header, include/fte.h)


def augmentation_draws(rng, num_channels):
    """The random draws of data_augmentation, in its order, ALL of them consumed whether applied or not:
    (flip, flags, brightness delta, hue delta, saturation factor).  `flags` holds the decisions
    delta < 0.1 / < 0.2 / < 1.0, taken on the float64 draws; gray images draw neither hue nor saturation."""
    flip = int(rng.random() < 0.5)
    brightness = rng.uniform(0, 0.2)
    flags = BRIGHTNESS if brightness < 0.1 else 0
    hue, saturation = 0.0, 1.0
    if num_channels == 3:
        hue = rng.uniform(0, 0.4)
        if hue < 0.2:
            flags |= HUE
        saturation = rng.uniform(0.6, 1.4)
        if saturation < 1.0:
            flags |= SATURATION
    return flip, flags, brightness, hue, saturation


def apply_augmentation(image, flip, flags, brightness, hue, saturation):
    """data_augmentation with the draws given: flip; darken; RGB only: hue shift by -hue, desaturate."""
    if flip:
        image = image[:, ::-1, :]
    if flags & BRIGHTNESS:
        image = image - brightness
    if image.shape[-1] == 3:
        if flags & HUE:
            image = adjust_hue(np.clip(image, 0, 1), -hue)
        if flags & SATURATION:
            image = adjust_saturation(np.clip(image, 0, 1), saturation)
    return np.ascontiguousarray(image, dtype=np.float32)


def data_augmentation(image, rng):
    """preprocessing.py:22-38: flip; with prob 1/2 darken by delta in [0,0.1); RGB only: with prob 1/2
    hue shift by -delta (delta in [0,0.2)), with prob 1/2 desaturate by a factor in [0.6,1)."""
    return apply_augmentation(image, *augmentation_draws(rng, image.shape[-1]))


# ------------------------------------------------------------------ geometric pair (preprocessing.py:41-71 of the reference)
GEOMETRIC = 2                                # bit of `augmentation`: zoom + affine before the flip / colour part
ZOOM, AFFINE = 8, 16                         # flag bits of the slot header's word 6 (include/fte.h: fte_preprocess_u8_geo)
LANDMARKS_X, LANDMARKS_Y = (38, 89, 64), (55, 55, 105)
# The landmarks are two eyes and the mouth of a 128 x 128 aligned face, in PIXELS of the image being warped whatever its size
# -- as the reference has them: on a 112 x 112 crop they sit 8 pixels low and right of the features, on a 32 x 24 image two of
# them lie outside it.  The warp stays a one-pixel perturbation either way (the solve is exact for any three points).


def _affine_table():
    """All 729 coefficient sets of _random_affine_distort: each landmark moves by -1, 0 or +1 pixel in x and in y (rnd in base 3,
    Python-2 integer division), A t = target solved in float64 for x and for y, the six coefficients (a0, a1, a2, b0, b1, b2)
    cast to float32.  An OUTPUT pixel (x, y) samples the source at (a0 x + a1 y + a2, b0 x + b1 y + b2)."""
    a = np.stack([np.asarray(LANDMARKS_X, np.float64), np.asarray(LANDMARKS_Y, np.float64), np.ones(3)], 1)
    table = np.empty((729, 6), dtype=np.float32)
    for rnd in range(729):
        dx = (rnd // 243 - 1, rnd % 81 // 27 - 1, rnd % 9 // 3 - 1)
        dy = (rnd % 243 // 81 - 1, rnd % 27 // 9 - 1, rnd % 3 - 1)
        table[rnd, :3] = np.linalg.solve(a, a[:, 0] + dx)
        table[rnd, 3:] = np.linalg.solve(a, a[:, 1] + dy)
    return table


AFFINE_TABLE = _affine_table()


def geometric_draws(rng, height, width):
    """The draws of the geometric pair for a height x width image, in order: the zoom's scale u in [0.5, 1.5) (float64, cast to
    float32, min with 1; the target shape is the float32 product truncated), then the affine index rnd in [0, 729).
    Returns (th, tw, rnd); (th, tw) == (height, width) -- about half of the draws -- means no zoom."""
    scale = min(np.float32(rng.uniform(0.5, 1.5)), np.float32(1))
    th, tw = int(scale * np.float32(height)), int(scale * np.float32(width))
    return th, tw, int(rng.integers(0, 729))


def zoom_in_out(image, th, tw):
    """_random_zoom_in_out with the target shape given: resize down to th x tw and back up, both TF-1.x bilinear
    (_decode_worker.resize_window); the same shape is the identity, as in TF."""
    from ._decode_worker import resize_window
    h, w = image.shape[:2]
    return resize_window(resize_window(image, th, tw), h, w)


def affine_warp(image, coef):
    """tf.contrib.image.transform(image, coef + [0, 0], 'BILINEAR') as the TF-1.x kernel computes it, in float32 with every
    operation rounded on its own: output pixel (x, y) reads (sx, sy) = ((a0 x + a1 y) + a2, (b0 x + b1 y) + b2); with
    f = floor, c = f + 1:  top = (cx - sx) R(fy, fx) + (sx - fx) R(fy, cx), bot the same on row cy,
    out = (cy - sy) top + (sy - fy) bot;  R is 0 outside the image."""
    h, w, _ = image.shape
    a0, a1, a2, b0, b1, b2 = (np.float32(v) for v in coef)
    x = np.arange(w, dtype=np.float32)[None, :]
    y = np.arange(h, dtype=np.float32)[:, None]
    sx = (a0 * x + a1 * y) + a2
    sy = (b0 * x + b1 * y) + b2
    fx, fy = np.floor(sx), np.floor(sy)
    cx, cy = fx + np.float32(1), fy + np.float32(1)

    def read(yy, xx):
        ok = (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)          # false for NaN as well
        yi = np.where(ok, yy, 0).astype(np.int64)
        xi = np.where(ok, xx, 0).astype(np.int64)
        return np.where(ok[:, :, None], image[yi, xi], np.float32(0))
    wl, wr = (cx - sx)[:, :, None], (sx - fx)[:, :, None]
    top = wl * read(fy, fx) + wr * read(fy, cx)
    bot = wl * read(cy, fx) + wr * read(cy, cx)
    out = (cy - sy)[:, :, None] * top + (sy - fy)[:, :, None] * bot
    assert out.dtype == np.float32
    return out


def geometric_augmentation(image, rng):
    """zoom, then affine, from draws taken here (u, then rnd)"""
    th, tw, rnd = geometric_draws(rng, image.shape[0], image.shape[1])
    return affine_warp(zoom_in_out(np.ascontiguousarray(image, dtype=np.float32), th, tw), AFFINE_TABLE[rnd])
