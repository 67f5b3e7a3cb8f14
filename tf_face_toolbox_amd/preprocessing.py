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
    out = (cy - sy) top + (sy - fy) bot;  R is 0 outside the image.  The host's one warp formula, over the whole image: align_warp
    (its none-of-four-taps rule gives the +0 this formula gives for the table's finite coordinates)."""
    return align_warp(image, coef, image.shape[0], image.shape[1])


def geometric_augmentation(image, rng):
    """zoom, then affine, from draws taken here (u, then rnd)"""
    th, tw, rnd = geometric_draws(rng, image.shape[0], image.shape[1])
    return affine_warp(zoom_in_out(np.ascontiguousarray(image, dtype=np.float32), th, tw), AFFINE_TABLE[rnd])


# ------------------------------------------------------------------ five-point alignment (not in the reference)
# The template of ArcFace's norm_crop for a 112 x 112 crop: (x, y) of left eye, right eye, nose, left and right mouth corner,
# pixel centres at integer coordinates (the cv2.warpAffine convention).
ALIGN_TEMPLATE_112 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]],
                              dtype=np.float64)


def align_template(in_h, in_w):
    """The template for an in_h x in_w crop: scaled by s = in_h / 112 and centred along x.  112 x 96: the SphereFace template
    (x - 8); 112 x 112: ALIGN_TEMPLATE_112 itself."""
    s = in_h / 112.0
    t = ALIGN_TEMPLATE_112 * s
    t[:, 0] += (in_w - 112.0 * s) / 2.0
    return t


def similarity_from_landmarks(src5, dst5):
    """The least-squares non-reflective similarity that maps src to dst, as a float64 [2, 3] matrix [[a, -b, tx], [b, a, ty]]:
    with centred points p (src) and q (dst), a = sum(p . q) / sum|p|^2, b = sum(p x q) / sum|p|^2, t = mean(q) - M mean(p).
    Points that (nearly) coincide have no similarity: ValueError."""
    src = np.asarray(src5, dtype=np.float64).reshape(-1, 2)
    dst = np.asarray(dst5, dtype=np.float64).reshape(-1, 2)
    ms, md = src.mean(0), dst.mean(0)
    p, q = src - ms, dst - md
    den = (p * p).sum()
    if not den >= 1e-12 * max(1.0, (ms * ms).sum()):              # (a NaN landmark is refused here too)
        raise ValueError('landmarks coincide (spread %g): no similarity maps them to the template' % den)
    a = (p * q).sum() / den
    b = (p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum() / den
    m = np.array([[a, -b], [b, a]])
    return np.concatenate([m, (md - m @ ms)[:, None]], 1)


def align_window(landmarks, h0, w0, in_h, in_w):
    """(wy0, wx0, wh, ww, m6) for an h0 x w0 image with the given five landmarks (10 numbers, source pixels): the window of the
    image that the aligned in_h x in_w crop can read -- the bounding box of the crop's four corners under the INVERSE similarity
    (float64), padded by 2 pixels and clamped to the image -- and the float32 inverse (a0, a1, a2, b0, b1, b2), its translation
    relative to the window's corner (subtracted in float64, then rounded): aligned pixel (x, y) reads the window at
    (a0 x + a1 y + a2, b0 x + b1 y + b2).  No intersection: a 1 x 1 window at (0, 0), which the warp leaves nearly everywhere.
    The window is part of the definition on the host and on the GPU: it is what lets a large frame with a small face fit a
    raw slot."""
    fwd = similarity_from_landmarks(landmarks, align_template(in_h, in_w))
    a, b = fwd[0, 0], fwd[1, 0]
    det = a * a + b * b
    if not (det > 0.0 and np.isfinite(det)):
        raise ValueError('the similarity from the landmarks to the template is singular (scale^2 = %g)' % det)
    inv = np.array([[a, b], [-b, a]]) / det
    t = -inv @ fwd[:, 2]
    corners = np.array([[0, 0], [in_w - 1, 0], [0, in_h - 1], [in_w - 1, in_h - 1]], dtype=np.float64)
    src = corners @ inv.T + t
    if not np.isfinite(src).all():
        raise ValueError('the similarity from the landmarks to the template is singular (scale^2 = %g)' % det)
    x_lo, y_lo = np.floor(src.min(0)) - 2
    x_hi, y_hi = np.ceil(src.max(0)) + 2
    x_lo, y_lo, x_hi, y_hi = max(x_lo, 0), max(y_lo, 0), min(x_hi, w0 - 1), min(y_hi, h0 - 1)
    if x_lo > x_hi or y_lo > y_hi:
        wy0, wx0, wh, ww = 0, 0, 1, 1
    else:
        wy0, wx0, wh, ww = int(y_lo), int(x_lo), int(y_hi - y_lo) + 1, int(x_hi - x_lo) + 1
    m6 = np.array([inv[0, 0], inv[0, 1], t[0] - wx0, inv[1, 0], inv[1, 1], t[1] - wy0]).astype(np.float32)
    return wy0, wx0, wh, ww, m6


def align_warp(window, m6, in_h, in_w, y0=0, win_h=None, x0=0, win_w=None):
    """Rows [y0, y0 + win_h) x columns [x0, x0 + win_w) of the aligned in_h x in_w image, warped from `window` (float32 in [0, 1],
    HWC: the source window of align_window, converted as _decode_worker._load's image is) by affine_warp's formula: aligned pixel
    (x, y) reads (sx, sy) = ((a0 x + a1 y) + a2, (b0 x + b1 y) + b2); with f = floor, c = f + 1:
    top = (cx - sx) R(fy, fx) + (sx - fx) R(fy, cx), bot the same on row cy, out = (cy - sy) top + (sy - fy) bot; R is 0 outside the
    window.  Float32, every operation rounded on its own.  A pixel NONE of whose four taps lies inside the window is 0: what the
    formula gives whenever the coordinates are finite, and the rule for the others (include/fte.h: fte_preprocess_u8_align)."""
    h, w, _ = window.shape
    win_h = in_h if win_h is None else win_h
    win_w = in_w if win_w is None else win_w
    a0, a1, a2, b0, b1, b2 = (np.float32(v) for v in m6)
    x = np.arange(x0, x0 + win_w).astype(np.float32)[None, :]
    y = np.arange(y0, y0 + win_h).astype(np.float32)[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        sx = (a0 * x + a1 * y) + a2
        sy = (b0 * x + b1 * y) + b2
        fx, fy = np.floor(sx), np.floor(sy)
        cx, cy = fx + np.float32(1), fy + np.float32(1)
        xl, xr = (fx >= 0) & (fx <= w - 1), (cx >= 0) & (cx <= w - 1)          # false for NaN as well
        yt, yb = (fy >= 0) & (fy <= h - 1), (cy >= 0) & (cy <= h - 1)

        def read(yy, xx, ok):
            yi = np.where(ok, yy, 0).astype(np.int64)
            xi = np.where(ok, xx, 0).astype(np.int64)
            return np.where(ok[:, :, None], window[yi, xi], np.float32(0))
        wl, wr = (cx - sx)[:, :, None], (sx - fx)[:, :, None]
        top = wl * read(fy, fx, yt & xl) + wr * read(fy, cx, yt & xr)
        bot = wl * read(cy, fx, yb & xl) + wr * read(cy, cx, yb & xr)
        out = (cy - sy)[:, :, None] * top + (sy - fy)[:, :, None] * bot
    out = np.where(((yt | yb) & (xl | xr))[:, :, None], out, np.float32(0))
    assert out.dtype == np.float32
    return out


def aligned_image(raw, landmarks, in_h, in_w, y0=0, win_h=None, x0=0, win_w=None):
    """The host aligned transform up to the flip: decoded uint8 HWC image + landmarks -> the float32 [0, 1] window
    [y0, y0 + win_h) x [x0, x0 + win_w) of the aligned in_h x in_w image."""
    wy0, wx0, wh, ww, m6 = align_window(landmarks, raw.shape[0], raw.shape[1], in_h, in_w)
    window = raw[wy0:wy0 + wh, wx0:wx0 + ww].astype(np.float32) * np.float32(1.0 / 255.0)
    return align_warp(window, m6, in_h, in_w, y0, win_h, x0, win_w)


def read_landmarks(landmark_list_path, image_paths):
    """The landmark file (`path x1 y1 ... x5 y5` per line: source pixels of left eye, right eye, nose, left and right mouth
    corner) as a float32 [len(image_paths), 10] array in the order of image_paths.  ValueError for a malformed line (its number)
    and for listed images without landmarks (the first one and how many)."""
    import os
    table = {}
    with open(os.path.expanduser(landmark_list_path), 'r') as f:
        for num, line in enumerate(f, 1):
            part = line.split()
            if not part:
                continue
            try:
                vals = np.asarray([float(v) for v in part[1:]], dtype=np.float32)
            except ValueError:
                vals = None
            if vals is None or vals.size != 10 or not np.isfinite(vals).all():
                raise ValueError('%s, line %d: expected `path x1 y1 x2 y2 x3 y3 x4 y4 x5 y5`' % (landmark_list_path, num))
            table[part[0]] = vals
    missing = [p for p in image_paths if p not in table]
    if missing:
        raise ValueError('%s has no landmarks for %d of the %d listed images, the first being %s'
                         % (landmark_list_path, len(missing), len(image_paths), missing[0]))
    out = np.empty((len(image_paths), 10), dtype=np.float32)
    for i, p in enumerate(image_paths):
        out[i] = table[p]
    return out
