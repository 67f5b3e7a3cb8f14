"""Plain per-pixel restatement of the loader's colour augmentation (fte_preprocess_u8_aug, include/fte.h), written from the
contract with np.float32 scalars -- one rounding per operation, numpy's floor-mod for `%` -- independently of the array code in
tf_face_toolbox_amd/preprocessing.py and of the kernel.  Shared by tests/test_augment_host.py and tests/test_gpu_augment.py,
with the seed list and the hand-built "edge" slots both use."""
import numpy as np

F = np.float32
SEEDS = list(range(7, 71))                      # 64 seeds: every flag combination occurs for every geometry (asserted by the tests)
GEOMS = [(120, 116, 112, 112), (128, 128, 112, 112), (112, 96, -1, -1), (37, 29, 32, 24), (300, 280, 224, 224)]    # test_gpu_loader.py's


def _clip01(x):
    return min(max(x, F(0)), F(1))


def rgb_to_hsv(r, g, b):
    mx, mn = max(r, g, b), min(r, g, b)
    d = mx - mn
    s = d / mx if mx > 0 else F(0)
    dz = d if d > 0 else F(1)
    if mx == r:
        h = (g - b) / dz % F(6)
    elif mx == g:
        h = (b - r) / dz + F(2)
    else:
        h = (r - g) / dz + F(4)
    h = h / F(6)
    return (h if d > 0 else F(0)), s, mx


def hsv_to_rgb(h, s, v):
    h6 = h * F(6)
    c = v * s
    x = c * (F(1) - abs(h6 % F(2) - F(1)))
    i = int(np.floor(h6)) % 6
    z = F(0)
    r, g, b = [(c, x, z), (x, c, z), (z, c, x), (z, x, c), (x, z, c), (c, z, x)][i]
    m = v - c
    return r + m, g + m, b + m


def hue_after_shift(h, delta):
    return (h + (-delta)) % F(1)


def pixel(v, flags, brightness, hue, saturation):
    """one pixel (1 or 3 float32 values in [0, 1], resized / cropped / flipped) -> its normalised, augmented values"""
    v = [F(x) for x in v]
    assert all(type(x) is np.float32 for x in (brightness, hue, saturation))
    if flags & 1:
        v = [x - brightness for x in v]
    if len(v) == 3:
        if flags & 2:
            h, s, val = rgb_to_hsv(*[_clip01(x) for x in v])
            v = hsv_to_rgb(hue_after_shift(h, hue), s, val)
        if flags & 4:
            h, s, val = rgb_to_hsv(*[_clip01(x) for x in v])
            v = hsv_to_rgb(h, _clip01(s * saturation), val)
    out = [(x - F(0.5)) / F(0.5) for x in v]
    assert all(type(x) is np.float32 for x in out)
    return out


def header(slot):
    """(mode, h0, w0, y0, x0, flip, flags, brightness, hue, saturation) of a slot"""
    hd = slot[:64].view(np.int32)
    return tuple(int(x) for x in hd[:7]) + tuple(hd[7:10].view(np.float32))


def restate_slot(slot, ch, in_h, in_w, out_h, out_w):
    """what fte_preprocess_u8_aug computes from one slot: the host's resize of the window, then pixel() one pixel at a time"""
    from tf_face_toolbox_amd import _decode_worker as dw
    mode, h0, w0, y0, x0, flip, flags, brightness, hue, saturation = header(slot)
    if mode == 1:
        return slot[64:64 + out_h * out_w * ch * 4].view(np.float32).reshape(out_h, out_w, ch).copy()
    raw = slot[64:64 + h0 * w0 * ch].reshape(h0, w0, ch)
    img = dw.resize_window(raw, in_h, in_w, y0, out_h, x0, out_w)
    if flip:
        img = img[:, ::-1, :]
    assert img.dtype == np.float32
    out = np.empty((out_h, out_w, ch), dtype=np.float32)
    for y in range(out_h):
        for x in range(out_w):
            out[y, x] = pixel(img[y, x], flags, brightness, hue, saturation)
    return out


# ------------------------------------------------------------------ the hand-built edge image and its headers
EDGE_SIDE = 16
HUE_PIXEL = (200, 120, 40)                      # its hue is the hue delta of the edge headers, exactly and one ulp to either side
EDGE_BRIGHTNESS, EDGE_SATURATION = F(0.0625), F(0.75)
EDGE_NAMED = [(0, 0, 0), (255, 255, 255), (128, 128, 128),
              (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
              (200, 200, 50), (30, 180, 180),     # two equal maxima: r == g > b, g == b > r
              (50, 200, 200), (200, 50, 200), (7, 7, 9), (100, 100, 101), (1, 0, 0), (3, 9, 12), (12, 9, 3), (254, 255, 253),
              HUE_PIXEL]


def edge_image():
    """16 x 16 x 3 uint8: the named pixels first, seeded random colours after"""
    img = np.random.default_rng(0).integers(0, 256, (EDGE_SIDE * EDGE_SIDE, 3)).astype(np.uint8)
    img[:len(EDGE_NAMED)] = EDGE_NAMED
    return img.reshape(EDGE_SIDE, EDGE_SIDE, 3)


def hue_pixel_hue(flags):
    """hue of HUE_PIXEL at the point the hue step sees it under `flags` (after the brightness step, if any)"""
    v = [F(x) * F(1.0 / 255.0) for x in HUE_PIXEL]
    if flags & 1:
        v = [x - EDGE_BRIGHTNESS for x in v]
    return rgb_to_hsv(*[_clip01(x) for x in v])[0]


def edge_slots(ch=3):
    """24 slots of the edge image passed straight through (h0, w0 = in_h, in_w = 16: no resize, no crop): the 8 flag
    combinations x a hue delta equal to HUE_PIXEL's hue, one ulp above it and one ulp below it (the floor-mod wrap of
    h - delta: 0, a tiny negative sum that wraps to exactly 1.0, a tiny positive one); flips alternate."""
    img = edge_image() if ch == 3 else edge_image()[:, :, 1:2]
    buf = np.zeros((24, 64 + EDGE_SIDE * EDGE_SIDE * 4), dtype=np.uint8)
    for i in range(24):
        flags, k = i % 8, i // 8
        h = hue_pixel_hue(flags)
        hue = [h, np.nextafter(h, F(1)), np.nextafter(h, F(0))][k]
        hd = buf[i, :64].view(np.int32)
        hd[:7] = (0, EDGE_SIDE, EDGE_SIDE, 0, 0, (i // 4) % 2, flags)
        hd[7:10].view(np.float32)[:] = (EDGE_BRIGHTNESS, hue, EDGE_SATURATION)
        buf[i, 64:64 + img.size] = img.reshape(-1)
    return buf
