"""Worker-process side of the input pipeline (tf_face_toolbox_amd/data.py): decode (or the row of a pre-decoded image pack, packs.py)
+ resize + crop + flip / augmentation + normalise of ONE image, written straight into a shared batch buffer.  Imports numpy and PIL only -- a worker process
(started as `python -m tf_face_toolbox_amd._decode_worker`) never loads torch or touches the GPU.  Mirrors data.py:206-223 of the reference (the tf.data map function)."""
from collections import namedtuple

import numpy as np

_RESIZE_TABLES = {}
_SHM = {}


def _resize_table(n_in, n_out):
    """Source rows / lerp weights of TF-1.x ResizeBilinear with align_corners=False (the default of
    tf.image.resize_images, data.py:213): in = out * (n_in / n_out) -- NO half-pixel centres in TF 1.x --
    low = floor(in), high = min(low + 1, n_in - 1), weight of `high` = in - low, all in float32 like the TF kernel."""
    key = (n_in, n_out)
    t = _RESIZE_TABLES.get(key)
    if t is None:
        pos = np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))
        lo = np.floor(pos).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        t = _RESIZE_TABLES[key] = (lo, hi, (pos - lo).astype(np.float32))
    return t


_S255 = np.float32(1.0 / 255.0)


def resize_window(image, height, width, y0=0, win_h=None, x0=0, win_w=None):
    """Rows [y0, y0 + win_h) x columns [x0, x0 + win_w) of tf.image.resize_images(image, [height, width]) as TF 1.x computes it
    on a float32 HWC image: bilinear, align_corners=False, no antialiasing (PIL's BILINEAR widens its kernel when shrinking and
    gives different pixels), float32 arithmetic in the kernel's own order -- the two neighbours of a row are blended along x
    first, then the two rows along y.  `image` may be uint8: it is scaled by 1/255 (convert_image_dtype) on the way, element
    by element, i.e. to exactly the values a conversion of the whole image would give.  Only the window is computed: a
    random crop of the resized image costs the crop's area, not the image's (the pipeline's second largest cost after the
    JPEG decode).  Same size and a full window -> the (converted) image itself (TF skips the op)."""
    h, w = image.shape[:2]
    win_h = height if win_h is None else win_h
    win_w = width if win_w is None else win_w
    u8 = image.dtype == np.uint8
    if (h, w) == (height, width):
        out = image[y0:y0 + win_h, x0:x0 + win_w]
        return out.astype(np.float32) * _S255 if u8 else out
    ylo, yhi, yw = (t[y0:y0 + win_h] for t in _resize_table(h, height))
    xlo, xhi, xw = (t[x0:x0 + win_w] for t in _resize_table(w, width))

    s = _S255 if u8 else None

    def blend_x(rows):                                            # rows: the gathered source rows, [win_h, w, c]
        left, right = np.take(rows, xlo, axis=1), np.take(rows, xhi, axis=1)
        if u8:
            left = left.astype(np.float32); left *= s
            right = right.astype(np.float32); right *= s
        right -= left
        right *= xw3
        right += left
        return right
    xw3 = xw[None, :, None]
    top = blend_x(image[ylo])
    bot = blend_x(image[yhi])
    bot -= top
    bot *= yw[:, None, None]
    bot += top
    return bot


def resize_bilinear_tf1(image, height, width):
    """tf.image.resize_images(image, [height, width]) of TF 1.x (see resize_window)."""
    return resize_window(image, height, width)


def _load(path, num_channels):
    """tf.read_file + decode_jpeg(channels): uint8 HWC"""
    from PIL import Image
    img = Image.open(path)
    img = img.convert('RGB' if num_channels == 3 else 'L')
    a = np.asarray(img, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], num_channels)


_PACKS = {}


def _pack(pack):
    """The ImagePack a task names by its file path, memory-mapped once per process and cached (as _SHM caches the batch
    buffers); an ImagePack (the loader's own, in-process use) or None is passed through."""
    if pack is None or not isinstance(pack, str):
        return pack
    p = _PACKS.get(pack)
    if p is None:
        from .packs import ImagePack
        p = _PACKS[pack] = ImagePack(pack)
    return p


def _image(path, num_channels, pack=None):
    """the decoded uint8 HWC image of an item: _load(path) of a file, or -- `path` an int -- that row of the pack"""
    if isinstance(path, str):
        return _load(path, num_channels)
    pack = _pack(pack)
    if pack is None:
        raise ValueError('row index %r without a pack' % (path,))
    if pack.shape[2] != num_channels:
        raise ValueError('%s holds %d-channel images, the loader asks for %d' % (pack.path, pack.shape[2], num_channels))
    if not 0 <= path < pack.num_rows:
        raise ValueError('%s has no row %d' % (pack.path, path))
    return pack.image(path)


def _window(raw, landmarks, path, height, width, y0=0, win_h=None, x0=0, win_w=None):
    """The window of the resized height x width image (resize_window) or, with landmarks, of the aligned one in its place
    (preprocessing.aligned_image; a refusal names the image)."""
    if landmarks is None:
        return resize_window(raw, height, width, y0, win_h, x0, win_w)
    from .preprocessing import aligned_image
    try:
        return aligned_image(raw, landmarks, height, width, y0, win_h, x0, win_w)
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))


def decode(path, num_channels, height, width, landmarks=None, pack=None):
    """tf.read_file + decode_jpeg(channels) + convert_image_dtype(float32) + resize_images (data.py:208-213).  landmarks (10
    numbers): five-point alignment to height x width in place of the resize.  pack: `path` is a row of that image pack."""
    return _window(_image(path, num_channels, pack), landmarks, path, height, width)


GEO_WITH_LANDMARKS = ('the geometric augmentation (augmentation & 2) is not available together with landmarks: the aligned '
                      'transform supports augmentation 0 and 1')


def _crop_corner(rng, input_height, input_width, crop_height, crop_width):
    """the first draws of an example: (y0, x0) of tf.random_crop, or (0, 0) and no draw without a crop"""
    if crop_height == -1 or crop_width == -1:
        return 0, 0
    y0 = int(rng.integers(0, input_height - crop_height + 1))
    return y0, int(rng.integers(0, input_width - crop_width + 1))


def _finish(raw, input_height, input_width, crop_height, crop_width, augmentation, rng, landmarks=None, path=None):
    if landmarks is not None and augmentation & 2:                  # alignment replaces the resize; the draws are the same
        raise ValueError(GEO_WITH_LANDMARKS)
    cropped = crop_height != -1 and crop_width != -1
    y0, x0 = _crop_corner(rng, input_height, input_width, crop_height, crop_width)
    # tf.random_crop: only the cropped window is resized (aligned)
    image = _window(raw, landmarks, path, input_height, input_width, y0, crop_height if cropped else None, x0, crop_width if cropped else None)
    if augmentation & 2:                                            # the geometric pair: zoom, then affine (draws u, rnd)
        from .preprocessing import geometric_augmentation
        image = geometric_augmentation(image, rng)
    if augmentation & 1:
        from .preprocessing import data_augmentation
        image = data_augmentation(image, rng)
    elif rng.random() < 0.5:                                        # tf.image.random_flip_left_right
        image = image[:, ::-1, :]
    return (np.ascontiguousarray(image, dtype=np.float32) - 0.5) / 0.5


def train_example(path, num_channels, input_height, input_width, crop_height, crop_width, augmentation, rng, landmarks=None, pack=None):
    return _finish(_image(path, num_channels, pack), input_height, input_width, crop_height, crop_width, augmentation, rng, landmarks, path)


HEADER_BYTES = 64            # per raw slot: the 16 words below + padding (include/fte.h: fte_preprocess_u8, _aug, _geo)
ALIGN_HEADER_BYTES = 128     # per ALIGNED raw slot: the same 16 words with h0, w0 = the shape of the source window, the inverse
#                              similarity in words 16..21, words 22..31 = 0 (include/fte.h: fte_preprocess_u8_align)
# The header's fields as words of its int32 view -- fte.h's layout, named here once:
W_MODE, W_H0, W_W0, W_Y0, W_X0, W_FLIP, W_FLAGS = range(7)
W_COLOUR = slice(7, 10)      # float32 bits: brightness delta, hue delta, saturation factor
W_GEO = slice(10, 13)        # th, tw (the zoom's target shape), rnd (the affine index)
W_M6 = slice(16, 22)         # float32 bits: (a0, a1, a2, b0, b1, b2) of an aligned slot


def slot_header(hd, h0, w0, num_channels, input_height, input_width, crop_height, crop_width, rng, augmentation=0, m6=None):
    """The header words of a mode-0 raw slot into hd (int32 [16]; aligned: [32], with the inverse similarity m6 for words 16..21):
    {0, h0, w0, y0, x0, flip}, then the draws of train_example() for the seeded `rng`, taken in its order -- crop corner, the
    geometric pair (words 6, 10..12), the colour augmentation (words 6..9) or the flip -- and zeros.  rng None: the evaluation
    transform (full window, no flip).  The ONE place that draws for a raw slot: slots of decoded files, aligned slots, slots of
    pack rows and the header-only slots of a resident pack all come through here."""
    hd[:] = 0
    y0 = x0 = flip = 0
    if rng is not None:
        y0, x0 = _crop_corner(rng, input_height, input_width, crop_height, crop_width)
        if augmentation & 2:
            from .preprocessing import AFFINE, ZOOM, geometric_draws
            out_h, out_w = (crop_height, crop_width) if crop_height != -1 and crop_width != -1 else (input_height, input_width)
            th, tw, rnd = geometric_draws(rng, out_h, out_w)
            hd[W_FLAGS] = AFFINE | (ZOOM if (th, tw) != (out_h, out_w) else 0)
            hd[W_GEO] = (th, tw, rnd)
        if augmentation & 1:
            from .preprocessing import augmentation_draws
            flip, flags, brightness, hue, saturation = augmentation_draws(rng, num_channels)
            hd[W_FLAGS] |= flags
            hd[W_COLOUR].view(np.float32)[:] = (brightness, hue, saturation)
        else:
            flip = int(rng.random() < 0.5)
    hd[:W_FLAGS] = (0, h0, w0, y0, x0, flip)
    if m6 is not None:
        hd[W_M6].view(np.float32)[:] = m6


def raw_example(slot, path, num_channels, input_height, input_width, crop_height, crop_width, rng, augmentation=0, landmarks=None,
                pack=None, header_only=False):
    """The DECODED image and the draws of train_example() (seeded the same way, drawn in the same order) into one slot of a raw
    batch buffer -- resize / crop / flip / normalise then run on the GPU (fte_preprocess_u8) and give the bits train_example()
    gives.  rng None: the evaluation transform (full window, no flip).  An image too large for its slot is transformed here
    and stored finished (mode 1).  augmentation: the draws of preprocessing.data_augmentation as well (header words 6..9: flag
    bits and the float32 brightness delta, hue delta and saturation factor), applied on the GPU by fte_preprocess_u8_aug.
    augmentation & 2: the geometric pair's draws too (word 6 bits 8 = zoom applied, 16 = affine; words 10..12 = the zoom's target
    shape th, tw and the affine index rnd), applied by fte_preprocess_u8_geo.  landmarks (10 numbers): an ALIGNED slot instead --
    a 128-byte header, then the WINDOW of the decoded image that the aligned image reads (preprocessing.align_window) with the
    inverse similarity relative to it; fte_preprocess_u8_align warps, flips, colours and normalises.
    pack (an image pack or its file path): `path` is a row index and the slot gets that row, all row_stride bytes of it, where a
    file's decoded pixels would go.  header_only: the 64 header bytes alone (h0, w0 = the pack's image shape) -- the rows of a
    pack resident on the GPU are put behind them there (fte_pack_gather_slots)."""
    header, m6 = HEADER_BYTES, None
    if pack is not None and landmarks is not None:
        raise ValueError('landmarks together with a pack: a pack is aligned when it is made, its rows are not aligned again')
    if pack is not None:
        pack = _pack(pack)
        raw = _image(path, num_channels, pack)                      # checks the row and the channels; a view, nothing is read yet
        body = None if header_only else pack.rows[path]
    elif landmarks is None:
        body = raw = _load(path, num_channels)
    else:
        from .preprocessing import align_window
        if augmentation & 2:
            raise ValueError(GEO_WITH_LANDMARKS)
        header, raw = ALIGN_HEADER_BYTES, _load(path, num_channels)
        try:
            wy0, wx0, wh, ww, m6 = align_window(landmarks, raw.shape[0], raw.shape[1], input_height, input_width)
        except ValueError as e:
            raise ValueError('%s: %s' % (path, e))
        body = raw[wy0:wy0 + wh, wx0:wx0 + ww]
    hd = slot[:header].view(np.int32)
    if body is not None and body.size > slot.size - header:         # does not fit: finished on the host, mode 1
        if rng is None:
            image = (_window(raw, landmarks, path, input_height, input_width) - np.float32(0.5)) / np.float32(0.5)
        else:
            image = _finish(raw, input_height, input_width, crop_height, crop_width, augmentation, rng, landmarks, path)
        slot[header:header + image.size * 4] = np.ascontiguousarray(image, dtype=np.float32).reshape(-1).view(np.uint8)
        cropped = crop_height != -1 and crop_width != -1
        hd[:] = 0
        hd[:W_FLAGS] = (1,) + ((crop_height, crop_width) if cropped else (input_height, input_width)) + (0, 0, 0)
        return
    h0, w0 = (raw if m6 is None else body).shape[:2]
    slot_header(hd, h0, w0, num_channels, input_height, input_width, crop_height, crop_width, rng, augmentation, m6)
    if body is not None:
        slot[header:header + body.size] = body.reshape(-1)


def _buffer(name, shape, dtype):
    """The shared batch buffer a task names: anonymous shared memory behind the file DESCRIPTOR this process inherited from the
    parent (data._WorkerPool: memfd_create + pass_fds), or a file path."""
    batch = _SHM.get(name)
    if batch is None or batch.shape != tuple(shape) or batch.dtype != dtype:
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if isinstance(name, int):
            import mmap
            mm = mmap.mmap(name, nbytes)
            batch = _SHM[name] = np.frombuffer(mm, dtype=dtype).reshape(tuple(shape))
        else:
            batch = _SHM[name] = np.memmap(name, dtype=dtype, mode='r+', shape=tuple(shape))
    return batch


Task = namedtuple('Task', 'buffer shape rows num_channels in_h in_w crop_h crop_w augmentation raw pack header_only',
                  defaults=(0, None, False))


def fill_rows(task):
    """A Task, or the bare tuple of its fields in order (raw, pack, header_only may be left off): decode the listed images
    rows = [(row, path, seed), ...] (seed None: the evaluation transform) into rows of the shared batch buffer -- a
    float32 array of finished examples, or with raw = 1 a uint8 array [rows, slot bytes] of decoded images + draws (the colour
    augmentation's included) for the GPU transform.  A row may carry a fourth item, the image's 10 landmark numbers: it is aligned
    instead of resized (an aligned raw slot has the 128-byte header).  With a pack path (packs.py) a row's `path` is an int, the
    row of that pack, read where a file would have been decoded; header_only: raw slots of 64 bytes, the draws alone.  Returns
    the number of rows written (errors propagate)."""
    t = Task(*task)
    more = {} if t.pack is None else {'pack': _pack(t.pack)}
    size = (t.num_channels, t.in_h, t.in_w)
    if t.raw:
        if t.header_only:
            more['header_only'] = True
        batch = _buffer(t.buffer, t.shape, np.uint8)
        for row, path, seed, *lm in t.rows:
            raw_example(batch[row], path, *size, t.crop_h, t.crop_w, None if seed is None else np.random.default_rng(seed),
                        t.augmentation, *lm, **more)
        return len(t.rows)
    batch = _buffer(t.buffer, t.shape, np.float32)
    for row, path, seed, *lm in t.rows:
        if seed is None:                          # evaluation: decode + resize + normalise, nothing random (data.py:153-191)
            batch[row] = (decode(path, *size, *lm, **more) - np.float32(0.5)) / np.float32(0.5)
        else:
            batch[row] = train_example(path, *size, t.crop_h, t.crop_w, t.augmentation, np.random.default_rng(seed), *lm, **more)
    return len(t.rows)


def main():
    """Worker loop: length-prefixed pickled tasks on stdin, one ('ok', rows) / ('err', text) reply each on stdout."""
    import pickle
    import struct
    import sys
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    while True:
        hdr = inp.read(4)
        if len(hdr) < 4:
            return
        task = pickle.loads(inp.read(struct.unpack('<I', hdr)[0]))
        try:
            msg = ('ok', fill_rows(task))
        except BaseException as e:               # noqa: B902 -- reported to the parent, which raises it in the training thread
            msg = ('err', '%s: %s' % (type(e).__name__, e))
        b = pickle.dumps(msg)
        out.write(struct.pack('<I', len(b)) + b)
        out.flush()


if __name__ == '__main__':
    main()
