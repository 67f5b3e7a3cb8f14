"""Pre-decoded image packs (`.fpk`): one flat file of uint8 image rows of ONE shape, decoded once by pack_list.py, from which the
loader feeds in place of decoding a JPEG per image and step (data.train_inputs / eval_inputs, packed_data_path=...).  numpy
only: the decode workers import this module and must not load torch.

Layout, version 1, little-endian, every offset and count 64-bit:

    byte   0  magic        8 bytes  b'FTEPACK\\0'
           8  version      uint32   1
          12  channels     uint32   C (1 or 3)
          16  num_rows     uint64   N
          24  height       uint32   H
          28  width        uint32   W
          32  row_stride   uint64   bytes per row: a multiple of 64, >= H * W * C; the padding bytes are zero
          40  data_offset  uint64   4096: N rows of row_stride bytes (page-aligned, so that a row is 64-byte aligned in a mapping)
          48  labels_offset uint64  data_offset + N * row_stride: int32 labels[N], -1 for a list without labels
          56  paths_offset uint64   labels_offset + 4 * N: the list's paths, UTF-8, joined by '\\n'
          64  paths_bytes  uint64   the file ends at paths_offset + paths_bytes
          72  zero to byte 4096
"""
import os
import struct

import numpy as np

MAGIC = b'FTEPACK\0'
VERSION = 1
DATA_OFFSET = 4096
_HEADER = struct.Struct('<8sIIQIIQQQQQ')


def row_stride_of(height, width, channels):
    return (height * width * channels + 63) // 64 * 64


def write_pack(path, images, labels, paths):
    """Write a pack of len(paths) rows: `images` yields the uint8 [H, W, C] images in row order (an array [N, H, W, C] will do),
    labels is a sequence of N ints or None (stored as -1), paths the N strings of the list.  The file is written under a
    temporary name next to `path` and renamed, so a reader never sees half a pack.  An image of another shape than the first is
    refused by the name of its path.  Returns (N, H, W, C, row_stride)."""
    paths = [str(p) for p in paths]
    n = len(paths)
    if n < 1:
        raise ValueError('%s: a pack needs at least one image' % path)
    for p in paths:
        if '\n' in p:
            raise ValueError('%s: a path with a line break cannot be stored: %r' % (path, p))
    lab = np.full(n, -1, dtype='<i4') if labels is None else np.asarray(labels, dtype='<i4').reshape(-1)
    if lab.size != n:
        raise ValueError('%s: %d labels for %d paths' % (path, lab.size, n))
    names = '\n'.join(paths).encode('utf-8')
    tmp = '%s.tmp.%d' % (path, os.getpid())
    shape = stride = None
    done = 0
    try:
        with open(tmp, 'wb') as f:
            f.write(b'\0' * DATA_OFFSET)
            for img in images:
                img = np.asarray(img)
                if done >= n:
                    raise ValueError('%s: more images than paths (%d)' % (path, n))
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (1, 3):
                    raise ValueError('%s: %s is not a uint8 [H, W, 1 | 3] image but %s %s' % (path, paths[done], img.dtype, img.shape))
                if shape is None:
                    shape = tuple(int(v) for v in img.shape)
                    stride = row_stride_of(*shape)
                    pad = b'\0' * (stride - shape[0] * shape[1] * shape[2])
                elif tuple(img.shape) != shape:
                    raise ValueError('%s: %s decodes to %s, the images before it to %s -- a pack holds images of one shape'
                                     % (path, paths[done], 'x'.join(map(str, img.shape)), 'x'.join(map(str, shape))))
                f.write(np.ascontiguousarray(img).tobytes())
                f.write(pad)
                done += 1
            if done != n:
                raise ValueError('%s: %d images for %d paths' % (path, done, n))
            labels_offset = DATA_OFFSET + n * stride
            f.write(lab.tobytes())
            f.write(names)
            f.seek(0)
            f.write(_HEADER.pack(MAGIC, VERSION, shape[2], n, shape[0], shape[1], stride, DATA_OFFSET, labels_offset,
                                 labels_offset + 4 * n, len(names)))
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return (n,) + shape + (stride,)


class ImagePack(object):
    """A pack opened read-only: `rows` is an np.memmap [N, row_stride] of the image rows, `labels` int32 [N], `paths` the list's
    paths; shape = (H, W, C).  A file that is not a version-1 pack, or whose size is not what its header implies, is refused by
    name (ValueError)."""

    def __init__(self, path):
        self.path = os.path.abspath(os.path.expanduser(path))
        size = os.path.getsize(self.path)
        with open(self.path, 'rb') as f:
            head = f.read(_HEADER.size)
            if len(head) < _HEADER.size or head[:8] != MAGIC:
                raise ValueError('%s: not an image pack (no %r magic)' % (path, MAGIC))
            (_, version, c, n, h, w, stride, data_offset, labels_offset, paths_offset, paths_bytes) = _HEADER.unpack(head)
            if version != VERSION:
                raise ValueError('%s: pack version %d, this reader knows version %d' % (path, version, VERSION))
            if stride % 64:
                raise ValueError('%s: row stride %d is not a multiple of 64' % (path, stride))
            if n < 1 or c not in (1, 3) or h < 1 or w < 1 or stride < h * w * c or data_offset != DATA_OFFSET or \
                    labels_offset != data_offset + n * stride or paths_offset != labels_offset + 4 * n:
                raise ValueError('%s: inconsistent pack header (N %d, %d x %d x %d, stride %d, offsets %d / %d / %d)'
                                 % (path, n, h, w, c, stride, data_offset, labels_offset, paths_offset))
            if size != paths_offset + paths_bytes:
                raise ValueError('%s: the file has %d bytes, its header implies %d (%s)'
                                 % (path, size, paths_offset + paths_bytes, 'truncated' if size < paths_offset + paths_bytes else 'trailing bytes'))
            f.seek(labels_offset)
            self.labels = np.frombuffer(f.read(4 * n), dtype='<i4').astype(np.int32)
            self.paths = f.read(paths_bytes).decode('utf-8').split('\n')
        if len(self.paths) != n:
            raise ValueError('%s: %d paths for %d rows' % (path, len(self.paths), n))
        self.num_rows, self.shape, self.row_stride, self.data_offset = n, (h, w, c), stride, data_offset
        self.rows = np.memmap(self.path, dtype=np.uint8, mode='r', offset=data_offset, shape=(n, stride))
        self.has_labels = bool((self.labels >= 0).all())

    def __len__(self):
        return self.num_rows

    def image(self, row):
        """the uint8 [H, W, C] image of a row (a view of the mapping)"""
        h, w, c = self.shape
        return self.rows[row, :h * w * c].reshape(h, w, c)

    def describe(self):
        return '%s: %d images of %d x %d x %d, row stride %d, %.1f MB' % ((self.path, self.num_rows) + self.shape
                                                                           + (self.row_stride, self.num_rows * self.row_stride / 1e6))
