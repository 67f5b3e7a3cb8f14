#!/usr/bin/env python
"""pack_list.py -- decode a list's images ONCE into an image pack (tf_face_toolbox_amd/packs.py, `.fpk`): a flat file of uint8 rows
that train.py / evaluate.py --packed_data_path read in place of decoding a JPEG per image and step.  Host only (numpy + PIL, as
the decode workers): no GPU.

    python pack_list.py --data_list_path L --out P.fpk [--is_color 1]
                        [--landmark_list_path LM --input_height H --input_width W] [--resize_height H --resize_width W]

Row k is the image of the list's k-th entry, its label the entry's label (-1 for a list of paths only).

* Plain: the row is the uint8 image a decode worker produces for the path, byte for byte.  LOSSLESS: a loader fed from the pack
  delivers the batches of the list, bit for bit.  All images must decode to one shape; the first that differs is named.
* --landmark_list_path: the row is the five-point aligned H x W crop, round(255 x) of the host aligned image -- the bytes align.py
  stores in its PNGs.  (Training from such a pack equals training from align.py's PNG list, not from the landmarks: the rounding
  to uint8 happens here.)
* --resize_height / --resize_width, for lists of mixed sizes: the row is round(255 x) of the loader's own bilinear resize to
  H x W.  THIS QUANTISES: the loader resizes in float32 and never rounds to bytes, so a pack made with --resize_* is NOT bit-equal
  to training from the list.

The decode runs in worker processes, at most data.usable_cpus() of them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser(description='Decode the images of a list once into an image pack (.fpk).')
    parser.add_argument('--data_list_path', type=str, required=True, help='`path` or `path label` per line.')
    parser.add_argument('--out', type=str, required=True, help='The pack to write (suggested suffix .fpk); written under a temporary name and renamed.')
    parser.add_argument('--is_color', type=int, default=1, help='Whether to read inputs as RGB images.')
    parser.add_argument('--landmark_list_path', type=str, default=None,
                        help='`path x1 y1 ... x5 y5` per line: rows are the five-point aligned --input_height x --input_width crops, '
                             'the bytes align.py writes (round(255 x) of the aligned image).')
    parser.add_argument('--input_height', type=int, default=112, help='Height of the aligned crop (--landmark_list_path).')
    parser.add_argument('--input_width', type=int, default=112, help='Width of the aligned crop (--landmark_list_path).')
    parser.add_argument('--resize_height', type=int, default=-1,
                        help='With --resize_width, for lists of mixed sizes: rows are round(255 x) of the bilinear resize to this shape.  '
                             'This QUANTISES: such a pack is NOT bit-equal to training from the list.  Without it (and without '
                             'landmarks) nothing is lossy.')
    parser.add_argument('--resize_width', type=int, default=-1, help='See --resize_height.')
    parser.add_argument('--workers', type=int, default=-1, help='Decode processes; default and upper bound: the usable CPUs.  0 = in this process.')
    return parser


def resized_u8(path, num_channels, height, width):
    """round(255 x) of the loader's resize x in [0, 1] of a decoded image, uint8 HWC"""
    from tf_face_toolbox_amd import _decode_worker as dw
    x = dw.resize_window(dw._load(path, num_channels), height, width)
    return np.clip(np.rint(x.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)


def _row(job):
    """one row's image; runs in a worker process.  job = (mode, path, channels, height, width, landmarks)"""
    mode, path, num_channels, height, width, lm = job
    if mode == 'align':
        from align import aligned_u8
        return aligned_u8(path, np.asarray(lm, dtype=np.float32), num_channels, height, width)
    if mode == 'resize':
        return resized_u8(path, num_channels, height, width)
    from tf_face_toolbox_amd import _decode_worker as dw
    return dw._load(path, num_channels)


def main(argv=None):
    FLAGS = build_parser().parse_args(argv)
    from tf_face_toolbox_amd import packs
    from tf_face_toolbox_amd.data import _list_entries, usable_cpus
    resize = FLAGS.resize_height != -1 or FLAGS.resize_width != -1
    if resize and (FLAGS.resize_height < 1 or FLAGS.resize_width < 1):
        raise SystemExit('--resize_height and --resize_width go together and are positive')
    if resize and FLAGS.landmark_list_path is not None:
        raise SystemExit('--resize_height / --resize_width together with --landmark_list_path: the aligned crop has its own shape '
                         '(--input_height x --input_width)')
    entries = _list_entries(FLAGS.data_list_path)
    if not entries:
        raise SystemExit('%s lists no images' % FLAGS.data_list_path)
    paths = [e[0] for e in entries]
    labelled = [len(e) > 1 for e in entries]
    if any(labelled) and not all(labelled):
        raise SystemExit('%s: some lines carry a label and some do not' % FLAGS.data_list_path)
    labels = [int(e[1]) for e in entries] if all(labelled) else None
    num_channels = 3 if FLAGS.is_color else 1
    if FLAGS.landmark_list_path is not None:
        from tf_face_toolbox_amd.preprocessing import read_landmarks
        lms = read_landmarks(FLAGS.landmark_list_path, paths)
        jobs = [('align', p, num_channels, FLAGS.input_height, FLAGS.input_width, tuple(lm.tolist())) for p, lm in zip(paths, lms)]
    elif resize:
        jobs = [('resize', p, num_channels, FLAGS.resize_height, FLAGS.resize_width, None) for p in paths]
    else:
        jobs = [('load', p, num_channels, 0, 0, None) for p in paths]
    workers = usable_cpus() if FLAGS.workers < 0 else min(FLAGS.workers, usable_cpus())
    workers = min(workers, len(jobs))
    t0 = time.time()
    pool = None
    try:
        if workers > 1:
            from concurrent.futures import ProcessPoolExecutor
            import multiprocessing
            pool = ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context('spawn'))
            images = pool.map(_row, jobs, chunksize=max(1, min(64, len(jobs) // (4 * workers))))
        else:
            images = (_row(j) for j in jobs)
        try:
            n, h, w, c, stride = packs.write_pack(FLAGS.out, images, labels, paths)
        except ValueError as e:                    # an image of another shape (named by its path), an unreadable header, ...
            raise SystemExit('pack_list.py: %s%s' % (e, '' if resize or FLAGS.landmark_list_path else
                                                     ' (--resize_height / --resize_width packs a list of mixed sizes, lossily)'))
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
    mode = 'aligned crops (rounded to uint8)' if FLAGS.landmark_list_path else 'resized, QUANTISED to uint8' if resize else 'lossless'
    print('%d images of %d x %d x %d packed into %s in %.1f s: %s, row stride %d, %d bytes, labels %s, %d decode processes'
          % (n, h, w, c, FLAGS.out, time.time() - t0, mode, stride, os.path.getsize(FLAGS.out), 'yes' if labels is not None else 'none', workers))
    return 0


if __name__ == '__main__':
    sys.exit(main())
