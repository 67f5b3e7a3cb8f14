#!/usr/bin/env python
"""align.py -- write the five-point aligned crops the loader computes (train.py / evaluate.py --landmark_list_path) as PNG files:
to cache an aligned data set once, or to look at what the loader sees.  Host only (numpy + PIL, as the decode workers): no GPU.

    python align.py --data_list_path L --landmark_list_path P --input_height 112 --input_width 112 --out_dir D [--out_list L2]

Every image of L is decoded, aligned to input_height x input_width by the host definition (tf_face_toolbox_amd/preprocessing.py:
align_window, align_warp) and stored as round(255 * x) of that [0, 1] image under D, its relative path kept (an absolute path
keeps its components below the root), the extension replaced by .png.  L2 (default D/list.txt) repeats L with the new paths,
written ABSOLUTE so that the list is valid from any working directory; a label column is kept."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_list_path', type=str, required=True, help='`path` or `path label` per line.')
    parser.add_argument('--landmark_list_path', type=str, required=True, help='`path x1 y1 x2 y2 x3 y3 x4 y4 x5 y5` per line, source pixels.')
    parser.add_argument('--input_height', type=int, default=112, help='Height of the aligned crop.')
    parser.add_argument('--input_width', type=int, default=112, help='Width of the aligned crop.')
    parser.add_argument('--is_color', type=int, default=1, help='Whether to read inputs as RGB images.')
    parser.add_argument('--out_dir', type=str, required=True, help='Directory the crops are written under.')
    parser.add_argument('--out_list', type=str, default=None, help='The list that points at the crops (default: <out_dir>/list.txt).')
    return parser


def aligned_u8(path, landmarks, num_channels, height, width):
    """round(255 * x) of the host aligned image x in [0, 1], uint8 HWC"""
    from tf_face_toolbox_amd import _decode_worker as dw          # numpy + PIL only
    x = dw.decode(path, num_channels, height, width, landmarks)
    return np.clip(np.rint(x.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)


def out_name(path):
    rel = os.path.normpath(path)
    rel = os.path.splitdrive(rel)[1].lstrip(os.sep)
    rel = os.sep.join(p for p in rel.split(os.sep) if p not in ('..', '.', ''))
    return os.path.splitext(rel)[0] + '.png'


def main(argv=None):
    from PIL import Image
    FLAGS = build_parser().parse_args(argv)
    from tf_face_toolbox_amd import preprocessing as pp
    with open(os.path.expanduser(FLAGS.data_list_path), 'r') as f:
        lines = [ln.split() for ln in f if ln.split()]
    paths = [p[0] for p in lines]
    landmarks = pp.read_landmarks(FLAGS.landmark_list_path, paths)
    num_channels = 3 if FLAGS.is_color else 1
    out_list = FLAGS.out_list or os.path.join(FLAGS.out_dir, 'list.txt')
    os.makedirs(FLAGS.out_dir, exist_ok=True)
    written = []
    for part, lm in zip(lines, landmarks):
        img = aligned_u8(part[0], lm, num_channels, FLAGS.input_height, FLAGS.input_width)
        dst = os.path.join(os.path.abspath(FLAGS.out_dir), out_name(part[0]))
        os.makedirs(os.path.dirname(dst) or '.', exist_ok=True)
        Image.fromarray(img if num_channels == 3 else img[:, :, 0]).save(dst)
        written.append(' '.join([dst] + part[1:]))
    with open(out_list, 'w') as f:
        f.write('\n'.join(written) + '\n')
    print('%d aligned %d x %d crops under %s, list %s' % (len(written), FLAGS.input_height, FLAGS.input_width, FLAGS.out_dir, out_list))
    return 0


if __name__ == '__main__':
    sys.exit(main())
