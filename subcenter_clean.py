#!/usr/bin/env python
"""subcenter_clean.py -- the second stage of sub-center ArcFace (Deng et al., ECCV 2020) after `train.py --sub_centers K`:
keep the dominant centre of every class, drop the training samples further than --angle degrees from it, write the cleaned list and
a K = 1 checkpoint the run continues from (train.py without --sub_centers, --pretrained_path or a model directory holding it).

  python evaluate.py --net_name SphereNet-ArcFace --model_name m --fea_name train --data_list_path train.txt ...
  python subcenter_clean.py --feature_path features/SphereNet-ArcFace_m/train_20000.mat --data_list_path train.txt \\
      --model_path models/SphereNet-ArcFace_m --sub_centers 3 --angle 75 --out_list train_clean.txt --out_model models/clean/clean.ckpt-0

The rules are tf_face_toolbox_amd/subcenter.py's; the classifier's optimizer slots are zeroed in --out_model."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--feature_path', type=str, required=True, help="features of the training list: evaluate.py's .mat (`wfea` [N, D]) or a .npy")
    parser.add_argument('--data_list_path', type=str, required=True, help='the labelled training list the features were extracted from (`path label` per line).')
    parser.add_argument('--model_path', type=str, required=True, help='the K-centre checkpoint file, or the directory whose latest checkpoint is taken.')
    parser.add_argument('--sub_centers', type=int, required=True, help='K the model was trained with (1..8).')
    parser.add_argument('--angle', type=float, default=75.0, help='drop samples further than this many degrees from the dominant centre of their class.')
    parser.add_argument('--out_list', type=str, required=True, help='the kept lines of --data_list_path, in order and unchanged.')
    parser.add_argument('--out_model', type=str, required=True, help='the checkpoint with the [D, C] classifier of dominant centres.')
    parser.add_argument('--chunk', type=int, default=65536, help='samples per launch of the assignment kernel.')
    return parser


def read_list(path):
    """-> (lines as written, labels) of the non-blank lines: the rows evaluate.py extracts features for"""
    lines, labels = [], []
    for line in open(path):
        part = line.split()
        if not part:
            continue
        if len(part) < 2:
            raise SystemExit('%s: a line without a label: %r' % (path, line))
        lines.append(line)
        labels.append(int(part[1]))
    return lines, np.asarray(labels, dtype=np.int64)


def read_features(path):
    if path.endswith('.npy'):
        return np.load(path)
    from scipy.io import loadmat
    return loadmat(path)['wfea']


def main(argv=None):
    FLAGS = build_parser().parse_args(argv)
    import torch
    from tf_face_toolbox_amd import heads, saver, subcenter
    try:
        K = heads.check_sub_centers(FLAGS.sub_centers)
    except ValueError as e:
        raise SystemExit('--sub_centers: %s' % e)
    if not 0.0 <= FLAGS.angle <= 180.0:
        raise SystemExit('--angle must lie in [0, 180] degrees: got %g' % FLAGS.angle)
    path = FLAGS.model_path
    if os.path.isdir(path):
        path = saver.latest_checkpoint(path)
        if not path:
            raise SystemExit('No checkpoint file found in %s' % FLAGS.model_path)
    state = torch.load(path, map_location='cpu')
    W = state['variables'][subcenter.CLASSIFIER]
    if W.shape[1] % K:
        raise SystemExit('%s: the classifier has %d columns, not a multiple of --sub_centers %d' % (path, W.shape[1], K))
    lines, labels = read_list(FLAGS.data_list_path)
    feats = np.ascontiguousarray(read_features(FLAGS.feature_path), dtype=np.float32)
    if feats.shape[0] != len(lines):
        raise SystemExit('%d features in %s but %d labelled lines in %s' % (feats.shape[0], FLAGS.feature_path, len(lines), FLAGS.data_list_path))
    torch.cuda.set_device(0)
    res = subcenter.clean(feats, labels, W, K, FLAGS.angle, FLAGS.chunk, torch.device('cuda', 0))
    torch.cuda.synchronize()
    keep = res['keep'].numpy()
    for out in (FLAGS.out_list, FLAGS.out_model):
        if os.path.dirname(out):
            os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(FLAGS.out_list, 'w') as f:
        f.writelines(l for l, k in zip(lines, keep) if k)
    torch.save(subcenter.reduce_checkpoint(state, res['weights']), FLAGS.out_model)
    subcenter.report(res)
    print('%d classes, %d -> 1 centres: %s, %s' % (res['kept'].numel(), K, FLAGS.out_list, FLAGS.out_model))
    return FLAGS


if __name__ == '__main__':
    from train import _run_and_leave
    _run_and_leave(main)
