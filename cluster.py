#!/usr/bin/env python
"""cluster.py -- group the embeddings of an unlabelled or badly labelled image list into identities: pseudo-labels for more
training data, a check for one person split over several classes, or a look at a scraped list before use.

  python evaluate.py --net_name SphereNet-ArcFace --model_name m --fea_name scraped --data_list_path scraped.txt ...
  python cluster.py --feature_path features/SphereNet-ArcFace_m/scraped_20000.mat --data_list_path scraped.txt --k 32 \\
      --method rank_order --theta T --min_size 2 --out_list scraped_clustered.txt --output_json scraped_clusters.json
  python cluster.py ... --method threshold --min_score S --mutual 1

The kNN graph, the link rule and the connected components run on the GPU (tf_face_toolbox_amd/clustering.py).
--out_list holds `path cluster_id` for every kept row, ids dense from 0: train.py reads it as it is.  When the input list has a
label column the clustering scores against it are printed (and written to --output_json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_K = 64


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--feature_path', type=str, required=True, help="features of the list: evaluate.py's .mat (`wfea` [N, D]) or a .npy")
    parser.add_argument('--data_list_path', type=str, required=True, help='the list the features were extracted from (`path` or `path label` per line).')
    parser.add_argument('--k', type=int, default=32, help='neighbours per row, 1..64 (a size, not a tuned value).')
    parser.add_argument('--method', type=str, required=True, choices=('rank_order', 'threshold'),
                        help='rank_order: approximate rank-order links (Otto, Wang, Jain 2018); threshold: a cosine floor on the kNN graph.')
    parser.add_argument('--theta', type=float, default=None,
                        help='rank_order: link when the rank-order distance is below this.  Required, no default: a good value has not been '
                             'measured on real embeddings.')
    parser.add_argument('--min_score', type=float, default=None,
                        help='cosine floor of a link.  Required for threshold (no default: a good value has not been measured on real '
                             'embeddings), optional for rank_order.')
    parser.add_argument('--mutual', type=int, default=0, help='threshold: 1 keeps a link only when the neighbour lists the row back.')
    parser.add_argument('--min_size', type=int, default=1, help='clusters with fewer rows are dropped from --out_list.')
    parser.add_argument('--chunk_rows', type=int, default=None, help='rows per chunk of the kNN search (default: chunks below 2 GiB).')
    parser.add_argument('--out_list', type=str, required=True, help='`path cluster_id` for every row of a kept cluster, in list order.')
    parser.add_argument('--output_json', type=str, default=None, help='the counts (and, with labels, the scores) as JSON.')
    return parser


def check_flags(FLAGS):
    if not 1 <= FLAGS.k <= MAX_K:
        raise SystemExit('--k must lie in 1..%d: got %d' % (MAX_K, FLAGS.k))
    if FLAGS.method == 'rank_order':
        if FLAGS.theta is None:
            raise SystemExit('--method rank_order needs --theta (no default: nobody has measured a good one on real embeddings)')
        if not (FLAGS.theta > 0 and np.isfinite(FLAGS.theta)):
            raise SystemExit('--theta must be finite and positive: got %g' % FLAGS.theta)
        if FLAGS.mutual:
            raise SystemExit('--mutual belongs to --method threshold')
    else:
        if FLAGS.min_score is None:
            raise SystemExit('--method threshold needs --min_score (no default: nobody has measured a good one on real embeddings)')
        if FLAGS.theta is not None:
            raise SystemExit('--theta belongs to --method rank_order')
    if FLAGS.min_size < 1:
        raise SystemExit('--min_size must be at least 1: got %d' % FLAGS.min_size)
    if FLAGS.chunk_rows is not None and FLAGS.chunk_rows < 1:
        raise SystemExit('--chunk_rows must be positive: got %d' % FLAGS.chunk_rows)


def read_list(path):
    """-> (paths, labels or None) of the non-blank lines: the rows evaluate.py extracts features for.  Labels only when every
    line has an integer second column."""
    paths, labels = [], []
    for line in open(path):
        part = line.split()
        if not part:
            continue
        paths.append(part[0])
        labels.append(part[1] if len(part) > 1 else None)
    try:
        labels = np.asarray([int(v) for v in labels], dtype=np.int64)
    except (TypeError, ValueError):
        labels = None
    return paths, labels


def read_features(path):
    if path.endswith('.npy'):
        return np.load(path)
    from scipy.io import loadmat
    return loadmat(path)['wfea']


def write_list(path, paths, ids):
    """`path cluster_id` per row with an id >= 0, in list order -> the number of lines written"""
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    kept = 0
    with open(path, 'w') as f:
        for p, c in zip(paths, ids):
            if c >= 0:
                f.write('%s %d\n' % (p, c))
                kept += 1
    return kept


def main(argv=None):
    FLAGS = build_parser().parse_args(argv)
    check_flags(FLAGS)
    paths, labels = read_list(FLAGS.data_list_path)
    feats = np.ascontiguousarray(read_features(FLAGS.feature_path), dtype=np.float32)
    if feats.ndim != 2 or feats.shape[0] != len(paths):
        raise SystemExit('%s features in %s but %d lines in %s' % (feats.shape, FLAGS.feature_path, len(paths), FLAGS.data_list_path))
    import torch
    from tf_face_toolbox_amd import clustering
    torch.cuda.set_device(0)
    ids = clustering.cluster(feats, FLAGS.k, FLAGS.method, theta=FLAGS.theta, min_score=FLAGS.min_score, mutual=bool(FLAGS.mutual),
                             min_size=FLAGS.min_size, chunk_rows=FLAGS.chunk_rows)
    kept = write_list(FLAGS.out_list, paths, ids)
    res = {'rows': len(paths), 'kept_rows': kept, 'kept_clusters': int(ids.max()) + 1 if kept else 0, 'k': FLAGS.k, 'method': FLAGS.method,
           'theta': FLAGS.theta, 'min_score': FLAGS.min_score, 'mutual': int(bool(FLAGS.mutual)), 'min_size': FLAGS.min_size}
    print('%d rows -> %d clusters of at least %d rows holding %d rows: %s' % (res['rows'], res['kept_clusters'], FLAGS.min_size, kept, FLAGS.out_list))
    if labels is not None:
        res['scores'] = clustering.clustering_scores(ids, labels)
        print('against the list labels: ' + ', '.join('%s %.4f' % (k, v) if isinstance(v, float) else '%s %d' % (k, v)
                                                        for k, v in res['scores'].items()))
    if FLAGS.output_json:
        if os.path.dirname(FLAGS.output_json):
            os.makedirs(os.path.dirname(FLAGS.output_json), exist_ok=True)
        with open(FLAGS.output_json, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    FLAGS.result = res
    return FLAGS


if __name__ == '__main__':
    from train import _run_and_leave
    _run_and_leave(main)
