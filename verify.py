#!/usr/bin/env python
"""verify.py -- score the embeddings evaluate.py wrote (`wfea` in a .mat) against the list that produced them:
  --protocol pairs      LFW-style 10-fold verification accuracy on the listed pairs of --pairs_path (pairs.txt format);
  --protocol all_pairs  TAR at FAR 1e-6 .. 1e-3 over every pair of the set, labels from the list's second column;
  --protocol identify   closed-set 1:N identification (rank-1 / 5 / 10 and the CMC) against --gallery_feature_path /
                        --gallery_list_path, or leave-one-out on the one set when no gallery is given.
The products, top-k and histograms run on the GPU (tf_face_toolbox_amd.verification)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser(description='Face verification / identification scoring of evaluate.py features.')
    parser.add_argument('--protocol', type=str, required=True, choices=('pairs', 'all_pairs', 'identify'), help='Scoring protocol.')
    parser.add_argument('--feature_path', type=str, required=True, help='.mat file written by evaluate.py (variable wfea).')
    parser.add_argument('--data_list_path', type=str, required=True, help='The list evaluate.py extracted the features from.')
    parser.add_argument('--pairs_path', type=str, help='pairs.txt of the pairs protocol.')
    parser.add_argument('--folds', type=int, default=0, help='Folds of the pairs protocol (default: the pairs.txt header).')
    parser.add_argument('--gallery_feature_path', type=str, help='identify: .mat of the gallery (default: leave-one-out).')
    parser.add_argument('--gallery_list_path', type=str, help='identify: list of the gallery.')
    parser.add_argument('--nbins', type=int, default=8192, help='all_pairs: histogram bins over [-1, 1].')
    parser.add_argument('--chunk_rows', type=int, default=0, help='Rows per chunk handed to the library (default: below 2 GiB).')
    parser.add_argument('--output_json', type=str, help='Also write the results as JSON to this path.')
    return parser


def _features(path):
    from scipy.io import loadmat
    return np.asarray(loadmat(path)['wfea'], np.float32)


def _labels(list_path):
    from tf_face_toolbox_amd.data import get_image_paths_and_labels
    paths, labels, _, _ = get_image_paths_and_labels(list_path)
    return paths, np.asarray(labels, np.int64)


def _device_rows(x):
    import torch
    from tf_face_toolbox_amd import verification as V
    return V.normalize(torch.from_numpy(np.ascontiguousarray(x)).cuda())


def run(FLAGS):
    import torch
    from tf_face_toolbox_amd import verification as V
    from tf_face_toolbox_amd.data import get_image_paths

    torch.cuda.set_device(0)
    t0 = time.time()
    chunk = FLAGS.chunk_rows or None
    res = {'protocol': FLAGS.protocol}
    try:
        feats = _features(FLAGS.feature_path)
        if FLAGS.protocol == 'pairs':
            if not FLAGS.pairs_path:
                raise SystemExit('--protocol pairs needs --pairs_path')
            paths, n = get_image_paths(FLAGS.data_list_path)
            if n != feats.shape[0]:
                raise SystemExit('%s has %d rows, %s lists %d images' % (FLAGS.feature_path, feats.shape[0], FLAGS.data_list_path, n))
            pairs, same, folds = V.read_lfw_pairs(FLAGS.pairs_path)
            ia, ib = V.map_pairs_to_rows(pairs, paths)
            scores = V.pair_scores(_device_rows(feats), ia, ib).cpu().numpy()
            mean, std, thrs = V.kfold_accuracy(scores, same, FLAGS.folds or folds)
            res.update(pairs=len(pairs), accuracy=mean, std=std, thresholds=thrs)
            print('%d pairs, %d folds: accuracy %.4f +- %.4f' % (len(pairs), FLAGS.folds or folds, mean, std))
        elif FLAGS.protocol == 'all_pairs':
            _, labels = _labels(FLAGS.data_list_path)
            if len(labels) != feats.shape[0]:
                raise SystemExit('%s has %d rows, %s lists %d images' % (FLAGS.feature_path, feats.shape[0], FLAGS.data_list_path, len(labels)))
            hg, hi = V.score_histograms(_device_rows(feats), labels, FLAGS.nbins, chunk)
            table = V.tar_at_far(hg, hi)
            res.update(genuine=int(hg.sum()), impostor=int(hi.sum()), tar_at_far=table)
            print('%d images: %d genuine pairs, %d impostor pairs' % (len(labels), int(hg.sum()), int(hi.sum())))
            print('%10s %10s %14s %10s' % ('FAR', 'TAR', 'achieved FAR', 'threshold'))
            for r in table:
                if r['tar'] == 'n/a':
                    print('%10.0e %10s %14s %10s' % (r['far'], 'n/a', 'n/a', 'n/a'))
                else:
                    print('%10.0e %10.4f %14.3e %10.4f' % (r['far'], r['tar'], r['achieved_far'], r['threshold']))
        else:
            _, plabels = _labels(FLAGS.data_list_path)
            if FLAGS.gallery_feature_path:
                if not FLAGS.gallery_list_path:
                    raise SystemExit('--gallery_feature_path needs --gallery_list_path')
                gfeats = _features(FLAGS.gallery_feature_path)
                _, glabels = _labels(FLAGS.gallery_list_path)
                excl = False
            else:
                gfeats, glabels, excl = feats, plabels, True
            probes = _device_rows(feats)
            gallery = probes if gfeats is feats else _device_rows(gfeats)
            k = min(10, gallery.shape[0] - (1 if excl else 0))
            if k < 1:
                raise SystemExit('identify: the gallery has no row to rank')
            _, index = V.topk_search(probes, gallery, k, exclude_self=excl, chunk_rows=chunk)
            curve = V.cmc(index.cpu().numpy(), plabels, glabels, ranks=tuple(range(1, k + 1)))
            res.update(probes=int(probes.shape[0]), gallery=int(gallery.shape[0]), leave_one_out=excl,
                       cmc={str(r): v for r, v in curve.items()})
            print('%d probes, %d gallery rows%s' % (probes.shape[0], gallery.shape[0], ' (leave-one-out)' if excl else ''))
            print('  '.join('rank-%d %.4f' % (r, curve[r]) for r in (1, 5, 10) if r in curve))
            print('CMC: ' + ' '.join('%.4f' % curve[r] for r in sorted(curve)))
    finally:
        try:                                # never raise from a finally block: an error on its way out stays the one reported
            torch.cuda.synchronize()
        except Exception as e:
            print('verify.py: device synchronise failed during shutdown: %s' % e, file=sys.stderr)
            FLAGS._shutdown_failed = True
    res['seconds'] = time.time() - t0
    print('verify.py: %s done in %.2f s' % (FLAGS.protocol, res['seconds']))
    if FLAGS.output_json:
        with open(FLAGS.output_json, 'w') as f:
            json.dump(res, f, indent=1)
    return FLAGS


if __name__ == '__main__':
    from train import _run_and_leave           # leaves with the real status once the device is drained
    _run_and_leave(lambda: run(build_parser().parse_args()))
