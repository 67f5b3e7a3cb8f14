#!/usr/bin/env python
"""verify.py -- score the embeddings evaluate.py wrote (`wfea` in a .mat) against the list that produced them:
  --protocol pairs      LFW-style 10-fold verification accuracy on the listed pairs of --pairs_path (pairs.txt format);
  --protocol all_pairs  TAR at FAR 1e-6 .. 1e-3 over every pair of the set, labels from the list's second column;
  --protocol identify   closed-set 1:N identification (rank-1 / 5 / 10 and the CMC) against --gallery_feature_path /
                        --gallery_list_path, or leave-one-out on the one set when no gallery is given;
  --protocol templates  IJB-style 1:1 template verification: TAR at FAR 1e-6 .. 1e-1 over the pairs of --template_pairs, the
                        templates of --template_metadata compared by pooled features (--fusion pool) or by set-to-set softmax
                        score fusion (--fusion softmax);
  --protocol template_search  IJB-style open-set 1:N search of pooled probe templates (--template_metadata) against pooled
                        gallery templates (--gallery_metadata): rank-1 / 5 / 10, the CMC and TPIR at FPIR 0.01 / 0.1;
  --protocol megaface   MegaFace challenge-1 style: the labelled set (FaceScrub) against the first N rows of
                        --distractor_feature_path / --distractor_list_path for each N of --distractor_sizes (after removing the
                        rows of --distractor_exclude): per size the rank-1 rate and CMC of every ordered same-label pair (ties
                        count against the pair) and TAR at FAR 1e-6 .. 1e-3 with set x distractor impostors.
A `{split}` in any path with --splits (e.g. 1-10) runs every split and reports the mean and std over them.
The products, top-k, histograms, pooling, fusion and the MegaFace scan run on the GPU (tf_face_toolbox_amd.verification,
DESIGN.md 4.10 - 4.12)."""
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
    parser.add_argument('--protocol', type=str, required=True, choices=('pairs', 'all_pairs', 'identify', 'templates', 'template_search', 'megaface'), help='Scoring protocol.')
    parser.add_argument('--feature_path', type=str, required=True, help='.mat file written by evaluate.py (variable wfea).')
    parser.add_argument('--data_list_path', type=str, required=True, help='The list evaluate.py extracted the features from.')
    parser.add_argument('--pairs_path', type=str, help='pairs.txt of the pairs protocol.')
    parser.add_argument('--folds', type=int, default=0, help='Folds of the pairs protocol (default: the pairs.txt header).')
    parser.add_argument('--gallery_feature_path', type=str, help='identify: .mat of the gallery (default: leave-one-out).')
    parser.add_argument('--gallery_list_path', type=str, help='identify: list of the gallery.')
    parser.add_argument('--nbins', type=int, default=8192, help='all_pairs / megaface: histogram bins over [-1, 1].')
    parser.add_argument('--chunk_rows', type=int, default=0, help='Rows per chunk handed to the library (default: below 2 GiB).')
    parser.add_argument('--template_metadata', type=str, help='templates / template_search: IJB-style metadata CSV of the set '
                        '(columns TEMPLATE_ID, SUBJECT_ID, FILE, MEDIA_ID; the probe set of template_search).')
    parser.add_argument('--template_pairs', type=str, help='templates: pairs `t1 t2 [label]` (no label: genuine when the subjects match).')
    parser.add_argument('--fusion', type=str, default='pool', choices=('pool', 'softmax'), help='templates: pooled features or '
                        'set-to-set softmax score fusion.')
    parser.add_argument('--betas', type=str, default='0:20', help='templates --fusion softmax: betas, `a:b[:step]` (inclusive) or '
                        'a comma list; 1..32 values in [0, 40].')
    parser.add_argument('--weight_column', type=str, help='templates / template_search: metadata column of per-image pooling weights.')
    parser.add_argument('--weight_by_norm', type=int, default=0, help='templates (--fusion pool) / template_search: 1 = pool the unit '
                        'features with the norms of the raw features as the per-image weights (the quality score of a MagFace model: '
                        'verification.feature_quality).  Not together with --weight_column.')
    parser.add_argument('--gallery_metadata', type=str, help='template_search: metadata CSV of the gallery templates.')
    parser.add_argument('--distractor_feature_path', type=str, help='megaface: .mat of the distractor features (wfea).')
    parser.add_argument('--distractor_list_path', type=str, help='megaface: the distractor list (paths only; row i = line i).')
    parser.add_argument('--distractor_exclude', type=str, help='megaface: noise list, one path per line; a distractor whose path '
                        'equals one or ends with / + one is dropped before anything else.')
    parser.add_argument('--distractor_sizes', type=str, default='10,100,1000,10000,100000,1000000',
                        help='megaface: distractor set sizes N (the first N kept rows); a size above the kept count is capped.')
    parser.add_argument('--splits', type=str, help='Values of {split} in the paths: `1-10` or a comma list (default: one run).')
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


def parse_betas(text):
    """`a:b[:step]` (b included) or a comma list"""
    if ':' in text:
        part = [float(v) for v in text.split(':')]
        a, b, st = part[0], part[1], (part[2] if len(part) > 2 else 1.0)
        if st <= 0:
            raise ValueError('betas %r: step must be positive' % text)
        return [a + i * st for i in range(int(np.floor((b - a) / st + 1e-9)) + 1)]
    return [float(v) for v in text.split(',') if v.strip()]


def parse_splits(text):
    """`1-10` or a comma list -> ['1', ..., '10']; None -> [None]"""
    if not text:
        return [None]
    out = []
    for part in text.split(','):
        if '-' in part.strip()[1:]:
            a, b = part.split('-', 1)
            out.extend(str(i) for i in range(int(a), int(b) + 1))
        elif part.strip():
            out.append(part.strip())
    return out


def _split_path(path, split):
    return path.replace('{split}', split) if path and split is not None else path


def _template_set(meta_path, feature_path, list_path, weight_column):
    """metadata, checked feature rows and the CSR grouping of one template set"""
    from tf_face_toolbox_amd import verification as V
    from tf_face_toolbox_amd.data import get_image_paths
    meta = V.read_template_metadata(meta_path, weight_column)
    paths, _ = get_image_paths(list_path)
    V.check_data_list(paths, meta, list_path)
    feats = _features(feature_path)
    if feats.shape[0] != len(meta['file']):
        raise ValueError('%s has %d rows, %s has %d' % (feature_path, feats.shape[0], meta_path, len(meta['file'])))
    return meta, feats, V.build_templates(meta)


def _pooled(feats, tpl, meta, weight_by_norm=False):
    """the pooled template features; weight_by_norm: the norm of each raw row is its weight (else the metadata column, or 1)"""
    import torch
    from tf_face_toolbox_amd import verification as V
    if weight_by_norm:
        rows, weights = V.normalize(torch.from_numpy(np.ascontiguousarray(feats)).cuda(), return_norms=True)
    else:
        rows, weights = _device_rows(feats), meta['weight']
    return V.template_pool(rows, tpl['members'], tpl['media_off'], tpl['tmpl_off'], weights)


def weight_flags_check(FLAGS):
    """--weight_by_norm: refuse it beside --weight_column and where nothing is pooled"""
    if not getattr(FLAGS, 'weight_by_norm', 0):
        return
    if FLAGS.weight_column:
        raise SystemExit('--weight_by_norm 1 and --weight_column both set the per-image pooling weights: give one of them')
    if FLAGS.protocol not in ('templates', 'template_search') or (FLAGS.protocol == 'templates' and FLAGS.fusion != 'pool'):
        raise SystemExit('--weight_by_norm 1 weights the pooled template features: --protocol templates (--fusion pool) or template_search')


def run_templates(FLAGS, split):
    """one split of --protocol templates"""
    from tf_face_toolbox_amd import verification as V
    if not FLAGS.template_metadata or not FLAGS.template_pairs:
        raise SystemExit('--protocol templates needs --template_metadata and --template_pairs')
    sp = lambda p: _split_path(p, split)
    meta, feats, tpl = _template_set(sp(FLAGS.template_metadata), sp(FLAGS.feature_path), sp(FLAGS.data_list_path), FLAGS.weight_column)
    subj = dict(zip(tpl['template_ids'].tolist(), tpl['subjects'].tolist()))
    t1, t2, genuine = V.read_template_pairs(sp(FLAGS.template_pairs), subj)
    ia, ib = V.template_index(tpl['template_ids'], t1), V.template_index(tpl['template_ids'], t2)
    if FLAGS.fusion == 'pool':
        scores = V.pair_scores(_pooled(feats, tpl, meta, bool(FLAGS.weight_by_norm)), ia, ib).cpu().numpy()
    else:
        scores = V.set_pair_scores(_device_rows(feats), tpl['members'], tpl['media_off'], tpl['tmpl_off'], ia, ib,
                                   parse_betas(FLAGS.betas)).cpu().numpy()
    table = V.tar_at_far_scores(scores, genuine)
    print('%s%d templates, %d pairs (%d genuine), fusion %s' % ('split %s: ' % split if split is not None else '',
          len(tpl['template_ids']), len(t1), int(genuine.sum()), FLAGS.fusion))
    print('%10s %10s %14s %10s' % ('FAR', 'TAR', 'achieved FAR', 'threshold'))
    for r in table:
        if r['tar'] == 'n/a':
            print('%10.0e %10s %14s %10s' % (r['far'], 'n/a', 'n/a', 'n/a'))
        else:
            print('%10.0e %10.4f %14.3e %10.4f' % (r['far'], r['tar'], r['achieved_far'], r['threshold']))
    return {'templates': len(tpl['template_ids']), 'pairs': len(t1), 'genuine': int(genuine.sum()), 'fusion': FLAGS.fusion,
            'tar_at_far': table}


def run_template_search(FLAGS, split):
    """one split of --protocol template_search"""
    from tf_face_toolbox_amd import verification as V
    if not (FLAGS.template_metadata and FLAGS.gallery_metadata and FLAGS.gallery_feature_path and FLAGS.gallery_list_path):
        raise SystemExit('--protocol template_search needs --template_metadata, --gallery_metadata, --gallery_feature_path and '
                         '--gallery_list_path')
    sp = lambda p: _split_path(p, split)
    pmeta, pfeats, ptpl = _template_set(sp(FLAGS.template_metadata), sp(FLAGS.feature_path), sp(FLAGS.data_list_path), FLAGS.weight_column)
    gmeta, gfeats, gtpl = _template_set(sp(FLAGS.gallery_metadata), sp(FLAGS.gallery_feature_path), sp(FLAGS.gallery_list_path),
                                        FLAGS.weight_column)
    by_norm = bool(FLAGS.weight_by_norm)
    P, G = _pooled(pfeats, ptpl, pmeta, by_norm), _pooled(gfeats, gtpl, gmeta, by_norm)
    k = min(10, G.shape[0])
    s, i = V.topk_search(P, G, k, chunk_rows=FLAGS.chunk_rows or None)
    res = V.open_set_identification(s.cpu().numpy(), i.cpu().numpy(), ptpl['subjects'], gtpl['subjects'], ranks=tuple(range(1, k + 1)))
    print('%sprobe templates %d (%d mated), gallery templates %d' % ('split %s: ' % split if split is not None else '',
          len(ptpl['subjects']), res['mated'], len(gtpl['subjects'])))
    print('  '.join('rank-%d %s' % (r, _fmt(res['cmc'][r])) for r in (1, 5, 10) if r in res['cmc']))
    print('  '.join('TPIR@FPIR=%g %s' % (t['fpir'], _fmt(t['tpir'])) for t in res['tpir_at_fpir']))
    return {'probe_templates': len(ptpl['subjects']), 'gallery_templates': len(gtpl['subjects']), 'mated': res['mated'],
            'non_mated': res['non_mated'], 'cmc': {str(r): v for r, v in res['cmc'].items()}, 'tpir_at_fpir': res['tpir_at_fpir']}


def run_megaface(FLAGS):
    """--protocol megaface"""
    from tf_face_toolbox_amd import verification as V
    from tf_face_toolbox_amd.data import get_image_paths
    if not FLAGS.distractor_feature_path or not FLAGS.distractor_list_path:
        raise SystemExit('--protocol megaface needs --distractor_feature_path and --distractor_list_path')
    feats = _features(FLAGS.feature_path)
    _, labels = _labels(FLAGS.data_list_path)
    if len(labels) != feats.shape[0]:
        raise SystemExit('%s has %d rows, %s lists %d images' % (FLAGS.feature_path, feats.shape[0], FLAGS.data_list_path, len(labels)))
    dfeats = _features(FLAGS.distractor_feature_path)
    dpaths, nd = get_image_paths(FLAGS.distractor_list_path)
    if nd != dfeats.shape[0]:
        raise SystemExit('%s has %d rows, %s lists %d paths' % (FLAGS.distractor_feature_path, dfeats.shape[0], FLAGS.distractor_list_path, nd))
    if dfeats.shape[1] != feats.shape[1]:
        raise SystemExit('megaface: the probe features are %d wide, the distractors %d' % (feats.shape[1], dfeats.shape[1]))
    excluded = 0
    if FLAGS.distractor_exclude:
        keep = V.megaface_exclude(dpaths, get_image_paths(FLAGS.distractor_exclude)[0])
        excluded = int((~keep).sum())
        dfeats = dfeats[keep]
    print('megaface: %d distractors listed, %d removed by %s, %d kept' % (nd, excluded, FLAGS.distractor_exclude or 'no noise list',
                                                                         dfeats.shape[0]))
    try:
        sizes = V.megaface_sizes([int(v) for v in FLAGS.distractor_sizes.split(',') if v.strip()], dfeats.shape[0])
    except ValueError as e:
        raise SystemExit('verify.py: %s' % e)
    Ns = [N for N, _ in sizes]
    probes = _device_rows(feats)
    r = V.megaface_evaluate(probes, labels, _device_rows(dfeats[:Ns[-1]]), Ns, FLAGS.nbins, FLAGS.chunk_rows or None)
    ids = len(np.unique(labels))
    print('%d probes of %d identities (%d with a single image add no pair), %d genuine pairs' % (len(labels), ids, r['singletons'], r['pairs']))
    table = V.megaface_tar_table(r['genuine_hist'], r['impostor_hist'], Ns)
    out = []
    for b, (N, capped) in enumerate(sizes):
        shown = V.megaface_cmc(r['rank'][b], V.megaface_report_ranks(N))
        full = V.megaface_cmc(r['rank'][b], V.megaface_report_ranks(N, range(1, 11)))
        print('size %d%s: rank-1 %s' % (N, ' (capped: fewer distractors kept than requested)' if capped else '', _fmt(shown[1])))
        print('  CMC: ' + '  '.join('%d: %s' % (k, _fmt(v)) for k, v in shown.items()))
        print('  %10s %10s %14s %10s' % ('FAR', 'TAR', 'achieved FAR', 'threshold'))
        for t in table[b]['tar_at_far']:
            if t['tar'] == 'n/a':
                print('  %10.0e %10s %14s %10s' % (t['far'], 'n/a', 'n/a', 'n/a'))
            else:
                print('  %10.0e %10.4f %14.3e %10.4f' % (t['far'], t['tar'], t['achieved_far'], t['threshold']))
        out.append({'size': N, 'capped': capped, 'rank1': full[1], 'cmc': {str(k): v for k, v in full.items()},
                    'impostor': table[b]['impostor'], 'tar_at_far': table[b]['tar_at_far']})
    return {'probes': len(labels), 'identities': ids, 'singletons': r['singletons'], 'genuine_pairs': r['pairs'],
            'genuine': int(r['genuine_hist'].sum()), 'distractors': nd, 'excluded': excluded, 'kept': int(dfeats.shape[0]),
            'sizes': out}


def _fmt(v):
    return v if isinstance(v, str) else '%.4f' % v


def summarise_splits(per_split):
    """mean and std (ddof = 0) over splits of every numeric metric: TAR per FAR, the CMC, TPIR per FPIR"""
    vals = {}
    for r in per_split:
        for row in r.get('tar_at_far', []):
            vals.setdefault('TAR@FAR=%g' % row['far'], []).append(row['tar'])
        for rank, v in r.get('cmc', {}).items():
            vals.setdefault('rank-%s' % rank, []).append(v)
        for row in r.get('tpir_at_fpir', []):
            vals.setdefault('TPIR@FPIR=%g' % row['fpir'], []).append(row['tpir'])
    out = {}
    for name, v in vals.items():
        if any(isinstance(x, str) for x in v):
            out[name] = {'mean': 'n/a', 'std': 'n/a'}
        else:
            out[name] = {'mean': float(np.mean(v)), 'std': float(np.std(v))}
    return out


def run_template_protocol(FLAGS):
    """templates / template_search over every split of --splits; with more than one, per-split results and their summary"""
    one = run_templates if FLAGS.protocol == 'templates' else run_template_search
    splits = parse_splits(FLAGS.splits)
    per = []
    for sp in splits:
        try:
            per.append(one(FLAGS, sp))
        except (ValueError, KeyError) as e:
            raise SystemExit('verify.py: %s%s' % ('split %s: ' % sp if sp is not None else '', e.args[0] if e.args else e))
    if splits == [None]:
        return per[0]
    summary = summarise_splits(per)
    print('over %d splits (mean +- std):' % len(splits))
    for name, v in summary.items():
        print('  %-16s %s' % (name, 'n/a' if v['mean'] == 'n/a' else '%.4f +- %.4f' % (v['mean'], v['std'])))
    return {'splits': dict(zip(splits, per)), 'summary': summary}


def run(FLAGS):
    import torch
    from tf_face_toolbox_amd import verification as V
    from tf_face_toolbox_amd.data import get_image_paths

    weight_flags_check(FLAGS)
    torch.cuda.set_device(0)
    t0 = time.time()
    chunk = FLAGS.chunk_rows or None
    res = {'protocol': FLAGS.protocol}
    try:
        if FLAGS.protocol in ('templates', 'template_search'):
            res.update(run_template_protocol(FLAGS))
        elif FLAGS.protocol == 'megaface':
            res.update(run_megaface(FLAGS))
        elif FLAGS.protocol == 'pairs':
            feats = _features(FLAGS.feature_path)
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
            feats = _features(FLAGS.feature_path)
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
            feats = _features(FLAGS.feature_path)
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
