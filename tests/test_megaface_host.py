"""CPU: the host half of the MegaFace protocol (verification.py megaface_*): genuine pairs and their CSR, noise removal, size
capping, thresholds -> counts -> ranks -> CMC with ties, the per-size TAR table, against hand-built answers and the float64
restatement (megaface_ref.py), and the verify.py --protocol megaface flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import megaface_ref as mr
from tf_face_toolbox_amd import verification as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_and_csr_with_singletons():
    labels = [7, 3, 7, 9, 3, 7, 5]                      # 7: rows 0, 2, 5; 3: rows 1, 4; 9 and 5 single
    ip, ig, off, single = V.megaface_pairs(labels)
    assert single == 2
    assert off.tolist() == [0, 2, 3, 5, 5, 6, 8, 8]
    assert list(zip(ip.tolist(), ig.tolist())) == [(0, 2), (0, 5), (1, 4), (2, 0), (2, 5), (4, 1), (5, 0), (5, 2)]
    rp, rg = mr.pairs(labels)
    assert ip.tolist() == rp.tolist() and ig.tolist() == rg.tolist()
    assert mr.singletons(labels) == 2
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 40, 300)
    ip, ig, off, single = V.megaface_pairs(lab)
    rp, rg = mr.pairs(lab)
    assert ip.tolist() == rp.tolist() and ig.tolist() == rg.tolist() and single == mr.singletons(lab)
    assert np.all(np.diff(off) == np.bincount(ip, minlength=300))
    ip, ig, off, single = V.megaface_pairs([1, 2, 3])
    assert len(ip) == 0 and off.tolist() == [0, 0, 0, 0] and single == 3


def test_exclusion_exact_and_suffix():
    paths = ['/mf/FlickrFinal2/a/b/123.jpg', 'b/123.jpg', '/mf/FlickrFinal2/c/123.jpg', 'x/ab/123.jpg', '/mf/z/9.jpg',
             '/mf/z/19.jpg', 'top.jpg']
    noise = ['b/123.jpg', '9.jpg', '/mf/z/19.jpg', 'op.jpg', '']
    keep = V.megaface_exclude(paths, noise)
    assert keep.tolist() == [False, False, True, True, False, False, True]
    assert keep.tolist() == mr.excluded(paths, [e for e in noise if e]).tolist()
    assert V.megaface_exclude(paths, []).all()


def test_size_capping_and_dedup():
    assert V.megaface_sizes([10, 100, 1000], 5000) == [(10, False), (100, False), (1000, False)]
    assert V.megaface_sizes([1000, 10, 100, 100, 10000, 100000], 500) == [(10, False), (100, False), (500, True)]
    assert V.megaface_sizes([10, 500, 1000], 500) == [(10, False), (500, False)]
    assert V.megaface_sizes([10, 100], 7) == [(7, True)]
    assert V.megaface_sizes([10, 100, 1000, 10000], 500) == mr.sizes([10, 100, 1000, 10000], 500)
    with pytest.raises(ValueError):
        V.megaface_sizes([0, 10], 100)
    with pytest.raises(ValueError):
        V.megaface_sizes([10], 0)


def _host_counts(scores_pd, thr, off):
    """what fte_megaface_scan's counts mean, on the host: counts[j] = #{d : s(p, d) >= thr[j]}"""
    out = np.zeros(len(thr), np.int64)
    for p in range(len(off) - 1):
        for j in range(off[p], off[p + 1]):
            out[j] = np.sum(scores_pd[p] >= thr[j])
    return out


def test_thresholds_counts_ranks_cmc_with_ties():
    labels = [0, 0, 0, 1, 1]
    ip, ig, off, _ = V.megaface_pairs(labels)
    # genuine scores in pair order: (0,1) .5 (0,2) .25 (1,0) .5 (1,2) .5 (2,0) .25 (2,1) .5 (3,4) .75 (4,3) .75
    scores = np.array([.5, .25, .5, .5, .25, .5, .75, .75], np.float32)
    thr, perm = V.megaface_thresholds(scores, off)
    assert thr.tolist() == [.5, .25, .5, .5, .5, .25, .75, .75]
    assert perm.tolist() == [0, 1, 2, 3, 5, 4, 6, 7]
    # distractor scores per probe (3 distractors): ties with a genuine score count against it
    spd = np.array([[.5, .1, .3], [.6, .5, .5], [.25, .25, -1], [.75, .8, .1], [.7, .0, .0]], np.float32)
    counts = _host_counts(spd, thr, off)
    rank = np.empty(len(ip), np.int64)
    rank[perm] = counts + 1
    assert rank.tolist() == [2, 3, 4, 4, 3, 1, 3, 1]
    c = V.megaface_cmc(rank, (1, 2, 3, 4, 5))
    assert c == {1: 2 / 8, 2: 3 / 8, 3: 6 / 8, 4: 1.0, 5: 1.0}
    assert c == mr.cmc(rank, (1, 2, 3, 4, 5))
    assert V.megaface_cmc(np.zeros(0, np.int64), (1,)) == {1: 'n/a'}
    assert V.megaface_report_ranks(1000) == (1, 5, 10, 100, 1000)
    assert V.megaface_report_ranks(999) == (1, 5, 10, 100, 1000)
    assert V.megaface_report_ranks(10, range(1, 11)) == tuple(range(1, 11))
    assert V.megaface_report_ranks(5, range(1, 11)) == (1, 2, 3, 4, 5, 6)
    # against the float64 restatement on a random set
    rng = np.random.default_rng(3)
    P = mr.vr.normalize(rng.standard_normal((30, 8)))
    D = mr.vr.normalize(rng.standard_normal((50, 8)))
    lab = rng.integers(0, 6, 30)
    ip, ig, off, _ = V.megaface_pairs(lab)
    sg = (P[ip] * P[ig]).sum(1)
    thr, perm = V.megaface_thresholds(sg, off)
    rank = np.empty(len(ip), np.int64)
    rank[perm] = _host_counts(P @ D.T, thr.astype(np.float64), off) + 1
    ref = mr.ranks(P, D, ip, ig, [50])[0]
    assert np.mean(rank == ref) > 0.99                   # thresholds are fp32-rounded here


def test_tar_table_per_size():
    nb = 256
    hg = np.zeros(nb, np.uint64)
    hg[200] = 90
    hg[100] = 10
    his = []
    for N in (1000, 100000, 2000000):
        hi = np.zeros(nb, np.uint64)
        hi[128] = N - 1
        hi[210] = 1
        his.append(hi)
    t = V.megaface_tar_table(hg, his, [1000, 100000, 2000000])
    assert [r['size'] for r in t] == [1000, 100000, 2000000] and [r['impostor'] for r in t] == [1000, 100000, 2000000]
    f = {r['size']: {x['far']: x for x in r['tar_at_far']} for r in t}
    assert f[1000][1e-6]['tar'] == 'n/a' and f[1000][1e-4]['tar'] == 'n/a'
    assert f[1000][1e-3]['tar'] == 0.9 and f[1000][1e-3]['achieved_far'] == 1e-3
    assert f[100000][1e-5]['tar'] == 0.9 and f[100000][1e-6]['tar'] == 'n/a'
    assert f[2000000][1e-6]['tar'] == 0.9 and f[2000000][1e-6]['achieved_far'] == 5e-7   # one impostor <= 1e-6 * 2M
    assert f[1000][1e-3]['threshold'] == -1.0 + 2.0 * 129 / nb
    for r, hi in zip(t, his):
        assert r['tar_at_far'] == V.tar_at_far(hg, hi)


def test_verify_help_lists_megaface():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    out = ' '.join(r.stdout.split())
    for flag in ('megaface', '--distractor_feature_path', '--distractor_list_path', '--distractor_exclude', '--distractor_sizes',
                 '--output_json'):
        assert flag in out
    import verify
    a = verify.build_parser().parse_args(['--protocol', 'megaface', '--feature_path', 'f', '--data_list_path', 'l'])
    assert a.distractor_sizes == '10,100,1000,10000,100000,1000000'
