"""CPU: the host half of the evaluation path (tf_face_toolbox_amd/verification.py) -- the pairs.txt parser and row mapping,
the k-fold protocol, TAR@FAR from histograms, CMC -- against hand-built answers and the float64 restatement (verify_ref.py),
and the verify.py command line surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verify_ref as vr
from tf_face_toolbox_amd import verification as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_parser_and_row_mapping(tmp_path):
    p = tmp_path / 'pairs.txt'
    p.write_text('2\t2\nAlice\t1\t2\nBob\t1\t3\nAlice\t1\tBob\t2\nCarol\t1\tBob\t1\n'
                 'Carol\t1\t2\nAlice\t2\t1\nBob\t3\tCarol\t2\nAlice\t2\tCarol\t1\n')
    pairs, same, folds = V.read_lfw_pairs(str(p))
    assert folds == 2 and len(pairs) == 8
    assert pairs[0] == ('Alice', 1, 'Alice', 2) and pairs[2] == ('Alice', 1, 'Bob', 2)
    assert same.tolist() == [True, True, False, False, True, True, False, False]
    images = ['/data/lfw/Alice/Alice_0001.jpg', '/data/lfw/Alice/Alice_0002.jpg', 'lfw/Bob/Bob_0001.png', 'lfw/Bob/Bob_0002.png',
              'lfw/Bob/Bob_0003.png', 'Carol/Carol_0001.jpg', 'x/Carol/Carol_0002.jpg', 'x/NotAlice/Alice_0001.jpg']
    ia, ib = V.map_pairs_to_rows(pairs, images)
    assert ia.tolist() == [0, 2, 0, 5, 5, 1, 4, 1]
    assert ib.tolist() == [1, 4, 3, 2, 6, 0, 6, 5]
    with pytest.raises(KeyError):
        V.map_pairs_to_rows([('Dave', 1, 'Dave', 2)], images)


def test_kfold_accuracy_hand_built():
    # fold 1 = [0.9 s, 0.1 d], fold 2 = [0.8 s, 0.85 d]
    scores = [0.9, 0.1, 0.8, 0.85]
    same = [True, False, True, False]
    mean, std, thr = V.kfold_accuracy(scores, same, folds=2)
    # test fold 1 trains on fold 2: t = 0.8 -> 1/2 and t = 0.85 -> 0/2 ... candidates 0.8, 0.85, inf give 1/2, 0/2, 1/2: the smallest
    assert thr[0] == 0.8
    # test fold 2 trains on fold 1: t = 0.1 -> 1/2, t = 0.9 -> 2/2, inf -> 1/2
    assert thr[1] == 0.9
    assert mean == pytest.approx((1.0 + 0.5) / 2) and std == pytest.approx(0.25)
    assert (mean, std, thr) == vr.kfold_accuracy(scores, same, 2)


def test_kfold_accuracy_ties_take_the_smallest_threshold():
    scores = [0.5, 0.5, 0.5, 0.5, 0.2, 0.2]
    same = [True, False, True, False, True, False]
    mean, std, thr = V.kfold_accuracy(scores, same, folds=3)
    assert (mean, std, thr) == vr.kfold_accuracy(scores, same, 3)
    assert all(t in (0.2, 0.5) for t in thr)


def test_kfold_accuracy_separable_and_random():
    rng = np.random.default_rng(3)
    same = np.tile([True] * 30 + [False] * 30, 10)
    s = np.where(same, rng.uniform(0.5, 1.0, same.size), rng.uniform(-1.0, 0.4, same.size))
    s[::60] = 0.5                                      # every fold holds the lowest genuine score: no test fold falls below it
    assert V.kfold_accuracy(s, same)[:2] == (1.0, 0.0)
    s = rng.normal(size=600).round(2)                  # many ties
    same = rng.random(600) < 0.5
    got = V.kfold_accuracy(s, same)
    ref = vr.kfold_accuracy(s, same)
    assert got[0] == pytest.approx(ref[0], abs=1e-12) and got[1] == pytest.approx(ref[1], abs=1e-12) and got[2] == ref[2]


def test_tar_at_far_matches_sorted_scores_on_bin_edges():
    nbins = 256
    rng = np.random.default_rng(7)
    edges = -1.0 + 2.0 * np.arange(nbins) / nbins
    gen = edges[rng.integers(150, 256, 3000)]
    imp = edges[rng.integers(0, 200, 20000)]
    hg = np.bincount(vr.bins(gen, nbins), minlength=nbins)
    hi = np.bincount(vr.bins(imp, nbins), minlength=nbins)
    fars = (1e-5, 1e-3, 1e-2)
    got = V.tar_at_far(hg, hi, fars)
    ref = vr.tar_at_far_sorted(gen, imp, nbins, fars)
    assert got[0]['tar'] == 'n/a' and ref[0] is None       # 20 000 impostors < 1 / 1e-5
    for g, r in zip(got[1:], ref[1:]):
        assert (g['tar'], g['achieved_far'], g['threshold']) == pytest.approx(r, abs=1e-12)
        assert g['achieved_far'] <= g['far']


def test_tar_at_far_reports_na_when_impostors_are_too_few():
    hg = np.zeros(256, np.uint64)
    hi = np.zeros(256, np.uint64)
    hg[200] = 10
    hi[10] = 999
    got = V.tar_at_far(hg, hi, fars=(1e-3, 1e-2))
    assert got[0]['tar'] == 'n/a' and got[0]['threshold'] == 'n/a'
    assert got[1]['tar'] == 1.0 and got[1]['achieved_far'] == 0.0


def test_cmc_hand_built():
    gl = np.array([0, 1, 2, 0, 1])
    pl = np.array([0, 1, 2, 3])
    index = np.array([[3, 1, 2], [0, 2, 4], [1, -1, -1], [0, 1, 2]])
    got = V.cmc(index, pl, gl, ranks=(1, 2, 3))
    assert got == {1: 0.25, 2: 0.25, 3: 0.5}
    assert got == vr.cmc(index, pl, gl, (1, 2, 3))


def test_verify_cli_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ('--protocol', 'pairs', 'all_pairs', 'identify', '--pairs_path', '--gallery_feature_path', '--gallery_list_path'):
        assert flag in out.stdout
