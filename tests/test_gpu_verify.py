"""-m gpu: the evaluation path (include/fte.h "Evaluation: similarity search and score statistics", verification.py, verify.py)
against the float64 restatement (tests/verify_ref.py): normalisation, pair scores, fused top-k, fused score histograms, the
C-ABI error codes, determinism across calls and chunkings, and the three verify.py protocols end to end."""
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest
import torch

import verify_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from tf_face_toolbox_amd import _lib, verification as V

TOL = 2e-6


def _rows(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _norm_dev(x):
    return V.normalize(torch.from_numpy(x).cuda())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_normalize_and_pair_scores():
    rng = np.random.default_rng(1)
    x = _rows(rng, 300, 100) * rng.uniform(0.01, 50, (300, 1)).astype(np.float32)
    x[7] = 0.0                                                   # zero row: stays zero (max(|x|, eps))
    y, norms = V.normalize(torch.from_numpy(x).cuda(), return_norms=True)
    assert y.shape == (300, 128) and torch.all(y[:, 100:] == 0)
    yh = y.cpu().numpy().astype(np.float64)
    ref = vr.normalize(x)
    assert np.abs(yh[:, :100] - ref).max() <= TOL
    assert np.abs(norms.cpu().numpy() - np.linalg.norm(x.astype(np.float64), axis=1)).max() <= 1e-6 * np.linalg.norm(x, axis=1).max()
    ia = rng.integers(0, 300, 6000)
    ib = rng.integers(0, 300, 6000)
    got = V.pair_scores(y, ia, ib).cpu().numpy()
    assert np.abs(got - vr.pair_scores(ref, ia, ib)).max() <= TOL
    # aliasing x == y through the C ABI gives the same bits as a separate output
    a = torch.from_numpy(x[:, :96].copy()).cuda()
    b = torch.empty_like(a)
    _lib.call('fte_l2_normalize_rows', a, b, None, 300, 96, _stream())
    _lib.call('fte_l2_normalize_rows', a, a, None, 300, 96, _stream())
    assert torch.equal(a, b)


def _check_topk(P, Gm, k, s, i, exclude_self=False):
    """P, Gm: normalised float32 host rows; s, i: the GPU result"""
    ref = P.astype(np.float64) @ Gm.astype(np.float64).T
    m, n = ref.shape
    assert s.shape == (m, k) and i.shape == (m, k)
    for r in range(m):
        idx = i[r]
        real = idx >= 0
        want_real = min(k, n - (1 if exclude_self else 0))
        assert real.sum() == want_real, (r, idx)
        idx = idx[real]
        assert len(set(idx.tolist())) == len(idx)
        assert np.all(idx < n)
        if exclude_self:
            assert r not in idx
        assert np.abs(s[r, real] - ref[r, idx]).max() <= TOL, r
        sr = s[r, real]
        assert np.all((sr[:-1] > sr[1:]) | ((sr[:-1] == sr[1:]) & (idx[:-1] < idx[1:]))), r      # the order of fte.h
        rest = np.ones(n, bool)
        rest[idx] = False
        if exclude_self:
            rest[r] = False
        if rest.any() and len(idx):
            assert ref[r, rest].max() <= sr[-1] + TOL, r


SHAPES = [(1, 1, 32, 1), (1, 63, 512, 10), (33, 65, 2048, 64), (33, 63, 32, 1), (257, 65, 512, 64), (257, 100003, 512, 10),
          (33, 100003, 2048, 64), (1, 100003, 32, 64), (257, 63, 2048, 10), (33, 1000, 100, 10)]


@pytest.mark.parametrize('m,n,d,k', SHAPES)
def test_topk_against_float64(m, n, d, k):
    rng = np.random.default_rng(m * 7 + n + d + k)
    P = _norm_dev(_rows(rng, m, d))
    G = _norm_dev(_rows(rng, n, d))
    s, i = V.topk_search(P, G, k)
    _check_topk(P.cpu().numpy(), G.cpu().numpy(), k, s.cpu().numpy(), i.cpu().numpy())


def test_topk_duplicates_come_back_in_index_order_and_exclude_self():
    rng = np.random.default_rng(5)
    base = _rows(rng, 200, 64)
    G = np.concatenate([base, base[:50], base[:50]])          # rows j, 200 + j and 250 + j equal for j < 50
    Gd = _norm_dev(G)
    s, i = V.topk_search(Gd[:50], Gd, 3)
    i = i.cpu().numpy()
    s = s.cpu().numpy()
    assert np.array_equal(i, np.stack([np.arange(50), 200 + np.arange(50), 250 + np.arange(50)], 1))
    assert np.all(s[:, 0] == s[:, 1]) and np.all(s[:, 1] == s[:, 2])
    X = _norm_dev(_rows(rng, 333, 128))
    s, i = V.topk_search(X, X, 10, exclude_self=True)
    Xh = X.cpu().numpy()
    _check_topk(Xh, Xh, 10, s.cpu().numpy(), i.cpu().numpy(), exclude_self=True)
    s, i = V.topk_search(X[:5], X[:5], 5, exclude_self=True)          # k == n: the last slot is empty
    assert np.all(i.cpu().numpy()[:, 4] == -1) and np.all(np.isneginf(s.cpu().numpy()[:, 4]))


def test_c_abi_error_codes():
    rng = np.random.default_rng(2)
    P = _norm_dev(_rows(rng, 8, 64))
    G = _norm_dev(_rows(rng, 20, 64))
    s = torch.empty(8, 64, device='cuda')
    i = torch.empty(8, 64, dtype=torch.int32, device='cuda')
    wsb = _lib.query('fte_topk_search_ws_bytes', 8, 20, 64, 10)
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    q = lambda *a: _lib.query('fte_topk_search', *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])
    assert q(P, G, 8, 20, 64, 10, 0, 0, 0, s, i, ws, wsb, _stream()) == 0
    assert q(P, G, 8, 20, 64, 21, 0, 0, 0, s, i, ws, wsb, _stream()) == -1            # k > n
    assert q(P, G, 8, 20, 48, 10, 0, 0, 0, s, i, ws, wsb, _stream()) == -1            # d % 32
    assert q(P, G, 8, 20, 64, 65, 0, 0, 0, s, i, ws, wsb, _stream()) == -1            # k > 64
    assert q(P, G, 8, 20, 64, 10, 0, 0, 0, s, i, ws, wsb - 1, _stream()) == -2        # short ws
    assert q(P, G, 8, 20, 64, 10, 0, 0, 0, s, i, None, 0, _stream()) == -2
    h = torch.zeros(512, dtype=torch.int64, device='cuda')
    lab = torch.zeros(20, dtype=torch.int32, device='cuda')
    qh = lambda *a: _lib.query('fte_score_histograms', *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])
    assert qh(G, lab, 20, G, lab, 20, 64, 1, 512, h, h, _stream()) == 0
    assert qh(G, lab, 20, G, lab, 20, 64, 1, 384, h, h, _stream()) == -1              # not a power of two
    assert qh(G, lab, 20, G, lab, 20, 64, 1, 16384, h, h, _stream()) == -1
    assert qh(G, lab, 20, G, lab, 19, 64, 1, 512, h, h, _stream()) == -1              # same with na != nb
    assert qh(G, lab, 20, G, lab, 20, 48, 0, 512, h, h, _stream()) == -1
    torch.cuda.synchronize()


def _clustered(rng, n, d, classes):
    labels = rng.integers(0, classes, n)
    centers = _rows(rng, classes, d)
    x = centers[labels] + 0.9 * _rows(rng, n, d)
    return x.astype(np.float32), labels


def test_histograms_against_float64():
    rng = np.random.default_rng(11)
    nbins = 8192
    x, labels = _clustered(rng, 2500, 256, 250)
    X = _norm_dev(x)
    hg, hi = V.score_histograms(X, labels, nbins)
    rg, ri, s64, b64, g = vr.histograms(X.cpu().numpy(), labels, nbins)
    c = np.bincount(labels)
    ng = int(sum(comb(int(v), 2) for v in c))
    assert int(hg.sum()) == ng and int(hi.sum()) == comb(2500, 2) - ng
    amb = vr.edge_distance(s64, nbins) < 1e-6
    near = np.zeros(nbins, bool)
    for b in b64[amb]:
        near[max(b - 1, 0):b + 2] = True
    assert np.array_equal(hg[~near].astype(np.int64), rg[~near]) and np.array_equal(hi[~near].astype(np.int64), ri[~near])
    assert np.abs(hg.astype(np.int64) - rg).sum() + np.abs(hi.astype(np.int64) - ri).sum() <= 2 * amb.sum()


def test_determinism_across_calls_and_chunkings():
    rng = np.random.default_rng(13)
    n, d = 3001, 512
    x, labels = _clustered(rng, n, d, 300)
    X = _norm_dev(x)
    P = X[:257]
    ref = [t.cpu().numpy() for t in V.topk_search(P, X, 64)]
    again = [t.cpu().numpy() for t in V.topk_search(P, X, 64)]
    assert all(np.array_equal(a, b) for a, b in zip(ref, again))
    href = V.score_histograms(X, labels, 4096)
    for rows in (n, 1000, 97):
        got = [t.cpu().numpy() for t in V.topk_search(P, X, 64, chunk_rows=rows)]
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1]), rows
        h = V.score_histograms(X, labels, 4096, chunk_rows=rows)
        assert np.array_equal(h[0], href[0]) and np.array_equal(h[1], href[1]), rows
    assert np.array_equal(V.score_histograms(X, labels, 4096)[0], href[0])


def test_histogram_totals_beyond_32_bits():
    n, d = 92700, 512
    assert comb(n, 2) > 2 ** 32
    g = torch.Generator(device='cuda').manual_seed(3)
    X = V.normalize(torch.randn(n, d, device='cuda', generator=g))
    labels = np.arange(n) // 10                              # 9270 classes of 10
    hg, hi = V.score_histograms(X, labels, 8192)
    ng = 9270 * comb(10, 2)
    assert int(hg.sum()) == ng
    assert int(hi.sum()) == comb(n, 2) - ng


# ------------------------------------------------------------------ verify.py end to end
def _write_set(tmp, name, x, paths, labels):
    from scipy.io import savemat
    savemat(str(tmp / (name + '.mat')), {'wfea': x})
    with open(str(tmp / (name + '.txt')), 'w') as f:
        for p, l in zip(paths, labels):
            f.write('%s %d\n' % (p, l))
    return str(tmp / (name + '.mat')), str(tmp / (name + '.txt'))


def _verify(args, tmp):
    out = str(tmp / 'res.json')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py')] + args + ['--output_json', out], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.load(open(out)), r.stdout


def test_verify_cli_three_protocols(tmp_path):
    rng = np.random.default_rng(21)
    ids, per = 60, 10
    labels = np.repeat(np.arange(ids), per)
    centers = _rows(rng, ids, 100)
    x = (centers[labels] + 1.1 * _rows(rng, ids * per, 100)).astype(np.float32)
    names = ['Person_%02d' % c for c in range(ids)]
    paths = ['/lfw/%s/%s_%04d.jpg' % (names[l], names[l], j % per + 1) for j, l in enumerate(labels)]
    fmat, flist = _write_set(tmp_path, 'set', x, paths, labels)
    xn = vr.normalize(x)

    # pairs: 10 folds of 30 same + 30 different, in pairs.txt layout
    lines, same, ia, ib = ['10\t30'], [], [], []
    for f in range(10):
        for t in range(30):
            c = rng.integers(ids)
            a, b = rng.choice(per, 2, replace=False)
            lines.append('%s\t%d\t%d' % (names[c], a + 1, b + 1))
            same.append(True); ia.append(c * per + a); ib.append(c * per + b)
        for t in range(30):
            c1, c2 = rng.choice(ids, 2, replace=False)
            a, b = rng.integers(per, size=2)
            lines.append('%s\t%d\t%s\t%d' % (names[c1], a + 1, names[c2], b + 1))
            same.append(False); ia.append(c1 * per + a); ib.append(c2 * per + b)
    (tmp_path / 'pairs.txt').write_text('\n'.join(lines) + '\n')
    res, _ = _verify(['--protocol', 'pairs', '--feature_path', fmat, '--data_list_path', flist, '--pairs_path',
                      str(tmp_path / 'pairs.txt')], tmp_path)
    ref = vr.kfold_accuracy(vr.pair_scores(xn, ia, ib), same, 10)
    assert res['pairs'] == 600
    assert abs(res['accuracy'] - ref[0]) <= 1.5 / 60 and abs(res['std'] - ref[1]) <= 0.05

    # all pairs
    res, text = _verify(['--protocol', 'all_pairs', '--feature_path', fmat, '--data_list_path', flist], tmp_path)
    ng = ids * comb(per, 2)
    assert res['genuine'] == ng and res['impostor'] == comb(ids * per, 2) - ng
    rg, ri, s64, _, g = vr.histograms(xn, labels, 8192)
    refs = vr.tar_at_far_sorted(s64[g], s64[~g], 8192, (1e-6, 1e-5, 1e-4, 1e-3))
    for row, r in zip(res['tar_at_far'], refs):
        if r is None:
            assert row['tar'] == 'n/a'
        else:
            assert abs(row['tar'] - r[0]) <= 3.0 / ng and abs(row['threshold'] - r[2]) <= 2.0 * 2 / 8192
    assert 'n/a' in text

    # identify: leave-one-out, then a probe / gallery split
    res, _ = _verify(['--protocol', 'identify', '--feature_path', fmat, '--data_list_path', flist], tmp_path)
    _, idx = vr.topk(xn, xn, 10, exclude_self=True)
    ref = vr.cmc(idx, labels, labels, range(1, 11))
    for r in range(1, 11):
        assert abs(res['cmc'][str(r)] - ref[r]) <= 1.0 / len(labels), r
    probe = np.arange(len(labels)) % per == 0
    pmat, plist = _write_set(tmp_path, 'probe', x[probe], [p for p, q in zip(paths, probe) if q], labels[probe])
    gmat, glist = _write_set(tmp_path, 'gallery', x[~probe], [p for p, q in zip(paths, probe) if not q], labels[~probe])
    res, _ = _verify(['--protocol', 'identify', '--feature_path', pmat, '--data_list_path', plist, '--gallery_feature_path', gmat,
                      '--gallery_list_path', glist], tmp_path)
    _, idx = vr.topk(xn[probe], xn[~probe], 10)
    ref = vr.cmc(idx, labels[probe], labels[~probe], range(1, 11))
    assert not res['leave_one_out']
    for r in range(1, 11):
        assert abs(res['cmc'][str(r)] - ref[r]) <= 1.0 / probe.sum(), r
