"""-m gpu: the MegaFace scan (include/fte.h "MegaFace", verification.py megaface_*, verify.py --protocol megaface) against the
float64 restatement (tests/megaface_ref.py): exact counts and histograms on exactly representable rows, bounds on Gaussian rows,
ties with a copied row, bucket boundaries, determinism across chunkings and calls, agreement with fte_score_histograms and
topk_search, bad CSR lists, the C-ABI error codes, and the CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import megaface_ref as mr
from search_cases import exact_rows
import verify_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from tf_face_toolbox_amd import _lib, verification as V


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _exact_rows(rng, n, d=64):
    """16 entries of +-0.25 per row: norm exactly 1, every dot product an exact multiple of 1/16 in fp32 (many ties)"""
    return exact_rows(rng, n, d)


def _clustered_exact(rng, ids, per, d=64):
    """rows of `ids` identities that share most of their signs with a centre row (high genuine scores, still exact)"""
    c = _exact_rows(rng, ids, d)
    labels = np.repeat(np.arange(ids), per)
    x = c[labels].copy()
    for i in range(len(x)):
        nz = np.nonzero(x[i])[0]
        flip = rng.choice(nz, rng.integers(0, 5), replace=False)
        x[i, flip] *= -1
    return x, labels


def _dev(x):
    return V.normalize(torch.from_numpy(np.ascontiguousarray(x)).cuda())


def _scan(P, D, labels, Ns, nbins=1024, chunk_rows=None):
    ip, ig, off, _ = V.megaface_pairs(labels)
    sg = V.megaface_pair_scores(P, ip, ig).cpu().numpy()
    thr, perm = V.megaface_thresholds(sg, off)
    counts, hist = V.megaface_scan(P, D, Ns, off, thr, nbins, chunk_rows)
    rank = np.empty((len(Ns), len(ip)), np.int64)
    rank[:, perm] = counts.astype(np.int64) + 1
    return ip, ig, sg, rank, counts, hist


def test_exact_rows_match_float64():
    rng = np.random.default_rng(11)
    x, labels = _clustered_exact(rng, 23, 9)
    labels[-1] = 99                                       # a single-image identity: no pair
    dx = _exact_rows(rng, 3000)
    dx[100:130] = x[rng.choice(len(x), 30)]               # exact copies of probe-set rows: ties with genuine scores
    P, D = _dev(x), _dev(dx)
    assert torch.equal(P.cpu(), torch.from_numpy(x)) and torch.equal(D.cpu(), torch.from_numpy(dx))
    Ns = [10, 100, 1000, 3000]
    ip, ig, sg, rank, _, hist = _scan(P, D, labels, Ns)
    rp, rg = mr.pairs(labels)
    assert ip.tolist() == rp.tolist() and ig.tolist() == rg.tolist()
    assert np.array_equal(sg.astype(np.float64), (x[ip].astype(np.float64) * x[ig]).sum(1))
    ref = mr.ranks(x, dx, ip, ig, Ns)
    assert np.array_equal(rank, ref)
    assert rank[-1].max() > 1 and (rank[-1] == 1).any()
    for b, N in enumerate(Ns):
        assert np.array_equal(hist[b], mr.impostor_hist(x, dx, N, 1024))


def test_gaussian_rows_between_strict_and_loose():
    rng = np.random.default_rng(12)
    ids, per, d = 12, 12, 128
    c = rng.standard_normal((ids, d))
    labels = np.repeat(np.arange(ids), per)
    x = (c[labels] + 1.6 * rng.standard_normal((ids * per, d))).astype(np.float32)
    dx = rng.standard_normal((5000, d)).astype(np.float32)
    P, D = _dev(x), _dev(dx)
    Ns = [64, 1000, 5000]
    ip, ig, sg, rank, _, _ = _scan(P, D, labels, Ns)
    Pn, Dn = P.cpu().numpy().astype(np.float64), D.cpu().numpy().astype(np.float64)
    assert np.abs(sg - (Pn[ip] * Pn[ig]).sum(1)).max() < 2e-6
    lo, hi = mr.counts_bounds(Pn, Dn, ip, ig, Ns)
    assert np.all(rank - 1 >= lo) and np.all(rank - 1 <= hi)
    assert rank[-1].max() > 1


def test_copied_row_ties_and_counts():
    rng = np.random.default_rng(13)
    ids, per, d = 8, 6, 512
    c = rng.standard_normal((ids, d))
    labels = np.repeat(np.arange(ids), per)
    x = (c[labels] + 0.8 * rng.standard_normal((ids * per, d))).astype(np.float32)
    dx = rng.standard_normal((9000, d)).astype(np.float32)
    g = 7
    for k in (4101, 8999):                                # a copy of probe-set row g in two buckets, off 64-row steps
        dx[k] = x[g]
    P, D = _dev(x), _dev(dx)
    assert torch.equal(D[4101], P[g])
    Ns = [100, 4101, 4102, 9000]
    ip, ig, sg, rank, _, _ = _scan(P, D, labels, Ns)
    sel = ig == g
    assert sel.sum() == per - 1
    assert np.all(rank[2][sel] >= 2) and np.all(rank[3][sel] >= 3)
    assert np.all(rank[3][sel] - rank[2][sel] >= 1) and np.all(rank[2][sel] - rank[1][sel] >= 1)


def test_bucket_boundaries_equal_prefix_scans():
    rng = np.random.default_rng(14)
    x, labels = _clustered_exact(rng, 10, 7)
    dx = _exact_rows(rng, 4097)
    P, D = _dev(x), _dev(dx)
    Ns = [10, 100, 1000, 4097]
    _, _, _, rank, counts, hist = _scan(P, D, labels, Ns)
    ip, ig, off, _ = V.megaface_pairs(labels)
    thr, _ = V.megaface_thresholds(V.megaface_pair_scores(P, ip, ig).cpu().numpy(), off)
    for b, N in enumerate(Ns):
        c1, h1 = V.megaface_scan(P, D[:N], [N], off, thr, 1024)
        assert np.array_equal(c1[0], counts[b]) and np.array_equal(h1[0], hist[b])
    assert np.array_equal(rank, mr.ranks(x, dx, ip, ig, Ns))


def test_determinism_across_chunkings_and_calls():
    rng = np.random.default_rng(15)
    ids, per, d = 20, 8, 96
    labels = np.repeat(np.arange(ids), per)
    x = (rng.standard_normal((ids, d))[labels] + 2.0 * rng.standard_normal((ids * per, d))).astype(np.float32)
    dx = rng.standard_normal((6000, d)).astype(np.float32)
    P, D = _dev(x), _dev(dx)
    Ns = [10, 1000, 6000]
    base = _scan(P, D, labels, Ns, 8192)
    assert base[3][-1].max() > 1
    for cr in (None, 1000, 97):
        r = _scan(P, D, labels, Ns, 8192, cr)
        assert np.array_equal(r[4], base[4]) and np.array_equal(r[5], base[5])


def test_histogram_matches_score_histograms_and_rank1_matches_topk():
    rng = np.random.default_rng(16)
    ids, per, d = 30, 5, 128
    labels = np.repeat(np.arange(ids), per)
    x = (rng.standard_normal((ids, d))[labels] + 1.5 * rng.standard_normal((ids * per, d))).astype(np.float32)
    dx = rng.standard_normal((3000, d)).astype(np.float32)
    P, D = _dev(x), _dev(dx)
    Ns = [700, 3000]
    ip, ig, sg, rank, _, hist = _scan(P, D, labels, Ns, 2048)
    m = P.shape[0]
    for b, N in enumerate(Ns):
        hg = torch.zeros(2048, dtype=torch.int64, device='cuda')
        hi = torch.zeros(2048, dtype=torch.int64, device='cuda')
        la = torch.zeros(N, dtype=torch.int32, device='cuda')
        lb = torch.ones(m, dtype=torch.int32, device='cuda')
        _lib.call('fte_score_histograms', D[:N].contiguous(), la, N, P, lb, m, d, 0, 2048, hg, hi, _stream())
        assert int(hg.sum()) == 0 and np.array_equal(hi.cpu().numpy().astype(np.uint64), hist[b])
        s1, _ = V.topk_search(P, D[:N], 1)
        top = s1.cpu().numpy()[:, 0]
        assert np.array_equal(rank[b] == 1, sg > top[ip])
        assert (rank[b] == 1).any() and (rank[b] > 1).any()


def test_bad_csr_lists_are_skipped():
    rng = np.random.default_rng(17)
    x, labels = _clustered_exact(rng, 6, 5)
    dx = _exact_rows(rng, 700)
    dx[10:20] = x[0:10]                                   # copies of identities 0 and 1: every one of their pairs counts
    P, D = _dev(x), _dev(dx)
    m, d = P.shape
    ip, ig, off, _ = V.megaface_pairs(labels)
    thr, _ = V.megaface_thresholds(V.megaface_pair_scores(P, ip, ig).cpu().numpy(), off)
    T = len(thr)
    good_c, good_h = V.megaface_scan(P, D, [700], off, thr, 512)
    bad = off.copy()
    bad[3] = T + 5                                        # probe 2 runs past the list, probe 3 decreases
    bad[6] = -1                                           # probes 5 and 6 start or end before it
    skipped = np.zeros(T, bool)
    for p in (2, 3, 5, 6):
        skipped[off[p]:off[p + 1]] = True
    c = torch.zeros(T, dtype=torch.int64, device='cuda')
    h = torch.zeros(512, dtype=torch.int64, device='cuda')
    wsb = _lib.query('fte_megaface_scan_ws_bytes', m, T)
    assert wsb == 8 * T
    ws = torch.full((wsb,), 7, dtype=torch.uint8, device='cuda')     # the call clears it
    t = torch.from_numpy(thr).cuda()
    _lib.call('fte_megaface_scan', P, m, D, 700, d, torch.from_numpy(bad.astype(np.int32)).cuda(), t, T, 512, c, h, ws, wsb, _stream())
    c = c.cpu().numpy().astype(np.uint64)
    assert np.array_equal(c[~skipped], good_c[0][~skipped]) and np.all(c[skipped] == 0)
    assert np.array_equal(h.cpu().numpy().astype(np.uint64), good_h[0])
    assert good_c[0][skipped].sum() > 0


def test_c_abi_error_codes():
    rng = np.random.default_rng(18)
    P = _dev(_exact_rows(rng, 8))
    D = _dev(_exact_rows(rng, 20))
    off = torch.tensor([0, 1, 2, 2, 2, 2, 2, 2, 2], dtype=torch.int32, device='cuda')
    thr = torch.tensor([0.5, 0.25], device='cuda')
    c = torch.zeros(2, dtype=torch.int64, device='cuda')
    h = torch.zeros(8192, dtype=torch.int64, device='cuda')
    wsb = _lib.query('fte_megaface_scan_ws_bytes', 8, 2)
    assert wsb == 16 and _lib.query('fte_megaface_scan_ws_bytes', 0, 2) == 0 and _lib.query('fte_megaface_scan_ws_bytes', 8, 0) == 0
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    q = lambda *a: _lib.query('fte_megaface_scan', *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])
    S = _stream()
    assert q(P, 8, D, 20, 64, off, thr, 2, 256, c, h, ws, wsb, S) == 0
    assert q(P, 8, D, 20, 64, off, thr, 2, 8192, c, h, ws, wsb, S) == 0
    assert q(None, 8, D, 20, 64, off, thr, 2, 256, c, h, ws, wsb, S) == -1
    assert q(P, 8, D, 20, 64, None, thr, 2, 256, c, h, ws, wsb, S) == -1
    assert q(P, 8, D, 20, 64, off, thr, 2, 256, None, h, ws, wsb, S) == -1
    assert q(P, 8, D, 20, 64, off, thr, 2, 256, c, None, ws, wsb, S) == -1
    assert q(P, 8, D, 20, 48, off, thr, 2, 256, c, h, ws, wsb, S) == -1               # d % 32
    assert q(P, 8, D, 20, 16, off, thr, 2, 256, c, h, ws, wsb, S) == -1
    for nb in (128, 384, 16384):                                                       # nbins outside 256..8192 / 2^k
        assert q(P, 8, D, 20, 64, off, thr, 2, nb, c, h, ws, wsb, S) == -1
    assert q(P, 0, D, 20, 64, off, thr, 2, 256, c, h, ws, wsb, S) == -1
    assert q(P, 8, D, 0, 64, off, thr, 2, 256, c, h, ws, wsb, S) == -1
    assert q(P, 8, D, 20, 64, off, thr, 0, 256, c, h, ws, wsb, S) == -1
    assert q(P, 8, D, 1 << 21, 512, off, thr, 2, 256, c, h, ws, wsb, S) == -1         # a 4 GiB distractor range
    assert q(P, 8, D, 20, 64, off, thr, 2, 256, c, h, ws, wsb - 1, S) == -2           # short ws
    assert q(P, 8, D, 20, 64, off, thr, 2, 256, c, h, None, 0, S) == -2
    ia = torch.tensor([0, 7, 8, -1, 3], dtype=torch.int32, device='cuda')
    ib = torch.tensor([19, 0, 0, 0, 20], dtype=torch.int32, device='cuda')
    out = torch.empty(5, device='cuda')
    qp = lambda *a: _lib.query('fte_megaface_pair_scores', *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])
    assert qp(P, 8, D, 20, 64, ia, ib, 5, out, S) == 0
    o = out.cpu().numpy()
    Ph, Dh = P.cpu().numpy(), D.cpu().numpy()
    assert o[0] == np.dot(Ph[0].astype(np.float64), Dh[19]) and o[1] == np.dot(Ph[7].astype(np.float64), Dh[0])
    assert np.isnan(o[2:]).all()                                                       # an index outside its set
    assert qp(P, 8, D, 20, 48, ia, ib, 5, out, S) == -1
    assert qp(P, 8, D, 20, 64, ia, None, 5, out, S) == -1
    assert qp(P, 8, D, 20, 64, ia, ib, 0, out, S) == -1
    assert qp(P, 8, D, 1 << 21, 512, ia, ib, 5, out, S) == -1
    torch.cuda.synchronize()


def _write(tmp, name, x, lines):
    from scipy.io import savemat
    savemat(str(tmp / (name + '.mat')), {'wfea': x})
    with open(str(tmp / (name + '.txt')), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return str(tmp / (name + '.mat')), str(tmp / (name + '.txt'))


def test_verify_cli_megaface(tmp_path):
    rng = np.random.default_rng(19)
    x, labels = _clustered_exact(rng, 15, 8)
    labels[0] = 77                                        # one single-image identity
    dx = _exact_rows(rng, 2600)
    dx[50] = x[3]
    dpaths = ['/mf/FlickrFinal2/%03d/%d_%d.jpg' % (i % 97, i, i % 7) for i in range(len(dx))]
    noise = [dpaths[5][len('/mf/FlickrFinal2/'):], dpaths[77], '%d_%d.jpg' % (300, 300 % 7)]
    (tmp_path / 'noise.txt').write_text('\n'.join(noise) + '\n')
    keep = mr.excluded(dpaths, noise)
    assert (~keep).sum() == 3
    fmat, flist = _write(tmp_path, 'fs', x, ['fs/%d/%d.png %d' % (l, i, l) for i, l in enumerate(labels)])
    dmat, dlist = _write(tmp_path, 'dis', dx, dpaths)
    out = str(tmp_path / 'mf.json')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py'), '--protocol', 'megaface', '--feature_path', fmat,
                        '--data_list_path', flist, '--distractor_feature_path', dmat, '--distractor_list_path', dlist,
                        '--distractor_exclude', str(tmp_path / 'noise.txt'), '--distractor_sizes', '10,100,1000,10000,100000',
                        '--nbins', '1024', '--output_json', out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    kept = dx[keep]
    assert res['excluded'] == 3 and res['kept'] == len(kept) and res['distractors'] == len(dx)
    assert res['singletons'] == 1 and res['probes'] == len(x)
    ip, ig = mr.pairs(labels)
    assert res['genuine_pairs'] == len(ip)
    sizes = mr.sizes([10, 100, 1000, 10000, 100000], len(kept))
    assert [(s['size'], s['capped']) for s in res['sizes']] == [(N, c) for N, c in sizes]
    assert sizes[-1] == (len(kept), True)
    Ns = [N for N, _ in sizes]
    ref = mr.ranks(x, kept, ip, ig, Ns)
    iu = [(i, j) for i in range(len(x)) for j in range(i + 1, len(x)) if labels[i] == labels[j]]
    gen = np.array([np.dot(x[i].astype(np.float64), x[j]) for i, j in iu], np.float32)
    hg = np.bincount(vr.bins(gen, 1024), minlength=1024).astype(np.uint64)
    for b, s in enumerate(res['sizes']):
        N = s['size']
        ks = V.megaface_report_ranks(N, range(1, 11))
        assert s['cmc'] == {str(k): v for k, v in mr.cmc(ref[b], ks).items()}
        assert s['rank1'] == mr.cmc(ref[b], [1])[1]
        assert s['impostor'] == len(x) * N
        want = V.tar_at_far(hg, mr.impostor_hist(x, kept, N, 1024))
        assert s['tar_at_far'] == json.loads(json.dumps(want))
    assert 'size %d (capped' % len(kept) in r.stdout and 'rank-1' in r.stdout
