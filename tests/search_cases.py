"""Host-only (numpy) inputs, expectations and case tables for the evaluation kernels of csrc/search.hip at the shapes and ties
their code branches on (tests/test_gpu_search_edges.py runs them on the GPU, tests/test_search_cases_host.py proves on the CPU
that the expectations are unique, so the GPU tests compare bit for bit).

The technique is that of tests/test_gpu_megaface.py: rows with 16 entries of +-1/4.  Every product of two entries is +-1/16, so
every dot product is an exact multiple of 1/16 in [-1, 1] and every fp32 partial sum of it is exact in any order: the score a
kernel computes IS the float64 score, whatever its k order, tile or slice.  Scores take at most 33 values, so ties are the rule,
and what a kernel does with them (the index tie-break of the top-k, the half-open bin edges, the >= of a rank) decides the output.
Written from the contracts of include/fte.h, independently of the package code."""
import numpy as np

import verify_ref as vr

CUS = 256                              # MI355X: the CU count the slice plans below are stated for


def exact_rows(rng, n, d, scale=0.25):
    """[n, d] float32, 16 entries of +-scale per row (d >= 16).  scale 0.25: norm exactly 1 and every dot product an exact
    multiple of 1/16 in fp32 (many ties); scale 0.5: norm 2, dot products multiples of 1/4 in [-4, 4]."""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, rng.choice(d, 16, replace=False)] = rng.choice([-scale, scale], 16)
    return x


# ------------------------------------------------------------------ expectations (float64)
def topk_expected(P, G, k, gallery_base=0, probe_base=0, exclude_self=False):
    """(scores float64 [m, k], index int64 [m, k]): per probe the k best gallery rows by (score descending, global index
    ascending), without the pair probe_base + i == gallery_base + j when exclude_self; (-inf, -1) where fewer than k remain;
    the index is gallery_base + j."""
    s = np.asarray(P, np.float64) @ np.asarray(G, np.float64).T
    m, n = s.shape
    out_s = np.full((m, k), -np.inf)
    out_i = np.full((m, k), -1, np.int64)
    order = np.argsort(-s, axis=1, kind='stable')           # stable: equal scores stay in index order
    for i in range(m):
        o = order[i]
        if exclude_self:
            o = o[o + gallery_base != probe_base + i]
        o = o[:k]
        out_s[i, :len(o)] = s[i, o]
        out_i[i, :len(o)] = o + gallery_base
    return out_s, out_i


def merge_expected(in_s, in_i, k):
    """in_s / in_i [m, lists, k] -> (scores float64 [m, k], index int64 [m, k]): the k best of the union of the slots with
    index >= 0 by (score descending, index ascending), padded with (-inf, -1)."""
    in_s = np.asarray(in_s, np.float64)
    in_i = np.asarray(in_i, np.int64)
    m = in_s.shape[0]
    out_s = np.full((m, k), -np.inf)
    out_i = np.full((m, k), -1, np.int64)
    for r in range(m):
        s, i = in_s[r].ravel(), in_i[r].ravel()
        real = i >= 0
        s, i = s[real], i[real]
        o = np.lexsort((i, -s))[:k]
        out_s[r, :len(o)] = s[o]
        out_i[r, :len(o)] = i[o]
    return out_s, out_i


def hist_expected(A, la, B, lb, same, nbins):
    """(genuine, impostor) uint64 [nbins]: every pair (i of A, j of B), only i < j when same; the float64 score rounded to fp32
    goes to verify_ref.bins (fte.h's fp32 bin expression), of genuine when la[i] == lb[j]."""
    s = (np.asarray(A, np.float64) @ np.asarray(B, np.float64).T).astype(np.float32)
    la, lb = np.asarray(la), np.asarray(lb)
    keep = np.ones(s.shape, bool)
    if same:
        keep = np.arange(s.shape[0])[:, None] < np.arange(s.shape[1])[None, :]
    g = la[:, None] == lb[None, :]
    b = vr.bins(s, nbins)
    hg = np.bincount(b[keep & g], minlength=nbins).astype(np.uint64)
    hi = np.bincount(b[keep & ~g], minlength=nbins).astype(np.uint64)
    return hg, hi


def set_score_expected(x, rowsA, rowsB):
    """the float64 sum of the |A| |B| scores divided by |A| |B| (fte_set_pair_scores at beta = 0)"""
    x = np.asarray(x, np.float64)
    s = x[np.asarray(rowsA, np.int64)] @ x[np.asarray(rowsB, np.int64)].T
    return float(s.sum() / s.size)


# ------------------------------------------------------------------ the top-k slice plan (restated from s_topk_slices)
def topk_slices(m, n, cus=CUS):
    """gallery slices of the partial pass: about 8 one-wave blocks per CU over the 32-probe blocks, at most 64 (the merge's
    lists) and at most one per 64-row step"""
    ptiles, nsteps = (m + 31) // 32, (n + 63) // 64
    S = (8 * cus + ptiles - 1) // ptiles
    return max(1, min(S, 64, nsteps))


def steps_per_slice(m, n, cus=CUS):
    nsteps = (n + 63) // 64
    S = topk_slices(m, n, cus)
    return (nsteps + S - 1) // S


def empty_slices(m, n, cus=CUS):
    """trailing slices that start at or past the last step and so write an empty list"""
    nsteps, S, sps = (n + 63) // 64, topk_slices(m, n, cus), steps_per_slice(m, n, cus)
    return sum(1 for s in range(S) if s * sps >= nsteps)


# ------------------------------------------------------------------ case tables
# fte_l2_normalize_rows: (n, d).  n % 4 != 0: a last block with idle waves; d < 64, == 64, 65: idle lanes, one pass, a second pass
NORMALIZE_SHAPES = [(1, 1), (3, 32), (5, 63), (4, 64), (7, 65), (9, 100), (2, 2048)]

# fte_pair_scores: (npairs, d), a diagonal through {1, 3, 4, 5, 257} x {1, 32, 63, 64, 65, 512} that covers every value of both
PAIR_SHAPES = [(1, 1), (3, 32), (4, 63), (5, 64), (257, 65), (1, 512), (257, 32), (3, 512), (5, 1)]

# fte_topk_search.  rows: 'random' (exact rows), 'dups' (200 copies of one gallery row, in every 64-row step), 'X' (probes and
# gallery are ranges of one set of 300 exact rows, d = 64).  slices / steps / empty: the launch at 256 CUs the case is for.
# ties: 'overflow' = some probe has more rows tied with its k-th score than places left for them (the tie rule decides WHICH rows
# come back); 'order' = k takes every candidate, so equal scores only have to come back in index order; None for n = 1.
X_ROWS, X_D, X_SEED = 300, 64, 77
TOPK_CASES = [
    dict(name='slices64_compact', m=33, n=16421, d=32, k=64, rows='random', seed=101, slices=64, steps=5, empty=12,
         ties='overflow', every_probe=True),
    dict(name='one_probe_slices_of_2', m=1, n=4133, d=32, k=10, rows='random', seed=102, slices=64, steps=2, empty=31,
         ties='overflow', every_probe=True),
    dict(name='many_probe_blocks', m=4101, n=4133, d=32, k=64, rows='random', seed=103, slices=16, steps=5, empty=3,
         ties='overflow', every_probe=True),
    dict(name='n1', m=1, n=1, d=32, k=1, rows='random', seed=104, slices=1, steps=1, empty=0, ties=None),
    dict(name='ragged_step_k_eq_n', m=5, n=63, d=64, k=63, rows='random', seed=105, slices=1, steps=1, empty=0, ties='order'),
    dict(name='full_step_k_eq_n', m=5, n=64, d=64, k=64, rows='random', seed=106, slices=1, steps=1, empty=0, ties='order'),
    dict(name='full_step_plus_one_row', m=5, n=65, d=96, k=64, rows='random', seed=107, slices=2, steps=1, empty=0,
         ties='overflow'),
    dict(name='more_duplicates_than_k', m=40, n=1000, d=64, k=64, rows='dups', seed=108, slices=16, steps=1, empty=0,
         ties='overflow'),
    dict(name='X_self_inside', m=300, n=300, d=64, k=10, rows='X', p0=0, g0=0, excl=1, slices=5, steps=1, empty=0,
         ties='overflow'),
    dict(name='X_self_inside_offset', m=70, n=129, d=64, k=10, rows='X', p0=100, g0=64, excl=1, slices=3, steps=1, empty=0,
         ties='overflow'),
    dict(name='X_self_outside', m=50, n=100, d=64, k=10, rows='X', p0=200, g0=0, excl=1, slices=2, steps=1, empty=0,
         ties='overflow'),
    # not in the list the issue gives: the self row is inside the chunk for probes 0..43 and, for the others, on the rows
    # 80..105 that the last step reads through the min(., n - 1) clamp
    dict(name='X_self_inside_for_some', m=70, n=80, d=64, k=10, rows='X', p0=100, g0=64, excl=1, slices=2, steps=1, empty=0,
         ties='overflow'),
    dict(name='X_k_eq_n_excl', m=33, n=33, d=64, k=33, rows='X', p0=10, g0=10, excl=1, slices=1, steps=1, empty=0, ties='order'),
]
DUP_POS = np.arange(200) * 5 + 2       # 2, 7, ..., 997: 12 or 13 in each 64-row step, 8 in the last (40 rows)
DUP_PROBES = 8                         # the first probes ARE the duplicated row: 200 gallery rows at score 1


def x_set():
    return exact_rows(np.random.default_rng(X_SEED), X_ROWS, X_D)


def topk_inputs(case):
    """(P [m, d], G [n, d]) float32 host rows of a TOPK_CASES entry"""
    m, n, d = case['m'], case['n'], case['d']
    if case['rows'] == 'X':
        X = x_set()
        return X[case['p0']:case['p0'] + m].copy(), X[case['g0']:case['g0'] + n].copy()
    rng = np.random.default_rng(case['seed'])
    P, G = exact_rows(rng, m, d), exact_rows(rng, n, d)
    if case['rows'] == 'dups':
        G[DUP_POS] = G[DUP_POS[0]]
        P[:DUP_PROBES] = G[DUP_POS[0]]
    return P, G


def topk_expected_of(case):
    P, G = topk_inputs(case)
    return topk_expected(P, G, case['k'], case.get('g0', 0), case.get('p0', 0), bool(case.get('excl', 0)))


# fte_topk_merge: m x lists x k; lists = 1 (a copy), 63 / 64 (the last lanes of the wave), k = 64 (the contract's largest)
MERGE_M, MERGE_LISTS, MERGE_K = (1, 5), (1, 2, 3, 63, 64), (1, 7, 64)
MERGE_SCORES = np.asarray([0.75, 0.5, 0.25, 0.0, -0.5], np.float32)


def merge_inputs(rng, m, lists, k):
    """(in_s float32, in_i int32) [m, lists, k]: per row a pool of disjoint indices dealt to the lists, each list sorted in the
    contract's order with scores from MERGE_SCORES (ties cross lists), some lists short and padded with (-inf, -1), some empty;
    the last row (m > 1) has every list empty."""
    in_s = np.full((m, lists, k), -np.inf, np.float32)
    in_i = np.full((m, lists, k), -1, np.int32)
    for r in range(m):
        if m > 1 and r == m - 1:
            continue
        pool = rng.permutation(lists * k * 3)[:lists * k].reshape(lists, k)
        for l in range(lists):
            fill = int(rng.choice([k, k, rng.integers(0, k + 1), 0]))
            if lists == 1 and r == 0:
                fill = k
            idx = pool[l, :fill]
            sc = rng.choice(MERGE_SCORES, fill)
            o = np.lexsort((idx, -sc.astype(np.float64)))
            in_s[r, l, :fill] = sc[o]
            in_i[r, l, :fill] = idx[o]
    return in_s, in_i


# fte_score_histograms.  same = 1: n around the 32-row b tile and the 64-row a step (triangle mask, tile skip, ragged clamps);
# same = 0: (na, nb) with one row, one tile, ragged tiles.  Labels 0..3 so both histograms fill.
HIST_D, HIST_SEED = 32, 55
HIST_SAME_N = [1, 2, 31, 32, 33, 63, 64, 65, 97, 130]
HIST_RECT = [(1, 1), (1, 33), (65, 1), (64, 32), (63, 31), (130, 97)]
HIST_NBINS = [256, 8192]
HIST_CHUNK_ROWS = [130, 64, 33, 7]


def hist_set(n=130, d=HIST_D, scale=0.25, seed=HIST_SEED):
    """(rows, labels): exact rows with random labels 0..3"""
    rng = np.random.default_rng(seed)
    return exact_rows(rng, n, d, scale), rng.integers(0, 4, n).astype(np.int32)


def hist_dup_set():
    """97 rows, 40 of them copies of earlier rows: pairs with s == 1.0f, which the clamp sends to the last bin"""
    x, lab = hist_set(97, 64, seed=56)
    x[50:90] = x[5:45]
    lab[50:90] = lab[5:45]
    lab[60:70] = (lab[15:25] + 1) % 4   # ten of the copies under another label: 1.0 in the impostor histogram too
    return x, lab


# fte_template_pool
POOL_D = [1, 63, 64, 65, 512, 513, 1024, 1100]          # 64 * PC = 512: the register path up to 512, column chunks beyond
POOL_NT = [1, 5]
POOL_MEDIA = [1, 3, 4, 5, 8, 9]                         # members per media around PU = 4 rows in flight
POOL_BITWISE_D = [65, 512, 513, 1100]


def pool_lists(nt):
    """CSR lists of nt templates over rows 0 .. n - 1; template t has t % 3 + 1 media, media sizes cycle through POOL_MEDIA"""
    members, media_off, tmpl_off = [], [0], [0]
    q = 0
    for t in range(nt):
        for _ in range(t % 3 + 1):
            c = POOL_MEDIA[q % len(POOL_MEDIA)]
            members.extend(range(len(members), len(members) + c))
            media_off.append(len(members))
            q += 1
        tmpl_off.append(len(media_off) - 1)
    return np.asarray(members, np.int32), np.asarray(media_off, np.int32), np.asarray(tmpl_off, np.int32)


def pool_exact_lists():
    """templates whose pooled sum is exact in fp32 for small-integer rows and weight 1: media of 1, 2 or 4 members (the mean
    divides by a power of two).  Returns (members, media_off, tmpl_off)"""
    sizes = [[1], [2], [4], [1, 2, 4], [4, 4, 2, 1, 1], [2, 2]]
    members, media_off, tmpl_off = [], [0], [0]
    for t in sizes:
        for c in t:
            members.extend(range(len(members), len(members) + c))
            media_off.append(len(members))
        tmpl_off.append(len(media_off) - 1)
    return np.asarray(members, np.int32), np.asarray(media_off, np.int32), np.asarray(tmpl_off, np.int32)


def pool_exact_sum(x, members, media_off, tmpl_off):
    """v [n_templates, d] in float64 for pool_exact_lists-like templates (weight 1): exact, and equal to its fp32 rounding"""
    x = np.asarray(x, np.float64)
    v = np.zeros((len(tmpl_off) - 1, x.shape[1]))
    for t in range(len(tmpl_off) - 1):
        for m in range(tmpl_off[t], tmpl_off[t + 1]):
            r = members[media_off[m]:media_off[m + 1]]
            v[t] += x[r].sum(0) / len(r)
    return v


# fte_set_pair_scores: template sizes around the 16 x 16 tile and the two-tile step; every ordered pair
SET_SIZES = [1, 15, 16, 17, 31, 32, 33, 48]
SET_D = [32, 64, 512]
SET_NPAIRS = [1, 5, 64]
SET_TOL = 2.0 ** -22                   # one fp32 division: <= 2^-24; one miscounted element: >= 1 / (16 * 48 * 48) = 2.7e-5
SET_BETAS = list(range(0, 41, 2))


def set_lists():
    """(members, media_off, tmpl_off, rows per template): template t is SET_SIZES[t] consecutive rows, one media each"""
    off = np.concatenate([[0], np.cumsum(SET_SIZES)])
    members = np.arange(off[-1], dtype=np.int32)
    rows = [np.arange(off[t], off[t + 1]) for t in range(len(SET_SIZES))]
    return members, off.astype(np.int32), np.arange(len(SET_SIZES) + 1, dtype=np.int32), rows


def set_rows(d, seed=66):
    return exact_rows(np.random.default_rng(seed + d), int(np.sum(SET_SIZES)), d)


# MegaFace: pairs around the 32-pair wave, probes around MF_MP = 64 against rows around the 64-row step
MF_NPAIRS = [1, 31, 32, 33, 65]
MF_M = [1, 63, 64, 65]
MF_N = [1, 63, 64, 65, 129]
MF_D = 64


def mf_sets(m, n, seed=88):
    """(probes [m, d], labels [m], distractors [n, d]): identities of three rows, so every probe but a last odd one has pairs"""
    rng = np.random.default_rng(seed + 1000 * m + n)
    return exact_rows(rng, m, MF_D), (np.arange(m) // 3).astype(np.int64), exact_rows(rng, n, MF_D)
