"""-m gpu: the streaming pointwise kernel (csrc/pw16.hip) through fte_conv2d_bn_fwd under bf16 storage at the shapes its planner and its
block map BRANCH on -- every default-reachable instantiation, 1 / 2 / 3 / 5 / 8 column tiles, grids with dead blocks, idle waves, 1 .. 11
tiles per wave, last tiles of 1 .. 6 rows, the caps on the row blocks, the hooked four-wave K = 256 forms -- plain and with the BN in front
folded into the loader.  tests/pw16_cases.py is the table, tests/pw16_map.py says which launch a case must make (asserted by EQUALITY with the
launch record) and how many partial rows it writes, tests/test_pw16_map_host.py proves on the CPU that the table reaches every class.  The
checks are tests/tile_worker.py's bn_exact (selection filter x position-coded input: z bit for bit) and bn_random (element-wise z, float64
statistics of the stored z), both with guard rows, canaries in every output and a NaN-filled workspace; hooked cases run them in a child
process.  Each check prints one `PW16_EDGE` line (pytest -s)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pw16_cases
import pw16_map

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

if torch.cuda.is_available():
    import tile_worker as tw
    from util_gpu import query


def _id(c):
    return 'x'.join(str(v) for v in c)


def _dims(case):
    M, K, N = case
    return (M, 1, 1, K, N, 1, 1)          # M = n * h * w: any factorisation will do


def _report(case, form, what, syms, errs, fails):
    print('PW16_EDGE %-16s %-6s %-6s %s  %s' % (_id(case), form, what, ','.join(syms), ' '.join('%s=%.3e' % kv for kv in sorted(errs.items()))))
    assert not fails, '%s %s %s %s:\n  ' % (_id(case), form, what, syms) + '\n  '.join(fails)


@pytest.mark.parametrize('fold', [False, True], ids=['plain', 'folded'])
@pytest.mark.parametrize('case', [c for c, _ in pw16_cases.CASES], ids=_id)
def test_edge(case, fold):
    M, K, N = case
    L = pw16_map.launch(M, K, N, fold=fold)
    assert query('fte_conv2d_bn_fwd_folds', M, 1, 1, K, N, 1, 1, 1) == 1
    form = 'folded' if fold else 'plain'
    for what, fn in (('exact', tw.bn_exact), ('random', tw.bn_random)):
        syms, errs, fails = fn(_dims(case), fold, L['nrb'])
        assert syms == [L['symbol']], (syms, L)
        _report(case, form, what, syms, errs, fails)


def test_below_the_floor_of_32_rows_runs_the_tile_kernels():
    """M = 31: pw16_plan refuses, fte_conv2d_bn_fwd_folds says 0, no pw16 symbol in the records -- and the results are still right"""
    case = pw16_cases.BELOW_FLOOR
    M, K, N = case
    assert pw16_map.launch(M, K, N) is None
    assert query('fte_conv2d_bn_fwd_folds', M, 1, 1, K, N, 1, 1, 1) == 0 and query('fte_conv2d_bn_fwd_folds', M + 1, 1, 1, K, N, 1, 1, 1) == 1
    for what, fn in (('exact', tw.bn_exact), ('random', tw.bn_random)):
        syms, errs, fails = fn(_dims(case), False, None)
        assert syms and not [s for s in syms if 'pw16' in s], syms
        _report(case, 'plain', what, syms, errs, fails)


def _run_hooked(cases, env, timeout=600):
    e = dict(os.environ)
    for k in ('FTE_PW16', 'FTE_PW16_BLOCKS', 'FTE_PW16_K256'):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, 'tile_worker.py'), json.dumps(cases)], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert lines, 'tile_worker produced no result line:\n' + r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(lines[-1])['cases'], r


HOOKED_ENVS = sorted({tuple(sorted(e.items())) for _, e, _ in pw16_cases.HOOKED})


@pytest.mark.parametrize('env', HOOKED_ENVS, ids=lambda e: ','.join('%s=%s' % kv for kv in e))
def test_edge_hooked(env):
    """FTE_PW16_BLOCKS / FTE_PW16_K256 are read once per process: one child per environment, every case of it plain and folded"""
    env = dict(env)
    mine = [c for c, e, _ in pw16_cases.HOOKED if e == env]
    cases = [[kind] + list(_dims(c)[:5]) + [1] for c in mine for kind in ('bnfwd1', 'bnfold1')]
    res, proc = _run_hooked(cases, env)
    assert len(res) == len(cases)
    for c in res:
        kind, M, _, _, K, N, _ = c['case']
        L = pw16_map.launch(M, K, N, fold=kind == 'bnfold1', **pw16_cases.hooks(env))
        errs = {k: v for k, v in c['errors'].items() if isinstance(v, (int, float))}
        assert c['errors']['symbols_per_call'] == [[L['symbol']], [L['symbol']]], (c['errors']['symbols_per_call'], L)
        _report((M, K, N), 'folded' if kind == 'bnfold1' else 'plain', 'both', c['symbols'], errs, c['errors']['fails'])
        assert c['ok']
    assert proc.returncode == 0, proc.stderr[-4000:]


# ---- hard statistics -----------------------------------------------------------------------------------------------------------------
KINDS = ['const', 'alt', 'drift', 'single', 'late', 'normal', 'normal', 'normal']
# per-channel limits: the module limits of tests/test_gpu_bn_fusion.py made relative to the channel --
# |mean - ref| <= 2e-6 max(1, max|z_c|), |rstd - ref| <= 4e-6 max(1, rstd_ref_c).  Measured on MI355X (error / scale, 64 -> 64 | 64 -> 192
# at 66049 rows), none widened: mean <= 8.2e-8 on every kind; rstd const 7.8e-8 | 7.8e-8, alt 4.3e-8 | 4.3e-8, drift 3.7e-6 | 2.9e-6 (the
# first partial's mean is the outlier bn_finalize merges around), single 6.1e-8 | 1.0e-7, late 3.6e-7 | 1.3e-7, normal 7.6e-8 | 1.8e-7
HARD_MEAN, HARD_RSTD = 2e-6, 4e-6


def _hard_input(M, K, first_rows, r):
    """[M, K] bf16-exact columns, kind k mod 8: a constant | 100 + {0, 0.5} by row parity (mean = 200 x spread, at the bf16 step) | the
    first 256 rows near -8, the rest near +8 (the first partial's mean an outlier) | zero but one row | zero in the first tile of EVERY
    wave (rows < first_rows) | three normal columns"""
    x = tw._bf64(r.standard_normal((M, K)))
    m = np.arange(M)
    for k in range(K):
        kind, rep = KINDS[k % 8], k // 8
        if kind == 'const':
            x[:, k] = 1.5 * (1 + rep)
        elif kind == 'alt':
            x[:, k] = 100.0 + 0.5 * ((m + rep) % 2)
        elif kind == 'drift':
            x[:, k] = tw._bf64(np.where(m < 256, -8.0, 8.0) + 0.25 * r.standard_normal(M))
        elif kind == 'single':
            x[:, k] = 0.0
            x[(M - 1) if rep % 2 == 0 else (37 * rep) % M, k] = 1.0 + rep
        elif kind == 'late':
            x[:first_rows, k] = 0.0
    return x


@pytest.mark.parametrize('case', [c for c, _ in pw16_cases.HARD_STATS], ids=_id)
def test_hard_statistics(case):
    """crafted input columns copied to the output channels by a unit selection filter: the epilogue's shifted sums, the Chan merges of
    the half-waves and waves, and bn_finalize's merge around the first partial's mean, on channels that are no i.i.d. normal"""
    M, K, N = case
    L = pw16_map.launch(M, K, N)
    r = np.random.default_rng(33)
    x = _hard_input(M, K, L['nrb'] * L['nw'] * 32, r)
    assert L['nrb'] * L['nw'] * 32 < M
    wt, sel, _ = tw.selection_filter(K, N, unit=True)
    gamma = 1 + 0.2 * r.standard_normal(N); beta = 0.3 * r.standard_normal(N)
    mm = r.standard_normal(N) * 0.1; mv = 1 + 0.1 * r.random(N)
    o = tw.bn_fwd_call(tw._dev16(x), wt, _dims(case), gamma, beta, mm, mv, None, L['nrb'])
    assert o['symbols'] == [L['symbol']], (o['symbols'], L)
    assert not o['fails'], o['fails']
    zs = tw._host16(o['z16'])
    assert np.array_equal(zs, x[:, sel]), 'z is not the selected input columns'
    mean, var = zs.mean(axis=0), zs.var(axis=0)
    rstd = 1.0 / np.sqrt(var + tw.BN_EPS)
    em = np.abs(o['stats']['mean'] - mean) / np.maximum(1.0, np.abs(zs).max(axis=0))
    er = np.abs(o['stats']['rstd'] - rstd) / np.maximum(1.0, rstd)
    kinds = np.array([KINDS[k % 8] for k in sel])
    bad = []
    for kind in sorted(set(KINDS)):
        s = kinds == kind
        print('PW16_HARD %-16s %-7s channels %3d  mean err / scale %.3e (limit %.1e)  rstd err / scale %.3e (limit %.1e)' % (
            _id(case), kind, int(s.sum()), em[s].max(), HARD_MEAN, er[s].max(), HARD_RSTD))
        if em[s].max() > HARD_MEAN or er[s].max() > HARD_RSTD:
            bad.append((kind, float(em[s].max()), float(er[s].max())))
    # a constant channel: variance 0, rstd = 1 / sqrt(eps), finite
    c = kinds == 'const'
    assert np.all(var[c] == 0) and np.isfinite(o['stats']['rstd'][c]).all()
    assert not bad, bad
