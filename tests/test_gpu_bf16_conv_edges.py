"""-m gpu: the bf16 conv kernels (csrc/igemm16.hip: igemm16rw_kernel, igemm16p_kernel, igemm16_kernel; csrc/wgrad16.hip: wgrad16_kernel,
wgrad16p_kernel) at the shapes their windows and plans branch on -- non-square images (the 56x48 / 28x24 / 14x12 / 7x6 stages of a 112x96
run), every rung of the window-capacity ladder of igemm16_launch, one-tile / ragged / many-image tiles, one, three and six 64-channel
chunks, the 1x1 ladder, and the filter-gradient kernels at their capacity edges, both block maps and empty slot ranges.

Each case (tests/bf16_edge_cases.py) runs in a worker (tests/tile_worker.py, one process per environment: the planner's switches are read
once per process; FTE_PICK_WANT16 puts the 128-row tiles on these small shapes) and asserts
  * the recorded kernel symbol == the prediction of the host model tests/win16_map.py (which tests/test_win16_map_host.py checks on the
    CPU and against the host planner) -- if model and C++ drift apart, a test here fails;
  * the worker's checks: every stored bf16 value against the float64 oracle of the same bf16 inputs (2^-8 |ref| + 2e-5 scale), dw within
    2e-5 max-abs, dalpha / dbias within 2e-5 rel-L2; canaries (guard rows behind row M, no element unwritten, workspace tail untouched);
    and for 3x3 the EXACT placement of a position-coded input under a one-tap-per-channel filter, bit for bit.

Expectations corrected against the issue's table (the C++ decides; tests/test_win16_map_host.py CORRECTED):
  * 1x1 (2, 7, 6, 512, 64): M = 84 gives ONE tile of 256 x 64 and one of 128 x 64, so no FTE_PICK_WANT16 value selects the 128 x 64 tile;
    the launch runs on the register-staged 64 x 64 kernel (asserted: no igemm16 symbol).  The nearest shape that reaches the 128 x 64 forms,
    (4, 7, 6, 512, 64), M = 168, is added (three-stage ring igemm16_kernel<128,64,4,2,0,3,4,...>).
  * 1x1 filter gradient (3, 9, 7, 64, 128): 189 pixels are three K-pieces, fewer than wgrad16p_plan's four: refused (asserted), the
    per-tile result checked.  (1, 23, 11, 64, 128), 253 pixels = four pieces with a last piece of 61 rows, is added.
  * (5, 7, 7, 64, 128) and (5, 9, 7, 192, 128): the data gradients have N = 64 / 192, whose first candidate tile is 256 x 64; they run in
    the FTE_PICK_WANT16 = 2 / 8 groups (256 x 64 window kernel), the forwards with the N % 128 == 0 cases.

After a worker ends by a signal, exit 134 / 139 or its time limit, that test fails with the worker's stderr tail and every later test of
the module skips: nothing further is started on the GPU.

Measured on an MI355X host (16 CPUs): the module takes 18.3 s of wall time, 51 tests; the slowest worker is the default-environment one
(the 800-image case and the filter gradients) at 3.4 s, the others take 2.3-2.9 s each -- process start, float64 oracle and all.  Five
times that is below the floor, so every worker's time limit is the floor of 60 s."""
import json
import os
import subprocess
import sys
import time

import pytest

import bf16_edge_cases as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# seconds: 5 x the measured wall time of each worker (2.9, 2.4, 2.4, 2.3, 3.4, 2.4 s), floor 60
TIMEOUTS = {'want1': 60, 'want2': 60, 'want16': 60, 'want8': 60, 'default': 60, 'minp1': 60}
STATE = {'dead': None, 'results': {}, 'seconds': {}}
CASES = [(g, c[0]) for g, _, cases in E.GROUPS for c in cases]


def _worker(group):
    """results of the group's worker (started once): {case id: [worker records of its kinds]}"""
    if group in STATE['results']:
        return STATE['results'][group]
    if STATE['dead']:
        pytest.skip('nothing more is started on the GPU: ' + STATE['dead'])
    _, env, cases = next(g for g in E.GROUPS if g[0] == group)
    flat, where = E.worker_cases(cases)
    e = {k: v for k, v in os.environ.items() if not k.startswith('FTE_') or k == 'FTE_LIB'}
    e.update(env)
    e['FTE_MFMA_DTYPE'] = 'bf16s'
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, 'tile_worker.py'), json.dumps(flat)], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=TIMEOUTS[group])
    except subprocess.TimeoutExpired as x:
        STATE['dead'] = 'the worker of group %s ran into its time limit of %d s' % (group, TIMEOUTS[group])
        err = x.stderr.decode(errors='replace') if isinstance(x.stderr, bytes) else (x.stderr or '')
        pytest.fail(STATE['dead'] + '\n' + err[-4000:])
    STATE['seconds'][group] = time.time() - t0
    print('worker %s: %.1f s' % (group, STATE['seconds'][group]))
    if r.returncode < 0 or r.returncode in (134, 139):
        STATE['dead'] = 'the worker of group %s ended with status %d' % (group, r.returncode)
        pytest.fail(STATE['dead'] + '\n' + r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert lines, 'tile_worker produced no result line (exit %d):\n%s%s' % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    recs = json.loads(lines[-1])['cases']
    assert len(recs) == len(flat)
    out = {c[0]: recs[a:b] for c, (a, b) in zip(cases, where)}
    STATE['results'][group] = out
    return out


def _resident(symbols):
    return sorted(s for s in symbols if s.startswith(('igemm16', 'wgrad16')))


@pytest.mark.parametrize('group,cid', CASES, ids=['%s-%s' % gc for gc in CASES])
def test_case(group, cid):
    _, env, cases = next(g for g in E.GROUPS if g[0] == group)
    case = next(c for c in cases if c[0] == cid)
    recs = _worker(group)[cid]
    what, val = E.expected(case, env, cus=_cus())
    for rec in recs:
        print('%s %s: symbols %s splits %s errors %s' % (cid, rec['case'], rec['symbols'], rec['splits'], json.dumps(rec['errors'])))
    for rec in recs:
        if what == 'symbol':
            assert _resident(rec['symbols']) == ([val] if val else []), (cid, rec['case'], rec['symbols'], val)
            assert rec['symbols'], (cid, rec['case'])
        elif what == 'plan':
            assert _resident(rec['symbols']) == [val['symbol']] and rec['splits'] == [val['S']], (cid, rec['symbols'], rec['splits'], val)
        else:
            assert rec['symbols'] and not _resident(rec['symbols']), (cid, rec['symbols'])
        assert rec['ok'], 'check failure: %s' % json.dumps(rec)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count
