"""CPU: the conv planner (csrc/conv_plan.h) compiled alone with g++ answers what tests/golden/conv_plans.json recorded from the planner
before it became a header -- every field of every plan, for every case and environment of tests/conv_plan_cases.py -- the table hits
every branch it names, the built library's *_ws_bytes queries equal the recorded ones, and on two other device sizes the plans keep the
invariants the launches rely on."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import conv_plan_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_recording():
    """the recording in full: it is written short (its own `format` entry says how)"""
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_plans.json')))
    rows = lambda rp: rp + [0] * (10 - len(rp))

    def ctx(v):
        if isinstance(v, list):
            return rows(v)
        v = dict(v, **{k: rows(v[k]) for k in ('fwd', 'fwd_nows') if k in v})
        if 'fwd' in v:
            v.setdefault('fwd_nows', v['fwd'])
        if 'cls' in v:
            v['cls'] = [k[:4] + [rows(k[4])] for k in v['cls']]
        return v
    for recs in gold['plans'].values():
        for r in recs:
            if 'ctx' in r:
                full = {}
                for k, v in r['ctx'].items():
                    full[k] = full[v] if isinstance(v, str) else ctx(v)
                r['ctx'] = full
    for per_case in gold['ws'].values():
        for case, ans in per_case.items():
            per_algo = ans if isinstance(ans[0], list) else [ans] * 3
            k3 = case.split()[6] == '3'
            per_case[case] = [a + (a[:3] if k3 else []) for a in per_algo for _dtype in (0, 1)]
    return gold


GOLD = _load_recording()
ENVS = C.by_environment()
BPC = GOLD['device']['sk_blocks_per_cu']
CONV_Q = ['fte_conv2d_fwd_ws_bytes', 'fte_conv2d_dgrad_ws_bytes', 'fte_conv2d_wgrad_ws_bytes', 'fte_conv2d_dgrad_bn_ws_bytes']
CONV3_Q = ['fte_conv3x3_fwd_ws_bytes', 'fte_conv3x3_dgrad_ws_bytes', 'fte_conv3x3_wgrad_ws_bytes']


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('conv_plan') / 'conv_plan_dump')
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'conv_plan_dump.cpp')])
    return exe


def run_dump(exe, tmp_path, env, cases, cus=None, layouts=False):
    path = str(tmp_path / 'cases.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(C.case_line(c) for c in cases) + '\n')
    e = {k: v for k, v in os.environ.items() if not k.startswith('FTE_')}
    e.update(env)
    cmd = [exe, path, str(cus or GOLD['device']['cus'])] + [str(b) for b in BPC] + (['--layouts'] if layouts else [])
    recs = [json.loads(line) for line in subprocess.check_output(cmd, env=e).decode().splitlines()]
    assert [r.pop('case') for r in recs] == [list(c) for c in cases]
    return recs


def test_the_recording_covers_the_table():
    assert GOLD['device']['cus'] == 256 and BPC == [6, 5, 4, 4, 3, 3]
    assert sorted(GOLD['plans']) == sorted(ENVS)
    for key, (_, cases) in ENVS.items():
        assert len(GOLD['plans'][key]) == len(cases), key
        assert sorted(GOLD['ws'][key]) == sorted(C.case_line(c) for c in cases if c[0] == 'conv'), key
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'conv_plans.json')) < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'heads.npz'))


def test_every_case_hits_the_branches_it_names_and_every_branch_is_named():
    """from the recorded plans alone"""
    named = set()
    for case, env, tags in C.CASES:
        cases = ENVS[C.env_key(env)][1]
        rec = GOLD['plans'][C.env_key(env)][cases.index(case)]
        for t in tags:
            assert C.TAGS[t](case, rec), (t, case, env, rec)
            named.add(t)
    assert named == set(C.TAGS), sorted(set(C.TAGS) - named)


@pytest.mark.parametrize('key', sorted(ENVS))
def test_the_header_answers_the_recorded_plans(dump, tmp_path, key):
    env, cases = ENVS[key]
    got = run_dump(dump, tmp_path, env, cases)
    for c, g, want in zip(cases, got, GOLD['plans'][key]):
        assert g == want, (key, c)


_QUERY = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
cases = json.loads(sys.argv[2])
for n in %r: getattr(lib, n).restype = ctypes.c_size_t
lib.fte_gemm_ws_bytes.restype = ctypes.c_size_t
out = {}
for c in cases:
    ans = []
    if c[0] == 'conv':
        for algo in (0, 1, 2):
            for dtype in (0, 1):
                assert lib.fte_set_conv_algo(algo) == 0 and lib.fte_set_mfma_dtype(dtype) == 0
                ans.append([getattr(lib, q)(*c[1:]) for q in %r] + ([getattr(lib, q)(*(c[1:6] + c[7:])) for q in %r] if c[6] == 3 else []))
    elif c[0] == 'dense':
        for dtype in (0, 1):
            assert lib.fte_set_mfma_dtype(dtype) == 0
            ans.append(lib.fte_gemm_ws_bytes(*c[1:]))
    else:
        continue
    out[' '.join(str(v) for v in c)] = ans
print(json.dumps(out))
''' % (CONV_Q + CONV3_Q, CONV_Q, CONV3_Q)


@pytest.mark.parametrize('key', sorted(ENVS))
def test_the_library_answers_the_recorded_workspace_sizes(key):
    """the seven conv queries and fte_gemm_ws_bytes of the built libfte.so, under every fte_set_conv_algo / fte_set_mfma_dtype value; the
    library reads its switches once per process, hence a child per environment (loading the library needs no GPU)"""
    lib = os.path.join(ROOT, 'tf_face_toolbox_amd', 'libfte.so')
    if not os.path.exists(lib):
        subprocess.check_call(['bash', os.path.join(ROOT, 'tf_face_toolbox_amd', 'csrc', 'build.sh')])
    env, cases = ENVS[key]
    e = {k: v for k, v in os.environ.items() if not k.startswith('FTE_')}
    e.update(env)
    e['HIP_VISIBLE_DEVICES'] = ''            # the recording's device is "none": 256 CUs, the compiled stream-K figures
    got = json.loads(subprocess.check_output([sys.executable, '-c', _QUERY, lib, json.dumps([list(c) for c in cases])], env=e).decode())
    want = dict(GOLD['ws'][key], **GOLD['gemm_ws'][key])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (key, k)


def test_the_layout_totals_are_the_recorded_queries(dump, tmp_path):
    """the driver's maximum of `total` over the three contexts IS the query: forward and data gradient equal the recorded answers, the filter
    gradient (whose resident-kernel slabs wgrad16.hip plans) never exceeds it"""
    for key, (env, cases) in ENVS.items():
        convs = [c for c in cases if c[0] == 'conv']
        for c, r in zip(convs, run_dump(dump, tmp_path, env, convs, layouts=True)):
            rec = GOLD['ws'][key][C.case_line(c)]
            for algo in (0, 1, 2):
                fwd, dgrad, wgrad = r['query'][algo]
                want = rec[algo * 2]
                if 'fwd' in r['ctx']['f32']:
                    assert fwd == want[0], (key, c, algo)
                if 'cls' in r['ctx']['f32']:
                    assert dgrad == want[1], (key, c, algo)
                if 'wgrad' in r:
                    assert wgrad <= want[2], (key, c, algo)


def _check_rows(M, N, K, rp, cus, what):
    tile, rows, mt, mode, ttile, tmt, splits, kchunk, pw, workers = rp
    dims = {C.T128: (128, 128), C.T256x64: (256, 64), C.T128x64: (128, 64), C.T64: (64, 64), C.T192: (192, 64)}
    bm, bn = dims[tile]
    if mode == 3:
        iters = C._up(M, bm) * (N // bn) * (K // 32)
        assert 0 < workers <= iters and workers <= cus * 6, what
        assert rows == M and mt == C._up(M, bm), what
        assert pw == workers * bm * bn * 4 + (workers * 4 + 255) // 256 * 256, what
        return
    assert workers == 0, what
    assert mt == C._up(rows, bm) and (rows == M or rows % bm == 0), what
    tail_rows = M - rows
    if mode == 0:
        assert tail_rows == 0 and pw == 0 and tmt == 0, what
    elif mode == 1:
        assert tail_rows > 0 and ttile == C.T64 and tmt == C._up(tail_rows, 64) and pw == 0, what
    else:
        tbm, tbn = dims[ttile]
        assert mode == 2 and tail_rows > 0 and tmt == C._up(tail_rows, tbm) * 4, what
        assert kchunk % 32 == 0 and splits == C._up(K, kchunk) and splits >= 2, what
        assert pw == splits * C._up(tail_rows, tbm) * (N // tbn) * tbm * tbn * 4, what


@pytest.mark.parametrize('cus', [104, 304])
def test_invariants_on_other_devices(dump, tmp_path, cus):
    """no recording to compare with: a smaller and a larger device keep what the launches rely on -- stream-K workers <= iterations, the
    workspace bytes of the chosen mode, main + tail rows = M, and a query total that covers every context's layout"""
    for key, (env, cases) in ENVS.items():
        for c, r in zip(cases, run_dump(dump, tmp_path, env, cases, cus=cus, layouts=True)):
            what = (cus, key, c)
            if c[0] == 'rows':
                for ctx, rp in r['ctx'].items():
                    _check_rows(c[1], c[2], c[3], rp, cus, what + (ctx,))
            if c[0] != 'conv':
                continue
            _, n, h, w, cin, cout, k, s = c
            for ctx, p in r['ctx'].items():
                if 'fwd' in p:
                    M, N, K = C._mnk_fwd(c)
                    _check_rows(M, N, K, p['fwd'], cus, what + (ctx, 'fwd'))
                    _check_rows(M, N, K, p['fwd_nows'], cus, what + (ctx, 'fwd_nows'))
                    assert p['fwd_nows'][C.PW_BYTES] == 0 and p['fwd_total'] >= p['fwd'][C.PW_BYTES]
                    if ctx.endswith('bn'):
                        assert p['fwd'][C.TAIL_MODE] < 2, what
                for ntap, hq, wq, mtiles, rp in p.get('cls', []):
                    _check_rows(n * hq * wq, cin, ntap * cout, rp, cus, what + (ctx, 'dgrad'))
                    assert mtiles == rp[C.MAIN_MT] + rp[C.TAIL_MT]
                if 'cls' in p:
                    assert p['dgrad_total'] >= p['dgrad_need'], what
                    assert p['dgrad_rows'] == (p['merged'][1] if p['merged'][0] else sum(k[3] for k in p['cls'])), what
            for algo in (0, 1, 2):
                for ctx in ('f32', 'bf16', 's16'):
                    p = r['ctx'][ctx]
                    assert r['query'][algo][0] >= p.get('fwd', [0] * 10)[C.PW_BYTES] and r['query'][algo][1] >= p.get('dgrad_need', 0), what
            for ctx in ('f32', 'bf16', 's16'):          # the contexts the query is the maximum of (recorded algo: 2)
                assert r['query'][2][0] >= r['ctx'][ctx].get('fwd_total', 0) and r['query'][2][1] >= r['ctx'][ctx].get('dgrad_total', 0), what
            if 'wino_ws' in r:
                for op, (v, u, slab, total) in enumerate(r['wino_ws']):
                    assert v % 256 == 0 and v <= u <= slab <= total, what
                    if r['sized'][2][op]:
                        assert r['query'][2][op] >= total, what
