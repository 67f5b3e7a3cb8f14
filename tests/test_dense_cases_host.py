"""CPU: the case tables of tests/dense_ref.py hit the branches they name.  The plan columns (tile, splits, kchunk) of the dense cases are
what the planner header answers at 256 CUs (tests/conv_plan_dump.cpp, built with g++ as tests/test_conv_plan_host.py does); the `kmf`
predicate, the three k_reduce_rows2 plans, k_conv_first_wgrad_blocks, the rows per block and the trips per wave are asserted on the
host mirrors; fte_gemm_ws_bytes and fte_conv3x3_first_wgrad_ws_bytes of the built libfte.so (loading it needs no GPU) answer 0 for the
arguments the entry points reject and the mirrors' figures for every table case."""
import json
import os
import re
import subprocess
import sys

import pytest

import dense_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS, BPC = 256, [6, 5, 4, 4, 3, 3]          # the device of tests/golden/conv_plans.json


@pytest.fixture(scope='module')
def dense_lines(tmp_path_factory):
    """{(m, n, k): the `dense` line of the dump}; every table case has k >= 64, below which the dump's nt product has no tile"""
    d = tmp_path_factory.mktemp('dense_plan')
    exe = str(d / 'conv_plan_dump')
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'conv_plan_dump.cpp')])
    shapes = sorted({(c.m, c.n, c.k) for c in D.DENSE_CASES})
    assert all(k >= 64 for _, _, k in shapes)
    path = str(d / 'cases.txt')
    with open(path, 'w') as f:
        f.write(''.join('dense %d %d %d\n' % s for s in shapes))
    env = {k: v for k, v in os.environ.items() if not k.startswith('FTE_')}
    out = subprocess.check_output([exe, path, str(CUS)] + [str(b) for b in BPC], env=env).decode().splitlines()
    recs = [json.loads(line) for line in out]
    assert [tuple(r['case'][1:]) for r in recs] == shapes
    return dict(zip(shapes, recs))


def test_the_mirrors_follow_the_sources():
    src = lambda name: open(os.path.join(ROOT, 'tf_face_toolbox_amd', 'csrc', name)).read()
    assert re.search(r'constexpr long REDUCE_SCRATCH_FLOATS = 1 << 18;', src('conv_plan.h'))
    assert re.search(r'b > 2048 \? 2048 : \(b < 1 \? 1 : b\)', src('kernels.hip')) and D.FIRST_WGRAD_BLOCK_CAP == 2048
    assert re.search(r'\(p\.a_KC % 32 == 0\) && \(p\.M % 32 == 0\) && \(\(kend - kbeg\) % BK == 0\) && nsteps > 0', src('igemm.hip'))
    names = [c.name for c in D.DENSE_CASES]
    assert len(set(names)) == len(names) and set(D.NT_FUSED) == {c.name for c in D.NT_CASES} and set(D.BF16_CASES) == set(D.BF16_PLANS) <= set(names)


@pytest.mark.parametrize('case', D.DENSE_CASES, ids=lambda c: c.name)
def test_dense_plan_columns_and_branches(dense_lines, case):
    tile, splits, kchunk, slab = dense_lines[(case.m, case.n, case.k)]['f32'][D.DUMP_COLUMN[case.product]]
    assert (tile, splits, kchunk) == (case.tile, case.splits, case.kchunk)
    assert slab == D.dense_need_bytes(case)
    got = D.dense_facts(case)
    for key, want in case.facts.items():
        assert got[key] == want, (case.name, key, got[key], want)
    if case.name in D.BF16_PLANS:
        assert tuple(dense_lines[(case.m, case.n, case.k)]['bf16'][D.DUMP_COLUMN[case.product]][:2]) == D.BF16_PLANS[case.name]
    if case.name in D.NT_FUSED:         # the fused epilogue runs unsplit on pick_tile's tile of the [m, k] output
        ftile, part_rows = D.NT_FUSED[case.name]
        assert ftile == tile and part_rows == D.up(case.m, D.TILE_DIMS[tile][0])


def test_the_dense_table_names_every_branch_of_the_issue():
    by = {c.name: c for c in D.DENSE_CASES}
    f = {n: D.dense_facts(c) for n, c in by.items()}
    # the 256x64 tile under nn and under the [n][k] B layout of nt, the 128x64 tile under nn, each with a ragged last row tile
    assert by['nn_256x64'].tile == D.T256x64 and by['nt_256x64'].tile == D.T256x64 and by['nn_128x64'].tile == D.T128x64
    assert all(0 < f[n]['last_tile_rows'] < D.TILE_DIMS[by[n].tile][0] for n in ('nn_256x64', 'nt_256x64', 'nn_128x64'))
    # tn: k % 32 != 0 (slow gather everywhere), fast in every split but the last, a ragged last row tile, a reduction below one K-step
    assert by['tn_slow_gather'].k % 32 and not any(f['tn_slow_gather']['kmf'])
    assert f['tn_fast_then_slow']['kmf'] == [True] * 7 + [False] and f['tn_fast_then_slow']['last_range'] % 32
    assert by['tn_ragged_rows'].k % 128 and f['tn_ragged_rows']['kmf'] == [True, False]
    assert by['tn_short'].m < 32 and by['tn_short'].k % 32
    # the slab reduction: the slab kernel, and reduce_rows_kernel where a bias / an activation rides in it or the slabs are short
    plans = {f[n].get('reduce_plain') for n in by} | {f['nn_split4_bias_act']['reduce_bias']}
    assert {'slabs64', 'rows1'} <= plans
    # the dalpha partial rows of the fused nt: amod = 64 and amod = k between them reach the slab kernel, the two-pass
    # reduce_rows_q_kernel and the one-launch reduce_rows_kernel
    got = {D.nt_dalpha_reduce_plan(c, a)[0] for c in D.NT_CASES for a in (64, c.k)}
    assert {'slabs64', 'q2', 'rows1'} <= got, got
    assert D.nt_dalpha_reduce_plan(by['nt_256x64'], 64) == ('q2', 3)
    for c in D.NT_CASES:
        assert D.nt_fused_need_bytes(c) <= D.align_up(D.up(c.m, 64) * c.k * 4) + D.SCRATCH_BYTES


def test_reduce_plan_mirror_on_both_sides_of_its_conditions():
    P = D.reduce_rows2_plan
    assert P(2, 4096)[0] == 'slabs64' and P(2, 4092)[0] == 'rows1' and P(32, 4096)[0] == 'slabs16' and P(1, 4096)[0] == 'rows1'
    assert P(32, 4096 * 64)[0] == 'slabs64' and P(2, 4096, bias=True)[0] == 'rows1' and P(2, 4096, act=True)[0] == 'rows1'
    assert P(255, 288) == ('q1', 1) and P(256, 288) == ('q2', 8) and P(31, 288)[0] == 'rows1' and P(74, 864, scratch=False)[0] == 'rows1'
    assert P(74, 1024)[0] == 'q1' and P(74, 1028) == ('rows2', 4) and P(63, 1728)[0] == 'rows1'
    assert P(2048, 288) == ('q2', 64)


FWD = {c: D.first_fwd_geometry(c) for c in D.FIRST_FWD_CASES}
WG = {c: D.first_wgrad_geometry(c) for c in D.FIRST_WGRAD_CASES}


def test_first_conv_forward_cases_hit_their_branches():
    assert FWD[(2, 3, 32, 1, 64, 1)]['groups_per_row'] == 1 and FWD[(2, 3, 32, 1, 64, 1)]['last_group_pixels'] == 32
    assert FWD[(1, 5, 33, 3, 64, 1)]['groups_per_row'] == 2 and FWD[(1, 5, 33, 3, 64, 1)]['last_group_pixels'] == 1
    g = FWD[(1, 2, 130, 3, 32, 2)]
    assert (g['ho'], g['wo'], g['pt'], g['pl'], g['groups_per_row'], g['last_group_pixels']) == (1, 65, 0, 0, 3, 1)
    g = FWD[(2, 7, 9, 1, 64, 2)]
    assert (g['ho'], g['wo'], g['pt'], g['pl']) == (4, 5, 1, 1)
    for c in ((1, 1, 1, 3, 64, 1), (1, 1, 1, 1, 32, 2)):
        assert (FWD[c]['ho'], FWD[c]['wo'], FWD[c]['pt'], FWD[c]['pl'], FWD[c]['groups']) == (1, 1, 1, 1, 1) and FWD[c]['idle_waves'] == 3
    g = FWD[(1, 3, 112, 3, 64, 1)]
    assert g['groups_per_row'] == 4 and g['last_group_pixels'] == 16 and g['groups'] == 12 and g['blocks'] == 3
    g = FWD[(2, 6, 9, 3, 64, 2)]
    assert (g['pt'], g['pl']) == (0, 1)                       # the one shape whose two pads differ: a swapped pad moves every tap
    assert sorted({(c[3], c[4]) for c in D.FIRST_FWD_CASES}) == [(1, 32), (1, 64), (3, 32), (3, 64)]       # every kernel instance
    assert {c[5] for c in D.FIRST_FWD_CASES if c[3] == 3} == {1, 2}
    assert all(c in D.FIRST_FWD_CASES for c in D.FIRST_S16_FWD + [D.FIRST_COMBO_CASE])


def test_first_conv_filter_gradient_cases_hit_their_branches():
    small = [WG[c] for c in D.FIRST_FWD_CASES]
    assert all(g['blocks'] == 1 and g['reduce'] == ('rows1', 1) for g in small)                   # one partial row
    trips = set().union(*(g['wave_trips'] for g in small))
    assert {0, 1, 2, 3} <= trips, trips                                                          # the pipelined loop at 1, 2 and 3 trips
    assert any(t % 2 for t in trips if t > 3) and any(t % 2 == 0 for t in trips if t > 3)        # ... and long odd / even runs
    assert {g['trips_per_row'] for g in small} >= {1, 3, 4, 5, 9, 14}
    assert sum(g['last_trip_pixels'] == 1 for g in small) >= 3 and any(g['idle_waves'] for g in small)
    assert WG[(1, 1, 17, 3, 32, 1)]['wave_trips'] == {0, 3} and WG[(1, 1, 17, 3, 32, 1)]['last_trip_pixels'] == 1
    assert WG[(2, 6, 9, 3, 64, 2)]['pt'] != WG[(2, 6, 9, 3, 64, 2)]['pl']
    g = WG[(3, 112, 112, 3, 64, 1)]
    assert (g['blocks'], g['rows_per_block'], g['empty_blocks'], g['cols'], g['reduce']) == (74, 5, 6, 1728, ('rows2', 4))
    g = WG[(3, 112, 112, 3, 32, 1)]
    assert (g['blocks'], g['cols'], g['reduce']) == (74, 864, ('q1', 1))
    g = WG[(11, 112, 112, 1, 32, 1)]
    assert (g['blocks'], g['cols'], g['reduce']) == (270, 288, ('q2', 8))
    g = WG[D.FIRST_WGRAD_CAP]
    # (4704 output rows on 2048 blocks: three rows each, so the last 480 blocks get none and write zeros)
    assert 21 * 224 * 224 > 512 * 2048 and (g['blocks'], g['rows_per_block'], g['empty_blocks'], g['reduce']) == (2048, 3, 480, ('q2', 64))
    assert D.first_wgrad_blocks(512 * 2048) == 2048 and D.first_wgrad_blocks(512 * 2047) == 2047 and D.first_wgrad_blocks(1) == 1
    assert all(c in D.FIRST_WGRAD_CASES for c in D.FIRST_S16_WGRAD)
    assert {WG[c]['reduce'][0] for c in D.FIRST_S16_WGRAD} >= {'rows1', 'q1'}


_QUERY = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.fte_gemm_ws_bytes.restype = ctypes.c_size_t
lib.fte_conv3x3_first_wgrad_ws_bytes.restype = ctypes.c_size_t
req = json.loads(sys.argv[2])
out = {'gemm': [], 'first': []}
for dtype in (0, 1):
    assert lib.fte_set_mfma_dtype(dtype) == 0
    out['gemm'].append([lib.fte_gemm_ws_bytes(*a) for a in req['gemm']])
assert lib.fte_set_mfma_dtype(0) == 0
out['first'] = [lib.fte_conv3x3_first_wgrad_ws_bytes(*a) for a in req['first']]
print(json.dumps(out))
'''
BAD_GEMM = [(8, 0, 64), (8, 64, 0), (8, -64, 64), (8, 64, -64), (8, -128, -128), (0, 64, 64), (-3, 64, 64), (0, 0, 0)]
BAD_FIRST = [(1, 8, 8, 3, 64, 0), (1, 8, 8, 3, 64, 3), (1, 8, 8, 3, 64, -1), (0, 8, 8, 3, 64, 1), (1, 0, 8, 3, 64, 1), (1, 8, 0, 3, 64, 2),
             (-1, 8, 8, 3, 64, 1), (1, 8, 8, 2, 64, 1), (1, 8, 8, 3, 48, 1)]


def test_the_workspace_queries_answer_zero_for_rejected_arguments_and_the_old_values_otherwise(dense_lines):
    """(the rejected arguments used to end the process in an integer division by zero: plan_splits divides by the tile count,
    same_pads by the stride)"""
    lib = os.path.join(ROOT, 'tf_face_toolbox_amd', 'libfte.so')
    if not os.path.exists(lib):
        subprocess.check_call(['bash', os.path.join(ROOT, 'tf_face_toolbox_amd', 'csrc', 'build.sh')])
    shapes = sorted(dense_lines)
    firsts = D.FIRST_WGRAD_CASES
    env = {k: v for k, v in os.environ.items() if not k.startswith('FTE_')}
    env['HIP_VISIBLE_DEVICES'] = ''
    req = {'gemm': BAD_GEMM + shapes, 'first': BAD_FIRST + firsts}
    got = json.loads(subprocess.check_output([sys.executable, '-c', _QUERY, lib, json.dumps(req)], env=env).decode())
    for mode, key in enumerate(('f32', 'bf16')):
        ans = got['gemm'][mode]
        assert ans[:len(BAD_GEMM)] == [0] * len(BAD_GEMM), (key, ans[:len(BAD_GEMM)])
        for s, a in zip(shapes, ans[len(BAD_GEMM):]):
            assert a == D.gemm_ws_bytes(*s, [p[3] for p in dense_lines[s][key]]), (key, s, a)
    assert got['first'][:len(BAD_FIRST)] == [0] * len(BAD_FIRST)
    for c, a in zip(firsts, got['first'][len(BAD_FIRST):]):
        assert a == D.first_wgrad_ws_bytes(c), (c, a)
    # what a product's own launch needs never exceeds the layer's query
    for c in D.DENSE_CASES:
        q = D.gemm_ws_bytes(c.m, c.n, c.k, [p[3] for p in dense_lines[(c.m, c.n, c.k)]['f32']])
        assert D.dense_need_bytes(c) <= q and (c.name not in D.NT_FUSED or D.nt_fused_need_bytes(c) <= q)
