"""CPU: the case table of tests/test_gpu_pw16_edges.py (tests/pw16_cases.py) reaches every branch of the streaming pointwise kernel's
planner and block map it was written for, by the launcher's own arithmetic (tests/pw16_map.py).  Every case names its classes; a case that
the model does not put in one of them fails here, so the table cannot quietly shrink back to power-of-two column-tile counts with one or
two tiles per wave."""
import pytest

import pw16_cases
import pw16_map


def _inst(K, nb, nw):
    return lambda L: (L['symbol'].split('<')[1].split(',')[:3]) == [str(K), str(nb), str(nw)]


def _eq(key, v):
    return lambda L: L[key] == v


def _tiles(lo, hi):
    return lambda L: (L['tiles_min'], L['tiles_max']) == (lo, hi)


CLASSES = {
    # the instantiation pw16_launch picks: (K, NB, NW)
    'k64_nb256': _inst(64, 256, 8), 'k64_nb128': _inst(64, 128, 8), 'k64_nb64': _inst(64, 64, 8),
    'k128_nb128': _inst(128, 128, 8), 'k128_nb64': _inst(128, 64, 8),
    'k256_nb64_w8': _inst(256, 64, 8), 'k256_nb128_w4': _inst(256, 128, 4), 'k256_nb64_w4': _inst(256, 64, 4),
    # column tiles
    'nct1': _eq('nct', 1), 'nct2': _eq('nct', 2), 'nct3': _eq('nct', 3), 'nct5': _eq('nct', 5), 'nct8': _eq('nct', 8),
    # row blocks, the grid's dead blocks (rb >= nrb), idle waves in live blocks
    'nrb4': _eq('nrb', 4), 'nrb8': _eq('nrb', 8), 'nrb13': _eq('nrb', 13),
    'nrb32_capped': lambda L: L['nrb'] == 32 and (L['tiles'] + L['nw'] - 1) // L['nw'] > 32,
    'nrb128_capped': lambda L: L['nrb'] == 128 and (L['tiles'] + L['nw'] - 1) // L['nw'] > 128,
    'nrb512_capped': lambda L: L['nrb'] == 512 and (L['tiles'] + L['nw'] - 1) // L['nw'] > 512,
    'two_rb_per_xcd': lambda L: (L['nrb'] + 7) // 8 == 2,
    'dead_blocks': lambda L: L['dead_blocks'] > 0, 'dead3': _eq('dead_blocks', 3), 'dead7': _eq('dead_blocks', 7), 'no_dead': _eq('dead_blocks', 0),
    'idle_waves': lambda L: L['idle_waves'] > 0, 'idle7': _eq('idle_waves', 7), 'no_idle': _eq('idle_waves', 0),
    # tiles per wave
    'one_tile': _eq('tiles', 1), 'one_tile_per_wave': _tiles(1, 1), 'tiles_1_2': _tiles(1, 2), 'tiles_2_3': _tiles(2, 3),
    'tiles_3_4': _tiles(3, 4), 'tiles_5_6': _tiles(5, 6), 'tiles_10_11': _tiles(10, 11),
    # rows of the last tile
    'no_tail': _eq('last_rows', 32), 'tail1': _eq('last_rows', 1), 'tail3': _eq('last_rows', 3), 'tail4': _eq('last_rows', 4),
    'tail5': _eq('last_rows', 5), 'tail6': _eq('last_rows', 6), 'tail8': _eq('last_rows', 8), 'tail14': _eq('last_rows', 14),
    'm_not_32': lambda L: L['M'] % 32 != 0,
}

REQUIRED_DEFAULT = ['k64_nb256', 'k64_nb128', 'k64_nb64', 'k128_nb128', 'k128_nb64', 'k256_nb64_w8', 'nct1', 'nct2', 'nct3', 'nct5', 'nct8',
                    'nrb4', 'nrb8', 'nrb13', 'nrb32_capped', 'nrb128_capped', 'two_rb_per_xcd', 'dead_blocks', 'dead3', 'dead7', 'no_dead',
                    'idle_waves', 'idle7', 'no_idle', 'one_tile', 'tiles_2_3', 'no_tail', 'tail1', 'tail3', 'tail4', 'tail5', 'tail6', 'm_not_32']
REQUIRED_HOOKED = ['k256_nb128_w4', 'k256_nb64_w4', 'nrb512_capped', 'tiles_5_6', 'tiles_10_11']
REQUIRED_HARD = ['nct1', 'nct3', 'tiles_3_4', 'tail1']
# one case has to carry all of a row
REQUIRED_TOGETHER = [
    ('k64_nb128', 'one_tile', 'idle7', 'dead7'), ('k64_nb64', 'nct3', 'tail3'), ('k256_nb64_w8', 'tail4'),
    ('k64_nb256', 'nct2', 'nrb4', 'dead_blocks', 'idle_waves', 'tail5'), ('k128_nb64', 'nct3'), ('k128_nb128', 'nct3'), ('k256_nb64_w8', 'nct5'),
    ('nrb8', 'no_dead', 'no_idle', 'no_tail'), ('nrb13', 'two_rb_per_xcd', 'dead3'), ('nct8', 'nrb32_capped', 'tiles_2_3', 'tail6'),
    ('nrb128_capped', 'tiles_2_3', 'tail1'),
]

ALL = [('default', c, {}, t) for c, t in pw16_cases.CASES] + [('hooked', c, e, t) for c, e, t in pw16_cases.HOOKED] + \
      [('hard', c, {}, t) for c, t in pw16_cases.HARD_STATS]


def _launch(case, env, fold=False):
    L = pw16_map.launch(*case, fold=fold, **pw16_cases.hooks(env))
    assert L is not None, 'pw16_plan refuses %r' % (case,)
    return dict(L, M=case[0])


@pytest.mark.parametrize('table,case,env,tags', ALL, ids=['%s-%s' % (t, 'x'.join(map(str, c))) for t, c, _, _ in ALL])
def test_case_reaches_the_classes_it_is_there_for(table, case, env, tags):
    assert tags, 'a case without a class has no reason to be in the table'
    L = _launch(case, env)
    for tag in tags:
        assert tag in CLASSES, 'unknown class %r' % tag
        assert CLASSES[tag](L), 'the launch model does not put %r %r in class %r: %r' % (case, env, tag, L)
    # the folded form differs in the PRO slot of the symbol only
    F = _launch(case, env, fold=True)
    assert F['symbol'] == L['symbol'][:-4] + '1,1>' and {k: v for k, v in F.items() if k != 'symbol'} == {k: v for k, v in L.items() if k != 'symbol'}


@pytest.mark.parametrize('table,required', [(pw16_cases.CASES, REQUIRED_DEFAULT), ([(c, t) for c, _, t in pw16_cases.HOOKED], REQUIRED_HOOKED),
                                            (pw16_cases.HARD_STATS, REQUIRED_HARD)], ids=['default', 'hooked', 'hard'])
def test_every_class_has_a_case(table, required):
    have = set(t for _, tags in table for t in tags)
    assert not [r for r in required if r not in have], [r for r in required if r not in have]


def test_the_combined_classes_sit_on_one_case():
    for row in REQUIRED_TOGETHER:
        assert any(all(t in tags for t in row) for _, tags in pw16_cases.CASES), row


def test_every_default_reachable_instantiation_is_in_the_table():
    """(K, NB, NW) over every N the planner takes, times PRO = plain / folded (every case runs both), EPI = statistics"""
    reach = pw16_map.reachable()
    assert reach == {(64, 256, 8), (64, 128, 8), (64, 64, 8), (128, 128, 8), (128, 64, 8), (256, 64, 8)}
    want = {pw16_map.symbol(K, nb, nw, fold) for K, nb, nw in reach for fold in (False, True)}
    have = {_launch(c, {}, fold)['symbol'] for c, _ in pw16_cases.CASES for fold in (False, True)}
    assert want == have, sorted(want ^ have)
    # and the hooked table adds exactly the two four-wave K = 256 forms
    extra = pw16_map.reachable(k256=0) - reach
    assert extra == {(256, 128, 4), (256, 64, 4)}
    hooked = {_launch(c, e)['symbol'] for c, e, _ in pw16_cases.HOOKED}
    assert {pw16_map.symbol(K, nb, nw, False) for K, nb, nw in extra} <= hooked


def test_partial_rows_fit_the_workspace_grant():
    """nrb partial rows [3][N] against the (ceil(M / 64) + 2) rows of fte_conv2d_bn_fwd_ws_bytes, for every case and both K = 256 forms
    (four waves per block make twice the row blocks of eight)"""
    shapes = [c for _, c, _, _ in ALL]
    for M, K, N in shapes:
        for k256 in (0, 1):
            for blocks in (8, 256, 100000):
                p = pw16_map.plan(M, K, N, blocks=blocks, k256=k256)
                assert p is not None and p['nrb'] <= pw16_map.ws_rows(M), (M, K, N, k256, blocks, p)
    # the smallest shapes the planner takes, and every row count around a tile boundary
    for M in list(range(32, 300)) + [511, 512, 513, 4095, 4096, 4097]:
        for K, N in [(64, 64), (128, 64), (256, 64), (256, 128), (64, 512)]:
            for k256 in (0, 1):
                p = pw16_map.plan(M, K, N, blocks=100000, k256=k256)
                assert p['nrb'] <= pw16_map.ws_rows(M), (M, K, N, k256, p)


def test_below_the_floor_and_refusals():
    M, K, N = pw16_cases.BELOW_FLOOR
    assert M == 31 and pw16_map.plan(M, K, N) is None and pw16_map.plan(M + 1, K, N) is not None
    assert pw16_map.plan(4096, 512, 512) is None and pw16_map.plan(4096, 320, 64) is None and pw16_map.plan(4096, 64, 96) is None
    assert pw16_map.plan((1 << 31) // (2 * 512), 64, 512) is None and pw16_map.plan((1 << 31) // (2 * 512) - 1, 64, 512) is not None


def test_model_on_the_issue_table():
    """the numbers the cases were chosen by"""
    L = pw16_map.launch(32, 64, 128)
    assert (L['symbol'], L['grid'], L['dead_blocks'], L['idle_waves'], L['tiles']) == ('pw16_kernel<64,128,8,0,1>', 8, 7, 7, 1)
    L = pw16_map.launch(805, 64, 512, fold=True)
    assert (L['symbol'], L['nct'], L['nrb'], L['grid'], L['dead_blocks'], L['tiles'], L['idle_waves'], L['last_rows']) == \
        ('pw16_kernel<64,256,8,1,1>', 2, 4, 16, 8, 26, 6, 5)
    L = pw16_map.launch(3256, 64, 256)
    assert (L['nrb'], L['grid'], L['dead_blocks'], L['tiles']) == (13, 16, 3, 102)
    L = pw16_map.launch(16422, 256, 512)
    assert (L['nb'], L['nct'], L['nrb'], L['tiles_min'], L['tiles_max'], L['last_rows']) == (64, 8, 32, 2, 3, 6)
    L = pw16_map.launch(131406, 64, 64, blocks=100000)
    assert (L['nrb'], L['grid'], L['dead_blocks'], L['tiles_min'], L['tiles_max']) == (512, 512, 0, 1, 2)
    assert pw16_map.launch(805, 256, 128, k256=0)['symbol'] == 'pw16_kernel<256,128,4,0,1>'
    assert pw16_map.launch(805, 256, 192, k256=0)['symbol'] == 'pw16_kernel<256,64,4,0,1>'
    assert pw16_map.launch(805, 256, 128)['symbol'] == 'pw16_kernel<256,64,8,0,1>'
