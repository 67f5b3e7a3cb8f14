"""CPU: the case table of tests/test_gpu_wino_edges.py (tests/wino_cases.py) reaches every branch of the Winograd launchers it was written
for, by the launchers' own arithmetic (tests/wino_map.py) at the MI355X's 256 CUs.  Every case names its classes; a case that the model
does not put in one of them fails here, so the table cannot quietly shrink back to half-tile launches of SphereNet's own layers."""
import pytest

import wino_cases
import wino_map

CUS = 256


def _fwd(case):
    n, h, w, cin, cout = case
    M, MB, th, tw = wino_map.geom(n, h, w)
    return M, MB, th, tw, wino_map.mm_plan(MB, cout, CUS)


def _whole(c):
    return _fwd(c)[4]['symbols'] == ['wino_mm_kernel<0,2>']


def _half(c):
    return _fwd(c)[4]['symbols'] == ['wino_mm_kernel<0,1>']


def _nch(nv):
    return lambda c: c[4] == nv


def _tw(v):
    return lambda c: wino_map.geom(*c[:3])[3] == v


def _p(v):
    return lambda c: (c[3] // 64) * (c[4] // 64) == v and wino_map.wgrad_splits(c[3], c[4]) == 256 // v


def _shares(c):
    MB = wino_map.geom(*c[:3])[1]
    return wino_map.wgrad_shares(MB, wino_map.wgrad_splits(c[3], c[4]))


CLASSES = {
    # block order of wino_mm (keyed on NB = cout / 64)
    'grp8': lambda c: _fwd(c)[4]['order'] == 8,
    'plain': lambda c: _fwd(c)[4]['order'] == 'plain',
    # kernel form and rounds
    'whole': _whole,
    'half': _half,
    'one_round': lambda c: _fwd(c)[4]['rounds'] == 1,
    'two_rounds': lambda c: _fwd(c)[4]['rounds'] == 2 and _fwd(c)[4]['last_valid'] > 0,
    'two_tiles_per_block': lambda c: _whole(c) and _fwd(c)[4]['max_tiles'] == 2,
    'empty_blocks': lambda c: _whole(c) and _fwd(c)[4]['empty_blocks'] > 0,
    'tiles128': lambda c: _half(c) and _fwd(c)[4]['tiles'] == 128,
    'smallest_whole': lambda c: _whole(c) and c[0] > 1 and _half((c[0] - 1,) + tuple(c[1:])),
    # shapes
    'odd': lambda c: c[1] % 2 == 1 and c[2] % 2 == 1,
    'ragged': lambda c: _fwd(c)[0] % 64 != 0 and _fwd(c)[1] > 1,
    'm_lt_64': lambda c: _fwd(c)[0] < 64,
    'one_tile': lambda c: _fwd(c)[0] == 1,
    'two_tiles': lambda c: _fwd(c)[0] == 2,
    'k64': lambda c: c[3] == 64,
    'k512': lambda c: c[3] == 512,
    'n64': _nch(64), 'n128': _nch(128), 'n192': _nch(192), 'n256': _nch(256), 'n384': _nch(384), 'n512': _nch(512), 'n2048': _nch(2048),
    'cin_gt_cout': lambda c: c[3] > c[4],
    # filter gradient: shares, dz walker
    'p8': _p(8), 'p32': _p(32), 'p128': _p(128), 'p256': _p(256),
    'wgrad_direct': lambda c: wino_map.wgrad_splits(c[3], c[4]) == 0,
    'p_not_dividing_256': lambda c: (c[3] // 64) * (c[4] // 64) <= 256 and 256 % ((c[3] // 64) * (c[4] // 64)) != 0,
    'p_above_256': lambda c: (c[3] // 64) * (c[4] // 64) > 256,
    'tw1': _tw(1), 'tw2': _tw(2), 'tw3': _tw(3),
    'step_spans_images': lambda c: wino_map.geom(*c[:3])[2] * wino_map.geom(*c[:3])[3] < 8 and c[0] > 1,
    'carry_twice': lambda c: wino_map.geom(*c[:3])[2] * wino_map.geom(*c[:3])[3] <= 4 and c[0] > 2,
    'empty_shares255': lambda c: len(_shares(c)) == 256 and sorted(_shares(c))[-2:] == [0, 1],
}

# every class the table has to reach, and the table it has to be reached in
REQUIRED_MM = ['grp8', 'plain', 'whole', 'half', 'one_round', 'two_rounds', 'two_tiles_per_block', 'empty_blocks', 'tiles128', 'smallest_whole',
               'odd', 'ragged', 'm_lt_64', 'one_tile', 'two_tiles', 'k64', 'k512', 'n64', 'n128', 'n192', 'n256', 'n384', 'n512', 'n2048',
               'cin_gt_cout']
REQUIRED_WGRAD = ['p8', 'p32', 'p128', 'p256', 'cin_gt_cout', 'tw1', 'tw2', 'tw3', 'step_spans_images', 'carry_twice', 'empty_shares255']
REQUIRED_NOSPLIT = ['wgrad_direct', 'p_not_dividing_256', 'p_above_256']
# combinations the whole-tile kernel has never met: one case has to carry all of a row
REQUIRED_TOGETHER = [
    ('grp8', 'two_rounds', 'whole', 'two_tiles_per_block', 'k64', 'odd', 'ragged'),
    ('grp8', 'half'),
    ('plain', 'two_rounds', 'whole', 'two_tiles_per_block'),
    ('plain', 'half', 'n192'), ('plain', 'half', 'n384'), ('plain', 'half', 'n2048'),
    ('whole', 'one_round', 'empty_blocks', 'odd', 'n512'),
    ('whole', 'n64', 'odd'), ('whole', 'n128', 'odd'), ('whole', 'n256', 'k64'),
    ('cin_gt_cout', 'k512'),
]

ALL = [('mm', c, t) for c, t in wino_cases.MM_CASES] + [('wgrad', c, t) for c, t in wino_cases.WGRAD_CASES] + \
      [('nosplit', c, t) for c, t in wino_cases.NOSPLIT_CASES]


@pytest.mark.parametrize('table,case,tags', ALL, ids=['%s-%s' % (t, 'x'.join(map(str, c))) for t, c, _ in ALL])
def test_case_reaches_the_classes_it_is_there_for(table, case, tags):
    assert tags, 'a case without a class has no reason to be in the table'
    for tag in tags:
        assert tag in CLASSES, 'unknown class %r' % tag
        assert CLASSES[tag](case), 'the launch model does not put %r in class %r: %r' % (case, tag, _fwd(case))
    n, h, w, cin, cout = case
    assert cin % 64 == 0 and cout % 64 == 0 and h >= 2 and w >= 2          # wino_shape_ok
    if table != 'nosplit':
        # the tolerances were set on reductions of at most 512 channels: the large channel counts sit on the N side only
        assert cin <= 512 or table == 'wgrad', case


@pytest.mark.parametrize('table,required', [(wino_cases.MM_CASES, REQUIRED_MM), (wino_cases.WGRAD_CASES, REQUIRED_WGRAD),
                                            (wino_cases.NOSPLIT_CASES, REQUIRED_NOSPLIT)], ids=['mm', 'wgrad', 'nosplit'])
def test_every_class_has_a_case(table, required):
    have = set(t for _, tags in table for t in tags)
    assert not [r for r in required if r not in have], [r for r in required if r not in have]


def test_the_combined_classes_sit_on_one_case():
    for row in REQUIRED_TOGETHER:
        assert any(all(t in tags for t in row) for _, tags in wino_cases.MM_CASES), row


def test_kept_cases_are_winograd_filter_gradients_on_ragged_row_blocks():
    for c in wino_cases.KEPT_CASES:
        assert wino_map.wgrad_splits(c[3], c[4]) > 0 and wino_map.geom(*c[:3])[0] % 64 != 0, c


def test_model_on_the_launches_the_suite_has_pinned():
    """the symbol lists tests/test_gpu_tiles.py pins on the device (256 CUs), from the model"""
    def syms(n, h, w, c, epi=0):
        return wino_map.mm_plan(wino_map.geom(n, h, w)[1], c, CUS, epi)['symbols']
    assert syms(72, 14, 14, 256) == ['wino_mm_kernel<0,2>'] and syms(136, 7, 7, 512) == ['wino_mm_kernel<0,2>']
    assert syms(64, 7, 7, 512) == ['wino_mm_kernel<0,1>'] and syms(64, 7, 7, 512, 1) == ['wino_mm_kernel<1,1>']
    assert syms(84, 14, 14, 256) == ['wino_mm_kernel<0,2>'] and syms(40, 14, 14, 256) == ['wino_mm_kernel<0,1>']
    p = wino_map.mm_plan(17, 512, CUS)
    assert (p['nvirt'], p['grid'], p['last_valid'], p['empty_blocks'], p['order']) == (144, 144, 136, 8, 4)
    p = wino_map.mm_plan(17, 1024, CUS)
    assert (p['nvirt'], p['grid'], p['rounds'], p['last_valid'], p['max_tiles']) == (272, 256, 2, 16, 2)
    p = wino_map.mm_plan(88, 192, CUS)
    assert (p['nvirt'], p['rounds'], p['last_valid'], p['order']) == (264, 2, 8, 'plain')
    assert [wino_map.wgrad_splits(64 * a, 64 * b) for a, b in [(1, 1), (1, 8), (8, 1), (4, 8), (8, 16), (16, 16), (3, 1), (32, 16)]] == \
        [256, 32, 32, 8, 2, 1, 0, 0]
    # every valid id decodes to a different block, and all blocks are covered, in each order class
    for MB, N in [(17, 1024), (17, 512), (88, 192), (5, 64), (3, 2048), (9, 256)]:
        nv = wino_map.mm_plan(MB, N, CUS)['nvirt']
        blocks = [wino_map.decode(v, MB, N) for v in range(nv)]
        blocks = [b for b in blocks if b is not None]
        assert sorted(blocks) == [(mb, nb) for mb in range(MB) for nb in range(N // 64)], (MB, N)
