"""CPU: SphereNet's planning without a device -- the options record, the part-shard split point, the Winograd keep / lean plan and the
dz / skip-gradient rotation of the backward walk (nets/sphere.py read_options, nets/sphere_plan.py).  The expected split points and
the rotation sequences were recorded from the walks as they were before planning became plain functions (_fwd_split with the library's
planner stubbed; _body_walk with the launches stubbed, logging the identities of the dz_prev / raw arguments of the data gradients)."""
import pytest

from tf_face_toolbox_amd.nets.sphere import Options, SphereNet, read_options
from tf_face_toolbox_amd.nets.sphere_plan import StageRing, split_point, wino_plan

DEFAULTS = Options(bf16_copies=True, wino_keep=True, wino_lean=True, side_stream='size', fwd_halves='auto', fwd_split=None,
                   fwd_halves_min=128, dz_buffers=3)


def _convs(h=112, w=112):
    return SphereNet()._conv_specs(h, w, 3)


def wino_everywhere(n, h, w, cin, cout, stride, op):
    return 1 if stride == 1 else 0


def test_read_options_defaults():
    assert read_options({}) == DEFAULTS
    assert isinstance(read_options(), Options)               # the process environment
    with pytest.raises(AttributeError):
        read_options({}).dz_buffers = 2


@pytest.mark.parametrize('env,field,want', [
    ({'FTE_BF16_COPIES': '0'}, 'bf16_copies', False), ({'FTE_BF16_COPIES': '1'}, 'bf16_copies', True),
    ({'FTE_WINO_KEEP': '0'}, 'wino_keep', False), ({'FTE_WINO_KEEP': '1'}, 'wino_keep', True),
    ({'FTE_WINO_LEAN': '0'}, 'wino_lean', False), ({'FTE_WINO_LEAN': '1'}, 'wino_lean', True),
    ({}, 'side_stream', 'size'), ({'FTE_SIDE_STREAM': '0'}, 'side_stream', 'off'), ({'FTE_SIDE_STREAM': '1'}, 'side_stream', 'forced'),
    ({}, 'fwd_halves', 'auto'), ({'FTE_FWD_HALVES': '0'}, 'fwd_halves', 'off'), ({'FTE_FWD_HALVES': '1'}, 'fwd_halves', 'forced'),
    ({'FTE_FWD_HALVES': 'auto'}, 'fwd_halves', 'auto'),
    ({}, 'fwd_split', None), ({'FTE_FWD_SPLIT': '192'}, 'fwd_split', 192), ({'FTE_FWD_SPLIT': '0'}, 'fwd_split', 0),
    ({'FTE_FWD_HALVES_MIN': '32'}, 'fwd_halves_min', 32),
    ({'FTE_DZ_BUFFERS': '1'}, 'dz_buffers', 2), ({'FTE_DZ_BUFFERS': '2'}, 'dz_buffers', 2), ({'FTE_DZ_BUFFERS': '3'}, 'dz_buffers', 3),
    ({'FTE_DZ_BUFFERS': '4'}, 'dz_buffers', 4),
])
def test_read_options_each_switch(env, field, want):
    got = read_options(env)
    assert getattr(got, field) == want
    assert got._replace(**{field: getattr(DEFAULTS, field)}) == DEFAULTS      # ... and moves nothing else


def test_the_net_reads_its_switches_once_at_construction(monkeypatch):
    monkeypatch.setenv('FTE_DZ_BUFFERS', '2')
    monkeypatch.setenv('FTE_BF16_COPIES', '0')
    net = SphereNet()
    monkeypatch.setenv('FTE_DZ_BUFFERS', '3')
    assert net.options.dz_buffers == 2 and net.bf16_copies is False
    assert net.one_stream is False and net._trace_dz is None


def _split(n, hw=(112, 112), algo=wino_everywhere, **opts):
    convs = _convs(*hw)
    options = DEFAULTS._replace(**opts)
    kept, _ = wino_plan(convs, n, algo, options, False)
    return split_point(convs, kept, n, algo, options)


def test_tiles_and_granule():
    convs = _convs()
    assert [c.tiles for c in convs if c.hin == 14][0] == 49      # 64 / gcd(64, 49): a part must be a multiple of 64 images
    assert [c.tiles for c in _convs(40, 24)[:2]] == [20 * 12, 10 * 6]


@pytest.mark.parametrize('n,want', [(128, 64), (136, 64), (512, 256), (100, 0), (1, 0)])
def test_split_point_112(n, want):
    assert _split(n) == want


def test_split_point_other_cases():
    assert _split(128, (40, 24)) == 64
    # one part plans another algorithm than the whole shard (the 14x14 stage at 64 images)
    assert _split(128, algo=lambda n, h, w, ci, co, s, op: 1 if s == 1 and not (n == 64 and h == 14) else 0) == 0
    assert _split(128, algo=lambda *a: 0) == 0                   # no Winograd layer
    assert _split(128, fwd_halves='off') == 0
    assert _split(8, fwd_halves='forced', fwd_split=4) == 0      # 4 images x 49 tiles end inside a 64-tile row block
    assert _split(8, (40, 24), fwd_halves='forced', fwd_split=4) == 0
    assert _split(64) == 0 and _split(64, fwd_halves='forced') == 0 and _split(64, fwd_halves_min=32) == 0      # 32 is no multiple of 64
    assert _split(128, fwd_halves_min=256) == 0 and _split(128, fwd_halves='forced', fwd_halves_min=256) == 64


def test_wino_plan():
    convs = _convs()
    keep, lean = wino_plan(convs, 64, wino_everywhere, DEFAULTS, False)
    assert keep == [l > 0 and c.stride == 1 for l, c in enumerate(convs)]
    assert sum(lean) == 8 and all(c.second == 1 for c, f in zip(convs, lean) if f)
    for options, s16 in ((DEFAULTS._replace(wino_keep=False), False), (DEFAULTS, True)):
        keep, lean = wino_plan(convs, 64, wino_everywhere, options, s16)
        assert not any(keep) and not any(lean)
    # no Winograd filter gradient (op 2) in the 14x14 stage: none of its four blocks is lean, no layer there keeps a pack
    deny = lambda n, h, w, ci, co, s, op: 0 if (op == 2 and h == 14) else wino_everywhere(n, h, w, ci, co, s, op)
    keep, lean = wino_plan(convs, 64, deny, DEFAULTS, False)
    assert sum(lean) == 4 and not any(keep[l] for l, c in enumerate(convs) if c.hin == 14)
    # ... denied for the second conv of that stage's first block only: the block is not lean, its first conv keeps its pack
    l2 = [l for l, c in enumerate(convs) if c.hin == 14 and c.second == 1][0]
    state = {}

    def algo(n, h, w, ci, co, s, op):
        if op == 2 and h == 14:
            state['seen'] = state.get('seen', 0) + 1
            if state['seen'] == 2:                                  # the filter-gradient question about layer l2 (layers are asked in order)
                return 0
        return wino_everywhere(n, h, w, ci, co, s, op)
    keep, lean = wino_plan(convs, 64, algo, DEFAULTS, False)
    assert not keep[l2] and keep[l2 - 1] and not lean[l2] and sum(lean) == 7


# (stage, dz buffer, skip-gradient buffer or None) of every data gradient from the last layer down, SphereNet-20, as recorded
ROTATION = {
    2: [(3, 1, None), (3, 0, None), (2, 0, 0), (2, 1, None), (2, 0, 1), (2, 1, None), (2, 0, 0), (2, 1, None), (2, 0, 1), (2, 1, None),
        (2, 0, None), (1, 0, 0), (1, 1, None), (1, 0, 1), (1, 1, None), (1, 0, None), (0, 0, 0), (0, 1, None), (0, 0, None)],
    3: [(3, 1, None), (3, 2, None), (2, 0, 0), (2, 1, None), (2, 2, 1), (2, 0, None), (2, 1, 0), (2, 2, None), (2, 0, 1), (2, 1, None),
        (2, 2, None), (1, 0, 0), (1, 1, None), (1, 2, 1), (1, 0, None), (1, 1, None), (0, 0, 0), (0, 1, None), (0, 2, None)],
}


@pytest.mark.parametrize('buffers', [2, 3])
def test_rotation_hands_out_the_recorded_sequence_and_no_live_buffer(buffers):
    convs = _convs()
    rings = [StageRing([('dz', si, i) for i in range(buffers)], [('raw', si, i) for i in range(2)]) for si in range(4)]
    dz, d_out = rings[convs[-1].stage].reset()               # what the dense layer's backward writes
    assert (dz, d_out) == (('dz', 3, 0), ('raw', 3, 0))
    seq = []
    for l in range(len(convs) - 1, 0, -1):                   # the protocol of SphereNet._body_walk
        c, p = convs[l], convs[l - 1]
        ring = rings[p.stage]
        dz_prev, raw = ring.reset() if p.stage != c.stage else ring.advance()
        assert dz_prev is not dz and dz_prev is not d_out and raw is not d_out and raw is not dz      # never a buffer the launch reads
        raw = raw if p.second == 1 else None
        seq.append((dz_prev[1], dz_prev[2], None if raw is None else raw[2]))
        if raw is not None:
            d_out = raw
            ring.take_raw()
        dz = dz_prev
    assert seq == ROTATION[buffers]
