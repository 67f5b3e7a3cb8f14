"""-m gpu: the Winograd kernels (csrc/wino.hip) through the C ABI at the shapes their launchers and block maps BRANCH on -- block order
(XCD groups of 8 / plain), whole- and half-tile kernel, one and two rounds, grids with empty blocks, 1 .. 16 .. 32 column blocks, one- and
two-tile launches, every share count of the filter gradient and its dz walker at 1-3 tiles per image row -- against the float64 oracle's
DIRECT convolution, with the tolerances of tests/test_gpu_wino.py (tests/util_gpu.py), unchanged.  tests/wino_cases.py is the table,
tests/wino_map.py says which launches a case must make (asserted by EQUALITY with the launch records, for the device's own CU count), and
tests/test_wino_map_host.py proves on the CPU that the table reaches every class at 256 CUs.  Each check prints one `WINO_EDGE` line
(pytest -s): the figures of profiles/wino_edges.md."""
import numpy as np
import pytest
import torch

from oracle import ops
import wino_cases
import wino_map

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, dev, host, stream, ws, check_maxabs, check_rell2
    from tf_face_toolbox_amd import _lib

DIRECT, WINOGRAD, AUTO = 0, 1, 2
EINVAL, EWORKSPACE = -1, -2


def _id(c):
    return 'x'.join(str(v) for v in c)


def _swap(c):
    return c[:3] + (c[4], c[3])


FWD_CASES = [c for c, _ in wino_cases.MM_CASES]
# the data gradient's product is N = cin, K = cout: the swapped pair keeps a case in its class; as given too where cin > cout
DGRAD_CASES = [_swap(c) for c in FWD_CASES] + [c for c in FWD_CASES if c[3] > c[4]]
WGRAD_CASES = FWD_CASES + [c for c, _ in wino_cases.WGRAD_CASES if c not in FWD_CASES]
NOSPLIT_CASES = [c for c, _ in wino_cases.NOSPLIT_CASES]


@pytest.fixture
def winograd():
    prev = query('fte_get_conv_algo')
    call('fte_set_conv_algo', WINOGRAD)
    yield
    call('fte_set_conv_algo', prev)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _class_note():
    if _cus() != 256:
        print('WINO_EDGE note: %d CUs, not 256: the classes of tests/wino_cases.py are not asserted on this device; symbols are '
              'compared with the model for %d CUs and every value is checked' % (_cus(), _cus()))


def _mm_symbols(case, epi):
    """the launches wino_mm makes for the case's forward (epi 0: N = cout) or data-gradient (epi 1: N = cin) product on this device"""
    n, h, w, cin, cout = case
    return wino_map.mm_plan(wino_map.geom(n, h, w)[1], cin if epi else cout, _cus(), epi)['symbols']


def _symbols(fn):
    """kernel symbols of the MFMA launches `fn` makes"""
    call('fte_prof_enable', 1)
    fn()
    torch.cuda.synchronize()
    call('fte_prof_enable', 0)
    return [r[5] for r in _lib.prof_records(shapes=True)]


def _where(got, ref, case, what):
    """the worst element of an activation-shaped tensor: (n, y, x, channel) and the (mb, nb) block of the product that wrote it"""
    idx = np.unravel_index(np.argmax(np.abs(got - ref)), ref.shape)
    if ref.ndim == 4 and ref.shape[0] == case[0]:
        mb, nb = wino_map.block_of(idx[:3], idx[3], *case[:3])
        return '%s worst at (n, y, x, c) = %s: got %.6g, ref %.6g; row block mb = %d, column block nb = %d' % (
            what, tuple(int(i) for i in idx), got[idx], ref[idx], mb, nb)
    if ref.ndim == 4:
        return '%s worst at (kh, kw, ci, co) = %s: got %.6g, ref %.6g; cin block %d, cout block %d' % (
            what, tuple(int(i) for i in idx), got[idx], ref[idx], idx[2] // 64, idx[3] // 64)
    return '%s worst at %s: got %.6g, ref %.6g' % (what, tuple(int(i) for i in idx), got[idx], ref[idx])


def _check(kind, got, ref, case, what, syms=()):
    got = host(got) if isinstance(got, torch.Tensor) else got
    try:
        v = (check_rell2 if kind == 'rell2' else check_maxabs)(got, ref, what=what)
    except AssertionError as e:
        raise AssertionError('%s %s: %s\n%s' % (_id(case), list(syms), e, _where(got, ref, case, what)))
    print('WINO_EDGE %-7s %-18s %-12s %.3e  %s' % (what.split()[0], _id(case), ' '.join(what.split()[1:]), v, ','.join(syms)))
    return v


# references: computed once per case and product, never modified
_REFS = {}


def _ref(kind, case):
    key = (kind, case)
    if key not in _REFS:
        _REFS[key] = {'fwd': _ref_fwd, 'dgrad': _ref_dgrad, 'wgrad': _ref_wgrad}[kind](case)
        for v in _REFS[key].values():
            v.setflags(write=False)
    return _REFS[key]


def _ref_fwd(case):
    n, h, w, cin, cout = case
    r = np.random.default_rng(21)
    x = r.standard_normal((n, h, w, cin)); wt = r.standard_normal((3, 3, cin, cout)) * 0.05
    b = r.standard_normal(cout); al = 0.25 + 0.1 * r.standard_normal(cout)
    plain = ops.conv2d_fwd(x, wt, 1)
    z = plain + b
    res = r.standard_normal(z.shape)
    return dict(x=x, wt=wt, b=b, al=al, res=res, plain=plain, z=z, y=ops.prelu_fwd(z, al) + res)


def _ref_dgrad(case):
    n, h, w, cin, cout = case
    r = np.random.default_rng(22)
    wt = r.standard_normal((3, 3, cin, cout)) * 0.05
    dz = r.standard_normal((n, h, w, cout))
    dx, _ = ops.conv2d_bwd(np.zeros((n, h, w, cin)), wt, dz, 1, need_dw=False)
    dx = np.ascontiguousarray(dx)
    addin = r.standard_normal(dx.shape); zprev = r.standard_normal(dx.shape); alp = 0.25 + 0.1 * r.standard_normal(cin)
    zprev[0, 0, 0, :4] = 0.0
    g = dx + addin
    dzprev, dalpha = ops.prelu_bwd(zprev, alp, g)
    return dict(wt=wt, dz=dz, addin=addin, zprev=zprev, alp=alp, dx=dx, g=g, dzprev=dzprev, dalpha=dalpha, dbias=dzprev.sum(axis=(0, 1, 2)))


def _ref_wgrad(case):
    n, h, w, cin, cout = case
    r = np.random.default_rng(23)
    x = r.standard_normal((n, h, w, cin)); dz = r.standard_normal((n, h, w, cout))
    _, dw = ops.conv2d_bwd(x, np.zeros((3, 3, cin, cout)), dz, 1, need_dx=False)
    return dict(x=x, dz=dz, dw=dw)


@pytest.mark.parametrize('case', FWD_CASES, ids=_id)
def test_edge_fwd(winograd, case):
    n, h, w, cin, cout = case
    _class_note()
    f = _ref('fwd', case)
    shape = f['z'].shape
    assert query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 0) == WINOGRAD
    x, wt = dev(f['x']), dev(f['wt'])
    z = torch.full(shape, 7.0, device='cuda'); y = torch.full(shape, 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_fwd_ws_bytes', n, h, w, cin, cout, 1))
    args = (x, wt, dev(f['b']), dev(f['al']), dev(f['res']), z, y, n, h, w, cin, cout, 1, wsb, nb, stream())
    syms = _symbols(lambda: call('fte_conv3x3_fwd', *args))
    assert syms == _mm_symbols(case, 0), (syms, _mm_symbols(case, 0))
    _check('maxabs', z, f['z'], case, 'fwd z', syms); _check('maxabs', y, f['y'], case, 'fwd y', syms)
    y2 = torch.full(shape, 7.0, device='cuda')
    call('fte_conv3x3_fwd', x, wt, None, None, None, None, y2, n, h, w, cin, cout, 1, wsb, nb, stream())
    _check('maxabs', y2, f['plain'], case, 'fwd plain', syms)
    # bit-identical run to run (fixed summation orders, no atomics), with every tensor and without
    z3 = torch.full(shape, 7.0, device='cuda'); y3 = torch.full(shape, 7.0, device='cuda')
    call('fte_conv3x3_fwd', *(args[:5] + (z3, y3) + args[7:]))
    assert torch.equal(z, z3) and torch.equal(y, y3)
    y4 = torch.full(shape, 7.0, device='cuda')
    call('fte_conv3x3_fwd', x, wt, None, None, None, None, y4, n, h, w, cin, cout, 1, wsb, nb, stream())
    assert torch.equal(y2, y4)


@pytest.mark.parametrize('case', DGRAD_CASES, ids=_id)
def test_edge_dgrad_with_prelu_backward(winograd, case):
    n, h, w, cin, cout = case
    _class_note()
    f = _ref('dgrad', case)
    shape = f['dx'].shape
    assert query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 1) == WINOGRAD
    dz, wt = dev(f['dz']), dev(f['wt'])
    raw = torch.full(shape, 7.0, device='cuda'); dzp = torch.full(shape, 7.0, device='cuda')
    da = torch.full((cin,), 7.0, device='cuda'); db = torch.full((cin,), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_dgrad_ws_bytes', n, h, w, cin, cout, 1))
    args = (dz, wt, dev(f['addin']), dev(f['zprev']), dev(f['alp']), raw, dzp, da, db, n, h, w, cin, cout, 1, wsb, nb, stream())
    syms = _symbols(lambda: call('fte_conv3x3_dgrad', *args))
    assert syms == _mm_symbols(case, 1), (syms, _mm_symbols(case, 1))
    _check('maxabs', raw, f['g'], case, 'dgrad raw', syms); _check('maxabs', dzp, f['dzprev'], case, 'dgrad dzprev', syms)
    _check('rell2', da, f['dalpha'], case, 'dgrad dalpha', syms); _check('rell2', db, f['dbias'], case, 'dgrad dbias', syms)
    dzp2 = torch.full(shape, 7.0, device='cuda')
    call('fte_conv3x3_dgrad', dz, wt, None, None, None, None, dzp2, None, None, n, h, w, cin, cout, 1, wsb, nb, stream())
    _check('maxabs', dzp2, f['dx'], case, 'dgrad plain', syms)
    raw3 = torch.full(shape, 7.0, device='cuda'); dzp3 = torch.full(shape, 7.0, device='cuda')
    da3 = torch.full((cin,), 7.0, device='cuda'); db3 = torch.full((cin,), 7.0, device='cuda')
    call('fte_conv3x3_dgrad', *(args[:5] + (raw3, dzp3, da3, db3) + args[9:]))
    assert torch.equal(raw, raw3) and torch.equal(dzp, dzp3) and torch.equal(da, da3) and torch.equal(db, db3)
    dzp4 = torch.full(shape, 7.0, device='cuda')
    call('fte_conv3x3_dgrad', dz, wt, None, None, None, None, dzp4, None, None, n, h, w, cin, cout, 1, wsb, nb, stream())
    assert torch.equal(dzp2, dzp4)


@pytest.mark.parametrize('case', WGRAD_CASES, ids=_id)
def test_edge_wgrad(winograd, case):
    n, h, w, cin, cout = case
    f = _ref('wgrad', case)
    S = wino_map.wgrad_splits(cin, cout)
    assert query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 2) == (WINOGRAD if S else DIRECT)
    x, dz = dev(f['x']), dev(f['dz'])
    dw = torch.full((3, 3, cin, cout), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, 1))
    syms = _symbols(lambda: call('fte_conv3x3_wgrad', x, dz, dw, n, h, w, cin, cout, 1, wsb, nb, stream()))
    if S:
        assert syms == ['wino_wgrad_kernel'], syms
    else:                   # no share count for this channel pair: the direct kernels, never a Winograd launch
        assert syms and all(s_.startswith('igemm') for s_ in syms), syms
    _check('maxabs', dw, f['dw'], case, 'wgrad dw', sorted(set(syms)))
    dw2 = torch.full((3, 3, cin, cout), 7.0, device='cuda')
    call('fte_conv3x3_wgrad', x, dz, dw2, n, h, w, cin, cout, 1, wsb, nb, stream())
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize('case', NOSPLIT_CASES, ids=_id)
def test_no_split_count_sends_the_filter_gradient_direct(winograd, case):
    """(cin / 64) (cout / 64) does not divide 256, or exceeds it: forward and data gradient stay Winograd, the filter gradient runs the
    direct kernels and matches the oracle; a kept V pack is refused with the code of a kept pack under FTE_CONV_DIRECT, dw untouched."""
    n, h, w, cin, cout = case
    assert wino_map.wgrad_splits(cin, cout) == 0
    assert [query('fte_conv3x3_algo', n, h, w, cin, cout, 1, op) for op in (0, 1, 2)] == [WINOGRAD, WINOGRAD, DIRECT]
    f = _ref('wgrad', case)
    x, dz = dev(f['x']), dev(f['dz'])
    dw = torch.full((3, 3, cin, cout), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, 1))
    syms = _symbols(lambda: call('fte_conv3x3_wgrad', x, dz, dw, n, h, w, cin, cout, 1, wsb, nb, stream()))
    assert syms and all(s_.startswith('igemm') for s_ in syms), syms
    _check('maxabs', dw, f['dw'], case, 'wgrad dw(no-split)', sorted(set(syms)))
    # a valid pack: written by the forward pass of this very layer
    vb = query('fte_wino_pack_bytes', n, h, w, cin)
    assert vb == 16 * 4 * wino_map.geom(n, h, w)[1] * 64 * cin
    vpack = torch.empty(vb // 4, device='cuda')
    wt = torch.zeros(3, 3, cin, cout, device='cuda'); y = torch.empty(n, h, w, cout, device='cuda')
    wsf, nbf = ws(query('fte_conv3x3_fwd_ws_bytes', n, h, w, cin, cout, 1))
    call('fte_conv3x3_fwd_keep', x, wt, None, None, None, None, y, n, h, w, cin, cout, 1, vpack, wsf, nbf, stream())
    dw7 = torch.full((3, 3, cin, cout), 7.0, device='cuda')
    syms = _symbols(lambda: _expect(EWORKSPACE, 'fte_conv3x3_wgrad_kept', x.data_ptr(), dz.data_ptr(), dw7.data_ptr(), n, h, w, cin, cout, 1,
                                    vpack.data_ptr(), wsb.data_ptr(), nb, 0))
    assert syms == [] and bool((dw7 == 7.0).all())


def _expect(code, name, *args):
    r = query(name, *args)
    assert r == code, '%s returned %d, not %d' % (name, r, code)


@pytest.mark.parametrize('case', wino_cases.KEPT_CASES, ids=_id)
def test_kept_pack_on_ragged_row_blocks(winograd, case):
    """fte_conv3x3_fwd_keep writes V with the 256-thread tile transform, fte_conv3x3_wgrad transforms x itself with the 512-thread one:
    the same products bit for bit, on row blocks that are partly filled"""
    n, h, w, cin, cout = case
    r = np.random.default_rng(25)
    x = dev(r.standard_normal((n, h, w, cin))); wt = dev(r.standard_normal((3, 3, cin, cout)) * 0.05)
    dz = dev(r.standard_normal((n, h, w, cout)))
    assert query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 0) == WINOGRAD and query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 2) == WINOGRAD
    vpack = torch.full((query('fte_wino_pack_bytes', n, h, w, cin) // 4,), 7.0, device='cuda')
    wsb, nb = ws(max(query('fte_conv3x3_fwd_ws_bytes', n, h, w, cin, cout, 1), query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, 1)))
    y1 = torch.full((n, h, w, cout), 7.0, device='cuda'); y2 = torch.full_like(y1, 7.0)
    call('fte_conv3x3_fwd', x, wt, None, None, None, None, y1, n, h, w, cin, cout, 1, wsb, nb, stream())
    call('fte_conv3x3_fwd_keep', x, wt, None, None, None, None, y2, n, h, w, cin, cout, 1, vpack, wsb, nb, stream())
    assert torch.equal(y1, y2)
    dw1 = torch.full((3, 3, cin, cout), 7.0, device='cuda'); dw2 = torch.full_like(dw1, 7.0)
    call('fte_conv3x3_wgrad', x, dz, dw1, n, h, w, cin, cout, 1, wsb, nb, stream())
    syms = _symbols(lambda: call('fte_conv3x3_wgrad_kept', x, dz, dw2, n, h, w, cin, cout, 1, vpack, wsb, nb, stream()))
    assert syms == ['wino_wgrad_kernel'], syms
    assert torch.equal(dw1, dw2)
    print('WINO_EDGE kept    %-18s bit-equal' % _id(case))


FALLBACK = (3, 9, 7, 64, 128)


def test_small_workspace_sends_both_gradients_direct():
    """a workspace of the DIRECT setting's size under FTE_CONV_WINOGRAD: data gradient and filter gradient run the direct kernels (never
    an error, never a partial Winograd launch) and match the oracle"""
    n, h, w, cin, cout = FALLBACK
    prev = query('fte_get_conv_algo')
    try:
        call('fte_set_conv_algo', DIRECT)
        small_d = query('fte_conv3x3_dgrad_ws_bytes', n, h, w, cin, cout, 1); small_w = query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, 1)
        call('fte_set_conv_algo', WINOGRAD)
        big_d = query('fte_conv3x3_dgrad_ws_bytes', n, h, w, cin, cout, 1); big_w = query('fte_conv3x3_wgrad_ws_bytes', n, h, w, cin, cout, 1)
        assert big_d > small_d and big_w > small_w
        assert query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 1) == WINOGRAD and query('fte_conv3x3_algo', n, h, w, cin, cout, 1, 2) == WINOGRAD
        f = _ref('dgrad', FALLBACK)
        shape = f['dx'].shape
        raw = torch.full(shape, 7.0, device='cuda'); dzp = torch.full(shape, 7.0, device='cuda')
        da = torch.full((cin,), 7.0, device='cuda'); db = torch.full((cin,), 7.0, device='cuda')
        wsb = torch.empty(small_d // 4 + 4, device='cuda')
        args = (dev(f['dz']), dev(f['wt']), dev(f['addin']), dev(f['zprev']), dev(f['alp']), raw, dzp, da, db, n, h, w, cin, cout, 1, wsb, small_d, stream())
        syms = _symbols(lambda: call('fte_conv3x3_dgrad', *args))
        assert syms and all(s_.startswith('igemm') for s_ in syms), syms
        _check('maxabs', raw, f['g'], FALLBACK, 'dgrad raw(small-ws)', sorted(set(syms)))
        _check('maxabs', dzp, f['dzprev'], FALLBACK, 'dgrad dzprev(small-ws)', sorted(set(syms)))
        _check('rell2', da, f['dalpha'], FALLBACK, 'dgrad dalpha(small-ws)', sorted(set(syms)))
        _check('rell2', db, f['dbias'], FALLBACK, 'dgrad dbias(small-ws)', sorted(set(syms)))
        g = _ref('wgrad', FALLBACK)
        dw = torch.full((3, 3, cin, cout), 7.0, device='cuda')
        wsb = torch.empty(small_w // 4 + 4, device='cuda')
        syms = _symbols(lambda: call('fte_conv3x3_wgrad', dev(g['x']), dev(g['dz']), dw, n, h, w, cin, cout, 1, wsb, small_w, stream()))
        assert syms and all(s_.startswith('igemm') for s_ in syms), syms
        _check('maxabs', dw, g['dw'], FALLBACK, 'wgrad dw(small-ws)', sorted(set(syms)))
    finally:
        call('fte_set_conv_algo', prev)


def test_misaligned_pointers_are_argument_errors(winograd):
    """every tensor of the Winograd path moves 16 bytes per lane: a pointer 4 bytes off 16-byte alignment is FTE_EINVAL, nothing launched,
    nothing written"""
    n, h, w, cin, cout = FALLBACK
    pad = 8
    t = lambda *s: torch.full((int(np.prod(s)) + pad,), 7.0, device='cuda')       # room behind the shifted pointer
    x, wt, b, al, res, z, y = t(n, h, w, cin), t(3, 3, cin, cout), t(cout), t(cout), t(n, h, w, cout), t(n, h, w, cout), t(n, h, w, cout)
    dz, addin, zprev, alp, raw, dzp, dw = t(n, h, w, cout), t(n, h, w, cin), t(n, h, w, cin), t(cin), t(n, h, w, cin), t(n, h, w, cin), t(3, 3, cin, cout)
    vpack = t(query('fte_wino_pack_bytes', n, h, w, cin) // 4)
    nb = max(query('fte_conv3x3_%s_ws_bytes' % k, n, h, w, cin, cout, 1) for k in ('fwd', 'dgrad', 'wgrad'))
    wsb = torch.full((nb // 4 + pad,), 7.0, device='cuda')
    da, db = t(cin), t(cin)
    outs = [z, y, raw, dzp, dw, da, db, vpack, wsb]
    dims = [n, h, w, cin, cout, 1]

    def sweep(name, args, exempt=()):
        """one call per tensor of `args` with that pointer shifted by 4 bytes; the unshifted call is never made (it would write)"""
        for i, a in enumerate(args):
            if not isinstance(a, torch.Tensor) or any(a is e for e in exempt):
                continue
            p = [(q.data_ptr() + (4 if j == i else 0)) if isinstance(q, torch.Tensor) else q for j, q in enumerate(args)]
            syms = _symbols(lambda: _expect(EINVAL, name, *p))
            assert syms == [], (name, i, syms)
            assert all(bool((o == 7.0).all()) for o in outs), (name, i)

    sweep('fte_conv3x3_fwd', [x, wt, b, al, res, z, y] + dims + [wsb, nb, 0])
    sweep('fte_conv3x3_fwd_keep', [x, wt, b, al, res, z, y] + dims + [vpack, wsb, nb, 0])
    sweep('fte_conv3x3_dgrad', [dz, wt, addin, zprev, alp, raw, dzp, da, db] + dims + [wsb, nb, 0], exempt=(da, db))      # [cin] rows: 4-byte stores
    sweep('fte_conv3x3_wgrad', [x, dz, dw] + dims + [wsb, nb, 0])
    sweep('fte_conv3x3_wgrad_kept', [x, dz, dw] + dims + [vpack, wsb, nb, 0])


DGRAD_ONE = [(3, 9, 7, 128, 64), (5, 29, 27, 512, 64)]          # one partly filled row block (half tiles) | 17 row blocks of whole tiles


@pytest.mark.parametrize('case', DGRAD_ONE, ids=_id)
@pytest.mark.parametrize('which', ['dalpha', 'dbias'])
def test_dgrad_one_reduction_only(winograd, case, which):
    """dalpha without dbias and dbias without dalpha (zprev present): the row reduction over the one partial array"""
    n, h, w, cin, cout = case
    f = _ref('dgrad', case)
    dzp = torch.full(f['dx'].shape, 7.0, device='cuda')
    out = torch.full((cin,), 7.0, device='cuda')
    wsb, nb = ws(query('fte_conv3x3_dgrad_ws_bytes', n, h, w, cin, cout, 1))
    da, db = (out, None) if which == 'dalpha' else (None, out)
    syms = _symbols(lambda: call('fte_conv3x3_dgrad', dev(f['dz']), dev(f['wt']), dev(f['addin']), dev(f['zprev']), dev(f['alp']), None, dzp, da, db,
                                 n, h, w, cin, cout, 1, wsb, nb, stream()))
    assert syms == _mm_symbols(case, 1), (syms, _mm_symbols(case, 1))
    _check('maxabs', dzp, f['dzprev'], case, 'dgrad dzprev(%s-only)' % which, syms)
    _check('rell2', out, f[which], case, 'dgrad %s(only)' % which, syms)
