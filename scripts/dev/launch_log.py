"""Launch log of the SphereNet walks: every _lib.call, _lib.query and stream operation of a construction pass, three seeded Momentum
steps and one is_training=False forward, one row per event in order, for a list of configurations (nets, precision modes, switches).
Made to compare two trees of this package that load one libfte.so (FTE_LIB): a refactor of nets/sphere.py must leave the rows alone.

    python scripts/dev/launch_log.py --tree . --out logs/new [--standin] [--only TEXT]
    python scripts/dev/launch_log.py --tree ../parent --out logs/old [--standin]
    python scripts/dev/launch_log.py --compare logs/old logs/new

Rows.  C: entry point, then per argument a scalar, None, T<k>:<dtype>:<shape> (k: ordinal of the pointer's first appearance; every tensor
seen is kept alive, so an address names one buffer) and the stream as S<k>.  W / R: wait_event, wait_stream, record_event, record_stream.
Q: a query and its answer.  D: SHA-256 over params, grads with the loss slots, and state after a step (device runs only).
--compare holds the C, W, R and D rows of every configuration against each other, in order; Q rows are listed when their sequence
differs but do not fail it (they launch nothing, and which walk asks the library for the precision mode is the nets' business).
--standin runs without a device: tensors on the CPU, _lib.call does nothing, _lib.query answers from a fixed table, stand-in streams."""
import argparse, hashlib, os, sys

N, H, W, CH, NCLS = 8, 40, 24, 3, 10
NETS = [(net, mode) for net in ('SphereNet', 'SphereNet-ASoftmax') for mode in ('f32', 'bf16', 'bf16-nocopies', 'bf16s')] + \
       [('SphereNet-ArcFace', 'f32'), ('SphereNet-ArcFace-sampled', 'f32'), ('SphereNet-AdaFace', 'f32')]


def configurations():
    """(title, net, mode, env, extras)"""
    out = []
    for side in (None, '0', '1'):
        env = {} if side is None else {'FTE_SIDE_STREAM': side}
        out += [(' '.join([net, mode] + ['%s=%s' % kv for kv in env.items()]), net, mode, env, {}) for net, mode in NETS]
    a = 'SphereNet-ASoftmax'
    for k in ('FTE_WINO_KEEP', 'FTE_WINO_LEAN'):
        out.append(('%s f32 %s=0' % (a, k), a, 'f32', {k: '0'}, {}))
    out.append((a + ' f32 FTE_DZ_BUFFERS=2', a, 'f32', {'FTE_DZ_BUFFERS': '2'}, {}))
    out.append((a + ' bf16s FTE_DZ_BUFFERS=2', a, 'bf16s', {'FTE_DZ_BUFFERS': '2'}, {}))
    out.append((a + ' f32 conv_algo=0', a, 'f32', {}, {'algo': 0}))
    out.append((a + ' f32 backward_stages', a, 'f32', {}, {'stages': True}))
    out.append((a + ' bf16 one_stream', a, 'bf16', {}, {'one_stream': True}))
    out.append((a + ' f32 128 images FTE_FWD_HALVES=1', a, 'f32', {'FTE_FWD_HALVES': '1'}, {'n': 128}))
    out.append((a + ' f32 192 images FTE_FWD_HALVES=1 FTE_FWD_SPLIT=128', a, 'f32', {'FTE_FWD_HALVES': '1', 'FTE_FWD_SPLIT': '128'}, {'n': 192}))
    return out


class Log(object):
    def __init__(self, torch):
        self.torch, self.rows, self.keep, self.ptrs, self.streams, self.events = torch, [], [], {}, {}, {}

    def _ord(self, table, key):
        return table.setdefault(key, len(table))

    def stream(self, handle):
        return 'S%d' % self._ord(self.streams, handle)

    def arg(self, a, last):
        if a is None:
            return 'None'
        if hasattr(a, 'data_ptr'):
            self.keep.append(a)
            return 'T%d:%s:%s' % (self._ord(self.ptrs, a.data_ptr()), str(a.dtype).replace('torch.', ''), 'x'.join(map(str, a.shape)))
        if last and isinstance(a, int) and a in self.streams:
            return self.stream(a)
        return repr(a)

    def call(self, name, args):
        self.rows.append('C %s %s' % (name, ' '.join(self.arg(a, i == len(args) - 1) for i, a in enumerate(args))))

    def event(self, ev):
        self.keep.append(ev)
        return 'E%d' % self._ord(self.events, id(ev))


class StandinStream(object):
    """what the walks use of torch.cuda.Stream"""
    handles = 0

    def __init__(self, *a, **kw):
        StandinStream.handles += 1
        self.cuda_stream = 0xA0000000 + StandinStream.handles

    def wait_event(self, ev): pass
    def wait_stream(self, s): pass
    def record_event(self, ev=None): return object()
    def synchronize(self): pass


class StandinLib(object):
    """_lib.query from a fixed table: Winograd (1) for every stride-1 3x3 layer in fp32 unless fte_set_conv_algo(0), 4 KiB workspaces"""
    def __init__(self):
        self.mfma, self.algo = 0, 1

    def call(self, name, args):
        if name == 'fte_set_mfma_dtype':
            self.mfma = args[0]
        if name == 'fte_set_conv_algo':
            self.algo = args[0]

    def query(self, name, *a):
        if name == 'fte_get_mfma_dtype':
            return self.mfma
        if name == 'fte_get_conv_algo':
            return self.algo
        if name == 'fte_conv3x3_algo':
            return 1 if a[5] == 1 and self.mfma == 0 and self.algo != 0 else 0
        if name == 'fte_wino_pack_bytes':
            n, h, w, c = a
            return (n * ((h + 1) // 2) * ((w + 1) // 2) + 63) // 64 * 64 * c * 16 * 4
        if name.endswith('_ws_bytes'):
            return 4096
        raise KeyError('no stand-in answer for %s%r' % (name, a))


def instrument(torch, _lib, log, standin):
    """route _lib.call / _lib.query and the stream operations through `log`"""
    real_call, real_query = _lib.call, _lib.query
    fake = StandinLib() if standin else None

    def call(name, *args):
        log[0].call(name, args)
        return fake.call(name, args) if standin else real_call(name, *args)

    def query(name, *args):
        r = fake.query(name, *args) if standin else real_query(name, *args)
        log[0].rows.append('Q %s %s -> %r' % (name, ' '.join(map(repr, args)), r))
        return r
    _lib.call, _lib.query = call, query
    if standin:
        main = StandinStream()
        _lib.load = lambda: None
        torch.cuda.Stream, torch.cuda.current_stream, torch.cuda.synchronize = StandinStream, lambda *a: main, lambda *a: None
        torch.cuda.current_device = lambda: 0
    S = torch.cuda.Stream

    def wrap(name, tag, what):
        inner = getattr(S, name)

        def op(self, *a):
            r = inner(self, *a)
            log[0].rows.append('%s %s %s %s' % (tag, name, log[0].stream(self.cuda_stream), what(a, r)))
            return r
        setattr(S, name, op)
    wrap('wait_event', 'W', lambda a, r: log[0].event(a[0]))
    wrap('wait_stream', 'W', lambda a, r: log[0].stream(a[0].cuda_stream))
    wrap('record_event', 'R', lambda a, r: log[0].event(r))
    inner_rs = torch.Tensor.record_stream

    def record_stream(self, s):
        log[0].rows.append('R record_stream %s %s' % (log[0].arg(self, False), log[0].stream(s.cuda_stream)))
        return None if standin else inner_rs(self, s)
    torch.Tensor.record_stream = record_stream


def run_one(torch, pkg, _lib, log, cfg, standin):
    title, name, mode, env, extra = cfg
    n = extra.get('n', N)
    dev = torch.device('cpu' if standin else 'cuda:0')

    class OnDevice(torch.Tensor):                        # (stand-in inputs pass the nets' "is a device tensor" checks)
        is_cuda = property(lambda self: True)
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(n, H, W, CH, generator=g) * 2 - 1).to(dev)
    y = torch.randint(0, NCLS, (n,), generator=g, dtype=torch.int32).to(dev)
    if standin:
        x, y = x.as_subclass(OnDevice), y.as_subclass(OnDevice)
    saved = {k: os.environ.get(k) for k in env}
    prev_algo = _lib.query('fte_get_conv_algo')
    log[0] = Log(torch)
    log[0].stream(torch.cuda.current_stream().cuda_stream)
    try:
        os.environ.update(env)
        _lib.set_mfma_dtype(mode.split('-')[0])
        if 'algo' in extra:
            _lib.call('fte_set_conv_algo', extra['algo'])
        net = pkg.net_select(name.replace('-sampled', ''), 'NCHW', 5e-4)
        if mode.endswith('nocopies'):
            net.bf16_copies = False
        if name.endswith('-sampled'):
            net.set_sample_rate(0.8, 3)                  # S = 8 classes of 10
        net.seed = 11
        if extra.get('one_stream'):
            net.one_stream = True
        if extra.get('stages'):
            def backward():
                for stage in net.backward_stages():
                    stage()
                    torch.cuda.synchronize()
            net.backward = backward
        step, losses, names, others = pkg.Singular(net, 0.05, 'Momentum')({'images': x, 'labels': y, 'num_classes': NCLS, 'num_examples': n})
        for k in range(3):
            log[0].rows.append('- step %d' % k)
            step()
            torch.cuda.synchronize()
            if not standin:
                h = hashlib.sha256()
                for t in [net.params, net.grads] + list(net.state.values()):
                    h.update(t.detach().cpu().numpy().tobytes())
                log[0].rows.append('D step %d %s' % (k, h.hexdigest()))
        log[0].rows.append('- eval')
        net.forward(x, is_training=False)
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        _lib.set_mfma_dtype('f32')
        _lib.call('fte_set_conv_algo', prev_algo)
    return log[0].rows


def compare(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        ra, rb = [open(os.path.join(d, f)).read().splitlines() for d in (a, b)]
        hard = [[r for r in rows if r[0] != 'Q'] for rows in (ra, rb)]
        soft = [[r for r in rows if r[0] == 'Q'] for rows in (ra, rb)]
        same = hard[0] == hard[1]
        bad += not same
        digests = sum(r[0] == 'D' for r in hard[0])
        print('| `%s` | %d / %d | %s | %s | %d / %d%s |' % (f[:-4], len(hard[0]), len(hard[1]), 'identical' if same else 'DIFFERENT',
              ('equal' if same else 'see log') if digests else '-', len(soft[0]), len(soft[1]), '' if soft[0] == soft[1] else ' (differ)'))
        if not same:
            k = next((i for i, (p, q) in enumerate(zip(*hard)) if p != q), min(map(len, hard)))
            print('    first difference at row %d:\n      %s\n      %s' % (k, hard[0][k:k + 1], hard[1][k:k + 1]))
    print('%d configurations, %d differ' % (len(os.listdir(a)), bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    ap.add_argument('--out')
    ap.add_argument('--standin', action='store_true')
    ap.add_argument('--only', default='')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(*args.compare) else 0)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import tf_face_toolbox_amd as pkg
    from tf_face_toolbox_amd import _lib
    assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(args.tree)), pkg.__file__
    log = [Log(torch)]
    instrument(torch, _lib, log, args.standin)
    os.makedirs(args.out, exist_ok=True)
    for cfg in configurations():
        if args.only in cfg[0]:
            rows = run_one(torch, pkg, _lib, log, cfg, args.standin)
            with open(os.path.join(args.out, cfg[0].replace(' ', '_') + '.log'), 'w') as f:
                f.write('\n'.join(rows) + '\n')
            print('%-70s %6d rows' % (cfg[0], len(rows)), flush=True)


if __name__ == '__main__':
    main()
