"""Planning for the graph engine (nets/graph.py): everything that is decided before a buffer exists.  Plain functions of the
graph description (the op list the oracle executes too, oracle/graphnet.py), the variable spec and the options record; no device
tensor is made here and nothing of libfte.so is called, so a plan can be built, dumped and compared on any machine.

  read_options   every FTE_* switch of the graph engine, read once when a net is built
  compile_net    stem width, shapes, typed plan ops, fusion tables -> Plan
  segments       the equal-bytes rule that cuts the body into all-reduce buckets

A plan op is a named record, one type per kind; field 0 is the kind and field 1 the output tensor."""
import os
from collections import namedtuple

Options = namedtuple('Options', [
    'bn_fuse',          # FTE_BN_FUSE (1): a conv / grouped conv leaves the batch statistics of the BN behind it in its epilogue
    'bn_fuse_3x3',      # FTE_BN_FUSE_3X3 (1): ... the 3x3 and grouped convs under bf16 storage too
    'bn_fuse_bwd',      # FTE_BN_FUSE_BWD (0, opt-in): a conv's data gradient takes the mask / sums of the BN layer below
    'bn_fuse_gbwd',     # FTE_BN_FUSE_GBWD (0, opt-in): a grouped conv's data gradient does
    'bn_fold',          # FTE_BN_FOLD (1): the normalise pass of a BN + ReLU moves into its consumer's operand loader
    'bn_gather',        # FTE_BN_GATHER (1): a BN whose only consumer is a channel gather is applied inside the gather
    'se_fuse',          # FTE_SE_FUSE (1): BN -> SE gate -> add -> ReLU as one plan op ('seblock'); 'selin' (no ReLU) has no other form
    'se_act_fuse',      # FTE_SE_ACT_FUSE (1): the unfused SE gate's dense layers carry their activation
    'se_dense',         # FTE_SE_DENSE (1): the fused SE block's dense layers through fte_dense_small where it applies
    'direct_stem',      # FTE_DIRECT_STEM (1): a 3x3 stem of <= 32 filters is stored 32 wide and runs on the direct kernel
    'gconv_mfma',       # FTE_GCONV_MFMA (1): grouped 3x3 on the bf16 matrix cores in the bf16 modes
    'side_stream',      # FTE_SIDE_STREAM (1): filter gradients (and what follows below) on a second stream
    'side_prio',        # FTE_SIDE_PRIO (0): that stream's priority
    'side_batch',       # FTE_SIDE_BATCH (3): filter gradients queued before the side stream is released
    'shortcut_side',    # FTE_SHORTCUT_SIDE (1): the residual blocks' shortcut branches run on the side stream in the forward walk
    'head_side',        # FTE_HEAD_SIDE (1): the classifier's filter gradient runs there
    'reg_side',         # FTE_REG_SIDE (1): the weight-decay sum runs there, under the first layers
    'pack_after_stem',  # FTE_PACK_AFTER_STEM (1): bf16 storage, 7x7 stem: the filter packs start behind the im2col
    'pack_head',        # FTE_PACK_HEAD (4): filters packed on the main stream before the walk starts
    'grad_buckets',     # FTE_GRAD_BUCKETS (4): all-reduce buckets of the body
])


def read_options(env=None):
    """The graph engine's switches as one immutable record.  GraphNet.build() calls this, so a switch acts on the nets built after
    it is set (the precision mode is not one of them: it is asked of _lib at every step)."""
    env = os.environ if env is None else env
    on = lambda k: env.get(k, '1') != '0'
    return Options(
        bn_fuse=on('FTE_BN_FUSE'), bn_fuse_3x3=on('FTE_BN_FUSE_3X3'), bn_fuse_bwd=env.get('FTE_BN_FUSE_BWD', '0') == '1',
        bn_fuse_gbwd=env.get('FTE_BN_FUSE_GBWD', '0') == '1', bn_fold=on('FTE_BN_FOLD'), bn_gather=on('FTE_BN_GATHER'),
        se_fuse=on('FTE_SE_FUSE'), se_act_fuse=on('FTE_SE_ACT_FUSE'), se_dense=on('FTE_SE_DENSE'), direct_stem=on('FTE_DIRECT_STEM'),
        gconv_mfma=env.get('FTE_GCONV_MFMA', '1') != '0', side_stream=on('FTE_SIDE_STREAM'), side_prio=int(env.get('FTE_SIDE_PRIO', '0')),
        side_batch=int(env.get('FTE_SIDE_BATCH', '3')), shortcut_side=on('FTE_SHORTCUT_SIDE'), head_side=on('FTE_HEAD_SIDE'),
        reg_side=on('FTE_REG_SIDE'), pack_after_stem=on('FTE_PACK_AFTER_STEM'), pack_head=int(env.get('FTE_PACK_HEAD', '4')),
        grad_buckets=int(env.get('FTE_GRAD_BUCKETS', '4')))


# ---- plan ops -------------------------------------------------------------------------------------------
Conv = namedtuple('Conv', 'kind out inp wname stride')
GConv = namedtuple('GConv', 'kind out inp wname stride groups')
DwConv = namedtuple('DwConv', 'kind out inp wname stride')
Bn = namedtuple('Bn', 'kind out inp pre res relu')                    # 'bn', and 'bnstats' (statistics only: applied inside a gather)
BnPrelu = namedtuple('BnPrelu', 'kind out inp pre alpha')
# w1 .. hidden: weight / bias names of the gate's two dense layers and the (padded) hidden width
Se = namedtuple('Se', 'kind out inp pre scope1 scope2 w1 b1 w2 b2 hidden')
SeBlock = namedtuple('SeBlock', 'kind out inp pre shortcut se y s')    # se: the Se it absorbed; y, s: the BN output / gated tensor that no longer exist
# BN -> SE gate -> add shortcut with NO activation (the SE-IResNet block tail): the fields of SeBlock, kernels of their own
SeLin = namedtuple('SeLin', SeBlock._fields)
AddRelu = namedtuple('AddRelu', 'kind out a b')
Add = namedtuple('Add', 'kind out a b')                                # a bare add behind an SE gate: exists only until _fuse_se_lin has run
# ins: (a, b | None); outs / bwd: [(tensor, table)], table = int32 words (src << 16 | channel, -1: none); gouts: (out0, out1 | None)
Gather = namedtuple('Gather', 'kind out ins outs gouts bwd')
MaxPool = namedtuple('MaxPool', 'kind out inp')
Gap = namedtuple('Gap', 'kind out inp')
Dropout = namedtuple('Dropout', 'kind out inp keep')
Fc = namedtuple('Fc', 'kind out inp wname bias embed')                # embed: a dense layer of the body (on a flattened map), not the classifier

RECORDS = {'conv': Conv, 'gconv': GConv, 'dwconv': DwConv, 'bn': Bn, 'bnstats': Bn, 'bnprelu': BnPrelu, 'seblock': SeBlock, 'se': Se,
           'selin': SeLin, 'addrelu': AddRelu, 'gather': Gather, 'maxpool': MaxPool, 'gap': Gap, 'dropout': Dropout, 'fc': Fc}

Plan = namedtuple('Plan', 'plan shapes real_c narrow embed_in folded se_fused fuse_fwd fuse_bwd fold_apply shortcut_fwd shortcut_shared '
                          'has_classifier')


def stem_kpad(k, cin):
    """rows of the im2col'ed stem weight, zero-padded to a multiple of 32 (7*7*3 = 147 -> 160, 3*3*3 = 27 -> 32)"""
    return (k * k * cin + 31) // 32 * 32


def shuffle_perm(c, data_format):
    """_channel_shuffle (nets/shufflenet_v2.py:66-77) as an index vector: out[k] = in[perm[k]].  The reference's NCHW
    branch views channels as [2, C/2] and transposes; its NHWC branch views them as [C/2, 2] -- a different permutation."""
    assert c % 2 == 0, c
    if data_format == 'NCHW':
        return [j * (c // 2) + i for i in range(c // 2) for j in range(2)]
    return [i * 2 + j for j in range(2) for i in range(c // 2)]


def direct_stem(k, cin, cout, options):
    """3x3 first conv on 1 / 3 image channels with 32 or 64 stored filters: fte_conv3x3_first_* (K = 9*cin is too short for
    the GEMM path's im2col round trip through HBM)"""
    return k == 3 and cin in (1, 3) and cout in (32, 64) and options.direct_stem


def _pad(c, p):
    return (c + p - 1) // p * p


def _out_size(size, stride):
    return -(-size // stride)                            # 'SAME' padding


def narrow_variables(graph, spec, channel_pad, options):
    """A 3x3 stem of at most 32 filters (ShuffleNet-v2 small: 24) is stored 32 channels wide, not channel_pad wide: its
    56x56 output is the largest tensor of the net, and every pass over it (BN statistics / apply, max-pool, their
    gradients) is pure HBM traffic -- 64-wide storage made 62 % of those bytes padding.  -> the variables (filter, BN
    gamma / beta) that follow that width."""
    narrow = set()
    if channel_pad > 32 and options.direct_stem:
        for op in graph:
            if op[0] == 'conv':
                _, out, _, wname, _ = op
                k, _, cin, cout = spec[wname][0]
                if cin <= 4 and k == 3 and cout <= 32:
                    narrow.add(wname)
                    for o2 in graph:
                        if o2[0] == 'bn' and o2[2] == out:
                            narrow.update([o2[3] + '/gamma', o2[3] + '/beta'])
    return narrow


def infer_shapes(graph, spec, in_hwc, channel_pad, narrow, num_classes, logits_width):      # (one branch per graph kind: longer than the rest)
    """-> shapes: stored (channel-padded) shape of every tensor; real_c: its true channel count; embed_in: 'embed_w' variable ->
    (h, w, c) of the feature map its FC flattens."""
    h, w, c = in_hwc
    shp = {'images': (h, w, c)}
    real = {'images': c}
    embed_in = {}
    pc = lambda cc: _pad(cc, channel_pad)

    def put(name, hh, ww, cc):
        real[name] = cc
        shp[name] = (hh, ww, pc(cc))
    for op in graph:
        kind, out, inp = op[0], op[1], op[2]
        if kind == 'conv':
            _, _, _, wname, stride = op
            ih, iw, _ = shp[inp]
            k, _, cin, cout = spec[wname][0]
            assert cin == real[inp], (op, cin, real[inp])
            put(out, _out_size(ih, stride), _out_size(iw, stride), cout)
            if wname in narrow:
                shp[out] = shp[out][:2] + (_pad(cout, 32),)
        elif kind in ('gconv', 'dwconv'):
            stride = op[4]
            ih, iw, _ = shp[inp]
            put(out, _out_size(ih, stride), _out_size(iw, stride), real[inp])
        elif kind in ('bn', 'relu', 'dropout', 'se', 'add', 'prelu'):
            shp[out] = shp[inp]
            real[out] = real[inp]
        elif kind == 'maxpool':
            ih, iw, cp = shp[inp]
            put(out, _out_size(ih, 2), _out_size(iw, 2), real[inp])
            shp[out] = shp[out][:2] + (cp,)                 # keeps its input's stored width
        elif kind == 'gap':
            shp[out] = (shp[inp][2],)
            real[out] = real[inp]
        elif kind == 'fc' and spec[op[3]][1] == 'embed_w':      # dense layer on the flattened [n, h w c] map (or on [n, c])
            wname = op[3]
            fin, d = spec[wname][0]
            src = shp[inp]
            assert channel_pad == 1 and fin == _prod(src) and d % 64 == 0 and fin % 32 == 0, (op, src, fin, d)
            embed_in[wname] = src if len(src) == 3 else (1, 1, src[0])
            shp[out] = (d,)
            real[out] = d
        elif kind == 'fc':
            shp[out] = (logits_width,)
            real[out] = num_classes
        elif kind == 'split':
            _, _, _, out_b = op
            ih, iw, _ = shp[inp]
            cc = real[inp]
            put(out, ih, iw, int(0.5 * cc))
            put(out_b, ih, iw, cc - int(0.5 * cc))
        elif kind == 'shufsplit':
            _, _, a, b, out_x, _ = op
            ih, iw, _ = shp[a]
            cc = real[a] + real[b]
            put(out, ih, iw, int(0.5 * cc))
            put(out_x, ih, iw, cc - int(0.5 * cc))
        elif kind == 'shufcat':
            _, _, a, b, _ = op
            ih, iw, _ = shp[a]
            put(out, ih, iw, real[a] + real[b])
        else:
            raise ValueError(kind)
    _check_narrow_consumers(graph, spec, shp, real, pc)
    return shp, real, embed_in


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _check_narrow_consumers(graph, spec, shp, real, pc):
    """A tensor stored narrower than channel_pad (the 32-wide stem) may only feed ops that take their width from the stored
    input: BN / ReLU / max-pool, the channel gathers, and a 1x1 conv (which reads a valid row prefix).  A 3x3, grouped or
    depthwise conv, an SE gate or an add would lay out its weights / output for pc(real) channels while the kernel is
    launched with the stored width -- a silent wrong stride.  No net of the factory does that; a new one must not."""
    narrow_stored = {n for n in shp if n != 'images' and len(shp[n]) == 3 and shp[n][2] != pc(real[n])}
    for op in graph:
        ins = [a for a in op[2:] if isinstance(a, str) and a in narrow_stored]
        if not ins:
            continue
        ok = op[0] in ('bn', 'relu', 'maxpool', 'split', 'shufsplit', 'shufcat', 'dropout') or \
            (op[0] == 'conv' and spec[op[3]][0][0] == 1)
        assert ok, 'op %r consumes %s, which is stored %d channels wide (not %d): unsupported consumer of the narrow stem' % (
            op, ins[0], shp[ins[0]][2], pc(real[ins[0]]))


def _table(entries, width):
    """int32 words of a gather table of `width` slots from [(src, channel) or None]"""
    t = [-1] * width
    for k, e in enumerate(entries):
        if e is not None:
            t[k] = (e[0] << 16) | e[1]
    return t


def gather_tables(op, shapes, real_c):
    """Forward and backward channel-gather tables of a split / shufsplit / shufcat graph op (fte_channel_gather) -> Gather"""
    kind, out = op[0], op[1]
    real, shp = real_c, shapes
    if kind == 'split':                                   # nets/shufflenet_v2.py:60-64
        _, _, inp, out_b = op
        cc = real[inp]
        h = int(0.5 * cc)
        fwd = [(out, _table([(0, k) for k in range(h)], shp[out][2])),
               (out_b, _table([(0, h + k) for k in range(cc - h)], shp[out_b][2]))]
        bwd = [(inp, _table([(0, k) if k < h else (1, k - h) for k in range(cc)], shp[inp][2]))]
        return Gather('gather', out, (inp, None), fwd, (out, out_b), bwd)
    a, b = op[2], op[3]
    ca, cb = real[a], real[b]
    cc = ca + cb
    perm = shuffle_perm(cc, op[-1])                       # shuffled[k] = cat[perm[k]]
    src = [(0, j) if j < ca else (1, j - ca) for j in perm]
    if kind == 'shufsplit':
        out_x = op[4]
        h = int(0.5 * cc)
        fwd = [(out, _table(src[:h], shp[out][2])), (out_x, _table(src[h:], shp[out_x][2]))]
        gouts = (out, out_x)
        where = lambda k: (0, k) if k < h else (1, k - h)
    else:
        fwd = [(out, _table(src, shp[out][2]))]
        gouts = (out, None)
        where = lambda k: (0, k)
    inv = [None] * cc
    for k, j in enumerate(perm):
        inv[j] = where(k)
    bwd = [(a, _table(inv[:ca], shp[a][2])), (b, _table(inv[ca:], shp[b][2]))]
    return Gather('gather', out, (a, b), fwd, gouts, bwd)


def graph_inputs(op):
    """tensors a GRAPH op reads"""
    if op[0] in ('add', 'shufsplit', 'shufcat'):
        return [op[2], op[3]]
    return [op[2]]


def plan_inputs(op):
    """tensors a PLAN op reads"""
    kind = op[0]
    if kind == 'gather':
        return [x for x in op.ins if x is not None]
    if kind == 'bn':
        return [op.inp] + ([op.res] if op.res is not None else [])
    if kind in ('addrelu', 'add'):
        return [op.a, op.b]
    if kind in ('seblock', 'selin'):
        return [op.inp, op.shortcut]
    return [op.inp] if kind in RECORDS else graph_inputs(op)


def op_weight_names(op):
    """filters of a plan op, in arena order"""
    kind = op[0]
    if kind in ('conv', 'gconv', 'dwconv') or (kind == 'fc' and op.embed):
        return [op.wname]
    if kind in ('se', 'seblock', 'selin'):
        se = op.se if kind != 'se' else op
        return [se.w1, se.w2]
    return []


def _users(ops, inputs):
    users = {}
    for j, op in enumerate(ops):
        for x in inputs(op):
            users.setdefault(x, []).append(j)
    return users


def _defined_before(graph, name, idx):
    if name == 'images':
        return True
    for j in range(idx):
        o = graph[j]
        if o[1] == name or (o[0] == 'split' and o[3] == name) or (o[0] == 'shufsplit' and o[4] == name):
            return True
    return False


def _se_record(op, spec, channel_pad):
    """('se', out, inp, prefix[, scope1, scope2]) -> Se with the names of the two FCs and the (stored) hidden width resolved"""
    _, out, inp, pre = op[:4]
    s1, s2 = (op[4], op[5]) if len(op) > 4 else ('fc1', 'fc2')
    w1 = pre + '/%s/weights' % s1
    return Se('se', out, inp, pre, s1, s2, w1, pre + '/%s/biases' % s1, pre + '/%s/weights' % s2, pre + '/%s/biases' % s2,
              _pad(spec[w1][0][-1], channel_pad))


def _fuse_graph(graph, spec, shapes, real_c, channel_pad, name, hidden_pad=None):
    """Graph ops -> plan ops: bn -> relu, bn -> add -> relu and bn -> prelu become one BN op each, add -> relu one 'addrelu', the
    channel splits / shuffles one 'gather' with its tables; everything else is typed as it stands."""
    g = graph
    users = _users(g, graph_inputs)
    plan, skip = [], set()
    for i, op in enumerate(g):
        if i in skip:
            continue
        kind = op[0]
        if kind == 'bn':
            _, out, inp, pre = op
            res, relu, final = None, 0, out
            u = users.get(out, [])
            if len(u) == 1 and g[u[0]][0] == 'relu':
                relu, final = 1, g[u[0]][1]
                skip.add(u[0])
            elif len(u) == 1 and g[u[0]][0] == 'prelu':      # bn -> prelu: one plan op (fte_bn_prelu_apply / _train_bwd)
                _, pout, _, alpha = g[u[0]]
                skip.add(u[0])
                plan.append(BnPrelu('bnprelu', pout, inp, pre, alpha))
                continue
            elif len(u) == 1 and g[u[0]][0] == 'add':
                _, aout, a, b = g[u[0]]
                other = b if a == out else a
                u2 = users.get(aout, [])
                if len(u2) == 1 and g[u2[0]][0] == 'relu' and _defined_before(g, other, i):
                    res, relu, final = other, 1, g[u2[0]][1]
                    skip.update([u[0], u2[0]])
                elif not any(g[k][0] == 'relu' for k in u2) and other != out and _defined_before(g, other, i):
                    # bn -> add with NO activation (the IResNet block's last BN plus shortcut): fte_bn_apply(res, relu = 0);
                    # backward: the gradient goes unmasked into the BN backward and unchanged to the shortcut
                    res, final = other, aout
                    skip.add(u[0])
            plan.append(Bn('bn', final, inp, pre, res, relu))
        elif kind == 'prelu':
            raise ValueError('%s: prelu %r does not directly follow a bn that feeds nothing else (its input is %r): only the fused '
                             'bn -> prelu pair is implemented' % (name, op[1], op[2]))
        elif kind == 'add':
            _, out, a, b = op
            u = users.get(out, [])
            if not any(g[k][0] == 'relu' for k in u) and any(o[0] == 'se' and o[1] in (a, b) for o in g[:i]):
                plan.append(Add('add', out, a, b))           # SE gate -> add, no activation: _fuse_se_lin takes it (or compile_net raises)
                continue
            assert len(u) == 1 and g[u[0]][0] == 'relu', 'a bare add is always followed by a ReLU in these nets'
            skip.add(u[0])
            plan.append(AddRelu('addrelu', g[u[0]][1], a, b))
        elif kind in ('split', 'shufsplit', 'shufcat'):
            plan.append(gather_tables(op, shapes, real_c))
        elif kind == 'se':
            plan.append(_se_record(op, spec, channel_pad if hidden_pad is None else hidden_pad))
        elif kind == 'fc':
            plan.append(Fc(*op, embed=spec[op[3]][1] == 'embed_w'))
        elif kind in RECORDS:
            plan.append(RECORDS[kind](*op))
        else:
            plan.append(op)                                  # (a kind no walk knows, e.g. a bare relu: the walks raise on it)
    return plan


def _fuse_se_blocks(plan, shapes, feature_name, se_fused, tail='addrelu', record=SeBlock):
    """('bn', y, z, pre, None, 0) -> ('se', s, y, ...) -> ('addrelu', out, s, shortcut), each the only user of its input, becomes
    ('seblock', out, z, pre, shortcut, se op, y, s) at the add's place (nets/resnet.py:63-92 with use_se).  With tail = 'add' and
    record = SeLin: the same sequence ending in an add without activation -> 'selin' (the SE-IResNet block, nets/iresnet.py)."""
    users = _users(plan, plan_inputs)
    drop, repl = set(), {}
    for j, op in enumerate(plan):
        if op[0] != 'bn' or op.res is not None or op.relu or len(shapes[op.out]) != 3 or op.out == feature_name:
            continue
        u = users.get(op.out, [])
        if len(u) != 1 or plan[u[0]][0] != 'se' or plan[u[0]].inp != op.out:
            continue
        se = plan[u[0]]
        u2 = users.get(se.out, [])
        if len(u2) != 1 or plan[u2[0]][0] != tail or se.out == feature_name:
            continue
        ar = plan[u2[0]]
        sc = ar.b if ar.a == se.out else ar.a
        if sc == se.out or shapes[sc] != shapes[op.out] or shapes[op.out][-1] % 4:
            continue
        repl[u2[0]] = record(record.__name__.lower(), ar.out, op.inp, op.pre, sc, se, op.out, se.out)
        drop.update([j, u[0]])
        se_fused[op.out] = ('y', ar.out, op.inp)
        se_fused[se.out] = ('s', ar.out, op.inp)
    return [repl.get(j, op) for j, op in enumerate(plan) if j not in drop]


def _fold_into_gathers(plan, pusers, feature_name):
    """A BN(+ReLU) output whose only consumer is a channel gather (conv3_1x1 and the stride-2 shortcut's 1x1 of a
    ShuffleNet block, nets/shufflenet_v2.py:96-113) is normalised INSIDE the gather: the BN op keeps its statistics
    pass only ('bnstats'), the gather applies scale / shift / ReLU to that source on the way
    (fte_channel_gather_affine), and the normalised tensor is never written (FTE_BN_GATHER=0: off, A/B hook).
    -> folded: name -> (z, relu)"""
    folded = {}
    for j, op in enumerate(plan):
        if op[0] == 'bn' and op.res is None:
            u = pusers.get(op.out, [])
            if len(u) == 1 and plan[u[0]][0] == 'gather' and op.out != feature_name:
                plan[j] = op._replace(kind='bnstats')
                folded[op.out] = (op.inp, op.relu)
    return folded


def _bn_fusion(plan, pusers, feature_name):
    """"BN fusion" (fte.h): a conv / grouped conv whose output feeds ONE batch norm leaves that layer's batch statistics in its
    epilogue (fuse_fwd: plan index of the conv -> plan index of the BN), and the data gradient that completes the gradient of
    a BN layer's OUTPUT -- the dgrad of its first consumer in plan order, which runs last in the backward walk and takes the
    other consumer's contribution through `addin` -- applies the ReLU mask and leaves the two sums of the BN backward
    (fuse_bwd: name of the BN output -> plan index of the BN).  Which of them can run fused (MFMA conv path, storage
    mode, grouped conv on the bf16 MFMA) is decided where they run.  FTE_BN_FUSE=0: off (A/B hook).
    The backward half is OPT-IN (FTE_BN_FUSE_BWD=1 / FTE_BN_FUSE_GBWD=1).  Measured on MI355X at 128 images per GPU, ms per step,
    forward only / + conv data gradients / + grouped-conv data gradients / no fusion: ResNeXt-50 7.84 / 7.91 / 8.17 / 8.23, ResNet-50
    7.27 / 7.38 / - / 7.66, SE-ResNet-50 9.52 / 9.40 / - / 9.87, ShuffleNet-v2 (fp32, 256) 8.10 / 8.11 / - / 8.60: the tile kernels'
    epilogue waits for its three extra inputs with 3 blocks per CU, which costs what the separate reduce pass cost."""
    fuse_fwd, fuse_bwd = {}, {}
    producer = {op[1]: j for j, op in enumerate(plan) if op[0] in ('conv', 'gconv')}
    prelu_net = any(op[0] == 'bnprelu' for op in plan)
    for j, op in enumerate(plan):
        if op[0] not in ('bn', 'bnstats', 'seblock', 'selin', 'bnprelu'):
            continue
        i = producer.get(op.inp)
        if i is not None and pusers.get(op.inp, []) == [j]:
            fuse_fwd[i] = j
        us = pusers.get(op.out, [])
        if op[0] == 'bn' and us and op.out != feature_name and not prelu_net:      # (the opt-in backward fusion is not taken by the BN + PReLU nets)
            first = plan[us[0]]
            if (first[0] == 'conv' and len(us) <= 2) or (first[0] == 'gconv' and len(us) == 1):
                fuse_bwd[op.out] = j
    return fuse_fwd, fuse_bwd


def _fold_apply(plan, pusers, feature_name, fuse_fwd):
    """... and the normalise pass of a BN + ReLU whose output feeds ONE conv / grouped conv that itself runs fused can move into
    that consumer's operand loader (fold_apply: plan index of the BN -> plan index of the consumer): the consumer reads the
    BN's input z, applies scale / shift / ReLU on the way to the matrix cores and writes the normalised tensor back for the
    filter gradient; the bn_apply launch and its pass over the tensor disappear (fte.h, fte_conv2d_bn_fwd's in_scale).
    Whether the consumer's kernel takes it (bf16 storage, pointwise stride-1 conv of 64 / 128 / 256 channels, or a
    stride-1 grouped conv on the bf16 MFMA) is decided where it runs.  FTE_BN_FOLD=0: off (A/B hook)."""
    fold = {}
    fused_bns = set(fuse_fwd.values())
    for j, op in enumerate(plan):
        if op[0] == 'bn' and op.res is None and op.relu and op.out != feature_name and j in fused_bns:
            us = pusers.get(op.out, [])
            if len(us) == 1 and us[0] in fuse_fwd and plan[us[0]][0] in ('conv', 'gconv') and plan[us[0]].inp == op.out:
                fold[j] = us[0]
    return fold


def _shortcut_branches(plan, pusers, feature_name):
    """Shortcut branches of the residual blocks (conv 1x1 -> BN without activation, consumed only as the `res` of the block's last
    BN or by its add + ReLU): independent of the block's main branch, so the forward walk queues them on the side stream and the
    consumer waits for their event (shortcut_fwd: plan index -> True for the conv and the BN).  FTE_SHORTCUT_SIDE=0: off (A/B hook)."""
    shortcut_fwd = {}
    producer = {op[1]: j for j, op in enumerate(plan) if op[0] == 'conv'}
    for j, op in enumerate(plan):
        if op[0] != 'bn' or op.res is not None or op.relu:
            continue
        us = pusers.get(op.out, [])
        if len(us) != 1 or op.out == feature_name:
            continue
        cons = plan[us[0]]
        as_res = (cons[0] == 'bn' and cons.res == op.out and cons.inp != op.out) or (cons[0] == 'addrelu' and op.out in (cons.a, cons.b)) or \
            (cons[0] in ('seblock', 'selin') and cons.shortcut == op.out and cons.inp != op.out)
        i = producer.get(op.inp)
        if as_res and i is not None and pusers.get(op.inp, []) == [j] and i == j - 1:
            shortcut_fwd[i] = True
            shortcut_fwd[j] = True
    return shortcut_fwd


def compile_net(graph, spec, in_hwc, channel_pad, feature_name, options, num_classes, logits_width, name='', se_hidden_pad=None):
    """The whole static analysis of a net -> Plan.  `spec`: variable name -> (reference shape, kind); `logits_width`: stored
    columns of the classifier output; `se_hidden_pad`: multiple the SE gates' hidden width is stored at (None: channel_pad)."""
    narrow = narrow_variables(graph, spec, channel_pad, options)
    shapes, real_c, embed_in = infer_shapes(graph, spec, in_hwc, channel_pad, narrow, num_classes, logits_width)
    plan = _fuse_graph(graph, spec, shapes, real_c, channel_pad, name, se_hidden_pad)
    # SE residual block: BN (no activation) -> SE gate -> add shortcut -> ReLU becomes ONE plan op whose kernels read the BN's input z
    # and write the block's output; the BN output and the gated tensor never exist (csrc/layers.hip "SE residual block",
    # fte_se_*).  FTE_SE_FUSE=0: the separate ops (A/B hook).
    se_fused = {}
    if options.se_fuse:
        plan = _fuse_se_blocks(plan, shapes, feature_name, se_fused)
        # ... and without the ReLU (the SE-IResNet block tail): 'selin', fte_se_lin_* (csrc/iresnet.hip)
        plan = _fuse_se_blocks(plan, shapes, feature_name, se_fused, 'add', SeLin)
    bare = [op.out for op in plan if op[0] == 'add']
    if bare:
        raise ValueError('%s: BN -> SE gate -> add without an activation (%s%s) runs only as the fused plan op %r; %s' % (
            name, bare[0], ', ...' if len(bare) > 1 else '', 'selin',
            'there is no unfused path for it: unset FTE_SE_FUSE=0' if not options.se_fuse else
            'the BN, the gate and the add must each be the only reader of their input, and the shortcut must have the shape of the BN output'))
    pusers = _users(plan, plan_inputs)
    folded = _fold_into_gathers(plan, pusers, feature_name) if options.bn_gather else {}
    fuse_fwd, fuse_bwd = _bn_fusion(plan, pusers, feature_name) if options.bn_fuse else ({}, {})
    fold_apply = _fold_apply(plan, pusers, feature_name, fuse_fwd) if fuse_fwd and options.bn_fold else {}
    shortcut_fwd = _shortcut_branches(plan, pusers, feature_name) if options.shortcut_side else {}
    # tensors read by a BN AND by the activation-free shortcut of a later BN (the input of an IResNet identity block): the only
    # place where two gradient contributions are summed outside a conv's `addin` (_add); everywhere else a second one is a plan bug (_put)
    shortcut_shared = {op.res for op in plan if op[0] == 'bn' and op.res is not None and not op.relu} | \
        {op.shortcut for op in plan if op[0] == 'selin'}
    last = plan[-1]
    return Plan(plan, shapes, real_c, narrow, embed_in, folded, se_fused, fuse_fwd, fuse_bwd, fold_apply, shortcut_fwd, shortcut_shared,
                last[0] == 'fc' and spec[last.wname][1] == 'cls_w')


def segments(plan, variables, small_end, cls_start, has_classifier, want):
    """[(plan lo, plan hi, arena a, arena b)] in forward order: the body's plan split into `want` (FTE_GRAD_BUCKETS, default 4) runs
    of about equal filter bytes.  The filters lie in the arena in the order the plan uses them, so a run of ops owns a contiguous
    arena range; the first segment's range starts at 0 and so carries gamma / beta / biases of the whole net (0.1 - 0.4 MB: final
    early, reduced last, at no cost).  A net whose filters are not in plan order keeps ONE body segment."""
    nops = len(plan) - (1 if has_classifier else 0)
    one = [(0, nops, 0, cls_start)]
    offs = []                                        # (plan index, first arena offset, end offset) of every op with filters
    owned = set()
    for j in range(nops):
        names = op_weight_names(plan[j])
        if names:
            vs = [variables[w] for w in names]
            owned.update(names)
            offs.append((j, min(v.offset for v in vs), max(v.offset + v.size for v in vs)))
    mono = all(offs[i][2] <= offs[i + 1][1] for i in range(len(offs) - 1)) and (not offs or offs[0][1] >= small_end)
    # every variable of the body range that SOME plan op names must belong to an op seen above: a bucket's all-reduce is issued when
    # the ops of its plan range have been walked, so a variable of another kind of op (none today; e.g. a mid-plan fc) could land in a
    # bucket reduced before its gradient is final.  (Variables no op names -- ShuffleNet-v2-large's dead convs -- have no gradient.)
    named = {x for op in plan[:nops] for x in op if isinstance(x, str) and x in variables}
    stray = [k for k in named if small_end <= variables[k].offset < cls_start and k not in owned]
    if want <= 1 or not mono or stray or len(offs) < want:
        return one
    total = offs[-1][2] - offs[0][1]
    cuts, acc, k = [], 0, 1                          # cut BEFORE the op at which the running size passes k / want of the total
    for i, (j, a, b) in enumerate(offs):
        if k < want and i > 0 and acc >= total * k / want:
            cuts.append((j, a))
            k += 1
        acc += b - a
    segs, lo, a0 = [], 0, 0
    for j, a in cuts:
        segs.append((lo, j, a0, a))
        lo, a0 = j, a
    segs.append((lo, nops, a0, cls_start))
    return segs

