#!/usr/bin/env python
"""train.py -- the reference's training CLI (train.py:33-262) on the MI355X engine.

Same flags, defaults, assertions, LR schedules, log line and checkpoint cadence as the reference
(SURVEY.md Appendix D).  One process per GPU: `python train.py --num_gpus N ...` (the reference's invocation) starts its own N
ranks through torch.distributed.run; under torch.distributed.run it runs as one rank (WORLD_SIZE must equal --num_gpus).
Extra, not in the reference: --synthetic 1 trains on a resident random batch when no list is given,
--max_steps stops early (smoke runs)."""
import argparse
import math
import os
import sys
import time
from datetime import datetime

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    # Name configures
    parser.add_argument('--net_name', type=str, help='Name of the network architecture.')
    parser.add_argument('--model_name', type=str, help='Name of the training model.')
    # Directory configures
    parser.add_argument('--train_dir', type=str, default='train', help='Root directory where to write event logs.')
    parser.add_argument('--model_dir', type=str, default='models', help='Root directory where to save checkpoints.')
    parser.add_argument('--pretrained_path', type=str, default='', help='Path to save pretrained checkpoints.')
    # Data configure
    parser.add_argument('--data_format', type=str, default='NCHW', help='The format of data in the network (NCHW(default) or NHWC).')
    parser.add_argument('--train_list_path', type=str, help='Path to the list of training data.')
    parser.add_argument('--input_height', type=int, default=384, help='The height of input images.')
    parser.add_argument('--input_width', type=int, default=128, help='The width of input images.')
    parser.add_argument('--crop_height', type=int, default=-1, help='The height of input images.')
    parser.add_argument('--crop_width', type=int, default=-1, help='The width of input images.')
    parser.add_argument('--is_color', type=int, default=1, help='Whether to read inputs as RGB images.')
    parser.add_argument('--augmentation', type=int, default=0, help='Data augmentation of the training set: 0 = random flip only, 1 = flip + colour (brightness, hue, saturation), '
                        '2 = geometric (low-resolution zoom, one-pixel affine warp) + flip, 3 = geometric + colour.')
    # Hyperparameters configure
    parser.add_argument('--batch_size', type=int, default=-1, help='Number of sampled images in a batch.')
    parser.add_argument('--num_classes', type=int, default=-1, help='Number of sampled classesin a batch.')
    parser.add_argument('--num_per_class', type=int, default=-1, help='Number of sampled images per class in a batch.')
    parser.add_argument('--optimizer', type=str, default='Momentum', help='Type of optimizer.')
    parser.add_argument('--init_lr', type=float, default=0.1, help='Initial learning rate.')
    parser.add_argument('--lr_decay_method', type=str, default='step', help='Learning rate strategy (step/cosine/exp).')
    parser.add_argument('--lr_decay_rate', type=float, default=0.1, help='Learning rate decay rate.')
    parser.add_argument('--lr_decay_epoch', type=str, default='', help='Boundaries of decaying learning rate in step lr_decay')
    parser.add_argument('--max_epoches', type=int, help='Number of batches to run.')
    parser.add_argument('--weight_decay', type=float, default=5e-4, help='Factor for weight decaying.')
    # Device configures
    parser.add_argument('--num_gpus', type=int, default=4, help='Number of GPUs to use.')
    # Interval configures
    parser.add_argument('--display_interval', type=int, default=10, help='Internal iterations of verbose.')
    parser.add_argument('--save_interval', type=int, default=1000, help='Internal iterations of saving models.')
    # Not in the reference
    parser.add_argument('--synthetic', type=int, default=0, help='1: resident random batch instead of a list file.')
    parser.add_argument('--synthetic_classes', type=int, default=10575)
    parser.add_argument('--sync_centers', type=int, default=0,
                        help='center-loss nets under --num_gpus > 1.  0 (default) = the reference: every replica keeps and updates its own '
                             '`centers` table from its own shard (loss.py:34-39) and the tables drift apart; 1 = the replicas all-gather '
                             "each step's scatter rows and keep ONE table, equal to the single-tower update of the global batch.")
    parser.add_argument('--max_steps', type=int, default=-1, help='Stop after this many steps (smoke runs).')
    parser.add_argument('--mfma_dtype', type=str, default='f32',
                        help='f32 (the reference arithmetic), bf16 (bf16 MFMA operands, fp32 accumulate and storage) or bf16s (bf16 operands and bf16 '
                             'storage of activations / inter-layer gradients; fp32 accumulate, sums and master weights: SphereNet).')
    for flag, what in (('--margin_scale', 'scale S'), ('--margin', 'angular margin m (ArcFace, CurricularFace; AdaFace: the margin m its per-image margins scale; MagFace: refused, see --magface)'),
                       ('--margin_cos', 'cosine margin m3 (CosFace; not an AdaFace, CurricularFace or MagFace parameter)')):
        parser.add_argument(flag, type=float, default=None,
                            help='additive-margin nets (SphereNet-ArcFace / -CosFace / -AdaFace / -CurricularFace, ResNet-50-arcface / -cosface / -adaface / -curricularface) only: the %s; '
                                 "default: the net's preset (ArcFace S = 64, m = 0.5, m3 = 0; CosFace S = 64, m = 0, m3 = 0.35; AdaFace S = 64, m = 0.4; CurricularFace S = 64, m = 0.5; MagFace S = 64)" % what)
    parser.add_argument('--magface', type=str, default=None,
                        help='MagFace nets (SphereNet-MagFace, ResNet-50-magface, [SE-]IResNet-*-magface) only: l_a,u_a,l_m,u_m,lambda_g -- the norm '
                             "range, the margin range and the regulariser's weight; default 10,110,0.45,0.8,35 (the paper's MS1M-V2 values). "
                             '--margin_scale sets S.')
    parser.add_argument('--sample_rate', type=float, default=1.0,
                        help='SphereNet-ArcFace / SphereNet-CosFace (one GPU; --num_gpus > 1 with --sync_sample 1): the fraction of the classes the margin head runs over per '
                             "step (Partial FC: the batch's own classes plus a seeded random sample of the others; 0.1 is the usual value). "
                             'A float in (0, 1]; 1 (default) = the dense head.')
    parser.add_argument('--sample_seed', type=int, default=0, help='seed of the per-step class sample of --sample_rate.')
    parser.add_argument('--sync_sample', type=int, default=0,
                        help='--sample_rate < 1 under --num_gpus > 1 (refused without it): 1 = the ranks all-gather their labels and draw ONE '
                             'class sample per step from the global batch; the compact gradient of the sampled classifier columns is '
                             'all-reduced instead of the dense one.  Implies --compact_head_update 1.')
    parser.add_argument('--compact_head_update', type=int, default=0,
                        help='--sample_rate < 1: 1 = the classifier and its optimizer slots are updated straight from the compact gradient '
                             'of the sampled columns (one fused kernel, the same values bit for bit); the dense classifier gradient is '
                             'never written.')
    parser.add_argument('--sub_centers', type=int, default=1,
                        help='SphereNet-ArcFace / -CosFace, ResNet-50-arcface / -cosface: K centres per class (sub-center ArcFace), 1..8; the class '
                             'logit is the max cosine over its centres.  1 (default) = one centre, the head as it always was.  Not with '
                             '--sample_rate < 1.  subcenter_clean.py reduces a trained K-centre model to K = 1 and cleans the list.')
    parser.add_argument('--landmark_list_path', type=str, default=None,
                        help='`path x1 y1 x2 y2 x3 y3 x4 y4 x5 y5` per line (source pixels of left eye, right eye, nose, left and right mouth '
                             'corner) for every image of --train_list_path: the images are five-point aligned to --input_height x --input_width '
                             '(the ArcFace template, scaled by height / 112 and centred) in place of the resize.  --augmentation 0 or 1.')
    parser.add_argument('--shard_classes', type=int, default=0,
                        help='SphereNet-ArcFace / SphereNet-CosFace under --num_gpus > 1: 1 = the classifier is split by class over the ranks '
                             '(model-parallel head): rank r holds C / num_gpus columns with their optimizer slots, the features of the global '
                             'batch are all-gathered, the classifier gradient is never all-reduced and the checkpoints stay dense.  Not with '
                             '--sample_rate < 1, --sync_sample 1 or --sub_centers > 1.  0 (default) = every rank holds the whole classifier.')
    parser.add_argument('--packed_data_path', type=str, default=None,
                        help='An image pack made by pack_list.py, in place of --train_list_path: the images were decoded once, the loader '
                             'reads uint8 rows (same batches as the list the pack was made from, bit for bit).  Not with --train_list_path, '
                             '--synthetic 1 or --landmark_list_path (a pack is aligned when it is made); the pack must carry labels.')
    parser.add_argument('--pack_on_gpu', type=int, default=0,
                        help='--packed_data_path: 1 = the whole pack is uploaded once and stays in device memory (every rank holds it); the '
                             'host then only draws.  0 (default) = the workers copy rows out of the memory-mapped file.')
    return parser


SAMPLED_NETS = ('SphereNet-ArcFace', 'SphereNet-CosFace')


def shard_flags_check(FLAGS):
    """--shard_classes: refuse what the sharded classifier does not do, before anything is built or communicated"""
    if not getattr(FLAGS, 'shard_classes', 0):
        return
    if FLAGS.num_gpus < 2:
        raise SystemExit('--shard_classes 1 splits the classifier over the ranks: it needs --num_gpus > 1 (got %d)' % FLAGS.num_gpus)
    if FLAGS.net_name not in SAMPLED_NETS:
        raise SystemExit('--shard_classes 1: only %s have a sharded classifier, not %s' % (' / '.join(SAMPLED_NETS), FLAGS.net_name))
    from tf_face_toolbox_amd import heads
    try:
        heads.check_sharding('arcface', FLAGS.sample_rate, bool(FLAGS.sync_sample), FLAGS.sub_centers, FLAGS.net_name)
        if FLAGS.synthetic:                               # (a list's class count is known once it is read: the wrapper refuses there)
            heads.shard_range(FLAGS.synthetic_classes, FLAGS.num_gpus, 0)
    except ValueError as e:
        raise SystemExit('--shard_classes 1: %s' % e)


def landmark_flags_check(FLAGS):
    """--landmark_list_path: refuse what the aligned transform does not do, before anything is built"""
    if getattr(FLAGS, 'landmark_list_path', None) is None:
        return
    if FLAGS.augmentation & 2:
        raise SystemExit('--landmark_list_path: the geometric augmentation (--augmentation 2 | 3) is not available together with '
                         'landmarks; use --augmentation 0 or 1 (got %d)' % FLAGS.augmentation)
    if FLAGS.synthetic:
        raise SystemExit('--landmark_list_path: --synthetic 1 reads no images')


def pack_flags_check(FLAGS, list_flag='train_list_path'):
    """--packed_data_path / --pack_on_gpu: refuse the combinations a pack does not serve, before anything is built (evaluate.py
    checks its flags here too, with list_flag='data_list_path')"""
    packed = getattr(FLAGS, 'packed_data_path', None)
    if packed is None:
        if getattr(FLAGS, 'pack_on_gpu', 0):
            raise SystemExit('--pack_on_gpu 1 needs --packed_data_path')
        return
    if getattr(FLAGS, list_flag, None) is not None:
        raise SystemExit('--packed_data_path replaces --%s: give one of them, not both' % list_flag)
    if getattr(FLAGS, 'synthetic', 0):
        raise SystemExit('--packed_data_path: --synthetic 1 reads no images')
    if getattr(FLAGS, 'landmark_list_path', None) is not None:
        raise SystemExit('--packed_data_path together with --landmark_list_path: a pack is aligned when it is made '
                         '(pack_list.py --landmark_list_path)')
    if list_flag == 'train_list_path':
        from tf_face_toolbox_amd.packs import ImagePack
        try:
            pack = ImagePack(packed)
        except (OSError, ValueError) as e:
            raise SystemExit('--packed_data_path: %s' % e)
        if not pack.has_labels:
            raise SystemExit('--packed_data_path: %s has no labels (it was made from a list of paths only): training needs them' % packed)


def sample_flags_check(FLAGS):
    """--sample_rate / --sample_seed: refuse what the sampled-class head does not do, before anything is built"""
    if not 0.0 < FLAGS.sample_rate <= 1.0:
        raise SystemExit('--sample_rate must lie in (0, 1]: got %g' % FLAGS.sample_rate)
    if FLAGS.sample_rate < 1.0 and FLAGS.net_name not in SAMPLED_NETS:
        raise SystemExit('--sample_rate %g: only %s have a sampled-class head, not %s'
                         % (FLAGS.sample_rate, ' / '.join(SAMPLED_NETS), FLAGS.net_name))
    if FLAGS.sample_rate < 1.0 and FLAGS.num_gpus > 1 and not getattr(FLAGS, 'sync_sample', 0):
        raise SystemExit('--sample_rate %g: the sampled-class head runs on one GPU only (--num_gpus %d)' % (FLAGS.sample_rate, FLAGS.num_gpus))


def sub_centers_flags_check(FLAGS):
    """--sub_centers: refuse what the K-centre head does not do, before anything is built"""
    from tf_face_toolbox_amd.nets.net_base import sub_centers_check
    try:
        sub_centers_check(FLAGS.net_name, FLAGS.sub_centers, FLAGS.sample_rate)
    except ValueError as e:
        raise SystemExit('--sub_centers %d: %s' % (FLAGS.sub_centers, e))


def is_magface_net(name):
    return name == 'SphereNet-MagFace' or name.endswith('-magface')


def magface_notice(scale, l_a, u_a, l_m, u_m, lambda_g):
    """the line train.py prints once when lambda_g is below the paper's bound for a unique optimum in the norm, else None"""
    from tf_face_toolbox_amd.nets.net_base import magface_lambda_bound
    bound = magface_lambda_bound(scale, l_a, u_a, l_m, u_m)
    if lambda_g < bound:
        return ('MagFace: lambda_g = %g is below S k_m u_a^2 l_a^2 / (u_a^2 - l_a^2) = %.4g: the loss has no unique optimum in the '
                'feature norm (Meng et al. 2021, the condition of their Property 2)' % (lambda_g, bound))
    return None


def magface_flags_check(FLAGS):
    """--magface and the margin flags of a MagFace net: refuse what does not belong, before anything is built.  Leaves the five
    numbers (or None) in FLAGS.magface_values."""
    FLAGS.magface_values = None
    magnet = is_magface_net(FLAGS.net_name)
    if FLAGS.magface is not None and not magnet:
        raise SystemExit('--magface: only the MagFace nets (SphereNet-MagFace, ResNet-50-magface, [SE-]IResNet-*-magface) take it, not %s'
                         % FLAGS.net_name)
    if not magnet:
        return
    for flag in ('margin', 'margin_cos'):
        if getattr(FLAGS, flag) is not None:
            raise SystemExit('--%s: %s has no such parameter; its margin range is set by --magface l_a,u_a,l_m,u_m,lambda_g'
                             % (flag, FLAGS.net_name))
    from tf_face_toolbox_amd.nets.net_base import MAGFACE_PRESET, magface_params
    vals = MAGFACE_PRESET[1:]
    if FLAGS.magface is not None:
        try:
            vals = tuple(float(v) for v in FLAGS.magface.split(','))
        except ValueError:
            vals = ()
        if len(vals) != 5:
            raise SystemExit('--magface takes five numbers l_a,u_a,l_m,u_m,lambda_g: got %r' % FLAGS.magface)
    try:
        FLAGS.magface_values = magface_params(FLAGS.margin_scale, *vals)[1:]
    except ValueError as e:
        raise SystemExit('--magface: %s' % e)


def FLAGS_assertion(FLAGS):
    """train.py:95-99."""
    assert FLAGS.data_format in ['NCHW', 'NHWC'], 'Unknown data format.'
    assert FLAGS.batch_size != -1 or (FLAGS.num_classes != -1 and FLAGS.num_per_class != -1)
    assert (FLAGS.num_classes != -1 and FLAGS.num_per_class != -1 and (FLAGS.num_classes * FLAGS.num_per_class) % FLAGS.num_gpus == 0) \
        or (FLAGS.batch_size % FLAGS.num_gpus == 0 and FLAGS.batch_size != -1)
    assert FLAGS.optimizer in ['Momentum', 'Adam'], 'Unsupported optimizer.'


def lr_config(FLAGS, method, batches_per_epoch):
    """train.py:122-144 as a function of the global step (tf.train.piecewise_constant /
    exponential_decay / cosine_decay semantics)."""
    if method == 'step':
        if FLAGS.lr_decay_epoch == '':
            raise ValueError('Empty learning rate decay epoch boundaries.')
        decay_boundary = [(int(epoch) - 1) * batches_per_epoch for epoch in FLAGS.lr_decay_epoch.split(',')]
        decay_value = [FLAGS.init_lr] + [FLAGS.init_lr * FLAGS.lr_decay_rate ** (p + 1) for p in range(len(decay_boundary))]

        def lr(step):       # value[i] for boundary[i-1] < step <= boundary[i]
            k = 0
            while k < len(decay_boundary) and step > decay_boundary[k]:
                k += 1
            return decay_value[k]
    elif method == 'exp':
        decay_step = int(FLAGS.lr_decay_epoch) * batches_per_epoch
        decay_steps = int(FLAGS.max_epoches) * batches_per_epoch + 1 - decay_step

        def lr(step):
            if step < decay_step:
                return FLAGS.init_lr
            return FLAGS.init_lr * 0.001 ** ((step - decay_step) / float(decay_steps))
    elif method == 'cosine':
        total = FLAGS.max_epoches * batches_per_epoch

        def lr(step):
            return FLAGS.init_lr * 0.5 * (1 + math.cos(math.pi * min(step, total) / total))
    else:
        raise ValueError('Unsupported learning rate decaying method.')
    return lr


def format_str(losses_name):
    """train.py:146-152, verbatim."""
    outputs = '[%s] Epoch/Step %d/%d, lr = %g\n'
    for loss_id, loss_name in enumerate(losses_name):
        outputs += '[%s]    Loss #' + str(loss_id) + ': ' + loss_name + ' = %.6f\n'
    outputs += '[%s]    batch_time = %.1fms/batch, throughput = %.1fimages/s'
    return outputs


def train(FLAGS):
    import torch
    import torch.distributed as dist
    from tf_face_toolbox_amd import net_select, Singular, DataParallel_margin, saver
    from tf_face_toolbox_amd.data import train_inputs, synthetic_inputs

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if FLAGS.num_gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python train.py --num_gpus N` as the reference is invoked: this process starts the N ranks as fresh children (it has not
        # touched the GPU and never will), passes their output through and exits with their status
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(FLAGS.num_gpus),
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        env.setdefault('OMP_NUM_THREADS', '8')
        raise SystemExit(subprocess.run(cmd, env=env).returncode)
    if FLAGS.num_gpus != world:
        raise SystemExit('--num_gpus %d but WORLD_SIZE is %d: one process per GPU (python -m torch.distributed.run --nproc-per-node %d '
                         '--master-addr 127.0.0.1 train.py ..., or plain `python train.py --num_gpus %d`, which launches them)'
                         % (FLAGS.num_gpus, world, FLAGS.num_gpus, FLAGS.num_gpus))
    # FTE_BENCH_SHARED_GPU=1 (tests only, as in bench.py): all ranks on the GPUs that exist, gloo as the transport -- RCCL refuses two
    # ranks on one device and the test boxes have one GPU; everything else of the N > 1 path is what a multi-GPU node runs
    shared = os.environ.get('FTE_BENCH_SHARED_GPU') == '1'
    if shared:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if shared:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=device)
    from tf_face_toolbox_amd import _lib
    _lib.set_mfma_dtype(FLAGS.mfma_dtype)

    batch_size = FLAGS.batch_size if FLAGS.batch_size != -1 else FLAGS.num_classes * FLAGS.num_per_class
    # Data I/O (train.py:161-170)
    if FLAGS.synthetic:
        h = FLAGS.crop_height if FLAGS.crop_height != -1 else FLAGS.input_height
        w = FLAGS.crop_width if FLAGS.crop_width != -1 else FLAGS.input_width
        inputs = synthetic_inputs(batch_size, h, w, FLAGS.is_color, FLAGS.synthetic_classes, device, rank, world)
    else:
        inputs = train_inputs(FLAGS.train_list_path, input_height=FLAGS.input_height, input_width=FLAGS.input_width,
                              crop_height=FLAGS.crop_height, crop_width=FLAGS.crop_width, is_color=FLAGS.is_color,
                              augmentation=FLAGS.augmentation, batch_size=FLAGS.batch_size, num_classes=FLAGS.num_classes,
                              num_per_class=FLAGS.num_per_class, device=device, seed=1234, rank=rank, world_size=world,
                              landmark_list_path=getattr(FLAGS, 'landmark_list_path', None),
                              packed_data_path=getattr(FLAGS, 'packed_data_path', None), pack_on_gpu=bool(getattr(FLAGS, 'pack_on_gpu', 0)))
        if inputs['packed'] is not None and rank == 0:
            print('image pack %s, %s' % (inputs['pack'], {'host': 'rows read from the host mapping', 'gpu': 'resident in device memory'}[inputs['packed']]))
    try:
        batches_per_epoch = inputs['num_examples'] // batch_size + 1                                  # train.py:172
        network = net_select(FLAGS.net_name, FLAGS.data_format, FLAGS.weight_decay, sub_centers=FLAGS.sub_centers)      # train.py:174
        margins = (FLAGS.margin_scale, FLAGS.margin, FLAGS.margin_cos)
        if getattr(network, 'margin_scale', None) is not None and margins != (None, None, None):
            network.set_margin(*margins)
        if getattr(FLAGS, 'magface_values', None) is not None:
            network.set_magface(*FLAGS.magface_values)
            notice = magface_notice(network.margin_scale, *network.magface)
            if notice and rank == 0:
                print(notice)
        if FLAGS.sample_rate < 1.0:
            network.set_sample_rate(FLAGS.sample_rate, FLAGS.sample_seed)
        lr = lr_config(FLAGS, FLAGS.lr_decay_method, batches_per_epoch)                              # train.py:176
        if FLAGS.num_gpus > 1:                                                                        # train.py:178-183
            model = DataParallel_margin(network, lr, optimizer=FLAGS.optimizer, weight_decay=FLAGS.weight_decay, num_gpus=FLAGS.num_gpus,
                                        sync_centers=bool(FLAGS.sync_centers), sync_sample=bool(FLAGS.sync_sample),
                                        shard_classes=bool(FLAGS.shard_classes))
        else:
            model = Singular(network, lr, optimizer=FLAGS.optimizer, weight_decay=FLAGS.weight_decay)
        compact = FLAGS.sample_rate < 1.0 and bool(FLAGS.compact_head_update or (FLAGS.sync_sample and FLAGS.num_gpus > 1))
        if compact:
            network.compact_head_update = True
        train_ops, losses, losses_name, others = model(inputs)
        if FLAGS.sample_rate < 1.0:
            print('Sampled-class head: sample_rate = %g, sample_seed = %d, S = %d of %d classes per step'
                  % (FLAGS.sample_rate, FLAGS.sample_seed, network.sample_size, network.num_classes))
            if compact:
                print('Sampled-class head mode: %s, compact classifier update (no dense classifier gradient)'
                      % ('one shared sample over %d ranks' % FLAGS.num_gpus if FLAGS.num_gpus > 1 else 'one GPU'))

        if FLAGS.shard_classes:
            per_rank = (network.num_classes + world - 1) // world
            print('classifier: %d shards of %s classes (%s in all; rank %d holds classes %d..%d)'
                  % (world, format(per_rank, ','), format(network.num_classes, ','), rank, network.shard[0], network.shard[1] - 1))

        tag = FLAGS.net_name + '_' + FLAGS.model_name
        ckpt_dir = os.path.join(FLAGS.model_dir, tag)
        latest = saver.latest_checkpoint(ckpt_dir)                                                    # train.py:207-215
        if latest:
            model.global_step = saver.restore(network, latest, optimizer=model._opt)
            print('Model restored from %s' % ckpt_dir)
        elif FLAGS.pretrained_path != '':
            saver.restore(network, FLAGS.pretrained_path, only=model.pretrained_param)
            print('Network parameters initialized from %s' % FLAGS.pretrained_path)
        else:
            print('Network parameters initialized from scratch.')
        if world > 1:
            model.comm.broadcast(model.replicated_params(), src=0)      # (a sharded classifier: every rank read its own columns)

        print('%s training start...' % tag)
        step, epoch = 0, 1
        time_sim, image_sim = 0.0, 0.0
        first_step, settled = None, None                          # (step, wall clock) 20 steps after the start: the sustained rate printed at the end
        while epoch <= FLAGS.max_epoches:                                                             # train.py:223-250
            step = model.global_step
            epoch = step // batches_per_epoch + 1
            start_time = time.time()
            first_step = step if first_step is None else first_step
            if settled is None and step - first_step >= 20:
                settled = (step, start_time)
            train_ops()
            losses_value = [float(l) for l in losses]            # reading the losses synchronises, like sess.run
            last_done = time.time()
            duration = last_done - start_time
            if not all(math.isfinite(v) for v in losses_value):
                raise SystemExit('Model diverged with losses = %s' % losses_value)
            if step % FLAGS.display_interval == 0 and rank == 0:
                format_list = [datetime.now(), epoch, step, model.learning_rate]
                for loss_value in losses_value:
                    format_list.extend([datetime.now(), loss_value])
                format_list.extend([datetime.now(), duration * 1000, batch_size / duration])
                print(format_str(losses_name) % tuple(format_list))
                for other_name, other_value in others.items():
                    print('%s: %s' % (other_name, other_value))
            if step > 0:
                time_sim += duration
                image_sim += batch_size / duration
            last = step == FLAGS.max_epoches * batches_per_epoch or (FLAGS.max_steps > 0 and step + 1 >= FLAGS.max_steps)
            # a sharded classifier is saved dense: putting it together is a collective, so EVERY rank enters save() at a save step (the
            # condition depends on the step alone) and rank 0 writes the file
            if ((step > 0 and step % FLAGS.save_interval == 0) or last) and (rank == 0 or FLAGS.shard_classes):
                path = saver.save(network, model._opt.slots, model.global_step, os.path.join(ckpt_dir, tag + '.ckpt'), write=rank == 0)
                if rank == 0:
                    print('[%s]: Model has been saved in Iteration %d (%s)' % (datetime.now(), step, path))
            if FLAGS.max_steps > 0 and step + 1 >= FLAGS.max_steps:
                break
        if rank == 0 and step > 0:
            print('mean batch_time=%.2f, mean throughput=%.2f' % (time_sim / step * 1000, image_sim / step))
            if settled is not None and step + 1 > settled[0]:      # not in the reference: images / wall clock once the pipeline has settled
                print('sustained throughput=%.2f images/s over steps %d..%d' % ((step + 1 - settled[0]) * batch_size / (last_done - settled[1]), settled[0], step))
        if world > 1:
            dist.barrier()
    finally:
        # orderly shutdown, whatever happened above: stop the input pipeline's producer thread and wait for it, end the decode
        # workers and release their shared buffers, drain the device, leave the process group
        close = inputs.get('close')
        try:
            if close is not None and not close():
                print('train.py: the input pipeline did not shut down cleanly', file=sys.stderr)
                FLAGS._shutdown_failed = True
        except Exception as e:                 # never raise from here: the error that brought us here (if any) must stay the one reported
            print('train.py: closing the input pipeline failed: %s' % e, file=sys.stderr)
            FLAGS._shutdown_failed = True
        try:
            torch.cuda.synchronize()
        except Exception as e:                 # a device fault is what brought us here: report it, keep the original error
            print('train.py: device synchronise failed during shutdown: %s' % e, file=sys.stderr)
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def main(argv=None):
    FLAGS = build_parser().parse_args(argv)
    FLAGS_assertion(FLAGS)
    shard_flags_check(FLAGS)
    sample_flags_check(FLAGS)
    sub_centers_flags_check(FLAGS)
    magface_flags_check(FLAGS)
    landmark_flags_check(FLAGS)
    pack_flags_check(FLAGS)
    os.makedirs(os.path.join(FLAGS.train_dir, FLAGS.net_name + '_' + FLAGS.model_name), exist_ok=True)
    os.makedirs(os.path.join(FLAGS.model_dir, FLAGS.net_name + '_' + FLAGS.model_name), exist_ok=True)
    train(FLAGS)
    return FLAGS


def _run_and_leave(fn):
    """Runs the program and leaves with ITS status.  By the time fn() returns or raises, everything this program started has been
    shut down in order (train()'s finally block: producer thread joined, decode workers reaped, device drained, process group
    destroyed), so nothing of ours can still fail.  What remains is interpreter / HIP runtime teardown, where ROCm 7 occasionally
    ends a finished process with std::terminate (exit code -6: torch's helper threads race the runtime's static destructors).
    Only when the GPU runtime was initialised, os._exit skips that teardown -- with the real status (a failure stays a failure;
    round 2 left with an unconditional 0)."""
    import traceback
    status = 0
    try:
        status = 1 if getattr(fn(), '_shutdown_failed', False) else 0
    except SystemExit as e:
        if e.code is None or e.code == 0:
            status = 0
        elif isinstance(e.code, int):
            status = e.code
        else:
            print(e.code, file=sys.stderr)
            status = 1
    except BaseException:                      # noqa: B902
        traceback.print_exc()
        status = 1
    sys.stdout.flush()
    sys.stderr.flush()
    gpu_up = False
    try:
        import torch
        gpu_up = torch.cuda.is_initialized()
    except Exception:
        pass
    if gpu_up:
        os._exit(status)
    sys.exit(status)


if __name__ == '__main__':
    _run_and_leave(main)
