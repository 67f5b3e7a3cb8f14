"""Worker of tests/test_gpu_sharded_head_dp.py and tests/test_sharded_head_host.py, modelled on tests/pfc_dp_worker.py.

    shard_dp_worker.py steps FIX OUT NAME STEPS    one rank of a DataParallel_margin(shard_classes=True) run
    shard_dp_worker.py loss FIX OUT NAME 0         one rank of loss.sharded_margin_loss on a head-only problem
    shard_dp_worker.py rs FIX OUT - 0              _HostComm.reduce_scatter_sum over gloo on CPU tensors (no GPU is touched)

FIX (npz) carries x, y, ncls, the parameters 'p:<name>', opt, lr, save_at (steps after which every rank enters saver.save; -1:
never), ckpt (the checkpoint prefix) and restore (a checkpoint to start from; '': the fixture's parameters).
With a GPU per rank: device = LOCAL_RANK, backend 'nccl' (= RCCL); on a one-GPU box all ranks share device 0 over gloo
(FTE_TEST_FORCE_GLOO=1 keeps gloo on a multi-GPU box).  The result file records which ran."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLS = 'classifier/fc_classifier/weights'


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


class Recording(object):
    """the wrappers' collective layer with a log: (kind, elements, touches the classifier's gradient range)"""

    def __init__(self, inner):
        self.inner, self.log, self.net = inner, [], None

    def _note(self, kind, t):
        hit = False
        if self.net is not None and getattr(self.net, 'grads', None) is not None:
            g = self.net.grads
            lo, hi = g.data_ptr() + 4 * self.net.cls_start, g.data_ptr() + 4 * self.net.arena_size
            hit = t.data_ptr() < hi and t.data_ptr() + 4 * t.numel() > lo
        self.log.append('%s:%d:%d' % (kind, t.numel(), int(hit)))

    def world_size(self):
        return self.inner.world_size()

    def rank(self):
        return self.inner.rank()

    def all_reduce_async(self, t):
        self._note('all_reduce', t)
        return self.inner.all_reduce_async(t)

    def broadcast(self, t, src=0):
        self._note('broadcast', t)
        self.inner.broadcast(t, src)

    def all_gather(self, out, t):
        self._note('all_gather', out)
        self.inner.all_gather(out, t)

    def reduce_scatter_sum(self, out, inp):
        self._note('reduce_scatter', inp)
        self.inner.reduce_scatter_sum(out, inp)


def steps(d, out, name, nsteps, rank, world, res):
    from tf_face_toolbox_amd import net_select, DataParallel_margin, saver
    from tf_face_toolbox_amd.data_parallel import _HostComm
    x, y = d['x'], d['y']
    n, ncls = x.shape[0], int(d['ncls'])
    sh = n // world
    xs = torch.tensor(x[rank * sh:(rank + 1) * sh], dtype=torch.float32, device='cuda')
    ys = torch.tensor(y[rank * sh:(rank + 1) * sh], dtype=torch.int32, device='cuda')
    net = net_select(name, 'NCHW', 5e-4)
    net.seed = 100 + rank                                   # the ranks start DIFFERENT
    comm = Recording(_HostComm())
    comm.net = net
    model = DataParallel_margin(net, float(d['lr']), str(d['opt']), num_gpus=world, comm=comm, shard_classes=True)
    inputs = {'images': xs, 'labels': ys, 'num_classes': ncls, 'num_examples': n, 'batch_size': n}
    step, losses, names, _ = model(inputs)
    torch.cuda.synchronize()
    lo, hi = net.shard
    ld = net.shard_cols
    res['range'] = np.array([lo, hi, ld, net.arena_size, net.cls_start])
    res['setup_calls'] = np.array(comm.log)
    # after the construction pass: the backbone is rank 0's, the shard is the rank's own columns of ITS dense initial value
    res['init_backbone_sha'] = np.array(sha(net.params[:net.cls_start]))
    res['init_shard'] = net.view(CLS).reshape(512, ld).cpu().numpy()
    dense = net_select(name, 'NCHW', 5e-4)
    dense.seed = 100 + rank
    dense.build(x.shape[1], x.shape[2], x.shape[3], ncls, 'cuda')
    res['init_dense_cols'] = dense.get_variable(CLS)[:, lo:hi].cpu().numpy()
    res['init_dense_backbone_sha'] = np.array(sha(dense.params[:dense.cls_start]))
    del dense
    if str(d['restore']):
        model.global_step = saver.restore(net, str(d['restore']), optimizer=model._opt)
    else:
        net.load_params({k[2:]: d[k] for k in d.files if k.startswith('p:')})      # every rank keeps its own classifier columns
    hist, shas, calls = [], [], []
    for t in range(nsteps):
        del comm.log[:]
        step()
        torch.cuda.synchronize()
        calls.append('|'.join(comm.log))
        hist.append([float(v) for v in losses])
        shas.append(sha(net.params[:net.cls_start]))           # the backbone bytes, after every step
        for i, c in enumerate(net.convs):                      # this shard's pre-activations: the oracle's kink side
            res['z:%d:%s' % (t, c.name)] = net.z[i].cpu().numpy()
        if t + 1 == int(d['save_at']):
            del comm.log[:]
            saver.save(net, model._opt.slots, model.global_step, str(d['ckpt']), write=rank == 0)
            res['save_calls'] = np.array(comm.log)
            res['saved_shard'] = net.view(CLS).reshape(512, ld).cpu().numpy()
            res['saved_slot_shard'] = net.view(CLS, model._opt.slots[0]).reshape(512, ld).cpu().numpy()
    for k in net.variables:                                    # (the classifier: dense, a collective every rank enters)
        res['w:' + k] = net.get_variable(k).cpu().numpy()
    res['shard'] = net.view(CLS).reshape(512, ld).cpu().numpy()
    res['slot_shard'] = net.view(CLS, model._opt.slots[0]).reshape(512, ld).cpu().numpy()
    res['logits_shape'] = np.array(net.logits_buf[:, :hi - lo].shape)
    res['arena_sha'] = np.array(sha(net.params))
    res['slots_sha'] = np.array([sha(s) for s in model._opt.slots])
    res['losses'] = np.array(hist)
    res['backbone_sha'] = np.array(shas)
    res['calls'] = np.array(calls)
    res['global_step'] = np.array(model.global_step)


def loss(d, out, rank, world, res):
    """sharded_margin_loss on features x [N, D], the dense classifier w [D, C] and labels y: this rank's rows and columns"""
    from tf_face_toolbox_amd import heads
    from tf_face_toolbox_amd.data_parallel import _HostComm
    from tf_face_toolbox_amd.loss import sharded_margin_loss
    x, w, y, C = d['x'], d['w'], d['y'], int(d['ncls'])
    n = x.shape[0] // world
    lo, hi = heads.shard_range(C, world, rank)
    ld = heads.shard_ld(C, world)
    ws = np.zeros((x.shape[1], ld), np.float32)
    ws[:, :hi - lo] = w[:, lo:hi]
    dev = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device='cuda')
    l, dx, dw = sharded_margin_loss(dev(x[rank * n:(rank + 1) * n]), dev(ws), dev(y[rank * n:(rank + 1) * n], torch.int32), lo, C,
                                    _HostComm(), *[float(v) for v in d['preset']])
    torch.cuda.synchronize()
    res.update(loss=np.array(float(l)), dx=dx.cpu().numpy(), dw=dw.cpu().numpy(), range=np.array([lo, hi, ld]))


def reduce_scatter_cpu(out):
    """gloo, CPU tensors: reduce_scatter_sum against the sum the test computes by hand"""
    import torch.distributed as dist
    from tf_face_toolbox_amd.data_parallel import _HostComm
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    rows, d = 3, 5
    inp = torch.arange(world * rows * d, dtype=torch.float32).reshape(world * rows, d) * (rank + 1) + rank
    got = torch.full((rows, d), -1.0)
    _HostComm().reduce_scatter_sum(got, inp.clone())
    np.savez(out + '.rank%d.npz' % rank, got=got.numpy(), inp=inp.numpy(), backend=np.array(dist.get_backend()))
    dist.barrier()
    dist.destroy_process_group()


def main():
    mode, fix, out, name, nsteps = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
    if mode == 'rs':
        return reduce_scatter_cpu(out)
    import torch.distributed as dist
    d = np.load(fix)
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    local = int(os.environ.get('LOCAL_RANK', rank))
    rccl = torch.cuda.device_count() >= world and os.environ.get('FTE_TEST_FORCE_GLOO') != '1'
    if rccl:
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        torch.cuda.set_device(0)
        dist.init_process_group('gloo')
    res = {'backend': np.array('nccl' if rccl else 'gloo'), 'device': np.array(torch.cuda.current_device())}
    if mode == 'steps':
        steps(d, out, name, nsteps, rank, world, res)
    else:
        loss(d, out, rank, world, res)
    np.savez(out + '.rank%d.npz' % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
    sys.stdout.flush()
    if sys.argv[1] != 'rs':
        os._exit(0)
