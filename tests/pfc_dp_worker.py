"""Worker of tests/test_gpu_partial_fc_dp.py, modelled on tests/dp_worker.py.

    pfc_dp_worker.py dp FIX OUT NAME STEPS       one rank of a DataParallel_margin(sync_sample=True) run of a net with a sample rate
    pfc_dp_worker.py refuse FIX OUT NAME 0       the same construction with a sample smaller than the global batch: writes the error
    pfc_dp_worker.py single FIX OUT NAME STEPS   one process, Singular with compact_head_update (run under a kernel tracer)

With a GPU per rank: device = LOCAL_RANK, backend 'nccl' (= RCCL); on a one-GPU box all ranks share device 0 over gloo
(FTE_TEST_FORCE_GLOO=1 keeps gloo on a multi-GPU box).  The result file records which ran."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_face_toolbox_amd import net_select, DataParallel_margin, Singular   # noqa: E402


def _net(name, d, seed, rate):
    n, h, w, ch = d['x'].shape
    net = net_select(name, 'NCHW', 5e-4)
    net.seed = seed
    net.build(h, w, ch, int(d['ncls']), 'cuda')
    net.set_sample_rate(rate, int(d['sample_seed']))
    return net


def single(d, out, name, steps):
    net = _net(name, d, 7, float(d['rate']))
    net.compact_head_update = True
    xs = torch.tensor(d['x'], dtype=torch.float32, device='cuda')
    ys = torch.tensor(d['y'], dtype=torch.int32, device='cuda')
    step, losses, _, _ = Singular(net, 0.05, 'Momentum')({'images': xs, 'labels': ys, 'num_classes': int(d['ncls']), 'num_examples': len(ys)})
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    np.savez(out + '.single.npz', loss=float(losses[0]))


def main():
    mode, fix, out, name, steps = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
    d = np.load(fix)
    if mode == 'single':
        torch.cuda.set_device(0)
        return single(d, out, name, steps)
    import torch.distributed as dist
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    local = int(os.environ.get('LOCAL_RANK', rank))
    rccl = torch.cuda.device_count() >= world and os.environ.get('FTE_TEST_FORCE_GLOO') != '1'
    if rccl:
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        torch.cuda.set_device(0)
        dist.init_process_group('gloo')
    x, y = d['x'], d['y']
    n, ncls = x.shape[0], int(d['ncls'])
    sh = n // world
    xs = torch.tensor(x[rank * sh:(rank + 1) * sh], dtype=torch.float32, device='cuda')
    ys = torch.tensor(y[rank * sh:(rank + 1) * sh], dtype=torch.int32, device='cuda')
    net = _net(name, d, 100 + rank, float(d['rate']))       # replicas start DIFFERENT: the wrapper's broadcast must make them equal
    if rank == 0:
        net.load_params({k[2:]: d[k] for k in d.files if k.startswith('p:')})
    model = DataParallel_margin(net, 0.05, 'Momentum', num_gpus=world, sync_sample=True)
    inputs = {'images': xs, 'labels': ys, 'num_classes': ncls, 'num_examples': n, 'batch_size': n}
    res = {'backend': np.array('nccl' if rccl else 'gloo'), 'device': np.array(torch.cuda.current_device())}
    if mode == 'refuse':
        try:
            model(inputs)
            res['error'] = np.array('')
        except ValueError as e:
            res['error'] = np.array(str(e))
    else:
        step, losses, names, _ = model(inputs)
        hist, shas = [], []
        S = net.sample_size
        for t in range(steps):
            step()
            torch.cuda.synchronize()
            hist.append([float(v) for v in losses])
            shas.append(hashlib.sha256(net.params.cpu().numpy().tobytes()).hexdigest())      # every variable, after every step
            res['index:%d' % t] = net.class_index[:S].cpu().numpy()
            for i, c in enumerate(net.convs):                                                  # this shard's pre-activations: the oracle's kink side
                res['z:%d:%s' % (t, c.name)] = net.z[i].cpu().numpy()
        for k in net.variables:
            res['w:' + k] = net.get_variable(k).cpu().numpy()
        res['losses'] = np.array(hist)
        res['arena_sha'] = np.array(shas)
        res['compact'] = np.array([net.compact_active(), net.sample_comm is not None])
    np.savez(out + '.rank%d.npz' % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
    sys.stdout.flush()
    if sys.argv[1] != 'single':     # 'single' runs under a kernel tracer, which writes its files when the interpreter exits normally
        os._exit(0)
