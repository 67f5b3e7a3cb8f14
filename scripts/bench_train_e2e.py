"""End-to-end throughput of train.py fed by the real input pipeline (list file of JPEGs -> decode workers -> pinned staging ->
GPU step), to be read against bench.py's synthetic-input figure: does the loader keep the GPU busy?

    python scripts/bench_train_e2e.py [--net SphereNet-ASoftmax] [--batch 512] [--steps 60] [--images 4096] [--src 250]
                                      [--augmentation 0|1|2|3] [--packed 0|1 [--pack_on_gpu 0|1]] [--synthetic 0|1]

Writes N synthetic JPEGs (src x src, CASIA-WebFace crops are 250 x 250) and a list file to a temporary directory, then runs
train.py (resize to 128 x 128, random crop 112 x 112, flip -- the reference's SphereFace recipe) as a child process and prints
its own 'mean throughput' line.  --packed 1: the set is packed first (pack_list.py, lossless) and train.py reads the pack
(--packed_data_path; --pack_on_gpu 1: resident in device memory).  --synthetic 1: the same command on a resident random batch,
the rate the step itself sustains -- the figure the other three are read against."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', default='SphereNet-ASoftmax')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--src', type=int, default=250)
    ap.add_argument('--mfma_dtype', default='f32')
    ap.add_argument('--augmentation', type=int, choices=[0, 1, 2, 3], default=0,
                    help='passed to train.py: 1 = the colour augmentation, 2 = the geometric pair, 3 = both')
    ap.add_argument('--packed', type=int, default=0, help='1: pack the generated set and train from the pack')
    ap.add_argument('--pack_on_gpu', type=int, default=0, help='--packed 1: the pack resident in device memory')
    ap.add_argument('--synthetic', type=int, default=0, help='1: train.py --synthetic 1 (no images are written or read)')
    ap.add_argument('--data_dir', default=None, help='keep the JPEGs, their list and the pack here and reuse them (several runs on ONE set)')
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:                          # checkpoints and logs: always fresh (train.py resumes from a checkpoint it finds)
        data_dir = d if a.data_dir is None else os.path.abspath(a.data_dir)
        os.makedirs(data_dir, exist_ok=True)
        lst = os.path.join(data_dir, 'list_%d_%d.txt' % (a.images, a.src))
        if not a.synthetic and not os.path.exists(lst):
            base = rng.integers(0, 255, (a.src, a.src, 3), dtype=np.uint8)
            lines = []
            for i in range(a.images):
                p = os.path.join(data_dir, '%d_%06d.jpg' % (a.src, i))
                Image.fromarray(np.roll(base, i * 7, axis=1)).save(p, quality=90)
                lines.append('%s %d' % (p, i % 1000))
            open(lst, 'w').write('\n'.join(lines) + '\n')
        source = ['--train_list_path', lst]
        if a.synthetic:
            source = ['--synthetic', '1', '--synthetic_classes', '1000']
        elif a.packed:
            pack = os.path.join(data_dir, 'set_%d_%d.fpk' % (a.images, a.src))
            r = None if os.path.exists(pack) else subprocess.run([sys.executable, os.path.join(ROOT, 'pack_list.py'), '--data_list_path', lst, '--out', pack], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, cwd=ROOT)
            if r is not None:
                print(r.stdout.strip())
                if r.returncode:
                    return r.returncode
            source = ['--packed_data_path', pack, '--pack_on_gpu', str(a.pack_on_gpu)]
        cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--net_name', a.net, '--model_name', 'e2e', '--train_dir', os.path.join(d, 'train'),
               '--model_dir', os.path.join(d, 'models')] + source + ['--input_height', '128', '--input_width', '128',
               '--crop_height', '112', '--crop_width', '112', '--batch_size', str(a.batch), '--num_gpus', '1', '--init_lr', '0.001',
               '--max_epoches', '1000', '--lr_decay_epoch', '400,800', '--max_steps', str(a.steps), '--display_interval', '20', '--save_interval', '100000',
               '--mfma_dtype', a.mfma_dtype] + (['--augmentation', str(a.augmentation)] if a.augmentation else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        tail = [ln for ln in out.stdout.splitlines() if 'mean throughput' in ln or 'sustained' in ln or 'Error' in ln or 'error' in ln or 'image pack' in ln]
        print('\n'.join(tail[-4:]) if tail else out.stdout[-2000:])
        return out.returncode


if __name__ == '__main__':
    sys.exit(main())
