"""-m gpu: SphereNet's backward walk comes out the same bit for bit however it is scheduled -- two or three dz buffers per stage
(FTE_DZ_BUFFERS), filter gradients on the second stream or one chain, backward() or backward_stages() one callable at a time -- in
each precision mode: the same kernels run on the same operands in the same order (nets/sphere.py _body_walk).  8 images of 40x24x3:
stages of 20x12, 10x6, 5x3 (odd) and 3x2, every residual block lean in fp32 (tests/test_gpu_wino_lean_epilogue.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import spherenet as osn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tf_face_toolbox_amd import _lib, net_select

N, H, W, CH, NCLS = 8, 40, 24, 3, 10


def _arena(env=None, one_stream=False, stages=False):
    """the gradient arena (with the loss slots) of one training pass: forward, loss, backward"""
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)                               # the net reads its switches when it is constructed
        net = net_select('SphereNet-ASoftmax', 'NCHW', 5e-4)
        net.build(H, W, CH, NCLS, 'cuda')
        net.load_params(osn.perturb_params(osn.init_params(11, CH, NCLS, H, W), 12))
        r = np.random.default_rng(5)
        x = torch.tensor(r.uniform(-1, 1, (N, H, W, CH)), dtype=torch.float32, device='cuda')
        y = torch.tensor(r.integers(0, NCLS, N), dtype=torch.int32, device='cuda')
        net.tower_scale = 1.0
        net.one_stream = one_stream
        logits = net.forward(x, y, num_classes=NCLS, is_training=True)
        assert (net._side_stream(N) is None) == one_stream
        assert len(net.bwd[0].dz) == int(env.get('FTE_DZ_BUFFERS', 3))
        net.loss_function('TOWER', y, **logits)
        if stages:
            for stage in net.backward_stages():
                stage()
                torch.cuda.synchronize()
        else:
            net.backward()
        torch.cuda.synchronize()
        return net.grads.clone()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'bf16s'])      # fp32, bf16 operands read as copies, bf16 storage
def test_backward_walk_is_bit_equal_however_it_is_scheduled(mode):
    prev = _lib.precision_mode()
    _lib.set_mfma_dtype(mode)
    try:
        base = _arena({'FTE_DZ_BUFFERS': '3'})      # two streams, three dz buffers, backward()
        assert float(base.abs().max()) > 0 and bool(torch.isfinite(base).all())
        assert torch.equal(base, _arena({'FTE_DZ_BUFFERS': '2'})), 'FTE_DZ_BUFFERS 2 against 3'
        assert torch.equal(base, _arena(one_stream=True)), 'one stream against two'
        assert torch.equal(base, _arena(stages=True)), 'backward_stages() stepped against backward()'
    finally:
        _lib.set_mfma_dtype(prev)
