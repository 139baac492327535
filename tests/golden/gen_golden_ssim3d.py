#!/usr/bin/env python3
"""Generate ``ssim3d.npz``: the REFERENCE's own ``ssim.py`` run in fp64 on (N, C, T, H, W) inputs.

Runs only where the reference checkout is present (it is imported at generation time, nothing of it is copied); the tests
only ever see the ``.npz``.  Inputs are not stored: ``ssim3d_truth.inputs(shape, seed)`` regenerates them.

Per case: the value(s) in fp64 and the gradients w.r.t. both inputs -- in full (float32) where the case has fewer than 20 000
elements, otherwise every STRIDE-th element of the flattened gradient (fp64) with its sum and abs-sum.
  level/<shape>/{ssim, cs}          (N, C) of ``_ssim`` (one scale), gradients under the weights ``ssim3d_truth.upstream``
  ssim/<shape>/{per, nonneg}        public ``ssim(size_average=False)`` on an anti-correlated pair (Y = 1 - X), relu off / on
  ms/<shape>/{val, per}             public ``ms_ssim``; gradients of the scalar

Usage:  python tests/golden/gen_golden_ssim3d.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ssim3d_truth as T3  # noqa: E402

REF = '/root/reference'
SEED, STRIDE, FULL_BELOW = T3.SEED, T3.STRIDE, 20000


def put_grad(out, key, g):
    g = g.detach().double().reshape(-1)
    if g.numel() < FULL_BELOW:
        out[key] = g.float().numpy()
    else:
        out[key + '_sample'] = g[::STRIDE].numpy()
        out[key + '_sums'] = np.array([g.sum().item(), g.abs().sum().item()], np.float64)


def main():
    sys.path.insert(0, REF)
    import ssim as RS
    out = {}
    for shape in T3.LEVEL_SHAPES:
        x, y = T3.inputs(shape, SEED)
        x, y = x.double().requires_grad_(True), y.double().requires_grad_(True)
        win = RS._fspecial_gauss_1d(11, 1.5).repeat([shape[1], 1, 1, 1, 1])
        s, cs = RS._ssim(x, y, data_range=1.0, win=win, size_average=False)
        ws, wc = T3.upstream(shape, SEED)
        ((s * ws.double()).sum() + (cs * wc.double()).sum()).backward()
        k = 'level/' + T3.tag(shape)
        out[k + '/ssim'], out[k + '/cs'] = s.detach().numpy(), cs.detach().numpy()
        put_grad(out, k + '/dX', x.grad)
        put_grad(out, k + '/dY', y.grad)
    shape = T3.LEVEL_SHAPES[0]
    x, _ = T3.inputs(shape, SEED)
    x = x.double()
    k = 'ssim/' + T3.tag(shape)
    out[k + '/per'] = RS.ssim(x, 1 - x, data_range=1.0, size_average=False).numpy()
    out[k + '/nonneg'] = RS.ssim(x, 1 - x, data_range=1.0, size_average=False, nonnegative_ssim=True).numpy()
    for shape in T3.MS_SHAPES:
        x, y = T3.inputs(shape, SEED)
        x, y = x.double().requires_grad_(True), y.double().requires_grad_(True)
        v = RS.ms_ssim(x, y, data_range=1.0)
        v.backward()
        k = 'ms/' + T3.tag(shape)
        out[k + '/val'] = np.array(v.item(), np.float64)
        out[k + '/per'] = RS.ms_ssim(x.detach(), y.detach(), data_range=1.0, size_average=False).numpy()
        put_grad(out, k + '/dX', x.grad)
        put_grad(out, k + '/dY', y.grad)
    path = os.path.join(HERE, 'ssim3d.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
