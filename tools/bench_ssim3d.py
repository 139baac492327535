#!/usr/bin/env python3
"""Time one volumetric SSIM level (csrc/ssim3d.hip) against the stock-op composition a user would otherwise run
(tests/golden/ssim3d_truth.py in fp32 on the device: fifteen depthwise conv3d calls plus the elementwise tail).

Forward alone and forward + backward, warm, HIP events, the two alternated within every repeat, median and spread over the
repeats.  The outputs of the two are compared at the timed size first.  Prints a markdown report (profiles/ssim3d_level.md is
one); needs a GPU -- there is no CPU fallback to time.

    python tools/bench_ssim3d.py [--shape 2 4 16 256 256] [--repeats 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import ssim3d_truth as T3  # noqa: E402

C1, C2 = 0.01 ** 2, 0.03 ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=5, default=[2, 4, 16, 256, 256])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ssim3d needs a GPU'
    from fcd_gan_pytorch_amd import _lib, _ops as ops
    shape = tuple(a.shape)
    x, y = T3.inputs(shape, 1)
    ws, wc = T3.upstream(shape, 1)
    x, y, ws, wc, g = x.cuda(), y.cuda(), ws.cuda(), wc.cuda(), T3.taps().cuda()

    def fused(backward):
        xg, yg = x.detach().requires_grad_(backward), y.detach().requires_grad_(backward)
        s, cs = ops.ssim_level(xg, yg, g, C1, C2)
        if backward:
            ((s * ws).sum() + (cs * wc).sum()).backward()
        return s, cs, xg.grad, yg.grad

    def stock(backward):
        xg, yg = x.detach().requires_grad_(backward), y.detach().requires_grad_(backward)
        with torch.set_grad_enabled(backward):
            s, cs = T3.level(xg, yg, g, C1, C2)
        if backward:
            ((s * ws).sum() + (cs * wc).sum()).backward()
        return s, cs, xg.grad, yg.grad

    def timed(fn, backward):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(backward)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # same function at the timed size?
    rf, rs = fused(True), stock(True)
    diffs = []
    for name, p, q in zip(('ssim', 'cs', 'dX', 'dY'), rf, rs):
        diffs.append((name, (p - q).abs().max().item() / max(q.abs().max().item(), 1e-30)))
    for _ in range(a.warmup):
        for bw in (False, True):
            fused(bw), stock(bw)
    torch.cuda.synchronize()
    t = {(n, bw): [] for n in ('fused', 'stock') for bw in (False, True)}
    for _ in range(a.repeats):
        for bw in (False, True):
            t[('fused', bw)].append(timed(fused, bw))
            t[('stock', bw)].append(timed(stock, bw))
    vox = 1
    for s in shape:
        vox *= s
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = ['# One volumetric SSIM level, fused kernel against the stock-op composition', '',
             'Shape (N, C, T, H, W) = %s, float32, 11-tap window; %s; library build stamp `%s`.' %
             (shape, torch.cuda.get_device_name(0), _lib.build_hash()),
             'Warm, HIP events around each call (autograd graph construction included in both), %d repeats with the two '
             'alternated inside every repeat; median [min .. max] in ms.' % a.repeats, '',
             '| | fused (`ops.ssim_level`) | stock ops (`ssim3d_truth.level`, fp32) | ratio |', '|---|---|---|---|']
    for bw, label in ((False, 'forward'), (True, 'forward + backward')):
        f, s = t[('fused', bw)], t[('stock', bw)]
        lines.append('| %s | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.1fx |' %
                     (label, med[('fused', bw)], min(f), max(f), med[('stock', bw)], min(s), max(s),
                      med[('stock', bw)] / med[('fused', bw)]))
    fwd_bytes = 8.0 * vox
    lines += ['', 'Algorithmic bytes of the forward pass: X and Y read once, 8 B/voxel = %.1f MB; over the fused forward '
              'time that is %.0f GB/s (call time, two launches and the host side included -- not a kernel time).' %
              (fwd_bytes / 1e6, fwd_bytes / (med[('fused', False)] * 1e-3) / 1e9),
              '', 'Largest difference between the two at this size, relative to the largest magnitude of the stock result: ' +
              ', '.join('%s %.2e' % d for d in diffs) + '.']
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
