#!/usr/bin/env python3
"""Host feed vs device-resident feed of one training phase: the same epochs of ``steps.usss_g_pretrain_step`` on one synthetic
4-band uint16 scene, once through ``demos._Epoch`` (NumPy tile cutting, DataLoader collate, pinned prefetch thread) and once
through ``tiles.ResidentSceneSet.epoch`` (one cut launch per batch), same seeds, same statistics, same batches.

Prints ONE JSON line: per feed the ms/step (wall, device drained at the end of every epoch) and the host CPU ms/step
(``time.process_time``: all threads of the process, so the prefetch thread counts) as median / min / max over ``--repeats``
alternating runs, and the time of the statistics (host ``demos._tile_stats`` vs ``ResidentScene.statistics()``).

    python tools/bench_resident_feed.py --size 2048 --patch 256 --batch 8 --epochs 2 --repeats 3
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fcd_gan_pytorch_amd import Loss, Module, demos, optim, steps, tiles  # noqa: E402


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--bands', type=int, default=4)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--pad', type=int, default=0)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--epochs', type=int, default=2, help='timed epochs per run (one more runs first, untimed)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    dev = torch.device('cuda')
    rng = np.random.default_rng(a.seed)
    shape = (a.bands, a.size, a.size)
    t1 = rng.integers(100, 3000, shape).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, shape)).clip(0, 65535).astype(np.uint16)
    patch, pad = (a.patch, a.patch), (a.pad, a.pad)

    # ---- statistics: host tile loop vs one device pass over the resident scene (upload not counted: it is needed anyway)
    scene = tiles.ResidentScene(t1, t2, None, patch, pad, device=dev)
    scene.statistics()                                                       # first call: table upload, kernel load
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = scene.statistics()
    stats_dev_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host_stats = demos._tile_stats(t1, t2, patch)
    stats_host_ms = (time.perf_counter() - t0) * 1e3
    stats_rel = max(float(np.max(np.abs(h - d) / np.abs(d))) for h, d in zip(host_stats, stats))
    scene.set_stats(stats)
    ds = tiles.PairTileDataset(t1, t2, None, patch, pad, stats=stats)          # both feeds: the SAME statistics
    feed = tiles.ResidentSceneSet([scene])

    torch.manual_seed(a.seed)
    netG = Module.Generator(n_channels=a.bands).to(dev).train()
    crit = Loss.CNetLoss(channel=a.bands, perception_layer=1, perception_perBand=True, allow_seeded=True).to(dev)
    optG = optim.Adam(netG.parameters(), lr=2e-4, betas=(0.9, 0.99))

    def epochs(kind, first, count):
        n = 0
        for ep in range(first, first + count):
            it = feed.epoch(a.batch, ep) if kind == 'resident' else demos._Epoch(ds, a.batch, ep, dev)
            for (x, y, item, r), real, w in it:
                steps.usss_g_pretrain_step(netG, crit, optG, x, y, perception_weight=0.4, ssim_weight=0, loss_scale=w.loss_scale)
                n += 1
            torch.cuda.synchronize()
        return n

    res = {'host': dict(ms=[], cpu=[]), 'resident': dict(ms=[], cpu=[])}
    for kind in res:
        epochs(kind, 0, 1)                                                    # untimed
    steps_per_run = 0
    for rep in range(a.repeats):
        for kind in ('host', 'resident') if rep % 2 == 0 else ('resident', 'host'):
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            steps_per_run = epochs(kind, 1, a.epochs)
            w1, c1 = time.perf_counter(), time.process_time()
            res[kind]['ms'].append((w1 - w0) * 1e3 / steps_per_run)
            res[kind]['cpu'].append((c1 - c0) * 1e3 / steps_per_run)
    out = dict(tool='bench_resident_feed', device=torch.cuda.get_device_name(0), scene=list(shape), sample='uint16',
               patch=a.patch, pad=a.pad, batch=a.batch, tiles=len(ds), steps_per_run=steps_per_run, repeats=a.repeats,
               step='usss_g_pretrain_step',
               host_ms_per_step=summary(res['host']['ms']), resident_ms_per_step=summary(res['resident']['ms']),
               host_cpu_ms_per_step=summary(res['host']['cpu']), resident_cpu_ms_per_step=summary(res['resident']['cpu']),
               stats_host_ms=round(stats_host_ms, 2), stats_device_ms=round(stats_dev_ms, 3),
               stats_max_rel_diff=float('%.3e' % stats_rel))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
