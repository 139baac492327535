#!/usr/bin/env python3
"""Wall time of one inference pass over a synthetic set of scenes of unequal size, on two routes:

  (a) ``per_scene``: a loop of ``demos.infer_scene_resident``, one call per scene -- the only resident route before the set
      stitch.  Its batches end at scene borders, so it does NOT form the batches of the reference's test pass.
  (b) ``set``: ``demos.infer_scene_set_resident`` -- one ``fcd_scene_set_cut`` and one ``fcd_scene_set_stitch`` per batch, batches
      running across scene borders.

For each route: the wall time of a whole pass (host clock around a synchronised pass, the final device-to-host copies
included) and ``net_ms``, the time of the Segmentor alone over batches of the same sizes on tiles that already lie on the
device; ``outside_ms`` is their difference -- cutting, stitching, tables, index uploads, map allocation and copies.  The routes
alternate inside every repetition, their order swapping from one repetition to the next; after ``--warmup`` passes of each the
result is the median, minimum and maximum over ``--repeats`` repetitions, in milliseconds.  Prints ONE JSON line.

    python tools/bench_scene_set_infer.py --sizes 1000x1200,700x900,500x400 --bands 4 --patch 256 --pad 8 --batch 8
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

from fcd_gan_pytorch_amd import Module, demos, steps, tiles  # noqa: E402


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def batch_sizes(counts, batch):
    """Sizes of the batches when each of ``counts`` tiles lists is walked on its own in batches of ``batch``."""
    out = []
    for n in counts:
        out += [batch] * (n // batch) + ([n % batch] if n % batch else [])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='1000x1200,700x900,500x400', help='HxW of every scene, comma separated')
    ap.add_argument('--bands', type=int, default=4)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--pad', type=int, default=8)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    patch, pad, C = (a.patch, a.patch), (a.pad, a.pad), a.bands
    sizes = [tuple(int(v) for v in s.split('x')) for s in a.sizes.split(',')]
    scenes = []
    for H, W in sizes:
        t1 = rng.integers(100, 3000, (C, H, W)).astype(np.uint16)
        t2 = (t1 + rng.integers(-40, 40, (C, H, W))).clip(0, 65535).astype(np.uint16)
        ref = rng.integers(1, 3, (1, H, W)).astype(np.uint8)
        scenes.append(tiles.ResidentScene(t1, t2, ref, patch, pad, device=dev, stats=tuple(rng.uniform(500, 1500, (4, C)))))
    feed = tiles.ResidentSceneSet(scenes)
    torch.manual_seed(0)
    net = Module.Segmentor(C, bilinear=True).to(dev).eval()

    def per_scene():
        return [demos.infer_scene_resident(net, s, dev, batch_size=a.batch) for s in scenes]

    def as_set():
        return demos.infer_scene_set_resident(net, feed, dev, batch_size=a.batch)

    # both routes see every tile once: the same pixels are scored (the maps differ in nothing but who made the batches -- in
    # eval mode a tile's density does not depend on its batch)
    one, two = per_scene(), as_set()
    same = all(np.array_equal(o['density'], d) and np.array_equal(o['color'], c)
               for o, d, c in zip(one, two['density'], two['color']))
    same = same and bool((sum(o['evaluator']._sync() for o in one) == two['evaluator']._sync()).all())

    tile = lambda n: torch.randn((n, C, a.patch, a.patch), device=dev)
    shapes = {'per_scene': batch_sizes(feed.numlist, a.batch), 'set': batch_sizes([len(feed)], a.batch)}
    inputs = {n: (tile(n), tile(n)) for n in set(shapes['per_scene'] + shapes['set'])}

    def net_only(route):
        def run():
            with torch.no_grad():
                for n in shapes[route]:
                    steps.infer_density(net, inputs[n][0], inputs[n][1], 0.5)
        return run

    variants = {'per_scene': per_scene, 'set': as_set, 'per_scene_net': net_only('per_scene'), 'set_net': net_only('set')}
    for fn in variants.values():
        for _ in range(a.warmup):
            wall(fn)
    names, times = list(variants), {k: [] for k in variants}
    for rep in range(a.repeats):
        for k in names[::-1] if rep % 2 else names:
            times[k].append(wall(variants[k]))
    out = dict(tool='bench_scene_set_infer', device=torch.cuda.get_device_name(0), sample='uint16', bands=C, scenes=sizes,
               patch=a.patch, pad=a.pad, batch=a.batch, tiles=feed.numlist, warmup=a.warmup, repeats=a.repeats,
               batches={k: len(v) for k, v in shapes.items()}, maps_equal=same)
    for route in ('per_scene', 'set'):
        outside = [p - n for p, n in zip(times[route], times[route + '_net'])]
        out[route] = dict(pass_ms=summary(times[route]), net_ms=summary(times[route + '_net']), outside_ms=summary(outside))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
