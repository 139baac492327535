#!/usr/bin/env python3
"""Kernel times of the resident feed's cut and extrema (csrc/scene.hip), by device events, at the bench shape:

  * ``fcd_scene_set_cut`` (NORMALIZE), ``fcd_scene_set_cut_aug`` in mode 2 (SCALE) with ``--rects`` rectangles per tile, and --
    with ``--other-lib PATH``, another build of libfcdgan_hip.so (for instance the parent commit's) -- that build's
    ``fcd_scene_set_cut`` on the same buffers, the variants ALTERNATING inside every repetition; the two plain cuts are also
    compared bit for bit;
  * ``fcd_scene_minmax`` next to ``fcd_scene_stats`` on a ``--stat-size``^2 scene of ``--stat-bands`` bands.

Every repetition times ``--launches`` back-to-back launches between two events (after a warm-up of as many); the result is
the median, minimum and maximum over ``--repeats`` repetitions, in microseconds per launch.  Prints ONE JSON line.

    python tools/bench_augment_feed.py --bands 13 --patch 256 --batch 8 --repeats 7
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fcd_gan_pytorch_amd import _lib, _ops as ops, tiles, transforms  # noqa: E402


def summary(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches           # microseconds per launch


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bands', type=int, default=13)
    ap.add_argument('--size', type=int, default=1024, help='side of the scene the tiles are cut from')
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--pad', type=int, default=0)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rects', type=int, default=5)
    ap.add_argument('--stat-size', type=int, default=2048)
    ap.add_argument('--stat-bands', type=int, default=4)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--other-lib', default=None, help='another build of libfcdgan_hip.so whose fcd_scene_set_cut is timed too')
    a = ap.parse_args()
    dev = torch.device('cuda')
    lib, P = _lib.lib, ctypes.c_void_p
    rng = np.random.default_rng(0)
    p = lambda t: None if t is None else P(t.data_ptr())
    stream = lambda: P(torch.cuda.current_stream().cuda_stream)

    # ---- the cut: one uint16 scene, NORMALIZE statistics for the plain cut, SCALE ranges + rectangles for the other
    shape = (a.bands, a.size, a.size)
    t1 = rng.integers(100, 3000, shape).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, shape)).clip(0, 65535).astype(np.uint16)
    patch, pad = (a.patch, a.patch), (a.pad, a.pad)
    C, n = a.bands, a.batch
    scene = tiles.ResidentScene(t1, t2, None, patch, pad, device=dev, stats=tuple(rng.uniform(500, 1500, (4, C))))
    feed = tiles.ResidentSceneSet([scene])
    index = feed.index(rng.integers(0, len(feed), n).tolist())
    tab, _ = feed.table.to(dev)
    ranges = torch.from_numpy(transforms.SCALE([[100.0, 3000.0]] * C, [[60.0, 3040.0]] * C).params(C)).to(dev)
    eraser = transforms.RANDOM_ERASER_MULTI_REGION(multi_region=a.rects, origin_prob=-1.0, rng=random.Random(0))
    regions = []
    while len(regions) < n:                              # exactly --rects rectangles in every tile
        r = eraser.draw((C, a.patch, a.patch))
        if len(r) == a.rects:
            regions.append(r)
    rects = ops.erase_rects(regions, n, a.rects, patch, device=dev)
    x = torch.empty((n, C, a.patch, a.patch), dtype=torch.float32, device=dev)
    y, x2 = torch.empty_like(x), torch.empty_like(x)
    sig = _lib._SIGS['fcd_scene_set_cut']

    def plain(l, out_x):
        return lambda: l.fcd_scene_set_cut(p(feed._descs), 1, feed.sample_type, C, p(tab), len(feed.table), p(index.dev), n,
                                           a.patch, a.patch, p(feed._stats_dev), p(out_x), p(y), None, None, None, stream())
    aug = lambda: lib.fcd_scene_set_cut_aug(p(feed._descs), 1, feed.sample_type, C, p(tab), len(feed.table), p(index.dev), n,
                                            a.patch, a.patch, p(ranges), 2, -1.0, 1.0, p(rects.dev), a.rects, p(x), p(y), None,
                                            None, None, stream())
    aug0 = lambda: lib.fcd_scene_set_cut_aug(p(feed._descs), 1, feed.sample_type, C, p(tab), len(feed.table), p(index.dev), n,
                                             a.patch, a.patch, p(ranges), 2, -1.0, 1.0, None, 0, p(x), p(y), None, None, None,
                                             stream())
    variants = {'set_cut': plain(lib, x), 'set_cut_aug_scale_%drects' % a.rects: aug, 'set_cut_aug_scale_0rects': aug0}
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        other.fcd_scene_set_cut.restype, other.fcd_scene_set_cut.argtypes = sig
        variants['set_cut_other_lib'] = plain(other, x2)
        assert variants['set_cut']() == 0 and variants['set_cut_other_lib']() == 0
        torch.cuda.synchronize()
        same = bool(torch.equal(x, x2))
    times = {k: [] for k in variants}
    for fn in variants.values():
        assert fn() == 0, _lib.lib.fcd_last_error_string()
        timed(fn, a.launches)                            # warm-up
    names = list(variants)
    for rep in range(a.repeats):
        for k in names[rep % len(names):] + names[:rep % len(names)]:
            times[k].append(timed(variants[k], a.launches))
    cut_bytes = 2 * n * C * a.patch * a.patch * (4 + 2)   # fp32 written + uint16 read, x and y

    # ---- extrema next to the statistics
    sshape = (a.stat_bands, a.stat_size, a.stat_size)
    s1 = torch.from_numpy(rng.integers(1, 4000, sshape).astype(np.uint16).view(np.int16)).to(dev)
    s2 = torch.from_numpy(rng.integers(1, 4000, sshape).astype(np.uint16).view(np.int16)).to(dev)
    grid = tiles.TileGrid(a.stat_size, a.stat_size, patch, (0, 0))
    table = ops.scene_tile_table(grid, range(len(grid)))
    tdev, T, SC = table.to(dev), len(table), a.stat_bands
    totals = torch.empty(1 + 4 * SC, dtype=torch.int64, device=dev)
    ext, cnt = torch.empty(4 * SC, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    wsb = lib.fcd_scene_minmax_ws_bytes(SC, T, a.patch)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stat = {
        'scene_stats': lambda: lib.fcd_scene_stats(p(s1), p(s2), ops.SAMPLE_U16, SC, a.stat_size, a.stat_size, p(tdev), T, a.patch,
                                                   a.patch, p(totals), None, 0, stream()),
        'scene_minmax': lambda: lib.fcd_scene_minmax(p(s1), p(s2), ops.SAMPLE_U16, SC, a.stat_size, a.stat_size, p(tdev), T,
                                                     a.patch, a.patch, p(ext), p(cnt), p(ws), wsb, stream())}
    stimes = {k: [] for k in stat}
    few = max(1, a.launches // 10)
    for fn in stat.values():
        assert fn() == 0, _lib.lib.fcd_last_error_string()
        timed(fn, few)
    for rep in range(a.repeats):
        for k in (list(stat) if rep % 2 == 0 else list(stat)[::-1]):
            stimes[k].append(timed(stat[k], few))
    out = dict(tool='bench_augment_feed', device=torch.cuda.get_device_name(0), sample='uint16', bands=C, patch=a.patch, batch=n,
               launches=a.launches, repeats=a.repeats, cut_bytes=cut_bytes,
               us_per_launch={k: summary(v) for k, v in times.items()},
               stat_scene=list(sshape), stat_launches=few, stat_us_per_launch={k: summary(v) for k, v in stimes.items()})
    if a.other_lib:
        out['plain_cut_equals_other_lib'] = same
    print(json.dumps(out))


if __name__ == '__main__':
    main()
