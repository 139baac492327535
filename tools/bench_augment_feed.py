#!/usr/bin/env python3
"""Kernel times of the resident scene layer (csrc/scene.hip), by device events:

  * at the bench shape, tiles cut from one uint16 scene: ``fcd_scene_set_cut`` (NORMALIZE), ``fcd_scene_set_cut_aug`` in mode 2
    (SCALE) with ``--rects`` rectangles per tile and with none, ``fcd_scene_cut`` of the same tiles;
  * on a ``--stat-size``^2 scene of ``--stat-bands`` bands tiled by ``--patch``: ``fcd_scene_stats`` (uint16 and float32),
    ``fcd_scene_minmax``, and ``fcd_scene_stitch`` / ``fcd_tile_confusion_items`` over the tiles of that grid.

With ``--other-lib PATH``, another build of libfcdgan_hip.so (for instance the parent commit's), every one of these is PAIRED:
that build's entry point runs in the same process on the same inputs, the variants ALTERNATING and rotating their order inside
every repetition.  The outputs of each pair are compared as bit patterns (``equals_other_lib``; a float32 statistics case of 2
bands, 8 x 4200 in one tile -- it crosses the 4096-column segment -- is compared too, not timed), and
``median_vs_other_spread`` says where this build's median lies against the other build's own minimum - maximum over the
repetitions: ``inside``, ``below`` (faster) or ``above by`` so many microseconds.  The exit status is 1 when a pair differs
in a single bit, else 2 when a median lies above.

Every repetition times ``--launches`` back-to-back launches between two events (a tenth of that for the whole-scene passes),
after a warm-up of as many; the result is the median, minimum and maximum over ``--repeats`` repetitions, in microseconds per
launch.  Prints ONE JSON line.

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

OTHER = '_other_lib'
PAIRED = ('fcd_scene_cut', 'fcd_scene_set_cut', 'fcd_scene_set_cut_aug', 'fcd_scene_stats', 'fcd_scene_minmax', 'fcd_scene_stitch',
          'fcd_tile_confusion_items')


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


def same_bits(u, v):
    """Two tensors as integers of their element size, so that NaN compares by its bits."""
    as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[u.element_size()]
    return bool(torch.equal(u.view(as_int), v.view(as_int)))


def run(cases, libs, launches, repeats):
    """``cases``: name -> (alloc, call); ``alloc()`` makes the output tensors of one variant, ``call(lib, *outputs)`` the launch.
    Every case runs once per library of ``libs`` (suffix -> library) on outputs of its own.  Returns the times per variant and,
    with two libraries, whether the outputs of each pair agree bit for bit after their first launch."""
    variants, outs = {}, {}
    for name, (alloc, call) in cases.items():
        for tag, l in libs.items():
            outs[name + tag] = alloc()
            variants[name + tag] = call(l, *outs[name + tag])
    for fn in variants.values():
        assert fn() == 0, _lib.lib.fcd_last_error_string()
    torch.cuda.synchronize()
    equal = {name: all(same_bits(u, v) for u, v in zip(outs[name], outs[name + OTHER])) for name in cases} if OTHER in libs else {}
    for fn in variants.values():
        timed(fn, launches)                              # warm-up
    names, times = list(variants), {k: [] for k in variants}
    for rep in range(repeats):
        # rotate the start and walk backwards every other repetition: what ran just before a variant (and left ITS inputs in the
        # caches) changes from repetition to repetition, so neither build of a pair always runs behind the other
        order = names[rep % len(names):] + names[:rep % len(names)]
        for k in order[::-1] if rep % 2 else order:
            times[k].append(timed(variants[k], launches))
    return times, equal


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
    ap.add_argument('--other-lib', default=None, help='another build of libfcdgan_hip.so that every kernel is paired with')
    a = ap.parse_args()
    dev = torch.device('cuda')
    P = ctypes.c_void_p
    rng = np.random.default_rng(0)
    p = lambda t: None if t is None else P(t.data_ptr())
    stream = lambda: P(torch.cuda.current_stream().cuda_stream)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    libs = {'': _lib.lib}
    if a.other_lib:
        libs[OTHER] = ctypes.CDLL(a.other_lib)
        for name in PAIRED:
            fn = getattr(libs[OTHER], name)
            fn.restype, fn.argtypes = _lib._SIGS[name]

    # ---- the cut: one uint16 scene, NORMALIZE statistics for the plain cuts, SCALE ranges + rectangles for the other
    shape = (a.bands, a.size, a.size)
    t1 = rng.integers(100, 3000, shape).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, shape)).clip(0, 65535).astype(np.uint16)
    patch, pad = (a.patch, a.patch), (a.pad, a.pad)
    C, n = a.bands, a.batch
    scene = tiles.ResidentScene(t1, t2, None, patch, pad, device=dev, stats=tuple(rng.uniform(500, 1500, (4, C))))
    feed = tiles.ResidentSceneSet([scene])
    items = rng.integers(0, len(feed), n).tolist()
    index = feed.index(items)
    tab, _ = feed.table.to(dev)
    one = ops.scene_tile_table(scene.grid, items).to(dev)                # the same tiles as a table of fcd_scene_cut
    ranges = torch.from_numpy(transforms.SCALE([[100.0, 3000.0]] * C, [[60.0, 3040.0]] * C).params(C)).to(dev)
    eraser = transforms.RANDOM_ERASER_MULTI_REGION(multi_region=a.rects, origin_prob=-1.0, rng=random.Random(0))
    regions = []
    while len(regions) < n:                              # exactly --rects rectangles in every tile
        r = eraser.draw((C, a.patch, a.patch))
        if len(r) == a.rects:
            regions.append(r)
    rects = ops.erase_rects(regions, n, a.rects, patch, device=dev)
    set_args = (p(feed._descs), 1, feed.sample_type, C, p(tab), len(feed.table), p(index.dev), n, a.patch, a.patch)

    def set_cut_aug(erase, R):
        return lambda l, x, y: lambda: l.fcd_scene_set_cut_aug(*set_args, p(ranges), 2, -1.0, 1.0, erase, R, p(x), p(y), None, None,
                                                               None, stream())
    xy = lambda: (f32(n, C, a.patch, a.patch), f32(n, C, a.patch, a.patch))
    cut = {
        'set_cut': (xy, lambda l, x, y: lambda: l.fcd_scene_set_cut(*set_args, p(feed._stats_dev), p(x), p(y), None, None, None,
                                                                    stream())),
        'set_cut_aug_scale_%drects' % a.rects: (xy, set_cut_aug(p(rects.dev), a.rects)),
        'set_cut_aug_scale_0rects': (xy, set_cut_aug(None, 0)),
        'scene_cut': (xy, lambda l, x, y: lambda: l.fcd_scene_cut(p(scene.x), p(scene.y), scene.sample_type, None, 0, C, a.size, a.size,
                                                                  p(one), n, a.patch, a.patch, p(scene._stats_dev), p(x), p(y), None,
                                                                  None, stream()))}
    times, equal = run(cut, libs, a.launches, a.repeats)
    cut_bytes = 2 * n * C * a.patch * a.patch * (4 + 2)   # fp32 written + uint16 read, x and y

    # ---- the whole-scene passes: statistics, extrema, and stitch / confusion counts over the tiles of the same grid
    SC, S = a.stat_bands, a.stat_size
    sshape = (SC, S, S)
    u16 = lambda: torch.from_numpy(rng.integers(1, 4000, sshape).astype(np.uint16).view(np.int16)).to(dev)
    s1, s2 = u16(), u16()
    g1, g2 = (torch.from_numpy(rng.normal(1000.0, 300.0, sshape).astype(np.float32)).to(dev) for _ in range(2))
    grid = tiles.TileGrid(S, S, patch, (0, 0))
    table = ops.scene_tile_table(grid, range(len(grid)))
    tdev, T = table.to(dev), len(table)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)

    def stats(x, y, st, dtype, H=S, W=S, tb=tdev, nt=T, ph=a.patch, pw=a.patch):
        wsb = _lib.lib.fcd_scene_stats_ws_bytes(st, x.shape[0], nt, ph)
        alloc = lambda: (torch.empty(1 + 4 * x.shape[0], dtype=dtype, device=dev), torch.empty(wsb, dtype=torch.uint8, device=dev))
        return alloc, lambda l, out, ws: lambda: l.fcd_scene_stats(p(x), p(y), st, x.shape[0], H, W, p(tb), nt, ph, pw, p(out),
                                                                   p(ws) if wsb else None, wsb, stream())
    mwsb = _lib.lib.fcd_scene_minmax_ws_bytes(SC, T, a.patch)
    cmap = torch.from_numpy(rng.uniform(0, 1, (T, 1, a.patch, a.patch)).astype(np.float32)).to(dev)
    ref_scene = torch.from_numpy(rng.integers(1, 3, (1, S, S)).astype(np.float32)).to(dev)          # gt_map (1, 2)
    ref_tiles = torch.from_numpy(rng.integers(0, 2, (T, 1, a.patch, a.patch)).astype(np.float32)).to(dev)
    rect_table = ops.scene_set_table([grid]).to(dev)[1]
    every = torch.arange(T, dtype=torch.int32, device=dev)
    whole = {
        'scene_stats': stats(s1, s2, ops.SAMPLE_U16, torch.int64),
        'scene_stats_f32': stats(g1, g2, ops.SAMPLE_F32, torch.float64),
        'scene_minmax': (lambda: (f32(4 * SC), i64(1), torch.empty(mwsb, dtype=torch.uint8, device=dev)),
                         lambda l, ext, cnt, ws: lambda: l.fcd_scene_minmax(p(s1), p(s2), ops.SAMPLE_U16, SC, S, S, p(tdev), T, a.patch,
                                                                            a.patch, p(ext), p(cnt), p(ws), mwsb, stream())),
        'scene_stitch': (lambda: (torch.zeros(1, S, S, device=dev), torch.zeros(1, S, S, device=dev), i64(4)),
                         lambda l, density, color, counts: lambda: l.fcd_scene_stitch(
                             p(cmap), p(tdev), T, a.patch, a.patch, 0, 0, 0.5, 1.0, 2.0, 0.0, 1.0, 1, p(ref_scene), S, S, p(density),
                             p(color), p(counts), stream())),
        'tile_confusion_items': (lambda: (i64(4),),
                                 lambda l, counts: lambda: l.fcd_tile_confusion_items(
                                     p(cmap), p(ref_tiles), p(rect_table), T, p(every), T, a.patch, a.patch, 0.5, 0.0, 1.0, 0.0, 1.0,
                                     p(counts), stream()))}
    few = max(1, a.launches // 10)
    stimes, sequal = run(whole, libs, few, a.repeats)
    equal.update(sequal)
    if a.other_lib:                                      # equality only: one tile whose rows cross the 4096-column segment
        e1, e2 = (rng.normal(0.0, 50.0, (2, 8, 4200)).astype(np.float32) for _ in range(2))
        e1[:, :, ::7] = 0.0                              # masked-out columns on both sides of the segment border
        e1, e2 = torch.from_numpy(e1).to(dev), torch.from_numpy(e2).to(dev)
        egrid = tiles.TileGrid(4200, 8, (4200, 8), (0, 0))
        etab = ops.scene_tile_table(egrid, range(len(egrid)))
        alloc, call = stats(e1, e2, ops.SAMPLE_F32, torch.float64, H=8, W=4200, tb=etab.to(dev), nt=len(etab), ph=8, pw=4200)
        outs = {tag: alloc() for tag in libs}
        for tag, l in libs.items():
            assert call(l, *outs[tag])() == 0, _lib.lib.fcd_last_error_string()
        torch.cuda.synchronize()
        equal['scene_stats_f32_2x8x4200'] = same_bits(outs[''][0], outs[OTHER][0])
    out = dict(tool='bench_augment_feed', device=torch.cuda.get_device_name(0), sample='uint16', bands=C, patch=a.patch, batch=n,
               launches=a.launches, repeats=a.repeats, cut_bytes=cut_bytes,
               us_per_launch={k: summary(v) for k, v in times.items()},
               stat_scene=list(sshape), stat_tiles=T, stat_launches=few, stat_us_per_launch={k: summary(v) for k, v in stimes.items()})
    if a.other_lib:
        both = dict(times, **stimes)
        out['plain_cut_equals_other_lib'] = equal['set_cut']
        out['equals_other_lib'] = equal
        spread = {}
        for k in both:
            if k + OTHER in both:
                m, lo, hi = statistics.median(both[k]), min(both[k + OTHER]), max(both[k + OTHER])
                spread[k] = 'inside' if lo <= m <= hi else 'below' if m < lo else 'above by %.2f' % (m - hi)
        out['median_vs_other_spread'] = spread
        slower = any(v.startswith('above') for v in spread.values())
    print(json.dumps(out))
    return 1 if not all(equal.values()) else 2 if a.other_lib and slower else 0


if __name__ == '__main__':
    sys.exit(main())
