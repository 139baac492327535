#!/usr/bin/env python3
"""Region maps derived from a change map: the device route (csrc/regions.hip) against the NumPy oracle, on two seeded uint8
maps of ``--size`` x ``--size`` -- ``blobs`` (foreground density about 0.02 in rectangles: the typical component count) and
``checker`` (a checkerboard at connectivity 1: one component per foreground pixel, the largest count there is; the derive
itself runs it at the reference's connectivity 2, where it is ONE component through every tile border).

Per case and entry point (``fcd_label_components``, ``fcd_component_boxes``, ``fcd_region_paint``): device events around
``--launches`` back-to-back launches after a warm-up of as many, ``--repeats`` repetitions, median / min / max in microseconds
per launch, and the achieved bytes/s against the bytes the entry point MUST move (map in + labels out; labels in + boxes out;
map out).  End to end: ``tiles.region_map`` on a resident tensor (label + read K + boxes + paint, host clock, device drained)
and from a host array (upload and download included), against ``tiles.region_map_host`` on this machine (plain NumPy / Python,
one thread, ``--host-repeats`` runs).  The device map must equal the host map.

Prints ONE JSON line; ``--md FILE`` also writes the figures as a table between the ``measured`` markers of that file.

    python tools/bench_region_derive.py --size 2048 --launches 50 --repeats 7 --md profiles/region_derive.md
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

from fcd_gan_pytorch_amd import _lib, _ops as ops, tiles  # noqa: E402

BEGIN, END = '<!-- measured:begin -->', '<!-- measured:end -->'


def summary(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def blobs(size, seed, density=0.02):
    rng = np.random.default_rng(seed)
    m = np.zeros((size, size), np.uint8)
    while m.mean() < density:
        h, w = (int(v) for v in rng.integers(4, 25, 2))
        y, x = int(rng.integers(0, size - h)), int(rng.integers(0, size - w))
        m[y:y + h, x:x + w] = 1
    return m


def checker(size):
    return (1 - np.indices((size, size)).sum(0) % 2).astype(np.uint8)


def device_us(fn, launches, repeats):
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return out


def wall_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def run_case(name, m, connectivity, a):
    lib, dev = _lib.lib, torch.device('cuda')
    H, W = m.shape
    N = H * W
    t = torch.from_numpy(m).to(dev)
    labels, K = ops.label_components(t, 0, connectivity=connectivity)
    boxes = ops.component_boxes(labels, K)
    region = ops.region_paint(boxes, H, W, a.expand)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.fcd_label_components_ws_bytes(H, W)
    ws = ops._ws(nbytes, dev)
    p = ops._p
    calls = {
        'label_components': (lambda: _lib.check(lib.fcd_label_components(p(t), ops.SAMPLE_U8, H, W, 0.0, connectivity, 0, 0, p(labels),
                                                                         p(count), p(ws), nbytes, ops._stream())), N * (1 + 4)),
        'component_boxes': (lambda: _lib.check(lib.fcd_component_boxes(p(labels), H, W, K, p(boxes), ops._stream())), N * 4 + K * 16),
        'region_paint': (lambda: _lib.check(lib.fcd_region_paint(p(boxes), K, H, W, a.expand, 0, 0, p(region), ops._stream())),
                         N + K * 16),
    }
    out = dict(case=name, connectivity=connectivity, K=K)
    for key, (fn, must_move) in calls.items():
        us = summary(device_us(fn, a.launches, a.repeats))
        out[key] = dict(us_per_launch=us, must_move_bytes=must_move, achieved_GBps=round(must_move / us['median'] / 1e3, 1))
    return out


def run_end_to_end(name, m, a):
    dev = torch.device('cuda')
    t = torch.from_numpy(m).to(dev)
    got = tiles.region_map(t, expand=a.expand)                                  # warm
    out = dict(case=name,
               resident_ms=summary(wall_ms(lambda: tiles.region_map(t, expand=a.expand), a.repeats)),
               from_host_array_ms=summary(wall_ms(lambda: tiles.region_map(m, expand=a.expand, device=dev), a.repeats)))
    host = []
    for _ in range(max(a.host_repeats, 1)):
        t0 = time.perf_counter()
        want = tiles.region_map_host(m, expand=a.expand)
        host.append((time.perf_counter() - t0) * 1e3)
    out['host_numpy_ms'] = summary(host)
    out['equals_host'] = bool(np.array_equal(got.cpu().numpy(), want))
    return out


def table(res):
    rows = ['| case | entry point | K | us per launch: median (min - max) | bytes it must move | achieved GB/s |', '|---|---|---|---|---|---|']
    for c in res['kernels']:
        for key in ('label_components', 'component_boxes', 'region_paint'):
            u = c[key]['us_per_launch']
            rows.append('| `%s`, connectivity %d | `fcd_%s` | %d | %.2f (%.2f - %.2f) | %d | %.1f |'
                        % (c['case'], c['connectivity'], key, c['K'], u['median'], u['min'], u['max'], c[key]['must_move_bytes'],
                           c[key]['achieved_GBps']))
    rows += ['', '| case | `region_map`, resident tensor, ms | `region_map`, host array in and out, ms | `region_map_host`, ms | maps equal |',
             '|---|---|---|---|---|']
    f = lambda s: '%.2f (%.2f - %.2f)' % (s['median'], s['min'], s['max'])
    for c in res['end_to_end']:
        rows.append('| `%s` | %s | %s | %s | %s |' % (c['case'], f(c['resident_ms']), f(c['from_host_array_ms']), f(c['host_numpy_ms']),
                                                     c['equals_host']))
    return '\n'.join(rows)


def write_md(path, res):
    block = '%s\n```json\n%s\n```\n\n%s\n%s' % (BEGIN, json.dumps(res), table(res), END)
    text = open(path).read() if os.path.exists(path) else '# Region maps derived on the device\n\n%s\n%s\n' % (BEGIN, END)
    if BEGIN not in text or END not in text:
        raise SystemExit('%s has no %s ... %s block' % (path, BEGIN, END))
    head, rest = text.split(BEGIN, 1)
    with open(path, 'w') as f:
        f.write(head + block + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--expand', type=int, default=10)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--host-repeats', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_region_derive needs a GPU: there is no fallback to time')
    maps = {'blobs': blobs(a.size, a.seed), 'checker': checker(a.size)}
    res = dict(tool='bench_region_derive', device=torch.cuda.get_device_name(0), size=a.size, sample='uint8', expand=a.expand,
               launches=a.launches, repeats=a.repeats, host_repeats=a.host_repeats, host_threads=1,
               density={k: round(float(v.mean()), 4) for k, v in maps.items()}, kernels=[], end_to_end=[])
    for name, conn in (('blobs', 2), ('checker', 2), ('checker', 1)):
        res['kernels'].append(run_case(name, maps[name], conn, a))
    for name in maps:
        res['end_to_end'].append(run_end_to_end(name, maps[name], a))
    print(json.dumps(res))
    if a.md:
        write_md(a.md, res)


if __name__ == '__main__':
    main()
