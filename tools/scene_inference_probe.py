"""Whole-scene inference: the host tile loop (``demos.infer_scene``) against the device-resident path
(``demos.infer_scene_resident``), each on normalised tiles and on raw tiles (NORMALIZE folded into the first convolution).

Input: a synthetic 4-band uint16 2048x2048 pair with a reference map, 256^2 patches, pad 10, batch 8, eval mode -- generated
from a seed, nothing is read from outside the repository.

  python tools/scene_inference_probe.py [--out timing.md]
      one warm pass, then ``--passes`` timed passes of every variant, ALTERNATING the variants; each timing is a host clock
      around a pass that ends in a device synchronise.  Reports the median wall time per scene and the time outside netS
      (pass time minus the summed device-event time of the network calls).
  rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/scene_inference_probe.py --trace-pass
      the resident path alone (1 warm + 1 pass), for a kernel trace in a run of its own
  python tools/scene_inference_probe.py --trace-report DIR [--out trace.md]
      kernel times of fcd_scene_cut / fcd_scene_stitch out of that trace as achieved bytes/s over their ALGORITHMIC bytes (cut:
      read blocks in, canvases out; stitch: cmap and reference centres in, two maps out), against the HBM peak of the MI355X.

There is no raw route in ``demos.infer_scene``; ``_infer_scene_host_raw`` below restates its loop over ``tiles.RawTiles`` +
``steps.infer_density_raw`` so that the folded-NORMALIZE network can be timed behind the host loop too."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZE, BANDS, PATCH, PAD, BATCH = 2048, 4, (256, 256), (10, 10), 8
HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12      # MI355X HBM3E: spec; measured float4 copy (79 % of spec)


def synthetic_scene(size=SIZE, seed=7):
    rng = np.random.default_rng(seed)
    t1 = rng.integers(100, 3000, (BANDS, size, size)).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, t1.shape)).clip(0, 65535).astype(np.uint16)
    ref = np.ones((1, size, size), np.uint8)
    for k in range(12):                                   # a dozen changed rectangles
        r0, c0 = rng.integers(0, size - 200, 2)
        h, w = rng.integers(40, 200, 2)
        t2[:, r0:r0 + h, c0:c0 + w] = rng.integers(100, 3000, (BANDS, h, w))
        ref[:, r0:r0 + h, c0:c0 + w] = 2
    return t1, t2, ref


def algorithmic_bytes(grid, bands, sample_bytes):
    """(cut, stitch) bytes of ONE pass over the scene, summed over the tiles in the batches the pass runs."""
    cut = stitch = 0
    pw, ph = grid.patch_size
    for item in range(len(grid)):
        (x0, y0, w, h), (rx, ry, rw, rh), _ = grid.slices(item)
        cut += rw * rh * (2 * bands * sample_bytes + 4) + ph * pw * 4 * (2 * bands + 2)      # + float32 reference, + ref and valid tiles
        stitch += w * h * 4 * (2 + 2)                                                      # cmap + reference in, density + color out
    return cut, stitch


def build(device):
    import torch
    import fcd_gan_pytorch_amd as p
    t1, t2, ref = synthetic_scene()
    stats = p.demos._tile_stats(t1, t2, PATCH)
    ds = p.tiles.PairTileDataset(t1, t2, ref, PATCH, PAD, stats=stats)
    scene = p.tiles.ResidentScene(t1, t2, ref, PATCH, PAD, stats=stats, device=device)
    torch.manual_seed(0)
    net = p.Module.Segmentor(BANDS, bilinear=True).to(device).eval()
    return p, net, ds, scene


def _infer_scene_host_raw(p, net, ds, dev):
    """``demos.infer_scene`` over raw tiles: the same host loop, ``steps.infer_density_raw`` as the network call."""
    import torch
    grid = ds.grid
    density = np.zeros((1, grid.ysize, grid.xsize), np.float32)
    color = np.zeros_like(density)
    acc = p.metrics.Evaluator(2)
    with torch.no_grad():
        for (x, y, item, r, valid), real, _ in p.demos._Epoch(p.tiles.RawTiles(ds), BATCH, 0, dev, shuffle=False):
            cmap, mask = p.steps.infer_density_raw(net, x, y, valid, ds.stats, 0.5)
            maskf = mask.to(cmap.dtype)
            items = item.tolist()[:real]
            own = torch.zeros_like(mask)
            for i, it in enumerate(items):
                r0, r1, c0, c1 = grid.eff_range(it)
                own[i, :, r0:r1, c0:c1] = True
            acc.add_batch_map(r, maskf, (1, 2), (0, 1), valid=own)
            codes = p.metrics.changemap_codes(maskf, r, True, ref_map=(1, 2), dt_map=(0, 1))
            cm_h, co_h = cmap.cpu().numpy(), codes.cpu().numpy()
            for i, it in enumerate(items):
                grid.write_center(density, cm_h[i], it)
                grid.write_center(color, co_h[i], it)
    return dict(density=density, color=color, evaluator=acc)


class NetClock:
    """Device-event time of every network call of a pass (``steps.infer_density`` / ``infer_density_raw``)."""

    def __init__(self, p):
        import torch
        self.torch, self.p, self.pairs = torch, p, []
        self.orig = (p.steps.infer_density, p.steps.infer_density_raw)

        def wrap(fn):
            def timed(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*a, **k)
                e1.record()
                self.pairs.append((e0, e1))
                return out
            return timed
        p.steps.infer_density, p.steps.infer_density_raw = wrap(self.orig[0]), wrap(self.orig[1])

    def take_ms(self):
        ms = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return ms

    def close(self):
        self.p.steps.infer_density, self.p.steps.infer_density_raw = self.orig


def timing(args):
    import torch
    assert torch.cuda.is_available(), 'the probe measures on the GPU; there is no CPU figure'
    dev = torch.device('cuda', 0)
    p, net, ds, scene = build(dev)
    variants = [
        ('infer_scene (host tile loop)', lambda: p.demos.infer_scene(net, ds, dev, batch_size=BATCH)),
        ('infer_scene_resident', lambda: p.demos.infer_scene_resident(net, scene, dev, batch_size=BATCH)),
        ('host tile loop, raw tiles', lambda: _infer_scene_host_raw(p, net, ds, dev)),
        ('infer_scene_resident, raw=True', lambda: p.demos.infer_scene_resident(net, scene, dev, batch_size=BATCH, raw=True)),
    ]
    clock = NetClock(p)
    wall = {name: [] for name, _ in variants}
    outside = {name: [] for name, _ in variants}
    results = {}
    for rep in range(args.passes + 1):                    # pass 0 warms every variant up
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            net_ms = clock.take_ms()
            if rep:
                wall[name].append(ms)
                outside[name].append(ms - net_ms)
            results[name] = res
    clock.close()
    base, resd = results[variants[0][0]], results[variants[1][0]]
    same = all(np.array_equal(base[k], resd[k]) for k in ('density', 'color')) and \
        np.array_equal(base['evaluator']._sync(), resd['evaluator']._sync())
    raw_err = float(np.abs(results[variants[3][0]]['density'] - base['density']).max())
    grid = ds.grid
    out = ['## Wall time per scene', '',
           'Synthetic %d-band uint16 %dx%d pair + reference map, %dx%d patches, pad %d, batch %d, eval mode: %d tiles, %d batches.'
           % (BANDS, SIZE, SIZE, PATCH[0], PATCH[1], PAD[0], BATCH, len(grid), -(-len(grid) // BATCH)),
           'One warm pass, then %d timed passes per variant, variants alternating; host clock around a pass that ends in a device '
           'synchronise.  "outside netS" = pass time minus the summed device-event time of the network calls.' % args.passes, '',
           '| variant | median ms / scene | passes (ms) | outside netS, median ms | outside netS (ms) |', '|---|---|---|---|---|']
    for name, _ in variants:
        out.append('| %s | %.1f | %s | %.1f | %s |' % (name, statistics.median(wall[name]), ', '.join('%.1f' % v for v in wall[name]),
                                                      statistics.median(outside[name]), ', '.join('%.1f' % v for v in outside[name])))
    m = {name: (statistics.median(wall[name]), statistics.median(outside[name])) for name, _ in variants}
    a, b = m[variants[0][0]], m[variants[1][0]]
    out += ['', 'Resident path vs `infer_scene`, same scene, same call: end to end %.1f ms vs %.1f ms (%s); outside the network %.1f ms '
            'vs %.1f ms (%s).' % (b[0], a[0], 'not slower' if b[0] <= a[0] else 'SLOWER', b[1], a[1],
                                  'smaller' if b[1] < a[1] else 'NOT smaller'),
            'density, color and confusion matrix of the resident path equal `infer_scene` bit for bit: %s; raw=True density differs '
            'from the normalised path by at most %.2e.' % ('yes' if same else 'NO', raw_err)]
    out += ['', whole_scene_launches(p, scene)]
    return '\n'.join(out)


def whole_scene_launches(p, scene, reps=20):
    """What the two kernels reach when a launch is long enough to stream: ALL tiles of the scene in one launch, device events
    around ``reps`` back-to-back launches (3 warm ones first)."""
    import torch
    grid, n = scene.grid, len(scene)
    table = p._ops.scene_tile_table(grid, range(n))
    cm = torch.rand((n, 1, grid.patch_size[1], grid.patch_size[0]), device=scene.device)
    dens, col = scene.new_maps()
    counts = torch.zeros(4, dtype=torch.int64, device=scene.device)

    def per_launch_us(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    t_cut = per_launch_us(lambda: scene.cut(table))
    t_st = per_launch_us(lambda: p._ops.scene_stitch(cm, table, dens, col, ref=scene.ref, counts=counts))
    cut_b, st_b = algorithmic_bytes(grid, scene.bands, scene.x.element_size())
    out = ['## One launch over all %d tiles (device events around %d back-to-back launches)' % (n, reps), '',
           '| kernel | us / launch | algorithmic bytes | achieved | of 8.0 TB/s spec | of 6.29 TB/s measured copy |', '|---|---|---|---|---|---|']
    for name, us, nb in (('fcd_scene_cut', t_cut, cut_b), ('fcd_scene_stitch', t_st, st_b)):
        rate = nb / (us * 1e-6)
        out.append('| %s | %.1f | %.1f MB | %.2f TB/s | %.1f %% | %.1f %% |' % (name, us, nb / 1e6, rate / 1e12, 100 * rate / HBM_PEAK_SPEC,
                                                                          100 * rate / HBM_PEAK_MEASURED))
    return '\n'.join(out)


def trace_pass():
    import torch
    dev = torch.device('cuda', 0)
    p, net, ds, scene = build(dev)
    for _ in range(2):
        p.demos.infer_scene_resident(net, scene, dev, batch_size=BATCH)
        torch.cuda.synchronize()


def trace_report(directory):
    files = glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('no *kernel_trace.csv under %s (run rocprofv3 with --kernel-trace -f csv)' % directory)
    per = {}
    for f in files:
        with open(f, newline='') as fh:
            for row in csv.DictReader(fh):
                d = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
                calls, total = per.get(row['Kernel_Name'], (0, 0))
                per[row['Kernel_Name']] = (calls + 1, total + d)
    sys.path.insert(0, ROOT)
    from fcd_gan_pytorch_amd import tiles
    grid = tiles.TileGrid(SIZE, SIZE, PATCH, PAD)
    cut_b, stitch_b = algorithmic_bytes(grid, BANDS, 2)
    passes = 2
    total_ns = sum(t for _, t in per.values())
    out = ['## Kernel trace of the resident path (rocprofv3 --kernel-trace --stats, a run of its own: %d passes)' % passes, '',
           '| kernel | calls | total us | avg us | algorithmic bytes / pass | achieved | of 8.0 TB/s spec | of 6.29 TB/s measured copy |',
           '|---|---|---|---|---|---|---|---|']
    for key, nbytes in (('fcd_scene_cut_kernel', cut_b), ('fcd_scene_stitch_kernel', stitch_b)):
        hit = [(n, v) for n, v in per.items() if key in n]
        if not hit:
            out.append('| %s | not in the trace | | | | | | |' % key)
            continue
        calls, ns = sum(v[0] for _, v in hit), sum(v[1] for _, v in hit)
        rate = nbytes * passes / (ns * 1e-9)
        out.append('| %s | %d | %.1f | %.2f | %.1f MB | %.2f TB/s | %.1f %% | %.1f %% |'
                   % (key, calls, ns / 1e3, ns / 1e3 / calls, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_PEAK_SPEC,
                      100 * rate / HBM_PEAK_MEASURED))
    out += ['', 'Total kernel time in the trace: %.2f ms over %d dispatches.  Top kernels:' % (total_ns / 1e6, sum(c for c, _ in per.values())),
            '', '| kernel | calls | total ms | % |', '|---|---|---|---|']
    for name, (calls, ns) in sorted(per.items(), key=lambda kv: -kv[1][1])[:12]:
        out.append('| %s | %d | %.2f | %.1f |' % (name[:110], calls, ns / 1e6, 100.0 * ns / total_ns))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--trace-pass', action='store_true')
    ap.add_argument('--trace-report', metavar='DIR')
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.trace_pass:
        trace_pass()
        return
    txt = trace_report(args.trace_report) if args.trace_report else timing(args)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
