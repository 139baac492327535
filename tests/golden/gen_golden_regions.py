#!/usr/bin/env python3
"""Fixtures for the region maps derived from a change map (tiles.region_map / region_map_host, csrc/regions.hip) ->
regions.npz, byte for byte the same on every run (fixed seeds, sorted keys, zip entries without a clock).

The reference makes these maps with skimage (OSCDProcess.py:56-73, BuildingProcess.py:127-145): ``measure.label(connectivity=2)``,
``regionprops`` boxes, every box grown by ``region_expand`` and clamped.  skimage is not on the build machine, so the
reference's own two scripts cannot be run here and this file RESTATES them on scipy: ``scipy.ndimage.label`` with
``structure=np.ones((3, 3))`` for connectivity 2 (the default structure for connectivity 1), ``find_objects`` for the boxes,
and the reference's clamp lines copied in meaning:  lo = lo - e if lo - e > lo_bound else lo_bound;  hi = hi + e if hi + e <
hi_bound else hi_bound.  The region map does not depend on how the components are numbered; only the label images lean on
scipy's numbering (raster order of each component's first pixel).  With a slice every slice is labelled on its own, as
BuildingProcess does, and the components are renumbered over the scene in raster order of their first pixel; a box is clamped
to its slice's rectangle cut to the scene.

Per case ``<name>``: map (uint8 unless said), thresh, slice (0, 0: none), and for connectivity c in conns: labels<c> (int32),
boxes<c> (int32 (K,4) min_y, min_x, max_y, max_x half-open); region<e> (uint8) for e in EXPANDS at connectivity 2."""
import io
import os
import zipfile

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
EXPANDS = (0, 3, 10, 500)


def save(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def serpentine(n):
    a = np.zeros((n, n), np.uint8)
    a[0::2] = 1
    a[1::4, n - 1] = 1
    a[3::4, 0] = 1
    return a


def spiral(n):
    a = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = 1
    while True:
        for _ in range(2):                                   # straight on, else one turn to the right
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not a[ny, nx] and not (0 <= fy < n and 0 <= fx < n and a[fy, fx]):
                y, x = ny, nx
                a[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return a


def edges16(H, W):
    near = lambda n: np.isin(np.arange(n) % 16, (15, 0, 1))
    return (near(H)[:, None] | near(W)[None, :]).astype(np.uint8)


def cases():
    """name -> (map, thresh, slice or None, connectivities)"""
    rng = np.random.default_rng(2718)
    both = (1, 2)
    out = {}
    out['one_fg'] = (np.ones((1, 1), np.uint8), 0, None, both)
    out['one_bg'] = (np.zeros((1, 1), np.uint8), 0, None, both)
    runs = (np.arange(300) // 7 % 2).astype(np.uint8)
    out['row300'] = (runs[None, :].copy(), 0, None, both)
    out['col300'] = (runs[:, None].copy(), 0, None, both)
    out['rand01'] = ((rng.random((67, 45)) < 0.1).astype(np.uint8), 0, None, both)
    out['rand05'] = ((rng.random((67, 45)) < 0.5).astype(np.uint8), 0, None, both)
    out['checker'] = ((1 - np.indices((131, 197)).sum(0) % 2).astype(np.uint8), 0, None, both)
    out['all_fg'] = (np.full((131, 197), 7, np.uint8), 0, None, both)
    out['all_bg'] = (np.zeros((131, 197), np.uint8), 0, None, both)
    out['serpentine'] = (serpentine(160), 0, None, both)
    out['spiral'] = (spiral(160), 0, None, both)
    d = np.eye(160, dtype=np.uint8)
    out['diagonals'] = (d | d[:, ::-1], 0, None, both)
    out['edges16'] = (edges16(131, 197), 0, None, both)
    blobs = (ndimage.uniform_filter(rng.random((131, 197)), 9) > 0.52).astype(np.uint8) * 255
    out['sliced'] = (blobs, 0, (50, 64), both)
    out['u16'] = (rng.integers(0, 3, (67, 45)).astype(np.uint16), 1, None, both)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.0, 1e-30], np.float32)
    out['f32'] = (vals[rng.integers(0, len(vals), (67, 45))], 0, None, both)
    return out


def label_blocks(fg, conn, sl):
    """scipy labels, every slice on its own, renumbered in raster order of each component's first pixel."""
    structure = np.ones((3, 3)) if conn == 2 else None
    H, W = fg.shape
    sh, sw = sl or (H, W)
    lab = np.zeros((H, W), np.int64)
    k = 0
    for y0 in range(0, H, sh):
        for x0 in range(0, W, sw):
            part, n = ndimage.label(fg[y0:y0 + sh, x0:x0 + sw], structure=structure)
            lab[y0:y0 + sh, x0:x0 + sw] = np.where(part > 0, part + k, 0)
            k += n
    flat = lab.ravel()
    ids, first = np.unique(flat[flat > 0], return_index=True)
    order = np.zeros(k + 1, np.int64)
    order[ids[np.argsort(first)]] = np.arange(1, len(ids) + 1)
    return order[lab].astype(np.int32), k


def boxes_of(lab):
    return np.array([[s[0].start, s[1].start, s[0].stop, s[1].stop] for s in ndimage.find_objects(lab)], np.int32).reshape(-1, 4)


def region_of(fg, e, sl):
    """The reference's loop, slice by slice (OSCDProcess.py:59-73 is the one-slice case)."""
    H, W = fg.shape
    sh, sw = sl or (H, W)
    region = np.zeros((H, W), np.uint8)
    for y0 in range(0, H, sh):
        for x0 in range(0, W, sw):
            block = fg[y0:y0 + sh, x0:x0 + sw]
            out = region[y0:y0 + sh, x0:x0 + sw]
            lab, _ = ndimage.label(block, structure=np.ones((3, 3)))
            for s in ndimage.find_objects(lab):
                min_y, min_x, max_y, max_x = s[0].start, s[1].start, s[0].stop, s[1].stop
                min_y = min_y - e if (min_y - e) > 0 else 0
                min_x = min_x - e if (min_x - e) > 0 else 0
                max_y = max_y + e if (max_y + e) < block.shape[0] else block.shape[0]
                max_x = max_x + e if (max_x + e) < block.shape[1] else block.shape[1]
                out[min_y:max_y, min_x:max_x] = 255
    return region


def main():
    out = {}
    names = []
    for name, (m, thresh, sl, conns) in cases().items():
        names.append(name)
        with np.errstate(invalid='ignore'):
            fg = m.astype(np.float64) > thresh
        out[name + '/map'] = m
        out[name + '/thresh'] = np.array(thresh, np.float64)
        out[name + '/slice'] = np.array(sl or (0, 0), np.int64)
        out[name + '/conns'] = np.array(conns, np.int64)
        for c in conns:
            lab, k = label_blocks(fg, c, sl)
            assert lab.max(initial=0) == k
            out['%s/labels%d' % (name, c)] = lab
            out['%s/boxes%d' % (name, c)] = boxes_of(lab)
            assert len(out['%s/boxes%d' % (name, c)]) == k
        for e in EXPANDS:
            out['%s/region%d' % (name, e)] = region_of(fg, e, sl)
    assert len(out['checker/boxes2']) == 1 and len(out['checker/boxes1']) == (131 * 197 + 1) // 2
    assert len(out['serpentine/boxes1']) == 1 and len(out['spiral/boxes1']) == 1 and len(out['diagonals/boxes2']) == 1
    out['cases'] = np.array(names)
    out['expands'] = np.array(EXPANDS, np.int64)
    path = os.path.join(HERE, 'regions.npz')
    save(path, out)
    print('wrote regions.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
