#!/usr/bin/env python3
"""Fixtures for the reference's OTHER pre-processing (build container only): CommonFunc.NORMALIZE / SCALE / SCALE_NORM,
RANDOM_ERASER / RANDOM_ERASER_MULTI_REGION, Dataset_maxmin, and data_utils.GDALDataset with ``enhance=`` and ``transforms=``
(in-memory GDAL stand-in from gen_golden_tiles.py).  -> augment.npz, byte for byte the same on every run (fixed seeds, sorted
keys, zip entries without a clock).

Scenes: the two sizes of datasets.npz (4x70x90, 4x55x48), patch (40, 32), padding (4, 3), uint16 samples in [1, 4000).  In each
scene a 6x6 block is zero in every band of x -- invalid by the band-sum mask -- and holds 0 and 65535 in y: extremes that
only a mask taken from y, or no mask, would pick up.  No valid sample is 0, so Dataset_maxmin's zero-minimum quirk stays out."""
import io
import os
import random
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_tiles as T  # noqa: E402

PATCH, PAD = (40, 32), (4, 3)
SIZES = {'abudhabi': (4, 70, 90), 'paris': (4, 55, 48)}
BLOCK = {'abudhabi': (20, 50), 'paris': (30, 10)}            # top-left (row, column) of the 6x6 invalid block
ITEMS = {'abudhabi': [0, 8], 'paris': [0, 1, 2, 3, 4, 5]}    # the dataset items kept (every item is DRAWN, in order)
ERASER_SEED, ITEM_SEED, DRAWS = 11, 5, 60


def save(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def scenes(rng):
    out = {}
    for nm, (nb, ys, xs) in SIZES.items():
        x = rng.integers(1, 4000, (nb, ys, xs)).astype(np.uint16)
        y = rng.integers(1, 4000, (nb, ys, xs)).astype(np.uint16)
        r, c = BLOCK[nm]
        x[:, r:r + 6, c:c + 6] = 0
        y[:, r:r + 6, c:c + 6] = (np.indices((6, 6)).sum(0) % 2 * 65535).astype(np.uint16)
        out[nm] = (x, y)
    return out


def main():
    T.install_stubs()
    sys.path.insert(0, T.REF)
    import CommonFunc as RC
    import data_utils as RD
    out = {}
    rng = np.random.default_rng(404)

    # ---- the three enhancers on a float64 block, both switches
    block = rng.uniform(0, 4000, (4, 20, 30))
    stats = np.stack([rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4), rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4)])
    ranges = np.stack([np.stack([rng.uniform(0, 50, 4), rng.uniform(3000, 4100, 4)], 1) for _ in range(2)])   # (2, 4, 2)
    out['enh/block'], out['enh/stats'], out['enh/ranges'] = block, stats, ranges
    out['enh/scale'] = np.array([-1.0, 1.0, 0.25, 3.0])
    lists = [ranges[k].tolist() for k in range(2)]
    objs = {'normalize': RC.NORMALIZE(*[s.tolist() for s in stats]), 'scale': RC.SCALE(lists[0], lists[1]),
            'scale_norm': RC.SCALE_NORM(lists[0], lists[1], [-1, 1]), 'scale_norm_b': RC.SCALE_NORM(lists[0], lists[1], [0.25, 3.0])}
    for name, obj in objs.items():
        for switch in (1, 2):
            out['enh/%s/%d' % (name, switch)] = obj(block.copy(), switch=switch)

    # ---- eraser draws: 60 per class and threshold after random.seed, the erased images of the first five
    image = torch.from_numpy(rng.uniform(1, 2, (3, 32, 40)).astype(np.float32))
    out['erase/image'] = image.numpy()
    out['erase/meta'] = np.array([ERASER_SEED, DRAWS], np.int64)
    for cls, make in (('single', RC.RANDOM_ERASER), ('multi', RC.RANDOM_ERASER_MULTI_REGION)):
        for thresh in (0.3, 0.01):
            random.seed(ERASER_SEED)
            obj = make(erase_thresh=thresh)
            rects, counts, images = [], [], []
            for k in range(DRAWS):
                img, region = obj(image.clone())
                region = [list(region)] if cls == 'single' else [list(r) for r in region]
                rects += region
                counts.append(len(region))
                if k < 5:
                    images.append(img.numpy())
            tag = 'erase/%s/%g' % (cls, thresh)
            out[tag + '/rects'] = np.array(rects, np.int64).reshape(-1, 4)
            out[tag + '/counts'] = np.array(counts, np.int64)
            out[tag + '/images'] = np.stack(images)
            if thresh == 0.01:                                # the clamp h = floor(xsize * ysize * thresh / w) reaches 0
                r = out[tag + '/rects']
                assert ((r[:, 3] == 0) & (r[:, 2] > 0)).any(), 'no h == 0 among the draws of %s' % tag

    # ---- Dataset_maxmin and GDALDataset(enhance=SCALE, transforms=RANDOM_ERASER_MULTI_REGION) on the two scenes
    tmp = tempfile.mkdtemp()
    for nm, (x, y) in scenes(rng).items():
        T.SCENES['x'], T.SCENES['y'] = x, y
        out['%s/x' % nm], out['%s/y' % nm] = x, y
        plain = RD.GDALDataset('x', 'y', patch_size=PATCH, overlap_padding=PAD)
        for i in range(len(plain)):                           # every tile keeps valid pixels
            assert (plain[i][0].sum(0) != 0).any()
        t1, t2 = os.path.join(tmp, nm + '_1.txt'), os.path.join(tmp, nm + '_2.txt')
        a1, a2 = RC.Dataset_maxmin(t1, t2, plain)
        out['%s/maxmin' % nm] = np.array([[[float(v) for v in r] for r in a] for a in (a1, a2)], np.float64)      # (2, 4, 2)
        out['%s/maxmin_txt1' % nm], out['%s/maxmin_txt2' % nm] = np.array(open(t1).read()), np.array(open(t2).read())
        b1, b2 = RC.Dataset_maxmin(t1, t2, plain)             # the second call reads the files
        assert np.array_equal(np.array(b1), out['%s/maxmin' % nm][0]) and np.array_equal(np.array(b2), out['%s/maxmin' % nm][1])
        r1, r2 = (out['%s/maxmin' % nm][k].tolist() for k in range(2))
        random.seed(ITEM_SEED)
        ds = RD.GDALDataset('x', 'y', enhance=RC.SCALE(r1, r2), transforms=RC.RANDOM_ERASER_MULTI_REGION(),
                            patch_size=PATCH, overlap_padding=PAD)
        for i in range(len(ds)):
            px, py, _, _ = ds[i]
            if i in ITEMS[nm]:
                out['%s/item%d/x' % (nm, i)], out['%s/item%d/y' % (nm, i)] = px.numpy(), py.numpy()
    out['meta'] = np.array([PATCH[0], PATCH[1], PAD[0], PAD[1], ITEM_SEED], np.int64)
    path = os.path.join(HERE, 'augment.npz')
    save(path, out)
    print('wrote augment.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
