"""Host side of the reference's other pre-processing (fcd_gan_pytorch_amd/transforms.py; tiles.PairTileDataset(enhance=,
transforms=); tiles.dataset_maxmin; _ops.erase_rects; the argument checks of fcd_scene_set_cut_aug / fcd_scene_minmax) against
what the reference wrote (tests/golden/augment.npz, gen_golden_augment.py).  Everything is compared bit for bit: the enhancers
are the same float64 expressions, the erasers the same calls to ``random`` in the same order.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import random
import types

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, datasets, tiles, transforms

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
NAMES = ['abudhabi', 'paris']
KEPT = {'abudhabi': [0, 8], 'paris': [0, 1, 2, 3, 4, 5]}
ERASERS = {'single': transforms.RANDOM_ERASER, 'multi': transforms.RANDOM_ERASER_MULTI_REGION}


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, 'augment.npz'))
    return {k: z[k] for k in z.files}


def geometry():
    pw, ph, padx, pady, seed = (int(v) for v in golden()['meta'])
    return (pw, ph), (padx, pady), seed


def enhancers():
    z = golden()
    stats, ranges = z['enh/stats'], z['enh/ranges']
    lists = [ranges[k].tolist() for k in range(2)]
    return {'normalize': transforms.NORMALIZE(*[s.tolist() for s in stats]), 'scale': transforms.SCALE(lists[0], lists[1]),
            'scale_norm': transforms.SCALE_NORM(lists[0], lists[1], [-1, 1]),
            'scale_norm_b': transforms.SCALE_NORM(lists[0], lists[1], [0.25, 3.0])}


def regions_of(cls, thresh):
    """The fixture's draws as the erasers return them: one 4-tuple per draw (single), one list of lists per draw (multi)."""
    z = golden()
    tag = 'erase/%s/%g' % (cls, thresh)
    rects, counts = z[tag + '/rects'].tolist(), z[tag + '/counts'].tolist()
    out, at = [], 0
    for c in counts:
        out.append(tuple(rects[at]) if cls == 'single' else rects[at:at + c])
        at += c
    assert at == len(rects)
    return out


# ------------------------------------------------------------------------------------------------- enhancers
@pytest.mark.parametrize('name', ['normalize', 'scale', 'scale_norm', 'scale_norm_b'])
def test_enhancers_equal_the_reference_bit_for_bit(name):
    z = golden()
    enh = enhancers()[name]
    assert enh.kind == {'normalize': 1, 'scale': 2}.get(name, 3)
    for switch in (1, 2):
        block = z['enh/block'].copy()
        got = enh(block, switch=switch)
        assert got is block                                                 # in place, and returned
        np.testing.assert_array_equal(got, z['enh/%s/%d' % (name, switch)])
        t = torch.from_numpy(z['enh/block'].copy())                         # tensors too
        np.testing.assert_array_equal(enh(t, switch=switch).numpy(), z['enh/%s/%d' % (name, switch)])
    p = enh.params(4)
    assert p.shape == (4, 4) and p.dtype == np.float64
    if name == 'normalize':
        np.testing.assert_array_equal(p, z['enh/stats'])
    else:
        np.testing.assert_array_equal(p, z['enh/ranges'].transpose(0, 2, 1).reshape(4, 4))     # loX, hiX, loY, hiY
    np.testing.assert_array_equal(enh.params(2), p[:, :2])
    with pytest.raises(ValueError, match="The input channel doesn't match the"):
        enh.params(5)


def test_more_bands_than_entries_raises_the_reference_message():
    five = np.zeros((5, 2, 2))
    e = enhancers()
    for switch in (1, 2):
        with pytest.raises(ValueError, match="The input channel doesn't match the stats list"):
            e['normalize'](five.copy(), switch=switch)
    for name in ('scale', 'scale_norm'):
        with pytest.raises(ValueError, match="The input channel doesn't match the range list"):
            e[name](five.copy(), switch=1)
        with pytest.raises(ValueError, match="The input channel doesn't match the scale list"):
            e[name](five.copy(), switch=2)
    with pytest.raises(ValueError):
        transforms.enhancer('gamma', None, None)


# ------------------------------------------------------------------------------------------------- erasers
@pytest.mark.parametrize('thresh', [0.3, 0.01])
@pytest.mark.parametrize('cls', ['single', 'multi'])
def test_eraser_draws_equal_the_reference(cls, thresh):
    z = golden()
    seed, draws = (int(v) for v in z['erase/meta'])
    want = regions_of(cls, thresh)
    images = z['erase/%s/%g/images' % (cls, thresh)]
    assert len(want) == draws == 60
    # the module-level random, like the reference
    random.seed(seed)
    t = ERASERS[cls](erase_thresh=thresh)
    got = []
    for k in range(draws):
        img, region = t(torch.from_numpy(z['erase/image'].copy()))
        got.append(region)
        if k < 5:
            np.testing.assert_array_equal(img.numpy(), images[k])
            again, same = t(torch.from_numpy(z['erase/image'].copy()), region)          # the paired call: no draw, same region
            assert same is region
            np.testing.assert_array_equal(again.numpy(), images[k])
    assert got == want
    # an rng= instance gives the module's sequence for the same seed, and draw() alone is forward() without the image
    t = ERASERS[cls](erase_thresh=thresh, rng=random.Random(seed))
    state = random.getstate()
    assert [t.draw((3, 32, 40)) for _ in range(draws)] == want
    assert random.getstate() == state                                       # the module's generator was not touched
    assert t.max_regions == (1 if cls == 'single' else 5)
    if thresh == 0.01:                                                      # the clamp reaches h == 0; such a rectangle erases nothing
        flat = z['erase/%s/%g/rects' % (cls, thresh)]
        assert ((flat[:, 3] == 0) & (flat[:, 2] > 0)).any()
    if cls == 'single':
        assert (0, 0, 0, 0) in want                                         # a kept image
    else:
        assert [] in want
    assert transforms.RANDOM_ERASER_MULTI_REGION(multi_region=0).max_regions == 1


# ------------------------------------------------------------------------------------------------- datasets
@pytest.mark.parametrize('nm', NAMES)
def test_pair_tile_dataset_with_both_hooks_equals_the_reference_items(nm):
    z = golden()
    patch, pad, seed = geometry()
    r1, r2 = (z['%s/maxmin' % nm][k].tolist() for k in range(2))
    for make in (tiles.PairTileDataset, datasets.RegionTileDataset):
        random.seed(seed)
        ds = make(z['%s/x' % nm], z['%s/y' % nm], patch_size=patch, overlap_padding=pad, enhance=transforms.SCALE(r1, r2),
                  transforms=transforms.RANDOM_ERASER_MULTI_REGION())
        for i in range(len(ds)):                                            # every item draws, in order
            item = ds[i]
            if i in KEPT[nm]:
                np.testing.assert_array_equal(item[0].numpy(), z['%s/item%d/x' % (nm, i)])
                np.testing.assert_array_equal(item[1].numpy(), z['%s/item%d/y' % (nm, i)])
            assert item[0].dtype == torch.float32 and not item[3].any()     # ref untouched (there is none)
    erased = sum(int((z['%s/item%d/x' % (nm, i)] == 0).sum()) for i in KEPT[nm])
    assert erased > 0


def test_hooks_that_exclude_each_other():
    z = golden()
    patch, pad, _ = geometry()
    x, y = z['paris/x'], z['paris/y']
    stats = tuple(z['enh/stats'])
    with pytest.raises(ValueError, match='not both'):
        tiles.PairTileDataset(x, y, None, patch, pad, stats=stats, enhance=enhancers()['scale'])
    with pytest.raises(ValueError, match='not both'):
        datasets.RegionTileDataset(x, y, patch_size=patch, overlap_padding=pad, stats=stats, enhance=enhancers()['scale'])
    ds = tiles.PairTileDataset(x, y, None, patch, pad, stats=stats, transforms=transforms.RANDOM_ERASER())
    with pytest.raises(ValueError, match='raw'):
        ds.raw_item(0)
    assert len(tiles.PairTileDataset(x, y, None, patch, pad, stats=stats).raw_item(0)) == 5     # without transforms: as before
    # NORMALIZE as an enhancer is the stats route
    a = tiles.PairTileDataset(x, y, None, patch, pad, stats=stats)
    b = tiles.PairTileDataset(x, y, None, patch, pad, enhance=transforms.NORMALIZE(*stats))
    for i in range(len(a)):
        assert torch.equal(a[i][0], b[i][0]) and torch.equal(a[i][1], b[i][1])


# ------------------------------------------------------------------------------------------------- max / min
@pytest.mark.parametrize('nm', NAMES)
def test_dataset_maxmin_equals_the_reference(nm, tmp_path):
    z = golden()
    patch, pad, _ = geometry()
    ds = tiles.PairTileDataset(z['%s/x' % nm], z['%s/y' % nm], None, patch, pad)
    t1, t2 = str(tmp_path / 'a.txt'), str(tmp_path / 'b.txt')
    a1, a2 = tiles.dataset_maxmin(t1, t2, ds)
    assert isinstance(a1, list) and all(isinstance(v, float) for r in a1 + a2 for v in r)
    np.testing.assert_array_equal(np.array([a1, a2]), z['%s/maxmin' % nm])
    assert open(t1).read() == str(z['%s/maxmin_txt1' % nm]) and open(t2).read() == str(z['%s/maxmin_txt2' % nm])
    assert tiles.dataset_maxmin(t1, t2, None) == (a1, a2)                   # round trip of its own text: the files are read
    # the text the reference wrote
    u1, u2 = str(tmp_path / 'r1.txt'), str(tmp_path / 'r2.txt')
    open(u1, 'w').write(str(z['%s/maxmin_txt1' % nm]))
    open(u2, 'w').write(str(z['%s/maxmin_txt2' % nm]))
    b1, b2 = tiles.dataset_maxmin(u1, u2, None)
    np.testing.assert_array_equal(np.array([b1, b2]), z['%s/maxmin' % nm])
    # the y extremes inside the block that x masks out did not get in
    assert z['%s/y' % nm].max() == 65535 and z['%s/y' % nm].min() == 0 and np.array(a2).max() < 4000 and np.array(a2).min() >= 1
    # scene_maxmin shares the cache: it reads these files, and what it writes (repr) loads in dataset_maxmin
    assert tiles.scene_maxmin(t1, t2, None) == (a1, a2)
    vals = ([[1 / 3, 2.5e-7], [-7.0, 1e300]], [[5e-324, 0.1], [3.0, 4.0]])
    scene = types.SimpleNamespace(maxmin=lambda overlap_padding=(0, 0): vals)
    s1, s2 = str(tmp_path / 's1.txt'), str(tmp_path / 's2.txt')
    assert tiles.scene_maxmin(s1, s2, scene) == vals
    assert open(s1).read().startswith('max: ') and open(s1).read().splitlines()[1].startswith('min: ')
    assert tiles.scene_maxmin(s1, s2, None) == vals and tiles.dataset_maxmin(s1, s2, None) == vals


def test_dataset_maxmin_keeps_the_reference_quirks(tmp_path):
    patch, pad = (8, 8), (0, 0)
    x = np.empty((2, 8, 16), np.float32)
    x[0], x[1] = 5.0, -6.0                        # band sums of -1: every pixel valid; band 1 all negative
    x[0, 0, 0], x[1, 0, 0] = 0.0, -9.0            # a valid pixel with a 0 sample in band 0 of the first tile
    x[0, :, 8:] = 7.0                             # the second tile
    got, _ = tiles.dataset_maxmin(str(tmp_path / 'a'), str(tmp_path / 'b'), tiles.PairTileDataset(x, x, None, patch, pad))
    assert got[0] == [7.0, 7.0]                   # the first tile's minimum 0 reads as "unset": the second tile's 7 replaces it
    assert got[1] == [-9.0, 0.0]                  # the maximum started at 0
    empty = np.zeros((1, 8, 8), np.float32)
    with pytest.raises(Exception):                # a tile without a valid pixel: the reference raises too
        tiles.dataset_maxmin(str(tmp_path / 'c'), str(tmp_path / 'd'), tiles.PairTileDataset(empty, empty, None, patch, pad))


# ------------------------------------------------------------------------------------------------- erase_rects
def test_erase_rects_validation():
    patch = (40, 32)
    single, multi = regions_of('single', 0.01), regions_of('multi', 0.3)
    r = ops.erase_rects(single[:10], 10, 1, patch)
    assert r.rows.shape == (10, 1, 4) and r.rows.dtype == np.int32 and r.R == 1 and len(r) == 10 and r.dev is None
    np.testing.assert_array_equal(r.rows[:, 0], np.array(single[:10]))
    m = ops.erase_rects(multi[:10] + [None], 11, 5, patch)
    assert m.rows.shape == (11, 5, 4) and not m.rows[10].any()
    for t, reg in enumerate(multi[:10]):
        np.testing.assert_array_equal(m.rows[t, :len(reg)], np.array(reg, np.int32).reshape(-1, 4))
        assert not m.rows[t, len(reg):].any()                               # unused slots are empty
    part = m[2:5]
    assert isinstance(part, ops.EraseRects) and len(part) == 3 and part.patch == patch
    np.testing.assert_array_equal(part.rows, m.rows[2:5])
    with pytest.raises(TypeError):
        m[::2]
    ops.erase_rects([(0, 0, 40, 32)], 1, 1, patch)                          # the whole tile
    ops.erase_rects([[[39, 31, 1, 1]] * 16], 1, 16, patch)                  # 16, ending exactly on the edge
    bad = {'past the right edge': [(1, 0, 40, 1)], 'past the bottom edge': [(0, 31, 1, 2)], 'a negative x': [(-1, 0, 2, 2)],
           'a negative h': [(0, 0, 2, -1)], 'a huge w': [(1, 0, 2 ** 31, 1)]}
    for what, reg in bad.items():
        with pytest.raises(_lib.FcdError, match='negative entry or leaves'):
            ops.erase_rects(reg, 1, 1, patch)
    with pytest.raises(_lib.FcdError, match='at most 16'):
        ops.erase_rects([[[0, 0, 1, 1]] * 17], 1, 17, patch)
    with pytest.raises(_lib.FcdError, match='17 rectangles'):
        ops.erase_rects([[[0, 0, 1, 1]] * 17], 1, 16, patch)
    with pytest.raises(_lib.FcdError, match='2 regions for 3 tiles'):
        ops.erase_rects(single[:2], 3, 1, patch)
    with pytest.raises(_lib.FcdError, match='four integers'):
        ops.erase_rects([[(0, 0, 1.5, 1)]], 1, 1, patch)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.erase_rects(single[:2], 2, 1, patch, device='cpu')


# ------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_validate_their_arguments_without_launching():
    lib = _lib.lib
    a = ctypes.c_void_p(4096)        # a non-null address that is never dereferenced: every call below fails its checks first
    err = lambda: lib.fcd_last_error_string()

    def cut(mode=2, erase=None, R=0, st=1, descs=a, n=3):
        return lib.fcd_scene_set_cut_aug(descs, 2, st, 4, a, 15, a, n, 32, 40, None, mode, -1.0, 1.0, erase, R, a, a, None, None,
                                         None, None)
    assert cut(descs=None) == -1 and b'fcd_scene_set_cut_aug: bad arguments' in err()
    for mode in (-1, 4):
        assert cut(mode=mode) == -1 and b'enhancement mode' in err()
    assert cut(erase=a, R=17) == -1 and b'at most 16' in err()
    assert cut(erase=a, R=-1) == -1 and b'at most 16' in err()
    assert cut(erase=None, R=3) == -1 and b'rectangle list' in err()
    assert cut(erase=a, R=0) == -1 and b'rectangle list' in err()
    assert cut(st=5) == -1 and b'sample type 5' in err()
    assert cut(n=2 ** 30) == -1 and b'exceed 2^31 - 1' in err()

    def minmax(x=a, st=1, C=4, n=2, out=a, count=a, ws=a, wsb=1 << 20):
        return lib.fcd_scene_minmax(x, a, st, C, 64, 64, a, n, 32, 32, out, count, ws, wsb, None)
    assert minmax(x=None) == -1 and b'fcd_scene_minmax: bad arguments' in err()
    assert minmax(count=None) == -1 and minmax(n=0) == -1
    assert minmax(st=3) == -1 and b'sample type 3' in err()
    assert minmax(C=33) == -1 and b'at most 32' in err()
    need = lib.fcd_scene_minmax_ws_bytes(4, 2, 32)
    assert need > 0 and need % (4 * 4 * 4 + 8) == 0                         # whole partial rows: 4*C floats and a 64-bit count
    assert lib.fcd_scene_minmax_ws_bytes(33, 2, 32) == 0 and lib.fcd_scene_minmax_ws_bytes(4, 0, 32) == 0
    assert minmax(ws=None, wsb=0) == -1 and b'workspace' in err()
    assert minmax(wsb=need - 1) == -1 and b'workspace' in err()
    assert ops.ERASE_MAX == 16
