"""The reference's other pre-processing on the device-resident feed (csrc/scene.hip: fcd_scene_set_cut_aug, fcd_scene_minmax;
tiles.ResidentScene(enhance=) / maxmin, tiles.ResidentSceneSet(transforms=), demos.demo_usss(enhance=, transforms=)) against the
host route it stands in for -- ``RegionTileDataset(enhance=, transforms=)`` / ``MultiSceneDataset`` / ``demos._Epoch`` /
``tiles.dataset_maxmin`` -- and against what the reference wrote (tests/golden/augment.npz).

Everything is compared BIT-EXACT: the enhancement is the host's float64 expression evaluated per sample with true divisions,
erasing is an assignment of +0, the extrema are samples of the scene."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, datasets, demos, dp, tiles, transforms
from test_transforms_host import ERASERS, golden, regions_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
NAMES = ['abudhabi', 'paris']
PATCH, PAD = (40, 32), (4, 3)
MIXED = [0, 9, 3, 14, 3, 10, 8, 9, 0, 12, 5, 11, 5]            # alternates between the two scenes, with repeats


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def _np(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _arrays(nm, dtype='uint16'):
    """The fixture scene pair ``nm`` (+ a made-up reference and region map) as uint16, uint8 or float32 samples."""
    z = golden()
    x, y = z['%s/x' % nm], z['%s/y' % nm]
    if dtype == 'uint8':
        x, y = (x % 251).astype(np.uint8), (y % 251).astype(np.uint8)
    elif dtype == 'float32':
        x, y = (x.astype(np.float32) / 7).astype(np.float32), (y.astype(np.float32) / 3).astype(np.float32)
    rng = np.random.default_rng(len(nm))
    ref = rng.integers(1, 3, (1,) + x.shape[1:]).astype(np.uint8)
    region = (rng.integers(0, 2, (1,) + x.shape[1:]) * 255).astype(np.uint8)
    return x, y, ref, region


def _enhancer(mode, k, dtype='uint16'):
    """A made-up enhancer of kind ``mode`` for scene ``k`` (per-scene parameters; SCALE_NORM: one range for the set)."""
    rng = np.random.default_rng(100 * mode + k)
    top = {'uint16': 4000.0, 'uint8': 250.0, 'float32': 1300.0}[dtype]
    if mode == 0:
        return None
    if mode == 1:
        return transforms.NORMALIZE(*[rng.uniform(0.2 * top, 0.7 * top, 4).tolist() for _ in range(4)])
    r1, r2 = ([[float(lo), float(hi)] for lo, hi in zip(rng.uniform(0, 0.05 * top, 4), rng.uniform(0.8 * top, top, 4))] for _ in range(2))
    return transforms.SCALE(r1, r2) if mode == 2 else transforms.SCALE_NORM(r1, r2, [0.25, 3.0])


@functools.lru_cache(maxsize=None)
def _scenes(modes=(1, 1), dtype='uint16'):
    """The two fixture scenes as ResidentScenes with enhancers of the given kinds (0: none); shared, never modified."""
    out = []
    for k, nm in enumerate(NAMES):
        x, y, ref, region = _arrays(nm, dtype)
        out.append(tiles.ResidentScene(x, y, ref, PATCH, PAD, device=DEV, region=region, enhance=_enhancer(modes[k], k, dtype)))
    return tuple(out)


def _host(modes=(1, 1), dtype='uint16', erasers=None):
    ds = []
    for k, nm in enumerate(NAMES):
        x, y, ref, region = _arrays(nm, dtype)
        ds.append(datasets.RegionTileDataset(x, y, region=region, ref=ref, patch_size=PATCH, overlap_padding=PAD,
                                             enhance=_enhancer(modes[k], k, dtype), transforms=erasers[k] if erasers else None))
    return datasets.MultiSceneDataset(ds, NAMES)


def _host_items(ds, items):
    got = [ds[int(i)] for i in items]
    return tuple(np.stack([g[k].numpy() for g in got]) for k in (0, 1, 3, 4))


def _erased(base, regions):
    """NumPy truth: the (n,C,ph,pw) tiles ``base`` with the regions of every tile assigned +0."""
    out = base.copy()
    for t, reg in enumerate(regions):
        if reg is None:
            continue
        reg = [reg] if len(reg) == 4 and not hasattr(reg[0], '__len__') else reg
        for x, y, w, h in reg:
            out[t, :, y:y + h, x:x + w] = 0.0
    return out


# ============================================================================================= 1. enhancement
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32'])
@pytest.mark.parametrize('mode', [1, 2, 3])
def test_set_cut_modes_equal_the_host_datasets(mode, dtype):
    host, res = _host((mode, mode), dtype), tiles.ResidentSceneSet(_scenes((mode, mode), dtype), NAMES)
    assert res.mode == mode and (mode != 3 or res.scale == (0.25, 3.0))
    for items in (list(range(15)), MIXED):
        hx, hy, hr, hg = _host_items(host, items)
        for erase in (None, [None] * len(items)):              # the second: fcd_scene_set_cut_aug with empty lists, mode 1 too
            gx, gy, gr, gg, gv = _np(res.cut(items, erase=erase))
            assert _bits(gx).tobytes() == _bits(hx).tobytes(), 'x, mode %d, %s' % (mode, dtype)
            assert _bits(gy).tobytes() == _bits(hy).tobytes(), 'y, mode %d, %s' % (mode, dtype)
            _eq(gr, hr, 'ref'); _eq(gg, hg, 'region')
    rx, ry, _, _ = _host_items(_host((0, 0), dtype), MIXED)
    raw = _np(res.cut(MIXED, raw=True))
    _eq(raw[0], rx, 'raw x'); _eq(raw[1], ry, 'raw y')
    # one scene cut on its own honours its enhancer too (what infer_scene_resident does)
    scene = res.scenes[1]
    sx, sy, sr, sv = _np(scene.cut(range(len(scene))))
    hx, hy, hr, _ = _host_items(host, range(9, 15))
    _eq(sx, hx, 'single-scene x'); _eq(sy, hy, 'single-scene y'); _eq(sr, hr, 'single-scene ref')
    assert sv.shape == (6, 1, 32, 40) and set(np.unique(sv)) == {0.0, 1.0}
    px, py, _, _ = _np(scene.cut(range(len(scene)), raw=True))
    _eq(px, _host_items(_host((0, 0), dtype), range(9, 15))[0], 'single-scene raw x')


def test_a_scene_without_enhancer_stays_raw_and_kinds_do_not_mix():
    res = tiles.ResidentSceneSet(_scenes((2, 0)), NAMES)
    assert res.mode == 2
    gx, gy, _, _, _ = _np(res.cut(range(15)))
    hx, hy, _, _ = _host_items(_host((2, 0)), range(15))
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y')
    _eq(gx[9:], _host_items(_host((0, 0)), range(9, 15))[0], 'the scene without an enhancer: plain samples')
    assert gx[:9].max() <= 1.5 and gx[9:].max() > 1000
    with pytest.raises(_lib.FcdError, match='enhancer kind'):
        tiles.ResidentSceneSet(_scenes((2, 1)), NAMES)
    a, b = _scenes((3, 3))
    x, y, ref, region = _arrays('paris')
    other = transforms.SCALE_NORM(b.enhance.scale_list1, b.enhance.scale_list2, [-1, 1])
    with pytest.raises(_lib.FcdError, match='enhancer kind'):
        tiles.ResidentSceneSet([a, tiles.ResidentScene(x, y, ref, PATCH, PAD, device=DEV, enhance=other)])
    with pytest.raises(ValueError, match='not both'):
        tiles.ResidentScene(x, y, ref, PATCH, PAD, device=DEV, stats=tuple(np.ones((4, 4))), enhance=other)
    # set_stats stays and means NORMALIZE; set_enhance replaces it
    s = tiles.ResidentScene(x, y, ref, PATCH, PAD, device=DEV, stats=tuple(np.ones((4, 4))))
    assert s.enhance_kind == 1
    s.set_enhance(other)
    assert s.enhance_kind == 3 and s.stats is None and s.enhance_scale == (-1.0, 1.0)
    s.set_enhance(None)
    assert s.enhance_kind == 0 and s._stats_dev is None
    with pytest.raises(_lib.FcdError, match='mode'):
        ops.scene_set_cut(res._descs, res.table, res.index([0]), 4, res.sample_type, mode=4)


# ============================================================================================= 2. erasing
@pytest.mark.parametrize('thresh', [0.3, 0.01])
@pytest.mark.parametrize('cls', ['single', 'multi'])
def test_device_erasing_equals_the_host_eraser(cls, thresh):
    host = _host(erasers=[ERASERS[cls](erase_thresh=thresh, rng=random.Random(7 + k)) for k in range(2)])
    res = tiles.ResidentSceneSet(_scenes(), NAMES,
                                 transforms=[ERASERS[cls](erase_thresh=thresh, rng=random.Random(7 + k)) for k in range(2)])
    hx, hy, hr, hg = _host_items(host, range(15))              # the host draws item by item, in order
    (batch, real, w), = list(res.epoch(15, 0, shuffle=False))  # one batch = the items in order: the same draws
    gx, gy, gitem, gr, gg = batch
    assert gitem.tolist() == list(range(15)) and real == 15
    _eq(gx.cpu().numpy(), hx, 'x'); _eq(gy.cpu().numpy(), hy, 'y'); _eq(gr.cpu().numpy(), hr, 'ref'); _eq(gg.cpu().numpy(), hg, 'region')
    plain = _host_items(_host(), range(15))[0]
    assert (hx != plain).any(), 'nothing was erased: the comparison shows nothing'


HAND = [
    [(0, 0, 40, 32)],                                          # the whole tile
    [[0, 0, 1, 1], [39, 0, 1, 1], [0, 31, 1, 1], [39, 31, 1, 1]],      # a 1x1 at each corner
    [[5, 5, 20, 10], [15, 10, 20, 15]],                        # two overlapping
    [[3, 3, 0, 5], [3, 3, 5, 0]],                              # w == 0 and h == 0: empty slots
    [[30, 20, 10, 12]],                                        # ends exactly on the tile's right and bottom edge
    [[2 * k, k, 3, 2] for k in range(16)],                     # 16 in one tile
    None,
]


def test_hand_made_regions():
    res = tiles.ResidentSceneSet(_scenes(), NAMES)
    items = MIXED[:len(HAND)]
    base = _np(res.cut(items))
    got = _np(res.cut(items, erase=HAND))
    for k, what in ((0, 'x'), (1, 'y')):
        want = _erased(base[k], HAND)
        _eq(got[k], want, what)                                # inside: zeros; outside: the un-erased cut
        assert not _bits(got[k])[want == 0].any(), 'a zero that is not +0.0'
    for k, what in ((2, 'ref'), (3, 'region'), (4, 'valid')):
        _eq(got[k], base[k], what + ' is never erased')
    assert not got[0][0].any() and not got[1][0].any()
    _eq(got[0][3], base[0][3], 'empty slots erase nothing')
    assert (got[0][5] == 0).sum() > (base[0][5] == 0).sum()
    rects = res.erase_rects(HAND, len(HAND))
    assert rects.R == 16 and torch.equal(res.cut(items, erase=rects)[0], res.cut(items, erase=HAND)[0])
    with pytest.raises(_lib.FcdError, match='EraseRects of these'):
        res.cut(items[:3], erase=rects)
    with pytest.raises(_lib.FcdError, match='leaves'):
        res.cut([0], erase=[(1, 0, 40, 1)])
    with pytest.raises(ValueError, match='raw'):
        res.cut([0], raw=True, erase=[None])


def test_erasing_assigns_plus_zero_over_nan_and_inf():
    x, y, ref, region = _arrays('paris', 'float32')
    x, y = x.copy(), y.copy()
    x[0, 5, 6], x[1, 5, 7], x[2, 6, 6], x[3, 6, 7] = np.nan, np.inf, -np.inf, -0.0
    y[0, 5, 6], y[1, 6, 6] = -np.inf, np.nan
    for enh in (None, _enhancer(1, 1, 'float32'), transforms.SCALE([[100.0, 50.0]] * 4, [[100.0, 50.0]] * 4)):
        res = tiles.ResidentSceneSet([tiles.ResidentScene(x, y, None, PATCH, PAD, device=DEV, enhance=enh)])
        bx, by, _, _, _ = _np(res.cut([0]))
        assert np.isnan(bx[0, 0, 5 + 3, 6 + 4]) and np.isinf(bx[0, 1, 5 + 3, 7 + 4])      # tile 0 sits at (4, 3) in its canvas
        gx, gy, _, _, _ = _np(res.cut([0], erase=[[[9, 7, 4, 4]]]))
        for g, b in ((gx, bx), (gy, by)):
            assert not _bits(g[0, :, 7:11, 9:13]).any(), 'not +0.0 (NaN, inf or a set sign bit) under the rectangle'
            keep = np.ones(g.shape, bool)
            keep[0, :, 7:11, 9:13] = False
            assert _bits(g)[keep].tobytes() == _bits(b)[keep].tobytes()
    # the inverted SCALE range makes negative results: an erased -x is +0 all the same, and the un-erased cut has its sign
    assert (bx[0, :, 7:11, 9:13] < 0).any()


def test_a_tile_wider_than_one_wave_trip():
    x, y, ref, region = _arrays('abudhabi')
    patch, pad = (70, 9), (0, 0)
    enh = _enhancer(2, 0)
    res = tiles.ResidentSceneSet([tiles.ResidentScene(x, y, ref, patch, pad, device=DEV, enhance=enh)])
    host = datasets.RegionTileDataset(x, y, ref=ref, patch_size=patch, overlap_padding=pad, enhance=enh)
    n = len(res)
    assert n == 16
    regions = [[[60, 2, 10, 5], [66, 0, 4, 9], [0, 8, 64, 1]] if t % 2 == 0 else [(63, 0, 2, 9)] for t in range(n)]
    hx = np.stack([host[i][0].numpy() for i in range(n)])
    hy = np.stack([host[i][1].numpy() for i in range(n)])
    gx, gy, gr, _, gv = _np(res.cut(range(n), erase=regions))
    _eq(gx, _erased(hx, regions), 'x'); _eq(gy, _erased(hy, regions), 'y')
    _eq(gr, np.stack([host[i][3].numpy() for i in range(n)]), 'ref')
    assert (gx[0, :, 2:7, 64:70] == 0).all() and (hx[0, :, 2:7, 64:70] != 0).all()


def test_erasing_with_more_planes_than_the_grid_holds():
    res = tiles.ResidentSceneSet(_scenes(), NAMES)
    reps = 400
    items = list(range(15)) * reps
    assert len(items) * (2 * 4 + 3) > 65535
    one = [[[t, t, 20, 10], [39 - t, 31 - t, 1, 1]] for t in range(15)]
    x, y, r, g, v = res.cut(items, erase=res.erase_rects(one * reps, len(items)))
    base = _np(res.cut(range(15)))
    for t, h, what in ((x, _erased(base[0], one), 'x'), (y, _erased(base[1], one), 'y'), (r, base[2], 'ref'), (g, base[3], 'region'),
                       (v, base[4], 'valid')):
        t = t.view((reps, 15) + t.shape[1:])
        assert torch.equal(t, torch.from_numpy(h).to(DEV)[None].expand_as(t)), what


# ============================================================================================= 3. the epoch feed
def _host_epoch(ds, batch, seed, ragged, rank, world):
    ep = demos._Epoch(ds, batch, seed, DEV, ragged=ragged)
    ep.sampler = dp.RankStridedBatches(len(ds), batch, seed=seed, rank=rank, world=world, ragged=ragged)
    return ep


@pytest.mark.parametrize('rank,world', [(0, 1), (1, 2)])
def test_two_epochs_with_transforms_equal_the_host_epochs(rank, world):
    make = lambda: [transforms.RANDOM_ERASER_MULTI_REGION(rng=random.Random(21)), transforms.RANDOM_ERASER(rng=random.Random(22))]
    host = _host(erasers=make())
    res = tiles.ResidentSceneSet(_scenes(), NAMES, transforms=make())
    erased = 0
    for seed in (5, 6):                                        # consecutive epochs: the generators run on
        want = list(_host_epoch(host, 4, seed, 'pad', rank, world))
        got = list(res.epoch(4, seed, ragged='pad', rank=rank, world=world))
        assert len(got) == len(want) > 0
        for b, ((gb, greal, gw), (hb, hreal, hw)) in enumerate(zip(got, want)):
            assert torch.equal(gb[2], hb[2].cpu()) and greal == hreal and float(gw) == float(hw)
            for k, what in ((0, 'x'), (1, 'y'), (3, 'ref'), (4, 'region')):
                _eq(gb[k].cpu().numpy(), hb[k].cpu().numpy(), '%s of batch %d, epoch seed %d' % (what, b, seed))
            erased += int((gb[0] == 0).sum())
    assert erased > 0


def test_epoch_with_transforms_makes_one_region_upload_and_no_host_wait(monkeypatch):
    res = tiles.ResidentSceneSet(_scenes(), NAMES, transforms=transforms.RANDOM_ERASER_MULTI_REGION(rng=random.Random(3)))
    res.cut([0])                                               # the set's tables go up once per set, not per epoch: before the watch
    index_uploads, rect_uploads, cuts = [], [], []
    init, to, cut = ops.TileIndex.__init__, ops.EraseRects.to, ops.scene_set_cut

    def counting_init(self, items, size, device=None, _view=None):
        if _view is None:
            index_uploads.append(len(items))
        init(self, items, size, device, _view)

    def counting_to(self, device):
        if self.dev is None and self.R > 0:
            rect_uploads.append(len(self))
        return to(self, device)

    def watching_cut(descs, table, index, *a, **k):
        cuts.append((index, k.get('erase')))
        return cut(descs, table, index, *a, **k)
    monkeypatch.setattr(ops.TileIndex, '__init__', counting_init)
    monkeypatch.setattr(ops.EraseRects, 'to', counting_to)
    monkeypatch.setattr(ops, 'scene_set_cut', watching_cut)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):                      # the control: the mode is live on this build
            torch.zeros(4).to(DEV)
        seen = 0
        for (x, y, item, r, g), real, w in res.epoch(4, 5):    # iterate and cut only; nothing may raise
            seen += x.shape[0]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    plan = tiles.EpochPlan(15, 4, 5)
    assert seen == len(plan.flat) == 15
    assert index_uploads == [15] and rect_uploads == [15]      # ONE index upload and ONE region upload for the epoch
    assert len(cuts) == len(plan) == 4
    ibase, rbase = cuts[0][0].dev, cuts[0][1].dev
    assert rbase.is_cuda and rbase.dtype == torch.int32 and tuple(rbase.shape[1:]) == (5, 4)
    for b, (idx, rects) in enumerate(cuts):                    # every batch: device slices of those two uploads
        assert isinstance(rects, ops.EraseRects) and len(rects) == len(idx) == len(plan.batches[b])
        assert idx.dev.data_ptr() == ibase.data_ptr() + 4 * plan.offsets[b]
        assert rects.dev.data_ptr() == rbase.data_ptr() + 4 * 4 * 5 * plan.offsets[b]


# ============================================================================================= 4. min / max
def _truth_maxmin(x, y, patch, pad):
    """NumPy truth: per band [min, max] of x and of y over the pixels some tile reads whose fp32 band sum of x (in band order) is
    non-zero; NaN samples skipped; + the valid count with pixels counted once per tile that reads them."""
    C, H, W = x.shape
    grid = tiles.TileGrid(W, H, patch, pad)
    s = np.zeros((H, W), np.float32)
    with np.errstate(invalid='ignore'):
        for c in range(C):
            s = (s + x[c].astype(np.float32)).astype(np.float32)
    mask = s != 0
    seen, n = np.zeros((H, W), bool), 0
    for item in range(len(grid)):
        _, (rx, ry, rw, rh), _ = grid.slices(item)
        m = mask[ry:ry + rh, rx:rx + rw]
        n += int(m.sum())
        seen[ry:ry + rh, rx:rx + rw] |= m
    out = []
    for a in (x, y):
        rows = []
        for c in range(C):
            v = a[c][seen].astype(np.float64)
            v = v[~np.isnan(v)]
            rows.append([float(v.min()), float(v.max())] if v.size else [float('inf'), float('-inf')])
        out.append(rows)
    return out[0], out[1], n


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32'])
@pytest.mark.parametrize('nm', NAMES)
def test_device_maxmin_equals_the_numpy_truth_and_the_reference(nm, dtype, tmp_path):
    x, y, _, _ = _arrays(nm, dtype)
    scene = tiles.ResidentScene(x, y, None, PATCH, PAD, device=DEV)
    for pad in ((0, 0), PAD):
        w1, w2, n = _truth_maxmin(x, y, PATCH, pad)
        g1, g2 = scene.maxmin(pad)
        assert g1 == w1 and g2 == w2 and scene.stats_count == n
        assert all(isinstance(v, float) for r in g1 + g2 for v in r)
    if dtype == 'uint16':                                       # the fixture scenes: what the reference's Dataset_maxmin returned
        z = golden()
        _eq(np.array(scene.maxmin()), z['%s/maxmin' % nm], 'device extrema vs the reference-written fixture')
        assert y.max() == 65535 and y.min() == 0 and np.array(g2).max() < 4000 and np.array(g2).min() >= 1   # y under the x mask
        ds = tiles.PairTileDataset(x, y, None, PATCH, PAD)
        t1, t2 = str(tmp_path / 'a.txt'), str(tmp_path / 'b.txt')
        host = tiles.dataset_maxmin(t1, t2, ds)
        assert tiles.scene_maxmin(t1, t2, None) == host == (g1, g2)          # files of dataset_maxmin load in scene_maxmin
        s1, s2 = str(tmp_path / 's1.txt'), str(tmp_path / 's2.txt')
        first = tiles.scene_maxmin(s1, s2, scene)
        assert first == (g1, g2) and tiles.scene_maxmin(s1, s2, None) == first == tiles.dataset_maxmin(s1, s2, None)


def test_maxmin_edge_values():
    rng = np.random.default_rng(9)
    x = rng.uniform(-50, 50, (3, 64, 80)).astype(np.float32)
    y = rng.uniform(-50, 50, (3, 64, 80)).astype(np.float32)
    x[1] = -np.abs(x[1]) - 1                                    # an all-negative band: its true (negative) maximum comes back
    x[:, :32, :40] = 0                                          # tile 0 of the (40, 32) tiling without a valid pixel: skipped
    y[:, 3, 3] = 1e6                                            # a y extreme under the x mask: ignored
    x[0, 40, 50], x[2, 41, 50] = np.inf, -np.inf                # +-inf take part
    y[0, 42, 50] = np.nan                                       # NaN is skipped; the pixel still counts as valid
    x[2, 50, 60] = np.nan                                       # a NaN in x: the band sum is NaN != 0, valid; the sample is skipped
    scene = tiles.ResidentScene(x, y, None, (40, 32), (0, 0), device=DEV)
    g1, g2 = scene.maxmin()
    w1, w2, n = _truth_maxmin(x, y, (40, 32), (0, 0))
    assert g1 == w1 and g2 == w2 and scene.stats_count == n == 64 * 80 - 32 * 40
    assert g1[0][1] == float('inf') and g1[2][0] == float('-inf') and g1[1][1] < 0
    assert max(r[1] for r in g2) < 1e6 and not any(np.isnan(v) for r in g1 + g2 for v in r)
    again = scene.maxmin()
    assert again == (g1, g2)
    empty = tiles.ResidentScene(np.zeros((1, 8, 8), np.uint8), np.ones((1, 8, 8), np.uint8), None, (8, 8), (0, 0), device=DEV)
    with pytest.raises(_lib.FcdError, match='no valid pixel'):
        empty.maxmin()


@pytest.mark.parametrize('dtype', [np.uint16, np.float32])
def test_maxmin_across_the_4096_column_segment(dtype):
    rng = np.random.default_rng(4)
    x = rng.integers(100, 200, (2, 2, 4100)).astype(dtype)
    y = rng.integers(100, 200, (2, 2, 4100)).astype(dtype)
    x[0, 1, 4098], x[1, 0, 4097], y[1, 1, 4099], y[0, 0, 4096] = 7, 900, 3, 950            # extrema behind column 4096
    x[:, 0, 4099] = 0                                                                       # an invalid pixel there ...
    y[0, 0, 4099] = 1                                                                       # ... hides this minimum
    scene = tiles.ResidentScene(x, y, None, (4100, 2), (0, 0), device=DEV)
    assert len(scene) == 1
    g1, g2 = scene.maxmin()
    w1, w2, n = _truth_maxmin(x, y, (4100, 2), (0, 0))
    assert g1 == w1 and g2 == w2 and scene.stats_count == n == 2 * 4100 - 1
    assert g1[0][0] == 7 and g1[1][1] == 900 and g2[1][0] == 3 and g2[0][1] == 950 and g2[0][0] >= 100


# ============================================================================================= 5. inference and end to end
def test_infer_scene_resident_with_scale_equals_infer_scene():
    from fcd_gan_pytorch_amd import Module
    z = np.load(os.path.join(GOLDEN, 'tiles.npz'))
    x, y, r = z['a/x'], z['a/y'], z['a/r']
    patch, pad = (40, 40), (5, 5)
    scene = tiles.ResidentScene(x, y, r, patch, pad, device=DEV)
    r1, r2 = scene.maxmin()
    enh = transforms.SCALE(r1, r2)
    scene.set_enhance(enh)
    torch.manual_seed(1234)
    net = Module.Segmentor(4, bilinear=True).to(DEV).eval()
    want = demos.infer_scene(net, tiles.PairTileDataset(x, y, r, patch, pad, enhance=enh), DEV, batch_size=3)
    got = demos.infer_scene_resident(net, scene, DEV, batch_size=3)
    _eq(got['density'], want['density'], 'density'); _eq(got['color'], want['color'], 'color')
    _eq(got['evaluator']._sync(), want['evaluator']._sync(), 'confusion matrix')
    assert got['evaluator']._sync().sum() == x.shape[1] * x.shape[2]
    plain = demos.infer_scene_resident(net, tiles.ResidentScene(x, y, r, patch, pad, device=DEV), DEV, batch_size=3)
    assert (plain['density'] != got['density']).any()          # the enhancer was applied


TILE = 176          # MS-SSIM refuses tiles of 160 pixels or fewer (tests/test_gpu_scene_train.py)


def test_demo_usss_with_scale_and_erasing_on_the_resident_route(tmp_path, monkeypatch):
    H = W = 2 * TILE
    rng = np.random.default_rng(11)
    t1 = rng.integers(100, 3000, (4, H, W)).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, (4, H, W))).clip(0, 65535).astype(np.uint16)
    t2[:, 90:210, 250:330] = rng.integers(100, 3000, (4, 120, 80))
    ref = np.ones((1, H, W), np.uint8)
    ref[:, 90:210, 250:330] = 2
    first = []
    cut = ops.scene_set_cut

    def watching_cut(*a, **k):
        out = cut(*a, **k)
        if not first and k.get('erase') is not None:
            first.append((k['erase'].rows.copy(), out[0].clone(), out[1].clone(), k['mode']))
        return out
    monkeypatch.setattr(ops, 'scene_set_cut', watching_cut)
    txt = (str(tmp_path / 'x.txt'), str(tmp_path / 'y.txt'))
    out = demos.demo_usss(t1, t2, ref, patch_size=(TILE, TILE), overlap_padding=(0, 0), epochs_g=1, epochs_s=1, epochs_joint=1,
                          batch_size=2, allow_seeded=True, stats_txt=txt, resident_training=True, resident_inference=True,
                          enhance='scale', transforms=transforms.RANDOM_ERASER_MULTI_REGION(rng=random.Random(1)))
    hist = out['history']
    assert [len(hist[k]) for k in ('g', 's', 'joint')] == [1, 1, 1]
    assert all(np.isfinite(v) for k in hist for v in hist[k])
    assert out['train_evaluator']._sync().sum() == H * W
    assert out['evaluator']._sync().sum() == H * W
    # the ranges went through the cache, and they are the scene's extrema
    r1, r2 = tiles.dataset_maxmin(txt[0], txt[1], None)
    assert [r[0] for r in r1] == t1.reshape(4, -1).min(1).tolist() and [r[1] for r in r2] == t2.reshape(4, -1).max(1).tolist()
    # the first training batch of the feed: exact zeros where the drawn rectangles lie, scaled samples elsewhere
    rows, x, y, mode = first[0]
    assert mode == 2 and rows.shape[0] == 2 and (rows[..., 2] * rows[..., 3]).sum() > 0
    for t in range(2):
        for ex, ey, ew, eh in rows[t]:
            assert not x[t, :, ey:ey + eh, ex:ex + ew].any() and not y[t, :, ey:ey + eh, ex:ex + ew].any()
    assert 0 < float(x.max()) <= 1.0 and float(x.min()) >= 0.0
    # inference never erases: the density is what infer_scene gives over the un-augmented SCALE dataset
    ds = tiles.PairTileDataset(t1, t2, ref, (TILE, TILE), (0, 0), enhance=transforms.SCALE(r1, r2))
    _eq(demos.infer_scene(out['netS'], ds, DEV, batch_size=2)['density'], out['density'], 'infer_scene on the trained net')
    with pytest.raises(ValueError, match='enhance'):
        demos.demo_usss(t1, t2, ref, enhance='gamma')


def test_demo_usss_with_scale_norm_and_erasing_on_the_host_route(tmp_path):
    H = W = 2 * TILE
    rng = np.random.default_rng(12)
    t1 = rng.integers(100, 3000, (4, H, W)).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, (4, H, W))).clip(0, 65535).astype(np.uint16)
    ref = rng.integers(1, 3, (1, H, W)).astype(np.uint8)
    txt = (str(tmp_path / 'x.txt'), str(tmp_path / 'y.txt'))
    eraser = transforms.RANDOM_ERASER(origin_prob=0.0, rng=random.Random(2))
    out = demos.demo_usss(t1, t2, ref, patch_size=(TILE, TILE), overlap_padding=(0, 0), epochs_g=1, epochs_s=0, epochs_joint=0,
                          batch_size=2, allow_seeded=True, stats_txt=txt, enhance='scale_norm', scale_range=(0, 1), transforms=eraser)
    assert len(out['history']['g']) == 1 and np.isfinite(out['history']['g'][0])
    assert eraser.rng.getstate() != random.Random(2).getstate()            # the training tiles drew from it
    assert out['evaluator']._sync().sum() == H * W
    r1, r2 = tiles.dataset_maxmin(txt[0], txt[1], None)                    # the ranges went through the cache
    assert [r[1] for r in r1] == t1.reshape(4, -1).max(1).tolist()
    ds = tiles.PairTileDataset(t1, t2, ref, (TILE, TILE), (0, 0), enhance=transforms.SCALE_NORM(r1, r2, [0, 1]))
    _eq(demos.infer_scene(out['netS'], ds, DEV, batch_size=2)['density'], out['density'], 'inference: same enhancer, no erasing')
    # the resident inference route gives the same map for the same net
    scene = tiles.ResidentScene(t1, t2, ref, (TILE, TILE), (0, 0), device=DEV, enhance=ds.enhance)
    _eq(demos.infer_scene_resident(out['netS'], scene, DEV, batch_size=2)['density'], out['density'], 'resident inference')
