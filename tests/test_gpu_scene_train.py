"""The device-resident training feed (csrc/scene.hip: fcd_scene_stats, fcd_scene_set_cut, fcd_tile_confusion_items;
tiles.ResidentScene.statistics, tiles.ResidentSceneSet, demos.demo_usss(resident_training=True), demos.demo_rsss on a set)
against the host route it stands in for -- ``RegionTileDataset`` / ``MultiSceneDataset`` / ``demos._Epoch`` /
``Evaluator.add_batch_map`` -- and against what the reference wrote (tests/golden/{stats,tiles,datasets}.npz).

Tiles and counts are compared BIT-EXACT.  The statistics have three bounds, none of them measured on the code under test:
  * integer scenes against the exact rational moments (tests/test_scene_train_host.py:exact_stats): 2^-50 relative = 4 fp64
    ulps (the device sums are exact integers; the host rounds mean, variance and square root once each);
  * against the reference-written fixture: 2^-22 relative = two fp32 ulps (the reference rounds through fp32);
  * float32 scenes against a long-double evaluation: n * 2^-50 (sequential fp64 summation is (n - 1) * 2^-53 at worst; the
    factor 8 covers the two passes and the square root)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, datasets, demos, dp, metrics, tiles
from test_scene_train_host import ULP32_2, exact_stats, stats_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
ULP64_4 = 2.0 ** -50


@functools.lru_cache(maxsize=None)
def _z(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: z[k] for k in z.files}


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def _np(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.abs(want)))


# ============================================================================================= 1. statistics
def _tiles_case(tag):
    z = _z('tiles')
    nb, ys, xs, pw, ph, padx, pady, n = [int(v) for v in z[tag + '/meta']]
    return z[tag + '/x'], z[tag + '/y'], (pw, ph), (padx, pady)


def _device_stats(x, y, patch, pad):
    scene = tiles.ResidentScene(x, y, None, patch, pad, device=DEV)
    got = np.stack(scene.statistics(pad))
    assert got.dtype == np.float64 and got.shape == (4, x.shape[0])
    return got, scene.stats_count


@pytest.mark.parametrize('tag,pad,count', [('s1', 'own', 8934), ('s1', (0, 0), 5667), ('s2', 'own', 5609), ('s2', (0, 0), 3505),
                                           ('c', 'own', None), ('c', (0, 0), None), ('s1-uint8', 'own', None)])
def test_integer_statistics_equal_the_exact_moments(tag, pad, count):
    if tag == 'c':
        x, y, patch, own = _tiles_case('c')
        fixture = None
    else:
        x, y, patch, own, fixture = stats_case(tag[:2])
    if tag.endswith('uint8'):
        x, y, fixture = (x % 256).astype(np.uint8), (y % 256).astype(np.uint8), None
    fixture = fixture if pad == 'own' else None
    pad = own if pad == 'own' else pad
    want, n = exact_stats(x, y, patch, pad)
    got, gn = _device_stats(x, y, patch, pad)
    rel = _rel(got, want)
    print('\n[stats] %s pad %s: n %d, device vs exact moments max rel %.3e' % (tag, pad, gn, rel))
    assert gn == n and (count is None or n == count)
    assert rel <= ULP64_4
    if fixture is not None:
        rel = _rel(got, fixture)
        print('[stats] %s: device vs the reference-written fixture max rel %.3e' % (tag, rel))
        assert rel <= ULP32_2


def test_integer_statistics_do_not_overflow_32_bits():
    x = np.full((1, 300, 300), 65535, np.uint16)
    got, n = _device_stats(x, x, (128, 128), (0, 0))
    assert n == 300 * 300
    _eq(got, np.array([[65535.0], [0.0], [65535.0], [0.0]]), 'mean 65535, std 0, exactly')
    table = ops.scene_tile_table(tiles.TileGrid(300, 300, (128, 128), (0, 0)), range(9))
    table.rows[:, 6] = 2 ** 15                                            # rw, rh as if the tiles were huge: the guard speaks first
    table.rows[:, 7] = 2 ** 15
    with pytest.raises(_lib.FcdError, match='2\\^64'):
        ops.scene_stats(torch.zeros((1, 300, 300), dtype=torch.int16, device=DEV),
                        torch.zeros((1, 300, 300), dtype=torch.int16, device=DEV), table, sample_type=ops.SAMPLE_U16)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.scene_stats(torch.zeros((1, 300, 300), dtype=torch.uint8), torch.zeros((1, 300, 300), dtype=torch.uint8), table)


def _float_truth(x, y, patch, pad):
    """Long-double masked statistics of a float32 pair over the tiling; mask = fp32 band sum in band order != 0 (NaN: valid)."""
    C, H, W = x.shape
    grid = tiles.TileGrid(W, H, patch, pad)
    s = np.zeros((H, W), np.float32)
    for c in range(C):
        s = (s + x[c]).astype(np.float32)
    mask = s != 0
    vals = [[[] for _ in range(C)] for _ in range(2)]
    n = 0
    for item in range(len(grid)):
        _, (rx, ry, rw, rh), _ = grid.slices(item)
        m = mask[ry:ry + rh, rx:rx + rw]
        n += int(m.sum())
        for k, a in enumerate((x, y)):
            for c in range(C):
                vals[k][c].append(a[c, ry:ry + rh, rx:rx + rw][m].astype(np.longdouble))
    out = np.empty((4, C), np.float64)
    for k in range(2):
        for c in range(C):
            v = np.concatenate(vals[k][c])
            mean = v.sum() / np.longdouble(n)
            out[2 * k, c] = float(mean)
            out[2 * k + 1, c] = float(np.sqrt(((v - mean) ** 2).sum() / np.longdouble(n - 1)))
    return out, n, mask


def test_float32_statistics():
    x16, y16, patch, pad, _ = stats_case('s1')
    x, y = (x16.astype(np.float32) / 7).astype(np.float32), (y16.astype(np.float32) / 7).astype(np.float32)
    want, n, _ = _float_truth(x, y, patch, pad)
    got, gn = _device_stats(x, y, patch, pad)
    rel = _rel(got, want)
    print('\n[stats] float32 s1: n %d, device vs long double max rel %.3e (bound %.3e)' % (gn, rel, n * ULP64_4))
    assert gn == n == 8934
    assert rel <= n * ULP64_4
    again, _ = _device_stats(x, y, patch, pad)
    assert again.tobytes() == got.tobytes(), 'two runs differ'
    # a pair (+a, -a) in the two bands of one pixel: band sum 0, the pixel does not count
    cx, cy, cpatch, cpad = _tiles_case('c')
    fx, fy = (cx.astype(np.float32) / 7).astype(np.float32), (cy.astype(np.float32) / 3).astype(np.float32)
    base, bn, _ = _float_truth(fx, fy, cpatch, (0, 0))
    fx[0, 20, 30], fx[1, 20, 30] = 123.25, -123.25
    want, n, mask = _float_truth(fx, fy, cpatch, (0, 0))
    assert not mask[20, 30] and n == bn - 1
    got, gn = _device_stats(fx, fy, cpatch, (0, 0))
    assert gn == n and _rel(got, want) <= n * ULP64_4
    # one NaN sample in band 1 of x: the pixel is valid (NaN != 0), exactly meanX[1] and stdX[1] become NaN
    fx[1, 40, 10] = np.nan
    _, n, mask = _float_truth(fx, fy, cpatch, (0, 0))
    assert mask[40, 10]
    got, gn = _device_stats(fx, fy, cpatch, (0, 0))
    assert gn == n
    bad = np.zeros((4, 2), bool)
    bad[0, 1] = bad[1, 1] = True
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()


def test_stats_auto_and_from_device():
    x, y, patch, pad, _ = stats_case('s1')
    want, _ = exact_stats(x, y, patch, (0, 0))
    scene = tiles.ResidentScene(x, y, None, patch, pad, stats='auto', device=DEV)
    _eq(np.stack(scene.stats), np.stack(scene.statistics()), "stats='auto' = statistics()")
    assert _rel(np.stack(scene.stats), want) <= ULP64_4 and scene._stats_dev is not None
    ds = tiles.PairTileDataset(x, y, None, patch, pad, stats=scene.stats)
    gx, gy, _, _ = _np(scene.cut(range(len(scene))))
    _eq(gx, np.stack([ds[i][0].numpy() for i in range(len(ds))]), 'x normalised with the device statistics')
    # the same scene from tensors that are on the device already (uint16 bits in an int16 tensor)
    dx = torch.from_numpy(x.view(np.int16)).to(DEV)
    dy = torch.from_numpy(y.view(np.int16)).to(DEV)
    twin = tiles.ResidentScene.from_device(dx, dy, patch_size=patch, overlap_padding=pad, stats=scene.stats,
                                           sample_type=ops.SAMPLE_U16)
    assert twin.x.data_ptr() == dx.data_ptr() and twin.ref is None and twin.region is None
    _eq(np.stack(twin.statistics()), np.stack(scene.stats), 'statistics of the from_device twin')
    tx, ty, _, _ = _np(twin.cut(range(len(twin))))
    _eq(tx, gx, 'x of the twin'); _eq(ty, gy, 'y of the twin')
    with pytest.raises(_lib.FcdError):
        tiles.ResidentScene.from_device(dx.cpu(), dy.cpu(), patch_size=patch, overlap_padding=pad, sample_type=ops.SAMPLE_U16)


# ============================================================================================= 2. the set cut
NAMES = ['abudhabi', 'paris']
PATCH, PAD = (40, 32), (4, 3)


def _arrays(nm):
    z = _z('datasets')
    xname = str(z['%s/xname' % nm])
    yname = nm + ('_2' if xname.endswith('_1') else '_1')
    return z['%s/%s' % (nm, xname)], z['%s/%s' % (nm, yname)], z['%s/%s-cm.tif' % (nm, nm)], z['%s/%s-region.tif' % (nm, nm)]


def _made_up_stats(k):
    rng = np.random.default_rng(100 + k)
    return (rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4), rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4))


@functools.lru_cache(maxsize=None)
def _pair(with_stats, patch=PATCH, pad=PAD):
    """(host MultiSceneDataset, ResidentSceneSet) over the two fixture scenes; shared, never modified."""
    host, res = [], []
    for k, nm in enumerate(NAMES):
        x, y, ref, region = _arrays(nm)
        st = _made_up_stats(k) if with_stats else None
        host.append(datasets.RegionTileDataset(x, y, region=region, ref=ref, patch_size=patch, overlap_padding=pad, stats=st))
        res.append(tiles.ResidentScene(x, y, ref, patch, pad, stats=st, device=DEV, region=region))
    return datasets.MultiSceneDataset(host, NAMES), tiles.ResidentSceneSet(res, NAMES)


def _host_items(ds, items):
    got = [ds[int(i)] for i in items]
    return tuple(np.stack([g[k].numpy() for g in got]) for k in (0, 1, 3, 4))


def _host_valid(ds, items):
    out = []
    for i in items:
        s, cur = ds.locate(i)
        out.append(ds.scenes[s].raw_item(cur)[4].numpy())
    return np.stack(out)


def _poisoned(n, C, patch):
    pw, ph = patch
    return tuple(torch.full(s, float('nan'), device=DEV) for s in ((n, C, ph, pw), (n, C, ph, pw), (n, 1, ph, pw), (n, 1, ph, pw),
                                                                    (n, 1, ph, pw)))


MIXED = [0, 9, 3, 14, 3, 10, 8, 9, 0, 12, 5, 11, 5]            # alternates between the two scenes, with repeats


@pytest.mark.parametrize('with_stats', [False, True], ids=['raw', 'per_scene_stats'])
@pytest.mark.parametrize('items', [list(range(15)), MIXED], ids=['all', 'mixed'])
def test_set_cut_equals_the_host_datasets(items, with_stats):
    host, res = _pair(with_stats)
    z = _z('datasets')
    assert len(res) == len(host) == 15 and res.cumlen == host.cumlen
    assert [res.locate(i) for i in range(15)] == [host.locate(i) for i in range(15)]
    assert [res.eff_range(i) for i in range(15)] == [host.eff_range(i) for i in range(15)]
    _eq(res.table.rects, z['eff'], 'the rectangle table = the reference-written EffRange')
    out = _poisoned(len(items), 4, PATCH)
    got = res.cut(items, out=out)
    assert all(g is o for g, o in zip(got, out))
    gx, gy, gr, gg, gv = _np(got)
    hx, hy, hr, hg = _host_items(host, items)
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y'); _eq(gr, hr, 'ref'); _eq(gg, hg, 'region'); _eq(gv, _host_valid(host, items), 'valid')
    assert not any(np.isnan(a).any() for a in (gx, gy, gr, gg, gv))       # every element was written
    assert set(np.unique(gg)).issubset({0.0, 1.0})
    if not with_stats:                                                    # what the reference itself wrote (no NORMALIZE there)
        for pos, it in enumerate(items):
            if it in z['pick']:
                for a, key in ((gx, 'x'), (gy, 'y'), (gr, 'ref'), (gg, 'region')):
                    _eq(a[pos], z['item%d/%s' % (it, key)], '%s of item %d' % (key, it))
    raw = _np(res.cut(items, raw=True))
    rx, ry, _, _ = _host_items(_pair(False)[0], items)
    _eq(raw[0], rx, 'raw x'); _eq(raw[1], ry, 'raw y')


def test_set_cut_rejects_what_it_cannot_read():
    host, res = _pair(False)
    with pytest.raises(_lib.FcdError, match='tile index'):
        res.cut([0, 15])
    with pytest.raises(_lib.FcdError, match='tile index'):
        res.cut([])
    idx = res.index([1, 2])
    with pytest.raises(_lib.FcdError, match='descs'):
        ops.scene_set_cut(res._descs.cpu(), res.table, idx, 4, res.sample_type)
    with pytest.raises(_lib.FcdError, match='descs'):
        ops.scene_set_cut(res._descs[:1], res.table, idx, 4, res.sample_type)
    with pytest.raises(_lib.FcdError, match='TileIndex'):
        ops.scene_set_cut(res._descs, res.table, idx.dev, 4, res.sample_type)
    with pytest.raises(_lib.FcdError, match='TileIndex'):
        ops.scene_set_cut(res._descs, res.table, ops.TileIndex([1, 2], 16, DEV), 4, res.sample_type)
    with pytest.raises(_lib.FcdError, match='S\\*4\\*C'):
        ops.scene_set_cut(res._descs, res.table, idx, 4, res.sample_type, stats=torch.zeros(16, dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.FcdError, match='out x'):
        ops.scene_set_cut(res._descs, res.table, idx, 4, res.sample_type, out=_poisoned(3, 4, PATCH))


def test_region_rule_and_absent_maps():
    ax, ay, aref, _ = _arrays('abudhabi')
    px, py, pref, _ = _arrays('paris')
    H, W = ax.shape[1:]
    cycle = np.array([0, 7, 125, 126, 255], np.uint8)
    region = cycle[np.arange(H * W) % 5].reshape(1, H, W)
    host = datasets.MultiSceneDataset([
        datasets.RegionTileDataset(ax, ay, region=region, ref=aref, patch_size=PATCH, overlap_padding=PAD),
        datasets.RegionTileDataset(px, py, region=None, ref=None, patch_size=PATCH, overlap_padding=PAD)])
    res = tiles.ResidentSceneSet([tiles.ResidentScene(ax, ay, aref, PATCH, PAD, device=DEV, region=region),
                                  tiles.ResidentScene(px, py, None, PATCH, PAD, device=DEV)])
    assert res.scenes[0].region.dtype == torch.uint8 and res.has_region and res.has_ref
    got = res.cut(range(15), out=_poisoned(15, 4, PATCH))
    gx, gy, gr, gg, gv = _np(got)
    hx, hy, hr, hg = _host_items(host, range(15))
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y'); _eq(gr, hr, 'ref'); _eq(gg, hg, 'region')
    assert not gg[9:].any() and not gr[9:].any()                           # the scene without maps: zero tiles, written
    want = np.array([0, 7, 125, 1, 1], np.float32)
    for item in range(9):                                                  # the rule itself, from the scene
        _, (rx, ry, rw, rh), (wx, wy, ww, wh) = host.scenes[0].grid.slices(item)
        canvas = np.zeros((32, 40), np.float32)
        canvas[wy:wy + wh, wx:wx + ww] = want[(np.arange(H * W) % 5).reshape(H, W)[ry:ry + rh, rx:rx + rw]]
        _eq(gg[item, 0], canvas, 'region tile %d' % item)
    assert set(np.unique(gg)) == {0.0, 1.0, 7.0, 125.0}


def test_mixed_geometry():
    z = _z('tiles')
    a = tiles.ResidentScene(z['a/x'], z['a/y'], z['a/r'], (40, 40), (5, 5), device=DEV)
    d = tiles.ResidentScene(z['d/x'], z['d/y'], z['d/r'], (40, 40), (5, 5), device=DEV)
    with pytest.raises(_lib.FcdError, match='band count'):
        tiles.ResidentSceneSet([a, d])
    with pytest.raises(_lib.FcdError, match='patch size'):
        tiles.ResidentSceneSet([a, tiles.ResidentScene(z['a/x'], z['a/y'], z['a/r'], (40, 32), (5, 5), device=DEV)])
    with pytest.raises(_lib.FcdError, match='sample type'):
        tiles.ResidentSceneSet([a, tiles.ResidentScene((z['a/x'] % 256).astype(np.uint8), (z['a/y'] % 256).astype(np.uint8), None,
                                                       (40, 40), (5, 5), device=DEV)])
    # a 131x97 scene (20 tiles, clipped right and bottom) and a 29x27 crop of it: ONE tile larger than its scene, clipped on every side
    crop = tuple(np.ascontiguousarray(z[k][:, 10:37, 20:49]) for k in ('a/x', 'a/y', 'a/r'))
    st = tuple(z['a/stats'])
    small = tiles.ResidentScene(crop[0], crop[1], crop[2], (40, 40), (5, 5), stats=st, device=DEV)
    big = tiles.ResidentScene(z['a/x'], z['a/y'], z['a/r'], (40, 40), (5, 5), stats=st, device=DEV)
    res = tiles.ResidentSceneSet([small, big])
    host = datasets.MultiSceneDataset([
        datasets.RegionTileDataset(crop[0], crop[1], ref=crop[2], patch_size=(40, 40), overlap_padding=(5, 5), stats=st),
        datasets.RegionTileDataset(z['a/x'], z['a/y'], ref=z['a/r'], patch_size=(40, 40), overlap_padding=(5, 5), stats=st)])
    assert len(small) == 1 and len(res) == len(host) == 21 and not res.has_region
    gx, gy, gr, gg, gv = _np(res.cut(range(21), out=_poisoned(21, 4, (40, 40))))
    hx, hy, hr, hg = _host_items(host, range(21))
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y'); _eq(gr, hr, 'ref'); _eq(gg, hg, 'region'); _eq(gv, _host_valid(host, range(21)), 'valid')
    assert gv[0].sum() == 27 * 29


# ============================================================================================= 3. grid limits
def test_more_planes_than_the_grid_holds():
    host, res = _pair(True)
    reps = 400
    items = list(range(15)) * reps
    assert len(items) * (2 * 4 + 3) > 65535
    x, y, r, g, v = res.cut(items)
    hx, hy, hr, hg = _host_items(host, range(15))
    hv = _host_valid(host, range(15))
    for t, h, what in ((x, hx, 'x'), (y, hy, 'y'), (r, hr, 'ref'), (g, hg, 'region'), (v, hv, 'valid')):
        t = t.view((reps, 15) + t.shape[1:])
        assert torch.equal(t, torch.from_numpy(h).to(DEV)[None].expand_as(t)), what


def test_set_offsets_beyond_2_to_the_31():
    """A one-band 46400^2 uint8 scene (2.15e9 samples, filled on the device, no host array) behind a small scene in one set:
    the last tile's scene offsets do not fit 32 bits."""
    S, patch, pad = 46400, (128, 128), (4, 4)
    grid = tiles.TileGrid(S, S, patch, pad)
    (x0, y0, w, h), (rx, ry, rw, rh), (wx, wy, ww, wh) = grid.slices(len(grid) - 1)
    assert (ry * S + rx) > 2 ** 31 and x0 + w == S and y0 + h == S
    gen = torch.Generator(device=DEV).manual_seed(3)
    small = torch.randint(1, 256, (1, 70, 90), dtype=torch.uint8, device=DEV, generator=gen)
    scene = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    block = torch.randint(0, 256, (rh, rw), dtype=torch.uint8, device=DEV, generator=gen)
    scene[0, ry:ry + rh, rx:rx + rw] = block
    res = tiles.ResidentSceneSet([
        tiles.ResidentScene.from_device(small, small, ref=small, region=small, patch_size=patch, overlap_padding=pad),
        tiles.ResidentScene.from_device(scene, scene, ref=scene, region=scene, patch_size=patch, overlap_padding=pad)])
    assert len(res) == 1 + len(grid) and res.locate(len(res) - 1) == (1, len(grid) - 1)
    x, y, r, g, v = res.cut([len(res) - 1, 0])
    want = torch.zeros((128, 128), device=DEV)
    want[wy:wy + wh, wx:wx + ww] = block.float()
    assert torch.equal(x[0, 0], want) and torch.equal(y[0, 0], want) and torch.equal(r[0, 0], want)
    assert torch.equal(g[0, 0], torch.where(want > 125, torch.ones_like(want), want))
    assert v[0, 0].sum().item() == rw * rh
    first = torch.zeros((128, 128), device=DEV)
    first[4:4 + 70, 4:4 + 90] = small[0].float()
    assert torch.equal(x[1, 0], first)
    del scene, res
    torch.cuda.empty_cache()


# ============================================================================================= 4. the epoch feed
def _host_epoch(ds, batch, seed, ragged, rank, world):
    ep = demos._Epoch(ds, batch, seed, DEV, ragged=ragged)
    ep.sampler = dp.RankStridedBatches(len(ds), batch, seed=seed, rank=rank, world=world, ragged=ragged)
    return ep


@pytest.mark.parametrize('ragged', ['pad', 'drop', 'weighted'])
@pytest.mark.parametrize('rank,world', [(0, 1), (0, 2), (1, 2)])
def test_epoch_feed_equals_the_host_epoch(ragged, rank, world):
    host, res = _pair(True)
    want = list(_host_epoch(host, 4, 5, ragged, rank, world))
    got = list(res.epoch(4, 5, ragged=ragged, rank=rank, world=world))
    assert len(got) == len(want) == len(res.epoch(4, 5, ragged=ragged, rank=rank, world=world)) > 0
    for b, ((gb, greal, gw), (hb, hreal, hw)) in enumerate(zip(got, want)):
        assert len(gb) == len(hb) == 5
        gx, gy, gitem, gr, gg = gb
        hx, hy, hitem, hr, hg = hb
        assert gitem.dtype == torch.int64 and not gitem.is_cuda and torch.equal(gitem, hitem.cpu())
        for g, h, what in ((gx, hx, 'x'), (gy, hy, 'y'), (gr, hr, 'ref'), (gg, hg, 'region')):
            assert g.is_cuda and g.dtype == torch.float32
            _eq(g.cpu().numpy(), h.cpu().numpy(), '%s of batch %d' % (what, b))
        assert greal == hreal and float(gw) == float(hw) and gw.loss_scale == hw.loss_scale
        assert (gw.rects is None) == (greal == 0) and (greal == 0 or gw.rects.n == greal)


def test_epoch_makes_no_copy_and_no_host_wait(monkeypatch):
    host, res = _pair(True)
    res.cut([0])                                               # the set's tables go up once per set, not per epoch: before the watch
    uploads, cuts = [], []
    init, cut = ops.TileIndex.__init__, ops.scene_set_cut

    def counting_init(self, items, size, device=None, _view=None):
        if _view is None:
            uploads.append(len(items))
        init(self, items, size, device, _view)

    def watching_cut(descs, table, index, *a, **k):
        cuts.append((table, index))
        return cut(descs, table, index, *a, **k)
    monkeypatch.setattr(ops.TileIndex, '__init__', counting_init)
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
    assert seen == len(plan.flat) == 15 and uploads == [15]    # ONE index upload for the epoch
    assert len(cuts) == len(plan) == 4 and all(t is res.table for t, _ in cuts)
    base = cuts[0][1].dev
    for b, (_, idx) in enumerate(cuts):                        # every batch: a device slice of that one upload
        assert isinstance(idx, ops.TileIndex) and idx.dev.is_cuda
        assert idx.dev.data_ptr() == base.data_ptr() + 4 * plan.offsets[b] and len(idx) == len(plan.batches[b])


# ============================================================================================= 5. the metric
def test_add_tiles_with_device_rectangles():
    z = _z('tiles')
    gt, pre = torch.from_numpy(z['metrics/gt']), torch.from_numpy(z['metrics/pre'])       # (3,50,60)
    ref_tiles, cmap = gt.float()[:, None].to(DEV), pre.float()[:, None].to(DEV)
    grid = tiles.TileGrid(140, 110, (60, 50), (5, 7))            # 3 x 4 tiles, the last column 40 wide, the last row 2 high
    table = ops.scene_set_table([grid])
    items = [8, 11, 0]
    rects = [grid.eff_range(i) for i in items]
    assert len(table) == 12 and len(set(rects)) == 3
    _eq(table.rects[items], np.array(rects), 'rectangle table')
    index = ops.TileIndex(items, len(table), DEV)
    for n in (3, 2):                                                       # 2: the trailing duplicate is left out
        dev_ev, host_ev, map_ev = metrics.Evaluator(2), metrics.Evaluator(2), metrics.Evaluator(2)
        dev_ev.add_tiles(ref_tiles, cmap, ops.DeviceRects(table, index, n), 0.5, [1, 2], [0, 1])
        host_ev.add_tiles(ref_tiles, cmap, rects[:n], 0.5, [1, 2], [0, 1])
        valid = demos._valid_centres(types.SimpleNamespace(eff_range=grid.eff_range), gt[:, None], items, n)
        map_ev.add_batch_map(gt[:, None], pre[:, None], [1, 2], [0, 1], valid=valid)
        got = dev_ev._dev_counts.cpu().numpy()
        _eq(got, host_ev._dev_counts.cpu().numpy(), 'device vs host rectangles, n = %d' % n)
        _eq(got, map_ev._dev_counts.numpy(), 'device rectangles vs add_batch_map, n = %d' % n)
        assert got.sum() == sum((r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in rects[:n])
    dev_ev.add_tiles(ref_tiles, cmap, ops.DeviceRects(table, index[1:3]), 0.5, [1, 2], [0, 1])   # a slice; accumulates
    host_ev.add_tiles(ref_tiles, cmap, rects[1:3], 0.5, [1, 2], [0, 1])
    _eq(dev_ev._dev_counts.cpu().numpy(), host_ev._dev_counts.cpu().numpy(), 'slice of the index')
    with pytest.raises(_lib.FcdError, match='rectangles for'):
        dev_ev.add_tiles(ref_tiles[:2], cmap[:2], ops.DeviceRects(table, index, 3), 0.5, [1, 2], [0, 1])
    with pytest.raises(_lib.FcdError, match='validated for patch'):
        dev_ev.add_tiles(ref_tiles[..., :40], cmap[..., :40], ops.DeviceRects(table, index, 3), 0.5, [1, 2], [0, 1])


# ============================================================================================= 6. end to end
# Tile size: the criteria run MS-SSIM whatever its weight, and MS-SSIM refuses tiles of 160 pixels or fewer (the reference's own
# assertion, ssim.py: four 2x downsamplings under an 11-tap window).  So these two runs use 176-pixel tiles, the smallest size
# the other demo tests use, with the layout asked for: a scene of 2 x 2 tiles, batch 2 (USSS); two scenes of different sizes,
# ten tiles with clipped borders, batch 3 with a ragged last batch (RSSS).
TILE = 176


def test_demo_usss_with_resident_training(tmp_path):
    H = W = 2 * TILE
    rng = np.random.default_rng(11)
    t1 = rng.integers(100, 3000, (4, H, W)).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, (4, H, W))).clip(0, 65535).astype(np.uint16)
    t2[:, 90:210, 250:330] = rng.integers(100, 3000, (4, 120, 80))
    ref = np.ones((1, H, W), np.uint8)
    ref[:, 90:210, 250:330] = 2
    txt = (str(tmp_path / 'x.txt'), str(tmp_path / 'y.txt'))
    stats = tiles.scene_meanstd(txt[0], txt[1], tiles.ResidentScene(t1, t2, None, (TILE, TILE), (0, 0), device=DEV))
    want, _ = exact_stats(t1, t2, (TILE, TILE), (0, 0))
    assert _rel(np.array(stats), want) <= ULP64_4
    out = demos.demo_usss(t1, t2, ref, patch_size=(TILE, TILE), overlap_padding=(0, 0), epochs_g=2, epochs_s=1, epochs_joint=1,
                          batch_size=2, allow_seeded=True, stats_txt=txt, resident_training=True, resident_inference=True)
    hist = out['history']
    assert [len(hist[k]) for k in ('g', 's', 'joint')] == [2, 1, 1]
    assert all(np.isfinite(v) for k in hist for v in hist[k])
    assert out['train_evaluator']._sync().sum() == H * W
    assert out['evaluator']._sync().sum() == H * W
    ds = tiles.PairTileDataset(t1, t2, ref, (TILE, TILE), (0, 0), stats=tuple(np.asarray(v, np.float64) for v in stats))
    _eq(demos.infer_scene(out['netS'], ds, DEV, batch_size=2)['density'], out['density'], 'infer_scene on the trained net')


def test_demo_rsss_on_a_resident_scene_set():
    scenes, pixels = [], 0
    for nm in NAMES:                                                       # the two fixture scenes, repeated 4 x 4: 280x360 and 220x192
        x, y, ref, region = (np.ascontiguousarray(np.tile(a, (1, 4, 4))) for a in _arrays(nm))
        scenes.append(tiles.ResidentScene(x, y, ref, (TILE, TILE), (4, 4), device=DEV, region=region))
        pixels += x.shape[1] * x.shape[2]
    res = tiles.ResidentSceneSet(scenes, NAMES)
    assert res.numlist == [6, 4] and pixels == 16 * (70 * 90 + 55 * 48)
    out = demos.demo_rsss(res, epochs_g=1, epochs_adv=1, init_batch_size=3, batch_size=3, allow_seeded=True)
    hist = out['history']
    assert len(hist['g']) == 1 and len(hist['adv']) == 1
    assert np.isfinite(hist['g']).all() and np.isfinite(hist['adv']).all() and len(hist['adv'][0]) == 4
    assert out['evaluator']._sync().sum() == pixels                       # the owned centres = every scene pixel once
    with pytest.raises(ValueError, match='region'):
        demos.demo_rsss(tiles.ResidentSceneSet([tiles.ResidentScene(*_arrays('paris')[:3], (TILE, TILE), (4, 4), device=DEV)]),
                        epochs_g=0, epochs_adv=0, allow_seeded=True)
