"""Device-resident scene inference (csrc/scene.hip: fcd_scene_cut, fcd_scene_stitch, fcd_tile_confusion) against the host
loop it replaces -- ``PairTileDataset.__getitem__`` / ``raw_item``, ``TileGrid.write_center``, ``metrics.changemap_codes``,
``Evaluator.add_batch_map``, ``demos.infer_scene`` -- and against the arrays the reference itself wrote
(tests/golden/tiles.npz).  The kernels copy, compare and count: every comparison is BIT-EXACT (``assert_array_equal``);
the only tolerance in this file is the one tests/test_gpu_interchange.py already uses for ``Segmentor.forward_raw`` against the
normalised path.

Geometries (the smallest that cover every branch of the border rule): a = 131x97 scene, 4 bands, 40^2 patches, pad 5, 20
tiles (odd widths, clipped right / bottom tiles); b = one 220^2 canvas larger than its 200^2 scene; c = 50x64 scene,
non-square 32x24 patches, pads 4 and 3; d = 256^2 patches whose four tiles are mostly border."""
import functools
import os

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, demos, dp, metrics, tiles

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = os.path.join(os.path.dirname(__file__), 'golden', 'tiles.npz')
TAGS = ['a', 'b', 'c', 'd']


@functools.lru_cache(maxsize=None)
def _z():
    z = np.load(G)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _case(tag):
    """Scene, geometry and statistics of a fixture tag + the host dataset (never modified by a test)."""
    z = _z()
    nb, ys, xs, pw, ph, padx, pady, n = [int(v) for v in z[tag + '/meta']]
    st = z[tag + '/stats']
    c = dict(x=z[tag + '/x'], y=z[tag + '/y'], r=z[tag + '/r'], H=ys, W=xs, patch=(pw, ph), pad=(padx, pady), n=n,
             stats=(st[0], st[1], st[2], st[3]))
    c['ds'] = tiles.PairTileDataset(c['x'], c['y'], c['r'], c['patch'], c['pad'], stats=c['stats'])
    assert len(c['ds']) == n
    return c


def _host_tiles(ds, items=None):
    """(x, y, ref) of the host path, stacked."""
    items = range(len(ds)) if items is None else items
    got = [ds[int(i)] for i in items]
    return tuple(np.stack([g[k].numpy() for g in got]) for k in (0, 1, 3))


def _host_raw(ds, items=None):
    items = range(len(ds)) if items is None else items
    got = [ds.raw_item(int(i)) for i in items]
    return tuple(np.stack([g[k].numpy() for g in got]) for k in (0, 1, 3, 4))


def _np(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


# ============================================================================================= 1. cut == the reference's tiles
@pytest.mark.parametrize('tag', TAGS)
def test_cut_equals_host_tiles_and_reference_arrays(tag):
    c, z = _case(tag), _z()
    scene = tiles.ResidentScene(c['x'], c['y'], c['r'], c['patch'], c['pad'], stats=c['stats'], device=DEV)
    assert scene.x.element_size() == 2 and len(scene) == c['n']           # uint16 stays uint16 on the device
    gx, gy, gr, gv = _np(scene.cut(range(c['n'])))
    hx, hy, hr = _host_tiles(c['ds'])
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y'); _eq(gr, hr, 'ref')
    for item in z[tag + '/pick']:                                         # what the reference itself wrote
        _eq(gx[item], z['%s/item%d/x' % (tag, item)], 'x of item %d' % item)
        _eq(gy[item], z['%s/item%d/y' % (tag, item)], 'y of item %d' % item)
        _eq(gr[item], z['%s/item%d/ref' % (tag, item)], 'ref of item %d' % item)
    rx, ry, rr, rv = _np(scene.cut(range(c['n']), raw=True))
    wx, wy, wr, wv = _host_raw(c['ds'])
    _eq(rx, wx, 'raw x'); _eq(ry, wy, 'raw y'); _eq(rr, wr, 'raw ref'); _eq(rv, wv, 'valid'); _eq(gv, wv, 'valid (normalised cut)')


# ============================================================================================= 2. sample types, poisoned canvases
def _scene_a_as(kind):
    c = _case('a')
    if kind == 'uint8':
        return (c['x'] % 256).astype(np.uint8), (c['y'] % 256).astype(np.uint8)
    if kind == 'uint16':
        return c['x'], c['y']
    x = (c['x'].astype(np.float32) / 7 - 100).astype(np.float32)           # negative and fractional values
    y = (c['y'].astype(np.float32) / 3 - 500).astype(np.float32)
    x[1, 50, 60] = np.nan                                                  # inside the read block of tile (2, 1) = item 9
    x[2, 10, 10] = np.inf
    y[0, 96, 130] = -np.inf                                                # the last pixel of the scene
    y[3, 31, 29] = np.nan                                                  # in the overlap of four tiles
    return x, y


@pytest.mark.parametrize('kind', ['uint8', 'uint16', 'float32'])
@pytest.mark.parametrize('raw', [False, True])
def test_cut_sample_types_match_host_path_and_write_every_element(kind, raw):
    c = _case('a')
    x, y = _scene_a_as(kind)
    ds = tiles.PairTileDataset(x, y, c['r'], c['patch'], c['pad'], stats=c['stats'])
    scene = tiles.ResidentScene(x, y, c['r'], c['patch'], c['pad'], stats=c['stats'], device=DEV)
    assert scene.x.element_size() == x.dtype.itemsize
    n, (pw, ph) = c['n'], c['patch']
    table = ops.scene_tile_table(scene.grid, range(n))
    out = tuple(torch.full(s, float('nan'), device=DEV) for s in ((n, 4, ph, pw), (n, 4, ph, pw), (n, 1, ph, pw), (n, 1, ph, pw)))
    got = ops.scene_cut(scene.x, scene.y, table, ref=scene.ref, stats=None if raw else scene._stats_dev,
                        sample_type=scene.sample_type, out=out)
    assert all(g is o for g, o in zip(got, out))
    gx, gy, gr, gv = _np(got)
    if raw:
        hx, hy, hr, hv = _host_raw(ds)
    else:
        hx, hy, hr = _host_tiles(ds)
        hv = _host_raw(ds)[3]
    _eq(gx, hx, 'x'); _eq(gy, hy, 'y'); _eq(gr, hr, 'ref'); _eq(gv, hv, 'valid')
    assert not np.isnan(gr).any() and not np.isnan(gv).any()               # no poison left (x / y carry the planted NaN only)
    if kind == 'float32':
        assert np.isnan(gx).sum() == np.isnan(hx).sum() > 0 and np.isinf(gy).sum() == np.isinf(hy).sum() > 0
    else:
        assert np.isfinite(gx).all() and np.isfinite(gy).all()
    # the reference map in its own sample type (uint8, as stored) gives the tiles of the float32 upload
    ref_u8 = torch.from_numpy(c['r']).to(DEV)
    assert ref_u8.dtype == torch.uint8
    gr8 = ops.scene_cut(scene.x, scene.y, table, ref=ref_u8, sample_type=scene.sample_type)[2]
    _eq(gr8.cpu().numpy(), hr, 'ref tiles from the uint8 map')


def test_cut_rejects_what_it_cannot_read():
    c = _case('c')
    scene = tiles.ResidentScene(c['x'], c['y'], c['r'], c['patch'], c['pad'], stats=c['stats'], device=DEV)
    table = ops.scene_tile_table(scene.grid, [0, 1])
    with pytest.raises(_lib.FcdError, match='uint8, uint16 or float32'):
        ops.scene_cut(scene.x.double(), scene.y.double(), table)
    with pytest.raises(_lib.FcdError, match='uint8, uint16 or float32'):
        ops.scene_cut(scene.x, scene.y, table)                            # int16 bits without saying that they are uint16
    with pytest.raises(_lib.FcdError, match='validated for scene'):
        ops.scene_cut(scene.x[:, :-1], scene.y[:, :-1], table, sample_type=scene.sample_type)
    with pytest.raises(_lib.FcdError, match='TileTable'):
        ops.scene_cut(scene.x, scene.y, torch.from_numpy(table.rows).to(DEV), sample_type=scene.sample_type)
    with pytest.raises(_lib.FcdError, match='4\\*C'):
        ops.scene_cut(scene.x, scene.y, table, stats=scene._stats_dev[:3], sample_type=scene.sample_type)


# ============================================================================================= 3. stitch == the host loop
def _eff_mask(grid, items, shape):
    m = torch.zeros(shape, dtype=torch.bool)
    for i, it in enumerate(items):
        r0, r1, c0, c1 = grid.eff_range(it)
        m[i, :, r0:r1, c0:c1] = True
    return m


@functools.lru_cache(maxsize=None)
def _cmap(tag, thresh):
    """uniform(0,1) density tiles with the threshold itself, its two fp32 neighbours and a NaN planted in owned centres and
    garbage (NaN, 9.0) everywhere outside them."""
    c = _case(tag)
    grid, n, (pw, ph), (padx, pady) = c['ds'].grid, c['n'], c['patch'], c['pad']
    rng = np.random.default_rng(len(tag) + int(thresh * 10))
    cm = rng.uniform(0, 1, (n, 1, ph, pw)).astype(np.float32)
    t32 = np.float32(thresh)
    cm[0, 0, pady + 1, padx + 1] = t32                                     # must NOT count as changed
    cm[0, 0, pady + 1, padx + 2] = np.nextafter(t32, np.float32(1))        # the next fp32 above: changed
    cm[0, 0, pady + 1, padx + 3] = np.nextafter(t32, np.float32(0))        # the next fp32 below: not changed
    cm[1, 0, pady + 2, padx + 2] = np.nan                                  # written through, thresholds to 0
    eff = _eff_mask(grid, range(n), cm.shape).numpy()
    jj, ii = np.meshgrid(np.arange(ph), np.arange(pw), indexing='ij')
    garbage = np.where((ii + jj) % 2 == 0, np.float32(np.nan), np.float32(9.0)).astype(np.float32)
    cm = np.where(eff, cm, garbage[None, None]).astype(np.float32)
    return cm


def _host_stitch(c, cm, ref, thresh, gt_map, pre_map, write_color, items=None, fill=-7.0):
    """density / color by TileGrid.write_center over cmap and metrics.changemap_codes, counts by Evaluator.add_batch_map."""
    grid = c['ds'].grid
    items = list(range(c['n'])) if items is None else items
    cmt = torch.from_numpy(np.ascontiguousarray(cm))
    maskf = (cmt > thresh).to(cmt.dtype)                                   # steps.infer_density: cmap > prob_thresh, in fp32
    dens = np.full((1, c['H'], c['W']), fill, np.float32)
    col = np.full((1, c['H'], c['W']), fill, np.float32)
    counts = np.zeros(4, np.int64)
    if ref is not None:
        rds = tiles.PairTileDataset(c['x'], c['y'], ref, c['patch'], c['pad'])
        rt = torch.stack([rds[int(i)][3] for i in items])
        ev = metrics.Evaluator(2)
        ev.add_batch_map(rt, maskf, gt_map, pre_map, valid=_eff_mask(grid, items, cmt.shape))
        counts = ev._dev_counts.numpy().copy()
    if ref is not None and write_color:
        codes = metrics.changemap_codes(maskf, rt, True, ref_map=gt_map, dt_map=pre_map)
    else:
        codes = metrics.changemap_codes(maskf, maskf, False, dt_map=pre_map)
    for i, it in enumerate(items):
        grid.write_center(dens, cm[i], it)
        grid.write_center(col, codes[i].numpy(), it)
    return dens, col, counts


def _dev_stitch(c, cm, ref, thresh, gt_map, pre_map, write_color, batches=None, fill=-7.0):
    grid = c['ds'].grid
    cmd = torch.from_numpy(np.ascontiguousarray(cm)).to(DEV)
    dens = torch.full((1, c['H'], c['W']), fill, device=DEV)
    col = torch.full((1, c['H'], c['W']), fill, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    refd = None if ref is None else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(DEV)
    for items, n_real in (batches or [(list(range(c['n'])), c['n'])]):
        table = ops.scene_tile_table(grid, items)
        ops.scene_stitch(cmd[items], table, dens, col, n=n_real, prob_thresh=thresh, gt_map=gt_map, pre_map=pre_map,
                         write_color=write_color, ref=refd, counts=counts)
    return dens.cpu().numpy(), col.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize('maps', [((1, 2), (0, 1)), ((2, 1), (1, 0))], ids=['maps', 'maps_swapped'])
@pytest.mark.parametrize('thresh', [0.5, 0.6])
@pytest.mark.parametrize('tag', ['a', 'c'])
def test_stitch_equals_host_loop(tag, thresh, maps):
    c, cm = _case(tag), _cmap(tag, thresh)
    gt_map, pre_map = maps
    nodata = c['r'].copy()
    nodata[0, ::3, ::5] = 0                                                # neither gt value: no cell, colour code 0
    for ref, write_color in ((c['r'], True), (nodata, True), (c['r'], False), (None, True)):
        what = '%s ref, write_color=%s' % ('no' if ref is None else 'nodata' if ref is nodata else 'full', write_color)
        hd, hc, hn = _host_stitch(c, cm, ref, thresh, gt_map, pre_map, write_color)
        gd, gc, gn = _dev_stitch(c, cm, ref, thresh, gt_map, pre_map, write_color)
        _eq(gd, hd, 'density, ' + what); _eq(gc, hc, 'color, ' + what); _eq(gn, hn, 'counts, ' + what)
        assert not (gd == -7).any() and not (gc == -7).any()               # every scene pixel is owned by exactly one tile
        assert not (gd == 9.0).any() and np.isnan(gd).sum() == 1           # nothing of the pad ring, the planted centre NaN only
        assert set(np.unique(gc)).issubset({0.0, 1.0, 2.0, 3.0} if write_color and ref is not None else {0.0, 1.0})
        if ref is c['r']:
            assert gn.sum() == c['H'] * c['W']
        elif ref is nodata:
            assert gn.sum() == c['H'] * c['W'] - (nodata == 0).sum()
            assert (gc[nodata == 0] == 0).all() if write_color else True
        else:
            assert gn.sum() == 0
    # the planted values, read back from the density map (tile 0 owns the scene's top-left corner)
    t32 = np.float32(thresh)
    _eq(gd[0, 1, 1:4], np.array([t32, np.nextafter(t32, np.float32(1)), np.nextafter(t32, np.float32(0))], np.float32), 'planted')
    changed = 1.0 if pre_map[1] == 1 else 0.0                              # no reference: colour 1 where pre == pre_map[1]
    _eq(gc[0, 1, 1:4], np.array([1 - changed, changed, 1 - changed], np.float32), 'threshold is exclusive, in fp32')


@pytest.mark.parametrize('tag', TAGS)
def test_stitch_reproduces_the_reference_written_map(tag):
    """The per-item patches of test_tile_geometry_patches_and_writeback_bit_exact, stitched on the device."""
    c, z = _case(tag), _z()
    (pw, ph), ds = c['patch'], c['ds']
    cm = np.stack([(torch.full((1, ph, pw), float(item)) + ds[item][0][0:1] * 0 + ds[item][0][0:1].mean()).numpy()
                   for item in range(c['n'])])
    gd, gc, gn = _dev_stitch(c, cm, None, 0.5, (1, 2), (0, 1), True, fill=0.0)
    _eq(gd, z[tag + '/written'], 'written')


# ============================================================================================= 4. padding, accumulation, determinism
def test_stitch_in_padded_batches_accumulates_like_one_call():
    c, cm = _case('a'), _cmap('a', 0.5)
    n = c['n']
    batches = [(list(range(b, min(b + 3, n))), min(3, n - b)) for b in range(0, n, 3)]
    assert batches[-1] == ([18, 19], 2)
    batches[-1] = ([18, 19, 0], 2)                                         # padded by a duplicate of the head, n_real = 2
    one = _dev_stitch(c, cm, c['r'], 0.5, (1, 2), (0, 1), True)
    many = _dev_stitch(c, cm, c['r'], 0.5, (1, 2), (0, 1), True, batches=batches)
    again = _dev_stitch(c, cm, c['r'], 0.5, (1, 2), (0, 1), True, batches=batches)
    for a, b, d, what in zip(one, many, again, ('density', 'color', 'counts')):
        _eq(b, a, what + ': batches of 3 vs one call')
        assert b.tobytes() == d.tobytes(), what + ': two identical runs differ'
    assert one[2].sum() == c['H'] * c['W']                                 # the padded duplicate was not counted twice


def test_more_planes_and_tiles_than_the_grid_holds():
    """65,544 tiles of geometry c = 393,264 cut planes: more than the y dimension of a grid holds (65,535), so the grid-stride
    loops of all three kernels go round (cf. test_normalize_tiles_beyond_the_grid_cap)."""
    c = _case('c')
    reps, n = 5462, c['n']
    assert reps * n > 65535
    items = list(range(n)) * reps
    scene = tiles.ResidentScene(c['x'], c['y'], c['r'], c['patch'], c['pad'], stats=c['stats'], device=DEV)
    table = ops.scene_tile_table(scene.grid, items)
    x, y, r, valid = scene.cut(table)
    hx, hy, hr = _host_tiles(c['ds'])
    gx, gy, gr = (t.view((reps, n) + t.shape[1:]) for t in (x, y, r))
    for t, h, what in ((gx, hx, 'x'), (gy, hy, 'y'), (gr, hr, 'ref')):
        assert torch.equal(t, torch.from_numpy(h).to(DEV)[None].expand_as(t)), what
    del x, y, gx, gy
    cm = _cmap('c', 0.5)
    cmd = torch.from_numpy(cm).to(DEV).repeat(reps, 1, 1, 1)
    dens, col = scene.new_maps()
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.scene_stitch(cmd, table, dens, col, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), ref=scene.ref, counts=counts)
    hd, hc, hn = _host_stitch(c, cm, c['r'], 0.5, (1, 2), (0, 1), True)
    _eq(dens.cpu().numpy(), hd, 'density'); _eq(col.cpu().numpy(), hc, 'color'); _eq(counts.cpu().numpy(), hn * reps, 'counts')
    ev = metrics.Evaluator(2)
    ev.add_tiles(r, cmd, [scene.grid.eff_range(i) for i in range(n)] * reps, 0.5, (1, 2), (0, 1))
    _eq(ev._dev_counts.cpu().numpy(), hn * reps, 'add_tiles counts')


def test_offsets_beyond_2_to_the_31():
    """A one-band 46400^2 scene has 2.15e9 samples: the last tile's scene offsets do not fit 32 bits.  uint8 samples and device-
    side fills keep this at ~2 GB for the scene and no host array; the maps are allocated, not filled."""
    S, patch, pad = 46400, (64, 64), (4, 4)
    assert S * S > 2 ** 31
    grid = tiles.TileGrid(S, S, patch, pad)
    last = len(grid) - 1
    (x0, y0, w, h), (rx, ry, rw, rh), (wx, wy, ww, wh) = grid.slices(last)
    assert (y0 * S + x0) > 2 ** 31 and x0 + w == S and y0 + h == S
    scene = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    block = torch.randint(0, 256, (rh, rw), dtype=torch.uint8, device=DEV, generator=g)
    scene[0, ry:ry + rh, rx:rx + rw] = block
    table = ops.scene_tile_table(grid, [last, 0])
    x, y, r, valid = ops.scene_cut(scene, scene, table, ref=scene)
    want = torch.zeros((64, 64), device=DEV)
    want[wy:wy + wh, wx:wx + ww] = block.float()
    assert torch.equal(x[0, 0], want) and torch.equal(y[0, 0], want) and torch.equal(r[0, 0], want)
    assert valid[0, 0].sum().item() == rw * rh and not x[1].any()
    del scene
    dens = torch.empty((1, S, S), device=DEV)
    col = torch.empty((1, S, S), device=DEV)
    dens[0, y0:, x0:] = -7; col[0, y0:, x0:] = -7
    cm = torch.rand((2, 1, 64, 64), device=DEV, generator=g)
    ops.scene_stitch(cm, table, dens, col, n=1, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1))
    assert torch.equal(dens[0, y0:, x0:], cm[0, 0, 4:4 + h, 4:4 + w])
    assert torch.equal(col[0, y0:, x0:], (cm[0, 0, 4:4 + h, 4:4 + w] > 0.5).float())
    del dens, col
    torch.cuda.empty_cache()                                               # 17 GB of maps: hand them back at once


# ============================================================================================= 5. Evaluator.add_tiles
def test_add_tiles_equals_add_batch_map():
    z = _z()
    gt, pre = torch.from_numpy(z['metrics/gt']), torch.from_numpy(z['metrics/pre'])
    ref_tiles, cmap = gt.float()[:, None].to(DEV), pre.float()[:, None].to(DEV)       # (3,1,50,60); 0/1 densities, threshold 0.5
    want = metrics.Evaluator(2)
    valid = torch.zeros(gt.shape, dtype=torch.bool)
    valid[:, 5:20, 7:33] = True
    want.add_batch_map(gt, pre, [1, 2], [0, 1], valid=valid)
    want = want._dev_counts.numpy()
    ev = metrics.Evaluator(2)
    ev.add_tiles(ref_tiles, cmap, [(5, 20, 7, 33)] * 3, 0.5, [1, 2], [0, 1])
    assert ev._dev_counts.dtype == torch.int64 and ev._dev_counts.is_cuda
    _eq(ev._dev_counts.cpu().numpy(), want, 'counts over the rectangle')
    assert int(ev._dev_counts.sum()) == 3 * 15 * 26
    ev.add_tiles(ref_tiles, cmap, [(5, 20, 7, 33)] * 3, 0.5, [1, 2], [0, 1])
    _eq(ev._dev_counts.cpu().numpy(), 2 * want, 'called twice')
    ev.add_batch_map(gt.to(DEV), pre.to(DEV), [1, 2], [0, 1], valid=valid.to(DEV))     # the two entry points share one counter
    _eq(ev._sync().reshape(-1), 3.0 * want, 'add_tiles + add_batch_map')
    ev.reset()
    ev.add_tiles(ref_tiles, cmap, [(0, 50, 0, 60)] * 3, 0.5, [1, 2], [0, 1])
    _eq(ev._sync(), z['metrics/cm'], 'confusion matrix over the full tiles')
    got = np.array([ev.Pixel_Accuracy(), ev.Pixel_Kappa(), ev.Pixel_Precision_Rate(), ev.Pixel_Recall_Rate(),
                    ev.Pixel_F1_score(), ev.Mean_Intersection_over_Union()[0], ev.Mean_Intersection_over_Union()[1],
                    ev.Frequency_Weighted_Intersection_over_Union(), ev.Pixel_Accuracy_Class()[0]])
    _eq(got, z['metrics/scores'], 'scores')
    ev.reset()
    ev.add_tiles(ref_tiles, cmap, [(5, 20, 7, 33)] * 2, 0.5, [1, 2], [0, 1])             # fewer rects: padded duplicates left out
    assert int(ev._dev_counts.sum()) == 2 * 15 * 26
    with pytest.raises(_lib.FcdError, match='leaves'):
        ev.add_tiles(ref_tiles, cmap, [(5, 51, 7, 33)] * 3, 0.5, [1, 2], [0, 1])
    with pytest.raises(_lib.FcdError, match='leaves'):
        ev.add_tiles(ref_tiles, cmap, [(-1, 20, 7, 33)] * 3, 0.5, [1, 2], [0, 1])


# ============================================================================================= 6. end to end
PATCH, PAD, BATCH = (40, 40), (5, 5), 3


@functools.lru_cache(maxsize=None)
def _net_and_host_result():
    """The seeded Segmentor and what demos.infer_scene gives on scene a: computed once, shared, never modified."""
    from fcd_gan_pytorch_amd import Module
    c = _case('a')
    torch.manual_seed(1234)
    net = Module.Segmentor(4, bilinear=True).to(DEV).eval()
    ds = tiles.PairTileDataset(c['x'], c['y'], c['r'], PATCH, PAD, stats=c['stats'])
    return net, demos.infer_scene(net, ds, DEV, batch_size=BATCH)


def _resident(c):
    return tiles.ResidentScene(c['x'], c['y'], c['r'], PATCH, PAD, stats=c['stats'], device=DEV)


def test_infer_scene_resident_equals_infer_scene():
    c = _case('a')
    net, want = _net_and_host_result()
    got = demos.infer_scene_resident(net, _resident(c), DEV, batch_size=BATCH)
    assert got['density'].dtype == np.float32 and got['density'].shape == (1, c['H'], c['W'])
    _eq(got['density'], want['density'], 'density'); _eq(got['color'], want['color'], 'color')
    cm = got['evaluator']._sync()
    _eq(cm, want['evaluator']._sync(), 'confusion matrix')
    assert cm.sum() == c['H'] * c['W']
    assert not net.training


def test_infer_scene_resident_raw_stays_within_the_forward_raw_bound():
    c = _case('a')
    net, want = _net_and_host_result()
    got = demos.infer_scene_resident(net, _resident(c), DEV, batch_size=BATCH, raw=True)
    err = np.abs(got['density'] - want['density']).max()
    print('\n[scene] raw (folded NORMALIZE) vs normalised density: max |diff| %.3e' % err)
    assert err <= 2e-5, err                                                # the bound of tests/test_gpu_interchange.py
    safe = np.abs(want['density'] - 0.5) > 2e-5
    _eq(got['color'][safe], want['color'][safe], 'colour codes outside the margin')
    assert got['evaluator']._sync().sum() == c['H'] * c['W']
    with pytest.raises(RuntimeError):
        demos.infer_scene_resident(net, _resident(c), DEV, batch_size=BATCH, raw=True, eval_mode=False)
    with pytest.raises(TypeError):
        demos.infer_scene_resident(net, tiles.PairTileDataset(c['x'], c['y'], c['r'], PATCH, PAD), DEV)


def test_infer_scene_resident_with_a_forced_one_rank_exchange(tmp_path):
    """One rank cannot show a cross-rank sum, but it does send the device maps, the BatchNorm buffers and the counts through
    the collectives: a one-rank sum is the identity, so the maps must not change by a bit."""
    import torch.distributed as dist
    c = _case('a')
    net, want = _net_and_host_result()
    with _lib.switched(DP_FORCE_EXCHANGE=1):
        prev = dp.force_exchange(bool(_lib.switch('DP_FORCE_EXCHANGE')))
        dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
        try:
            assert dp.exchanging() == 1
            got = demos.infer_scene_resident(net, _resident(c), DEV, batch_size=BATCH)
            cm = got['evaluator']._sync()
        finally:
            dist.destroy_process_group()
            dp.force_exchange(prev)
    _eq(got['density'], want['density'], 'density'); _eq(got['color'], want['color'], 'color')
    _eq(cm, want['evaluator']._sync(), 'confusion matrix')


def test_demo_usss_with_resident_inference(tmp_path):
    H = W = 256
    rng = np.random.default_rng(11)
    t1 = rng.integers(100, 3000, (4, H, W)).astype(np.uint16)
    t2 = (t1 + rng.integers(-40, 40, (4, H, W))).clip(0, 65535).astype(np.uint16)
    t2[:, 60:140, 200:250] = rng.integers(100, 3000, (4, 80, 50))
    ref = np.ones((1, H, W), np.uint8)
    ref[:, 60:140, 200:250] = 2
    px, py, pr = str(tmp_path / 'T1.tif'), str(tmp_path / 'T2.tif'), str(tmp_path / 'ref.tif')
    tiles.write_tiff(px, t1); tiles.write_tiff(py, t2); tiles.write_tiff(pr, ref)
    out = demos.demo_usss(px, py, pr, patch_size=(256, 256), overlap_padding=(0, 0), epochs_g=2, epochs_s=1, epochs_joint=1,
                          batch_size=2, allow_seeded=True, out_density=str(tmp_path / 'density.tif'), resident_inference=True)
    dens = tiles.read_tiff(str(tmp_path / 'density.tif'))
    assert dens.dtype == np.float32 and dens.shape == (1, H, W)
    _eq(dens, out['density'], 'density TIFF')
    cm = out['evaluator']._sync()
    assert cm.sum() == H * W
    pred = (dens > 0.5)[0]
    assert cm[1, 1] == np.sum(pred & (ref[0] == 2)) and cm[0, 1] == np.sum(pred & (ref[0] == 1))
    # the default route over the trained net gives the same map
    ds = tiles.PairTileDataset(t1, t2, ref, (256, 256), (0, 0), stats=demos._tile_stats(t1, t2, (256, 256)))
    _eq(demos.infer_scene(out['netS'], ds, DEV, batch_size=2)['density'], dens, 'infer_scene on the trained net')
