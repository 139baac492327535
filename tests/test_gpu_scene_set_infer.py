"""Inference over a scene set (csrc/scene.hip: fcd_scene_set_stitch; _ops.scene_set_stitch, tiles.ResidentSceneSet.new_maps /
stitch, demos.infer_scene_set / infer_scene_set_resident, demos.demo_rsss(test_dataset=...)) against the host route it stands
in for: ``MultiSceneDataset.write_center``, the rules of ``metrics.changemap_codes`` and ``np.sum`` per cell and scene, all in
a NumPy loop in this file.  The kernel copies floats and counts integers, so everything is compared BIT-EXACT."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import Module, _lib, _ops as ops, datasets, demos, dp, metrics, tiles

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
NAMES = ['abudhabi', 'paris']
PATCH, PAD = (40, 32), (4, 3)                               # 9 + 6 tiles, the right and bottom ones clipped
GT, PRE = (1, 2), (0, 1)
TILE = 176                                                  # the demo runs: MS-SSIM refuses tiles of 160 pixels or fewer


@functools.lru_cache(maxsize=None)
def _z():
    z = np.load(os.path.join(GOLDEN, 'datasets.npz'))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _arrays(nm, reps=1):
    """x, y, ref, region of a fixture scene, repeated ``reps`` x ``reps``; shared, never modified."""
    z = _z()
    xname = str(z['%s/xname' % nm])
    yname = nm + ('_2' if xname.endswith('_1') else '_1')
    out = (z['%s/%s' % (nm, xname)], z['%s/%s' % (nm, yname)], z['%s/%s-cm.tif' % (nm, nm)], z['%s/%s-region.tif' % (nm, nm)])
    return tuple(np.ascontiguousarray(np.tile(a, (1, reps, reps))) for a in out)


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def _host_set(refs, patch=PATCH, pad=PAD, reps=1):
    """The host MultiSceneDataset whose ``locate`` / ``write_center`` / grids the expected values are made with."""
    return datasets.MultiSceneDataset([tiles.PairTileDataset(_arrays(nm, reps)[0], _arrays(nm, reps)[1], r, patch, pad)
                                       for nm, r in zip(NAMES, refs)], NAMES)


def _resident_set(refs, patch=PATCH, pad=PAD, reps=1):
    return tiles.ResidentSceneSet([tiles.ResidentScene(_arrays(nm, reps)[0], _arrays(nm, reps)[1], r, patch, pad, device=DEV)
                                   for nm, r in zip(NAMES, refs)], NAMES)


def _refs(reps=1):
    return [_arrays(nm, reps)[2] for nm in NAMES]


def _expected(host, cmap, items, thresh, write_color=True, start=None):
    """What the stitch must leave: ``(density[s], color[s], counts (S,4))`` from a NumPy loop over the tiles -- the density and
    the colour codes (metrics.changemap_codes' rules, the later one winning; detection only without a reference or with
    ``write_color`` off) go through ``MultiSceneDataset.write_center``, the cells are ``np.sum`` over the owned centre."""
    dens, col = (start if start is not None else (host.new_outputs(), host.new_outputs()))
    counts = np.zeros((len(host.scenes), 4), np.int64)
    thresh = np.float32(thresh)
    for pos, it in enumerate(items):
        s, cur = host.locate(it)
        scene = host.scenes[s]
        p = cmap[pos]
        with np.errstate(invalid='ignore'):
            pre = (p > thresh).astype(np.float32)                           # fp32 compare; a NaN is not above anything
        code = np.zeros_like(p)
        if scene.ref is not None:
            g = scene.grid.read_patch(scene.ref, cur, np.float32)
            r0, r1, c0, c1 = host.eff_range(it)
            win = (slice(None), slice(r0, r1), slice(c0, c1))
            for i in range(2):
                for j in range(2):
                    counts[s, 2 * i + j] += np.sum((g[win] == GT[i]) & (pre[win] == PRE[j]))
        if scene.ref is not None and write_color:
            code[(pre == PRE[0]) & (g == GT[1])] = 1
            code[(pre == PRE[1]) & (g == GT[0])] = 2
            code[(pre == PRE[1]) & (g == GT[1])] = 3
        else:
            code[pre == PRE[1]] = 1
        host.write_center(dens, p, it)
        host.write_center(col, code, it)
    return dens, col, counts


def _cmap(n, patch, seed, plant=True):
    """Seeded uniform density tiles (n,1,ph,pw); planted: elements exactly 0.5, exactly 0.25 and NaN."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (n, 1, patch[1], patch[0])).astype(np.float32)
    if plant:
        where = rng.uniform(0, 1, c.shape)
        c[where < 0.04] = 0.5
        c[(where >= 0.04) & (where < 0.08)] = 0.25
        c[(where >= 0.08) & (where < 0.12)] = np.nan
    return c


def _poisoned(res):
    maps = res.new_maps()
    assert float(maps.flat_density.abs().sum()) == 0 and float(maps.flat_color.abs().sum()) == 0        # zeroed
    maps.flat_density.fill_(float('nan'))
    maps.flat_color.fill_(float('nan'))
    return maps


def _check(maps, counts, want, what):
    dens, col, cnt = want
    for s in range(len(dens)):
        assert tuple(maps.density[s].shape) == dens[s].shape
        _eq(maps.density[s].cpu().numpy(), dens[s], '%s: density of scene %d' % (what, s))
        _eq(maps.color[s].cpu().numpy(), col[s], '%s: color of scene %d' % (what, s))
    _eq(counts.cpu().numpy(), cnt, '%s: per-scene counters' % what)


ALL = list(range(15))
# every item once, alternating between the two scenes (items 0..8 / 9..14) as long as the smaller one lasts
_rng = np.random.default_rng(5)
_A, _B = _rng.permutation(9).tolist(), (9 + _rng.permutation(6)).tolist()
MIXED = [v for pair in zip(_A, _B) for v in pair] + _A[6:]
assert sorted(MIXED) == ALL


# ============================================================================================= 1. the kernel against the host loop
@pytest.mark.parametrize('write_color', [True, False], ids=['color', 'detection'])
@pytest.mark.parametrize('thresh', [0.5, 0.25])
@pytest.mark.parametrize('items', [ALL, MIXED], ids=['in_order', 'mixed'])
def test_stitch_equals_the_host_loop(items, thresh, write_color):
    host, res = _host_set(_refs()), _resident_set(_refs())
    assert res.numlist == [9, 6] and res.table.offsets.tolist() == [0, 70 * 90, 70 * 90 + 55 * 48]
    cmap = _cmap(15, PATCH, 1)
    cm = torch.from_numpy(cmap).to(DEV)
    maps, counts = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    index = res.index(items)
    assert res.stitch(cm, index, maps, prob_thresh=thresh, gt_map=GT, pre_map=PRE, write_color=write_color,
                      scene_counts=counts) is maps
    want = _expected(host, cmap, items, thresh, write_color)
    _check(maps, counts, want, 'stitch')
    # the owned centres tile each scene exactly: no poison is left, the only NaNs are the planted ones
    assert not torch.isnan(maps.flat_color).any()
    assert int(torch.isnan(maps.flat_density).sum()) == sum(int(np.isnan(d).sum()) for d in want[0]) > 0
    assert int(counts.sum()) == 70 * 90 + 55 * 48                          # reference values are {1, 2}: every pixel in a cell
    # the sum of the rows = the existing kernel on the same tiles
    ev = metrics.Evaluator(2)
    ev.add_tiles(res.cut(index)[2], cm, res.rects(index), thresh, GT, PRE)
    _eq(counts.sum(0).cpu().numpy(), ev._dev_counts.cpu().numpy(), 'sum of the rows vs fcd_tile_confusion_items')
    # evaluators over the rows, without a copy
    row = metrics.Evaluator(2).attach_counts(counts[1])
    assert row._dev_counts.data_ptr() == counts[1].data_ptr()
    _eq(row._sync(), want[2][1].reshape(2, 2).astype(np.float64), 'evaluator over a row')


# ============================================================================================= 2. reference sample types
def test_reference_maps_of_integer_sample_types():
    refs = _refs()
    scenes = []
    for k, nm in enumerate(NAMES):
        x, y = (torch.from_numpy(a.astype(np.float32)).to(DEV) for a in _arrays(nm)[:2])
        if k == 0:
            r, rt = torch.from_numpy(refs[k].astype(np.uint8)).to(DEV), None
        else:                                                              # uint16 bits held in an int16 tensor
            r, rt = torch.from_numpy(refs[k].astype(np.uint16).view(np.int16)).to(DEV), ops.SAMPLE_U16
        scenes.append(tiles.ResidentScene.from_device(x, y, ref=r, patch_size=PATCH, overlap_padding=PAD, ref_type=rt))
    res = tiles.ResidentSceneSet(scenes, NAMES)
    assert [s.ref_type for s in res.scenes] == [ops.SAMPLE_U8, ops.SAMPLE_U16]
    cmap = _cmap(15, PATCH, 2)
    maps, counts = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    res.stitch(torch.from_numpy(cmap).to(DEV), MIXED, maps, scene_counts=counts)
    _check(maps, counts, _expected(_host_set(refs), cmap, MIXED, 0.5), 'integer reference maps')


# ============================================================================================= 3. a scene without a reference
def test_a_scene_without_a_reference():
    refs = [_refs()[0], None]
    host, res = _host_set(refs), _resident_set(refs)
    cmap = _cmap(15, PATCH, 3)
    cm = torch.from_numpy(cmap).to(DEV)
    maps, counts = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    res.stitch(cm, MIXED, maps, scene_counts=counts)
    want = _expected(host, cmap, MIXED, 0.5)
    _check(maps, counts, want, 'no reference for paris')
    assert want[2][1].sum() == 0 and want[2][0].sum() == 70 * 90          # its row stays zero
    assert set(np.unique(want[1][1])) == {0.0, 1.0}                        # detection only
    both = _expected(_host_set(_refs()), cmap, MIXED, 0.5)                 # the other scene does not notice
    _eq(maps.color[0].cpu().numpy(), both[1][0], 'abudhabi next to a scene without a reference')
    _eq(counts[0].cpu().numpy(), both[2][0], 'abudhabi next to a scene without a reference')
    # no counters at all: the maps alone
    maps2 = _poisoned(res)
    res.stitch(cm, MIXED, maps2)
    assert torch.equal(maps2.flat_color, maps.flat_color)
    assert torch.equal(torch.nan_to_num(maps2.flat_density, nan=-1.0), torch.nan_to_num(maps.flat_density, nan=-1.0))


# ============================================================================================= 4. batches
def test_ragged_batches_accumulate_to_one_launch():
    host, res = _host_set(_refs()), _resident_set(_refs())
    cmap = _cmap(15, PATCH, 4)
    sizes, extra = [5, 3, 6, 1], 2                                         # every batch drags two padded duplicates along
    flat, rows, at = [], [], 0
    for real in sizes:
        chunk = MIXED[at:at + real]
        flat += chunk + [chunk[0], MIXED[0]][:extra]
        rows.append(list(range(at, at + real)))
        at += real
    index = res.index(flat)
    maps, counts = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    at = 0
    for real, r in zip(sizes, rows):
        part = index[at:at + real + extra]
        assert len(part) == real + extra and part.host.tolist() == flat[at:at + real + extra]
        tiles_b = np.concatenate([cmap[r], np.full((extra,) + cmap.shape[1:], np.nan, np.float32)])       # pads: poison
        res.stitch(torch.from_numpy(tiles_b).to(DEV), part, maps, n=real, scene_counts=counts)
        at += real + extra
    want = _expected(host, cmap, MIXED, 0.5)
    _check(maps, counts, want, 'four launches')
    one, c1 = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    res.stitch(torch.from_numpy(cmap).to(DEV), MIXED, one, scene_counts=c1)
    assert torch.equal(c1, counts) and torch.equal(one.flat_color, maps.flat_color)


# ============================================================================================= 5. grid limits
def test_more_tiles_than_the_grid_holds():
    """722 tiles of 24x20 in a seeded order: two workgroups per tile and 256 tile slots, so every workgroup goes round the
    grid-stride loop three times and meets a change of scene inside it."""
    patch, pad = (24, 20), (2, 2)
    host, res = _host_set(_refs(5), patch, pad, 5), _resident_set(_refs(5), patch, pad, 5)
    n = len(res)
    assert res.numlist == [506, 216] and n > 512
    items = np.random.default_rng(6).permutation(n).tolist()
    cmap = _cmap(n, patch, 7, plant=False)
    maps, counts = _poisoned(res), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    res.stitch(torch.from_numpy(cmap).to(DEV), items, maps, scene_counts=counts)
    want = _expected(host, cmap, items, 0.5)
    _check(maps, counts, want, '722 tiles')
    assert not torch.isnan(maps.flat_density).any() and int(counts.sum()) == 25 * (70 * 90 + 55 * 48)


def test_map_offsets_beyond_2_to_the_31():
    """A small scene in front of a one-band 46400^2 uint8 scene (filled on the device, no host array): the big scene's last tile
    lands beyond element 2^31 of the flat maps."""
    S, patch, pad = 46400, (128, 128), (4, 4)
    grid = tiles.TileGrid(S, S, patch, pad)
    (x0, y0, w, h), _, _ = grid.slices(len(grid) - 1)
    assert x0 + w == S and y0 + h == S and 70 * 90 + y0 * S + x0 > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(3)
    small = torch.randint(1, 3, (1, 70, 90), dtype=torch.uint8, device=DEV, generator=gen)
    scene = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    block = torch.randint(1, 3, (h, w), dtype=torch.uint8, device=DEV, generator=gen)
    scene[0, y0:y0 + h, x0:x0 + w] = block
    res = tiles.ResidentSceneSet([
        tiles.ResidentScene.from_device(small, small, ref=small, patch_size=patch, overlap_padding=pad),
        tiles.ResidentScene.from_device(scene, scene, ref=scene, patch_size=patch, overlap_padding=pad)])
    assert len(res) == 1 + len(grid) and res.table.offsets.tolist() == [0, 6300, 6300 + S * S]
    maps, counts = res.new_maps(), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    cm = torch.rand((2, 1, 128, 128), device=DEV, generator=gen)
    res.stitch(cm, [len(res) - 1, 0], maps, scene_counts=counts)

    def rules(p, g):                                                       # the colour rules and the four cells, on the device
        pre = (p > 0.5).float()
        code = torch.zeros_like(p)
        code[(pre == 0) & (g == 2)] = 1
        code[(pre == 1) & (g == 1)] = 2
        code[(pre == 1) & (g == 2)] = 3
        return code, torch.stack([((g == GT[i]) & (pre == PRE[j])).sum() for i in range(2) for j in range(2)])
    p_big, p_small = cm[0, 0, 4:4 + h, 4:4 + w], cm[1, 0, 4:4 + 70, 4:4 + 90]
    code_big, cnt_big = rules(p_big, block.float())
    code_small, cnt_small = rules(p_small, small[0].float())
    assert torch.equal(maps.density[1][0, y0:, x0:], p_big) and torch.equal(maps.color[1][0, y0:, x0:], code_big)
    assert torch.equal(maps.density[0][0], p_small) and torch.equal(maps.color[0][0], code_small)
    assert torch.equal(counts, torch.stack([cnt_small, cnt_big]))
    # two untouched probes: the big scene's first row (right behind the small map) and the pixels left of the written window
    assert float(maps.flat_density[6300:6300 + S].abs().sum()) == 0 and float(maps.flat_color[6300:6300 + S].abs().sum()) == 0
    assert float(maps.density[1][0, y0:, x0 - 64:x0].abs().sum()) == 0 and float(maps.color[1][0, y0:, x0 - 64:x0].abs().sum()) == 0
    del scene, res, maps
    torch.cuda.empty_cache()


# ============================================================================================= 6. what the host refuses
def test_rejections_come_before_any_launch():
    res, other = _resident_set(_refs()), _resident_set(_refs())
    cm = torch.rand((4, 1, 32, 40), device=DEV)
    maps, counts = res.new_maps(), torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    bad = [
        ('appears 2 times', dict(index=res.index([0, 9, 0]), n=3)),                                   # a repeated item
        ('n = 4 with 3 indices', dict(index=res.index([0, 9, 1]), n=4)),                              # n too large
        ('n = 5', dict(index=res.index([0, 9, 1, 2, 3]), n=5)),                                       # more than there are tiles
        ('validated against it', dict(index=ops.TileIndex([0, 1], 16, DEV))),                         # an index of another table
        ('validated against it', dict(index=[0, 1])),
        ('maps must be', dict(maps=other.new_maps())),                                                # maps of another set
        ('maps must be', dict(maps=(maps.flat_density, maps.flat_color))),
        ('scene_counts must be', dict(scene_counts=torch.zeros(4, dtype=torch.int64, device=DEV))),   # shape
        ('scene_counts must be', dict(scene_counts=torch.zeros((2, 4), dtype=torch.int32, device=DEV))),    # dtype
        ('scene_counts must be', dict(scene_counts=torch.zeros((2, 4), dtype=torch.int64))),          # device
        ('scene_counts must be', dict(scene_counts=torch.zeros((4, 2), dtype=torch.int64, device=DEV).t())),
        ('cmap must be', dict(cmap=torch.rand((4, 1, 32, 32), device=DEV))),                          # another patch
        ('cmap must be', dict(cmap=torch.rand((4, 2, 32, 40), device=DEV))),
    ]
    for what, kw in bad:
        args = dict(cmap=cm, descs=res._descs, table=res.table, index=res.index([0, 9, 1]), maps=maps, scene_counts=counts)
        args.update(kw)
        with pytest.raises(_lib.FcdError, match=what):
            ops.scene_set_stitch(**args)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.scene_set_stitch(cm.cpu(), res._descs, res.table, res.index([0, 9, 1]), maps)
    assert float(maps.flat_density.abs().sum()) == 0 and float(maps.flat_color.abs().sum()) == 0 and int(counts.sum()) == 0
    res.stitch(cm, [0, 9, 1, 0], maps, n=3, scene_counts=counts)           # the repeat is a padded duplicate: fine
    assert int(counts.sum()) > 0


# ============================================================================================= 7. the two inference routes
def _stats(k):
    rng = np.random.default_rng(100 + k)
    return (rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4), rng.uniform(500, 3000, 4), rng.uniform(300, 1500, 4))


@functools.lru_cache(maxsize=None)
def _infer_pair(with_region=False):
    """(host MultiSceneDataset, ResidentSceneSet) over the two fixture scenes repeated 4 x 4 (280x360 and 220x192) in 176-pixel
    tiles: 6 + 4 tiles, so the second batch of four holds tiles of both scenes.  Shared, never modified."""
    host, res = [], []
    for k, nm in enumerate(NAMES):
        x, y, ref, region = _arrays(nm, 4)
        region = region if with_region else None
        host.append(datasets.RegionTileDataset(x, y, region=region, ref=ref, patch_size=(TILE, TILE), overlap_padding=(4, 4),
                                               stats=_stats(k)))
        res.append(tiles.ResidentScene(x, y, ref, (TILE, TILE), (4, 4), stats=_stats(k), device=DEV, region=region))
    return datasets.MultiSceneDataset(host, NAMES), tiles.ResidentSceneSet(res, NAMES)


PIXELS = 16 * (70 * 90 + 55 * 48)


def _net():
    torch.manual_seed(1234)
    return Module.Segmentor(4, bilinear=True).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _host_result(eval_mode):
    """``infer_scene_set`` on the seeded Segmentor and the net it left behind: computed once, shared, never modified."""
    net = _net()
    return demos.infer_scene_set(net, _infer_pair()[0], DEV, batch_size=4, eval_mode=eval_mode), net


def _same_result(got, want, what):
    assert got['names'] == want['names'] == NAMES
    for s in range(2):
        assert got['density'][s].dtype == np.float32 and got['density'][s].shape == want['density'][s].shape
        _eq(got['density'][s], want['density'][s], '%s: density of scene %d' % (what, s))
        _eq(got['color'][s], want['color'][s], '%s: color of scene %d' % (what, s))
    cms = [(g._sync(), w._sync()) for g, w in zip(got['scene_evaluators'], want['scene_evaluators'])]
    for s, (g, w) in enumerate(cms):
        _eq(g, w, '%s: counts of scene %d' % (what, s))
    total = got['evaluator']._sync()
    _eq(total, want['evaluator']._sync(), '%s: overall counts' % what)
    _eq(total, cms[0][0] + cms[1][0], '%s: the overall matrix is the sum of the scenes' % what)
    assert total.sum() == PIXELS and [c[0].sum() for c in cms] == [16 * 70 * 90, 16 * 55 * 48]


@pytest.mark.parametrize('eval_mode', [True, False], ids=['eval', 'train'])
def test_infer_scene_set_resident_equals_infer_scene_set(eval_mode):
    host, res = _infer_pair()
    assert res.numlist == host.numlist == [6, 4]
    want, host_net = _host_result(eval_mode)
    net = _net()
    got = demos.infer_scene_set_resident(net, res, DEV, batch_size=4, eval_mode=eval_mode)
    _same_result(got, want, 'resident vs host')
    assert not net.training and not host_net.training
    buffers = list(zip(net.named_buffers(), host_net.named_buffers()))
    assert buffers
    for (name, a), (_, b) in buffers:
        assert torch.equal(a, b), name                                     # the train-mode pass moved them alike
    moved = any(not torch.equal(a, b) for (_, a), (_, b) in zip(net.named_buffers(), _net().named_buffers()))
    assert moved == (not eval_mode)
    with pytest.raises(TypeError):
        demos.infer_scene_set_resident(net, host, DEV)
    with pytest.raises(TypeError):
        demos.infer_scene_set(net, res, DEV)


@pytest.mark.parametrize('route', ['resident', 'host'])
def test_score_only(route):
    host, res = _infer_pair()
    want, _ = _host_result(False)
    fn, ds = (demos.infer_scene_set_resident, res) if route == 'resident' else (demos.infer_scene_set, host)
    got = fn(_net(), ds, DEV, batch_size=4, eval_mode=False, score_only=True)
    assert got['density'] is None and got['color'] is None and got['names'] == NAMES
    cm = got['evaluator']._sync()
    _eq(cm, want['evaluator']._sync(), 'score_only vs the full pass')
    assert cm.sum() == PIXELS


def test_infer_scene_set_resident_with_a_forced_one_rank_exchange(tmp_path):
    """One rank cannot show a cross-rank sum, but it does send the flat maps, the BatchNorm buffers and the counters through the
    collectives: a one-rank sum is the identity, so nothing may change by a bit."""
    import torch.distributed as dist
    _, res = _infer_pair()
    want, _ = _host_result(True)
    with _lib.switched(DP_FORCE_EXCHANGE=1):
        prev = dp.force_exchange(bool(_lib.switch('DP_FORCE_EXCHANGE')))
        dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
        try:
            assert dp.exchanging() == 1
            got = demos.infer_scene_set_resident(_net(), res, DEV, batch_size=4)
            for ev in got['scene_evaluators'] + [got['evaluator']]:
                ev._sync()
        finally:
            dist.destroy_process_group()
            dp.force_exchange(prev)
    _same_result(got, want, 'one-rank exchange')


# ============================================================================================= 8. end to end
def test_demo_rsss_with_a_test_set(tmp_path):
    host, res = _infer_pair(True)
    kw = dict(epochs_g=1, epochs_adv=2, init_batch_size=3, batch_size=3, allow_seeded=True, test_batch_size=4)
    out = demos.demo_rsss(res, test_dataset=res, out_dir=str(tmp_path), **kw)
    hist, test = out['history'], out['test']
    assert len(hist['test']) == 2 and len(hist['adv']) == 2
    for row in hist['test']:
        assert sorted(row) == sorted(['OA', 'Kappa', 'precision', 'recall', 'F1', 'mIoU', 'cIoU'])
        assert all(np.isfinite(v) for v in row.values()), row
    assert test['evaluator']._sync().sum() == PIXELS
    assert sorted(os.listdir(str(tmp_path))) == sorted('%s_%s.tif' % (nm, k) for nm in NAMES for k in ('density', 'binary'))
    for s, nm in enumerate(NAMES):
        _eq(tiles.read_tiff(str(tmp_path / ('%s_density.tif' % nm))), test['density'][s], 'density TIFF of ' + nm)
        _eq(tiles.read_tiff(str(tmp_path / ('%s_binary.tif' % nm))), test['color'][s], 'binary TIFF of ' + nm)
    # the same run with the test set held on the host
    out_h = demos.demo_rsss(res, test_dataset=host, **kw)
    assert out_h['history']['test'] == hist['test']
    for s in range(2):
        _eq(out_h['test']['density'][s], test['density'][s], 'final density, host test set, scene %d' % s)
        _eq(out_h['test']['color'][s], test['color'][s], 'final color, host test set, scene %d' % s)
    # without a test set: today's keys
    plain = demos.demo_rsss(res, epochs_g=0, epochs_adv=1, batch_size=3, allow_seeded=True)
    assert sorted(plain) == sorted(['netS', 'netD', 'netG', 'history', 'evaluator', 'vgg_pretrained'])
    assert sorted(plain['history']) == ['adv', 'g']
    with pytest.raises(TypeError, match='test_dataset'):
        demos.demo_rsss(res, epochs_g=0, epochs_adv=0, allow_seeded=True, test_dataset=res.scenes[0])
