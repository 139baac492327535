"""Host side of the device-resident training feed (tiles.ResidentSceneSet, _ops.scene_stats / scene_set_cut): the exact-moment
helper the GPU tests use as their truth, pinned against what the reference wrote (tests/golden/stats.npz); the statistics text
cache; the validation of a scene set's tile table; the epoch plan against dp.RankStridedBatches; and the C ABI's argument
checks.  Nothing here needs a GPU."""
import ctypes
import fractions
import math
import os
import types

import numpy as np
import pytest

from fcd_gan_pytorch_amd import _lib, _ops as ops, dp, tiles

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
ULP32_2 = 2.0 ** -22          # two fp32 ulps, relative: the reference rounds its tile means and its result to fp32


def exact_stats(x, y, patch, pad):
    """CommonFunc.Dataset_mean / Dataset_std (CommonFunc.py:436-500) in exact arithmetic: over every tile of the
    (patch, pad) tiling, the pixels of the read rectangle whose band sum of x is non-zero; mean = S1 / n and
    std = sqrt((n S2 - S1^2) / (n (n - 1))) as rationals of Python integers, rounded to fp64 at the very end.
    x, y: (C,H,W) integer arrays.  Returns ((meanX, stdX, meanY, stdY) as (4,C) float64, n)."""
    C, H, W = x.shape
    grid = tiles.TileGrid(W, H, patch, pad)
    n, s1, s2 = 0, [[0] * C, [0] * C], [[0] * C, [0] * C]
    for item in range(len(grid)):
        _, (rx, ry, rw, rh), _ = grid.slices(item)
        bx = x[:, ry:ry + rh, rx:rx + rw].astype(np.int64)
        by = y[:, ry:ry + rh, rx:rx + rw].astype(np.int64)
        valid = bx.sum(axis=0) != 0
        n += int(valid.sum())
        for k, b in enumerate((bx, by)):
            for c in range(C):
                v = [int(t) for t in b[c][valid]]
                s1[k][c] += sum(v)
                s2[k][c] += sum(t * t for t in v)
    out = np.empty((4, C), np.float64)
    for k in range(2):
        for c in range(C):
            out[2 * k, c] = float(fractions.Fraction(s1[k][c], n))
            out[2 * k + 1, c] = math.sqrt(float(fractions.Fraction(n * s2[k][c] - s1[k][c] ** 2, n * (n - 1))))
    return out, n


def stats_case(tag):
    z = np.load(os.path.join(GOLDEN, 'stats.npz'))
    nb, ys, xs, pw, ph, ox, oy = [int(v) for v in z[tag + '/meta']]
    return z[tag + '/x'], z[tag + '/y'], (pw, ph), (ox, oy), z[tag + '/mean_std']


@pytest.mark.parametrize('tag,count', [('s1', 8934), ('s2', 5609)])
def test_exact_moments_agree_with_the_reference_written_statistics(tag, count):
    x, y, patch, pad, fixture = stats_case(tag)
    got, n = exact_stats(x, y, patch, pad)
    assert n == count
    rel = np.abs(got - fixture) / np.abs(fixture)
    print('\n[stats] %s: exact moments vs the reference-written fixture, max rel %.3e' % (tag, rel.max()))
    assert rel.max() <= ULP32_2
    # the conversion the device route uses on its integer totals is the same arithmetic
    m, s = ops._exact_meanstd(4, 1 + 2 + 3 + 6, 1 + 4 + 9 + 36)
    assert m == 3.0 and s == math.sqrt(14 / 3)


def test_scene_meanstd_round_trip_is_exact_and_cross_readable(tmp_path):
    vals = (np.array([1977.6169590329078, 1 / 3]), np.array([1144.8944091796875, 2 ** -40]),
            np.array([2007.1130263223273, 1e300]), np.array([1161.8195800781251, 5e-324]))
    scene = types.SimpleNamespace(statistics=lambda overlap_padding=(0, 0): vals)
    tx, ty = str(tmp_path / 'x.txt'), str(tmp_path / 'y.txt')
    first = tiles.scene_meanstd(tx, ty, scene)
    for a, b in zip(first, vals):
        assert a == b.tolist()
    assert open(tx).read().split()[0] == 'mean:' and open(tx).read().splitlines()[1].startswith('std:')
    scene.statistics = None                                              # the second call must read the files
    again = tiles.scene_meanstd(tx, ty, scene)
    assert again == first                                                # exact: repr round-trips every float
    assert tuple(tiles.dataset_meanstd(tx, ty, None)) == again           # dataset_meanstd reads what scene_meanstd wrote
    # and the other way round: a cache written by dataset_meanstd loads in scene_meanstd
    x, y, patch, pad, _ = stats_case('s1')
    ds = tiles.PairTileDataset(x, y, None, patch, pad)
    ux, uy = str(tmp_path / 'ux.txt'), str(tmp_path / 'uy.txt')
    wrote = tiles.dataset_meanstd(ux, uy, ds)
    assert tuple(tiles.scene_meanstd(ux, uy, None)) == tuple(tiles.dataset_meanstd(ux, uy, ds))
    np.testing.assert_array_equal(np.array(tiles.scene_meanstd(ux, uy, None)), np.array(wrote))


def _set_rows(sizes, patch=(40, 32), pad=(4, 3)):
    grids = [tiles.TileGrid(w, h, patch, pad) for w, h in sizes]
    return ops.scene_set_table(grids)


def test_set_table_validation():
    sizes = [(90, 70), (48, 55)]
    table = _set_rows(sizes)
    assert len(table) == 15 and table.rows.shape == (15, 13) and table.rects.shape == (15, 4)
    assert table.rows[:, 12].tolist() == [0] * 9 + [1] * 6
    ops.validate_set_rows(table.rows, sizes, 40, 32, 4, 3)
    rows = table.rows.copy()
    rows[10, 12] = 0                 # a tile of paris attributed to abudhabi is fine (it fits), the reverse is not
    ops.validate_set_rows(rows, sizes, 40, 32, 4, 3)
    rows = table.rows.copy()
    rows[8, 12] = 1                  # the last tile of abudhabi (90 wide) read from paris (48 wide)
    with pytest.raises(_lib.FcdError, match='scene 1 of the set.*leaves the scene'):
        ops.validate_set_rows(rows, sizes, 40, 32, 4, 3)
    for bad in (2, -1):
        rows = table.rows.copy()
        rows[3, 12] = bad
        with pytest.raises(_lib.FcdError, match='scene index'):
            ops.validate_set_rows(rows, sizes, 40, 32, 4, 3)
        with pytest.raises(_lib.FcdError, match='scene index'):
            ops.SceneSetTable(rows, table.rects, sizes, (40, 32), (4, 3))
    with pytest.raises(_lib.FcdError, match=r'\(T,13\)'):
        ops.validate_set_rows(table.rows[:, :12], sizes, 40, 32, 4, 3)
    rects = table.rects.copy()
    rects[0, 1] = 33
    with pytest.raises(_lib.FcdError, match='rectangle'):
        ops.SceneSetTable(table.rows, rects, sizes, (40, 32), (4, 3))

    def scene(bands=4, sample_type=ops.SAMPLE_U16, patch=(40, 32), pad=(4, 3), device='cuda:0'):
        return types.SimpleNamespace(bands=bands, sample_type=sample_type, device=device,
                                     grid=tiles.TileGrid(64, 64, patch, pad))
    tiles.check_scene_set([scene(), scene()])
    for what, other in (('band count', scene(bands=1)), ('sample type', scene(sample_type=ops.SAMPLE_U8)),
                        ('patch size', scene(patch=(32, 32))), ('overlap padding', scene(pad=(4, 4)))):
        with pytest.raises(_lib.FcdError, match=what):
            tiles.check_scene_set([scene(), other])
    with pytest.raises(_lib.FcdError, match='patch size and padding'):
        ops.scene_set_table([tiles.TileGrid(64, 64, (40, 32), (4, 3)), tiles.TileGrid(64, 64, (32, 32), (4, 3))])
    with pytest.raises(_lib.FcdError):
        tiles.check_scene_set([])
    # an index list is validated against the table before it is uploaded (no device is touched when it is wrong)
    for items in ([0, 15], [-1], []):
        with pytest.raises(_lib.FcdError, match='tile index'):
            ops.TileIndex(items, 15, 'cuda')
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.TileIndex([0, 1], 15, 'cpu')


@pytest.mark.parametrize('ragged', ['pad', 'drop', 'weighted'])
@pytest.mark.parametrize('rank,world', [(0, 1), (0, 2), (1, 2)])
def test_epoch_plan_equals_rank_strided_batches(ragged, rank, world):
    for n, batch, seed, shuffle in ((15, 4, 5, True), (15, 4, 5, False), (9, 2, 1007, True), (5, 4, 3, True), (8, 4, 0, True)):
        sampler = dp.RankStridedBatches(n, batch, seed=seed, shuffle=shuffle, rank=rank, world=world, ragged=ragged)
        want = [list(b) for b in sampler]
        plan = tiles.EpochPlan(n, batch, seed, shuffle=shuffle, ragged=ragged, rank=rank, world=world)
        assert plan.batches == want and plan.pads == sampler.pads and plan.scales == sampler.scales
        assert len(plan) == len(want) == len(sampler)
        assert plan.flat == [i for b in want for i in b]
        assert [plan.flat[plan.offsets[b]:plan.offsets[b + 1]] for b in range(len(plan))] == want
        assert all(0 <= i < n for i in plan.flat)


def test_scene_entry_points_validate_their_arguments_without_launching():
    lib = _lib.lib
    P = ctypes.c_void_p
    a = P(4096)                      # a non-null address that is never dereferenced: every call below fails its checks first
    err = lambda: lib.fcd_last_error_string()
    ok_stats = dict(x=a, y=a, st=1, C=4, H=64, W=64, table=a, n=2, ph=32, pw=32, out=a, ws=None, wsb=0, stream=None)

    def stats(**kw):
        k = dict(ok_stats, **kw)
        return lib.fcd_scene_stats(k['x'], k['y'], k['st'], k['C'], k['H'], k['W'], k['table'], k['n'], k['ph'], k['pw'], k['out'],
                                   k['ws'], k['wsb'], k['stream'])
    assert stats(x=None) == -1 and b'fcd_scene_stats: bad arguments' in err()
    assert stats(n=0) == -1 and b'bad arguments' in err()
    assert stats(st=3) == -1 and b'sample type 3' in err()
    assert stats(C=33) == -1 and b'at most 32' in err()
    assert stats(n=2 ** 31 - 1, ph=2 ** 15, pw=2 ** 15) == -1 and b'2^64' in err()         # n ph pw 65535^2 >= 2^64
    assert stats(st=2) == -1 and b'workspace' in err()                                      # float32 without its workspace
    assert lib.fcd_scene_stats_ws_bytes(1, 4, 2, 32) == 0                                   # integer scenes need none
    need = lib.fcd_scene_stats_ws_bytes(2, 4, 2, 32)
    assert need > 0 and need % (8 * (1 + 2 * 4)) == 0                                       # whole partial rows of 1 + 2C doubles
    assert lib.fcd_scene_stats_ws_bytes(2, 33, 2, 32) == 0
    assert stats(st=2, ws=a, wsb=need - 8) == -1 and b'workspace' in err()

    def cut(descs=a, S=2, st=1, C=4, table=a, T=15, index=a, n=3, ph=32, pw=40, x=a, y=a):
        return lib.fcd_scene_set_cut(descs, S, st, C, table, T, index, n, ph, pw, None, x, y, None, None, None, None)
    assert cut(descs=None) == -1 and b'fcd_scene_set_cut: bad arguments' in err()
    assert cut(index=None) == -1 and cut(T=0) == -1 and cut(S=0) == -1 and cut(y=None) == -1
    assert cut(st=7) == -1 and b'sample type 7' in err()
    assert cut(n=2 ** 30, C=4) == -1 and b'exceed 2^31 - 1' in err()
    assert lib.fcd_tile_confusion_items(a, a, a, 0, a, 1, 8, 8, 0.5, 0, 1, 0, 1, a, None) == -1
    assert b'fcd_tile_confusion_items: bad arguments' in err()
    assert ctypes.sizeof(ctypes.c_int64) * ops.SCENE_DESC_COLS == 64                        # fcd_scene_desc, as _ops lays it out
