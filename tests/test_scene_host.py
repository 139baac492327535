"""Host side of the device-resident scene inference (csrc/scene.hip): the tile table the kernels read is
``TileGrid.slices`` row for row -- pinned by the arrays the reference's own GDALDataset produced (tests/golden/tiles.npz,
``<tag>/slices``) -- and every row is validated on the host before anything is uploaded, so a kernel can never be handed a
rectangle that leaves its buffers.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, tiles

G = os.path.join(os.path.dirname(__file__), 'golden', 'tiles.npz')


def _grid(z, tag):
    nb, ys, xs, pw, ph, padx, pady, n = [int(v) for v in z[tag + '/meta']]
    return tiles.TileGrid(xs, ys, (pw, ph), (padx, pady)), n


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd'])
def test_tile_table_is_the_reference_slices(tag):
    z = np.load(G)
    grid, n = _grid(z, tag)
    table = ops.scene_tile_table(grid, range(n))
    assert table.rows.dtype == np.int32 and table.rows.shape == (n, 12) and len(table) == n
    np.testing.assert_array_equal(table.rows, z[tag + '/slices'].astype(np.int32))
    assert table.geom == (grid.xsize, grid.ysize) + grid.patch_size + grid.pad
    # any subset / order / duplicates (the padded last batch of a data-parallel rank) are rows of the same table
    pick = [n - 1, 0, 0]
    np.testing.assert_array_equal(ops.scene_tile_table(grid, pick).rows, z[tag + '/slices'][pick].astype(np.int32))


class _BentGrid(tiles.TileGrid):
    """A TileGrid whose ``slices`` is off by ``delta`` in one of its 12 numbers (or whose pad is larger than the one the tiles
    were laid out with) -- what a bug in the tiling arithmetic would hand the kernels."""

    def __init__(self, *a, column=None, delta=0, **k):
        super().__init__(*a, **k)
        self.column, self.delta = column, delta

    def slices(self, item):
        flat = sum((list(t) for t in super().slices(item)), [])
        if self.column is not None:
            flat[self.column] += self.delta
        return tuple(flat[0:4]), tuple(flat[4:8]), tuple(flat[8:12])


X0, Y0, OW, OH, RX, RY, RW, RH, WX, WY, WW, WH = range(12)


@pytest.mark.parametrize('column,delta,what', [
    (RX, 1, 'read rectangle leaves the scene'),          # rx + rw > W on the right-most tiles
    (RY, 3, 'read rectangle leaves the scene'),
    (WY, 1, 'canvas window leaves the patch'),           # wy + wh > ph on the full-height tiles
    (WX, 2, 'canvas window leaves the patch'),
    (RX, -1, 'negative'),                                # negative origin on the left-most tiles
    (WY, -6, 'negative'),
    (Y0, -1, 'negative'),
    (X0, 2, 'owned rectangle leaves the scene'),
    (OH, 1, 'owned rectangle'),                          # leaves the scene at the bottom or, shifted by the pad, the patch
])
def test_tile_table_validation_rejects_out_of_range_rows(column, delta, what):
    grid = _BentGrid(131, 97, (40, 40), (5, 5), column=column, delta=delta)
    with pytest.raises(_lib.FcdError, match=what):
        ops.scene_tile_table(grid, range(len(grid)))


def test_tile_table_validation_wants_window_and_read_rectangle_of_one_size():
    # the cut kernel reads ww x wh elements from (rx, ry): a wider read rectangle that still fits the scene is a bent row too
    grid = _BentGrid(131, 97, (40, 40), (5, 5), column=RW, delta=1)
    with pytest.raises(_lib.FcdError, match='differ in size'):
        ops.scene_tile_table(grid, [0, 1])


def test_tile_table_validation_of_the_pad_shift():
    """The stitch kernel reads cmap[pady + j][padx + i] for j < h, i < w: an owned rectangle that fits the scene but, shifted by
    the pad, leaves the canvas must be refused (here: rows laid out for pad 5 used with pad 11: 11 + 30 > 40)."""
    rows = ops.scene_tile_table(tiles.TileGrid(131, 97, (40, 40), (5, 5)), range(20)).rows
    ops.validate_tile_rows(rows, 131, 97, 40, 40, 5, 5)
    with pytest.raises(_lib.FcdError, match='shifted by the pad'):
        ops.validate_tile_rows(rows, 131, 97, 40, 40, 11, 5)
    with pytest.raises(_lib.FcdError, match='shifted by the pad'):
        ops.validate_tile_rows(rows, 131, 97, 40, 40, 5, 11)
    with pytest.raises(_lib.FcdError, match=r'\(n,12\)'):
        ops.validate_tile_rows(rows[:, :11], 131, 97, 40, 40, 5, 5)
    with pytest.raises(_lib.FcdError):
        ops.validate_tile_rows(rows[:0], 131, 97, 40, 40, 5, 5)


def test_scene_ops_reject_host_tensors_and_foreign_tables():
    grid = tiles.TileGrid(50, 64, (32, 24), (4, 3))
    table = ops.scene_tile_table(grid, range(len(grid)))
    sx = torch.zeros((2, 64, 50), dtype=torch.uint8)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.scene_cut(sx, sx, table)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        table.to('cpu')
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        tiles.ResidentScene(np.zeros((2, 64, 50), np.uint8), np.zeros((2, 64, 50), np.uint8), device='cpu')
    with pytest.raises(_lib.FcdError, match='uint8, uint16 or float32'):
        tiles.ResidentScene(np.zeros((2, 64, 50), np.float64), np.zeros((2, 64, 50), np.float64))
    with pytest.raises(ValueError):
        tiles.ResidentScene(np.zeros((2, 64, 50), np.uint8), np.zeros((2, 64, 51), np.uint8))
    cm = torch.zeros((len(grid), 1, 24, 32))
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.scene_stitch(cm, table, torch.zeros((1, 64, 50)), torch.zeros((1, 64, 50)))
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.tile_confusion(cm, cm, [grid.eff_range(0)], torch.zeros(4, dtype=torch.int64))


def test_c_abi_refuses_bad_scene_arguments_without_launching():
    lib = _lib.lib
    # sample type 7 does not exist; pointers are never dereferenced on the host
    rc = lib.fcd_scene_cut(16, 16, 7, None, 0, 4, 8, 8, 16, 1, 8, 8, None, 16, 16, None, None, None)
    assert rc == -1 and b'sample type' in lib.fcd_last_error_string()
    rc = lib.fcd_scene_cut(16, 16, 0, 16, 0, 4, 8, 8, 16, 1, 8, 8, None, 16, 16, None, None, None)     # ref without ref tiles
    assert rc == -1 and b'go together' in lib.fcd_last_error_string()
    rc = lib.fcd_scene_stitch(16, 16, 1, 8, 8, 4, 0, 0.5, 1, 2, 0, 1, 1, None, 8, 8, 16, 16, None, None)    # 2 * padx >= pw
    assert rc == -1 and b'bad arguments' in lib.fcd_last_error_string()
    rc = lib.fcd_tile_confusion(16, 16, 16, 1, 8, 8, 0.5, 1, 2, 0, 1, None, None)                          # no counter
    assert rc == -1 and b'bad arguments' in lib.fcd_last_error_string()
