"""Host side of inference over a scene set (fcd_scene_set_stitch): the offsets of the per-scene maps inside the two flat
buffers and the check that no item is stitched twice in one launch.  Pure host code: no device, no kernel."""
import numpy as np
import pytest

from fcd_gan_pytorch_amd import _lib, _ops as ops, tiles

PATCH, PAD = (40, 32), (4, 3)
GRIDS = [tiles.TileGrid(90, 70, PATCH, PAD), tiles.TileGrid(48, 55, PATCH, PAD), tiles.TileGrid(7, 3, PATCH, PAD)]
SIZES = [(90, 70), (48, 55), (7, 3)]


def test_map_offsets_of_grids_of_unequal_size():
    off = ops.scene_map_offsets(GRIDS)
    assert off.dtype == np.int64 and off.tolist() == [0, 6300, 6300 + 2640, 6300 + 2640 + 21]
    assert ops.scene_map_offsets(SIZES).tolist() == off.tolist()           # (W, H) pairs serve as well
    ops.validate_map_offsets(off, SIZES)
    ops.validate_map_offsets(off, GRIDS)
    assert ops.scene_map_offsets(GRIDS[:1]).tolist() == [0, 6300]
    big = ops.scene_map_offsets([(46400, 46400), (90, 70)])                # no 32-bit arithmetic on the way
    assert big.tolist() == [0, 46400 * 46400, 46400 * 46400 + 6300] and big[1] > 2 ** 31


def test_the_set_table_carries_the_offsets_of_its_grids():
    table = ops.scene_set_table(GRIDS[:2])
    assert table.offsets.tolist() == [0, 6300, 8940] and table.sizes == SIZES[:2]
    assert len(table) == 9 + 6


@pytest.mark.parametrize('offsets,what', [
    ([1, 6301, 8941, 8962], 'start at 0'),                                 # a non-zero start
    ([0, 6300, 8941, 8962], 'spans'),                                      # a span that differs from H*W
    ([0, 6299, 8940, 8961], 'spans'),
    ([0, 6300, 3660, 3681], 'decreasing'),                                 # a decreasing array
    ([0, 6300, 8940], 'expected 4'),                                       # a wrong length
    ([0, 6300, 8940, 8961, 8961], 'expected 4'),
    ([[0, 6300, 8940, 8961]], 'expected 4'),
    (np.array([0, 6300, 8940, 8961], np.float64), 'expected 4'),           # not integers
])
def test_validate_map_offsets_rejects(offsets, what):
    with pytest.raises(_lib.FcdError, match=what):
        ops.validate_map_offsets(np.asarray(offsets), SIZES)


def test_repeated_items_are_rejected_among_the_first_n_only():
    items = np.array([0, 9, 3, 14, 3, 10], np.int32)
    ops.check_unique_items(items, 4)                                       # the repeat is a trailing padded duplicate
    ops.check_unique_items(items[:4], 4)
    with pytest.raises(_lib.FcdError, match='item 3 appears 2 times among the first 5'):
        ops.check_unique_items(items, 5)
    with pytest.raises(_lib.FcdError, match='item 3 appears 2 times'):
        ops.check_unique_items(items, 6)
    for n in (0, -1, 7):
        with pytest.raises(_lib.FcdError, match='n = %d with 6 indices' % n):
            ops.check_unique_items(items, n)
    ops.check_unique_items(np.arange(1000)[::-1], 1000)
