"""Region maps from a change map, host side (no GPU): the NumPy oracle ``tiles.region_map_host`` against the scipy-written
fixture tests/golden/regions.npz and against scipy itself, the C ABI's argument validation (csrc/regions.hip refuses before it
launches), the workspace bound, and the label.txt helpers of BuildingProcess.py:129,167."""
import ctypes
import functools
import os

import numpy as np
import pytest

from fcd_gan_pytorch_amd import _lib, tiles

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, 'regions.npz'))
    return {k: z[k] for k in z.files}


def case(name):
    """(map, thresh, slice or None, connectivities) of a fixture case."""
    z = fixture()
    sl = tuple(int(v) for v in z[name + '/slice'])
    return z[name + '/map'], float(z[name + '/thresh']), (sl if sl[0] else None), [int(c) for c in z[name + '/conns']]


CASES = [str(n) for n in fixture()['cases']]
EXPANDS = [int(e) for e in fixture()['expands']]


def test_fixture_holds_the_cases():
    z = fixture()
    assert set(CASES) >= {'one_fg', 'one_bg', 'row300', 'col300', 'rand01', 'rand05', 'checker', 'all_fg', 'all_bg', 'serpentine',
                          'spiral', 'diagonals', 'edges16', 'sliced', 'u16', 'f32'}
    assert EXPANDS == [0, 3, 10, 500]
    assert len(z['checker/boxes1']) == (131 * 197 + 1) // 2 and len(z['checker/boxes2']) == 1
    assert z['u16/map'].dtype == np.uint16 and z['f32/map'].dtype == np.float32 and np.isnan(z['f32/map']).any()
    assert case('sliced')[2] == (50, 64)


@pytest.mark.parametrize('name', CASES)
def test_host_oracle_equals_the_fixture(name):
    z = fixture()
    m, thresh, sl, conns = case(name)
    with np.errstate(invalid='ignore'):
        fg = m.astype(np.float64) > thresh
    for c in conns:
        lab, K = tiles.label_components_host(fg, c, sl)
        np.testing.assert_array_equal(lab, z['%s/labels%d' % (name, c)])
        np.testing.assert_array_equal(tiles.component_boxes_host(lab, K), z['%s/boxes%d' % (name, c)])
    for e in EXPANDS:
        got = tiles.region_map_host(m[None], expand=e, thresh=thresh, slice=sl)
        assert got.dtype == np.uint8 and got.shape == (1,) + m.shape
        np.testing.assert_array_equal(got[0], z['%s/region%d' % (name, e)])


@pytest.mark.parametrize('seed,shape,density', [(5, (83, 120), 0.35), (6, (150, 61), 0.6)])
def test_host_oracle_equals_scipy(seed, shape, density):
    ndimage = pytest.importorskip('scipy.ndimage')
    fg = np.random.default_rng(seed).random(shape) < density
    for c, structure in ((1, None), (2, np.ones((3, 3)))):
        want, K = ndimage.label(fg, structure=structure)
        lab, k = tiles.label_components_host(fg, c)
        assert k == K
        np.testing.assert_array_equal(lab, want)
        boxes = np.array([[s[0].start, s[1].start, s[0].stop, s[1].stop] for s in ndimage.find_objects(want)])
        np.testing.assert_array_equal(tiles.component_boxes_host(lab, k), boxes)
    want = np.zeros(shape, np.uint8)                       # OSCDProcess.py:62-73 on the connectivity-2 boxes
    for min_y, min_x, max_y, max_x in boxes:
        want[max(min_y - 10, 0):min(max_y + 10, shape[0]), max(min_x - 10, 0):min(max_x + 10, shape[1])] = 255
    np.testing.assert_array_equal(tiles.region_map_host(fg.astype(np.uint8) * 2, thresh=1)[0], want)


def test_region_map_host_never_touches_the_device(monkeypatch):
    from fcd_gan_pytorch_amd import _ops
    for fn in ('label_components', 'component_boxes', 'region_paint'):
        monkeypatch.setattr(_ops, fn, lambda *a, **k: pytest.fail('the host oracle called the device'))
    assert tiles.region_map_host(np.eye(5, dtype=np.float32), expand=1).tolist() == [np.full((5, 5), 255).tolist()]


# ---- C ABI: refused before anything is launched -------------------------------------------------------------------------
P = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused by the argument checks


def _refused(rc, *words):
    msg = _lib.lib.fcd_last_error_string().decode()
    assert rc == -1, msg
    for w in words:
        assert w in msg, msg


def test_cabi_argument_validation_without_gpu():
    lib = _lib.lib
    label = lambda H, W, st=0, conn=2, sh=0, sw=0, ws=1 << 20: lib.fcd_label_components(P, st, H, W, 0.0, conn, sh, sw, P, P, P, ws, None)
    _refused(label(1 << 16, 1 << 15), 'fcd_label_components', '2^31')
    _refused(label(46341, 46341), 'fcd_label_components', '2^31')
    _refused(label(8, 8, conn=3), 'connectivity 3')
    _refused(label(8, 8, conn=0), 'connectivity 0')
    _refused(label(8, 8, st=3), 'sample type 3')
    _refused(label(8, 8, st=-1), 'sample type -1')
    _refused(label(8, 8, sh=4, sw=0), 'slice 4 x 0')
    _refused(label(8, 8, sh=0, sw=4), 'slice 0 x 4')
    _refused(label(8, 8, sh=-2, sw=-2), 'slice')
    _refused(label(64, 64, ws=0), 'workspace')
    _refused(label(0, 8), 'bad arguments')
    paint = lambda e, sh=0, sw=0, H=8, W=8: lib.fcd_region_paint(P, 1, H, W, e, sh, sw, P, None)
    _refused(paint(-1), 'expand -1')
    _refused(paint(3, 4, 0), 'slice 4 x 0')
    _refused(paint(3, 0, 4), 'slice 0 x 4')
    _refused(paint(3, H=1 << 16, W=1 << 15), '2^31')
    _refused(lib.fcd_component_boxes(P, 1 << 16, 1 << 15, 1, P, None), '2^31')
    _refused(lib.fcd_component_boxes(P, 8, 8, 65, P, None), '65 components')
    _refused(lib.fcd_component_boxes(P, 8, 8, -1, P, None), 'bad arguments')


@pytest.mark.parametrize('H,W', [(1, 1), (1, 2), (1, 300), (300, 1), (67, 45), (131, 197), (2048, 2048), (32, 1025), (46340, 46340),
                                 (1, 2 ** 31 - 1)])
def test_workspace_stays_within_eight_bytes_per_pixel(H, W):
    ws = _lib.lib.fcd_label_components_ws_bytes(H, W)
    assert 0 < ws and ws + 4 * H * W <= 8 * H * W           # labels (int32) + workspace
    assert ws % 4 == 0


def test_workspace_of_a_refused_size_is_zero():
    lib = _lib.lib
    assert lib.fcd_label_components_ws_bytes(1 << 16, 1 << 15) == 0
    assert lib.fcd_label_components_ws_bytes(0, 5) == 0 and lib.fcd_label_components_ws_bytes(5, -1) == 0


def test_wrappers_reject_cpu_tensors():
    import torch
    from fcd_gan_pytorch_amd import _ops as ops
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.label_components(torch.zeros(4, 4, dtype=torch.uint8), 0)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.component_boxes(torch.zeros(4, 4, dtype=torch.int32), 1)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        ops.region_paint(torch.zeros(1, 4, dtype=torch.int32), 4, 4, 1)
    with pytest.raises(_lib.FcdError, match='no CPU fallback'):
        tiles.region_map(np.zeros((4, 4), np.uint8), device='cpu')


# ---- label.txt --------------------------------------------------------------------------------------------------------------
def test_slice_labels_and_label_txt(tmp_path):
    """A 5 x 7 map cut into 2 x 3 slices: ny = 3 (the last one a single row), nx = 3 (the last one a single column).
    Foreground at (0,0), (1,2) -> slice (0,0); (3,6) -> slice (1,2); (4,3) -> slice (2,1).  Checked by hand."""
    m = np.zeros((5, 7), np.uint8)
    m[0, 0] = m[1, 2] = m[3, 6] = m[4, 3] = 9
    want = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0]])
    got = tiles.slice_change_labels(m, (2, 3), (5, 7))
    assert got.shape == (3, 3)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(tiles.slice_change_labels(m[None], (2, 3), (5, 7)), want)
    np.testing.assert_array_equal(tiles.slice_change_labels(m, (2, 3), (5, 7), thresh=9), 0 * want)
    lab, K = tiles.label_components_host(m > 0, 2, (2, 3))
    boxes = tiles.component_boxes_host(lab, K)
    assert boxes.tolist() == [[0, 0, 1, 1], [1, 2, 2, 3], [3, 6, 4, 7], [4, 3, 5, 4]]
    np.testing.assert_array_equal(tiles.slice_change_labels(boxes, (2, 3), (5, 7)), want)
    np.testing.assert_array_equal(tiles.slice_change_labels(np.zeros((0, 4), np.int32), (2, 3), (5, 7)), 0 * want)
    path = str(tmp_path / 'label.txt')
    tiles.write_label_txt(path, got, (2, 3))
    assert open(path).read() == ('0_0.tif,0,0,1\n0_2.tif,0,0,0\n0_4.tif,0,0,0\n'          # x outer, y inner; named by first pixel
                                 '3_0.tif,0,0,0\n3_2.tif,0,0,0\n3_4.tif,0,0,1\n'
                                 '6_0.tif,0,0,0\n6_2.tif,0,0,1\n6_4.tif,0,0,0\n')
    tiles.write_label_txt(path, got[:1, :2], (2, 3), ext='.png')
    assert open(path).read() == '0_0.png,0,0,1\n3_0.png,0,0,0\n'
    # the sliced region map, every box grown by 1 inside its own slice (rows 0-1 | 2-3 | 4, columns 0-2 | 3-5 | 6)
    o, F = 0, 255
    assert tiles.region_map_host(m, expand=1, slice=(2, 3))[0].tolist() == [[F, F, F, o, o, o, o],
                                                                           [F, F, F, o, o, o, o],
                                                                           [o, o, o, o, o, o, F],
                                                                           [o, o, o, o, o, o, F],
                                                                           [o, o, o, F, F, o, o]]
