"""Region maps derived from a change map on the device (csrc/regions.hip: fcd_label_components, fcd_component_boxes,
fcd_region_paint; _ops.label_components / component_boxes / region_paint; tiles.region_map, ResidentScene.derive_region,
demos.demo_rsss(region_from_ref=)) against the scipy-written fixture tests/golden/regions.npz and the NumPy oracle
``tiles.region_map_host``.  Everything is integer: labels, K, boxes and maps are compared EXACTLY."""
import os

import numpy as np
import pytest
import torch

from fcd_gan_pytorch_amd import _lib, _ops as ops, datasets, demos, tiles
from test_regions_host import CASES, EXPANDS, case, fixture

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _up(m):
    """A fixture map on the device + its sample type (uint16 travels as int16 bits)."""
    st = {1: ops.SAMPLE_U8, 2: ops.SAMPLE_U16, 4: ops.SAMPLE_F32}[m.dtype.itemsize]
    return torch.from_numpy(m.view(np.int16) if m.dtype == np.uint16 else m).to(DEV), st


@pytest.mark.parametrize('name', CASES)
def test_labels_boxes_and_maps_equal_the_fixture(name):
    z = fixture()
    m, thresh, sl, conns = case(name)
    t, st = _up(m)
    H, W = m.shape
    for c in conns:
        want = z['%s/labels%d' % (name, c)]
        labels, K = ops.label_components(t, thresh, sample_type=st, connectivity=c, slice=sl)
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (H, W)
        assert K == int(want.max(initial=0))
        np.testing.assert_array_equal(labels.cpu().numpy(), want, err_msg='labels, connectivity %d' % c)
        boxes = ops.component_boxes(labels, K)
        assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (K, 4)
        np.testing.assert_array_equal(boxes.cpu().numpy(), z['%s/boxes%d' % (name, c)], err_msg='boxes, connectivity %d' % c)
        if c == 2:
            for e in EXPANDS:
                region = ops.region_paint(boxes, H, W, e, slice=sl)
                assert region.dtype == torch.uint8 and tuple(region.shape) == (H, W)
                np.testing.assert_array_equal(region.cpu().numpy(), z['%s/region%d' % (name, e)], err_msg='expand %d' % e)
    # the public route, host input -> NumPy, device input -> device tensor
    got = tiles.region_map(m[None], expand=10, thresh=thresh, slice=sl, device=DEV)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (1, H, W)
    np.testing.assert_array_equal(got[0], z['%s/region10' % name])
    got = tiles.region_map(t, expand=3, thresh=thresh, slice=sl, sample_type=st)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W)
    np.testing.assert_array_equal(got.cpu().numpy()[0], z['%s/region3' % name])


def test_two_launches_agree_bit_for_bit():
    m, thresh, sl, _ = case('rand05')
    t, st = _up(m)
    runs = []
    for _ in range(2):
        labels, K = ops.label_components(t, thresh, sample_type=st)
        runs.append((labels.cpu().numpy(), K, ops.component_boxes(labels, K).cpu().numpy()))
    assert runs[0][1] == runs[1][1]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()


@pytest.mark.parametrize('name', ['rand01', 'all_bg', 'sliced'])
def test_outputs_are_fully_written(name):
    """labels, count, boxes and region handed over full of garbage: every element comes back written."""
    z = fixture()
    m, thresh, sl, _ = case(name)
    t, st = _up(m)
    H, W = m.shape
    sh, sw = sl or (0, 0)
    labels = torch.full((H, W), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    nbytes = _lib.lib.fcd_label_components_ws_bytes(H, W)
    ws = torch.full((max(nbytes, 16),), 0xa5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.fcd_label_components(ops._p(t), st, H, W, thresh, 2, sh, sw, ops._p(labels), ops._p(count), ops._p(ws), nbytes,
                                             ops._stream()))
    want = z[name + '/labels2']
    K = int(count.item())
    assert K == int(want.max(initial=0))
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    boxes = torch.full((max(K, 1), 4), -123456, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.fcd_component_boxes(ops._p(labels), H, W, K, ops._p(boxes), ops._stream()))
    np.testing.assert_array_equal(boxes.cpu().numpy()[:K], z[name + '/boxes2'])
    region = torch.full((H, W), 0x5a, dtype=torch.uint8, device=DEV)
    assert ops.region_paint(boxes[:K], H, W, 10, slice=sl, out=region) is region
    np.testing.assert_array_equal(region.cpu().numpy(), z[name + '/region10'])


def test_wrappers_validate_before_launch():
    t = torch.zeros((8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.FcdError, match='connectivity'):
        ops.label_components(t, 0, connectivity=3)
    with pytest.raises(_lib.FcdError, match='slice'):
        ops.label_components(t, 0, slice=(4, 0))
    with pytest.raises(_lib.FcdError, match=r'\(H,W\)'):
        ops.label_components(torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV), 0)
    with pytest.raises(_lib.FcdError, match='uint8, uint16 or float32'):
        ops.label_components(t.double(), 0)
    labels = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.FcdError, match='components'):
        ops.component_boxes(labels, 65)
    with pytest.raises(_lib.FcdError, match='int32'):
        ops.component_boxes(labels.long(), 1)
    boxes = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.FcdError, match='expand'):
        ops.region_paint(boxes, 8, 8, -1)
    with pytest.raises(_lib.FcdError, match='out must be'):
        ops.region_paint(boxes, 8, 8, 1, out=torch.zeros((8, 7), dtype=torch.uint8, device=DEV))


# ---- the resident scene ------------------------------------------------------------------------------------------------------
def _scene_arrays(seed, H, W):
    """A seeded uint16 scene pair and an OSCD-style change map (1 = unchanged, 2 = changed) with a few blobs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 4000, (4, H, W)).astype(np.uint16)
    y = rng.integers(1, 4000, (4, H, W)).astype(np.uint16)
    ref = np.ones((1, H, W), np.uint8)
    for _ in range(5):
        r, c = int(rng.integers(0, H - 6)), int(rng.integers(0, W - 6))
        ref[0, r:r + int(rng.integers(1, 12)), c:c + int(rng.integers(1, 12))] = 2
    return x, y, ref


def test_resident_scene_derives_its_region():
    x, y, ref = _scene_arrays(3, 131, 197)
    want = tiles.region_map_host(ref, expand=10, thresh=1)
    assert 0 < (want == 255).mean() < 1
    scene = tiles.ResidentScene(x, y, ref, (64, 64), (8, 8), device=DEV, region='derive', region_thresh=1)
    assert scene.region.dtype == torch.uint8 and tuple(scene.region.shape) == (1, 131, 197) and scene.region_type == ops.SAMPLE_U8
    np.testing.assert_array_equal(scene.region.cpu().numpy(), want)
    # tensors that already live on the device, the reference map in its own uint8 samples; another recipe
    dev = tiles.ResidentScene.from_device(scene.x, scene.y, ref=torch.from_numpy(ref).to(DEV), patch_size=(64, 64),
                                          overlap_padding=(8, 8), sample_type=ops.SAMPLE_U16)
    assert dev.region is None
    got = dev.derive_region(1, expand=3, slice=(50, 64))
    assert got is dev.region
    np.testing.assert_array_equal(got.cpu().numpy(), tiles.region_map_host(ref, expand=3, thresh=1, slice=(50, 64)))
    auto = tiles.ResidentScene.from_device(scene.x, scene.y, ref=scene.ref, region='derive', region_thresh=1, region_expand=0,
                                           patch_size=(64, 64), overlap_padding=(8, 8), sample_type=ops.SAMPLE_U16)
    np.testing.assert_array_equal(auto.region.cpu().numpy(), tiles.region_map_host(ref, expand=0, thresh=1))
    with pytest.raises(ValueError, match='reference map'):
        tiles.ResidentScene(x, y, None, (64, 64), (8, 8), device=DEV, region='derive')


def test_set_cut_region_tiles_equal_the_host_dataset():
    """Two scenes of different sizes, patch 64, padding 8: the region tiles cut from the DERIVED maps equal the tiles of
    ``RegionTileDataset(region=region_map_host(...))`` bit for bit -- also after a scene of a standing set derives and the set
    is refreshed."""
    patch, pad = (64, 64), (8, 8)
    arrays = [_scene_arrays(21, 131, 197), _scene_arrays(22, 90, 70)]
    host = datasets.MultiSceneDataset([datasets.RegionTileDataset(x, y, region=tiles.region_map_host(ref, 10, 1), ref=ref,
                                                                  patch_size=patch, overlap_padding=pad) for x, y, ref in arrays])
    want = np.stack([host[i][4].numpy() for i in range(len(host))])
    assert set(np.unique(want)) == {0.0, 1.0}
    res = tiles.ResidentSceneSet([tiles.ResidentScene(x, y, ref, patch, pad, device=DEV, region='derive', region_thresh=1)
                                  for x, y, ref in arrays])
    assert len(res) == len(host) and res.has_region
    np.testing.assert_array_equal(res.cut(list(range(len(res))))[3].cpu().numpy(), want)
    late = tiles.ResidentSceneSet([tiles.ResidentScene(x, y, ref, patch, pad, device=DEV) for x, y, ref in arrays])
    assert not late.has_region
    for s in late.scenes:
        s.derive_region(1, expand=10)
    late.refresh()
    assert late.has_region
    np.testing.assert_array_equal(late.cut(list(range(len(late))))[3].cpu().numpy(), want)


TILE = 176          # MS-SSIM refuses tiles of 160 pixels or fewer (tests/test_gpu_scene_train.py)


def test_demo_rsss_derives_the_regions_it_needs():
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'datasets.npz'))

    def arrays(nm):                                          # the two fixture scenes, repeated 4 x 4: 280x360 and 220x192
        xname = str(z['%s/xname' % nm])
        yname = nm + ('_2' if xname.endswith('_1') else '_1')
        return tuple(np.ascontiguousarray(np.tile(z[k], (1, 4, 4))) for k in ('%s/%s' % (nm, xname), '%s/%s' % (nm, yname),
                                                                             '%s/%s-cm.tif' % (nm, nm)))
    make = lambda: tiles.ResidentSceneSet([tiles.ResidentScene(*arrays(nm), (TILE, TILE), (4, 4), device=DEV)
                                           for nm in ('abudhabi', 'paris')])
    res = make()
    assert res.numlist == [6, 4] and not res.has_region
    with pytest.raises(ValueError, match='region'):
        demos.demo_rsss(res, epochs_g=0, epochs_adv=1, init_batch_size=3, batch_size=3, allow_seeded=True)
    out = demos.demo_rsss(res, epochs_g=0, epochs_adv=1, init_batch_size=3, batch_size=3, allow_seeded=True, region_from_ref=(1, 10))
    hist = out['history']
    assert len(hist['g']) == 0 and len(hist['adv']) == 1 and len(hist['adv'][0]) == 4 and np.isfinite(hist['adv']).all()
    assert res.has_region
    for s, nm in zip(res.scenes, ('abudhabi', 'paris')):
        np.testing.assert_array_equal(s.region.cpu().numpy(), tiles.region_map_host(arrays(nm)[2], expand=10, thresh=1))
