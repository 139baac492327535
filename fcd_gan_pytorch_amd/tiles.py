"""Tile geometry, minimal TIFF I/O and host->device feeding for the hot path
(SURVEY.md section 8f rows 1 and 4).

The reference tiles a big GeoTIFF pair into overlapped patches through GDAL
(``GDALDataset``, data_utils.py:28-236): stride = patch - 2*pad, every patch is read
with ``pad`` pixels of context (clipped at the scene border), zero-embedded into a
fixed ``patch_size`` canvas, and only its centre is written back.  GDAL is not
available here, so this module restates the *arithmetic* (``TileGrid``), reads /
writes baseline TIFF itself (uncompressed strips; uint8 / uint16 / float32; chunky or
planar samples -- what config[0]'s synthetic 4-band T1/T2 pair needs) and feeds the GPU
from a background thread through pinned staging buffers (``Prefetcher``).

Per-band normalisation ``(x - mean) / std`` (``NORMALIZE``, CommonFunc.py:199-224) is
applied on the host copy exactly like the reference (``enhance``), or on device via
``normalize_``.
"""
import math
import struct
import threading
import queue

import os

import numpy as np
import torch


# ----------------------------------------------------------------------- geometry
class TileGrid:
    """Overlapped tiling of an (xsize, ysize) scene -- data_utils.py:57-70,142-176.
    ``patch_size`` and ``overlap_padding`` are (x, y) pairs like the reference's."""

    def __init__(self, xsize, ysize, patch_size=(200, 200), overlap_padding=(10, 10)):
        self.xsize, self.ysize = int(xsize), int(ysize)
        self.patch_size = (int(patch_size[0]), int(patch_size[1]))
        self.pad = (int(overlap_padding[0]), int(overlap_padding[1]))
        sx = self.patch_size[0] - 2 * self.pad[0]
        sy = self.patch_size[1] - 2 * self.pad[1]
        if sx <= 0 or sy <= 0:
            raise ValueError('patch_size must exceed twice the overlap padding')
        self.xstart = list(range(0, self.xsize, sx))
        self.xend = [x + sx for x in self.xstart if x + sx < self.xsize] + [self.xsize]
        self.ystart = list(range(0, self.ysize, sy))
        self.yend = [y + sy for y in self.ystart if y + sy < self.ysize] + [self.ysize]

    def patch_count(self):
        return len(self.xstart), len(self.ystart)

    def __len__(self):
        return len(self.xstart) * len(self.ystart)

    def item_xy(self, item):
        ny = len(self.ystart)
        return int(math.floor(item / ny)), int(item % ny)

    def slices(self, item):
        """(slice, slice_read, slice_write), each (x0, y0, w, h):
        slice = the centre region this tile owns in the scene; slice_read = what is read
        (centre + clipped context); slice_write = where the read block sits in the canvas."""
        ix, iy = self.item_xy(item)
        px, py = self.pad
        x0, x1, y0, y1 = self.xstart[ix], self.xend[ix], self.ystart[iy], self.yend[iy]
        own = (x0, y0, x1 - x0, y1 - y0)
        ox = 0 if x0 - px > 0 else px
        oy = 0 if y0 - py > 0 else py
        rx0 = x0 - px if x0 - px > 0 else 0
        ry0 = y0 - py if y0 - py > 0 else 0
        rx1 = x1 + px if x1 + px < self.xsize else self.xsize
        ry1 = y1 + py if y1 + py < self.ysize else self.ysize
        return own, (rx0, ry0, rx1 - rx0, ry1 - ry0), (ox, oy, rx1 - rx0, ry1 - ry0)

    def read_patch(self, scene, item, dtype=np.float64):
        """scene: (bands, ysize, xsize) array -> (bands, patch_y, patch_x) zero-embedded patch
        (data_utils.py:98-118)."""
        _, (rx, ry, rw, rh), (wx, wy, ww, wh) = self.slices(item)
        canvas = np.zeros((scene.shape[0], self.patch_size[1], self.patch_size[0]), dtype=dtype)
        canvas[:, wy:wy + wh, wx:wx + ww] = scene[:, ry:ry + rh, rx:rx + rw]
        return canvas

    def write_center(self, out_scene, patch, item):
        """Write only the owned centre of a (bands, patch_y, patch_x) result back into
        out_scene (bands, ysize, xsize) -- data_utils.py:205-213,230-236."""
        (x0, y0, w, h), _, _ = self.slices(item)
        px, py = self.pad
        out_scene[:, y0:y0 + h, x0:x0 + w] = patch[:, py:py + h, px:px + w]

    def eff_range(self, item):
        """Rows/cols of a patch that are scored by the metrics (OSCD_Dataset_RSS.EffRange,
        data_utils.py:390-400 semantics: the owned centre inside the canvas)."""
        (x0, y0, w, h), _, _ = self.slices(item)
        px, py = self.pad
        return py, py + h, px, px + w


# --------------------------------------------------------------------- TIFF codec
_TIFF_TYPES = {1: ('B', 1), 2: ('c', 1), 3: ('H', 2), 4: ('I', 4), 5: ('II', 8), 16: ('Q', 8)}
_NP_OF = {(1, 8): np.uint8, (1, 16): np.uint16, (1, 32): np.uint32, (2, 16): np.int16, (2, 32): np.int32,
          (3, 32): np.float32, (3, 64): np.float64}


def read_tiff(path):
    """Baseline TIFF reader: uncompressed, strip-organised, chunky or planar samples.
    Returns a (bands, height, width) array in the file's sample dtype."""
    with open(path, 'rb') as f:
        data = f.read()
    bo = {b'II': '<', b'MM': '>'}.get(data[:2])
    if bo is None or struct.unpack(bo + 'H', data[2:4])[0] != 42:
        raise ValueError('%s: not a classic TIFF file' % path)
    off = struct.unpack(bo + 'I', data[4:8])[0]
    n = struct.unpack(bo + 'H', data[off:off + 2])[0]
    tags = {}
    for i in range(n):
        e = off + 2 + 12 * i
        tag, typ, cnt = struct.unpack(bo + 'HHI', data[e:e + 8])
        if typ not in _TIFF_TYPES:
            continue
        code, size = _TIFF_TYPES[typ]
        total = size * cnt
        voff = e + 8 if total <= 4 else struct.unpack(bo + 'I', data[e + 8:e + 12])[0]
        if typ == 5:
            vals = struct.unpack(bo + 'I' * (2 * cnt), data[voff:voff + total])
        elif typ == 2:
            vals = (data[voff:voff + cnt],)
        else:
            vals = struct.unpack(bo + code * cnt, data[voff:voff + total])
        tags[tag] = vals
    W, H = tags[256][0], tags[257][0]
    spp = tags.get(277, (1,))[0]
    bits = tags.get(258, (1,) * spp)
    if tags.get(259, (1,))[0] != 1:
        raise ValueError('%s: compressed TIFF is not supported' % path)
    if 324 in tags:
        raise ValueError('%s: tiled TIFF is not supported' % path)
    fmt = tags.get(339, (1,) * spp)[0]
    planar = tags.get(284, (1,))[0]
    dt = _NP_OF.get((fmt, bits[0]))
    if dt is None or any(b != bits[0] for b in bits):
        raise ValueError('%s: unsupported sample format %r / bits %r' % (path, fmt, bits))
    dt = np.dtype(dt).newbyteorder(bo)
    offs, cnts = tags[273], tags[279]
    raw = b''.join(data[o:o + c] for o, c in zip(offs, cnts))
    arr = np.frombuffer(raw, dtype=dt)
    if planar == 2:
        out = arr[:spp * H * W].reshape(spp, H, W)
    else:
        out = arr[:H * W * spp].reshape(H, W, spp).transpose(2, 0, 1)
    return np.ascontiguousarray(out).astype(dt.newbyteorder('='))


def write_tiff(path, array, planar=True, rows_per_strip=None):
    """Write a (bands, H, W) (or (H, W)) uint8 / uint16 / float32 array as baseline TIFF
    (little-endian, uncompressed strips)."""
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[None]
    fmt_bits = {np.dtype(np.uint8): (1, 8), np.dtype(np.uint16): (1, 16), np.dtype(np.float32): (3, 32)}.get(a.dtype)
    if fmt_bits is None:
        raise ValueError('write_tiff supports uint8, uint16 and float32, got %s' % a.dtype)
    fmt, bits = fmt_bits
    spp, H, W = a.shape
    rps = H if rows_per_strip is None else int(rows_per_strip)
    nstrips_plane = (H + rps - 1) // rps
    if planar and spp > 1:
        payload = [np.ascontiguousarray(a[b, r:r + rps]).astype('<' + a.dtype.str[1:]).tobytes()
                   for b in range(spp) for r in range(0, H, rps)]
        planar_cfg = 2
    else:
        chunky = np.ascontiguousarray(a.transpose(1, 2, 0))
        payload = [chunky[r:r + rps].astype('<' + a.dtype.str[1:]).tobytes() for r in range(0, H, rps)]
        planar_cfg = 1
    nstr = len(payload)
    assert nstr == nstrips_plane * (spp if planar_cfg == 2 else 1)
    entries = []     # (tag, type, count, values)

    def ent(tag, typ, vals):
        entries.append((tag, typ, len(vals), list(vals)))
    ent(256, 4, [W]); ent(257, 4, [H]); ent(258, 3, [bits] * spp); ent(259, 3, [1])
    rgb = spp == 3 and a.dtype == np.uint8           # like GDAL: 3 x uint8 is written as RGB
    ent(262, 3, [2 if rgb else 1]); ent(273, 4, [0] * nstr); ent(277, 3, [spp]); ent(278, 4, [rps])
    ent(279, 4, [len(p) for p in payload]); ent(284, 3, [planar_cfg]); ent(339, 3, [fmt] * spp)
    if spp > 1 and not rgb:
        ent(338, 3, [0] * (spp - 1))          # ExtraSamples: unspecified
    entries.sort(key=lambda e: e[0])
    ifd_off = 8
    ifd_size = 2 + 12 * len(entries) + 4
    extra_off = ifd_off + ifd_size
    extra = b''
    recs = []
    strip_slot = None
    for tag, typ, cnt, vals in entries:
        code = {3: 'H', 4: 'I'}[typ]
        blob = struct.pack('<' + code * cnt, *vals)
        if len(blob) <= 4:
            recs.append([tag, typ, cnt, blob.ljust(4, b'\0'), None])
        else:
            recs.append([tag, typ, cnt, struct.pack('<I', extra_off + len(extra)), len(extra)])
            if tag == 273:
                strip_slot = (len(extra), cnt)
            extra += blob + (b'\0' if len(blob) % 2 else b'')
        if tag == 273 and len(blob) <= 4:
            strip_slot = ('inline', len(recs) - 1)
    data_off = extra_off + len(extra)
    offs, o = [], data_off
    for p in payload:
        offs.append(o)
        o += len(p)
    blob = struct.pack('<' + 'I' * nstr, *offs)
    if strip_slot[0] == 'inline':
        recs[strip_slot[1]][3] = blob.ljust(4, b'\0')
    else:
        extra = extra[:strip_slot[0]] + blob + extra[strip_slot[0] + len(blob):]
    with open(path, 'wb') as f:
        f.write(b'II' + struct.pack('<HI', 42, ifd_off))
        f.write(struct.pack('<H', len(recs)))
        for tag, typ, cnt, val, _ in recs:
            f.write(struct.pack('<HHI', tag, typ, cnt) + val)
        f.write(struct.pack('<I', 0))
        f.write(extra)
        for p in payload:
            f.write(p)


# ------------------------------------------------------- region maps from a change map
# The reference prepares its regional supervision offline (OSCDProcess.py:56-73, BuildingProcess.py:127-145,167): threshold the
# change map, ``skimage.measure.label(connectivity=2)``, ``regionprops`` boxes, every box grown by ``region_expand = 10`` pixels,
# clamped and filled with 255 -- per 200x200 slice for the sliced WHU set, with one changed / unchanged flag per slice in
# label.txt.  ``region_map`` does it on the device (csrc/regions.hip), ``region_map_host`` restates it in NumPy.
# ``slice`` = (slice_h, slice_w) everywhere.  Recipes: OSCD ``thresh=1``, WHU ``thresh=0, slice=(200, 200)``.
def _plane(ref):
    """A change map given as (H,W) or (1,H,W) -> the (H,W) plane."""
    a = np.asarray(ref)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2 or a.size == 0:
        raise ValueError('the change map must be (H,W) or (1,H,W), got shape %s' % (np.asarray(ref).shape,))
    return a


def _slice_pair(slice):
    if slice is None:
        return None
    sh, sw = (int(v) for v in slice)
    if sh <= 0 or sw <= 0:
        raise ValueError('slice = (slice_h, slice_w), both positive, or None; got %r' % (slice,))
    return sh, sw


def label_components_host(fg, connectivity=2, slice=None):
    """``(labels int32 (H,W), K)`` of a boolean plane, numbered in raster order of each component's first pixel
    (``scipy.ndimage.label``'s numbering), with connectivity cut at the borders of ``slice``.  Row runs by NumPy, a union-find over
    the runs in plain Python: the oracle of ``_ops.label_components``, no scipy or skimage."""
    fg = np.asarray(fg, dtype=bool)
    H, W = fg.shape
    if connectivity not in (1, 2):
        raise ValueError('connectivity %r (1: 4 neighbours, 2: 8 neighbours)' % (connectivity,))
    sl = _slice_pair(slice)
    link = np.zeros((H, W), dtype=bool)                  # pixel continues the run of its left neighbour
    link[:, 1:] = fg[:, 1:] & fg[:, :-1]
    if sl:
        link[:, ::sl[1]] = False
    starts = fg & ~link
    ends = fg.copy()
    ends[:, :-1] &= ~link[:, 1:]
    ry, rx0 = np.nonzero(starts)
    rx1 = np.nonzero(ends)[1] + 1                        # same raster order: the k-th end closes the k-th start
    n = len(ry)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    first = np.searchsorted(ry, np.arange(H + 1))        # runs of row y: first[y] .. first[y + 1]
    reach = 1 if connectivity == 2 else 0                # a diagonal touch: the upper run ends where this one starts
    x0, x1 = rx0.tolist(), rx1.tolist()
    col = (rx0 // sl[1]).tolist() if sl else None
    for y in range(1, H):
        if sl and y % sl[0] == 0:
            continue
        a, a_end, b, b_end = int(first[y]), int(first[y + 1]), int(first[y - 1]), int(first[y])
        while a < a_end and b < b_end:
            if x0[a] < x1[b] + reach and x0[b] < x1[a] + reach and (col is None or col[a] == col[b]):
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if x1[b] <= x1[a]:                           # the run that ends first cannot touch anything further right
                b += 1
            else:
                a += 1
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    is_root = root == np.arange(n)
    rank = np.cumsum(is_root)                            # runs are in raster order, a root is its component's first run
    lab = rank[root] if n else root
    flat = np.zeros(H * W + 1, dtype=np.int64)
    np.add.at(flat, ry * W + rx0, lab)
    np.add.at(flat, ry * W + rx1, -lab)
    return np.cumsum(flat[:-1]).reshape(H, W).astype(np.int32), int(is_root.sum())


def component_boxes_host(labels, K):
    """int32 (K,4) ``min_y, min_x, max_y, max_x`` (half-open, ``regionprops.bbox``) of labels 1..K."""
    labels = np.asarray(labels)
    boxes = np.empty((K, 4), dtype=np.int64)
    boxes[:, :2] = max(labels.shape)
    boxes[:, 2:] = 0
    y, x = np.nonzero(labels)
    k = labels[y, x].astype(np.int64) - 1
    np.minimum.at(boxes[:, 0], k, y)
    np.minimum.at(boxes[:, 1], k, x)
    np.maximum.at(boxes[:, 2], k, y + 1)
    np.maximum.at(boxes[:, 3], k, x + 1)
    return boxes.astype(np.int32)


def region_paint_host(boxes, H, W, expand, slice=None):
    """uint8 (H,W): 255 inside every box grown by ``expand`` and clamped with the reference's rule (OSCDProcess.py:68-73), against
    the scene or, with ``slice``, against the box's own slice cut to the scene (BuildingProcess.py:140-145)."""
    sl = _slice_pair(slice)
    e = int(expand)
    if e < 0:
        raise ValueError('expand %d is negative' % e)
    region = np.zeros((H, W), dtype=np.uint8)
    for min_y, min_x, max_y, max_x in np.asarray(boxes, dtype=np.int64).reshape(-1, 4).tolist():
        y0, x0, y1, x1 = 0, 0, H, W
        if sl:
            y0, x0 = min_y // sl[0] * sl[0], min_x // sl[1] * sl[1]
            y1, x1 = min(y0 + sl[0], H), min(x0 + sl[1], W)
        min_y = min_y - e if (min_y - e) > y0 else y0
        min_x = min_x - e if (min_x - e) > x0 else x0
        max_y = max_y + e if (max_y + e) < y1 else y1
        max_x = max_x + e if (max_x + e) < x1 else x1
        region[min_y:max_y, min_x:max_x] = 255
    return region


def region_map_host(ref, expand=10, thresh=0, slice=None, connectivity=2):
    """The region supervision map of a change map in plain NumPy / Python: uint8 (1,H,W), 255 inside the grown bounding box of
    every connected component of ``double(ref) > thresh`` (NaN: background), 0 elsewhere.  Never touches the device: the oracle
    of :func:`region_map`."""
    a = _plane(read_tiff(ref) if isinstance(ref, str) else ref)
    with np.errstate(invalid='ignore'):
        fg = a.astype(np.float64) > float(thresh)
    labels, K = label_components_host(fg, connectivity, slice)
    return region_paint_host(component_boxes_host(labels, K), a.shape[0], a.shape[1], expand, slice)[None]


def _region_on_device(plane, sample_type, thresh, expand, slice, connectivity=2):
    """(H,W) device plane -> uint8 (1,H,W) region map on the device: label, boxes, paint (``_ops``)."""
    from . import _ops as ops
    labels, K = ops.label_components(plane, thresh, sample_type=sample_type, connectivity=connectivity, slice=slice)
    boxes = ops.component_boxes(labels, K)
    return ops.region_paint(boxes, labels.shape[0], labels.shape[1], expand, slice=slice)[None]


def region_map(ref, expand=10, thresh=0, slice=None, device='cuda', sample_type=None):
    """:func:`region_map_host` on the device (``_ops.label_components`` / ``component_boxes`` / ``region_paint``): ``ref`` is a
    (1,H,W) or (H,W) array, the path of a TIFF, or a device tensor (``sample_type=_ops.SAMPLE_U16`` for uint16 bits held in an
    int16 tensor); uint8, uint16 or float32 samples.  Returns the uint8 (1,H,W) 0 / 255 map as a NumPy array for host input and
    as a device tensor for device input."""
    from . import _ops as ops
    if torch.is_tensor(ref) and ref.is_cuda:
        t = ref[0] if ref.dim() == 3 and ref.shape[0] == 1 else ref
        return _region_on_device(t, sample_type, thresh, expand, slice)
    a = _plane(read_tiff(ref) if isinstance(ref, str) else (ref.numpy() if torch.is_tensor(ref) else ref))
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype not in (np.uint8, np.uint16, np.float32):
        raise ops._lib.FcdError('region_map: the change map must hold uint8, uint16 or float32 samples, got %s' % a.dtype)
    device = ops._upload_device(device, 'the change map goes')
    st = {1: ops.SAMPLE_U8, 2: ops.SAMPLE_U16, 4: ops.SAMPLE_F32}[a.dtype.itemsize]
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)
    return _region_on_device(t, st, thresh, expand, slice).cpu().numpy()


def slice_change_labels(boxes_or_ref, slice, shape, thresh=0):
    """The (ny,nx) 0 / 1 array of BuildingProcess.py:129 for a scene of ``shape`` = (H,W) cut into ``slice`` = (slice_h, slice_w):
    a slice is 1 when it holds any foreground.  From the (K,4) component boxes labelled WITH that slice (every box then lies in
    one slice) this is a few lines on the host; a change map of ``shape`` (or (1,H,W)) is thresholded here (``> thresh``)."""
    sh, sw = _slice_pair(slice)
    H, W = (int(v) for v in shape)
    a = boxes_or_ref.cpu().numpy() if torch.is_tensor(boxes_or_ref) else np.asarray(boxes_or_ref)
    out = np.zeros((-(-H // sh), -(-W // sw)), dtype=np.int64)
    if a.shape in ((H, W), (1, H, W)):
        with np.errstate(invalid='ignore'):
            y, x = np.nonzero(_plane(a).astype(np.float64) > float(thresh))
    elif a.ndim == 2 and a.shape[1] == 4:
        y, x = a[:, 0], a[:, 1]
    else:
        raise ValueError('slice_change_labels: (K,4) boxes or a change map of shape %s, got shape %s' % ((H, W), a.shape))
    out[np.asarray(y) // sh, np.asarray(x) // sw] = 1
    return out


def write_label_txt(path, labels, slice, ext='.tif'):
    """label.txt as BuildingProcess.py:167 writes it: one line ``'{x}_{y}{ext},0,0,{label}'`` per slice, named by the slice's
    first pixel, x outer and y inner (BuildingProcess.py:99-100).  ``labels`` = the (ny,nx) array of :func:`slice_change_labels`."""
    sh, sw = _slice_pair(slice)
    labels = np.asarray(labels)
    with open(path, 'w') as f:
        for i in range(labels.shape[1]):
            for j in range(labels.shape[0]):
                f.write('{}_{}{},0,0,{}\n'.format(i * sw, j * sh, ext, int(labels[j, i])))


# ------------------------------------------------------------------------ dataset
def _load_scenes(scene_x, scene_y, ref=None, region=None, as_arrays=False):
    """The scene pair and its optional (1,H,W) maps, each given as a (bands,H,W) array or as the path of a TIFF: read, and
    checked to agree in size, with the reference's messages (data_utils.py:51,83,259).  ``as_arrays`` (the resident scene, which
    uploads them): the scenes and the region map are made NumPy arrays, and the scenes must have three dimensions."""
    def load(a, convert=as_arrays):
        a = read_tiff(a) if isinstance(a, str) else a
        return np.asarray(a) if convert and a is not None else a
    scene_x, scene_y, ref, region = load(scene_x), load(scene_y), load(ref, False), load(region)
    if scene_x.shape != scene_y.shape or (as_arrays and scene_x.ndim != 3):
        raise ValueError("Image sizes don't match")
    for m in (ref, region):
        if m is not None and (m.shape[0] != 1 or m.shape[1:] != scene_x.shape[1:]):
            raise ValueError("Reference sizes don't match image")
    return scene_x, scene_y, ref, region


class PairTileDataset(torch.utils.data.Dataset):
    """In-memory restatement of GDALDataset (data_utils.py:28-140): a bi-temporal scene pair
    (+ optional reference map) cut into overlapped patches.  ``__getitem__`` returns the
    reference's tuple ``(x, y, item, ref)`` of float32 tensors (data_utils.py:140)."""

    def __init__(self, scene_x, scene_y, ref=None, patch_size=(200, 200), overlap_padding=(10, 10),
                 stats=None, enhance=None, transforms=None):
        if stats is not None and enhance is not None:
            raise ValueError('PairTileDataset: give stats (NORMALIZE) or enhance, not both')
        scene_x, scene_y, ref, _ = _load_scenes(scene_x, scene_y, ref)
        self.x, self.y, self.ref = scene_x, scene_y, ref
        self.grid = TileGrid(scene_x.shape[2], scene_x.shape[1], patch_size, overlap_padding)
        self.stats = stats            # (meanX, stdX, meanY, stdY) per band, NORMALIZE semantics
        # the reference's two hooks (data_utils.py:110-112,126-128): ``enhance(block, switch=1 | 2)`` on the read block in float64
        # (a ``transforms.NORMALIZE`` / ``SCALE`` / ``SCALE_NORM``), ``transforms`` on the two float32 tensors after placement
        # (a ``transforms.RANDOM_ERASER...``: the region drawn for x is reused for y)
        self.enhance, self.transforms = enhance, transforms

    def __len__(self):
        return len(self.grid)

    def _norm(self, a, mean, std):
        a = a.astype(float)
        for b in range(a.shape[0]):
            a[b] = (a[b] - mean[b]) / std[b]
        return a

    def raw_item(self, item):
        """The patch WITHOUT host normalisation: ``(x_raw, y_raw, item, ref, valid)`` with ``valid`` (1,py,px) = 1 on
        the window that holds scene pixels.  Normalise on the device (``_ops.normalize_tiles``: one fused pass, fp64 per
        element, bit-identical to ``__getitem__``) or not at all (``Segmentor.forward_raw`` folds the statistics into
        its first convolution).  Not with ``transforms``: erasing raw samples before the device normalises them would not
        give the zeros the reference trains on."""
        if self.transforms is not None:
            raise ValueError('raw_item: a dataset with transforms has no raw route (erase after normalisation)')
        _, (rx, ry, rw, rh), (wx, wy, ww, wh) = self.grid.slices(item)
        px, py = self.grid.patch_size
        cx = np.zeros((self.x.shape[0], py, px), dtype=np.float32)
        cy = np.zeros_like(cx)
        cx[:, wy:wy + wh, wx:wx + ww] = self.x[:, ry:ry + rh, rx:rx + rw]
        cy[:, wy:wy + wh, wx:wx + ww] = self.y[:, ry:ry + rh, rx:rx + rw]
        r = np.zeros((1, py, px), dtype=np.float32)
        if self.ref is not None:
            r[:, wy:wy + wh, wx:wx + ww] = self.ref[:, ry:ry + rh, rx:rx + rw]
        valid = np.zeros((1, py, px), dtype=np.float32)
        valid[:, wy:wy + wh, wx:wx + ww] = 1.0
        return (torch.from_numpy(cx), torch.from_numpy(cy), torch.tensor(item), torch.from_numpy(r),
                torch.from_numpy(valid))

    def __getitem__(self, item):
        _, (rx, ry, rw, rh), (wx, wy, ww, wh) = self.grid.slices(item)
        bx = np.array(self.x[:, ry:ry + rh, rx:rx + rw], dtype=float)
        by = np.array(self.y[:, ry:ry + rh, rx:rx + rw], dtype=float)
        if self.stats is not None:                      # 'enhance' runs on the read block (data_utils.py:106-108)
            bx = self._norm(bx, self.stats[0], self.stats[1])
            by = self._norm(by, self.stats[2], self.stats[3])
        if self.enhance is not None:
            bx = self.enhance(bx, switch=1)
            by = self.enhance(by, switch=2)
        px, py = self.grid.patch_size
        cx = np.zeros((bx.shape[0], py, px), dtype=float)
        cy = np.zeros_like(cx)
        cx[:, wy:wy + wh, wx:wx + ww] = bx
        cy[:, wy:wy + wh, wx:wx + ww] = by
        r = np.zeros((1, py, px), dtype=float)
        if self.ref is not None:
            r[:, wy:wy + wh, wx:wx + ww] = self.ref[:, ry:ry + rh, rx:rx + rw]
        tx, ty = torch.from_numpy(cx).float(), torch.from_numpy(cy).float()
        if self.transforms is not None:
            tx, sync = self.transforms(tx)
            ty, _ = self.transforms(ty, sync)
        return tx, ty, torch.tensor(item), torch.from_numpy(r).float()


class RawTiles(torch.utils.data.Dataset):
    """View of a PairTileDataset that yields ``raw_item`` tuples (normalisation left to the device)."""

    def __init__(self, ds):
        self.ds, self.grid, self.ref, self.stats = ds, ds.grid, ds.ref, ds.stats

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, item):
        return self.ds.raw_item(item)


class ResidentScene:
    """A bi-temporal scene pair (+ optional reference map) that lives in device memory for a whole inference pass: uploaded
    ONCE in its own sample type (uint8 / uint16 / float32 -- a uint16 scene is half the bytes of its fp32 tiles), cut into
    the tiles of ``PairTileDataset`` on the device (``_ops.scene_cut``: same values bit for bit, no host loop, no pinned
    staging).  The reference map goes up as float32, the form the stitch kernel compares in; the optional weak ``region`` mask
    (GDALDataset_RSS, data_utils.py:239-290) stays in its own sample type.  One scene; several of them make a
    ``ResidentSceneSet``, the training feed.  ``stats='auto'``: the scene's own statistics (:meth:`statistics`), taken on the
    device before anything is cut.  ``region='derive'``: the region map is made from the reference map on the device
    (:meth:`derive_region` with ``region_thresh``, ``region_expand``, ``region_slice``)."""

    def __init__(self, scene_x, scene_y, ref=None, patch_size=(200, 200), overlap_padding=(10, 10), stats=None, device='cuda',
                 region=None, enhance=None, region_thresh=0, region_expand=10, region_slice=None):
        from . import _ops as ops
        if stats is not None and enhance is not None:
            raise ValueError('ResidentScene: give stats (NORMALIZE) or enhance, not both')
        derive = isinstance(region, str) and region == 'derive'
        if derive and ref is None:
            raise ValueError("ResidentScene: region='derive' needs the reference map")
        scene_x, scene_y, ref, region = _load_scenes(scene_x, scene_y, ref, None if derive else region, as_arrays=True)
        if scene_x.dtype != scene_y.dtype or scene_x.dtype not in (np.uint8, np.uint16, np.float32):
            raise ops._lib.FcdError('ResidentScene: both scenes must be uint8, uint16 or float32 arrays of one type, got %s / %s'
                                    % (scene_x.dtype, scene_y.dtype))
        if region is not None and region.dtype not in (np.uint8, np.uint16, np.float32):
            raise ops._lib.FcdError('ResidentScene: the region map must be uint8, uint16 or float32, got %s' % region.dtype)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops._lib.FcdError('ResidentScene lives on a CUDA/ROCm device, not %s (no CPU fallback)' % self.device)
        sample_type = {1: ops.SAMPLE_U8, 2: ops.SAMPLE_U16, 4: ops.SAMPLE_F32}

        def up(a):          # uint16 samples travel as int16 bits (same bytes; the kernel reads them as uint16)
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(self.device)
        self._attach(up(scene_x), up(scene_y), sample_type[scene_x.dtype.itemsize],
                     None if ref is None else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(self.device),
                     ops.SAMPLE_F32, None if region is None else up(region),
                     0 if region is None else sample_type[region.dtype.itemsize], patch_size, overlap_padding, stats)
        if enhance is not None:
            self.set_enhance(enhance)
        if derive:
            self.derive_region(region_thresh, region_expand, region_slice)

    @classmethod
    def from_device(cls, x, y, ref=None, region=None, patch_size=(200, 200), overlap_padding=(10, 10), stats=None,
                    sample_type=None, ref_type=None, region_type=None, region_thresh=0, region_expand=10, region_slice=None):
        """A ResidentScene over tensors that already live on the device, copied nowhere: ``x``, ``y`` (C,H,W) of uint8, uint16 or
        float32 samples (``sample_type=_ops.SAMPLE_U16`` for uint16 bits held in an int16 tensor), ``ref`` / ``region`` (1,H,W)
        likewise (``ref_type`` / ``region_type``).  The stitch kernel of ``infer_scene_resident`` wants a float32 ``ref``.
        ``region='derive'``: as in the constructor."""
        from . import _ops as ops
        derive = isinstance(region, str) and region == 'derive'
        if derive:
            if ref is None:
                raise ValueError("ResidentScene: region='derive' needs the reference map")
            region = None
        x, y, st, _, _, _ = ops._scene_pair('ResidentScene', x, y, sample_type, one_device=True)
        maps = []
        for t, typ, name in ((ref, ref_type, 'reference map'), (region, region_type, 'region map')):
            if t is None:
                maps += [None, 0]
                continue
            t, typ = ops._scene_tensor(t, name, typ)
            if t.numel() != x.shape[1] * x.shape[2] or t.device != x.device:
                raise ValueError("Reference sizes don't match image")
            maps += [t, typ]
        self = cls.__new__(cls)
        self.device = x.device
        self._attach(x, y, st, maps[0], maps[1], maps[2], maps[3], patch_size, overlap_padding, stats)
        if derive:
            self.derive_region(region_thresh, region_expand, region_slice)
        return self

    def _attach(self, x, y, sample_type, ref, ref_type, region, region_type, patch_size, overlap_padding, stats):
        self.x, self.y, self.sample_type = x, y, sample_type
        self.ref, self.ref_type, self.region, self.region_type = ref, ref_type, region, region_type
        self.bands = int(x.shape[0])
        self.grid = TileGrid(int(x.shape[2]), int(x.shape[1]), patch_size, overlap_padding)
        self.stats, self._stats_dev, self.stats_count = None, None, None
        self._clear_enhance()
        if isinstance(stats, str):
            if stats != 'auto':
                raise ValueError("stats: (meanX, stdX, meanY, stdY), None or 'auto'")
            stats = self.statistics()
        self.set_stats(stats)

    def _clear_enhance(self):
        """No enhancer, and no private one-scene set made for one (``cut``)."""
        self.enhance, self.enhance_kind, self.enhance_scale, self._solo = None, 0, None, None

    def set_stats(self, stats):
        """``stats`` = (meanX, stdX, meanY, stdY) per band, NORMALIZE semantics (as PairTileDataset), or None."""
        from . import _ops as ops
        self.stats, self._stats_dev = stats, None
        self._clear_enhance()
        if stats is not None:
            s = np.stack([np.asarray(v, dtype=np.float64).reshape(-1) for v in stats])
            if s.shape != (4, self.bands):
                raise ops._lib.FcdError("ResidentScene: The input channel doesn't match the stats list")   # CommonFunc.py:212
            self._stats_dev = torch.from_numpy(np.ascontiguousarray(s)).to(self.device)
            self.enhance_kind = 1

    def set_enhance(self, enh):
        """``enh`` = a ``transforms.NORMALIZE`` / ``SCALE`` / ``SCALE_NORM`` (the object ``PairTileDataset(enhance=)`` takes), or
        None.  ``NORMALIZE`` is ``set_stats`` with its four lists; the other two put their per-band ranges where the statistics
        go and switch the cut to their formula (``_ops.scene_set_cut(mode=)``)."""
        if enh is None or enh.kind == 1:
            self.set_stats(None if enh is None else tuple(np.asarray(v, np.float64) for v in enh.params(self.bands)))
            self.enhance = enh
            return
        self.set_stats(None)
        self._stats_dev = torch.from_numpy(np.ascontiguousarray(enh.params(self.bands))).to(self.device)
        self.enhance, self.enhance_kind = enh, int(enh.kind)
        self.enhance_scale = (float(enh.scale[0]), float(enh.scale[1])) if enh.kind == 3 else None

    def derive_region(self, thresh, expand=10, slice=None):
        """Make the region map from the reference map where it lies (:func:`region_map`: components of ``ref > thresh``, their
        boxes grown by ``expand``; ``slice`` = (slice_h, slice_w) for the sliced recipe) and install it as ``self.region``, uint8
        (1,H,W) of 0 / 255.  OSCD: ``thresh=1``; WHU: ``thresh=0, slice=(200, 200)``.  A scene that already belongs to a
        ``ResidentSceneSet`` needs the set's ``refresh()`` afterwards: the set keeps the address of the map it was made with."""
        from . import _ops as ops
        if self.ref is None:
            raise ValueError('ResidentScene.derive_region needs the reference map')
        plane = self.ref.reshape(self.grid.ysize, self.grid.xsize)
        self.region = _region_on_device(plane, self.ref_type, thresh, expand, slice)
        self.region_type = ops.SAMPLE_U8
        self._solo = None                # a private one-scene set holds the old map's address
        return self.region

    def maxmin(self, overlap_padding=(0, 0)):
        """Two lists of ``[min, max]`` per band, of scene x and of scene y: the TRUE masked extrema over the tiling of this scene
        with its own patch size and ``overlap_padding``, taken on the device (``_ops.scene_minmax``; mask = band sum of scene x
        non-zero) -- what ``dataset_maxmin`` returns whenever no valid sample is 0 and every band has a positive maximum.  Two
        quirks of the reference's fold are NOT imitated: it treats a running minimum of exactly 0 as unset (so a valid 0 sample
        can be lost as the minimum) and starts the maximum at 0 (so an all-negative band returns 0).  A tile without a valid
        pixel is skipped; the reference raises on such a tile.  Float32 scenes: NaN samples are skipped, +-inf take part.
        ``stats_count`` keeps the number of valid pixels."""
        lo_x, hi_x, lo_y, hi_y = self._scan('scene_minmax', overlap_padding)
        return ([[float(a), float(b)] for a, b in zip(lo_x, hi_x)], [[float(a), float(b)] for a, b in zip(lo_y, hi_y)])

    def _scan(self, op, overlap_padding):
        """``_ops.scene_stats`` / ``_ops.scene_minmax`` over the tiling of this scene with its own patch size and
        ``overlap_padding``: the four per-band arrays; the valid-pixel count goes to ``stats_count``."""
        from . import _ops as ops
        grid = TileGrid(self.grid.xsize, self.grid.ysize, self.grid.patch_size, overlap_padding)
        *out, self.stats_count = getattr(ops, op)(self.x, self.y, ops.scene_tile_table(grid, range(len(grid))),
                                                  sample_type=self.sample_type)
        return tuple(out)

    def statistics(self, overlap_padding=(0, 0)):
        """``(meanX, stdX, meanY, stdY)`` as float64 arrays: CommonFunc.Dataset_mean / Dataset_std over the tiling of this scene
        with its own patch size and ``overlap_padding`` -- what ``demos._tile_stats`` computes on the host, here in one pass
        over the resident samples (``_ops.scene_stats``).  The values are the EXACT masked moments (integer scenes) or their
        fp64 evaluation (float32); the host functions round every tile mean to fp32, so the two routes agree to about seven
        digits.  Where the reference gives NaN (a tile without a valid pixel: mean of an empty selection times weight 0) this
        gives the finite statistic of the remaining tiles.  ``stats_count`` keeps the number of valid pixels."""
        return self._scan('scene_stats', overlap_padding)

    def __len__(self):
        return len(self.grid)

    def table(self, items):
        from . import _ops as ops
        return items if isinstance(items, ops.TileTable) else ops.scene_tile_table(self.grid, items)

    def cut(self, items, raw=False):
        """``(x, y, ref, valid)`` of the tiles ``items`` (indices or a tile table), all on the device: x, y as
        ``PairTileDataset.__getitem__`` returns them (normalised with ``stats`` when given) or, with ``raw=True``, as
        ``raw_item`` does (plain samples -- for ``Segmentor.forward_raw``); ``ref`` (None without a reference map) and the
        ``valid`` window mask are (n,1,py,px).  A scene with an enhancer (``set_enhance``) is cut with it, like
        ``PairTileDataset(enhance=)``."""
        from . import _ops as ops
        if self.enhance_kind > 1 and not raw:
            # SCALE / SCALE_NORM: the set cut has the modes -- a private one-scene set over the same tensors, same tiles
            table = self.table(items)
            if table.items is None:
                raise ops._lib.FcdError('ResidentScene.cut: with SCALE / SCALE_NORM pass tile indices or a table made from them')
            if self._solo is None:
                self._solo = ResidentSceneSet([self])
            x, y, ref, _, valid = ops.scene_set_cut(self._solo._descs, self._solo.table, self._solo.index(table.items), self.bands,
                                                    self.sample_type, stats=self._solo._stats_dev, want_ref=self.ref is not None,
                                                    want_region=False, mode=self.enhance_kind,
                                                    scale=self.enhance_scale or (-1, 1))
            return x, y, ref, valid
        return ops.scene_cut(self.x, self.y, self.table(items), ref=self.ref, stats=None if raw else self._stats_dev,
                             sample_type=self.sample_type, ref_type=self.ref_type if self.ref is not None else None)

    def new_maps(self):
        """Zeroed ``density`` and ``color`` maps, (1,H,W) float32 on the device."""
        shape = (1, self.grid.ysize, self.grid.xsize)
        return (torch.zeros(shape, dtype=torch.float32, device=self.device),
                torch.zeros(shape, dtype=torch.float32, device=self.device))


class EpochWeight(float):
    """A batch's epoch weight ``n_real / len(dataset)`` (a float) that also carries the step's ``loss_scale`` (``dp`` ragged=
    'weighted') and, on the resident feed, ``rects``: the metric's rectangles of the batch's real tiles, on the device
    (``Evaluator.add_tiles``); None when the batch holds no real tile."""
    loss_scale = 1.0
    rects = None


class EpochPlan:
    """What one rank does in one epoch, known before its first batch: ``batches`` (lists of global items), ``pads`` (trailing
    padded duplicates per batch), ``scales`` (loss scale per batch) -- ``dp.RankStridedBatches``'s, same seed, same order --
    and ``flat`` / ``offsets``: all batches laid end to end, batch b = ``flat[offsets[b]:offsets[b + 1]]``.  Pure host code."""

    def __init__(self, n, batch_size, seed, shuffle=True, ragged='pad', rank=None, world=None):
        from . import dp
        sampler = dp.RankStridedBatches(n, batch_size, seed=seed, shuffle=shuffle, rank=rank, world=world, ragged=ragged)
        self.batches = [list(b) for b in sampler]
        self.pads, self.scales, self.n = list(sampler.pads), list(sampler.scales), int(n)
        self.flat = [i for b in self.batches for i in b]
        self.offsets = [0]
        for b in self.batches:
            self.offsets.append(self.offsets[-1] + len(b))

    def __len__(self):
        return len(self.batches)


def check_scene_set(scenes):
    """Raise FcdError unless the scenes of a set share band count, sample type, patch size, padding and device (host check;
    reads ``bands``, ``sample_type``, ``grid.patch_size``, ``grid.pad`` and ``device`` only)."""
    from . import _ops as ops
    scenes = list(scenes)
    if not scenes:
        raise ops._lib.FcdError('ResidentSceneSet: no scene')
    for what, get in (('band count', lambda s: s.bands), ('sample type', lambda s: s.sample_type),
                      ('patch size', lambda s: tuple(s.grid.patch_size)), ('overlap padding', lambda s: tuple(s.grid.pad)),
                      ('device', lambda s: s.device)):
        got = [get(s) for s in scenes]
        if any(g != got[0] for g in got):
            raise ops._lib.FcdError('ResidentSceneSet: the scenes must share one %s, got %s' % (what, got))
    # one enhancement mode per launch: the scenes that have an enhancer share its kind and, for SCALE_NORM, its range
    # (scenes without one stay raw)
    kinds = [(getattr(s, 'enhance_kind', 0), getattr(s, 'enhance_scale', None)) for s in scenes]
    kinds = [k for k in kinds if k[0]]
    if any(k != kinds[0] for k in kinds):
        raise ops._lib.FcdError('ResidentSceneSet: the scenes must share one enhancer kind (and SCALE_NORM range), got %s' % (kinds,))


class ResidentSceneSet:
    """Several ``ResidentScene`` of different sizes as ONE training set -- ``datasets.MultiSceneDataset`` over
    ``RegionTileDataset`` with everything on the device.  Copies nothing: a descriptor table holds the scenes' addresses
    (the set keeps the scenes alive), the table of all tiles goes up once, and a batch is a list of global items cut in one
    launch (``_ops.scene_set_cut``) with each tile normalised by its own scene's statistics.  The scenes share band count,
    sample type, patch size and padding.  Statistics are read when the set is made: call :meth:`refresh` after
    ``ResidentScene.set_stats``."""

    def __init__(self, scenes, names=None, transforms=None):
        from . import _ops as ops
        self.scenes = list(scenes)
        check_scene_set(self.scenes)
        # ``transforms``: one eraser of ``transforms`` for every scene, or a list with one per scene (None entries allowed), as
        # OSCD_Dataset_RSS takes them; used by :meth:`epoch` only (``cut`` erases what it is handed)
        if transforms is not None and not isinstance(transforms, (list, tuple)):
            transforms = [transforms] * len(self.scenes)
        if transforms is not None and len(transforms) != len(self.scenes):
            raise ValueError("The list of transforms doesn't match the file list")          # data_utils.py:354-356
        self.transforms = None if transforms is None or all(t is None for t in transforms) else list(transforms)
        self.names = list(names) if names is not None else ['scene%d' % i for i in range(len(self.scenes))]
        self.numlist = [len(s) for s in self.scenes]
        self.cumlen = np.cumsum(np.array(self.numlist)).tolist()
        first = self.scenes[0]
        self.device, self.bands, self.sample_type = first.x.device, first.bands, first.sample_type
        self.patch_size, self.pad = first.grid.patch_size, first.grid.pad
        self.table = ops.scene_set_table([s.grid for s in self.scenes])
        self.refresh()

    def refresh(self):
        """Rebuild the descriptor table and the statistics array from the scenes' current tensors and statistics (after
        ``ResidentScene.set_stats`` / ``set_enhance`` / ``derive_region`` on a scene of the set)."""
        C = self.bands
        check_scene_set(self.scenes)
        self.has_ref = any(s.ref is not None for s in self.scenes)
        self.has_region = any(s.region is not None for s in self.scenes)
        kinds = [(s.enhance_kind, s.enhance_scale) for s in self.scenes if s.enhance_kind]
        self.mode, self.scale = (kinds[0][0], kinds[0][1] or (-1.0, 1.0)) if kinds else (1, (-1.0, 1.0))
        rows, stats = [], []
        for s in self.scenes:
            off = -1
            if s._stats_dev is not None:
                off = 4 * C * len(stats)
                stats.append(s._stats_dev.reshape(-1))
            rows.append([s.x.data_ptr(), s.y.data_ptr(), 0 if s.ref is None else s.ref.data_ptr(),
                         0 if s.region is None else s.region.data_ptr(), s.grid.ysize, s.grid.xsize, off,
                         (s.ref_type or 0) | ((s.region_type or 0) << 32)])
        # scenes without statistics keep offset -1; the array is indexed by the offsets alone, padded to S rows for the check
        pad = [torch.zeros(4 * C, dtype=torch.float64, device=self.device)] * (len(self.scenes) - len(stats))
        self._stats_dev = torch.cat(stats + pad) if stats else None
        self._descs = torch.from_numpy(np.array(rows, dtype=np.int64)).to(self.device)

    def __len__(self):
        return int(sum(self.numlist))

    def locate(self, item):
        """global item -> (scene index, item within the scene)  (data_utils.py:375-376)."""
        item = int(item)
        if item >= self.cumlen[-1] or item < 0:
            raise IndexError('item exceeds the len')
        ds = int(np.where(np.array(self.cumlen) > item)[0][0])
        return ds, (item - self.cumlen[ds - 1] if ds > 0 else item)

    def eff_range(self, item):
        ds, cur = self.locate(item)
        return self.scenes[ds].grid.eff_range(cur)

    def index(self, items):
        """The validated device copy of a list of global items (``_ops.TileIndex``): one upload, sliceable."""
        from . import _ops as ops
        return items if isinstance(items, ops.TileIndex) else ops.TileIndex(items, len(self.table), self.device)

    def rects(self, index, n=None):
        """The metric's rectangles (``eff_range``) of the first ``n`` tiles of ``index``, resident (``Evaluator.add_tiles``)."""
        from . import _ops as ops
        return ops.DeviceRects(self.table, self.index(index), n)

    def erase_rects(self, regions, n):
        """The validated rectangles (``_ops.EraseRects``) of ``n`` tiles from host regions, with as many slots per tile as the
        set's erasers can draw (16 without erasers)."""
        from . import _ops as ops
        R = max(t.max_regions for t in self.transforms if t is not None) if self.transforms else ops.ERASE_MAX
        return ops.erase_rects(regions, n, R, self.patch_size)

    def cut(self, items, raw=False, out=None, want_valid=True, erase=None):
        """``(x, y, ref, region, valid)`` of the global ``items`` (a list, or the ``TileIndex`` :meth:`index` returns), all on the
        device: x, y, ref as ``MultiSceneDataset([RegionTileDataset...])[i]`` returns them (each tile normalised with its own
        scene's statistics; ``raw=True``: plain samples), ``region`` binarised like data_utils.py:280, ``valid`` the window
        mask of ``raw_item``.  A scene without a reference / region map gives zero tiles.  The scenes' enhancer decides the
        formula (NORMALIZE, SCALE or SCALE_NORM).  ``erase``: one region per item as the erasers of ``transforms`` return them
        (or the ``EraseRects`` made from them), blanked in x and y alike; not with ``raw=True``."""
        from . import _ops as ops
        index = self.index(items)
        if erase is not None:
            if raw:
                raise ValueError('cut: erasing has no raw route (erase after normalisation)')
            if not isinstance(erase, ops.EraseRects):
                erase = self.erase_rects(erase, len(index))
        return ops.scene_set_cut(self._descs, self.table, index, self.bands, self.sample_type,
                                 stats=None if raw else self._stats_dev, want_valid=want_valid, out=out, mode=self.mode,
                                 scale=self.scale, erase=erase)

    def new_maps(self):
        """The zeroed output maps of the set (``_ops.SceneSetMaps``): one flat density and one flat colour buffer that hold the
        maps of all scenes end to end, the resident offsets, and ``density[s]`` / ``color[s]`` as (1,H_s,W_s) views."""
        from . import _ops as ops
        return ops.SceneSetMaps(self.table, self.device)

    def stitch(self, cmap, index, maps, n=None, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), write_color=True,
               scene_counts=None):
        """Write the owned centres of the first ``n`` density tiles ``cmap`` -- tile t = global item ``index[t]`` (the
        ``TileIndex`` of :meth:`index`, or a list) -- into ``maps`` (:meth:`new_maps`), each into its own scene's maps,
        colour-coded against that scene's reference map and counted per scene into ``scene_counts`` (device int64 (S,4)): one
        launch for tiles of several scenes (``_ops.scene_set_stitch``), the way out of what :meth:`cut` is the way in."""
        from . import _ops as ops
        return ops.scene_set_stitch(cmap, self._descs, self.table, self.index(index), maps, n=n, prob_thresh=prob_thresh,
                                    gt_map=gt_map, pre_map=pre_map, write_color=write_color, scene_counts=scene_counts)

    def epoch(self, batch_size, seed, shuffle=True, ragged='pad', rank=None, world=None):
        """An iterable with ``demos._Epoch``'s contract, ``((x, y, item, ref[, region]), n_real, weight)`` -- ``region`` when a
        scene of the set has one, ``item`` a CPU int64 tensor, ``weight`` an ``EpochWeight`` -- over the batches, pads and
        scales of ``dp.RankStridedBatches`` with the same seed."""
        return _ResidentEpoch(self, batch_size, seed, shuffle, ragged, rank, world)


class _ResidentEpoch:
    def __init__(self, scene_set, batch_size, seed, shuffle, ragged, rank, world):
        self.set = scene_set
        self.args = (len(scene_set), batch_size, seed, shuffle, ragged, rank, world)

    def __len__(self):
        return len(EpochPlan(*self.args))

    def __iter__(self):
        # the whole plan is known here: this rank's index list goes up ONCE (pinned, asynchronous) and every batch is cut from a
        # slice of it -- inside the epoch there is no host-to-device copy and nothing that makes the host wait for the device
        plan = EpochPlan(*self.args)
        index = self.set.index(plan.flat) if plan.flat else None
        return self._batches(plan, index, self._draw(plan))

    def _draw(self, plan):
        """With erasers: the regions of every entry of the flat plan, drawn here in plan order -- padded duplicates included, as
        the host loader fetches and draws them again -- each from its own scene's eraser, and uploaded ONCE next to the index."""
        s = self.set
        if s.transforms is None or not plan.flat:
            return None
        shape = (s.bands, s.patch_size[1], s.patch_size[0])
        regions = []
        for item in plan.flat:
            t = s.transforms[s.locate(item)[0]]
            regions.append(None if t is None else t.draw(shape))
        return s.erase_rects(regions, len(plan.flat)).to(s.device)

    def _batches(self, plan, index, rects=None):
        s = self.set
        for b, items in enumerate(plan.batches):
            part = index[plan.offsets[b]:plan.offsets[b + 1]]
            erase = None if rects is None else rects[plan.offsets[b]:plan.offsets[b + 1]]
            x, y, ref, region, _ = s.cut(part, want_valid=False, erase=erase)
            real = len(items) - plan.pads[b]
            w = EpochWeight(real / float(plan.n))
            w.loss_scale = plan.scales[b]
            w.rects = s.rects(part, real) if real > 0 else None
            item = torch.tensor(items, dtype=torch.int64)
            yield ((x, y, item, ref, region) if s.has_region else (x, y, item, ref)), real, w


# ------------------------------------------------------------------------ dataset statistics
def _valid(x):
    """Valid-pixel mask of a patch: pixels whose band sum is non-zero (nodata / zero padding excluded,
    CommonFunc.py:446) -- taken from the FIRST scene for both scenes, as the reference does."""
    return torch.sum(x, dim=0) != 0


def dataset_mean(dataset):
    """Per-band mean of both scenes over the valid pixels of all patches (CommonFunc.Dataset_mean,
    CommonFunc.py:436-465): per-patch means weighted by the patch's valid-pixel count."""
    npix, mx, my = [], [], []
    for i in range(len(dataset)):
        item = dataset[i]
        x, y = item[0], item[1]
        idx = _valid(x)
        npix.append(torch.sum(idx))
        mx.append(torch.mean(x[:, idx], 1))
        my.append(torch.mean(y[:, idx], 1))
    mx = torch.cat(mx).reshape(len(mx), -1)
    my = torch.cat(my).reshape(len(my), -1)
    npix = torch.tensor(npix).reshape(-1, 1)
    w = npix.repeat(1, mx.size()[1]) / torch.sum(npix)
    return torch.sum(mx * w, dim=0), torch.sum(my * w, dim=0)


def dataset_std(dataset, mean_x, mean_y):
    """Per-band standard deviation around the given means (CommonFunc.Dataset_std, CommonFunc.py:467-500):
    per-patch mean squared deviations weighted by n_i / (N - 1)."""
    npix, vx, vy = [], [], []
    mean_x = mean_x.reshape(-1, 1)
    mean_y = mean_y.reshape(-1, 1)
    for i in range(len(dataset)):
        item = dataset[i]
        x, y = item[0], item[1]
        idx = _valid(x)
        n = torch.sum(idx)
        npix.append(n)
        vx.append(torch.mean(torch.square(x[:, idx] - mean_x.repeat(1, n)), 1))
        vy.append(torch.mean(torch.square(y[:, idx] - mean_y.repeat(1, n)), 1))
    vx = torch.cat(vx).reshape(len(vx), -1)
    vy = torch.cat(vy).reshape(len(vy), -1)
    npix = torch.tensor(npix).reshape(-1, 1)
    w = npix.repeat(1, vx.size()[1]) / (torch.sum(npix) - 1)
    return torch.sqrt(torch.sum(vx * w, dim=0)), torch.sqrt(torch.sum(vy * w, dim=0))


def _cached_rows(paths, labels, compute, fmt):
    """The reference's text cache behind the four ``*_meanstd`` / ``*_maxmin`` functions: two files of two rows each,
    ``label: v v ...``.  Both files there: read back, ``((row, row), (row, row))`` of float lists.  Else ``compute()`` returns
    those rows of floats, which are written -- every value through ``fmt``: ``str``, or ``repr`` where the round trip must be
    exact; either text loads here -- and returned."""
    if not all(os.path.exists(p) for p in paths):
        files = compute()
        for path, rows in zip(paths, files):
            with open(path, 'w') as f:
                for label, row in zip(labels, rows):
                    f.write(label + ':' + ''.join(' {}'.format(fmt(v)) for v in row) + '\n')
        return files
    files = []
    for path in paths:
        with open(path) as f:
            lines = f.readlines()
        files.append(([float(v) for v in lines[0].split()[1:]], [float(v) for v in lines[1].split()[1:]]))
    return tuple(files)


def dataset_meanstd(txt_x, txt_y, dataset):
    """``(meanX, stdX, meanY, stdY)`` as lists of floats, cached in two text files in the reference's
    format (``mean: v v ...`` / ``std: v v ...``; CommonFunc.Dataset_meanstd, CommonFunc.py:373-434):
    computed and written when either file is missing, read back otherwise."""
    def compute():
        mx, my = dataset_mean(dataset)
        sx, sy = dataset_std(dataset, mx, my)
        return (mx.numpy().tolist(), sx.numpy().tolist()), (my.numpy().tolist(), sy.numpy().tolist())
    (mx, sx), (my, sy) = _cached_rows((txt_x, txt_y), ('mean', 'std'), compute, str)
    return mx, sx, my, sy


def scene_meanstd(txt_x, txt_y, scene, overlap_padding=(0, 0)):
    """``dataset_meanstd`` for a ``ResidentScene``: ``(meanX, stdX, meanY, stdY)`` as lists of floats, cached in the same two
    text files -- read back when both exist, else taken on the device (``scene.statistics``) and written.  The values are
    written with ``repr``, so reading them back is exact; files written by either function load in the other."""
    def compute():
        mx, sx, my, sy = ([float(v) for v in a] for a in scene.statistics(overlap_padding))
        return (mx, sx), (my, sy)
    (mx, sx), (my, sy) = _cached_rows((txt_x, txt_y), ('mean', 'std'), compute, repr)
    return mx, sx, my, sy


def _fold_maxmin(dataset):
    """The per-tile fold of CommonFunc.Dataset_maxmin (CommonFunc.py:298-324), quirks included: the running minimum counts as
    unset while it is exactly 0, and the maximum starts at 0 (an all-negative band returns 0).  A tile without a valid pixel
    raises, as the reference does (``torch.max`` of an empty selection)."""
    a1 = a2 = None
    for i in range(len(dataset)):
        item = dataset[i]
        x, y = item[0], item[1]
        if a1 is None:
            a1 = [[0.0, 0.0] for _ in range(x.size()[0])]
            a2 = [[0.0, 0.0] for _ in range(y.size()[0])]
        idx = _valid(x)
        for a, t in ((a1, x), (a2, y)):
            hi = torch.max(t[:, idx], dim=1)[0]
            lo = torch.min(t[:, idx], dim=1)[0]
            for b in range(t.size()[0]):
                a[b][0] = float(lo[b]) if a[b][0] == 0 else a[b][0]
                a[b][0] = float(lo[b]) if lo[b] < a[b][0] else a[b][0]
                a[b][1] = float(hi[b]) if hi[b] > a[b][1] else a[b][1]
    return a1, a2


def _cached_maxmin(txt1, txt2, compute, fmt):
    """``_cached_rows`` for two lists of ``[min, max]`` per band: the files hold a ``max:`` row above a ``min:`` row."""
    files = _cached_rows((txt1, txt2), ('max', 'min'),
                         lambda: tuple(([r[1] for r in a], [r[0] for r in a]) for a in compute()), fmt)
    return tuple([[lo, hi] for hi, lo in zip(*rows)] for rows in files)


def dataset_maxmin(txt1, txt2, dataset):
    """Two lists of ``[min, max]`` per band, of scene x and of scene y, over the valid pixels of all patches of an UNENHANCED
    tile dataset (CommonFunc.Dataset_maxmin, CommonFunc.py:294-370; the mask comes from the first scene), cached in the
    reference's two text files (``max: v v ...`` / ``min: v v ...``): computed and written when either file is missing, read
    back otherwise.  These are the ranges ``transforms.SCALE`` / ``SCALE_NORM`` take."""
    return _cached_maxmin(txt1, txt2, lambda: _fold_maxmin(dataset), str)


def scene_maxmin(txt1, txt2, scene, overlap_padding=(0, 0)):
    """``dataset_maxmin`` for a ``ResidentScene``: the same two text files -- read back when both exist, else taken on the device
    (``scene.maxmin``) and written with ``repr``, so reading them back is exact; files of either function load in the other."""
    return _cached_maxmin(txt1, txt2, lambda: scene.maxmin(overlap_padding), repr)


def normalize_(x, mean, std):
    """In-place per-band (x - mean) / std of an (N,C,H,W) device tensor (NORMALIZE on device)."""
    m = torch.as_tensor(mean, dtype=x.dtype, device=x.device).view(1, -1, 1, 1)
    s = torch.as_tensor(std, dtype=x.dtype, device=x.device).view(1, -1, 1, 1)
    return x.sub_(m).div_(s)


class Prefetcher:
    """Iterate a DataLoader-like iterable of tensor tuples from a background thread, staging
    each batch through pinned host memory and an asynchronous H2D copy on a side stream, so
    tile loading overlaps the train step (the reference loads on the main thread,
    num_workers=0, Demo_RSSS.py:242)."""

    def __init__(self, loader, device, depth=2):
        self.loader, self.device, self.depth = loader, torch.device(device), depth
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None

    def __iter__(self):
        q = queue.Queue(maxsize=self.depth)
        stop = object()
        failure = []

        def work():
            try:
                for batch in self.loader:
                    out = []
                    for t in batch:
                        if torch.is_tensor(t) and t.is_floating_point() and self.stream is not None:
                            p = t.pin_memory()
                            with torch.cuda.stream(self.stream):
                                d = p.to(self.device, non_blocking=True)
                            out.append((d, p))
                        else:
                            out.append((t, None))
                    ev = None
                    if self.stream is not None:
                        ev = torch.cuda.Event()
                        ev.record(self.stream)
                    q.put((out, ev))
            except BaseException as e:          # surfaced in the consumer: a dying loader must not end the epoch quietly
                failure.append(e)
            finally:
                q.put(stop)
        th = threading.Thread(target=work, daemon=True)
        th.start()
        while True:
            item = q.get()
            if item is stop:
                break
            out, ev = item
            if ev is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                for d, p in out:
                    if p is not None:
                        # the block was allocated on the copy stream: tell the caching allocator that the consumer
                        # stream uses it too, or it may be handed to the worker's next H2D copy while train-step
                        # kernels queued on the main stream still read it (the step functions never sync the host)
                        d.record_stream(cur)
            yield tuple(d for d, _ in out)
        th.join()
        if failure:
            raise failure[0]
