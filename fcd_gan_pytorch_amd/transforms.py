"""The reference's pre-processing hooks (CommonFunc.py:78-224) as host objects: the three *enhancers* ``NORMALIZE``, ``SCALE``
and ``SCALE_NORM`` (the ``enhance=`` hook of the dataset classes, called as ``enh(X, switch=1 or 2)`` on a (bands, h, w) block)
and the paired augmentation ``RANDOM_ERASER`` / ``RANDOM_ERASER_MULTI_REGION`` (the ``transforms=`` hook: ``x, sync = t(x)``
then ``y, _ = t(y, sync)`` blanks the same rectangles in both dates).  Class names, constructor arguments and call signatures
are the reference's; two things are added for the device route:

 * every enhancer has ``kind`` (1, 2, 3 = the C ABI's FCD_ENHANCE_*) and ``params(C)``, the (4, C) float64 array the set-cut
   kernel reads, so the same object configures ``tiles.PairTileDataset`` and ``tiles.ResidentScene``;
 * every eraser splits ``forward`` into ``draw(shape) -> region`` and ``apply(img, region)``: the resident feed draws the regions
   of a whole epoch on the host -- the same calls to ``random`` in the same order -- and erases on the device.

Where the reference prints a message and calls ``sys.exit``, these raise ``ValueError`` with that message."""
import math
import random

import numpy as np


class _Enhancer:
    kind = 0

    def __call__(self, X, switch=1):
        return self.forward(X, switch)

    def _rows(self):
        """((first row, second row, message), ...) for switch 1 and switch 2."""
        raise NotImplementedError

    def _check(self, nchannel, switch):
        a, b, msg = self._rows()[0 if switch == 1 else 1]
        if nchannel > len(a):
            raise ValueError(msg)
        return a, b

    def params(self, C):
        """(4, C) float64: the per-band parameters of scene x (two rows), then of scene y (two rows)."""
        C = int(C)
        out = np.empty((4, C), np.float64)
        for k, switch in enumerate((1, 2)):
            a, b = self._check(C, switch)
            out[2 * k] = [float(a[c]) for c in range(C)]
            out[2 * k + 1] = [float(b[c]) for c in range(C)]
        return out


class NORMALIZE(_Enhancer):
    """Zero mean and unit std per band: ``(X[b] - mean[b]) / std[b]``, in place."""
    kind = 1

    def __init__(self, meansX, stdX, meansY, stdY):
        self.meansX, self.stdX, self.meansY, self.stdY = meansX, stdX, meansY, stdY

    def _rows(self):
        msg = "The input channel doesn't match the stats list"
        return (self.meansX, self.stdX, msg), (self.meansY, self.stdY, msg)

    def forward(self, X, switch=1):
        mean, std = self._check(X.shape[0], switch)
        for b in range(X.shape[0]):
            X[b] = (X[b] - mean[b]) / std[b]
        return X


class SCALE(_Enhancer):
    """From the per-band value range [lo, hi] to [0, 1]: ``(X[b] - lo) / (hi - lo)``, in place."""
    kind = 2

    def __init__(self, scale_list1=[[0, 255], [0, 255], [0, 255]], scale_list2=[[0, 255], [0, 255], [0, 255]]):
        self.scale_list1, self.scale_list2 = scale_list1, scale_list2

    def _rows(self):
        return tuple(([r[0] for r in ranges], [r[1] for r in ranges], "The input channel doesn't match the %s list" % what)
                     for ranges, what in ((self.scale_list1, 'range'), (self.scale_list2, 'scale')))

    def _ranges(self, nchannel, switch):
        self._check(nchannel, switch)
        return self.scale_list1 if switch == 1 else self.scale_list2

    def forward(self, X, switch=1):
        ranges = self._ranges(X.shape[0], switch)
        for b in range(X.shape[0]):
            X[b] = (X[b] - ranges[b][0]) / (ranges[b][1] - ranges[b][0])
        return X


class SCALE_NORM(SCALE):
    """From the per-band value range to ``scale``: ``(s1 - s0) * (X[b] - lo) / (hi - lo) + s0``, evaluated in that order."""
    kind = 3

    def __init__(self, scale_list1=[[0, 255], [0, 255], [0, 255]], scale_list2=[[0, 255], [0, 255], [0, 255]], scale=[-1, 1]):
        super().__init__(scale_list1, scale_list2)
        self.scale = scale

    def forward(self, X, switch=1):
        ranges = self._ranges(X.shape[0], switch)
        for b in range(X.shape[0]):
            X[b] = (self.scale[1] - self.scale[0]) * (X[b] - ranges[b][0]) / (ranges[b][1] - ranges[b][0]) + self.scale[0]
        return X


class _Eraser:
    max_regions = 1

    def __init__(self, erase_thresh, origin_prob, rng):
        self.erase_thresh, self.origin_prob = erase_thresh, origin_prob
        self.rng = rng if rng is not None else random           # the module, like datasets.PairingDataset

    def __call__(self, img, region=None):
        return self.forward(img, region)

    def _rect(self, xsize, ysize):
        """One rectangle (x, y, w, h): four draws, then the area clamp -- which can leave h == 0."""
        r = self.rng
        x = r.randint(0, xsize - 1)
        y = r.randint(0, ysize - 1)
        w = r.randint(1, xsize - x)
        h = r.randint(1, ysize - y)
        if (w * h) / (xsize * ysize) > self.erase_thresh:
            h = math.floor(xsize * ysize * self.erase_thresh / w)
        return x, y, w, h

    def forward(self, img, region=None):
        if region is None:
            region = self.draw(img.shape)
        return self.apply(img, region), region


class RANDOM_ERASER(_Eraser):
    """With probability ``1 - origin_prob`` blank one random rectangle of at most ``erase_thresh`` of the image.
    ``forward(img, region=None) -> (img, region)``; the region of a kept image is ``(0, 0, 0, 0)``."""

    def __init__(self, erase_thresh=0.3, origin_prob=0.5, rng=None):
        super().__init__(erase_thresh, origin_prob, rng)

    def draw(self, shape):
        if self.rng.random() > self.origin_prob:
            band, ysize, xsize = shape
            return self._rect(xsize, ysize)
        return (0, 0, 0, 0)

    @staticmethod
    def apply(img, region):
        x, y, w, h = region
        img[:, y:y + h, x:x + w] = 0
        return img


class RANDOM_ERASER_MULTI_REGION(_Eraser):
    """With probability ``1 - origin_prob`` blank 1..``multi_region`` random rectangles, each clamped to ``erase_thresh`` of the
    image on its own.  The region is a list of ``[x, y, w, h]``, empty for a kept image."""

    def __init__(self, erase_thresh=0.3, origin_prob=0.2, multi_region=5, rng=None):
        super().__init__(erase_thresh, origin_prob, rng)
        self.multi_region = max(1, multi_region)

    @property
    def max_regions(self):
        return self.multi_region

    def draw(self, shape):
        region = []
        band, ysize, xsize = shape
        if self.rng.random() > self.origin_prob:
            for _ in range(self.rng.randint(1, self.multi_region)):
                region.append(list(self._rect(xsize, ysize)))
        return region

    @staticmethod
    def apply(img, region):
        for x, y, w, h in region:
            img[:, y:y + h, x:x + w] = 0
        return img


def enhancer(kind, rows1, rows2, scale=(-1, 1)):
    """The enhancer of ``kind`` ('normalize', 'scale', 'scale_norm') from per-scene parameters: ``rows1`` / ``rows2`` are
    (mean, std) for 'normalize' and lists of [min, max] per band (``tiles.dataset_maxmin``) for the other two."""
    if kind == 'normalize':
        return NORMALIZE(rows1[0], rows1[1], rows2[0], rows2[1])
    if kind == 'scale':
        return SCALE(rows1, rows2)
    if kind == 'scale_norm':
        return SCALE_NORM(rows1, rows2, list(scale))
    raise ValueError("enhance: 'normalize', 'scale' or 'scale_norm', got %r" % (kind,))
