"""Drop-in for the reference's ``ssim.py`` public surface -- ``ssim``, ``ms_ssim``,
``SSIM``, ``MS_SSIM`` with the same arguments, defaults and exceptions -- on the
fused HIP SSIM-level kernels: per level ONE kernel reads X and Y once, forms the
five Gaussian-window statistics on chip and reduces the ssim/cs maps per (n,c);
the padded 2x average pool between levels is a second small kernel.  Only the
O(levels*N*C) tail (relu, powers, product, mean) uses torch ops.
 * 2-D images (N,C,H,W): csrc/ssim.hip (one plane tile per workgroup) and the 2x2 pool;
 * volumes (N,C,T,H,W) -- the reference's ``conv3d`` / ``avg_pool3d`` branch (ssim.py:35-38,181-184), what
   ``SSIM(spatial_dims=3)`` / ``MS_SSIM(spatial_dims=3)`` are for: csrc/ssim3d.hip (a workgroup walks the depth axis of its
   plane tile) and the 2x2x2 pool.  As in the reference, trailing dimensions of extent 1 are squeezed first, so (N,C,1,H,W)
   is a 2-D case; any other rank raises the reference's ValueError.
Odd window <= 11 taps, float32 CUDA/ROCm tensors only (no CPU fallback).

Deliberate difference from the vendored pytorch-msssim (not on a demo's path; it RAISES instead of silently computing
something else):
 * windows longer than 11 taps -> error, for both ranks.
``gaussian_filter``'s "skip a spatial dimension shorter than the window, with a warning" (ssim.py:44-50) is reproduced [r4]: the
kernels apply the single tap 1 along such a dimension, independently per dimension.  For 2-D inputs this concerns ``ssim``
only (MS-SSIM's own assert, ssim.py:194-197, requires min(H, W) > 160 for the default window); the assert does not look at
T, so a volumetric ``ms_ssim`` skips the depth smoothing -- and warns -- at every level whose T is below the window.
A volumetric ``ms_ssim`` pools T as well; like the reference's ``avg_pool3d`` it raises RuntimeError when a level that is
pooled has an extent of 1 (five levels need T >= 9), here before anything is launched.
"""
import warnings

import torch

from . import _ops as ops

_DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # reference ssim.py:200


def _fspecial_gauss_1d(size, sigma):
    """1-D Gaussian taps as a (1,1,size) float tensor (reference ssim.py:9-23)."""
    offs = torch.arange(size, dtype=torch.float32) - (size // 2)
    g = torch.exp(-(offs * offs) / (2 * sigma ** 2))      # host-side, 11 numbers, fp32 like the reference
    return (g / g.sum()).view(1, 1, size)


_DEV_CONST = {}


def _dev_const(values, device):
    """A small constant vector on the device, uploaded ONCE per (values, device): the window taps and the level weights are the
    same 11 + 5 numbers in every call, and a host-to-device copy per call is both two launches per step and the one thing in the
    loss that a hipGraph capture of the train step cannot record (a caller's own ``torch.cuda.graph``)."""
    key = (tuple(float(v) for v in values), str(device))
    t = _DEV_CONST.get(key)
    if t is None:
        t = _DEV_CONST[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return t


def _taps_from(win, device):
    """Accept the reference's (C,1,1,k) / (C,1,1,1,k) / (1,1,k) window tensors; return the k taps."""
    w = win.reshape(-1, win.shape[-1])[0]
    if w.is_cuda:
        return w.to(device=device, dtype=torch.float32).contiguous()
    return _dev_const(w.tolist(), device)


def _check_pair(X, Y):
    if not X.shape == Y.shape:
        raise ValueError("Input images should have the same dimensions.")
    for d in range(len(X.shape) - 1, 1, -1):
        X = X.squeeze(dim=d)
        Y = Y.squeeze(dim=d)
    if not X.type() == Y.type():
        raise ValueError("Input images should have the same dtype.")
    return X, Y


def _warn_skipped(shape, win_size):
    """The reference's warning, from gaussian_filter (ssim.py:46-50): once per spatial dimension shorter than the window."""
    for i, sdim in enumerate(shape[2:]):
        if sdim < win_size:
            warnings.warn(f"Skipping Gaussian Smoothing at dimension 2+{i} for input: {shape} and win size: {win_size}")


def _pooled_shapes(shape, levels):
    """Shapes of the ``levels`` inputs of a volumetric MS-SSIM (avg_pool3d(2, padding = s % 2) between them); raises the
    pool's RuntimeError for a level that would have to pool an extent of 1 -- before any level is computed."""
    shapes = [tuple(shape)]
    for _ in range(levels - 1):
        ops.check_pool3d_extents(shapes[-1])
        shapes.append(shapes[-1][:2] + tuple((s + 2 * (s % 2) - 2) // 2 + 1 for s in shapes[-1][2:]))
    return shapes


def _consts(data_range, K):
    return (K[0] * data_range) ** 2, (K[1] * data_range) ** 2


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """Single-scale SSIM (reference ssim.py:95-150)."""
    X, Y = _check_pair(X, Y)
    if len(X.shape) not in (4, 5):
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    taps = _taps_from(win if win is not None else _fspecial_gauss_1d(win_size, win_sigma), X.device)
    _warn_skipped(X.shape, win_size)
    C1, C2 = _consts(data_range, K)
    per_channel, _ = ops.ssim_level(X, Y, taps, C1, C2)
    if nonnegative_ssim:
        per_channel = torch.relu(per_channel)
    return per_channel.mean() if size_average else per_channel.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None,
            K=(0.01, 0.03)):
    """Multi-scale SSIM (reference ssim.py:153-225): 5 levels, avg_pool2d / avg_pool3d(2, padding=s%2)
    between levels, relu on cs (levels 0-3) / ssim (level 4), product of powers."""
    X, Y = _check_pair(X, Y)
    if len(X.shape) not in (4, 5):
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((win_size - 1) * (2 ** 4))
    volume = len(X.shape) == 5
    if volume:                                        # the pool's RuntimeError, before anything touches the device
        _pooled_shapes(X.shape, len(weights) if weights is not None else len(_DEFAULT_WEIGHTS))
    w = _dev_const(list(weights) if weights is not None else list(_DEFAULT_WEIGHTS), X.device).to(X.dtype)
    taps = _taps_from(win if win is not None else _fspecial_gauss_1d(win_size, win_sigma), X.device)
    C1, C2 = _consts(data_range, K)
    levels = w.shape[0]
    terms = []
    for lvl in range(levels):
        if volume:                                    # T is not covered by the assert: levels may skip its smoothing
            _warn_skipped(X.shape, win_size)
        s_c, cs = ops.ssim_level(X, Y, taps, C1, C2)
        if lvl < levels - 1:
            terms.append(torch.relu(cs))
            X = ops.avgpool2_pad(X)
            Y = ops.avgpool2_pad(Y)
    terms.append(torch.relu(s_c))
    # prod_l term_l ** w_l (reference ssim.py:219-222: torch.prod over the stacked levels).  Written as a chain of products:
    # torch.prod's backward counts the zeros of its input with ``.item()`` -- a host synchronisation in the middle of every
    # backward pass that runs through MS-SSIM (the USSS steps), and not capturable in a hipGraph.  The chain's gradient w.r.t. a
    # level is the product of the other levels, which is what prod_backward computes on its zero-safe path.
    val = terms[0] ** w[0]
    for lvl in range(1, levels):
        val = val * terms[lvl] ** w[lvl]
    return val.mean() if size_average else val.mean(1)


class SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 K=(0.01, 0.03), nonnegative_ssim=False):
        super(SSIM, self).__init__()
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 weights=None, K=(0.01, 0.03)):
        super(MS_SSIM, self).__init__()
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win,
                       weights=self.weights, K=self.K)
