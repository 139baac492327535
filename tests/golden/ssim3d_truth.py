"""Yardstick for the volumetric SSIM / MS-SSIM tests: a short functional statement of the (N, C, T, H, W) level and of the
five-level product on stock ``torch.nn.functional`` ops, in the dtype of its inputs (fp64 inputs give the truth the kernels
are measured against; fp32 inputs give the composition a user of stock ops would run).

It imports neither the package nor the reference.  ``ssim3d.npz`` (written by ``gen_golden_ssim3d.py`` from the reference
itself) pins it: tests/test_ssim3d_cpu.py runs every fixture case through this module.

Rules it states (reference ssim.py:26-52, 55-92, 153-225):
 * the 1-D window is applied VALID along T, then H, then W, as a depthwise ``conv3d``; a dimension shorter than the window is
   left as it is;
 * mu1, mu2, E[x^2], E[y^2], E[xy] -> cs = (2 s12 + C2) / (s1 + s2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs,
   each averaged over the whole output volume per (n, c);
 * MS-SSIM: relu(cs) of levels 0..L-2 and relu(ssim) of the last level, each to the power of its weight, multiplied;
   ``avg_pool3d(kernel 2, padding = extent % 2)`` between levels (padding counted: divisor 8).
"""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# shapes of the level cases (tests/test_gpu_ssim3d.py says what each one exercises) and of the MS-SSIM cases
LEVEL_SHAPES = ((2, 2, 13, 12, 21), (1, 2, 11, 11, 11), (1, 1, 5, 7, 40), (1, 1, 2, 30, 9), (1, 1, 12, 9, 40),
                (1, 3, 4, 40, 70), (1, 1, 25, 20, 37))
MS_SHAPES = ((1, 2, 12, 161, 161), (1, 1, 9, 162, 165))


def tag(shape):
    return 'x'.join(str(s) for s in shape)


def inputs(shape, seed):
    """X uniform in [0, 1), Y = clamp(X + 0.3 normal, 0, 1), float32 (NumPy PCG64: independent of torch's RNG stream)."""
    rng = np.random.default_rng([seed] + list(shape))
    x = rng.random(shape, dtype=np.float32)
    y = np.clip(x + np.float32(0.3) * rng.standard_normal(shape, dtype=np.float32), 0.0, 1.0).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


def upstream(shape, seed):
    """Random weights (N, C) for the two outputs of a level: the gradients are compared under them."""
    rng = np.random.default_rng([seed, 99] + list(shape))
    n, c = shape[0], shape[1]
    return (torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)))


SEED = 2024       # of every fixture case
STRIDE = 127      # gen_golden_ssim3d.py keeps every STRIDE-th gradient element of a case too large to store in full


def assert_grad_matches_fixture(z, key, got, tol, what=''):
    """``got`` against the reference's gradient ``key`` of ssim3d.npz, by the project's rule for this op: max error <=
    tol * max|ref| + 1e-7.  A case stored in full is compared element by element; a sampled case on the stored elements,
    and its sum and abs-sum within n times the per-element bound (what that bound implies for a sum of n elements)."""
    got = got.detach().cpu().double().reshape(-1).numpy()
    if key in z.files:
        ref = z[key].astype(np.float64)
        assert got.shape == ref.shape, (what, key, got.shape, ref.shape)
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(got - ref).max()
        assert err <= tol * scale + 1e-7, '%s %s: max err %.3e (scale %.3e)' % (what, key, err, scale)
        return err / scale
    ref, sums = z[key + '_sample'], z[key + '_sums']
    scale = max(np.abs(ref).max(), 1e-6)
    err = np.abs(got[::STRIDE] - ref).max()
    assert err <= tol * scale + 1e-7, '%s %s: max sampled err %.3e (scale %.3e)' % (what, key, err, scale)
    room = got.size * (tol * scale + 1e-7)
    assert abs(got.sum() - sums[0]) <= room and abs(np.abs(got).sum() - sums[1]) <= room, (what, key, 'sums')
    return err / scale


def taps(size=11, sigma=1.5, dtype=torch.float32):
    """The normalised Gaussian taps, computed in float32 as the reference does, then cast."""
    d = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(d ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).to(dtype)


def blur(v, g):
    """VALID depthwise window along each of the three spatial axes that is at least as long as the window."""
    k, ch = g.numel(), v.shape[1]
    for axis in range(3):
        if v.shape[2 + axis] < k:
            continue
        shape = [1, 1, 1, 1, 1]
        shape[2 + axis] = k
        v = F.conv3d(v, g.to(v.dtype).view(shape).expand(ch, -1, -1, -1, -1).contiguous(), groups=ch)
    return v


def level(x, y, g, C1=0.01 ** 2, C2=0.03 ** 2):
    """(ssim[N, C], cs[N, C]) of one scale."""
    mx, my = blur(x, g), blur(y, g)
    vx = blur(x * x, g) - mx * mx
    vy = blur(y * y, g) - my * my
    cxy = blur(x * y, g) - mx * my
    cs = (2 * cxy + C2) / (vx + vy + C2)
    s = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
    return s.flatten(2).mean(-1), cs.flatten(2).mean(-1)


def pool(v):
    return F.avg_pool3d(v, kernel_size=2, padding=[s % 2 for s in v.shape[2:]])


def ssim(x, y, g, data_range=1.0, K=(0.01, 0.03), nonnegative=False, size_average=True):
    s, _ = level(x, y, g, (K[0] * data_range) ** 2, (K[1] * data_range) ** 2)
    if nonnegative:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ms_ssim(x, y, g, data_range=1.0, K=(0.01, 0.03), weights=WEIGHTS, size_average=True):
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    val = None
    for i, wgt in enumerate(weights):
        wgt = float(np.float32(wgt))                  # the reference holds the weights in a FloatTensor
        s, cs = level(x, y, g, C1, C2)
        last = i == len(weights) - 1
        term = torch.relu(s if last else cs) ** wgt
        val = term if val is None else val * term
        if not last:
            x, y = pool(x), pool(y)
    return val.mean() if size_average else val.mean(1)
