"""Volumetric (N, C, T, H, W) SSIM / MS-SSIM on the fused HIP kernels of csrc/ssim3d.hip, against the fp64 yardstick
``tests/golden/ssim3d_truth.py`` (pinned to the reference by tests/test_ssim3d_cpu.py) and the reference's own results in
``tests/golden/ssim3d.npz``.

Bounds are the project's own for this op (test_gpu_ops.py::test_ssim_level_and_msssim, same ``assert_close`` rule): 2e-5 of
scale on values, 1e-4 on gradients, 1e-5 absolute on MS-SSIM scalars.  The reference in fp32 is within 2.1e-6 / 1.2e-5 of
its own fp64 run on these shapes, so the bounds leave a kernel five to ten times the reference's own rounding."""
import os
import warnings

import numpy as np
import pytest
import torch

import ssim3d_truth as T3

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssim3d.npz')
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _ops():
    from fcd_gan_pytorch_amd import _ops as ops
    return ops


def _pssim():
    from fcd_gan_pytorch_amd import ssim as pssim
    return pssim


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def assert_close(got, ref, tol=2e-5, what=''):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert err <= tol * scale + 1e-7, '%s: max err %.3e (scale %.3e)' % (what, err, scale)


_TRUTH = {}


def level_truth(shape):
    """fp64 truth of a level case, computed once per shape: (x, y, ws, wc, ssim, cs, dX, dY), all on the CPU."""
    if shape not in _TRUTH:
        x, y = T3.inputs(shape, T3.SEED)
        ws, wc = T3.upstream(shape, T3.SEED)
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        s, cs = T3.level(xr, yr, T3.taps(dtype=torch.float64), C1, C2)
        ((s * ws.double()).sum() + (cs * wc.double()).sum()).backward()
        _TRUTH[shape] = (x, y, ws, wc, s.detach(), cs.detach(), xr.grad, yr.grad)
    return _TRUTH[shape]


def run_level(x, y, ws, wc):
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    s, cs = _ops().ssim_level(xg, yg, T3.taps().cuda(), C1, C2)
    ((s * ws.cuda()).sum() + (cs * wc.cuda()).sum()).backward()
    return s.detach(), cs.detach(), xg.grad, yg.grad


# (2,2,13,12,21) all three axes smoothed, output 3x2x11 | (1,2,11,11,11) one output voxel | (1,1,5,7,40) T and H skipped |
# (1,1,2,30,9) T and W skipped | (1,1,12,9,40) only H skipped | (1,3,4,40,70) T skipped, several tiles with ragged edges in
# both plane axes | (1,1,25,20,37) depth walk longer than two windows, odd tile remainders
@pytest.mark.parametrize('shape', T3.LEVEL_SHAPES)
def test_level_matches_truth_and_reference(gold, shape):
    x, y, ws, wc, s_ref, cs_ref, dx_ref, dy_ref = level_truth(shape)
    s, cs, dx, dy = run_level(x, y, ws, wc)
    assert s.shape == (shape[0], shape[1]) and dx.shape == tuple(shape)
    assert_close(s, s_ref, tol=2e-5, what='ssim')
    assert_close(cs, cs_ref, tol=2e-5, what='cs')
    assert_close(dx, dx_ref, tol=1e-4, what='dX')
    assert_close(dy, dy_ref, tol=1e-4, what='dY')
    k = 'level/' + T3.tag(shape)
    assert_close(s, torch.from_numpy(gold[k + '/ssim']), tol=2e-5, what='ssim vs reference')
    assert_close(cs, torch.from_numpy(gold[k + '/cs']), tol=2e-5, what='cs vs reference')
    T3.assert_grad_matches_fixture(gold, k + '/dX', dx, 1e-4, 'dX vs reference')
    T3.assert_grad_matches_fixture(gold, k + '/dY', dy, 1e-4, 'dY vs reference')


@pytest.mark.parametrize('shape', [(2, 3, 4, 40, 52), (1, 2, 10, 13, 31)])
def test_unsmoothed_depth_is_the_mean_of_the_slices(shape):
    """T below the window: the volume's level is the existing rank-4 kernel on the T slices of a channel, averaged over T --
    values and gradients.  The two kernels form every voxel's ssim / cs with the same arithmetic, but the volume kernel sums
    all slices of a tile in one fp64 chain and rounds the mean to fp32 once, the rank-4 route rounds per slice and averages in
    fp32: not bit-identical, so the comparison uses the op's bounds (2e-5 / 1e-4)."""
    N, C, T, H, W = shape
    x, y = T3.inputs(shape, T3.SEED + 1)
    ws, wc = T3.upstream(shape, T3.SEED + 1)
    s, cs, dx, dy = run_level(x, y, ws, wc)
    xg = x.cuda().requires_grad_(True)
    yg = y.cuda().requires_grad_(True)
    s2, cs2 = _ops().ssim_level(xg.reshape(N, C * T, H, W), yg.reshape(N, C * T, H, W), T3.taps().cuda(), C1, C2)
    s2, cs2 = s2.view(N, C, T).mean(-1), cs2.view(N, C, T).mean(-1)
    ((s2 * ws.cuda()).sum() + (cs2 * wc.cuda()).sum()).backward()
    assert_close(s, s2.cpu(), tol=2e-5, what='ssim')
    assert_close(cs, cs2.cpu(), tol=2e-5, what='cs')
    assert_close(dx, xg.grad.cpu(), tol=1e-4, what='dX')
    assert_close(dy, yg.grad.cpu(), tol=1e-4, what='dY')


@pytest.mark.parametrize('shape', [(2, 3, 5, 7, 9), (1, 2, 4, 6, 8), (1, 1, 2, 3, 2)])
def test_avgpool3d2_pad_matches_stock_fp64(shape):
    """forward within 1 ulp of the fp64 result (the kernel sums the eight values in fp64 and rounds once), backward exact
    (dy / 8 is exact in both)."""
    rng = np.random.default_rng([7] + list(shape))
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    xr = x.double().requires_grad_(True)
    yr = T3.pool(xr)
    dy = torch.from_numpy(rng.standard_normal(tuple(yr.shape)).astype(np.float32))
    yr.backward(dy.double())
    xg = x.cuda().requires_grad_(True)
    yg = _ops().avgpool2_pad(xg)
    yg.backward(dy.cuda())
    assert yg.shape == yr.shape
    got, ref = yg.detach().cpu().numpy(), yr.detach().numpy()
    assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    assert torch.equal(xg.grad.cpu().double(), xr.grad)


def test_public_ssim_on_volumes(gold):
    pssim = _pssim()
    shape = T3.LEVEL_SHAPES[0]
    N, C = shape[0], shape[1]
    x, y, ws, wc, s_ref, cs_ref, dx_ref, dy_ref = level_truth(shape)
    # class, scalar, backward to both inputs
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    v = pssim.SSIM(data_range=1.0, channel=C, spatial_dims=3)(xg, yg)
    v.backward()
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    v_ref = T3.ssim(xr, yr, T3.taps(dtype=torch.float64))
    v_ref.backward()
    assert v.shape == () and abs(v.item() - v_ref.item()) <= 2e-5
    assert_close(xg.grad, xr.grad, tol=1e-4, what='dX')
    assert_close(yg.grad, yr.grad, tol=1e-4, what='dY')
    # size_average=False -> (N,); nonnegative_ssim off / on, on an anti-correlated pair (negative per-channel values)
    k = 'ssim/' + T3.tag(shape)
    xa = x.cuda()
    per = pssim.SSIM(data_range=1.0, channel=C, spatial_dims=3, size_average=False)(xa, 1 - xa)
    non = pssim.SSIM(data_range=1.0, channel=C, spatial_dims=3, size_average=False, nonnegative_ssim=True)(xa, 1 - xa)
    assert per.shape == (N,) and non.shape == (N,)
    assert_close(per, torch.from_numpy(gold[k + '/per']), tol=2e-5, what='per sample')
    assert_close(non, torch.from_numpy(gold[k + '/nonneg']), tol=2e-5, what='nonnegative')
    assert per.max().item() < 0 and (non == 0).all()
    # the functional form with the (1, 1, k) window
    f = pssim.ssim(xa, 1 - xa, data_range=1.0, size_average=False, win=pssim._fspecial_gauss_1d(11, 1.5))
    assert torch.equal(f, per)
    # a short dimension warns with the reference's text
    xs, ys = T3.inputs((1, 1, 5, 7, 40), T3.SEED)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        pssim.ssim(xs.cuda(), ys.cuda(), data_range=1.0)
    msgs = [str(r.message) for r in rec]
    assert any('Skipping Gaussian Smoothing at dimension 2+0' in m for m in msgs)
    assert any('Skipping Gaussian Smoothing at dimension 2+1' in m for m in msgs)
    assert not any('dimension 2+2' in m for m in msgs)


_MS = {}


def ms_truth(shape):
    if shape not in _MS:
        x, y = T3.inputs(shape, T3.SEED)
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        v = T3.ms_ssim(xr, yr, T3.taps(dtype=torch.float64))
        v.backward()
        _MS[shape] = (x, y, v.item(), xr.grad, yr.grad)
    return _MS[shape]


def run_ms(x, y, C):
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    v = _pssim().MS_SSIM(data_range=1.0, channel=C, spatial_dims=3)(xg, yg)
    v.backward()
    return v.detach(), xg.grad, yg.grad


# (1,2,12,161,161): the smallest legal plane, 161 -> 81 -> 41 -> 21 -> 11 (last level: one output pixel per slice); T is
# smoothed at level 0 only, then 6, 3, 2, 1 with odd padding at 3.  (1,1,9,162,165): the smallest legal T, even / odd planes.
@pytest.mark.parametrize('shape', T3.MS_SHAPES)
def test_ms_ssim_on_volumes(gold, shape):
    x, y, v_ref, dx_ref, dy_ref = ms_truth(shape)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        v, dx, dy = run_ms(x, y, shape[1])
    k = 'ms/' + T3.tag(shape)
    assert abs(v.item() - v_ref) <= 1e-5 and abs(v.item() - float(gold[k + '/val'])) <= 1e-5
    assert_close(dx, dx_ref, tol=1e-4, what='dX')
    assert_close(dy, dy_ref, tol=1e-4, what='dY')
    T3.assert_grad_matches_fixture(gold, k + '/dX', dx, 1e-4, 'dX vs reference')
    T3.assert_grad_matches_fixture(gold, k + '/dY', dy, 1e-4, 'dY vs reference')
    per = _pssim().ms_ssim(x.cuda(), y.cuda(), data_range=1.0, size_average=False)
    assert per.shape == (shape[0],) and np.abs(per.cpu().double().numpy() - gold[k + '/per']).max() <= 1e-5
    # every level whose T is below the window warns about dimension 2+0 (T = 12: levels 1-4; T = 9: all five)
    short = [str(r.message) for r in rec if 'Skipping Gaussian Smoothing at dimension 2+0' in str(r.message)]
    t, expect = shape[2], []
    for _ in range(5):
        if t < 11:
            expect.append('torch.Size([%d, %d, %d,' % (shape[0], shape[1], t))
        t = (t + 2 * (t % 2) - 2) // 2 + 1
    assert len(expect) >= 4
    for e in expect:
        assert any(e in m for m in short), (e, short)


def test_ms_ssim_refuses_t8_and_launches_nothing():
    pssim = _pssim()
    x = torch.rand(1, 1, 8, 170, 170, device='cuda')
    from fcd_gan_pytorch_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_read(reset=True)
    _lib.lib.fcd_prof_enable(1)
    try:
        with pytest.raises(RuntimeError, match='smaller than kernel size'):
            pssim.ms_ssim(x, x, data_range=1.0)
        with pytest.raises(RuntimeError, match='smaller than kernel size'):
            pssim.MS_SSIM(data_range=1.0, channel=1, spatial_dims=3)(x, x)
        torch.cuda.synchronize()
        launches = sum(f['launches'] for f in _lib.prof_read(reset=True).values())
        pssim.ssim(x[:, :, :, :12, :12], x[:, :, :, :12, :12], data_range=1.0)      # (the counter does see a launch)
        counted = sum(f['launches'] for f in _lib.prof_read(reset=True).values())
    finally:
        _lib.lib.fcd_prof_enable(0)
    assert launches == 0 and counted == 1


def test_volume_ms_ssim_is_reproducible_bit_for_bit():
    shape = T3.MS_SHAPES[0]
    x, y = T3.inputs(shape, T3.SEED)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = run_ms(x, y, shape[1])
        b = run_ms(x, y, shape[1])
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_rank4_results_do_not_depend_on_rank5_calls():
    """No shared state: rank-4 ssim / ms_ssim (one shape of test_ssim_level_and_msssim) are bit-identical before and after a
    rank-5 call."""
    pssim = _pssim()
    rng = np.random.default_rng(71)
    x = torch.from_numpy(rng.random((1, 2, 200, 184), dtype=np.float32)).cuda()
    y = (x + 0.3 * torch.from_numpy(rng.standard_normal((1, 2, 200, 184)).astype(np.float32)).cuda()).clamp(0, 1)

    def rank4():
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        s = pssim.ssim(xg, yg, data_range=1.0)
        m = pssim.ms_ssim(xg, yg, data_range=1.0)
        (s + m).backward()
        return s.detach(), m.detach(), xg.grad, yg.grad
    before = rank4()
    xv, yv = T3.inputs(T3.LEVEL_SHAPES[0], T3.SEED)
    run_level(xv, yv, *T3.upstream(T3.LEVEL_SHAPES[0], T3.SEED))
    xm, ym = T3.inputs(T3.MS_SHAPES[1], T3.SEED)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        run_ms(xm, ym, 1)
    after = rank4()
    for p, q in zip(before, after):
        assert torch.equal(p, q)
