"""Volumetric (N, C, T, H, W) SSIM / MS-SSIM, the part that needs no GPU:
 * the yardstick ``tests/golden/ssim3d_truth.py`` against the reference's own results (``tests/golden/ssim3d.npz``), in fp64
   (it states the same function: agreement to fp64 rounding; the fixture keeps full gradients in float32, hence 1e-6 there)
   and in fp32 (inside the project's bounds for this op: 2e-5 of scale on values, 1e-4 on gradients, 1e-5 absolute on the
   MS-SSIM scalar);
 * the C entry points' argument validation (nothing is launched);
 * the public surface's rank / device / pooling errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ssim3d_truth as T3

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssim3d.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _close(got, ref, tol):
    got, ref = np.asarray(got.detach().double()), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    scale = max(np.abs(ref).max(), 1e-6)
    assert np.abs(got - ref).max() <= tol * scale + 1e-7, (np.abs(got - ref).max(), scale)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('shape', T3.LEVEL_SHAPES)
def test_truth_level_matches_reference(gold, shape, dtype):
    vtol, gtol = (1e-10, 1e-6) if dtype == torch.float64 else (2e-5, 1e-4)
    x, y = T3.inputs(shape, T3.SEED)
    x, y = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    s, cs = T3.level(x, y, T3.taps(dtype=dtype))
    ws, wc = T3.upstream(shape, T3.SEED)
    ((s * ws.to(dtype)).sum() + (cs * wc.to(dtype)).sum()).backward()
    k = 'level/' + T3.tag(shape)
    _close(s, gold[k + '/ssim'], vtol)
    _close(cs, gold[k + '/cs'], vtol)
    T3.assert_grad_matches_fixture(gold, k + '/dX', x.grad, gtol, 'truth')
    T3.assert_grad_matches_fixture(gold, k + '/dY', y.grad, gtol, 'truth')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_truth_public_ssim_matches_reference(gold, dtype):
    shape = T3.LEVEL_SHAPES[0]
    x, _ = T3.inputs(shape, T3.SEED)
    x = x.to(dtype)
    k = 'ssim/' + T3.tag(shape)
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    assert gold[k + '/per'].min() < 0 and gold[k + '/nonneg'].min() >= 0      # the pair is anti-correlated: relu matters
    _close(T3.ssim(x, 1 - x, T3.taps(dtype=dtype), size_average=False), gold[k + '/per'], tol)
    _close(T3.ssim(x, 1 - x, T3.taps(dtype=dtype), size_average=False, nonnegative=True), gold[k + '/nonneg'], tol)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('shape', T3.MS_SHAPES)
def test_truth_ms_ssim_matches_reference(gold, shape, dtype):
    vtol, gtol = (1e-10, 1e-9) if dtype == torch.float64 else (1e-5, 1e-4)
    x, y = T3.inputs(shape, T3.SEED)
    x, y = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    g = T3.taps(dtype=dtype)
    v = T3.ms_ssim(x, y, g)
    v.backward()
    k = 'ms/' + T3.tag(shape)
    assert abs(v.item() - float(gold[k + '/val'])) <= vtol
    assert np.abs(T3.ms_ssim(x.detach(), y.detach(), g, size_average=False).double().numpy() - gold[k + '/per']).max() <= vtol
    T3.assert_grad_matches_fixture(gold, k + '/dX', x.grad, gtol, 'truth ms')
    T3.assert_grad_matches_fixture(gold, k + '/dY', y.grad, gtol, 'truth ms')


def test_truth_refuses_to_pool_an_extent_of_one():
    """What the product has to reproduce: stock avg_pool3d raises for T = 8 and T = 3 (a pooled level reaches T = 1) and runs
    for T = 9."""
    g = T3.taps()
    for t in (8, 3):
        with pytest.raises(RuntimeError):
            T3.ms_ssim(torch.zeros(1, 1, t, 161, 161), torch.zeros(1, 1, t, 161, 161), g)
    assert T3.ms_ssim(torch.zeros(1, 1, 9, 161, 161), torch.zeros(1, 1, 9, 161, 161), g).item() == pytest.approx(1.0)


# ------------------------------------------------------------------------------------------------------------- C ABI
def _lib():
    from fcd_gan_pytorch_amd import _lib
    return _lib


def test_ws_bytes_formula():
    """max(forward: one fp64 {ssim, cs} pair per (n,c) and 16 x 32 plane tile; backward: four fp32 maps of the input volume)"""
    lib = _lib().lib
    for NC, T, H, W in ((3, 5, 20, 40), (8, 16, 256, 256), (2, 1, 1, 1)):
        fwd = 16 * NC * ((H + 15) // 16) * ((W + 31) // 32)
        bwd = 16 * NC * T * H * W
        assert lib.fcd_ssim3d_ws_bytes(NC, T, H, W) == max(fwd, bwd)
    assert lib.fcd_ssim3d_ws_bytes(0, 4, 4, 4) == 0 and lib.fcd_ssim3d_ws_bytes(1, 4, 0, 4) == 0


def test_level_entries_validate_before_any_launch():
    L = _lib()
    lib, p = L.lib, ctypes.c_void_p(4096)      # never dereferenced: every call below returns before a launch
    C1, C2 = 1e-4, 9e-4
    rc = lib.fcd_ssim3d_level_fwd(None, p, p, 11, p, 2, 12, 12, 12, C1, C2, p, 1 << 20, None)
    assert rc == -1 and b'fcd_ssim3d_level_fwd' in lib.fcd_last_error_string()
    rc = lib.fcd_ssim3d_level_bwd(p, p, p, 11, p, None, p, p, 2, 12, 12, 12, C1, C2, p, 1 << 20, None)
    assert rc == -1 and b'fcd_ssim3d_level_bwd' in lib.fcd_last_error_string()
    for win in (12, 13):                        # even; longer than 11 taps
        rc = lib.fcd_ssim3d_level_fwd(p, p, p, win, p, 2, 20, 20, 20, C1, C2, p, 1 << 20, None)
        assert rc == -1 and b'window %d' % win in lib.fcd_last_error_string()
        rc = lib.fcd_ssim3d_level_bwd(p, p, p, win, p, p, p, p, 2, 20, 20, 20, C1, C2, p, 1 << 20, None)
        assert rc == -1 and b'window %d' % win in lib.fcd_last_error_string()
    rc = lib.fcd_ssim3d_level_fwd(p, p, p, 11, p, 2, 0, 20, 20, C1, C2, p, 1 << 20, None)
    assert rc == -1
    # one byte short: forward needs its partials (16 B per (n,c) and tile of the OUTPUT plane), backward the four maps
    NC, T, H, W = 2, 13, 40, 70                 # output 3 x 30 x 60 -> 2 x 2 tiles
    need_f = 16 * NC * 2 * 2
    assert lib.fcd_ssim3d_level_fwd(p, p, p, 11, p, NC, T, H, W, C1, C2, p, need_f - 1, None) == -3
    assert b'workspace' in lib.fcd_last_error_string()
    need_b = 16 * NC * 3 * 30 * 60
    assert lib.fcd_ssim3d_level_bwd(p, p, p, 11, p, p, p, p, NC, T, H, W, C1, C2, p, need_b - 1, None) == -3
    assert lib.fcd_ssim3d_level_bwd(p, p, p, 11, p, p, p, p, NC, T, H, W, C1, C2, None, 1 << 30, None) == -3
    assert need_b <= lib.fcd_ssim3d_ws_bytes(NC, T, H, W)


def test_pool_entries_refuse_an_extent_below_two():
    lib, p = _lib().lib, ctypes.c_void_p(4096)
    for fn in (lib.fcd_avgpool3d2_pad_fwd, lib.fcd_avgpool3d2_pad_bwd):
        for T, H, W in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
            assert fn(p, p, 2, T, H, W, None) == -1
            assert b'smaller than' in lib.fcd_last_error_string()
        assert fn(None, p, 2, 8, 8, 8, None) == -1 and fn(p, p, 0, 8, 8, 8, None) == -1


# ---------------------------------------------------------------------------------------------------- public surface
@pytest.mark.parametrize('shape', [(4, 12, 12), (1, 1, 2, 2, 12, 12)])
def test_other_ranks_raise_the_reference_error(shape):
    from fcd_gan_pytorch_amd import ssim as pssim
    x = torch.rand(shape)
    for fn in (pssim.ssim, pssim.ms_ssim):
        with pytest.raises(ValueError, match='4-d or 5-d'):
            fn(x, x, data_range=1.0)
    with pytest.raises(ValueError, match='4-d or 5-d'):
        pssim.SSIM(data_range=1.0, channel=1, spatial_dims=3)(x, x)


def test_rank5_cpu_tensors_reach_the_hip_path_and_are_rejected_there():
    """No CPU fallback: a rank-5 CPU tensor passes the shape checks and is refused by the op layer."""
    L = _lib()
    from fcd_gan_pytorch_amd import ssim as pssim
    x = torch.rand(1, 2, 12, 12, 12)
    with pytest.raises(L.FcdError):
        pssim.ssim(x, x, data_range=1.0)
    with pytest.raises(L.FcdError):
        pssim.SSIM(data_range=1.0, channel=2, spatial_dims=3)(x, x)
    big = torch.zeros(1, 1, 9, 161, 161)
    with pytest.raises(L.FcdError):
        pssim.ms_ssim(big, big, data_range=1.0)
    with pytest.raises(L.FcdError):
        pssim.MS_SSIM(data_range=1.0, channel=1, spatial_dims=3)(big, big)
    # (N, C, 1, H, W) is squeezed to the 2-D case, as in the reference -- and refused all the same
    with pytest.raises(L.FcdError):
        pssim.ssim(x[:, :, :1], x[:, :, :1], data_range=1.0)


def test_ms_ssim_refuses_a_depth_the_pool_cannot_halve():
    L = _lib()
    from fcd_gan_pytorch_amd import ssim as pssim
    for t in (8, 3):
        x = torch.zeros(1, 1, t, 170, 170)
        with pytest.raises(RuntimeError, match='smaller than kernel size') as e:
            pssim.ms_ssim(x, x, data_range=1.0)
        assert not isinstance(e.value, L.FcdError)      # raised by the shape walk, before the op layer sees the tensors
    with pytest.raises(AssertionError):                 # the reference's assert still looks at min(H, W) only
        pssim.ms_ssim(torch.zeros(1, 1, 12, 160, 200), torch.zeros(1, 1, 12, 160, 200), data_range=1.0)
    from fcd_gan_pytorch_amd import _ops as ops
    with pytest.raises(RuntimeError, match='smaller than kernel size'):
        ops.avgpool2_pad(torch.zeros(1, 1, 1, 8, 8))
