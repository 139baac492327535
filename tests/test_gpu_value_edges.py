"""The HBM-bound kernels (BatchNorm family, activations, max-pool family, sigmoid head, masked loss sums, optimizers, SSIM,
tile normalisation) on the INPUTS at which each of them decides something: channel offsets far above the standard deviation,
constant and all-zero channels, +-0 / denormals / non-finite values at the activation kink, tied and non-finite pooling
windows, saturated logits, binary masks with empty samples, flat and identical images, and one case just past every
launcher's grid cap.  test_gpu_ops.py draws its inputs from N(0, 1), which reaches none of these.

Every check compares the HIP op with a plain reference computed on the CPU inside the test: fp64 torch ("truth") and, where
a bound is needed, the same composition in fp32 ("stock").  Checks that are not exact use one rule (``assert_rule``), per
compared tensor, per channel where the op works per channel:

    err(kernel vs truth) <= max(B, 4 x err(stock vs truth))

B is the project's existing bound for the op (test_gpu_ops.py: 2e-5 * scale on values, 5e-5 * scale on BatchNorm gradients,
6e-5 * scale behind the F(4x4) transforms, 2e-5 / 1e-4 on SSIM values / gradients, 1e-6 on optimizer states); the factor 4
leaves room for another, equally valid, rounding sequence.  Nothing is excluded where a result depends on a gate (ReLU sign,
pooling argmax): the inputs are built so that the fp64 truth stays at least ``MARGIN`` away from every gate, and that is
asserted on the truth before anything runs on the GPU.

Measured on MI355X (largest kernel error / stock error over the channels whose kernel error exceeds B; ``-`` = every
channel within B):

    check                                                        kernel/stock
    -----------------------------------------------------------  ------------
    bn_act y, channels with |mean| / std >= 30 (16 cases)         1.47
    bn_act dgamma, the same channels                              1.00
    bn_act dslope (PReLU, 2 sample groups)                        0.86
    bn_act dx, dbeta, running_mean, running_var                   -
    bn_act (2, 2, 520, 520), all tensors                          -
    bn_relu_pool_skip, bn_relu_head, bn_relu_conv3x3,
      conv2d(bn_groups) -> bn_act under offsets, all tensors      -
    bn_relu_head with saturated logits, all tensors               -
    adam / rmsprop, 20 steps (24 cases)                           -
    ssim rank 4: constants ssim 2.78, cs 2.77, dX 2.20; offset 100 ssim 1.40, cs 1.40, dX 1.08, dY 1.10
    ssim rank 5: constants cs 0.43, dX 0.94, dY 0.61; offset 100 cs 0.37, dX 0.72, dY 0.70
    ssim identical images, gradient (absolute)                    0.52  (zeros against zeros: 0 on both sides)

The offset channels are where the rule is needed at all: the mean is stored in fp32 on both sides, so at |mean| = 1e4 one ulp
of it (1e-3) goes into every xhat of the channel; kernel and stock make the same error there (ratio 1.00 on dgamma).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOMENTUM = 0.1
MARGIN = 1e-2          # distance the truth keeps from every gate: a decade above the ~1e-3 * gamma that one fp32 ulp of the mean
#                        costs, on either side, in a channel with |mean| = 1e4 (the integer-valued pooling inputs assert 1e-3)
FLT_MIN = float(np.finfo(np.float32).tiny)
ACTS = ('none', 'relu', 'leaky', 'prelu')


def _ops():
    from fcd_gan_pytorch_amd import _ops as ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    rng = np.random.default_rng([seed, len(shape)] + list(shape))
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def assert_close(got, ref, tol=2e-5, what=''):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert err <= tol * scale + 1e-7, '%s: max err %.3e (scale %.3e)' % (what, err, scale)


def assert_rule(got, truth, stock, tol, what, channel_dim=None, floor=1e-7, tensor_scale=False):
    """err(got vs truth) <= max(tol * scale + floor, 4 * err(stock vs truth)), per tensor or per index of ``channel_dim``
    (scale = largest |truth| of that tensor / channel; ``tensor_scale``: of the whole tensor although the errors are taken
    per channel -- for one-number-per-channel sums with cancellation, dgamma and dbeta, whose error does not shrink with a
    sum that happens to come out small: the scale test_gpu_ops.py uses for them).  Prints the figures before asserting."""
    got, truth, stock = got.detach().cpu().double(), truth.detach().cpu().double(), stock.detach().cpu().double()
    assert got.shape == truth.shape == stock.shape, (what, got.shape, truth.shape, stock.shape)
    assert torch.isfinite(truth).all() and torch.isfinite(stock).all(), what + ': reference is not finite'
    assert torch.isfinite(got).all(), what + ': kernel result is not finite'

    def rows(t):
        if channel_dim is None:
            return t.reshape(1, -1)
        return t.movedim(channel_dim, 0).reshape(t.shape[channel_dim], -1)
    ek, es = (rows(got) - rows(truth)).abs().amax(1), (rows(stock) - rows(truth)).abs().amax(1)
    scale = truth.abs().max().expand(ek.shape) if tensor_scale else rows(truth).abs().amax(1)
    base = tol * scale.clamp_min(1e-6) + floor
    over = ek > base                                   # the channels on which the ratio is taken
    assert bool((es[over] > 0).all()), what + ': stock error is zero where the kernel exceeds B'
    worst = (ek[over] / es[over]).max().item() if over.any() else float('nan')
    print('RULE %-58s kernel %.3e  stock %.3e  B %.3e  kernel/stock over B: %s' %
          (what, ek.max().item(), es.max().item(), base.min().item(), ('%.2f' % worst) if over.any() else '-'))
    bad = ek > torch.maximum(base, 4 * es)
    assert not bad.any(), '%s: rows %s: kernel err %s, stock err %s, B %s' % (
        what, bad.nonzero().flatten().tolist(), ek[bad].tolist(), es[bad].tolist(), base[bad].tolist())


def same_with_nans(got, ref):
    """``got == ref`` everywhere, NaNs in the same places (the sign of a zero is not looked at)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    return got.shape == ref.shape and torch.equal(torch.isnan(got), torch.isnan(ref)) and bool(((got == ref) | torch.isnan(ref)).all())


def run_ref(fn, leaves, buffers, dtype):
    """``fn(L, B) -> (outputs dict, loss)`` on CPU copies of ``leaves`` (differentiated) and ``buffers`` (updated in place) in
    ``dtype``; returns outputs, ``d<leaf>`` gradients and the buffers in one dict."""
    L = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in leaves.items()}
    B = {k: v.detach().cpu().to(dtype).clone() for k, v in buffers.items()}
    outs, loss = fn(L, B)
    loss.backward()
    res = {k: v.detach() for k, v in outs.items()}
    res.update({'d' + k: v.grad for k, v in L.items() if v.grad is not None})
    res.update(B)
    return res


def truth_and_stock(fn, leaves, buffers):
    return run_ref(fn, leaves, buffers, torch.float64), run_ref(fn, leaves, buffers, torch.float32)


def bn_train(x, L, B, groups):
    """torch's train-mode BatchNorm, once per sample group in order (the reference calls the layer once per group)."""
    Ng = x.shape[0] // groups
    return torch.cat([F.batch_norm(x[i * Ng:(i + 1) * Ng], B['running_mean'], B['running_var'], L['gamma'], L['beta'], True,
                                   MOMENTUM, EPS) for i in range(groups)])


def actf(t, act, slope=None):
    if act == 'relu':
        return F.relu(t)
    if act == 'leaky':
        return F.leaky_relu(t, 0.2)
    if act == 'prelu':
        return F.prelu(t, slope)
    return t


def act_code(ops, act):
    return {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'leaky': ops.ACT_LEAKY, 'prelu': ops.ACT_PRELU}[act]


def bn_params(C, seed):
    return dict(gamma=1 + 0.1 * rnd(C, seed=seed), beta=0.1 * rnd(C, seed=seed + 1)), \
        dict(running_mean=0.1 * rnd(C, seed=seed + 2), running_var=1 + 0.2 * torch.tanh(rnd(C, seed=seed + 3)))


def gpu_bn(P, B, train=True):
    bn = torch.nn.BatchNorm2d(P['gamma'].numel(), eps=EPS, momentum=MOMENTUM).cuda()
    with torch.no_grad():
        bn.weight.copy_(P['gamma']); bn.bias.copy_(P['beta'])
        bn.running_mean.copy_(B['running_mean']); bn.running_var.copy_(B['running_var'])
    bn.train(train)
    return bn


def bn_pre64(x, gamma, beta, groups):
    """fp64 pre-activation gamma * xhat + beta of a train-mode BatchNorm with per-group batch statistics."""
    xd, Ng = x.double(), x.shape[0] // groups
    out = []
    for i in range(groups):
        xi = xd[i * Ng:(i + 1) * Ng]
        m, v = xi.mean((0, 2, 3), keepdim=True), xi.var((0, 2, 3), unbiased=False, keepdim=True)
        out.append((xi - m) / torch.sqrt(v + EPS) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
    return torch.cat(out)


def windows(t):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the 2 x 2 pooling windows in ATen's scan order."""
    N, C, H, W = t.shape
    return t.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def unwindows(w):
    N, C, H2, W2, _ = w.shape
    return w.reshape(N, C, H2, W2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * H2, 2 * W2)


def gate_margins(x, gamma, beta, groups, pool):
    """(distance of the BatchNorm pre-activation from the ReLU kink, smallest lead of a positive window maximum over the
    runner-up) of the fp64 truth."""
    p = bn_pre64(x, gamma, beta, groups)
    lead = float('inf')
    if pool:
        top = windows(F.relu(p)).topk(2, -1).values
        live = (top[..., 0] > 0) & (top[..., 0] > top[..., 1])      # an exact tie (equal inputs, or a window that is 0 everywhere) is
        #                                                              settled by position, the first wins on both sides: no gate
        if live.any():
            lead = (top[..., 0] - top[..., 1])[live].min().item()
    return p.abs().min().item(), lead


def off_the_gates(x, gamma, beta, groups, pool=False, margin=MARGIN):
    """Nudge the few elements of ``x`` whose fp64 BatchNorm pre-activation lies within ``margin`` of 0 (and, with ``pool``, the
    window maxima that lead the runner-up by less than ``margin``) away from the gate.  The statistics move by ~1e-6 per
    round; a handful of rounds settles.  The caller asserts the result with :func:`gate_margins`."""
    x = x.clone()
    step = (4 * margin / gamma.abs()).view(1, -1, 1, 1)        # std of the random channels is ~1: moves the pre-activation by ~4 margins
    for _ in range(20):
        p = bn_pre64(x, gamma, beta, groups)
        bump = torch.where(p.abs() < margin, torch.where(p >= 0, 1.0, -1.0), 0.0).to(p.dtype)
        if pool:
            w = windows(F.relu(p))
            top = w.topk(2, -1).values
            near = (top[..., 0] > top[..., 1]) & (top[..., 0] - top[..., 1] < margin)
            lift = torch.zeros_like(w).scatter_(-1, w.argmax(-1, keepdim=True), near.unsqueeze(-1).to(w.dtype))
            bump = bump + unwindows(lift) * (bump == 0)
        if not bump.any():
            break
        x = (x.double() + bump * step.double()).float()
    return x


# ================================================================================================ 1. BatchNorm family
MEANS = [0.0, 1.0, 10.0, 30.0, 100.0, 1e3, 1e4, -1e3]      # channels 0 - 7; 8: the constant 3.25; 9: zeros


def offset_case(shape, groups, act, seed):
    """Input, parameters and upstream gradient of one bn_act case; with an activation, conditioned off the kink."""
    C = shape[1]
    assert C == 10
    x = rnd(*shape, seed=seed)
    for c, m in enumerate(MEANS):
        x[:, c] += m
    x[:, 8] = 3.25
    x[:, 9] = 0.0
    P, B = bn_params(C, seed + 1)
    P['beta'][8], P['beta'][9] = 0.5, -0.5
    if act != 'none':
        x = off_the_gates(x, P['gamma'], P['beta'], groups)
    return x, P, B, rnd(*shape, seed=seed + 7)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape,groups', [((4, 10, 12, 20), 1), ((4, 10, 12, 20), 2), ((4, 10, 9, 7), 1), ((4, 10, 9, 7), 2)],
                         ids=['f4-g1', 'f4-g2', 'scalar-g1', 'scalar-g2'])
def test_bn_act_under_channel_offsets_and_degenerate_channels(shape, groups, act):
    """Train-mode ``bn_act`` with |mean| / std from 0 to 1e4, a constant channel (variance exactly 0) and an all-zero channel:
    y, dx, dgamma, dbeta and both running statistics against the fp64 ATen composition, per channel.  var = E[x^2] - mean^2
    loses log10(mean^2 / var) digits: an fp32 accumulator, a dropped clamp or a wrong count is catastrophic at 1e4."""
    ops = _ops()
    x, P, B, g = offset_case(shape, groups, act, seed=211)
    slope = torch.tensor([0.25])
    if act != 'none':
        kink, _ = gate_margins(x, P['gamma'], P['beta'], groups, pool=False)
        assert kink >= MARGIN, kink
    stds = x[:, :8].double().std((0, 2, 3))
    assert abs(x[:, 6].double().mean().item()) / stds[6].item() > 5e3          # the ratio the case is about

    def fn(L, Bf):
        y = actf(bn_train(L['x'], L, Bf, groups), act, L['slope'])
        return dict(y=y), (y * g.to(y.dtype)).sum() + 0.0 * L['slope'].sum()
    leaves = dict(x=x, slope=slope, **P)
    T, S = truth_and_stock(fn, leaves, B)

    bn = gpu_bn(P, B)
    xg = x.cuda().requires_grad_(True)
    sg = slope.cuda().requires_grad_(True)
    y = ops.bn_act(xg, bn, act_code(ops, act), slope=sg if act == 'prelu' else None, slope_imm=0.2, groups=groups)
    y.backward(g.cuda())
    tag = 'bn_act[%s,%s,g%d] ' % ('f4' if shape[2] * shape[3] % 4 == 0 else 'scalar', act, groups)
    # (y of the two degenerate channels has its own bound below: stock computes (x - mean) = 0 and returns beta exactly)
    assert_rule(y[:, :8], T['y'][:, :8], S['y'][:, :8], 2e-5, tag + 'y', channel_dim=1)
    assert_rule(xg.grad, T['dx'], S['dx'], 5e-5, tag + 'dx', channel_dim=1)
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)
    if act == 'prelu':
        assert_rule(sg.grad, T['dslope'], S['dslope'], 5e-5, tag + 'dslope')
    assert int(bn.num_batches_tracked) == groups

    # the constant and the all-zero channel: x - mean is exactly 0, the variance is exactly 0
    yk, dg, rv = y.detach().cpu(), bn.weight.grad.cpu(), bn.running_var.cpu()
    decay = np.float32(1) - np.float32(MOMENTUM)
    for c, v in ((8, 3.25), (9, 0.0)):
        assert dg[c].item() == 0.0, ('dgamma', c, dg[c].item())
        want_rv = np.float32(B['running_var'][c].item())
        for _ in range(groups):
            want_rv = decay * want_rv + np.float32(MOMENTUM) * np.float32(0)         # an unbiased variance of exactly 0
        assert rv[c].item() == float(want_rv), ('running_var', c, rv[c].item(), float(want_rv))
        want = actf(P['beta'][c].view(1), act, slope).double().item()           # the activation of exactly beta, in fp32
        bound = 2.0 ** -22 * abs(v * P['gamma'][c].item()) / EPS ** 0.5               # rounding of shift = beta - mean * scale
        assert (yk[:, c].double() - want).abs().max().item() <= bound, (c, (yk[:, c].double() - want).abs().max().item(), bound)


def test_constant_channels_never_get_a_negative_variance():
    """Constants with a full 24-bit mantissa, 4 x 391 values per channel: 391 x^2 needs 57 bits, so sum x^2 is rounded in fp64
    and E[x^2] - mean^2 comes out as +-1e-16 * x^2 instead of 0, negative on about one channel in ten.  The variance is
    clamped at 0: the running variance (started at 0) is never negative and stays within the rounding of the fp64 sums (at
    most 32 roundings of 2^-53 on the way from x^2 to the variance: 7 adds per thread, 6 + 4 in the block reduction, the
    division, the product, the difference), dgamma is exactly 0 and y is act(beta) within the rounding of the shift term."""
    ops = _ops()
    N, C, H, W = 4, 64, 17, 23
    rng = np.random.default_rng(265)
    consts = (rng.uniform(1.0, 2.0, C) * 10.0 ** rng.uniform(-2, 6.4, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    consts[:4] = [5000001.0, -4194303.5, 1234.5677, 0.1]
    x = torch.from_numpy(consts).view(1, C, 1, 1).expand(N, C, H, W).contiguous()
    assert x.abs().max().item() < 2 ** 24 and bool((x.double().var((0, 2, 3)) == 0).all())
    g = rnd(N, C, H, W, seed=266)
    for groups in (1, 2):
        P, B = bn_params(C, 267)
        B['running_var'].zero_()
        B['running_mean'].zero_()
        bn = gpu_bn(P, B)
        xg = x.cuda().requires_grad_(True)
        y = ops.bn_act(xg, bn, ops.ACT_NONE, groups=groups)
        y.backward(g.cuda())
        rv = bn.running_var.cpu().double()
        assert bool((rv >= 0).all()), rv[rv < 0]
        assert bool((rv <= groups * MOMENTUM * 32 * 2.0 ** -53 * x[0, :, 0, 0].double() ** 2 * 1.001).all())
        assert bool((bn.weight.grad.cpu() == 0).all())
        assert torch.isfinite(y).all() and torch.isfinite(xg.grad).all()
        bound = 2.0 ** -22 * (x[0, :, 0, 0].double() * P['gamma'].double()).abs() / EPS ** 0.5
        err = (y.detach().cpu().double() - P['beta'].double().view(1, C, 1, 1)).abs().amax((0, 2, 3))
        assert bool((err <= bound).all()), (err / bound).max().item()
        ref = torch.zeros(C, dtype=torch.float64)           # the mean is the constant itself: momentum * c onto (1 - momentum) * previous
        for _ in range(groups):
            ref = 0.9 * ref + 0.1 * torch.from_numpy(consts).double()
        assert bool(((bn.running_mean.cpu().double() - ref).abs() <= 2e-6 * ref.abs()).all())      # a few fp32 roundings


def consumer_offsets(C):
    """Half the channels offset by 100, one by 1e3, the rest by 0."""
    off = torch.zeros(C)
    off[: C // 2] = 100.0
    off[C // 2] = 1e3
    return off


@pytest.mark.parametrize('case', [(4, 16, 16, 24, 2), (6, 8, 10, 12, 3)], ids=lambda c: 'x'.join(map(str, c)))
def test_bn_relu_pool_skip_under_channel_offsets(case):
    """``bn_relu_pool_skip`` (statistics, ReLU, 2 x 2 max-pool and both gradients from z alone) against the fp64 composition
    batch_norm -> relu -> {skip, max_pool2d}, on channels offset by 100 and 1e3, with the ReLU kink and the pooling argmax
    of the truth kept ``MARGIN`` away from a decision."""
    ops = _ops()
    N, C, H, W, G = case
    P, B = bn_params(C, 221)
    z = off_the_gates(rnd(N, C, H, W, seed=220) + consumer_offsets(C).view(1, -1, 1, 1), P['gamma'], P['beta'], G, pool=True)
    kink, lead = gate_margins(z, P['gamma'], P['beta'], G, pool=True)
    assert kink >= MARGIN and lead >= MARGIN, (kink, lead)
    gs, gp = rnd(N, C, H, W, seed=225), rnd(N, C, H // 2, W // 2, seed=226)

    def fn(L, Bf):
        a = F.relu(bn_train(L['z'], L, Bf, G))
        p = F.max_pool2d(a, 2)
        return dict(a=a, p=p), (a * gs.to(a.dtype)).sum() + (p * gp.to(a.dtype)).sum()
    T, S = truth_and_stock(fn, dict(z=z, **P), B)
    bn = gpu_bn(P, B)
    zin = z.cuda().requires_grad_(True)
    zz = zin * 1.0
    assert ops.bn_relu_pool_skip_ok(zz, bn, G)
    a, p = ops.bn_relu_pool_skip(zz, bn, groups=G)
    ((a * gs.cuda()).sum() + (p * gp.cuda()).sum()).backward()
    tag = 'bn_relu_pool_skip[%s] ' % 'x'.join(map(str, case))
    assert_rule(a, T['a'], S['a'], 2e-5, tag + 'a', channel_dim=1)
    assert_rule(p, T['p'], S['p'], 2e-5, tag + 'pooled', channel_dim=1)
    assert_rule(zin.grad, T['dz'], S['dz'], 5e-5, tag + 'dz', channel_dim=1)
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)


@pytest.mark.parametrize('case', [(4, 32, 32, 32, 2), (3, 21, 32, 36, 1)], ids=lambda c: 'x'.join(map(str, c)))
def test_bn_relu_head_under_channel_offsets(case):
    """``bn_relu_head`` against sigmoid(conv2d(relu(batch_norm(z)))) in fp64 with offset channels."""
    ops = _ops()
    N, C, H, W, G = case
    P, B = bn_params(C, 231)
    z = off_the_gates(rnd(N, C, H, W, seed=230) + consumer_offsets(C).view(1, -1, 1, 1), P['gamma'], P['beta'], G)
    assert gate_margins(z, P['gamma'], P['beta'], G, pool=False)[0] >= MARGIN
    w, b, g = rnd(1, C, 1, 1, seed=232, scale=C ** -0.5), rnd(1, seed=233, scale=0.1), rnd(N, 1, H, W, seed=234)

    def fn(L, Bf):
        y = torch.sigmoid(F.conv2d(F.relu(bn_train(L['z'], L, Bf, G)), L['w'], L['b']))
        return dict(y=y), (y * g.to(y.dtype)).sum()
    T, S = truth_and_stock(fn, dict(z=z, w=w, b=b, **P), B)
    bn = gpu_bn(P, B)
    zin, wg, bg = (t.cuda().requires_grad_(True) for t in (z, w, b))
    zz = zin * 1.0
    assert ops.bn_relu_head_ok(zz, bn, wg, G)
    y = ops.bn_relu_head(zz, bn, wg, bg, sigmoid=True, groups=G)
    y.backward(g.cuda())
    tag = 'bn_relu_head[%s] ' % 'x'.join(map(str, case))
    assert_rule(y, T['y'], S['y'], 2e-5, tag + 'y')
    assert_rule(zin.grad, T['dz'], S['dz'], 5e-5, tag + 'dz', channel_dim=1)
    assert_rule(wg.grad, T['dw'], S['dw'], 2e-5, tag + 'dw')
    assert_rule(bg.grad, T['db'], S['db'], 2e-5, tag + 'db')
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)


def test_bn_relu_conv3x3_under_channel_offsets():
    """``bn_relu_conv3x3`` (BatchNorm + ReLU applied by the F(4x4) input transform of the next convolution) against
    conv2d(relu(batch_norm(z))) in fp64 with offset channels.  What passes through the F(4x4) transforms carries their
    6e-5 (test_conv_winograd_path); the filter gradient keeps its 5e-5."""
    ops = _ops()
    # the smallest shape of test_bn_relu_applied_by_the_next_convolutions_loader that the fused loader takes
    for N, C, H, W, K, G in ((2, 96, 40, 36, 128, 2), (4, 128, 32, 32, 128, 2), (2, 128, 64, 64, 256, 1)):
        probe = torch.nn.BatchNorm2d(C).cuda().train()
        if ops.bn_relu_conv3x3_ok(torch.empty(N, C, H, W, device='cuda'), probe, torch.empty(K, C, 3, 3, device='cuda', requires_grad=True), G):
            break
    else:
        raise AssertionError('no shape takes the fused loader')
    P, B = bn_params(C, 241)
    z = off_the_gates(rnd(N, C, H, W, seed=240) + consumer_offsets(C).view(1, -1, 1, 1), P['gamma'], P['beta'], G)
    assert gate_margins(z, P['gamma'], P['beta'], G, pool=False)[0] >= MARGIN
    w, b, g = rnd(K, C, 3, 3, seed=242, scale=(2.0 / (C * 9)) ** 0.5), rnd(K, seed=243, scale=0.1), rnd(N, K, H, W, seed=244)

    def fn(L, Bf):
        y = F.conv2d(F.relu(bn_train(L['z'], L, Bf, G)), L['w'], L['b'], padding=1)
        return dict(y=y), (y * g.to(y.dtype)).sum()
    T, S = truth_and_stock(fn, dict(z=z, w=w, b=b, **P), B)
    bn = gpu_bn(P, B)
    zin, wg, bg = (t.cuda().requires_grad_(True) for t in (z, w, b))
    zz = zin * 1.0
    assert ops.bn_relu_conv3x3_ok(zz, bn, wg, G)
    y = ops.bn_relu_conv3x3(zz, bn, wg, bg, groups=G)
    y.backward(g.cuda())
    tag = 'bn_relu_conv3x3 '
    assert_rule(y, T['y'], S['y'], 6e-5, tag + 'y')
    assert_rule(zin.grad, T['dz'], S['dz'], 6e-5, tag + 'dz', channel_dim=1)
    assert_rule(wg.grad, T['dw'], S['dw'], 5e-5, tag + 'dw')
    assert_rule(bg.grad, T['db'], S['db'], 2e-5, tag + 'db')
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 6e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 6e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)


def test_output_transform_statistics_under_bias_offsets():
    """``conv2d(..., bn_groups=G)`` sums the BatchNorm statistics in its F(4x4) output transform; the offsets (100 on half the
    filters, 1e3 on one) enter through the convolution's bias, so sum y^2 is ~1e6 per element where the variance is ~1.
    Consumer: ``bn_act`` without an activation -- the gate of a ReLU behind a convolution cannot be kept off the kink by
    construction, and the statistics are what this case is about.  Against batch_norm(conv2d(x)) in fp64."""
    ops = _ops()
    N, C, H, W, K, G = 2, 64, 64, 64, 128, 2
    P, B = bn_params(K, 251)
    x = rnd(N, C, H, W, seed=250)
    w, g = rnd(K, C, 3, 3, seed=252, scale=(2.0 / (C * 9)) ** 0.5), rnd(N, K, H, W, seed=254)
    b = consumer_offsets(K) + rnd(K, seed=253, scale=0.1)

    def fn(L, Bf):
        y = bn_train(F.conv2d(L['x'], L['w'], L['b'], padding=1), L, Bf, G)
        return dict(y=y), (y * g.to(y.dtype)).sum()
    T, S = truth_and_stock(fn, dict(x=x, w=w, b=b, **P), B)
    bn = gpu_bn(P, B)
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    c = ops.conv2d(xg, wg, bg, 1, 1, bn_groups=G)
    assert getattr(c, '_fcd_bn', None) is not None, 'this layer must take the statistics from its output transform'
    y = ops.bn_act(c, bn, ops.ACT_NONE, groups=G)
    y.backward(g.cuda())
    tag = 'conv2d(bn_groups) -> bn_act '
    assert_rule(y, T['y'], S['y'], 6e-5, tag + 'y', channel_dim=1)
    assert_rule(xg.grad, T['dx'], S['dx'], 6e-5, tag + 'dx')
    assert_rule(wg.grad, T['dw'], S['dw'], 5e-5, tag + 'dw')
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)


def test_one_value_per_channel_in_training_is_refused():
    ops = _ops()
    P, B = bn_params(4, 261)
    x = rnd(1, 4, 1, 1, seed=260)
    with pytest.raises(ValueError):
        F.batch_norm(x, B['running_mean'].clone(), B['running_var'].clone(), P['gamma'], P['beta'], True, MOMENTUM, EPS)
    bn = gpu_bn(P, B)
    with pytest.raises(ValueError):
        ops.bn_act(x.cuda(), bn, ops.ACT_RELU)
    with pytest.raises(ValueError):
        ops.bn_act(rnd(2, 4, 1, 1, seed=262).cuda(), bn, ops.ACT_NONE, groups=2)        # one value per channel and group
    assert torch.equal(bn.running_mean.cpu(), B['running_mean']) and int(bn.num_batches_tracked) == 0
    bn.eval()
    assert ops.bn_act(x.cuda(), bn, ops.ACT_NONE).shape == x.shape                     # eval mode normalises a single value


# ================================================================================================ 2. activation kinks
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, FLT_MIN, -FLT_MIN, 1.0, -1.0, float('inf'), float('-inf'), float('nan')]


def kink_input(shape, finite_only):
    """Quarter-integer noise with the special values seeded at the front, in the middle, and over the last elements (the
    float4 kernel's last vector / the scalar kernel's tail)."""
    x = (rnd(*shape, seed=271) * 4).round() / 4
    flat = x.view(-1)
    vals = [v for v in SPECIALS if np.isfinite(v)] if finite_only else SPECIALS
    n, k = flat.numel(), len(vals)
    for start in (0, n // 2 - 3, n - k):
        flat[start:start + k] = torch.tensor(vals, dtype=torch.float32)
    return x


def identity_eval_bn(C):
    """Eval-mode BatchNorm with z == x: gamma 1, beta 0, running_mean 0 and a running_var with fl(running_var + eps) == 1."""
    eps32 = np.float32(EPS)
    rv = np.float32(1) - eps32
    for _ in range(4):
        if rv + eps32 == np.float32(1):
            break
        rv = np.nextafter(rv, np.float32(2) if rv + eps32 < 1 else np.float32(0))
    assert rv + eps32 == np.float32(1)
    bn = torch.nn.BatchNorm2d(C, eps=EPS).cuda()
    with torch.no_grad():
        bn.running_var.fill_(float(rv))
    return bn.eval()


@pytest.mark.parametrize('mode', ['bare', 'eval_bn'])
@pytest.mark.parametrize('act', ['relu', 'leaky', 'prelu'])
@pytest.mark.parametrize('shape', [(2, 3, 4, 8), (2, 3, 5, 7)], ids=['f4', 'scalar'])
def test_activation_kinks(shape, act, mode):
    """+-0, denormals, +-FLT_MIN, +-1, +-inf and NaN through the bare activation and through an eval-mode BatchNorm that is the
    identity: the forward equals ATen's under ``==`` with NaNs in the same places; dx and dslope exactly, on finite inputs
    (at 0: ReLU 0, leaky / PReLU the slope; a zero adds 0 to dslope)."""
    ops = _ops()
    C = shape[1]
    g = (rnd(*shape, seed=272) * 4).round() / 4
    g[g == 0] = 0.5
    for finite_only in (False, True):
        x = kink_input(shape, finite_only)
        sr = torch.tensor([0.25], requires_grad=True)
        xr = x.clone().requires_grad_(True)
        yr = actf(xr, act, sr)
        yr.backward(g)
        xg = x.cuda().requires_grad_(True)
        sg = torch.tensor([0.25], device='cuda', requires_grad=True)
        y = ops.bn_act(xg, identity_eval_bn(C) if mode == 'eval_bn' else None, act_code(ops, act), slope=sg if act == 'prelu' else None,
                       slope_imm=0.2)
        y.backward(g.cuda())
        assert same_with_nans(y, yr), (act, mode, finite_only, y.detach().cpu().view(-1)[:12], yr.detach().view(-1)[:12])
        fin = torch.isfinite(x)
        assert torch.equal(xg.grad.cpu()[fin], xr.grad[fin]), (act, mode, 'dx')
        zero = x == 0
        want0 = {'relu': 0.0, 'leaky': 0.2, 'prelu': 0.25}[act]
        assert torch.equal(xg.grad.cpu()[zero], (g[zero] * np.float32(want0))), (act, mode, 'dx at 0')
        if act == 'prelu' and finite_only:
            # quarter-integer g and x: the sum over x <= 0 is a multiple of 1/16 plus terms below 1e-37, so fp64 summation in any
            # order rounds to the same float as long as the main part is not 0
            main = (g.double() * x.double())[(x <= -0.25)].sum().item()
            assert main != 0.0
            want = np.float32((g.double() * x.double())[x <= 0].sum().item())
            assert sg.grad.item() == float(want), (sg.grad.item(), float(want))


# ================================================================================================ 3. max-pool family
POOL_SHAPES = [(2, 3, 8, 8), (1, 5, 11, 13), (1, 2, 2, 2)]


def tie_input(shape, seed):
    rng = np.random.default_rng([seed] + list(shape))
    return torch.from_numpy(rng.integers(-2, 3, size=shape).astype(np.float32))


def seed_nonfinite(x):
    """NaN / +inf / -inf into the pooling windows, cycling through patterns: one per window in every slot, and several per
    window (NaN after NaN: the later one wins; +inf twice: the first wins; a window of -inf; NaN before and after +inf)."""
    nan, inf = float('nan'), float('inf')
    pats = [[(0, nan)], [(1, nan)], [(2, nan)], [(3, nan)], [(0, inf)], [(3, inf)], [(1, -inf)], [(2, -inf)],
            [(0, nan), (3, nan)], [(1, inf), (2, inf)], [(0, -inf), (1, -inf), (2, -inf), (3, -inf)], [(0, nan), (1, inf)],
            [(1, inf), (3, nan)], [(0, -inf), (2, nan), (3, inf)], [(0, inf), (1, nan), (2, nan)], []]
    x = x.clone()
    N, C, H, W = x.shape
    i = 0
    for n in range(N):
        for c in range(C):
            for p in range(H // 2):
                for q in range(W // 2):
                    for slot, v in pats[i % len(pats)]:
                        x[n, c, 2 * p + slot // 2, 2 * q + slot % 2] = v
                    i += 1
    return x


@pytest.mark.parametrize('nonfinite', [False, True], ids=['ties', 'ties+nonfinite'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda c: 'x'.join(map(str, c)))
def test_maxpool_ties_and_nonfinite_route_like_aten(shape, nonfinite):
    """``maxpool2`` and ``maxpool2_skip`` (pool only, skip only, both) on windows that nearly all tie and, seeded, hold NaN and
    infinities: forward identical to ``F.max_pool2d`` and the gradient on the element ATen picks (first maximum wins, a NaN
    beats everything, the last NaN of a window wins)."""
    ops = _ops()
    x = tie_input(shape, 281)
    w = windows(x[:, :, : shape[2] // 2 * 2, : shape[3] // 2 * 2])
    tied = ((w == w.amax(-1, keepdim=True)).sum(-1) >= 2).float().mean().item()
    assert tied > 0.3 or w.numel() <= 8, tied                            # the maximum of a window is shared more often than not
    if nonfinite:
        x = seed_nonfinite(x)
    gp = tie_input((shape[0], shape[1], shape[2] // 2, shape[3] // 2), 282) + 0.5         # never 0: a routed gradient shows
    gs = tie_input(shape, 283) + 0.25

    def loss_of(use, skip, p, gs_, gp_):
        terms = ([] if use == 'skip_only' else [(p * gp_).sum()]) + ([] if use in ('pool_only', 'plain') else [(skip * gs_).sum()])
        return sum(terms)

    def ref(use):
        xr = x.clone().requires_grad_(True)
        p = F.max_pool2d(xr, 2)
        loss_of(use, xr, p, gs, gp).backward()
        return p.detach(), xr.grad
    for use in ('plain', 'pool_only', 'skip_only', 'both'):
        p_ref, dx_ref = ref(use)
        xg = x.cuda().requires_grad_(True)
        if use == 'plain':
            p = ops.maxpool2(xg)
            (p * gp.cuda()).sum().backward()
        else:
            skip, p = ops.maxpool2_skip(xg)
            assert same_with_nans(skip, x)
            loss_of(use, skip, p, gs.cuda(), gp.cuda()).backward()
        assert same_with_nans(p, p_ref), (use, 'forward')
        if not nonfinite:
            assert torch.equal(p.detach().cpu(), p_ref)
        assert torch.equal(xg.grad.cpu(), dx_ref), (use, 'dx')


@pytest.mark.parametrize('case', [(2, 3, 8, 8, 1), (4, 16, 16, 24, 2)], ids=lambda c: 'x'.join(map(str, c)))
def test_bn_relu_pool_skip_on_tied_windows(case):
    """Integer-valued z: equal inputs stay equal through BatchNorm, so nearly every window ties exactly and distinct values lie
    gamma / std apart.  Both outputs and dz against the fp64 composition, and the positions the pooled gradient is routed to
    (recovered from dz of a pool-only run by undoing the BatchNorm backward with the truth's per-channel sums)."""
    ops = _ops()
    N, C, H, W, G = case
    z = tie_input((N, C, H, W), 291)
    P, B = bn_params(C, 292)
    kink, lead = gate_margins(z, P['gamma'], P['beta'], G, pool=True)
    assert kink >= 1e-3 and lead >= 1e-3, (kink, lead)
    gs = rnd(N, C, H, W, seed=295)
    gp = rnd(N, C, H // 2, W // 2, seed=296)
    gp = torch.where(gp >= 0, 0.5 + gp, -0.5 + gp)                           # |gp| >= 0.5: a routed gradient is unmistakable
    for use in ('both', 'pool_only'):
        def fn(L, Bf):
            a = F.relu(bn_train(L['z'], L, Bf, G))
            p = F.max_pool2d(a, 2)
            return dict(a=a, p=p), (p * gp.to(a.dtype)).sum() + ((a * gs.to(a.dtype)).sum() if use == 'both' else 0.0)
        T, S = truth_and_stock(fn, dict(z=z, **P), B)
        bn = gpu_bn(P, B)
        zin = z.cuda().requires_grad_(True)
        zz = zin * 1.0
        assert ops.bn_relu_pool_skip_ok(zz, bn, G)
        a, p = ops.bn_relu_pool_skip(zz, bn, groups=G)
        ((p * gp.cuda()).sum() + ((a * gs.cuda()).sum() if use == 'both' else 0.0)).backward()
        tag = 'bn_relu_pool_skip ties[%s,%s] ' % ('x'.join(map(str, case)), use)
        assert_rule(a, T['a'], S['a'], 2e-5, tag + 'a', channel_dim=1)
        assert_rule(p, T['p'], S['p'], 2e-5, tag + 'pooled', channel_dim=1)
        assert_rule(zin.grad, T['dz'], S['dz'], 5e-5, tag + 'dz', channel_dim=1)
        if use == 'pool_only':
            # dz = scale * (d - mean(d) - xhat * mean(d * xhat)) with d the routed, ReLU-gated pooled gradient: solve for d
            zd, Ng = z.double(), N // G
            routed_true = torch.zeros_like(zd)
            d_rec = torch.zeros_like(zd)
            a64 = T['a']
            pick = unwindows(torch.zeros_like(windows(a64)).scatter_(-1, windows(a64).argmax(-1, keepdim=True), 1.0))
            routed_true = pick * F.interpolate(gp.double(), scale_factor=2, mode='nearest') * (a64 > 0)
            for i in range(G):
                sl = slice(i * Ng, (i + 1) * Ng)
                m, v = zd[sl].mean((0, 2, 3), keepdim=True), zd[sl].var((0, 2, 3), unbiased=False, keepdim=True)
                xhat = (zd[sl] - m) / torch.sqrt(v + EPS)
                sc = P['gamma'].double().view(1, -1, 1, 1) / torch.sqrt(v + EPS)
                k1 = routed_true[sl].mean((0, 2, 3), keepdim=True)
                k2 = (routed_true[sl] * xhat).mean((0, 2, 3), keepdim=True)
                d_rec[sl] = zin.grad.cpu().double()[sl] / sc + k1 + xhat * k2
            assert (routed_true != 0).sum() > 0
            assert torch.equal(d_rec.abs() > 0.25, routed_true != 0), 'pooled gradient routed to other positions than ATen routes it to'


# ================================================================================================ 4. sigmoid head saturation
def test_conv1x1_head_saturated_logits():
    """Logits from below -100 to above +100: ``1 / (1 + __expf(-v))`` must land on 0 and 1 without a NaN, and y (1 - y) must
    switch the gradient off there."""
    ops = _ops()
    N, C, H, W = 1, 8, 32, 32
    x, w, b, g = rnd(N, C, H, W, seed=301, scale=50.0), rnd(1, C, 1, 1, seed=302, scale=C ** -0.5), rnd(1, seed=303), rnd(N, 1, H, W, seed=304)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    logit = F.conv2d(xr, wr, br)
    assert logit.min().item() <= -100 and logit.max().item() >= 100, (logit.min().item(), logit.max().item())
    yr = torch.sigmoid(logit)
    yr.backward(g.double())
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    assert ops.conv1x1_head_supported(xg, wg)
    y = ops.conv1x1_head(xg, wg, bg, sigmoid=True)
    y.backward(g.cuda())
    yk = y.detach().cpu()
    assert torch.isfinite(yk).all() and yk.min().item() >= 0.0 and yk.max().item() <= 1.0
    assert yk.min().item() == 0.0 and yk.max().item() == 1.0                      # both ends really saturate in fp32
    for t in (xg.grad, wg.grad, bg.grad):
        assert torch.isfinite(t).all()
    assert_close(y, yr, what='y')
    assert_close(xg.grad, xr.grad, what='dx')
    assert_close(wg.grad, wr.grad, what='dw')
    assert_close(bg.grad, br.grad, what='db')
    xf = x.cuda().requires_grad_(True)
    ops.conv1x1_head(xf, w.cuda(), b.cuda(), sigmoid=True).backward(g.cuda())
    assert torch.isfinite(xf.grad).all()
    assert_close(xf.grad, xr.grad, what='dx (frozen filter)')


def test_bn_relu_head_saturated_logits():
    ops = _ops()
    N, C, H, W, G = 1, 8, 32, 32, 1
    P, B = bn_params(C, 311)
    z = off_the_gates(rnd(N, C, H, W, seed=310), P['gamma'], P['beta'], G)
    assert gate_margins(z, P['gamma'], P['beta'], G, pool=False)[0] >= MARGIN
    w, g = rnd(1, C, 1, 1, seed=312, scale=120.0 * C ** -0.5), rnd(N, 1, H, W, seed=314)
    b = torch.tensor([-float((w.view(-1) * 0.4).sum())])                     # centres the logits: E relu(N(0, 1)) = 0.4

    def fn(L, Bf):
        logit = F.conv2d(F.relu(bn_train(L['z'], L, Bf, G)), L['w'], L['b'])
        y = torch.sigmoid(logit)
        return dict(y=y, logit=logit), (y * g.to(y.dtype)).sum()
    T, S = truth_and_stock(fn, dict(z=z, w=w, b=b, **P), B)
    assert T['logit'].min().item() <= -100 and T['logit'].max().item() >= 100, (T['logit'].min().item(), T['logit'].max().item())
    for frozen in (False, True):
        bn = gpu_bn(P, B)
        zin = z.cuda().requires_grad_(True)
        wg, bg = (t.cuda().requires_grad_(not frozen) for t in (w, b))
        zz = zin * 1.0
        assert ops.bn_relu_head_ok(zz, bn, wg, G)
        y = ops.bn_relu_head(zz, bn, wg, bg, sigmoid=True, groups=G)
        y.backward(g.cuda())
        yk = y.detach().cpu()
        assert torch.isfinite(yk).all() and yk.min().item() >= 0.0 and yk.max().item() <= 1.0
        tag = 'bn_relu_head saturated%s ' % (' (frozen filter)' if frozen else '')
        assert_rule(y, T['y'], S['y'], 2e-5, tag + 'y')
        # per tensor: y (1 - y) is formed from the fp32 y on both sides, and where y -> 1 its rounding (6e-8 on 1 - y = 1e-5 .. 1e-3)
        # is the whole error -- per channel the kernel / stock ratio is a quotient of two sums of such random roundings
        assert_rule(zin.grad, T['dz'], S['dz'], 5e-5, tag + 'dz')
        assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma')
        assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta')
        if not frozen:
            assert_rule(wg.grad, T['dw'], S['dw'], 2e-5, tag + 'dw')
            assert_rule(bg.grad, T['db'], S['db'], 2e-5, tag + 'db')


# ================================================================================================ 5. masked loss kernels
LOSS_SHAPES = [(2, 2, 130, 130), (3, 5, 17, 23)]


def loss_case(shape, complement):
    """a, b, binary mask; a == b on a block where the weight is 1 (the L1 kink with a live weight)."""
    N, C, H, W = shape
    a, b = rnd(N, C, H, W, seed=321), rnd(N, C, H, W, seed=322)
    m = (rnd(N, 1, H, W, seed=323) > 0).float()
    m[:, :, : H // 3, : W // 2] = 0.0 if complement else 1.0
    a[:, :, : H // 3, : W // 2] = b[:, :, : H // 3, : W // 2]
    w = (1 - m) if complement else m
    assert set(m.unique().tolist()) == {0.0, 1.0} and bool((w[:, :, : H // 3, : W // 2] == 1).all())
    assert bool((w.sum((1, 2, 3)) > 0).all())
    return a, b, m


def masked_terms(ar, br, mr, kind, complement):
    w = (1 - mr) if complement else mr
    d = (ar - br) * w
    return (d.abs() if kind == 0 else d * d).sum((1, 2, 3)), w.sum((1, 2, 3))


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('complement', [False, True])
@pytest.mark.parametrize('kind', [0, 1])
def test_masked_sums_and_ratio_mean_on_binary_masks(kind, complement, shape):
    """Binary masks, an exact-zero difference under a live weight, and (130 x 130) a plane longer than one sweep of the
    strided reduction (64 blocks x 256 pixels): against fp64 autograd under the bounds of test_gpu_ops.py."""
    ops = _ops()
    N, C, H, W = shape
    assert (H * W > 64 * 256) == (shape == LOSS_SHAPES[0])          # 130 x 130 enters the second sweep, 17 x 23 does not
    a, b, m = loss_case(shape, complement)
    coef, cw = rnd(N, seed=324), rnd(N, seed=325)
    ar, br, mr = (t.double().requires_grad_(True) for t in (a, b, m))
    num, ws = masked_terms(ar, br, mr, kind, complement)
    (num * coef.double() + ws * cw.double()).sum().backward()
    ag, bg, mg = (t.cuda().requires_grad_(True) for t in (a, b, m))
    n2, w2 = ops.masked_sums(ag, bg, mg, kind, complement)
    (n2 * coef.cuda() + w2 * cw.cuda()).sum().backward()
    assert_close(n2, num, what='num')
    assert_close(w2, ws, what='wsum')
    assert w2.cpu().tolist() == ws.tolist()                         # a count of ones is exact
    assert_close(ag.grad, ar.grad, what='da')
    assert_close(bg.grad, br.grad, what='db')
    assert_close(mg.grad, mr.grad, what='dm')
    if kind == 0:
        blk = (slice(None), slice(None), slice(0, H // 3), slice(0, W // 2))
        assert bool((ag.grad.cpu()[blk] == 0).all()) and bool((bg.grad.cpu()[blk] == 0).all())       # the L1 kink
    scale = 1.0 / C
    ar, br, mr = (t.double().requires_grad_(True) for t in (a, b, m))
    num, ws = masked_terms(ar, br, mr, kind, complement)
    ref = (num * scale / ws).sum() / N
    (ref * 1.7).backward()
    for skip_zero in (False, True):
        ag, bg, mg = (t.cuda().requires_grad_(True) for t in (a, b, m))
        out = ops.masked_ratio_mean(ag, bg, mg, kind, complement, scale, skip_zero)
        (out * 1.7).backward()
        assert_close(out, ref, tol=2e-6, what='loss')
        assert_close(ag.grad, ar.grad, tol=2e-6, what='da')
        assert_close(bg.grad, br.grad, tol=2e-6, what='db')
        assert_close(mg.grad, mr.grad, tol=2e-6, what='dm')


def same_class_and_value(got, ref, tol, what):
    """Non-finite entries of the same class in the same places; the finite rest within ``tol`` of scale."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    for name, f in (('nan', torch.isnan), ('+inf', torch.isposinf), ('-inf', torch.isneginf)):
        assert torch.equal(f(got), f(ref)), '%s: %s in other places (%d vs %d)' % (what, name, int(f(got).sum()), int(f(ref).sum()))
    fin = torch.isfinite(ref)
    if fin.any():
        assert_close(got[fin], ref[fin], tol=tol, what=what)


@pytest.mark.parametrize('complement', [False, True])
@pytest.mark.parametrize('kind', [0, 1])
def test_masked_ratio_mean_when_every_sample_is_empty(kind, complement):
    """wsum == 0 in every sample.  ``skip_zero`` (the reference's ``continue``): the loss and every gradient are exactly 0.
    Without it the kernel computes 0 / 0: the non-finite values sit where the same fp32 expression puts them through
    autograd."""
    ops = _ops()
    N, C, H, W = 3, 5, 17, 23
    a, b = rnd(N, C, H, W, seed=331), rnd(N, C, H, W, seed=332)
    m = torch.ones(N, 1, H, W) if complement else torch.zeros(N, 1, H, W)
    scale = 1.0 / C
    ag, bg, mg = (t.cuda().requires_grad_(True) for t in (a, b, m))
    out = ops.masked_ratio_mean(ag, bg, mg, kind, complement, scale, True)
    (out * 1.7).backward()
    assert out.item() == 0.0
    for t in (ag.grad, bg.grad, mg.grad):
        assert bool((t == 0).all()) and torch.isfinite(t).all()
    ar, br, mr = (t.clone().requires_grad_(True) for t in (a, b, m))
    num, ws = masked_terms(ar, br, mr, kind, complement)
    assert bool((ws == 0).all())
    ref = (num * scale / ws).sum() / N
    (ref * 1.7).backward()
    ag, bg, mg = (t.cuda().requires_grad_(True) for t in (a, b, m))
    out = ops.masked_ratio_mean(ag, bg, mg, kind, complement, scale, False)
    (out * 1.7).backward()
    same_class_and_value(out, ref, 2e-6, 'loss')
    same_class_and_value(ag.grad, ar.grad, 2e-6, 'da')
    same_class_and_value(bg.grad, br.grad, 2e-6, 'db')
    same_class_and_value(mg.grad, mr.grad, 2e-6, 'dm')


# ================================================================================================ 6. beyond the grid caps
@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_optimizer_step_beyond_the_grid_cap(kind):
    ops = _ops()
    n = 4096 * 256 + 257
    assert n > 4096 * 256
    p0, gs = rnd(n, seed=341), [rnd(n, seed=342), rnd(n, seed=343) * 0.1]
    p0[-1] = 7.5
    for g in gs:
        g[-1] = -3.0
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=2e-3, betas=(0.9, 0.99)) if kind == 'adam' else torch.optim.RMSprop([pr], lr=5e-4)
    pg = p0.cuda()
    s1, s2 = torch.zeros_like(pg), torch.zeros_like(pg)
    for step, g in enumerate(gs, 1):
        pr.grad = g.clone()
        opt.step()
        if kind == 'adam':
            ops.adam_step(pg, g.cuda(), s1, s2, 2e-3, 0.9, 0.99, 1e-8, 0.0, step)
        else:
            ops.rmsprop_step(pg, g.cuda(), s1, 5e-4, 0.99, 1e-8, 0.0)
    st = opt.state[pr]
    assert (pr.detach() != p0).float().mean().item() > 0.99                    # stock moved (nearly) every element: so must the kernel
    assert_close(pg, pr, tol=1e-6, what=kind)
    assert_close(pg[-300:], pr[-300:], tol=1e-6, what=kind + ' tail')
    assert abs(pg[-1].item() - pr[-1].item()) <= 1e-6 * 7.5
    if kind == 'adam':
        assert_close(s1, st['exp_avg'], tol=1e-6, what='exp_avg')
        assert_close(s2, st['exp_avg_sq'], tol=1e-6, what='exp_avg_sq')
        assert_close(s2[-300:], st['exp_avg_sq'][-300:], tol=1e-6, what='exp_avg_sq tail')
    else:
        assert_close(s1, st['square_avg'], tol=1e-6, what='square_avg')
        assert_close(s1[-300:], st['square_avg'][-300:], tol=1e-6, what='square_avg tail')


def test_maxpool_beyond_the_grid_cap():
    ops = _ops()
    shape = (1, 9, 1024, 1024)
    assert 9 * 512 * 512 > 8192 * 256
    x = rnd(*shape, seed=351)
    x[0, -1, -1, -1] = 100.0
    g = rnd(1, 9, 512, 512, seed=352)
    g[0, -1, -1, -1] = 77.0
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    yr.backward(g)
    xg = x.cuda().requires_grad_(True)
    y = ops.maxpool2(xg)
    y.backward(g.cuda())
    assert torch.equal(y.detach().cpu(), yr.detach())
    assert torch.equal(xg.grad.cpu(), xr.grad)
    assert y[0, -1, -1, -1].item() == 100.0 and xg.grad[0, -1, -1, -1].item() == 77.0


def host_normalize(x, mean, std, valid=None):
    out = ((x.double() - torch.tensor(mean, dtype=torch.float64).view(1, -1, 1, 1)) /
           torch.tensor(std, dtype=torch.float64).view(1, -1, 1, 1)).float()
    return out if valid is None else torch.where(valid != 0, out, torch.zeros_like(out))


def test_normalize_tiles_beyond_the_grid_cap():
    ops = _ops()
    shape = (1, 3, 840, 840)
    assert 3 * 840 * 840 > 8192 * 256
    x = (rnd(*shape, seed=361) * 900 + 3000).round().clamp(0, 65535)
    x[0, -1, -1, -1] = 65535.0
    mean, std = [2971.3, 3104.9, 2856.75], [913.2, 877.01, 1021.5]
    want = host_normalize(x, mean, std)
    got = ops.normalize_tiles(x.cuda(), mean, std).cpu()
    assert torch.equal(got, want)
    assert got[0, -1, -1, -1].item() == want[0, -1, -1, -1].item() != 0.0


def test_bn_act_beyond_the_plane_grid_cap():
    """HW = 520 * 520 = 270 400 is 67 chunks of 4096: ``plane_grid`` caps at 64, the apply kernels sweep a fifth time."""
    ops = _ops()
    shape, groups = (2, 2, 520, 520), 1
    assert -(-shape[2] * shape[3] // (256 * 4 * 4)) > 64
    P, B = bn_params(2, 371)
    x = rnd(*shape, seed=370) * 1.5 + 0.3
    x[-1, -1, -1, -1] = 6.0
    x = off_the_gates(x, P['gamma'], P['beta'], groups)
    assert gate_margins(x, P['gamma'], P['beta'], groups, pool=False)[0] >= MARGIN
    g = rnd(*shape, seed=372)
    g[-1, -1, -1, -1] = 5.0

    def fn(L, Bf):
        y = F.relu(bn_train(L['x'], L, Bf, groups))
        return dict(y=y), (y * g.to(y.dtype)).sum()
    T, S = truth_and_stock(fn, dict(x=x, **P), B)
    assert T['y'][-1, -1, -1, -1].item() > 1.0 and abs(T['dx'][-1, -1, -1, -1].item()) > 1.0
    bn = gpu_bn(P, B)
    xg = x.cuda().requires_grad_(True)
    y = ops.bn_act(xg, bn, ops.ACT_RELU, groups=groups)
    y.backward(g.cuda())
    tag = 'bn_act[520x520] '
    assert_rule(y, T['y'], S['y'], 2e-5, tag + 'y', channel_dim=1)
    assert_rule(xg.grad, T['dx'], S['dx'], 5e-5, tag + 'dx', channel_dim=1)
    assert_rule(y[:, :, -40:], T['y'][:, :, -40:], S['y'][:, :, -40:], 2e-5, tag + 'y, last rows', channel_dim=1)
    assert_rule(xg.grad[:, :, -40:], T['dx'][:, :, -40:], S['dx'][:, :, -40:], 5e-5, tag + 'dx, last rows', channel_dim=1)
    assert_rule(bn.weight.grad, T['dgamma'], S['dgamma'], 5e-5, tag + 'dgamma', channel_dim=0, tensor_scale=True)
    assert_rule(bn.bias.grad, T['dbeta'], S['dbeta'], 5e-5, tag + 'dbeta', channel_dim=0, tensor_scale=True)
    assert_rule(bn.running_mean, T['running_mean'], S['running_mean'], 2e-5, tag + 'running_mean', channel_dim=0)
    assert_rule(bn.running_var, T['running_var'], S['running_var'], 2e-5, tag + 'running_var', channel_dim=0)


# ================================================================================================ 7. optimizer kernels
def optimizer_grads(n, steps, seed):
    """A block that is exactly 0 in every step, a block at 1e-30 (its square underflows), the rest N(0, 1)."""
    z, t = n // 3, 2 * n // 3
    gs = []
    for s in range(steps):
        g = rnd(n, seed=seed + s)
        g[:z] = 0.0
        g[z:t] = 1e-30
        gs.append(g)
    return gs, z


def stock_run(kind, p0, gs, wd, grad_scale, lrs, dtype):
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = (torch.optim.Adam([p], lr=lrs[0], betas=(0.9, 0.99), eps=1e-8, weight_decay=wd) if kind == 'adam'
           else torch.optim.RMSprop([p], lr=lrs[0], alpha=0.99, eps=1e-8, weight_decay=wd))
    for s, g in enumerate(gs):
        opt.param_groups[0]['lr'] = lrs[s]
        p.grad = (g * np.float32(grad_scale)).to(dtype)                    # the fp32 product the kernel forms, then cast
        opt.step()
    return p.detach()


@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('n', [1, 255, 257])
@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_optimizer_kernels_with_weight_decay_grad_scale_and_zero_gradients(kind, n, wd, grad_scale):
    """20 steps, learning rate changed after step 10, against torch.optim in fp32 (1e-6, the bound of
    test_adam_rmsprop_match_torch) and under the tolerance rule against an fp64 run; the ``_h`` variants (scalars read from
    device memory) bit for bit."""
    ops = _ops()
    steps = 20
    lrs = [1e-2] * 10 + [3e-3] * 10
    p0 = rnd(n, seed=381) + 0.5
    gs, z = optimizer_grads(n, steps, 382)
    stock, truth = stock_run(kind, p0, gs, wd, grad_scale, lrs, torch.float32), stock_run(kind, p0, gs, wd, grad_scale, lrs, torch.float64)
    pg, ph = p0.cuda(), p0.cuda()
    s1, s2, h1, h2 = (torch.zeros(n, device='cuda') for _ in range(4))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.99))
    for s, g in enumerate(gs):
        gg, step = g.cuda(), s + 1
        if kind == 'adam':
            ops.adam_step(pg, gg, s1, s2, lrs[s], 0.9, 0.99, 1e-8, wd, step, grad_scale)
            hyper = torch.tensor([lrs[s], 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)], dtype=torch.float32).cuda()
            ops.adam_step_h(ph, gg, h1, h2, hyper, 0.9, 0.99, 1e-8, wd, grad_scale)
        else:
            ops.rmsprop_step(pg, gg, s1, lrs[s], 0.99, 1e-8, wd, grad_scale)
            ops.rmsprop_step_h(ph, gg, h1, torch.tensor([lrs[s]], dtype=torch.float32).cuda(), 0.99, 1e-8, wd, grad_scale)
    assert (stock - p0).abs().max().item() > 1e-3                                  # the run moved something
    assert_close(pg, stock, tol=1e-6, what=kind)
    assert_rule(pg, truth, stock, 1e-6, '%s[n=%d,wd=%g,gs=%g] p' % (kind, n, wd, grad_scale))
    assert torch.equal(ph, pg) and torch.equal(h1, s1) and torch.equal(h2, s2), '_h variant differs'
    if wd == 0.0 and z:
        assert torch.equal(pg[:z].cpu(), p0[:z]), 'zero gradient, no weight decay: the parameter must not move'
        assert torch.equal(stock[:z], p0[:z])
    if wd != 0.0 and z:
        assert (stock[:z] != p0[:z]).all()                                         # weight decay alone moves it


@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_optimizer_classes_with_weight_decay(kind):
    """``optim.Adam`` / ``optim.RMSprop`` (flat buffers, one launch) with weight decay over parameters of 3, 1, 35 and 216
    elements; gradients from plain autograd, accumulated over steps except for one ``zero_grad()`` followed by
    ``p.grad = None`` on one parameter (a gradient that does not live in the flat buffer); against torch.optim."""
    from fcd_gan_pytorch_amd import optim as foptim
    shapes = [(3,), (1,), (5, 7), (8, 3, 3, 3)]
    init = [rnd(*s, seed=391 + i) for i, s in enumerate(shapes)]
    tgt = [rnd(*s, seed=395 + i) for i, s in enumerate(shapes)]
    ours = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    theirs = [torch.nn.Parameter(t.clone()) for t in init]
    if kind == 'adam':
        o = foptim.Adam(ours, lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-2)
        t = torch.optim.Adam(theirs, lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-2)
    else:
        o = foptim.RMSprop(ours, lr=1e-2, weight_decay=1e-2)
        t = torch.optim.RMSprop(theirs, lr=1e-2, weight_decay=1e-2)
    for step in range(5):
        for opt, ps, tg in ((o, ours, [q.cuda() for q in tgt]), (t, theirs, tgt)):
            if step == 2:
                opt.zero_grad()
                ps[2].grad = None
            loss = sum(((p - q) ** 2).sum() * (0.5 + i) for i, (p, q) in enumerate(zip(ps, tg)))
            loss.backward()
            opt.step()
    for i, (p, q) in enumerate(zip(ours, theirs)):
        assert (q.detach() - init[i]).abs().max().item() > 1e-3
        assert_close(p, q, tol=1e-6, what='%s parameter %d' % (kind, i))


# ================================================================================================ 8. SSIM on flat / identical images
def ssim_inputs(kind, shape):
    """(X, Y) of one of the edge inputs, any rank: piecewise-constant 8 x 4 blocks in the last two axes."""
    if kind == 'blocks' or kind == 'identical':
        H, W = shape[-2:]
        lv = torch.from_numpy(np.random.default_rng(401).integers(0, 4, size=shape[:-2] + (-(-H // 8), -(-W // 4))).astype(np.float32)) / 3
        x = lv.repeat_interleave(8, -2).repeat_interleave(4, -1)[..., :H, :W].contiguous()
        y = x.clone() if kind == 'identical' else (x + 0.05 * rnd(*shape, seed=402)).clamp(0, 1)
        return x, y
    if kind == 'constants':
        return torch.full(shape, 0.7), torch.full(shape, 0.2)
    if kind == 'zeros':
        return torch.zeros(shape), torch.zeros(shape)
    assert kind == 'offset100'
    return 100 + rnd(*shape, seed=403), 100 + rnd(*shape, seed=404)


SSIM_KINDS = ['blocks', 'identical', 'constants', 'zeros', 'offset100']


@pytest.mark.parametrize('kind', SSIM_KINDS)
@pytest.mark.parametrize('shape', [(1, 2, 40, 52), (1, 1, 12, 13, 21)], ids=['rank4', 'rank5'])
def test_ssim_level_on_flat_identical_and_offset_images(shape, kind):
    """sigma^2 = E[x^2] - mu^2 is pure rounding noise on flat regions (against C2 = 9e-4) and loses four digits at an offset
    of 100: the fused level against the op-by-op restatement of the reference (rank 4: oracle.losses.ssim_level; rank 5:
    tests/golden/ssim3d_truth.py) in fp64, with the same restatement in fp32 as the yardstick."""
    ops = _ops()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    if len(shape) == 4:
        from oracle import losses as ol
        level = lambda X, Y, dt: ol.ssim_level(X, Y, ol.gauss_window().to(dt))
        win = ol.gauss_window()
    else:
        import ssim3d_truth as T3
        level = lambda X, Y, dt: T3.level(X, Y, T3.taps(dtype=dt), C1, C2)
        win = T3.taps()
    x, y = ssim_inputs(kind, shape)
    N, C = shape[:2]
    ws, wc = rnd(N, C, seed=405), rnd(N, C, seed=406)

    def fn(L, Bf):
        s, cs = level(L['x'], L['y'], L['x'].dtype)
        return dict(ssim=s, cs=cs), (s * ws.to(s.dtype)).sum() + (cs * wc.to(s.dtype)).sum()
    T, S = truth_and_stock(fn, dict(x=x, y=y), {})
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    s, cs = ops.ssim_level(xg, yg, win.cuda(), C1, C2)
    ((s * ws.cuda()).sum() + (cs * wc.cuda()).sum()).backward()
    tag = 'ssim[rank%d,%s] ' % (len(shape), kind)
    if kind in ('identical', 'zeros'):
        assert (T['ssim'] - 1).abs().max().item() < 1e-12 and (T['cs'] - 1).abs().max().item() < 1e-12
        assert T['dx'].abs().max().item() < 1e-12 and T['dy'].abs().max().item() < 1e-12          # the truth is 1 with gradient 0
        ulp = 2.0 ** -23
        assert (s.detach().cpu().double() - 1).abs().max().item() <= ulp, (s - 1).abs().max().item()
        assert (cs.detach().cpu().double() - 1).abs().max().item() <= ulp, (cs - 1).abs().max().item()
        for got, name in ((xg.grad, 'dx'), (yg.grad, 'dy')):
            ek = (got.cpu().double() - T[name]).abs().max().item()
            es = (S[name].double() - T[name]).abs().max().item()
            print('RULE %-58s kernel %.3e  stock %.3e  (absolute)' % (tag + name, ek, es))
            assert torch.isfinite(got).all()
            assert ek <= 4 * es, (tag + name, ek, es)
        return
    assert_rule(s, T['ssim'], S['ssim'], 2e-5, tag + 'ssim')
    assert_rule(cs, T['cs'], S['cs'], 2e-5, tag + 'cs')
    assert_rule(xg.grad, T['dx'], S['dx'], 1e-4, tag + 'dX')
    assert_rule(yg.grad, T['dy'], S['dy'], 1e-4, tag + 'dY')


# ================================================================================================ 9. normalize_tiles outside the valid window
def test_normalize_tiles_ignores_what_lies_outside_the_valid_window():
    ops = _ops()
    N, C, H, W = 2, 3, 9, 11
    x = (rnd(N, C, H, W, seed=411) * 900 + 3000).round().clamp(0, 65535)
    valid = torch.zeros(N, 1, H, W)
    valid[0, :, :6, :7] = 1.0
    valid[1, :, 2:, 3:] = 1.0
    out_of = (valid == 0).expand(N, C, H, W)
    junk = torch.tensor([float('nan'), float('inf'), 65535.0, float('-inf')]).repeat(out_of.sum().item() // 4 + 1)[: out_of.sum().item()]
    x[out_of] = junk
    mean, std = [2971.3, 3104.9, 2856.75], [913.2, 877.01, 1021.5]
    got = ops.normalize_tiles(x.cuda(), mean, std, valid=valid.cuda()).cpu()
    assert bool((got[out_of] == 0).all())
    inside = ~out_of
    want = host_normalize(x, mean, std)
    assert torch.equal(got[inside], want[inside]) and bool((want[inside] != 0).any())
