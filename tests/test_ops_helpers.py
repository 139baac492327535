"""The shared helpers of the autograd op layer (_ops.py) that hold a rule every op relies on, on CPU tensors: when the BatchNorm
partial-sum tag of a convolution's output may still be used, and when a cached filter pack is rebuilt."""
import torch


def _ops():
    from fcd_gan_pytorch_amd import _ops as ops
    return ops


def _tagged(groups=2, split=4):
    z = torch.zeros(4, 8, 4, 4)
    buf = torch.zeros(16, dtype=torch.float64)
    z._fcd_bn = (buf, split, groups, z.data_ptr(), z._version)      # what _tag_bn leaves behind
    return z, buf


def test_bn_parts_returns_the_sums_only_for_the_tensor_as_the_kernel_wrote_it():
    ops = _ops()
    z, buf = _tagged(groups=2, split=4)
    got = ops._bn_parts(z, 2)
    assert got is not None and got[0] is buf and got[1] == 4
    assert ops._bn_parts(torch.zeros(2, 2, 2, 2), 1) is None            # no tag
    assert ops._bn_parts(z, 1) is None and ops._bn_parts(z, 4) is None      # another group count
    other = torch.zeros(4, 8, 4, 4)
    other._fcd_bn = z._fcd_bn                                           # the tag copied onto a different tensor
    assert other._version == z._version and ops._bn_parts(other, 2) is None
    z0, _ = _tagged(groups=2, split=0)                                  # the producing layer left no sums
    assert ops._bn_parts(z0, 2) is None
    z.add_(1)                                                           # in-place edit: same storage, later version
    assert z._fcd_bn[3] == z.data_ptr() and ops._bn_parts(z, 2) is None


def test_pack_cache_packs_once_per_weight_version_and_key():
    ops = _ops()
    w = torch.arange(24, dtype=torch.float32).reshape(2, 3, 2, 2).transpose(0, 1)      # (non-contiguous: the pack step gets a contiguous copy)
    calls = []

    def packer(tag, scale):
        def pack(src, buf):
            assert src.is_contiguous() and not src.requires_grad and buf.dtype == torch.float32 and buf.numel() == w.numel()
            calls.append(tag)
            buf.copy_(src.reshape(-1) * scale)
        return pack

    a = ops._cached_pack(w, 'a', w.numel, packer('a', 2.0))
    assert calls == ['a'] and torch.equal(a, w.reshape(-1) * 2.0)
    assert ops._cached_pack(w, 'a', w.numel, packer('a', 2.0)) is a and calls == ['a']      # second call: same buffer, nothing packed
    b = ops._cached_pack(w, ('b', 1), w.numel, packer('b', 3.0))                            # two keys on one weight do not collide
    assert calls == ['a', 'b'] and b is not a and torch.equal(b, w.reshape(-1) * 3.0) and torch.equal(a, w.reshape(-1) * 2.0)
    assert ops._cached_pack(w, 'a', w.numel, packer('a', 2.0)) is a and calls == ['a', 'b']
    ver, buf = w.__dict__['_fcd_pack']['a']                                                 # what refresh_packs reads
    assert ver == w._version and buf is a and set(w.__dict__['_fcd_pack']) == {'a', ('b', 1)}

    w.mul_(2.0)                                                                             # in-place edit of the weight: packs again
    a2 = ops._cached_pack(w, 'a', w.numel, packer('a', 2.0))
    assert calls == ['a', 'b', 'a'] and a2 is not a and torch.equal(a2, w.reshape(-1) * 2.0)
    assert w.__dict__['_fcd_pack']['a'][0] == w._version
    assert ops._cached_pack(w, ('b', 1), w.numel, packer('b', 3.0)) is not b and calls == ['a', 'b', 'a', 'b']

    ops.invalidate_packs([w])                                                               # drops the entries
    assert '_fcd_pack' not in w.__dict__
    a3 = ops._cached_pack(w, 'a', w.numel, packer('a', 2.0))
    assert calls == ['a', 'b', 'a', 'b', 'a'] and a3 is not a2
