"""The gate of the augmenting ingest on the GPU (csrc/augment.hip: sp_augment_ingest_gated / sp_augment_ingest_bwd_gated; ops.
augment_ingest_image(..., p=) / augment_ingest_image_pair(..., p=)), through the C ABI and through ops.

Every comparison is for EQUALITY OF BITS: a live image (u7 < p) must be the ungated entry's image and a dead one the plain ingest's
(sp_ingest_image / sp_ingest_image_bwd with scale3 / shift3 NULL), so the ungated entries and the plain ingest are the references and
no tolerance exists.  (tests/test_gpu_augment.py holds the ungated entries to their rounding bound against float64.)

Cases: 5 images of 3 x 16 x 24 (one statistics partial per image and direction) and of 3 x 56 x 52 (8736 source elements = two forward
partials of 8192, 2912 pixels = two backward partials of 2048); u7 = {0, 0.25, nextafter(0.5, 0), 0.5, 0.75} against p = 0.5: images
0 - 2 live, 3 - 4 dead, the strict compare decided at u7 == p and one ulp below; fp32 / bf16 / fp16 storage; NCHW and channels-last
sources; policies 7 (two launches per direction) and 6 (one).  The operands are random normals (not exact in 16 bits) with a -0.0, a
value the plain ingest turns into +0.0 (x * 1 + 0)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SHAPES = ((16, 24), (56, 52))
POLICIES = (7, 6)
LAYOUTS = ("nchw", "channels_last")
N = 5
U7 = (0.0, 0.25, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.5, 0.75)
LIVE, DEAD = slice(0, 3), slice(3, 5)
CANARY = 1234.5
PAD = 64

ids = dict(ids=lambda v: str(v).split(".")[-1] if isinstance(v, torch.dtype) else ("%dx%d" % v if isinstance(v, tuple) else str(v)))


def _dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _operands(hw):
    """Source, dy and uniforms of one map size (host, fp32): computed once, shared, never written."""
    h, w = hw
    g = torch.Generator().manual_seed(40 + h)
    x, dy = torch.randn(N, 3, h, w, generator=g), torch.randn(N, 3, h, w, generator=g)
    x[:, 1, 2, 3] = -0.0
    u = torch.rand(N, 8, generator=g)
    u[:, 7] = torch.tensor(U7)
    return x, dy, u


def _source(x, layout, dev):
    x = x.to(dev)
    return x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous()


def _padded_dy(dy, dtype, dev):
    n, _, h, w = dy.shape
    full = ops.nhwc_empty(n, ops.pad_channels(3, dtype), h, w, dtype, dev)
    full.fill_(7.0)                                       # junk in the padding channels: no sum may read it
    full[:, :3] = dy.to(dev, dtype)
    return full


def _p(value, dev):
    return torch.tensor([value], dtype=torch.float32, device=dev)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


class _Run:
    """One forward and one backward call through the C ABI on windows carved out of canary-filled buffers.  entry: "gated" (with p),
    "ungated" or "plain".  The partials' interior is NaN on entry: a result that read a value nobody wrote is NaN."""

    def __init__(self, xs, dyp, u, policy, dtype, entry, p=None):
        dev = xs.device
        n, _, h, w = xs.shape
        cp, esz = ops.pad_channels(3, dtype), torch.empty((), dtype=dtype).element_size()
        self.out = torch.full((PAD + n * h * w * cp + PAD,), CANARY, dtype=dtype, device=dev)
        self.grad = torch.full((PAD + n * h * w * 3 + PAD,), CANARY, dtype=dtype, device=dev)
        self.parts = [torch.full((PAD + n * ops.augment_slices(h, w, b) + PAD,), CANARY, dtype=torch.float32, device=dev) for b in (False, True)]
        for part in self.parts:
            part[PAD:-PAD] = float("nan")
        at = lambda t, size: ctypes.c_void_p(t.data_ptr() + PAD * size)      # noqa: E731
        dt, st = ops.sp_dtype(dtype), ops.stream()
        if entry == "plain":
            L.call("sp_ingest_image", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, 3, h, w, cp, None, None, dt, st)
            L.call("sp_ingest_image_bwd", ops.ptr(dyp), cp, at(self.grad, esz), 3, n * h * w, None, dt, st)
        elif entry == "ungated":
            L.call("sp_augment_ingest", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   at(self.parts[0], 4), dt, st)
            L.call("sp_augment_ingest_bwd", ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy, at(self.parts[1], 4), dt, st)
        else:
            L.call("sp_augment_ingest_gated", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   at(self.parts[0], 4), ops.ptr(p), dt, st)
            L.call("sp_augment_ingest_bwd_gated", ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy, at(self.parts[1], 4),
                   ops.ptr(p), dt, st)
        torch.cuda.synchronize()
        for buf in [self.out, self.grad] + self.parts:
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), entry
        self.y = _bits(self.out[PAD:-PAD].view(n, h, w, cp))               # (n, h, w, cp) bits
        self.dx = _bits(self.grad[PAD:-PAD].view(n, h, w, 3))


@pytest.mark.parametrize("hw", SHAPES, **ids)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_live_images_are_the_ungated_entry_and_dead_ones_the_plain_ingest_bit_for_bit(dtype, policy, layout, hw):
    dev = _dev()
    x, dy, u = _operands(hw)
    xs, dyp, ud = _source(x, layout, dev), _padded_dy(dy, dtype, dev), u.to(dev)
    ungated, plain = _Run(xs, dyp, ud, policy, dtype, "ungated"), _Run(xs, dyp, ud, policy, dtype, "plain")
    gated = _Run(xs, dyp, ud, policy, dtype, "gated", _p(0.5, dev))
    for name in ("y", "dx"):
        got = getattr(gated, name)
        assert torch.equal(got[LIVE], getattr(ungated, name)[LIVE]), (name, "live")
        assert torch.equal(got[DEAD], getattr(plain, name)[DEAD]), (name, "dead")
        # the two references differ on every image (u falls as it may): the comparison above is not blind to the gate
        for i in range(N):
            assert not torch.equal(getattr(ungated, name)[i], getattr(plain, name)[i]), (name, i)
    assert bool((gated.y[..., 3:] == 0).all())                                               # the padding channels
    # the plain ingest's -0.0 -> +0.0 on a dead image, to the bit
    assert int(gated.y[3, 2, 3, 1]) == 0 and int(plain.y[3, 2, 3, 1]) == 0
    # p = 1 is the ungated call, p = 0 the plain ingest, over the whole batch; two runs agree
    one, zero = _Run(xs, dyp, ud, policy, dtype, "gated", _p(1.0, dev)), _Run(xs, dyp, ud, policy, dtype, "gated", _p(0.0, dev))
    again = _Run(xs, dyp, ud, policy, dtype, "gated", _p(0.5, dev))
    for name in ("y", "dx"):
        assert torch.equal(getattr(one, name), getattr(ungated, name)), (name, "p = 1")
        assert torch.equal(getattr(zero, name), getattr(plain, name)), (name, "p = 0")
        assert torch.equal(getattr(again, name), getattr(gated, name)), (name, "second run")
    # no live image's result leaned on a partial nobody wrote (their interior was NaN on entry)
    assert not bool(torch.isnan(gated.out[PAD:-PAD].float()).any()) and not bool(torch.isnan(gated.grad[PAD:-PAD].float()).any())


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_ops_carry_the_gate_forward_and_backward_and_the_pair_form_equals_two_single_calls(dtype):
    dev = _dev()
    hw = (56, 52)
    x, dy, u = _operands(hw)
    ud, p = u.to(dev), _p(0.5, dev)
    ops.set_compute_dtype(dtype)
    try:
        for policy in POLICIES:
            for layout in LAYOUTS:
                xs = _source(x, layout, dev)
                dyp = _padded_dy(dy, dtype, dev)
                ref = _Run(xs, dyp, ud, policy, dtype, "gated", p)
                xr = xs.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
                y = ops.augment_ingest_image(xr, dtype, ud, policy, p=p)
                (dx,) = torch.autograd.grad(y, xr, dyp)
                assert dx.dtype == torch.float32 and dx.shape == xr.shape
                assert torch.equal(_bits(y.detach().permute(0, 2, 3, 1)), ref.y), (policy, layout)
                want_dx = ref.grad[PAD:-PAD].view(N, hw[0], hw[1], 3).float()               # stored in the compute type, handed back as fp32
                assert torch.equal(_bits(dx.permute(0, 2, 3, 1)), _bits(want_dx)), (policy, layout)
            xa, xb = _source(x, "nchw", dev), _source(x.flip(0), "channels_last", dev)
            ub = u.flip(0).contiguous().to(dev)
            pair = ops.augment_ingest_image_pair(xa, xb, dtype, ud, ub, policy, p=p)
            assert not pair.requires_grad and tuple(pair.shape) == (2 * N, ops.pad_channels(3, dtype)) + hw
            single = torch.cat([ops.augment_ingest_image(xa, dtype, ud, policy, p=p).permute(0, 2, 3, 1),
                                ops.augment_ingest_image(xb, dtype, ub, policy, p=p).permute(0, 2, 3, 1)])
            assert torch.equal(_bits(pair.permute(0, 2, 3, 1)), _bits(single)), policy
            # p = None is today's path
            assert torch.equal(_bits(ops.augment_ingest_image(xa, dtype, ud, policy)), _bits(ops.augment_ingest_image(xa, dtype, ud, policy, p=_p(1.0, dev))))
    finally:
        ops.set_compute_dtype(torch.float32)


def test_a_null_p_dev_and_a_host_p_are_refused_with_nothing_written():
    dev = _dev()
    x, dy, u = _operands((16, 24))
    xs, dyp, ud = _source(x, "nchw", dev), _padded_dy(dy, torch.float32, dev), u.to(dev)
    n, _, h, w = xs.shape
    out = torch.full((n * h * w * 4,), CANARY, device=dev)
    grad = torch.full((n * h * w * 3,), CANARY, device=dev)
    part = torch.full((n,), CANARY, device=dev)
    lib = L.lib()
    assert lib.sp_augment_ingest_gated(ops.ptr(xs), L.SP_F32, *xs.stride(), ops.ptr(out), n, h, w, 4, ops.ptr(ud), 7, ops.ptr(part), None,
                                       L.SP_F32, ops.stream()) != 0
    assert b"p_dev" in lib.sp_last_error_string()
    assert lib.sp_augment_ingest_bwd_gated(ops.ptr(dyp), 4, ops.ptr(grad), n, h, w, ops.ptr(ud), 7, ops.ptr(part), None, L.SP_F32,
                                           ops.stream()) != 0
    assert b"p_dev" in lib.sp_last_error_string()
    torch.cuda.synchronize()
    for buf in (out, grad, part):
        assert bool((buf == CANARY).all())
    for bad in (0.5, torch.tensor([0.5]), torch.tensor([0.5, 0.5], device=dev), torch.tensor([0.5], device=dev, dtype=torch.float64)):
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image(xs, torch.float32, ud, 7, p=bad)
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image_pair(xs, xs, torch.float32, ud, ud, 7, p=bad)
