"""The augmenting ingest on the GPU, op by op (csrc/augment.hip; ops.augment_ingest_image / augment_ingest_image_pair) against the
float64 restatement of tests/augment_restated.py.

THE BOUND is augment_restated.forward_bound / backward_bound, per element: the first-order propagation of U = 2^-24 per fp32 operation
through the transform's expressions, times 1 + 2^-10, derived in that module's docstring and shown to hold for the fp32 restatement
alone by tests/test_augment_host.py.  It needs the per-image sums to be exact, so the operands are multiples of 2^-8 in [-1, 1) on maps
of at most 64 x 64 and o, s, k are multiples of 2^-4 (augment_restated.bound_cases: translations at -r, 0, +r on both axes, cutout
centres at 0, the middle and the last value).  A result stored in bfloat16 / float16 adds half a unit in the last place of the
stored value (augment_restated.stored_bound).  Where the policy has no color part the kernels only move data and the comparison is
for equality.

Shapes: 16 x 24; 20 x 20 (r = 3, q = 10); 48 x 64, which is 9216 source elements = two forward partials of 8192 (the second a
quarter full) and 3072 pixels = two backward partials of 2048; 64 x 64 (two whole backward partials)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_restated as A  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
COLOR_POLICIES = ("color", "color,translation", "color,cutout", "color,translation,cutout")
MOVE_POLICIES = ("translation", "cutout", "translation,cutout")
SHAPES = tuple(shape[2:] for shape, _ in A.bound_cases())
CANARY = 1234.5
LAST = 1.0 - 2.0 ** -24


def _dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(hw):
    """Operands, uniforms and the float64 results with their bounds for one map size: computed once, shared, never written."""
    (shape, u), = [c for c in A.bound_cases() if c[0][2:] == hw]
    i = SHAPES.index(hw)
    x, dy = A.exact_operands(shape, 100 + i), A.exact_operands(shape, 200 + i)
    ref = {}
    for policy in COLOR_POLICIES + MOVE_POLICIES:
        ref[policy] = (A.forward(x, u, policy), A.forward_bound(x, u, policy), A.backward(dy, u, policy), A.backward_bound(dy, u, policy))
    return x, dy, u, ref


def _layout(x, layout):
    """The source as the kernel may meet it: NCHW-contiguous, channels-last (both one dense run per image), or a strided view."""
    if layout == "nchw":
        return x.contiguous()
    if layout == "channels_last":
        return x.contiguous(memory_format=torch.channels_last)
    big = torch.full((x.shape[0], 3, x.shape[2] + 2, 2 * x.shape[3] + 3), CANARY, dtype=x.dtype, device=x.device)
    view = big[:, :, 1:-1, 1:-2:2]
    view.copy_(x)
    return view


def _padded_dy(dy, dtype, dev):
    """dy on the 3 real channels of a padded NHWC tensor whose padding channels hold junk the backward must not read into its sums."""
    n, _, h, w = dy.shape
    cp = ops.pad_channels(3, dtype)
    full = ops.nhwc_empty(n, cp, h, w, dtype, dev)
    full.fill_(7.0)
    full[:, :3] = dy.to(dev, dtype)
    return full


def _run(x_cpu, dy_cpu, u_cpu, policy, dtype, layout="nchw", src_dtype=torch.float32):
    dev = _dev()
    x = _layout(x_cpu.to(dev, src_dtype), layout).requires_grad_(True)
    u = u_cpu.to(dev)
    y = ops.augment_ingest_image(x, dtype, u, policy)
    assert y.dtype == dtype and tuple(y.shape) == (x.shape[0], ops.pad_channels(3, dtype)) + tuple(x.shape[2:]) and ops.is_nhwc(y)
    (dx,) = torch.autograd.grad(y, x, _padded_dy(dy_cpu, dtype, dev))
    assert dx.dtype == src_dtype and dx.shape == x.shape
    torch.cuda.synchronize()
    return y.detach(), dx.detach()


def _bits(t):
    t = t.contiguous()                                   # logical (n, c, h, w) order whatever the strides were
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _check(y, dx, ref, dtype, what):
    want_y, bound_y, want_dx, bound_dx = ref
    assert bool((y[:, 3:] == 0).all()), what                                   # the padding channels
    for got, want, bound, name in ((y[:, :3], want_y, bound_y, "forward"), (dx, want_dx, bound_dx, "backward")):
        err = (got.double().cpu() - want).abs()
        lim = A.stored_bound(want, bound, dtype)
        worst = float((err - lim).max())
        print("%s %s: max error %.3e, bound at that element %.3e" % (what, name, float(err.max()), float(lim.flatten()[int(err.argmax())])))
        assert bool((err <= lim).all()), (what, name, worst)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", ["nchw", "channels_last", "strided"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_color_policies_within_the_rounding_bound_of_float64(dtype, layout, hw):
    x, dy, u, ref = _case(hw)
    ops.set_compute_dtype(dtype)
    try:
        for policy in COLOR_POLICIES:
            y, dx = _run(x, dy, u, policy, dtype, layout)
            _check(y, dx, ref[policy], dtype, (policy, str(dtype), layout, hw))
    finally:
        ops.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_source_in_the_compute_type(dtype):
    """The source may be in the compute type (16-byte loads of 8 elements in the statistics launch); the operands are exact in it."""
    x, dy, u, ref = _case((48, 64))
    for layout in ("nchw", "channels_last", "strided"):
        y, dx = _run(x, dy, u, "color,translation,cutout", dtype, layout, src_dtype=dtype)
        _check(y, dx, ref["color,translation,cutout"], dtype, ("16-bit source", str(dtype), layout))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_random_uniforms_within_the_bound(dtype):
    """o, s, k as they fall (no multiples of 2^-4): the sums are exact whatever o is, and the bound charges every rounding, that of
    1 - k and 1 - s included.  34 images: 32 random rows of u, all zeros, all 1 - 2^-24."""
    g = torch.Generator().manual_seed(5)
    n, h, w = 34, 20, 20
    u = torch.rand(n, 8, generator=g)
    u[32], u[33] = 0.0, LAST
    x, dy = A.exact_operands((n, 3, h, w), 6), A.exact_operands((n, 3, h, w), 7)
    policy = "color,translation,cutout"
    ref = (A.forward(x, u, policy), A.forward_bound(x, u, policy), A.backward(dy, u, policy), A.backward_bound(dy, u, policy))
    y, dx = _run(x, dy, u, policy, dtype)
    _check(y, dx, ref, dtype, ("random u", str(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_translation_and_cutout_alone_move_data_bit_for_bit(dtype):
    """Without color there is one launch per direction and no arithmetic: every value arrives as the plain ingest would store it
    (fp32 -> 16-bit by round-to-nearest-even, as torch converts), zeros elsewhere - forward and backward, for operands that are NOT
    exact in 16 bits and uniforms as they fall (the decoding of t and c on the device against ops.augment_decode), u = 0 and
    u = 1 - 2^-24 included."""
    g = torch.Generator().manual_seed(9)
    for (h, w), layout in (((16, 24), "nchw"), ((20, 20), "channels_last"), ((48, 64), "strided")):
        n = 34
        u = torch.rand(n, 8, generator=g)
        u[32], u[33] = 0.0, LAST
        x = torch.randn(n, 3, h, w, generator=g)
        dy = torch.randn(n, 3, h, w, generator=g).to(dtype).float()             # dy arrives in the compute type
        for policy in MOVE_POLICIES:
            y, dx = _run(x, dy, u, policy, dtype, layout)
            want_y = A.forward(x.to(dtype), u, policy, dtype)
            want_dx = A.backward(dy, u, policy, torch.float32)
            assert bool((y[:, 3:] == 0).all())
            assert torch.equal(_bits(y[:, :3].cpu()), _bits(want_y)), (policy, h, w)
            assert torch.equal(_bits(dx.cpu()), _bits(want_dx)), (policy, h, w)
    x, dy, u, ref = _case((64, 64))
    for policy in MOVE_POLICIES:
        y, dx = _run(x, dy, u, policy, dtype)
        assert torch.equal(y[:, :3].double().cpu(), ref[policy][0]) and torch.equal(dx.double().cpu(), ref[policy][2])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_pair_form_equals_two_single_calls_and_runs_repeat_bit_for_bit(dtype):
    dev = _dev()
    x, dy, u, _ = _case((48, 64))
    xa, xb = x.to(dev), x.flip(0).to(dev).contiguous(memory_format=torch.channels_last)
    ua, ub = u.to(dev), u.flip(1).contiguous().to(dev)
    for policy in ("color,translation,cutout", "translation,cutout", "color"):
        pair = ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, policy)
        assert not pair.requires_grad and tuple(pair.shape) == (2 * x.shape[0], ops.pad_channels(3, dtype), 48, 64)
        single = torch.cat([ops.augment_ingest_image(xa, dtype, ua, policy).permute(0, 2, 3, 1),
                            ops.augment_ingest_image(xb, dtype, ub, policy).permute(0, 2, 3, 1)]).permute(0, 3, 1, 2)
        assert torch.equal(_bits(pair), _bits(single)), policy
        runs = [_run(x, dy, u, policy, dtype) for _ in range(2)]
        assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), policy


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_canaries_around_the_outputs_and_the_partials_are_intact(dtype):
    """The entry points called on windows carved out of canary-filled buffers: the padded output, the partials (two per image and
    direction at 48 x 64) and the gradient are written, nothing in front of or behind them is; the results are those of the ops."""
    dev = _dev()
    x, dy, u, _ = _case((48, 64))
    n, _, h, w = x.shape
    cp = ops.pad_channels(3, dtype)
    esz = torch.empty((), dtype=dtype).element_size()
    xs, ud = x.to(dev), u.to(dev)
    dyp = _padded_dy(dy, dtype, dev)
    for policy in ("color,translation,cutout", "translation,cutout"):
        mask = ops.augment_policy(policy)
        y_api, dx_api = _run(x, dy, u, policy, dtype)
        pad = 64
        out = torch.full((pad + n * h * w * cp + pad,), CANARY, dtype=dtype, device=dev)
        grad = torch.full((pad + n * h * w * 3 + pad,), CANARY, dtype=dtype, device=dev)
        parts = [torch.full((pad + n * ops.augment_slices(h, w, b) + pad,), CANARY, dtype=torch.float32, device=dev) for b in (False, True)]
        at = lambda t, size: ctypes.c_void_p(t.data_ptr() + pad * size)      # noqa: E731
        L.call("sp_augment_ingest", ops.ptr(xs), L.SP_F32, *xs.stride(), at(out, esz), n, h, w, cp, ops.ptr(ud), mask, at(parts[0], 4),
               ops.sp_dtype(dtype), ops.stream())
        L.call("sp_augment_ingest_bwd", ops.ptr(dyp), cp, at(grad, esz), n, h, w, ops.ptr(ud), mask, at(parts[1], 4), ops.sp_dtype(dtype),
               ops.stream())
        torch.cuda.synchronize()
        for buf in [out, grad] + parts:
            assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), policy
        for part in parts:                                   # every partial written with color, none without
            inner = part[pad:-pad]
            assert bool((inner != CANARY).all()) if mask & 1 else bool((inner == CANARY).all()), policy
        got_y = out[pad:-pad].view(n, h, w, cp).permute(0, 3, 1, 2)
        got_dx = grad[pad:-pad].view(n, h, w, 3).permute(0, 3, 1, 2)
        assert torch.equal(_bits(got_y), _bits(y_api)), policy
        assert torch.equal(got_dx.float(), dx_api), policy


def test_bad_arguments_raise():
    dev = _dev()
    u = torch.zeros(2, 8, device=dev)
    img = torch.zeros(2, 3, 8, 8, device=dev)
    for bad_img, bad_u in ((torch.zeros(2, 4, 8, 8, device=dev), u), (torch.zeros(2, 1, 8, 8, device=dev), u), (torch.zeros(3, 8, 8, device=dev), u),
                           (img, torch.zeros(3, 8, device=dev)), (img, torch.zeros(2, 7, device=dev)), (img, torch.zeros(2, 8)),
                           (img, torch.zeros(2, 8, device=dev, dtype=torch.float64))):
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image(bad_img, torch.float32, bad_u, "color")
    with pytest.raises(L.SempyrError):
        ops.augment_ingest_image(img, torch.float32, u, "color,mixup")
    with pytest.raises(L.SempyrError):
        ops.augment_ingest_image_pair(img, torch.zeros(2, 3, 8, 4, device=dev), torch.float32, u, u, "color")
