"""The geometric augmenting ingest on the GPU, op by op (csrc/augment.hip: THE GEOMETRIC FAMILY; ops.augment_geom_decode and the
table= form of ops.augment_ingest_image / augment_ingest_image_pair) against the float64 restatement of
tests/geom_restated.py.

THE BOUND is geom_restated.forward_bound / backward_bound, per element, derived in that module's docstring and shown to hold for the
fp32 restatement alone by tests/test_geom_host.py; a 16-bit result adds augment_restated.stored_bound's store term.  The apply tests
read the table BACK from the device and give the same table to the reference, so the decode's error stays out of them; the decode is
tested on its own.  Operands are augment_restated.exact_operands (multiples of 2^-8: sum(x) is exact on maps up to 64 x 64).

Shapes: 4 x 4; 16 x 16; 40 x 40 (1600 pixels: no multiple of the block of 256, seven blocks); 64 x 64 (two statistics slices per
direction); 8 x 24 (non-square: no rot90).  Six images per call (geom_restated.end_rows: every flip x k at both ends of the scale and
the rotation range, the identity, one row inside).

THE DECODE'S TOLERANCE on scale and rotate rows.  exp2f, sinf and cosf on the device are not specified to an ulp, so the tolerance is
measured: the largest |device table entry - float64 table entry| over this test's rows was 1.39e-07 on the linear entries (m00 m01 m10
m11; half a unit in the last place of a product of magnitude up to 1.32 is 6e-08) and 1.01e-05 on the offsets (m02 m12 at 64 x 64: sums of
two products of magnitude ~40 each, whose own rounding is 2e-06 apiece); the tolerances are 2x those, tests/test_gpu_fp8.py's margin,
and the linear one must stay below 2^-18 = 3.8e-06 (1e-3 pixel across 256) - asserted."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_restated as A  # noqa: E402
import geom_restated as G  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ids = dict(ids=lambda d: str(d).split(".")[-1] if isinstance(d, torch.dtype) else ("%dx%d" % d if isinstance(d, tuple) else str(d)))
SHAPES = ((4, 4), (16, 16), (40, 40), (64, 64), (8, 24))
LAYOUTS = ("nchw", "channels_last", "strided")
POLICIES = ("", "cutout", "color", "color,cutout")
ALL = 15
CANARY = 1234.5
PAD = 64
LAST = G.LAST
DECODE_LINEAR_MEASURED = 1.39e-07
DECODE_OFFSET_MEASURED = 1.01e-05


def _dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _geom_for(hw, geom):
    return geom if hw[0] == hw[1] else geom & ~G.ROT90


@functools.lru_cache(maxsize=None)
def _operands(hw):
    """x, dy, u, v for one map size: computed once, shared, never written.  o, s, k over their ranges, translations at -r, 0, +r, one
    window at an edge (row 0), v at the ends of its ranges."""
    h, w = hw
    v = G.end_rows()
    n = v.shape[0]
    ry, rx, _, _, ny, nx = ops.augment_geometry(h, w)
    osk = [(-0.5, 0.0, 0.5), (0.4375, 1.9375, 1.4375), (0.0, 1.0, 1.0), (-0.25, 0.5, 0.75), (0.125, 1.5, 1.25), (0.3125, 0.0625, 0.5625)]
    moves = [(-ry, -rx, 0, 0), (ry, rx, ny - 1, nx - 1), (0, 0, ny // 2, nx // 2), (-ry, rx, ny - 1, 0), (ry, 0, 0, nx // 2), (0, -rx, ny // 2, nx - 1)]
    u = torch.tensor([A.u_for(o, s, k, ty, tx, cy, cx, h, w) for (o, s, k), (ty, tx, cy, cx) in zip(osk, moves)], dtype=torch.float32)
    i = SHAPES.index(hw)
    return A.exact_operands((n, 3, h, w), 300 + i), A.exact_operands((n, 3, h, w), 400 + i), u, v


_REF = {}


def _reference(hw, policy, geom, tab):
    """The float64 results and their bounds for one (map, policy, geom) with the device's own table: computed once."""
    key = (hw, policy, geom)
    if key not in _REF:
        x, dy, u, _ = _operands(hw)
        _REF[key] = (tab.clone(), G.forward(x, u, tab, policy), G.forward_bound(x, u, tab, policy),
                     G.backward(dy, u, tab, policy), G.backward_bound(dy, u, tab, policy))
    assert torch.equal(_REF[key][0], tab)          # the decode repeats bit for bit
    return _REF[key][1:]


def _layout(x, layout):
    if layout == "nchw":
        return x.contiguous()
    if layout == "channels_last":
        return x.contiguous(memory_format=torch.channels_last)
    big = torch.full((x.shape[0], 3, x.shape[2] + 2, 2 * x.shape[3] + 3), CANARY, dtype=x.dtype, device=x.device)
    view = big[:, :, 1:-1, 1:-2:2]
    view.copy_(x)
    return view


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


def _run(x_cpu, dy_cpu, u_cpu, tab, policy, dtype, layout="nchw", src_dtype=torch.float32, p=None):
    dev = _dev()
    x = _layout(x_cpu.to(dev, src_dtype), layout).requires_grad_(True)
    y = ops.augment_ingest_image(x, dtype, u_cpu.to(dev), policy, p=p, table=tab.to(dev))
    assert y.dtype == dtype and tuple(y.shape) == (x.shape[0], ops.pad_channels(3, dtype)) + tuple(x.shape[2:]) and ops.is_nhwc(y)
    (dx,) = torch.autograd.grad(y, x, _padded_dy(dy_cpu, dtype, dev))
    assert dx.dtype == src_dtype and dx.shape == x.shape
    torch.cuda.synchronize()
    return y.detach(), dx.detach()


def _check(y, dx, ref, dtype, what):
    want_y, bound_y, want_dx, bound_dx = ref
    assert bool((y[:, 3:] == 0).all()), what                                   # the padding channels
    for got, want, bound, name in ((y[:, :3], want_y, bound_y, "forward"), (dx, want_dx, bound_dx, "backward")):
        err = (got.double().cpu() - want).abs()
        lim = A.stored_bound(want, bound, dtype)
        print("%s %s: max error %.3e, bound at that element %.3e" % (what, name, float(err.max()), float(lim.flatten()[int(err.argmax())])))
        assert bool((err <= lim).all()), (what, name, float((err - lim).max()))


def _decode(hw, geom, u=None, v=None, policy="translation"):
    _, _, u0, v0 = _operands(hw)
    u, v = (u0 if u is None else u), (v0 if v is None else v)
    dev = _dev()
    tab = ops.augment_geom_decode(u.to(dev), v.to(dev), hw[0], hw[1], policy, geom)
    torch.cuda.synchronize()
    return tab.cpu()


# ---- (a) exact cases with hand-written tables --------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 4), (16, 16)], **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_hand_written_exact_tables_equal_the_float64_restatement(dtype, hw):
    """Every flip x k, half-pixel and whole-pixel shifts, L = 2 I, L = I / 2 on multiples of 2^-8: every product and sum is exact in
    fp32, so forward and backward EQUAL the float64 restatement (rounded to the storage type in 16 bit), without and with a window."""
    h, w = hw
    tabs = torch.cat(G.exact_tables(h, w))
    for at, layout in zip(range(0, tabs.shape[0], 5), LAYOUTS):
        tab = tabs[at:at + 5]
        n = tab.shape[0]
        x, dy = A.exact_operands((n, 3, h, w), 500 + at), A.exact_operands((n, 3, h, w), 600 + at)
        u = torch.tensor([A.u_for(h=h, w=w, cy=i, cx=w - i) for i in range(n)], dtype=torch.float32)
        for policy in ("", "cutout"):
            y, dx = _run(x, dy, u, tab, policy, dtype, layout)
            want_y, want_dx = G.forward(x, u, tab, policy), G.backward(dy, u, tab, policy)
            assert bool((y[:, 3:] == 0).all())
            assert torch.equal(_bits(y[:, :3].cpu()), _bits(want_y.float().to(dtype))), (policy, at)
            assert torch.equal(_bits(dx.cpu()), _bits(want_dx.float().to(dtype).float())), (policy, at)
            assert float(want_y.abs().max()) > 0 and float(want_dx.abs().max()) > 0


# ---- (b) decode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (64, 64), (8, 24)], **ids)
def test_decode_rows_without_scale_and_rotate_are_bit_exact(hw):
    """Flip, rot90 and translation rows against the host restatement: uniforms as they fall, both sides of every bin edge, 0 and
    1 - 2^-24; with and without the translation bit; 200 rows, so more than one block of the decode launch."""
    h, w = hw
    g = torch.Generator().manual_seed(h)
    n = 200
    u, v = torch.rand(n, 8, generator=g), torch.rand(n, 4, generator=g)
    half, quarter = torch.tensor(0.5), torch.tensor([0.25, 0.5, 0.75])
    v[:4, 0] = torch.tensor([0.0, float(torch.nextafter(half, torch.tensor(0.0))), 0.5, LAST])
    v[:8, 1] = torch.cat([torch.tensor([0.0, LAST]), quarter, torch.nextafter(quarter, torch.tensor(0.0))])
    u[:2, 3:5] = torch.tensor([[0.0, LAST], [LAST, 0.0]])
    for geom in (G.XFLIP, G.ROT90, G.XFLIP | G.ROT90):
        if _geom_for(hw, geom) != geom:
            continue
        for policy in ("translation", "color,cutout"):
            got = _decode(hw, geom, u, v, policy)
            want = ops.augment_geom_table(u, v, h, w, policy, geom)
            assert torch.equal(got, want), (geom, policy)
            assert set(got[:, [0, 1, 3, 4]].abs().flatten().tolist()) == {0.0, 1.0} and bool((got[:, 6:] == 0).all())
            if geom & G.ROT90:
                assert len({tuple(r) for r in got[:, [0, 1, 3, 4]].tolist()}) == (8 if geom & G.XFLIP else 4)


@pytest.mark.parametrize("hw", [(16, 16), (64, 64), (8, 24)], **ids)
def test_decode_scale_and_rotate_rows_against_float64(hw):
    """See the module docstring: the measured error, printed, against twice the recorded measurement."""
    h, w = hw
    g = torch.Generator().manual_seed(7 * h)
    n = 200
    u, v = torch.rand(n, 8, generator=g), torch.rand(n, 4, generator=g)
    v[:6] = G.end_rows()
    v[6:8, 2:] = torch.tensor([[0.0, 0.0], [LAST, LAST]])
    worst = [0.0, 0.0]
    for geom in (G.SCALE, G.ROTATE, G.SCALE | G.ROTATE, ALL):
        geom = _geom_for(hw, geom)
        got = _decode(hw, geom, u, v).double()
        want = ops.augment_geom_table(u, v, h, w, "translation", geom, torch.float64)
        err = (got - want).abs()
        worst = [max(worst[0], float(err[:, [0, 1, 3, 4]].max())), max(worst[1], float(err[:, [2, 5]].max()))]
        assert bool((got[:, 6:] == 0).all())
    print("decode %dx%d: largest error %.3e on the linear entries, %.3e on the offsets" % (h, w, worst[0], worst[1]))
    assert 2 * DECODE_LINEAR_MEASURED < 2.0 ** -18
    assert worst[0] <= 2 * DECODE_LINEAR_MEASURED and worst[1] <= 2 * DECODE_OFFSET_MEASURED


# ---- (c) apply, (d) adjoint ---------------------------------------------------------------------------------------------------
def _apply_case(hw, policy, geom, dtype, layout, src_dtype=torch.float32):
    x, dy, u, _ = _operands(hw)
    tab = _decode(hw, geom)
    ref = _reference(hw, policy, geom, tab)
    y, dx = _run(x, dy, u, tab, policy, dtype, layout, src_dtype)
    _check(y, dx, ref, dtype, (policy, geom, str(dtype), layout, hw))
    if dtype == torch.float32:
        # (d) the adjoint from the GPU's own outputs: <T(x), dy> = <x, T'(dy)> up to what each side may be off by.  With color T is
        # affine, not linear: its value at 0 goes to the left (from the float64 restatement: it is a constant of the case)
        y0 = G.forward(torch.zeros_like(x), u, tab, policy) if "color" in policy else 0.0
        terms = (y[:, :3].double().cpu() - y0) * dy.double()
        lhs, size = float(terms.sum()), float(terms.abs().sum())
        rhs = float((x.double() * dx.double().cpu()).sum())
        slack = float((ref[1] * dy.double().abs()).sum() + (ref[3] * x.double().abs()).sum())
        print("adjoint %s: |lhs - rhs| = %.3e, slack %.3e, sum |terms| = %.3e" % ((policy, geom, hw), abs(lhs - rhs), slack, size))
        assert abs(lhs - rhs) <= slack and slack <= 1e-2 * size          # (the slack is a worst-case sum of the per-element bounds)


@pytest.mark.parametrize("geom", range(1, 16))
def test_every_combination_of_parts_within_the_bound(geom):
    """All 15 subsets of the four parts at both ends of each range, with color and cutout and with neither, fp32 (the adjoint check
    included) - on 16 x 16, and on 8 x 24 where the subset has no rot90."""
    for hw in ((16, 16), (8, 24)):
        if _geom_for(hw, geom) != geom:
            continue
        for policy, layout in (("color,cutout", "nchw"), ("", "strided")):
            _apply_case(hw, policy, geom, torch.float32, layout)


@pytest.mark.parametrize("hw", SHAPES, **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_all_parts_on_every_shape_storage_type_and_layout(dtype, hw):
    geom = _geom_for(hw, ALL)
    ops.set_compute_dtype(dtype)
    try:
        for i, policy in enumerate(POLICIES):
            _apply_case(hw, policy, geom, dtype, LAYOUTS[i % 3])
        _apply_case(hw, "color,cutout", geom, dtype, "channels_last")
        if dtype != torch.float32:          # the source in the compute type (the operands are exact in it)
            _apply_case(hw, "color,cutout", geom, dtype, "nchw", src_dtype=dtype)
    finally:
        ops.set_compute_dtype(torch.float32)


# ---- (e) structure and gate ---------------------------------------------------------------------------------------------------
class _Run:
    """One forward and one backward call through the C ABI on windows carved out of canary-filled buffers.  entry: "geom" (p: a device
    tensor or None for a NULL p_dev) or "plain".  The partials' interior is NaN on entry: a result that read a value nobody wrote is NaN."""

    def __init__(self, xs, dyp, u, tab, policy, dtype, entry, p=None):
        dev = xs.device
        n, _, h, w = xs.shape
        cp, esz = ops.pad_channels(3, dtype), torch.empty((), dtype=dtype).element_size()
        self.out = torch.full((PAD + n * h * w * cp + PAD,), CANARY, dtype=dtype, device=dev)
        self.grad = torch.full((PAD + n * h * w * 3 + PAD,), CANARY, dtype=dtype, device=dev)
        self.parts = [torch.full((PAD + n * ops.augment_geom_slices(h, w, b) + PAD,), CANARY, dtype=torch.float32, device=dev) for b in (False, True)]
        self.table = torch.full((PAD + n * 8 + PAD,), CANARY, dtype=torch.float32, device=dev)
        self.table[PAD:-PAD] = tab.flatten()
        for part in self.parts:
            part[PAD:-PAD] = float("nan")
        at = lambda t, size: ctypes.c_void_p(t.data_ptr() + PAD * size)      # noqa: E731
        dt, st = ops.sp_dtype(dtype), ops.stream()
        if entry == "plain":
            L.call("sp_ingest_image", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, 3, h, w, cp, None, None, dt, st)
            L.call("sp_ingest_image_bwd", ops.ptr(dyp), cp, at(self.grad, esz), 3, n * h * w, None, dt, st)
        else:
            L.call("sp_augment_geom_ingest", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   at(self.table, 4), at(self.parts[0], 4), ops.ptr(p), dt, st)
            L.call("sp_augment_geom_ingest_bwd", ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy, at(self.table, 4),
                   at(self.parts[1], 4), ops.ptr(p), dt, st)
        torch.cuda.synchronize()
        for buf in [self.out, self.grad, self.table] + self.parts:
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), entry
        assert torch.equal(self.table[PAD:-PAD].cpu(), tab.flatten().cpu())              # the apply entries only read the table
        self.y = _bits(self.out[PAD:-PAD].view(n, h, w, cp))               # (n, h, w, cp) bits
        self.dx = _bits(self.grad[PAD:-PAD].view(n, h, w, 3))


@pytest.mark.parametrize("hw", [(40, 40), (64, 64), (8, 24)], **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_canaries_nan_partials_repeat_runs_and_the_gate(dtype, hw):
    """Through the C ABI: nothing outside the buffers is written, no result leans on a partial nobody wrote, two runs agree to the bit,
    a NULL p_dev equals p = 1; with u7 on either side of p = 0.5 (0.5 itself is dead: the compare is strict) the dead images EQUAL the
    plain ingest and the live ones the ungated result, forward and backward; the translation bit of `policy` changes nothing."""
    dev = _dev()
    x, dy, u, _ = _operands(hw)
    geom = _geom_for(hw, ALL)
    tab = _decode(hw, geom).to(dev)
    u = u.clone()
    u[:, 7] = torch.tensor([0.25, 0.75, 0.5, float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0))), LAST, 0.0])
    live, dead = [0, 3, 5], [1, 2, 4]
    ud, dyp = u.to(dev), _padded_dy(dy, dtype, dev)
    for policy, layout in ((5, "strided"), (4, "channels_last")):
        xs = _layout(x.to(dev), layout)
        ungated, plain = _Run(xs, dyp, ud, tab, policy, dtype, "geom"), _Run(xs, dyp, ud, tab, policy, dtype, "plain")
        gated = _Run(xs, dyp, ud, tab, policy, dtype, "geom", _p(0.5, dev))
        one, again = _Run(xs, dyp, ud, tab, policy, dtype, "geom", _p(1.0, dev)), _Run(xs, dyp, ud, tab, policy, dtype, "geom", _p(0.5, dev))
        zero, moved = _Run(xs, dyp, ud, tab, policy, dtype, "geom", _p(0.0, dev)), _Run(xs, dyp, ud, tab, policy | 2, dtype, "geom")
        for name in ("y", "dx"):
            got = getattr(gated, name)
            assert torch.equal(got[live], getattr(ungated, name)[live]), (name, "live")
            assert torch.equal(got[dead], getattr(plain, name)[dead]), (name, "dead")
            for i in range(x.shape[0]):
                assert not torch.equal(getattr(ungated, name)[i], getattr(plain, name)[i]), (name, i)
            assert torch.equal(getattr(one, name), getattr(ungated, name)), (name, "p = 1 against a NULL p_dev")
            assert torch.equal(getattr(zero, name), getattr(plain, name)), (name, "p = 0")
            assert torch.equal(getattr(again, name), getattr(gated, name)), (name, "second run")
            assert torch.equal(getattr(moved, name), getattr(ungated, name)), (name, "the translation bit")
        assert bool((gated.y[..., 3:] == 0).all()) and bool((ungated.y[..., 3:] == 0).all())
        for run in (gated, ungated):
            assert not bool(torch.isnan(run.out[PAD:-PAD].float()).any()) and not bool(torch.isnan(run.grad[PAD:-PAD].float()).any())
        for part in ungated.parts:                           # every partial written with color, none without
            inner = part[PAD:-PAD]
            assert bool(torch.isfinite(inner).all()) if policy & 1 else bool(torch.isnan(inner).all())
        # the ops carry table and gate to the same entries, forward and backward
        y, dx = _run(x, dy, u, tab.cpu(), policy, dtype, layout, p=_p(0.5, dev))
        assert torch.equal(_bits(y.permute(0, 2, 3, 1)), gated.y) and torch.equal(_bits(dx.to(dtype).permute(0, 2, 3, 1)), gated.dx)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_pair_form_equals_two_single_calls(dtype):
    dev = _dev()
    hw = (40, 40)
    x, _, u, _ = _operands(hw)
    tab = _decode(hw, ALL).to(dev)
    xa, xb = x.to(dev), x.flip(0).to(dev).contiguous(memory_format=torch.channels_last)
    ua, ub = u.to(dev), u.flip(0).contiguous().to(dev)
    ta, tb = tab, tab.flip(0).contiguous()
    for policy in ("color,cutout", "cutout"):
        for p in (None, _p(0.5, dev)):
            pair = ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, policy, p=p, table_a=ta, table_b=tb)
            assert not pair.requires_grad and tuple(pair.shape) == (2 * x.shape[0], ops.pad_channels(3, dtype), 40, 40)
            single = torch.cat([ops.augment_ingest_image(xa, dtype, ua, policy, p=p, table=ta).permute(0, 2, 3, 1),
                                ops.augment_ingest_image(xb, dtype, ub, policy, p=p, table=tb).permute(0, 2, 3, 1)]).permute(0, 3, 1, 2)
            assert torch.equal(_bits(pair), _bits(single)), policy
    with pytest.raises(L.SempyrError):
        ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, "cutout", table_a=ta)


def test_bad_arguments_raise_and_launch_nothing():
    dev = _dev()
    u, v = torch.zeros(2, 8, device=dev), torch.zeros(2, 4, device=dev)
    img = torch.zeros(2, 3, 8, 8, device=dev)
    good = torch.zeros(2, 8, device=dev)
    for bad in (torch.zeros(3, 8, device=dev), torch.zeros(2, 6, device=dev), torch.zeros(2, 8), torch.zeros(2, 8, device=dev, dtype=torch.float64),
                torch.zeros(2, 16, device=dev)[:, ::2]):
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image(img, torch.float32, u, "color", table=bad)
    for bad_u, bad_v, geom, hw in ((u, torch.zeros(2, 3, device=dev), 1, (8, 8)), (u, torch.zeros(3, 4, device=dev), 1, (8, 8)), (u, v, 0, (8, 8)),
                                   (u, v, 2, (8, 12)), (u.double(), v, 1, (8, 8))):
        out = torch.full((2, 8), CANARY, device=dev)
        with pytest.raises(L.SempyrError):
            ops.augment_geom_decode(bad_u, bad_v, hw[0], hw[1], "translation", geom, out=out)
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())
    with pytest.raises(L.SempyrError):
        ops.augment_geom_decode(u, v, 8, 8, "translation", "flip")
    assert ops.augment_geom_decode(u, v, 8, 8, "translation", "xflip", out=good) is good
