"""ADA's color group in the augmenting ingest on the GPU, op by op (csrc/augment.hip: THE COLOR MATRIX; ops.augment_cmat_decode and the
ctable= form of ops.augment_ingest_image / augment_ingest_image_pair) against the float64 restatement of
tests/cmat_restated.py, in the plain family (no affine table) and in the geometric one.

THE BOUND is cmat_restated.forward_bound / backward_bound, per element, derived in that module's docstring and shown to hold for the
fp32 restatement alone by tests/test_cmat_host.py; a 16-bit result adds augment_restated.stored_bound's store term.  The apply tests
read the ctable (and the affine table) BACK from the device and give the same tables to the reference, so the decodes' errors stay out
of them; the decode is tested on its own.  Operands are augment_restated.exact_operands (multiples of 2^-8: sum(x) is exact on maps up
to 64 x 64).

Shapes: 4 x 4; 16 x 16; 40 x 40 (1600 pixels: no multiple of the block of 256, partial 16 x 16 tiles); 64 x 64 (two forward partials
per image); 8 x 24 (non-square, partial tiles: no rot90).  Six images per call (cmat_restated.end_rows: every normal at +-5.77, theta at
-pi and just below pi, z7 on either side of 0.5, the identity, one row inside; geom_restated.end_rows for v).

THE DECODE'S TOLERANCE on rows with brightness, contrast, hue or saturation.  logf, cosf, sinf and exp2f on the device are not specified
to an ulp, so the tolerance is measured: the largest |device entry - float64 entry| over this test's rows, relative to the row's largest
entry (at least 1: entries reach c s = 400 at the ends of the ranges), was 3.26e-07 - five units in the last place of that entry (the
exponent given to exp2f is a normal of magnitude up to 5.77 whose own last place is 4.8e-07, times log 2, and the factors c and s
multiply); the tolerance is 2x that, the margin of tests/test_gpu_geom.py's decode."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_restated as A  # noqa: E402
import cmat_restated as C  # noqa: E402
import geom_restated as G  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ids = dict(ids=lambda d: str(d).split(".")[-1] if isinstance(d, torch.dtype) else ("%dx%d" % d if isinstance(d, tuple) else str(d)))
SHAPES = ((4, 4), (16, 16), (40, 40), (64, 64), (8, 24))
LAYOUTS = ("nchw", "channels_last", "strided")
GEOM_ALL = 15
CANARY = 1234.5
PAD = 64
LAST = C.LAST
DECODE_MEASURED = 3.26e-07


def _dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _geom_for(hw, geom):
    return geom if hw[0] == hw[1] else geom & ~G.ROT90


@functools.lru_cache(maxsize=None)
def _operands(hw):
    """x, dy, u, v, z for one map size: computed once, shared, never written.  o, s, k over their ranges, translations at -r, 0, +r, one
    window at an edge (row 0), v and z at the ends of their ranges."""
    h, w = hw
    v, z = G.end_rows(), C.end_rows()
    n = z.shape[0]
    ry, rx, _, _, ny, nx = ops.augment_geometry(h, w)
    osk = [(-0.5, 0.0, 0.5), (0.4375, 1.9375, 1.4375), (0.0, 1.0, 1.0), (-0.25, 0.5, 0.75), (0.125, 1.5, 1.25), (0.3125, 0.0625, 0.5625)]
    moves = [(-ry, -rx, 0, 0), (ry, rx, ny - 1, nx - 1), (0, 0, ny // 2, nx // 2), (-ry, rx, ny - 1, 0), (ry, 0, 0, nx // 2), (0, -rx, ny // 2, nx - 1)]
    u = torch.tensor([A.u_for(o, s, k, ty, tx, cy, cx, h, w) for (o, s, k), (ty, tx, cy, cx) in zip(osk, moves)], dtype=torch.float32)
    i = SHAPES.index(hw)
    return A.exact_operands((n, 3, h, w), 700 + i), A.exact_operands((n, 3, h, w), 800 + i), u, v, z


def _decode(z, cmat):
    ct = ops.augment_cmat_decode(z.to(_dev()), cmat)
    torch.cuda.synchronize()
    return ct.cpu()


@functools.lru_cache(maxsize=None)
def _tables(hw, geom, cmat):
    """The device's own tables for the shared operands: (affine table or None, ctable), read back once."""
    _, _, u, v, z = _operands(hw)
    tab = None
    if geom:
        tab = ops.augment_geom_decode(u.to(_dev()), v.to(_dev()), hw[0], hw[1], "translation", geom).cpu()
    return tab, _decode(z, cmat)


_REF = {}


def _reference(hw, policy, geom, cmat):
    """The float64 results and their bounds for one (map, policy, geom, cmat) with the device's own tables: computed once."""
    key = (hw, policy, geom, cmat)
    if key not in _REF:
        x, dy, u, _, _ = _operands(hw)
        tab, ct = _tables(hw, geom, cmat)
        _REF[key] = (C.forward(x, u, ct, policy, tab), C.forward_bound(x, u, ct, policy, tab),
                     C.backward(dy, u, ct, policy, tab), C.backward_bound(dy, u, ct, policy, tab),
                     C.forward(torch.zeros_like(x), u, ct, policy, tab))
    return _REF[key]


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


def _run(x_cpu, dy_cpu, u_cpu, ct, tab, policy, dtype, layout="nchw", src_dtype=torch.float32, p=None):
    dev = _dev()
    x = _layout(x_cpu.to(dev, src_dtype), layout).requires_grad_(True)
    kw = {} if ct is None else {"ctable": ct.to(dev)}
    y = ops.augment_ingest_image(x, dtype, u_cpu.to(dev), policy, p=p, table=None if tab is None else tab.to(dev), **kw)
    assert y.dtype == dtype and tuple(y.shape) == (x.shape[0], ops.pad_channels(3, dtype)) + tuple(x.shape[2:]) and ops.is_nhwc(y)
    (dx,) = torch.autograd.grad(y, x, _padded_dy(dy_cpu, dtype, dev))
    assert dx.dtype == src_dtype and dx.shape == x.shape
    torch.cuda.synchronize()
    return y.detach(), dx.detach()


def _check(y, dx, ref, dtype, what):
    want_y, bound_y, want_dx, bound_dx = ref[:4]
    assert bool((y[:, 3:] == 0).all()), what                                   # the padding channels
    for got, want, bound, name in ((y[:, :3], want_y, bound_y, "forward"), (dx, want_dx, bound_dx, "backward")):
        err = (got.double().cpu() - want).abs()
        lim = A.stored_bound(want, bound, dtype)
        print("%s %s: max error %.3e, bound at that element %.3e" % (what, name, float(err.max()), float(lim.flatten()[int(err.argmax())])))
        assert bool((err <= lim).all()), (what, name, float((err - lim).max()))


# ---- (a) decode ---------------------------------------------------------------------------------------------------------------------
def _decode_rows(seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(200, 8, generator=g)          # more than one block of the decode launch
    z[:6] = C.end_rows()
    half = torch.tensor(0.5)
    z[6:11, 7] = torch.tensor([0.0, float(torch.nextafter(half, torch.tensor(0.0))), 0.5, float(torch.nextafter(half, torch.tensor(1.0))), LAST])
    z[11:15, :6] = torch.tensor([[0.0] * 6, [LAST] * 6, [LAST, 0.5] * 3, [0.0, LAST] * 3])
    z[15:17, 6] = torch.tensor([0.0, LAST])
    return z


def test_decode_rows_without_a_random_factor_are_bit_exact():
    """Luma flip alone (no hue, contrast, saturation, brightness: nothing goes through libm) against the host restatement, z7 on both
    sides of 0.5: the rows are I or I - 2 J / 3 rounded once, offsets 0."""
    z = _decode_rows(1)
    got = _decode(z, C.LUMAFLIP)
    want = ops.augment_cmat_table(z, C.LUMAFLIP)
    assert torch.equal(_bits(got), _bits(want))
    assert len({tuple(r) for r in got.tolist()}) == 2 and bool((got[:, [3, 7, 11]] == 0).all())
    flipped = got[z[:, 7] < 0.5]
    assert flipped.shape[0] > 50 and float((C.matrix(flipped.double())[0] - (torch.eye(3, dtype=torch.float64) - 2.0 / 3.0)).abs().max()) <= 2.0 ** -24
    # and into a buffer the caller brings: nothing outside the n x 12 floats is written
    dev = _dev()
    buf = torch.full((PAD + 200 * 12 + PAD,), CANARY, device=dev)
    out = buf[PAD:-PAD].view(200, 12)
    assert ops.augment_cmat_decode(z.to(dev), "lumaflip", out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got) and bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def test_decode_rows_with_random_factors_against_float64():
    """See the module docstring: the measured error, printed, against twice the recorded measurement - all 30 other subsets.  Rows
    with brightness and / or contrast alone are exactly diagonal on the device too."""
    z = _decode_rows(2)
    worst = 0.0
    for cmat in range(1, 32):
        if cmat == C.LUMAFLIP:
            continue
        got = _decode(z, cmat)
        want = ops.augment_cmat_table(z, cmat, torch.float64)
        assert bool(torch.isfinite(got).all())
        err = float(((got.double() - want).abs().max(dim=1).values / want.abs().max(dim=1).values.clamp(min=1.0)).max())
        worst = max(worst, err)
        Lm, t = C.matrix(got)
        assert torch.equal(t[:, 0], t[:, 1]) and torch.equal(t[:, 0], t[:, 2])
        if not cmat & ~(C.BRIGHTNESS | C.CONTRAST):
            c = Lm[:, 0, 0]
            assert torch.equal(Lm, torch.diag_embed(torch.stack([c, c, c], dim=1)))
        if not cmat & C.BRIGHTNESS:
            assert bool((t == 0).all())
    print("decode: largest error relative to the row's largest entry %.3e" % worst)
    assert worst <= 2 * DECODE_MEASURED


# ---- (b) exact cases with hand-written tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 4), (16, 16)], **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_hand_written_exact_ctables_equal_the_float64_restatement(dtype, hw):
    """The six channel permutations, diag(2, 0.5, -1) with offsets (0.25, -0.5, 1) and a full matrix of eighths on multiples of 2^-8:
    every product and sum is exact in fp32, so forward and backward EQUAL the float64 restatement (rounded to the storage type in 16
    bit) - in the plain family with translation and window, and in the geometric family with section 16's exact tables."""
    h, w = hw
    cts = torch.cat(C.exact_tables())
    n = cts.shape[0]
    tabs = torch.cat(G.exact_tables(h, w))
    x, dy = A.exact_operands((n, 3, h, w), 510), A.exact_operands((n, 3, h, w), 610)
    ry, rx = ops.augment_geometry(h, w)[:2]
    u = torch.tensor([A.u_for(h=h, w=w, ty=(i % 3 - 1) * ry, tx=(1 - i % 3) * rx, cy=i % (h + 1), cx=(w - i) % (w + 1)) for i in range(n)],
                     dtype=torch.float32)
    cases = [(None, cts, "nchw"), (tabs[:n], cts, "channels_last"), (tabs[-n:], cts.roll(3, 0), "strided")]
    for tab, ct, layout in cases:
        for policy in ("", "translation,cutout"):
            y, dx = _run(x, dy, u, ct, tab, policy, dtype, layout)
            want_y, want_dx = C.forward(x, u, ct, policy, tab), C.backward(dy, u, ct, policy, tab)
            assert bool((y[:, 3:] == 0).all())
            assert torch.equal(_bits(y[:, :3].cpu()), _bits(want_y.float().to(dtype))), (policy, layout)
            assert torch.equal(_bits(dx.cpu()), _bits(want_dx.float().to(dtype).float())), (policy, layout)
            assert float(want_y.abs().max()) > 0 and float(want_dx.abs().max()) > 0


# ---- (c) bound, (d) adjoint -----------------------------------------------------------------------------------------------------------
def _apply_case(hw, policy, geom, cmat, dtype, layout, src_dtype=torch.float32):
    x, dy, u, _, _ = _operands(hw)
    tab, ct = _tables(hw, geom, cmat)
    ref = _reference(hw, policy, geom, cmat)
    y, dx = _run(x, dy, u, ct, tab, policy, dtype, layout, src_dtype)
    _check(y, dx, ref, dtype, (policy, geom, cmat, str(dtype), layout, hw))
    if dtype == torch.float32:
        # (d) the adjoint from the GPU's own outputs: <T(x), dy> = <x, T'(dy)> up to what each side may be off by.  T is affine (the
        # offsets, and the mean of `color`): its value at 0 goes to the left (from the float64 restatement: a constant of the case)
        terms = (y[:, :3].double().cpu() - ref[4]) * dy.double()
        lhs, size = float(terms.sum()), float(terms.abs().sum())
        rhs = float((x.double() * dx.double().cpu()).sum())
        slack = float((ref[1] * dy.double().abs()).sum() + (ref[3] * x.double().abs()).sum())
        print("adjoint %s: |lhs - rhs| = %.3e, slack %.3e, sum |terms| = %.3e" % ((policy, geom, cmat, hw), abs(lhs - rhs), slack, size))
        assert abs(lhs - rhs) <= slack and size > 0


@pytest.mark.parametrize("cmat", range(1, 32))
def test_every_subset_of_the_words_within_the_bound(cmat):
    """All 31 subsets at both ends of each range, the ctable read back from the device: with color and without, with translation and
    cutout and without, in the plain family and through a geometric table (all four parts; 8 x 24: without rot90), fp32, the adjoint
    check included."""
    for hw, policy, geom, layout in (((16, 16), "color,translation,cutout", 0, "nchw"), ((16, 16), "", 0, "strided"),
                                     ((16, 16), "color,cutout", GEOM_ALL, "channels_last"), ((8, 24), "", GEOM_ALL & ~G.ROT90, "nchw"),
                                     ((8, 24), "color", 0, "channels_last"), ((8, 24), "translation,cutout", 0, "nchw")):
        _apply_case(hw, policy, geom, cmat, torch.float32, layout)


@pytest.mark.parametrize("hw", SHAPES, **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_all_words_on_every_shape_storage_type_and_layout(dtype, hw):
    geom = _geom_for(hw, GEOM_ALL)
    ops.set_compute_dtype(dtype)
    try:
        for i, policy in enumerate(("", "translation,cutout", "color", "color,translation,cutout")):
            _apply_case(hw, policy, 0, C.ALL, dtype, LAYOUTS[i % 3])
            _apply_case(hw, policy, geom, C.ALL, dtype, LAYOUTS[(i + 1) % 3])
        if dtype != torch.float32:          # the source in the compute type (the operands are exact in it)
            _apply_case(hw, "color,translation,cutout", 0, C.ALL, dtype, "nchw", src_dtype=dtype)
            _apply_case(hw, "color,cutout", geom, C.ALL, dtype, "channels_last", src_dtype=dtype)
    finally:
        ops.set_compute_dtype(torch.float32)


# ---- (e) the identity, structure and gate -------------------------------------------------------------------------------------------
class _Run:
    """One forward and one backward call through the C ABI on windows carved out of canary-filled buffers.  entry: "cmat" (tab: a device
    affine table or None for the plain family; ct: the ctable; p: a device tensor or None for a NULL p_dev), "old" (the entries without a
    ctable, ct ignored) or "plain" (sp_ingest_image / _bwd).  The partials' interior is NaN on entry: a result that read a value nobody
    wrote is NaN."""

    def __init__(self, xs, dyp, u, tab, ct, policy, dtype, entry, p=None):
        dev = xs.device
        n, _, h, w = xs.shape
        cp, esz = ops.pad_channels(3, dtype), torch.empty((), dtype=dtype).element_size()
        self.out = torch.full((PAD + n * h * w * cp + PAD,), CANARY, dtype=dtype, device=dev)
        self.grad = torch.full((PAD + n * h * w * 3 + PAD,), CANARY, dtype=dtype, device=dev)
        self.parts = [torch.full((PAD + n * ops.augment_geom_slices(h, w, b) + PAD,), CANARY, dtype=torch.float32, device=dev) for b in (False, True)]
        self.ctable = torch.full((PAD + n * 12 + PAD,), CANARY, dtype=torch.float32, device=dev)
        self.ctable[PAD:-PAD] = ct.flatten()
        for part in self.parts:
            part[PAD:-PAD] = float("nan")
        at = lambda t, size: ctypes.c_void_p(t.data_ptr() + PAD * size)      # noqa: E731
        dt, st = ops.sp_dtype(dtype), ops.stream()
        if entry == "plain":
            L.call("sp_ingest_image", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, 3, h, w, cp, None, None, dt, st)
            L.call("sp_ingest_image_bwd", ops.ptr(dyp), cp, at(self.grad, esz), 3, n * h * w, None, dt, st)
        elif entry == "old" and tab is not None:
            L.call("sp_augment_geom_ingest", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   ops.ptr(tab), at(self.parts[0], 4), ops.ptr(p), dt, st)
            L.call("sp_augment_geom_ingest_bwd", ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy, ops.ptr(tab),
                   at(self.parts[1], 4), ops.ptr(p), dt, st)
        elif entry == "old":
            gated = ("_gated", (ops.ptr(p),)) if p is not None else ("", ())
            L.call("sp_augment_ingest" + gated[0], ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   at(self.parts[0], 4), *gated[1], dt, st)
            L.call("sp_augment_ingest_bwd" + gated[0], ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy,
                   at(self.parts[1], 4), *gated[1], dt, st)
        else:
            L.call("sp_augment_cmat_ingest", ops.ptr(xs), L.SP_F32, *xs.stride(), at(self.out, esz), n, h, w, cp, ops.ptr(u), policy,
                   ops.ptr(tab), at(self.ctable, 4), at(self.parts[0], 4), ops.ptr(p), dt, st)
            L.call("sp_augment_cmat_ingest_bwd", ops.ptr(dyp), cp, at(self.grad, esz), n, h, w, ops.ptr(u), policy, ops.ptr(tab),
                   at(self.ctable, 4), at(self.parts[1], 4), ops.ptr(p), dt, st)
        torch.cuda.synchronize()
        for buf in [self.out, self.grad, self.ctable] + self.parts:
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), entry
        assert torch.equal(self.ctable[PAD:-PAD].cpu(), ct.flatten().cpu())              # the apply entries only read the ctable
        self.y = _bits(self.out[PAD:-PAD].view(n, h, w, cp))               # (n, h, w, cp) bits
        self.dx = _bits(self.grad[PAD:-PAD].view(n, h, w, 3))
        self.yf = self.out[PAD:-PAD].view(n, h, w, cp).permute(0, 3, 1, 2)
        self.dxf = self.grad[PAD:-PAD].view(n, h, w, 3).permute(0, 3, 1, 2)


@pytest.mark.parametrize("hw", [(16, 16), (40, 40), (8, 24)], **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_identity_ctable_through_the_new_entries_equals_the_old_entries(dtype, hw):
    """A call through the entries without a ctable and the same call through the new entries with the identity matrix: bit for bit
    where the old call only moves data (no color: 1 x + 0 y + 0 z + 0 is x), within the bound of the OLD transform where it computes."""
    dev = _dev()
    x, dy, u, v, _ = _operands(hw)
    eye = C.identity_table(x.shape[0]).to(dev)
    geom = _geom_for(hw, GEOM_ALL)
    tab = _tables(hw, geom, C.ALL)[0]
    ud, dyp = u.to(dev), _padded_dy(dy, dtype, dev)
    for table in (None, tab.to(dev)):
        for policy, layout, p in ((6, "strided", None), (0, "nchw", _p(0.5, dev)), (7, "channels_last", None), (5, "nchw", _p(1.0, dev))):
            xs = _layout(x.to(dev), layout)
            old, new = _Run(xs, dyp, ud, table, eye, policy, dtype, "old", p), _Run(xs, dyp, ud, table, eye, policy, dtype, "cmat", p)
            if not policy & 1:
                assert torch.equal(new.y, old.y) and torch.equal(new.dx, old.dx), (policy, table is None)
            else:
                if table is None:
                    ref = (A.forward(x, u, policy), A.forward_bound(x, u, policy), A.backward(dy, u, policy), A.backward_bound(dy, u, policy))
                else:
                    ref = (G.forward(x, u, tab, policy), G.forward_bound(x, u, tab, policy), G.backward(dy, u, tab, policy),
                           G.backward_bound(dy, u, tab, policy))
                _check(new.yf, new.dxf, ref, dtype, ("identity", policy, table is None, hw))
                print("identity %s: bits equal forward %s, backward %s" % ((policy, table is None), torch.equal(new.y, old.y), torch.equal(new.dx, old.dx)))


@pytest.mark.parametrize("hw", [(40, 40), (64, 64), (8, 24)], **ids)
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_canaries_nan_partials_repeat_runs_and_the_gate(dtype, hw):
    """Through the C ABI, both families: nothing outside the buffers is written, the padding channels are zero, no result leans on a
    partial nobody wrote (NaN partials are ignored without color), two runs agree to the bit, a NULL p_dev equals p = 1; with u7 on
    either side of p = 0.5 (0.5 itself is dead: the compare is strict) the dead images EQUAL the plain ingest and the live ones the
    ungated result, forward and backward."""
    dev = _dev()
    x, dy, u, _, _ = _operands(hw)
    geom = _geom_for(hw, GEOM_ALL)
    tab, ct = _tables(hw, geom, C.ALL)
    tab, ct = tab.to(dev), ct.to(dev)
    u = u.clone()
    u[:, 7] = torch.tensor([0.25, 0.75, 0.5, float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0))), LAST, 0.0])
    live, dead = [0, 3, 5], [1, 2, 4]
    ud, dyp = u.to(dev), _padded_dy(dy, dtype, dev)
    for table, policy, layout in ((None, 7, "strided"), (None, 6, "channels_last"), (tab, 5, "strided"), (tab, 4, "channels_last")):
        xs = _layout(x.to(dev), layout)
        run = lambda entry, p=None: _Run(xs, dyp, ud, table, ct, policy, dtype, entry, p)      # noqa: E731
        ungated, plain, gated = run("cmat"), run("plain"), run("cmat", _p(0.5, dev))
        one, again, zero = run("cmat", _p(1.0, dev)), run("cmat", _p(0.5, dev)), run("cmat", _p(0.0, dev))
        for name in ("y", "dx"):
            got = getattr(gated, name)
            assert torch.equal(got[live], getattr(ungated, name)[live]), (name, "live")
            assert torch.equal(got[dead], getattr(plain, name)[dead]), (name, "dead")
            for i in range(x.shape[0]):
                assert not torch.equal(getattr(ungated, name)[i], getattr(plain, name)[i]), (name, i)
            assert torch.equal(getattr(one, name), getattr(ungated, name)), (name, "p = 1 against a NULL p_dev")
            assert torch.equal(getattr(zero, name), getattr(plain, name)), (name, "p = 0")
            assert torch.equal(getattr(again, name), getattr(gated, name)), (name, "second run")
        assert bool((gated.y[..., 3:] == 0).all()) and bool((ungated.y[..., 3:] == 0).all())
        for r in (gated, ungated):
            assert not bool(torch.isnan(r.out[PAD:-PAD].float()).any()) and not bool(torch.isnan(r.grad[PAD:-PAD].float()).any())
        for part in ungated.parts:                           # every partial written with color, none without
            inner = part[PAD:-PAD]
            assert bool(torch.isfinite(inner).all()) if policy & 1 else bool(torch.isnan(inner).all())
        # the ops carry ctable, table and gate to the same entries, forward and backward
        y, dx = _run(x, dy, u, ct.cpu(), None if table is None else table.cpu(), policy, dtype, layout, p=_p(0.5, dev))
        assert torch.equal(_bits(y.permute(0, 2, 3, 1)), gated.y) and torch.equal(_bits(dx.to(dtype).permute(0, 2, 3, 1)), gated.dx)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_pair_form_equals_two_single_calls(dtype):
    dev = _dev()
    hw = (40, 40)
    x, _, u, _, _ = _operands(hw)
    tab, ct = _tables(hw, GEOM_ALL, C.ALL)
    tab, ct = tab.to(dev), ct.to(dev)
    xa, xb = x.to(dev), x.flip(0).to(dev).contiguous(memory_format=torch.channels_last)
    ua, ub = u.to(dev), u.flip(0).contiguous().to(dev)
    ta, tb = tab, tab.flip(0).contiguous()
    ca, cb = ct, ct.flip(0).contiguous()
    for policy in ("color,translation,cutout", "cutout"):
        for p in (None, _p(0.5, dev)):
            for tables in ((None, None), (ta, tb)):
                pair = ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, policy, p=p, table_a=tables[0], table_b=tables[1], ctable=(ca, cb))
                assert not pair.requires_grad and tuple(pair.shape) == (2 * x.shape[0], ops.pad_channels(3, dtype), 40, 40)
                single = torch.cat([ops.augment_ingest_image(xa, dtype, ua, policy, p=p, table=tables[0], ctable=ca).permute(0, 2, 3, 1),
                                    ops.augment_ingest_image(xb, dtype, ub, policy, p=p, table=tables[1], ctable=cb).permute(0, 2, 3, 1)]).permute(0, 3, 1, 2)
                assert torch.equal(_bits(pair), _bits(single)), policy
                other = ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, policy, p=p, table_a=tables[0], table_b=tables[1])
                assert not torch.equal(_bits(pair), _bits(other))
    for bad in ((ca,), (ca, None), ca):
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image_pair(xa, xb, dtype, ua, ub, "cutout", ctable=bad)


def test_bad_arguments_raise_and_launch_nothing():
    dev = _dev()
    u, z = torch.zeros(2, 8, device=dev), torch.zeros(2, 8, device=dev)
    img = torch.zeros(2, 3, 8, 8, device=dev)
    for bad in (torch.zeros(3, 12, device=dev), torch.zeros(2, 8, device=dev), torch.zeros(2, 12), torch.zeros(2, 12, device=dev, dtype=torch.float64),
                torch.zeros(2, 24, device=dev)[:, ::2], torch.zeros(25, device=dev)[1:].view(2, 12)):
        with pytest.raises(L.SempyrError):
            ops.augment_ingest_image(img, torch.float32, u, "color", ctable=bad)
    for bad_z, cmat in ((torch.zeros(2, 7, device=dev), 31), (z, 0), (z.double(), 31), (torch.zeros(2, 16, device=dev)[:, ::2], 31), (z, 32)):
        out = torch.full((2, 12), CANARY, device=dev)
        with pytest.raises(L.SempyrError):
            ops.augment_cmat_decode(bad_z, cmat, out=out)
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())
    with pytest.raises(L.SempyrError):
        ops.augment_cmat_decode(z, "luma")
    with pytest.raises(L.SempyrError):
        ops.augment_cmat_decode(z, 31, out=torch.zeros(2, 8, device=dev))
    good = torch.zeros(2, 12, device=dev)
    assert ops.augment_cmat_decode(z, "hue", out=good) is good
