"""Integer operands for the exact tests of the MFMA convolution / linear kernels (tests/test_gpu_exact.py) and the comparison that
goes with them.  Everything here runs on the CPU.

What "exact" rests on: the operands are integers the storage type holds exactly, and every partial sum of a result - in ANY order,
so through atomics, slabs, split-K and the K-split of the last round alike - stays below 2^24 in magnitude (times the denominator
of a power-of-two scale: 0.25 after average pooling), so every fp32 addition is exact.  The kernel's result is then the float64
reference after at most ONE round-to-nearest-even into the storage type, bit for bit; no tolerance appears anywhere.

Two regimes.  unit: ternary activations, ternary weights with at most 200 non-zeros per output row, |bias| <= 8, |residual| <= 16 -
every output is an integer of magnitude <= 256 that the 16-bit types hold exactly, so every single product counts.  wide: dense
integers as large as the storage type's significand allows against dense ternary values (wide-w: the other way round, 8-bit
weights) - partial sums of 15 and more bits, so an intermediate that passes through 16 bits, or a 12-bit fp32 operand that passes
through a shorter multiply, shows."""
import torch

LIMIT = 1 << 24                      # integers of magnitude <= 2^24 are exact in fp32
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 12}     # operand bits: the significand, 12 in fp32 (products of 24)
F16_MAX = 65504.0
UNIT_NNZ, UNIT_BIAS, UNIT_RES = 200, 8, 16


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def integers(shape, amax: int, g: torch.Generator) -> torch.Tensor:
    """Dense float64 integers, uniform in [-amax, amax]."""
    return torch.randint(-amax, amax + 1, tuple(shape), generator=g).double()


def ternary(shape, g: torch.Generator) -> torch.Tensor:
    return integers(shape, 1, g)


def sparse_ternary_rows(rows: int, cols: int, g: torch.Generator, nnz: int = UNIT_NNZ) -> torch.Tensor:
    """[rows][cols] in {-1, 0, 1} with at most `nnz` non-zeros per row (three quarters of a short row), at random places."""
    keep = min(nnz, max(1, (3 * cols) // 4))
    rank = torch.rand(rows, cols, generator=g).argsort(1).argsort(1)
    sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    return sign * (rank < keep).double()


def wide_amax(dtype, k: int, extras: int = 0, other: int = 1, denom: int = 1) -> int:
    """Largest operand magnitude of the wide regime: the storage type's significand, and k products against |other| <= `other` plus
    `extras` (bias, residuals) below 2^24 / denom (denom: the denominator a power-of-two scale gives the values)."""
    return max(1, min((1 << SIG_BITS[dtype]) - 1, ((LIMIT - 1) // denom - extras) // (k * other)))


def f16_amax(amax: int, k: int, dtype, gain: int = 1) -> int:
    """fp16 storage: lowers amax so that six standard deviations of `gain` x a sum of k products (uniform integers against dense
    ternary values: variance amax^2 / 3 * 2 / 3 each) stay below the largest finite value; check_reference() asserts the outcome."""
    if dtype != torch.float16:
        return amax
    return max(1, min(amax, int(F16_MAX / (6.0 * gain * (2.0 * k / 9.0) ** 0.5))))


def check_reference(ref: torch.Tensor, bound: float, dtype, regime: str, denom: int = 1, what="") -> None:
    """The three conditions a case has to meet on the CPU before anything is launched.  ref: the float64 reference (for a weight
    gradient: the fp32 result); bound: an upper bound of every partial sum's magnitude, sum |a| |b| + |extras|; denom: the
    denominator the values may carry (4 after average pooling, the 0.25 slope, the pooled-gradient input; 2 / 8 with group scales)."""
    assert ref.dtype == torch.float64, what
    assert torch.equal(ref * denom, (ref * denom).round()), (what, "the reference is not integral (x %d)" % denom)
    assert bound * denom < LIMIT, (what, "partial sums reach %.0f x %d >= 2^24" % (bound, denom))
    if dtype == torch.float16:
        assert float(ref.abs().max()) < F16_MAX, (what, float(ref.abs().max()))
    if regime == "unit" and denom == 1:
        assert torch.equal(ref, ref.to(dtype).double()), (what, "a unit-regime value is not representable in the storage type")


def expected(ref: torch.Tensor, dtype) -> torch.Tensor:
    """What the kernel must store: ONE round-to-nearest-even of the exact value (the identity in the unit regime)."""
    return ref.to(dtype)


def lrelu_f32(v: torch.Tensor) -> torch.Tensor:
    """LeakyReLU(0.2) as the epilogues compute it: one rounded fp32 product of an exactly held value."""
    v32 = v.float()
    assert torch.equal(v32.double(), v), "LeakyReLU input is not exact in fp32"
    return torch.where(v32 > 0, v32, v32 * 0.2).double()


def assert_exact(got: torch.Tensor, want: torch.Tensor, what="", names=None) -> None:
    """got == want element for element (torch.equal: no tolerance; -0 equals +0).  On a mismatch the message says how many elements
    differ, which indices of every axis they touch and the first few (index, got, want) - the element pattern is the finding."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | (got.isnan() != want.isnan())
    idx = bad.nonzero()
    names = names or ["axis%d" % i for i in range(got.dim())]
    axes = []
    for a, name in enumerate(names):
        u = idx[:, a].unique().tolist()
        axes.append("%s: %s" % (name, u if len(u) <= 24 else "%d values, %d .. %d" % (len(u), u[0], u[-1])))
    first = ["%s got %r want %r" % (tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:6]]
    raise AssertionError("%s: %d of %d elements differ; %s; first: %s" % (what, int(bad.sum()), got.numel(), "; ".join(axes), " | ".join(first)))


def assert_sentinel(buf: torch.Tensor, sentinel: float, what="") -> None:
    assert bool((buf.detach().cpu().double() == sentinel).all()), (what, "the sentinel beyond the valid channels was overwritten")


# ----------------------------------------------------------------------------------------------
# case builders: operands, float64 reference and the CPU checks, shared by the GPU tests and the harness self-test
# ----------------------------------------------------------------------------------------------
class Case(dict):
    __getattr__ = dict.__getitem__


def conv_case(dtype, n, h, w, cin, cout, k, regime, bias=False, res=0, act=0, mask=False, pool2=0, up=False, groups=False, seed=0,
              amax=None) -> Case:
    """One launch of sp_conv2d_igemm in exact form (include/sempyr.h: sp_conv_params):
        y = act((conv(x, w) * scale[group] + bias) * slope(mask) + res1 + res2), pooled 2x2 (1: average, 2: maximum) before the bias.
    cin counts the packed channels (cin_p); the weight is the raw forward packing [cout][k * k][cin].  act: 0 none, 1 LeakyReLU(0.2),
    2 ReLU.  up: x is at half resolution and stands for 0.25 x its nearest-neighbour expansion.  groups: the two halves of the batch
    carry the accumulator scales 0.5 and 2.0.  mask: slope 0.25 where the mask operand is <= 0.  regime: unit | wide | wide-w.
    Tensors are float64, activations NCHW; `want` is the NHWC tensor the kernel must store."""
    import torch.nn.functional as F
    g = gen(seed)
    kk = k * k * cin
    hin, win = (h // 2, w // 2) if up else (h, w)
    ho, wo = (h // 2, w // 2) if pool2 else (h, w)
    denom = (4 if pool2 == 1 else 1) * (4 if up else 1) * (4 if mask else 1) * (2 if groups else 1)
    side = UNIT_RES if regime == "unit" else (1 << SIG_BITS[dtype]) - 1
    bmax = UNIT_BIAS if regime == "unit" else (1 << SIG_BITS[dtype]) - 1
    extras = (bmax if bias else 0) + res * side
    smax = 2 if groups else 1
    if regime == "unit":
        x, wt = ternary((n, cin, hin, win), g), sparse_ternary_rows(cout, kk, g)
    elif regime == "wide":
        a = amax or f16_amax(wide_amax(dtype, kk, extras, smax, denom), kk, dtype, smax)
        x, wt = integers((n, cin, hin, win), a, g), ternary((cout, kk), g)
    else:
        assert regime == "wide-w", regime
        a = amax or f16_amax(min(255, wide_amax(dtype, kk, extras, smax, denom)), kk, dtype, smax)
        x, wt = ternary((n, cin, hin, win), g), integers((cout, kk), a, g)
    b = integers((cout,), bmax, g) if bias else None
    rs = [integers((n, cout, ho, wo), side, g) for _ in range(res)]
    ms = integers((n, cout, ho, wo), 2, g) if mask else None
    xin = 0.25 * F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    conv = F.conv2d(xin, wt.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous(), padding=k // 2)
    split = n // 2
    if groups:
        conv[:split] *= 0.5
        conv[split:] *= 2.0
    pre = conv                                     # at the full resolution, before the bias: what a max-pooling routes on
    v = F.avg_pool2d(conv, 2) if pool2 == 1 else F.max_pool2d(conv, 2) if pool2 == 2 else conv
    if b is not None:
        v = v + b.view(1, -1, 1, 1)
    if ms is not None:
        v = v * torch.where(ms > 0, 1.0, 0.25).double()
    for r in rs:
        v = v + r
    bound = float(xin.abs().max()) * float(wt.abs().sum(1).max()) * smax + extras
    what = (str(dtype), n, h, w, cin, cout, k, regime)
    check_reference(v, bound, dtype, regime, denom, what)
    ref = lrelu_f32(v) if act == 1 else torch.relu(v) if act == 2 else v
    return Case(x=x, wt=wt, b=b, rs=rs, ms=ms, v=v, pre=pre, ref=ref, want=expected(ref, dtype).permute(0, 2, 3, 1).contiguous(),
                split=split, denom=denom, bound=bound, ho=ho, wo=wo, hin=hin, win=win, what=what)


def wgrad_case(dtype, n, split, h, w, cin, cout, k, pooled, seed=0) -> Case:
    """One accumulating weight-gradient call: ternary x [n][cin][h][w], integer dy (|dy| as large as n h w allows below 2^24 and the
    storage type holds), destinations that START with non-zero integers.  A pooled dy stands for 0.25 x its expansion.  Per group
    (lo, hi): the fp32 contents dW [cout][k * k][cin] and dbias [cout] must have afterwards, from float64 autograd."""
    import torch.nn.functional as F
    g = gen(seed)
    denom = 4 if pooled else 1
    npix = n * h * w
    a = wide_amax(dtype, npix, 16, 1, denom)
    x = ternary((n, cin, h, w), g)
    dy = integers((n, cout, h // 2, w // 2) if pooled else (n, cout, h, w), a, g)
    dyf = 0.25 * F.interpolate(dy, scale_factor=2, mode="nearest") if pooled else dy
    groups = []
    for lo, hi in ([(0, split), (split, n)] if split else [(0, n)]):
        w0 = integers((cout, k * k, cin), 16, g)
        w0[w0 == 0] = 5.0
        b0 = integers((cout,), 16, g)
        b0[b0 == 0] = -3.0
        wref = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x[lo:hi], wref, padding=k // 2).backward(dyf[lo:hi])
        dw = wref.grad.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        db = dyf[lo:hi].sum((0, 2, 3))
        what = (str(dtype), n, split, h, w, cin, cout, k, pooled, lo)
        bound = float(dyf.abs().max()) * (hi - lo) * h * w + 16
        check_reference(w0 + dw, bound, torch.float32, "wide", denom, what)
        check_reference(b0 + db, bound, torch.float32, "wide", denom, what)
        groups.append(Case(lo=lo, hi=hi, w0=w0, b0=b0, dw=dw, db=db, want_w=(w0 + dw).float(), want_b=(b0 + db).float()))
    return Case(x=x, dy=dy, groups=groups, denom=denom, amax=a)


def linear_case(dtype, k, n, b, regime, seed=0) -> Case:
    """y = relu(x W^T + bias + res) with W [n][k]; dx = dz W; dW = dz^T x, dbias = sum_b dz (dz ternary).  regime as conv_case."""
    g = gen(seed)
    side = UNIT_RES if regime == "unit" else (1 << SIG_BITS[dtype]) - 1
    bmax = UNIT_BIAS if regime == "unit" else (1 << SIG_BITS[dtype]) - 1
    if regime == "unit":
        x, wt = ternary((b, k), g), sparse_ternary_rows(n, k, g)
    elif regime == "wide":
        x, wt = integers((b, k), f16_amax(wide_amax(dtype, k, bmax + side), k, dtype), g), ternary((n, k), g)
    else:
        x, wt = ternary((b, k), g), integers((n, k), f16_amax(min(255, wide_amax(dtype, k, bmax + side)), max(k, n), dtype), g)
    bias, res = integers((n,), bmax, g), integers((b, n), side, g)
    v = x @ wt.t() + bias + res
    what = (str(dtype), k, n, b, regime)
    check_reference(v, float(x.abs().max()) * float(wt.abs().sum(1).max()) + bmax + side, dtype, regime, 1, what)
    # input gradient: the weight's magnitude bounds what dz may hold
    wmax = float(wt.abs().max())
    dz = integers((b, n), f16_amax(wide_amax(dtype, n, 0, int(wmax)), n, dtype) if regime != "wide-w" else 1, g)
    dx = dz @ wt
    check_reference(dx, float(dz.abs().max()) * float(wt.abs().sum(0).max()), dtype, "wide", 1, what)
    dzt = ternary((b, n), g)
    dw, db = dzt.t() @ x, dzt.sum(0)
    check_reference(dw, float(x.abs().max()) * b, torch.float32, "wide", 1, what)
    return Case(x=x, wt=wt, bias=bias, res=res, v=v, ref=torch.relu(v), want=expected(torch.relu(v), dtype), dz=dz, dx=dx,
                want_dx=expected(dx, dtype), dzt=dzt, want_dw=dw.float(), want_db=db.float(), what=what)


def pack_reference(wt: torch.Tensor, cin_p: int, cout_p: int, dtype):
    """The two packings of an OIHW weight (include/sempyr.h: sp_pack_weight) as torch permutations: forward [cout][taps][cin_p],
    input gradient [cin][flipped taps][cout_p], zeros in the padding."""
    cout, cin, kh, kw = wt.shape
    fwd = torch.zeros(cout, kh * kw, cin_p, dtype=torch.float64)
    fwd[:, :, :cin] = wt.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    dg = torch.zeros(cin, kh * kw, cout_p, dtype=torch.float64)
    dg[:, :, :cout] = wt.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, kh * kw, cout)
    return fwd.to(dtype), dg.to(dtype)
