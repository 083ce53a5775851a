"""Operands, float64 references, CPU-checked conditions and the comparison for the tests of the batch-norm kernels (csrc/norm.hip) and
the bilinear x2 kernels (csrc/resample.hip): tests/test_gpu_norm_exact.py; the self-test of everything here: tests/test_norm_harness.py.
Everything in this module runs on the CPU.  Tensors are NHWC [n][h][w][c] float64 unless said otherwise.

sums      statistics.  x = integers in [-7, 7] + a per-channel (and per-group) integer offset in [-8, 8] ([-2, 2] + [-2, 2] where the
          pixel count needs it), held exactly by the storage type, sum x^2 < 2^24 per channel: every fp32 partial sum is exact in ANY
          order, so the finalize kernel sees the exact integers S and Q.  mean = fl32(S / count) bit for bit (one IEEE double division).
          invstd within ONE fp32 ulp of fl32(1 / sqrt(Q / count - m m + eps)) taken in float64: a contraction of gq / cnt - m * m into
          an fma changes the double by at most one rounding of m m <= 256, 2^-45 absolute against var + eps >= 1/4, so the two doubles
          round to the same or to neighbouring floats.  Running statistics: exact where the count is dyadic (a power of two, or 3 x
          one with S made divisible by 3), momentum = 0.5 and running_mean integral; otherwise within ulp32(max(|old|, |momentum x
          batch|)) of the float64 value (the result's magnitude is at most twice that maximum, half an ulp of it is the bound), the
          second step of a pair on top of (1 - momentum) x the first step's ulp.
affine    apply with GIVEN statistics: mean, bias, x integers, invstd a power of two in [1/4, 2], scale an integer in [-3, 3]:
          a = scale invstd, b = bias - mean a and z = a x + b are multiples of 1/4 below 2^20 - exact in fp32 with or without fma.
          y = act(z) rounded ONCE to the storage type; LeakyReLU is max(z, fl32(0.2f z)), the product formed in float32 here too.
backward  sp_bn_backward with given statistics: dy = 5 k (fl32(0.2f x 5k) = k exactly: 0.2f exceeds 1/5 by 1.49e-8 relative, below
          the half ulp 2^-25), scale in {+-1/2, +-1, +-2}, bias in {+-4, +-8}, x = mean + d q with d in [-12, 12] and q = max(1,
          1 / |scale invstd|): z = scale xhat + bias takes both signs and 0 in every (sample, channel), and its sign differs from
          xhat's for more than a tenth of the elements.  Sums of dz and dz xhat are multiples of 1/4 below 2^22: dgamma, dbeta, demb,
          and c1 = fl32(s1 / count), c2 likewise are exact for every count.  dx = invstd (dz scale - c1 - xhat c2) is exact (one
          rounding to storage) where every intermediate is an fp32 number (checked per case: the small power-of-two counts);
          otherwise three fp32 roundings of magnitudes <= T = |dz scale| + |c1| + |xhat c2| and the storage rounding:
              B_dx = e + urel (|dx| + e) + eta,   e = invstd x 3 x 2^-24 x T (1 + 2^-20).
interp    the bilinear x2 (align_corners) of integers, on its own and fused with the apply.  Exact position p = o (I - 1) / (2I - 1);
          the kernels form fl32(fl32((I-1)/(2I-1)) o): |position error| <= E(o) = 2 x 2^-24 x p (1 + 2^-24).  The interpolant is
          continuous and piecewise linear, so a position off by E moves it by at most E x the largest slope of the segment and its two
          neighbours (a row position next to an integer may land in the neighbouring segment; a column keeps its segment and
          extrapolates).  Each of the two blends (1 - l) s0 + l s1 costs at most four fp32 roundings of values <= M (1 - l, two
          products, the sum), M the largest |source| among the taps and the neighbouring rows:
              B_up = (E_h S_h + E_w S_w + 8 x 2^-24 M)(1 + 2^-20);   stored: + urel (|ref| + B_up) + eta.
          The backward is the transpose: per tap |dy| (E_h |w_w| + E_w |w_h| + E_h E_w) + 12 x 2^-24 |w_h| |w_w| |dy| (1 - l, the
          product and four additions per axis).  sp_bn_apply_up2 normalises u = up2(x): 16-bit storage rounds u first,
              B_u = B_up + urel16 (|u| + B_up),   B_z = |a| B_u + 2 x 2^-24 (|z| + |a| B_u)      (the fma, the LeakyReLU product),
          and LeakyReLU is 1-Lipschitz.  Where an axis has extent 1 its weight is exactly 0 and its terms vanish: H = W = 1 is the
          identity and is held to torch.equal.

dense     the chains statistics -> apply -> backward (plain, pair, and the up2 family in fp32 storage) on Gaussian operands against
          float64, the later calls fed with the statistics the device computed: dense_case derives the per-element bounds.

urel is the relative error of one round-to-nearest into the storage type (2^-8 bf16, 2^-11 fp16, 2^-24 fp32); eta = 2^-25 covers
fp16's subnormals.  No element is excluded anywhere and no share of outliers is admitted."""
import numpy as np
import torch

import exact_util as X
from attention_exact_util import assert_within
from exact_util import Case, assert_exact, expected   # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
UREL = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
ETA = {BF16: 0.0, F16: 2.0 ** -25, F32: 0.0}
U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
EPS = float(np.float32(1e-5))
MAX_PARTS = 1024                       # csrc/norm.hip: BN_MAX_PARTS
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
CLASSES = 5
AXES = ["image", "row", "column", "channel"]

# ---- shapes (n, h, w, c): the smallest that reach each edge ----------------------------------------------------------------------
BASE = (2, 8, 8, 64)
SMALL = [BASE, (1, 4, 16, 12), (2, 4, 8, 20), (4, 4, 4, 96), (2, 8, 8, 136), (3, 5, 7, 20), (2, 16, 16, 64)]
WIDE = {F32: (1, 8, 8, 1032), BF16: (1, 4, 4, 2056), F16: (1, 4, 4, 2056)}       # the second trip of the channel-group loop
# 129 channel groups leave one pixel per block step, so pixels / 8 blocks are asked for: the cheapest way past a clamp of the row count
CLAMP = [(1, 512, 512, 64), (1, 64, 128, 1024), (1, 96, 86, 516)]                # 1024 partial rows (the last: 1032 asked for, every type)
PAIR_CLAMP = (4, 64, 64, 64)
PAIR_CLAMP_516 = (4, 36, 38, 516)                                                # 512 rows per group: 513 asked for with split = 1
BWD_CLAMP = (3, 64, 64, 64)                                                      # up2_grid's budget in fp32
BWD_CLAMP_516 = (3, 48, 57, 516)                                                 # 1024 / n rows per sample: 3 x 342 asked for
TINY = [(2, 1, 1, 8), (1, 1, 5, 8), (1, 5, 1, 8), (1, 2, 2, 8), (1, 2, 3, 8), (1, 2, 4, 8)]      # every residue of OW mod 4
UP = TINY + [(3, 5, 7, 20), (2, 8, 8, 64), (2, 4, 8, 20), (4, 4, 4, 96)]
ROW_CAP = (1, 32770, 1, 8)                                                       # 65540 output rows against the 65535-row grid cap
ROW_CAP_BWD = (2, 32770, 1, 8)                                                   # the backward's grid walks INPUT rows: 65540 of them
UP2_EXACT = [(2, 8, 8, 64), (3, 5, 7, 20), (2, 4, 8, 20), (4, 4, 4, 96), (2, 2, 3, 8), (3, 176, 2, 8)]     # 16-bit up2 reductions, constant maps
DTYPES = (F32, BF16, F16)


def sid(shape):
    return "x".join(str(a) for a in shape)


# ---- the launchers' plans, restated (csrc/norm.hip) -------------------------------------------------------------------------------
def vec(dt, c):
    return 4 if dt == F32 or c % 8 else 8


def pix_par(dt, c):
    return 256 // min(c // vec(dt, c), 256)


def stat_blocks(pixels, dt, c):
    return max(1, min(MAX_PARTS, pixels // (pix_par(dt, c) * 8)))


def pair_blocks(pix_a, pix_b, dt, c):
    return min(stat_blocks(max(pix_a, pix_b), dt, c), MAX_PARTS // 2)


def bwd_blocks(n, hw, dt, c):
    b = stat_blocks(hw, dt, c)
    return b if b * n <= MAX_PARTS else max(MAX_PARTS // n, 1)


def up2_rows(n, h, w, dt, c):
    """Partial rows per sample of the up2 reductions (up2_grid)."""
    gx = max(1, ((2 * w + 2) // 4 + 1 + pix_par(dt, c) - 1) // pix_par(dt, c))
    budget = max(1, MAX_PARTS // n)
    gx = min(gx, budget)
    return gx * max(1, min(budget // gx, 2 * h))


def ulp32(t):
    """The spacing of fp32 at |t| (float64 tensor)."""
    return torch.from_numpy(np.spacing(np.abs(t.numpy()).astype(np.float32)).astype(np.float64))


def held(t, dt):
    return torch.equal(t.to(dt).double(), t)


def f32_exact(t):
    return torch.equal(t.float().double(), t)


def act64(z, act):
    """act(z) of an exactly held fp32 z, as the kernels form it: LeakyReLU = max(z, fl32(0.2f z))."""
    if act == ACT_NONE:
        return z
    if act == ACT_RELU:
        return torch.relu(z)
    assert act == ACT_LRELU and f32_exact(z)
    z32 = z.numpy().astype(np.float32)
    return torch.from_numpy(np.maximum(z32, z32 * np.float32(0.2)).astype(np.float64))


def classes_of(n):
    """Class indices with class 0, the last class and (n >= 3) a repeated class."""
    return torch.tensor(([CLASSES - 1, 0, CLASSES - 1, 2] * ((n + 3) // 4))[:n] if n >= 2 else [CLASSES - 1], dtype=torch.int64)


def _seed(shape, salt):
    n, h, w, c = shape
    return salt * 7919 + 131 * n + 17 * h + 5 * w + c


# ------------------------------------------------------------------------------------------------------------------------------------
# sums
# ------------------------------------------------------------------------------------------------------------------------------------
def _odd_part(v):
    while v % 2 == 0:
        v //= 2
    return v


def sums_case(dt, shape, split=0, first=0, momentum=None, training=True, rep=1) -> Case:
    """sp_bn_stats (split == 0) / sp_bn_stats_pair; rep = 4: sp_bn_stats_up2 of a 1 x 1 map, whose expansion repeats every pixel.  want: mean / invstd [groups][c], the running statistics after the call, with
    the kind of comparison each gets (checks: name -> ("exact", want) | ("within", float64 reference, bound))."""
    n, h, w, c = shape
    what = ("sums", NAME[dt], shape, split, first)
    g = X.gen(_seed(shape, 1 + split))
    small = n * h * w * 225 >= X.LIMIT
    amax, omax = (2, 2) if small else (7, 8)
    x = X.integers(shape, amax, g)
    groups = [(0, split), (split, n)] if split else [(0, n)]
    counts = [rep * (hi - lo) * h * w for lo, hi in groups]
    dyadic = all(_odd_part(k) in (1, 3) for k in counts)
    for (lo, hi), cnt in zip(groups, counts):
        off = X.integers((c,), omax, g)
        x[lo:hi] += off
        if dyadic and _odd_part(cnt) == 3:                     # make S divisible by 3: the mean becomes dyadic
            v = x[lo, 0, 0] - torch.remainder(x[lo:hi].sum((0, 1, 2)), 3)
            x[lo, 0, 0] = torch.where(v < off - amax, v + 3, v)
    if h * w == 1 and n >= 2 and not split:                    # one pixel per sample: keep two of them 2 apart, or var < 1/4
        x[1] = torch.where((x[1] - x[0]).abs() < 2, x[0] - 2 * torch.sign(x[0]) + 2 * (x[0] == 0).double(), x[1])
    assert held(x, dt) and float(x.abs().max()) <= amax + omax, what
    if momentum is None:
        momentum = 0.5 if dyadic else 0.001
    mom = float(np.float32(momentum))
    rm0 = X.integers((c,), 8, g)
    rv0 = (1 + torch.randint(0, 12, (c,), generator=g).double()) / 4
    mean, inv, stats = [], [], []
    for (lo, hi), cnt in zip(groups, counts):
        xs = x[lo:hi]
        s, q = rep * xs.sum((0, 1, 2)), rep * (xs * xs).sum((0, 1, 2))
        assert float(q.max()) < X.LIMIT, (what, "sum x^2 reaches 2^24")
        m = s / cnt
        var = q / cnt - m * m
        assert float(m.abs().max()) <= 16 and float(var.min()) >= 0.25, (what, "|m| <= 16, var >= 1/4")
        if _odd_part(cnt) in (1, 3) and dyadic:
            assert f32_exact(m), (what, "the mean is not an fp32 number")
        mean.append(m)
        inv.append(1.0 / torch.sqrt(var + EPS))
        stats.append((m, var * cnt / (cnt - 1) if cnt > 1 else var))
    if split:                                                  # the two rows differ in every channel (and nearly every mean does)
        assert bool(((mean[0] != mean[1]) | (inv[0] != inv[1])).all()) and int((mean[0] != mean[1]).sum()) >= 0.9 * c, (what, "rows coincide")
    mean, inv = torch.stack(mean), torch.stack(inv)
    checks = {}
    if training:
        checks["mean"] = ("exact", mean.float())
        checks["invstd"] = ("within", inv, ulp32(inv))
        rm, rv = rm0, rv0
        brm, brv = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
        exact_rm = dyadic and mom == 0.5
        for gi in ([first, 1 - first] if split else [0]):
            m, unb = stats[gi]
            drm, drv = (1 - mom) * rm + mom * m, (1 - mom) * rv + mom * unb
            brm = (1 - mom) * brm + ulp32(torch.maximum(rm.abs(), (mom * m).abs()))
            brv = (1 - mom) * brv + ulp32(torch.maximum(rv.abs(), (mom * unb).abs()))
            if exact_rm:
                assert f32_exact(drm), (what, "running_mean leaves fp32 although every term is dyadic")
                brm = torch.zeros_like(brm)
            ref_rm, ref_rv = drm, drv
            rm, rv = drm.float().double(), drv.float().double()          # what the next step reads back
        checks["running_mean"] = ("exact", ref_rm.float()) if exact_rm else ("within", ref_rm, brm)
        checks["running_var"] = ("within", ref_rv, brv)
    else:
        inv = (1.0 / torch.sqrt(rv0 + EPS)).unsqueeze(0)
        checks["mean"] = ("exact", rm0.float().unsqueeze(0))
        checks["invstd"] = ("within", inv, 2 * ulp32(inv))
        checks["running_mean"] = ("exact", rm0.float())
        checks["running_var"] = ("exact", rv0.float())
    return Case(regime="sums", what=what, dtype=dt, shape=shape, rep=rep, split=split, first=first, momentum=mom, training=training, x=x,
                rm0=rm0, rv0=rv0, groups=groups, counts=counts, dyadic=dyadic, pow2=all(_odd_part(k) == 1 for k in counts),
                checks=checks, inv=inv)


def block_rows(x2, blocks, pp, drop_last=False):
    """[blocks][c][2] fp32: the partial rows of bn_stats_kernel over the pixels x2 [pixels][c] (fp32) - block b owns the pixels p
    with (p // pix_par) % blocks == b.  drop_last: the walk stops one pixel early (a planted fault)."""
    pixels, c = x2.shape
    if drop_last:
        x2, pixels = x2[:-1], pixels - 1
    owner = (torch.arange(pixels) // pp) % blocks
    part = torch.zeros(blocks, c, 2, dtype=torch.float32)
    part[:, :, 0].index_add_(0, owner, x2)
    part[:, :, 1].index_add_(0, owner, x2 * x2)
    return part


def restate_sums(c: Case, drop_last=False, skip_row=False, same_stats=False, swap_first=False, round16=False) -> Case:
    """The statistics kernels in fp32 / float64 as csrc/norm.hip states them.  The keywords plant the faults the tests exist for."""
    dt, (n, h, w, ch) = c.dtype, c.shape
    rm, rv = c.rm0.float(), c.rv0.float()
    if not c.training:
        return Case(mean=rm.clone().unsqueeze(0), invstd=(1.0 / torch.sqrt(rv + np.float32(EPS))).unsqueeze(0), running_mean=rm, running_var=rv)
    pp = pix_par(dt, ch)
    blocks = pair_blocks(c.counts[0], c.counts[1], dt, ch) if c.split else stat_blocks(c.counts[0], dt, ch)
    sums = []
    for lo, hi in c.groups:
        part = block_rows(c.x[lo:hi].reshape(-1, ch).float().repeat_interleave(c.rep, 0), blocks, pp, drop_last)
        if round16:
            part = part.to(BF16 if dt == F32 else dt).float()
        sums.append(part[:blocks - 1 if skip_row and blocks > 1 else blocks].double().sum(0))
    mean, inv = torch.zeros(len(sums), ch), torch.zeros(len(sums), ch)
    first = 1 - c.first if swap_first else c.first
    for gi in ([first, 1 - first] if c.split else [0]):
        src = sums[0] if same_stats else sums[gi]
        cnt = c.counts[0] if same_stats else c.counts[gi]
        m = src[:, 0] / cnt
        var = (src[:, 1] / cnt - m * m).clamp_min(0)
        mean[gi], inv[gi] = m.float(), (1.0 / torch.sqrt(var + EPS)).float()
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        rm = ((1.0 - c.momentum) * rm.double() + c.momentum * m).float()
        rv = ((1.0 - c.momentum) * rv.double() + c.momentum * unb).float()
    return Case(mean=mean, invstd=inv, running_mean=rm, running_var=rv)


# ------------------------------------------------------------------------------------------------------------------------------------
# affine
# ------------------------------------------------------------------------------------------------------------------------------------
SOURCES = ("gamma-beta", "gamma", "none", "emb")


def _affine_params(shape, source, g, scales, biases, groups=1, force=()):
    """mean, invstd [groups][c]; gamma, beta, emb, cls as the ABI takes them (None = a null pointer); scale, bias [n][c]."""
    n, c = shape[0], shape[3]
    pick = lambda vals, *size: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), size, generator=g)]      # noqa: E731
    mean = X.integers((groups, c), 8, g)
    invstd = pick([0.25, 0.5, 1.0, 2.0], groups, c)
    gamma = beta = emb = cls = None
    if source == "emb":
        emb = torch.cat((pick(scales, CLASSES, c), pick(biases, CLASSES, c)), 1)
        for i, v in enumerate(force):                          # (every class: whichever the batch uses)
            emb[:, i] = v
        cls = classes_of(n)
        scale, bias = emb[cls, :c], emb[cls, c:]
    else:
        gamma = pick(scales, c) if source != "none" else None
        for i, v in enumerate(force if gamma is not None else ()):
            gamma[i] = v
        beta = pick(biases, c) if source == "gamma-beta" else None
        scale = (gamma if gamma is not None else torch.ones(c, dtype=torch.float64)).expand(n, c)
        bias = (beta if beta is not None else torch.zeros(c, dtype=torch.float64)).expand(n, c)
    return mean, invstd, gamma, beta, emb, cls, scale, bias


def per_sample(stat, n, split):
    """[groups][c] statistics -> [n][1][1][c]."""
    idx = (torch.arange(n) >= split).long() if split else torch.zeros(n, dtype=torch.long)
    return stat[idx].view(n, 1, 1, -1)


def affine_case(dt, shape, source, act, split=0) -> Case:
    """sp_bn_apply / sp_bn_apply_pair (split > 0: [2][c] statistics) with chosen statistics; want: y in the storage type."""
    n, h, w, c = shape
    what = ("affine", NAME[dt], shape, source, act, split)
    g = X.gen(_seed(shape, 11 + SOURCES.index(source) + 4 * act + 16 * split))
    groups = 2 if split else 1
    mean, invstd, gamma, beta, emb, cls, scale, bias = _affine_params(shape, source, g, [-3, -2, -1, 0, 1, 2, 3], list(range(-8, 9)), groups, force=(0, -2, 3))
    if source != "none":
        assert bool((scale == 0).any()) and bool((scale < 0).any()), (what, "no zero / negative scale")
    if split:
        assert bool(((mean[0] != mean[1]) | (invstd[0] != invstd[1])).sum() > c // 2), what
    x = X.integers(shape, 15, g)
    a = scale.view(n, 1, 1, c) * per_sample(invstd, n, split)
    b = bias.view(n, 1, 1, c) - per_sample(mean, n, split) * a
    z = a * x + b
    for t in (a, b, a * x, z):
        assert torch.equal(t * 4, (t * 4).round()) and float(t.abs().max()) < 2 ** 20, (what, "not a multiple of 1/4 below 2^20")
    assert held(x, dt), what
    y = act64(z, act)
    return Case(regime="affine", what=what, dtype=dt, shape=shape, split=split, act=act, x=x, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                emb=emb, cls=cls, scale=scale, bias=bias, a=a, b=b, z=z, y=y, checks={"y": ("exact", expected(y, dt))})


def restate_apply(c: Case, same_stats=False, round16=False) -> Case:
    """bn_apply_kernel in fp32: a = scale invstd, b = bias - mean a, y = act(fma(a, x, b)) - the fma as the exact product and one add."""
    n = c.shape[0]
    split = 0 if same_stats else c.split
    a = c.scale.float().view(n, 1, 1, -1) * per_sample(c.invstd.float(), n, split)
    b = c.bias.float().view(n, 1, 1, -1) - per_sample(c.mean.float(), n, split) * a
    z = (a.double() * c.x + b.double()).float()                          # one rounding: the fma
    if round16:
        z = z.to(BF16 if c.dtype == F32 else c.dtype).float()
    y = z if c.act == ACT_NONE else torch.relu(z) if c.act == ACT_RELU else torch.maximum(z, z * np.float32(0.2))
    return Case(y=y.to(c.dtype))


# ------------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------------
def backward_case(dt, shape, source, act, up=False) -> Case:
    """sp_bn_backward with chosen statistics (up: sp_bn_backward_up2 of a 1 x 1 map - shape is that of u, x is u[:, :1, :1])."""
    n, h, w, c = shape
    what = ("backward", NAME[dt], shape, source, act)
    g = X.gen(_seed(shape, 41 + SOURCES.index(source) + 4 * act))
    mean, invstd, gamma, beta, emb, cls, scale, bias = _affine_params(shape, source, g, [-2, -1, -0.5, 0.5, 1, 2], [-8, -4, 4, 8])
    act_bias = source in ("gamma-beta", "emb")              # otherwise bias = 0: z = scale xhat, the kink sits at xhat = 0
    mu, isd = mean.view(1, 1, 1, c), invstd.view(1, 1, 1, c)
    sc, bi = scale.reshape(n, 1, 1, c), bias.reshape(n, 1, 1, c)
    q = torch.clamp(1.0 / (sc.abs() * isd), min=1.0)
    d = X.integers(shape, 12, g)
    if up:
        d = d[:, :1, :1].expand(shape).clone()               # (one source pixel per sample: no room for the conditions per channel)
    else:
        flat = d.view(n, h * w, c)
        flat[:, 0] = (-bi / (sc * isd * q))[:, 0, 0]           # z = 0 in every (sample, channel) ...
        flat[:, 1], flat[:, 2] = 12.0, -12.0                   # ... and both signs: |scale invstd q| >= 1, |bias| <= 8
    x = mu + d * q
    assert torch.equal(x, x.round()) and held(x, dt), what
    xh = (x - mu) * isd
    z = sc * xh + bi
    assert torch.equal(z * 8, (z * 8).round()) and float(xh.abs().max()) <= 24, what
    k = X.integers(shape, 8, g)
    dy = 5 * k
    assert held(dy, dt), what
    assert torch.equal(torch.from_numpy((dy.numpy().astype(np.float32) * np.float32(0.2)).astype(np.float64)), k), "fl32(0.2f x 5k) != k"
    per = lambda t: t.reshape(n, -1, c)                                                                           # noqa: E731
    if not up:
        assert bool((per(z) == 0).any(1).all()), (what, "no z = 0")
        assert bool((per(z) > 0).any(1).all()) and bool((per(z) < 0).any(1).all()), (what, "one sign of z only")
    differ = float(((z > 0) != (xh > 0)).double().mean())
    if act_bias and not up:
        assert differ >= 0.1, (what, "the sign of z follows xhat: %.3f" % differ)
    dz = torch.where(z > 0, dy, k) if act == ACT_LRELU else dy
    sa, sb = dz.sum((1, 2)), (dz * xh).sum((1, 2))                          # [n][c]
    assert torch.equal(sb * 4, (sb * 4).round()), what
    assert float(dz.abs().sum((1, 2)).sum(0).max()) < 2 ** 22 and float((dz * xh).abs().sum((1, 2)).sum(0).max()) < 2 ** 22, what
    count = n * h * w
    c1 = ((scale * sa).sum(0) / count).float().double()
    c2 = ((scale * sb).sum(0) / count).float().double()
    t1 = dz * sc
    t2 = t1 - c1
    t3 = xh * c2
    t4 = t2 - t3
    dx = isd * t4
    checks = {"c_tmp": ("exact", torch.cat((c1, c2)).float())}
    if emb is None:
        checks["dgamma"] = ("exact", sb.sum(0).float())
        checks["dbeta"] = ("exact", sa.sum(0).float())
    else:
        demb = torch.zeros(CLASSES, 2 * c, dtype=torch.float64)
        demb.index_add_(0, cls, torch.cat((sb, sa), 1))
        assert int((demb.abs().sum(1) == 0).sum()) >= 1, (what, "no unused class")
        checks["demb"] = ("exact", demb.float())
    dx_exact = all(f32_exact(t) for t in (t1, t2, t3, t4, dx))
    if dx_exact:
        checks["dx"] = ("exact", expected(dx, dt))
    else:
        e = isd * 3 * U32 * (t1.abs() + c1.abs() + t3.abs()) * SLACK
        checks["dx"] = ("within", dx, e + UREL[dt] * (dx.abs() + e) + ETA[dt])
    return Case(regime="backward", what=what, dtype=dt, shape=shape, act=act, x=x, dy=dy, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                emb=emb, cls=cls, scale=scale, bias=bias, z=z, xh=xh, dz=dz, dx_exact=dx_exact, differ=differ, checks=checks)


def restate_backward(c: Case, act_from_xhat=False, unmerged=False, unwritten=False, round16=False, drop_last=False, skip_row=False) -> Case:
    """bn_bwd_reduce_kernel -> bn_bwd_finalize_kernel -> bn_bwd_apply_kernel in fp32 / float64; the keywords plant faults."""
    dt, (n, h, w, ch) = c.dtype, c.shape
    r16 = (lambda t: t.to(BF16 if dt == F32 else dt).float()) if round16 else (lambda t: t)
    mu, isd = c.mean.float().view(1, 1, 1, ch), c.invstd.float().view(1, 1, 1, ch)
    sc, bi = c.scale.float().reshape(n, 1, 1, ch), c.bias.float().reshape(n, 1, 1, ch)
    x, dy = c.x.float(), c.dy.float()
    xh = (x - mu) * isd
    dz = dy
    if c.act == ACT_LRELU:
        dz = torch.where((xh if act_from_xhat else sc * xh + bi) > 0, dy, np.float32(0.2) * dy)
    blocks, pp = bwd_blocks(n, h * w, dt, ch), pix_par(dt, ch)
    owner = (torch.arange(h * w - (1 if drop_last else 0)) // pp) % blocks
    sa, sb = torch.zeros(n, ch, dtype=torch.float64), torch.zeros(n, ch, dtype=torch.float64)
    for i in range(n):
        part = torch.zeros(blocks, ch, 2, dtype=torch.float32)
        a2, b2 = dz[i].reshape(-1, ch), r16(dz[i] * xh[i]).reshape(-1, ch)
        part[:, :, 0].index_add_(0, owner, a2[:len(owner)])
        part[:, :, 1].index_add_(0, owner, b2[:len(owner)])
        tot = r16(part)[:blocks - 1 if skip_row and blocks > 1 else blocks].double().sum(0)
        sa[i], sb[i] = tot[:, 0], tot[:, 1]
    count = n * h * w
    s = c.scale.float().double()
    c1, c2 = ((s * sa).sum(0) / count).float(), ((s * sb).sum(0) / count).float()
    out = Case(c_tmp=torch.cat((c1, c2)))
    if c.emb is None:
        out.update(dgamma=sb.sum(0).float(), dbeta=sa.sum(0).float())
    else:
        rows = torch.cat((sb.float(), sa.float()), 1)
        demb = torch.full((CLASSES, 2 * ch), float("nan") if unwritten else 0.0)
        for i in range(n):
            k = int(c.cls[i])
            if bool((c.cls[:i] == k).any()):
                continue
            demb[k] = rows[i] if unmerged else rows[c.cls == k].sum(0)
        out.update(demb=demb)
    out.update(dx=(isd * (dz * sc - c1 - xh * c2)).to(dt))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# interp: the bilinear x2 kernels
# ------------------------------------------------------------------------------------------------------------------------------------
def axis_taps(i_ext):
    """Per output index o of 2 x i_ext: lower tap i0, upper tap i1, exact upper weight l, the fp32 position error E(o)."""
    o_ext = 2 * i_ext
    o = torch.arange(o_ext, dtype=torch.float64)
    pos = o * (i_ext - 1) / (o_ext - 1)
    i0 = torch.where(o == 0, torch.zeros_like(o), torch.floor((o - 1) / 2)).long()
    i1 = torch.clamp(i0 + 1, max=i_ext - 1)
    lam = torch.where(i1 > i0, pos - i0, torch.zeros_like(pos))
    assert float(lam.min()) >= 0 and float(lam.max()) < 1
    return i0, i1, lam, 2 * U32 * pos * (1 + U32)


def _near(t, dim, lo, hi, fn):
    """fn (amax / amin style reduction by torch.maximum) of t shifted by lo .. hi along dim, edges clamped."""
    size = t.shape[dim]
    out = None
    for s in range(lo, hi + 1):
        idx = torch.clamp(torch.arange(size) + s, 0, size - 1)
        v = t.index_select(dim, idx)
        out = v if out is None else fn(out, v)
    return out


def up2_reference(src):
    """float64 bilinear x2 (align_corners) of src [n][h][w][c] and B_up, the bound of the fp32 kernels' own error (before storage)."""
    n, h, w, c = src.shape
    h0, h1, lh, eh = axis_taps(h)
    w0, w1, lw, ew = axis_taps(w)
    rows = src[:, h0] * (1 - lh).view(1, -1, 1, 1) + src[:, h1] * lh.view(1, -1, 1, 1)
    ref = rows[:, :, w0] * (1 - lw).view(1, 1, -1, 1) + rows[:, :, w1] * lw.view(1, 1, -1, 1)
    dv = torch.zeros_like(src)
    dv[:, :h - 1] = (src[:, 1:] - src[:, :-1]).abs()                      # slope of the row segment (k, k + 1); 0 past the end
    dv = _near(dv, 1, -1, 1, torch.maximum)
    sh = torch.maximum(dv[:, h0][:, :, w0], dv[:, h0][:, :, w1])
    dw = torch.zeros_like(src)
    dw[:, :, :w - 1] = (src[:, :, 1:] - src[:, :, :-1]).abs()
    dw = _near(dw, 1, -1, 2, torch.maximum)
    sw = dw[:, h0][:, :, w0]
    m = _near(src.abs(), 1, -1, 2, torch.maximum)
    m = torch.maximum(m[:, h0][:, :, w0], m[:, h0][:, :, w1])
    blends = (4.0 if h > 1 else 0.0) + (4.0 if w > 1 else 0.0)
    bound = (eh.view(1, -1, 1, 1) * sh + ew.view(1, 1, -1, 1) * sw + blends * U32 * m) * SLACK
    return ref, bound


def stored(ref, err, dt):
    """The bound of a value with fp32 error `err` after its rounding to the storage type."""
    return err + UREL[dt] * (ref.abs() + err) + ETA[dt]


def up_fwd_case(dt, shape, gauss=False) -> Case:
    """sp_upsample2_fwd of integers (gauss: of N(0, 1) rounded through the storage type - the same bound)."""
    g = X.gen(_seed(shape, 71))
    x = torch.randn(*shape, generator=g).to(dt).double() if gauss else X.integers(shape, 15, g)
    assert held(x, dt)
    ref, b = up2_reference(x)
    identity = shape[1] == 1 and shape[2] == 1
    assert not identity or float(b.max()) == 0.0
    return Case(regime="interp", what=("up_fwd", NAME[dt], shape, gauss), dtype=dt, shape=shape, x=x,
                checks={"y": ("exact", expected(ref, dt)) if identity else ("within", ref, stored(ref, b, dt))})


def up_bwd_reference(dy):
    """float64 transpose of the bilinear x2 applied to dy [n][2h][2w][c], and the bound of the fp32 kernel's own error."""
    n, h, w, c = dy.shape[0], dy.shape[1] // 2, dy.shape[2] // 2, dy.shape[3]
    h0, h1, lh, eh = axis_taps(h)
    w0, w1, lw, ew = axis_taps(w)
    eh = torch.where(h1 > h0, eh, torch.zeros_like(eh))                   # a clamped upper tap folds both weights into one: 1 exactly
    ew = torch.where(w1 > w0, ew, torch.zeros_like(ew))

    def fold(t, dim, i0, i1, lo_w, hi_w, size):
        shape_w = [1, 1, 1, 1]
        shape_w[dim] = -1
        out_shape = list(t.shape)
        out_shape[dim] = size
        out = torch.zeros(out_shape, dtype=torch.float64)
        out.index_add_(dim, i0, t * lo_w.view(shape_w))
        out.index_add_(dim, i1, t * hi_w.view(shape_w))
        return out

    fh = lambda t, a, b_: fold(t, 1, h0, h1, a, b_, h)                                                         # noqa: E731
    fw = lambda t, a, b_: fold(t, 2, w0, w1, a, b_, w)                                                         # noqa: E731
    ref = fw(fh(dy, 1 - lh, lh), 1 - lw, lw)
    ady = dy.abs()
    mag = fw(fh(ady, 1 - lh, lh), 1 - lw, lw)
    err = fw(fh(ady, eh, eh), 1 - lw, lw) + fw(fh(ady, 1 - lh, lh), ew, ew) + fw(fh(ady, eh, eh), ew, ew)
    rounds = (6.0 if h > 1 else 4.0) + (6.0 if w > 1 else 4.0)            # an axis of extent 1: weights 0 and 1, only the additions round
    return ref, (err + rounds * U32 * mag) * SLACK, err


def up_bwd_case(dt, shape, gauss=False) -> Case:
    """sp_upsample2_bwd of integers (gauss: of rounded N(0, 1)) dy [n][2h][2w][c]; shape is that of dx."""
    n, h, w, c = shape
    g = X.gen(_seed(shape, 73))
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g).to(dt).double() if gauss else X.integers((n, 2 * h, 2 * w, c), 15, g)
    assert held(dy, dt)
    ref, b, err = up_bwd_reference(dy)
    identity = h == 1 and w == 1 and not gauss
    if identity:
        assert float(err.max()) == 0.0 and f32_exact(ref)
    return Case(regime="interp", what=("up_bwd", NAME[dt], shape, gauss), dtype=dt, shape=shape, dy=dy,
                checks={"dx": ("exact", expected(ref, dt)) if identity else ("within", ref, stored(ref, b, dt))})


def apply_up_case(dt, shape, source, act, split=0) -> Case:
    """sp_bn_apply_upsample2(_pair): the affine case's act(z), then the bilinear x2."""
    c = affine_case(dt, shape, source, act, split)
    ref, b = up2_reference(c.y)
    identity = shape[1] == 1 and shape[2] == 1
    c.update(regime="interp", what=("apply_up",) + c.what[1:],
             checks={"y": ("exact", expected(ref, dt)) if identity else ("within", ref, stored(ref, b, dt))})
    return c


def up_apply_case(dt, shape, source, act) -> Case:
    """sp_bn_apply_up2: u = up2(x) (rounded to 16-bit storage), then the affine case's z = a u + b and the activation."""
    c = affine_case(dt, shape, source, act)
    n, ch = shape[0], shape[3]
    u, bu = up2_reference(c.x)
    identity = shape[1] == 1 and shape[2] == 1
    if dt != F32:
        bu = bu + UREL[dt] * (u.abs() + bu)
    z = c.a * u + c.b
    bz = c.a.abs() * bu + 2 * U32 * (z.abs() + c.a.abs() * bu) * SLACK
    if identity:
        y = act64(z, act)
        checks = {"y": ("exact", expected(y, dt))}
    else:
        y = z if act == ACT_NONE else torch.relu(z) if act == ACT_RELU else torch.where(z > 0, z, 0.2 * z)
        checks = {"y": ("within", y, stored(y, bz, dt))}
    c.update(regime="interp", what=("up_apply",) + c.what[1:], checks=checks)
    return c


def restate_up2(src, dt, clamp_short=False, round16=False):
    """upsample2_fwd_kernel / the blend of bn_apply_upsample2_kernel in fp32: rows first, then columns, the weights from
    fl32(fl32((I - 1) / (2I - 1)) o) as the kernels form them.  src [n][h][w][c] fp32; returns fp32 (not yet stored)."""
    n, h, w, c = src.shape
    f = np.float32
    sh = f(h - 1) / f(2 * h - 1) if 2 * h > 1 else f(0)
    sw = f(w - 1) / f(2 * w - 1) if 2 * w > 1 else f(0)
    fh = (np.arange(2 * h, dtype=np.float32) * sh).astype(np.float32)
    h0 = fh.astype(np.int64)
    h1 = h0 + (h0 < h - 1)
    lh = torch.from_numpy(fh - h0.astype(np.float32)).view(1, -1, 1, 1)
    ow = np.arange(2 * w)
    w0 = np.where(ow == 0, 0, (ow - 1) >> 1)
    lw = torch.from_numpy(np.where(ow == 0, f(0), (ow.astype(np.float32) * sw).astype(np.float32) - w0.astype(np.float32)).astype(np.float32)).view(1, 1, -1, 1)
    top = w - 2 if clamp_short and w > 1 else w - 1
    wa, wb = np.minimum(w0, top), np.minimum(w0 + 1, top)
    rows = (1 - lh) * src[:, torch.from_numpy(h0)] + lh * src[:, torch.from_numpy(h1)]
    if round16:
        rows = rows.to(BF16 if dt == F32 else dt).float()
    return (1 - lw) * rows[:, :, torch.from_numpy(wa)] + lw * rows[:, :, torch.from_numpy(wb)]


def restate_up_bwd(dy, h, w):
    """upsample2_bwd_kernel in fp32: the four row weights first, then the four column weights (tap_weight's arithmetic)."""
    f = np.float32

    def weights(i_ext):
        o_ext = 2 * i_ext
        s = f(i_ext - 1) / f(o_ext - 1) if o_ext > 1 else f(0)
        wt = torch.zeros(i_ext, 4, dtype=torch.float32)
        idx = torch.zeros(i_ext, 4, dtype=torch.long)
        for i in range(i_ext):
            for j in range(4):
                o = 2 * i - 1 + j
                idx[i, j] = min(max(o, 0), o_ext - 1)
                if o < 0 or o >= o_ext:
                    continue
                i0 = 0 if o == 0 else (o - 1) >> 1
                lam = f(0) if o == 0 else f(s * f(o)) - f(i0)
                i1 = min(i0 + 1, i_ext - 1)
                wt[i, j] = float(f((f(1) - lam if i0 == i else f(0)) + (lam if i1 == i else f(0))))
        return wt, idx

    wh, ih = weights(h)
    ww, iw = weights(w)
    vs = torch.zeros(dy.shape[0], h, dy.shape[2], dy.shape[3], dtype=torch.float32)
    for j in range(4):
        vs = vs + wh[:, j].view(1, -1, 1, 1) * dy[:, ih[:, j]]
    out = torch.zeros(dy.shape[0], h, w, dy.shape[3], dtype=torch.float32)
    for j in range(4):
        out = out + ww[:, j].view(1, 1, -1, 1) * vs[:, :, iw[:, j]]
    return out


def restate_interp(c: Case, clamp_short=False, round16=False, same_stats=False) -> Case:
    kind, dt = c.what[0], c.dtype
    lrelu = lambda z: torch.maximum(z, z * np.float32(0.2))                                                     # noqa: E731
    if kind == "up_fwd":
        return Case(y=restate_up2(c.x.float(), dt, clamp_short, round16).to(dt))
    if kind == "up_bwd":
        return Case(dx=restate_up_bwd(c.dy.float(), c.shape[1], c.shape[2]).to(dt))
    if kind == "apply_up":
        low = Case(c)
        low.update(dtype=F32)                                    # the fused kernel blends act(z) in fp32, before any storage rounding
        src = restate_apply(low, same_stats).y
        return Case(y=restate_up2(src, dt, clamp_short, round16).to(dt))
    assert kind == "up_apply", kind
    u = restate_up2(c.x.float(), dt, clamp_short)
    if dt != F32:
        u = u.to(dt).float()
    z = (c.a.float().double() * u.double() + c.b.float().double()).float()
    y = z if c.act == ACT_NONE else torch.relu(z) if c.act == ACT_RELU else lrelu(z)
    return Case(y=y.to(dt))


# ------------------------------------------------------------------------------------------------------------------------------------
# dense: sp_bn_stats(_pair) -> sp_bn_apply(_pair) -> sp_bn_backward on Gaussian operands against float64
# ------------------------------------------------------------------------------------------------------------------------------------
S2 = 1.0 + 2.0 ** -9                   # second-order terms where every relative perturbation stays under 2^-10 (the plain chains)
UP2_DENSE_16 = [(2, 8, 8, 64), (3, 5, 7, 20), (2, 4, 8, 20), (4, 4, 4, 96), (3, 176, 2, 8)]
UP2_DENSE = [(2, 8, 8, 64), (3, 5, 7, 20), (2, 4, 8, 20), (4, 4, 4, 96), (1, 2, 3, 8), (3, 176, 2, 8)]     # the last: 3 x 352 rows asked of up2_grid
DENSE = [BASE, (1, 4, 16, 12), (2, 4, 8, 20), (4, 4, 4, 96), (2, 8, 8, 136), (3, 5, 7, 20), (2, 16, 16, 64)]


def _walk(pixels, blocks, pp):
    """The longest chain of dependent fp32 additions behind one partial row: a thread's grid-stride walk, then the block's lanes."""
    return -(-(-(-pixels // pp)) // blocks) + pp


def up2_walk(n, h, w, dt, c):
    """The longest chain of fp32 additions behind a partial row of the up2 reductions: rows per block x column steps x 4, then the lanes."""
    pp = pix_par(dt, c)
    nq = (2 * w + 2) // 4 + 1
    gx = min(max(1, (nq + pp - 1) // pp), max(1, MAX_PARTS // n))
    gy = up2_rows(n, h, w, dt, c) // gx
    return -(-2 * h // gy) * -(-nq // (gx * pp)) * 4 + pp


def _dense_params(source, n, c, rnd):
    """gamma, beta, emb, cls as the ABI takes them and scale, bias [n][c]: scale = 1 + 0.3 N, bias = 0.2 N, held by fp32."""
    gamma = beta = emb = cls = None
    if source == "emb":
        emb = torch.cat((1 + 0.3 * rnd(CLASSES, c), 0.2 * rnd(CLASSES, c)), 1).float().double()
        cls = classes_of(n)
        return gamma, beta, emb, cls, emb[cls, :c], emb[cls, c:]
    if source != "none":
        gamma = (1 + 0.3 * rnd(c)).float().double()
    if source == "gamma-beta":
        beta = (0.2 * rnd(c)).float().double()
    scale = (gamma if gamma is not None else torch.ones(c, dtype=torch.float64)).expand(n, c)
    bias = (beta if beta is not None else torch.zeros(c, dtype=torch.float64)).expand(n, c)
    return gamma, beta, emb, cls, scale, bias


def _dense_stats(x, e_u, groups, counts, walks, what, rel_max=2.0 ** -10):
    """Per group: float64 mean and invstd [groups][c], their bounds d_m and d_is, and the second-order factor s2."""
    mean, inv, d_m, d_is, s2 = [], [], [], [], S2
    for (lo, hi), cnt, k in zip(groups, counts, walks):
        xs, es = x[lo:hi], e_u[lo:hi]
        m, q = xs.mean((0, 1, 2)), (xs * xs).sum((0, 1, 2))
        var = q / cnt - m * m
        isd = 1.0 / torch.sqrt(var + EPS)
        ds = (k * U32 * xs.abs().sum((0, 1, 2)) + es.sum((0, 1, 2))) / cnt
        dvar = ((k + 1) * U32 * q + (2 * xs.abs() * es + es * es).sum((0, 1, 2))) / cnt + 2 * m.abs() * ds + ds * ds
        rel = float((dvar / (var + EPS)).max())
        assert rel < rel_max, what
        s2 = max(s2, 1.0 + 2.0 ** -9 + 4 * rel)               # (1 + d)^-1/2 and the products of two perturbations, d <= rel
        mean.append(m)
        inv.append(isd)
        d_m.append(ds + U32 * m.abs())
        d_is.append(isd * dvar / (2 * (var + EPS)) + U32 * isd)
    return torch.stack(mean), torch.stack(inv), torch.stack(d_m) * s2, torch.stack(d_is) * s2, s2


def _dense_forward(x, e_u, mu, isd, dm, dis, sc, bi, s2):
    """xhat, z and the bounds E_xh, E_z of what the kernels hold of them."""
    xc = x - mu
    xh = xc * isd
    z = sc * xh + bi
    e_xh = (isd * (dm + e_u) + xc.abs() * dis + 2 * U32 * xh.abs()) * s2
    e_z = (sc.abs() * (dis * xc.abs() + isd * (dm + e_u)) + U32 * ((sc * xh).abs() + 2 * (mu * sc * isd).abs() + bi.abs() + z.abs())) * s2
    return xh, z, e_xh, e_z


def dense_backward_checks(c: Case, dy) -> dict:
    """c_tmp, dgamma / dbeta or demb, dx of sp_bn_backward(_up2) for the gradient dy (stored operands, float64) on the case's forward:
    name -> ("within", float64 reference, bound), by the derivation of dense_case."""
    dt, (n, h, w, ch), s2 = c.dtype, c.shape, c.s2
    sc, scale, xh, e_xh, isd, dis = c.scale.reshape(n, 1, 1, ch), c.scale, c.xh, c.e_xh, c.isd, c.dis
    cnt = c.counts[0]
    neg = (c.z <= 0) if c.act == ACT_LRELU else torch.zeros_like(c.z, dtype=torch.bool)
    dz = torch.where(neg, 0.2 * dy, dy)
    e_dz = torch.where(neg, 1.1 * U32 * dz.abs(), torch.zeros_like(dz))
    sa, sb = dz.sum((1, 2)), (dz * xh).sum((1, 2))
    d_a = (e_dz.sum((1, 2)) + c.kb * U32 * dz.abs().sum((1, 2))) * s2
    d_b = ((dz.abs() * e_xh + e_dz * xh.abs() + U32 * (dz * xh).abs()).sum((1, 2)) + c.kb * U32 * (dz * xh).abs().sum((1, 2))) * s2
    c1, c2 = (scale * sa).sum(0) / cnt, (scale * sb).sum(0) / cnt
    d_c1 = ((scale.abs() * d_a).sum(0) / cnt + U32 * c1.abs()) * s2
    d_c2 = ((scale.abs() * d_b).sum(0) / cnt + U32 * c2.abs()) * s2
    checks = {"c_tmp": ("within", torch.cat((c1, c2)), torch.cat((d_c1, d_c2)))}
    if c.emb is None:
        checks["dgamma"] = ("within", sb.sum(0), (d_b.sum(0) + U32 * sb.sum(0).abs()) * s2)
        checks["dbeta"] = ("within", sa.sum(0), (d_a.sum(0) + U32 * sa.sum(0).abs()) * s2)
    else:
        rows, d_rows = torch.cat((sb, sa), 1), torch.cat((d_b, d_a), 1)
        demb, d_demb, mag = (torch.zeros(CLASSES, 2 * ch, dtype=torch.float64) for _ in range(3))
        demb.index_add_(0, c.cls, rows)
        d_demb.index_add_(0, c.cls, d_rows + U32 * rows.abs())
        mag.index_add_(0, c.cls, rows.abs())
        members = torch.bincount(c.cls, minlength=CLASSES).double().view(-1, 1)
        checks["demb"] = ("within", demb, (d_demb + (members - 1).clamp_min(0) * U32 * mag) * s2)
    t_mag = (dz * sc).abs() + c1.abs() + (xh * c2).abs()
    dx = isd * (dz * sc - c1 - xh * c2)
    e_dx = (isd * (e_dz * sc.abs() + d_c1 + e_xh * c2.abs() + xh.abs() * d_c2 + 4 * U32 * t_mag) + dis * dx.abs() / isd + U32 * dx.abs()) * s2
    checks["dx"] = ("within", dx, stored(dx, e_dx, dt))
    return checks


def _nudge_low(x_low, off, dt):
    """x_low with the heaviest tap of every offending output of its expansion moved by 1/4, rounded through the storage type."""
    n, h, w, c = x_low.shape
    th, tw = axis_taps(h), axis_taps(w)
    h0, w0 = torch.where(th[2] < 0.5, th[0], th[1]), torch.where(tw[2] < 0.5, tw[0], tw[1])
    hit = torch.zeros(x_low.shape, dtype=torch.float64)
    hit.index_put_((torch.arange(n).view(n, 1, 1, 1), h0.view(1, -1, 1, 1), w0.view(1, 1, -1, 1), torch.arange(c).view(1, 1, 1, c)),
                   off.double(), accumulate=True)
    return torch.where(hit > 0, x_low + 0.25, x_low).to(dt).double()


def dense_case(dt, shape, source, act, split=0, up=False, fused=False) -> Case:
    """x = 1.5 N(0, 1) + 0.3 and dy = N(0, 1) rounded through the storage type, scale = 1 + 0.3 N, bias = 0.2 N in fp32; the float64
    reference of the chain from these stored operands and, per element, the bounds (u32 = 2^-24; k = the longest chain of fp32
    additions behind a partial row, _walk; A = sum |x|, Q = sum x^2 over the group, M its pixel count):

        dS <= k u32 A, dQ <= (k + 1) u32 Q                  an fp32 sum of k terms is off by at most (k - 1) u32 sum |terms|; x x rounds
        d_m  = dS / M + u32 |m|                                                                   (mean_out is rounded to fp32)
        d_var = dQ / M + 2 |m| dS / M + (dS / M)^2,   d_is = is d_var / (2 (var + eps)) + u32 is  (asserted: d_var < 2^-10 (var + eps))
        E_xh = is d_m + |x - m| d_is + 2 u32 |xhat|                                              (x - mean and the product round)
        E_z  = |scale| (d_is |x - m| + is d_m) + u32 (|scale xhat| + 2 |m scale is| + |bias| + |z|)
               a = fl(scale is), b = fl(bias - fl(mean a)), z = fma(a, x, b): a's rounding acts on x - mean, b's own two roundings
               are absolute - they do not cancel when |mean| exceeds the spread
        E_y  = E_z + 2 u32 |z|                               LeakyReLU is 1-Lipschitz; its product rounds, 0.2f is off by 1.5e-8
        E_dz = 1.1 u32 |dz| where z <= 0, else 0              asserted: every |z| >= tau = 64 E_z and the backward's own z, off by at
                                                             most |scale| E_xh + 2 u32 (|scale xhat| + |z|), stays within tau too -
                                                             offending x were nudged by 1/4 until none was left; nothing is excluded
        d_a[n] = sum E_dz + k' u32 sum |dz|,   d_b[n] = sum (|dz| E_xh + E_dz |xhat| + u32 |dz xhat|) + k' u32 sum |dz xhat|
        d_c1 = sum_n |scale| d_a / M + u32 |c1|,  d_c2 likewise;  dgamma: sum_n d_b + u32 |dgamma|,  dbeta likewise;
        demb[k]: sum over the class's samples of d + u32 |s_n| (each sample's sum passes through fp32), + (members - 1) u32 sum |s_n|
        E_dx = is (E_dz |scale| + d_c1 + E_xh |c2| + |xhat| d_c2 + 4 u32 T) + d_is |dx| / is + u32 |dx|,  T = |dz scale| + |c1| + |xhat c2|
    every line times s2 = 1 + 2^-9 + 4 max d_var / (var + eps) for the second-order terms; values that are stored take urel (|ref| + E) + eta on top.

    up: the sp_bn_*_up2 chain.  shape is that of the stored x; the normalised tensor is u = up2(x), which the kernels hold with the
    error e_u = B_up (+ urel16 (|u| + B_up) + eta: 16-bit storage rounds u before it is used) per element.  Then every x above is
    the float64 u and dS gains sum e_u, dQ gains sum (2 |u| e_u + e_u^2), E_xh gains is e_u, E_z gains |scale| is e_u; k is
    up2_walk.  dx is du = d loss / d u; what sp_upsample2_bwd makes of the device's du is checked by up_bwd_reference.
    In 16-bit storage e_u is 2^-8 / 2^-11 of |u|: the bounds stand as derived but are that wide (d_var up to 2^-5 of var is
    admitted there, s2 grows with it).  tau = 64 E_z then covers a large share of all z in bf16 and 3.6 % in fp16, where moving a
    source pixel moves up to nine outputs and the nudging stalls at a handful of offenders: the 16-bit up2 chain is built without
    activation (asserted), where no kink exists.  What these wide bounds cannot see in the 16-bit up2 reductions, and the LeakyReLU
    backward, the constant maps hold exactly (sums_case / backward_case with rep).

    fused: the chain sp_bn_stats -> sp_bn_apply_upsample2(_pair) | sp_upsample2_bwd -> sp_bn_backward.  The fused apply blends
    act(z) in fp32: its reference is up2 of the float64 y with B_up of y plus the blend of E_y (the weights are positive and add
    up to 1, times 1 + 2 E for the rounded weights).  dy has the expanded shape; the backward's dy is what sp_upsample2_bwd left
    on the device, so its checks are built afterwards from that tensor (dense_backward_checks)."""
    assert not up or not (split or fused), "the up2 chain: one group"
    assert not (up and dt != F32 and act != ACT_NONE), "the 16-bit up2 chain has no tau to stand on: no activation"
    low = shape
    if up:
        shape = (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
    n, h, w, c = shape
    what = ("dense-up2" if up else "dense-fused" if fused else "dense", NAME[dt], shape, source, act, split)
    g = X.gen(_seed(shape, 91 + SOURCES.index(source) + 4 * act + 16 * split + 64 * fused))

    def rnd(*size):
        return torch.randn(*size, generator=g)

    x_low = x = (rnd(*low) * 1.5 + 0.3).to(dt).double()
    e_u = torch.zeros(shape, dtype=torch.float64)
    dy = rnd(n, 2 * h, 2 * w, c).to(dt).double() if fused else rnd(*shape).to(dt).double()
    gamma, beta, emb, cls, scale, bias = _dense_params(source, n, c, rnd)
    sc, bi = scale.reshape(n, 1, 1, c), bias.reshape(n, 1, 1, c)
    groups = [(0, split), (split, n)] if split else [(0, n)]
    counts = [(hi - lo) * h * w for lo, hi in groups]
    pp = pix_par(dt, c)
    blocks = pair_blocks(counts[0], counts[1], dt, c) if split else stat_blocks(counts[0], dt, c)
    walks = [up2_walk(n, low[1], low[2], dt, c) if up else _walk(cnt, blocks, pp) for cnt in counts]
    for _ in range(40):
        if up:
            x, e_u = up2_reference(x_low)
            if dt != F32:                                      # 16-bit storage rounds u before it is used
                e_u = e_u + UREL[dt] * (x.abs() + e_u) + ETA[dt]
        mean, inv, d_m, d_is, s2 = _dense_stats(x, e_u, groups, counts, walks, what, 2.0 ** -5 if up and dt != F32 else 2.0 ** -10)
        mu, isd, dm, dis = (per_sample(t, n, split) for t in (mean, inv, d_m, d_is))
        xh, z, e_xh, e_z = _dense_forward(x, e_u, mu, isd, dm, dis, sc, bi, s2)
        tau = 64 * e_z
        off = (z.abs() < tau) if act == ACT_LRELU else torch.zeros_like(z, dtype=torch.bool)
        if not bool(off.any()):
            break
        if up:
            x_low = _nudge_low(x_low, off, dt)
        else:
            x_low = x = torch.where(off, x + 0.25, x).to(dt).double()
    assert not bool(off.any()), (what, "an element stays within tau of the kink")
    if act == ACT_LRELU:
        assert bool(((sc.abs() * e_xh + 2 * U32 * ((sc * xh).abs() + z.abs())) * s2 <= tau).all()), what
    y = z if act == ACT_NONE else torch.where(z > 0, z, 0.2 * z)
    e_y = e_z + (2 * U32 * z.abs() if act == ACT_LRELU else 0.0)
    if fused:
        y_up, b_up = up2_reference(y)
        e_up = b_up + up2_reference(e_y)[0] * (1 + 2 * U32 * max(h, w))
        checks = {"mean": ("within", mean, d_m), "invstd": ("within", inv, d_is), "y": ("within", y_up, stored(y_up, e_up, dt))}
    else:
        checks = {"mean": ("within", mean, d_m), "invstd": ("within", inv, d_is), "y": ("within", y, stored(y, e_y, dt))}
    kb = up2_walk(n, low[1], low[2], dt, c) if up else _walk(h * w, bwd_blocks(n, h * w, dt, c), pp)
    out = Case(regime="dense", what=what, dtype=dt, shape=shape, split=split, act=act, up=up, fused=fused, x=x, x_low=x_low, dy=dy, gamma=gamma,
               beta=beta, emb=emb, cls=cls, scale=scale, bias=bias, groups=groups, counts=counts, first=0, momentum=float(np.float32(0.001)),
               rm0=torch.zeros(c, dtype=torch.float64), rv0=torch.ones(c, dtype=torch.float64), checks=checks,
               z=z, tau=tau, xh=xh, e_xh=e_xh, isd=isd, dis=dis, s2=s2, kb=kb)
    if not split and not fused:                                # the backward, from the statistics the device computed
        checks.update(dense_backward_checks(out, dy))
    return out


def lane_rows(vals, blocks, pp):
    """[blocks][c] fp32: the sum of vals [pixels][c] (fp32) per block in the kernels' own order - every thread adds its pixels in
    ascending order (pixel p belongs to lane p % pix_par of block (p // pix_par) % blocks), then the block adds its lanes in order."""
    pixels, c = vals.shape
    p = torch.arange(pixels)
    lanes = torch.zeros(blocks * pp, c, dtype=torch.float32)
    lanes.index_add_(0, ((p // pp) % blocks) * pp + p % pp, vals)
    lanes = lanes.view(blocks, pp, c)
    out = torch.zeros(blocks, c, dtype=torch.float32)
    for k in range(pp):
        out = out + lanes[:, k]
    return out


def restate_dense(c: Case, round16=False, same_stats=False, drop_last=False, act_from_xhat=False) -> Case:
    """The chain in fp32 as csrc/norm.hip states it (partial rows in the kernels' order, added in float64)."""
    dt, (n, h, w, ch) = c.dtype, c.shape
    r16 = (lambda t: t.to(BF16 if dt == F32 else dt).float()) if round16 else (lambda t: t)
    pp = pix_par(dt, ch)
    blocks = pair_blocks(c.counts[0], c.counts[1], dt, ch) if c.split else stat_blocks(c.counts[0], dt, ch)
    xk = c.x.float()
    if c.up:                                                   # (the partial rows in the plain kernels' order: any order has to pass)
        xk = restate_up2(c.x_low.float(), dt, round16=round16).to(dt).float()
    mean, inv = [], []
    for (lo, hi), cnt in zip(c.groups, c.counts):
        x2 = xk[lo:hi].reshape(-1, ch)
        if drop_last:
            x2 = x2[:-1]
        s, q = lane_rows(x2, blocks, pp).double().sum(0), r16(lane_rows(x2 * x2, blocks, pp)).double().sum(0)
        m = s / cnt
        var = (q / cnt - m * m).clamp_min(0)
        mean.append(m.float()), inv.append((1.0 / torch.sqrt(var + EPS)).float())
    mean, inv = torch.stack(mean), torch.stack(inv)
    split = 0 if same_stats else c.split
    mu, isd = per_sample(mean, n, split), per_sample(inv, n, split)
    sc, bi = c.scale.float().reshape(n, 1, 1, ch), c.bias.float().reshape(n, 1, 1, ch)
    x, dy = xk, c.dy.float()
    a = sc * isd
    b = bi - mu * a
    z = r16((a.double() * x.double() + b.double()).float())
    y = z if c.act == ACT_NONE else torch.maximum(z, z * np.float32(0.2))
    out = Case(mean=mean, invstd=inv, y=(restate_up2(y, dt, round16=round16) if c.fused else y).to(dt))
    if c.split:
        return out
    if c.fused:                                                # the backward's dy: what the fold of the expanded gradient stores
        dy = restate_up_bwd(dy, h, w).to(dt)
        out.update(dlow=dy)
        dy = dy.float()
    xh = (x - mu) * isd
    dz = dy if c.act == ACT_NONE else torch.where((xh if act_from_xhat else sc * xh + bi) > 0, dy, np.float32(0.2) * dy)
    bb = bwd_blocks(n, h * w, dt, ch)
    sa = torch.stack([lane_rows(dz[i].reshape(-1, ch), bb, pp).double().sum(0) for i in range(n)])
    sb = torch.stack([r16(lane_rows((dz[i] * xh[i]).reshape(-1, ch), bb, pp)).double().sum(0) for i in range(n)])
    s = c.scale.float().double()
    c1, c2 = ((s * sa).sum(0) / c.counts[0]).float(), ((s * sb).sum(0) / c.counts[0]).float()
    out.update(c_tmp=torch.cat((c1, c2)))
    if c.emb is None:
        out.update(dgamma=sb.sum(0).float(), dbeta=sa.sum(0).float())
    else:
        rows = torch.cat((sb.float(), sa.float()), 1)
        demb = torch.zeros(CLASSES, 2 * ch)
        for i in range(n):
            if not bool((c.cls[:i] == c.cls[i]).any()):
                members = (c.cls == c.cls[i]).nonzero().flatten().tolist()
                acc = rows[members[0]].clone()
                for j in members[1:]:
                    acc = acc + rows[j]
                demb[int(c.cls[i])] = acc
        out.update(demb=demb)
    out.update(dx=(isd * (dz * sc - c1 - xh * c2)).to(dt))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def compare(c: Case, got: Case, parts=None) -> float:
    """Every entry of c.checks against got[name]: torch.equal, or |got - reference| <= bound element for element (a NaN fails either).
    Returns the worst ratio of error to bound among the bounded comparisons (0 where all were exact)."""
    worst = 0.0
    for name, check in c.checks.items():
        if parts is not None and name not in parts:
            continue
        g = got[name].detach().cpu()
        tag = "%s %s" % (c.what, name)
        names = AXES if g.dim() == 4 else None
        if check[0] == "exact":
            assert_exact(g.reshape(check[1].shape), check[1], tag, names)
        else:
            assert g.dtype == (c.dtype if g.dim() == 4 else F32), (tag, g.dtype)
            worst = max(worst, assert_within(g.reshape(check[1].shape), check[1], check[2], tag, names))
    return worst
