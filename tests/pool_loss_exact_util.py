"""Operands, float64 references, CPU-checked conditions and the comparison for the tests of the pooling kernels (csrc/resample.hip) and
of the discriminator head and the losses (csrc/losses.hip): tests/test_gpu_pool_exact.py and tests/test_gpu_loss_exact.py; the
self-test of everything here: tests/test_pool_loss_harness.py.  Everything in this module runs on the CPU.  Activations are NHWC
[n][h][w][c] float64 unless said otherwise; a 2x2 window is scanned (0,0), (0,1), (1,0), (1,1).  The references are written from
the definitions in torch / numpy float64; fp32 appears in them only where the DEFINITION that is pinned contains an fp32 rounding.

pool-avg       sp_avgpool2_fwd/bwd, sp_act_avgpool2_fwd/bwd.  x = integers the storage type holds (|x| < 2^8 bf16, 2^11 fp16, 2^12
               fp32): the four-term sum and the x 0.25 are exact in fp32, the stored average is ONE round-to-nearest-even of the
               float64 value.  Every case plants the windows (M, M+1, M, M+1) and (M+1, M+2, M+1, M+2), M = 2^(p-1), and their
               negatives: averages M + 1/2 and M + 3/2 are exact ties of a p-bit format, one resolved downwards and one upwards, so
               truncation, round-half-up and round-half-away all show.  DEFINITION: y_act of sp_avgpool2_fwd is act of the UNROUNDED
               average, rounded once (the fused kernel never sees the stored average; torch on the stored tensor would round twice) -
               the builder asserts that the two definitions differ in the case.  LeakyReLU is max(v, fl32(0.2f v)), the product
               formed in float32 in the reference too.  sp_avgpool2_bwd is 0.25 dy: a power-of-two scaling, bit for bit.
               sp_act_avgpool2_bwd is dx = act'(x) ga + 0.25 gp with ga = 5 k, |k| <= 12: fl32(0.2f x 5k) = k exactly (0.2f exceeds
               1/5 by 1.49e-8 relative, below the half ulp 2^-25), so both terms and their sum (a multiple of 1/4 below 2^7) are
               exact.  Where x <= 0 the operands keep |k + 0.25 gp| > |k| / 2, so a compiler that contracts the product and the sum
               into one fma (exact product k (1 + 1.49e-8), one rounding at |k + 0.25 gp|) arrives at the same float.  x takes both
               signs, +0 and -0 in every channel group; the slope at x == 0 is 0.2 (0 for ReLU), as torch's.
pool-max       sp_maxpool2_fwd/bwd/bwd_idx.  Compared by value (torch.equal: -0 equals +0).  Windows are built from the 15 possible
               tie sets: the maximum sits at every single position, every pair, every triple and all four somewhere, the others
               strictly below; an all-negative and an all-zero window follow (relu = 1: the gradient must be 0 there).  The gradient
               goes to the FIRST maximum in scan order.  sp_maxpool2_bwd_idx reads two bits per pooled element from 32-bit words
               built HERE: from the float64 routing, and from a table that runs through all four codes in each of the 16 slots of
               every word; its pooled values take both signs and 0 (gate: m > 0).
pool-adaptive  sp_adaptive_avgpool_fwd/bwd.  Window [floor(o I / O), ceil((o + 1) I / O)).  Integer operands (multiples of 5 under an
               input LeakyReLU, gradients multiples of 20 there), so every window sum S is exact.  Where every window count is a power
               of two (8 -> 7, 4 -> 2, 2 -> 1, I -> I) results are exact.  Otherwise the kernel forms fl32(S fl32(1 / cnt)), two fp32
               roundings of a value |y|:
                   e = 2 x 2^-24 |y| (1 + 2^-20);   stored: e + urel (|y| + e) + eta
               (e = 0, and torch.equal, for the elements whose own count is a power of two).  Backward: input pixel (h, w) lies in at
               most two windows per axis, so dx = act'(x) sum of at most four products dy fl32(1 / cnt): e per term plus three
               additions of partial sums <= T = sum |dy / cnt|:
                   e_dx = 5 x 2^-24 T (1 + 2^-20),   under LeakyReLU at x <= 0: 0.2 e_dx + 2^-24 |dx|   (the product by 0.2f)
               (0 where every window over the pixel has a power-of-two count), then the storage rounding as above.
loss-sqerr     0.5 mean((p - t)^2), p integers with |p - t| <= 3, t in {0, 1}: every fp32 partial sum is an integer below 2^24
               (asserted per block of the multi-block kernel, with the launcher's grid formula restated).  The forward is
               fl32(exact) where n is a power of two (every quotient and sum is dyadic); otherwise within
                   (h + 2^-45 |exact|) (1 + 2^-20),   h = half the spacing of fp32 at |exact|
               - at most 256 double quotients and their atomic sums, each within 2^-53, then one rounding to float: the result is
               fl32(exact), or its neighbour where exact lies within 2^-45 |exact| of the midpoint.  h is 2^-25 |exact| only just
               below a power of two and reaches 2^-24 |exact| at one: a bound of (2^-25 + 2^-45) |exact| for every value, as first
               proposed for these tests, rejects fl32(exact) itself (n = 51200: exact 2.00845703125, nearest float 8.6e-8 away,
               2^-25 |exact| = 6.0e-8), so the spacing takes its place - no float but the nearest (two at a midpoint) passes.
               Backward: fl32(fl32(gout / n) d), restated in numpy float32, bit for bit (no additions:
               nothing to contract).
loss-dhead     pred[i][j][c] = x[j][c] E[cls[i]][c] + (wc . x[j] + bc) and its gradients.  |x|, |E| <= 3, |wc| <= 24, |dpred| <= 2, |bc| <= 9,
               B <= 20, F <= 264: every sum is an integer below 2^24 in any order (asserted), so pred, dE, dwc, dbc and the sdp
               scratch are exact and dx is one rounding to storage.  dE is compared over the WHOLE num_classes x F table: rows of
               absent classes are exactly 0.
loss-rec       sum over levels of mean(|maxpool(real) - maxpool(fake)| maxpool(mask)), pooling 2x2 (4-D levels) or pairs (2-D).
               Features are integers in [-2, 2], masks {0, 1} ({0, 1/2, 1, 2} in one case): block partials are multiples of 1/2
               below 2^24.  Where every level's count is a power of two each mean is dyadic, their double sum L is exact and the
               result is fl32(fl32(L) weight) bit for bit, weight in {1, 1/4}.  A level with another count (K = 365: 182 B) brings
               that level's blocks x 2^-53 |L_level| of double error: the result is within (h(L) + blocks 2^-53 |L_level|)
               (1 + 2^-20) weight, h as above.  Backward, bit for bit: g = fl32(fl32(gout weight) / fl32(count)); fl32(-g s m) at the FIRST
               maximum of the fake window, 0 elsewhere (by value), s = sign((r - f) m), rounded once to storage; the odd tail of a
               2-D level is written 0.  Levels of 64 windows and more contain ties inside fake windows, windows with r == f, zero-mask
               windows, and windows whose real and fake maxima sit at different positions (asserted).
loss-div       mean|z1 - z2| / (mean|img1 - img2| + 1e-8).  Integer images and z: both sums are exact.  out[0] and out[1] are the two
               double expressions of div_finalize_kernel restated in numpy float64, cast to float32, times weight in float32, bit for
               bit.  Backward: +-fl32(gout out[1]) by the sign of img1 - img2, 0 where the halves are equal (one element in eight is
               forced equal), rounded once to storage; gout is chosen so that the coefficient is a normal fp16 number.

urel is the relative error of one round-to-nearest into the storage type (2^-8 bf16, 2^-11 fp16, 2^-24 fp32); eta = 2^-25 covers
fp16's subnormals.  No element is excluded anywhere and no share of outliers is admitted."""
import numpy as np
import torch

import exact_util as X
from attention_exact_util import assert_within
from exact_util import Case, assert_exact, assert_sentinel, expected   # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (F32, BF16, F16)
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
UREL = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
ETA = {BF16: 0.0, F16: 2.0 ** -25, F32: 0.0}
U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
AXES = ["image", "row", "column", "channel"]
NUM_CLASSES = 301
F02 = np.float32(0.2)

# ---- shapes: the smallest that reach each edge -------------------------------------------------------------------------------------
POOL = [(1, 2, 2, 4), (2, 2, 6, 8), (2, 6, 2, 8), (1, 4, 4, 12), (3, 6, 10, 20), (2, 8, 12, 64), (1, 4, 4, 136)]
POOL_CLAMP = {F32: (1, 256, 256, 132), BF16: (1, 256, 256, 264), F16: (1, 256, 256, 264)}     # 128 x 128 x 33 items > 2048 x 256
IDX = [(2, 4, 4, 16), (1, 4, 6, 32), (3, 2, 4, 48)]
IDX_CLAMP = {F32: (1, 128, 128, 528), BF16: (1, 128, 128, 1040), F16: (1, 128, 128, 1040)}   # 64 x 64 x 132 / 130 items
# (n, h, w, c, oh, ow, act_in)
# 3 -> 2 (windows [0, 2), [1, 3)) and the upsampling 2 -> 3 (windows of 1, 2, 1) have power-of-two counts as well
ADAPTIVE_EXACT = [(2, 8, 8, 8, 7, 7, ACT_NONE), (2, 8, 8, 12, 7, 7, ACT_RELU), (3, 4, 4, 20, 2, 2, ACT_NONE), (5, 2, 2, 136, 1, 1, ACT_LRELU),
                  (1, 3, 3, 4, 2, 2, ACT_NONE), (2, 2, 2, 8, 3, 3, ACT_NONE), (2, 2, 2, 8, 3, 3, ACT_LRELU), (2, 5, 5, 8, 5, 5, ACT_NONE),
                  (2, 64, 64, 264, 64, 64, ACT_NONE)]                                                    # the last: 540672 items, two trips
ADAPTIVE_BOUND = [(2, 5, 5, 8, 3, 3, ACT_NONE), (2, 7, 7, 12, 3, 3, ACT_NONE), (3, 6, 10, 20, 3, 7, ACT_NONE), (2, 5, 5, 8, 3, 3, ACT_LRELU),
                  (2, 7, 7, 8, 3, 3, ACT_RELU), (1, 5, 7, 4, 2, 3, ACT_LRELU)]
DHEAD = [(1, 8), (2, 72), (3, 128), (5, 200), (8, 128), (20, 264), (8, 256), (3, 264), (5, 72), (20, 8)]          # (B, F)
CLASS_KINDS = ("equal", "distinct", "mix", "last")
SQERR = [1, 3, 4, 7, 4096, 16384, 16388, 20000, 51200, 51203, 1 << 18, (1 << 18) + 1, (1 << 18) + 5, 1 << 20]
SQERR_SMALL_MAX = 1 << 18                                            # sp_sqerr_loss_fwd: one block up to here
REC_4D = [(2, 2, 2, 4), (2, 4, 6, 8), (1, 8, 8, 20), (2, 128, 128, 132)]
REC_2D = [(2, 2), (3, 7), (2, 365), (2, 4096)]
REC_MAX_LEVELS = 8
DIV = [(48, 1), (1000, 128), (70000, 300), ((1 << 18) + 520, 128)]           # (half_elems, half_z): 256 forward blocks, 1024 backward blocks


def sid(shape):
    return "x".join(str(a) for a in shape)


def _seed(*parts):
    s = 12345
    for p in parts:
        for a in (p if isinstance(p, (tuple, list)) else (p,)):
            s = (s * 1000003 + (sum(map(ord, a)) if isinstance(a, str) else int(a))) % (1 << 31)
    return s


# ---- the launchers' plans, restated ------------------------------------------------------------------------------------------------
def vec(dt, c):
    return 4 if dt == F32 or c % 8 else 8


def pool_grid(items):
    """csrc/resample.hip: ew_grid."""
    return max(1, min(2048, (items + 255) // 256))


def ew_grid(items):
    """csrc/losses.hip: ew_grid."""
    return max(1, min(1024, (items + 255) // 256))


def red_grid(items):
    return min(256, ew_grid(items))


# ---- roundings ---------------------------------------------------------------------------------------------------------------------
def held(t, dt):
    return torch.equal(t.to(dt).double(), t)


def f32_exact(t):
    return torch.equal(t.float().double(), t)


def _bits(t):
    return t.float().contiguous().numpy().view(np.uint32)


def ties(t, dt):
    """Where the fp32-exact t lies exactly halfway between two neighbours of the 16-bit type (normal range)."""
    assert f32_exact(t)
    if dt == F32:
        return torch.zeros_like(t, dtype=torch.bool)
    low, half = (0xffff, 0x8000) if dt == BF16 else (0x1fff, 0x1000)
    return torch.from_numpy((_bits(t) & low) == half) & (t.abs() >= 2.0 ** -14)


def truncated(t32, dt):
    """The planted defect: the low bits are dropped instead of rounded."""
    if dt == F32:
        return t32.float()
    mask = np.uint32(0xffff0000 if dt == BF16 else 0xffffe000)
    return torch.from_numpy((_bits(t32) & mask).view(np.float32)).to(dt)


def store(t32, dt, trunc=False):
    return truncated(t32, dt) if trunc else t32.float().to(dt)


def act64(v, act):
    """act(v) of an fp32-exact v as the kernels form it: LeakyReLU = max(v, fl32(0.2f v))."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.relu(v)
    assert act == ACT_LRELU
    return X.lrelu_f32(v)


def act32(v32, act):
    if act == ACT_NONE:
        return v32
    if act == ACT_RELU:
        return torch.clamp_min(v32, 0.0)
    a = v32.numpy()
    return torch.from_numpy(np.maximum(a, F02 * a))


def stored(ref, err, dt):
    """The bound of a value with fp32 error `err` after its rounding to the storage type."""
    return err + UREL[dt] * (ref.abs() + err) + ETA[dt]


# ---- windows -----------------------------------------------------------------------------------------------------------------------
def windows(x):
    """[n][h][w][c] -> [n][h/2][w/2][c][4] in scan order."""
    return torch.stack((x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]), -1)


def unwindows(v):
    n, oh, ow, c, _ = v.shape
    x = torch.zeros(n, 2 * oh, 2 * ow, c, dtype=v.dtype)
    x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2] = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
    return x


def expand2(p):
    return p.repeat_interleave(2, 1).repeat_interleave(2, 2)


def first_max(v):
    """Index of the first maximum along the last axis, from the definition: the earliest position that equals the maximum."""
    eq = v == v.max(-1, keepdim=True).values
    return ((eq.cumsum(-1) == 1) & eq).long().argmax(-1)


def one_hot(best, k=4):
    return torch.nn.functional.one_hot(best, k).double()


def _signed_zeros(x, g):
    """Half of the zeros become -0."""
    flip = (x == 0) & (torch.rand(x.shape, generator=g) < 0.5)
    x[flip] = -0.0
    return x


def _plant_signs(x):
    """Window (0, 0) of image 0 holds a positive value, a negative one, +0 and -0 in every channel."""
    x[0, 0, 0], x[0, 0, 1], x[0, 1, 0], x[0, 1, 1] = x[0, 0, 0].abs() + 1, -x[0, 0, 1].abs() - 1, 0.0, -0.0
    return x


# ------------------------------------------------------------------------------------------------------------------------------------
# pool-avg
# ------------------------------------------------------------------------------------------------------------------------------------
def avg_case(dt, shape, act=ACT_LRELU) -> Case:
    """sp_avgpool2_fwd (y, y_act) and sp_avgpool2_bwd (dx of an integer dy)."""
    n, h, w, c = shape
    g = X.gen(_seed(shape, "avg", act))
    p = X.SIG_BITS[dt]
    amax = (1 << p) - 1
    x = X.integers(shape, amax, g)
    m = float(1 << (p - 1))
    a, b = torch.tensor([m, m + 1, m, m + 1]).double(), torch.tensor([m + 1, m + 2, m + 1, m + 2]).double()
    v = windows(x)
    for ch, pat in enumerate((a, b, -a, -b)):                      # c >= 4 everywhere
        v[0, 0, 0, ch::4] = pat
    x = unwindows(v)
    assert held(x, dt)
    avg = windows(x).sum(-1) * 0.25
    assert f32_exact(avg) and float(windows(x).abs().sum(-1).max()) < X.LIMIT
    ya = act64(avg, act)
    if dt != F32:
        t = ties(avg, dt)
        up = expected(avg, dt).double().abs() > avg.abs()
        assert bool((t & up).any()) and bool((t & ~up).any()), "no tie in both directions"
        if act == ACT_LRELU:
            twice = expected(act64(expected(avg, dt).double(), act), dt)
            assert not torch.equal(twice, expected(ya, dt)), "act of the stored average is the same tensor"
    dy = X.integers((n, h // 2, w // 2, c), amax, g)
    dx = expand2(dy) * 0.25
    assert held(dx, dt)
    return Case(dtype=dt, shape=shape, act=act, x=x, dy=dy, avg=avg, what=("avg", NAME[dt], shape, act),
                checks=dict(y=("exact", expected(avg, dt)), y_act=("exact", expected(ya, dt)), dx=("exact", expected(dx, dt))))


def restate_avg(c: Case, trunc=False, act_after=False) -> Case:
    dt = c.dtype
    v = windows(c.x.float())
    a = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    a = a * 0.25
    y = store(a, dt, trunc)
    ya = store(act32(y.float() if act_after else a, c.act), dt, trunc)
    return Case(y=y, y_act=ya, dx=store(expand2(c.dy.float()) * 0.25, dt, trunc))


FORMS = ("both", "ga", "gp")


def act_avg_case(dt, shape, act, form="both") -> Case:
    """sp_act_avgpool2_fwd (ya = act(x), yp = avgpool(x)) and sp_act_avgpool2_bwd (dx = act'(x) ga + 0.25 gp; form: which of the two
    gradients the call gets)."""
    n, h, w, c = shape
    g = X.gen(_seed(shape, "actavg", act, form))
    x = _plant_signs(_signed_zeros(X.integers(shape, 3, g), g))
    k = X.integers(shape, 12, g)
    gp = X.integers((n, h // 2, w // 2, c), 40, g)
    p = expand2(gp) * 0.25 if form != "ga" else torch.zeros(shape, dtype=torch.float64)
    if form == "gp":
        k = torch.zeros_like(k)
    if act == ACT_LRELU:                    # the sum must not cancel where the slope is 0.2f: with or without an fma the same float
        flip = (x <= 0) & (k != 0) & ((k + p).abs() <= 0.5 * k.abs())
        k = torch.where(flip, -k, k)
        assert not bool(((x <= 0) & (k != 0) & ((k + p).abs() <= 0.5 * k.abs())).any())
    ga = 5.0 * k
    lo = torch.from_numpy((F02 * ga.float().numpy()).astype(np.float64))
    assert act != ACT_LRELU or torch.equal(lo, k), "fl32(0.2f x 5k) != k"
    term = ga if act == ACT_NONE else torch.where(x > 0, ga, k if act == ACT_LRELU else torch.zeros_like(k))
    dx = term + p
    assert held(x, dt) and held(ga, dt) and held(gp, dt) and f32_exact(dx)
    for grp in range(c // 4):
        xs = x[..., 4 * grp:4 * grp + 4]
        neg0 = (xs == 0) & torch.signbit(xs)
        pos0 = (xs == 0) & ~torch.signbit(xs)
        assert bool((xs > 0).any()) and bool((xs < 0).any()) and bool(neg0.any()) and bool(pos0.any()), ("signs", grp)
    ya, yp = act64(x, act), windows(x).sum(-1) * 0.25
    return Case(dtype=dt, shape=shape, act=act, form=form, x=x, ga=None if form == "gp" else ga, gp=None if form == "ga" else gp,
                what=("act_avg", NAME[dt], shape, act, form),
                checks=dict(ya=("exact", expected(ya, dt)), yp=("exact", expected(yp, dt)), dx=("exact", expected(dx, dt))))


def restate_act_avg(c: Case, trunc=False, slope0=False) -> Case:
    dt, x = c.dtype, c.x.float()
    v = windows(x)
    a = (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]) * 0.25
    slope = np.float32(0.2 if c.act == ACT_LRELU else 0.0)
    fac = torch.where(x > 0, 1.0, float(slope)).float() if c.act != ACT_NONE else torch.ones_like(x)
    if slope0:
        fac = torch.where(x == 0, torch.zeros_like(fac), fac)
    gterm = c.ga.float() * fac if c.ga is not None else torch.zeros_like(x)
    pterm = expand2(c.gp.float() * 0.25) if c.gp is not None else torch.zeros_like(x)
    return Case(ya=store(act32(x, c.act), dt, trunc), yp=store(a, dt, trunc), dx=store(gterm + pterm, dt, trunc))


# ------------------------------------------------------------------------------------------------------------------------------------
# pool-max
# ------------------------------------------------------------------------------------------------------------------------------------
_TIE_SETS = torch.tensor([[(m >> k) & 1 for k in range(4)] for m in range(1, 16)] + [[1, 0, 1, 0], [1, 1, 1, 1]]).double()


def tie_windows(n, oh, ow, c, g):
    """[n][oh][ow][c][4] small integers: the window at flat index i takes tie set (i + 7 (i / c)) mod 17 (15: all negative, 16: all
    zero): c + 7 is no multiple of 17 for any channel count of the tables, so a channel sees another set at every pixel."""
    assert (c + 7) % 17
    idx = torch.arange(n * oh * ow * c).view(n, oh, ow, c)
    pat = (idx + 7 * (idx // c)) % 17
    base = X.integers((n, oh, ow, c), 2, g)
    low = torch.randint(1, 3, (n, oh, ow, c, 4), generator=g).double()
    v = base.unsqueeze(-1) - (1.0 - _TIE_SETS[pat]) * low
    v = torch.where((pat == 15).unsqueeze(-1), v - base.unsqueeze(-1) - 1.0, v)
    v = torch.where((pat == 16).unsqueeze(-1), torch.zeros_like(v), v)
    if idx.numel() >= 17:
        eq = v == v.max(-1, keepdim=True).values
        sets = set((eq.long() * torch.tensor([1, 2, 4, 8])).sum(-1).flatten().tolist())
        assert sets == set(range(1, 16)), "a tie set is missing"
        assert bool((v.max(-1).values < 0).any()) and bool((v == 0).all(-1).any())
    return v


def nonzero_integers(shape, amax, g):
    t = X.integers(shape, amax, g)
    t[t == 0] = 3.0
    return t


def max_case(dt, shape, relu=0) -> Case:
    n, h, w, c = shape
    g = X.gen(_seed(shape, "max", relu))
    v = tie_windows(n, h // 2, w // 2, c, g)
    x = unwindows(v)
    dy = nonzero_integers((n, h // 2, w // 2, c), 100, g)
    m = v.max(-1).values
    y = torch.relu(m) if relu else m
    gate = (m > 0).double() if relu else torch.ones_like(m)
    dx = unwindows(one_hot(first_max(v)) * (dy * gate).unsqueeze(-1))
    assert held(x, dt) and held(dy, dt)
    return Case(dtype=dt, shape=shape, relu=relu, x=x, dy=dy, what=("max", NAME[dt], shape, relu),
                checks=dict(y=("exact", expected(y, dt)), dx=("exact", expected(dx, dt))))


def restate_max(c: Case, last=False) -> Case:
    dt = c.dtype
    v = windows(c.x.float())
    m, best = v[..., 0], torch.zeros(v.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        gt = (v[..., k] >= m) if last else (v[..., k] > m)
        m, best = torch.where(gt, v[..., k], m), torch.where(gt, k, best)
    gv = c.dy.float() * ((m > 0).float() if c.relu else 1.0)
    return Case(y=store(torch.clamp_min(m, 0.0) if c.relu else m, dt), dx=store(unwindows(one_hot(best).float() * gv.unsqueeze(-1)), dt))


def pack_words(codes):
    """[n][oh][ow][c] codes 0..3 -> int32 [n oh ow][c / 16] holding the bits of the uint32 words (slot c & 15 of word c >> 4)."""
    c = codes.shape[-1]
    cd = codes.reshape(-1, c // 16, 16).long()
    words = (cd << (2 * torch.arange(16))).sum(-1)
    return torch.from_numpy(words.numpy().astype(np.uint32).view(np.int32).copy())


def max_idx_case(dt, shape, table) -> Case:
    """sp_maxpool2_bwd_idx.  table: "routing" (codes of the first maxima of tie_windows) | "slots" (all four codes in every slot)."""
    n, h, w, c = shape
    oh, ow = h // 2, w // 2
    g = X.gen(_seed(shape, "idx", table))
    if table == "routing":
        codes = first_max(tie_windows(n, oh, ow, c, g))
    else:
        ch = torch.arange(c).view(1, 1, 1, c)
        ppix = torch.arange(n * oh * ow).view(n, oh, ow, 1)
        codes = ((ch & 15) + ppix + (ch >> 4)) % 4
        per_slot = codes.reshape(-1, c // 16, 16)
        assert all(len(per_slot[:, wd, s].unique()) == 4 for wd in range(c // 16) for s in range(16)), "a slot misses a code"
    y = X.integers((n, oh, ow, c), 2, g)
    dy = nonzero_integers((n, oh, ow, c), 100, g)
    assert bool((y > 0).any()) and bool((y < 0).any()) and bool((y == 0).any())
    dx = unwindows(one_hot(codes) * (dy * (y > 0).double()).unsqueeze(-1))
    return Case(dtype=dt, shape=shape, y=y, dy=dy, codes=codes, words=pack_words(codes), what=("max_idx", NAME[dt], shape, table),
                checks=dict(dx=("exact", expected(dx, dt))))


def restate_max_idx(c: Case, word_off=0) -> Case:
    """Decodes the packed words as the kernel does: idx[ppix (C >> 4) + (c >> 4)] >> 2 (c & 15)."""
    n, h, w, ch = c.shape
    words = torch.from_numpy(c.words.numpy().view(np.uint32).astype(np.int64)).reshape(-1)
    cidx = torch.arange(ch)
    ppix = torch.arange(n * (h // 2) * (w // 2)).view(-1, 1)
    at = (ppix * (ch >> 4) + (cidx >> 4) + word_off) % words.numel()
    best = ((words[at] >> (2 * (cidx & 15))) & 3).view(n, h // 2, w // 2, ch)
    gv = torch.where(c.y.float() > 0, c.dy.float(), torch.zeros(()))
    return Case(dx=store(unwindows(one_hot(best).float() * gv.unsqueeze(-1)), c.dtype))


# ------------------------------------------------------------------------------------------------------------------------------------
# pool-adaptive
# ------------------------------------------------------------------------------------------------------------------------------------
def ad_bounds(i_ext, o_ext, floor_end=False):
    return [((o * i_ext) // o_ext, ((o + 1) * i_ext) // o_ext if floor_end else -((-(o + 1) * i_ext) // o_ext)) for o in range(o_ext)]


def _pow2(k):
    return k & (k - 1) == 0


def adaptive_case(dt, n, h, w, c, oh, ow, act_in) -> Case:
    g = X.gen(_seed((n, h, w, c, oh, ow), "adaptive", act_in))
    lrelu = act_in == ACT_LRELU
    x = X.integers((n, h, w, c), 12, g) * 5.0 if lrelu else X.integers((n, h, w, c), 100, g)
    x = _signed_zeros(x, g)
    x[0, 0, 0, 0::2], x[0, 0, 0, 1::2] = 0.0, -0.0
    dy = X.integers((n, oh, ow, c), 6, g) * 20.0 if lrelu else X.integers((n, oh, ow, c), 100, g)
    a = act64(x, act_in)
    assert held(x, dt) and held(dy, dt) and torch.equal(a, a.round())
    rows, cols = ad_bounds(h, oh), ad_bounds(w, ow)
    y = torch.zeros(n, oh, ow, c, dtype=torch.float64)
    cnt = torch.zeros(oh, ow, dtype=torch.long)
    acc, tsum = torch.zeros(n, h, w, c, dtype=torch.float64), torch.zeros(n, h, w, c, dtype=torch.float64)
    covers, rough = torch.zeros(h, w, dtype=torch.long), torch.zeros(h, w, dtype=torch.bool)
    for o, (h0, h1) in enumerate(rows):
        for q, (w0, w1) in enumerate(cols):
            k = (h1 - h0) * (w1 - w0)
            cnt[o, q] = k
            y[:, o, q] = a[:, h0:h1, w0:w1].sum((1, 2)) / k
            acc[:, h0:h1, w0:w1] += (dy[:, o, q] / k)[:, None, None]
            tsum[:, h0:h1, w0:w1] += (dy[:, o, q].abs() / k)[:, None, None]
            covers[h0:h1, w0:w1] += 1
            rough[h0:h1, w0:w1] |= not _pow2(k)
    assert int(covers.max()) <= 4 and int(covers.min()) >= 1
    p2 = torch.tensor([[_pow2(int(k)) for k in r] for r in cnt])
    exact = bool(p2.all())
    what = ("adaptive", NAME[dt], (n, h, w, c), (oh, ow), act_in)
    checks = {}
    # forward
    e = torch.where(p2.view(1, oh, ow, 1), 0.0, 2.0 * U32 * y.abs() * SLACK)
    if exact:
        assert f32_exact(y)
        checks["y"] = ("exact", expected(y, dt))
    else:
        assert bool((~p2).any())
        checks["y"] = ("within", y, stored(y, e, dt), dt)
        checks["y_pow2"] = ("exact_where", expected(y, dt), p2.view(1, oh, ow, 1).expand(n, oh, ow, c), "y")
    # backward
    smooth = ~rough.view(1, h, w, 1)
    e_dx = torch.where(smooth, 0.0, 5.0 * U32 * tsum * SLACK)
    if act_in == ACT_NONE:
        dx = acc
    elif act_in == ACT_RELU:
        dx, e_dx = torch.where(x > 0, acc, 0.0), torch.where(x > 0, e_dx, 0.0)
    else:
        neg = acc * float(F02)
        if exact:
            neg = torch.from_numpy((F02 * acc.float().numpy()).astype(np.float64))
            assert torch.equal(neg * 4, (neg * 4).round()), "0.2f x the pooled gradient is not exact"
        dx, e_dx = torch.where(x > 0, acc, neg), torch.where(x > 0, e_dx, 0.2 * e_dx + U32 * neg.abs())
    if exact:
        assert f32_exact(dx)
        checks["dx"] = ("exact", expected(dx, dt))
    else:
        checks["dx"] = ("within", dx, stored(dx, e_dx, dt), dt)
        where = smooth.expand(n, h, w, c) & ((x > 0) | (act_in != ACT_LRELU))
        checks["dx_pow2"] = ("exact_where", expected(dx, dt), where, "dx")
    return Case(dtype=dt, shape=(n, h, w, c), out=(oh, ow), act=act_in, x=x, dy=dy, exact=exact, what=what, checks=checks)


def restate_adaptive(c: Case, floor_end=False, trunc=False) -> Case:
    """The kernels' order: the window sum row by row, one multiplication by fl32(1 / cnt); the backward gathers o, then p."""
    dt, (n, h, w, ch), (oh, ow) = c.dtype, c.shape, c.out
    a = act32(c.x.float(), c.act)
    dy = c.dy.float()
    rows, cols = ad_bounds(h, oh, floor_end), ad_bounds(w, ow, floor_end)
    y = torch.zeros(n, oh, ow, ch)
    dx = torch.zeros(n, h, w, ch)
    for o, (h0, h1) in enumerate(rows):
        for q, (w0, w1) in enumerate(cols):
            s = torch.zeros(n, ch)
            for hh in range(h0, h1):
                for ww in range(w0, w1):
                    s = s + a[:, hh, ww]
            inv = float(np.float32(1.0) / np.float32(max(1, (h1 - h0) * (w1 - w0))))
            y[:, o, q] = s * inv
            dx[:, h0:h1, w0:w1] = dx[:, h0:h1, w0:w1] + (dy[:, o, q] * inv)[:, None, None]
    x = c.x.float()
    if c.act == ACT_LRELU:
        dx = torch.where(x > 0, dx, torch.from_numpy(F02 * dx.numpy()))
    elif c.act == ACT_RELU:
        dx = torch.where(x > 0, dx, torch.zeros(()))
    return Case(y=store(y, dt, trunc), dx=store(dx, dt, trunc))


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-sqerr
# ------------------------------------------------------------------------------------------------------------------------------------
def half_ulp32(v):
    """Half the spacing of fp32 at |v|: between 2^-25 |v| (just below a power of two) and 2^-24 |v| (at one)."""
    return 0.5 * float(np.spacing(np.float32(abs(v))))


def loss_bound(exact, blocks=256):
    """(half_ulp32(exact) + blocks x 2^-53 |exact|) (1 + 2^-20): the double quotients and atomic sums of `blocks` blocks, then one
    rounding to float."""
    return (half_ulp32(exact) + blocks * 2.0 ** -53 * abs(exact)) * SLACK


def sqerr_case(n, target, gout=0.7) -> Case:
    g = X.gen(_seed(n, "sqerr", int(target)))
    d = X.integers((n,), 3, g)
    d[-8:] = torch.where(d[-8:].abs() < 3, 3.0, d[-8:])            # the tail counts
    p = d + target
    s = float((d * d).sum())
    exact = 0.5 * s / n
    blocks = 1 if n <= SQERR_SMALL_MAX else red_grid(n)
    if blocks > 1:                                                 # block b: elements b 256 + t + k blocks 256
        pad = (-n) % (blocks * 256)
        per_block = torch.cat((d * d, torch.zeros(pad, dtype=torch.float64))).view(-1, blocks, 256).sum((0, 2))
        assert float(per_block.max()) < X.LIMIT and float(per_block.sum()) == s
    assert s < X.LIMIT if blocks == 1 else True
    d32 = d.numpy().astype(np.float32)
    gn = np.float32(gout) / np.float32(n)
    dp = torch.from_numpy((gn * d32).astype(np.float32))
    pow2 = _pow2(n)
    want = torch.tensor([exact], dtype=torch.float64)
    loss = ("exact", want.float()) if pow2 else ("within", want, torch.tensor([loss_bound(exact)], dtype=torch.float64), F32)
    assert not pow2 or float(want.float()) == exact
    return Case(n=n, target=float(target), gout=float(np.float32(gout)), p=p, blocks=blocks, exact=exact, what=("sqerr", n, target),
                checks=dict(loss=loss, dp=("exact", dp)))


def restate_sqerr(c: Case, drop_tail=False) -> Case:
    n, blocks = c.n, c.blocks
    d = c.p.numpy().astype(np.float32) - np.float32(c.target)
    sq = (d * d).astype(np.float64)                                # integers: every fp32 partial sum is exact in any order
    if drop_tail:
        sq[-1] = 0.0
    if blocks == 1:
        loss = np.float32(sq.sum() * 0.5 / float(n))
    else:
        pad = (-n) % (blocks * 256)
        tot = np.concatenate((sq, np.zeros(pad))).reshape(-1, blocks, 256).sum((0, 2)).astype(np.float32)
        acc = 0.0
        for t in tot:
            acc += float(t) * 0.5 / float(n)
        loss = np.float32(acc)
    gn = np.float32(c.gout) / np.float32(n)
    return Case(loss=torch.tensor([loss], dtype=torch.float32), dp=torch.from_numpy((gn * d).astype(np.float32)))


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-dhead
# ------------------------------------------------------------------------------------------------------------------------------------
def classes_of(kind, b):
    if kind == "equal":
        return torch.full((b,), 7, dtype=torch.int64)
    if kind == "distinct":
        return (torch.arange(b, dtype=torch.int64) * 13 + 2) % NUM_CLASSES
    if kind == "mix":
        return torch.tensor([5, 17, 5, 300, 17, 5, 41][:b] + [5, 300] * b, dtype=torch.int64)[:b]
    assert kind == "last"
    return torch.tensor([NUM_CLASSES - 1, 0, NUM_CLASSES - 1] * b, dtype=torch.int64)[:b]


def dhead_case(dt, b, f, kind) -> Case:
    g = X.gen(_seed((b, f), "dhead", kind))
    x, emb = X.integers((b, f), 3, g), X.integers((NUM_CLASSES, f), 3, g)
    wc, bc, dpred = X.integers((f,), 24, g), X.integers((1,), 9, g), X.integers((b, b, f), 2, g)
    cls = classes_of(kind, b)
    if kind == "distinct":
        assert len(cls.unique()) == b
    cl = x @ wc + bc                                                                     # [j]
    pred = x.unsqueeze(0) * emb[cls].unsqueeze(1) + cl.view(1, b, 1)
    sdp = dpred.sum((0, 2))                                                              # [j]
    dx = wc.unsqueeze(0) * sdp.unsqueeze(1) + (dpred * emb[cls].unsqueeze(1)).sum(0)
    de = torch.zeros(NUM_CLASSES, f, dtype=torch.float64)
    de.index_add_(0, cls, (dpred * x.unsqueeze(0)).sum(1))
    dwc, dbc = (x * sdp.unsqueeze(1)).sum(0), sdp.sum().view(1)
    s_max = 2 * b * f                                                                    # |sdp|
    bound = max(9 + 72 * f + 9, 24 * s_max + 6 * b, 6 * b * b, 3 * b * s_max, b * s_max)     # pred, dx, dE, dwc, dbc: sums of magnitudes
    assert bound < X.LIMIT and held(x, dt)
    if dt == F16:
        assert float(dx.abs().max()) < X.F16_MAX
    absent = torch.ones(NUM_CLASSES, dtype=torch.bool)
    absent[cls] = False
    assert bool((de[absent] == 0).all()) and int(absent.sum()) == NUM_CLASSES - len(cls.unique())
    return Case(dtype=dt, b=b, f=f, kind=kind, x=x, emb=emb, wc=wc, bc=bc, dpred=dpred, cls=cls, what=("dhead", NAME[dt], b, f, kind),
                checks=dict(pred=("exact", pred.float()), dx=("exact", expected(dx, dt)), demb=("exact", de.float()), dwc=("exact", dwc.float()),
                            dbc=("exact", dbc.float()), sdp=("exact", sdp.float())))


def restate_dhead(c: Case, last_writer=False, miss_last_row=False, trunc=False) -> Case:
    b, f = c.b, c.f
    x, emb, wc, dpred = c.x.float(), c.emb.float(), c.wc.float(), c.dpred.float()
    cls = c.cls.tolist()
    cl = (x * wc).sum(1) + c.bc.float()
    pred = torch.stack([x * emb[cls[i]] + cl.view(b, 1) for i in range(b)])
    sdp = torch.stack([dpred[:, j].sum() for j in range(b)])
    dx = torch.zeros(b, f)
    de = torch.zeros(NUM_CLASSES, f)
    for j in range(b):
        a = wc * sdp[j]
        for i in range(b):
            a = a + dpred[i, j] * emb[cls[i]]
        dx[j] = a
        if cls[j] not in cls[:j]:
            rows = [i for i in range(j, b) if cls[i] == cls[j]]
            if last_writer:
                rows = rows[-1:]
            gsum = torch.zeros(f)
            for i in rows:
                for k in range(b):
                    gsum = gsum + dpred[i, k] * x[k]
            de[cls[j]] = de[cls[j]] + gsum
    rows = b - b % 4 if miss_last_row else b
    dwc = torch.zeros(f)
    for j in range(rows):
        dwc = dwc + x[j] * sdp[j]
    return Case(pred=pred, dx=store(dx, c.dtype, trunc), demb=de, dwc=dwc, dbc=sdp.sum().view(1), sdp=sdp)


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-rec
# ------------------------------------------------------------------------------------------------------------------------------------
MASKS_01, MASKS_HALVES = (0.0, 1.0, 1.0), (0.0, 0.5, 1.0, 2.0)
LD_EXTRA = (3, 5, 7)                       # 2-D levels: row pitches of real, fake and dfake beyond K
# (levels, weight, mask values): one level; four levels, one-block and clamped ones mixed, one count no power of two; eight exact levels
REC_MULTI = [([(2, 4, 4, 8)], 1.0, MASKS_01),
             ([(2, 4, 6, 8), (2, 128, 128, 132), (2, 365), (2, 4096)], 0.25, MASKS_HALVES),
             ([(2, 2, 2, 4), (2, 4, 4, 8), (1, 8, 8, 16), (2, 2), (2, 4096), (4, 8), (1, 4, 4, 4), (2, 16)], 1.0, MASKS_01)]


def _pick(values, shape, g):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]


def _pairs(t):
    """[b][k] -> [b][k / 2][2] (the odd tail is dropped by the pool)."""
    k2 = t.shape[1] // 2
    return t[:, :2 * k2].reshape(t.shape[0], k2, 2)


def rec_level(dt, shape, gw, mask_values, seed) -> Case:
    """One pyramid level; shape (n, h, w, c) or (b, k).  gw = fl32(gout weight) of the call: dfake follows from it and the count."""
    g = X.gen(_seed(shape, "rec", seed))
    real, fake = X.integers(shape, 2, g), X.integers(shape, 2, g)
    four = len(shape) == 4
    mask = _pick(mask_values, shape[:3] if four else shape, g)
    if four:                                # a zero-mask window, and (where there is a second window) one whose first mask value is not its maximum
        mask[:, 0:2, 0:2] = 0.0
        if shape[2] >= 4:
            mask[:, 0, 2], mask[:, 0, 3] = 0.0, max(mask_values)
    else:
        mask[:, 0:2] = 0.0
        if shape[1] >= 4:
            mask[:, 2], mask[:, 3] = 0.0, max(mask_values)
    if four:
        n, h, w, c = shape
        wr, wf, wm = windows(real), windows(fake), windows(mask.unsqueeze(-1))
        items_f = items_b = n * (h // 2) * (w // 2) * (c // 4)
        count = n * (h // 2) * (w // 2) * c
    else:
        b, k = shape
        wr, wf, wm = _pairs(real), _pairs(fake), _pairs(mask)
        items_f, items_b, count = b * (k // 2), b * ((k + 1) // 2), b * (k // 2)
    r, f, m = wr.max(-1).values, wf.max(-1).values, wm.max(-1).values
    d = (r - f) * m
    total = float(d.abs().sum())
    if r.numel() >= 64:
        eqf = (wf == f.unsqueeze(-1)).sum(-1) > 1
        assert bool(eqf.any()), "no tie inside a fake window"
        assert bool(((r == f) & (m > 0)).any()) and bool((m == 0).any()) and bool(((m > 0) & (d != 0)).any())
        assert bool((first_max(wr) != first_max(wf)).any())
        assert bool((wm[..., 0] != wm.max(-1).values).any()), "the first mask value is the maximum everywhere"
    blocks_f, blocks_b = red_grid(items_f), ew_grid(items_b)
    per_block = 8.0 * (4 if four else 1) * -(-items_f // blocks_f)
    assert per_block < X.LIMIT and total * 2 == round(total * 2)
    gl = np.float32(gw) / np.float32(count)
    val = (np.float32(-gl) * torch.sign(d).numpy().astype(np.float32)) * m.expand_as(d).numpy().astype(np.float32)
    grad = one_hot(first_max(wf), wf.shape[-1]) * torch.from_numpy(val.astype(np.float64)).unsqueeze(-1)
    if four:
        dfake = unwindows(grad)
    else:
        dfake = torch.zeros(shape, dtype=torch.float64)
        dfake[:, :2 * (shape[1] // 2)] = grad.reshape(shape[0], -1)
    want = expected(dfake, dt)
    if dt == F16:
        nz = want.double().abs()[want != 0]
        assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -14, "a gradient is subnormal in fp16"
    return Case(shape=shape, four=four, real=real, fake=fake, mask=mask, count=count, total=total, mean=total / count, pow2=_pow2(count),
                blocks_f=blocks_f, blocks_b=blocks_b, dfake=want)


def rec_case(dt, shapes, weight=1.0, mask_values=MASKS_01, gout=5611.0) -> Case:
    gw = np.float32(gout) * np.float32(weight)
    levels = [rec_level(dt, s, gw, mask_values, i) for i, s in enumerate(shapes)]
    total = sum(lv.mean for lv in levels)                          # exact in double where every mean is dyadic
    w32 = np.float32(weight)
    pow2 = all(lv.pow2 for lv in levels)
    if pow2:
        loss = ("exact", torch.tensor([np.float32(total) * w32], dtype=torch.float32))
    else:
        bound = (half_ulp32(total) + sum(lv.blocks_f * 2.0 ** -53 * lv.mean for lv in levels if not lv.pow2)) * SLACK * float(w32)
        loss = ("within", torch.tensor([total * float(w32)], dtype=torch.float64), torch.tensor([bound], dtype=torch.float64), F32)
    checks = dict(loss=loss)
    for i, lv in enumerate(levels):
        checks["dfake%d" % i] = ("exact", lv.dfake)
    return Case(dtype=dt, levels=levels, weight=float(w32), gout=float(np.float32(gout)), pow2=pow2, total=total,
                what=("rec", NAME[dt], tuple(shapes), weight), checks=checks)


def restate_rec(c: Case, tail_unwritten=False, mask_first=False, count_c4=False, last_max=False, sentinel=-1536.0) -> Case:
    """fp32 block partials (exact), one double quotient per block added in block order, (float)acc * weight; the gradients with the
    kernels' own expressions."""
    dt = c.dtype
    acc = 0.0
    got = Case()
    gup = np.float32(c.gout) * np.float32(c.weight)
    for i, lv in enumerate(c.levels):
        real, fake, mask = lv.real.float(), lv.fake.float(), lv.mask.float()
        if lv.four:
            wr, wf, wm = windows(real), windows(fake), windows(mask.unsqueeze(-1))
            count = lv.count // 4 if count_c4 else lv.count
        else:
            wr, wf, wm = _pairs(real), _pairs(fake), _pairs(mask)
            count = lv.count
        m = wm[..., 0] if mask_first else wm.max(-1).values
        r, f = wr.max(-1).values, wf.max(-1).values
        terms = ((r - f) * m).abs().reshape(-1).double()
        per = -(-terms.numel() // lv.blocks_f)
        for blk in terms.split(per):
            acc += float(np.float32(float(blk.sum()))) / float(count)
        best = torch.zeros(f.shape, dtype=torch.long)
        fm = wf[..., 0]
        for k in range(1, wf.shape[-1]):
            gt = (wf[..., k] >= fm) if last_max else (wf[..., k] > fm)
            fm, best = torch.where(gt, wf[..., k], fm), torch.where(gt, k, best)
        d = (r - fm) * m
        gl = np.float32(gup) / np.float32(count)
        val = torch.from_numpy((np.float32(-gl) * torch.sign(d).numpy()) * m.expand_as(d).contiguous().numpy())
        grad = one_hot(best, wf.shape[-1]).float() * val.unsqueeze(-1)
        if lv.four:
            df = unwindows(grad)
        else:
            df = torch.full(lv.shape, sentinel if tail_unwritten else 0.0)
            df[:, :2 * (lv.shape[1] // 2)] = grad.reshape(lv.shape[0], -1)
        got["dfake%d" % i] = store(df, dt)
    got["loss"] = torch.tensor([np.float32(acc) * np.float32(c.weight)], dtype=torch.float32)
    return got


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-div
# ------------------------------------------------------------------------------------------------------------------------------------
def div_case(dt, half_elems, half_z, weight=1.0) -> Case:
    g = X.gen(_seed((half_elems, half_z), "div"))
    img = X.integers((2, half_elems), 7, g)
    same = torch.arange(half_elems) % 8 == 3
    img[1, same] = img[0, same]
    z = X.integers((2, half_z), 5, g)
    z[0, 0], z[1, 0] = 3.0, -1.0
    si, sz = float((img[0] - img[1]).abs().sum()), float((z[0] - z[1]).abs().sum())
    blocks = red_grid(half_elems)
    assert 14.0 * -(-half_elems // blocks) < X.LIMIT and 10.0 * half_z < X.LIMIT and si > 0 and held(img, dt)
    den, num = np.float64(si) / np.float64(half_elems), np.float64(sz) / np.float64(half_z)
    w32 = np.float32(weight)
    out0 = np.float32(num / (den + 1e-8)) * w32
    out1 = np.float32(-num / ((den + 1e-8) * (den + 1e-8)) / np.float64(half_elems)) * w32
    scale = 2.0 ** (-3 - int(np.floor(np.log2(abs(float(out1))))))                                           # |coef| in [1/8, 1/2)

    def rounds_up(mant):
        c64 = torch.tensor([float(np.float32(scale * mant) * out1)], dtype=torch.float64)
        return all(float(expected(c64, t).double().abs()) > float(c64.abs()) for t in (BF16, F16))
    mants = [1.0 + j / 128.0 for j in range(27, 128, 2)]
    mant = next((m for m in mants if rounds_up(m)), mants[0])     # where one exists: both 16-bit roundings go upwards, truncation shows
    gout = np.float32(scale * mant)
    coef = gout * out1
    assert 2.0 ** -14 <= abs(float(coef)) < 1.0
    s = torch.sign(img[0] - img[1])
    assert bool((s == 0).any()) and bool((s > 0).any()) and bool((s < 0).any())
    dimg = torch.stack((s * float(coef), -s * float(coef)))
    return Case(dtype=dt, half_elems=half_elems, half_z=half_z, weight=float(w32), gout=float(gout), rounds_up=rounds_up(mant), img=img, z=z, what=("div", NAME[dt], half_elems, half_z, weight),
                checks=dict(out=("exact", torch.tensor([out0, out1], dtype=torch.float32)), dimg=("exact", expected(dimg, dt))))


def restate_div(c: Case, trunc=False) -> Case:
    img, z = c.img.float(), c.z.float()
    si = float((img[0] - img[1]).abs().double().sum())              # integers: exact in fp32 per block and in the double atomics
    sz = float((z[0] - z[1]).abs().double().sum())
    den, num = si / float(c.half_elems), sz / float(c.half_z)
    w32 = np.float32(c.weight)
    out = np.array([np.float32(num / (den + 1e-8)) * w32, np.float32(-num / ((den + 1e-8) * (den + 1e-8)) / float(c.half_elems)) * w32], dtype=np.float32)
    coef = np.float32(c.gout) * out[1]
    s = torch.sign(img[0] - img[1])
    dimg = torch.stack((torch.from_numpy(coef * s.numpy()), torch.from_numpy(-coef * s.numpy())))
    return Case(out=torch.from_numpy(out), dimg=store(dimg, c.dtype, trunc))


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def compare(c: Case, got: Case, parts=None) -> float:
    """Every entry of c.checks against got: ("exact", want) torch.equal; ("within", reference, bound, dtype) |got - reference| <= bound
    element for element (a NaN fails either); ("exact_where", want, mask, name) torch.equal on the masked elements of got[name].
    parts: the names to look at (default: every check whose tensor is in got).  Returns the worst ratio of error to bound among the
    bounded comparisons (0 where all were exact)."""
    worst = 0.0
    for name, check in c.checks.items():
        src = check[3] if check[0] == "exact_where" else name
        if (parts is not None and src not in parts) or (parts is None and src not in got):
            continue
        g = got[src].detach().cpu()
        tag = "%s %s" % (c.what, name)
        names = AXES if check[1].dim() == 4 else None
        g = g.reshape(check[1].shape)
        if check[0] == "exact":
            assert_exact(g, check[1], tag, names)
        elif check[0] == "exact_where":
            assert_exact(torch.where(check[2], g, check[1]), check[1], tag, names)
        else:
            assert g.dtype == check[3], (tag, g.dtype)
            worst = max(worst, assert_within(g, check[1], check[2], tag, names))
    return worst
