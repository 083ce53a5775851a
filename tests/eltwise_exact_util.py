"""Operands, float64 references, CPU-checked conditions, fp32 restatements and the comparison for the tests of the element-wise glue
kernels (csrc/eltwise.hip, and sp_avgpool3s1_fwd / sp_global_avgpool_f32 of csrc/inception.hip): tests/test_gpu_eltwise_exact.py; the
self-test of everything here: tests/test_eltwise_harness.py.  Everything in this module runs on the CPU.  DESIGN.md section 21.

A case holds its operands IN THE STORAGE TYPE, laid out as the kernel reads them (input padding columns hold NaN), and for every
buffer the kernel writes a check over the WHOLE buffer body: the wanted values and a mask `keep` of the elements the contract says are
not written - those must still hold the canary the buffer was filled with.  Three kinds of comparison, in this order of preference:

exact       integer or dyadic operands chosen so that every fp32 intermediate is exact (asserted when the case is built): separate and
            fused multiply-add evaluation give the same float, `want` is ONE round-to-nearest-even of the float64 value into storage,
            torch.equal ("bits": the integer views are equal - pure copies, NaN payloads and -0 included).
restated    one fp32 operation followed by the storage rounding, nothing to contract: `want` is that expression in float32, bit for bit.
candidates  a product followed by a sum that the compiler may or may not contract: the element equals the storage rounding of the
            separate evaluation fl32(fl32(x y) + z) or that of the fused one fl32(x y + z).  The fused value is formed exactly: the
            product of two floats is exact in float64, and the sum is checked to be exact by its TwoSum remainder (fused32); any third
            value is rejected.
tanh        no exact regime: the float64 tanh of the held operand within e = 5 fp32 ulp (the accuracy OpenCL requires of tanh, which the
            device library is written to); a stored 16-bit element lies in [RN(ref - e), RN(ref + e)], roundings taken from float64
            directly.

No element is excluded anywhere and no share of outliers is admitted."""
import math
from fractions import Fraction

import numpy as np
import torch

import exact_util as X
import pool_loss_exact_util as P
from attention_exact_util import assert_within
from exact_util import SIG_BITS, Case, assert_exact, assert_sentinel          # noqa: F401
from pool_loss_exact_util import f32_exact, held, store

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (F32, BF16, F16)
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
CANARIES = (-1536.0, 768.0)                                        # held by all three storage types
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH)
F02 = np.float32(0.2)
NAN = float("nan")
TANH_ULPS = 5.0
INT_OF = {BF16: torch.int16, F16: torch.int16, F32: torch.int32}

# ---- shapes: the smallest that reach each edge -------------------------------------------------------------------------------------
TWO_TRIPS = 4 * (524288 + 37)                                     # 2048 x 256 groups of four and 37 more: a second trip for 37 threads
ACT_SIZES = [4, 1020, 1028, TWO_TRIPS]
ACT_BWD_VEC = [(5, 4, 4), (257, 8, 8), (8200, 256, 256)]           # (pixels, c, cp)
ACT_BWD_PAD = [(5, 3, 3), (7, 3, 4), (7, 3, 8), (4, 1, 4), (1030, 3, 8), (65600, 3, 8)]
SCALE_G = (0.0, 1.0, -3.0, 0.5)
SCALE_G_GENERAL = (0.3, -1.7, 1.1)
SCALE_BWD_SIZES = [4, 1028, 4 * (131072 + 37)]                     # the last: 512 blocks, 37 threads take a second trip
RESCALE_VEC = [(1, 4, 4, 8), (3, 64, 72, 64), (700, 64, 64, 64), (2100, 256, 256, 264)]          # (rows, c, ldx, ldy)
RESCALE_SCALAR = [(3, 365, 365, 365), (3, 365, 368, 368), (5, 366, 368, 368), (2, 64, 66, 64)]
SIG_EXACT = ((3.0, 77.0), (99.0, 0.5))                             # sig_a, sig_b: r = sig_a[0] sig_b[1] = 1.5; the other slots would change it
SIG_REAL = ((1.7320508, 0.57735026), (1.6180340, 0.61803401))      # {sigma, 1 / sigma} of two forwards
PERMUTE = [(1, 1, 1), (2, 3, 5), (3, 8, 64), (2, 512, 64), (2, 520, 509)]         # (B, C, HW); the last: 529360 items
CHANNEL_SUM = [(1, 3, 4), (5, 3, 3), (300, 6, 8), (450, 136, 136), (33, 1028, 1028), (5500, 12, 16), (16389, 1024, 1024)]   # (pixels, C, ld)
MASK_01, MASK_HALVES = (0.0, 1.0), (0.0, 0.5, 1.0, 2.0)             # products by powers of two: never rounded by the storage type
MASK_QUARTERS = (0.0, 0.75, 1.0, 1.5)                             # two more significand bits: the storage rounding acts
MASKS = (MASK_01, MASK_HALVES, MASK_QUARTERS)
MASK_MUL = [(1, 1, 1, 1), (3, 365, 365, 365), (3, 365, 368, 368), (2, 4096, 4096, 4100)]      # (B, K, ldf, ldo)
INGEST_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 16, 16), (3, 512, 512)]                   # (n, h, w); the last: 786432 pixels
INGEST_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F32, F16), (F16, F16)]   # (source, destination)
INGEST_LAYOUTS = ("nchw", "nhwc", "crop")
INGEST_SCALE, INGEST_SHIFT = (2.0, 0.5, -4.0), (1.0, -0.25, 3.0)
VGG_STD, VGG_MEAN = (0.229, 0.224, 0.225), (0.485, 0.456, 0.406)
VGG_SCALE, VGG_SHIFT = tuple(1.0 / s for s in VGG_STD), tuple(-m / s for m, s in zip(VGG_MEAN, VGG_STD))
AVG3 = [(1, 1, 1, 4), (2, 3, 3, 8), (2, 8, 5, 12), (1, 35, 35, 192)]               # (n, h, w, c)
GLOBAL_AVG = [(70, hw, 4) for hw in (1, 5, 64, 289)] + [(50, hw, 6) for hw in (1, 5, 64, 289)] + [(2, hw, 2048) for hw in (1, 5, 64, 289)]


def mask_concat_shapes(dt):
    return [(1, 4, 8), (128, 64, 68) if dt == F32 else (128, 64, 72), (8200, 252, 256)]         # (pixels, c, cp)


def sid(shape):
    return "x".join(str(a) for a in shape)


def sig(dt):
    """The operand limit of the storage type."""
    return (1 << SIG_BITS[dt]) - 1


_seed = P._seed


# ---- the launchers' plans, restated ------------------------------------------------------------------------------------------------
def grid_for(items):
    """csrc/eltwise.hip: grid_for."""
    return max(1, min(2048, (items + 255) // 256))


def scale_bwd_blocks(numel):
    return min(512, grid_for(numel // 4))


def channel_sum_plan(pixels, c):
    """(lanes per pixel, pixel lanes, blocks) of sp_channel_sum."""
    groups = (c + 3) // 4
    lanes = min(groups, 256)
    pix_par = 256 // lanes
    return lanes, pix_par, max(1, min(512, pixels // (pix_par * 32)))


def act_bwd_vector(pixels, c, cp):
    return c == cp and (pixels * c) % 4 == 0


def rescale_scalar(c, ldx, ldy):
    return bool((c & 3) or (ldx & 3) or (ldy & 3))


# ---- roundings ---------------------------------------------------------------------------------------------------------------------
def t32(a):
    """numpy float32 -> torch."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def n32(t):
    return t.float().contiguous().numpy()


def rn_direct(v64, dt):
    """ONE round-to-nearest-even of float64 values into the storage type (torch's double -> 16 bit passes through float: two)."""
    v = v64.double().numpy()
    if dt == F32:
        return torch.from_numpy(v.astype(np.float32))
    p, emin = (8, -126) if dt == BF16 else (11, -14)
    m, e = np.frexp(v)                                             # |m| in [0.5, 1)
    q = np.ldexp(1.0, np.maximum(e - p, emin - p + 1))             # the spacing at v (subnormals: the fixed one)
    r = np.rint(v / q) * q                                         # v / q: a power-of-two scaling, exact; rint: ties to even
    r = torch.from_numpy(r)
    out = r.to(dt)
    fin = out.isfinite()
    assert torch.equal(out.double()[fin], r[fin]), "rn_direct: the rounded value is not held"
    return out


def fused32(x, y, z):
    """fl32(x y + z) of float32 tensors, the value one fma gives.  x y is exact in float64 (48 bits); the float64 sum is exact where its
    TwoSum remainder is zero - asserted for every element, so the result is ONE rounding of the exact value."""
    p, zz = x.double() * y.double(), z.double()
    s = p + zz
    bb = s - p
    err = (p - (s - bb)) + (zz - bb)
    assert bool((err == 0).all()) and bool(s.isfinite().all()), "x y + z is not exact in float64"
    return s.float()


def fused_is_exact(x, y, z, picks):
    """The same claim in rationals, element by element at `picks`: float64(x) float64(y) + float64(z) IS the rational x y + z."""
    s = x.double() * y.double() + z.double()
    xf, yf, zf, sf = x.flatten(), y.flatten(), z.flatten(), s.flatten()
    return all(Fraction(float(xf[i])) * Fraction(float(yf[i])) + Fraction(float(zf[i])) == Fraction(float(sf[i])) for i in picks)


def separate32(x, y, z):
    return x.float() * y.float() + z.float()                       # two torch ops: two roundings


def as_bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def from_bits(bits, dt):
    return bits.to(INT_OF[dt]).contiguous().view(dt)


def decode(t, as_bf16=False):
    """The storage tensor as float32; as_bf16 (the planted defect): fp16 bits read as bf16."""
    if as_bf16 and t.dtype == F16:
        return t.contiguous().view(torch.int16).view(BF16).float()
    return t.float()


def body(numel, canary, dt):
    return torch.full((numel,), canary, dtype=dt)


def ulp32(ref64):
    """The fp32 ulp at the real number ref: 2^(floor(log2 |ref|) - 23), 2^-149 below the normal range."""
    _, e = np.frexp(ref64.double().numpy())
    return torch.from_numpy(np.ldexp(1.0, np.maximum(e - 24, -149)))


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def ints(shape, amax, g):
    return X.integers(shape, amax, g)


def lrelu_operands(dt, numel, g):
    """Integers |v| <= sig; every group of four holds +0 and -0 (at rotating slots) and the groups' other slots alternate between any
    integer and a multiple of 5."""
    s = sig(dt)
    x = ints((numel // 4, 4), s, g)
    grp = torch.arange(numel // 4)
    x[grp % 2 == 0] = (x[grp % 2 == 0] / 5).trunc() * 5
    x[grp, grp % 4] = 0.0
    x[grp, (grp + 1 + (grp // 4) % 3) % 4] = -0.0
    return x.reshape(-1)


def tanh_grid(dt):
    """Every bf16 value in [-9.5, 9.5], +-0 and +-inf; fp16: every value in that range (about as many); fp32: bit patterns at a stride of
    65521 (a prime next to bf16's 65536, so the low bits vary)."""
    if dt == BF16:
        pos = from_bits(torch.arange(0, 0x4118 + 1), BF16)
    elif dt == F16:
        pos = from_bits(torch.arange(0, 0x48C0 + 1), F16)
    else:
        pos = from_bits(torch.arange(0, 0x41180000 + 1, 65521), F32)
    assert float(pos.double().max()) <= 9.5 and bool(pos.isfinite().all())
    inf = torch.tensor([float("inf")], dtype=dt)
    return torch.cat((pos, -pos, inf, -inf))


def random_bits(dt, numel, g, quiet_nans=True):
    """Any bit pattern; NaNs carry random payloads (quiet_nans: with the quiet bit set), and +-0, +-inf and NaNs of both signs - one of
    them signalling unless quiet_nans - are planted at the front."""
    if dt == F32:
        b = torch.randint(-(1 << 31), 1 << 31, (numel,), generator=g, dtype=torch.int64)
        plant = [0, -(1 << 31), 0x7f800000, 0xff800000 - (1 << 32), 0x7fc00001, 0xffc12345 - (1 << 32), 0x7f800001, 0x7fffffff]
        if quiet_nans:
            nan = (b & 0x7f800000) == 0x7f800000
            b = torch.where(nan & ((b & 0x007fffff) != 0), b | 0x00400000, b)
            plant[6] = 0x7fc00002
    else:
        b = torch.randint(-(1 << 15), 1 << 15, (numel,), generator=g, dtype=torch.int64)
        exp, quiet = (0x7f80, 0x0040) if dt == BF16 else (0x7c00, 0x0200)
        plant = [0, -(1 << 15), exp, exp - (1 << 15), exp | quiet | 1, (exp | quiet | 0x15) - (1 << 15), exp | 1, 0x7fff]
        if quiet_nans:
            nan = ((b & exp) == exp) & ((b & (quiet * 2 - 1)) != 0)
            b = torch.where(nan, b | quiet, b)
            plant[6] = exp | quiet | 2
    k = min(numel, len(plant))
    b[:k] = torch.tensor(plant[:k])
    return from_bits(b, dt)


def quieted(x):
    """x as a conversion to float and back returns it: every NaN with its quiet bit set, sign and payload kept (IEEE 754 6.2: a
    format conversion delivers a quiet NaN, with the payload where it fits); everything else, subnormals included, unchanged.  fp32
    storage is moved as it is."""
    if x.dtype == F32:
        return x.clone()
    quiet = 0x0040 if x.dtype == BF16 else 0x0200
    bits = as_bits(x).long()
    return from_bits(torch.where(x.isnan(), bits | quiet, bits), x.dtype)


def pitched(t, ld):
    """[rows][c] -> the flat [rows x ld] operand with NaN in the padding columns."""
    rows, c = t.shape
    out = torch.full((rows, ld), NAN, dtype=t.dtype)
    out[:, :c] = t
    return out.reshape(-1)


def put(canary, dt, rows, ld, c, values, pad=None):
    """A [rows x ld] output body: values in columns [0, c); columns [c, ld) hold `pad` (None: unwritten, the canary)."""
    out = torch.full((rows, ld), canary if pad is None else pad, dtype=dt)
    out[:, :c] = values.reshape(rows, c)
    return out.reshape(-1)


def keep_cols(rows, ld, c):
    k = torch.zeros(rows, ld, dtype=torch.bool)
    k[:, c:] = True
    return k.reshape(-1)


def to_storage(v64, dt, what=""):
    assert held(v64, dt), ("the storage type does not hold an operand", what)
    return v64.to(dt)


def want_exact(v64, dt):
    assert f32_exact(v64), "the reference is not exact in fp32"
    return X.expected(v64, dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_act_fwd
# ------------------------------------------------------------------------------------------------------------------------------------
def act64(x, act):
    """The definition on the held operand, float64 (LeakyReLU: max(v, fl32(0.2f v)), the product formed in float32)."""
    v = x.double()
    if act == ACT_LRELU:
        return torch.maximum(v, t32(F02 * n32(x)).double())
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))           # NaN -> 0: fmaxf(NaN, 0) and the conv epilogues' v > 0 ? v : 0
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def act_fwd_case(dt, numel, act) -> Case:
    g = X.gen(_seed(numel, "act_fwd", act))
    assert numel % 4 == 0
    what = ("act_fwd", NAME[dt], numel, act)
    if act == ACT_NONE:
        x = random_bits(dt, numel, g, quiet_nans=False)
        assert dt == F32 or not torch.equal(as_bits(quieted(x)), as_bits(x)) or numel < 8, "no signalling NaN among the operands"
        return Case(dtype=dt, numel=numel, act=act, x=x, what=what, checks=dict(y=("bits", quieted(x), None)))
    if act == ACT_TANH:
        grid = tanh_grid(dt)
        idx = torch.arange(numel) % grid.numel() if numel >= grid.numel() else torch.linspace(0, grid.numel() - 1, numel).long()
        x = grid[idx].contiguous()
        return Case(dtype=dt, numel=numel, act=act, x=x, what=what, checks=dict(y=tanh_check(x, dt)))
    x = to_storage(lrelu_operands(dt, numel, g), dt)
    x5 = x.double()[(x.double() % 5 == 0)]
    assert torch.equal(t32(F02 * n32(x5)).double(), x5 / 5) and x5.numel() >= numel // 4, "fl32(0.2f x 5k) != k"
    grp = x.double().view(-1, 4)
    assert bool(((grp == 0) & torch.signbit(grp)).any(1).all()) and bool(((grp == 0) & ~torch.signbit(grp)).any(1).all())
    ref = act64(x, act)
    return Case(dtype=dt, numel=numel, act=act, x=x, what=what, checks=dict(y=("bits" if act == ACT_LRELU else "exact", want_exact(ref, dt), None)))


def tanh_check(x, dt):
    ref = torch.tanh(x.double())
    e = TANH_ULPS * ulp32(ref)
    e[ref == 0] = 0.0
    e[x.double().isinf()] = 0.0                                    # tanh(+-inf) = +-1 exactly
    lo, hi = rn_direct(ref - e, dt), rn_direct(ref + e, dt)
    assert bool((lo.double() <= hi.double())[~ref.isnan()].all())
    return ("tanh", ref, None, lo, hi, e)


SPECIAL_IN = [float("inf"), float("-inf"), NAN, -NAN, 1.0, -1.0, 0.0, -0.0]
SPECIAL_OUT = {ACT_NONE: SPECIAL_IN,
               ACT_LRELU: [float("inf"), float("-inf"), NAN, NAN, 1.0, -0.2, 0.0, -0.0],
               ACT_RELU: [float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
               ACT_TANH: [1.0, -1.0, NAN, NAN, math.tanh(1.0), -math.tanh(1.0), 0.0, -0.0]}


def act_special_case(dt, act) -> Case:
    """The table of DESIGN.md 21: NaN passes through NONE, LeakyReLU and tanh; ReLU(NaN) = 0."""
    x = torch.tensor(SPECIAL_IN, dtype=torch.float64).to(dt)
    table = torch.tensor(SPECIAL_OUT[act], dtype=torch.float64)
    ref = act64(x, act)
    assert torch.equal(ref.isnan(), table.isnan()) and bool(((ref - table).abs()[~ref.isnan() & ~ref.isinf()] < 1e-6).all()), "the table"
    check = tanh_check(x, dt) if act == ACT_TANH else ("exact", rn_direct(ref, dt), None)
    return Case(dtype=dt, numel=8, act=act, x=x, what=("act_special", NAME[dt], act), checks=dict(y=check))


def act32(v, act, slope0=False):
    if act == ACT_LRELU:
        out = torch.maximum(v, t32(F02 * n32(v)))
        return torch.where(v == 0, torch.zeros_like(v), out) if slope0 else out
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def restate_act_fwd(c: Case, canary=CANARIES[0], trunc=False, skip_tail=False, one_trip=False, as_bf16=False, raw_copy=False) -> Case:
    dt = c.dtype
    if c.act == ACT_NONE and not as_bf16:
        y = c.x.clone() if raw_copy else quieted(c.x)
    else:
        y = store(act32(decode(c.x, as_bf16), c.act), dt, trunc)
    out = body(c.numel, canary, dt)
    n = c.numel - 4 if skip_tail else c.numel
    n = min(n, 4 * 2048 * 256) if one_trip else n
    out[:n] = y[:n]
    return Case(y=out)


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_act_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
def act_bwd_case(dt, pixels, c, cp, act) -> Case:
    g = X.gen(_seed((pixels, c, cp), "act_bwd", act))
    s = sig(dt)
    shape = (pixels, c)
    if act == ACT_TANH:
        j = ints(shape, 16, g)
        y, dy = j / 16.0, ints(shape, s, g)
        dz = dy * (256.0 - j * j) / 256.0
        assert f32_exact(dy * (256.0 - j * j)) and float((dy * (256.0 - j * j)).abs().max()) < X.LIMIT
    else:
        y = ints(shape, 3, g)
        flat = y.view(-1)
        idx = torch.arange(flat.numel())
        flat[idx % 7 == 0] = 0.0
        flat[idx % 7 == 3] = -0.0
        k = ints(shape, s // 5, g)
        flat[1], flat[2] = 2.0, -2.0                                # y and dy of opposite signs: a slope chosen by dy shows
        k.view(-1)[1], k.view(-1)[2] = -1.0, 1.0
        dy = 5.0 * k
        if act == ACT_LRELU:
            assert torch.equal(t32(F02 * n32(dy)).double(), k), "fl32(0.2f x 5k) != k"
        dz = dy if act == ACT_NONE else torch.where(y > 0, dy, k if act == ACT_LRELU else torch.zeros_like(k))
        if flat.numel() >= 8:
            assert bool((y > 0).any()) and bool((y < 0).any()) and bool(((y == 0) & torch.signbit(y)).any()) and bool(((y == 0) & ~torch.signbit(y)).any())
            assert bool(((y <= 0) & (dy > 0)).any()) and bool(((y > 0) & (dy < 0)).any()), "y and dy never disagree in sign"
    want = put(0.0, dt, pixels, cp, c, want_exact(dz, dt), pad=0.0)
    return Case(dtype=dt, pixels=pixels, c=c, cp=cp, act=act, dy=to_storage(dy, dt).reshape(-1), y=to_storage(y, dt).reshape(-1),
                vector=act_bwd_vector(pixels, c, cp), what=("act_bwd", NAME[dt], (pixels, c, cp), act), checks=dict(dz=("exact", want, None)))


def restate_act_bwd(c: Case, canary=CANARIES[0], trunc=False, slope0=False, by_dy=False, pad="zero", one_trip=False, as_bf16=False) -> Case:
    """pad: "zero" | "unwritten" | "neighbour" (the planted defects)."""
    dt = c.dtype
    dy, y = decode(c.dy, as_bf16).view(c.pixels, c.c), decode(c.y, as_bf16).view(c.pixels, c.c)
    sel = dy if by_dy else y
    if c.act == ACT_LRELU:
        low = t32(F02 * n32(dy))
        d = torch.where(sel > 0, dy, low)
        if slope0:
            d = torch.where(sel == 0, torch.zeros_like(d), d)
    elif c.act == ACT_RELU:
        d = torch.where(sel > 0, dy, torch.zeros_like(dy))
    elif c.act == ACT_TANH:
        d = dy * (1.0 - y * y)
    else:
        d = dy
    out = torch.full((c.pixels, c.cp), canary if pad == "unwritten" else 0.0, dtype=dt)
    out[:, :c.c] = store(d, dt, trunc)
    if pad == "neighbour" and c.cp > c.c:
        out[:, c.c:] = out[:, c.c - 1:c.c]
    out = out.reshape(-1)
    if one_trip:
        first = (4 if c.vector else 1) * 2048 * 256
        out[first:] = canary
    return Case(dz=out)


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_scale_add, sp_scale_add_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
def scale_add_case(dt, numel, gv) -> Case:
    """y = g a + b.  g in SCALE_G: exact; any other g: candidates."""
    g = X.gen(_seed(numel, "scale_add", int(gv * 1000)))
    s = sig(dt)
    a, b = ints((numel,), s, g), ints((numel,), s, g)
    g32 = torch.tensor([gv], dtype=torch.float32)
    a_s, b_s = to_storage(a, dt), to_storage(b, dt)
    what = ("scale_add", NAME[dt], numel, gv)
    if gv in SCALE_G:
        ref = float(g32) * a + b
        check = ("exact", want_exact(ref, dt), None)
    else:
        sep, fus = separate32(g32, a_s.float(), b_s.float()), fused32(g32, a_s.float(), b_s.float())
        check = ("candidates", store(sep, dt), None, store(fus, dt))
    return Case(dtype=dt, numel=numel, a=a_s, b=b_s, g=g32, what=what, checks=dict(y=check))


def restate_scale_add(c: Case, canary=CANARIES[0], trunc=False, skip_tail=False, one_trip=False, fused=False, as_bf16=False) -> Case:
    a, b = decode(c.a, as_bf16), decode(c.b, as_bf16)
    v = fused32(c.g, a, b) if fused else separate32(c.g, a, b)
    out = body(c.numel, canary, c.dtype)
    n = c.numel - 4 if skip_tail else c.numel
    n = min(n, 4 * 2048 * 256) if one_trip else n
    out[:n] = store(v, c.dtype, trunc)[:n]
    return Case(y=out)


def block_sums(prod, blocks):
    """Per-block sums of the grid-stride loop over groups of four: group i belongs to block (i / 256) mod blocks."""
    n4 = prod.numel() // 4
    per = prod.view(n4, 4).sum(1)
    owner = (torch.arange(n4) // 256) % blocks
    return torch.zeros(blocks, dtype=torch.float64).index_add_(0, owner, per)


def scale_add_bwd_case(dt, numel, gv) -> Case:
    g = X.gen(_seed(numel, "scale_add_bwd", int(gv * 1000)))
    dy, a = ints((numel,), 15, g), X.ternary((numel,), g)
    dy[-4:], a[-4:] = torch.tensor([15.0, -15.0, 7.0, 15.0]), torch.tensor([1.0, -1.0, 1.0, 1.0])          # the tail counts
    assert float((dy * a).abs().sum()) < X.LIMIT, "sum |dy a| reaches 2^24"
    g32 = torch.tensor([gv], dtype=torch.float32)
    dy_s = to_storage(dy, dt)
    blocks = scale_bwd_blocks(numel)
    part = torch.zeros(512, dtype=torch.float32)
    part[:blocks] = block_sums(dy * a, blocks).float()
    keep = torch.arange(512) >= blocks
    da = store(t32(n32(g32) * n32(dy_s)), dt)                       # restated: one product, one storage rounding
    dg = torch.tensor([float((dy * a).sum())], dtype=torch.float32)
    assert float(dg) == float((dy * a).sum()) and float(block_sums(dy * a, blocks).sum()) == float(dg)
    return Case(dtype=dt, numel=numel, dy=dy_s, a=to_storage(a, dt), g=g32, blocks=blocks, what=("scale_add_bwd", NAME[dt], numel, gv),
                checks=dict(da=("exact", da, None), dg=("exact", dg, None), partials=("exact", part, keep)))


def restate_scale_add_bwd(c: Case, canary=CANARIES[0], trunc=False, skip_tail=False, one_trip=False, as_bf16=False) -> Case:
    dt = c.dtype
    dy, a = decode(c.dy, as_bf16), decode(c.a, as_bf16)
    n = c.numel - 4 if skip_tail else c.numel
    n = min(n, 4 * 512 * 256) if one_trip else n
    da = body(c.numel, canary, dt)
    da[:n] = store(dy * c.g, dt, trunc)[:n]
    prod = (dy * a).double()
    prod[n:] = 0.0
    part = torch.full((512,), canary, dtype=torch.float32)
    part[:c.blocks] = block_sums(prod, c.blocks).float()
    acc = np.float32(0.0)
    for v in part[:c.blocks].numpy():                              # column_sum_kernel adds the blocks; integers: any order is exact
        acc = np.float32(acc + v)
    return Case(da=da, dg=torch.tensor([acc], dtype=torch.float32), partials=part)


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_rescale_bias
# ------------------------------------------------------------------------------------------------------------------------------------
def rescale_case(dt, rows, c, ldx, ldy, bias, regime) -> Case:
    """y = (x - bias) r + bias, r = fl32(sig_a[0] sig_b[1]).  regime "exact": r = 1.5, integers; "real": candidates."""
    g = X.gen(_seed((rows, c, ldx, ldy), "rescale", int(bias), regime))
    s = sig(dt)
    sa, sb = (SIG_EXACT if regime == "exact" else SIG_REAL)
    sig_a, sig_b = torch.tensor(sa, dtype=torch.float32), torch.tensor(sb, dtype=torch.float32)
    r = t32(n32(sig_a[0:1]) * n32(sig_b[1:2]))
    if regime == "exact":
        x, bv = ints((rows, c), s, g), ints((c,), s, g)
        assert float(r) == 1.5 and float(sig_a[1] * sig_b[0]) != 1.5 and float(sig_a[0] * sig_b[0]) != 1.5
    else:
        x, bv = ints((rows, c), s, g) / 64.0, ints((c,), 4096, g) / 1024.0
    if not bias:
        bv = torch.zeros_like(bv)
    x_s = to_storage(x, dt)
    b32 = bv.float()
    assert torch.equal(b32.double(), bv)
    if regime == "exact":
        check = ("exact", put(0.0, dt, rows, ldy, c, want_exact((x - bv) * 1.5 + bv, dt)), keep_cols(rows, ldy, c))
    else:
        t = x_s.float() - b32
        assert torch.equal(t.double(), x - bv)                     # t = fl32(x - bias) happens to be exact for these operands
        sep, fus = separate32(t, r, b32.expand_as(t)), fused32(t, r.expand_as(t), b32.expand_as(t))
        check = ("candidates", put(0.0, dt, rows, ldy, c, store(sep, dt)), keep_cols(rows, ldy, c), put(0.0, dt, rows, ldy, c, store(fus, dt)))
    return Case(dtype=dt, rows=rows, c=c, ldx=ldx, ldy=ldy, x=pitched(x_s, ldx), bias=b32 if bias else None, sig_a=sig_a, sig_b=sig_b,
                scalar=rescale_scalar(c, ldx, ldy), what=("rescale_bias", NAME[dt], (rows, c, ldx, ldy), bias, regime), checks=dict(y=check))


def restate_rescale(c: Case, canary=CANARIES[0], trunc=False, slot="a0b1", skip_tail=False, pad=None, fused=False, as_bf16=False) -> Case:
    x = decode(c.x, as_bf16).view(c.rows, c.ldx)[:, :c.c]
    r = {"a0b1": c.sig_a[0:1] * c.sig_b[1:2], "a1b1": c.sig_a[1:2] * c.sig_b[1:2], "a0b0": c.sig_a[0:1] * c.sig_b[0:1]}[slot]
    b = c.bias if c.bias is not None else torch.zeros(c.c)
    t = x - b
    v = fused32(t, r.expand_as(t), b.expand_as(t)) if fused else separate32(t, r, b)
    y = store(v, c.dtype, trunc)
    if skip_tail:
        y[-1, c.c - (1 if c.scalar else 4):] = canary
    return Case(y=put(canary, c.dtype, c.rows, c.ldy, c.c, y, pad=pad))


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_permute_chw_hwc
# ------------------------------------------------------------------------------------------------------------------------------------
def permute_case(dt, b, c, hw, to_hwc) -> Case:
    g = X.gen(_seed((b, c, hw), "permute", to_hwc))
    src = random_bits(dt, b * c * hw, g, quiet_nans=False)
    bits = as_bits(src)
    want = bits.view(b, c, hw).transpose(1, 2) if to_hwc else bits.view(b, hw, c).transpose(1, 2)
    return Case(dtype=dt, b=b, c=c, hw=hw, to_hwc=to_hwc, src=src, what=("permute", NAME[dt], (b, c, hw), to_hwc),
                checks=dict(dst=("bits", from_bits(want.reshape(-1), dt), None)))


def restate_permute(c: Case, canary=CANARIES[0], swapped=False, one_trip=False) -> Case:
    """i enumerates the destination, as the kernel's loop does."""
    total = c.b * c.c * c.hw
    i = torch.arange(total)
    img, r = i // (c.c * c.hw), i % (c.c * c.hw)
    if bool(c.to_hwc) != swapped:
        s = img * c.c * c.hw + (r % c.c) * c.hw + r // c.c
    else:
        s = img * c.c * c.hw + (r % c.hw) * c.c + r // c.hw
    out = as_bits(c.src)[s]
    if one_trip:
        out[2048 * 256:] = as_bits(torch.tensor([canary], dtype=c.dtype))[0]
    return Case(dst=from_bits(out, c.dtype))


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_channel_sum
# ------------------------------------------------------------------------------------------------------------------------------------
def channel_block_rows(x, pixels, c, blocks, pix_par):
    owner = (torch.arange(pixels) // pix_par) % blocks             # pixel p = (block + k blocks) pix_par + lane
    return torch.zeros(blocks, c, dtype=torch.float64).index_add_(0, owner, x)


def channel_sum_case(dt, pixels, c, ld) -> Case:
    g = X.gen(_seed((pixels, c, ld), "channel_sum"))
    amax = min(sig(dt), (X.LIMIT - 1) // pixels)
    x = ints((pixels, c), amax, g)
    assert pixels * amax < X.LIMIT and float(x.abs().sum(0).max()) < X.LIMIT
    _, pix_par, blocks = channel_sum_plan(pixels, c)
    part = torch.zeros(512, c, dtype=torch.float32)
    part[:blocks] = channel_block_rows(x, pixels, c, blocks, pix_par).float()
    keep = (torch.arange(512) >= blocks).view(512, 1).expand(512, c).reshape(-1)
    out = x.sum(0)
    assert torch.equal(out.float().double(), out) and torch.equal(part.double().sum(0), out)
    return Case(dtype=dt, pixels=pixels, c=c, ld=ld, x=pitched(to_storage(x, dt), ld), blocks=blocks, pix_par=pix_par,
                what=("channel_sum", NAME[dt], (pixels, c, ld)), checks=dict(out=("exact", out.float(), None), partials=("exact", part.reshape(-1), keep)))


def restate_channel_sum(c: Case, canary=CANARIES[0], drop_block=None, one_round=False, skip_tail=False, sum_padding=False, as_bf16=False) -> Case:
    x = decode(c.x, as_bf16).view(c.pixels, c.ld)
    if sum_padding and c.ld > c.c:
        x = x.clone()
        x[:, c.c - 1] = x[:, c.c - 1] + x[:, c.c]                  # a lane that adds the first padding column: NaN
    x = x[:, :c.c].double()
    ch = c.c - (c.c % 4 or 4) if skip_tail else c.c
    ch = min(ch, 1024) if one_round else ch
    part = torch.full((512, c.c), canary, dtype=torch.float32)
    part[:c.blocks, :ch] = channel_block_rows(x, c.pixels, c.c, c.blocks, c.pix_par).float()[:, :ch]
    rows = [b for b in range(c.blocks) if b != drop_block]
    out = torch.full((c.c,), canary, dtype=torch.float32)
    out[:ch] = part[rows][:, :ch].double().sum(0).float()            # integers below 2^24: the float32 sums are these in any order
    return Case(out=out, partials=part.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_mask_concat, sp_mask_mul_2d
# ------------------------------------------------------------------------------------------------------------------------------------
def mask_concat_case(dt, pixels, c, cp, values) -> Case:
    g = X.gen(_seed((pixels, c, cp), "mask_concat", len(values)))
    feat = ints((pixels, c), sig(dt), g)
    feat[:, 0], feat[:, c - 1] = feat[:, 0].abs() + 1, -feat[:, c - 1].abs() - 1
    mask = P._pick(values, (pixels,), g)
    mask[0] = max(values)
    if pixels >= len(values):
        mask[:len(values)] = torch.tensor(values, dtype=torch.float64)
    ref = torch.zeros(pixels, cp, dtype=torch.float64)
    ref[:, :c], ref[:, c] = feat * mask.view(-1, 1), mask
    assert cp > c and cp % 4 == 0 and c % 4 == 0
    return Case(dtype=dt, pixels=pixels, c=c, cp=cp, feat=to_storage(feat, dt).reshape(-1), mask=mask.float(),
                what=("mask_concat", NAME[dt], (pixels, c, cp), values), checks=dict(out=("exact", want_exact(ref, dt).reshape(-1), None)))


def restate_mask_concat(c: Case, canary=CANARIES[0], trunc=False, mask_at=0, pad="zero", one_trip=False, as_bf16=False) -> Case:
    feat = decode(c.feat, as_bf16).view(c.pixels, c.c)
    out = torch.full((c.pixels, c.cp), canary if pad == "unwritten" else 0.0, dtype=c.dtype)
    out[:, :c.c] = store(feat * c.mask.view(-1, 1), c.dtype, trunc)
    if c.c + mask_at < c.cp:
        out[:, c.c + mask_at] = store(c.mask, c.dtype, trunc)
    if pad == "neighbour":
        out[:, c.c + 1:] = out[:, c.c:c.c + 1]
    out = out.reshape(-1)
    if one_trip:
        out[4 * 2048 * 256:] = canary
    return Case(out=out)


def mask_mul_case(dt, b, k, ldf, ldo, values=MASK_HALVES) -> Case:
    g = X.gen(_seed((b, k, ldf, ldo), "mask_mul"))
    feat = ints((b, k), sig(dt), g)
    mask = P._pick(values, (b, k), g)
    ref = torch.zeros(b, ldo, dtype=torch.float64)
    ref[:, :k] = feat * mask
    return Case(dtype=dt, b=b, k=k, ldf=ldf, ldo=ldo, feat=pitched(to_storage(feat, dt), ldf), mask=mask.float().reshape(-1),
                what=("mask_mul_2d", NAME[dt], (b, k, ldf, ldo)), checks=dict(out=("exact", want_exact(ref, dt).reshape(-1), None)))


def restate_mask_mul(c: Case, canary=CANARIES[0], trunc=False, pad="zero", as_bf16=False) -> Case:
    feat = decode(c.feat, as_bf16).view(c.b, c.ldf)[:, :c.k]
    mask = c.mask.view(c.b, c.k)
    out = torch.full((c.b, c.ldo), canary if pad == "unwritten" else 0.0, dtype=c.dtype)
    out[:, :c.k] = store(feat * mask, c.dtype, trunc)
    if pad == "neighbour":
        out[:, c.k:] = out[:, c.k - 1:c.k]
    return Case(out=out.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_ingest_image, sp_ingest_image_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
def ingest_source(vals, layout):
    """[n][c][h][w] values of the source type -> (flat buffer, offset, (sn, sc, sh, sw)); every element of the buffer outside the image is NaN."""
    n, c, h, w = vals.shape
    if layout == "nchw":
        return vals.reshape(-1).clone(), 0, (c * h * w, h * w, w, 1)
    if layout == "nhwc":
        return vals.permute(0, 2, 3, 1).reshape(-1).clone(), 0, (h * w * c, 1, w * c, c)
    assert layout == "crop"
    big = torch.full((n, c, h + 3, w + 5), NAN, dtype=vals.dtype)
    big[:, :, 1:1 + h, 2:2 + w] = vals
    sh, sc, sn = w + 5, (h + 3) * (w + 5), c * (h + 3) * (w + 5)
    assert sn != c * h * w and sc != h * w and sh != w                # none of the dense strides but the unit one
    return big.reshape(-1), 1 * sh + 2, (sn, sc, sh, 1)


def ingest_case(src_dt, dt, n, h, w, c, cp, layout, regime) -> Case:
    """dst[n][h][w][cp] = src scale[ch % 3] + shift[ch % 3], zero in [c, cp).  regime: "exact" | "vgg" (candidates) | "plain" (no scale3 /
    shift3: a copy with one rounding)."""
    g = X.gen(_seed((n, h, w, c, cp), "ingest", layout, regime, NAME[src_dt]))
    lim = min(sig(src_dt), sig(dt))
    v = ints((n, c, h, w), lim, g) / 128.0
    v_s = to_storage(v, src_dt)
    scale, shift = {"exact": (INGEST_SCALE, INGEST_SHIFT), "vgg": (VGG_SCALE, VGG_SHIFT), "plain": (None, None)}[regime]
    sc32 = torch.tensor(scale or (1.0, 1.0, 1.0), dtype=torch.float32)[:c].view(1, c, 1, 1)
    sf32 = torch.tensor(shift or (0.0, 0.0, 0.0), dtype=torch.float32)[:c].view(1, c, 1, 1)
    if regime == "exact":
        assert len(set(scale)) == 3 and len(set(shift)) == 3
    nhwc = lambda t: put(0.0, dt, n * h * w, cp, c, t.permute(0, 2, 3, 1).reshape(-1, c), pad=0.0)          # noqa: E731
    if regime == "vgg":
        sep = separate32(v_s.float(), sc32, sf32.expand_as(v))
        fus = fused32(v_s.float(), sc32.expand_as(v), sf32.expand_as(v))
        check = ("candidates", nhwc(store(sep, dt)), None, nhwc(store(fus, dt)))
    else:
        check = ("exact", nhwc(want_exact(v * sc32.double() + sf32.double(), dt)), None)
    buf, off, strides = ingest_source(v_s, layout)
    return Case(dtype=dt, src_dtype=src_dt, n=n, h=h, w=w, c=c, cp=cp, layout=layout, src=buf, off=off, strides=strides, scale=scale, shift=shift,
                what=("ingest", NAME[src_dt], NAME[dt], (n, h, w, c, cp), layout, regime), checks=dict(dst=check))


def restate_ingest(c: Case, canary=CANARIES[0], trunc=False, shift_channel=0, pad="zero", one_trip=False, fused=False, as_bf16=False) -> Case:
    n, h, w, ch, cp = c.n, c.h, c.w, c.c, c.cp
    sn, sc, sh, sw = c.strides
    idx = (c.off + torch.arange(n).view(n, 1, 1, 1) * sn + torch.arange(h).view(1, h, 1, 1) * sh + torch.arange(w).view(1, 1, w, 1) * sw
           + torch.arange(ch).view(1, 1, 1, ch) * sc)
    v = decode(c.src, as_bf16)[idx]                                # [n][h][w][c]
    scale = torch.tensor(c.scale or (1.0, 1.0, 1.0), dtype=torch.float32)[(torch.arange(ch) + shift_channel) % 3]
    shift = torch.tensor(c.shift or (0.0, 0.0, 0.0), dtype=torch.float32)[torch.arange(ch) % 3]
    val = fused32(v, scale.expand_as(v), shift.expand_as(v)) if fused else separate32(v, scale, shift)
    out = torch.full((n * h * w, cp), canary if pad == "unwritten" else 0.0, dtype=c.dtype)
    out[:, :ch] = store(val, c.dtype, trunc).reshape(-1, ch)
    if pad == "neighbour" and cp > ch:
        out[:, ch:] = out[:, ch - 1:ch]
    if one_trip:
        out[2048 * 256:] = canary
    return Case(dst=out.reshape(-1))


def ingest_bwd_case(dt, pixels, c, cp, vgg=True) -> Case:
    """dsrc[p][c] = RN_storage(fl32(dy[p][c] scale[c % 3])): reads pitch cp (NaN in the padding), writes pitch c."""
    g = X.gen(_seed((pixels, c, cp), "ingest_bwd", int(vgg)))
    dy = to_storage(ints((pixels, c), sig(dt), g) / 64.0, dt)
    scale = VGG_SCALE if vgg else None
    sc32 = torch.tensor(scale or (1.0, 1.0, 1.0), dtype=torch.float32)[:c]
    want = store(t32(n32(dy) * n32(sc32)), dt)
    return Case(dtype=dt, pixels=pixels, c=c, cp=cp, dy=pitched(dy, cp), scale=scale, what=("ingest_bwd", NAME[dt], (pixels, c, cp), vgg),
                checks=dict(dsrc=("exact", want.reshape(-1), None)))


def restate_ingest_bwd(c: Case, canary=CANARIES[0], trunc=False, shift_channel=0, pitch=None, one_trip=False, as_bf16=False, once=False) -> Case:
    """once (the planted defect, what v_fma_mixlo_f16 computes): the exact product rounded ONCE into storage, skipping fl32."""
    flat = decode(c.dy, as_bf16)
    ld = pitch or c.cp
    idx = (torch.arange(c.pixels).view(-1, 1) * ld + torch.arange(c.c)) % flat.numel()
    scale = torch.tensor(c.scale or (1.0, 1.0, 1.0), dtype=torch.float32)[(torch.arange(c.c) + shift_channel) % 3]
    out = store(flat[idx] * scale, c.dtype, trunc)
    if once:
        out = rn_direct(flat[idx].double() * scale.double(), c.dtype)
    if one_trip:
        out[2048 * 256:] = canary
    return Case(dsrc=out.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_avgpool3s1_fwd, sp_global_avgpool_f32 (csrc/inception.hip)
# ------------------------------------------------------------------------------------------------------------------------------------
def window_sums(x):
    """3 x 3 sums with zero padding of [n][h][w][c]."""
    n, h, w, c = x.shape
    p = torch.zeros(n, h + 2, w + 2, c, dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x
    s = torch.zeros_like(x)
    for dy in range(3):
        for dx in range(3):
            s = s + p[:, dy:dy + h, dx:dx + w]
    return s


def avg3_case(dt, n, h, w, c) -> Case:
    g = X.gen(_seed((n, h, w, c), "avg3"))
    x = ints((n, h, w, c), sig(dt), g)
    x[:, 0, 0] = (x[:, 0, 0] / 9).trunc() * 9                      # a corner window: with a 1 x 1 map the sum itself is a multiple of 9
    if h >= 3 and w >= 3:
        x[:, 1, 1] = x[:, 1, 1] - (window_sums(x)[:, 1, 1] % 9)    # an interior window whose sum is a multiple of 9
        x[:, 1, 1] = torch.where(x[:, 1, 1].abs() > sig(dt), x[:, 1, 1] + 9 * torch.sign(-x[:, 1, 1]), x[:, 1, 1])
    s = window_sums(x)
    assert float(9 * x.abs().max()) < X.LIMIT and bool((s % 9 == 0).any()) and bool(((s % 9 != 0).any()) or h * w == 1)
    want = store(t32(n32(s) / np.float32(9.0)), dt)                # restated: fl32(S / 9), the divisor always 9
    ref = rn_direct(s / 9.0, dt) if dt == F32 else None            # fp32 storage: the same value from float64, ONE rounding
    assert ref is None or torch.equal(ref, want)
    return Case(dtype=dt, shape=(n, h, w, c), x=to_storage(x, dt).reshape(-1), what=("avgpool3s1", NAME[dt], (n, h, w, c)),
                checks=dict(y=("exact", want.reshape(-1), None)))


def restate_avg3(c: Case, canary=CANARIES[0], trunc=False, count_valid=False, as_bf16=False) -> Case:
    n, h, w, ch = c.shape
    x = decode(c.x, as_bf16).view(n, h, w, ch)
    s = window_sums(x)
    div = window_sums(torch.ones(1, h, w, 1)) if count_valid else torch.full((1, 1, 1, 1), 9.0)
    return Case(y=store(s / div, c.dtype, trunc).reshape(-1))


def global_avg_case(dt, n, hw, c) -> Case:
    g = X.gen(_seed((n, hw, c), "global_avg"))
    amax = min(sig(dt), (X.LIMIT - 1) // hw)
    x = ints((n, hw, c), amax, g)
    s = x.sum(1)
    assert hw * amax < X.LIMIT and n * c > 256
    want = t32(n32(s) / np.float32(hw))
    assert torch.equal(want, rn_direct(s / float(hw), F32))
    return Case(dtype=dt, n=n, hw=hw, c=c, x=to_storage(x, dt).reshape(-1), what=("global_avgpool", NAME[dt], (n, hw, c)),
                checks=dict(y=("exact", want.reshape(-1), None)))


def restate_global_avg(c: Case, canary=CANARIES[0], reciprocal=False, as_bf16=False) -> Case:
    x = decode(c.x, as_bf16).view(c.n, c.hw, c.c)
    s = torch.zeros(c.n, c.c)
    for k in range(c.hw):
        s = s + x[:, k]
    y = s * float(np.float32(1.0) / np.float32(c.hw)) if reciprocal else s / float(c.hw)
    return Case(y=y.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_nans(g, w):
    both = g.isnan() & w.isnan()
    z = torch.zeros((), dtype=g.dtype)
    return torch.where(both, z, g), torch.where(both, z, w)


def compare(c: Case, got: Case, canary=CANARIES[0], parts=None) -> float:
    """Every entry of c.checks against got, over the whole buffer body: the elements of `keep` must hold the canary.
    ("exact", want, keep) torch.equal by value (a NaN only where want has one); ("bits", want, keep) the integer views are equal;
    ("candidates", want_a, keep, want_b) every element equals one of the two; ("tanh", ref, keep, lo, hi, e) lo <= got <= hi.
    Returns the worst ratio of error to bound of the fp32 tanh comparisons (0 where everything was exact)."""
    worst = 0.0
    for name, check in c.checks.items():
        if (parts is not None and name not in parts) or (parts is None and name not in got):
            continue
        kind, want, keep = check[0], check[1], check[2]
        g = got[name].detach().cpu().reshape(-1)
        tag = "%s %s" % (c.what, name)
        if kind == "tanh":
            ref, lo, hi, e = check[1], check[3], check[4], check[5]
            assert g.dtype == lo.dtype, (tag, g.dtype)
            inside = torch.minimum(torch.maximum(g.double(), lo.double()), hi.double())          # NaN stays NaN
            gg, ww = _same_nans(g.double(), torch.where(ref.isnan(), ref, torch.where(g.isnan(), lo.double(), inside)))
            assert_exact(gg, ww, tag)
            if g.dtype == F32:                                     # the same bound as |got - ref| <= e, which also yields the ratio
                fin = ref.isfinite()
                worst = max(worst, assert_within(g[fin], ref[fin], e[fin], tag))
            continue
        assert g.dtype == want.dtype and g.shape == want.shape, (tag, g.dtype, want.dtype, g.shape, want.shape)
        fill = torch.tensor(canary, dtype=want.dtype)
        if kind == "candidates":
            other = check[3]
            want = torch.where((g == other) & (g != want), other, want)
        if keep is not None:
            want = torch.where(keep, fill, want)
        if kind == "bits":
            assert_exact(as_bits(g), as_bits(want), tag)
        else:
            gg, ww = _same_nans(g, want)
            assert_exact(gg, ww, tag)
    return worst


def tanh_error_ulps(c: Case, got) -> float:
    """The worst |got - tanh| of an fp32 result in fp32 ulp of the reference."""
    ref = c.checks["y"][1]
    g = got.detach().cpu().double().reshape(-1)
    ok = ref.isfinite() & (ref != 0)
    return float(((g - ref).abs()[ok] / ulp32(ref)[ok]).max())


# ------------------------------------------------------------------------------------------------------------------------------------
# the case tables: what tests/test_gpu_eltwise_exact.py launches and tests/test_eltwise_harness.py checks on the CPU, one list
# ------------------------------------------------------------------------------------------------------------------------------------
def ingest_cp(c, dt):
    return (c + 3) // 4 * 4 if dt == F32 else (c + 7) // 8 * 8


def _ingest_table(dt):
    rows = []
    for src_dt, dst_dt in INGEST_PAIRS:
        if dst_dt != dt:
            continue
        for n, h, w in INGEST_SHAPES[:3]:
            for c in (1, 2, 3):
                for cp in (c, ingest_cp(c, dt)):
                    for layout in INGEST_LAYOUTS:
                        rows += [(src_dt, dt, n, h, w, c, cp, layout, "exact"), (src_dt, dt, n, h, w, c, cp, layout, "vgg")]
                    rows.append((src_dt, dt, n, h, w, c, cp, "nchw", "plain"))
        n, h, w = INGEST_SHAPES[3]
        rows += [(src_dt, dt, n, h, w, 3, ingest_cp(3, dt), "crop", "exact"), (src_dt, dt, n, h, w, 3, 3, "nhwc", "vgg")]
    return rows


def _ingest_bwd_table(dt):
    rows = []
    for n, h, w in INGEST_SHAPES:
        for c in ((1, 2, 3) if n * h * w < 1000 else (3,)):
            for cp in (c, ingest_cp(c, dt)):
                rows += [(dt, n * h * w, c, cp, True)] + ([(dt, n * h * w, c, cp, False)] if n * h * w < 1000 else [])
    return rows


FAMILIES = {
    "act_fwd": (act_fwd_case, lambda dt: [(dt, n, a) for n in ACT_SIZES for a in ACTS]),
    "act_special": (act_special_case, lambda dt: [(dt, a) for a in ACTS]),
    "act_bwd": (act_bwd_case, lambda dt: [(dt, p, c, cp, a) for p, c, cp in ACT_BWD_VEC + ACT_BWD_PAD for a in ACTS]),
    "scale_add": (scale_add_case, lambda dt: [(dt, n, g) for n in ACT_SIZES for g in ((-3.0, 0.3) if n == TWO_TRIPS else SCALE_G + SCALE_G_GENERAL)]),
    "scale_add_bwd": (scale_add_bwd_case, lambda dt: [(dt, n, g) for n in SCALE_BWD_SIZES for g in ((0.3,) if n > 2000 else (0.3, -3.0, 0.5))]),
    "rescale": (rescale_case, lambda dt: [(dt,) + s + (b, r) for s in RESCALE_VEC + RESCALE_SCALAR for b in (True, False) for r in ("exact", "real")]),
    "permute": (permute_case, lambda dt: [(dt,) + s + (d,) for s in PERMUTE for d in (1, 0)]),
    "channel_sum": (channel_sum_case, lambda dt: [(dt,) + s for s in CHANNEL_SUM]),
    "mask_concat": (mask_concat_case, lambda dt: [(dt,) + s + (m,) for s in mask_concat_shapes(dt) for m in MASKS]),
    "mask_mul": (mask_mul_case, lambda dt: [(dt,) + s + (m,) for s in MASK_MUL for m in MASKS]),
    "ingest": (ingest_case, _ingest_table),
    "ingest_bwd": (ingest_bwd_case, _ingest_bwd_table),
    "avg3": (avg3_case, lambda dt: [(dt,) + s for s in AVG3]),
    "global_avg": (global_avg_case, lambda dt: [(dt,) + s for s in GLOBAL_AVG]),
}
RESTATE = {"act_fwd": restate_act_fwd, "act_special": restate_act_fwd, "act_bwd": restate_act_bwd, "scale_add": restate_scale_add,
           "scale_add_bwd": restate_scale_add_bwd, "rescale": restate_rescale, "permute": restate_permute, "channel_sum": restate_channel_sum,
           "mask_concat": restate_mask_concat, "mask_mul": restate_mask_mul, "ingest": restate_ingest, "ingest_bwd": restate_ingest_bwd,
           "avg3": restate_avg3, "global_avg": restate_global_avg}


def table(family, dt):
    return FAMILIES[family][1](dt)


def build(family, args) -> Case:
    return FAMILIES[family][0](*args)


def case_id(args):
    return "-".join(NAME[a] if a in NAME else sid(a) if isinstance(a, tuple) else str(a) for a in args)


def candidate_kinds(c: Case):
    return [k for k, v in c.checks.items() if v[0] == "candidates"]
