"""The geometric augmentation of the discriminator's inputs (csrc/augment.hip: THE GEOMETRIC FAMILY), restated in
torch for the tests: the decode, the bilinear forward and its backward - as autograd and as the closed-form gather - in float64 or
fp32, the rounding bound of the fp32 expressions, and one augmented training step composed from the oracle's own functions.  Not a test
module; nothing here runs on a GPU.

THE ROUNDING BOUND (forward_bound / backward_bound).  augment_restated.py's three rules - err(p + q) <= err(p) + err(q) + U |p + q|,
err(p c) <= |c| err(p) + U |p c|, err(p / 3) <= err(p) / 3 + U |p / 3|, U = 2^-24, magnitudes from the float64 evaluation, times
1 + 2^-10 for the second order - applied to what the kernels and the fp32 restatement evaluate on top of the color transform:

    y = (m00 h + m01 w) + m02      two products and two sums, each rounded once (never fused).  Every one of the four results is at
                                   most mag = |m00 h| + |m01 w| + |m02| in magnitude, so |dy| <= 4 U mag =: d_y (2 U mag where the
                                   products are exact, as for every table without scale and rotate; the bound does not lean on that).
                                   x likewise, d_x.  The table is taken as GIVEN (the tests read it back from the device), exact.
    y0 = floorf(y), fy = y - y0    exact (y and y0 are multiples of ulp(y) and 0 <= y - y0 < 1)
    1 - fy                         one rounding, U

FORWARD.  out = (1 - fy) ((1 - fx) e00 + fx e01) + fy ((1 - fx) e10 + fx e11), e.. = the color transform at the tap or 0 outside the
frame.  (i) The taps carry the color transform's own bound (augment_restated.forward_bound with the color bit alone).  (ii) As a
function of the real coordinates out is the zero-padded bilinear interpolant: continuous across every cell edge, with
|d out / d y| <= max - min of the tap values that bracket (y, x).  A coordinate error moves the evaluation point by at most (d_y, d_x),
possibly across a cell edge (floorf flips), so the slope is taken as D = max - min of e over the 4 x 4 neighbourhood rows y0 - 1 ... y0 +
2, columns x0 - 1 ... x0 + 2 (zero padded) - the 3 x 3 cells around the tap cell - and the term is D (d_y + d_x).  (iii) The bilinear
form itself: U per weight 1 - f, U per product, U per sum, by the three rules.

BACKWARD.  g1[i, j] = sum over outputs of omega dy, omega = hat(y - i) hat(x - j), hat(t) = max(0, 1 - |t|) - the same weights, seen
from the source pixel.  hat is continuous with slope 1, so a coordinate error changes one factor by at most d_y (d_x), and only where
|y - i| < 1 + d_y: |d omega| <= d_y hat(x - j) + d_x hat(y - i) + d_y d_x over the 4 x 4 neighbourhood.  Each term adds 3 U omega |dy|
(1 - f, the product of the two weights, the product with dy); the sum of at most 25 candidates adds 24 U sum(omega |dy|) in any order.
sum(g1) is NOT exact here (the weights are not dyadic).  The kernel takes it over OUTPUT pixels as sum((dy_0 + dy_1 + dy_2) W),
W = (in-frame weights on y) (in-frame weights on x): 2 U for the channel sum, U for each weight sum, 2 U for the two products, the
weights' coordinate error d_y + d_x (each in-frame weight sum changes by at most its d), and THE REDUCTION: assumed to be a tree in which
every term passes through at most R = 32 additions, R U sum |terms|.  That shape covers the kernel on the tests' maps (per thread at
most 2048 / 256 = 8 sequential adds, 6 shuffle levels, 3 adds over the block's 4 waves, slices - 1 <= 1 adds in the apply launch: 18)
and this module's fp32 restatement (a pairwise tree over at most 2^14 terms: 14).  Then augment_restated.py's backward chain
(Gm = G / (3HW); g2 = k g1 + (1 - k) Gm; dx = s g2 + (1 - s) mean3(g2)) with err(g1) and err(G) carried through the same rules.
S = sum(x) is taken as exact, as in augment_restated.py: the bound tests use its exact_operands on maps of at most 64 x 64."""
import torch

import augment_restated as A
from oracle import sempyr_oracle as O
from semantic_pyramid_for_image_generation_amd import ops

U = A.U
SECOND_ORDER = A.SECOND_ORDER
COLOR, TRANSLATION, CUTOUT = A.COLOR, A.TRANSLATION, A.CUTOUT
XFLIP, ROT90, SCALE, ROTATE = ops.GEOM_XFLIP, ops.GEOM_ROT90, ops.GEOM_SCALE, ops.GEOM_ROTATE
REDUCTION_DEPTH = 32


def table(u, v, h, w, policy, geom, dtype=torch.float64):
    """The decode (ops.augment_geom_table restates the kernel operation by operation): (n, 8) in `dtype`."""
    return ops.augment_geom_table(u, v, h, w, policy, geom, dtype)


def table_of(L, offset=(0.0, 0.0), n=1):
    """A hand-written table: linear part L = ((m00, m01), (m10, m11)), offsets (m02, m12), n equal rows, fp32."""
    row = [L[0][0], L[0][1], offset[0], L[1][0], L[1][1], offset[1], 0.0, 0.0]
    return torch.tensor([row] * n, dtype=torch.float32)


def keep_mask(u, h, w, policy):
    """(n, 1, h, w) bool: True outside the cutout window (OUTPUT coordinates); the translation lives in the table."""
    return A.keep_mask(u, h, w, ops.augment_policy(policy) & CUTOUT)


def color(x, u, policy, dtype):
    """Section 11's color transform of the source, pointwise, in `dtype` (identity without the color bit)."""
    return A.forward(x, u, ops.augment_policy(policy) & COLOR, dtype)


def coords(tab, h, w, dtype):
    """(y, x), each (n, h, w): (m00 h + m01 w) + m02 with every product and sum rounded once in `dtype`."""
    t = tab.to(dtype)
    hh = torch.arange(h, dtype=dtype).view(1, h, 1)
    ww = torch.arange(w, dtype=dtype).view(1, 1, w)
    m = [t[:, i].view(-1, 1, 1) for i in range(6)]
    return (m[0] * hh + m[1] * ww) + m[2], (m[3] * hh + m[4] * ww) + m[5]


def _tap(e, yy, xx):
    """e[n, :, yy, xx] with zero padding: yy, xx (n, h, w) integer-valued tensors."""
    n, c, h, w = e.shape
    valid = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).to(torch.int64).view(n, 1, h * w).expand(n, c, h * w)
    val = torch.gather(e.reshape(n, c, h * w), 2, idx).view(n, c, h, w)
    return torch.where(valid.view(n, 1, h, w), val, torch.zeros((), dtype=e.dtype))


def resample(e, tab, dtype):
    """The bilinear form on e (n, 3, h, w), zero padding (differentiable)."""
    n, _, h, w = e.shape
    y, x = coords(tab, h, w, dtype)
    y0, x0 = torch.floor(y), torch.floor(x)
    fy, fx = (y - y0).view(n, 1, h, w), (x - x0).view(n, 1, h, w)
    t00, t01, t10, t11 = _tap(e, y0, x0), _tap(e, y0, x0 + 1), _tap(e, y0 + 1, x0), _tap(e, y0 + 1, x0 + 1)
    return (1 - fy) * ((1 - fx) * t00 + fx * t01) + fy * ((1 - fx) * t10 + fx * t11)


def forward(x, u, tab, policy, dtype=torch.float64):
    """T(x; u, table): color at each tap, bilinear resampling through the table, the cutout window on the output (differentiable)."""
    n, c, h, w = x.shape
    assert c == 3 and tuple(tab.shape) == (n, 8)
    out = resample(color(x, u, policy, dtype), tab, dtype)
    return torch.where(keep_mask(u, h, w, policy), out, torch.zeros((), dtype=dtype))


def _inverse(tab, dtype):
    t = tab.to(dtype)
    r = 1 / (t[:, 0] * t[:, 4] - t[:, 1] * t[:, 3])
    return t[:, 4] * r, -t[:, 1] * r, -t[:, 3] * r, t[:, 0] * r


def gather_g1(dy, u, tab, policy, dtype=torch.float64, box=2):
    """g1 by the kernel's GATHER: for source pixel (i, j) the outputs within `box` of round(L^-1 ((i, j) - (m02, m12))) on each axis,
    each one's (y, x) by the forward's expression, accumulated in row-major order."""
    n, _, h, w = dy.shape
    d = torch.where(keep_mask(u, h, w, policy), dy.to(dtype), torch.zeros((), dtype=dtype))
    t = tab.to(dtype)
    m = [t[:, i].view(-1, 1, 1) for i in range(6)]
    inv = [a.view(-1, 1, 1) for a in _inverse(tab, dtype)]
    fi = torch.arange(h, dtype=dtype).view(1, h, 1).expand(n, h, w)
    fj = torch.arange(w, dtype=dtype).view(1, 1, w).expand(n, h, w)
    di, dj = fi - m[2], fj - m[5]
    hc = torch.round(inv[0] * di + inv[1] * dj).clamp(-3, h + 2)
    wc = torch.round(inv[2] * di + inv[3] * dj).clamp(-3, w + 2)
    g1 = torch.zeros(n, 3, h, w, dtype=dtype)
    for a in range(-box, box + 1):
        for b in range(-box, box + 1):
            hh, ww = hc + a, wc + b
            ok = (hh >= 0) & (hh < h) & (ww >= 0) & (ww < w)
            y = (m[0] * hh + m[1] * ww) + m[2]
            x = (m[3] * hh + m[4] * ww) + m[5]
            y0, x0 = torch.floor(y), torch.floor(x)
            fy, fx = y - y0, x - x0
            zero = torch.zeros((), dtype=dtype)
            wy = torch.where(y0 == fi, 1 - fy, torch.where(y0 + 1 == fi, fy, zero))
            wx = torch.where(x0 == fj, 1 - fx, torch.where(x0 + 1 == fj, fx, zero))
            wgt = torch.where(ok, wy * wx, zero).view(n, 1, h, w)
            g1 = g1 + wgt * _tap(d, hh, ww)
    return g1


def _tree_sum(t):
    """Pairwise tree over the last dimension (a fixed shape: at most ceil(log2 N) additions per term)."""
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def sum_g1(dy, u, tab, policy, dtype=torch.float64):
    """sum(g1) per image as the kernel takes it: over OUTPUT pixels outside the window, (dy_0 + dy_1 + dy_2) x (in-frame tap weights)."""
    n, _, h, w = dy.shape
    d = torch.where(keep_mask(u, h, w, policy), dy.to(dtype), torch.zeros((), dtype=dtype))
    y, x = coords(tab, h, w, dtype)
    zero = torch.zeros((), dtype=dtype)

    def axis(c, size):
        c0 = torch.floor(c)
        f = c - c0
        return torch.where((c0 >= 0) & (c0 < size), 1 - f, zero) + torch.where((c0 + 1 >= 0) & (c0 + 1 < size), f, zero)
    terms = ((d[:, 0] + d[:, 1]) + d[:, 2]) * (axis(y, h) * axis(x, w))
    return _tree_sum(terms.reshape(n, h * w))


def backward(dy, u, tab, policy, dtype=torch.float64, box=2):
    """The closed-form gradient of sum(T(x) * dy) with respect to x: the gather, then section 11's color backward."""
    policy = ops.augment_policy(policy)
    n, _, h, w = dy.shape
    g = gather_g1(dy, u, tab, policy, dtype, box)
    if policy & COLOR:
        _, s, k = (A._per_image(t, dtype, n) for t in ops.augment_decode(u, h, w, policy)[:3])
        gm = sum_g1(dy, u, tab, policy, dtype).view(n, 1, 1, 1) / (3 * h * w)
        g2 = k * g + (1 - k) * gm
        g = s * g2 + (1 - s) * A._mean3(g2)
    return g


def backward_autograd(dy, u, tab, policy, dtype=torch.float64):
    x = torch.zeros(dy.shape, dtype=dtype, requires_grad=True)
    (dx,) = torch.autograd.grad(forward(x, u, tab, policy, dtype), x, dy.to(dtype))
    return dx


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def _coord_err(tab, h, w):
    """(d_y, d_x), each (n, h, w): 4 U (|m0 h| + |m1 w| + |m2|)."""
    t = tab.double().abs()
    hh = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    ww = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    m = [t[:, i].view(-1, 1, 1) for i in range(6)]
    return 4 * U * (m[0] * hh + m[1] * ww + m[2]), 4 * U * (m[3] * hh + m[4] * ww + m[5])


def forward_bound(x, u, tab, policy):
    """Per output element: the most |fp32 evaluation - float64 evaluation| of forward() can be (module docstring)."""
    n, _, h, w = x.shape
    f64 = torch.float64
    e = color(x, u, policy, f64)
    e_e = A.forward_bound(x, u, ops.augment_policy(policy) & COLOR)
    y, xx = coords(tab, h, w, f64)
    y0, x0 = torch.floor(y), torch.floor(xx)
    fy, fx = (y - y0).view(n, 1, h, w), (xx - x0).view(n, 1, h, w)
    d_y, d_x = (t.view(n, 1, h, w) for t in _coord_err(tab, h, w))
    # (ii) the slope: max - min of e over the 4 x 4 neighbourhood, zero padded
    hi = torch.full((n, 3, h, w), -float("inf"), dtype=f64)
    lo = torch.full((n, 3, h, w), float("inf"), dtype=f64)
    for a in (-1, 0, 1, 2):
        for b in (-1, 0, 1, 2):
            t = _tap(e, y0 + a, x0 + b)
            hi, lo = torch.maximum(hi, t), torch.minimum(lo, t)
    err = (hi - lo) * (d_y + d_x)
    # (i) + (iii) the bilinear form by the three rules
    rows = []
    for a, wy in ((0, 1 - fy), (1, fy)):
        prods = []
        for b, wx in ((0, 1 - fx), (1, fx)):
            t, e_t = _tap(e, y0 + a, x0 + b), _tap(e_e, y0 + a, x0 + b)
            p = wx * t
            prods.append((p, wx * e_t + U * wx * t.abs() + U * p.abs()))          # the weight's own U (1 - f; charged for f too)
        s = prods[0][0] + prods[1][0]
        e_s = prods[0][1] + prods[1][1] + U * s.abs()
        r = wy * s
        rows.append((r, wy * e_s + U * wy * s.abs() + U * r.abs()))
    out = rows[0][0] + rows[1][0]
    err = err + rows[0][1] + rows[1][1] + U * out.abs()
    return torch.where(keep_mask(u, h, w, policy), err * SECOND_ORDER, torch.zeros((), dtype=f64))


def _scatter(vals, yy, xx, h, w):
    """Adds vals (n, c, h, w), one per OUTPUT pixel, into source positions (yy, xx) (n, h, w); positions outside the frame drop."""
    n, c = vals.shape[:2]
    valid = ((yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)).view(n, 1, h * w)
    idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).to(torch.int64).view(n, 1, h * w).expand(n, c, h * w)
    src = torch.where(valid, vals.reshape(n, c, h * w), torch.zeros((), dtype=vals.dtype))
    return torch.zeros(n, c, h * w, dtype=vals.dtype).scatter_add_(2, idx, src).view(n, c, h, w)


def backward_bound(dy, u, tab, policy):
    """Per input element: the most |fp32 evaluation - float64 evaluation| of backward() can be (module docstring)."""
    policy = ops.augment_policy(policy)
    n, _, h, w = dy.shape
    f64 = torch.float64
    zero = torch.zeros((), dtype=f64)
    d = torch.where(keep_mask(u, h, w, policy), dy.double(), zero)
    y, x = coords(tab, h, w, f64)
    y0, x0 = torch.floor(y), torch.floor(x)
    d_y, d_x = _coord_err(tab, h, w)
    e_g1 = torch.zeros(n, 3, h, w, dtype=f64)
    for a in (-1, 0, 1, 2):
        i = y0 + a
        hat_y = (1 - (y - i).abs()).clamp(min=0)
        dh_y = torch.where((y - i).abs() < 1 + d_y, d_y, zero)
        for b in (-1, 0, 1, 2):
            j = x0 + b
            hat_x = (1 - (x - j).abs()).clamp(min=0)
            dh_x = torch.where((x - j).abs() < 1 + d_x, d_x, zero)
            w_err = dh_y * hat_x + dh_x * hat_y + dh_y * dh_x + (3 + 24) * U * hat_y * hat_x
            e_g1 = e_g1 + _scatter(w_err.view(n, 1, h, w) * d.abs(), i, j, h, w)
    if not policy & COLOR:
        return e_g1 * SECOND_ORDER
    g1 = gather_g1(dy, u, tab, policy, f64)
    _, s, k = (A._per_image(t, f64, n) for t in ops.augment_decode(u, h, w, policy)[:3])

    def axis(c, size, dc):          # the in-frame weight sum and what a coordinate error can change it by
        c0 = torch.floor(c)
        f = c - c0
        wsum = torch.where((c0 >= 0) & (c0 < size), 1 - f, zero) + torch.where((c0 + 1 >= 0) & (c0 + 1 < size), f, zero)
        return wsum, torch.where((c > -1 - dc) & (c < size + dc), dc, zero)
    wy, e_wy = axis(y, h, d_y)
    wx, e_wx = axis(x, w, d_x)
    dsum = ((d[:, 0] + d[:, 1]) + d[:, 2]).abs()
    dabs = d.abs().sum(dim=1)
    terms = dsum * wy * wx
    e_terms = dabs * (e_wy * wx + e_wx * wy + e_wy * e_wx) + (2 * dabs + 4 * dsum) * U * wy * wx
    G = (((d[:, 0] + d[:, 1]) + d[:, 2]) * wy * wx).sum(dim=(1, 2)).view(n, 1, 1, 1)
    e_G = (e_terms.sum(dim=(1, 2)) + REDUCTION_DEPTH * U * terms.sum(dim=(1, 2))).view(n, 1, 1, 1)
    gm = G / (3 * h * w)
    e_gm = e_G / (3 * h * w) + U * gm.abs()
    t1 = k * g1
    e_t1 = k.abs() * e_g1 + U * t1.abs()
    t2 = (1 - k) * gm
    e_t2 = (1 - k).abs() * e_gm + U * (1 - k).abs() * gm.abs() + U * t2.abs()
    g2 = t1 + t2
    e_g2 = e_t1 + e_t2 + U * g2.abs()
    s01 = g2[:, 0:1] + g2[:, 1:2]
    e_s01 = e_g2[:, 0:1] + e_g2[:, 1:2] + U * s01.abs()
    s012 = s01 + g2[:, 2:3]
    e_s012 = e_s01 + e_g2[:, 2:3] + U * s012.abs()
    mm = s012 / 3
    e_mm = e_s012 / 3 + U * mm.abs()
    t3 = s * g2
    e_t3 = s.abs() * e_g2 + U * t3.abs()
    t4 = (1 - s) * mm
    e_t4 = (1 - s).abs() * e_mm + U * (1 - s).abs() * mm.abs() + U * t4.abs()
    dx = t3 + t4
    return (e_t3 + e_t4 + U * dx.abs()) * SECOND_ORDER


# ---- cases ----------------------------------------------------------------------------------------------------------------------
LAST = 1.0 - 2.0 ** -24


def v_for(flip=False, k=0, e=0.0, theta=0.0):
    """One row of v that decodes to these values: e in [-0.4, 0.4), theta in radians in [-pi / 4, pi / 4) (clamped to the largest fp32
    below 1 at the upper ends)."""
    import math
    return [0.25 if flip else 0.75, (k + 0.5) / 4.0, min((e + 0.4) / 0.8, LAST), min(theta / (math.pi / 2) + 0.5, LAST)]


def end_rows():
    """v rows at both ends of each range: every flip x k at e = -0.4 and (just below) +0.4, theta = -45 and (just below) +45 degrees."""
    import math
    rows = []
    for i, (e, theta) in enumerate(((-0.4, -math.pi / 4), (0.4, math.pi / 4), (-0.4, math.pi / 4), (0.4, -math.pi / 4), (0.0, 0.0), (0.1, 0.3))):
        rows.append(v_for(flip=bool(i % 2), k=i % 4, e=e, theta=theta))
    return torch.tensor(rows, dtype=torch.float32)


def exact_tables(h, w):
    """Hand-written tables whose arithmetic is exact on multiples of 2^-8: every flip x k about the centre (square maps), half-pixel and
    whole-pixel shifts, L = 2 I and L = I / 2."""
    c = (h - 1) / 2.0
    tabs = []
    for f in (1.0, -1.0):
        for L in (((1.0, 0.0), (0.0, 1.0)), ((0.0, 1.0), (-1.0, 0.0)), ((-1.0, 0.0), (0.0, -1.0)), ((0.0, -1.0), (1.0, 0.0))):
            L = (L[0], (f * L[1][0], f * L[1][1]))
            tabs.append(table_of(L, (c - (L[0][0] + L[0][1]) * c, c - (L[1][0] + L[1][1]) * c)))
    tabs += [table_of(((1.0, 0.0), (0.0, 1.0)), off) for off in ((0.5, 0.0), (0.0, -0.5), (1.5, 2.5))]
    tabs += [table_of(((2.0, 0.0), (0.0, 2.0)), (-c, -c)), table_of(((0.5, 0.0), (0.0, 0.5)), (c / 2, c / 2))]
    return tabs


def train_step_geom(G, D, V, opt_g, opt_d, images_real, labels, masks, noise_d, noise_g, u, v, policy, geom, w_rec=0.1, w_div=0.1,
                    tables=None, p=None, skip_dead_d_wgrad=False):
    """augment_restated.train_step_augmented with the geometric family: u (3, B, 8), v (3, B, 4); tables (3, B, 8) if the caller has
    them (the device's own), else decoded here in fp32.  p: None, or the gate's probability - image n of transform i is transformed iff
    u[i, n, 7] < p and passes as it is otherwise.  fp32, as the oracle computes."""
    b, _, h, w = images_real.shape
    if tables is None:
        tables = torch.stack([table(u[i], v[i], h, w, policy, geom, torch.float32) for i in range(3)])

    def T(x, i):
        t = forward(x, u[i], tables[i], policy, torch.float32)
        if p is None:
            return t
        live = (u[i][:, 7] < torch.tensor(p, dtype=torch.float32)).view(-1, 1, 1, 1)
        return torch.where(live, t, x)
    out = {}
    O.zero_grads(G); O.zero_grads(D)
    with torch.no_grad():
        feats_real = O.vgg16_forward(V, images_real)
        fake = O.generator_forward(G, noise_d, feats_real, masks, labels.float(), training=True)
    out["images_fake_d"] = fake
    pred_real = O.discriminator_forward(D, T(images_real, 0), labels, training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 1), labels, training=True)
    l_real, l_fake = O.lsgan_discriminator_loss(pred_real, pred_fake)
    (l_real + l_fake).backward()
    out["grads_d"] = [p.grad.detach().clone() for p in O.trainable(D)]
    opt_d.step()
    O.zero_grads(G); O.zero_grads(D)
    if skip_dead_d_wgrad:
        d_params = O.trainable(D)
        for q in d_params:
            q.requires_grad_(False)
    fake = O.generator_forward(G, noise_g, feats_real, masks, labels.float(), training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 2), labels, training=True)
    l_g = O.lsgan_generator_loss(pred_fake)
    l_div = w_div * O.diversity_loss(fake, noise_g)
    feats_fake = O.vgg16_forward(V, fake)
    l_rec = w_rec * O.semantic_reconstruction_loss(feats_real, feats_fake, masks)
    (l_g + l_rec + l_div).backward()
    if skip_dead_d_wgrad:
        for q in d_params:
            q.requires_grad_(True)
    out["grads_g"] = [p.grad.detach().clone() for p in O.trainable(G)]
    opt_g.step()
    out.update(images_fake_g=fake.detach(), loss_d_real=l_real.detach(), loss_d_fake=l_fake.detach(), loss_g=l_g.detach(),
               loss_rec=l_rec.detach().reshape(()), loss_div=l_div.detach())
    return out
