"""ADA's color group as one 3 x 4 matrix per image (csrc/augment.hip: THE COLOR MATRIX), restated in torch for the
tests: the decode (ops.augment_cmat_table) next to ADA's five homogeneous matrices multiplied step by step, the forward and its backward
- as autograd and as the closed form - in float64 or fp32 for both families (plain: tab=None; geometric: an affine table), the rounding
bound of the fp32 expressions, and one augmented training step composed from the oracle's own functions.  Not a test module; nothing
here runs on a GPU.

THE ROUNDING BOUND (forward_bound / backward_bound).  augment_restated.py's three rules - err(p + q) <= err(p) + err(q) + U |p + q|,
err(p c) <= |c| err(p) + U |p c| (c exact), err(p / 3) <= err(p) / 3 + U |p / 3|, U = 2^-24, magnitudes from the float64 evaluation,
times 1 + 2^-10 for the second order - applied to what the kernels and the fp32 restatement evaluate.  The ctable is taken as GIVEN (the
tests read it back from the device), exact.

FORWARD.  e'_r = ((L_r0 e_0 + L_r1 e_1) + L_r2 e_2) + L_r3 on top of the incoming bound err(e) - augment_restated.forward_bound's color
bound where `color` is on, else 0 (e is then the stored source value): U per product and per sum, three products and three sums per
channel.  A fused multiply-add rounds once where the rules charge twice, so the kernel's contraction stays inside.  Plain family: the
result is moved, nothing more.  Geometric family: geom_restated.forward_bound's terms (ii) and (iii) - the coordinate error against the
slope of e' over the 4 x 4 neighbourhood (zero padded: an out-of-frame tap is 0, not the offset), and the bilinear form - with e' and
err(e') at the taps.

BACKWARD.  g1'_c = (L_0c g1_0 + L_1c g1_1) + L_2c g1_2 on top of err(g1): 0 in the plain family (g1 is a moved copy of dy), geom_restated's
gather bound in the geometric one.  U per product and per sum again.  Without `color` that is all.  With it the statistics launch takes
G = sum(g1') over OUTPUT pixels: k_r = (L_r0 + L_r1) + L_r2 (U per sum); per pixel (k0 dy_0 + k1 dy_1) + k2 dy_2 (|dy_r| err(k_r) + U per
product, U per sum); in the geometric family times W = (in-frame weights on y) (in-frame weights on x) with geom_restated's charge - the
weights' coordinate errors, U for each weight sum and 2 U for the two products - and THE REDUCTION by geom_restated's rule: a tree in
which every term passes through at most R = 32 additions, R U sum |terms| (the plain statistics kernel has the geometric one's shape:
at most 2048 / 256 = 8 sequential adds per thread, 6 shuffle levels, 3 adds over the waves, slices - 1 <= 1 in the apply launch; this
module's fp32 restatement is a pairwise tree of depth <= 14).  G is NOT exact here even in the plain family: the matrix is not dyadic.
Then augment_restated.py's backward chain with err(g1') and err(G) carried through the same rules, as geom_restated.py does.
S = sum(x) is taken as exact, as there: the bound tests use augment_restated.exact_operands on maps of at most 64 x 64."""
import math

import torch

import augment_restated as A
import geom_restated as G
from oracle import sempyr_oracle as O
from semantic_pyramid_for_image_generation_amd import ops

U = A.U
SECOND_ORDER = A.SECOND_ORDER
COLOR, TRANSLATION, CUTOUT = A.COLOR, A.TRANSLATION, A.CUTOUT
BRIGHTNESS, CONTRAST, LUMAFLIP, HUE, SATURATION = ops.CMAT_BRIGHTNESS, ops.CMAT_CONTRAST, ops.CMAT_LUMAFLIP, ops.CMAT_HUE, ops.CMAT_SATURATION
ALL = 31
REDUCTION_DEPTH = G.REDUCTION_DEPTH
LAST = 1.0 - 2.0 ** -24
NRM_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))          # 5.768...: the largest |nrm|, at a = 1 - 2^-24


# ---- the decode -------------------------------------------------------------------------------------------------------------------
def table(z, cmat, dtype=torch.float64):
    """The decode (ops.augment_cmat_table restates the kernel operation by operation): (n, 12) in `dtype`."""
    return ops.augment_cmat_table(z, cmat, dtype)


def table_of(L, t=(0.0, 0.0, 0.0), n=1):
    """A hand-written ctable: L three rows of three, t the three offsets (ANY 3 x 4 map, not only a decodable one), n equal rows, fp32."""
    row = []
    for r in range(3):
        row += [L[r][0], L[r][1], L[r][2], t[r]]
    return torch.tensor([row] * n, dtype=torch.float32)


def identity_table(n=1):
    return table_of(((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), n=n)


def parts(z, cmat):
    """(bb, c, s, theta, f) in float64 from z (n, 8) fp32: what the five words draw; the identity's value where a word is left out."""
    cmat = ops.augment_cmat(cmat)
    zz = z.detach().to(torch.float32).double()
    n = zz.shape[0]
    two_pi, pi = float(torch.tensor(2.0 * math.pi, dtype=torch.float32)), float(torch.tensor(math.pi, dtype=torch.float32))
    nrm = lambda a, b: torch.sqrt(-2.0 * torch.log(1.0 - zz[:, a])) * torch.cos(two_pi * zz[:, b])      # noqa: E731
    one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    bb = float(torch.tensor(0.2, dtype=torch.float32)) * nrm(0, 1) if cmat & BRIGHTNESS else zero
    c = torch.exp2(0.5 * nrm(2, 3)) if cmat & CONTRAST else one
    s = torch.exp2(nrm(4, 5)) if cmat & SATURATION else one
    theta = (2.0 * zz[:, 6] - 1.0) * pi if cmat & HUE else zero
    f = torch.where(zz[:, 7] < 0.5, -one, one) if cmat & LUMAFLIP else one
    return bb, c, s, theta, f


def step_by_step(z, cmat):
    """ADA's five homogeneous 4 x 4 matrices multiplied one by one in its order, each on the left (Karras et al. 2020, appendix B: color
    transformations), float64 -> (n, 12) rows in the ctable's layout.  v = (1, 1, 1, 0) / sqrt 3 is the luma axis."""
    bb, c, s, theta, f = parts(z, cmat)
    n = bb.shape[0]
    eye = torch.eye(4, dtype=torch.float64)
    v = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float64) / math.sqrt(3.0)
    vv = torch.outer(v, v)
    K = torch.zeros(4, 4, dtype=torch.float64)          # the cross-product matrix of the axis: K x = v x x
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    rows = []
    for i in range(n):
        C = eye.clone()
        T = eye.clone()
        T[:3, 3] = bb[i]
        C = T @ C                                                            # brightness: translate by (b, b, b)
        Sc = eye.clone()
        Sc[0, 0] = Sc[1, 1] = Sc[2, 2] = c[i]
        C = Sc @ C                                                           # contrast: scale about 0
        C = (eye - 2.0 * vv * (1.0 if f[i] < 0 else 0.0)) @ C                # luma flip: Householder reflection along the luma axis
        ct, st = math.cos(float(theta[i])), math.sin(float(theta[i]))
        R = eye.clone()
        R[:3, :3] = (ct * eye + st * K + (1.0 - ct) * vv)[:3, :3]
        C = R @ C                                                            # hue: Rodrigues' rotation about the luma axis
        Sat = eye.clone()
        Sat[:3, :3] = (vv + (eye - vv) * s[i])[:3, :3]
        C = Sat @ C                                                          # saturation: scale the chroma plane
        rows.append(C[:3, :].reshape(12))
    return torch.stack(rows)


def closed_form(bb, c, s, theta, f):
    """The collapsed product in float64 from the five parts themselves: Lm = c (f P + s cos(theta) Q + s sin(theta) K), t = c f bb, in
    the decode's order of operations -> (n, 12)."""
    p, cs_ = c * f, c * s
    beta, gamma = cs_ * torch.cos(theta), (cs_ * torch.sin(theta)) * (1.0 / math.sqrt(3.0))
    d = (p - beta) / 3.0
    di, lo, hi, t = beta + d, d - gamma, d + gamma, p * bb
    return torch.stack([di, lo, hi, t, hi, di, lo, t, lo, hi, di, t], dim=1)


def matrix(ct):
    """(Lm (n, 3, 3), t (n, 3)) of a ctable."""
    m = ct.view(-1, 3, 4)
    return m[:, :, :3], m[:, :, 3]


def z_for(bright=0.0, contrast=0.0, sat=0.0, hue=0.5, flip=False):
    """One row of z: bright / contrast / sat in {-1, 0, 1} choose nrm = -NRM_MAX, 0, +NRM_MAX (Box-Muller at a = 1 - 2^-24 with b = 1/2 or
    0, or a = 0); hue is z6 itself; flip chooses the side of 0.5."""
    pair = {-1: (LAST, 0.5), 0: (0.0, 0.0), 1: (LAST, 0.0)}
    return list(pair[bright]) + list(pair[contrast]) + list(pair[sat]) + [hue, 0.25 if flip else 0.75]


def end_rows():
    """Six rows of z at both ends of each range: every normal at +-NRM_MAX (brightness +-1.15, contrast 2^+-2.88, saturation 2^+-5.77),
    theta at -pi and just below +pi, z7 on either side of 0.5 (one row next to it); the identity; one row inside."""
    below_half = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    rows = [z_for(1, 1, 1, LAST, False), z_for(-1, -1, -1, 0.0, True), z_for(1, -1, 1, 0.0, True), z_for(0, 0, 0, 0.5, False),
            [0.3, 0.1, 0.6, 0.7, 0.2, 0.4, 0.8, 0.5], [0.9, 0.3, 0.1, 0.9, 0.5, 0.25, 0.25, below_half]]
    return torch.tensor(rows, dtype=torch.float32)


def exact_tables():
    """Hand-written ctables whose arithmetic is exact on multiples of 2^-8: the six channel permutations, diag(2, 0.5, -1) with offsets
    (0.25, -0.5, 1), and a full matrix of eighths with offsets."""
    import itertools
    tabs = []
    for perm in itertools.permutations(range(3)):
        tabs.append(table_of([[1.0 if perm[r] == c else 0.0 for c in range(3)] for r in range(3)]))
    tabs.append(table_of(((2.0, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, -1.0)), (0.25, -0.5, 1.0)))
    tabs.append(table_of(((0.125, -0.375, 0.625), (0.875, 0.25, -0.5), (-0.75, 1.0, 0.375)), (0.125, -0.25, 0.5)))
    return tabs


# ---- the map, forward and backward -------------------------------------------------------------------------------------------------
def _rows(ct, dtype, n):
    t = ct.to(dtype)
    return [[t[:, 4 * r + i].view(n, 1, 1) for i in range(4)] for r in range(3)]


def apply(e, ct, dtype):
    """e'_r = ((L_r0 e_0 + L_r1 e_1) + L_r2 e_2) + L_r3 on e (n, 3, h, w), each product and sum once in `dtype` (differentiable)."""
    n = e.shape[0]
    return torch.stack([((l[0] * e[:, 0] + l[1] * e[:, 1]) + l[2] * e[:, 2]) + l[3] for l in _rows(ct, dtype, n)], dim=1)


def apply_t(g, ct, dtype):
    """g'_c = (L_0c g_0 + L_1c g_1) + L_2c g_2: the transposed 3 x 3 matrix."""
    n = g.shape[0]
    l = _rows(ct, dtype, n)
    return torch.stack([(l[0][c] * g[:, 0] + l[1][c] * g[:, 1]) + l[2][c] * g[:, 2] for c in range(3)], dim=1)


def _pointwise(x, u, policy, dtype):
    """Section 11's color transform of the source, pointwise (identity without the color bit; nothing is moved)."""
    return A.forward(x, u, ops.augment_policy(policy) & COLOR, dtype)


def forward(x, u, ct, policy, tab=None, dtype=torch.float64):
    """T(x; u, ctable[, table]): the color stage e, the matrix as its last step, then the plain family's translation and cutout
    (tab None) or the geometric family's resampling through `tab` and the cutout window (differentiable)."""
    policy = ops.augment_policy(policy)
    n, c, h, w = x.shape
    assert c == 3 and tuple(ct.shape) == (n, 12)
    e = apply(_pointwise(x, u, policy, dtype), ct, dtype)
    if tab is None:
        return A._move(e, u, policy)
    assert tuple(tab.shape) == (n, 8)
    return torch.where(G.keep_mask(u, h, w, policy), G.resample(e, tab, dtype), torch.zeros((), dtype=dtype))


def _axis_weights(c, size, zero):
    c0 = torch.floor(c)
    f = c - c0
    return torch.where((c0 >= 0) & (c0 < size), 1 - f, zero) + torch.where((c0 + 1 >= 0) & (c0 + 1 < size), f, zero)


def sum_g1(dy, u, ct, policy, tab=None, dtype=torch.float64):
    """sum(g1') per image as the statistics kernels take it: over OUTPUT pixels that show something, (k0 dy_0 + k1 dy_1) + k2 dy_2 with
    k_r = (L_r0 + L_r1) + L_r2, in the geometric family times the in-frame tap weights; a pairwise tree."""
    policy = ops.augment_policy(policy)
    n, _, h, w = dy.shape
    zero = torch.zeros((), dtype=dtype)
    keep = A.keep_mask(u, h, w, policy) if tab is None else G.keep_mask(u, h, w, policy)
    d = torch.where(keep, dy.to(dtype), zero)
    k = [(l[0] + l[1]) + l[2] for l in _rows(ct, dtype, n)]
    terms = (k[0] * d[:, 0] + k[1] * d[:, 1]) + k[2] * d[:, 2]
    if tab is not None:
        y, x = G.coords(tab, h, w, dtype)
        terms = terms * (_axis_weights(y, h, zero) * _axis_weights(x, w, zero))
    return G._tree_sum(terms.reshape(n, h * w))


def backward(dy, u, ct, policy, tab=None, dtype=torch.float64):
    """The closed-form gradient of sum(T(x) * dy) with respect to x: the family's g1, the transposed matrix, section 11's color backward."""
    policy = ops.augment_policy(policy)
    n, _, h, w = dy.shape
    g1 = A._move(dy.to(dtype), u, policy, inverse=True) if tab is None else G.gather_g1(dy, u, tab, policy, dtype)
    g = apply_t(g1, ct, dtype)
    if policy & COLOR:
        _, s, k = (A._per_image(t, dtype, n) for t in ops.augment_decode(u, h, w, policy)[:3])
        gm = sum_g1(dy, u, ct, policy, tab, dtype).view(n, 1, 1, 1) / (3 * h * w)
        g2 = k * g + (1 - k) * gm
        g = s * g2 + (1 - s) * A._mean3(g2)
    return g


def backward_autograd(dy, u, ct, policy, tab=None, dtype=torch.float64):
    x = torch.zeros(dy.shape, dtype=dtype, requires_grad=True)
    (dx,) = torch.autograd.grad(forward(x, u, ct, policy, tab, dtype), x, dy.to(dtype))
    return dx


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def _map_bound(e, e_e, rows, transposed):
    """(values, first-order errors) of the 3 x 4 map (or of its transposed 3 x 3 part) on e with incoming error e_e: U per product and sum."""
    out, err = [], []
    for r in range(3):
        l = [rows[i][r] for i in range(3)] if transposed else rows[r][:3]
        p = [l[i] * e[:, i] for i in range(3)]
        e_p = [l[i].abs() * e_e[:, i] + U * p[i].abs() for i in range(3)]
        s01 = p[0] + p[1]
        e_s01 = e_p[0] + e_p[1] + U * s01.abs()
        s012 = s01 + p[2]
        e_s = e_s01 + e_p[2] + U * s012.abs()
        if not transposed:
            s012 = s012 + rows[r][3]
            e_s = e_s + U * s012.abs()
        out.append(s012)
        err.append(e_s)
    return torch.stack(out, dim=1), torch.stack(err, dim=1)


def _geom_forward_terms(e, e_e, u, tab, policy):
    """geom_restated.forward_bound's terms (ii) and (iii) for tap values e with incoming error e_e (that function computes both from x)."""
    n, _, h, w = e.shape
    f64 = torch.float64
    y, xx = G.coords(tab, h, w, f64)
    y0, x0 = torch.floor(y), torch.floor(xx)
    fy, fx = (y - y0).view(n, 1, h, w), (xx - x0).view(n, 1, h, w)
    d_y, d_x = (t.view(n, 1, h, w) for t in G._coord_err(tab, h, w))
    hi = torch.full((n, 3, h, w), -float("inf"), dtype=f64)
    lo = torch.full((n, 3, h, w), float("inf"), dtype=f64)
    for a in (-1, 0, 1, 2):
        for b in (-1, 0, 1, 2):
            t = G._tap(e, y0 + a, x0 + b)
            hi, lo = torch.maximum(hi, t), torch.minimum(lo, t)
    err = (hi - lo) * (d_y + d_x)
    rows = []
    for a, wy in ((0, 1 - fy), (1, fy)):
        prods = []
        for b, wx in ((0, 1 - fx), (1, fx)):
            t, e_t = G._tap(e, y0 + a, x0 + b), G._tap(e_e, y0 + a, x0 + b)
            p = wx * t
            prods.append((p, wx * e_t + U * wx * t.abs() + U * p.abs()))
        s = prods[0][0] + prods[1][0]
        e_s = prods[0][1] + prods[1][1] + U * s.abs()
        r = wy * s
        rows.append((r, wy * e_s + U * wy * s.abs() + U * r.abs()))
    out = rows[0][0] + rows[1][0]
    err = err + rows[0][1] + rows[1][1] + U * out.abs()
    return torch.where(G.keep_mask(u, h, w, policy), err * SECOND_ORDER, torch.zeros((), dtype=f64))


def forward_bound(x, u, ct, policy, tab=None):
    """Per output element: the most |fp32 evaluation - float64 evaluation| of forward() can be (module docstring)."""
    policy = ops.augment_policy(policy)
    n = x.shape[0]
    e = _pointwise(x, u, policy, torch.float64)
    e_e = A.forward_bound(x, u, policy & COLOR)
    e2, e_e2 = _map_bound(e, e_e, _rows(ct, torch.float64, n), False)
    if tab is None:
        return A._move(e_e2 * SECOND_ORDER, u, policy)
    return _geom_forward_terms(e2, e_e2, u, tab, policy)


def backward_bound(dy, u, ct, policy, tab=None):
    """Per input element: the most |fp32 evaluation - float64 evaluation| of backward() can be (module docstring)."""
    policy = ops.augment_policy(policy)
    n, _, h, w = dy.shape
    f64 = torch.float64
    zero = torch.zeros((), dtype=f64)
    rows = _rows(ct, f64, n)
    if tab is None:
        g1 = A._move(dy.double(), u, policy, inverse=True)
        e_g1 = torch.zeros_like(g1)
        keep = A.keep_mask(u, h, w, policy)
    else:
        g1 = G.gather_g1(dy, u, tab, policy, f64)
        e_g1 = G.backward_bound(dy, u, tab, policy & ~COLOR) / SECOND_ORDER          # the gather's own first-order bound
        keep = G.keep_mask(u, h, w, policy)
    g, e_g = _map_bound(g1, e_g1, rows, True)
    if not policy & COLOR:
        return e_g * SECOND_ORDER
    # G = sum(g1') as the statistics launch takes it
    d = torch.where(keep, dy.double(), zero)
    S, e_S, Sabs = 0.0, 0.0, 0.0
    for r in range(3):
        l = rows[r]
        k01 = l[0] + l[1]
        k = k01 + l[2]
        e_k = U * k01.abs() + U * k.abs()
        p = k * d[:, r]
        e_p = d[:, r].abs() * e_k + U * p.abs()
        S, e_S, Sabs = S + p, e_S + e_p + (U * (S + p).abs() if r else 0.0), Sabs + p.abs()
    if tab is None:
        terms, e_terms, mags = S, e_S, Sabs
    else:
        y, x = G.coords(tab, h, w, f64)
        d_y, d_x = G._coord_err(tab, h, w)
        wy, wx = _axis_weights(y, h, zero), _axis_weights(x, w, zero)
        e_wy = torch.where((y > -1 - d_y) & (y < h + d_y), d_y, zero)
        e_wx = torch.where((x > -1 - d_x) & (x < w + d_x), d_x, zero)
        terms, mags = S * wy * wx, Sabs * wy * wx
        e_terms = Sabs * (e_wy * wx + e_wx * wy + e_wy * e_wx) + e_S * wy * wx + 4 * U * mags
    Gs = terms.sum(dim=(1, 2)).view(n, 1, 1, 1)
    e_G = (e_terms.sum(dim=(1, 2)) + REDUCTION_DEPTH * U * mags.sum(dim=(1, 2))).view(n, 1, 1, 1)
    _, s, k = (A._per_image(t, f64, n) for t in ops.augment_decode(u, h, w, policy)[:3])
    gm = Gs / (3 * h * w)
    e_gm = e_G / (3 * h * w) + U * gm.abs()
    t1 = k * g
    e_t1 = k.abs() * e_g + U * t1.abs()
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


# ---- one training step ----------------------------------------------------------------------------------------------------------------
def train_step_cmat(G_, D, V, opt_g, opt_d, images_real, labels, masks, noise_d, noise_g, u, v, z, policy, geom, cmat, w_rec=0.1, w_div=0.1,
                    tables=None, ctables=None, p=None, skip_dead_d_wgrad=False):
    """geom_restated.train_step_geom with the color matrix: u (3, B, 8), v (3, B, 4) or None without geometric words, z (3, B, 8);
    tables (3, B, 8) and ctables (3, B, 12) if the caller has them (the device's own), else decoded here in fp32.  p: None, or the gate's
    probability - image n of transform i is transformed iff u[i, n, 7] < p and passes as it is otherwise.  fp32, as the oracle computes."""
    b, _, h, w = images_real.shape
    geom = ops.augment_geom(geom)
    if tables is None and geom:
        tables = torch.stack([G.table(u[i], v[i], h, w, policy, geom, torch.float32) for i in range(3)])
    if ctables is None:
        ctables = torch.stack([table(z[i], cmat, torch.float32) for i in range(3)])

    def T(x, i):
        t = forward(x, u[i], ctables[i], policy, tables[i] if geom else None, torch.float32)
        if p is None:
            return t
        live = (u[i][:, 7] < torch.tensor(p, dtype=torch.float32)).view(-1, 1, 1, 1)
        return torch.where(live, t, x)
    out = {}
    O.zero_grads(G_); O.zero_grads(D)
    with torch.no_grad():
        feats_real = O.vgg16_forward(V, images_real)
        fake = O.generator_forward(G_, noise_d, feats_real, masks, labels.float(), training=True)
    out["images_fake_d"] = fake
    pred_real = O.discriminator_forward(D, T(images_real, 0), labels, training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 1), labels, training=True)
    l_real, l_fake = O.lsgan_discriminator_loss(pred_real, pred_fake)
    (l_real + l_fake).backward()
    out["grads_d"] = [q.grad.detach().clone() for q in O.trainable(D)]
    opt_d.step()
    O.zero_grads(G_); O.zero_grads(D)
    if skip_dead_d_wgrad:
        d_params = O.trainable(D)
        for q in d_params:
            q.requires_grad_(False)
    fake = O.generator_forward(G_, noise_g, feats_real, masks, labels.float(), training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 2), labels, training=True)
    l_g = O.lsgan_generator_loss(pred_fake)
    l_div = w_div * O.diversity_loss(fake, noise_g)
    feats_fake = O.vgg16_forward(V, fake)
    l_rec = w_rec * O.semantic_reconstruction_loss(feats_real, feats_fake, masks)
    (l_g + l_rec + l_div).backward()
    if skip_dead_d_wgrad:
        for q in d_params:
            q.requires_grad_(True)
    out["grads_g"] = [q.grad.detach().clone() for q in O.trainable(G_)]
    opt_g.step()
    out.update(images_fake_g=fake.detach(), loss_d_real=l_real.detach(), loss_d_fake=l_fake.detach(), loss_g=l_g.detach(),
               loss_rec=l_rec.detach().reshape(()), loss_div=l_div.detach())
    return out
