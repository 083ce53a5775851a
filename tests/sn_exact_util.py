"""Operands, float64 references, CPU-checked conditions and the comparison for the tests of the spectral-norm kernels
(csrc/spectral_norm.hip): tests/test_gpu_sn_exact.py; the self-test of everything here: tests/test_sn_harness.py.  The state machine
of sp_loss_scale_update (csrc/optim.hip) is restated at the end for tests/test_gpu_optim_guard_exact.py.  Everything in this module
runs on the CPU.  A weight is W [rows][cols] float64, cols = cin x taps (OIHW flattened).

blocks    W = 2^b x a sum of 4^m rank-one sign blocks r_k c_k^T of 4^p rows x 4^q columns on disjoint, randomly permuted rows and
          columns, zero elsewhere; u = +-2^-m on one row of each block.  Then ||W^T u|| = 2^(b+q), v = +-2^-(m+q), W v = +-2^(b+q-m) on
          the 4^(m+p) block rows, ||W v|| = sigma = 2^(b+p+q), u' = +-2^-(m+p): every value is a power of two, every sum exact, so
          any correctly rounded sqrtf and divide returns them and the whole forward is held to torch.equal.  The backward takes
          integer dWsn in [-3, 3] and a power-of-two grad_scale: <dWsn, W> is an integer multiple of 2^b below 2^12 x 2^b and
          dWsn - coef u v^T needs at most 22 bits (checked per case), so fused multiply-add contraction cannot matter.
integer   W uniform integers in [-3, 3], u in [-2, 2]: every partial sum of W^T u stays below 2^24, so the slab partials at part_off
          equal the int64 result bit for bit (slab boundaries, the 4-column and scalar paths, the bisection).  v, s = W v, u', sigma
          are held per element against float64 under the bounds of forward_reference.
dense     W ~ N(0, 0.02^2), u and v of unit norm, against float64 under the same bounds with the terms exact sums make vanish kept.

The bounds (forward_reference; U = 2^-24, one correctly rounded fp32 operation; gamma_d = d U bounds a sum of products whose
summation tree has depth d - depths(): a thread's walk, then the wave / block tree; R for W^T u, C for a row, T for sum s^2):
    t = W^T u          |dt_c|   <= gamma_R sum_r |W_rc| |u_r|                     (0 where the sums are exact integers)
    inv = 1 / ||t||    relative e_inv = gamma_C / 2 + 2 U                         (sum of squares, one sqrt, one reciprocal)
    v = t inv          |dv_c|   <= |dt_c| / ||t|| + |v_c| (||dt|| / ||t|| + e_inv + U)
    s = (W t) inv      |ds_r|   <= (sum_c |W_rc| |dt_c| + gamma_C sum_c |W_rc| |t_c|) / ||t|| + |s_r| (||dt|| / ||t|| + e_inv + U)
    sigma = tot / sqrt(tot), tot = sum s^2:   |dsigma| <= ||ds|| + sigma (gamma_T / 2 + 3 U)
    u' = s / sqrt(tot)                        |du_r|   <= |ds_r| / sigma + |u'_r| (||ds|| / sigma + gamma_T / 2 + 3 U)
each times 1 + 2^-6 for the second-order terms (every relative perturbation is asserted below 2^-8, and at most four products of
two of them stand behind a bound).  1 / sigma is held to fl32(1 / sigma) of the kernel's own sigma bit for bit, and both packings to fl_storage(fl32(W x that 1 / sigma)) bit for bit, in
every regime: the layout checks do not depend on sigma's rounding.

The backward is referred to the snapshots (u, v, 1 / sigma) the forward under test left in its scratch, in float64:
    grad = (G - (<G, W> / sigma) u v^T) / sigma x grad_scale (+ accumulate_from)
    |dgrad| <= ((D U sum |G| |W| / sigma + 3 U |c|) |u_r v_c| + U (|G| + |c u_r v_c|)) / sigma x scale + 2 U |grad| (+ U |result|)
with c = <G, W> / sigma and D the depth of the summation behind <G, W> (a thread's walk, the block tree, the partials or the atomic
adds, dot_depth / dot_depth_single); D U sum |G| |W| vanishes where the products are exact integers below 2^24.
No element is excluded anywhere and no share of outliers is admitted."""
from collections import namedtuple

import numpy as np
import torch

import exact_util as X
from attention_exact_util import assert_within
from exact_util import assert_exact, pack_reference

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (F32, BF16, F16)
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
S2 = 1.0 + 2.0 ** -6
SLAB, SN_GRID, MAX_LAYERS, DOT_BLOCKS, TR_CI = 128, 1024, 256, 512, 256          # csrc/spectral_norm.hip
JUNK = 77.0                                                                     # what the cin_p padding of a dWsn slot holds


class Case(X.Case):
    """exact_util.Case whose attributes can be assigned as well."""
    __setattr__ = dict.__setitem__


Spec = namedtuple("Spec", "rows cin taps kind")                                 # kind: conv | linear | plain


def cols_of(s):
    return s.cin * s.taps


# ---- shapes (rows, cin, taps, kind): the smallest that reach each branch ----------------------------------------------------------
FEW_ROWS = Spec(3, 64, 1, "conv")            # fewer rows than the four waves of a wv unit; cout_p padding
RGB = Spec(64, 3, 9, "conv")                 # cols = 27: scalar paths, vrun < run, the backward's non-16-byte branch
TWO_SLABS = Spec(130, 8, 9, "conv")          # two slabs, the second with 2 rows; cout_p = 136
LINEAR = Spec(257, 264, 1, "linear")         # three slabs, two column blocks
CHUNKS = Spec(40, 520, 9, "conv")            # three 256-channel chunks in the batched backward, the last with 8 channels
TAPS4 = Spec(16, 16, 4, "conv")              # the generic-taps staging loop, the transposing backward with taps neither 1 nor 9
BIG = Spec(768, 768, 1, "conv")              # rows x cols > 512 x 1024: SN_DOT_BLOCKS caps the backward grid
PLAIN = Spec(10, 36, 1, "plain")
PLAIN_RAGGED = Spec(37, 100, 1, "plain")     # 3700 elements: the last 1024-element chunk is ragged
MANY = Spec(20, 1028, 1, "linear")           # x 256: 1280 wtu and 1280 wv units, both above SN_GRID
RAGGED = [FEW_ROWS, RGB, TWO_SLABS, LINEAR, CHUNKS, TAPS4, PLAIN, PLAIN_RAGGED]
CAPPED = [BIG, TAPS4]                        # nb < gridDim.x for the small layer


def pad_to(c, m):
    return (c + m - 1) // m * m


def layout(specs, dt, dgrad=True, groups=None) -> Case:
    """Offsets, padding and alignment as ops.SpectralNormBank._build gives them (forward table, backward table, flat gradients)."""
    e = 4 if dt == F32 else 8
    esz = 4 if dt == F32 else 2
    ents, so, po, pb, wo, uo, vo = [], 0, 0, 0, 0, 0, 0
    max_rows = max_cols = max_pack = 1
    for s in specs:
        rows, cols = s.rows, cols_of(s)
        if s.kind == "conv":
            cin_p, cout_p = pad_to(s.cin, e), pad_to(rows, e)
        elif s.kind == "linear":
            cin_p, cout_p = pad_to(s.cin, 8), pad_to(rows, 8)
        else:
            cin_p, cout_p = s.cin, rows
        ent = Case(spec=s, rows=rows, cols=cols, cin=s.cin, taps=s.taps, cin_p=cin_p, cout_p=cout_p, kind=int(s.kind == "plain"))
        ent.update(w_off=wo, u_off=uo, v_off=vo)
        wo, uo, vo = wo + pad_to(rows * cols, 4), uo + pad_to(rows, 4), vo + pad_to(cols, 4)
        ent.scratch_off = so
        so += pad_to(cols + 2 * rows + 4, 4)
        ent.part_off = so
        ent.slabs = (rows + SLAB - 1) // SLAB
        so += pad_to(ent.slabs * cols, 4)
        ent.fwd_bytes = rows * cols * 4 if ent.kind else rows * s.taps * cin_p * esz
        ent.fwd_off = po
        po += pad_to(ent.fwd_bytes, 256)
        ent.dgrad_off, ent.dgrad_bytes = -1, 0
        if dgrad and not ent.kind:
            ent.dgrad_off, ent.dgrad_bytes = po, s.cin * s.taps * cout_p * esz
            po += pad_to(ent.dgrad_bytes, 256)
        tiles = 0 if ent.kind else ((cin_p + 31) // 32) * ((cout_p + 31) // 32)
        max_rows, max_cols = max(max_rows, rows), max(max_cols, cols)
        max_pack = max(max_pack, ent.fwd_bytes // (4 if ent.kind else esz), ent.dgrad_bytes // esz, tiles * 1024)
        ent.pack_block0 = pb
        ent.pack_width = (rows * cols + 1023) // 1024 if ent.kind else tiles
        pb += ent.pack_width
        ents.append(ent)
    ao, max_elems = 0, 1
    for ent in ents:
        ent.n_dw = ent.rows * ent.cols if ent.kind else ent.rows * ent.taps * ent.cin_p
        ent.dw_off, ent.dot_off, ent.db_off = ao, ao + ent.n_dw, ao + ent.n_dw + 1
        ao = pad_to(ent.db_off + ent.rows, 4)
        max_elems = max(max_elems, ent.rows * ent.cols)
    fo = 0
    groups = groups or [(0, len(ents))]
    for lo, hi in groups:
        for ent in ents[lo:hi]:
            ent.grad_off = fo
            fo += pad_to(ent.rows * ent.cols, 4)
        for ent in ents[lo:hi]:
            ent.bias_off = fo
            fo += pad_to(ent.rows, 4)
    return Case(entries=ents, dtype=dt, esz=esz, scratch_floats=so, pack_bytes=po, pack_blocks=pb, max_rows=max_rows, max_cols=max_cols,
                max_pack=max_pack, w_floats=wo, u_floats=uo, v_floats=vo, arena_floats=ao, flat_floats=fo, max_elems=max_elems, groups=groups)


def scratch_owned(lay, power_iter=True) -> torch.Tensor:
    """Mask over the scratch floats of what one sp_sn_forward call writes: [v | s | u | sigma, 1 / sigma] of every layer and, with a
    power iteration, the slab partials.  scal[2], scal[3], the padding and everything else stay as they were."""
    own = torch.zeros(lay.scratch_floats, dtype=torch.bool)
    for e in lay.entries:
        own[e.scratch_off:e.scratch_off + e.cols + 2 * e.rows + 2] = True
        if power_iter:
            own[e.part_off:e.part_off + e.slabs * e.cols] = True
    return own


def unpacked_blocks(lay, skip):
    """pack_block0 per layer and the flat grid of a forward that packs every layer but those in `skip` (ops._unpacked_table)."""
    b0, blocks = [], 0
    for i, e in enumerate(lay.entries):
        b0.append(blocks)
        if i not in skip:
            blocks += e.pack_width
    return b0, blocks


def f32_exact(t):
    return torch.equal(t.float().double(), t)


def held(t, dt):
    return torch.equal(t.to(dt).double(), t)


def integral(t):
    return torch.equal(t, t.round())


# ------------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------------
def block_params(rows, cols):
    """(m, p, q): 4^m blocks of 4^p rows x 4^q columns; p = 1 where the rows allow it (the new u then differs from the old one)."""
    for p in (1, 0):
        for m in (2, 1, 0):
            if 4 ** (m + p) <= rows and 4 ** m <= cols:
                q = max(k for k in (0, 1, 2) if 4 ** (m + k) <= cols)
                return m, p, q
    raise AssertionError((rows, cols))


def _pick(n, k, g, ends):
    """k distinct indices of range(n) in random order; ends: the first is 0 and the last is n - 1 (both sides of every boundary)."""
    if not ends or k < 2:
        return torch.randperm(n, generator=g)[:k]
    mid = torch.randperm(n - 2, generator=g)[:k - 2] + 1
    return torch.cat((torch.tensor([0]), mid, torch.tensor([n - 1])))


def blocks_layer(spec, idx, g) -> Case:
    rows, cols = spec.rows, cols_of(spec)
    m, p, q = block_params(rows, cols)
    b = idx % 3 - 1
    if b + p + q == 0:
        b = 1
    nb, br, bc = 4 ** m, 4 ** p, 4 ** q
    # the first row of a block carries u: block 0 starts at row 0 and the last block at the last row, so u reaches two slabs
    rsel = _pick(rows, nb * br, g, rows > SLAB and nb > 1).view(nb, br).clone()
    rsel[-1] = rsel[-1].flip(0)
    csel = _pick(cols, nb * bc, g, cols > 256).view(nb, bc)
    W = torch.zeros(rows, cols, dtype=torch.float64)
    u0 = torch.zeros(rows, dtype=torch.float64)
    sign = lambda *n: torch.randint(0, 2, n, generator=g).double() * 2 - 1                                       # noqa: E731
    for k in range(nb):
        W[rsel[k].view(-1, 1), csel[k].view(1, -1)] = 2.0 ** b * sign(br).view(-1, 1) * sign(bc).view(1, -1)
        u0[rsel[k, 0]] = float(sign(1)) * 2.0 ** -m
    v0 = X.integers((cols,), 5, g) + 0.5                       # never read by a power iteration: must be overwritten
    return Case(regime="blocks", spec=spec, W=W, u0=u0, v0=v0, m=m, p=p, q=q, b=b, urows=rsel[:, 0], bcols=csel)


def integer_layer(spec, idx, g) -> Case:
    rows, cols = spec.rows, cols_of(spec)
    W, u0, v0 = X.integers((rows, cols), 3, g), X.integers((rows,), 2, g), X.integers((cols,), 2, g)
    if not bool(u0.any()):
        u0[0] = 1.0
    return Case(regime="integer", spec=spec, W=W, u0=u0, v0=v0)


def dense_layer(spec, idx, g) -> Case:
    rows, cols = spec.rows, cols_of(spec)
    W = (0.02 * torch.randn(rows, cols, generator=g, dtype=torch.float64)).float().double()
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, generator=g, dtype=torch.float64), dim=0).float().double()      # noqa: E731
    return Case(regime="dense", spec=spec, W=W, u0=unit(rows), v0=unit(cols))


def depths(rows, cols):
    """Depths of the summation trees, products included: W^T u (a slab's rows in turn, at most 128, then the slabs in order), a row's
    dot with t and the sum of t^2 (64 lanes stride the columns, then six wave steps), sum s^2 (256 threads stride the rows, then the
    eight steps of the block tree)."""
    return min(rows, SLAB) + (rows + SLAB - 1) // SLAB + 1, -(-cols // 64) + 8, -(-rows // 256) + 9


def forward_reference(W, u0, v0, power_iter=True) -> Case:
    """float64 v, s, u', sigma and their bounds (module docstring); with exact integer sums the gamma terms vanish."""
    rows, cols = W.shape
    d_rows, d_cols, d_tot = depths(rows, cols)
    ints = integral(W) and integral(u0)
    if not power_iter:
        s = W @ v0
        sigma = s @ u0
        exact = integral(W) and integral(v0) and integral(u0) and float(W.abs() @ v0.abs() @ u0.abs()) < X.LIMIT
        ds = torch.zeros(rows, dtype=torch.float64) if exact else d_cols * U32 * (W.abs() @ v0.abs()) * SLACK
        dsig = 0.0 if exact else float(ds @ u0.abs() + d_tot * U32 * (s.abs() @ u0.abs())) * SLACK
        return Case(v=v0, s=s, u=u0, sigma=sigma, bv=torch.zeros(cols, dtype=torch.float64), bs=ds, bu=torch.zeros(rows, dtype=torch.float64),
                    bsigma=torch.tensor(dsig, dtype=torch.float64), exact=exact)
    A = W.abs().t() @ u0.abs()
    t = W.t() @ u0
    exact_t = ints and float(A.max()) < X.LIMIT
    dt_ = torch.zeros(cols, dtype=torch.float64) if exact_t else d_rows * U32 * A
    nt = float(t.norm())
    v = t / nt
    g_nn = 0.0 if exact_t and float((t * t).sum()) < X.LIMIT else d_cols * U32
    e_inv = g_nn / 2 + 2 * U32
    eps_t = float(dt_.norm()) / nt
    bv = dt_ / nt + v.abs() * (eps_t + e_inv + U32)
    wt = W.abs() @ t.abs()
    g_c = 0.0 if exact_t and float(wt.max()) < X.LIMIT else d_cols * U32
    s = W @ v
    ds = (W.abs() @ dt_ + g_c * wt) / nt + s.abs() * (eps_t + e_inv + U32)
    sigma = float(s.norm())
    g_tot = d_tot * U32
    bsigma = float(ds.norm()) + sigma * (g_tot / 2 + 3 * U32)
    u1 = s / sigma
    bu = ds / sigma + u1.abs() * (float(ds.norm()) / sigma + g_tot / 2 + 3 * U32)
    assert max(eps_t, e_inv, float(ds.norm()) / sigma, g_tot) < 2.0 ** -8, "a first-order bound needs small perturbations"
    return Case(v=v, s=s, u=u1, sigma=torch.tensor(sigma, dtype=torch.float64), bv=bv * S2, bs=ds * S2, bu=bu * S2,
                bsigma=torch.tensor(bsigma * S2, dtype=torch.float64), exact=False, exact_t=exact_t)


def slab_parts(W, u0):
    """[slabs][cols] float64: sum over the rows of each 128-row slab of W[r][c] u[r]."""
    rows = W.shape[0]
    return torch.stack([W[z:z + SLAB].t() @ u0[z:z + SLAB] for z in range(0, rows, SLAB)])


def finish_layer(L: Case, dt, power_iter=True) -> Case:
    """Adds the references, the CPU conditions and the checks (name -> ("exact", want) | ("within", ref, bound) | ("recip",) |
    ("same", name) | ("pack", which)) of one forward to a layer's operands."""
    W, u0, v0, spec = L.W, L.u0, L.v0, L.spec
    rows, cols = W.shape
    what = (L.regime, NAME[dt], tuple(spec), "eval" if not power_iter else "train")
    assert f32_exact(W) and f32_exact(u0) and f32_exact(v0), what
    r = forward_reference(W, u0, v0, power_iter)
    chk = {}
    if not power_iter:
        assert L.regime == "integer" and r.exact, what
        assert float(r.sigma) != 0.0 and float(r.sigma) != 1.0, (what, "sigma", float(r.sigma))
        chk.update(v=("exact", v0.float()), s=("exact", r.s.float()), usnap=("exact", u0.float()), sigma=("exact", r.sigma.float()),
                   u_out=("exact", u0.float()), v_out=("exact", v0.float()))
    else:
        parts = slab_parts(W, u0)
        if L.regime in ("blocks", "integer"):
            assert integral(W * 4) and float((W.abs().t() @ u0.abs()).max()) * 2 ** 8 < X.LIMIT and f32_exact(parts), (what, "partial sums reach 2^24")
            chk["parts"] = ("exact", parts.float())
        else:
            pb = torch.stack([W[z:z + SLAB].abs().t() @ u0[z:z + SLAB].abs() for z in range(0, rows, SLAB)]) * (min(rows, SLAB) + 1) * U32 * SLACK
            chk["parts"] = ("within", parts, pb)
        if L.regime == "blocks":
            m, p, q, b = L.m, L.p, L.q, L.b
            t = W.t() @ u0
            assert float(t.norm()) == 2.0 ** (b + q) and float(r.sigma) == 2.0 ** (b + p + q) != 1.0, (what, float(t.norm()), float(r.sigma))
            assert bool(((r.v.abs() == 2.0 ** -(m + q)) | (r.v == 0)).all()) and int((r.v != 0).sum()) == 4 ** (m + q), what
            assert bool(((r.u.abs() == 2.0 ** -(m + p)) | (r.u == 0)).all()) and int((r.u != 0).sum()) == 4 ** (m + p), what
            assert all(f32_exact(x) for x in (r.v, r.s, r.u)), what
            assert (p >= 1) == (not torch.equal(r.u, u0)), (what, "u' != u needs p >= 1")
            if rows > SLAB:
                assert int((parts.abs().sum(1) > 0).sum()) > 1, (what, "non-zero partials in one slab only")
            if cols > 256:
                nz = (W != 0).any(0)
                assert bool(nz[:256].any()) and bool(nz[256:].any()), (what, "blocks on one side of the 256-column boundary")
            for x in (W, W / r.sigma):
                assert held(x, dt), (what, "not representable in the storage type")
            chk.update(v=("exact", r.v.float()), s=("exact", r.s.float()), usnap=("exact", r.u.float()), sigma=("exact", r.sigma.float()))
        else:
            chk.update(v=("within", r.v, r.bv), s=("within", r.s, r.bs), usnap=("within", r.u, r.bu), sigma=("within", r.sigma, r.bsigma))
            if L.regime == "integer":
                assert r.exact_t, what
        chk.update(u_out=("same", "usnap"), v_out=("same", "v"))
    chk["inv_sigma"] = ("recip",)
    chk["fwd"] = ("pack", 0)
    if spec.kind != "plain":
        chk["dgrad"] = ("pack", 1)
    L.update(ref=r, checks=chk, what=what, dtype=dt, power_iter=power_iter)
    return L


def rows_fixed(spec):
    """Fewer than four rows: the blocks construction needs p = 0 and the iteration is a fixed point."""
    return spec.rows < 4


BUILDERS = {"blocks": blocks_layer, "integer": integer_layer, "dense": dense_layer}


def sn_case(regime, specs, dt, seed=0, power_iter=True, dgrad=True, groups=None) -> Case:
    """A table of layers in one regime: the layout, and per layer the operands, references, conditions and checks."""
    g = X.gen(1000 * seed + 17 * len(specs) + sum(s.rows + s.cin for s in specs[:8]) + {"blocks": 1, "integer": 2, "dense": 3}[regime])
    lay = layout(specs, dt, dgrad, groups)
    layers = []
    for i, s in enumerate(specs):
        L = finish_layer(BUILDERS[regime](s, i, g), dt, power_iter)
        L.ent = lay.entries[i]
        assert not power_iter or rows_fixed(s) or not torch.equal(L.ref.u.float(), L.u0.float()), (L.what, "u' == u")
        assert abs(float(L.ref.sigma) - 1) > 1e-3, (L.what, "sigma == 1")
        layers.append(L)
    return Case(regime=regime, dtype=dt, lay=lay, layers=layers, power_iter=power_iter, what=(regime, NAME[dt], len(specs)))


# ------------------------------------------------------------------------------------------------------------------------------------
# packings
# ------------------------------------------------------------------------------------------------------------------------------------
def packings(L: Case, inv_sigma, dt):
    """(forward, input-gradient) packing of fl32(W x inv_sigma) in the storage type; kind 1: the plain fp32 copy and None."""
    spec, e = L.spec, L.ent
    ws = (L.W.float() * inv_sigma.float().reshape(())).double()                # ONE fp32 product, then one rounding to storage
    if spec.kind == "plain":
        return ws.float(), None
    fwd, dg = pack_reference(ws.view(spec.rows, spec.cin, spec.taps, 1), e.cin_p, e.cout_p, dt)
    return fwd, (dg if e.dgrad_off >= 0 else None)


def pack_dw(L: Case, G):
    """dWsn [rows][cols] -> the fp32 forward packing [rows][taps][cin_p] with JUNK in the padding channels (kind 1: as it is)."""
    spec, e = L.spec, L.ent
    if spec.kind == "plain":
        return G.float().reshape(-1)
    out = torch.full((spec.rows, spec.taps, e.cin_p), JUNK, dtype=torch.float32)
    out[:, :, :spec.cin] = G.float().view(spec.rows, spec.cin, spec.taps).permute(0, 2, 1)
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------------
def dot_depth(rows, cols, cin, taps, plain, grid_x):
    """Depth of the fp32 summation behind <dWsn, W> in the batched kernels: a thread's walk, the block tree (8), the partials a
    thread adds (2), the second tree (8), the product (1)."""
    total = rows * cols
    nb = min(grid_x, (total + 1023) // 1024)
    if not plain and 1 < taps <= 9:
        chunks = (cin + TR_CI - 1) // TR_CI
        walk = -(-rows * chunks // nb) * -(-min(cin, TR_CI) * taps // 256)
    else:
        walk = -(-total // (nb * 256))
    return walk + 19


def dot_depth_single(rows, cols):
    """sp_sn_backward: a thread's walk, the block tree, one atomic add per block in any order, the product."""
    blocks = min(1024, (rows * cols + 1023) // 1024)
    return -(-rows * cols // (blocks * 256)) + 8 + blocks + 1


def grad_bias(L: Case, g, nonzero=True):
    G = X.integers(L.W.shape, 3, g) if L.regime != "dense" else torch.randn(L.W.shape, generator=g, dtype=torch.float64).float().double()
    db = X.integers((L.spec.rows,), 9, g)
    if not nonzero:
        G = torch.zeros_like(G)
    elif float((G * L.W).sum()) == 0.0:                        # <G, W> = 0 would take the correction term out of the case
        i = tuple((L.W != 0).nonzero()[0].tolist())
        G[i] = 3.0 if float(G[i]) != 3.0 else -3.0
    return G, db


def backward_checks(L: Case, snap: Case, G, depth, scale=1.0, prev=None, dot_given=None) -> dict:
    """grad [rows][cols] of one layer against float64 on the snapshots `snap` (usnap, v, inv_sigma: fp32 tensors the forward under
    test left behind): ("exact", want) in the blocks regime, ("within", ref, bound) elsewhere.  scale: fl32 grad_scale; prev: what
    accumulate_from holds; dot_given: dot_ready = 2 hands over <G, W / sigma> (fp32) instead of <G, W>."""
    W = L.W
    us, vs, isg = snap.usnap.double(), snap.v.double(), float(snap.inv_sigma.double())
    dot = float((G * W).sum())
    mag = float((G.abs() * W.abs()).sum())
    products_exact = integral(G) and integral(W * 4) and mag * 4 < X.LIMIT
    d_dot = 0.0 if products_exact else depth * U32 * mag * SLACK
    coef = dot * isg if dot_given is None else float(dot_given)
    d_coef = d_dot * isg if dot_given is None else 0.0
    uv = us.view(-1, 1) * vs.view(1, -1)
    corr = coef * uv
    inner = G - corr
    grad = inner * isg * scale
    out = grad if prev is None else prev + grad
    checks = {"dot": ("exact", torch.tensor(dot, dtype=torch.float32)) if products_exact else
              ("within", torch.tensor(dot, dtype=torch.float64), torch.tensor(d_dot, dtype=torch.float64))}
    if L.regime == "blocks":
        for x in (torch.tensor(coef, dtype=torch.float64), coef * us, corr, inner, inner * isg, grad, out):
            assert f32_exact(x), (L.what, "a backward intermediate leaves fp32")
        assert bool((corr != 0).any()), (L.what, "the correction term vanishes")
        checks["grad"] = ("exact", out.float())
        return checks
    e = ((d_coef + 3 * U32 * abs(coef)) * uv.abs() + U32 * (G.abs() + corr.abs())) * isg * abs(scale) + 2 * U32 * grad.abs()
    if prev is not None:
        e = e + U32 * (out.abs() + e)
    checks["grad"] = ("within", out, e * SLACK)
    return checks


def bias_want(db, scale=1.0, prev=None):
    """bias_grads: fl32(db x scale), added to what accumulate_from holds (one fp32 product, one fp32 addition)."""
    b = (db.float() * np.float32(scale))
    return b if prev is None else prev.float() + b


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32, with the defects the tests exist for
# ------------------------------------------------------------------------------------------------------------------------------------
def restate_forward(L: Case, dt, defects=()) -> Case:
    """sn_wtu / sn_tsum / sn_wv / sn_finalize / sn_pack in torch fp32.  defects: drop_first_slab, drop_last_row, skip_last_col,
    u_not_written, v_snap_before, sigma_no_div, taps_not_flipped, pad_not_zeroed, bisect_off_by_one."""
    W, u0, v0 = L.W.float(), L.u0.float(), L.v0.float()
    rows, cols = W.shape
    one = np.float32(1)
    if L.power_iter:
        Wp = W.clone()
        if "drop_last_row" in defects and rows % SLAB:
            Wp[-1] = 0
        if "skip_last_col" in defects and cols % 4:
            Wp[:, -1] = 0
        parts = torch.stack([(Wp[z:z + SLAB] * u0[z:z + SLAB].view(-1, 1)).sum(0) for z in range(0, rows, SLAB)])
        if "bisect_off_by_one" in defects:
            parts[0, :256] = float("nan")                     # the layer's first unit went to its neighbour: never written
        t = torch.zeros(cols)
        for z in range(parts.shape[0]):
            if not (z == 0 and "drop_first_slab" in defects):
                t = t + parts[z]
        inv = one / max(np.sqrt(np.float32((t * t).sum())), np.float32(1e-12))
        v = t * inv
        s = (W @ t) * inv
        tot = np.float32((s * s).sum())
        inv_norm = one / max(np.sqrt(tot), np.float32(1e-12))
        sigma = tot if "sigma_no_div" in defects else np.float32(tot * inv_norm)
        usnap = s * inv_norm
        out = Case(parts=parts, v=v0.clone() if "v_snap_before" in defects else v, s=s, usnap=usnap, v_out=v,
                   u_out=u0.clone() if "u_not_written" in defects else usnap)
    else:
        s = W @ v0
        sigma = np.float32((s * u0).sum())
        out = Case(v=v0.clone(), s=s, usnap=u0.clone(), u_out=u0.clone(), v_out=v0.clone())
    out.sigma = torch.tensor(sigma, dtype=torch.float32)
    out.inv_sigma = torch.tensor(one / np.float32(sigma), dtype=torch.float32)
    fwd, dg = packings(L, out.inv_sigma, dt)
    if L.spec.kind != "plain":
        if "pad_not_zeroed" in defects and L.ent.cin_p > L.spec.cin:
            fwd[0, 0, L.spec.cin] = 1.0
        if "taps_not_flipped" in defects and dg is not None and L.spec.taps > 1:
            dg = dg.flip(1)
    out.fwd, out.dgrad = fwd, dg
    return out


def restate_backward(L: Case, snap: Case, G, scale=1.0, prev=None, defects=()) -> Case:
    """sn_bwd_dot / sn_bwd_apply (batched) in torch fp32.  defects: coef_no_inv_sigma, drop_last_chunk, scale_ignored."""
    W, G32 = L.W.float(), G.float()
    if "drop_last_chunk" in defects and L.spec.cin > TR_CI:
        G32 = G32.clone().view(L.spec.rows, L.spec.cin, L.spec.taps)
        G32[:, (L.spec.cin - 1) // TR_CI * TR_CI:] = 0
        G32 = G32.view(W.shape)
    dot = np.float32((G32 * W).sum())
    isg = np.float32(snap.inv_sigma)
    coef = dot if "coef_no_inv_sigma" in defects else dot * isg
    gs = np.float32(1.0 if "scale_ignored" in defects else scale)
    grad = (G32 - (coef * snap.usnap.float()).view(-1, 1) * snap.v.float().view(1, -1)) * isg * gs
    return Case(dot=torch.tensor(dot, dtype=torch.float32), grad=grad if prev is None else prev.float() + grad)


# ------------------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def compare(L: Case, got: Case, parts=None, checks=None) -> float:
    """Every check of a layer (or `checks`) against got[name]; returns the worst error / bound of the bounded comparisons."""
    worst = 0.0
    for name, chk in (checks if checks is not None else L.checks).items():
        if parts is not None and name not in parts:
            continue
        tag = "%s %s" % (L.what, name)
        g = got[name]
        if chk[0] == "pack":
            want = packings(L, got.inv_sigma, L.dtype)[chk[1]]
            if want is None:
                assert g is None, tag
                continue
            assert_exact(g.reshape(want.shape), want, tag)
            continue
        g = g.detach().cpu()
        assert g.dtype == F32, (tag, g.dtype)
        if chk[0] == "exact":
            assert_exact(g.reshape(chk[1].shape), chk[1], tag)
        elif chk[0] == "same":
            assert_exact(g, got[chk[1]].detach().cpu().reshape(g.shape), tag + " against its snapshot")
        elif chk[0] == "recip":
            want = torch.tensor(np.float32(1) / np.float32(got.sigma), dtype=torch.float32)
            assert_exact(g.reshape(()), want, tag + " against fl32(1 / sigma)")
        else:
            worst = max(worst, assert_within(g.reshape(chk[1].shape), chk[1], chk[2], tag))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_loss_scale_update
# ------------------------------------------------------------------------------------------------------------------------------------
def loss_scale_step(st, growth, backoff, interval):
    """state = [scale, 1 / scale, clean steps, found, skipped steps] (fp32) after one sp_loss_scale_update."""
    f = np.float32
    scale, clean, skipped = f(st[0]), f(st[2]), f(st[4])
    if st[3] != 0:
        scale, clean, skipped = max(f(scale * f(backoff)), f(1)), f(0), f(skipped + 1)
    else:
        clean = f(clean + 1)
        if clean >= interval:
            scale, clean = min(f(scale * f(growth)), f(16777216)), f(0)
    return [float(scale), float(f(1) / scale), float(clean), 0.0, float(skipped)]
