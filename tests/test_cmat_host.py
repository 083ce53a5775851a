"""Host side of ADA's color group as one 3 x 4 matrix per image (csrc/augment.hip: THE COLOR MATRIX, DESIGN.md section 20;
tests/test_gpu_cmat.py and tests/test_gpu_cmat_step.py have the GPU side): the closed form against ADA's five matrices multiplied step by
step, the structure of the decoded rows, the distribution of the draws, the closed-form backward against autograd, the rounding bound
the GPU tests hold the kernels to, the parsing of the words, and the ABI's refusals.  No GPU."""
import ctypes
import math

import pytest
import torch

import augment_restated as A
import cmat_restated as C
import geom_restated as G
import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, ops

LAST = C.LAST
WORDS = "brightness,contrast,lumaflip,hue,saturation"
F64 = torch.float64


def _z(n, seed):
    return torch.rand(n, 8, generator=torch.Generator().manual_seed(seed))


# ---- the closed form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmat", range(1, 32))
def test_float64_closed_form_equals_adas_five_matrices_step_by_step(cmat):
    """Random rows and both ends of every range (nrm = +-5.77, theta = -pi and just below pi, z7 on either side of 0.5), every subset."""
    z = _z(256, cmat)
    z[:6] = C.end_rows()
    z[6:10, :6] = torch.tensor([[0.0] * 6, [LAST] * 6, [LAST, 0.5] * 3, [0.0, LAST] * 3])
    got, want = C.table(z, cmat), C.step_by_step(z, cmat)
    assert got.dtype == F64 and tuple(got.shape) == (256, 12)
    assert float((got - want).abs().max()) <= 1e-12          # absolute, at entries of up to c s = 400
    assert float((got - C.closed_form(*C.parts(z, cmat))).abs().max()) == 0.0          # ops' float64 decode IS the closed form
    assert bool((got[:, 3] == got[:, 7]).all()) and bool((got[:, 3] == got[:, 11]).all())      # one offset along the grey axis


def test_brightness_and_contrast_rows_are_exactly_diagonal_in_fp32():
    z = _z(512, 3)
    z[:6] = C.end_rows()
    for cmat in (C.BRIGHTNESS, C.CONTRAST, C.BRIGHTNESS | C.CONTRAST):
        tab = C.table(z, cmat, torch.float32)
        assert tab.dtype == torch.float32
        L, t = C.matrix(tab)
        c = L[:, 0, 0]
        assert torch.equal(L, torch.diag_embed(torch.stack([c, c, c], dim=1)))          # off-diagonal entries are 0, the diagonal is one c
        bb64, c64, _, _, _ = C.parts(z, cmat)
        assert float((c.double() - c64).abs().max() / c64.max()) < 1e-5
        if cmat & C.CONTRAST:
            assert float(c.min()) > 2.0 ** -2.9 and float(c.max()) < 2.0 ** 2.9 and float(c.max()) > 4.0
        else:
            assert bool((c == 1.0).all())
        # the offset is the fp32 product c * bb of the fp32 factors
        nrm = torch.sqrt(-2.0 * torch.log(1.0 - z[:, 0])) * torch.cos(torch.tensor(2.0 * math.pi, dtype=torch.float32) * z[:, 1])
        bb = torch.tensor(0.2, dtype=torch.float32) * nrm if cmat & C.BRIGHTNESS else torch.zeros(512)
        assert torch.equal(t[:, 0], c * bb) and torch.equal(t[:, 1], t[:, 0]) and torch.equal(t[:, 2], t[:, 0])
    assert bool((C.matrix(C.table(z, C.CONTRAST, torch.float32))[1] == 0).all())


def test_luma_flip_alone_is_the_householder_reflection_and_z7_is_compared_strictly():
    half = torch.tensor(0.5)
    z = torch.zeros(5, 8)
    z[:, 7] = torch.tensor([0.0, float(torch.nextafter(half, torch.tensor(0.0))), 0.5, float(torch.nextafter(half, torch.tensor(1.0))), LAST])
    want = torch.eye(3, dtype=F64) - 2.0 / 3.0
    for dtype, tol in ((F64, 1e-15), (torch.float32, 2.0 ** -24)):
        L, t = C.matrix(C.table(z, C.LUMAFLIP, dtype))
        assert bool((t == 0).all())
        for i in (0, 1):
            assert float((L[i].double() - want).abs().max()) <= tol
        for i in (2, 3, 4):
            assert torch.equal(L[i].double(), torch.eye(3, dtype=F64))
    # without the word z7 does nothing
    assert torch.equal(C.table(z, C.HUE, F64)[0], C.table(z, C.HUE, F64)[4])


def test_hue_alone_is_a_rotation_about_the_grey_axis():
    z = _z(128, 5)
    z[:2, 6] = torch.tensor([0.0, LAST])
    L, t = C.matrix(C.table(z, C.HUE))
    assert bool((t == 0).all())
    eye = torch.eye(3, dtype=F64).expand_as(L)
    assert float((L.transpose(1, 2) @ L - eye).abs().max()) <= 1e-12
    assert float((torch.linalg.det(L) - 1.0).abs().max()) <= 1e-12
    ones = torch.ones(128, 3, 1, dtype=F64)
    assert float((L @ ones - ones).abs().max()) <= 1e-12
    # theta = 2 pi / 3 maps the channels cyclically (the closed form from the angle itself: z6 = 5 / 6 is no fp32 number)
    one, zero = torch.ones(1, dtype=F64), torch.zeros(1, dtype=F64)
    L, _ = C.matrix(C.closed_form(zero, one, one, torch.tensor([2.0 * math.pi / 3.0], dtype=F64), one))
    cyc = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=F64)
    assert float((L[0] - cyc).abs().max()) <= 1e-12
    L, _ = C.matrix(C.closed_form(zero, one, one, torch.tensor([-2.0 * math.pi / 3.0], dtype=F64), one))
    assert float((L[0] - cyc.t()).abs().max()) <= 1e-12


@pytest.mark.parametrize("cmat", [31, 30, 14, 24, 6, 17])
def test_grey_axis_and_determinant(cmat):
    """Lm (1, 1, 1) = p (1, 1, 1) with p = c f, and det Lm = f c^3 s^2."""
    z = _z(256, 11 + cmat)
    z[:6] = C.end_rows()
    bb, c, s, theta, f = C.parts(z, cmat)
    L, t = C.matrix(C.table(z, cmat))
    p = (c * f).view(-1, 1, 1)
    ones = torch.ones(256, 3, 1, dtype=F64)
    scale = L.abs().amax(dim=(1, 2)).clamp(min=1.0).view(-1, 1, 1)
    assert float((L @ ones - p * ones).abs().max()) <= 1e-12
    det = f * c ** 3 * s ** 2
    assert float(((torch.linalg.det(L) - det).abs() / scale.view(-1) ** 3).max()) <= 1e-12
    assert float((t[:, 0] - c * f * bb).abs().max()) <= 1e-12
    if not cmat & C.LUMAFLIP:
        assert bool((f == 1).all())
    else:
        assert bool((f[z[:, 7] < 0.5] == -1).all()) and bool((f[z[:, 7] >= 0.5] == 1).all()) and {-1.0, 1.0} == set(f.tolist())


def test_the_ends_of_z0_give_finite_rows_and_the_ranges_are_what_the_header_says():
    z = torch.zeros(4, 8)
    z[:, 7] = 0.75
    z[0, 0:6] = 0.0
    z[1, 0:6] = torch.tensor([LAST, 0.0] * 3)
    z[2, 0:6] = torch.tensor([LAST, 0.5] * 3)
    z[3, 0:6] = LAST
    for dtype in (F64, torch.float32):
        tab = C.table(z, 31, dtype)
        assert bool(torch.isfinite(tab).all())
    bb, c, s, _, _ = C.parts(z, 31)
    assert bb[0] == 0 and c[0] == 1 and s[0] == 1                                           # z0 = 0: nrm = 0
    assert abs(C.NRM_MAX - 5.768) < 1e-3
    assert abs(float(bb[1]) - 0.2 * C.NRM_MAX) < 1e-6 and abs(float(bb[2]) + 0.2 * C.NRM_MAX) < 1e-6
    assert abs(math.log2(float(c[1])) - 0.5 * C.NRM_MAX) < 1e-6 and abs(math.log2(float(s[2])) + C.NRM_MAX) < 1e-5
    g = _z(4096, 9)
    bb, c, s, theta, _ = C.parts(g, 31)
    assert float(bb.abs().max()) <= 0.2 * C.NRM_MAX and float(theta.min()) >= -math.pi - 1e-6 and float(theta.max()) < math.pi


def test_a_word_left_out_is_the_identity_and_calls_no_libm_function(monkeypatch):
    """Each word left out leaves its factor at the constant; the fp32 restatement then never calls log / sqrt / cos / sin / exp2."""
    z = _z(64, 13)
    calls = []
    for name in ("log", "sqrt", "cos", "sin", "exp2"):
        real = getattr(torch, name)
        monkeypatch.setattr(torch, name, lambda *a, _n=name, _f=real, **k: (calls.append(_n), _f(*a, **k))[1])
    tab = C.table(z, C.LUMAFLIP, torch.float32)
    assert calls == []
    tab = C.table(z, C.HUE, torch.float32)
    assert sorted(set(calls)) == ["cos", "sin"]
    del calls[:]
    tab = C.table(z, C.BRIGHTNESS | C.LUMAFLIP, torch.float32)
    assert sorted(set(calls)) == ["cos", "log", "sqrt"]
    del calls[:]
    tab = C.table(z, C.CONTRAST | C.SATURATION, torch.float32)
    assert sorted(set(calls)) == ["cos", "exp2", "log", "sqrt"] and calls.count("exp2") == 2
    monkeypatch.undo()
    for cmat in range(1, 32):
        bb, c, s, theta, f = C.parts(z, cmat)
        for word, value, ident in ((C.BRIGHTNESS, bb, 0.0), (C.CONTRAST, c, 1.0), (C.SATURATION, s, 1.0), (C.HUE, theta, 0.0), (C.LUMAFLIP, f, 1.0)):
            if not cmat & word:
                assert bool((value == ident).all()), (cmat, word)
        # what the row looks like: no brightness -> no offset; no hue -> symmetric; no hue, saturation, lumaflip -> diagonal
        L, t = C.matrix(C.table(z, cmat, torch.float32))
        if not cmat & C.BRIGHTNESS:
            assert bool((t == 0).all())
        if not cmat & C.HUE:
            assert torch.equal(L, L.transpose(1, 2))
        if not cmat & (C.HUE | C.SATURATION | C.LUMAFLIP):
            assert bool((L[:, 0, 1:] == 0).all()) and bool((L[:, 1, 2] == 0).all())


def test_brightness_draws_are_normal_with_standard_deviation_0_2():
    """65 536 rows of a fixed seed: the mean within 5 standard errors (0.2 / 256) of 0, the standard deviation within 5 of its own
    (0.2 / sqrt(2 x 65 536)) of 0.2.  Seed 2020 gives a mean of -1.37e-04 (0.2 standard errors) and a deviation of 0.19952 (0.9 of its own)."""
    n = 65536
    z = _z(n, 2020)
    t = C.matrix(C.table(z, C.BRIGHTNESS, torch.float32))[1][:, 0].double()
    mean, std = float(t.mean()), float(t.std())
    print("brightness over %d rows: mean %.3e, std %.5f" % (n, mean, std))
    assert abs(mean) <= 5 * 0.2 / 256
    assert abs(std - 0.2) <= 5 * 0.2 / math.sqrt(2 * n)
    # the other two normals use the same Box-Muller: log2 of contrast has deviation 0.5, of saturation 1
    _, c, s, _, _ = C.parts(z, 31)
    assert abs(float(torch.log2(c).std()) - 0.5) <= 5 * 0.5 / math.sqrt(2 * n) and abs(float(torch.log2(s).std()) - 1.0) <= 5 / math.sqrt(2 * n)


# ---- backward and bound ----------------------------------------------------------------------------------------------------------------
def _case(h, w, geom):
    """u over its ranges with a window at an edge, v and z at the ends of theirs; the fp32 tables of both decodes."""
    v, z = G.end_rows(), C.end_rows()
    n = z.shape[0]
    osk = [(-0.5, 0.0, 0.5), (0.4375, 1.9375, 1.4375), (0.0, 1.0, 1.0), (-0.25, 0.5, 0.75), (0.125, 1.5, 1.25), (0.3125, 0.0625, 0.5625)]
    u = torch.tensor([A.u_for(o, s, k, ty, tx, None, None, h, w) for (o, s, k), (ty, tx) in
                      zip(osk, [(-1, 1), (1, 0), (0, 0), (0, -1), (1, 1), (-1, -1)])], dtype=torch.float32)
    u[0, 5:7] = torch.tensor([0.0, LAST])
    tab = G.table(u, v, h, w, "translation", geom, torch.float32) if geom else None
    return n, u, z, tab


@pytest.mark.parametrize("policy", ["", "color", "translation,cutout", "color,translation,cutout"])
@pytest.mark.parametrize("h,w,geom", [(12, 12, 0), (7, 11, 0), (12, 12, 15), (7, 11, 13)])
def test_closed_form_backward_equals_autograd(h, w, geom, policy):
    """With and without color, with and without a geometric table, with the cutout window; every word, rows at the ends of the ranges
    and hand-written full matrices.  1e-12 absolute, at gradients of up to several hundred (entries of Lm reach 400)."""
    n, u, z, tab = _case(h, w, geom)
    dy = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(7), dtype=F64)
    for ct in (C.table(z, 31, torch.float32), torch.cat(C.exact_tables()[-2:] * 3), C.table(z, C.HUE | C.BRIGHTNESS, torch.float32)):
        want = C.backward_autograd(dy, u, ct, policy, tab)
        got = C.backward(dy, u, ct, policy, tab)
        assert float(want.abs().max()) > 0.1
        assert float((got - want).abs().max()) <= 1e-12
    # the identity matrix gives the families as they are
    eye = C.identity_table(n)
    x = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(8), dtype=F64)
    if tab is None:
        assert torch.equal(C.forward(x, u, eye, policy), A.forward(x, u, policy))
        assert float((C.backward(dy, u, eye, policy) - A.backward(dy, u, policy)).abs().max()) <= 1e-12
    else:
        assert torch.equal(C.forward(x, u, eye, policy, tab), G.forward(x, u, tab, policy))
        assert float((C.backward(dy, u, eye, policy, tab) - G.backward(dy, u, tab, policy)).abs().max()) <= 1e-12


@pytest.mark.parametrize("policy", ["", "color", "translation,cutout", "color,translation,cutout"])
@pytest.mark.parametrize("h,w,geom", [(16, 16, 0), (64, 64, 0), (8, 24, 0), (16, 16, 15), (40, 40, 15), (8, 24, 13)])
def test_fp32_restatement_alone_stays_within_the_rounding_bound_of_float64(h, w, geom, policy):
    """On augment_restated.exact_operands the fp32 evaluation of the forward and of the closed-form backward stays within
    cmat_restated.forward_bound / backward_bound of the float64 one, with ONE fp32 ctable (and affine table) in both.  The bound is
    derived in that module's docstring from the roundings of the expressions; nothing in it comes from a kernel's output."""
    n, u, z, tab = _case(h, w, geom)
    x, dy = A.exact_operands((n, 3, h, w), 31), A.exact_operands((n, 3, h, w), 32)
    for cmat in (31, C.HUE | C.SATURATION, C.BRIGHTNESS | C.CONTRAST | C.LUMAFLIP):
        ct = C.table(z, cmat, torch.float32)
        for fn, bound_fn, arg in ((C.forward, C.forward_bound, x), (C.backward, C.backward_bound, dy)):
            want = fn(arg, u, ct, policy, tab, F64)
            got = fn(arg, u, ct, policy, tab, torch.float32)
            assert got.dtype == torch.float32
            bound = bound_fn(arg, u, ct, policy, tab)
            excess = (got.double() - want).abs() - bound
            assert float(excess.max()) <= 0.0, (fn.__name__, policy, cmat, float(excess.max()))
            # against the largest value the map can make of |e| <= 16 (section 16's figure for the color stage): some two dozen roundings in
            # the plain family, the coordinate term of the geometric one on top (section 16: up to 2^-9 of |e|)
            scale = 3.0 * float(ct.abs().max()) * 16.0
            assert 0.0 < float(bound.max()) <= (2.0 ** -9 if geom else 2.0 ** -19) * scale


def test_exact_ctables_make_the_fp32_restatement_exact():
    h = w = 16
    u = torch.tensor([A.u_for(ty=1, tx=-2, h=h, w=w)], dtype=torch.float32)
    x, dy = A.exact_operands((1, 3, h, w), 41), A.exact_operands((1, 3, h, w), 42)
    for ct in C.exact_tables():
        for tab in [None] + G.exact_tables(h, w):
            for fn, arg in ((C.forward, x), (C.backward, dy)):
                assert torch.equal(fn(arg, u, ct, "translation,cutout", tab, torch.float32).double(), fn(arg, u, ct, "translation,cutout", tab, F64))
    perm = C.forward(x, u, C.exact_tables()[3], "", None, F64)          # the permutation (1, 2, 0): out_r = x_perm[r]
    assert torch.equal(perm, x.double()[:, [1, 2, 0]])


# ---- words, wrapper, ABI ---------------------------------------------------------------------------------------------------------------
def test_the_words_parse_and_the_other_parsers_keep_refusing_them():
    assert (ops.CMAT_BRIGHTNESS, ops.CMAT_CONTRAST, ops.CMAT_LUMAFLIP, ops.CMAT_HUE, ops.CMAT_SATURATION) == (1, 2, 4, 8, 16)
    assert ops.augment_cmat(WORDS) == 31 and ops.augment_cmat("hue, brightness") == 9 and ops.augment_cmat(None) == 0 and ops.augment_cmat("") == 0
    assert ops.augment_cmat(31) == 31 and ops.augment_cmat(0) == 0
    for bad in ("color", "xflip", "luma", "hue,flip", 32, -1, True, 1.5):
        with pytest.raises(_lib.SempyrError):
            ops.augment_cmat(bad)
    for old in ("", None, "color", "cutout, color", "color,translation,cutout", 0, 5, 7, "color,xflip", "rotate, rot90 ,cutout"):
        assert ops.augment_split3(old) == ops.augment_split(old) + (0,)
    assert ops.augment_split3("hue") == (0, 0, 8)
    assert ops.augment_split3("color,brightness,xflip, saturation ,cutout") == (5, 1, 17)
    assert ops.augment_split3("color,translation,cutout,xflip,rot90,scale,rotate," + WORDS) == (7, 15, 31)
    for bad in ("flip", "color,flip,hue", "hue,rotation", "luma", 8, -1, 1.5, True):
        with pytest.raises(_lib.SempyrError):
            ops.augment_split3(bad)
    # augment_split still returns pairs and still refuses the new words; augment_policy and augment_geom too
    assert ops.augment_split("color,xflip") == (1, 1)
    for fn in (ops.augment_split, ops.augment_policy, ops.augment_geom):
        for word in WORDS.split(","):
            with pytest.raises(_lib.SempyrError):
                fn(word)
        with pytest.raises(_lib.SempyrError):
            fn("color,brightness" if fn is not ops.augment_geom else "xflip,brightness")
    with pytest.raises(_lib.SempyrError):
        ops.augment_cmat_table(torch.zeros(2, 7), 31)


def test_wrapper_construction_sets_the_three_masks_and_the_log_string():
    G_, D = torch.nn.Linear(2, 2), sp.Discriminator(channel_factor=16)
    G_.latent_dimensions = 2
    make = lambda aug, **kw: sp.ModelWrapper(G_, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment=aug, **kw)      # noqa: E731
    mw = make("saturation,rotate,cutout,hue,xflip,color,brightness")
    assert (mw._aug_policy, mw._aug_geom, mw._aug_cmat) == (5, 9, 25)
    assert mw.logger.hyperparameter["augment"] == "color,cutout,xflip,rotate,brightness,hue,saturation"
    only = make("lumaflip,contrast")
    assert (only._aug_policy, only._aug_geom, only._aug_cmat) == (0, 0, 6) and only.logger.hyperparameter["augment"] == "contrast,lumaflip"
    full = make("color,translation,cutout,xflip,rot90,scale,rotate," + WORDS)
    assert full.logger.hyperparameter["augment"] == "color,translation,cutout,xflip,rot90,scale,rotate," + WORDS
    with pytest.raises(_lib.SempyrError):
        make("color,luma")
    img = torch.zeros(2, 3, 4, 4)
    for old_words in ("color", "color,xflip"):
        old = make(old_words)
        assert old._aug_cmat == 0 and old._augment_cmat_rows(img, None) is None and old._aug_ctables is None
        with pytest.raises(_lib.SempyrError, match="augment_z"):          # z for a wrapper without the words
            old._augment_cmat_rows(img, torch.zeros(3, 2, 8))
    off = make("")
    assert "augment" not in off.logger.hyperparameter
    with pytest.raises(_lib.SempyrError, match="augment_z"):
        off._augment_cmat_rows(img, torch.zeros(3, 2, 8))
    with pytest.raises(_lib.SempyrError):          # a wrong shape
        mw._augment_cmat_rows(img, torch.zeros(3, 2, 4))
    assert mw._augment_cmat_rows(img, torch.zeros(3, 2, 8)).shape == (3, 2, 8)
    assert only._augment_rows(img, None).shape == (3, 2, 8)          # the gate's draw u7 exists with the new words alone
    # the gate may ride on the new words alone - but its state lives on a GPU, so here only the refusal without any word
    with pytest.raises(_lib.SempyrError, match="nothing to gate"):
        make("", augment_p=0.5)
    # Discriminator rows keep today's shape without a ctable
    from semantic_pyramid_for_image_generation_amd import models
    u, t, c = object(), object(), object()
    assert models._aug_row(u) == (u, None, None) and models._aug_row((u, t)) == (u, t, None) and models._aug_row((u, None, c)) == (u, None, c)
    seen = []
    mw.discriminator._augment = None
    mw._d_call(lambda: seen.append(mw.discriminator._augment), (u,), tables=(t,))
    mw._d_call(lambda: seen.append(mw.discriminator._augment), (u,))
    mw._d_call(lambda: seen.append(mw.discriminator._augment), (u,), ctables=(c,))
    mw._d_call(lambda: seen.append(mw.discriminator._augment), (u, u), tables=(t, t), ctables=(c, c))
    assert seen == [(5, (u, t)), (5, u), (5, (u, None, c)), (5, (u, t, c), (u, t, c))] and mw.discriminator._augment is None


def test_header_declares_the_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert protos["sp_augment_cmat_decode"][1] == [p, i32, i32, p, p]
    assert protos["sp_augment_cmat_ingest"][1] == [p, i32, i64, i64, i64, i64, p, i32, i32, i32, i32, p, i32, p, p, p, p, i32, p]
    assert protos["sp_augment_cmat_ingest_bwd"][1] == [p, i32, p, i32, i32, i32, p, i32, p, p, p, p, i32, p]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sp_augment_cmat_decode", "sp_augment_cmat_ingest", "sp_augment_cmat_ingest_bwd"):
        for suffix in ("", "__b16", "__h16"):
            assert hasattr(handle, name + suffix), name + suffix
    text = open(_lib.HEADER).read()
    assert "SP_CMAT_BRIGHTNESS = 1, SP_CMAT_CONTRAST = 2, SP_CMAT_LUMAFLIP = 4, SP_CMAT_HUE = 8, SP_CMAT_SATURATION = 16" in text


def test_every_refusal_needs_no_gpu():
    """The launchers check their arguments before they touch the device: NULL z / ctable, cmat outside 1 ... 31, n <= 0, and what the
    augmenting ingest refuses already (NULL pointers, cp < 3, a bad dtype, a bad policy, color without partials), under the new names."""
    lib = _lib.lib()
    raw = (ctypes.c_float * 96)()
    b = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)          # 16-byte aligned, as a ctable has to be
    dec = lib.sp_augment_cmat_decode
    assert dec(None, 1, 31, b, None) != 0 and b"sp_augment_cmat_decode" in lib.sp_last_error_string()
    assert dec(b, 1, 31, None, None) != 0 and b"sp_augment_cmat_decode" in lib.sp_last_error_string()
    for n in (0, -1):
        assert dec(b, n, 31, b, None) != 0 and b"sp_augment_cmat_decode" in lib.sp_last_error_string()
    for cmat in (0, 32, -1):
        assert dec(b, 1, cmat, b, None) != 0 and b"cmat" in lib.sp_last_error_string()
    fwd = lib.sp_augment_cmat_ingest
    good = [b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 5, b, b, b, None, 0, None]

    def refused(fn, args, at, value):
        a = list(args)
        a[at] = value
        return fn(*a) != 0
    assert refused(fwd, good, 0, None) and b"sp_augment_cmat_ingest:" in lib.sp_last_error_string()
    assert refused(fwd, good, 6, None) and refused(fwd, good, 11, None)                                       # dst, u
    assert refused(fwd, good, 14, None) and b"sp_augment_cmat_ingest:" in lib.sp_last_error_string()          # ctable
    assert refused(fwd, good, 14, ctypes.c_void_p(b.value + 4))                                               # a misaligned ctable
    assert refused(fwd, good, 10, 2)                                                                          # cp < 3
    assert refused(fwd, good, 1, 7) and refused(fwd, good, 17, 7)                                             # bad dtypes
    assert refused(fwd, good, 12, 8) and b"sp_augment_cmat_ingest:" in lib.sp_last_error_string()             # policy out of range
    assert refused(fwd, good, 15, None)                                                                       # color without partials
    assert refused(fwd, good, 7, 0) and refused(fwd, good, 7, -3) and refused(fwd, good, 8, 0)                # n <= 0, h = 0
    plain = list(good)
    plain[13] = None                                                                                          # the plain family: the same checks
    assert refused(fwd, plain, 14, None) and refused(fwd, plain, 0, None) and refused(fwd, plain, 15, None) and refused(fwd, plain, 7, 0)
    bwd = lib.sp_augment_cmat_ingest_bwd
    good = [b, 4, b, 1, 4, 4, b, 5, b, b, b, None, 0, None]
    assert refused(bwd, good, 0, None) and b"sp_augment_cmat_ingest_bwd" in lib.sp_last_error_string()
    assert refused(bwd, good, 2, None) and refused(bwd, good, 6, None)                                        # dsrc, u
    assert refused(bwd, good, 9, None) and b"sp_augment_cmat_ingest_bwd" in lib.sp_last_error_string()        # ctable
    assert refused(bwd, good, 1, 2) and refused(bwd, good, 12, 7) and refused(bwd, good, 7, 8) and refused(bwd, good, 10, None)
    assert refused(bwd, good, 3, 0)
    # the python layer refuses before any launch too
    with pytest.raises(_lib.SempyrError):
        ops.augment_cmat_decode(torch.zeros(2, 8), 31)                                                        # a CPU tensor
    with pytest.raises(_lib.SempyrError):
        ops.augment_ingest_image(torch.zeros(2, 3, 8, 8), torch.float32, torch.zeros(2, 8), "color", ctable=torch.zeros(2, 12))
