"""Host side of the geometric augmentation (csrc/augment.hip: THE GEOMETRIC FAMILY; tests/test_gpu_geom.py and
tests/test_gpu_geom_step.py have the GPU side): the definition against grid_sample, flip, rot90 and section 11's translation, the
closed-form gather against autograd and the size of its box, the decode's ranges, the rounding bound the GPU tests hold the kernels to,
the parsing of the words, and the ABI's refusals.  No GPU."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import augment_restated as A
import geom_restated as G
import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, ops

LAST = G.LAST
ALL = "xflip,rot90,scale,rotate"


def _rand(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _uv(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 8, generator=g), torch.rand(n, 4, generator=g)


@pytest.mark.parametrize("h,w,geom", [(12, 12, ALL), (9, 9, "rot90,rotate"), (8, 12, "xflip,scale,rotate"), (5, 7, "scale")])
def test_float64_restatement_is_grid_sample_with_zero_padding_and_aligned_corners(h, w, geom):
    n = 6
    u, v = _uv(n, 3 * h + w)
    v[:4] = G.end_rows()[:4]
    tab = G.table(u, v, h, w, "translation", geom)
    x = _rand((n, 3, h, w), 1)
    y, xx = G.coords(tab, h, w, torch.float64)
    grid = torch.stack([2 * xx / (w - 1) - 1, 2 * y / (h - 1) - 1], dim=-1)
    want = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    got = G.forward(x, u, tab, "", torch.float64)
    assert float((got - want).abs().max()) <= 1e-12
    assert float(want.abs().max()) > 0.1


def test_integer_maps_equal_flip_rot90_and_section_11s_translation_exactly():
    n, h = 8, 12
    x = _rand((n, 3, h, h), 2)
    u, _ = _uv(n, 5)
    v = torch.tensor([G.v_for(flip=bool(i % 2), k=i % 4) for i in range(n)], dtype=torch.float32)
    for dtype in (torch.float64, torch.float32):
        xd = x.to(dtype)
        got = G.forward(xd, u, G.table(u, v, h, h, "", "xflip", dtype), "", dtype)
        for i in range(n):
            assert torch.equal(got[i], xd[i].flip(-1) if i % 2 else xd[i])
        got = G.forward(xd, u, G.table(u, v, h, h, "", "rot90", dtype), "", dtype)
        for i in range(n):
            assert torch.equal(got[i], torch.rot90(xd[i], i % 4, (-2, -1))), i
        got = G.forward(xd, u, G.table(u, v, h, h, "", "xflip,rot90", dtype), "", dtype)
        for i in range(n):          # out = rot90^k(flip(x)): the inverse map applies F last, so the flip acts on the source first
            assert torch.equal(got[i], torch.rot90(xd[i].flip(-1) if i % 2 else xd[i], i % 4, (-2, -1))), i
        # translation alone, through a table: section 11's translation (non-square map too)
        for hh, ww in ((h, h), (8, 20)):
            xs = _rand((n, 3, hh, ww), 3).to(dtype)
            tab = ops.augment_geom_table(u, v, hh, ww, "translation", 0, dtype)
            assert torch.equal(G.forward(xs, u, tab, "", dtype), A.forward(xs, u, "translation", dtype))
            assert torch.equal(G.backward(xs, u, tab, "", dtype), A.backward(xs, u, "translation", dtype))
    # rows without scale and rotate are exact: entries in {-1, 0, 1}
    tab = G.table(u, v, h, h, "translation", "xflip,rot90", torch.float32)
    assert set(tab[:, [0, 1, 3, 4]].abs().flatten().tolist()) == {0.0, 1.0}
    assert torch.equal(tab.double(), G.table(u, v, h, h, "translation", "xflip,rot90", torch.float64))


def _end_case(h, w, geom):
    v = G.end_rows()
    n = v.shape[0]
    u, _ = _uv(n, h)
    u[0, 3:7] = torch.tensor([0.0, LAST, 0.0, LAST])
    return u, v, G.table(u, v, h, w, "translation", geom)


@pytest.mark.parametrize("policy", ["", "cutout", "color", "color,cutout"])
@pytest.mark.parametrize("h,w,geom", [(12, 12, ALL), (7, 11, "xflip,scale,rotate")])
def test_closed_form_gather_equals_autograd_with_the_box_of_2_and_not_with_1(h, w, geom, policy):
    """e = -0.4 and (just below) +0.4, theta = -45 and (just below) +45 degrees, every flip x k: the +-2 box holds every contributor; a
    +-1 box loses some where the image is magnified (L^-1 has scale 2^e = 1.32 and the rotation spreads it by sqrt(2))."""
    u, v, tab = _end_case(h, w, geom)
    n = v.shape[0]
    dy = _rand((n, 3, h, w), 7)
    want = G.backward_autograd(dy, u, tab, policy)
    got = G.backward(dy, u, tab, policy, box=2)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((G.backward(dy, u, tab, policy, box=3) - want).abs().max()) <= 1e-12
    short = G.backward(dy, u, tab, policy, box=1)
    assert float((short[1] - want[1]).abs().max()) > 1e-3          # row 1: e = +0.4, theta = +45 degrees


def test_box_of_2_holds_at_the_tables_the_entries_are_specified_for():
    """L = I / 2 (L^-1 = 2 I, |a00| + |a01| = 2: the edge of the specification) and L = 2 I, with half-pixel offsets."""
    h = w = 12
    u = torch.zeros(1, 8)
    dy = _rand((1, 3, h, w), 9)
    for L, off in ((((0.5, 0.0), (0.0, 0.5)), (2.75, 1.25)), (((2.0, 0.0), (0.0, 2.0)), (-5.5, -3.0)), (((0.0, -0.5), (0.5, 0.0)), (6.25, 0.0))):
        tab = G.table_of(L, off)
        assert float((G.backward(dy, u, tab, "") - G.backward_autograd(dy, u, tab, "")).abs().max()) <= 1e-12


def test_decode_reaches_k_0_to_3_and_no_other_and_both_sides_of_the_flip():
    edges = torch.tensor([0.25, 0.5, 0.75])
    probe = torch.cat([torch.tensor([0.0, LAST]), torch.arange(0, 4096, dtype=torch.float32) / 4096.0, edges,
                       torch.nextafter(edges, torch.tensor(0.0)), torch.nextafter(edges, torch.tensor(1.0))])
    n = probe.numel()
    u = torch.zeros(n, 8)
    v = torch.zeros(n, 4)
    v[:, 1] = probe
    v[:, 0] = 0.75
    tab = ops.augment_geom_table(u, v, 8, 8, 0, "rot90")
    quarter = {(1.0, 0.0, 0.0, 1.0): 0, (0.0, 1.0, -1.0, 0.0): 1, (-1.0, 0.0, 0.0, -1.0): 2, (0.0, -1.0, 1.0, 0.0): 3}
    ks = [quarter[tuple(float(t) + 0.0 for t in row[[0, 1, 3, 4]])] for row in tab]
    assert sorted(set(ks)) == [0, 1, 2, 3]
    assert ks[0] == 0 and ks[1] == 3                                   # v1 = 0 and v1 = 1 - 2^-24
    want = torch.floor(4.0 * probe.double()).clamp(max=3).to(torch.int64).tolist()
    assert ks == want
    v = torch.zeros(4, 4)
    v[:, 0] = torch.tensor([0.0, float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0))), 0.5, LAST])
    tab = ops.augment_geom_table(torch.zeros(4, 8), v, 8, 8, 0, "xflip")
    assert tab[:, 4].tolist() == [-1.0, -1.0, 1.0, 1.0] and tab[:, 0].tolist() == [1.0] * 4          # flip = v0 < 0.5, strict
    assert tab[:, 5].tolist() == [7.0, 7.0, 0.0, 0.0]
    # the ranges of scale and rotation: magnification 2^e in [0.758, 1.32), |theta| <= 45 degrees
    v = torch.tensor([[0.75, 0.0, 0.0, 0.0], [0.75, 0.0, LAST, LAST]])
    tab = ops.augment_geom_table(torch.zeros(2, 8), v, 8, 8, 0, "scale", torch.float64)
    assert abs(float(tab[0, 0]) - 2 ** 0.4) < 1e-6 and abs(float(tab[1, 0]) - 2 ** -0.4) < 1e-6
    tab = ops.augment_geom_table(torch.zeros(2, 8), v, 8, 8, 0, "rotate", torch.float64)
    assert abs(float(tab[0, 3]) + math.sin(math.pi / 4)) < 1e-6 and abs(float(tab[1, 3]) - math.sin(math.pi / 4)) < 1e-6
    with pytest.raises(_lib.SempyrError):
        ops.augment_geom_table(torch.zeros(2, 8), v, 8, 12, 0, "rot90")
    with pytest.raises(_lib.SempyrError):
        ops.augment_geom_table(torch.zeros(2, 8), torch.zeros(2, 3), 8, 8, 0, "xflip")


@pytest.mark.parametrize("policy", ["", "cutout", "color", "color,cutout"])
@pytest.mark.parametrize("h,w,geom", [(16, 16, ALL), (40, 40, ALL), (64, 64, ALL), (8, 24, "xflip,scale,rotate")])
def test_fp32_restatement_alone_stays_within_the_rounding_bound_of_float64(h, w, geom, policy):
    """On augment_restated.exact_operands (S = sum(x) exact in fp32) the fp32 evaluation of the forward and of the gather backward
    stays within geom_restated.forward_bound / backward_bound of the float64 one, with ONE fp32 table in both.  The bound is derived
    in that module's docstring from the roundings of the expressions; nothing in it comes from a kernel's output."""
    v = G.end_rows()
    n = v.shape[0]
    u = A.bound_cases()[0][1][:n].clone() if (h, w) == (16, 24) else torch.tensor(
        [A.u_for(o, s, k, ty, tx, None, None, h, w) for (o, s, k), (ty, tx) in zip(
            [(-0.5, 0.0, 0.5), (0.4375, 1.9375, 1.4375), (0.0, 1.0, 1.0), (-0.25, 0.5, 0.75), (0.125, 1.5, 1.25), (0.3125, 0.0625, 0.5625)],
            [(-1, 1), (1, 0), (0, 0), (0, -1), (1, 1), (-1, -1)])], dtype=torch.float32)
    u[0, 5:7] = torch.tensor([0.0, LAST])          # a window at an edge
    tab = G.table(u, v, h, w, "translation", geom, torch.float32)
    x = A.exact_operands((n, 3, h, w), 31)
    dy = A.exact_operands((n, 3, h, w), 32)
    assert torch.equal(x.sum(dim=(1, 2, 3)).double(), x.double().sum(dim=(1, 2, 3)))
    for fn, bound_fn, arg in ((G.forward, G.forward_bound, x), (G.backward, G.backward_bound, dy)):
        want = fn(arg, u, tab, policy, torch.float64)
        got = fn(arg, u, tab, policy, torch.float32)
        assert got.dtype == torch.float32
        bound = bound_fn(arg, u, tab, policy)
        excess = (got.double() - want).abs() - bound
        assert float(excess.max()) <= 0.0, (fn.__name__, policy, (h, w), float(excess.max()))
        assert 0.0 < float(bound.max()) <= 2.0 ** -9          # at most a few coordinate roundings at magnitude ~200 times |e| <= 16
    # fp32 autograd agrees with the fp32 gather within the same bound
    diff = (G.backward_autograd(dy, u, tab, policy, torch.float32).double() - G.backward(dy, u, tab, policy, torch.float64)).abs()
    assert float((diff - G.backward_bound(dy, u, tab, policy)).max()) <= 0.0


def test_exact_tables_make_the_fp32_restatement_exact():
    """Hand-written tables - flip x k, half-pixel shifts, L = 2 I, L = I / 2 - on multiples of 2^-8: fp32 equals float64."""
    h = w = 16
    u = torch.zeros(1, 8)
    x, dy = A.exact_operands((1, 3, h, w), 41), A.exact_operands((1, 3, h, w), 42)
    for tab in G.exact_tables(h, w):
        for fn, arg in ((G.forward, x), (G.backward, dy)):
            assert torch.equal(fn(arg, u, tab, "cutout", torch.float32).double(), fn(arg, u, tab, "cutout", torch.float64))


def test_augment_split_keeps_the_old_strings_and_parses_the_new_words():
    for old in ("", None, "color", "cutout, color", "color,translation,cutout", 0, 5, 7):
        assert ops.augment_split(old) == (ops.augment_policy(old), 0)
    assert ops.augment_split("color,xflip") == (1, 1)
    assert ops.augment_split("rotate, rot90 ,cutout") == (4, 10)
    assert ops.augment_split(ALL) == (0, 15)
    assert ops.augment_split("color,xflip,rot90,scale,rotate,translation,cutout") == (7, 15)
    assert ops.augment_geom("scale") == 4 and ops.augment_geom(None) == 0 and ops.augment_geom(15) == 15 and ops.augment_geom("") == 0
    assert (ops.GEOM_XFLIP, ops.GEOM_ROT90, ops.GEOM_SCALE, ops.GEOM_ROTATE) == (1, 2, 4, 8)
    for bad in ("flip", "color,flip", "rotation", "color,rotation", "colour", 8, -1, 1.5, True):
        with pytest.raises(_lib.SempyrError):
            ops.augment_split(bad)
    for bad in ("flip", "color", 16, -1, True, 1.5):
        with pytest.raises(_lib.SempyrError):
            ops.augment_geom(bad)
    G_, D = torch.nn.Linear(2, 2), sp.Discriminator(channel_factor=16)
    G_.latent_dimensions = 2
    mw = sp.ModelWrapper(G_, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="rotate,cutout,xflip,color")
    assert (mw._aug_policy, mw._aug_geom) == (5, 9) and mw.logger.hyperparameter["augment"] == "color,cutout,xflip,rotate"
    only = sp.ModelWrapper(G_, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="rot90")
    assert (only._aug_policy, only._aug_geom) == (0, 2) and only.logger.hyperparameter["augment"] == "rot90"
    with pytest.raises(_lib.SempyrError):
        sp.ModelWrapper(G_, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="color,rotation")
    old = sp.ModelWrapper(G_, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="color")
    assert old._aug_geom == 0 and old._augment_geom_rows(torch.zeros(2, 3, 4, 4), None) is None
    with pytest.raises(_lib.SempyrError):          # v for a wrapper without geometric words
        old._augment_geom_rows(torch.zeros(2, 3, 4, 4), torch.zeros(3, 2, 4))
    with pytest.raises(_lib.SempyrError):          # a wrong shape
        mw._augment_geom_rows(torch.zeros(2, 3, 4, 4), torch.zeros(3, 2, 8))
    assert mw._augment_geom_rows(torch.zeros(2, 3, 4, 4), torch.zeros(3, 2, 4)).shape == (3, 2, 4)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert protos["sp_augment_geom_slices"][1] == [i32, i32, i32, p]
    assert protos["sp_augment_geom_decode"][1] == [p, p, i32, i32, i32, i32, i32, p, p]
    assert protos["sp_augment_geom_ingest"][1] == [p, i32, i64, i64, i64, i64, p, i32, i32, i32, i32, p, i32, p, p, p, i32, p]
    assert protos["sp_augment_geom_ingest_bwd"][1] == [p, i32, p, i32, i32, i32, p, i32, p, p, p, i32, p]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sp_augment_geom_slices", "sp_augment_geom_decode", "sp_augment_geom_ingest", "sp_augment_geom_ingest_bwd"):
        assert hasattr(handle, name), name
    text = open(_lib.HEADER).read()
    assert "SP_GEOM_XFLIP = 1, SP_GEOM_ROT90 = 2, SP_GEOM_SCALE = 4, SP_GEOM_ROTATE = 8" in text


def test_every_refusal_needs_no_gpu():
    """The launchers check their arguments before they touch the device: NULL pointers, cp < 3, a bad dtype, geom outside 1 ... 15,
    rot90 on a non-square map, color without partials."""
    assert ops.augment_geom_slices(16, 24, False) == 1 and ops.augment_geom_slices(64, 64, False) == 2 and ops.augment_geom_slices(64, 64, True) == 2
    lib = _lib.lib()
    out = ctypes.c_int64(0)
    assert lib.sp_augment_geom_slices(0, 4, 0, ctypes.byref(out)) != 0
    assert lib.sp_augment_geom_slices(4, 4, 0, None) != 0
    buf = (ctypes.c_float * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    dec = lib.sp_augment_geom_decode
    assert dec(None, b, 1, 4, 4, 2, 1, b, None) != 0
    assert b"sp_augment_geom_decode" in lib.sp_last_error_string()
    assert dec(b, None, 1, 4, 4, 2, 1, b, None) != 0
    assert dec(b, b, 1, 4, 4, 2, 1, None, None) != 0
    assert dec(b, b, 0, 4, 4, 2, 1, b, None) != 0
    for geom in (0, 16, -1):
        assert dec(b, b, 1, 4, 4, 2, geom, b, None) != 0
    assert dec(b, b, 1, 4, 8, 2, 2, b, None) != 0 and b"square" in lib.sp_last_error_string()          # rot90, non-square
    assert dec(b, b, 1, 4, 8, 2, 15, b, None) != 0
    assert dec(b, b, 1, 4, 4, 8, 1, b, None) != 0                                                       # policy out of range
    fwd = lib.sp_augment_geom_ingest
    good = [b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 5, b, b, None, 0, None]

    def refused(fn, args, at, value):
        a = list(args)
        a[at] = value
        return fn(*a) != 0
    assert refused(fwd, good, 0, None) and b"sp_augment_geom_ingest" in lib.sp_last_error_string()
    assert refused(fwd, good, 6, None) and refused(fwd, good, 11, None) and refused(fwd, good, 13, None)      # dst, u, table
    assert refused(fwd, good, 10, 2)                                                                          # cp < 3
    assert refused(fwd, good, 1, 7) and refused(fwd, good, 16, 7)                                             # bad dtypes
    assert refused(fwd, good, 12, 8)                                                                          # policy out of range
    assert refused(fwd, good, 14, None)                                                                       # color without partials
    assert refused(fwd, good, 8, 0)
    bwd = lib.sp_augment_geom_ingest_bwd
    good = [b, 4, b, 1, 4, 4, b, 5, b, b, None, 0, None]
    assert refused(bwd, good, 0, None) and b"sp_augment_geom_ingest_bwd" in lib.sp_last_error_string()
    assert refused(bwd, good, 2, None) and refused(bwd, good, 6, None) and refused(bwd, good, 8, None)        # dsrc, u, table
    assert refused(bwd, good, 1, 2) and refused(bwd, good, 11, 7) and refused(bwd, good, 7, 8) and refused(bwd, good, 9, None)
    # the python layer refuses before any launch too
    with pytest.raises(_lib.SempyrError):
        ops.augment_geom_decode(torch.zeros(2, 8), torch.zeros(2, 4), 8, 8, 0, "xflip")          # CPU tensors
    with pytest.raises(_lib.SempyrError):
        ops.augment_ingest_image(torch.zeros(2, 3, 8, 8), torch.float32, torch.zeros(2, 8), "color", table=torch.zeros(2, 8))
