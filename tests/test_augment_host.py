"""Host side of the differentiable augmentation (csrc/augment.hip; tests/test_gpu_augment.py and
tests/test_gpu_augment_step.py have the GPU side): the decoding of the uniforms, the restatement's closed-form backward against
autograd, the rounding bound the GPU tests hold the kernels to, the ABI, and the policy's parsing.  No GPU."""
import ctypes

import pytest
import torch

import augment_restated as A
import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, config, ops

LAST = 1.0 - 2.0 ** -24          # the largest fp32 below 1
POLICIES = ("color", "translation", "cutout", "color,translation", "color,cutout", "translation,cutout", "color,translation,cutout")


def _probe(count):
    """Uniforms that reach every bin of a `count`-way split: 0, the largest value below 1, a fine grid, and the fp32 neighbours of
    every bin edge j / count."""
    edges = torch.arange(1, count, dtype=torch.float64) / count
    near = torch.cat([edges.float(), torch.nextafter(edges.float(), torch.tensor(0.0)), torch.nextafter(edges.float(), torch.tensor(1.0))])
    grid = torch.arange(0, 8192, dtype=torch.float32) / 8192.0
    v = torch.cat([torch.tensor([0.0, LAST]), grid, near]).float()
    assert float(v.min()) == 0.0 and float(v.max()) == LAST
    return v


@pytest.mark.parametrize("h", [16, 20, 40, 256])
def test_decode_reaches_every_integer_of_each_range_and_no_other(h):
    """t in [-r, r] and c in [0, n - 1], all of them and nothing else, u = 0 and u = 1 - 2^-24 included (the product u * float(count)
    may round up to count: the min() of the definition is what keeps the last value inside); o and s stay in their half-open ranges, k = u2 + 0.5 reaches 1.5 by rounding."""
    w = h + 8
    ry, rx, qy, qx, ny, nx = ops.augment_geometry(h, w)
    assert (ry, rx) == (int(h / 8 + 0.5), int(w / 8 + 0.5)) and (qy, qx) == (int(h / 2 + 0.5), int(w / 2 + 0.5))
    assert (ny, nx) == (h + 1 - qy % 2, w + 1 - qx % 2)
    for col, count, lo in ((3, 2 * ry + 1, -ry), (4, 2 * rx + 1, -rx), (5, ny, 0), (6, nx, 0)):
        v = _probe(count)
        u = torch.zeros(v.numel(), 8)
        u[:, col] = v
        got = ops.augment_decode(u, h, w)[col]
        assert got.dtype == torch.int64
        assert sorted(set(got.tolist())) == list(range(lo, lo + count)), (h, col)
        assert int(got[0]) == lo and int(got[1]) == lo + count - 1            # u = 0 and u = 1 - 2^-24
        order = torch.argsort(v, stable=True)
        assert bool((got[order][1:] >= got[order][:-1]).all())                 # monotone in u
    v = _probe(7)
    u = v[:, None].repeat(1, 8)
    o, s, k = ops.augment_decode(u, h, w)[:3]
    assert all(t.dtype == torch.float32 for t in (o, s, k))
    assert float(o.min()) == -0.5 and float(o.max()) < 0.5
    assert float(s.min()) == 0.0 and float(s.max()) < 2.0
    assert float(k.min()) == 0.5 and float(k.max()) == 1.5          # (1 - 2^-24) + 0.5 is a tie in fp32 and rounds to even


def test_a_policy_part_left_out_decodes_to_the_identity():
    u = torch.rand(5, 8, generator=torch.Generator().manual_seed(0))
    o, s, k, ty, tx, _, _ = ops.augment_decode(u, 20, 20, "cutout")
    assert o.tolist() == [0.0] * 5 and s.tolist() == [1.0] * 5 and k.tolist() == [1.0] * 5 and ty.tolist() == [0] * 5 and tx.tolist() == [0] * 5
    x = torch.randn(5, 3, 20, 20, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.equal(A.forward(x, u, ""), x)
    assert torch.equal(A.backward(x, u, ""), x)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("shape", [(3, 3, 16, 24), (4, 3, 20, 20)])
def test_autograd_of_the_float64_restatement_equals_the_closed_form(shape, policy):
    g = torch.Generator().manual_seed(100 * len(policy) + shape[2])
    x = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    u = torch.rand(shape[0], 8, generator=g)
    u[0, 3:7] = torch.tensor([0.0, LAST, 0.0, LAST])          # a corner translation, a window that hangs over two edges
    (dx,) = torch.autograd.grad(A.forward(x, u, policy), x, dy)
    want = A.backward(dy, u, policy)
    assert float((dx - want).abs().max()) <= 1e-12


def test_u_for_decodes_to_what_it_was_asked_for():
    h, w = 20, 20
    u = torch.tensor([A.u_for(-0.25, 0.5, 0.75, -3, 3, 20, 0, h, w), A.u_for(0.4375, 1.9375, 1.4375, 3, 0, 0, 10, h, w)], dtype=torch.float32)
    o, s, k, ty, tx, cy, cx = ops.augment_decode(u, h, w)
    assert o.tolist() == [-0.25, 0.4375] and s.tolist() == [0.5, 1.9375] and k.tolist() == [0.75, 1.4375]
    assert ty.tolist() == [-3, 3] and tx.tolist() == [3, 0] and cy.tolist() == [20, 0] and cx.tolist() == [0, 10]


@pytest.mark.parametrize("policy", POLICIES)
def test_fp32_restatement_stays_within_the_rounding_bound_of_float64(policy):
    """The reference alone meets the bound the GPU tests use: on exact-sum operands (multiples of 2^-8 in [-1, 1), maps up to 64 x 64:
    every per-image sum is exact in fp32 in any order - asserted here) the fp32 evaluation of the transform and of its backward stays
    within augment_restated.forward_bound / backward_bound of the float64 one.  The bound is derived in that module's docstring from
    the roundings of the expressions: first-order propagation of U = 2^-24 per fp32 operation, times 1 + 2^-10 for the second-order
    terms; nothing in it comes from a kernel's output.  It is a few units in the last place, not a tolerance: at |x| < 1, o, s, k in
    range, every result stays below 16 and the bound below 2^-17 (asserted), and it is exactly 0 where the policy only moves data."""
    for i, (shape, u) in enumerate(A.bound_cases()):
        x = A.exact_operands(shape, 10 + i)
        dy = A.exact_operands(shape, 20 + i)
        assert torch.equal(x.sum(dim=(1, 2, 3)).double(), x.double().sum(dim=(1, 2, 3)))
        g1 = A.backward(dy, u, ops.augment_policy(policy) & ~A.COLOR, torch.float32)
        assert torch.equal(g1.sum(dim=(1, 2, 3)).double(), g1.double().sum(dim=(1, 2, 3)))
        for fn, bound_fn, arg in ((A.forward, A.forward_bound, x), (A.backward, A.backward_bound, dy)):
            want = fn(arg, u, policy, torch.float64)
            got = fn(arg, u, policy, torch.float32)
            assert got.dtype == torch.float32
            bound = bound_fn(arg, u, policy)
            assert bool(((got.double() - want).abs() <= bound).all()), (policy, shape, float(((got.double() - want).abs() - bound).max()))
            assert float(bound.max()) <= 2.0 ** -17
            if "color" not in policy:
                assert float(bound.max()) == 0.0 and torch.equal(got.double(), want)
            else:
                assert float(bound.max()) > 0.0
                # the bound is tight enough to notice one misplaced rounding: an error of 2^-16 on any element breaks it
                assert float(want.abs().max()) < 16.0


def test_header_declares_the_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert protos["sp_augment_slices"][1] == [i32, i32, i32, p]
    assert protos["sp_augment_ingest"][1] == [p, i32, i64, i64, i64, i64, p, i32, i32, i32, i32, p, i32, p, i32, p]
    assert protos["sp_augment_ingest_bwd"][1] == [p, i32, p, i32, i32, i32, p, i32, p, i32, p]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sp_augment_slices", "sp_augment_ingest", "sp_augment_ingest_bwd"):
        assert hasattr(handle, name), name
    text = open(_lib.HEADER).read()
    assert "The reference has NO counterpart" in text and "SP_AUG_COLOR = 1, SP_AUG_TRANSLATION = 2, SP_AUG_CUTOUT = 4" in text
    assert (ops.AUG_COLOR, ops.AUG_TRANSLATION, ops.AUG_CUTOUT) == (1, 2, 4)
    assert _lib.lib().sp_version() == 1


def test_slices_and_argument_errors_need_no_gpu():
    """sp_augment_slices is host-only: 8192 source elements per forward partial, 2048 pixels per backward partial.  The launchers check
    their arguments before they touch the device."""
    assert ops.augment_slices(16, 24, False) == 1 and ops.augment_slices(16, 24, True) == 1
    assert ops.augment_slices(48, 64, False) == 2 and ops.augment_slices(48, 64, True) == 2
    assert ops.augment_slices(256, 256, False) == 24 and ops.augment_slices(256, 256, True) == 32
    lib = _lib.lib()
    out = ctypes.c_int64(0)
    assert lib.sp_augment_slices(0, 4, 0, ctypes.byref(out)) != 0
    assert lib.sp_augment_slices(4096, 4096, 0, ctypes.byref(out)) != 0          # 3 h w beyond 2^24
    buf = (ctypes.c_float * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sp_augment_ingest(None, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 7, b, 0, None) != 0
    assert b"sp_augment_ingest" in lib.sp_last_error_string()
    assert lib.sp_augment_ingest(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, None, 7, b, 0, None) != 0       # no u
    assert lib.sp_augment_ingest(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 8, b, 0, None) != 0          # policy out of range
    assert lib.sp_augment_ingest(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 1, None, 0, None) != 0       # color without partials
    assert lib.sp_augment_ingest(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 2, b, 6, None, 0, None) != 0       # pitch below 3 channels
    assert lib.sp_augment_ingest_bwd(b, 4, b, 1, 4, 4, None, 6, None, 0, None) != 0
    assert lib.sp_augment_ingest_bwd(b, 4, b, 1, 4, 4, b, 1, None, 0, None) != 0
    assert b"sp_augment_ingest_bwd" in lib.sp_last_error_string()


def test_a_bad_policy_raises():
    for bad in ("flip", "color,flip", "colour", "color translation", 8, -1, 1.5, True):
        with pytest.raises(_lib.SempyrError):
            ops.augment_policy(bad)
    assert ops.augment_policy("") == 0 and ops.augment_policy(None) == 0
    assert ops.augment_policy("cutout, color") == 5 and ops.augment_policy("color,translation,cutout") == 7 and ops.augment_policy(6) == 6
    G, D = torch.nn.Linear(2, 2), sp.Discriminator(channel_factor=16)
    G.latent_dimensions = 2
    with pytest.raises(_lib.SempyrError):
        sp.ModelWrapper(G, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="color,rotation")
    with pytest.raises(_lib.SempyrError):                    # a caller's own discriminator cannot be armed
        sp.ModelWrapper(G, torch.nn.Linear(2, 2), None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="color")
    mw = sp.ModelWrapper(G, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None, augment="cutout,color")
    assert mw._aug_policy == 5 and mw.logger.hyperparameter["augment"] == "color,cutout"
    off = sp.ModelWrapper(G, D, None, None, vgg16=torch.nn.Identity(), save_data_path=None)
    assert off._aug_policy == 0 and "augment" not in off.logger.hyperparameter and D._augment is None
    with pytest.raises(_lib.SempyrError):                    # uniforms for a wrapper that augments nothing
        off._augment_rows(torch.zeros(2, 3, 4, 4), torch.zeros(3, 2, 8))
    assert off._augment_rows(torch.zeros(2, 3, 4, 4), None) is None
    with pytest.raises(_lib.SempyrError):
        mw._augment_rows(torch.zeros(2, 3, 4, 4), torch.zeros(3, 3, 8))


def test_config_reads_sp_augment(monkeypatch):
    assert config.Config().augment == ""
    monkeypatch.setenv("SP_AUGMENT", "color,translation")
    assert config.Config.from_env().augment == "color,translation"
    monkeypatch.delenv("SP_AUGMENT")
    assert config.Config.from_env().augment == ""


def test_non_image_input_raises_before_any_launch():
    u = torch.zeros(2, 8)
    with pytest.raises(_lib.SempyrError):
        ops.augment_ingest_image(torch.zeros(2, 3, 8, 8), torch.float32, u, "color")          # a CPU tensor
    with pytest.raises(_lib.SempyrError):
        ops.augment_decode(torch.zeros(2, 7), 8, 8)
