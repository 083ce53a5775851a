"""The element-wise glue kernels (csrc/eltwise.hip: ingest, masks, activations, attention residual, sigma rescale, permutation, channel
sums; csrc/inception.hip: avgpool3s1, global_avgpool) held to exact values, restated roundings, the two candidates of a contractible
multiply-add, and for tanh a bound of 5 fp32 ulp; operands, references, conditions and the comparison: tests/eltwise_exact_util.py,
checked against itself on the CPU by tests/test_eltwise_harness.py.  DESIGN.md section 21.

The C ABI is called directly, in fp32, bf16 and fp16 storage (the first op-level run of these kernels' fp16 compilation).  Every buffer
a kernel writes is the body of a flat allocation filled with a canary, with canary pads on both sides; the comparison covers the whole
body, so an element the contract says is not written must still hold the canary, and padding the contract says is zero must be zero.
Input padding holds NaN.  Every case is launched twice, into two different canaries; both results are compared.  Every pointer is
aligned as the product's are (16 bytes for fp32 vectors, 8 for 16-bit ones)."""
import ctypes

import pytest
import torch

import eltwise_exact_util as E
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = E.BF16, E.F16, E.F32
PAD = 64
SP_ERR_UNSUPPORTED = -3
BAD_DTYPES = (L.SP_F8, L.SP_F8_F16, 7)


def cases(family):
    rows = [a for dt in E.DTYPES for a in E.table(family, dt)]
    return dict(argnames="args", argvalues=rows, ids=[E.case_id(a) for a in rows])


class Out:
    """[PAD canary][numel x canary][PAD canary] on the device; .t is the body."""

    def __init__(self, numel, dtype, canary):
        self.numel, self.s = numel, canary
        self.buf = torch.full((PAD + numel + PAD,), canary, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + numel]
        assert self.t.data_ptr() % 16 == 0

    def host(self, what=""):
        torch.cuda.synchronize()
        E.assert_sentinel(torch.cat((self.buf[:PAD], self.buf[PAD + self.numel:])), self.s, what)
        return self.t.cpu()

    def untouched(self, what=""):
        torch.cuda.synchronize()
        E.assert_sentinel(self.buf, self.s, what)


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def run(c, launch):
    """launch(canary) -> {name: Out}; twice, into two canaries.  Returns the worst error / bound of the bounded comparisons and the last
    result."""
    worst, got = 0.0, None
    for canary in E.CANARIES:
        outs = launch(canary)
        got = E.Case({k: o.host(c.what) for k, o in outs.items()})
        worst = max(worst, E.compare(c, got, canary))
    return worst, got


def sp(dt):
    return ops.sp_dtype(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------------
def launch_act_fwd(c):
    x = dev(c.x)

    def go(canary):
        y = Out(c.numel, c.dtype, canary)
        L.call("sp_act_fwd", ops.ptr(x), ops.ptr(y.t), c.numel, c.act, sp(c.dtype), ops.stream())
        return dict(y=y)
    return go


@pytest.mark.parametrize(**cases("act_fwd"))
def test_act_fwd_copies_bits_restates_lrelu_and_bounds_tanh(args):
    """NONE: a bit copy; LeakyReLU: max(v, fl32(0.2f v)) bit for bit; ReLU by value; tanh within 5 fp32 ulp of float64 (printed)."""
    c = E.build("act_fwd", args)
    worst, got = run(c, launch_act_fwd(c))
    if c.act == E.ACT_TANH:
        assert worst <= 1.0
        if c.dtype == F32:
            print("tanh fp32 numel %d: worst error %.3f fp32 ulp against float64 (bound %.0f)" % (c.numel, E.tanh_error_ulps(c, got["y"]), E.TANH_ULPS))
    else:
        assert worst == 0.0


@pytest.mark.parametrize(**cases("act_special"))
def test_act_fwd_special_values_follow_the_table(args):
    """+-inf, NaN, +-0: NaN passes through NONE, LeakyReLU and tanh; ReLU(NaN) = 0 as in the convolution epilogues."""
    c = E.build("act_special", args)
    run(c, launch_act_fwd(c))


@pytest.mark.parametrize(**cases("act_bwd"))
def test_act_bwd_is_exact_in_both_kernels(args):
    c = E.build("act_bwd", args)
    dy, y = dev(c.dy), dev(c.y)

    def go(canary):
        dz = Out(c.pixels * c.cp, c.dtype, canary)
        L.call("sp_act_bwd", ops.ptr(dy), ops.ptr(y), ops.ptr(dz.t), c.pixels, c.c, c.cp, c.act, sp(c.dtype), ops.stream())
        return dict(dz=dz)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# attention residual
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**cases("scale_add"))
def test_scale_add_is_exact_or_one_of_two_candidates(args):
    c = E.build("scale_add", args)
    a, b, g = dev(c.a), dev(c.b), dev(c.g)

    def go(canary):
        y = Out(c.numel, c.dtype, canary)
        L.call("sp_scale_add", ops.ptr(a), ops.ptr(b), ops.ptr(g), ops.ptr(y.t), c.numel, sp(c.dtype), ops.stream())
        return dict(y=y)
    assert run(c, go)[0] == 0.0


@pytest.mark.parametrize(**cases("scale_add_bwd"))
def test_scale_add_bwd_restates_da_and_sums_dg_exactly(args):
    """partials: exactly 512 floats between canaries, [0, blocks) written with the blocks' own sums."""
    c = E.build("scale_add_bwd", args)
    dy, a, g = dev(c.dy), dev(c.a), dev(c.g)

    def go(canary):
        da, dg, part = Out(c.numel, c.dtype, canary), Out(1, F32, canary), Out(512, F32, canary)
        L.call("sp_scale_add_bwd", ops.ptr(dy), ops.ptr(a), ops.ptr(g), ops.ptr(da.t), ops.ptr(dg.t), ops.ptr(part.t), c.numel, sp(c.dtype),
               ops.stream())
        return dict(da=da, dg=dg, partials=part)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# sigma rescale
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**cases("rescale"))
def test_rescale_bias_reads_the_right_sigma_slots_and_keeps_the_padding(args):
    c = E.build("rescale", args)
    x, bias, sa, sb = dev(c.x), dev(c.bias), dev(c.sig_a), dev(c.sig_b)

    def go(canary):
        y = Out(c.rows * c.ldy, c.dtype, canary)
        L.call("sp_rescale_bias", ops.ptr(x), ops.ptr(y.t), c.rows, c.c, c.ldx, c.ldy, ops.ptr(bias), ops.ptr(sa), ops.ptr(sb), sp(c.dtype),
               ops.stream())
        return dict(y=y)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# permutation, channel sums
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**cases("permute"))
def test_permute_moves_bits_and_inverts_itself(args):
    c = E.build("permute", args)
    src = dev(c.src)
    total = c.b * c.c * c.hw

    def go(canary):
        dst, back = Out(total, c.dtype, canary), Out(total, c.dtype, canary)
        L.call("sp_permute_chw_hwc", ops.ptr(src), ops.ptr(dst.t), c.b, c.c, c.hw, c.to_hwc, sp(c.dtype), ops.stream())
        L.call("sp_permute_chw_hwc", ops.ptr(dst.t), ops.ptr(back.t), c.b, c.c, c.hw, 1 - c.to_hwc, sp(c.dtype), ops.stream())
        E.assert_exact(E.as_bits(back.host(c.what)), E.as_bits(c.src), "%s there and back" % (c.what,))
        return dict(dst=dst)
    assert run(c, go)[0] == 0.0


@pytest.mark.parametrize(**cases("channel_sum"))
def test_channel_sum_is_the_float64_sum_and_writes_only_its_blocks_rows(args):
    """partials: exactly 512 x C floats between canaries; out is followed by a canary; the padding columns of x hold NaN."""
    c = E.build("channel_sum", args)
    x = dev(c.x)

    def go(canary):
        out, part = Out(c.c, F32, canary), Out(512 * c.c, F32, canary)
        L.call("sp_channel_sum", ops.ptr(x), c.ld, c.pixels, c.c, ops.ptr(out.t), ops.ptr(part.t), sp(c.dtype), ops.stream())
        return dict(out=out, partials=part)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**cases("mask_concat"))
def test_mask_concat_puts_the_mask_in_channel_c_and_zeros_behind_it(args):
    c = E.build("mask_concat", args)
    feat, mask = dev(c.feat), dev(c.mask)

    def go(canary):
        out = Out(c.pixels * c.cp, c.dtype, canary)
        L.call("sp_mask_concat", ops.ptr(feat), ops.ptr(mask), ops.ptr(out.t), c.pixels, c.c, c.cp, sp(c.dtype), ops.stream())
        return dict(out=out)
    assert run(c, go)[0] == 0.0


@pytest.mark.parametrize(**cases("mask_mul"))
def test_mask_mul_2d_zeroes_the_padding_columns(args):
    c = E.build("mask_mul", args)
    feat, mask = dev(c.feat), dev(c.mask)

    def go(canary):
        out = Out(c.b * c.ldo, c.dtype, canary)
        L.call("sp_mask_mul_2d", ops.ptr(feat), c.ldf, ops.ptr(mask), ops.ptr(out.t), c.ldo, c.b, c.k, sp(c.dtype), ops.stream())
        return dict(out=out)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# ingest
# ------------------------------------------------------------------------------------------------------------------------------------
def float3(values):
    return None if values is None else ctypes.cast((ctypes.c_float * 3)(*values), ctypes.c_void_p)


def run_ingest(c):
    src = dev(c.src)
    at = ctypes.c_void_p(src.data_ptr() + c.off * src.element_size())
    sn, sc, sh, sw = c.strides

    def go(canary):
        dst = Out(c.n * c.h * c.w * c.cp, c.dtype, canary)
        L.call("sp_ingest_image", at, sp(c.src_dtype), sn, sc, sh, sw, ops.ptr(dst.t), c.n, c.c, c.h, c.w, c.cp, float3(c.scale), float3(c.shift),
               sp(c.dtype), ops.stream())
        return dict(dst=dst)
    assert run(c, go)[0] == 0.0


INGEST = {(s, d): [a for a in E.table("ingest", d) if a[0] == s] for s, d in E.INGEST_PAIRS}


@pytest.mark.parametrize("pair", E.INGEST_PAIRS, ids=["%s-to-%s" % (E.NAME[s], E.NAME[d]) for s, d in E.INGEST_PAIRS])
@pytest.mark.parametrize("shape", E.INGEST_SHAPES, ids=[E.sid(s) for s in E.INGEST_SHAPES])
def test_ingest_follows_strides_channels_and_padding(pair, shape):
    """Contiguous, channels-last and cropped sources; C in {1, 2, 3} at pitch C and at the padded pitch; per-channel scale and shift
    (exact), the VGG constants (candidates) and none."""
    rows = [a for a in INGEST[pair] if a[2:5] == shape]
    assert rows
    for a in rows:
        run_ingest(E.build("ingest", a))


@pytest.mark.parametrize(**cases("ingest_bwd"))
def test_ingest_bwd_reads_the_padded_pitch_and_writes_pitch_c(args):
    c = E.build("ingest_bwd", args)
    dy = dev(c.dy)

    def go(canary):
        dsrc = Out(c.pixels * c.c, c.dtype, canary)
        L.call("sp_ingest_image_bwd", ops.ptr(dy), c.cp, ops.ptr(dsrc.t), c.c, c.pixels, float3(c.scale), sp(c.dtype), ops.stream())
        return dict(dsrc=dsrc)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# the Inception pools
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**cases("avg3"))
def test_avgpool3s1_divides_every_window_sum_by_nine(args):
    c = E.build("avg3", args)
    n, h, w, ch = c.shape
    x = dev(c.x)

    def go(canary):
        y = Out(n * h * w * ch, c.dtype, canary)
        L.call("sp_avgpool3s1_fwd", ops.ptr(x), ops.ptr(y.t), n, h, w, ch, sp(c.dtype), ops.stream())
        return dict(y=y)
    assert run(c, go)[0] == 0.0


@pytest.mark.parametrize(**cases("global_avg"))
def test_global_avgpool_is_one_division_of_the_exact_sum(args):
    c = E.build("global_avg", args)
    x = dev(c.x)

    def go(canary):
        y = Out(c.n * c.c, F32, canary)
        L.call("sp_global_avgpool_f32", ops.ptr(x), ops.ptr(y.t), c.n, c.hw, c.c, sp(c.dtype), ops.stream())
        return dict(y=y)
    assert run(c, go)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals: valid device buffers, sized for fp32 and for every scratch extent, so that even a wrongly accepted call stays in bounds
# ------------------------------------------------------------------------------------------------------------------------------------
ROOM = 8192


def refusal_calls(lib, p, o1, o2, o3, st):
    """name -> f(dtype, act): every entry of csrc/eltwise.hip on small extents; p: an input of ROOM floats, o1 .. o3: outputs of ROOM."""
    return {
        "sp_ingest_image": lambda d, a: lib.sp_ingest_image(p, L.SP_F32, 12, 4, 2, 1, o1, 1, 3, 2, 2, 4, None, None, d, st),
        "sp_ingest_image_bwd": lambda d, a: lib.sp_ingest_image_bwd(p, 4, o1, 3, 4, None, d, st),
        "sp_mask_concat": lambda d, a: lib.sp_mask_concat(p, p, o1, 4, 4, 8, d, st),
        "sp_mask_mul_2d": lambda d, a: lib.sp_mask_mul_2d(p, 8, p, o1, 8, 2, 8, d, st),
        "sp_act_fwd": lambda d, a: lib.sp_act_fwd(p, o1, 16, a, d, st),
        "sp_act_bwd": lambda d, a: lib.sp_act_bwd(p, p, o1, 4, 4, 4, a, d, st),
        "sp_act_bwd (re-pitching)": lambda d, a: lib.sp_act_bwd(p, p, o1, 4, 3, 4, a, d, st),
        "sp_scale_add": lambda d, a: lib.sp_scale_add(p, p, p, o1, 16, d, st),
        "sp_rescale_bias": lambda d, a: lib.sp_rescale_bias(p, o1, 2, 8, 8, 8, p, p, p, d, st),
        "sp_rescale_bias (scalar)": lambda d, a: lib.sp_rescale_bias(p, o1, 2, 7, 8, 8, p, p, p, d, st),
        "sp_scale_add_bwd": lambda d, a: lib.sp_scale_add_bwd(p, p, p, o1, o2, o3, 16, d, st),
        "sp_permute_chw_hwc": lambda d, a: lib.sp_permute_chw_hwc(p, o1, 2, 3, 4, 1, d, st),
        "sp_channel_sum": lambda d, a: lib.sp_channel_sum(p, 8, 4, 8, o1, o3, d, st),
    }


def test_an_unknown_dtype_or_activation_is_refused_and_nothing_is_written():
    lib, st = L.lib(), ops.stream()
    src = torch.ones(ROOM, dtype=F32, device=DEV)
    outs = [Out(ROOM, F32, E.CANARIES[0]) for _ in range(3)]
    calls = refusal_calls(lib, ops.ptr(src), *[ops.ptr(o.t) for o in outs], st)
    for name, f in calls.items():
        for d in BAD_DTYPES:
            assert f(d, E.ACT_LRELU) == SP_ERR_UNSUPPORTED, (name, d)
            assert name.split(" ")[0].encode() in lib.sp_last_error_string(), (name, lib.sp_last_error_string())
    for name in ("sp_act_fwd", "sp_act_bwd", "sp_act_bwd (re-pitching)"):
        for d in (L.SP_F32, L.SP_BF16, L.SP_F16):
            for act in (-1, 4, 7):
                assert calls[name](d, act) == SP_ERR_UNSUPPORTED, (name, d, act)
    for o in outs:
        o.untouched("a refused call wrote")
    for name, f in calls.items():                                  # the same calls are accepted in the three storage types
        for d in (L.SP_F32, L.SP_BF16, L.SP_F16):
            assert f(d, E.ACT_LRELU) == 0, (name, d, lib.sp_last_error_string())
    torch.cuda.synchronize()


def test_the_two_16_bit_types_never_mix_in_any_ingest_entry():
    """A bf16 source under fp16 storage used to be read as fp16 bits; an fp16 source needs fp16 storage.  All five entries with a
    src_dtype parameter return SP_ERR_UNSUPPORTED for both mixes and leave the output as it was."""
    lib, st = L.lib(), ops.stream()
    n, h, w, cp = 1, 4, 4, 8
    src = torch.ones(ROOM, dtype=F32, device=DEV)
    u = torch.zeros(n, 8, dtype=F32, device=DEV)
    gate = torch.ones(1, dtype=F32, device=DEV)
    geo = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0]], dtype=F32, device=DEV)
    cmat = torch.tensor([[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=F32, device=DEV)
    dst = Out(ROOM, F32, E.CANARIES[0])
    p, o = ops.ptr(src), ops.ptr(dst.t)
    head = lambda s: (p, s, 3 * h * w, h * w, w, 1, o)                                                        # noqa: E731
    entries = {
        "sp_ingest_image": lambda s, d: lib.sp_ingest_image(*head(s), n, 3, h, w, cp, None, None, d, st),
        "sp_augment_ingest": lambda s, d: lib.sp_augment_ingest(*head(s), n, h, w, cp, ops.ptr(u), 0, None, d, st),
        "sp_augment_ingest_gated": lambda s, d: lib.sp_augment_ingest_gated(*head(s), n, h, w, cp, ops.ptr(u), 0, None, ops.ptr(gate), d, st),
        "sp_augment_geom_ingest": lambda s, d: lib.sp_augment_geom_ingest(*head(s), n, h, w, cp, ops.ptr(u), 0, ops.ptr(geo), None, None, d, st),
        "sp_augment_cmat_ingest": lambda s, d: lib.sp_augment_cmat_ingest(*head(s), n, h, w, cp, ops.ptr(u), 0, None, ops.ptr(cmat), None, None, d, st),
    }
    for name, f in entries.items():
        for s, d in ((L.SP_BF16, L.SP_F16), (L.SP_F16, L.SP_BF16), (L.SP_F16, L.SP_F32)):
            assert f(s, d) == SP_ERR_UNSUPPORTED, (name, s, d)
            assert name.encode() in lib.sp_last_error_string() and b"source" in lib.sp_last_error_string(), lib.sp_last_error_string()
    dst.untouched("a refused ingest wrote")
    for name, f in entries.items():                                # the pairs the product uses are accepted
        for s, d in ((L.SP_F32, L.SP_F16), (L.SP_F16, L.SP_F16), (L.SP_BF16, L.SP_BF16), (L.SP_F32, L.SP_F32)):
            assert f(s, d) == 0, (name, s, d, lib.sp_last_error_string())
    torch.cuda.synchronize()
    img = torch.zeros(1, 3, 4, 4, dtype=BF16, device=DEV)
    with pytest.raises(L.SempyrError, match="cannot be ingested"):
        ops.ingest_image(img, F16)
    with pytest.raises(L.SempyrError, match="cannot be ingested"):
        ops.ingest_image_pair(img.half(), img.half(), BF16)
    with pytest.raises(L.SempyrError, match="cannot be ingested"):
        ops.augment_ingest_image(img, F16, u, "translation")
    assert ops.ingest_image(img, BF16).dtype == BF16 and ops.ingest_image(img.float(), F16).dtype == F16
