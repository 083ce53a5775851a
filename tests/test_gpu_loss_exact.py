"""The discriminator head and the losses (csrc/losses.hip: dhead, LSGAN squared error, semantic reconstruction, diversity) held to
exact values and derived bounds; operands, references, conditions and the comparison: tests/pool_loss_exact_util.py, checked against
itself on the CPU by tests/test_pool_loss_harness.py.

The C ABI is called directly, in fp32, bf16 and fp16 storage.  Every output lies between sentinel pads and starts as sentinel, every
call is made twice with two different sentinels, and where a row pitch exceeds the width the sentinel beyond it must survive.  One
pass per family goes through the autograd functions of ops.py (the head through _DHeadFn with the two packed layers stood in for by
their pointers: discriminator_head itself only looks those up in the spectral-norm bank, whose weights are no integers)."""
import ctypes
import functools
import types

import pytest
import torch

import pool_loss_exact_util as P
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = P.BF16, P.F16, P.F32
SENTINELS, PAD = (-1536.0, 768.0), 64
SP_ERR_INVALID = -1
DT_IDS = [P.NAME[dt] for dt in P.DTYPES]
REC_MULTI = P.REC_MULTI


class Out:
    """[PAD sentinel][rows x pitch, sentinel][PAD sentinel] on the device; .t is the body, .host() its first `cols` columns."""

    def __init__(self, rows, cols, dtype, sentinel, pitch=None):
        self.rows, self.cols, self.pitch, self.s = rows, cols, pitch or cols, sentinel
        self.buf = torch.full((PAD + rows * self.pitch + PAD,), sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + rows * self.pitch]

    def host(self, what=""):
        torch.cuda.synchronize()
        body = self.t.view(self.rows, self.pitch)
        P.assert_sentinel(torch.cat((self.buf[:PAD], self.buf[PAD + self.rows * self.pitch:], body[:, self.cols:].reshape(-1))), self.s, what)
        return body[:, :self.cols].cpu()

    def untouched(self, what=""):
        torch.cuda.synchronize()
        P.assert_sentinel(self.buf, self.s, what)


def dev(t, dt, pitch=None):
    """The float64 operand in `dt` on the device, exactly; pitch: rows of that many elements, 99 behind the width."""
    out = t.to(dt).contiguous()
    assert torch.equal(out.double(), t.double()), "the type does not hold an operand exactly"
    if pitch is None:
        return out.to(DEV)
    buf = torch.full((t.shape[0], pitch), 99.0, dtype=dt, device=DEV)
    buf[:, :t.shape[1]] = out.to(DEV)
    return buf


@functools.lru_cache(maxsize=4)
def built(fn, *args):
    return getattr(P, fn)(*args)


def f32dev(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-dhead
# ------------------------------------------------------------------------------------------------------------------------------------
DHEAD = [(dt, b, f, kind) for dt in P.DTYPES for b, f in P.DHEAD for kind in P.CLASS_KINDS]


@pytest.mark.parametrize("dt,b,f,kind", DHEAD, ids=["%s-b%d-f%d-%s" % (P.NAME[dt], b, f, k) for dt, b, f, k in DHEAD])
def test_discriminator_head_is_exact_over_the_whole_embedding_table(dt, b, f, kind):
    c = built("dhead_case", dt, b, f, kind)
    sp, ldx, lddx = ops.sp_dtype(dt), f + 8, f + 16
    x, emb, wc, bc, dpred = dev(c.x, dt, ldx), dev(c.emb, F32), dev(c.wc, F32), dev(c.bc, F32), dev(c.dpred, F32)
    cls = c.cls.to(DEV)
    for s in SENTINELS:
        pred, dx, demb = Out(b * b, f, F32, s), Out(b, f, dt, s, lddx), Out(P.NUM_CLASSES, f, F32, s)
        dwc, dbc, sdp = Out(1, f, F32, s), Out(1, 1, F32, s), Out(1, b, F32, s)
        L.call("sp_dhead_fwd", ops.ptr(x), ldx, ops.ptr(emb), ops.ptr(cls), ops.ptr(wc), ops.ptr(bc), ops.ptr(pred.t), b, f, sp, ops.stream())
        L.call("sp_dhead_bwd", ops.ptr(dpred), ops.ptr(x), ldx, ops.ptr(emb), ops.ptr(cls), ops.ptr(wc), ops.ptr(dx.t), lddx, ops.ptr(demb.t),
               P.NUM_CLASSES, ops.ptr(dwc.t), ops.ptr(dbc.t), ops.ptr(sdp.t), b, f, sp, ops.stream())
        got = P.Case(pred=pred.host(c.what), dx=dx.host(c.what), demb=demb.host(c.what), dwc=dwc.host(c.what), dbc=dbc.host(c.what), sdp=sdp.host(c.what))
        assert P.compare(c, got) == 0.0
        assert bool((x[:, f:] == 99.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-sqerr
# ------------------------------------------------------------------------------------------------------------------------------------
def run_sqerr(c, misaligned):
    n = c.n
    base = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    off = 1 if misaligned else 0
    base[off:off + n] = c.p.float().to(DEV)
    p = ctypes.c_void_p(base.data_ptr() + 4 * off)
    assert (p.value % 16 != 0) == misaligned
    gout, acc = f32dev(c.gout), torch.zeros(1, dtype=torch.float64, device=DEV)
    worst = 0.0
    for s in SENTINELS:
        loss, dp = Out(1, 1, F32, s), Out(1, n, F32, s)
        L.call("sp_sqerr_loss_fwd", p, n, c.target, ops.ptr(acc), ops.ptr(loss.t), ops.stream())
        L.call("sp_sqerr_loss_bwd", p, n, c.target, ops.ptr(gout), ops.ptr(dp.t), ops.stream())
        worst = max(worst, P.compare(c, P.Case(loss=loss.host(c.what).reshape(1), dp=dp.host(c.what).reshape(-1))))
    return worst


@pytest.mark.parametrize("n", P.SQERR)
def test_sqerr_loss_is_the_nearest_float_and_its_gradient_bit_identical(n):
    worst = 0.0
    for target in (0.0, 1.0):
        c = built("sqerr_case", n, target)
        worst = max(worst, run_sqerr(c, False))
        if n <= P.SQERR_SMALL_MAX:
            worst = max(worst, run_sqerr(c, True))
    print("sqerr n %d: %s, worst error / bound %.3f" % (n, c.checks["loss"][0], worst))
    assert worst <= 1.0 and (worst == 0.0 or c.checks["loss"][0] == "within")


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-rec
# ------------------------------------------------------------------------------------------------------------------------------------
def rec_operands(c, s):
    """Per level: (real, fake, mask, dfake Out, ld_real, ld_fake, ld_dfake, dims) on the device."""
    dt, ops_ = c.dtype, []
    for lv in c.levels:
        if lv.four:
            n, h, w, ch = lv.shape
            real, fake, ld = dev(lv.real, dt), dev(lv.fake, dt), (ch, ch, ch)
            dfake = Out(n * h * w, ch, dt, s)
            dims = (n, h, w, ch)
        else:
            b, k = lv.shape
            ld = tuple(k + e for e in P.LD_EXTRA)
            real, fake = dev(lv.real, dt, ld[0]), dev(lv.fake, dt, ld[1])
            dfake = Out(b, k, dt, s, ld[2])
            dims = (b, 1, 1, k)
        ops_.append((real, fake, dev(lv.mask, F32), dfake, ld, dims))
    return ops_


def level_array(operands, n=None):
    arr = (L.SpRecLevel * (n or len(operands)))()
    for i in range(len(arr)):
        real, fake, mask, dfake, ld, dims = operands[i % len(operands)]
        lv = arr[i]
        lv.real, lv.fake, lv.mask, lv.dfake = real.data_ptr(), fake.data_ptr(), mask.data_ptr(), dfake.t.data_ptr()
        lv.ld_real, lv.ld_fake, lv.ld_dfake = ld
        lv.n, lv.h, lv.w_, lv.c = dims
    return arr


def rec_got(c, operands, loss):
    got = P.Case(loss=loss.host(c.what).reshape(1))
    for i, o in enumerate(operands):
        got["dfake%d" % i] = o[3].host((c.what, i)).reshape(c.levels[i].shape)
    return got


REC_ONE = [(dt, s) for dt in P.DTYPES for s in P.REC_4D + P.REC_2D]


@pytest.mark.parametrize("dt,shape", REC_ONE, ids=["%s-%s" % (P.NAME[dt], P.sid(s)) for dt, s in REC_ONE])
def test_reconstruction_loss_one_level_through_both_entry_points(dt, shape):
    sp = ops.sp_dtype(dt)
    worst = 0.0
    for weight in (1.0, 0.25):
        c = built("rec_case", dt, (shape,), weight)
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        for s in SENTINELS:
            operands = rec_operands(c, s)
            loss = Out(1, 1, F32, s)
            arr = level_array(operands)
            L.call("sp_rec_loss_fwd_levels", arr, 1, ops.ptr(acc), ops.ptr(loss.t), c.weight, sp, ops.stream())
            L.call("sp_rec_loss_bwd_levels", arr, 1, ops.ptr(f32dev(c.gout)), c.weight, sp, ops.stream())
            worst = max(worst, P.compare(c, rec_got(c, operands, loss)))
            assert float(acc.cpu()) == 0.0, "the shared accumulator is not back at zero"
            if weight == 1.0:                                      # the one-level entry points: the accumulator is the caller's
                real, fake, mask, _, ld, (n, h, w, ch) = operands[0]
                operands = rec_operands(c, s)
                dfake, loss = operands[0][3], Out(1, 1, F32, s)
                L.call("sp_rec_loss_fwd", ops.ptr(real), ld[0], ops.ptr(fake), ld[1], ops.ptr(mask), n, h, w, ch, ops.ptr(acc), sp, ops.stream())
                L.call("sp_f64_to_f32", ops.ptr(acc), ops.ptr(loss.t), 1, ops.stream())
                L.call("sp_rec_loss_bwd", ops.ptr(real), ld[0], ops.ptr(fake), ld[1], ops.ptr(mask), ops.ptr(f32dev(c.gout)), ops.ptr(dfake.t), ld[2],
                       n, h, w, ch, sp, ops.stream())
                worst = max(worst, P.compare(c, rec_got(c, operands, loss)))
                acc.zero_()
    print("rec %s %s: %s, worst error / bound %.3f" % (P.NAME[dt], shape, "exact" if c.pow2 else "within", worst))
    assert worst <= 1.0 and (worst == 0.0 or not c.pow2)


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_reconstruction_loss_over_several_levels(dt):
    """1, 4 and 8 levels (one-block and clamped levels mixed: block ranges of 1 .. 1024 blocks); 9 levels are refused."""
    sp = ops.sp_dtype(dt)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    for shapes, weight, masks in REC_MULTI:
        c = built("rec_case", dt, tuple(shapes), weight, masks)
        worst = 0.0
        for s in SENTINELS:
            operands = rec_operands(c, s)
            loss = Out(1, 1, F32, s)
            arr = level_array(operands)
            L.call("sp_rec_loss_fwd_levels", arr, len(operands), ops.ptr(acc), ops.ptr(loss.t), c.weight, sp, ops.stream())
            L.call("sp_rec_loss_bwd_levels", arr, len(operands), ops.ptr(f32dev(c.gout)), c.weight, sp, ops.stream())
            worst = max(worst, P.compare(c, rec_got(c, operands, loss)))
            assert float(acc.cpu()) == 0.0, "the shared accumulator is not back at zero"
        print("rec %s %d levels weight %g: %s, worst error / bound %.3f" % (P.NAME[dt], len(shapes), weight, "exact" if c.pow2 else "within", worst))
        assert worst <= 1.0 and (worst == 0.0 or not c.pow2)
    operands = rec_operands(c, SENTINELS[0])
    loss = Out(1, 1, F32, SENTINELS[0])
    arr = level_array(operands, P.REC_MAX_LEVELS + 1)
    lib = L.lib()
    assert lib.sp_rec_loss_fwd_levels(arr, P.REC_MAX_LEVELS + 1, ops.ptr(acc), ops.ptr(loss.t), 1.0, sp, ops.stream()) == SP_ERR_INVALID
    assert b"levels" in lib.sp_last_error_string()
    assert lib.sp_rec_loss_bwd_levels(arr, P.REC_MAX_LEVELS + 1, ops.ptr(f32dev(1.0)), 1.0, sp, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_rec_loss_fwd_levels(arr, 0, ops.ptr(acc), ops.ptr(loss.t), 1.0, sp, ops.stream()) == SP_ERR_INVALID
    loss.untouched("a refused call wrote the loss")
    for o in operands:
        o[3].untouched("a refused call wrote a gradient")
    assert float(acc.cpu()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# loss-div
# ------------------------------------------------------------------------------------------------------------------------------------
DIVS = [(dt, he, hz) for dt in P.DTYPES for he, hz in P.DIV]


@pytest.mark.parametrize("dt,half_elems,half_z", DIVS, ids=["%s-%d-%d" % (P.NAME[dt], he, hz) for dt, he, hz in DIVS])
def test_diversity_loss_is_bit_identical_to_the_double_restatement(dt, half_elems, half_z):
    sp = ops.sp_dtype(dt)
    for weight in (1.0, 0.25):
        c = built("div_case", dt, half_elems, half_z, weight)
        img, z, gout = dev(c.img, dt), dev(c.z, F32), f32dev(c.gout)
        acc = torch.zeros(2, dtype=torch.float64, device=DEV)
        for s in SENTINELS:
            for entry in (("sp_div_loss_fwd_w", "sp_div_loss_fwd") if weight == 1.0 else ("sp_div_loss_fwd_w",)):
                out, dimg = Out(1, 2, F32, s), Out(2, half_elems, dt, s)
                if entry == "sp_div_loss_fwd":
                    scratch = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)      # its own memset: the contents do not matter
                    L.call(entry, ops.ptr(img), half_elems, ops.ptr(z), half_z, ops.ptr(scratch), ops.ptr(out.t), sp, ops.stream())
                else:
                    L.call(entry, ops.ptr(img), half_elems, ops.ptr(z), half_z, ops.ptr(acc), ops.ptr(out.t), c.weight, sp, ops.stream())
                L.call("sp_div_loss_bwd", ops.ptr(img), half_elems, ops.ptr(out.t), ops.ptr(gout), ops.ptr(dimg.t), sp, ops.stream())
                assert P.compare(c, P.Case(out=out.host(c.what).reshape(2), dimg=dimg.host(c.what))) == 0.0
                assert acc.cpu().tolist() == [0.0, 0.0], "the shared accumulators are not back at zero"


# ------------------------------------------------------------------------------------------------------------------------------------
# the autograd functions
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_the_wrappers_hold_the_same_values(dt):
    ops.set_compute_dtype(dt)
    # head: x is a pitched view, the bias a leaf that wants its gradient
    c = built("dhead_case", dt, 5, 200, "mix")
    x = dev(c.x, dt, c.f + 8)[:, :c.f].requires_grad_(True)
    emb, wc = dev(c.emb, F32), dev(c.wc, F32)
    bc = dev(c.bc, F32).requires_grad_(True)
    pl_e = types.SimpleNamespace(fwd=emb.data_ptr(), rows=P.NUM_CLASSES, cols=c.f)
    pl_c = types.SimpleNamespace(fwd=wc.data_ptr(), rows=1, cols=c.f)
    pred = ops._DHeadFn.apply(x, None, None, bc, c.cls.to(DEV), pl_e, pl_c)
    pred.backward(dev(c.dpred, F32))
    assert P.compare(c, P.Case(pred=pred.detach().cpu(), dx=x.grad.cpu(), dbc=bc.grad.cpu())) == 0.0

    for n in (51203, (1 << 18) + 5, 1 << 20):
        c = built("sqerr_case", n, 1.0)
        p = c.p.float().to(DEV).requires_grad_(True)
        loss = ops.sqerr_loss(p, 1.0)
        loss.backward(torch.tensor(c.gout, device=DEV))
        assert P.compare(c, P.Case(loss=loss.detach().cpu().reshape(1), dp=p.grad.cpu())) <= 1.0

    shapes, weight, masks = REC_MULTI[1]
    c = built("rec_case", dt, tuple(shapes), weight, masks)
    fakes, reals, ms = [], [], []
    for lv in c.levels:
        if lv.four:
            fakes.append(dev(lv.fake, dt).permute(0, 3, 1, 2).requires_grad_(True))
            reals.append(dev(lv.real, dt).permute(0, 3, 1, 2).contiguous())              # NCHW memory: converted by the wrapper
            ms.append(dev(lv.mask, F32).unsqueeze(1))
        else:
            k = lv.shape[1]
            fakes.append(dev(lv.fake, dt, k + 5)[:, :k].requires_grad_(True))
            reals.append(dev(lv.real, dt, k + 3)[:, :k])
            ms.append(dev(lv.mask, F32))
    loss = ops.semantic_reconstruction_loss(reals, fakes, ms, c.weight)
    loss.backward(torch.tensor([c.gout], device=DEV))
    got = P.Case(loss=loss.detach().cpu().reshape(1))
    for i, (lv, f) in enumerate(zip(c.levels, fakes)):
        got["dfake%d" % i] = (f.grad.permute(0, 2, 3, 1) if lv.four else f.grad).contiguous().cpu()
    assert P.compare(c, got) <= 1.0
    assert float(ops._loss_acc(torch.device(DEV, torch.cuda.current_device())).abs().sum()) == 0.0

    c = built("div_case", dt, 1000, 128, 0.25)
    img = dev(c.img, dt).view(2, 5, 25, 8).permute(0, 3, 1, 2).requires_grad_(True)
    loss = ops.diversity_loss(img, dev(c.z, F32), c.weight)
    loss.backward(torch.tensor(c.gout, device=DEV))
    want = c.checks["out"][1]
    assert float(loss.detach()) == float(want[0])
    assert P.compare(c, P.Case(dimg=img.grad.permute(0, 2, 3, 1).contiguous().cpu().reshape(2, -1))) == 0.0
    assert float(ops._loss_acc(torch.device(DEV, torch.cuda.current_device())).abs().sum()) == 0.0
