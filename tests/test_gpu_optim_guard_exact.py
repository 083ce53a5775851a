"""The device-side guards of the fp16 mode (csrc/optim.hip) through the C ABI, every comparison exact: sp_check_finite,
sp_scale_f32 / sp_scale_f32_dev, sp_loss_scale_update and the skip path of sp_adam_multi_guarded.  Every buffer a kernel writes lies
between canaries.  (sp_ema_multi with the same flag: tests/test_gpu_ema.py.)"""
import ctypes

import numpy as np
import pytest
import torch

import exact_util as X
import sn_exact_util as S
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
CANARY, PAD = -1536.0, 64
SP_ERR_INVALID = -1
INF, NAN = float("inf"), float("nan")
CHECK_STRIDE = 2048 * 256 * 4 + 5            # the second trip of sp_check_finite's grid-stride loop: one float4 and a tail of one
SCALE_STRIDE = 4096 * 256 * 4 + 5            # ... and of sp_scale_f32's
_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("step_size", "<f4"), ("inv_sqrt_bc2", "<f4"),
                ("reserved", "<f4")])        # sp_adam_chunk (include/sempyr.h)


class Guarded:
    """[PAD canaries][n floats][PAD canaries] on the device; .t is the body (16-byte aligned), off: start it `off` floats later."""

    def __init__(self, body, off=0):
        self.n, self.off = body.numel(), off
        host = torch.full((PAD + off + self.n + PAD,), CANARY)
        host[PAD + off:PAD + off + self.n] = body.float()
        self.buf = host.to(DEV)
        self.t = self.buf[PAD + off:PAD + off + self.n]
        assert self.buf[PAD:].data_ptr() % 16 == 0

    def host(self, what=""):
        h = self.buf.cpu()
        edge = torch.cat((h[:PAD + self.off], h[PAD + self.off + self.n:]))
        assert bool((edge == CANARY).all()), (what, "a canary next to the buffer was overwritten")
        return h[PAD + self.off:PAD + self.off + self.n]


def finite_values(n, seed):
    """Finite fp32 values with +-3e38 and zeros among them, none subnormal."""
    g = X.gen(seed)
    x = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())).float()
    x[x.abs() < 1e-30] = 1.0
    x[::7] = 0.0
    x[1::11] = 3e38
    x[2::13] = -3e38
    return x


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_check_finite
# ------------------------------------------------------------------------------------------------------------------------------------
def positions(n, stride_at=None):
    pos = {"first": 0, "last": n - 1}
    if n >= 8:
        pos["body"] = (n // 4 // 2) * 4 + 1
    if n % 4 and n > 4:
        pos["tail"] = n - n % 4
    if stride_at is not None:
        pos["second trip"] = stride_at + 2
    return pos


@pytest.mark.parametrize("n", [1, 3, 8, 1029, CHECK_STRIDE], ids=str)
def test_check_finite_finds_one_bad_value_anywhere(n):
    """found starts at 0; a single +inf, -inf or NaN in the float4 body, the numel % 4 tail, the first and the last element and the
    second trip of the grid-stride loop sets it; +-3e38 and zeros leave it at 0; a found that starts at 1 stays 1 on clean input."""
    x = finite_values(n, n).to(DEV)
    assert x.data_ptr() % 16 == 0

    def found_after(start):
        f = Guarded(torch.tensor([start]))
        L.call("sp_check_finite", ops.ptr(x), n, ops.ptr(f.t), ops.stream())
        torch.cuda.synchronize()
        return float(f.host("found")[0])

    assert found_after(0.0) == 0.0
    assert found_after(1.0) == 1.0                            # the kernel never resets it
    for name, p in positions(n, 2048 * 256 * 4 if n == CHECK_STRIDE else None).items():
        keep = float(x[p])
        for bad in (INF, -INF, NAN):
            x[p] = bad
            assert found_after(0.0) == 1.0, (n, name, p, bad)
        x[p] = keep
    assert found_after(0.0) == 0.0


def test_check_finite_and_scale_refuse_a_misaligned_pointer():
    x = torch.zeros(64, device=DEV)
    f = Guarded(torch.zeros(1))
    lib = L.lib()
    off = ctypes.c_void_p(x.data_ptr() + 4)
    assert lib.sp_check_finite(off, 8, ops.ptr(f.t), ops.stream()) == SP_ERR_INVALID
    assert lib.sp_check_finite(ops.ptr(x), 0, ops.ptr(f.t), ops.stream()) == SP_ERR_INVALID
    assert lib.sp_check_finite(ops.ptr(x), 8, None, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_scale_f32(off, 8, 0.5, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_scale_f32_dev(off, 8, ops.ptr(f.t), ops.stream()) == SP_ERR_INVALID
    assert lib.sp_scale_f32_dev(ops.ptr(x), 8, None, ops.stream()) == SP_ERR_INVALID
    torch.cuda.synchronize()
    assert float(f.host("found")[0]) == 0.0 and float(x.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_scale_f32, sp_scale_f32_dev
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 8, 1029, SCALE_STRIDE], ids=str)
def test_scale_is_one_ieee_multiply(n):
    """x *= factor bit for bit against the CPU's fp32 product, factors 0.5 and 1/3, the canaries behind numel intact.  Inputs and
    results are kept out of the subnormal range (|x| in [1e-30, 3e38] or 0): what the device does with subnormals is not asked here."""
    x = finite_values(n, 3 * n + 1)
    for factor in (0.5, float(np.float32(1.0) / np.float32(3.0))):
        want = x * torch.tensor(factor, dtype=F32)
        assert not bool(((want != 0) & (want.abs() < 1.2e-38)).any())
        g = Guarded(x)
        L.call("sp_scale_f32", ops.ptr(g.t), n, factor, ops.stream())
        torch.cuda.synchronize()
        S.assert_exact(g.host("sp_scale_f32"), want, "sp_scale_f32 n %d factor %r" % (n, factor))
        # the _dev form reads the factor when the kernel runs: the device value changes between two calls
        g, fac = Guarded(x), Guarded(torch.tensor([factor]))
        L.call("sp_scale_f32_dev", ops.ptr(g.t), n, ops.ptr(fac.t), ops.stream())
        fac.t.fill_(0.25)
        L.call("sp_scale_f32_dev", ops.ptr(g.t), n, ops.ptr(fac.t), ops.stream())
        torch.cuda.synchronize()
        S.assert_exact(g.host("sp_scale_f32_dev"), want * torch.tensor(0.25), "sp_scale_f32_dev n %d factor %r then 0.25" % (n, factor))
        assert float(fac.host("factor")[0]) == 0.25


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_loss_scale_update
# ------------------------------------------------------------------------------------------------------------------------------------
SEQUENCES = {
    "growth to the 2^24 clamp, interval 1": ([2.0 ** 21, 2.0 ** -21, 0, 0, 0], 2.0, 0.5, 1, [0] * 6),
    "growth every third clean step": ([4.0, 0.25, 0, 0, 0], 2.0, 0.5, 3, [0] * 10),
    "backoff to the clamp at 1, skips counted": ([8.0, 0.125, 2, 0, 0], 2.0, 0.5, 3, [1] * 6),
    "found resets the clean count": ([16.0, 0.0625, 0, 0, 3], 4.0, 0.25, 3, [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_loss_scale_update_follows_the_restated_state_machine(name):
    st0, growth, backoff, interval, found = SEQUENCES[name]
    st = Guarded(torch.tensor(st0, dtype=F32))
    want = [float(v) for v in st0]
    for step, f in enumerate(found):
        st.t[3] = float(f)
        want[3] = float(f)
        L.call("sp_loss_scale_update", ops.ptr(st.t), growth, backoff, interval, ops.stream())
        torch.cuda.synchronize()
        want = S.loss_scale_step(want, growth, backoff, interval)
        got = st.host(name).tolist()
        assert got == want, (name, step, got, want)
        assert got[3] == 0.0 and got[1] == 1.0 / got[0]        # found consumed; 1 / scale exact for power-of-two scales
    assert 1.0 <= want[0] <= 2.0 ** 24


def test_loss_scale_update_refuses_bad_arguments():
    st = Guarded(torch.tensor([4.0, 0.25, 0, 1, 0]))
    lib, p = L.lib(), ops.ptr(st.t)
    for args in ((None, 2.0, 0.5, 1), (p, 0.5, 0.5, 1), (p, 2.0, 0.0, 1), (p, 2.0, 1.5, 1), (p, 2.0, 0.5, 0), (p, NAN, 0.5, 1), (p, 2.0, NAN, 1)):
        assert lib.sp_loss_scale_update(*args, ops.stream()) == SP_ERR_INVALID, args
    torch.cuda.synchronize()
    assert st.host("state").tolist() == [4.0, 0.25, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_adam_multi_guarded
# ------------------------------------------------------------------------------------------------------------------------------------
def adam_state(sizes_offs, seed):
    g = X.gen(seed)
    out = []
    for n, off in sizes_offs:
        p, gr, m = (torch.randn(n, generator=g) for _ in range(3))
        v = torch.rand(n, generator=g) * 1e-2
        out.append([Guarded(p, off), Guarded(gr, off), Guarded(m, off), Guarded(v, off)])
    return out


def chunk_table(state):
    tab = np.zeros(len(state), dtype=_DT)
    for i, (p, g, m, v) in enumerate(state):
        tab[i] = (p.t.data_ptr(), g.t.data_ptr(), m.t.data_ptr(), v.t.data_ptr(), p.n, 1e-3, 1.5, 0.0)
    return torch.from_numpy(tab.view(np.uint8)).to(DEV)


def test_adam_guarded_skips_everything_or_equals_the_plain_step():
    """*skip != 0: p, m and v of every chunk - an aligned one, a misaligned one, one of 65536 + 1 elements - keep their bits.
    *skip == 0: they equal sp_adam_multi on a copy bit for bit."""
    shapes = [(1000, 0), (1031, 1), (65536 + 1, 0), (3, 3)]
    hyper = (0.5, 0.999, 1e-8, 0.01)
    for skip_value in (1.0, -0.0, 0.0):
        a, b = adam_state(shapes, 9), adam_state(shapes, 9)
        before = [[t.host().clone() for t in ch] for ch in a]
        ta, tb = chunk_table(a), chunk_table(b)
        skip = Guarded(torch.tensor([skip_value]))
        L.call("sp_adam_multi_guarded", ops.ptr(ta), len(a), *hyper, ops.ptr(skip.t), ops.stream())
        L.call("sp_adam_multi", ops.ptr(tb), len(b), *hyper, ops.stream())
        torch.cuda.synchronize()
        assert float(skip.host("skip")[0]) == skip_value
        for i, (ch_a, ch_b, ch_0) in enumerate(zip(a, b, before)):
            for name, ga, gb, t0 in zip("pgmv", ch_a, ch_b, ch_0):
                want = t0 if skip_value == 1.0 or name == "g" else gb.host((i, name))
                S.assert_exact(ga.host((i, name)), want, "chunk %d %s with *skip = %r" % (i, name, skip_value))
                if name != "g":
                    assert not torch.equal(gb.host(), t0), "the plain step changed nothing"
    assert L.lib().sp_adam_multi_guarded(None, 1, *hyper, None, ops.stream()) == SP_ERR_INVALID
