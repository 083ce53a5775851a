"""The hinge / logistic losses and the LeCam regularizer through the C ABI (csrc/losses.hip: sp_gan_loss_fwd / _bwd, sp_lecam_fwd / _bwd;
DESIGN.md section 18) against tests/gan_loss_restated.py, which holds the definitions, the operands of the exact regimes and the
derivation of every bound (checked against itself on the CPU by tests/test_gan_loss_host.py).

Every size runs with the predictions 16-byte aligned and one float off alignment (the launchers have ONE route at every size: no
boundary to add to the sizes).  Every output lies between sentinel pads, which must survive."""
import ctypes

import numpy as np
import pytest
import torch

import gan_loss_restated as R
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
PAD, SENTINEL = 64, -1536.0
SP_ERR_INVALID = -1
KIND, ROLE = ops.GAN_LOSS_KINDS, ops.GAN_LOSS_ROLES
ALIGN_IDS = ["aligned", "misaligned"]


class Out:
    """[PAD sentinel][n values, sentinel][PAD sentinel] on the device, the body 16-byte aligned or one float off."""

    def __init__(self, n, misaligned=False):
        self.n, self.off = n, PAD + (1 if misaligned else 0)
        self.buf = torch.full((2 * PAD + n + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off)
        assert (self.ptr.value % 16 != 0) == misaligned

    def host(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert np.all(b[:self.off] == F(SENTINEL)) and np.all(b[self.off + self.n:] == F(SENTINEL)), "a write outside the output"
        return b[self.off:self.off + self.n].copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def place(values, misaligned):
    """The fp32 operand on the device at an aligned or a one-float-off address; (keep-alive tensor, pointer)."""
    values = np.asarray(values, dtype=F)
    base = torch.zeros(values.size + 8, dtype=torch.float32, device=DEV)
    off = 1 if misaligned else 0
    base[off:off + values.size] = torch.from_numpy(values).to(DEV)
    p = ctypes.c_void_p(base.data_ptr() + 4 * off)
    assert (p.value % 16 != 0) == misaligned
    return base, p


def f32dev(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def gan_run(p, kind, role, g, misaligned):
    keep, ptr = place(p, misaligned)
    loss, dp = Out(1), Out(p.size, misaligned)
    L.call("sp_gan_loss_fwd", ptr, p.size, KIND[kind], ROLE[role], loss.ptr, ops.stream())
    L.call("sp_gan_loss_bwd", ptr, p.size, KIND[kind], ROLE[role], ops.ptr(f32dev(g)), dp.ptr, ops.stream())
    return loss.host()[0], dp.host()


@pytest.mark.parametrize("misaligned", [False, True], ids=ALIGN_IDS)
@pytest.mark.parametrize("n", R.SIZES)
def test_hinge_is_the_nearest_float_and_its_gradient_bit_identical(n, misaligned):
    p = R.hinge_operands(n)
    for role in R.ROLES:
        for g in (1.0, 0.375):
            got, dp = gan_run(p, "hinge", role, g, misaligned)
            want = R.hinge_exact_loss(p, role)
            print("hinge", role, n, float(got), float(want))
            assert got.tobytes() == F(want).tobytes(), (role, float(got), float(want))
            assert dp.tobytes() == R.grad(p, "hinge", role, g).astype(F).tobytes(), role


@pytest.mark.parametrize("misaligned", [False, True], ids=ALIGN_IDS)
@pytest.mark.parametrize("n", R.SIZES)
def test_logistic_is_within_the_bound_of_the_float64_restatement(n, misaligned):
    p = R.logistic_operands(n)
    worst = [0.0, 0.0]
    for role in R.ROLES:
        g = 2.0
        got, dp = gan_run(p, "logistic", role, g, misaligned)
        _, exact, _ = R.loss(p, "logistic", role)
        bound = R.logistic_loss_bound(p, "logistic", role)
        dexact, dbound = R.grad(p, "logistic", role, g), R.logistic_grad_bound(p, "logistic", role, g)
        assert np.isfinite(got) and np.isfinite(dp).all()
        worst[0] = max(worst[0], abs(float(got) - exact) / bound)
        worst[1] = max(worst[1], float((np.abs(dp.astype(np.float64) - dexact) / dbound).max()))
    print("logistic n %d: worst error / bound: loss %.3f gradient %.3f" % (n, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_one_nan_among_1025_is_a_nan_loss_and_a_nan_gradient_there_only(kind):
    for role in R.ROLES:
        for misaligned in (False, True):
            p = R.logistic_operands(1025) if kind == "logistic" else R.hinge_operands(1025)
            p[600] = np.nan
            got, dp = gan_run(p, kind, role, 1.0, misaligned)
            assert np.isnan(got), (role, got)
            assert np.isnan(dp[600]) and np.isfinite(np.delete(dp, 600)).all(), role


def lecam_run(state, pr, pf, m, g, misaligned):
    """One forward and one backward launch on `state` with the restated machine's settings: (words, reg, dp_real, dp_fake)."""
    keep_r, ptr_r = place(pr, misaligned)
    keep_f, ptr_f = place(pf, misaligned)
    reg, dr, df = Out(1), Out(pr.size, misaligned), Out(pr.size, misaligned)
    L.call("sp_lecam_fwd", ptr_r, ptr_f, pr.size, float(m.weight), float(m.decay), m.start, int(m.rectified), ops.ptr(state), reg.ptr, ops.stream())
    L.call("sp_lecam_bwd", ptr_r, ptr_f, pr.size, float(m.weight), int(m.rectified), ops.ptr(state), ops.ptr(f32dev(g)), dr.ptr, df.ptr, ops.stream())
    return state.cpu().tolist(), reg.host()[0], dr.host(), df.host()


@pytest.mark.parametrize("rectified", [False, True], ids=["plain", "rectified"])
@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("n", [2, 4, 64, 512])
def test_lecam_exact_regime_is_bit_identical(n, start, rectified):
    for misaligned in (False, True):
        pr, pf = R.lecam_exact_operands(n)
        m = R.LeCam(weight=0.5, decay=0.5, start=start, rectified=rectified)
        state = torch.zeros(8, dtype=torch.int32, device=DEV)
        for step in range(start + 3):
            want_reg, _ = m.forward(pr, pf)
            want_dr, want_df = m.backward(pr, pf, 2.0)
            words, reg, dr, df = lecam_run(state, pr, pf, m, 2.0, misaligned)
            assert words == m.words(), (step, words, m.words())
            assert reg.tobytes() == F(want_reg).tobytes(), (step, float(reg), float(want_reg))
            assert dr.tobytes() == want_dr.astype(F).tobytes() and df.tobytes() == want_df.astype(F).tobytes(), step
        assert int(m.active) == 1 and float(reg) > 0


@pytest.mark.parametrize("misaligned", [False, True], ids=ALIGN_IDS)
@pytest.mark.parametrize("n", R.SIZES)
def test_lecam_general_regime_is_within_the_derived_bounds(n, misaligned):
    aligned = not misaligned
    m = R.LeCam(weight=0.3, decay=0.99, start=1, rectified=(n % 2 == 1))
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    worst = {"mean": 0.0, "reg": 0.0, "grad": 0.0}
    for step in range(3):
        pr, pf = R.lecam_general_operands(n, seed=step)
        words, reg, dr, df = lecam_run(state, pr, pf, m, 1.5, misaligned)
        dev_means = np.array(words[4:6], dtype=np.int32).view(F)
        for p, got in ((pr, dev_means[0]), (pf, dev_means[1])):
            exact = float(np.asarray(p, dtype=np.float64).mean())
            worst["mean"] = max(worst["mean"], abs(float(got) - exact) / R.lecam_mean_bound(p, got, aligned))
        _, exact_reg = m.forward(pr, pf, means=dev_means)            # the anchors GIVEN the device's means: bit for bit
        assert words == m.words(), (step, words, m.words())
        worst["reg"] = max(worst["reg"], abs(float(reg) - exact_reg) / R.lecam_reg_bound(exact_reg, n, aligned) if step >= 1 else float(reg != 0.0))
        for got, exact in zip((dr, df), m.backward(pr, pf, 1.5)):
            bound = R.lecam_grad_bound(exact)
            err = np.abs(got.astype(np.float64) - exact)
            worst["grad"] = max(worst["grad"], float(np.where(err == 0, 0.0, err / np.where(bound == 0, R.TINY, bound)).max()))
        if step == 0:                                                # below `start`: tracking only
            assert not dr.any() and not df.any() and reg == 0.0
        else:
            assert words[3] == 1 and (n < 4 or (reg > 0 and dr.any() and df.any()))
    print("lecam n %d: worst error / bound: %s" % (n, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert all(w <= 1.0 for w in worst.values()), worst


def test_state_behaviour_non_finite_means_refusals_and_determinism():
    n = 1025
    pr, pf = R.lecam_general_operands(n)
    m = R.LeCam(weight=0.3, decay=0.99, start=1)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    for _ in range(2):
        lecam_run(state, pr, pf, m, 1.0, False)
    before = state.cpu().tolist()
    assert before[2] == 2 and before[3] == 1
    for bad in (np.nan, np.inf, -np.inf):                              # a non-finite mean leaves the anchors and `updates` untouched
        broken = pf.copy()
        broken[511] = bad
        words, _, _, _ = lecam_run(state, pr, broken, m, 1.0, False)
        assert words[:3] == before[:3] and words[3] == 1 and words[4] == before[4], (bad, words, before)
        assert not np.isfinite(np.array(words[5:6], dtype=np.int32).view(F)[0])
    lecam_run(state, pr, pf, m, 1.0, False)
    assert state.cpu().tolist()[2] == 3
    # refusals: nothing launched, state and outputs untouched
    before = state.cpu().tolist()
    keep_r, ptr_r = place(pr, False)
    keep_f, ptr_f = place(pf, False)
    reg, dr, df, loss = Out(1), Out(n), Out(n), Out(1)
    lib = L.lib()
    s = ops.stream()
    nan, inf = float("nan"), float("inf")
    for weight, decay, start, numel in ((-0.5, 0.9, 0, n), (nan, 0.9, 0, n), (inf, 0.9, 0, n), (0.3, 1.0, 0, n), (0.3, -0.1, 0, n), (0.3, nan, 0, n),
                                        (0.3, 0.9, -1, n), (0.3, 0.9, 0, 0), (0.3, 0.9, 0, (1 << 24) + 1)):
        assert lib.sp_lecam_fwd(ptr_r, ptr_f, numel, weight, decay, start, 0, ops.ptr(state), reg.ptr, s) == SP_ERR_INVALID, (weight, decay, start, numel)
    for weight, numel in ((-0.5, n), (nan, n), (0.3, 0), (0.3, (1 << 24) + 1)):
        assert lib.sp_lecam_bwd(ptr_r, ptr_f, numel, weight, 0, ops.ptr(state), ops.ptr(f32dev(1.0)), dr.ptr, df.ptr, s) == SP_ERR_INVALID
    assert lib.sp_lecam_fwd(ptr_r, None, n, 0.3, 0.9, 0, 0, ops.ptr(state), reg.ptr, s) == SP_ERR_INVALID
    for kind, role, numel in ((2, 0, n), (-1, 0, n), (0, 3, n), (1, -1, n), (0, 0, 0), (1, 2, (1 << 24) + 1)):
        assert lib.sp_gan_loss_fwd(ptr_r, numel, kind, role, loss.ptr, s) == SP_ERR_INVALID, (kind, role, numel)
        assert lib.sp_gan_loss_bwd(ptr_r, numel, kind, role, ops.ptr(f32dev(1.0)), dr.ptr, s) == SP_ERR_INVALID, (kind, role, numel)
    assert b"numel" in lib.sp_last_error_string()
    assert state.cpu().tolist() == before and all(o.untouched() for o in (reg, dr, df, loss))
    # two identical runs: bit-identical outputs
    runs = []
    for _ in range(2):
        st = torch.zeros(8, dtype=torch.int32, device=DEV)
        rec = []
        for step in range(3):
            words, r, a, b = lecam_run(st, pr, pf, m, 1.0, step == 1)
            rec.append((words, r.tobytes(), a.tobytes(), b.tobytes()))
        for kind in R.KINDS:
            for role in R.ROLES:
                value, dp = gan_run(R.logistic_operands(51200), kind, role, 1.0, False)
                rec.append((value.tobytes(), dp.tobytes()))
        runs.append(rec)
    assert runs[0] == runs[1]


def test_the_autograd_wrappers_hold_the_same_values():
    p = R.hinge_operands(1025)
    for kind in R.KINDS:
        for role in R.ROLES:
            t = torch.from_numpy(p).to(DEV).requires_grad_(True)
            value = ops.gan_loss(t, kind, role)
            value.backward(torch.tensor(0.375, device=DEV))
            want, dp = gan_run(p, kind, role, 0.375, False)
            assert float(value) == float(want) and t.grad.cpu().numpy().tobytes() == dp.tobytes()
    with pytest.raises(L.SempyrError):
        ops.gan_loss(torch.zeros(4, device=DEV), "wgan", "g")
    pr, pf = R.lecam_exact_operands(64)
    lecam = ops.LeCam(DEV, weight=0.5, decay=0.5, start=1)
    m = R.LeCam(0.5, 0.5, 1)
    for step in range(3):
        a, b = torch.from_numpy(pr).to(DEV).requires_grad_(True), torch.from_numpy(pf).to(DEV).requires_grad_(True)
        reg = lecam(a.view(8, 8), b.view(8, 8))
        reg.backward(torch.tensor(2.0, device=DEV))
        want, _ = m.forward(pr, pf)
        dr, df = m.backward(pr, pf, 2.0)
        assert float(reg) == float(want) and lecam.state.cpu().tolist() == m.words()
        assert a.grad.cpu().numpy().tobytes() == dr.astype(F).tobytes() and b.grad.cpu().numpy().tobytes() == df.astype(F).tobytes()
    assert float(lecam.anchor_real) == float(m.a_real) and float(lecam.anchor_fake) == float(m.a_fake) and int(lecam.updates) == 3
    other = ops.LeCam(DEV, weight=1.0)
    ptr = other.state.data_ptr()
    other.load_state_dict(lecam.state_dict())
    assert other.state.data_ptr() == ptr and other.state.cpu().tolist() == m.words() and other.settings() == lecam.settings()
    with pytest.raises(L.SempyrError):
        lecam(torch.zeros(4, device=DEV), torch.zeros(5, device=DEV))
    for kw in ({"weight": -1.0}, {"weight": float("nan")}, {"weight": float("inf")}, {"weight": True}, {"weight": 1.0, "decay": 1.0},
               {"weight": 1.0, "decay": float("nan")}, {"weight": 1.0, "start": -1}, {"weight": 1.0, "start": 1.5}):
        with pytest.raises(L.SempyrError):
            ops.LeCam(DEV, **kw)
