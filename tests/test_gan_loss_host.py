"""tests/gan_loss_restated.py checked against itself and against torch on the CPU (the pattern of tests/test_pool_loss_harness.py): the
restated losses and gradients against torch autograd expressions in float64, the restated LeCam state machine step by step, the operand
builders of the exact regimes against their own conditions, three planted defects that the comparisons of tests/test_gpu_gan_loss.py
must reject, and the two config parsers."""
import numpy as np
import pytest
import torch

import gan_loss_restated as R
from semantic_pyramid_for_image_generation_amd import config

F = np.float32


def _torch_terms(p, kind, role):
    if kind == "hinge":
        return -p if role == "g" else torch.relu(1.0 - p if role == "d_real" else 1.0 + p)
    return torch.nn.functional.softplus(p if role == "d_fake" else -p, threshold=200.0)      # (the default of 20 is itself an approximation)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("role", R.ROLES)
def test_restated_losses_and_gradients_match_torch_autograd_in_float64(kind, role):
    for n in (1, 5, 1025):
        p = (R.hinge_operands(n) if kind == "hinge" else R.logistic_operands(n)).astype(np.float64)
        if kind == "hinge":
            p = p + np.where(np.abs(p) == 1.0, 0.0, 0.125)            # off the integers, the kink values kept
        g = 0.75
        t = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        want = _torch_terms(t, kind, role).mean()
        want.backward()
        _, mean, _ = R.loss(p, kind, role)
        assert mean == pytest.approx(float(want.detach()), rel=1e-13, abs=1e-300)
        c = float(R.coefficient(g, n))
        got = R.grad(p, kind, role, g)
        np.testing.assert_allclose(got, c * n * t.grad.numpy(), rtol=1e-12, atol=0.0)
        assert np.isfinite(got).all() and np.isfinite(mean)


def test_a_nan_prediction_is_a_nan_loss_and_a_nan_gradient_at_that_element():
    for kind in R.KINDS:
        for role in R.ROLES:
            p = R.logistic_operands(1025)
            p[77] = np.nan
            value, _, _ = R.loss(p, kind, role)
            dp = R.grad(p, kind, role, 1.0)
            assert np.isnan(value) and np.isnan(dp[77]) and np.isfinite(np.delete(dp, 77)).all()


def test_lecam_state_machine_step_by_step():
    pr, pf = np.array([1.0, 2.0, 3.0, 2.0], dtype=F), np.array([-1.0, 0.0, -1.0, 0.0], dtype=F)         # means 2 and -0.5
    m = R.LeCam(weight=2.0, decay=0.5, start=2)
    assert m.words() == [0] * 8
    for k in range(2):                                                 # tracking: plain assignment, inactive, reg exactly 0
        reg, _ = m.forward(pr * (k + 1), pf * (k + 1))
        assert (float(m.a_real), float(m.a_fake), int(m.updates), int(m.active), float(reg)) == (2.0 * (k + 1), -0.5 * (k + 1), k + 1, 0, 0.0)
        assert all(not d.any() for d in m.backward(pr, pf, 1.0))
    reg, exact = m.forward(pr, pf)                                     # the EMA: 0.5 * 4 + 0.5 * 2 = 3, 0.5 * -1 + 0.5 * -0.5 = -0.75
    assert (float(m.a_real), float(m.a_fake), int(m.updates), int(m.active)) == (3.0, -0.75, 3, 1)
    want = 2.0 * (np.sum((pr.astype(np.float64) + 0.75) ** 2) + np.sum((3.0 - pf.astype(np.float64)) ** 2)) / 4
    assert float(reg) == want == exact
    dr, df = m.backward(pr, pf, 0.5)                                   # c = 0.5 * 2 * (2 / 4) = 0.5
    assert dr.tolist() == (0.5 * (pr + 0.75)).tolist() and df.tolist() == (-0.5 * (3.0 - pf)).tolist()
    before = m.words()
    for bad in (np.nan, np.inf):                                       # a non-finite mean: anchors and count stay, the means are stored
        broken = pr.copy()
        broken[1] = bad
        m.forward(broken, pf)
        after = m.words()
        assert after[:3] == before[:3] and after[3] == 1 and after[5] == before[5] and not np.isfinite(m.m_real)
    m.updates = np.int32(R.INT_MAX - 1)
    m.forward(pr, pf)
    assert int(m.updates) == R.INT_MAX
    m.forward(pr, pf)
    assert int(m.updates) == R.INT_MAX and int(m.active) == 1      # saturated
    r = R.LeCam(weight=1.0, decay=0.5, start=0, rectified=True)       # active from the first call on; the rectifier cuts negative differences
    reg, _ = r.forward(pr, pf)
    assert (float(r.a_real), float(r.a_fake), int(r.active)) == (1.0, -0.25, 1)
    assert float(reg) == (np.sum((pr.astype(np.float64) + 0.25) ** 2) + np.sum(np.maximum(1.0 - pf.astype(np.float64), 0.0) ** 2)) / 4
    assert (r.backward(pr, -pf * 4, 1.0)[1] == 0.0).sum() == 2         # a_real - p_fake <= 0 where p_fake is 4: no gradient there


def test_the_operand_builders_meet_their_conditions():
    for n in R.SIZES:
        p = R.hinge_operands(n)
        for role in R.ROLES:
            t = R.terms(p, "hinge", role)
            assert np.all(t == np.round(t)) and np.abs(np.cumsum(np.abs(t))).max() < 2 ** 24
            assert float(R.hinge_exact_loss(p, role)) == pytest.approx(float(t.mean()), rel=2.0 ** -24)
        q = R.logistic_operands(n)
        assert q.dtype == F and np.isfinite(R.terms(q, "logistic", "d_real")).all()
    for n in (2, 4, 64, 512):
        for start in (0, 2):
            for rectified in (False, True):
                pr, pf = R.lecam_exact_operands(n)
                m = R.LeCam(weight=0.5, decay=0.5, start=start, rectified=rectified)
                for _ in range(start + 3):
                    reg, exact = m.forward(pr, pf)
                    assert float(reg) == exact                                        # no rounding anywhere
                    for a in (m.a_real, m.a_fake):
                        assert float(a) * 32 == round(float(a) * 32)
                    for d in m.backward(pr, pf, 2.0):
                        assert np.array_equal(d.astype(F).astype(np.float64), d)
                assert int(m.updates) == start + 3 and int(m.active) == 1 and float(reg) > 0
    with pytest.raises(AssertionError):
        R.lecam_exact_operands(768)


def test_planted_defects_are_rejected():
    # a dropped tail element: the exact hinge loss changes, and the general-regime LeCam mean leaves its bound
    for n in (3, 5, 1025, 16385):
        p = R.hinge_operands(n)
        for role in ("d_real", "g"):
            assert float(R.loss(p, "hinge", role, drop_tail=True)[0]) != float(R.hinge_exact_loss(p, role))
        pr, pf = R.lecam_general_operands(n)
        good, bad = R.LeCam(0.25, 0.99, 0), R.LeCam(0.25, 0.99, 0)
        good.forward(pr, pf)
        bad.forward(pr, pf, drop_tail=True)
        assert abs(float(bad.m_real) - float(good.m_real)) > R.lecam_mean_bound(pr, good.m_real, aligned=False)
    # an FMA-contracted EMA: one rounding fewer shows in the anchors' bits for these means
    plain, fused = R.LeCam(1.0, 0.99, 0), R.LeCam(1.0, 0.99, 0)
    differ = 0
    for i in range(8):
        pr, pf = R.lecam_general_operands(1025, seed=i)
        plain.forward(pr, pf)
        fused.forward(pr, pf, fma=True)
        differ += plain.words()[:2] != fused.words()[:2]
        fused.a_real, fused.a_fake = plain.a_real, plain.a_fake
    assert differ >= 1
    # a kink that counts <= instead of <: a gradient where the hinge's argument is exactly 0
    p = R.hinge_operands(1025)
    for role in ("d_real", "d_fake"):
        assert (R.grad(p, "hinge", role, 1.0) != R.grad(p, "hinge", role, 1.0, kink_le=True)).sum() == (p == (1.0 if role == "d_real" else -1.0)).sum() > 0


def test_bounds_are_what_the_docstring_derives():
    assert R.chain(51200, True) == 9 and R.chain(51200, False) == 18 and R.chain(5, True) == 6
    assert R.gamma(10) == pytest.approx(10 * R.U, rel=1e-6) and R.ulp(1.0) == 2.0 ** -23 and R.ulp(0.0) == 2.0 ** -149
    p = R.logistic_operands(1025)
    assert R.logistic_loss_bound(p, "logistic", "g") < 1e-4 and (R.logistic_grad_bound(p, "logistic", "g", 1.0) >= R.TINY).all()


def test_parse_gan_loss():
    assert [config.parse_gan_loss(t) for t in (None, "", "  ", "lsgan", "hinge", " logistic ")] == ["", "", "", "lsgan", "hinge", "logistic"]
    for bad in ("Hinge", "wgan", "hinge,logistic", 1, True, ["hinge"]):
        with pytest.raises(ValueError):
            config.parse_gan_loss(bad)
    assert config.Config().gan_loss == "" and config.Config().lecam == ""


def test_parse_lecam():
    assert [config.parse_lecam(t) for t in (None, "", " ", 0, 0.0, "0", "0:0.5")] == [None] * 7
    assert config.parse_lecam(0.3) == (0.3, 0.99, 1000) and config.parse_lecam(1) == (1.0, 0.99, 1000)
    assert config.parse_lecam("0.3") == (0.3, 0.99, 1000) and config.parse_lecam(" 0.3 : 0.5 ") == (0.3, 0.5, 1000)
    assert config.parse_lecam("1e-2:0:0") == (0.01, 0.0, 0) and config.parse_lecam("0.3:0.999:250") == (0.3, 0.999, 250)
    for bad in ("abc", "0.3:", ":0.5", "0.3::5", "0.3:1.0", "0.3:1", "0.3:-0.1", "0.3:0.9:1.5", "0.3:0.9:-1", "0.3:0.9:10:1", "nan", "inf",
                "-1", "0.3:nan", "0.3:0.9:x", "0.3:0.9:4294967296", -0.5, float("nan"), float("inf"), True, [0.3], (0.3, 0.9)):
        with pytest.raises(ValueError):
            config.parse_lecam(bad)
