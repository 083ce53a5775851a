"""The hinge / logistic adversarial losses and the LeCam regularizer (csrc/losses.hip: sp_gan_loss_*, sp_lecam_*)
restated for the tests: the definitions in numpy float64 / float32, the operand builders of the exact regimes with their conditions, the
derived bounds, and one training step on the oracle with the restated losses in place of LSGAN.  Not a test module; nothing here runs on
a GPU.

THE DEFINITIONS (include/sempyr.h).  p: n fp32 predictions, g: the seed, u = 2^-24.
    kind      D, real          D, fake          G
    hinge     max(0, 1 - p)    max(0, 1 + p)    -p
    logistic  softplus(-p)     softplus(p)      softplus(-p)             softplus(x) = max(x, 0) + log1p(exp(-|x|))
    loss = (float)(sum f(p) / n): the sum and the quotient in double, rounded once.
    dp   = c * f'(p), c = fl32(g / n).  Hinge: -c / +c where the argument of max is > 0 strictly, 0 where it is <= 0; -c for G.
           Logistic: -/+ c * sigmoid(-/+ p).  A NaN prediction: NaN loss, NaN dp at that element.
LeCam, state {a_real, a_fake, updates, active, m_real, m_fake, 0, 0}:
    m = (float)(sum(p) / n) for both inputs;  k = updates;  both means finite: k < start: a = m, else a = fl(fl(decay * a) + fl(fl(1 - decay) * m)),
    updates = min(k + 1, 2^31 - 1);  active = (k >= start);  reg = active ? (float)(weight * (S_r + S_f) / n) : 0 with the UPDATED anchors,
    S_r = sum h(p_real - a_fake)^2, S_f = sum h(a_real - p_fake)^2, h(x) = x or max(x, 0).
    dp_real = active ? c * h(p_real - a_fake) : 0, dp_fake = active ? -c * h(a_real - p_fake) : 0, c = fl(fl(g * weight) * fl(2 / n)).

THE BOUNDS.  The forward kernels are one block of 1024 threads.  A thread adds its terms into FOUR fp32 partial sums - 16-byte loads:
(t0 + t1) + (t2 + t3) of one load added to a partial, a partial serving every fourth load of the thread; 4-byte loads (a pointer that is
not 16-byte aligned): one term per addition - and everything behind the partials is double.  The longest chain of fp32 additions a term
passes through is therefore
    chain(n, aligned) = n // 16384 + 6   (aligned: floor(n / 4 / 4096) full trips + at most 3 single trips + 1 tail + the tree's 2)
    chain(n, misaligned) = n // 4096 + 6 (floor(n / 4096) full trips + at most 3 single trips; the same constant, for one formula)
and a sum of terms t_i computed with `e` rounded operations each differs from the exact sum by at most gamma(chain + e) * sum|t_i|,
gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 and section 4.2).  The double part adds
2^-53-sized terms, which the "+ 1" in every k below covers.  The final rounding to fp32 adds half an ulp of the result.
    LeCam means           e = 0:  |m - exact| <= gamma(chain + 1) * mean|p| + ulp(m) / 2
    LeCam regularizer     e = 3 (the difference, the square - a fused multiply-add only removes a rounding):
                          |reg - exact| <= gamma(chain + 4) * exact + ulp(reg) / 2       (every term is >= 0; exact: on the device's anchors)
    LeCam gradients       elementwise, the difference and the product with c:  |dp - exact| <= gamma(2) * |exact|
    anchors               bit for bit GIVEN the means: the three-rounding update is fully specified (the test feeds it the device's means).
    hinge                 exact: integers, every partial sum below 2^24, the loss the nearest float of the exact quotient (the double
                          quotient of two integers below 2^26 is never within 2^-53 of a float's rounding boundary unless it is on it).
    logistic loss         the issue's bound: (EPS + 2u) * mean|f| + ulp(loss) / 2, EPS = 2^-18 the project's allowance for the device's
                          expf / logf (tests/attention_exact_util.py)
    logistic gradient     |dp - exact| <= (EPS + 3u) * |exact| + TINY * max(1, |c|), exact = c * sigmoid in float64.  TINY = 2^-126, the
                          smallest normal fp32: below it the format holds no relative precision (c * sigmoid(-88) and sigmoid(-104) are
                          subnormal or zero in fp32), so a relative bound alone cannot be met by any fp32 result there."""
import math
from fractions import Fraction

import numpy as np
import torch

from oracle import sempyr_oracle as O

F = np.float32
U = 2.0 ** -24
EPS = 2.0 ** -18
TINY = 2.0 ** -126
KINDS = ("hinge", "logistic")
ROLES = ("d_real", "d_fake", "g")
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 16383, 16384, 16385, 51200)
INT_MAX = 2 ** 31 - 1


def gamma(k):
    return k * U / (1.0 - k * U)


def chain(n, aligned):
    return n // (16384 if aligned else 4096) + 6


def ulp(x):
    """The spacing of fp32 at |x| (of the smallest normal below it)."""
    return float(np.spacing(F(max(abs(float(x)), TINY))))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the losses
# ----------------------------------------------------------------------------------------------------------------------------------------
def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def terms(p, kind, role):
    """f(p) per element in float64 (NaN where p is NaN)."""
    p = np.asarray(p, dtype=np.float64)
    if kind == "hinge":
        if role == "g":
            return -p
        t = 1.0 - p if role == "d_real" else 1.0 + p
        return np.where(t > 0, t, np.where(t <= 0, 0.0, t))
    return _softplus(p if role == "d_fake" else -p)


def loss(p, kind, role, drop_tail=False):
    """(the fp32 loss, the float64 mean, the float64 mean of |f|).  drop_tail: a planted defect - the last element is not summed."""
    t = terms(p, kind, role)
    n = t.size
    if drop_tail:
        t = t[:-1]
    s = math.fsum(t.tolist()) if np.isfinite(t).all() else float(np.sum(t))
    return F(s / n), s / n, (math.fsum(np.abs(t).tolist()) / n if np.isfinite(t).all() else float("nan"))


def coefficient(g, n):
    return F(F(g) / F(n))


def grad(p, kind, role, g, kink_le=False):
    """dp per element in float64, c = fl32(g / n).  kink_le: a planted defect - the hinge's gradient is on where the argument is >= 0."""
    p = np.asarray(p, dtype=np.float64)
    c = float(coefficient(g, p.size))
    if kind == "hinge":
        if role == "g":
            return np.where(np.isnan(p), p, -c)
        t = 1.0 - p if role == "d_real" else 1.0 + p
        on = (t >= 0) if kink_le else (t > 0)
        return np.where(on, -c if role == "d_real" else c, np.where(np.isnan(t), t, 0.0))
    return c * _sigmoid(p) if role == "d_fake" else -c * _sigmoid(-p)


def hinge_operands(n, seed=0):
    """n integers in [-3, 3] as fp32, the kink values -1 and +1 among them wherever n allows, the last element never 0 (a dropped tail
    shows).  Every partial sum of every term is an integer of magnitude <= 4 n <= 2^24."""
    rng = np.random.default_rng(1000 + seed + n)
    p = rng.integers(-3, 4, size=n).astype(F)
    fixed = [1.0, -1.0, 3.0, -3.0, 0.0]
    for i, v in enumerate(fixed[:max(0, n - 1)]):
        p[i] = v
    p[-1] = -2.0 if n > 1 else 2.0
    assert 4 * n <= 2 ** 24 and np.all(p == np.round(p)) and np.abs(p).max() <= 3
    assert n < 3 or (np.any(p == 1.0) and np.any(p == -1.0))
    return p


def nearest_float(num, den):
    """The fp32 nearest to the exact quotient of two integers."""
    q = Fraction(int(num), int(den))
    f = F(float(q))                                        # (correctly rounded to double, then to float: module docstring)
    lo, hi = Fraction(float(np.nextafter(f, F(-np.inf)))), Fraction(float(np.nextafter(f, F(np.inf))))
    assert abs(q - Fraction(float(f))) <= min(abs(q - lo), abs(q - hi))
    return f


def hinge_exact_loss(p, role):
    t = terms(p, "hinge", role)
    assert np.all(t == np.round(t))
    return nearest_float(int(t.sum()), t.size)


def logistic_operands(n, seed=0):
    """n values in [-30, 30] as fp32 with +-88 and +-104 planted wherever n allows: expf(88.x) overflows, expf(-104) underflows."""
    rng = np.random.default_rng(2000 + seed + n)
    p = rng.uniform(-30.0, 30.0, size=n).astype(F)
    for i, v in enumerate([88.0, -88.0, 104.0, -104.0][:max(0, n - 1)]):
        p[(i * 7919) % n if n > 8 else i] = v
    assert np.abs(p).max() <= 104 and (n < 5 or sorted(set(p[np.abs(p) > 30].tolist())) == [-104.0, -88.0, 88.0, 104.0])
    return p


def logistic_loss_bound(p, kind, role):
    value, _, mean_abs = loss(p, kind, role)
    return (EPS + 2 * U) * mean_abs + ulp(value) / 2


def logistic_grad_bound(p, kind, role, g):
    exact = grad(p, kind, role, g)
    return (EPS + 3 * U) * np.abs(exact) + TINY * max(1.0, abs(float(coefficient(g, np.asarray(p).size))))


# ----------------------------------------------------------------------------------------------------------------------------------------
# LeCam
# ----------------------------------------------------------------------------------------------------------------------------------------
def _h(x, rectified):
    return np.where(x > 0, x, np.where(x <= 0, 0.0, x)) if rectified else x


class LeCam:
    """The eight words as numpy scalars of their own types and the two launches on them."""

    def __init__(self, weight, decay=0.99, start=1000, rectified=False):
        self.weight, self.decay, self.start, self.rectified = F(weight), F(decay), int(start), bool(rectified)
        self.a_real = self.a_fake = self.m_real = self.m_fake = F(0.0)
        self.updates = self.active = np.int32(0)

    def ema(self, a, m, fma=False):
        c = F(F(1.0) - self.decay)
        if fma:                                            # a planted defect: fl(decay * a + fl(c * m)), one rounding fewer
            return F(np.float64(self.decay) * np.float64(a) + np.float64(F(c * m)))
        return F(F(self.decay * a) + F(c * m))

    def forward(self, p_real, p_fake, means=None, fma=False, drop_tail=False):
        """One sp_lecam_fwd: updates the state; returns (reg as fp32, reg in float64).  means: (m_real, m_fake) to take in place of the
        restated ones (the device's, in the general regime: the anchors are specified GIVEN the means)."""
        pr, pf = np.asarray(p_real, dtype=np.float64).reshape(-1), np.asarray(p_fake, dtype=np.float64).reshape(-1)
        assert pr.size == pf.size
        n = pr.size
        if drop_tail:
            pr, pf = pr[:-1], pf[:-1]
        with np.errstate(over="ignore", invalid="ignore"):
            m_r, m_f = (F(np.sum(pr) / n), F(np.sum(pf) / n)) if means is None else (F(means[0]), F(means[1]))
        self.m_real, self.m_fake = m_r, m_f
        k = int(self.updates)
        if np.isfinite(m_r) and np.isfinite(m_f):
            if k < self.start:
                self.a_real, self.a_fake = m_r, m_f
            else:
                self.a_real, self.a_fake = self.ema(self.a_real, m_r, fma), self.ema(self.a_fake, m_f, fma)
            self.updates = np.int32(min(k + 1, INT_MAX))
        self.active = np.int32(1 if k >= self.start else 0)
        if not self.active:
            return F(0.0), 0.0
        with np.errstate(over="ignore", invalid="ignore"):
            s = np.sum(_h(pr - np.float64(self.a_fake), self.rectified) ** 2) + np.sum(_h(np.float64(self.a_real) - pf, self.rectified) ** 2)
            exact = float(np.float64(self.weight) * s / n)
            return F(exact), exact

    def coefficient(self, g, n):
        return F(F(F(g) * self.weight) * F(F(2.0) / F(n)))

    def backward(self, p_real, p_fake, g):
        """One sp_lecam_bwd on the state forward left: (dp_real, dp_fake) in float64."""
        pr, pf = np.asarray(p_real, dtype=np.float64), np.asarray(p_fake, dtype=np.float64)
        if not self.active:
            return np.zeros_like(pr), np.zeros_like(pf)
        c = np.float64(self.coefficient(g, pr.size))
        return c * _h(pr - np.float64(self.a_fake), self.rectified), -c * _h(np.float64(self.a_real) - pf, self.rectified)

    def words(self):
        """The state as the device holds it: 8 int32 words, the four floats by their bits."""
        bits = lambda v: int(np.array(v, dtype=F).view(np.int32))      # noqa: E731
        return [bits(self.a_real), bits(self.a_fake), int(self.updates), int(self.active), bits(self.m_real), bits(self.m_fake), 0, 0]


def lecam_exact_operands(n, seed=0):
    """(p_real, p_fake): n multiples of 1/4 in [-2, 2] each, arranged in pairs (x, m2 - x) so that each mean is the multiple m of 1/4
    it is built around, the last element not equal to the mean.  With decay 0.5, at most three updates past start and a power-of-two
    weight every intermediate is exact in fp32: the anchors are multiples of 2^-5, the differences of 2^-5 below 4, their squares of
    2^-10 below 16, and a sum of at most 2 x 512 of them stays below 2^24 x 2^-10."""
    assert n >= 2 and n & (n - 1) == 0 and n <= 512
    rng = np.random.default_rng(3000 + seed + n)
    out = []
    for mean in (0.5, -0.25):
        lo, hi = max(-2.0, 2 * mean - 2.0), min(2.0, 2 * mean + 2.0)
        x = rng.integers(int(lo * 4), int(hi * 4) + 1, size=n // 2).astype(np.float64) / 4
        p = np.stack([x, 2 * mean - x], axis=1).reshape(-1)
        if p[-1] == mean:
            p[-2], p[-1] = mean + 0.25, mean - 0.25
        assert np.all(p * 4 == np.round(p * 4)) and np.abs(p).max() <= 2 and p.sum() / n == mean and p[-1] != mean
        out.append(p.astype(F))
    return out


def lecam_general_operands(n, seed=0):
    rng = np.random.default_rng(4000 + seed + n)
    return (rng.normal(0.3, 1.0, size=n)).astype(F), (rng.normal(-0.2, 1.0, size=n)).astype(F)


def lecam_mean_bound(p, m, aligned):
    p = np.asarray(p, dtype=np.float64)
    return gamma(chain(p.size, aligned) + 1) * float(np.abs(p).mean()) + ulp(m) / 2


def lecam_reg_bound(exact, n, aligned):
    return gamma(chain(n, aligned) + 4) * abs(exact) + ulp(exact) / 2


def lecam_grad_bound(exact):
    return gamma(2) * np.abs(exact)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the training step on the oracle
# ----------------------------------------------------------------------------------------------------------------------------------------
def torch_d_loss(kind, pred_real, pred_fake):
    if kind == "lsgan":
        return O.lsgan_discriminator_loss(pred_real, pred_fake)
    if kind == "hinge":
        return torch.relu(1.0 - pred_real).mean(), torch.relu(1.0 + pred_fake).mean()
    return torch.nn.functional.softplus(-pred_real).mean(), torch.nn.functional.softplus(pred_fake).mean()


def torch_g_loss(kind, pred_fake):
    if kind == "lsgan":
        return O.lsgan_generator_loss(pred_fake)
    return -pred_fake.mean() if kind == "hinge" else torch.nn.functional.softplus(-pred_fake).mean()


class TorchLeCam:
    """The regularizer on torch tensors for the oracle's step: the state machine is LeCam's above (fp32 anchors, the means of the oracle's
    own predictions), the regularizer a differentiable torch expression with the anchors as constants."""

    def __init__(self, weight, decay, start, rectified=False):
        self.machine = LeCam(weight, decay, start, rectified)

    def __call__(self, pred_real, pred_fake):
        m = self.machine
        m.forward(pred_real.detach().numpy(), pred_fake.detach().numpy())
        if not m.active:
            return torch.zeros((), dtype=torch.float32)
        h = torch.relu if m.rectified else (lambda x: x)
        return float(m.weight) * ((h(pred_real - float(m.a_fake)) ** 2).mean() + (h(float(m.a_real) - pred_fake) ** 2).mean())


def train_step_restated(G, D, V, opt_g, opt_d, images_real, labels, masks, noise_d, noise_g, kind="lsgan", lecam=None, w_rec=0.1, w_div=0.1,
                        skip_dead_d_wgrad=False):
    """The oracle's train_step with the restated losses of `kind` in place of O.lsgan_* and, with `lecam` (a TorchLeCam), the regularizer
    added to the discriminator's objective - as ada_restated.train_step_gated is the oracle's step with the gate.  Also returns D's
    predictions of the discriminator phase and the regularizer."""
    out = {}
    O.zero_grads(G); O.zero_grads(D)
    with torch.no_grad():
        feats_real = O.vgg16_forward(V, images_real)
        fake = O.generator_forward(G, noise_d, feats_real, masks, labels.float(), training=True)
    out["images_fake_d"] = fake
    pred_real = O.discriminator_forward(D, images_real, labels, training=True)
    pred_fake = O.discriminator_forward(D, fake, labels, training=True)
    out["prediction_real"], out["prediction_fake"] = pred_real.detach().clone(), pred_fake.detach().clone()
    reg = lecam(pred_real, pred_fake) if lecam is not None else torch.zeros(())
    l_real, l_fake = torch_d_loss(kind, pred_real, pred_fake)
    (l_real + l_fake + reg).backward()
    out["grads_d"] = [q.grad.detach().clone() for q in O.trainable(D)]
    opt_d.step()
    O.zero_grads(G); O.zero_grads(D)
    if skip_dead_d_wgrad:
        d_params = O.trainable(D)
        for q in d_params:
            q.requires_grad_(False)
    fake = O.generator_forward(G, noise_g, feats_real, masks, labels.float(), training=True)
    pred_fake = O.discriminator_forward(D, fake, labels, training=True)
    l_g = torch_g_loss(kind, pred_fake)
    l_div = w_div * O.diversity_loss(fake, noise_g)
    feats_fake = O.vgg16_forward(V, fake)
    l_rec = w_rec * O.semantic_reconstruction_loss(feats_real, feats_fake, masks)
    (l_g + l_rec + l_div).backward()
    if skip_dead_d_wgrad:
        for q in d_params:
            q.requires_grad_(True)
    out["grads_g"] = [q.grad.detach().clone() for q in O.trainable(G)]
    opt_g.step()
    out.update(images_fake_g=fake.detach(), loss_d_real=l_real.detach(), loss_d_fake=l_fake.detach(), loss_g=l_g.detach(),
               loss_rec=l_rec.detach().reshape(()), loss_div=l_div.detach(), loss_lecam=reg.detach())
    return out
