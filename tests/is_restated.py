"""The Inception Score restated in float64 on the CPU, the reference of tests/test_is_host.py and tests/test_gpu_is.py.
The definition is the papers', not any package's: Salimans et al. 2016 ("Improved Techniques for Training GANs"), in the split form
that StyleGAN2-ADA (Karras et al. 2020) and torch-fidelity compute.

    l_ic  = x_i . w_c + b_c                      lse_i = m_i + log sum_c exp(l_ic - m_i), m_i = max_c l_ic
    p_ic  = exp(l_ic - lse_i)                    h_i   = sum_c p_ic (l_ic - lse_i)
    split s (0-based) = rows [floor(s n / S), floor((s + 1) n / S)), n_s of them;   q_sc = (1 / n_s) sum_{i in s} p_ic
    KL_s  = (1 / n_s) sum_{i in s} h_i - sum_c q_sc log q_sc   (0 log 0 = 0);   score_s = exp(KL_s)
    inception_score = mean_s score_s;   inception_score_std = sqrt(mean_s (score_s - mean)^2)   (the population form)

A non-finite logit makes its split's KL_s NaN, and with it both results."""
import math

import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
U64 = 1.01 * 2.0 ** -53             # float64 unit roundoff, second-order terms included
ULPS = 4                            # exp / log in double: OpenCL's limit (what the device's math library is built to) is 3 ulp; numpy's is below it
EPS_F = ULPS * 2.0 ** -52           # ... as a relative error


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def split_bounds(n, splits):
    return [(s * n // splits, (s + 1) * n // splits) for s in range(splits)]


def logits(x, w, b):
    """float64 logits of fp32 operands (the products are exact in float64, the sum is float64's)."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)


def row_stats(l):
    """(lse, h, p) per row of a float64 logit matrix."""
    l = np.asarray(l, dtype=np.float64)
    m = l.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(l - m).sum(axis=1, keepdims=True))
    logp = l - lse
    p = np.exp(logp)
    return lse[:, 0], (p * logp).sum(axis=1), p


def _xlogx(q):
    out = np.zeros_like(q)
    nz = q != 0
    out[nz] = q[nz] * np.log(q[nz])
    return out


def kl_splits(l, splits=10):
    """KL_s, float64 (splits,); NaN where a logit of the split is not finite."""
    l = np.asarray(l, dtype=np.float64)
    out = np.empty(splits)
    for s, (lo, hi) in enumerate(split_bounds(l.shape[0], splits)):
        assert hi > lo, "more splits than rows"
        if not np.all(np.isfinite(l[lo:hi])):
            out[s] = np.nan
            continue
        _, h, p = row_stats(l[lo:hi])
        q = p.sum(axis=0) / (hi - lo)
        out[s] = h.sum() / (hi - lo) - _xlogx(q).sum()
    return out


def colsums(l, splits):
    """(splits, C): per split the column sums of the softmax (finite logits)."""
    l = np.asarray(l, dtype=np.float64)
    return np.stack([row_stats(l[lo:hi])[2].sum(axis=0) for lo, hi in split_bounds(l.shape[0], splits)])


def score_from_kl(kl):
    scores = np.exp(np.asarray(kl, dtype=np.float64))
    mean = scores.mean()
    return float(mean), float(np.sqrt(((scores - mean) ** 2).mean()))


def inception_score(x, w, b, splits=10):
    """(inception_score, inception_score_std)."""
    return score_from_kl(kl_splits(logits(x, w, b), splits))


# ---- the same in other summation orders, and in extended precision --------------------------------------------------------------------
def _seq(a, axis):
    """A strictly sequential sum along `axis` (cumsum adds in index order; numpy.sum adds pairwise)."""
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def kl_splits_ordered(l, splits, order):
    """kl_splits with every sum in a stated order: "forward" / "reversed" (strictly sequential over classes and rows) or "blocks64"
    (the device's form: per block of 64 classes the state (m, s = sum exp(l - m), t = sum exp(l - m) l), the blocks merged online,
    h = t / s - lse; rows and classes summed forward)."""
    l = np.asarray(l, dtype=np.float64)
    if order == "reversed":
        l = l[::-1, ::-1]
        bounds = [(l.shape[0] - hi, l.shape[0] - lo) for lo, hi in split_bounds(l.shape[0], splits)]
    else:
        bounds = split_bounds(l.shape[0], splits)
    out = np.empty(splits)
    for s, (lo, hi) in enumerate(bounds):
        x = l[lo:hi]
        if order == "blocks64":
            m = np.full(x.shape[0], -np.inf)
            sm, t = np.zeros(x.shape[0]), np.zeros(x.shape[0])
            for c0 in range(0, x.shape[1], 64):
                blk = x[:, c0:c0 + 64]
                mn = np.maximum(m, blk.max(axis=1))
                f = np.exp(m - mn)
                e = np.exp(blk - mn[:, None])
                sm, t, m = sm * f + _seq(e, 1), t * f + _seq(e * blk, 1), mn
            lse = m + np.log(sm)
            h = t / sm - lse
        else:
            m = x.max(axis=1)
            lse = m + np.log(_seq(np.exp(x - m[:, None]), 1))
            h = None
        logp = x - lse[:, None]
        p = np.exp(logp)
        if h is None:
            h = _seq(p * logp, 1)
        q = _seq(p, 0) / (hi - lo)
        out[s] = _seq(h, 0) / (hi - lo) - _seq(_xlogx(q), 0)
    return out


def kl_splits_longdouble(l, splits):
    """kl_splits in numpy.longdouble (64 significand bits on x86), returned as longdouble."""
    l = np.asarray(l, dtype=np.longdouble)
    out = np.empty(splits, dtype=np.longdouble)
    for s, (lo, hi) in enumerate(split_bounds(l.shape[0], splits)):
        x = l[lo:hi]
        m = x.max(axis=1, keepdims=True)
        logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
        p = np.exp(logp)
        q = p.sum(axis=0) / np.longdouble(hi - lo)
        out[s] = (p * logp).sum() / np.longdouble(hi - lo) - _xlogx(q).sum()
    return out


# ---- error bounds ------------------------------------------------------------------------------------------------------
def _float64_terms(classes, n_s, lmax):
    """The float64 evaluation error of one computed KL_s against the true value for GIVEN logits with |l| <= lmax, for either form of
    h (sum p log p, or the online (m, s, t) merge with t / s - lse), any summation order and any segmentation of the classes.
    Returns (e_lse, e_h, r_q, e_kl): absolute bounds of lse_i and h_i, the relative bound of a column sum, the absolute bound of KL_s."""
    log_c = math.log(classes) if classes > 1 else 0.0
    span = 2.0 * lmax + log_c                                    # |l - lse| <= span
    assert span < 700.0, "exp(l - lse) must stay a normal number"
    rescales = 2 * (-(-classes // 64)) + 2                       # tile steps + segment merges + the two halves of a row: each exp, *, +
    d_s = EPS_F + (classes - 1) * U64 + rescales * (EPS_F + 2 * U64)          # relative, s = sum of positive terms
    e_lse = 1.01 * d_s + EPS_F * log_c + U64 * (lmax + log_c)                 # log(1 + d_s); log's own error (1 <= s <= C); m + log s
    # h as t / s - lse: t and s each within d_s (+ the product), |t| / s <= lmax; the division, the subtraction
    e_h_online = lmax * (2.02 * d_s + 3.02 * U64) + U64 * (2.0 * lmax + log_c) + e_lse
    # h as sum p logp: logp within e1, p relatively within r_p, products and a sum of C terms with sum p |logp| <= span
    e1 = e_lse + U64 * span
    r_p = 1.01 * e1 + EPS_F
    e_h_direct = span * (r_p + classes * U64) + e1
    e_h = max(e_h_online, e_h_direct)
    r_q = r_p + n_s * U64                                        # a column sum of n_s positive terms, divided by n_s
    # sum_c q log q under q (1 + delta): |delta| (q |log q| + 1.01 q) per class, sum q = 1, sum q |log q| <= log C; log, product, C-term sum
    e_q = r_q * (log_c + 1.01) + 1.01 * (EPS_F + (classes + 1) * U64) * log_c
    e_mean_h = e_h + (n_s + 1) * U64 * max(log_c, 1.0)           # |h_i| <= log C
    e_kl = e_mean_h + e_q + 2 * U64 * max(log_c, 1.0)
    return e_lse, e_h, r_q, e_kl


def row_exact_bounds(classes, lmax):
    """(|lse_i - restated|, |h_i - restated|) for exact logits: the device and the restatement are each within the float64 terms."""
    e_lse, e_h, _, _ = _float64_terms(classes, 1, lmax)
    return 2.0 * e_lse, 2.0 * e_h


def colsum_total_bound(classes, n_s, lmax):
    """|sum_c colsum[s][c] - n_s|: every p relatively within r_q's terms, and the checking sum of C terms."""
    return n_s * (_float64_terms(classes, n_s, lmax)[2] + classes * U64)


def kl_exact_bound(classes, n_s, lmax):
    """|KL_s(device) - KL_s(restated)| for logits that are exact in fp32 (the exact regime): both are float64 evaluations of the same
    numbers, each within the float64 terms of the true value."""
    return 2.0 * _float64_terms(classes, n_s, lmax)[3]


def logit_error(x, w, b):
    """e_ic = 1.01 (gamma_d + 2u) (sum_l |x_il| |w_cl| + |b_c|): a length-d fp32 dot in any order, the bias added."""
    x, w, b = (np.abs(np.asarray(v, dtype=np.float64)) for v in (x, w, b))
    d = x.shape[1]
    gamma = d * U / (1.0 - d * U)
    return 1.01 * (gamma + 2 * U) * (x @ w.T + b)


def kl_general_bound(l, err, splits):
    """(first order, total) per split for logits within `err` of l.  First order: sum_ic |dKL_s / dl_ic| e_ic,
    dKL_s / dl_ic = p_ic (a_ic - K_i) / n_s, a_ic = log(p_ic / q_sc), K_i = sum_c p_ic a_ic.  Total: by the mean value theorem
    |dKL_s| <= sup sum |g_ic(xi)| e_ic over the segment; with E = max e_ic every log p and log q moves by <= 2 E, so a by <= 4 E,
    K_i by <= 4 E + (e^{2E} - 1)(A_i + 4 E), A_i = sum_c p_ic |a_ic|, and p by the factor e^{2E}; plus the float64 terms."""
    l, err = np.asarray(l, dtype=np.float64), np.asarray(err, dtype=np.float64)
    first, total = np.empty(splits), np.empty(splits)
    for s, (lo, hi) in enumerate(split_bounds(l.shape[0], splits)):
        _, _, p = row_stats(l[lo:hi])
        e = err[lo:hi]
        q = p.sum(axis=0) / (hi - lo)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(p > 0, np.log(p) - np.log(q)[None, :], 0.0)
        k = (p * a).sum(axis=1, keepdims=True)
        big_a = (p * np.abs(a)).sum(axis=1, keepdims=True)
        emax = float(e.max())
        grow = math.expm1(2.0 * emax)
        first[s] = (p * np.abs(a - k) * e).sum() / (hi - lo)
        moved = np.abs(a - k) + 8.0 * emax + grow * (big_a + 4.0 * emax)
        total[s] = (1.0 + grow) * (p * moved * e).sum() / (hi - lo) + kl_exact_bound(l.shape[1], hi - lo, float(np.abs(l[lo:hi]).max()) + emax)
    return first, total


def score_bounds(kl, kl_bound):
    """(|mean - restated|, |std - restated|) for KL_s within kl_bound[s]: score_s moves by at most exp(KL_s) (e^bound - 1); the mean by
    the mean of that, the population std (a seminorm of the scores) by its maximum; a few float64 roundings on top."""
    kl, kl_bound = np.asarray(kl, dtype=np.float64), np.broadcast_to(np.asarray(kl_bound, dtype=np.float64), np.shape(kl))
    move = np.exp(kl) * np.expm1(kl_bound) + 16 * U64 * np.exp(kl)
    return float(move.mean()), float(move.max())


# ---- the operand sets both test files use ---------------------------------------------------------------------------------------------
# (n, classes, d): every shape of tests/test_gpu_is.py's exact regime
EXACT_CASES = [(2, 3, 8), (131, 72, 72), (389, 1000, 72), (389, 1000, 2048), (131, 40, 70), (5, 72, 72)]
EXACT_LMAX = 26                     # 8 entries of +-1 against activations <= 3, bias within [-2, 2]

_EXACT = {}


def exact_operands(n, classes, d, seed=None):
    """Exact regime: integer activations in {0..3}, every class row exactly 8 entries of +-1 (the rest zero), integer bias in [-2, 2];
    |dot| <= 24, so every logit is an exact integer in fp32 whatever the summation order.  (x, w, b, float64 logits), computed once."""
    key = (n, classes, d, seed)
    if key not in _EXACT:
        rng = np.random.RandomState(n + classes + d if seed is None else seed)
        x = rng.randint(0, 4, size=(n, d)).astype(np.float32)
        w = np.zeros((classes, d), dtype=np.float32)
        for c in range(classes):
            w[c, rng.choice(d, 8, replace=False)] = rng.choice([-1.0, 1.0], 8)
        b = rng.randint(-2, 3, size=classes).astype(np.float32)
        _EXACT[key] = (x, w, b, logits(x, w, b))
    return _EXACT[key]


def check_exact(x, w, b, l):
    """The conditions of the exact regime, asserted before any launch, and one that keeps the case meaningful: the mean over the rows
    of max_c p_ic lies in (0.05, 0.9) - neither uniform nor one-hot (rows of at least 40 classes)."""
    assert x.dtype == w.dtype == b.dtype == np.float32
    assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 3
    assert np.all((np.abs(w) == 1).sum(axis=1) == 8) and np.all((w != 0).sum(axis=1) == 8)
    assert np.array_equal(b, np.round(b)) and np.abs(b).max() <= 2
    assert np.array_equal(l, np.round(l)) and np.abs(l).max() <= EXACT_LMAX
    assert np.array_equal((x @ w.T + b).astype(np.float64), l)              # fp32 arithmetic gives the same integers
    if w.shape[0] >= 40:
        peak = row_stats(l)[2].max(axis=1).mean()
        assert 0.05 < peak < 0.9, peak


_GENERAL = {}


def general_operands(n=389, classes=1000, d=72, seed=5):
    """General regime: ReLU-of-normal rows, normal class rows scaled by 2 / sqrt(d), normal bias scaled by 0.1, rounded to fp32.
    (x, w, b, float64 logits, e_ic), computed once."""
    key = (n, classes, d, seed)
    if key not in _GENERAL:
        rng = np.random.RandomState(seed)
        x = np.maximum(rng.standard_normal((n, d)), 0).astype(np.float32)
        w = (rng.standard_normal((classes, d)) * (2.0 / math.sqrt(d))).astype(np.float32)
        b = (0.1 * rng.standard_normal(classes)).astype(np.float32)
        _GENERAL[key] = (x, w, b, logits(x, w, b), logit_error(x, w, b))
    return _GENERAL[key]
