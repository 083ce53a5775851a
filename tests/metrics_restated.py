"""The pair-set metrics restated in float64 on the CPU, the reference of tests/test_metrics_host.py and
tests/test_gpu_metrics.py.  Definitions from the papers, not from any package:

    KID                  Binkowski et al. 2018 ("Demystifying MMD GANs"), subsets and kernel as in StyleGAN2-ADA (Karras et al. 2020)
    precision / recall   Kynkaanniemi et al. 2019 ("Improved Precision and Recall Metric for Assessing Generative Models")
    density / coverage   Naeem et al. 2020 ("Reliable Fidelity and Diversity Metrics for Generative Models")

D(x, y) is the SQUARED Euclidean distance; every ball is closed (<=); the self entry of a radius is excluded by index."""
import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
EXACT_LIMIT = 2 ** 22               # exact regime: d * amax^2 <= 2^22, so norms, dots and (na + nb) - 2 dot stay below 2^24


def sqdist(a, b):
    """(na, nb) float64 squared distances, from differences (no cancellation of large numbers)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        diff = b - a[i]
        out[i] = np.einsum("jk,jk->j", diff, diff)
    return out


def sqdist_gram(a, b):
    """The same through the Gram matrix - exact for integer operands, and fast at d = 2048."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2.0 * (a @ b.T)


def kth_smallest(dist, k, same=False):
    """Row-wise k-th smallest (k = 1: the smallest); same: entry (i, i) is left out by index."""
    dist = np.array(dist, dtype=np.float64)
    if same:
        assert dist.shape[0] == dist.shape[1]
        dist[np.arange(dist.shape[0]), np.arange(dist.shape[0])] = np.inf
    assert k < dist.shape[1] - (1 if same else 0)
    return np.sort(dist, axis=1)[:, k - 1]


def radii(x, k, dist_fn=sqdist):
    return kth_smallest(dist_fn(x, x), k, same=True)


def cover(dist, rad_a=None, rad_b=None):
    """What sp_pairset_cover returns for the (na, nb) matrix: row_count, col_count, row_min, col_min (counts None without radii)."""
    row_count = (dist <= rad_b[None, :]).sum(1).astype(np.int32) if rad_b is not None else None
    col_count = (dist <= rad_a[:, None]).sum(0).astype(np.int32) if rad_a is not None else None
    return row_count, col_count, dist.min(1), dist.min(0)


def prdc(real, fake, nearest_k=5, dist_fn=sqdist):
    real_r, fake_r = radii(real, nearest_k, dist_fn), radii(fake, nearest_k, dist_fn)
    dist = dist_fn(fake, real)                                   # rows: fake j, columns: real i
    inside_real = dist <= real_r[None, :]                        # f_j in the ball of r_i
    inside_fake = dist <= fake_r[:, None]                        # r_i in the ball of f_j
    m = fake.shape[0]
    return {"precision": float(inside_real.any(1).mean()),
            "recall": float(inside_fake.any(0).mean()),
            "density": float(inside_real.sum() / (nearest_k * m)),
            "coverage": float((dist.min(0) <= real_r).mean())}


def kid_indices(n_real, n_fake, num_subsets=100, max_subset_size=1000, seed=0):
    """The pinned draw order: per subset x = m fake rows first, then y = m real rows, numpy RandomState(seed).choice without replacement."""
    m = min(n_real, n_fake, max_subset_size)
    rs = np.random.RandomState(seed)
    ix, iy = [], []
    for _ in range(num_subsets):
        ix.append(rs.choice(n_fake, m, replace=False))
        iy.append(rs.choice(n_real, m, replace=False))
    return np.asarray(ix, dtype=np.int32).reshape(num_subsets, m), np.asarray(iy, dtype=np.int32).reshape(num_subsets, m), m


def poly3_sum(a, b, skip_diag=False):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    k = (a @ b.T / a.shape[1] + 1.0) ** 3
    return float(k.sum() - (np.trace(k) if skip_diag else 0.0))


def kid_from_sums(sxx, syy, sxy, m):
    """sxx / syy: off-diagonal Gram sums per subset, sxy: full sums."""
    sxx, syy, sxy = (np.asarray(v, dtype=np.float64) for v in (sxx, syy, sxy))
    t = ((sxx + syy) / (m - 1) - 2.0 * sxy / m).sum()
    return float(t / len(sxx) / m)


def kid(real, fake, num_subsets=100, max_subset_size=1000, seed=0):
    ix, iy, m = kid_indices(real.shape[0], fake.shape[0], num_subsets, max_subset_size, seed)
    sxx = [poly3_sum(fake[i], fake[i], True) for i in ix]
    syy = [poly3_sum(real[i], real[i], True) for i in iy]
    sxy = [poly3_sum(fake[i], real[j]) for i, j in zip(ix, iy)]
    return kid_from_sums(sxx, syy, sxy, m)


# ---- operand conditions and bounds ------------------------------------------------------------------------------------------------
def check_exact(*sets):
    """Exact regime, asserted before any launch: integer features with d * amax^2 <= 2^22.  Every norm and every dot is then an integer
    of magnitude <= 2^22 and (|a|^2 + |b|^2) - 2 a.b, in any association, one below 2^24: exact in fp32 whatever the summation order."""
    d = sets[0].shape[1]
    amax = 0.0
    for s in sets:
        s = np.asarray(s)
        assert s.dtype == np.float32 and s.shape[1] == d
        assert np.array_equal(s, np.round(s)), "exact regime: the features are not integers"
        amax = max(amax, float(np.abs(s).max()))
    assert d * amax * amax <= EXACT_LIMIT, (d, amax)


def dist_error(a, b):
    """e_ij = 1.01 (gamma + 3u) S_ij, S_ij = |a_i|^2 + |b_j|^2 + 2 sum_l |a_il| |b_jl|: three length-d fp32 sums in any order, two
    additions, second-order terms."""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    d = a.shape[1]
    gamma = d * U / (1.0 - d * U)
    s = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (a @ b.T)
    return 1.01 * (gamma + 3 * U) * s


def count_bracket(dist, err, rad, rad_err, axis):
    """lo = #{D <= rad - e}, hi = #{D <= rad + e}, e = the distance's error + the radius' own; rad indexed along `axis` of dist
    (axis = 1: one radius per column, counts per row; axis = 0: one per row, counts per column)."""
    r = rad[None, :] if axis == 1 else rad[:, None]
    e = err + (rad_err[None, :] if axis == 1 else rad_err[:, None])
    return (dist <= r - e).sum(axis).astype(np.int64), (dist <= r + e).sum(axis).astype(np.int64)


def poly3_bound(terms):
    """Relative bound of a float64 sum of `terms` cubes: two roundings for t, two for the cube, terms - 1 additions of positive terms."""
    return 1.01 * (terms + 5) * 2.0 ** -53


# ---- the operand sets both test files use -------------------------------------------------------------------------------------------
# (na, nb, d, amax, signed): every shape of tests/test_gpu_metrics.py's exact regime
EXACT_CASES = [(2, 2, 8, 45, True), (129, 131, 72, 45, True), (129, 131, 72, 45, False), (389, 389, 2048, 45, True),
               (389, 389, 2048, 45, False), (1, 130, 72, 45, True), (130, 1, 72, 45, False), (389, 421, 2048, 45, False)]


def exact_sets(na, nb, d, amax, signed, seed):
    """Integer features in [-amax, amax] (signed) or [0, amax] as fp32, with planted duplicate rows: a[3] = a[1] and a[na - 1] = a[0]
    (one pair inside a 128-row block, one across block boundaries where na > 128), b[2] = a[1] where both exist."""
    rng = np.random.RandomState(seed)
    lo = -amax if signed else 0
    a = rng.randint(lo, amax + 1, size=(na, d)).astype(np.float32)
    b = rng.randint(lo, amax + 1, size=(nb, d)).astype(np.float32)
    if na >= 5:
        a[3] = a[1]
        a[na - 1] = a[0]
        if nb >= 3:
            b[2] = a[1]
    return a, b


_GENERAL = {}


def general_case(na=389, nb=421, d=72, ka=3, kb=5, seed=7):
    """General regime: ReLU of standard normal features rounded to fp32.  The float64 distances, radii (ka for a, kb for b), counts,
    the error bound of every distance and of every radius (taking the k-th smallest is 1-Lipschitz in the sup norm: max_j e_ij over
    the other rows), and the count brackets with the radius' own error included."""
    key = (na, nb, d, ka, kb, seed)
    if key in _GENERAL:
        return _GENERAL[key]
    rng = np.random.RandomState(seed)
    a = np.maximum(rng.standard_normal((na, d)), 0).astype(np.float32)
    b = np.maximum(rng.standard_normal((nb, d)), 0).astype(np.float32)
    dist, err = sqdist(a, b), dist_error(a, b)
    out = {"a": a, "b": b, "ka": ka, "kb": kb, "dist": dist, "err": err}
    for name, x, k in (("a", a, ka), ("b", b, kb)):
        e = dist_error(x, x)
        np.fill_diagonal(e, 0.0)
        out["rad_" + name] = radii(x, k)
        out["rad_%s_err" % name] = e.max(1)
    out["row_count"], out["col_count"], out["row_min"], out["col_min"] = cover(dist, out["rad_a"], out["rad_b"])
    out["row_lo"], out["row_hi"] = count_bracket(dist, err, out["rad_b"], out["rad_b_err"], axis=1)
    out["col_lo"], out["col_hi"] = count_bracket(dist, err, out["rad_a"], out["rad_a_err"], axis=0)
    out["row_min_err"], out["col_min_err"] = err.max(1), err.max(0)
    _GENERAL[key] = out
    return out
