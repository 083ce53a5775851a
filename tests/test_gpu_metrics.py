"""The pair-set kernels (csrc/metrics.hip) on the GPU, through the C ABI's thin bindings (ops.pairset_*) unless stated.

Exact regime (integer features, d * amax^2 <= 2^22: every norm, dot and distance is an exact fp32 integer whatever the order of
summation): the device EQUALS the float64 restatement (tests/metrics_restated.py), bit for bit.  General regime (ReLU of normal
features, d = 72): every distance is within e_ij = 1.01 (gamma + 3u) S_ij of its float64 value, so radii and minima are held to that
and counts to the bracket [#{D <= rad - e}, #{D <= rad + e}].  poly3: a float64 sum of T cubes against exact integer arithmetic,
relative bound 1.01 (T + 5) 2^-53.  The operand conditions are asserted on the CPU before anything is launched."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import metrics_restated as R
from semantic_pyramid_for_image_generation_amd import _lib as L
from semantic_pyramid_for_image_generation_amd import metrics as M
from semantic_pyramid_for_image_generation_amd import ops

pytestmark = pytest.mark.gpu
SEG_KEY = L.TUNE_KEYS["SP_PAIRSET_SEGMENTS"]


def _dev(x):
    torch.cuda.set_device(0)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _assert_equal_f32(got, want64, what):
    """got (device fp32) == the float64 reference, which must itself be an fp32 value: equality of the bits."""
    want32 = want64.astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want64), what
    g = got.cpu().numpy()
    bad = np.flatnonzero(g.view(np.int32) != want32.view(np.int32))
    assert bad.size == 0, (what, "%d of %d differ" % (bad.size, g.size), [(int(i), float(g[i]), float(want32[i])) for i in bad[:5]])


_SETS = {}


def _exact(na, nb, d, signed, same=False):
    """(a, b, float64 distances) of an exact-regime case, computed once and shared; same: b is a."""
    key = (na, nb, d, signed, same)
    if key not in _SETS:
        a, b = R.exact_sets(na, nb, d, 45, signed, seed=na + d)
        if same:
            b = a
        R.check_exact(a, b)
        _SETS[key] = (a, b, R.sqdist_gram(a, b))
    return _SETS[key]


# ---- knn ------------------------------------------------------------------------------------------------------------------------------
KNN_CASES = [(2, 2, 8, 1, False), (129, 131, 72, 1, False), (129, 131, 72, 3, False), (129, 131, 72, 16, False),
             (129, 129, 72, 3, True),           # same: the diagonal crosses the 64-column tiles of one 128-row block and enters a second
             (389, 389, 2048, 5, True)]


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "nonneg"])
@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: "%dx%d_d%d_k%d%s" % (c[0], c[1], c[2], c[3], "_same" if c[4] else ""))
def test_knn_exact(case, signed):
    na, nb, d, k, same = case
    a, b, dist = _exact(na, nb, d, signed, same)
    want = R.kth_smallest(dist, k, same=same)
    if na >= 5 and same:
        nearest = R.kth_smallest(dist, 1, same=True)
        assert nearest[1] == 0 and nearest[3] == 0 and nearest[0] == 0 and nearest[na - 1] == 0      # the planted duplicates: neighbours at distance 0
        assert np.all(want[[0, 1, 3, na - 1]] > 0)      # ... and one duplicate is one neighbour, not k of them
    ad = _dev(a)
    got = ops.pairset_knn(ad, ad if same else _dev(b), k, same=same)
    _assert_equal_f32(got, want, case)


@pytest.mark.parametrize("segments", [1, 3, 7])
def test_knn_forced_segments_give_the_same_bits(segments):
    a, _, dist = _exact(389, 389, 2048, True, True)
    want = R.kth_smallest(dist, 5, same=True)
    ad = _dev(a)
    lib = L.lib()
    try:
        assert lib.sp_set_tuning(SEG_KEY, segments) == 0
        got = ops.pairset_knn(ad, ad, 5, same=True)
        torch.cuda.synchronize()
    finally:
        lib.sp_set_tuning(SEG_KEY, -1)
    _assert_equal_f32(got, want, segments)


# ---- cover ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radii", ["a", "b", "both"])
@pytest.mark.parametrize("shape", [(1, 130, 72), (130, 1, 72), (389, 421, 2048)], ids=lambda s: "%dx%d_d%d" % s)
def test_cover_exact(shape, radii):
    """Radii that ARE distances of the matrix (the third smallest of each row / column where there are three): every row and column
    holds a tie at its radius, which <= counts and < would not."""
    na, nb, d = shape
    a, b, dist = _exact(na, nb, d, na == 1)
    rad_a = np.sort(dist, axis=1)[:, min(2, nb - 1)]
    rad_b = np.sort(dist, axis=0)[min(2, na - 1), :]
    assert np.all((dist == rad_a[:, None]).sum(1) >= 1) and np.all((dist == rad_b[None, :]).sum(0) >= 1)
    use_a, use_b = radii in ("a", "both"), radii in ("b", "both")
    want = R.cover(dist, rad_a if use_a else None, rad_b if use_b else None)
    got = ops.pairset_cover(_dev(a), _dev(b), rad_a=_dev(rad_a.astype(np.float32)) if use_a else None,
                            rad_b=_dev(rad_b.astype(np.float32)) if use_b else None)
    for name, g, w in zip(("row_count", "col_count"), got[:2], want[:2]):
        assert (g is None) == (w is None), name
        if w is not None:
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (name, shape, radii)
    _assert_equal_f32(got[2], want[2], "row_min")
    _assert_equal_f32(got[3], want[3], "col_min")
    if use_a and use_b and min(na, nb) > 2:
        assert int(want[0].sum()) >= 3 * nb and int(want[1].sum()) >= 3 * na                  # the ties are counted


# ---- poly3 ----------------------------------------------------------------------------------------------------------------------------
def _poly3_case(src, m, d, subsets, signed, seed):
    rng = np.random.RandomState(seed)
    amax = 45 if d > 72 else 9
    lo = -amax if signed else 0
    a = rng.randint(lo, amax + 1, size=(src, d)).astype(np.float32)
    b = rng.randint(lo, amax + 1, size=(src + 3, d)).astype(np.float32)
    assert d * amax * amax < 2 ** 24                                        # every dot is an exact fp32 integer
    ia = np.stack([rng.permutation(src)[:m] for _ in range(subsets)]).astype(np.int32)      # permuting, crossing the row blocks
    ib = np.stack([rng.permutation(src + 3)[:m] for _ in range(subsets)]).astype(np.int32)
    return a, b, ia, ib


def _poly3_exact(a, b, skip_diag):
    """(sum (dot + d)^3, sum |dot + d|^3, terms) in Python integers."""
    d = a.shape[1]
    t = (a.astype(np.int64) @ b.astype(np.int64).T + d).astype(object)
    if skip_diag:
        np.fill_diagonal(t, 0)
    cubes = t * t * t
    return int(cubes.sum()), int(abs(cubes).sum()), t.size - (t.shape[0] if skip_diag else 0)


@pytest.mark.parametrize("skip_diag", [False, True], ids=["full", "skip_diag"])
@pytest.mark.parametrize("case", [(130, 64, False), (130, 72, False), (257, 2048, False), (130, 72, True)],
                         ids=lambda c: "m%d_d%d%s" % (c[0], c[1], "_signed" if c[2] else ""))
def test_poly3_against_integer_arithmetic(case, skip_diag):
    m, d, signed = case
    subsets, src = 3, m + 43
    a, b, ia, ib = _poly3_case(src, m, d, subsets, signed, seed=m + d)
    got = ops.pairset_poly3(_dev(a), _dev(ia), _dev(b), _dev(ib), subsets, m, skip_diag).cpu().numpy()
    assert got.dtype == np.float64
    for s in range(subsets):
        total, total_abs, terms = _poly3_exact(a[ia[s]], b[ib[s]], skip_diag)
        assert terms == m * m - (m if skip_diag else 0)
        if not signed:
            assert total == total_abs
        err = abs(Fraction(float(got[s])) - Fraction(total, d ** 3))
        bound = Fraction(R.poly3_bound(terms)) * Fraction(total_abs, d ** 3)          # signed: taken on sum |t|^3
        print("poly3 m=%d d=%d subset %d: rel err %.3e, bound %.3e" % (m, d, s, float(err / Fraction(total_abs, d ** 3)), R.poly3_bound(terms)))
        assert err <= bound, (case, skip_diag, s, float(err), float(bound))


def test_poly3_without_tables_takes_the_first_rows():
    a, b, _, _ = _poly3_case(140, 130, 64, 1, False, seed=5)
    got = float(ops.pairset_poly3(_dev(a), None, _dev(b), None, 1, 130, False).cpu()[0])
    total, _, terms = _poly3_exact(a[:130], b[:130], False)
    assert abs(Fraction(got) - Fraction(total, 64 ** 3)) <= Fraction(R.poly3_bound(terms)) * Fraction(total, 64 ** 3)


# ---- general regime -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    g = R.general_case()
    for name in ("row", "col"):                                   # the condition on the inputs, before any launch
        assert ((g[name + "_lo"] != g[name + "_hi"]).mean()) <= 0.02
    return g


def test_general_regime_radii_counts_and_minima_within_the_bound(general):
    g = general
    ad, bd = _dev(g["a"]), _dev(g["b"])
    rad_a = ops.pairset_knn(ad, ad, g["ka"], same=True)
    rad_b = ops.pairset_knn(bd, bd, g["kb"], same=True)
    for name, got in (("a", rad_a), ("b", rad_b)):
        diff = np.abs(got.cpu().numpy().astype(np.float64) - g["rad_" + name])
        print("radius %s: max |err| / bound = %.3f" % (name, float((diff / g["rad_%s_err" % name]).max())))
        assert np.all(diff <= g["rad_%s_err" % name]), name
    row_count, col_count, row_min, col_min = ops.pairset_cover(ad, bd, rad_a=rad_a, rad_b=rad_b)
    for name, got in (("row", row_count), ("col", col_count)):
        c = got.cpu().numpy().astype(np.int64)
        assert np.all(g[name + "_lo"] <= c) and np.all(c <= g[name + "_hi"]), name
    for name, got in (("row", row_min), ("col", col_min)):
        diff = np.abs(got.cpu().numpy().astype(np.float64) - g[name + "_min"])
        assert np.all(diff <= g[name + "_min_err"]), name


def test_every_output_is_bit_identical_from_launch_to_launch(general):
    g = general
    ad, bd = _dev(g["a"]), _dev(g["b"])
    rng = np.random.RandomState(2)
    ia = _dev(np.stack([rng.permutation(389)[:200] for _ in range(3)]).astype(np.int32))
    ib = _dev(np.stack([rng.permutation(421)[:200] for _ in range(3)]).astype(np.int32))

    def run():
        rad_a = ops.pairset_knn(ad, ad, 3, same=True)
        rad_b = ops.pairset_knn(bd, ad, 5)
        cov = ops.pairset_cover(ad, bd, rad_a=rad_a, rad_b=rad_b)
        sums = ops.pairset_poly3(ad, ia, bd, ib, 3, 200, True)
        return [_bits(t) for t in (rad_a, rad_b) + tuple(cov) + (sums,)]

    first, second = run(), run()
    for i, (x, y) in enumerate(zip(first, second)):
        assert torch.equal(x, y), i


# ---- metrics.py -----------------------------------------------------------------------------------------------------------------------
def test_prdc_on_exact_operands_equals_the_restatement():
    real, fake, _ = _exact(129, 131, 72, False)
    want = R.prdc(real, fake, nearest_k=5, dist_fn=R.sqdist_gram)
    got = M.prdc(_dev(real), fake, nearest_k=5)                    # a device tensor and a numpy array (uploaded)
    assert sorted(got) == sorted(M.PRDC_KEYS)
    for key in M.PRDC_KEYS:
        assert got[key] == want[key], (key, got[key], want[key])   # ratios of equal integers
    same = M.prdc(real, real.copy(), nearest_k=3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0


def test_kid_on_exact_operands_within_the_propagated_bound():
    rng = np.random.RandomState(8)
    real = rng.randint(0, 10, size=(150, 72)).astype(np.float32)
    fake = rng.randint(0, 10, size=(140, 72)).astype(np.float32)
    subsets, size, seed, d = 3, 100, 4, 72
    ix, iy, m = R.kid_indices(150, 140, subsets, size, seed)
    assert m == 100
    want, tol = Fraction(0), Fraction(0)
    for s in range(subsets):
        sxx, _, txx = _poly3_exact(fake[ix[s]], fake[ix[s]], True)
        syy, _, tyy = _poly3_exact(real[iy[s]], real[iy[s]], True)
        sxy, _, txy = _poly3_exact(fake[ix[s]], real[iy[s]], False)
        sxx, syy, sxy = (Fraction(v, d ** 3) for v in (sxx, syy, sxy))
        want += (sxx + syy) / (m - 1) - 2 * sxy / m
        bound = Fraction(R.poly3_bound(max(txx, tyy, txy)))
        tol += bound * ((sxx + syy) / (m - 1) + 2 * sxy / m)
    want, tol = want / subsets / m, tol / subsets / m
    got = M.kid(_dev(real), _dev(fake), num_subsets=subsets, max_subset_size=size, seed=seed)
    print("kid %.17g, exact %.17g, |err| %.3e, bound %.3e" % (got, float(want), float(abs(Fraction(got) - want)), float(tol)))
    assert abs(Fraction(got) - want) <= tol
    assert abs(R.kid(real, fake, subsets, size, seed) - float(want)) <= float(tol)         # the restatement agrees with the integers


# ---- ModelWrapper.evaluate() end to end -----------------------------------------------------------------------------------------------
def test_evaluate_end_to_end(tmp_path):
    import _fid_child as C
    import inception_restated as IR
    import semantic_pyramid_for_image_generation_amd as sp
    from semantic_pyramid_for_image_generation_amd import fid
    weights = os.path.join(str(tmp_path), "inception_v3_google-random.pth")
    torch.save(IR.synth_state_dict(21), weights)
    ops.set_compute_dtype(torch.float32)
    plain, loader = C.setup(weights)
    torch.manual_seed(C.SEED)
    fid_plain = plain.validate()
    net = plain._inception
    mw = sp.ModelWrapper(plain.generator, plain.discriminator, None, loader, vgg16=plain.vgg16, save_data_path=None, inception=net,
                         metrics="kid,prdc")
    k = mw.metrics_nearest_k = 3
    torch.manual_seed(C.SEED)
    out = mw.evaluate()
    assert sorted(out) == ["coverage", "density", "fid", "kid", "precision", "recall"]
    assert all(math.isfinite(v) for v in out.values()) and mw.last_metrics == out
    assert mw.generator.training                                   # back in training mode
    assert abs(out["fid"] - fid_plain) <= 1e-9 * abs(fid_plain), (out["fid"], fid_plain)
    torch.manual_seed(C.SEED)
    again = mw.validate()                                          # validate() with metrics goes through evaluate(): still the FID, a float
    assert isinstance(again, float) and abs(again - fid_plain) <= 1e-9 * abs(fid_plain) and mw.generator.training

    # the restatement on the activations of fid.collect_activations under the same seed
    torch.manual_seed(C.SEED)
    mw.generator.eval()
    try:
        real, fake = fid.collect_activations(loader, mw.generator, mw.vgg16, device=torch.device("cuda", 0), inception=net)
    finally:
        mw.generator.train()
    n, m = real.shape[0], fake.shape[0]
    assert n == m == C.BATCH * C.BATCHES
    dist, err = R.sqdist(fake, real), R.dist_error(fake, real)     # rows: fake, columns: real
    rad, rad_err = {}, {}
    for name, x in (("real", real), ("fake", fake)):
        e = R.dist_error(x, x)
        np.fill_diagonal(e, 0.0)
        rad[name], rad_err[name] = R.radii(x, k), e.max(1)
    row_lo, row_hi = R.count_bracket(dist, err, rad["real"], rad_err["real"], axis=1)
    col_lo, col_hi = R.count_bracket(dist, err, rad["fake"], rad_err["fake"], axis=0)
    cmin, cmin_err = dist.min(0), err.max(0)
    bracket = {"precision": ((row_lo > 0).mean(), (row_hi > 0).mean()),
               "recall": ((col_lo > 0).mean(), (col_hi > 0).mean()),
               "density": (row_lo.sum() / (k * m), row_hi.sum() / (k * m)),
               "coverage": ((cmin + cmin_err <= rad["real"] - rad_err["real"]).mean(), (cmin - cmin_err <= rad["real"] + rad_err["real"]).mean())}
    for key, (lo, hi) in bracket.items():
        print("%s: %.6f in [%.6f, %.6f]" % (key, out[key], lo, hi))
        assert lo <= out[key] <= hi, (key, out[key], lo, hi)

    # KID: every dot is within eps = 1.01 gamma sum |a| |b| of its float64 value, t = dot / d + 1, so a cube moves by at most
    # 3 (|t| + eps / d)^2 eps / d; on top the float64 sum's own bound.  m = N: every subset is a permutation of all rows.
    d = real.shape[1]
    gamma = d * R.U / (1 - d * R.U)

    def sums(a, b, skip):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        t = a64 @ b64.T / d + 1.0
        eps = 1.01 * gamma * (np.abs(a64) @ np.abs(b64).T) / d
        cube, move = t ** 3, 3.0 * (np.abs(t) + eps) ** 2 * eps
        if skip:
            np.fill_diagonal(cube, 0.0)
            np.fill_diagonal(move, 0.0)
        return cube.sum(), move.sum() + R.poly3_bound(cube.size) * np.abs(cube).sum()

    (sxx, exx), (syy, eyy), (sxy, exy) = sums(fake, fake, True), sums(real, real, True), sums(fake, real, False)
    want = ((sxx + syy) / (m - 1) - 2 * sxy / m) / m
    tol = ((exx + eyy) / (m - 1) + 2 * exy / m) / m
    print("kid %.9g, restated %.9g, bound %.3e" % (out["kid"], want, tol))
    assert abs(out["kid"] - want) <= tol
