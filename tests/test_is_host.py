"""The Inception Score without a GPU: the float64 restatement (tests/is_restated.py) against hand-worked cases, the
operand conditions and the derived bounds of tests/test_gpu_is.py (asserted before any launch), the header and the workspace query, the
configuration and the wrapper."""
import ctypes
import math

import numpy as np
import pytest

import is_restated as R
from semantic_pyramid_for_image_generation_amd import _lib, config


# ---- the restatement against hand-worked cases ----------------------------------------------------------------------------------------
def test_equal_logit_columns_score_one():
    """Every row predicts the same distribution: p_i = q, KL = 0, IS = 1 - whatever that distribution is."""
    rng = np.random.RandomState(0)
    row = rng.standard_normal(7)
    l = np.tile(row, (30, 1))
    kl = R.kl_splits(l, 3)
    assert np.all(np.abs(kl) <= 1e-15)
    mean, std = R.score_from_kl(kl)
    assert abs(mean - 1.0) <= 1e-15 and std <= 1e-15
    assert np.all(np.abs(R.kl_splits(np.zeros((10, 5)), 2)) <= 1e-15)          # C equal columns: uniform rows


def test_one_hot_rows_over_k_classes_score_k():
    """Rows that are (nearly) one-hot, spread evenly over k of C classes: h -> 0, q -> uniform on k, KL -> log k."""
    k, c, reps = 4, 9, 6
    l = np.full((k * reps, c), -200.0)
    l[np.arange(k * reps), np.arange(k * reps) % k] = 200.0
    for splits in (1, 2, 3):                                                    # 24 rows: every split holds each class equally often
        kl = R.kl_splits(l, splits)
        assert np.all(np.abs(kl - math.log(k)) <= 1e-12), kl
    mean, std = R.score_from_kl(R.kl_splits(l, 2))
    assert abs(mean - k) <= 1e-11 and std <= 1e-11


def test_a_split_of_one_row_has_kl_zero():
    rng = np.random.RandomState(1)
    l = rng.standard_normal((5, 11)) * 3
    assert np.all(np.abs(R.kl_splits(l, 5)) <= 1e-15)                           # q = p: sum p log p - sum p log p
    assert abs(R.kl_splits(l[:1], 1)[0]) <= 1e-15


def test_split_boundaries_follow_the_floor_rule():
    b = R.split_bounds(389, 10)
    assert b == [(s * 389 // 10, (s + 1) * 389 // 10) for s in range(10)]
    assert b[0] == (0, 38) and b[1] == (38, 77) and b[-1] == (350, 389)
    assert sorted({hi - lo for lo, hi in b}) == [38, 39] and sum(hi - lo for lo, hi in b) == 389
    assert R.split_bounds(5, 5) == [(i, i + 1) for i in range(5)]
    # the restatement uses them: moving one row across a boundary changes exactly the two splits next to it
    rng = np.random.RandomState(2)
    l = rng.standard_normal((389, 6)) * 2
    kl = R.kl_splits(l, 10)
    for s, (lo, hi) in enumerate(b):
        assert kl[s] == R.kl_splits(l[lo:hi], 1)[0]


def test_the_population_std_is_used():
    kl = np.log(np.array([1.0, 2.0, 3.0, 6.0]))
    mean, std = R.score_from_kl(kl)
    assert abs(mean - 3.0) <= 1e-15
    assert abs(std - math.sqrt((4 + 1 + 0 + 9) / 4)) <= 1e-15                   # / S, not / (S - 1)
    assert abs(std - np.std(np.exp(kl))) <= 1e-15 and abs(std - np.std(np.exp(kl), ddof=1)) > 0.1
    from semantic_pyramid_for_image_generation_amd import metrics as M
    got = M.inception_score_from_kl(kl)
    assert sorted(got) == ["inception_score", "inception_score_std"]
    assert abs(got["inception_score"] - mean) <= 1e-15 and abs(got["inception_score_std"] - std) <= 1e-15
    assert all(math.isnan(v) for v in M.inception_score_from_kl([0.1, float("nan"), 0.2]).values())


def test_a_non_finite_logit_makes_its_split_nan_and_no_other():
    rng = np.random.RandomState(3)
    l = rng.standard_normal((30, 8))
    clean = R.kl_splits(l, 3)
    for bad in (np.nan, np.inf, -np.inf):
        x = l.copy()
        x[14, 2] = bad                                                          # split 1 of 3: rows 10..19
        kl = R.kl_splits(x, 3)
        assert math.isnan(kl[1]) and kl[0] == clean[0] and kl[2] == clean[2]
        assert all(math.isnan(v) for v in R.score_from_kl(kl))


# ---- exact regime: operands and bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: "%dx%d_d%d" % c)
def test_exact_regime_conditions(case):
    x, w, b, l = R.exact_operands(*case)
    R.check_exact(x, w, b, l)
    # whatever the summation order, fp32 gives the same integers: every partial sum is an integer of magnitude <= 24
    perm = np.random.RandomState(0).permutation(x.shape[1])
    assert np.array_equal((x[:, perm] @ w[:, perm].T + b).astype(np.float64), l)
    if case[1] >= 40:
        peak = R.row_stats(l)[2].max(axis=1).mean()
        score = R.score_from_kl(R.kl_splits(l, 1))[0]
        print("exact %s: mean max p %.2f, IS %.2f" % (case, peak, score))
        assert 0.05 < peak < 0.9 and score > 1.5


def test_check_exact_refuses_other_operands():
    x, w, b, l = R.exact_operands(131, 72, 72)
    with pytest.raises(AssertionError):
        R.check_exact(x + 0.5, w, b, l)
    with pytest.raises(AssertionError):
        R.check_exact(x, w * 2, b, l)
    with pytest.raises(AssertionError):
        R.check_exact(x, w, b + 3, R.logits(x, w, b + 3))


@pytest.mark.parametrize("case,splits", [((389, 1000, 72), 10), ((389, 1000, 2048), 3), ((131, 72, 72), 1), ((5, 72, 72), 5)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_exact_bound_covers_three_summation_orders_and_is_not_vacuous(case, splits):
    """R.kl_exact_bound against a numpy.longdouble evaluation: forward, reversed and per-64-class blocks merged online (the device's
    form) all lie within it - it is twice the float64 terms, so half of it covers each; and it is <= 1e-9."""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than float64 here"
    _, _, _, l = R.exact_operands(*case)
    n, classes = l.shape
    want = R.kl_splits_longdouble(l, splits)
    sizes = [hi - lo for lo, hi in R.split_bounds(n, splits)]
    bound = np.array([R.kl_exact_bound(classes, ns, R.EXACT_LMAX) for ns in sizes])
    assert np.all(bound <= 1e-9) and np.all(bound > 0)
    for order in ("forward", "reversed", "blocks64"):
        got = R.kl_splits_ordered(l, splits, order)
        err = np.abs((got.astype(np.longdouble) - want).astype(np.float64))
        print("%s %s: max |err| %.3e, bound / 2 %.3e" % (case, order, err.max(), bound.min() / 2))
        assert np.all(err <= bound / 2), (order, err.max())
    err = np.abs((R.kl_splits(l, splits).astype(np.longdouble) - want).astype(np.float64))
    assert np.all(err <= bound / 2)
    e_lse, e_h = R.row_exact_bounds(classes, R.EXACT_LMAX)
    assert 0 < e_lse <= 1e-9 and 0 < e_h <= 1e-9
    assert 0 < R.colsum_total_bound(classes, max(sizes), R.EXACT_LMAX) <= 1e-9 * max(sizes)


# ---- general regime -------------------------------------------------------------------------------------------------------------------
def test_general_bound_covers_fp32_logits_and_is_not_vacuous():
    """d = 72: the bound of KL_s from e_ic = 1.01 (gamma_d + 2u)(sum |x| |w| + |b|) covers logits formed by an fp32 matmul, and is at most
    1e-4 KL_s.  (Measured: first order 2.4e-5 on KL = 0.66, actual error 6e-9.)"""
    x, w, b, l, err = R.general_operands()
    l32 = (x @ w.T + b).astype(np.float64)                                      # numpy's fp32 matmul: some order of a length-72 sum
    assert np.all(np.abs(l32 - l) <= err)
    splits = 3
    want, got = R.kl_splits(l, splits), R.kl_splits(l32, splits)
    first, total = R.kl_general_bound(l, err, splits)
    print("general: KL %s, first order %s, total %s, actual %s" % (want, first, total, np.abs(got - want)))
    assert np.all(first <= total) and np.all(total <= 1.05 * first + 1e-8)       # the second-order and float64 terms are small beside it
    assert np.all(np.abs(got - want) <= total)
    assert np.all(total <= 1e-4 * want)
    assert np.all(want > 0.1)                                                   # the rows do differ: nothing like KL = 0
    mean_b, std_b = R.score_bounds(want, total)
    m0, s0 = R.score_from_kl(want)
    m1, s1 = R.score_from_kl(got)
    assert abs(m1 - m0) <= mean_b and abs(s1 - s0) <= std_b and mean_b <= 1e-3


def test_depth_2048_is_left_to_the_exact_regime():
    """At d = 2048 the worst-case gamma makes the general bound some 1e-3 of KL: too loose to hold a kernel to."""
    x, w, b, l, err = R.general_operands(64, 100, 2048, seed=6)
    first, total = R.kl_general_bound(l, err, 1)
    assert total[0] > 1e-4 * R.kl_splits(l, 1)[0]


# ---- header and workspace -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    for name in ("sp_pairset_softmax_workspace", "sp_pairset_lse", "sp_pairset_softmax_colsum"):
        assert name in protos, name
    text = open(_lib.HEADER).read()
    assert "Salimans" in text


def _ws(n, classes, d, splits):
    out = ctypes.c_int64(-1)
    rc = _lib.lib().sp_pairset_softmax_workspace(n, classes, d, splits, ctypes.byref(out))
    return rc, out.value


def _formula(n, classes, splits, forced=None):
    """max(24 n S_c, 8 splits ceil(ceil(n / splits) / 128) classes), S_c = min(CB, max(1, forced or ceil(6144 / RB)))."""
    rb, cb = -(-n // 128), -(-classes // 64)
    segs = min(cb, max(1, forced if forced is not None else -(-6144 // rb)))
    return max(24 * n * segs, 8 * splits * (-(-(-(-n // splits)) // 128)) * classes)


def test_workspace_answers_without_a_gpu_and_matches_the_formula():
    for n, classes, splits in ((2, 3, 1), (5, 72, 5), (131, 72, 1), (389, 1000, 1), (389, 1000, 3), (389, 1000, 10), (389, 40, 10),
                               (6000, 1000, 10), (50000, 1000, 10), (300, 100000, 7), (300, 100000, 300), (1 << 22, 1000, 10)):
        rc, got = _ws(n, classes, 2048, splits)
        assert rc == 0 and got == _formula(n, classes, splits), (n, classes, splits, got)
    assert _ws(6000, 1000, 2048, 10)[1] == 24 * 6000 * 16 == 2304000
    assert _ws(50000, 1000, 2048, 10)[1] == 24 * 50000 * 16 == 19200000          # against 200 MB of fp32 logits
    assert _ws(300, 100000, 2048, 300)[1] == 8 * 300 * 1 * 100000                # many classes and splits: the column partials are the larger part
    sizes = [_ws(n, 1000, 2048, 10)[1] for n in (389, 1000, 6000, 50000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4                       # grows with n


def test_workspace_follows_the_forced_segment_count():
    lib, key = _lib.lib(), _lib.TUNE_KEYS["SP_PAIRSET_SEGMENTS"]
    try:
        sizes = set()
        for forced in (1, 7, 11, 1000):                                          # 1: the column partials are the larger part
            assert lib.sp_set_tuning(key, forced) == 0
            rc, got = _ws(389, 1000, 2048, 3)
            assert rc == 0 and got == _formula(389, 1000, 3, forced), forced
            sizes.add(got)
        assert len(sizes) == 4
    finally:
        lib.sp_set_tuning(key, -1)


def test_workspace_rejects_what_the_kernels_would():
    lib = _lib.lib()
    for n, classes, d, splits in ((5, 0, 64, 1), (5, 10, 64, 0), (5, 10, 64, 6), (0, 10, 64, 1), (5, 10, 0, 1), (5, 10, 64, -1),
                                  (100000, 10, 64, 65536)):
        rc, _ = _ws(n, classes, d, splits)
        assert rc != 0, (n, classes, d, splits)
        assert b"sp_pairset_softmax_workspace" in lib.sp_last_error_string()
    assert lib.sp_pairset_softmax_workspace(5, 10, 64, 1, None) != 0
    assert _ws(5, 10, 64, 5)[0] == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every check below fails on the host (NULL pointers, n < splits, ld < d, a short workspace): nothing is launched, so it runs
    without a GPU; each failure carries a message."""
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    big = 1 << 20
    bad_lse = [(None, 4, 8, a, 3, 8, a, 8, a, a, a, big), (a, 4, 8, None, 3, 8, a, 8, a, a, a, big), (a, 4, 8, a, 3, 8, None, 8, a, a, a, big),
               (a, 4, 8, a, 3, 8, a, 8, None, a, a, big), (a, 4, 8, a, 3, 8, a, 8, a, None, a, big), (a, 4, 8, a, 3, 8, a, 8, a, a, None, big),
               (a, 4, 8, a, 0, 8, a, 8, a, a, a, big),             # classes < 1
               (a, 4, 8, a, 3, 8, a, 0, a, a, a, big),             # d < 1
               (a, 4, 8, a, 3, 8, a, 12, a, a, a, big),            # ld < d
               (a, 4, 8, a, 3, 4, a, 8, a, a, a, big),             # ldw < d
               (a, 4, 8, a, 3, 8, a, 8, a, a, a, 24 * 4 - 1)]      # a short workspace (one segment: 24 n bytes)
    for args in bad_lse:
        assert lib.sp_pairset_lse(*args, None) != 0, args
        assert b"sp_pairset_lse" in lib.sp_last_error_string()
    ok = (a, 4, 8, a, 3, 8, a, 8, a, a)
    bad_col = [ok + (0, a, a, a, big), ok + (5, a, a, a, big),      # splits < 1, n < splits
               ok + (2, None, a, a, big), ok + (2, a, None, a, big), ok + (2, a, a, None, big),
               ok + (2, a, a, a, 8 * 2 * 1 * 3 - 1),               # a short workspace
               (a, 4, 8, a, 3, 8, a, 8, None, a, 2, a, a, a, big), (a, 4, 8, a, 3, 8, a, 8, a, None, 2, a, a, a, big),
               (a, 4, 8, a, 3, 8, a, 12, a, a, 2, a, a, a, big)]   # ld < d
    for args in bad_col:
        assert lib.sp_pairset_softmax_colsum(*args, None) != 0, args
        assert b"sp_pairset_softmax_colsum" in lib.sp_last_error_string()


# ---- configuration, the extractor and the wrapper ---------------------------------------------------------------------------------------
def test_metrics_parsing_knows_is(monkeypatch):
    assert config.METRIC_NAMES == ("kid", "prdc", "is")
    assert config.parse_metrics("is, kid") == ("kid", "is") and config.parse_metrics("is") == ("is",)
    assert config.parse_metrics(["is", "prdc", "kid"]) == ("kid", "prdc", "is")
    with pytest.raises(ValueError):
        config.parse_metrics("inception_score")
    monkeypatch.setenv("SP_METRICS", "is")
    assert config.Config.from_env().metrics == "is"
    monkeypatch.setenv("SP_METRICS", "is,prdc")
    assert config.Config.from_env().metrics == "prdc,is"


def _wrapper(**kw):
    import semantic_pyramid_for_image_generation_amd as sp
    return sp.ModelWrapper(sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8), None, [("never", "read", [])],
                           vgg16=sp.VGG16(), save_data_path=None, **kw)


def test_wrapper_without_weights_reports_nan_under_the_new_keys(monkeypatch):
    monkeypatch.setattr(config.CFG, "inception_weights", "")
    mw = _wrapper(metrics="is")
    assert mw.metrics == ("is",) and mw.metrics_is_splits == 10 and mw.metrics_nearest_k == 5
    assert mw.logger.hyperparameter["metrics"] == "is"
    out = mw.evaluate()
    assert set(out) == {"fid", "inception_score", "inception_score_std"}
    assert all(math.isnan(v) for v in out.values()) and mw.last_metrics == pytest.approx(out, nan_ok=True)
    assert math.isnan(mw.validate()) and mw.generator.training
    out = _wrapper(metrics="kid,prdc,is").evaluate()
    assert sorted(out) == ["coverage", "density", "fid", "inception_score", "inception_score_std", "kid", "precision", "recall"]
    monkeypatch.setattr(config.CFG, "metrics", "is")
    assert _wrapper().metrics == ("is",)


def test_extractor_keeps_the_classifier_head_when_it_is_there():
    import torch
    import inception_restated as IR
    from semantic_pyramid_for_image_generation_amd import inception as I
    from semantic_pyramid_for_image_generation_amd._lib import SempyrError
    sd = IR.synth_state_dict(4)
    head = I.classifier_head(sd)
    assert head[0].shape == (1000, 2048) and head[1].shape == (1000,) and head[0].dtype == head[1].dtype == torch.float32
    assert torch.equal(head[0], sd["fc.weight"]) and head[0].is_contiguous()
    assert "fc" not in I.fold_state_dict(sd)                                    # the convolution table still skips it
    net = I.InceptionV3Features(sd, dtype=torch.bfloat16)
    got = net.classifier_head("cpu")
    assert got[0].dtype == torch.float32 and torch.equal(got[0], sd["fc.weight"]) and torch.equal(got[1], sd["fc.bias"])
    assert net.classifier_head("cpu") is got                                    # uploaded once per device
    bare = IR.synth_state_dict(4, with_fc=False)
    assert I.classifier_head(bare) is None
    assert I.InceptionV3Features(bare, dtype=torch.float32).classifier_head("cpu") is None      # and the FID still has its extractor
    for key, shape in (("fc.weight", (1008, 2048)), ("fc.weight", (1000, 2047)), ("fc.bias", (1008,))):
        wrong = dict(sd)
        wrong[key] = torch.zeros(shape)
        with pytest.raises(SempyrError, match=key.replace(".", r"\.")):
            I.InceptionV3Features(wrong, dtype=torch.float32)
    half = dict(sd)
    del half["fc.bias"]
    with pytest.raises(SempyrError, match=r"fc\.bias"):
        I.classifier_head(half)


def test_compute_names_the_missing_head():
    from semantic_pyramid_for_image_generation_amd import metrics as M
    from semantic_pyramid_for_image_generation_amd._lib import SempyrError
    x = np.zeros((4, 8), dtype=np.float32)
    with pytest.raises(SempyrError, match=r"fc\.weight"):
        M.compute(x, x, "is")
    assert M.IS_KEYS == ("inception_score", "inception_score_std")
