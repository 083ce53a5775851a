"""KID and precision / recall / density / coverage without a GPU: the header and the workspace query, the float64
restatement (tests/metrics_restated.py) against hand-worked cases, the operand conditions of tests/test_gpu_metrics.py, asserted
before any launch, and the configuration."""
import ctypes
import math
import re

import numpy as np
import pytest

import metrics_restated as R
from semantic_pyramid_for_image_generation_amd import _lib, config


# ---- header and workspace ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_key():
    protos = _lib.parse_header()
    for name in ("sp_pairset_workspace", "sp_pairset_knn", "sp_pairset_cover", "sp_pairset_poly3"):
        assert name in protos, name
    text = open(_lib.HEADER).read()
    assert re.search(r"SP_TUNE_PAIRSET_SEGMENTS\s*=\s*\d+", text)
    assert "SP_PAIRSET_SEGMENTS" in _lib.TUNE_KEYS
    for cite in ("Binkowski", "Kynkaanniemi", "Naeem"):
        assert cite in text, cite


def _ws(na, nb, d, k):
    out = ctypes.c_int64(-1)
    rc = _lib.lib().sp_pairset_workspace(na, nb, d, k, ctypes.byref(out))
    return rc, out.value


def _formula(na, nb, k, forced=None):
    """round8(4 (na + nb)) + max(round8(4 na S k), 8 RB CB), RB = ceil(na / 128), CB = ceil(nb / 64),
    S = min(CB, max(1, forced or ceil(6144 / RB)))."""
    r8 = lambda v: (v + 7) // 8 * 8                                          # noqa: E731
    rb, cb = -(-na // 128), -(-nb // 64)
    s = min(cb, max(1, forced if forced is not None else -(-6144 // rb)))
    return r8(4 * (na + nb)) + max(r8(4 * na * s * k), 8 * rb * cb)


def test_workspace_answers_without_a_gpu_and_matches_the_formula():
    for na, nb, k in ((2, 2, 1), (129, 131, 16), (389, 389, 5), (389, 421, 0), (6000, 6000, 5), (50000, 50000, 5), (1000, 1000, 0),
                      (1, 130, 0), (130, 1, 0)):
        rc, got = _ws(na, nb, 2048, k)
        assert rc == 0 and got == _formula(na, nb, k), (na, nb, k, got)
    assert _ws(50000, 50000, 2048, 5)[1] < 32 << 20                           # megabytes, not the 10 GB of the matrix


def test_workspace_follows_the_forced_segment_count():
    lib, key = _lib.lib(), _lib.TUNE_KEYS["SP_PAIRSET_SEGMENTS"]
    try:
        for forced in (1, 3, 7, 1000):
            assert lib.sp_set_tuning(key, forced) == 0
            rc, got = _ws(389, 389, 2048, 5)
            assert rc == 0 and got == _formula(389, 389, 5, forced), forced
        sizes = set()
        for forced in (1, 3, 7):
            lib.sp_set_tuning(key, forced)
            sizes.add(_ws(389, 389, 2048, 5)[1])
        assert len(sizes) == 3
    finally:
        lib.sp_set_tuning(key, -1)


def test_workspace_rejects_what_the_kernels_would():
    lib = _lib.lib()
    for na, nb, d, k in ((100, 100, 64, 17), (100, 5, 64, 5), (100, 5, 64, 6), (0, 5, 64, 1), (5, 0, 64, 0), (5, 5, 0, 1), (5, 5, 64, -1)):
        rc, _ = _ws(na, nb, d, k)
        assert rc != 0, (na, nb, d, k)
        assert b"sp_pairset_workspace" in lib.sp_last_error_string()
    assert lib.sp_pairset_workspace(5, 5, 64, 1, None) != 0
    assert _ws(100, 6, 64, 5)[0] == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every check below fails on the host (NULL sets, k against the row count, no workspace): nothing is launched, so it runs
    without a GPU; each failure carries a message."""
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    assert lib.sp_pairset_knn(None, 4, 8, a, 4, 8, 8, 1, 0, a, a, 1 << 20, None) != 0
    for k, same in ((4, 0), (5, 0), (3, 1), (17, 0), (0, 0)):                  # k >= nb; k >= nb - 1 when same; k outside [1, 16]
        assert lib.sp_pairset_knn(a, 4, 8, a, 4, 8, 8, k, same, a, a, 1 << 20, None) != 0, (k, same)
        assert b"sp_pairset_knn" in lib.sp_last_error_string()
    assert lib.sp_pairset_knn(a, 4, 8, a, 4, 8, 8, 1, 0, a, a, 8, None) != 0                                  # workspace too small
    assert lib.sp_pairset_knn(a, 4, 6, a, 4, 6, 6, 1, 0, a, a, 1 << 20, None) != 0                            # ld % 4
    assert lib.sp_pairset_cover(a, 4, 8, a, 4, 8, 8, None, None, None, None, None, None, a, 1 << 20, None) != 0   # no output
    assert lib.sp_pairset_cover(a, 4, 8, a, 4, 8, 8, None, None, a, None, None, None, a, 1 << 20, None) != 0      # row_count without rad_b
    assert b"sp_pairset_cover" in lib.sp_last_error_string()
    assert lib.sp_pairset_poly3(a, 4, 8, None, a, 4, 8, None, 8, 2, 4, 0, a, a, 1 << 20, None) != 0           # two subsets, no tables
    assert lib.sp_pairset_poly3(a, 4, 8, None, a, 4, 8, None, 8, 1, 5, 0, a, a, 1 << 20, None) != 0           # m beyond the rows
    assert lib.sp_pairset_poly3(a, 4, 8, None, a, 4, 8, None, 8, 1, 4, 0, a, None, 0, None) != 0              # no workspace
    assert b"sp_pairset_poly3" in lib.sp_last_error_string()


# ---- the restatement against hand-worked cases --------------------------------------------------------------------------------------
def _line(*xs):
    out = np.zeros((len(xs), 4))
    out[:, 0] = xs
    return out


def test_radii_of_points_on_a_line():
    x = _line(0, 1, 3, 7)
    assert R.radii(x, 1).tolist() == [1, 1, 4, 16]
    assert R.radii(x, 2).tolist() == [9, 4, 9, 36]
    assert R.radii(x, 1, R.sqdist_gram).tolist() == [1, 1, 4, 16]
    d = R.sqdist(x, _line(2, 10))
    assert d.tolist() == [[4, 100], [1, 81], [1, 49], [25, 9]]
    assert R.kth_smallest(d, 1).tolist() == [4, 1, 1, 9]


def test_a_fake_exactly_on_a_radius_counts():
    """Closed balls: f = 2 lies at squared distance 1 from r = 1 (radius 1: ON it) and 1 from r = 3 (radius 4: inside)."""
    real, fake = _line(0, 1, 3, 7), _line(2)
    fake3 = _line(2, 2.5, 20)                                    # 2.5 is in r = 3's ball only, 20 in none
    out = R.prdc(real, fake3, nearest_k=1)
    assert out["precision"] == 2 / 3
    assert out["density"] == (2 + 1 + 0) / (1 * 3)               # with < instead of <= the first fake would count once, not twice
    row_count, col_count, row_min, col_min = R.cover(R.sqdist(fake, real), rad_b=R.radii(real, 1))
    assert row_count.tolist() == [2] and col_count is None
    assert row_min.tolist() == [1] and col_min.tolist() == [4, 1, 1, 25]


def test_a_duplicate_row_is_a_neighbour_at_distance_zero():
    x = _line(0, 0, 5)
    assert R.radii(x, 1).tolist() == [0, 0, 25]                  # the self entry is excluded by index, not by value
    x3 = _line(4, 4, 4, 9)
    assert R.radii(x3, 2).tolist() == [0, 0, 0, 25]


def test_identical_sets_score_one():
    rng = np.random.RandomState(3)
    x = np.maximum(rng.standard_normal((40, 12)), 0)
    out = R.prdc(x, x.copy(), nearest_k=3)
    assert out["precision"] == out["recall"] == out["coverage"] == 1.0
    assert out["density"] >= 1.0                                 # every row holds itself and its 3 nearest: >= k + 1 ... / k


def test_recall_and_coverage_tell_fewer_kinds_from_worse_samples():
    real = _line(0, 1, 10, 11)
    fake = _line(0.3, 0.7, 0.5, 0.6)                             # good samples of ONE of the two modes
    out = R.prdc(real, fake, nearest_k=1)
    assert out["precision"] == 1.0 and out["coverage"] == 0.5 and out["recall"] == 0.0


def test_kid_of_a_hand_computed_case():
    """x (fake) = (1,0), (0,1), (1,1); y (real) = (2,0), (0,2), (0,0); d = 2, k = (u.v / 2 + 1)^3.
    x Gram off the diagonal: 1, 3.375, 3.375 twice = 15.5; y: 1, 1, 1 twice = 6; x.y: 8 + 1 + 1 + 1 + 8 + 1 + 8 + 8 + 1 = 37.
    t = (15.5 + 6) / 2 - 2 * 37 / 3; KID = t / 1 / 3.  m = N: every subset is a permutation, the sums do not depend on it."""
    fake = np.array([[1, 0], [0, 1], [1, 1]], dtype=np.float64)
    real = np.array([[2, 0], [0, 2], [0, 0]], dtype=np.float64)
    assert R.poly3_sum(fake, fake, True) == 15.5 and R.poly3_sum(real, real, True) == 6.0 and R.poly3_sum(fake, real) == 37.0
    want = ((15.5 + 6.0) / 2 - 2 * 37.0 / 3) / 3
    for subsets in (1, 4):
        assert abs(R.kid(real, fake, num_subsets=subsets, max_subset_size=1000, seed=0) - want) <= 1e-15 * abs(want) * 8


def test_kid_draw_order_is_pinned():
    """Per subset the fake rows are drawn first, then the real rows, from ONE RandomState(seed); int32 tables."""
    from semantic_pyramid_for_image_generation_amd import metrics as M
    ix, iy, m = R.kid_indices(7, 9, num_subsets=3, max_subset_size=5, seed=11)
    assert m == 5 and ix.dtype == iy.dtype == np.int32 and ix.shape == iy.shape == (3, 5)
    rs = np.random.RandomState(11)
    for s in range(3):
        assert ix[s].tolist() == rs.choice(9, 5, replace=False).tolist()          # x: fake rows (9 of them)
        assert iy[s].tolist() == rs.choice(7, 5, replace=False).tolist()          # y: real rows
    px, py, pm = M.kid_indices(7, 9, 3, 5, 11)
    assert pm == m and np.array_equal(px, ix) and np.array_equal(py, iy) and px.dtype == np.int32
    # m = 2 of 3 rows, two subsets: the restatement follows the tables
    fake = np.array([[1, 0], [0, 1], [1, 1]], dtype=np.float64)
    real = np.array([[2, 0], [0, 2], [0, 0]], dtype=np.float64)
    jx, jy, _ = R.kid_indices(3, 3, 2, 2, 0)
    t = 0.0
    for s in range(2):
        x, y = fake[jx[s]], real[jy[s]]
        k = lambda u, v: (u @ v / 2 + 1) ** 3                                     # noqa: E731
        t += (k(x[0], x[1]) * 2 + k(y[0], y[1]) * 2) / 1 - 2 * sum(k(u, v) for u in x for v in y) / 2
    assert abs(R.kid(real, fake, 2, 2, 0) - t / 2 / 2) <= 1e-14 * abs(t)


# ---- operand conditions of the GPU tests ------------------------------------------------------------------------------------------
def test_exact_regime_conditions():
    """d * amax^2 <= 2^22: every norm, every dot and (na + nb) - 2 dot in any association is an integer below 2^24."""
    for na, nb, d, amax, signed in R.EXACT_CASES:
        a, b = R.exact_sets(na, nb, d, amax, signed, seed=na + d)
        R.check_exact(a, b)
        dist = R.sqdist_gram(a, b)
        assert np.array_equal(dist, np.round(dist)) and dist.max() < 2 ** 24 and dist.min() >= 0
        assert np.array_equal(dist, R.sqdist(a, b))
    with pytest.raises(AssertionError):
        R.check_exact(np.full((2, 2048), 46, dtype=np.float32))                   # 2048 * 46^2 > 2^22
    with pytest.raises(AssertionError):
        R.check_exact(np.full((2, 8), 0.5, dtype=np.float32))


def test_general_regime_bracket_is_open_for_few_rows_and_columns():
    """The bound e_ij = 1.01 (gamma + 3u) S_ij brackets every count; the inputs of the GPU test leave the bracket open (lo != hi) for at
    most 2 % of the rows and 2 % of the columns (0.5 - 0.8 % at d = 72)."""
    g = R.general_case()
    for name in ("row", "col"):
        lo, hi = g[name + "_lo"], g[name + "_hi"]
        assert np.all(lo <= g[name + "_count"]) and np.all(g[name + "_count"] <= hi)
        assert (lo != hi).mean() <= 0.02, (name, (lo != hi).mean())
    assert g["err"].max() < 1e-3 * g["dist"].mean()


# ---- configuration and the wrapper ---------------------------------------------------------------------------------------------------
def test_metrics_parsing(monkeypatch):
    assert config.parse_metrics("") == () and config.parse_metrics(None) == ()
    assert config.parse_metrics("kid") == ("kid",) and config.parse_metrics(" prdc , kid ") == ("kid", "prdc")
    assert config.parse_metrics(["prdc"]) == ("prdc",)
    with pytest.raises(ValueError):
        config.parse_metrics("kid,fid2")
    assert config.Config().metrics == ""
    monkeypatch.setenv("SP_METRICS", "prdc,kid")
    assert config.Config.from_env().metrics == "kid,prdc"
    monkeypatch.setenv("SP_METRICS", "inception_score")
    with pytest.raises(ValueError):
        config.Config.from_env()
    monkeypatch.delenv("SP_METRICS")
    assert config.Config.from_env().metrics == ""


def _wrapper(**kw):
    import semantic_pyramid_for_image_generation_amd as sp
    return sp.ModelWrapper(sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8), None, [("never", "read", [])],
                           vgg16=sp.VGG16(), save_data_path=None, **kw)


def test_wrapper_keyword_config_and_errors(monkeypatch):
    monkeypatch.setattr(config.CFG, "inception_weights", "")
    mw = _wrapper()
    assert mw.metrics == () and mw.last_metrics is None
    assert math.isnan(mw.validate()) and mw.last_metrics is None             # off: validate() is what it was
    with pytest.raises(ValueError):
        _wrapper(metrics="kid,precision")
    monkeypatch.setattr(config.CFG, "metrics", "prdc")
    assert _wrapper().metrics == ("prdc",)
    assert _wrapper(metrics="").metrics == ()                                # the keyword wins over the configuration
    mw = _wrapper(metrics="kid,prdc")
    assert mw.metrics == ("kid", "prdc") and mw.logger.hyperparameter["metrics"] == "kid,prdc"
    assert math.isnan(mw.validate()) and math.isnan(mw.validate(device="cuda"))      # without weights: still nan
    out = mw.evaluate()
    assert sorted(out) == ["coverage", "density", "fid", "kid", "precision", "recall"]
    assert all(math.isnan(v) for v in out.values()) and mw.last_metrics == pytest.approx(out, nan_ok=True)
    assert mw.generator.training
