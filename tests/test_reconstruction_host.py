"""Host-side tests of the reconstruction-fidelity feature: the float64 restatement against hand-worked cases,
the conditions its derived bound must meet, the parsers, the C ABI's answers and refusals (no GPU needed), the wrapper option."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reconstruction_restated as R  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib, config  # noqa: E402

C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
# the shapes and scale counts of tests/test_gpu_reconstruction.py
CASES = (((2, 3, 44, 52), 3), ((3, 1, 76, 44), 2), ((1, 2, 176, 208), 5))


# ---- the restatement against hand-worked cases ----------------------------------------------------------------------------------------
def test_window_is_the_pinned_one():
    g = R.window()
    assert g.shape == (11,) and (g == g[::-1]).all() and abs(g.sum() - 1) < 1e-7
    assert (g.astype(np.float32).astype(np.float64) == g).all()               # fp32 numbers
    assert abs(g[5] / g[4] - math.exp(1 / 4.5)) < 1e-6                        # sigma 1.5


def test_identical_images_score_one_and_psnr_is_inf():
    x, _ = R.family("noise", (2, 3, 44, 52))
    st = R.stats(x, x, 3)
    assert np.abs(st["ssim_mean"] - 1).max() < 1e-12 and np.abs(st["cs_mean"] - 1).max() < 1e-12
    assert (st["sqerr"] == 0).all() and np.isposinf(R.psnr(st["sqerr"], 44 * 52)).all()


def test_negated_image_on_a_zero_mean_window():
    """One valid position (an 11 x 11 plane) of a point-antisymmetric plane: the window is symmetric, so mx = 0, l = 1 and
    ssim = cs = (C2 - 2 exx) / (C2 + 2 exx).  And on any plane: cs = (C2 - 2 sxx) / (C2 + 2 sxx), l = (C1 - 2 mx^2) / (C1 + 2 mx^2)."""
    rng = np.random.default_rng(3)
    half = rng.uniform(-0.5, 0.5, (11, 11))
    x = (half - half[::-1, ::-1]).astype(np.float32)[None, None]           # rounding keeps the antisymmetry
    g = R.window()
    exx = float(np.einsum("i,j,ij->", g, g, x[0, 0].astype(np.float64) ** 2))
    st = R.stats(x, -x, 1)
    want = (C2 - 2 * exx) / (C2 + 2 * exx)
    assert abs(st["cs_mean"][0, 0, 0] - want) < 1e-12 and abs(st["ssim_mean"][0, 0, 0] - want) < 1e-12
    x, _ = R.family("smooth", (1, 1, 30, 34))
    x = x + np.float32(0.125)
    cs, ssim, _, _ = R.maps(x, -x)
    mx = R.filt(x, g)
    sxx = R.filt(x.astype(np.float64) ** 2, g) - mx * mx
    assert np.abs(cs - (C2 - 2 * sxx) / (C2 + 2 * sxx)).max() < 1e-12
    assert np.abs(ssim / cs - (C1 - 2 * mx * mx) / (C1 + 2 * mx * mx)).max() < 1e-12


def test_a_constant_offset_changes_l_only():
    x, _ = R.family("noise", (1, 2, 30, 34))
    d = 0.25
    y = x.astype(np.float64) + d                                               # maps() takes float64 planes as they are
    cs, ssim, _, _ = R.maps(x, y)
    g = R.window()
    mx, s2 = R.filt(x, g), g.sum() ** 2                  # the fp32 taps sum to 1 within 2^-22 only: the offset's windowed mean is d s2
    # sxy = sxx + d mx (1 - s2), syy = sxx + (2 d mx + d^2 s2) (1 - s2): cs = 1 up to (1 - s2) (2 |d mx| + d^2) / C2 < 1e-6
    assert abs(1 - s2) < 2.0 ** -21 and np.abs(cs - 1).max() < 1e-6
    want_l = (2 * mx * (mx + d * s2) + C1) / (mx * mx + (mx + d * s2) ** 2 + C1)
    assert np.abs(ssim / cs - want_l).max() < 1e-12
    assert np.abs(want_l - 1).min() > 0.1                # ... and l is what moved


def test_psnr_of_a_known_mse():
    x = np.zeros((2, 3, 16, 12), dtype=np.float32)
    y = np.full_like(x, 0.5)
    y[1] = 0.125
    d = (x - y).astype(np.float64)
    sqerr = (d * d).sum(axis=(-2, -1))
    assert (sqerr[0] == 0.25 * 16 * 12).all()
    got = R.psnr(sqerr, 16 * 12)
    assert abs(got[0] - 10 * math.log10(4 / 0.25)) < 1e-12 and abs(got[1] - 10 * math.log10(4 / 0.015625)) < 1e-12


def test_ms_ssim_of_equal_scales_is_a_power():
    t = 0.83
    st = {"ssim_mean": np.full((2, 3, 5), t), "cs_mean": np.full((2, 3, 5), t),
          "bound_ssim": np.full((2, 3, 5), 1e-6), "bound_cs": np.full((2, 3, 5), 1e-6)}
    got, bound = R.ms_ssim(st)
    assert np.abs(got - t ** sum(R.MS_SSIM_WEIGHTS)).max() < 1e-14
    assert abs(sum(R.MS_SSIM_WEIGHTS) - 1.0001) < 1e-12
    first_order = got * sum(R.MS_SSIM_WEIGHTS) * 1e-6 / t                              # d(t^W) = W t^(W-1) dt
    assert (bound >= first_order * (1 - 1e-5)).all() and (bound <= first_order * (1 + 1e-5) + 1e-14).all()
    st["cs_mean"][:, :, 1] = -0.25                                                     # a clamped factor: the score is 0, the bound stays finite
    got, bound = R.ms_ssim(st)
    assert (got == 0).all() and (bound < 1e-13).all()
    st["cs_mean"][:, :, 1] = 5e-7                                                      # a factor inside its own bound of 0
    got, bound = R.ms_ssim(st)
    assert (bound >= got).all() and (bound < 0.05).all()


def test_pooling_rule_on_a_4x4_example():
    x = np.arange(16, dtype=np.float32).reshape(1, 1, 4, 4)
    assert (R.pool2(x)[0, 0] == np.array([[2.5, 4.5], [10.5, 12.5]], dtype=np.float32)).all()
    # the rule's order is part of it: ((a + b) + (c + d)) * 0.25 in fp32, here where another order rounds differently
    a, b, c, d = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    x = np.array([[a, b], [c, d]], dtype=np.float32)[None, None]
    assert R.pool2(x)[0, 0, 0, 0] == ((a + b) + (c + d)) * np.float32(0.25)
    assert R.pool2(x).dtype == np.float32


# ---- the conditions on the bound -------------------------------------------------------------------------------------------------------
def detection_distance(x, y, scales, variant):
    """Per scale: the largest move of an output (over planes and the two means) under a wrong variant, in units of THAT output's bound.
    A kernel computing the variant is caught at a scale when one output leaves its bound there."""
    st, sv = R.stats(x, y, scales), R.stats(x, y, scales, **variant)
    return np.maximum(np.abs(sv["ssim_mean"] - st["ssim_mean"]) / st["bound_ssim"],
                      np.abs(sv["cs_mean"] - st["cs_mean"]) / st["bound_cs"]).max(axis=(0, 1))


def check_bound_conditions(cases=CASES):
    """Asserted here and again by the GPU test before any launch (it imports this).  Returns the printed lines."""
    lines = []
    for shape, scales in cases:
        for name in R.FAMILIES:
            x, y = R.family(name, shape)
            st = R.stats(x, y, scales)
            worst = np.maximum(st["bound_ssim"], st["bound_cs"]).max(axis=(0, 1))
            lines.append("%s %-9s bound per scale %s" % (shape, name, " ".join("%.2e" % b for b in worst)))
            if name not in R.BOUNDED:
                continue                                                       # flat-dark: kept as a case, its bound printed, not capped
            assert (worst <= R.BOUND_CAP).all(), (shape, name, worst)
            for vname, variant in R.VARIANTS.items():
                dist = detection_distance(x, y, scales, variant)               # the smaller family decides: both are asserted
                lines.append("    %-18s moves the result by %s bounds" % (vname, " ".join("%.0f" % v for v in dist)))
                assert (dist > 10).all(), (shape, name, vname, dist)
    return lines


def test_bound_is_tight_where_it_must_be_and_wrong_variants_leave_it():
    print("\n".join(check_bound_conditions()))


def test_bound_holds_for_an_fp32_evaluation_on_the_host():
    """An fp32 numpy evaluation of the definition (separable, population form) stays inside the bound: the bound is not too small for
    the arithmetic it was derived for.  (Not the device's order of operations - the GPU test holds the kernel to it.)"""
    g = R.window().astype(np.float32)

    def filt32(v):
        h, w = v.shape[-2] - 10, v.shape[-1] - 10
        t = np.zeros(v.shape[:-1] + (w,), dtype=np.float32)
        for k in range(11):
            t = t + g[k] * v[..., :, k:k + w]
        o = np.zeros(v.shape[:-2] + (h, w), dtype=np.float32)
        for k in range(11):
            o = o + g[k] * t[..., k:k + h, :]
        return o
    for name in R.FAMILIES:
        x, y = R.family(name, (2, 3, 44, 52))
        st = R.stats(x, y, 1)
        mx, my = filt32(x), filt32(y)
        sxx, syy, sxy = filt32(x * x) - mx * mx, filt32(y * y) - my * my, filt32(x * y) - mx * my
        cs = (2 * sxy + np.float32(C2)) / (sxx + syy + np.float32(C2))
        ssim = (2 * mx * my + np.float32(C1)) / (mx * mx + my * my + np.float32(C1)) * cs
        assert cs.dtype == np.float32
        assert (np.abs(cs.astype(np.float64).mean(axis=(-2, -1)) - st["cs_mean"][:, :, 0]) <= st["bound_cs"][:, :, 0]).all(), name
        assert (np.abs(ssim.astype(np.float64).mean(axis=(-2, -1)) - st["ssim_mean"][:, :, 0]) <= st["bound_ssim"][:, :, 0]).all(), name


def test_dyadic_pair_is_exact():
    x, y, exact = R.dyadic_pair((2, 3, 44, 52))
    assert (x * 256 == np.round(x * 256)).all() and np.abs(x).max() <= 1
    assert (R.stats(x, y, 1)["sqerr"] == exact).all()


# ---- parsing ---------------------------------------------------------------------------------------------------------------------------
def test_reconstruction_parsing(monkeypatch):
    assert config.parse_reconstruction("") == () and config.parse_reconstruction(None) == ()
    assert config.parse_reconstruction(" ms_ssim , psnr ") == ("psnr", "ms_ssim")
    assert config.parse_reconstruction(["ssim"]) == ("ssim",)
    assert config.parse_reconstruction("psnr,ssim,ms_ssim") == config.RECONSTRUCTION_NAMES == ("psnr", "ssim", "ms_ssim")
    with pytest.raises(ValueError):
        config.parse_reconstruction("psnr,lpips")
    assert config.Config().reconstruction == "" and config.Config().reconstruction_levels == "0-6"
    monkeypatch.setenv("SP_RECONSTRUCTION", "ssim,psnr")
    assert config.Config.from_env().reconstruction == "psnr,ssim"
    monkeypatch.setenv("SP_RECONSTRUCTION", "fid")
    with pytest.raises(ValueError):
        config.Config.from_env()
    monkeypatch.delenv("SP_RECONSTRUCTION")
    assert config.Config.from_env().reconstruction == ""


def test_levels_parsing(monkeypatch):
    assert config.parse_levels("0-6") == (0, 1, 2, 3, 4, 5, 6) == config.parse_levels(None) == config.parse_levels("")
    assert config.parse_levels("0,3,6") == (0, 3, 6) and config.parse_levels(" 4-5, 0 ,5") == (0, 4, 5)
    assert config.parse_levels([6, 0]) == (0, 6) and config.parse_levels("3") == (3,)
    for bad in ("0-7", "7", "-1", "a", "3-1", "0--2", "1,,2", "0-2-4", [0, 7], [1.5], 3):
        with pytest.raises(ValueError):
            config.parse_levels(bad)
    monkeypatch.setenv("SP_RECONSTRUCTION_LEVELS", "0,6")
    assert config.Config.from_env().reconstruction_levels == "0,6"
    monkeypatch.setenv("SP_RECONSTRUCTION_LEVELS", "0-9")
    with pytest.raises(ValueError):
        config.Config.from_env()
    monkeypatch.delenv("SP_RECONSTRUCTION_LEVELS")
    assert config.Config.from_env().reconstruction_levels == "0-6"


def test_metric_names_and_the_table_are_as_they_were():
    assert config.METRIC_NAMES == ("kid", "prdc", "is")
    for word in ("SP_RECONSTRUCTION ", "SP_RECONSTRUCTION_LEVELS"):
        assert word in config.__doc__, word


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    assert len(protos["sp_ssim_workspace"][1]) == 6 and len(protos["sp_ssim_stats"][1]) == 24
    assert protos["sp_ssim_stats"][1][17] is ctypes.c_double                   # data_range
    text = open(_lib.HEADER).read()
    for cite in ("Wang, Bovik", "Wang, Simoncelli", "reconstruction.hip"):
        assert cite in text, cite


def _ws(n, c, h, w, scales):
    out = ctypes.c_int64(-1)
    rc = _lib.lib().sp_ssim_workspace(n, c, h, w, scales, ctypes.byref(out))
    return rc, out.value


def _formula(n, c, h, w, scales):
    """include/sempyr.h: sum_{j >= 1} 2 round8(4 P H_j W_j) + 8 P (T_0 + 2 sum_j T_j), T_j = ceil((H_j - 10) / 16) ceil((W_j - 10) / 32)."""
    r8 = lambda v: (v + 7) // 8 * 8                                            # noqa: E731
    tiles = lambda j: -(-((h >> j) - 10) // 16) * -(-((w >> j) - 10) // 32)    # noqa: E731
    p = n * c
    return sum(2 * r8(4 * p * (h >> j) * (w >> j)) for j in range(1, scales)) + 8 * p * (tiles(0) + 2 * sum(tiles(j) for j in range(scales)))


def test_workspace_answers_without_a_gpu_and_matches_the_formula():
    for args in ((1, 1, 11, 11, 1), (2, 3, 44, 52, 3), (3, 1, 76, 44, 2), (1, 2, 176, 208, 5), (40, 3, 256, 256, 5), (40, 3, 256, 256, 1),
                 (1, 3, 22, 26, 2)):
        rc, got = _ws(*args)
        assert rc == 0 and got == _formula(*args), (args, got)
    assert _ws(1, 1, 11, 11, 1)[1] == 8 * 3


def test_workspace_refusals():
    lib = _lib.lib()
    for args in ((0, 3, 44, 52, 1), (2, 0, 44, 52, 1), (2, 3, 10, 52, 1), (2, 3, 44, 10, 1), (2, 3, 44, 52, 0), (2, 3, 44, 52, 6),
                 (2, 3, 44, 52, 4),            # 44 / 8 is no integer
                 (2, 3, 40, 48, 3),            # 40 / 4 = 10 < 11
                 (2, 3, 176, 160, 5),          # 160 / 16 = 10 < 11
                 (2, 3, 45, 52, 2), (1 << 13, 1 << 12, 44, 52, 1), (2, 3, 32784, 52, 1), (-1, 3, 44, 52, 1)):
        rc, _ = _ws(*args)
        assert rc == -1, args
        assert b"sp_ssim_workspace" in lib.sp_last_error_string(), args
    assert lib.sp_ssim_workspace(2, 3, 44, 52, 1, None) == -1


def test_stats_refuses_bad_arguments_before_any_launch():
    """Every refusal the header lists, called without a GPU: each returns SP_ERR_INVALID with a message; nothing is launched (a launch
    without a device would come back as SP_ERR_LAUNCH, -2)."""
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    F32, BF16, F16 = _lib.SP_F32, _lib.SP_BF16, _lib.SP_F16
    big = 1 << 30

    def call(x=a, xd=F32, xs=(3 * 44 * 52, 44 * 52, 52, 1), y=a, yd=BF16, ys=(3 * 44 * 52, 44 * 52, 52, 1), shape=(2, 3, 44, 52), scales=3,
             data_range=2.0, ws=a, ws_bytes=big):
        return lib.sp_ssim_stats(x, xd, *xs, y, yd, *ys, *shape, scales, data_range, a, a, a, ws, ws_bytes, None)

    refusals = {
        "NULL x": dict(x=None), "NULL y": dict(y=None), "NULL workspace": dict(ws=None),
        "short workspace": dict(ws_bytes=_ws(2, 3, 44, 52, 3)[1] - 1), "no workspace bytes": dict(ws_bytes=0),
        "bad x dtype": dict(xd=2), "bad y dtype": dict(yd=4), "negative dtype": dict(xd=-1),
        "negative x stride": dict(xs=(3 * 44 * 52, 44 * 52, -52, 1)), "negative y stride": dict(ys=(-1, 44 * 52, 52, 1)),
        "n = 0": dict(shape=(0, 3, 44, 52)), "c = 0": dict(shape=(2, 0, 44, 52)), "h below 11": dict(shape=(2, 3, 8, 52), scales=1),
        "w below 11": dict(shape=(2, 3, 44, 10), scales=1), "n * c out of range": dict(shape=(1 << 13, 1 << 12, 44, 52)),
        "h out of range": dict(shape=(2, 3, 32784, 52), scales=1),
        "scales = 0": dict(scales=0), "scales = 6": dict(scales=6), "not divisible": dict(scales=4),
        "too small at the last scale": dict(shape=(2, 3, 40, 48)),
        "data_range 0": dict(data_range=0.0), "data_range negative": dict(data_range=-2.0), "data_range inf": dict(data_range=math.inf),
        "data_range nan": dict(data_range=math.nan),
    }
    for what, kw in refusals.items():
        assert call(**kw) == -1, what
        assert b"sp_ssim_" in lib.sp_last_error_string(), what
    assert (F32, BF16, F16) == (0, 1, 3)
    assert call(ws=ctypes.c_void_p(a.value + 4)) == -1 and b"aligned" in lib.sp_last_error_string()


def test_ops_and_module_are_there():
    from semantic_pyramid_for_image_generation_amd import ops, reconstruction
    assert ops.ssim_workspace_bytes(2, 3, 44, 52, 3) == _formula(2, 3, 44, 52, 3)
    with pytest.raises(_lib.SempyrError):
        ops.ssim_workspace_bytes(2, 3, 44, 52, 4)
    import torch
    with pytest.raises(_lib.SempyrError):                                      # no fallback: a CPU tensor is refused
        ops.ssim_stats(torch.zeros(1, 1, 11, 11), torch.zeros(1, 1, 11, 11))
    for name in ("psnr", "ssim", "ms_ssim", "compare", "evaluate_levels"):
        assert callable(getattr(reconstruction, name)), name
    assert reconstruction.MS_SSIM_WEIGHTS == R.MS_SSIM_WEIGHTS
    # the float64 formulas on the host side of the binding, on statistics made up here
    sq = torch.tensor([[0.0, 0.0], [3.0, 1.0]], dtype=torch.float64)
    got = reconstruction.psnr_from_stats(sq, 8)
    assert math.isinf(got[0].item()) and got[0].item() > 0 and abs(got[1].item() - 10 * math.log10(4 / (4.0 / 16))) < 1e-12
    t = torch.full((1, 2, 5), 0.83, dtype=torch.float64)
    assert abs(reconstruction.ms_ssim_from_stats(t, t).item() - 0.83 ** 1.0001) < 1e-14
    t[0, 0, 2] = -0.5                                                          # a negative cs mean is clamped: that channel's product is 0
    assert abs(reconstruction.ms_ssim_from_stats(t, t).item() - 0.5 * 0.83 ** 1.0001) < 1e-14
    t[0, 1, 4] = math.nan
    assert math.isnan(reconstruction.ms_ssim_from_stats(t, t).item())


# ---- the wrapper -----------------------------------------------------------------------------------------------------------------------
def _wrapper(**kw):
    import semantic_pyramid_for_image_generation_amd as sp
    return sp.ModelWrapper(sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8), None, [("never", "read", [])],
                           vgg16=sp.VGG16(), save_data_path=None, **kw)


def test_wrapper_option_on_and_off(monkeypatch):
    monkeypatch.setattr(config.CFG, "reconstruction", "")
    monkeypatch.setattr(config.CFG, "reconstruction_levels", "0-6")
    mw = _wrapper()
    assert mw.reconstruction == () and mw.reconstruction_levels == (0, 1, 2, 3, 4, 5, 6) and mw.last_reconstruction is None
    assert "reconstruction" not in mw.logger.hyperparameter
    assert mw.evaluate_reconstruction() == {} and mw.evaluate_reconstruction(device="cuda", use_ema=False) == {}
    assert mw.generator.training
    mw = _wrapper(reconstruction="ms_ssim,psnr", reconstruction_levels="0,6")
    assert mw.reconstruction == ("psnr", "ms_ssim") and mw.reconstruction_levels == (0, 6)
    assert mw.logger.hyperparameter["reconstruction"] == "psnr,ms_ssim" and mw.logger.hyperparameter["reconstruction_levels"] == "0,6"
    for bad in (dict(reconstruction="lpips"), dict(reconstruction="psnr", reconstruction_levels="0-7")):
        with pytest.raises(_lib.SempyrError):
            _wrapper(**bad)
    monkeypatch.setattr(config.CFG, "reconstruction", "ssim")
    monkeypatch.setattr(config.CFG, "reconstruction_levels", "2-3")
    mw = _wrapper()
    assert mw.reconstruction == ("ssim",) and mw.reconstruction_levels == (2, 3)
    assert _wrapper(reconstruction="").reconstruction == ()                    # the keyword wins over the configuration
    import semantic_pyramid_for_image_generation_amd as sp
    off = sp.ModelWrapper(sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8), None, None, vgg16=sp.VGG16(),
                          save_data_path=None, reconstruction="psnr")
    assert off.evaluate_reconstruction() == {}                                 # on, but no validation loader
