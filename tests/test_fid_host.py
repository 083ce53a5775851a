"""FID without a GPU: the Inception-v3 restatement's key set and size, the weight loader, the host BatchNorm folding and packing,
the Frechet distance against scipy's sqrtm, and validate() without weights (still nan)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_restated as R
from semantic_pyramid_for_image_generation_amd import fid, inception
from semantic_pyramid_for_image_generation_amd._lib import SempyrError


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict(0)


def test_restatement_sizes_and_keys(sd):
    assert R.param_count(sd) == R.TOTAL_PARAMS == 27_161_264
    assert R.param_count(sd, features_only=True) == R.FEATURE_PARAMS == 21_785_568
    convs = [c for c in R.basic_convs() if not c[0].startswith("AuxLogits.")]
    assert len(convs) == 94 == len(inception.CONV_LAYERS)
    # the library's layer table and the restatement agree on every layer's name and weight shape
    assert {n: (ci, co, k) for n, ci, co, k, _, _ in inception.CONV_LAYERS} == {n: (ci, co, k) for n, ci, co, k in convs}
    for name, cin, cout, (kh, kw), _, _ in inception.CONV_LAYERS:
        assert tuple(sd[name + ".conv.weight"].shape) == (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            assert tuple(sd["%s.bn.%s" % (name, k)].shape) == (cout,)
    # 5 keys per BasicConv2d (+ num_batches_tracked) and the two linear layers
    assert len(sd) == 96 * 6 + 4


def test_flops_per_image():
    """11.42 GFLOP per 299 x 299 image (2 x MAC), the figure tools/time_inception.py reports the fraction of peak against."""
    stem = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71}
    flops = 0
    for name, cin, cout, (kh, kw), s, _ in inception.CONV_LAYERS:
        if name in stem:
            o = stem[name]
        elif name.startswith(("Mixed_5", "Mixed_6a")):
            o = 17 if s == 2 else 35
        elif name.startswith(("Mixed_6", "Mixed_7a")):
            o = 8 if s == 2 else 17
        else:
            o = 8
        flops += 2 * o * o * cout * cin * kh * kw
    assert abs(flops / 1e9 - 11.42) < 0.01, flops


@pytest.mark.parametrize("aux,fc_,nbt", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
def test_loader_accepts_torchvision_keys(aux, fc_, nbt):
    sd = R.synth_state_dict(1, with_aux=aux, with_fc=fc_, with_nbt=nbt)
    net = inception.InceptionV3Features(sd, dtype=torch.float32)
    w, b = net._host["Mixed_7c.branch_pool"]
    assert tuple(w.shape) == (192, 2048) and tuple(b.shape) == (192,) and w.dtype == torch.float32
    assert tuple(net._host["Conv2d_1a_3x3"][0].shape) == (32, 9 * 8)          # the RGB input padded to 8 channels
    assert net._host["Conv2d_4a_3x3"][0].dtype == torch.float32
    assert inception.InceptionV3Features(sd, dtype=torch.bfloat16)._host["Conv2d_4a_3x3"][0].dtype == torch.bfloat16


def test_loader_reads_a_path(tmp_path, sd):
    p = tmp_path / "inception_v3_google-test.pth"
    torch.save(sd, str(p))
    a = inception.InceptionV3Features(str(p), dtype=torch.float32)
    b = inception.InceptionV3Features(sd, dtype=torch.float32)
    assert all(torch.equal(a._host[k][0], b._host[k][0]) and torch.equal(a._host[k][1], b._host[k][1]) for k in a._host)
    with pytest.raises(SempyrError, match="cannot read"):
        inception.InceptionV3Features(str(tmp_path / "missing.pth"))


@pytest.mark.parametrize("key", ["Mixed_6c.branch7x7dbl_3.conv.weight", "Conv2d_1a_3x3.bn.running_var", "Mixed_7c.branch_pool.bn.bias"])
def test_loader_names_a_missing_key(sd, key):
    bad = dict(sd)
    del bad[key]
    with pytest.raises(SempyrError, match="missing key " + key.replace(".", r"\.")):
        inception.InceptionV3Features(bad)


@pytest.mark.parametrize("key,shape", [("Mixed_6c.branch7x7dbl_3.conv.weight", (160, 160, 7, 1)), ("Mixed_5b.branch1x1.bn.weight", (65,))])
def test_loader_names_a_misshaped_key(sd, key, shape):
    bad = dict(sd)
    bad[key] = torch.zeros(shape)
    with pytest.raises(SempyrError, match=key.replace(".", r"\.") + r" has shape"):
        inception.InceptionV3Features(bad)


def test_loader_rejects_an_unknown_key(sd):
    bad = dict(sd)
    bad["Mixed_8a.branch1x1.conv.weight"] = torch.zeros(1)
    with pytest.raises(SempyrError, match=r"unexpected key Mixed_8a"):
        inception.InceptionV3Features(bad)


@pytest.mark.parametrize("name,pad", [("Conv2d_1a_3x3", (0, 0)), ("Mixed_6b.branch7x7_2", (0, 3)), ("Mixed_7b.branch3x3_2b", (1, 0)),
                                      ("Mixed_5b.branch5x5_2", (2, 2))])
def test_fold_equals_conv_then_bn(sd, name, pad):
    w = sd[name + ".conv.weight"].double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, w.shape[1], 9, 11), generator=g, dtype=torch.float64)
    bn = lambda k: sd[name + ".bn." + k].double()      # noqa: E731
    want = F.batch_norm(F.conv2d(x, w, padding=pad), bn("running_mean"), bn("running_var"), bn("weight"), bn("bias"),
                        training=False, eps=1e-3)
    wf, bf = inception.fold_bn(w, bn("weight"), bn("bias"), bn("running_mean"), bn("running_var"))
    got = F.conv2d(x, wf, bf, padding=pad)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_pack_layout(sd):
    w = sd["Mixed_6b.branch7x7dbl_2.conv.weight"]                     # (128, 128, 7, 1)
    p = inception.pack_conv(w, torch.float32)
    co, c, ky = 5, 77, 4
    assert p.shape == (128, 7 * 128) and p[co, ky * 128 + c] == w[co, c, ky, 0].float()
    p = inception.pack_conv(sd["Conv2d_1a_3x3.conv.weight"], torch.float32)      # cin 3 -> cin_p 8
    assert p.shape == (32, 72) and p[3, 4 * 8 + 1] == sd["Conv2d_1a_3x3.conv.weight"][3, 1, 1, 1]
    assert torch.count_nonzero(p.view(32, 9, 8)[:, :, 3:]) == 0


def _random_stats(rng, d, n):
    a = rng.standard_normal((n, d)) @ (rng.standard_normal((d, d)) * 0.3 + np.eye(d))
    return a.mean(0) + 0.1, np.cov(a, rowvar=False)


@pytest.mark.parametrize("d", [16, 64, 256])
def test_trace_sqrt_matches_scipy_sqrtm(d):
    rng = np.random.default_rng(d)
    _, s1 = _random_stats(rng, d, 4 * d)
    _, s2 = _random_stats(rng, d, 4 * d)
    a, b = fid.trace_sqrt_product(s1, s2), fid.trace_sqrt_product(s1, s2, method="sqrtm")
    assert abs(a - b) <= 1e-8 * abs(b)


def test_fid_matches_reference_formula():
    """frechet_inception_distance.py:101-123 written out with scipy.linalg.sqrtm, on well-conditioned random activations."""
    from scipy.linalg import sqrtm
    rng = np.random.default_rng(7)
    real = rng.standard_normal((400, 64)) @ (np.eye(64) + 0.2 * rng.standard_normal((64, 64)))
    fake = 0.9 * rng.standard_normal((400, 64)) + 0.3
    mu_r, mu_f = np.mean(real, axis=0), np.mean(fake, axis=0)
    cov_r, cov_f = np.cov(real, rowvar=False), np.cov(fake, rowvar=False)
    diff = mu_r - mu_f
    cov_mean, _ = sqrtm(cov_r @ cov_f, disp=False)
    want = diff @ diff + np.trace(cov_r) + np.trace(cov_f) - 2 * np.trace(cov_mean.real)
    got = fid.fid_from_activations(real.astype(np.float32).astype(np.float64), fake)
    assert abs(fid.fid_from_activations(real, fake) - want) <= 1e-8 * abs(want)
    assert abs(fid.fid_from_activations(real, fake, method="sqrtm") - want) <= 1e-12 * abs(want)
    assert math.isfinite(got)


def test_fid_of_identical_sets_is_zero():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((300, 48))
    assert abs(fid.fid_from_activations(x, x)) < 1e-9 * np.trace(np.cov(x, rowvar=False))


def test_validate_is_nan_without_weights(monkeypatch):
    import semantic_pyramid_for_image_generation_amd as sp
    from semantic_pyramid_for_image_generation_amd import config
    monkeypatch.setattr(config.CFG, "inception_weights", "")
    mw = sp.ModelWrapper(sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8), None, [("never", "read", [])],
                         vgg16=sp.VGG16(), save_data_path=None)
    assert math.isnan(mw.validate())
    assert math.isnan(mw.validate(device="cuda"))          # main.py:111's call
    assert mw.generator.training


def test_fid_needs_weights(monkeypatch):
    from semantic_pyramid_for_image_generation_amd import config
    monkeypatch.setattr(config.CFG, "inception_weights", "")
    with pytest.raises(SempyrError, match="SP_INCEPTION_WEIGHTS"):
        fid.frechet_inception_distance([], None, None)


def test_config_reads_the_weights_path(monkeypatch):
    from semantic_pyramid_for_image_generation_amd import config
    monkeypatch.setenv("SP_INCEPTION_WEIGHTS", "/some/inception_v3_google.pth")
    assert config.Config.from_env().inception_weights == "/some/inception_v3_google.pth"
    monkeypatch.delenv("SP_INCEPTION_WEIGHTS")
    assert config.Config.from_env().inception_weights == ""


def test_general_conv_struct_matches_header_and_bad_shapes_are_rejected():
    """sp_conv_general_params: the ctypes layout equals the header's, and arguments outside the contract come back as errors before
    anything is launched (no GPU needed: the checks run on the host)."""
    import ctypes
    import re
    from semantic_pyramid_for_image_generation_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(L.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct sp_conv_general_params \{(.*?)\}", text, flags=re.S).group(1)
    assert [n for n, _ in L.SpConvGeneralParams._fields_] == re.findall(r"(\w+)\s*[;,]", body)
    lib = L.lib()
    fake = 1 << 20                                   # aligned, never dereferenced: every call below fails its argument checks
    good = dict(dtype=L.SP_F32, x=fake, w=fake, bias=None, y=fake, n=1, h=17, w_=17, cin_p=16, ldx=16, cout=16, ldy=16, kh=3, kw=3,
                stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=L.ACT_RELU)
    cases = [(dict(cin_p=12, ldx=12), L.SP_F32, "cin_p"), (dict(kh=9), L.SP_F32, "kernel"), (dict(stride_h=3), L.SP_F32, "stride"),
             (dict(pad_w=3), L.SP_F32, "padding"), (dict(cout=18, ldy=20), L.SP_F32, "cout"), (dict(ldx=8), L.SP_F32, "ldx"),
             (dict(act=L.ACT_TANH), L.SP_F32, "act"), (dict(y=fake + 2), L.SP_F32, "alignment"), (dict(h=2, w_=2, pad_h=0, pad_w=0), L.SP_F32, "larger"),
             (dict(dtype=L.SP_F8), L.SP_F8, "dtype"), (dict(cin_p=12, ldx=12, dtype=L.SP_F16), L.SP_F16, "cin_p")]
    for change, _, needle in cases:
        p = L.SpConvGeneralParams(**dict(good, **change))
        rc = lib.sp_conv2d_general(ctypes.byref(p), None)
        assert rc in (-1, -3) and needle in lib.sp_last_error_string().decode(), (change, rc, lib.sp_last_error_string())
    for dt in (L.SP_F32, L.SP_F16):
        p = L.SpConvGeneralParams(**dict(good, dtype=dt, cin_p=12))
        p.struct_bytes = 48                          # a caller built against another layout
        assert lib.sp_conv2d_general(ctypes.byref(p), None) == -1 and "struct_bytes" in lib.sp_last_error_string().decode()
    assert lib.sp_conv2d_general(None, None) == -1
    assert lib.sp_maxpool3s2_fwd(fake, 6, fake, 8, 1, 9, 9, 6, L.SP_F32, None) == -1
    assert lib.sp_maxpool3s2_fwd(fake, 8, fake, 8, 1, 2, 9, 8, L.SP_F32, None) == -1
    assert lib.sp_avgpool3s1_fwd(fake, fake, 1, 9, 9, 6, L.SP_BF16, None) == -1
    assert lib.sp_inception_prep(fake, fake, fake, 1, 3, 8, 8, 299, 299, 4, L.SP_F32, None) == -1
    assert lib.sp_global_avgpool_f32(fake, fake, 1, 64, 2048, L.SP_F8, None) == -3
