"""The reconstruction-fidelity kernel (csrc/reconstruction.hip) on the GPU: ops.ssim_stats against the float64
restatement within the bound DERIVED in tests/reconstruction_restated.py, exact squared errors and pooled planes, every source
form bit for bit, locality, determinism, the three scores and ModelWrapper.evaluate_reconstruction() end to end.

Shapes are the smallest that reach every path: (2, 3, 44, 52) is two tiles across with a partial tile in both axes, and its third
scale is 11 x 13 (1 x 3 positions); (3, 1, 76, 44) is five tile rows with a short last one; (1, 2, 176, 208) is the smallest plane
family MS-SSIM's five scales admit with unequal sides.  The conditions on the bound are asserted on the CPU before any launch."""
import functools
import math

import numpy as np
import pytest
import torch

import reconstruction_restated as R
from test_reconstruction_host import CASES, check_bound_conditions
from semantic_pyramid_for_image_generation_amd import _lib as L
from semantic_pyramid_for_image_generation_amd import ops, reconstruction

pytestmark = pytest.mark.gpu


def _dev(x):
    torch.cuda.set_device(0)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _bits(*tensors):
    return [t.detach().cpu().contiguous().view(torch.int64) for t in tensors]


def _same_bits(got, want, what):
    for g, w, name in zip(_bits(*got), _bits(*want), ("ssim_mean", "cs_mean", "sqerr")):
        assert torch.equal(g, w), (what, name)


@functools.lru_cache(maxsize=None)
def _case(name, shape, scales):
    """(x, y, restated statistics) of an operand family at a shape, computed once and shared; never modified."""
    x, y = R.family(name, shape)
    return x, y, R.stats(x, y, scales)


@functools.lru_cache(maxsize=None)
def _conditions():
    return check_bound_conditions()


def _check(got, st, scales, what):
    """ssim_mean / cs_mean of `scales` scales within the restatement's bounds (the statistics of scale j do not depend on how many
    scales follow), sqerr within the float64 sum's own reordering error."""
    ssim_mean, cs_mean, sqerr = (t.cpu().numpy() for t in got)
    n, c = sqerr.shape
    assert ssim_mean.shape == cs_mean.shape == (n, c, scales)
    for key, arr, bkey in (("ssim_mean", ssim_mean, "bound_ssim"), ("cs_mean", cs_mean, "bound_cs")):
        err, bound = np.abs(arr - st[key][:, :, :scales]), st[bkey][:, :, :scales]
        print("%s %s: max err per scale %s, bound %s" % (what, key, " ".join("%.2e" % v for v in err.max(axis=(0, 1))),
                                                          " ".join("%.2e" % v for v in bound.max(axis=(0, 1)))))
        assert (err <= bound).all(), (what, key, err.max(), (err / bound).max())
    reorder = 2.0 ** -53 * 1e6                                                 # far fewer than 10^6 exact terms per plane here
    assert (np.abs(sqerr - st["sqerr"]) <= reorder * st["sqerr"]).all(), what


# ---- the statistics against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d_s%d" % (c[0] + (c[1],)))
def test_stats_match_the_restatement_within_the_derived_bound(case, name):
    _conditions()
    shape, scales = case
    x, y, st = _case(name, shape, scales)
    xd, yd = _dev(x), _dev(y)
    for s in ((1, 2, 3) if shape == (2, 3, 44, 52) else (scales,)):
        got = ops.ssim_stats(xd, yd, scales=s)
        assert all(t.dtype == torch.float64 and t.is_cuda for t in got)
        _check(got, st, s, "%s %s scales=%d" % (shape, name, s))


def test_identical_images():
    _conditions()
    shape, scales = (2, 3, 44, 52), 3
    x, _, _ = _case("smooth", shape, scales)
    st = R.stats(x, x, scales)
    ssim_mean, cs_mean, sqerr = ops.ssim_stats(_dev(x), _dev(x.copy()), scales=scales)
    assert (np.abs(ssim_mean.cpu().numpy() - 1) <= st["bound_ssim"]).all() and (np.abs(cs_mean.cpu().numpy() - 1) <= st["bound_cs"]).all()
    assert (sqerr == 0).all()
    assert torch.isposinf(reconstruction.psnr(_dev(x), _dev(x))).all()


def test_squared_error_is_exact_and_the_pooled_planes_match_bit_for_bit():
    """Pixels are multiples of 2^-8 in [-1, 1]: every (x - y)^2 and every float64 partial sum is exact, so sqerr must EQUAL the integer
    result scaled by 2^-16.  The workspace's first planes are scale 1 of x, then of y (include/sempyr.h: sp_ssim_workspace)."""
    for shape in ((2, 3, 44, 52), (3, 1, 76, 44)):
        x, y, exact = R.dyadic_pair(shape)
        n, c, h, w = shape
        ws = torch.zeros(ops.ssim_workspace_bytes(n, c, h, w, 2) // 8, dtype=torch.float64, device="cuda")
        _, _, sqerr = ops.ssim_stats(_dev(x), _dev(y), scales=2, workspace=ws)
        assert (sqerr.cpu().numpy() == exact).all(), shape
        assert (ops.ssim_stats(_dev(x), _dev(y), scales=1)[2].cpu().numpy() == exact).all(), shape
        planes = n * c * (h // 2) * (w // 2)
        assert planes * 4 % 8 == 0
        pooled = ws.view(torch.float32)[:2 * planes].cpu().numpy().reshape(2, n, c, h // 2, w // 2)
        for got, src in zip(pooled, (x, y)):
            assert (got.view(np.int32) == R.pool2(src).view(np.int32)).all(), shape
    # ... and on values that are NOT dyadic, where the order of the three additions shows
    x, y, _ = _case("noise", (2, 3, 44, 52), 3)
    ws = torch.zeros(ops.ssim_workspace_bytes(2, 3, 44, 52, 3) // 8, dtype=torch.float64, device="cuda")
    ops.ssim_stats(_dev(x), _dev(y), scales=3, workspace=ws)
    flat, off = ws.view(torch.float32).cpu().numpy(), 0
    xs, ys = R.pyramid(x, 3), R.pyramid(y, 3)
    for j in (1, 2):
        for src in (xs[j], ys[j]):
            assert src.size * 4 % 8 == 0
            assert (flat[off:off + src.size].view(np.int32) == src.ravel().view(np.int32)).all(), j
            off += src.size


# ---- sources ---------------------------------------------------------------------------------------------------------------------------
def test_every_source_form_gives_the_same_bits():
    """Values are multiples of 2^-6 in [-1, 1]: bf16 and fp16 hold them exactly, so a 16-bit channels-last y, a non-contiguous slice of
    a larger batch and 16-bit x must give the bits of the contiguous fp32 pair."""
    shape, scales = (2, 3, 44, 52), 3
    n, c, h, w = shape
    rng = np.random.default_rng(5)
    x = (rng.integers(-64, 65, shape) / 64.0).astype(np.float32)
    y = (rng.integers(-64, 65, shape) / 64.0).astype(np.float32)
    st = R.stats(x, y, scales)
    xd, yd = _dev(x), _dev(y)
    want = ops.ssim_stats(xd, yd, scales=scales)
    _check(want, st, scales, "dyadic fp32")
    for dtype in (torch.bfloat16, torch.float16):
        y16 = yd.to(dtype).contiguous(memory_format=torch.channels_last)
        assert y16.stride() == (c * h * w, 1, w * c, c) and torch.equal(y16.float(), yd)
        _same_bits(ops.ssim_stats(xd, y16, scales=scales), want, "y %s channels-last" % dtype)
        _same_bits(ops.ssim_stats(xd.to(dtype), y16, scales=scales), want, "x %s, y %s channels-last" % (dtype, dtype))
    _same_bits(ops.ssim_stats(xd.to(torch.float16), yd.to(torch.bfloat16), scales=scales), want, "x fp16, y bf16")
    big = torch.full((2 * n + 1, c + 1, h + 2, w + 3), float("nan"), dtype=torch.float32, device="cuda")
    view = big[1::2][:n, 1:, 1:-1, 2:-1]
    view.copy_(yd)
    assert not view.is_contiguous() and view.shape == yd.shape
    _same_bits(ops.ssim_stats(xd, view, scales=scales), want, "y a slice of a larger batch")
    _same_bits(ops.ssim_stats(view, xd, scales=scales), ops.ssim_stats(yd, xd, scales=scales), "x a slice")


# ---- locality --------------------------------------------------------------------------------------------------------------------------
def test_an_image_alone_gives_the_bits_it_gives_in_a_batch():
    x, y, _ = _case("smooth", (3, 1, 76, 44), 2)
    xd, yd = _dev(x), _dev(y)
    whole = ops.ssim_stats(xd, yd, scales=2)
    for i in range(3):
        _same_bits(ops.ssim_stats(xd[i:i + 1], yd[i:i + 1], scales=2), [t[i:i + 1] for t in whole], "image %d" % i)


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_pixel_poisons_exactly_its_own_plane(poison):
    shape, scales = (2, 3, 44, 52), 3
    x, y, _ = _case("noise", shape, scales)
    xd, yd = _dev(x), _dev(y)
    clean = ops.ssim_stats(xd, yd, scales=scales)
    for which in ("x", "y"):
        bad = (xd if which == "x" else yd).clone()
        bad[1, 0, 37, 45] = poison                                             # in the second tile across, the last rows down
        got = ops.ssim_stats(bad, yd, scales=scales) if which == "x" else ops.ssim_stats(xd, bad, scales=scales)
        hit = torch.zeros(2, 3, dtype=torch.bool, device="cuda")
        hit[1, 0] = True
        for g, w, name in zip(got, clean, ("ssim_mean", "cs_mean", "sqerr")):
            assert torch.isnan(g[hit]).all(), (which, name, g[hit])
            assert torch.equal(g[~hit].view(torch.int64), w[~hit].view(torch.int64)), (which, name)
    scores = reconstruction.compare(xd, bad, "psnr,ssim")
    assert all(math.isnan(v[1].item()) and math.isfinite(v[0].item()) for v in scores.values())


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits():
    x, y, _ = _case("noise", (1, 2, 176, 208), 5)
    xd, yd = _dev(x), _dev(y)
    first = ops.ssim_stats(xd, yd, scales=5)
    ws = torch.full((ops.ssim_workspace_bytes(1, 2, 176, 208, 5) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    _same_bits(ops.ssim_stats(xd, yd, scales=5, workspace=ws), first, "a second launch, on a workspace full of NaN")
    with pytest.raises(L.SempyrError):
        ops.ssim_stats(xd, yd, scales=5, workspace=ws[:-1])


# ---- the three scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
def test_scores_match_the_restatement_within_the_propagated_bound(name):
    shape = (1, 2, 176, 208)
    x, y, st = _case(name, shape, 5)
    xd, yd = _dev(x), _dev(y)
    want_ssim, b_ssim = R.ssim(st)
    want_ms, b_ms = R.ms_ssim(st)
    want_psnr, b_psnr = R.psnr(st["sqerr"], 176 * 208), R.psnr_bound(shape)
    got = {"psnr": reconstruction.psnr(xd, yd), "ssim": reconstruction.ssim(xd, yd), "ms_ssim": reconstruction.ms_ssim(xd, yd)}
    both = reconstruction.compare(xd, yd, ("ms_ssim", "psnr", "ssim"))
    assert list(both) == ["psnr", "ssim", "ms_ssim"]
    for key, want, bound in (("psnr", want_psnr, b_psnr), ("ssim", want_ssim, b_ssim), ("ms_ssim", want_ms, b_ms)):
        for src in (got, both):
            v = src[key]
            assert v.dtype == torch.float64 and v.is_cuda and v.shape == (1,)
            err = np.abs(v.cpu().numpy() - want)
            print("%s %s: %.12g, err %.2e, bound %.2e" % (name, key, v.item(), err.max(), np.max(bound)))
            assert (err <= bound).all(), (name, key, err, bound)
    with pytest.raises(L.SempyrError):
        reconstruction.ms_ssim(xd[:, :, :160], yd[:, :, :160])                 # 160 / 16 = 10 < 11: refused, not padded


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_reconstruction_end_to_end():
    import _fid_child as C
    import semantic_pyramid_for_image_generation_amd as sp
    from semantic_pyramid_for_image_generation_amd import misc
    ops.set_compute_dtype(torch.float32)
    try:
        base, loader = C.setup()
        mw = sp.ModelWrapper(base.generator, base.discriminator, None, loader, vgg16=base.vgg16, save_data_path=None,
                             reconstruction="psnr,ssim,ms_ssim", reconstruction_levels="0,6")
        torch.manual_seed(C.SEED)
        out = mw.evaluate_reconstruction()
        keys = ["%s_level%d" % (name, s) for s in (0, 6) for name in ("psnr", "ssim", "ms_ssim")]
        assert list(out) == keys and all(math.isfinite(v) for v in out.values()), out
        assert mw.last_reconstruction == out and mw.generator.training
        # the loop by hand under the same seed, every pair scored by the restatement
        dev = torch.device("cuda", 0)
        torch.manual_seed(C.SEED)
        want = {k: [] for k in keys}
        bound = {k: [] for k in keys}
        mw.generator.eval()
        try:
            with torch.no_grad():
                for images, labels, _ in loader:
                    images = images.to(dev)
                    b = images.shape[0]
                    feats = mw.vgg16(images)
                    for s in (0, 6):
                        masks = [m.expand(b, *m.shape[1:]).contiguous() for m in misc.get_masks_for_inference(s, add_batch_size=True, device=dev)]
                        z = torch.randn((b, mw.latent_dimensions), dtype=torch.float32, device=dev)
                        fake = mw.generator(input=z, features=feats, masks=masks, class_id=labels.to(dev).float())
                        assert fake.dtype == torch.float32
                        st = R.stats(images.cpu().numpy(), fake.float().cpu().numpy(), 5)
                        for name, (v, e) in (("psnr", (R.psnr(st["sqerr"], 256 * 256), np.full(b, R.psnr_bound(images.shape)))),
                                             ("ssim", R.ssim(st)), ("ms_ssim", R.ms_ssim(st))):
                            want["%s_level%d" % (name, s)].append(v)
                            bound["%s_level%d" % (name, s)].append(e)
        finally:
            mw.generator.train()
        for k in keys:
            w, e = np.concatenate(want[k]).mean(), np.concatenate(bound[k]).mean() + 16 * 2.0 ** -53 * abs(np.concatenate(want[k]).mean())
            print("%s: %.12g (restated %.12g, err %.2e, bound %.2e)" % (k, out[k], w, abs(out[k] - w), e))
            assert abs(out[k] - w) <= e, (k, out[k], w, e)
        # off: the wrapper built without the argument and one with the option off do what the parent's code path does - nothing is
        # drawn, launched or kept by the option, and validate() (no Inception weights here: nan) is untouched by it
        off = sp.ModelWrapper(base.generator, base.discriminator, None, loader, vgg16=base.vgg16, save_data_path=None, reconstruction="")
        for w_ in (base, off):
            torch.manual_seed(C.SEED)
            state = torch.cuda.get_rng_state(0)
            assert w_.reconstruction == () and w_.evaluate_reconstruction() == {}
            assert math.isnan(w_.validate())
            assert torch.equal(torch.cuda.get_rng_state(0), state) and w_.generator.training
        # ... and with weights, validate() gives the same FID with the option on as without the argument, under the same seed
        import inception_restated as IR
        from semantic_pyramid_for_image_generation_amd import inception
        net = inception.InceptionV3Features(IR.synth_state_dict(21))
        values = []
        for kw in (dict(), dict(reconstruction="psnr,ssim,ms_ssim", reconstruction_levels="0,6")):
            w_ = sp.ModelWrapper(base.generator, base.discriminator, None, loader, vgg16=base.vgg16, save_data_path=None, inception=net, **kw)
            torch.manual_seed(C.SEED)
            values.append(w_.validate())
        assert math.isfinite(values[0]) and values[0] == values[1], values
    finally:
        ops.set_compute_dtype(torch.float32)
