"""Per-image reconstruction fidelity: PSNR, SSIM and MS-SSIM of image k against ITS OWN inversion.

The set metrics (fid.py, metrics.py) compare the generated set with the real set; none of them says whether the generator, conditioned
on the features of level s of image k, gives image k back.  These three do.  All of them are functions of the statistics ONE call of
``ops.ssim_stats`` leaves on the device (csrc/reconstruction.hip; include/sempyr.h: sp_ssim_stats has the definition of the window,
the moments, the two maps and the pooling); the formulas below run in float64 on those (n, c, scales) / (n, c) tensors:

    psnr     10 log10(L^2 / (sum_c sqerr / (C H W)));  +inf for an identical pair
    ssim     mean_c ssim_mean[., c, 0]                                                     (Wang, Bovik, Sheikh, Simoncelli 2004)
    ms_ssim  mean_c [ prod_{j<4} max(cs_mean[., c, j], 0)^w_j * max(ssim_mean[., c, 4], 0)^w_4 ]     (Wang, Simoncelli, Bovik 2003)

with L the data range (2.0: the data and the generator's tanh live in [-1, 1]) and w = MS_SSIM_WEIGHTS.  MS-SSIM takes five scales, so H
and W must be divisible by 16 and >= 176 (256 qualifies); nothing is padded.  A NaN or infinity in a plane makes that image's scores NaN
and touches no other image.  No gradients: these are evaluation metrics, not losses.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import misc, ops
from ._lib import SempyrError
from .config import RECONSTRUCTION_NAMES, parse_levels, parse_reconstruction

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003
MS_SSIM_SCALES = len(MS_SSIM_WEIGHTS)


def psnr_from_stats(sqerr: torch.Tensor, pixels_per_plane: int, data_range: float = 2.0) -> torch.Tensor:
    """(n,) float64 from sqerr (n, c): 10 log10(L^2 / mse) with mse the mean over all c * pixels_per_plane values; +inf where mse == 0."""
    mse = sqerr.sum(dim=1) / float(sqerr.shape[1] * pixels_per_plane)
    return 10.0 * torch.log10(float(data_range) ** 2 / mse)


def ssim_from_stats(ssim_mean: torch.Tensor) -> torch.Tensor:
    """(n,) float64 from ssim_mean (n, c, scales): the channel mean of scale 0."""
    return ssim_mean[:, :, 0].mean(dim=1)


def ms_ssim_from_stats(ssim_mean: torch.Tensor, cs_mean: torch.Tensor) -> torch.Tensor:
    """(n,) float64 from the five-scale (n, c, 5) statistics: per channel the weighted product of the clamped cs means of scales 0..3 and
    the clamped ssim mean of scale 4, then the channel mean."""
    if ssim_mean.shape[-1] != MS_SSIM_SCALES or cs_mean.shape[-1] != MS_SSIM_SCALES:
        raise SempyrError("ms_ssim takes the statistics of %d scales, got %d" % (MS_SSIM_SCALES, ssim_mean.shape[-1]))
    w = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=ssim_mean.device)
    terms = torch.cat([cs_mean[:, :, :MS_SSIM_SCALES - 1], ssim_mean[:, :, MS_SSIM_SCALES - 1:]], dim=2)
    # clamp(min=0) keeps a NaN (torch.clamp propagates it), so a poisoned plane stays NaN
    return torch.pow(terms.clamp(min=0.0), w).prod(dim=2).mean(dim=1)


def _names(names) -> tuple:
    try:
        return parse_reconstruction(names)
    except ValueError as exc:
        raise SempyrError(str(exc)) from None


def compare(x: torch.Tensor, y: torch.Tensor, names, data_range: float = 2.0, workspace=None) -> Dict[str, torch.Tensor]:
    """{name: (n,) float64 device tensor} for the names asked (a comma-separated string or a sequence of psnr, ssim, ms_ssim) from ONE
    ops.ssim_stats call: five scales where ms_ssim is among them, one otherwise.  x, y: (n, c, h, w) on the GPU, any strides, fp32 /
    bf16 / fp16 each."""
    names = _names(names)
    if not names:
        return {}
    scales = MS_SSIM_SCALES if "ms_ssim" in names else 1
    ssim_mean, cs_mean, sqerr = ops.ssim_stats(x, y, scales=scales, data_range=data_range, workspace=workspace)
    out = {}
    if "psnr" in names:
        out["psnr"] = psnr_from_stats(sqerr, x.shape[2] * x.shape[3], data_range)
    if "ssim" in names:
        out["ssim"] = ssim_from_stats(ssim_mean)
    if "ms_ssim" in names:
        out["ms_ssim"] = ms_ssim_from_stats(ssim_mean, cs_mean)
    return out


def psnr(x: torch.Tensor, y: torch.Tensor, data_range: float = 2.0) -> torch.Tensor:
    """Peak signal-to-noise ratio per image in dB, (n,) float64 on the device; +inf for an identical pair."""
    return compare(x, y, ("psnr",), data_range)["psnr"]


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 2.0) -> torch.Tensor:
    """Structural similarity per image (11 x 11 Gaussian window, sigma 1.5, valid positions), (n,) float64 on the device."""
    return compare(x, y, ("ssim",), data_range)["ssim"]


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 2.0) -> torch.Tensor:
    """Five-scale structural similarity per image, (n,) float64 on the device; H and W divisible by 16 and >= 176."""
    return compare(x, y, ("ms_ssim",), data_range)["ms_ssim"]


@torch.no_grad()
def evaluate_levels(dataset_real, generator, vgg16, device="cuda", levels="0-6", names=RECONSTRUCTION_NAMES,
                    data_range: float = 2.0) -> Dict[str, float]:
    """{"<name>_level<s>": float64 mean over all images} for every name asked and every level s asked: how faithfully the generator
    (in whatever mode the caller left it) gives an image back from level s of its own VGG-16 pyramid alone.

    fid._collect's loop with level handling: per batch the images go to the device and through vgg16 ONCE; then, per level in ascending
    order, one randn(B, latent) and the generator on misc.get_masks_for_inference(s) broadcast to the batch (inference()'s stage index; the
    loader's own masks are ignored) with labels.float().  Each pair is scored by compare() into per-image device buffers; the means are
    taken on the device and cross to the host in ONE transfer at the end.  A psnr mean over a set that holds an identical pair is inf; a
    non-finite image makes its scores, and so the means they enter, NaN."""
    names = _names(names)
    try:
        levels = parse_levels(levels)
    except ValueError as exc:
        raise SempyrError(str(exc)) from None
    if not names:
        return {}
    latent = generator.module.latent_dimensions if hasattr(generator, "module") else generator.latent_dimensions
    scores = {(name, s): [] for s in levels for name in names}
    masks_cache = {}
    for images, labels, _ in dataset_real:
        images = images.to(device)
        b = images.shape[0]
        class_id = labels.to(device).float()
        features_real = vgg16(images)
        for s in levels:
            if (s, b) not in masks_cache:
                masks_cache[(s, b)] = [m.expand(b, *m.shape[1:]).contiguous()
                                       for m in misc.get_masks_for_inference(s, add_batch_size=True, device=device)]
            noise = torch.randn((b, latent), dtype=torch.float32, device=device)
            images_fake = generator(input=noise, features=features_real, masks=masks_cache[(s, b)], class_id=class_id)
            for name, value in compare(images, images_fake, names, data_range).items():
                scores[(name, s)].append(value)
    if not any(scores.values()):
        raise SempyrError("reconstruction fidelity over an empty validation loader")
    keys = ["%s_level%d" % (name, s) for s in levels for name in names]
    means = torch.stack([torch.cat(scores[(name, s)]).mean() for s in levels for name in names]).tolist()      # the one host transfer
    return dict(zip(keys, means))
