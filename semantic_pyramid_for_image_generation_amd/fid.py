"""Frechet Inception Distance (/root/reference/frechet_inception_distance.py:45-123).

The activations come from ``inception.InceptionV3Features`` on the device; the statistics run on the host in float64 as the
reference computes them (np.mean, np.cov(rowvar=False)):

    FID = |mu_r - mu_f|^2 + tr S_r + tr S_f - 2 tr sqrt(S_r S_f)

The reference takes tr sqrt(S_r S_f) from ``scipy.linalg.sqrtm(S_r @ S_f, disp=False)`` (real part).  For covariance matrices
(symmetric, positive semi-definite) the eigenvalues of S_r S_f are those of sqrt(S_r) S_f sqrt(S_r), which is symmetric PSD, so
the trace is the sum of the square roots of ITS eigenvalues: two ``eigh`` calls instead of a Schur decomposition, much faster at
2048 x 2048.  ``trace_sqrt_product(..., method='sqrtm')`` is the reference's form; tests/test_fid_host.py holds one to the other.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import SempyrError


def _psd_sqrt(a: np.ndarray) -> np.ndarray:
    w, v = np.linalg.eigh(a)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def trace_sqrt_product(a: np.ndarray, b: np.ndarray, method: str = "eigh") -> float:
    """tr sqrt(a @ b) for symmetric PSD a, b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if method == "sqrtm":
        from scipy.linalg import sqrtm
        m, _ = sqrtm(a @ b, disp=False)
        return float(np.trace(m.real))
    if method != "eigh":
        raise ValueError("method must be 'eigh' or 'sqrtm'")
    ra = _psd_sqrt(a)
    m = ra @ b @ ra
    w = np.linalg.eigvalsh((m + m.T) * 0.5)
    return float(np.sqrt(np.clip(w, 0.0, None)).sum())


def frechet_distance(mu1: np.ndarray, cov1: np.ndarray, mu2: np.ndarray, cov2: np.ndarray, method: str = "eigh") -> float:
    if mu1.shape != mu2.shape or cov1.shape != cov2.shape:
        raise ValueError("statistics of different shapes: %s / %s, %s / %s" % (mu1.shape, mu2.shape, cov1.shape, cov2.shape))
    diff = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(diff @ diff + np.trace(cov1) + np.trace(cov2) - 2.0 * trace_sqrt_product(cov1, cov2, method))


def fid_from_activations(real: np.ndarray, fake: np.ndarray, method: str = "eigh") -> float:
    """FID of two (N, 2048) activation sets (frechet_inception_distance.py:101-123), statistics in float64."""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    return frechet_distance(real.mean(axis=0), np.cov(real, rowvar=False), fake.mean(axis=0), np.cov(fake, rowvar=False), method)


def _extractor(inception):
    if inception is None:
        from .config import CFG
        if not CFG.inception_weights:
            raise SempyrError("FID needs Inception-v3 weights: pass inception= (an InceptionV3Features or a state-dict path) "
                              "or set SP_INCEPTION_WEIGHTS")
        inception = CFG.inception_weights
    if not callable(inception):
        from .inception import InceptionV3Features
        inception = InceptionV3Features(inception)
    return inception


@torch.no_grad()
def _collect(dataset_real, generator, vgg16, device, inception, on_device: bool):
    inception = _extractor(inception)
    latent = generator.module.latent_dimensions if hasattr(generator, "module") else generator.latent_dimensions
    keep = (lambda t: t) if on_device else (lambda t: t.cpu())
    real, fake = [], []
    for images, labels, masks in dataset_real:
        images = images.to(device)
        masks = [m.to(device) for m in masks]
        real.append(keep(inception(images)))
        features_real = vgg16(images)
        noise = torch.randn((images.shape[0], latent), dtype=torch.float32, device=device)
        images_fake = generator(input=noise, features=features_real, masks=masks, class_id=labels.to(device).float())
        fake.append(keep(inception(images_fake.float())))
    if not real:
        raise SempyrError("FID over an empty validation loader")
    return torch.cat(real), torch.cat(fake)


def collect_activations(dataset_real, generator, vgg16, device="cuda", inception=None):
    """The loop of frechet_inception_distance.py:63-97: per batch the real activations, vgg16(images), randn(B, latent), the
    generator (in whatever mode the caller left it) on the loader's masks and labels.float(), the fake activations.
    Returns the two (N, 2048) float32 arrays."""
    real, fake = _collect(dataset_real, generator, vgg16, device, inception, on_device=False)
    return real.numpy(), fake.numpy()


def collect_activations_device(dataset_real, generator, vgg16, device="cuda", inception=None):
    """The same loop, run once, with the two (N, 2048) float32 activation sets left ON THE DEVICE (what metrics.py's pair-set
    kernels read): no host transfer per batch."""
    return _collect(dataset_real, generator, vgg16, device, inception, on_device=True)


@torch.no_grad()
def frechet_inception_distance(dataset_real, generator, vgg16, device: str = "cuda", inception=None) -> float:
    """frechet_inception_distance.py:45-123.  `inception`: an InceptionV3Features, a torchvision inception_v3 state-dict path,
    or None for config.CFG.inception_weights (SP_INCEPTION_WEIGHTS)."""
    real, fake = collect_activations(dataset_real, generator, vgg16, device=device, inception=inception)
    return fid_from_activations(real, fake)


@torch.no_grad()
def evaluate(dataset_real, generator, vgg16, device: str = "cuda", inception=None, metrics="", nearest_k: int = 5,
             kid_subsets: int = 100, kid_subset_size: int = 1000, kid_seed: int = 0, is_splits: int = 10) -> dict:
    """ONE pass of the loader loop, every score from its activations: {"fid": ...} as frechet_inception_distance computes it (the
    same value for the same seed), plus what `metrics` names (config.parse_metrics: "kid" -> "kid"; "prdc" -> "precision",
    "recall", "density", "coverage"; "is" -> "inception_score", "inception_score_std" of the fake set under the extractor's
    classifier_head) from the activations kept on the device (metrics.py, csrc/metrics.hip)."""
    from . import metrics as M
    names = M.parse_metrics(metrics)
    inception = _extractor(inception)
    head = None
    if "is" in names:
        head = inception.classifier_head(device) if hasattr(inception, "classifier_head") else None
        if head is None:                                 # before the loader loop, not after it
            raise SempyrError("the Inception Score needs the classifier: the Inception-v3 state dict has no fc.weight / fc.bias")
    real, fake = collect_activations_device(dataset_real, generator, vgg16, device=device, inception=inception)
    out = M.compute(real, fake, names, nearest_k=nearest_k, head=head, is_splits=is_splits, num_subsets=kid_subsets,
                    max_subset_size=kid_subset_size, seed=kid_seed)
    out["fid"] = fid_from_activations(real.cpu().numpy(), fake.cpu().numpy())
    return out
