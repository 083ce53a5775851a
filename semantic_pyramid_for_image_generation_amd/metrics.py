"""Sample-quality metrics next to the FID, on the pair-set kernels of csrc/metrics.hip.

All of them are functions of the two (N, d) activation sets ``fid.collect_activations`` produces:

    kid(real, fake)    Kernel Inception Distance (Binkowski et al. 2018), subsets and polynomial kernel as StyleGAN2-ADA computes it:
                       m = min(N, M, max_subset_size); every subset draws m fake rows x, then m real rows y, without replacement
                       (numpy RandomState(seed).choice, in that order); k(u, v) = (u.v / d + 1)^3;
                       t += (S_xx - diag_xx + S_yy - diag_yy) / (m - 1) - 2 S_xy / m;  KID = t / num_subsets / m
    prdc(real, fake)   improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) with ONE
                       nearest_k: R_i / F_j = the k-th smallest squared distance to the OTHER rows of the own set (self excluded by
                       index: a duplicate row is a neighbour at distance 0); every ball is closed (<=)
                           precision = mean_j [exists i: D(f_j, r_i) <= R_i]      recall   = mean_i [exists j: D(r_i, f_j) <= F_j]
                           density   = sum_j #{i: D(f_j, r_i) <= R_i} / (k M)     coverage = mean_i [min_j D(r_i, f_j) <= R_i]
    inception_score(acts, weight, bias)
                       Inception Score (Salimans et al. 2016) of ONE set, in the split form StyleGAN2-ADA and torch-fidelity compute
                       (DESIGN.md 19): logits l = acts @ weight.T + bias (torchvision's fc: 1000 classes), p = softmax(l) in float64;
                       split s of S holds the rows [floor(s n / S), floor((s + 1) n / S)); q_s = mean of p over the split;
                       KL_s = mean_{i in s} sum_c p_ic log p_ic - sum_c q_sc log q_sc;  score_s = exp(KL_s);
                       inception_score = mean_s score_s, inception_score_std = sqrt(mean_s (score_s - mean)^2)  (numpy.std's default)

D is the squared Euclidean distance in fp32 on the exact fp32 MFMA; no N x M matrix is stored.  There is no host fallback: the
inputs go to the device and a missing library is an error.  One host synchronisation per call, at the end."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops
from ._lib import SempyrError
from .config import METRIC_NAMES, parse_metrics

NAMES = METRIC_NAMES
PRDC_KEYS = ("precision", "recall", "density", "coverage")
IS_KEYS = ("inception_score", "inception_score_std")


def _device_set(x, device=None) -> torch.Tensor:
    """fp32 (n, d) on the device, contiguous, d padded with zero columns to a multiple of 4 (the kernels read d columns of ld)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if x.dim() != 2 or x.dtype != torch.float32:
        raise SempyrError("metrics take fp32 (n, d) activation sets, got %s %s" % (x.dtype, tuple(x.shape)))
    if not x.is_cuda:
        x = x.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    d = x.shape[1]
    if d % 4 != 0:
        x = torch.nn.functional.pad(x, (0, 4 - d % 4))
    return x.contiguous()


def _pair(real, fake):
    real_t = _device_set(real, fake.device if isinstance(fake, torch.Tensor) and fake.is_cuda else None)
    fake_t = _device_set(fake, real_t.device)
    d = real.shape[1]
    if fake.shape[1] != d:
        raise SempyrError("metrics: real has %d columns, fake %d" % (d, fake.shape[1]))
    return real_t, fake_t, d


def prdc(real, fake, nearest_k: int = 5) -> Dict[str, float]:
    """{"precision", "recall", "density", "coverage"} of two fp32 (N, d) / (M, d) sets: two sp_pairset_knn launches for the radii,
    ONE sp_pairset_cover pass (rows = fake, columns = real) for everything else."""
    real_t, fake_t, d = _pair(real, fake)
    n, m = real_t.shape[0], fake_t.shape[0]
    need = max(ops.pairset_workspace_bytes(n, n, d, nearest_k), ops.pairset_workspace_bytes(m, m, d, nearest_k),
               ops.pairset_workspace_bytes(m, n, d, 0))
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=real_t.device)
    rad_r = ops.pairset_knn(real_t, real_t, nearest_k, same=True, d=d, workspace=ws)
    rad_f = ops.pairset_knn(fake_t, fake_t, nearest_k, same=True, d=d, workspace=ws)
    row_count, col_count, _, col_min = ops.pairset_cover(fake_t, real_t, rad_a=rad_f, rad_b=rad_r, d=d, workspace=ws)
    sums = torch.stack([(row_count > 0).sum(), (col_count > 0).sum(), row_count.sum(dtype=torch.int64), (col_min <= rad_r).sum()])
    n_prec, n_rec, n_dens, n_cov = (int(v) for v in sums.cpu())          # the one synchronisation; ratios of integers from here
    return {"precision": n_prec / m, "recall": n_rec / n, "density": n_dens / (nearest_k * m), "coverage": n_cov / n}


def kid_indices(n_real: int, n_fake: int, num_subsets: int, max_subset_size: int, seed: int):
    """The pinned draw order: per subset m fake rows, then m real rows.  (idx_fake, idx_real) int32 (num_subsets, m), and m."""
    m = min(n_real, n_fake, max_subset_size)
    rs = np.random.RandomState(seed)
    ix = np.empty((num_subsets, m), dtype=np.int32)
    iy = np.empty((num_subsets, m), dtype=np.int32)
    for s in range(num_subsets):
        ix[s] = rs.choice(n_fake, m, replace=False)
        iy[s] = rs.choice(n_real, m, replace=False)
    return ix, iy, m


def kid_sums(real, fake, num_subsets: int = 100, max_subset_size: int = 1000, seed: int = 0):
    """The three Gram sums per subset, float64 (3, num_subsets) on the host - S_xx and S_yy without their diagonals, S_xy whole -
    and m: one batched sp_pairset_poly3 launch each."""
    real_t, fake_t, d = _pair(real, fake)
    ix, iy, m = kid_indices(real_t.shape[0], fake_t.shape[0], num_subsets, max_subset_size, seed)
    if m < 2:
        raise SempyrError("KID needs at least two rows per set")
    ixd, iyd = torch.from_numpy(ix).to(real_t.device), torch.from_numpy(iy).to(real_t.device)
    need = num_subsets * ops.pairset_workspace_bytes(m, m, d, 0)
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=real_t.device)
    sxx = ops.pairset_poly3(fake_t, ixd, fake_t, ixd, num_subsets, m, True, d=d, workspace=ws)
    syy = ops.pairset_poly3(real_t, iyd, real_t, iyd, num_subsets, m, True, d=d, workspace=ws)
    sxy = ops.pairset_poly3(fake_t, ixd, real_t, iyd, num_subsets, m, False, d=d, workspace=ws)
    return torch.stack([sxx, syy, sxy]).cpu().numpy(), m


def kid(real, fake, num_subsets: int = 100, max_subset_size: int = 1000, seed: int = 0) -> float:
    sums, m = kid_sums(real, fake, num_subsets, max_subset_size, seed)
    t = ((sums[0] + sums[1]) / (m - 1) - 2.0 * sums[2] / m).sum()
    return float(t / num_subsets / m)


def inception_kl(acts, weight, bias, splits: int = 10) -> np.ndarray:
    """KL_s of every split, float64 (splits,) on the host: sp_pairset_lse (log-sum-exp and sum p log p per row), then
    sp_pairset_softmax_colsum (the marginals and KL per split) - the (n, classes) logit matrix is formed twice and never stored.  One
    transfer and one synchronisation, at the end.  A non-finite logit makes its split's entry NaN."""
    acts_t = _device_set(acts, next((t.device for t in (weight, bias) if isinstance(t, torch.Tensor) and t.is_cuda), None))
    weight_t = _device_set(weight, acts_t.device)
    d = acts.shape[1]
    if weight.shape[1] != d:
        raise SempyrError("inception score: the rows have %d columns, the class rows %d" % (d, weight.shape[1]))
    if isinstance(bias, np.ndarray):
        bias = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))
    if bias.dim() != 1 or bias.dtype != torch.float32 or bias.shape[0] != weight_t.shape[0]:
        raise SempyrError("inception score: the bias is fp32 (%d,), got %s %s" % (weight_t.shape[0], bias.dtype, tuple(bias.shape)))
    bias_t = bias.to(acts_t.device).contiguous()
    n, classes = acts_t.shape[0], weight_t.shape[0]
    need = ops.pairset_softmax_workspace_bytes(n, classes, d, splits)
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=acts_t.device)
    lse, h = ops.pairset_lse(acts_t, weight_t, bias_t, d=d, workspace=ws)
    _, kl = ops.pairset_softmax_colsum(acts_t, weight_t, bias_t, lse, h, splits, d=d, workspace=ws)
    return kl.cpu().numpy()                                      # the one synchronisation


def inception_score_from_kl(kl) -> Dict[str, float]:
    scores = np.exp(np.asarray(kl, dtype=np.float64))
    return {"inception_score": float(scores.mean()), "inception_score_std": float(scores.std())}       # population form; a NaN split: both NaN


def inception_score(acts, weight, bias, splits: int = 10) -> Dict[str, float]:
    """{"inception_score", "inception_score_std"} of one fp32 (n, d) activation set under the classifier (weight (classes, d), bias)."""
    return inception_score_from_kl(inception_kl(acts, weight, bias, splits))


def compute(real, fake, names, nearest_k: int = 5, head=None, is_splits: int = 10, **kid_args) -> Dict[str, float]:
    """The metrics named in `names` (parse_metrics) as one flat dict: "kid", the four PRDC_KEYS and / or the two IS_KEYS ("is": of the
    fake set, under head = (weight, bias) - InceptionV3Features.classifier_head)."""
    out: Dict[str, float] = {}
    names = parse_metrics(names)
    if "is" in names and head is None:
        raise SempyrError("the Inception Score needs the classifier: the Inception-v3 state dict has no fc.weight / fc.bias")
    if "kid" in names:
        out["kid"] = kid(real, fake, **kid_args)
    if "prdc" in names:
        out.update(prdc(real, fake, nearest_k=nearest_k))
    if "is" in names:
        out.update(inception_score(fake, head[0], head[1], splits=is_splits))
    return out
