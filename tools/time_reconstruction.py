#!/usr/bin/env python3
"""Times ops.ssim_stats alone at the workload's shape - batch 40 x 3 x 256 x 256, scales 1 and 5, an fp32 NCHW
real batch against an fp32 NCHW or a 16-bit fake batch (the NCHW view of the generator's padded NHWC buffer) - against the SAME
definition written in torch on the same device in the same call: the separable 11-tap window as two grouped F.conv2d per moment,
the five moments, the two maps, float64 means, F.avg_pool2d for the next scale, the squared error.  Device events around one eager call
(all of its launches); 512 MB are overwritten in front of every timed call, so every source is read from memory; 13 calls each.
The two sides are checked against each other before they are timed.  Needs a GPU.

Bytes: what the definition must move - per scale each image once (scale 0 in the sources' types, fp32 below) and the pooled planes written
once; the halo a tile re-reads (26 x 42 pixels staged per 16 x 32 positions, 2.1x) is not counted, it is served by the caches or it
is the kernel's own overhead.  The HBM fraction is those bytes over the median time over 8.0 TB/s (the part's specified rate).

    python3 tools/time_reconstruction.py [--batch 40] [--size 256] [--calls 13]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def window(device):
    e = [math.exp(-(k - 5) ** 2 / 4.5) for k in range(11)]
    return torch.tensor([v / sum(e) for v in e], dtype=torch.float64).float().to(device)


def torch_stats(x, y, scales, data_range=2.0):
    """The definition of include/sempyr.h's sp_ssim_stats in torch ops: (ssim_mean, cs_mean, sqerr), float64."""
    x, y = x.float(), y.float()
    n, c = x.shape[:2]
    g = window(x.device)
    kh, kv = g.view(1, 1, 1, 11).repeat(c, 1, 1, 1), g.view(1, 1, 11, 1).repeat(c, 1, 1, 1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    d = x - y
    sqerr = (d.double() * d.double()).sum(dim=(2, 3))
    ssim_mean, cs_mean = [], []
    for j in range(scales):
        f = lambda v: F.conv2d(F.conv2d(v, kh, groups=c), kv, groups=c)        # noqa: E731
        mx, my, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        mxx, myy, mxy = mx * mx, my * my, mx * my
        cs = (2 * (exy - mxy) + c2) / ((exx - mxx) + (eyy - myy) + c2)
        ssim = (2 * mxy + c1) / (mxx + myy + c1) * cs
        cs_mean.append(cs.double().mean(dim=(2, 3)))
        ssim_mean.append(ssim.double().mean(dim=(2, 3)))
        if j + 1 < scales:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return torch.stack(ssim_mean, dim=2), torch.stack(cs_mean, dim=2), sqerr


def needed_bytes(n, c, h, w, scales, x_bytes, y_bytes):
    total = n * c * h * w * (x_bytes + y_bytes)
    for j in range(1, scales):
        plane = n * c * (h >> j) * (w >> j) * 4
        total += 2 * plane * 2                             # both images: written once by scale j - 1, read once by scale j
    return total


def timed(fn, flush, calls):
    out = []
    for _ in range(calls + 2):                             # two calls in front: code objects, allocator, algorithm choice
        flush.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out = out[2:]
    return {"min_us": round(min(out), 1), "median_us": round(statistics.median(out), 1), "max_us": round(max(out), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=13)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reconstruction.py measures on the GPU; there is none here")
    n, s = args.batch, args.size
    real = torch.rand(n, 3, s, s, device="cuda") * 2 - 1
    fake32 = (0.7 * real + 0.3 * (torch.rand(n, 3, s, s, device="cuda") * 2 - 1)).contiguous()
    cp = ops.pad_channels(3, torch.bfloat16)
    nhwc = torch.zeros(n, s, s, cp, device="cuda", dtype=torch.bfloat16)
    nhwc[..., :3] = fake32.permute(0, 2, 3, 1).to(torch.bfloat16)
    fake16 = nhwc[..., :3].permute(0, 3, 1, 2)             # the generator's output form: an NCHW view of a padded NHWC buffer
    flush = torch.zeros(128 << 20, dtype=torch.int32, device="cuda")      # 512 MB
    print(json.dumps({"batch": n, "size": s, "calls": args.calls, "hbm_bytes_per_s": HBM_BYTES_PER_S}), flush=True)
    for scales in (1, 5):
        ws = torch.empty(ops.ssim_workspace_bytes(n, 3, s, s, scales) // 8 + 1, dtype=torch.float64, device="cuda")
        for name, fake, y_bytes in (("fp32", fake32, 4), ("bf16 nhwc view", fake16, 2)):
            got, want = ops.ssim_stats(real, fake, scales=scales, workspace=ws), torch_stats(real, fake, scales)
            agree = max((a - b).abs().max().item() for a, b in zip(got[:2], want[:2]))
            rel_sq = ((got[2] - want[2]).abs() / want[2]).max().item()
            need = needed_bytes(n, 3, s, s, scales, 4, y_bytes)
            for what, fn in (("sp_ssim_stats", lambda: ops.ssim_stats(real, fake, scales=scales, workspace=ws)),
                             ("torch conv2d form", lambda: torch_stats(real, fake, scales))):
                rec = timed(fn, flush, args.calls)
                rec.update(what=what, scales=scales, fake=name, needed_bytes=need,
                           needed_GB_per_s=round(need / rec["median_us"] / 1e3, 1),
                           hbm_fraction=round(need / (rec["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4),
                           max_abs_diff_of_the_two_sides=agree, max_rel_diff_sqerr=rel_sq)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
