#!/usr/bin/env python3
"""Times sp_apa_select alone: batch 20, 256 x 256, an fp32 NCHW real batch and the generator's 16-bit fake batch
(the NCHW view of its padded NHWC buffer), against a plain torch device copy of the same fp32 batch (dst.copy_(real)) in the same call.
Device events around one eager launch; 512 MB are overwritten in front of every timed call, so every source is read from memory;
13 calls each; the selections p = 0 (every image real), 0.5 (w_u alternating around it) and 1 (every image fake).  Needs a GPU.

    python3 tools/time_apa.py [--batch 20] [--size 256] [--dtype bf16|fp16|fp32] [--calls 13]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402


def timed(fn, flush, calls):
    out = []
    for _ in range(calls + 2):                             # two calls in front: code object, allocator
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
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=("bf16", "fp16", "fp32"), default="bf16")
    ap.add_argument("--calls", type=int, default=13)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_apa.py measures on the GPU; there is none here")
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    n, s = args.batch, args.size
    real = torch.randn(n, 3, s, s, device="cuda")
    cp = ops.pad_channels(3, dtype)
    fake = torch.randn(n, s, s, cp, device="cuda").to(dtype)[..., :3].permute(0, 3, 1, 2)
    dst = torch.empty(n, 3, s, s, device="cuda")
    flush = torch.zeros(128 << 20, dtype=torch.int32, device="cuda")      # 512 MB
    alternating = torch.tensor([0.25, 0.75] * n, device="cuda")[:n].contiguous()
    p = torch.zeros(1, device="cuda")
    batch_bytes = real.numel() * 4
    print(json.dumps({"batch": n, "size": s, "fake_dtype": args.dtype, "fp32_batch_bytes": batch_bytes, "calls": args.calls}), flush=True)
    rows = [("torch dst.copy_(real)", lambda: dst.copy_(real), None)]
    for value, name in ((0.0, "p = 0 (all real)"), (0.5, "p = 0.5 (alternating)"), (1.0, "p = 1 (all fake)")):
        rows.append(("sp_apa_select " + name, lambda: ops.apa_select(real, fake, alternating, p, out=dst), value))
    for name, fn, value in rows:
        if value is not None:
            p.fill_(value)
        rec = timed(fn, flush, args.calls)
        rec["what"] = name
        rec["GB_per_s_of_2x_fp32_batch"] = round(2 * batch_bytes / rec["median_us"] / 1e3, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
