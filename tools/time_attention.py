#!/usr/bin/env python3
"""Times sp_attention_fwd and sp_attention_bwd alone (csrc/attention.hip) at the workload's shape and a few others: device events
around 50 back-to-back calls (the operands stay in the caches, as they are behind the 1x1 convolutions of the step), 9 such windows
each, us per call.  SEMPYR_LIB selects the library, so two builds are compared by alternating processes; with a library that has
SP_TUNE_ATTN_PIECES the piece counts in --pieces are forced one after the other (-1 = the plan).  --phases: the TIMING build of the
one-slab-per-query-block backward (SP_TUNE_ATTN_PIECES = 4096) per shape and the cycles per wave it counted in each phase, averaged
over every wave of every block.  Needs a GPU.

    python3 tools/time_attention.py [--dtype bf16|fp16] [--pieces=-1,16,8,4] [--phases] [--shapes n,nk,d,dv,batch ...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_pyramid_for_image_generation_amd import _lib as L, ops  # noqa: E402

SHAPES = ["1024,256,32,128,20", "1024,256,32,128,40", "1024,256,32,128,8", "1024,256,32,128,4", "256,64,32,64,40", "4096,256,32,64,4"]
KEY = 30          # SP_TUNE_ATTN_PIECES (include/sempyr.h); a library from before it rejects the key


def window(fn, calls=50, windows=9):
    for _ in range(5):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return {"min_us": round(min(out), 2), "median_us": round(statistics.median(out), 2), "max_us": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--pieces", default="-1")
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_attention.py measures on the GPU; there is none here")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    sp = ops.sp_dtype(dt)
    has_key = L.lib().sp_set_tuning(KEY, -1) == 0
    pieces = [int(p) for p in args.pieces.split(",")] if has_key else [-1]
    print(json.dumps({"library": os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH), "dtype": args.dtype,
                      "has_pieces_key": has_key}), flush=True)
    for shape in args.shapes:
        n, nk, d, dv, b = (int(x) for x in shape.split(","))
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device="cuda") * scale).to(dt)      # noqa: E731
        q, k, v, do = rnd(b, n, d, scale=0.7), rnd(b, nk, d, scale=0.7), rnd(b, nk, dv), rnd(b, n, dv)
        o, dq, dk, dvo = torch.empty_like(do), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        lse = torch.empty(b, n, device="cuda")
        slabs = ctypes.c_int64(-1)
        L.call("sp_attention_bwd_slabs", n, nk, d, dv, sp, ctypes.byref(slabs))
        dk32 = torch.empty(slabs.value, b, nk, d, device="cuda")
        dv32 = torch.empty(slabs.value, b, nk, dv, device="cuda")
        fwd = lambda: L.call("sp_attention_fwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(o), ops.ptr(lse), b, n, nk, d, dv, sp, ops.stream())      # noqa: E731
        bwd = lambda: L.call("sp_attention_bwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(do), ops.ptr(lse), ops.ptr(dq), ops.ptr(dk32),      # noqa: E731
                             ops.ptr(dv32), ops.ptr(dk), ops.ptr(dvo), b, n, nk, d, dv, sp, ops.stream())
        if args.phases:
            if not has_key:
                raise SystemExit("--phases needs a library with SP_TUNE_ATTN_PIECES")
            fwd()
            L.call("sp_set_tuning", KEY, 4096)
            try:
                bwd()
                bwd()
                torch.cuda.synchronize()
            finally:
                L.call("sp_set_tuning", KEY, -1)
            c = dk32.view(slabs.value * b, nk * d)[:, :32].view(-1, 4, 8)[:, :, :6].double().cpu()      # [block][wave][phase]
            tot = c.sum(2)
            rec = {"shape": shape, "what": "phases of attn_bwd_mfma_kernel<TIMING>", "blocks": c.shape[0],
                   "cycles_per_wave_mean": [round(float(x), 0) for x in c.mean((0, 1))],
                   "share": [round(float(x), 3) for x in (c.sum((0, 1)) / c.sum())],
                   "phases": ["stage K Q dO V + barrier", "phase 1 to dS", "dQ + stores", "phase 2 + barriers", "phase 3 dV + slab stores", "phase 3 dK + stores"],
                   "total_cycles_per_wave": {"min": float(tot.min()), "mean": round(float(tot.mean()), 0), "max": float(tot.max())}}
            print(json.dumps(rec), flush=True)
            continue
        for p in pieces:
            if has_key:
                L.call("sp_set_tuning", KEY, p)
            for name, fn in (("fwd", fwd), ("bwd+reduce", bwd)):
                rec = window(fn)
                rec.update(shape=shape, pieces=p, what=name)
                print(json.dumps(rec), flush=True)
        if has_key:
            L.call("sp_set_tuning", KEY, -1)


if __name__ == "__main__":
    main()
