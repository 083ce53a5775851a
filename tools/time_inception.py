#!/usr/bin/env python3
"""Throughput of the FID's Inception-v3 feature extractor (semantic_pyramid_for_image_generation_amd/inception.py).

    python tools/time_inception.py [--batch 40] [--iters 20] [--validate-images 6000]

Prints one JSON line per mode: images / s at the given batch and the fraction of the 2.5 PFLOP/s bf16 dense MFMA peak at
11.42 GFLOP per 299 x 299 image, for the library's kernels in fp32 and bf16 and for torch's own GPU F.conv2d path on the same
(folded) network as a yardstick; then the wall time of one ModelWrapper.validate() over --validate-images synthetic validation
images (batch 40, channel factor 1 generator, bf16).  Random weights: the timing does not depend on their values.  Every GPU step
runs in a child process under `timeout` (tools/time_inception.py --child <mode>), so a stuck step ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GFLOP_PER_IMAGE = 11.42
PEAK_BF16 = 2.5e15


def _time(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def child(mode, batch, iters, n_validate):
    import torch
    import torch.nn.functional as F
    import inception_restated as R
    from semantic_pyramid_for_image_generation_amd import inception, ops
    torch.cuda.set_device(0)
    sd = R.synth_state_dict(0)
    images = (torch.rand((batch, 3, 256, 256)) * 2 - 1).cuda()
    out = {"mode": mode, "batch": batch}
    if mode in ("fp32", "bf16", "fp16"):
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
        net = inception.InceptionV3Features(sd, dtype=dt)
        sec = _time(lambda: net(images), iters)
    elif mode.startswith("torch_"):
        dt = torch.float32 if mode == "torch_fp32" else torch.bfloat16
        folded = {k: (w.to(dt).cuda(), b.to(dt).cuda()) for k, (w, b) in inception.fold_state_dict(sd).items()}
        spec = {n: (s, p) for n, _, _, _, s, p in inception.CONV_LAYERS}

        def bc(_sd, name, x, stride=1, padding=0):     # the restatement's conv -> BN -> ReLU with the BN folded: conv + bias -> ReLU
            w, b = folded[name]
            return F.relu(F.conv2d(x, w, b, stride=stride, padding=padding))
        R._bc = bc
        x = R.prepare(images).to(dt).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            sec = _time(lambda: R.features(None, x), iters)
    elif mode == "validate":
        from semantic_pyramid_for_image_generation_amd import params, synthetic
        import semantic_pyramid_for_image_generation_amd as sp
        from oracle import sempyr_oracle as O
        ops.set_compute_dtype(torch.bfloat16)
        G, D, V = sp.Generator(channels_factor=1), sp.Discriminator(channel_factor=1), sp.VGG16()
        G.load_state_dict(params.synth_state_dict(O.layout_template(O.generator_layout(1)), 0))
        D.load_state_dict(params.synth_state_dict(O.layout_template(O.discriminator_layout(1)), 1))
        V.load_state_dict(params.synth_state_dict(O.layout_template(O.vgg16_layout()), 2))
        G.cuda(); D.cuda(); V.cuda().eval()
        b = 40
        proto = synthetic.synthetic_batch(b, 0)

        class Loader:                # n_validate images in batches of 40, like main.py:84-87's validation loader
            def __iter__(self):
                for _ in range(n_validate // b):
                    yield proto[0], proto[1], list(proto[2])
        mw = sp.ModelWrapper(G, D, None, Loader(), vgg16=V, save_data_path=None,
                             inception=inception.InceptionV3Features(sd, dtype=torch.bfloat16))
        t0 = time.perf_counter()
        fid = mw.validate()
        torch.cuda.synchronize()
        out.update(images=n_validate // b * b, seconds=round(time.perf_counter() - t0, 2), fid=fid)
        print(json.dumps(out), flush=True)
        return
    out.update(img_per_s=round(batch / sec, 1), ms_per_batch=round(sec * 1e3, 3),
               frac_of_bf16_peak=round(batch / sec * GFLOP_PER_IMAGE * 1e9 / PEAK_BF16, 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--validate-images", type=int, default=6000)
    ap.add_argument("--modes", default="bf16,fp32,fp16,torch_bf16,torch_fp32,validate")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.batch, a.iters, a.validate_images)
        return
    for mode in a.modes.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--batch", str(a.batch),
               "--iters", str(a.iters), "--validate-images", str(a.validate_images)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"mode": mode, "error": "exit status %d" % rc}), flush=True)
            sys.exit(1)                 # a failed / stuck GPU step ends the run


if __name__ == "__main__":
    main()
