"""Independent CPU restatement of torchvision's Inception3 (eval mode, transform_input=False) up to Mixed_7c + the global average,
i.e. /root/reference/frechet_inception_distance.py:11-42, written with torch.nn.functional only (torchvision is not installed).
The GPU path (semantic_pyramid_for_image_generation_amd/inception.py) is held to it by tests/test_gpu_fid.py.

Also: a seeded generator of a full torchvision-keyed inception_v3 state dict (AuxLogits and fc included).  The BatchNorm
statistics are deliberately not the identity, so that a folding mistake shows, and the conv weights are He-scaled, so that the
activations stay O(1) through the 94 layers."""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn.functional as F

TOTAL_PARAMS = 27_161_264          # torchvision's published inception_v3 parameter count (AuxLogits and fc included)
FEATURE_PARAMS = 21_785_568        # ... of the part up to Mixed_7c


def basic_convs():
    """(name, cin, cout, (kh, kw)) of every BasicConv2d, in torchvision's module order, AuxLogits included."""
    out = []

    def c(name, cin, cout, k):
        out.append((name, cin, cout, k if isinstance(k, tuple) else (k, k)))

    c("Conv2d_1a_3x3", 3, 32, 3); c("Conv2d_2a_3x3", 32, 32, 3); c("Conv2d_2b_3x3", 32, 64, 3)
    c("Conv2d_3b_1x1", 64, 80, 1); c("Conv2d_4a_3x3", 80, 192, 3)
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(blk + ".branch1x1", cin, 64, 1)
        c(blk + ".branch5x5_1", cin, 48, 1); c(blk + ".branch5x5_2", 48, 64, 5)
        c(blk + ".branch3x3dbl_1", cin, 64, 1); c(blk + ".branch3x3dbl_2", 64, 96, 3); c(blk + ".branch3x3dbl_3", 96, 96, 3)
        c(blk + ".branch_pool", cin, pf, 1)
    c("Mixed_6a.branch3x3", 288, 384, 3)
    c("Mixed_6a.branch3x3dbl_1", 288, 64, 1); c("Mixed_6a.branch3x3dbl_2", 64, 96, 3); c("Mixed_6a.branch3x3dbl_3", 96, 96, 3)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(blk + ".branch1x1", 768, 192, 1)
        c(blk + ".branch7x7_1", 768, c7, 1); c(blk + ".branch7x7_2", c7, c7, (1, 7)); c(blk + ".branch7x7_3", c7, 192, (7, 1))
        c(blk + ".branch7x7dbl_1", 768, c7, 1); c(blk + ".branch7x7dbl_2", c7, c7, (7, 1)); c(blk + ".branch7x7dbl_3", c7, c7, (1, 7))
        c(blk + ".branch7x7dbl_4", c7, c7, (7, 1)); c(blk + ".branch7x7dbl_5", c7, 192, (1, 7))
        c(blk + ".branch_pool", 768, 192, 1)
    c("AuxLogits.conv0", 768, 128, 1); c("AuxLogits.conv1", 128, 768, 5)
    c("Mixed_7a.branch3x3_1", 768, 192, 1); c("Mixed_7a.branch3x3_2", 192, 320, 3)
    c("Mixed_7a.branch7x7x3_1", 768, 192, 1); c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1)); c("Mixed_7a.branch7x7x3_4", 192, 192, 3)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(blk + ".branch1x1", cin, 320, 1)
        c(blk + ".branch3x3_1", cin, 384, 1); c(blk + ".branch3x3_2a", 384, 384, (1, 3)); c(blk + ".branch3x3_2b", 384, 384, (3, 1))
        c(blk + ".branch3x3dbl_1", cin, 448, 1); c(blk + ".branch3x3dbl_2", 448, 384, 3)
        c(blk + ".branch3x3dbl_3a", 384, 384, (1, 3)); c(blk + ".branch3x3dbl_3b", 384, 384, (3, 1))
        c(blk + ".branch_pool", cin, 192, 1)
    return out


def synth_state_dict(seed: int = 0, with_aux: bool = True, with_fc: bool = True, with_nbt: bool = True) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, cin, cout, (kh, kw) in basic_convs():
        if name.startswith("AuxLogits.") and not with_aux:
            continue
        fan_in = cin * kh * kw
        sd[name + ".conv.weight"] = torch.randn((cout, cin, kh, kw), generator=g) * (2.0 / fan_in) ** 0.5
        sd[name + ".bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_var"] = 0.5 + 1.5 * torch.rand(cout, generator=g)
        if with_nbt:
            sd[name + ".bn.num_batches_tracked"] = torch.tensor(1000, dtype=torch.int64)
    if with_aux:
        sd["AuxLogits.fc.weight"] = 0.01 * torch.randn((1000, 768), generator=g)
        sd["AuxLogits.fc.bias"] = torch.zeros(1000)
    if with_fc:
        sd["fc.weight"] = 0.01 * torch.randn((1000, 2048), generator=g)
        sd["fc.bias"] = torch.zeros(1000)
    return sd


def param_count(sd, features_only: bool = False) -> int:
    """Parameters (not buffers) of the state dict, as sum(p.numel() for p in model.parameters()) counts them."""
    n = 0
    for k, v in sd.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        if features_only and k.startswith(("AuxLogits.", "fc.")):
            continue
        n += v.numel()
    return n


def _bc(sd, name, x, stride=1, padding=0):
    x = F.conv2d(x, sd[name + ".conv.weight"].to(x.dtype), stride=stride, padding=padding)
    p = lambda k: sd[name + ".bn." + k].to(x.dtype)      # noqa: E731
    x = F.batch_norm(x, p("running_mean"), p("running_var"), p("weight"), p("bias"), training=False, eps=0.001)
    return F.relu(x)


def _pool(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1)      # count_include_pad=True (torch's default)


def inception_a(sd, b, x):
    return torch.cat([_bc(sd, b + ".branch1x1", x),
                      _bc(sd, b + ".branch5x5_2", _bc(sd, b + ".branch5x5_1", x), padding=2),
                      _bc(sd, b + ".branch3x3dbl_3", _bc(sd, b + ".branch3x3dbl_2", _bc(sd, b + ".branch3x3dbl_1", x), padding=1), padding=1),
                      _bc(sd, b + ".branch_pool", _pool(x))], 1)


def inception_b(sd, b, x):
    return torch.cat([_bc(sd, b + ".branch3x3", x, stride=2),
                      _bc(sd, b + ".branch3x3dbl_3", _bc(sd, b + ".branch3x3dbl_2", _bc(sd, b + ".branch3x3dbl_1", x), padding=1), stride=2),
                      F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_c(sd, b, x):
    b7 = _bc(sd, b + ".branch7x7_1", x)
    b7 = _bc(sd, b + ".branch7x7_2", b7, padding=(0, 3))
    b7 = _bc(sd, b + ".branch7x7_3", b7, padding=(3, 0))
    d = _bc(sd, b + ".branch7x7dbl_1", x)
    d = _bc(sd, b + ".branch7x7dbl_2", d, padding=(3, 0))
    d = _bc(sd, b + ".branch7x7dbl_3", d, padding=(0, 3))
    d = _bc(sd, b + ".branch7x7dbl_4", d, padding=(3, 0))
    d = _bc(sd, b + ".branch7x7dbl_5", d, padding=(0, 3))
    return torch.cat([_bc(sd, b + ".branch1x1", x), b7, d, _bc(sd, b + ".branch_pool", _pool(x))], 1)


def inception_d(sd, b, x):
    b3 = _bc(sd, b + ".branch3x3_2", _bc(sd, b + ".branch3x3_1", x), stride=2)
    b7 = _bc(sd, b + ".branch7x7x3_1", x)
    b7 = _bc(sd, b + ".branch7x7x3_2", b7, padding=(0, 3))
    b7 = _bc(sd, b + ".branch7x7x3_3", b7, padding=(3, 0))
    b7 = _bc(sd, b + ".branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_e(sd, b, x):
    b3 = _bc(sd, b + ".branch3x3_1", x)
    b3 = torch.cat([_bc(sd, b + ".branch3x3_2a", b3, padding=(0, 1)), _bc(sd, b + ".branch3x3_2b", b3, padding=(1, 0))], 1)
    d = _bc(sd, b + ".branch3x3dbl_2", _bc(sd, b + ".branch3x3dbl_1", x), padding=1)
    d = torch.cat([_bc(sd, b + ".branch3x3dbl_3a", d, padding=(0, 1)), _bc(sd, b + ".branch3x3dbl_3b", d, padding=(1, 0))], 1)
    return torch.cat([_bc(sd, b + ".branch1x1", x), b3, d, _bc(sd, b + ".branch_pool", _pool(x))], 1)


def normalize_m1_1_batch(x):
    """/root/reference/misc.py:112-121, verbatim arithmetic."""
    f = x.view(x.shape[0], -1)
    mn, mx = torch.min(f, dim=1)[0][:, None, None, None], torch.max(f, dim=1)[0][:, None, None, None]
    return 2 * ((x - mn) / (mx - mn)) - 1


def prepare(images):
    """frechet_inception_distance.py:71-77 in fp32."""
    x = normalize_m1_1_batch(images.float())
    if x.shape[2] != 299 or x.shape[3] != 299:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    return x


def features(sd, x):
    """Mixed_7c activations averaged to (B, 2048); x is the prepared (B, 3, 299, 299) input."""
    x = _bc(sd, "Conv2d_1a_3x3", x, stride=2)
    x = _bc(sd, "Conv2d_2a_3x3", x)
    x = _bc(sd, "Conv2d_2b_3x3", x, padding=1)
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = _bc(sd, "Conv2d_3b_1x1", x)
    x = _bc(sd, "Conv2d_4a_3x3", x)
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = inception_a(sd, b, x)
    x = inception_b(sd, "Mixed_6a", x)
    for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = inception_c(sd, b, x)
    x = inception_d(sd, "Mixed_7a", x)
    x = inception_e(sd, "Mixed_7b", x)
    x = inception_e(sd, "Mixed_7c", x)
    return F.adaptive_avg_pool2d(x, (1, 1)).view(x.shape[0], 2048)
