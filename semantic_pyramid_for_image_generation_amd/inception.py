"""Inception-v3 feature extractor of the FID metric on the library's kernels (/root/reference/frechet_inception_distance.py:11-42).

The reference builds ``torchvision.models.inception_v3(pretrained=True, transform_input=False)``, hooks ``Mixed_7c`` and takes
``adaptive_avg_pool2d(., 1)`` -> (B, 2048).  ``InceptionV3Features`` restates exactly that network in eval mode, forward only:

  * it reads a torchvision-keyed ``inception_v3`` state dict (a path for ``torch.load`` or a dict) - the file torchvision's
    download leaves in torch's hub cache; ``AuxLogits.*`` (not run in eval mode) and ``num_batches_tracked`` are ignored;
    ``fc.weight`` / ``fc.bias`` (the reference computes the logits and never uses them) are no part of the forward either, but are
    kept as the classifier head of the Inception Score (``classifier_head``, metrics.py) when both are present;
  * every BasicConv2d (conv without bias -> BatchNorm2d(eps=0.001) -> ReLU) is folded on the host in float64 into packed
    weights [cout][kh*kw][cin_p] in the compute dtype and an fp32 bias, once;
  * ``forward(images)`` takes NCHW fp32 images on the device (any size; they are normalised per image to [-1, 1] and resized
    to 299 x 299 bilinearly, frechet_inception_distance.py:71-77) and returns the (B, 2048) fp32 activations.

Activations are NHWC in the compute dtype; each Inception block's branches store into channel slices of the block's output,
so the concatenations cost nothing (include/sempyr.h: sp_conv2d_general, sp_maxpool3s2_fwd, sp_avgpool3s1_fwd,
sp_inception_prep, sp_global_avgpool_f32).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Mapping, Optional, Tuple, Union

import torch

from . import _lib as L
from . import ops
from ._lib import SempyrError

BN_EPS = 1e-3
INPUT_SIZE = 299
FEATURES = 2048
CLASSES = 1000                                      # torchvision's classifier, not the TF graph's 1008


def _conv_table() -> List[Tuple[str, int, int, Tuple[int, int], int, Tuple[int, int]]]:
    """(layer, cin, cout, (kh, kw), stride, (pad_h, pad_w)) of the 94 BasicConv2d of torchvision's Inception3 up to Mixed_7c."""
    t = []

    def c(name, cin, cout, k, s=1, p=(0, 0)):
        t.append((name, cin, cout, k if isinstance(k, tuple) else (k, k), s, p if isinstance(p, tuple) else (p, p)))

    c("Conv2d_1a_3x3", 3, 32, 3, s=2)
    c("Conv2d_2a_3x3", 32, 32, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, p=1)
    c("Conv2d_3b_1x1", 64, 80, 1)
    c("Conv2d_4a_3x3", 80, 192, 3)
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(blk + ".branch1x1", cin, 64, 1)
        c(blk + ".branch5x5_1", cin, 48, 1)
        c(blk + ".branch5x5_2", 48, 64, 5, p=2)
        c(blk + ".branch3x3dbl_1", cin, 64, 1)
        c(blk + ".branch3x3dbl_2", 64, 96, 3, p=1)
        c(blk + ".branch3x3dbl_3", 96, 96, 3, p=1)
        c(blk + ".branch_pool", cin, pf, 1)
    c("Mixed_6a.branch3x3", 288, 384, 3, s=2)
    c("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, p=1)
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, s=2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(blk + ".branch1x1", 768, 192, 1)
        c(blk + ".branch7x7_1", 768, c7, 1)
        c(blk + ".branch7x7_2", c7, c7, (1, 7), p=(0, 3))
        c(blk + ".branch7x7_3", c7, 192, (7, 1), p=(3, 0))
        c(blk + ".branch7x7dbl_1", 768, c7, 1)
        c(blk + ".branch7x7dbl_2", c7, c7, (7, 1), p=(3, 0))
        c(blk + ".branch7x7dbl_3", c7, c7, (1, 7), p=(0, 3))
        c(blk + ".branch7x7dbl_4", c7, c7, (7, 1), p=(3, 0))
        c(blk + ".branch7x7dbl_5", c7, 192, (1, 7), p=(0, 3))
        c(blk + ".branch_pool", 768, 192, 1)
    c("Mixed_7a.branch3x3_1", 768, 192, 1)
    c("Mixed_7a.branch3x3_2", 192, 320, 3, s=2)
    c("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), p=(0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), p=(3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, s=2)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(blk + ".branch1x1", cin, 320, 1)
        c(blk + ".branch3x3_1", cin, 384, 1)
        c(blk + ".branch3x3_2a", 384, 384, (1, 3), p=(0, 1))
        c(blk + ".branch3x3_2b", 384, 384, (3, 1), p=(1, 0))
        c(blk + ".branch3x3dbl_1", cin, 448, 1)
        c(blk + ".branch3x3dbl_2", 448, 384, 3, p=1)
        c(blk + ".branch3x3dbl_3a", 384, 384, (1, 3), p=(0, 1))
        c(blk + ".branch3x3dbl_3b", 384, 384, (3, 1), p=(1, 0))
        c(blk + ".branch_pool", cin, 192, 1)
    return t


CONV_LAYERS = _conv_table()
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
_IGNORED_PREFIXES = ("AuxLogits.", "fc.")


def fold_bn(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor,
            eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """BatchNorm2d in eval form folded into the bias-free convolution before it, in float64:
    bn(conv(x, w)) = conv(x, w * s) + (beta - mean * s), s = gamma / sqrt(var + eps)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s[:, None, None, None], beta.double() - mean.double() * s


def _cin_p(cin: int) -> int:
    return ops.pad_to(cin, 8)


def pack_conv(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """OIHW -> [cout][kh*kw][cin_p] (cin_p = cin rounded up to 8, pad channels zero) in `dtype`, flattened per output channel."""
    cout, cin, kh, kw = w.shape
    cp = _cin_p(cin)
    out = torch.zeros((cout, kh, kw, cp), dtype=torch.float64)
    out[..., :cin] = w.permute(0, 2, 3, 1)
    return out.reshape(cout, kh * kw * cp).to(dtype).contiguous()


def _load(weights) -> Mapping[str, torch.Tensor]:
    if isinstance(weights, Mapping):
        return weights
    try:
        sd = torch.load(weights, map_location="cpu")
    except Exception as e:                          # noqa: BLE001 - reported with the path
        raise SempyrError("cannot read Inception-v3 weights from %r: %s" % (weights, e)) from e
    if not isinstance(sd, Mapping):
        raise SempyrError("%r holds a %s, not a state dict" % (weights, type(sd).__name__))
    return sd


def fold_state_dict(weights) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """layer -> (folded OIHW weight, bias), float64, from a torchvision-keyed inception_v3 state dict; a missing, mis-shaped or
    unknown key raises SempyrError naming it."""
    sd = _load(weights)
    known = set()
    out = {}
    for name, cin, cout, (kh, kw), _, _ in CONV_LAYERS:
        want = {name + ".conv.weight": (cout, cin, kh, kw)}
        want.update({"%s.bn.%s" % (name, k): (cout,) for k in BN_KEYS})
        for key, shape in want.items():
            if key not in sd:
                raise SempyrError("Inception-v3 state dict: missing key %s" % key)
            got = tuple(sd[key].shape)
            if got != shape:
                raise SempyrError("Inception-v3 state dict: %s has shape %s, expected %s" % (key, got, shape))
        known.update(want)
        g = lambda k: sd["%s.bn.%s" % (name, k)]       # noqa: E731
        out[name] = fold_bn(sd[name + ".conv.weight"], g("weight"), g("bias"), g("running_mean"), g("running_var"))
    for key in sd:
        if key not in known and not key.startswith(_IGNORED_PREFIXES) and not key.endswith(".num_batches_tracked"):
            raise SempyrError("Inception-v3 state dict: unexpected key %s (not part of torchvision's inception_v3)" % key)
    return out


def classifier_head(weights) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """(fc.weight (1000, 2048), fc.bias (1000,)) as contiguous fp32 host tensors from a torchvision-keyed inception_v3 state dict, or
    None when it has neither; one without the other, or a mis-shaped one, raises SempyrError naming the key."""
    sd = _load(weights)
    want = {"fc.weight": (CLASSES, FEATURES), "fc.bias": (CLASSES,)}
    have = [k for k in want if k in sd]
    if not have:
        return None
    for key, shape in want.items():
        if key not in sd:
            raise SempyrError("Inception-v3 state dict: %s without %s" % (have[0], key))
        got = tuple(sd[key].shape)
        if got != shape:
            raise SempyrError("Inception-v3 state dict: %s has shape %s, expected %s" % (key, got, shape))
    return sd["fc.weight"].detach().float().contiguous(), sd["fc.bias"].detach().float().contiguous()


class InceptionV3Features:
    """(B, 3, H, W) fp32 images -> (B, 2048) fp32 Mixed_7c activations, averaged over 8 x 8 (frechet_inception_distance.py:38-41)."""

    def __init__(self, weights: Union[str, Mapping[str, torch.Tensor]], dtype: Optional[torch.dtype] = None):
        self.dtype = dtype if dtype is not None else ops.compute_dtype()
        ops.sp_dtype(self.dtype)                   # float32 / bfloat16 / float16 only
        self._spec = {name: (cin, cout, k, s, p) for name, cin, cout, k, s, p in CONV_LAYERS}
        self._host = {}
        weights = _load(weights)
        for name, (w, b) in fold_state_dict(weights).items():
            self._host[name] = (pack_conv(w, self.dtype), b.float().contiguous())
        self._dev = {}                              # device -> {layer: (packed weight, bias)}
        self._head_host = classifier_head(weights)  # fp32 whatever the compute dtype: the logits of the Inception Score
        self._head_dev = {}                         # device -> (weight, bias)

    # ---- building blocks ------------------------------------------------------------------------------------------------------
    def _params(self, device) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {n: (w.to(device), b.to(device)) for n, (w, b) in self._host.items()}
        return self._dev[key]

    def classifier_head(self, device) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(fc.weight (1000, 2048), fc.bias (1000,)) in fp32 on `device`, uploaded once; None when the state dict had no fc.*."""
        if self._head_host is None:
            return None
        key = str(device)
        if key not in self._head_dev:
            self._head_dev[key] = tuple(t.to(device) for t in self._head_host)
        return self._head_dev[key]

    def _conv(self, name: str, x: torch.Tensor, out: Optional[torch.Tensor] = None, off: int = 0) -> torch.Tensor:
        cin, cout, (kh, kw), s, (ph, pw) = self._spec[name]
        n, h, w, ldx = x.shape
        oh, ow = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
        if out is None:
            out = torch.empty((n, oh, ow, cout), dtype=self.dtype, device=x.device)
        wt, b = self._p[name]
        prm = L.SpConvGeneralParams(dtype=ops.sp_dtype(self.dtype), x=x.data_ptr(), w=wt.data_ptr(), bias=b.data_ptr(),
                                    y=out.data_ptr() + off * out.element_size(), n=n, h=h, w_=w, cin_p=_cin_p(cin), ldx=ldx,
                                    cout=cout, ldy=out.shape[3], kh=kh, kw=kw, stride_h=s, stride_w=s, pad_h=ph, pad_w=pw,
                                    act=L.ACT_RELU)
        L.call("sp_conv2d_general", ctypes.byref(prm), ops.stream())
        return out

    def _maxpool(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, off: int = 0) -> torch.Tensor:
        n, h, w, c = x.shape
        if out is None:
            out = torch.empty((n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), dtype=self.dtype, device=x.device)
        L.call("sp_maxpool3s2_fwd", ops.ptr(x), c, ctypes.c_void_p(out.data_ptr() + off * out.element_size()), out.shape[3],
               n, h, w, c, ops.sp_dtype(self.dtype), ops.stream())
        return out

    def _avgpool(self, x: torch.Tensor) -> torch.Tensor:
        n, h, w, c = x.shape
        out = torch.empty_like(x)
        L.call("sp_avgpool3s1_fwd", ops.ptr(x), ops.ptr(out), n, h, w, c, ops.sp_dtype(self.dtype), ops.stream())
        return out

    def _new(self, x: torch.Tensor, h: int, c: int) -> torch.Tensor:
        return torch.empty((x.shape[0], h, h, c), dtype=self.dtype, device=x.device)

    # ---- Inception blocks (torchvision's InceptionA..E; branch outputs in torch.cat order) ----------------------------------------
    def _block_a(self, blk: str, x: torch.Tensor, pf: int) -> torch.Tensor:
        y = self._new(x, x.shape[1], 224 + pf)
        self._conv(blk + ".branch1x1", x, y, 0)
        self._conv(blk + ".branch5x5_2", self._conv(blk + ".branch5x5_1", x), y, 64)
        t = self._conv(blk + ".branch3x3dbl_2", self._conv(blk + ".branch3x3dbl_1", x))
        self._conv(blk + ".branch3x3dbl_3", t, y, 128)
        self._conv(blk + ".branch_pool", self._avgpool(x), y, 224)
        return y

    def _block_b(self, x: torch.Tensor) -> torch.Tensor:
        y = self._new(x, (x.shape[1] - 3) // 2 + 1, 384 + 96 + x.shape[3])
        self._conv("Mixed_6a.branch3x3", x, y, 0)
        t = self._conv("Mixed_6a.branch3x3dbl_2", self._conv("Mixed_6a.branch3x3dbl_1", x))
        self._conv("Mixed_6a.branch3x3dbl_3", t, y, 384)
        self._maxpool(x, y, 480)
        return y

    def _block_c(self, blk: str, x: torch.Tensor) -> torch.Tensor:
        y = self._new(x, x.shape[1], 768)
        self._conv(blk + ".branch1x1", x, y, 0)
        t = self._conv(blk + ".branch7x7_2", self._conv(blk + ".branch7x7_1", x))
        self._conv(blk + ".branch7x7_3", t, y, 192)
        t = self._conv(blk + ".branch7x7dbl_1", x)
        for i in (2, 3, 4):
            t = self._conv(blk + ".branch7x7dbl_%d" % i, t)
        self._conv(blk + ".branch7x7dbl_5", t, y, 384)
        self._conv(blk + ".branch_pool", self._avgpool(x), y, 576)
        return y

    def _block_d(self, x: torch.Tensor) -> torch.Tensor:
        y = self._new(x, (x.shape[1] - 3) // 2 + 1, 320 + 192 + x.shape[3])
        self._conv("Mixed_7a.branch3x3_2", self._conv("Mixed_7a.branch3x3_1", x), y, 0)
        t = self._conv("Mixed_7a.branch7x7x3_1", x)
        for i in (2, 3):
            t = self._conv("Mixed_7a.branch7x7x3_%d" % i, t)
        self._conv("Mixed_7a.branch7x7x3_4", t, y, 320)
        self._maxpool(x, y, 512)
        return y

    def _block_e(self, blk: str, x: torch.Tensor) -> torch.Tensor:
        y = self._new(x, x.shape[1], 2048)
        self._conv(blk + ".branch1x1", x, y, 0)
        t = self._conv(blk + ".branch3x3_1", x)
        self._conv(blk + ".branch3x3_2a", t, y, 320)
        self._conv(blk + ".branch3x3_2b", t, y, 704)
        t = self._conv(blk + ".branch3x3dbl_2", self._conv(blk + ".branch3x3dbl_1", x))
        self._conv(blk + ".branch3x3dbl_3a", t, y, 1088)
        self._conv(blk + ".branch3x3dbl_3b", t, y, 1472)
        self._conv(blk + ".branch_pool", self._avgpool(x), y, 1856)
        return y

    # ---- public -----------------------------------------------------------------------------------------------------------------
    def prepare(self, images: torch.Tensor) -> torch.Tensor:
        """misc.normalize_m1_1_batch -> bilinear 299 x 299 -> NHWC (B, 299, 299, 8) in the compute dtype, channels 3..7 zero."""
        ops.require_gpu(images)
        if images.dim() != 4:
            raise SempyrError("InceptionV3Features: images must be (B, C, H, W), got %s" % (tuple(images.shape),))
        x = images.float().contiguous()
        n, c = x.shape[:2]
        if c > 8:
            raise SempyrError("InceptionV3Features: at most 8 input channels (got %d)" % c)
        mm = torch.empty(2 * n, dtype=torch.float32, device=x.device)
        y = torch.empty((n, INPUT_SIZE, INPUT_SIZE, 8), dtype=self.dtype, device=x.device)
        L.call("sp_inception_prep", ops.ptr(x), ops.ptr(mm), ops.ptr(y), n, c, x.shape[2], x.shape[3], INPUT_SIZE, INPUT_SIZE, 8,
               ops.sp_dtype(self.dtype), ops.stream())
        return y

    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        x = self.prepare(images)
        self._p = self._params(x.device)
        for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = self._conv(name, x)
        x = self._maxpool(x)
        x = self._conv("Conv2d_4a_3x3", self._conv("Conv2d_3b_1x1", x))
        x = self._maxpool(x)
        for blk, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
            x = self._block_a(blk, x, pf)
        x = self._block_b(x)
        for blk in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._block_c(blk, x)
        x = self._block_d(x)
        x = self._block_e("Mixed_7b", x)
        x = self._block_e("Mixed_7c", x)
        n, h, w, c = x.shape
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        L.call("sp_global_avgpool_f32", ops.ptr(x), ops.ptr(out), n, h * w, c, ops.sp_dtype(self.dtype), ops.stream())
        return out

    __call__ = forward
