"""ModelWrapper with the reference's constructor and ``train()`` signature (/root/reference/model_wrapper.py).

The loop body (model_wrapper.py:131-190) is ``train_step``: one discriminator step then one generator step.
What differs from the reference, without changing any observable result:
  * the discriminator's weight gradients of the GENERATOR step are not computed - the reference computes
    them and zeroes them unused at the top of the next iteration (model_wrapper.py:136-137,174,188);
  * gradients w.r.t. the real images, the masks and the latent vector (all dead) are not computed;
  * the five loss scalars are fetched with ONE device->host transfer per iteration instead of ten ``.item()``
    calls (model_wrapper.py:192-202);
  * multi-GPU is one process per GPU with an RCCL all-reduce of the gradients (``distributed.GradientReducer``)
    instead of single-process nn.DataParallel (main.py:91-94).
``validate`` computes the FID (fid.frechet_inception_distance) with an Inception-v3 on the library's kernels
(inception.InceptionV3Features) when it has weights - the constructor's ``inception`` keyword or SP_INCEPTION_WEIGHTS, a
torchvision inception_v3 state dict - and returns nan without them; ``inference`` writes the reference's 7 x 7 sample grid as a
PNG (misc.save_image_grid - torchvision is not a dependency).
Beyond the reference: with ``generator_ema`` (or SP_G_EMA) an exponential moving average of the generator's parameters is kept on the
device (optim.ParameterEMA), updated behind every generator optimizer step, swapped in for ``validate`` / ``inference`` and saved
beside the four reference keys of a checkpoint.  Off by default: nothing of it runs then.
Likewise ``augment`` (or SP_AUGMENT): differentiable augmentation - color, translation, cutout - of every image the discriminator
sees, applied inside its ingest pass (csrc/augment.hip): three independent transforms per step from one
(3, B, 8) draw of uniforms made in front of the latents.  Off by default: no draw, no launch, no allocation.
The words xflip, rot90, scale and rotate in the same string add the geometric family: the transforms compose with
the translation into one affine map per image, resampled bilinearly in the same pass; a step then also draws (3, B, 4) uniforms right
behind the first draw and decodes all 3B maps with one launch.  Without those words: no draw, no launch, no allocation, as before.
The words brightness, contrast, lumaflip, hue and saturation add ADA's color group: one 3 x 4 matrix per image,
applied to every source pixel as the last step of the color stage in the same pass; a step then draws one more (3, B, 8) tensor of
uniforms behind the others and decodes all 3B matrices with one launch.  Without those words: no draw, no launch, no allocation either.
And ``clip_grad_norm`` (or SP_CLIP_GRAD_NORM): each network's gradients are clipped by their global norm in front of its optimizer
step - one norm for D's step, one for G's - and a step whose norm is not finite is skipped, in every storage mode, on the device
(optim.Adam(max_grad_norm=...)); the two norms join the step's results and the log.  ``inf`` monitors and guards
and never scales.  A foreign optimizer (torch.optim.Adam) gets torch.nn.utils.clip_grad_norm_ in front of its step() instead: the
clipping and the norm, but NO guard beyond the fp16 mode's.  Off by default: no launch, no allocation, no new result.
And ``augment_p`` (or SP_AUGMENT_P; with ``augment`` only): each image in front of D is transformed with probability p and passes
untouched otherwise (the gate of csrc/augment.hip) - a fixed p, or one steered on the device from D's predictions
on the real images (ops.AdaptiveAugment: one counting launch inside the D phase, one adjusting launch behind Adam(G), no host sync);
p and the signal r_t then join the step's results, the log and the checkpoint.  Off by default: every image is transformed, as above.
And ``metrics`` (or SP_METRICS): besides the FID, ``evaluate()`` scores KID, precision, recall, density and coverage and / or the
Inception Score ("is": ``inception_score``, ``inception_score_std`` of the fake set over ``metrics_is_splits`` splits) from the
same activations, kept on the device (metrics.py, csrc/metrics.hip, DESIGN.md sections 17 and 19); ``validate()`` still returns the FID, keeps
the dict in ``last_metrics`` and ``train()`` logs its keys beside ``fid``.  Off by default: validate() is exactly what it was.
And ``apa`` (or SP_APA): adaptive pseudo augmentation (Jiang et al. 2021, "Deceive D") - with probability p an image
of the discriminator's REAL branch is replaced by a generated one that keeps the "real" label (ops.apa_select: one launch in front of
whatever module D is, from one more (B,) draw of uniforms behind the augmentation's and in front of the latents); a fixed p, or one
steered as augment_p is, by a second ops.AdaptiveAugment with its own state; the generator, the VGG-16 and the whole G step keep the true
real images.  It needs neither ``augment`` nor this package's Discriminator.  Off by default: no draw, no launch, no allocation, no key.
And ``reconstruction`` (or SP_RECONSTRUCTION) with ``reconstruction_levels`` (or SP_RECONSTRUCTION_LEVELS, "0-6"): per-level
reconstruction fidelity - ``evaluate_reconstruction()`` scores every validation image against its own inversion from each level's
features alone with PSNR, SSIM and / or MS-SSIM (reconstruction.py, csrc/reconstruction.hip), keeps the dict in
``last_reconstruction`` and ``train()`` logs its keys where it logs the FID.  It needs no Inception weights and adds nothing to
``evaluate()``'s dict.  Off by default: no launch, no allocation, no draw; train(), validate(), evaluate() and inference() are what they were.
"""
from __future__ import annotations

import os
from datetime import datetime
from typing import Dict, Optional, Union

import torch
import torch.nn as nn

from . import misc, ops, profiling
from .config import CFG
from .lossfunction import GAN_LOSSES, DiversityLoss, LSGANDiscriminatorLoss, LSGANGeneratorLoss, SemanticReconstructionLoss
from .models import VGG16, Discriminator, Generator, _class_index


def _unwrap(module):
    return module.module if hasattr(module, "module") and isinstance(module.module, nn.Module) else module


class ModelWrapper(object):
    def __init__(self,
                 generator: Union[Generator, nn.DataParallel],
                 discriminator: Union[Discriminator, nn.DataParallel],
                 training_dataset,
                 validation_dataset,
                 vgg16: Union[VGG16, nn.DataParallel] = None,
                 generator_optimizer: torch.optim.Optimizer = None,
                 discriminator_optimizer: torch.optim.Optimizer = None,
                 generator_loss: nn.Module = None,
                 discriminator_loss: nn.Module = None,
                 semantic_reconstruction_loss: nn.Module = None,
                 diversity_loss: nn.Module = None,
                 save_data_path: Optional[str] = 'saved_data',
                 gradient_reducer=None,
                 inception=None,
                 generator_ema=None,
                 augment=None,
                 clip_grad_norm=None,
                 augment_p=None,
                 metrics=None,
                 gan_loss=None,
                 lecam=None,
                 apa=None,
                 reconstruction=None,
                 reconstruction_levels=None) -> None:
        # nn.DataParallel wrappers are unwrapped: data parallelism is one process per GPU here
        self.generator = _unwrap(generator)
        self.discriminator = _unwrap(discriminator)
        self.training_dataset = training_dataset
        self.validation_dataset_fid = validation_dataset
        self.vgg16 = _unwrap(vgg16) if vgg16 is not None else VGG16()
        self.generator_optimizer = generator_optimizer
        self.discriminator_optimizer = discriminator_optimizer
        # gan_loss: "lsgan", "hinge" or "logistic" installs this package's pair of adversarial loss modules (lossfunction.GAN_LOSSES); None:
        # CFG.gan_loss (SP_GAN_LOSS - main.py's fixed keywords); "" = the modules the caller passed, LSGAN by default, as ever.
        from .config import parse_gan_loss, parse_lecam
        try:
            self.gan_loss = parse_gan_loss(CFG.gan_loss if gan_loss is None else gan_loss)
        except ValueError as exc:
            raise ops.L.SempyrError(str(exc)) from None
        if self.gan_loss:
            if generator_loss is not None or discriminator_loss is not None:
                raise ops.L.SempyrError("gan_loss=%r installs its own pair of loss modules, but generator_loss / discriminator_loss were "
                                        "passed as well: give one or the other" % (self.gan_loss,))
            generator_loss, discriminator_loss = (cls() for cls in GAN_LOSSES[self.gan_loss])
        self.generator_loss = generator_loss if generator_loss is not None else LSGANGeneratorLoss()
        self.discriminator_loss = discriminator_loss if discriminator_loss is not None else LSGANDiscriminatorLoss()
        self.semantic_reconstruction_loss = (semantic_reconstruction_loss if semantic_reconstruction_loss is not None
                                             else SemanticReconstructionLoss())
        self.diversity_loss = diversity_loss if diversity_loss is not None else DiversityLoss()
        self.latent_dimensions = self.generator.latent_dimensions
        self.gradient_reducer = gradient_reducer
        self._inception = inception                # InceptionV3Features, a weights path, or None (CFG.inception_weights)
        for parameter in self.vgg16.parameters():            # model_wrapper.py:67-68
            parameter.requires_grad = False
        self.logger = misc.Logger()
        self.path_save_models = self.path_save_plots = self.path_save_metrics = None
        if save_data_path is not None:
            stamp = str(datetime.now())
            self.path_save_models = os.path.join(save_data_path, 'models_' + stamp)
            self.path_save_plots = os.path.join(save_data_path, 'plots_' + stamp)
            self.path_save_metrics = os.path.join(save_data_path, 'metrics_' + stamp)
            for p in (self.path_save_models, self.path_save_plots, self.path_save_metrics):
                os.makedirs(p, exist_ok=True)
        for name in ('generator', 'discriminator', 'vgg16', 'generator_optimizer', 'discriminator_optimizer',
                     'generator_loss', 'discriminator_loss', 'diversity_loss', 'semantic_reconstruction_loss'):
            self.logger.hyperparameter[name] = str(getattr(self, name))
        # generator_ema: a decay or an optim.ParameterEMA; None: CFG.g_ema (SP_G_EMA - the reference's main.py builds the wrapper with
        # fixed keywords), 0 = off.  The average needs the generator on the GPU already (main.py:58 puts it there).
        self.generator_ema = None
        if generator_ema is None:
            generator_ema = CFG.g_ema
        if generator_ema:
            from . import optim
            if not isinstance(generator_ema, optim.ParameterEMA):
                if isinstance(generator_ema, bool):
                    raise ops.L.SempyrError("generator_ema takes a decay or an optim.ParameterEMA")
                generator_ema = optim.ParameterEMA(self.generator, decay=float(generator_ema))
            self.generator_ema = generator_ema
            self.logger.hyperparameter['generator_ema'] = str({"decay": self.generator_ema.decay, "warmup": self.generator_ema.warmup})
        # augment: "color,translation,cutout" or a subset; None: CFG.augment (SP_AUGMENT - main.py's fixed keywords again); "" = off.
        # Fixed for the wrapper's life.  _aug_policy is the bit mask of ops.augment_policy (0 = off: nothing below ever runs).
        if augment is None:
            augment = CFG.augment
        # _aug_geom: the geometric words of the same string (ops.augment_split; 0: the wrapper is exactly what it is without them).
        # _aug_cmat: ADA's color words of the same string (ops.augment_split3; 0: likewise).
        self._aug_policy, self._aug_geom, self._aug_cmat = ops.augment_split3(augment)
        if self._aug_policy or self._aug_geom or self._aug_cmat:
            if not isinstance(self.discriminator, Discriminator):
                raise ops.L.SempyrError("augment: the transform runs inside this package's Discriminator's ingest pass; a caller's own "
                                        "discriminator module cannot be armed")
            self.logger.hyperparameter['augment'] = ",".join([w for w, bit in ops._AUG_WORDS.items() if self._aug_policy & bit]
                                                              + [w for w, bit in ops._GEOM_WORDS.items() if self._aug_geom & bit]
                                                              + [w for w, bit in ops._CMAT_WORDS.items() if self._aug_cmat & bit])
        # augment_p: the probability with which an image in front of D is transformed (with augment only).  None: CFG.augment_p
        # (SP_AUGMENT_P); "" = off: every image, nothing below exists.  A number in [0, 1]: fixed.  "adaptive" / "adaptive:<target>" or an
        # ops.AdaptiveAugment: steered on the device.  _ada owns the device state; it is allocated HERE, outside any graph's pool.
        self._ada = self._make_augment_p(CFG.augment_p if augment_p is None else augment_p)
        if self.gan_loss:
            self.logger.hyperparameter['gan_loss'] = self.gan_loss
        # lecam: LeCam regularization of the discriminator (ops.LeCam) - a weight, "weight[:decay[:start]]" or an
        # ops.LeCam; None: CFG.lecam (SP_LECAM); "" / 0 = off: nothing below exists.  _lecam owns the device state (the two anchors); it is
        # allocated HERE, outside any graph's pool.  _lecam_reg: the regularizer of the last eager discriminator phase.
        self._lecam = self._make_lecam(CFG.lecam if lecam is None else lecam, parse_lecam)
        self._lecam_reg = None
        # apa: adaptive pseudo augmentation - None: CFG.apa (SP_APA); "" = off: nothing below exists.  A number in
        # [0, 1]: fixed p.  "adaptive" / "adaptive:<target>" or an ops.AdaptiveAugment: steered on the device, by a controller of its own
        # beside augment_p's.  _apa owns the device state; it is allocated HERE, outside any graph's pool.
        self._apa = self._make_apa(CFG.apa if apa is None else apa)
        # metrics: what validate() / evaluate() score besides the FID - a comma-separated subset of kid, prdc, is (metrics.py, DESIGN.md
        # sections 17, 19); None: CFG.metrics (SP_METRICS); "" = off: validate() is exactly what it is without.  An unknown word is an error
        # here.  metrics_nearest_k: the k of the precision / recall / density / coverage radii; metrics_is_splits: the splits of the
        # Inception Score; last_metrics: evaluate()'s last dict.
        from .config import parse_metrics
        self.metrics = parse_metrics(CFG.metrics if metrics is None else metrics)
        self.metrics_nearest_k = 5
        self.metrics_is_splits = 10
        self.last_metrics = None
        if self.metrics:
            self.logger.hyperparameter['metrics'] = ",".join(self.metrics)
        # reconstruction: what evaluate_reconstruction() scores - a comma-separated subset of psnr, ssim, ms_ssim (reconstruction.py,
        # DESIGN.md section 23); None: CFG.reconstruction (SP_RECONSTRUCTION); "" = off.  reconstruction_levels: the pyramid levels it
        # inverts from ("0-6", "0,3,6", a mix, or a sequence of integers); None: CFG.reconstruction_levels.  A bad word or level is an
        # error here.  last_reconstruction: evaluate_reconstruction()'s last dict.
        from .config import parse_levels, parse_reconstruction
        try:
            self.reconstruction = parse_reconstruction(CFG.reconstruction if reconstruction is None else reconstruction)
            self.reconstruction_levels = parse_levels(CFG.reconstruction_levels if reconstruction_levels is None else reconstruction_levels)
        except ValueError as exc:
            raise ops.L.SempyrError(str(exc)) from None
        self.last_reconstruction = None
        if self.reconstruction:
            self.logger.hyperparameter['reconstruction'] = ",".join(self.reconstruction)
            self.logger.hyperparameter['reconstruction_levels'] = ",".join(str(s) for s in self.reconstruction_levels)
        self._d_params = [p for p in self.discriminator.parameters()]
        self._g_params = [p for p in self.generator.parameters()]
        # clip_grad_norm: a threshold > 0 or inf; None: CFG.clip_grad_norm (SP_CLIP_GRAD_NORM - main.py's fixed keywords once more); 0 = off.
        # It applies to each network on its own.  This package's Adam carries it itself (max_grad_norm: norm, coefficient, guard and step
        # on the device); a foreign optimizer gets torch's clip_grad_norm_ in front of its step (_optimizer_step) - no guard there.
        if clip_grad_norm is None:
            clip_grad_norm = CFG.clip_grad_norm
        self.clip_grad_norm = None
        if not isinstance(clip_grad_norm, bool) and isinstance(clip_grad_norm, (int, float)) and clip_grad_norm == 0:
            clip_grad_norm = None
        if clip_grad_norm is not None:
            from . import optim
            self.clip_grad_norm = optim.check_max_grad_norm(clip_grad_norm, "clip_grad_norm")
            for name in ('generator_optimizer', 'discriminator_optimizer'):
                optimizer = getattr(self, name)
                if isinstance(optimizer, optim.Adam):
                    if optimizer.max_grad_norm is not None and optimizer.max_grad_norm != self.clip_grad_norm:
                        raise ops.L.SempyrError("clip_grad_norm=%r, but the %s already has max_grad_norm=%r"
                                                % (self.clip_grad_norm, name, optimizer.max_grad_norm))
                    optimizer.max_grad_norm = self.clip_grad_norm
            self.logger.hyperparameter['clip_grad_norm'] = str(self.clip_grad_norm)
            self._grad_norm = {}           # "d" / "g": the norm the last optimizer step of that network measured (a device tensor)
        # every gradient of a network lives in ONE flat fp32 buffer (ops.SpectralNormBank.flat; param.grad are views of it):
        # D runs twice per backward (real, fake) and its gradients meet there instead of in 59 autograd sums, and the
        # data-parallel reducer all-reduces ranges of the buffer in place.  SP_DIRECT_GRADS=0: plain autograd gradients.
        self._banks = {}
        if CFG.direct_grads:
            for key, net, passes in (("d", self.discriminator, 2), ("g", self.generator, 1)):
                bank = getattr(net, "_bank", None)
                if bank is not None:
                    bank.direct_grads = True
                    bank.expected_passes = passes
                    bank.set_groups(4 if gradient_reducer is not None else 1)
                    self._banks[key] = bank
        self._graph_state = None
        self.graph_after_iterations = CFG.graph_after       # train(): eager iterations before the step is captured (0 = never)
        self._eager_run, self._eager_sig, self._graph_failed = 0, None, False
        # (real images tensor, its ._version, its VGG pyramid) where the previous iteration computed it ahead (train_step: next_images_real)
        self._vgg_ahead = None
        # (fake images of the generator step with their autograd graph, their latents) where the discriminator phase has already taken
        # that forward together with its own (_d_phase: Generator.forward_pair)
        self._fake_ahead = None
        # the step's (3, B, 8) affine tables of the geometric augmentation where the discriminator phase has decoded them (_d_phase)
        self._aug_tables = None
        # likewise the step's (3, B, 12) color matrices
        self._aug_ctables = None
        self._capturing = False
        self._fired = set()
        self.iterations = 0

    # ------------------------------------------------------------------------------------------
    # data parallelism: flat, in-place, overlapped gradient reduction (distributed.GradientReducer)
    # ------------------------------------------------------------------------------------------
    def _arm_reducer(self, key: str) -> None:
        """Before a backward pass launched eagerly: the bank's layer groups hand their flat range to the reducer the moment
        their batched spectral-norm backward has been enqueued - while the rest of the backward pass still runs."""
        bank = self._banks.get(key)
        if bank is None:
            return
        bank.on_group_done = None
        self._fired = set()
        # (fp16 mode: the loss scale comes off the whole flat buffer after the backward pass - ranges go to the wire only then)
        if self.gradient_reducer is not None and not self._capturing and self.gradient_reducer.active() and ops.loss_scale() == 1.0:
            red = self.gradient_reducer

            def done(start, stop, bank=bank):
                self._fired.add((start, stop))
                bucket = max(1, red.bucket_bytes // 4)
                for a in range(start, stop, bucket):
                    red.reduce_range(bank.flat, a, min(stop, a + bucket))
            bank.on_group_done = done

    def _finish_backward(self, key: str) -> None:
        """After .backward(): non-SN gradients move into the flat buffer (inside the captured graph too)."""
        bank = self._banks.get(key)
        if bank is not None:
            bank.on_group_done = None
            bank.collect_extra()
            if bank.flat is not None:
                # fp16 mode: the loss scale has come off the spectral-normalised layers' gradients inside their batched
                # backward; the tail of the buffer (gradients that arrived through autograd) loses it here (16-byte aligned offset)
                ops.unscale_(bank.flat, bank.sn_floats)
        elif ops.loss_scale() != 1.0:
            raise ops.L.SempyrError("the fp16 storage mode needs the flat gradient buffers (config.CFG.direct_grads) for its loss scale")

    def _start_reduce(self, key: str, params, eager: bool) -> None:
        """Enqueues (side stream) whatever of the network's gradients has not been handed over by the group hooks."""
        red = self.gradient_reducer
        if red is None or not red.active():
            return
        bank = self._banks.get(key)
        if bank is None or bank.flat is None:
            red.reduce(params)                        # loose gradients: flatten / all-reduce / scatter back
            return
        fired = self._fired if eager else set()
        todo = []
        # replayed graphs: the whole buffer is final here - no collective below 8 MB (SpectralNormBank.flat_ranges); eager launches: the
        # groups have handed their own ranges over from inside the backward pass, what is left is matched against them group by group
        for a, b in bank.flat_ranges(max(1, red.bucket_bytes // 4), **({"min_floats": 0} if eager else {})):
            if not any(fa <= a and b <= fb for fa, fb in fired):
                todo.append((a, b))
        red.reduce_flat(bank.flat, todo)
        # safety net: a gradient that does not live in the flat buffer (a parameter the bank does not know) is reduced on its own
        lo = bank.flat.data_ptr()
        hi = lo + 4 * bank.flat.numel()
        loose = [p for p in params if p.grad is not None and not (lo <= p.grad.data_ptr() < hi)]
        if loose:
            red.reduce(loose)

    def _join_reduce(self, tag: str = "") -> None:
        if self.gradient_reducer is not None:
            self.gradient_reducer.join(tag)

    def _optimizer_step(self, key: str, optimizer) -> None:
        """optimizer.step() - in the fp16 storage mode behind the overflow guard of the dynamic loss scale (ops.LossScaler): the
        network's flat gradient buffer (already averaged over the ranks, so every rank decides alike) is screened for inf / NaN, the
        step is skipped where one is found, and the scale is backed off / grown - all on the device for this package's Adam
        (sp_adam_multi_guarded); a foreign optimizer costs one host sync per step for the same decision.  The generator's step
        (key "g") ends with the update of its weight average where there is one (self.generator_ema): one more eager launch, skipped
        with the step - on the device through the same flag (read before sc.update() clears it), or on the host.
        With clip_grad_norm this package's Adam measures the norm, clips and guards inside its step (every storage mode, no host sync),
        and without a loss scaler the weight average follows its skip flag (with one, the scaler's flag stays: a sum of squares is
        non-finite exactly when an element is, so the two agree).  A foreign optimizer gets torch.nn.utils.clip_grad_norm_ (foreach,
        itself sync-free) in front of its step(): clipping and a norm, but no guard beyond the fp16 mode's.  Either way the norm of the
        step is left in self._grad_norm[key] as a device tensor."""
        from . import optim
        ema = self.generator_ema if key == "g" else None
        bank = self._banks.get(key)
        sc = ops.loss_scaler(bank.flat.device) if bank is not None and bank.flat is not None else None
        own = isinstance(optimizer, optim.Adam)
        clip = self.clip_grad_norm
        if clip is not None and own and optimizer.max_grad_norm != clip:
            raise ops.L.SempyrError("clip_grad_norm=%r, but the optimizer's max_grad_norm is %r" % (clip, optimizer.max_grad_norm))

        if clip is not None and not own:
            self._grad_norm[key] = torch.nn.utils.clip_grad_norm_(self._d_params if key == "d" else self._g_params, clip, foreach=True)
        if sc is None:
            optimizer.step()
            if ema is not None:
                ema.update(found_inf=ops.ptr(optimizer.skip_flag) if clip is not None and own else None)
        else:
            sc.check(bank.flat)
            if own:
                optimizer.step(found_inf=sc.found_ptr)
                if ema is not None:
                    ema.update(found_inf=sc.found_ptr)
            elif not sc.values()["found"]:
                optimizer.step()
                if ema is not None:
                    ema.update()
            sc.update()
        if clip is not None and own:
            self._grad_norm[key] = optimizer.grad_norm

    def _make_augment_p(self, spec):
        """The constructor's augment_p -> an ops.AdaptiveAugment (fixed or adaptive) or None (off)."""
        if isinstance(spec, str):
            spec = spec.strip()
            if spec == "":
                return None
        if isinstance(spec, bool) or spec is None:
            raise ops.L.SempyrError("augment_p takes a probability in [0, 1], 'adaptive', 'adaptive:<target>' or an ops.AdaptiveAugment (got %r)" % (spec,))
        if not (self._aug_policy or self._aug_geom or self._aug_cmat):
            raise ops.L.SempyrError("augment_p=%r, but this ModelWrapper augments nothing (augment / SP_AUGMENT): there is nothing to gate" % (spec,))
        device = next(self.discriminator.parameters()).device
        if isinstance(spec, ops.AdaptiveAugment):
            ada = spec
        else:
            if device.type != "cuda":
                raise ops.L.SempyrError("augment_p: the gate's state lives on the discriminator's GPU; move the discriminator there first")
            try:
                if isinstance(spec, str) and (spec == "adaptive" or spec.startswith("adaptive:")):
                    # counted around the D loss module's own decision threshold: 0.5 for LSGAN (and for a foreign module), 0 for hinge / logistic
                    kw = {"threshold": float(getattr(self.discriminator_loss, "decision_threshold", 0.5))}
                    ada = ops.AdaptiveAugment(device, target=float(spec[9:]), **kw) if spec != "adaptive" else ops.AdaptiveAugment(device, **kw)
                else:
                    ada = ops.AdaptiveAugment(device, p=float(spec), adaptive=False)
            except ValueError:
                raise ops.L.SempyrError("augment_p takes a probability in [0, 1], 'adaptive' or 'adaptive:<target>' (got %r)" % (spec,)) from None
        self.logger.hyperparameter['augment_p'] = str(dict(ada.settings(), p=float(ada.p)) if not ada.adaptive else ada.settings())
        return ada

    def _make_apa(self, spec):
        """The constructor's apa -> an ops.AdaptiveAugment (fixed or adaptive) or None (off).  The controller is ops.AdaptiveAugment as it
        stands, in an instance of its own; its threshold is the D loss module's decision_threshold, as augment_p takes it."""
        from .config import parse_apa
        if isinstance(spec, ops.AdaptiveAugment):
            apa = spec
        else:
            try:
                fields = parse_apa(spec)
            except ValueError:
                raise ops.L.SempyrError("apa takes a probability in [0, 1], 'adaptive', 'adaptive:<target>' or an ops.AdaptiveAugment "
                                        "(got %r)" % (spec,)) from None
            if fields is None:
                return None
            device = next(self.discriminator.parameters()).device
            if device.type != "cuda":
                raise ops.L.SempyrError("apa: the probability's state lives on the discriminator's GPU; move the discriminator there first")
            if fields[0] == "adaptive":
                apa = ops.AdaptiveAugment(device, target=fields[1], threshold=float(getattr(self.discriminator_loss, "decision_threshold", 0.5)))
            else:
                apa = ops.AdaptiveAugment(device, p=fields[1], adaptive=False)
        self.logger.hyperparameter['apa'] = str(dict(apa.settings(), p=float(apa.p)) if not apa.adaptive else apa.settings())
        return apa

    def _make_lecam(self, spec, parse):
        """The constructor's lecam -> an ops.LeCam or None (off)."""
        if isinstance(spec, ops.LeCam):
            lecam = spec
        else:
            try:
                fields = parse(spec)
            except ValueError as exc:
                raise ops.L.SempyrError(str(exc)) from None
            if fields is None:
                return None
            device = next(self.discriminator.parameters()).device
            if device.type != "cuda":
                raise ops.L.SempyrError("lecam: the anchors live on the discriminator's GPU; move the discriminator there first")
            lecam = ops.LeCam(device, fields[0], decay=fields[1], start=fields[2])
        self.logger.hyperparameter['lecam'] = str(lecam.settings())
        return lecam

    def _with_lecam(self, out: Dict[str, torch.Tensor], reg) -> Dict[str, torch.Tensor]:
        """The step's results plus, with LeCam on ONLY, the regularizer of its discriminator phase and the two anchors (views of the device
        state, as augment_p is one of the controller's)."""
        if self._lecam is None:
            return out
        out = dict(out)
        out["loss_discriminator_lecam"] = reg.detach().reshape(())
        out["lecam_anchor_real"], out["lecam_anchor_fake"] = self._lecam.anchor_real.reshape(()), self._lecam.anchor_fake.reshape(())
        return out

    def _adaptive(self) -> bool:
        return self._ada is not None and self._ada.adaptive

    def _with_augment_p(self, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The step's results plus, with the adaptive controller on ONLY, p and the signal r_t of the last full window: views of the
        controller's device state (as the gradient norms are views of the clip state), read after the step's adjust launch."""
        if not self._adaptive():
            return out
        out = dict(out)
        out["augment_p"], out["augment_rt"] = self._ada.p.reshape(()), self._ada.r.reshape(())
        return out

    def _apa_adaptive(self) -> bool:
        return self._apa is not None and self._apa.adaptive

    def _with_apa(self, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The step's results plus, with APA's adaptive controller on ONLY, its p and r_t: views of its device state, as augment_p's are."""
        if not self._apa_adaptive():
            return out
        out = dict(out)
        out["apa_p"], out["apa_rt"] = self._apa.p.reshape(()), self._apa.r.reshape(())
        return out

    def _with_grad_norms(self, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The step's results plus, with clip_grad_norm on ONLY, the two gradient norms its optimizer steps measured (device tensors; this
        package's Adam hands out views of its clip state, which its next step overwrites - as the graphs' static outputs are)."""
        if self.clip_grad_norm is None:
            return out
        out = dict(out)
        for key, name in (("d", "grad_norm_discriminator"), ("g", "grad_norm_generator")):
            if key in self._grad_norm:
                out[name] = self._grad_norm[key].detach().reshape(())
        return out

    # ------------------------------------------------------------------------------------------
    def _g_pair_ok(self) -> bool:
        """Both generator forwards of the iteration in one pass (config.CFG.g_pair): this package's generator in training mode.  (Under
        data parallelism the discriminator's gradient all-reduce then hides behind _g_features instead of the generator forward.)"""
        return CFG.g_pair and isinstance(self.generator, Generator) and self.generator.training

    def _uniform_rows(self, images_real, given, width, on, name, off_text):
        """The step's (3, B, width) uniforms - row 0: the real images of the D step, 1: its fake images, 2: the fake images of the G step in
        front of D - drawn here unless the caller brings them (`given`), or None where `on` is false (then bringing them raises)."""
        if not on:
            if given is not None:
                raise ops.L.SempyrError("%s given, but this ModelWrapper %s" % (name, off_text))
            return None
        shape = (3, images_real.shape[0], width)
        if given is None:
            return torch.rand(shape, dtype=torch.float32, device=images_real.device)
        if tuple(given.shape) != shape:
            raise ops.L.SempyrError("%s must be %s (three transforms x batch x %d uniforms), got %s" % (name, shape, width, tuple(given.shape)))
        return given.detach().to(device=images_real.device, dtype=torch.float32).contiguous()

    def _augment_rows(self, images_real, augment_u):
        """The step's (3, B, 8) uniforms (_uniform_rows) - or None with augmentation off.  Drawn FIRST in a step (before the latents)."""
        return self._uniform_rows(images_real, augment_u, 8, self._aug_policy or self._aug_geom or self._aug_cmat, "augment_u",
                                  "augments nothing (augment / SP_AUGMENT)")

    def _augment_geom_rows(self, images_real, augment_v):
        """The step's (3, B, 4) uniforms of the geometric words (_uniform_rows) - or None without geometric words.  Drawn right behind the
        (3, B, 8) draw and in front of the latents."""
        return self._uniform_rows(images_real, augment_v, 4, self._aug_geom, "augment_v",
                                  "has no geometric augmentation (xflip / rot90 / scale / rotate in augment / SP_AUGMENT)")

    def _augment_cmat_rows(self, images_real, augment_z):
        """The step's (3, B, 8) uniforms of the color-matrix words (_uniform_rows) - or None without them.  Drawn right behind the draw of
        the geometric words (or the first draw where there are none) and in front of the latents."""
        return self._uniform_rows(images_real, augment_z, 8, self._aug_cmat, "augment_z",
                                  "has no color-matrix augmentation (brightness / contrast / lumaflip / hue / saturation in augment / SP_AUGMENT)")

    def _apa_rows(self, images_real, apa_w):
        """The step's (B,) uniforms of the pseudo augmentation, one per image of D's real branch - drawn here unless the caller brings
        them, or None with APA off (then bringing them raises).  Drawn right behind the augmentation's draws (first where there are none)
        and in front of the latents."""
        if self._apa is None:
            if apa_w is not None:
                raise ops.L.SempyrError("apa_w given, but this ModelWrapper has no pseudo augmentation (apa / SP_APA)")
            return None
        shape = (images_real.shape[0],)
        if apa_w is None:
            return torch.rand(shape, dtype=torch.float32, device=images_real.device)
        if tuple(apa_w.shape) != shape:
            raise ops.L.SempyrError("apa_w must be %s (one uniform per image), got %s" % (shape, tuple(apa_w.shape)))
        return apa_w.detach().to(device=images_real.device, dtype=torch.float32).contiguous()

    def _apa_images(self, images_real, images_fake, apa_w, out=None):
        """What D's real branch sees with APA on: image i is the pseudo source's iff apa_w[i] < p, else the real one (ops.apa_select, one
        launch, into `out` - the graphs' static buffer - if given).  THE PSEUDO SOURCE, one rule: the fake images of the generator step
        where the discriminator phase's pair forward has made them (self._fake_ahead: fresh latents, the same labels, features and masks -
        what the official implementation draws at extra cost), detached; else the D step's own fake images.  Row i pairs with label i
        either way."""
        pseudo = self._fake_ahead[0] if self._fake_ahead is not None else images_fake
        if tuple(pseudo.shape) != tuple(images_real.shape):
            raise ops.L.SempyrError("apa: the generated images %s do not have the real images' shape %s" % (tuple(pseudo.shape), tuple(images_real.shape)))
        return ops.apa_select(images_real, pseudo.detach(), apa_w, self._apa.p, out=out)

    def _augment_ctables(self, images_real, aug_z, out=None):
        """The step's (3, B, 12) color matrices: all 3B rows in ONE decode launch (into `out`, the graphs' static buffer, if given) - or
        None without color-matrix words."""
        if aug_z is None:
            return None
        return ops.augment_cmat_decode(aug_z, self._aug_cmat, out=out).view(3, images_real.shape[0], 12)

    def _augment_tables(self, images_real, aug_u, aug_v, out=None):
        """The step's (3, B, 8) affine tables: all 3B rows in ONE decode launch (into `out`, the graphs' static buffer, if given) - or
        None without geometric words."""
        if aug_v is None:
            return None
        b, _, h, w = images_real.shape
        return ops.augment_geom_decode(aug_u, aug_v, h, w, self._aug_policy, self._aug_geom, out=out).view(3, b, 8)

    def _d_call(self, fn, rows, *args, tables=None, ctables=None):
        """fn(*args) - the discriminator's forward or forward_pair - armed with these rows of uniforms (and, with geometric words, their
        affine tables; with color-matrix words, their color matrices) for that one call (None: as it is)."""
        if rows is None:
            return fn(*args)
        D = self.discriminator
        if ctables is not None:
            rows = tuple(zip(rows, tables if tables is not None else (None,) * len(rows), ctables))
        elif tables is not None:
            rows = tuple(zip(rows, tables))
        D._augment = (self._aug_policy,) + tuple(rows)
        D._augment_p = self._ada.p if self._ada is not None else None
        try:
            return fn(*args)
        finally:
            D._augment = None
            D._augment_p = None

    def _d_phase(self, images_real, labels, labels_f, masks, noise_d, features_real=None, noise_g=None, aug_u=None, aug_v=None,
                 aug_t_out=None, aug_z=None, aug_c_out=None, apa_w=None, apa_out=None):
        """model_wrapper.py:136-160: forward passes and backward of the discriminator step (everything but Adam).  features_real: the
        pyramid of images_real where an earlier generator step has already computed it (_g_rest, next_images_real).  noise_g: the
        latents of the generator step, for the case that its forward is taken in the same pass as this step's (_g_pair_ok).  aug_u: the
        step's uniforms (_augment_rows) - D sees T(real; aug_u[0]) and T(fake; aug_u[1]); the generator and the VGG-16 see the images.
        aug_v: the uniforms of the geometric words (_augment_geom_rows); their tables are decoded HERE - one launch, inside the first
        captured graph - into aug_t_out (or a fresh tensor) and left in self._aug_tables for the generator step.  aug_z: the uniforms of the
        color-matrix words (_augment_cmat_rows), decoded likewise into aug_c_out and left in self._aug_ctables.  apa_w: the uniforms of the
        pseudo augmentation (_apa_rows) - D's real branch then sees _apa_images(...) (into apa_out or a fresh tensor) in place of
        images_real; the VGG-16, the generator's conditioning and everything behind this phase keep images_real."""
        G, D, V = self.generator, self.discriminator, self.vgg16
        aug_t = self._aug_tables = self._augment_tables(images_real, aug_u, aug_v, aug_t_out)
        aug_c = self._aug_ctables = self._augment_ctables(images_real, aug_z, aug_c_out)
        G.zero_grad()
        D.zero_grad()
        self._fake_ahead = None
        with torch.no_grad():
            if features_real is None:
                features_real = V(images_real)
            if noise_d is None:
                noise_d = torch.randn((images_real.shape[0], self.latent_dimensions), dtype=torch.float32, device=images_real.device)
        if self._g_pair_ok():
            if noise_g is None:                       # (the reference draws it later, model_wrapper.py:168 - nothing else draws in between)
                noise_g = torch.randn((images_real.shape[0], self.latent_dimensions), dtype=torch.float32, device=images_real.device)
            images_fake_g, images_fake = G.forward_pair(noise_g, noise_d, features_real, masks, labels_f)
            self._fake_ahead = (images_fake_g, noise_g)
        else:
          with torch.no_grad():
            if hasattr(G, "map_mode"):
                G.map_mode = "stash"                  # this forward and the G step's see the same pyramid, masks and weights
            images_fake = G(input=noise_d, features=features_real, masks=masks, class_id=labels_f)
        # one launch behind the generator's forward(s) and in front of D (inside the first captured graph)
        images_for_d = images_real if apa_w is None else self._apa_images(images_real, images_fake, apa_w, apa_out)
        if CFG.d_pair and hasattr(D, "forward_pair") and D.training and images_fake.shape == images_real.shape:
            rows = None if aug_u is None else (aug_u[0], aug_u[1])
            prediction_real, prediction_fake = self._d_call(D.forward_pair, rows, images_for_d, images_fake, labels,
                                                            tables=None if aug_t is None else (aug_t[0], aug_t[1]),
                                                            ctables=None if aug_c is None else (aug_c[0], aug_c[1]))     # one trunk pass over 2B images
        else:
            prediction_real = self._d_call(D, None if aug_u is None else (aug_u[0],), images_for_d, labels,
                                           tables=None if aug_t is None else (aug_t[0],), ctables=None if aug_c is None else (aug_c[0],))
            prediction_fake = self._d_call(D, None if aug_u is None else (aug_u[1],), images_fake, labels,
                                           tables=None if aug_t is None else (aug_t[1],), ctables=None if aug_c is None else (aug_c[1],))
        if self._adaptive():
            # the overfitting signal's counts (sp_ada_observe): one launch on D's fp32 predictions, inside the first captured graph; p
            # itself moves only behind Adam(G) (train_step), so every gate of this step reads the same value
            self._ada.observe(prediction_real)
        if self._apa_adaptive():
            # APA's own counts, right behind: over the whole real branch, replaced rows included (the official implementation's choice)
            self._apa.observe(prediction_real)
        terms = []
        if self._lecam is not None:
            # one launch right behind it, inside the first captured graph too: means, anchors and the regularizer, whatever loss module
            # follows; its gradient joins D's through one more seed (the fp16 mode's scale included)
            reg = self._lecam(prediction_real.float(), prediction_fake.float())
            # kept DETACHED: a tensor with its grad_fn would hold this iteration's autograd graph - and the eager-stream gradient
            # accumulators of the parameters with it - alive into a later capture_graphs(), which must start without any
            self._lecam_reg = reg.detach()
            terms = [reg]
        loss_d_real, loss_d_fake = self.discriminator_loss(prediction_real, prediction_fake)
        self._arm_reducer("d")
        # d(real + fake): one seed per loss instead of a sum kernel and autograd's own seed (model_wrapper.py:158-160)
        terms = [loss_d_real, loss_d_fake] + terms
        torch.autograd.backward(terms, ops.backward_seeds(terms))
        self._finish_backward("d")
        return features_real, loss_d_real, loss_d_fake

    def _g_forward(self, images_real, labels_f, masks, features_real, noise_g):
        """model_wrapper.py:165-172: the generator forward of the G step.  It does not read the discriminator, so D's gradient
        all-reduce and D's Adam step may still be in flight / pending while it runs (train_step)."""
        G = self.generator
        G.zero_grad()
        ahead, self._fake_ahead = self._fake_ahead, None
        if ahead is not None:                         # taken in the discriminator phase's pass (Generator.forward_pair)
            return ahead
        if noise_g is None:
            noise_g = torch.randn((images_real.shape[0], self.latent_dimensions), dtype=torch.float32, device=images_real.device)
        if hasattr(G, "map_mode"):
            G.map_mode = "reuse"                      # the masked-feature mappings come from the D step's forward (other sigma only)
        return G(input=noise_g, features=features_real, masks=masks, class_id=labels_f), noise_g

    def _vgg_pair_ok(self, images_fake, next_images_real) -> bool:
        """One VGG pass over [fake | next real] pays where a batch alone leaves CUs idle in the pyramid's deep stages (batch 20 at
        256 x 256: 80 work items on 256 CUs in the 16 x 16 stage, 320 in the 32 x 32 stage): same box, bf16 15.73 -> 15.58 ms, fp32
        103.5 -> 102.2 ms per step; at batch 32 the stages are full already and the pass costs 0.7 % (the second half cannot pool in
        the convolution epilogue) - so: up to 24 images of 256 x 256 (n x (H / 64) x (W / 64) <= 384)."""
        if not (CFG.vgg_pair and next_images_real is not None and hasattr(self.vgg16, "forward_pair") and ops.vgg_fp8() == 0
                and next_images_real.is_cuda and tuple(next_images_real.shape) == tuple(images_fake.shape)):
            return False
        n, _, h, w = images_fake.shape
        return n * (h // 64) * (w // 64) <= 384

    def _g_features(self, images_fake, noise_g, w_div, next_images_real=None):
        """The part of the generator step that does NOT read the discriminator (model_wrapper.py:179-186): the diversity loss and the
        frozen VGG-16's pass over the fake images.  train_step runs it BEFORE the discriminator's optimizer step: under data parallelism
        this pass (1.7 ms at batch 20) - together with the generator forward, where that has not already ridden in the discriminator
        phase (_g_pair_ok) - is what the discriminator's gradient all-reduce hides behind.  next_images_real: the real images of the NEXT
        iteration, whose pyramid (model_wrapper.py:141 of that iteration; the network is frozen) is taken in the same pass
        (VGG16.forward_pair).  Returns (diversity loss, features of the fake images, features of the next real images or None)."""
        # the weights ride inside this package's loss kernels; a caller's own loss module is weighted the reference's way
        if isinstance(self.diversity_loss, DiversityLoss):
            loss_div = self.diversity_loss(images_fake, noise_g, weight=w_div)
        else:
            loss_div = w_div * self.diversity_loss(images_fake, noise_g)
        features_next = None
        if self._vgg_pair_ok(images_fake, next_images_real):
            features_fake, features_next = self.vgg16.forward_pair(images_fake, next_images_real)
        else:
            features_fake = self.vgg16(images_fake)
        return loss_div, features_fake, features_next

    def _g_rest(self, images_fake, noise_g, labels, masks, features_real, w_rec, w_div, next_images_real=None, features_next_out=None,
                ahead=None, aug_u=None, aug_t=None, aug_c=None):
        """model_wrapper.py:174-188: D(fake), the generator and reconstruction losses, backward (everything but Adam).  aug_u: the step's
        uniforms - D sees T(fake; aug_u[2]), whose backward carries D's image gradient through T; every other loss sees the images.  ahead: what
        _g_features has already computed for these fake images (train_step: in front of the discriminator's optimizer step); without
        it that part runs here.  features_next_out: static tensors to copy the next batch's pyramid into after the backward pass
        (captured graphs); it is kept in self._vgg_ahead."""
        D = self.discriminator
        D.zero_grad()
        if ahead is None:
            ahead = self._g_features(images_fake, noise_g, w_div, next_images_real)
        loss_div, features_fake, features_next = ahead
        for p in self._d_params:                               # dead D weight gradients are skipped
            p.requires_grad_(False)
        try:
            prediction_fake = self._d_call(D, None if aug_u is None else (aug_u[2],), images_fake, labels,
                                           tables=None if aug_t is None else (aug_t[2],), ctables=None if aug_c is None else (aug_c[2],))
            loss_g = self.generator_loss(prediction_fake)
            if isinstance(self.semantic_reconstruction_loss, SemanticReconstructionLoss):
                loss_rec = self.semantic_reconstruction_loss(features_real, features_fake, masks, weight=w_rec)
            else:
                loss_rec = w_rec * self.semantic_reconstruction_loss(features_real, features_fake, masks)
            self._arm_reducer("g")
            # backward of (loss_g + loss_rec + loss_div) (model_wrapper.py:187-188): one seed per term
            terms = [loss_g, loss_rec, loss_div]
            torch.autograd.backward(terms, ops.backward_seeds(terms))
            self._finish_backward("g")
            self._vgg_ahead = None
            if features_next is not None:
                if features_next_out is not None:                # (after the backward pass: it still read this iteration's features)
                    with torch.no_grad():                        # one multi-tensor launch instead of seven copies
                        torch._foreach_copy_(list(features_next_out), list(features_next))
                    features_next = features_next_out
                self._vgg_ahead = (next_images_real, next_images_real._version, features_next, self._mode_key())
        finally:
            for p in self._d_params:
                p.requires_grad_(True)
        return loss_g, loss_rec, loss_div

    def _features_ahead(self, images_real):
        """The pyramid of images_real if the previous iteration computed it ahead (same tensor object, not written since)."""
        ahead, self._vgg_ahead = self._vgg_ahead, None
        if ahead is not None and ahead[0] is images_real and ahead[1] == images_real._version and ahead[3] == self._mode_key():
            return ahead[2]
        return None

    @staticmethod
    def _mode_key():
        """What a pyramid computed ahead depends on beside the images: the storage type and the fp8 slice (round-4 ADVICE)."""
        return (ops.compute_dtype(), ops.vgg_fp8())

    def train_step(self, images_real: torch.Tensor, labels: torch.Tensor, masks, w_rec: float = 0.1, w_div: float = 0.1,
                   noise_d: Optional[torch.Tensor] = None, noise_g: Optional[torch.Tensor] = None,
                   next_images_real: Optional[torch.Tensor] = None, augment_u: Optional[torch.Tensor] = None,
                   augment_v: Optional[torch.Tensor] = None, augment_z: Optional[torch.Tensor] = None,
                   apa_w: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One iteration of model_wrapper.py:131-190 on tensors already on the device.  ``noise_d`` / ``noise_g``
        replace the two ``torch.randn`` draws (model_wrapper.py:147,168) for parity runs, ``augment_u`` ((3, B, 8), with augmentation
        on only) the ``torch.rand`` draw in front of them, ``augment_v`` ((3, B, 4), with geometric words only) the one right behind
        it, ``augment_z`` ((3, B, 8), with color-matrix words only) the one behind that, ``apa_w`` ((B,), with APA on only) the one behind
        those and in front of the latents.  Returns the loss scalars as device tensors (no host sync).

        ``next_images_real`` (optional): the real images of the NEXT call (the same tensor object must then be passed as its
        ``images_real``).  The frozen VGG-16 sees them in the pass it makes over this iteration's fake images - one pass over 2B
        images instead of two over B (config.CFG.vgg_pair) - and the next call finds its pyramid computed.  Results do not change:
        the network is frozen and in eval mode.

        Order of work (results identical to the reference's order): D phase (with both generator forwards where _g_pair_ok); [D gradients
        -> side stream]; what the G phase can do without the discriminator - the generator forward if it is still due, the diversity
        loss, the VGG-16 pass over the fake images; join; Adam(D); rest of the G phase; [G gradients -> side stream]; join; Adam(G)."""
        # the one-hot labels become class indices ONCE per step (the reference's modules take the argmax in every forward,
        # models.py:151,501: five reductions and a float copy per step; our modules pass indices through)
        # - only for this package's modules: a caller's own module may take the argmax of what it is given (round-4 ADVICE)
        raw_labels = labels
        idx = _class_index(labels)
        labels = idx if isinstance(self.discriminator, Discriminator) else raw_labels
        labels_f = idx if isinstance(self.generator, Generator) else raw_labels
        aug_u = self._augment_rows(images_real, augment_u)
        aug_v = self._augment_geom_rows(images_real, augment_v)
        aug_z = self._augment_cmat_rows(images_real, augment_z)
        apa_w = self._apa_rows(images_real, apa_w)
        with profiling.range("D phase"):
            features_real, loss_d_real, loss_d_fake = self._d_phase(images_real, labels, labels_f, masks, noise_d,
                                                                      self._features_ahead(images_real), noise_g, aug_u, aug_v, aug_z=aug_z,
                                                                      apa_w=apa_w)
            self._start_reduce("d", self._d_params, eager=True)
        with profiling.range("G forward"):
            images_fake, noise_g = self._g_forward(images_real, labels_f, masks, features_real, noise_g)
            ahead = self._g_features(images_fake, noise_g, w_div, next_images_real)
        with profiling.range("Adam(D)"):
            self._join_reduce("d")
            self._optimizer_step("d", self.discriminator_optimizer)
        with profiling.range("G rest"):
            loss_g, loss_rec, loss_div = self._g_rest(images_fake, noise_g, labels, masks, features_real, w_rec, w_div, next_images_real,
                                                      ahead=ahead, aug_u=aug_u, aug_t=self._aug_tables, aug_c=self._aug_ctables)
            self._start_reduce("g", self._g_params, eager=True)
        with profiling.range("Adam(G)"):
            self._join_reduce("g")
            self._optimizer_step("g", self.generator_optimizer)
            if self._adaptive():
                self._ada.adjust(images_real.shape[0])
            if self._apa_adaptive():
                self._apa.adjust(images_real.shape[0])
        self.iterations += 1
        out = self._with_augment_p(self._with_grad_norms({"loss_discriminator_real": loss_d_real.detach(), "loss_discriminator_fake": loss_d_fake.detach(),
                                     "loss_generator": loss_g.detach(), "loss_generator_semantic_reconstruction": loss_rec.detach().reshape(()),
                                     "loss_generator_diversity": loss_div.detach(), "images_fake": images_fake.detach()}))
        return self._with_apa(self._with_lecam(out, self._lecam_reg))

    # ------------------------------------------------------------------------------------------
    def capture_graphs(self, images_real: torch.Tensor, labels: torch.Tensor, masks, w_rec: float = 0.1, w_div: float = 0.1) -> None:
        """Records train_step as THREE HIP graphs over static copies of the inputs - the D phase, the generator forward of the G
        phase, the rest of the G phase (~1000 kernel launches together); train_step_graphed() then costs three graph launches
        plus the two optimizer steps, so the step time no longer depends on how fast the host can enqueue.  The cut after the
        generator forward is where a multi-GPU run hides the discriminator's gradient all-reduce (distributed.py).  The shapes
        are static (fixed batch, 256x256); call after a few eager steps (lazy state: packed VGG weights, kernel
        attributes).  The two latent draws stay eager (two tiny launches into static buffers), so the device RNG is
        consumed exactly as in train_step()."""
        import gc
        for bank in self._banks.values():
            if bank.flat is None:
                raise RuntimeError("capture_graphs(): run at least one eager train_step() first (the flat gradient buffers and the "
                                   "packed VGG weights are allocated lazily and must not be born inside a graph's memory pool)")
        self.generator.zero_grad()
        self.discriminator.zero_grad()
        gc.collect()                       # no autograd nodes of earlier (eager-stream) iterations may survive into the capture
        torch.cuda.synchronize()
        st = self._graph_state = {}
        st["flat_ptrs"] = self._flat_ptrs()
        st["images"], st["labels"], st["masks"] = images_real.clone(), labels.clone(), [m.clone() for m in masks]
        st["w"] = (w_rec, w_div)
        st["mode"] = self._mode_key()
        zdim = (images_real.shape[0], self.latent_dimensions)
        st["noise_d"] = torch.zeros(zdim, dtype=torch.float32, device=images_real.device)
        st["noise_g"] = torch.zeros(zdim, dtype=torch.float32, device=images_real.device)
        # the step's uniforms of the augmentation: a static buffer the transform launches INSIDE the graphs decode on the device;
        # train_step_graphed refills it in front of every replay (None with augmentation off: no buffer, no draw)
        st["augment_u"] = (torch.zeros((3, zdim[0], 8), dtype=torch.float32, device=images_real.device)
                           if self._aug_policy or self._aug_geom or self._aug_cmat else None)
        # likewise the uniforms of the geometric words and the tables the first graph's decode launch writes and all three transforms read
        st["augment_v"] = torch.zeros((3, zdim[0], 4), dtype=torch.float32, device=images_real.device) if self._aug_geom else None
        st["augment_t"] = torch.zeros((3 * zdim[0], 8), dtype=torch.float32, device=images_real.device) if self._aug_geom else None
        # and the uniforms of the color-matrix words with the matrices the first graph's second decode launch writes
        st["augment_z"] = torch.zeros((3, zdim[0], 8), dtype=torch.float32, device=images_real.device) if self._aug_cmat else None
        st["augment_c"] = torch.zeros((3 * zdim[0], 12), dtype=torch.float32, device=images_real.device) if self._aug_cmat else None
        # and the uniforms of the pseudo augmentation with the batch D's real branch reads (None with APA off: no buffer, no draw)
        st["apa_w"] = torch.zeros((zdim[0],), dtype=torch.float32, device=images_real.device) if self._apa is not None else None
        st["apa_images"] = torch.zeros_like(images_real, dtype=torch.float32, memory_format=torch.contiguous_format) if self._apa is not None else None
        # The pyramid of the real images is computed AHEAD (config.CFG.vgg_pair): the generator-step graph takes the next batch's real
        # images (st["images_next"]) through the VGG pass it makes over the fake images and leaves their features in st["feats_real"],
        # which the discriminator-step graph of the next replay reads.  Eager once here, so that the first replay finds them.
        st["feats_real"] = None
        if self._vgg_pair_ok(st["images"], st["images"]):
            with torch.no_grad():
                st["feats_real"] = [f.detach().clone() for f in self.vgg16(st["images"])]
            st["images_next"] = st["images"].clone()
            st["next_is_resident"] = True      # st["images_next"] holds what st["images"] holds (until a caller streams batches in)
            st["resident_ok"] = True           # st["feats_real"] is the pyramid of what st["images"] holds
            st["announced"] = None             # (tensor, version) whose pyramid st["feats_real"] holds, if a caller announced it
        handed_over = self._vgg_ahead      # the eager iteration in front of this capture announced its successor
        self._vgg_ahead = None
        # the zero-at-rest counters of the convolution kernels' K-split (ops._split_sync) are per stream: create the capture stream's
        # area BEFORE the capture, so that its zero fill is not a node of every replay
        if torch.cuda.graph.default_capture_stream is None:
            torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
        with torch.cuda.stream(torch.cuda.graph.default_capture_stream):
            ops._split_sync(images_real.device)
        torch.cuda.synchronize()
        self._capturing = True
        try:
            gd = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gd):
                cls = st["cls"] = _class_index(st["labels"])          # recomputed by every replay of this graph; the other two read it
                lab_d = cls if isinstance(self.discriminator, Discriminator) else st["labels"]      # (a caller's own module gets what it was written for)
                lab_g = cls if isinstance(self.generator, Generator) else st["labels"]
                feats, l_real, l_fake = self._d_phase(st["images"], lab_d, lab_g, st["masks"], st["noise_d"], st["feats_real"], st["noise_g"],
                                                      st["augment_u"], st["augment_v"], st["augment_t"], st["augment_z"], st["augment_c"],
                                                      st["apa_w"], st["apa_images"])
            st["lecam_reg"] = self._lecam_reg                      # (None with LeCam off) the first graph's static output
            st["d_grads"] = [p.grad for p in self._d_params]
            # second graph: what the generator step can do in front of the discriminator's optimizer step - its forward, unless that rode
            # in the discriminator phase's pass (Generator.forward_pair), the diversity loss and the VGG-16 pass over the fake images
            gf = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf, pool=gd.pool()):
                fake, _ = self._g_forward(st["images"], lab_g, st["masks"], feats, st["noise_g"])
                ahead = self._g_features(fake, st["noise_g"], w_div, st.get("images_next"))
            st["noise_g_early"] = self._g_pair_ok()             # both latents feed the FIRST graph then
            gg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gg, pool=gd.pool()):
                l_g, l_rec, l_div = self._g_rest(fake, st["noise_g"], lab_d, st["masks"], feats, w_rec, w_div, st.get("images_next"),
                                                 st["feats_real"], ahead=ahead, aug_u=st["augment_u"], aug_t=self._aug_tables,
                                                 aug_c=self._aug_ctables)
            st["g_grads"] = [p.grad for p in self._g_params]
        except BaseException:
            ops.drop_wgrad_reduce()            # queued slab reductions of the abandoned capture point into its (released) pool
            self._graph_state = None
            raise
        finally:
            self._capturing = False
            self._vgg_ahead = None
            self._fake_ahead = None
        if handed_over is not None and st["feats_real"] is not None and handed_over[0]._version == handed_over[1]:
            with torch.no_grad():                               # ... the first replay finds that batch's pyramid as the eager loop would
                for dst, src in zip(st["feats_real"], handed_over[2]):
                    dst.copy_(src)
            st["announced"] = (handed_over[0], handed_over[1])
            st["resident_ok"] = handed_over[0] is images_real       # (the resident batch announced as its own successor: bench.py)
        st["gd"], st["gf"], st["gg"], st["feats"] = gd, gf, gg, feats
        st["out"] = {"loss_discriminator_real": l_real.detach(), "loss_discriminator_fake": l_fake.detach(),
                     "loss_generator": l_g.detach(), "loss_generator_semantic_reconstruction": l_rec.detach().reshape(()),
                     "loss_generator_diversity": l_div.detach(), "images_fake": fake.detach()}

    def _flat_ptrs(self):
        """Addresses of the two networks' flat gradient buffers (None where not allocated): what captured graphs are tied to."""
        out = []
        for net in (self.generator, self.discriminator):
            bank = getattr(net, "_bank", None)
            flat = getattr(bank, "flat", None) if bank is not None else None
            out.append(flat.data_ptr() if flat is not None else None)
        return tuple(out)

    def train_step_graphed(self, images_real: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, masks=None,
                           noise_d: Optional[torch.Tensor] = None, noise_g: Optional[torch.Tensor] = None,
                           next_images_real: Optional[torch.Tensor] = None, augment_u: Optional[torch.Tensor] = None,
                           augment_v: Optional[torch.Tensor] = None, augment_z: Optional[torch.Tensor] = None,
                           apa_w: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """train_step() through the captured graphs (capture_graphs() first).  images / labels / masks: new batch to copy into
        the graphs' static inputs, or None to reuse the resident one.  next_images_real: as in train_step() - the next call's real
        images, whose VGG pyramid this call computes ahead; without it (and outside the resident mode) the next call computes its
        pyramid eagerly in front of its first graph.  The returned tensors are the graphs' static outputs: they are overwritten by
        the next call."""
        st = self._graph_state
        if st is None or st.get("flat_ptrs") != self._flat_ptrs():
            self._graph_state = None
            raise RuntimeError("train_step_graphed(): the networks' flat gradient buffers were re-allocated after capture_graphs() "
                               "(parameters or compute dtype changed) - capture again")
        if st.get("augment_u") is None:
            self._augment_rows(st["images"], augment_u)         # (augmentation off: raises if the caller brings uniforms)
        elif augment_u is None:
            st["augment_u"].uniform_()                          # first, as train_step() draws: the same RNG stream
        else:
            st["augment_u"].copy_(self._augment_rows(st["images"], augment_u))
        if st.get("augment_v") is None:
            self._augment_geom_rows(st["images"], augment_v)    # (no geometric words: raises if the caller brings uniforms)
        elif augment_v is None:
            st["augment_v"].uniform_()                          # right behind the first draw, as train_step() draws
        else:
            st["augment_v"].copy_(self._augment_geom_rows(st["images"], augment_v))
        if st.get("augment_z") is None:
            self._augment_cmat_rows(st["images"], augment_z)    # (no color-matrix words: raises if the caller brings uniforms)
        elif augment_z is None:
            st["augment_z"].uniform_()                          # behind the draws above and in front of the latents, as train_step() draws
        else:
            st["augment_z"].copy_(self._augment_cmat_rows(st["images"], augment_z))
        if st.get("apa_w") is None:
            self._apa_rows(st["images"], apa_w)                 # (APA off: raises if the caller brings uniforms)
        elif apa_w is None:
            st["apa_w"].uniform_()                              # behind the augmentation's draws and in front of the latents, as train_step() draws
        else:
            st["apa_w"].copy_(self._apa_rows(st["images"], apa_w))
        if noise_d is None:
            st["noise_d"].normal_()
        else:
            st["noise_d"].copy_(noise_d)
        if st["noise_g_early"]:                                 # both generator forwards run in the first graph: it needs both draws
            if noise_g is None:
                st["noise_g"].normal_()
            else:
                st["noise_g"].copy_(noise_g)
        ahead = st.get("feats_real") is not None
        feats_ok = ahead and st["resident_ok"]                  # resident batch: its pyramid is what the last replay left behind
        if images_real is not None and images_real is not st["images"]:
            st["images"].copy_(images_real, non_blocking=True)
            if ahead:
                ann = st["announced"]
                feats_ok = ann is not None and ann[0] is images_real and ann[1] == images_real._version
                st["next_is_resident"] = False
        if ahead:
            if next_images_real is not None:
                st["images_next"].copy_(next_images_real, non_blocking=True)
                st["next_is_resident"] = False
                st["announced"] = (next_images_real, next_images_real._version)
            else:
                st["announced"] = None
                if images_real is None and not st["next_is_resident"]:
                    # back in the resident mode after streamed batches: the batch to take ahead is the resident one again (round-4
                    # ADVICE: the flag stayed False for good and every later resident replay recomputed its pyramid eagerly)
                    st["images_next"].copy_(st["images"])
                    st["next_is_resident"] = True
            # after this call st["feats_real"] holds the pyramid of st["images_next"]: the resident batch's only while both buffers agree
            st["resident_ok"] = st["next_is_resident"]
            if not feats_ok:                                    # nobody computed this batch's pyramid ahead: now, eagerly
                with torch.no_grad():
                    for dst, src in zip(st["feats_real"], self.vgg16(st["images"])):
                        dst.copy_(src)
        if labels is not None and labels is not st["labels"]:
            st["labels"].copy_(labels, non_blocking=True)
        if masks is not None and masks is not st["masks"]:
            for dst, src in zip(st["masks"], masks):
                dst.copy_(src, non_blocking=True)
        with profiling.range("D phase"):
            st["gd"].replay()
            for p, g in zip(self._d_params, st["d_grads"]):
                p.grad = g
            self._start_reduce("d", self._d_params, eager=False)
        if not st["noise_g_early"]:
            if noise_g is None:
                st["noise_g"].normal_()
            else:
                st["noise_g"].copy_(noise_g)
        with profiling.range("G forward"):
            st["gf"].replay()                                   # (generator forward,) diversity loss, VGG pass: overlap the D gradient all-reduce
        with profiling.range("Adam(D)"):
            self._join_reduce("d")
            self._optimizer_step("d", self.discriminator_optimizer)
        with profiling.range("G rest"):
            st["gg"].replay()
            for p, g in zip(self._g_params, st["g_grads"]):
                p.grad = g
            for p in self._d_params:
                p.grad = None
            self._start_reduce("g", self._g_params, eager=False)
        with profiling.range("Adam(G)"):
            self._join_reduce("g")
            self._optimizer_step("g", self.generator_optimizer)
            if self._adaptive():
                self._ada.adjust(st["images"].shape[0])             # eager, as the optimizer steps: p moves between replays
            if self._apa_adaptive():
                self._apa.adjust(st["images"].shape[0])
        self.iterations += 1
        return self._with_apa(self._with_lecam(self._with_augment_p(self._with_grad_norms(st["out"])), st.get("lecam_reg")))

    # ------------------------------------------------------------------------------------------
    def _batch_signature(self, images_real, labels, masks):
        return (tuple(images_real.shape), images_real.dtype, tuple(labels.shape), labels.dtype,
                tuple((tuple(m.shape), m.dtype) for m in masks), str(images_real.device))

    def _train_iteration(self, images_real, labels, masks, w_rec: float, w_div: float, next_images_real=None) -> Dict[str, torch.Tensor]:
        """One iteration of train(): the first ``graph_after_iterations`` batches (config.CFG.graph_after, default 3; 0 = never)
        run eagerly, then - the batch shapes being static, as with the reference's drop_last loader (main.py:80-88) - the step
        is captured once and every further batch of the same shapes REPLAYS the three HIP graphs (its tensors are copied into
        the graphs' static inputs).  A batch of other shapes, or any failure to capture, runs eagerly.  Replay and eager
        launches execute the same kernels in the same order on the same RNG stream: the logged metrics are identical
        (tests/test_gpu_frontdoor.py).  An iteration without an announced successor (next_images_real is None: an epoch's last) runs
        eagerly even after the capture: the captured generator-step graph always takes the NEXT batch's VGG pyramid in its pass
        over the fake images."""
        after = self.graph_after_iterations
        sig = self._batch_signature(images_real, labels, masks)
        st = self._graph_state
        if st is not None and st.get("flat_ptrs") != self._flat_ptrs():
            if self._reducer_active():
                # one rank replaying while another launches eagerly would pair different sequences of collectives (or hang); a
                # re-allocation is deterministic program state, so it either happens on every rank or is a bug: fail loudly
                raise RuntimeError("ModelWrapper.train(): the flat gradient buffers were re-allocated under a captured graph in a "
                                   "data-parallel job - re-create the ModelWrapper on every rank")
            st = self._graph_state = None                       # gradient buffers re-allocated: eager steps, then a fresh capture
            self._eager_run = 0
        if st is not None and st.get("sig") == sig and st.get("w") == (w_rec, w_div):
            # the captured generator-step graph takes the next batch's VGG pyramid in its pass over the fake images; an iteration
            # without a successor (an epoch's last) runs eagerly instead - the same kernels as the eager loop, one iteration per epoch
            if st.get("feats_real") is None or next_images_real is not None:
                return self.train_step_graphed(images_real, labels, masks, next_images_real=next_images_real)
            ann = st.get("announced")
            if ann is not None and ann[0] is images_real and ann[1] == images_real._version:
                self._vgg_ahead = (images_real, ann[1], st["feats_real"], st.get("mode"))       # computed ahead by the last replay
            st["announced"] = None
        out = self.train_step(images_real, labels, masks, w_rec=w_rec, w_div=w_div, next_images_real=next_images_real)
        if st is not None and st.get("sig") == sig and st.get("w") == (w_rec, w_div) and next_images_real is None:
            return out                                          # (an epoch's last iteration under a valid capture: nothing to re-capture)
        if st is not None and st.get("sig") == sig and st.get("w") != (w_rec, w_div):
            st = self._graph_state = None                       # other loss weights than the captured ones: capture again (round-4 ADVICE)
            self._eager_run = 0
        if after and after > 0 and images_real.is_cuda and not self._graph_failed:
            self._eager_run = self._eager_run + 1 if sig == self._eager_sig else 1
            self._eager_sig = sig
            if self._eager_run >= after:
                try:
                    self.capture_graphs(images_real, labels, masks, w_rec=w_rec, w_div=w_div)
                    self._graph_state["sig"] = sig
                except Exception as exc:                  # a caller's module the capture cannot hold: stay eager, say so once
                    self._graph_state = None
                    self._graph_failed = True
                    import warnings
                    warnings.warn("ModelWrapper.train(): HIP-graph capture failed (%s); continuing with eager launches" % (exc,))
                if self._reducer_active() and not self._ranks_agree(self._graph_state is not None):
                    # data parallelism: every rank replays or none does (bench.py does the same) - the eager path hands its
                    # gradient ranges over group by group, the replay path bucket by bucket: mixed ranks would mismatch
                    self._graph_state = None
                    self._graph_failed = True
        return out

    def _reducer_active(self) -> bool:
        return self.gradient_reducer is not None and self.gradient_reducer.active()

    def _ranks_agree(self, ok: bool) -> bool:
        """all-reduce(MIN) of a per-rank flag over the reducer's process group (one host sync, once per capture attempt)."""
        import torch.distributed as dist
        red = self.gradient_reducer
        dev = next(self.generator.parameters()).device
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev if dist.get_backend(red.group) == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=red.group)
        return bool(int(flag.item()))

    def _device_batches(self, device):
        """One pass over the training loader: (images, labels, masks, next batch's images or None), every batch moved to the device when
        it is FETCHED - one batch ahead where config.CFG.vgg_pair is on, so that an iteration can hand the next one's real images to the
        frozen VGG-16 together with its own fake images (train_step: next_images_real).  The tensors are those of model_wrapper.py:
        133-135; a next batch of another shape (a last, smaller batch) is simply not announced."""
        def fetch(it):
            batch = next(it, None)
            if batch is None:
                return None
            images_real, labels, masks = batch
            return images_real.detach().to(device), labels.to(device), [m.detach().to(device) for m in masks]
        it = iter(self.training_dataset)
        cur = fetch(it)
        while cur is not None:
            nxt = fetch(it) if CFG.vgg_pair else None
            ahead = nxt[0] if nxt is not None and nxt[0].shape == cur[0].shape else None
            yield cur[0], cur[1], cur[2], ahead
            cur = nxt if CFG.vgg_pair else fetch(it)

    def train(self, epochs: int = 20, validate_after_n_iterations: int = 100000, device: str = 'cuda',
              save_model_after_n_epochs: int = 1, w_rec: float = 0.1, w_div: float = 0.1) -> None:
        """model_wrapper.py:93-228."""
        from tqdm import tqdm
        self.logger.hyperparameter['w_rec'] = str(w_rec)
        self.logger.hyperparameter['w_div'] = str(w_div)
        bs = self.training_dataset.batch_size
        validate_after_n_iterations = max(bs, (validate_after_n_iterations // bs) * bs)
        self.generator.train()
        self.discriminator.train()
        self.vgg16.eval()
        self.generator.to(device)
        self.discriminator.to(device)
        self.vgg16.to(device)
        self.progress_bar = tqdm(total=epochs * len(self.training_dataset.dataset), dynamic_ncols=True)
        self.progress_bar.set_description('Validation')
        self.inference(device=device)
        fid = self.validate()
        names = ("loss_generator_diversity", "loss_generator_semantic_reconstruction", "loss_generator",
                 "loss_discriminator_fake", "loss_discriminator_real")
        if self.clip_grad_norm is not None:                     # the two gradient norms ride in the same host transfer
            names += ("grad_norm_discriminator", "grad_norm_generator")
        if self._adaptive():                                    # ... and so do the gate's probability and its signal
            names += ("augment_p", "augment_rt")
        if self._lecam is not None:                             # ... and the regularizer with its two anchors
            names += ("loss_discriminator_lecam", "lecam_anchor_real", "lecam_anchor_fake")
        if self._apa_adaptive():                                # ... and the pseudo augmentation's probability and signal
            names += ("apa_p", "apa_rt")
        for epoch in range(epochs):
            self.generator.train()
            self.discriminator.train()
            self.vgg16.eval()
            for images_real, labels, masks, next_images_real in self._device_batches(device):
                self.progress_bar.update(n=images_real.shape[0])
                out = self._train_iteration(images_real, labels, masks, w_rec, w_div, next_images_real)
                vals = torch.stack([out[n].float().reshape(()) for n in names]).tolist()      # the single host sync
                l_div, l_rec, l_g, l_df, l_dr = vals[:5]
                self.progress_bar.set_description(
                    'FID={:.4f}, Loss Div={:.4f}, Loss Rec={:.4f}, Loss G={:.4f}, Loss D={:.4f}'.format(
                        fid, l_div, l_rec, l_g, l_df + l_dr))
                self.logger.log(metric_name='loss_discriminator_real', value=l_dr)
                self.logger.log(metric_name='loss_discriminator_fake', value=l_df)
                self.logger.log(metric_name='loss_generator', value=l_g)
                self.logger.log(metric_name='loss_generator_semantic_reconstruction', value=l_rec)
                self.logger.log(metric_name='loss_generator_diversity', value=l_div)
                for n, v in zip(names[5:], vals[5:]):
                    self.logger.log(metric_name=n, value=v)
                self.logger.log(metric_name='iterations', value=self.progress_bar.n)
                self.logger.log(metric_name='epoch', value=epoch)
                if self.progress_bar.n % validate_after_n_iterations == 0:
                    self.progress_bar.set_description('Validation')
                    fid = self.validate()
                    self.inference(device=device)
                    self.logger.log(metric_name='fid', value=fid)
                    if self.metrics and self.last_metrics is not None:
                        for key, value in self.last_metrics.items():
                            if key != 'fid':
                                self.logger.log(metric_name=key, value=value)
                    if self.reconstruction:
                        for key, value in self.evaluate_reconstruction(device=device).items():
                            self.logger.log(metric_name=key, value=value)
                    self.logger.log(metric_name='iterations_fid', value=self.progress_bar.n)
                    if self.path_save_metrics is not None:
                        self.logger.save_metrics(self.path_save_metrics)
            if epoch % save_model_after_n_epochs == 0 and self.path_save_models is not None:
                checkpoint = {"generator": self.generator.state_dict(),
                              "discriminator": self.discriminator.state_dict(),
                              "generator_optimizer": self.generator_optimizer.state_dict(),
                              "discriminator_optimizer": self.discriminator_optimizer.state_dict()}
                ema = self.generator_ema
                if ema is not None and ema.num_updates > 0:
                    # beyond the four reference keys: a state dict a Generator loads as it is (averaged parameters, live buffers)
                    checkpoint["generator_ema"] = ema.averaged_state_dict(self.generator)
                    checkpoint["generator_ema_state"] = {"decay": ema.decay, "warmup": ema.warmup, "num_updates": ema.num_updates}
                if self._adaptive():
                    checkpoint["augment_state"] = self._ada.state_dict()
                if self._lecam is not None:
                    checkpoint["lecam_state"] = self._lecam.state_dict()
                if self._apa_adaptive():
                    checkpoint["apa_state"] = self._apa.state_dict()
                torch.save(checkpoint,
                           os.path.join(self.path_save_models, 'checkpoint_{}.pt'.format(str(epoch).zfill(3))))
            self.inference(device=device)
            if self.path_save_metrics is not None:
                self.logger.save_metrics(self.path_save_metrics)
        self.progress_bar.close()

    def load_generator_ema(self, checkpoint_or_state) -> None:
        """Restores the generator's weight average for a resumed run (the reference's main.py does not): a checkpoint of train()
        (its "generator_ema" / "generator_ema_state" keys) or a ParameterEMA.state_dict()."""
        ema = self.generator_ema
        if ema is None:
            raise ops.L.SempyrError("load_generator_ema(): this ModelWrapper keeps no generator average (generator_ema / SP_G_EMA)")
        state = checkpoint_or_state
        if "parameters" not in state:
            if "generator_ema" not in state:
                raise ops.L.SempyrError("load_generator_ema(): neither a ParameterEMA state nor a checkpoint with a 'generator_ema' key")
            state = dict(state.get("generator_ema_state", {}), parameters=state["generator_ema"])
        ema.load_state_dict(state)

    def load_augment_state(self, checkpoint_or_state) -> None:
        """Restores the adaptive augmentation's controller for a resumed run: a checkpoint of train() (its "augment_state" key) or an
        AdaptiveAugment.state_dict().  The device state is written in place: captured graphs stay valid."""
        if not self._adaptive():
            raise ops.L.SempyrError("load_augment_state(): this ModelWrapper steers no augmentation probability (augment_p / SP_AUGMENT_P)")
        state = checkpoint_or_state
        if "state" not in state:
            if "augment_state" not in state:
                raise ops.L.SempyrError("load_augment_state(): neither an AdaptiveAugment state nor a checkpoint with an 'augment_state' key")
            state = state["augment_state"]
        self._ada.load_state_dict(state)

    def load_apa_state(self, checkpoint_or_state) -> None:
        """Restores the pseudo augmentation's controller for a resumed run: a checkpoint of train() (its "apa_state" key) or an
        AdaptiveAugment.state_dict().  The device state is written in place: captured graphs stay valid."""
        if not self._apa_adaptive():
            raise ops.L.SempyrError("load_apa_state(): this ModelWrapper steers no pseudo-augmentation probability (apa / SP_APA)")
        state = checkpoint_or_state
        if "state" not in state:
            if "apa_state" not in state:
                raise ops.L.SempyrError("load_apa_state(): neither an AdaptiveAugment state nor a checkpoint with an 'apa_state' key")
            state = state["apa_state"]
        self._apa.load_state_dict(state)

    def load_lecam_state(self, checkpoint_or_state) -> None:
        """Restores the LeCam anchors for a resumed run: a checkpoint of train() (its "lecam_state" key) or an ops.LeCam.state_dict().
        The device state is written in place: captured graphs stay valid."""
        if self._lecam is None:
            raise ops.L.SempyrError("load_lecam_state(): this ModelWrapper has no LeCam regularizer (lecam / SP_LECAM)")
        state = checkpoint_or_state
        if "state" not in state:
            if "lecam_state" not in state:
                raise ops.L.SempyrError("load_lecam_state(): neither an ops.LeCam state nor a checkpoint with a 'lecam_state' key")
            state = state["lecam_state"]
        self._lecam.load_state_dict(state)

    def _ema_scope(self, use_ema):
        """The context validate() / inference() run in: the generator's weight average swapped in (ParameterEMA.applied) where one
        exists and use_ema is None or true, else nothing.  use_ema=True without an average is an error."""
        import contextlib
        ema = self.generator_ema
        have = ema is not None and ema.num_updates > 0
        if use_ema and not have:
            raise ops.L.SempyrError("use_ema=True: there is no generator average (generator_ema / SP_G_EMA off, or no update yet)")
        if have and (use_ema is None or use_ema):
            return ema.applied()
        return contextlib.nullcontext()

    @torch.no_grad()
    def validate(self, device: str = 'cuda', use_ema=None) -> float:
        """With a generator weight average (generator_ema) the FID is the AVERAGED generator's unless use_ema is False.
        model_wrapper.py:231-244: the FID over the validation loader, generator in eval mode and back in train mode afterwards.
        The Inception-v3 weights are the constructor's ``inception`` or else CFG.inception_weights (SP_INCEPTION_WEIGHTS); with
        neither (or no validation loader) the result is nan.  `device` is accepted for main.py:111's call and ignored: the
        networks run where the generator's parameters are."""
        if self.metrics:
            return float(self.evaluate(device=device, use_ema=use_ema)["fid"])
        src = self._fid_extractor()
        if src is None:
            return float('nan')
        from .fid import frechet_inception_distance
        dev = next(self.generator.parameters()).device
        with self._ema_scope(use_ema):
            self.generator.eval()
            self.vgg16.eval()
            try:
                fid = frechet_inception_distance(dataset_real=self.validation_dataset_fid, generator=self.generator, vgg16=self.vgg16,
                                                 device=dev, inception=src)
            finally:
                self.generator.train()
        return float(fid)

    def _fid_extractor(self):
        """The Inception-v3 extractor of validate() / evaluate(), built once; None without weights or without a validation loader."""
        src = self._inception if self._inception is not None else (CFG.inception_weights or None)
        if src is None or self.validation_dataset_fid is None:
            return None
        from .inception import InceptionV3Features
        if not isinstance(src, InceptionV3Features):
            src = InceptionV3Features(src)
            self._inception = src                  # built once
        return src

    @torch.no_grad()
    def evaluate(self, device: str = 'cuda', use_ema=None) -> Dict[str, float]:
        """validate() as a dict: "fid" (the same value validate() returns for the same seed) and, from the SAME activations kept on the
        device, what the wrapper's ``metrics`` name - "kid"; "precision", "recall", "density", "coverage"; "inception_score",
        "inception_score_std" (of the generated images; needs fc.weight / fc.bias in the Inception state dict) (fid.evaluate, metrics.py).
        The same weight-average scope and eval / train handling as validate(); without weights or a loader every value is nan.  The
        dict is kept in ``last_metrics``."""
        from .metrics import IS_KEYS, PRDC_KEYS
        keys = ["fid"] + (["kid"] if "kid" in self.metrics else []) + (list(PRDC_KEYS) if "prdc" in self.metrics else [])
        keys += list(IS_KEYS) if "is" in self.metrics else []
        src = self._fid_extractor()
        if src is None:
            self.last_metrics = {k: float('nan') for k in keys}
            return dict(self.last_metrics)
        from .fid import evaluate
        dev = next(self.generator.parameters()).device
        with self._ema_scope(use_ema):
            self.generator.eval()
            self.vgg16.eval()
            try:
                out = evaluate(dataset_real=self.validation_dataset_fid, generator=self.generator, vgg16=self.vgg16, device=dev,
                               inception=src, metrics=self.metrics, nearest_k=self.metrics_nearest_k,
                               is_splits=self.metrics_is_splits)
            finally:
                self.generator.train()
        self.last_metrics = {k: float(out[k]) for k in keys}
        return dict(self.last_metrics)

    @torch.no_grad()
    def evaluate_reconstruction(self, device: str = 'cuda', use_ema=None) -> Dict[str, float]:
        """Per-level reconstruction fidelity over the validation loader: {"psnr_level<s>", "ssim_level<s>", "ms_ssim_level<s>"} for the
        names of ``reconstruction`` and the levels of ``reconstruction_levels`` - the float64 mean over all validation images of the score
        of each image against the generator's output from level s of that image's own VGG-16 pyramid (reconstruction.evaluate_levels;
        level s = inference()'s stage index, the loader's masks are ignored).  The same weight-average scope and eval / train handling as
        evaluate(); it needs no Inception weights.  {} when the option is off or there is no validation loader.  A psnr mean over a set
        with an identical pair is inf.  The dict is kept in ``last_reconstruction``.  `device` is accepted and ignored, as in validate()."""
        if not self.reconstruction or self.validation_dataset_fid is None:
            self.last_reconstruction = {}
            return {}
        from .reconstruction import evaluate_levels
        dev = next(self.generator.parameters()).device
        with self._ema_scope(use_ema):
            self.generator.eval()
            self.vgg16.eval()
            try:
                out = evaluate_levels(dataset_real=self.validation_dataset_fid, generator=self.generator, vgg16=self.vgg16, device=dev,
                                      levels=self.reconstruction_levels, names=self.reconstruction)
            finally:
                self.generator.train()
        self.last_reconstruction = {k: float(v) for k, v in out.items()}
        return dict(self.last_reconstruction)

    @torch.no_grad()
    def inference(self, device: str = 'cuda', use_ema=None) -> None:
        """With a generator weight average (generator_ema) the samples are the AVERAGED generator's unless use_ema is False.
        model_wrapper.py:247-296: 7 validation images x the 7 single-stage mask sets (misc.get_masks_for_inference), one fake image
        each from a fresh latent, generator in eval mode, saved as the reference's 7 x 7 grid ``predictions_<n>.png`` (every image
        scaled to [0, 1] by its own range, misc.normalize_0_1_batch); the generator goes back to training mode.  The draws follow the
        reference's order: np.random.choice over range(len(validation loader)), then one torch.randn per (image, stage)."""
        if self.validation_dataset_fid is None or self.path_save_plots is None:
            return
        from .data import image_label_list_of_masks_collate_function
        import numpy as np
        self.generator.to(device)
        self.vgg16.to(device)
        with self._ema_scope(use_ema):
            self.generator.eval()
            try:
                idx = np.random.choice(range(len(self.validation_dataset_fid)), replace=False, size=7)
                images, labels, _ = image_label_list_of_masks_collate_function([self.validation_dataset_fid.dataset[i] for i in idx])
                masks_levels = [misc.get_masks_for_inference(stage, add_batch_size=True, device=device) for stage in range(7)]
                fakes = torch.empty((7 ** 2,) + tuple(images.shape[1:]), dtype=torch.float32, device=device)
                counter = 0
                for image, label in zip(images, labels):
                    image, label = image.detach().to(device)[None], label.to(device)[None]
                    feats = self.vgg16(image)                      # (frozen, eval mode: the reference recomputes the same pyramid per stage)
                    for masks in masks_levels:
                        z = torch.randn(1, self.latent_dimensions, dtype=torch.float32, device=device)
                        fakes[counter] = self.generator(input=z, features=feats, masks=masks, class_id=label.float()).float()[0]
                        counter += 1
                n = getattr(self, "progress_bar", None)
                misc.save_image_grid(misc.normalize_0_1_batch(fakes), os.path.join(self.path_save_plots, 'predictions_{}.png'.format(n.n if n is not None else 0)),
                                     nrow=7)
            finally:
                self.generator.train()
