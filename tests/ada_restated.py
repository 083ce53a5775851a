"""The adaptive augmentation (csrc/augment.hip: the gate and its controller) restated for the tests: the controller
in numpy int32 / float32, the gate composed from tests/augment_restated.py - per image, its forward / backward where the image is live
and the identity where it is dead - and one gated training step on the oracle.  Not a test module; nothing here runs on a GPU.

THE DEFINITION (include/sempyr.h).  Image n is live iff float32(u[n, 7]) < float32(p), strictly.  The controller's state is eight 32-bit
words {p, r_last, pos, neg, total, steps, adjustments, reserved}:
    observe(x, threshold)   pos += #(x > threshold), neg += #(x < threshold), total += len(x); equal values and NaN count in total only
    adjust(interval, target, step)   steps += 1; at steps >= interval: steps = 0 and, if total > 0,
        r = float32(pos - neg) / float32(total)          (conversions round to nearest, one fp32 division)
        p = min(1, max(0, p + d)), d = step if r > target, -step if r < target, else 0          (one fp32 addition)
        r_last = r; pos = neg = total = 0; adjustments += 1"""
import numpy as np
import torch

import augment_restated as A
from oracle import sempyr_oracle as O

F = np.float32


class Controller:
    """The eight words as numpy scalars of their own types: every operation below is the one the kernel performs, in its precision."""

    def __init__(self, p=0.0):
        self.p, self.r_last = F(p), F(0.0)
        self.pos = self.neg = self.total = self.steps = self.adjustments = np.int32(0)

    def observe(self, x, threshold):
        x, t = np.asarray(x, dtype=F).reshape(-1), F(threshold)
        self.pos = np.int32(self.pos + np.count_nonzero(x > t))          # a comparison with NaN is false on both sides
        self.neg = np.int32(self.neg + np.count_nonzero(x < t))
        self.total = np.int32(self.total + x.size)

    def adjust(self, interval, target, step):
        target, step = F(target), F(step)
        self.steps = np.int32(self.steps + 1)
        if self.steps < interval:
            return
        self.steps = np.int32(0)
        if self.total <= 0:
            return
        r = F(F(np.int32(self.pos - self.neg)) / F(self.total))
        d = step if r > target else (F(-step) if r < target else F(0.0))
        self.p = F(min(F(1.0), max(F(0.0), F(self.p + d))))
        self.r_last = r
        self.pos = self.neg = self.total = np.int32(0)
        self.adjustments = np.int32(self.adjustments + 1)

    def words(self):
        """The state as the device holds it: 8 int32 words, the two floats by their bits."""
        return [int(np.array(self.p, dtype=F).view(np.int32)), int(np.array(self.r_last, dtype=F).view(np.int32)), int(self.pos), int(self.neg),
                int(self.total), int(self.steps), int(self.adjustments), 0]


def live(u, p):
    """(n,) bool: u[:, 7] < p, both as fp32, strictly."""
    u7 = u.detach().to("cpu", torch.float32)[:, 7].numpy()
    return torch.from_numpy(u7 < F(p))


def _gate(fn, t, u, p, policy, dtype):
    """fn (augment_restated.forward / backward) on the live images, the identity on the dead ones."""
    keep = live(u, p)
    out = t.to(dtype)
    idx = torch.nonzero(keep).flatten()
    return out.index_copy(0, idx, fn(t[idx], u[idx], policy, dtype)) if idx.numel() else out


def forward(x, u, p, policy, dtype=torch.float64):
    """The gated transform: T(x_n; u_n) where image n is live, x_n where it is dead (differentiable)."""
    return _gate(A.forward, x, u, p, policy, dtype)


def backward(dy, u, p, policy, dtype=torch.float64):
    """Its closed-form gradient: augment_restated.backward where live, dy itself where dead."""
    return _gate(A.backward, dy, u, p, policy, dtype)


def train_step_gated(G, D, V, opt_g, opt_d, images_real, labels, masks, noise_d, noise_g, u, p, policy, w_rec=0.1, w_div=0.1,
                     skip_dead_d_wgrad=False):
    """augment_restated.train_step_augmented with the gate in front of each of the three transforms: the same p for all three, as the
    training step holds it constant.  Also returns D's predictions on the (gated) real images: what the controller observes."""
    T = lambda x, i: forward(x, u[i], p, policy, torch.float32)      # noqa: E731
    out = {}
    O.zero_grads(G); O.zero_grads(D)
    with torch.no_grad():
        feats_real = O.vgg16_forward(V, images_real)
        fake = O.generator_forward(G, noise_d, feats_real, masks, labels.float(), training=True)
    out["images_fake_d"] = fake
    pred_real = O.discriminator_forward(D, T(images_real, 0), labels, training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 1), labels, training=True)
    out["prediction_real"] = pred_real.detach().clone()
    l_real, l_fake = O.lsgan_discriminator_loss(pred_real, pred_fake)
    (l_real + l_fake).backward()
    out["grads_d"] = [q.grad.detach().clone() for q in O.trainable(D)]
    opt_d.step()
    O.zero_grads(G); O.zero_grads(D)
    if skip_dead_d_wgrad:
        d_params = O.trainable(D)
        for q in d_params:
            q.requires_grad_(False)
    fake = O.generator_forward(G, noise_g, feats_real, masks, labels.float(), training=True)
    pred_fake = O.discriminator_forward(D, T(fake, 2), labels, training=True)
    l_g = O.lsgan_generator_loss(pred_fake)
    l_div = w_div * O.diversity_loss(fake, noise_g)
    feats_fake = O.vgg16_forward(V, fake)
    l_rec = w_rec * O.semantic_reconstruction_loss(feats_real, feats_fake, masks)
    (l_g + l_rec + l_div).backward()
    if skip_dead_d_wgrad:
        for q in d_params:
            q.requires_grad_(True)
    out["grads_g"] = [q.grad.detach().clone() for q in O.trainable(G)]
    opt_g.step()
    out.update(images_fake_g=fake.detach(), loss_d_real=l_real.detach(), loss_d_fake=l_fake.detach(), loss_g=l_g.detach(),
               loss_rec=l_rec.detach().reshape(()), loss_div=l_div.detach())
    return out
