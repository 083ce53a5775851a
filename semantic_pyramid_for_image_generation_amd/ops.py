"""Host-side operators: torch.autograd.Function wrappers that enqueue the libsempyr.so kernels.

PyTorch is plumbing here (device memory, streams, the autograd graph); every arithmetic pass over an
activation or weight goes through the C ABI of include/sempyr.h.  Activations are torch tensors of
LOGICAL shape (N, C, H, W) whose memory is dense NHWC ("channels_last"), in the compute dtype
(float32 for the parity mode, bfloat16 for the throughput mode, float16 for BASELINE.json config 5); 2-D activations are (B, K)
row-major.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List, Optional, Sequence

import torch

from . import _lib as L
from .config import CFG

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = L.ACT_NONE, L.ACT_LRELU, L.ACT_RELU, L.ACT_TANH

_STATE = {"dtype": torch.float32, "vgg_fp8": int(CFG.vgg_fp8), "loss_scale": float(CFG.f16_loss_scale)}


def set_compute_dtype(dtype: torch.dtype) -> None:
    """float32: exact-fp32 MFMA path used for parity; bfloat16: bf16 MFMA, fp32 accumulate; float16 (BASELINE.json config 5,
    "fp16 activations"): the same kernels compiled for IEEE half storage / v_mfma_f32_16x16x32_f16 (SP_F16) - 10 mantissa bits
    instead of 7, but 5 exponent bits: ModelWrapper multiplies the loss gradient by loss_scale() so that the activation
    gradients (1e-5 ... 1e-9 in this network: means over 51 200 / 5.2 M elements) stay above fp16's 6e-5 normal range, and
    divides the parameter gradients by it again (they are fp32 in every mode)."""
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("compute dtype must be torch.float32, torch.bfloat16 or torch.float16")
    _STATE["dtype"] = dtype


def is_16bit(dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16)


def loss_scale() -> float:
    """The fp16 mode's INITIAL loss scale (config.CFG.f16_loss_scale, default 2^16; set_loss_scale); 1.0 outside the fp16 mode - and 1.0
    means "no scaling".  The scale in force lives on the device and moves (loss_scaler)."""
    return float(_STATE["loss_scale"]) if _STATE["dtype"] == torch.float16 else 1.0


def set_loss_scale(value: float, growth: float = 2.0, backoff: float = 0.5, growth_interval: int = 2000) -> None:
    """(Re)starts the fp16 mode's loss scale at `value` (1.0 switches scaling off) with torch.cuda.amp.GradScaler's policy: an
    optimizer step whose gradients hold an inf / NaN is skipped and the scale multiplied by `backoff`; after `growth_interval`
    clean optimizer steps it is multiplied by `growth`."""
    _STATE["loss_scale"] = float(value)
    _STATE["ls_policy"] = (float(growth), float(backoff), int(growth_interval))
    # existing device states are re-initialised IN PLACE: captured graphs have their address baked in (backward seeds, the unscale pass,
    # the spectral-norm backward's 1 / scale, the overflow flag) - dropping the tensor would leave replays on freed memory while the
    # optimizer guard watched a new one (round-5 ADVICE)
    for sc in _SCALERS.values():
        sc.state.copy_(torch.tensor([float(value), 1.0 / float(value), 0.0, 0.0, 0.0], dtype=torch.float32))


class LossScaler:
    """Device state of the dynamic loss scale: {scale, 1 / scale, clean steps, non-finite found, steps skipped} (include/sempyr.h:
    sp_loss_scale_update).  Everything that uses the scale reads it from device memory when its kernel RUNS - the seeds of
    .backward() are views of state[0], the batched spectral-norm backward and the unscale pass take a pointer to state[1] - so a
    captured graph follows the scale without a re-capture and nothing ever syncs with the host (round-4 ADVICE: the static 2^16
    had no overflow check - one inf in an fp16 activation gradient would have poisoned Adam's moments for good)."""

    def __init__(self, device, scale: float):
        self.state = torch.tensor([scale, 1.0 / scale, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    @property
    def inv_ptr(self):
        return ctypes.c_void_p(self.state.data_ptr() + 4)

    @property
    def found_ptr(self):
        return ctypes.c_void_p(self.state.data_ptr() + 12)

    def check(self, flat: torch.Tensor) -> None:
        """found |= any non-finite value in `flat` (a network's flat gradient buffer, after the all-reduce where there is one)."""
        L.call("sp_check_finite", ptr(flat), flat.numel(), self.found_ptr, stream())

    def update(self) -> None:
        growth, backoff, interval = _STATE.get("ls_policy", (2.0, 0.5, 2000))
        L.call("sp_loss_scale_update", ptr(self.state), growth, backoff, interval, stream())

    def values(self) -> dict:
        """Host copy (syncs): for tests and reports."""
        s = self.state.tolist()
        return {"scale": s[0], "clean_steps": int(s[2]), "found": bool(s[3]), "skipped_steps": int(s[4])}


_SCALERS = {}


def loss_scaler(device) -> Optional[LossScaler]:
    """The dynamic loss scale of `device` (fp16 mode with scaling on), else None."""
    s = loss_scale()
    if s == 1.0:
        return None
    key = str(torch.device(device))
    sc = _SCALERS.get(key)
    if sc is None:
        sc = _SCALERS[key] = LossScaler(device, s)
    return sc


_SCALE_SEED = {}


def backward_seeds(losses) -> List[torch.Tensor]:
    """grad_tensors for torch.autograd.backward(losses, ...): d(sum of the losses) / d(loss) = 1 (times the fp16 mode's loss scale)
    per loss, as cached tensors of each loss's shape - summing the losses first and letting autograd make its own seed costs an add per
    loss, a fill and a reduction wherever the shapes differ (five tiny launches in the generator step).  fp16 mode: views of the
    device-resident scale (the losses are scalars / one-element tensors), so the seeds follow the dynamic scale."""
    out = []
    for t in losses:
        sc = loss_scaler(t.device)
        if sc is not None:
            if t.numel() != 1:
                raise L.SempyrError("the fp16 mode's loss scale seeds scalar losses only (got shape %s)" % (tuple(t.shape),))
            out.append(sc.state[0:1].reshape(t.shape))
            continue
        key = (str(t.device), tuple(t.shape))
        seed = _SCALE_SEED.get(key)
        if seed is None:
            seed = _SCALE_SEED[key] = torch.ones(tuple(t.shape), dtype=torch.float32, device=t.device)
        out.append(seed)
    return out


_LOSS_ACC = {}


def _loss_acc(device) -> torch.Tensor:
    """fp64 accumulators of the one-launch loss forms (include/sempyr.h: zero on entry, left zero): [0:2] diversity, [2] reconstruction."""
    t = _LOSS_ACC.get(str(device))
    if t is None:
        t = _LOSS_ACC[str(device)] = torch.zeros(4, dtype=torch.float64, device=device)
    return t


def unscale_(flat: torch.Tensor, start: int = 0) -> None:
    """flat[start:] *= 1 / (the loss scale in force), in place, one launch of the library (no-op outside the fp16 mode).  The
    spectral-normalised layers' gradients lose the scale inside the batched backward (sp_sn_backward_batched_dscaled); this is for the
    tail of a bank's buffer - the few parameters whose gradients arrive through autograd (ops.SpectralNormBank.collect_extra)."""
    sc = loss_scaler(flat.device)
    if sc is not None and flat.numel() > start:
        L.call("sp_scale_f32_dev", ctypes.c_void_p(flat.data_ptr() + 4 * start), flat.numel() - start, sc.inv_ptr, stream())


def compute_dtype() -> torch.dtype:
    return _STATE["dtype"]


def set_vgg_fp8(mode) -> None:
    """BASELINE.json config 5's fp8 slice: with 16-bit storage (bf16 or fp16), the 3x3 layers of the frozen VGG-16 pyramid that the
    ping-pong kernel covers (Cout > 64 on maps >= 32 wide: 8 of its 13 convolutions, 79 % of its FLOPs) run on the fp8 MFMA with
    e4m3 operands (per-channel filter scales, per-tensor activation scales by delayed scaling) in the NO-GRADIENT pass only
    (features of the real images, model_wrapper.py:144-146) - the pass whose activations no backward pass reads; everything else,
    and every backward, stays 16-bit.  1 / True: on; 0 / False: off (default).
    Off by default because it does not meet the bar it is held to (tests/test_gpu_fp8.py): e4m3 has 4 significant bits and the
    pyramid's dot products are sums of random-sign terms, so a tap carries 4-8 % relative noise however long the sum is; the
    reconstruction-loss gradient w.r.t. the image then keeps a cosine of ~0.45 with the fp32 gradient against 0.84 (bf16) / 0.99
    (fp16) for plain 16-bit storage.  Round 3's `mode 2` (the pass WITH gradient in e4m3 too: cosine 0.18) is gone."""
    mode = int(mode)
    if mode not in (0, 1):
        raise ValueError("set_vgg_fp8: 0 / 1 (the gradient-pass form of round 3 was removed: its gradient had cosine 0.18 with fp32)")
    _STATE["vgg_fp8"] = mode


def vgg_fp8() -> int:
    return int(_STATE.get("vgg_fp8", 0)) if is_16bit(_STATE["dtype"]) else 0


def sp_dtype(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return L.SP_F32
    if dtype == torch.bfloat16:
        return L.SP_BF16
    if dtype == torch.float16:
        return L.SP_F16
    raise TypeError("unsupported activation dtype %s" % dtype)


def chunk_elems(dtype: torch.dtype) -> int:
    return 4 if dtype == torch.float32 else 8


def pad_to(c: int, m: int) -> int:
    return (c + m - 1) // m * m


def pad_channels(c: int, dtype: torch.dtype) -> int:
    return pad_to(c, chunk_elems(dtype))


def stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def require_gpu(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise L.SempyrError("sempyr ops run on the GPU only (got a %s tensor); the CPU restatement lives in oracle/ "
                            "and is test infrastructure, not a fallback" % t.device)


def nhwc_empty(n: int, c: int, h: int, w: int, dtype, device) -> torch.Tensor:
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def nhwc_zeros(n: int, c: int, h: int, w: int, dtype, device) -> torch.Tensor:
    return torch.zeros((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def is_nhwc(t: torch.Tensor) -> bool:
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def as_nhwc(t: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Dense NHWC memory in `dtype` (layout/dtype conversion of foreign tensors only; ours already comply)."""
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if not is_nhwc(t):
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def as_rows(t: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t


def dims(t: torch.Tensor):
    n, c, h, w = t.shape
    return n, h, w, c


# ======================================================================================================
# spectral-norm bank: all SN layers of one network, normalised + packed by one batched call per forward
# ======================================================================================================
class PackedLayer:
    """Per-forward view of one layer: pointers into the pack arena / scratch of that forward, and where its weight
    gradient goes in the gradient arena of the matching backward."""
    __slots__ = ("fwd", "dgrad", "scratch", "rows", "cols", "cin", "taps", "cin_p", "cout_p", "kind", "keep", "module",
                 "call", "slot", "dw_off", "n_dw", "db_off")

    @property
    def handle(self):
        """This layer's output of _SNBankFn for the forward in flight (None without autograd).  The handles live on the
        bank only while the forward runs: the SNCall is referenced from the autograd node, so keeping them here would
        tie call -> handle -> node -> call into a cycle that keeps whole autograd graphs alive until the GC runs."""
        hs = self.call.bank.handles
        return hs[self.slot] if hs is not None else None


class SNCall:
    """One forward of a network's spectral-norm bank: packed weights + the (u, v, sigma) snapshots, plus - once a
    backward reaches it - the fp32 gradient arena [dW | dot | dbias] of every layer (zero-filled ONCE per backward pass;
    the weight-gradient kernels accumulate into their slots and _SNBankFn turns all of them into d weight_orig with one
    batched call)."""

    def __init__(self, bank: "SpectralNormBank", pack: torch.Tensor, scratch: torch.Tensor, dtype):
        self.bank, self.pack, self.scratch, self.dtype = bank, pack, scratch, dtype
        self.arena: Optional[torch.Tensor] = None
        self.touched, self.bias_touched = set(), set()
        self.layers: List[PackedLayer] = []
        for i, (spec, ent, lay) in enumerate(zip(bank.specs, bank.entries, bank.grad_layout)):
            p = PackedLayer()
            p.fwd = pack.data_ptr() + ent.fwd_off if ent.fwd_off >= 0 else 0
            p.dgrad = pack.data_ptr() + ent.dgrad_off if ent.dgrad_off >= 0 else 0
            p.scratch = scratch.data_ptr() + 4 * ent.scratch_off
            p.rows, p.cols, p.cin, p.taps, p.cin_p, p.cout_p, p.kind = (ent.rows, ent.cols, ent.cin, ent.taps,
                                                                       ent.cin_p, ent.cout_p, ent.kind)
            p.keep = (pack, scratch)
            p.module = spec[0]
            p.call, p.slot = self, i
            p.dw_off, p.n_dw, p.db_off = lay
            self.layers.append(p)

    def grad_arena(self) -> torch.Tensor:
        if self.arena is None:
            self.arena = torch.zeros(self.bank.arena_floats, dtype=torch.float32, device=self.scratch.device)
        return self.arena

    def dw_slot(self, p: PackedLayer) -> torch.Tensor:
        self.touched.add(p.slot)
        return self.grad_arena()[p.dw_off:p.dw_off + p.n_dw]

    def db_slot(self, p: PackedLayer) -> torch.Tensor:
        self.bias_touched.add(p.slot)
        return self.grad_arena()[p.db_off:p.db_off + p.rows]


_ZERO1 = {}


def _zero1(device) -> torch.Tensor:
    """Constant gradient handed to a layer's bank handle (the real gradient travels through the arena)."""
    z = _ZERO1.get(device)
    if z is None:
        z = _ZERO1[device] = torch.zeros(1, dtype=torch.float32, device=device)
    return z


class _SNBankFn(torch.autograd.Function):
    """weight_orig of the layers of ONE GROUP of a bank -> one 1-element handle per layer.  The layer functions take their
    handle as an input, so autograd runs this node's backward once all weight-gradient kernels of the group have accumulated
    into the arena; it then applies d(W/sigma)/dW to the group's layers in one batched call (torch.nn.utils.spectral_norm
    backward).  A bank is cut into a few groups of consecutive layers (SpectralNormBank.groups): the groups near the output
    finish early in the backward pass, which is what lets their gradient all-reduce start while the rest still computes."""

    @staticmethod
    def forward(ctx, call: SNCall, group: int, *weights):
        ctx.call, ctx.group = call, group
        dev = weights[0].device
        return tuple(torch.empty(1, dtype=torch.float32, device=dev) for _ in weights)

    @staticmethod
    def backward(ctx, *_):
        call, g = ctx.call, ctx.group
        bank = call.bank
        lo, hi = bank.groups[g]
        n = hi - lo
        if call.arena is None:
            return (None,) * (n + 2)
        if CFG.wgrad_side_stream:
            join_wgrad_stream(call.arena.device)          # weight-gradient launches that ran on the side stream wrote the arena
        flush_wgrad_reduce()                              # ... and the queued slab reductions of the pass add their sums to it now
        table = ctypes.c_void_p(bank.bwd_table_dev.data_ptr() + lo * ctypes.sizeof(L.SpSnBwdLayer))
        dots = torch.empty(n * 512, dtype=torch.float32, device=call.arena.device)     # per-block partial <dW, W> sums
        start, stop = bank.group_range[g]
        if bank.direct_grads:
            # direct mode: the gradients of every pass of the window meet in the bank's persistent flat buffer and the
            # parameters' .grad are views of it - autograd neither sums nor stores anything for these parameters
            bank.enter_backward(call.arena.device, g)
            prev = bank.flat if bank.group_count[g] > 0 else None
            # (fp16 mode: the loss scale in force comes off right here, where the fp32 parameter gradients are formed)
            sc = loss_scaler(call.arena.device)
            if sc is not None:
                L.call("sp_sn_backward_batched_dscaled", table, n, bank.max_elems, ptr(call.arena), ptr(call.scratch),
                       ptr(bank.flat), ptr(prev), ptr(bank.flat), ptr(dots), sc.inv_ptr, stream())
            else:
                L.call("sp_sn_backward_batched_scaled", table, n, bank.max_elems, ptr(call.arena), ptr(call.scratch),
                       ptr(bank.flat), ptr(prev), ptr(bank.flat), ptr(dots), 1.0, stream())
            bank.group_count[g] += 1
            for i in range(lo, hi):
                m = bank.specs[i][0]
                if i in call.touched:
                    bank.win_touched.add(i)
                if i in call.bias_touched:
                    bank.win_bias.add(i)
                if i in bank.win_touched and ctx.needs_input_grad[i - lo + 2]:
                    m.weight_orig.grad = bank.w_views[i]
                if i in bank.win_bias and m.bias.requires_grad:
                    m.bias.grad = bank.b_views[i]
            if bank.on_group_done is not None and bank.group_count[g] == bank.expected_passes:
                bank.on_group_done(start, stop)
            return (None,) * (n + 2)
        grads = torch.empty(stop - start, dtype=torch.float32, device=call.arena.device)
        # the table's offsets address the bank-wide flat layout: hand the kernel the base this group's slice would have there
        L.call("sp_sn_backward_batched", table, n, bank.max_elems, ptr(call.arena), ptr(call.scratch),
               ctypes.c_void_p(grads.data_ptr() - 4 * start), None, None, ptr(dots), stream())
        out = [None, None]
        for i in range(lo, hi):
            m = bank.specs[i][0]
            if i in call.touched and ctx.needs_input_grad[i - lo + 2]:
                off = bank.grad_offs[i] - start
                out.append(grads[off:off + m.weight_orig.numel()].view(m.weight_orig.shape))
            else:
                out.append(None)
        return tuple(out)


class SpectralNormBank:
    """specs: list of (module, kind, need_dgrad); module has weight_orig / weight_u / weight_v.
    kind: 'conv' (O,I,kh,kw), 'linear' (O,K), 'plain' (fp32 copy, e.g. the SN embedding)."""

    def __init__(self, specs: Sequence, extra_params: Sequence = ()):
        self.specs = list(specs)
        # layer groups of the batched backward: 1 = one launch pair per pass (single GPU); ModelWrapper asks for 4 when a
        # gradient reducer is attached, so that the late layers' gradients can go to the wire while the early ones still compute
        # (each extra group costs two small launches per backward pass: +0.18 ms per step at 4 groups, measured)
        self.n_groups = 1
        for i, (m, _, _) in enumerate(self.specs):
            m._sn_bank, m._sn_slot = self, i
        self.current: Optional[SNCall] = None
        self.handles = None
        self._key = None
        # direct_grads (opt-in, ModelWrapper sets it): the weight_orig / bias gradients are accumulated by the kernels into ONE
        # persistent flat fp32 buffer (`flat`) and param.grad are views of it.  A network that runs SEVERAL forward passes per
        # backward (D(real) and D(fake), model_wrapper.py:150-160) gets them summed there, without per-parameter autograd
        # additions; and the data-parallel reducer all-reduces contiguous ranges of the buffer in place.  A window of passes
        # ends when the parameters' .grad are reset (zero_grad): see enter_backward().  torch.autograd.grad() does not see
        # these gradients - leave the flag off for anything but .backward() training steps.
        # extra_params: the network's parameters that are NOT spectral-normalised layers (class embeddings of the conditional
        # BatchNorm layers, the attention gate ...): collect_extra() moves their autograd gradients into the tail of `flat`.
        self.direct_grads = False
        self.extra_params = list(extra_params)
        self.flat = None
        self.group_count: List[int] = []
        self.win_touched, self.win_bias = set(), set()
        self.expected_passes = 1               # passes per window after which on_group_done fires (ModelWrapper: 2 for D, 1 for G)
        self.pair: Optional["PairPass"] = None # set while the trunk of a two-group pass runs (begin_pair)
        self.on_group_done = None              # callable(start, stop): floats [start, stop) of `flat` are final (eager launches only)

    def set_groups(self, n_groups: int) -> None:
        if n_groups != self.n_groups:
            self.n_groups = n_groups
            self._key = None                       # the tables are rebuilt by the next forward

    def _alloc_flat(self, device) -> None:
        self.flat = torch.zeros(self.flat_floats, dtype=torch.float32, device=device)
        self._make_views()

    def _make_views(self) -> None:
        """The parameters' windows into `flat` for the CURRENT layout (grad_offs / bias_offs / extra_offs) and a fresh window
        of passes.  Called for a new buffer and whenever a rebuild changed the layout under a retained buffer."""
        self.w_views = [self.flat[o:o + m.weight_orig.numel()].view(m.weight_orig.shape)
                        for o, (m, _, _) in zip(self.grad_offs, self.specs)]
        self.b_views = [self.flat[o:o + m.weight_orig.shape[0]] for o, (m, _, _) in zip(self.bias_offs, self.specs)]
        self.extra_views = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(self.extra_offs, self.extra_params)]
        self.group_count = [0] * len(self.groups)
        self.win_touched, self.win_bias = set(), set()
        self._view_layout = (tuple(self.grad_offs), tuple(self.bias_offs), tuple(self.extra_offs), len(self.groups))

    def enter_backward(self, device, group: int) -> None:
        """Start of a group's batched backward (direct mode).  The window continues iff the gradients this group assigned in the
        previous pass are still in place (zero_grad(set_to_none=True) or a manual reset starts a new one)."""
        if self.flat is None or self.flat.device != device:
            self._alloc_flat(device)
        if self.group_count[group] > 0:
            lo, hi = self.groups[group]
            probe = next((i for i in range(lo, hi) if i in self.win_touched), None)
            gr = self.specs[probe][0].weight_orig.grad if probe is not None else None
            if gr is None or gr.data_ptr() != self.w_views[probe].data_ptr():
                self.group_count[group] = 0
                self.win_touched -= set(range(lo, hi))
                self.win_bias -= set(range(lo, hi))

    def collect_extra(self) -> None:
        """After .backward() (direct mode): the autograd gradients of the non-SN parameters move into their slots at the tail
        of `flat` (one multi-tensor copy) and .grad becomes the view, so that EVERY gradient of the network lives in `flat`."""
        if not self.direct_grads or self.flat is None:
            return
        # ... and so do biases of spectral-normalised layers whose gradient came through autograd instead of a kernel's bias slot
        # (the discriminator's classification head, _DHeadFn.backward: without this its gradient sat outside `flat`, i.e. outside
        # everything the data-parallel reducer all-reduces)
        pairs = list(zip(self.extra_params, self.extra_views))
        for (m, _, _), v in zip(self.specs, self.b_views):
            b = getattr(m, "bias", None)
            if b is not None:
                pairs.append((b, v))
        src, dst, moved = [], [], []
        for p, v in pairs:
            if p.grad is not None and p.grad.data_ptr() != v.data_ptr():
                src.append(p.grad.reshape(v.shape) if p.grad.is_contiguous() else p.grad.contiguous().reshape(v.shape))
                dst.append(v)
                moved.append((p, v))
        if src:
            torch._foreach_copy_(dst, src)
            for p, v in moved:
                p.grad = v

    def _build(self, dtype, device):
        e = chunk_elems(dtype)
        esz = 4 if dtype == torch.float32 else 2
        table = (L.SpSnLayer * len(self.specs))()
        scratch_off, pack_off, pack_blocks = 0, 0, 0
        max_rows = max_cols = max_pack = 1
        for i, (m, kind, need_dgrad) in enumerate(self.specs):
            w = m.weight_orig
            rows = w.shape[0]
            ent = table[i]
            if kind == "conv":
                cin, taps = w.shape[1], w.shape[2] * w.shape[3]
                cin_p, cout_p = pad_to(cin, e), pad_to(rows, e)
            elif kind == "linear":
                cin, taps = w.shape[1], 1
                cin_p, cout_p = pad_to(cin, 8), pad_to(rows, 8)
            else:
                cin, taps = w[0].numel(), 1
                cin_p, cout_p = cin, rows
            cols = cin * taps
            ent.w, ent.u, ent.v = w.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr()
            ent.rows, ent.cols, ent.cin, ent.taps, ent.cin_p, ent.cout_p = rows, cols, cin, taps, cin_p, cout_p
            ent.kind = 1 if kind == "plain" else 0
            ent.scratch_off = scratch_off
            scratch_off += pad_to(cols + 2 * rows + 4, 4)
            ent.part_off = scratch_off                    # ceil(rows/128) x cols partial sums of W^T u (summed in slab order)
            scratch_off += pad_to(((rows + 127) // 128) * cols, 4)
            fwd_bytes = rows * cols * 4 if kind == "plain" else rows * taps * cin_p * esz
            ent.fwd_off = pack_off
            pack_off += pad_to(fwd_bytes, 256)
            fwd_elems = rows * cols if kind == "plain" else rows * taps * cin_p
            dg_elems = 0
            if need_dgrad and kind != "plain":
                ent.dgrad_off = pack_off
                dg_elems = cin * taps * cout_p
                pack_off += pad_to(dg_elems * esz, 256)
            else:
                ent.dgrad_off = -1
            max_rows, max_cols = max(max_rows, rows), max(max_cols, cols)
            tiles = ((cin_p + 31) // 32) * ((cout_p + 31) // 32) if kind != "plain" else 0   # 32x32xtaps tiles of sn_pack_kernel
            max_pack = max(max_pack, fwd_elems, dg_elems, tiles * 1024)
            ent.pack_block0 = pack_blocks                 # 1-D grid of the packing kernel: this layer's first block
            pack_blocks += tiles if kind != "plain" else (rows * cols + 1023) // 1024
        self.entries = [table[i] for i in range(len(self.specs))]
        raw = bytes(table)
        self.table_dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self._table_host = table
        self.scratch_floats, self.pack_bytes = scratch_off, pack_off
        self.max_rows, self.max_cols, self.max_pack, self.pack_blocks = max_rows, max_cols, max_pack, pack_blocks
        # groups of consecutive layers with about the same number of weights each (forward order)
        n = len(self.entries)
        sizes = [ent.rows * ent.cols for ent in self.entries]
        total, k = sum(sizes), min(self.n_groups, n)
        self.groups, lo, acc = [], 0, 0
        for i in range(n):
            acc += sizes[i]
            left_groups, left_layers = k - len(self.groups) - 1, n - i - 1
            if left_groups > 0 and left_layers >= left_groups and (acc >= total * (len(self.groups) + 1) / k or left_layers == left_groups):
                self.groups.append((lo, i + 1))
                lo = i + 1
        self.groups.append((lo, n))
        # gradient arena (per pass): per layer [dW (forward packing, fp32) | dot | dbias(rows)]; flat gradient buffer (persistent
        # in direct mode): per group [d weight_orig of its layers | d bias of its layers], then the non-SN parameters
        btab = (L.SpSnBwdLayer * n)()
        arena_off, max_elems = 0, 1
        self.grad_layout = []
        for i, ent in enumerate(self.entries):
            n_dw = ent.rows * ent.cols if ent.kind == 1 else ent.rows * ent.taps * ent.cin_p
            dw_off, dot_off, db_off = arena_off, arena_off + n_dw, arena_off + n_dw + 1
            arena_off = pad_to(db_off + ent.rows, 4)
            b = btab[i]
            b.w, b.dw_off, b.dot_off, b.scratch_off = ent.w, dw_off, dot_off, ent.scratch_off
            b.rows, b.cols, b.cin, b.taps, b.cin_p, b.plain = ent.rows, ent.cols, ent.cin, ent.taps, ent.cin_p, ent.kind
            b.db_off = db_off
            self.grad_layout.append((dw_off, n_dw, db_off))
            max_elems = max(max_elems, ent.rows * ent.cols)
        flat_off = 0
        self.grad_offs, self.bias_offs, self.group_range = [0] * n, [0] * n, []
        for lo, hi in self.groups:
            g0 = flat_off
            for i in range(lo, hi):
                self.grad_offs[i] = btab[i].grad_off = flat_off
                flat_off += pad_to(self.entries[i].rows * self.entries[i].cols, 4)
            for i in range(lo, hi):
                self.bias_offs[i] = btab[i].bias_off = flat_off
                flat_off += pad_to(self.entries[i].rows, 4)
            self.group_range.append((g0, flat_off))
        self.sn_floats = flat_off
        self.extra_offs = []
        for p in self.extra_params:
            self.extra_offs.append(flat_off)
            flat_off += pad_to(p.numel(), 4)
        self.arena_floats, self.flat_floats, self.max_elems = arena_off, flat_off, max_elems
        # a rebuild (compute-dtype switch, re-allocated parameters) keeps the flat gradient buffer when its size is unchanged: captured
        # graphs, the Adam plans and the parameters' .grad views all point into it (round-2 ADVICE: a silent re-allocation would leave
        # them on the old buffer while the reducer averaged the new, empty one); a changed size drops it - model_wrapper then refuses
        # to replay graphs captured on the old one
        old_flat = getattr(self, "flat", None)
        self.flat = old_flat if (old_flat is not None and old_flat.numel() == flat_off and old_flat.device == torch.device(device)) else None
        layout = (tuple(self.grad_offs), tuple(self.bias_offs), tuple(self.extra_offs), len(self.groups))
        if self.flat is not None and getattr(self, "_view_layout", None) != layout:
            # same size, other offsets (set_groups() changed the group count: the total is a sum of padded sizes, the per-layer
            # offsets are not - round-3 ADVICE): the kernels will write at the NEW offsets, so the parameters' windows are rebuilt
            # and every gradient still viewing the old ones is dropped (its contents are stale under the new layout anyway)
            lo = self.flat.data_ptr()
            hi = lo + 4 * self.flat.numel()
            for m, _, _ in self.specs:
                for p in m.parameters(recurse=False):
                    if p.grad is not None and lo <= p.grad.data_ptr() < hi:
                        p.grad = None
            for p in self.extra_params:
                if p.grad is not None and lo <= p.grad.data_ptr() < hi:
                    p.grad = None
            self.flat.zero_()
            self._make_views()
        self.bwd_table_dev = torch.frombuffer(bytearray(bytes(btab)), dtype=torch.uint8).to(device)

    def _unpacked_table(self, skip: frozenset):
        """(device table, pack blocks) of a forward that packs every layer BUT those in `skip` (slots): the same entries with the
        skipped layers' block ranges of the packing kernel's 1-D grid made empty - their slices of the pack arena stay unwritten.
        For the second forward of a two-group pass, whose convolution trunk runs on the first forward's packing (begin_pair,
        models.Generator.forward_pair): the power iteration and the (u, v, sigma) snapshot are per forward, the packed copy is not."""
        cache = self.__dict__.setdefault("_nopack_tables", {})
        hit = cache.get(skip)
        if hit is not None and hit[2] is self._table_host:
            return hit[0], hit[1]
        n = len(self.specs)
        tab = (L.SpSnLayer * n)()
        ctypes.memmove(tab, self._table_host, ctypes.sizeof(tab))
        blocks = 0
        for i in range(n):
            ent = self.entries[i]
            width = (self.entries[i + 1].pack_block0 if i + 1 < n else self.pack_blocks) - ent.pack_block0
            tab[i].pack_block0 = blocks
            if i not in skip:
                blocks += width
        dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.table_dev.device)
        # every layer skipped: -1 = no packing launch at all (a grid of one block would be handed to the last layer, whose tile 0 it
        # would write although that layer was skipped)
        blocks = blocks if blocks > 0 else -1
        cache[skip] = (dev, blocks, self._table_host)
        return dev, blocks

    def begin(self, training: bool, dtype, device, skip_pack: Optional[frozenset] = None) -> SNCall:
        """skip_pack: slots of layers whose packed weights this forward will not be asked for (_unpacked_table)."""
        key = (dtype, str(device)) + tuple((m.weight_orig.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr())
                                           for m, _, _ in self.specs)
        if key != self._key:
            self._build(dtype, device)
            self._key = key
        drop_wgrad_reduce()                   # (no reduction of an earlier backward pass is pending here unless that pass was abandoned)
        pack = torch.empty(self.pack_bytes, dtype=torch.uint8, device=device)
        scratch = torch.empty(self.scratch_floats, dtype=torch.float32, device=device)
        table, blocks = (self.table_dev, self.pack_blocks) if not skip_pack else self._unpacked_table(skip_pack)
        L.call("sp_sn_forward", ptr(table), len(self.specs), self.max_rows, self.max_cols, self.max_pack,
               ptr(scratch), self.scratch_floats, ptr(pack), 1 if training else 0, sp_dtype(dtype), blocks, stream())
        call = self.current = SNCall(self, pack, scratch, dtype)
        weights = [m.weight_orig for m, _, _ in self.specs]
        self.handles = None
        if torch.is_grad_enabled() and any(w.requires_grad for w in weights):
            # the gradient arena is zero-filled NOW, on the stream the forward starts on: weight-gradient kernels of layers whose
            # forward ran on a side stream accumulate into it from that stream (models.Generator._map_features_ahead), and every
            # stream the forward forks waits for this one first
            call.grad_arena()
            hs = []
            for g, (lo, hi) in enumerate(self.groups):
                hs.extend(_SNBankFn.apply(call, g, *weights[lo:hi]))
            self.handles = hs
        return call

    def begin_pair(self, training: bool, dtype, device, split: int, trunk_slots: Optional[frozenset] = None) -> "PairPass":
        """Two consecutive forwards of the bank (two power iterations: the reference's D(real) then D(fake)) for ONE two-group
        pass.  Leaves forward a current (its packing serves the trunk) with `pair` set; use_call() switches between the two for
        the layers that run per group."""
        call_a = self.begin(training, dtype, device)
        handles_a = self.handles
        # trunk_slots: the layers every launch of which takes forward a's packing (+ the per-group scale) - forward b does not pack them
        call_b = self.begin(training, dtype, device, skip_pack=trunk_slots if CFG.sn_skip_pack else None)
        handles_b = self.handles
        scales = torch.empty(2 * len(self.specs), dtype=torch.float32, device=device)
        L.call("sp_sn_pair_scales", ptr(self.table_dev), len(self.specs), ptr(call_a.scratch), ptr(call_b.scratch), ptr(scales), stream())
        pair = PairPass(call_a, call_b, handles_a, handles_b, scales, split)
        self.current, self.handles, self.pair = call_a, handles_a, pair
        return pair

    def use_call(self, call: SNCall, handles, pair: Optional["PairPass"] = None) -> None:
        self.current, self.handles, self.pair = call, handles, pair

    def end(self) -> None:
        self.current = None
        self.handles = None
        self.pair = None

    def flat_ranges(self, bucket_floats: int, min_floats: int = (8 << 20) // 4):
        """Contiguous [start, stop) ranges covering the whole flat gradient buffer, the groups that finish first in a backward pass
        (the last ones in forward order) first, each cut into buckets of at most `bucket_floats`.  No collective below
        `min_floats` (8 MB: a ring all-reduce over xGMI is latency-bound below that - round-5 VERDICT, next #7b) among the layer
        groups unless the whole buffer is smaller: a short group joins the neighbour it touches in memory (the order then follows the
        later of the two), and the remainder of a cut joins the bucket in front of it; the tail of autograd-delivered gradients
        stays a (small) collective of its own at the end."""
        spans = [(a, b) for a, b in reversed(self.group_range) if b > a]
        tail = (self.sn_floats, self.flat_floats) if self.flat_floats > self.sn_floats else None
        if tail is not None and self.flat_floats < 2 * min_floats:
            spans.append(tail)                                # a small network: one or two collectives in all
            tail = None
        merged = list(spans)
        while len(merged) > 1:
            short = [i for i, (a, b) in enumerate(merged) if b - a < min_floats]
            if not short:
                break
            i = short[0]
            a, b = merged[i]
            # the neighbour in memory: the one that finishes closest in the backward order (nearest position in the list)
            cand = [j for j, (c, d) in enumerate(merged) if j != i and (d == a or c == b)]
            if not cand:
                break
            j = min(cand, key=lambda k: abs(k - i))
            c, d = merged[j]
            merged[max(i, j)] = (min(a, c), max(b, d))        # (ready only when the later of the two is)
            del merged[min(i, j)]
        if tail is not None:
            # the gradients that arrive through autograd (a few scalars and embeddings, final only after the backward pass) touch the
            # group that finishes FIRST: joined to it they would hold its reduction back to the end - they go last, on their own
            merged.append(tail)
        out = []
        for a, b in merged:
            while a < b:
                e = min(b, a + bucket_floats)
                if b - e < min_floats and b - a >= min_floats:   # (a remainder too short for a collective of its own)
                    e = b
                out.append((a, e))
                a = e
        return out


def packed_layer(module, training: bool, dtype, device) -> PackedLayer:
    """The PackedLayer of `module` for the forward in flight; a layer used on its own (unit tests, a block
    called outside its network) gets a private one-layer bank."""
    bank = getattr(module, "_sn_bank", None)
    if bank is not None and bank.current is not None and bank.current.dtype == dtype:
        return bank.current.layers[module._sn_slot]
    solo = getattr(module, "_sn_solo", None)
    if solo is None:
        saved = (getattr(module, "_sn_bank", None), getattr(module, "_sn_slot", None))
        solo = SpectralNormBank([(module, module._sn_kind, True)])
        module._sn_solo = solo
        module._sn_bank, module._sn_slot = saved
    call = solo.begin(training, dtype, device)
    solo.current = None          # not end(): the caller still reads this forward's handle; the next begin() replaces it
    return call.layers[0]


# ======================================================================================================
# convolution / linear
# ======================================================================================================
# bench.py sets this to a list to time the convolution launches with events on the launch stream (eager steps only): entries
# (start, end, algorithmic flops, family in {"fwd", "dgrad", "wgrad"}, None, route, shape, network) - the fifth slot is unused
# (bench.py tells the dominant kernel by the route the library reports)
KERNEL_PROBE = None
# which network the probed launches belong to: "sn" = the spectral-normalised layers of G and D (the north-star's "3x3 spectral-norm
# conv backward" is a sub-total over these), "vgg" while the frozen pyramid runs (models._VGGPyramidFn sets it)
PROBE_NET = ["sn"]


def _probed(family: str, flops: float, fn, shape=None) -> None:
    """flops: EXECUTED multiply-adds x 2 of the launch on the layer's real channel counts (zero-padded channels - RGB 3 -> 8,
    513 -> 520 - are not work)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    route = L.lib().sp_last_route().decode()          # the kernel the entry point chose (include/sempyr.h: sp_last_route)
    KERNEL_PROBE.append((e0, e1, flops, family, None, route, shape, PROBE_NET[0]))


TUNE_CONV_TALL, TUNE_IGEMM_DMA, TUNE_WGRAD_ROWS, TUNE_DETERMINISTIC = 0, 1, 2, 3
TUNE_CONV1X1_SPLITK, TUNE_WGRAD1X1, TUNE_CONV_CIN8, TUNE_CONV_THINCO = 17, 18, 19, 20
_POOL2_BWD_FUSED = CFG.pool2_bwd_fused     # A/B switch (profiles/README.md)


def set_tuning(key: int, value: int) -> None:
    """Kernel-selection knob of the library (include/sempyr.h: sp_set_tuning); value < 0 restores the default."""
    L.call("sp_set_tuning", key, value)
    _CONV_WS_CACHE.clear()
    _WS_CACHE.clear()
    _POOLED_WGRAD_CACHE.clear()
    _LIN_WS_CACHE.clear()


def conv_launch(x, w_ptr: int, bias, y, res1, res2, mask_src, slope: float, n, h, w, cin_p, cout, ldy, ksize, act,
                dtype, pool2: bool = False, in_up2: bool = False, family: str = "fwd", img_scale: int = 0, img_split: int = 0,
                k_real: Optional[int] = None, pool_idx: Optional[torch.Tensor] = None) -> None:
    """k_real: the layer's real reduction channels where cin_p counts zero padding (bench.py's FLOP bookkeeping only).
    pool_idx (with pool2 = 2): int32 tensor that receives the window positions of the maxima (include/sempyr.h)."""
    if KERNEL_PROBE is not None:
        _probed(family, 2.0 * n * h * w * (k_real if k_real is not None else cin_p) * cout * ksize * ksize,
                lambda: _conv_launch(x, w_ptr, bias, y, res1, res2, mask_src, slope, n, h, w, cin_p, cout, ldy, ksize, act, dtype, pool2, in_up2,
                                     img_scale, img_split, pool_idx),
                (ksize, cin_p, cout, h, w, n))
        return
    _conv_launch(x, w_ptr, bias, y, res1, res2, mask_src, slope, n, h, w, cin_p, cout, ldy, ksize, act, dtype, pool2, in_up2, img_scale, img_split,
                 pool_idx)


def conv_pool2_ok(h: int, w: int, cout: int, ksize: int) -> bool:
    """Layers whose following 2x2 average pooling can ride in the convolution's epilogue (include/sempyr.h: pool2)."""
    return ksize == 3 and cout > 32 and cout % 16 == 0 and h % 8 == 0 and w % 32 == 0


def conv_pool_idx_ok(n: int, h: int, w: int, cin_p: int, cout: int, dtype) -> bool:
    """3x3 layers whose following ReLU + MaxPool2d(2) can ride in the epilogue WITH the window positions recorded for the backward pass
    (include/sempyr.h: sp_conv_params.pool_idx; mirrors the library's admission test)."""
    esz = 4 if dtype == torch.float32 else 2
    return (conv_pool2_ok(h, w, cout, 3) and cout % 16 == 0 and n * h * w * cin_p * esz < (1 << 30) and cout * 9 * cin_p * esz < (1 << 30))


# sp_conv_params.split_sync: the zero-at-rest counters of the 3x3 kernels' K-split of their last partial round - one area per
# (device, stream), so that launches on different streams never share one (include/sempyr.h); allocated on first use (inside a graph
# capture: from the graph's pool, its zero fill captured with it)
_SPLIT_SYNC = {}


def _split_sync(device) -> torch.Tensor:
    key = (torch.device(device).index, torch.cuda.current_stream(device).cuda_stream)
    t = _SPLIT_SYNC.get(key)
    if t is None:
        t = _SPLIT_SYNC[key] = torch.zeros(L.SP_CONV_SPLIT_SYNC_BYTES // 4, dtype=torch.int32, device=device)
    return t


def _conv_launch(x, w_ptr: int, bias, y, res1, res2, mask_src, slope: float, n, h, w, cin_p, cout, ldy, ksize, act,
                 dtype, pool2: bool = False, in_up2: bool = False, img_scale: int = 0, img_split: int = 0, pool_idx=None) -> None:
    """img_scale: device ADDRESS of the two per-group accumulator scales of a two-group batch (include/sempyr.h), 0 = none."""
    p = L.SpConvParams()
    if pool_idx is not None:
        p.pool_idx = pool_idx.data_ptr()
    if img_scale:
        p.img_scale, p.img_split = img_scale, img_split
    p.x, p.w, p.bias, p.y = x.data_ptr(), w_ptr, (bias.data_ptr() if bias is not None else None), y.data_ptr()
    p.res1 = res1.data_ptr() if res1 is not None else None
    p.res2 = res2.data_ptr() if res2 is not None else None
    p.mask_src = mask_src.data_ptr() if mask_src is not None else None
    p.mask_neg_slope = slope
    p.n, p.h, p.w_, p.cin_p, p.cout, p.ldy, p.ksize, p.act, p.dtype = n, h, w, cin_p, cout, ldy, ksize, act, sp_dtype(dtype)
    p.pool2, p.in_up2 = int(pool2), (1 if in_up2 else 0)        # pool2: False/0, True/1 = average, 2 = maximum
    # small-spatial 3x3 layers (4x4 .. 16x16): lend the fp32 scratch the kernel asks for to split K across blocks; 16-bit layers on
    # the ping-pong kernel: the partial tiles of the K-split of its last, partial round of work items (csrc/conv_pp.hip).  The
    # library says which layers those are (0 bytes for every other one; cached per shape)
    ws_bytes = conv_workspace_bytes(n, h, w, cin_p, cout, ksize, dtype)
    if ws_bytes:
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws_bytes
        if dtype != torch.float32:
            p.split_sync = _split_sync(x.device).data_ptr()
    L.call("sp_conv2d_igemm", ctypes.byref(p), stream())


def act_backward(dy: torch.Tensor, y: torch.Tensor, act: int, c_pad: Optional[int] = None) -> torch.Tensor:
    """dz = dy * act'(.) from the post-activation y (NHWC or rows); optional channel re-pitch with zero padding."""
    if dy.dim() == 4:
        n, h, w, c = dims(dy)
        cp = c if c_pad is None else c_pad
        dz = nhwc_empty(n, cp, h, w, dy.dtype, dy.device)
        pixels = n * h * w
    else:
        pixels, c = dy.shape
        cp = c if c_pad is None else c_pad
        dz = torch.empty((pixels, cp), dtype=dy.dtype, device=dy.device)
    L.call("sp_act_bwd", ptr(dy), ptr(y), ptr(dz), pixels, c, cp, act, sp_dtype(dy.dtype), stream())
    return dz


_WS_CACHE = {}
_POOLED_WGRAD_CACHE = {}
_CONV_WS_CACHE = {}
_LIN_WS_CACHE = {}


def conv_workspace_bytes(n, h, w, cin_p, cout, ksize, dtype) -> int:
    key = (n, h, w, cin_p, cout, ksize, dtype)
    v = _CONV_WS_CACHE.get(key)
    if v is None:
        out = ctypes.c_int64(0)
        L.call("sp_conv2d_workspace", n, h, w, cin_p, cout, ksize, sp_dtype(dtype), ctypes.byref(out))
        v = _CONV_WS_CACHE[key] = int(out.value)
    return v


def wgrad_workspace_floats(n, h, w, cin_p, cout, ksize, dtype) -> int:
    key = (n, h, w, cin_p, cout, ksize, dtype)
    v = _WS_CACHE.get(key)
    if v is None:
        out = ctypes.c_int64(0)
        L.call("sp_conv2d_wgrad_workspace", n, h, w, cin_p, cout, ksize, sp_dtype(dtype), ctypes.byref(out))
        v = _WS_CACHE[key] = int(out.value)
    return v


def wgrad_reads_pooled(n, split, h, w, cin_p, cout, ld_dy, ksize, want_dbias: bool, ws_floats, dtype) -> bool:
    """Whether the weight gradient of a pool2 layer can read the gradient at the pooled resolution (sp_conv2d_wgrad_accum_pooled, or
    sp_conv2d_wgrad_accum_pair with dy_pooled, for split > 0): the library's route query with the very arguments of the launch, cached per
    shape.  False: the pooling's backward is written out first."""
    key = (n, split, h, w, cin_p, cout, ld_dy, ksize, want_dbias, ws_floats, dtype)
    v = _POOLED_WGRAD_CACHE.get(key)
    if v is None:
        try:
            L.wgrad_route(n, split, h, w, cin_p, cout, ld_dy, ksize, 1, want_dbias, ws_floats, sp_dtype(dtype))
            v = True
        except L.SempyrError:
            v = False
        _POOLED_WGRAD_CACHE[key] = v
    return v


_WGRAD_STREAMS = {}

# Deferred slab reductions (include/sempyr.h: sp_wgrad_reduce_defer / _flush; CFG.defer_wgrad_reduce).  The 1x1 / 8-channel streaming
# weight-gradient launches of a backward pass queue their reduce kernels - 31 launches of ~5 us per training step - and the bank's
# backward node (which runs once every layer has accumulated) flushes them in one launch.  The workspaces that hold the partial tiles
# stay alive in _DEFERRED_WS until then.
_DEFERRED_WS = []


def _launch_wgrad_deferring(launch, ws, defer_ok: bool = True) -> None:
    """Runs a weight-gradient launch with the library's reductions deferred (only around launches this module issues: a caller of the raw
    C ABI keeps immediate reductions).  defer_ok = False: a launch whose bias slot goes back to AUTOGRAD (a bank without direct
    gradients): autograd may add to it or sum it with another contribution before the bank's backward node flushes the queue, so its
    reduction runs at once (round-5 ADVICE)."""
    if not CFG.defer_wgrad_reduce or ws is None or not defer_ok:
        launch()
        return
    L.call("sp_wgrad_reduce_defer", 1)
    try:
        launch()
    except BaseException:
        drop_wgrad_reduce()                 # an abandoned pass: nothing queued may outlive its workspaces
        raise
    finally:
        L.call("sp_wgrad_reduce_defer", 0)
    if int(L.lib().sp_wgrad_reduce_pending()):
        _DEFERRED_WS.append(ws)


def flush_wgrad_reduce() -> None:
    if _DEFERRED_WS or int(L.lib().sp_wgrad_reduce_pending()):
        L.call("sp_wgrad_reduce_flush", 1, stream())
        _DEFERRED_WS.clear()


def drop_wgrad_reduce() -> None:
    """Forgets queued reductions without running them.  The queue is process-wide host state holding raw pointers (csrc/reduce_queue.hip);
    a backward pass or a graph capture that raised midway leaves entries that point into freed arenas or an abandoned capture pool, and
    the next flush would add stale slabs to whatever lives there now (round-5 ADVICE).  Called where no entry can be legitimate: at the
    start of every forward of a bank (every backward pass ends with its flush) and in the failure paths of the capture."""
    if _DEFERRED_WS or int(L.lib().sp_wgrad_reduce_pending()):
        L.call("sp_wgrad_reduce_flush", 0, stream())
        _DEFERRED_WS.clear()



def _on_wgrad_stream(launch, tensors) -> None:
    """Experiment (config.CFG.wgrad_side_stream, off by default): the weight gradient of a layer depends on nothing the rest of the
    backward pass waits for (its results are read by the batched spectral-norm backward at the very end), so it can run on a SIDE
    stream - a parallel branch of the captured graph - and fill the CUs the input-gradient launches leave idle in their last round.
    `tensors`: everything the launch reads or writes that was allocated on the current stream."""
    dev = tensors[0].device
    main = torch.cuda.current_stream(dev)
    side = _WGRAD_STREAMS.get(dev)
    if side is None:
        side = _WGRAD_STREAMS[dev] = torch.cuda.Stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        launch()
    for t in tensors:
        if t is not None:
            t.record_stream(side)


def _wgrad_aside(h: int, w: int) -> bool:
    """CFG.wgrad_side_stream: 0 = never, 1 = every layer, N > 1 = layers whose maps have at most N pixels (the small-map layers, whose
    weight-gradient and input-gradient launches each leave most CUs idle)."""
    lim = CFG.wgrad_side_stream
    return bool(lim) and (lim == 1 or h * w <= lim)


def _wgrad_launch(entry: str, pointers, ws_floats: int, ints, operands, flops: float, shape, aside: bool = False, defer_ok: bool = True) -> None:
    """One weight-gradient launch of `entry` (pointers, scratch, scratch floats, ints, stream): lends the scratch the library asked for,
    then runs it under bench.py's probe (flops, shape), on the side stream (aside; operands: the tensors it reads there) or with its slab
    reductions deferred (defer_ok: _launch_wgrad_deferring)."""
    ws = torch.empty(ws_floats, dtype=torch.float32, device=operands[0].device) if ws_floats else None

    def launch():
        L.call(entry, *pointers, ptr(ws), ws_floats, *ints, stream())
    if KERNEL_PROBE is not None:
        _probed("wgrad", flops, launch, shape)
    elif aside:
        _on_wgrad_stream(launch, [*operands, ws])
    else:
        _launch_wgrad_deferring(launch, ws, defer_ok)


def join_wgrad_stream(device) -> None:
    side = _WGRAD_STREAMS.get(device)
    if side is not None:
        torch.cuda.current_stream(device).wait_stream(side)


class PairPass:
    """Two forwards of one network whose convolution trunk runs as ONE batch of two groups (the discriminator's D(real) and
    D(fake) of a step, model_wrapper.py:153-155): images [0, split) belong to forward `a`, the rest to forward `b`, which ran one
    more power iteration.  Every launch uses a's packing W / sigma_a with the per-group accumulator scales {1, sigma_a / sigma_b}
    of its layer (sp_conv_params.img_scale); the weight gradient is taken per group - each into its own forward's arena, since the
    spectral-norm backward of a group needs that group's (u, v, sigma)."""
    __slots__ = ("call_a", "call_b", "handles_a", "handles_b", "scales", "split")

    def __init__(self, call_a, call_b, handles_a, handles_b, scales, split):
        self.call_a, self.call_b, self.handles_a, self.handles_b, self.scales, self.split = call_a, call_b, handles_a, handles_b, scales, split

    def scale_ptr(self, slot: int) -> int:
        return self.scales.data_ptr() + 8 * slot


class Dest:
    """Where an operator's forward leaves its output, handed over OUTSIDE autograd's view of the arguments: `t` is a dense slice of a
    larger buffer (one group's images of a two-group batch, models.Generator.forward_pair).  filled = False: the operator's launch
    writes into it; filled = True: a launch over the whole buffer has already produced it and the operator only builds its autograd
    node around it.  The Function returns a fresh alias of the memory (t.detach()), so autograd never sees the buffer itself."""
    __slots__ = ("t", "filled", "extra")

    def __init__(self, t: torch.Tensor, filled: bool = False, extra=None):
        self.t, self.filled, self.extra = t, filled, extra


def _dest_tensor(dest: Optional["Dest"], shape, like: torch.Tensor) -> torch.Tensor:
    if tuple(dest.t.shape) != tuple(shape) or dest.t.dtype != like.dtype or not (is_nhwc(dest.t) if dest.t.dim() == 4 else dest.t.is_contiguous()):
        raise L.SempyrError("destination slice %s %s does not fit the output %s %s" % (tuple(dest.t.shape), dest.t.dtype, tuple(shape), like.dtype))
    return dest.t.detach()


class _ConvFn(torch.autograd.Function):
    """`handle` is the layer's output of _SNBankFn: it stands for weight_orig in the autograd graph.  pair (a PairPass) with
    handle_b = the same layer's handle of the second forward: a two-group batch."""

    @staticmethod
    def forward(ctx, x, handle, bias, res1, res2, pl: PackedLayer, ksize: int, act: int, cout: int, premasked: bool = False,
                mask_input: bool = False, pool2: bool = False, handle_b=None, pair: Optional[PairPass] = None, dest: Optional[Dest] = None):
        require_gpu(x)
        ctx.premasked, ctx.mask_input, ctx.pool2 = premasked, mask_input, pool2
        ctx.pair = pair
        img_scale, img_split = (pair.scale_ptr(pl.slot), pair.split) if pair is not None else (0, 0)
        n, h, w, cin_p = dims(x)
        if cin_p != pl.cin_p:
            raise L.SempyrError("conv input has %d channels, packed weights expect %d" % (cin_p, pl.cin_p))
        if pool2 and (premasked or not conv_pool2_ok(h, w, cout, ksize)):
            raise L.SempyrError("pool2 epilogue is not available for this layer (see conv_pool2_ok)")
        # pool2: y (and res1 / res2) live at the pooled resolution - avgpool2(conv) + bias + residuals, one launch
        if dest is not None:
            y = _dest_tensor(dest, (n, cout, h // 2, w // 2) if pool2 else (n, cout, h, w), x)
        else:
            y = nhwc_empty(n, cout, h // 2, w // 2, x.dtype, x.device) if pool2 else nhwc_empty(n, cout, h, w, x.dtype, x.device)
        if dest is None or not dest.filled:
            conv_launch(x, pl.fwd, bias, y, res1, res2, None, 0.0, n, h, w, cin_p, cout, cout, ksize, act, x.dtype, pool2,
                        img_scale=img_scale, img_split=img_split, k_real=pl.cin)
        ctx.pl, ctx.ksize, ctx.act, ctx.cout = pl, ksize, act, cout
        ctx.has_res = (res1 is not None, res2 is not None)
        ctx.save_for_backward(x, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        pl, ksize, act, cout = ctx.pl, ctx.ksize, ctx.act, ctx.cout
        dt = x.dtype
        dy = as_nhwc(dy, dt)
        n, h, w, cin_p = dims(x)
        cout_p = pad_channels(cout, dt)
        if ctx.premasked and cout_p == cout:
            dz = dy             # the consumer's input-gradient epilogue already applied act'(y) (mask_input)
        elif act != ACT_NONE or cout_p != cout:
            dz = act_backward(dy, y if y is not None else dy, act, cout_p)
        else:
            dz = dy
        dres = dz if cout_p == cout else None
        need = ctx.needs_input_grad
        ws_floats = wgrad_workspace_floats(n, h, w, cin_p, cout, ksize, dt) if need[1] else 0
        # gradient of the fused average pooling: every pooled gradient spreads (x 1/4) over its 2x2 window.  The input- and
        # weight-gradient kernels read the pooled tensor through that expansion (in_up2 / sp_conv2d_wgrad_accum_pooled) where
        # they can; otherwise it is written out first.
        up2 = ctx.pool2 and _POOL2_BWD_FUSED and is_16bit(dt) and (not need[0] or conv_pool2_ok(h, w, pl.cin, ksize)) \
            and (not need[1] or wgrad_reads_pooled(n, ctx.pair.split if ctx.pair is not None else 0, h, w, cin_p, cout, cout_p, ksize, bool(need[2]),
                                                   ws_floats, dt))
        if ctx.pool2 and not up2:
            dz_full = nhwc_empty(n, cout_p, h, w, dt, x.device)
            L.call("sp_avgpool2_bwd", ptr(dz), ptr(dz_full), n, h, w, cout_p, sp_dtype(dt), stream())
            dz = dz_full
        dx = dh = db = None
        if need[0]:
            if not pl.dgrad:
                raise L.SempyrError("input gradient requested from a layer packed without dgrad weights")
            # the dgrad packing has pl.cin rows; padded input channels (if any) receive an exact zero gradient
            dx = (nhwc_empty if pl.cin == cin_p else nhwc_zeros)(n, cin_p, h, w, dt, x.device)
            # mask_input: x is the LeakyReLU output of a `premasked` producer - multiply dx by lrelu'(x) in the epilogue
            pair = ctx.pair
            conv_launch(dz, pl.dgrad, None, dx, None, None, x if ctx.mask_input else None, 0.2, n, h, w, pl.cout_p, pl.cin, cin_p,
                        ksize, ACT_NONE, dt, in_up2=up2, family="dgrad", img_scale=pair.scale_ptr(pl.slot) if pair is not None else 0,
                        img_split=pair.split if pair is not None else 0, k_real=cout)
        dhb = None
        if need[1] and ctx.pair is not None:
            # two-group batch: one weight-gradient launch per group (contiguous image ranges of x and dz), each into the arena of
            # ITS forward - the batched spectral-norm backward of a forward needs that forward's (u, v, sigma)
            pair = ctx.pair
            if not pair.call_a.bank.direct_grads:
                raise L.SempyrError("a two-group pass needs the bank's direct gradients (ModelWrapper sets them up)")
            pa, pb = pair.call_a.layers[pl.slot], pair.call_b.layers[pl.slot]
            dwa, dwb = pair.call_a.dw_slot(pa), pair.call_b.dw_slot(pb)
            dba = pair.call_a.db_slot(pa) if need[2] else None
            dbb = pair.call_b.db_slot(pb) if need[2] else None
            # ONE launch over both groups where the row walker takes the layer (half the partial-tile traffic), else the two
            # groups one after the other - decided inside the library (include/sempyr.h: sp_conv2d_wgrad_accum_pair)
            _wgrad_launch("sp_conv2d_wgrad_accum_pair", (ptr(x), ptr(dz), ptr(dwa), ptr(dba), ptr(dwb), ptr(dbb)), ws_floats,
                          (n, pair.split, h, w, cin_p, cout, cout_p, ksize, 1 if up2 else 0, sp_dtype(dt)), (x, dz),
                          2.0 * n * h * w * pl.cin * cout * ksize * ksize, (ksize, cin_p, cout, h, w, n), aside=_wgrad_aside(h, w))
            dh = dhb = _zero1(x.device)
        elif need[1]:
            # weight (+ bias) gradient accumulate into this layer's slots of the pass-wide arena; the spectral-norm
            # backward of all layers runs later, batched, in _SNBankFn.backward
            dwsn = pl.call.dw_slot(pl)
            if need[2]:
                db = pl.call.db_slot(pl)
            direct_bias = db is not None and pl.call.bank.direct_grads
            _wgrad_launch("sp_conv2d_wgrad_accum_pooled" if up2 else "sp_conv2d_wgrad_accum", (ptr(x), ptr(dz), ptr(dwsn), ptr(db)), ws_floats,
                          (n, h, w, cin_p, cout, cout_p, ksize, sp_dtype(dt)), (x, dz), 2.0 * n * h * w * pl.cin * cout * ksize * ksize,
                          (ksize, cin_p, cout, h, w, n), aside=_wgrad_aside(h, w) and pl.call.bank.direct_grads,
                          defer_ok=db is None or pl.call.bank.direct_grads)
            dh = _zero1(x.device)
            if direct_bias:
                db = None                # accumulated in the bank's persistent slot; _SNBankFn.backward assigns bias.grad
        elif need[2]:
            db = torch.empty(cout, dtype=torch.float32, device=x.device)
            pooled = 4 if up2 else 1      # the bias gradient is the plain sum of the pooled gradient (4 x 1/4)
            part = torch.empty(512 * cout, dtype=torch.float32, device=x.device)
            L.call("sp_channel_sum", ptr(dz), cout_p, n * h * w // pooled, cout, ptr(db), ptr(part), sp_dtype(dt), stream())
        if (ctx.has_res[0] and need[3]) or (ctx.has_res[1] and need[4]):
            if dres is None:
                raise L.SempyrError("residual gradient with padded channels is not supported")
        return (dx, dh, db, dres if ctx.has_res[0] and need[3] else None, dres if ctx.has_res[1] and need[4] else None,
                None, None, None, None, None, None, None, dhb, None, None)


def sn_conv2d(x, module, ksize: int, act: int = ACT_NONE, res1=None, res2=None, premasked: bool = False, mask_input: bool = False,
              pool2: bool = False, dest: Optional[Dest] = None):
    """Spectral-normalised conv (weight_orig/sigma) + bias (+res1 +res2) -> act, one fused launch.
    premasked / mask_input fuse the LeakyReLU backward of a conv -> LeakyReLU -> conv pair into the second conv's
    input-gradient epilogue: the producer (act = LReLU, premasked=True) skips its own act'(y) pass because its ONLY
    consumer (mask_input=True) returns dL/dy already multiplied by lrelu'(y)."""
    pl = packed_layer(module, module.training, x.dtype, x.device)
    if premasked and (act != ACT_LRELU or pad_channels(module.weight_orig.shape[0], x.dtype) != module.weight_orig.shape[0]):
        raise L.SempyrError("premasked needs a LeakyReLU epilogue and an unpadded channel count")
    bank = getattr(module, "_sn_bank", None)
    pair = bank.pair if bank is not None and bank.current is pl.call else None
    if pair is not None:
        hb = pair.handles_b[pl.slot] if pair.handles_b is not None else None
        return _ConvFn.apply(x, pl.handle, module.bias, res1, res2, pl, ksize, act, module.weight_orig.shape[0], premasked, mask_input,
                             pool2, hb, pair, dest)
    return _ConvFn.apply(x, pl.handle, module.bias, res1, res2, pl, ksize, act, module.weight_orig.shape[0], premasked, mask_input,
                         pool2, None, None, dest)


def conv_two_groups(x_all: torch.Tensor, module, pl: PackedLayer, scale_ptr: int, split: int, act: int = ACT_NONE, res1=None, res2=None) -> torch.Tensor:
    """The forward launch of a spectral-normalised convolution over a batch of TWO groups that belong to two forwards of the network
    (other sigma: per-group accumulator scales, sp_conv_params.img_scale), WITHOUT autograd: models.Generator.forward_pair builds the
    first group's autograd node around its slice of the result (sn_conv2d(..., dest=Dest(y[:split], filled=True)))."""
    with torch.no_grad():
        require_gpu(x_all)
        n, h, w, cin_p = dims(x_all)
        if cin_p != pl.cin_p:
            raise L.SempyrError("conv input has %d channels, packed weights expect %d" % (cin_p, pl.cin_p))
        cout, ksize = module.weight_orig.shape[0], module.kernel_size
        y = nhwc_empty(n, cout, h, w, x_all.dtype, x_all.device)
        conv_launch(x_all, pl.fwd, module.bias, y, res1, res2, None, 0.0, n, h, w, cin_p, cout, cout, ksize, act, x_all.dtype,
                    img_scale=scale_ptr, img_split=split, k_real=pl.cin)
    return y


def conv_tail_ok(x: torch.Tensor, m3, m1, with_grad: bool = False) -> bool:
    """True if conv3x3(m3) -> act -> conv1x1(m1) -> act can run as ONE launch with the 1x1 layer in the 3x3's epilogue
    (include/sempyr.h: sp_conv_params.tail_w).  with_grad = False: a forward pass without autograd (the 64-channel tensor is never
    written); True: the pass with autograd, where the launch also stores the 64-channel tensor the backward pass reads
    (config.CFG.fuse_tail_grad)."""
    n, h, w, c = dims(x)
    if with_grad != torch.is_grad_enabled() or (with_grad and not CFG.fuse_tail_grad):
        return False
    return (CFG.fuse_tail and is_16bit(x.dtype) and m3.kernel_size == 3 and m1.kernel_size == 1
            and m3.out_channels == 64 and m1.in_channels == 64 and m1.out_channels <= 4 and h % 16 == 0 and w % 32 == 0)


def sn_conv2d_tail(x, m3, act3: int, m1, act1: int, keep_mid: bool = False):
    """act1(conv1x1(act3(conv3x3(x)))) of two spectral-normalised layers in one launch (no autograd of its own; conv_tail_ok): the
    generator's last two layers (models.py:55-61).  keep_mid = False: the 64-channel intermediate is neither written nor read back;
    True: it is stored as well and (intermediate, output) is returned - the caller builds the two layers' autograd nodes around them
    (Dest(..., filled=True)), so that the pass WITH gradient saves the 1x1 layer's launch and its read of the 168 MB tensor."""
    require_gpu(x)
    x = x.detach()
    pl3 = packed_layer(m3, m3.training, x.dtype, x.device)
    pl1 = packed_layer(m1, m1.training, x.dtype, x.device)
    n, h, w, cin_p = dims(x)
    cout1 = m1.out_channels
    y = nhwc_empty(n, cout1, h, w, x.dtype, x.device)
    mid = nhwc_empty(n, 64, h, w, x.dtype, x.device) if keep_mid else None
    p = L.SpConvParams()
    p.x, p.w, p.bias, p.y = x.data_ptr(), pl3.fwd, (m3.bias.data_ptr() if m3.bias is not None else None), (mid.data_ptr() if keep_mid else None)
    p.n, p.h, p.w_, p.cin_p, p.cout, p.ldy, p.ksize, p.act, p.dtype = n, h, w, cin_p, 64, 64, 3, act3, sp_dtype(x.dtype)
    p.tail_w, p.tail_bias, p.tail_y = pl1.fwd, (m1.bias.data_ptr() if m1.bias is not None else None), y.data_ptr()
    p.tail_cout, p.tail_act, p.tail_ld = cout1, act1, cout1

    def launch():
        L.call("sp_conv2d_igemm", ctypes.byref(p), stream())
    if KERNEL_PROBE is not None:
        _probed("fwd", 2.0 * n * h * w * 64 * (9 * pl3.cin + cout1), launch, (3, cin_p, 64, h, w, n))
    else:
        launch()
    return (mid, y) if keep_mid else y


class _ReusedLayerFn(torch.autograd.Function):
    """The output of a spectral-normalised conv3x3 / linear layer for the forward in flight, derived from the SAME layer's output
    of an earlier forward on the same input and the same weight_orig (sp_rescale_bias: only sigma has moved on).  The backward is
    the layer's own - weight and bias gradients from the saved input into the current forward's arena; the input needs none."""

    @staticmethod
    def forward(ctx, handle, bias, x_saved, y_prev, pl_prev: PackedLayer, pl: PackedLayer, ksize: int, cout: int, dest: Optional[Dest] = None):
        require_gpu(y_prev)
        sig_prev = ctypes.c_void_p(pl_prev.scratch + 4 * (pl_prev.cols + 2 * pl_prev.rows))
        sig_now = ctypes.c_void_p(pl.scratch + 4 * (pl.cols + 2 * pl.rows))
        y = _dest_tensor(dest, y_prev.shape, y_prev) if dest is not None else torch.empty_like(y_prev)
        if y_prev.dim() == 4:
            n, h, w, c = dims(y_prev)
            rows, ld = n * h * w, c
        else:
            rows, c = y_prev.shape
            ld = y_prev.stride(0)
        L.call("sp_rescale_bias", ptr(y_prev), ptr(y), rows, c, ld, y.stride(0) if y.dim() == 2 else c, ptr(bias), sig_prev, sig_now,
               sp_dtype(y_prev.dtype), stream())
        ctx.pl, ctx.ksize, ctx.cout, ctx.keep = pl, ksize, cout, pl_prev.keep
        ctx.save_for_backward(x_saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        pl, ksize, cout = ctx.pl, ctx.ksize, ctx.cout
        need = ctx.needs_input_grad
        dt = x.dtype
        if not need[0]:
            return (None,) * 9
        dwsn = pl.call.dw_slot(pl)
        db = pl.call.db_slot(pl) if need[1] else None
        if x.dim() == 4:
            dy = as_nhwc(dy, dt)
            n, h, w, cin_p = dims(x)
            cout_p = pad_channels(cout, dt)
            if cout_p != cout:
                raise L.SempyrError("a reused layer needs an unpadded channel count")
            _wgrad_launch("sp_conv2d_wgrad_accum", (ptr(x), ptr(dy), ptr(dwsn), ptr(db)), wgrad_workspace_floats(n, h, w, cin_p, cout, ksize, dt),
                          (n, h, w, cin_p, cout, cout_p, ksize, sp_dtype(dt)), (x, dy), 2.0 * n * h * w * pl.cin * cout * ksize * ksize,
                          (ksize, cin_p, cout, h, w, n), defer_ok=db is None or pl.call.bank.direct_grads)
        else:
            dy = as_rows(dy, dt)
            b, k = x.shape
            if db is None:
                db = torch.empty(pl.rows, dtype=torch.float32, device=x.device)
            L.call("sp_linear_wgrad", ptr(x), x.stride(0), ptr(dy), dy.stride(0), ptr(dwsn), pl.cin_p, ptr(db), b, k, pl.rows, sp_dtype(dt), stream())
        direct = pl.call.bank.direct_grads
        return _zero1(x.device), (None if (direct or not need[1]) else db), None, None, None, None, None, None, None


def reused_layer(module, x_saved, y_prev, pl_prev: PackedLayer, dest: Optional[Dest] = None):
    """`module` applied to `x_saved` in the forward in flight, computed from its output `y_prev` of the earlier forward whose
    PackedLayer is pl_prev (see _ReusedLayerFn)."""
    pl = packed_layer(module, module.training, y_prev.dtype, y_prev.device)
    ksize = getattr(module, "kernel_size", 1)
    return _ReusedLayerFn.apply(pl.handle, module.bias, x_saved, y_prev, pl_prev, pl, ksize, module.weight_orig.shape[0], dest)


def linear_launch(x, w_ptr: int, kp: int, bias, res, y, b: int, k: int, n: int, act: int) -> None:
    """y[b][n] = act(x W^T + bias + res); large bf16 matrices go through the MFMA split-K path (fp32 scratch)."""
    scratch = None
    if is_16bit(x.dtype) and b <= 64:
        key = (b, k, n)
        floats = _LIN_WS_CACHE.get(key)
        if floats is None:
            out = ctypes.c_int64(0)
            L.call("sp_linear_workspace", b, k, n, sp_dtype(x.dtype), ctypes.byref(out))
            floats = _LIN_WS_CACHE[key] = int(out.value)
        if floats:
            scratch = torch.empty(floats, dtype=torch.float32, device=x.device)
    L.call("sp_linear_fwd_ws", ptr(x), x.stride(0), ctypes.c_void_p(w_ptr), kp, ptr(bias), ptr(res), ptr(y), y.stride(0), b, k, n, act,
           sp_dtype(x.dtype), ptr(scratch), stream())


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, handle, bias, res, pl: PackedLayer, act: int):
        require_gpu(x)
        b, k = x.shape
        n = pl.rows
        y = torch.empty((b, n), dtype=x.dtype, device=x.device)
        linear_launch(x, pl.fwd, pl.cin_p, bias, res, y, b, k, n, act)
        ctx.pl, ctx.act, ctx.has_res = pl, act, res is not None
        ctx.save_for_backward(x, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        pl, act = ctx.pl, ctx.act
        dt = x.dtype
        dy = as_rows(dy, dt)
        b, k = x.shape
        n = pl.rows
        dz = act_backward(dy, y, act) if act != ACT_NONE else dy
        need = ctx.needs_input_grad
        dx = dh = db = None
        if need[0]:
            dx = torch.empty((b, k), dtype=dt, device=x.device)
            linear_launch(dz, pl.dgrad, pl.cout_p, None, None, dx, b, n, k, ACT_NONE)
        if need[1] or need[2]:
            if need[1]:
                dwsn, db = pl.call.dw_slot(pl), pl.call.db_slot(pl)
                dh = _zero1(x.device)
            else:
                dwsn = torch.empty(n * pl.cin_p, dtype=torch.float32, device=x.device)
                db = torch.empty(n, dtype=torch.float32, device=x.device)
            L.call("sp_linear_wgrad", ptr(x), x.stride(0), ptr(dz), dz.stride(0), ptr(dwsn), pl.cin_p, ptr(db), b, k, n,
                   sp_dtype(dt), stream())
            if not need[2] or (need[1] and pl.call.bank.direct_grads):
                db = None                # direct mode: _SNBankFn.backward moves the arena slot into bias.grad
        return dx, dh, db, (dz if ctx.has_res and need[3] else None), None, None


def sn_linear(x, module, act: int = ACT_NONE, res=None):
    pl = packed_layer(module, module.training, x.dtype, x.device)
    return _LinearFn.apply(x, pl.handle, module.bias, res, pl, act)


# ======================================================================================================
# normalisation
# ======================================================================================================
class _BatchNormFn(torch.autograd.Function):
    """x -> act(scale * xhat + bias); (scale,bias) from (gamma,beta) or from emb[cls] (conditional)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, emb, cls, running_mean, running_var, momentum, eps, training, act, upsample=False, dest: Optional[Dest] = None):
        """upsample: False; True = CBN -> act -> bilinear x2 in one pass (sp_bn_apply_upsample2); "before" = the normalised tensor
        is the bilinear x2 expansion of x, never materialised (sp_bn_*_up2: the generator's final block)."""
        require_gpu(x)
        n, h, w, c = dims(x)
        dev = x.device
        if dest is not None and dest.filled:
            # a launch set over a two-group batch has already produced this group's output and statistics (sp_bn_stats_pair /
            # sp_bn_apply_pair, models._GeneratorPair.batch_norm): only the autograd node is built here
            if upsample == "before" or dest.extra is None:
                raise L.SempyrError("batch_norm: a filled destination needs its (mean, invstd) and the plain or the up-sampling form")
            mean, invstd = dest.extra
            y = _dest_tensor(dest, (n, c, 2 * h, 2 * w) if upsample else (n, c, h, w), x)
            ctx.act, ctx.training, ctx.upsample = act, training, upsample
            ctx.save_for_backward(x, gamma, beta, emb, cls, mean, invstd)
            return y
        sums = torch.empty(1024 * 2 * c, dtype=torch.float32, device=dev)        # per-block partial sums
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty(c, dtype=torch.float32, device=dev)
        if upsample == "before":
            if training:
                L.call("sp_bn_stats_up2", ptr(x), n, h, w, c, ptr(sums), eps, momentum, ptr(running_mean), ptr(running_var), ptr(mean),
                       ptr(invstd), sp_dtype(x.dtype), stream())
            else:
                L.call("sp_bn_stats", ptr(x), n, 4 * h * w, c, ptr(sums), eps, momentum, ptr(running_mean), ptr(running_var), 0, ptr(mean),
                       ptr(invstd), sp_dtype(x.dtype), stream())          # eval: from the running statistics, x is not read
            y = nhwc_empty(n, c, 2 * h, 2 * w, x.dtype, dev)
            L.call("sp_bn_apply_up2", ptr(x), ptr(y), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(emb), ptr(cls), act,
                   sp_dtype(x.dtype), stream())
            ctx.act, ctx.training, ctx.upsample = act, training, upsample
            ctx.save_for_backward(x, gamma, beta, emb, cls, mean, invstd)
            return y
        L.call("sp_bn_stats", ptr(x), n, h * w, c, ptr(sums), eps, momentum, ptr(running_mean), ptr(running_var),
               1 if training else 0, ptr(mean), ptr(invstd), sp_dtype(x.dtype), stream())
        if upsample:
            # the bilinear x2 upsampling that follows rides in the apply pass (include/sempyr.h: sp_bn_apply_upsample2)
            y = nhwc_empty(n, c, 2 * h, 2 * w, x.dtype, dev)
            L.call("sp_bn_apply_upsample2", ptr(x), ptr(y), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(emb),
                   ptr(cls), act, sp_dtype(x.dtype), stream())
        else:
            y = _dest_tensor(dest, (n, c, h, w), x) if dest is not None else nhwc_empty(n, c, h, w, x.dtype, dev)
            L.call("sp_bn_apply", ptr(x), ptr(y), n, h * w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(emb), ptr(cls), act,
                   sp_dtype(x.dtype), stream())
        ctx.act, ctx.training, ctx.upsample = act, training, upsample
        ctx.save_for_backward(x, gamma, beta, emb, cls, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, emb, cls, mean, invstd = ctx.saved_tensors
        if not ctx.training:
            raise L.SempyrError("backward through eval-mode BatchNorm is not part of the training path")
        n, h, w, c = dims(x)
        dev, dt = x.device, x.dtype
        dy = as_nhwc(dy, dt)
        if ctx.upsample == "before":
            du = nhwc_empty(n, c, 2 * h, 2 * w, dt, dev)
            red = torch.empty(1024 * 2 * c, dtype=torch.float32, device=dev)
            ctmp = torch.empty(2 * c, dtype=torch.float32, device=dev)
            dgamma = dbeta = demb = None
            classes = 0
            if emb is not None:
                demb = torch.empty_like(emb)
                classes = emb.shape[0]
            else:
                dgamma = torch.empty(c, dtype=torch.float32, device=dev)
                dbeta = torch.empty(c, dtype=torch.float32, device=dev)
            L.call("sp_bn_backward_up2", ptr(dy), ptr(x), ptr(du), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(emb),
                   ptr(cls), ctx.act, ptr(red), ptr(ctmp), ptr(dgamma), ptr(dbeta), ptr(demb), classes, sp_dtype(dt), stream())
            dx = nhwc_empty(n, c, h, w, dt, dev)
            L.call("sp_upsample2_bwd", ptr(du), ptr(dx), n, h, w, c, sp_dtype(dt), stream())
            return dx, dgamma, dbeta, demb, None, None, None, None, None, None, None, None, None
        if ctx.upsample:
            dlow = nhwc_empty(n, c, h, w, dt, dev)
            L.call("sp_upsample2_bwd", ptr(dy), ptr(dlow), n, h, w, c, sp_dtype(dt), stream())
            dy = dlow
        dx = nhwc_empty(n, c, h, w, dt, dev)
        red = torch.empty(1024 * 2 * c, dtype=torch.float32, device=dev)         # per-(sample, block) partial sums
        ctmp = torch.empty(2 * c, dtype=torch.float32, device=dev)
        dgamma = dbeta = demb = None
        classes = 0
        if emb is not None:
            demb = torch.empty_like(emb)
            classes = emb.shape[0]
        else:
            dgamma = torch.empty(c, dtype=torch.float32, device=dev)
            dbeta = torch.empty(c, dtype=torch.float32, device=dev)
        L.call("sp_bn_backward", ptr(dy), ptr(x), ptr(dx), n, h * w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(emb),
               ptr(cls), ctx.act, ptr(red), ptr(ctmp), ptr(dgamma), ptr(dbeta), ptr(demb), classes, sp_dtype(dt), stream())
        return dx, dgamma, dbeta, demb, None, None, None, None, None, None, None, None, None


def batch_norm(x, gamma, beta, emb, cls, running_mean, running_var, momentum, eps, training, act, upsample=False, dest: Optional[Dest] = None):
    if dest is not None and upsample and not dest.filled:
        raise L.SempyrError("batch_norm: an unfilled destination slice goes with the plain (not up-sampling) form")
    return _BatchNormFn.apply(x, gamma, beta, emb, cls, running_mean, running_var, momentum, eps, training, act, upsample, dest)


# ======================================================================================================
# resampling
# ======================================================================================================
class _Upsample2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest: Optional[Dest] = None):
        require_gpu(x)
        n, h, w, c = dims(x)
        y = _dest_tensor(dest, (n, c, 2 * h, 2 * w), x) if dest is not None else nhwc_empty(n, c, 2 * h, 2 * w, x.dtype, x.device)
        if dest is None or not dest.filled:
            L.call("sp_upsample2_fwd", ptr(x), ptr(y), n, h, w, c, sp_dtype(x.dtype), stream())
        ctx.shape = (n, h, w, c)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, h, w, c = ctx.shape
        dy = as_nhwc(dy)
        dx = nhwc_empty(n, c, h, w, dy.dtype, dy.device)
        L.call("sp_upsample2_bwd", ptr(dy), ptr(dx), n, h, w, c, sp_dtype(dy.dtype), stream())
        return dx, None


def upsample2(x, dest: Optional[Dest] = None):
    return _Upsample2Fn.apply(x, dest)


class _AvgPool2Fn(torch.autograd.Function):
    """Returns (pooled, act(pooled)) when act != NONE - the discriminator needs both (models.py:459-462)."""

    @staticmethod
    def forward(ctx, x, act):
        require_gpu(x)
        n, h, w, c = dims(x)
        y = nhwc_empty(n, c, h // 2, w // 2, x.dtype, x.device)
        y2 = nhwc_empty(n, c, h // 2, w // 2, x.dtype, x.device) if act != ACT_NONE else None
        L.call("sp_avgpool2_fwd", ptr(x), ptr(y), ptr(y2), act, n, h, w, c, sp_dtype(x.dtype), stream())
        ctx.shape, ctx.act = (n, h, w, c), act
        if act == ACT_NONE:
            return y
        ctx.save_for_backward(y2)
        return y, y2

    @staticmethod
    def backward(ctx, dy, dy2=None):
        n, h, w, c = ctx.shape
        g = None
        if dy is not None:
            g = as_nhwc(dy)
        if ctx.act != ACT_NONE and dy2 is not None:
            (y2,) = ctx.saved_tensors
            g2 = act_backward(as_nhwc(dy2), y2, ctx.act)
            g = g2 if g is None else g + g2
        dx = nhwc_empty(n, c, h, w, g.dtype, g.device)
        L.call("sp_avgpool2_bwd", ptr(g), ptr(dx), n, h, w, c, sp_dtype(g.dtype), stream())
        return dx, None


def avgpool2(x, act: int = ACT_NONE):
    return _AvgPool2Fn.apply(x, act)


class _ActAvgPool2Fn(torch.autograd.Function):
    """(act(x), avgpool2(x)) in one pass; one backward kernel instead of act'/pool'/sum (include/sempyr.h: sp_act_avgpool2_*)."""

    @staticmethod
    def forward(ctx, x, act):
        require_gpu(x)
        n, h, w, c = dims(x)
        ya = nhwc_empty(n, c, h, w, x.dtype, x.device)
        yp = nhwc_empty(n, c, h // 2, w // 2, x.dtype, x.device)
        L.call("sp_act_avgpool2_fwd", ptr(x), ptr(ya), ptr(yp), act, n, h, w, c, sp_dtype(x.dtype), stream())
        ctx.act = act
        ctx.save_for_backward(x)
        return ya, yp

    @staticmethod
    def backward(ctx, ga, gp):
        (x,) = ctx.saved_tensors
        n, h, w, c = dims(x)
        if ga is None and gp is None:
            return None, None
        ga = as_nhwc(ga, x.dtype) if ga is not None else None
        gp = as_nhwc(gp, x.dtype) if gp is not None else None
        dx = nhwc_empty(n, c, h, w, x.dtype, x.device)
        L.call("sp_act_avgpool2_bwd", ptr(ga), ptr(gp), ptr(x), ptr(dx), ctx.act, n, h, w, c, sp_dtype(x.dtype), stream())
        return dx, None


def act_avgpool2(x, act: int):
    return _ActAvgPool2Fn.apply(x, act)


class _MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest: Optional[Dest] = None):
        require_gpu(x)
        n, h, w, c = dims(x)
        y = _dest_tensor(dest, (n, c, h // 2, w // 2), x) if dest is not None else nhwc_empty(n, c, h // 2, w // 2, x.dtype, x.device)
        if dest is None or not dest.filled:
            L.call("sp_maxpool2_fwd", ptr(x), ptr(y), n, h, w, c, 0, sp_dtype(x.dtype), stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, h, w, c = dims(x)
        dy = as_nhwc(dy, x.dtype)
        dx = nhwc_empty(n, c, h, w, x.dtype, x.device)
        L.call("sp_maxpool2_bwd", ptr(dy), ptr(x), ptr(dx), n, h, w, c, 0, sp_dtype(x.dtype), stream())
        return dx, None


def maxpool2(x, dest: Optional[Dest] = None):
    return _MaxPool2Fn.apply(x, dest)


class _AdaptiveAvgFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow, act_in):
        require_gpu(x)
        n, h, w, c = dims(x)
        y = nhwc_empty(n, c, oh, ow, x.dtype, x.device)
        L.call("sp_adaptive_avgpool_fwd", ptr(x), ptr(y), n, h, w, c, oh, ow, act_in, sp_dtype(x.dtype), stream())
        ctx.cfg = (oh, ow, act_in)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        oh, ow, act_in = ctx.cfg
        n, h, w, c = dims(x)
        dy = as_nhwc(dy, x.dtype)
        dx = nhwc_empty(n, c, h, w, x.dtype, x.device)
        L.call("sp_adaptive_avgpool_bwd", ptr(dy), ptr(x), ptr(dx), n, h, w, c, oh, ow, act_in, sp_dtype(x.dtype), stream())
        return dx, None, None, None


def adaptive_avgpool(x, oh: int, ow: int, act_in: int = ACT_NONE):
    return _AdaptiveAvgFn.apply(x, oh, ow, act_in)


# ======================================================================================================
# elementwise
# ======================================================================================================
class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        require_gpu(x)
        y = torch.empty_like(x)      # preserves the NHWC strides
        L.call("sp_act_fwd", ptr(x), ptr(y), x.numel(), act, sp_dtype(x.dtype), stream())
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = as_nhwc(dy, y.dtype) if y.dim() == 4 else as_rows(dy, y.dtype)
        return act_backward(dy, y, ctx.act), None


def activation(x, act: int):
    return _ActFn.apply(x, act)


class _ScaleAddFn(torch.autograd.Function):
    """y = gamma * a + b   (models.py:274)."""

    @staticmethod
    def forward(ctx, a, b, gamma, dest: Optional[Dest] = None):
        require_gpu(a)
        y = _dest_tensor(dest, a.shape, a) if dest is not None else torch.empty_like(a)
        if dest is None or not dest.filled:
            L.call("sp_scale_add", ptr(a), ptr(b), ptr(gamma), ptr(y), a.numel(), sp_dtype(a.dtype), stream())
        ctx.save_for_backward(a, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, gamma = ctx.saved_tensors
        dy = as_nhwc(dy, a.dtype)
        da = torch.empty_like(a)
        dg = torch.empty(1, dtype=torch.float32, device=a.device)
        part = torch.empty(512, dtype=torch.float32, device=a.device)
        L.call("sp_scale_add_bwd", ptr(dy), ptr(a), ptr(gamma), ptr(da), ptr(dg), ptr(part), a.numel(), sp_dtype(a.dtype), stream())
        return da, dy, dg, None


class _SplitRowsFn(torch.autograd.Function):
    """(B, K) rows -> rows [0, split) and [split, B) as two dense tensors (and back), through the library's copy pass - no
    torch slicing / cat kernels in the autograd graph."""

    @staticmethod
    def forward(ctx, x, split):
        require_gpu(x)
        x = as_rows(x)
        b, k = x.shape
        esz = x.element_size()
        ya = torch.empty((split, k), dtype=x.dtype, device=x.device)
        yb = torch.empty((b - split, k), dtype=x.dtype, device=x.device)
        L.call("sp_act_fwd", ptr(x), ptr(ya), split * k, ACT_NONE, sp_dtype(x.dtype), stream())
        L.call("sp_act_fwd", ctypes.c_void_p(x.data_ptr() + split * k * esz), ptr(yb), (b - split) * k, ACT_NONE, sp_dtype(x.dtype), stream())
        ctx.cfg = (b, k, split)
        return ya, yb

    @staticmethod
    def backward(ctx, ga, gb):
        b, k, split = ctx.cfg
        ref = ga if ga is not None else gb
        dx = torch.empty((b, k), dtype=ref.dtype, device=ref.device)
        esz = dx.element_size()
        for g, lo, rows in ((ga, 0, split), (gb, split, b - split)):
            dst = ctypes.c_void_p(dx.data_ptr() + lo * k * esz)
            if g is None:
                dx.narrow(0, lo, rows).zero_()
            else:
                L.call("sp_act_fwd", ptr(as_rows(g, dx.dtype)), dst, rows * k, ACT_NONE, sp_dtype(dx.dtype), stream())
        return dx, None


def split_rows(x, split: int):
    return _SplitRowsFn.apply(x, split)


def scale_add(a, b, gamma, dest: Optional[Dest] = None):
    return _ScaleAddFn.apply(a, b, gamma, dest)


class _PermuteFn(torch.autograd.Function):
    """(B, C*HW) in NCHW-flatten order -> NHWC tensor (B, C, H, W) (models.py:83), or back."""

    @staticmethod
    def forward(ctx, x, c, h, w, to_nhwc, dest: Optional[Dest] = None):
        require_gpu(x)
        b = x.shape[0]
        if to_nhwc and dest is not None:
            y = _dest_tensor(dest, (b, c, h, w), x)
        elif to_nhwc:
            y = nhwc_empty(b, c, h, w, x.dtype, x.device)
        else:
            y = torch.empty((b, c * h * w), dtype=x.dtype, device=x.device)
        L.call("sp_permute_chw_hwc", ptr(x), ptr(y), b, c, h * w, 1 if to_nhwc else 0, sp_dtype(x.dtype), stream())
        ctx.cfg = (b, c, h, w, to_nhwc)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, c, h, w, to_nhwc = ctx.cfg
        if to_nhwc:
            dy = as_nhwc(dy)
            dx = torch.empty((b, c * h * w), dtype=dy.dtype, device=dy.device)
        else:
            dy = as_rows(dy)
            dx = nhwc_empty(b, c, h, w, dy.dtype, dy.device)
        L.call("sp_permute_chw_hwc", ptr(dy), ptr(dx), b, c, h * w, 0 if to_nhwc else 1, sp_dtype(dy.dtype), stream())
        return dx, None, None, None, None, None


def rows_to_nhwc(x, c, h, w, dest: Optional[Dest] = None):
    return _PermuteFn.apply(x, c, h, w, True, dest)


def _float3(values):
    """scale3 / shift3 of the plain ingest for L.call: a 3-float array behind a void pointer (which keeps it alive), or None."""
    return None if values is None else ctypes.cast((ctypes.c_float * 3)(*values), ctypes.c_void_p)


def _ingest_src_dtype(img: torch.Tensor, dtype) -> int:
    """src_dtype of every ingest entry, plain and augmenting: the image's own type, which must be fp32 or the storage type itself.  The
    two 16-bit types never mix: each compilation of the library decodes a 16-bit source as ITS 16-bit type (include/sempyr.h refuses the
    mix with SP_ERR_UNSUPPORTED; this says which tensor it was)."""
    if img.dtype != torch.float32 and img.dtype != dtype and is_16bit(img.dtype) and is_16bit(dtype):
        raise L.SempyrError("the ingest takes an fp32 image or one of the storage type: a %s image cannot be ingested into %s storage "
                            "(convert it first)" % (img.dtype, dtype))
    return sp_dtype(img.dtype)


class _IngestFn(torch.autograd.Function):
    """3-channel image (any strides; fp32 or compute dtype) -> NHWC with zero-padded channels, optional affine."""

    @staticmethod
    def forward(ctx, img, dtype, scale3, shift3):
        require_gpu(img)
        n, c, h, w = img.shape
        cp = pad_channels(c, dtype)
        y = nhwc_empty(n, cp, h, w, dtype, img.device)
        sn, scs, sh, sw = img.stride()
        L.call("sp_ingest_image", ptr(img), _ingest_src_dtype(img, dtype), sn, scs, sh, sw, ptr(y), n, c, h, w, cp, _float3(scale3), _float3(shift3),
               sp_dtype(dtype), stream())
        ctx.cfg = (n, c, h, w, cp, scale3, img.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w, cp, scale3, src_dtype = ctx.cfg
        dy = as_nhwc(dy)
        dsrc = nhwc_empty(n, c, h, w, dy.dtype, dy.device)
        L.call("sp_ingest_image_bwd", ptr(dy), cp, ptr(dsrc), c, n * h * w, _float3(scale3), sp_dtype(dy.dtype), stream())
        if dsrc.dtype != src_dtype:
            dsrc = dsrc.to(src_dtype)
        return dsrc, None, None, None


def ingest_image(img, dtype, scale3=None, shift3=None):
    return _IngestFn.apply(img, dtype, scale3, shift3)


def ingest_image_pair(img_a: torch.Tensor, img_b: torch.Tensor, dtype, scale3=None, shift3=None) -> torch.Tensor:
    """Two image batches (any strides; fp32 or compute dtype) -> ONE padded NHWC batch [a | b], optional per-channel affine (no
    autograd of its own: the discriminator step needs no image gradients, model_wrapper.py:150-160; the VGG pyramid's two-group pass
    takes the image gradient of group a in its own backward)."""
    with torch.no_grad():
        require_gpu(img_a)
        na, c, h, w = img_a.shape
        nb = img_b.shape[0]
        cp = pad_channels(c, dtype)
        y = nhwc_empty(na + nb, cp, h, w, dtype, img_a.device)
        esz = y.element_size()
        sc, sf = _float3(scale3), _float3(shift3)
        for img, off in ((img_a.detach(), 0), (img_b.detach(), na)):
            sn, scs, sh, sw = img.stride()
            L.call("sp_ingest_image", ptr(img), _ingest_src_dtype(img, dtype), sn, scs, sh, sw, ctypes.c_void_p(y.data_ptr() + off * h * w * cp * esz),
                   img.shape[0], c, h, w, cp, sc, sf, sp_dtype(dtype), stream())
    return y


# ---- differentiable augmentation inside the ingest pass (csrc/augment.hip; the transform is defined there and in DESIGN.md 11) ----
AUG_COLOR, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4
_AUG_WORDS = {"color": AUG_COLOR, "translation": AUG_TRANSLATION, "cutout": AUG_CUTOUT}


def _word_mask(value, table, what) -> int:
    """A comma-separated string of `table`'s words (any subset, any order; "" / None = none) or the bit mask itself -> the bit mask.
    what: how the errors name the family ("augmentation policy")."""
    if value is None:
        return 0
    if isinstance(value, int) and not isinstance(value, bool):
        if not 0 <= value <= sum(table.values()):
            raise L.SempyrError("%s mask %d: not an OR of %s" % (what, value, ", ".join("%s (%d)" % wb for wb in table.items())))
        return value
    if not isinstance(value, str):
        raise L.SempyrError("%s: a comma-separated string of %s (got %r)" % (what, " / ".join(table), value))
    mask = 0
    for word in value.split(","):
        word = word.strip()
        if not word:
            continue
        if word not in table:
            raise L.SempyrError("%s word %r: choose among %s" % (what, word, ", ".join(table)))
        mask |= table[word]
    return mask


def augment_policy(policy) -> int:
    """"color,translation,cutout" (any subset, any order; "" / None = none) or the bit mask itself -> the bit mask of
    include/sempyr.h's SP_AUG_*.  An unknown word raises."""
    return _word_mask(policy, _AUG_WORDS, "augmentation policy")


def augment_geometry(h: int, w: int):
    """(r_y, r_x, q_y, q_x, n_y, n_x) of an h x w map: translation radius, cutout window size and number of cutout centres, with
    the kernel's fp32 operations (csrc/augment.hip: aug_geom)."""
    hw = torch.tensor([h, w], dtype=torch.float32)
    ry, rx = (int(v) for v in (hw / 8.0 + 0.5).to(torch.int64))
    qy, qx = (int(v) for v in (hw / 2.0 + 0.5).to(torch.int64))
    return ry, rx, qy, qx, h + 1 - (qy % 2), w + 1 - (qx % 2)


def augment_decode(u: torch.Tensor, h: int, w: int, policy=7):
    """The kernel's decoding of `u` ((n, 8) uniforms in [0, 1)) for h x w images, on the host with the same fp32 operations:
    (o, s, k, t_y, t_x, c_y, c_x), fp32 / int64 tensors of n entries.  A part the policy leaves out decodes to the identity
    (o = 0, s = k = 1, t = 0); c_y / c_x mean nothing without cutout.  The cutout rows are [c_y - q_y // 2, c_y - q_y // 2 + q_y)
    cut with [0, h), q_y from augment_geometry()."""
    policy = augment_policy(policy)
    u = u.detach().to("cpu", torch.float32)
    if u.dim() != 2 or u.shape[1] != 8:
        raise L.SempyrError("augment_decode: u must be (n, 8), got %s" % (tuple(u.shape),))
    ry, rx, _, _, ny, nx = augment_geometry(h, w)
    n = u.shape[0]
    o, s, k = torch.zeros(n), torch.ones(n), torch.ones(n)
    ty = tx = torch.zeros(n, dtype=torch.int64)
    if policy & AUG_COLOR:
        o, s, k = u[:, 0] - 0.5, 2.0 * u[:, 1], u[:, 2] + 0.5

    def pick(col, count):          # min(int(floorf(u * float(count))), count - 1): one fp32 multiply, then floor
        return torch.floor(u[:, col] * torch.tensor(float(count), dtype=torch.float32)).to(torch.int64).clamp(max=count - 1)
    if policy & AUG_TRANSLATION:
        ty, tx = pick(3, 2 * ry + 1) - ry, pick(4, 2 * rx + 1) - rx
    cy, cx = pick(5, ny), pick(6, nx)
    return o, s, k, ty, tx, cy, cx


# the geometric family (csrc/augment.hip: THE GEOMETRIC FAMILY): a SEPARATE mask, so that augment_policy keeps refusing what it refused
GEOM_XFLIP, GEOM_ROT90, GEOM_SCALE, GEOM_ROTATE = 1, 2, 4, 8
_GEOM_WORDS = {"xflip": GEOM_XFLIP, "rot90": GEOM_ROT90, "scale": GEOM_SCALE, "rotate": GEOM_ROTATE}


def augment_geom(words) -> int:
    """"xflip,rot90,scale,rotate" (any subset, any order; "" / None = none) or the bit mask itself -> the bit mask of include/sempyr.h's
    SP_GEOM_*.  An unknown word raises (the words of augment_policy included: augment_split takes both families)."""
    return _word_mask(words, _GEOM_WORDS, "geometric augmentation")


def augment_split(policy):
    """One comma-separated string holding words of both families (or None, or augment_policy's bit mask) -> (policy bits, geom bits).
    A string without geometric words returns (augment_policy(policy), 0), and raises where augment_policy raises."""
    if not isinstance(policy, str):
        return augment_policy(policy), 0
    words = [w.strip() for w in policy.split(",")]
    geom = augment_geom(",".join(w for w in words if w in _GEOM_WORDS))
    return augment_policy(",".join(w for w in words if w not in _GEOM_WORDS)), geom


def augment_geom_table(u: torch.Tensor, v: torch.Tensor, h: int, w: int, policy, geom, dtype=torch.float32) -> torch.Tensor:
    """The decode launch's table ((n, 8): m00 m01 m02 m10 m11 m12 0 0) restated on the host from u (n, 8) and v (n, 4), operation by
    operation in `dtype`: fp32 gives the kernel's bits for rows without scale and rotate (entries in {-1, 0, 1}, exact offsets) and
    the kernel's expressions around the host's exp2 / cos / sin otherwise; float64 is the reference of the scale and rotate rows."""
    policy, geom = augment_policy(policy), augment_geom(geom)
    u = u.detach().to("cpu", torch.float32)
    v = v.detach().to("cpu", torch.float32)
    if u.dim() != 2 or u.shape[1] != 8 or v.dim() != 2 or tuple(v.shape) != (u.shape[0], 4):
        raise L.SempyrError("augment_geom_table: u must be (n, 8) and v (n, 4), got %s and %s" % (tuple(u.shape), tuple(v.shape)))
    if geom & GEOM_ROT90 and h != w:
        raise L.SempyrError("augment_geom_table: rot90 needs a square map (got %d x %d)" % (h, w))
    n = u.shape[0]
    const = lambda x: torch.tensor(x, dtype=torch.float32).to(dtype)      # noqa: E731  (the kernel's fp32 constants)
    vv = v.to(dtype)
    one, zero = torch.ones(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    a00, a01, a10, a11 = one, zero, zero, one
    if geom & (GEOM_SCALE | GEOM_ROTATE):
        gs, c, s = one, one, zero
        if geom & GEOM_SCALE:
            gs = torch.exp2(-(const(0.8) * vv[:, 2] - const(0.4)))
        if geom & GEOM_ROTATE:
            theta = (vv[:, 3] - 0.5) * const(math.pi / 2)
            c, s = torch.cos(theta), torch.sin(theta)
        a00, a01, a10, a11 = gs * c, -(gs * s), gs * s, gs * c
    if geom & GEOM_ROT90:
        k = torch.floor(4.0 * v[:, 1]).to(torch.int64).clamp(max=3)         # fp32, as the kernel
        for r in range(1, 4):                                               # Q . A: the rows swap, the new second row changes sign
            sel = k >= r
            a00, a01, a10, a11 = torch.where(sel, a10, a00), torch.where(sel, a11, a01), torch.where(sel, -a00, a10), torch.where(sel, -a01, a11)
    if geom & GEOM_XFLIP:
        flip = v[:, 0] < 0.5
        a10, a11 = torch.where(flip, -a10, a10), torch.where(flip, -a11, a11)
    ty, tx = augment_decode(u, h, w, policy & AUG_TRANSLATION)[3:5]
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    dy, dx = ty.to(dtype) - cy, tx.to(dtype) - cx
    m02 = (a00 * dy + a01 * dx) + cy
    m12 = (a10 * dy + a11 * dx) + cx
    return torch.stack([a00, a01, m02, a10, a11, m12, zero, zero], dim=1)


def augment_geom_decode(u: torch.Tensor, v: torch.Tensor, h: int, w: int, policy, geom, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE launch (include/sempyr.h: sp_augment_geom_decode): the affine tables of all rows of u (..., 8) and v (..., 4), contiguous fp32
    on the GPU, for h x w maps -> (rows, 8) fp32 (into `out` if given).  Reads only the policy's translation bit.
    augment_geom_table restates it on the host."""
    policy, geom = augment_policy(policy), augment_geom(geom)
    require_gpu(u)
    ok = lambda t, k: t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 2 and t.shape[-1] == k      # noqa: E731
    if not (ok(u, 8) and ok(v, 4) and u.shape[:-1] == v.shape[:-1] and u.device == v.device and u.numel() > 0):
        raise L.SempyrError("augment_geom_decode: u (..., 8) and v (..., 4) must be contiguous fp32 tensors on one GPU with the same leading "
                            "shape (got %s %s, %s %s)" % (tuple(u.shape), u.dtype, tuple(v.shape), v.dtype))
    n = u.numel() // 8
    if out is None:
        out = torch.empty((n, 8), dtype=torch.float32, device=u.device)
    elif not (ok(out, 8) and out.numel() == n * 8 and out.device == u.device):
        raise L.SempyrError("augment_geom_decode: out must be a contiguous fp32 tensor of %d x 8 on u's GPU" % n)
    L.call("sp_augment_geom_decode", ptr(u), ptr(v), n, h, w, policy, geom, ptr(out), stream())
    return out


# ADA's color group (csrc/augment.hip: THE COLOR MATRIX): a third mask, so that augment_policy and augment_geom keep refusing
# what they refused
CMAT_BRIGHTNESS, CMAT_CONTRAST, CMAT_LUMAFLIP, CMAT_HUE, CMAT_SATURATION = 1, 2, 4, 8, 16
_CMAT_WORDS = {"brightness": CMAT_BRIGHTNESS, "contrast": CMAT_CONTRAST, "lumaflip": CMAT_LUMAFLIP, "hue": CMAT_HUE,
               "saturation": CMAT_SATURATION}


def augment_cmat(words) -> int:
    """"brightness,contrast,lumaflip,hue,saturation" (any subset, any order; "" / None = none) or the bit mask itself -> the bit mask of
    include/sempyr.h's SP_CMAT_*.  An unknown word raises (the words of the other two families included: augment_split3 takes all)."""
    return _word_mask(words, _CMAT_WORDS, "color-matrix augmentation")


def augment_split3(policy):
    """One comma-separated string holding words of all three families (or None, or augment_policy's bit mask) -> (policy bits, geom
    bits, cmat bits).  Without color-matrix words: augment_split(policy) + (0,), raising where augment_split raises."""
    if not isinstance(policy, str):
        return augment_split(policy) + (0,)
    words = [w.strip() for w in policy.split(",")]
    cmat = augment_cmat(",".join(w for w in words if w in _CMAT_WORDS))
    return augment_split(",".join(w for w in words if w not in _CMAT_WORDS)) + (cmat,)


def augment_cmat_table(z: torch.Tensor, cmat, dtype=torch.float32) -> torch.Tensor:
    """The decode launch's ctable ((n, 12): L00 L01 L02 t L10 L11 L12 t L20 L21 L22 t) restated on the host from z (n, 8), operation by
    operation in `dtype`: fp32 gives the kernel's bits for rows without brightness, contrast, hue and saturation and the kernel's
    expressions around the host's log / sqrt / cos / sin / exp2 otherwise; float64 is the reference.  A part left out is not
    computed: its factor is the constant (no libm call)."""
    cmat = augment_cmat(cmat)
    z = z.detach().to("cpu", torch.float32)
    if z.dim() != 2 or z.shape[1] != 8:
        raise L.SempyrError("augment_cmat_table: z must be (n, 8), got %s" % (tuple(z.shape),))
    n = z.shape[0]
    const = lambda x: torch.tensor(x, dtype=torch.float32).to(dtype)      # noqa: E731  (the kernel's fp32 constants)
    zz = z.to(dtype)
    one, zero = torch.ones(n, dtype=dtype), torch.zeros(n, dtype=dtype)

    def nrm(a, b):          # Box-Muller: sqrtf(-2 * logf(1 - a)) * cosf(float(2 pi) * b)
        return torch.sqrt(-2.0 * torch.log(1.0 - zz[:, a])) * torch.cos(const(2.0 * math.pi) * zz[:, b])
    bb, c, s, cs, sn, f = zero, one, one, one, zero, one
    if cmat & CMAT_BRIGHTNESS:
        bb = const(0.2) * nrm(0, 1)
    if cmat & CMAT_CONTRAST:
        c = torch.exp2(0.5 * nrm(2, 3))
    if cmat & CMAT_SATURATION:
        s = torch.exp2(nrm(4, 5))
    if cmat & CMAT_HUE:
        theta = (2.0 * zz[:, 6] - 1.0) * const(math.pi)
        cs, sn = torch.cos(theta), torch.sin(theta)
    if cmat & CMAT_LUMAFLIP:
        f = torch.where(z[:, 7] < 0.5, -one, one)
    p, cs_ = c * f, c * s
    # 1 / sqrt 3 belongs to the closed form (K is a cross-product matrix only with it), not to the draw: rounded to `dtype`, not to fp32
    beta, gamma = cs_ * cs, (cs_ * sn) * torch.tensor(1.0 / math.sqrt(3.0), dtype=dtype)
    d = (p - beta) / 3.0
    di, lo, hi, t = beta + d, d - gamma, d + gamma, p * bb
    return torch.stack([di, lo, hi, t, hi, di, lo, t, lo, hi, di, t], dim=1)


def augment_cmat_decode(z: torch.Tensor, cmat, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE launch (include/sempyr.h: sp_augment_cmat_decode): the color matrices of all rows of z (..., 8), contiguous fp32 on the GPU
    -> (rows, 12) fp32 (into `out` if given).  augment_cmat_table restates it on the host."""
    cmat = augment_cmat(cmat)
    require_gpu(z)
    ok = lambda t, k: t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 2 and t.shape[-1] == k      # noqa: E731
    if not (ok(z, 8) and z.numel() > 0):
        raise L.SempyrError("augment_cmat_decode: z (..., 8) must be a contiguous fp32 tensor on the GPU (got %s %s)" % (tuple(z.shape), z.dtype))
    n = z.numel() // 8
    if out is None:
        out = torch.empty((n, 12), dtype=torch.float32, device=z.device)
    elif not (ok(out, 12) and out.numel() == n * 12 and out.device == z.device):
        raise L.SempyrError("augment_cmat_decode: out must be a contiguous fp32 tensor of %d x 12 on z's GPU" % n)
    L.call("sp_augment_cmat_decode", ptr(z), n, cmat, ptr(out), stream())
    return out


def _augment_ctable(ctable, n, device):
    """The color matrices of the sp_augment_cmat_* entries: contiguous fp32 (n, 12) on the images' GPU, 16-byte aligned.  None: the
    entries without one."""
    if ctable is None:
        return None
    if not (isinstance(ctable, torch.Tensor) and ctable.is_cuda and ctable.device == device and ctable.dtype == torch.float32
            and tuple(ctable.shape) == (n, 12) and ctable.is_contiguous() and ctable.data_ptr() % 16 == 0):
        raise L.SempyrError("the color-matrix augmenting ingest takes ctable as a contiguous, 16-byte aligned fp32 (n, 12) tensor on the "
                            "images' GPU, one row per image (got %r for %d images)"
                            % (((tuple(ctable.shape), ctable.dtype, str(ctable.device)) if isinstance(ctable, torch.Tensor) else ctable), n))
    return ctable


def _augment_table(table, n, device):
    """The affine table of the geometric entries: contiguous fp32 (n, 8) on the images' GPU.  None: the existing entries."""
    if table is None:
        return None
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.device == device and table.dtype == torch.float32
            and tuple(table.shape) == (n, 8) and table.is_contiguous()):
        raise L.SempyrError("the geometric augmenting ingest takes table as a contiguous fp32 (n, 8) tensor on the images' GPU, one row per "
                            "image (got %r for %d images)" % (((tuple(table.shape), table.dtype, str(table.device))
                                                                 if isinstance(table, torch.Tensor) else table), n))
    return table


def _augment_args(img, u, policy):
    require_gpu(img)
    policy = augment_policy(policy)
    if img.dim() != 4 or img.shape[1] != 3:
        raise L.SempyrError("the augmenting ingest takes 3-channel images (n, 3, h, w), got %s" % (tuple(img.shape),))
    if not (u.is_cuda and u.dtype == torch.float32 and tuple(u.shape) == (img.shape[0], 8) and u.is_contiguous()):
        raise L.SempyrError("the augmenting ingest takes u as a contiguous fp32 (n, 8) tensor on the GPU, one row per image (got %s %s for "
                            "%d images)" % (tuple(u.shape), u.dtype, img.shape[0]))
    return policy


def _augment_slices(entry, h, w, backward):
    out = ctypes.c_int64(0)
    L.call(entry, h, w, 1 if backward else 0, ctypes.byref(out))
    return int(out.value)


def augment_slices(h: int, w: int, backward: bool) -> int:
    """Partials per image that the statistics launch of the augmenting ingest writes (include/sempyr.h: sp_augment_slices)."""
    return _augment_slices("sp_augment_slices", h, w, backward)


def augment_geom_slices(h: int, w: int, backward: bool) -> int:
    """Partials per image of the geometric entries' statistics launch (include/sempyr.h: sp_augment_geom_slices)."""
    return _augment_slices("sp_augment_geom_slices", h, w, backward)


def _augment_partials(n, h, w, policy, backward, device, geom=False):
    if not policy & AUG_COLOR:
        return None
    return torch.empty((n, (augment_geom_slices if geom else augment_slices)(h, w, backward)), dtype=torch.float32, device=device)


def _augment_gate(p, device):
    """The gate's probability for the gated entries (include/sempyr.h): a 1-element fp32 tensor on the images' device, read by the
    kernel when it runs.  None: the ungated entries."""
    if p is None:
        return None
    if not (isinstance(p, torch.Tensor) and p.is_cuda and p.device == device and p.dtype == torch.float32 and p.numel() == 1):
        raise L.SempyrError("the gated augmenting ingest takes p as a 1-element fp32 tensor on the images' GPU (got %r)"
                            % (((tuple(p.shape), p.dtype, str(p.device)) if isinstance(p, torch.Tensor) else p),))
    return p


def _augment_entry(backward, p, table, part, ctable=None):
    """(name, arguments between `policy` and `dtype`) of the entry for this call - include/sempyr.h: the color-matrix entries with a
    ctable (table and p may be NULL there), the geometric entries with a table (p may be NULL there), the gated ones with p alone,
    else the plain ones."""
    bwd = "_bwd" if backward else ""
    if ctable is not None:
        return "sp_augment_cmat_ingest" + bwd, (ptr(table), ptr(ctable), ptr(part), ptr(p))
    if table is not None:
        return "sp_augment_geom_ingest" + bwd, (ptr(table), ptr(part), ptr(p))
    if p is not None:
        return "sp_augment_ingest%s_gated" % bwd, (ptr(part), ptr(p))
    return "sp_augment_ingest" + bwd, (ptr(part),)


def _augment_fwd(img, y_ptr, dtype, cp, u, policy, p=None, table=None, ctable=None):
    n, _, h, w = img.shape
    sn, scs, sh, sw = img.stride()
    part = _augment_partials(n, h, w, policy, False, img.device, table is not None)
    name, extra = _augment_entry(False, p, table, part, ctable)
    L.call(name, ptr(img), _ingest_src_dtype(img, dtype), sn, scs, sh, sw, y_ptr, n, h, w, cp, ptr(u), policy, *extra, sp_dtype(dtype), stream())


class _AugmentIngestFn(torch.autograd.Function):
    """_IngestFn with the augmentation applied in the same pass: T(img; u) -> NHWC with zero-padded channels; gradients flow through T."""

    @staticmethod
    def forward(ctx, img, dtype, u, policy, p=None, table=None, ctable=None):
        n, c, h, w = img.shape
        cp = pad_channels(c, dtype)
        y = nhwc_empty(n, cp, h, w, dtype, img.device)
        _augment_fwd(img, ptr(y), dtype, cp, u, policy, p, table, ctable)
        ctx.ctable = ctable                # None: the entries without one; else the backward applies the transposed matrices of the same rows
        ctx.cfg = (n, h, w, cp, policy, img.dtype)
        ctx.u = u
        ctx.table = table                  # None: the existing entries; else the geometric ones, whose backward gathers through the same table
        ctx.p = p                          # the gate reads the SAME device value in the backward pass: p is constant through a step
        return y

    @staticmethod
    def backward(ctx, dy):
        n, h, w, cp, policy, src_dtype = ctx.cfg
        dy = as_nhwc(dy)
        dsrc = nhwc_empty(n, 3, h, w, dy.dtype, dy.device)
        part = _augment_partials(n, h, w, policy, True, dy.device, ctx.table is not None)
        name, extra = _augment_entry(True, ctx.p, ctx.table, part, ctx.ctable)
        L.call(name, ptr(dy), cp, ptr(dsrc), n, h, w, ptr(ctx.u), policy, *extra, sp_dtype(dy.dtype), stream())
        if dsrc.dtype != src_dtype:
            dsrc = dsrc.to(src_dtype)
        return dsrc, None, None, None, None, None, None


def augment_ingest_image(img: torch.Tensor, dtype, u: torch.Tensor, policy, p: Optional[torch.Tensor] = None,
                         table: Optional[torch.Tensor] = None, ctable: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_image(T(img; u), dtype) in the ingest's own pass (csrc/augment.hip): u = (n, 8) fp32 uniforms on the device, one row per
    image, decoded in the kernel (augment_decode restates it); policy = "color,translation,cutout", a subset, or the bit mask.
    p: None, or the gate - a 1-element fp32 device tensor read when the kernels run: image i is transformed iff u[i, 7] < p, else it
    is ingested as ingest_image does it, bit for bit, forward and backward (AdaptiveAugment.p is such a tensor).
    table: None, or the (n, 8) affine table of augment_geom_decode: the geometric entries then resample the image through it (bilinear,
    zero padding; the backward is the adjoint by gather) and take the policy's color and cutout bits only - the translation is in the table.
    ctable: None, or the (n, 12) color matrices of augment_cmat_decode (any 3 x 4 matrices): the color-matrix entries then apply row i to
    every source pixel of image i as the last step of its color stage, in either family; the backward applies the transposed matrix."""
    policy = _augment_args(img, u, policy)
    return _AugmentIngestFn.apply(img, dtype, u, policy, _augment_gate(p, img.device), _augment_table(table, img.shape[0], img.device),
                                  _augment_ctable(ctable, img.shape[0], img.device))


def augment_ingest_image_pair(img_a: torch.Tensor, img_b: torch.Tensor, dtype, u_a: torch.Tensor, u_b: torch.Tensor, policy,
                              p: Optional[torch.Tensor] = None, table_a: Optional[torch.Tensor] = None,
                              table_b: Optional[torch.Tensor] = None, ctable=None) -> torch.Tensor:
    """ingest_image_pair with each batch under its own transform: ONE padded NHWC batch [T(a; u_a) | T(b; u_b)], no autograd of
    its own (the discriminator step needs no image gradient).  p: the gate of augment_ingest_image, for both batches.  table_a /
    table_b: both None, or each batch's affine table (augment_ingest_image's table).  ctable: None, or the pair (ctable_a, ctable_b) of
    the batches' color matrices (augment_ingest_image's ctable)."""
    with torch.no_grad():
        img_a, img_b = img_a.detach(), img_b.detach()
        policy = _augment_args(img_a, u_a, policy)
        _augment_args(img_b, u_b, policy)
        p = _augment_gate(p, img_a.device)
        na, c, h, w = img_a.shape
        if tuple(img_b.shape[1:]) != (c, h, w):
            raise L.SempyrError("augment_ingest_image_pair: image shapes differ (%s, %s)" % (tuple(img_a.shape), tuple(img_b.shape)))
        cp = pad_channels(c, dtype)
        y = nhwc_empty(na + img_b.shape[0], cp, h, w, dtype, img_a.device)
        esz = y.element_size()
        if (table_a is None) != (table_b is None):
            raise L.SempyrError("augment_ingest_image_pair: give both tables or none")
        table_a, table_b = _augment_table(table_a, na, img_a.device), _augment_table(table_b, img_b.shape[0], img_a.device)
        if ctable is None:
            ctable = (None, None)
        elif not (isinstance(ctable, (tuple, list)) and len(ctable) == 2 and ctable[0] is not None and ctable[1] is not None):
            raise L.SempyrError("augment_ingest_image_pair: ctable is None or the pair (ctable_a, ctable_b)")
        ct_a, ct_b = _augment_ctable(ctable[0], na, img_a.device), _augment_ctable(ctable[1], img_b.shape[0], img_a.device)
        for img, u, t, ct, off in ((img_a, u_a, table_a, ct_a, 0), (img_b, u_b, table_b, ct_b, na)):
            _augment_fwd(img, ctypes.c_void_p(y.data_ptr() + off * h * w * cp * esz), dtype, cp, u, policy, p, t, ct)
    return y


class AdaptiveAugment:
    """The probability p with which the augmenting ingest transforms an image, and its controller (Karras et al. 2020, "ADA";
    include/sempyr.h: sp_ada_observe / sp_ada_adjust).  The state - {p, r_last, pos, neg, total, steps,
    adjustments, reserved}, 8 x 4 bytes - lives on the device from construction on (never inside a graph's pool); the gated ingest
    kernels read p through a pointer when they run and the two controller launches read and write the rest, so nothing syncs with the
    host and a captured graph follows p without a re-capture (as ops.LossScaler's scale).
        observe(pred)   counts pred > threshold / pred < threshold (D's fp32 predictions on the real images; threshold 0.5 is the midpoint
                        of the LSGAN targets 1 and 0)
        adjust(batch)   once per training step: after `interval` steps r = (pos - neg) / total, and p moves by
                        step = float32(interval * batch / speed_images) towards 1 while r > target, towards 0 while r < target
    adaptive=False: a fixed p that is never observed or adjusted (both calls do nothing)."""

    def __init__(self, device, p: float = 0.0, target: float = 0.6, interval: int = 4, speed_images: int = 500_000, threshold: float = 0.5,
                 adaptive: bool = True):
        p, target, threshold = float(p), float(target), float(threshold)
        if not 0.0 <= p <= 1.0:
            raise L.SempyrError("AdaptiveAugment: p must lie in [0, 1], got %r" % (p,))
        if not -1.0 <= target <= 1.0:
            raise L.SempyrError("AdaptiveAugment: target must lie in [-1, 1], got %r" % (target,))
        if int(interval) != interval or interval < 1:
            raise L.SempyrError("AdaptiveAugment: interval must be an integer >= 1, got %r" % (interval,))
        if not speed_images > 0:
            raise L.SempyrError("AdaptiveAugment: speed_images must be > 0, got %r" % (speed_images,))
        if threshold != threshold:
            raise L.SempyrError("AdaptiveAugment: threshold is NaN")
        self.target, self.interval, self.speed_images, self.threshold, self.adaptive = target, int(interval), speed_images, threshold, bool(adaptive)
        self.state = torch.zeros(8, dtype=torch.int32, device=device)
        self.state[0:1].view(torch.float32).fill_(p)

    @property
    def p(self) -> torch.Tensor:
        """The 1-element fp32 view of the state that the gated ingest takes."""
        return self.state[0:1].view(torch.float32)

    @property
    def r(self) -> torch.Tensor:
        return self.state[1:2].view(torch.float32)

    def step_size(self, batch: int) -> float:
        """float32(interval * batch / speed_images), at most 1."""
        return min(1.0, float(torch.tensor(self.interval * int(batch) / self.speed_images, dtype=torch.float32)))

    def observe(self, pred: torch.Tensor) -> None:
        if not self.adaptive:
            return
        pred = pred.detach()
        if not (pred.is_cuda and pred.device == self.state.device and pred.dtype == torch.float32 and pred.numel() >= 1):
            raise L.SempyrError("AdaptiveAugment.observe: fp32 predictions on the state's GPU (got %s %s)" % (tuple(pred.shape), pred.dtype))
        pred = pred.contiguous()
        L.call("sp_ada_observe", ptr(pred), pred.numel(), self.threshold, ptr(self.state), stream())

    def adjust(self, batch: int) -> None:
        if not self.adaptive:
            return
        L.call("sp_ada_adjust", ptr(self.state), self.interval, self.target, self.step_size(batch), stream())

    def values(self) -> dict:
        """Host copy (syncs): for tests and logs."""
        s = self.state.cpu()
        f = s[0:2].view(torch.float32).tolist()
        i = s.tolist()
        return {"p": f[0], "r_last": f[1], "pos": i[2], "neg": i[3], "total": i[4], "steps": i[5], "adjustments": i[6]}

    def settings(self) -> dict:
        return {"target": self.target, "interval": self.interval, "speed_images": self.speed_images, "threshold": self.threshold,
                "adaptive": self.adaptive}

    def state_dict(self) -> dict:
        return dict(self.settings(), state=self.state.detach().cpu().clone())

    def load_state_dict(self, sd: dict) -> None:
        """Restores the device state IN PLACE (captured graphs have its address baked in) and the settings that came with it."""
        state = sd["state"]
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.int32 and tuple(state.shape) == (8,)):
            raise L.SempyrError("AdaptiveAugment.load_state_dict: 'state' must be an int32 tensor of 8 words")
        for key in ("target", "interval", "speed_images", "threshold", "adaptive"):
            if key in sd:
                setattr(self, key, sd[key])
        self.state.copy_(state)


def apa_select(real: torch.Tensor, fake: torch.Tensor, w_u: torch.Tensor, p: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adaptive pseudo augmentation's selection (Jiang et al. 2021; include/sempyr.h: sp_apa_select), ONE launch: a
    contiguous fp32 (n, 3, h, w) batch whose image i is fake[i] iff w_u[i] < p (strict, fp32), else real[i] - 16-bit values widened
    exactly, fp32 values bit for bit.  real / fake: 3-channel batches of one shape on the GPU, any strides, each fp32 or a 16-bit type
    (the two 16-bit types never mix: the storage type of the call is the 16-bit type among them).  w_u: (n,) fp32 uniforms on that
    device; p: the 1-element fp32 device tensor of the gate (_augment_gate; AdaptiveAugment.p is one), read when the kernel runs.
    out: the result's buffer (the graphs' static one), else a fresh tensor.  Runs under no_grad: the result carries no autograd graph -
    APA feeds detached images to D."""
    with torch.no_grad():
        real, fake = real.detach(), fake.detach()
        require_gpu(real)
        if real.dim() != 4 or real.shape[1] != 3 or tuple(fake.shape) != tuple(real.shape) or fake.device != real.device:
            raise L.SempyrError("apa_select takes two 3-channel batches (n, 3, h, w) of one shape on one GPU, got %s and %s"
                                % (tuple(real.shape), tuple(fake.shape)))
        p = _augment_gate(p, real.device)
        if p is None:
            raise L.SempyrError("apa_select takes p as a 1-element fp32 tensor on the images' GPU (got None)")
        n, _, h, w = real.shape
        if not (isinstance(w_u, torch.Tensor) and w_u.device == real.device and w_u.dtype == torch.float32 and tuple(w_u.shape) == (n,)
                and w_u.is_contiguous()):
            raise L.SempyrError("apa_select takes w_u as a contiguous fp32 (n,) tensor on the images' GPU, one uniform per image (got %r for "
                                "%d images)" % (((tuple(w_u.shape), w_u.dtype, str(w_u.device)) if isinstance(w_u, torch.Tensor) else w_u), n))
        # the storage type: the 16-bit type among the sources (fp32 without one); _ingest_src_dtype refuses the other 16-bit type
        dtype = real.dtype if is_16bit(real.dtype) else (fake.dtype if is_16bit(fake.dtype) else torch.float32)
        dt_real, dt_fake = _ingest_src_dtype(real, dtype), _ingest_src_dtype(fake, dtype)
        if out is None:
            out = torch.empty((n, 3, h, w), dtype=torch.float32, device=real.device)
        elif not (out.device == real.device and out.dtype == torch.float32 and tuple(out.shape) == (n, 3, h, w) and out.is_contiguous()):
            raise L.SempyrError("apa_select: out must be a contiguous fp32 %s tensor on the images' GPU (got %s %s)"
                                % ((n, 3, h, w), tuple(out.shape), out.dtype))
        L.call("sp_apa_select", ptr(real), dt_real, *real.stride(), ptr(fake), dt_fake, *fake.stride(), ptr(out), n, h, w, ptr(w_u), ptr(p),
               sp_dtype(dtype), stream())
    return out


def mask_concat(feat: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """cat(feat * mask, mask) with the channel count padded to a 16-byte multiple (models.py:94).  No autograd:
    the features come from the frozen VGG under no_grad and mask gradients are dead."""
    with torch.no_grad():
        feat = as_nhwc(feat.detach(), compute_dtype())
        require_gpu(feat)
        n, h, w, c = dims(feat)
        cp = pad_channels(c + 1, feat.dtype)
        mask = mask.detach().to(torch.float32).contiguous()
        out = nhwc_empty(n, cp, h, w, feat.dtype, feat.device)
        L.call("sp_mask_concat", ptr(feat), ptr(mask), ptr(out), n * h * w, c, cp, sp_dtype(feat.dtype), stream())
    return out


def mask_mul_2d(feat: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        feat = as_rows(feat.detach(), compute_dtype())
        require_gpu(feat)
        b, k = feat.shape
        mask = mask.detach().to(torch.float32).contiguous()
        out = torch.empty((b, k), dtype=feat.dtype, device=feat.device)
        L.call("sp_mask_mul_2d", ptr(feat), feat.stride(0), ptr(mask), ptr(out), k, b, k, sp_dtype(feat.dtype), stream())
    return out


# ======================================================================================================
# attention core
# ======================================================================================================
class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, dest: Optional[Dest] = None):
        """dest (filled): extra = the log-sum-exp rows of the same images, as the launch over the whole batch left them."""
        require_gpu(q)
        b, hq, wq, d = dims(q)
        _, hk, wk, dv = dims(v)
        n, nk = hq * wq, hk * wk
        if dest is not None:
            if not dest.filled or dest.extra is None:
                raise L.SempyrError("attention_core: a destination must come filled, with its log-sum-exp rows")
            o, lse = _dest_tensor(dest, (b, dv, hq, wq), q), dest.extra
        else:
            o = nhwc_empty(b, dv, hq, wq, q.dtype, q.device)
            lse = torch.empty((b, n), dtype=torch.float32, device=q.device)
            L.call("sp_attention_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, n, nk, d, dv, sp_dtype(q.dtype), stream())
        ctx.save_for_backward(q, k, v, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, lse = ctx.saved_tensors
        b, hq, wq, d = dims(q)
        _, hk, wk, dv = dims(v)
        n, nk = hq * wq, hk * wk
        do = as_nhwc(do, q.dtype)
        dq, dk, dvv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        nqb = _attention_slabs(n, nk, d, dv, q.dtype)   # scratch: one partial slab per query block (include/sempyr.h)
        dk32 = torch.empty(nqb * b * nk * d, dtype=torch.float32, device=q.device)
        dv32 = torch.empty(nqb * b * nk * dv, dtype=torch.float32, device=q.device)
        L.call("sp_attention_bwd", ptr(q), ptr(k), ptr(v), ptr(do), ptr(lse), ptr(dq), ptr(dk32), ptr(dv32), ptr(dk), ptr(dvv),
               b, n, nk, d, dv, sp_dtype(q.dtype), stream())
        return dq, dk, dvv, None


_ATTN_SLABS = {}


def _attention_slabs(n, nk, d, dv, dtype) -> int:
    key = (n, nk, d, dv, dtype)
    v = _ATTN_SLABS.get(key)
    if v is None:
        out = ctypes.c_int64(0)
        L.call("sp_attention_bwd_slabs", n, nk, d, dv, sp_dtype(dtype), ctypes.byref(out))
        v = _ATTN_SLABS[key] = int(out.value)
    return v


def attention_core(q, k, v, dest: Optional[Dest] = None):
    return _AttentionFn.apply(q, k, v, dest)


def attention_raw(q, k, v):
    """(output, log-sum-exp rows) of the attention core without autograd (a batch of two groups, models.Generator.forward_pair)."""
    with torch.no_grad():
        require_gpu(q)
        b, hq, wq, d = dims(q)
        _, hk, wk, dv = dims(v)
        n, nk = hq * wq, hk * wk
        o = nhwc_empty(b, dv, hq, wq, q.dtype, q.device)
        lse = torch.empty((b, n), dtype=torch.float32, device=q.device)
        L.call("sp_attention_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, n, nk, d, dv, sp_dtype(q.dtype), stream())
    return o, lse


# ======================================================================================================
# discriminator head and losses
# ======================================================================================================
class _DHeadFn(torch.autograd.Function):
    """pred[i][j][c] = x[j][c] * E_sn[cls[i]][c] + (wc_sn . x[j] + bc)  (models.py:149-155)."""

    @staticmethod
    def forward(ctx, x, h_emb, h_cls, cls_b, cls, pl_emb: PackedLayer, pl_cls: PackedLayer):
        require_gpu(x)
        b, f = x.shape
        pred = torch.empty((b, b, f), dtype=torch.float32, device=x.device)
        L.call("sp_dhead_fwd", ptr(x), x.stride(0), ctypes.c_void_p(pl_emb.fwd), ptr(cls), ctypes.c_void_p(pl_cls.fwd), ptr(cls_b),
               ptr(pred), b, f, sp_dtype(x.dtype), stream())
        ctx.pls = (pl_emb, pl_cls)
        ctx.save_for_backward(x, cls)
        return pred

    @staticmethod
    def backward(ctx, dpred):
        x, cls = ctx.saved_tensors
        pl_emb, pl_cls = ctx.pls
        b, f = x.shape
        dpred = dpred.contiguous().float()
        dev = x.device
        need = ctx.needs_input_grad
        dx = torch.empty_like(x)
        # gradients w.r.t. the normalised embedding / classifier go to the layers' arena slots (or to scratch if unused)
        demb_sn = pl_emb.call.dw_slot(pl_emb) if need[1] else torch.empty(pl_emb.rows * pl_emb.cols, dtype=torch.float32, device=dev)
        dwc_sn = pl_cls.call.dw_slot(pl_cls) if need[2] else torch.empty(f, dtype=torch.float32, device=dev)
        # direct mode: the classification bias gradient goes to the layer's bias slot of the arena, so the batched spectral-norm
        # backward moves it into the flat buffer BEFORE the group's on_group_done hook hands that range to the reducer (round-3
        # ADVICE: returned through autograd it reached `flat` only after .backward(), i.e. after the range had been all-reduced)
        slot_bias = need[2] and need[3] and pl_cls.call.bank.direct_grads
        dbc = pl_cls.call.db_slot(pl_cls) if slot_bias else torch.empty(1, dtype=torch.float32, device=dev)
        sdp = torch.empty(b, dtype=torch.float32, device=dev)             # per-sample sums between the call's two kernels
        L.call("sp_dhead_bwd", ptr(dpred), ptr(x), x.stride(0), ctypes.c_void_p(pl_emb.fwd), ptr(cls), ctypes.c_void_p(pl_cls.fwd),
               ptr(dx), dx.stride(0), ptr(demb_sn), pl_emb.rows, ptr(dwc_sn), ptr(dbc), ptr(sdp), b, f, sp_dtype(x.dtype), stream())
        z = _zero1(dev)
        return dx, (z if need[1] else None), (z if need[2] else None), (dbc if need[3] and not slot_bias else None), None, None, None


def discriminator_head(x, emb_module, cls_module, cls_idx):
    pl_e = packed_layer(emb_module, emb_module.training, x.dtype, x.device)
    pl_c = packed_layer(cls_module, cls_module.training, x.dtype, x.device)
    return _DHeadFn.apply(x, pl_e.handle, pl_c.handle, cls_module.bias, cls_idx, pl_e, pl_c)


class _SqErrLossFn(torch.autograd.Function):
    """0.5 * mean((p - target)^2)   (lossfunction.py:137,164)."""

    @staticmethod
    def forward(ctx, p, target):
        require_gpu(p)
        p = p.contiguous().float()
        acc = torch.empty(1, dtype=torch.float64, device=p.device)        # (used above 2^18 elements only; an allocation, no launch)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sp_sqerr_loss_fwd", ptr(p), p.numel(), float(target), ptr(acc), ptr(loss), stream())
        ctx.target = float(target)
        ctx.save_for_backward(p)
        return loss

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        g = g.contiguous().float()
        dp = torch.empty_like(p)
        L.call("sp_sqerr_loss_bwd", ptr(p), p.numel(), ctx.target, ptr(g), ptr(dp), stream())
        return dp, None


def sqerr_loss(p, target: float):
    return _SqErrLossFn.apply(p, target)


GAN_LOSS_KINDS = {"hinge": 0, "logistic": 1}
GAN_LOSS_ROLES = {"d_real": 0, "d_fake": 1, "g": 2}


class _GanLossFn(torch.autograd.Function):
    """mean f(p) of the hinge / logistic losses (include/sempyr.h: sp_gan_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, p, kind, role):
        require_gpu(p)
        p = p.contiguous().float()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sp_gan_loss_fwd", ptr(p), p.numel(), kind, role, ptr(loss), stream())
        ctx.kind, ctx.role = kind, role
        ctx.save_for_backward(p)
        return loss

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        g = g.contiguous().float()
        dp = torch.empty_like(p)
        L.call("sp_gan_loss_bwd", ptr(p), p.numel(), ctx.kind, ctx.role, ptr(g), ptr(dp), stream())
        return dp, None, None


def gan_loss(p, kind: str, role: str):
    """kind "hinge" | "logistic", role "d_real" | "d_fake" | "g": the mean of max(0, 1 -/+ p) / -p, or of softplus(-/+ p) / softplus(-p),
    over the fp32 predictions p, as a differentiable scalar (LSGAN stays ops.sqerr_loss)."""
    if kind not in GAN_LOSS_KINDS or role not in GAN_LOSS_ROLES:
        raise L.SempyrError("gan_loss: kind must be one of %s and role one of %s (got %r, %r)"
                            % (sorted(GAN_LOSS_KINDS), sorted(GAN_LOSS_ROLES), kind, role))
    return _GanLossFn.apply(p, GAN_LOSS_KINDS[kind], GAN_LOSS_ROLES[role])


class _LeCamFn(torch.autograd.Function):
    """One forward launch (means, anchors, regularizer) and one backward launch on the LeCam state (sp_lecam_fwd / sp_lecam_bwd)."""

    @staticmethod
    def forward(ctx, pred_real, pred_fake, lecam):
        pred_real, pred_fake = pred_real.contiguous(), pred_fake.contiguous()
        reg = torch.empty((), dtype=torch.float32, device=pred_real.device)
        L.call("sp_lecam_fwd", ptr(pred_real), ptr(pred_fake), pred_real.numel(), lecam.weight, lecam.decay, lecam.start,
               int(lecam.rectified), ptr(lecam.state), ptr(reg), stream())
        ctx.lecam = lecam
        ctx.save_for_backward(pred_real, pred_fake)
        return reg

    @staticmethod
    def backward(ctx, g):
        pred_real, pred_fake = ctx.saved_tensors
        lecam = ctx.lecam
        g = g.contiguous().float()
        d_real, d_fake = torch.empty_like(pred_real), torch.empty_like(pred_fake)
        L.call("sp_lecam_bwd", ptr(pred_real), ptr(pred_fake), pred_real.numel(), lecam.weight, int(lecam.rectified), ptr(lecam.state),
               ptr(g), ptr(d_real), ptr(d_fake), stream())
        return d_real, d_fake, None


class LeCam:
    """The LeCam regularizer of the discriminator (Tseng et al., CVPR 2021; include/sempyr.h: sp_lecam_fwd / sp_lecam_bwd; DESIGN.md
    section 18): D's predictions are pulled towards moving averages ("anchors") of its own mean prediction on the opposite class,
        reg = weight * (mean h(pred_real - a_fake)^2 + mean h(a_real - pred_fake)^2),   h(x) = x, or max(x, 0) if rectified.
    The state - {a_real, a_fake, updates, active, m_real, m_fake, 0, 0}, 8 x 4 bytes - lives on the device from construction on (never
    inside a graph's pool), as AdaptiveAugment.state does: nothing syncs with the host and a captured graph follows the anchors.
        __call__(pred_real, pred_fake)   one launch: the two means, the anchor update (plain assignment of the means during the first
                        `start` calls, then a = decay * a + (1 - decay) * mean; a call whose means are not finite leaves the anchors and
                        the count alone), and the regularizer on the UPDATED anchors - 0 during the first `start` calls.  Differentiable
                        in both predictions (the anchors are constants); the backward reads the state that forward left."""

    def __init__(self, device, weight: float, decay: float = 0.99, start: int = 1000, rectified: bool = False):
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) < math.inf:
            raise L.SempyrError("LeCam: weight must be a finite number >= 0, got %r" % (weight,))
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise L.SempyrError("LeCam: decay must lie in [0, 1), got %r" % (decay,))
        if isinstance(start, bool) or int(start) != start or not 0 <= start < 2 ** 31:
            raise L.SempyrError("LeCam: start must be an integer >= 0, got %r" % (start,))
        self.weight, self.decay, self.start, self.rectified = float(weight), float(decay), int(start), bool(rectified)
        self.state = torch.zeros(8, dtype=torch.int32, device=device)

    @property
    def anchor_real(self) -> torch.Tensor:
        return self.state[0:1].view(torch.float32)

    @property
    def anchor_fake(self) -> torch.Tensor:
        return self.state[1:2].view(torch.float32)

    @property
    def updates(self) -> torch.Tensor:
        return self.state[2:3]

    def __call__(self, pred_real: torch.Tensor, pred_fake: torch.Tensor) -> torch.Tensor:
        for t in (pred_real, pred_fake):
            if not (t.is_cuda and t.device == self.state.device and t.dtype == torch.float32 and t.numel() >= 1):
                raise L.SempyrError("LeCam: fp32 predictions on the state's GPU (got %s %s)" % (tuple(t.shape), t.dtype))
        if pred_real.numel() != pred_fake.numel():
            raise L.SempyrError("LeCam: %d real and %d fake predictions (the two must be as many)" % (pred_real.numel(), pred_fake.numel()))
        return _LeCamFn.apply(pred_real, pred_fake, self)

    def values(self) -> dict:
        """Host copy (syncs): for tests and logs."""
        s = self.state.cpu()
        f = s.view(torch.float32).tolist()
        i = s.tolist()
        return {"anchor_real": f[0], "anchor_fake": f[1], "updates": i[2], "active": i[3], "mean_real": f[4], "mean_fake": f[5]}

    def settings(self) -> dict:
        return {"weight": self.weight, "decay": self.decay, "start": self.start, "rectified": self.rectified}

    def state_dict(self) -> dict:
        return dict(self.settings(), state=self.state.detach().cpu().clone())

    def load_state_dict(self, sd: dict) -> None:
        """Restores the device state IN PLACE (captured graphs have its address baked in) and the settings that came with it."""
        state = sd["state"]
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.int32 and tuple(state.shape) == (8,)):
            raise L.SempyrError("LeCam.load_state_dict: 'state' must be an int32 tensor of 8 words")
        for key in ("weight", "decay", "start", "rectified"):
            if key in sd:
                setattr(self, key, sd[key])
        self.state.copy_(state)


def _level_geometry(t: torch.Tensor):
    if t.dim() == 4:
        n, h, w, c = dims(t)
        return n, h, w, c, c
    return t.shape[0], 1, 1, t.shape[1], t.stride(0)


class _RecLossFn(torch.autograd.Function):
    """weight * sum over pyramid levels of mean(|maxpool2(real) - maxpool2(fake)| * maxpool2(mask))  (lossfunction.py:31-68), all
    levels in ONE launch forward and ONE backward (sp_rec_loss_fwd_levels / _bwd_levels).  Inputs after (n_levels, weight): fake
    features (differentiable); real features and masks are constants."""

    @staticmethod
    def _levels(prepared, dfakes=None):
        arr = (L.SpRecLevel * len(prepared))()
        for i, (f, r, m) in enumerate(prepared):
            n, h, w, c, ld = _level_geometry(f)
            lv = arr[i]
            lv.real, lv.fake, lv.mask = r.data_ptr(), f.data_ptr(), m.data_ptr()
            lv.ld_real, lv.ld_fake, lv.n, lv.h, lv.w_, lv.c = _level_geometry(r)[4], ld, n, h, w, c
            if dfakes is not None and dfakes[i] is not None:
                lv.dfake = dfakes[i].data_ptr()
                lv.ld_dfake = c if f.dim() == 4 else dfakes[i].stride(0)
        return arr

    @staticmethod
    def forward(ctx, n_levels, weight, *tensors):
        fakes = tensors[:n_levels]
        reals = tensors[n_levels:2 * n_levels]
        masks = tensors[2 * n_levels:]
        dev = fakes[0].device
        require_gpu(fakes[0])
        dt = fakes[0].dtype
        prepared = []
        for f, r, m in zip(fakes, reals, masks):
            if f.dtype != dt:
                raise L.SempyrError("semantic reconstruction loss: the levels must share one storage type")
            if f.dim() == 4:
                f, r = as_nhwc(f), as_nhwc(r.detach(), dt)
            else:
                f, r = as_rows(f), as_rows(r.detach(), dt)
            prepared.append((f, r, m.detach().to(torch.float32).contiguous()))
        loss = torch.empty(1, dtype=torch.float32, device=dev)       # the reference's loss is shape (1,) (lossfunction.py:42)
        acc = _loss_acc(dev)
        L.call("sp_rec_loss_fwd_levels", _RecLossFn._levels(prepared), n_levels, ctypes.c_void_p(acc.data_ptr() + 16), ptr(loss),
               float(weight), sp_dtype(dt), stream())
        ctx.n_levels, ctx.weight = n_levels, float(weight)
        ctx.save_for_backward(*[t for trip in prepared for t in trip])
        return loss

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g = g.contiguous().float()
        prepared, dfakes = [], []
        for i in range(ctx.n_levels):
            if not ctx.needs_input_grad[2 + i]:
                continue
            f, r, m = saved[3 * i:3 * i + 3]
            n, h, w, c, ld = _level_geometry(f)
            prepared.append((f, r, m))
            dfakes.append(torch.empty_like(f) if f.dim() == 4 else torch.empty((n, c), dtype=f.dtype, device=f.device))
        if prepared:
            L.call("sp_rec_loss_bwd_levels", _RecLossFn._levels(prepared, dfakes), len(prepared), ptr(g), ctx.weight,
                   sp_dtype(prepared[0][0].dtype), stream())
        it = iter(dfakes)
        grads = [next(it) if ctx.needs_input_grad[2 + i] else None for i in range(ctx.n_levels)]
        return (None, None, *grads, *([None] * (2 * ctx.n_levels)))


def semantic_reconstruction_loss(features_real, features_fake, masks, weight: float = 1.0):
    n = len(features_fake)
    return _RecLossFn.apply(n, weight, *features_fake, *features_real, *masks)


class _DivLossFn(torch.autograd.Function):
    """mean|z1 - z2| / (mean|img1 - img2| + 1e-8) over the two halves of the batch (lossfunction.py:92-110)."""

    @staticmethod
    def forward(ctx, img, z, weight):
        require_gpu(img)
        b = img.shape[0]
        if b < 2 or b % 2:
            raise L.SempyrError("diversity loss needs an even batch size > 1 (got %d)" % b)
        img = as_nhwc(img)
        z = z.detach().to(torch.float32).contiguous()
        half = img.numel() // 2
        out = torch.empty(2, dtype=torch.float32, device=img.device)      # weight * (loss, d loss / d |img1 - img2| per element)
        L.call("sp_div_loss_fwd_w", ptr(img), half, ptr(z), z.numel() // 2, ptr(_loss_acc(img.device)), ptr(out), float(weight),
               sp_dtype(img.dtype), stream())
        ctx.save_for_backward(img, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        img, out = ctx.saved_tensors
        g = g.contiguous().float()
        dimg = torch.empty_like(img)
        L.call("sp_div_loss_bwd", ptr(img), img.numel() // 2, ptr(out), ptr(g), ptr(dimg), sp_dtype(img.dtype), stream())
        return dimg, None, None


def diversity_loss(img, z, weight: float = 1.0):
    return _DivLossFn.apply(img, z, weight)


# ======================================================================================================
# fp8 (OCP e4m3) convolution path - BASELINE.json config 5 (include/sempyr.h: SP_F8)
# ======================================================================================================
def quantize_fp8(x: torch.Tensor, inv_scale: torch.Tensor, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC bf16 / fp32 activation -> uint8 tensor of e4m3 bytes with the same geometry, q = sat(x * inv_scale[0])."""
    require_gpu(x)
    n, h, w, c = dims(x)
    q = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device).permute(0, 3, 1, 2)
    L.call("sp_quantize_fp8", ptr(x), ptr(q), n * h * w * c, ptr(inv_scale), ptr(amax), sp_dtype(x.dtype), stream())
    return q


def pack_weight_fp8(w: torch.Tensor):
    """Conv weight (O, I, 3, 3) fp32 on the device -> (e4m3 bytes [O][9][cin_p], per-output-channel scales [O], cin_p)."""
    require_gpu(w)
    o, i = w.shape[0], w.shape[1]
    cin_p = pad_to(i, 16)
    out = torch.empty(o * 9 * cin_p, dtype=torch.uint8, device=w.device)
    scale = torch.empty(o, dtype=torch.float32, device=w.device)
    L.call("sp_pack_weight_fp8", ptr(w.contiguous()), o, i, cin_p, ptr(out), ptr(scale), stream())
    return out, scale, cin_p


def conv_launch_f8(x8: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, x_scale: torch.Tensor, bias, y, y8, y8_inv_scale, y8_amax,
                   n: int, h: int, w: int, cin_p: int, cout: int, act: int, pool2: int = 0) -> None:
    """3x3 convolution on the fp8 MFMA (sp_conv2d_igemm with dtype SP_F8): x8 / w8 e4m3 bytes, y bf16 and / or y8 e4m3 outputs."""
    p = L.SpConvParams()
    p.x, p.w, p.bias = x8.data_ptr(), w8.data_ptr(), (bias.data_ptr() if bias is not None else None)
    p.y = y.data_ptr() if y is not None else None
    p.n, p.h, p.w_, p.cin_p, p.cout, p.ldy, p.ksize, p.act = n, h, w, cin_p, cout, cout, 3, act
    p.dtype = L.SP_F8_F16 if compute_dtype() == torch.float16 else L.SP_F8       # e4m3 operands; 16-bit outputs in the storage type
    p.pool2 = pool2
    p.x_scale, p.w_scale = x_scale.data_ptr(), w_scale.data_ptr()
    p.y8 = y8.data_ptr() if y8 is not None else None
    p.y8_inv_scale = y8_inv_scale.data_ptr() if y8_inv_scale is not None else None
    p.y8_amax = y8_amax.data_ptr() if y8_amax is not None else None
    if KERNEL_PROBE is not None:
        _probed("fwd", 2.0 * n * h * w * cin_p * cout * 9, lambda: L.call("sp_conv2d_igemm", ctypes.byref(p), stream()), (3, cin_p, cout, h, w, n))
        return
    L.call("sp_conv2d_igemm", ctypes.byref(p), stream())


# ---- pair-set metrics (csrc/metrics.hip): thin calls; metrics.py holds the definitions ------------------------------
def pairset_workspace_bytes(na: int, nb: int, d: int, k: int) -> int:
    """sp_pairset_workspace (host logic: works without a GPU); SempyrError with the library's message for k > 16 or k >= nb."""
    out = ctypes.c_int64(0)
    L.call("sp_pairset_workspace", na, nb, d, k, ctypes.byref(out))
    return int(out.value)


def _pairset_set(x: torch.Tensor) -> torch.Tensor:
    require_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous() or x.shape[1] % 4 != 0:
        raise L.SempyrError("pair-set kernels take contiguous fp32 (n, d) tensors with d % 4 == 0 (metrics.py pads), got %s %s"
                            % (x.dtype, tuple(x.shape)))
    return x


def _pairset_ws(workspace: Optional[torch.Tensor], need: int, device) -> torch.Tensor:
    if workspace is None:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
    if workspace.numel() * workspace.element_size() < need:
        raise L.SempyrError("pair-set workspace of %d bytes needed, %d given" % (need, workspace.numel() * workspace.element_size()))
    return workspace


def pairset_knn(a: torch.Tensor, b: torch.Tensor, k: int, same: bool = False, d: Optional[int] = None, workspace=None) -> torch.Tensor:
    """radius[i] = k-th smallest squared distance from a_i to the rows of b (same: b is a, the own row skipped by index).  d: the
    leading columns read (default all)."""
    a, b = _pairset_set(a), _pairset_set(b)
    d = a.shape[1] if d is None else d
    ws = _pairset_ws(workspace, pairset_workspace_bytes(a.shape[0], b.shape[0], d, k), a.device)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    L.call("sp_pairset_knn", ptr(a), a.shape[0], a.shape[1], ptr(b), b.shape[0], b.shape[1], d, k, int(same), ptr(out), ptr(ws),
           ws.numel() * ws.element_size(), stream())
    return out


def pairset_cover(a: torch.Tensor, b: torch.Tensor, rad_a: Optional[torch.Tensor] = None, rad_b: Optional[torch.Tensor] = None,
                  d: Optional[int] = None, workspace=None):
    """(row_count, col_count, row_min, col_min) of sp_pairset_cover in one pass; a count is None without its radii."""
    a, b = _pairset_set(a), _pairset_set(b)
    d = a.shape[1] if d is None else d
    na, nb = a.shape[0], b.shape[0]
    ws = _pairset_ws(workspace, pairset_workspace_bytes(na, nb, d, 0), a.device)
    row_count = torch.empty(na, dtype=torch.int32, device=a.device) if rad_b is not None else None
    col_count = torch.empty(nb, dtype=torch.int32, device=a.device) if rad_a is not None else None
    row_min = torch.empty(na, dtype=torch.float32, device=a.device)
    col_min = torch.empty(nb, dtype=torch.float32, device=a.device)
    L.call("sp_pairset_cover", ptr(a), na, a.shape[1], ptr(b), nb, b.shape[1], d, ptr(rad_a), ptr(rad_b), ptr(row_count), ptr(col_count),
           ptr(row_min), ptr(col_min), ptr(ws), ws.numel() * ws.element_size(), stream())
    return row_count, col_count, row_min, col_min


def pairset_poly3(a: torch.Tensor, idx_a: Optional[torch.Tensor], b: torch.Tensor, idx_b: Optional[torch.Tensor], subsets: int, m: int,
                  skip_diag: bool, d: Optional[int] = None, workspace=None) -> torch.Tensor:
    """float64 [subsets]: per subset the sum over its m x m pairs of (a_i.b_j / d + 1)^3; idx_*: int32 (subsets, m) on the device."""
    a, b = _pairset_set(a), _pairset_set(b)
    d = a.shape[1] if d is None else d
    for idx in (idx_a, idx_b):
        if idx is not None and (idx.dtype != torch.int32 or not idx.is_cuda or not idx.is_contiguous() or idx.numel() != subsets * m):
            raise L.SempyrError("pair-set index tables are contiguous int32 (subsets, m) device tensors")
    ws = _pairset_ws(workspace, subsets * pairset_workspace_bytes(m, m, d, 0), a.device)
    out = torch.empty(subsets, dtype=torch.float64, device=a.device)
    L.call("sp_pairset_poly3", ptr(a), a.shape[0], a.shape[1], ptr(idx_a), ptr(b), b.shape[0], b.shape[1], ptr(idx_b), d, subsets, m,
           int(skip_diag), ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream())
    return out


# ---- Inception Score on the same main loop (csrc/metrics.hip): thin calls; metrics.py holds the definition -------------
def pairset_softmax_workspace_bytes(n: int, classes: int, d: int, splits: int) -> int:
    """sp_pairset_softmax_workspace (host logic: works without a GPU); SempyrError with the library's message for n < splits."""
    out = ctypes.c_int64(0)
    L.call("sp_pairset_softmax_workspace", n, classes, d, splits, ctypes.byref(out))
    return int(out.value)


def _pairset_head(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, d: Optional[int]):
    a, w = _pairset_set(a), _pairset_set(w)
    require_gpu(bias)
    if bias.dtype != torch.float32 or bias.dim() != 1 or not bias.is_contiguous() or bias.shape[0] != w.shape[0]:
        raise L.SempyrError("pair-set softmax: the bias is a contiguous fp32 (%d,) tensor, got %s %s" % (w.shape[0], bias.dtype, tuple(bias.shape)))
    return a, w, bias, (a.shape[1] if d is None else d)


def pairset_lse(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, d: Optional[int] = None, workspace=None):
    """(lse, h), float64 (n,) each: the log-sum-exp of the logits a @ w.T + bias of every row and sum_c p log p of its softmax."""
    a, w, bias, d = _pairset_head(a, w, bias, d)
    n = a.shape[0]
    ws = _pairset_ws(workspace, pairset_softmax_workspace_bytes(n, w.shape[0], d, 1), a.device)
    lse = torch.empty(n, dtype=torch.float64, device=a.device)
    h = torch.empty(n, dtype=torch.float64, device=a.device)
    L.call("sp_pairset_lse", ptr(a), n, a.shape[1], ptr(w), w.shape[0], w.shape[1], ptr(bias), d, ptr(lse), ptr(h), ptr(ws),
           ws.numel() * ws.element_size(), stream())
    return lse, h


def pairset_softmax_colsum(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, lse: torch.Tensor, h: torch.Tensor, splits: int,
                           d: Optional[int] = None, workspace=None):
    """(colsum, kl), float64 (splits, classes) and (splits,): per split the column sums of the softmax and its KL; lse, h: pairset_lse's."""
    a, w, bias, d = _pairset_head(a, w, bias, d)
    n, classes = a.shape[0], w.shape[0]
    for v in (lse, h):
        if v.dtype != torch.float64 or not v.is_cuda or not v.is_contiguous() or v.numel() != n:
            raise L.SempyrError("pair-set softmax: lse and h are contiguous float64 (%d,) device tensors" % n)
    ws = _pairset_ws(workspace, pairset_softmax_workspace_bytes(n, classes, d, splits), a.device)
    colsum = torch.empty((splits, classes), dtype=torch.float64, device=a.device)
    kl = torch.empty(splits, dtype=torch.float64, device=a.device)
    L.call("sp_pairset_softmax_colsum", ptr(a), n, a.shape[1], ptr(w), classes, w.shape[1], ptr(bias), d, ptr(lse), ptr(h), splits,
           ptr(colsum), ptr(kl), ptr(ws), ws.numel() * ws.element_size(), stream())
    return colsum, kl


# ---- reconstruction fidelity (csrc/reconstruction.hip): thin calls; reconstruction.py holds the scores -------------------
def ssim_workspace_bytes(n: int, c: int, h: int, w: int, scales: int) -> int:
    """sp_ssim_workspace (host logic: works without a GPU); SempyrError with the library's message for a shape the kernel refuses."""
    out = ctypes.c_int64(0)
    L.call("sp_ssim_workspace", n, c, h, w, scales, ctypes.byref(out))
    return int(out.value)


def ssim_stats(x: torch.Tensor, y: torch.Tensor, scales: int = 1, data_range: float = 2.0, workspace: Optional[torch.Tensor] = None):
    """(ssim_mean, cs_mean, sqerr) of include/sempyr.h's sp_ssim_stats: float64 device tensors (n, c, scales), (n, c, scales) and (n, c).
    x, y: (n, c, h, w) batches of one shape on one GPU, any strides, each fp32, bf16 or fp16 (read as they are: no copy, no cast).
    workspace: a device tensor of at least ssim_workspace_bytes() bytes, 8-byte aligned (default: a fresh one); it is left holding the
    pooled planes and partial sums in the layout the header states."""
    with torch.no_grad():
        x, y = x.detach(), y.detach()
        require_gpu(x)
        if x.dim() != 4 or tuple(y.shape) != tuple(x.shape) or y.device != x.device:
            raise L.SempyrError("ssim_stats takes two (n, c, h, w) batches of one shape on one GPU, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        n, c, h, w = x.shape
        ws = _pairset_ws(workspace, ssim_workspace_bytes(n, c, h, w, scales), x.device)
        ssim_mean = torch.empty((n, c, scales), dtype=torch.float64, device=x.device)
        cs_mean = torch.empty((n, c, scales), dtype=torch.float64, device=x.device)
        sqerr = torch.empty((n, c), dtype=torch.float64, device=x.device)
        L.call("sp_ssim_stats", ptr(x), sp_dtype(x.dtype), *x.stride(), ptr(y), sp_dtype(y.dtype), *y.stride(), n, c, h, w, scales,
               float(data_range), ptr(ssim_mean), ptr(cs_mean), ptr(sqerr), ptr(ws), ws.numel() * ws.element_size(), stream())
    return ssim_mean, cs_mean, sqerr
