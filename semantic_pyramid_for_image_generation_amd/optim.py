"""Multi-tensor Adam on the HIP path, and `ParameterEMA`: an exponential moving average of a network's parameters
in one flat device buffer, updated by one launch behind the optimizer step and evaluated by exchanging it with the parameters in place.

`Adam` IS a torch.optim.Adam (same constructor, param_groups, per-parameter state {step, exp_avg, exp_avg_sq} and
state_dict, so checkpoints written by the reference - model_wrapper.py:215-223 - load unchanged); only `.step()` is
replaced: every parameter of a group is updated by ONE launch of sp_adam_multi instead of torch's foreach kernels.
There is no fallback: parameters must be fp32 on the GPU, amsgrad / maximize / capturable are rejected.

Host cost: the chunk table (pointers, lengths) of a group is built ONCE per set of (parameter, gradient, moment) addresses and
cached; a step only refreshes the two bias-correction columns with vectorised numpy and uploads the table through pinned
memory.  The per-parameter ``state['step']`` tensors torch keeps are brought up to date lazily (state_dict(), or whenever the
cached plan is dropped) - round 1 incremented 286 CPU tensors and rebuilt the table every call (~5 ms of Python per step).
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _lib as L
from .ops import ptr, stream

CHUNK = 65536
_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("step_size", "<f4"),
                ("inv_sqrt_bc2", "<f4"), ("reserved", "<f4")])
_EMA_DT = np.dtype([("avg", "<u8"), ("p", "<u8"), ("n", "<i4"), ("reserved", "<i4")])       # sp_ema_chunk (include/sempyr.h)


class _Plan:
    __slots__ = ("key", "params", "keep", "table", "idx", "steps", "total", "synced")


def check_max_grad_norm(value, what="max_grad_norm"):
    """None (off), or the clipping threshold as a float: > 0, +inf allowed ("monitor and guard, never scale").  bool, NaN and values <= 0
    are errors - 0 is not "off" here, that is spelled None."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise L.SempyrError("%s takes None or a number > 0 (inf allowed), got %r" % (what, value))
    value = float(value)
    if not value > 0.0:                                   # NaN fails this too
        raise L.SempyrError("%s must be > 0 (inf allowed), got %r" % (what, value))
    return value


class Adam(torch.optim.Adam):
    """``max_grad_norm`` (beyond torch.optim.Adam; None = off: exactly the launches above and no state tensor): clip the gradients by
    their GLOBAL norm over all of this optimizer's groups - torch.nn.utils.clip_grad_norm_'s definition - and skip the step when that norm
    is not finite, all on the device.  A step is then: every group's chunk table, one sp_grad_sqnorm_multi per group into one partials
    buffer, ONE sp_grad_clip_finalize, one sp_adam_multi_clipped per group.  The gradients are read twice and never written: the
    step uses fp32(g * coefficient).  ``clip_state`` is the five-float device state {norm, coefficient, skip flag, steps skipped, steps
    clipped} (include/sempyr.h: sp_grad_clip_finalize), ``grad_norm`` and ``skip_flag`` are views of its [0] and [2]; nothing is read on
    the host.  It is no entry of ``defaults`` / ``param_groups`` / ``state_dict()``: checkpoints stay what torch.optim.Adam reads and
    writes.  (As with ``found_inf``, the host-side step count that feeds the bias corrections still advances on a skipped step.)"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None, **kw):
        if amsgrad or kw.get("maximize") or kw.get("capturable") or kw.get("differentiable"):
            raise L.SempyrError("sempyr Adam supports the reference's configuration only (no amsgrad / maximize / capturable)")
        max_grad_norm = check_max_grad_norm(max_grad_norm)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False, fused=False)
        self._ring = {}            # per group: two pinned host tables + the event of their last upload
        self._plans = {}           # per group: cached chunk table
        self._max_grad_norm = max_grad_norm
        self._clip = None          # max_grad_norm only: [state (5 floats), partials (fp64, one per chunk)] on the parameters' device

    # ------------------------------------------------------------------------------------------ gradient clipping
    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value) -> None:
        self._max_grad_norm = check_max_grad_norm(value)
        if self._max_grad_norm is None:
            self._clip = None

    def _clip_buffers(self, n_partials=0):
        """[state, partials]: allocated once on the device of the first parameter, the partials grown only when the chunk count does."""
        if self._max_grad_norm is None:
            raise AttributeError("this Adam has no gradient clipping state (max_grad_norm is None)")
        if self._clip is None:
            dev = self.param_groups[0]["params"][0].device
            if dev.type != "cuda":
                raise L.SempyrError("sempyr Adam needs contiguous fp32 GPU parameters (got %s)" % (dev,))
            self._clip = [torch.zeros(5, dtype=torch.float32, device=dev), torch.zeros(max(n_partials, 1024), dtype=torch.float64, device=dev)]
        if self._clip[1].numel() < n_partials:
            self._clip[1] = torch.zeros(n_partials, dtype=torch.float64, device=self._clip[0].device)
        return self._clip

    @property
    def clip_state(self) -> torch.Tensor:
        return self._clip_buffers()[0]

    @property
    def grad_norm(self) -> torch.Tensor:
        return self._clip_buffers()[0][0]

    @property
    def skip_flag(self) -> torch.Tensor:
        return self._clip_buffers()[0][2]

    # ------------------------------------------------------------------------------------------ step bookkeeping
    def _sync_steps(self) -> None:
        """Writes the step counts the cached plans hold into torch's per-parameter ``state['step']`` tensors."""
        for plan in self._plans.values():
            if plan is not None and not plan.synced:
                for p, t in zip(plan.params, plan.steps):
                    self.state[p]["step"].fill_(float(t))
                plan.synced = True

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._plans = {}
        return super().load_state_dict(state_dict)

    def _build_plan(self, gi, group, key) -> _Plan:
        self._sync_steps()
        ps, gs, ms, vs, ns, steps, plist, keep = [], [], [], [], [], [], [], []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise L.SempyrError("sempyr Adam needs contiguous fp32 GPU parameters (got %s %s)" % (p.device, p.dtype))
            if g.is_sparse:
                raise L.SempyrError("sempyr Adam does not support sparse gradients")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            plist.append(p)
            ps.append(p.data_ptr()); gs.append(g.data_ptr()); ms.append(st["exp_avg"].data_ptr()); vs.append(st["exp_avg_sq"].data_ptr())
            ns.append(p.numel())
            steps.append(float(st["step"]))
        plan = _Plan()
        plan.key, plan.params, plan.keep = key, plist, keep
        plan.steps = np.asarray(steps, dtype=np.float64)
        plan.synced = True
        if not ps:
            plan.total, plan.table, plan.idx = 0, None, None
            return plan
        n = np.asarray(ns, dtype=np.int64)
        reps = (n + CHUNK - 1) // CHUNK
        total = int(reps.sum())
        idx = np.repeat(np.arange(len(ns)), reps)                          # tensor of each chunk
        first = np.cumsum(reps) - reps
        off = (np.arange(total) - first[idx]) * CHUNK                      # element offset of each chunk in its tensor
        tab = np.zeros(total, dtype=_DT)
        byte_off = (off * 4).astype(np.uint64)
        tab["p"] = np.asarray(ps, dtype=np.uint64)[idx] + byte_off
        tab["g"] = np.asarray(gs, dtype=np.uint64)[idx] + byte_off
        tab["m"] = np.asarray(ms, dtype=np.uint64)[idx] + byte_off
        tab["v"] = np.asarray(vs, dtype=np.uint64)[idx] + byte_off
        tab["n"] = np.minimum(n[idx] - off, CHUNK).astype(np.int32)
        plan.total, plan.table, plan.idx = total, tab, idx
        return plan

    def _prepare(self, gi, group):
        """One group's share of a step in front of its launches: the cached chunk table (re)built, the step counts advanced, the two
        bias-correction columns refreshed and the table uploaded.  Returns (plan, device table) or None where no parameter has a gradient."""
        if group.get("amsgrad") or group.get("maximize"):
            raise L.SempyrError("sempyr Adam: amsgrad / maximize are not supported")
        lr, (b1, b2) = float(group["lr"]), group["betas"]
        # the plan stays valid while every parameter keeps its gradient (and moment) storage: true for the flat gradient
        # buffers of the training step and for captured graphs; fp32 / contiguity are checked when a plan is built
        key = tuple((p.data_ptr(), g.data_ptr(), g.dtype == torch.float32 and g.is_contiguous())
                    for p in group["params"] for g in (p.grad,) if g is not None)
        plan = self._plans.get(gi)
        if plan is None or plan.key != key:
            if any(not k[2] for k in key):
                raise L.SempyrError("sempyr Adam needs contiguous fp32 gradients")
            plan = self._plans[gi] = self._build_plan(gi, group, key)
        if plan.total == 0:
            return None
        plan.steps += 1.0
        plan.synced = False
        tab = plan.table
        tab["step_size"] = (lr / (1.0 - b1 ** plan.steps)).astype(np.float32)[plan.idx]
        tab["inv_sqrt_bc2"] = (1.0 / np.sqrt(1.0 - b2 ** plan.steps)).astype(np.float32)[plan.idx]
        dev = plan.params[0].device
        with torch.cuda.device(dev):
            # the chunk table goes up through pinned memory (a pageable copy would make the host wait for the stream);
            # two tables alternate and each waits for its own previous upload before it is overwritten
            ring = self._ring.setdefault(gi, {"i": 0, "slots": [None, None]})
            ring["i"] ^= 1
            slot = ring["slots"][ring["i"]]
            nbytes = tab.nbytes
            if slot is None or slot[0].numel() < nbytes:
                slot = [torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True), None]
                ring["slots"][ring["i"]] = slot
            if slot[1] is not None:
                slot[1].synchronize()
            slot[0][:nbytes].numpy()[:] = tab.view(np.uint8)
            tab_dev = slot[0][:nbytes].to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            slot[1] = ev
        return plan, tab_dev

    @staticmethod
    def _hyper(group):
        (b1, b2) = group["betas"]
        return float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])

    @torch.no_grad()
    def step(self, closure=None, found_inf=None):
        """found_inf (optional, the fp16 mode's ops.LossScaler): a device float; the launch updates NOTHING when it is non-zero
        (sp_adam_multi_guarded) - the step is skipped on the device, without a host sync.  (The host-side step count that feeds the
        bias corrections still advances on a skipped step; torch's fused Adam takes it back.)

        With ``max_grad_norm``: the tables of ALL groups first, then one sp_grad_sqnorm_multi per group, ONE sp_grad_clip_finalize over
        all of them (the norm is global, as clip_grad_norm_ over every parameter is) and one sp_adam_multi_clipped per group, which
        also does nothing when the norm is not finite - found_inf is passed through as before.  The same wart again: the host-side step
        count advances on a step the device skipped."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._max_grad_norm is None:
            for gi, group in enumerate(self.param_groups):
                ready = self._prepare(gi, group)
                if ready is None:
                    continue
                plan, tab_dev = ready
                with torch.cuda.device(plan.params[0].device):
                    if found_inf is not None:
                        L.call("sp_adam_multi_guarded", ptr(tab_dev), plan.total, *self._hyper(group), found_inf, stream())
                    else:
                        L.call("sp_adam_multi", ptr(tab_dev), plan.total, *self._hyper(group), stream())
            return loss
        ready = [(group, r) for group, r in ((group, self._prepare(gi, group)) for gi, group in enumerate(self.param_groups)) if r is not None]
        if not ready:
            return loss
        state, partials = self._clip_buffers(sum(plan.total for _, (plan, _) in ready))
        if any(plan.params[0].device != state.device for _, (plan, _) in ready):
            raise L.SempyrError("sempyr Adam: max_grad_norm needs every parameter group on one device (the norm is global)")
        with torch.cuda.device(state.device):
            first = 0
            for _, (plan, tab_dev) in ready:
                L.call("sp_grad_sqnorm_multi", ptr(tab_dev), plan.total, ctypes.c_void_p(partials.data_ptr() + 8 * first), stream())
                first += plan.total
            L.call("sp_grad_clip_finalize", ptr(partials), first, self._max_grad_norm, ptr(state), stream())
            for group, (plan, tab_dev) in ready:
                L.call("sp_adam_multi_clipped", ptr(tab_dev), plan.total, *self._hyper(group), found_inf, ptr(state), stream())
        return loss


class ParameterEMA:
    """Exponential moving average of ``module``'s parameters on the device: avg += (p - avg) * (1 - decay) after every optimizer step.
    The reference has no average of its own (it scores, samples and saves the last iterate: model_wrapper.py:231-296, :215-223); a
    SAGAN-family generator trained at lr 1e-5 and batch 20 is normally evaluated from one.

    There is no second network.  The average lives in ONE flat fp32 buffer (a window per parameter, in ``named_parameters()`` order,
    each at an offset padded to 4 floats so that it is 16-byte aligned), and it is evaluated by exchanging its values with the
    parameters' IN PLACE (`swap`, `applied`): no address changes, so captured graphs, Adam's cached chunk tables and the flat gradient
    buffer stay valid, and the spectral-norm bank re-packs from ``weight_orig`` in every forward anyway.

    What is averaged: the parameters, nothing else.  What is not: the buffers.  In eval mode a spectral-norm layer's sigma is
    computed from the LIVE ``weight_u`` / ``weight_v`` against the averaged ``weight_orig`` (the power iteration tracks the raw
    weights, a few 1e-5 steps away), and the BatchNorm running statistics (momentum 0.001) are slow averages already.

    Host cost: the chunk table (pointers and lengths only - `sp_ema_chunk`) is built and uploaded once, and again only when a
    parameter's ``data_ptr()`` or device changes; the buffer then follows the parameters to their device and keeps its values.
    Parameters must be contiguous fp32 on one GPU (`SempyrError` otherwise): there is no fallback."""

    def __init__(self, module, decay: float = 0.999, warmup: bool = False):
        named = [(n, p) for n, p in module.named_parameters()]
        if not named:
            raise L.SempyrError("ParameterEMA: the module has no parameters")
        self._params = [p for _, p in named]
        self._check_params()
        self._init_state([(n, tuple(p.shape)) for n, p in named], decay, warmup, self._params[0].device)

    def _init_state(self, named_shapes, decay, warmup, device) -> None:
        """Layout and storage (no kernel, no parameter is read): named_shapes = [(name, shape)] in named_parameters() order."""
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise L.SempyrError("ParameterEMA: decay must lie in [0, 1] (got %r)" % (decay,))
        self.decay, self.warmup, self.num_updates = decay, bool(warmup), 0
        self._names = [n for n, _ in named_shapes]
        self._shapes = [tuple(s) for _, s in named_shapes]
        self._numels = [int(np.prod(s, dtype=np.int64)) for s in self._shapes]
        offs, off = [], 0
        for n in self._numels:
            offs.append(off)
            off += (n + 3) // 4 * 4
        self._offsets = offs
        self.buffer = torch.zeros(max(off, 4), dtype=torch.float32, device=device)
        self._windows = self._make_windows()
        self._key, self._table_dev, self._total = None, None, 0
        self._swapped = False

    def _make_windows(self):
        return [self.buffer[o:o + n].view(s) for o, n, s in zip(self._offsets, self._numels, self._shapes)]

    def _check_params(self) -> None:
        dev = self._params[0].device
        for p in self._params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == dev):
                raise L.SempyrError("ParameterEMA needs contiguous fp32 parameters on one GPU (got %s %s)" % (p.device, p.dtype))

    def _plan(self):
        """The device chunk table; rebuilt (and the buffer moved) only when a parameter's address or device has changed."""
        key = tuple((p.data_ptr(), p.device) for p in self._params)
        if key != self._key:
            self._check_params()
            dev = self._params[0].device
            if self.buffer.device != dev:
                self.buffer = self.buffer.to(dev)
                self._windows = self._make_windows()
            n = np.asarray(self._numels, dtype=np.int64)
            reps = (n + CHUNK - 1) // CHUNK
            total = int(reps.sum())
            idx = np.repeat(np.arange(len(n)), reps)                           # tensor of each chunk
            first = np.cumsum(reps) - reps
            off = (np.arange(total) - first[idx]) * CHUNK                      # element offset of each chunk in its tensor
            tab = np.zeros(total, dtype=_EMA_DT)
            byte_off = (off * 4).astype(np.uint64)
            tab["avg"] = np.uint64(self.buffer.data_ptr()) + (np.asarray(self._offsets, dtype=np.uint64) * np.uint64(4))[idx] + byte_off
            tab["p"] = np.asarray([k[0] for k in key], dtype=np.uint64)[idx] + byte_off
            tab["n"] = np.minimum(n[idx] - off, CHUNK).astype(np.int32)
            self._total = total
            self._table_dev = torch.from_numpy(tab.view(np.uint8).copy()).to(dev) if total else None      # static: uploaded once
            self._key = key
        return self._table_dev, self._total

    # ------------------------------------------------------------------------------------------ update / swap
    @torch.no_grad()
    def update(self, found_inf=None) -> None:
        """Call after the optimizer step.  The FIRST call only initialises the average to the parameters it sees (one
        torch._foreach_copy_, no kernel); every later call is one sp_ema_multi launch on the current stream.  With ``warmup`` the
        decay in force is min(decay, (1 + n) / (10 + n)), n = ``num_updates``: the calls made so far.  found_inf (optional, as in
        `Adam.step`): a device float; the launch changes NOTHING when it is non-zero - the optimizer step it follows was skipped on
        the device.  (The host-side counter ``num_updates`` still advances on such a skipped step, as Adam's step count does.)"""
        if self._swapped:
            raise L.SempyrError("ParameterEMA.update(): the average is swapped into the parameters - swap back first")
        table, total = self._plan()
        n = self.num_updates
        self.num_updates = n + 1
        if n == 0:
            torch._foreach_copy_(self._windows, [p.detach() for p in self._params])
            return
        if total == 0:
            return
        decay = min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay
        with torch.cuda.device(self.buffer.device):
            L.call("sp_ema_multi", ptr(table), total, 1.0 - decay, found_inf, stream())

    def swap(self) -> None:
        """Exchanges the average and the parameters in place (one sp_swap_multi launch on the current stream); a second call puts
        both back bit for bit."""
        if self.num_updates == 0:
            raise L.SempyrError("ParameterEMA.swap(): the average has not been initialised (no update() yet, nothing loaded)")
        table, total = self._plan()
        if total:
            with torch.cuda.device(self.buffer.device):
                L.call("sp_swap_multi", ptr(table), total, stream())
        self._swapped = not self._swapped

    @property
    def swapped(self) -> bool:
        return self._swapped

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied(): ...`` - the module holds the average inside the block and its own parameters after it (also when the
        block raises).  Not re-entrant."""
        if self._swapped:
            raise L.SempyrError("ParameterEMA.applied(): already swapped in (nested use)")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ------------------------------------------------------------------------------------------ state
    def _average_tensors(self):
        """Where the average is right now: its windows, or - while swapped in - the parameters."""
        return [p.detach() for p in self._params] if self._swapped else self._windows

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "parameters": {n: t.clone() for n, t in zip(self._names, self._average_tensors())}}

    @torch.no_grad()
    def load_state_dict(self, state) -> None:
        """``state``: what `state_dict` returns.  ``state["parameters"]`` may also be a plain state dict of the module (a generator's,
        or `averaged_state_dict`'s): every parameter name must be there with its shape, buffers and other extra keys are ignored.
        ``decay`` / ``warmup`` / ``num_updates`` are taken where present; a loaded average counts as initialised."""
        if self._swapped:
            raise L.SempyrError("ParameterEMA.load_state_dict(): the average is swapped into the parameters - swap back first")
        tensors = state["parameters"]
        missing = [n for n in self._names if n not in tensors]
        if missing:
            raise L.SempyrError("ParameterEMA.load_state_dict(): missing parameters %s" % (missing[:5],))
        for n, s in zip(self._names, self._shapes):
            if tuple(tensors[n].shape) != s:
                raise L.SempyrError("ParameterEMA.load_state_dict(): %s has shape %s, expected %s" % (n, tuple(tensors[n].shape), s))
        decay = float(state.get("decay", self.decay))
        if not 0.0 <= decay <= 1.0:
            raise L.SempyrError("ParameterEMA.load_state_dict(): decay must lie in [0, 1] (got %r)" % (decay,))
        for n, w in zip(self._names, self._windows):
            w.copy_(tensors[n])
        self.decay, self.warmup = decay, bool(state.get("warmup", self.warmup))
        self.num_updates = max(1, int(state.get("num_updates", self.num_updates)))

    def averaged_state_dict(self, module):
        """``module.state_dict()`` with every parameter replaced by (a copy of) its average; the buffers are the live ones (weight_u /
        weight_v, BatchNorm running statistics, num_batches_tracked).  Loads straight into a Generator - this package's or the
        reference's."""
        out = module.state_dict()
        for n, t in zip(self._names, self._average_tensors()):
            if n not in out:
                raise L.SempyrError("ParameterEMA.averaged_state_dict(): the module has no parameter %s" % n)
            out[n] = t.clone()
        return out
