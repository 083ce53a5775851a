"""Gradient clipping by global norm (csrc/optim.hip: sp_grad_sqnorm_multi, sp_grad_clip_finalize, sp_adam_multi_clipped) restated in numpy:
the fp64 sum of squares per chunk, the finalize state machine, and "a clipped Adam step is the plain Adam step on fp32(g * coefficient)".
tests/test_clip_host.py holds this restatement to torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64; tests/test_gpu_clip.py
holds the kernels to it.

Exact operands: integer-valued fp32 gradients with |g| <= 1024 in at most 2^20 elements.  Every square is an integer <= 2^20, every partial
sum an integer < 2^40 < 2^53: an exact fp64 number in ANY order of addition, so the kernel's order does not enter the comparison."""
import math

import numpy as np

MAX_ABS, MAX_ELEMENTS = 1024, 1 << 20
CHUNK = 65536
EPS_NORM = 1e-6                         # torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6)
SIZES = (1, 7, 4096, 70000)             # the tensors of the step tests: one element, a scalar tail, whole float4s, two chunks


def assert_exact_operands(arrays):
    """The premises of the exact comparisons, over ALL arrays that enter one sum."""
    total = 0
    for g in arrays:
        g = np.asarray(g)
        assert g.dtype == np.float32
        assert bool(np.all(g == np.rint(g))), "integer-valued gradients"
        assert g.size == 0 or float(np.abs(g).max()) <= MAX_ABS
        total += g.size
    assert total <= MAX_ELEMENTS


def integer_gradients(n, seed, scale=MAX_ABS):
    """n integer-valued fp32 values in [-scale, scale], zeros and both signs among them wherever n allows."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-scale, scale + 1, size=n).astype(np.float32)
    if n >= 3:
        g[n // 2] = 0.0
        g[0], g[-1] = -float(scale), float(scale)
    assert_exact_operands([g])
    return g


def real_gradients(n, seed):
    """normal x 1e-3 in fp32: the inexact case (tests bound it, they do not compare it exactly)."""
    return (np.random.default_rng(seed).standard_normal(n) * 1e-3).astype(np.float32)


def sqnorm(g):
    """sum (double)g[i]^2 - numpy's pairwise order; exact for assert_exact_operands' inputs, whatever the order."""
    g64 = np.asarray(g, dtype=np.float64)
    return float(np.sum(g64 * g64))


def sqnorm_fsum(g):
    """The same sum correctly rounded (math.fsum over the exact fp64 products): the reference of the real-valued case."""
    g64 = np.asarray(g, dtype=np.float64)
    return math.fsum((g64 * g64).tolist())


def chunks(n, chunk=CHUNK):
    """(offset, length) of the host's split of an n-element tensor."""
    return [(lo, min(chunk, n - lo)) for lo in range(0, n, chunk)]


def coefficient64(total, max_norm):
    """The clip coefficient in fp64, BEFORE its one rounding to fp32: min(1, max_norm / (sqrt(total) + 1e-6))."""
    return min(1.0, float(np.float64(max_norm) / (np.sqrt(np.float64(total)) + np.float64(EPS_NORM))))


def finalize(state, partials, max_norm):
    """sp_grad_clip_finalize: state = [norm, coefficient, skip flag, steps skipped, steps clipped] (fp32 values as Python floats) ->
    the state after one call.  The partials are added in fp64 (math.fsum: exact for integer-valued partials; callers with other
    values bound the result instead)."""
    assert max_norm > 0.0
    partials = [float(x) for x in np.asarray(partials, dtype=np.float64).ravel()]
    total = math.fsum(partials) if all(math.isfinite(x) for x in partials) else float(np.sum(np.asarray(partials)))
    out = [float(v) for v in state]
    with np.errstate(invalid="ignore", over="ignore"):
        out[0] = float(np.float32(np.sqrt(np.float64(total))))
    if not math.isfinite(total):
        out[1], out[2] = 0.0, 1.0
        out[3] += 1.0
        return out
    out[1] = float(np.float32(coefficient64(total, max_norm)))
    out[2] = 0.0
    if out[1] < 1.0:
        out[4] += 1.0
    return out


def scaled_gradient(g, coef, dtype=np.float32):
    """What the clipped step reads where the plain step reads g: ONE product in `dtype`, rounded once (Tensor.mul_)."""
    g = np.asarray(g, dtype=dtype)
    return (g * dtype(coef)).astype(dtype)


def adam_step64(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay=0.0):
    """torch/optim/adam.py's _single_tensor_adam (amsgrad = False) in float64, in its operation order; returns (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def clipped_adam_steps64(ps, grads_per_step, max_norm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """`len(grads_per_step)` clipped steps over the tensors `ps`, everything in float64: per step the GLOBAL norm over all tensors, the
    coefficient, and the plain Adam step on g * coefficient.  Returns (parameters, [(norm, coefficient64)] per step)."""
    ps = [np.asarray(p, dtype=np.float64) for p in ps]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    log = []
    for step, grads in enumerate(grads_per_step, 1):
        total = math.fsum(sqnorm_fsum(g) for g in grads)
        coef = coefficient64(total, max_norm)
        log.append((math.sqrt(total), coef))
        for i, g in enumerate(grads):
            ps[i], ms[i], vs[i] = adam_step64(ps[i], scaled_gradient(g, coef, np.float64), ms[i], vs[i], step, lr, betas[0], betas[1], eps,
                                              weight_decay)
    return ps, log
