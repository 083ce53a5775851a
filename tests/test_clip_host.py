"""Host side of gradient clipping by global norm (optim.Adam(max_grad_norm=...), ModelWrapper(clip_grad_norm=...), SP_CLIP_GRAD_NORM,
sp_grad_sqnorm_multi / sp_grad_clip_finalize / sp_adam_multi_clipped): the ABI, the refusals that come before any launch, argument
validation, and the numpy restatement (tests/clip_restated.py) held to torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64.
Nothing here needs a GPU (tests/test_gpu_clip.py has the rest).

Bounds.  Norm and coefficient (before its fp32 rounding) against torch in float64: 1e-12 relative - both sides evaluate the same
expression in float64 and differ in the ORDER of at most 74 104 additions of non-negative terms (n * 2^-53 = 8e-12 is the worst case of
a sequential sum; torch's and numpy's pairwise / vectorised sums and math.fsum stay some 1e-16 apart).  Parameters after three float64
Adam steps: 1e-9 of max(|p|, lr) - the quotient m / (sqrt(v) + eps) amplifies a 1e-12 relative change of the gradient by at most
|g| / (sqrt(v_hat) + eps) <= 1 / sqrt(1 - beta2) ~ 32 per step, times lr."""
import ctypes
import math

import numpy as np
import pytest
import torch

import clip_restated as C
import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, config, optim

INF, NAN = float("inf"), float("nan")
NAMES = ("sp_grad_sqnorm_multi", "sp_grad_clip_finalize", "sp_adam_multi_clipped")


def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    P, I, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert protos["sp_grad_sqnorm_multi"][1] == [P, I, P, P]
    assert protos["sp_grad_clip_finalize"][1] == [P, I, D, P, P]
    assert protos["sp_adam_multi_clipped"][1] == [P, I, D, D, D, D, P, P, P]
    assert protos["sp_adam_multi_guarded"][1] == [P, I, D, D, D, D, P, P]          # the neighbours keep their prototypes
    assert protos["sp_adam_multi"][1] == [P, I, D, D, D, D, P]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name


def test_argument_errors_return_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()                          # never dereferenced: the errors come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert ctypes.addressof(buf) % 8 == 0
    for bad in (0.0, -1.0, NAN, -INF):
        assert lib.sp_grad_clip_finalize(p, 1, bad, p, None) != 0, bad
        assert b"sp_grad_clip_finalize" in lib.sp_last_error_string()
    assert lib.sp_grad_clip_finalize(None, 1, 1.0, p, None) != 0
    assert lib.sp_grad_clip_finalize(p, 1, 1.0, None, None) != 0
    assert lib.sp_grad_clip_finalize(p, 0, 1.0, p, None) != 0
    assert lib.sp_grad_sqnorm_multi(None, 1, p, None) != 0
    assert b"sp_grad_sqnorm_multi" in lib.sp_last_error_string()
    assert lib.sp_grad_sqnorm_multi(p, 1, None, None) != 0
    assert lib.sp_grad_sqnorm_multi(p, 0, p, None) != 0
    hyper = (0.9, 0.999, 1e-8, 0.0)
    assert lib.sp_adam_multi_clipped(None, 1, *hyper, None, p, None) != 0
    assert b"sp_adam_multi_clipped" in lib.sp_last_error_string()
    assert lib.sp_adam_multi_clipped(p, 1, *hyper, None, None, None) != 0          # the clip state is required here
    assert lib.sp_adam_multi_clipped(p, 0, *hyper, None, p, None) != 0
    with pytest.raises(_lib.SempyrError):
        _lib.call("sp_grad_clip_finalize", p, 1, 0.0, p, None)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_operand_builders_assert_their_premises():
    for n in (1, 3, 4, 255, 65536):
        g = C.integer_gradients(n, n)
        assert g.dtype == np.float32 and g.shape == (n,)
        if n >= 3:
            assert (g == 0).any() and (g < 0).any() and (g > 0).any()
    with pytest.raises(AssertionError):
        C.assert_exact_operands([np.array([0.5], dtype=np.float32)])
    with pytest.raises(AssertionError):
        C.assert_exact_operands([np.array([1025.0], dtype=np.float32)])
    with pytest.raises(AssertionError):
        C.assert_exact_operands([np.zeros(C.MAX_ELEMENTS, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    with pytest.raises(AssertionError):
        C.assert_exact_operands([np.zeros(3, dtype=np.float64)])
    # the premise's consequence: the worst case stays an exact fp64 integer, in any order
    worst = np.full(C.MAX_ELEMENTS, float(C.MAX_ABS), dtype=np.float32)
    assert C.sqnorm(worst) == C.sqnorm_fsum(worst) == float(C.MAX_ELEMENTS * C.MAX_ABS ** 2) < 2.0 ** 53
    g = C.integer_gradients(70000, 3)
    assert C.sqnorm(g) == C.sqnorm(g[::-1]) == C.sqnorm_fsum(g) == float(sum(int(x) ** 2 for x in g))
    assert C.chunks(70000) == [(0, 65536), (65536, 4464)] and C.chunks(1) == [(0, 1)] and C.chunks(65536) == [(0, 65536)]


def test_finalize_state_machine():
    st = [7.0, 7.0, 1.0, 2.0, 3.0]
    st = C.finalize(st, [9.0, 16.0], max_norm=10.0)                       # norm 5 below 10
    assert st == [5.0, 1.0, 0.0, 2.0, 3.0]
    st = C.finalize(st, [9.0, 16.0], max_norm=2.5)                        # above: 2.5 / (5 + 1e-6)
    assert st[0] == 5.0 and st[2:] == [0.0, 2.0, 4.0]
    assert st[1] == float(np.float32(2.5 / (5.0 + 1e-6))) and 0.4999 < st[1] < 0.5
    st = C.finalize(st, [9.0, 16.0], max_norm=INF)
    assert st == [5.0, 1.0, 0.0, 2.0, 4.0]
    st = C.finalize(st, [9.0, INF], max_norm=INF)
    assert st[0] == INF and st[1:] == [0.0, 1.0, 3.0, 4.0]
    st = C.finalize(st, [NAN, 1.0], max_norm=1.0)
    assert math.isnan(st[0]) and st[1:] == [0.0, 1.0, 4.0, 4.0]
    st = C.finalize(st, [0.0], max_norm=1.0)                              # a clean call clears the flag and keeps the counts
    assert st == [0.0, 1.0, 0.0, 4.0, 4.0]
    assert C.finalize(st, list(range(1000)), max_norm=INF)[0] == float(np.float32(math.sqrt(499500.0)))
    with pytest.raises(AssertionError):
        C.finalize(st, [1.0], max_norm=0.0)


def test_scaling_by_one_is_the_identity_and_rounds_once():
    g = C.real_gradients(4096, 1)
    assert C.scaled_gradient(g, 1.0).tobytes() == g.tobytes()
    c = float(np.float32(0.3))
    want = (g.astype(np.float64) * np.float64(np.float32(c))).astype(np.float32)      # the exact product, rounded once
    assert C.scaled_gradient(g, c).tobytes() == want.tobytes()


def _torch_reference(ps, grads_per_step, max_norm, lr, betas, eps, weight_decay):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64 over the same tensors; returns (parameters, [(norm, coefficient)])."""
    params = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float64)).clone()) for p in ps]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    log = []
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(np.asarray(g, dtype=np.float64)).clone()
        before = [p.grad.clone() for p in params]
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        # the coefficient torch applied, read back from the largest gradient element
        i = max(range(len(params)), key=lambda k: float(before[k].abs().max()))
        j = int(before[i].abs().argmax())
        log.append((norm, float(params[i].grad.reshape(-1)[j] / before[i].reshape(-1)[j])))
        opt.step()
    return [p.detach().numpy() for p in params], log


@pytest.mark.parametrize("kind", ["integer", "real"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_restatement_against_torch_in_float64(kind, weight_decay):
    """Three steps on tensors of 1, 7, 4 096 and 70 000 elements; the thresholds are chosen so that steps clip and do not clip."""
    rng = np.random.default_rng(0)
    ps = [rng.standard_normal(n) for n in C.SIZES]
    make = (lambda n, s: C.integer_gradients(n, s, scale=4 + 300 * (s % 3))) if kind == "integer" else C.real_gradients
    grads = [[make(n, 10 * step + i) for i, n in enumerate(C.SIZES)] for step in range(3)]
    norms = [math.sqrt(math.fsum(C.sqnorm_fsum(g) for g in gs)) for gs in grads]
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    seen = set()
    for max_norm in (sorted(norms)[1], 0.25 * min(norms), INF):
        got_p, got_log = C.clipped_adam_steps64(ps, grads, max_norm, **hyper)
        want_p, want_log = _torch_reference(ps, grads, max_norm, **hyper)
        clipped = 0
        for (norm, coef), (tnorm, tcoef), exact in zip(got_log, want_log, norms):
            assert abs(norm - tnorm) <= 1e-12 * tnorm, (max_norm, norm, tnorm)
            assert abs(coef - tcoef) <= 1e-12 * tcoef + 4e-16, (max_norm, coef, tcoef)      # (+ the read-back quotient's own rounding)
            assert norm == exact
            clipped += int(coef < 1.0)
        assert clipped == sum(1 for nm in norms if max_norm / (nm + 1e-6) < 1.0), (max_norm, got_log)
        seen.add(clipped)
        for a, b in zip(got_p, want_p):
            assert float(np.abs(a - b).max()) <= 1e-9 * max(float(np.abs(b).max()), hyper["lr"])
    assert 0 in seen and 3 in seen and len(seen) == 3, seen                   # never, sometimes and always clipped
    # the state machine's coefficient is the float64 one rounded once
    parts = [C.sqnorm(g) for g in grads[0]]
    st = C.finalize([0.0] * 5, parts, 0.25 * min(norms))
    assert st[1] == float(np.float32(C.coefficient64(math.fsum(parts), 0.25 * min(norms)))) and st[4] == 1.0


# ---- argument validation ------------------------------------------------------------------------------------------------------------
def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_adam_max_grad_norm_validation():
    assert optim.Adam(_params()).max_grad_norm is None
    assert optim.Adam(_params(), max_grad_norm=None).max_grad_norm is None
    assert optim.Adam(_params(), max_grad_norm=2).max_grad_norm == 2.0
    assert optim.Adam(_params(), max_grad_norm=0.5).max_grad_norm == 0.5
    assert optim.Adam(_params(), max_grad_norm=INF).max_grad_norm == INF
    for bad in (True, False, NAN, 0, 0.0, -1.0, -INF, "1.0", [1.0]):
        with pytest.raises(_lib.SempyrError):
            optim.Adam(_params(), max_grad_norm=bad)
    opt = optim.Adam(_params())
    with pytest.raises(_lib.SempyrError):
        opt.max_grad_norm = -2.0
    assert opt.max_grad_norm is None


def test_adam_keeps_the_setting_out_of_defaults_groups_and_state_dict():
    plain, on = optim.Adam(_params(), lr=1e-4), optim.Adam(_params(), lr=1e-4, max_grad_norm=1.0)
    ref = torch.optim.Adam(_params(), lr=1e-4, foreach=False, fused=False)
    assert set(on.defaults) == set(plain.defaults) == set(ref.defaults)
    assert set(on.param_groups[0]) == set(plain.param_groups[0]) == set(ref.param_groups[0])
    assert "max_grad_norm" not in on.defaults and "max_grad_norm" not in on.param_groups[0]
    sd_on, sd_ref = on.state_dict(), ref.state_dict()
    assert set(sd_on) == set(sd_ref) == {"state", "param_groups"}
    assert set(sd_on["param_groups"][0]) == set(sd_ref["param_groups"][0])
    ref.load_state_dict(sd_on)                                            # torch's Adam reads what this one writes
    # off: no state tensor, and the attributes that hand it out do not exist
    assert plain._clip is None and on._clip is None                       # (on: allocated by the first step, on the GPU)
    for name in ("clip_state", "grad_norm", "skip_flag"):
        assert not hasattr(plain, name), name
    assert not any(isinstance(v, torch.Tensor) for v in vars(plain).values())


def test_config_parses_sp_clip_grad_norm(monkeypatch):
    monkeypatch.delenv("SP_CLIP_GRAD_NORM", raising=False)
    assert config.Config.from_env().clip_grad_norm == 0.0 and config.Config().clip_grad_norm == 0.0
    for text, want in (("", 0.0), ("0", 0.0), ("0.0", 0.0), ("1", 1.0), ("2.5", 2.5), ("inf", INF), (" 10 ", 10.0)):
        monkeypatch.setenv("SP_CLIP_GRAD_NORM", text)
        assert config.Config.from_env().clip_grad_norm == want, text
    for text in ("-1", "nan", "-inf", "off"):
        monkeypatch.setenv("SP_CLIP_GRAD_NORM", text)
        with pytest.raises(ValueError):
            config.Config.from_env()


def _networks():
    return sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8)


def test_wrapper_without_the_switch_is_what_it_was():
    assert config.CFG.clip_grad_norm == 0.0, "this test needs SP_CLIP_GRAD_NORM unset"
    G, D = _networks()
    og, od = optim.Adam(G.parameters(), lr=1e-5), optim.Adam(D.parameters(), lr=1e-5)
    keys = (list(G.state_dict()), list(D.state_dict()), og.state_dict()["param_groups"], od.state_dict()["param_groups"])
    for value in (None, 0, 0.0):
        mw = sp.ModelWrapper(G, D, None, None, generator_optimizer=og, discriminator_optimizer=od, save_data_path=None, clip_grad_norm=value)
        assert mw.clip_grad_norm is None
        assert "clip_grad_norm" not in mw.logger.hyperparameter
        assert og.max_grad_norm is None and od.max_grad_norm is None
        assert not hasattr(mw, "_grad_norm")
        assert not any(isinstance(v, torch.Tensor) for v in vars(mw).values())
        assert mw._with_grad_norms({"a": 1}) == {"a": 1}
    assert (list(G.state_dict()), list(D.state_dict()), og.state_dict()["param_groups"], od.state_dict()["param_groups"]) == keys


def test_wrapper_validates_and_arms_the_optimizers(monkeypatch):
    G, D = _networks()
    for bad in (True, False, NAN, -1.0, -INF, "1"):
        with pytest.raises(_lib.SempyrError):
            sp.ModelWrapper(G, D, None, None, save_data_path=None, clip_grad_norm=bad)
    og, od = optim.Adam(G.parameters(), lr=1e-5), torch.optim.Adam(D.parameters(), lr=1e-5)
    sd_g, sd_d = list(G.state_dict()), list(D.state_dict())
    mw = sp.ModelWrapper(G, D, None, None, generator_optimizer=og, discriminator_optimizer=od, save_data_path=None, clip_grad_norm=INF)
    assert mw.clip_grad_norm == INF and og.max_grad_norm == INF
    assert mw.logger.hyperparameter["clip_grad_norm"] == "inf"
    assert not hasattr(od, "max_grad_norm")                                # a foreign optimizer is left as it is
    assert (list(G.state_dict()), list(D.state_dict())) == (sd_g, sd_d)
    assert set(og.state_dict()) == {"state", "param_groups"}
    # the same value again is fine, another one is a contradiction
    sp.ModelWrapper(G, D, None, None, generator_optimizer=og, save_data_path=None, clip_grad_norm=INF)
    with pytest.raises(_lib.SempyrError):
        sp.ModelWrapper(G, D, None, None, generator_optimizer=og, save_data_path=None, clip_grad_norm=3.0)
    # the environment's way in (main.py passes fixed keywords)
    monkeypatch.setattr(config.CFG, "clip_grad_norm", 2.0)
    o2 = optim.Adam(G.parameters(), lr=1e-5)
    mw = sp.ModelWrapper(G, D, None, None, generator_optimizer=o2, save_data_path=None)
    assert mw.clip_grad_norm == 2.0 and o2.max_grad_norm == 2.0 and mw.logger.hyperparameter["clip_grad_norm"] == "2.0"
