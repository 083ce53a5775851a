"""Gradient clipping by global norm on the GPU: sp_grad_sqnorm_multi, sp_grad_clip_finalize and sp_adam_multi_clipped through the C ABI
against the numpy restatement (tests/clip_restated.py), optim.Adam(max_grad_norm=...), and ModelWrapper(clip_grad_norm=...) in the
training step - eager and replayed, clipping, the foreign optimizer, and the non-finite guard in the bf16 and fp16 modes.

What is compared exactly and why: integer-valued gradients (|g| <= 1024, <= 2^20 elements) make every partial sum an exact fp64 integer
in any order (clip_restated's docstring), so the kernels' sums must EQUAL the float64 sums; the coefficient is then a correctly rounded
fp64 sqrt, add and divide rounded to fp32 once - its bits must equal numpy's; and the clipped step reads fp32(g * coefficient), one IEEE
product, so it must equal the plain kernel on gradients that torch.mul scaled in fp32, bit for bit.  Every buffer a kernel writes lies
between canaries."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_restated as C  # noqa: E402
import golden_util as gu  # noqa: E402
import semantic_pyramid_for_image_generation_amd as sp  # noqa: E402
from oracle import sempyr_oracle as O  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops, optim, params, synthetic  # noqa: E402

DEV = "cuda"
F32 = torch.float32
PAD = 64
SP_ERR_INVALID = -1
INF, NAN = float("inf"), float("nan")
_DT = optim._DT                                                    # sp_adam_chunk (include/sempyr.h)
LENGTHS = (1, 3, 4, 255, 1025, 65535, 65536)                       # one chunk each: tail only, float4 + tail, whole float4s, a full chunk
LOSS_NAMES = ("loss_discriminator_real", "loss_discriminator_fake", "loss_generator", "loss_generator_semantic_reconstruction",
              "loss_generator_diversity")
NORM_NAMES = ("grad_norm_discriminator", "grad_norm_generator")


@pytest.fixture(autouse=True)
def _reset():
    torch.cuda.set_device(0)
    yield
    ops.set_compute_dtype(torch.float32)
    ops.set_loss_scale(65536.0)


class Guarded:
    """[PAD canaries][n values][PAD canaries] on the device; .t is the body, `off` elements past a 16-byte boundary."""

    def __init__(self, body, off=0, canary=-1536.0):
        body = torch.as_tensor(body)
        self.n, self.off, self.canary = body.numel(), off, canary
        host = torch.full((PAD + off + self.n + PAD,), canary, dtype=body.dtype)
        host[PAD + off:PAD + off + self.n] = body.reshape(-1)
        self.buf = host.to(DEV)
        self.t = self.buf[PAD + off:PAD + off + self.n]
        assert self.buf[PAD:].data_ptr() % 16 == 0

    def host(self, what=""):
        h = self.buf.cpu()
        edge = torch.cat((h[:PAD + self.off], h[PAD + self.off + self.n:]))
        assert bool((edge == self.canary).all()), (what, "a canary next to the buffer was overwritten")
        return h[PAD + self.off:PAD + self.off + self.n]


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _table(rows):
    """rows of (p, g, m, v, n) addresses (0 = NULL) -> the device chunk table."""
    tab = np.zeros(len(rows), dtype=_DT)
    for i, (p, g, m, v, n) in enumerate(rows):
        tab[i] = (p, g, m, v, n, 1e-3, 1.5, 0.0)
    return torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)


# ---- 1, 2: sp_grad_sqnorm_multi -------------------------------------------------------------------------------------------------------
def _sqnorm_case(make, off):
    """One gradient buffer holding the seven chunks (each starting `off` floats past a 16-byte boundary), the g-and-n-only table, the
    guarded partials."""
    grads = [make(n, 100 + i) for i, n in enumerate(LENGTHS)]
    starts, at = [], 0
    for n in LENGTHS:
        starts.append(at + off)
        at += (n + off + 3) // 4 * 4 + 4                            # a gap of canary-free zeros is fine: the kernel only reads
    buf = torch.zeros(at, dtype=F32)
    for s, g in zip(starts, grads):
        buf[s:s + len(g)] = torch.from_numpy(g)
    buf = buf.to(DEV)
    assert buf.data_ptr() % 16 == 0
    table = _table([(0, buf.data_ptr() + 4 * s, 0, 0, n) for s, n in zip(starts, LENGTHS)])       # p, m, v NULL: they are not read
    assert all(((buf.data_ptr() + 4 * s) % 16 == 0) == (off == 0) for s in starts)
    partials = Guarded(torch.full((len(LENGTHS),), -7.0, dtype=torch.float64), canary=-1536.0)
    L.call("sp_grad_sqnorm_multi", ops.ptr(table), len(LENGTHS), ops.ptr(partials.t), ops.stream())
    torch.cuda.synchronize()
    return grads, partials.host("partials").tolist()


@pytest.mark.parametrize("off", [0, 1], ids=["float4", "scalar"])
def test_sqnorm_is_exact_on_integer_gradients(off):
    grads, got = _sqnorm_case(C.integer_gradients, off)
    C.assert_exact_operands(grads)
    assert any((g == 0).any() for g in grads) and any((g < 0).any() for g in grads)
    want = [C.sqnorm(g) for g in grads]
    assert got == want, (off, got, want)


@pytest.mark.parametrize("off", [0, 1], ids=["float4", "scalar"])
def test_sqnorm_on_real_gradients_within_the_derived_bound(off):
    """|partial - fsum| <= n * 2^-53 * fsum: the products are exact, and each of the n - 1 additions of non-negative terms rounds by at
    most 2^-53 of a partial sum that is no larger than the total."""
    grads, got = _sqnorm_case(C.real_gradients, off)
    for n, g, have in zip(LENGTHS, grads, got):
        want = C.sqnorm_fsum(g)
        err, lim = abs(have - want), n * 2.0 ** -53 * want
        print("sqnorm real n %6d off %d: |partial - fsum| = %.3e, bound %.3e" % (n, off, err, lim))
        assert err <= lim, (n, off, have, want)


def test_sqnorm_refuses_bad_arguments():
    x = torch.zeros(8, device=DEV)
    table = _table([(0, x.data_ptr(), 0, 0, 8)])
    part = Guarded(torch.full((1,), -7.0, dtype=torch.float64))
    lib = L.lib()
    assert lib.sp_grad_sqnorm_multi(None, 1, ops.ptr(part.t), ops.stream()) == SP_ERR_INVALID
    assert lib.sp_grad_sqnorm_multi(ops.ptr(table), 0, ops.ptr(part.t), ops.stream()) == SP_ERR_INVALID
    assert lib.sp_grad_sqnorm_multi(ops.ptr(table), 1, None, ops.stream()) == SP_ERR_INVALID
    torch.cuda.synchronize()
    assert part.host("partials").tolist() == [-7.0]


# ---- 3: sp_grad_clip_finalize ---------------------------------------------------------------------------------------------------------
def _finalize(state, partials, max_norm):
    """One call on guarded buffers; returns the state after it as a list of floats (canaries checked)."""
    st = Guarded(torch.tensor(state, dtype=F32))
    part = Guarded(torch.tensor(partials, dtype=torch.float64))
    L.call("sp_grad_clip_finalize", ops.ptr(part.t), len(partials), float(max_norm), ops.ptr(st.t), ops.stream())
    torch.cuda.synchronize()
    assert _same_bits(part.host("partials").view(torch.float32), torch.tensor(partials, dtype=torch.float64).view(torch.float32))
    return st.host("state").tolist()


def _f32_bits(x):
    return int(np.float32(x).view(np.int32))


def test_finalize_coefficient_counters_and_flag():
    st0 = [7.0, 7.0, 1.0, 2.0, 3.0]
    # below the threshold: exactly 1.0f, nothing counted, the stale flag cleared
    got = _finalize(st0, [9.0, 16.0], 10.0)
    assert got == C.finalize(st0, [9.0, 16.0], 10.0) == [5.0, 1.0, 0.0, 2.0, 3.0]
    # above: the coefficient's bits are the restatement's, [4] counts
    for partials, max_norm in (([9.0, 16.0], 2.5), ([2.0, 3.0, 6.0], 1.0), ([1e12, 7.0], 1.0 / 3.0), ([12345.0] * 37, 100.0)):
        got, want = _finalize(st0, partials, max_norm), C.finalize(st0, partials, max_norm)
        assert _f32_bits(got[1]) == _f32_bits(want[1]) and got[1] < 1.0, (partials, max_norm, got, want)
        assert _f32_bits(got[0]) == _f32_bits(want[0])
        assert got[2:] == [0.0, 2.0, 4.0] == want[2:]
    # max_norm = inf: exactly 1.0f whatever the norm
    assert _finalize(st0, [1e30, 1e30], INF) == [float(np.float32(math.sqrt(2e30))), 1.0, 0.0, 2.0, 3.0]
    assert _finalize(st0, [0.0], 1.0) == [0.0, 1.0, 0.0, 2.0, 3.0]             # a zero norm: 1 / 1e-6, clamped to 1


def test_finalize_non_finite_sum_skips_and_a_clean_call_clears_the_flag():
    st = [5.0, 1.0, 0.0, 2.0, 3.0]
    for bad in (INF, NAN):
        got = _finalize(st, [4.0, bad, 1.0], 10.0)
        want = C.finalize(st, [4.0, bad, 1.0], 10.0)
        assert got[1:] == [0.0, 1.0, st[3] + 1.0, 3.0] == want[1:], (bad, got, want)
        assert math.isinf(got[0]) if bad == INF else math.isnan(got[0])
        st = got
    got = _finalize([0.0 if math.isnan(v) else v for v in st], [4.0], INF)     # a clean call: flag cleared, the count stays
    assert got == [2.0, 1.0, 0.0, 4.0, 3.0]


@pytest.mark.parametrize("n", [1, 2, 300, 1000])
def test_finalize_sums_integer_partials_exactly(n):
    """n integer partials < 2^30 (n <= 1000: the sum stays below 2^40): every order of addition gives the exact sum, so norm and
    coefficient must equal the restatement's bits - across one thread (n = 1, 2), one round of 256 (300) and several (1000)."""
    rng = np.random.default_rng(n)
    partials = [float(v) for v in rng.integers(0, 1 << 30, size=n)]
    total = float(sum(int(v) for v in partials))
    assert total < 2.0 ** 40 and math.fsum(partials) == total
    max_norm = 0.5 * math.sqrt(total)
    got, want = _finalize([0.0] * 5, partials, max_norm), C.finalize([0.0] * 5, partials, max_norm)
    assert got[0] == float(np.float32(math.sqrt(total)))
    assert [_f32_bits(v) for v in got] == [_f32_bits(v) for v in want], (got, want)
    assert got[4] == 1.0 and 0.49 < got[1] < 0.51


def test_finalize_refuses_bad_arguments_without_a_launch():
    st = Guarded(torch.tensor([5.0, 0.5, 1.0, 2.0, 3.0]))
    part = Guarded(torch.tensor([4.0], dtype=torch.float64))
    lib, s, p = L.lib(), ops.ptr(st.t), ops.ptr(part.t)
    for max_norm in (0.0, -1.0, NAN):
        assert lib.sp_grad_clip_finalize(p, 1, max_norm, s, ops.stream()) == SP_ERR_INVALID, max_norm
    assert lib.sp_grad_clip_finalize(None, 1, 1.0, s, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_grad_clip_finalize(p, 1, 1.0, None, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_grad_clip_finalize(p, 0, 1.0, s, ops.stream()) == SP_ERR_INVALID
    torch.cuda.synchronize()
    assert st.host("state").tolist() == [5.0, 0.5, 1.0, 2.0, 3.0]


# ---- 4: sp_adam_multi_clipped ---------------------------------------------------------------------------------------------------------
HYPER = (0.5, 0.999, 1e-8)


def _adam_state(seed, scale_g=None):
    """p, g, m, v (guarded) of the four tensors of clip_restated.SIZES; scale_g: a device fp32 scalar every gradient is multiplied by
    first (torch.mul in fp32: one IEEE product per element)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in C.SIZES:
        p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
        v = torch.rand(n, generator=gen) * 1e-2
        if scale_g is not None:
            g = torch.mul(g.to(DEV), scale_g).cpu()
        out.append([Guarded(p), Guarded(g), Guarded(m), Guarded(v)])
    return out


def _adam_table(state):
    rows = []
    for p, g, m, v in state:
        for lo, n in C.chunks(p.n):
            rows.append(tuple(t.t.data_ptr() + 4 * lo for t in (p, g, m, v)) + (n,))
    assert len(rows) == 5                                                      # 70 000 elements: two chunks
    return _table(rows), len(rows)


def _host(state, what):
    return [[t.host((what, i, name)) for name, t in zip("pgmv", ch)] for i, ch in enumerate(state)]


def _assert_states_equal(a, b, what, skip_g=False):
    for i, (ca, cb) in enumerate(zip(a, b)):
        for name, ta, tb in zip("pgmv", ca, cb):
            if skip_g and name == "g":
                continue
            assert _same_bits(ta, tb), (what, "tensor", i, name, int((_bits(ta) != _bits(tb)).sum()))


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_clipped_with_coefficient_one_is_the_guarded_step(weight_decay):
    a, b = _adam_state(9), _adam_state(9)
    before = _host(a, "before")
    (ta, na), (tb, nb) = _adam_table(a), _adam_table(b)
    clip = Guarded(torch.tensor([7.0, 1.0, 0.0, 3.0, 4.0]))
    L.call("sp_adam_multi_clipped", ops.ptr(ta), na, *HYPER, weight_decay, None, ops.ptr(clip.t), ops.stream())
    L.call("sp_adam_multi_guarded", ops.ptr(tb), nb, *HYPER, weight_decay, None, ops.stream())
    torch.cuda.synchronize()
    ha, hb = _host(a, "clipped"), _host(b, "guarded")
    _assert_states_equal(ha, hb, "coefficient 1.0, weight decay %r" % weight_decay)
    assert clip.host("clip state").tolist() == [7.0, 1.0, 0.0, 3.0, 4.0]       # read only
    for ch, ch0 in zip(ha, before):
        assert _same_bits(ch[1], ch0[1])                                       # the gradients are not written
        assert not any(torch.equal(ch[k], ch0[k]) for k in (0, 2, 3)), "the step changed nothing"


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("coef", [0.5, 0.3], ids=["half", "0.3"])
def test_clipped_is_the_plain_step_on_prescaled_gradients(coef, weight_decay):
    """The single-rounding contract: fp32(g * coefficient) is what the step reads - not a product fused into g - m or g + wd * p."""
    c32 = torch.tensor(coef, dtype=F32, device=DEV)
    a, b = _adam_state(21), _adam_state(21, scale_g=c32)
    g_before = [ch[1].host() for ch in a]
    (ta, na), (tb, nb) = _adam_table(a), _adam_table(b)
    clip = Guarded(torch.tensor([7.0, float(c32), 0.0, 3.0, 4.0]))
    L.call("sp_adam_multi_clipped", ops.ptr(ta), na, *HYPER, weight_decay, None, ops.ptr(clip.t), ops.stream())
    L.call("sp_adam_multi", ops.ptr(tb), nb, *HYPER, weight_decay, ops.stream())
    torch.cuda.synchronize()
    ha, hb = _host(a, "clipped"), _host(b, "plain on scaled")
    _assert_states_equal(ha, hb, "coefficient %r, weight decay %r" % (coef, weight_decay), skip_g=True)
    for ch, g0 in zip(ha, g_before):
        assert _same_bits(ch[1], g0)                                           # the clipped launch does not write its gradients


@pytest.mark.parametrize("how", ["clip flag", "skip pointer", "both"])
def test_clipped_skips_everything_on_either_flag(how):
    a = _adam_state(33)
    before = _host(a, "before")
    ta, na = _adam_table(a)
    clip = Guarded(torch.tensor([7.0, 0.5, 1.0 if how != "skip pointer" else 0.0, 3.0, 4.0]))
    skip = Guarded(torch.tensor([1.0 if how != "clip flag" else 0.0]))
    L.call("sp_adam_multi_clipped", ops.ptr(ta), na, *HYPER, 0.01, ops.ptr(skip.t), ops.ptr(clip.t), ops.stream())
    torch.cuda.synchronize()
    _assert_states_equal(_host(a, how), before, how)
    assert L.lib().sp_adam_multi_clipped(ops.ptr(ta), na, *HYPER, 0.01, None, None, ops.stream()) == SP_ERR_INVALID
    assert L.lib().sp_adam_multi_clipped(None, na, *HYPER, 0.01, None, ops.ptr(clip.t), ops.stream()) == SP_ERR_INVALID


# ---- 5: optim.Adam(max_grad_norm=...) -------------------------------------------------------------------------------------------------
def _prescaled_run(params0, groups, grads_per_step, coefs, adam_kw):
    """The reference of the clipped optimizer: a PLAIN optim.Adam over copies of params0 (a list per group; groups: per-group options) that
    steps on gradients scaled by torch.mul in fp32 with the given coefficient of each step.  Returns the parameters, flat."""
    ps = [[torch.nn.Parameter(p.detach().clone()) for p in grp] for grp in params0]
    opt = optim.Adam([dict(params=grp, **kw) for grp, kw in zip(ps, groups)], **adam_kw)
    flat = [p for grp in ps for p in grp]
    for p in flat:
        p.grad = torch.zeros_like(p)
    for grads, coef in zip(grads_per_step, coefs):
        c32 = torch.tensor(float(coef), dtype=F32, device=DEV)
        for p, g in zip(flat, grads):
            p.grad.copy_(torch.mul(g.to(DEV), c32))
        opt.step()
    torch.cuda.synchronize()
    return flat


def test_adam_with_two_groups_clips_by_the_global_norm():
    gen = torch.Generator().manual_seed(4)
    params0 = [[torch.randn(n, generator=gen).to(DEV) for n in C.SIZES[:3]], [torch.randn(C.SIZES[3], generator=gen).to(DEV)]]
    groups = [dict(lr=1e-3), dict(lr=3e-4, weight_decay=0.01)]
    sizes = [p.numel() for grp in params0 for p in grp]
    # three steps of integer gradients of growing size: with max_norm between them the first is not clipped, the others are
    grads_np = [[C.integer_gradients(n, 50 * step + i, scale=(2, 40, 1024)[step]) for i, n in enumerate(sizes)] for step in range(3)]
    for gs in grads_np:
        C.assert_exact_operands(gs)
    totals = [math.fsum(C.sqnorm(g) for g in gs) for gs in grads_np]
    max_norm = 2.0 * math.sqrt(totals[0])
    assert math.sqrt(totals[0]) < max_norm < math.sqrt(totals[1]) < math.sqrt(totals[2])
    ps = [[torch.nn.Parameter(p.clone()) for p in grp] for grp in params0]
    opt = optim.Adam([dict(params=grp, **kw) for grp, kw in zip(ps, groups)], max_grad_norm=max_norm)
    flat = [p for grp in ps for p in grp]
    for p in flat:
        p.grad = torch.zeros_like(p)
    state, coefs = [0.0] * 5, []
    for step, gs in enumerate(grads_np):
        for p, g in zip(flat, gs):
            p.grad.copy_(torch.from_numpy(g))
        opt.step()
        # the restatement sees the per-chunk partials the optimizer's tables produce (any split gives the same exact sum)
        state = C.finalize(state, [C.sqnorm(g[lo:lo + n]) for g in gs for lo, n in C.chunks(len(g))], max_norm)
        got = opt.clip_state.tolist()
        assert [_f32_bits(v) for v in got] == [_f32_bits(v) for v in state], (step, got, state)
        assert float(opt.grad_norm) == float(np.float32(math.sqrt(totals[step])))             # over BOTH groups
        assert float(opt.skip_flag) == 0.0
        assert opt.grad_norm.data_ptr() == opt.clip_state.data_ptr() and opt.skip_flag.data_ptr() == opt.clip_state.data_ptr() + 8
        coefs.append(state[1])
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] < coefs[1] and state[4] == 2.0 and state[3] == 0.0
    want = _prescaled_run(params0, groups, [[torch.from_numpy(g) for g in gs] for gs in grads_np], coefs, {})
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(flat, want)):
        assert _same_bits(a, b), ("parameter", i, int((_bits(a) != _bits(b)).sum()))
        assert not torch.equal(a.detach(), [p for grp in params0 for p in grp][i])
    sd = opt.state_dict()
    ref = torch.optim.Adam([dict(params=[torch.nn.Parameter(p.clone()) for p in grp], **kw) for grp, kw in zip(params0, groups)])
    rd = ref.state_dict()
    assert set(sd) == set(rd) and [set(g) for g in sd["param_groups"]] == [set(g) for g in rd["param_groups"]]
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values()) and len(sd["state"]) == 4
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())


def test_adam_without_max_grad_norm_launches_nothing_new(monkeypatch):
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    ps = [torch.nn.Parameter(torch.randn(n).to(DEV)) for n in (7, 70000)]
    for p in ps:
        p.grad = torch.randn_like(p)
    off = optim.Adam([dict(params=ps[:1]), dict(params=ps[1:])], max_grad_norm=None)
    off.step()
    assert calls == ["sp_adam_multi", "sp_adam_multi"], calls
    assert off._clip is None and not hasattr(off, "clip_state") and not hasattr(off, "grad_norm") and not hasattr(off, "skip_flag")
    del calls[:]
    on = optim.Adam([dict(params=ps[:1]), dict(params=ps[1:])], max_grad_norm=INF)
    on.step()
    on.step()
    want = ["sp_grad_sqnorm_multi"] * 2 + ["sp_grad_clip_finalize"] + ["sp_adam_multi_clipped"] * 2
    assert calls == want * 2, calls
    buffers = (on._clip[0].data_ptr(), on._clip[1].data_ptr())
    on.step()
    assert (on._clip[0].data_ptr(), on._clip[1].data_ptr()) == buffers       # allocated once, reused
    torch.cuda.synchronize()


# ---- 6: the training step -------------------------------------------------------------------------------------------------------------
CF, BATCH = 8, 2


def _networks():
    Gsd = params.synth_state_dict(O.layout_template(O.generator_layout(CF)), 0)
    Dsd = params.synth_state_dict(O.layout_template(O.discriminator_layout(CF)), 1)
    Vsd = params.synth_state_dict(O.layout_template(O.vgg16_layout()), 2)
    G, D, V = sp.Generator(channels_factor=CF), sp.Discriminator(channel_factor=CF), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    return G.cuda(), D.cuda(), V.cuda().eval()


def _wrapper(clip, adam=None, **kw):
    adam = adam or sp.optim.Adam
    G, D, V = _networks()
    mw = sp.ModelWrapper(G, D, None, None, vgg16=V, generator_optimizer=adam(G.parameters(), lr=1e-5),
                         discriminator_optimizer=adam(D.parameters(), lr=1e-5), save_data_path=None, clip_grad_norm=clip, **kw)
    G.train(); D.train()
    return mw


def _record_steps(mw, keep_grads=False):
    """Wraps mw._optimizer_step: in front of every optimizer step the float64 norm of the network's flat gradient buffer (and of its
    parameters' .grad, which are views of it) is taken, behind it the optimizer's clip state.  Returns the list the records go to."""
    log = []
    inner = mw._optimizer_step

    def step(key, optimizer):
        ps = mw._d_params if key == "d" else mw._g_params
        rec = {"key": key, "flat_norm": float(mw._banks[key].flat.double().norm()),
               "grad_norm": math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps if p.grad is not None))}
        if keep_grads:
            rec["params"] = [p.detach().clone() for p in ps] if not any(r["key"] == key for r in log) else None
            rec["grads"] = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for p in ps]
        inner(key, optimizer)
        if isinstance(optimizer, optim.Adam) and optimizer.max_grad_norm is not None:
            rec["state"] = optimizer.clip_state.tolist()
        log.append(rec)
    mw._optimizer_step = step
    return log


@pytest.fixture(scope="module")
def stepped():
    """Eager, eager, capture, replayed - with clip_grad_norm = inf and without it: same states, batch and latents, fp32 parity mode."""
    torch.cuda.set_device(0)
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = synthetic.synthetic_batch(BATCH, 0)
    images, labels, masks = images.cuda(), labels.cuda(), [m.cuda() for m in masks]
    noise = torch.randn(6, BATCH, 128, generator=torch.Generator().manual_seed(1)).cuda()
    rec = {"batch": (images, labels, masks), "noise": noise}
    for name, clip in (("inf", INF), ("plain", None)):
        mw = _wrapper(clip)
        log = _record_steps(mw)
        outs = []
        for it in range(2):
            out = mw.train_step(images, labels, masks, noise_d=noise[2 * it], noise_g=noise[2 * it + 1], next_images_real=images)
            outs.append({k: (v.clone() if k != "images_fake" else None) for k, v in out.items()})
        mw.capture_graphs(images, labels, masks)
        out = mw.train_step_graphed(noise_d=noise[4], noise_g=noise[5])
        outs.append({k: (v.clone() if k != "images_fake" else None) for k, v in out.items()})
        torch.cuda.synchronize()
        rec[name] = {"mw": mw, "outs": outs, "log": log,
                     "params": [p.detach().clone() for p in list(mw.generator.parameters()) + list(mw.discriminator.parameters())]}
    return rec


def test_monitoring_changes_nothing_and_adds_exactly_two_results(stepped):
    on, off = stepped["inf"], stepped["plain"]
    for it, (a, b) in enumerate(zip(on["outs"], off["outs"])):
        assert set(b) == set(LOSS_NAMES) | {"images_fake"}, (it, sorted(b))
        assert set(a) == set(b) | set(NORM_NAMES), (it, sorted(a))
        for n in LOSS_NAMES:
            assert _same_bits(a[n].reshape(1), b[n].reshape(1)), (it, n, float(a[n]), float(b[n]))
        for n in NORM_NAMES:
            assert a[n].is_cuda and a[n].dim() == 0 and a[n].dtype == F32
    for i, (a, b) in enumerate(zip(on["params"], off["params"])):
        assert _same_bits(a, b), ("parameter", i)
    st_g, st_d = on["mw"].generator_optimizer.clip_state.tolist(), on["mw"].discriminator_optimizer.clip_state.tolist()
    assert st_g[1:] == [1.0, 0.0, 0.0, 0.0] and st_d[1:] == [1.0, 0.0, 0.0, 0.0]        # never scaled, never skipped
    assert not hasattr(off["mw"].generator_optimizer, "clip_state") and off["mw"].clip_grad_norm is None


def test_logged_norms_are_the_float64_norms_of_the_flat_buffers(stepped):
    """1e-6 relative: the kernels' fp64 sum is some 1e-13 from the float64 norm of the same bits, the result is rounded to fp32 once
    (2^-24 = 6e-8)."""
    on = stepped["inf"]
    assert [r["key"] for r in on["log"]] == ["d", "g"] * 3
    for it, out in enumerate(on["outs"]):
        for rec, name in zip(on["log"][2 * it:2 * it + 2], NORM_NAMES):
            got, want = float(out[name]), rec["flat_norm"]
            print("step %d %s: logged %.9g, float64 norm of flat %.9g, of the .grad views %.9g" % (it, name, got, want, rec["grad_norm"]))
            assert want > 0.0 and abs(got - want) <= 1e-6 * want, (it, name, got, want)
            assert got == rec["state"][0]


def test_clipping_in_the_step_equals_prescaled_gradients(stepped):
    """clip_grad_norm = half the smaller of the two norms the first step measured: both networks clip in the first step.  Two eager
    steps; the parameters must equal a plain optim.Adam's on the recorded gradients scaled by the restated coefficients."""
    first = stepped["inf"]["log"][:2]
    clip = 0.5 * min(r["flat_norm"] for r in first)
    images, labels, masks = stepped["batch"]
    noise = stepped["noise"]
    mw = _wrapper(clip)
    log = _record_steps(mw, keep_grads=True)
    for it in range(2):
        out = mw.train_step(images, labels, masks, noise_d=noise[2 * it], noise_g=noise[2 * it + 1], next_images_real=images)
    torch.cuda.synchronize()
    assert set(NORM_NAMES) <= set(out)
    for key, net, opt in (("d", mw.discriminator, mw.discriminator_optimizer), ("g", mw.generator, mw.generator_optimizer)):
        recs = [r for r in log if r["key"] == key]
        assert len(recs) == 2 and recs[0]["params"] is not None
        state, coefs = [0.0] * 5, []
        for r in recs:
            partials = [C.sqnorm(c) for g in r["grads"] for c in np.split(g.reshape(-1).cpu().numpy(), range(C.CHUNK, g.numel(), C.CHUNK))]
            state = C.finalize(state, partials, clip)
            assert _f32_bits(r["state"][1]) == _f32_bits(state[1]), (key, r["state"], state)
            assert r["state"][2:] == state[2:]
            coefs.append(state[1])
        assert coefs[0] < 0.51 and recs[-1]["state"][4] >= 1.0 and recs[-1]["state"][3] == 0.0, (key, coefs, recs[-1]["state"])
        want = _prescaled_run([recs[0]["params"]], [dict()], [r["grads"] for r in recs], coefs, dict(lr=1e-5))
        for i, (a, b) in enumerate(zip(net.parameters(), want)):
            assert _same_bits(a, b), (key, "parameter", i, int((_bits(a) != _bits(b)).sum()))
    # the discriminator's first norm is the one the monitoring run measured: no optimizer step lies in front of that gradient
    assert log[0]["key"] == "d" and log[0]["flat_norm"] == first[0]["flat_norm"]


def test_foreign_optimizer_goes_through_torchs_utility(stepped, monkeypatch):
    """torch.optim.Adam with the setting on: torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True) in front of each step(), and
    its norm is what gets logged.  torch's fp32 reduction is not this package's to hold: 1e-4 relative only says it is the same quantity
    (fp32 sums over up to 8e6 elements in torch's blocked order stay far inside it)."""
    seen = []
    real = torch.nn.utils.clip_grad_norm_

    def spy(parameters, max_norm, *a, **kw):
        seen.append((len(list(parameters)), max_norm, kw.get("foreach")))
        return real(parameters, max_norm, *a, **kw)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    images, labels, masks = stepped["batch"]
    noise = stepped["noise"]
    mw = _wrapper(INF, adam=torch.optim.Adam)
    log = _record_steps(mw)
    out = mw.train_step(images, labels, masks, noise_d=noise[0], noise_g=noise[1], next_images_real=images)
    torch.cuda.synchronize()
    assert seen == [(len(mw._d_params), INF, True), (len(mw._g_params), INF, True)], seen
    assert not hasattr(mw.generator_optimizer, "max_grad_norm")
    for rec, name in zip(log, NORM_NAMES):
        got = float(out[name])
        assert abs(got - rec["grad_norm"]) <= 1e-4 * rec["grad_norm"], (name, got, rec)
    # max_norm = inf scales by exactly 1: the step is the one the monitoring run of this package's Adam took only up to the two
    # optimizers' different arithmetic, so the losses of step one - computed before any optimizer step - agree bit for bit
    for n in LOSS_NAMES[:2]:
        assert _same_bits(out[n].reshape(1), stepped["inf"]["outs"][0][n].reshape(1)), n


# ---- 7: the guard ---------------------------------------------------------------------------------------------------------------------
def _small_wrapper(dtype, **kw):
    import test_gpu_step as S
    meta, _ = gu.load("step_cf4_b4_seed1")
    ops.set_compute_dtype(dtype)
    G, D, V = S.build(meta)
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=None, validation_dataset=None,
                         generator_optimizer=sp.optim.Adam(G.parameters(), lr=meta["lr"]),
                         discriminator_optimizer=sp.optim.Adam(D.parameters(), lr=meta["lr"]), save_data_path=None, **kw)
    G.train(); D.train()
    images, labels, masks = gu.golden_batches(meta["batch_size"], meta["seed"])[0]
    return mw, (images.cuda(), labels.cuda(), [m.cuda() for m in masks])


def _g_state(mw):
    opt = mw.generator_optimizer
    ps = list(mw.generator.parameters())
    have = [p for p in ps if "exp_avg" in opt.state.get(p, {})]
    assert len(have) > len(ps) // 2
    return ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in have], [opt.state[p]["exp_avg_sq"].clone() for p in have],
            mw.generator_ema.buffer.clone())


def _all_same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


def test_one_nan_in_bf16_skips_the_generator_step_and_its_average():
    mw, (images, labels, masks) = _small_wrapper(torch.bfloat16, clip_grad_norm=INF, generator_ema=0.999)
    assert ops.loss_scaler(images.device) is None                                # no loss scaler in this mode: the new guard alone
    for _ in range(2):                                                           # (the first update only initialises the average)
        mw.train_step(images, labels, masks)
    opt, ema = mw.generator_optimizer, mw.generator_ema
    assert opt.clip_state.tolist()[2:] == [0.0, 0.0, 0.0] and ema.num_updates == 2
    inner, snap = mw._optimizer_step, {}

    def poisoned(key, optimizer):
        if key == "g":                                                           # behind the generator phase's backward
            bank, grad = mw._banks["g"], mw._g_params[0].grad
            at = (grad.data_ptr() - bank.flat.data_ptr()) // 4
            assert 0 <= at < bank.flat.numel()
            bank.flat[at] = NAN
            snap["before"] = _g_state(mw)
        inner(key, optimizer)
    mw._optimizer_step = poisoned
    d_before = [p.detach().clone() for p in mw.discriminator.parameters()]
    mw.train_step(images, labels, masks)
    mw._optimizer_step = inner
    torch.cuda.synchronize()
    after = _g_state(mw)
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), after[:3], snap["before"][:3]):
        assert _all_same(a, b), name
    assert _same_bits(after[3], snap["before"][3]), "the average moved behind a skipped step"
    st = opt.clip_state.tolist()
    assert st[1:4] == [0.0, 1.0, 1.0] and math.isnan(st[0]), st
    assert mw.discriminator_optimizer.clip_state.tolist()[2:4] == [0.0, 0.0]     # D's own step was clean and ran
    assert not _all_same([p.detach() for p in mw.discriminator.parameters()], d_before)
    # the next clean step updates again; the count stays
    out = mw.train_step(images, labels, masks)
    torch.cuda.synchronize()
    clean = _g_state(mw)
    assert not _all_same(clean[0], after[0]) and not _same_bits(clean[3], after[3])
    st = opt.clip_state.tolist()
    assert st[1:4] == [1.0, 0.0, 1.0] and math.isfinite(st[0]) and st[0] > 0.0, st
    assert all(bool(torch.isfinite(p).all()) for p in clean[0]) and math.isfinite(float(out["grad_norm_generator"]))


def test_f16_overflow_is_skipped_as_before_and_the_two_flags_agree():
    ops.set_loss_scale(2.0 ** 40, growth_interval=3)
    mw, (images, labels, masks) = _small_wrapper(torch.float16, clip_grad_norm=INF)
    own_g = [p.detach().clone() for p in mw.generator.parameters()]
    own_d = [p.detach().clone() for p in mw.discriminator.parameters()]
    inner, flags = mw._optimizer_step, []

    def watched(key, optimizer):                                                 # the scaler's flag, read before sc.update() clears it
        sc = ops.loss_scaler(images.device)
        sc.check(mw._banks[key].flat)
        flags.append(sc.values()["found"])
        inner(key, optimizer)
        flags.append(optimizer.clip_state.tolist()[2] == 1.0)
    mw._optimizer_step = watched
    mw.train_step(images, labels, masks)
    torch.cuda.synchronize()
    v = ops.loss_scaler(images.device).values()
    assert v["skipped_steps"] == 2 and not v["found"] and v["scale"] == 2.0 ** 38, v      # skipped as today, and the scale backed off twice
    assert flags == [True, True, True, True], flags                                     # [2] agrees with the scaler's flag, D and G
    assert _all_same(own_g, [p.detach() for p in mw.generator.parameters()])
    assert _all_same(own_d, [p.detach() for p in mw.discriminator.parameters()])
    for opt in (mw.generator_optimizer, mw.discriminator_optimizer):
        st = opt.clip_state.tolist()
        assert st[1:4] == [0.0, 1.0, 1.0], st


# ---- train(): the log and the checkpoint ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_adam", [True, False], ids=["sempyr Adam", "torch Adam"])
def test_train_logs_the_two_norms_and_adds_nothing_to_the_checkpoint(tmp_path, monkeypatch, own_adam):
    """ModelWrapper.train() over the two golden batches (channel factor 4, batch 4, fp32) with the switch coming from
    config.CFG.clip_grad_norm (SP_CLIP_GRAD_NORM: main.py builds the wrapper with fixed keywords, and torch.optim.Adam)."""
    import os

    import make_golden
    from semantic_pyramid_for_image_generation_amd import config
    meta, _ = gu.load("step_cf4_b4_seed1")
    ops.set_compute_dtype(torch.float32)
    Gsd, Dsd, Vsd = gu.synth_states(meta)
    monkeypatch.setattr(config.CFG, "clip_grad_norm", INF)
    G, D, V = sp.Generator(channels_factor=meta["cf"]).cuda(), sp.Discriminator(channel_factor=meta["cf"]).cuda(), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    loader = make_golden.TwoBatchLoader(make_golden.golden_batches(meta["batch_size"], meta["seed"]), meta["batch_size"])
    adam = sp.optim.Adam if own_adam else torch.optim.Adam
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=loader, validation_dataset=None,
                         generator_optimizer=adam(G.parameters(), lr=meta["lr"]), discriminator_optimizer=adam(D.parameters(), lr=meta["lr"]),
                         save_data_path=str(tmp_path))
    assert mw.clip_grad_norm == INF and mw.logger.hyperparameter["clip_grad_norm"] == "inf"
    log = _record_steps(mw)
    torch.manual_seed(1234)
    mw.train(epochs=1, device="cuda")
    m = mw.logger.metrics
    assert len(m["loss_generator"]) == 2 and len(m["grad_norm_discriminator"]) == 2 and len(m["grad_norm_generator"]) == 2
    for it in range(2):
        for rec, name in zip(log[2 * it:2 * it + 2], NORM_NAMES):
            got, want = m[name][it], rec["grad_norm"]
            assert isinstance(got, float) and abs(got - want) <= (1e-6 if own_adam else 1e-4) * want, (it, name, got, want)
    ck = torch.load(os.path.join(mw.path_save_models, "checkpoint_000.pt"), map_location="cpu")
    assert set(ck) == {"generator", "discriminator", "generator_optimizer", "discriminator_optimizer"}
    assert set(ck["generator_optimizer"]) == {"state", "param_groups"}
    assert "max_grad_norm" not in ck["generator_optimizer"]["param_groups"][0]
