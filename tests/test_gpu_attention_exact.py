"""The attention kernels (csrc/attention.hip) held to an exact selection and to derived bounds; operands, references, conditions
and the comparison: tests/attention_exact_util.py, checked against itself on the CPU by tests/test_attention_harness.py.

The C ABI is called directly.  o, lse, dq, dk and dv lie between canary rows and start as canaries themselves, the fp32 slab scratch
starts as NaN (every slab element the reduction reads must have been written) with canaries behind it.  select: torch.equal.  pair:
the 16-bit forward exact, |lse - ln 2| <= 2^-20, B = 2^-18 x T for the gradients and the fp32 forward.  dense: the per-element bounds
of attention_exact_util.dense_case.  The route of every case comes from sp_attention_route, and the slab count must agree with it."""
import ctypes
import functools

import pytest
import torch

import attention_exact_util as A
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = A.BF16, A.F16, A.F32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
SLAB = {"mfma": 64, "valu tq32": 32, "valu tq16": 16}
CANARY, PAD = -1536.0, 8                 # held exactly by every storage type; 8 rows keep the 16-byte alignment of the body
TABLE_IDS = ["%s-%s" % (NAME[dt], A.case_id(c)) for dt, c in A.TABLE]
SEEN = set()                             # (16-bit storage, (forward, backward)) of every launch pair


class Guarded:
    """[PAD canary rows][rows x cols, filled with `body`][PAD canary rows] on the device; .t is the body."""

    def __init__(self, rows, cols, dtype, body=CANARY):
        self.rows = rows
        self.buf = torch.full((PAD + rows + PAD, cols), CANARY, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + rows]
        self.t.fill_(body)

    def check(self, what):
        edge = torch.cat((self.buf[:PAD], self.buf[PAD + self.rows:])).cpu()
        assert bool((edge == CANARY).all()), (what, "a canary row next to the buffer was overwritten")


@functools.lru_cache(maxsize=None)
def built(regime, dt, case, shifted=False):
    return A.build(regime, dt, case, shifted)


def _dev(t, dt):
    out = t.to(dt).contiguous()
    assert torch.equal(out.double(), t), "the storage type does not hold an operand exactly"
    return out.to(DEV)


def launch(c, dt):
    """sp_attention_fwd, then sp_attention_bwd on the lse it stored.  Returns the five results on the host and the routes."""
    n, nk, d, dv, b = c.dims
    sp = ops.sp_dtype(dt)
    route = L.attention_route(n, nk, d, dv, sp)
    slabs = ctypes.c_int64(-1)
    L.call("sp_attention_bwd_slabs", n, nk, d, dv, sp, ctypes.byref(slabs))
    assert slabs.value == -(-n // SLAB[route[1]]), (c.what, route, slabs.value)
    q, k, v, do = (_dev(c[x], dt) for x in ("q", "k", "v", "do"))
    o, lse, dq = Guarded(b * n, dv, dt), Guarded(b * n, 1, F32), Guarded(b * n, d, dt)
    dk, dvv = Guarded(b * nk, d, dt), Guarded(b * nk, dv, dt)
    dk32 = Guarded(slabs.value * b * nk, d, F32, float("nan"))
    dv32 = Guarded(slabs.value * b * nk, dv, F32, float("nan"))
    L.call("sp_attention_fwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(o.t), ops.ptr(lse.t), b, n, nk, d, dv, sp, ops.stream())
    L.call("sp_attention_bwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(do), ops.ptr(lse.t), ops.ptr(dq.t), ops.ptr(dk32.t),
           ops.ptr(dv32.t), ops.ptr(dk.t), ops.ptr(dvv.t), b, n, nk, d, dv, sp, ops.stream())
    torch.cuda.synchronize()
    for name, g in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dvv), ("dk slabs", dk32), ("dv slabs", dv32)):
        g.check((c.what, name))
    SEEN.add((dt != F32, route))
    got = A.Case(o=o.t.cpu().view(b, n, dv), lse=lse.t.cpu().view(b, n), dq=dq.t.cpu().view(b, n, d), dk=dk.t.cpu().view(b, nk, d),
                 dv=dvv.t.cpu().view(b, nk, dv))
    return got, route


@pytest.mark.parametrize("dt,case", A.TABLE, ids=TABLE_IDS)
def test_select_is_exact(dt, case):
    """One key's score is 0, every other at most -128: O[i] = V[a_i], lse = 0, dV[j] = the sum of dO over the queries that target j,
    dQ = dK = 0 - bit for bit."""
    c = built("select", dt, case)
    got, route = launch(c, dt)
    assert A.compare(c, got) == 0.0
    print("select %s %s %s: exact" % (NAME[dt], case, route))


@pytest.mark.parametrize("dt,case", A.SHIFTED_CASES, ids=["%s-%s" % (NAME[dt], A.case_id(c)) for dt, c in A.SHIFTED_CASES])
def test_select_shifted_is_exact(dt, case):
    """Without the constant block the top score stays where it is (several hundred): lse must equal it exactly, everything else as before."""
    c = built("select", dt, case, True)
    got, _ = launch(c, dt)
    assert A.compare(c, got) == 0.0


@pytest.mark.parametrize("dt,case", A.TABLE, ids=TABLE_IDS)
def test_pair_forward_exact_backward_within_b(dt, case):
    """P = 1/2, 1/2.  (Whether the 16-bit gradients come out equal bit for bit as well is printed, not required: the backward's P is
    exp(s - lse) of a rounded lse.)"""
    c = built("pair", dt, case)
    got, route = launch(c, dt)
    exact = all(torch.equal(got[x], A.expected(c.ref[x], dt)) for x in ("dq", "dk", "dv"))
    worst = A.compare(c, got)
    print("pair %s %s %s: worst error / bound %.4f, gradients %s" % (NAME[dt], case, route, worst, "bit-exact" if exact else "within B"))


@pytest.mark.parametrize("dt,case", A.TABLE, ids=TABLE_IDS)
def test_dense_within_the_derived_bounds(dt, case):
    """Gaussian operands against float64, every element within its own bound, no share of outliers."""
    c = built("dense", dt, case)
    got, route = launch(c, dt)
    ratios = {}
    for x in ("o", "lse", "dq", "dk", "dv"):
        ref = c.lse if x == "lse" else c.ref[x]
        ratios[x] = float(((got[x].double() - ref).abs() / c.bound[x]).max())
    print("dense %s %s %s: error / bound %s" % (NAME[dt], case, route, " ".join("%s %.3f" % kv for kv in ratios.items())))
    A.compare(c, got)


def test_every_admitted_route_ran():
    """Every pair of kernels the table stands for (the CPU harness shows these are all the dispatch admits) has been launched - by the
    tests above, or here where they did not run in this process."""
    for dt, case in A.TABLE:
        if (dt != F32, L.attention_route(*case[:4], ops.sp_dtype(dt))) not in SEEN:
            c = built("select", dt, case)
            assert A.compare(c, launch(c, dt)[0]) == 0.0
    assert {r for _, r in SEEN} == {("mfma", "mfma"), ("mfma", "valu tq32"), ("mfma", "valu tq16"), ("valu tq32",) * 2, ("valu tq16",) * 2}
    assert {r for sixteen, r in SEEN if not sixteen} == {("valu tq32",) * 2, ("valu tq16",) * 2}


@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
def test_autograd_node_around_a_filled_destination_equals_the_plain_call(dt):
    """models._GeneratorPair.attention: one launch over a batch of two groups (ops.attention_raw), then ops.attention_core around the
    first group's slice and its lse rows.  Output and the three gradients equal those of the plain call on the first group."""
    g = torch.Generator().manual_seed(3)
    groups, hq, wq, hk, wk, d, dv = 2, 10, 10, 12, 8, 32, 64
    mk = lambda h, w, c, s=1.0: (torch.randn(2 * groups, h, w, c, generator=g) * s).to(dt).to(DEV).permute(0, 3, 1, 2)     # noqa: E731
    q, k, v = mk(hq, wq, d, 0.7), mk(hk, wk, d, 0.7), mk(hk, wk, dv)
    do = mk(hq, wq, dv)[:groups]
    o, lse = ops.attention_raw(q, k, v)
    qa, ka, va = (t[:groups].detach().requires_grad_(True) for t in (q, k, v))
    oa = ops.attention_core(qa, ka, va, ops.Dest(o[:groups], True, lse[:groups]))
    oa.backward(do)
    qb, kb, vb = (t[:groups].detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (q, k, v))
    ob = ops.attention_core(qb, kb, vb)
    ob.backward(do)
    assert torch.equal(oa, ob) and torch.equal(o[:groups], ob)
    for a, b in ((qa, qb), (ka, kb), (va, vb)):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    assert float(qa.grad.float().abs().max()) > 0
