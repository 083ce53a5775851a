"""Operands, float64 references and comparisons for the tests of the attention kernels (tests/test_gpu_attention_exact.py; the
self-test of everything here: tests/test_attention_harness.py).  Everything in this module runs on the CPU.

o = softmax(q k^T) v with q [b][n][d], k [b][nk][d], v [b][nk][dv]; lse [b][n] is the row's log-sum-exp.  Three regimes:

select   the softmax is an exact SELECTION.  Key j carries the bits of j as +-1 over nb = ceil(log2 nk) dimensions, repeated `rep`
         times inside the first 3d/4 dimensions; the last d/4 dimensions of every key are 1.  Query i is scale x code(a_i) for a
         random target key a_i and holds -top / (d/4) in its last d/4 entries, so the score of key j is
         -2 x rep x scale x hamming(a_i, j): 0 for the target, <= -gap (gap = 2 x rep x scale >= 128) for every other key.
         exp(-gap) underflows to 0 in fp32, the sum is 1, P is one-hot and lse is 0: O[i] = V[a_i], dV[j] = sum of dO[i] over the
         queries that target j, dQ = 0, dK = 0 - torch.equal, no tolerance.  `shifted` drops the constant block of the queries:
         the scores keep their top value and lse must equal it exactly (the max subtraction).
pair     the query is scale/2 x (code(a) + code(b)) with b one bit away from a (b = a where that key does not exist): two scores
         are 0, the rest <= -gap, P = 1/2, 1/2.  The forward is exact in 16-bit storage; the backward recomputes P as
         exp(s - lse) from a rounded lse with the fast exp / log, so P is 1/2 only to about 2^-21 and the gradients (and the fp32
         forward) get the bound B = 2^-18 x T per element, T the float64 sum of the magnitudes of the element's terms
         (2^-21 compounded over the three places P enters, with a factor 2 on top).  B < 1/8, half the smallest non-zero term.
dense    Gaussian operands rounded through the storage type against float64, per-element bounds built from the float64
         reference's own magnitudes (dense_case).  No share of outliers.

How far the dense bounds reach (measured by the restatement below, nothing tuned on a GPU).  u = 2^-9 (bf16) / 2^-12 (fp16) is HALF
the unit roundoff of the type: a round-to-nearest of x in [1, 2) is off by up to 2^-9 of 2, that is 2u of x.  So the two roundings a
result goes through (P or dS once, the result once) take the whole first term, 2 x 2u x T, in the worst case: the leading 2 is no
margin there, and errors that line up reach it (the restatement: 0.91 of the bound).  The second term keeps its margin: s, lse and
s - lse are each rounded once to fp32 at a magnitude below 32 (asserted), 3 x 2^-20 < 2^-18 of P, against the 2 x 2^-18 granted (the
restatement in fp32 storage: 0.55)."""
import math

import torch

import exact_util as X
from exact_util import Case, assert_exact, check_reference, expected   # noqa: F401  (the exact tests' comparison, reused)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U = {BF16: 2.0 ** -9, F16: 2.0 ** -12, F32: 0.0}       # half the unit roundoff of the storage type (fp32: nothing is rounded to storage)
ETA = {BF16: 0.0, F16: 2.0 ** -25, F32: 0.0}           # half the smallest subnormal: fp16 rounds values below 2^-14 absolutely
EPS = 2.0 ** -18                                       # pair / dense: what the fp32 exp / log and a rounded lse leave of P, relative
LSE_PAIR = 2.0 ** -20                                  # pair: |lse - ln 2|
B_MAX = 0.125                                          # pair: the bound stays below half the smallest non-zero term (1/4)

# (n, nk, d, dv, batch): the smallest shapes that reach each path and edge of csrc/attention.hip
MFMA_CASES = [
    (64, 32, 32, 32, 1),          # two key fragments: waves 2 and 3 of the backward's phase 3 own none
    (1, 32, 32, 32, 1),           # N = 1
    (17, 64, 64, 32, 2),          # one live query in wave 1
    (100, 96, 32, 64, 3),         # ragged wave and block; slab offsets use the batch
    (130, 256, 32, 128, 2),       # V staged in LDS by the backward, at equality of its size test
    (70, 256, 64, 160, 1),        # V from global memory; partial second dV pass
    (65, 224, 64, 256, 2),        # 14 key fragments over 4 waves; two full dV passes
    (1024, 256, 64, 256, 1),      # the workload's shape: 16 slabs
]
MIXED_CASES = [                   # MFMA forward, VALU backward (dv % 32 == 16): the backward gets an lse of the fast exp / log
    (100, 64, 32, 48, 2),
    (33, 32, 64, 16, 1),
    (40, 96, 32, 240, 1),
    (40, 256, 64, 240, 1),        # ... and the backward in its 16-query form (the only such shapes: nk = 256, d = 64, dv >= 208)
]
VALU_CASES = [
    (37, 16, 8, 12, 2),
    (64, 48, 32, 32, 1),          # nk % 32 != 0 although d would suit the MFMA
    (20, 255, 16, 4, 1),
    (40, 256, 64, 200, 1),        # 16 queries per block
]
F32_CASES = [
    (37, 16, 8, 12, 2),
    (100, 96, 32, 64, 3),
    (40, 256, 64, 176, 1),        # 32 queries per block at the LDS limit: 163 456 B
    (40, 256, 64, 192, 1),        # 16 queries per block: 32 would need 165 504 B
]
CASES_16 = MFMA_CASES + MIXED_CASES + VALU_CASES
SHIFTED_CASES = [(BF16, MFMA_CASES[3]), (F16, MFMA_CASES[6]), (BF16, VALU_CASES[0]), (F32, F32_CASES[0])]
TABLE = [(dt, c) for c in CASES_16 for dt in (BF16, F16)] + [(F32, c) for c in F32_CASES]


def case_id(c):
    return "-".join(str(a) for a in c)


# ----------------------------------------------------------------------------------------------
# float64 attention and its gradients, every intermediate kept
# ----------------------------------------------------------------------------------------------
def attention64(q, k, v, do, p=None) -> Case:
    """Everything of o = softmax(q k^T) v and its backward in float64.  p: the probabilities, where they are known exactly."""
    s = q @ k.transpose(1, 2)
    lse = torch.logsumexp(s, 2)
    if p is None:
        p = torch.exp(s - lse.unsqueeze(2))
    o = p @ v
    dp = do @ v.transpose(1, 2)
    drow = (p * dp).sum(2, keepdim=True)
    ds = p * (dp - drow)
    return Case(s=s, lse=lse, p=p, o=o, dp=dp, drow=drow, ds=ds, dq=ds @ k, dk=ds.transpose(1, 2) @ q, dv=p.transpose(1, 2) @ do)


def term_sums(r: Case, q, k, v, do) -> Case:
    """Per element of each result, the float64 sum of the magnitudes of its terms (what an error relative to P or dS multiplies)."""
    w = r.p * (r.dp.abs() + r.drow.abs())                       # |terms| of dS: P (|dP| + |Drow|)
    return Case(o=r.p @ v.abs(), dv=r.p.transpose(1, 2) @ do.abs(), dq_p=w @ k.abs(), dk_p=w.transpose(1, 2) @ q.abs(),
                dq_s=r.ds.abs() @ k.abs(), dk_s=r.ds.abs().transpose(1, 2) @ q.abs(),
                lse=(r.p * (q.abs() @ k.abs().transpose(1, 2))).sum(2))


def _held(t, dtype) -> bool:
    return torch.equal(t.to(dtype).double(), t)


# ----------------------------------------------------------------------------------------------
# select / pair: codes
# ----------------------------------------------------------------------------------------------
def code_plan(nk: int, d: int):
    """(nb, rep, scale, gap, cb): bits per key, repetitions inside the first 3d/4 dimensions, the power-of-two query scale with
    gap = 2 x rep x scale >= 128, the width of the constant block."""
    assert d % 4 == 0 and nk >= 2, (nk, d)
    nb = max(1, math.ceil(math.log2(nk)))
    rep = (3 * d // 4) // nb
    assert rep >= 1, ("the code of %d keys does not fit 3/4 of %d dimensions" % (nk, d))
    scale = 1
    while 2 * rep * scale < 128:
        scale *= 2
    return nb, rep, scale, 2 * rep * scale, d // 4


def codes(idx: torch.Tensor, nb: int, rep: int, d: int) -> torch.Tensor:
    """[..., d] float64: bit t of idx as +-1 (set: +1) at dimensions r * nb + t for r < rep, 0 elsewhere."""
    bits = ((idx.unsqueeze(-1) >> torch.arange(nb)) & 1).double() * 2 - 1
    out = torch.zeros(tuple(idx.shape) + (d,), dtype=torch.float64)
    out[..., :rep * nb] = bits.repeat(*([1] * idx.dim()), rep)
    return out


def coded_case(regime, dtype, n, nk, d, dv, batch, shifted=False, seed=0) -> Case:
    """Operands, exact P and float64 reference of the select / pair regime, with every condition the regime rests on asserted."""
    assert regime in ("select", "pair") and not (shifted and regime == "pair"), (regime, shifted)
    what = (regime + ("-shifted" if shifted else ""), str(dtype), n, nk, d, dv, batch)
    g = X.gen(seed + 7 * n + nk + d + dv)
    nb, rep, scale, gap, cb = code_plan(nk, d)
    k = codes(torch.arange(nk), nb, rep, d).expand(batch, nk, d).clone()
    k[..., d - cb:] = 1.0
    a = torch.randint(0, nk, (batch, n), generator=g)
    if regime == "pair":
        b = a ^ (1 << torch.randint(0, nb, (batch, n), generator=g))
        b = torch.where(b < nk, b, a)
    else:
        b = a
    q = 0.5 * scale * (codes(a, nb, rep, d) + codes(b, nb, rep, d))
    top = scale * rep * (nb - (a != b).double())                                 # the score of keys a and b before the shift
    if not shifted:
        q[..., d - cb:] = (-top / cb).unsqueeze(-1)
    v = X.ternary((batch, nk, dv), g)
    p = torch.zeros(batch, n, nk, dtype=torch.float64)
    p.scatter_(2, a.unsqueeze(2), 0.5)
    p.scatter_add_(2, b.unsqueeze(2), torch.full((batch, n, 1), 0.5, dtype=torch.float64))
    # scores: integers, the maximum reached by the targets alone, everything else at least `gap` below
    s = q @ k.transpose(1, 2)
    best = top if shifted else torch.zeros_like(top)
    assert torch.equal(s, s.round()) and torch.equal(s.amax(2), best), (what, "scores")
    assert torch.equal(s == best.unsqueeze(2), p > 0), (what, "the maximum is reached by another key")
    assert float((s - best.unsqueeze(2))[p == 0].max()) <= -gap, (what, "gap")
    assert gap >= 128 and float(torch.exp(torch.tensor(-float(gap), dtype=F32))) == 0.0, (what, gap)
    assert float((torch.softmax(s, 2) - p).abs().max()) <= 1e-40, (what, "the float64 softmax is not the indicator")
    for name, t in (("q", q), ("k", k), ("v", v)):
        assert _held(t, dtype), (what, "%s is not held exactly by the storage type" % name)
    density = 0.25
    while True:                                            # dO: ternary, thinned until every reference value is representable
        gd = X.gen(seed + 1000 + n + dv)
        do = X.ternary((batch, n, dv), gd) * (torch.rand(batch, n, dv, generator=gd) < density * 1.5).double()
        r = attention64(q, k, v, do, p)
        t = term_sums(r, q, k, v, do)
        bound = Case(o=EPS * t.o, dq=EPS * t.dq_p, dk=EPS * t.dk_p, dv=EPS * t.dv)
        ok = all(_held(r[x], dtype) for x in ("o", "ds", "dq", "dk", "dv"))
        if regime == "pair":
            ok = ok and max(float(bound[x].max()) for x in ("o", "dq", "dk", "dv")) < B_MAX
        if ok:
            break
        density /= 2
        assert density >= 2.0 ** -8, (what, "no dO density makes the reference representable")
    assert float(do.abs().sum()) > 0, (what, "dO is empty")
    lse = (best + math.log(2.0) * (a != b).double())
    assert float((r.lse - lse).abs().max()) <= 1e-12, what
    if regime == "select":
        assert torch.equal(r.o, torch.gather(v, 1, a.unsqueeze(2).expand(batch, n, dv))), what
        assert float(r.dq.abs().max()) == 0 and float(r.dk.abs().max()) == 0, what
        want_dv = torch.zeros(batch, nk, dv, dtype=torch.float64).index_put_(
            (torch.arange(batch).unsqueeze(1).expand(batch, n), a), do, accumulate=True)
        assert torch.equal(r.dv, want_dv), what
    else:
        assert torch.equal(r.ds * 4, (r.ds * 4).round()), (what, "dS is no multiple of 1/4")
    return Case(regime=regime, shifted=shifted, what=what, dtype=dtype, q=q, k=k, v=v, do=do, a=a, b=b, ref=r, lse=lse, bound=bound,
                gap=gap, density=density, dims=(n, nk, d, dv, batch))


# ----------------------------------------------------------------------------------------------
# dense
# ----------------------------------------------------------------------------------------------
def dense_case(dtype, n, nk, d, dv, batch, seed=0) -> Case:
    """Gaussian q, k (x 0.7), v, dO rounded through the storage type; the float64 reference and the per-element bounds

    (u = 2^-9 bf16, 2^-12 fp16, 0 fp32)

        O    2 (2u + 2^-18) sum_j P |V|                    P rounded once, the result rounded once, exp / log noise
        dV   2 (2u + 2^-18) sum_i P |dO|
        dQ   2 (2u sum_j |dS| |K| + 2^-18 sum_j P (|dP| + |Drow|) |K|)       dS rounded once, the result once; noise of P inside dS
        dK   as dQ with Q and the sum over i
        lse  2 x 2^-18 (1 + |lse| + sum_j P_j sum_c |q_c| |k_jc|)

    lse: d lse / d s_j = P_j and an fp32 score of d <= 64 products is off by at most 64 x 2^-24 = 2^-18 of sum_c |q_c| |k_jc|; the
    sum of exponentials, its logarithm and the final addition add 2^-18 (1 + |lse|) at the very most.  The leading 2 is the margin
    for the accumulation order.
    subnormals: fp16 rounds a value below 2^-14 with an ABSOLUTE error of up to 2^-25, which u |x| does not cover - and most
    probabilities of a 256-key softmax are that small.  Every bound therefore gains eta x (1 + sum |other operand|) with eta = 2^-25
    in fp16 (0 in bf16, whose subnormals lie below 2^-126): eta per rounded P or dS against the operand it multiplies, eta for the
    result.  Nothing here was tuned on a GPU; the fp32 restatement of the kernels' arithmetic (restate) has to pass every bound
    (tests/test_attention_harness.py; how close it comes and why: the module's docstring)."""
    g = X.gen(seed + 13 * n + nk + d + dv)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dtype).double()      # noqa: E731
    q, k = rnd(batch, n, d, scale=0.7), rnd(batch, nk, d, scale=0.7)
    v, do = rnd(batch, nk, dv), rnd(batch, n, dv)
    r = attention64(q, k, v, do)
    assert float(r.s.abs().max()) < 32 and float(r.lse.abs().max()) < 32, "2^-18 of P assumes scores and lse below 32"
    t = term_sums(r, q, k, v, do)
    u, eta = U[dtype], ETA[dtype]
    sub = lambda other, axis: eta * (1 + other.abs().sum(axis, keepdim=True))      # noqa: E731  (see "subnormals" above)
    bound = Case(o=2 * (2 * u + EPS) * t.o + sub(v, 1), dv=2 * (2 * u + EPS) * t.dv + sub(do, 1),
                 dq=2 * (2 * u * t.dq_s + EPS * t.dq_p) + sub(k, 1), dk=2 * (2 * u * t.dk_s + EPS * t.dk_p) + sub(q, 1),
                 lse=2 * EPS * (1 + r.lse.abs() + t.lse))
    return Case(regime="dense", shifted=False, what=("dense", str(dtype), n, nk, d, dv, batch), dtype=dtype, q=q, k=k, v=v, do=do, ref=r,
                lse=r.lse, bound=bound, dims=(n, nk, d, dv, batch))


def build(regime, dtype, case, shifted=False) -> Case:
    return dense_case(dtype, *case) if regime == "dense" else coded_case(regime, dtype, *case, shifted=shifted)


# ----------------------------------------------------------------------------------------------
# the kernels' arithmetic restated in fp32 torch (what the comparison is tried on without a GPU)
# ----------------------------------------------------------------------------------------------
def restate(c: Case, lse_from=None, slab: int = 64) -> Case:
    """fp32 accumulation throughout; P (forward), P and dS (backward) and the results rounded to the storage type, as the MFMA kernels
    do; the backward takes P from the forward's lse; dK / dV as per-block slabs of `slab` queries added in block order.
    lse_from: the lse the backward uses instead (a planted fault)."""
    dt = c.dtype
    rt = lambda t: t.to(dt).float()                                                                      # noqa: E731
    q, k, v, do = (c[x].float() for x in ("q", "k", "v", "do"))
    s = q @ k.transpose(1, 2)
    m = s.amax(2, keepdim=True)
    e = torch.exp(s - m)
    tot = e.sum(2, keepdim=True)
    o = rt(rt(e / tot) @ v)
    lse = (m + torch.log(tot)).squeeze(2)
    lb = lse if lse_from is None else lse_from
    p = torch.exp(s - lb.unsqueeze(2))
    dp = do @ v.transpose(1, 2)
    ds = p * (dp - (p * dp).sum(2, keepdim=True))
    dq = rt(rt(ds) @ k)
    n = q.shape[1]
    dk_slabs = [rt(ds[:, i:i + slab]).transpose(1, 2) @ q[:, i:i + slab] for i in range(0, n, slab)]
    dv_slabs = [rt(p[:, i:i + slab]).transpose(1, 2) @ do[:, i:i + slab] for i in range(0, n, slab)]
    return Case(o=o.to(dt), lse=lse, dq=dq.to(dt), dk=sum(dk_slabs[1:], dk_slabs[0]).to(dt), dv=sum(dv_slabs[1:], dv_slabs[0]).to(dt),
                dk_slabs=dk_slabs, dv_slabs=dv_slabs)


# ----------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------
AXES = ["image", "row", "channel"]


def assert_within(got, ref, bound, what="", names=None) -> float:
    """|got - ref| <= bound element for element (NaN fails); returns the worst ratio of error to bound.  The message names the pattern
    of the failing elements like assert_exact."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()
        names = names or ["axis%d" % i for i in range(got.dim())]
        axes = []
        for ax, name in enumerate(names):
            uq = idx[:, ax].unique().tolist()
            axes.append("%s: %s" % (name, uq if len(uq) <= 24 else "%d values, %d .. %d" % (len(uq), uq[0], uq[-1])))
        first = ["%s got %r want %r bound %.3g" % (tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)]))
                 for i in idx[:6]]
        raise AssertionError("%s: %d of %d elements differ by more than their bound; %s; first: %s"
                             % (what, int(bad.sum()), got.numel(), "; ".join(axes), " | ".join(first)))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def compare(c: Case, got: Case, parts=("o", "lse", "dq", "dk", "dv")) -> float:
    """got: o, dq, dk, dv in the storage type and lse in fp32, [batch][rows][channels] resp. [batch][n].  select: torch.equal for all
    five.  pair: the forward exact in 16-bit storage, |lse - ln 2| <= 2^-20, B for the gradients and the fp32-storage forward.  dense:
    the bounds of dense_case.  Returns the worst ratio of error to bound among the bounded comparisons (0 where all were exact)."""
    dt, r, worst = c.dtype, c.ref, 0.0
    tag = lambda x: "%s %s" % (c.what, x)                                                                # noqa: E731
    for x in parts:
        assert got[x].dtype == (F32 if x == "lse" else dt), (tag(x), got[x].dtype)
        if x == "lse":
            if c.regime == "select":
                assert_exact(got.lse, c.lse.float(), tag("lse"), AXES[:2])
            else:
                bound = c.bound.lse if c.regime == "dense" else torch.full_like(c.lse, LSE_PAIR)
                worst = max(worst, assert_within(got.lse, c.lse, bound, tag("lse"), AXES[:2]))
        elif c.regime == "select" or (c.regime == "pair" and x == "o" and dt != F32):
            assert_exact(got[x], expected(r[x], dt), tag(x), AXES)
        else:
            worst = max(worst, assert_within(got[x], r[x], c.bound[x], tag(x), AXES))
    return worst
