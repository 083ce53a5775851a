"""The harness of tests/test_gpu_attention_exact.py checked against itself on the CPU (tests/attention_exact_util.py): every case of
the table meets the conditions its regime rests on, the fp32 restatement of the kernels' arithmetic passes all three regimes, the
comparison rejects the faults the tests exist to catch, and the table reaches every pair of kernels the dispatch admits
(sp_attention_route: host-only)."""
import ctypes
import functools

import pytest
import torch

import attention_exact_util as A
from semantic_pyramid_for_image_generation_amd import _lib as L

BF16, F16, F32 = A.BF16, A.F16, A.F32
SP = {BF16: L.SP_BF16, F16: L.SP_F16, F32: L.SP_F32}
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
SLAB = {"mfma": 64, "valu tq32": 32, "valu tq16": 16}
TABLE_IDS = ["%s-%s" % (NAME[dt], A.case_id(c)) for dt, c in A.TABLE]


@functools.lru_cache(maxsize=None)
def built(regime, dt, case, shifted=False):
    return A.build(regime, dt, case, shifted)


def slab_of(dt, case) -> int:
    n, nk, d, dv, _ = case
    return SLAB[L.attention_route(n, nk, d, dv, SP[dt])[1]]


@functools.lru_cache(maxsize=None)
def _restated(dt, case):
    """regime -> the restatement's worst ratio of error to bound, after every check of the case."""
    worst = {}
    for regime in ("select", "pair", "dense"):
        c = built(regime, dt, case)
        if regime != "dense":
            assert c.gap >= 128 and 2.0 ** -8 <= c.density <= 0.25
            for x in ("o", "dq", "dk", "dv"):
                assert torch.equal(A.expected(c.ref[x], dt).double(), c.ref[x]), (c.what, x)
        if regime == "pair":
            assert max(float(c.bound[x].max()) for x in ("o", "dq", "dk", "dv")) < A.B_MAX
            assert float(c.ref.p.max()) == (0.5 if bool((c.a != c.b).all()) else 1.0)
        got = A.restate(c, slab=slab_of(dt, case))
        worst[regime] = A.compare(c, got)
        if regime == "pair" and dt != F32:
            for x in ("dq", "dk", "dv"):                              # (on the CPU the rounded results come out exact as well)
                A.assert_exact(got[x], A.expected(c.ref[x], dt), c.what)
    return worst


@pytest.mark.parametrize("dt,case", A.TABLE, ids=TABLE_IDS)
def test_conditions_hold_and_the_restatement_passes(dt, case):
    """Building a case asserts its conditions (exact operands, integer scores, a single maximum at 0, exp(-gap) == 0 in fp32, the
    float64 softmax within 1e-40 of the indicator, every reference value representable, B < 1/8); the kernels' arithmetic restated
    in fp32 - P from lse; P, dS and the results rounded to the storage type; slabs added in block order - then passes the comparison."""
    worst = _restated(dt, case)
    assert worst["select"] == 0.0                                       # nothing in this regime is compared through a bound
    assert worst["pair"] <= 0.01                                        # only lse: |fl32(ln 2) - ln 2| against 2^-20
    assert worst["dense"] <= 1.0


@pytest.mark.parametrize("dt,case", A.SHIFTED_CASES, ids=["%s-%s" % (NAME[dt], A.case_id(c)) for dt, c in A.SHIFTED_CASES])
def test_shifted_selection_keeps_its_top_score_in_lse(dt, case):
    c = built("select", dt, case, True)
    assert float(c.lse.min()) >= 128 and torch.equal(c.lse, c.lse.round())
    assert A.compare(c, A.restate(c, slab=slab_of(dt, case))) == 0.0
    got = A.restate(c)
    got.lse = got.lse - c.lse.float()                                   # an lse that forgot the maximum it subtracted
    with pytest.raises(AssertionError, match="elements differ"):
        A.compare(c, got, parts=("lse",))


def test_restatement_stays_within_every_bound_over_the_table():
    """The figures of DESIGN.md section 2: the restatement's worst error / bound over the table, per regime and storage type.  It does
    not stay below half of the dense bound - u is half the unit roundoff, so two roundings that line up use the whole first term
    (attention_exact_util's docstring) - and the bound was left as tight as that."""
    worst = {}
    for dt, case in A.TABLE:
        for regime, w in _restated(dt, case).items():
            worst[(regime, NAME[dt])] = max(worst.get((regime, NAME[dt]), 0.0), w)
    print("restatement, worst error / bound: " + ", ".join("%s %s %.3f" % (r, n, w) for (r, n), w in sorted(worst.items())))
    assert all(w <= 1.0 for w in worst.values()), worst          # (recorded: dense 0.884 bf16, 0.912 fp16, 0.550 fp32; pair 0.002)
    assert all(w == 0.0 for (r, _), w in worst.items() if r == "select"), worst


# ----------------------------------------------------------------------------------------------
# planted faults
# ----------------------------------------------------------------------------------------------
FAULT_CASES = [(BF16, (100, 96, 32, 64, 3)), (F16, (70, 256, 64, 160, 1)), (F32, (37, 16, 8, 12, 2)), (BF16, (1024, 256, 64, 256, 1))]
FAULT_IDS = ["%s-%s" % (NAME[dt], A.case_id(c)) for dt, c in FAULT_CASES]


def _with(c, **kw):
    out = A.Case(c)
    out.update(kw)
    return out


def _rejected(c, got, parts=("o", "lse", "dq", "dk", "dv")):
    with pytest.raises(AssertionError, match="elements differ"):
        A.compare(c, got, parts)


@pytest.mark.parametrize("regime", ["select", "pair", "dense"])
@pytest.mark.parametrize("dt,case", FAULT_CASES, ids=FAULT_IDS)
def test_planted_faults_are_rejected(dt, case, regime):
    c = built(regime, dt, case)
    n, nk, d, dv, batch = case
    slab = slab_of(dt, case)
    good = A.restate(c, slab=slab)
    A.compare(c, good)
    # 1. two keys swapped inside a 32-key step, in V only (the P registers and the V fragments disagree about the key order)
    j1 = int(c.a[0, 0]) if regime != "dense" else 5
    j2 = j1 ^ 16 if (j1 ^ 16) < nk else j1 ^ 1
    assert j1 // 32 == j2 // 32
    v2 = c.v.clone()
    v2[:, [j1, j2]] = c.v[:, [j2, j1]]
    assert not torch.equal(v2, c.v)
    bad = A.restate(_with(c, v=v2), slab=slab)
    _rejected(c, bad, ("o",))
    if regime != "select":
        _rejected(c, bad, ("dq", "dk"))                                 # (in a selection dP cancels exactly, whatever V holds)
    # 2. the last query of a ragged tail missing from dK / dV
    assert float(c.do[:, -1].abs().sum()) > 0
    short = A.restate(_with(c, q=c.q[:, :-1], do=c.do[:, :-1]), slab=slab)
    _rejected(c, _with(good, dk=short.dk, dv=short.dv), ("dk", "dv"))
    _rejected(c, _with(good, dv=short.dv), ("dv",))
    # 3. a row past N counted: the clamped load makes it the last query once more
    twice = A.restate(_with(c, q=torch.cat((c.q, c.q[:, -1:]), 1), do=torch.cat((c.do, c.do[:, -1:]), 1)), slab=slab)
    _rejected(c, _with(good, dk=twice.dk, dv=twice.dv), ("dk", "dv"))
    # 4. one slab left out of the sum
    if n > slab:
        for skip in (0, len(good.dv_slabs) - 1):
            dvs = [s for i, s in enumerate(good.dv_slabs) if i != skip]
            dks = [s for i, s in enumerate(good.dk_slabs) if i != skip]
            _rejected(c, _with(good, dv=sum(dvs[1:], dvs[0]).to(dt)), ("dv",))
            if regime != "select":
                _rejected(c, _with(good, dk=sum(dks[1:], dks[0]).to(dt)), ("dk",))
    # 5. the log-sum-exp of the neighbouring query: stored one row off by the forward, read one row off by the backward.  Visible
    #    where neighbouring rows differ in lse: always in the dense regime; a selection's rows all hold 0.
    if regime == "dense" and n > 1:
        _rejected(c, _with(good, lse=good.lse.roll(1, 1)), ("lse",))
        off = A.restate(c, lse_from=good.lse.roll(1, 1), slab=slab)
        for x in ("dq", "dk", "dv"):
            _rejected(c, off, (x,))


def test_a_single_misplaced_product_cannot_hide_in_the_pair_bound():
    """B < 1/8 and every non-zero term of dQ is a multiple of 1/4: one term of one element taken out is rejected."""
    c = built("pair", F32, (100, 96, 32, 64, 3))
    good = A.restate(c)
    A.compare(c, good)
    terms = (c.ref.ds.unsqueeze(3) * c.k.unsqueeze(1))                  # [b][i][j][d]
    idx = (terms != 0).nonzero()
    assert len(idx) > 100 and float(terms[terms != 0].abs().min()) >= 0.25
    for b_, i, j, dd in idx[:: len(idx) // 25].tolist():
        dq = good.dq.clone()
        dq[b_, i, dd] -= float(terms[b_, i, j, dd])
        with pytest.raises(AssertionError, match="1 of .* elements differ"):
            A.compare(c, _with(good, dq=dq), ("dq",))


# ----------------------------------------------------------------------------------------------
# routes
# ----------------------------------------------------------------------------------------------
def _slabs(n, nk, d, dv, sp) -> int:
    out = ctypes.c_int64(-1)
    L.call("sp_attention_bwd_slabs", n, nk, d, dv, sp, ctypes.byref(out))
    return out.value


def test_the_table_reaches_every_route_the_dispatch_admits():
    """Every (forward, backward) pair of kernels that sp_attention_route names anywhere on a grid over the supported extents is the
    route of at least one case of the table, per storage class; the slab count agrees with the backward's route for every case."""
    reached = {(dt != F32, L.attention_route(c[0], c[1], c[2], c[3], SP[dt])) for dt, c in A.TABLE}
    admitted = set()
    for sp in (L.SP_BF16, L.SP_F16, L.SP_F32):
        for nk in (1, 15, 16, 31, 32, 33, 48, 64, 96, 128, 224, 255, 256):
            for d in (1, 8, 16, 31, 32, 33, 48, 64):
                for dv in range(1, 257):
                    admitted.add((sp != L.SP_F32, L.attention_route(70, nk, d, dv, sp)))
    names = {"mfma", "valu tq32", "valu tq16"}
    assert all(f in names and b in names for _, (f, b) in admitted)
    assert admitted - reached == set(), "routes no case reaches: %s" % sorted(admitted - reached)
    assert reached - admitted == set()
    # what the dispatch admits: the VALU kernels share their query count, the MFMA backward implies the MFMA forward, fp32 is VALU only
    assert admitted == {(True, ("mfma", "mfma")), (True, ("mfma", "valu tq32")), (True, ("mfma", "valu tq16")),
                        (True, ("valu tq32", "valu tq32")), (True, ("valu tq16", "valu tq16")),
                        (False, ("valu tq32", "valu tq32")), (False, ("valu tq16", "valu tq16"))}
    for dt, c in A.TABLE:
        n, nk, d, dv, _ = c
        bwd = L.attention_route(n, nk, d, dv, SP[dt])[1]
        assert _slabs(n, nk, d, dv, SP[dt]) == -(-n // SLAB[bwd]), (NAME[dt], c, bwd)
    # the two 16-bit flavours route alike
    for _, c in A.TABLE:
        assert L.attention_route(*c[:4], L.SP_BF16) == L.attention_route(*c[:4], L.SP_F16)


def test_the_table_rows_carry_the_routes_their_labels_promise():
    route = lambda c, dt: L.attention_route(*c[:4], SP[dt])                                                # noqa: E731
    assert all(route(c, dt) == ("mfma", "mfma") for c in A.MFMA_CASES for dt in (BF16, F16))
    assert all(route(c, BF16)[0] == "mfma" and route(c, BF16)[1].startswith("valu") for c in A.MIXED_CASES)
    assert [route(c, BF16)[1] for c in A.MIXED_CASES] == ["valu tq32"] * 3 + ["valu tq16"]
    assert [route(c, F16) for c in A.VALU_CASES] == [("valu tq32",) * 2] * 3 + [("valu tq16",) * 2]
    assert [route(c, F32) for c in A.F32_CASES] == [("valu tq32",) * 2] * 3 + [("valu tq16",) * 2]


def test_route_query_rejects_what_the_launchers_reject():
    f, b = ctypes.c_char_p(), ctypes.c_char_p()
    lib = L.lib()
    for n, nk, d, dv in ((64, 257, 32, 32), (64, 32, 65, 32), (64, 32, 32, 257), (0, 32, 32, 32), (64, 0, 32, 32)):
        assert lib.sp_attention_route(n, nk, d, dv, L.SP_BF16, ctypes.byref(f), ctypes.byref(b)) == -1, (n, nk, d, dv)
    assert lib.sp_attention_route(64, 32, 32, 32, L.SP_BF16, None, ctypes.byref(b)) == -1
    assert lib.sp_attention_route(64, 32, 32, 32, L.SP_F8, ctypes.byref(f), ctypes.byref(b)) == -1
    with pytest.raises(L.SempyrError, match="sp_attention_route"):
        L.attention_route(64, 300, 32, 32, L.SP_F32)
