"""The MFMA attention kernels with a block walking several query blocks (csrc/attention.hip: attn_fwd_mfma_kernel,
attn_bwd_res_kernel), the piece count forced through SP_TUNE_ATTN_PIECES: the selection regime bit for bit and the dense regime inside
the derived bounds of tests/attention_exact_util.py, on the canary-guarded buffers of tests/test_gpu_attention_exact.py.  The scratch
is sized for one slab per query block as ops.py sizes it and starts as NaN: the slabs past the plan's count must still be NaN after the
call (neither written nor read), the ones before it fully written."""
import ctypes

import pytest
import torch

import attention_exact_util as A
from test_gpu_attention_exact import BF16, F16, F32, NAME, Guarded, _dev, built
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

KEY = L.TUNE_KEYS["SP_ATTN_PIECES"]
# ((n, nk, d, dv, batch), pieces forced)
FORCED = [
    ((128, 32, 32, 32, 1), 1),            # two iterations with carried accumulators
    ((130, 256, 32, 128, 2), 1),          # the workload's layout at its LDS size; the last query block has 2 live queries
    ((130, 256, 32, 128, 2), 2),          # pieces of unequal length (2 + 1)
    ((130, 256, 32, 128, 2), 3),
    ((200, 96, 32, 64, 3), 3),            # a walk of 2, 2 pieces; slab offsets use the batch
    ((65, 64, 64, 32, 1), 4),             # the count clamps to the 2 query blocks, no piece is empty (D = 64: a slab per query block)
]
WORKLOAD = (1024, 256, 32, 128, 20)
FORWARD = ((1024, 256, 32, 128, 3), 8)
IDS = ["%s-%s-p%d" % (NAME[dt], A.case_id(c), p) for c, p in FORCED for dt in (BF16, F16)]
TABLE = [(dt, c, p) for c, p in FORCED for dt in (BF16, F16)]


def div_up(a, b):
    return -(-a // b)


def plan(c, dt, cus=0):
    n, nk, d, dv, b = c.dims
    f, w, s = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    L.call("sp_attention_plan", b, n, nk, d, dv, ops.sp_dtype(dt), cus, ctypes.byref(f), ctypes.byref(w), ctypes.byref(s))
    return f.value, w.value, s.value


def launch(c, dt, pieces):
    """Forward and backward with the piece count forced (None: the plan).  Returns the five results on the host and the plan."""
    n, nk, d, dv, b = c.dims
    sp = ops.sp_dtype(dt)
    assert L.attention_route(n, nk, d, dv, sp) == ("mfma", "mfma"), c.what
    nqb = div_up(n, 64)
    slabs = ctypes.c_int64(-1)
    L.call("sp_attention_bwd_slabs", n, nk, d, dv, sp, ctypes.byref(slabs))
    assert slabs.value == nqb, (c.what, slabs.value)
    q, k, v, do = (_dev(c[x], dt) for x in ("q", "k", "v", "do"))
    o, lse, dq = Guarded(b * n, dv, dt), Guarded(b * n, 1, F32), Guarded(b * n, d, dt)
    dk, dvv = Guarded(b * nk, d, dt), Guarded(b * nk, dv, dt)
    dk32 = Guarded(nqb * b * nk, d, F32, float("nan"))
    dv32 = Guarded(nqb * b * nk, dv, F32, float("nan"))
    try:
        if pieces is not None:
            L.call("sp_set_tuning", KEY, pieces)
        fw, bw, used = plan(c, dt)
        L.call("sp_attention_fwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(o.t), ops.ptr(lse.t), b, n, nk, d, dv, sp, ops.stream())
        L.call("sp_attention_bwd", ops.ptr(q), ops.ptr(k), ops.ptr(v), ops.ptr(do), ops.ptr(lse.t), ops.ptr(dq.t), ops.ptr(dk32.t),
               ops.ptr(dv32.t), ops.ptr(dk.t), ops.ptr(dvv.t), b, n, nk, d, dv, sp, ops.stream())
        torch.cuda.synchronize()
    finally:
        L.lib().sp_set_tuning(KEY, -1)
    for name, g in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dvv), ("dk slabs", dk32), ("dv slabs", dv32)):
        g.check((c.what, name))
    for name, g in (("dk", dk32), ("dv", dv32)):
        nan = torch.isnan(g.t.cpu())
        assert not bool(nan[:used * b * nk].any()), (c.what, name, "a slab the reduction adds holds a NaN")
        assert bool(nan[used * b * nk:].all()), (c.what, name, "a slab past the plan's count was written")
    got = A.Case(o=o.t.cpu().view(b, n, dv), lse=lse.t.cpu().view(b, n), dq=dq.t.cpu().view(b, n, d), dk=dk.t.cpu().view(b, nk, d),
                 dv=dvv.t.cpu().view(b, nk, dv))
    return got, (fw, bw, used)


def forced_plan(case, pieces):
    """What the issue's table says the forced count comes to: the walk, and the slabs in use."""
    n, _, d, _, _ = case
    nqb = div_up(n, 64)
    walk = div_up(nqb, min(max(pieces, 1), nqb))
    return walk, (walk if d == 32 else 0), div_up(nqb, walk) if d == 32 else nqb


@pytest.mark.parametrize("dt,case,pieces", TABLE, ids=IDS)
def test_select_is_exact_for_a_forced_piece_count(dt, case, pieces):
    c = built("select", dt, case)
    got, p = launch(c, dt, pieces)
    assert p == forced_plan(case, pieces), (case, pieces, p)
    assert A.compare(c, got) == 0.0


@pytest.mark.parametrize("dt,case,pieces", TABLE, ids=IDS)
def test_dense_within_the_derived_bounds_for_a_forced_piece_count(dt, case, pieces):
    c = built("dense", dt, case)
    got, p = launch(c, dt, pieces)
    assert p == forced_plan(case, pieces), (case, pieces, p)
    print("dense %s %s pieces %d plan %s: worst error / bound %.3f" % (NAME[dt], case, pieces, p, A.compare(c, got)))


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_the_workloads_plan_selects_exactly(dt):
    """Batch 20 of the workload's shape on the plan itself: 320 query blocks, a walk of 2, 8 of the 16 slabs in use."""
    c = built("select", dt, WORKLOAD)
    assert plan(c, dt, 256) == (1, 2, 8)
    got, p = launch(c, dt, None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert p == plan(c, dt, cus), (p, cus)
    assert A.compare(c, got) == 0.0


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("regime", ["select", "dense"])
def test_forward_walking_two_query_blocks(regime, dt):
    case, pieces = FORWARD
    c = built(regime, dt, case)
    got, p = launch(c, dt, pieces)
    assert p == (2, 2, 8), p
    worst = A.compare(c, got)
    assert regime == "dense" or worst == 0.0
