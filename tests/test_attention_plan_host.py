"""The walk of the MFMA attention kernels (csrc/attention.hip: attn_walk, seen through sp_attention_plan) is a pure function of
(batch, query blocks, CUs, SP_TUNE_ATTN_PIECES): re-derived here and compared over a grid, without a GPU (the CU count is passed in)."""
import ctypes

import pytest

from semantic_pyramid_for_image_generation_amd import _lib as L

KEY = L.TUNE_KEYS["SP_ATTN_PIECES"]
LDS = 160 * 1024


def div_up(a, b):
    return -(-a // b)


def walk(batch, nqb, slots, pieces):
    """The smallest walk that brings batch x ceil(nqb / walk) blocks down to `slots`; a forced piece count clamps to [1, nqb]."""
    if pieces >= 0:
        return div_up(nqb, min(max(pieces, 1), nqb))
    r = 1
    while r < nqb and batch * div_up(nqb, r) > slots:
        r += 1
    return r


def plan(batch, n, nk, d, dv, dtype, cus):
    f, b, s = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    L.call("sp_attention_plan", batch, n, nk, d, dv, dtype, cus, ctypes.byref(f), ctypes.byref(b), ctypes.byref(s))
    return f.value, b.value, s.value


def expect(batch, n, nk, d, dv, cus, pieces):
    nqb = div_up(n, 64)
    fwd_slots = 2 * cus if 2 * nk * (dv * 2 + 32) <= LDS else cus
    res_lds = nk * (d * 2 + 32) + nk * (dv * 2 + 16) + 64 * (d * 2 + 32) + 64 * (dv * 2 + 32) + 2 * 32 * (nk * 2 + 32)
    resident = d == 32 and dv <= 128 and res_lds <= LDS
    bw = walk(batch, nqb, cus, pieces) if resident else 0
    return walk(batch, nqb, fwd_slots, pieces), bw, div_up(nqb, bw) if bw else nqb


@pytest.fixture
def key():
    L.lib()
    yield lambda v: L.call("sp_set_tuning", KEY, v)
    L.lib().sp_set_tuning(KEY, -1)


def test_the_workload_gets_the_plan_it_was_sized_for(key):
    key(-1)
    for dt in (L.SP_BF16, L.SP_F16):
        assert plan(20, 1024, 256, 32, 128, dt, 256) == (1, 2, 8)          # 320 blocks: two per CU forward, a walk of 2 backward
        assert plan(40, 1024, 256, 32, 128, dt, 256) == (2, 3, 6)          # 640 blocks; backward pieces of 3, 3, 3, 3, 3, 1
        assert plan(8, 1024, 256, 32, 128, dt, 256) == (1, 1, 16)          # 128 blocks already fit
    assert plan(20, 1024, 256, 32, 128, L.SP_BF16, 304) == (1, 2, 8)
    assert plan(20, 1024, 256, 32, 128, L.SP_BF16, 64) == (3, 6, 3)


def test_plan_is_a_pure_function_of_batch_blocks_cus_and_the_key(key):
    shapes = [(256, 32, 128), (256, 32, 64), (96, 32, 64), (32, 32, 32), (256, 64, 128), (64, 64, 32), (256, 64, 256)]
    for pieces in (-1, 0, 1, 2, 3, 5, 8, 16, 1000):
        key(pieces)
        for nk, d, dv in shapes:
            for batch in (1, 3, 20, 40, 64):
                for n in (1, 64, 65, 130, 200, 1024, 4096):
                    for cus in (1, 64, 256, 304):
                        got = plan(batch, n, nk, d, dv, L.SP_BF16, cus)
                        assert got == expect(batch, n, nk, d, dv, cus, pieces), (pieces, nk, d, dv, batch, n, cus, got)
                        assert got == plan(batch, n, nk, d, dv, L.SP_F16, cus) == plan(batch, n, nk, d, dv, L.SP_BF16, cus)
                        fw, bw, slabs = got
                        nqb = div_up(n, 64)
                        assert 1 <= fw <= nqb and 1 <= slabs <= nqb
                        if bw:
                            assert (slabs - 1) * bw < nqb <= slabs * bw, "an empty piece"


def test_shapes_off_the_mfma_route_have_no_walk(key):
    key(-1)
    assert plan(4, 100, 64, 32, 48, L.SP_BF16, 256) == (1, 0, 4)          # MFMA forward, VALU backward: 32 queries per slab
    assert plan(4, 100, 48, 32, 32, L.SP_BF16, 256) == (0, 0, 4)
    assert plan(4, 100, 96, 32, 64, L.SP_F32, 256) == (0, 0, 4)
    key(2)
    assert plan(4, 100, 96, 32, 64, L.SP_F32, 256) == (0, 0, 4)           # the key moves nothing there
    assert plan(1, 1024, 256, 64, 256, L.SP_BF16, 256) == (8, 0, 16)      # D = 64: the backward keeps a slab per query block
