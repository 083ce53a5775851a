"""The harness of tests/test_gpu_eltwise_exact.py checked against itself on the CPU (tests/eltwise_exact_util.py): every case of the GPU
module, in all three storage types, meets the conditions its regime rests on (building a case asserts them); the fp32 restatement of
the kernels' arithmetic passes the comparison with zero differences (in the candidate regime in both evaluations, in the tanh regime
below 1.0 of the bound); and the comparison rejects the defects the tests exist to catch, each planted into the restatement."""
import numpy as np
import pytest
import torch

import eltwise_exact_util as E

BF16, F16, F32 = E.BF16, E.F16, E.F32
DT_IDS = [E.NAME[dt] for dt in E.DTYPES]
WORST = {}


@pytest.fixture
def ratios():
    """The figures of DESIGN.md section 21: a test's worst error / bound per bounded comparison, printed when the test ends."""
    WORST.clear()
    yield WORST
    print("restatement, worst error / bound: " + ", ".join("%s %.3f" % (k, w) for k, w in sorted(WORST.items())))
    assert all(w < 1.0 for w in WORST.values()), dict(WORST)


def rejected(c, got, canary=E.CANARIES[0], parts=None):
    with pytest.raises(AssertionError, match="elements differ"):
        E.compare(c, got, canary, parts)


# ------------------------------------------------------------------------------------------------------------------------------------
# conditions and restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_conditions_hold_and_the_restatement_passes(family, dt, ratios):
    rows = E.table(family, dt)
    assert rows
    for args in rows:
        c = E.build(family, args)
        for canary in E.CANARIES:
            w = E.compare(c, E.RESTATE[family](c, canary), canary)
            if any(k[0] == "tanh" for k in c.checks.values()):
                if dt == F32:
                    ratios["tanh " + E.NAME[dt]] = max(ratios.get("tanh " + E.NAME[dt], 0.0), w)
            else:
                assert w == 0.0
        if E.candidate_kinds(c):                                   # the fused evaluation is the other admitted value
            got = E.RESTATE[family](c, fused=True)
            assert E.compare(c, got) == 0.0
            name = E.candidate_kinds(c)[0]
            a, b = c.checks[name][1], c.checks[name][3]
            no_sum = family == "rescale" and c.bias is None         # nothing is added: one product, both evaluations are one float
            assert a.numel() < 1000 or dt != F32 or torch.equal(a, b) == no_sum, (c.what, "the two candidates never differ")


def test_the_shapes_reach_the_edges_they_are_there_for():
    assert E.grid_for(E.TWO_TRIPS // 4) == 2048 and E.TWO_TRIPS // 4 - 2048 * 256 == 37
    n = E.SCALE_BWD_SIZES[-1]
    assert E.scale_bwd_blocks(n) == 512 and n // 4 - 512 * 256 == 37 and E.scale_bwd_blocks(1028) == 2 and E.scale_bwd_blocks(4) == 1
    assert [E.act_bwd_vector(*s) for s in E.ACT_BWD_VEC] == [True] * 3 and not any(E.act_bwd_vector(*s) for s in E.ACT_BWD_PAD)
    assert 8200 * 256 // 4 > 2048 * 256 and 65600 * 8 > 2048 * 256 and 1030 * 8 > 256
    assert [E.rescale_scalar(*s[1:]) for s in E.RESCALE_VEC + E.RESCALE_SCALAR] == [False] * 4 + [True] * 4
    assert 2100 * 256 // 4 < 2048 * 256 < 2100 * 256                # more than one block, pitch ldy beyond c
    b, c, hw = E.PERMUTE[-1]
    assert 2048 * 256 < b * c * hw < 2 * 2048 * 256
    plans = [E.channel_sum_plan(p, c) for p, c, _ in E.CHANNEL_SUM]
    assert plans[3] == (34, 7, 2) and 256 - 34 * 7 == 18            # 34 lanes per pixel, 7 pixel lanes, 18 idle threads
    assert plans[4][0] == 256 and (1028 + 3) // 4 > 256             # a second cbase round
    assert plans[5] == (3, 85, 2) and plans[6] == (256, 1, 512) and 16389 // 32 == 512 and 16389 > 512 * 32
    assert [s[2] & 3 for s in E.CHANNEL_SUM][:3] == [0, 3, 0] and plans[0][2] == 1
    for dt in E.DTYPES:
        p, c, cp = E.mask_concat_shapes(dt)[-1]
        assert p * cp // 4 > 2048 * 256 and all(s[1] % 4 == 0 and s[2] % 4 == 0 and s[2] > s[1] for s in E.mask_concat_shapes(dt))
    n, h, w = E.INGEST_SHAPES[-1]
    assert n * h * w > 2048 * 256
    assert all(n * c > 256 for n, _, c in E.GLOBAL_AVG) and 35 * 35 * 192 // 4 > 256


def test_the_multiples_of_five_are_exact_under_the_slope():
    k = np.arange(-819, 820, dtype=np.float32)
    assert np.array_equal(E.F02 * (np.float32(5.0) * k), k) and float(np.abs(5 * k).max()) == 4095.0
    j = torch.arange(-16, 17).double().view(-1, 1)
    dy = torch.arange(-4095, 4096).double().view(1, -1)
    y = (j / 16).float()
    one = torch.ones_like(y)
    assert torch.equal(E.fused32(-y, y, one), 1.0 - y * y)          # 1 - y^2 = (256 - j^2) / 256 with or without an fma
    assert torch.equal((dy.float() * (1.0 - y * y)).double(), dy * (256 - j * j) / 256)        # and the one product that follows is exact


def test_the_fused_candidate_is_the_exact_value_rounded_once():
    g = E.X.gen(3)
    x, y, z = [1.0 + torch.rand(4096, generator=g) for _ in range(3)]           # one binade: the exact sum has 49 bits
    f = E.fused32(x, y, z)
    assert E.fused_is_exact(x, y, z, range(0, 4096, 16))            # the float64 sum IS the rational x y + z there
    assert not torch.equal(f, E.separate32(x, y, z))                # and the two evaluations differ somewhere
    with pytest.raises(AssertionError, match="not exact in float64"):
        E.fused32(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([2.0 ** 40]))
    for fam, args in (("scale_add", (F32, 1028, 0.3)), ("rescale", (BF16, 3, 365, 368, 368, True, "real")),
                      ("ingest", (F32, F16, 2, 16, 16, 3, 8, "crop", "vgg"))):
        c = E.build(fam, args)
        name = E.candidate_kinds(c)[0]
        third = c.checks[name][1].clone()
        both = c.checks[name][1] == c.checks[name][3]
        keep = c.checks[name][2]
        at = int(((both & ~keep) if keep is not None else both).long().argmax())
        third[at] = third[at] + (8.0 if c.dtype == BF16 else 1.0)     # neither candidate
        got = E.RESTATE[fam](c)
        got[name][at] = third[at]
        rejected(c, got)


def test_rn_direct_rounds_once():
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -133 * 1.5, 65520.0], dtype=torch.float64)
    assert E.rn_direct(v[:4], BF16).double().tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, 2.0 ** -132]
    h = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -11, 2.0 ** -24 * 2.5, 2.0 ** -25], dtype=torch.float64)
    assert E.rn_direct(h, F16).double().tolist() == [1.0 + 2.0 ** -10, 1.0, 2.0 ** -23, 0.0]
    assert E.ulp32(torch.tensor([1.0, 0.75, 1e-45], dtype=torch.float64)).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -149]


# ------------------------------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_truncation_into_storage_is_rejected(dt):
    for fam, args in (("act_fwd", (dt, 1028, E.ACT_LRELU)), ("scale_add", (dt, 1028, 0.3)), ("scale_add_bwd", (dt, 1028, 0.3)),
                      ("rescale", (dt, 3, 64, 72, 64, True, "exact")), ("mask_concat", (dt, 128, 64, 72, E.MASK_QUARTERS)),
                      ("mask_mul", (dt, 3, 365, 368, 368, E.MASK_QUARTERS)), ("ingest", (F32, dt, 2, 16, 16, 3, 8, "nchw", "exact")),
                      ("ingest_bwd", (dt, 512, 3, 8, True)), ("avg3", (dt, 2, 8, 5, 12)), ("act_bwd", (dt, 257, 8, 8, E.ACT_TANH))):
        c = E.build(fam, args)
        rejected(c, E.RESTATE[fam](c, trunc=True))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_a_skipped_last_group_of_four_is_rejected(dt):
    for n in E.ACT_SIZES[:3]:
        c = E.build("act_fwd", (dt, n, E.ACT_LRELU))
        rejected(c, E.restate_act_fwd(c, skip_tail=True))
        c = E.build("scale_add", (dt, n, -3.0))
        rejected(c, E.restate_scale_add(c, skip_tail=True))
    for n in E.SCALE_BWD_SIZES[:2]:
        c = E.build("scale_add_bwd", (dt, n, 0.3))
        got = E.restate_scale_add_bwd(c, skip_tail=True)
        rejected(c, got, parts=("da",))
        rejected(c, got, parts=("dg",))
        rejected(c, got, parts=("partials",))
    for s in E.RESCALE_VEC + E.RESCALE_SCALAR:
        c = E.build("rescale", (dt,) + s + (True, "exact"))
        rejected(c, E.restate_rescale(c, skip_tail=True))
    for s in E.CHANNEL_SUM:
        c = E.build("channel_sum", (dt,) + s)
        got = E.restate_channel_sum(c, skip_tail=True)
        rejected(c, got, parts=("out",))
        rejected(c, got, parts=("partials",))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_a_skipped_second_trip_is_rejected(dt):
    for act in E.ACTS:
        c = E.build("act_fwd", (dt, E.TWO_TRIPS, act))
        rejected(c, E.restate_act_fwd(c, one_trip=True))
    for s in (E.ACT_BWD_VEC[-1], E.ACT_BWD_PAD[-1]):
        c = E.build("act_bwd", (dt,) + s + (E.ACT_LRELU,))
        rejected(c, E.restate_act_bwd(c, one_trip=True))
    c = E.build("scale_add", (dt, E.TWO_TRIPS, -3.0))
    rejected(c, E.restate_scale_add(c, one_trip=True))
    c = E.build("scale_add_bwd", (dt, E.SCALE_BWD_SIZES[-1], 0.3))
    got = E.restate_scale_add_bwd(c, one_trip=True)
    rejected(c, got, parts=("da",))
    rejected(c, got, parts=("dg",))
    for d in (0, 1):
        c = E.build("permute", (dt,) + E.PERMUTE[-1] + (d,))
        rejected(c, E.restate_permute(c, one_trip=True))
    c = E.build("mask_concat", (dt,) + E.mask_concat_shapes(dt)[-1] + (E.MASK_HALVES,))
    rejected(c, E.restate_mask_concat(c, one_trip=True))
    for a in E.table("ingest", dt):
        if a[2:5] == E.INGEST_SHAPES[-1]:
            c = E.build("ingest", a)
            rejected(c, E.restate_ingest(c, one_trip=True))
    c = E.build("ingest_bwd", (dt, 3 * 512 * 512, 3, E.ingest_cp(3, dt), True))
    rejected(c, E.restate_ingest_bwd(c, one_trip=True))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_padding_left_unwritten_or_filled_with_the_neighbour_is_rejected(dt):
    for pad in ("unwritten", "neighbour"):
        for s in E.ACT_BWD_PAD:
            if s[2] > s[1]:
                c = E.build("act_bwd", (dt,) + s + (E.ACT_LRELU,))
                rejected(c, E.restate_act_bwd(c, pad=pad))
        for s in E.mask_concat_shapes(dt):
            if s[2] > s[1] + 1:
                c = E.build("mask_concat", (dt,) + s + (E.MASK_HALVES,))
                rejected(c, E.restate_mask_concat(c, pad=pad))
        for s in E.MASK_MUL:
            if s[3] > s[1]:
                c = E.build("mask_mul", (dt,) + s + (E.MASK_HALVES,))
                rejected(c, E.restate_mask_mul(c, pad=pad))
        c = E.build("ingest", (F32, dt, 2, 3, 5, 2, E.ingest_cp(2, dt), "nchw", "exact"))
        rejected(c, E.restate_ingest(c, pad=pad))
    for s in E.RESCALE_VEC + E.RESCALE_SCALAR:                     # the other contract: y's columns [c, ldy) are NOT written
        if s[3] > s[1]:
            c = E.build("rescale", (dt,) + s + (True, "exact"))
            rejected(c, E.restate_rescale(c, pad=0.0))
    c = E.build("channel_sum", (dt, 300, 6, 8))                     # a lane that adds a padding column of the input: NaN
    rejected(c, E.restate_channel_sum(c, sum_padding=True), parts=("out",))
    c = E.build("ingest_bwd", (dt, 15, 2, E.ingest_cp(2, dt), True))    # dy read at pitch c instead of cp
    rejected(c, E.restate_ingest_bwd(c, pitch=2))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_the_mask_channel_one_too_far_is_rejected(dt):
    for s in E.mask_concat_shapes(dt):
        for m in E.MASKS:
            c = E.build("mask_concat", (dt,) + s + (m,))
            rejected(c, E.restate_mask_concat(c, mask_at=1))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_leaky_relu_slope_defects_are_rejected(dt):
    for s in E.ACT_BWD_VEC + E.ACT_BWD_PAD:
        c = E.build("act_bwd", (dt,) + s + (E.ACT_LRELU,))
        rejected(c, E.restate_act_bwd(c, slope0=True))              # slope 0 at y == 0
        rejected(c, E.restate_act_bwd(c, by_dy=True))               # the slope applied by the sign of dy, not selected by y
        c = E.build("act_bwd", (dt,) + s + (E.ACT_RELU,))
        rejected(c, E.restate_act_bwd(c, by_dy=True))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_channel_sum_defects_are_rejected(dt):
    for s in E.CHANNEL_SUM:
        c = E.build("channel_sum", (dt,) + s)
        if c.blocks > 1:
            for b in (0, c.blocks - 1):
                rejected(c, E.restate_channel_sum(c, drop_block=b), parts=("out",))
    c = E.build("channel_sum", (dt, 33, 1028, 1028))
    got = E.restate_channel_sum(c, one_round=True)
    rejected(c, got, parts=("out",))
    rejected(c, got, parts=("partials",))
    got = E.restate_channel_sum(c)
    got["partials"][c.blocks * c.c] = 0.0                           # a row beyond the launched blocks written
    rejected(c, got, parts=("partials",))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_the_wrong_sigma_slot_is_rejected(dt):
    for s in E.RESCALE_VEC + E.RESCALE_SCALAR:
        for regime in ("exact", "real"):
            c = E.build("rescale", (dt,) + s + (True, regime))
            rejected(c, E.restate_rescale(c, slot="a1b1"))
            rejected(c, E.restate_rescale(c, slot="a0b0"))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_the_next_channels_scale_is_rejected(dt):
    for layout in E.INGEST_LAYOUTS:
        for ch in (1, 2, 3):
            c = E.build("ingest", (F32, dt, 2, 3, 5, ch, E.ingest_cp(ch, dt), layout, "exact"))
            rejected(c, E.restate_ingest(c, shift_channel=1))
    c = E.build("ingest_bwd", (dt, 30, 3, E.ingest_cp(3, dt), True))
    rejected(c, E.restate_ingest_bwd(c, shift_channel=1))


@pytest.mark.parametrize("dt", E.DTYPES, ids=DT_IDS)
def test_a_swapped_permute_direction_is_rejected(dt):
    for s in E.PERMUTE[1:]:
        for d in (0, 1):
            c = E.build("permute", (dt,) + s + (d,))
            rejected(c, E.restate_permute(c, swapped=True))


def test_fp16_operands_decoded_as_bf16_are_rejected():
    for fam, args in (("act_fwd", (F16, 1028, E.ACT_LRELU)), ("act_bwd", (F16, 257, 8, 8, E.ACT_LRELU)), ("scale_add", (F16, 1028, -3.0)),
                      ("scale_add_bwd", (F16, 1028, 0.3)), ("rescale", (F16, 3, 64, 72, 64, True, "exact")), ("channel_sum", (F16, 300, 6, 8)),
                      ("mask_concat", (F16, 128, 64, 72, E.MASK_01)), ("mask_mul", (F16, 3, 365, 368, 368, E.MASK_01)),
                      ("ingest", (F16, F16, 2, 16, 16, 3, 8, "nhwc", "exact")), ("ingest_bwd", (F16, 512, 3, 8, True)),
                      ("avg3", (F16, 2, 8, 5, 12)), ("global_avg", (F16, 50, 64, 6))):
        c = E.build(fam, args)
        rejected(c, E.RESTATE[fam](c, as_bf16=True))


def test_one_rounding_of_the_exact_product_into_fp16_is_rejected():
    """What the fp16 compilation computed before its single-element stores were given an fp32 register (v_fma_mixlo_f16): the product
    rounded once into fp16 differs from RN(fl32(product)) where fl32 lands on a tie of the 16-bit format."""
    c = E.build("ingest_bwd", (F16, 512, 3, 3, True))
    rejected(c, E.restate_ingest_bwd(c, once=True))
    c = E.build("ingest_bwd", (F32, 512, 3, 3, True))
    assert E.compare(c, E.restate_ingest_bwd(c, once=True)) == 0.0  # fp32 storage: the same rounding


def test_the_copy_is_pinned_to_the_bit():
    for dt in (BF16, F16):                                         # 16 bit: a signalling NaN comes out quiet, so a raw copy is another result
        c = E.build("act_fwd", (dt, 1028, E.ACT_NONE))
        rejected(c, E.restate_act_fwd(c, raw_copy=True))
        got = E.restate_act_fwd(c)
        got["y"][1] = 0.0                                          # -0 became +0
        rejected(c, got)
    c = E.build("act_fwd", (F32, 1028, E.ACT_NONE))
    assert E.compare(c, E.restate_act_fwd(c, raw_copy=True)) == 0.0 and bool(c.x.isnan().any())


def test_the_pool_divisors_are_pinned():
    for dt in E.DTYPES:
        c = E.build("avg3", (dt, 2, 3, 3, 8))
        rejected(c, E.restate_avg3(c, count_valid=True))           # count_include_pad: corners and edges divide by 9 too
    c = E.build("global_avg", (F32, 70, 289, 4))
    rejected(c, E.restate_global_avg(c, reciprocal=True))           # s * fl32(1 / hw) is another float than fl32(s / hw)


def test_the_comparison_rejects_a_nan_a_tanh_past_its_bound_and_a_touched_canary():
    c = E.build("act_fwd", (F32, 1028, E.ACT_TANH))
    got = E.restate_act_fwd(c)
    ref, e = c.checks["y"][1], c.checks["y"][5]
    at = int((e > 0).long().argmax())
    bad = got["y"].clone()
    bad[at] = float(ref[at] + 1.5 * e[at])
    rejected(c, E.Case(y=bad))
    bad = got["y"].clone()
    bad[at] = float("nan")
    rejected(c, E.Case(y=bad))
    for dt in (BF16, F16):                                         # 16 bit: one storage step beyond [RN(ref - e), RN(ref + e)]
        c = E.build("act_fwd", (dt, 1028, E.ACT_TANH))
        hi = c.checks["y"][4]
        at = int(((hi.double() > 0.25) & (hi.double() < 0.5)).long().argmax())
        bad = hi.clone()
        bad[at] = float(hi[at]) + (2.0 ** -9 if dt == BF16 else 2.0 ** -12)
        assert float(bad[at]) > float(hi[at])
        rejected(c, E.Case(y=bad))
        assert E.compare(c, E.Case(y=hi)) == 0.0 and E.compare(c, E.Case(y=c.checks["y"][3])) == 0.0
    for act in E.ACTS:                                             # the table: a NaN where none belongs, and a number where NaN belongs
        c = E.build("act_special", (F32, act))
        got = E.restate_act_fwd(c)
        bad = got["y"].clone()
        bad[4] = float("nan")
        rejected(c, E.Case(y=bad))
        if act != E.ACT_RELU:
            bad = got["y"].clone()
            bad[2] = 0.0
            rejected(c, E.Case(y=bad))
    c = E.build("rescale", (F32, 1, 4, 4, 8, True, "exact"))
    got = E.restate_rescale(c, E.CANARIES[1])
    assert E.compare(c, got, E.CANARIES[1]) == 0.0
    rejected(c, got, E.CANARIES[0])                                 # the other canary in the columns [c, ldy)
