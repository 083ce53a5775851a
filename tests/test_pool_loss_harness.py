"""The harness of tests/test_gpu_pool_exact.py and tests/test_gpu_loss_exact.py checked against itself on the CPU
(tests/pool_loss_exact_util.py): every case of the GPU modules meets the conditions its regime rests on (building a case asserts them),
the fp32 restatement of the kernels' arithmetic is torch.equal in the exact comparisons and below 1.0 of every derived bound, and the
comparison rejects the defects the tests exist to catch, each planted into the restatement."""
import pytest
import torch

import pool_loss_exact_util as P

BF16, F16, F32 = P.BF16, P.F16, P.F32
DT_IDS = [P.NAME[dt] for dt in P.DTYPES]
WORST = {}
REC_MULTI = P.REC_MULTI


def passes(c, got, key=None, exact=False):
    w = P.compare(c, got)
    exact_only = all(k[0] != "within" for k in c.checks.values())
    assert w <= 1.0 and (w == 0.0 or not exact_only) and (w == 0.0 or not exact)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), w)
    return w


@pytest.fixture
def ratios():
    """The figures of DESIGN.md section 14: a test's worst error / bound per comparison, printed when the test ends."""
    WORST.clear()
    yield WORST
    print("restatement, worst error / bound: " + ", ".join("%s %.3f" % (" ".join(map(str, k)), w) for k, w in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values()), dict(WORST)


def rejected(c, got, parts=None):
    with pytest.raises(AssertionError, match="elements differ"):
        P.compare(c, got, parts)


# ------------------------------------------------------------------------------------------------------------------------------------
# conditions and restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_pool_conditions_hold_and_the_restatement_is_exact(dt):
    for shape in P.POOL:
        for act in (P.ACT_LRELU, P.ACT_RELU):
            c = P.avg_case(dt, shape, act)
            assert passes(c, P.restate_avg(c)) == 0.0
        for act in (P.ACT_NONE, P.ACT_LRELU, P.ACT_RELU):
            for form in P.FORMS:
                c = P.act_avg_case(dt, shape, act, form)
                assert passes(c, P.restate_act_avg(c)) == 0.0
        for relu in (0, 1):
            c = P.max_case(dt, shape, relu)
            assert passes(c, P.restate_max(c)) == 0.0
    for shape in P.IDX:
        for table in ("routing", "slots"):
            c = P.max_idx_case(dt, shape, table)
            assert passes(c, P.restate_max_idx(c)) == 0.0


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_pool_clamp_cases_build_and_pass(dt):
    shape = P.POOL_CLAMP[dt]
    c = P.avg_case(dt, shape)
    assert passes(c, P.restate_avg(c)) == 0.0
    c = P.act_avg_case(dt, shape, P.ACT_LRELU)
    assert passes(c, P.restate_act_avg(c)) == 0.0
    c = P.max_case(dt, shape, 1)
    assert passes(c, P.restate_max(c)) == 0.0
    c = P.max_idx_case(dt, P.IDX_CLAMP[dt], "slots")
    assert passes(c, P.restate_max_idx(c)) == 0.0


def test_the_clamp_shapes_reach_the_clamps():
    for dt in P.DTYPES:
        n, h, w, c = P.POOL_CLAMP[dt]
        items = n * (h // 2) * (w // 2) * c // P.vec(dt, c)
        assert 2048 * 256 < items < 2 * 2048 * 256 and P.pool_grid(items) == 2048            # a second, partial trip of the grid-stride loop
        assert P.pool_grid(4 * items) == 2048 and (4 * items) % (2048 * 256) != 0              # sp_avgpool2_bwd walks the input: five trips
        n, h, w, c = P.IDX_CLAMP[dt]
        assert c % 16 == 0 and n * (h // 2) * (w // 2) * c // (4 if dt == F32 else 8) > 2048 * 256
    assert [P.vec(BF16, s[3]) for s in P.POOL] == [4, 8, 8, 4, 4, 8, 8] and all(P.vec(F32, s[3]) == 4 for s in P.POOL)
    a = P.ADAPTIVE_EXACT[-1]
    assert a[0] * a[4] * a[5] * (a[3] // 4) > 2048 * 256 and a[0] * a[1] * a[2] * (a[3] // 4) > 2048 * 256
    n, h, w, c = P.REC_4D[-1]
    items = n * (h // 2) * (w // 2) * (c // 4)
    assert items > 1024 * 256 and P.red_grid(items) == 256 and P.ew_grid(items) == 1024
    assert P.red_grid(P.DIV[-2][0]) == 256 and P.ew_grid(P.DIV[-1][0]) == 1024 and P.DIV[-1][0] > 1024 * 256 and P.DIV[1][0] % 256
    bf = [(b * f % 1024 == 0, f % 64 == 0, f % 256 == 0, b % 4 == 0) for b, f in P.DHEAD]
    assert all({True, False} == set(col) for col in zip(*bf))
    assert {b for b, _ in P.DHEAD} == {1, 2, 3, 5, 8, 20} and {f for _, f in P.DHEAD} == {8, 72, 128, 200, 256, 264}
    assert [n for n in P.SQERR if n > P.SQERR_SMALL_MAX] == [(1 << 18) + 1, (1 << 18) + 5, 1 << 20] and P.red_grid(1 << 20) == 256


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_adaptive_conditions_hold_and_the_restatement_passes(dt, ratios):
    for a in P.ADAPTIVE_EXACT:
        c = P.adaptive_case(dt, *a)
        assert c.exact and passes(c, P.restate_adaptive(c)) == 0.0
    for a in P.ADAPTIVE_BOUND:
        c = P.adaptive_case(dt, *a)
        assert not c.exact and c.checks["y"][0] == "within" and c.checks["dx"][0] == "within"
        passes(c, P.restate_adaptive(c), ("adaptive", P.NAME[dt]))


def test_sqerr_conditions_hold_and_the_restatement_passes(ratios):
    for n in P.SQERR:
        for target in (0.0, 1.0):
            c = P.sqerr_case(n, target)
            assert (c.checks["loss"][0] == "exact") == (n & (n - 1) == 0)
            passes(c, P.restate_sqerr(c), ("sqerr", "fp32"), exact=c.checks["loss"][0] == "exact")


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_dhead_and_div_conditions_hold_and_the_restatement_is_exact(dt):
    for b, f in P.DHEAD:
        for kind in P.CLASS_KINDS:
            c = P.dhead_case(dt, b, f, kind)
            assert passes(c, P.restate_dhead(c)) == 0.0
    for half_elems, half_z in P.DIV:
        for weight in (1.0, 0.25):
            c = P.div_case(dt, half_elems, half_z, weight)
            assert passes(c, P.restate_div(c)) == 0.0


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_rec_conditions_hold_and_the_restatement_passes(dt, ratios):
    for shape in P.REC_4D + P.REC_2D:
        for weight in (1.0, 0.25):
            c = P.rec_case(dt, [shape], weight)
            passes(c, P.restate_rec(c), ("rec", P.NAME[dt]), exact=c.pow2)
    for shapes, weight, masks in REC_MULTI:
        c = P.rec_case(dt, shapes, weight, masks)
        passes(c, P.restate_rec(c), ("rec", P.NAME[dt]), exact=c.pow2)
    assert P.rec_case(dt, REC_MULTI[0][0]).pow2 and P.rec_case(dt, REC_MULTI[2][0]).pow2 and len(REC_MULTI[2][0]) == P.REC_MAX_LEVELS


# ------------------------------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_truncation_to_16_bit_is_rejected(dt):
    for shape in P.POOL:                                           # the planted ties: every shape, the one-window map included
        c = P.avg_case(dt, shape)
        rejected(c, P.restate_avg(c, trunc=True), ("y",))
        rejected(c, P.restate_avg(c, trunc=True), ("y_act",))
    c = P.adaptive_case(dt, *P.ADAPTIVE_BOUND[0])
    rejected(c, P.restate_adaptive(c, trunc=True), ("y",))
    c = P.dhead_case(dt, 20, 264, "mix")
    rejected(c, P.restate_dhead(c, trunc=True), ("dx",))
    c = P.div_case(dt, 1000, 128)
    assert c.rounds_up
    rejected(c, P.restate_div(c, trunc=True), ("dimg",))


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_leaky_relu_after_the_storage_rounding_is_rejected(dt):
    for shape in P.POOL:
        c = P.avg_case(dt, shape, P.ACT_LRELU)
        rejected(c, P.restate_avg(c, act_after=True), ("y_act",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_slope_zero_at_zero_is_rejected(dt):
    for shape in P.POOL:
        for form in ("both", "ga"):
            c = P.act_avg_case(dt, shape, P.ACT_LRELU, form)
            rejected(c, P.restate_act_avg(c, slope0=True), ("dx",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_the_last_maximum_on_a_tie_is_rejected(dt):
    for shape in P.POOL:
        c = P.max_case(dt, shape, 0)
        rejected(c, P.restate_max(c, last=True), ("dx",))
    c = P.rec_case(dt, [(2, 4, 6, 8), (2, 365)])
    got = P.restate_rec(c, last_max=True)
    rejected(c, got, ("dfake0",))
    rejected(c, got, ("dfake1",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_a_shifted_index_word_is_rejected(dt):
    for shape in P.IDX:
        for table in ("routing", "slots"):
            c = P.max_idx_case(dt, shape, table)
            rejected(c, P.restate_max_idx(c, word_off=1), ("dx",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_an_adaptive_window_end_off_by_one_is_rejected(dt):
    for a in P.ADAPTIVE_BOUND + P.ADAPTIVE_EXACT[:2]:
        c = P.adaptive_case(dt, *a)
        got = P.restate_adaptive(c, floor_end=True)
        rejected(c, got, ("y",))
        rejected(c, got, ("dx",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_rec_defects_are_rejected(dt):
    c = P.rec_case(dt, [(3, 7), (2, 365)])
    got = P.restate_rec(c, tail_unwritten=True)                    # the sentinel survives in the odd tail
    rejected(c, got, ("dfake0",))
    rejected(c, got, ("dfake1",))
    for shapes in ([(2, 4, 6, 8)], [(2, 365)], [(1, 8, 8, 16), (2, 4096)]):
        c = P.rec_case(dt, shapes, 1.0, P.MASKS_HALVES)
        got = P.restate_rec(c, mask_first=True)                    # the mask at the window's first pixel
        rejected(c, got, ("loss",))
        rejected(c, got, ("dfake0",))
    for shapes in ([(2, 4, 6, 8)], [(1, 8, 8, 16), (2, 4096)]):
        c = P.rec_case(dt, shapes)
        got = P.restate_rec(c, count_c4=True)                      # count with C / 4
        rejected(c, got, ("loss",))
        rejected(c, got, ("dfake0",))


def test_a_dropped_tail_element_of_sqerr_is_rejected():
    for n in (3, 7, 51203, (1 << 18) + 1, (1 << 18) + 5):
        c = P.sqerr_case(n, 1.0)
        rejected(c, P.restate_sqerr(c, drop_tail=True), ("loss",))


@pytest.mark.parametrize("dt", P.DTYPES, ids=DT_IDS)
def test_dhead_defects_are_rejected(dt):
    for b, f in P.DHEAD:
        if b >= 3:
            for kind in ("equal", "mix", "last"):
                c = P.dhead_case(dt, b, f, kind)
                rejected(c, P.restate_dhead(c, last_writer=True), ("demb",))
        if b % 4:
            c = P.dhead_case(dt, b, f, "mix")
            rejected(c, P.restate_dhead(c, miss_last_row=True), ("dwc",))
    c = P.dhead_case(dt, 5, 72, "distinct")
    got = P.restate_dhead(c)
    got["demb"][299] = 1.0                                         # an absent class row that is not zero
    rejected(c, got, ("demb",))


def test_the_comparison_rejects_a_nan_and_an_error_past_the_bound():
    c = P.adaptive_case(F32, *P.ADAPTIVE_BOUND[0])
    got = P.restate_adaptive(c)
    ref, bound = c.checks["y"][1], c.checks["y"][2]
    worst = int((bound > 0).long().flatten().argmax())
    bad = got["y"].clone()
    bad.view(-1)[worst] = float(ref.view(-1)[worst] + 1.5 * bound.view(-1)[worst])
    with pytest.raises(AssertionError, match="differ by more than their bound"):
        P.compare(c, P.Case(y=bad))
    bad = got["y"].clone()
    bad.view(-1)[0] = float("nan")
    with pytest.raises(AssertionError):
        P.compare(c, P.Case(y=bad))
    assert torch.equal(P.truncated(torch.tensor([257.0]), BF16).float(), torch.tensor([256.0]))
    assert bool(P.ties(torch.tensor([128.5, 129.0, 1024.5]).double(), BF16).tolist() == [True, False, False])
    assert bool(P.ties(torch.tensor([1024.5, 128.5]).double(), F16).tolist() == [True, False])
