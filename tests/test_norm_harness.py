"""The harness of tests/test_gpu_norm_exact.py checked against itself on the CPU (tests/norm_exact_util.py): every case of the GPU
module meets the conditions its regime rests on (building a case asserts them), the fp32 restatement of the kernels' arithmetic is
torch.equal in the exact comparisons and below 1.0 of every derived bound, and the comparison rejects the defects the tests exist to
catch, each planted into the restatement."""
import functools

import pytest
import torch

import norm_exact_util as N

BF16, F16, F32 = N.BF16, N.F16, N.F32
DT_IDS = [N.NAME[dt] for dt in N.DTYPES]
WORST = {}


@functools.lru_cache(maxsize=16)
def built(fn, *args):
    return getattr(N, fn)(*args)


def passes(c, got, key=None):
    w = N.compare(c, got)
    exact_only = all(k[0] == "exact" for k in c.checks.values())
    assert w <= 1.0 and (w == 0.0 or not exact_only)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), w)
    return w


@pytest.fixture
def ratios():
    """The figures of DESIGN.md section 2: a test's worst error / bound per comparison, printed when the test ends."""
    WORST.clear()
    yield WORST
    print("restatement, worst error / bound: " + ", ".join("%s %s %.3f" % (k[0], k[1], w) for k, w in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values()), dict(WORST)


def rejected(c, got, parts=None):
    with pytest.raises(AssertionError, match="elements differ"):
        N.compare(c, got, parts)


def splits_of(n):
    return [0] + ([1] if n >= 2 else []) + ([3] if n == 4 else [])


# ------------------------------------------------------------------------------------------------------------------------------------
# conditions and restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_sums_conditions_hold_and_the_restatement_passes(dt, ratios):
    for shape in N.SMALL + [N.WIDE[dt]] + N.CLAMP:
        c = built("sums_case", dt, shape)
        passes(c, N.restate_sums(c), ("sums", N.NAME[dt]))
        assert c.checks["mean"][0] == "exact" and c.checks["invstd"][0] == "within"
        assert (c.checks["running_mean"][0] == "exact") == c.dyadic
    for shape in (N.BASE, (3, 5, 7, 20)):
        c = built("sums_case", dt, shape, 0, 0, 0.001)
        passes(c, N.restate_sums(c), ("sums", N.NAME[dt]))
    c = built("sums_case", dt, N.BASE, 0, 0, None, False)
    passes(c, N.restate_sums(c))
    for shape in ((4, 4, 4, 96), N.PAIR_CLAMP):
        for split in (1, 3):
            for first in (0, 1):
                c = built("sums_case", dt, shape, split, first)
                assert c.checks["running_mean"][0] == "exact"
                passes(c, N.restate_sums(c), ("sums", N.NAME[dt]))
    for split in (1, 3):
        c = built("sums_case", dt, N.PAIR_CLAMP_516, split, split // 3)
        assert c.momentum < 0.01
        passes(c, N.restate_sums(c), ("sums", N.NAME[dt]))
    c = built("sums_case", dt, (2, 1, 1, 8), 0, 0, None, True, 4)
    passes(c, N.restate_sums(c))


def test_the_clamp_shapes_reach_the_clamps():
    for dt in N.DTYPES:
        asked = lambda pixels, c: pixels // (N.pix_par(dt, c) * 8)                                               # noqa: E731
        assert [N.stat_blocks(s[0] * s[1] * s[2], dt, s[3]) for s in N.CLAMP] == [N.MAX_PARTS, N.MAX_PARTS if dt == F32 else 512, N.MAX_PARTS]
        assert asked(96 * 86, 516) == 1032 and asked(512 * 512, 64) == (2048 if dt == F32 else 1024)
        n, h, w, c = N.PAIR_CLAMP_516
        assert asked(3 * h * w, c) == 513 and N.pair_blocks(h * w, 3 * h * w, dt, c) == N.MAX_PARTS // 2
        n, h, w, c = N.BWD_CLAMP_516
        assert n * asked(h * w, c) == 1026 and N.bwd_blocks(n, h * w, dt, c) == N.MAX_PARTS // n
        n, h, w, c = N.BWD_CLAMP
        assert n * N.up2_rows(n, h, w, dt, c) == (1017 if dt == F32 else 768)          # up2_grid: 3 x 384 asked for, 3 x 3 x 113 granted in fp32
        assert N.stat_blocks(2 * 16 * 16, dt, 64) == (4 if dt == F32 else 2)     # (2, 16, 16, 64): several partial rows
        assert N.WIDE[dt][3] // N.vec(dt, N.WIDE[dt][3]) == (258 if dt == F32 else 257)          # two / one live group in the second trip
        assert [N.pix_par(dt, c) for c in (96, 136)] == ([10, 7] if dt == F32 else [21, 15])
    assert N.vec(BF16, 12) == 4 and N.vec(F16, 20) == 4 and N.vec(BF16, 64) == 8
    assert N.ROW_CAP[0] * 2 * N.ROW_CAP[1] > 65535             # output rows: sp_upsample2_fwd, sp_bn_apply_upsample2
    assert N.ROW_CAP[0] * N.ROW_CAP[1] <= 65535 < N.ROW_CAP_BWD[0] * N.ROW_CAP_BWD[1]        # input rows: sp_upsample2_bwd needs its own shape
    assert 3 * 352 > N.MAX_PARTS and all(3 * N.up2_rows(3, 176, 2, dt, 8) == 1023 for dt in N.DTYPES)
    assert sorted((2 * s[2]) % 4 for s in N.TINY[3:]) == [0, 0, 2] and sorted(s[2] for s in N.TINY[3:]) == [2, 3, 4]


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_affine_conditions_hold_and_the_restatement_is_exact(dt):
    for shape in N.SMALL + [N.WIDE[dt]]:
        for source in N.SOURCES:
            for act in (N.ACT_NONE, N.ACT_LRELU, N.ACT_RELU):
                c = built("affine_case", dt, shape, source, act)
                assert passes(c, N.restate_apply(c)) == 0.0
        for split in splits_of(shape[0])[1:]:
            c = built("affine_case", dt, shape, "emb", N.ACT_LRELU, split)
            assert passes(c, N.restate_apply(c)) == 0.0


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_backward_conditions_hold_and_the_restatement_passes(dt, ratios):
    for shape in N.SMALL + [N.WIDE[dt], N.BWD_CLAMP]:
        count = shape[0] * shape[1] * shape[2]
        for source in N.SOURCES:
            for act in (N.ACT_NONE, N.ACT_LRELU):
                c = built("backward_case", dt, shape, source, act)
                assert c.dx_exact == (count & (count - 1) == 0), c.what
                assert all(v[0] == "exact" for k, v in c.checks.items() if k != "dx")
                assert c.differ >= 0.1 or source in ("gamma", "none")
                passes(c, N.restate_backward(c), ("backward", N.NAME[dt]))
    for source, act in (("emb", N.ACT_LRELU), ("gamma-beta", N.ACT_NONE)):
        c = built("backward_case", dt, N.BWD_CLAMP_516, source, act)
        passes(c, N.restate_backward(c), ("backward", N.NAME[dt]))
    for source in N.SOURCES:
        c = built("backward_case", dt, (2, 2, 2, 8), source, N.ACT_LRELU, True)
        assert c.dx_exact and passes(c, N.restate_backward(c)) == 0.0


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_interp_conditions_hold_and_the_restatement_passes(dt, ratios):
    for shape in N.UP + [N.ROW_CAP]:
        cases = [built("up_fwd_case", dt, shape), built("up_bwd_case", dt, shape)]
        if shape != N.ROW_CAP:
            for c in (built("up_fwd_case", dt, shape, True), built("up_bwd_case", dt, shape, True)):
                passes(c, N.restate_interp(c), (c.what[0] + " gauss", N.NAME[dt]))
        for split in splits_of(shape[0]):
            cases += [built("apply_up_case", dt, shape, s, a, split) for s, a in (("emb", 1), ("gamma-beta", 0), ("none", 2))]
        if shape != N.ROW_CAP:
            cases += [built("up_apply_case", dt, shape, s, a) for s, a in (("emb", 1), ("gamma-beta", 0), ("gamma", 2))]
        for c in cases:
            w = passes(c, N.restate_interp(c), (c.what[0], N.NAME[dt]))
            assert (shape[1] * shape[2] == 1) == all(v[0] == "exact" for v in c.checks.values()) and (w == 0.0 or shape[1] * shape[2] > 1)


DENSE_FORMS = (("emb", N.ACT_LRELU), ("gamma-beta", N.ACT_LRELU), ("gamma", N.ACT_NONE), ("none", N.ACT_LRELU))


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_dense_conditions_hold_and_the_restatement_passes(dt, ratios):
    """Building a case asserts that no |z| lies within tau of the kink and that the statistics' perturbation stays first-order; the
    chain restated in fp32 (partial rows in the kernels' order) stays below every bound; planted faults do not."""
    for shape in N.DENSE:
        for source, act in DENSE_FORMS:
            c = built("dense_case", dt, shape, source, act)
            if act == N.ACT_LRELU:
                assert bool((c.z.abs() >= c.tau).all())
            for k, v in c.checks.items():
                got = N.restate_dense(c)[k].double().reshape(v[1].shape)
                key = ("dense " + k, N.NAME[dt])
                WORST[key] = max(WORST.get(key, 0.0), float(((got - v[1]).abs()[v[2] > 0] / v[2][v[2] > 0]).max()))
            passes(c, N.restate_dense(c))
            rejected(c, N.restate_dense(c, drop_last=True), ("mean", "invstd"))
            rejected(c, N.restate_dense(c, round16=True))
            if act == N.ACT_LRELU and source != "none":
                rejected(c, N.restate_dense(c, act_from_xhat=True), ("dx",))
        for split in splits_of(shape[0])[1:]:
            c = built("dense_case", dt, shape, "emb", N.ACT_LRELU, split)
            passes(c, N.restate_dense(c))
            rejected(c, N.restate_dense(c, same_stats=True), ("y",))


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_dense_fused_conditions_hold_and_the_restatement_passes(dt, ratios):
    """The chain through the fused apply and the fold: the backward's checks are built from the dy the restatement's fold stored."""
    for shape in N.DENSE:
        for source, act in DENSE_FORMS[:3]:
            c = built("dense_case", dt, shape, source, act, 0, False, True)
            r = N.restate_dense(c)
            ref, bound, _ = N.up_bwd_reference(c.dy)
            N.assert_within(r.dlow, ref, N.stored(ref, bound, dt), c.what)
            full = N.Case(c)
            full.update(checks=dict(c.checks, **N.dense_backward_checks(c, r.dlow.double())))
            passes(full, r, ("dense-fused", N.NAME[dt]))
            rejected(full, N.restate_dense(c, round16=True), ("y",))
            if act == N.ACT_LRELU:
                rejected(full, N.restate_dense(c, act_from_xhat=True), ("dx",))
        for split in splits_of(shape[0])[1:]:
            c = built("dense_case", dt, shape, "emb", N.ACT_LRELU, split, False, True)
            passes(c, N.restate_dense(c), ("dense-fused", N.NAME[dt]))
            rejected(c, N.restate_dense(c, same_stats=True), ("y",))


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_up2_constant_maps_are_exact_in_16_bit_storage(dt):
    """An integer per (sample, channel) survives the fp32 blend and the 16-bit rounding of u: the expansion is the integer again."""
    for shape in N.UP2_EXACT:
        n, h, w, ch = shape
        c = built("sums_case", dt, (n, 1, 1, ch), 0, 0, None, True, 4 * h * w)
        u = N.restate_up2(c.x.expand(n, h, w, ch).float(), dt).to(dt)
        assert torch.equal(u.double(), c.x.expand(n, 2 * h, 2 * w, ch))
        passes(c, N.restate_sums(c))
        rejected(c, N.restate_sums(c, drop_last=True), ("mean",))
        for source, act in (("emb", N.ACT_LRELU), ("gamma-beta", N.ACT_LRELU), ("gamma", N.ACT_NONE)):
            b = built("backward_case", dt, (n, 2 * h, 2 * w, ch), source, act, True)
            assert all(v[0] == "exact" for k, v in b.checks.items() if k != "dx")
            passes(b, N.restate_backward(b))
            rejected(b, N.restate_backward(b, drop_last=True), ("demb",) if source == "emb" else ("dbeta", "dgamma"))


def test_dense_up2_conditions_hold_and_the_restatement_passes(ratios):
    for shape in N.UP2_DENSE:
        for source, act in (("emb", N.ACT_LRELU), ("gamma-beta", N.ACT_LRELU), ("gamma", N.ACT_NONE)):
            c = built("dense_case", F32, shape, source, act, 0, True)
            for k, v in c.checks.items():
                got = N.restate_dense(c)[k].double().reshape(v[1].shape)
                WORST[("dense-up2 " + k, "fp32")] = max(WORST.get(("dense-up2 " + k, "fp32"), 0.0), float(((got - v[1]).abs()[v[2] > 0] / v[2][v[2] > 0]).max()))
            passes(c, N.restate_dense(c))
            rejected(c, N.restate_dense(c, drop_last=True), ("mean", "invstd"))
            rejected(c, N.restate_dense(c, round16=True))
    n, h, w, ch = N.UP2_DENSE[-1]
    assert n * 2 * h > N.MAX_PARTS and n * N.up2_rows(n, h, w, F32, ch) == 1023
    with pytest.raises(AssertionError, match="no activation"):
        N.dense_case(F16, N.BASE, "gamma", N.ACT_LRELU, 0, True)
    for dt in (BF16, F16):                                     # wide bounds: what they do reject is asserted, nothing more is claimed
        for shape in N.UP2_DENSE_16:
            for source in ("emb", "gamma"):
                c = built("dense_case", dt, shape, source, N.ACT_NONE, 0, True)
                passes(c, N.restate_dense(c), ("dense-up2", N.NAME[dt]))
                bad = N.restate_dense(c)
                bad.update(dx=bad.dx.roll(1, 2))                # du one column off
                rejected(c, bad, ("dx",))


# ------------------------------------------------------------------------------------------------------------------------------------
# planted faults
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_planted_faults_in_the_statistics_are_rejected(dt):
    for shape in (N.BASE, (3, 5, 7, 20), (2, 16, 16, 64), (4, 4, 4, 96), N.WIDE[dt], N.CLAMP[1]):
        c = built("sums_case", dt, shape)
        rejected(c, N.restate_sums(c, drop_last=True), ("mean",))              # the last pixel of a block's walk dropped
        rejected(c, N.restate_sums(c, drop_last=True), ("invstd",))
        if N.stat_blocks(c.counts[0], dt, shape[3]) > 1:
            rejected(c, N.restate_sums(c, skip_row=True), ("mean",))           # the last partial row skipped
        if c.counts[0] >= 64:                                                  # (16 pixels of |x| <= 15 still fit fp16's 11 bits)
            rejected(c, N.restate_sums(c, round16=True), ("mean", "invstd"))   # partial sums through 16 bits
    for shape in ((4, 4, 4, 96), N.PAIR_CLAMP, N.PAIR_CLAMP_516):
        for split in (1, 3):
            for first in ((0, 1) if shape[3] != 516 else (split // 3,)):
                c = built("sums_case", dt, shape, split, first)
                rejected(c, N.restate_sums(c, same_stats=True), ("mean",))     # the second group given the first group's statistics
                rejected(c, N.restate_sums(c, same_stats=True), ("invstd",))
                if c.dyadic:
                    rejected(c, N.restate_sums(c, swap_first=True), ("running_mean",))      # first_group swapped
                rejected(c, N.restate_sums(c, drop_last=True), ("mean",))
                if N.pair_blocks(c.counts[0], c.counts[1], dt, shape[3]) > 1:
                    rejected(c, N.restate_sums(c, skip_row=True), ("mean",))
    c = built("sums_case", dt, N.BASE, 0, 0, None, False)
    good = N.restate_sums(c)
    rejected(c, N.Case(good, mean=good.mean + 2.0 ** -20), ("mean",))


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_planted_faults_in_the_apply_are_rejected(dt):
    for shape in ((4, 4, 4, 96), (2, 4, 8, 20)):
        for split in splits_of(shape[0])[1:]:
            c = built("affine_case", dt, shape, "emb", N.ACT_LRELU, split)
            rejected(c, N.restate_apply(c, same_stats=True))
            c = built("apply_up_case", dt, shape, "emb", N.ACT_LRELU, split)
            rejected(c, N.restate_interp(c, same_stats=True))
    for act in (N.ACT_NONE, N.ACT_LRELU):                      # (every z of this regime fits 8 bits: a 16-bit z shows in interp / backward)
        c = built("affine_case", dt, N.BASE, "gamma-beta", act)
        bad = N.restate_apply(c)
        bad.y[-1, -1, -1, -4:] = -1536.0                                       # the last vector never stored
        rejected(c, bad)


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_planted_faults_in_the_backward_are_rejected(dt):
    for shape in (N.BASE, (3, 5, 7, 20), (4, 4, 4, 96), (2, 16, 16, 64), N.BWD_CLAMP):
        for source in ("gamma-beta", "emb"):
            c = built("backward_case", dt, shape, source, N.ACT_LRELU)
            sums = ("dgamma", "dbeta") if source != "emb" else ("demb",)
            rejected(c, N.restate_backward(c, act_from_xhat=True), sums)       # act' taken from xhat > 0
            rejected(c, N.restate_backward(c, act_from_xhat=True), ("dx",))
            rejected(c, N.restate_backward(c, drop_last=True), sums)
            if shape[0] * shape[1] * shape[2] >= 512:                          # (smaller sums fit fp16's 11 bits)
                rejected(c, N.restate_backward(c, round16=True), sums + ("c_tmp",))
            if N.bwd_blocks(shape[0], shape[1] * shape[2], dt, shape[3]) > 1:
                rejected(c, N.restate_backward(c, skip_row=True), sums)
            if source == "emb":
                if shape[0] >= 3:
                    rejected(c, N.restate_backward(c, unmerged=True), ("demb",))            # classes not merged
                rejected(c, N.restate_backward(c, unwritten=True), ("demb",))  # unused rows left unwritten


@pytest.mark.parametrize("dt", N.DTYPES, ids=DT_IDS)
def test_planted_faults_in_the_interpolation_are_rejected(dt):
    for shape in ((1, 2, 2, 8), (1, 2, 3, 8), (1, 2, 4, 8), (1, 1, 5, 8), (3, 5, 7, 20), (2, 8, 8, 64)):
        for c in (built("up_fwd_case", dt, shape), built("apply_up_case", dt, shape, "gamma-beta", N.ACT_NONE, 0),
                  built("up_apply_case", dt, shape, "gamma-beta", N.ACT_NONE)):
            rejected(c, N.restate_interp(c, clamp_short=True))                 # the last source column clamped to W - 2
    for shape in ((3, 5, 7, 20), (2, 8, 8, 64)):
        if dt == F32 or shape[3] >= 8:
            c = built("up_fwd_case", dt, shape)
            rejected(c, N.restate_interp(c, round16=True) if dt == F32 else N.Case(y=N.restate_up2(c.x.float(), BF16 if dt == F16 else dt, round16=True).to(dt)))
    c = built("up_fwd_case", dt, N.ROW_CAP)                                    # the rows past the 65535-row grid never produced
    bad = N.restate_interp(c)
    bad.y[:, 65535:] = -1536.0
    rejected(c, bad)
    c = built("up_bwd_case", dt, N.ROW_CAP_BWD)                # the second trip of the backward's row loop dropped
    bad = N.restate_interp(c)
    passes(c, bad)
    bad.dx.view(-1, 8)[65535:] = -1536.0
    rejected(c, bad)
    c = built("up_bwd_case", dt, (2, 8, 8, 64))
    good = N.restate_interp(c)
    short = N.restate_up_bwd(torch.cat((c.dy[:, :-1], torch.zeros_like(c.dy[:, :1])), 1).float(), 8, 8).to(dt)     # the last output row unheard
    rejected(c, N.Case(good, dx=short))
