"""The harness of tests/test_gpu_exact.py checked against itself on the CPU: the comparison accepts the unaltered reference of each
regime and rejects the three alterations the exact tests exist to catch - a product that is missing, an intermediate that passed through
16 bits, a destination that was overwritten instead of accumulated into - and a multiply on a shortened operand in fp32 mode.  The rounded
intermediate is shown to stay within the 8e-3 of max|ref| the Gaussian tests grant."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as X

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def test_operand_helpers_keep_their_promises():
    g = X.gen(1)
    w = X.sparse_ternary_rows(37, 2304, g)
    assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0} and int((w != 0).sum(1).max()) == X.UNIT_NNZ
    w = X.sparse_ternary_rows(5, 9, g)
    assert int((w != 0).sum(1).max()) == 6
    x = X.integers((4, 1000), 255, g)
    assert float(x.abs().max()) == 255 and torch.equal(x, x.round()) and torch.equal(x, x.to(BF16).double())
    # the largest operand of the wide regime: the significand, then the 2^24 bound, then (fp16) the largest finite value
    assert X.wide_amax(BF16, 1152) == 255 and X.wide_amax(F16, 1152) == 2047 and X.wide_amax(F32, 72) == 4095
    assert X.wide_amax(F32, 9 * 520) == (X.LIMIT - 1) // (9 * 520) and X.wide_amax(BF16, 98304, 16, 1, 4) == 42
    assert X.f16_amax(2047, 1152, F16) == 682 and X.f16_amax(2047, 1152, BF16) == 2047


def test_reference_conditions_are_enforced():
    ok = torch.tensor([3.0, -200.0, 0.0], dtype=torch.float64)
    X.check_reference(ok, 240, BF16, "unit")
    X.check_reference(ok / 4, 240, BF16, "unit", denom=4)
    with pytest.raises(AssertionError, match="not integral"):
        X.check_reference(ok / 4, 240, BF16, "unit")
    with pytest.raises(AssertionError, match="2\\^24"):
        X.check_reference(ok, X.LIMIT, BF16, "wide")
    with pytest.raises(AssertionError, match="2\\^24"):
        X.check_reference(ok, X.LIMIT // 4, BF16, "wide", denom=4)
    with pytest.raises(AssertionError, match="not representable"):
        X.check_reference(torch.tensor([257.0], dtype=torch.float64), 300, BF16, "unit")
    X.check_reference(torch.tensor([257.0], dtype=torch.float64), 300, F16, "unit")
    with pytest.raises(AssertionError):
        X.check_reference(torch.tensor([70000.0], dtype=torch.float64), 70000, F16, "wide")


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
def test_a_missing_product_is_rejected_in_the_unit_regime(dtype):
    """Every output of the unit regime is held exactly, so ONE product taken out of ONE output changes what is stored, at every place tried."""
    c = X.conv_case(dtype, 2, 5, 7, 40, 24, 3, "unit", bias=True, res=1)
    want = c.want
    X.assert_exact(X.expected(c.ref, dtype).permute(0, 2, 3, 1).contiguous(), want, "unaltered")
    w4 = c.wt.view(24, 3, 3, 40)
    tried = 0
    for co, r, s, ci in (w4 != 0).nonzero()[::97].tolist():
        for n_, y, x_ in ((0, 0, 0), (1, 4, 6), (0, 2, 3)):
            yy, xx = y + r - 1, x_ + s - 1
            if not (0 <= yy < 5 and 0 <= xx < 7) or c.x[n_, ci, yy, xx] == 0:
                continue
            alt = c.ref.clone()
            alt[n_, co, y, x_] -= w4[co, r, s, ci] * c.x[n_, ci, yy, xx]
            got = X.expected(alt, dtype).permute(0, 2, 3, 1).contiguous()
            with pytest.raises(AssertionError, match="1 of .* elements differ"):
                X.assert_exact(got, want, "one product removed")
            tried += 1
    assert tried >= 20, tried


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_an_intermediate_rounded_to_16_bits_is_rejected_in_the_wide_regime(dtype):
    """The sum over the first half of K handed over in the storage type (a partial tile of a K-split, a split-K slab) and the second half
    added to it: rejected, and within the Gaussian tests' tolerance."""
    n, h, w, cin, cout = 2, 8, 32, 264, 80
    c = X.conv_case(dtype, n, h, w, cin, cout, 3, "wide")
    X.assert_exact(X.expected(c.ref, dtype).permute(0, 2, 3, 1).contiguous(), c.want, "unaltered")
    w4 = c.wt.view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    half = cin // 2
    first = F.conv2d(c.x[:, :half], w4[:, :half].contiguous(), padding=1)
    second = F.conv2d(c.x[:, half:], w4[:, half:].contiguous(), padding=1)
    assert torch.equal(first + second, c.ref)                                     # integer arithmetic: the split itself changes nothing
    assert float(first.abs().max()) >= 2 ** 14                                    # partial sums of 15 bits and more
    alt = first.to(dtype).double() + second
    got = X.expected(alt, dtype).permute(0, 2, 3, 1).contiguous()
    with pytest.raises(AssertionError, match="elements differ"):
        X.assert_exact(got, c.want, "half of K handed over in 16 bits")
    assert float((got.double() - c.want.double()).abs().max()) <= 8e-3 * float(c.want.double().abs().max())


def test_a_short_multiply_is_rejected_in_fp32_mode():
    """12-bit operands: a multiply that keeps 11 significant bits of an operand (a 10-bit mantissa: a reduced-precision MFMA path)
    changes the result - by a few 1e-4 of max|ref|, the order of the 2e-4 the fp32 parity tests grant on Gaussian operands."""
    c = X.conv_case(F32, 1, 8, 32, 8, 64, 3, "wide")
    X.assert_exact(X.expected(c.ref, F32).permute(0, 2, 3, 1).contiguous(), c.want, "unaltered")
    assert 4000 <= float(c.x.abs().max()) <= 4095
    x10 = (c.x / 2).round() * 2                                                   # eleven significant bits of twelve
    alt = F.conv2d(x10, c.wt.view(64, 3, 3, 8).permute(0, 3, 1, 2).contiguous(), padding=1)
    with pytest.raises(AssertionError, match="elements differ"):
        X.assert_exact(X.expected(alt, F32).permute(0, 2, 3, 1).contiguous(), c.want, "10-bit mantissa")
    assert float((alt - c.ref).abs().max()) <= 1e-3 * float(c.ref.abs().max())      # (a difference of a few 1e-4 of max|ref|)


def test_an_overwritten_destination_is_rejected():
    """The accumulating weight-gradient entry points: the destination starts with non-zero integers everywhere, so a result stored over
    it differs from the expected contents in every element."""
    c = X.wgrad_case(BF16, 3, 2, 8, 32, 16, 16, 3, pooled=1)
    assert len(c.groups) == 2 and c.denom == 4
    for grp in c.groups:
        assert bool((grp.w0 != 0).all()) and bool((grp.b0 != 0).all())
        X.assert_exact((grp.w0 + grp.dw).float(), grp.want_w, "accumulated")
        X.assert_exact((grp.b0 + grp.db).float(), grp.want_b, "accumulated bias")
        with pytest.raises(AssertionError, match="%d of %d elements differ" % (grp.dw.numel(), grp.dw.numel())):
            X.assert_exact(grp.dw.float(), grp.want_w, "overwritten")
        with pytest.raises(AssertionError, match="elements differ"):
            X.assert_exact(grp.db.float(), grp.want_b, "overwritten bias")
    # the two groups are not interchangeable either
    with pytest.raises(AssertionError, match="elements differ"):
        X.assert_exact(c.groups[0].want_w, c.groups[1].want_w, "the other group's buffer")


def test_linear_and_packing_references():
    c = X.linear_case(BF16, 136, 77, 5, "unit")
    assert torch.equal(c.want.double(), c.ref) and int((c.wt != 0).sum(1).max()) <= X.UNIT_NNZ
    c = X.linear_case(F16, 365, 130, 48, "wide")
    assert float(c.x.abs().max()) > 255 and float(c.ref.abs().max()) < X.F16_MAX
    wt = X.integers((5, 3, 3, 3), 100, X.gen(2))
    fwd, dg = X.pack_reference(wt, 8, 8, BF16)
    assert fwd.shape == (5, 9, 8) and dg.shape == (3, 9, 8) and float(fwd[:, :, 3:].abs().max()) == 0 and float(dg[:, :, 5:].abs().max()) == 0
    assert float(fwd[4, 2 * 3 + 1, 2]) == float(wt[4, 2, 2, 1]) and float(dg[2, 0 * 3 + 1, 4]) == float(wt[4, 2, 2, 1])      # tap (2, 1) flips to (0, 1)


def test_assert_exact_reports_the_element_pattern():
    want = torch.zeros(2, 4, 8, 16)
    got = want.clone()
    got[1, :, 7, 3] = 1.0
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, want, "case", names=["n", "row", "col", "ch"])
    msg = str(e.value)
    assert "4 of 1024 elements differ" in msg and "n: [1]" in msg and "col: [7]" in msg and "ch: [3]" in msg and "row: [0, 1, 2, 3]" in msg
    X.assert_exact(torch.tensor([-0.0]), torch.tensor([0.0]))
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([1.0]), torch.tensor([1.0], dtype=torch.float64))
