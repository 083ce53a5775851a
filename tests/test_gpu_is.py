"""The Inception Score kernels (csrc/metrics.hip) on the GPU, through the C ABI's thin bindings (ops.pairset_lse,
ops.pairset_softmax_colsum) unless stated.

Exact regime (integer activations in {0..3}, class rows of eight +-1, integer bias: every logit is an exact fp32 integer whatever the
order of summation): what is left is float64 exp / log and summation order, and the device is held to the bounds derived in
tests/is_restated.py (R.row_exact_bounds, R.colsum_total_bound, R.kl_exact_bound, all <= 1e-9).  General regime (ReLU-of-normal rows,
d = 72): KL_s within R.kl_general_bound of the float64 restatement.  The operand conditions are asserted on the CPU before any launch."""
import math
import os

import numpy as np
import pytest
import torch

import is_restated as R
from semantic_pyramid_for_image_generation_amd import _lib as L
from semantic_pyramid_for_image_generation_amd import metrics as M
from semantic_pyramid_for_image_generation_amd import ops

pytestmark = pytest.mark.gpu
SEG_KEY = L.TUNE_KEYS["SP_PAIRSET_SEGMENTS"]


def _dev(x):
    torch.cuda.set_device(0)
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _rows(x):
    """fp32 (n, d) on the device with d padded by zero columns to a multiple of 4 (the kernels read d of ld columns)."""
    d = x.shape[1]
    return _dev(np.pad(x, ((0, 0), (0, -d % 4))))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


_CASES = {}


def _exact(n, classes, d):
    """(x, w, b, logits, device operands) of an exact-regime case, conditions asserted, computed once and shared."""
    key = (n, classes, d)
    if key not in _CASES:
        x, w, b, l = R.exact_operands(n, classes, d)
        R.check_exact(x, w, b, l)
        _CASES[key] = (x, w, b, l, (_rows(x), _rows(w), _dev(b)))
    return _CASES[key]


def _check_rows(l, lse, h, what):
    want_lse, want_h, _ = R.row_stats(l)
    e_lse, e_h = R.row_exact_bounds(l.shape[1], R.EXACT_LMAX)
    d_lse = np.abs(lse.cpu().numpy() - want_lse).max()
    d_h = np.abs(h.cpu().numpy() - want_h).max()
    print("%s: max |lse err| %.3e (bound %.3e), max |h err| %.3e (bound %.3e)" % (what, d_lse, e_lse, d_h, e_h))
    assert d_lse <= e_lse and d_h <= e_h, what


# ---- lse / h per row ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 3, 8), (131, 72, 72), (389, 1000, 72), (389, 1000, 2048), (131, 40, 70)], ids=lambda c: "%dx%d_d%d" % c)
def test_lse_and_h_exact(case):
    """(131, 72, 72): a second row block and a partial second class block; C = 1000: 15 full class blocks + 40 classes; (131, 40, 70):
    fewer than 64 classes (the upper half of every row holds 8 of them) and the scalar K tail of d % 4 != 0."""
    n, classes, d = case
    _, _, _, l, (xd, wd, bd) = _exact(n, classes, d)
    lse, h = ops.pairset_lse(xd, wd, bd, d=d)
    assert lse.dtype == h.dtype == torch.float64 and lse.shape == h.shape == (n,)
    _check_rows(l, lse, h, case)


def test_lse_forced_segments_agree_and_repeat_bit_for_bit():
    n, classes, d = 389, 1000, 72
    _, _, _, l, (xd, wd, bd) = _exact(n, classes, d)
    lib = L.lib()
    e_lse, e_h = R.row_exact_bounds(classes, R.EXACT_LMAX)
    got = {}
    try:
        for segments in (1, 3, 7):
            assert lib.sp_set_tuning(SEG_KEY, segments) == 0
            lse, h = ops.pairset_lse(xd, wd, bd, d=d)
            lse2, h2 = ops.pairset_lse(xd, wd, bd, d=d)
            torch.cuda.synchronize()
            _check_rows(l, lse, h, "segments %d" % segments)
            assert torch.equal(_bits(lse), _bits(lse2)) and torch.equal(_bits(h), _bits(h2)), segments
            got[segments] = (lse.cpu().numpy(), h.cpu().numpy())
    finally:
        lib.sp_set_tuning(SEG_KEY, -1)
    for segments in (3, 7):
        assert np.abs(got[segments][0] - got[1][0]).max() <= e_lse and np.abs(got[segments][1] - got[1][1]).max() <= e_h


# ---- colsum and kl --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,splits", [((389, 1000, 72), 1), ((389, 1000, 72), 3), ((389, 1000, 72), 10), ((5, 72, 72), 5),
                                         ((389, 1000, 2048), 10), ((131, 40, 70), 2)], ids=lambda v: str(v).replace(" ", ""))
def test_colsum_and_kl_exact(case, splits):
    """n = 389: S = 3 and 10 put split boundaries inside 128-row blocks of the array, splits 38 and 39 rows long side by side; S = 1 is
    four row blocks of one split; S = n = 5: one row per split, KL = 0."""
    n, classes, d = case
    _, _, _, l, (xd, wd, bd) = _exact(n, classes, d)
    lse, h = ops.pairset_lse(xd, wd, bd, d=d)
    colsum, kl = ops.pairset_softmax_colsum(xd, wd, bd, lse, h, splits, d=d)
    assert colsum.dtype == kl.dtype == torch.float64 and colsum.shape == (splits, classes) and kl.shape == (splits,)
    want_cs, want_kl = R.colsums(l, splits), R.kl_splits(l, splits)
    cs, k = colsum.cpu().numpy(), kl.cpu().numpy()
    for s, (lo, hi) in enumerate(R.split_bounds(n, splits)):
        ns = hi - lo
        tb = R.colsum_total_bound(classes, ns, R.EXACT_LMAX)
        assert abs(cs[s].sum() - ns) <= tb, (s, cs[s].sum(), ns, tb)
        assert np.abs(cs[s] - want_cs[s]).max() <= tb                          # every column too: its error is part of the row's
        kb = R.kl_exact_bound(classes, ns, R.EXACT_LMAX)
        assert kb <= 1e-9 and abs(k[s] - want_kl[s]) <= kb, (s, k[s], want_kl[s], kb)
    print("%s S=%d: max |kl err| %.3e, bound %.3e" % (case, splits, np.abs(k - want_kl).max(), R.kl_exact_bound(classes, n // splits, R.EXACT_LMAX)))
    if splits == n:
        assert np.all(np.abs(k) <= R.kl_exact_bound(classes, 1, R.EXACT_LMAX))
    colsum2, kl2 = ops.pairset_softmax_colsum(xd, wd, bd, lse, h, splits, d=d)
    assert torch.equal(_bits(colsum), _bits(colsum2)) and torch.equal(_bits(kl), _bits(kl2))


# ---- general regime -------------------------------------------------------------------------------------------------------------------
def test_general_regime_kl_within_the_bound():
    x, w, b, l, err = R.general_operands()                        # (389, 1000, 72)
    splits = 3
    want = R.kl_splits(l, splits)
    _, total = R.kl_general_bound(l, err, splits)
    assert np.all(total <= 1e-4 * want)                            # the condition on the inputs, before any launch
    xd, wd, bd = _rows(x), _rows(w), _dev(b)
    lse, h = ops.pairset_lse(xd, wd, bd, d=72)
    _, kl = ops.pairset_softmax_colsum(xd, wd, bd, lse, h, splits, d=72)
    got = kl.cpu().numpy()
    print("general: KL %s, |err| %s, bound %s" % (want, np.abs(got - want), total))
    assert np.all(np.abs(got - want) <= total)
    # every row's lse is within its largest logit error (lse is 1-Lipschitz in the sup norm) and the float64 terms
    e_lse, _ = R.row_exact_bounds(1000, float(np.abs(l).max()))
    assert np.all(np.abs(lse.cpu().numpy() - R.row_stats(l)[0]) <= err.max(axis=1) + e_lse)


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_activation_makes_its_split_nan_and_no_other(bad):
    n, classes, d, splits = 389, 1000, 72, 3
    x, w, b, l, (xd, wd, bd) = _exact(n, classes, d)
    lse, h = ops.pairset_lse(xd, wd, bd, d=d)
    _, clean = ops.pairset_softmax_colsum(xd, wd, bd, lse, h, splits, d=d)
    row = 200                                                      # split 1 of 3: rows 129..258
    assert R.split_bounds(n, splits)[1][0] <= row < R.split_bounds(n, splits)[1][1]
    xb = x.copy()
    xb[row, int(np.flatnonzero(w[5])[0])] = bad                    # a column class 5 reads: a NaN logit, or +-inf ones (and NaN where w = 0)
    xbd = _rows(xb)
    lse_b, h_b = ops.pairset_lse(xbd, wd, bd, d=d)
    _, kl = ops.pairset_softmax_colsum(xbd, wd, bd, lse_b, h_b, splits, d=d)
    kl, clean = kl.cpu(), clean.cpu()
    assert math.isnan(float(kl[1]))
    assert torch.equal(_bits(kl[[0, 2]]), _bits(clean[[0, 2]]))
    assert math.isnan(float(lse_b[row])) and math.isnan(float(h_b[row]))
    keep = torch.from_numpy(np.arange(n) != row)
    assert torch.equal(_bits(lse_b)[keep], _bits(lse)[keep]) and torch.equal(_bits(h_b)[keep], _bits(h)[keep])
    out = M.inception_score(xbd, wd, bd, splits=splits)
    assert math.isnan(out["inception_score"]) and math.isnan(out["inception_score_std"])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_a_message_and_the_outputs_untouched():
    n, classes, d = 131, 72, 72
    _, _, _, _, (xd, wd, bd) = _exact(n, classes, d)
    lib = L.lib()
    lse, h = ops.pairset_lse(xd, wd, bd, d=d)
    mark = -12345.5
    ws = torch.empty(1 << 16, dtype=torch.float64, device=xd.device)
    wsb = ws.numel() * 8
    lse_o, h_o = torch.full((n,), mark, dtype=torch.float64, device=xd.device), torch.full((n,), mark, dtype=torch.float64, device=xd.device)
    colsum_o = torch.full((n + 1, classes), mark, dtype=torch.float64, device=xd.device)
    kl_o = torch.full((n + 1,), mark, dtype=torch.float64, device=xd.device)
    p = ops.ptr

    def lse_call(ld=72, bytes_=wsb):
        return lib.sp_pairset_lse(p(xd), n, ld, p(wd), classes, 72, p(bd), d, p(lse_o), p(h_o), p(ws), bytes_, None)

    def col_call(splits=3, ld=72, bytes_=wsb):
        return lib.sp_pairset_softmax_colsum(p(xd), n, ld, p(wd), classes, 72, p(bd), d, p(lse), p(h), splits, p(colsum_o), p(kl_o), p(ws),
                                             bytes_, None)

    assert ops.pairset_softmax_workspace_bytes(n, classes, d, 3) == max(24 * n * 2, 8 * 3 * classes)
    for call, who in ((lambda: lse_call(ld=68), b"sp_pairset_lse"),                              # ld < d
                      (lambda: lse_call(bytes_=24 * n * 2 - 8), b"sp_pairset_lse"),              # a short workspace (two segments)
                      (lambda: col_call(splits=n + 1), b"sp_pairset_softmax_colsum"),            # n < splits
                      (lambda: col_call(ld=68), b"sp_pairset_softmax_colsum"),
                      (lambda: col_call(bytes_=8 * 3 * classes - 8), b"sp_pairset_softmax_colsum")):
        assert call() != 0
        msg = lib.sp_last_error_string()
        assert who in msg and len(msg) > len(who) + 10, msg
    torch.cuda.synchronize()
    for t in (lse_o, h_o, colsum_o, kl_o):
        assert bool((t == mark).all())
    with pytest.raises(L.SempyrError, match="splits"):
        ops.pairset_softmax_colsum(xd, wd, bd, lse, h, n + 1, d=d)
    assert lse_call() == 0 and col_call() == 0                     # the same calls go through once the arguments are right
    torch.cuda.synchronize()
    assert not bool((lse_o == mark).any()) and not bool((kl_o[:3] == mark).any()) and bool((kl_o[3:] == mark).all())


# ---- metrics.py -----------------------------------------------------------------------------------------------------------------------
def test_inception_score_equals_the_restatement_within_the_propagated_bound():
    n, classes, d, splits = 389, 1000, 72, 10
    x, w, b, l, (xd, wd, bd) = _exact(n, classes, d)
    want_kl = R.kl_splits(l, splits)
    kb = np.array([R.kl_exact_bound(classes, hi - lo, R.EXACT_LMAX) for lo, hi in R.split_bounds(n, splits)])
    want_mean, want_std = R.score_from_kl(want_kl)
    mean_b, std_b = R.score_bounds(want_kl, kb)
    assert mean_b <= 1e-8 and 4.0 < want_mean < 10.0 and want_std > 0.05
    for acts, head in ((xd, (wd, bd)), (x, (w, b)), (x, (wd, bd))):          # device tensors; numpy arrays (uploaded); a mix
        kl = M.inception_kl(acts, head[0], head[1], splits=splits)
        assert isinstance(kl, np.ndarray) and kl.dtype == np.float64 and kl.shape == (splits,)
        assert np.all(np.abs(kl - want_kl) <= kb)
        out = M.inception_score(acts, head[0], head[1], splits=splits)
        assert sorted(out) == ["inception_score", "inception_score_std"]
        assert abs(out["inception_score"] - want_mean) <= mean_b and abs(out["inception_score_std"] - want_std) <= std_b
        assert out == M.inception_score_from_kl(kl)                            # from the same kl: bit-identical launches
    print("IS %.12f +- %.12f, restated %.12f +- %.12f" % (out["inception_score"], out["inception_score_std"], want_mean, want_std))
    assert M.compute(xd, xd, "is", head=(wd, bd), is_splits=splits) == out
    with pytest.raises(L.SempyrError, match=r"fc\.weight"):
        M.compute(xd, xd, "is")


# ---- ModelWrapper.evaluate() end to end -----------------------------------------------------------------------------------------------
def test_evaluate_end_to_end(tmp_path):
    import _fid_child as C
    import inception_restated as IR
    import semantic_pyramid_for_image_generation_amd as sp
    from semantic_pyramid_for_image_generation_amd import fid
    sd = IR.synth_state_dict(21)
    weights = os.path.join(str(tmp_path), "inception_v3_google-random.pth")
    torch.save(sd, weights)
    ops.set_compute_dtype(torch.float32)
    plain, loader = C.setup(weights)
    torch.manual_seed(C.SEED)
    fid_plain = plain.validate()
    net = plain._inception
    mw = sp.ModelWrapper(plain.generator, plain.discriminator, None, loader, vgg16=plain.vgg16, save_data_path=None, inception=net,
                         metrics="kid,is")
    splits = mw.metrics_is_splits = 3
    torch.manual_seed(C.SEED)
    out = mw.evaluate()
    assert sorted(out) == ["fid", "inception_score", "inception_score_std", "kid"]
    assert all(math.isfinite(v) for v in out.values()) and mw.last_metrics == out
    assert out["inception_score"] >= 1.0
    assert mw.generator.training                                   # back in training mode
    assert abs(out["fid"] - fid_plain) <= 1e-9 * abs(fid_plain), (out["fid"], fid_plain)

    # the restatement on the fake activations of fid.collect_activations under the same seed
    torch.manual_seed(C.SEED)
    mw.generator.eval()
    try:
        _, fake = fid.collect_activations(loader, mw.generator, mw.vgg16, device=torch.device("cuda", 0), inception=net)
    finally:
        mw.generator.train()
    assert fake.shape == (C.BATCH * C.BATCHES, 2048)
    w, b = sd["fc.weight"].numpy(), sd["fc.bias"].numpy()
    l = R.logits(fake, w, b)
    want_kl = R.kl_splits(l, splits)
    _, total = R.kl_general_bound(l, R.logit_error(fake, w, b), splits)          # d = 2048: loose (the worst-case gamma), accepted here
    want_mean, want_std = R.score_from_kl(want_kl)
    mean_b, std_b = R.score_bounds(want_kl, total)
    print("IS %.9f +- %.9f, restated %.9f +- %.9f, bounds %.3e / %.3e (KL bound %s)"
          % (out["inception_score"], out["inception_score_std"], want_mean, want_std, mean_b, std_b, total))
    assert abs(out["inception_score"] - want_mean) <= mean_b and abs(out["inception_score_std"] - want_std) <= std_b

    # a state dict without fc.*: "is" names what is missing, before the loader is walked
    bare = sp.ModelWrapper(plain.generator, plain.discriminator, None, loader, vgg16=plain.vgg16, save_data_path=None,
                           inception=IR.synth_state_dict(21, with_fc=False), metrics="is")
    with pytest.raises(L.SempyrError, match=r"fc\.weight"):
        bare.evaluate()
    assert bare.generator.training
