"""The MFMA convolution and linear kernels held to EXACT integer arithmetic (helpers and the reasoning: tests/exact_util.py).

Operands are integers the storage type holds exactly and every partial sum stays below 2^24, so every fp32 accumulation is exact in
any order - atomics, slabs, split-K and the K-split of the last round included - and the stored result must equal the float64
reference after ONE round-to-nearest-even, bit for bit.  No tolerance appears in this module: a case is exact, or it is absent (with
its reason in the table).  Every case is launched twice into outputs pre-filled with two different sentinels (the blocks are
persistent; where the pitch exceeds the channel count the sentinel beyond it must survive).

Left out because they cannot be exact: tanh epilogues (every route the boundary table reaches through tanh is reached here through a
pitch that is no multiple of 8, which takes the same general epilogue) and the fp8 slice (its scales).  The other kernel families
have exact tests of their own: attention in tests/test_gpu_attention_exact.py, batch norm and the bilinear x2 in
tests/test_gpu_norm_exact.py, spectral norm and the loss-scale guards in tests/test_gpu_sn_exact.py and
tests/test_gpu_optim_guard_exact.py, the pooling kernels in tests/test_gpu_pool_exact.py, the discriminator head and the losses in
tests/test_gpu_loss_exact.py.  Still without: the elementwise kernels of csrc/eltwise.hip."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_util as X
from semantic_pyramid_for_image_generation_amd import _lib as L, ops
from test_conv_routes import BF16 as SP_BF16, BOUNDARIES, F32 as SP_F32, TANH
from test_gpu_fid import FORMS, _run_conv
from test_gpu_ops import PP_SPLIT_CASES, PPW_SPLIT_CASES, ROUTE_CASES, WGRAD_ROUTE_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, B16, H16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "fp32", B16: "bf16", H16: "fp16"}
SENTINELS = (-1024.0, 1536.0)
NHWC = ["image", "row", "column", "channel"]
SEEN, SEEN_ROWS = set(), set()               # (fp32 storage, route) of every forward launch; the route rows that ran
WSEEN, WSEEN_ROWS = set(), set()             # the same for the weight gradient


def _id(v):
    if isinstance(v, torch.dtype):
        return NAME[v]
    if isinstance(v, str):
        return v
    if isinstance(v, dict):
        return "+".join("%s=%d" % kv for kv in sorted(v.items()))
    if isinstance(v, tuple) and v and isinstance(v[0], str):
        return v[0]
    if isinstance(v, tuple):
        return "-".join(str(a) for a in [a for a in v if isinstance(a, int) and not isinstance(a, bool)][:6])
    return "default"


def _last_route() -> str:
    return L.lib().sp_last_route().decode()


@contextlib.contextmanager
def knobs(kn):
    try:
        for key, v in (kn or {}).items():
            ops.set_tuning(L.TUNE_KEYS[key], v)
        yield
    finally:
        for key in (kn or {}):
            ops.set_tuning(L.TUNE_KEYS[key], -1)


def _nhwc(t, dt, ld=None):
    """float64 NCHW on the host -> dense [n][h][w][ld] in dt on the device (channels past c zero), checked to hold the same integers."""
    n, c, h, w = t.shape
    out = torch.zeros((n, h, w, ld or c), dtype=dt)
    out[..., :c] = t.permute(0, 2, 3, 1).to(dt)
    assert torch.equal(out[..., :c].double(), t.permute(0, 2, 3, 1)), "the storage type does not hold an operand exactly"
    return out.to(DEV)


def _rows(t, dt):
    out = t.to(dt).contiguous()
    assert torch.equal(out.double(), t), "the storage type does not hold an operand exactly"
    return out.to(DEV)


@functools.lru_cache(maxsize=2)
def _conv_case(*args, **kw):
    return X.conv_case(*args, **kw)


# ----------------------------------------------------------------------------------------------
# forward convolution: ops._conv_launch on raw packed weights
# ----------------------------------------------------------------------------------------------
def run_forward(dt, n, h, w, cin, cout, k, regime, route=None, exact_route=False, ldy=None, idx=False, kn=None, build_dt=None, amax=None,
                **ep):
    """ep: the epilogue of exact_util.conv_case.  build_dt: the operands of another storage type's case (shared reference)."""
    c = _conv_case(build_dt or dt, n, h, w, cin, cout, k, regime, amax=amax, **ep)
    want = c.want
    if build_dt is not None and build_dt != dt:
        X.check_reference(c.v, c.bound, dt, regime, c.denom, c.what)
        want = X.expected(c.ref, dt).permute(0, 2, 3, 1).contiguous()
    ld = ldy or cout
    act, pool2, up, groups = ep.get("act", 0), ep.get("pool2", 0), ep.get("up", False), ep.get("groups", False)
    xd = _nhwc(c.x, dt)
    wd = _rows(c.wt, dt)
    bd = c.b.float().to(DEV) if c.b is not None else None
    rd = [_nhwc(r, dt, ld) for r in c.rs] + [None, None]
    md = _nhwc(c.ms, dt, ld) if c.ms is not None else None
    scales = torch.tensor([0.5, 2.0], device=DEV) if groups else None
    what = "%s %s" % (NAME[dt], (n, h, w, cin, cout, k, regime, ldy, sorted(ep.items())))
    for s in SENTINELS:
        y = torch.full((n, c.ho, c.wo, ld), s, dtype=dt, device=DEV)
        pidx = torch.full((n * c.ho * c.wo * (cout // 16),), -1, dtype=torch.int32, device=DEV) if idx else None
        with knobs(kn):
            ops._conv_launch(xd, wd.data_ptr(), bd, y, rd[0], rd[1], md, 0.25, n, h, w, cin, cout, ld, k, act, dt, pool2, up,
                             img_scale=scales.data_ptr() if groups else 0, img_split=c.split if groups else 0, pool_idx=pidx)
            got_route = _last_route()
        SEEN.add((dt == F32, got_route))
        if route is not None:
            assert got_route == route if exact_route else got_route.startswith(route), (what, got_route, route)
        X.assert_exact(y[..., :cout], want, "%s on %s" % (what, got_route), NHWC)
        if ld > cout:
            X.assert_sentinel(y[..., cout:], s, what)
        if idx:
            _check_pool_routing(c, y, pidx, dt, n, h, w, cout, what)
    return got_route


def _check_pool_routing(c, y, pidx, dt, n, h, w, cout, what):
    """sp_maxpool2_bwd_idx on an integer gradient against float64 autograd of relu(max_pool2d(.)): the first maximum in scan order
    takes the gradient where the pooled value is positive.  By design (include/sempyr.h: pool_idx) the maximum is taken over the
    values AS THE STORAGE TYPE HOLDS THEM - the element the unfused pooling would pick from the stored tensor - so two sums that
    differ exactly but round to one 16-bit value tie, and the first wins: the reference pools the once-rounded conv + bias (rounding
    is monotone: the pooled VALUES above are unaffected)."""
    gy = X.integers((n, cout, h // 2, w // 2), 16, X.gen(77))
    leaf = X.expected(c.pre + (c.b.view(1, -1, 1, 1) if c.b is not None else 0.0), dt).double().requires_grad_(True)
    torch.relu(F.max_pool2d(leaf, 2)).backward(gy)
    dx = torch.full((n, h, w, cout), 99.0, dtype=dt, device=DEV)
    L.call("sp_maxpool2_bwd_idx", ops.ptr(_nhwc(gy, dt)), ops.ptr(y), ops.ptr(pidx), ops.ptr(dx), n, h, w, cout, ops.sp_dtype(dt), ops.stream())
    X.assert_exact(dx, leaf.grad.permute(0, 2, 3, 1).contiguous().to(dt), what + ": gradient routed by pool_idx", NHWC)


def _route_rows():
    """Every row of ROUTE_CASES, then the first row of tests/test_conv_routes.py's boundary table for every route not among them (tanh
    rows aside), then the two routes that table reaches through tanh only, reached through a pitch of the output that is no multiple of
    8: the same general epilogue, and exact."""
    rows = [(dt, n, h, w, cin, cout, k, None, route) for dt, n, h, w, cin, cout, k, route in ROUTE_CASES]
    have = {(r[0] == F32, r[-1]) for r in rows}
    for _, a, want in BOUNDARIES:
        key = (a.get("dtype", SP_BF16) == SP_F32, want)
        if key in have or a.get("act") == TANH or a.get("lend") is False:
            continue
        have.add(key)
        rows.append((F32 if key[0] else B16, a["n"], a["h"], a["w"], a["cin_p"], a["cout"], a.get("ksize", 3), a.get("ldy"), want))
    rows += [(B16, 1, 16, 32, 32, 64, 3, 84, "conv3x3_pp<16bit,1>"), (B16, 8, 64, 64, 96, 512, 3, 516, "conv3x3_tall<16bit,2,16>")]
    return rows


ROUTE_ROWS = _route_rows()
# routes of the pinned set that no exact case reaches (at most two, each with its reason): none - see _route_rows
EXCLUDED = set()


def _rid(r):
    return "%s-%dx%dx%d-%d-%d-k%d%s" % (NAME[r[0]], r[1], r[2], r[3], r[4], r[5], r[6], "-ld%d" % r[7] if r[7] else "")


@pytest.mark.parametrize("regime", ["unit", "wide", "wide-w"])
@pytest.mark.parametrize("row", ROUTE_ROWS, ids=_rid)
def test_forward_smallest_shape_of_every_route(row, regime):
    dt, n, h, w, cin, cout, k, ldy, route = row
    assert run_forward(dt, n, h, w, cin, cout, k, regime, route=route, exact_route=True, ldy=ldy) == route
    SEEN_ROWS.add((row, regime))


# (n, h, w, cin, cout, k, route) - partial output-channel tiles (80, 136, 320, 520), partial K chunks (72, 136, 264, 520), maps that are
# no tile multiples where a route takes them (5 x 7, 12 x 24, 40 x 24), batch > 1; never the benchmark's sizes
EDGES_16 = [
    (2, 8, 32, 72, 80, 3, "conv3x3_pp<16bit,2,FAST>"), (1, 16, 64, 136, 136, 3, "conv3x3_pp<16bit,2>"),
    (1, 8, 32, 264, 320, 3, "conv3x3_pp<16bit,2,FAST>"), (2, 8, 32, 520, 136, 3, "conv3x3_pp<16bit,2>"),
    (2, 16, 32, 72, 64, 3, "conv3x3_pp<16bit,1,FAST>"), (1, 16, 32, 136, 40, 3, "conv3x3_pp<16bit,1>"),
    (2, 32, 64, 264, 48, 3, "conv3x3_pp<16bit,1,FAST>"),
    (2, 8, 32, 72, 64, 3, "conv3x3_halo<16bit>"), (3, 24, 32, 136, 56, 3, "conv3x3_halo<16bit>"),
    (2, 5, 7, 72, 80, 3, "conv_igemm_dma+finalize (split-K)"), (1, 12, 24, 136, 136, 3, "conv_igemm_dma+finalize (split-K)"),
    (1, 40, 24, 264, 320, 3, "conv_igemm_dma+finalize (split-K)"), (3, 5, 7, 520, 136, 3, "conv_igemm_dma+finalize (split-K)"),
    (2, 12, 24, 72, 16, 3, "conv_igemm (register-staged)"),
    (32, 16, 16, 72, 320, 3, "conv3x3_pp<16bit,2,FAST,w16>"), (16, 16, 16, 136, 520, 3, "conv_igemm_dma"),
    (8, 64, 64, 104, 512, 3, "conv3x3_ppw<16bit> (64 co x 4 rows per wave)"),
    (2, 16, 64, 64, 4, 3, "conv3x3_thinco"), (3, 8, 32, 32, 2, 3, "conv3x3_thinco"), (2, 16, 32, 8, 64, 3, "conv3x3_cin8"),
    (2, 5, 7, 72, 80, 1, "conv1x1_direct"), (3, 12, 24, 136, 136, 1, "conv1x1_splitk"), (2, 5, 7, 520, 80, 1, "conv1x1_splitk"),
]
EDGES_F32 = [
    (2, 16, 32, 12, 40, 3, "conv3x3_tall<f32,1,16>"), (2, 8, 32, 72, 80, 3, "conv3x3_tall<f32,2,8>"), (2, 8, 32, 36, 56, 3, "conv3x3_halo<f32>"),
    (2, 5, 7, 36, 80, 3, "conv_igemm_dma+finalize (split-K)"), (1, 12, 24, 72, 136, 3, "conv_igemm_dma+finalize (split-K)"),
]
EDGE_RUNS = [(B16, "unit", e) for e in EDGES_16] + [(H16, "wide", e) for e in EDGES_16] + [(B16, "wide", e) for e in EDGES_16[::3]] + \
            [(F32, r, e) for e in EDGES_F32 for r in ("unit", "wide")]


@pytest.mark.parametrize("dt,regime,edge", EDGE_RUNS, ids=_id)
def test_forward_edges_of_tiles_chunks_and_maps(dt, regime, edge):
    n, h, w, cin, cout, k, route = edge
    run_forward(dt, n, h, w, cin, cout, k, regime, route=route, exact_route=True, bias=True)


# (name, storage, n, h, w, cin, cout, k, route prefix, knobs, takes pooling and the pooled-gradient input)
EPILOGUE_BASES = [
    ("pp2", B16, 2, 16, 32, 72, 80, 3, "conv3x3_pp<16bit,2", None, True), ("pp1", B16, 2, 16, 32, 72, 64, 3, "conv3x3_pp<16bit,1", None, True),
    ("halo", B16, 2, 8, 32, 72, 64, 3, "conv3x3_halo<16bit>", None, True), ("ppw", B16, 2, 16, 32, 72, 144, 3, "conv3x3_ppw", {"SP_CONV_PPW": 2}, True),
    ("tall-fp32", F32, 2, 16, 32, 36, 80, 3, "conv3x3_tall<f32,2,8>", None, True), ("pp2-fp16", H16, 2, 16, 32, 72, 80, 3, "conv3x3_pp<16bit,2", None, True),
    ("igemm", B16, 2, 5, 7, 72, 80, 3, "conv_igemm_dma", None, False), ("1x1", B16, 3, 12, 24, 136, 136, 1, "conv1x1", None, False),
]
# epilogue operands in exact form (include/sempyr.h: sp_conv_params); tanh is absent: it is not exact
EPILOGUES = [
    ("bias-relu", dict(bias=True, act=2), False), ("bias-res1-lrelu", dict(bias=True, res=1, act=1), False), ("res2", dict(res=2), False),
    ("mask-bias-res1", dict(mask=True, bias=True, res=1), False), ("groups-bias-res1", dict(groups=True, bias=True, res=1), False),
    ("avgpool-bias-res2", dict(pool2=1, bias=True, res=2), True), ("avgpool-groups-res1", dict(pool2=1, groups=True, bias=True, res=1), True),
    ("maxpool-bias-relu", dict(pool2=2, bias=True, act=2), True), ("maxpool-bias-relu-idx", dict(pool2=2, bias=True, act=2, idx=True), True), ("up2-mask", dict(up=True, mask=True), True),
    ("up2-groups", dict(up=True, groups=True), True),
]
# (conv_ppw.hip records no window positions: with pool_idx the launch goes to conv_pp.hip, which the pp2 base covers)
EPILOGUE_RUNS = [(b, e, r) for b in EPILOGUE_BASES for e in EPILOGUES for r in ("unit", "wide")
                 if (b[10] or not e[2]) and not (b[0] == "ppw" and e[1].get("idx"))]


@pytest.mark.parametrize("base,ep,regime", EPILOGUE_RUNS, ids=_id)
def test_forward_epilogue_operands(base, ep, regime):
    _, dt, n, h, w, cin, cout, k, route, kn, _ = base
    run_forward(dt, n, h, w, cin, cout, k, regime, route=route, kn=kn, **ep[1])


_PP_SPLITS = {(3, 160, 128, 32, 64), (4, 256, 256, 64, 64), (11, 264, 384, 32, 64), (33, 136, 128, 64, 64)}
_PPW_SPLITS = {(20, 512, 256, 32, 32), (36, 192, 128, 64, 64)}
SPLIT_RUNS = [(c, None, dt) for c in PP_SPLIT_CASES if c[:5] in _PP_SPLITS for dt in (B16, H16)] + \
             [(c, {"SP_CONV_PPW": 2}, dt) for c in PPW_SPLIT_CASES if c[:5] in _PPW_SPLITS for dt in (B16, H16)]


@pytest.mark.parametrize("case,kn,dt", SPLIT_RUNS, ids=_id)
def test_forward_k_split_of_the_last_round(case, kn, dt):
    """conv_pp.hip / conv_ppw.hip (forced): the smallest cases of the tail-split tables whose last round splits K, in the wide regime -
    a partial tile handed over in 16 bits would show - on operands both 16-bit types hold (one reference for the two); the counters of
    the caller's area are zero afterwards."""
    n, cin, cout, h, w, act, res, mask, pool2, up, bias, groups = case
    assert len(SPLIT_RUNS) == 12
    route = run_forward(dt, n, h, w, cin, cout, 3, "wide", route="conv3x3_ppw" if kn else "conv3x3_pp<16bit,2", kn=kn, build_dt=B16,
                        bias=bias, res=res, act=act, mask=mask, pool2=pool2, up=up, groups=groups)
    assert ops.conv_workspace_bytes(n, h, w, cin, cout, 3, dt) > 0, route
    torch.cuda.synchronize()
    assert ops._SPLIT_SYNC
    for t in ops._SPLIT_SYNC.values():
        assert int(t.abs().sum()) == 0


def test_forward_cases_reach_every_route_of_the_default_knobs():
    """The route rows name every (storage, route) pair tests/test_conv_routes.py pins for the default knobs, less EXCLUDED; where all of
    them ran in this session, the launches reported them all."""
    pinned = {(a.get("dtype", SP_BF16) == SP_F32, want) for _, a, want in BOUNDARIES}
    assert len(pinned) == 23 and len(EXCLUDED) <= 2
    assert pinned - EXCLUDED <= {(r[0] == F32, r[-1]) for r in ROUTE_ROWS}
    if len(SEEN_ROWS) == 3 * len(ROUTE_ROWS):
        assert pinned - EXCLUDED <= SEEN, sorted(pinned - EXCLUDED - SEEN)


# ----------------------------------------------------------------------------------------------
# packing and input gradient
# ----------------------------------------------------------------------------------------------
# (real cin, real cout, k, n, h, w, storage): the roles of Cin and Cout swap in the launch - Cin 3 -> 8 and 513 -> 520 give partial
# output tiles with a padded pitch, Cout 3 and 80 a padded reduction (cout_p)
DGRAD_CASES = [(3, 64, 3, 1, 8, 32, B16), (513, 64, 3, 1, 8, 32, B16), (64, 3, 3, 2, 16, 32, B16), (72, 80, 3, 2, 16, 32, B16), (72, 80, 3, 2, 5, 7, B16),
               (513, 80, 1, 2, 8, 8, B16), (3, 64, 1, 2, 8, 8, B16), (64, 80, 3, 2, 16, 32, H16), (3, 64, 3, 1, 16, 32, F32), (36, 80, 3, 2, 8, 32, F32)]
# ... and the shape of every forward route row as the input-gradient launch of the layer with Cin and Cout exchanged
DGRAD_CASES += [(cout, cin, k, n, h, w, dt) for dt, n, h, w, cin, cout, k, _ in ROUTE_CASES]


@pytest.mark.parametrize("regime", ["unit", "wide-w"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "%s-%d-%d-k%d-%dx%dx%d" % (NAME[c[6]], c[0], c[1], c[2], c[3], c[4], c[5]))
def test_packings_and_input_gradient(case, regime):
    """sp_pack_weight on a ternary / 8-bit fp32 weight: both packings equal their torch permutation bit for bit (flipped taps for the
    input gradient, zeros in the cin_p / cout_p padding, written into a dirty buffer); then the input gradient of an integer dy
    through the dgrad packing against float64 conv_transpose2d."""
    cin, cout, k, n, h, w, dt = case
    g = X.gen(5)
    e = ops.chunk_elems(dt)
    cin_p, cout_p = ops.pad_to(cin, e), ops.pad_to(cout, e)
    kk = k * k * cout
    if regime == "unit":
        rows = X.sparse_ternary_rows(cin, kk, g)
    else:
        rows = X.integers((cin, kk), X.f16_amax(min(255, X.wide_amax(dt, k * k * cout_p)), kk, dt), g)
    wt = rows.view(cin, k, k, cout).permute(3, 0, 1, 2).contiguous()              # OIHW
    dy = X.ternary((n, cout, h, w), g)
    ref = F.conv_transpose2d(dy, wt, padding=k // 2)
    X.check_reference(ref, float(rows.abs().sum(1).max()), dt, regime, 1, case)
    fwd = torch.full((cout * k * k * cin_p,), 3.0, dtype=dt, device=DEV)
    dg = torch.full((cin * k * k * cout_p,), 3.0, dtype=dt, device=DEV)
    L.call("sp_pack_weight", ops.ptr(wt.float().to(DEV)), cout, cin * k * k, cin, k * k, cin_p, cout_p, 0, 0, ops.ptr(fwd), ops.ptr(dg),
           ops.sp_dtype(dt), ops.stream())
    want_fwd, want_dg = X.pack_reference(wt, cin_p, cout_p, dt)
    X.assert_exact(fwd.view(cout, k * k, cin_p), want_fwd, "forward packing", ["cout", "tap", "cin_p"])
    X.assert_exact(dg.view(cin, k * k, cout_p), want_dg, "input-gradient packing", ["cin", "tap", "cout_p"])
    dyd = _nhwc(dy, dt, cout_p)
    want = X.expected(ref, dt).permute(0, 2, 3, 1).contiguous()
    for s in SENTINELS:
        dx = torch.full((n, h, w, cin_p), s, dtype=dt, device=DEV)
        ops._conv_launch(dyd, dg.data_ptr(), None, dx, None, None, None, 0.25, n, h, w, cout_p, cin, cin_p, k, 0, dt)
        SEEN.add((dt == F32, _last_route()))
        X.assert_exact(dx[..., :cin], want, "%s dx on %s" % (case, _last_route()), NHWC)
        if cin_p > cin:
            X.assert_sentinel(dx[..., cin:], s, case)


# ----------------------------------------------------------------------------------------------
# weight and bias gradient: the accumulating entry points
# ----------------------------------------------------------------------------------------------
# the rows of WGRAD_ROUTE_CASES (route asserted); the narrow maps of test_wgrad_row_walker_narrow_maps_bf16 (SP_WGRAD_ROWS = 3) and three of
# WGRAD_1X1_CASES as (route or None, storage, n, split, h, w, cin, cout, k, pooled, bias gradient, knobs)
_NARROW = [(128, 256, 3, 2, 8, 8), (520, 128, 3, 1, 8, 8), (64, 72, 3, 5, 8, 8), (512, 512, 3, 20, 8, 8), (72, 64, 3, 3, 16, 16)]
_STREAM = [(72, 128, 1, 3, 41, 24), (64, 136, 1, 2, 32, 48), (8, 48, 3, 3, 64, 128)]
WGRAD_RUNS = list(WGRAD_ROUTE_CASES) + \
    [(None, B16, n, 0, h, w, cin, cout, k, 0, 1, {"SP_WGRAD_ROWS": 3}) for cin, cout, k, n, h, w in _NARROW] + \
    [(None, B16, n, 0, h, w, cin, cout, k, 0, 1, {}) for cin, cout, k, n, h, w in _STREAM]


@pytest.mark.parametrize("case", WGRAD_RUNS, ids=lambda c: "%s-%s-n%d.%d-%dx%d-%d-%d-k%d%s" % ((c[0] or "any").split(" ")[0], NAME[c[1]], c[2], c[3], c[4], c[5],
                                                                                             c[6], c[7], c[8], "-pooled" if c[9] else ""))
def test_weight_and_bias_gradient_accumulate_exactly(case):
    """sp_conv2d_wgrad_accum / _pooled / _pair into destinations that start with non-zero integers (an overwrite fails), two groups into
    their two buffers, against float64 autograd; the floats around the destinations keep their marker."""
    want_route, dt, n, split, h, w, cin, cout, k, pooled, bias, kn = case
    c = X.wgrad_case(dt, n, split, h, w, cin, cout, k, pooled)
    cp = ops.pad_to(cout, ops.chunk_elems(dt))
    xd, dyd = _nhwc(c.x, dt), _nhwc(c.dy, dt, cp)
    ndw = cout * k * k * cin
    for rep in range(2):
        bufs = []
        for grp in c.groups:
            buf = torch.full((ndw + cout + 8,), 7.0)
            buf[:ndw] = grp.w0.flatten().float()
            buf[ndw + 4:ndw + 4 + cout] = grp.b0.float()
            bufs.append(buf.to(DEV))
        dws = [ops.ptr(b) for b in bufs]
        dbs = [ctypes.c_void_p(b.data_ptr() + 4 * (ndw + 4)) if bias else None for b in bufs]
        with knobs(kn):
            floats = ops.wgrad_workspace_floats(n, h, w, cin, cout, k, dt)
            ws = torch.empty(floats, device=DEV) if floats else None
            if split:
                L.call("sp_conv2d_wgrad_accum_pair", ops.ptr(xd), ops.ptr(dyd), dws[0], dbs[0], dws[1], dbs[1], ops.ptr(ws), floats, n, split, h, w, cin,
                       cout, cp, k, pooled, ops.sp_dtype(dt), ops.stream())
            else:
                L.call("sp_conv2d_wgrad_accum_pooled" if pooled else "sp_conv2d_wgrad_accum", ops.ptr(xd), ops.ptr(dyd), dws[0], dbs[0], ops.ptr(ws), floats,
                       n, h, w, cin, cout, cp, k, ops.sp_dtype(dt), ops.stream())
            got_route = _last_route()
        WSEEN.add(got_route)
        if want_route is not None:
            assert got_route == want_route, (case, got_route)
        for buf, grp in zip(bufs, c.groups):
            what = "%s images [%d, %d) on %s" % (case[1:11], grp.lo, grp.hi, got_route)
            X.assert_exact(buf[:ndw].view(cout, k * k, cin), grp.want_w, "dW " + what, ["cout", "tap", "cin"])
            X.assert_exact(buf[ndw + 4:ndw + 4 + cout], grp.want_b if bias else grp.b0.float(), "dbias " + what, ["cout"])
            X.assert_sentinel(buf[ndw:ndw + 4], 7.0, what)
            X.assert_sentinel(buf[ndw + 4 + cout:], 7.0, what)
    if want_route is not None:
        WSEEN_ROWS.add(case[:11])


def test_weight_gradient_cases_reach_every_route_name():
    names = {c[0] for c in WGRAD_ROUTE_CASES}
    assert len(names) == 12                    # every string wgrad_route_name() can return (tests/test_wgrad_routes.py)
    if len(WSEEN_ROWS) == len(WGRAD_ROUTE_CASES):
        assert names <= WSEEN, sorted(names - WSEEN)


# ----------------------------------------------------------------------------------------------
# linear: ops.linear_launch with both packings, sp_linear_wgrad
# ----------------------------------------------------------------------------------------------
# (k, n, batch, forward only) of test_sn_linear: one launch; slabs + finalize; the four-fragment form of 33 - 64 rows
LINEAR_SHAPES = [(128, 128, 2, False), (136, 77, 5, False), (4096, 365, 3, False), (128, 16384, 20, True), (365, 130, 48, False), (2048, 1000, 33, False)]
LINEAR_RUNS = [(s, dt, r) for s in LINEAR_SHAPES for dt in (B16, F32) for r in ("unit", "wide", "wide-w")] + \
              [(s, H16, "wide") for s in LINEAR_SHAPES[1:4]]


@pytest.mark.parametrize("shape,dt,regime", LINEAR_RUNS, ids=_id)
def test_linear_forward_input_gradient_and_weight_gradient(shape, dt, regime):
    k, n, b, fwd_only = shape
    c = X.linear_case(dt, k, n, b, regime)
    kp, np_ = ops.pad_to(k, 8), ops.pad_to(n, 8)
    fwd = torch.full((n * kp,), 3.0, dtype=dt, device=DEV)
    dg = torch.full((k * np_,), 3.0, dtype=dt, device=DEV)
    L.call("sp_pack_weight", ops.ptr(c.wt.float().to(DEV)), n, k, k, 1, kp, np_, 0, 0, ops.ptr(fwd), ops.ptr(dg), ops.sp_dtype(dt), ops.stream())
    want_fwd, want_dg = X.pack_reference(c.wt.view(n, k, 1, 1), kp, np_, dt)
    X.assert_exact(fwd.view(n, 1, kp), want_fwd, "forward packing", ["n", "tap", "kp"])
    X.assert_exact(dg.view(k, 1, np_), want_dg, "input-gradient packing", ["k", "tap", "np"])
    xd, bd, rd = _rows(c.x, dt), c.bias.float().to(DEV), _rows(c.res, dt)
    for s in SENTINELS:
        y = torch.full((b, n), s, dtype=dt, device=DEV)
        ops.linear_launch(xd, fwd.data_ptr(), kp, bd, rd, y, b, k, n, ops.ACT_RELU)
        X.assert_exact(y, c.want, "%s y" % (c.what,), ["row", "n"])
    if fwd_only:
        return
    dzd = _rows(c.dz, dt)
    for s in SENTINELS:
        dx = torch.full((b, k), s, dtype=dt, device=DEV)
        ops.linear_launch(dzd, dg.data_ptr(), np_, None, None, dx, b, n, k, ops.ACT_NONE)
        X.assert_exact(dx, c.want_dx, "%s dx" % (c.what,), ["row", "k"])
    if dt == H16:
        return                                # sp_linear_wgrad takes fp32 and bf16 storage
    dztd = _rows(c.dzt, dt)
    for s in SENTINELS:
        dw = torch.full((n, kp), s, dtype=torch.float32, device=DEV)
        db = torch.full((n,), s, dtype=torch.float32, device=DEV)
        L.call("sp_linear_wgrad", ops.ptr(xd), k, ops.ptr(dztd), n, ops.ptr(dw), kp, ops.ptr(db), b, k, n, ops.sp_dtype(dt), ops.stream())
        X.assert_exact(dw[:, :k], c.want_dw, "%s dW" % (c.what,), ["n", "k"])
        X.assert_exact(dw[:, k:], torch.zeros(n, kp - k), "%s dW padding" % (c.what,), ["n", "k"])
        X.assert_exact(db, c.want_db, "%s dbias" % (c.what,), ["n"])


# ----------------------------------------------------------------------------------------------
# the Inception extractor's general convolution
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [B16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%dx%d_s%d_p%d%d_c%d-%d_%d" % (f[2] + (f[3],) + f[4] + (f[0], f[1], f[5])))
def test_general_convolution_forms(form, dt):
    """sp_conv2d_general over the 14 forms of tests/test_gpu_fid.py at batch 1 in the unit regime: relu(conv + bias), every product
    counts."""
    cin, cout, (kh, kw), stride, pad, hw = form
    g = X.gen(9)
    x = X.ternary((1, cin, hw, hw), g)
    wt = X.sparse_ternary_rows(cout, cin * kh * kw, g).view(cout, cin, kh, kw)
    b = X.integers((cout,), X.UNIT_BIAS, g)
    v = F.conv2d(x, wt, b, stride=stride, padding=pad)
    X.check_reference(v, float(wt.abs().sum((1, 2, 3)).max()) + X.UNIT_BIAS, dt, "unit", 1, form)
    want = X.expected(torch.relu(v), dt).permute(0, 2, 3, 1).contiguous()
    for s in SENTINELS:
        y = torch.full(tuple(want.shape), s, dtype=dt)
        got = _run_conv(x.float(), wt.float(), b.float(), dt, stride, pad, y=y)
        X.assert_exact(got, want, "%s %s" % (NAME[dt], form), NHWC)
