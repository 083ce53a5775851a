"""Which kernel the accumulating weight-gradient entry points pick, asked through sp_conv2d_wgrad_route (csrc/conv_wgrad.hip: wgrad_plan) -
host logic, no GPU, no launch.

The benchmark's layers: tests/golden/wgrad_routes_b20.json holds every weight-gradient call of one training step at channel_factor 1,
batch 20, in bf16 and fp32 - entry point, integer arguments, scratch lent, whether a bias gradient was asked for - with the route the
launch reported on an MI355X.  The boundary table gives the smallest shape that reaches each route and the nearest shape on the other
side of the rule that admits it."""
import contextlib
import ctypes
import json
import os
import re

import pytest
import torch

from semantic_pyramid_for_image_generation_amd import _lib as L, ops

BF16, F32 = L.SP_BF16, L.SP_F32
TORCH = {BF16: torch.bfloat16, F32: torch.float32, L.SP_F16: torch.float16}
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wgrad_routes_b20.json")
SOURCE = os.path.join(os.path.dirname(L.HEADER), "..", "semantic_pyramid_for_image_generation_amd", "csrc", "conv_wgrad.hip")
ROWS, DET, WGRAD1X1, PP = (L.TUNE_KEYS[k] for k in ("SP_WGRAD_ROWS", "SP_DETERMINISTIC", "SP_WGRAD1X1", "SP_WGRAD_PP"))
NOT_COVERED = "sp_conv2d_wgrad_accum_pooled: shape not covered by the row-walking kernel (w % 32, h % 2)"

CIN8, CIN8_2G = "wgrad3x3_cin8_stream + reduce", "wgrad3x3_cin8_stream (two groups) + 2 x reduce"
S1X1, S1X1_2G = "wgrad1x1_stream + reduce", "wgrad1x1_stream (two groups) + 2 x reduce"
PP3, PP3_2G = "conv_wgrad_pp3 (row walker, ping-pong) + rows_reduce", "conv_wgrad_pp3 (row walker, ping-pong, two groups) + 2 x rows_reduce"
ROWS0, ROWS16, ROWS8 = ("conv_wgrad_rows<%d> + rows_reduce" % nw for nw in (0, 16, 8))
TAP9, TAP_F32, TAP_16 = "conv_wgrad9 (per-tap, <= 64 channels)", "conv_wgrad<f32> (per-tap)", "conv_wgrad<16bit> (per-tap)"


@contextlib.contextmanager
def tuned(knobs):
    try:
        for k, v in knobs.items():
            ops.set_tuning(k, v)
        yield
    finally:
        for k in knobs:
            ops.set_tuning(k, -1)


def scratch(n, h, w, cin_p, cout, ksize=3, dtype=BF16, **_):
    return ops.wgrad_workspace_floats(n, h, w, cin_p, cout, ksize, TORCH[dtype])


def ask(n, h, w, cin_p, cout, ksize=3, dtype=BF16, split=0, pooled=0, dbias=1, ws=None, tune=None):
    """(rc, route or error message) of the query, lent the scratch sp_conv2d_wgrad_workspace asks for (ws: another amount)."""
    with tuned(tune or {}):
        e = 4 if dtype == F32 else 8
        out = ctypes.c_char_p()
        rc = L.lib().sp_conv2d_wgrad_route(n, split, h, w, cin_p, cout, (cout + e - 1) // e * e, ksize, pooled, dbias,
                                           scratch(n, h, w, cin_p, cout, ksize, dtype) if ws is None else ws, dtype, ctypes.byref(out))
        return rc, (out.value.decode() if rc == 0 else L.lib().sp_last_error_string().decode())


def test_benchmark_calls_keep_their_routes():
    fix = json.load(open(GOLDEN))
    seen = set()
    for row in fix["rows"]:
        v = dict(zip(fix["columns"], row))
        pooled = v["entry"] == "sp_conv2d_wgrad_accum_pooled" or v["dy_pooled"]
        assert (v["entry"] == "sp_conv2d_wgrad_accum_pair") == (v["split"] > 0)
        got = L.wgrad_route(v["n"], v["split"], v["h"], v["w_"], v["cin_p"], v["cout"], v["ld_dy"], v["ksize"], pooled, v["want_dbias"],
                            v["workspace_floats"], v["dtype"])
        assert got == v["route"], v
        seen.add((v["dtype"], v["route"]))
    assert len(fix["rows"]) == 104 and len(seen) == 9, (len(fix["rows"]), sorted(seen))
    assert (BF16, PP3_2G) in seen and (BF16, S1X1_2G) in seen and (BF16, CIN8_2G) in seen and (F32, TAP9) in seen


def test_benchmark_calls_are_lent_the_scratch_the_query_sizes():
    fix = json.load(open(GOLDEN))
    ops._WS_CACHE.clear()
    for row in fix["rows"]:
        v = dict(zip(fix["columns"], row))
        assert ops.wgrad_workspace_floats(v["n"], v["h"], v["w_"], v["cin_p"], v["cout"], v["ksize"], TORCH[v["dtype"]]) == v["workspace_floats"], v


# (what, arguments of ask(), route) - default knobs unless `tune` says otherwise; neighbours sit on both sides of one rule
BOUNDARIES = [
    ("8-channel input on 16384 pixels: the streaming kernel", dict(n=1, h=128, w=128, cin_p=8, cout=16), CIN8),
    ("... 8192 pixels: the row walker is fine", dict(n=1, h=64, w=128, cin_p=8, cout=16), PP3),
    ("... two groups whose boundary falls between two pixel splits", dict(n=6, h=128, w=128, cin_p=8, cout=16, split=3), CIN8_2G),
    ("... inside a split: one group after the other", dict(n=6, h=128, w=128, cin_p=8, cout=16, split=2), CIN8),
    ("3x3 on a map 32 wide: the ping-pong row walker", dict(n=1, h=8, w=32, cin_p=16, cout=16), PP3),
    ("... 8 wide: per-tap", dict(n=1, h=8, w=8, cin_p=16, cout=16), TAP_16),
    ("... an odd row count", dict(n=1, h=7, w=32, cin_p=16, cout=16), TAP_16),
    ("... SP_TUNE_WGRAD_ROWS = 0", dict(n=1, h=8, w=32, cin_p=16, cout=16, tune={ROWS: 0}), TAP_16),
    ("... two groups whose boundary falls between two blocks of 8 rows", dict(n=3, h=4, w=32, cin_p=16, cout=16, split=2), PP3_2G),
    ("... inside a block: one group after the other", dict(n=3, h=4, w=32, cin_p=16, cout=16, split=1), PP3),
    ("16 x 16 maps: two images side by side", dict(n=1, h=16, w=16, cin_p=16, cout=16), ROWS16),
    ("... SP_TUNE_WGRAD_ROWS = 2 keeps narrow maps per-tap", dict(n=1, h=16, w=16, cin_p=16, cout=16, tune={ROWS: 2}), TAP_16),
    ("8 x 8 maps walk four images side by side only with SP_TUNE_WGRAD_ROWS = 3", dict(n=1, h=8, w=8, cin_p=16, cout=16, tune={ROWS: 3}), ROWS8),
    ("the 4-wave row walker only with SP_TUNE_WGRAD_PP = 0", dict(n=1, h=8, w=32, cin_p=16, cout=16, tune={PP: 0}), ROWS0),
    ("fp32, w % 32 == 0, 16 .. 64 inputs, <= 64 outputs: all nine taps per block", dict(n=1, h=8, w=32, cin_p=16, cout=64, dtype=F32), TAP9),
    ("... 65 outputs", dict(n=1, h=8, w=32, cin_p=16, cout=65, dtype=F32), TAP_F32),
    ("... 12 inputs", dict(n=1, h=8, w=32, cin_p=12, cout=64, dtype=F32), TAP_F32),
    ("... 68 inputs", dict(n=1, h=8, w=32, cin_p=68, cout=64, dtype=F32), TAP_F32),
    ("... 16 wide", dict(n=1, h=8, w=16, cin_p=16, cout=64, dtype=F32), TAP_F32),
    ("16-bit 1x1: the streaming kernel", dict(n=1, h=8, w=8, cin_p=16, cout=16, ksize=1), S1X1),
    ("... SP_TUNE_WGRAD1X1 = 0", dict(n=1, h=8, w=8, cin_p=16, cout=16, ksize=1, tune={WGRAD1X1: 0}), TAP_16),
    ("... fp32", dict(n=1, h=8, w=8, cin_p=16, cout=16, ksize=1, dtype=F32), TAP_F32),
    ("... two groups whose boundary falls between two splits of 256 pixels", dict(n=4, h=8, w=16, cin_p=16, cout=16, ksize=1, split=2), S1X1_2G),
    ("... inside a split: one group after the other", dict(n=4, h=8, w=16, cin_p=16, cout=16, ksize=1, split=1), S1X1),
]


@pytest.mark.parametrize("what,args,want", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_route_boundaries(what, args, want):
    assert ask(**args) == (0, want)


def test_fp16_storage_takes_the_16bit_routes():
    """SP_F16 goes to the twin compiled for half precision: the same plan, the same names."""
    for _, args, want in BOUNDARIES:
        if args.get("dtype", BF16) == BF16:
            assert ask(**dict(args, dtype=L.SP_F16)) == (0, want)


def test_every_route_name_is_pinned():
    """The twelve strings wgrad_route_name() can return, read from its source, all appear in the boundary table."""
    text = open(SOURCE).read()
    body = text[text.index("const char* wgrad_route_name("):]
    names = set(re.findall(r'"([^"]+)"', body[:body.index("\n}\n")]))
    assert len(names) == 12, sorted(names)
    assert names == {want for _, _, want in BOUNDARIES}


POOLED = [  # (what, uncovered, knobs, its covered neighbour)
    ("a map 16 wide", dict(n=1, h=8, w=16, cin_p=16, cout=16), {}, dict(w=32)),
    ("x of 1 GiB", dict(n=8, h=256, w=256, cin_p=1024, cout=16), {}, dict(n=7)),
    ("dy of 1 GiB", dict(n=8, h=256, w=256, cin_p=16, cout=1024), {}, dict(n=7)),
    ("deterministic mode, 576 tile pairs", dict(n=1, h=8, w=32, cin_p=1536, cout=1536), {DET: 1}, dict(cout=1344)),
]


@pytest.mark.parametrize("what,args,tune,covered", POOLED, ids=[p[0] for p in POOLED])
def test_pooled_gradients_are_read_by_the_row_walker_or_refused(what, args, tune, covered):
    assert ask(pooled=1, tune=tune, **args) == (-1, NOT_COVERED)                       # SP_ERR_INVALID, as the entry point answers
    assert ask(pooled=1, tune=tune, **dict(args, **covered)) == (0, PP3)
    # two groups of such a layer, one after the other: refused as well
    n = 2 * args["n"]
    assert ask(pooled=1, tune=tune, split=n // 2, **dict(args, n=n)) == (-1, NOT_COVERED)


def test_pooled_argument_checks_keep_their_messages():
    assert ask(1, 8, 32, 16, 16, ksize=1, pooled=1) == (-1, "sp_conv2d_wgrad_accum_pooled: bf16 3x3 layers only")
    assert ask(1, 8, 32, 16, 16, dtype=F32, pooled=1) == (-1, "sp_conv2d_wgrad_accum_pooled: bf16 3x3 layers only")
    assert ask(1, 7, 32, 16, 16, pooled=1) == (-1, "sp_conv2d_wgrad_accum_pooled: bad dims")
    assert ask(1, 8, 32, 12, 16, pooled=1) == (-1, "sp_conv2d_wgrad_accum_pooled: cin_p=12 and ld_dy=16 must be multiples of 8")
    # the pair entry point checks what its single-group twin checks
    assert ask(2, 8, 32, 12, 16, split=1) == (-1, "sp_conv2d_wgrad_accum_pair: cin_p=12 and ld_dy=16 must be multiples of 8")
    assert ask(2, 8, 32, 16, 16, split=2) == (-1, "sp_conv2d_wgrad_accum_pair: bad args")
    assert ask(2, 8, 32, 16, 16, ksize=5, ws=0) == (-1, "sp_conv2d_wgrad_accum: ksize 5 unsupported")


SLAB_FLOATS = 512 * (9 * 64 * 64 + 64)       # the row walker's slab area: 512 partial tiles + bias rows (csrc/conv_wgrad_rows.hip)


def stream_floats(n, h, w, cin_p, cout, ksize):
    """What a streaming kernel's plan uses (csrc/conv_wgrad_1x1.hip: w1_split): ~256 blocks over the 64 x 64 tiles of dW and the pixel
    splits, at least four 64-pixel stages per split, one (dW + bias row) slab per split - none for a single split."""
    tiles = (cin_p + 63) // 64 * ((cout + 63) // 64)
    stages = (n * h * w + 63) // 64
    nsplit = max(1, min((256 + tiles - 1) // tiles, stages // 4))
    nsplit = -(-stages // -(-stages // nsplit))
    return nsplit * (cout * ksize * ksize * cin_p + (cout + 3) // 4 * 4) if nsplit > 1 else 0


@pytest.mark.parametrize("what,args,want", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_workspace_query_covers_what_the_route_uses(what, args, want):
    """The query sizes at least the scratch the reported route's plan uses, and with it lent the route carries its reduce-pass name: the
    row walker's slab area; for the streaming kernels the slabs of their pixel splits - lent exactly those the route stays, one float
    less loses it; the per-tap kernels keep their route with any scratch."""
    a = dict(args)
    tune = a.pop("tune", None)
    with tuned(tune or {}):
        ws = scratch(**a)
    assert ask(tune=tune, ws=ws, **a) == (0, want)
    if "rows_reduce" in want:
        assert ws >= SLAB_FLOATS
    elif "reduce" in want:
        split, n = a.get("split", 0), a["n"]
        groups = [n] if split == 0 or "two groups" in want else [split, n - split]
        need = max(stream_floats(g, a["h"], a["w"], a["cin_p"], a["cout"], a.get("ksize", 3)) for g in groups)
        assert ws >= need
        assert ask(tune=tune, ws=need, **a) == (0, want)
        if need:
            assert ask(tune=tune, ws=need - 1, **a)[1] != want
    else:
        assert ask(tune=tune, ws=0, **a) == (0, want)


def test_set_tuning_clears_the_pooled_cache():
    """ops.wgrad_reads_pooled caches the query's answer per shape and set_tuning drops it: 576 tile pairs are covered until the
    deterministic mode is switched on."""
    args = (1, 0, 8, 32, 1536, 1536, 1536, 3, True, scratch(1, 8, 32, 1536, 1536), torch.bfloat16)
    assert ops.wgrad_reads_pooled(*args) and args in ops._POOLED_WGRAD_CACHE
    with tuned({DET: 1}):
        assert not ops._POOLED_WGRAD_CACHE and not ops.wgrad_reads_pooled(*args)
    assert ops.wgrad_reads_pooled(*args)
