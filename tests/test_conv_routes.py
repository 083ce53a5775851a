"""Which kernel sp_conv2d_igemm picks, asked through sp_conv2d_route (csrc/conv_igemm.hip: conv_plan) - host logic, no GPU, no launch.

The benchmark's layers: tests/golden/conv_routes_b20.json holds every parameter block of one training step at channel_factor 1,
batch 20, in bf16 and fp32, with the route the launch reported on an MI355X.  The boundary table gives the smallest shape that
reaches each route with default knobs and the nearest shape on the other side of the rule that admits it."""
import ctypes
import json
import os

import pytest
import torch

from semantic_pyramid_for_image_generation_amd import _lib as L, ops

BF16, F32, F8 = L.SP_BF16, L.SP_F32, L.SP_F8
TORCH = {BF16: torch.bfloat16, F32: torch.float32}
PTR = 64            # any non-NULL address: the plan never dereferences a pointer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes_b20.json")


def block(n, h, w, cin_p, cout, ksize=3, dtype=BF16, lend=True, **fields):
    """A parameter block as ops._conv_launch fills it: the scratch sp_conv2d_workspace asks for (lend=False: none), the counters with it
    for 16-bit storage.  `fields` override anything."""
    p = L.SpConvParams()
    p.x = p.w = p.y = PTR
    p.n, p.h, p.w_, p.cin_p, p.cout, p.ldy, p.ksize, p.dtype = n, h, w, cin_p, cout, cout, ksize, dtype
    ws = ops.conv_workspace_bytes(n, h, w, cin_p, cout, ksize, TORCH[dtype]) if lend and dtype in TORCH else 0
    if ws:
        p.workspace, p.workspace_bytes = PTR, ws
        if dtype != F32:
            p.split_sync = PTR
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_benchmark_layers_keep_their_routes():
    fix = json.load(open(GOLDEN))
    ints, ptrs = fix["ints"], fix["pointers"]
    seen = set()
    ops._CONV_WS_CACHE.clear()
    for row in fix["rows"]:
        v = dict(zip(ints, row[:len(ints)]))
        flags, want = row[len(ints)], row[len(ints) + 1]
        p = L.SpConvParams()
        p.x = p.w = PTR
        for k, x in v.items():
            setattr(p, k, x)
        for k, f in zip(ptrs, flags):
            if f == "1":
                setattr(p, k, PTR)
        assert L.conv_route(p) == want, (v, flags)
        # the scratch recorded is the scratch the query sizes (ops._conv_launch lends exactly that)
        assert ops.conv_workspace_bytes(v["n"], v["h"], v["w_"], v["cin_p"], v["cout"], v["ksize"], TORCH[v["dtype"]]) == v["workspace_bytes"], v
        seen.add((v["dtype"], want))
    assert len(fix["rows"]) == 325 and len(seen) == 18, (len(fix["rows"]), sorted(seen))
    # the routes of bench.py's dominant-kernel accounting are among them
    assert (BF16, "conv3x3_pp<16bit,2,FAST>") in seen and (F32, "conv3x3_tall<f32,2,8>") in seen


TANH = L.ACT_TANH
# (what, block arguments, route) - default knobs; pairs sit on both sides of one rule
BOUNDARIES = [
    ("<= 4 output channels from 32 / 64 inputs on whole 8 x 32 patches", dict(n=1, h=8, w=32, cin_p=32, cout=3), "conv3x3_thinco"),
    ("... five channels: the register-staged igemm", dict(n=1, h=8, w=32, cin_p=32, cout=5), "conv_igemm (register-staged)"),
    ("... 128 inputs", dict(n=1, h=8, w=32, cin_p=128, cout=3), "conv_igemm (register-staged)"),
    ("8-channel input on 16 x 32 patches", dict(n=1, h=16, w=32, cin_p=8, cout=16), "conv3x3_cin8"),
    ("... on 8 rows, 64 channels: the halo kernel", dict(n=1, h=8, w=32, cin_p=8, cout=64), "conv3x3_halo<16bit>"),
    ("1x1: K of 4 - 24 steps and few blocks splits over the waves", dict(n=1, h=4, w=4, cin_p=128, cout=3, ksize=1), "conv1x1_splitk"),
    ("... three K-steps", dict(n=1, h=4, w=4, cin_p=96, cout=3, ksize=1), "conv1x1_direct"),
    ("... 320 blocks of 32 px x 64 co", dict(n=5, h=64, w=32, cin_p=128, cout=64, ksize=1), "conv1x1_splitk"),
    ("... 640 blocks", dict(n=5, h=64, w=32, cin_p=128, cout=65, ksize=1), "conv1x1_direct"),
    ("... 1024 input channels: 32 steps", dict(n=1, h=8, w=8, cin_p=1024, cout=64, ksize=1), "conv1x1_direct"),
    ("... 1032: past the direct kernel's weight tile", dict(n=1, h=8, w=8, cin_p=1032, cout=64, ksize=1), "conv1x1_splitk"),
    ("... 1032 on a big map", dict(n=20, h=32, w=32, cin_p=1032, cout=64, ksize=1), "conv_igemm (register-staged)"),
    ("17 - 64 channels on 16 x 32 patches: the 64-channel ping-pong form", dict(n=1, h=16, w=32, cin_p=32, cout=64), "conv3x3_pp<16bit,1,FAST>"),
    ("... with tanh: its general epilogue", dict(n=1, h=16, w=32, cin_p=32, cout=64, act=TANH), "conv3x3_pp<16bit,1>"),
    ("... 8 rows: cout 64 stays on the halo kernel", dict(n=1, h=8, w=32, cin_p=32, cout=64), "conv3x3_halo<16bit>"),
    ("... cout 80 on the same map: the 8-row ping-pong form", dict(n=1, h=8, w=32, cin_p=32, cout=80), "conv3x3_pp<16bit,2,FAST>"),
    ("... its general epilogue", dict(n=1, h=8, w=32, cin_p=32, cout=80, act=TANH), "conv3x3_pp<16bit,2>"),
    ("... a pitch that is no multiple of 8", dict(n=1, h=8, w=32, cin_p=32, cout=80, ldy=84), "conv3x3_pp<16bit,2>"),
    ("thin output on a big map below the thinco kernel's reach", dict(n=4, h=256, w=256, cin_p=32, cout=8), "conv3x3_tall<16bit,1,16>"),
    ("256 16-row items = two exact rounds of 8-row items, K of three chunks", dict(n=8, h=64, w=64, cin_p=96, cout=512), "conv3x3_ppw<16bit> (64 co x 4 rows per wave)"),
    ("... K of two chunks: priced at 2.04 items", dict(n=8, h=64, w=64, cin_p=64, cout=512), "conv3x3_pp<16bit,2,FAST>"),
    ("... with tanh the lockstep 16-row kernel keeps the layer", dict(n=8, h=64, w=64, cin_p=96, cout=512, act=TANH), "conv3x3_tall<16bit,2,16>"),
    ("16-wide maps: 64 items of 128 co x 16 x 16 px", dict(n=32, h=16, w=16, cin_p=8, cout=256), "conv3x3_pp<16bit,2,FAST,w16>"),
    ("... 62 items", dict(n=31, h=16, w=16, cin_p=8, cout=256), "conv_igemm_dma"),
    ("small maps: the LDS-DMA igemm, 9 K-steps do not split", dict(n=1, h=4, w=4, cin_p=64, cout=32), "conv_igemm_dma"),
    ("... 18 K-steps do", dict(n=1, h=4, w=4, cin_p=128, cout=32), "conv_igemm_dma+finalize (split-K)"),
    ("... not without the scratch", dict(n=1, h=4, w=4, cin_p=128, cout=32, lend=False), "conv_igemm_dma"),
    ("... 16 output channels", dict(n=1, h=4, w=4, cin_p=128, cout=16), "conv_igemm (register-staged)"),
    ("... 8192 pixels", dict(n=32, h=16, w=16, cin_p=64, cout=128), "conv_igemm_dma"),
    ("... 8448 pixels", dict(n=33, h=16, w=16, cin_p=64, cout=128), "conv_igemm (register-staged)"),
    ("fp32: the tall kernel on 16 rows", dict(n=1, h=16, w=32, cin_p=8, cout=64, dtype=F32), "conv3x3_tall<f32,1,16>"),
    ("... 8 rows", dict(n=1, h=8, w=32, cin_p=8, cout=64, dtype=F32), "conv3x3_halo<f32>"),
    ("... cout 80 on 8 rows", dict(n=1, h=8, w=32, cin_p=8, cout=80, dtype=F32), "conv3x3_tall<f32,2,8>"),
    ("... 16-row items where they save rounds: 256 against 512", dict(n=8, h=64, w=64, cin_p=8, cout=512, dtype=F32), "conv3x3_tall<f32,2,16>"),
    ("... 1x1", dict(n=1, h=4, w=4, cin_p=128, cout=64, ksize=1, dtype=F32), "conv_igemm (register-staged)"),
    ("... small 3x3", dict(n=1, h=4, w=4, cin_p=8, cout=32, dtype=F32), "conv_igemm_dma"),
    ("... 16 K-steps split", dict(n=1, h=4, w=4, cin_p=64, cout=32, dtype=F32), "conv_igemm_dma+finalize (split-K)"),
]


@pytest.mark.parametrize("what,args,want", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_route_boundaries(what, args, want):
    assert L.conv_route(block(**args)) == want


def test_every_route_of_the_default_knobs_is_pinned():
    """23 names: every string conv_route_name() can return except the forced-only ones (halo / tall<16bit,2,8> behind SP_TUNE_*) and fp8."""
    pinned = {(a.get("dtype", BF16) == F32, want) for _, a, want in BOUNDARIES}
    assert len(pinned) == 23, sorted(pinned)


UNSUPPORTED = [
    ("the fused tail with cout != 64", dict(n=1, h=16, w=32, cin_p=32, cout=48, tail_w=PTR, tail_y=PTR, tail_cout=3, tail_ld=3),
     "sp_conv2d_igemm: the fused 1x1 tail needs 16-bit storage, a 3x3 layer with cout == 64, h % 16 == 0, w % 32 == 0, ldy % 8 == 0, no pooling"),
    ("pool_idx above 1 GiB", dict(n=64, h=256, w=256, cin_p=128, cout=128, pool2=2, act=L.ACT_RELU, pool_idx=PTR),
     "sp_conv2d_igemm: pool_idx needs operands below 1 GiB (n*h*w*cin_p, cout*9*cin_p)"),
    ("fp8 on cout <= 64", dict(n=1, h=16, w=32, cin_p=32, cout=64, dtype=F8, x_scale=PTR, w_scale=PTR),
     "sp_conv2d_igemm: SP_F8 covers 3x3 layers with cout > 64, h % 8 == 0, w % 32 == 0 only"),
]


@pytest.mark.parametrize("what,args,message", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_unsupported_blocks_say_why(what, args, message):
    out = ctypes.c_char_p()
    assert L.lib().sp_conv2d_route(ctypes.byref(block(**args)), ctypes.byref(out)) == -3          # SP_ERR_UNSUPPORTED
    assert L.lib().sp_last_error_string().decode() == message
    # ... and the same blocks on the supported side of the rule
    ok = dict(args)
    ok.update({"the fused tail with cout != 64": dict(cout=64), "pool_idx above 1 GiB": dict(n=8), "fp8 on cout <= 64": dict(cout=80)}[what])
    assert L.conv_route(block(**ok)) in ("conv3x3_pp<16bit,1,FAST>", "conv3x3_pp<16bit,2>", "conv3x3_pp<f8,2>")


def test_split_k_suffix_goes_with_the_workspace():
    """Over the boundary table: the igemm's name carries the split-K suffix exactly when sp_conv2d_workspace reports bytes for the layer
    and the block lends them; and the query reports nothing for what ops._conv_launch used to leave unasked (1x1, big fp32 maps)."""
    igemm = 0
    for _, a, _ in BOUNDARIES:
        a = dict(a)
        a.pop("lend", None)
        dtype = a.get("dtype", BF16)
        ws = ops.conv_workspace_bytes(a["n"], a["h"], a["w"], a["cin_p"], a["cout"], a.get("ksize", 3), TORCH[dtype])
        if a.get("ksize", 3) == 1 or (dtype == F32 and a["n"] * a["h"] * a["w"] > 8192):
            assert ws == 0, a
        for lend in (True, False):
            r = L.conv_route(block(lend=lend, **a))
            if r.startswith("conv_igemm_dma"):
                igemm += 1
                assert r.endswith("+finalize (split-K)") == (ws > 0 and lend), (a, lend, ws, r)
            else:
                assert "split-K" not in r
    assert igemm >= 12, igemm
