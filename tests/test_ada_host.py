"""Host side of the adaptive augmentation (csrc/augment.hip: the gate and its controller; DESIGN.md section 15;
tests/test_gpu_augment_gate.py, tests/test_gpu_ada_controller.py and tests/test_gpu_ada_step.py have the GPU side): the restated
controller and gate of tests/ada_restated.py against the definition, value by value, and what the library and the host refuse without
touching a device.  Everything here is exact: the controller's arithmetic is integer counts, one fp32 division and one fp32 addition."""
import ctypes

import numpy as np
import pytest
import torch

import ada_restated as R
import augment_restated as A
from semantic_pyramid_for_image_generation_amd import _lib, ops
from semantic_pyramid_for_image_generation_amd.config import CFG, Config

F = np.float32
QUARTER = F(0.25)


def test_controller_moves_by_exactly_one_step_and_clamps_at_both_ends():
    c = R.Controller(0.0)
    seen = []
    for _ in range(6):
        c.observe([1.0, 1.0, 0.0], 0.5)               # r = 1 / 3 > target
        c.adjust(1, 0.0, QUARTER)
        seen.append(float(c.p))
    assert seen == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]   # exact: multiples of 2^-2; the clamp at 1 holds
    assert c.r_last == F(F(1) / F(3)) and c.adjustments == 6
    for want in (0.75, 0.5, 0.25, 0.0, 0.0):
        c.observe([0.0, 0.0, 1.0], 0.5)               # r = -1 / 3 < target
        c.adjust(1, 0.0, QUARTER)
        assert float(c.p) == want                     # ... and the clamp at 0
    # a step that is no power of two: p is the fp32 sum, rounded once
    c = R.Controller(0.1)
    step = F(0.3)
    c.observe([1.0], 0.5)
    c.adjust(1, 0.0, step)
    assert c.p == F(F(0.1) + step)
    # a step beyond the room that is left lands ON the bound
    c = R.Controller(0.9)
    c.observe([1.0], 0.5)
    c.adjust(1, 0.0, F(0.3))
    assert c.p == F(1.0)


def test_controller_holds_p_where_r_is_exactly_the_target():
    c = R.Controller(0.5)
    c.observe([1.0, 1.0, 1.0, 0.0], 0.5)              # r = 2 / 4, exactly
    c.adjust(1, 0.5, QUARTER)
    assert c.p == F(0.5) and c.r_last == F(0.5) and c.adjustments == 1
    assert (c.pos, c.neg, c.total, c.steps) == (0, 0, 0, 0)


def test_controller_waits_for_a_full_window_and_ignores_an_empty_one():
    c = R.Controller(0.5)
    for i in range(2):
        c.observe([1.0, 1.0], 0.5)
        c.adjust(3, 0.0, QUARTER)
        assert c.p == F(0.5) and c.steps == i + 1 and c.total == 2 * (i + 1) and c.adjustments == 0
    c.observe([1.0, 0.0], 0.5)
    c.adjust(3, 0.0, QUARTER)                         # third step: r = (5 - 1) / 6
    assert c.p == F(0.75) and c.r_last == F(F(4) / F(6)) and c.adjustments == 1
    assert (c.pos, c.neg, c.total, c.steps) == (0, 0, 0, 0)
    before = c.words()
    c.adjust(1, 0.0, QUARTER)                         # a full window without an observation: only the step count starts again
    assert c.words() == before
    c.adjust(2, 0.0, QUARTER)
    assert c.steps == 1
    c.adjust(2, 0.0, QUARTER)
    assert c.steps == 0 and c.p == F(0.75) and c.adjustments == 1


def test_values_at_the_threshold_and_nan_count_in_the_total_only():
    t = F(0.5)
    above, below = np.nextafter(t, F(1)), np.nextafter(t, F(0))
    c = R.Controller()
    c.observe([t, above, below, np.nan, np.inf, -np.inf, t, np.nan], t)
    assert (c.pos, c.neg, c.total) == (2, 2, 8)
    c = R.Controller()
    c.observe([np.nan, t], t)
    c.adjust(1, 0.0, QUARTER)                          # r = 0 / 2 == target 0: p stays
    assert c.p == F(0) and c.r_last == F(0) and c.adjustments == 1


def test_the_gate_is_a_strict_fp32_compare():
    half = F(0.5)
    last = np.nextafter(F(1), F(0))                   # the largest uniform in [0, 1)
    u = torch.zeros(6, 8)
    u[:, 7] = torch.tensor([0.0, 0.25, float(np.nextafter(half, F(0))), 0.5, 0.75, float(last)])
    assert R.live(u, 0.5).tolist() == [True, True, True, False, False, False]       # u7 == p is dead
    assert R.live(u, 0.0).tolist() == [False] * 6                                   # p = 0: nobody, not even u7 = 0
    assert R.live(u, 1.0).tolist() == [True] * 6                                    # p = 1: everybody
    assert R.live(u, float("nan")).tolist() == [False] * 6
    # composed: the live images are augment_restated's, the dead ones pass as they are, forward and backward
    x = A.exact_operands((6, 3, 16, 24), 3)
    u[:, :7] = torch.rand(6, 7, generator=torch.Generator().manual_seed(4))
    for fn, plain in ((R.forward, A.forward), (R.backward, A.backward)):
        got = fn(x, u, 0.5, 7)
        assert torch.equal(got[:3], plain(x[:3], u[:3], 7)) and torch.equal(got[3:], x[3:].double())
        assert torch.equal(fn(x, u, 1.0, 7), plain(x, u, 7)) and torch.equal(fn(x, u, 0.0, 7), x.double())
    xr = x.clone().requires_grad_(True)
    dy = A.exact_operands((6, 3, 16, 24), 5)
    (R.forward(xr, u, 0.5, 7) * dy).sum().backward()
    assert torch.allclose(xr.grad.double(), R.backward(dy, u, 0.5, 7), rtol=0, atol=1e-5)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert protos["sp_augment_ingest_gated"][1] == [p, i32, i64, i64, i64, i64, p, i32, i32, i32, i32, p, i32, p, p, i32, p]
    assert protos["sp_augment_ingest_bwd_gated"][1] == [p, i32, p, i32, i32, i32, p, i32, p, p, i32, p]
    assert protos["sp_ada_observe"][1] == [p, i64, f32, p, p]
    assert protos["sp_ada_adjust"][1] == [p, i32, f32, f32, p]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sp_augment_ingest_gated", "sp_augment_ingest_bwd_gated", "sp_ada_observe", "sp_ada_adjust"):
        assert hasattr(handle, name), name


def test_refused_arguments_launch_nothing():
    """Every refusal happens in front of the launch (SP_ERR_INVALID and a message that names the entry point): callable without a GPU."""
    lib = _lib.lib()
    b = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(256)))
    # a NULL p_dev is refused; so is everything the ungated entries refuse
    assert lib.sp_augment_ingest_gated(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 7, b, None, 0, None) != 0
    assert b"sp_augment_ingest_gated" in lib.sp_last_error_string() and b"p_dev" in lib.sp_last_error_string()
    assert lib.sp_augment_ingest_bwd_gated(b, 4, b, 1, 4, 4, b, 7, b, None, 0, None) != 0
    assert b"sp_augment_ingest_bwd_gated" in lib.sp_last_error_string() and b"p_dev" in lib.sp_last_error_string()
    assert lib.sp_augment_ingest_gated(None, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 7, b, b, 0, None) != 0
    assert lib.sp_augment_ingest_gated(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 8, b, b, 0, None) != 0        # policy out of range
    assert lib.sp_augment_ingest_gated(b, 0, 48, 16, 4, 1, b, 1, 4, 4, 4, b, 1, None, b, 0, None) != 0     # color without partials
    assert lib.sp_augment_ingest_bwd_gated(b, 4, b, 1, 4, 4, None, 6, None, b, 0, None) != 0               # no u
    assert lib.sp_augment_ingest_bwd_gated(b, 2, b, 1, 4, 4, b, 6, None, b, 0, None) != 0                  # pitch below 3 channels
    for numel in (0, -1, (1 << 24) + 1):
        assert lib.sp_ada_observe(b, numel, 0.5, b, None) != 0
        assert b"sp_ada_observe" in lib.sp_last_error_string()
    assert lib.sp_ada_observe(None, 4, 0.5, b, None) != 0 and lib.sp_ada_observe(b, 4, 0.5, None, None) != 0
    nan = float("nan")
    for interval, target, step in ((0, 0.0, 0.25), (-3, 0.0, 0.25), (1, 1.5, 0.25), (1, -1.5, 0.25), (1, nan, 0.25), (1, 0.0, -0.25),
                                   (1, 0.0, 1.5), (1, 0.0, nan)):
        assert lib.sp_ada_adjust(b, interval, target, step, None) != 0, (interval, target, step)
        assert b"sp_ada_adjust" in lib.sp_last_error_string()
    assert lib.sp_ada_adjust(None, 1, 0.0, 0.25, None) != 0


def test_host_settings():
    assert Config().augment_p == "" and isinstance(CFG.augment_p, str)
    with pytest.raises(_lib.SempyrError):
        ops._augment_gate(0.5, torch.device("cpu"))                      # a Python number is no device value
    with pytest.raises(_lib.SempyrError):
        ops._augment_gate(torch.tensor([0.5]), torch.device("cpu"))      # nor is a host tensor
    assert ops._augment_gate(None, torch.device("cpu")) is None
    for bad in ({"p": 1.5}, {"p": -0.1}, {"target": 2.0}, {"interval": 0}, {"interval": 1.5}, {"speed_images": 0}, {"threshold": float("nan")}):
        with pytest.raises(_lib.SempyrError):
            ops.AdaptiveAugment("cpu", **bad)
