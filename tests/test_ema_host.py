"""Host side of the generator weight average (optim.ParameterEMA, sp_ema_multi / sp_swap_multi, ModelWrapper's generator_ema): ABI,
table layout, argument errors, rejections and the state dict - everything that needs no GPU (tests/test_gpu_ema.py has the rest)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, config, optim

CTYPE_OF = {"float*": "<u8", "int32_t": "<i4"}


def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    assert protos["sp_ema_multi"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert protos["sp_swap_multi"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "sp_ema_multi") and hasattr(handle, "sp_swap_multi")


def test_table_dtype_matches_the_header_struct():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct sp_ema_chunk \{(.*?)\}", text, flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            ty, name = decl.rsplit(" ", 1)
            fields.append((name, CTYPE_OF[ty.strip()]))
    assert [(n, optim._EMA_DT[n].str) for n in optim._EMA_DT.names] == fields
    assert [n for n, _ in fields] == ["avg", "p", "n", "reserved"]
    assert optim._EMA_DT.itemsize == 24 and [optim._EMA_DT.fields[n][1] for n in optim._EMA_DT.names] == [0, 8, 16, 20]


def test_argument_errors_return_before_any_launch():
    lib = _lib.lib()
    table = (ctypes.c_uint8 * 24)()                       # one (never dereferenced) chunk: the errors come first
    tp = ctypes.cast(table, ctypes.c_void_p)
    assert lib.sp_ema_multi(None, 1, 0.5, None, None) != 0
    assert b"sp_ema_multi" in lib.sp_last_error_string()
    assert lib.sp_ema_multi(tp, 0, 0.5, None, None) != 0
    assert lib.sp_ema_multi(tp, -3, 0.5, None, None) != 0
    assert lib.sp_ema_multi(tp, 1, -0.1, None, None) != 0
    assert lib.sp_ema_multi(tp, 1, 1.5, None, None) != 0
    assert lib.sp_ema_multi(tp, 1, float("nan"), None, None) != 0
    assert lib.sp_swap_multi(None, 1, None) != 0
    assert b"sp_swap_multi" in lib.sp_last_error_string()
    assert lib.sp_swap_multi(tp, 0, None) != 0
    with pytest.raises(_lib.SempyrError):
        _lib.call("sp_ema_multi", None, 1, 0.5, None, None)


def test_cpu_module_is_rejected():
    with pytest.raises(_lib.SempyrError):
        optim.ParameterEMA(torch.nn.Linear(3, 2))
    with pytest.raises(_lib.SempyrError):
        optim.ParameterEMA(torch.nn.ReLU())               # no parameters at all


def _hand_filled(named_shapes, decay=0.75, warmup=True):
    """A ParameterEMA whose layout and (host) storage are filled by hand: what the constructor does after it has checked that the
    parameters are on a GPU.  The state-dict code reads and writes the windows only."""
    ema = optim.ParameterEMA.__new__(optim.ParameterEMA)
    ema._init_state(named_shapes, decay, warmup, "cpu")
    ema._params = []
    return ema


def test_layout_pads_every_window_to_four_floats():
    ema = _hand_filled([("a", (3,)), ("b", ()), ("c", (2, 4)), ("d", (5, 1))])
    assert ema._offsets == [0, 4, 8, 16] and ema.buffer.numel() == 24
    assert [tuple(w.shape) for w in ema._windows] == [(3,), (), (2, 4), (5, 1)]
    assert all(w.data_ptr() % 16 == ema.buffer.data_ptr() % 16 for w in ema._windows)


def test_state_dict_round_trip_and_mismatches():
    shapes = [("w", (3, 2)), ("b", (3,)), ("s", ())]
    src = _hand_filled(shapes)
    g = torch.Generator().manual_seed(5)
    for w in src._windows:
        w.copy_(torch.randn(w.shape, generator=g))
    src.num_updates = 17
    state = src.state_dict()
    assert set(state) == {"decay", "warmup", "num_updates", "parameters"}
    assert (state["decay"], state["warmup"], state["num_updates"]) == (0.75, True, 17)
    assert list(state["parameters"]) == ["w", "b", "s"]
    assert all(t.data_ptr() != w.data_ptr() for t, w in zip(state["parameters"].values(), src._windows))      # copies
    dst = _hand_filled(shapes, decay=0.5, warmup=False)
    dst.load_state_dict(state)
    assert (dst.decay, dst.warmup, dst.num_updates) == (0.75, True, 17)
    assert torch.equal(dst.buffer, src.buffer)
    # a missing name, another shape
    with pytest.raises(_lib.SempyrError):
        dst.load_state_dict(dict(state, parameters={k: v for k, v in state["parameters"].items() if k != "b"}))
    with pytest.raises(_lib.SempyrError):
        dst.load_state_dict(dict(state, parameters=dict(state["parameters"], b=torch.zeros(4))))
    with pytest.raises(_lib.SempyrError):
        dst.load_state_dict(dict(state, decay=1.5))
    assert torch.equal(dst.buffer, src.buffer)                                    # a rejected state changes nothing
    # swapped in: neither update nor load
    dst._swapped = True
    with pytest.raises(_lib.SempyrError):
        dst.update()
    with pytest.raises(_lib.SempyrError):
        dst.load_state_dict(state)
    with pytest.raises(_lib.SempyrError):
        with dst.applied():
            pass


def test_plain_generator_state_dict_is_accepted():
    G = sp.Generator(channels_factor=8)
    named = [(n, tuple(p.shape)) for n, p in G.named_parameters()]
    ema = _hand_filled(named, decay=0.999, warmup=False)
    sd = G.state_dict()
    assert len(sd) > len(named)                                                   # buffers (weight_u, running_mean ...) ride along
    ema.load_state_dict({"parameters": sd})
    assert (ema.decay, ema.warmup) == (0.999, False) and ema.num_updates == 1      # a loaded average counts as initialised
    for (n, p), w in zip(G.named_parameters(), ema._windows):
        assert torch.equal(w, p.detach()), n
    assert ema.buffer.numel() >= sum(p.numel() for p in G.parameters())
    sizes = [p.numel() for p in G.parameters()]
    # the shapes tests/test_gpu_ema.py relies on at this channel factor
    assert max(sizes) == 8388608 and min(sizes) == 1 and sum(1 for s in sizes if s % 4) >= 5


def test_config_parses_sp_g_ema(monkeypatch):
    monkeypatch.delenv("SP_G_EMA", raising=False)
    assert config.Config.from_env().g_ema == 0.0 and config.Config().g_ema == 0.0
    monkeypatch.setenv("SP_G_EMA", "0.999")
    assert config.Config.from_env().g_ema == 0.999
    monkeypatch.setenv("SP_G_EMA", "0")
    assert config.Config.from_env().g_ema == 0.0


def test_wrapper_without_the_switch_keeps_no_average(monkeypatch):
    assert config.CFG.g_ema == 0.0, "this test needs SP_G_EMA unset"
    G, D = sp.Generator(channels_factor=8), sp.Discriminator(channel_factor=8)
    mw = sp.ModelWrapper(G, D, None, None, save_data_path=None, generator_ema=None)
    assert mw.generator_ema is None
    assert "generator_ema" not in mw.logger.hyperparameter
    with pytest.raises(_lib.SempyrError):
        mw.load_generator_ema({"parameters": {}})
    with pytest.raises(_lib.SempyrError):                                          # a CPU generator cannot carry one
        sp.ModelWrapper(G, D, None, None, save_data_path=None, generator_ema=0.999)
