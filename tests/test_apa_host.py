"""Host side of adaptive pseudo augmentation (csrc/apa.hip: sp_apa_select; ops.apa_select; ModelWrapper(apa=...), SP_APA; DESIGN.md section
22; tests/test_gpu_apa.py and tests/test_gpu_apa_step.py have the GPU side): the torch restatement of tests/apa_restated.py against the
definition value by value, every accepted and every malformed SP_APA value, every refusal of the C entry in front of its launch, and
the wrapper's constructor and draw errors.  Nothing here needs a GPU; everything is exact."""
import ctypes

import numpy as np
import pytest
import torch

import apa_restated as R
import semantic_pyramid_for_image_generation_amd as sp
from semantic_pyramid_for_image_generation_amd import _lib, config, ops

F = np.float32


def test_selection_is_a_strict_fp32_compare_and_an_exact_copy():
    half = F(0.5)
    last = np.nextafter(F(1), F(0))                   # the largest uniform in [0, 1)
    w = torch.tensor([0.0, 0.25, float(np.nextafter(half, F(0))), 0.5, 0.75, float(last)])
    assert R.taken(w, 0.5).tolist() == [True, True, True, False, False, False]       # w == p is not taken
    assert R.taken(w, 0.0).tolist() == [False] * 6                                   # p = 0: nobody, not even w = 0
    assert R.taken(w, 1.0).tolist() == [True] * 6                                    # p = 1: everybody
    assert R.taken(w, float("nan")).tolist() == [False] * 6
    # the compare is made in fp32: a p that rounds to 0.5 takes what 0.5 takes
    assert R.taken(w, 0.5 + 2.0 ** -30).tolist() == R.taken(w, 0.5).tolist()
    s = R.straddling(6, 0.5)
    assert s[1].item() == 0.5 and s[2].item() == float(np.nextafter(half, F(0))) and R.taken(s, 0.5).tolist() == [True, False, True, False, True, False]
    real, fake = R.values((6, 3, 3, 5), 1), R.values((6, 3, 3, 5), 2)
    got = R.select(real, fake, w, 0.5)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got[:3], fake[:3]) and torch.equal(got[3:], real[3:]) and not torch.equal(fake, real)
    assert torch.equal(R.select(real, fake, w, 0.0), real) and torch.equal(R.select(real, fake, w, 1.0), fake)
    for dtype in (torch.bfloat16, torch.float16):     # the widening is exact: the 16-bit source's own values arrive
        f16 = torch.randn(6, 3, 3, 5, generator=torch.Generator().manual_seed(3)).to(dtype)
        got = R.select(real, f16, w, 1.0)
        assert torch.equal(got.to(dtype), f16) and torch.equal(got.double(), f16.double())


def test_selection_passes_nan_payloads_infinities_and_the_sign_of_zero():
    words = torch.tensor([0x7FC00000, 0x7FC12345, -0x3FEDCB, 0x7F800000, -0x800000, -0x80000000, 1, 0], dtype=torch.int32)   # NaNs, +-inf, -0, a denormal
    real = R.values((2, 3, 2, 4), 4)
    fake = R.values((2, 3, 2, 4), 5)
    real[0, 0].view(-1).copy_(words.view(torch.float32))
    fake[1, 2].view(-1).copy_(words.view(torch.float32))
    w = torch.tensor([0.75, 0.25])
    got = R.select(real, fake, w, 0.5)
    assert torch.equal(R.bits(got[0, 0]).view(-1), words) and torch.equal(R.bits(got[1, 2]).view(-1), words)
    assert torch.equal(R.bits(got[0]), R.bits(real[0])) and torch.equal(R.bits(got[1]), R.bits(fake[1]))


def test_source_variants_hold_the_values_in_the_layouts_they_name():
    x = R.values((5, 3, 8, 24), 6)
    for kind in R.REAL_KINDS:
        v = R.real_variant(x, kind)
        assert torch.equal(v, x) and tuple(v.shape) == tuple(x.shape)
    assert R.real_variant(x, "nchw").stride() == (3 * 8 * 24, 8 * 24, 24, 1)
    assert R.real_variant(x, "channels_last").stride() == (3 * 8 * 24, 1, 3 * 24, 3)
    sl = R.real_variant(x, "slice")
    assert sl.stride() == (3 * 10 * 27, 10 * 27, 27, 1) and sl.storage_offset() % 4 != 0 and not sl.is_contiguous()
    for dtype, cp in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float16, 8)):
        v = R.fake_variant(x, dtype)
        assert v.dtype == dtype and torch.equal(v.float(), x) and v.stride() == (8 * 24 * cp, 1, 24 * cp, cp)


def test_config_parses_every_accepted_value_and_refuses_the_rest(monkeypatch):
    P = config.parse_apa
    for off in (None, "", "   "):
        assert P(off) is None
    assert P(0) == ("fixed", 0.0) and P(1) == ("fixed", 1.0) and P(0.25) == ("fixed", 0.25) and P("0.25") == ("fixed", 0.25) and P(" 1 ") == ("fixed", 1.0)
    assert P("adaptive") == ("adaptive", 0.6) and P("adaptive:0.3") == ("adaptive", 0.3) and P(" adaptive:-1 ") == ("adaptive", -1.0)
    for bad in ("sometimes", "1.5", 1.5, -0.25, "-0.25", "nan", float("nan"), True, False, "adaptive:", "adaptive:2", "adaptive:x", "adaptive0.3",
                "adaptive:nan", [0.5], "0.5:4"):
        with pytest.raises(ValueError):
            P(bad)
    assert config.Config().apa == "" and isinstance(config.CFG.apa, str)
    for text, want in (("", ""), (" adaptive:0.3 ", "adaptive:0.3"), ("0.5", "0.5"), ("adaptive", "adaptive")):
        monkeypatch.setenv("SP_APA", text)
        assert config.Config.from_env().apa == want
    for bad in ("sometimes", "1.5", "adaptive:2"):       # a malformed value fails where the configuration is read: at import
        monkeypatch.setenv("SP_APA", bad)
        with pytest.raises(ValueError):
            config.Config.from_env()
    monkeypatch.delenv("SP_APA")
    assert config.Config.from_env().apa == ""


def test_header_declares_the_entry_point_and_the_library_exports_it():
    protos = _lib.parse_header()
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert protos["sp_apa_select"] == (ctypes.c_int, [p, i32, i64, i64, i64, i64, p, i32, i64, i64, i64, i64, p, i32, i32, i32, p, p, i32, p])
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sp_apa_select", "sp_apa_select__b16", "sp_apa_select__h16"):
        assert hasattr(handle, name), name


def _call(lib, **kw):
    """sp_apa_select on host buffers with one argument changed; every such call must be refused in front of the launch."""
    b = kw.pop("buf")
    a = dict(real=b, real_dtype=0, rs=(48, 16, 4, 1), fake=b, fake_dtype=0, fs=(48, 16, 4, 1), dst=b, n=1, h=4, w=4, w_u=b, p_dev=b, dtype=0)
    a.update(kw)
    return lib.sp_apa_select(a["real"], a["real_dtype"], *a["rs"], a["fake"], a["fake_dtype"], *a["fs"], a["dst"], a["n"], a["h"], a["w"],
                             a["w_u"], a["p_dev"], a["dtype"], None)


def test_refused_arguments_launch_nothing():
    """Every refusal happens in front of the launch, with a message that names the entry point: callable without a GPU (a launch on
    this machine would fail with SP_ERR_LAUNCH, -2, which no case below returns)."""
    lib = _lib.lib()
    hold = ctypes.create_string_buffer(256)
    b = ctypes.c_void_p(ctypes.addressof(hold))
    INVALID, UNSUPPORTED = -1, -3
    for name in ("real", "fake", "dst", "w_u", "p_dev"):
        assert _call(lib, buf=b, **{name: None}) == INVALID, name
        assert b"sp_apa_select" in lib.sp_last_error_string() and b"NULL" in lib.sp_last_error_string()
    for name in ("n", "h", "w"):
        for value in (0, -1):
            assert _call(lib, buf=b, **{name: value}) == INVALID, (name, value)
            assert b"sp_apa_select" in lib.sp_last_error_string()
    assert _call(lib, buf=b, n=65536) == INVALID and _call(lib, buf=b, h=1 << 15, w=(1 << 13) + 1) == INVALID
    for name in ("dtype", "real_dtype", "fake_dtype"):
        for value in (-1, 2, 4, 5, 99):                  # SP_F8 and SP_F8_F16 included: the kernel has no fp8 form
            assert _call(lib, buf=b, **{name: value}) == INVALID, (name, value)
            assert b"sp_apa_select" in lib.sp_last_error_string() and b"dtype" in lib.sp_last_error_string()
    assert _call(lib, buf=b, rs=(48, 16, -4, 1)) == INVALID and _call(lib, buf=b, fs=(-48, 16, 4, 1)) == INVALID
    # the two 16-bit types never mix (SP_F32 0, SP_BF16 1, SP_F16 3): sp_ingest_image's rule, for either source
    SP_F32, SP_BF16, SP_F16 = _lib.SP_F32, _lib.SP_BF16, _lib.SP_F16
    for src in ("real_dtype", "fake_dtype"):
        assert _call(lib, buf=b, dtype=SP_F16, **{src: SP_BF16}) == UNSUPPORTED, src
        assert b"sp_apa_select" in lib.sp_last_error_string() and b"SP_BF16" in lib.sp_last_error_string()
        for storage in (SP_BF16, SP_F32):
            assert _call(lib, buf=b, dtype=storage, **{src: SP_F16}) == UNSUPPORTED, (src, storage)
            assert b"sp_apa_select" in lib.sp_last_error_string() and b"SP_F16" in lib.sp_last_error_string()
    assert _call(lib, buf=b, dtype=SP_F16, real_dtype=SP_F16, fake_dtype=SP_BF16) == UNSUPPORTED
    assert _call(lib, buf=b, dtype=SP_BF16, real_dtype=SP_BF16, fake_dtype=SP_F16) == UNSUPPORTED


def test_the_op_checks_its_arguments_on_the_host():
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(_lib.SempyrError):
        ops.apa_select(x, x, torch.zeros(2), torch.zeros(1))          # host tensors: the op runs on the GPU only
    assert callable(ops.apa_select)
    # the 16-bit mix is refused by the same check the ingest makes, tensor by tensor
    with pytest.raises(_lib.SempyrError):
        ops._ingest_src_dtype(torch.zeros(1, dtype=torch.float16), torch.bfloat16)
    with pytest.raises(_lib.SempyrError):
        ops._ingest_src_dtype(torch.zeros(1, dtype=torch.bfloat16), torch.float16)


def _wrapper(D=None, **kw):
    G = torch.nn.Linear(2, 2)
    G.latent_dimensions = 2
    return sp.ModelWrapper(G, D if D is not None else sp.Discriminator(channel_factor=16), None, None, vgg16=torch.nn.Identity(),
                           save_data_path=None, **kw)


def test_wrapper_off_by_default_and_its_errors(monkeypatch):
    assert config.CFG.apa == "", "this test needs SP_APA unset"
    x = torch.zeros(2, 3, 4, 4)
    for off in ({}, {"apa": None}, {"apa": ""}):
        mw = _wrapper(**off)
        assert mw._apa is None and "apa" not in mw.logger.hyperparameter and not mw._apa_adaptive()
        assert mw._apa_rows(x, None) is None and mw._with_apa({"a": 1}) == {"a": 1}
        with pytest.raises(_lib.SempyrError):                    # uniforms for a wrapper without APA
            mw._apa_rows(x, torch.zeros(2))
        with pytest.raises(_lib.SempyrError):
            mw.train_step(x, torch.zeros(2, 4), [], apa_w=torch.zeros(2))
        with pytest.raises(_lib.SempyrError):
            mw.load_apa_state({"state": torch.zeros(8, dtype=torch.int32)})
    for bad in ("sometimes", 1.5, -0.25, True, "adaptive:2", "adaptive:", [0.5]):
        with pytest.raises(_lib.SempyrError):
            _wrapper(apa=bad)
    for spec in (0.5, "0.5", "adaptive", "adaptive:0.3"):        # the state lives on the discriminator's GPU: a CPU discriminator has none
        with pytest.raises(_lib.SempyrError):
            _wrapper(apa=spec)
    monkeypatch.setattr(config.CFG, "apa", "adaptive")           # the environment's way in (main.py passes fixed keywords)
    with pytest.raises(_lib.SempyrError):
        _wrapper()
    assert _wrapper(apa="")._apa is None                         # ... which the keyword overrides


def test_wrapper_takes_a_controller_without_augment_and_with_a_foreign_discriminator():
    """APA sits in front of whatever module D is and needs no augment: an ops.AdaptiveAugment instance (on the host here) is taken as it
    is, fixed or adaptive, beside an augment_p controller of its own."""
    x = torch.zeros(2, 3, 4, 4)
    fixed = ops.AdaptiveAugment("cpu", p=0.5, adaptive=False)
    foreign = torch.nn.Linear(2, 2)
    mw = _wrapper(D=foreign, apa=fixed)
    assert mw._apa is fixed and not mw._apa_adaptive() and mw._ada is None and mw._aug_policy == 0
    assert "'p': 0.5" in mw.logger.hyperparameter["apa"]
    assert mw._with_apa({"a": 1}) == {"a": 1}                     # a fixed p: no new result
    w = mw._apa_rows(x, None)
    assert tuple(w.shape) == (2,) and w.dtype == torch.float32 and bool(((w >= 0) & (w < 1)).all())
    given = torch.tensor([0.25, 0.75], dtype=torch.float64)
    assert torch.equal(mw._apa_rows(x, given), given.float()) and mw._apa_rows(x, given).dtype == torch.float32
    for wrong in (torch.zeros(3), torch.zeros(2, 1), torch.zeros(1, 2)):
        with pytest.raises(_lib.SempyrError):
            mw._apa_rows(x, wrong)
    with pytest.raises(_lib.SempyrError):                         # a fixed p has no controller state to restore
        mw.load_apa_state({"state": torch.zeros(8, dtype=torch.int32)})
    steered = ops.AdaptiveAugment("cpu", target=0.3, interval=2, speed_images=64)
    ada = ops.AdaptiveAugment("cpu", target=0.7)
    mw = _wrapper(apa=steered, augment="color", augment_p=ada)
    assert mw._apa is steered and mw._ada is ada and mw._apa.state.data_ptr() != mw._ada.state.data_ptr()
    assert "0.3" in mw.logger.hyperparameter["apa"] and "0.7" in mw.logger.hyperparameter["augment_p"]
    out = mw._with_apa(mw._with_augment_p({"a": 1}))
    assert set(out) == {"a", "apa_p", "apa_rt", "augment_p", "augment_rt"} and out["apa_p"].shape == ()
    sd = steered.state_dict()
    sd["state"] = torch.tensor([0x3E800000, 0, 3, 1, 4, 1, 2, 0], dtype=torch.int32)
    mw.load_apa_state({"apa_state": sd})
    assert float(mw._apa.p) == 0.25 and mw._apa.values()["adjustments"] == 2 and mw._ada.values()["p"] == 0.0
    with pytest.raises(_lib.SempyrError):
        mw.load_apa_state({"augment_state": sd})
