"""Adaptive pseudo augmentation inside the training step (ModelWrapper(apa=...), SP_APA; tests/test_gpu_apa.py
holds the kernel op by op): channel_factor 2, batch 2, fp32 parity mode unless a test says otherwise - the configuration of
tests/test_gpu_ada_step.py.
  * off: the wrapper built without the keyword - the device RNG stream is the two latent draws and nothing else, sp_apa_select is never
    called, the graphs hold no buffer of it, no result key (the checkpoint's keys with APA off are pinned by
    tests/test_gpu_ada_step.py::test_train_logs_p_and_r_and_saves_the_state, which lists them all);
  * fixed p = 0, latents and augmentation uniforms given: every result equals the APA-off wrapper's bit for bit;
  * fixed p = 1, with the generator's pair forward on and off: loss_discriminator_real is the real-label loss of a deep copy of D, taken
    before the step, on the pseudo source of that branch of the rule; the VGG-16 and the generator step keep the true real images;
  * p = 0.5 with apa_w given: exactly the rows with w < 0.5 are replaced, eager and in the replayed graphs' static buffer;
  * three replayed steps with fresh draws equal three eager steps bit for bit while an adaptive p moves, beside an augment_p controller
    that walks its own way;
  * APA with six augmentation words and augment_p="adaptive" in one step, in fp32, bf16 and fp16 storage;
  * "apa_state" round-trips into a wrapper whose graphs are already captured; train() logs apa_p / apa_rt and saves the state.
The thresholds of the adaptive cases are tests/test_gpu_ada_step.py's (its docstring): every prediction of the untrained discriminator
lies above -0.5, so a controller that counts around -0.5 with target -1 sees r > -1 and walks up by exactly one step per window."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_util as gu  # noqa: E402
import semantic_pyramid_for_image_generation_amd as sp  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import config, ops  # noqa: E402

CF, BATCH, SEED = 2, 2, 21
POLICY = "color,translation,cutout"
SIX_WORDS = "color,translation,cutout,xflip,rotate,brightness"
LOSS_NAMES = ("loss_discriminator_real", "loss_discriminator_fake", "loss_generator", "loss_generator_semantic_reconstruction",
              "loss_generator_diversity")
THRESHOLD_BELOW = -0.5


@pytest.fixture(autouse=True)
def _dtype_reset():
    yield
    ops.set_compute_dtype(torch.float32)


@pytest.fixture(scope="module")
def states():
    return gu.synth_states({"cf": CF, "seed": SEED})


@pytest.fixture(scope="module")
def batch():
    images, labels, masks = gu.golden_batches(BATCH, 6)[0]
    return images, labels, masks


def _wrapper(states, **kw):
    torch.cuda.set_device(0)
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF), sp.Discriminator(channel_factor=CF), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    G, D, V = G.cuda(), D.cuda(), V.cuda().eval()
    kw = {k: (v(D) if callable(v) else v) for k, v in kw.items()}
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=None, validation_dataset=None,
                         generator_optimizer=sp.optim.Adam(G.parameters(), lr=1e-5), discriminator_optimizer=sp.optim.Adam(D.parameters(), lr=1e-5),
                         save_data_path=None, **kw)
    G.train(); D.train()
    return mw


def _controller(speed, p=0.0, target=-1.0, interval=1, threshold=THRESHOLD_BELOW):
    return lambda D: ops.AdaptiveAugment(next(D.parameters()).device, p=p, target=target, interval=interval, speed_images=speed,
                                         threshold=threshold)


def _cuda(batch):
    images, labels, masks = batch
    return images.cuda(), labels.cuda(), [m.cuda() for m in masks]


def _record(out):
    rec = {k: out[k].detach().float().cpu().clone() for k in LOSS_NAMES}
    rec["pixels"] = out["images_fake"].detach().float().clone()
    for k in ("augment_p", "augment_rt", "apa_p", "apa_rt"):
        if k in out:
            rec[k] = float(out[k])
    rec["keys"] = sorted(out.keys())
    return rec


def _same(a, b, names=LOSS_NAMES):
    for k in names:
        assert torch.equal(a[k], b[k]), (k, a[k], b[k])
    assert torch.equal(a["pixels"], b["pixels"])


def _spy_calls(monkeypatch):
    names = []
    orig = L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(L, "call", call)
    return names


def _spy_select(monkeypatch):
    """Every ops.apa_select call of a step: clones of (real, fake as fp32, w_u, result) and the real argument's address."""
    seen = []
    orig = ops.apa_select

    def apa_select(real, fake, w_u, p, out=None):
        got = orig(real, fake, w_u, p, out=out)
        if torch.cuda.is_current_stream_capturing():       # (a capture only records the launch: nothing to look at yet)
            return got
        seen.append({"real": real.detach().clone(), "fake": fake.detach().float().clone(), "fake_dtype": fake.dtype, "w": w_u.clone(),
                     "out": got.clone(), "real_ptr": real.data_ptr(), "p": float(p)})
        return got
    monkeypatch.setattr(ops, "apa_select", apa_select)
    return seen


def _given(seed=12):
    gen = torch.Generator().manual_seed(seed)
    nd, ng = torch.randn(BATCH, 128, generator=gen), torch.randn(BATCH, 128, generator=gen)
    u = torch.rand(3, BATCH, 8, generator=gen)
    return nd.cuda(), ng.cuda(), u.cuda()


def test_off_nothing_of_apa_runs(states, batch, monkeypatch):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    names = _spy_calls(monkeypatch)
    runs = []
    for kw in ({}, {"apa": None}, {"apa": ""}):
        mw = _wrapper(states, **kw)
        assert mw._apa is None and "apa" not in mw.logger.hyperparameter
        assert not any(isinstance(v, torch.Tensor) for v in vars(mw).values())
        recs = []
        for i in range(2):
            torch.manual_seed(3 + i)
            recs.append(_record(mw.train_step(images, labels, masks, next_images_real=images)))
        torch.cuda.synchronize()
        rng = torch.cuda.get_rng_state().clone()
        torch.manual_seed(4)                                # the stream of a step: the two latent draws and nothing else
        torch.randn((BATCH, 128), device="cuda"); torch.randn((BATCH, 128), device="cuda")
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(), rng)
        with pytest.raises(L.SempyrError):
            mw.train_step(images, labels, masks, apa_w=torch.zeros(BATCH, device="cuda"))
        runs.append(recs)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a["keys"] == b["keys"] and "apa_p" not in a["keys"] and "apa_rt" not in a["keys"]
            _same(a, b)
    # the graphs hold no buffer of it, a replay draws what the eager step draws, and uniforms for it are an error there too
    mw.capture_graphs(images, labels, masks)
    st = mw._graph_state
    assert st["apa_w"] is None and st["apa_images"] is None
    torch.manual_seed(9)
    out = mw.train_step_graphed(images, labels, masks, next_images_real=images)
    torch.cuda.synchronize()
    rng = torch.cuda.get_rng_state().clone()
    assert "apa_p" not in out
    torch.manual_seed(9)
    torch.randn((BATCH, 128), device="cuda"); torch.randn((BATCH, 128), device="cuda")
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    with pytest.raises(L.SempyrError):
        mw.train_step_graphed(images, labels, masks, apa_w=torch.zeros(BATCH, device="cuda"))
    assert "sp_apa_select" not in names and len(names) > 100


def test_fixed_p_zero_equals_the_wrapper_without_apa_bit_for_bit(states, batch, monkeypatch):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    nd, ng, u = _given()
    names = _spy_calls(monkeypatch)
    recs = []
    for kw in ({}, {"apa": 0.0}, {"apa": "0"}):
        mw = _wrapper(states, augment=POLICY, **kw)
        steps = []
        for i in range(2):
            names.clear()
            extra = {"apa_w": torch.tensor([0.0, 0.5], device="cuda")} if kw else {}     # w = 0 is not below p = 0
            steps.append(_record(mw.train_step(images, labels, masks, noise_d=nd + i, noise_g=ng - i, augment_u=u, next_images_real=images, **extra)))
            assert names.count("sp_apa_select") == (1 if kw else 0)
        if kw:
            assert not mw._apa.adaptive and mw._apa.values()["p"] == 0.0 and "apa" in mw.logger.hyperparameter
            assert mw._apa.values()["total"] == 0 and mw._apa.values()["steps"] == 0        # a fixed p: never observed, never adjusted
        recs.append(steps)
    for other in recs[1:]:
        for a, b in zip(recs[0], other):
            assert a["keys"] == b["keys"]                       # a fixed p: no new result
            _same(a, b)


@pytest.mark.parametrize("g_pair", [True, False], ids=["pair_forward", "single_forwards"])
def test_fixed_p_one_shows_d_the_pseudo_source_under_the_real_label(states, batch, monkeypatch, g_pair):
    """Both branches of the source rule.  With the pair forward the pseudo source is the generator step's fake batch (the step's
    images_fake result: fresh latents); without it the D step's own fake batch, G(noise_d)."""
    ops.set_compute_dtype(torch.float32)
    monkeypatch.setattr(config.CFG, "g_pair", g_pair)
    images, labels, masks = _cuda(batch)
    nd, ng, _ = _given()
    off = _wrapper(states)
    assert off._g_pair_ok() == g_pair
    ref = _record(off.train_step(images, labels, masks, noise_d=nd, noise_g=ng))
    mw = _wrapper(states, apa=1.0)
    D = mw.discriminator
    d_before = copy.deepcopy(D)
    seen = _spy_select(monkeypatch)
    d_calls, v_inputs = [], []
    for fn_name in ("forward_pair", "forward"):
        def spy(*args, _orig=getattr(D, fn_name), _name=fn_name):
            d_calls.append((_name, [a.detach().clone() for a in args]))
            return _orig(*args)
        monkeypatch.setattr(D, fn_name, spy)
    v_forward = mw.vgg16.forward

    def v_spy(x, *a, **k):
        v_inputs.append(x.data_ptr())
        return v_forward(x, *a, **k)
    monkeypatch.setattr(mw.vgg16, "forward", v_spy)
    out = mw.train_step(images, labels, masks, noise_d=nd, noise_g=ng)
    got = _record(out)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0]["p"] == 1.0 and seen[0]["real_ptr"] == images.data_ptr()
    pseudo = seen[0]["fake"]
    assert torch.equal(seen[0]["out"], pseudo) and not torch.equal(pseudo, images)       # every row replaced
    if g_pair:
        assert torch.equal(pseudo, got["pixels"])                                          # the generator step's images: fresh latents
    else:
        assert not torch.equal(pseudo, got["pixels"])
        name, args = [c for c in d_calls if c[0] == "forward_pair"][0] if any(c[0] == "forward_pair" for c in d_calls) else d_calls[1]
        assert torch.equal(pseudo, args[1 if name == "forward_pair" else 0].float())      # D's own fake batch of this step
    # the discriminator phase's call on the copy taken before the step: the same entry, the same arguments
    name, args = d_calls[0]
    assert torch.equal(args[0], pseudo)                                                    # D's real branch saw the pseudo source
    res = getattr(d_before, name)(*args)
    if name == "forward_pair":
        pred_real, pred_fake = res
    else:
        pred_real, pred_fake = res, d_before(*d_calls[1][1])
    want_real, want_fake = mw.discriminator_loss(pred_real, pred_fake)
    print("loss_discriminator_real", float(got["loss_discriminator_real"]), float(want_real.detach()), "off", float(ref["loss_discriminator_real"]))
    assert torch.equal(got["loss_discriminator_real"], want_real.detach().float().cpu())
    assert torch.equal(got["loss_discriminator_fake"], want_fake.detach().float().cpu())
    assert not torch.equal(got["loss_discriminator_real"], ref["loss_discriminator_real"])
    # the VGG-16 saw the true real images (then the fake ones), and what does not read D is what it is with APA off
    assert v_inputs[0] == images.data_ptr() and len(v_inputs) == 2
    _same(got, ref, names=("loss_generator_semantic_reconstruction", "loss_generator_diversity", "loss_discriminator_fake"))


def test_p_half_replaces_exactly_the_rows_below_it_eager_and_replayed(states, batch, monkeypatch):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    nd, ng, _ = _given()
    mw = _wrapper(states, apa=0.5)
    seen = _spy_select(monkeypatch)
    w = torch.tensor([0.25, 0.75])
    out = mw.train_step(images, labels, masks, noise_d=nd, noise_g=ng, apa_w=w, next_images_real=images)       # (a host tensor is moved)
    s = seen[0]
    assert torch.equal(s["out"][0], s["fake"][0]) and torch.equal(s["out"][1], images[1]) and not torch.equal(s["out"][0], images[0])
    assert torch.equal(s["fake"], out["images_fake"].float()) and s["w"].tolist() == [0.25, 0.75]
    for wrong in (torch.zeros(BATCH + 1), torch.zeros(BATCH, 1)):
        with pytest.raises(L.SempyrError):
            mw.train_step(images, labels, masks, apa_w=wrong)
    mw.capture_graphs(images, labels, masks)
    st = mw._graph_state
    assert tuple(st["apa_w"].shape) == (BATCH,) and tuple(st["apa_images"].shape) == tuple(images.shape) and st["apa_images"].dtype == torch.float32
    for w, rows in ((torch.tensor([0.75, 0.25]), (False, True)), (torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0)))]), (False, True)),
                    (torch.tensor([0.0, 0.125]), (True, True)), (torch.tensor([0.5, 0.99]), (False, False))):
        out = mw.train_step_graphed(images, labels, masks, noise_d=nd, noise_g=ng, apa_w=w.cuda(), next_images_real=images)
        torch.cuda.synchronize()
        pseudo = out["images_fake"].float()                 # the pair forward made it: the generator step's fake batch (static)
        for i, taken in enumerate(rows):
            src, other = (pseudo, images) if taken else (images, pseudo)
            assert torch.equal(st["apa_images"][i], src[i]) and not torch.equal(st["apa_images"][i], other[i]), (w.tolist(), i)
    with pytest.raises(L.SempyrError):
        mw.train_step_graphed(images, labels, masks, apa_w=torch.zeros(BATCH + 1, device="cuda"))


def _steps(states, batch, graphed, apa=True):
    """Four steps from one seed per step: the first eager (a capture needs one eager step in front of it), then three that are replayed
    through the graphs captured behind it if `graphed`, eager otherwise.  APA's p walks by 0.25 per step, augment_p's by 0.125."""
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    kw = {"apa": _controller(4 * BATCH)} if apa else {}
    mw = _wrapper(states, augment=POLICY, augment_p=_controller(8 * BATCH), **kw)
    recs = []
    for i in range(4):
        if graphed and i == 1:
            mw.capture_graphs(images, labels, masks)
            ptrs, gd = (mw._apa.state.data_ptr(), mw._ada.state.data_ptr()), mw._graph_state["gd"]
        torch.manual_seed(100 + i)
        step = mw.train_step_graphed if graphed and i >= 1 else mw.train_step
        recs.append(_record(step(images, labels, masks, next_images_real=images)))      # (the results are views of the states: read now)
    if graphed:
        assert (mw._apa.state.data_ptr(), mw._ada.state.data_ptr()) == ptrs and mw._graph_state["gd"] is gd       # one capture served every p
    return recs, mw


def test_replayed_steps_equal_eager_steps_while_both_controllers_walk(states, batch):
    eager, mw_e = _steps(states, batch, graphed=False)
    assert [r["apa_p"] for r in eager] == [0.25, 0.5, 0.75, 1.0] and [r["augment_p"] for r in eager] == [0.125, 0.25, 0.375, 0.5]
    assert all(r["apa_rt"] > -1.0 and r["augment_rt"] > -1.0 for r in eager)
    assert {"apa_p", "apa_rt", "augment_p", "augment_rt"} <= set(eager[0]["keys"])
    replayed, mw_r = _steps(states, batch, graphed=True)
    for i, (a, b) in enumerate(zip(eager, replayed)):
        print("step", i, [(k, float(a[k]), float(b[k])) for k in LOSS_NAMES], [(k, a[k], b[k]) for k in ("apa_p", "apa_rt", "augment_p", "augment_rt")])
    for i, (a, b) in list(enumerate(zip(eager, replayed)))[1:]:
        _same(a, b)
        for k in ("apa_p", "apa_rt", "augment_p", "augment_rt"):
            assert a[k] == b[k], (i, k)
    # each controller counted B predictions per step in its own 8 words, and neither wrote the other's
    for mw in (mw_e, mw_r):
        va, vd = mw._apa.values(), mw._ada.values()
        assert (va["p"], va["adjustments"], va["steps"], va["total"]) == (1.0, 4, 0, 0) and (vd["p"], vd["adjustments"], vd["steps"], vd["total"]) == (0.5, 4, 0, 0)
        assert mw._apa.state.data_ptr() != mw._ada.state.data_ptr()
    assert mw_e._apa.state.cpu().tolist() == mw_r._apa.state.cpu().tolist() and mw_e._ada.state.cpu().tolist() == mw_r._ada.state.cpu().tolist()
    # augment_p's walk is the walk it takes without APA beside it
    alone, _ = _steps(states, batch, graphed=False, apa=False)
    assert [r["augment_p"] for r in alone] == [r["augment_p"] for r in eager] and "apa_p" not in alone[0]["keys"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_apa_beside_six_augmentation_words_and_adaptive_augment_p(states, batch, monkeypatch, dtype):
    ops.set_compute_dtype(dtype)
    images, labels, masks = _cuda(batch)
    names = _spy_calls(monkeypatch)
    seen = _spy_select(monkeypatch)
    mw = _wrapper(states, augment=SIX_WORDS, augment_p=_controller(8 * BATCH, p=0.5), apa=_controller(4 * BATCH, p=0.5))
    grads = {}
    og = mw.generator_optimizer
    orig = og.step

    def step(*a, **k):
        grads["g"] = [p.grad.detach().float().clone() for p in mw.generator.parameters()]
        return orig(*a, **k)
    og.step = step
    torch.manual_seed(5)
    out = mw.train_step(images, labels, masks, apa_w=torch.tensor([0.25, 0.75]))
    for n in LOSS_NAMES:
        v = float(out[n])
        assert np.isfinite(v) and 0.0 <= v < 10.0, (n, v)
    assert bool(torch.isfinite(out["images_fake"].float()).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads["g"])
    assert sum(int(bool((g != 0).any())) for g in grads["g"]) >= len(grads["g"]) // 2
    # one selection, from the storage type's fake batch, in front of the three augmenting ingests of the step
    assert names.count("sp_apa_select") == 1 and len(seen) == 1 and seen[0]["fake_dtype"] == dtype
    assert names.index("sp_apa_select") < min(i for i, n in enumerate(names) if n.startswith("sp_augment_") and n.endswith("_ingest"))
    s = seen[0]
    assert torch.equal(s["out"][0], s["fake"][0]) and torch.equal(s["out"][1], images[1]) and s["real_ptr"] == images.data_ptr()
    va, vd = mw._apa.values(), mw._ada.values()
    assert (va["p"], va["adjustments"]) == (0.75, 1) and (vd["p"], vd["adjustments"]) == (0.625, 1) and va["r_last"] > -1.0 and vd["r_last"] > -1.0
    assert float(out["apa_p"]) == 0.75 and float(out["augment_p"]) == 0.625


def test_state_round_trips_into_a_wrapper_whose_graphs_are_captured(states, batch):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    make = _controller(8 * BATCH, interval=2)               # step 0.25 every second step
    mw = _wrapper(states, apa=make)
    for i in range(3):
        torch.manual_seed(200 + i)
        mw.train_step(images, labels, masks, next_images_real=images)
    v = mw._apa.values()
    assert (v["p"], v["steps"], v["adjustments"]) == (0.25, 1, 1) and v["total"] > 0 and v["total"] % BATCH == 0      # a window half full
    checkpoint = {"apa_state": mw._apa.state_dict()}
    other = _wrapper(states, apa=make)
    torch.manual_seed(1)
    other.train_step(images, labels, masks, next_images_real=images)
    other.capture_graphs(images, labels, masks)
    ptr, gd = other._apa.state.data_ptr(), other._graph_state["gd"]
    other.load_apa_state(checkpoint)
    assert other._apa.state.data_ptr() == ptr and other._apa.state.cpu().tolist() == mw._apa.state.cpu().tolist()
    # the captured graph reads the restored p: w = 0.125 is below 0.25 now (it was not below the fresh controller's 0), w = 0.25 is not
    nd, ng, _ = _given()
    out = other.train_step_graphed(images, labels, masks, noise_d=nd, noise_g=ng, apa_w=torch.tensor([0.125, 0.25], device="cuda"), next_images_real=images)
    torch.cuda.synchronize()
    st = other._graph_state
    assert st["gd"] is gd and torch.equal(st["apa_images"][0], out["images_fake"].float()[0]) and torch.equal(st["apa_images"][1], images[1])
    # ... and the restored window closes on this step, as the original's does on its fourth
    torch.manual_seed(203)
    assert float(mw.train_step(images, labels, masks, next_images_real=images)["apa_p"]) == 0.5 and float(out["apa_p"]) == 0.5
    with pytest.raises(L.SempyrError):
        other.load_apa_state({"generator": {}})
    with pytest.raises(L.SempyrError):
        _wrapper(states, apa=0.5).load_apa_state(checkpoint)          # a fixed p steers nothing


def test_train_logs_p_and_r_and_saves_the_state(states, tmp_path, monkeypatch):
    """ModelWrapper.train() over two golden batches with the switch coming from config.CFG (SP_APA: how the reference's main.py, which
    builds the wrapper with fixed keywords, turns it on), without any augmentation.  The default window is 4 steps, so two iterations
    only count."""
    import make_golden
    ops.set_compute_dtype(torch.float32)
    torch.cuda.set_device(0)
    monkeypatch.setattr(config.CFG, "apa", "adaptive:0.25")
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF).cuda(), sp.Discriminator(channel_factor=CF).cuda(), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    loader = make_golden.TwoBatchLoader(make_golden.golden_batches(BATCH, 6), BATCH)
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=loader, validation_dataset=None,
                         generator_optimizer=torch.optim.Adam(G.parameters(), lr=1e-5),
                         discriminator_optimizer=torch.optim.Adam(D.parameters(), lr=1e-5), save_data_path=str(tmp_path))
    assert mw._apa.adaptive and mw._apa.target == 0.25 and mw._apa.threshold == 0.5 and mw._ada is None
    assert "0.25" in mw.logger.hyperparameter["apa"] and "augment_p" not in mw.logger.hyperparameter
    torch.manual_seed(1234)
    mw.train(epochs=1, device="cuda")
    assert mw.logger.metrics["apa_p"] == [0.0, 0.0] and mw.logger.metrics["apa_rt"] == [0.0, 0.0]
    assert len(mw.logger.metrics["loss_generator"]) == 2 and "augment_p" not in mw.logger.metrics
    ck = torch.load(os.path.join(mw.path_save_models, "checkpoint_000.pt"), map_location="cpu")
    assert set(ck) == {"generator", "discriminator", "generator_optimizer", "discriminator_optimizer", "apa_state"}
    sd = ck["apa_state"]
    assert (sd["target"], sd["interval"], sd["speed_images"], sd["threshold"], sd["adaptive"]) == (0.25, 4, 500_000, 0.5, True)
    p_bits, r_bits, pos, neg, total, steps, adjustments, reserved = sd["state"].tolist()
    assert (p_bits, r_bits, steps, adjustments, reserved) == (0, 0, 2, 0, 0) and pos + neg <= total and total > 0 and total % (2 * BATCH) == 0
    resumed = _wrapper(states, apa="adaptive")
    assert resumed._apa.target == 0.6
    resumed.load_apa_state(ck)
    assert resumed._apa.target == 0.25 and resumed._apa.state.cpu().tolist() == sd["state"].tolist()
