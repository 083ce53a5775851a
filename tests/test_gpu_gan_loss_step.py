"""The hinge / logistic losses and the LeCam regularizer inside the training step (ModelWrapper(gan_loss=..., lecam=...); DESIGN.md
section 18; tests/test_gpu_gan_loss.py holds the kernels op by op): channel_factor 2, batch 2, fp32 parity mode unless a test says
otherwise; states and batch as tests/test_gpu_ada_step.py builds them.
  * both unset: the wrapper built without the keywords, bit for bit, and no ops.LeCam;
  * one D+G step per kind against the oracle's forwards with the restated losses (gan_loss_restated.train_step_restated), to the
    tolerances of tests/test_gpu_augment_step.py (losses and pixels 1e-3, gradient norms 5e-3) - and the oracle's LSGAN losses differ
    from the restated ones by more than that, so the comparison sees the kind;
  * LeCam on LSGAN (start 1, decay 0.5, weight 1), three steps against the restated step; anchors to 1e-4 absolute (the tolerance
    tests/test_gpu_ada_step.py documents for the predictions they are means of);
  * five replayed steps equal five eager ones bit for bit with hinge and LeCam on;
  * the LeCam state round-trips through a checkpoint of train(); the log holds the three keys;
  * the adaptive augmentation counts around the D loss module's decision threshold;
  * bf16 and fp16: one step with logistic + LeCam, finite losses and generator gradients."""
import gc
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_loss_restated as R  # noqa: E402
import golden_util as gu  # noqa: E402
import semantic_pyramid_for_image_generation_amd as sp  # noqa: E402
from oracle import sempyr_oracle as O  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import lossfunction, ops  # noqa: E402

CF, BATCH, SEED = 2, 2, 21
LOSS_NAMES = ("loss_discriminator_real", "loss_discriminator_fake", "loss_generator", "loss_generator_semantic_reconstruction",
              "loss_generator_diversity")
LECAM_NAMES = ("loss_discriminator_lecam", "lecam_anchor_real", "lecam_anchor_fake")
PAIRS = (("loss_discriminator_real", "loss_d_real"), ("loss_discriminator_fake", "loss_d_fake"), ("loss_generator", "loss_g"),
         ("loss_generator_semantic_reconstruction", "loss_rec"), ("loss_generator_diversity", "loss_div"))
UNSET = object()


@pytest.fixture(autouse=True)
def _reset():
    yield
    ops.set_compute_dtype(torch.float32)
    ops.set_loss_scale(65536.0)


@pytest.fixture(scope="module")
def states():
    return gu.synth_states({"cf": CF, "seed": SEED})


@pytest.fixture(scope="module")
def batch():
    images, labels, masks = gu.golden_batches(BATCH, 6)[0]
    return images, labels, masks


def _wrapper(states, gan_loss=UNSET, lecam=UNSET, adam=None, **kw):
    torch.cuda.set_device(0)
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF), sp.Discriminator(channel_factor=CF), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    G, D, V = G.cuda(), D.cuda(), V.cuda().eval()
    adam = adam or sp.optim.Adam
    if gan_loss is not UNSET:
        kw["gan_loss"] = gan_loss
    if lecam is not UNSET:
        kw["lecam"] = lecam(D) if callable(lecam) else lecam
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=None, validation_dataset=None,
                         generator_optimizer=adam(G.parameters(), lr=1e-5), discriminator_optimizer=adam(D.parameters(), lr=1e-5),
                         save_data_path=None, **kw)
    G.train(); D.train()
    return mw


def _cuda(batch):
    images, labels, masks = batch
    return images.cuda(), labels.cuda(), [m.cuda() for m in masks]


def _record(out):
    rec = {k: float(out[k]) for k in LOSS_NAMES + LECAM_NAMES if k in out}
    rec["pixels"] = out["images_fake"].detach().float().clone()
    rec["keys"] = sorted(out.keys())
    return rec


def _spy(mw):
    """Copies of the gradients each optimizer step sees."""
    grads = {}

    def spy(orig, key, net):
        def step(*a, **k):
            grads[key] = [p.grad.detach().float().cpu().clone() for p in net.parameters()]
            return orig(*a, **k)
        return step
    od, og = mw.discriminator_optimizer, mw.generator_optimizer
    od.step, og.step = spy(od.step, "d", mw.discriminator), spy(og.step, "g", mw.generator)
    return grads


def _norms(grads):
    return np.array([float(g.double().norm()) for g in grads])


def _norms_differ(got, want):
    """Per parameter: outside the gradient-norm tolerance of tests/test_gpu_augment_step.py."""
    gn, wn = _norms(got), _norms(want)
    return np.abs(gn - wn) > 5e-3 * wn + 1e-5 * wn.max()


def _latents(seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(BATCH, 128, generator=gen), torch.randn(BATCH, 128, generator=gen)


def test_off_is_off(states, batch):
    images, labels, masks = _cuda(batch)
    runs = []
    for kw in ({}, {"gan_loss": None, "lecam": None}, {"gan_loss": "", "lecam": ""}, {"lecam": 0}):
        mw = _wrapper(states, **kw)
        assert mw._lecam is None and mw.gan_loss == "" and "lecam" not in mw.logger.hyperparameter and "gan_loss" not in mw.logger.hyperparameter
        assert type(mw.discriminator_loss) is sp.LSGANDiscriminatorLoss and type(mw.generator_loss) is sp.LSGANGeneratorLoss
        recs = []
        for i in range(2):
            torch.manual_seed(3 + i)
            recs.append(_record(mw.train_step(images, labels, masks)))
        torch.cuda.synchronize()
        recs.append(torch.cuda.get_rng_state().clone())
        runs.append(recs)
        with pytest.raises(L.SempyrError):
            mw.load_lecam_state({"state": torch.zeros(8, dtype=torch.int32)})
    for other in runs[1:]:
        for a, b in zip(runs[0][:2], other[:2]):
            assert a["keys"] == b["keys"] and not set(LECAM_NAMES) & set(a["keys"])
            for k in LOSS_NAMES:
                assert a[k] == b[k], k
            assert torch.equal(a["pixels"], b["pixels"])
        assert torch.equal(runs[0][2], other[2])


def test_settings_are_parsed_and_refused(states):
    mw = _wrapper(states, "hinge", "0.3:0.9:5")
    assert type(mw.discriminator_loss) is sp.HingeDiscriminatorLoss and type(mw.generator_loss) is sp.HingeGeneratorLoss
    assert mw._lecam.settings() == {"weight": 0.3, "decay": 0.9, "start": 5, "rectified": False}
    assert mw.logger.hyperparameter["gan_loss"] == "hinge" and "0.3" in mw.logger.hyperparameter["lecam"]
    assert mw.logger.hyperparameter["discriminator_loss"] == "HingeDiscriminatorLoss"
    assert _wrapper(states, "lsgan", 0.5)._lecam.settings() == {"weight": 0.5, "decay": 0.99, "start": 1000, "rectified": False}
    own = _wrapper(states, "logistic", lambda D: ops.LeCam(next(D.parameters()).device, 2.0, rectified=True))
    assert own._lecam.rectified and type(own.generator_loss) is sp.LogisticGeneratorLoss
    for bad in ({"gan_loss": "wgan"}, {"gan_loss": 3}, {"lecam": "0.3:1.5"}, {"lecam": "x"}, {"lecam": -1.0}, {"lecam": True},
                {"gan_loss": "hinge", "discriminator_loss": sp.LSGANDiscriminatorLoss()}, {"gan_loss": "lsgan", "generator_loss": sp.LSGANGeneratorLoss()}):
        with pytest.raises(L.SempyrError):
            _wrapper(states, **bad)
    assert (sp.LSGANDiscriminatorLoss.decision_threshold, sp.HingeDiscriminatorLoss.decision_threshold,
            sp.LogisticDiscriminatorLoss.decision_threshold) == (0.5, 0.0, 0.0)
    assert set(lossfunction.GAN_LOSSES) == {"lsgan", "hinge", "logistic"}


def _oracle(states, kind, lecam=None):
    Gsd, Dsd, Vsd = states
    oG, oD, oV = O.make_state(Gsd), O.make_state(Dsd), O.make_state(Vsd, frozen=True)
    return oG, oD, oV, torch.optim.Adam(O.trainable(oG), lr=1e-5), torch.optim.Adam(O.trainable(oD), lr=1e-5)


@pytest.mark.parametrize("kind", ["hinge", "logistic"])
def test_one_step_per_kind_matches_the_restated_oracle_step(states, batch, kind):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = batch
    nd, ng = _latents(12)
    mw = _wrapper(states, kind, adam=torch.optim.Adam)
    grads = _spy(mw)
    out = mw.train_step(images.cuda(), labels.cuda(), [m.cuda() for m in masks], noise_d=nd.cuda(), noise_g=ng.cuda())
    torch.cuda.synchronize()
    assert not set(LECAM_NAMES) & set(out)
    oG, oD, oV, og, od = _oracle(states, kind)
    ref = R.train_step_restated(oG, oD, oV, og, od, images, labels, masks, nd, ng, kind=kind, skip_dead_d_wgrad=True)
    for a, r in PAIRS:
        print(kind, a, float(out[a]), float(ref[r]))
        assert float(out[a]) == pytest.approx(float(ref[r]), rel=1e-3, abs=1e-6), a
    err = float((out["images_fake"].float().cpu() - ref["images_fake_g"]).abs().max())
    print("pixels", err)
    assert err <= 1e-3
    for key, rkey, net in (("d", "grads_d", mw.discriminator), ("g", "grads_g", mw.generator)):
        names = [n for n, _ in net.named_parameters()]
        want = [g.float() for g in ref[rkey]]
        assert len(grads[key]) == len(want) == len(names)
        bad = _norms_differ(grads[key], want)
        assert not bad.any(), (key, [(names[i], _norms(grads[key])[i], _norms(want)[i]) for i in np.nonzero(bad)[0][:5]])
    # the oracle's LSGAN losses of the same step are outside that tolerance: a wrapper still on LSGAN would have failed above
    oG, oD, oV, og, od = _oracle(states, "lsgan")
    ls = O.train_step(oG, oD, oV, og, od, images, labels, masks, nd, ng, skip_dead_d_wgrad=True)
    for k in ("loss_d_real", "loss_d_fake", "loss_g"):
        print("lsgan", k, float(ls[k]), float(ref[k]))
        assert not float(ls[k]) == pytest.approx(float(ref[k]), rel=1e-3, abs=1e-6), k


def _clone_state(S):
    return {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in S.items()}


def test_lecam_on_lsgan_three_steps_match_the_restated_step(states, batch):
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = batch
    mw = _wrapper(states, lecam=lambda D: ops.LeCam(next(D.parameters()).device, 1.0, decay=0.5, start=1), adam=torch.optim.Adam)
    grads = _spy(mw)
    oG, oD, oV, og, od = _oracle(states, "lsgan")
    lecam = R.TorchLeCam(1.0, 0.5, 1)
    dev = _cuda(batch)
    for step in range(3):
        nd, ng = _latents(40 + step)
        # the same step from the same weights WITHOUT the regularizer (its optimizers are throw-aways: only the gradients are read)
        cG, cD = _clone_state(oG), _clone_state(oD)
        plain = R.train_step_restated(cG, cD, oV, torch.optim.Adam(O.trainable(cG), lr=1e-5), torch.optim.Adam(O.trainable(cD), lr=1e-5),
                                      images, labels, masks, nd, ng, skip_dead_d_wgrad=True)
        out = mw.train_step(*dev, noise_d=nd.cuda(), noise_g=ng.cuda())
        torch.cuda.synchronize()
        got = {k: float(out[k]) for k in LOSS_NAMES + LECAM_NAMES}
        ref = R.train_step_restated(oG, oD, oV, og, od, images, labels, masks, nd, ng, lecam=lecam, skip_dead_d_wgrad=True)
        m = lecam.machine
        print("step", step, got, float(ref["loss_lecam"]), float(m.a_real), float(m.a_fake))
        for a, r in PAIRS:
            assert got[a] == pytest.approx(float(ref[r]), rel=1e-3, abs=1e-6), (step, a)
        assert got["lecam_anchor_real"] == pytest.approx(float(m.a_real), abs=1e-4) and got["lecam_anchor_fake"] == pytest.approx(float(m.a_fake), abs=1e-4)
        want_d = [g.float() for g in ref["grads_d"]]
        assert not _norms_differ(grads["d"], want_d).any(), step
        differs = _norms_differ(grads["d"], [g.float() for g in plain["grads_d"]])
        if step == 0:
            assert got["loss_discriminator_lecam"] == 0.0 and float(ref["loss_lecam"]) == 0.0 and not differs.any()
            assert all(torch.allclose(a, b, rtol=1e-6, atol=1e-12) for a, b in zip(ref["grads_d"], plain["grads_d"]))
        else:
            assert got["loss_discriminator_lecam"] > 0.0
            # reg = mean d_r^2 + mean d_f^2 (weight 1) with every difference d = prediction - anchor off by at most delta = 2e-4 (1e-4 for
            # the prediction, 1e-4 for the anchor): |reg - want| <= 2 delta (rms d_r + rms d_f) + 2 delta^2 <= 2 delta sqrt(2 want) + 2 delta^2
            want, delta = float(ref["loss_lecam"]), 2e-4
            assert abs(got["loss_discriminator_lecam"] - want) <= 2 * delta * (2 * want) ** 0.5 + 2 * delta ** 2, (step, got, want)
            assert differs.any(), step
    assert mw._lecam.values()["updates"] == 3 and mw._lecam.values()["active"] == 1


def _steps(states, batch, graphed):
    """Six steps from one seed per step: the first eager, then five replayed through the graphs captured behind it if `graphed`."""
    ops.set_compute_dtype(torch.float32)
    gc.collect()                                    # both runs start as capture_graphs() itself starts: nothing of an earlier test's
    torch.cuda.synchronize()                        # wrappers alive or in flight
    images, labels, masks = _cuda(batch)
    mw = _wrapper(states, "hinge", lambda D: ops.LeCam(next(D.parameters()).device, 1.0, decay=0.5, start=2))
    recs = []
    for i in range(6):
        if graphed and i == 1:
            mw.capture_graphs(images, labels, masks)
            state_ptr, gd = mw._lecam.state.data_ptr(), mw._graph_state["gd"]
        torch.manual_seed(100 + i)
        if graphed and i >= 1:
            out = mw.train_step_graphed(images, labels, masks, next_images_real=images)
        else:
            out = mw.train_step(images, labels, masks, next_images_real=images)
        rec = _record(out)
        rec["state"] = mw._lecam.state.cpu().tolist()
        recs.append(rec)
    if graphed:
        assert mw._lecam.state.data_ptr() == state_ptr and mw._graph_state["gd"] is gd
    return recs


def test_replay_equals_eager_bit_for_bit_with_hinge_and_lecam(states, batch):
    """Measured: run on its own, and behind any ONE other test of this file, every figure of the five replayed steps equals the eager
    one.  Behind tests/test_block_golden.py + tests/test_gpu_gan_loss.py + the tests above in one process the EAGER run came out
    different twice: once loss_discriminator_fake of step 0 0.9762067795 against 0.9762110114, once loss_generator of step 3
    0.008699833415 against 0.008699837141; the replayed figures were those of the run on its own every time, and the same sequence with
    a device synchronisation behind every pair pass passed; so did the whole GPU suite in its natural order in one process and this
    file on its own.  The cause was not found; nothing this test checks was relaxed."""
    eager, replayed = _steps(states, batch, False), _steps(states, batch, True)
    for i, (a, b) in enumerate(zip(eager, replayed)):
        print("step", i, [(k, a[k], b[k]) for k in LOSS_NAMES + LECAM_NAMES], a["state"], b["state"])
    assert [r["state"][2] for r in replayed] == [1, 2, 3, 4, 5, 6] and [r["state"][3] for r in replayed] == [0, 0, 1, 1, 1, 1]
    assert set(LECAM_NAMES) <= set(replayed[1]["keys"])
    for i, (a, b) in list(enumerate(zip(eager, replayed)))[1:]:
        for k in LOSS_NAMES + LECAM_NAMES:
            assert a[k] == b[k], (i, k, a[k], b[k])
        assert torch.equal(a["pixels"], b["pixels"]) and a["state"] == b["state"], i
    assert replayed[1]["loss_discriminator_lecam"] == 0.0 and replayed[5]["loss_discriminator_lecam"] > 0.0


def test_train_logs_the_three_keys_and_the_checkpoint_round_trips(states, tmp_path, monkeypatch):
    """ModelWrapper.train() over two golden batches with both switches coming from config.CFG (SP_GAN_LOSS / SP_LECAM: how the reference's
    main.py, which builds the wrapper with fixed keywords, turns them on)."""
    import make_golden
    from semantic_pyramid_for_image_generation_amd import config
    ops.set_compute_dtype(torch.float32)
    torch.cuda.set_device(0)
    monkeypatch.setattr(config.CFG, "gan_loss", "hinge")
    monkeypatch.setattr(config.CFG, "lecam", "0.5:0.9:1")
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF).cuda(), sp.Discriminator(channel_factor=CF).cuda(), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    loader = make_golden.TwoBatchLoader(make_golden.golden_batches(BATCH, 6), BATCH)
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=loader, validation_dataset=None,
                         generator_optimizer=torch.optim.Adam(G.parameters(), lr=1e-5),
                         discriminator_optimizer=torch.optim.Adam(D.parameters(), lr=1e-5), save_data_path=str(tmp_path))
    assert type(mw.discriminator_loss) is sp.HingeDiscriminatorLoss and mw._lecam.settings()["decay"] == 0.9
    torch.manual_seed(1234)
    mw.train(epochs=1, device="cuda")
    for k in LECAM_NAMES:
        assert len(mw.logger.metrics[k]) == 2 and all(np.isfinite(v) for v in mw.logger.metrics[k]), k
    assert mw.logger.metrics["loss_discriminator_lecam"][0] == 0.0 and mw.logger.metrics["loss_discriminator_lecam"][1] > 0.0
    ck = torch.load(os.path.join(mw.path_save_models, "checkpoint_000.pt"), map_location="cpu")
    assert set(ck) == {"generator", "discriminator", "generator_optimizer", "discriminator_optimizer", "lecam_state"}
    sd = ck["lecam_state"]
    assert (sd["weight"], sd["decay"], sd["start"], sd["rectified"]) == (0.5, 0.9, 1, False)
    assert sd["state"].tolist() == mw._lecam.state.cpu().tolist() and sd["state"].tolist()[2:4] == [2, 1]
    fresh = _wrapper(states, "hinge", 0.25)
    ptr = fresh._lecam.state.data_ptr()
    fresh.load_lecam_state(ck)
    assert fresh._lecam.state.data_ptr() == ptr and fresh._lecam.state.cpu().tolist() == sd["state"].tolist()
    assert fresh._lecam.settings() == mw._lecam.settings()
    with pytest.raises(L.SempyrError):
        fresh.load_lecam_state({"generator": {}})
    with pytest.raises(L.SempyrError):
        _wrapper(states, "hinge", "").load_lecam_state(ck)             # ("": off, whatever config.CFG says)


def test_adaptive_augmentation_counts_around_the_loss_modules_threshold(states):
    kw = {"augment": "translation", "augment_p": "adaptive"}
    assert _wrapper(states, "hinge", **kw)._ada.threshold == 0.0
    assert _wrapper(states, "logistic", **dict(kw, augment_p="adaptive:0.3"))._ada.threshold == 0.0
    assert _wrapper(states, "lsgan", **kw)._ada.threshold == 0.5 and _wrapper(states, **kw)._ada.threshold == 0.5
    torch.cuda.set_device(0)
    own = ops.AdaptiveAugment(torch.device("cuda", 0), threshold=0.25)
    mw = _wrapper(states, "hinge", **dict(kw, augment_p=own))
    assert mw._ada is own and own.threshold == 0.25

    class Foreign(torch.nn.Module):
        def forward(self, prediction_real, prediction_fake):
            return ops.sqerr_loss(prediction_real, 1.0), ops.sqerr_loss(prediction_fake, 0.0)
    assert _wrapper(states, discriminator_loss=Foreign(), **kw)._ada.threshold == 0.5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16_bit_step_with_logistic_and_lecam_is_finite(states, batch, dtype):
    ops.set_compute_dtype(dtype)
    images, labels, masks = _cuda(batch)
    mw = _wrapper(states, "logistic", lambda D: ops.LeCam(next(D.parameters()).device, 1.0, decay=0.5, start=0))
    seen = {}
    og = mw.generator_optimizer
    orig = og.step

    def step(*a, **k):
        seen["g"] = [p.grad.detach().float().clone() for p in mw.generator.parameters()]
        return orig(*a, **k)
    og.step = step
    torch.manual_seed(5)
    out = mw.train_step(images, labels, masks)
    for n in LOSS_NAMES + LECAM_NAMES:
        v = float(out[n])
        assert np.isfinite(v) and -10.0 < v < 10.0, (n, v)
    assert float(out["loss_discriminator_lecam"]) > 0.0 and mw._lecam.values()["active"] == 1
    assert bool(torch.isfinite(out["images_fake"].float()).all())
    assert all(bool(torch.isfinite(g).all()) for g in seen["g"])
    nonzero = sum(int(bool((g != 0).any())) for g in seen["g"])
    assert nonzero >= len(seen["g"]) // 2, (nonzero, len(seen["g"]))
