"""The geometric augmentation inside the training step (ModelWrapper(augment="...,xflip,rot90,scale,rotate"); tests/test_gpu_geom.py
holds the kernels to their bound op by op): channel_factor 2, batch 2, fp32 parity mode unless a test says otherwise - the shapes and
tolerances of tests/test_gpu_augment_step.py.
  * without geometric words the wrapper draws, launches and allocates what it did before them: the device RNG stream is the (3, B, 8)
    draw and the two latent draws, no geometric entry point is called, no buffer of theirs exists, and train() writes the reference's
    checkpoint keys;
  * uniforms given: one full D+G step against the oracle's step with the restated transform in front of every discriminator forward
    (geom_restated.train_step_geom) - losses and pixels 1e-3, the norm of every parameter-gradient tensor and 16 samples of each 5e-3 -
    also with both auxiliary loss weights 0, so that every generator gradient has come through the gather;
  * eager and replayed steps agree bit for bit over three steps with fresh draws;
  * a fixed augment_p = 0.5 step with one live and one dead image per row;
  * bf16: one step with finite losses and non-zero generator gradients."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_restated as A  # noqa: E402
import geom_restated as GR  # noqa: E402
import golden_util as gu  # noqa: E402
import semantic_pyramid_for_image_generation_amd as sp  # noqa: E402
from oracle import sempyr_oracle as O  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

CF, BATCH, SEED = 2, 2, 21
OLD = "color,translation,cutout"
POLICY = "color,xflip,rot90,scale,rotate,translation,cutout"
LOSS_NAMES = ("loss_discriminator_real", "loss_discriminator_fake", "loss_generator", "loss_generator_semantic_reconstruction",
              "loss_generator_diversity")


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


def _wrapper(states, augment, adam=None, **kw):
    torch.cuda.set_device(0)
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF), sp.Discriminator(channel_factor=CF), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    G, D, V = G.cuda(), D.cuda(), V.cuda().eval()
    adam = adam or sp.optim.Adam
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=None, validation_dataset=None,
                         generator_optimizer=adam(G.parameters(), lr=1e-5), discriminator_optimizer=adam(D.parameters(), lr=1e-5),
                         save_data_path=None, augment=augment, **kw)
    G.train(); D.train()
    return mw


def _cuda(batch):
    images, labels, masks = batch
    return images.cuda(), labels.cuda(), [m.cuda() for m in masks]


def _record(out):
    rec = {k: float(out[k]) for k in LOSS_NAMES}
    rec["pixels"] = out["images_fake"].detach().float().clone()
    return rec


def _spy_calls(monkeypatch):
    names = []
    orig = L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(L, "call", call)
    return names


def test_without_geometric_words_nothing_of_them_runs(states, batch, monkeypatch):
    """The old words alone: the step's device RNG stream is torch.rand((3, B, 8)) and the two latent draws and nothing else, a step
    that draws equals the step given those very draws, eager and replayed; no sp_augment_geom_* entry is called, the graphs hold no
    buffer for v or the tables, the discriminator's armed rows are plain tensors, the log keeps its string; augment_v is an error."""
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    names = _spy_calls(monkeypatch)
    mw = _wrapper(states, OLD)
    assert (mw._aug_policy, mw._aug_geom) == (7, 0) and mw.logger.hyperparameter["augment"] == OLD
    torch.manual_seed(3)
    drawn = _record(mw.train_step(images, labels, masks, next_images_real=images))
    torch.cuda.synchronize()
    rng = torch.cuda.get_rng_state().clone()
    torch.manual_seed(3)
    u = torch.rand((3, BATCH, 8), dtype=torch.float32, device="cuda")
    nd, ng = torch.randn((BATCH, 128), device="cuda"), torch.randn((BATCH, 128), device="cuda")
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    other = _wrapper(states, OLD)
    given = _record(other.train_step(images, labels, masks, next_images_real=images, noise_d=nd, noise_g=ng, augment_u=u))
    for k in LOSS_NAMES:
        assert drawn[k] == given[k], k
    assert torch.equal(drawn["pixels"], given["pixels"])
    assert mw._aug_tables is None and mw.discriminator._augment is None
    with pytest.raises(L.SempyrError):
        mw.train_step(images, labels, masks, augment_v=torch.zeros(3, BATCH, 4, device="cuda"))
    mw.capture_graphs(images, labels, masks)
    st = mw._graph_state
    assert st["augment_u"].shape == (3, BATCH, 8) and st["augment_v"] is None and st["augment_t"] is None
    torch.manual_seed(5)
    mw.train_step_graphed(images, labels, masks, next_images_real=images)
    torch.cuda.synchronize()
    rng = torch.cuda.get_rng_state().clone()
    torch.manual_seed(5)
    torch.rand((3, BATCH, 8), device="cuda"), torch.randn((BATCH, 128), device="cuda"), torch.randn((BATCH, 128), device="cuda")
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    with pytest.raises(L.SempyrError):
        mw.train_step_graphed(images, labels, masks, augment_v=torch.zeros(3, BATCH, 4, device="cuda"))
    assert "sp_augment_ingest" in names and not [n for n in names if "geom" in n]
    # with the words the same spy sees the new entries: one decode per step
    names.clear()
    on = _wrapper(states, POLICY)
    assert on.logger.hyperparameter["augment"] == "color,translation,cutout,xflip,rot90,scale,rotate"
    on.train_step(images, labels, masks)
    assert names.count("sp_augment_geom_decode") == 1 and names.count("sp_augment_geom_ingest") == 3
    assert names.count("sp_augment_geom_ingest_bwd") == 1 and "sp_augment_ingest" not in names


def test_train_takes_the_words_from_the_configuration_and_writes_the_reference_checkpoint_keys(states, tmp_path, monkeypatch):
    import make_golden
    from semantic_pyramid_for_image_generation_amd import config
    ops.set_compute_dtype(torch.float32)
    torch.cuda.set_device(0)
    monkeypatch.setattr(config.CFG, "augment", POLICY)
    Gsd, Dsd, Vsd = states
    G, D, V = sp.Generator(channels_factor=CF).cuda(), sp.Discriminator(channel_factor=CF).cuda(), sp.VGG16()
    G.load_state_dict(Gsd); D.load_state_dict(Dsd); V.load_state_dict(Vsd)
    loader = make_golden.TwoBatchLoader(make_golden.golden_batches(BATCH, 6), BATCH)
    mw = sp.ModelWrapper(generator=G, discriminator=D, vgg16=V, training_dataset=loader, validation_dataset=None,
                         generator_optimizer=torch.optim.Adam(G.parameters(), lr=1e-5),
                         discriminator_optimizer=torch.optim.Adam(D.parameters(), lr=1e-5), save_data_path=str(tmp_path))
    assert (mw._aug_policy, mw._aug_geom) == (7, 15)
    torch.manual_seed(1234)
    mw.train(epochs=1, device="cuda")
    assert len(mw.logger.metrics["loss_generator"]) == 2 and all(np.isfinite(v) for v in mw.logger.metrics["loss_generator"])
    ck = torch.load(os.path.join(mw.path_save_models, "checkpoint_000.pt"), map_location="cpu")
    assert set(ck) == {"generator", "discriminator", "generator_optimizer", "discriminator_optimizer"}


@pytest.mark.parametrize("w_rec,w_div", [(0.1, 0.1), (0.0, 0.0)], ids=["reference_weights", "adversarial_loss_alone"])
def test_geometric_step_matches_the_restated_oracle_step(states, batch, w_rec, w_div):
    """One D+G step with u and v given, against the oracle's step with the restated transform (host-decoded fp32 tables) in front of
    every discriminator forward on identical parameters, inputs and latents.  Second case: both auxiliary loss weights 0, so that every
    generator gradient has come through the gather.  The geometric part did run: the D losses differ from those of the color,
    translation, cutout transform of the same u by more than the tolerance."""
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = batch
    Gsd, Dsd, Vsd = states
    gen = torch.Generator().manual_seed(12)
    nd, ng = torch.randn(BATCH, 128, generator=gen), torch.randn(BATCH, 128, generator=gen)
    u, v = torch.rand(3, BATCH, 8, generator=gen), torch.rand(3, BATCH, 4, generator=gen)
    mw = _wrapper(states, POLICY, adam=torch.optim.Adam)
    G, D = mw.generator, mw.discriminator
    grads = {}

    def spy(orig, key, net):
        def step(*a, **k):
            grads[key] = [p.grad.detach().float().cpu().clone() for p in net.parameters()]
            return orig(*a, **k)
        return step
    od, og = mw.discriminator_optimizer, mw.generator_optimizer
    od.step, og.step = spy(od.step, "d", D), spy(og.step, "g", G)
    out = mw.train_step(images.cuda(), labels.cuda(), [m.cuda() for m in masks], noise_d=nd.cuda(), noise_g=ng.cuda(), augment_u=u.cuda(),
                        augment_v=v.cuda(), w_rec=w_rec, w_div=w_div)
    torch.cuda.synchronize()
    assert D._augment is None
    policy, geom = ops.augment_split(POLICY)
    oG, oD, oV = O.make_state(Gsd), O.make_state(Dsd), O.make_state(Vsd, frozen=True)
    ref = GR.train_step_geom(oG, oD, oV, torch.optim.Adam(O.trainable(oG), lr=1e-5), torch.optim.Adam(O.trainable(oD), lr=1e-5),
                             images, labels, masks, nd, ng, u, v, policy, geom, w_rec=w_rec, w_div=w_div, skip_dead_d_wgrad=True)
    pairs = (("loss_discriminator_real", "loss_d_real"), ("loss_discriminator_fake", "loss_d_fake"), ("loss_generator", "loss_g"),
             ("loss_generator_semantic_reconstruction", "loss_rec"), ("loss_generator_diversity", "loss_div"))
    for a, r in pairs:
        print(a, float(out[a]), float(ref[r]))
        assert float(out[a]) == pytest.approx(float(ref[r]), rel=1e-3, abs=1e-6), a
    err = float((out["images_fake"].float().cpu() - ref["images_fake_g"]).abs().max())
    print("pixels", err)
    assert err <= 1e-3
    for key, rkey, net in (("d", "grads_d", D), ("g", "grads_g", G)):
        names = [n for n, _ in net.named_parameters()]
        got, want = grads[key], [g.float() for g in ref[rkey]]
        assert len(got) == len(want) == len(names)
        wn = np.array([float(g.double().norm()) for g in want])
        gn = np.array([float(g.double().norm()) for g in got])
        print(key, "gradient norms: worst relative difference", float((np.abs(gn - wn) / (wn + 1e-5 * wn.max())).max()))
        bad = np.abs(gn - wn) > 5e-3 * wn + 1e-5 * wn.max()
        assert not bad.any(), (key, [(names[i], gn[i], wn[i]) for i in np.nonzero(bad)[0][:5]])
        s, rs = gu.grad_samples(got), gu.grad_samples(want)
        print(key, "gradient samples", float(np.abs(s - rs).max() / np.abs(rs).max()))
        assert np.abs(s - rs).max() <= 5e-3 * np.abs(rs).max(), (key, float(np.abs(s - rs).max() / np.abs(rs).max()))
    # the color-only transform of the same u gives other discriminator losses: the comparison above is not blind to the geometry
    oD = O.make_state(Dsd)
    with torch.no_grad():
        old = O.lsgan_discriminator_loss(O.discriminator_forward(oD, A.forward(images, u[0], OLD, torch.float32), labels, training=True),
                                         O.discriminator_forward(oD, A.forward(ref["images_fake_d"], u[1], OLD, torch.float32), labels, training=True))
    for got, name in zip(old, ("loss_d_real", "loss_d_fake")):
        print(name, "color only", float(got), "with the geometry", float(ref[name]))
        assert abs(float(got) - float(ref[name])) > 1e-3 * abs(float(ref[name])) + 1e-6, name


def test_replayed_steps_match_eager_steps_bit_for_bit(states, batch):
    """The decode launch and the three transforms sit inside the captured graphs and read static buffers.  Same states, a step from
    given uniforms and latents, then three steps that draw them (u, then v, then the latents; replay: uniform_() into the static
    buffers in that order): losses, pixels, the generator's parameters and the device RNG state agree exactly."""
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = _cuda(batch)
    gen = torch.Generator().manual_seed(31)
    nd, ng = torch.randn(BATCH, 128, generator=gen).cuda(), torch.randn(BATCH, 128, generator=gen).cuda()
    u, v = torch.rand(3, BATCH, 8, generator=gen).cuda(), torch.rand(3, BATCH, 4, generator=gen).cuda()
    outs = []
    for graphed in (False, True):
        mw = _wrapper(states, POLICY)
        torch.manual_seed(11)
        mw.train_step(images, labels, masks, next_images_real=images)                     # warm-up step (eager in both runs)
        if graphed:
            mw.capture_graphs(images, labels, masks)
            st = mw._graph_state
            assert st["augment_u"].shape == (3, BATCH, 8) and st["augment_v"].shape == (3, BATCH, 4) and st["augment_t"].shape == (3 * BATCH, 8)
        step = ((lambda **kw: mw.train_step_graphed(images, labels, masks, next_images_real=images, **kw)) if graphed
                else (lambda **kw: mw.train_step(images, labels, masks, next_images_real=images, **kw)))
        recs = [_record(step(noise_d=nd, noise_g=ng, augment_u=u, augment_v=v))]
        torch.manual_seed(17)
        recs += [_record(step()) for _ in range(3)]
        recs[-1]["G"] = [p.detach().clone() for p in mw.generator.parameters()]
        torch.cuda.synchronize()
        recs[-1]["rng"] = torch.cuda.get_rng_state().clone()
        assert mw.discriminator._augment is None
        outs.append(recs)
        if graphed:
            with pytest.raises(L.SempyrError):
                step(augment_v=torch.zeros(3, BATCH, 8, device="cuda"))
    for eager, replayed in zip(*outs):
        for k in LOSS_NAMES:
            assert replayed[k] == eager[k], (k, replayed[k], eager[k])
        assert torch.equal(replayed["pixels"], eager["pixels"])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][-1]["G"], outs[1][-1]["G"]))
    assert torch.equal(outs[0][-1]["rng"], outs[1][-1]["rng"])
    losses = [r["loss_discriminator_real"] for r in outs[0]]
    assert len(set(losses)) == len(losses)          # (fresh draws: another transform every step)


def test_fixed_p_step_with_one_live_and_one_dead_image_per_row(states, batch):
    """augment_p = 0.5 with u7 = 0.25 (live) and 0.75 (dead) in each of the three transforms: the restated step transforms the live image
    and passes the dead one as it is."""
    ops.set_compute_dtype(torch.float32)
    images, labels, masks = batch
    Gsd, Dsd, Vsd = states
    gen = torch.Generator().manual_seed(41)
    nd, ng = torch.randn(BATCH, 128, generator=gen), torch.randn(BATCH, 128, generator=gen)
    u, v = torch.rand(3, BATCH, 8, generator=gen), torch.rand(3, BATCH, 4, generator=gen)
    u[:, :, 7] = torch.tensor([[0.25, 0.75], [0.75, 0.25], [0.25, 0.75]])
    mw = _wrapper(states, POLICY, adam=torch.optim.Adam, augment_p=0.5)
    out = mw.train_step(images.cuda(), labels.cuda(), [m.cuda() for m in masks], noise_d=nd.cuda(), noise_g=ng.cuda(), augment_u=u.cuda(),
                        augment_v=v.cuda())
    torch.cuda.synchronize()
    policy, geom = ops.augment_split(POLICY)
    refs = {}
    for p in (0.5, None):
        oG, oD, oV = O.make_state(Gsd), O.make_state(Dsd), O.make_state(Vsd, frozen=True)
        refs[p] = GR.train_step_geom(oG, oD, oV, torch.optim.Adam(O.trainable(oG), lr=1e-5), torch.optim.Adam(O.trainable(oD), lr=1e-5),
                                     images, labels, masks, nd, ng, u, v, policy, geom, p=p, skip_dead_d_wgrad=True)
    ref = refs[0.5]
    for a, r in (("loss_discriminator_real", "loss_d_real"), ("loss_discriminator_fake", "loss_d_fake"), ("loss_generator", "loss_g"),
                 ("loss_generator_semantic_reconstruction", "loss_rec"), ("loss_generator_diversity", "loss_div")):
        print(a, float(out[a]), float(ref[r]), float(refs[None][r]))
        assert float(out[a]) == pytest.approx(float(ref[r]), rel=1e-3, abs=1e-6), a
    assert float((out["images_fake"].float().cpu() - ref["images_fake_g"]).abs().max()) <= 1e-3
    # the ungated step is another step: the comparison is not blind to the gate
    assert abs(float(refs[None]["loss_d_real"]) - float(ref["loss_d_real"])) > 1e-3 * abs(float(ref["loss_d_real"]))


def test_geometric_step_bf16_has_finite_losses_and_generator_gradients(states, batch):
    ops.set_compute_dtype(torch.bfloat16)
    images, labels, masks = _cuda(batch)
    mw = _wrapper(states, POLICY)
    seen = {}
    og = mw.generator_optimizer
    orig = og.step

    def step(*a, **k):
        seen["g"] = [p.grad.detach().float().clone() for p in mw.generator.parameters()]
        return orig(*a, **k)
    og.step = step
    torch.manual_seed(5)
    out = mw.train_step(images, labels, masks)
    for n in LOSS_NAMES:
        val = float(out[n])
        assert np.isfinite(val) and 0.0 <= val < 10.0, (n, val)
    assert bool(torch.isfinite(out["images_fake"].float()).all())
    assert all(bool(torch.isfinite(g).all()) for g in seen["g"])
    nonzero = sum(int(bool((g != 0).any())) for g in seen["g"])
    assert nonzero >= len(seen["g"]) // 2, (nonzero, len(seen["g"]))
