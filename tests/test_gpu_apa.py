"""sp_apa_select on the device, op by op (csrc/apa.hip; ops.apa_select), against the torch restatement of
tests/apa_restated.py.  EVERY comparison is bitwise: the kernel compares two fp32 values, copies fp32 words and widens 16-bit values.
  n = 5; maps 1 x 1, 3 x 5, 4 x 4, 8 x 24, 64 x 64 (a single pixel, odd widths for the vector tail, more than one block per image);
  real: fp32 NCHW, fp32 channels-last, a strided slice of a larger tensor - crossed with
  fake: fp32, bf16, fp16 as the padded-NHWC-backed NCHW view the generator returns.
Per case: w_u straddling p (one row == p: not taken; one row nextafter(p, 0): taken), p = 0 (the real batch bit for bit), p = 1 (the
fake batch widened), NaN and +-inf planted in both sources, canaries on both sides of dst, two runs identical.  Beside that: p changed
between two replays of one captured graph, 16-bit real sources, and the refused 16-bit mix."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import apa_restated as R  # noqa: E402
from semantic_pyramid_for_image_generation_amd import _lib as L  # noqa: E402
from semantic_pyramid_for_image_generation_amd import ops  # noqa: E402

N = 5
P = 0.3
CANARY = -123456.0
SPECIALS = (float("nan"), float("inf"), float("-inf"))


def _dev_p(p):
    return torch.tensor([p], dtype=torch.float32, device="cuda")


def _sources(h, w, real_kind, fake_dtype):
    """One (real, fake) pair on the device in the named layouts, with NaN, +inf and -inf planted in every image of both sources (at
    positions that depend on the image, first and last pixel included), so that whichever source an image comes from, they must arrive."""
    real, fake = R.values((N, 3, h, w), 11), R.values((N, 3, h, w), 12)
    for src in (real, fake):
        flat = src.view(N, -1)
        for i in range(N):
            for k, s in enumerate(SPECIALS):
                flat[i, (i * 7 + k * (3 * h * w - 1) // 2) % (3 * h * w)] = s
    return R.real_variant(real.cuda(), real_kind), R.fake_variant(fake.cuda(), fake_dtype)


def _run(real, fake, w_u, p_dev):
    """ops.apa_select into the middle of a canary-filled buffer: (result, canaries intact)."""
    n, _, h, w = real.shape
    numel = n * 3 * h * w
    pad = 64                                               # floats: keeps the result 16-byte aligned, as a fresh tensor is
    buf = torch.full((numel + 2 * pad,), CANARY, dtype=torch.float32, device="cuda")
    out = buf[pad:pad + numel].view(n, 3, h, w)
    got = ops.apa_select(real, fake, w_u, p_dev, out=out)
    assert got.data_ptr() == out.data_ptr()
    ok = bool((buf[:pad] == CANARY).all()) and bool((buf[pad + numel:] == CANARY).all())
    return got, ok


@pytest.mark.parametrize("fake_dtype", R.FAKE_DTYPES, ids=["fake_fp32", "fake_bf16", "fake_fp16"])
@pytest.mark.parametrize("real_kind", R.REAL_KINDS)
@pytest.mark.parametrize("hw", R.MAPS, ids=["%dx%d" % m for m in R.MAPS])
def test_selection_equals_the_restatement_bit_for_bit(hw, real_kind, fake_dtype):
    h, w = hw
    real, fake = _sources(h, w, real_kind, fake_dtype)
    assert not real.requires_grad and fake.dtype == fake_dtype
    w_u = R.straddling(N, P).cuda()
    take = R.taken(w_u.cpu(), P).tolist()
    assert take == [True, False, True, False, True] and w_u[1].item() == float(np.float32(P))
    # straddling p: exactly the rows below p come from the fake batch; the row ON p does not, the row one step below it does
    want = R.select(real, fake, w_u, P)
    got, canaries = _run(real, fake, w_u, _dev_p(P))
    assert canaries
    assert got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad
    assert torch.equal(R.bits(got), R.bits(want))
    for i in range(N):                                    # ... said once more without the restatement's select
        src = fake if take[i] else real
        assert torch.equal(R.bits(got[i]), R.bits(src[i].float())), i
    for s in SPECIALS:                                    # the planted values arrived, from whichever source was selected
        hit = torch.isnan(got) if s != s else got == s
        assert bool(hit.view(N, -1).any(dim=1).all())
    # two runs are identical
    again, canaries = _run(real, fake, w_u, _dev_p(P))
    assert canaries and torch.equal(R.bits(again), R.bits(got))
    # p = 0: the real batch bit for bit (not even w = 0 is below it); p = 1: the fake batch, widened
    w0 = torch.tensor([0.0, 0.25, 0.5, 0.75, float(np.nextafter(np.float32(1), np.float32(0)))], device="cuda")
    got0, c0 = _run(real, fake, w0, _dev_p(0.0))
    got1, c1 = _run(real, fake, w0, _dev_p(1.0))
    assert c0 and c1
    assert torch.equal(R.bits(got0), R.bits(real.contiguous()))
    assert torch.equal(R.bits(got1), R.bits(fake.float()))
    # a fresh result tensor (no out=) holds the same
    assert torch.equal(R.bits(ops.apa_select(real, fake, w_u, _dev_p(P))), R.bits(want))


def test_nan_payloads_and_the_sign_of_zero_pass_through_fp32_sources():
    words = torch.tensor([0x7FC00000, 0x7FC12345, -0x3FEDCB, 0x7F800000, -0x800000, -0x80000000, 1, 0], dtype=torch.int32)
    for real_kind in R.REAL_KINDS:
        real, fake = R.values((2, 3, 2, 4), 4), R.values((2, 3, 2, 4), 5)
        real[0, 0].view(-1).copy_(words.view(torch.float32))
        fake[1, 2].view(-1).copy_(words.view(torch.float32))
        real, fake = R.real_variant(real.cuda(), real_kind), R.fake_variant(fake.cuda(), torch.float32)
        got = ops.apa_select(real, fake, torch.tensor([0.75, 0.25], device="cuda"), _dev_p(0.5))
        assert torch.equal(R.bits(got[0, 0]).view(-1).cpu(), words) and torch.equal(R.bits(got[1, 2]).view(-1).cpu(), words)
        assert torch.equal(R.bits(got[0]), R.bits(real[0].contiguous())) and torch.equal(R.bits(got[1]), R.bits(fake[1].contiguous()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16_bit_real_sources_and_plain_layouts_of_the_fake(dtype):
    """Beyond the layouts a training step meets: a 16-bit real batch (NCHW: 8-byte loads; channels-last: element loads), an NCHW fake,
    and both sources of the one 16-bit type."""
    h, w = 8, 24
    x, y = R.values((N, 3, h, w), 21), R.values((N, 3, h, w), 22)
    w_u = R.straddling(N, P).cuda()
    for real in (x.cuda().to(dtype), R.real_variant(x.cuda(), "channels_last").to(dtype), R.real_variant(x.cuda().to(dtype), "slice")):
        for fake in (y.cuda(), y.cuda().to(dtype), R.fake_variant(y.cuda(), dtype)):
            got, canaries = _run(real, fake, w_u, _dev_p(P))
            assert canaries and torch.equal(R.bits(got), R.bits(R.select(real, fake, w_u, P)))


def test_a_captured_graph_follows_p_without_a_recapture():
    h, w = 8, 24
    real, fake = _sources(h, w, "nchw", torch.bfloat16)
    w_u = torch.tensor([0.1, 0.3, 0.5, 0.7, 0.9], device="cuda")
    p_dev = _dev_p(0.0)
    out = torch.zeros((N, 3, h, w), dtype=torch.float32, device="cuda")
    ops.apa_select(real, fake, w_u, p_dev, out=out)        # (the library is loaded and the kernel resident before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.apa_select(real, fake, w_u, p_dev, out=out)
    seen = []
    for p in (0.0, 0.4, 0.8, 1.0, 0.4):
        p_dev.fill_(p)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(R.bits(out), R.bits(R.select(real, fake, w_u, p))), p
        seen.append([bool(torch.equal(R.bits(out[i]), R.bits(fake[i].float()))) for i in range(N)])
    assert seen == [[False] * 5, [True, True, False, False, False], [True, True, True, True, False], [True] * 5,
                    [True, True, False, False, False]]
    # fresh uniforms in the static buffer change the selection likewise
    w_u.copy_(torch.tensor([0.9, 0.7, 0.5, 0.3, 0.1], device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out), R.bits(R.select(real, fake, w_u, 0.4)))


def test_the_16_bit_mix_and_malformed_arguments_are_refused():
    x = R.values((N, 3, 4, 4), 31).cuda()
    w_u, p = torch.zeros(N, device="cuda"), _dev_p(0.5)
    before = torch.full((N, 3, 4, 4), CANARY, device="cuda")
    out = before.clone()
    for real, fake in ((x.bfloat16(), x.half()), (x.half(), x.bfloat16()), (x.half(), R.fake_variant(x, torch.bfloat16))):
        with pytest.raises(L.SempyrError):
            ops.apa_select(real, fake, w_u, p, out=out)
    # ... and by the library itself, whatever the host checks: SP_ERR_UNSUPPORTED (-3), nothing launched
    lib = L.lib()
    for rt, ft, st in ((L.SP_BF16, L.SP_F32, L.SP_F16), (L.SP_F32, L.SP_F16, L.SP_BF16), (L.SP_F16, L.SP_F32, L.SP_F32)):
        rc = lib.sp_apa_select(ops.ptr(x), rt, *x.stride(), ops.ptr(x), ft, *x.stride(), ops.ptr(out), N, 4, 4, ops.ptr(w_u), ops.ptr(p), st, ops.stream())
        assert rc == -3 and b"sp_apa_select" in lib.sp_last_error_string()
    for bad in (dict(w_u=torch.zeros(N + 1, device="cuda")), dict(w_u=torch.zeros(N, device="cuda", dtype=torch.float64)), dict(w_u=torch.zeros(N)),
                dict(p=0.5), dict(p=torch.tensor([0.5])), dict(p=torch.zeros(2, device="cuda")), dict(p=None),
                dict(fake=x[:, :, :, :3]), dict(fake=x[:4]), dict(real=x[:, :2], fake=x[:, :2]),
                dict(out=torch.zeros((N, 3, 4, 4), device="cuda", dtype=torch.float16)), dict(out=torch.zeros((N, 3, 4, 5), device="cuda")),
                dict(out=torch.zeros((N, 4, 4, 3), device="cuda").permute(0, 3, 1, 2))):
        kw = dict(real=x, fake=x, w_u=w_u, p=p, out=out)
        kw.update(bad)
        with pytest.raises(L.SempyrError):
            ops.apa_select(kw["real"], kw["fake"], kw["w_u"], kw["p"], out=kw["out"])
    torch.cuda.synchronize()
    assert torch.equal(out, before)                       # nothing was launched


def test_the_result_carries_no_autograd_graph():
    x = R.values((N, 3, 4, 4), 41).cuda().requires_grad_(True)
    y = (R.values((N, 3, 4, 4), 42).cuda().requires_grad_(True) * 1.0)
    got = ops.apa_select(x, y, R.straddling(N, P).cuda(), _dev_p(P))
    assert not got.requires_grad and got.grad_fn is None
