"""Adaptive pseudo augmentation's selection restated in torch (include/sempyr.h: sp_apa_select), and the sources
the tests feed it.  Everything is exact: a compare in fp32, a select, and widenings of 16-bit values."""
import numpy as np
import torch

F = np.float32
MAPS = ((1, 1), (3, 5), (4, 4), (8, 24), (64, 64))
REAL_KINDS = ("nchw", "channels_last", "slice")
FAKE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def taken(w_u: torch.Tensor, p) -> torch.Tensor:
    """Image i is the generated one iff w_u[i] < p: strict, both sides fp32 (a NaN p takes nothing)."""
    return w_u.to(torch.float32) < torch.tensor(float(p) if not isinstance(p, torch.Tensor) else p.item(), dtype=torch.float32)


def select(real: torch.Tensor, fake: torch.Tensor, w_u: torch.Tensor, p) -> torch.Tensor:
    """The contiguous fp32 (n, 3, h, w) batch sp_apa_select writes; float() of a 16-bit tensor is exact, of an fp32 one the identity."""
    take = taken(w_u, p).to(real.device)
    return torch.where(take[:, None, None, None], fake.to(torch.float32), real.to(torch.float32)).contiguous()


def bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 values as their words: what a bitwise comparison compares (NaN payloads, the sign of zero)."""
    return t.contiguous().view(torch.int32)


def straddling(n: int, p: float) -> torch.Tensor:
    """n >= 4 uniforms around p (0 < p < 1): row 0 far below, row 1 exactly p (NOT taken), row 2 the fp32 value just below p (taken),
    row 3 far above, the rest alternating 0 (taken) and the largest uniform below 1 (not taken)."""
    p32 = F(p)
    w = [F(p32 / 4), p32, np.nextafter(p32, F(0)), F(p32 + (1 - p32) / 2)] + [np.nextafter(F(1), F(0)) if i % 2 else F(0.0) for i in range(n - 4)]
    return torch.tensor(np.array(w, dtype=np.float32))


def values(shape, seed: int, dtype=torch.float32) -> torch.Tensor:
    """Values that a 16-bit type holds exactly too (multiples of 1/8 in [-4, 4)), so every dtype variant of a source shows the same
    numbers; no two neighbours alike, so that a misplaced element shows."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 32, shape, generator=g).to(torch.float32) / 8).to(dtype)


def real_variant(x: torch.Tensor, kind: str) -> torch.Tensor:
    """x (n, 3, h, w) fp32 in one of the layouts a caller's real batch comes in: NCHW, channels-last, or a slice of a larger tensor (other
    batch pitch, row pitch and a base that is not 16-byte aligned)."""
    n, c, h, w = x.shape
    if kind == "nchw":
        return x.contiguous()
    if kind == "channels_last":
        y = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
        y.copy_(x)
        return y
    if kind == "slice":
        big = torch.full((n + 1, c, h + 2, w + 3), -77.0, dtype=x.dtype, device=x.device)
        view = big[1:, :, 1:h + 1, 1:w + 1]
        view.copy_(x)
        return view
    raise ValueError(kind)


def fake_variant(x: torch.Tensor, dtype) -> torch.Tensor:
    """x (n, 3, h, w) as the generator returns its images: the NCHW view of a padded NHWC buffer whose pixel pitch is 16 bytes' worth of
    channels (4 in fp32, 8 in a 16-bit type).  The padding channels hold a value no image has."""
    n, c, h, w = x.shape
    cp = 4 if dtype == torch.float32 else 8
    buf = torch.full((n, h, w, cp), 99.0, dtype=dtype, device=x.device)
    view = buf[..., :c].permute(0, 3, 1, 2)
    view.copy_(x.to(dtype))
    return view
