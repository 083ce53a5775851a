"""Float64 numpy restatement of the reconstruction-fidelity statistics (include/sempyr.h: sp_ssim_stats) and a
DERIVED bound on what an fp32 evaluation of them may differ by.  Test infrastructure: nothing here is imported by the package.

Definition (restated): window g[k] = fp32(exp(-(k - 5)^2 / 4.5) / Z), Z the float64 sum; valid positions only; windowed means mx, my,
exx, eyy, exy; sxx = exx - mx^2, syy = eyy - my^2, sxy = exy - mx my (population form); C1 = (0.01 L)^2, C2 = (0.03 L)^2;
cs = (2 sxy + C2) / (sxx + syy + C2), l = (2 mx my + C1) / (mx^2 + my^2 + C1), ssim = l cs; float64 means over the positions; the next
scale is ((a + b) + (c + d)) * 0.25 in fp32; sqerr = float64 sum of (double)(x - y in fp32)^2.

The bound is first order in the unit roundoff u = 2^-24 and comes from OPERATION COUNTS, not from any measured error.  With A(.) the
windowed mean of a non-negative plane and p = 2 j the roundings the j poolings in front of scale j put on a pixel (two additions each; the
multiplication by 0.25 is exact):
    moments    a separable moment is 11 + 11 multiply-adds, each term of it passing at most 22 roundings:
               e(mx) = (22 + p) u A|x|, likewise my;   e(exx) = (23 + 2 p) u A(x^2) (the square is rounded once more, and carries the pixel's
               perturbation twice), likewise eyy and e(exy) = (23 + 2 p) u A|x y|
    products   e(mx^2) = 2 |mx| e(mx) + u mx^2, likewise my^2;   e(mx my) = |mx| e(my) + |my| e(mx) + u |mx my|
    the three subtractions   e(sxx) = e(exx) + e(mx^2) + u |sxx|, likewise syy and sxy (a fused multiply-subtract is no worse)
    the four forms   e(2 sxy + C2) = 2 e(sxy) + u C2 + u |2 sxy + C2|          (u C2: the constant is an fp32 number)
                     e(sxx + syy + C2) = e(sxx) + e(syy) + u |sxx + syy| + u C2 + u |sxx + syy + C2|
                     e(2 mx my + C1) = 2 e(mx my) + u C1 + u |2 mx my + C1|
                     e(mx^2 + my^2 + C1) = e(mx^2) + e(my^2) + u (mx^2 + my^2) + u C1 + u (mx^2 + my^2 + C1)
    quotients  e(n / d) = e(n) / d + |n / d| e(d) / d + u |n / d| with the ACTUAL float64 denominators d (both are >= C > 0)
    product    e(l cs) = |l| e(cs) + |cs| e(l) + u |l cs|
    mean       the mean of the per-position bounds, plus the float64 sum's own error: positions * 2^-53 * mean |map|
"""
import numpy as np

U = 2.0 ** -24
TAPS, HALO = 11, 10
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(sigma=1.5):
    """The eleven taps: fp32-rounded, returned as float64."""
    k = np.arange(TAPS, dtype=np.float64)
    e = np.exp(-(k - 5.0) ** 2 / (2.0 * sigma * sigma))
    return (e / e.sum()).astype(np.float32).astype(np.float64)


def pool2(x):
    """The next scale of (..., H, W) planes in fp32: ((a + b) + (c + d)) * 0.25."""
    x = np.asarray(x, dtype=np.float32)
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    return ((a + b) + (c + d)) * np.float32(0.25)


def filt(v, g, pad=False):
    """Separable windowed mean of (..., H, W) float64 planes: valid positions, or zero padding to the same size."""
    v = np.asarray(v, dtype=np.float64)
    if pad:
        v = np.pad(v, [(0, 0)] * (v.ndim - 2) + [(5, 5), (5, 5)])
    h, w = v.shape[-2] - HALO, v.shape[-1] - HALO
    t = sum(g[k] * v[..., :, k:k + w] for k in range(TAPS))
    return sum(g[k] * t[..., k:k + h, :] for k in range(TAPS))


def maps(x, y, data_range=2.0, sigma=1.5, pad=False, cov_scale=1.0, pool_roundings=0):
    """(cs, ssim, bound_cs, bound_ssim) per position of (..., H, W) planes, float64.  sigma / pad / cov_scale are the knobs of the
    deliberately wrong variants (1.4, zero padding, 121 / 120); the bounds belong to the definition (the defaults)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    g = window(sigma)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = filt(x, g, pad), filt(y, g, pad)
    exx, eyy, exy = filt(x * x, g, pad), filt(y * y, g, pad), filt(x * y, g, pad)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = (exx - mxx) * cov_scale, (eyy - myy) * cov_scale, (exy - mxy) * cov_scale
    ncs, dcs = 2.0 * sxy + c2, sxx + syy + c2
    nl, dl = 2.0 * mxy + c1, mxx + myy + c1
    cs, l = ncs / dcs, nl / dl
    ssim = l * cs
    # ---- the bound (module docstring) ----
    p = float(pool_roundings)
    e_mx, e_my = (22 + p) * U * filt(np.abs(x), g, pad), (22 + p) * U * filt(np.abs(y), g, pad)
    e_exx, e_eyy, e_exy = ((23 + 2 * p) * U * m for m in (exx, eyy, filt(np.abs(x * y), g, pad)))
    e_mxx = 2 * np.abs(mx) * e_mx + U * mxx
    e_myy = 2 * np.abs(my) * e_my + U * myy
    e_mxy = np.abs(mx) * e_my + np.abs(my) * e_mx + U * np.abs(mxy)
    e_sxx = e_exx + e_mxx + U * np.abs(sxx)
    e_syy = e_eyy + e_myy + U * np.abs(syy)
    e_sxy = e_exy + e_mxy + U * np.abs(sxy)
    e_ncs = 2 * e_sxy + U * c2 + U * np.abs(ncs)
    e_dcs = e_sxx + e_syy + U * np.abs(sxx + syy) + U * c2 + U * np.abs(dcs)
    e_nl = 2 * e_mxy + U * c1 + U * np.abs(nl)
    e_dl = e_mxx + e_myy + U * (mxx + myy) + U * c1 + U * np.abs(dl)
    e_cs = e_ncs / np.abs(dcs) + np.abs(cs) * e_dcs / np.abs(dcs) + U * np.abs(cs)
    e_l = e_nl / np.abs(dl) + np.abs(l) * e_dl / np.abs(dl) + U * np.abs(l)
    e_ssim = np.abs(l) * e_cs + np.abs(cs) * e_l + U * np.abs(ssim)
    return cs, ssim, e_cs, e_ssim


def pyramid(x, scales):
    """[X_0, .., X_{scales-1}] as fp32 arrays: X_0 the widened input, then the fp32 pooling rule."""
    out = [np.asarray(x, dtype=np.float32)]
    for _ in range(scales - 1):
        assert out[-1].shape[-2] % 2 == 0 and out[-1].shape[-1] % 2 == 0
        out.append(pool2(out[-1]))
    return out


def stats(x, y, scales=1, data_range=2.0, **variant):
    """ssim_mean, cs_mean (n, c, scales), sqerr (n, c) and the bounds bound_ssim, bound_cs (n, c, scales), all float64.  x, y: (n, c,
    h, w) arrays of values an fp32 holds exactly."""
    xs, ys = pyramid(x, scales), pyramid(y, scales)
    n, c = xs[0].shape[:2]
    ssim_mean, cs_mean = np.empty((n, c, scales)), np.empty((n, c, scales))
    b_ssim, b_cs = np.empty((n, c, scales)), np.empty((n, c, scales))
    for j in range(scales):
        assert xs[j].shape[-2] >= TAPS and xs[j].shape[-1] >= TAPS, "a plane below 11 x 11 is refused, not padded"
        cs, ssim, e_cs, e_ssim = maps(xs[j], ys[j], data_range, pool_roundings=2 * j, **variant)
        count = cs.shape[-2] * cs.shape[-1]
        cs_mean[:, :, j], ssim_mean[:, :, j] = cs.mean(axis=(-2, -1)), ssim.mean(axis=(-2, -1))
        b_cs[:, :, j] = e_cs.mean(axis=(-2, -1)) + count * 2.0 ** -53 * np.abs(cs).mean(axis=(-2, -1))
        b_ssim[:, :, j] = e_ssim.mean(axis=(-2, -1)) + count * 2.0 ** -53 * np.abs(ssim).mean(axis=(-2, -1))
    d = (xs[0] - ys[0]).astype(np.float64)            # the difference in fp32, widened
    sqerr = (d * d).sum(axis=(-2, -1))
    return {"ssim_mean": ssim_mean, "cs_mean": cs_mean, "sqerr": sqerr, "bound_ssim": b_ssim, "bound_cs": b_cs}


def psnr(sqerr, pixels_per_plane, data_range=2.0):
    """(n,) from sqerr (n, c); +inf for an identical pair."""
    mse = sqerr.sum(axis=1) / (sqerr.shape[1] * pixels_per_plane)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(data_range ** 2 / mse)


def ssim(st):
    """((n,) score, (n,) bound): the channel mean of scale 0; the bound is the channel mean of the bounds."""
    return st["ssim_mean"][:, :, 0].mean(axis=1), st["bound_ssim"][:, :, 0].mean(axis=1)


def ms_ssim(st):
    """((n,) score, (n,) bound) from five-scale statistics.  f(t) = max(t, 0)^w is non-decreasing and the factors are non-negative, so
    with every factor anywhere inside its own bound the channel's product lies between the products at the interval ends; the bound is
    the larger distance to them (channel mean), plus 64 float64 roundoffs for pow / prod / mean.  No linearisation: it holds at a
    clamped factor too."""
    w = np.asarray(MS_SSIM_WEIGHTS)
    t = np.concatenate([st["cs_mean"][:, :, :4], st["ssim_mean"][:, :, 4:]], axis=2)
    e = np.concatenate([st["bound_cs"][:, :, :4], st["bound_ssim"][:, :, 4:]], axis=2)
    f = lambda v: np.prod(np.maximum(v, 0.0) ** w, axis=2)                      # noqa: E731
    mid, lo, hi = f(t), f(t - e), f(t + e)
    return mid.mean(axis=1), np.maximum(hi - mid, mid - lo).mean(axis=1) + 64 * 2.0 ** -53


def psnr_bound(shape):
    """What a float64 sum of c h w exact squares in another order may move the PSNR by: the sum's relative error is at most
    c h w 2^-53 (first order), 10 log10 turns a relative error r into 10 r / ln 10; plus 8 roundoffs of 100 dB for the formula itself."""
    _, c, h, w = shape
    return 10.0 / np.log(10.0) * c * h * w * 2.0 ** -53 + 800 * 2.0 ** -53


# ---- operand families (values an fp32 holds exactly; seeded) ----
def _octave_noise(rng, shape, amp):
    """White uniform noise at every resolution h / 2^o x w / 2^o the shape admits (o < 5), each held over its 2^o x 2^o blocks and added
    up: a plane that is still noise after every pooling."""
    n, c, h, w = shape
    out = np.zeros(shape)
    for o in range(5):
        s = 1 << o
        if h % s or w % s:
            break
        out += np.kron(rng.uniform(-amp, amp, (n, c, h // s, w // s)), np.ones((s, s)))
    return out


def _octave_waves(rng, shape, amp):
    """Six octaves of products of sinusoids (wavelengths 5 .. 160 pixels), random phases per plane: structure at every scale's window."""
    n, c, h, w = shape
    r, q = np.arange(h)[:, None], np.arange(w)[None, :]
    out = np.zeros(shape)
    for o in range(6):
        lam = 5.0 * 2 ** o
        p1, p2 = rng.uniform(0, 6.28, (2, n, c, 1, 1))
        out += amp * np.sin(6.28 * r / lam + p1) * np.cos(6.28 * q / (1.3 * lam) + p2)
    return out


def family(name, shape, seed=0):
    """(x, y) float32 (n, c, h, w) in [-1, 1].  The two bounded families are zero-mean with local variances of the order of C2, where the
    constants, the window and the covariance's normalisation all matter to the result (at full contrast the quotients are scale-free
    and a wrong 121 / 120 is invisible); y = 0.6 x + an independent plane of the same kind.
    noise      multi-resolution uniform noise (amplitude 0.05 per octave; 0.03 in y's own part)
    smooth     six octaves of smooth waves (same amplitudes) plus white noise of amplitude 0.01
    flat-dark  a nearly constant plane at -0.98 (cancellation in exx - mx^2), y likewise"""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    if name == "noise":
        x = _octave_noise(rng, shape, 0.05)
        y = 0.6 * x + _octave_noise(rng, shape, 0.03)
    elif name == "smooth":
        x = _octave_waves(rng, shape, 0.05)
        y = 0.6 * x + _octave_waves(rng, shape, 0.03)
        x, y = x + rng.uniform(-0.01, 0.01, shape), y + rng.uniform(-0.01, 0.01, shape)
    elif name == "flat-dark":
        x = -0.98 + rng.uniform(-0.004, 0.004, shape)
        y = -0.98 + rng.uniform(-0.004, 0.004, shape)
    else:
        raise ValueError(name)
    return np.clip(x, -1, 1).astype(np.float32), np.clip(y, -1, 1).astype(np.float32)


def dyadic_pair(shape, seed=0):
    """(x, y) float32 whose pixels are multiples of 2^-8 in [-1, 1], and the exact sqerr (n, c) as a Python-integer sum scaled by 2^-16."""
    rng = np.random.default_rng([seed, 77])
    xi, yi = rng.integers(-256, 257, shape), rng.integers(-256, 257, shape)
    exact = ((xi - yi) ** 2).sum(axis=(-2, -1)).astype(np.float64) / 65536.0          # < 2^53: exact
    return (xi / 256.0).astype(np.float32), (yi / 256.0).astype(np.float32), exact


FAMILIES = ("noise", "smooth", "flat-dark")
BOUNDED = ("noise", "smooth")          # the families whose bound is asserted <= BOUND_CAP at every scale
BOUND_CAP = 2e-4
VARIANTS = {"sigma 1.4": dict(sigma=1.4), "zero padding": dict(pad=True), "121/120 covariance": dict(cov_scale=121.0 / 120.0)}
