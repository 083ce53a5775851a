// Differentiable augmentation of the discriminator's input images inside the ingest pass (Zhao et al. 2020, "DiffAugment").
// The reference has no counterpart.  These kernels REPLACE sp_ingest_image / sp_ingest_image_bwd (eltwise.hip) where a caller arms
// them: same source, same padded NHWC destination, the transform applied on the way.
//
// THE TRANSFORM (stated once here and in DESIGN.md section 11; include/sempyr.h repeats it for the ABI's reader).
// One row u of 8 fp32 uniforms in [0, 1) per image; policy = any subset of color / translation / cutout, a part left out is the
// identity; 3-channel H x W images; fp32 arithmetic whatever the storage type.  Forward, in this order:
//   color        o = u0 - 0.5, s = 2 u1, k = u2 + 0.5
//                b = x + o;  a = (b - m) s + m, m = (b_0 + b_1 + b_2) / 3;  e = (a - M) k + M, M = sum(x) / (3 H W) + o
//                (saturation keeps the per-pixel channel mean, so ONE reduction of the raw input gives the contrast's mean)
//   translation  r_y = int(H / 8 + 0.5), t_y = min(int(floorf(u3 * float(2 r_y + 1))), 2 r_y) - r_y; t_x from W and u4
//                out[h, w] = e[h + t_y, w + t_x], 0 outside the frame
//   cutout       q_y = int(H / 2 + 0.5), n_y = H + 1 - (q_y % 2), c_y = min(int(floorf(u5 * float(n_y))), n_y - 1); rows
//                [c_y - q_y / 2, c_y - q_y / 2 + q_y) cut with [0, H) are zeroed, columns likewise from W and u6; u7 is unused
//                by the ungated entries and is the GATE's draw on the gated ones (below)
// Backward:  g1[c, h, w] = dy[c, h - t_y, w - t_x] where that position is inside the frame and outside the window, else 0;
//            Gm = sum(g1) / (3 H W);  g2 = k g1 + (1 - k) Gm;  dx_c = s g2_c + (1 - s) (g2_0 + g2_1 + g2_2) / 3.
//
// LAUNCHES.  With color, two per application and direction: a statistics launch - grid (slices, images), 16-byte loads, wave-64
// shuffle + LDS block sum, ONE fp32 partial per block - and the apply launch - grid (blocks, images), which adds its image's
// partials in slice order (no float atomics: bit-identical from run to run).  Without color: the apply launch alone, which then only
// moves data.  u is read and decoded on the device, so a captured graph replays with whatever the buffer holds.
//
// THE GATE (Karras et al. 2020, "ADA").  sp_augment_ingest_gated / sp_augment_ingest_bwd_gated take p_dev, one fp32
// value in device memory read when the kernel RUNS: image n is LIVE iff u[n * 8 + 7] < p_dev[0] (strict, fp32).  A live image gets what the
// ungated entry computes for it; a dead one gets bit for bit what sp_ingest_image / sp_ingest_image_bwd write with scale3 / shift3 NULL -
// no color arithmetic, no translation, no window ((b - m) * 1 + m is not the identity in fp32).  The same kernels serve both forms: the
// ungated entries pass p_dev = NULL (every image live), so p = 1 IS the ungated result and p = 0 the plain ingest.  A dead image's
// statistics blocks leave at once and write nothing; its apply blocks never read its partials.
// THE CONTROLLER.  sp_ada_observe counts D's predictions on the real images above and below a threshold into the 8-word state,
// sp_ada_adjust moves p by one step per full window from r = (pos - neg) / total; both are one block, integer counts (no order
// dependence), state read and written on the device - a captured graph holds the observe launch and follows p through the pointer.
//
// THE GEOMETRIC FAMILY (Karras et al. 2020: pixel blitting and general geometric transforms; include/sempyr.h
// repeats it).  x-flip, 90-degree rotations, isotropic scaling and arbitrary rotation compose with the translation into ONE 2 x 3 affine
// map per image.  A row v of 4 fp32 uniforms in [0, 1) joins u; geom = any OR of SP_GEOM_XFLIP 1 / ROT90 2 / SCALE 4 / ROTATE 8, a
// part left out is the identity and is not computed.  Decode (fp32):
//   flip = v0 < 0.5f;  k = min(int(floorf(4 v1)), 3);  e = 0.8f v2 - 0.4f, g = exp2f(-e) (magnification 2^e in [0.758, 1.32));
//   theta = (v3 - 0.5f) float(pi / 2), c = cosf(theta), s = sinf(theta) ([-45, 45) degrees: with rot90 the whole circle);
//   t_y, t_x from u3, u4 as above (0 without SP_AUG_TRANSLATION);  cy = (H - 1) / 2, cx = (W - 1) / 2.
// The INVERSE map takes an output pixel (h, w) to source coordinates (y, x) = L ((h, w) + (t_y, t_x) - (cy, cx)) + (cy, cx) with
//   L = F Q^k g [[c, -s], [s, c]], rows in (y, x) order, Q = [[0, 1], [-1, 0]] as exact row swaps and sign changes, F = diag(1, -1) if flip.
// Table row: {m00, m01, m02, m10, m11, m12, 0, 0}, (m00 m01; m10 m11) = L, (m02, m12) = L (t_y - cy, t_x - cx) + (cy, cx); a row
// without scale and rotate is EXACT (entries in {-1, 0, 1}).  rot90 needs H == W.
// Forward: y = (m00 h + m01 w) + m02, x likewise - products and sums rounded once each, never fused (geom_coord), so both passes get the
// same bits; y0 = floorf(y), fy = y - y0;  out = (1 - fy) ((1 - fx) e[y0, x0] + fx e[y0, x0 + 1]) + fy ((1 - fx) e[y0 + 1, x0] + fx
// e[y0 + 1, x0 + 1]) with e the color transform of the SOURCE evaluated at each tap (its mean M is still the one reduction of the raw
// input); a tap outside the frame contributes 0 (grid_sample bilinear / zeros / align_corners=True); then the cutout window zeroes its
// OUTPUT pixels.  Backward: g1[c, i, j] = sum over outputs (h, w) outside the window of omega(h, w -> i, j) dy[c, h, w], then the color
// backward unchanged.  It is a GATHER: for source pixel (i, j), q = L^-1 ((i, j) - (m02, m12)), and the contributing outputs lie within
// |h - round(q_y)| <= 2, |w - round(q_x)| <= 2 - the pre-image of the tap square (-1, 1)^2 under L^-1 = A has half-extent |a00| + |a01|
// <= 1.32 sqrt(2) = 1.87 per axis and rounding adds 0.5, so 2.37 < 3.  At most 25 candidates, each one's (y, x) recomputed by the
// forward's expression, summed in row-major order, the ranges cut with the frame BEFORE the loops: no index depends on the table's
// values (the forward compares floorf(y) with the frame as a float before it becomes an int).  The apply entries are specified for the
// tables the decode writes and for any table with |a00| + |a01| <= 2 and |a10| + |a11| <= 2, A the inverse of its linear part; any
// other table is safe but its backward may miss contributions.  sum(g1) for the color backward is taken over OUTPUT pixels outside the
// window, (dy_0 + dy_1 + dy_2) x (sum of the in-frame tap weights), partials in slice order as above.  The gate is unchanged.
// LAUNCHES: decode - one thread per image, n x 8 floats; apply forward - grid (blocks, images), one output pixel per thread in 16 x 16
// tiles (geom_tile_pixel), four taps x three channels from the strided source (a block's footprint is a patch of some 30 x 30 pixels
// that stays in L2; no LDS staging), one 16-byte padded store; backward - one source pixel per thread in the same tiles, up to 25
// 16-byte loads of padded dy pixels, L^-1 once per block.
//
// THE COLOR MATRIX (Karras et al. 2020: ADA's color group - brightness, contrast, luma flip, hue rotation, saturation; DESIGN.md section
// 20; include/sempyr.h repeats it).  ONE affine map of RGB per image: no reduction, no launch besides one decode per step, and the
// backward is the transposed 3 x 3 matrix.  Images are valued as the generator emits them (contrast and luma flip act about 0).  A row z
// of 8 fp32 uniforms in [0, 1) joins u and v; cmat = any OR of SP_CMAT_BRIGHTNESS 1 / CONTRAST 2 / LUMAFLIP 4 / HUE 8 / SATURATION 16, a
// part left out is the identity and is not computed.  Decode (fp32, every product and sum rounded once), with
//   nrm(a, b) = sqrtf(-2 * logf(1 - a)) * cosf(float(2 pi) * b)      (Box-Muller; 1 - a >= 2^-24, so |nrm| <= 5.77):
//   bb = 0.2f nrm(z0, z1) (else 0);  c = exp2f(0.5f nrm(z2, z3)) (else 1);  s = exp2f(nrm(z4, z5)) (else 1);
//   theta = (2 z6 - 1) float(pi), cs = cosf(theta), sn = sinf(theta) (else cs = 1, sn = 0 exactly);  f = z7 < 0.5f ? -1 : 1 (else 1).
// With P = J / 3 the projector on the grey axis (1, 1, 1) / sqrt 3, Q = I - P and K the cross-product matrix of that axis, ADA's five
// homogeneous matrices in its order (brightness, contrast, luma flip, hue as Rodrigues' rotation about the grey axis, saturation, each
// multiplied on the left) collapse to  out = Lm x + t (1, 1, 1),  Lm = c (f P + s cos(theta) Q + s sin(theta) K),  t = c f bb:
//   p = c f;  cs_ = c s;  beta = cs_ cs;  gamma = (cs_ sn) float(1 / sqrt 3);  d = (p - beta) / 3;
//   Lm_ii = beta + d;  Lm_01 = Lm_12 = Lm_20 = d - gamma;  Lm_02 = Lm_10 = Lm_21 = d + gamma;  t = p bb.
// Brightness and / or contrast alone is exactly diag(c) with offset c bb; luma flip alone is I - 2 J / 3 to rounding.
// Table row (the "ctable"): 12 floats {L00, L01, L02, t, L10, L11, L12, t, L20, L21, L22, t} - three 16-byte quadruples, row-major.
// Forward: the last step of the pointwise color stage e of the SOURCE pixel (after `color`, before translation / resampling / cutout):
//   e'_r = ((L_r0 e_0 + L_r1 e_1) + L_r2 e_2) + L_r3      (the compiler may contract it into FMAs)
// In the geometric family it is evaluated at each tap, as aug_color_fwd is: a tap outside the frame still contributes 0.  The apply
// entries take ANY 3 x 4 table.  Backward: after the family's g1,  g1'_c = (L_0c g1_0 + L_1c g1_1) + L_2c g1_2,  then the color backward
// unchanged on g1'.  Its statistics launch needs sum(g1') before g1 exists: per output pixel (k0 dy_0 + k1 dy_1) + k2 dy_2 with
// k_r = (L_r0 + L_r1) + L_r2, times the in-frame tap weights in the geometric family.  Without `color` the matrix adds no statistics
// launch in either direction.  The gate is unchanged: a dead image never reads its ctable row.
// LAUNCHES: cmat_decode_kernel - one thread per row, n x 12 floats; the apply and backward statistics kernels take `ctable`, NULL for the
// entries above (their bits are unchanged); with a table each block reads its image's 12 floats once as three 16-byte loads from a
// block-uniform address (wave-uniform: the compiler turns them into scalar loads, one of 32 and one of 16 bytes).  ctable must be 16-byte
// aligned.  float(1 / sqrt 3) above is the fp32 rounding of the closed form's constant; a float64 reference uses 1 / sqrt 3 itself.
#include "common.h"

namespace {

constexpr int AUG_FWD_SLICE = 8192;      // source elements (of the 3 H W of an image) per statistics block, forward
constexpr int AUG_BWD_SLICE = 2048;      // dy pixels per statistics block, backward
constexpr int AUG_APPLY_BLOCKS = 128;    // apply blocks per image at most (grid-stride beyond)

// what depends on the map size alone (host)
struct AugGeom { int H, W, ry, rx, qy, qx, ny, nx; };

inline AugGeom aug_geom(int h, int w) {
    AugGeom g;
    g.H = h; g.W = w;
    g.ry = (int)((float)h / 8.f + 0.5f); g.rx = (int)((float)w / 8.f + 0.5f);
    g.qy = (int)((float)h / 2.f + 0.5f); g.qx = (int)((float)w / 2.f + 0.5f);
    g.ny = h + 1 - (g.qy % 2); g.nx = w + 1 - (g.qx % 2);
    return g;
}

// one image's decoded row of u; the window is [y0, y1) x [x0, x1) in OUTPUT coordinates (empty without cutout)
struct AugImage { float o, s, k; int ty, tx, y0, y1, x0, x1; };

__device__ __forceinline__ AugImage aug_decode(const float* __restrict__ u, int policy, const AugGeom& g) {
    AugImage a;
    a.o = 0.f; a.s = 1.f; a.k = 1.f;
    a.ty = a.tx = 0;
    a.y0 = a.y1 = a.x0 = a.x1 = 0;
    if (policy & SP_AUG_COLOR) { a.o = u[0] - 0.5f; a.s = 2.f * u[1]; a.k = u[2] + 0.5f; }
    if (policy & SP_AUG_TRANSLATION) {
        a.ty = min((int)floorf(u[3] * (float)(2 * g.ry + 1)), 2 * g.ry) - g.ry;
        a.tx = min((int)floorf(u[4] * (float)(2 * g.rx + 1)), 2 * g.rx) - g.rx;
    }
    if (policy & SP_AUG_CUTOUT) {
        const int cy = min((int)floorf(u[5] * (float)g.ny), g.ny - 1);
        const int cx = min((int)floorf(u[6] * (float)g.nx), g.nx - 1);
        a.y0 = cy - g.qy / 2; a.y1 = a.y0 + g.qy;
        a.x0 = cx - g.qx / 2; a.x1 = a.x0 + g.qx;
    }
    return a;
}

// the cutout window holds output position (h, w)
__device__ __forceinline__ bool aug_in_window(const AugImage& a, int h, int w) { return h >= a.y0 && h < a.y1 && w >= a.x0 && w < a.x1; }

// output position (h, w) shows source pixel (h + ty, w + tx): false where that is outside the frame or (h, w) is in the window
__device__ __forceinline__ bool aug_live(const AugImage& a, const AugGeom& g, int h, int w) {
    const int hs = h + a.ty, ws = w + a.tx;
    return hs >= 0 && hs < g.H && ws >= 0 && ws < g.W && !aug_in_window(a, h, w);
}

// an image's partials, added in slice order by every thread alike (a handful of floats; the loads are wave-uniform)
__device__ __forceinline__ float aug_total(const float* __restrict__ partials, int n, int nsl) {
    float t = 0.f;
    for (int i = 0; i < nsl; ++i) t += partials[(long)n * nsl + i];
    return t;
}

template <typename T> struct Vec16 { static constexpr int N = 16 / (int)sizeof(T); };

// the gate: true where image n is transformed.  p_dev == NULL: the ungated entries (every image).  Strict fp32 compare; a NaN p is dead.
__device__ __forceinline__ bool aug_gate(const float* __restrict__ u, const float* __restrict__ p_dev, int n) {
    return p_dev == nullptr || u[(long)n * 8 + 7] < p_dev[0];
}

// one padded NHWC pixel: 3 values and CP - 3 zeros (one 16-byte store where the pitch is 16 bytes)
template <typename TD>
__device__ __forceinline__ void aug_st_padded(TD* __restrict__ d, int CP, const float (&e)[3]) {
    if (CP == 4) {
        const float v[4] = {e[0], e[1], e[2], 0.f};
        VecIO<TD, 4>::st(d, v);
    } else if (sizeof(TD) == 2 && CP == 8) {
        const float v[8] = {e[0], e[1], e[2], 0.f, 0.f, 0.f, 0.f, 0.f};
        VecIO<bf16, 8>::st(reinterpret_cast<bf16*>(d), v);
    } else {
        for (int c = 0; c < CP; ++c) Elem<TD>::st(d + c, c < 3 ? e[c] : 0.f);
    }
}

// a dead image, forward (both families): ingest_kernel's values (x * 1 + 0 with scale3 / shift3 NULL: x, and -0 becomes +0) through these
// kernels' stores - bit for bit what sp_ingest_image writes
template <typename TS, typename TD>
__device__ __forceinline__ void aug_dead_fwd(const TS* __restrict__ src, long sn, long sc, long sh, long sw, TD* __restrict__ dst, const AugGeom& g,
                                             int CP, int n) {
    const int HW = g.H * g.W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const int h = p / g.W, w = p - h * g.W;
        const TS* s = src + (long)n * sn + (long)h * sh + (long)w * sw;
        float e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = Elem<TS>::ld(s + c * sc) + 0.f;
        aug_st_padded(dst + ((long)n * HW + p) * CP, CP, e);
    }
}

// color of one source pixel, forward (both families); M: the contrast's mean (header comment)
__device__ __forceinline__ void aug_color_fwd(float (&e)[3], const AugImage& a, float M) {
    float b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = e[c] + a.o;
    const float m = (b[0] + b[1] + b[2]) / 3.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sat = (b[c] - m) * a.s + m;
        e[c] = (sat - M) * a.k + M;
    }
}

// the color matrix of one image (header comment: THE COLOR MATRIX): three rows {L_r0, L_r1, L_r2, t}
struct CMat { float4 r[3]; };

// block-uniform address: three 16-byte loads per block.  ctable == NULL (the entries without one): never applied, nothing is read.
__device__ __forceinline__ CMat cmat_load(const float* __restrict__ ctable, int n) {
    CMat m;
    if (ctable != nullptr) {
        const float4* t = reinterpret_cast<const float4*>(ctable + (long)n * 12);
        m.r[0] = t[0]; m.r[1] = t[1]; m.r[2] = t[2];
    } else {
        m.r[0] = make_float4(1.f, 0.f, 0.f, 0.f); m.r[1] = make_float4(0.f, 1.f, 0.f, 0.f); m.r[2] = make_float4(0.f, 0.f, 1.f, 0.f);
    }
    return m;
}

// e'_r = ((L_r0 e_0 + L_r1 e_1) + L_r2 e_2) + L_r3: the last step of a source pixel's color stage
__device__ __forceinline__ void cmat_fwd(float (&e)[3], const CMat& m) {
    const float e0 = e[0], e1 = e[1], e2 = e[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) e[r] = ((m.r[r].x * e0 + m.r[r].y * e1) + m.r[r].z * e2) + m.r[r].w;
}

// g1'_c = (L_0c g1_0 + L_1c g1_1) + L_2c g1_2: the transposed 3 x 3 matrix, in front of the color backward
__device__ __forceinline__ void cmat_bwd(float (&v)[3], const CMat& m) {
    const float g0 = v[0], g1 = v[1], g2 = v[2];
    v[0] = (m.r[0].x * g0 + m.r[1].x * g1) + m.r[2].x * g2;
    v[1] = (m.r[0].y * g0 + m.r[1].y * g1) + m.r[2].y * g2;
    v[2] = (m.r[0].z * g0 + m.r[1].z * g1) + m.r[2].z * g2;
}

// sum_c g1'_c of one output pixel's dy: (k0 dy_0 + k1 dy_1) + k2 dy_2, k_r = (L_r0 + L_r1) + L_r2
__device__ __forceinline__ float cmat_bwd_sum(const float (&v)[3], const CMat& m) {
    const float k0 = (m.r[0].x + m.r[0].y) + m.r[0].z, k1 = (m.r[1].x + m.r[1].y) + m.r[1].z, k2 = (m.r[2].x + m.r[2].y) + m.r[2].z;
    return (k0 * v[0] + k1 * v[1]) + k2 * v[2];
}

// ---- statistics, forward: partial sums of the raw source --------------------------------------------
// dense: the image's 3 H W elements are one contiguous, 16-byte aligned run (NCHW-contiguous or channels-last): 16-byte loads.
template <typename TS>
__global__ __launch_bounds__(256) void aug_stats_fwd_kernel(const TS* __restrict__ src, long sn, long sc, long sh, long sw, int H, int W,
                                                            int dense, float* __restrict__ partials, const float* __restrict__ u,
                                                            const float* __restrict__ p_dev) {
    __shared__ float red[4];
    constexpr int V = Vec16<TS>::N;
    const int n = blockIdx.y;
    if (!aug_gate(u, p_dev, n)) return;      // a dead image: nobody reads its partials (block-uniform)
    const long total = 3L * H * W;
    const long beg = (long)blockIdx.x * AUG_FWD_SLICE;
    const long end = beg + AUG_FWD_SLICE < total ? beg + AUG_FWD_SLICE : total;
    const TS* base = src + (long)n * sn;
    float acc = 0.f;
    if (dense) {
        const long nvec = (end - beg) / V;
        for (long i = threadIdx.x; i < nvec; i += 256) {
            float v[V];
            VecIO<TS, V>::ld(base + beg + i * V, v);
#pragma unroll
            for (int r = 0; r < V; ++r) acc += v[r];
        }
        for (long i = beg + nvec * V + threadIdx.x; i < end; i += 256) acc += Elem<TS>::ld(base + i);
    } else {
        const long HW = (long)H * W;
        for (long i = beg + threadIdx.x; i < end; i += 256) {
            const int c = (int)(i / HW);
            const int r = (int)(i - c * HW);
            const int h = r / W, w = r - h * W;
            acc += Elem<TS>::ld(base + c * sc + h * sh + w * sw);
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[(long)n * gridDim.x + blockIdx.x] = acc;
}

// ---- apply, forward: what ingest_kernel does, through the transform ----------------------------------
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void aug_apply_fwd_kernel(const TS* __restrict__ src, long sn, long sc, long sh, long sw,
                                                            TD* __restrict__ dst, AugGeom g, int CP, const float* __restrict__ u,
                                                            int policy, const float* __restrict__ ctable,
                                                            const float* __restrict__ partials, int nsl, const float* __restrict__ p_dev) {
    const int n = blockIdx.y;
    const int HW = g.H * g.W;
    if (!aug_gate(u, p_dev, n)) { aug_dead_fwd(src, sn, sc, sh, sw, dst, g, CP, n); return; }
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);
    const CMat cm = cmat_load(ctable, n);
    const bool color = (policy & SP_AUG_COLOR) != 0, cmat = ctable != nullptr;
    float M = 0.f;
    if (color) M = aug_total(partials, n, nsl) / (float)(3 * HW) + a.o;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const int h = p / g.W, w = p - h * g.W;
        float e[3] = {0.f, 0.f, 0.f};
        if (aug_live(a, g, h, w)) {
            const TS* s = src + (long)n * sn + (long)(h + a.ty) * sh + (long)(w + a.tx) * sw;
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = Elem<TS>::ld(s + c * sc);
            if (color) aug_color_fwd(e, a, M);
            if (cmat) cmat_fwd(e, cm);
        }
        aug_st_padded(dst + ((long)n * HW + p) * CP, CP, e);
    }
}

// the 3 real channels of one padded dy pixel (one 16-byte load where the pitch is 16 bytes)
template <typename T>
__device__ __forceinline__ void aug_ld3(const T* __restrict__ p, int CP, float (&v)[3]) {
    constexpr int V = Vec16<T>::N;
    if (CP == V) {
        float t[V];
        VecIO<T, V>::ld(p, t);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = Elem<T>::ld(p + c);
    }
}

// one gradient pixel of pitch 3, element by element as ingest_bwd_kernel stores it
template <typename T>
__device__ __forceinline__ void aug_st3(T* d, const float (&v)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Elem<T>::st(d + c, v[c]);
}

// a dead image, backward (both families): ingest_bwd_kernel's values (dy * 1 with scale3 NULL) - bit for bit what sp_ingest_image_bwd writes
template <typename T>
__device__ __forceinline__ void aug_dead_bwd(const T* __restrict__ dy, int CP, T* __restrict__ dsrc, const AugGeom& g, int n) {
    const int HW = g.H * g.W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        float v[3];
        aug_ld3(dy + ((long)n * HW + p) * CP, CP, v);
        aug_st3(dsrc + ((long)n * HW + p) * 3, v);
    }
}

// color of one source pixel, backward (both families): g1 -> dx; Gm = sum(g1) / (3 H W)
__device__ __forceinline__ void aug_color_bwd(float (&v)[3], const AugImage& a, float Gm) {
    float g2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g2[c] = a.k * v[c] + (1.f - a.k) * Gm;
    const float m = (g2[0] + g2[1] + g2[2]) / 3.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = a.s * g2[c] + (1.f - a.s) * m;
}

// ---- statistics, backward: partial sums of g1 = the dy values that reach an input pixel --------------
template <typename T>
__global__ __launch_bounds__(256) void aug_stats_bwd_kernel(const T* __restrict__ dy, int CP, AugGeom g, const float* __restrict__ u,
                                                            int policy, const float* __restrict__ ctable, float* __restrict__ partials,
                                                            const float* __restrict__ p_dev) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    if (!aug_gate(u, p_dev, n)) return;      // a dead image: nobody reads its partials (block-uniform)
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);
    const CMat cm = cmat_load(ctable, n);
    const bool cmat = ctable != nullptr;
    const int HW = g.H * g.W;
    const int beg = blockIdx.x * AUG_BWD_SLICE;
    const int end = beg + AUG_BWD_SLICE < HW ? beg + AUG_BWD_SLICE : HW;
    float acc = 0.f;
    for (int p = beg + threadIdx.x; p < end; p += 256) {
        const int h = p / g.W, w = p - h * g.W;
        if (aug_live(a, g, h, w)) {
            float v[3];
            aug_ld3(dy + ((long)n * HW + p) * CP, CP, v);
            acc += cmat ? cmat_bwd_sum(v, cm) : (v[0] + v[1]) + v[2];
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[(long)n * gridDim.x + blockIdx.x] = acc;
}

// ---- apply, backward: padded dy -> NHWC gradient of pitch 3 (what ingest_bwd_kernel writes) ------------
template <typename T>
__global__ __launch_bounds__(256) void aug_apply_bwd_kernel(const T* __restrict__ dy, int CP, T* __restrict__ dsrc, AugGeom g,
                                                            const float* __restrict__ u, int policy, const float* __restrict__ ctable,
                                                            const float* __restrict__ partials, int nsl, const float* __restrict__ p_dev) {
    const int n = blockIdx.y;
    const int HW = g.H * g.W;
    if (!aug_gate(u, p_dev, n)) { aug_dead_bwd(dy, CP, dsrc, g, n); return; }
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);
    const CMat cm = cmat_load(ctable, n);
    const bool color = (policy & SP_AUG_COLOR) != 0, cmat = ctable != nullptr;
    float Gm = 0.f;
    if (color) Gm = aug_total(partials, n, nsl) / (float)(3 * HW);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const int h = p / g.W, w = p - h * g.W;
        const int ho = h - a.ty, wo = w - a.tx;      // the output position that shows this input pixel
        float v[3] = {0.f, 0.f, 0.f};
        if (ho >= 0 && ho < g.H && wo >= 0 && wo < g.W && !aug_in_window(a, ho, wo))
            aug_ld3(dy + ((long)n * HW + (long)ho * g.W + wo) * CP, CP, v);
        if (cmat) cmat_bwd(v, cm);
        if (color) aug_color_bwd(v, a, Gm);
        aug_st3(dsrc + ((long)n * HW + p) * 3, v);
    }
}

inline int aug_slices(int h, int w, bool backward) {
    return backward ? sp_div_up((long)h * w, AUG_BWD_SLICE) : sp_div_up(3L * h * w, AUG_FWD_SLICE);
}
inline int aug_apply_blocks(int h, int w) {
    const int b = sp_div_up((long)h * w, 256);
    return b < AUG_APPLY_BLOCKS ? b : AUG_APPLY_BLOCKS;
}
// 3 H W <= 2^24: float(3 H W) is exact, and pixel indices fit an int with room to spare
inline bool aug_dims_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && 3L * h * w <= (1L << 24); }

// ---- the geometric family: one 2 x 3 affine map per image, bilinear taps (header comment: THE GEOMETRIC FAMILY) ----------------------
struct GeomMap { float m00, m01, m02, m10, m11, m12; };

__device__ __forceinline__ GeomMap geom_map(const float* __restrict__ table, int n) {
    const float* t = table + (long)n * 8;
    GeomMap m;
    m.m00 = t[0]; m.m01 = t[1]; m.m02 = t[2]; m.m10 = t[3]; m.m11 = t[4]; m.m12 = t[5];
    return m;
}

// (m0 h + m1 w) + m2 with every product and sum rounded once: no contraction, so the forward and the backward kernel (and the decode's
// offsets, which use the same form) get the SAME bits from the same operands
__device__ __forceinline__ float geom_coord(float m0, float m1, float m2, float h, float w) {
    return __fadd_rn(__fadd_rn(__fmul_rn(m0, h), __fmul_rn(m1, w)), m2);
}

// one axis of a bilinear sample at coordinate y: taps i0 and i0 + 1 with weights w0 = 1 - f and w1 = f; in0 / in1: that tap is inside
// [0, size).  y0 is compared as a float BEFORE it becomes an int: a coordinate far outside the frame (or NaN) never becomes an index.
struct GeomAxis { int i0; float w0, w1; bool in0, in1; };

__device__ __forceinline__ GeomAxis geom_axis(float y, int size) {
    GeomAxis a;
    const float y0 = floorf(y);
    const float f = __fsub_rn(y, y0);
    const bool near = y0 >= -1.f && y0 <= (float)(size - 1);
    a.i0 = near ? (int)y0 : -2;
    a.w0 = __fsub_rn(1.f, f);
    a.w1 = f;
    a.in0 = near && a.i0 >= 0;
    a.in1 = near && a.i0 + 1 < size;
    return a;
}

// The apply kernels walk the map in tiles of 16 x 16 pixels, one per block and trip, each wave an 8 x 8 quarter: under a rotation a
// wave's taps then fall into ~11 source rows (8 at 0 degrees, the same after a rot90) where 64 pixels of one output row would fall
// into up to 64.  false: the pixel lies outside the map (a partial tile).
__device__ __forceinline__ bool geom_tile_pixel(int t, int tiles_w, const AugGeom& g, int& h, int& w) {
    const int th = t / tiles_w, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    h = th * 16 + (q >> 1) * 8 + (lane >> 3);
    w = (t - th * tiles_w) * 16 + (q & 1) * 8 + (lane & 7);
    return h < g.H && w < g.W;
}

// decode: one thread per image, n x 8 floats.  Without scale and rotate the linear part is never multiplied: entries in {-1, 0, 1}.
__global__ __launch_bounds__(64) void geom_decode_kernel(const float* __restrict__ u, const float* __restrict__ v, int n, AugGeom g, int policy,
                                                         int geom, float* __restrict__ table) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* vi = v + (long)i * 4;
    float a00 = 1.f, a01 = 0.f, a10 = 0.f, a11 = 1.f;
    if (geom & (SP_GEOM_SCALE | SP_GEOM_ROTATE)) {
        float gs = 1.f, c = 1.f, s = 0.f;
        if (geom & SP_GEOM_SCALE) gs = exp2f(-__fsub_rn(__fmul_rn(0.8f, vi[2]), 0.4f));
        if (geom & SP_GEOM_ROTATE) {
            const float theta = __fmul_rn(__fsub_rn(vi[3], 0.5f), 1.57079632679489661923f);
            c = cosf(theta);
            s = sinf(theta);
        }
        a00 = __fmul_rn(gs, c); a01 = -__fmul_rn(gs, s); a10 = __fmul_rn(gs, s); a11 = __fmul_rn(gs, c);
    }
    if (geom & SP_GEOM_ROT90) {
        const int k = min((int)floorf(__fmul_rn(4.f, vi[1])), 3);
        for (int r = 0; r < k; ++r) {          // Q . A: the rows swap, the new second row changes sign
            const float b0 = a00, b1 = a01;
            a00 = a10; a01 = a11; a10 = -b0; a11 = -b1;
        }
    }
    if ((geom & SP_GEOM_XFLIP) && vi[0] < 0.5f) { a10 = -a10; a11 = -a11; }
    const AugImage t = aug_decode(u + (long)i * 8, policy & SP_AUG_TRANSLATION, g);
    const float cy = (float)(g.H - 1) * 0.5f, cx = (float)(g.W - 1) * 0.5f;
    const float dy = (float)t.ty - cy, dx = (float)t.tx - cx;          // half-integers: exact
    float* row = table + (long)i * 8;
    row[0] = a00; row[1] = a01; row[2] = geom_coord(a00, a01, cy, dy, dx);
    row[3] = a10; row[4] = a11; row[5] = geom_coord(a10, a11, cx, dy, dx);
    row[6] = 0.f; row[7] = 0.f;
}

// ---- apply, forward: one output pixel per thread, four taps x three channels from the strided source, color per tap -------------------
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void geom_apply_fwd_kernel(const TS* __restrict__ src, long sn, long sc, long sh, long sw,
                                                             TD* __restrict__ dst, AugGeom g, int CP, const float* __restrict__ u,
                                                             int policy, const float* __restrict__ table, const float* __restrict__ ctable,
                                                             const float* __restrict__ partials, int nsl, const float* __restrict__ p_dev) {
    const int n = blockIdx.y;
    const int HW = g.H * g.W;
    const TS* base = src + (long)n * sn;
    if (!aug_gate(u, p_dev, n)) { aug_dead_fwd(src, sn, sc, sh, sw, dst, g, CP, n); return; }
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);          // color and cutout only: the entry masks the translation out
    const GeomMap m = geom_map(table, n);
    const CMat cm = cmat_load(ctable, n);
    const bool color = (policy & SP_AUG_COLOR) != 0, cmat = ctable != nullptr;
    float M = 0.f;
    if (color) M = aug_total(partials, n, nsl) / (float)(3 * HW) + a.o;
    const int tiles_w = (g.W + 15) >> 4, tiles = ((g.H + 15) >> 4) * tiles_w;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        int h, w;
        if (!geom_tile_pixel(t, tiles_w, g, h, w)) continue;
        const int p = h * g.W + w;
        float e[3] = {0.f, 0.f, 0.f};
        if (!aug_in_window(a, h, w)) {
            const float hf = (float)h, wf = (float)w;
            const GeomAxis ay = geom_axis(geom_coord(m.m00, m.m01, m.m02, hf, wf), g.H);
            const GeomAxis ax = geom_axis(geom_coord(m.m10, m.m11, m.m12, hf, wf), g.W);
            float t[2][2][3];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    t[r][q][0] = t[r][q][1] = t[r][q][2] = 0.f;
                    if ((r ? ay.in1 : ay.in0) && (q ? ax.in1 : ax.in0)) {          // a tap outside the frame contributes 0
                        const TS* s = base + (long)(ay.i0 + r) * sh + (long)(ax.i0 + q) * sw;
#pragma unroll
                        for (int c = 0; c < 3; ++c) t[r][q][c] = Elem<TS>::ld(s + c * sc);
                        if (color) aug_color_fwd(t[r][q], a, M);
                        if (cmat) cmat_fwd(t[r][q], cm);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                e[c] = ay.w0 * (ax.w0 * t[0][0][c] + ax.w1 * t[0][1][c]) + ay.w1 * (ax.w0 * t[1][0][c] + ax.w1 * t[1][1][c]);
        }
        aug_st_padded(dst + ((long)n * HW + p) * CP, CP, e);
    }
}

// ---- statistics, backward: sum(g1) taken over OUTPUT pixels: (dy_0 + dy_1 + dy_2) x (sum of the in-frame tap weights) ----------------
template <typename T>
__global__ __launch_bounds__(256) void geom_stats_bwd_kernel(const T* __restrict__ dy, int CP, AugGeom g, const float* __restrict__ u,
                                                             int policy, const float* __restrict__ table, const float* __restrict__ ctable,
                                                             float* __restrict__ partials, const float* __restrict__ p_dev) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    if (!aug_gate(u, p_dev, n)) return;      // a dead image: nobody reads its partials (block-uniform)
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);
    const GeomMap m = geom_map(table, n);
    const CMat cm = cmat_load(ctable, n);
    const bool cmat = ctable != nullptr;
    const int HW = g.H * g.W;
    const int beg = blockIdx.x * AUG_BWD_SLICE;
    const int end = beg + AUG_BWD_SLICE < HW ? beg + AUG_BWD_SLICE : HW;
    float acc = 0.f;
    for (int p = beg + threadIdx.x; p < end; p += 256) {
        const int h = p / g.W, w = p - h * g.W;
        if (aug_in_window(a, h, w)) continue;
        const float hf = (float)h, wf = (float)w;
        const GeomAxis ay = geom_axis(geom_coord(m.m00, m.m01, m.m02, hf, wf), g.H);
        const GeomAxis ax = geom_axis(geom_coord(m.m10, m.m11, m.m12, hf, wf), g.W);
        if ((ay.in0 || ay.in1) && (ax.in0 || ax.in1)) {
            const float wy = (ay.in0 ? ay.w0 : 0.f) + (ay.in1 ? ay.w1 : 0.f);
            const float wx = (ax.in0 ? ax.w0 : 0.f) + (ax.in1 ? ax.w1 : 0.f);
            float v[3];
            aug_ld3(dy + ((long)n * HW + p) * CP, CP, v);
            acc += (cmat ? cmat_bwd_sum(v, cm) : (v[0] + v[1]) + v[2]) * (wy * wx);
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[(long)n * gridDim.x + blockIdx.x] = acc;
}

// ---- apply, backward: the adjoint by GATHER.  One source pixel per thread; the outputs that can reach it lie within 2 of
// round(L^-1 ((i, j) - (m02, m12))) on each axis (header comment: the box), at most 25 padded dy pixels, row-major order ---------------
template <typename T>
__global__ __launch_bounds__(256) void geom_apply_bwd_kernel(const T* __restrict__ dy, int CP, T* __restrict__ dsrc, AugGeom g,
                                                             const float* __restrict__ u, int policy, const float* __restrict__ table,
                                                             const float* __restrict__ ctable, const float* __restrict__ partials, int nsl,
                                                             const float* __restrict__ p_dev) {
    __shared__ float inv[4];
    const int n = blockIdx.y;
    const int HW = g.H * g.W;
    if (!aug_gate(u, p_dev, n)) { aug_dead_bwd(dy, CP, dsrc, g, n); return; }      // (block-uniform: no thread of a dead image's block reaches the barrier below)
    const AugImage a = aug_decode(u + (long)n * 8, policy, g);
    const GeomMap m = geom_map(table, n);
    if (threadIdx.x == 0) {                  // the image's L^-1, once per block
        const float r = 1.f / (m.m00 * m.m11 - m.m01 * m.m10);
        inv[0] = m.m11 * r; inv[1] = -m.m01 * r; inv[2] = -m.m10 * r; inv[3] = m.m00 * r;
    }
    __syncthreads();
    const CMat cm = cmat_load(ctable, n);
    const bool color = (policy & SP_AUG_COLOR) != 0, cmat = ctable != nullptr;
    float Gm = 0.f;
    if (color) Gm = aug_total(partials, n, nsl) / (float)(3 * HW);
    const int tiles_w = (g.W + 15) >> 4, tiles = ((g.H + 15) >> 4) * tiles_w;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        int i, j;
        if (!geom_tile_pixel(t, tiles_w, g, i, j)) continue;
        const int p = i * g.W + j;
        const float fi = (float)i, fj = (float)j;
        const float di = fi - m.m02, dj = fj - m.m12;
        // the box's centre, clipped as a FLOAT (fmaxf / fminf drop a NaN), then the ranges cut with the frame: from here on no index
        // depends on the table's values
        const int hc = (int)fminf(fmaxf(rintf(inv[0] * di + inv[1] * dj), -3.f), (float)(g.H + 2));
        const int wc = (int)fminf(fmaxf(rintf(inv[2] * di + inv[3] * dj), -3.f), (float)(g.W + 2));
        const int h_lo = max(hc - 2, 0), h_hi = min(hc + 2, g.H - 1);
        const int w_lo = max(wc - 2, 0), w_hi = min(wc + 2, g.W - 1);
        float v[3] = {0.f, 0.f, 0.f};
        for (int h = h_lo; h <= h_hi; ++h) {
            for (int w = w_lo; w <= w_hi; ++w) {
                if (aug_in_window(a, h, w)) continue;
                const float hf = (float)h, wf = (float)w;
                const float y = geom_coord(m.m00, m.m01, m.m02, hf, wf);          // the forward's expression: the forward's weights
                const float y0 = floorf(y);
                const bool r0 = y0 == fi, r1 = y0 + 1.f == fi;
                if (!(r0 || r1)) continue;
                const float x = geom_coord(m.m10, m.m11, m.m12, hf, wf);
                const float x0 = floorf(x);
                const bool q0 = x0 == fj, q1 = x0 + 1.f == fj;
                if (!(q0 || q1)) continue;
                const float fy = __fsub_rn(y, y0), fx = __fsub_rn(x, x0);
                const float wgt = (r0 ? __fsub_rn(1.f, fy) : fy) * (q0 ? __fsub_rn(1.f, fx) : fx);
                float d[3];
                aug_ld3(dy + ((long)n * HW + (long)h * g.W + w) * CP, CP, d);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] += wgt * d[c];
            }
        }
        if (cmat) cmat_bwd(v, cm);
        if (color) aug_color_bwd(v, a, Gm);
        aug_st3(dsrc + ((long)n * HW + p) * 3, v);
    }
}

// ---- the color matrix's decode: one thread per row of z, n x 12 floats (header comment: THE COLOR MATRIX) -----------------------------
// Box-Muller: |nrm| <= sqrt(-2 log 2^-24) = 5.77
__device__ __forceinline__ float cmat_nrm(float a, float b) {
    return __fmul_rn(__fsqrt_rn(__fmul_rn(-2.f, logf(__fsub_rn(1.f, a)))), cosf(__fmul_rn(6.28318530717958647692f, b)));
}

__global__ __launch_bounds__(64) void cmat_decode_kernel(const float* __restrict__ z, int n, int cmat, float* __restrict__ ctable) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* zi = z + (long)i * 8;
    float bb = 0.f, c = 1.f, s = 1.f, cs = 1.f, sn = 0.f, f = 1.f;
    if (cmat & SP_CMAT_BRIGHTNESS) bb = __fmul_rn(0.2f, cmat_nrm(zi[0], zi[1]));
    if (cmat & SP_CMAT_CONTRAST) c = exp2f(__fmul_rn(0.5f, cmat_nrm(zi[2], zi[3])));
    if (cmat & SP_CMAT_SATURATION) s = exp2f(cmat_nrm(zi[4], zi[5]));
    if (cmat & SP_CMAT_HUE) {
        const float theta = __fmul_rn(__fsub_rn(__fmul_rn(2.f, zi[6]), 1.f), 3.14159265358979323846f);
        cs = cosf(theta);
        sn = sinf(theta);
    }
    if ((cmat & SP_CMAT_LUMAFLIP) && zi[7] < 0.5f) f = -1.f;
    const float p = __fmul_rn(c, f), cs_ = __fmul_rn(c, s);
    const float beta = __fmul_rn(cs_, cs), gamma = __fmul_rn(__fmul_rn(cs_, sn), 0.57735026918962576451f);
    const float d = __fdiv_rn(__fsub_rn(p, beta), 3.f);
    const float di = __fadd_rn(beta, d), lo = __fsub_rn(d, gamma), hi = __fadd_rn(d, gamma), t = __fmul_rn(p, bb);
    float4* row = reinterpret_cast<float4*>(ctable + (long)i * 12);
    row[0] = make_float4(di, lo, hi, t);
    row[1] = make_float4(hi, di, lo, t);
    row[2] = make_float4(lo, hi, di, t);
}

inline int geom_apply_blocks(int h, int w) {          // one block per 16 x 16 tile, AUG_APPLY_BLOCKS at most (the kernels stride beyond)
    const int b = ((h + 15) >> 4) * ((w + 15) >> 4);
    return b < AUG_APPLY_BLOCKS ? b : AUG_APPLY_BLOCKS;
}

// ---- the host side: ONE checked call path for the three entry families (plain, gated, geometric) ----------------------------------------
// What an extern "C" entry was given.  Forward: src -> dst with the source's strides.  Backward: src = dy, dst = dsrc, src_dtype = dtype,
// no strides.  geom: a geometric entry, which resamples through `table`; ctable: NULL, or the color matrices of the sp_augment_cmat_*
// entries (which then also choose the family: geom = table non-NULL); p_dev NULL: every image is live.
struct AugCall {
    const char* name;
    const void* src; int32_t src_dtype; int64_t sn, sc, sh, sw;
    void* dst;
    int32_t n, h, w, cp;
    const float* u; int32_t policy;
    bool geom; const float* table; const float* ctable;
    float* partials; const float* p_dev;
    int32_t dtype; sp_stream_t stream;
};

// forward: with color the statistics launch (the mean of the RAW input, whatever the family), then the plain or the geometric apply launch
template <typename TS, typename TD>
void aug_launch_fwd(const AugCall& c, const AugGeom& g) {
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    const TS* src = (const TS*)c.src;
    int nsl = 0;
    if (c.policy & SP_AUG_COLOR) {
        nsl = aug_slices(g.H, g.W, false);
        const bool run = (c.sw == 1 && c.sh == g.W && c.sc == (long)g.H * g.W) || (c.sc == 1 && c.sw == 3 && c.sh == 3L * g.W);
        const int dense = run && reinterpret_cast<uintptr_t>(c.src) % 16 == 0 && (c.sn * (long)sizeof(TS)) % 16 == 0;
        hipLaunchKernelGGL(aug_stats_fwd_kernel<TS>, dim3(nsl, c.n), dim3(256), 0, s, src, c.sn, c.sc, c.sh, c.sw, g.H, g.W, dense, c.partials, c.u, c.p_dev);
    }
    if (c.geom) {
        hipLaunchKernelGGL((geom_apply_fwd_kernel<TS, TD>), dim3(geom_apply_blocks(g.H, g.W), c.n), dim3(256), 0, s, src, c.sn, c.sc, c.sh, c.sw,
                           (TD*)c.dst, g, c.cp, c.u, c.policy, c.table, c.ctable, c.partials, nsl, c.p_dev);
    } else {
        hipLaunchKernelGGL((aug_apply_fwd_kernel<TS, TD>), dim3(aug_apply_blocks(g.H, g.W), c.n), dim3(256), 0, s, src, c.sn, c.sc, c.sh, c.sw,
                           (TD*)c.dst, g, c.cp, c.u, c.policy, c.ctable, c.partials, nsl, c.p_dev);
    }
}

// backward: the family's statistics launch (the geometric one weighs dy by its taps), then its apply launch
template <typename T>
void aug_launch_bwd(const AugCall& c, const AugGeom& g) {
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    const T* dy = (const T*)c.src;
    int nsl = 0;
    if (c.policy & SP_AUG_COLOR) {
        nsl = aug_slices(g.H, g.W, true);
        if (c.geom) {
            hipLaunchKernelGGL(geom_stats_bwd_kernel<T>, dim3(nsl, c.n), dim3(256), 0, s, dy, c.cp, g, c.u, c.policy, c.table, c.ctable, c.partials, c.p_dev);
        } else {
            hipLaunchKernelGGL(aug_stats_bwd_kernel<T>, dim3(nsl, c.n), dim3(256), 0, s, dy, c.cp, g, c.u, c.policy, c.ctable, c.partials, c.p_dev);
        }
    }
    if (c.geom) {
        hipLaunchKernelGGL(geom_apply_bwd_kernel<T>, dim3(geom_apply_blocks(g.H, g.W), c.n), dim3(256), 0, s, dy, c.cp, (T*)c.dst, g, c.u, c.policy,
                           c.table, c.ctable, c.partials, nsl, c.p_dev);
    } else {
        hipLaunchKernelGGL(aug_apply_bwd_kernel<T>, dim3(aug_apply_blocks(g.H, g.W), c.n), dim3(256), 0, s, dy, c.cp, (T*)c.dst, g, c.u, c.policy,
                           c.ctable, c.partials, nsl, c.p_dev);
    }
}

// every ingest entry's body: the checks, their messages under the entry's own name, then the launches of its direction
int aug_run(AugCall c, bool backward) {
    SP_CHECK_ARG(c.src && c.dst && c.u && (c.table || !c.geom) && c.cp >= 3, "%s: bad args", c.name);
    SP_CHECK_ARG(aug_dims_ok(c.n, c.h, c.w), "%s: n=%d h=%d w=%d (need 3*h*w <= 2^24, n <= 65535)", c.name, c.n, c.h, c.w);
    SP_CHECK_ARG((c.src_dtype == SP_F32 || c.src_dtype == SP_BF16) && (c.dtype == SP_F32 || c.dtype == SP_BF16), "%s: bad dtype", c.name);
    SP_CHECK_ARG(c.policy >= 0 && c.policy <= 7, "%s: bad policy %d", c.name, c.policy);
    SP_CHECK_ARG(c.partials || !(c.policy & SP_AUG_COLOR), "%s: the color policy needs the partials buffer", c.name);
    if (c.geom) c.policy &= SP_AUG_COLOR | SP_AUG_CUTOUT;          // the translation is in the table
    const AugGeom g = aug_geom(c.h, c.w);
    const bool s32 = c.src_dtype == SP_F32, d32 = c.dtype == SP_F32;
    if (backward) {
        if (d32) aug_launch_bwd<float>(c, g);
        else aug_launch_bwd<bf16>(c, g);
    } else if (s32) {
        if (d32) aug_launch_fwd<float, float>(c, g);
        else aug_launch_fwd<float, bf16>(c, g);
    } else {
        if (d32) aug_launch_fwd<bf16, float>(c, g);
        else aug_launch_fwd<bf16, bf16>(c, g);
    }
    SP_LAUNCH_CHECK();
    return SP_OK;
}

// sp_augment_slices and sp_augment_geom_slices: the partials of both families have one size
int aug_slices_entry(const char* name, int32_t h, int32_t w_, int32_t backward, int64_t* slices_out) {
    SP_CHECK_ARG(slices_out && aug_dims_ok(1, h, w_), "%s: bad args (h=%d w=%d)", name, h, w_);
    *slices_out = aug_slices(h, w_, backward != 0);
    return SP_OK;
}

// ---- the gate's controller: 8 words of state {p, r_last, pos, neg, total, steps, adjustments, reserved} ----------------------
// ONE block of 1024 threads: integer counts, so the result does not depend on any order.  Eight independent 16-byte loads per thread
// and trip where pred is 16-byte aligned (a single dependent load per trip took 15 us for D's 51 200 predictions); a slot past the end
// holds the threshold itself, which counts on neither side.
__global__ __launch_bounds__(1024) void ada_observe_kernel(const float* __restrict__ pred, int numel, float threshold, int* __restrict__ state) {
    __shared__ int cnt[2][16];
    constexpr int U = 8;
    int pos = 0, neg = 0;
    const int n4 = (reinterpret_cast<uintptr_t>(pred) & 15) == 0 ? numel / 4 : 0;
    const float4* p4 = reinterpret_cast<const float4*>(pred);
    for (int base = 0; base < n4; base += U * 1024) {
        float4 v[U];
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const int i = base + r * 1024 + (int)threadIdx.x;
            v[r] = i < n4 ? p4[i] : make_float4(threshold, threshold, threshold, threshold);
        }
#pragma unroll
        for (int r = 0; r < U; ++r) {
            pos += (v[r].x > threshold) + (v[r].y > threshold) + (v[r].z > threshold) + (v[r].w > threshold);
            neg += (v[r].x < threshold) + (v[r].y < threshold) + (v[r].z < threshold) + (v[r].w < threshold);
        }
    }
    for (int i = n4 * 4 + threadIdx.x; i < numel; i += 1024) {
        const float x = pred[i];
        pos += x > threshold ? 1 : 0;      // equal values and NaN: neither
        neg += x < threshold ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o, 64); neg += __shfl_xor(neg, o, 64); }
    if ((threadIdx.x & 63) == 0) { cnt[0][threadIdx.x >> 6] = pos; cnt[1][threadIdx.x >> 6] = neg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tp = 0, tn = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { tp += cnt[0][k]; tn += cnt[1][k]; }
        state[2] += tp;
        state[3] += tn;
        state[4] += numel;
    }
}

__global__ void ada_adjust_kernel(int* __restrict__ state, int interval, float target, float step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float* f = reinterpret_cast<float*>(state);
    const int steps = state[5] + 1;
    if (steps < interval) { state[5] = steps; return; }
    state[5] = 0;
    const int total = state[4];
    if (total <= 0) return;                // a full window without an observation: only the step count starts again
    const float r = __fdiv_rn(__int2float_rn(state[2] - state[3]), __int2float_rn(total));
    const float d = r > target ? step : (r < target ? -step : 0.f);
    f[0] = fminf(1.f, fmaxf(0.f, __fadd_rn(f[0], d)));
    f[1] = r;
    state[2] = 0; state[3] = 0; state[4] = 0;
    state[6] += 1;
}

}  // namespace

extern "C" int sp_augment_slices(int32_t h, int32_t w_, int32_t backward, int64_t* slices_out) {
    return aug_slices_entry("sp_augment_slices", h, w_, backward, slices_out);
}

extern "C" int sp_augment_geom_slices(int32_t h, int32_t w_, int32_t backward, int64_t* slices_out) {
    return aug_slices_entry("sp_augment_geom_slices", h, w_, backward, slices_out);
}

extern "C" int sp_augment_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                                 int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, float* partials,
                                 int32_t dtype, sp_stream_t stream) {
    return aug_run({"sp_augment_ingest", src, src_dtype, sn, sc, sh, sw, dst, n, h, w_, cp, u, policy, false, nullptr, nullptr, partials, nullptr, dtype, stream}, false);
}

extern "C" int sp_augment_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                                     int32_t policy, float* partials, int32_t dtype, sp_stream_t stream) {
    return aug_run({"sp_augment_ingest_bwd", dy, dtype, 0, 0, 0, 0, dsrc, n, h, w_, cp, u, policy, false, nullptr, nullptr, partials, nullptr, dtype, stream}, true);
}

extern "C" int sp_augment_ingest_gated(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                                       int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, float* partials,
                                       const float* p_dev, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(p_dev, "sp_augment_ingest_gated: p_dev is NULL (the ungated entry is sp_augment_ingest)");
    return aug_run({"sp_augment_ingest_gated", src, src_dtype, sn, sc, sh, sw, dst, n, h, w_, cp, u, policy, false, nullptr, nullptr, partials, p_dev, dtype, stream}, false);
}

extern "C" int sp_augment_ingest_bwd_gated(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                                           int32_t policy, float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(p_dev, "sp_augment_ingest_bwd_gated: p_dev is NULL (the ungated entry is sp_augment_ingest_bwd)");
    return aug_run({"sp_augment_ingest_bwd_gated", dy, dtype, 0, 0, 0, 0, dsrc, n, h, w_, cp, u, policy, false, nullptr, nullptr, partials, p_dev, dtype, stream}, true);
}

extern "C" int sp_augment_geom_decode(const float* u, const float* v, int32_t n, int32_t h, int32_t w_, int32_t policy, int32_t geom,
                                      float* table, sp_stream_t stream) {
    SP_CHECK_ARG(u && v && table, "sp_augment_geom_decode: bad args");
    SP_CHECK_ARG(aug_dims_ok(1, h, w_) && n >= 1 && n <= (1 << 24), "sp_augment_geom_decode: n=%d h=%d w=%d (need 3*h*w <= 2^24, n <= 2^24)", n, h, w_);
    SP_CHECK_ARG(policy >= 0 && policy <= 7, "sp_augment_geom_decode: bad policy %d", policy);
    SP_CHECK_ARG(geom >= 1 && geom <= 15, "sp_augment_geom_decode: bad geom %d (an OR of xflip 1, rot90 2, scale 4, rotate 8)", geom);
    SP_CHECK_ARG(!(geom & SP_GEOM_ROT90) || h == w_, "sp_augment_geom_decode: rot90 needs a square map (h=%d w=%d)", h, w_);
    hipLaunchKernelGGL(geom_decode_kernel, dim3(sp_div_up((long)n, 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), u, v, n, aug_geom(h, w_),
                       policy, geom, table);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_augment_geom_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                                      int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, const float* table,
                                      float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream) {
    return aug_run({"sp_augment_geom_ingest", src, src_dtype, sn, sc, sh, sw, dst, n, h, w_, cp, u, policy, true, table, nullptr, partials, p_dev, dtype, stream}, false);
}

extern "C" int sp_augment_geom_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                                          int32_t policy, const float* table, float* partials, const float* p_dev, int32_t dtype,
                                          sp_stream_t stream) {
    return aug_run({"sp_augment_geom_ingest_bwd", dy, dtype, 0, 0, 0, 0, dsrc, n, h, w_, cp, u, policy, true, table, nullptr, partials, p_dev, dtype, stream}, true);
}

extern "C" int sp_augment_cmat_decode(const float* z, int32_t n, int32_t cmat, float* ctable, sp_stream_t stream) {
    SP_CHECK_ARG(z && ctable && reinterpret_cast<uintptr_t>(ctable) % 16 == 0, "sp_augment_cmat_decode: bad args (z, ctable non-NULL, ctable 16-byte aligned)");
    SP_CHECK_ARG(n >= 1 && n <= (1 << 24), "sp_augment_cmat_decode: n=%d (need 1 ... 2^24)", n);
    SP_CHECK_ARG(cmat >= 1 && cmat <= 31, "sp_augment_cmat_decode: bad cmat %d (an OR of brightness 1, contrast 2, lumaflip 4, hue 8, saturation 16)", cmat);
    hipLaunchKernelGGL(cmat_decode_kernel, dim3(sp_div_up((long)n, 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), z, n, cmat, ctable);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_augment_cmat_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                                      int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, const float* table,
                                      const float* ctable, float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(ctable && reinterpret_cast<uintptr_t>(ctable) % 16 == 0, "sp_augment_cmat_ingest: ctable is NULL or not 16-byte aligned");
    return aug_run({"sp_augment_cmat_ingest", src, src_dtype, sn, sc, sh, sw, dst, n, h, w_, cp, u, policy, table != nullptr, table, ctable, partials, p_dev,
                    dtype, stream}, false);
}

extern "C" int sp_augment_cmat_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                                          int32_t policy, const float* table, const float* ctable, float* partials, const float* p_dev,
                                          int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(ctable && reinterpret_cast<uintptr_t>(ctable) % 16 == 0, "sp_augment_cmat_ingest_bwd: ctable is NULL or not 16-byte aligned");
    return aug_run({"sp_augment_cmat_ingest_bwd", dy, dtype, 0, 0, 0, 0, dsrc, n, h, w_, cp, u, policy, table != nullptr, table, ctable, partials, p_dev,
                    dtype, stream}, true);
}

extern "C" int sp_ada_observe(const float* pred, int64_t numel, float threshold, void* state, sp_stream_t stream) {
    SP_CHECK_ARG(pred && state, "sp_ada_observe: bad args");
    SP_CHECK_ARG(numel >= 1 && numel <= (1L << 24), "sp_ada_observe: numel=%ld (need 1 ... 2^24)", (long)numel);
    hipLaunchKernelGGL(ada_observe_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), pred, (int)numel, threshold, (int*)state);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_ada_adjust(void* state, int32_t interval, float target, float step, sp_stream_t stream) {
    SP_CHECK_ARG(state && interval >= 1, "sp_ada_adjust: bad args (interval=%d)", interval);
    SP_CHECK_ARG(step >= 0.f && step <= 1.f && target >= -1.f && target <= 1.f, "sp_ada_adjust: step=%g target=%g (need step in [0, 1], target in [-1, 1])",
                 (double)step, (double)target);
    hipLaunchKernelGGL(ada_adjust_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (int*)state, interval, target, step);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
