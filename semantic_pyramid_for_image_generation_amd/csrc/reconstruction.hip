// Reconstruction fidelity of an image pair: the sufficient statistics of PSNR, SSIM (Wang et al. 2004) and MS-SSIM (Wang et al. 2003).
// include/sempyr.h has the definition (sp_ssim_stats), DESIGN.md section 23 the design and the error bound.
//
// The sources come with element strides and a dtype of their own (fp32, bf16 or fp16); a 16-bit value is widened from its BIT PATTERN
// (bf16: the upper half of an fp32; fp16: the compiler's _Float16), so this file is compiled ONCE, as metrics.hip.  fp32 arithmetic.
//
//   grid        one launch per scale, a flat grid of P * T blocks of 256 threads: block b owns tile b % T of plane b / T, a tile being
//               TH x TW = 16 x 32 window positions.  A last launch of one thread per (plane, scale) adds the blocks' partial sums.
//   stage       the tile's (TH + 10) x (TW + 10) pixels of BOTH images go to LDS as fp32 (zeros past the plane: they feed only
//               positions that are masked out).  Each pixel of the stage is loaded by exactly one thread.
//   ownership   a block owns the pixels [r0, r0 + TH) x [c0, c0 + TW) of its tile, extended to the plane's edge in the last tile row /
//               column (at most 10 more, all of them in its stage): every pixel of the plane has exactly one owner.  The owner adds
//               the pixel's squared difference (scale 0) and, TH, TW and the plane's sizes being even, writes the 2 x 2-pooled
//               pixels of its area for the next scale from LDS.
//   horizontal  a thread takes 4 consecutive positions of one stage row: 14 pixels of x and of y into registers, 11 fma taps for each of
//               x, y, xx, yy, xy (the squares rounded once), five rows of LDS.  Pitches 43 and 33: conflict-free b32 reads and writes.
//   vertical    a thread takes one column and 2 consecutive rows: 12 values per moment, 11 fma taps each; then cs and l * cs in fp32.
//   reduction   the maps' values are widened to float64 per thread, added over the wave by shuffles, over the four waves in wave
//               order: one float64 per (plane, tile) and quantity in the workspace.  No atomics of any kind.
#include "common.h"
#include <cmath>

namespace {

constexpr int TH = 16, TW = 32, HALO = 10, TAPS = 11;
constexpr int SH = TH + HALO, SW = TW + HALO;          // 26 x 42 staged pixels
constexpr int SP = 43;                                 // stage pitch (floats): 4 consecutive rows x 8 groups of 4 columns hit 32 banks
constexpr int HP = 33;                                 // pitch of the horizontally filtered rows
constexpr int CG = TW / 4;                             // column groups of the horizontal pass

struct SsimSrc { const void* p; long sn, sc, sh, sw; int dtype; };
struct SsimWin { float g[TAPS]; };

struct SsimArgs {
    SsimSrc x, y;
    int C, H, W;                 // channels (plane = n * C + c), this scale's plane
    int tiles_h, tiles_w;
    float c1, c2;
    SsimWin win;
    float* pool_x; float* pool_y;      // [P][H / 2][W / 2] of the next scale, or NULL at the last one
    double* part_ssim; double* part_cs; double* part_sq;      // [P][T]; part_sq NULL past scale 0
};

__device__ __forceinline__ float ssim_load(const SsimSrc& s, long off) {
    if (s.dtype == SP_F32) return ((const float*)s.p)[off];
    const unsigned short b = ((const unsigned short*)s.p)[off];
    if (s.dtype == SP_BF16) return __uint_as_float((unsigned)b << 16);
    union { unsigned short u; _Float16 h; } v; v.u = b;
    return (float)v.h;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void ssim_scale_kernel(SsimArgs a) {
    __shared__ float sx[SH * SP], sy[SH * SP];
    __shared__ float hm[5][SH * HP];
    __shared__ double red[4][3];
    const int tid = threadIdx.x;
    const int T = a.tiles_h * a.tiles_w;
    const int plane = blockIdx.x / T, tile = blockIdx.x - plane * T;
    const int ty = tile / a.tiles_w, tx = tile - ty * a.tiles_w;
    const int r0 = ty * TH, c0 = tx * TW;
    const int n = plane / a.C, c = plane - n * a.C;
    const int H = a.H, W = a.W;
    // the pixels this block owns: its tile, up to the plane's edge in the last tile row / column (<= SH x SW, all staged)
    const int own_h = ty == a.tiles_h - 1 ? H - r0 : TH, own_w = tx == a.tiles_w - 1 ? W - c0 : TW;
    const long bx = (long)n * a.x.sn + (long)c * a.x.sc, by = (long)n * a.y.sn + (long)c * a.y.sc;

    double sq = 0.0;
    for (int i = tid; i < SH * SW; i += 256) {
        const int r = i / SW, q = i - r * SW;
        const int gr = r0 + r, gc = c0 + q;
        float vx = 0.f, vy = 0.f;
        if (gr < H && gc < W) {                                    // nothing is read outside the plane
            vx = ssim_load(a.x, bx + (long)gr * a.x.sh + (long)gc * a.x.sw);
            vy = ssim_load(a.y, by + (long)gr * a.y.sh + (long)gc * a.y.sw);
            if (a.part_sq != nullptr && r < own_h && q < own_w) {
                const float d = vx - vy;
                const double dd = (double)d;
                sq += (d - d == 0.f) ? dd * dd : (double)NAN;      // a NaN or infinite difference: NaN, whatever the rest sums to
            }
        }
        sx[r * SP + q] = vx;
        sy[r * SP + q] = vy;
    }
    __syncthreads();

    if (a.pool_x != nullptr) {
        const int ph = own_h >> 1, pw = own_w >> 1, H2 = H >> 1, W2 = W >> 1;
        float* px = a.pool_x + ((long)plane * H2 + (r0 >> 1)) * W2 + (c0 >> 1);
        float* py = a.pool_y + ((long)plane * H2 + (r0 >> 1)) * W2 + (c0 >> 1);
        for (int i = tid; i < ph * pw; i += 256) {
            const int r = i / pw, q = i - r * pw;
            const float* s0 = sx + (2 * r) * SP + 2 * q;
            const float* s1 = sy + (2 * r) * SP + 2 * q;
            px[(long)r * W2 + q] = ((s0[0] + s0[1]) + (s0[SP] + s0[SP + 1])) * 0.25f;
            py[(long)r * W2 + q] = ((s1[0] + s1[1]) + (s1[SP] + s1[SP + 1])) * 0.25f;
        }
    }

    // horizontal 11 taps: item = (stage row, group of 4 positions)
    for (int item = tid; item < SH * CG; item += 256) {
        const int r = item / CG, q0 = (item - r * CG) * 4;
        float vx[14], vy[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) { vx[k] = sx[r * SP + q0 + k]; vy[k] = sy[r * SP + q0 + k]; }
        float xx[14], yy[14], xy[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) { xx[k] = vx[k] * vx[k]; yy[k] = vy[k] * vy[k]; xy[k] = vx[k] * vy[k]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const float g = a.win.g[k];
                m0 = fmaf(g, vx[j + k], m0); m1 = fmaf(g, vy[j + k], m1);
                m2 = fmaf(g, xx[j + k], m2); m3 = fmaf(g, yy[j + k], m3); m4 = fmaf(g, xy[j + k], m4);
            }
            const int o = r * HP + q0 + j;
            hm[0][o] = m0; hm[1][o] = m1; hm[2][o] = m2; hm[3][o] = m3; hm[4][o] = m4;
        }
    }
    __syncthreads();

    // vertical 11 taps: thread = (column, pair of rows)
    double s_ssim = 0.0, s_cs = 0.0;
    {
        const int q = tid & (TW - 1), rr = (tid >> 5) * 2;
        float m[5][2];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            float v[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = hm[t][(rr + k) * HP + q];
            float u0 = 0.f, u1 = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) { const float g = a.win.g[k]; u0 = fmaf(g, v[k], u0); u1 = fmaf(g, v[k + 1], u1); }
            m[t][0] = u0; m[t][1] = u1;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (r0 + rr + j < H - HALO && c0 + q < W - HALO) {
                const float mx = m[0][j], my = m[1][j];
                const float mxx = mx * mx, myy = my * my, mxy = mx * my;
                const float sxx = m[2][j] - mxx, syy = m[3][j] - myy, sxy = m[4][j] - mxy;
                const float cs = (2.f * sxy + a.c2) / (sxx + syy + a.c2);
                const float l = (2.f * mxy + a.c1) / (mxx + myy + a.c1);
                s_cs += (double)cs;
                s_ssim += (double)(l * cs);
            }
        }
    }
    s_ssim = wave_sum(s_ssim); s_cs = wave_sum(s_cs); sq = wave_sum(sq);
    if ((tid & 63) == 0) { red[tid >> 6][0] = s_ssim; red[tid >> 6][1] = s_cs; red[tid >> 6][2] = sq; }
    __syncthreads();
    if (tid == 0) {
        const long o = (long)plane * T + tile;
        a.part_ssim[o] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        a.part_cs[o] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        if (a.part_sq != nullptr) a.part_sq[o] = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
    }
}

struct SsimFin {
    const double* part_ssim[5]; const double* part_cs[5]; const double* part_sq;
    int tiles[5]; double count[5];
    int planes, scales;
    double* ssim_mean; double* cs_mean; double* sqerr;
};

// one thread per (plane, scale): the tiles' partial sums in index order
__global__ __launch_bounds__(256) void ssim_finalize_kernel(SsimFin f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= f.planes * f.scales) return;
    const int plane = i / f.scales, j = i - plane * f.scales;
    const int T = f.tiles[j];
    const double* ps = f.part_ssim[j] + (long)plane * T;
    const double* pc = f.part_cs[j] + (long)plane * T;
    double s = 0.0, cs = 0.0;
    for (int t = 0; t < T; ++t) { s += ps[t]; cs += pc[t]; }
    if (f.ssim_mean != nullptr) f.ssim_mean[i] = s / f.count[j];
    if (f.cs_mean != nullptr) f.cs_mean[i] = cs / f.count[j];
    if (j == 0 && f.sqerr != nullptr) {
        const double* pq = f.part_sq + (long)plane * T;
        double q = 0.0;
        for (int t = 0; t < T; ++t) q += pq[t];
        f.sqerr[plane] = q;
    }
}

inline long round8(long v) { return (v + 7) & ~7L; }
inline long tiles_of(int h, int w) { return (long)sp_div_up(h - HALO, TH) * sp_div_up(w - HALO, TW); }

// the shape rules shared by the two entry points; 0, or the message is set
int ssim_shape_ok(const char* who, int n, int c, int h, int w, int scales) {
    SP_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1 && (long)n * c <= (1L << 24) && h <= 32768 && w <= 32768,
                 "%s: n=%d c=%d h=%d w=%d (need n, c, h, w >= 1, n*c <= 2^24, h, w <= 32768)", who, n, c, h, w);
    SP_CHECK_ARG(scales >= 1 && scales <= 5, "%s: scales=%d (need 1 .. 5)", who, scales);
    const int m = 1 << (scales - 1);
    SP_CHECK_ARG(h % m == 0 && w % m == 0 && h / m >= TAPS && w / m >= TAPS,
                 "%s: h=%d w=%d with %d scales (need h, w divisible by %d and h/%d, w/%d >= 11; nothing is padded)", who, h, w, scales, m, m, m);
    SP_CHECK_ARG((long)n * c * tiles_of(h, w) <= 0x7fffffffL, "%s: n=%d c=%d h=%d w=%d is more than 2^31 - 1 tiles", who, n, c, h, w);
    return SP_OK;
}

}  // namespace

extern "C" int sp_ssim_workspace(int32_t n, int32_t c, int32_t h, int32_t w_, int32_t scales, int64_t* bytes) {
    SP_CHECK_ARG(bytes != nullptr, "sp_ssim_workspace: bytes must not be NULL");
    const int rc = ssim_shape_ok("sp_ssim_workspace", n, c, h, w_, scales);
    if (rc != SP_OK) return rc;
    const long P = (long)n * c;
    long total = 0, tiles = tiles_of(h, w_);
    for (int j = 0; j < scales; ++j) {
        if (j > 0) total += 2 * round8(4 * P * (h >> j) * (w_ >> j));
        tiles += 2 * tiles_of(h >> j, w_ >> j);
    }
    *bytes = total + 8 * P * tiles;
    return SP_OK;
}

extern "C" int sp_ssim_stats(const void* x, int32_t x_dtype, int64_t xn, int64_t xc, int64_t xh, int64_t xw,
                             const void* y, int32_t y_dtype, int64_t yn, int64_t yc, int64_t yh, int64_t yw,
                             int32_t n, int32_t c, int32_t h, int32_t w_, int32_t scales, double data_range,
                             double* ssim_mean, double* cs_mean, double* sqerr,
                             void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    SP_CHECK_ARG(x && y && workspace, "sp_ssim_stats: x, y and workspace must not be NULL");
    const auto known = [](int32_t t) { return t == SP_F32 || t == SP_BF16 || t == SP_F16; };
    SP_CHECK_ARG(known(x_dtype) && known(y_dtype), "sp_ssim_stats: bad dtype (x_dtype %d, y_dtype %d; need SP_F32 / SP_BF16 / SP_F16)", x_dtype, y_dtype);
    SP_CHECK_ARG(xn >= 0 && xc >= 0 && xh >= 0 && xw >= 0 && yn >= 0 && yc >= 0 && yh >= 0 && yw >= 0, "sp_ssim_stats: negative stride");
    int rc = ssim_shape_ok("sp_ssim_stats", n, c, h, w_, scales);
    if (rc != SP_OK) return rc;
    SP_CHECK_ARG(std::isfinite(data_range) && data_range > 0.0, "sp_ssim_stats: data_range=%g (need finite and > 0)", data_range);
    int64_t need = 0;
    rc = sp_ssim_workspace(n, c, h, w_, scales, &need);
    if (rc != SP_OK) return rc;
    SP_CHECK_ARG(workspace_bytes >= need, "sp_ssim_stats: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
    SP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "sp_ssim_stats: workspace must be 8-byte aligned");

    const long P = (long)n * c;
    // the layout sp_ssim_workspace states: pooled planes of x and y per scale >= 1, then the partial sums
    char* base = (char*)workspace;
    float* pool_x[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* pool_y[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int j = 1; j < scales; ++j) {
        const long b = round8(4 * P * (h >> j) * (w_ >> j));
        pool_x[j] = (float*)base; base += b;
        pool_y[j] = (float*)base; base += b;
    }
    SsimFin fin = {};
    for (int j = 0; j < scales; ++j) {
        const long T = tiles_of(h >> j, w_ >> j);
        fin.part_ssim[j] = (double*)base; base += 8 * P * T;
        fin.part_cs[j] = (double*)base; base += 8 * P * T;
        fin.tiles[j] = (int)T;
        fin.count[j] = (double)((h >> j) - HALO) * (double)((w_ >> j) - HALO);
    }
    fin.part_sq = (double*)base;
    fin.planes = (int)P; fin.scales = scales;
    fin.ssim_mean = ssim_mean; fin.cs_mean = cs_mean; fin.sqerr = sqerr;

    SsimWin win;
    {
        double e[TAPS], z = 0.0;
        for (int k = 0; k < TAPS; ++k) { e[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5); z += e[k]; }
        for (int k = 0; k < TAPS; ++k) win.g[k] = (float)(e[k] / z);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (int j = 0; j < scales; ++j) {
        const int H = h >> j, W = w_ >> j;
        SsimArgs a;
        if (j == 0) {
            a.x = {x, xn, xc, xh, xw, x_dtype};
            a.y = {y, yn, yc, yh, yw, y_dtype};
        } else {
            a.x = {pool_x[j], (long)c * H * W, (long)H * W, W, 1, SP_F32};
            a.y = {pool_y[j], (long)c * H * W, (long)H * W, W, 1, SP_F32};
        }
        a.C = c; a.H = H; a.W = W;
        a.tiles_h = sp_div_up(H - HALO, TH); a.tiles_w = sp_div_up(W - HALO, TW);
        a.c1 = (float)((0.01 * data_range) * (0.01 * data_range));
        a.c2 = (float)((0.03 * data_range) * (0.03 * data_range));
        a.win = win;
        a.pool_x = j + 1 < scales ? pool_x[j + 1] : nullptr;
        a.pool_y = j + 1 < scales ? pool_y[j + 1] : nullptr;
        a.part_ssim = const_cast<double*>(fin.part_ssim[j]);
        a.part_cs = const_cast<double*>(fin.part_cs[j]);
        a.part_sq = j == 0 ? const_cast<double*>(fin.part_sq) : nullptr;
        hipLaunchKernelGGL(ssim_scale_kernel, dim3((unsigned)(P * fin.tiles[j])), dim3(256), 0, s, a);
        SP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(sp_div_up(P * scales, 256)), dim3(256), 0, s, fin);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
