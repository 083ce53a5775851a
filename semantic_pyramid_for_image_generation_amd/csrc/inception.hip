// Inception-v3 feature extractor of the FID metric (/root/reference/frechet_inception_distance.py:11-42, torchvision's Inception3 in
// eval mode): forward only, NHWC, the compute dtype of the rest of the library (fp32 / bf16 / fp16 - the fp16 twin is this file
// compiled with -DSP_H16_FP16, as every other source).
//
//   sp_conv2d_general     BasicConv2d with its BatchNorm folded in: y[:, :, :, 0:cout] of a wider tensor = ReLU(conv(x, w) + b) for
//                         any kh, kw <= 7, stride 1 / 2, independent pad_h / pad_w - the implicit GEMM of every one of the 94 layers.
//   sp_maxpool3s2_fwd     F.max_pool2d(kernel_size=3, stride=2) into a channel slice (stem, Mixed_6a, Mixed_7a)
//   sp_avgpool3s1_fwd     F.avg_pool2d(kernel_size=3, stride=1, padding=1), count_include_pad: the pool branch of InceptionA / C / E
//   sp_inception_prep     misc.normalize_m1_1_batch + F.interpolate(bilinear, align_corners=False) + NCHW fp32 -> padded NHWC
//   sp_global_avgpool_f32 F.adaptive_avg_pool2d(Mixed_7c, 1) as fp32 rows
#include "common.h"

namespace {

// ---- the convolution ------------------------------------------------------------------------------------------------------------
// Implicit GEMM: D[co][px] = sum_k W[co][k] X[px][k], k = (ky * kw + kx) * cin_p + c.  A block of 256 threads owns 64 output pixels x
// 64 output channels; each of its four waves a 32 x 32 quarter (2 x 2 MFMA tiles of 16 x 16).  The K loop walks the flattened
// (tap, channel) index in chunks of 32: every thread stages 8 consecutive k of one pixel row and 8 of one weight row (cin_p % 8 == 0,
// so a group of 8 never straddles two taps), the next chunk is fetched into registers while the current one is multiplied.
// MFMA: A = weights (rows = output channels), B = pixels, so a lane's four accumulators are four consecutive channels of ONE pixel
// and the epilogue stores them as one 8- / 16-byte write into the channel slice.
constexpr int BM = 64, BN = 64, KC = 32;

template <typename T> struct Vec8;
template <> struct Vec8<bf16> {
    uint4 v;
    __device__ __forceinline__ void zero() { v = make_uint4(0, 0, 0, 0); }
    __device__ __forceinline__ void ld(const bf16* p) { v = *reinterpret_cast<const uint4*>(p); }
    __device__ __forceinline__ void st(bf16* p) const { *reinterpret_cast<uint4*>(p) = v; }
};
template <> struct Vec8<float> {
    float4 a, b;
    __device__ __forceinline__ void zero() { a = b = make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ __forceinline__ void ld(const float* p) { a = reinterpret_cast<const float4*>(p)[0]; b = reinterpret_cast<const float4*>(p)[1]; }
    __device__ __forceinline__ void st(float* p) const { reinterpret_cast<float4*>(p)[0] = a; reinterpret_cast<float4*>(p)[1] = b; }
};
// LDS row pitch in elements: 16-byte aligned rows, shifted by 16 bytes per row against bank conflicts
template <typename T> struct Ldk { static constexpr int v = KC + 16 / (int)sizeof(T); };

struct GeoArgs {
    int n, h, w, cin_p, ldx, cout, ldy, kh, kw, sh, sw, ph, pw, oh, ow, act;
};

template <typename T>
__global__ __launch_bounds__(256) void conv_general_kernel(const T* __restrict__ x, const T* __restrict__ wt, const float* __restrict__ bias,
                                                           T* __restrict__ y, GeoArgs g) {
    constexpr int LDK = Ldk<T>::v;
    __shared__ __attribute__((aligned(16))) T sA[BM * LDK];
    __shared__ __attribute__((aligned(16))) T sB[BN * LDK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const long M = (long)g.n * g.oh * g.ow;
    const long m0 = (long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;
    const int K = g.kh * g.kw * g.cin_p;
    const int nchunks = (K + KC - 1) / KC;

    // the staging row of this thread: pixel m0 + r of the A tile, output channel co0 + r of the B tile
    const int r = t >> 2, kv = (t & 3) * 8;
    const long m = m0 + r;
    const bool m_ok = m < M;
    int iy0 = 0, ix0 = 0;
    const T* xn = x;
    if (m_ok) {
        const int ohw = g.oh * g.ow;
        const int img = (int)(m / ohw), rem = (int)(m - (long)img * ohw);
        const int oy = rem / g.ow, ox = rem - oy * g.ow;
        iy0 = oy * g.sh - g.ph;
        ix0 = ox * g.sw - g.pw;
        xn = x + (long)img * g.h * g.w * g.ldx;
    }
    const bool co_ok = co0 + r < g.cout;
    const T* wrow = wt + (long)(co0 + r) * K;

    auto load = [&](int kc, Vec8<T>& va, Vec8<T>& vb) {
        const int kg = kc * KC + kv;
        va.zero();
        vb.zero();
        if (kg < K) {
            if (co_ok) vb.ld(wrow + kg);
            if (m_ok) {
                const int tap = kg / g.cin_p, c = kg - tap * g.cin_p;
                const int ky = tap / g.kw, kx = tap - ky * g.kw;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) va.ld(xn + ((long)iy * g.w + ix) * g.ldx + c);
            }
        }
    };

    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    Vec8<T> va, vb;
    load(0, va, vb);
    for (int kc = 0; kc < nchunks; ++kc) {
        va.st(&sA[r * LDK + kv]);
        vb.st(&sB[r * LDK + kv]);
        __syncthreads();
        if (kc + 1 < nchunks) load(kc + 1, va, vb);
        const int row = lane & 15, kq = lane >> 4;
        if constexpr (sizeof(T) == 2) {
            uint4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const uint4*>(&sB[(wn * 32 + i * 16 + row) * LDK + 8 * kq]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const uint4*>(&sA[(wm * 32 + j * 16 + row) * LDK + 8 * kq]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[i]), __builtin_bit_cast(bf16x8_t, b[j]),
                                                                        acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                float a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = reinterpret_cast<const float*>(sB)[(wn * 32 + i * 16 + row) * LDK + 4 * kk + kq];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = reinterpret_cast<const float*>(sA)[(wm * 32 + j * 16 + row) * LDK + 4 * kk + kq];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: lane -> pixel (lane & 15) of a 16-pixel tile, 4 consecutive channels (lane >> 4) * 4 + reg
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long mo = m0 + wm * 32 + j * 16 + (lane & 15);
        if (mo >= M) continue;
        T* yrow = y + mo * g.ldy;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int co = co0 + wn * 32 + i * 16 + (lane >> 4) * 4;
            if (co >= g.cout) continue;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = acc[i][j][q] + (bias ? bias[co + q] : 0.f);
            apply_act_vec<4, false>(v, g.act);
            Elem<T>::st4(yrow + co, v);
        }
    }
}

// ---- pools --------------------------------------------------------------------------------------------------------------------
// one thread per (output pixel, group of 4 channels)
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int n, int h, int w,
                                                         int c, int oh, int ow) {
    const int cg = c / 4;
    const long items = (long)n * oh * ow * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int q = (int)(i % cg);
        const long p = i / cg;
        const int ox = (int)(p % ow), oy = (int)((p / ow) % oh), img = (int)(p / ((long)ow * oh));
        const T* base = x + (((long)img * h + 2 * oy) * w + 2 * ox) * ldx + 4 * q;
        float m[4];
        Elem<T>::ld4(base, m);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (dy == 0 && dx == 0) continue;
                float v[4];
                Elem<T>::ld4(base + ((long)dy * w + dx) * ldx, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
            }
        Elem<T>::st4(y + p * ldy + 4 * q, m);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool3s1_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int h, int w, int c) {
    const int cg = c / 4;
    const long items = (long)n * h * w * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int q = (int)(i % cg);
        const long p = i / cg;
        const int ox = (int)(p % w), oy = (int)((p / w) % h), img = (int)(p / ((long)w * h));
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int iy = oy - 1; iy <= oy + 1; ++iy) {
            if (iy < 0 || iy >= h) continue;
            for (int ix = ox - 1; ix <= ox + 1; ++ix) {
                if (ix < 0 || ix >= w) continue;
                float v[4];
                Elem<T>::ld4(x + (((long)img * h + iy) * w + ix) * c + 4 * q, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += v[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = s[e] / 9.f;          // count_include_pad: the divisor is always 9
        Elem<T>::st4(y + p * c + 4 * q, s);
    }
}

// ---- input preparation ----------------------------------------------------------------------------------------------------------
// per-image min / max over all channels and pixels (misc.normalize_m1_1_batch flattens the image): one block per image
__global__ __launch_bounds__(256) void image_minmax_kernel(const float* __restrict__ x, long per_image, float* __restrict__ mm) {
    __shared__ float smin[4], smax[4];
    const float* p = x + (long)blockIdx.x * per_image;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long i = threadIdx.x; i < per_image; i += 256) {
        const float v = p[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        mm[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// torch's upsample_bilinear2d, align_corners=False, no scale factor: src = (in / out) * (dst + 0.5) - 0.5, clamped at 0
__device__ __forceinline__ void bilinear_src(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// one thread per output pixel: the (normalised) source pixels are interpolated per channel, channels c .. cp-1 are written as zeros
template <typename T>
__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ x, const float* __restrict__ mm, T* __restrict__ y, int n, int c,
                                                   int h, int w, int oh, int ow, int cp) {
    const long items = (long)n * oh * ow;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % ow), oy = (int)((i / ow) % oh), img = (int)(i / ((long)ow * oh));
        int y0, y1, x0, x1;
        float hl0, hl1, wl0, wl1;
        bilinear_src(oy, h, oh, y0, y1, hl0, hl1);
        bilinear_src(ox, w, ow, x0, x1, wl0, wl1);
        const float lo = mm[2 * img], rng = mm[2 * img + 1] - lo;
        T* out = y + i * cp;
        for (int ch = 0; ch < cp; ch += 4) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = 0.f;
                if (ch + e < c) {
                    const float* pl = x + ((long)img * c + ch + e) * h * w;
                    // misc.normalize_m1_1_batch: 2 * ((x - min) / (max - min)) - 1, then the interpolation of the normalised image
                    const float a = 2.f * ((pl[(long)y0 * w + x0] - lo) / rng) - 1.f, b = 2.f * ((pl[(long)y0 * w + x1] - lo) / rng) - 1.f;
                    const float cc = 2.f * ((pl[(long)y1 * w + x0] - lo) / rng) - 1.f, d = 2.f * ((pl[(long)y1 * w + x1] - lo) / rng) - 1.f;
                    v[e] = hl0 * (wl0 * a + wl1 * b) + hl1 * (wl0 * cc + wl1 * d);
                }
            }
            Elem<T>::st4(out + ch, v);
        }
    }
}

// one thread per (image, channel): mean over the h * w pixels, in pixel order
template <typename T>
__global__ __launch_bounds__(256) void global_avg_kernel(const T* __restrict__ x, float* __restrict__ y, int n, int hw, int c) {
    const long items = (long)n * c;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % c), img = (int)(i / c);
        const T* p = x + (long)img * hw * c + ch;
        float s = 0.f;
        for (int k = 0; k < hw; ++k) s += Elem<T>::ld(p + (long)k * c);
        y[i] = s / (float)hw;
    }
}

inline int grid_for(long items) {
    const long b = (items + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
inline bool aligned(const void* p, int bytes) { return ((uintptr_t)p % bytes) == 0; }
// storage types of this file (SP_F16 arrives here as SP_BF16 of the fp16 compilation)
#define SP_CHECK_DTYPE(dtype, name) do { if ((dtype) != SP_F32 && (dtype) != SP_BF16) { \
    sp_set_error("%s: dtype %d not supported (SP_F32 / SP_BF16 / SP_F16)", name, (int)(dtype)); return SP_ERR_UNSUPPORTED; } } while (0)

}  // namespace

extern "C" int sp_conv2d_general(const sp_conv_general_params* p, sp_stream_t stream) {
    SP_CHECK_ARG(p != nullptr, "sp_conv2d_general: NULL params");
    SP_CHECK_ARG(p->struct_bytes == (int32_t)sizeof(sp_conv_general_params),
                 "sp_conv2d_general: struct_bytes %d != sizeof(sp_conv_general_params) %d (header / library mismatch)", p->struct_bytes,
                 (int)sizeof(sp_conv_general_params));
    const sp_conv_general_params& q = *p;
    SP_CHECK_DTYPE(q.dtype, "sp_conv2d_general");
    SP_CHECK_ARG(q.x && q.w && q.y, "sp_conv2d_general: x, w and y are required");
    SP_CHECK_ARG(q.n > 0 && q.h > 0 && q.w_ > 0 && q.cout > 0, "sp_conv2d_general: empty shape n=%d h=%d w=%d cout=%d", q.n, q.h, q.w_, q.cout);
    SP_CHECK_ARG(q.kh >= 1 && q.kh <= 7 && q.kw >= 1 && q.kw <= 7, "sp_conv2d_general: kernel %dx%d outside 1..7", q.kh, q.kw);
    SP_CHECK_ARG((q.stride_h == 1 || q.stride_h == 2) && (q.stride_w == 1 || q.stride_w == 2), "sp_conv2d_general: stride must be 1 or 2");
    SP_CHECK_ARG(q.pad_h >= 0 && q.pad_w >= 0 && q.pad_h < q.kh && q.pad_w < q.kw, "sp_conv2d_general: padding must be in [0, k)");
    SP_CHECK_ARG(q.cin_p > 0 && q.cin_p % 8 == 0, "sp_conv2d_general: cin_p %d must be a positive multiple of 8", q.cin_p);
    SP_CHECK_ARG(q.ldx >= q.cin_p && q.ldx % 8 == 0, "sp_conv2d_general: ldx %d must be >= cin_p and a multiple of 8", q.ldx);
    SP_CHECK_ARG(q.cout % 4 == 0 && q.ldy % 4 == 0 && q.ldy >= q.cout, "sp_conv2d_general: cout %d / ldy %d (multiples of 4, ldy >= cout)",
                 q.cout, q.ldy);
    SP_CHECK_ARG(q.act == SP_ACT_NONE || q.act == SP_ACT_RELU, "sp_conv2d_general: act must be NONE or RELU");
    const int es = q.dtype == SP_F32 ? 4 : 2;
    SP_CHECK_ARG(aligned(q.x, 16) && aligned(q.w, 16) && aligned(q.y, 4 * es) && (!q.bias || aligned(q.bias, 4)),
                 "sp_conv2d_general: x and w need 16-byte alignment, y (the slice start) %d-byte alignment", 4 * es);
    const int oh = (q.h + 2 * q.pad_h - q.kh) / q.stride_h + 1, ow = (q.w_ + 2 * q.pad_w - q.kw) / q.stride_w + 1;
    SP_CHECK_ARG(q.h + 2 * q.pad_h >= q.kh && q.w_ + 2 * q.pad_w >= q.kw, "sp_conv2d_general: kernel larger than the padded input");
    const long M = (long)q.n * oh * ow;
    const long K = (long)q.kh * q.kw * q.cin_p;
    SP_CHECK_ARG((M + BM - 1) / BM < (1L << 31) && K < (1L << 30) && (long)q.n * q.h * q.w_ * q.ldx < (1L << 40),
                 "sp_conv2d_general: tensor too large");
    GeoArgs g{q.n, q.h, q.w_, q.cin_p, q.ldx, q.cout, q.ldy, q.kh, q.kw, q.stride_h, q.stride_w, q.pad_h, q.pad_w, oh, ow, q.act};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((q.cout + BN - 1) / BN));
    if (q.dtype == SP_F32)
        hipLaunchKernelGGL(conv_general_kernel<float>, grid, dim3(256), 0, s, (const float*)q.x, (const float*)q.w, q.bias, (float*)q.y, g);
    else
        hipLaunchKernelGGL(conv_general_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)q.x, (const bf16*)q.w, q.bias, (bf16*)q.y, g);
    SP_LAUNCH_CHECK();
    sp_note_route("conv_general");
    return SP_OK;
}

extern "C" int sp_maxpool3s2_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype,
                                 sp_stream_t stream) {
    SP_CHECK_ARG(x && y && n > 0 && c > 0 && c % 4 == 0 && ldx >= c && ldy >= c && ldx % 4 == 0 && ldy % 4 == 0,
                 "sp_maxpool3s2_fwd: bad args (c %d, ldx %d, ldy %d: multiples of 4, ld >= c)", c, ldx, ldy);
    SP_CHECK_ARG(h >= 3 && w_ >= 3, "sp_maxpool3s2_fwd: input %dx%d smaller than the 3x3 window", h, w_);
    SP_CHECK_DTYPE(dtype, "sp_maxpool3s2_fwd");
    const int es = dtype == SP_F32 ? 4 : 2;
    SP_CHECK_ARG(aligned(x, 4 * es) && aligned(y, 4 * es), "sp_maxpool3s2_fwd: x / y need %d-byte alignment", 4 * es);
    const int oh = (h - 3) / 2 + 1, ow = (w_ - 3) / 2 + 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int g = grid_for((long)n * oh * ow * (c / 4));
    if (dtype == SP_F32) hipLaunchKernelGGL(maxpool3s2_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x, ldx, (float*)y, ldy, n, h, w_, c, oh, ow);
    else hipLaunchKernelGGL(maxpool3s2_kernel<bf16>, dim3(g), dim3(256), 0, s, (const bf16*)x, ldx, (bf16*)y, ldy, n, h, w_, c, oh, ow);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_avgpool3s1_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(x && y && n > 0 && h > 0 && w_ > 0 && c > 0 && c % 4 == 0, "sp_avgpool3s1_fwd: bad args (c %d: a multiple of 4)", c);
    SP_CHECK_DTYPE(dtype, "sp_avgpool3s1_fwd");
    const int es = dtype == SP_F32 ? 4 : 2;
    SP_CHECK_ARG(aligned(x, 4 * es) && aligned(y, 4 * es), "sp_avgpool3s1_fwd: x / y need %d-byte alignment", 4 * es);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int g = grid_for((long)n * h * w_ * (c / 4));
    if (dtype == SP_F32) hipLaunchKernelGGL(avgpool3s1_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x, (float*)y, n, h, w_, c);
    else hipLaunchKernelGGL(avgpool3s1_kernel<bf16>, dim3(g), dim3(256), 0, s, (const bf16*)x, (bf16*)y, n, h, w_, c);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_inception_prep(const float* x, float* minmax, void* y, int32_t n, int32_t c, int32_t h, int32_t w_, int32_t oh, int32_t ow,
                                 int32_t cp, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(x && minmax && y && n > 0 && c > 0 && h > 0 && w_ > 0 && oh > 0 && ow > 0, "sp_inception_prep: bad args");
    SP_CHECK_ARG(cp >= c && cp % 8 == 0, "sp_inception_prep: cp %d must be >= c %d and a multiple of 8", cp, c);
    SP_CHECK_DTYPE(dtype, "sp_inception_prep");
    const int es = dtype == SP_F32 ? 4 : 2;
    SP_CHECK_ARG(aligned(y, 4 * es), "sp_inception_prep: y needs %d-byte alignment", 4 * es);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(image_minmax_kernel, dim3(n), dim3(256), 0, s, x, (long)c * h * w_, minmax);
    SP_LAUNCH_CHECK();
    const int g = grid_for((long)n * oh * ow);
    if (dtype == SP_F32) hipLaunchKernelGGL(prep_kernel<float>, dim3(g), dim3(256), 0, s, x, (const float*)minmax, (float*)y, n, c, h, w_, oh, ow, cp);
    else hipLaunchKernelGGL(prep_kernel<bf16>, dim3(g), dim3(256), 0, s, x, (const float*)minmax, (bf16*)y, n, c, h, w_, oh, ow, cp);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_global_avgpool_f32(const void* x, float* y, int32_t n, int32_t hw, int32_t c, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(x && y && n > 0 && hw > 0 && c > 0, "sp_global_avgpool_f32: bad args");
    SP_CHECK_DTYPE(dtype, "sp_global_avgpool_f32");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int g = grid_for((long)n * c);
    if (dtype == SP_F32) hipLaunchKernelGGL(global_avg_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)x, y, n, hw, c);
    else hipLaunchKernelGGL(global_avg_kernel<bf16>, dim3(g), dim3(256), 0, s, (const bf16*)x, y, n, hw, c);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
