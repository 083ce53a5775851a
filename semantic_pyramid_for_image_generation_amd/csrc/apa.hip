// Adaptive pseudo augmentation (Jiang et al. 2021, "Deceive D", APA): the selection of the discriminator's real branch, one launch.
// include/sempyr.h has the definition (sp_apa_select), DESIGN.md section 22 the design.
//
// dst is a contiguous fp32 n x 3 x h x w batch.  Image i of it is float(fake[i]) iff w_u[i] < p_dev[0] (strict, fp32: the compare of the
// augmenting ingest's gate, csrc/augment.hip), else float(real[i]).  p_dev[0] is read when the kernel RUNS: grid, addresses and every
// host value are the same for every p, so a captured graph follows p without a re-capture.  The grid is (blocks, images): an image's
// choice is one compare on two block-uniform loads, the branch is block-uniform, and a block reads only the source it chose.
//
// Pure data movement: a 16-bit value is widened (exact), an fp32 value passes through registers untouched (NaN payloads and infinities
// arrive as they are).  No atomics, no reduction: two runs give the same bits.
//
// A thread takes 4 consecutive pixels of the flattened map with their 3 channels and writes three 16-byte stores, one per plane of dst
// (a wave: 1 KiB contiguous per plane), where dst is 16-byte aligned and h w % 4 == 0; else element stores.  How it reads them is chosen
// per source on the host from strides and alignment alone:
//   APA_PLANAR  pixels contiguous within a channel plane (NCHW, or a slice of one whose rows stay dense): one load of 4 elements per
//               channel - 16 bytes in fp32, 8 in a 16-bit type;
//   APA_PIXEL   channels contiguous within a pixel whose pitch is a multiple of 4 elements and whose rows are dense (the padded NHWC
//               buffer behind the generator's NCHW view: pitch 8 in a 16-bit type, 4 in fp32): one load of 4 elements per pixel, of which
//               3 are used - every byte of the buffer is fetched once, in order.  The group that holds an image's LAST pixel takes the
//               element loads below: the 4th element of that pixel need not exist in a caller's buffer;
//   APA_GENERIC anything else (channels-last without padding, a slice with a row pitch, a broadcast): one load per element through
//               the four strides.
#include "common.h"

namespace {

// the dispatcher hands this compilation SP_BF16 for ITS 16-bit type (common.h) and the sources' types as the caller gave them
#ifdef SP_H16_FP16
constexpr int APA_OWN16 = SP_F16, APA_OTHER16 = SP_BF16;
#else
constexpr int APA_OWN16 = SP_BF16, APA_OTHER16 = SP_F16;
#endif

constexpr int APA_BLOCKS = 128;          // blocks per image at most (grid-stride beyond), as the augmenting ingest's apply launches

enum { APA_GENERIC = 0, APA_PLANAR = 1, APA_PIXEL = 2 };

// one source as an entry was given it, plus how its loads go (host: apa_mode)
struct ApaSrc { const void* p; long sn, sc, sh, sw; int mode; };

// 4 pixels x 3 channels of dst at pixel p0: three 16-byte stores, or the elements below HW one by one
__device__ __forceinline__ void apa_store(float* __restrict__ dst, int HW, int p0, const float (&v)[3][4], bool vec) {
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Elem<float>::st4(dst + (long)c * HW + p0, v[c]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p0 + j < HW) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[(long)c * HW + p0 + j] = v[c][j];
            }
        }
    }
}

// One image, one source.  The groups a vector load serves come first, in a loop of their own with nothing but that load in it (in one
// loop with the element loads the compiler merges the three forms into twelve element loads); what is left - every group of
// APA_GENERIC, an image's last group or two of the other forms - takes the element loads.
template <typename TS, int MODE>
__device__ __forceinline__ void apa_copy(const TS* __restrict__ src, long sc, long sh, long sw, float* __restrict__ dst, int W, int HW, bool dvec) {
    const int groups = (HW + 3) >> 2;
    // APA_PLANAR: every full group.  APA_PIXEL: the groups in front of the one that holds the last pixel (p0 + 4 < HW).
    const int nvec = MODE == APA_PLANAR ? HW >> 2 : (MODE == APA_PIXEL ? (HW - 1) >> 2 : 0);
    for (int g = blockIdx.x * 256 + threadIdx.x; g < nvec; g += gridDim.x * 256) {
        const int p0 = g * 4;
        float v[3][4];
        if (MODE == APA_PLANAR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Elem<TS>::ld4(src + c * sc + p0, v[c]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t[4];
                Elem<TS>::ld4(src + (long)(p0 + j) * sw, t);
                v[0][j] = t[0]; v[1][j] = t[1]; v[2][j] = t[2];
            }
        }
        apa_store(dst, HW, p0, v, dvec);           // (dvec false: a full group's four pixels, all below HW)
    }
    for (int g = nvec + blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int p0 = g * 4;
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = min(p0 + j, HW - 1);     // (a slot past the end repeats the last pixel; it is never stored)
            const int h = p / W, w = p - h * W;
            const TS* s = src + (long)h * sh + (long)w * sw;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = Elem<TS>::ld(s + c * sc);
        }
        apa_store(dst, HW, p0, v, dvec && p0 + 4 <= HW);
    }
}

template <typename TS>
__device__ __forceinline__ void apa_copy_image(const ApaSrc& a, int i, float* __restrict__ dst, int W, int HW, bool dvec) {
    const TS* src = (const TS*)a.p + (long)i * a.sn;
    if (a.mode == APA_PLANAR) apa_copy<TS, APA_PLANAR>(src, a.sc, a.sh, a.sw, dst, W, HW, dvec);
    else if (a.mode == APA_PIXEL) apa_copy<TS, APA_PIXEL>(src, a.sc, a.sh, a.sw, dst, W, HW, dvec);
    else apa_copy<TS, APA_GENERIC>(src, a.sc, a.sh, a.sw, dst, W, HW, dvec);
}

template <typename TR, typename TF>
__global__ __launch_bounds__(256) void apa_select_kernel(ApaSrc real, ApaSrc fake, float* __restrict__ dst, int W, int HW, int dvec,
                                                         const float* __restrict__ w_u, const float* __restrict__ p_dev) {
    const int i = blockIdx.y;
    float* d = dst + (long)i * 3 * HW;
    if (w_u[i] < p_dev[0]) apa_copy_image<TF>(fake, i, d, W, HW, dvec != 0);        // strict fp32 compare; a NaN p takes nothing
    else apa_copy_image<TR>(real, i, d, W, HW, dvec != 0);
}

// the load form a source admits: from its strides, its element size and its base address alone
int apa_mode(const void* p, int esz, long sn, long sc, long sh, long sw, int h, int w) {
    const bool aligned = reinterpret_cast<uintptr_t>(p) % (4 * esz) == 0 && sn % 4 == 0;
    if (aligned && sw == 1 && (sh == w || h == 1) && sc % 4 == 0) return APA_PLANAR;
    if (aligned && sc == 1 && sw >= 4 && sw % 4 == 0 && (sh == (long)w * sw || h == 1)) return APA_PIXEL;
    return APA_GENERIC;
}

template <typename TR, typename TF>
void apa_launch(const ApaSrc& real, const ApaSrc& fake, float* dst, int n, int h, int w, const float* w_u, const float* p_dev, hipStream_t s) {
    const int HW = h * w;
    const int dvec = reinterpret_cast<uintptr_t>(dst) % 16 == 0 && HW % 4 == 0;
    const int blocks = min(APA_BLOCKS, sp_div_up((HW + 3) / 4, 256));
    hipLaunchKernelGGL((apa_select_kernel<TR, TF>), dim3(blocks, n), dim3(256), 0, s, real, fake, dst, w, HW, dvec, w_u, p_dev);
}

}  // namespace

extern "C" int sp_apa_select(const void* real, int32_t real_dtype, int64_t rn, int64_t rc, int64_t rh, int64_t rw,
                             const void* fake, int32_t fake_dtype, int64_t fn, int64_t fc, int64_t fh, int64_t fw,
                             float* dst, int32_t n, int32_t h, int32_t w_,
                             const float* w_u, const float* p_dev, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(real && fake && dst && w_u && p_dev, "sp_apa_select: real, fake, dst, w_u and p_dev must not be NULL");
    SP_CHECK_ARG(n >= 1 && n <= 65535 && h >= 1 && w_ >= 1 && (long)h * w_ <= (1L << 28), "sp_apa_select: n=%d h=%d w=%d (need n in [1, 65535], h, w >= 1, h*w <= 2^28)",
                 n, h, w_);
    const auto known = [](int32_t t) { return t == SP_F32 || t == SP_BF16 || t == SP_F16; };
    SP_CHECK_ARG((dtype == SP_F32 || dtype == SP_BF16) && known(real_dtype) && known(fake_dtype),
                 "sp_apa_select: bad dtype (dtype, real_dtype, fake_dtype: SP_F32 / SP_BF16 / SP_F16; got real_dtype %d, fake_dtype %d)", real_dtype, fake_dtype);
    if (real_dtype == APA_OTHER16 || fake_dtype == APA_OTHER16) {      // the two 16-bit types never mix: sp_ingest_image's rule
        sp_set_error(APA_OWN16 == SP_F16 ? "sp_apa_select: an SP_BF16 source needs SP_BF16 or SP_F32 storage"
                                         : "sp_apa_select: an SP_F16 source needs SP_F16 storage");
        return SP_ERR_UNSUPPORTED;
    }
    SP_CHECK_ARG(rn >= 0 && rc >= 0 && rh >= 0 && rw >= 0 && fn >= 0 && fc >= 0 && fh >= 0 && fw >= 0, "sp_apa_select: negative stride");
    const bool r32 = real_dtype == SP_F32, f32 = fake_dtype == SP_F32;
    const ApaSrc r = {real, rn, rc, rh, rw, apa_mode(real, r32 ? 4 : 2, rn, rc, rh, rw, h, w_)};
    const ApaSrc f = {fake, fn, fc, fh, fw, apa_mode(fake, f32 ? 4 : 2, fn, fc, fh, fw, h, w_)};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (r32) {
        if (f32) apa_launch<float, float>(r, f, dst, n, h, w_, w_u, p_dev, s);
        else apa_launch<float, bf16>(r, f, dst, n, h, w_, w_u, p_dev, s);
    } else {
        if (f32) apa_launch<bf16, float>(r, f, dst, n, h, w_, w_u, p_dev, s);
        else apa_launch<bf16, bf16>(r, f, dst, n, h, w_, w_u, p_dev, s);
    }
    SP_LAUNCH_CHECK();
    return SP_OK;
}
