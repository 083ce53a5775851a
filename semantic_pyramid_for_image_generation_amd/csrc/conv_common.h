// Pieces shared by the implicit-GEMM convolution kernels (conv_igemm.hip, conv_pp.hip, conv_ppw.hip): MFMA wrappers, compile-time
// loops, the epilogues (bias / activation-derivative mask / residuals / activation / 2x2 pooling), the ping-pong kernels' work items
// and tail split, and the inline-asm LDS / wait helpers.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include "common.h"

namespace {

template <typename T> struct Mma;
template <> struct Mma<bf16> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    }
};

struct f8 { uint8_t v; };                        // OCP e4m3 storage (SP_F8): 16 elements per 16-byte fragment read
template <> struct Mma<f8> {
    // a / b: 16 consecutive k of one row (bytes 0-7 feed the first MFMA, 8-15 the second; A and B use the same split, so the
    // sum over the 64-byte chunk is complete)
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& c) {
        const long a0 = (long)(((unsigned long long)a.y << 32) | a.x), a1 = (long)(((unsigned long long)a.w << 32) | a.z);
        const long b0 = (long)(((unsigned long long)b.y << 32) | b.x), b1 = (long)(((unsigned long long)b.w << 32) | b.z);
        c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a0, b0, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a1, b1, c, 0, 0, 0);
    }
};

template <int... I, typename F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// two-group batches (sp_conv_params.img_scale): the scale of the group output pixel `pix` belongs to (pix counts OUTPUT pixels)
__device__ __forceinline__ float conv_img_scale(const sp_conv_params& p, long pix) {
    return p.img_scale != nullptr ? p.img_scale[pix >= p.split_pix_ ? 1 : 0] : 1.f;
}

template <typename T>
__device__ __forceinline__ void conv_epilogue4(const sp_conv_params& p, float (&v)[4], long pix, int co, bool vec_ok, bool add_bias = true) {
    if (p.img_scale != nullptr && add_bias) {      // (add_bias == false: the caller pre-added the bias and has applied the scale itself)
        const float sc = conv_img_scale(p, pix);
        v[0] *= sc; v[1] *= sc; v[2] *= sc; v[3] *= sc;
    }
    T* __restrict__ yg = reinterpret_cast<T*>(p.y);
    const T* r1 = reinterpret_cast<const T*>(p.res1);
    const T* r2 = reinterpret_cast<const T*>(p.res2);
    const T* ms = reinterpret_cast<const T*>(p.mask_src);
    const long off = pix * p.ldy + co;
    if (vec_ok) {
        if (p.bias && add_bias) {
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + co);
            v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
        }
        float t[4];
        if (ms) {
            Elem<T>::ld4(ms + off, t);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= (t[r] > 0.f ? 1.f : p.mask_neg_slope);
        }
        if (r1) { Elem<T>::ld4(r1 + off, t); v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3]; }
        if (r2) { Elem<T>::ld4(r2 + off, t); v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3]; }
        apply_act_vec<4>(v, p.act);
        Elem<T>::st4(yg + off, v);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (co + r >= p.cout) break;
            float sv = v[r];
            if (p.bias && add_bias) sv += p.bias[co + r];
            if (ms) sv *= (Elem<T>::ld(ms + off + r) > 0.f ? 1.f : p.mask_neg_slope);
            if (r1) sv += Elem<T>::ld(r1 + off + r);
            if (r2) sv += Elem<T>::ld(r2 + off + r);
            Elem<T>::st(yg + off + r, apply_act(sv, p.act));
        }
    }
}

// 16 consecutive output channels of one pixel (the tall kernel's permuted fragment rows): 16-byte loads / stores.
template <typename T> struct Wide16;
template <> struct Wide16<bf16> {
    static __device__ __forceinline__ void ld(const bf16* p, float (&o)[16]) {
        const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 8);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) { o[2 * k] = bf16_bits_to_f32(w[k] & 0xffffu); o[2 * k + 1] = bf16_bits_to_f32(w[k] >> 16); }
    }
    static __device__ __forceinline__ void st(bf16* p, const float (&o)[16]) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = f32x2_to_bf16x2(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(p + 8) = make_uint4(w[4], w[5], w[6], w[7]);
    }
};
template <> struct Wide16<float> {
    static __device__ __forceinline__ void ld(const float* p, float (&o)[16]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float4 t = *reinterpret_cast<const float4*>(p + 4 * k); o[4 * k] = t.x; o[4 * k + 1] = t.y; o[4 * k + 2] = t.z; o[4 * k + 3] = t.w; }
    }
    static __device__ __forceinline__ void st(float* p, const float (&o)[16]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(p + 4 * k) = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
};
// bias / mask / residuals / activation of 16 consecutive channels of one pixel, in place (everything of the epilogue but the store)
template <typename T, bool TANH_OK = true>
__device__ __forceinline__ void conv_epilogue16_values(const sp_conv_params& p, float (&v)[16], long off, int co, bool add_bias = true) {
    const T* r1 = reinterpret_cast<const T*>(p.res1);
    const T* r2 = reinterpret_cast<const T*>(p.res2);
    const T* ms = reinterpret_cast<const T*>(p.mask_src);
    float t[16];
    if (p.bias && add_bias) {
        Wide16<float>::ld(p.bias + co, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] += t[r];
    }
    if (ms) {
        Wide16<T>::ld(ms + off, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] *= (t[r] > 0.f ? 1.f : p.mask_neg_slope);
    }
    if (r1) {
        Wide16<T>::ld(r1 + off, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] += t[r];
    }
    if (r2) {
        Wide16<T>::ld(r2 + off, t);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] += t[r];
    }
    apply_act_vec<16, TANH_OK>(v, p.act);
}
template <typename T>
__device__ __forceinline__ void conv_epilogue16(const sp_conv_params& p, float (&v)[16], long pix, int co, bool add_bias = true) {
    const long off = pix * p.ldy + co;
    if (p.img_scale != nullptr && add_bias) {
        const float sc = conv_img_scale(p, pix);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] *= sc;
    }
    conv_epilogue16_values<T>(p, v, off, co, add_bias);
    Wide16<T>::st(reinterpret_cast<T*>(p.y) + off, v);
}

// 2x2 average pooling fused into the epilogue (pool2): the two rows of a pair are two fragments of the SAME lane, the two
// columns sit in lanes l and l ^ 1 (DPP quad_perm [1,0,3,2]).  a / b: vertical sums of the column halves 0..15 / 16..31 of a
// 32-pixel row pair.  Even lanes finish the pooled pixel of half a, odd lanes the one of half b, so every lane stores one
// pooled pixel x 16 channels; bias / residuals / activation apply at the pooled resolution (conv_epilogue16 on pooled pixels).
__device__ __forceinline__ float dpp_xor1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
// pool2 == 2: 2x2 MAX pooling (the frozen VGG-16 stages: conv -> ReLU -> MaxPool; bias and a monotonic activation commute
// with the maximum, and so does the bf16 rounding: bit-identical to the separate pooling kernel).
__device__ __forceinline__ float pool2_combine(float x, float y, bool is_max) { return is_max ? fmaxf(x, y) : x + y; }
template <typename T>
__device__ __forceinline__ void conv_epilogue_pool2(const sp_conv_params& p, const float (&a)[16], const float (&b)[16], int lane,
                                                    long ppix_row, int pcol0, int co, bool add_bias = true) {
    // a co-tile past Cout (Cout % 16 == 0 is all the API asks of a pooled layer) has whole 16-channel groups outside the tensor: not
    // stored (they would land on the next pooled pixel; lanes l and l ^ 1 share their group, so the exchange below stays paired)
    if (co + 16 > p.cout) return;
    const bool odd = lane & 1;
    const bool is_max = p.pool2 == 2;
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float recv = dpp_xor1(odd ? a[c] : b[c]);
        const float mine = odd ? b[c] : a[c];
        v[c] = is_max ? fmaxf(mine, recv) : (mine + recv) * 0.25f;
    }
    conv_epilogue16<T>(p, v, ppix_row + pcol0 + (odd ? 8 : 0) + ((lane & 15) >> 1), co, add_bias);
}

// pool2 == 2 with sp_conv_params.pool_idx: the maximum AND its window position.  a0 / a1: the lane's column of half a in the upper /
// lower row of the pair, b0 / b1 likewise for half b (raw accumulators).  The position is the FIRST maximum in scan order
// (row 0: columns 0, 1; row 1: columns 0, 1 - a later element wins only if strictly greater, as in sp_maxpool2_bwd and torch) over
// the values the separate path would have stored and compared: accumulator (+ bias) rounded to the storage type (ReLU is monotonic
// and decides nothing where the maximum is positive; where it is not, the gradient is zero whatever the position).
template <typename T> __device__ __forceinline__ float round_to_storage(float v);
template <> __device__ __forceinline__ float round_to_storage<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to_storage<bf16>(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }
// two values at once (one packed conversion instead of two)
template <typename T> __device__ __forceinline__ void round_pair_to_storage(float& a, float& b);
template <> __device__ __forceinline__ void round_pair_to_storage<float>(float&, float&) {}
template <> __device__ __forceinline__ void round_pair_to_storage<bf16>(float& a, float& b) {
    const uint32_t w = f32x2_to_bf16x2(a, b);
    a = h16_lo_to_f32(w);
    b = h16_hi_to_f32(w);
}
template <typename T>
__device__ __forceinline__ void conv_epilogue_pool2_idx(const sp_conv_params& p, const float (&a0)[16], const float (&a1)[16],
                                                        const float (&b0)[16], const float (&b1)[16], int lane, long ppix_row, int pcol0,
                                                        int co, bool add_bias = true) {
    if (co + 16 > p.cout) return;
    const bool odd = lane & 1;
    float bias[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) bias[c] = 0.f;
    if (p.bias && add_bias) Wide16<float>::ld(p.bias + co, bias);
    // even lanes finish the pooled pixel of half a (they hold its even column, lane ^ 1 the odd one), odd lanes the one of half b.
    // Channel by channel (value and row flag travel through one DPP move each): nothing but v[] and idx lives across the loop -
    // these kernels have no register to spare beside their accumulators, and a spill would put scratch traffic on the counted
    // vmcnt waits of their LDS-DMA pipelines
    float v[16];
    unsigned idx = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float ra0 = a0[c] + bias[c], ra1 = a1[c] + bias[c], rb0 = b0[c] + bias[c], rb1 = b1[c] + bias[c];
        round_pair_to_storage<T>(ra0, ra1);
        round_pair_to_storage<T>(rb0, rb1);
        const bool fa = ra1 > ra0, fb = rb1 > rb0;                            // the vertical maximum sits in row 1 (only if strictly greater)
        const float ma = fa ? ra1 : ra0, mb = fb ? rb1 : rb0;
        const float mine = odd ? mb : ma;
        const int mine_row = (odd ? fb : fa) ? 1 : 0;
        const float recv = dpp_xor1(odd ? ma : mb);
        const int recv_row = __builtin_amdgcn_update_dpp(0, (odd ? fa : fb) ? 1 : 0, 0xB1, 0xF, 0xF, true);
        // column 0 of the window is the even lane's, column 1 the odd lane's
        const float m0 = odd ? recv : mine, m1 = odd ? mine : recv;
        const int r0 = odd ? recv_row : mine_row, r1 = odd ? mine_row : recv_row;
        const bool col1 = m1 > m0 || (m1 == m0 && r1 < r0);
        v[c] = col1 ? m1 : m0;
        idx |= (unsigned)(col1 ? (2 * r1 + 1) : (2 * r0)) << (2 * c);
    }
    const long ppix = ppix_row + pcol0 + (odd ? 8 : 0) + ((lane & 15) >> 1);
    p.pool_idx[ppix * (p.cout >> 4) + (co >> 4)] = idx;
    conv_epilogue16<T>(p, v, ppix, co, false);                            // (bias already added; no scale, mask or residuals with pool2 == 2)
}

// the kernels' buffer descriptors take 32-bit byte offsets: both operands (n*h*w*cin_p, cout*k*k*cin_p elements of `esz` bytes) below 1 GiB
inline bool conv_operands_below_1g(const sp_conv_params& p, long esz) {
    return (long)p.n * p.h * p.w_ * p.cin_p * esz < (1L << 30) && (long)p.cout * p.ksize * p.ksize * p.cin_p * esz < (1L << 30);
}

// ---- The forward route: the kernel sp_conv2d_igemm launches for a parameter block.  conv_igemm.hip's conv_plan() decides it without
// touching the device, dispatch() launches it, sp_conv2d_route() reports it.
constexpr int NUM_CU = 256;                   // MI355X: the persistent kernels run one block per CU, and time goes by rounds of them
enum ConvKernel { CK_UNSUPPORTED, CK_THINCO, CK_CIN8, CK_1X1_SPLITK, CK_1X1_DIRECT, CK_HALO_64, CK_HALO_128, CK_TALL_1_16, CK_TALL_2_16, CK_TALL_2_8,
                  CK_PP_8ROW, CK_PP_16ROW, CK_PP_W16, CK_PPW, CK_IGEMM_DMA, CK_IGEMM };
// the instantiation within the family, as bits (0: the general one).  FAST / TIMING / IDX / TAIL / F8: conv_pp.hip's template flags
// (IDX also the halo and tall kernels'); POOL / TIMING / LA: conv_ppw.hip's; SPLITK: the LDS-DMA igemm with its finalize pass
enum { CV_FAST = 1, CV_TIMING = 2, CV_IDX = 4, CV_TAIL = 8, CV_F8 = 16, CV_POOL = 32, CV_LA = 64, CV_SPLITK = 128 };
struct ConvRoute {
    int kernel, form;               // ConvKernel, CV_* bits
    int co_t, px_t, ksplit;         // the igemm kernels' output tile, the LDS-DMA one's K splits
    const char* error;              // CK_UNSUPPORTED: the message
};
// sp_last_route() / sp_conv2d_route(): the one place the names live - bench.py's route tables and the tests match on them
inline const char* conv_route_name(int kernel, int form, bool f32) {
    switch (kernel) {
        case CK_THINCO: return "conv3x3_thinco";
        case CK_CIN8: return "conv3x3_cin8";
        case CK_1X1_SPLITK: return "conv1x1_splitk";
        case CK_1X1_DIRECT: return "conv1x1_direct";
        case CK_HALO_64: case CK_HALO_128: return f32 ? "conv3x3_halo<f32>" : "conv3x3_halo<16bit>";
        case CK_TALL_1_16: return f32 ? "conv3x3_tall<f32,1,16>" : "conv3x3_tall<16bit,1,16>";
        case CK_TALL_2_16: return f32 ? "conv3x3_tall<f32,2,16>" : "conv3x3_tall<16bit,2,16>";
        case CK_TALL_2_8: return f32 ? "conv3x3_tall<f32,2,8>" : "conv3x3_tall<16bit,2,8>";
        case CK_PP_8ROW: return (form & CV_F8) ? "conv3x3_pp<f8,2>" : (form & CV_FAST) ? "conv3x3_pp<16bit,2,FAST>" : "conv3x3_pp<16bit,2>";
        case CK_PP_16ROW: return (form & CV_FAST) ? "conv3x3_pp<16bit,1,FAST>" : "conv3x3_pp<16bit,1>";
        case CK_PP_W16: return "conv3x3_pp<16bit,2,FAST,w16>";
        case CK_PPW: return "conv3x3_ppw<16bit> (64 co x 4 rows per wave)";
        case CK_IGEMM_DMA: return (form & CV_SPLITK) ? "conv_igemm_dma+finalize (split-K)" : "conv_igemm_dma";
        case CK_IGEMM: return "conv_igemm (register-staged)";
    }
    return "";
}

// Work items of the ping-pong forms on these dims, 0 where the form does not take them: the admission of its launcher on the dims
// (sp_conv_pp_form / sp_conv_ppw_form add the epilogue's), shared with sp_conv2d_workspace().
inline long pp_items_8row(int n, int h, int w, int cout) {            // conv_pp.hip: 128 co x 8 x 32 px
    return h % 8 != 0 || w % 32 != 0 || cout <= 64 ? 0 : (long)n * (h / 8) * (w / 32) * ((cout + 127) / 128);
}
inline long pp_items_16row(int n, int h, int w, int cout) {           // conv_pp.hip: 64 co x 16 x 32 px
    return h % 16 != 0 || w % 32 != 0 || cout <= 16 || cout > 64 ? 0 : (long)n * (h / 16) * (w / 32);
}
inline long pp_items_w16(int n, int h, int w, int cout) {             // conv_pp.hip: 128 co x 16 x 16 px, maps 16 wide, >= 64 items
    const long items = (long)n * (h / 16) * ((cout + 127) / 128);
    return w != 16 || h % 16 != 0 || cout <= 64 || items < 64 ? 0 : items;
}
inline long ppw_items(int n, int h, int w, int cout) {                // conv_ppw.hip: 128 co x 16 x 32 px
    return h % 16 != 0 || w % 32 != 0 || cout <= 64 ? 0 : (long)n * (h / 16) * (w / 32) * ((cout + 127) / 128);
}
inline long pp_items(int kernel, int n, int h, int w, int cout) {     // ... by form (CK_PP_8ROW / CK_PP_16ROW / CK_PP_W16)
    return kernel == CK_PP_W16 ? pp_items_w16(n, h, w, cout) : kernel == CK_PP_16ROW ? pp_items_16row(n, h, w, cout) : pp_items_8row(n, h, w, cout);
}

// ---- K-split of the LAST, partial round of a ping-pong launch ("tail split"; the scheme and its hand-over: the top of conv_pp.hip).
// The plan serves the launchers and sp_conv2d_workspace(), the piece decoding below the kernels.
constexpr int SK_MAX_PARTS = 4;
// The last round takes `chunk` per 32-channel chunk of its longest piece plus, per piece handed over, `near` (two full rounds or more
// in front of the owner's piece hide more of it) or `far`; a piece is `slab_floats` fp32 values (8 waves x 64 lanes x accumulators).
struct TailSplitModel { long chunk, near, far; int slab_floats; };
// conv_pp.hip's items, 64 accumulators: ~3.7 us per chunk, 4 - 6 us per piece handed over - the slabs of P - 1 contributors drain
// through the memory side, the owner fetches them one round trip each (measured, profiles/README.md round 6)
constexpr TailSplitModel SK_PP = {37, 40, 60, 8 * 64 * 64};
// conv_ppw.hip's 16-row items, 128 accumulators: ~1.8 x an 8-row item (6.7 us per chunk), a piece handed over ~1.5 x (twice the
// bytes, the same latency chain)
constexpr TailSplitModel SK_PPW = {67, 60, 90, 8 * 64 * 128};

struct TailSplit { int parts, tail_items, grid; };
// the plan for `total` items of `kchunks` chunks each; parts <= 1: no split (grid: the unsplit launch's).  total < 256 (less than one
// round: e.g. 80 items of 128 co x 16 x 16 px for 512 -> 512 on 16 x 16 maps at batch 20): every item is a tail item and the grid is
// tail_items * parts blocks of one piece each (SP_TUNE_CONV_PP_SPLIT = 2 keeps the split to launches of at least one full round).
inline TailSplit tail_split_plan(int total, int kchunks, const TailSplitModel& m, long workspace_bytes) {
    TailSplit r{0, 0, total < NUM_CU ? total : NUM_CU};
    // (less than one round: one block per item - rounded down to a multiple of 8 for the XCD remap, 100 items became 96 blocks of
    // which four took two items, i.e. two rounds; the kernels skip the remap when the grid is not a multiple of 8)
    const int mode = sp_tune(SP_TUNE_CONV_PP_SPLIT, 1);
    if (!mode || total <= 0 || (total < NUM_CU && mode == 2)) return r;
    const int R = total % NUM_CU;
    if (R == 0) return r;
    int pmax = NUM_CU / R;
    if (pmax > SK_MAX_PARTS) pmax = SK_MAX_PARTS;
    // a piece has at least two chunks, and the split must save at least a twentieth of the round
    int P = 1;
    long best = m.chunk * kchunks;
    const long handover = total >= 2 * NUM_CU ? m.near : m.far;
    for (int q = 2; q <= pmax && kchunks / q >= 2; ++q) {
        const long c = m.chunk * ((kchunks + q - 1) / q) + handover * (q - 1);
        if (c < best && 20 * c < 19 * m.chunk * kchunks) { best = c; P = q; }
    }
    if (P < 2 || (long)R * P * m.slab_floats * 4 > workspace_bytes) return r;
    r.parts = P; r.tail_items = R;
    r.grid = total < NUM_CU ? R * P : NUM_CU;
    return r;
}
// sp_conv2d_workspace(): bytes of fp32 scratch with which a launch of `items` items splits its last round (0: it would not)
inline long tail_split_bytes(long items, int kchunks, const TailSplitModel& m) {
    if (items >= (1L << 30)) return 0;
    const TailSplit sk = tail_split_plan((int)items, kchunks, m, 1L << 40);
    return (long)sk.tail_items * sk.parts * m.slab_floats * 4;
}
// the kernels' sk_arg: pieces per tail item; bit 8 with SP_TUNE_CONV_PP_SPLIT = 3 (tests): the closing piece stores and counts like
// every other piece, so the re-read order runs on every split launch
inline int tail_split_arg(const TailSplit& sk) { return sk.parts | (sp_tune(SP_TUNE_CONV_PP_SPLIT, 1) == 3 ? 256 : 0); }

// dispatch(): what a launch of `total` 8-row items (conv_pp.hip) costs, in hundredths of the time of one item on every CU - whole rounds
// without the split; with it the longest piece of the last round plus the hand-over of the partial tiles.  This price does not follow
// the plan exactly: it takes 100 / P of an item for the longest piece where the plan takes ceil(kchunks / P) / kchunks, and prices a
// hand-over at 162 / kchunks (the far cost, 60 / 37) also where the plan takes the near one (total >= 512).  Making the two agree moves
// launches between the 8-row and the 16-row kernel: a change to measure on its own.
inline long pp_rounds100(long total, int cin_p, long workspace_bytes) {
    const int kchunks = (cin_p + 31) / 32;
    if (total < (1L << 30)) {
        const TailSplit sk = tail_split_plan((int)total, kchunks, SK_PP, workspace_bytes);
        if (sk.parts > 1 && total >= NUM_CU) return 100 * (total / NUM_CU) + 100 / sk.parts + 162 * (sk.parts - 1) / kchunks + 1;
    }
    return 100 * ((total + NUM_CU - 1) / NUM_CU);
}

// The piece decoding in the kernels: sk_arg first thing, then (assign) the block's share - the first full_total items go round robin as
// ever (`bid`: the XCD-remapped block index of a grid of `grid`), the rest in K pieces: piece `part` of tail item j runs on the block
// with the PHYSICAL index j * parts + part.  The order of these steps and of the locals in assign() is the order the kernels were
// tuned with: it decides the code the compiler emits for them, register allocation included.
struct TailPiece {
    int parts;                      // pieces per tail item (0 / 1: no split)
    bool peek;                      // the closing piece looks at the counter first (tail_split_arg)
    int my_items;                   // this block's full items
    bool has_tail;                  // its tail piece, if any:
    int item, j, part, k0, k1;      //   item number (-1: none), tail index, piece, chunks [k0, k1)
    bool owner;                     // the piece that adds the others and runs the epilogue
    int nchunks;                    // the block's chunks of work

    __device__ __forceinline__ explicit TailPiece(int sk_arg) : parts(sk_arg & 255), peek(!(sk_arg & 256)) {}
    __device__ __forceinline__ void assign(int total, int grid, int bid, int kchunks) {
        const int full_total = parts > 1 ? (total / grid) * grid : total;
        my_items = (full_total - bid + grid - 1) / grid;
        int t_j = 0, t_k1 = 0, t_k0 = 0, t_part = 0, t_item = -1;
        if (parts > 1 && (int)blockIdx.x < (total - full_total) * parts) {
            t_j = (int)blockIdx.x / parts;
            t_part = (int)blockIdx.x - t_j * parts;
            t_item = full_total + t_j;
            t_k0 = t_part * kchunks / parts;
            t_k1 = (t_part + 1) * kchunks / parts;
        }
        item = t_item; part = t_part; k0 = t_k0; k1 = t_k1; j = t_j;
        has_tail = t_item >= 0;
        owner = t_part == parts - 1;
        nchunks = my_items * kchunks + (has_tail ? t_k1 - t_k0 : 0);
    }
};

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int OFF> __device__ __forceinline__ void lds_rd128(uint4& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
template <int N> __device__ __forceinline__ void wait_lgkm() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace
