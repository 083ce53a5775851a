// Skinny linear layers (batch <= 32 rows per tile): y = act(x W^T + b + res), weight-bandwidth bound.
// Replaces nn.Linear at models.py:28,128,132,356,359 and the VGG-16 classifier (models.py:210-213);
// with the transposed packing it is also the input-gradient pass.  One wave owns NR output features
// and streams their packed weight rows with 16-byte loads; the activation chunk (B x 512) is staged
// once per block in LDS as fp32, so rows of x may have any pitch/alignment (K = 365 occurs).
#include <type_traits>
#include <utility>
#include "common.h"

namespace {

constexpr int LIN_KC = 512;     // k per LDS chunk
constexpr int LIN_BMAX = 32;
constexpr int LIN_NB = 8;       // output features per block
constexpr int LIN_PITCH = LIN_KC + 1;

// thread = (output feature tid >> 5, batch row tid & 31): the 32 lanes of a half-wave read the same 16 bytes of the weight
// row (one broadcast load) and 32 different activation rows from LDS (pitch 513 floats: conflict free); no cross-lane
// reduction.  The activation chunk is staged as fp32 with scalar loads, so rows of x may have any pitch / alignment
// (K = 365 occurs); packed weight rows are zero-padded to kp (a multiple of 8).
template <typename T>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ wp, int kp,
                                                         const float* __restrict__ bias, const T* __restrict__ res,
                                                         T* __restrict__ y, int ldy, int B, int K, int N, int act) {
    extern __shared__ __attribute__((aligned(16))) float xs[];     // [LIN_BMAX][LIN_PITCH]
    const int tid = threadIdx.x;
    const int b = tid & 31, nl = tid >> 5;
    const int b0 = blockIdx.y * LIN_BMAX;
    const int nb = min(LIN_BMAX, B - b0);
    const int n = blockIdx.x * LIN_NB + nl;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += LIN_KC) {
        __syncthreads();
        for (int e = tid; e < LIN_BMAX * LIN_KC; e += 256) {
            const int bb = e / LIN_KC, k = e - bb * LIN_KC;
            float v = 0.f;
            if (bb < nb && k0 + k < K) v = Elem<T>::ld(x + (long)(b0 + bb) * ldx + k0 + k);
            xs[bb * LIN_PITCH + k] = v;
        }
        __syncthreads();
        if (n < N) {
            const int kend = min(LIN_KC, kp - k0);
            const T* wr = wp + (long)n * kp + k0;
            const float* xr = xs + b * LIN_PITCH;
            for (int kk = 0; kk < kend; kk += 8) {
                float w8[8];
                Elem<T>::ld4(wr + kk, w8);
                Elem<T>::ld4(wr + kk + 4, w8 + 4);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += w8[q] * xr[kk + q];
            }
        }
    }
    if (n < N && b < nb) {
        float v = acc + (bias ? bias[n] : 0.f);
        const long off = (long)(b0 + b) * ldy + n;
        if (res) v += Elem<T>::ld(res + off);
        Elem<T>::st(y + off, apply_act(v, act));
    }
}

// dW[n][k] = sum_b dy[b][n] * x[b][k]  (fp32, layout [N][kp]);  db[n] = sum_b dy[b][n]
constexpr int LW_NR = 8;
template <typename T>
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int ldd,
                                                           float* __restrict__ dw, int kp, float* __restrict__ db, int B,
                                                           int K, int N) {
    // a thread owns FOUR consecutive columns k .. k + 3 of LW_NR consecutive rows: x[b][k..] is loaded once per batch row (8 / 16
    // bytes) and reused for all rows, the fp32 results leave as 16-byte stores.  The dy[b][n0..n0+8) values every thread needs are
    // staged in LDS once, and the x loads of four batch rows are in flight together: the plain loop over the batch was a chain of
    // B dependent round trips (load -> wait -> 32 FMAs), 24 us for a layer whose operands and output are a few megabytes.
    // History: one row per thread re-read x for every output row (86 us on the 4096 x 2048 layer); one column per thread stored
    // 4 bytes per lane (24.6 us); four columns per thread: 24.1 us (not store bound either); this form: round 4.
    __shared__ float dys[32][LW_NR];
    const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int n0 = blockIdx.y * LW_NR;
    const bool live = k < kp;
    float acc[LW_NR][4], bs[LW_NR];
#pragma unroll
    for (int j = 0; j < LW_NR; ++j) { acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f; bs[j] = 0.f; }
    const bool vec = k + 4 <= K && ((ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
    for (int b0 = 0; b0 < B; b0 += 32) {
        const int nb = min(32, B - b0);
        __syncthreads();
        {
            const int bb = threadIdx.x / LW_NR, j = threadIdx.x % LW_NR;
            dys[bb][j] = (bb < nb && n0 + j < N) ? Elem<T>::ld(dy + (long)(b0 + bb) * ldd + n0 + j) : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        for (int b = 0; b < nb; b += 4) {
            float xv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xv[u][0] = xv[u][1] = xv[u][2] = xv[u][3] = 0.f;
                // (unconditional: a batch row past the group re-reads its last row - its dy values in LDS are zeros; a load under
                // `if (b + u < nb)` cost an exec branch and a full `vmcnt(0)` each)
                const int br = b + u < nb ? b + u : nb - 1;
                const T* xr = x + (long)(b0 + br) * ldx + k;
                if (vec) Elem<T>::ld4(xr, xv[u]);
                else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (k + q < K) xv[u][q] = Elem<T>::ld(xr + q);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int j = 0; j < LW_NR; ++j) {
                    const float d = dys[b + u][j];
                    bs[j] += d;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[j][q] += d * xv[u][q];
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < LW_NR; ++j) {
        if (n0 + j >= N) break;
        *reinterpret_cast<float4*>(dw + (long)(n0 + j) * kp + k) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);   // kp % 8 == 0, k % 4 == 0
        if (db && k == 0) db[n0 + j] = bs[j];
    }
}

// ---- bf16 MFMA split-K path for the big weight matrices (VGG classifier 25088x4096 / 4096x4096, G 4096x2048):
// D[n][b] += sum_{k in slice} Wp[n][k] x[b][k].  The weight rows are the MFMA A operand and are read straight from
// HBM in fragment order (lane = (row, 8 consecutive k), 16 bytes each, 16 loads in flight per lane); the batch slice
// x[0..32)[k-slice] is the B operand, staged once per block in LDS.  grid = (N/128, K/kslice): hundreds of blocks
// stream disjoint weight panels concurrently; partial sums meet in an fp32 scratch via atomics, a second tiny
// kernel applies bias / residual / activation.
// LM_KS = k per block: 1024 for very long rows (25 splits of the 25088-wide classifier input), 512 otherwise (4096-wide
// layers: 8 splits x 32 row tiles = 256 blocks instead of 128)

// the layer's epilogue, for launches whose single K-split finishes the layer itself (y != nullptr: no slab, no finalize pass)
template <int... I, typename F>
__device__ __forceinline__ void lin_static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void lin_static_for(F&& f) { lin_static_for_impl(std::make_integer_sequence<int, N>{}, f); }

struct LinTail { const float* bias; const bf16* res; bf16* y; int ldy, act; };

// NB = 16-row batch fragments per block: 2 (up to 32 rows) or 4 (up to 64 - round 5: the two-batch VGG-16 pass hands its 40 / 64 rows
// over in ONE launch, so FC1's 205 MB of weights are streamed once instead of once per group)
template <int LM_KS, int NB = 2>
__global__ __launch_bounds__(256) void linear_mfma_kernel(const bf16* __restrict__ x, int ldx, const bf16* __restrict__ wp, int kp,
                                                          float* __restrict__ acc_out, int B, int K, int N, LinTail tail) {
    // the x tile is staged XS columns at a time (two phases for a 1024-wide K range): [16 * NB][XS] in LDS stays at 33 / 66 KB, so two
    // blocks share a CU and one streams while the other stages, multiplies or stores its slab
    constexpr int XS = LM_KS < 512 ? LM_KS : 512;
    constexpr int LM_PITCH = XS * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) char xs_raw[];     // [16 * NB][LM_PITCH bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 128 + wave * 32;
    const int k0 = blockIdx.y * LM_KS;
    const int klen = min(LM_KS, kp - k0);                            // multiple of 8 (kp is)
    const int frow = lane & 15, g = lane >> 4;
    const bf16* wrow[2];
    bool wok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + i * 16 + frow;
        wok[i] = n < N;
        wrow[i] = wp + (long)(wok[i] ? n : 0) * kp + k0 + g * 8;
    }
    // The weights are the traffic (a block streams 128 rows x LM_KS once; the x tile is re-read from L2 by every block): their loads run
    // LA groups of U k-steps ahead of the MFMAs through a ring of LA + 1 register sets, the first LA groups are requested right behind
    // the loads of the x tile and before it is staged (round 5: the single-buffered loop had a block's 64 KB in flight, then nothing
    // while it multiplied; FC1 of the VGG-16 classifier streamed at 1.7 TB/s).  Every load is UNCONDITIONAL: under a per-lane
    // condition hipcc wrapped each one in an exec branch and followed some with `s_waitcnt vmcnt(0)` + a register copy.  A lane
    // whose k-chunk lies past the K range re-reads the range's first chunk of its own row instead - its x counterpart is zero
    // padding, and a non-finite weight there belongs to the same row's sum anyway; rows past N read row 0 and are never stored.
    constexpr int U = 4, LA = 3, NBUF = LA + 1;
    constexpr int NG = LM_KS / 32 / U;                                // groups of a full K range
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    uint4 a[NBUF][2][U];
    auto load_group = [&](uint4 (&dst)[2][U], int q) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = q * U + u;
            const bool k_ok = kk * 32 + g * 8 < klen;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16* src = k_ok ? wrow[i] + kk * 32 : wrow[i] - g * 8;
                const u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(src));     // streamed once: FC1's 205 MB need not sweep the L2
                dst[i][u] = make_uint4(t.x, t.y, t.z, t.w);
            }
        }
    };
    // x[0..16 NB)[k0 + phase * XS ..) (zero padded): loads into registers first, the LDS writes once they have landed
    const bool vec = ((ldx & 7) == 0) && ((K & 7) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);     // whole 16-byte chunks only
    constexpr int XCH = 16 * NB * (XS / 8) / 256;                     // 16-byte chunks per thread and phase
    static_assert(XCH * 256 == 16 * NB * (XS / 8), "x tile: whole chunks per thread");
    uint4 xv[XCH];
    auto x_issue = [&](int ph) {
#pragma unroll
        for (int c = 0; c < XCH; ++c) {
            const int e = c * 256 + tid;
            const int b = e / (XS / 8), kl = (e - b * (XS / 8)) * 8, kc = ph * XS + kl;
            const bool ok = b < B && kc < klen && k0 + kc + 8 <= K;
            const u32x4_t t = *reinterpret_cast<const u32x4_t*>(x + (ok ? (long)b * ldx + k0 + kc : 0L));
            xv[c] = ok ? make_uint4(t.x, t.y, t.z, t.w) : make_uint4(0, 0, 0, 0);
        }
    };
    auto x_commit = [&](int ph) {
#pragma unroll
        for (int c = 0; c < XCH; ++c) {
            const int e = c * 256 + tid;
            const int b = e / (XS / 8), kl = (e - b * (XS / 8)) * 8, kc = ph * XS + kl;
            *reinterpret_cast<uint4*>(xs_raw + b * LM_PITCH + kl * 2) = xv[c];
        }
    };
    auto x_stage_slow = [&](int ph) {                                 // unaligned rows (ldx % 8 != 0) or K % 8 != 0: element loads
        for (int e = tid; e < 16 * NB * (XS / 8); e += 256) {
            const int b = e / (XS / 8), kl = (e - b * (XS / 8)) * 8, kc = ph * XS + kl;
            uint16_t t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = (b < B && kc < klen && k0 + kc + q < K) ? x[(long)b * ldx + k0 + kc + q].v : (uint16_t)0;
            *reinterpret_cast<uint4*>(xs_raw + b * LM_PITCH + kl * 2) = make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
        }
    };
    if (vec) x_issue(0);
    lin_static_for<(LA < NG ? LA : NG)>([&](auto qc) { load_group(a[decltype(qc)::value], decltype(qc)::value); });
    if (vec) x_commit(0); else x_stage_slow(0);
    __syncthreads();
    f32x4_t acc[2][NB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto mma_group = [&](const uint4 (&src)[2][U], int q) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = q * U + u;
            uint4 bx[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j)
                bx[j] = *reinterpret_cast<const uint4*>(xs_raw + (j * 16 + frow) * LM_PITCH + ((kk * 32) % XS + g * 8) * 2);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, src[i][u]), __builtin_bit_cast(bf16x8_t, bx[j]),
                                                                        acc[i][j], 0, 0, 0);
        }
    };
    constexpr int GPP = XS / 32 / U;                                  // groups per staging phase
    lin_static_for<NG>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if constexpr (q > 0 && q % GPP == 0) {                        // next phase of the x tile (every wave is done reading the previous one)
            if (vec) x_issue(q / GPP);
            if constexpr (q + LA < NG) load_group(a[(q + LA) % NBUF], q + LA);
            __syncthreads();
            if (vec) x_commit(q / GPP); else x_stage_slow(q / GPP);
            __syncthreads();
        } else {
            if constexpr (q + LA < NG) load_group(a[(q + LA) % NBUF], q + LA);
        }
        mma_group(a[q % NBUF], q);
    });
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int b = j * 16 + (lane & 15);
            if (b >= B) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + i * 16 + (lane >> 4) * 4 + r;
                if (n >= N) continue;
                if (tail.y == nullptr) {
                    acc_out[((long)blockIdx.y * B + b) * N + n] = acc[i][j][r];            // this K-split's slab [B][N]
                } else {                                                                     // the only K-split: the layer's epilogue
                    const long off = (long)b * tail.ldy + n;
                    float v = acc[i][j][r] + (tail.bias ? tail.bias[n] : 0.f);
                    if (tail.res) v += Elem<bf16>::ld(tail.res + off);
                    Elem<bf16>::st(tail.y + off, apply_act(v, tail.act));
                }
            }
        }
}

template <typename T>
__global__ void linear_finalize_kernel(const float* __restrict__ acc, int nsplit, const float* __restrict__ bias, const T* __restrict__ res,
                                       T* __restrict__ y, int ldy, int B, int N, int act) {
    const long total = (long)B * N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int b = (int)(e / N), n = (int)(e - (long)b * N);
        float v = bias ? bias[n] : 0.f;
#pragma unroll 8
        for (int z = 0; z < nsplit; ++z) v += acc[z * total + e];
        const long off = (long)b * ldy + n;
        if (res) v += Elem<T>::ld(res + off);
        Elem<T>::st(y + off, apply_act(v, act));
    }
}

}  // namespace

// K per block: 1024 for the 25088-wide classifier input, 512 for the 2048 / 4096-wide layers, 128 for the small ones (a
// 768 -> 128 layer then runs on 6 blocks + the finalize pass instead of 16 single-wave dot-product loops: 25 -> ~8 us)
// Rows of up to 1024 values take ONE split (K per block = the smallest of 128 / 512 / 1024 that covers the row): the block applies
// bias / residual / activation from its registers and the finalize launch - ~5 us of queue time, as much as the layer itself - is gone
// (the latent / linear-block 128 -> 128 layers, D's 768 -> 128, the 365 -> 128 class mapping and their input gradients).
// Larger matrices - K range per block of the split-K MFMA kernel: the widest of 1024 / 512 / 256 / 128 that still yields LIN_MIN_BLOCKS = 256 blocks (measured per shape, scratch/bench_linear.py; blocks
// keep the weight stream going while a neighbour stages its x tile or stores its slab; a wider range means fewer fp32 slabs - every
// split writes and the finalize pass re-reads batch x n floats); SP_TUNE_LINEAR_KS forces a width
constexpr int LIN_MIN_BLOCKS = 256;
static inline int linear_ks(int kp, int n) {
    const int forced = sp_tune(SP_TUNE_LINEAR_KS, 0);
    if (forced == 1024 || forced == 512 || forced == 256 || forced == 128) return forced;
    const long nt = (n + 127) / 128;
    // small layers (the rule above): one split, no finalize launch - the widths this kernel is instantiated for that cover the row
    if ((long)n * kp <= (1L << 18) && kp <= 1024) return kp > 512 ? 1024 : (kp > 256 ? 512 : (kp > 128 ? 256 : 128));
    for (int ks = 1024; ks > 128; ks >>= 1)
        if (nt * ((kp + ks - 1) / ks) >= LIN_MIN_BLOCKS) return ks;
    return 128;
}
static inline bool linear_use_mfma(int dtype, int batch, int k, int n) { return dtype == SP_BF16 && batch <= 64 && (long)k * n >= (1L << 12); }

template <int KS, int NB>
static void launch_linear_mfma_nb(dim3 grid, hipStream_t s, const bf16* x, int ldx, const bf16* w, int kp, float* scratch, int batch, int k, int n,
                                  const LinTail& tail) {
    const int lds = 16 * NB * ((KS < 512 ? KS : 512) * 2 + 16);
    (void)sp_lds_limit<linear_mfma_kernel<KS, NB>>(lds);          // (a refusal shows as the launch error the caller checks for)
    hipLaunchKernelGGL((linear_mfma_kernel<KS, NB>), grid, dim3(256), lds, s, x, ldx, w, kp, scratch, batch, k, n, tail);
}

template <int KS>
static void launch_linear_mfma(dim3 grid, hipStream_t s, const bf16* x, int ldx, const bf16* w, int kp, float* scratch, int batch, int k, int n,
                               const LinTail& tail) {
    if (batch <= 32) launch_linear_mfma_nb<KS, 2>(grid, s, x, ldx, w, kp, scratch, batch, k, n, tail);
    else launch_linear_mfma_nb<KS, 4>(grid, s, x, ldx, w, kp, scratch, batch, k, n, tail);
}

extern "C" int sp_linear_fwd(const void* x, int32_t ldx, const void* w_packed, int32_t kp, const float* bias,
                             const void* res, void* y, int32_t ldy, int32_t batch, int32_t k, int32_t n, int32_t act,
                             int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(x && w_packed && y, "sp_linear_fwd: null pointer");
    SP_CHECK_ARG(batch > 0 && k > 0 && n > 0 && kp >= k && ldx >= k && ldy >= n, "sp_linear_fwd: bad dims");
    SP_CHECK_ARG(dtype == SP_F32 || dtype == SP_BF16, "sp_linear_fwd: bad dtype %d", dtype);
    SP_CHECK_ARG(kp % 8 == 0, "sp_linear_fwd: kp=%d must be a multiple of 8", kp);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid(sp_div_up(n, LIN_NB), sp_div_up(batch, LIN_BMAX));
    const int lds = LIN_BMAX * LIN_PITCH * sizeof(float);
    if (dtype == SP_F32) {
        if (const int rc = sp_lds_limit<linear_fwd_kernel<float>>(lds)) return rc;
        hipLaunchKernelGGL(linear_fwd_kernel<float>, grid, dim3(256), lds, s, (const float*)x, ldx, (const float*)w_packed, kp, bias,
                           (const float*)res, (float*)y, ldy, batch, k, n, act);
    } else {
        if (const int rc = sp_lds_limit<linear_fwd_kernel<bf16>>(lds)) return rc;
        hipLaunchKernelGGL(linear_fwd_kernel<bf16>, grid, dim3(256), lds, s, (const bf16*)x, ldx, (const bf16*)w_packed, kp, bias,
                           (const bf16*)res, (bf16*)y, ldy, batch, k, n, act);
    }
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_linear_wgrad(const void* x, int32_t ldx, const void* dy, int32_t ld_dy, float* dw, int32_t kp,
                               float* dbias, int32_t batch, int32_t k, int32_t n, int32_t dtype, sp_stream_t stream) {
    SP_CHECK_ARG(x && dy && dw, "sp_linear_wgrad: null pointer");
    SP_CHECK_ARG(batch > 0 && k > 0 && n > 0 && kp >= k, "sp_linear_wgrad: bad dims");
    SP_CHECK_ARG(dtype == SP_F32 || dtype == SP_BF16, "sp_linear_wgrad: bad dtype %d", dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SP_CHECK_ARG(kp % 4 == 0 && (reinterpret_cast<uintptr_t>(dw) & 15) == 0, "sp_linear_wgrad: kp %% 4 == 0 and a 16-byte aligned dw are required");
    dim3 grid(sp_div_up(kp, 1024), sp_div_up(n, LW_NR));
    if (dtype == SP_F32)
        hipLaunchKernelGGL(linear_wgrad_kernel<float>, grid, dim3(256), 0, s, (const float*)x, ldx, (const float*)dy, ld_dy, dw, kp, dbias, batch, k, n);
    else
        hipLaunchKernelGGL(linear_wgrad_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, ldx, (const bf16*)dy, ld_dy, dw, kp, dbias, batch, k, n);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_linear_fwd_ws(const void* x, int32_t ldx, const void* w_packed, int32_t kp, const float* bias,
                                const void* res, void* y, int32_t ldy, int32_t batch, int32_t k, int32_t n, int32_t act,
                                int32_t dtype, float* scratch, sp_stream_t stream) {
    // big bf16 matrices: MFMA split-K, one fp32 slab [batch][n] per K-split in the caller's scratch (plain stores, summed by
    // the finalize pass; the first version met in one slab through atomics after a fill); everything else: the direct kernel
    const bool big = scratch != nullptr && linear_use_mfma(dtype, batch, k, n);
    if (!big) return sp_linear_fwd(x, ldx, w_packed, kp, bias, res, y, ldy, batch, k, n, act, dtype, stream);
    SP_CHECK_ARG(x && w_packed && y, "sp_linear_fwd_ws: null pointer");
    SP_CHECK_ARG(batch > 0 && k > 0 && n > 0 && kp >= k && kp % 8 == 0 && ldx >= k && ldy >= n, "sp_linear_fwd_ws: bad dims");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ks = linear_ks(kp, n);
    const int nsplit = sp_div_up(kp, ks);
    dim3 grid(sp_div_up(n, 128), nsplit);
    const LinTail tail{bias, (const bf16*)res, nsplit == 1 ? (bf16*)y : nullptr, ldy, act};
    if (ks == 1024) launch_linear_mfma<1024>(grid, s, (const bf16*)x, ldx, (const bf16*)w_packed, kp, scratch, batch, k, n, tail);
    else if (ks == 512) launch_linear_mfma<512>(grid, s, (const bf16*)x, ldx, (const bf16*)w_packed, kp, scratch, batch, k, n, tail);
    else if (ks == 256) launch_linear_mfma<256>(grid, s, (const bf16*)x, ldx, (const bf16*)w_packed, kp, scratch, batch, k, n, tail);
    else launch_linear_mfma<128>(grid, s, (const bf16*)x, ldx, (const bf16*)w_packed, kp, scratch, batch, k, n, tail);
    SP_LAUNCH_CHECK();
    if (nsplit == 1) return SP_OK;
    int fb = sp_div_up((long)batch * n, 256);
    if (fb > 1024) fb = 1024;
    hipLaunchKernelGGL(linear_finalize_kernel<bf16>, dim3(fb), dim3(256), 0, s, scratch, nsplit, bias, (const bf16*)res, (bf16*)y, ldy, batch, n, act);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_linear_workspace(int32_t batch, int32_t k, int32_t n, int32_t dtype, int64_t* floats_out) {
    SP_CHECK_ARG(floats_out && batch > 0 && k > 0 && n > 0, "sp_linear_workspace: bad args");
    const int kp = (k + 7) / 8 * 8;
    const bool big = linear_use_mfma(dtype, batch, k, n);
    *floats_out = big ? (int64_t)sp_div_up(kp, linear_ks(kp, n)) * batch * n : 0;      // (ask again after changing SP_TUNE_LINEAR_KS)
    return SP_OK;
}
