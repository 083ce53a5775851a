// Multi-tensor Adam: every parameter of a network in ONE launch (torch.optim.Adam at main.py:64-65, .step() at
// model_wrapper.py:162,190 - the reference runs torch's per-tensor / foreach kernels: hundreds of launches per step).
// The host splits the tensors into chunks of <= 65536 elements; one block per chunk, so small tensors (biases,
// u / v vectors) cost one short block each and the big weight matrices spread over many.  Update rule and
// operation order follow torch/optim/adam.py (_single_tensor_adam, amsgrad = False, maximize = False):
//   g'  = g + wd * p
//   m  += (g' - m) * (1 - beta1)                      (Tensor.lerp_)
//   v   = v * beta2 + (1 - beta2) * g' * g'           (mul_ + addcmul_)
//   p  -= step_size * m / (sqrt(v) / sqrt(bc2) + eps), step_size = lr / bc1  (per-tensor scalars: the step count is
//                                                      per parameter, so they travel in the chunk table)
// Beside it, in the same one-block-per-chunk form: the exponential moving average of a network's parameters and the in-place exchange
// that evaluates it (sp_ema_multi / sp_swap_multi; the reference has no average).
#include "common.h"

namespace {

// g * coef rounded to fp32 ONCE (sp_adam_multi_clipped): the empty asm makes the product a value of its own, so that it cannot be
// contracted into the g - m or g + wd * p that follows (hipcc contracts across statements, and __fmul_rn is a plain product in this
// toolchain's headers).  g * 1.0f is g.
__device__ __forceinline__ float mul_rounded_once(float g, float coef) {
    float r = __fmul_rn(g, coef);
    asm("" : "+v"(r));
    return r;
}

// CLIP (sp_adam_multi_clipped): clip = {norm, coefficient, skip flag, ...} of sp_grad_clip_finalize - nothing is done when clip[2] != 0
// either, and every gradient is read as fp32(g * clip[1]).  CLIP = false is the kernel sp_adam_multi / sp_adam_multi_guarded always had.
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_multi_kernel(const sp_adam_chunk* __restrict__ chunks, float omb1, float beta2, float omb2,
                                                         float eps, float wd, const float* __restrict__ skip, const float* __restrict__ clip) {
    if (skip != nullptr && *skip != 0.f) return;          // sp_adam_multi_guarded: non-finite gradients were found - no update at all
    float coef = 1.f;
    if constexpr (CLIP) {
        if (clip[2] != 0.f) return;                       // the sum of squares was not finite: no update at all
        coef = clip[1];
    }
    const sp_adam_chunk c = chunks[blockIdx.x];
    const bool vec = (((uintptr_t)c.p | (uintptr_t)c.g | (uintptr_t)c.m | (uintptr_t)c.v) & 15) == 0;
    const int n4 = vec ? c.n >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 p = reinterpret_cast<float4*>(c.p)[i];
        const float4 g4 = reinterpret_cast<const float4*>(c.g)[i];
        float4 m = reinterpret_cast<float4*>(c.m)[i], v = reinterpret_cast<float4*>(c.v)[i];
        float pp[4] = {p.x, p.y, p.z, p.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w}, mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gc = CLIP ? mul_rounded_once(gg[r], coef) : gg[r];
            const float g = wd != 0.f ? gc + wd * pp[r] : gc;
            mm[r] = mm[r] + (g - mm[r]) * omb1;
            vv[r] = vv[r] * beta2 + omb2 * g * g;
            const float denom = sqrtf(vv[r]) * c.inv_sqrt_bc2 + eps;
            pp[r] = pp[r] - c.step_size * (mm[r] / denom);
        }
        reinterpret_cast<float4*>(c.p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        reinterpret_cast<float4*>(c.m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
        reinterpret_cast<float4*>(c.v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
        const float gc = CLIP ? mul_rounded_once(c.g[i], coef) : c.g[i];
        const float g = wd != 0.f ? gc + wd * c.p[i] : gc;
        const float m = c.m[i] + (g - c.m[i]) * omb1;
        const float v = c.v[i] * beta2 + omb2 * g * g;
        const float denom = sqrtf(v) * c.inv_sqrt_bc2 + eps;
        c.p[i] = c.p[i] - c.step_size * (m / denom);
        c.m[i] = m;
        c.v[i] = v;
    }
}

// The four wave sums of a 256-thread block, added by thread 0 in the order ((w0 + w1) + w2) + w3; the result is valid in thread 0 only.
__device__ __forceinline__ double block_sum_256_f64(double v, double* scratch /* 4 doubles, LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // lane l holds the same tree's sum in every lane
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

__device__ __forceinline__ double add_squares(double acc, const float4 v) {
    const double x = v.x, y = v.y, z = v.z, w = v.w;
    acc += x * x;
    acc += y * y;
    acc += z * z;
    acc += w * w;
    return acc;
}

// sp_grad_sqnorm_multi: partials[chunk] = sum g[i]^2 in fp64, one block per chunk in adam_multi_kernel's form (float4 where g is 16-byte
// aligned).  A product of two fp32 values is exact in fp64 (48 bits), so only the additions round.  Fixed order: thread t adds its
// elements in index order (float4 i = t, t + 256, ..., each x, y, z, w; then the tail), the 64 lanes of a wave meet in an xor-shuffle
// tree (offsets 32 ... 1), the four waves through LDS.  No atomics; only the g and n columns of the table are read.
__global__ __launch_bounds__(256) void grad_sqnorm_multi_kernel(const sp_adam_chunk* __restrict__ chunks, double* __restrict__ partials) {
    __shared__ double scratch[4];
    const float* __restrict__ g = chunks[blockIdx.x].g;
    const int n = chunks[blockIdx.x].n;
    const int n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? n >> 2 : 0;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    double acc = 0.0;
    int i = threadIdx.x;
    // eight loads in flight per thread (the one stream of this pass would otherwise wait for every float4 in turn); the order of the
    // additions is the plain loop's
    for (; i + 7 * 256 < n4; i += 8 * 256) {
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = g4[i + k * 256];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = add_squares(acc, v[k]);
    }
    for (; i < n4; i += 256) acc = add_squares(acc, g4[i]);
    for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) {
        const double x = g[i];
        acc += x * x;
    }
    const double total = block_sum_256_f64(acc, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// sp_grad_clip_finalize: one block.  sum = the partials in fp64 in a fixed order - thread t adds partials[t], partials[t + 256], ...,
// then block_sum_256_f64's tree - and thread 0 writes the five floats of the state.
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ partials, int n, double max_norm,
                                                                 float* __restrict__ st) {
    __shared__ double scratch[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
    const double sum = block_sum_256_f64(acc, scratch);
    if (threadIdx.x != 0) return;
    const bool bad = !((sum - sum) == 0.0);                            // +-inf or NaN (a sum of squares is never negative)
    const double norm = __dsqrt_rn(sum);
    float coef = 0.f;
    if (!bad) coef = (float)fmin(1.0, __ddiv_rn(max_norm, norm + 1e-6));   // torch.nn.utils.clip_grad_norm_'s formula, rounded to fp32 once
    st[0] = (float)norm;
    st[1] = coef;
    st[2] = bad ? 1.f : 0.f;
    if (bad) st[3] += 1.f;
    else if (coef < 1.f) st[4] += 1.f;
}

// Exponential moving average of a network's parameters (sp_ema_multi) and the in-place exchange that evaluates it (sp_swap_multi):
// one block per chunk, the form of adam_multi_kernel.  avg += (p - avg) * (1 - decay) is Tensor.lerp_'s order, as for Adam's m.
__global__ __launch_bounds__(256) void ema_multi_kernel(const sp_ema_chunk* __restrict__ chunks, float omd, const float* __restrict__ skip) {
    if (skip != nullptr && *skip != 0.f) return;          // the optimizer step was skipped (non-finite gradients): the average stays too
    const sp_ema_chunk c = chunks[blockIdx.x];
    const bool vec = (((uintptr_t)c.avg | (uintptr_t)c.p) & 15) == 0;
    const int n4 = vec ? c.n >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 a = reinterpret_cast<float4*>(c.avg)[i];
        const float4 p = reinterpret_cast<const float4*>(c.p)[i];
        a.x = a.x + (p.x - a.x) * omd; a.y = a.y + (p.y - a.y) * omd; a.z = a.z + (p.z - a.z) * omd; a.w = a.w + (p.w - a.w) * omd;
        reinterpret_cast<float4*>(c.avg)[i] = a;
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) c.avg[i] = c.avg[i] + (c.p[i] - c.avg[i]) * omd;
}

__global__ __launch_bounds__(256) void swap_multi_kernel(const sp_ema_chunk* __restrict__ chunks) {
    const sp_ema_chunk c = chunks[blockIdx.x];
    const bool vec = (((uintptr_t)c.avg | (uintptr_t)c.p) & 15) == 0;
    const int n4 = vec ? c.n >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 a = reinterpret_cast<float4*>(c.avg)[i];
        const float4 p = reinterpret_cast<float4*>(c.p)[i];
        reinterpret_cast<float4*>(c.avg)[i] = p;
        reinterpret_cast<float4*>(c.p)[i] = a;
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
        const float a = c.avg[i], p = c.p[i];
        c.avg[i] = p;
        c.p[i] = a;
    }
}

__global__ __launch_bounds__(256) void scale_f32_kernel(float* __restrict__ x, long n4, long n, float f, const float* __restrict__ fdev) {
    if (fdev != nullptr) f = *fdev;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        v.x *= f; v.y *= f; v.z *= f; v.w *= f;
        reinterpret_cast<float4*>(x)[i] = v;
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] *= f;
}

// any non-finite value in x -> *found = 1 (every thread that sees one stores the same value: no atomics, no reset here)
__global__ __launch_bounds__(256) void check_finite_kernel(const float* __restrict__ x, long n4, long n, float* __restrict__ found) {
    const long stride = (long)gridDim.x * 256;
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        // x - x is 0 for every finite x and NaN for +-inf / NaN
        const float t = (v.x - v.x) + (v.y - v.y) + (v.z - v.z) + (v.w - v.w);
        bad |= !(t == 0.f);
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) bad |= !((x[i] - x[i]) == 0.f);
    if (bad) *found = 1.f;
}

// state: [0] scale, [1] 1 / scale, [2] clean optimizer steps since the scale last changed, [3] non-finite gradients found (consumed here),
// [4] optimizer steps skipped so far - torch.cuda.amp.GradScaler's policy, entirely on the device
__global__ void loss_scale_update_kernel(float* __restrict__ st, float growth, float backoff, float interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float scale = st[0], clean = st[2];
    if (st[3] != 0.f) {
        scale = fmaxf(scale * backoff, 1.f);
        clean = 0.f;
        st[4] += 1.f;
    } else {
        clean += 1.f;
        if (clean >= interval) { scale = fminf(scale * growth, 16777216.f); clean = 0.f; }
    }
    st[0] = scale; st[1] = 1.f / scale; st[2] = clean; st[3] = 0.f;
}

}  // namespace

extern "C" int sp_check_finite(const float* x, int64_t numel, float* found, sp_stream_t stream) {
    SP_CHECK_ARG(x && found && numel > 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0, "sp_check_finite: bad args (16-byte aligned pointer, numel > 0)");
    long blocks = (numel / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(check_finite_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, (long)(numel / 4), (long)numel, found);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_loss_scale_update(float* state, float growth, float backoff, int32_t interval, sp_stream_t stream) {
    SP_CHECK_ARG(state && growth >= 1.f && backoff > 0.f && backoff <= 1.f && interval > 0, "sp_loss_scale_update: bad args");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), state, growth, backoff, (float)interval);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scale_f32_dev(float* x, int64_t numel, const float* factor_dev, sp_stream_t stream) {
    SP_CHECK_ARG(x && factor_dev && numel > 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0, "sp_scale_f32_dev: bad args (16-byte aligned pointer, numel > 0)");
    long blocks = (numel / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(scale_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, (long)(numel / 4),
                       (long)numel, 1.f, factor_dev);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scale_f32(float* x, int64_t numel, float factor, sp_stream_t stream) {
    SP_CHECK_ARG(x && numel > 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0, "sp_scale_f32: bad args (16-byte aligned pointer, numel > 0)");
    long blocks = (numel / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(scale_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, (long)(numel / 4),
                       (long)numel, factor, (const float*)nullptr);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

static int adam_multi_launch(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps, double weight_decay,
                             const float* skip_if_nonzero, const float* clip_state, sp_stream_t stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto kernel = clip_state != nullptr ? adam_multi_kernel<true> : adam_multi_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(256), 0, s, chunks_dev, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                       (float)eps, (float)weight_decay, skip_if_nonzero, clip_state);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_adam_multi_guarded(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                                     double weight_decay, const float* skip_if_nonzero, sp_stream_t stream) {
    SP_CHECK_ARG(chunks_dev && n_chunks > 0, "sp_adam_multi: bad args");
    return adam_multi_launch(chunks_dev, n_chunks, beta1, beta2, eps, weight_decay, skip_if_nonzero, nullptr, stream);
}

extern "C" int sp_adam_multi_clipped(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                                     double weight_decay, const float* skip_if_nonzero, const float* clip_state, sp_stream_t stream) {
    SP_CHECK_ARG(chunks_dev && n_chunks > 0 && clip_state, "sp_adam_multi_clipped: bad args (chunk table, n_chunks > 0, clip_state)");
    return adam_multi_launch(chunks_dev, n_chunks, beta1, beta2, eps, weight_decay, skip_if_nonzero, clip_state, stream);
}

extern "C" int sp_grad_sqnorm_multi(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double* partials, sp_stream_t stream) {
    SP_CHECK_ARG(chunks_dev && n_chunks > 0 && partials && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
                 "sp_grad_sqnorm_multi: bad args (chunk table, n_chunks > 0, 8-byte aligned partials)");
    hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3(n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), chunks_dev, partials);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_grad_clip_finalize(const double* partials, int32_t n_partials, double max_norm, float* state, sp_stream_t stream) {
    SP_CHECK_ARG(partials && n_partials > 0 && state && max_norm > 0.0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
                 "sp_grad_clip_finalize: bad args (partials, n_partials > 0, max_norm > 0 (inf allowed, NaN not), state)");
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partials, (int)n_partials,
                       max_norm, state);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_adam_multi(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                             double weight_decay, sp_stream_t stream) {
    return sp_adam_multi_guarded(chunks_dev, n_chunks, beta1, beta2, eps, weight_decay, nullptr, stream);
}

extern "C" int sp_ema_multi(const sp_ema_chunk* chunks_dev, int32_t n_chunks, float one_minus_decay, const float* skip_if_nonzero,
                            sp_stream_t stream) {
    SP_CHECK_ARG(chunks_dev && n_chunks > 0 && one_minus_decay >= 0.f && one_minus_decay <= 1.f,
                 "sp_ema_multi: bad args (chunk table, n_chunks > 0, 0 <= one_minus_decay <= 1)");
    hipLaunchKernelGGL(ema_multi_kernel, dim3(n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), chunks_dev, one_minus_decay,
                       skip_if_nonzero);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_swap_multi(const sp_ema_chunk* chunks_dev, int32_t n_chunks, sp_stream_t stream) {
    SP_CHECK_ARG(chunks_dev && n_chunks > 0, "sp_swap_multi: bad args (chunk table, n_chunks > 0)");
    hipLaunchKernelGGL(swap_multi_kernel, dim3(n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), chunks_dev);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
