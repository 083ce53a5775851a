/* sempyr.h - C ABI of libsempyr.so, the MI355X (gfx950) kernel library under the Semantic-Pyramid
 * GAN training step.
 *
 * The reference (/root/reference) is pure PyTorch and has NO FFI layer of its own; its arithmetic is
 * the stock torch ops called from models.py / lossfunction.py.  This header is therefore the boundary
 * a maintainer binds underneath those modules: every entry point names the reference call site(s)
 * whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - Plain C: pointers + sizes only, no torch types.  All pointers are DEVICE pointers borrowed for
 *     the call (caller-allocated, e.g. torch tensors via data_ptr()); nothing is allocated or freed,
 *     no call synchronises.  `stream` is a hipStream_t passed as void*.
 *   - Return 0 on success, negative sp_status otherwise; sp_last_error_string() gives the reason
 *     (thread-local).  Nothing throws.
 *   - Activations are NHWC ("channels-last"): element (n,h,w,c) at ((n*H+h)*W+w)*ld + c, where ld is
 *     the channel pitch in elements.  `dtype` selects the HBM storage type of activations and packed
 *     weights (SP_F32 / SP_BF16 / SP_F16); accumulation is always fp32.  Master weights, biases, statistics,
 *     gradients of parameters and loss scalars are always fp32.
 *   - Packed conv weights: [Cout][kh*kw][cin_p] (K-contiguous per output channel), cin_p = Cin rounded
 *     up to a 16-byte multiple.  The same kernel computes the input gradient from the "dgrad" packing
 *     [Cin][flipped taps][cout_p].
 */
#ifndef SEMPYR_H
#define SEMPYR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_VERSION 1

typedef void* sp_stream_t;

enum sp_status { SP_OK = 0, SP_ERR_INVALID = -1, SP_ERR_LAUNCH = -2, SP_ERR_UNSUPPORTED = -3 };
enum sp_dtype { SP_F32 = 0, SP_BF16 = 1, SP_F8 = 2 /* OCP e4m3 operands, see sp_conv_params: x_scale .. y8_amax; 16-bit outputs bf16 */,
                SP_F16 = 3 /* IEEE half-precision storage, v_mfma_f32_16x16x32_f16, fp32 accumulate: accepted wherever SP_BF16 is (same
                            * layouts, same kernels compiled for the other 16-bit type) - BASELINE.json config 5's "fp16 activations" */,
                SP_F8_F16 = 4 /* sp_conv2d_igemm only: SP_F8 operands with fp16 (not bf16) 16-bit outputs */ };
enum sp_act { SP_ACT_NONE = 0, SP_ACT_LRELU = 1, SP_ACT_RELU = 2, SP_ACT_TANH = 3 };

int sp_version(void);

/* Knobs for tests and A/B measurements.  The library reads NO environment variables: every switch goes through this call
 * (the Python binding forwards SP_* environment variables of the same names at load time, _lib.py).  value < 0 restores the
 * built-in default.  Except SP_TUNE_DETERMINISTIC none of them changes results beyond fp summation order.
 *   SP_TUNE_CONV_TALL        0 = never use conv3x3_tall_kernel, 1 = where its tiles fill the chip (default), 2 / 3 = force the 16- / 8-row form
 *   SP_TUNE_IGEMM_DMA        0 = never use the LDS-DMA igemm kernel, 1 = small-spatial 3x3 layers (default), 2 = everywhere
 *   SP_TUNE_WGRAD_ROWS       0 = never use the row-walker 3x3 weight-gradient kernel, 1 = maps >= 32 wide and 16 x 16 maps (default),
 *                            2 = maps >= 32 wide only, 3 = 8 x 8 maps too
 *   SP_TUNE_DETERMINISTIC    1 = the reductions behind gradients, parameters and normalisation statistics run in a fixed
 *                            order (per-split partial slabs + ordered reduce instead of fp32 atomics): those tensors are
 *                            bit-identical run to run (tests/test_gpu_step.py).  NOT covered: the scalar loss VALUES (fp64
 *                            atomics over blocks: equal to ~1e-16 relative, not bit for bit) and the <dW, W> dot of
 *                            sp_conv2d_wgrad_fused; a row-walker launch whose workspace is too small for its slabs does not
 *                            happen in this mode (the ordered per-tap kernels take the layer; sp_conv2d_wgrad_accum_pooled,
 *                            which has no other kernel, reports an error) - no silent fall-back to atomics.  0 = atomics where they are
 *                            faster; default (-1): on for SP_F32 storage (the parity mode), off for SP_BF16
 *   SP_TUNE_SPLITK_TARGET / _MINSTEPS     split-K plan of the small-spatial 3x3 forward / input-gradient layers (384 / 6)
 *   SP_TUNE_CONV1X1_DIRECT   0 = 1x1 layers on the tiled igemm kernel (default 1: direct kernel)
 *   SP_TUNE_CONV_SHORT       0 = Cout > 64 layers on the register-staged halo kernel (default 1: 8-row tall kernel)
 *   SP_TUNE_WGRAD9_BLOCKS, _WGRAD_BLOCKS, _WGRAD_MINSTEPS, _WGRAD_SMALL_M, _WGRAD_K1_TILE64   per-tap weight-gradient plan
 *   SP_TUNE_WGRAD_ROWS_THIN, _WGRAD_ROWS_BLOCKS, _WGRAD_ROWS_SLABS                            row-walker plan
 *   SP_TUNE_CONV_STAGGER     0 = both halves of a tall-kernel block issue their LDS-DMA at the head of a stage; 1 = the second half
 *                            issues a third of the way into its MFMA stream (default: 1 for the 16-row 128-co tile, 0 otherwise)
 *   SP_TUNE_CONV1X1_SPLITK   a bf16 1x1 layer (128 <= Cin <= 768) splits K over the four waves of a block while it has at most
 *                            this many (32-pixel x 64-channel) blocks (default 320: the 2x2 .. 8x8 maps at batch 20; 0 = never)
 *   SP_TUNE_WGRAD1X1         block target of the streaming weight-gradient kernel of the bf16 1x1 layers (default 256; 0 = those
 *                            layers stay on the per-tap kernel)
 *   SP_TUNE_CONV_CIN8        0 = the 3x3 layers with an 8-channel input (the padded RGB images) stay on the generic kernels (default 1)
 *   SP_TUNE_CONV_THINCO      0 = the 3x3 layers with at most 4 output channels (input gradients towards the images) stay on the
 *                            generic kernels (default 1)
 *   SP_TUNE_CONV_PP          bf16 3x3 layers with Cout > 64: 0 = conv3x3_tall_kernel (round 2's lockstep schedule), 1 = the ping-pong
 *                            schedule of conv_pp.hip, tile height by round count (default), 8 / 16 = force that tile height
 *   SP_TUNE_WGRAD_PP         0 = the 3x3 weight gradient of wide maps stays on the 4-wave row walker (default 1: its ping-pong form),
 *                            2 = like 1 (it used to select the alternating-row ping-pong kernel, which is gone), 3 = the cycle-stamp build of the
 *                            ping-pong form (writes per-wave segment cycles into the scratch instead of a gradient)
 *   SP_TUNE_IGEMM_TILE       output tile of the LDS-DMA igemm on small-spatial 3x3 layers with Cout > 64: 0 = 64 co x 64 px, 1 = 128 x 128,
 *                            2 = 128 co x 64 px, 3 = 64 co x 128 px; default: 0, or 2 where 64 x 64 tiles make 1 - 2 rounds of the chip and K is long
 *   SP_TUNE_CONV_PPW         16-bit 3x3 layers with Cout > 64 on 16 x 32-pixel patches: the ping-pong kernel with 64 co x 4 rows per wave
 *                            (conv_ppw.hip) where the round count favours 16-row items; 0 = off (tall<2,16> / the 8-row form), 2 = wherever eligible,
 *                            3 = like 1 (it used to price the 16-row form with its K-split: step-neutral, round6_ab_ppw_pricing_step.txt)
 *   SP_TUNE_LINEAR_KS        K range per block of the split-K MFMA linear kernel: 1024 / 512 / 256 / 128 (default: the widest that yields 256 blocks)
 *   SP_TUNE_BN_ITERS         pixels per thread of the elementwise BatchNorm passes (grid sizing; default 2)
 *   SP_TUNE_CONV_PP_SPLIT    0 = the ping-pong 3x3 kernels never split the work items of their last, partial round along K (default 1: they
 *                            do where sp_conv_params.workspace holds the partial tiles - sp_conv2d_workspace() says how many bytes - and
 *                            sp_conv_params.split_sync the counters; 2 = only launches of at least one full round of the 256 blocks; 3 (tests) = like
 *                            1, and the closing piece of an item stores and counts like every other piece - the hand-over's re-read
 *                            path, which otherwise runs only when a block is delayed, on every split launch)
 *   SP_TUNE_CONV_PP_PRIO     bit 0: s_setprio 1 around every MFMA segment of the ping-pong kernel (default 1); bit 1: static priority 1
 *                            for the second-dispatched half of the block
 *   SP_TUNE_PAIRSET_SEGMENTS the pair-set kernels (sp_pairset_knn / _cover) cut the column blocks of a row block into this many segments
 *                            (default: what gives 6144 blocks; always clamped to [1, column blocks]); sp_pairset_workspace follows it
 *   SP_TUNE_ATTN_PIECES      the 16-bit MFMA attention kernels give an image this many blocks, each walking ceil(nqb / pieces) of its
 *                            nqb = ceil(n / 64) query blocks (default: one query block each where batch x nqb blocks find a slot on
 *                            the chip, otherwise the shortest walk that brings them down to one round; clamped to [1, nqb]);
 *                            sp_attention_plan says what a launch gets.  4096 (diagnostics, tools/time_attention.py --phases):
 *                            sp_attention_bwd launches the TIMING build of its one-slab-per-query-block kernel and no reduce -
 *                            the slabs then hold cycle counts per phase and dk / dv are not written */
enum { SP_TUNE_CONV_TALL = 0, SP_TUNE_IGEMM_DMA = 1, SP_TUNE_WGRAD_ROWS = 2, SP_TUNE_DETERMINISTIC = 3,
       SP_TUNE_SPLITK_TARGET = 4, SP_TUNE_SPLITK_MINSTEPS = 5, SP_TUNE_CONV1X1_DIRECT = 6, SP_TUNE_CONV_SHORT = 7,
       SP_TUNE_WGRAD9_BLOCKS = 8, SP_TUNE_WGRAD_BLOCKS = 9, SP_TUNE_WGRAD_MINSTEPS = 10, SP_TUNE_WGRAD_SMALL_M = 11,
       SP_TUNE_WGRAD_K1_TILE64 = 12, SP_TUNE_WGRAD_ROWS_THIN = 13, SP_TUNE_WGRAD_ROWS_BLOCKS = 14, SP_TUNE_WGRAD_ROWS_SLABS = 15,
       SP_TUNE_CONV_STAGGER = 16, SP_TUNE_CONV1X1_SPLITK = 17, SP_TUNE_WGRAD1X1 = 18, SP_TUNE_CONV_CIN8 = 19, SP_TUNE_CONV_THINCO = 20, SP_TUNE_CONV_PP = 21, SP_TUNE_CONV_PP_PRIO = 22, SP_TUNE_WGRAD_PP = 23, SP_TUNE_BN_ITERS = 24, SP_TUNE_IGEMM_TILE = 25, SP_TUNE_CONV_PPW = 26, SP_TUNE_LINEAR_KS = 27, SP_TUNE_CONV_PP_SPLIT = 28, SP_TUNE_PAIRSET_SEGMENTS = 29, SP_TUNE_ATTN_PIECES = 30, SP_TUNE_COUNT = 31 };
int sp_set_tuning(int32_t key, int32_t value);
const char* sp_last_error_string(void);
/* Name of the kernel (route) the last sp_conv2d_igemm / sp_conv2d_wgrad* call of THIS thread launched ("" before the first one):
 * lets a profiler-less caller attribute its event timings to kernels (bench.py's per-route table).  Static strings. */
const char* sp_last_route(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution as NHWC implicit GEMM on MFMA (3x3 stride 1 pad 1, or 1x1).
 * Replaces nn.Conv2d forward at models.py:34,55,58,232-243,299,303,309,312,394,398,403,439,443,448
 * and the torchvision VGG-16 `features` convs (models.py:176,201-202); with the dgrad packing it is
 * also the input-gradient pass autograd runs for them at model_wrapper.py:160,188.
 *   y = act( (conv(x, w) + bias) * slope(mask_src) + res1 + res2 )
 *   slope(m) = m > 0 ? 1 : mask_neg_slope   (only when mask_src != NULL; used to fold the derivative
 *   of a LeakyReLU/ReLU that precedes the convolution into its input-gradient pass)
 * ---------------------------------------------------------------------------------------------- */
typedef struct sp_conv_params {
    const void* x;          /* [n][h][w][cin_p]                      dtype */
    const void* w;          /* [cout][ksize*ksize][cin_p]            dtype */
    const float* bias;      /* [cout] or NULL                                */
    void* y;                /* [n][h][w][ldy] (cout valid channels)   dtype */
    const void* res1;       /* like y, or NULL                               */
    const void* res2;       /* like y, or NULL                               */
    const void* mask_src;   /* like y, or NULL                               */
    float mask_neg_slope;
    int32_t n, h, w_, cin_p, cout, ldy, ksize, act, dtype;
    void* workspace;        /* optional fp32 scratch of sp_conv2d_workspace() bytes: lets small-spatial layers split K, and the 16-bit 3x3
                             * ping-pong kernel split the items of its last partial round (conv_pp.hip, "tail split"); NULL = never */
    int64_t workspace_bytes;
    int32_t pool2;          /* 2: y is [n][h/2][w/2][ldy] and y = act(maxpool2x2(conv) + bias) - conv -> ReLU -> nn.MaxPool2d(2) of
                             * the frozen VGG-16 stages (models.py:158-216) when the unpooled tensor is not needed (no-grad
                             * pass); no residuals, act NONE / ReLU / LeakyReLU.
                             * 1: y, res1, res2 are [n][h/2][w/2][ldy] and y = act(avgpool2x2(conv) + bias + res1 + res2): the
                             * nn.AvgPool2d(2) that follows the second convolution of a discriminator block (models.py:407-417,
                             * 452-462) rides in the epilogue.  3x3, cout > 32 and a multiple of 16, h % 8 == 0, w % 32 == 0,
                             * ldy % 8 == 0, no mask_src; anything else is rejected (SP_ERR_INVALID) */
    int32_t in_up2;         /* 1: x is [n][h/2][w/2][cin_p] and the convolution runs over 1/4 x its nearest-neighbour x2 expansion,
                             * i.e. over the gradient of a 2x2 average pooling that is never written out (input-gradient pass of
                             * a pool2 layer).  3x3, cout > 32, h % 8 == 0, w % 32 == 0 (SP_ERR_INVALID otherwise) */
    /* dtype == SP_F8 (BASELINE.json config 5: fp8 MFMA implicit-GEMM path; the frozen VGG-16 pyramid's 3x3 layers with
     * cout > 64, w % 32 == 0, h % 8 == 0, models.py:183-216): x and w hold OCP e4m3 bytes (cin_p a multiple of 16), the MFMA
     * is v_mfma_f32_16x16x32_fp8_fp8, accumulation fp32:
     *   v = act( conv(x, w) * x_scale[0] * w_scale[co] + bias[co] ), optionally 2x2 max-pooled (pool2 = 2),
     * stored as bf16 into y (may be NULL) and / or re-quantised, q = sat(v * y8_inv_scale[0]), as e4m3 into y8 (may be NULL;
     * same [n][h][w][ldy] geometry) for the next layer of the chain; max|v| is merged into y8_amax[0] (atomic max on the fp32
     * bit pattern, v >= 0 after ReLU) for the delayed scaling of the next call.  act NONE / ReLU, no residuals, no mask_src,
     * no in_up2, pool2 0 / 2, cout % 16 == 0.  All scale pointers are DEVICE pointers (no host round trip). */
    const float* x_scale;   /* [1]    dequantisation scale of x                      (SP_F8 only) */
    const float* w_scale;   /* [cout] dequantisation scale per output channel        (SP_F8 only) */
    void* y8;               /* e4m3 output or NULL                                   (SP_F8 only) */
    const float* y8_inv_scale; /* [1] quantisation scale of y8 (1 / its dequantisation scale), required with y8 */
    float* y8_amax;         /* [1] running max of v, or NULL                         (SP_F8 only) */
    /* Two-group batch (SP_F32 / SP_BF16): img_scale != NULL multiplies the fp32 accumulator of image n by img_scale[n >= img_split]
     * BEFORE bias / mask / residuals / activation:  y = act((conv(x, w) * img_scale[g(n)] + bias) * slope(mask_src) + res1 + res2).
     * It lets the discriminator's D(real) and D(fake) passes of one step (model_wrapper.py:153-155) - same weight_orig, but a
     * different spectral-norm sigma each, since every forward advances the power iteration (models.py:128-135) - run as ONE launch
     * over 2B images with the packing W / sigma_real and img_scale = {1, sigma_real / sigma_fake}; the same launch form computes the
     * input gradient (dgrad packing).  DEVICE pointer to 2 floats, both > 0.  NULL: no scaling (img_split ignored). */
    const float* img_scale;
    int32_t img_split;      /* images [0, img_split) use img_scale[0], the rest img_scale[1] */
    int32_t reserved_;
    int64_t split_pix_;     /* set by the library (first OUTPUT pixel index of the second group); callers leave it 0 */
    /* Fused 1x1 tail (16-bit storage, 3x3, cout == 64, h % 16 == 0, w % 32 == 0, ldy % 8 == 0, no pooling; SP_ERR_UNSUPPORTED elsewhere):
     *   tail_y[n,h,w,o] = tail_act( sum_c tail_w[o][c] * y[n,h,w,c] + tail_bias[o] ),  o < tail_cout <= 4
     * computed in the epilogue from the (16-bit rounded) y of this launch - the generator's last two layers, conv3x3 -> LeakyReLU ->
     * conv1x1 -> tanh (models.py:55-61), in one launch.  y may then be NULL (a forward pass that never looks at the 64-channel tensor
     * again): the 168 MB tensor of the 256 x 256 layer is neither written nor read back.  tail_w: [tail_cout][64] in the storage type
     * (the forward packing of the 1x1 layer), tail_y pitch tail_ld elements. */
    const void* tail_w;
    const float* tail_bias;
    void* tail_y;
    int32_t tail_cout, tail_act, tail_ld, reserved2_;
    /* pool2 == 2 only (conv -> ReLU -> MaxPool2d(2), the VGG-16 stages of /root/reference/models.py:183-216 in the pass WITH gradient):
     * where to leave the window position of every pooled element, so that the unpooled tensor never reaches HBM and the pooling's
     * backward (sp_maxpool2_bwd_idx) needs neither it nor a recomputation.  One uint32 per (pooled pixel, group of 16 channels),
     * [n * (h/2) * (w/2)][cout / 16]: bits 2c .. 2c+1 = 2 * row + column of the FIRST maximum (scan order, as torch's max_pool2d
     * routes its gradient) of channel 16 g + c, taken over the values as the storage type holds them - exactly the element
     * sp_maxpool2_bwd would pick from the stored unpooled tensor.  NULL: not recorded. */
    uint32_t* pool_idx;
    /* Round 6: counters of the 3x3 ping-pong kernels' K-split of their last partial round of work items (conv_pp.hip / conv_ppw.hip).
     * NULL: the launch never splits.  Otherwise SP_CONV_SPLIT_SYNC_BYTES of device memory that is ZERO when first handed to the
     * library and is left zero by every launch that used it (the kernels clean up behind themselves): one such area per STREAM
     * makes concurrent launches on different streams safe - the library keeps no device-side state of its own.  Needs
     * `workspace` for the partial tiles (sp_conv2d_workspace). */
    int32_t* split_sync;
} sp_conv_params;
#define SP_CONV_SPLIT_SYNC_BYTES 8192
int sp_conv2d_igemm(const sp_conv_params* p, sp_stream_t stream);
/* Bytes of fp32 scratch sp_conv2d_igemm wants in sp_conv_params.workspace to split the K loop of this shape over several
 * blocks (3x3 layers of small spatial extent: too few output tiles to fill 256 CUs); 0 = it would not split.  The scratch
 * holds one partial [n*h*w][cout] slab per split; it needs no initialisation and carries nothing between calls. */
int sp_conv2d_workspace(int32_t n, int32_t h, int32_t w_, int32_t cin_p, int32_t cout, int32_t ksize, int32_t dtype,
                        int64_t* bytes_out);
/* *route = the name sp_last_route() would report after sp_conv2d_igemm(p), without launching anything (same argument checks, same
 * errors; host-only: callable without a GPU).  It looks at p->workspace / workspace_bytes / split_sync but never dereferences a pointer. */
int sp_conv2d_route(const sp_conv_params* p, const char** route);

/* Weight gradient of the same convolution (autograd of nn.Conv2d at model_wrapper.py:160,188):
 *   dw[co][tap][ci] (+)= sum_{n,h,w} dy[n,h,w,co] * x[n,h+dr,w+ds,ci]      fp32, layout [cout][taps][cin_p]
 * dw is zeroed by the call, then accumulated with split-K partial sums. */
int sp_conv2d_wgrad(const void* x, const void* dy, float* dw, int32_t n, int32_t h, int32_t w_,
                    int32_t cin_p, int32_t cout, int32_t ld_dy, int32_t ksize, int32_t dtype,
                    sp_stream_t stream);

/* Same, plus by-products that cost no extra pass over the activations: dbias[cout] = sum_{n,h,w} dy (the bias
 * gradient; NULL to skip) and dot[0] = <dw, w_packed> where w_packed is the forward packing (W/sigma) of this layer,
 * i.e. the inner product the spectral-norm backward needs (NULL/NULL to skip).  dw, dbias, dot are zeroed by the call. */
int sp_conv2d_wgrad_fused(const void* x, const void* dy, float* dw, float* dbias, const void* w_packed, float* dot,
                          float* workspace, int64_t workspace_floats, int32_t n, int32_t h, int32_t w_, int32_t cin_p,
                          int32_t cout, int32_t ld_dy, int32_t ksize, int32_t dtype, sp_stream_t stream);
/* sp_conv2d_wgrad_fused without its fill: ACCUMULATES into dw [cout][taps][cin_p] and, if given, dbias [cout]; the caller
 * has zero-filled them (one fill for a whole network's gradient arena).  workspace (may be NULL): fp32 scratch of
 * sp_conv2d_wgrad_workspace() floats for per-block partial tiles - with it the split-K blocks merge through plain stores
 * and one reduce pass instead of serialised fp32 atomics. */
int sp_conv2d_wgrad_accum(const void* x, const void* dy, float* dw, float* dbias, float* workspace, int64_t workspace_floats,
                          int32_t n, int32_t h, int32_t w_, int32_t cin_p, int32_t cout, int32_t ld_dy, int32_t ksize,
                          int32_t dtype, sp_stream_t stream);
/* sp_conv2d_wgrad_accum for a pool2 layer: dy is the gradient at the POOLED resolution [n][h/2][w/2][ld_dy] and stands for
 * 1/4 x its nearest-neighbour x2 expansion (n, h, w_ describe x).  Only what the row-walking kernel takes (bf16, 3x3, w % 32 == 0,
 * h % 2 == 0, operands below 1 GiB; in the deterministic mode its slabs lent and at most 512 tile pairs): SP_ERR_INVALID otherwise.
 * sp_conv2d_wgrad_route() with dy_pooled = 1 says beforehand which it is. */
int sp_conv2d_wgrad_accum_pooled(const void* x, const void* dy, float* dw, float* dbias, float* workspace, int64_t workspace_floats,
                                 int32_t n, int32_t h, int32_t w_, int32_t cin_p, int32_t cout, int32_t ld_dy, int32_t ksize,
                                 int32_t dtype, sp_stream_t stream);
int sp_conv2d_wgrad_workspace(int32_t n, int32_t h, int32_t w_, int32_t cin_p, int32_t cout, int32_t ksize,
                              int32_t dtype, int64_t* floats_out);
/* sp_conv2d_wgrad_accum for a two-group batch (sp_conv_params.img_scale; the discriminator's D(real) | D(fake) pass): images
 * [0, split) accumulate into (dw_a, dbias_a), images [split, n) into (dw_b, dbias_b) - the spectral-norm backward of each forward
 * needs ITS weight gradient.  dy_pooled != 0: dy is at the pooled resolution as in sp_conv2d_wgrad_accum_pooled.  Where the row-walking
 * kernel takes the layer and the group boundary falls between two of its blocks this is ONE launch over all n images plus one
 * reduce pass per group (half the partial-tile traffic of two launches); otherwise the two groups run one after the other.
 * workspace: sp_conv2d_wgrad_workspace() floats for n images. */
int sp_conv2d_wgrad_accum_pair(const void* x, const void* dy, float* dw_a, float* dbias_a, float* dw_b, float* dbias_b, float* workspace,
                               int64_t workspace_floats, int32_t n, int32_t split, int32_t h, int32_t w_, int32_t cin_p, int32_t cout,
                               int32_t ld_dy, int32_t ksize, int32_t dy_pooled, int32_t dtype, sp_stream_t stream);
/* *route = the name sp_last_route() would report after the accumulating call with these arguments - split = 0 and dy_pooled = 0:
 * sp_conv2d_wgrad_accum, dy_pooled != 0: sp_conv2d_wgrad_accum_pooled, split > 0: sp_conv2d_wgrad_accum_pair (where its two groups run one
 * after the other: the second group's route) - without launching anything: same argument checks, same plan, same errors (an uncovered
 * pooled shape: SP_ERR_INVALID).  Host-only: callable without a GPU.  want_dbias: the call is given a bias gradient to fill;
 * workspace_floats: the scratch it is lent (0 = none). */
int sp_conv2d_wgrad_route(int32_t n, int32_t split, int32_t h, int32_t w_, int32_t cin_p, int32_t cout, int32_t ld_dy, int32_t ksize,
                          int32_t dy_pooled, int32_t want_dbias, int64_t workspace_floats, int32_t dtype, const char** route);
/* Deferred slab reductions.  The streaming weight-gradient kernels of the 1x1 and 8-channel 3x3 layers split the pixels over blocks,
 * leave one partial tile per split in the workspace and a second, tiny launch adds the partial tiles to dW in a fixed order.  Nothing
 * reads dW before the end of a backward pass (model_wrapper.py:160,188: the optimizer step), so a caller may collect those launches:
 *   sp_wgrad_reduce_defer(1)        from now on sp_conv2d_wgrad_accum* QUEUE that reduction instead of launching it (a layer whose dW
 *                                    is already queued keeps its own launch);
 *   sp_wgrad_reduce_flush(1, s)     ONE launch per 48 queued reductions on stream s (descriptors by value: capturable), the same
 *                                    arithmetic in the same order - bit-identical to the separate launches;
 *   sp_wgrad_reduce_flush(0, s)     drops the queue (a pass that was abandoned); sp_wgrad_reduce_pending() = its length;
 *   sp_wgrad_reduce_defer(0)        back to immediate reductions (what is queued stays queued until the flush).
 * The caller keeps every workspace alive until the flush and flushes on the stream the weight-gradient launches ran on.  The queue is
 * host state of the process (not thread-safe: one thread drives the passes of a device, as torch's autograd does). */
int sp_wgrad_reduce_defer(int32_t on);
int sp_wgrad_reduce_flush(int32_t run, sp_stream_t stream);
int sp_wgrad_reduce_pending(void);

/* ------------------------------------------------------------------------------------------------
 * Skinny linear layers: y = act(x W^T + bias + res), batch rows of any pitch, weights packed [n][kp]
 * (kp = K rounded up to 8, zero padded).  Replaces nn.Linear at models.py:28,128,132,356,359 and the
 * VGG-16 classifier (models.py:210-213); with the transposed packing [K][np] it is the dgrad pass.
 * ---------------------------------------------------------------------------------------------- */
int sp_linear_fwd(const void* x, int32_t ldx, const void* w_packed, int32_t kp, const float* bias,
                  const void* res, void* y, int32_t ldy, int32_t batch, int32_t k, int32_t n, int32_t act,
                  int32_t dtype, sp_stream_t stream);
/* Same contract with an fp32 scratch of sp_linear_workspace() floats supplied by the caller: large bf16 matrices
 * (batch <= 32) take the MFMA split-K path (weight panels streamed by hundreds of blocks; every K-split
 * stores its partial [batch][n] slab, a finalize pass sums them and applies bias / residual / activation).  The scratch
 * needs no initialisation.  scratch == NULL: sp_linear_fwd. */
int sp_linear_workspace(int32_t batch, int32_t k, int32_t n, int32_t dtype, int64_t* floats_out);
int sp_linear_fwd_ws(const void* x, int32_t ldx, const void* w_packed, int32_t kp, const float* bias,
                     const void* res, void* y, int32_t ldy, int32_t batch, int32_t k, int32_t n, int32_t act,
                     int32_t dtype, float* scratch, sp_stream_t stream);
/* dw[n][kp] = sum_b dy[b][n] x[b][k] (fp32), dbias[n] = sum_b dy[b][n] (may be NULL). */
int sp_linear_wgrad(const void* x, int32_t ldx, const void* dy, int32_t ld_dy, float* dw, int32_t kp,
                    float* dbias, int32_t batch, int32_t k, int32_t n, int32_t dtype, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Spectral normalisation of every layer of one network, batched (torch.nn.utils.spectral_norm, the
 * forward-pre-hook behind models.py:28,34,55,58,128,132,135,232-243,299-315,356-360,393-404,438-449):
 * one power iteration (in place on u, v) when power_iter != 0, sigma = u.(W v), then W/sigma is written
 * in the packings the conv / linear kernels read.  The table lives in DEVICE memory.
 *   scratch (fp32, per call, needs no initialisation): per layer at scratch_off: v-snapshot[cols], s[rows], u-snapshot[rows],
 *   {sigma, 1/sigma, -, -}; at part_off: ceil(rows/128) x cols floats (W^T u is formed as per-row-slab partial sums that are
 *   added in a fixed order: the forward pass is bit-reproducible)
 *   pack_arena (per call): per layer fwd packing at fwd_off, dgrad packing at dgrad_off (byte offsets, -1 = none)
 *   max_pack_elems: >= the element count of the largest packing and >= 1024 * ceil(cin_p/32) * ceil(cout_p/32) of every
 *   layer (the packing kernel moves 32 x 32 x taps tiles; this bounds its 2-D grid).  taps <= 9.
 *   pack_blocks > 0: the packing kernel runs on a 1-D grid of exactly that many blocks and layer i owns blocks
 *   [pack_block0[i], pack_block0[i+1]) - ceil(cin_p/32)*ceil(cout_p/32) of them (kind 1: ceil(rows*cols/1024)).  The 2-D grid
 *   (pack_blocks == 0) launches max-tiles x n_layers blocks, 90 % of which exit at once for a network with one big layer.
 *   pack_blocks == -1: nothing is packed (the power iteration and the snapshots only; the pack arena stays as it is) - a table
 *   whose block ranges are ALL empty cannot be expressed with pack_blocks > 0.
 *   Alignment (the table lives on the device, so only the two base pointers can be - and are - checked by the launcher; the
 *   rest is the caller's contract): w, u, v of every layer, scratch and pack_arena are 16-byte aligned; scratch_off and part_off
 *   are multiples of 4 floats (the forward reads and writes 16 bytes at a time wherever cols % 4 == 0; the batched backward
 *   tests the alignment and falls back to scalar accesses); fwd_off and dgrad_off are multiples of 8 bytes.  n_layers <= 256.
 *   taps <= 9 in every entry (the packing and the batched backward stage a 32- or 256-channel x taps tile in LDS sized for 9).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sp_sn_layer {
    const float* w;        /* weight_orig viewed [rows][cols] (OIHW flattened, cols = cin*taps)   */
    float* u;              /* weight_u [rows]  (updated in place)                                  */
    float* v;              /* weight_v [cols]  (updated in place)                                  */
    int64_t scratch_off;   /* in floats                                                             */
    int64_t part_off;      /* in floats: ceil(rows/128) x cols partial sums of W^T u (power iteration only; summed in order) */
    int64_t fwd_off;       /* bytes; layout [rows][taps][cin_p] dtype, or plain fp32 [rows][cols] if kind==1 */
    int64_t dgrad_off;     /* bytes; layout [cin][flipped taps][cout_p] dtype                       */
    int32_t rows, cols, cin, taps, cin_p, cout_p, kind, pack_block0;
} sp_sn_layer;
int sp_sn_forward(const sp_sn_layer* table_dev, int32_t n_layers, int32_t max_rows, int32_t max_cols,
                  int64_t max_pack_elems, float* scratch, int64_t scratch_floats, void* pack_arena,
                  int32_t power_iter, int32_t dtype, int32_t pack_blocks, sp_stream_t stream);
/* Two forwards of one network whose activations run as ONE two-group batch (sp_conv_params.img_scale; the discriminator's
 * D(real) / D(fake), model_wrapper.py:153-155): forward a packed W / sigma_a, forward b (one more power iteration) has sigma_b.
 * out[2 i] = 1, out[2 i + 1] = sigma_a / sigma_b for layer i - the per-group accumulator scales of a launch that uses a's
 * packing.  scratch_a / scratch_b: the scratch buffers of the two sp_sn_forward calls (same table). */
int sp_sn_pair_scales(const sp_sn_layer* table_dev, int32_t n_layers, const float* scratch_a, const float* scratch_b, float* out,
                      sp_stream_t stream);
/* The same backward for every layer of a network in one call (two launches).  Offsets are in floats: dw_off / dot_off
 * into `arena` (the caller zero-fills the arena once per backward pass; the weight-gradient kernels accumulate the
 * dW slots, this call the dots), scratch_off into the scratch of the matching sp_sn_forward call, grad_off into
 * `grads` (out, [rows][cols] per layer).  A layer whose dW slot was never written yields a zero gradient.
 * max_elems: largest rows*cols of the table.  accumulate_from (NULL, or a buffer laid out like `grads`, `grads` itself
 * included): the result is added to it - the gradients of a second forward through the same network (D(real) and D(fake),
 * model_wrapper.py:150-160) land on the first one's without one autograd addition per parameter.  bias_grads (NULL to
 * skip): the layers' bias-gradient slots of the arena are copied (accumulate_from == NULL) or added into it.
 * dot_partials: n_layers x 512 floats of scratch (no initialisation): per-block partial sums of <dW, W>, added in block order;
 * layer i uses its first min(512, ceil(max_elems / 1024), ceil(rows * cols / 1024)) entries, the others are not touched.
 * table_dev may point INTO a larger table (layers lo .. hi of it, n_layers = hi - lo): grad_off / bias_off keep addressing the
 * whole of `grads` / `bias_grads`, and nothing outside the ranges of the layers given is written.  taps <= 9. */
typedef struct sp_sn_bwd_layer {
    const float* w;        /* weight_orig [rows][cols] */
    int64_t dw_off, dot_off, scratch_off, grad_off;
    int32_t rows, cols, cin, taps, cin_p, plain;
    int32_t db_off, bias_off;  /* bias gradient: arena[db_off .. +rows) -> bias_grads[bias_off .. +rows) (floats) */
} sp_sn_bwd_layer;
int sp_sn_backward_batched(const sp_sn_bwd_layer* table_dev, int32_t n_layers, int64_t max_elems, float* arena,
                           const float* scratch, float* grads, const float* accumulate_from, float* bias_grads,
                           float* dot_partials, sp_stream_t stream);
/* The same with every gradient it writes (weights and biases) multiplied by grad_scale: the SP_F16 mode's static loss scale comes
 * off where the (fp32) parameter gradients are formed, without a pass of its own over the buffer. */
int sp_sn_backward_batched_scaled(const sp_sn_bwd_layer* table_dev, int32_t n_layers, int64_t max_elems, float* arena,
                                  const float* scratch, float* grads, const float* accumulate_from, float* bias_grads,
                                  float* dot_partials, float grad_scale, sp_stream_t stream);
/* ... and with the factor read from device memory (grad_scale_dev[0]) when the kernel runs: the SP_F16 mode's DYNAMIC loss scale
 * (sp_loss_scale_update) - a captured graph keeps working while the scale moves. */
int sp_sn_backward_batched_dscaled(const sp_sn_bwd_layer* table_dev, int32_t n_layers, int64_t max_elems, float* arena,
                                   const float* scratch, float* grads, const float* accumulate_from, float* bias_grads,
                                   float* dot_partials, const float* grad_scale_dev, sp_stream_t stream);

/* One-off packing of a frozen, non-normalised fp32 weight (the VGG-16 pyramid, models.py:176-181) into the
 * same two packings.  chw_c > 0: the input-feature index is permuted from NCHW-flatten (c*chw_hw + s) to
 * NHWC (s*chw_c + c) order (models.py:208 flattens NCHW; the kernels keep NHWC). */
int sp_pack_weight(const float* w, int32_t rows, int32_t cols, int32_t cin, int32_t taps, int32_t cin_p,
                   int32_t cout_p, int32_t chw_c, int32_t chw_hw, void* fwd, void* dgrad, int32_t dtype,
                   sp_stream_t stream);
/* Backward of one layer: grad[rows][cols] = (dwsn - <dwsn, W/sigma> u v^T) / sigma with the u, v, sigma
 * snapshots of the forward whose scratch slice is passed.  dwsn is fp32 in the forward packing
 * (plain != 0: [rows][cols]).  dot_tmp: one float; dot_ready = 1: it already holds <dwsn, w_orig>;
 * dot_ready = 2: it holds <dwsn, w_orig / sigma> (delivered by sp_conv2d_wgrad_fused); dot_ready = 3: it is
 * already zero-filled (sp_conv2d_wgrad_fused given `dot` without `w_packed`) and the dot product is formed here. */
int sp_sn_backward(const float* dwsn, const float* w_orig, const float* layer_scratch, int32_t rows, int32_t cols,
                   int32_t cin, int32_t taps, int32_t cin_p, int32_t plain, float* dot_tmp, int32_t dot_ready,
                   float* grad, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * (Conditional) BatchNorm, training mode (nn.BatchNorm2d at models.py:53,484; ConditionalBatchNorm.forward
 * models.py:491-506).  sp_bn_stats: batch mean / invstd (+ running-stat update with the unbiased variance;
 * training == 0 derives them from the running statistics instead).  sp_bn_apply:
 *   y = act(scale[n,c] * (x - mean[c]) * invstd[c] + bias[n,c]),  (scale,bias) = (gamma,beta) or, when emb != NULL,
 *   the two halves of emb[cls[n]] (row = [scale(C) | bias(C)]).  partials: 1024*2*C floats of scratch (per-block
 *   partial sums, added in fp64 by a second kernel: deterministic, no atomics).
 * ---------------------------------------------------------------------------------------------- */
int sp_bn_stats(const void* x, int32_t n, int64_t hw, int32_t c, float* partials, float eps, float momentum,
                float* running_mean, float* running_var, int32_t training, float* mean_out, float* invstd_out,
                int32_t dtype, sp_stream_t stream);
int sp_bn_apply(const void* x, void* y, int32_t n, int64_t hw, int32_t c, const float* mean, const float* invstd,
                const float* gamma, const float* beta, const float* emb, const int64_t* cls, int32_t act,
                int32_t dtype, sp_stream_t stream);
/* sp_bn_apply fused with the bilinear x2 upsampling (align_corners=True) that follows CBN -> LeakyReLU in a generator block
 * (models.py:296-298): y is [n][2h][2w][c]; every output pixel normalises + activates its four source pixels on the fly. */
/* The same for a batch of TWO groups - images [0, split) and [split, n) belong to two forwards of the network (round 5: the generator's
 * two forwards of an iteration in one pass, model_wrapper.py:144-151,165-172) - each group normalised by ITS OWN batch statistics, in
 * one launch set: mean2 / invstd2 are [2][c]; the running statistics take the two batches one after the other, group `first_group`
 * first (the forward the reference runs first).  Training mode.  cls: n class indices. */
int sp_bn_stats_pair(const void* x, int32_t n, int32_t split, int64_t hw, int32_t c, float* partials, float eps, float momentum,
                     float* running_mean, float* running_var, int32_t first_group, float* mean2, float* invstd2, int32_t dtype,
                     sp_stream_t stream);
int sp_bn_apply_pair(const void* x, void* y, int32_t n, int32_t split, int64_t hw, int32_t c, const float* mean2, const float* invstd2,
                     const float* gamma, const float* beta, const float* emb, const int64_t* cls, int32_t act, int32_t dtype,
                     sp_stream_t stream);
int sp_bn_apply_upsample2_pair(const void* x, void* y, int32_t n, int32_t split, int32_t h, int32_t w_, int32_t c, const float* mean2,
                               const float* invstd2, const float* gamma, const float* beta, const float* emb, const int64_t* cls,
                               int32_t act, int32_t dtype, sp_stream_t stream);   /* sp_bn_apply_upsample2 on a batch of two groups */
int sp_bn_apply_upsample2(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, const float* emb,
                          const int64_t* cls, int32_t act, int32_t dtype, sp_stream_t stream);
/* dy is the gradient w.r.t. the (activated) output; partials: 1024*2*c floats, c_tmp: 2*c floats of scratch.  Every sample owns
 * floor(1024 / n) >= 1 of the 1024 partial rows [c][2], so 1 <= n <= 1024 (SP_ERR_INVALID otherwise, before any launch).
 * Parameter gradients: dgamma/dbeta [c] (plain) or demb [num_classes][2c] (conditional; zeroed by the call). */
int sp_bn_backward(const void* dy, const void* x, void* dx, int32_t n, int64_t hw, int32_t c, const float* mean,
                   const float* invstd, const float* gamma, const float* beta, const float* emb, const int64_t* cls,
                   int32_t act, float* partials, float* c_tmp, float* dgamma, float* dbeta, float* demb,
                   int32_t num_classes, int32_t dtype, sp_stream_t stream);

/* BatchNorm (+ activation) of u = bilinear x2 (align_corners=True) of a stored tensor x [n][h][w][c], without materialising u: the
 * generator's final block, UpsamplingBilinear2d -> BatchNorm2d -> LeakyReLU (models.py:52-54).  Same statistics / running-stat /
 * gradient semantics as sp_bn_stats / sp_bn_apply / sp_bn_backward applied to u [n][2h][2w][c] (u takes the storage type's rounding,
 * as if it had been written); y and dy are [n][2h][2w][c]; sp_bn_backward_up2 writes du = d loss / d u [n][2h][2w][c] - the caller
 * folds it back with sp_upsample2_bwd.  partials: 1024*2*c floats, c_tmp: 2*c floats of scratch.  c / (16-byte group) <= 256. */
int sp_bn_stats_up2(const void* x, int32_t n, int32_t h, int32_t w_, int32_t c, float* partials, float eps, float momentum,
                    float* running_mean, float* running_var, float* mean_out, float* invstd_out, int32_t dtype, sp_stream_t stream);
int sp_bn_apply_up2(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, const float* emb, const int64_t* cls, int32_t act, int32_t dtype,
                    sp_stream_t stream);
int sp_bn_backward_up2(const void* dy, const void* x, void* du, int32_t n, int32_t h, int32_t w_, int32_t c, const float* mean,
                       const float* invstd, const float* gamma, const float* beta, const float* emb, const int64_t* cls,
                       int32_t act, float* partials, float* c_tmp, float* dgamma, float* dbeta, float* demb, int32_t num_classes,
                       int32_t dtype, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling / resampling (NHWC, c % 4 == 0).
 *   avg-pool 2x2 (models.py:406,451); optional second output y_act = act(y)
 *   max-pool 2x2/2 (models.py:245; VGG features models.py:203), relu != 0 fuses the preceding ReLU
 *   adaptive avg-pool (models.py:126 and the VGG 8->7 avgpool models.py:206), act_in fuses a preceding activation
 *   bilinear x2 align_corners=True (nn.UpsamplingBilinear2d, models.py:52,298,308)
 * ---------------------------------------------------------------------------------------------- */
int sp_avgpool2_fwd(const void* x, void* y, void* y_act, int32_t act, int32_t n, int32_t h, int32_t w_, int32_t c,
                    int32_t dtype, sp_stream_t stream);
int sp_avgpool2_bwd(const void* dy, void* dx, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype,
                    sp_stream_t stream);
/* y_act = act(x) and y_pool = avgpool2x2(x) in one pass over x (the two consumers of a discriminator block's input,
 * models.py:452-462: LeakyReLU -> conv and AvgPool -> 1x1 conv); backward: dx = act'(x) * d_act + expand(d_pool) / 4, either
 * gradient may be NULL.  act: NONE / LeakyReLU(0.2) / ReLU. */
int sp_act_avgpool2_fwd(const void* x, void* y_act, void* y_pool, int32_t act, int32_t n, int32_t h, int32_t w_, int32_t c,
                        int32_t dtype, sp_stream_t stream);
int sp_act_avgpool2_bwd(const void* d_act, const void* d_pool, const void* x, void* dx, int32_t act, int32_t n, int32_t h,
                        int32_t w_, int32_t c, int32_t dtype, sp_stream_t stream);
int sp_maxpool2_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t relu, int32_t dtype,
                    sp_stream_t stream);
int sp_maxpool2_bwd(const void* dy, const void* x, void* dx, int32_t n, int32_t h, int32_t w_, int32_t c,
                    int32_t relu, int32_t dtype, sp_stream_t stream);
/* Backward of conv -> ReLU -> MaxPool2d(2) from what the fused epilogue left behind (sp_conv_params.pool_idx): dx [n][h][w][c] gets
 * dy [n][h/2][w/2][c] at the recorded window position where the pooled value y is positive, zero elsewhere - bit for bit what
 * sp_maxpool2_bwd(relu = 1) computes from the unpooled tensor.  c % 16 == 0. */
int sp_maxpool2_bwd_idx(const void* dy, const void* y, const uint32_t* idx, void* dx, int32_t n, int32_t h, int32_t w_, int32_t c,
                        int32_t dtype, sp_stream_t stream);
int sp_adaptive_avgpool_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t oh,
                            int32_t ow, int32_t act_in, int32_t dtype, sp_stream_t stream);
int sp_adaptive_avgpool_bwd(const void* dy, const void* x, void* dx, int32_t n, int32_t h, int32_t w_, int32_t c,
                            int32_t oh, int32_t ow, int32_t act_in, int32_t dtype, sp_stream_t stream);
int sp_upsample2_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype,
                     sp_stream_t stream);
int sp_upsample2_bwd(const void* dy, void* dx, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype,
                     sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SAGAN attention core (torch.bmm + softmax + torch.bmm at models.py:262-270): o = softmax(q k^T) v, no
 * 1/sqrt(d) scale.  q [b][n][d], k [b][nk][d], v [b][nk][dv], o [b][n][dv]; lse [b][n] fp32 saved for backward.
 * Backward: dk_f32 / dv_f32 are fp32 scratch of sp_attention_bwd_slabs() slabs of [b][nk][d] resp. [b][nk][dv] floats (one
 * partial sum per query block - 64 queries on the bf16 MFMA path, 32 or 16 on the fp32 path - added in block order by the
 * call: no atomics, no initialisation needed); dk / dv receive the result.  Where K and V fit the LDS next to the block's tiles
 * the MFMA backward sums the query blocks a block walks in registers and uses only the first sp_attention_plan() slabs; it
 * neither writes nor reads the rest.  The walk follows the batch, so an image's dk / dv may differ in the last fp32 bits
 * between batch sizes; the same call gives the same bits every time.
 * ---------------------------------------------------------------------------------------------- */
int sp_attention_bwd_slabs(int32_t n, int32_t nk, int32_t d, int32_t dv, int32_t dtype, int64_t* slabs_out);
int sp_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int32_t batch, int32_t n,
                     int32_t nk, int32_t d, int32_t dv, int32_t dtype, sp_stream_t stream);
int sp_attention_bwd(const void* q, const void* k, const void* v, const void* dout, const float* lse, void* dq,
                     float* dk_f32, float* dv_f32, void* dk, void* dv_out, int32_t batch, int32_t n, int32_t nk,
                     int32_t d, int32_t dv, int32_t dtype, sp_stream_t stream);
/* *fwd / *bwd = the kernel sp_attention_fwd / sp_attention_bwd would launch for these extents and this storage type: "mfma",
 * "valu tq32" or "valu tq16" (the VALU kernels in their 32- and 16-query forms).  Same extent checks as the launchers, the same
 * predicates as their dispatch; host-only like sp_conv2d_route: touches no device state, callable without a GPU. */
int sp_attention_route(int32_t n, int32_t nk, int32_t d, int32_t dv, int32_t dtype, const char** fwd, const char** bwd);
/* The walk of the MFMA kernels for a launch of `batch` images on a device of `cus` compute units (cus <= 0: the current device's,
 * read once): *fwd_walk / *bwd_walk = consecutive 64-query blocks one block walks (0: the forward is not on the MFMA kernel / the
 * backward is not on its K/V-resident form), *bwd_slabs = the slabs of the scratch the backward writes and adds.  A pure
 * function of its arguments and SP_TUNE_ATTN_PIECES; host-only with cus > 0. */
int sp_attention_plan(int32_t batch, int32_t n, int32_t nk, int32_t d, int32_t dv, int32_t dtype, int32_t cus,
                      int32_t* fwd_walk, int32_t* bwd_walk, int32_t* bwd_slabs);

/* ------------------------------------------------------------------------------------------------
 * Glue: image ingest (NCHW/NHWC 3-channel source -> padded NHWC, optional affine = kornia.normalize at
 * models.py:195-197; scale3/shift3 are HOST pointers to 3 floats), mask application (models.py:78,80,94),
 * activations, attention residual (models.py:274), NCHW-flatten <-> NHWC permutation (models.py:83,208),
 * per-channel sums (bias gradients).
 * Every entry of this group refuses, before any launch, a `dtype` other than SP_F32 / SP_BF16 / SP_F16 with SP_ERR_UNSUPPORTED
 * (SP_F8 and SP_F8_F16 included: these kernels have no fp8 form); sp_act_fwd / sp_act_bwd refuse an `act` outside sp_act likewise.
 * src_dtype is SP_F32 or the storage type itself.  The two 16-bit types never mix, in sp_ingest_image and in every sp_augment_*_ingest
 * entry with a src_dtype: an SP_BF16 source under SP_F16 storage, and an SP_F16 source under SP_BF16 or SP_F32 storage, are
 * SP_ERR_UNSUPPORTED and nothing is launched (each compilation of the kernels decodes a 16-bit source as ITS 16-bit type).
 * sp_act_fwd: NONE copies, LeakyReLU is max(v, fl32(0.2f v)), ReLU(NaN) = 0 (fmaxf, as the convolution epilogues' v > 0 ? v : 0), NaN
 * passes through the other three.  DESIGN.md section 21.
 * ---------------------------------------------------------------------------------------------- */
int sp_ingest_image(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                    int32_t n, int32_t c, int32_t h, int32_t w_, int32_t cp, const float* scale3,
                    const float* shift3, int32_t dtype, sp_stream_t stream);
int sp_ingest_image_bwd(const void* dy, int32_t cp, void* dsrc, int32_t c, int64_t pixels, const float* scale3,
                        int32_t dtype, sp_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Differentiable augmentation inside the ingest pass (Zhao et al. 2020, "DiffAugment").  The reference has NO counterpart: its
 * discriminator sees the images as they are (model_wrapper.py:153-155,174).  Off unless a caller asks for it.
 *
 * One application takes one row u of 8 fp32 uniforms in [0, 1) per image (a DEVICE pointer, n x 8, decoded in the kernel: no host
 * value depends on it) and `policy`, any OR of SP_AUG_COLOR / SP_AUG_TRANSLATION / SP_AUG_CUTOUT; a part that is left out is the
 * identity.  Images are 3-channel, H x W.  Arithmetic is fp32 whatever the storage type.  Forward, in this order:
 *   color        o = u0 - 0.5, s = 2 u1, k = u2 + 0.5
 *                b = x + o                                        brightness
 *                a = (b - m) s + m,  m = (b_0 + b_1 + b_2) / 3    saturation (per pixel, over the 3 channels)
 *                e = (a - M) k + M,  M = sum(x) / (3 H W) + o     contrast; saturation keeps the per-pixel channel mean, so the mean
 *                                                                 of a over (c, h, w) is the mean of the raw input plus o
 *   translation  r_y = int(H / 8 + 0.5), t_y = min(int(floorf(u3 * float(2 r_y + 1))), 2 r_y) - r_y; t_x likewise from W and u4
 *                (one fp32 multiply, then floor);  out[h, w] = e[h + t_y, w + t_x], 0 outside the frame
 *   cutout       q_y = int(H / 2 + 0.5), n_y = H + 1 - (q_y % 2), c_y = min(int(floorf(u5 * float(n_y))), n_y - 1); the rows
 *                [c_y - q_y / 2, c_y - q_y / 2 + q_y) (integer division) cut with [0, H); columns likewise from W and u6; the output
 *                is 0 inside the window.  u7 is unused by sp_augment_ingest / _bwd; on the gated entries below it is the gate's draw.
 * Backward, for dy on the output:
 *   g1[c, h, w] = dy[c, h - t_y, w - t_x] where that position is inside the frame and outside the window, else 0
 *   Gm = sum(g1) / (3 H W);  g2 = k g1 + (1 - k) Gm  (every input pixel);  dx_c = s g2_c + (1 - s) (g2_0 + g2_1 + g2_2) / 3
 *
 * sp_augment_ingest stands where sp_ingest_image stands: the same source (any strides, fp32 or the compute type), the same
 * destination (padded NHWC of cp channels in the compute type, padding channels zero); sp_augment_ingest_bwd stands where
 * sp_ingest_image_bwd stands (padded dy -> NHWC gradient of pitch 3 in dy's type).  With SP_AUG_COLOR each is TWO launches: a
 * statistics launch (forward: sums of x; backward: sums of g1 over the 3 real channels of dy) that writes one fp32 partial per
 * slice of an image into `partials` (n x sp_augment_slices() floats, no initialisation needed), and the apply launch, which adds
 * an image's partials in slice order - no float atomics, bit-identical from run to run.  Without SP_AUG_COLOR: one launch, pure
 * data movement, `partials` may be NULL.
 * ---------------------------------------------------------------------------------------------- */
enum { SP_AUG_COLOR = 1, SP_AUG_TRANSLATION = 2, SP_AUG_CUTOUT = 4 };
/* partials per image of the statistics launch (backward != 0: of sp_augment_ingest_bwd); host-only */
int sp_augment_slices(int32_t h, int32_t w_, int32_t backward, int64_t* slices_out);
int sp_augment_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                      int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, float* partials,
                      int32_t dtype, sp_stream_t stream);
int sp_augment_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                          int32_t policy, float* partials, int32_t dtype, sp_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Adaptive augmentation (Karras et al. 2020, "ADA"): each image is transformed with a probability p that lives in DEVICE memory and
 * is steered by an overfitting signal from the discriminator's predictions on the real images.  The reference has NO counterpart.
 *
 * THE GATE.  sp_augment_ingest_gated / sp_augment_ingest_bwd_gated take the arguments of sp_augment_ingest / sp_augment_ingest_bwd
 * plus p_dev, one fp32 value in device memory, read when the kernel RUNS (a captured graph follows it without a re-capture):
 *   image n is LIVE iff u[n * 8 + 7] < p_dev[0]   (strict, fp32; u7 is the one uniform of a row the transform itself does not read)
 *   a live image gets exactly what the ungated entry computes for it;
 *   a dead image gets BIT FOR BIT what sp_ingest_image / sp_ingest_image_bwd write for it with scale3 / shift3 NULL, in every storage
 *   type: no color arithmetic ((b - m) * 1 + m is not the identity in fp32), no translation, no window.
 * p_dev[0] = 1.0f therefore equals the ungated entries bit for bit and p_dev[0] = 0.0f is the plain ingest.  The statistics launches
 * skip a dead image's blocks: its partials are never written and never read, and `partials` still needs no initialisation.  Fixed-order
 * partial sums, no float atomics, as the ungated entries (the same kernels).  A NULL p_dev is refused (SP_ERR_INVALID, nothing launched).
 *
 * THE CONTROLLER.  Two one-block launches on ONE state buffer of 8 x 4 bytes in device memory (4-byte aligned):
 *   slot 0 f32 p   1 f32 r_last   2 i32 pos   3 i32 neg   4 i32 total   5 i32 steps   6 i32 adjustments   7 reserved, zero
 *   sp_ada_observe  pos += #(pred[i] > threshold), neg += #(pred[i] < threshold), total += numel.  Equal values and NaN count in total
 *                   only.  Integer arithmetic: the result does not depend on any order.  numel in [1, 2^24], else refused.
 *   sp_ada_adjust   steps += 1.  If steps >= interval: steps = 0, and if total > 0 also
 *                     r = float(pos - neg) / float(total)        both conversions round to nearest; ONE fp32 division
 *                     p = fminf(1, fmaxf(0, p + d)),  d = step if r > target, -step if r < target, else 0        ONE fp32 addition
 *                     r_last = r;  pos = neg = total = 0;  adjustments += 1
 *                   (a full window with total == 0 only starts the step count again).  interval >= 1, step in [0, 1], target in
 *                   [-1, 1], else refused (NaN included).  A refusal launches nothing and leaves the state as it is.
 * &state[0] is what the gated entries take as p_dev.
 * ---------------------------------------------------------------------------------------------- */
int sp_augment_ingest_gated(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                            int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, float* partials,
                            const float* p_dev, int32_t dtype, sp_stream_t stream);
int sp_augment_ingest_bwd_gated(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                                int32_t policy, float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream);
int sp_ada_observe(const float* pred, int64_t numel, float threshold, void* state, sp_stream_t stream);
int sp_ada_adjust(void* state, int32_t interval, float target, float step, sp_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Adaptive pseudo augmentation (Jiang et al. 2021, "Deceive D", APA): with a probability p that lives in DEVICE memory, an image of
 * the discriminator's real branch is replaced by a generated one that keeps the "real" label.  The reference has NO counterpart.
 * csrc/apa.hip, DESIGN.md section 22.  ONE launch, pure data movement:
 *   dst      contiguous fp32 n x 3 x h x w_
 *   dst[i] = float(fake[i])  iff  w_u[i] < p_dev[0]   (strict, fp32 - the gate's compare above; a NaN p takes nothing)
 *            float(real[i])  otherwise
 * real / fake: 3-channel batches with the ELEMENT strides (rn, rc, rh, rw) / (fn, fc, fh, fw) of their n, c, h, w axes (any layout;
 * strides >= 0), each of type real_dtype / fake_dtype: SP_F32 or the storage type `dtype`, under sp_ingest_image's rule - the two
 * 16-bit types never mix: an SP_BF16 source under SP_F16 storage, and an SP_F16 source under SP_BF16 or SP_F32 storage, are
 * SP_ERR_UNSUPPORTED and nothing is launched.  `dtype` chooses the compilation that decodes a 16-bit source, nothing else.
 * A 16-bit value is widened exactly; an fp32 value passes bit for bit, NaN payloads and infinities included.
 * w_u: n fp32 uniforms in device memory, one per image; p_dev: one fp32 value in device memory (&state[0] of the controller above,
 * in an instance of its own).  Both are read when the kernel RUNS: no host value, grid size or address depends on them, and a captured
 * graph follows p without a re-capture.  An image's choice is uniform over a block (grid: blocks x images), so a block reads only the
 * source it chose.  No atomics, no reduction: two runs give the same bits.  dst must not overlap a source.
 * Refused with SP_ERR_INVALID before any launch: a NULL real, fake, dst, w_u or p_dev; n, h or w_ < 1 (and n > 65535, h * w_ > 2^28);
 * a dtype, real_dtype or fake_dtype that is no SP_F32 / SP_BF16 / SP_F16; a negative stride.
 * ---------------------------------------------------------------------------------------------- */
int sp_apa_select(const void* real, int32_t real_dtype, int64_t rn, int64_t rc, int64_t rh, int64_t rw,
                  const void* fake, int32_t fake_dtype, int64_t fn, int64_t fc, int64_t fh, int64_t fw,
                  float* dst, int32_t n, int32_t h, int32_t w_,
                  const float* w_u, const float* p_dev, int32_t dtype, sp_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Geometric augmentation inside the ingest pass (Karras et al. 2020, "ADA": pixel blitting and general geometric transforms): x-flip,
 * 90-degree rotations, isotropic scaling and arbitrary rotation compose with the translation above into ONE 2 x 3 affine map per image,
 * applied by bilinear resampling; the backward pass is the exact adjoint computed by GATHER (no float atomics, fixed summation order).
 * The reference has NO counterpart.  DESIGN.md section 16.
 *
 * One application takes the image's row u of 8 uniforms, with the meaning above (u0-u2 color, u3-u4 translation, u5-u6 cutout, u7 the
 * gate), a row v of 4 fp32 uniforms in [0, 1) and `geom`, any OR of SP_GEOM_*; a part that is left out is the identity and is not computed.
 * Decode (fp32):
 *   flip  = v0 < 0.5f
 *   k     = min(int(floorf(4 * v1)), 3)
 *   e     = 0.8f * v2 - 0.4f, g = exp2f(-e): the image is magnified by 2^e, in [0.758, 1.32)
 *   theta = (v3 - 0.5f) * float(pi / 2), c = cosf(theta), s = sinf(theta): [-45, 45) degrees, so with rot90 the whole circle is reached
 *   t_y, t_x from u3, u4 as above (0 without SP_AUG_TRANSLATION);  cy = (H - 1) / 2, cx = (W - 1) / 2
 * The INVERSE map takes an output pixel (h, w) to source coordinates (y, x).  Its linear part, rows in (y, x) order, is
 *   L = F . Q^k . g . [[c, -s], [s, c]],   Q = [[0, 1], [-1, 0]] applied as exact row swaps and sign changes,   F = diag(1, -1) if flip
 * and the full map is (y, x) = L . ((h, w) + (t_y, t_x) - (cy, cx)) + (cy, cx).  The table row of an image is
 *   {m00, m01, m02, m10, m11, m12, 0, 0},   (m00 m01; m10 m11) = L,   (m02, m12) = L . (t_y - cy, t_x - cx) + (cy, cx)
 * evaluated as m02 = (m00 (t_y - cy) + m01 (t_x - cx)) + cy with every product and sum rounded once.  A row without scale and rotate is
 * EXACT: entries in {-1, 0, 1}, exact offsets.  SP_GEOM_ROT90 needs H == W.
 * Forward, with e the color transform above of the SOURCE (pointwise, evaluated at each tap; its mean is still one reduction of the
 * raw input):
 *   y = (m00 h + m01 w) + m02, x = (m10 h + m11 w) + m12   every product and sum rounded once to fp32 (no fused multiply-add), so that
 *   y0 = floorf(y), fy = y - y0; x0, fx likewise            both passes see the same coordinates
 *   out[c, h, w] = (1 - fy) ((1 - fx) e[y0, x0] + fx e[y0, x0 + 1]) + fy ((1 - fx) e[y0 + 1, x0] + fx e[y0 + 1, x0 + 1])
 *   a tap outside the frame contributes 0 (zero padding: grid_sample(bilinear, zeros, align_corners=True) on the same coordinates);
 *   then the cutout window, in OUTPUT coordinates, zeroes its pixels.
 * Backward:  g1[c, i, j] = sum over output pixels (h, w) outside the window of omega(h, w -> i, j) dy[c, h, w], omega the bilinear weight
 * above; then the color backward unchanged (Gm = sum(g1) / (3 H W), g2, dx).  For source pixel (i, j) the contributing outputs lie
 * within |h - round(q_y)| <= 2, |w - round(q_x)| <= 2 of q = L^-1 ((i, j) - (m02, m12)): at most 25 candidates, each one's (y, x)
 * recomputed with the forward's expression, accumulated in row-major order; the candidate ranges are clipped to the frame BEFORE the
 * loops, so no index depends on the table's values.  sum(g1) is taken over OUTPUT pixels outside the window as
 * sum (dy_0 + dy_1 + dy_2) (sum of the in-frame tap weights), partials in a fixed order.
 * The apply entries are specified for the tables the decode writes and for any table whose linear part's inverse A = L^-1 has
 * |a00| + |a01| <= 2 and |a10| + |a11| <= 2 (the pre-image of a tap square then has half-extent <= 2 per axis, and rounding adds 0.5).
 * Any other table (a singular one, NaN) is still safe - every index is checked against the frame - but the backward may miss
 * contributions.
 *
 * sp_augment_geom_decode      ONE tiny launch: n x 8 floats into `table` from u (n x 8) and v (n x 4); reads only `policy`'s
 *                             translation bit.  geom in 1 ... 15, else refused.
 * sp_augment_geom_ingest      stands where sp_augment_ingest_gated stands; sp_augment_geom_ingest_bwd where sp_augment_ingest_bwd_gated
 *                             stands.  `policy` contributes its color and cutout bits only: the translation is in the table.  p_dev is
 *                             the gate (image n is live iff u[n * 8 + 7] < p_dev[0]; a dead image gets bit for bit what
 *                             sp_ingest_image(_bwd) writes); p_dev == NULL: every image is live.
 * sp_augment_geom_slices      host-only: sizes `partials` (n x slices floats, needed with SP_AUG_COLOR only).
 * Refusals launch nothing: NULL pointers, cp < 3, a bad dtype, a bad geom, rot90 on a non-square map, missing partials with color.
 * ---------------------------------------------------------------------------------------------- */
enum { SP_GEOM_XFLIP = 1, SP_GEOM_ROT90 = 2, SP_GEOM_SCALE = 4, SP_GEOM_ROTATE = 8 };
int sp_augment_geom_slices(int32_t h, int32_t w_, int32_t backward, int64_t* slices_out);
int sp_augment_geom_decode(const float* u, const float* v, int32_t n, int32_t h, int32_t w_, int32_t policy, int32_t geom,
                           float* table, sp_stream_t stream);
int sp_augment_geom_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                           int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, const float* table,
                           float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream);
int sp_augment_geom_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                               int32_t policy, const float* table, float* partials, const float* p_dev, int32_t dtype,
                               sp_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * ADA's color group inside the ingest pass (Karras et al. 2020, "ADA": brightness, contrast, luma flip, hue rotation, saturation): ONE
 * affine map of RGB per image, a 3 x 4 matrix.  No reduction and no launch besides one decode per step; the backward is the transposed
 * 3 x 3 matrix.  The reference has NO counterpart.  DESIGN.md section 20.
 *
 * Images are 3-channel, valued as the generator emits them (contrast and luma flip act about 0); fp32 arithmetic whatever the storage
 * type.  One application takes the image's rows u and v with their meaning unchanged, a row z of 8 fp32 uniforms in [0, 1) and `cmat`,
 * any OR of SP_CMAT_*; a part that is left out is the identity and is not computed.
 * Decode (fp32, every product and sum rounded once), with nrm(a, b) = sqrtf(-2 * logf(1 - a)) * cosf(float(2 pi) * b) (Box-Muller;
 * 1 - a >= 2^-24, so |nrm| <= 5.77):
 *   brightness  bb = 0.2f * nrm(z0, z1)                                                   left out: 0
 *   contrast    c  = exp2f(0.5f * nrm(z2, z3))                                            left out: 1
 *   saturation  s  = exp2f(nrm(z4, z5))                                                   left out: 1
 *   hue         theta = (2 z6 - 1) * float(pi), cs = cosf(theta), sn = sinf(theta)        left out: cs = 1, sn = 0 exactly
 *   luma flip   f  = z7 < 0.5f ? -1 : 1                                                   left out: 1
 * With P = J / 3 the projector on the grey axis (1, 1, 1) / sqrt 3, Q = I - P and K the cross-product matrix of that axis, ADA's five
 * homogeneous matrices in its order (brightness, contrast, luma flip, hue, saturation, each multiplied on the left) collapse to
 *   out = Lm x + t (1, 1, 1),   Lm = c (f P + s cos(theta) Q + s sin(theta) K),   t = c f bb
 * evaluated as  p = c f;  cs_ = c s;  beta = cs_ cs;  gamma = (cs_ sn) float(1 / sqrt 3);  d = (p - beta) / 3;
 *   Lm_ii = beta + d;  Lm_01 = Lm_12 = Lm_20 = d - gamma;  Lm_02 = Lm_10 = Lm_21 = d + gamma;  t = p bb.
 * (float(1 / sqrt 3) is the kernel's fp32 rounding of the closed form's constant 1 / sqrt 3, a rounding like any other of the decode:
 * a float64 reference of Lm uses 1 / sqrt 3 itself, which differs by 3e-8 relative in gamma.)
 * A row with brightness and / or contrast alone is exactly diag(c) with offset c bb; luma flip alone is I - 2 J / 3 to rounding.
 * Table row (the "ctable"): 12 floats {L00, L01, L02, t, L10, L11, L12, t, L20, L21, L22, t}: three 16-byte quadruples, row-major.
 * Forward: the last step of the pointwise color stage e of the SOURCE pixel - after `color` above when that is on too, before
 * translation / resampling / cutout:  e'_r = ((L_r0 e_0 + L_r1 e_1) + L_r2 e_2) + L_r3  (the kernel may contract into FMAs).  In the
 * geometric family it is evaluated at each tap, so a tap outside the frame still contributes 0 and the window still zeroes its outputs.
 * Backward: after the family's g1,  g1'_c = (L_0c g1_0 + L_1c g1_1) + L_2c g1_2,  then the color backward unchanged on g1'.  Its
 * statistics launch takes sum(g1') per output pixel as (k0 dy_0 + k1 dy_1) + k2 dy_2, k_r = (L_r0 + L_r1) + L_r2, times the in-frame tap
 * weights in the geometric family.  Without SP_AUG_COLOR there is no statistics launch in either direction.  The gate is unchanged.
 *
 * sp_augment_cmat_decode      ONE tiny launch: n x 12 floats into `ctable` from z (n x 8).  cmat in 1 ... 31 and n in 1 ... 2^24, else
 *                             refused.
 * sp_augment_cmat_ingest      `table` NULL: stands where sp_augment_ingest_gated stands (the plain family); non-NULL: where
 * sp_augment_cmat_ingest_bwd  sp_augment_geom_ingest stands.  p_dev NULL: every image is live.  ANY 3 x 4 ctable is admitted, not only
 *                             decoded ones.  `partials` is sized by sp_augment_slices / sp_augment_geom_slices as before.
 * `ctable` must be 16-byte aligned in all three entries (a row is read and written as three 16-byte quadruples; a row's pitch of 48
 * bytes keeps every row aligned).
 * Refusals launch nothing: NULL z / ctable, a ctable that is not 16-byte aligned, a bad cmat, n <= 0 (decode: n > 2^24), and everything
 * the entries above refuse.
 * ---------------------------------------------------------------------------------------------- */
enum { SP_CMAT_BRIGHTNESS = 1, SP_CMAT_CONTRAST = 2, SP_CMAT_LUMAFLIP = 4, SP_CMAT_HUE = 8, SP_CMAT_SATURATION = 16 };
int sp_augment_cmat_decode(const float* z, int32_t n, int32_t cmat, float* ctable, sp_stream_t stream);
int sp_augment_cmat_ingest(const void* src, int32_t src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* dst,
                           int32_t n, int32_t h, int32_t w_, int32_t cp, const float* u, int32_t policy, const float* table,
                           const float* ctable, float* partials, const float* p_dev, int32_t dtype, sp_stream_t stream);
int sp_augment_cmat_ingest_bwd(const void* dy, int32_t cp, void* dsrc, int32_t n, int32_t h, int32_t w_, const float* u,
                               int32_t policy, const float* table, const float* ctable, float* partials, const float* p_dev,
                               int32_t dtype, sp_stream_t stream);
int sp_mask_concat(const void* feat, const float* mask, void* out, int64_t pixels, int32_t c, int32_t cp,
                   int32_t dtype, sp_stream_t stream);
int sp_mask_mul_2d(const void* feat, int32_t ldf, const float* mask, void* out, int32_t ldo, int32_t batch,
                   int32_t k, int32_t dtype, sp_stream_t stream);
int sp_act_fwd(const void* x, void* y, int64_t numel, int32_t act, int32_t dtype, sp_stream_t stream);
/* dz = dy * act'(.) evaluated from the POST-activation y; pitch c -> cp (zero padded). */
int sp_act_bwd(const void* dy, const void* y, void* dz, int64_t pixels, int32_t c, int32_t cp, int32_t act,
               int32_t dtype, sp_stream_t stream);
int sp_scale_add(const void* a, const void* b, const float* g, void* y, int64_t numel, int32_t dtype,
                 sp_stream_t stream);
/* y[row][c] = (x[row][c] - bias[c]) * (sig_a[0] * sig_b[1]) + bias[c]: the output of a spectral-normalised layer re-expressed under
 * the sigma of ANOTHER forward of the same weights - conv(x, W / sigma_b) + b from conv(x, W / sigma_a) + b without running the layer
 * again.  The generator's masked-feature mappings (models.py:78-94) see the same pyramid, masks and weight_orig in both generator
 * forwards of a step (model_wrapper.py:147-151,168-172); only the power iteration has advanced.  sig_a / sig_b: DEVICE pointers to
 * the {sigma, 1 / sigma} pairs in the two sp_sn_forward scratches; rows x c elements, pitches ldx / ldy; bias may be NULL. */
int sp_rescale_bias(const void* x, void* y, int64_t rows, int32_t c, int32_t ldx, int32_t ldy, const float* bias, const float* sig_a,
                    const float* sig_b, int32_t dtype, sp_stream_t stream);
/* dg[0] = <dy, a>: per-block partial sums in `partials` (512 floats of scratch), added in block order by a second kernel */
int sp_scale_add_bwd(const void* dy, const void* a, const float* g, void* da, float* dg, float* partials, int64_t numel,
                     int32_t dtype, sp_stream_t stream);
int sp_permute_chw_hwc(const void* src, void* dst, int32_t batch, int32_t c, int32_t hw, int32_t to_hwc,
                       int32_t dtype, sp_stream_t stream);
/* out[c] = sum over pixels; partials: 512 * c floats of scratch (per-block partial rows, added in block order) */
int sp_channel_sum(const void* x, int32_t ld, int64_t pixels, int32_t c, float* out, float* partials, int32_t dtype,
                   sp_stream_t stream);
int sp_f64_to_f32(const double* src, float* dst, int32_t n, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Discriminator head (models.py:149-155; pred is the (B,B,F) tensor the reference produces) and the
 * losses (lossfunction.py:137,164 LSGAN; :31-68 semantic reconstruction, one call per pyramid level,
 * accumulating into acc; :92-110 diversity).  gout = device pointer to the upstream gradient scalar.
 * sp_dhead_bwd: scratch = `batch` floats (per-sample sums handed from the first kernel to the second; no initialisation; the
 * call keeps no state of its own, so it is re-entrant per stream); demb [num_classes][f] is zeroed by the call.
 * ---------------------------------------------------------------------------------------------- */
int sp_dhead_fwd(const void* x, int32_t ldx, const float* emb_sn, const int64_t* cls, const float* wc,
                 const float* bc, float* pred, int32_t batch, int32_t f, int32_t dtype, sp_stream_t stream);
int sp_dhead_bwd(const float* dpred, const void* x, int32_t ldx, const float* emb_sn, const int64_t* cls,
                 const float* wc, void* dx, int32_t lddx, float* demb, int32_t num_classes, float* dwc, float* dbc,
                 float* scratch, int32_t batch, int32_t f, int32_t dtype, sp_stream_t stream);
int sp_sqerr_loss_fwd(const float* p, int64_t numel, float target, double* acc_tmp, float* loss, sp_stream_t stream);
int sp_sqerr_loss_bwd(const float* p, int64_t numel, float target, const float* gout, float* dp, sp_stream_t stream);
int sp_rec_loss_fwd(const void* real, int32_t ld_real, const void* fake, int32_t ld_fake, const float* mask,
                    int32_t n, int32_t h, int32_t w_, int32_t c, double* acc, int32_t dtype, sp_stream_t stream);
int sp_rec_loss_bwd(const void* real, int32_t ld_real, const void* fake, int32_t ld_fake, const float* mask,
                    const float* gout, void* dfake, int32_t ld_dfake, int32_t n, int32_t h, int32_t w_, int32_t c,
                    int32_t dtype, sp_stream_t stream);
int sp_div_loss_fwd(const void* img, int64_t half_elems, const float* z, int64_t half_z, double* acc_tmp,
                    float* out2, int32_t dtype, sp_stream_t stream);
int sp_div_loss_bwd(const void* img, int64_t half_elems, const float* fwd_out2, const float* gout, void* dimg,
                    int32_t dtype, sp_stream_t stream);
/* One-launch forms of the loss plumbing (a small launch costs ~5 us of queue time whatever it computes; the three generator losses
 * used to take 36 launches).  `weight`: the factor the caller multiplies the loss by (model_wrapper.py:183-186's w_rec / w_div) - the
 * value written is weight * loss and the backward forms scale by it, so no elementwise launch is needed around them.  `acc`: fp64
 * accumulators (1 for the reconstruction loss, 2 for the diversity loss) that are ZERO on entry and left zero: allocate and clear
 * once, pass to every call of one stream.
 * sp_rec_loss_fwd_levels / _bwd_levels: all pyramid levels (<= 8) of lossfunction.py:31-68 in one launch each; a level with
 * h = w_ = 1 is a 2-D (fully connected) level with c features per row.  sp_sqerr_loss_fwd itself runs as one block up to 2^18 elements. */
typedef struct sp_rec_level {
    const void* real; const void* fake; const float* mask;
    void* dfake;                                   /* backward only */
    int32_t ld_real, ld_fake, ld_dfake, n, h, w_, c, reserved_;
} sp_rec_level;
int sp_rec_loss_fwd_levels(const sp_rec_level* levels, int32_t n_levels, double* acc, float* loss, float weight,
                           int32_t dtype, sp_stream_t stream);
int sp_rec_loss_bwd_levels(const sp_rec_level* levels, int32_t n_levels, const float* gout, float weight,
                           int32_t dtype, sp_stream_t stream);
int sp_div_loss_fwd_w(const void* img, int64_t half_elems, const float* z, int64_t half_z, double* acc,
                      float* out2, float weight, int32_t dtype, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Hinge and non-saturating logistic adversarial losses, and the LeCam regularizer of the discriminator (Tseng et al., CVPR 2021,
 * "Regularizing GANs under limited data").  The reference has NO counterpart (it trains with LSGAN, sp_sqerr_loss_*).  DESIGN.md
 * section 18.  fp32 only: p is a contiguous fp32 tensor of `numel` predictions, numel in [1, 2^24], else refused; a refusal launches
 * nothing (and leaves the LeCam state as it is).
 *
 * sp_gan_loss_fwd   loss[0] = (float)(sum f(p[i]) / numel), kind 0 = hinge, 1 = logistic; role 0 = D on real, 1 = D on fake, 2 = G:
 *                       hinge     max(0, 1 - p)    max(0, 1 + p)    -p
 *                       logistic  softplus(-p)     softplus(p)      softplus(-p)      softplus(x) = max(x, 0) + log1pf(expf(-|x|))
 *                   ONE block: fp32 partial sums in a fixed order, combined in double, rounded once.  No atomics.  A NaN prediction
 *                   gives a NaN loss.
 * sp_gan_loss_bwd   dp[i] = c * f'(p[i]),  c = gout[0] / (float)numel (one fp32 division).  Hinge: -c / +c where the argument of max is
 *                   > 0 strictly, 0 where it is <= 0 (torch's relu convention), -c for G.  Logistic: -/+ c * sigmoid(-/+ p), sigmoid(x)
 *                   = 1 / (1 + expf(-x)) for x >= 0, e / (1 + e) with e = expf(x) otherwise (no overflow for any finite x).  A NaN
 *                   prediction gives a NaN dp at that element - never a silent zero.
 *
 * THE LECAM STATE.  8 x 4 bytes in device memory (4-byte aligned):
 *   slot 0 f32 a_real   1 f32 a_fake   2 i32 updates   3 i32 active   4 f32 m_real   5 f32 m_fake   6, 7 zero
 * sp_lecam_fwd      one block, in this order:  m_r = (float)(sum(pred_real) / numel), m_f likewise (slots 4, 5);  k = updates;
 *                   if both means are finite:  k < start: a_real = m_r, a_fake = m_f;  else a = fadd(fmul(decay, a), fmul(1.0f - decay, m))
 *                   (three fp32 roundings, no FMA);  updates = min(k + 1, 2^31 - 1);   active = (k >= start);
 *                   reg[0] = active ? (float)((double)weight * (S_r + S_f) / numel) : 0,  S_r = sum h(pred_real - a_fake)^2,
 *                   S_f = sum h(a_real - pred_fake)^2 with the UPDATED anchors, h(x) = x or, rectified != 0, max(x, 0).
 *                   weight >= 0 finite, decay in [0, 1), start >= 0, else refused (NaN included).
 * sp_lecam_bwd      dpred_real[i] = active ? c * h(pred_real[i] - a_fake) : 0,  dpred_fake[i] = active ? -c * h(a_real - pred_fake[i]) : 0,
 *                   c = gout[0] * weight * (2 / numel) in fp32; the anchors and `active` are read from the state the forward left.
 * ---------------------------------------------------------------------------------------------- */
int sp_gan_loss_fwd(const float* p, int64_t numel, int32_t kind, int32_t role, float* loss, sp_stream_t stream);
int sp_gan_loss_bwd(const float* p, int64_t numel, int32_t kind, int32_t role, const float* gout, float* dp, sp_stream_t stream);
int sp_lecam_fwd(const float* pred_real, const float* pred_fake, int64_t numel, float weight, float decay, int32_t start,
                 int32_t rectified, void* state, float* reg, sp_stream_t stream);
int sp_lecam_bwd(const float* pred_real, const float* pred_fake, int64_t numel, float weight, int32_t rectified, const void* state,
                 const float* gout, float* dpred_real, float* dpred_fake, sp_stream_t stream);

/* fp8 (OCP e4m3) helpers of the SP_F8 convolution path (BASELINE.json config 5).
 * sp_quantize_fp8: q[i] = e4m3(sat(x[i] * inv_scale[0])) for a bf16 / fp32 tensor of `numel` elements (numel % 16 == 0);
 *   amax (may be NULL): max|x| merged into amax[0].
 * sp_pack_weight_fp8: conv weight [cout][cin][3][3] fp32 (OIHW, the frozen VGG-16 filters) -> e4m3 [cout][9][cin_p] in the
 *   forward packing of sp_conv2d_igemm with ONE scale per output channel, w_scale[co] = max|w[co]| / 448 (pad channels zero).
 * sp_fp8_update_scales: delayed scaling - for each of n slots: if amax[i] > 0: scale[i] = margin * amax[i] / 448,
 *   inv_scale[i] = 1 / scale[i]; amax[i] = 0.  One launch, no host sync. */
int sp_quantize_fp8(const void* x, void* q, int64_t numel, const float* inv_scale, float* amax, int32_t dtype, sp_stream_t stream);
int sp_pack_weight_fp8(const float* w, int32_t cout, int32_t cin, int32_t cin_p, void* out, float* w_scale, sp_stream_t stream);
int sp_fp8_update_scales(float* amax, float* scale, float* inv_scale, int32_t n, float margin, sp_stream_t stream);

/* kornia.normalize_min_max(image[None], min_val=-1, max_val=1) of the reference's data pipeline (/root/reference/data.py:53), for a
 * whole batch on the device: y = (hi - lo) * (x - min) / (max - min + eps) + lo in fp32, operation for operation as torch evaluates
 * it (bit-identical).  x, y: [batch][channels][hw] contiguous fp32 (NCHW, what TVF.to_tensor yields); per_channel != 0: min / max per
 * (image, channel) plane - kornia's definition (x.view(B, C, -1).min(-1)); 0: per image over all channels.  eps: kornia uses 1e-6. */
int sp_minmax_normalize(const float* x, float* y, int32_t batch, int32_t channels, int64_t hw, float lo, float hi, float eps,
                        int32_t per_channel, sp_stream_t stream);

/* A batch of training masks generated on the device: misc.get_masks_for_training
 * (/root/reference/misc.py:13-68) for every sample of the batch in one launch - stage ~ choice([0..6, 0, 1]) counted from the deep
 * end, with probability p_random_mask (reference: 0.3) and 0 < stage < 6 a 0/1 shape map on the next finer level expanded
 * nearest-neighbour to all finer levels, everything deeper than the stage zero, exact 0.0f / 1.0f.  The shape map holds 1 - 4
 * shapes of the four kinds skimage.draw.random_shapes draws (rectangle, circle, triangle, ellipse), each inside a random bounding box.  The seven outputs are the
 * reference's list order, fp32, [batch][1][S][S] contiguous / [batch][4096] / [batch][365].  All randomness is integer
 * arithmetic on splitmix64(seed, sample, draw): the same (seed, batch) gives the same masks on every device, and the oracle
 * restates the generator bit for bit (tests/test_gpu_next_rows.py). */
int sp_training_masks(float* m128, float* m64, float* m32, float* m16, float* m8, float* m4096, float* m365,
                      int32_t batch, uint64_t seed, float p_random_mask, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-tensor Adam: torch.optim.Adam (main.py:64-65; .step() at model_wrapper.py:162,190) for every parameter of
 * a network in one launch.  The host splits the fp32 tensors into chunks (<= 65536 elements each); step_size =
 * lr / (1 - beta1^step) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step) are per parameter (torch keeps a step count
 * per parameter).  amsgrad / maximize are not supported (the reference uses the defaults).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sp_adam_chunk {
    float* p;              /* parameter (updated in place) */
    const float* g;        /* gradient */
    float* m;              /* exp_avg (updated in place) */
    float* v;              /* exp_avg_sq (updated in place) */
    int32_t n;             /* elements in this chunk */
    float step_size;
    float inv_sqrt_bc2;
    float reserved;
} sp_adam_chunk;
/* hyper-parameters are doubles: torch derives (1 - beta) from the Python float and only then rounds to fp32 */
int sp_adam_multi(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                  double weight_decay, sp_stream_t stream);

/* x[i] *= factor for an fp32 buffer (16-byte aligned), in place: takes the static loss scale of the SP_F16 storage mode off a
 * network's flat gradient buffer before the optimizer step (the activation gradients of this network - means over 5e4 ... 5e6
 * elements - would be subnormal in fp16 without it; the reference trains in fp32, model_wrapper.py:160,188). */
int sp_scale_f32(float* x, int64_t numel, float factor, sp_stream_t stream);
int sp_scale_f32_dev(float* x, int64_t numel, const float* factor_dev, sp_stream_t stream);   /* factor_dev[0] read on the device */

/* Dynamic loss scaling of the SP_F16 storage mode, entirely on the device (no host sync, graph-safe; torch.cuda.amp.GradScaler's
 * policy - the reference trains in fp32 and needs none, model_wrapper.py:160-162,188-190).  fp16 activation gradients overflow to
 * inf above 65504 and one such step would poison Adam's moments for good, so per optimizer step:
 *   sp_check_finite        found[0] = 1 if x holds any inf / NaN (x: a network's flat fp32 gradient buffer, 16-byte aligned; found is
 *                          only ever set here - sp_loss_scale_update clears it)
 *   sp_adam_multi_guarded  sp_adam_multi that does NOTHING when skip_if_nonzero[0] != 0 (NULL: plain sp_adam_multi)
 *   sp_loss_scale_update   state = {scale, 1 / scale, clean steps, found, skipped steps}: found -> scale *= backoff (>= 1), clean = 0,
 *                          skipped += 1; else clean += 1 and after `interval` clean steps scale *= growth (<= 2^24); found = 0. */
int sp_check_finite(const float* x, int64_t numel, float* found, sp_stream_t stream);
int sp_adam_multi_guarded(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                          double weight_decay, const float* skip_if_nonzero, sp_stream_t stream);
int sp_loss_scale_update(float* state, float growth, float backoff, int32_t interval, sp_stream_t stream);

/* Gradient clipping by GLOBAL norm with a non-finite guard for every storage mode, entirely on the device (no host sync; the reference
 * has neither: its optimizer step is the bare torch.optim.Adam.step() of model_wrapper.py:162,190).  torch.nn.utils.clip_grad_norm_'s
 * definition, on the chunk table the Adam step already has.  fp32 only, as sp_adam_multi.  Per optimizer step:
 *   sp_grad_sqnorm_multi   partials[c] = sum over chunk c of (double)g[i] * (double)g[i].  One 256-thread block per chunk, float4 loads
 *                          where g is 16-byte aligned, scalar loads otherwise.  Every product is exact in fp64 (24-bit operands: 48 bits),
 *                          only the additions round, and their order is fixed: thread t adds its elements in index order (float4 t,
 *                          t + 256, ... each as x, y, z, w; then the tail elements n4 * 4 + t, + 256, ...), the 64 lanes of a wave meet in
 *                          an xor-shuffle tree (offsets 32, 16, 8, 4, 2, 1), thread 0 adds the four wave sums as ((w0 + w1) + w2) + w3.
 *                          No atomics, nothing depends on launch order.  Reads ONLY the g and n columns of the table (p, m, v may be
 *                          NULL); partials: n_chunks doubles, 8-byte aligned.
 *   sp_grad_clip_finalize  one block: sum = the partials in fp64, again in a fixed order - thread t (of 256) adds partials[t],
 *                          partials[t + 256], ... in index order, then the same wave tree and ((w0 + w1) + w2) + w3 - and
 *                            state[0] = (float)sqrt(sum)                                  the global gradient norm
 *                            state[1] = (float)min(1, max_norm / (sqrt(sum) + 1e-6))      the coefficient: fp64 with correctly rounded sqrt and
 *                                                                                         divide, rounded to fp32 ONCE; 0 when sum is not finite
 *                            state[2] = 1 if sum is not finite (an inf or a NaN among the gradients), else 0      written by every call
 *                            state[3] += 1 when state[2] is set        steps skipped so far (only ever grows)
 *                            state[4] += 1 when state[1] < 1 (finite)  steps clipped so far (only ever grows)
 *                          max_norm = +inf gives exactly 1.0f (monitor and guard, never scale); max_norm <= 0 or NaN and NULL pointers
 *                          are refused (SP_ERR_INVALID, nothing launched).
 *   sp_adam_multi_clipped  sp_adam_multi_guarded (skip_if_nonzero as there, NULL allowed) that ALSO does nothing when clip_state[2] != 0
 *                          and reads fp32(g * clip_state[1]) wherever that kernel reads g: the product is rounded to fp32 once and is
 *                          never contracted into the operation that follows, so the step IS the plain step on gradients scaled by one
 *                          fp32 multiply (Tensor.mul_), and a coefficient of exactly 1.0f is the identity.  The gradients are not
 *                          written.  clip_state: sp_grad_clip_finalize's five floats (required). */
int sp_grad_sqnorm_multi(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double* partials, sp_stream_t stream);
int sp_grad_clip_finalize(const double* partials, int32_t n_partials, double max_norm, float* state, sp_stream_t stream);
int sp_adam_multi_clipped(const sp_adam_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, double eps,
                          double weight_decay, const float* skip_if_nonzero, const float* clip_state, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exponential moving average (EMA) of a network's parameters, kept on the device.  The reference has NO average of its own:
 * it scores, samples and saves the raw last-iterate generator (validate() / inference() at model_wrapper.py:231-296, the checkpoint at
 * model_wrapper.py:215-223).  These two entry points stand beside its generator step (optimizer .step() at model_wrapper.py:190):
 *   sp_ema_multi   avg[i] = avg[i] + (p[i] - avg[i]) * one_minus_decay for every chunk in one launch, in fp32 and in Tensor.lerp_'s
 *                  order (the form sp_adam_multi's first moment uses); launched right behind the optimizer step.  one_minus_decay
 *                  must lie in [0, 1] (NaN is rejected).  skip_if_nonzero: NULL, or a device float - the launch changes NOTHING when it
 *                  is non-zero (sp_adam_multi_guarded's meaning: the optimizer step it follows was skipped).
 *   sp_swap_multi  exchanges avg[i] and p[i]: the average is evaluated (and saved) through the network's own parameter storage - no
 *                  address changes, so captured graphs, the optimizer's chunk tables and the flat gradient buffer stay valid - and a
 *                  second call puts the raw parameters back bit for bit.
 * fp32 only; one 256-thread block per chunk (<= 65536 elements, as sp_adam_chunk), float4 where both pointers of a chunk are 16-byte
 * aligned, scalar otherwise.  A chunk's two ranges must not overlap each other or another chunk's.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sp_ema_chunk {
    float* avg;            /* the average's window (updated / exchanged in place) */
    float* p;              /* parameter (read by sp_ema_multi, exchanged by sp_swap_multi) */
    int32_t n;             /* elements in this chunk */
    int32_t reserved;
} sp_ema_chunk;
int sp_ema_multi(const sp_ema_chunk* chunks_dev, int32_t n_chunks, float one_minus_decay, const float* skip_if_nonzero,
                 sp_stream_t stream);
int sp_swap_multi(const sp_ema_chunk* chunks_dev, int32_t n_chunks, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FID: the Inception-v3 feature extractor (torchvision's Inception3, eval mode, transform_input=False) that
 * /root/reference/frechet_inception_distance.py:11-42 hooks at Mixed_7c, forward only (inception.hip).
 *
 * sp_conv2d_general: one BasicConv2d (conv without bias -> BatchNorm2d(eps=0.001) -> ReLU) with the BatchNorm folded into
 * the packed weights and `bias` on the host - every one of the network's 94 convolutions, the forms torch.nn.Conv2d takes
 * inside torchvision's InceptionA..E and stem (1x1, 3x3, 5x5, 1x7 / 7x1, 1x3 / 3x1; stride 1 or 2; padding per axis):
 *   y[n, oy, ox, co] = act( sum_{ky,kx,c} x[n, oy*stride_h - pad_h + ky, ox*stride_w - pad_w + kx, c] * w[co][ky*kw + kx][c] + bias[co] )
 * oh = (h + 2 pad_h - kh) / stride_h + 1, ow likewise.  x: [n][h][w][ldx] (channels [0, cin_p) read; cin_p % 8 == 0, the 3-channel
 * image is padded to 8), w: [cout][kh*kw][cin_p], y: [n][oh][ow][ldy] - `y` may point INTO a wider tensor (the channel slice of an
 * Inception block's concat, torch.cat(outputs, 1)): channels outside [0, cout) of each row are never written.  cout % 4 == 0,
 * ldy % 4 == 0, kh, kw <= 7, pad < k, act NONE / RELU, x and w 16-byte aligned, y 4-element aligned.  dtype SP_F32 (exact f32
 * MFMA) / SP_BF16 / SP_F16.  struct_bytes must be sizeof(sp_conv_general_params): a caller built against another layout gets
 * SP_ERR_INVALID instead of a misread struct.  Shapes outside the contract: SP_ERR_INVALID, dtypes: SP_ERR_UNSUPPORTED. */
typedef struct sp_conv_general_params {
    int32_t struct_bytes;   /* sizeof(sp_conv_general_params) */
    int32_t dtype;
    const void* x;
    const void* w;
    const float* bias;      /* [cout] or NULL */
    void* y;
    int32_t n, h, w_, cin_p, ldx, cout, ldy, kh, kw, stride_h, stride_w, pad_h, pad_w, act;
} sp_conv_general_params;
int sp_conv2d_general(const sp_conv_general_params* p, sp_stream_t stream);
/* F.max_pool2d(kernel_size=3, stride=2) (Inception3's stem and InceptionB / InceptionD's pool branch): x [n][h][w][ldx] ->
 * y [n][(h-3)/2+1][(w-3)/2+1][ldy], channels [0, c); y may be a channel slice of a wider tensor.  c, ldx, ldy % 4 == 0. */
int sp_maxpool3s2_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype,
                      sp_stream_t stream);
/* F.avg_pool2d(kernel_size=3, stride=1, padding=1) with count_include_pad=True (the divisor is always 9): the pool branch of
 * InceptionA / C / E.  x, y: [n][h][w][c], c % 4 == 0. */
int sp_avgpool3s1_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t dtype, sp_stream_t stream);
/* Input preparation of frechet_inception_distance.py:71-77,92-96: misc.normalize_m1_1_batch (min / max over each WHOLE image,
 * no eps: 2 * ((x - min) / (max - min)) - 1) then F.interpolate(size=(oh, ow), mode='bilinear', align_corners=False) in fp32.
 * x: [n][c][h][w] fp32 (NCHW), minmax: 2n floats of scratch (left holding each image's min, max), y: [n][oh][ow][cp] in dtype,
 * channels [c, cp) zero; cp % 8 == 0. */
int sp_inception_prep(const float* x, float* minmax, void* y, int32_t n, int32_t c, int32_t h, int32_t w_, int32_t oh, int32_t ow,
                      int32_t cp, int32_t dtype, sp_stream_t stream);
/* F.adaptive_avg_pool2d(Mixed_7c, (1, 1)).view(B, 2048) (frechet_inception_distance.py:38-41): x [n][hw][c] in dtype -> y [n][c] fp32. */
int sp_global_avgpool_f32(const void* x, float* y, int32_t n, int32_t hw, int32_t c, int32_t dtype, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pair-set metrics on two activation sets (metrics.hip; fp32 only, exact fp32 MFMA, the N x M matrix is never stored):
 *   KID                       Binkowski, Sutherland, Arbel, Gretton 2018, "Demystifying MMD GANs", as StyleGAN2-ADA computes it
 *                             (Karras et al. 2020, "Training Generative Adversarial Networks with Limited Data": polynomial kernel
 *                             k(u, v) = (u.v / d + 1)^3 over subsets of m rows)
 *   precision / recall        Kynkaanniemi, Karras, Laine, Lehtinen, Aila 2019, "Improved Precision and Recall Metric for Assessing
 *                             Generative Models": closed balls of radius = distance to the k-th nearest neighbour in the own set
 *   density / coverage        Naeem, Oh, Uh, Choi, Yoo 2020, "Reliable Fidelity and Diversity Metrics for Generative Models"
 * a: [na][lda], b: [nb][ldb] row-major fp32, d columns read; lda, ldb % 4 == 0, both 16-byte aligned; na, nb <= 2^22, d <= 2^20.
 * D(i, j) = max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j) in fp32 - the SQUARED Euclidean distance, no square root anywhere (every
 * comparison is monotone in it); the norms are fp32 sums of squares.  Every output is bit-identical from launch to launch (integer
 * atomics and fixed-order partials only).  Every launching entry point takes `workspace` (8-byte aligned) of at least
 * sp_pairset_workspace() bytes; a failed check returns SP_ERR_INVALID with a message before any launch. */

/* Host logic only (callable without a GPU): the scratch bytes of sp_pairset_knn (k >= 1) / sp_pairset_cover (k = 0) on na x nb rows;
 * sp_pairset_poly3 wants `subsets` times the answer for (m, m, d, 0).
 *   bytes = round8(4 (na + nb)) + max(round8(4 na S k), 8 ceil(na / 128) ceil(nb / 64))
 * S = min(ceil(nb / 64), max(1, ceil(6144 / ceil(na / 128)))) segments of the column blocks, or what SP_TUNE_PAIRSET_SEGMENTS forces
 * (clamped likewise).  k > 16 or k >= nb: SP_ERR_INVALID. */
int sp_pairset_workspace(int32_t na, int32_t nb, int32_t d, int32_t k, int64_t* bytes);
/* radius[i] = the k-th smallest of { D(a_i, b_j) : j } (k = 1: the nearest), 1 <= k <= 16.  same != 0: b IS a (same pointer, na == nb)
 * and j == i is skipped BY INDEX, not by value - a duplicate row is a neighbour at distance 0 (the radii R_i of precision / recall /
 * coverage: Kynkaanniemi et al. 2019 section 3, Naeem et al. 2020 section 3).  k >= nb, or k >= nb - 1 when same: SP_ERR_INVALID. */
int sp_pairset_knn(const float* a, int32_t na, int32_t lda, const float* b, int32_t nb, int32_t ldb, int32_t d, int32_t k,
                   int32_t same, float* radius, void* workspace, int64_t workspace_bytes, sp_stream_t stream);
/* One pass over the tiles of D:
 *   row_count[i] = #{ j : D(i, j) <= rad_b[j] }    col_count[j] = #{ i : D(i, j) <= rad_a[i] }    (closed balls, <=, as both papers write)
 *   row_min[i]   = min_j D(i, j)                   col_min[j]   = min_i D(i, j)
 * With a = fake, b = real and the radii of two sp_pairset_knn launches: precision = mean [row_count > 0],
 * density = sum row_count / (k M), recall = mean [col_count > 0], coverage = mean [col_min <= rad_b].
 * Any output may be NULL; row_count needs rad_b, col_count needs rad_a.  Counts are int32. */
int sp_pairset_cover(const float* a, int32_t na, int32_t lda, const float* b, int32_t nb, int32_t ldb, int32_t d,
                     const float* rad_a, const float* rad_b, int32_t* row_count, int32_t* col_count, float* row_min,
                     float* col_min, void* workspace, int64_t workspace_bytes, sp_stream_t stream);
/* out[z] = the float64 sum over the m x m pairs (p, q) of subset z of t^3, t = (double)(a_i.b_j) / (double)d + 1.0, the cube two
 * float64 multiplications; i = idx_a[z * m + p], j = idx_b[z * m + q] (int32 tables on the device; NULL = the first m rows, one
 * subset only; an index outside [0, src) reads a row of zeros).  skip_diag != 0 leaves out p == q (the positions, not the indices):
 * the S_xx - diag_xx of the unbiased MMD^2 estimate.  a: [src_a][lda], b: [src_b][ldb].  subsets <= 65535. */
int sp_pairset_poly3(const float* a, int32_t src_a, int32_t lda, const int32_t* idx_a, const float* b, int32_t src_b, int32_t ldb,
                     const int32_t* idx_b, int32_t d, int32_t subsets, int32_t m, int32_t skip_diag, double* out,
                     void* workspace, int64_t workspace_bytes, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Inception Score on the same main loop (metrics.hip): Salimans, Goodfellow, Zaremba, Cheung, Radford, Chen 2016,
 * "Improved Techniques for Training GANs", in the split form StyleGAN2-ADA and torch-fidelity compute.  a: [n][lda] rows (the
 * activations), w: [classes][ldw] class rows (the classifier's weight), bias: [classes]; fp32, d columns read; lda, ldw % 4 == 0, a and w
 * 16-byte aligned; n, classes <= 2^22, d <= 2^20.  l_ic = (double)(a_i.w_c in fp32 on the exact fp32 MFMA) + (double)bias_c; everything
 * after that is float64 with exp / log in double.  The n x classes logit matrix is never stored: it is formed once per entry point.
 * Split s of S holds the rows [floor(s n / S), floor((s + 1) n / S)), n_s of them.  A non-finite logit makes its row's lse and h, and
 * its split's kl, NaN (the maximum keeps a NaN); the other splits are untouched.  No float atomics, fixed summation order: every output
 * is bit-identical from launch to launch.  A failed check returns SP_ERR_INVALID with a message before any launch. */

/* Host logic only (callable without a GPU): the scratch bytes that serve both entry points below,
 *   bytes = max(24 n S_c, 8 splits ceil(ceil(n / splits) / 128) classes)
 * S_c = min(ceil(classes / 64), max(1, ceil(6144 / ceil(n / 128)))) segments of the class blocks, or what SP_TUNE_PAIRSET_SEGMENTS
 * forces (clamped likewise): an online-softmax state of three float64 per (row, segment); one float64 per (split, 128-row block of the
 * split, class).  splits outside [1, 65535] or n < splits: SP_ERR_INVALID. */
int sp_pairset_softmax_workspace(int32_t n, int32_t classes, int32_t d, int32_t splits, int64_t* bytes);
/* lse[i] = m_i + log sum_c exp(l_ic - m_i), m_i = max_c l_ic, and h[i] = sum_c p_ic log p_ic, p_ic = exp(l_ic - lse[i]), formed as
 * (sum_c e_ic l_ic) / (sum_c e_ic) - lse[i] from the online merge of (m, sum e, sum e l) over the class blocks.  float64 [n] each.
 * Needs the first term of sp_pairset_softmax_workspace (its answer for any `splits` covers it). */
int sp_pairset_lse(const float* a, int32_t n, int32_t lda, const float* w, int32_t classes, int32_t ldw, const float* bias, int32_t d,
                   double* lse, double* h, void* workspace, int64_t workspace_bytes, sp_stream_t stream);
/* colsum[s][c] = sum_{i in split s} exp(l_ic - lse[i]) (float64 [splits][classes]; every row of it sums to n_s) and
 * kl[s] = (1 / n_s) sum_{i in s} h[i] - sum_c q_sc log q_sc, q_sc = colsum[s][c] / n_s, 0 log 0 = 0 (float64 [splits]); lse and h are
 * sp_pairset_lse's outputs for the same operands.  exp(kl[s]) is the split's score; the Inception Score is their mean. */
int sp_pairset_softmax_colsum(const float* a, int32_t n, int32_t lda, const float* w, int32_t classes, int32_t ldw, const float* bias,
                              int32_t d, const double* lse, const double* h, int32_t splits, double* colsum, double* kl,
                              void* workspace, int64_t workspace_bytes, sp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction fidelity of an image pair (reconstruction.hip): the sufficient statistics of PSNR, SSIM (Wang, Bovik,
 * Sheikh, Simoncelli 2004, "Image Quality Assessment: From Error Visibility to Structural Similarity") and MS-SSIM (Wang, Simoncelli,
 * Bovik 2003, "Multi-scale Structural Similarity for Image Quality Assessment").  The reference has NO counterpart.
 * x, y: images [n][c][h][w_] addressed by the ELEMENT strides of their n, c, h, w axes (any layout, strides >= 0), each with its own
 * dtype SP_F32 / SP_BF16 / SP_F16; a 16-bit value is widened exactly (by bit pattern: the file is compiled once), arithmetic is fp32.
 *   window   g[k] = fp32(exp(-(k - 5)^2 / 4.5) / Z), k = 0..10, Z the float64 sum of the eleven exponentials; 2-D window g (x) g
 *            (11 x 11, sigma 1.5), VALID positions only: (H_j - 10) x (W_j - 10) at scale j, no padding
 *   moments  mx, my, exx, eyy, exy = windowed means of x, y, x^2, y^2, x y (horizontal 11 taps, then vertical 11 taps, fp32 fma);
 *            sxx = exx - mx^2, syy = eyy - my^2, sxy = exy - mx my (population form, no 121 / 120)
 *   maps     C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range:   cs = (2 sxy + C2) / (sxx + syy + C2),
 *            l = (2 mx my + C1) / (mx^2 + my^2 + C1),   ssim = l cs
 *   ssim_mean[n][c][j], cs_mean[n][c][j]   float64 means of the two maps over the valid positions of scale j
 *   next scale   X_{j+1}[p][q] = ((X_j[2p][2q] + X_j[2p][2q+1]) + (X_j[2p+1][2q] + X_j[2p+1][2q+1])) * 0.25 in fp32
 *   sqerr[n][c]  float64 sum over the plane of (double)d * (double)d, d = x - y in fp32 on the widened values
 * scales in [1, 5]; h and w_ divisible by 2^(scales-1) with h >> (scales-1) and w_ >> (scales-1) >= 11 (refused, never padded).
 * A NaN or an infinity in a plane of x or y (or a difference / moment that overflows fp32) makes the outputs of THAT (n, c) NaN and
 * touches no other plane.  One launch per scale (a block owns a 16 x 32 tile of positions of one plane, stages the tile and its
 * 10-pixel halo of both images in LDS, and writes the 2 x 2-pooled pixels it owns for the next scale) and one that adds the blocks'
 * float64 partial sums in index order: no float atomics, every output bit-identical from launch to launch, nothing read outside the
 * planes, no host synchronisation.  Any output pointer may be NULL.
 * Refused with SP_ERR_INVALID and a message before any launch: a NULL x, y or workspace; workspace_bytes below sp_ssim_workspace();
 * a dtype that is no SP_F32 / SP_BF16 / SP_F16; a negative stride; n, c, h, w_ < 1, n * c > 2^24, h or w_ > 32768, more than
 * 2^31 - 1 tiles, scales outside [1, 5] or the divisibility / minimum-size rule; a data_range that is not finite or <= 0.
 *
 * sp_ssim_workspace: host logic only (callable without a GPU).  With P = n c, H_j = h >> j, W_j = w_ >> j and
 * T_j = ceil((H_j - 10) / 16) ceil((W_j - 10) / 32) tiles per plane,
 *   bytes = sum_{j=1}^{scales-1} 2 round8(4 P H_j W_j)  +  8 P (T_0 + 2 sum_{j=0}^{scales-1} T_j)
 * laid out in that order: for j = 1 .. scales-1 the pooled fp32 planes [P][H_j][W_j] of x, then of y; then per scale the float64
 * partial sums [P][T_j] of ssim, then of cs; then [P][T_0] of the squared error.  The workspace must be 8-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int sp_ssim_workspace(int32_t n, int32_t c, int32_t h, int32_t w_, int32_t scales, int64_t* bytes);
int sp_ssim_stats(const void* x, int32_t x_dtype, int64_t xn, int64_t xc, int64_t xh, int64_t xw,
                  const void* y, int32_t y_dtype, int64_t yn, int64_t yc, int64_t yh, int64_t yw,
                  int32_t n, int32_t c, int32_t h, int32_t w_, int32_t scales, double data_range,
                  double* ssim_mean, double* cs_mean, double* sqerr,
                  void* workspace, int64_t workspace_bytes, sp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMPYR_H */
