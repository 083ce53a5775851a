// Pair-set kernels of the sample-quality metrics next to the FID: KID (Binkowski et al. 2018, "Demystifying MMD GANs"),
// improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020).  All of them are functions of the
// N x M matrix of row products of two activation sets; at 50 000 x 50 000 that matrix is 10 GB, so it is never stored: ONE tiled Gram
// main loop on the exact fp32 MFMA (v_mfma_f32_16x16x4_f32: bitwise an fmaf chain along K) with three reducing epilogues.  fp32 only,
// compiled once (as reduce_queue.hip).  The Inception Score (Salimans et al. 2016) rides on the same main loop with two
// more epilogues: its N x classes logit matrix (A = activations, B = the classifier's weight rows) is formed twice and never stored.
//
//   main loop   a block of 256 threads owns 128 rows of A x 64 rows of B; both sets are row-major [n][ld] and are read along K in chunks
//               of 32 (zero-filled past d and past the last row), staged global -> registers -> LDS while the chunk before is multiplied.
//               Its four waves are 2 x 2, each 64 x 32 = 4 x 2 MFMA tiles.  Rows may be gathered through an int32 index table.
//   grid        blockIdx.y = row block, blockIdx.x = segment of the column blocks (knn / cover: the columns are cut into S segments so
//               that row blocks x S fills the chip several times over, SP_TUNE_PAIRSET_SEGMENTS forces S; poly3: one column block each), blockIdx.z = subset.
//   distance    D_ij = max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j) in fp32, the norms from a launch of their own (fp32 sums of squares).
//   knn         the tile of D goes to LDS (over the staging buffers); two threads per row keep the 16 smallest of their half of the columns
//               in registers (branch-free insertion), meet in LDS at the end of the segment and leave k values per (row, segment) in the
//               workspace; a merge launch reads the segments in order.  The k-th smallest of a multiset does not depend on the order.
//   cover       the same tile in LDS; 128 threads scan rows (counts against rad_b, minimum; carried over the segment), 64 scan columns
//               (counts against rad_a, minimum).  They meet in global memory through INTEGER atomics only: atomicAdd on int32 counts and
//               atomicMin on the bit patterns of the non-negative distances, which order as the floats do.  No float atomics.
//   poly3       t = (double)dot / d + 1, t * t * t in float64, summed per lane, per wave (shuffles), per block in a fixed order; one
//               float64 per tile in the workspace, a finalize launch adds the tiles of a subset in tile order.
//   lse         l = (double)dot + (double)bias; the fp32 dots go to LDS, two threads per row fold their 32 columns into the online
//               softmax state (m = max l, s = sum exp(l - m), t = sum exp(l - m) l) in float64, carried over the segment; the halves meet
//               in LDS, one state per (row, segment) goes to the workspace and a merge launch (one thread per row, segments in order)
//               leaves lse = m + log s and h = t / s - lse = sum_c p log p.  The maximum keeps a NaN; a column past the last class is
//               skipped, not entered.
//   colsum      the same tile again, p = exp(l - lse_i) in float64; blockIdx.z = split, whose rows [floor(z n / S), floor((z + 1) n / S))
//               are blocked from the split's first row, so no block straddles two splits.  A lane adds its 16 rows of a column, the
//               four row groups of a wave meet by shuffles, the two waves of a column in LDS: one float64 per (split, row block,
//               column) in the workspace; a finalize launch adds the row blocks in order, a second one forms KL per split.
// Every output is bit-identical from launch to launch.
#include "common.h"

namespace {

constexpr int BM = 128, BN = 64, KC = 32, LDK = KC + 4;      // LDK: 16-byte aligned rows; 36 r mod 64 is a distinct multiple of 4 for r < 16
constexpr int LDD = BN + 1;                                  // pitch of the distance tile: row and column scans both conflict-free
constexpr int SM_STAGE = (BM + BN) * LDK, SM_DIST = BM * LDD;
constexpr int SM_FLOATS = SM_STAGE > SM_DIST ? SM_STAGE : SM_DIST;
constexpr int KMAX = 16;
constexpr int SEG_BLOCKS = 6144;                              // blocks a knn / cover launch aims at: 8 x 768
constexpr unsigned INF_BITS = 0x7f800000u;

enum { EPI_KNN = 0, EPI_COVER = 1, EPI_POLY3 = 2, EPI_LSE = 3, EPI_COLSUM = 4 };

struct PsArgs {
    const float* a; const float* b;
    const int* idx_a; const int* idx_b;      // optional gathers: position p of subset z reads row idx[z * na + p]
    int na, nb;                              // rows of this pass (positions)
    int src_a, src_b;                        // rows of the arrays behind the gathers (a position beyond them reads zeros)
    int d, lda, ldb;
    int cblocks, segs;
    int same, k, skip_diag;
    const float* norm_a; const float* norm_b;
    const float* rad_a; const float* rad_b;
    float* lists;                            // knn: [na][segs][k]
    int* row_count; int* col_count; unsigned* row_min; unsigned* col_min;
    double* partials;                        // poly3: [subsets][row blocks][column blocks]
    const float* bias;                       // lse / colsum: [nb], added to the dot in float64
    double* stats;                           // lse: [na][segs][3] = (m, s, t) per (row, segment)
    const double* lse;                       // colsum: [na]
    int splits;                              // colsum: blockIdx.z = split
    double* colpart;                         // colsum: [splits][gridDim.y][nb]
};

__device__ __forceinline__ float4 load_k4(const float* row, int kg, int d) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row == nullptr || kg >= d) return v;
    if (kg + 4 <= d) return *reinterpret_cast<const float4*>(row + kg);
    v.x = row[kg];                                           // the K tail of a depth that is no multiple of 4
    if (kg + 1 < d) v.y = row[kg + 1];
    if (kg + 2 < d) v.z = row[kg + 2];
    return v;
}

__device__ __forceinline__ void insert16(float (&best)[KMAX], float v) {
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        const float lo = fminf(best[q], v);
        v = fmaxf(best[q], v);
        best[q] = lo;
    }
}

__device__ __forceinline__ float clamp0(float v) { return v > 0.f ? v : 0.f; }

// the larger of two logits; a NaN on either side stays (fmax would drop it)
__device__ __forceinline__ double max_nan(double m, double l) { return (l > m || l != l) ? l : m; }

// online-softmax states (m, s = sum exp(l - m), t = sum exp(l - m) l): the second one joins the first.  (-inf, 0, 0) is the state of
// no column at all and the identity here; a state whose logits are all -inf has s = NaN and is not mistaken for it.
__device__ __forceinline__ void lse_merge(double& m, double& s, double& t, double m2, double s2, double t2) {
    const double ninf = -__builtin_inf();
    if (m2 == ninf && s2 == 0.0) return;
    if (m == ninf && s == 0.0) { m = m2; s = s2; t = t2; return; }
    const double mn = max_nan(m, m2);
    const double fa = exp(m - mn), fb = exp(m2 - mn);
    s = s * fa + s2 * fb;
    t = t * fa + t2 * fb;
    m = mn;
}

template <int EPI>
__global__ __launch_bounds__(256) void pairset_kernel(PsArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[SM_FLOATS];
    __shared__ float s_ra[BM], s_rb[BN];
    __shared__ double s_part[4];
    float* sA = smem;
    float* sB = smem + BM * LDK;
    float* sD = smem;                                        // the distance tile lies over the staging buffers
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    int r0 = blockIdx.y * BM, r_end = g.na;                   // this block's rows: [r0, min(r0 + 128, r_end))
    if constexpr (EPI == EPI_COLSUM) {                       // the rows of split z, blocked from its first row
        r0 += (int)((long)blockIdx.z * g.na / g.splits);
        r_end = (int)((long)(blockIdx.z + 1) * g.na / g.splits);
        if (r0 >= r_end) return;                             // past the split's last row block (the whole block: no barrier is left waiting)
    }
    const int cb0 = (int)((long)blockIdx.x * g.cblocks / g.segs), cb1 = (int)((long)(blockIdx.x + 1) * g.cblocks / g.segs);
    const long zoff_a = (long)blockIdx.z * g.na, zoff_b = (long)blockIdx.z * g.nb;
    const int nchunks = (g.d + KC - 1) / KC;

    // staging: thread t moves the float4 column q of the rows lr, lr + 32, ... of each tile
    const int q4 = (t & 7) * 4, lr = t >> 3;
    const float* pa[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int pos = r0 + lr + 32 * p;
        int row = -1;
        if (pos < r_end) row = g.idx_a != nullptr ? g.idx_a[zoff_a + pos] : pos;
        pa[p] = (row >= 0 && row < g.src_a) ? g.a + (long)row * g.lda : nullptr;
    }

    float best[KMAX];                                        // knn: this thread's half of row (t & 127)
    int row_cnt = 0;                                         // cover: row t < 128
    float row_min = __builtin_inff();
    double psum = 0.0;                                       // poly3
    double lm = -__builtin_inf(), ls = 0.0, lt = 0.0;        // lse: this thread's half of row (t & 127)
    if constexpr (EPI == EPI_KNN) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) best[q] = __builtin_inff();
    }
    if constexpr (EPI == EPI_COVER) {
        if (t < BM) s_ra[t] = (g.rad_a != nullptr && r0 + t < g.na) ? g.rad_a[r0 + t] : -1.f;      // -1: no distance is below it
    }

    for (int cb = cb0; cb < cb1; ++cb) {
        const int c0 = cb * BN;
        const float* pb[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int pos = c0 + lr + 32 * p;
            int row = -1;
            if (pos < g.nb) row = g.idx_b != nullptr ? g.idx_b[zoff_b + pos] : pos;
            pb[p] = (row >= 0 && row < g.src_b) ? g.b + (long)row * g.ldb : nullptr;
        }
        if constexpr (EPI == EPI_COVER) {
            if (t < BN) s_rb[t] = (g.rad_b != nullptr && c0 + t < g.nb) ? g.rad_b[c0 + t] : -1.f;
        }
        if constexpr (EPI == EPI_LSE || EPI == EPI_COLSUM) {
            if (t < BN) s_rb[t] = c0 + t < g.nb ? g.bias[c0 + t] : 0.f;
        }

        f32x4_t acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

        float4 va[4], vb[2];
#pragma unroll
        for (int p = 0; p < 4; ++p) va[p] = load_k4(pa[p], q4, g.d);
#pragma unroll
        for (int p = 0; p < 2; ++p) vb[p] = load_k4(pb[p], q4, g.d);
        for (int kc = 0; kc < nchunks; ++kc) {
#pragma unroll
            for (int p = 0; p < 4; ++p) *reinterpret_cast<float4*>(&sA[(lr + 32 * p) * LDK + q4]) = va[p];
#pragma unroll
            for (int p = 0; p < 2; ++p) *reinterpret_cast<float4*>(&sB[(lr + 32 * p) * LDK + q4]) = vb[p];
            __syncthreads();
            if (kc + 1 < nchunks) {
                const int kg = (kc + 1) * KC + q4;
#pragma unroll
                for (int p = 0; p < 4; ++p) va[p] = load_k4(pa[p], kg, g.d);
#pragma unroll
                for (int p = 0; p < 2; ++p) vb[p] = load_k4(pb[p], kg, g.d);
            }
            const int row = lane & 15, kq = lane >> 4;
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                float fa[4], fb[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = sA[(wm * 64 + i * 16 + row) * LDK + 4 * kk + kq];
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = sB[(wn * 32 + j * 16 + row) * LDK + 4 * kk + kq];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }

        // a lane's accumulators: A rows wm * 64 + i * 16 + (lane >> 4) * 4 + reg, B row wn * 32 + j * 16 + (lane & 15)
        if constexpr (EPI == EPI_POLY3) {
            const double dd = (double)g.d;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ar = r0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                        const int bc = c0 + wn * 32 + j * 16 + (lane & 15);
                        const double tv = (double)acc[i][j][r] / dd + 1.0;
                        const double cube = __dmul_rn(__dmul_rn(tv, tv), tv);          // two roundings: never contracted into the sum
                        if (ar < g.na && bc < g.nb && !(g.skip_diag && ar == bc)) psum += cube;
                    }
        } else if constexpr (EPI == EPI_LSE) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sD[(wm * 64 + i * 16 + (lane >> 4) * 4 + r) * LDD + wn * 32 + j * 16 + (lane & 15)] = acc[i][j][r];
            __syncthreads();
            const int hb = (t >> 7) * 32;
            int nc = g.nb - (c0 + hb);                       // this half's columns that are classes
            nc = nc > 32 ? 32 : nc;
            if (nc > 0) {
                const float* drow = sD + (t & 127) * LDD + hb;
                double mt = -__builtin_inf();
                for (int c = 0; c < nc; ++c) mt = max_nan(mt, (double)drow[c] + (double)s_rb[hb + c]);
                const double mn = max_nan(lm, mt);
                const double fs = exp(lm - mn);              // the first tile: exp(-inf) = 0 on (0, 0)
                ls *= fs;
                lt *= fs;
                lm = mn;
#pragma unroll 4
                for (int c = 0; c < nc; ++c) {
                    const double l = (double)drow[c] + (double)s_rb[hb + c];
                    const double e = exp(l - mn);
                    ls += e;
                    lt += e * l;
                }
            }
            __syncthreads();                                 // the next tile's staging writes go over the tile
        } else if constexpr (EPI == EPI_COLSUM) {
            double cs[2] = {0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ar = r0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                    if (ar < r_end) {
                        const double lse = g.lse[ar];
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            cs[j] += exp(((double)acc[i][j][r] + (double)s_rb[wn * 32 + j * 16 + (lane & 15)]) - lse);
                    }
                }
            double* sC = reinterpret_cast<double*>(smem);    // [2][BN]: free after the main loop's last barrier
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                cs[j] += __shfl_xor(cs[j], 16, 64);          // the four row groups of the wave; a + b == b + a: every lane holds the same bits
                cs[j] += __shfl_xor(cs[j], 32, 64);
                if (lane < 16) sC[wm * BN + wn * 32 + j * 16 + lane] = cs[j];
            }
            __syncthreads();
            if (t < BN && c0 + t < g.nb)
                g.colpart[((long)blockIdx.z * gridDim.y + blockIdx.y) * g.nb + c0 + t] = sC[t] + sC[BN + t];
            __syncthreads();
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int lc = wn * 32 + j * 16 + (lane & 15), bc = c0 + lc;
                const bool c_ok = bc < g.nb;
                const float nbv = c_ok ? g.norm_b[bc] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int la = wm * 64 + i * 16 + (lane >> 4) * 4 + r, ar = r0 + la;
                        float dist = __builtin_inff();
                        if (c_ok && ar < g.na && !(g.same && ar == bc)) dist = clamp0((g.norm_a[ar] + nbv) - 2.f * acc[i][j][r]);
                        sD[la * LDD + lc] = dist;
                    }
            }
            __syncthreads();
            if constexpr (EPI == EPI_KNN) {
                const float* drow = sD + (t & 127) * LDD + (t >> 7) * 32;
#pragma unroll 4
                for (int c = 0; c < 32; ++c) insert16(best, drow[c]);
            } else {
                if (t < BM) {
                    const float* drow = sD + t * LDD;
                    for (int c = 0; c < BN; ++c) {
                        const float v = drow[c];
                        row_cnt += v <= s_rb[c] ? 1 : 0;
                        row_min = fminf(row_min, v);
                    }
                } else if (t < BM + BN) {
                    const int c = t - BM;
                    int cnt = 0;
                    float mn = __builtin_inff();
                    for (int r = 0; r < BM; ++r) {
                        const float v = sD[r * LDD + c];
                        cnt += v <= s_ra[r] ? 1 : 0;
                        mn = fminf(mn, v);
                    }
                    if (c0 + c < g.nb) {
                        if (g.col_count != nullptr && cnt != 0) atomicAdd(&g.col_count[c0 + c], cnt);
                        if (g.col_min != nullptr) atomicMin(&g.col_min[c0 + c], __float_as_uint(mn));
                    }
                }
            }
            __syncthreads();                                 // the next tile's staging writes go over the distance tile
        }
    }

    if constexpr (EPI == EPI_KNN) {
        // the two halves of a row meet: the upper half leaves its list in LDS (free after the barrier above), the lower one takes it in
        float* sL = smem;                                    // [128][KMAX + 1]
        const int r = t & 127;
        if (t >= BM) {
#pragma unroll
            for (int q = 0; q < KMAX; ++q) sL[r * (KMAX + 1) + q] = best[q];
        }
        __syncthreads();
        if (t < BM && r0 + r < g.na) {
#pragma unroll
            for (int q = 0; q < KMAX; ++q) insert16(best, sL[r * (KMAX + 1) + q]);
            float* out = g.lists + ((long)(r0 + r) * g.segs + blockIdx.x) * g.k;
#pragma unroll
            for (int q = 0; q < KMAX; ++q)
                if (q < g.k) out[q] = best[q];
        }
    }
    if constexpr (EPI == EPI_COVER) {
        if (t < BM && r0 + t < g.na && cb1 > cb0) {
            if (g.row_count != nullptr && row_cnt != 0) atomicAdd(&g.row_count[r0 + t], row_cnt);
            if (g.row_min != nullptr) atomicMin(&g.row_min[r0 + t], __float_as_uint(row_min));
        }
    }
    if constexpr (EPI == EPI_LSE) {
        // the two halves of a row meet as in knn, the lower columns first
        double* sS = reinterpret_cast<double*>(smem);        // [128][3]
        const int r = t & 127;
        if (t >= BM) {
            sS[r * 3 + 0] = lm;
            sS[r * 3 + 1] = ls;
            sS[r * 3 + 2] = lt;
        }
        __syncthreads();
        if (t < BM && r0 + r < g.na) {
            lse_merge(lm, ls, lt, sS[r * 3 + 0], sS[r * 3 + 1], sS[r * 3 + 2]);
            double* out = g.stats + ((long)(r0 + r) * g.segs + blockIdx.x) * 3;
            out[0] = lm;
            out[1] = ls;
            out[2] = lt;
        }
    }
    if constexpr (EPI == EPI_POLY3) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) psum += __shfl_xor(psum, o, 64);
        if (lane == 0) s_part[wave] = psum;
        __syncthreads();
        if (t == 0)
            g.partials[((long)blockIdx.z * gridDim.y + blockIdx.y) * g.cblocks + blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
    }
}

// |x_i|^2 as an fp32 sum of squares: one wave per row, lane l takes the elements l, l + 64, ..., then the butterfly
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ x, int n, int d, int ld, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = x + (long)row * ld;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s += p[k] * p[k];
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ lists, int na, int segs, int k, float* __restrict__ radius) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    float best[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) best[q] = __builtin_inff();
    const float* p = lists + (long)i * segs * k;
    for (int e = 0; e < segs * k; ++e) insert16(best, p[e]);
    float r = best[0];
#pragma unroll
    for (int q = 1; q < KMAX; ++q)
        if (q == k - 1) r = best[q];
    radius[i] = r;
}

__global__ __launch_bounds__(256) void cover_init_kernel(int* row_count, int* col_count, unsigned* row_min, unsigned* col_min, int na, int nb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < na) {
        if (row_count != nullptr) row_count[i] = 0;
        if (row_min != nullptr) row_min[i] = INF_BITS;
    }
    if (i < nb) {
        if (col_count != nullptr) col_count[i] = 0;
        if (col_min != nullptr) col_min[i] = INF_BITS;
    }
}

__global__ __launch_bounds__(64) void poly3_finalize_kernel(const double* __restrict__ partials, int subsets, int tiles, double* __restrict__ out) {
    const int z = blockIdx.x * 64 + threadIdx.x;
    if (z >= subsets) return;
    const double* p = partials + (long)z * tiles;
    double s = 0.0;
    for (int e = 0; e < tiles; ++e) s += p[e];
    out[z] = s;
}

__global__ __launch_bounds__(256) void lse_merge_kernel(const double* __restrict__ stats, int n, int segs, double* __restrict__ lse,
                                                        double* __restrict__ h) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* p = stats + (long)i * segs * 3;
    double m = p[0], s = p[1], t = p[2];
    for (int e = 1; e < segs; ++e) lse_merge(m, s, t, p[3 * e], p[3 * e + 1], p[3 * e + 2]);
    const double v = m + log(s);
    lse[i] = v;
    h[i] = t / s - v;                                        // sum_c p_c l_c - lse = sum_c p_c log p_c
}

// colsum[s][c] = the partials of split s in row-block order; only the row blocks that hold rows of the split were written
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const double* __restrict__ part, int n, int splits, int classes, int rbmax,
                                                              double* __restrict__ colsum) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)splits * classes) return;
    const int z = (int)(e / classes), c = (int)(e % classes);
    const int ns = (int)((long)(z + 1) * n / splits) - (int)((long)z * n / splits), rb = (ns + BM - 1) / BM;
    double s = 0.0;
    for (int y = 0; y < rb; ++y) s += part[((long)z * rbmax + y) * classes + c];
    colsum[e] = s;
}

// kl[z] = (1 / n_z) sum_{i in z} h_i - sum_c q log q, q = colsum[z][c] / n_z, 0 log 0 = 0: one block per split, each thread a strided sum,
// the 256 sums added pairwise in a fixed tree
__global__ __launch_bounds__(256) void softmax_kl_kernel(const double* __restrict__ h, const double* __restrict__ colsum, int n, int splits,
                                                         int classes, double* __restrict__ kl) {
    __shared__ double red_h[256], red_q[256];
    const int z = blockIdx.x, t = threadIdx.x;
    const int lo = (int)((long)z * n / splits), hi = (int)((long)(z + 1) * n / splits);
    const double ns = (double)(hi - lo);
    double sh = 0.0, sq = 0.0;
    for (int i = lo + t; i < hi; i += 256) sh += h[i];
    for (int c = t; c < classes; c += 256) {
        const double q = colsum[(long)z * classes + c] / ns;
        sq += q == 0.0 ? 0.0 : q * log(q);                   // a NaN goes through
    }
    red_h[t] = sh;
    red_q[t] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red_h[t] += red_h[t + o];
            red_q[t] += red_q[t + o];
        }
        __syncthreads();
    }
    if (t == 0) kl[z] = red_h[0] / ns - red_q[0];
}

inline long round8(long bytes) { return (bytes + 7) / 8 * 8; }
inline int row_blocks(int na) { return sp_div_up(na, BM); }
inline int col_blocks(int nb) { return sp_div_up(nb, BN); }
// segments of the column blocks.  A block re-stages its A tile for every column block anyway, so short segments lose nothing in the main
// loop; what they buy is an even finish: the chip holds 768 blocks of the knn kernel (3 per CU), and with about eight rounds of
// them the last, partial round is a small part of the launch (measured, profiles/metrics_ab.txt).  Never more than column blocks.
inline int segments(int na, int nb) {
    const int cb = col_blocks(nb);
    int s = sp_tune(SP_TUNE_PAIRSET_SEGMENTS, sp_div_up(SEG_BLOCKS, row_blocks(na)));
    return s < 1 ? 1 : (s > cb ? cb : s);
}
inline long norms_bytes(int na, int nb) { return round8(4L * ((long)na + nb)); }
inline long workspace_need(int na, int nb, int k) {
    const long lists = round8(4L * na * segments(na, nb) * k), tiles = 8L * row_blocks(na) * col_blocks(nb);
    return norms_bytes(na, nb) + (lists > tiles ? lists : tiles);
}

// the Inception Score passes: (m, s, t) per (row, segment) / one float64 per (split, row block of the split, class)
inline int split_row_blocks(int n, int splits) { return row_blocks(sp_div_up(n, splits)); }
inline long lse_stats_bytes(int n, int classes) { return 24L * n * segments(n, classes); }
inline long colsum_part_bytes(int n, int classes, int splits) { return 8L * splits * split_row_blocks(n, splits) * classes; }

int check_sets(const char* who, const void* a, int na, int lda, const void* b, int nb, int ldb, int d) {
    SP_CHECK_ARG(a != nullptr && b != nullptr, "%s: a NULL set", who);
    SP_CHECK_ARG(na >= 1 && nb >= 1 && na <= (1 << 22) && nb <= (1 << 22), "%s: na = %d, nb = %d outside [1, 2^22]", who, na, nb);
    SP_CHECK_ARG(d >= 1 && d <= (1 << 20), "%s: d = %d outside [1, 2^20]", who, d);
    SP_CHECK_ARG(lda >= d && ldb >= d && lda % 4 == 0 && ldb % 4 == 0, "%s: lda = %d, ldb = %d must be multiples of 4 and >= d = %d", who, lda, ldb, d);
    SP_CHECK_ARG(((uintptr_t)a | (uintptr_t)b) % 16 == 0, "%s: the sets must be 16-byte aligned", who);
    return SP_OK;
}

int launch_norms(const float* x, int n, int d, int ld, float* out, hipStream_t s) {
    hipLaunchKernelGGL(row_norms_kernel, dim3(sp_div_up(n, 4)), dim3(256), 0, s, x, n, d, ld, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

}  // namespace

extern "C" int sp_pairset_workspace(int32_t na, int32_t nb, int32_t d, int32_t k, int64_t* bytes) {
    SP_CHECK_ARG(bytes != nullptr, "sp_pairset_workspace: bytes is NULL");
    SP_CHECK_ARG(na >= 1 && nb >= 1 && na <= (1 << 22) && nb <= (1 << 22), "sp_pairset_workspace: na = %d, nb = %d outside [1, 2^22]", na, nb);
    SP_CHECK_ARG(d >= 1 && d <= (1 << 20), "sp_pairset_workspace: d = %d outside [1, 2^20]", d);
    SP_CHECK_ARG(k >= 0 && k <= KMAX, "sp_pairset_workspace: k = %d outside [0, %d]", k, KMAX);
    SP_CHECK_ARG(k < nb, "sp_pairset_workspace: k = %d needs more than %d rows to choose from", k, nb);
    *bytes = workspace_need(na, nb, k);
    return SP_OK;
}

extern "C" int sp_pairset_knn(const float* a, int32_t na, int32_t lda, const float* b, int32_t nb, int32_t ldb, int32_t d, int32_t k,
                              int32_t same, float* radius, void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    if (int rc = check_sets("sp_pairset_knn", a, na, lda, b, nb, ldb, d)) return rc;
    SP_CHECK_ARG(radius != nullptr, "sp_pairset_knn: radius is NULL");
    SP_CHECK_ARG(k >= 1 && k <= KMAX, "sp_pairset_knn: k = %d outside [1, %d]", k, KMAX);
    SP_CHECK_ARG(!same || (na == nb && a == b && lda == ldb), "sp_pairset_knn: same = 1 needs b == a (na = %d, nb = %d)", na, nb);
    SP_CHECK_ARG(k < (same ? nb - 1 : nb), "sp_pairset_knn: k = %d needs more than %d other rows", k, same ? nb - 1 : nb);
    const long need = workspace_need(na, nb, k);
    SP_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0,
                 "sp_pairset_knn: workspace of %ld bytes (8-byte aligned) needed, %ld given", need, (long)workspace_bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* norm_a = reinterpret_cast<float*>(workspace);
    float* norm_b = same ? norm_a : norm_a + na;
    if (int rc = launch_norms(a, na, d, lda, norm_a, s)) return rc;
    if (!same)
        if (int rc = launch_norms(b, nb, d, ldb, norm_b, s)) return rc;
    PsArgs g = {};
    g.a = a; g.b = b; g.na = na; g.nb = nb; g.src_a = na; g.src_b = nb; g.d = d; g.lda = lda; g.ldb = ldb;
    g.cblocks = col_blocks(nb); g.segs = segments(na, nb); g.same = same ? 1 : 0; g.k = k;
    g.norm_a = norm_a; g.norm_b = norm_b;
    g.lists = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + norms_bytes(na, nb));
    hipLaunchKernelGGL(pairset_kernel<EPI_KNN>, dim3(g.segs, row_blocks(na), 1), dim3(256), 0, s, g);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_merge_kernel, dim3(sp_div_up(na, 256)), dim3(256), 0, s, (const float*)g.lists, na, g.segs, k, radius);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_pairset_cover(const float* a, int32_t na, int32_t lda, const float* b, int32_t nb, int32_t ldb, int32_t d,
                                const float* rad_a, const float* rad_b, int32_t* row_count, int32_t* col_count, float* row_min,
                                float* col_min, void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    if (int rc = check_sets("sp_pairset_cover", a, na, lda, b, nb, ldb, d)) return rc;
    SP_CHECK_ARG(row_count != nullptr || col_count != nullptr || row_min != nullptr || col_min != nullptr, "sp_pairset_cover: no output asked for");
    SP_CHECK_ARG((row_count == nullptr || rad_b != nullptr) && (col_count == nullptr || rad_a != nullptr),
                 "sp_pairset_cover: row_count needs rad_b, col_count needs rad_a");
    const long need = workspace_need(na, nb, 0);
    SP_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0,
                 "sp_pairset_cover: workspace of %ld bytes (8-byte aligned) needed, %ld given", need, (long)workspace_bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* norm_a = reinterpret_cast<float*>(workspace);
    float* norm_b = norm_a + na;
    if (int rc = launch_norms(a, na, d, lda, norm_a, s)) return rc;
    if (int rc = launch_norms(b, nb, d, ldb, norm_b, s)) return rc;
    PsArgs g = {};
    g.a = a; g.b = b; g.na = na; g.nb = nb; g.src_a = na; g.src_b = nb; g.d = d; g.lda = lda; g.ldb = ldb;
    g.cblocks = col_blocks(nb); g.segs = segments(na, nb);
    g.norm_a = norm_a; g.norm_b = norm_b; g.rad_a = rad_a; g.rad_b = rad_b;
    g.row_count = row_count; g.col_count = col_count;
    g.row_min = reinterpret_cast<unsigned*>(row_min); g.col_min = reinterpret_cast<unsigned*>(col_min);
    hipLaunchKernelGGL(cover_init_kernel, dim3(sp_div_up(na > nb ? na : nb, 256)), dim3(256), 0, s, g.row_count, g.col_count, g.row_min, g.col_min, na, nb);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pairset_kernel<EPI_COVER>, dim3(g.segs, row_blocks(na), 1), dim3(256), 0, s, g);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_pairset_poly3(const float* a, int32_t src_a, int32_t lda, const int32_t* idx_a, const float* b, int32_t src_b, int32_t ldb,
                                const int32_t* idx_b, int32_t d, int32_t subsets, int32_t m, int32_t skip_diag, double* out,
                                void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    if (int rc = check_sets("sp_pairset_poly3", a, src_a, lda, b, src_b, ldb, d)) return rc;
    SP_CHECK_ARG(out != nullptr, "sp_pairset_poly3: out is NULL");
    SP_CHECK_ARG(subsets >= 1 && subsets <= 65535, "sp_pairset_poly3: subsets = %d outside [1, 65535]", subsets);
    SP_CHECK_ARG(m >= 1 && m <= (1 << 22), "sp_pairset_poly3: m = %d outside [1, 2^22]", m);
    SP_CHECK_ARG(subsets == 1 || (idx_a != nullptr && idx_b != nullptr), "sp_pairset_poly3: more than one subset needs both index tables");
    SP_CHECK_ARG((idx_a != nullptr || m <= src_a) && (idx_b != nullptr || m <= src_b), "sp_pairset_poly3: m = %d rows of %d / %d without an index table", m, src_a, src_b);
    const long tiles = (long)row_blocks(m) * col_blocks(m), need = (long)subsets * workspace_need(m, m, 0);
    SP_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0,
                 "sp_pairset_poly3: workspace of %ld bytes (8-byte aligned; subsets x sp_pairset_workspace(m, m, d, 0)) needed, %ld given", need, (long)workspace_bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PsArgs g = {};
    g.a = a; g.b = b; g.idx_a = idx_a; g.idx_b = idx_b; g.na = m; g.nb = m; g.src_a = src_a; g.src_b = src_b; g.d = d; g.lda = lda; g.ldb = ldb;
    g.cblocks = col_blocks(m); g.segs = g.cblocks; g.skip_diag = skip_diag ? 1 : 0;
    g.partials = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pairset_kernel<EPI_POLY3>, dim3(g.cblocks, row_blocks(m), subsets), dim3(256), 0, s, g);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly3_finalize_kernel, dim3(sp_div_up(subsets, 64)), dim3(64), 0, s, (const double*)g.partials, subsets, (int)tiles, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

namespace {

int check_softmax(const char* who, const float* a, int n, int lda, const float* w, int classes, int ldw, const float* bias, int d) {
    SP_CHECK_ARG(a != nullptr && w != nullptr && bias != nullptr, "%s: a NULL operand (rows, class rows, bias)", who);
    SP_CHECK_ARG(n >= 1 && n <= (1 << 22), "%s: n = %d outside [1, 2^22]", who, n);
    SP_CHECK_ARG(classes >= 1 && classes <= (1 << 22), "%s: classes = %d outside [1, 2^22]", who, classes);
    SP_CHECK_ARG(d >= 1 && d <= (1 << 20), "%s: d = %d outside [1, 2^20]", who, d);
    SP_CHECK_ARG(lda >= d && ldw >= d && lda % 4 == 0 && ldw % 4 == 0, "%s: lda = %d, ldw = %d must be multiples of 4 and >= d = %d", who, lda, ldw, d);
    SP_CHECK_ARG(((uintptr_t)a | (uintptr_t)w) % 16 == 0, "%s: the rows and the class rows must be 16-byte aligned", who);
    return SP_OK;
}

PsArgs softmax_args(const float* a, int n, int lda, const float* w, int classes, int ldw, const float* bias, int d) {
    PsArgs g = {};
    g.a = a; g.b = w; g.na = n; g.nb = classes; g.src_a = n; g.src_b = classes; g.d = d; g.lda = lda; g.ldb = ldw;
    g.cblocks = col_blocks(classes); g.bias = bias;
    return g;
}

}  // namespace

extern "C" int sp_pairset_softmax_workspace(int32_t n, int32_t classes, int32_t d, int32_t splits, int64_t* bytes) {
    SP_CHECK_ARG(bytes != nullptr, "sp_pairset_softmax_workspace: bytes is NULL");
    SP_CHECK_ARG(n >= 1 && n <= (1 << 22), "sp_pairset_softmax_workspace: n = %d outside [1, 2^22]", n);
    SP_CHECK_ARG(classes >= 1 && classes <= (1 << 22), "sp_pairset_softmax_workspace: classes = %d outside [1, 2^22]", classes);
    SP_CHECK_ARG(d >= 1 && d <= (1 << 20), "sp_pairset_softmax_workspace: d = %d outside [1, 2^20]", d);
    SP_CHECK_ARG(splits >= 1 && splits <= 65535, "sp_pairset_softmax_workspace: splits = %d outside [1, 65535]", splits);
    SP_CHECK_ARG(n >= splits, "sp_pairset_softmax_workspace: n = %d rows cannot fill %d splits", n, splits);
    const long stats = lse_stats_bytes(n, classes), part = colsum_part_bytes(n, classes, splits);
    *bytes = stats > part ? stats : part;
    return SP_OK;
}

extern "C" int sp_pairset_lse(const float* a, int32_t n, int32_t lda, const float* w, int32_t classes, int32_t ldw, const float* bias,
                              int32_t d, double* lse, double* h, void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    if (int rc = check_softmax("sp_pairset_lse", a, n, lda, w, classes, ldw, bias, d)) return rc;
    SP_CHECK_ARG(lse != nullptr && h != nullptr, "sp_pairset_lse: lse or h is NULL");
    const long need = lse_stats_bytes(n, classes);
    SP_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0,
                 "sp_pairset_lse: workspace of %ld bytes (8-byte aligned) needed, %ld given", need, (long)workspace_bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PsArgs g = softmax_args(a, n, lda, w, classes, ldw, bias, d);
    g.segs = segments(n, classes);
    g.stats = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pairset_kernel<EPI_LSE>, dim3(g.segs, row_blocks(n), 1), dim3(256), 0, s, g);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(lse_merge_kernel, dim3(sp_div_up(n, 256)), dim3(256), 0, s, (const double*)g.stats, n, g.segs, lse, h);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_pairset_softmax_colsum(const float* a, int32_t n, int32_t lda, const float* w, int32_t classes, int32_t ldw,
                                         const float* bias, int32_t d, const double* lse, const double* h, int32_t splits,
                                         double* colsum, double* kl, void* workspace, int64_t workspace_bytes, sp_stream_t stream) {
    if (int rc = check_softmax("sp_pairset_softmax_colsum", a, n, lda, w, classes, ldw, bias, d)) return rc;
    SP_CHECK_ARG(lse != nullptr && h != nullptr && colsum != nullptr && kl != nullptr, "sp_pairset_softmax_colsum: lse, h, colsum or kl is NULL");
    SP_CHECK_ARG(splits >= 1 && splits <= 65535, "sp_pairset_softmax_colsum: splits = %d outside [1, 65535]", splits);
    SP_CHECK_ARG(n >= splits, "sp_pairset_softmax_colsum: n = %d rows cannot fill %d splits", n, splits);
    const long need = colsum_part_bytes(n, classes, splits);
    SP_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0,
                 "sp_pairset_softmax_colsum: workspace of %ld bytes (8-byte aligned) needed, %ld given", need, (long)workspace_bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PsArgs g = softmax_args(a, n, lda, w, classes, ldw, bias, d);
    g.segs = g.cblocks;                                      // one column block per block, as poly3
    g.lse = lse; g.splits = splits;
    g.colpart = reinterpret_cast<double*>(workspace);
    const int rbmax = split_row_blocks(n, splits);
    hipLaunchKernelGGL(pairset_kernel<EPI_COLSUM>, dim3(g.cblocks, rbmax, splits), dim3(256), 0, s, g);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(sp_div_up((long)splits * classes, 256)), dim3(256), 0, s, (const double*)g.colpart, n,
                       splits, classes, rbmax, colsum);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_kl_kernel, dim3(splits), dim3(256), 0, s, h, (const double*)colsum, n, splits, classes, kl);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
