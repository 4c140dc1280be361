// mse_search.hip — fused LAPQ-style MSE range search for quantiser INITIALISATION (calibration).
//
// UniformAffineQuantizer.init_quantization_scale with scale_method = 'mse' (reference qdiff/quant_layer.py:138-140, 162-177,
// quantize() :183-190) tries 80 shrink factors of [x_min, x_max]; for each it quantises the whole tensor and scores the
// L_2.4 error: ~14 elementwise / reduction launches per factor over the tensor, ~1100 launches per quantiser.  Here the
// tensor is read twice (min / max, then scores) and the 80 scores are accumulated side by side.
// A GROUP is what one search covers: a row (per_row = 1: channel-wise weights) or all rows together (per_row = 0: an
// activation tensor, or a channel slice of one read in place as B strided rows).  Per group, operation by operation
// (FP contraction off, IEEE division), as ATen evaluates the composition ON THE DEVICE:
//     hi = x_max * f_i;  lo = x_min * f_i;  span = always_zero ? hi : hi - lo
//     d  = span * (1.0f / levels)           ATen divides a device tensor by a host scalar as a product with its reciprocal
//     z  = always_zero ? 0 : rint(-lo / d)
//     per element:  v = rint(x / d) + z;  c = v is NaN ? v : min(max(v, 0), qmax);  xq = (c - z) * d;  term = |x - xq|^2.4
//     score_i = (float)(sum of the terms / element count): each lane adds the at most 8 terms of one chunk in fp32, every
//               further addition is fp64 in a fixed order (wave butterfly, waves in order, blocks in order); one rounding
//     selection: best = 1e10f; ascending i; taken only when score_i < best.  Nothing taken: index = -1, delta = zero_point = 0.
// NaN propagates as in ATen: min / max of a group that holds a NaN are NaN, clamp keeps a NaN, a NaN score is never better.
// The power is the device library's powf (the composition's own): a log2 / exp2 form loses ~2.4 * |log2 t| ulp per term,
// past the bound of 2 x the composition's score error that the tests hold this kernel to.
//
// Launch forms (qd_mse_search_form is the one rule):
//   row form     per_row = 1.  One block per row does min / max, candidates, scores and selection in one launch; the row is
//                read again for the scores, chunk by chunk.  cols <= 512: a block is one wave (QD_MSE_FORM_WAVE), else four.
//   spread form  per_row = 0.  (1) min / max partials per block, (2) every block reduces those partials (same order in every
//                block), scores its chunks and leaves [block][80] fp64 partial sums, (3) one block adds them in block order
//                and selects.  At most 2048 blocks; a block strides over chunks.
// The candidates' (d, z) are wave-uniform: LDS, read as broadcasts.  No floating-point atomics: two runs agree bit for bit.
// A lane's four elements are one 16-byte load when they lie in one row at an aligned address, else four 4-byte loads.
#include "common.h"

namespace {

constexpr int MS_NC = 80;                 // candidates at most
constexpr int MS_MAX_BLOCKS = 2048;       // spread form
constexpr int MS_WAVE_COLS = 512;         // row form: longest row a single wave takes

struct MsParams {
    const float* x;
    long ldx;
    int rows, cols;
    long n;                               // rows * cols (< 2^31)
    const float* factors;
    int n_cand;
    float levels, qmax;
    int always_zero;
    float *delta, *zp, *x_min, *x_max;
    int* index;
    float* scores;
};

// Four consecutive elements of the dense index space [0, n) of a row-strided tensor starting at i0 (i0 % 4 == 0): element i
// lives at base + (i / cols) * ld + i % cols.  Returns the mask of the elements that exist (i < n); the others read as 0.
__device__ __forceinline__ unsigned ms_load4(const float* __restrict__ base, long ld, int cols, long n, long i0, float (&v)[4]) {
    if (i0 >= n) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 0.f;
        return 0u;
    }
    const int r = (int)(i0 / cols), c = (int)(i0 - (long)r * cols);
    const float* src = base + (long)r * ld + c;
    if (i0 + 4 <= n && c + 4 <= cols) {
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[j];
        }
        return 15u;
    }
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j;
        v[j] = 0.f;
        if (i < n) {
            const int rj = (int)(i / cols);
            v[j] = base[(long)rj * ld + (int)(i - (long)rj * cols)];
            m |= 1u << j;
        }
    }
    return m;
}

struct MsRange {
    float mn, mx;
    bool nan;
};

__device__ __forceinline__ void ms_range_add(MsRange& a, float v, bool valid) {
    a.nan |= valid && (v != v);
    a.mn = (valid && v < a.mn) ? v : a.mn;
    a.mx = (valid && v > a.mx) ? v : a.mx;
}

// min / max / NaN flag of a block of THREADS; every thread receives the result.  ATen's rule: a NaN makes both NaN.
template <int THREADS>
__device__ __forceinline__ void ms_range_block(MsRange a, float& x_min, float& x_max) {
    constexpr int WAVES = THREADS / 64;
    __shared__ float smn[WAVES], smx[WAVES];
    __shared__ int snan[WAVES];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float omn = __shfl_xor(a.mn, o), omx = __shfl_xor(a.mx, o);
        a.mn = omn < a.mn ? omn : a.mn;
        a.mx = omx > a.mx ? omx : a.mx;
    }
    const bool wnan = __any(a.nan);
    __syncthreads();                                    // the arrays may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = a.mn, smx[threadIdx.x >> 6] = a.mx, snan[threadIdx.x >> 6] = wnan;
    __syncthreads();
    float mn = smn[0], mx = smx[0];
    bool nan = snan[0] != 0;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        mn = smn[w] < mn ? smn[w] : mn;
        mx = smx[w] > mx ? smx[w] : mx;
        nan |= snan[w] != 0;
    }
    x_min = nan ? __builtin_nanf("") : mn;
    x_max = nan ? __builtin_nanf("") : mx;
}

__device__ __forceinline__ float2 ms_candidate(float x_min, float x_max, float f, float levels, int always_zero) {
#pragma clang fp contract(off)
    const float hi = x_max * f, lo = x_min * f;
    const float rl = 1.0f / levels;
    const float d = (always_zero ? hi : hi - lo) * rl;
    const float z = always_zero ? 0.f : rintf(-lo / d);
    return make_float2(d, z);
}

__device__ __forceinline__ float ms_term(float x, float d, float z, float qmax) {
#pragma clang fp contract(off)
    const float v = rintf(x / d) + z;
    const float t = fminf(fmaxf(v, 0.f), qmax);
    const float c = (v != v) ? v : t;                   // ATen's clamp keeps a NaN; fminf / fmaxf would drop it
    const float xq = (c - z) * d;
    return powf(fabsf(x - xq), 2.4f);
}

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The n_cand scores of one chunk (two quads per lane; `valid` = bit per element) added to the wave's running sums: lane l
// keeps candidate l in acc0 and candidate 64 + l in acc1.
__device__ __forceinline__ void ms_score_chunk(const float (&xv)[8], unsigned valid, const float2* cand, int n_cand, float qmax,
                                               double& acc0, double& acc1) {
    const bool q0 = __any((valid & 15u) != 0), q1 = __any((valid >> 4) != 0);      // wave-uniform
    if (!q0 && !q1) return;
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int c = 0; c < n_cand; ++c) {
        const float2 dz = cand[c];
        float s = 0.f;
        if (q0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = ms_term(xv[j], dz.x, dz.y, qmax);
                s += ((valid >> j) & 1u) ? t : 0.f;
            }
        }
        if (q1) {
#pragma unroll
            for (int j = 4; j < 8; ++j) {
                const float t = ms_term(xv[j], dz.x, dz.y, qmax);
                s += ((valid >> j) & 1u) ? t : 0.f;
            }
        }
        const double t = ms_wave_sum((double)s);
        if (lane == (c & 63)) {
            if (c < 64) acc0 += t;
            else acc1 += t;
        }
    }
}

// The sums of a block's waves, in wave order: thread c (c < n_cand, strided) receives candidate c's through `f`.
template <int THREADS, typename F>
__device__ __forceinline__ void ms_block_sums(double acc0, double acc1, int n_cand, F f) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double wsum[WAVES][MS_NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wsum[wave][lane] = acc0;
    if (lane < MS_NC - 64) wsum[wave][64 + lane] = acc1;
    __syncthreads();
    for (int c = threadIdx.x; c < n_cand; c += THREADS) {
        double s = wsum[0][c];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += wsum[w][c];
        f(c, s);
    }
}

// one thread: the composition's selection over the scores in LDS, and the group's outputs
__device__ __forceinline__ void ms_select(const MsParams& p, int g, const float* sc, const float2* cand, float x_min, float x_max) {
    float best = 1e10f;
    int idx = -1;
    for (int c = 0; c < p.n_cand; ++c)
        if (sc[c] < best) best = sc[c], idx = c;
    p.delta[g] = idx >= 0 ? cand[idx].x : 0.f;
    p.zp[g] = idx >= 0 ? cand[idx].y : 0.f;
    p.index[g] = idx;
    p.x_min[g] = x_min, p.x_max[g] = x_max;
}

// ---- row form ----------------------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void mse_search_row_kernel(MsParams p) {
    __shared__ float2 cand[MS_NC];
    __shared__ float sc[MS_NC];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = p.x + (long)r * p.ldx;
    const long cols = p.cols;
    constexpr int SPAN = THREADS * 8;

    MsRange a{__builtin_inff(), -__builtin_inff(), false};
    for (long base = 0; base < cols; base += THREADS * 4) {
        float v[4];
        const unsigned m = ms_load4(row, cols, p.cols, cols, base + tid * 4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) ms_range_add(a, v[j], (m >> j) & 1u);
    }
    float x_min, x_max;
    ms_range_block<THREADS>(a, x_min, x_max);
    for (int c = tid; c < p.n_cand; c += THREADS) cand[c] = ms_candidate(x_min, x_max, p.factors[c], p.levels, p.always_zero);
    __syncthreads();

    double acc0 = 0., acc1 = 0.;
    for (long base = 0; base < cols; base += SPAN) {
        float xv[8], lo[4], hi[4];
        const unsigned m0 = ms_load4(row, cols, p.cols, cols, base + tid * 4, lo);
        const unsigned m1 = ms_load4(row, cols, p.cols, cols, base + THREADS * 4 + tid * 4, hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = lo[j], xv[4 + j] = hi[j];
        ms_score_chunk(xv, m0 | (m1 << 4), cand, p.n_cand, p.qmax, acc0, acc1);
    }
    ms_block_sums<THREADS>(acc0, acc1, p.n_cand, [&](int c, double s) {
        const float v = (float)(s / (double)cols);
        sc[c] = v;
        if (p.scores) p.scores[(long)r * p.n_cand + c] = v;
    });
    __syncthreads();
    if (tid == 0) ms_select(p, r, sc, cand, x_min, x_max);
}

// ---- spread form -------------------------------------------------------------------------------------------------------
constexpr int MS_T = 256, MS_SPAN = MS_T * 8;

__global__ __launch_bounds__(MS_T) void mse_search_minmax_kernel(MsParams p, float* __restrict__ part) {
    const int tid = threadIdx.x;
    MsRange a{__builtin_inff(), -__builtin_inff(), false};
    for (long base = (long)blockIdx.x * MS_SPAN; base < p.n; base += (long)gridDim.x * MS_SPAN) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float v[4];
            const unsigned m = ms_load4(p.x, p.ldx, p.cols, p.n, base + q * (MS_T * 4) + tid * 4, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) ms_range_add(a, v[j], (m >> j) & 1u);
        }
    }
    float x_min, x_max;
    ms_range_block<MS_T>(a, x_min, x_max);
    if (tid == 0) part[2 * blockIdx.x] = x_min, part[2 * blockIdx.x + 1] = x_max;
}

// min / max of the block partials (a NaN partial = that block saw a NaN), the same in every block that calls it
__device__ __forceinline__ void ms_range_of_partials(const float* __restrict__ part, int nblk, float& x_min, float& x_max) {
    MsRange a{__builtin_inff(), -__builtin_inff(), false};
    for (int b = threadIdx.x; b < nblk; b += MS_T) {
        ms_range_add(a, part[2 * b], true);
        ms_range_add(a, part[2 * b + 1], true);
    }
    ms_range_block<MS_T>(a, x_min, x_max);
}

__global__ __launch_bounds__(MS_T) void mse_search_score_kernel(MsParams p, const float* __restrict__ part, double* __restrict__ sums) {
    __shared__ float2 cand[MS_NC];
    const int tid = threadIdx.x;
    float x_min, x_max;
    ms_range_of_partials(part, gridDim.x, x_min, x_max);
    for (int c = tid; c < p.n_cand; c += MS_T) cand[c] = ms_candidate(x_min, x_max, p.factors[c], p.levels, p.always_zero);
    __syncthreads();
    double acc0 = 0., acc1 = 0.;
    for (long base = (long)blockIdx.x * MS_SPAN; base < p.n; base += (long)gridDim.x * MS_SPAN) {
        float xv[8], lo[4], hi[4];
        const unsigned m0 = ms_load4(p.x, p.ldx, p.cols, p.n, base + tid * 4, lo);
        const unsigned m1 = ms_load4(p.x, p.ldx, p.cols, p.n, base + MS_T * 4 + tid * 4, hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = lo[j], xv[4 + j] = hi[j];
        ms_score_chunk(xv, m0 | (m1 << 4), cand, p.n_cand, p.qmax, acc0, acc1);
    }
    ms_block_sums<MS_T>(acc0, acc1, p.n_cand, [&](int c, double s) { sums[(long)blockIdx.x * MS_NC + c] = s; });
}

__global__ __launch_bounds__(MS_T) void mse_search_finalise_kernel(MsParams p, const float* __restrict__ part,
                                                                   const double* __restrict__ sums, int nblk) {
    __shared__ float2 cand[MS_NC];
    __shared__ float sc[MS_NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float x_min, x_max;
    ms_range_of_partials(part, nblk, x_min, x_max);
    for (int c = tid; c < p.n_cand; c += MS_T) cand[c] = ms_candidate(x_min, x_max, p.factors[c], p.levels, p.always_zero);
    for (int c = wave; c < p.n_cand; c += MS_T / 64) {          // lane l adds blocks l, l + 64, ... in order; then the butterfly
        double s = 0.;
        for (int b = lane; b < nblk; b += 64) s += sums[(long)b * MS_NC + c];
        s = ms_wave_sum(s);
        if (lane == 0) {
            const float v = (float)(s / (double)p.n);
            sc[c] = v;
            if (p.scores) p.scores[c] = v;
        }
    }
    __syncthreads();
    if (tid == 0) ms_select(p, 0, sc, cand, x_min, x_max);
}

int ms_spread_blocks(int64_t n) {
    const int64_t chunks = (n + MS_SPAN - 1) / MS_SPAN;
    return (int)(chunks < MS_MAX_BLOCKS ? chunks : MS_MAX_BLOCKS);
}

int64_t ms_part_bytes(int nblk) { return ((int64_t)nblk * 2 * sizeof(float) + 15) / 16 * 16; }

}  // namespace

extern "C" int qd_mse_search_form(int64_t rows, int64_t cols, int per_row) {
    if (rows <= 0 || cols <= 0) return -1;
    if (!per_row) return QD_MSE_FORM_SPREAD;
    return cols <= MS_WAVE_COLS ? QD_MSE_FORM_WAVE : QD_MSE_FORM_BLOCK;
}

extern "C" int64_t qd_mse_search_ws_bytes(int64_t rows, int64_t cols, int per_row, int n_cand) {
    if (qd_mse_search_form(rows, cols, per_row) != QD_MSE_FORM_SPREAD || n_cand < 1 || n_cand > MS_NC) return 0;
    const int nblk = ms_spread_blocks(rows * cols);
    return ms_part_bytes(nblk) + (int64_t)nblk * MS_NC * sizeof(double);
}

extern "C" int qd_mse_search(const float* x, int64_t rows, int64_t cols, int64_t ldx, int per_row, const float* factors, int n_cand,
                             int levels, int qmax, int always_zero, float* delta, float* zero_point, float* x_min, float* x_max,
                             int32_t* index, float* scores, void* ws, void* stream) {
    QD_REQUIRE(x && factors && delta && zero_point && x_min && x_max && index, "qd_mse_search: null pointer");
    QD_REQUIRE(rows > 0 && cols > 0, "qd_mse_search: empty tensor (rows = %ld, cols = %ld)", (long)rows, (long)cols);
    QD_REQUIRE(n_cand >= 1 && n_cand <= MS_NC, "qd_mse_search: n_cand must be in 1..%d (got %d)", MS_NC, n_cand);
    QD_REQUIRE(rows < (1L << 31) && cols < (1L << 31) && rows * cols < (1L << 31),
               "qd_mse_search: %ld x %ld elements do not fit the 31-bit index", (long)rows, (long)cols);
    QD_REQUIRE(rows == 1 || ldx >= cols, "qd_mse_search: row stride %ld shorter than a row of %ld", (long)ldx, (long)cols);
    QD_REQUIRE(levels >= 1 && qmax >= 0, "qd_mse_search: levels must be at least 1 and qmax at least 0 (got %d, %d)", levels, qmax);
    QD_REQUIRE(qd_aligned(x, 4), "qd_mse_search: x must be 4-byte aligned");
    const int form = qd_mse_search_form(rows, cols, per_row);
    QD_REQUIRE(form != QD_MSE_FORM_SPREAD || (ws && qd_aligned(ws, 16)),
               "qd_mse_search: the spread form needs a 16-byte aligned workspace of qd_mse_search_ws_bytes");
    MsParams p;
    p.x = x, p.ldx = rows == 1 ? (long)cols : (long)ldx, p.rows = (int)rows, p.cols = (int)cols, p.n = (long)(rows * cols);
    p.factors = factors, p.n_cand = n_cand, p.levels = (float)levels, p.qmax = (float)qmax, p.always_zero = always_zero ? 1 : 0;
    p.delta = delta, p.zp = zero_point, p.x_min = x_min, p.x_max = x_max, p.index = index, p.scores = scores;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (form == QD_MSE_FORM_WAVE) {
        hipLaunchKernelGGL(mse_search_row_kernel<64>, dim3((unsigned)rows), dim3(64), 0, s, p);
    } else if (form == QD_MSE_FORM_BLOCK) {
        hipLaunchKernelGGL(mse_search_row_kernel<256>, dim3((unsigned)rows), dim3(256), 0, s, p);
    } else {
        const int nblk = ms_spread_blocks(p.n);
        float* part = reinterpret_cast<float*>(ws);
        double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ms_part_bytes(nblk));
        hipLaunchKernelGGL(mse_search_minmax_kernel, dim3(nblk), dim3(MS_T), 0, s, p, part);
        hipLaunchKernelGGL(mse_search_score_kernel, dim3(nblk), dim3(MS_T), 0, s, p, (const float*)part, sums);
        hipLaunchKernelGGL(mse_search_finalise_kernel, dim3(1), dim3(MS_T), 0, s, p, (const float*)part, (const double*)sums, nblk);
    }
    QD_LAUNCH_CHECK("qd_mse_search");
    return 0;
}
