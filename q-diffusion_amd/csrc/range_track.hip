// range_track.hip — fused EMA range tracking and no-grad fake-quantisation of an activation tensor (calibration).
//
// UniformAffineQuantizer.forward with running_stat set (reference qdiff/quant_layer.py:77-78 -> act_momentum_update :91-110, then
// the simulation :82-88; the README's `--running_stat --rs_sm_only` commands drive it from scripts/txt2img.py:457-468) runs two
// whole-tensor reductions, a chain of scalar launches and six elementwise launches per quantiser and forward: ~56 B moved per
// element.  Here: two launches, 12 B per element (read; read and write).
//   (1) range_partials_kernel   grid-stride over 2048-element chunks of the dense index space; a lane keeps min / max / NaN flag;
//                               wave butterfly in registers, the four waves through LDS; ONE {min, max, nan} record per block.
//   (2) apply_kernel<TRACK>     every block reduces ALL records (at most RT_MAX_BLOCKS x 16 B, L2-resident) in the same order, so
//                               every block derives the same state; block 0 alone writes it to state_out.  The old range comes
//                               from range_in, which no launch writes: nothing races.  Then the block quantises its chunks of x
//                               into the dense y.  TRACK = false is the plain form: (delta, zero_point) are device scalars.
// No atomics, no tickets, no block waits on another: nothing can hang, and two runs agree bit for bit.
// State, operation by operation in fp32 (FP contraction off, IEEE division), as ATen evaluates the composition ON THE DEVICE — it
// divides a tensor by a host scalar as a product with the scalar's fp32 reciprocal (rlev below; see mse_search.hip):
//     mn' = x_min * m + min(x) * om             mx' = x_max * m + max(x) * om            m = float32(0.95), om = float32(1 - 0.95)
//     symmetric:    delta = max(|mn'|, |mx'|) * (1.0f / n_levels)                        (a NaN on either side is kept)
//     always_zero:  delta = mx' * (1.0f / (n_levels - 1))
//     affine:       delta = (mx' - mn') * (1.0f / (n_levels - 1))
//     delta = max(delta, 1e-8f), a NaN stays;   zp = rint(-mn' / delta) affine, 0 always_zero, zero_point_in[0] symmetric
//     y = (clamp(rint(x / delta) + zp, qmin, qmax) - zp) * delta, the clamp keeping a NaN     (qd_fakequant_one<true>, common.h)
// A NaN anywhere in x makes min(x) and max(x) NaN, as in ATen.  Which of +0 / -0 wins a min / max tie is not pinned.
// Geometry: `rows` rows of `cols` consecutive floats, row r at x + r * ldx; counts and indices are 64-bit (the 16·8 x 4096 x 4096
// self-attention map of SD holds exactly 2^31 elements).  A quad of the DENSE index space (i % 4 == 0, so its four y are one
// 16-byte store) is one 16-byte load when it lies inside one row at a 16-byte address — within a row that is the same answer
// for every quad, so it is decided per row — else four 4-byte loads, each located in its own row: bytes in the gaps between
// strided rows are never read.  A chunk's (row, column) is one uniform 64-bit division per block and chunk, not per lane.
#include "common.h"

namespace {

constexpr int RT_T = 256;                     // threads per block
constexpr int RT_CHUNK = RT_T * 8;            // elements a block takes per sweep: two quads per lane
constexpr int RT_MAX_BLOCKS = 2048;           // 256 CUs x 8 blocks of four waves = 8 waves per SIMD: every CU full

struct RtParams {
    const float* x;
    long rows, cols, ldx, n;                  // n = rows * cols
    float m, om, rlev, lo, hi;
    int mode;
    const float *range_in, *zp_in;            // tracked form: {x_min, x_max} before the call; symmetric zero point
    float* state_out;                         // tracked form: {x_min, x_max, delta, zero_point}
    const float *delta, *zp;                  // plain form
    float* y;
};

struct RtRange {
    float mn, mx;
    bool nan;
};

__device__ __forceinline__ void rt_range_add(RtRange& a, float v, bool valid) {
    a.nan |= valid && (v != v);
    a.mn = (valid && v < a.mn) ? v : a.mn;
    a.mx = (valid && v > a.mx) ? v : a.mx;
}

// the range of the block's 256 lanes, in every thread: butterfly over the wave in registers, the four waves through LDS
__device__ __forceinline__ RtRange rt_block_range(RtRange a) {
    __shared__ float smn[RT_T / 64], smx[RT_T / 64];
    __shared__ int snan[RT_T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float omn = __shfl_xor(a.mn, o), omx = __shfl_xor(a.mx, o);
        a.mn = omn < a.mn ? omn : a.mn;
        a.mx = omx > a.mx ? omx : a.mx;
    }
    const bool wnan = __any(a.nan);
    if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = a.mn, smx[threadIdx.x >> 6] = a.mx, snan[threadIdx.x >> 6] = wnan;
    __syncthreads();
    RtRange r{smn[0], smx[0], snan[0] != 0};
#pragma unroll
    for (int w = 1; w < RT_T / 64; ++w) {
        r.mn = smn[w] < r.mn ? smn[w] : r.mn;
        r.mx = smx[w] > r.mx ? smx[w] : r.mx;
        r.nan |= snan[w] != 0;
    }
    return r;
}

// (row, column) of the chunk that starts at dense index `base`: uniform over the block
__device__ __forceinline__ void rt_chunk_origin(const RtParams& p, long base, long& r0, long& c0) {
    r0 = p.rows == 1 ? 0 : base / p.cols;
    c0 = base - r0 * p.cols;
}

// (row, column) of the element `o` (< RT_CHUNK) past a chunk origin with c0 < cols
__device__ __forceinline__ void rt_locate(const RtParams& p, long r0, long c0, int o, long& r, long& c) {
    r = r0, c = c0 + o;
    if (p.cols >= RT_CHUNK) {                 // at most one row boundary inside a chunk
        if (c >= p.cols) c -= p.cols, ++r;
    } else {                                  // c < 2 * RT_CHUNK: a 32-bit division
        const int k = (int)c / (int)p.cols;
        r += k, c -= (long)k * p.cols;
    }
}

// The quad of the dense index space at (r, c), r < rows, c < cols.  Returns the mask of the elements that exist; the others
// read as 0.  Only addresses x + rj * ldx + cj with rj < rows, cj < cols are formed.
__device__ __forceinline__ unsigned rt_load4(const RtParams& p, long r, long c, float (&v)[4]) {
    const float* src = p.x + r * p.ldx + c;
    if (c + 4 <= p.cols) {
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[j];
        }
        return 15u;
    }
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long rj = r, cj = c + j;              // c < cols and j <= 3: at most three rows further
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (cj >= p.cols) cj -= p.cols, ++rj;
        v[j] = 0.f;
        if (rj < p.rows) {
            v[j] = p.x[rj * p.ldx + cj];
            mask |= 1u << j;
        }
    }
    return mask;
}

__global__ __launch_bounds__(RT_T) void range_partials_kernel(RtParams p, float4* __restrict__ part) {
    const int tid = threadIdx.x;
    RtRange a{__builtin_inff(), -__builtin_inff(), false};
    for (long base = (long)blockIdx.x * RT_CHUNK; base < p.n; base += (long)gridDim.x * RT_CHUNK) {
        long r0, c0;
        rt_chunk_origin(p, base, r0, c0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o = q * (RT_T * 4) + tid * 4;
            if (base + o >= p.n) continue;
            long r, c;
            rt_locate(p, r0, c0, o, r, c);
            float v[4];
            const unsigned mask = rt_load4(p, r, c, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) rt_range_add(a, v[j], (mask >> j) & 1u);
        }
    }
    a = rt_block_range(a);
    if (tid == 0) part[blockIdx.x] = make_float4(a.mn, a.mx, a.nan ? 1.f : 0.f, 0.f);
}

struct RtState {
    float mn, mx, delta, zp;
};

// the composition's scalar chain (act_momentum_update) on the tensor's range; xmin / xmax are NaN when x holds one
__device__ __forceinline__ RtState rt_state(const RtParams& p, float xmin, float xmax) {
#pragma clang fp contract(off)
    RtState s;
    s.mn = p.range_in[0] * p.m + xmin * p.om;
    s.mx = p.range_in[1] * p.m + xmax * p.om;
    float span;
    if (p.mode == QD_RANGE_SYMMETRIC) {
        const float a = fabsf(s.mn), b = fabsf(s.mx);
        span = (a != a || b != b) ? a + b : fmaxf(a, b);            // torch.max keeps a NaN; fmaxf would drop it
    } else {
        span = p.mode == QD_RANGE_ALWAYS_ZERO ? s.mx : s.mx - s.mn;
    }
    const float d = span * p.rlev;
    s.delta = d < 1e-8f ? 1e-8f : d;                                // torch.clamp(min=1e-8): a NaN stays
    s.zp = p.mode == QD_RANGE_AFFINE ? rintf(-s.mn / s.delta) : p.mode == QD_RANGE_ALWAYS_ZERO ? 0.f : p.zp_in[0];
    return s;
}

template <bool TRACK>
__global__ __launch_bounds__(RT_T) void apply_kernel(RtParams p, const float4* __restrict__ part, int npart) {
    const int tid = threadIdx.x;
    float d, zp;
    if constexpr (TRACK) {
        RtRange a{__builtin_inff(), -__builtin_inff(), false};
        for (int b = tid; b < npart; b += RT_T) {
            const float4 t = part[b];
            a.mn = t.x < a.mn ? t.x : a.mn;
            a.mx = t.y > a.mx ? t.y : a.mx;
            a.nan |= t.z != 0.f;
        }
        a = rt_block_range(a);
        const float nanv = __builtin_nanf("");
        const RtState s = rt_state(p, a.nan ? nanv : a.mn, a.nan ? nanv : a.mx);
        if (blockIdx.x == 0 && tid == 0) p.state_out[0] = s.mn, p.state_out[1] = s.mx, p.state_out[2] = s.delta, p.state_out[3] = s.zp;
        if (!p.y) return;                                           // the state alone (the integer path quantises by itself)
        d = s.delta, zp = s.zp;
    } else {
        d = p.delta[0], zp = p.zp[0];
    }
    for (long base = (long)blockIdx.x * RT_CHUNK; base < p.n; base += (long)gridDim.x * RT_CHUNK) {
        long r0, c0;
        rt_chunk_origin(p, base, r0, c0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o = q * (RT_T * 4) + tid * 4;
            const long i = base + o;
            if (i >= p.n) continue;
            long r, c;
            rt_locate(p, r0, c0, o, r, c);
            float v[4];
            const unsigned mask = rt_load4(p, r, c, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = qd_fakequant_one<true>(v[j], d, zp, p.lo, p.hi);
            if (mask == 15u) {
                *reinterpret_cast<float4*>(p.y + i) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((mask >> j) & 1u) p.y[i + j] = v[j];
            }
        }
    }
}

int rt_blocks(int64_t n) {
    const int64_t chunks = (n + RT_CHUNK - 1) / RT_CHUNK;
    return (int)(chunks < RT_MAX_BLOCKS ? chunks : RT_MAX_BLOCKS);
}

// the argument checks the two entries share; fills the geometry
int rt_geometry(const char* who, const float* x, int64_t rows, int64_t cols, int64_t ldx, int qmin, int qmax, const float* y,
                RtParams& p) {
    QD_REQUIRE(x, "%s: null pointer (x)", who);
    QD_REQUIRE(rows > 0 && cols > 0, "%s: empty tensor (rows = %ld, cols = %ld)", who, (long)rows, (long)cols);
    QD_REQUIRE(rows <= INT64_MAX / cols, "%s: %ld x %ld elements do not fit the 64-bit index", who, (long)rows, (long)cols);
    QD_REQUIRE(rows == 1 || ldx >= cols, "%s: row stride %ld shorter than a row of %ld", who, (long)ldx, (long)cols);
    QD_REQUIRE(qmin <= qmax, "%s: empty code range [%d, %d]", who, qmin, qmax);
    QD_REQUIRE(qd_aligned(x, 4), "%s: x must be 4-byte aligned", who);
    QD_REQUIRE(qd_aligned(y, 16), "%s: y must be 16-byte aligned", who);
    p.x = x, p.rows = (long)rows, p.cols = (long)cols, p.ldx = rows == 1 ? (long)cols : (long)ldx, p.n = (long)(rows * cols);
    p.lo = (float)qmin, p.hi = (float)qmax;
    return 0;
}

}  // namespace

extern "C" int64_t qd_range_track_ws_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || rows > INT64_MAX / cols) return 0;
    return (int64_t)rt_blocks(rows * cols) * sizeof(float4);
}

extern "C" int qd_range_track(const float* x, int64_t rows, int64_t cols, int64_t ldx, float m, float om, int mode, int n_levels,
                              int qmin, int qmax, const float* range_in, const float* zero_point_in, float* state_out, float* y,
                              void* ws, void* stream) {
    RtParams p{};
    QD_REQUIRE(range_in && state_out && ws, "qd_range_track: null pointer (range_in, state_out or ws)");
    QD_REQUIRE(mode == QD_RANGE_AFFINE || mode == QD_RANGE_ALWAYS_ZERO || mode == QD_RANGE_SYMMETRIC,
               "qd_range_track: unknown mode %d", mode);
    QD_REQUIRE(mode != QD_RANGE_SYMMETRIC || zero_point_in, "qd_range_track: null pointer (the symmetric mode reads zero_point_in)");
    QD_REQUIRE(n_levels >= 2, "qd_range_track: n_levels must be at least 2 (got %d)", n_levels);
    if (rt_geometry("qd_range_track", x, rows, cols, ldx, qmin, qmax, y, p)) return 1;
    QD_REQUIRE(qd_aligned(ws, 16), "qd_range_track: ws must be 16-byte aligned (qd_range_track_ws_bytes)");
    p.m = m, p.om = om, p.mode = mode;
    p.rlev = 1.0f / (float)(mode == QD_RANGE_SYMMETRIC ? n_levels : n_levels - 1);
    p.range_in = range_in, p.zp_in = zero_point_in, p.state_out = state_out, p.y = y;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nblk = rt_blocks(p.n);
    float4* part = reinterpret_cast<float4*>(ws);
    hipLaunchKernelGGL(range_partials_kernel, dim3(nblk), dim3(RT_T), 0, s, p, part);
    hipLaunchKernelGGL(apply_kernel<true>, dim3(y ? nblk : 1), dim3(RT_T), 0, s, p, (const float4*)part, nblk);
    QD_LAUNCH_CHECK("qd_range_track");
    return 0;
}

extern "C" int qd_fakequant_rows(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* delta, const float* zero_point,
                                 int qmin, int qmax, float* y, void* stream) {
    RtParams p{};
    QD_REQUIRE(delta && zero_point && y, "qd_fakequant_rows: null pointer (delta, zero_point or y)");
    if (rt_geometry("qd_fakequant_rows", x, rows, cols, ldx, qmin, qmax, y, p)) return 1;
    p.delta = delta, p.zp = zero_point, p.y = y;
    hipLaunchKernelGGL(apply_kernel<false>, dim3(rt_blocks(p.n)), dim3(RT_T), 0, reinterpret_cast<hipStream_t>(stream), p,
                       (const float4*)nullptr, 0);
    QD_LAUNCH_CHECK("qd_fakequant_rows");
    return 0;
}
