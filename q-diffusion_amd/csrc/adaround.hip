// adaround.hip — fused AdaRound forward / backward / rounding regulariser for CALIBRATION.
//
// The weight phase of block / layer reconstruction (reference qdiff/block_recon.py:48-166) trains `alpha` of every
// AdaRoundQuantizer of the unit through autograd on
//     w_hat = (clamp(floor(w / delta) + h(alpha) + zp, 0, n_levels - 1) - zp) * delta          (adaptive_rounding.py:39-74)
//     h     = clamp(sigmoid(alpha) * (zeta - gamma) + gamma, 0, 1)
// and evaluates h a second time for the regulariser sum(1 - |2 h - 1|^b) (block_recon.py:217-229): ~20 elementwise kernels
// forward and ~25 backward over the weight tensor, with about ten saved fp32 intermediates per weight.  Here: one kernel
// forward (8 B read, 4 B written per weight) that also leaves the block-level partial sums of the regulariser (the fp32 terms
// summed in fp64: the caller rounds their total once, so reg_sum is the correctly rounded sum of the terms), and one
// backward (12 B read, 4 B written) that recomputes everything from w and alpha and writes d(loss)/d(alpha) of BOTH chains.
// The quantiser is channel-wise: delta / zp hold one value per row; a row is `cols` consecutive floats starting at
// w + row * ldw (the two halves of a split shortcut are read in place; gw of the backward likewise with ldg: a half receives a
// channel slice of the gradient of the concatenated weight), everything else is dense [rows][cols].
// The arithmetic follows the autograd graph operation by operation (FP contraction off), in autograd's order:
//     forward:   base = floor(w / delta) (IEEE division); s = 1 / (1 + exp(-alpha)); hr = s * (zeta - gamma) + gamma;
//                h = min(max(hr, 0), 1); c = (base + h) + zp; w_hat = (min(max(c, 0), n_levels - 1) - zp) * delta
//                regulariser term = 1 - (|h - 0.5| * 2)^b
//     backward:  rec = gw * delta; 0 unless 0 <= c <= n_levels - 1; 0 unless 0 <= hr <= 1 (closed intervals: ATen's clamp
//                backward); * (zeta - gamma); * (1 - s) * s
//                reg = -greg * (b * v^(b - 1)) * 2 * sgn(h - 0.5), v = |h - 0.5| * 2; 0 unless 0 <= hr <= 1; * (zeta - gamma);
//                * (1 - s) * s
//                galpha = rec + reg                                  (autograd accumulates the two chains at alpha)
// exp / pow are the device library's: w_hat differs from the composition only where h is soft, by the last places of exp.
#include "common.h"

namespace {

constexpr int AR_VEC = 4;
constexpr int AR_SPAN = 256 * AR_VEC;

struct ArParams {
    const float* w;
    const float* alpha;
    const float* delta;
    const float* zp;
    int rows, cols;
    long ldw;
    int n;                   // rows * cols
    float top;               // n_levels - 1
    float gamma, zg;         // zg = zeta - gamma
    float b;                 // <= 0: no regulariser
};

struct ArElem {
    float s, hr, h, c;
};

__device__ __forceinline__ ArElem ar_eval(float w, float a, float d, float zp, float gamma, float zg) {
#pragma clang fp contract(off)
    ArElem e;
    const float base = floorf(w / d);
    e.s = 1.f / (1.f + expf(-a));
    e.hr = e.s * zg + gamma;
    e.h = fminf(fmaxf(e.hr, 0.f), 1.f);
    e.c = (base + e.h) + zp;
    return e;
}

__device__ __forceinline__ float ar_fwd_one(float w, float a, float d, float zp, const ArParams& p, double& reg) {
#pragma clang fp contract(off)
    const ArElem e = ar_eval(w, a, d, zp, p.gamma, p.zg);
    if (p.b > 0.f) reg += (double)(1.f - powf(fabsf(e.h - 0.5f) * 2.f, p.b));     // fp32 terms, as in autograd; their SUM in fp64
    return (fminf(fmaxf(e.c, 0.f), p.top) - zp) * d;
}

__device__ __forceinline__ float ar_bwd_one(float w, float a, float g, float d, float zp, const ArParams& p, float ngreg, bool reg_on) {
#pragma clang fp contract(off)
    const ArElem e = ar_eval(w, a, d, zp, p.gamma, p.zg);
    const bool soft = e.hr >= 0.f && e.hr <= 1.f;
    float rec = g * d;
    rec = (e.c >= 0.f && e.c <= p.top) ? rec : 0.f;
    rec = soft ? rec : 0.f;
    rec = rec * p.zg;
    rec = (rec * (1.f - e.s)) * e.s;
    if (!reg_on) return rec;
    const float u = e.h - 0.5f;
    const float v = fabsf(u) * 2.f;
    float reg = ngreg * (p.b * powf(v, p.b - 1.f));
    reg = reg * 2.f;
    reg = reg * (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f));
    reg = soft ? reg : 0.f;
    reg = reg * p.zg;
    reg = (reg * (1.f - e.s)) * e.s;
    return rec + reg;
}

// Four consecutive elements of the dense index space starting at i0 (i0 % 4 == 0, i0 + 4 <= n) of a row-strided tensor
// (element i lives at src + (i / cols) * ld + i % cols): one 16-byte lane when the four lie in one row at an aligned address,
// otherwise read one by one (a lane that straddles a row end: cols % 4 != 0; an odd ld or offset).
__device__ __forceinline__ void ar_load_rows(const float* __restrict__ base, long ld, int cols, int i0, float (&v)[4]) {
    const int r = i0 / cols, c = i0 - r * cols;
    const float* src = base + (long)r * ld + c;
    if (c + AR_VEC <= cols) {
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j, rj = i / cols;
            v[j] = base[(long)rj * ld + (i - rj * cols)];
        }
    }
}

__device__ __forceinline__ void ar_load_w(const ArParams& p, int i0, float (&wv)[4], float (&dv)[4], float (&zv)[4]) {
    ar_load_rows(p.w, p.ldw, p.cols, i0, wv);
    const int r = i0 / p.cols, left = p.cols - (i0 - r * p.cols);      // elements of the four that still belong to row r
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rj = j < left ? r : (i0 + j) / p.cols;
        dv[j] = p.delta[rj], zv[j] = p.zp[rj];
    }
}

__device__ __forceinline__ void ar_load_w1(const ArParams& p, int i, float& w, float& d, float& z) {
    const int r = i / p.cols;
    w = p.w[(long)r * p.ldw + (i - r * p.cols)];
    d = p.delta[r], z = p.zp[r];
}

__global__ __launch_bounds__(256) void adaround_fwd_kernel(ArParams p, float* __restrict__ w_hat, double* __restrict__ part) {
    __shared__ double red[4];
    const long i0l = ((long)blockIdx.x * 256 + threadIdx.x) * AR_VEC;
    double reg = 0.;
    if (i0l + AR_VEC <= p.n) {
        const int i0 = (int)i0l;
        float wv[4], dv[4], zv[4], o[4];
        ar_load_w(p, i0, wv, dv, zv);
        const float4 a = *reinterpret_cast<const float4*>(p.alpha + i0);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ar_fwd_one(wv[j], av[j], dv[j], zv[j], p, reg);
        *reinterpret_cast<float4*>(w_hat + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (long i = i0l; i < p.n; ++i) {
            float w, d, z;
            ar_load_w1(p, (int)i, w, d, z);
            w_hat[i] = ar_fwd_one(w, p.alpha[i], d, z, p, reg);
        }
    }
    if (part == nullptr) return;                        // uniform: no regulariser asked for
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) reg += __shfl_xor(reg, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = reg;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void adaround_bwd_kernel(ArParams p, const float* __restrict__ gw, long ldg,
                                                           const float* __restrict__ greg, float* __restrict__ galpha) {
    const long i0l = ((long)blockIdx.x * 256 + threadIdx.x) * AR_VEC;
    const bool reg_on = greg != nullptr && p.b > 0.f;
    const float ngreg = reg_on ? -greg[0] : 0.f;
    if (i0l + AR_VEC <= p.n) {
        const int i0 = (int)i0l;
        float wv[4], dv[4], zv[4], gv[4], o[4];
        ar_load_w(p, i0, wv, dv, zv);
        ar_load_rows(gw, ldg, p.cols, i0, gv);
        const float4 a = *reinterpret_cast<const float4*>(p.alpha + i0);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ar_bwd_one(wv[j], av[j], gv[j], dv[j], zv[j], p, ngreg, reg_on);
        *reinterpret_cast<float4*>(galpha + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (long i = i0l; i < p.n; ++i) {
            float w, d, z;
            ar_load_w1(p, (int)i, w, d, z);
            const int r = (int)i / p.cols;
            galpha[i] = ar_bwd_one(w, p.alpha[i], gw[(long)r * ldg + ((int)i - r * p.cols)], d, z, p, ngreg, reg_on);
        }
    }
}

int ar_params(const char* who, const float* w, int64_t rows, int64_t cols, int64_t ldw, const float* alpha, const float* delta,
              const float* zp, int n_levels, float gamma, float zeta, float reg_b, ArParams& p) {
    QD_REQUIRE(w && alpha && delta && zp, "%s: null pointer", who);
    QD_REQUIRE(rows > 0 && cols > 0, "%s: empty tensor (rows = %ld, cols = %ld)", who, (long)rows, (long)cols);
    QD_REQUIRE(ldw >= cols, "%s: row stride %ld shorter than a row of %ld", who, (long)ldw, (long)cols);
    QD_REQUIRE(rows * cols < (1L << 31), "%s: %ld x %ld elements do not fit the 31-bit index", who, (long)rows, (long)cols);
    QD_REQUIRE(n_levels >= 2, "%s: n_levels must be at least 2 (got %d)", who, n_levels);
    QD_REQUIRE(zeta > gamma, "%s: the stretch needs zeta > gamma", who);
    QD_REQUIRE(qd_aligned(w, 4) && qd_aligned(alpha, 16), "%s: alpha must be 16-byte aligned (w: 4-byte)", who);
    p.w = w, p.alpha = alpha, p.delta = delta, p.zp = zp;
    p.rows = (int)rows, p.cols = (int)cols, p.ldw = (long)ldw, p.n = (int)(rows * cols);
    p.top = (float)(n_levels - 1);
    p.gamma = gamma, p.zg = (float)((double)zeta - (double)gamma);
    p.b = reg_b;
    return 0;
}

}  // namespace

extern "C" int64_t qd_adaround_blocks(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (rows * cols + AR_SPAN - 1) / AR_SPAN;
}

extern "C" int qd_adaround_fwd(const float* w, int64_t rows, int64_t cols, int64_t ldw, const float* alpha, const float* delta,
                               const float* zero_point, int n_levels, float gamma, float zeta, float reg_b, float* w_hat,
                               double* reg_part, void* stream) {
    ArParams p;
    if (int rc = ar_params("qd_adaround_fwd", w, rows, cols, ldw, alpha, delta, zero_point, n_levels, gamma, zeta, reg_b, p)) return rc;
    QD_REQUIRE(w_hat, "qd_adaround_fwd: null pointer");
    QD_REQUIRE(qd_aligned(w_hat, 16), "qd_adaround_fwd: w_hat must be 16-byte aligned");
    QD_REQUIRE(reg_b <= 0.f || reg_part, "qd_adaround_fwd: reg_b > 0 needs the buffer of partial sums");
    hipLaunchKernelGGL(adaround_fwd_kernel, dim3((unsigned)qd_adaround_blocks(rows, cols)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), p, w_hat, reg_b > 0.f ? reg_part : nullptr);
    QD_LAUNCH_CHECK("qd_adaround_fwd");
    return 0;
}

extern "C" int qd_adaround_bwd(const float* gw, int64_t ldg, const float* w, int64_t rows, int64_t cols, int64_t ldw, const float* alpha,
                               const float* delta, const float* zero_point, int n_levels, float gamma, float zeta, float reg_b,
                               const float* greg, float* galpha, void* stream) {
    ArParams p;
    if (int rc = ar_params("qd_adaround_bwd", w, rows, cols, ldw, alpha, delta, zero_point, n_levels, gamma, zeta, reg_b, p)) return rc;
    QD_REQUIRE(gw && galpha, "qd_adaround_bwd: null pointer");
    QD_REQUIRE(ldg >= cols, "qd_adaround_bwd: gw row stride %ld shorter than a row of %ld", (long)ldg, (long)cols);
    QD_REQUIRE(qd_aligned(gw, 4) && qd_aligned(galpha, 16), "qd_adaround_bwd: galpha must be 16-byte aligned (gw: 4-byte)");
    hipLaunchKernelGGL(adaround_bwd_kernel, dim3((unsigned)qd_adaround_blocks(rows, cols)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), p, gw, (long)ldg, greg, galpha);
    QD_LAUNCH_CHECK("qd_adaround_bwd");
    return 0;
}
