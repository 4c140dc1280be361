// recon_loss.hip — fused reconstruction term of the calibration objective and its gradient.
//
// Every iteration of recon._reconstruct gathers the target rows (`cache[idx]`), evaluates lp_loss(pred, tgt, 2) =
// (pred - tgt).abs().pow(2).sum(1).mean() (reference qdiff/quant_layer.py:26-33) or the diagonal-Fisher term
// ((pred - tgt).pow(2) * grad.pow(2)).sum(1).mean() (qdiff/block_recon.py:192-215) and lets autograd walk the chain back: about
// ten full-tensor launches.  Here: ONE streaming pass that reads pred, reads the target (and the Fisher gradient) IN PLACE from
// the cache row idx[b], writes dloss/dpred and keeps the loss terms in registers, plus a one-block finalise.  12 B per element
// for MSE (16 for FISHER_DIAG), no gathered copy.
//
// Geometry.  A sample is a logical [C][S] map (S = the product of the spatial extents); it is dense either channel-major
// (NCHW: c * S + s) or channels-last (s * C + c).  pred sample b starts at pred + b * ldp, cache row r at cache + r * ldc,
// gpred is dense in pred's order.  All element indices are 64-bit.
//   flat  (pred and cache in the same order)   a work item is 4096 consecutive elements of one sample: four quads per lane,
//         16-byte loads and stores when the three (four) sample bases are 16-byte aligned, else — and for the last quad of a
//         sample whose size is no multiple of 4 — 4-byte accesses, each guarded by the sample's size.
//   mixed (one NCHW, the other channels-last)  with x pred's fast axis and y its slow one, pred is y * NX + x and the cache row
//         is x * NY + y.  A work item is a 64 x 64 tile.  The block reads the cache side along ITS fast axis (a wave = 64
//         consecutive floats of y), stores it to LDS as [x][y] with rows padded to 65 floats, and reads it back as [y][x]: lane l
//         then touches word 65 l + const, i.e. bank (l + const) mod 64 — no conflicts either way.  pred is read and gpred written
//         along x.  Ragged tiles are predicated per element; nothing is padded in memory.
// Blocks take work items grid-stride (at most 2048 blocks).  A lane adds the 16 terms of an item pairwise and chains the items
// (three for a 16 x 320 x 64 x 64 output); the block's sum is a wave butterfly and ((w0 + w1) + (w2 + w3)) through LDS: ONE fp32
// partial per block.  The finalise block adds at most 2048 partials as the same tree and multiplies by inv.  No atomics, a fixed
// order: two runs agree bit for bit.
//
// Arithmetic, operation by operation in fp32 (FP contraction off), as autograd evaluates the composition for an upstream
// gradient of 1.  inv = 1.0f / float(M), M = B * S: mean's backward divides by the count, which ATen does as a product with the
// fp32 reciprocal.  d = pred - tgt.
//   MSE, p = 2     term = |d| * |d|                       gpred = (inv * (2 * |d|)) * sgn(d)         sgn(0) = sgn(NaN) = 0
//   FISHER_DIAG    term = (d * d) * (g * g)               gpred = (inv * (g * g)) * (2 * d)
// (pow's backward is grad * (2 * x^1); the factor orders above are the ones the installed torch was seen to use.)
// A NaN in pred reaches the loss and that one element of gpred.  An idx[b] outside [0, cache_rows) is never dereferenced: the
// sample's target reads as NaN, so the loss and that sample's gpred are NaN.
#include "common.h"

namespace {

constexpr int RL_T = 256;                     // threads per block
constexpr int RL_ITEM = RL_T * 16;            // flat: elements of a work item
constexpr int RL_TILE = 64;                   // mixed: tile edge
constexpr int RL_PAD = RL_TILE + 1;           // mixed: LDS row stride in floats
constexpr int RL_MAX_BLOCKS = 2048;           // 256 CUs x 8 blocks of four waves; also what the finalise block takes in one sweep

struct RlParams {
    const float *pred, *tgt, *grad;
    const int64_t* idx;
    float* gpred;
    long B, cache_rows, ldp, ldc, cs;         // cs = C * S, the elements of a sample
    long nx, ny, tx;                          // mixed: extents of pred's fast and slow axis, tiles along x
    long per;                                 // work items per sample
    float inv;
};

// one element: the loss term, and the gradient into gp
template <bool FISHER>
__device__ __forceinline__ float rl_one(float p, float t, float g, float inv, float& gp) {
#pragma clang fp contract(off)
    const float d = p - t;
    if constexpr (FISHER) {
        const float g2 = g * g;
        gp = (inv * g2) * (2.f * d);
        return (d * d) * g2;
    } else {
        const float a = fabsf(d);
        gp = (inv * (2.f * a)) * (float)((d > 0.f) - (d < 0.f));
        return a * a;
    }
}

__device__ __forceinline__ float rl_pairwise16(float (&t)[16]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int h = 8; h > 0; h >>= 1)
#pragma unroll
        for (int j = 0; j < h; ++j) t[j] = t[j] + t[j + h];
    return t[0];
}

// the sum of the block's 256 lanes, valid in thread 0: butterfly over the wave, ((w0 + w1) + (w2 + w3)) through LDS
__device__ __forceinline__ float rl_block_sum(float v) {
#pragma clang fp contract(off)
    __shared__ float sw[RL_T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

struct RlSample {
    const float *p, *t, *g;
    float* o;
    bool ok;                                  // idx[b] names a cache row
};

template <bool FISHER>
__device__ __forceinline__ RlSample rl_sample(const RlParams& p, long b) {
    const long r = p.idx[b];
    RlSample s;
    s.ok = r >= 0 && r < p.cache_rows;
    const long row = s.ok ? r : 0;
    s.p = p.pred + b * p.ldp, s.t = p.tgt + row * p.ldc, s.g = FISHER ? p.grad + row * p.ldc : nullptr, s.o = p.gpred + b * p.cs;
    return s;
}

template <bool FISHER>
__global__ __launch_bounds__(RL_T) void rl_flat_kernel(RlParams p, float* __restrict__ part) {
    const int tid = threadIdx.x;
    const float nanv = __builtin_nanf("");
    const long items = p.B * p.per;
    float acc = 0.f;
    for (long w = blockIdx.x; w < items; w += gridDim.x) {
        const long b = w / p.per, off = (w - b * p.per) * RL_ITEM;
        const RlSample s = rl_sample<FISHER>(p, b);
        uintptr_t bits = reinterpret_cast<uintptr_t>(s.p) | reinterpret_cast<uintptr_t>(s.t) | reinterpret_cast<uintptr_t>(s.o);
        if (FISHER) bits |= reinterpret_cast<uintptr_t>(s.g);
        const bool vec = (bits & 15) == 0;
        float pv[16], tv[16], gv[16], term[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                               // all loads of the item first: sixteen floats per stream in flight
            const long o = off + q * (RL_T * 4) + tid * 4;
            if (vec && o + 4 <= p.cs) {
                const float4 a = *reinterpret_cast<const float4*>(s.p + o);
                pv[4 * q] = a.x, pv[4 * q + 1] = a.y, pv[4 * q + 2] = a.z, pv[4 * q + 3] = a.w;
                if (s.ok) {
                    const float4 c = *reinterpret_cast<const float4*>(s.t + o);
                    tv[4 * q] = c.x, tv[4 * q + 1] = c.y, tv[4 * q + 2] = c.z, tv[4 * q + 3] = c.w;
                    if constexpr (FISHER) {
                        const float4 e = *reinterpret_cast<const float4*>(s.g + o);
                        gv[4 * q] = e.x, gv[4 * q + 1] = e.y, gv[4 * q + 2] = e.z, gv[4 * q + 3] = e.w;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = o + j < p.cs;
                    pv[4 * q + j] = in ? s.p[o + j] : 0.f;
                    tv[4 * q + j] = in && s.ok ? s.t[o + j] : 0.f;
                    if constexpr (FISHER) gv[4 * q + j] = in && s.ok ? s.g[o + j] : 0.f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long o = off + q * (RL_T * 4) + tid * 4;
            float gp[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                const bool in = o + j < p.cs;
                const float t = s.ok ? tv[e] : nanv, g = FISHER ? (s.ok ? gv[e] : nanv) : 0.f;
                const float v = rl_one<FISHER>(pv[e], t, g, p.inv, gp[j]);
                term[e] = in ? v : 0.f;
            }
            if (vec && o + 4 <= p.cs) {
                *reinterpret_cast<float4*>(s.o + o) = make_float4(gp[0], gp[1], gp[2], gp[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (o + j < p.cs) s.o[o + j] = gp[j];
            }
        }
        acc = acc + rl_pairwise16(term);
    }
    acc = rl_block_sum(acc);
    if (tid == 0) part[blockIdx.x] = acc;
}

template <bool FISHER>
__global__ __launch_bounds__(RL_T) void rl_mixed_kernel(RlParams p, float* __restrict__ part) {
    __shared__ float st[RL_TILE * RL_PAD];
    __shared__ float sg[FISHER ? RL_TILE * RL_PAD : 1];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const float nanv = __builtin_nanf("");
    const long items = p.B * p.per;
    float acc = 0.f;
    for (long w = blockIdx.x; w < items; w += gridDim.x) {
        const long b = w / p.per, rem = w - b * p.per;
        const long tyi = rem / p.tx, x0 = (rem - tyi * p.tx) * RL_TILE, y0 = tyi * RL_TILE;
        const RlSample s = rl_sample<FISHER>(p, b);
        const long yc = y0 + l;                                     // the cache side along its fast axis y, into LDS as [x][y]
#pragma unroll
        for (int k = 0; k < RL_TILE / 4; ++k) {
            const int xr = wv + 4 * k;
            const long xc = x0 + xr;
            const bool in = xc < p.nx && yc < p.ny && s.ok;
            st[xr * RL_PAD + l] = in ? s.t[xc * p.ny + yc] : nanv;
            if constexpr (FISHER) sg[xr * RL_PAD + l] = in ? s.g[xc * p.ny + yc] : nanv;
        }
        __syncthreads();
        const long xp = x0 + l;                                     // pred and gpred along their fast axis x; LDS read back as [y][x]
        float term[16];
#pragma unroll
        for (int k = 0; k < RL_TILE / 4; ++k) {
            const int yr = wv + 4 * k;
            const long yp = y0 + yr;
            term[k] = 0.f;
            if (xp < p.nx && yp < p.ny) {
                const long e = yp * p.nx + xp;
                float gp;
                term[k] = rl_one<FISHER>(s.p[e], st[l * RL_PAD + yr], FISHER ? sg[l * RL_PAD + yr] : 0.f, p.inv, gp);
                s.o[e] = gp;
            }
        }
        acc = acc + rl_pairwise16(term);
        __syncthreads();                                            // the tile is free for the next item
    }
    acc = rl_block_sum(acc);
    if (tid == 0) part[blockIdx.x] = acc;
}

// loss = (the tree sum of the partials) * inv: eight per lane pairwise, then the block's tree
__global__ __launch_bounds__(RL_T) void rl_finalise_kernel(const float* __restrict__ part, int npart, float inv, float* __restrict__ loss) {
#pragma clang fp contract(off)
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = threadIdx.x * 8 + j;
        t[j] = i < npart ? part[i] : 0.f;
    }
    const float v = rl_block_sum(((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])));
    if (threadIdx.x == 0) loss[0] = v * inv;
}

// g *= gout[0] unless gout[0] is exactly 1: then no byte of g is touched
__global__ __launch_bounds__(RL_T) void rl_scale_kernel(float* __restrict__ g, long n, const float* __restrict__ gout) {
    const float s = gout[0];
    if (s == 1.f) return;
    for (long i = (long)blockIdx.x * RL_T + threadIdx.x; i < n; i += (long)gridDim.x * RL_T) g[i] = g[i] * s;
}

static_assert(RL_MAX_BLOCKS == RL_T * 8, "the finalise block takes every partial in one sweep of eight per lane");

}  // namespace

extern "C" int64_t qd_recon_loss_ws_bytes(int64_t B, int64_t C, int64_t S) {
    if (B <= 0 || C <= 0 || S <= 0) return 0;
    return (int64_t)RL_MAX_BLOCKS * sizeof(float);
}

extern "C" int qd_recon_loss(const float* pred, int64_t ldp, int pred_cl, const float* tgt_cache, const float* grad_cache,
                             int64_t cache_rows, int64_t ldc, int cache_cl, const int64_t* idx, int64_t B, int64_t C, int64_t S,
                             int mode, float* loss, float* gpred, void* ws, void* stream) {
    QD_REQUIRE(pred && tgt_cache && idx && loss && gpred && ws, "qd_recon_loss: null pointer (pred, tgt_cache, idx, loss, gpred or ws)");
    QD_REQUIRE(mode == QD_RECON_MSE || mode == QD_RECON_FISHER_DIAG, "qd_recon_loss: unknown mode %d", mode);
    QD_REQUIRE(mode != QD_RECON_FISHER_DIAG || grad_cache, "qd_recon_loss: null pointer (FISHER_DIAG reads grad_cache)");
    QD_REQUIRE(B > 0 && C > 0 && S > 0 && cache_rows > 0, "qd_recon_loss: empty tensor (B = %ld, C = %ld, S = %ld, cache rows = %ld)",
               (long)B, (long)C, (long)S, (long)cache_rows);
    QD_REQUIRE(C <= INT64_MAX / S && B <= INT64_MAX / (C * S) && cache_rows <= INT64_MAX / (C * S),
               "qd_recon_loss: %ld x %ld x %ld elements do not fit the 64-bit index", (long)B, (long)C, (long)S);
    const int64_t cs = C * S;
    QD_REQUIRE(B == 1 || ldp >= cs, "qd_recon_loss: sample stride %ld of pred shorter than a sample of %ld", (long)ldp, (long)cs);
    QD_REQUIRE(cache_rows == 1 || ldc >= cs, "qd_recon_loss: row stride %ld of the cache shorter than a row of %ld", (long)ldc, (long)cs);
    QD_REQUIRE(qd_aligned(pred, 4) && qd_aligned(tgt_cache, 4) && qd_aligned(grad_cache, 4) && qd_aligned(gpred, 4) && qd_aligned(loss, 4) &&
                   qd_aligned(ws, 4), "qd_recon_loss: pred, the caches, gpred, loss and ws must be 4-byte aligned");
    QD_REQUIRE(qd_aligned(idx, 8), "qd_recon_loss: idx must be 8-byte aligned");
    RlParams p{};
    p.pred = pred, p.tgt = tgt_cache, p.grad = grad_cache, p.idx = idx, p.gpred = gpred;
    p.B = (long)B, p.cache_rows = (long)cache_rows, p.ldp = B == 1 ? (long)cs : (long)ldp, p.ldc = cache_rows == 1 ? (long)cs : (long)ldc;
    p.cs = (long)cs;
    p.inv = 1.0f / (float)(B * S);
    const bool mixed = C > 1 && S > 1 && (pred_cl != 0) != (cache_cl != 0);       // with C = 1 or S = 1 the two orders are one
    if (mixed) {
        p.nx = pred_cl ? (long)C : (long)S, p.ny = pred_cl ? (long)S : (long)C;
        p.tx = (p.nx + RL_TILE - 1) / RL_TILE;
        p.per = p.tx * ((p.ny + RL_TILE - 1) / RL_TILE);
    } else {
        p.per = (p.cs + RL_ITEM - 1) / RL_ITEM;
    }
    QD_REQUIRE(p.per <= INT64_MAX / p.B, "qd_recon_loss: too many work items");
    const long items = p.B * p.per;
    const int nblk = (int)(items < RL_MAX_BLOCKS ? items : RL_MAX_BLOCKS);
    const bool fisher = mode == QD_RECON_FISHER_DIAG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* part = reinterpret_cast<float*>(ws);
    if (mixed) {
        if (fisher) hipLaunchKernelGGL(rl_mixed_kernel<true>, dim3(nblk), dim3(RL_T), 0, s, p, part);
        else hipLaunchKernelGGL(rl_mixed_kernel<false>, dim3(nblk), dim3(RL_T), 0, s, p, part);
    } else {
        if (fisher) hipLaunchKernelGGL(rl_flat_kernel<true>, dim3(nblk), dim3(RL_T), 0, s, p, part);
        else hipLaunchKernelGGL(rl_flat_kernel<false>, dim3(nblk), dim3(RL_T), 0, s, p, part);
    }
    hipLaunchKernelGGL(rl_finalise_kernel, dim3(1), dim3(RL_T), 0, s, (const float*)part, nblk, p.inv, loss);
    QD_LAUNCH_CHECK("qd_recon_loss");
    return 0;
}

extern "C" int qd_recon_loss_scale(float* gpred, int64_t n, const float* gout, void* stream) {
    QD_REQUIRE(gpred && gout, "qd_recon_loss_scale: null pointer (gpred or gout)");
    QD_REQUIRE(n > 0, "qd_recon_loss_scale: empty tensor (n = %ld)", (long)n);
    QD_REQUIRE(qd_aligned(gpred, 4) && qd_aligned(gout, 4), "qd_recon_loss_scale: gpred and gout must be 4-byte aligned");
    const int64_t want = (n + RL_T - 1) / RL_T;
    hipLaunchKernelGGL(rl_scale_kernel, dim3((int)(want < RL_MAX_BLOCKS ? want : RL_MAX_BLOCKS)), dim3(RL_T), 0,
                       reinterpret_cast<hipStream_t>(stream), gpred, (long)n, gout);
    QD_LAUNCH_CHECK("qd_recon_loss_scale");
    return 0;
}
