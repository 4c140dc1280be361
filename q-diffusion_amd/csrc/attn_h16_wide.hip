// attn_h16_wide.hip — fused fp16 / bf16 attention for head dims 264 .. 512: the one-head mid-block attention of the first-stage
// decoders (reference ldm/modules/diffusionmodules/model.py:144-196: 512 channels, 4096 tokens for an SD latent).
//
// attn_h16.hip gives one wave 32 queries and ALL d channels: at d = 512 that is 256 accumulator registers for O^T plus 128 for
// the query fragment, more than a wave has.  Here the HEAD DIM is split across the four waves of a block instead:
//   * a block owns 32 queries of one (b, h); wave w owns the channel slice [128w, 128w + 128) of q, k and v.  Blocks of one
//     head are consecutive logical ids, remapped to share an XCD (qd_xcd_remap);
//   * scores: every wave contracts its slice (at most 8 k-steps of v_mfma_f32_32x32x16_{f16,bf16}, transposed as in attn_h16.hip:
//     a lane owns ONE query) into a partial 32 keys x 32 queries tile and writes it to LDS; after one barrier every wave adds the
//     partial tiles of the slices that hold channels in the fixed order 0, 1, 2, 3 (fp32 adds).  All four waves then hold the
//     same bits, and two runs give the same bits;
//   * softmax: each wave runs the online maximum / sum / exact rescale of attn_h16.hip on the full tile itself — redundant on
//     purpose (16 v_exp_f32 per lane per tile against 16 MFMAs per wave per tile): the row maximum, the row sum and P stay
//     lane-local, P goes from the score registers into the P.V MFMA without leaving the lane;
//   * P.V: a wave multiplies P into its own 128 output channels only: 4 O^T tiles of 16 accumulator registers, 32 registers of
//     query fragment;
//   * slices beyond d (d = 264: slice 2 holds 8 channels, slice 3 none) skip their k-steps and output tiles (wave-uniform):
//     they add nothing to the sum of partial tiles and store nothing;
//   * K / V tiles of 32 keys are staged cooperatively by the 256 threads through registers into a double-buffered LDS ring, the
//     next tile's global loads issued before this tile's MFMAs (attn_h16.hip, T14), converting fp32 / fp16 / bf16 inputs of any
//     (b, token, head) strides.  Two barriers per tile: one for the partial tiles, one for the ring.
// LDS (dynamic, sized by d; the function attribute is raised once per device): K rows of 2*ceil(d/16) + 1 16-byte chunks (odd, as
// in attn_h16.hip); V^T rows of 32 keys = 4 chunks with ONE pad chunk per FOUR rows (17 chunks per four channels, odd: the
// 16 rows a ds_read_b128 lane group reads land on 16 different chunk slots of the 256-byte bank window).  attn_h16.hip's pad
// chunk per V^T row would make the two stages 148480 B at d = 512 and leave no room for the 16 KB of partial tiles in the 160 KB
// of a CU; with this padding a block takes 152576 B at d = 512, so ONE block (four waves, one per SIMD) is resident per CU.
#include "attn_h16_frag.h"
#include <cmath>

namespace {

struct AttnW {
    const char* q;
    const char* k;
    const char* v;
    long qs[3], ks[3], vs[3];     // element strides (b, token, head); the channel stride is 1
    void* out;
    long ldo;
    int T, S, H, d, gx, nblk;
    float c2;                     // scale * log2(e)
    int out_dtype;
};

constexpr int AW_XCH = 4 * 4096;                               // four partial 32 x 32 fp32 tiles

// LDS bytes of one K + V^T stage for head dim d
__host__ __device__ inline int aw_kbytes(int d) { return 32 * (2 * ((d + 15) >> 4) + 1) * 16; }
__host__ __device__ inline int aw_vbytes(int d) { return (((d + 31) & ~31) >> 2) * 17 * 16; }
// byte offset of V^T row `row` (a channel) inside the V^T stage
__device__ __forceinline__ int aw_vrow(int row) { return row * 64 + (row >> 2) * 16; }

template <bool BF, int DT>
__global__ __launch_bounds__(256, 1) void attn_h16_wide_kernel(const AttnW p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, half = lane >> 5;
    const int lblk = qd_xcd_remap(blockIdx.x, p.nblk);
    const int bh = lblk / p.gx, qb = lblk - bh * p.gx;
    const int b = bh / p.H, hh = bh - b * p.H;
    const int qi = qb * 32 + frow;                             // this lane's query (the same in all four waves)
    const int d = p.d, S = p.S;
    const int dk = (d + 15) >> 4, dv = (d + 31) & ~31;         // k-steps of the whole head dim; V^T rows staged
    const int KRB = (2 * dk + 1) * 16;                         // bytes per K row
    const int KB = aw_kbytes(d), STAGE = KB + aw_vbytes(d);
    unsigned char* xch = smem + 2 * STAGE;
    const int c0 = 128 * wave;                                 // this wave's channel slice
    const int nk = min(max(dk - 8 * wave, 0), 8);              // its k-steps
    const int nt = min(max((d - c0 + 31) >> 5, 0), 4);         // its 32-channel output tiles
    const int ns = (d + 127) >> 7;                             // slices that hold channels
    const int nku = 64 * dk, nvu = 2 * dv;                     // staging units: K (key, 8 channels), V (key pair, 8 channels)

    // ---- query fragment: channels c0 + 16kk + 8*half .. +7 of query qi (B operand of the score MFMA) ----
    v4i qf[8];
    {
        const long qoff = (long)b * p.qs[0] + (long)qi * p.qs[1] + (long)hh * p.qs[2];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int c = c0 + 16 * kk + 8 * half;
            qf[kk] = ah_convert<BF, DT>(ah_load8<DT>(p.q, qoff + c, qi < p.T && c < d));
        }
    }

    const long kbase = (long)b * p.ks[0] + (long)hh * p.ks[2];
    const long vbase = (long)b * p.vs[0] + (long)hh * p.vs[2];
    Raw8 kr[8], vr[4][2];
    auto issue = [&](int jt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u;
            const int key = jt * 32 + (idx & 31), c = 8 * (idx >> 5);
            kr[u] = ah_load8<DT>(p.k, kbase + (long)key * p.ks[1] + c, idx < nku && key < S && c < d);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u;
            const int key = jt * 32 + 2 * (idx & 15), c = 8 * (idx >> 4);
            const bool ok = idx < nvu && c < d;
            const long off = vbase + (long)key * p.vs[1] + c;
            vr[u][0] = ah_load8<DT>(p.v, off, ok && key < S);
            vr[u][1] = ah_load8<DT>(p.v, off + p.vs[1], ok && key + 1 < S);
        }
    };
    // keys past S and channels past d are written as zeros: masked probabilities meet finite V, padded channels add nothing
    auto commit = [&](int buf) __attribute__((always_inline)) {
        unsigned char* ks = smem + buf * STAGE;
        unsigned char* vs = ks + KB;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + 256 * u;
            if (idx < nku) *reinterpret_cast<v4i*>(ks + (idx & 31) * KRB + (idx >> 5) * 16) = ah_convert<BF, DT>(kr[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u;
            if (idx < nvu) {
                const v4i w0 = ah_convert<BF, DT>(vr[u][0]), w1 = ah_convert<BF, DT>(vr[u][1]);
                unsigned char* col = vs + ah_vpos(2 * (idx & 15)) * 2;
                const int r0 = 8 * (idx >> 4);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned w = __builtin_amdgcn_perm((unsigned)w1[i >> 1], (unsigned)w0[i >> 1], (i & 1) ? 0x07060302u : 0x05040100u);
                    *reinterpret_cast<unsigned*>(col + aw_vrow(r0 + i)) = w;
                }
            }
        }
    };

    const int ntile = (S + 31) >> 5;
    issue(0);
    commit(0);
    __syncthreads();

    const float c2 = p.c2;
    float mrun = -INFINITY, l = 0.f;                           // running row maximum (raw score), this half's row sum
    v16f o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;

    for (int jt = 0; jt < ntile; ++jt) {
        const unsigned char* ks = smem + (jt & 1) * STAGE;
        const unsigned char* vs = ks + KB;
        const bool more = jt + 1 < ntile;
        if (more) issue(jt + 1);

        // ---- partial S^T tile of this wave's slice: acc[r] = score(query qi, key jt*32 + (r&3) + 8(r>>2) + 4*half) ----
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
            if (kk < nk) {
                const v4i kf = *reinterpret_cast<const v4i*>(ks + frow * KRB + (2 * (8 * wave + kk) + half) * 16);
                acc = ah_mfma<BF>(kf, qf[kk], acc);
            }
        // ---- the full tile: partial tiles of slices 0 .. ns-1 added in that order, by every wave ----
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<v4f*>(xch + wave * 4096 + (g * 64 + lane) * 16) = v4f{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            v4f s = *reinterpret_cast<const v4f*>(xch + (g * 64 + lane) * 16);
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (w < ns) s += *reinterpret_cast<const v4f*>(xch + w * 4096 + (g * 64 + lane) * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * g + j] = s[j];
        }
        if (jt * 32 + 32 > S) {                                // ragged last tile
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= S) acc[r] = -INFINITY;
        }

        // ---- online softmax (scale > 0: the maximum of the raw scores is the maximum of the scaled ones) ----
        float tmax = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, acc[r]);
        tmax = ah_max_halves(tmax);                            // key 0 of the tile is valid: finite
        const float mnew = fmaxf(mrun, tmax);
        if (__any(mnew > mrun)) {
            const float alpha = __builtin_amdgcn_exp2f(mrun * c2 - mnew * c2);   // 1 where the row max stayed; 0 on the first tile
            l *= alpha;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
                }
            mrun = mnew;
        }
        const float nms = -(mrun * c2);
        float e[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[r], c2, nms));
            l += e[r];
        }
        v4i pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) pf[s][j] = (int)ah_pack2<BF>(e[8 * s + 2 * j], e[8 * s + 2 * j + 1]);

        // ---- O^T += V^T . P^T on this wave's channels ----
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const v4i vf = *reinterpret_cast<const v4i*>(vs + aw_vrow(c0 + 32 * t + frow) + (2 * s + half) * 16);
                    o[t] = ah_mfma<BF>(vf, pf[s], o[t]);
                }
            }

        if (more) commit((jt + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: normalise, store merged-head rows out[b*T + qi][hh*d + c] ----
    const float inv = 1.0f / ah_sum_halves(l);
    if (qi >= p.T) return;
    const long row = ((long)b * p.T + qi) * p.ldo + (long)hh * d;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 32 * t + 8 * g + 4 * half;      // registers 4g .. 4g+3: channels c .. c+3
            if (t >= nt || c >= d) continue;
            const float y0 = o[t][4 * g] * inv, y1 = o[t][4 * g + 1] * inv, y2 = o[t][4 * g + 2] * inv, y3 = o[t][4 * g + 3] * inv;
            if (p.out_dtype == QD_F32) {
                *reinterpret_cast<v4f*>(reinterpret_cast<float*>(p.out) + row + c) = v4f{y0, y1, y2, y3};
            } else {
                uint2 w;
                if (p.out_dtype == QD_F16) { w.x = ah_pack2<false>(y0, y1); w.y = ah_pack2<false>(y2, y3); }
                else { w.x = ah_pack2<true>(y0, y1); w.y = ah_pack2<true>(y2, y3); }
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.out) + row + c) = w;
            }
        }
}

constexpr int AW_LDS_MAX = 2 * (32 * 65 * 16 + 128 * 17 * 16) + AW_XCH;      // d = 512: 152576 B of the CU's 163840

// above 64 KB the dynamic LDS of a kernel has to be allowed first: once per instantiation and device
template <bool BF, int DT>
hipError_t launch_wide(const AttnW& a, dim3 grid, hipStream_t st) {
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_h16_wide_kernel<BF, DT>), hipFuncAttributeMaxDynamicSharedMemorySize, AW_LDS_MAX);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
    const size_t lds = 2 * (size_t)(aw_kbytes(a.d) + aw_vbytes(a.d)) + AW_XCH;
    hipLaunchKernelGGL((attn_h16_wide_kernel<BF, DT>), grid, dim3(256), lds, st, a);
    return hipSuccess;
}

template <bool BF>
hipError_t launch_wide_in(const AttnW& a, int in_dtype, dim3 grid, hipStream_t st) {
    if (in_dtype == QD_F32) return launch_wide<BF, QD_F32>(a, grid, st);
    if (in_dtype == QD_F16) return launch_wide<BF, QD_F16>(a, grid, st);
    return launch_wide<BF, QD_BF16>(a, grid, st);
}

}  // namespace

extern "C" int qd_attn_h16_wide(const void* q, const void* k, const void* v, int in_dtype, int B, int T, int S, int H, int d,
                                int64_t qsb, int64_t qst, int64_t qsh, int64_t qsd, int64_t ksb, int64_t kst, int64_t ksh, int64_t ksd,
                                int64_t vsb, int64_t vst, int64_t vsh, int64_t vsd, float scale, int op_dtype, void* out, int out_dtype,
                                int64_t ldo, void* stream) {
    QD_REQUIRE(q && k && v && out, "qd_attn_h16_wide: null pointer");
    QD_REQUIRE(in_dtype == QD_F32 || in_dtype == QD_F16 || in_dtype == QD_BF16, "qd_attn_h16_wide: in_dtype must be f32/f16/bf16 (got %d)", in_dtype);
    QD_REQUIRE(op_dtype == QD_F16 || op_dtype == QD_BF16, "qd_attn_h16_wide: op_dtype must be f16/bf16 (got %d)", op_dtype);
    QD_REQUIRE(out_dtype == QD_F32 || out_dtype == QD_F16 || out_dtype == QD_BF16, "qd_attn_h16_wide: out_dtype must be f32/f16/bf16 (got %d)", out_dtype);
    QD_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "qd_attn_h16_wide: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    QD_REQUIRE(d >= 264 && d <= 512 && d % 8 == 0, "qd_attn_h16_wide: head dim %d unsupported (a multiple of 8 in [264, 512])", d);
    QD_REQUIRE(std::isfinite(scale) && scale > 0.f, "qd_attn_h16_wide: scale must be finite and positive");
    QD_REQUIRE(ldo >= (int64_t)H * d && ldo % 4 == 0 && qd_aligned(out, out_dtype == QD_F32 ? 16 : 8),
               "qd_attn_h16_wide: ldo must be >= H*d and a multiple of 4, out aligned to 4 elements");
    QD_REQUIRE(ah_layout_ok(q, in_dtype, qsb, qst, qsh, qsd) && ah_layout_ok(k, in_dtype, ksb, kst, ksh, ksd) &&
               ah_layout_ok(v, in_dtype, vsb, vst, vsh, vsd),
               "qd_attn_h16_wide: q/k/v need channel stride 1, 16-byte aligned bases and b/token/head strides that keep 16-byte alignment");
    const int64_t gx = (T + 31) / 32;
    QD_REQUIRE((int64_t)B * H * gx < (1L << 31) && (int64_t)B * T < (1L << 31), "qd_attn_h16_wide: too many blocks");
    AttnW a{};
    a.q = reinterpret_cast<const char*>(q); a.k = reinterpret_cast<const char*>(k); a.v = reinterpret_cast<const char*>(v);
    const int64_t qs[3] = {qsb, qst, qsh}, ks[3] = {ksb, kst, ksh}, vs[3] = {vsb, vst, vsh};
    for (int i = 0; i < 3; ++i) { a.qs[i] = qs[i]; a.ks[i] = ks[i]; a.vs[i] = vs[i]; }
    a.out = out; a.ldo = ldo;
    a.T = T; a.S = S; a.H = H; a.d = d; a.gx = (int)gx; a.nblk = (int)((int64_t)B * H * gx);
    a.c2 = scale * 1.4426950408889634f;
    a.out_dtype = out_dtype;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nblk);
    const hipError_t e = op_dtype == QD_BF16 ? launch_wide_in<true>(a, in_dtype, grid, st) : launch_wide_in<false>(a, in_dtype, grid, st);
    QD_REQUIRE(e == hipSuccess, "qd_attn_h16_wide: raising the dynamic LDS limit to %d bytes failed: %s", AW_LDS_MAX, hipGetErrorString(e));
    QD_LAUNCH_CHECK("qd_attn_h16_wide");
    return 0;
}
