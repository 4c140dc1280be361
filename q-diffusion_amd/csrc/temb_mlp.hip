// temb_mlp.hip — K6: the timestep-embedding MLPs as ONE launch per dependency level.
//
// Replaces (reference ldm/modules/diffusionmodules/openaimodel.py:758-759 `time_embed` = Linear -> SiLU -> Linear, and
// qdiff/quant_block.py:98-107 / ddim diffusion.py:127 the per-ResBlock `emb_layers` = SiLU -> Linear on the SAME
// embedding): in the reference every one of those Linears is a QuantModule — its own activation quantiser on
// SiLU(emb), 4/8-bit weights — evaluated on M = batch rows.  As generic GEMM launches they are ~70 tiny dependent
// launches per UNet evaluation (SiLU, row quantiser, split-K contraction, split-K finalise for each of 22 ResBlocks + 2)
// that cost ~0.7 ms of a 24 ms SD evaluation while moving 13 MB.  Here one launch evaluates L Linears that share one
// input: block = (layer, 64 output channels); it quantises SiLU(x) with THAT layer's activation quantiser into LDS
// (exact torch.round(x / delta) codes), contracts against the layer's MFMA-tile-ordered weights (the same packed array
// the generic kernel reads: 32 consecutive channels of one 16-wide K chunk are 256 / 512 contiguous bytes, so lanes =
// channels gives coalesced loads) with v_dot4 (M is 16..64 rows: the matrix pipe has nothing to amortise), and applies the
// generic kernel's epilogue — I = acc - z'*Wsum - zw*(Asum - K*z'), out = float(I)*scale + bias — in the same float
// order, so the results equal the generic path's bit for bit whenever the SiLU inputs do.
// Bound: latency (the launch is ~10 us; 13 MB of weights would take 3 us at HBM speed).
#include "common.h"
#include "wq_codes.h"

namespace {

struct TembLayer {
    const uint8_t* w;        // tile-ordered weights (qd_pack_weights_t4 / _t8), K-step 0 of the layer's only segment
    const float*   scale;    // [Cout] delta_x * delta_w[n]
    const int*     zc;       // [Cout] z' * Wsum[n] or NULL
    const int*     zw;       // [Cout] weight zero point of the stored operand or NULL
    const float*   bias;     // [Cout] or NULL
    const float*   qp;       // float[4] activation quantiser (qd_make_qparams)
    const int*     zfill;    // {z', K*z'} or NULL
    int Cout, out_off;
};

// Round 6: grid = (blocks, row groups).  The (layer, 64-channel) blocks of the 22 embedding projections number 40 .. 80 — a
// quarter of the CUs, one wave per SIMD each, every block quantising ALL rows for itself (SiLU + the exact division: the bulk
// of its time).  blockIdx.y now selects a slice of `rpb` rows: the same work per row, spread over the idle CUs (rows are
// independent: same bytes).
template <int WB, int RB>   // RB = rows per pass (accumulators per thread)
__global__ __launch_bounds__(256) void temb_kernel(const float* __restrict__ x, long ldx, int Btot, int rpb, int K, int silu,
                                                   const TembLayer* __restrict__ layers, const int2* __restrict__ blocks,
                                                   float qmin, float qmax, int off, float* __restrict__ out, long ldo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int b_first = blockIdx.y * rpb;
    const int B = min(rpb, Btot - b_first);
    if (B <= 0) return;
    x += (long)b_first * ldx;
    out += (long)b_first * ldo;
    int8_t* codes = reinterpret_cast<int8_t*>(sm);                       // [B][K]
    int* sAsum = reinterpret_cast<int*>(sm + (size_t)B * K);              // [B]
    int* sRed = sAsum + ((B + 3) & ~3);                                   // [4 parts][RB][64]
    const int2 bl = blocks[blockIdx.x];
    const TembLayer L = layers[bl.x];
    const int n0 = bl.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int part = __builtin_amdgcn_readfirstlane(tid >> 6);           // wave = K partition
    const QP q = qd_load_qp(L.qp);

    // ---- 1. SiLU -> this layer's activation quantiser -> int8 rows in LDS, row sums ---------------------------------
    for (int b = tid; b < B; b += 256) sAsum[b] = 0;                     // B may exceed the block (K = 128: up to 352 rows per launch)
    __syncthreads();
    const int k4n = K >> 2;
    auto quant = [&](auto ft) __attribute__((always_inline)) {
    constexpr bool FAST = decltype(ft)::value;
    for (int idx = tid; idx < B * k4n; idx += 256) {
        const int b = idx / k4n, k4 = idx - b * k4n;
        const float4 v = *reinterpret_cast<const float4*>(x + (long)b * ldx + k4 * 4);
        float e[4] = {v.x, v.y, v.z, v.w};
        unsigned u = 0;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float y = e[j];
            if (silu) y = y / (1.0f + expf(-y));                   // torch's silu: x / (1 + exp(-x))
            const int c = qd_code_t<FAST>(y, q, qmin, qmax) - off;
            s += c;
            u |= (unsigned)(c & 0xff) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(codes + (long)b * K + k4 * 4) = u;
        atomicAdd(&sAsum[b], s);
    }
    };
    QD_FAST_DISPATCH(q.fast, quant);
    __syncthreads();

    // ---- 2. contraction: lane = output channel, wave = every 4th 16-wide K chunk ---------------------------------------
    const int n = n0 + lane;
    const int ntiles = (L.Cout + 31) >> 5;
    const bool nin = (n >> 5) < ntiles;                                   // the tile exists in the packed array
    constexpr int UB = WB * 2;                                            // bytes of one (channel, 16-K chunk) unit
    const uint8_t* wn = L.w + ((long)(n >> 5) * 4 * 32 + (n & 31)) * UB;  // + (kstep*ntiles*4 + chunk%4) * 32 * UB
    const int nchunk = K >> 4;
    const int kz = L.zfill ? L.zfill[1] : 0;
    float sc = 0.f, bias_n = 0.f;
    int zc_n = 0, zw_n = 0;
    if (n < L.Cout) {
        sc = L.scale[n];
        if (L.zc) zc_n = L.zc[n];
        if (L.zw) zw_n = L.zw[n];
        if (L.bias) bias_n = L.bias[n];
    }
    for (int b0 = 0; b0 < B; b0 += RB) {
        int acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0;
        for (int c = part; c < nchunk; c += 4) {
            v4i wv = {0, 0, 0, 0};
            if (nin) {
                const uint8_t* src = wn + ((long)(c >> 2) * ntiles * 4 + (c & 3)) * 32 * UB;
                if constexpr (WB == 4) {
                    const uint2 pk = *reinterpret_cast<const uint2*>(src);
                    wv = v4i{(int)(pk.x & 0x0F0F0F0Fu), (int)((pk.x >> 4) & 0x0F0F0F0Fu),
                             (int)(pk.y & 0x0F0F0F0Fu), (int)((pk.y >> 4) & 0x0F0F0F0Fu)};
                } else {
                    wv = *reinterpret_cast<const v4i*>(src);
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (b0 + r < B) {                                          // wave-uniform
                    const v4i a = *reinterpret_cast<const v4i*>(codes + (long)(b0 + r) * K + c * 16);   // broadcast read
                    int s = acc[r];
                    s = __builtin_amdgcn_sdot4(a.x, wv.x, s, false);
                    s = __builtin_amdgcn_sdot4(a.y, wv.y, s, false);
                    s = __builtin_amdgcn_sdot4(a.z, wv.z, s, false);
                    acc[r] = __builtin_amdgcn_sdot4(a.w, wv.w, s, false);
                }
            }
        }
        // ---- 3. combine the four K partitions, epilogue ---------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < RB; ++r) sRed[(part * RB + r) * 64 + lane] = acc[r];
        __syncthreads();
        for (int r = part; r < RB; r += 4) {                               // wave w finishes rows w, w+4, ...
            const int b = b0 + r;
            if (b < B && n < L.Cout) {
                const int a = sRed[r * 64 + lane] + sRed[(RB + r) * 64 + lane] + sRed[(2 * RB + r) * 64 + lane] + sRed[(3 * RB + r) * 64 + lane];
                const int I = a - zc_n - zw_n * (sAsum[b] - kz);
                out[(long)b * ldo + L.out_off + n] = (float)I * sc + bias_n;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Weights-only form (qd_temb_mlp_wq_h16): the same Linears in the reference's (weight_quant, act_quant) = (True, False) state
// (quant_layer.py:620-631), where each was a torch SiLU, a qd_rows_to_h16 and a qd_conv2d_wq_h16 launch whose 128 x 128 tile
// held 2 .. 64 real rows:
//     out[b][out_off + n] = delta[n] * sum_k r(silu?(x[b][k])) * (q[k][n] - z[n]) + bias[n]
// r = the ONE rounding to fp16 / bf16 (nearest even, the packing functions of qd_rows_to_h16).
// One wave = one 32-row x 32-channel tile of one layer on v_mfma_f32_32x32x16_{f16,bf16}, and it walks K exactly as
// wq_h16_kernel (csrc/wq_h16.hip) walks it for the same output element: 64-channel K-steps in order, in each the four MFMAs
// (g, u) over k = g*32 + half*16 + u*8 + 0..7, the same A / B lane maps, the weight fragment q - z by the same functions
// (wq_magic / wq_frag of wq_codes.h), channels past K as zeros, then qd_wq_affine(acc, delta, 0, bias).  The same operand values in the same
// places of the same instructions give the same fp32 bits, so the results equal the unsplit generic path's bit for bit
// whenever the SiLU values do — the property the int8 kernel above has towards qd_conv2d_i8 — and a model does not move when the
// knob flips.  (An FMA or dot2 chain sums in another order: agreement to rounding only, and in a network of fp16 roundings a
// 1e-7 difference in the embedding flips operand roundings downstream.)  With 2 .. 64 rows most of the 32-row tile is idle;
// the launch is bound by latency either way.  The operand fragment is made in registers (8 floats -> SiLU -> 8 halves per
// lane and MFMA): no LDS, no barrier, any number of rows.  block = 64 channels of a layer = 2 waves, grid.y = 32-row groups.
// ---------------------------------------------------------------------------------------------
struct TembWqLayer {
    const uint8_t* w;        // tile-ordered codes (qd_pack_weights_t4 / _t8), K-step 0 of the layer's only segment
    const float*   delta;    // [Cout] delta_w[n]
    const int*     z;        // [Cout] RAW weight zero point
    const float*   bias;     // [Cout] or NULL
    int Cout, out_off;
};

typedef float tw_v16f __attribute__((ext_vector_type(16)));

template <int WB, bool FH>
__global__ __launch_bounds__(128) void temb_wq_kernel(const float* __restrict__ x, long ldx, int B, int K, int silu,
                                                      const TembWqLayer* __restrict__ layers, const int2* __restrict__ blocks,
                                                      float* __restrict__ out, long ldo) {
    constexpr int UB = 2 * WB, TB = 256 * WB;                  // bytes of one unit (16 codes of a channel), of one (K-step, 32-channel) tile
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frow = lane & 31, fhalf = lane >> 5;
    const int2 bl = blocks[blockIdx.x];
    const TembWqLayer L = layers[bl.x];
    const int n0 = bl.y + 32 * wave;
    if (n0 >= L.Cout) return;                                  // (wave-uniform; the kernel has no barrier)
    const int m0 = blockIdx.y * 32, row = m0 + frow;
    const bool rok = row < B;
    const float* xr = x + (long)(rok ? row : 0) * ldx;
    const int n = n0 + frow;
    const bool nok = n < L.Cout;
    const int ntiles = (L.Cout + 31) >> 5;
    const int z = nok ? L.z[n] : 0;
    const _Float16 hz = (_Float16)(float)(-(1024 + z));        // exact: |1024 + z| <= 2048
    const v2h nz = {hz, hz};
    const float dl = nok ? L.delta[n] : 0.f, bias = (nok && L.bias) ? L.bias[n] : 0.f;
    tw_v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nst = (K + 63) >> 6;
    for (int ks = 0; ks < nst; ++ks) {
        const uint8_t* wsrc = L.w + ((long)ks * ntiles + (n0 >> 5)) * TB;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            v4i mag[2];
            const uint8_t* bp = wsrc + ((g * 2 + fhalf) * 32 + frow) * UB;
            if constexpr (WB == 4) {
                const uint2 raw = *reinterpret_cast<const uint2*>(bp);
                mag[0] = wq_magic<4>(raw.x, 0u);
                mag[1] = wq_magic<4>(raw.y, 0u);
            } else {
                const v4i raw = *reinterpret_cast<const v4i*>(bp);
                mag[0] = wq_magic<8>((unsigned)raw.x, (unsigned)raw.y);
                mag[1] = wq_magic<8>((unsigned)raw.z, (unsigned)raw.w);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k0 = ks * 64 + g * 32 + fhalf * 16 + u * 8;
                v4i af = {0, 0, 0, 0};                             // rows past B and channels past K read zeros
                if (rok && k0 < K) {
                    const float4 v0 = *reinterpret_cast<const float4*>(xr + k0), v1 = *reinterpret_cast<const float4*>(xr + k0 + 4);
                    float e[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    if (silu) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) e[j] = e[j] / (1.0f + expf(-e[j]));   // torch's silu: x / (1 + exp(-x))
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) af[j] = (int)(FH ? qd_pack2h(e[2 * j], e[2 * j + 1]) : qd_pack2bf(e[2 * j], e[2 * j + 1]));
                }
                const v4i bf = wq_frag<FH>(mag[u], nz);
                if constexpr (FH)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, af), __builtin_bit_cast(v8h, bf), acc, 0, 0, 0);
                else
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, af), __builtin_bit_cast(v8bf, bf), acc, 0, 0, 0);
            }
        }
    }
    if (!nok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                              // C layout: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 half
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        if (m < B) out[(long)m * ldo + L.out_off + n] = qd_wq_affine(acc[r], dl, 0.f, bias);
    }
}

}  // namespace

extern "C" int qd_temb_mlp_wq_h16(const float* x, int64_t ldx, int B, int K, int apply_silu, const void* layers, int n_layers,
                                  const int32_t* blocks, int n_blocks, int wbits, int act_dtype, float* out, int64_t ldo,
                                  void* stream) {
    QD_REQUIRE(x && layers && blocks && out, "qd_temb_mlp_wq_h16: null pointer");
    QD_REQUIRE(B > 0 && K > 0 && n_layers > 0 && n_blocks > 0, "qd_temb_mlp_wq_h16: bad shape (B = %d, K = %d, %d layers, %d blocks)", B, K, n_layers, n_blocks);
    QD_REQUIRE(K % 16 == 0, "qd_temb_mlp_wq_h16: K must be a multiple of 16 (got %d)", K);
    QD_REQUIRE(wbits == 4 || wbits == 8, "qd_temb_mlp_wq_h16: wbits must be 4 or 8");
    QD_REQUIRE(act_dtype == QD_F16 || act_dtype == QD_BF16, "qd_temb_mlp_wq_h16: act_dtype must be f16/bf16");
    QD_REQUIRE(ldx >= K && ldx % 4 == 0 && qd_aligned(x, 16), "qd_temb_mlp_wq_h16: x rows must be 16-byte aligned");
    QD_REQUIRE(ldo > 0, "qd_temb_mlp_wq_h16: bad output row stride");
    const int groups = (B + 31) / 32;                          // 32-row tiles
    QD_REQUIRE(groups <= 65535, "qd_temb_mlp_wq_h16: %d rows need %d row groups of 32 (the grid holds 65535)", B, groups);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto* L = reinterpret_cast<const TembWqLayer*>(layers);
    const auto* bl = reinterpret_cast<const int2*>(blocks);
    const bool fh = act_dtype == QD_F16;
    auto launch = [&](auto wb, auto fh16) {
        hipLaunchKernelGGL((temb_wq_kernel<decltype(wb)::value, decltype(fh16)::value>), dim3(n_blocks, groups), dim3(128), 0, st, x, (long)ldx, B, K,
                           apply_silu, L, bl, out, (long)ldo);
    };
    auto operands = [&](auto wb) { if (fh) launch(wb, std::true_type{}); else launch(wb, std::false_type{}); };
    if (wbits == 4) operands(std::integral_constant<int, 4>{});
    else operands(std::integral_constant<int, 8>{});
    QD_LAUNCH_CHECK("qd_temb_mlp_wq_h16");
    return 0;
}

extern "C" int qd_temb_mlp(const float* x, int64_t ldx, int B, int K, int apply_silu, const void* layers, int n_layers,
                           const int32_t* blocks, int n_blocks, int wbits, int qmin, int qmax, int off, float* out,
                           int64_t ldo, void* stream) {
    QD_REQUIRE(x && layers && blocks && out, "qd_temb_mlp: null pointer");
    QD_REQUIRE(B > 0 && K > 0 && K % 16 == 0 && n_layers > 0 && n_blocks > 0, "qd_temb_mlp: bad shape (K must be a multiple of 16, got %d)", K);
    QD_REQUIRE(wbits == 4 || wbits == 8, "qd_temb_mlp: wbits must be 4 or 8");
    QD_REQUIRE(ldx % 4 == 0 && qd_aligned(x, 16), "qd_temb_mlp: x rows must be 16-byte aligned");
    constexpr int RB = 16;
    // row groups: enough that the launch has about two blocks per CU, at least 4 rows each
    int groups = (512 + n_blocks - 1) / n_blocks;
    if (groups > (B + 3) / 4) groups = (B + 3) / 4;
    if (groups < 1) groups = 1;
    const int rpb = (B + groups - 1) / groups;
    groups = (B + rpb - 1) / rpb;
    const size_t lds = (size_t)rpb * K + (size_t)((rpb + 3) & ~3) * 4 + 4 * RB * 64 * 4;
    QD_REQUIRE(lds <= 64 * 1024, "qd_temb_mlp: %d rows x K = %d do not fit LDS (call it on at most %d rows at a time)", rpb, K, (int)((64 * 1024 - 20000) / K));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto* L = reinterpret_cast<const TembLayer*>(layers);
    const auto* bl = reinterpret_cast<const int2*>(blocks);
    if (wbits == 4)
        hipLaunchKernelGGL((temb_kernel<4, RB>), dim3(n_blocks, groups), dim3(256), lds, st, x, (long)ldx, B, rpb, K, apply_silu, L, bl, (float)qmin, (float)qmax, off, out, (long)ldo);
    else
        hipLaunchKernelGGL((temb_kernel<8, RB>), dim3(n_blocks, groups), dim3(256), lds, st, x, (long)ldx, B, rpb, K, apply_silu, L, bl, (float)qmin, (float)qmax, off, out, (long)ldo);
    QD_LAUNCH_CHECK("qd_temb_mlp");
    return 0;
}
