// wq_h16.hip — the weights-only contraction, its split-K finalise pass and the producer of its operand rows.
// ---------------------------------------------------------------------------------------------
// Weights-only mode (qd_conv2d_wq_h16): fp16 / bf16 activation rows x the tile-ordered int4 / int8 weight CODES of
// qd_pack_weights_t4 / _t8, fp32 accumulation on v_mfma_f32_32x32x16_{f16,bf16}.  This is the reference's
// (weight_quant, act_quant) = (True, False) state of QuantModule.forward (quant_layer.py:620-631: fp conv of the
// fake-quantised weight) without ever materialising that weight:
//     out[m][n] = sum_seg delta_seg[n] * sum_k x[m][k] * (q[k][n] - z_seg[n]) + bias[n] (+ residual[m][n])
// The zero point is subtracted in registers: in the MFMA B layout the output channel is fixed per lane, so z[n] is a
// lane constant.  One 8-byte unit of a t4 tile (16 bytes of a t8 tile) holds the 16 contiguous channels
// cbase .. cbase+15 of one output channel; after the unpack its first and second halves ARE the 8-contiguous-k B
// fragments of two 32x32x16 MFMAs (lane map: k = 8 * (lane >> 5) + j).  A code q becomes the half 1024 + q by the
// 0x6400 | q bit pattern (one v_perm_b32 per two codes), and one v_pk_add_f16 against -(1024 + z) leaves q - z, exact
// in fp16 for |q - z| <= 2048.  bf16 operands go on from that exact fp16 pair (v_cvt_pk_bf16_f32): exact while
// |q - z| <= 256, which the caller guarantees.  (wq_codes.h: the unpack, shared with temb_mlp.hip.)
// Block = 128 x 128 outputs, 4 waves as 2 x 2, wave tile 64 x 64 (MT = NT = 2).  One K-step = 64 channels of one tap of one
// segment: 128 rows x 128 bytes of halves + 4 weight tiles, double-buffered in LDS through registers (the next step's
// global loads are in flight while the current one is contracted; one barrier per step).
// ---------------------------------------------------------------------------------------------
#include "common.h"
#include "wq_codes.h"

namespace {

// the epilogue forms of this file, numbered as igemm_dma.hip numbers its own (O_PART: split-K partial)
enum { O_F32 = 0, O_F16 = 1, O_PART = 4, O_GEGLU_H = 8 };

__device__ __forceinline__ constexpr int crow(int r) { return (r & 3) + 8 * (r >> 2); }   // C-layout row of register r (+ 4*half)

struct WqSeg {
    int c0, clen, kstep0, nst;            // halves; clen % 8 == 0; nst = 64-channel K-steps per tap
    const float* delta;                   // [Cout] delta_w[n]
    const int*   z;                       // [Cout] raw weight zero point z[n]
};

struct WqD {
    const unsigned short* x;              // [B*H*W][ldx] fp16 / bf16 rows
    const uint8_t* wt;
    void* out;
    const void* residual;
    const float* bias;
    const float* rowbias;                 // [B][ldrb] fp32, one row per sample (the timestep-embedding projection), or NULL
    long ldx, ldo;
    // A split-K partial (O_PART) has no residual and no row bias: their leading dimensions carry the slice geometry under names
    // of their own.  The struct keeps its size, so the hidden kernel arguments behind it keep their offsets and the kernels of
    // the unsplit launch their code.
    union { long ldr;  long part_it_per; };                   // O_PART: K-steps per slice
    union { long ldrb; long part_tiles; };                    // O_PART: output tiles per slice
    int H, W, Ho, Wo, Cout, kw, stride, pad_t, pad_l, taps;
    int M, nseg, ntiles, nblk_n;
    WqSeg seg[2];
};

// OUT == O_PART is the split-K form: grid = tiles x nsplit, slice s = block / tiles contracts the global K-steps
// [s * it_per, min((s + 1) * it_per, total)) (order: segment, tap, 64-channel step, as advance() walks them) and writes its
// SCALED partial facc + acc * delta, fp32 without bias / rowbias / residual, to ws[s][m][n] (p.out, row-major [nsplit][M][Cout]);
// wq_splitk_finalize_kernel sums the slices in index order and applies the rest of the epilogue.  No slice is empty (host).
template <int WB, bool FH, bool SPLIT, int OUT>
__global__ __launch_bounds__(256, 2) void wq_h16_kernel(const WqD p) {
    constexpr int MT = 2, NT = 2, BM = 128;
    constexpr bool PART = OUT == O_PART;
    constexpr int TB = 256 * WB;                               // bytes of one (K-step, 32-channel) weight tile
    constexpr int A_BYTES = BM * 128, B_BYTES = 4 * TB, STAGE = A_BYTES + B_BYTES;
    constexpr int NBL = B_BYTES / 4096;                        // 16-byte weight loads per thread per stage
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 31, fhalf = lane >> 5;
    const int lblk = qd_xcd_remap(blockIdx.x, gridDim.x);
    const int it_per = PART ? (int)p.part_it_per : 0, tiles = PART ? (int)p.part_tiles : 1;
    const int slice = PART ? lblk / tiles : 0;
    const int logical = PART ? lblk - slice * tiles : lblk;
    const int mb = logical / p.nblk_n, nb = logical % p.nblk_n;
    const int m0 = mb * BM, n0 = nb * 128;

    // ---- loader: thread -> rows (tid >> 3) + 32 i, 16-byte chunk lq = 8 channels; LDS chunk swizzled by (row & 7) ----
    const int lq = tid & 7;
    const int HoWo = p.Ho * p.Wo;
    long a_pix[4];                                             // first pixel (b, 0, 0) of the row's sample
    int a_ih[4], a_iw[4];
    unsigned a_dst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (tid >> 3) + 32 * i, m = m0 + r;
        const int mm = m < p.M ? m : 0;
        const int b = mm / HoWo, rem = mm - b * HoWo;
        const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
        a_pix[i] = (long)b * p.H * p.W;
        a_ih[i] = m < p.M ? ho * p.stride - p.pad_t : -(1 << 28);   // rows past M read zeros (never inside the image)
        a_iw[i] = wo * p.stride - p.pad_l;
        a_dst[i] = r * 128 + ((lq ^ (r & 7)) * 16);
    }
    int ls = 0, lt = 0, lr = 0, lc = 0, lcs = 0;                // loader position: segment, tap (row, column), K-step
    if constexpr (PART) {                                       // ... of the slice's first global K-step
        int g = slice * it_per;
        const int n0steps = p.taps * p.seg[0].nst;
        if (SPLIT && g >= n0steps) { ls = 1; g -= n0steps; }
        const int nst = p.seg[SPLIT ? ls : 0].nst;
        lt = g / nst; lcs = g - lt * nst;
        lr = lt / p.kw; lc = lt - lr * p.kw;
    }
    v4i ra[4], rb[NBL];
    auto fetch = [&]() __attribute__((always_inline)) {
        const WqSeg& sg = p.seg[SPLIT ? ls : 0];
        const int ch = lcs * 64 + lq * 8;
        const bool cok = ch < sg.clen;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ih = a_ih[i] + lr, iw = a_iw[i] + lc;
            const bool ok = cok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            ra[i] = ok ? *reinterpret_cast<const v4i*>(p.x + (a_pix[i] + (long)ih * p.W + iw) * p.ldx + sg.c0 + ch) : v4i{0, 0, 0, 0};
        }
        const long kstep = sg.kstep0 + (long)lt * sg.nst + lcs;
        const uint8_t* wsrc = p.wt + (kstep * p.ntiles + (long)nb * 4) * TB;
#pragma unroll
        for (int l = 0; l < NBL; ++l) {
            const int byte = (tid + 256 * l) * 16;
            rb[l] = nb * 4 + byte / TB < p.ntiles ? *reinterpret_cast<const v4i*>(wsrc + byte) : v4i{0, 0, 0, 0};
        }
    };
    auto store = [&](unsigned st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<v4i*>(smem + st + a_dst[i]) = ra[i];
#pragma unroll
        for (int l = 0; l < NBL; ++l) *reinterpret_cast<v4i*>(smem + st + A_BYTES + (tid + 256 * l) * 16) = rb[l];
    };
    auto advance = [&]() __attribute__((always_inline)) {
        if (++lcs == p.seg[SPLIT ? ls : 0].nst) {
            lcs = 0;
            if (++lc == p.kw) { lc = 0; ++lr; }
            if (++lt == p.taps) { lt = 0; lr = 0; lc = 0; ++ls; }
        }
    };

    // ---- per-lane constants: the lane's output channel n of each n-tile, per segment ----
    v2h nz[2][NT];
    float dl[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + wn * 64 + j * 32 + frow;
            const bool ok = n < p.Cout && s < p.nseg;
            const int z = ok ? p.seg[s].z[n] : 0;
            const _Float16 h = (_Float16)(float)(-(1024 + z));      // exact: |1024 + z| <= 2048
            nz[s][j] = v2h{h, h};
            dl[s][j] = ok ? p.seg[s].delta[n] : 0.f;
        }

    v16f acc[MT][NT];
    float facc[SPLIT ? MT : 1][SPLIT ? NT : 1][16];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] = 0.f;
                if constexpr (SPLIT) facc[i][j][r] = 0.f;
            }

    const int nst0 = p.taps * p.seg[0].nst;
    const int total = nst0 + (SPLIT ? p.taps * p.seg[1].nst : 0);
    unsigned a_off[MT][4];                                     // [i][g * 2 + u]: A fragment of K-group g, MFMA u
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int gu = 0; gu < 4; ++gu) {
            const int row = wm * 64 + i * 32 + frow;
            const int q = (gu >> 1) * 4 + fhalf * 2 + (gu & 1);
            a_off[i][gu] = row * 128 + ((q ^ (row & 7)) * 16);
        }
    constexpr int UB = 2 * WB;                                 // bytes of one unit (16 codes of one channel)
    const unsigned b_off = A_BYTES + wn * 2 * TB + (fhalf * 32 + frow) * UB;   // + g * 64 * UB + j * TB

    auto compute = [&](unsigned st, int sidx) __attribute__((always_inline)) {
        const unsigned char* S = smem + st;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            v4i af[MT][2];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int u = 0; u < 2; ++u) af[i][u] = *reinterpret_cast<const v4i*>(S + a_off[i][g * 2 + u]);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const unsigned char* bp = S + b_off + g * 64 * UB + j * TB;
                v4i mag[2];
                if constexpr (WB == 4) {
                    const uint2 raw = *reinterpret_cast<const uint2*>(bp);
                    mag[0] = wq_magic<4>(raw.x, 0u);
                    mag[1] = wq_magic<4>(raw.y, 0u);
                } else {
                    const v4i raw = *reinterpret_cast<const v4i*>(bp);
                    mag[0] = wq_magic<8>((unsigned)raw.x, (unsigned)raw.y);
                    mag[1] = wq_magic<8>((unsigned)raw.z, (unsigned)raw.w);
                }
                const v2h z2 = (SPLIT && sidx) ? nz[1][j] : nz[0][j];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const v4i bf = wq_frag<FH>(mag[u], z2);
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        if constexpr (FH)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, af[i][u]), __builtin_bit_cast(v8h, bf),
                                                                                acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, af[i][u]), __builtin_bit_cast(v8bf, bf),
                                                                                 acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
    };

    // the slice's K range — computed HERE, ahead of the prologue fetch: next to `cur` / `nxt` below, hipcc allocates the scalar
    // registers of the fp16-output unsplit instantiations differently (tools/isa_diff.py against the parent then lists them)
    const int it0 = PART ? slice * it_per : 0;
    const int it1 = PART ? (it0 + it_per < total ? it0 + it_per : total) : total;
    fetch();
    store(0);
    advance();
    __syncthreads();
    unsigned cur = 0, nxt = STAGE;
    for (int it = it0; it < it1; ++it) {
        const bool more = it + 1 < it1;
        if (more) fetch();
        compute(cur, SPLIT && it >= nst0 ? 1 : 0);
        if (more) {
            store(nxt);
            advance();
        }
        if constexpr (SPLIT) {
            if (it == nst0 - 1) {                                // segment 0 done: scale it into the fp32 total (flush_segment0)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            facc[i][j][r] = acc[i][j][r] * dl[0][j];
                            acc[i][j][r] = 0.f;
                        }
            }
        }
        __syncthreads();
        const unsigned t = cur; cur = nxt; nxt = t;
    }

    // ---- QD_EPI_GEGLU_H16: the weight rows are 32-column tiles interleaved value, gate, value, ... (geglu_row_perm), so the
    // wave's n-tile j = 0 is a value tile and j = 1 its gate tile: acc[i][0][r] and acc[i][1][r] of one lane are the value and
    // the gate of output feature (n0 + wn * 64) / 2 + frow.  Affine part and GEGLU through the functions qd_conv2d_wq_h16 +
    // qd_geglu_h16 use (common.h), ONE rounding to the operand type.  The wave's 64 x 32 results go through its own region of
    // the LDS ring (idle after the last K-step; rows padded to 80 bytes so that the two half-waves, 4 rows apart, hit
    // different banks) and leave as 16-byte pieces: four per row instead of 32 two-byte stores.  Channels [F, ldo) are
    // written as zeros by the last block of the row of blocks.
    if constexpr (OUT == O_GEGLU_H) {
        static_assert(!SPLIT, "the GEGLU epilogue takes one segment");
        constexpr int GROW = 80;                                // staged row: 64 bytes of results + 16 bytes of padding
        static_assert(4 * 64 * GROW <= 2 * STAGE, "the staged tiles fit the ring");
        unsigned short* const outp = reinterpret_cast<unsigned short*>(p.out);
        const int F = p.Cout >> 1;
        const int ncol = n0 + wn * 64;                          // first (value) column of the wave; Cout % 64 == 0
        unsigned char* const stg = smem + wave * (64 * GROW);
        if (ncol < p.Cout) {
            const float dv = dl[0][0], dg = dl[0][1];
            const float bv = p.bias ? p.bias[ncol + frow] : 0.f, bg = p.bias ? p.bias[ncol + 32 + frow] : 0.f;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float y = qd_geglu_f(qd_wq_affine(acc[i][0][r], dv, 0.f, bv), qd_wq_affine(acc[i][1][r], dg, 0.f, bg));
                    // pin the fp32 rounding of the last product: left alone, the compiler fuses that multiply with the
                    // conversion (v_fma_mixlo_f16: one rounding instead of two) and the fp16 rows are no longer those of
                    // qd_geglu_h16, which converts the rounded fp32 value
                    asm volatile("" : "+v"(y));
                    const unsigned short h = (unsigned short)((FH ? qd_pack2h(y, 0.f) : qd_pack2bf(y, 0.f)) & 0xffffu);
                    *reinterpret_cast<unsigned short*>(stg + (i * 32 + crow(r) + 4 * fhalf) * GROW + frow * 2) = h;
                }
        }
        __syncthreads();
        if (ncol < p.Cout) {
            const int f0 = ncol >> 1;                           // the wave's 32 features start here: 64-byte aligned in the row
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int pc = lane + 64 * t, row = pc >> 2, q = pc & 3;
                const long m = m0 + wm * 64 + row;
                if (m < p.M) *reinterpret_cast<v4i*>(outp + m * p.ldo + f0 + q * 8) = *reinterpret_cast<const v4i*>(stg + row * GROW + q * 16);
            }
        }
        const int npad = (int)((p.ldo - F) >> 3);               // 16-byte pieces of zeros per row
        if (nb == p.nblk_n - 1 && npad > 0) {
            for (int idx = tid; idx < BM * npad; idx += 256) {
                const int row = idx / npad, q = idx - row * npad;
                const long m = m0 + row;
                if (m < p.M) *reinterpret_cast<v4i*>(outp + m * p.ldo + F + q * 8) = v4i{0, 0, 0, 0};
            }
        }
    } else if constexpr (PART) {
    // ---- split-K partial in the C layout.  The live accumulator belongs to segment 1 only when the slice reaches past the
    // boundary; a slice that ends at or before it scales with delta_0 (after a flush acc is 0 and facc is the whole partial).
    float* const ws = reinterpret_cast<float*>(p.out) + (long)slice * p.M * p.Cout;
    const bool seg1 = SPLIT && it1 > nst0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * 64 + j * 32 + frow;
        if (n >= p.Cout) continue;
        const float d = seg1 ? dl[1][j] : dl[0][j];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + wm * 64 + i * 32 + crow(r) + 4 * fhalf;
                if (m >= p.M) continue;
                ws[m * p.Cout + n] = qd_wq_affine(acc[i][j][r], d, SPLIT ? facc[SPLIT ? i : 0][SPLIT ? j : 0][r] : 0.f, 0.f);
            }
    }
    } else {
    // ---- epilogue in the C layout: lane = column, 16 rows per lane; 32 lanes write 32 consecutive columns of a row ----
    const int sl = SPLIT ? 1 : 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * 64 + j * 32 + frow;
        if (n >= p.Cout) continue;
        const float d = dl[sl][j], bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + wm * 64 + i * 32 + crow(r) + 4 * fhalf;
                if (m >= p.M) continue;
                float v = qd_wq_affine(acc[i][j][r], d, SPLIT ? facc[SPLIT ? i : 0][SPLIT ? j : 0][r] : 0.f, bias);
                if (p.rowbias) v += p.rowbias[((int)m / HoWo) * p.ldrb + n];
                if constexpr (OUT == O_F32) {
                    if (p.residual) v += reinterpret_cast<const float*>(p.residual)[m * p.ldr + n];
                    reinterpret_cast<float*>(p.out)[m * p.ldo + n] = v;
                } else {
                    if (p.residual) v += __half2float(reinterpret_cast<const __half*>(p.residual)[m * p.ldr + n]);
                    reinterpret_cast<__half*>(p.out)[m * p.ldo + n] = __float2half(v);
                }
            }
    }
    }
}

// fp32 / fp16 / bf16 logical [B][C][S] (element strides sb, sc, ss) -> fp16 / bf16 rows out[(b*S+s)*ldo + oc0 + c - c0] for
// channels [c0, c0+clen), zeros up to clen_pad.  Thread = (row, 8 channels); sfast: threads run along S first (NCHW input:
// coalesced reads), else along the channel groups (channels-last input and the output rows: coalesced both ways).
template <typename TI>
__device__ __forceinline__ float wq_ld(const TI* p);
template <> __device__ __forceinline__ float wq_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float wq_ld<__half>(const __half* p) { return __half2float(*p); }
template <> __device__ __forceinline__ float wq_ld<unsigned short>(const unsigned short* p) { return qd_bf2f(*p); }

template <typename TI>
__global__ __launch_bounds__(256) void rows_h16_kernel(const TI* __restrict__ x, long S, long sb, long sc, long ss, int c0, int clen,
                                                       int G, long total, unsigned short* __restrict__ out, long ldo, int oc0,
                                                       int fh, int sfast) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    long s, b;
    int g;
    if (sfast) { s = gid % S; const long rest = gid / S; g = (int)(rest % G); b = rest / G; }
    else { g = (int)(gid % G); const long rest = gid / G; s = rest % S; b = rest / S; }
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = g * 8 + e;
        f[e] = c < clen ? wq_ld<TI>(x + b * sb + (long)(c0 + c) * sc + s * ss) : 0.f;
    }
    v4i pk;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk[e] = fh ? (int)qd_pack2h(f[2 * e], f[2 * e + 1]) : (int)qd_pack2bf(f[2 * e], f[2 * e + 1]);
    *reinterpret_cast<v4i*>(out + (b * S + s) * ldo + oc0 + g * 8) = pk;
}

// split-K second pass of the weights-only contraction: sums the scaled fp32 partials ws[s][m][n] in slice order (no atomics:
// the same bits from run to run), then bias, rowbias[m / HoWo] and residual in the order and through the functions of the
// unsplit epilogue.  VEC: thread = 4 consecutive columns (16-byte partial / bias / rowbias lanes; fp32 rows leave as 16 bytes,
// fp16 rows as 8), chosen by the host when Cout, the leading dimensions and every pointer allow; else thread = one element.
template <int OUT, bool VEC>
__global__ __launch_bounds__(256) void wq_splitk_finalize_kernel(const float* __restrict__ ws, int nsplit, long M, int Cout, int HoWo,
                                                                 const float* __restrict__ bias, const float* __restrict__ rowbias,
                                                                 long ldrb, const void* __restrict__ residual, long ldr,
                                                                 void* __restrict__ out, long ldo) {
    constexpr int V = VEC ? 4 : 1;
    const long MN = M * Cout;
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= MN) return;
    const long m = e / Cout;
    const int  n = (int)(e - m * Cout);
    float v[V];
    if constexpr (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(ws + e);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        for (int s = 1; s < nsplit; ++s) {
            const float4 b = *reinterpret_cast<const float4*>(ws + (long)s * MN + e);
            v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
        }
    } else {
        v[0] = ws[e];
        for (int s = 1; s < nsplit; ++s) v[0] += ws[(long)s * MN + e];
    }
    const float* rb = rowbias ? rowbias + (m / HoWo) * ldrb + n : nullptr;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        v[c] = qd_wq_affine(v[c], 1.f, 0.f, bias ? bias[n + c] : 0.f);
        if (rb) v[c] += rb[c];
    }
    if constexpr (OUT == O_F32) {
        const float* r = reinterpret_cast<const float*>(residual);
        float* o = reinterpret_cast<float*>(out) + m * ldo + n;
        if (r) {
#pragma unroll
            for (int c = 0; c < V; ++c) v[c] += r[m * ldr + n + c];
        }
        if constexpr (VEC) *reinterpret_cast<float4*>(o) = float4{v[0], v[1], v[2], v[3]};
        else *o = v[0];
    } else {
        const __half* r = reinterpret_cast<const __half*>(residual);
        __half* o = reinterpret_cast<__half*>(out) + m * ldo + n;
        if (r) {
#pragma unroll
            for (int c = 0; c < V; ++c) v[c] += __half2float(r[m * ldr + n + c]);
        }
        if constexpr (VEC) {
            union { __half h[4]; uint2 u; } pk;
#pragma unroll
            for (int c = 0; c < 4; ++c) pk.h[c] = __float2half(v[c]);
            *reinterpret_cast<uint2*>(o) = pk.u;
        } else {
            *o = __float2half(v[0]);
        }
    }
}

// qd_wq_h16_config: -1 = policy, 0 = never split, n >= 2 = force n slices
static int& wq_splitk_knob() {
    static int v = -1;
    return v;
}

// Split-K policy of qd_conv2d_wq_h16, next to choose_splitk of the integer path.  Both segment counts; never
// the GEGLU epilogue (its M x 2F grids fill the chip, and a finalise could not keep its one rounding).  No slice is empty:
// nsplit = ceil(total / it_per).
int choose_wq_splitk(const qd_conv_desc* d, int* it_per) {
    // blocks the split should reach and the fewest K-steps a slice may hold.  PROVISIONAL: the integer path's target of one block per
    // CU and a guess at the slice length; no timing backs either yet
    constexpr long kTarget = 256, kMinSteps = 8;
    *it_per = 0;
    const int forced = wq_splitk_knob();
    if (forced == 0 || d->epilogue != QD_EPI_LINEAR || (d->nseg != 1 && d->nseg != 2)) return 1;
    const long M = (long)d->B * d->Ho * d->Wo;
    const long tiles = ((M + 127) / 128) * (((long)d->Cout + 127) / 128);
    long total = 0;
    for (int s = 0; s < d->nseg; ++s) total += (long)d->kh * d->kw * ((d->seg[s].clen + 63) / 64);
    if (M <= 0 || d->Cout <= 0 || total < 2) return 1;
    long S;
    if (forced >= 2) {
        S = forced < total ? forced : total;
    } else {
        if (total < 4 * kMinSteps) return 1;                       // a second launch is a fixed cost a short K loop cannot pay back
        S = kTarget / tiles;                                       // < 2: the plain launch already reaches half the target
        if (S > total / kMinSteps) S = total / kMinSteps;
        if (S > 32) S = 32;
    }
    if (S < 2 || tiles * S >= (1L << 31)) return 1;
    *it_per = (int)((total + S - 1) / S);
    return (int)((total + *it_per - 1) / *it_per);
}

// One call of the contraction as a plain value: plan_wq() fills it without a HIP call, launch_wq() issues it.
struct WqLaunch {
    WqD      k;              // the contraction's descriptor.  Sliced: out = the workspace, no bias / rowbias / residual, part_it_per / part_tiles set
    int      wb;             // wq_h16_kernel<wb, fh, split, out>
    bool     fh, split;      // fp16 (else bf16) operands; two segments
    int      out;            // O_F32 / O_F16 / O_GEGLU_H, sliced: O_PART
    unsigned grid;           // tiles, sliced: tiles x nsplit
    int      nsplit;         // K slices; >= 2: wq_splitk_finalize_kernel<rows, vec> follows, with the arguments below
    int      rows;           // the call's epilogue form, O_F32 / O_F16 / O_GEGLU_H (= out unless sliced)
    bool     vec;            // sliced: Cout, the leading dimensions and every pointer allow four columns per thread
    unsigned fin_grid;
    const float *bias, *rowbias;
    const void*  residual;
    void*        dst;
    long         ldrb, ldr, ldo;
};

// Every refusal of qd_conv2d_wq_h16, the kernel's descriptor and the slicing decision.  A launch is sliced only when the caller lent a
// workspace, the policy wants >= 2 slices and the workspace holds them; otherwise it is the one launch, silently.
int plan_wq(const qd_conv_desc* d, int act_dtype, WqLaunch* L) {
    QD_REQUIRE(d != nullptr, "qd_conv2d_wq_h16: null descriptor");
    QD_REQUIRE(d->x && d->w && d->out, "qd_conv2d_wq_h16: null tensor pointer");
    QD_REQUIRE(d->res_period == 0, "qd_conv2d_wq_h16: res_period is not supported (qd_conv2d_i8 with the linear epilogue only)");
    QD_REQUIRE(act_dtype == QD_F16 || act_dtype == QD_BF16, "qd_conv2d_wq_h16: act_dtype must be QD_F16 or QD_BF16");
    QD_REQUIRE(d->w_tiled && (d->wbits == 4 || d->wbits == 8), "qd_conv2d_wq_h16: weights must be tile-ordered codes of qd_pack_weights_t4 / _t8 (w_tiled = 1, wbits 4 / 8)");
    QD_REQUIRE(d->out_dtype == QD_F32 || d->out_dtype == QD_F16 || d->epilogue == QD_EPI_GEGLU_H16, "qd_conv2d_wq_h16: out_dtype must be f32/f16");
    QD_REQUIRE(d->nseg == 1 || d->nseg == 2, "qd_conv2d_wq_h16: nseg must be 1 or 2");
    const bool geglu = d->epilogue == QD_EPI_GEGLU_H16;
    QD_REQUIRE((d->epilogue == QD_EPI_LINEAR || geglu) && !d->gn_part && !d->upsample2x,
               "qd_conv2d_wq_h16: linear epilogue only (no GroupNorm statistics or up-sampling)");
    if (geglu) {                                               // out = operand rows [M][ldo] of value * gelu(gate), F = Cout / 2
        QD_REQUIRE(d->nseg == 1 && d->Cout % 64 == 0, "qd_conv2d_wq_h16: GEGLU epilogue: one segment, Cout = 2 F with F %% 32 == 0 (Cout=%d)", d->Cout);
        QD_REQUIRE(d->out_dtype == act_dtype, "qd_conv2d_wq_h16: GEGLU epilogue: out_dtype must be act_dtype (operand rows)");
        QD_REQUIRE(d->residual == nullptr && d->rowbias == nullptr, "qd_conv2d_wq_h16: GEGLU epilogue takes no residual and no rowbias");
        QD_REQUIRE(d->ldo >= d->Cout / 2 && d->ldo % 8 == 0 && qd_aligned(d->out, 16),
                   "qd_conv2d_wq_h16: GEGLU epilogue: out rows must be 16-byte aligned with ldo %% 8 == 0 and ldo >= F");
    }
    QD_REQUIRE(!d->rowbias || d->ld_rowbias >= d->Cout, "qd_conv2d_wq_h16: ld_rowbias shorter than Cout");
    QD_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->Cout > 0, "qd_conv2d_wq_h16: bad shape");
    QD_REQUIRE(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->kh * d->kw <= 32, "qd_conv2d_wq_h16: bad kernel/stride (at most 32 taps)");
    QD_REQUIRE(d->pad_t >= 0 && d->pad_l >= 0 && d->pad_t < 64 && d->pad_l < 64, "qd_conv2d_wq_h16: bad padding");
    QD_REQUIRE((long)d->B * d->Ho * d->Wo < (1L << 31), "qd_conv2d_wq_h16: M overflows int32");
    QD_REQUIRE(d->ldx % 8 == 0 && qd_aligned(d->x, 16) && qd_aligned(d->w, 16), "qd_conv2d_wq_h16: x/w must be 16-byte aligned, ldx %% 8 == 0");
    QD_REQUIRE((geglu || d->ldo >= d->Cout) && (!d->residual || d->ldr >= d->Cout), "qd_conv2d_wq_h16: ldo / ldr shorter than Cout");
    WqD k{};
    k.x = reinterpret_cast<const unsigned short*>(d->x); k.wt = d->w; k.out = d->out; k.residual = d->residual; k.bias = d->bias;
    k.rowbias = d->rowbias; k.ldrb = d->ld_rowbias;
    k.ldx = d->ldx; k.ldo = d->ldo; k.ldr = d->ldr;
    k.H = d->H; k.W = d->W; k.Ho = d->Ho; k.Wo = d->Wo; k.Cout = d->Cout;
    k.kw = d->kw; k.stride = d->stride; k.pad_t = d->pad_t; k.pad_l = d->pad_l; k.taps = d->kh * d->kw;
    k.M = d->B * d->Ho * d->Wo; k.nseg = d->nseg; k.ntiles = (d->Cout + 31) / 32;
    for (int s = 0; s < d->nseg; ++s) {
        const qd_conv_seg& g = d->seg[s];
        QD_REQUIRE(g.clen > 0 && g.clen % 8 == 0 && g.c0 % 8 == 0 && g.c0 >= 0 && g.c0 + g.clen <= d->ldx,
                   "qd_conv2d_wq_h16: segment %d c0/clen must be multiples of 8 inside the row", s);
        QD_REQUIRE(g.scale && g.zw, "qd_conv2d_wq_h16: segment %d needs scale (delta_w) and zw (raw zero points)", s);
        QD_REQUIRE(!g.zc && !g.zfill && !g.fill16, "qd_conv2d_wq_h16: segment %d: zc / zfill / fill16 must be NULL", s);
        k.seg[s] = WqSeg{g.c0, g.clen, g.kstep0, (g.clen + 63) / 64, g.scale, g.zw};
    }
    const long M = k.M, N = d->Cout;
    const long nbm = (M + 127) / 128, nbn = (N + 127) / 128;
    QD_REQUIRE(nbm * nbn < (1L << 31), "qd_conv2d_wq_h16: too many tiles");
    k.nblk_n = (int)nbn;
    *L = WqLaunch{};
    L->wb = d->wbits; L->fh = act_dtype == QD_F16; L->split = d->nseg == 2;
    L->out = L->rows = geglu ? O_GEGLU_H : d->out_dtype == QD_F16 ? O_F16 : O_F32;
    L->grid = (unsigned)(nbm * nbn);
    L->nsplit = 1;
    int it_per = 0;
    const int nsplit = d->splitk_ws ? choose_wq_splitk(d, &it_per) : 1;
    if (nsplit >= 2 && d->splitk_ws_bytes >= (int64_t)nsplit * M * N * 4) {
        QD_REQUIRE(qd_aligned(d->splitk_ws, 16), "qd_conv2d_wq_h16: splitk_ws must be 16-byte aligned");
        const int esz = L->rows == O_F16 ? 2 : 4;
        L->vec = N % 4 == 0 && d->ldo % 4 == 0 && qd_aligned(d->out, 4 * esz) && (!d->bias || qd_aligned(d->bias, 16)) &&
                 (!d->rowbias || (qd_aligned(d->rowbias, 16) && d->ld_rowbias % 4 == 0)) &&
                 (!d->residual || (qd_aligned(d->residual, 4 * esz) && d->ldr % 4 == 0));
        L->fin_grid = (unsigned)(((L->vec ? M * N / 4 : M * N) + 255) / 256);
        L->bias = d->bias; L->rowbias = d->rowbias; L->ldrb = d->ld_rowbias; L->residual = d->residual; L->ldr = d->ldr;
        L->dst = d->out; L->ldo = d->ldo;
        k.out = d->splitk_ws; k.part_it_per = it_per; k.part_tiles = nbm * nbn; k.residual = nullptr; k.rowbias = nullptr; k.bias = nullptr;
        L->out = O_PART;
        L->grid = (unsigned)(nbm * nbn * nsplit);
        L->nsplit = nsplit;
    }
    L->k = k;
    return 0;
}

template <int WB_, bool FH_>
struct WqOp { static constexpr int WB = WB_; static constexpr bool FH = FH_; };
template <bool FLAG_, int OUT_>
struct WqForm { static constexpr bool FLAG = FLAG_; static constexpr int OUT = OUT_; };   // FLAG: two segments (contraction) / four columns per thread (finalise)
// THE lists of built kernels: f(WqOp<...>{}, WqForm<...>{}) for the contraction the tuple names, f(WqForm<...>{}) for the finalise
// form; false if the library has none such.
template <class F>
bool visit_wq(int wb, bool fh, bool split, int out, F f) {
    auto forms = [&](auto op) {
        auto among = [&](auto... v) { return ((decltype(v)::FLAG == split && decltype(v)::OUT == out && (f(op, v), true)) || ...); };
        return among(WqForm<false, O_F32>{}, WqForm<false, O_F16>{}, WqForm<true, O_F32>{}, WqForm<true, O_F16>{}, WqForm<false, O_PART>{},
                     WqForm<true, O_PART>{}, WqForm<false, O_GEGLU_H>{});
    };
    auto ops = [&](auto... op) { return ((decltype(op)::WB == wb && decltype(op)::FH == fh && forms(op)) || ...); };
    return ops(WqOp<4, true>{}, WqOp<4, false>{}, WqOp<8, true>{}, WqOp<8, false>{});
}
template <class F>
bool visit_wq_finalize(int rows, bool vec, F f) {
    auto among = [&](auto... v) { return ((decltype(v)::FLAG == vec && decltype(v)::OUT == rows && (f(v), true)) || ...); };
    return among(WqForm<true, O_F32>{}, WqForm<false, O_F32>{}, WqForm<true, O_F16>{}, WqForm<false, O_F16>{});
}

// The only place that launches wq_h16_kernel and wq_splitk_finalize_kernel: the plan's contraction, or (finalise) the pass over its slices.
int launch_wq(const WqLaunch& L, bool finalise, hipStream_t st) {
    const WqD& k = L.k;
    bool done;
    if (!finalise)
        done = visit_wq(L.wb, L.fh, L.split, L.out, [&](auto op, auto v) {
            using Op = decltype(op);
            using V = decltype(v);
            hipLaunchKernelGGL((wq_h16_kernel<Op::WB, Op::FH, V::FLAG, V::OUT>), dim3(L.grid), dim3(256), 0, st, k);
        });
    else
        done = L.nsplit >= 2 && visit_wq_finalize(L.rows, L.vec, [&](auto v) {
            using V = decltype(v);
            hipLaunchKernelGGL((wq_splitk_finalize_kernel<V::OUT, V::FLAG>), dim3(L.fin_grid), dim3(256), 0, st, reinterpret_cast<const float*>(k.out),
                               L.nsplit, (long)k.M, k.Cout, k.Ho * k.Wo, L.bias, L.rowbias, L.ldrb, L.residual, L.ldr, L.dst, L.ldo);
        });
    QD_REQUIRE(done, "qd_conv2d_wq_h16: the launch plan names no built kernel (wbits %d, fh=%d, split=%d, out=%d, rows=%d, %d slices%s)", L.wb,
               (int)L.fh, (int)L.split, L.out, L.rows, L.nsplit, finalise ? ", finalise" : "");
    return 0;
}

int run_wq_h16(const qd_conv_desc* d, int act_dtype, void* stream) {
    WqLaunch L;
    if (const int rc = plan_wq(d, act_dtype, &L)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = launch_wq(L, false, st)) return rc;
    if (L.nsplit < 2) {
        QD_LAUNCH_CHECK("qd_conv2d_wq_h16");
        return 0;
    }
    QD_LAUNCH_CHECK("qd_conv2d_wq_h16 (split-K)");
    if (const int rc = launch_wq(L, true, st)) return rc;
    QD_LAUNCH_CHECK("qd_conv2d_wq_h16 (split-K finalise)");
    return 0;
}

}  // namespace

extern "C" int qd_conv2d_wq_h16(const qd_conv_desc* d, int act_dtype, void* stream) { return run_wq_h16(d, act_dtype, stream); }

// The launch form qd_conv2d_wq_h16(d, act_dtype) would take now: its plan.
extern "C" int qd_conv2d_wq_h16_form(const qd_conv_desc* d, int act_dtype, int32_t* form4) {
    QD_REQUIRE(form4 != nullptr, "qd_conv2d_wq_h16_form: null form4");
    WqLaunch L;
    if (const int rc = plan_wq(d, act_dtype, &L)) return rc;
    const bool sliced = L.nsplit >= 2;
    form4[0] = L.nsplit; form4[1] = sliced ? (int)L.k.part_it_per : 0;
    form4[2] = L.rows == O_GEGLU_H ? 2 : L.rows == O_F16 ? 1 : 0; form4[3] = sliced && L.vec ? 1 : 0;
    return 0;
}

extern "C" int64_t qd_conv2d_wq_h16_splitk_ws_bytes(const qd_conv_desc* d) {
    if (!d) return 0;
    int it_per;
    const int S = choose_wq_splitk(d, &it_per);
    return S < 2 ? 0 : (int64_t)S * d->B * d->Ho * d->Wo * d->Cout * 4;
}

extern "C" void qd_wq_h16_config(int splitk) { wq_splitk_knob() = splitk < 0 ? -1 : (splitk == 1 ? 0 : splitk); }

extern "C" int qd_rows_to_h16(const void* x, int x_dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                              int c0, int clen, int clen_pad, void* out, int out_dtype, int64_t ldo, int oc0, void* stream) {
    QD_REQUIRE(x && out, "qd_rows_to_h16: null pointer");
    QD_REQUIRE(x_dtype == QD_F32 || x_dtype == QD_F16 || x_dtype == QD_BF16, "qd_rows_to_h16: x_dtype must be f32/f16/bf16");
    QD_REQUIRE(out_dtype == QD_F16 || out_dtype == QD_BF16, "qd_rows_to_h16: out_dtype must be f16/bf16");
    QD_REQUIRE(B > 0 && C > 0 && S > 0 && c0 >= 0 && clen > 0 && c0 + clen <= C, "qd_rows_to_h16: bad shape / channel range");
    QD_REQUIRE(clen_pad >= clen && clen_pad % 8 == 0 && oc0 % 8 == 0 && oc0 >= 0 && oc0 + clen_pad <= ldo && ldo % 8 == 0 && qd_aligned(out, 16),
               "qd_rows_to_h16: clen_pad / oc0 / ldo must be multiples of 8 inside the row, out 16-byte aligned");
    const int G = clen_pad / 8;
    const long total = (long)B * S * G;
    const int sfast = ss == 1 && sc != 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    unsigned short* o = reinterpret_cast<unsigned short*>(out);
    const int fh = out_dtype == QD_F16;
    auto launch = [&](auto* xt) {                              // xt: x in its element type (bf16 as unsigned short)
        hipLaunchKernelGGL(rows_h16_kernel<std::remove_cv_t<std::remove_pointer_t<decltype(xt)>>>, grid, block, 0, st, xt, (long)S, (long)sb, (long)sc,
                           (long)ss, c0, clen, G, total, o, (long)ldo, oc0, fh, sfast);
    };
    if (x_dtype == QD_F32) launch(reinterpret_cast<const float*>(x));
    else if (x_dtype == QD_F16) launch(reinterpret_cast<const __half*>(x));
    else launch(reinterpret_cast<const unsigned short*>(x));
    QD_LAUNCH_CHECK("qd_rows_to_h16");
    return 0;
}

