// attn_h16.hip — fused fp16 / bf16 attention for the weights-only state (weight_quant, act_quant) = (True, False).
//
// Replaces (reference qdiff/quant_block.py:190-221 with use_act_quant False, and the legacy attention
// ldm/modules/diffusionmodules/openaimodel.py:373-406): einsum(q, k) -> * scale -> fp32 softmax -> einsum(P, v), four
// library passes over a T x S fp32 score matrix.  Here one flash-style sweep per query block: online row maximum and sum,
// O rescaled when the maximum moves, one normalisation in the epilogue; the score matrix never leaves the registers.
//
// Layout (the orientation of attn_i8.hip):
//   * one wave owns 32 queries, a block of 4 waves 128 queries of one (b, h); blocks of one head are consecutive logical ids,
//     remapped so that they share an XCD (qd_xcd_remap, as QD_ATTN_XCD does for the integer kernel);
//   * scores are computed TRANSPOSED on v_mfma_f32_32x32x16_{f16,bf16}: A = 32 keys x 16 channels (LDS), B = the wave's
//     query fragment (registers, loaded once).  The C layout leaves every lane with ONE query (lane & 31) and 16 of the 32
//     keys of the tile: row max / row sum are lane-local plus one v_permlane32_swap with the other half-wave;
//   * P goes into the P.V MFMA without leaving the lane: registers 8s..8s+7 of the score tile, converted pairwise to the
//     operand type, are the B fragment of k-step s of O^T = V^T . P^T (cdna_hip_programming.md §3 "An accumulator tile as
//     the next MFMA's operand").  The k order inside a step is permuted (element j of half h is key 16s + 8(j>>2) + 4h + (j&3)),
//     so V^T is written to LDS in that key order and the A fragment is one ds_read_b128;
//   * O^T keeps the query on the lane too, so the rescale factor of a row is lane-local: O *= alpha is 16 * NT multiplies,
//     skipped (wave-uniform) on tiles where no row maximum of the wave moved — an exact rescale, no deferred maximum (T13);
//   * K / V tiles of 32 keys are register-staged (T14: the next tile's global loads are issued before this tile's MFMAs and
//     written to the other half of a double-buffered LDS ring after them; one barrier per tile).  The staging converts the
//     fp32 / fp16 / bf16 input (a template parameter) to the operand type, reading runs of 8 channels of any (b, token, head)
//     strides with channel stride 1: no host-side head split or cast.
//   * LDS rows have an ODD number of 16-byte chunks (K: 2*DK + 1, V^T: 5), which makes every ds_read_b128 lane group of the
//     fragment reads conflict-free (rows r mod 16 of a group are distinct); the row lengths (48, 80, 160 halves) are not
//     powers of two, so this padding replaces the XOR swizzle of the integer kernel.
// Padding: scores contract over d padded to 16 (DK = d/16 k-steps: d = 40 -> 48, 17 % idle), P.V produces 32-channel
// tiles (NT = ceil(d / 32): d = 40 -> 64, 37 % of the P.V MFMAs idle, d = 80 -> 96, 17 %).  DESIGN.md §4.13 records why the
// 16x16x32 form does not take the P.V side here.
#include "common.h"
#include <cmath>

namespace {

struct AttnH {
    const char* q;
    const char* k;
    const char* v;
    long qs[3], ks[3], vs[3];     // element strides (b, token, head); the channel stride is 1
    void* out;
    long ldo;
    int T, S, H, d, gx, nblk;
    float c2;                     // scale * log2(e)
    int out_f16;
};

struct Raw8 { v4i a, b; };        // 8 input elements as loaded: fp32 -> a, b; fp16 / bf16 -> a

// 8 consecutive channels (element offset `off`, channel stride 1, 16-byte aligned) of an fp32 / fp16 / bf16 tensor; zeros when !ok
template <int DT>
__device__ __forceinline__ Raw8 ah_load8(const char* base, long off, bool ok) {
    Raw8 r{{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (!ok) return r;
    if constexpr (DT == QD_F32) {
        const float* p = reinterpret_cast<const float*>(base) + off;
        r.a = *reinterpret_cast<const v4i*>(p);
        r.b = *reinterpret_cast<const v4i*>(p + 4);
    } else {
        r.a = *reinterpret_cast<const v4i*>(reinterpret_cast<const unsigned short*>(base) + off);
    }
    return r;
}

template <int DT>
__device__ __forceinline__ float ah_elem(const Raw8& r, int j) {
    if constexpr (DT == QD_F32) return __int_as_float(j < 4 ? r.a[j] : r.b[j - 4]);
    const unsigned w = (unsigned)r.a[j >> 1];
    const unsigned short h = (unsigned short)((j & 1) ? (w >> 16) : (w & 0xffffu));
    if constexpr (DT == QD_BF16) return qd_bf2f(h);
    return (float)__builtin_bit_cast(_Float16, h);
}

template <bool BF>
__device__ __forceinline__ unsigned ah_pack2(float x, float y) {
    if constexpr (BF) return qd_pack2bf(x, y);
    else {
        const _Float16 a = (_Float16)x, b = (_Float16)y;       // round to nearest even
        return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
    }
}

// 8 elements -> 8 operand halves (4 dwords); a 16-bit input of the operand type is passed through unchanged
template <bool BF, int DT>
__device__ __forceinline__ v4i ah_convert(const Raw8& r) {
    if constexpr (DT == (BF ? QD_BF16 : QD_F16)) return r.a;
    v4i o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (int)ah_pack2<BF>(ah_elem<DT>(r, 2 * j), ah_elem<DT>(r, 2 * j + 1));
    return o;
}

template <bool BF>
__device__ __forceinline__ v16f ah_mfma(const v4i& a, const v4i& b, const v16f& c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

// value of the same query row held by the other half-wave (lane ^ 32) combined with this lane's: {x, other} in some order
__device__ __forceinline__ float ah_max_halves(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float ah_sum_halves(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// LDS position of key `kk` (0..31) inside a V^T row: the k order of the P fragments (see the header)
__device__ __forceinline__ int ah_vpos(int kk) {
    const int s = kk >> 4, rem = kk & 15;
    return 16 * s + 8 * ((rem >> 2) & 1) + 4 * (rem >> 3) + (rem & 3);
}

// Head dims up to 160 (DK <= 10) run two blocks per CU.  The wide ones (DK = 11 .. 16, d = 168 .. 256: the one-head attention of the
// DDIM UNet) fill the register file at one wave per SIMD — the query fragment is 4 DK registers, the O^T tiles
// 16 NT — hence the launch bounds; the body is the same.
template <bool BF, int DK, int DT>
__global__ __launch_bounds__(256, DK > 10 ? 1 : 2) void attn_h16_kernel(const AttnH p) {
    constexpr int NT = (DK + 1) / 2;                           // 32-channel output tiles
    constexpr int KC = 2 * DK + 1;                             // 16-byte chunks per K row (odd: conflict-free reads)
    constexpr int VC = 5;                                      // 16-byte chunks per V^T row (32 keys = 4, + 1)
    constexpr int KB = 32 * KC * 16, VB = 32 * NT * VC * 16, STAGE = KB + VB;
    constexpr int NKU = 64 * DK, NVU = 64 * NT;                // staging units: K (key, 8 channels), V (key pair, 8 channels)
    constexpr int KU = (NKU + 255) / 256, VU = (NVU + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 31, half = lane >> 5;
    const int lblk = qd_xcd_remap(blockIdx.x, p.nblk);
    const int bh = lblk / p.gx, qb = lblk - bh * p.gx;
    const int b = bh / p.H, hh = bh - b * p.H;
    const int qi = qb * 128 + wave * 32 + frow;                // this lane's query
    const int d = p.d, S = p.S;

    // ---- query fragment: channels 16kk + 8*half .. +7 of query qi (B operand of the score MFMA) ----
    v4i qf[DK];
    {
        const long qoff = (long)b * p.qs[0] + (long)qi * p.qs[1] + (long)hh * p.qs[2];
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
            const int c = 16 * kk + 8 * half;
            qf[kk] = ah_convert<BF, DT>(ah_load8<DT>(p.q, qoff + c, qi < p.T && c < d));
        }
    }

    const long kbase = (long)b * p.ks[0] + (long)hh * p.ks[2];
    const long vbase = (long)b * p.vs[0] + (long)hh * p.vs[2];
    Raw8 kr[KU], vr[VU][2];
    auto issue = [&](int jt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int idx = tid + 256 * u;
            const int key = jt * 32 + (idx & 31), c = 8 * (idx >> 5);
            kr[u] = ah_load8<DT>(p.k, kbase + (long)key * p.ks[1] + c, idx < NKU && key < S && c < d);
        }
#pragma unroll
        for (int u = 0; u < VU; ++u) {
            const int idx = tid + 256 * u;
            const int key = jt * 32 + 2 * (idx & 15), c = 8 * (idx >> 4);
            const bool ok = idx < NVU && c < d;
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
        for (int u = 0; u < KU; ++u) {
            const int idx = tid + 256 * u;
            if (idx < NKU) *reinterpret_cast<v4i*>(ks + (idx & 31) * (KC * 16) + (idx >> 5) * 16) = ah_convert<BF, DT>(kr[u]);
        }
#pragma unroll
        for (int u = 0; u < VU; ++u) {
            const int idx = tid + 256 * u;
            if (idx < NVU) {
                const v4i c0 = ah_convert<BF, DT>(vr[u][0]), c1 = ah_convert<BF, DT>(vr[u][1]);
                unsigned char* row = vs + (8 * (idx >> 4)) * (VC * 16) + ah_vpos(2 * (idx & 15)) * 2;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned w = __builtin_amdgcn_perm((unsigned)c1[i >> 1], (unsigned)c0[i >> 1], (i & 1) ? 0x07060302u : 0x05040100u);
                    *reinterpret_cast<unsigned*>(row + i * (VC * 16)) = w;
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
    v16f o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;

    for (int jt = 0; jt < ntile; ++jt) {
        const unsigned char* ks = smem + (jt & 1) * STAGE;
        const unsigned char* vs = ks + KB;
        const bool more = jt + 1 < ntile;
        if (more) issue(jt + 1);

        // ---- S^T tile: acc[r] = score(query qi, key jt*32 + (r&3) + 8(r>>2) + 4*half) ----
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
            const v4i kf = *reinterpret_cast<const v4i*>(ks + frow * (KC * 16) + (2 * kk + half) * 16);
            acc = ah_mfma<BF>(kf, qf[kk], acc);
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
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
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

        // ---- O^T += V^T . P^T ----
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v4i vf = *reinterpret_cast<const v4i*>(vs + (32 * t + frow) * (VC * 16) + (2 * s + half) * 16);
                o[t] = ah_mfma<BF>(vf, pf[s], o[t]);
            }

        if (more) commit((jt + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: normalise, store merged-head rows out[b*T + qi][hh*d + c] ----
    const float inv = 1.0f / ah_sum_halves(l);
    if (qi >= p.T) return;
    const long row = ((long)b * p.T + qi) * p.ldo + (long)hh * d;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * t + 8 * g + 4 * half;           // registers 4g .. 4g+3: channels c .. c+3
            if (c >= d) continue;
            const float y0 = o[t][4 * g] * inv, y1 = o[t][4 * g + 1] * inv, y2 = o[t][4 * g + 2] * inv, y3 = o[t][4 * g + 3] * inv;
            if (p.out_f16) {
                uint2 w;
                w.x = ah_pack2<false>(y0, y1);
                w.y = ah_pack2<false>(y2, y3);
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.out) + row + c) = w;
            } else {
                *reinterpret_cast<v4f*>(reinterpret_cast<float*>(p.out) + row + c) = v4f{y0, y1, y2, y3};
            }
        }
}

template <bool BF, int DT>
void launch_h16(const AttnH& a, int DK, dim3 grid, hipStream_t st) {
    switch (DK) {
#define QD_AH(N) case N: hipLaunchKernelGGL((attn_h16_kernel<BF, N, DT>), grid, dim3(256), 0, st, a); break;
        QD_AH(1) QD_AH(2) QD_AH(3) QD_AH(4) QD_AH(5) QD_AH(6) QD_AH(7) QD_AH(8) QD_AH(9) QD_AH(10)
        QD_AH(11) QD_AH(12) QD_AH(13) QD_AH(14) QD_AH(15) QD_AH(16)
#undef QD_AH
    }
}

template <bool BF>
void launch_h16_in(const AttnH& a, int in_dtype, int DK, dim3 grid, hipStream_t st) {
    if (in_dtype == QD_F32) launch_h16<BF, QD_F32>(a, DK, grid, st);
    else if (in_dtype == QD_F16) launch_h16<BF, QD_F16>(a, DK, grid, st);
    else launch_h16<BF, QD_BF16>(a, DK, grid, st);
}

// runs of 8 channels are read as 16- / 32-byte vectors: channel stride 1, every run 16-byte aligned
bool ah_layout_ok(const void* base, int dt, int64_t sb, int64_t st, int64_t sh, int64_t sd) {
    const int64_t m = dt == QD_F32 ? 4 : 8;                    // elements per 16 bytes
    return sd == 1 && qd_aligned(base, 16) && sb % m == 0 && st % m == 0 && sh % m == 0;
}

}  // namespace

extern "C" int qd_attn_h16(const void* q, const void* k, const void* v, int in_dtype, int B, int T, int S, int H, int d,
                           int64_t qsb, int64_t qst, int64_t qsh, int64_t qsd, int64_t ksb, int64_t kst, int64_t ksh, int64_t ksd,
                           int64_t vsb, int64_t vst, int64_t vsh, int64_t vsd, float scale, int op_dtype, void* out, int out_dtype,
                           int64_t ldo, void* stream) {
    QD_REQUIRE(q && k && v && out, "qd_attn_h16: null pointer");
    QD_REQUIRE(in_dtype == QD_F32 || in_dtype == QD_F16 || in_dtype == QD_BF16, "qd_attn_h16: in_dtype must be f32/f16/bf16 (got %d)", in_dtype);
    QD_REQUIRE(op_dtype == QD_F16 || op_dtype == QD_BF16, "qd_attn_h16: op_dtype must be f16/bf16 (got %d)", op_dtype);
    QD_REQUIRE(out_dtype == QD_F32 || out_dtype == QD_F16, "qd_attn_h16: out_dtype must be f32/f16 (got %d)", out_dtype);
    QD_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "qd_attn_h16: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    QD_REQUIRE(d >= 8 && d <= 256 && d % 8 == 0, "qd_attn_h16: head dim %d unsupported (a multiple of 8 in [8, 256])", d);
    QD_REQUIRE(std::isfinite(scale) && scale > 0.f, "qd_attn_h16: scale must be finite and positive");
    QD_REQUIRE(ldo >= (int64_t)H * d && ldo % 4 == 0 && qd_aligned(out, out_dtype == QD_F32 ? 16 : 8),
               "qd_attn_h16: ldo must be >= H*d and a multiple of 4, out aligned to 4 elements");
    QD_REQUIRE(ah_layout_ok(q, in_dtype, qsb, qst, qsh, qsd) && ah_layout_ok(k, in_dtype, ksb, kst, ksh, ksd) &&
               ah_layout_ok(v, in_dtype, vsb, vst, vsh, vsd),
               "qd_attn_h16: q/k/v need channel stride 1, 16-byte aligned bases and b/token/head strides that keep 16-byte alignment");
    const int64_t gx = (T + 127) / 128;
    QD_REQUIRE((int64_t)B * H * gx < (1L << 31) && (int64_t)B * T < (1L << 31), "qd_attn_h16: too many blocks");
    AttnH a{};
    a.q = reinterpret_cast<const char*>(q); a.k = reinterpret_cast<const char*>(k); a.v = reinterpret_cast<const char*>(v);
    const int64_t qs[3] = {qsb, qst, qsh}, ks[3] = {ksb, kst, ksh}, vs[3] = {vsb, vst, vsh};
    for (int i = 0; i < 3; ++i) { a.qs[i] = qs[i]; a.ks[i] = ks[i]; a.vs[i] = vs[i]; }
    a.out = out; a.ldo = ldo;
    a.T = T; a.S = S; a.H = H; a.d = d; a.gx = (int)gx; a.nblk = (int)((int64_t)B * H * gx);
    a.c2 = scale * 1.4426950408889634f;
    a.out_f16 = out_dtype == QD_F16;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)a.nblk);
    if (op_dtype == QD_BF16) launch_h16_in<true>(a, in_dtype, (d + 15) / 16, grid, st);
    else launch_h16_in<false>(a, in_dtype, (d + 15) / 16, grid, st);
    QD_LAUNCH_CHECK("qd_attn_h16");
    return 0;
}
