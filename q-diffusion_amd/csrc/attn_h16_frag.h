// attn_h16_frag.h — the lane-level pieces the fp16 / bf16 attention kernels share (attn_h16.hip, attn_h16_wide.hip): staging
// loads of 8 channels, conversion to the operand type, the 32x32x16 MFMA, the half-wave exchanges of the transposed score
// tile and the key order of a V^T row.  attn_h16.hip's header comment describes the layout they belong to.
#pragma once
#include "common.h"

namespace {

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

// LDS position of key `kk` (0..31) inside a V^T row: the k order of the P fragments (see attn_h16.hip's header)
__device__ __forceinline__ int ah_vpos(int kk) {
    const int s = kk >> 4, rem = kk & 15;
    return 16 * s + 8 * ((rem >> 2) & 1) + 4 * (rem >> 3) + (rem & 3);
}

// runs of 8 channels are read as 16- / 32-byte vectors: channel stride 1, every run 16-byte aligned
inline bool ah_layout_ok(const void* base, int dt, int64_t sb, int64_t st, int64_t sh, int64_t sd) {
    const int64_t m = dt == QD_F32 ? 4 : 8;                    // elements per 16 bytes
    return sd == 1 && qd_aligned(base, 16) && sb % m == 0 && st % m == 0 && sh % m == 0;
}

}  // namespace
