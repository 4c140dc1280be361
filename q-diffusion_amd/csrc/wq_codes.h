// wq_codes.h — the code unpack of the weights-only kernels (device only): tile-ordered int4 / int8 weight CODES of
// qd_pack_weights_t4 / _t8 -> the fp16 / bf16 B fragment q - z of v_mfma_f32_32x32x16_{f16,bf16}.  One copy, included by
// wq_h16.hip (qd_conv2d_wq_h16) and temb_mlp.hip (qd_temb_mlp_wq_h16): the second equals the first bit for bit because both
// execute THESE operations, as both call qd_wq_affine / qd_geglu_f of common.h.
#pragma once
#include "common.h"

typedef _Float16 v2h __attribute__((ext_vector_type(2)));

// 8 codes of a unit -> the halves 1024 + q of K order 0..7 (the 0x6400 | q bit pattern, one v_perm_b32 per two codes)
template <int WB>
__device__ __forceinline__ v4i wq_magic(unsigned x, unsigned y) {
    if constexpr (WB == 4) {                                  // one word of raw nibbles: lo nibbles are codes 0..3, hi nibbles 4..7 (y unused)
        const unsigned lo = x & 0x0F0F0F0Fu, hi = (x >> 4) & 0x0F0F0F0Fu;
        return v4i{(int)__builtin_amdgcn_perm(0x64646464u, lo, 0x04010400u), (int)__builtin_amdgcn_perm(0x64646464u, lo, 0x04030402u),
                   (int)__builtin_amdgcn_perm(0x64646464u, hi, 0x04010400u), (int)__builtin_amdgcn_perm(0x64646464u, hi, 0x04030402u)};
    } else {                                                  // two words of stored bytes q - 128
        x ^= 0x80808080u;
        y ^= 0x80808080u;
        return v4i{(int)__builtin_amdgcn_perm(0x64646464u, x, 0x04010400u), (int)__builtin_amdgcn_perm(0x64646464u, x, 0x04030402u),
                   (int)__builtin_amdgcn_perm(0x64646464u, y, 0x04010400u), (int)__builtin_amdgcn_perm(0x64646464u, y, 0x04030402u)};
    }
}
// halves 1024 + q -> the B fragment (q - z) in the operand type; nz = {-(1024 + z), -(1024 + z)}
template <bool FH>
__device__ __forceinline__ v4i wq_frag(const v4i& mag, const v2h nz) {
    v4i r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // (through a scalar: hipcc folds __builtin_bit_cast of a vector SUBSCRIPT to element 0 for every e)
        const int w = mag[e];
        const v2h d = __builtin_bit_cast(v2h, w) + nz;                // v_pk_add_f16: exact integers
        if constexpr (FH) r[e] = __builtin_bit_cast(int, d);
        else r[e] = (int)qd_pack2bf((float)d[0], (float)d[1]);
    }
    return r;
}
