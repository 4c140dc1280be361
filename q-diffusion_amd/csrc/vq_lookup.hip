// vq_lookup.hip — nearest-codebook lookup of the VQ first stage (qd_vq_lookup; DESIGN.md §4.11 addendum 2).
//
// Replaces VectorQuantizer.indices / get_codebook_entry of qdiff/arch/first_stage.py (reference: the `self.quantize` call of
// ldm/models/autoencoder.py:274-283), which materialise the [pixels][n_e] fp32 distance matrix.  Here the matrix never exists:
//
//   * a block of 256 lanes owns a tile of 1024 pixels, four per lane (pixel tile*1024 + k*256 + lane: coalesced loads).  Their
//     NEGATED channels sit in VGPRs as two packed pairs, so one code costs v_pk_fma_f32 x channels x 2 plus four
//     compare / select pairs against ONE broadcast LDS read;
//   * LDS holds a stage of 512 codes as records {e_0 .. e_{E-1}, 0 .., h} of 4 (E <= 3), 8 (E <= 7) or 12 (E = 8) floats with
//     h = |e|^2 / 2 in slot EC (the channel count of the instantiation), written by the lanes that fetched the rows: there is no
//     prepare launch.  Every lane of a wave reads the same record (a broadcast, no bank conflicts), 16 bytes per ds_read.  The
//     rows of the next stage are fetched into registers BEFORE the scan of the current one and committed to the other buffer
//     after it: one barrier per stage;
//   * the grid is pixel tiles x code slices (vq_choose, the one rule).  With one slice the block walks the whole codebook and
//     emits; with more, slice s scans codes [s*per, (s+1)*per) and writes (score, index) to ws[s][pixel], and vq_merge_kernel
//     takes the slices in index order with a strict <, which keeps the first minimum, then emits.
//
// Score of code j for a pixel: s = h_j; s = fma(-z_c, e_jc, s) for c = 0 .. E-1 (fp32).  h_j: sum of e_jc^2 in channel order in
// fp64, halved, rounded ONCE to fp32.  The padded channels of a record and of a pixel are zeros: fma(-0, 0, s) = s exactly.
// Unused records of a stage carry h = +inf and lose every strict comparison.  No atomics anywhere.
#include "common.h"
#include <algorithm>

namespace {

constexpr int VQ_THREADS = 256;                    // lanes of a block
constexpr int VQ_PPL = 4;                          // pixels per lane
constexpr int VQ_TILE = VQ_THREADS * VQ_PPL;       // pixels per block
constexpr int VQ_STAGE = 512;                      // codes per LDS stage (two stages resident)
constexpr int VQ_RPL = VQ_STAGE / VQ_THREADS;      // records a lane stages
constexpr int VQ_MIN_SLICE = 128;                  // codes per slice are a multiple of this
constexpr int VQ_MAX_SLICES = 64;
constexpr int VQ_FULL_TILES = 256;                 // pixel tiles that fill the chip by themselves (one block per CU)
constexpr int VQ_TARGET_BLOCKS = 512;              // below that: slices so that tiles x slices reaches two blocks per CU

struct VqArgs {
    const void* z;
    int z_dtype, E;
    long P, S, sb, sc, ss;
    const float* cb;
    int n_e, per;                                  // per: codes per slice
    const float* table;
    int T, out_dtype;
    int32_t* indices;
    void* out;
    long ldo;
    uint2* ws;                                     // [slices][P] {score bits, index}
};

int& vq_knob() {
    static int slices = -1;
    return slices;
}

// THE rule: code slices and codes per slice for P pixels and n_e codes (launcher, qd_vq_lookup_ws_bytes, qd_vq_lookup_form).
struct VqForm { int slices, per; };
VqForm vq_choose(int64_t P, int n_e) {
    const int64_t tiles = (P + VQ_TILE - 1) / VQ_TILE;
    const int most = std::min(VQ_MAX_SLICES, (n_e + VQ_MIN_SLICE - 1) / VQ_MIN_SLICE);
    int64_t want = vq_knob() >= 1 ? vq_knob() : (tiles >= VQ_FULL_TILES ? 1 : (VQ_TARGET_BLOCKS + tiles - 1) / tiles);
    want = std::max<int64_t>(1, std::min<int64_t>(want, most));
    int per = (int)((n_e + want - 1) / want);
    per = (per + VQ_MIN_SLICE - 1) / VQ_MIN_SLICE * VQ_MIN_SLICE;
    return VqForm{(n_e + per - 1) / per, per};                   // no slice is empty
}

__device__ __forceinline__ float vq_ldz(const void* z, int dt, long off) {
    if (dt == QD_F32) return reinterpret_cast<const float*>(z)[off];
    if (dt == QD_F16) return __half2float(reinterpret_cast<const __half*>(z)[off]);
    return qd_bf2f(reinterpret_cast<const unsigned short*>(z)[off]);
}

// ---- staging: global rows -> registers (fetch), registers -> LDS records (commit) ----
template <int EC>
__device__ __forceinline__ void vq_fetch(float (&e)[VQ_RPL][EC], const float* cb, int E, int j0, int jend, int tid) {
#pragma unroll
    for (int u = 0; u < VQ_RPL; ++u) {
        const int j = j0 + tid + u * VQ_THREADS;
        const float* row = cb + (long)j * E;
#pragma unroll
        for (int c = 0; c < EC; ++c) e[u][c] = (j < jend && c < E) ? row[c] : 0.f;
    }
}

template <int EC, int REC>
__device__ __forceinline__ void vq_commit(const float (&e)[VQ_RPL][EC], float* buf, int j0, int jend, int tid) {
#pragma unroll
    for (int u = 0; u < VQ_RPL; ++u) {
        const int r = tid + u * VQ_THREADS;
        double h = 0.0;
        float rec[REC];
#pragma unroll
        for (int c = 0; c < REC; ++c) rec[c] = 0.f;
#pragma unroll
        for (int c = 0; c < EC; ++c) {
            rec[c] = e[u][c];
            h = __builtin_fma((double)e[u][c], (double)e[u][c], h);
        }
        rec[EC] = j0 + r < jend ? (float)(0.5 * h) : __builtin_inff();
        v4f* dst = reinterpret_cast<v4f*>(buf + r * REC);
#pragma unroll
        for (int q = 0; q < REC / 4; ++q) dst[q] = v4f{rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]};
    }
}

// ---- the scan of one stage: n4 records (a multiple of four), global index of record 0 = jbase ----
template <int EC, int REC>
__device__ __forceinline__ void vq_scan(const float* buf, int n4, int jbase, const v2f (&nz)[2][EC], float (&best)[VQ_PPL], int (&idx)[VQ_PPL]) {
#pragma unroll 4
    for (int r = 0; r < n4; ++r) {
        const v4f* src = reinterpret_cast<const v4f*>(buf + r * REC);
        float rec[REC];
#pragma unroll
        for (int q = 0; q < REC / 4; ++q) {
            const v4f v = src[q];
            rec[4 * q] = v[0]; rec[4 * q + 1] = v[1]; rec[4 * q + 2] = v[2]; rec[4 * q + 3] = v[3];
        }
        v2f a0 = qd_splat2(rec[EC]), a1 = a0;
#pragma unroll
        for (int c = 0; c < EC; ++c) {
            a0 = qd_fma2(nz[0][c], qd_splat2(rec[c]), a0);
            a1 = qd_fma2(nz[1][c], qd_splat2(rec[c]), a1);
        }
        const int j = jbase + r;
        const float s[VQ_PPL] = {a0.x, a0.y, a1.x, a1.y};
#pragma unroll
        for (int k = 0; k < VQ_PPL; ++k) {
            const bool lt = s[k] < best[k];                      // strict, ascending j: the first minimum; NaN never wins
            best[k] = lt ? s[k] : best[k];
            idx[k] = lt ? j : idx[k];
        }
    }
}

// ---- one pixel's results: its index, and row table[j] widened to ldo columns with 16-byte stores ----
__device__ __forceinline__ void vq_emit(const VqArgs& a, long p, int j) {
    if (a.indices) a.indices[p] = j;
    if (!a.out) return;
    float t[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) t[c] = c < a.T ? a.table[(long)j * a.T + c] : 0.f;
    if (a.out_dtype == QD_F32) {
        v4f* o = reinterpret_cast<v4f*>(reinterpret_cast<float*>(a.out) + p * a.ldo);
        const int chunks = (int)(a.ldo / 4);
        o[0] = v4f{t[0], t[1], t[2], t[3]};
        if (chunks > 1) o[1] = v4f{t[4], t[5], t[6], t[7]};      // (one chunk: ldo = 4 >= T, so t[4..7] are zeros anyway)
        for (int q = 2; q < chunks; ++q) o[q] = v4f{0.f, 0.f, 0.f, 0.f};
    } else {
        v4i* o = reinterpret_cast<v4i*>(reinterpret_cast<unsigned short*>(a.out) + p * a.ldo);
        const int chunks = (int)(a.ldo / 8);
        v4i w;
        if (a.out_dtype == QD_F16)
            w = v4i{(int)qd_pack2h(t[0], t[1]), (int)qd_pack2h(t[2], t[3]), (int)qd_pack2h(t[4], t[5]), (int)qd_pack2h(t[6], t[7])};
        else
            w = v4i{(int)qd_pack2bf(t[0], t[1]), (int)qd_pack2bf(t[2], t[3]), (int)qd_pack2bf(t[4], t[5]), (int)qd_pack2bf(t[6], t[7])};
        o[0] = w;
        for (int q = 1; q < chunks; ++q) o[q] = v4i{0, 0, 0, 0};
    }
}

// grid (pixel tiles, code slices).  DIRECT: one slice, the block emits; else (score, index) per pixel to ws[slice].
template <int EC, int REC, bool DIRECT>
__global__ __launch_bounds__(VQ_THREADS) void vq_scan_kernel(const VqArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][VQ_STAGE * REC];
    const int tid = threadIdx.x, slice = DIRECT ? 0 : (int)blockIdx.y;
    const int j0 = slice * a.per, j1 = min(a.n_e, j0 + a.per);
    float e[VQ_RPL][EC];
    vq_fetch<EC>(e, a.cb, a.E, j0, j1, tid);                    // the first stage's rows are in flight while the pixels load

    const long p0 = (long)blockIdx.x * VQ_TILE + tid;
    v2f nz[2][EC];
#pragma unroll
    for (int k = 0; k < VQ_PPL; ++k) {
        const long p = p0 + k * VQ_THREADS;
        const bool in = p < a.P;
        const long base = in ? (p / a.S) * a.sb + (p % a.S) * a.ss : 0;
#pragma unroll
        for (int c = 0; c < EC; ++c) nz[k >> 1][c][k & 1] = (in && c < a.E) ? -vq_ldz(a.z, a.z_dtype, base + c * a.sc) : 0.f;
    }
    float best[VQ_PPL];
    int idx[VQ_PPL];
#pragma unroll
    for (int k = 0; k < VQ_PPL; ++k) { best[k] = __builtin_inff(); idx[k] = 0; }

    vq_commit<EC, REC>(e, lds[0], j0, j1, tid);
    __syncthreads();
    int cur = 0;
    for (int js = j0; js < j1; js += VQ_STAGE, cur ^= 1) {
        const int next = js + VQ_STAGE;
        const bool more = next < j1;                             // uniform
        if (more) vq_fetch<EC>(e, a.cb, a.E, next, j1, tid);
        const int n = min(VQ_STAGE, j1 - js);
        vq_scan<EC, REC>(lds[cur], (n + 3) & ~3, js, nz, best, idx);
        if (more) vq_commit<EC, REC>(e, lds[cur ^ 1], next, j1, tid);   // that buffer's scan ended before the last barrier
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < VQ_PPL; ++k) {
        const long p = p0 + k * VQ_THREADS;
        if (p >= a.P) continue;
        if constexpr (DIRECT) vq_emit(a, p, idx[k]);
        else a.ws[(long)slice * a.P + p] = uint2{__float_as_uint(best[k]), (unsigned)idx[k]};
    }
}

__global__ __launch_bounds__(VQ_THREADS) void vq_merge_kernel(const VqArgs a, int slices) {
    const long p = (long)blockIdx.x * VQ_THREADS + threadIdx.x;
    if (p >= a.P) return;
    float best = __builtin_inff();
    int idx = 0;
    for (int s = 0; s < slices; ++s) {                           // ascending code ranges, strict <: the first minimum survives
        const uint2 w = a.ws[(long)s * a.P + p];
        const float sc = __uint_as_float(w.x);
        const bool lt = sc < best;
        best = lt ? sc : best;
        idx = lt ? (int)w.y : idx;
    }
    vq_emit(a, p, idx);
}

template <int EC, int REC>
void vq_launch(const VqArgs& a, int slices, hipStream_t st) {
    const unsigned tiles = (unsigned)((a.P + VQ_TILE - 1) / VQ_TILE);
    if (slices == 1) {
        hipLaunchKernelGGL((vq_scan_kernel<EC, REC, true>), dim3(tiles), dim3(VQ_THREADS), 0, st, a);
        return;
    }
    hipLaunchKernelGGL((vq_scan_kernel<EC, REC, false>), dim3(tiles, (unsigned)slices), dim3(VQ_THREADS), 0, st, a);
    hipLaunchKernelGGL(vq_merge_kernel, dim3((unsigned)((a.P + VQ_THREADS - 1) / VQ_THREADS)), dim3(VQ_THREADS), 0, st, a, slices);
}

bool vq_shape_ok(int64_t B, int64_t S, int n_e) { return B > 0 && S > 0 && B <= (1ll << 31) / S && B * S < (1ll << 31) && n_e >= 1 && n_e <= (1 << 20); }

}  // namespace

extern "C" void qd_vq_config(int slices) { vq_knob() = slices < 1 ? -1 : slices; }

extern "C" int qd_vq_lookup_form(int64_t B, int64_t S, int n_e, int32_t* form2) {
    QD_REQUIRE(form2 != nullptr, "qd_vq_lookup_form: null form2");
    QD_REQUIRE(vq_shape_ok(B, S, n_e), "qd_vq_lookup_form: need B, S >= 1, B*S < 2^31 and n_e in [1, 2^20]");
    const VqForm f = vq_choose(B * S, n_e);
    form2[0] = f.slices;
    form2[1] = f.slices > 1 ? 2 : 1;
    return 0;
}

extern "C" int64_t qd_vq_lookup_ws_bytes(int64_t B, int64_t S, int n_e) {
    if (!vq_shape_ok(B, S, n_e)) return 0;
    const VqForm f = vq_choose(B * S, n_e);
    return f.slices > 1 ? (int64_t)f.slices * B * S * (int64_t)sizeof(uint2) : 0;
}

extern "C" int qd_vq_lookup(const void* z, int z_dtype, int64_t B, int64_t S, int e_dim, int64_t sb, int64_t sc, int64_t ss,
                            const float* codebook, int n_e, const float* table, int t_dim, int32_t* indices, void* out, int out_dtype,
                            int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    QD_REQUIRE(z && codebook, "qd_vq_lookup: null z / codebook");
    QD_REQUIRE(z_dtype == QD_F32 || z_dtype == QD_F16 || z_dtype == QD_BF16, "qd_vq_lookup: z_dtype must be f32/f16/bf16");
    QD_REQUIRE(vq_shape_ok(B, S, n_e), "qd_vq_lookup: need B, S >= 1, B*S < 2^31 and n_e in [1, 2^20]");
    QD_REQUIRE(e_dim >= 1 && e_dim <= 8, "qd_vq_lookup: e_dim %d outside [1, 8]", e_dim);
    QD_REQUIRE(qd_aligned(z, z_dtype == QD_F32 ? 4 : 2) && qd_aligned(codebook, 4), "qd_vq_lookup: z / codebook not aligned to their element");
    if (!table) { table = codebook; t_dim = e_dim; }
    QD_REQUIRE(t_dim >= 1 && t_dim <= 8 && qd_aligned(table, 4), "qd_vq_lookup: t_dim %d outside [1, 8] (or table unaligned)", t_dim);
    QD_REQUIRE(indices || out, "qd_vq_lookup: indices and out are both null");
    QD_REQUIRE(!indices || qd_aligned(indices, 4), "qd_vq_lookup: indices not 4-byte aligned");
    if (out) {
        QD_REQUIRE(out_dtype == QD_F32 || out_dtype == QD_F16 || out_dtype == QD_BF16, "qd_vq_lookup: out_dtype must be f32/f16/bf16");
        const int chunk = out_dtype == QD_F32 ? 4 : 8;           // elements of a 16-byte store
        QD_REQUIRE(ldo >= t_dim && ldo % chunk == 0 && qd_aligned(out, 16),
                   "qd_vq_lookup: ldo must cover t_dim and be a multiple of %d elements, out 16-byte aligned", chunk);
    }
    const int64_t P = B * S;
    const VqForm f = vq_choose(P, n_e);
    if (f.slices > 1)
        QD_REQUIRE(ws && qd_aligned(ws, 8) && ws_bytes >= (int64_t)f.slices * P * (int64_t)sizeof(uint2),
                   "qd_vq_lookup: %d code slices need %lld bytes of 8-byte aligned workspace (qd_vq_lookup_ws_bytes), got %lld", f.slices,
                   (long long)((int64_t)f.slices * P * (int64_t)sizeof(uint2)), (long long)(ws ? ws_bytes : 0));
    VqArgs a;
    a.z = z; a.z_dtype = z_dtype; a.E = e_dim;
    a.P = (long)P; a.S = (long)S; a.sb = (long)sb; a.sc = (long)sc; a.ss = (long)ss;
    a.cb = codebook; a.n_e = n_e; a.per = f.per;
    a.table = table; a.T = t_dim; a.out_dtype = out_dtype;
    a.indices = indices; a.out = out; a.ldo = (long)ldo;
    a.ws = reinterpret_cast<uint2*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (e_dim <= 3) vq_launch<3, 4>(a, f.slices, st);
    else if (e_dim <= 7) vq_launch<7, 8>(a, f.slices, st);
    else vq_launch<8, 12>(a, f.slices, st);
    QD_LAUNCH_CHECK("qd_vq_lookup");
    return 0;
}
