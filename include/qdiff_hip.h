/*
 * qdiff_hip.h — C ABI of libqdiff_hip.so, the MI355X (gfx950) integer engine that sits under
 * the q-diffusion `qdiff` Python API.
 *
 * The reference (Xiuyu-Li/q-diffusion) has no FFI layer: its hot path is a chain of ATen calls
 * issued from qdiff/quant_layer.py, qdiff/adaptive_rounding.py and qdiff/quant_block.py.  Each
 * entry point below replaces one of those implicit op sequences and cites
 * the reference lines whose arithmetic it reproduces.
 *
 * Conventions
 *   - plain C: raw device pointers, ints, POD structs; no torch types.  `stream` is a hipStream_t
 *     passed as void*.  All kernels are enqueued on `stream` and return without synchronising
 *     (safe inside hipGraph capture: no allocation, no sync, no host read-back).
 *   - every function returns 0 on success, non-zero on error; qd_last_error() returns a
 *     thread-local message.  Nothing falls back to the host: a bad argument is an error.
 *   - the library is stateless (no global mutable state besides the thread-local error text).
 *   - quantisation parameters that the reference keeps as tensors / nn.Parameters (delta,
 *     zero_point) are read by the kernels from DEVICE memory, so the host never has to .item() them.
 *
 * Integer conventions
 *   activation code  q  = clamp(rint(x/delta) + zp, qmin, qmax)        (quant_layer.py:82-87)
 *   stored byte      a' = q - off,  off = 128 for unsigned 8-bit grids, 0 for signed grids
 *   "true zero"      z' = zp - off  (the byte that dequantises to 0.0; used for conv padding)
 *   weight code      W  = clamp(floor(w/dw)+(alpha>=0)+zw, 0, 2^b-1)   (adaptive_rounding.py:49-59)
 *   stored weight    w' = W (int4 path: the raw nibble, unpacked in-kernel) or W - 128 (int8 path); the
 *                    per-channel remainder zw resp. zw-128 is restored in the epilogue through activation
 *                    row sums (qd_conv_seg.zw).
 */
#ifndef QDIFF_HIP_H
#define QDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_ABI_VERSION 20

/* element types of floating-point tensors crossing the ABI */
enum { QD_F32 = 0, QD_F16 = 1, QD_BF16 = 2 };
/* epilogues of qd_conv2d_i8 */
enum { QD_EPI_LINEAR = 0, QD_EPI_GEGLU_I8 = 1, QD_EPI_HEADS_I8 = 2, QD_EPI_HEADS_T_I8 = 3, QD_EPI_GEGLU_H16 = 4 /* qd_conv2d_wq_h16 only */ };

int         qd_abi_version(void);
const char* qd_last_error(void);
/* 1 if a gfx950 device is visible to this process, else 0 (never throws). */
int         qd_device_ok(void);

/* Box calibration (ABI v20; measurement aid of bench.py, not on the product path): `blocks` workgroups of 256 threads run `iters`
 * iterations of kind 0: 8 dense v_mfma_i32_32x32x32_i8 per wave (four independent accumulators; 8 * 65536 integer ops each), or
 * kind 1: 32 v_exp_f32 per wave (four independent registers).  ticks[block] = elapsed shader-clock ticks of the block's first wave;
 * the caller times the launch (HIP events): 512 blocks = two waves per SIMD, 1024 = four.  sink: one int the kernel never writes. */
int qd_box_probe(int kind, int blocks, int iters, long long* ticks, int* sink, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quantiser parameters.  Every entry point below that takes `qparams` / `oq_params` expects a device float[4]
 *     {delta, zero_point, rinv, fast} produced by qd_make_qparams from the reference's per-tensor delta / zero_point
 *     (quant_layer.py:66-89; both read from DEVICE memory, no host round trip).  rinv is the correctly rounded
 *     reciprocal of delta; fast != 0 certifies — by an exhaustive check over all 2^23 mantissas — that
 *     y = x*rinv; e = fma(-y, delta, x); q = fma(e, rinv, y) equals the IEEE quotient x / delta bit for bit for this
 *     delta, so the kernels may use it instead of the division that torch.round(x / delta) semantics require;
 *     otherwise they divide.  Codes are bit-identical either way.
 * ------------------------------------------------------------------------------------------ */
int qd_make_qparams(const float* delta, const float* zero_point, float* out4, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1  activation quantiser.   Replaces UniformAffineQuantizer.forward on an *input activation*
 *     (qdiff/quant_layer.py:66-89) and the two-quantizer + torch.cat split path of
 *     QuantModule.forward (quant_layer.py:256-264).
 *
 *     x is a logical [B][C][S] tensor addressed by element strides (sb, sc, ss): NCHW-contiguous
 *     is (C*S, S, 1), channels_last / token-major is (S*C, 1, C).  Channels [c0, c0+clen) are
 *     quantised with qparams (qd_make_qparams) and written as
 *     int8 to out[(b*S+s)*ldo + oc0 + (c-c0)]; channels up to clen_pad are filled with the
 *     "true zero" byte so that padded K lanes contribute nothing.
 *     qmin/qmax/off describe the integer grid (see header comment).
 * ------------------------------------------------------------------------------------------ */
int qd_quantize_act(const void* x, int x_dtype, int64_t B, int64_t C, int64_t S,
                    int64_t sb, int64_t sc, int64_t ss,
                    int c0, int clen, int clen_pad,
                    const float* qparams, int qmin, int qmax, int off,
                    int8_t* out, int64_t ldo, int oc0, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  weight packer.   Replaces the per-forward weight fake-quant of AdaRoundQuantizer.forward
 *     (qdiff/adaptive_rounding.py:49-61, branch learned_hard_sigmoid / soft_targets=False) and of
 *     UniformAffineQuantizer.forward on weights (quant_layer.py:82-88; round-to-nearest) by a
 *     one-time pack.  w is the fp32 weight viewed as [Cout][Cin_total][taps] (PyTorch OIHW with
 *     HW flattened); the channel slice [c0, c0+clen) is quantised with per-out-channel delta/zp
 *     (fp32 [Cout]) and, when alpha != NULL (same layout as the slice, [Cout][clen][taps]),
 *     AdaRound hard rounding.  Output row n, tap t: bytes [kofs, kofs+clen_pad) of
 *     wq[(n*taps+t)*ldk ...] hold W-128 (bits==8 → mode 8) or W-zw (mode 0: direct s8) ;
 *     mode 4 packs W as nibbles (two per byte, layout in DESIGN.md §4.2) at byte offset kofs/2.
 *     wsum[n] += sum of the stored s8 values (mode 8/0) or of (W-zw) (mode 4) over the slice.
 *     codes (optional, may be NULL): int32 [Cout][clen][taps] raw W codes for tests.
 * ------------------------------------------------------------------------------------------ */
int qd_pack_weights(const float* w, const float* alpha, const float* delta, const float* zp,
                    int Cout, int Cin_total, int taps, int c0, int clen, int clen_pad,
                    int n_levels, int mode, uint8_t* wq, int64_t ldk, int kofs,
                    int32_t* wsum, int32_t* codes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3/K4  integer convolution / GEMM.   Replaces fwd_func(input, weight, bias, **fwd_kwargs) of
 *     QuantModule.forward (qdiff/quant_layer.py:276 → F.conv2d / F.conv1d(k=1) / F.linear on
 *     dequantised fp32 operands) by an implicit GEMM on the integer codes:
 *        M = B*Ho*Wo, N = Cout, K = taps * sum(seg.clen)
 *        out[m][n] = sum_seg scale_s[n] * I_s[m][n] + bias[n] + rowbias[b(m)][n] + residual[m][n]
 *        I_s = acc_s - zc_s[n] - zw_s[n] * (Asum_s[m] - kz_s)
 *     acc_s is the exact int32 MFMA accumulator of stored bytes; zc/zw/kz restore the zero points
 *     (DESIGN.md §3).  Two segments implement the split-shortcut of quant_layer.py:257-269.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t        c0;       /* first channel of the segment inside an x row (bytes)              */
    int32_t        clen;     /* channel count, multiple of 16 (padded)                            */
    int32_t        kofs;     /* reserved (row-major weight layouts of ABI <= 9); ignored                */
    int32_t        kstep0;   /* index of the segment's first 64-wide K-step in the tiled weight array    */
    const int8_t*  wzp;     /* reserved (ABI <= 9); ignored                                              */
    const float*   scale;    /* [Cout]  delta_x * delta_w[n]                                       */
    const int32_t* zc;       /* [Cout]  z' * Wsum[n]            or NULL (symmetric activations)    */
    const int32_t* zw;       /* [Cout]  zw[n]-128 (int8 tiles) | zw[n] (int4 tiles)                          */
    const int32_t* zfill;    /* [2] {z', K_seg*z'} device scalars or NULL (= 0)                    */
    const int8_t*  fill16;   /* 16 bytes of z' — the source of out-of-image taps for the LDS-DMA loader —
                                or NULL (= zeros)                                                  */
} qd_conv_seg;

typedef struct {
    const int8_t*  x;        /* [B][H][W][ldx] stored activation bytes                            */
    const uint8_t* w;        /* MFMA-tile-ordered weights of qd_pack_weights_t4 (wbits=4) / _t8 (wbits=8) */
    void*          out;      /* [M][ldo]                                                           */
    const float*   bias;     /* [Cout] or NULL                                                     */
    const float*   rowbias;  /* [B][ld_rowbias] per-sample per-channel add (timestep emb) or NULL  */
    const void*    residual; /* [M][ldr] same dtype as out, or NULL                                */
    int64_t        ldx, ldk, ldo, ldr, ld_rowbias;
    int32_t        B, H, W, Ho, Wo, Cout;
    int32_t        kh, kw, stride, pad_t, pad_l;
    int32_t        wbits;    /* 8 or 4 (16: qd_conv2d_bf16)                                        */
    int32_t        out_dtype;/* QD_F32 / QD_F16                                                    */
    int32_t        nseg;     /* 1 or 2                                                             */
    int32_t        w_tiled;  /* must be 1 (the row-major layouts of ABI <= 9 are gone)                  */
    int32_t        epilogue; /* QD_EPI_LINEAR, or QD_EPI_GEGLU_I8 (w_tiled only): the weight rows were packed
                                interleaved per 32 (value tile, gate tile, value tile, ...); the epilogue computes
                                value*gelu(gate) (ldm/modules/attention.py:42-44) and writes it QUANTISED with
                                oq_* (the act quantiser of the following Linear) as int8 rows out[M][ldo]        */
    qd_conv_seg    seg[2];
    const float*   oq_params;/* QD_EPI_GEGLU_I8: {delta, zero_point} of the output quantiser (device)             */
    int32_t        oq_min, oq_max, oq_off, _pad2;
    void*          splitk_ws;      /* optional scratch of >= qd_conv2d_i8_splitk_ws_bytes(d) bytes (16-B aligned); when
                                      given, layers too small to fill the chip are contracted split-K: int32 partials
                                      per K range (exact), then one pass that sums them and applies the epilogue.
                                      NULL = never split.  Results do not depend on it (integer partial sums).       */
    int64_t        splitk_ws_bytes;
    /* QD_EPI_HEADS_I8 / QD_EPI_HEADS_T_I8 (w_tiled, one segment): the Linear is a q/k/v projection of an
     * attention block (qdiff/quant_block.py:190-221).  Rows are m = b*hd_T + t, columns n = h*hd_d + dd.
     * y = (I*scale + bias) * oq_prescale is quantised with oq_* (the block's act_quantizer_q/k/v) and
     * written as int8 in the operand layout of qd_attn_i8, exactly what qd_quantize_heads would produce:
     *   HEADS_I8  : out[(b*H+h)][hd_Tpad][hd_dpad]               (transpose=0 layout)
     *   HEADS_T_I8: out[(b*H+h)][hd_dpad][hd_Tpad], key-permuted (transpose=1 layout); hd_sum[(b*H+h)][hd_dpad]
     *               += column sums (caller zeroes hd_sum first).
     * HEADS_I8 also accepts an fp32 `residual` (added before the quantiser): with hd_H = 1, hd_d = Cout it is
     * "Linear + residual -> int8 rows of the next Linear" (transformer FF output feeding SpatialTransformer.proj_out).
 * Pad bytes are not written: out must be zero-initialised once (it can then be reused).
     * hd_T must be a multiple of 128 (a tile of rows never straddles two samples).  Weights: int4 tiles of any width,
     * or int8 tiles with Cout > 64 (the 1x1 q / k / v convolutions of the pixel-space AttnBlock, quant_block.py:354-386). */
    int32_t        hd_H, hd_d, hd_T, hd_Tpad, hd_dpad;
    float          oq_prescale;
    int32_t*       hd_sum;
    /* optional (w_tiled, QD_EPI_LINEAR, fp32 out, Ho*Wo % 128 == 0): the kernel also writes the first level of the
     * GroupNorm statistics of its output, gn_part[b][Ho*Wo/128][Cout][2] = {sum, sum of squares} over each 128-row
     * chunk, which qd_groupnorm_silu_quant accepts as part_in (one pass over the tensor less).  Disables split-K.
     * gn_ld: channels per chunk row of the statistics buffer (0 = Cout).  A value > Cout lets two producers write the
     * statistics of the two halves of a skip concatenation (openaimodel.py:776) into column ranges of one buffer, the
     * same way `out` + `ldo` place their fp32 rows into column ranges of one activation buffer: the concatenation
     * then costs no copy at all. */
    float*         gn_part;
    int64_t        gn_ld;
    /* non-zero: x holds the HALF-resolution map [B][H/2][W/2][ldx] and the convolution runs on its nearest-neighbour 2x
     * up-sampling (Upsample: openaimodel.py:105-120, ddim diffusion.py:36-52) — H, W are the up-sampled sizes; the
     * replication happens in the im2col source address, no up-sampled tensor exists.  Needs stride 1, kh*kw > 1, even H, W. */
    int32_t        upsample2x;
    /* residual row period (the field that used to be _pad3; size and offsets unchanged): 0 = output row m adds residual row m.
     * P > 0: output row m adds residual[(m % P) * ldr + n] — the residual holds P rows only, those of the first P / (Ho*Wo)
     * samples, and every later group of samples re-reads them (the two halves of a classifier-free-guidance batch share
     * everything up to the first cross-attention: nothing is duplicated in memory).  The mapping is per row: a tile may straddle
     * the period.  Needs a residual, M % P == 0 and P % (Ho*Wo) == 0.  qd_conv2d_i8 with QD_EPI_LINEAR only (fp32 / fp16 rows,
     * either block form, one or two segments); such a descriptor is never contracted split-K (qd_conv2d_i8_splitk_ws_bytes = 0),
     * so the bytes do not depend on splitk_ws.  Every other entry and epilogue refuses a non-zero value. */
    int32_t        res_period;
} qd_conv_desc;

int qd_conv2d_i8(const qd_conv_desc* d, void* stream);

/* qd_conv_config (ABI v20): kgroups 1 (default; initial value QD_KGROUPS) = a launch with at most one output tile per CU and at least
 * eight K-steps runs 512-thread blocks whose two groups of four waves contract alternate K-steps and add their int32
 * accumulators in LDS before the (unchanged) epilogue — two waves per SIMD where the four-wave block leaves one; 0 = always the
 * four-wave block; -1 = leave unchanged.  The integers, and therefore the bytes written, are the same either way.
 * The argument is a bit field: bit 0 is the K-group choice above; bit 1 (value 2, so 2 or 3; for tests) sends every block of the
 * linear epilogues (fp32 / fp16 / bf16 rows, int32 accumulators, split-K partials) through the generic body that otherwise only
 * blocks with a ragged edge take, instead of the full-tile body — again the same bytes.  Every call with a non-negative argument
 * sets both bits, so qd_conv_config(0) and qd_conv_config(1) also restore the default epilogue choice. */
void qd_conv_config(int kgroups);

/* Grouped launch (ABI v20): n = 1..3 descriptors of ONE problem shape with head-layout epilogues (QD_EPI_HEADS_I8 / _T_I8) — the
 * q / k / v projections of an attention block, which the reference evaluates as three Linears on the rows of one LayerNorm
 * (qdiff/quant_block.py:193-199, ldm attention.py:174-182; the DDIM AttnBlock's q / k / v convolutions diffusion.py:142-144; the
 * three row subsets of the LDM AttentionBlock's qkv conv1d, openaimodel.py:311-326) — as ONE launch whose grid's second
 * dimension selects the descriptor: three 256-block launches (one wave per SIMD each) become one that fills the chip, two
 * prologue ramps and two dependent-launch boundaries disappear.  Members that do not qualify (different shapes, another
 * epilogue, a tile shape the group kernel is not built for) run as the n single launches of qd_conv2d_i8: the bytes written are
 * the same either way. */
int qd_conv2d_i8_group(const qd_conv_desc* const* descs, int n, void* stream);

/* Scratch bytes qd_conv2d_i8 would use for a split-K contraction of this descriptor (shape fields only are
 * read); 0 when the layer is launched unsplit. */
int64_t qd_conv2d_i8_splitk_ws_bytes(const qd_conv_desc* d);

/* Launch-form query (ABI v20, additive; a pure host function): form4 = {rows per block, columns per block, threads per block,
 * K slices} of the launch qd_conv2d_i8(d, stream) would make NOW — the state of qd_conv_config and of the environment knobs
 * the library read (QD_KGROUPS, QD_WIDE_MINK, QD_WIDE_MINBLK, QD_SPLITK_TARGET) included; d->splitk_ws / splitk_ws_bytes decide
 * as they do for the launch (K slices > 1 = the split-K schedule: that many partial contractions plus the finalise pass).
 * Threads per block is 512 for the two-K-group block of qd_conv_config, 256 otherwise.  The descriptor goes through the
 * launcher's own checks and tile choice with the launch withheld, so the answer cannot drift from the launcher; it returns
 * non-zero with qd_last_error wherever qd_conv2d_i8 would refuse the descriptor.  Nothing is launched and no pointer of the
 * descriptor is followed (null tests and alignment only).  For tests, which assert with it the tile a case was written for,
 * and for tools; not on any launch path.  The exact-accumulator hook qd_conv2d_i8_acc always takes 128-row tiles. */
int qd_conv2d_i8_form(const qd_conv_desc* d, int32_t* form4);

/* K2b  tile-ordered int4 packer for the LDS-DMA contraction kernel (csrc/igemm_dma.hip).  Same code
 *     formula as qd_pack_weights (adaptive_rounding.py:49-59).  Output wt[kstep][ntile][1024 B]:
 *     kstep enumerates (tap, 64-channel step) of the slice starting at kstep0, ntile = n/32, and each
 *     1-KB block is [ksub(2)][half(2)][n%32][8 B] = the 16 nibbles of row n for
 *     K = ksub*32 + half*16 + 0..15 (nibble order inside the 8 bytes as in qd_pack_weights mode 4).
 *     The stored operand is the RAW code W (0..15); its zero point is restored in the epilogue
 *     through qd_conv_seg.zw[n] = zw[n] and activation row sums.  wsum[n] += sum W over the slice. */
int qd_pack_weights_t4(const float* w, const float* alpha, const float* delta, const float* zp,
                       int Cout, int Cin_total, int taps, int c0, int clen, int clen_pad, int n_levels,
                       uint8_t* wt, int kstep0, int ntiles, int32_t* wsum, void* stream);

/* K2c  the same tile order for 8-bit weights: wt[kstep][ntile][2 KB], each block [ksub(2)][half(2)][n%32][16 B] =
 *     the 16 stored bytes W-128 of row n for K = ksub*32 + half*16 + 0..15 (qd_conv_desc.wbits = 8, w_tiled = 1,
 *     qd_conv_seg.zw[n] = zw[n]-128).  wsum[n] += sum (W-128) over the slice. */
int qd_pack_weights_t8(const float* w, const float* alpha, const float* delta, const float* zp,
                       int Cout, int Cin_total, int taps, int c0, int clen, int clen_pad, int n_levels,
                       uint8_t* wt, int kstep0, int ntiles, int32_t* wsum, void* stream);

/* Test hook: same contraction, but writes the raw int32 I_s[m][n] of segment 0 (after zero-point
 * restoration) to iout[M][Cout].  Used for the bit-exact accumulator tests (oracle tier T0). */
int qd_conv2d_i8_acc(const qd_conv_desc* d, int32_t* iout, void* stream);

/* ------------------------------------------------------------------------------------------
 * K6  timestep-embedding MLPs.   Replaces `time_embed` = Linear -> SiLU -> Linear (ldm openaimodel.py:758-759; ddim
 *     diffusion.py:318-320) and the per-ResBlock `emb_layers` / `temb_proj` = SiLU -> Linear on the shared embedding
 *     (openaimodel.py:225-232 with qdiff/quant_block.py:98-107; ddim diffusion.py:127), every Linear a QuantModule
 *     (quant_layer.py:248-279) on M = batch rows: one launch evaluates n_layers Linears that share the input x [B][K]
 *     (fp32, row stride ldx): out[b][layer.out_off + n] = Linear_layer(act_quant_layer(silu?(x)))[b][n].
 *     layers: DEVICE array of n_layers records, 64 bytes each:
 *         { const uint8_t* w (tile-ordered weights, first K-step of the only segment); const float* scale;
 *           const int32_t* zc; const int32_t* zw; const float* bias; const float* qparams (float[4]);
 *           const int32_t* zfill; int32_t Cout; int32_t out_off; }          (semantics of qd_conv_seg / qd_conv_desc)
 *     blocks: DEVICE int32 [n_blocks][2] = {layer index, first output channel}: one workgroup per 64 output channels.
 *     qmin/qmax/off: the (common) activation grid.  B*K must fit LDS (<= ~44 KB): callers split taller batches.
 *     Results equal qd_quantize_act + qd_conv2d_i8 on the same SiLU values bit for bit (same integers, same float order).
 * ------------------------------------------------------------------------------------------ */
int qd_temb_mlp(const float* x, int64_t ldx, int B, int K, int apply_silu, const void* layers, int n_layers,
                const int32_t* blocks, int n_blocks, int wbits, int qmin, int qmax, int off, float* out, int64_t ldo,
                void* stream);

/* K6w  (additive in ABI 20) the same Linears in the weights-only state (weight_quant, act_quant) = (True, False)
 *     (quant_layer.py:620-631: the fp Linear of the fake-quantised weight; openaimodel.py:758-759 `time_embed`,
 *     openaimodel.py:225-232 with qdiff/quant_block.py:98-107 `emb_layers`, ddim diffusion.py:127 `temb_proj`, 318-320
 *     `temb.dense`), which ran as a torch SiLU, a qd_rows_to_h16 and a qd_conv2d_wq_h16 launch per Linear.  One launch
 *     evaluates n_layers Linears that share the fp32 input x [B][K] (row stride ldx, rows 16-byte aligned, K % 16 == 0):
 *         out[b][out_off_l + n] = delta_l[n] * sum_k r(silu?(x[b][k])) * (q_l[k][n] - z_l[n]) + bias_l[n]
 *     r: the one rounding to act_dtype (QD_F16 / QD_BF16, nearest even, as qd_rows_to_h16); silu = x / (1 + exp(-x)) in
 *     fp32 as in qd_temb_mlp; q: the tile-ordered codes of qd_pack_weights_t4 / _t8 (the array qd_conv2d_wq_h16 reads);
 *     z: the RAW weight zero point, subtracted from the code before the multiply (no row sums); fp32 accumulation.
 *     layers: DEVICE array of n_layers records, 40 bytes each:
 *         { const uint8_t* w (first K-step of the layer's ONLY segment: the caller checks that there is one);
 *           const float* delta; const int32_t* z; const float* bias (or NULL); int32_t Cout; int32_t out_off; }
 *     blocks: DEVICE int32 [n_blocks][2] = {layer index, first output channel}: one workgroup per 64 output channels.
 *     Any B > 0 (32-row MFMA tiles).  Each output element is accumulated exactly as qd_conv2d_wq_h16 accumulates it unsplit (the
 *     same instruction, K order and epilogue), so the results equal that path's bit for bit whenever the SiLU values do.
 *     Columns of out outside every [out_off_l, out_off_l + Cout_l) are never written.  bf16 operands carry q - z exactly
 *     only while |q - z| <= 256 (the caller checks, as for qd_conv2d_wq_h16). */
int qd_temb_mlp_wq_h16(const float* x, int64_t ldx, int B, int K, int apply_silu, const void* layers, int n_layers,
                       const int32_t* blocks, int n_blocks, int wbits, int act_dtype, float* out, int64_t ldo,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  GroupNorm -> SiLU -> quantise.   Replaces nn.GroupNorm(32,C) / GroupNorm32 → x*sigmoid(x)
 *     → act_quantizer of the following QuantModule (ddim/models/diffusion.py:121-123,127-130;
 *     ldm/modules/diffusionmodules/openaimodel.py:201-205,225-232, util.py:214-216;
 *     qdiff/quant_layer.py:82-88).  x is channels-last [B][S][C] (ldx = row stride, elements).
 *     ws: workspace of qd_groupnorm_ws_bytes(B,C,S) bytes.  apply_silu=0 gives GroupNorm→quant
 *     (attention blocks: openaimodel.py:324, attention.py:280-281, ddim diffusion.py:175).
 *     Two-quantizer outputs are not needed here (split only affects 1x1 skips).
 *     If yout != NULL the fp32 normalised (+SiLU) tensor is also written ([B*S][ldy]).
 *     part_in != NULL: the first statistics level was already produced by the kernel that wrote x
 *     (qd_conv_desc.gn_part: [B][nchunk_in][part_ld >= C][2] sums / sums of squares per row chunk; part_ld = 0
 *     means C); the statistics pass over x is skipped.
 *     raw != NULL (and raw->out != NULL): see qd_raw_quant above.
 * ------------------------------------------------------------------------------------------ */
/* Optional second output of qd_groupnorm_silu_quant: the RAW (un-normalised) input quantised for another consumer of
 * the same tensor, i.e. the 1x1 skip connection of a residual block, which reads the very tensor `in_layers` normalises
 * (qdiff/quant_block.py:108-111; openaimodel.py:266-278), with up to two channel segments that carry their own
 * activation quantisers (the split shortcut, quant_layer.py:257-269).  Codes are those of qd_quantize_act, written to
 * out[row][oc0 + (c - c0)] for c in [c0, c0 + clen); c0 / clen / oc0 are multiples of 16.                               */
typedef struct {
    int32_t      c0, clen, oc0;
    int32_t      qmin, qmax, off;
    const float* qparams;
} qd_raw_seg;
typedef struct {
    int8_t*    out;       /* [B*S][ldo] int8 rows of the consumer (NULL: no raw output) */
    int64_t    ldo;
    int32_t    nseg;      /* 1 or 2 */
    int32_t    _pad;
    qd_raw_seg seg[2];
} qd_raw_quant;

int64_t qd_groupnorm_ws_bytes(int64_t B, int64_t C, int64_t S);
int qd_groupnorm_silu_quant(const void* x, int x_dtype, int64_t B, int64_t S, int C, int64_t ldx,
                            int groups, float eps, const float* gamma, const float* beta,
                            int apply_silu,
                            const float* qparams, int qmin, int qmax, int off,
                            int8_t* out, int64_t ldo, float* yout, int64_t ldy,
                            void* ws, const float* part_in, int nchunk_in, int64_t part_ld, const qd_raw_quant* raw,
                            void* stream);
/* The same for the second norm of a `use_scale_shift_norm` residual block (qdiff/quant_block.py:99-103, openaimodel.py:
 * 266-272: `h = out_norm(h) * (1 + scale) + shift`, then SiLU -> Dropout -> conv): mod holds one fp32 row per sample,
 * [B][mod_ld >= 2 C] = scale | shift, the two halves of the block's embedding projection (th.chunk(emb_out, 2, dim=1)).
 * The modulation is folded into the per-(sample, channel) affine of the normalisation; no raw second output.            */
int qd_groupnorm_mod_silu_quant(const void* x, int x_dtype, int64_t B, int64_t S, int C, int64_t ldx,
                                int groups, float eps, const float* gamma, const float* beta,
                                int apply_silu,
                                const float* qparams, int qmin, int qmax, int off,
                                int8_t* out, int64_t ldo, float* yout, int64_t ldy,
                                void* ws, const float* part_in, int nchunk_in, int64_t part_ld,
                                const float* mod, int64_t mod_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9a LayerNorm -> quantise (up to 3 consumers).  Replaces nn.LayerNorm (attention.py:229-231)
 *     followed by the act_quantizers of to_q/to_k/to_v (or the GEGLU proj) QuantModules.
 *     x: [M][C] rows (ldx elements).  nout in 1..3; out[i] int8 [M][ldo].
 * ------------------------------------------------------------------------------------------ */
int qd_layernorm_quant(const void* x, int x_dtype, int64_t M, int C, int64_t ldx, float eps,
                       const float* gamma, const float* beta, int nout,
                       const float* const* qparams, const int* qmin, const int* qmax, const int* off,
                       int8_t* const* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9b GEGLU -> quantise.  Replaces `x, gate = proj(x).chunk(2,-1); x*F.gelu(gate)`
 *     (ldm/modules/attention.py:42-44) + the act_quantizer of the FF output Linear.
 *     h: [M][2F] (ldh), out int8 [M][ldo].
 * ------------------------------------------------------------------------------------------ */
int qd_geglu_quant(const void* h, int h_dtype, int64_t M, int F, int64_t ldh,
                   const float* qparams, int qmin, int qmax, int off,
                   int8_t* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * K7/K8 quantised attention.   Replaces the q/k/v/probability quantisers + the two einsum/bmm
 *     contractions + fp32 softmax of cross_attn_forward (qdiff/quant_block.py:190-221),
 *     QuantQKMatMul/QuantSMVMatMul (:123-134,152-157 with openaimodel.py:384-406) and
 *     QuantAttnBlock.forward (:354-386).
 *
 *     Step 1  qd_quantize_heads: x logical [B][T][H][d] (element strides sb, st, sh, sd),
 *             y = x*prescale quantised like K1 and written head-major:
 *               transpose=0:  out[(b*H+h)][Tpad][dpad]  (+ rsum[(b*H+h)][Tpad] = row sums)
 *               transpose=1:  out[(b*H+h)][dpad][Tpad] with the key index permuted inside each
 *                             32-key tile   (+ rsum[(b*H+h)][dpad] = column sums)
 *             Padding rows/cols are zero bytes; buffers must be Tpad = ceil32(T), dpad = ceil32(d).
 *     Step 2  qd_attn_i8: for every (b,h): S = (q-zq)(k-zk)^T * cs ; P = softmax_j(S);
 *             u = clamp(rint(P/dw)+zpw, wmin, wmax);  O = sum_j (u-zpw)(v-zv) * dw*dv.
 *             O is written as out[b][t][h*d + c] (merged heads, ldo = row stride, fp32).
 *     prm: device float[16] = {cs (=dq*dk*scale), zq', zk', dw, zpw, dv_dw (=dw*dv), zv', ...}
 *          (layout in DESIGN.md §4.4); built once on device by the host, never read back.
 *     out8 != NULL: O is not written as fp32 but quantised with oq_* = the act quantiser of the Linear that
 *           consumes it (to_out[0], quant_block.py:221 -> quant_layer.py:256) and stored as its int8 input rows
 *           out8[b*T+t][ldo8] (K1 semantics; H*d must already be that Linear's padded input width).
 *           The row stride of the output written (ldo8, else ldo) must be below 2^24 elements: the epilogue addresses
 *           the 32 rows of a wave with 32-bit byte offsets from one 64-bit row base.
 *     q_asym: 0 when zq' == 0 (symmetric q quantiser), else 1: the kernel then restores the per-key term
 *           -zq' * sum_d k'[j][d].  qsum is ignored (may be NULL): the per-query terms -zk'*qsum_i + d*zq'*zk' are
 *           constant along a softmax row and cancel exactly.
 *     kterm (ABI 18; the slot that used to be `ksum`): NULL, or the table qd_attn_keyterm wrote for THIS k operand and
 *           THIS prm.  Shapes with qd_attn_uses_keyterm(d, S, q_asym) == 1 (SD's 4096-token level; the rule: next paragraph)
 *           then seed the score accumulators from the table instead of issuing constant-operand MFMAs (2 of the 4
 *           score MFMAs of a 32x32 tile carried no data); results are bit-identical with and without it.  Other shapes
 *           ignore it.
 *     Which kernel runs: ONE rule, the table of DESIGN.md §4.4 (head dim, key count, q symmetry, table present, the knobs of
 *           qd_attn_config -> kernel family / per-key term mode / launches).  qd_attn_i8_form answers it for a call;
 *           qd_attn_uses_keyterm and qd_attn_ws_bytes are its corollaries for a shape.
 *     qd_attn_keyterm: kterm[bh][j] = 0x4B400000 - zq' * sum_{c < dpad} k[bh][j][c]  (int32 [BH][Spad], dpad 32, 64 or 96; pad
 *           bytes of k are zero).  One pass over the K operand; recompute whenever k or prm[1] changes — a cross-attention
 *           whose context is constant over a sampling run computes it once (quant_block.py:193-195 recomputes k per step).
 *     qd_attn_config: process-wide launcher knobs, -1 = leave unchanged.  pipe_mode 0 = register-fed kernel everywhere,
 *           2 = LDS-staged kernel where it pays (default), 3 = LDS-staged wherever eligible; xcd 0/1 = XCD-aware block
 *           order; ktab 0 = ignore kterm (constant-operand MFMAs, A/B runs); lean 0 = attn_kernel for every head dim, 1 = lean /
 *           LDS-staged kernels for d < 64 (default), 3 = also d = 80 on the lean kernel (measured slower).  Initial values:
 *           QD_ATTN_PIPE / QD_ATTN_XCD / QD_ATTN_KTAB / QD_ATTN_LEAN, read once.
 *     ws / ws_bytes (ABI v20): scratch of the LDS-staged path, which runs as THREE launches since round 6 — per-query softmax
 *           statistics first (sweep 1 at up to 6 waves per SIMD), then the probability / P.V sweep for blocks that need only the
 *           lo operand bytes of the 16-bit codes (4 waves per SIMD) and for the others (3): 16 bytes per padded query + 4 per
 *           128-query block.  qd_attn_ws_bytes(BH, T, S, d) is the size for a shape (0: the shape runs on a one-kernel path
 *           and ws may be NULL); contents are undefined afterwards, one buffer may serve every call of a stream.
 * ------------------------------------------------------------------------------------------ */
int qd_quantize_heads(const void* x, int x_dtype, int B, int T, int H, int d,
                      int64_t sb, int64_t st, int64_t sh, int64_t sd, float prescale,
                      const float* qparams, int qmin, int qmax, int off, int transpose,
                      int8_t* out, int32_t* rsum, int Tpad, int dpad, void* stream);

int qd_attn_uses_keyterm(int d, int S, int q_asym);
int qd_attn_keyterm(const int8_t* k, int BH, int Spad, int dpad, const float* prm, int32_t* kterm, void* stream);
void qd_attn_config(int pipe_mode, int xcd, int ktab, int lean);
int64_t qd_attn_ws_bytes(int BH, int T, int S, int d);
int qd_attn_i8(const int8_t* q, const int8_t* k, const int8_t* vt,
               const int32_t* qsum, const int32_t* kterm, const int32_t* vsum,
               int BH, int H, int T, int S, int d, int Tpad, int Spad, int dpad,
               const float* prm, int wbits, int wmin, int wmax, int q_asym,
               float* out, int64_t ldo,
               int8_t* out8, int64_t ldo8, const float* oq_params, int oq_min, int oq_max, int oq_off,
               void* ws, int64_t ws_bytes, void* stream);
/* qd_attn_i8_qp (additive in ABI 20): qd_attn_i8 whose query operand has a head PERIOD.  q (and qsum) hold q_heads heads,
 * [q_heads][Tpad][dpad]; head bh of the launch reads the q rows of head bh % q_heads.  Everything else stays per bh: k, vt, vsum,
 * kterm, the workspace, the output rows.  BH % q_heads == 0 and q_heads % H == 0 (whole samples repeat).  q_heads = BH is
 * qd_attn_i8, which is implemented as exactly that call; every launch form (attn_kernel, the lean kernel, the statistics + P.V
 * launches) takes the period.  Cross-attention of a classifier-free-guidance batch: both halves share the queries, each half has
 * its own context. */
int qd_attn_i8_qp(const int8_t* q, const int8_t* k, const int8_t* vt,
                  const int32_t* qsum, const int32_t* kterm, const int32_t* vsum,
                  int BH, int H, int T, int S, int d, int Tpad, int Spad, int dpad,
                  const float* prm, int wbits, int wmin, int wmax, int q_asym,
                  float* out, int64_t ldo,
                  int8_t* out8, int64_t ldo8, const float* oq_params, int oq_min, int oq_max, int oq_off,
                  void* ws, int64_t ws_bytes, void* stream, int q_heads);
/* qd_attn_i8_form (additive in ABI 20): the launch form qd_attn_i8_qp would take for these arguments under the current knobs —
 * the launcher's own checks and kernel choice with the launch withheld: no HIP call, no pointer followed; it refuses what the
 * launcher refuses, with the launcher's message.  The stream's slot holds form4 (4 ints, host memory):
 *   form4[0] kernel family: 0 attn_kernel, 1 register-fed lean kernel, 2 LDS-staged (statistics + two P.V launches)
 *   form4[1] DT = dpad / 32
 *   form4[2] families 1, 2: per-key term mode, 0 none (symmetric q) / 1 constant-operand MFMAs / 2 key-term table; family 0: q_asym
 *   form4[3] launches: 1, or 3 for family 2 */
int qd_attn_i8_form(const int8_t* q, const int8_t* k, const int8_t* vt,
                    const int32_t* qsum, const int32_t* kterm, const int32_t* vsum,
                    int BH, int H, int T, int S, int d, int Tpad, int Spad, int dpad,
                    const float* prm, int wbits, int wmin, int wmax, int q_asym,
                    float* out, int64_t ldo,
                    int8_t* out8, int64_t ldo8, const float* oq_params, int oq_min, int oq_max, int oq_off,
                    void* ws, int64_t ws_bytes, int32_t* form4, int q_heads);

/* ------------------------------------------------------------------------------------------
 * K7s/K8s  the two attention contractions as standalone batched integer GEMMs, for callers that use
 *     QuantQKMatMul / QuantSMVMatMul on their own (qdiff/quant_block.py:114-160 with the softmax applied by the
 *     caller in between, ldm openaimodel.py:384-406).  Operands are the same qd_quantize_heads layouts.
 *     qd_bmm_qk_i8: out[bh][t][s] = cs * sum_d (q'-zq')(k'-zk')   prm = {cs, zq', zk'} (device floats);
 *                   out rows have stride ldo, heads stride bstride (elements).
 *     qd_bmm_pv_i8: w[bh][t][s] fp32 probabilities (row stride ldw, head stride wbstride) are quantised with
 *                   u = clamp(rint(w/dw)+zpw, wmin, wmax) and contracted with v:
 *                   out[bh][c][t] = dw*dv * sum_s (u-zpw)(v'-zv')   ("bct": row stride ldo, head stride obstride);
 *                   vt / vsum = transpose=1 output of qd_quantize_heads; prm[3..6] = {dw, zpw, dw*dv, zv'}.
 *                   wbits 8 or 16, wmax - wmin < 2^wbits.  Bounds on S (refused with a message, nothing is launched): the
 *                   kernel sums a query's S codes and accumulates the lo / hi code bytes against v' in int32, so
 *                   S * (wmax - wmin) < 2^31 (S <= 32768 for a full 16-bit grid) and S < 131072 (S products of at most
 *                   128 * 128 = 2^14 per byte accumulator); everything after the accumulators is 64-bit.
 *     Both refuse a head-dim pad outside {32, 64, 96, 128, 160, 256}.
 * ------------------------------------------------------------------------------------------ */
int qd_bmm_qk_i8(const int8_t* q, const int8_t* k, int BH, int T, int S, int d, int Tpad, int Spad, int dpad,
                 const float* prm, float* out, int64_t ldo, int64_t bstride, void* stream);
int qd_bmm_pv_i8(const float* w, int64_t ldw, int64_t wbstride, const int8_t* vt, const int32_t* vsum,
                 int BH, int T, int S, int d, int Spad, int dpad, const float* prm, int wbits, int wmin, int wmax,
                 float* out, int64_t ldo, int64_t obstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibration: fused fake-quantisation of an activation tensor, forward and backward, for the
 *     step-size phase of block / layer reconstruction (qdiff/block_recon.py:72-110 trains `delta` by autograd through
 *     UniformAffineQuantizer.forward, quant_layer.py:82-88, with the straight-through rounding of :16-20).
 *     y      = (clamp(rint(x / delta) + zp, qmin, qmax) - zp) * delta
 *     gx     = d(loss)/dx       (the gradient passes where the un-clamped code lies in [qmin, qmax])
 *     gdelta_part[b] = block b's share of d(loss)/d(delta); the caller sums qd_fakequant_blocks(n) partials.
 *     delta / zero_point are device scalars (the reference keeps them as tensors / Parameters).  fp32 only.
 * ------------------------------------------------------------------------------------------ */
int64_t qd_fakequant_blocks(int64_t n);
int qd_fakequant_fwd(const float* x, int64_t n, const float* delta, const float* zero_point, int qmin, int qmax, float* y,
                     void* stream);
int qd_fakequant_bwd(const float* x, const float* gy, int64_t n, const float* delta, const float* zero_point, int qmin, int qmax,
                     float* gx, float* gdelta_part, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibration: fused AdaRound quantiser of a weight tensor, forward, backward and rounding
 *     regulariser, for the weight phase of block / layer reconstruction.  Replaces the autograd composition of
 *     AdaRoundQuantizer.forward / get_soft_targets (qdiff/adaptive_rounding.py:39-74) and the second evaluation of the soft
 *     targets by the regulariser of LossFunction.__call__ (qdiff/block_recon.py:217-229).
 *     The quantiser is channel-wise: row r of `rows` is the `cols` floats at w + r * ldw (ldw >= cols: the two halves of a
 *     split shortcut are read in place); gw of the backward likewise with row stride ldg >= cols (a half receives a channel
 *     slice of the concatenated weight's gradient); delta / zero_point hold `rows` floats; alpha, w_hat, galpha are dense
 *     [rows][cols] and 16-byte aligned.  w and gw need no alignment beyond their type: rows that do not start on 16 bytes
 *     are read float by float.  rows * cols < 2^31.  fp32 only.  FP contraction is off; the operation order is autograd's.
 *       base = floor(w / delta); s = 1 / (1 + exp(-alpha)); hr = s * (zeta - gamma) + gamma; h = clamp(hr, 0, 1);
 *       c = base + h + zp;  w_hat = (clamp(c, 0, n_levels - 1) - zp) * delta
 *     reg_b > 0: reg_part[k] = block k's share of sum(1 - (|h - 0.5| * 2)^reg_b), the fp32 terms added in fp64; the caller
 *     sums qd_adaround_blocks(rows, cols) partials in fp64 and rounds once.  reg_b <= 0: no regulariser, reg_part may be null.
 *     Backward (recomputes everything from w and alpha):
 *       rec = gw * delta, 0 unless 0 <= c <= n_levels - 1, 0 unless 0 <= hr <= 1, * (zeta - gamma), * (1 - s) * s
 *       reg = -greg[0] * (b * v^(b - 1)) * 2 * sgn(h - 0.5) with v = |h - 0.5| * 2, 0 unless 0 <= hr <= 1, * (zeta - gamma),
 *             * (1 - s) * s          (only with greg, a DEVICE scalar d(loss)/d(reg sum), non-null and reg_b > 0)
 *       galpha = rec + reg
 * ------------------------------------------------------------------------------------------ */
int64_t qd_adaround_blocks(int64_t rows, int64_t cols);
int qd_adaround_fwd(const float* w, int64_t rows, int64_t cols, int64_t ldw, const float* alpha, const float* delta,
                    const float* zero_point, int n_levels, float gamma, float zeta, float reg_b, float* w_hat, double* reg_part,
                    void* stream);
int qd_adaround_bwd(const float* gw, int64_t ldg, const float* w, int64_t rows, int64_t cols, int64_t ldw, const float* alpha,
                    const float* delta, const float* zero_point, int n_levels, float gamma, float zeta, float reg_b,
                    const float* greg, float* galpha, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibration: fused MSE range search that INITIALISES a quantiser.  Replaces the LAPQ-style loop over
 *     80 shrink factors of UniformAffineQuantizer.init_quantization_scale with scale_method = 'mse' (reference
 *     qdiff/quant_layer.py:138-140 channel-wise, :162-177 the search, :183-190 quantize()): per factor a quantise and an
 *     L_2.4 score over the whole tensor, ~14 launches each.
 *     Geometry: `rows` rows of `cols` consecutive floats, row r at x + r * ldx (ldx >= cols when rows > 1; 4-byte aligned:
 *     a channel slice is read in place).  per_row = 1: one search per row, G = rows groups (channel-wise weights).
 *     per_row = 0: ONE search over all rows together, G = 1 (an activation tensor; the x[:, :split] / x[:, split:] slices
 *     of a split layer's input as B strided rows).  rows * cols < 2^31.  fp32 only.
 *     factors: n_cand (1..80) shrink factors f_i; the host passes float32(1.0 - i * 0.01).  levels = 2^n_bits - 1 divides
 *     the range, qmax = n_levels - 1 clamps the codes (they differ for a symmetric quantiser, as in the reference).
 *     Per group and candidate i, operation by operation (no contraction, IEEE division), as ATen evaluates the
 *     composition on the device — it divides a tensor by a host scalar as a product with the scalar's fp32 reciprocal:
 *       hi = x_max * f_i;  lo = x_min * f_i;  d = (always_zero ? hi : hi - lo) * (1.0f / levels)
 *       z  = always_zero ? 0 : rint(-lo / d)
 *       per element:  c = clamp(rint(x / d) + z, 0, qmax);  xq = (c - z) * d;  term = |x - xq|^2.4     (fp32, powf)
 *       score_i = mean of the terms: a lane adds at most 8 terms in fp32, everything after that in fp64 in a fixed order;
 *                 the fp64 total is divided by the element count and rounded to fp32 once
 *     Selection: best = 1e10f, ascending i, i taken only when score_i < best.  Nothing taken: index = -1 and
 *     delta = zero_point = 0.  NaN as in ATen: x_min / x_max of a group holding a NaN are NaN, clamp keeps a NaN, a NaN
 *     score is never better — so a constant row (d = 0, z = -inf) and a row of zeros (z = NaN) take nothing.
 *     Outputs: delta, zero_point, x_min, x_max, index hold G values; scores (may be null) holds [G][n_cand].
 *     ws: qd_mse_search_ws_bytes(rows, cols, per_row, n_cand) bytes, 16-byte aligned (0 bytes: may be null).
 *     qd_mse_search_form: the launch form the library takes, the one rule —  per_row = 1: one launch, a block per row,
 *     QD_MSE_FORM_WAVE (64 threads) when cols <= 512, else QD_MSE_FORM_BLOCK (256);  per_row = 0: QD_MSE_FORM_SPREAD, three
 *     launches (min / max partials; [block][n_cand] fp64 partial sums; finalise).  -1 for an empty tensor.
 *     No floating-point atomics: results are bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
enum { QD_MSE_FORM_WAVE = 0, QD_MSE_FORM_BLOCK = 1, QD_MSE_FORM_SPREAD = 2 };
int qd_mse_search_form(int64_t rows, int64_t cols, int per_row);
int64_t qd_mse_search_ws_bytes(int64_t rows, int64_t cols, int per_row, int n_cand);
int qd_mse_search(const float* x, int64_t rows, int64_t cols, int64_t ldx, int per_row, const float* factors, int n_cand,
                  int levels, int qmax, int always_zero, float* delta, float* zero_point, float* x_min, float* x_max,
                  int32_t* index, float* scores, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * First-stage decoder: the convolutions of the KL-f8 / VQ-f4 `Decoder`
 *     (ldm/modules/diffusionmodules/model.py:465-572 `Decoder.forward`: conv_in, ResnetBlock :80-141, AttnBlock :144-196
 *     q/k/v/proj_out, Upsample :48-63 nearest-2x + conv, conv_out; called from ldm/models/autoencoder.py:330-333 `decode`
 *     and ldm/models/diffusion/ddpm.py `decode_first_stage`) as bf16 x bf16 -> fp32 implicit GEMMs on
 *     v_mfma_f32_32x32x16_bf16 — the loader, ring and epilogue of qd_conv2d_i8 in its floating-point mode.
 *
 *     qd_conv2d_bf16: same descriptor as qd_conv2d_i8 with
 *         x          bf16 channels-last rows [B*H*W][ldx]; ldx, seg[0].c0, seg[0].clen count bf16 ELEMENTS (multiples of 8)
 *         w          tile-ordered bf16 of qd_pack_weights_bf16 (wbits = 16, w_tiled = 1)
 *         nseg = 1, epilogue = QD_EPI_LINEAR; seg[0].scale / zc / zw / zfill / fill16 unused (out-of-image taps read 0)
 *         out        out[m][n] = sum_k x w + bias[n] (+ residual[m][n]); out_dtype = QD_F32 or QD_BF16, the residual has
 *                    the type of the output
 *         gn_part, upsample2x, kh/kw/stride/pad as for qd_conv2d_i8; rowbias, split-K, oq_* / hd_* unused.
 *     qd_pack_weights_bf16: fp32 [Cout][Cin][taps] (OIHW) -> bf16 (round to nearest even) in the order the kernel reads:
 *         per (tap, 32-channel K-step, 32-output-channel tile) 2 KB as [k-half (16 ch)][lane-half (8 ch)][n % 32][8 bf16];
 *         channels Cin .. clen_pad-1 (clen_pad % 8 == 0 = the descriptor's clen) are zero.  wt: qd_pack_weights_bf16_bytes.
 *     qd_groupnorm_silu_bf16: GroupNorm (+ SiLU) of fp32 rows into bf16 rows (model.py:38-45 `Normalize` / `nonlinearity`
 *         in front of every convolution); ws / part_in / nchunk_in / part_ld as for qd_groupnorm_silu_quant.
 *
 *     fp16 operands (ABI 18): the reference decodes under fp16 autocast (scripts/txt2img.py:231-236), i.e. with IEEE halves
 *     (11 significant bits) where bf16 has 8.  Same kernels, same bytes per K-step, v_mfma_f32_32x32x16_f16 at the same rate:
 *         qd_pack_weights_h16(..., wbits, ...)     wbits 16 = bf16 (what qd_pack_weights_bf16 does), 17 = fp16
 *         qd_conv2d_bf16 with desc.wbits = 17      x / w are halves; out_dtype QD_F32 or QD_F16 (residual of that type)
 *         qd_groupnorm_silu_h16(..., out_dtype, ...)  QD_BF16 or QD_F16 rows
 * ------------------------------------------------------------------------------------------ */
int qd_conv2d_bf16(const qd_conv_desc* d, void* stream);
int64_t qd_pack_weights_bf16_bytes(int Cout, int taps, int clen_pad);
int qd_pack_weights_bf16(const float* w, int Cout, int Cin, int taps, int clen_pad, uint8_t* wt, void* stream);
int qd_groupnorm_silu_bf16(const float* x, int64_t B, int64_t S, int C, int64_t ldx, int groups, float eps,
                           const float* gamma, const float* beta, int apply_silu, void* out, int64_t ldo, void* ws,
                           const float* part_in, int nchunk_in, int64_t part_ld, void* stream);
int qd_pack_weights_h16(const float* w, int Cout, int Cin, int taps, int clen_pad, int wbits, uint8_t* wt, void* stream);
int qd_groupnorm_silu_h16(const float* x, int64_t B, int64_t S, int C, int64_t ldx, int groups, float eps,
                          const float* gamma, const float* beta, int apply_silu, int out_dtype, void* out, int64_t ldo, void* ws,
                          const float* part_in, int nchunk_in, int64_t part_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weights-only layers (additive in ABI 20).  Replaces the (weight_quant, act_quant) = (True, False) state of
 *     QuantModule.forward (qdiff/quant_layer.py:620-631: fwd_func on the fake-quantised fp32 weight, i.e.
 *     F.conv2d / F.conv1d / F.linear of quant_layer.py:276 with UniformAffineQuantizer / AdaRoundQuantizer applied to the
 *     weight only, quant_layer.py:82-88, adaptive_rounding.py:49-61) by a contraction of the PACKED weight codes with fp16 or
 *     bf16 activations and fp32 accumulation (v_mfma_f32_32x32x16_f16 / _bf16):
 *        out[m][n] = sum_seg delta_s[n] * sum_k x[m][k] * (q_s[k][n] - z_s[n]) + bias[n] (+ residual[m][n])
 *     The zero point is subtracted from the code in registers (no activation row sums), so every product is exact in fp32.
 *
 *     qd_conv2d_wq_h16: the descriptor of qd_conv2d_i8 with
 *         x          fp16 (act_dtype = QD_F16) or bf16 (QD_BF16) channels-last rows [B*H*W][ldx] of qd_rows_to_h16;
 *                    ldx, seg.c0, seg.clen count ELEMENTS (multiples of 8); channels of a segment past its real width
 *                    must be zero (qd_rows_to_h16 writes them so)
 *         w          the tile-ordered codes of qd_pack_weights_t4 (wbits = 4) / _t8 (wbits = 8), w_tiled = 1, seg.kstep0
 *                    as for qd_conv2d_i8: the packs of the integer path serve this mode unchanged
 *         seg.scale  [Cout] delta_w[n] of the segment's weight quantiser;  seg.zw: [Cout] its RAW zero point z[n]
 *                    in [-128, 255] (not zw - 128);  seg.zc / zfill / fill16 must be NULL
 *         nseg 1 or 2 (split shortcut, quant_layer.py:257-269: each segment its own delta / z), epilogue = QD_EPI_LINEAR
 *         (or QD_EPI_GEGLU_H16, below), out_dtype QD_F32 or QD_F16 (the residual has the type of the output), kh/kw/stride/pad_t/pad_l as for
 *         qd_conv2d_i8; out-of-image taps, K tails and M tails read zeros.  gn_part, upsample2x must be unset;
 *         oq_* / hd_* are ignored.
 *         splitk_ws  optional fp32 scratch (16-byte aligned).  The launch is contracted split-K only when
 *                    splitk_ws is non-NULL, splitk_ws_bytes >= nsplit * M * Cout * 4 and the policy returns nsplit >= 2
 *                    (qd_conv2d_wq_h16_splitk_ws_bytes(d) != 0); otherwise it is the one launch it always was, the same
 *                    bytes.  Split: grid = tiles x nsplit, slice s contracts the K-steps [s * it_per, (s + 1) * it_per) of
 *                    the order segment, tap, 64-channel step and writes its scaled fp32 partial to ws[s][m][n]; a second
 *                    launch sums the slices in index order (no atomics: the same bits from run to run) and adds bias,
 *                    rowbias and residual as the unsplit epilogue does.  Both segment counts; QD_EPI_GEGLU_H16 never splits.
 *                    The fp32 sum is associated differently from the unsplit launch: results agree to rounding, not bit
 *                    for bit.
 *         rowbias    optional fp32 [B][ld_rowbias] (ld_rowbias >= Cout): row b is added to every output row of sample b
 *                    after the bias and before the residual, as in qd_conv2d_i8 (the timestep-embedding add
 *                    `h + emb_out` of qdiff/quant_block.py:92-98).  NULL leaves the output bytes as they were.
 *         epilogue = QD_EPI_GEGLU_H16: the layer is a GEGLU projection, Cout = 2 F with F % 32 == 0, and w was
 *                    packed with its rows in 32-row tiles interleaved value, gate, value, ... (qdiff.engine.geglu_row_perm;
 *                    seg.scale, seg.zw and bias in that order too).  out then receives the operand rows of the next layer,
 *                    out[m][f] = value * gelu(gate) with value / gate the affine results of features f and F + f, gelu through
 *                    the erf of qd_geglu_h16, rounded ONCE to out_dtype = act_dtype; [M][ldo] with ldo >= F, ldo % 8 == 0,
 *                    16-byte aligned, channels [F, ldo) written as zeros.  One segment, no residual, no rowbias.  The bytes
 *                    are those of the linear epilogue (fp32 out, un-permuted pack) followed by qd_geglu_h16.
 *         bf16 operands carry q - z exactly only while |q - z| <= 256 for every stored code: the caller checks (8-bit
 *         codes with z < -1 can exceed it); fp16 is exact for every zero point in [-128, 255].
 *     qd_rows_to_h16: the producer of those rows.  x is a logical [B][C][S] fp32 / fp16 / bf16 tensor addressed by element
 *         strides (sb, sc, ss) as in qd_quantize_act; channels [c0, c0+clen) are rounded to out_dtype (QD_F16 / QD_BF16,
 *         nearest even) and written to out[(b*S+s)*ldo + oc0 + (c-c0)], channels up to clen_pad are set to zero.
 *         One call per segment; clen_pad, oc0 and ldo are multiples of 8.
 * ------------------------------------------------------------------------------------------ */
int qd_conv2d_wq_h16(const qd_conv_desc* d, int act_dtype, void* stream);
/* Scratch bytes qd_conv2d_wq_h16 would use for a split-K contraction of this descriptor, nsplit * M * Cout * 4 with nsplit <= 32
 * under the policy; 0 when the layer is launched unsplit.  Pure host function: shape fields, nseg, seg[].clen and epilogue only
 * are read, no pointer is followed, no GPU is needed. */
int64_t qd_conv2d_wq_h16_splitk_ws_bytes(const qd_conv_desc* d);
/* Launch-form query (additive in ABI 20; a pure host function): the launches qd_conv2d_wq_h16(d, act_dtype, stream) would make NOW,
 * the state of qd_wq_h16_config included.  form4 = {K slices (1 = one pass), K-steps per slice (0 for one pass), epilogue form
 * (0 fp32 rows, 1 fp16 rows, 2 GEGLU operand rows), 1 if the split-K finalise pass is the vectorised form (four columns per thread;
 * 0 for one pass)}.  d->splitk_ws / splitk_ws_bytes decide as they do for the launch: a NULL or too small workspace gives the one
 * pass, without an error.  The descriptor goes through the launcher's own checks and decisions with the launch withheld, so the
 * answer cannot drift from the launcher; it returns non-zero with qd_last_error wherever qd_conv2d_wq_h16 would refuse the
 * descriptor, with the same message.  Nothing is launched and no pointer of the descriptor is followed (null tests and alignment
 * only).  For tests and tools; not on any launch path. */
int qd_conv2d_wq_h16_form(const qd_conv_desc* d, int act_dtype, int32_t* form4);
/* qd_wq_h16_config (additive in ABI 20): splitk -1 = the policy (default); 0 = never split; n >= 2 = force n slices (clamped to
 * the K-step count so that no slice is empty; QD_EPI_GEGLU_H16 still unsplit); 1 = one slice, the same as 0.  qd_conv2d_wq_h16_splitk_ws_bytes honours it.
 * For tests and measurements. */
void qd_wq_h16_config(int splitk);
int qd_rows_to_h16(const void* x, int x_dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                   int c0, int clen, int clen_pad, void* out, int out_dtype, int64_t ldo, int oc0, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weights-only attention (state (weight_quant, act_quant) = (True, False))
 *
 *     qd_attn_h16: out = softmax(q k^T * scale) v per (b, h), one fused sweep (online softmax, the T x S score matrix is never
 *         written).  Replaces the floating-point attention of reference qdiff/quant_block.py:190-221 (use_act_quant False:
 *         einsum, * scale, softmax, einsum) and the legacy attention ldm/modules/diffusionmodules/openaimodel.py:373-406.
 *         q          logical [B][T][H][d], k and v [B][S][H][d], all of type in_dtype (QD_F32 / QD_F16 / QD_BF16), addressed by
 *                    element strides (sb, s_token, sh, sd); sd must be 1 and every run of 8 channels 16-byte aligned
 *                    (16-byte aligned bases, the other strides multiples of 16 bytes' worth of elements).  Values are rounded
 *                    to op_dtype (QD_F16 / QD_BF16, nearest even) when a tile is staged.
 *         d          a multiple of 8 in [8, 256]; any T >= 1, S >= 1; no mask.  scale > 0.  Head dims above 160 (the one-head
 *                    attention of the DDIM UNet) run one wave per SIMD.
 *         out        merged-head rows out[b*T + t][h*d + c], out_dtype QD_F32 or QD_F16, row stride ldo (>= H*d, a multiple
 *                    of 4 elements, out aligned to 4 elements).
 *         Scores accumulate in fp32 (v_mfma_f32_32x32x16_{f16,bf16}), the softmax runs in fp32 (exp2 with scale*log2 e
 *         folded in), P is rounded to op_dtype for the P.V product.
 * ------------------------------------------------------------------------------------------ */
int qd_attn_h16(const void* q, const void* k, const void* v, int in_dtype, int B, int T, int S, int H, int d,
                int64_t qsb, int64_t qst, int64_t qsh, int64_t qsd, int64_t ksb, int64_t kst, int64_t ksh, int64_t ksd,
                int64_t vsb, int64_t vst, int64_t vsh, int64_t vsd, float scale, int op_dtype, void* out, int out_dtype,
                int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weights-only producers (additive in ABI 20): the floating-point glue between the kernels of a
 *     weights-only block written straight as the fp16 / bf16 operand rows [M][ldo] that qd_conv2d_wq_h16 reads.  Input rows
 *     are fp32 or fp16 (x_dtype QD_F32 / QD_F16), 16-byte aligned with a row stride of a multiple of 16 bytes; arithmetic is
 *     fp32; the result is rounded ONCE (nearest even) to out_dtype (QD_F16 / QD_BF16); channels [C, ldo) of every row are
 *     written as zeros; ldo is a multiple of 8 and out is 16-byte aligned.  Rows outside [0, M) are not touched.
 *
 *     qd_layernorm_h16: nn.LayerNorm over the last axis of rows [M][C] (ldm/modules/attention.py:229-231, norm1 / norm2 /
 *         norm3 of BasicTransformerBlock) -> ONE row buffer, shared by every consumer (to_q / to_k / to_v): there is no
 *         per-consumer quantiser in this state.  C a multiple of 8, at most 2048; gamma / beta fp32, 16-byte aligned.
 *     qd_geglu_h16: h[:, :F] * gelu(h[:, F:2F]) with the erf GELU (attention.py:37-44 GEGLU.forward) of rows [M][ldh >= 2F]
 *         -> the operand rows of the feed-forward output Linear.  F a multiple of 8.
 *     qd_groupnorm_h16: GroupNorm (+ SiLU when apply_silu) of channels-last rows [B*S][C] -> operand rows: `in_layers` /
 *         `out_layers` norm + SiLU of ResBlock (ldm/modules/diffusionmodules/openaimodel.py:201-232, qdiff/quant_block.py:
 *         83-111); apply_silu = 0 is the plain Normalize in front of an attention block or a SpatialTransformer's proj_in.
 *         gamma / beta may be NULL.  C a multiple of 8 and of groups.  ws: qd_groupnorm_ws_bytes(B, C, S) bytes.
 *     qd_groupnorm_mod_h16 (additive in ABI 20): `out_norm(h) * (1 + scale) + shift` (+ SiLU) of a
 *         use_scale_shift_norm ResBlock (qdiff/quant_block.py:99-103) -> operand rows.  mod: fp32 [B][mod_ld >= 2C] rows
 *         scale | shift, one per sample (the two halves of the embedding projection), as in qd_groupnorm_mod_silu_quant; it
 *         is folded into the per-(sample, channel) affine, a' = a (1 + scale), sh' = sh (1 + scale) + shift in fp32, so with
 *         mod all zeros the rows are value-equal to qd_groupnorm_h16's.  Otherwise the arguments and checks of
 *         qd_groupnorm_h16; mod must not be NULL.
 *     qd_groupnorm_resample_h16 (additive in ABI 20): GroupNorm (+ SiLU) of a channels-last [B][H][W][C] map
 *         resampled BEFORE the one rounding: `in_layers[:-1]` and `h_upd` of an `updown` ResBlock (qdiff/quant_block.py:84-90)
 *         -> the operand rows of `in_layers[-1]`.  Statistics over the full-resolution input; ws: qd_groupnorm_ws_bytes(B, C, H*W).
 *         resample = 1: the 2x2 average of ResBlock(down=True) (openaimodel.py:134-160: Downsample(channels, False) =
 *             AvgPool2d(2, 2)); out rows [B * H/2 * W/2][ldo]; each output is ((y00 + y01) + (y10 + y11)) * 0.25f of the four
 *             fp32 post-SiLU values y(2h+dy, 2w+dx) = y_dydx, in exactly that order, then one round-to-nearest-even.  H and W
 *             must be even.
 *         resample = 2: nearest 2x of ResBlock(up=True) (openaimodel.py:91-117: Upsample(channels, False) =
 *             F.interpolate(scale_factor=2, mode="nearest")); out rows [B * 2H * 2W][ldo]; the rounded result of input pixel
 *             (h, w) is written to the four rows (2h + dy, 2w + dx): value-equal to qd_groupnorm_h16's rows replicated.
 *         Any other resample is refused.
 * ------------------------------------------------------------------------------------------ */
int qd_layernorm_h16(const void* x, int x_dtype, int64_t M, int C, int64_t ldx, float eps, const float* gamma,
                     const float* beta, void* out, int out_dtype, int64_t ldo, void* stream);
int qd_geglu_h16(const void* h, int h_dtype, int64_t M, int F, int64_t ldh, void* out, int out_dtype, int64_t ldo,
                 void* stream);
int qd_groupnorm_h16(const void* x, int x_dtype, int64_t B, int64_t S, int C, int64_t ldx, int groups, float eps,
                     const float* gamma, const float* beta, int apply_silu, void* out, int out_dtype, int64_t ldo,
                     void* ws, void* stream);
int qd_groupnorm_mod_h16(const void* x, int x_dtype, int64_t B, int64_t S, int C, int64_t ldx, int groups, float eps,
                         const float* gamma, const float* beta, const float* mod, int64_t mod_ld, int apply_silu, void* out,
                         int out_dtype, int64_t ldo, void* ws, void* stream);
int qd_groupnorm_resample_h16(const void* x, int x_dtype, int64_t B, int H, int W, int C, int64_t ldx, int groups, float eps,
                              const float* gamma, const float* beta, int apply_silu, int resample, void* out, int out_dtype,
                              int64_t ldo, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QDIFF_HIP_H */
