"""Cases and helpers of test_conv_tall_tiles_gpu.py: qd_conv2d_i8 on its 256-row tiles (MT = 2: `<2,5,4,1>` 256 x 160,
`<2,4,4,1>` 256 x 128, `<2,4,4,1,8>` 256 x 128 behind int8 weights), at the smallest shapes that reach them.

TEST INFRASTRUCTURE.  A launch takes the tall tile when its 256-row blocks still number 256 (one per CU), so every shape here is
wide (N = 800: five 160-column blocks, not a multiple of 320 or 224; N = 1024 / 1000 / 1002: eight 128-column blocks) and has
just over 51 or 31 row blocks; K stays at a few steps unless K is the edge.  No case computes its tile: `launch_forms` asks the
library (qd_conv2d_i8_form) about every launch right before it is made, and the helpers assert the answer.

Each case compares the one launch on all M rows
  (a) bit for bit with the same plan, weights and operand bytes launched in slices of whole samples that the library puts on
      128-row tiles — the tile the rest of the suite ties to the integer oracle; the epilogue is one template whose float
      sequence fma(I, scale, bias) + rowbias + residual does not depend on MT — and
  (b) with the CPU oracle (R.quant_module_forward + row bias + residual; comparison and bound of test_random_conv_shapes, step 3)
      on whole samples: the first, the last and one whose rows cross from one 256-row tile into the next.
"""
import contextlib
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from oracle import quant_ref as R


@contextlib.contextmanager
def launch_forms():
    """The forms (rows per block, columns per block, threads per block, K slices) of every hip.conv2d_i8 launch made inside the
    block, each asked of the library for the very ConvCall right before it is launched (None for the exact-accumulator hook,
    which has no query: it is built for 128 rows only)."""
    from qdiff import hip
    forms, real = [], hip.conv2d_i8

    def spy(c, acc_out=None):
        forms.append(hip.conv2d_i8_form(c) if acc_out is None else None)
        return real(c, acc_out=acc_out)
    hip.conv2d_i8 = spy
    try:
        yield forms
    finally:
        hip.conv2d_i8 = real


def one_form(forms, rows, cols, threads=None):
    """Exactly one launch, on rows x cols blocks, in one pass over K (threads: 512 = two K-groups, 256 = the four-wave block)."""
    assert len(forms) == 1 and forms[0] is not None, forms
    assert (forms[0][0], forms[0][1], forms[0][3]) == (rows, cols, 1), f"launch form {forms[0]}: the case is written for {rows} x {cols} blocks"
    assert threads is None or forms[0][2] == threads, f"launch form {forms[0]}: the case is written for {threads} threads per block"


def case(name, N, B, hw, wbits=4, Cin=16, k=3, stride=1, sym=False, dt=torch.float32, ups=False, acc=False):
    """hw: the stored activation map (half resolution when ups); dt: type of the output rows and of the residual."""
    return NS(name=name, N=N, B=B, hw=hw, wbits=wbits, Cin=Cin, k=k, stride=stride, sym=sym, dt=dt, ups=ups, acc=acc,
              cols=160 if N % 160 == 0 else 128)


F16 = torch.float16
# M % 256: 0, 64 (the second half-tile of the last block wholly past M), 128, 200 (partly past M), on each of the three tiles; samples
# of 64 rows (four to a tile) and of 100 rows (boundaries at irregular rows) with 3 x 3 / pad 1, so that image borders fall in
# both halves of a tile; asymmetric activations (out-of-image taps hold the zero point: zc, zfill, fill16) and symmetric ones.
CASES = [
    # ---- 256 x 160, int4 weights: N = 800, M just above 51 x 256 = 13056
    case("t160_hw256_m13312_tail0_acc", 800, 52, (16, 16), acc=True),
    case("t160_hw64_m13120_tail64_stride2", 800, 205, (16, 16), stride=2),
    case("t160_hw128_m13184_tail128_sym_f16", 800, 103, (8, 16), sym=True, dt=F16),
    case("t160_1x1_hw8_m13256_tail200_one_kstep", 800, 1657, (2, 4), k=1, Cin=64),
    case("t160_hw100_m13100_cin72_18_ksteps_f16", 800, 131, (10, 10), Cin=72, dt=F16),          # ragged last K-step of every tap; the ring wraps
    case("t160_upsample2x_hw64_m13120_acc", 800, 205, (4, 4), ups=True, acc=True),
    case("t160_1x1_cin320_five_ksteps_sym", 800, 52, (16, 16), k=1, Cin=320, sym=True),         # odd step count
    # ---- 256 x 128, int4 weights: M just above 31 x 256 = 7936; N = 1000: ragged last column block on vector stores; N = 1002: the
    # per-element paths (N % 4 != 0)
    case("t128_n1024_hw64_m8000_tail64_acc", 1024, 125, (8, 8), acc=True),
    case("t128_n1000_hw100_m13000_tail200_sym", 1000, 130, (10, 10), sym=True),
    case("t128_n1002_hw128_m8064_tail128", 1002, 63, (8, 16)),
    case("t128_n1002_hw128_m8064_f16", 1002, 63, (8, 16), dt=F16),
    case("t128_n1024_hw256_m8192_tail0_f16", 1024, 32, (16, 16), dt=F16),
    case("t128_n1000_stride2_cin72_f16", 1000, 125, (16, 16), stride=2, Cin=72, dt=F16),
    case("t128_n1024_upsample2x_sym", 1024, 125, (4, 4), ups=True, sym=True),
    # ---- 256 x 128, int8 weights
    case("w8_n1024_hw64_m8000_tail64_acc", 1024, 125, (8, 8), wbits=8, acc=True),
    case("w8_n1000_hw100_m13000_tail200", 1000, 130, (10, 10), wbits=8),
    case("w8_n1002_hw128_m8064_tail128_f16", 1002, 63, (8, 16), wbits=8, dt=F16),
    case("w8_n1024_hw256_m8192_tail0_sym", 1024, 32, (16, 16), wbits=8, sym=True),
    case("w8_n1024_1x1_hw8_m8200_one_kstep", 1024, 1025, (2, 4), wbits=8, k=1, Cin=64),
]


@functools.lru_cache(maxsize=None)
def layer(device, N, Cin, k, wbits):
    """Weights, AdaRound quantiser and packed codes of one layer: made once, shared by every case of that layer."""
    from qdiff import engine
    g = torch.Generator().manual_seed(7 * N + 3 * Cin + k + wbits)
    w = torch.randn(N, Cin, k, k, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    delta, zp = R.uaq_init_scale(w, wbits, False, True, "max")
    q = NS(delta=delta, zero_point=zp, n_bits=wbits, sym=False, n_levels=2 ** wbits, alpha=torch.rand(w.shape, generator=g) - 0.5,
           soft_targets=False)
    pack = engine.pack_module_weights(w.to(device), [q], 0)
    assert pack.tiled and pack.wbits == wbits
    return NS(w=w, bias=bias, q=q, pack=pack, codes=R.adaround_codes(w, q.delta, q.zero_point, q.alpha, q.n_levels))


def build(cuda, c, seed=0):
    """Operands of a case: quantised rows, a row bias that differs strongly from sample to sample, a residual of the output's
    type (kept fp16-representable, so that the fp32 and the fp16 launches add the same numbers)."""
    from qdiff import engine
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c.name)))
    h, w_ = c.hw
    x = torch.randn(c.B, c.Cin, h, w_, generator=g)
    x = x if c.sym else F.silu(x)
    ly = layer(cuda, c.N, c.Cin, c.k, c.wbits)
    d, z = R.uaq_init_scale(x, 8, c.sym, False, "max")
    aq = NS(delta=torch.tensor(float(d)), zero_point=z, n_bits=8, sym=c.sym)
    plan = engine.build_conv_plan(ly.pack, [aq], c.k, c.k, c.stride, c.k // 2, ly.bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, c.B, c.Cin, h * w_, (c.Cin * h * w_, h * w_, 1))
    H, W = (2 * h, 2 * w_) if c.ups else (h, w_)
    Ho, Wo = engine.conv_out_hw(H, W, plan)
    S, M = Ho * Wo, c.B * Ho * Wo
    rowbias = torch.randn(c.B, c.N, generator=g) + 3.0 * ((torch.arange(c.B) % 5) - 2.0)[:, None]
    residual = torch.randn(M, c.N, generator=g).half().float()
    return NS(c=c, ly=ly, x=x, aq=aq, z=z, plan=plan, xq=xq, H=H, W=W, Ho=Ho, Wo=Wo, S=S, S_in=h * w_, M=M,
              rowbias=rowbias.to(cuda), residual=residual.to(cuda), rowbias_cpu=rowbias, residual_cpu=residual)


def launch(t, rows, b0=0, b1=None, dt=None, residual=None, threads=None, **kw):
    """The case's convolution on samples [b0, b1) as ONE launch that the library must put on `rows` x t.c.cols blocks; row bias,
    residual and operand rows sliced to match.  residual: rows of all M outputs (default: the case's)."""
    from qdiff import engine
    c = t.c
    b1 = c.B if b1 is None else b1
    dt = c.dt if dt is None else dt
    res = (t.residual if residual is None else residual)[b0 * t.S:b1 * t.S].to(dt)
    with launch_forms() as forms:
        out = engine.conv_forward(t.plan, t.xq[b0 * t.S_in:b1 * t.S_in], b1 - b0, t.H, t.W, rowbias=t.rowbias[b0:b1], residual=res,
                                  out_dtype=dt, splitk=False, upsample2x=c.ups, **kw)
    one_form(forms, rows, c.cols, threads)
    return out


def slices(B, n=2):
    """n slices of whole samples, of unequal length when n does not divide B."""
    cut = [B * i // n for i in range(n + 1)]
    return list(zip(cut[:-1], cut[1:]))


def sliced(t, dt=None, n=2, residual=None):
    """The rows of all M outputs from launches on 128-row tiles (asserted per launch)."""
    return torch.cat([launch(t, 128, b0, b1, dt=dt, residual=residual) for b0, b1 in slices(t.c.B, n)])


def sliced_accumulators_are_exact(t):
    """qd_conv2d_i8_acc on the slices (128-row tiles by construction: O_I32 is built for MT = 1 only) against the integer oracle:
    the operand bytes of THIS case are what the 128-row rows above were contracted from."""
    from qdiff import engine
    c = t.c
    acc = torch.zeros((t.M, c.N), dtype=torch.int32, device=t.xq.device)
    for b0, b1 in slices(c.B):
        engine.conv_forward(t.plan, t.xq[b0 * t.S_in:b1 * t.S_in], b1 - b0, t.H, t.W, acc_out=acc[b0 * t.S:b1 * t.S], upsample2x=c.ups)
    torch.cuda.synchronize()
    xc = R.uaq_codes(t.x, t.aq.delta, t.z, 8, c.sym)
    if c.ups:
        xc = xc.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    want = R.int_conv_exact(xc, int(t.z), t.ly.codes, t.ly.q.zero_point.reshape(-1).long(), "conv2d", dict(stride=c.stride, padding=c.k // 2))
    got = acc.cpu().view(c.B, t.Ho, t.Wo, c.N).permute(0, 3, 1, 2).long()
    assert torch.equal(got, want), f"accumulators: max |diff| = {(got - want).abs().max().item()}"


def oracle_samples(t):
    """The first sample, the last, and one whose rows cross from one 256-row tile into the next (samples that are whole tiles
    never do: the middle one then)."""
    B, S = t.c.B, t.S
    cross = next((b for b in range(1, B - 1) if (b * S) % 256 != 0 and (b * S) // 256 != ((b + 1) * S - 1) // 256), B // 2)
    return sorted({0, cross, B - 1})


def oracle_rows(t, b, rowbias=None, residual=None):
    """fp32 rows [S][N] of sample b from the reference's fake-quantised layer, plus row bias and residual rows (default: the
    case's own; a test of the comparison's teeth passes wrong ones)."""
    c, ly = t.c, t.ly
    xb = t.x[b:b + 1]
    if c.ups:
        xb = F.interpolate(xb, scale_factor=2.0, mode="nearest")
    want = R.quant_module_forward(xb, ly.w, ly.bias, "conv2d", dict(stride=c.stride, padding=c.k // 2),
                                  [dict(delta=ly.q.delta, zero_point=ly.q.zero_point, alpha=ly.q.alpha, n_levels=ly.q.n_levels)],
                                  [dict(delta=t.aq.delta, zero_point=t.z, n_bits=8, sym=c.sym)])
    rows = want[0].permute(1, 2, 0).reshape(t.S, c.N)
    rows = rows + (t.rowbias_cpu[b][None, :] if rowbias is None else rowbias)
    return rows + (t.residual_cpu[b * t.S:(b + 1) * t.S] if residual is None else residual)


def within_oracle_bound(got, want):
    """Comparison and bound of test_random_conv_shapes, step 3 (there over the whole output, here over the samples checked: the
    range is at most that of the whole, so this is never the looser)."""
    diff, rng = (got - want).abs().max().item(), want.abs().max().item()
    print(f"oracle: max |diff| {diff:.3e}, bound {2e-5 * rng + 1e-6:.3e}")
    return diff <= 2e-5 * rng + 1e-6


def matches_oracle(t, out32, samples=None, **wrong):
    """out32: the fp32 rows of all M outputs.  wrong: rowbias=f(b) / residual=f(b) giving deliberately wrong rows of sample b."""
    samples = oracle_samples(t) if samples is None else samples
    got = torch.cat([out32[b * t.S:(b + 1) * t.S].cpu() for b in samples])
    want = torch.cat([oracle_rows(t, b, **{k: f(b) for k, f in wrong.items()}) for b in samples])
    return within_oracle_bound(got, want)


def check_case(t):
    """Both comparisons of a case for plain rows (fp32 or fp16 with a residual of the same type)."""
    c = t.c
    full = launch(t, 256)
    ref = sliced(t)
    torch.cuda.synchronize()
    assert full.dtype == c.dt and torch.isfinite(full.float()).all() and full.float().abs().max() > 0
    assert torch.equal(full, ref), f"256-row tile differs from the 128-row tile on {(full != ref).any(1).sum().item()} rows"
    if c.dt == torch.float32:
        full32 = full
    else:
        # fp16 rows are the fp32 value rounded once on the store (test_conv_fp16_stream_is_the_rounded_fp32_epilogue), also on this tile:
        # the oracle's bound is checked on the fp32 rows of the same tile, the fp16 rows against their rounding
        full32 = launch(t, 256, dt=torch.float32)
        torch.cuda.synchronize()
        assert torch.equal(full, full32.half())
    assert matches_oracle(t, full32)
    if c.acc:
        sliced_accumulators_are_exact(t)
    return full, ref
