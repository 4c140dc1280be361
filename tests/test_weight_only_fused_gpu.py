"""Fused weights-only blocks (engine.WEIGHT_ONLY_FUSE) on the GPU: the three producers (qd_layernorm_h16, qd_geglu_h16,
qd_groupnorm_h16) against fp64, the row bias of qd_conv2d_wq_h16, every covered block against today's unfused kernel route,
and whole UNets against the reference's weights-only golden output.

Producer bound, per output element, against the fp64 evaluation `ref` of the same op on the same input:
    |out - ref| <= half an ulp of the output type at ref  +  T
half ulp = 2^-11 |ref| (fp16; 2^-25 below the normal range: half the subnormal step 2^-24) or 2^-8 |ref| (bf16), and T the
fp32 term of the op, derived from the operations the op needs (u = 2^-24, the fp32 unit roundoff), not from the kernel:
  LayerNorm  y = (x - m) r g + b over C channels.  A sum of C fp32 terms is off by at most C u mean|x| in any order, so
             dm = C u mean|x|; x - m then carries u |x - m| + dm; the variance (C squares) and 1/sqrt are off by at most
             (C / 2 + 8) u relative in r; three more roundings for the two products and the add:
             T = u [ |g| r (|x - m| + C mean|x|) + (C / 2 + 12) |z g| + 2 (|z g| + |b|) ],  z = (x - m) r.
  GEGLU      y = a * 0.5 g (1 + erf(g / sqrt 2)).  The kernel's erf is stated to < 1 ulp (csrc/common.h), i.e. 2^-23 absolute
             (|erf| <= 1); the rounded argument moves erf by at most u (t erf'(t) <= 0.5); 1 + erf rounds by u: 2^-22 on the
             bracket, times 0.5 |a g|, plus three roundings of the products:  T = 2^-23 |a g| + 3 u |y|.
  GroupNorm  statistics over n = S C / G elements as fp32 partial sums of at most 32 rows (then fp64): dm = 33 u E|x|,
             dvar = 33 u E[x^2] + 2 |m| dm, rho = dvar / (2 (var + eps)) + 2 u on a = r g; the affine x a + (b - m a) carries
             (|x a| + |m a|) (rho + 3 u) + |a| dm + u (|b| + |y|); SiLU has slope <= 1.1 and exp / the quotient cost
             (|y| + 6) u relative:  T = 1.1 [ ... ] + (|y| + 6) u |out|.
As a cross-check that T is not tuned to the kernel, the library's fp32 op followed by .to(dtype) is measured against the same
bound: the kernel's worst error / bound must not exceed twice the library's.
"""
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

from golden_util import load_fixture
from test_weight_only_gpu import BOUNDS, MODELS, _codes, _fp64_conv, _layer, _metrics, _resume, _run, _wquant

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture
def knob():
    """The engine with all three weights-only knobs restored afterwards."""
    from qdiff import engine
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE)
    yield engine
    engine.set_weight_only_kernel(prev[0])
    engine.set_weight_only_attention(prev[1])
    engine.set_weight_only_fusion(prev[2])


def _half_ulp(ref, dt):
    if dt == torch.float16:
        return torch.maximum(2.0 ** -11 * ref.abs(), torch.full_like(ref, 2.0 ** -25))
    return torch.maximum(2.0 ** -8 * ref.abs(), torch.full_like(ref, 2.0 ** -134))


GUARD = 3          # rows in front of and behind `out` that no launch may touch


def _guarded(M, ldo, dt, dev):
    buf = torch.full((M + 2 * GUARD, ldo), 7.5, dtype=dt, device=dev)
    return buf, buf[GUARD:GUARD + M]


def _check_rows(buf, out, C, ref, tol, what):
    torch.cuda.synchronize()
    assert (buf[:GUARD] == 7.5).all() and (buf[-GUARD:] == 7.5).all(), f"{what}: rows outside [0, M) were written"
    assert (out[:, C:] == 0).all(), f"{what}: pad columns are not zero"
    err = (out[:, :C].double().cpu() - ref).abs()
    return (err / tol).max().item()


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta, eps):
    """fp64 LayerNorm of the rows x [M, C] (any float type, any device) and the fp32 term T of the bound, both on the CPU."""
    C = x.shape[1]
    xd, gd, bd = x.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    m = xd.mean(1, keepdim=True)
    r = 1 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    z = (xd - m) * r
    ref = z * gd + bd
    T = U * (gd.abs() * r * ((xd - m).abs() + C * xd.abs().mean(1, keepdim=True)) + (C / 2 + 12) * (z * gd).abs()
             + 2 * ((z * gd).abs() + bd.abs()))
    return ref, T


def _ln_lib(x, gamma, beta, eps, odt):
    """The library's fp32 LayerNorm followed by the cast, on the device of x."""
    return F.layer_norm(x.float(), (x.shape[1],), gamma.to(x.device), beta.to(x.device), eps).to(odt)


def _ln_launch(dev, x, gamma, beta, eps, odt, pad):
    """qd_layernorm_h16 of the CPU rows x into guarded rows on dev -> (buffer, rows)."""
    from qdiff import hip
    M, C = x.shape
    buf, out = _guarded(M, C + pad, odt, dev)
    hip.layernorm_h16(x.to(dev), M, C, C, eps, gamma.to(dev), beta.to(dev), out, C + pad)
    return buf, out


def _ln_case(dev, seed, C, M, xdt, odt, pad, gscale=1.0, drop_beta=False, x=None, gamma=None, beta=None):
    g = torch.Generator().manual_seed(seed)
    if x is None:
        x = (torch.randn(M, C, generator=g) * (0.2 + 3 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).to(xdt)
    if gamma is None:
        gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    eps = 1e-5
    ref, T = _ln_ref(x, gamma, beta, eps)
    tol = _half_ulp(ref, odt) + T
    buf, out = _ln_launch(dev, x, gamma * gscale, torch.zeros(C) if drop_beta else beta, eps, odt, pad)
    worst = _check_rows(buf, out, C, ref, tol, f"layernorm C={C} M={M}")
    lib = _ln_lib(x.to(dev), gamma, beta, eps, odt)
    worst_lib = ((lib.double().cpu() - ref).abs() / tol).max().item()
    return worst, worst_lib


LN_WIDTHS = [64, 128, 320, 640, 1280] + [8, 40, 104, 512, 520, 1024, 1536, 2048]     # the golden models' C first


def _producer_draws(widths, n, seed):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        C = widths[i % len(widths)]
        out.append((100 + i, C, rnd.choice([1, 2, 3, 7, 9, 31, 77, 130, 257]), torch.float32 if i % 2 == 0 else torch.float16,
                    torch.float16 if (i // 2) % 2 == 0 else torch.bfloat16, rnd.choice([0, 8, 16, 56])))
    return out


def _ids(c):
    return f"{c[0]}-C{c[1]}-M{c[2]}-{str(c[3])[6:]}-{str(c[4])[6:]}-pad{c[5]}"


@pytest.mark.parametrize("case", _producer_draws(LN_WIDTHS, 65, 1), ids=_ids)
def test_layernorm_h16_matches_fp64(cuda, case):
    seed, C, M, xdt, odt, pad = case
    worst, lib = _ln_case(cuda, seed, C, M, xdt, odt, pad)
    print(f"\nlayernorm_h16 {_ids(case)}: kernel {worst:.3f} x bound, library fp32 + cast {lib:.3f} x bound")
    assert worst <= 1.0 and worst <= 2 * lib


@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_layernorm_bound_bites(cuda, odt):
    assert _ln_case(cuda, 5, 320, 64, torch.float32, odt, 0)[0] <= 1.0
    assert _ln_case(cuda, 5, 320, 64, torch.float32, odt, 0, gscale=1.01)[0] > 1.0
    assert _ln_case(cuda, 5, 320, 64, torch.float32, odt, 0, drop_beta=True)[0] > 1.0


# ---- GEGLU -------------------------------------------------------------------------------------------------------------------
def _geglu_ref(h, Fd):
    """fp64 GEGLU of the rows h [M, >= 2 F] (value columns first) and the fp32 term T of the bound, both on the CPU."""
    hd = h.double().cpu()
    a, gt = hd[:, :Fd], hd[:, Fd:2 * Fd]
    ref = a * (0.5 * gt * (1 + torch.erf(gt / math.sqrt(2))))
    return ref, 2.0 ** -23 * (a * gt).abs() + 3 * U * ref.abs()


def _geglu_lib(h, Fd, odt):
    """The library's fp32 GELU times the value followed by the cast, on the device of h."""
    hl = h.float()
    return (hl[:, :Fd] * F.gelu(hl[:, Fd:2 * Fd])).to(odt)


def _geglu_launch(dev, h, Fd, odt, pad):
    """qd_geglu_h16 of the CPU rows h into guarded rows on dev -> (buffer, rows)."""
    from qdiff import hip
    M = h.shape[0]
    buf, out = _guarded(M, Fd + pad, odt, dev)
    hip.geglu_h16(h.to(dev), M, Fd, h.shape[1], out, Fd + pad)
    return buf, out


def _geglu_case(dev, seed, Fd, M, xdt, odt, pad, tanh=False, h=None):
    g = torch.Generator().manual_seed(seed)
    if h is None:
        h = (torch.randn(M, 2 * Fd, generator=g) * 2.5).to(xdt)
    ref, T = _geglu_ref(h, Fd)
    tol = _half_ulp(ref, odt) + T
    if tanh:                                                 # what a kernel with the tanh approximation would write
        buf, out = _guarded(M, Fd + pad, odt, dev)
        out[:, :Fd] = (h.to(dev).float()[:, :Fd] * F.gelu(h.to(dev).float()[:, Fd:], approximate="tanh")).to(odt)
        out[:, Fd:] = 0
    else:
        buf, out = _geglu_launch(dev, h, Fd, odt, pad)
    worst = _check_rows(buf, out, Fd, ref, tol, f"geglu F={Fd} M={M}")
    lib = _geglu_lib(h.to(dev), Fd, odt)
    return worst, ((lib.double().cpu() - ref).abs() / tol).max().item()


GEGLU_WIDTHS = [256, 512, 1280, 2560, 5120] + [8, 24, 72, 200, 1032]                   # the golden models' F = 4 C first


@pytest.mark.parametrize("case", _producer_draws(GEGLU_WIDTHS, 60, 2), ids=_ids)
def test_geglu_h16_matches_fp64(cuda, case):
    seed, Fd, M, xdt, odt, pad = case
    worst, lib = _geglu_case(cuda, seed, Fd, M, xdt, odt, pad)
    print(f"\ngeglu_h16 {_ids(case)}: kernel {worst:.3f} x bound, library fp32 + cast {lib:.3f} x bound")
    assert worst <= 1.0 and worst <= 2 * lib


@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_geglu_bound_bites(cuda, odt):
    assert _geglu_case(cuda, 6, 1280, 64, torch.float32, odt, 0)[0] <= 1.0
    assert _geglu_case(cuda, 6, 1280, 64, torch.float32, odt, 0, tanh=True)[0] > 1.0


# ---- GroupNorm (+ SiLU) ------------------------------------------------------------------------------------------------------
def _gn_ref(x, G, gamma, beta, eps, silu):
    """fp64 GroupNorm (+ SiLU) of x [B, S, C] as rows [B * S, C] and the fp32 term T of the bound, both on the CPU."""
    B, S, C = x.shape
    xd = x.double().cpu().view(B, S, G, C // G)
    m = xd.mean((1, 3), keepdim=True)
    var = xd.var((1, 3), unbiased=False, keepdim=True)
    ex2, eabs = (xd * xd).mean((1, 3), keepdim=True), xd.abs().mean((1, 3), keepdim=True)
    gm, bt = gamma.double().cpu().view(1, 1, G, C // G), beta.double().cpu().view(1, 1, G, C // G)
    a = gm / torch.sqrt(var + eps)
    y = (xd - m) * a + bt
    ref = y * torch.sigmoid(y) if silu else y
    dm = 33 * U * eabs
    rho = (33 * U * ex2 + 2 * m.abs() * dm) / (2 * (var + eps)) + 2 * U
    T = 1.1 * (((xd * a).abs() + (m * a).abs()) * (rho + 3 * U) + a.abs() * dm + U * (bt.abs() + y.abs())) + (y.abs() + 6) * U * ref.abs()
    return ref.reshape(B * S, C), T.reshape(B * S, C)


def _gn_lib(x, G, gamma, beta, eps, silu, odt):
    """The library's fp32 GroupNorm (+ SiLU) followed by the cast, as rows [B * S, C], on the device of x."""
    B, S, C = x.shape
    lib = F.group_norm(x.float().permute(0, 2, 1), G, gamma.to(x.device), beta.to(x.device), eps)
    return (F.silu(lib) if silu else lib).permute(0, 2, 1).reshape(B * S, C).to(odt)


def _gn_launch(dev, x, G, gamma, beta, eps, silu, odt, pad):
    """qd_groupnorm_h16 of the CPU tensor x [B, S, C] into guarded rows on dev -> (buffer, rows)."""
    from qdiff import hip
    B, S, C = x.shape
    buf, out = _guarded(B * S, C + pad, odt, dev)
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=dev)
    hip.groupnorm_h16(x.to(dev).view(B * S, C), B, S, C, C, G, eps, gamma.to(dev), beta.to(dev), silu, out, C + pad, ws)
    return buf, out


def _gn_case(dev, seed, C, S, B, xdt, odt, pad, silu, groups=None, gscale=1.0, drop_beta=False, x=None, gamma=None, beta=None):
    G = groups or (32 if C % 32 == 0 else 8 if C % 8 == 0 else 1)
    g = torch.Generator().manual_seed(seed)
    if x is None:
        x = (torch.randn(B, S, C, generator=g) * (0.3 + 2 * torch.rand(1, 1, C, generator=g)) + 0.5 * torch.randn(1, 1, C, generator=g)).to(xdt)
    if gamma is None:
        gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    eps = 1e-5
    ref, T = _gn_ref(x, G, gamma, beta, eps, silu)
    tol = _half_ulp(ref, odt) + T
    buf, out = _gn_launch(dev, x, G, gamma * gscale, torch.zeros(C) if drop_beta else beta, eps, silu, odt, pad)
    worst = _check_rows(buf, out, C, ref, tol, f"groupnorm C={C} S={S} B={B}")
    lib = _gn_lib(x.to(dev), G, gamma, beta, eps, silu, odt)
    return worst, ((lib.double().cpu() - ref).abs() / tol).max().item()


GN_WIDTHS = [32, 64, 96, 128, 192, 224, 256, 320, 448, 640, 672, 896, 960, 1120, 1280, 1344, 1568, 1792, 1920, 2560] + [8, 40, 72]


def _gn_draws():
    rnd = random.Random(3)
    out = []
    for i in range(69):
        C = GN_WIDTHS[i % len(GN_WIDTHS)]
        S = rnd.choice([4, 9, 16, 63, 64, 100, 256, 257, 289, 1024])
        out.append((300 + i, C, S, rnd.choice([1, 2, 3]), torch.float32 if i % 2 == 0 else torch.float16,
                    torch.float16 if (i // 2) % 2 == 0 else torch.bfloat16, rnd.choice([0, 8, 24]), i % 3 != 2))
    return out


@pytest.mark.parametrize("case", _gn_draws(), ids=lambda c: f"{c[0]}-C{c[1]}-S{c[2]}-B{c[3]}-{str(c[4])[6:]}-{str(c[5])[6:]}-pad{c[6]}-silu{int(c[7])}")
def test_groupnorm_h16_matches_fp64(cuda, case):
    seed, C, S, B, xdt, odt, pad, silu = case
    worst, lib = _gn_case(cuda, seed, C, S, B, xdt, odt, pad, silu)
    print(f"\ngroupnorm_h16 C={C} S={S} B={B} {xdt} -> {odt} silu={silu}: kernel {worst:.3f} x bound, library fp32 + cast {lib:.3f} x bound")
    assert worst <= 1.0 and worst <= 2 * lib


@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_bound_bites(cuda, odt, silu):
    assert _gn_case(cuda, 7, 320, 256, 2, torch.float32, odt, 0, silu)[0] <= 1.0
    assert _gn_case(cuda, 7, 320, 256, 2, torch.float32, odt, 0, silu, gscale=1.01)[0] > 1.0
    assert _gn_case(cuda, 7, 320, 256, 2, torch.float32, odt, 0, silu, drop_beta=True)[0] > 1.0


# ---- row bias of qd_conv2d_wq_h16 ----------------------------------------------------------------------------------------------
def _rowbias_case(dev, kind, wbits, act, out_dtype, split, B, Cin, Cout, H, W, k, stride, seed):
    """test_weight_only_gpu._run_case (the same fp64 reference and tolerance formula) with a row bias: one fp32 row per sample
    added to every output row of that sample, |rowbias| joining bias and residual in the `extra` term."""
    from types import SimpleNamespace as NS
    from qdiff import engine
    g = torch.Generator().manual_seed(seed)
    x, w = _layer(kind, B, Cin, Cout, H, W, k, stride, g)
    pad = k // 2 if kind == "conv2d" else 0
    bounds = [(0, Cin)] if not split else [(0, split), (split, Cin)]
    qs = [_wquant(w[:, a:b], wbits, "range", g) for a, b in bounds]
    bias = torch.randn(Cout, generator=g)
    pack = engine.pack_module_weights(w.to(dev), [NS(**{**vars(q), "delta": q.delta.to(dev), "zero_point": q.zero_point.to(dev)})
                                                   for q in qs], split or 0)
    kh, kw = (k, k) if kind == "conv2d" else (1, 1)
    plan = engine.build_wonly_plan(pack, kh, kw, stride if kind == "conv2d" else 1, pad, bias.to(dev), act)
    xd = x.to(dev)
    if kind == "conv2d":
        sb, sc, sh, sw = xd.stride()
        xh = engine.wonly_rows(xd, plan, B, Cin, H * W, (sb, sc, sw))
        Ho, Wo = engine.conv_out_hw(H, W, plan)
        geo = (B, H, W, Ho, Wo)
    else:                                                    # linear on [B, W, Cin] tokens: B samples of W rows
        rows = xd.reshape(-1, Cin)
        xh = engine.wonly_rows(rows, plan, 1, Cin, rows.shape[0], (0, 1, rows.stride(0)))
        geo = (B, 1, W, 1, W)
    M = geo[0] * geo[3] * geo[4]
    res = torch.randn(M, Cout, generator=g).to(out_dtype)
    ld = Cout + 8                                            # rows wider than Cout: ld_rowbias is honoured
    rb = torch.randn(B, ld, generator=g) * 2
    out = engine.wonly_forward(plan, xh, *geo, out_dtype=out_dtype, residual=res.to(dev), rowbias=rb.to(dev)[:, :Cout])
    out0 = engine.wonly_forward(plan, xh, *geo, out_dtype=out_dtype, residual=res.to(dev))
    torch.cuda.synchronize()
    xr = x.to(act).double()
    ref = torch.zeros(())
    S = torch.zeros(())
    for (a, b), q in zip(bounds, qs):
        shape = (-1,) + (1,) * (w.dim() - 1)
        wq = ((_codes(w[:, a:b], q) - q.zero_point.view(shape)) * q.delta.view(shape)).double()
        xs = xr[:, a:b] if kind != "linear" else xr[..., a:b]
        ref = ref + _fp64_conv(kind, xs, wq, stride, pad)
        S = S + _fp64_conv(kind, xs.abs(), wq.abs(), stride, pad)
    if kind == "conv2d":
        ref, S = ref.permute(0, 2, 3, 1).reshape(M, Cout), S.permute(0, 2, 3, 1).reshape(M, Cout)
    else:
        ref, S = ref.reshape(M, Cout), S.reshape(M, Cout)
    rbm = rb[:, :Cout].double().repeat_interleave(M // B, dim=0)
    ref0 = ref + bias.double() + res.double()
    ref = ref0 + rbm
    extra = bias.double().abs() + res.double().abs() + rbm.abs()
    tol = kh * kw * Cin * 2.0 ** -26 * S + 2.0 ** -22 * (extra + ref.abs())
    tol0 = kh * kw * Cin * 2.0 ** -26 * S + 2.0 ** -22 * (extra - rbm.abs() + ref0.abs())
    if out_dtype == torch.float16:
        tol = tol * (1 + 2.0 ** -11) + 2.0 ** -11 * ref.abs() + 2.0 ** -24
        tol0 = tol0 * (1 + 2.0 ** -11) + 2.0 ** -11 * ref0.abs() + 2.0 ** -24
    worst = ((out.double().cpu() - ref).abs() / tol).max().item()
    worst0 = ((out0.double().cpu() - ref0).abs() / tol0).max().item()
    # the bound bites: the bias row of the WRONG sample misses it (B >= 2)
    wrong = ((out.double().cpu() - (ref0 + rbm.flip(0))).abs() / tol).max().item()
    return worst, worst0, wrong


ROWBIAS_CASES = [("conv2d", 1, 1, 0), ("conv2d", 3, 1, 0), ("conv2d", 3, 2, 0), ("conv2d", 3, 1, 40), ("conv2d", 1, 1, 24), ("linear", 1, 1, 0),
                 ("linear", 1, 1, 32)]


@pytest.mark.parametrize("kind,k,stride,split", ROWBIAS_CASES)
@pytest.mark.parametrize("wbits,act,odt", [(4, torch.float16, torch.float32), (8, torch.bfloat16, torch.float32), (4, torch.bfloat16, torch.float16),
                                           (8, torch.float16, torch.float16)])
def test_rowbias_matches_fp64(cuda, kind, k, stride, split, wbits, act, odt):
    for seed, (B, Cin, Cout, H, W) in enumerate([(2, 104, 96, 9, 11), (3, 72, 130, 5, 17)]):
        worst, worst0, wrong = _rowbias_case(cuda, kind, wbits, act, odt, split, B, Cin, Cout, H, W, k, stride, 40 + seed)
        print(f"\nrowbias {kind} k={k} s={stride} split={split} W{wbits} {act} -> {odt}: {worst:.3f} x bound (without: {worst0:.3f}, wrong sample: {wrong:.3g})")
        assert worst <= 1.0 and worst0 <= 1.0 and wrong > 1.0


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def _covered(qnn):
    from qdiff.quant_block import QuantBasicTransformerBlock, QuantResBlock
    return [(n, m) for n, m in qnn.named_modules()
            if isinstance(m, QuantBasicTransformerBlock) or (isinstance(m, QuantResBlock) and not m.updown and not m.use_scale_shift_norm)]


def _reset(engine):
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0


@pytest.mark.parametrize("name", ["sd_tiny", "ldm_tiny", "sd_full", "ldm_full"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_blocks_against_the_unfused_kernel_route(cuda, knob, name, dt):
    """Every covered block, teacher-forced with its input of a knobs-off fp32 evaluation: the fused route's error against the
    knobs-off fp32 output of the block (as a fraction of that output's range) is at most twice the error of today's unfused
    kernel route (layer knob on, fusion off) on the same input, with a floor of one ulp of the operand type (2^-10 / 2^-7) of
    the range.  With the attention knob off and on (the yardstick run has the same attention knob)."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    blocks = _covered(qnn)
    assert blocks
    rec = {}
    hooks = []
    for n, b in blocks:
        hooks.append(b.register_forward_pre_hook(lambda m, a, k, n=n: rec.__setitem__(n, [a, k, None]), with_kwargs=True))
        hooks.append(b.register_forward_hook(lambda m, a, o, n=n: rec[n].__setitem__(2, o)))
    knob.set_weight_only_kernel(None)
    knob.set_weight_only_attention(None)
    knob.set_weight_only_fusion(False)
    try:
        _run(qnn, fx, cuda)
    finally:
        for h in hooks:
            h.remove()                                       # a hooked block falls back
    floor = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    knob.set_weight_only_kernel(dt)
    bad = []
    for attn in (None, dt):
        knob.set_weight_only_attention(attn)
        for n, b in blocks:
            a, k, ref = rec[n]
            rng = ref.abs().max().item()
            with torch.no_grad():
                knob.set_weight_only_fusion(False)
                e0 = (b(*a, **k) - ref).abs().max().item() / rng
                knob.set_weight_only_fusion(True)
                _reset(knob)
                y = b(*a, **k)
                e1 = (y - ref).abs().max().item() / rng
            assert sum(knob.WONLY_FUSED.values()) == 1, f"{n} did not take the fused route"
            assert y.dtype == ref.dtype and y.shape == ref.shape
            print(f"[block-parity] {name} {str(dt)[6:]} attn={'on' if attn else 'off'} {n} ({type(b).__name__}): "
                  f"unfused {e0:.3e} fused {e1:.3e} of range (bound {max(2 * e0, floor):.3e})")
            if e1 > max(2 * e0, floor):
                bad.append((n, attn, e0, e1))
    assert not bad, bad


# ---- whole UNets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("attn", [False, True], ids=["libattn", "attn"])
def test_fused_unet_matches_reference(cuda, knob, name, dt, attn):
    """State (True, False), layer knob and fusion on, against the reference's weights-only golden `out_w`, inside
    tests/test_weight_only_gpu.py's BOUNDS; every plain residual block and every transformer block on the fused route; two runs
    bit-equal; a model without a covered block bit-equal to fusion off."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_attention(dt if attn else None)
    knob.set_weight_only_fusion(False)
    y_off = _run(qnn, fx, cuda)
    knob.set_weight_only_fusion(True)
    _reset(knob)
    y = _run(qnn, fx, cuda)
    took = dict(knob.WONLY_FUSED)
    y2 = _run(qnn, fx, cuda)
    from qdiff.quant_block import QuantBasicTransformerBlock, QuantResBlock
    covered = _covered(qnn)
    want = {"resblock": sum(isinstance(m, QuantResBlock) for _, m in covered),
            "transformer": sum(isinstance(m, QuantBasicTransformerBlock) for _, m in covered)}
    d, cos = _metrics(y, fx["out_w"])
    d0, cos0 = _metrics(y_off, fx["out_w"])
    print(f"\n[{name}] fused {dt} attn={attn}: {took} blocks fused, {d:.3e} of range, cosine {cos:.7f} (fusion off: {d0:.3e}, {cos0:.7f})")
    assert took == want
    assert y.dtype == torch.float32 and torch.equal(y, y2)
    if not covered:
        assert torch.equal(y, y_off)
    tol, cmin = BOUNDS[dt]
    assert d <= tol and cos >= cmin


def test_packed_checkpoint_runs_the_fused_route_bit_identically(cuda, knob):
    """save_packed_ckpt -> load_packed_ckpt(free_weights=True) into a model whose fp32 weights differ: the fused route gives the
    source model's output bit for bit."""
    import tempfile
    import qdiff
    from golden_util import build_engine_model, quant_params
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    fx = load_fixture("model_sd_tiny.pt")
    src = _resume(fx, cuda)
    knob.set_weight_only_kernel(torch.float16)
    knob.set_weight_only_attention(torch.float16)
    knob.set_weight_only_fusion(True)
    src.set_quant_state(True, False)
    _reset(knob)
    y_src = _run(src, fx, cuda)
    n_src = dict(knob.WONLY_FUSED)
    src.set_quant_state(True, True)
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    model = build_engine_model(spec)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    dst = qdiff.QuantModel(model.to(cuda), wq, aq, sm_abit=spec["sm_abit"]).to(cuda).eval()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "packed.pt")
        save_packed_ckpt(src, path)
        load_packed_ckpt(dst, path, free_weights=True)
    dst.set_quant_state(True, False)
    _reset(knob)
    y = _run(dst, fx, cuda)
    assert dict(knob.WONLY_FUSED) == n_src and sum(n_src.values()) > 0
    assert torch.equal(y, y_src)
