"""GPU parity tests of every C-ABI entry point against the CPU oracle (oracle/quant_ref.py).

Integer work (codes, packed weights, int32 accumulators) must match BIT-EXACTLY (oracle tier T0);
floating-point outputs are compared with the tolerance written in each test (tier T1).
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import quant_ref as R

pytestmark = pytest.mark.gpu


def _aq(delta, zp, n_bits=8, sym=False):
    return NS(delta=torch.tensor(float(delta)), zero_point=zp, n_bits=n_bits, sym=sym)


def _grid_off(n_bits, sym):
    return 0 if sym or n_bits < 8 else 128


# ------------------------------------------------------------------------------------------------
# K1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("C", [3, 48, 100])
def test_quantize_act_bit_exact(cuda, layout, sym, C):
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(1)
    B, H, W = 2, 9, 7
    x = torch.randn(B, C, H, W, generator=g) * 2.0
    x[0, 0, 0, :4] = torch.tensor([0.5, 1.5, 2.5, -0.5]) * 0.037  # exact ties: round-half-even
    delta, zp = 0.037, (0 if sym else 131)
    codes = R.uaq_codes(x, torch.tensor(delta), zp, 8, sym)
    off = _grid_off(8, sym)
    xd = x.to(cuda)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    S = H * W
    sb, sc, sh, sw = xd.stride()
    assert sh == W * sw
    grid = engine.act_grid(8, sym)
    qp = torch.tensor([delta, float(zp)], device=cuda)
    ldo = hip.pad16(C) + 16
    out = torch.full((B * S, ldo), 77, dtype=torch.int8, device=cuda)
    hip.quantize_act(xd, B, C, S, (sb, sc, sw), qp, grid, out, ldo, oc0=16)
    torch.cuda.synchronize()
    got = out.cpu().view(B, H, W, ldo)
    want = (codes - off).permute(0, 2, 3, 1).to(torch.int8)
    assert torch.equal(got[..., 16:16 + C], want)
    assert (got[..., :16] == 77).all()                       # untouched prefix
    assert (got[..., 16 + C:] == zp - off).all()              # pad lanes hold "true zero"


def test_exact_fast_division_certificate(cuda):
    """qd_make_qparams: the kernels replace x / delta by y = x*rinv; e = fma(-y, delta, x); q = fma(e, rinv, y) only when
    the device-side exhaustive check (all 2^23 mantissas) certified bit equality for that delta.  Codes must equal
    torch.round(x / delta) bit for bit either way; awkward deltas (all-ones mantissa, denormal-adjacent, huge) included."""
    import struct
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(4)
    ones = struct.unpack("f", struct.pack("I", 0x3dffffff))[0]          # mantissa all ones
    deltas = [0.037, 0.0151234, 1e-3, 1.0, 3.0000002, ones, 7.3e-7, 123.456, 1e-30] + [float(v) for v in torch.rand(8, generator=g) * 0.1 + 1e-4]
    x = torch.cat([torch.randn(1 << 16, generator=g) * 3.0, torch.tensor([0.0, -0.0, 0.5 * 0.037, 1.5 * 0.037, 2.5 * 0.037, 1e-20, -1e-20])])
    M = x.numel()
    xd = x.to(cuda)
    grid = engine.act_grid(8, False)
    fast = 0
    for d in deltas:
        dt = torch.tensor(d, dtype=torch.float32)
        qp = hip.make_qparams(dt.to(cuda), torch.tensor(128.0, device=cuda))
        vals = qp.cpu()
        assert vals[0].item() == dt.item() and vals[1].item() == 128.0
        fast += int(vals[3].item() != 0)
        out = torch.empty((1, hip.pad16(M)), dtype=torch.int8, device=cuda)
        hip.quantize_act(xd, 1, M, 1, (0, 1, 0), qp, grid, out, hip.pad16(M))
        want = torch.clamp(torch.round(x / dt) + 128.0, 0, 255) - 128
        assert torch.equal(out.cpu()[0, :M].float(), want), d
    print(f"\n[fastdiv] {fast} of {len(deltas)} deltas certified for the 3-instruction quotient")
    assert fast >= len(deltas) - 3


def test_quantize_act_split_segments(cuda):
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(2)
    B, C, H, W, split = 2, 80, 4, 4, 32
    x = torch.randn(B, C, H, W, generator=g)
    p0, p1 = (0.02, 120), (0.05, 97)
    xd = x.to(cuda)
    out = torch.zeros((B * H * W, 80), dtype=torch.int8, device=cuda)
    grid = engine.act_grid(8, False)
    for (c0, clen, oc0, (d, z)) in [(0, split, 0, p0), (split, C - split, 32, p1)]:
        hip.quantize_act(xd, B, C, H * W, (C * H * W, H * W, 1), torch.tensor([d, float(z)], device=cuda), grid, out, 80,
                         c0=c0, clen=clen, oc0=oc0)
    got = out.cpu().view(B, H, W, 80).permute(0, 3, 1, 2)
    w0 = R.uaq_codes(x[:, :split], torch.tensor(p0[0]), p0[1], 8, False) - 128
    w1 = R.uaq_codes(x[:, split:], torch.tensor(p1[0]), p1[1], 8, False) - 128
    assert torch.equal(got[:, :32].long(), w0) and torch.equal(got[:, 32:].long(), w1)


# ------------------------------------------------------------------------------------------------
# K2
# ------------------------------------------------------------------------------------------------
def _weight_quantizer(w, n_bits, adaround, g):
    delta, zp = R.uaq_init_scale(w, n_bits, False, True, "max")
    q = NS(delta=delta, zero_point=zp, n_bits=n_bits, sym=False, n_levels=2 ** n_bits)
    if adaround:
        q.alpha = (torch.rand(w.shape, generator=g) - 0.5)
        q.soft_targets = False
    return q


def _codes(w, q):
    if getattr(q, "alpha", None) is not None:
        return R.adaround_codes(w, q.delta, q.zero_point, q.alpha, q.n_levels)
    return R.nearest_codes(w, q.delta, q.zero_point, q.n_levels)


@pytest.mark.parametrize("n_bits,adaround", [(8, True), (8, False), (4, True), (4, False), (6, True)])
def test_pack_weights_codes_bit_exact(cuda, n_bits, adaround):
    from qdiff import hip
    g = torch.Generator().manual_seed(3)
    Cout, Cin, kh = 37, 40, 3
    w = torch.randn(Cout, Cin, kh, kh, generator=g) * 0.1
    q = _weight_quantizer(w, n_bits, adaround, g)
    want = _codes(w, q)
    taps = kh * kh
    ldk = 64
    for mode in ([8, 0] if n_bits > 4 else [4, 8]):
        wq =torch.zeros(Cout * taps * ldk // (2 if mode == 4 else 1), dtype=torch.uint8, device=cuda)
        wsum = torch.zeros(Cout, dtype=torch.int32, device=cuda)
        codes = torch.zeros((Cout, Cin, taps), dtype=torch.int32, device=cuda)
        hip.pack_weights(w.to(cuda), q.alpha.to(cuda) if adaround else None, q.delta.reshape(-1).to(cuda),
                         q.zero_point.reshape(-1).to(cuda), Cout, Cin, taps, 0, Cin, 2 ** n_bits, mode, wq, ldk, 0, wsum, codes)
        torch.cuda.synchronize()
        assert torch.equal(codes.cpu().long().view(Cout, Cin, kh, kh), want)
        zp = q.zero_point.reshape(-1).long()
        if mode == 8:
            rows = wq.cpu().view(torch.int8).view(Cout, taps, ldk).long()
            got = rows[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, kh, kh)
            assert torch.equal(got, want - 128)
            assert (rows[:, :, Cin:48] == 0).all()
            assert torch.equal(wsum.cpu().long(), (want - 128).sum(dim=(1, 2, 3)))
        elif mode == 0:
            # direct mode: the stored byte is the low byte of W - zw (an s8 wherever W - zw fits one: every zero point of the
            # 6-bit grid here, zw = 128 alone on the full 8-bit grid); the sum is that of W - zw itself
            direct = want - zp.view(-1, 1, 1, 1)
            rows = wq.cpu().view(Cout, taps, ldk).long()
            got = rows[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, kh, kh)
            assert torch.equal(got, direct & 0xff)
            assert n_bits == 8 or torch.equal(wq.cpu().view(torch.int8).view(Cout, taps, ldk).long()[:, :, :Cin].permute(0, 2, 1).reshape(want.shape), direct)
            assert (rows[:, :, Cin:48] == 0).all()
            assert torch.equal(wsum.cpu().long(), direct.sum(dim=(1, 2, 3)))
        else:
            raw = wq.cpu().view(Cout, taps, ldk // 2).long()
            lo, hi = raw & 15, raw >> 4
            k = torch.zeros(Cout, taps, ldk, dtype=torch.long)
            for chunk in range(ldk // 16):
                for word in range(2):
                    for b in range(4):
                        byte = chunk * 8 + word * 4 + b
                        k[:, :, chunk * 16 + word * 8 + b] = lo[:, :, byte]
                        k[:, :, chunk * 16 + word * 8 + 4 + b] = hi[:, :, byte]
            got = k[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, kh, kh)
            assert torch.equal(got, want)
            pad = 48 - Cin
            assert torch.equal(wsum.cpu().long(), (want - zp.view(-1, 1, 1, 1)).sum(dim=(1, 2, 3)) - zp * pad * taps)


# ------------------------------------------------------------------------------------------------
# K3/K4: exact accumulators and fp epilogue
# ------------------------------------------------------------------------------------------------
CONV_CASES = [
    # name,            B, Cin, H,  W, Cout, k, stride, pad, asym_pad
    ("c3x3_s1",        2, 48, 12, 12, 40, 3, 1, 1, False),
    ("c3x3_big",       4, 64, 32, 32, 256, 3, 1, 1, False),   # exercises the 128x128 tile
    ("c3x3_s2_p1",     2, 32, 16, 16, 48, 3, 2, 1, False),
    ("c3x3_s2_asym",   2, 32, 16, 16, 48, 3, 2, 0, True),     # CIFAR Downsample: F.pad(0,1,0,1)+pad 0
    ("c1x1",           3, 80, 8, 8, 96, 1, 1, 0, False),
    ("stem_c3",        2, 3, 16, 16, 32, 3, 1, 1, False),
    ("out_c4",         2, 64, 16, 16, 4, 3, 1, 1, False),
    ("k224",           2, 224, 8, 8, 64, 3, 1, 1, False),      # K-step tail masking (224 = 3.5 * 64)
    ("n96_tail",       2, 64, 8, 8, 96, 1, 1, 0, False),       # N tail: 3 n-tiles under a 4-tile block
    ("n224_m_tail",    3, 96, 7, 7, 224, 3, 1, 1, False),      # LDM width (NT=7), ragged M (147 rows)
    ("n320_big",       8, 320, 32, 32, 320, 3, 1, 1, False),   # 256x160 tile of the DMA kernel
]


def _run_conv(cuda, x, w, bias, q, aq, k, stride, pad, asym_pad, acc=False, rowbias=None, residual=None):
    from qdiff import engine
    B, Cin, H, W = x.shape
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], k, k, stride, pad, bias.to(cuda) if bias is not None else None)
    xd = x.to(cuda)
    xq = engine.quantize_rows(xd, plan, B, Cin, H * W, (Cin * H * W, H * W, 1))
    if asym_pad:
        Ho, Wo = (H + 1 - k) // stride + 1, (W + 1 - k) // stride + 1
    else:
        Ho, Wo = engine.conv_out_hw(H, W, plan)
    acc_out = torch.zeros((B * Ho * Wo, plan.Cout), dtype=torch.int32, device=cuda) if acc else None
    out = engine.conv_forward(plan, xq, B, H, W, Ho, Wo, acc_out=acc_out,
                              rowbias=rowbias.to(cuda) if rowbias is not None else None,
                              residual=residual.to(cuda) if residual is not None else None)
    torch.cuda.synchronize()
    return out.cpu().view(B, Ho, Wo, -1).permute(0, 3, 1, 2), pack.mode


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
@pytest.mark.parametrize("w_bits", [8, 4])
@pytest.mark.parametrize("a_sym", [True, False])
def test_conv_int32_accumulators_bit_exact(cuda, case, w_bits, a_sym):
    _, B, Cin, H, W, Cout, k, stride, pad, asym_pad = case
    g = torch.Generator().manual_seed(hash(case[0]) % 1000 + w_bits)
    x = torch.randn(B, Cin, H, W, generator=g)
    x = F.silu(x) if not a_sym else x
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    q = _weight_quantizer(w, w_bits, True, g)
    d, z = R.uaq_init_scale(x, 8, a_sym, False, "max")
    aq = _aq(d, z, 8, a_sym)
    got, mode = _run_conv(cuda, x, w, None, q, aq, k, stride, pad, asym_pad, acc=True)
    xc = R.uaq_codes(x, aq.delta, aq.zero_point, 8, a_sym)
    xin = xc
    kw = dict(stride=stride, padding=pad)
    if asym_pad:
        xin = F.pad(xc - int(z), (0, 1, 0, 1)) + int(z)      # pad holds real 0 == code zp
    want = R.int_conv_exact(xin, int(z), _codes(w, q), q.zero_point.reshape(-1).long(), "conv2d", kw)
    assert mode == (4 if w_bits == 4 else 8)
    assert torch.equal(got.long(), want), f"max |diff| = {(got.long() - want).abs().max().item()}"


@pytest.mark.parametrize("case", CONV_CASES[:5], ids=[c[0] for c in CONV_CASES[:5]])
@pytest.mark.parametrize("w_bits", [8, 4])
def test_conv_fp32_matches_fake_quant(cuda, case, w_bits):
    """vs the reference's fp32 simulation (tier T1): rel tolerance 2e-5 of the output range
    (SURVEY.md §7 measured 3e-7; fp32 accumulation order differs)."""
    _, B, Cin, H, W, Cout, k, stride, pad, asym_pad = case
    g = torch.Generator().manual_seed(11)
    x = F.silu(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)
    q = _weight_quantizer(w, w_bits, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    aq = _aq(d, z)
    rowbias = torch.randn(B, Cout, generator=g)
    got, _ = _run_conv(cuda, x, w, bias, q, aq, k, stride, pad, asym_pad, rowbias=rowbias)
    xin = F.pad(x, (0, 1, 0, 1)) if asym_pad else x
    want = R.quant_module_forward(xin, w, bias, "conv2d", dict(stride=stride, padding=pad),
                                  [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=q.n_levels)],
                                  [dict(delta=aq.delta, zero_point=z, n_bits=8, sym=False)])
    want = want + rowbias[:, :, None, None]
    tol = 2e-5 * want.abs().max().item()
    assert (got - want).abs().max().item() <= tol


import os
os.environ.setdefault("QD_WIDE_MINBLK", "4")      # read once by the library: lets the small test shapes take the 128 x 320 tile
os.environ.setdefault("QD_WIDE_MINK", "64")

WIDE_CASES = [
    # name,             B, Cin,  H,  W, Cout, k   — N % 320 == 0: the shapes the 128 x 320 tile of 2 x 2 waves covers
    ("n320_ragged_m",   3, 96, 13, 13, 320, 3),   # 507 rows: ragged last M block
    ("n640_k1",         2, 320, 16, 16, 640, 1),
    ("n320_k960",       1, 960, 24, 24, 320, 3),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_conv_wide_tiles_match_fake_quant(cuda, case):
    """fp32 output (+ row bias + residual) of 320-multiple-wide layers vs the reference's simulation, 2e-5 of range.  These
    shapes take the 128 x 320 tile of 2 x 2 waves (block-count and K thresholds lowered through the environment above; asserted
    through qd_conv2d_i8_form); the 128 x 160 tile is covered by the other convolution tests, the 256 x 160 tile by
    test_conv_tall_tiles_gpu.py."""
    from conv_tall_tile_cases import launch_forms, one_form
    from qdiff import engine
    _, B, Cin, H, W, Cout, k = case
    g = torch.Generator().manual_seed(23)
    x = F.silu(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    aq = _aq(d, z)
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [aq], k, k, 1, k // 2, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * W, (Cin * H * W, H * W, 1))
    rowbias = torch.randn(B, Cout, generator=g).to(cuda)
    residual = torch.randn(B * H * W, Cout, generator=g).to(cuda)
    with launch_forms() as forms:
        a = engine.conv_forward(plan, xq, B, H, W, rowbias=rowbias, residual=residual, splitk=False)
    one_form(forms, 128, 320)
    torch.cuda.synchronize()
    want = R.quant_module_forward(x, w, bias, "conv2d", dict(stride=1, padding=k // 2),
                                  [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=q.n_levels)],
                                  [dict(delta=aq.delta, zero_point=z, n_bits=8, sym=False)])
    want = want + rowbias.cpu()[:, :, None, None] + residual.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    got = a.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert (got - want).abs().max().item() <= 2e-5 * want.abs().max().item()


def test_conv_split_two_segments(cuda):
    """1x1 split shortcut (quant_layer.py:257-269): two activation + two weight quantisers."""
    from qdiff import engine
    g = torch.Generator().manual_seed(5)
    for w_bits in (8, 4):
        B, C, H, W, Cout, split = 2, 224 + 96, 8, 8, 72, 224
        x = torch.randn(B, C, H, W, generator=g)
        x[:, split:] *= 3.0
        w = torch.randn(Cout, C, 1, 1, generator=g) * 0.05
        bias = torch.randn(Cout, generator=g)
        q0 = _weight_quantizer(w[:, :split], w_bits, True, g)
        q1 = _weight_quantizer(w[:, split:], w_bits, True, g)
        d0, z0 = R.uaq_init_scale(x[:, :split], 8, False, False, "max")
        d1, z1 = R.uaq_init_scale(x[:, split:], 8, False, False, "max")
        a0, a1 = _aq(d0, z0), _aq(d1, z1)
        pack = engine.pack_module_weights(w.to(cuda), [q0, q1], split)
        plan = engine.build_conv_plan(pack, [a0, a1], 1, 1, 1, 0, bias.to(cuda))
        xq = engine.quantize_rows(x.to(cuda), plan, B, C, H * W, (C * H * W, H * W, 1))
        res = torch.randn(B * H * W, Cout, generator=g)
        out = engine.conv_forward(plan, xq, B, H, W, residual=res.to(cuda))
        torch.cuda.synchronize()
        got = out.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
        want = R.quant_module_forward(
            x, w, bias, "conv2d", dict(stride=1, padding=0),
            [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=q.n_levels) for q in (q0, q1)],
            [dict(delta=a.delta, zero_point=a.zero_point, n_bits=8, sym=False) for a in (a0, a1)], split=split)
        want = want + res.view(B, H, W, Cout).permute(0, 3, 1, 2)
        assert (got - want).abs().max().item() <= 2e-5 * want.abs().max().item()


SPLITK_CASES = [
    # name, B, Cin, H, W, Cout, k     (M = B*H*W small, K long: the layers the library contracts split-K)
    ("emb_m16",      16, 1280, 1, 1, 1280, 1),     # time-embedding Linear: M=16
    ("emb_m1",        1, 320, 1, 1, 1280, 1),      # a single sample: M=1
    ("mid_8x8",       4, 640, 8, 8, 1280, 3),      # 8x8 middle-block conv: M=256, K=5760
    ("ctx_kv",        2, 768, 1, 77, 320, 1),      # cross-attention k/v projection of 77 context tokens
    ("m1024_ragged",  1, 352, 30, 33, 224, 3),     # ragged M (990), K tail (352 = 5.5 * 64), NT=7
]


@pytest.mark.parametrize("case", SPLITK_CASES, ids=[c[0] for c in SPLITK_CASES])
def test_conv_splitk_is_bit_identical_to_unsplit(cuda, case):
    """Split-K partials are int32 (exact) and the finalise pass runs the same float sequence as the fused
    epilogue, so the schedule must not change a single output bit; both also match the fp32 fake-quant."""
    from qdiff import engine, hip
    _, B, Cin, H, W, Cout, k = case
    g = torch.Generator().manual_seed(21)
    x = F.silu(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    aq = _aq(d, z)
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], k, k, 1, k // 2, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * W, (Cin * H * W, H * W, 1))
    rowbias = torch.randn(B, Cout, generator=g).to(cuda)
    residual = torch.randn(B * H * W, Cout, generator=g).to(cuda)
    desc_probe = hip.ConvCall(x=xq, w=pack.wq, ldx=plan.ldx, ldk=pack.ldk, B=B, H=H, W=W, Ho=H, Wo=W, Cout=Cout, kh=k, kw=k,
                              stride=1, pad_t=k // 2, pad_l=k // 2, wbits=4, w_tiled=pack.tiled, segs=plan.segs)
    if pack.tiled:
        assert hip.splitk_ws_bytes(desc_probe) > 0, "case is meant to take the split-K schedule"
    a = engine.conv_forward(plan, xq, B, H, W, rowbias=rowbias, residual=residual)
    b = engine.conv_forward(plan, xq, B, H, W, rowbias=rowbias, residual=residual, splitk=False)
    torch.cuda.synchronize()
    assert torch.equal(a, b), f"max |diff| = {(a - b).abs().max().item()}"
    want = R.quant_module_forward(x, w, bias, "conv2d", dict(stride=1, padding=k // 2),
                                  [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=q.n_levels)],
                                  [dict(delta=aq.delta, zero_point=z, n_bits=8, sym=False)])
    want = want + rowbias.cpu()[:, :, None, None] + residual.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    got = a.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert (got - want).abs().max().item() <= 2e-5 * want.abs().max().item()


def test_linear_tokens(cuda):
    from qdiff import engine
    g = torch.Generator().manual_seed(6)
    M, K, N = 2 * 77, 768, 320
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.03
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    aq = _aq(d, z)
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], 1, 1, 1, 0, None)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    out = engine.conv_forward(plan, xq, 1, 1, M)
    torch.cuda.synchronize()
    want = R.quant_module_forward(x, w, None, "linear", {}, [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=16)],
                                  [dict(delta=aq.delta, zero_point=z, n_bits=8, sym=False)])
    assert (out.cpu() - want).abs().max().item() <= 2e-5 * want.abs().max().item()


# ------------------------------------------------------------------------------------------------
# K5 / K9
# ------------------------------------------------------------------------------------------------
def _code_mismatch(got, want):
    diff = (got.long() - want.long()).abs()
    return diff.max().item(), (diff > 0).float().mean().item()


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("C,S", [(64, 100), (320, 64), (1920, 16)])
def test_groupnorm_silu_quant(cuda, silu, C, S):
    """float path differs from torch GroupNorm by rounding only, so codes may flip by one on exact
    ties: allow <= 0.1 % of elements off by one code, none by more."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(7)
    B = 3
    x = torch.randn(B, C, 1, S, generator=g) * 2 + 0.3
    gn = torch.nn.GroupNorm(32, C, eps=1e-6)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g))
        gn.bias.copy_(torch.randn(C, generator=g))
        y = gn(x)
        y = R.silu(y) if silu else y
    d, z = R.uaq_init_scale(y, 8, False, False, "max")
    want = R.uaq_codes(y, d, z, 8, False) - 128
    rows = x.to(cuda).permute(0, 2, 3, 1).reshape(B * S, C).contiguous()
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    yo = torch.empty((B * S, C), dtype=torch.float32, device=cuda)
    hip.groupnorm_silu_quant(rows, B, S, C, C, 32, 1e-6, gn.weight.data.to(cuda), gn.bias.data.to(cuda), silu,
                             torch.tensor([float(d), float(z)], device=cuda), engine.act_grid(8, False), out, C, ws, yout=yo, ldy=C)
    torch.cuda.synchronize()
    yref = y.permute(0, 2, 3, 1).reshape(B * S, C)
    assert (yo.cpu() - yref).abs().max().item() <= 1e-5 * max(1.0, yref.abs().max().item())
    mx, frac = _code_mismatch(out.cpu(), want.permute(0, 2, 3, 1).reshape(B * S, C))
    assert mx <= 1 and frac <= 1e-3


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("C,S,from_part", [(64, 100, False), (384, 256, False), (768, 64, True)])
def test_groupnorm_modulated_silu_quant(cuda, silu, C, S, from_part):
    """qd_groupnorm_mod_silu_quant: `GroupNorm(h) * (1 + scale) + shift` of a use_scale_shift_norm residual block
    (reference quant_block.py:99-103) -> SiLU -> codes, the modulation folded into the normalisation's per-(sample, channel)
    affine.  Same criterion as the plain kernel: fp32 output within rounding of the torch composition, codes off by at most
    one on <= 0.1 % of the elements.  from_part: statistics from first-level partial sums (the producer-epilogue route)."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(9)
    B = 3
    x = torch.randn(B, C, 1, S, generator=g) * 2 + 0.3
    mod = torch.randn(B, 2 * C + 8, generator=g) * 0.7                     # rows wider than 2C: mod_ld is honoured
    gn = torch.nn.GroupNorm(32, C, eps=1e-5)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g))
        gn.bias.copy_(torch.randn(C, generator=g))
        y = gn(x) * (1 + mod[:, :C, None, None]) + mod[:, C:2 * C, None, None]
        y = R.silu(y) if silu else y
    d, z = R.uaq_init_scale(y, 8, False, False, "max")
    want = R.uaq_codes(y, d, z, 8, False) - 128
    rows = x.to(cuda).permute(0, 2, 3, 1).reshape(B * S, C).contiguous()
    part = None
    if from_part:
        nchunk = 4
        r = rows.view(B, nchunk, S // nchunk, C).double()
        part = torch.stack([r.sum(2), (r * r).sum(2)], dim=-1).float().contiguous()      # [B][nchunk][C][2]
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    yo = torch.empty((B * S, C), dtype=torch.float32, device=cuda)
    hip.groupnorm_silu_quant(rows, B, S, C, C, 32, 1e-5, gn.weight.data.to(cuda), gn.bias.data.to(cuda), silu,
                             torch.tensor([float(d), float(z)], device=cuda), engine.act_grid(8, False), out, C, ws, yout=yo, ldy=C,
                             part=part, mod=mod.to(cuda))
    torch.cuda.synchronize()
    yref = y.permute(0, 2, 3, 1).reshape(B * S, C)
    assert (yo.cpu() - yref).abs().max().item() <= 1e-5 * max(1.0, yref.abs().max().item())
    mx, frac = _code_mismatch(out.cpu(), want.permute(0, 2, 3, 1).reshape(B * S, C))
    assert mx <= 1 and frac <= 1e-3


def test_layernorm_quant_three_consumers(cuda):
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(8)
    M, C = 70, 320
    x = torch.randn(M, C, generator=g) * 1.7
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(C, generator=g))
        ln.bias.copy_(torch.randn(C, generator=g))
        y = ln(x)
    params = [(0.031, 120), (0.02, 133), (0.05, 100)]
    outs = [torch.empty((M, C), dtype=torch.int8, device=cuda) for _ in params]
    hip.layernorm_quant(x.to(cuda), M, C, C, ln.eps, ln.weight.data.to(cuda), ln.bias.data.to(cuda),
                        [torch.tensor([d, float(z)], device=cuda) for d, z in params], [engine.act_grid(8, False)] * 3, outs, C)
    torch.cuda.synchronize()
    for o, (d, z) in zip(outs, params):
        mx, frac = _code_mismatch(o.cpu(), R.uaq_codes(y, torch.tensor(d), z, 8, False) - 128)
        assert mx <= 1 and frac <= 1e-3


def test_geglu_quant(cuda):
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(9)
    M, Fdim = 50, 640
    h = torch.randn(M, 2 * Fdim, generator=g)
    y = R.geglu(h)
    d, z = R.uaq_init_scale(y, 8, False, False, "max")
    out = torch.empty((M, Fdim), dtype=torch.int8, device=cuda)
    hip.geglu_quant(h.to(cuda), M, Fdim, 2 * Fdim, torch.tensor([float(d), float(z)], device=cuda), engine.act_grid(8, False), out, Fdim)
    torch.cuda.synchronize()
    mx, frac = _code_mismatch(out.cpu(), R.uaq_codes(y, d, z, 8, False) - 128)
    assert mx <= 1 and frac <= 1e-3


# ------------------------------------------------------------------------------------------------
# K7/K8
# ------------------------------------------------------------------------------------------------
ATTN_CASES = [
    # name, B, H, T, S, d, sm_bits, sym, scale
    ("sd_self_d40", 2, 8, 96, 96, 40, 16, False, 40 ** -0.5),
    ("sd_cross_77", 2, 8, 64, 77, 80, 16, False, 80 ** -0.5),
    ("sd_d160", 1, 8, 64, 64, 160, 16, False, 160 ** -0.5),
    ("cifar_c256_sym", 2, 1, 256, 256, 256, 8, True, 256 ** -0.5),
    ("cifar_mid_T16", 2, 1, 16, 16, 256, 8, True, 256 ** -0.5),
    ("ldm_d32", 2, 14, 64, 64, 32, 8, False, 1.0),
    # the shape that takes 25 % of an SD evaluation: 64x64 self-attention, d = 40 padded to 64, 16-bit probabilities,
    # asymmetric q (attn_kernel<2, P16, ASYM>): 128 key tiles per sweep, int64 hi/lo recombination with large code sums
    ("sd_self_4096", 2, 8, 4096, 4096, 40, 16, False, 40 ** -0.5),
    # q >= 0: its asymmetric zero point is 0, i.e. the stored zero point is -128 and -zq' = 128 does not fit one signed
    # operand byte (the kernel's two-constant c1/c2 path); ragged T and S exercise the peeled tail tile with it
    ("sd_qpos_zq-128", 2, 8, 200, 77, 40, 16, False, 40 ** -0.5),
    # SD's 1024-token level on the register-fed lean kernel with three K slabs (d = 80 padded to 96) and the key-term table
    ("sd_self_d80_1024", 1, 8, 1024, 1024, 80, 16, False, 80 ** -0.5),
    # diffuse rows under a fine probability grid (codes ~300 of 1024 keys, a few rows above the grid: clamped): the per-query
    # code shift with signed hi bytes and the per-tile hi skip of attn_pv_kernel, held to the oracle directly
    ("sd_self_flatgrid_1024", 1, 4, 256, 1024, 40, 16, False, 40 ** -0.5),
]
# LSUN-Churches LDM-8 (8 heads on 192 / 384 / 768 channels: head dims 24 / 48 / 96, 8-bit operands — asymmetric as the
# README runs this model, one symmetric case — 8-bit probabilities, tokens 1024 .. 4): the lean kernel's 8-bit-probability
# instances and the 4-token middle block.  Collected late: added after the round's last GPU run.
ATTN_CASES_LATE = [
    ("ldm_churches_d24", 2, 8, 1024, 1024, 24, 8, False, 1.0),
    ("ldm_churches_d48", 2, 8, 256, 256, 48, 8, False, 1.0),
    ("ldm_churches_d48_sym", 2, 8, 256, 256, 48, 8, True, 1.0),
    ("ldm_churches_d96", 2, 8, 64, 64, 96, 8, False, 1.0),
    ("ldm_churches_mid_T4", 2, 8, 4, 4, 96, 8, False, 1.0),
]
ATTN_PARAMS = [pytest.param(c, id=c[0]) for c in ATTN_CASES + ATTN_CASES_LATE]


@pytest.mark.parametrize("case", ATTN_PARAMS)
def test_attention_fused(cuda, case):
    """Fused attention vs the integer oracle (exact integer contractions, fp64 softmax): the only
    fp work is the softmax, so 16-bit probability codes may differ by a few ulps of exp():
    tolerance 2e-4 of the output range; vs the reference's fp32 simulation 1e-3.
    This criterion is statistical; exactness (known operand codes, decided rows equal to the integer oracle bit for bit,
    every launch form) is held by tests/test_attention_exact_gpu.py."""
    from qdiff import engine
    name, B, H, T, S, d, smb, sym, scale = case
    g = torch.Generator().manual_seed(12)
    q = torch.randn(B, T, H * d, generator=g)
    k = torch.randn(B, S, H * d, generator=g)
    v = torch.randn(B, S, H * d, generator=g)
    pre = (d ** -0.25) if name.startswith("ldm") else 1.0
    if "qpos" in name:
        q = q.abs()
    if "flatgrid" in name:
        q = q * 0.25

    def mk(t, n_bits=8, s=sym, always_zero=False):
        dd, zz = R.uaq_init_scale(t, n_bits, s, False, "max", always_zero)
        return dict(delta=dd, zero_point=zz, n_bits=n_bits, sym=s)
    aq_q, aq_k, aq_v = mk(q * pre), mk(k * pre), mk(v)
    if "qpos" in name:
        assert int(aq_q["zero_point"]) == 0
    heads = lambda t, L: t.view(B, L, H, d).permute(0, 2, 1, 3).reshape(B * H, L, d)
    with torch.no_grad():
        sim = torch.einsum("bid,bjd->bij", heads(q, T) * pre, heads(k, S) * pre) * scale
        p = sim.softmax(-1)
    w_sym = sym if name.startswith("cifar") else False
    aq_w = mk(p, smb, w_sym, always_zero=not name.startswith("cifar"))
    if "flatgrid" in name:
        aq_w["delta"] = torch.tensor(1.0 / (S * 300.0))
    want_int, _ = R.attention_int(heads(q, T), heads(k, S), heads(v, S), scale, aq_q, aq_k, aq_v, aq_w, pre_scale=pre)
    want_fq = R.attention_fq(heads(q, T), heads(k, S), heads(v, S), scale, aq_q, aq_k, aq_v, aq_w, pre_scale=pre)
    ns = lambda a: NS(delta=a["delta"], zero_point=a["zero_point"], n_bits=a["n_bits"], sym=a["sym"])
    ap = engine.build_attn_plan(ns(aq_q), ns(aq_k), ns(aq_v), ns(aq_w), scale, pre, cuda)
    C = H * d
    from qdiff import hip
    try:
        if "d80" in name:
            hip.attn_config(lean=3)              # opt-in: d = 80 on the register-fed lean kernel with three K slabs
        out = engine.attention(ap, q.to(cuda), k.to(cuda), v.to(cuda), B, T, S, H, d,
                               (T * C, C, d, 1), (S * C, C, d, 1), (S * C, C, d, 1))
    finally:
        hip.attn_config(lean=1)
    torch.cuda.synchronize()
    got = out.cpu().view(B, T, H, d).permute(0, 2, 1, 3).reshape(B * H, T, d)
    rng = want_int.abs().max().item()
    diff = (got.double() - want_int).abs()
    # bulk: fp32-softmax rounding only.  A probability whose p/delta_w lands on a .5 tie may round the
    # other way than the fp64 oracle: one code on one P element moves one output ROW by <= delta_w*delta_v*127
    # (visible on the coarse 8-bit grids only) -> allow <= 1 % of outputs beyond the bulk bound, none beyond 2e-2.
    assert (diff > 2e-4 * rng).float().mean().item() <= 1e-2
    assert diff.max().item() <= 2e-2 * rng
    assert ((got - want_fq).abs() > 1e-3 * rng).float().mean().item() <= 1e-2


@pytest.mark.parametrize("shape", [(2, 320, 32, 320, 3), (1, 640, 16, 640, 3), (2, 320, 64, 320, 1), (3, 96, 16, 200, 3), (16, 256, 8, 1280, 3),
                                   (4, 160, 64, 640, 3), (8, 64, 64, 320, 1), (2, 224, 32, 224, 3), (3, 96, 16, 196, 3), (3, 96, 16, 198, 3),
                                   (2, 64, 32, 128, 3), (1, 32, 16, 64, 1)])
def test_conv_fp16_stream_is_the_rounded_fp32_epilogue(cuda, shape):
    """fp16 activation stream (out / residual stored as halves): the epilogue computes the SAME fp32 value and rounds it once
    (RN) on the store, reads the residual as float(half) — so with a half-representable residual the fp16 output equals
    `fp32_output.half()` bit for bit, the GroupNorm statistics (taken from the fp32 values) are identical, on the 128x320
    tile, the 256x160 / 128x160 tiles, a ragged width (scalar path) and the split-K schedule alike.  Round 5: the full-line
    epilogue (two MFMA tiles per transposition, 16-byte lanes) — the added shapes hit the 128 x 320 tile of 2 x 2 waves (its
    second wave column starts in the upper half of a line), the 256 x 160 tile with odd N blocks, the 224-wide tile whose row
    stride is not a multiple of a line, a width that is a multiple of 8 but not of 32 (200), widths that fall back to the
    8-byte / scalar forms (196, 198) and the 128- / 64-wide tiles."""
    from qdiff import engine
    B, Cin, H, Cout, k = shape
    g = torch.Generator().manual_seed(53)
    x = F.silu(torch.randn(B, Cin, H, H, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], k, k, 1, k // 2,
                                  torch.randn(Cout, generator=g).to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * H, (Cin * H * H, H * H, 1))
    rowbias = torch.randn(B, Cout, generator=g).to(cuda)
    res16 = torch.randn(B * H * H, Cout, generator=g).to(cuda).half()
    gn = (H * H) % 128 == 0
    for kw in (dict(gn_stats=gn, splitk=False), dict()):
        o32 = engine.conv_forward(plan, xq, B, H, H, rowbias=rowbias, residual=res16.float(), out_dtype=torch.float32, **kw)
        o16 = engine.conv_forward(plan, xq, B, H, H, rowbias=rowbias, residual=res16, out_dtype=torch.float16, **kw)
        torch.cuda.synchronize()
        assert o16.dtype == torch.float16 and torch.equal(o16, o32.half())
        if hasattr(o32, "qd_gn_part"):
            assert hasattr(o16, "qd_gn_part") and torch.equal(o16.qd_gn_part, o32.qd_gn_part)


@pytest.mark.parametrize("B,H,C1,C2,Cmid", [(2, 16, 320, 160, 320), (1, 32, 640, 320, 160)])
def test_concatenation_slot_fp16_rows(cuda, B, H, C1, C2, Cmid):
    """The full-line fp16 epilogue writing into a column range of a wider buffer (engine.CatSlot: ldo > Cout, the second side
    starts C1 columns in): values = the plain fp16 output, statistics = the fp32 run's, bit for bit."""
    from qdiff import engine
    g = torch.Generator().manual_seed(72)
    S = H * H
    engine.set_stream_dtype(torch.float16)
    try:
        slot = engine.CatSlot(C1, C2)
        for side, Cout in enumerate((C1, C2)):
            x = F.silu(torch.randn(B, Cmid, H, H, generator=g))
            w = torch.randn(Cout, Cmid, 3, 3, generator=g) * 0.05
            d, z = R.uaq_init_scale(x, 8, False, False, "max")
            plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(d, z)], 3, 3, 1, 1,
                                          torch.randn(Cout, generator=g).to(cuda))
            xq = engine.quantize_rows(x.to(cuda), plan, B, Cmid, S, (Cmid * S, S, 1))
            o32 = engine.conv_forward(plan, xq, B, H, H, gn_stats=True, splitk=False, out_dtype=torch.float32)
            plain = engine.conv_forward(plan, xq, B, H, H, gn_stats=True, splitk=False)
            got = engine.conv_forward(plan, xq, B, H, H, gn_stats=True, splitk=False, slot=slot.side(side))
            torch.cuda.synchronize()
            assert got.dtype == torch.float16 and got.stride(0) == C1 + C2
            assert torch.equal(plain, o32.half()) and torch.equal(got, plain)
            assert torch.equal(got.qd_gn_part, o32.qd_gn_part)
    finally:
        engine.set_stream_dtype(torch.float32)


@pytest.mark.parametrize("C,S,silu,raw", [(320, 256, True, False), (640, 64, True, True), (1920, 16, False, True), (64, 100, True, False)])
def test_groupnorm_fp16_rows_16_byte_lanes(cuda, C, S, silu, raw):
    """Producers of the fp16 activation stream (8 halves per lane: gn_partial_h8 / gn_apply_rows_h8): the same halves widened to
    fp32 and sent through the fp32 kernels give the same first-level statistics, the same int8 codes and the same raw
    (skip-connection) codes, bit for bit — the arithmetic per element is identical, only the access width differs."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(17)
    B = 2
    x16 = (torch.randn(B * S, C + 16, generator=g) * 2 + 0.3).half().to(cuda)[:, :C]          # strided rows: ldx = C + 16
    x32 = x16.float()
    gn = torch.nn.GroupNorm(32, C, eps=1e-6).to(cuda)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g))
        gn.bias.copy_(torch.randn(C, generator=g))
    qp = torch.tensor([0.043, 131.0], device=cuda)
    grid = engine.act_grid(8, False)
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    res = {}
    for tag, rows in (("h", x16), ("f", x32)):
        out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
        rawd = None
        if raw:
            half = C // 2
            rawd = dict(out=torch.zeros((B * S, C), dtype=torch.int8, device=cuda),
                        segs=[dict(c0=0, clen=half, oc0=0, qparams=torch.tensor([0.05, 120.0], device=cuda), grid=grid),
                              dict(c0=half, clen=C - half, oc0=half, qparams=torch.tensor([0.07, 140.0], device=cuda), grid=grid)])
        hip.groupnorm_silu_quant(rows, B, S, C, rows.stride(0), 32, 1e-6, gn.weight.data, gn.bias.data, silu, qp, grid, out, C, ws, raw=rawd)
        torch.cuda.synchronize()
        res[tag] = (out.clone(), None if rawd is None else rawd["out"].clone())
    assert torch.equal(res["h"][0], res["f"][0])
    if raw:
        assert torch.equal(res["h"][1], res["f"][1]) and res["h"][1].abs().max() > 0


@pytest.mark.parametrize("M,C", [(70, 320), (128, 640), (33, 1280)])
def test_layernorm_fp16_rows_16_byte_lanes(cuda, M, C):
    """ln_quant_h8: LayerNorm + three quantisers on fp16 rows with 8 halves per lane.  Against the fp32 kernel on the same
    (widened) values: the statistics are summed in another lane order, so a code may move by one on a tie — <= 1e-3 of the
    elements, none by more; against torch on the widened values: the bound of test_layernorm_quant_three_consumers."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(8)
    x16 = (torch.randn(M, C, generator=g) * 1.7).half()
    x = x16.float()
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(C, generator=g))
        ln.bias.copy_(torch.randn(C, generator=g))
        y = ln(x)
    params = [(0.031, 120), (0.02, 133), (0.05, 100)]
    qps = [torch.tensor([d, float(z)], device=cuda) for d, z in params]
    outs = {}
    for tag, rows in (("h", x16.to(cuda)), ("f", x.to(cuda))):
        o = [torch.empty((M, C), dtype=torch.int8, device=cuda) for _ in params]
        hip.layernorm_quant(rows, M, C, C, ln.eps, ln.weight.data.to(cuda), ln.bias.data.to(cuda), qps, [engine.act_grid(8, False)] * 3, o, C)
        torch.cuda.synchronize()
        outs[tag] = o
    for oh_, of_, (d, z) in zip(outs["h"], outs["f"], params):
        mx, frac = _code_mismatch(oh_.cpu(), of_.cpu())
        assert mx <= 1 and frac <= 1e-3
        mx, frac = _code_mismatch(oh_.cpu(), R.uaq_codes(y, torch.tensor(d), z, 8, False) - 128)
        assert mx <= 1 and frac <= 1e-3


def test_linear_to_rows_with_fp16_residual(cuda):
    """QD_EPI_HEADS_I8 ("Linear + residual -> the next Linear's int8 rows") with the residual stored as halves: the same
    bytes as with the residual widened to fp32 first."""
    from qdiff import engine
    g = torch.Generator().manual_seed(59)
    B, T, K, N = 2, 256, 1280, 320
    x = torch.randn(B * T, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    q = _weight_quantizer(w, 4, True, g)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(dx, zx)], 1, 1, 1, 0, torch.randn(N, generator=g).to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, B * T, (0, 1, K))
    res16 = torch.randn(B * T, N, generator=g).to(cuda).half()
    y = engine.conv_forward(plan, xq, 1, 1, B * T, residual=res16.float(), out_dtype=torch.float32)
    w2 = torch.randn(N, N, generator=g) * 0.05
    q2 = _weight_quantizer(w2, 4, True, g)
    d2, z2 = R.uaq_init_scale(y.cpu(), 8, False, False, "max")
    nxt = engine.build_conv_plan(engine.pack_module_weights(w2.to(cuda), [q2], 0), [_aq(d2, z2)], 1, 1, 1, 0, None)
    assert engine.rows_i8_fusable(plan, nxt, T)
    a = engine.linear_to_rows_i8(plan, xq, B, T, nxt, residual=res16.float())
    b = engine.linear_to_rows_i8(plan, xq, B, T, nxt, residual=res16)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and a.abs().max() > 0


PIPE_CASES = [
    # name,            B, H, T,    S,    d,  sm_bits, q_sym, q_nonneg, peaky
    ("even_tiles",     2, 4, 160,  256,  40, 16, False, False, False),     # 8 full key tiles, no ragged tile
    ("odd_tiles",      1, 8, 96,   224,  40, 16, False, False, False),     # 7 full tiles
    ("odd_plus_tail",  2, 4, 64,   237,  40, 16, False, False, False),     # 7 full + ragged
    ("even_plus_tail", 2, 4, 64,   77,   40, 16, False, False, False),     # 2 full + ragged (the cross-attention shape)
    ("tail_only",      1, 4, 200,  19,   40, 16, False, False, False),     # the ragged tile alone
    ("one_tile",       1, 4, 64,   32,   40, 16, False, False, False),
    ("hi_dead_4096",   1, 2, 256,  4096, 40, 16, False, False, False),     # thousands of keys: no code reaches 256 (8-bit constants)
    ("hi_live_peaky",  2, 4, 128,  320,  40, 16, False, False, True),      # sharp rows: hi bytes alive, upper clamp possible
    ("p8_asym",        2, 8, 128,  192,  24, 8,  False, False, False),     # dpad 32 (DT = 1), 8-bit probabilities
    ("p8_sym_d48",     2, 8, 96,   160,  48, 8,  True,  False, False),
    ("p16_sym",        1, 4, 96,   130,  40, 16, True,  False, True),
    ("zq-128_fallback", 2, 4, 96,  77,   40, 16, False, True,  False),     # -zq' = 128: the unpipelined two-constant body
    ("ragged_T_blocks", 2, 4, 300, 200,  40, 16, False, False, False),     # 3 query blocks per head, the last one with idle waves
    ("octaves_repeat", 1, 2, 256,  512,  40, 16, False, False, "huge"),    # the row maximum rises > 64 octaves after tile 0: repeat pass
    ("d80_three_slabs", 2, 4, 160, 544,  80, 16, False, False, True),      # dpad 96: register-fed kernel in both modes; table vs constant-operand MFMAs
    ("d80_zq-128",     1, 4, 96,  77,   80, 16, False, True,  False),
    # round 6: rows whose codes reach 256 are shifted per query (signed hi byte, hi MFMAs skipped per tile when every shifted code
    # of the wave's tile fits the lo byte).  flatmix: head 0 peaked (codes up to 65535: shifted by -32768), the others diffuse at
    # three widths (all tiles skip / some tiles carry codes below the lo byte's window / too wide for the flat rule), ragged S;
    # flatgrid: every row diffuse under a probability grid 220 x finer than the data needs (codes ~300 of 4096 keys; the few
    # rows that exceed the grid take the clamped body with the shift)
    ("flatmix",        2, 4, 128,  237,  40, 16, False, False, "flatmix"),
    ("flatgrid_4096",  1, 2, 256,  4096, 40, 16, False, False, "flatgrid"),
    ("flatgrid_tail",  1, 4, 160,  1000, 40, 16, False, False, "flatgrid"),
]


@pytest.mark.parametrize("case", PIPE_CASES, ids=[c[0] for c in PIPE_CASES])
def test_attention_lds_equals_lean(cuda, case):
    """attn_lds_kernel (K / V^T tiles staged once per block in LDS by DMA, one-tile-deep software pipeline, hi-byte skip)
    against attn_lean_kernel on the same operands: the arithmetic, the operand order and the summation order are the same, so
    outputs must be BIT-IDENTICAL.  (The lean kernel itself is held to the integer oracle by test_attention_fused.)"""
    from qdiff import engine
    name, B, H, T, S, d, smb, qsym, qpos, peaky = case
    g = torch.Generator().manual_seed(77)
    C = H * d
    q, k, v = (torch.randn(B, L, C, generator=g) for L in (T, S, S))
    if qpos:
        q = q.abs()
    if peaky == "huge":
        q, k = q * 6.0, k * 6.0
        k[:, :40] *= 0.02                        # small scores in the first key tile, large ones later
    elif peaky == "flatmix":
        qh = q.view(B, T, H, d)
        qh[:, :, 0] *= 4.0
        for h, f in ((1, 0.05), (2, 0.3), (3, 0.8)):
            qh[:, :, h] *= f
    elif peaky == "flatgrid":
        q = q * 0.25
    elif peaky:
        q, k = q * 3.0, k * 3.0

    def mk(t, n_bits=8, s=False, always_zero=False):
        dd, zz = R.uaq_init_scale(t, n_bits, s, False, "max", always_zero)
        return NS(delta=dd, zero_point=zz, n_bits=n_bits, sym=s)
    heads = lambda t, L: t.view(B, L, H, d).permute(0, 2, 1, 3).reshape(B * H, L, d)
    scale = d ** -0.5
    p = (torch.einsum("bid,bjd->bij", heads(q, T), heads(k, S)) * scale).softmax(-1)
    aw = mk(p, smb, False, True)
    if peaky == "flatgrid":
        aw.delta = torch.tensor(1.0 / (S * 300.0))             # the mean probability 1 / S has code 300
    ap = engine.build_attn_plan(mk(q, 8, qsym), mk(k, 8, qsym), mk(v, 8, qsym), aw, scale, 1.0, cuda)
    Tp, Sp, dp = engine.pad32(T), engine.pad32(S), engine.pad32(d)
    q8 = torch.zeros((B * H, Tp, dp), dtype=torch.int8, device=cuda)
    k8 = torch.zeros((B * H, Sp, dp), dtype=torch.int8, device=cuda)
    v8 = torch.zeros((B * H, dp, Sp), dtype=torch.int8, device=cuda)
    vsum = torch.zeros((B * H, dp), dtype=torch.int32, device=cuda)
    for which, (t, L, buf) in enumerate(((q, T, q8), (k, S, k8), (v, S, v8))):
        engine.heads_from_float(ap, which, t.to(cuda), B, L, H, d, (L * C, C, d, 1), buf, vsum)
    from qdiff import hip
    outs, forms = {}, {}
    rows = torch.empty((B * T, C), dtype=torch.float32, device=cuda)        # the form query's output argument: never written
    try:
        # pipe 0: attn_lean_kernel (register-fed, one kernel), 3: the LDS-staged path on every eligible shape — three launches
        # since round 6: statistics, lo-only P.V, hi + lo P.V (every block runs in exactly one of the two); ktab 1: per-key
        # zero-point term from the qd_attn_keyterm table (accumulator seeds), 0: from constant-operand MFMAs (the register-fed
        # kernel in both modes) — the accumulators hold the same integers
        for mode in (0, 3):
            for ktab in (1, 0):
                hip.attn_config(pipe_mode=mode, ktab=ktab, lean=3 if d >= 64 else 1)
                forms[(mode, ktab)] = hip.attn_i8_form(q8, k8, v8, vsum, B * H, H, T, S, d, Tp, Sp, dp, ap.prm, ap.wbits, ap.wmin, ap.wmax,
                                                       ap.asym, rows, rows.stride(0))
                o = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d)
                torch.cuda.synchronize()
                outs[(mode, ktab)] = o.clone()
    finally:
        hip.attn_config(pipe_mode=2, ktab=1, lean=1)
    # the settings are the kernels the comment above names, by the launcher's own answer (qd_attn_i8_form): both families where the
    # shape is LDS-eligible, and the register-fed kernel with constant-operand MFMAs for an asymmetric q without a table
    if d % 32 and d < 64 and Sp <= 16384:
        assert len({f[0] for f in forms.values()}) >= 2, forms
    if ap.asym:
        assert forms[(3, 0)][0] == 1 and forms[(3, 0)][2] == 1, forms
    ref = outs[(0, 1)]
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    for key, o in outs.items():
        assert torch.equal(ref, o), (key, (ref - o).abs().max().item())


def test_attention_keyterm_table(cuda):
    """qd_attn_keyterm: seeds 0x4B400000 - zq' * (row sums of the stored K bytes), for dpad 64 and 32."""
    from qdiff import hip
    g = torch.Generator().manual_seed(5)
    for BH, Spad, dpad, zq in ((6, 96, 64, -9), (4, 160, 32, -128), (3, 4096, 64, 127), (5, 1024, 96, -77)):
        k8 = torch.randint(-128, 128, (BH, Spad, dpad), dtype=torch.int8, generator=g)
        prm = torch.zeros(16)
        prm[1] = float(zq)
        got = hip.attn_keyterm(k8.to(cuda), BH, Spad, dpad, prm.to(cuda))
        torch.cuda.synchronize()
        want = (0x4B400000 - zq * k8.long().sum(-1)).to(torch.int32)
        assert torch.equal(got.cpu(), want)


# The block form each case below must take WITH two K-groups, asserted through qd_conv2d_i8_form: (rows, columns, threads); without
# them the same tile on 256 threads.  Every N % 320 == 0 case runs the 128 x 320 tile of 2 x 2 waves here, whatever its K and
# block count: this file lowers that tile's thresholds through the environment (QD_WIDE_MINBLK / QD_WIDE_MINK above).  The
# 128 x 160 and 256-row forms of the variant are compared in test_random_shapes_gpu.py (N = 160) and test_conv_tall_tiles_gpu.py.
_K2_CASES = [
    ((2, 1280, 16, 1280, 3, 4, torch.float32), (128, 320, 512)),     # SD 16 x 16 level: 180 K-steps
    ((4, 640, 32, 640, 3, 4, torch.float32), (128, 320, 512)),       # SD 32 x 32 level: 90 K-steps
    ((1, 320, 64, 320, 3, 4, torch.float32), (128, 320, 512)),       # 45 K-steps (odd: the second group's last round is a zero stage)
    ((2, 1280, 16, 1280, 1, 4, torch.float32), (128, 320, 512)),     # 1 x 1, 20 K-steps (+ head-layout epilogues: 8 heads of 160)
    ((2, 640, 16, 320, 1, 4, torch.float32), (128, 320, 512)),       # heads of 40 on 10 steps
    ((16, 1280, 8, 1280, 3, 4, torch.float32), (128, 320, 512)),     # 8 x 8 level: split-K partials (second half of the test)
    ((2, 1920, 16, 1280, 3, 4, torch.float32), (128, 320, 512)),
    ((3, 200, 16, 320, 3, 4, torch.float32), (128, 320, 512)),       # K tail (200 = 3 x 64 + 8), odd step counts
    ((2, 448, 32, 448, 3, 4, torch.float32), (128, 224, 512)),       # LDM-4: 224-wide tiles
    ((2, 672, 16, 896, 1, 4, torch.float32), (128, 224, 512)),
    ((8, 256, 16, 256, 3, 8, torch.float32), (128, 128, 512)),       # CIFAR int8: 128-wide
    ((4, 128, 32, 128, 3, 8, torch.float32), (128, 128, 512)),
    ((2, 192, 16, 64, 3, 4, torch.float32), (128, 64, 256)),         # 64-wide: no two-K-group form, compares trivially equal
    ((2, 1280, 16, 1280, 3, 4, torch.float16), (128, 320, 256)),     # fp16 rows on the 128 x 320 tile: the four-wave block only,
    ((4, 640, 32, 640, 3, 4, torch.float16), (128, 320, 256))]       # trivially equal (the variant's fp16 form is the 128 x 160 tile's)
_K2_FORMS = dict(_K2_CASES)


@pytest.mark.parametrize("B,Cin,H,Cout,k,wbits,dt", [c for c, _ in _K2_CASES])
def test_conv_two_k_groups_equal_the_four_wave_block(cuda, B, Cin, H, Cout, k, wbits, dt):
    """Round 6: launches with at most one tile per CU run 512-thread blocks whose two groups of four waves contract alternate
    K-steps and add their int32 accumulators in LDS (igemm_body, KS = 2).  Integer adds commute: the output — rows, with
    row bias, residual and GroupNorm statistics of the epilogue — equals the four-wave kernel's bit for bit (qd_conv_config
    switches the variant; shapes the variant is not built for fall back and compare trivially equal)."""
    from conv_tall_tile_cases import launch_forms
    from qdiff import engine, hip
    form = _K2_FORMS[(B, Cin, H, Cout, k, wbits, dt)]
    g = torch.Generator().manual_seed(61)
    x = F.silu(torch.randn(B, Cin, H, H, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    q = _weight_quantizer(w, wbits, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], k, k, 1, k // 2, torch.randn(Cout, generator=g).to(cuda))
    rows = x.permute(0, 2, 3, 1).reshape(B * H * H, Cin).contiguous().to(cuda)
    xq = engine.quantize_rows(rows, plan, 1, Cin, B * H * H, (0, 1, Cin))
    residual = (torch.randn(B * H * H, Cout, generator=g)).to(cuda).to(dt)
    rowbias = torch.randn(B, Cout, generator=g).to(cuda)
    outs = {}
    try:
        for kg in (1, 0):
            hip.conv_config(kgroups=kg)
            with launch_forms() as forms:
                o = engine.conv_forward(plan, xq, B, H, H, rowbias=rowbias, residual=residual, out_dtype=dt, splitk=False, gn_stats=(H * H) % 128 == 0)
            assert forms == [(form[0], form[1], form[2] if kg else 256, 1)], forms
            torch.cuda.synchronize()
            outs[kg] = (o.clone(), getattr(o, "qd_gn_part", None))
    finally:
        hip.conv_config(kgroups=1)
    assert torch.equal(outs[1][0], outs[0][0]) and torch.isfinite(outs[1][0].float()).all() and outs[1][0].float().abs().max() > 0
    if outs[0][1] is not None:
        assert torch.equal(outs[1][1], outs[0][1])
    # the same for the split-K schedule (partials of every K slice from two K-groups) and, on 1 x 1 layers with whole heads, for
    # the head-layout epilogues (q / k rows, transposed v + column sums)
    res = {}
    try:
        for kg in (1, 0):
            hip.conv_config(kgroups=kg)
            o = engine.conv_forward(plan, xq, B, H, H, residual=residual, out_dtype=dt)            # the library decides about split-K
            got = [o.clone()]
            T = H * H
            if k == 1 and T % 128 == 0 and Cout % 8 == 0 and (Cout // 8) % 4 == 0 and wbits == 4 and dt == torch.float32:
                d8 = Cout // 8
                mkq = lambda dl, zp: NS(delta=torch.tensor(dl), zero_point=torch.tensor(float(zp)), n_bits=8, sym=False)
                ap = engine.build_attn_plan(mkq(0.05, 128), mkq(0.05, 120), mkq(0.04, 131), NS(delta=torch.tensor(1.0 / 65535), zero_point=torch.tensor(0.0), n_bits=16, sym=False),
                                            1.0, 0.7, cuda)
                for which in (0, 2):
                    shape = (B * 8, engine.pad32(d8), engine.pad32(T)) if which == 2 else (B * 8, engine.pad32(T), engine.pad32(d8))
                    buf = torch.zeros(shape, dtype=torch.int8, device=cuda)
                    vs = torch.zeros((B * 8, engine.pad32(d8)), dtype=torch.int32, device=cuda)
                    engine.project_heads(plan, xq, B, T, 8, ap, which, buf, vs)
                    got += [buf, vs]
            torch.cuda.synchronize()
            res[kg] = got
    finally:
        hip.conv_config(kgroups=1)
    assert len(res[1]) == len(res[0]) and all(torch.equal(a, b) for a, b in zip(res[1], res[0]))


@pytest.mark.parametrize("T,N,K,H", [(128, 320, 320, 8), (256, 640, 640, 8), (512, 320, 1280, 8), (128, 288, 320, 8), (256, 1280, 320, 8),
                                     (128, 256, 640, 8),
                                     # the LDM AttentionBlock's role projections (QuantModule.head_plans): LDM-4 beds, 32 channels
                                     # per head at 448 / 672 / 896 channels; LSUN-churches LDM-8, 8 heads of 24 / 48 / 96
                                     (256, 448, 448, 14), (128, 672, 672, 21), (128, 896, 896, 28), (256, 192, 192, 8), (128, 384, 384, 8),
                                     (128, 768, 768, 8)])
def test_projection_heads_epilogue_matches_quantize_heads(cuda, T, N, K, H):
    _heads_epilogue_case(cuda, T, N, K, H, 4)


@pytest.mark.parametrize("T,N,K,H", [(256, 256, 256, 1), (128, 128, 256, 1), (128, 256, 128, 2), (384, 192, 64, 1)])
def test_projection_heads_epilogue_with_int8_weights(cuda, T, N, K, H):
    """The same epilogues behind int8 weights (128-wide tiles; the q / k / v convolutions of the CIFAR W8A8 attention block:
    one head as wide as the layer, 256 channels)."""
    _heads_epilogue_case(cuda, T, N, K, H, 8)


def _heads_epilogue_case(cuda, T, N, K, H, wbits):
    """q/k/v projections that write attention operand bytes from the GEMM epilogue (QD_EPI_HEADS_*) produce
    exactly the bytes (and V column sums) of the fp32 projection followed by qd_quantize_heads.  Round 5: head dims that are
    multiples of 8 (40 / 80 / 160 / 32) leave 8 codes per lane (two tiles per transposition); d = 36 keeps the 4-code form."""
    from qdiff import engine
    B = 2
    d = N // H
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B * T, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.1
    q = _weight_quantizer(w, wbits, True, g)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    aq = _aq(dx, zx)
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], 1, 1, 1, 0, bias.to(cuda))
    assert pack.tiled and pack.wbits == wbits and engine.heads_fusable(plan, T, H)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, B * T, (0, 1, K))
    y = engine.conv_forward(plan, xq, 1, 1, B * T)                       # fp32 projection [B*T][N]

    def mk(t, always_zero=False):
        dd, zz = R.uaq_init_scale(t, 8, False, False, "max", always_zero)
        return NS(delta=dd, zero_point=zz, n_bits=8, sym=False)
    yc = y.cpu()
    pre = 0.7
    aw = NS(delta=torch.tensor(1.0 / 65535), zero_point=torch.tensor(0.0), n_bits=16, sym=False)
    ap = engine.build_attn_plan(mk(yc * pre), mk(yc * pre), mk(yc), aw, 1.0, pre, cuda)
    Tpad, dpad = engine.pad32(T), engine.pad32(d)
    for which in (0, 1, 2):
        shape = (B * H, dpad, Tpad) if which == 2 else (B * H, Tpad, dpad)
        want = torch.zeros(shape, dtype=torch.int8, device=cuda)
        got = torch.zeros(shape, dtype=torch.int8, device=cuda)
        ws = torch.zeros((B * H, dpad), dtype=torch.int32, device=cuda)
        gs = torch.full((B * H, dpad), 7, dtype=torch.int32, device=cuda)   # project_heads must zero it itself
        engine.heads_from_float(ap, which, y, B, T, H, d, (T * N, N, d, 1), want, ws)
        engine.project_heads(plan, xq, B, T, H, ap, which, got, gs)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (which, (got != want).float().mean().item())
        if which == 2:
            assert torch.equal(gs, ws)
    # round 6: the three projections as ONE grouped launch (qd_conv2d_i8_group; three different weight matrices and input rows,
    # one shape) write exactly the bytes of three single launches — whichever tile the library picks, and also where it declines
    # to group (tile not built for groups) and falls back to single launches
    members, singles = [], []
    vs_g = torch.full((B * H, dpad), 5, dtype=torch.int32, device=cuda)
    vs_s = torch.full((B * H, dpad), 9, dtype=torch.int32, device=cuda)
    for which in (0, 1, 2):
        wi = torch.randn(N, K, generator=g) * 0.05
        xi = torch.randn(B * T, K, generator=g)
        pk = engine.pack_module_weights(wi.to(cuda), [_weight_quantizer(wi, wbits, True, g)], 0)
        di, zi = R.uaq_init_scale(xi, 8, False, False, "max")
        pl = engine.build_conv_plan(pk, [_aq(di, zi)], 1, 1, 1, 0, (torch.randn(N, generator=g) * 0.1).to(cuda))
        xqi = engine.quantize_rows(xi.to(cuda), pl, 1, K, B * T, (0, 1, K))
        shape = (B * H, dpad, Tpad) if which == 2 else (B * H, Tpad, dpad)
        bg, bs = torch.zeros(shape, dtype=torch.int8, device=cuda), torch.zeros(shape, dtype=torch.int8, device=cuda)
        members.append((pl, xqi, which, bg))
        singles.append((pl, xqi, which, bs))
    engine.project_heads_group(members, B, T, H, ap, vs_g)
    for pl, xqi, which, bs in singles:
        engine.project_heads(pl, xqi, B, T, H, ap, which, bs, vs_s)
    torch.cuda.synchronize()
    for (_, _, which, bg), (_, _, _, bs) in zip(members, singles):
        assert torch.equal(bg, bs) and bg.float().abs().max() > 0, which
    assert torch.equal(vs_g, vs_s)


def test_grouped_projections_where_the_single_launch_takes_the_tall_tile(cuda):
    """M = 2 x 16384 rows, N = 320, int4 weights: the smallest M at which a single launch takes 256-row tiles (256 of them: one
    per CU) while a member of a grouped launch takes 128-row tiles.  (a) the q / k / v group of one shape writes exactly the
    bytes and V column sums of three single launches; (b) so does the group whose q member has N = 640 — a shape mismatch, which
    makes the library run every member as the single launch it would be on its own."""
    from qdiff import engine, hip
    B, T, H, K = 2, 16384, 8, 64
    g = torch.Generator().manual_seed(77)
    mkq = lambda dl, zp: NS(delta=torch.tensor(dl), zero_point=torch.tensor(float(zp)), n_bits=8, sym=False)
    ap = engine.build_attn_plan(mkq(0.05, 128), mkq(0.05, 120), mkq(0.04, 131), NS(delta=torch.tensor(1.0 / 65535), zero_point=torch.tensor(0.0), n_bits=16, sym=False),
                                1.0, 0.7, cuda)

    def member(N):
        wi = torch.randn(N, K, generator=g) * 0.05
        xi = torch.randn(B * T, K, generator=g)
        pk = engine.pack_module_weights(wi.to(cuda), [_weight_quantizer(wi, 4, True, g)], 0)
        di, zi = R.uaq_init_scale(xi, 8, False, False, "max")
        pl = engine.build_conv_plan(pk, [_aq(di, zi)], 1, 1, 1, 0, (torch.randn(N, generator=g) * 0.1).to(cuda))
        assert engine.heads_fusable(pl, T, H)
        return pl, engine.quantize_rows(xi.to(cuda), pl, 1, K, B * T, (0, 1, K))

    q320, q640, k320, v320 = member(320), member(640), member(320), member(320)
    probe = torch.zeros((B * H, engine.pad32(T), engine.pad32(40)), dtype=torch.int8, device=cuda)
    assert hip.conv2d_i8_form(engine._heads_call(*q320, B, T, H, ap, 0, probe, None))[:2] == (256, 160)
    for q in (q320, q640):
        bufs = {}
        for how in ("group", "single"):
            outs = []
            for (pl, xq), which in zip((q, k320, v320), (0, 1, 2)):
                dpad = engine.pad32(pl.Cout // H)
                shape = (B * H, dpad, engine.pad32(T)) if which == 2 else (B * H, engine.pad32(T), dpad)
                outs.append(torch.zeros(shape, dtype=torch.int8, device=cuda))
            vs = torch.full((B * H, engine.pad32(40)), 5 if how == "group" else 9, dtype=torch.int32, device=cuda)
            if how == "group":
                engine.project_heads_group([(pl, xq, which, o) for ((pl, xq), which, o) in zip((q, k320, v320), (0, 1, 2), outs)], B, T, H, ap, vs)
            else:
                for (pl, xq), which, o in zip((q, k320, v320), (0, 1, 2), outs):
                    engine.project_heads(pl, xq, B, T, H, ap, which, o, vs)
            bufs[how] = outs + [vs]
        torch.cuda.synchronize()
        for a, b in zip(bufs["group"], bufs["single"]):
            assert torch.equal(a, b) and a.float().abs().max() > 0, q[0].Cout


def test_attention_quantised_output_matches_quantise_rows(cuda):
    """qd_attn_i8 with out8: the bytes equal K1 applied to its own fp32 output (same float, same rounding)."""
    from qdiff import engine
    B, H, T, S, d = 2, 8, 160, 77, 40
    g = torch.Generator().manual_seed(41)
    C = H * d
    q, k, v = (torch.randn(B, L, C, generator=g) for L in (T, S, S))

    def mk(t, n_bits=8, always_zero=False):
        dd, zz = R.uaq_init_scale(t, n_bits, False, False, "max", always_zero)
        return NS(delta=dd, zero_point=zz, n_bits=n_bits, sym=False)
    heads = lambda t, L: t.view(B, L, H, d).permute(0, 2, 1, 3).reshape(B * H, L, d)
    p = (torch.einsum("bid,bjd->bij", heads(q, T), heads(k, S)) * d ** -0.5).softmax(-1)
    ap = engine.build_attn_plan(mk(q), mk(k), mk(v), mk(p, 16, True), d ** -0.5, 1.0, cuda)
    Tp, Sp, dp = engine.pad32(T), engine.pad32(S), engine.pad32(d)
    q8 = torch.zeros((B * H, Tp, dp), dtype=torch.int8, device=cuda)
    k8 = torch.zeros((B * H, Sp, dp), dtype=torch.int8, device=cuda)
    v8 = torch.zeros((B * H, dp, Sp), dtype=torch.int8, device=cuda)
    vsum = torch.zeros((B * H, dp), dtype=torch.int32, device=cuda)
    for which, (t, L, buf) in enumerate(((q, T, q8), (k, S, k8), (v, S, v8))):
        engine.heads_from_float(ap, which, t.to(cuda), B, L, H, d, (L * C, C, d, 1), buf, vsum)
    o = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d)
    # consumer: a Linear with C inputs whose act quantiser is initialised on the attention output
    w = torch.randn(C, C, generator=g) * 0.05
    wq = _weight_quantizer(w, 4, True, g)
    do, zo = R.uaq_init_scale(o.cpu(), 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [wq], 0), [_aq(do, zo)], 1, 1, 1, 0, None)
    want = engine.quantize_rows(o, plan, 1, C, B * T, (0, 1, C))
    got = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d, out_plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,C,H,Cout,k", [(2, 64, 16, 320, 3), (3, 320, 16, 160, 1), (1, 96, 32, 640, 3)])
def test_conv_emits_groupnorm_statistics(cuda, B, C, H, Cout, k):
    """gn_stats=True: the GEMM epilogue writes per-128-row {sum, sumsq} of its own output; GroupNorm fed with them
    produces the same codes as the two-pass kernel (statistics differ only by fp32 summation order)."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(51)
    x = F.silu(torch.randn(B, C, H, H, generator=g))
    w = torch.randn(Cout, C, k, k, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], k, k, 1, k // 2, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, C, H * H, (C * H * H, H * H, 1))
    res = torch.randn(B * H * H, Cout, generator=g).to(cuda)
    out = engine.conv_forward(plan, xq, B, H, H, residual=res, gn_stats=True, splitk=False)
    ref = engine.conv_forward(plan, xq, B, H, H, residual=res, splitk=False)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and hasattr(out, "qd_gn_part")
    part = out.qd_gn_part.cpu().double()
    ch = ref.cpu().double().view(B, H * H // 128, 128, Cout)
    want = torch.stack([ch.sum(2), (ch * ch).sum(2)], dim=-1)
    assert (part - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    # consumer
    gn = torch.nn.GroupNorm(32, Cout).to(cuda)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(Cout, generator=g)); gn.bias.copy_(torch.randn(Cout, generator=g))
    y = F.silu(F.group_norm(ref.view(B, H * H, Cout).permute(0, 2, 1), 32, gn.weight, gn.bias, gn.eps)).cpu()
    dy, zy = R.uaq_init_scale(y, 8, False, False, "max")
    w2 = torch.randn(32, Cout, 1, 1, generator=g) * 0.05
    plan2 = engine.build_conv_plan(engine.pack_module_weights(w2.to(cuda), [_weight_quantizer(w2, 4, True, g)], 0), [_aq(dy, zy)], 1, 1, 1, 0, None)
    a, _ = engine.groupnorm_silu_quant(ref, B, H * H, Cout, gn, True, plan=plan2)
    b, _ = engine.groupnorm_silu_quant(out, B, H * H, Cout, gn, True, plan=plan2, part=out.qd_gn_part)
    torch.cuda.synchronize()
    diff = (a.int() - b.int()).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() <= 1e-3


@pytest.mark.parametrize("B,H,C1,C2,Cmid", [(2, 16, 320, 160, 320), (1, 32, 640, 320, 160)])
def test_concatenation_slot_and_raw_quant(cuda, B, H, C1, C2, Cmid):
    """engine.CatSlot: two convolutions write their outputs and GroupNorm statistics into the two column ranges of one
    buffer (ldo / gn_ld); the concatenation is a view whose values and statistics equal those of the separately
    allocated outputs, and GroupNorm over the view — reading strided rows and strided statistics (part_ld) — gives the
    codes of GroupNorm over the copied concatenation.  qd_raw_quant: the split 1x1 skip connection's int8 rows written
    by the same pass are bit-identical to qd_quantize_act's."""
    from qdiff import engine, quant_block as qb
    g = torch.Generator().manual_seed(71)
    S = H * H
    plans, xqs, outs_plain = [], [], []
    for Cout in (C1, C2):
        x = F.silu(torch.randn(B, Cmid, H, H, generator=g))
        w = torch.randn(Cout, Cmid, 3, 3, generator=g) * 0.05
        d, z = R.uaq_init_scale(x, 8, False, False, "max")
        plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(d, z)], 3, 3, 1, 1,
                                      torch.randn(Cout, generator=g).to(cuda))
        plans.append(plan)
        xqs.append(engine.quantize_rows(x.to(cuda), plan, B, Cmid, S, (Cmid * S, S, 1)))
        outs_plain.append(engine.conv_forward(plan, xqs[-1], B, H, H, gn_stats=True, splitk=False))
    slot = engine.CatSlot(C1, C2)
    a = engine.conv_forward(plans[0], xqs[0], B, H, H, gn_stats=True, splitk=False, slot=slot.side(0))
    b = engine.conv_forward(plans[1], xqs[1], B, H, H, gn_stats=True, splitk=False, slot=slot.side(1))
    torch.cuda.synchronize()
    assert a.stride(0) == C1 + C2 and b.stride(0) == C1 + C2 and b.data_ptr() == a.data_ptr() + 4 * C1
    assert torch.equal(a, outs_plain[0]) and torch.equal(b, outs_plain[1])
    assert torch.equal(a.qd_gn_part, outs_plain[0].qd_gn_part) and torch.equal(b.qd_gn_part, outs_plain[1].qd_gn_part)
    cat = qb.cat_channels(qb._rows_to_nchw(a, B, H, H), qb._rows_to_nchw(b, B, H, H))
    copy = torch.cat([qb._rows_to_nchw(outs_plain[0], B, H, H), qb._rows_to_nchw(outs_plain[1], B, H, H)], dim=1)
    assert cat.data_ptr() == a.data_ptr() and torch.equal(cat, copy)                   # a view of the slot buffer
    assert cat.qd_gn_part.data_ptr() == a.qd_gn_part.data_ptr() and cat.qd_gn_part.shape[2] == C1 + C2
    # consumers of the concatenation: GroupNorm -> conv1's rows, and the split skip connection's rows from the same pass
    C = C1 + C2
    gn = torch.nn.GroupNorm(32, C).to(cuda)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g)); gn.bias.copy_(torch.randn(C, generator=g))
    y = F.silu(gn(copy)).cpu()
    dy, zy = R.uaq_init_scale(y, 8, False, False, "max")
    w1 = torch.randn(32, C, 1, 1, generator=g) * 0.05
    plan1 = engine.build_conv_plan(engine.pack_module_weights(w1.to(cuda), [_weight_quantizer(w1, 4, True, g)], 0), [_aq(dy, zy)], 1, 1, 1, 0, None)
    wsk = torch.randn(64, C, 1, 1, generator=g) * 0.05
    qs = [_weight_quantizer(wsk[:, :C1], 4, True, g), _weight_quantizer(wsk[:, C1:], 4, True, g)]
    cc = copy.cpu()
    aqs = [_aq(*R.uaq_init_scale(cc[:, :C1], 8, False, False, "max")), _aq(*R.uaq_init_scale(cc[:, C1:], 8, False, False, "max"))]
    plan_sk = engine.build_conv_plan(engine.pack_module_weights(wsk.to(cuda), qs, C1), aqs, 1, 1, 1, 0, None)
    rows_view, rows_copy = qb._nhwc_rows(cat), qb._nhwc_rows(copy)
    assert rows_view.stride(0) == C and rows_view.data_ptr() == a.data_ptr()
    ref_codes, _ = engine.groupnorm_silu_quant(rows_copy, B, S, C, gn, True, plan=plan1)                    # two-pass statistics, copy
    got_codes, _, got_raw = engine.groupnorm_silu_quant(rows_view, B, S, C, gn, True, plan=plan1, part=rows_view.qd_gn_part,
                                                        raw_plan=plan_sk)
    ref_raw = engine.quantize_rows(copy, plan_sk, B, C, S, (C * S, 1, C))
    torch.cuda.synchronize()
    diff = (ref_codes.int() - got_codes.int()).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() <= 1e-3
    assert torch.equal(got_raw, ref_raw)
    # one side of the slot read on its own (the encoder's next block): strided rows and a strided statistics column range
    gn2 = torch.nn.GroupNorm(32, C2).to(cuda)
    y2 = F.silu(gn2(qb._rows_to_nchw(outs_plain[1], B, H, H))).cpu()
    d2, z2 = R.uaq_init_scale(y2, 8, False, False, "max")
    w2 = torch.randn(32, C2, 1, 1, generator=g) * 0.05
    plan2 = engine.build_conv_plan(engine.pack_module_weights(w2.to(cuda), [_weight_quantizer(w2, 4, True, g)], 0), [_aq(d2, z2)], 1, 1, 1, 0, None)
    r1, _ = engine.groupnorm_silu_quant(outs_plain[1], B, S, C2, gn2, True, plan=plan2, part=outs_plain[1].qd_gn_part)
    r2, _ = engine.groupnorm_silu_quant(b, B, S, C2, gn2, True, plan=plan2, part=b.qd_gn_part)
    torch.cuda.synchronize()
    assert torch.equal(r1, r2)


def test_linear_residual_to_int8_rows_matches_unfused(cuda):
    """QD_EPI_HEADS_I8 with one full-width head + fp32 residual == fp32 Linear(+residual) followed by K1."""
    from qdiff import engine
    B, T, K, N = 2, 256, 1280, 320
    g = torch.Generator().manual_seed(61)
    x = torch.randn(B * T, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.03
    bias = torch.randn(N, generator=g) * 0.1
    res = torch.randn(B * T, N, generator=g).to(cuda)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(dx, zx)], 1, 1, 1, 0, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, B * T, (0, 1, K))
    y = engine.conv_forward(plan, xq, 1, 1, B * T, residual=res)
    w2 = torch.randn(64, N, generator=g) * 0.05
    dy, zy = R.uaq_init_scale(y.cpu(), 8, False, False, "max")
    nxt = engine.build_conv_plan(engine.pack_module_weights(w2.to(cuda), [_weight_quantizer(w2, 4, True, g)], 0), [_aq(dy, zy)], 1, 1, 1, 0, None)
    assert engine.rows_i8_fusable(plan, nxt, T)
    want = engine.quantize_rows(y, nxt, 1, N, B * T, (0, 1, N))
    got = engine.linear_to_rows_i8(plan, xq, B, T, nxt, residual=res)
    torch.cuda.synchronize()
    assert torch.equal(got, want)



def test_standalone_qk_smv_matmuls_vs_reference_golden(cuda):
    """QuantQKMatMul / QuantSMVMatMul on their own through qd_bmm_qk_i8 / qd_bmm_pv_i8 vs the real reference's
    outputs (tests/golden/ops.pt, ldm_qk_smv): exact integers and one fp32 multiply -> 2e-6 of range."""
    from golden_util import load_fixture
    from test_host_logic import _standalone_matmul_modules
    c = [a for a in load_fixture("ops.pt")["attention"] if a["kind"] == "ldm_qk_smv"][0]
    qk, smv = _standalone_matmul_modules(c)
    qk, smv = qk.to(cuda), smv.to(cuda)
    with torch.no_grad():
        w = qk(c["q"].to(cuda), c["k"].to(cuda)).cpu()
        a = smv(torch.softmax(c["weight"].float(), dim=-1).to(cuda), c["v"].to(cuda)).cpu()
    assert (w - c["weight"]).abs().max() <= 2e-6 * c["weight"].abs().max()
    assert (a - c["out"]).abs().max() <= 2e-6 * c["out"].abs().max()


@pytest.mark.parametrize("smb", [8, 16])
def test_standalone_bmm_kernels_asymmetric_ragged(cuda, smb):
    """Asymmetric 8-bit q/k/v, 8/16-bit probabilities, ragged T/S, d=40: vs the fp64 evaluation of the reference formula."""
    from qdiff import engine
    BH, d, T, S = 6, 40, 100, 77
    g = torch.Generator().manual_seed(71)
    q, k, v = (torch.randn(BH, d, L, generator=g) for L in (T, S, S))
    scale = d ** -0.25

    def mk(t, n_bits=8, always_zero=False):
        dd, zz = R.uaq_init_scale(t, n_bits, False, False, "max", always_zero)
        return NS(delta=dd, zero_point=zz, n_bits=n_bits, sym=False, inited=True, running_stat=False)
    aq_q, aq_k, aq_v = mk(q * scale), mk(k * scale), mk(v)
    # codes with the reference's fp32 arithmetic (IEEE division, round-half-even), contraction in fp64
    fq = lambda t, a: (torch.clamp(torch.round(t.float() / a.delta.float()) + float(a.zero_point), 0, 2 ** a.n_bits - 1)
                       - float(a.zero_point)).double() * float(a.delta)
    want_w = torch.einsum("bct,bcs->bts", fq(q * torch.tensor(scale), aq_q), fq(k * torch.tensor(scale), aq_k))
    got_w = engine.qk_matmul_int(aq_q, aq_k, q.to(cuda), k.to(cuda), scale).cpu()
    assert (got_w.double() - want_w).abs().max() <= 2e-6 * want_w.abs().max()
    p = torch.softmax(got_w, dim=-1)
    aq_w = mk(p, smb, always_zero=True)
    want_a = torch.einsum("bts,bcs->bct", fq(p, aq_w), fq(v, aq_v))
    got_a = engine.smv_matmul_int(aq_w, aq_v, p.to(cuda), v.to(cuda)).cpu()
    assert (got_a.double() - want_a).abs().max() <= 2e-6 * want_a.abs().max()


@pytest.mark.parametrize("w_bits,B,K,widths", [(4, 16, 1280, (320, 640, 1280, 320)), (4, 5, 224, (224, 448)), (8, 64, 512, (128, 256, 256)),
                                                (4, 40, 1280, (1280,)),
                                                (8, 300, 128, (512,)), (8, 700, 128, (512, 128))])   # > 256 rows per launch (K = 128: the DDIM time MLP)
def test_temb_mlp_equals_generic_path(cuda, w_bits, B, K, widths):
    """K6 (qd_temb_mlp): L Linears sharing one input, each with its own activation quantiser, in one launch — equal BIT FOR
    BIT to qd_quantize_act + qd_conv2d_i8 per layer (same codes, same integers, same float order); with the SiLU folded in,
    equal to the generic path on torch's SiLU up to the last ulp of exp() (codes may flip on exact ties only)."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(81)
    x = torch.randn(B, K, generator=g) * 1.5
    plans = []
    for i, n in enumerate(widths):
        w = torch.randn(n, K, generator=g) * 0.05
        q = _weight_quantizer(w, w_bits, True, g)
        for silu_in in (x, F.silu(x)):
            pass
        d, z = R.uaq_init_scale(F.silu(x) * (1.0 + 0.1 * i), 8, False, False, "max")
        plans.append(engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], 1, 1, 1, 0,
                                            (torch.randn(n, generator=g) * 0.1).to(cuda)))
    offs, tot = [], 0
    for n in widths:
        offs.append(tot)
        tot += (n + 63) // 64 * 64
    xd = x.to(cuda)
    for silu in (False, True):
        out = torch.full((B, tot), float("nan"), device=cuda)
        hip.temb_mlp(xd, silu, plans, offs, out)
        y = F.silu(xd) if silu else xd
        torch.cuda.synchronize()
        for p, off in zip(plans, offs):
            xq = engine.quantize_rows(y, p, 1, K, B, (0, 1, K))
            want = engine.conv_forward(p, xq, 1, 1, B, 1, B, splitk=False)
            got = out[:, off:off + p.Cout]
            if not silu:
                assert torch.equal(got, want)
            else:
                bad = (got != want).float().mean().item()
                assert bad <= 2e-2 and (got - want).abs().max().item() <= 2e-3 * want.abs().max().item(), (bad,)


@pytest.mark.parametrize("sym,shape", [(False, (4, 320, 32, 32)), (True, (3, 77, 768)), (False, (5, 1031))])
def test_fused_fakequant_forward_backward_matches_autograd(cuda, sym, shape):
    """csrc/fakequant.hip vs the autograd composition of UniformAffineQuantizer.forward (reference quant_layer.py:82-88 with
    round_ste :16-20): y and dL/dx bit-identical, dL/d(delta) to summation order (1e-5 relative)."""
    from qdiff import quant_layer as ql
    g = torch.Generator().manual_seed(91)
    x = (torch.randn(shape, generator=g) * 1.3).to(cuda)
    w = torch.randn(shape, generator=g).to(cuda)
    q = ql.UniformAffineQuantizer(n_bits=8, symmetric=sym, channel_wise=False, scale_method="max", leaf_param=True)
    with torch.no_grad():
        q(x * 0.8)                                            # data-dependent init on a narrower tensor: some codes clamp
    res = {}
    for fused in (False, True):
        ql.FUSED_FAKEQUANT = fused
        xi = x.clone().requires_grad_(True)
        q.delta.grad = None
        y = q(xi)
        (y * w).sum().backward()
        res[fused] = (y.detach().clone(), xi.grad.clone(), q.delta.grad.clone())
    ql.FUSED_FAKEQUANT = True
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    # dL/d(delta) is a sum of N signed terms that largely cancel: both the fused kernel and autograd's composition are
    # judged against the fp64 evaluation of the same terms, relative to the sum of their magnitudes
    lo, hi = q.code_range()
    dl = q.delta.detach()
    zpv = float(q.zero_point) if not torch.is_tensor(q.zero_point) else float(q.zero_point.reshape(-1)[0])
    dv = x / dl
    codes = torch.round(dv) + zpv
    qv = codes.clamp(lo, hi)
    mask = ((codes >= lo) & (codes <= hi)).double()
    a = w.double() * (qv.double() - zpv)
    b = (w.double() * dl.double()) * mask * (dv.double() / dl.double())
    truth, scale = float((a - b).sum()), float(a.abs().sum() + b.abs().sum())
    gd_f, gd_c = float(res[True][2]), float(res[False][2])
    assert abs(gd_f - truth) <= 1e-5 * scale, (gd_f, gd_c, truth, scale)
    assert abs(gd_c - truth) <= 1e-5 * scale, (gd_f, gd_c, truth, scale)
    assert bool(((codes < lo) | (codes > hi)).any()), "the test tensor never clamps"


@pytest.mark.parametrize("B,C,h,Cout,wb", [(2, 640, 16, 640, 4), (1, 96, 8, 320, 4), (2, 320, 32, 320, 4), (16, 256, 8, 1280, 4), (3, 128, 4, 128, 8)])
def test_conv_folds_nearest_upsampling(cuda, B, C, h, Cout, wb):
    """qd_conv_desc.upsample2x: the gather kernel reads the half-resolution int8 map and convolves its nearest-neighbour 2x
    up-sampling (reference openaimodel.py:105-120: F.interpolate(nearest) then conv) — bit-identical to replicating the
    int8 rows first and running the plain descriptor; the (16, 256, 8, 1280) case takes the split-K schedule."""
    from qdiff import engine
    g = torch.Generator().manual_seed(31)
    x = F.silu(torch.randn(B, C, h, h, generator=g))
    w = torch.randn(Cout, C, 3, 3, generator=g) * 0.05
    q = _weight_quantizer(w, wb, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], 3, 3, 1, 1,
                                  torch.randn(Cout, generator=g).to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, C, h * h, (C * h * h, h * h, 1))
    up = xq.view(B, h, 1, h, 1, -1).expand(B, h, 2, h, 2, xq.shape[1]).reshape(B * 4 * h * h, xq.shape[1])
    assert engine.upsample_fold_ok(plan, 2 * h, 2 * h)
    for kw in (dict(gn_stats=True, splitk=False), dict()):
        want = engine.conv_forward(plan, up, B, 2 * h, 2 * h, **kw)
        got = engine.conv_forward(plan, xq, B, 2 * h, 2 * h, upsample2x=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        if hasattr(want, "qd_gn_part"):
            assert torch.equal(got.qd_gn_part, want.qd_gn_part)
