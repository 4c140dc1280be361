"""GPU tests at the VALUE edges of the integer kernels (the shape edges are tests/test_hip_kernels.py and
tests/test_random_shapes_gpu.py): exact rounding ties, clamp boundaries, +-inf and huge finite inputs, zero points at the grid
ends, grids that clip a large share of their inputs, saturated contraction operands, degenerate and offset normalisation
statistics, and the grouped-launch contract.

Every reference is the oracle (oracle/quant_ref.py) or an fp64 evaluation of the reference formula.  Pure quantisers are
compared bit for bit; producers with float work before the quantiser through tests/edge_util.tie_aware_check (rule and
derivation of its window w in that module and at each use).  Run with -s to see the accepted tie-window mismatches.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from edge_util import device_rows, edge_values, f32_from_bits, params, tie_aware_check
from oracle import quant_ref as R
from test_hip_kernels import _aq, _codes, _weight_quantizer

pytestmark = pytest.mark.gpu

DELTA_FAST = 0.037                          # certified for the three-instruction quotient (qd_make_qparams)
DELTA_SLOW = f32_from_bits(0x3cffffff)      # all-ones mantissa (0.031249998); its flag is cleared by hand -> IEEE division


def _grid(n_bits, sym):
    from qdiff import engine
    return engine.act_grid(n_bits, sym)


# (id, n_bits, sym, zero point)
QGRIDS = [(f"u8_zp{z}", 8, False, z) for z in (0, 1, 127, 128, 254, 255)] + \
         [(f"u4_zp{z}", 4, False, z) for z in (0, 7, 15)] + [("s8", 8, True, 0)]


def _qparams(cuda, delta, zp, fast):
    """fast: the certified three-instruction quotient (the flag must be set for this delta); else the flag is cleared, which
    is what the kernels see for a delta the certificate rejects: the IEEE division path."""
    from qdiff import hip
    qp = hip.make_qparams(torch.tensor(delta, device=cuda), torch.tensor(float(zp), device=cuda))
    if fast:
        assert qp.cpu()[3].item() != 0, f"delta {delta!r} is not certified"
    else:
        qp[3] = 0.0
    return qp


# ------------------------------------------------------------------------------------------------
# (a) quantisers with no float work before them: bit-exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("path", ["fastdiv", "ieee_div"])
@pytest.mark.parametrize("qg", QGRIDS, ids=[c[0] for c in QGRIDS])
def test_quantize_act_value_edges(cuda, qg, path, dtype, layout):
    """qd_quantize_act on exact ties, clamp boundaries (+- 0.5 code and the fp32 neighbours), +-0, huge finite values up to
    FLT_MAX and +-inf: codes equal the oracle's clamp(round(x / delta) + zp) bit for bit on both quotient paths.  NCHW
    takes the strided kernel, NHWC the row kernel with a 37-channel tail (the scalar run-time quotient)."""
    from qdiff import hip
    _, n_bits, sym, zp = qg
    delta = DELTA_FAST if path == "fastdiv" else DELTA_SLOW
    grid = _grid(n_bits, sym)
    qmin, qmax = R.code_range(n_bits, sym)
    g = torch.Generator().manual_seed(1000 + zp + n_bits)
    B, C, H, W = 2, 37, 5, 8
    v, nties = edge_values(delta, zp, qmin, qmax, B * C * H * W, g, half=(dtype == "f16"))
    if dtype == "f32":
        assert nties >= 4, "no exact ties were constructed"
    v = v[:B * C * H * W]
    x = v[torch.randperm(v.numel(), generator=g)].view(B, C, H, W)
    xd = x.to(cuda).half() if dtype == "f16" else x.to(cuda)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    qp = _qparams(cuda, delta, zp, path == "fastdiv")
    S = H * W
    sb, sc, sh, sw = xd.stride()
    ldo = hip.pad16(C) + 16
    out = torch.full((B * S, ldo), 77, dtype=torch.int8, device=cuda)
    hip.quantize_act(xd, B, C, S, (sb, sc, sw), qp, grid, out, ldo, oc0=16)
    torch.cuda.synchronize()
    want = R.uaq_codes(xd.float().cpu(), torch.tensor(delta), zp, n_bits, sym) - grid.off
    got = out.cpu().view(B, H, W, ldo)[..., 16:16 + C].permute(0, 3, 1, 2).long()
    bad = got != want
    assert not bool(bad.any()), (f"{int(bad.sum())} codes differ; inputs {xd.float().cpu()[bad][:8].tolist()} "
                                 f"got {got[bad][:8].tolist()} want {want[bad][:8].tolist()}")


@pytest.mark.parametrize("path", ["fastdiv", "ieee_div"])
@pytest.mark.parametrize("zp", [0, 128, 255], ids=["u8_zp0", "u8_zp128", "u8_zp255"])
def test_quantize_heads_value_edges(cuda, zp, path):
    """qd_quantize_heads (row layout) on the same edge values: codes and their per-(head, token) sums equal the oracle's."""
    from qdiff import hip
    delta = DELTA_FAST if path == "fastdiv" else DELTA_SLOW
    grid = _grid(8, False)
    g = torch.Generator().manual_seed(77 + zp)
    B, T, H, d = 2, 45, 2, 32
    v, _ = edge_values(delta, zp, 0, 255, B * T * H * d, g)
    x = v[:B * T * H * d][torch.randperm(B * T * H * d, generator=g)].view(B, T, H * d)
    Tpad, dpad = hip.pad32(T), hip.pad32(d)
    out = torch.zeros((B * H, Tpad, dpad), dtype=torch.int8, device=cuda)
    rsum = torch.zeros((B * H, Tpad), dtype=torch.int32, device=cuda)
    qp = _qparams(cuda, delta, zp, path == "fastdiv")
    hip.quantize_heads(x.to(cuda), B, T, H, d, (T * H * d, H * d, d, 1), 1.0, qp, grid, False, out, rsum, Tpad, dpad)
    torch.cuda.synchronize()
    want = (R.uaq_codes(x, torch.tensor(delta), zp, 8, False) - grid.off).view(B, T, H, d).permute(0, 2, 1, 3).reshape(B * H, T, d)
    got = out.cpu()[:, :T, :d].long()
    assert torch.equal(got, want), f"{int((got != want).sum())} codes differ"
    assert torch.equal(rsum.cpu()[:, :T].long(), want.sum(-1))


def test_certificate_rejects_a_delta_and_its_division_path_saturates(cuda):
    """qd_make_qparams refuses the fast quotient for delta >= 3e38 (x * rinv would leave the normal range); the kernels then
    divide.  With delta = 3.1e38 the grid spans only zp - 1 .. zp + 1 of the finite range: exact ties +-delta/2 (a power-of-two
    scaling of delta, so the division is exactly 0.5) and their neighbours, +-delta, +-FLT_MAX and +-inf quantise to the
    oracle's codes on the flag the certificate itself wrote (not cleared by hand)."""
    from qdiff import hip
    grid = _grid(8, False)
    d = float(torch.tensor(3.1e38, dtype=torch.float32))
    qp = hip.make_qparams(torch.tensor(d, device=cuda), torch.tensor(128.0, device=cuda))
    assert qp.cpu()[3].item() == 0, "the certificate accepted delta = 3.1e38"
    h = torch.tensor(d / 2, dtype=torch.float32)
    near = [float(torch.nextafter(h, torch.tensor(v))) for v in (float("inf"), 0.0)]
    x = torch.tensor([0.0, -0.0, d / 2, -d / 2, d, -d, 3.4028235e38, -3.4028235e38, float("inf"), float("-inf"), 1.0, -1.0,
                      1e37, -1e37] + near + [-v for v in near], dtype=torch.float32).repeat(4)
    assert bool(((x[2:4] / torch.tensor(d)).abs() == 0.5).all())
    M = x.numel()
    out = torch.empty((1, hip.pad16(M)), dtype=torch.int8, device=cuda)
    hip.quantize_act(x.to(cuda), 1, M, 1, (0, 1, 0), qp, grid, out, hip.pad16(M))
    torch.cuda.synchronize()
    want = R.uaq_codes(x, torch.tensor(d), 128, 8, False) - 128
    assert torch.equal(out.cpu()[0, :M].long(), want), (out.cpu()[0, :M].tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------
# (f) fused fake-quant at ties and clamp boundaries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_fakequant_ties_and_clamp_boundaries(cuda, sym):
    """qd_fakequant_fwd / _bwd vs the autograd composition (quant_layer.UniformAffineQuantizer with the fused path off) on
    exact ties, values exactly at qmin / qmax (the clamp passes the gradient on the CLOSED interval), one code beyond them and
    the +-0.5 boundaries: y and dL/dx bit-identical, dL/d(delta) within 1e-5 of the fp64 sum's magnitude."""
    from qdiff import quant_layer as ql
    g = torch.Generator().manual_seed(93)
    q = ql.UniformAffineQuantizer(n_bits=8, symmetric=sym, channel_wise=False, scale_method="max", leaf_param=True)
    with torch.no_grad():
        q((torch.randn(4096, generator=g) * 1.3).to(cuda))
    lo, hi = q.code_range()
    dl = float(q.delta)
    zpv = float(q.zero_point) if not torch.is_tensor(q.zero_point) else float(q.zero_point.reshape(-1)[0])
    v, nties = edge_values(dl, zpv, lo, hi, 4000, g)
    v = v[torch.isfinite(v) & (v.abs() < 1e30)]                 # (the composition's round_ste turns inf into NaN)
    exact = torch.tensor([(lo - zpv) * dl, (hi - zpv) * dl, (lo - zpv - 1) * dl, (hi - zpv + 1) * dl], dtype=torch.float32)
    x = torch.cat([v, exact])
    x = torch.cat([x, x[: (-x.numel()) % 4 + 4]]).to(cuda)
    w = torch.randn(x.shape, generator=g).to(cuda)
    res = {}
    for fused in (False, True):
        ql.FUSED_FAKEQUANT = fused
        xi = x.clone().requires_grad_(True)
        q.delta.grad = None
        y = q(xi)
        (y * w).sum().backward()
        res[fused] = (y.detach().clone(), xi.grad.clone(), q.delta.grad.clone())
    ql.FUSED_FAKEQUANT = True
    assert nties >= 4
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    dv = x / q.delta.detach()
    codes = torch.round(dv) + zpv
    assert bool((codes == lo).any()) and bool((codes == hi).any()) and bool((codes < lo).any()) and bool((codes > hi).any())
    mask = ((codes >= lo) & (codes <= hi)).double()
    a = w.double() * (codes.clamp(lo, hi).double() - zpv)
    b = (w.double() * dl) * mask * (dv.double() / dl)
    truth, scale = float((a - b).sum()), float(a.abs().sum() + b.abs().sum())
    assert abs(float(res[True][2]) - truth) <= 1e-5 * scale


# ------------------------------------------------------------------------------------------------
# (c) contraction: exact int32 accumulators at saturation
# ------------------------------------------------------------------------------------------------
def _splitk_chosen(plan, xq, B, H, Ho):
    """The library would contract this layer split-K when allowed (else two of the four launch variants are one launch)."""
    from qdiff import hip
    out = torch.empty((B * Ho * Ho, plan.Cout), dtype=torch.float32, device=xq.device)
    call = hip.ConvCall(x=xq, w=plan.pack.wq, out=out, bias=plan.bias, ldx=plan.ldx, ldk=plan.pack.ldk, ldo=out.stride(0),
                        B=B, H=H, W=H, Ho=Ho, Wo=Ho, Cout=plan.Cout, kh=plan.kh, kw=plan.kw, stride=plan.stride,
                        pad_t=plan.pad, pad_l=plan.pad, wbits=plan.pack.wbits, w_tiled=plan.pack.tiled, segs=plan.segs)
    return hip.splitk_ws_bytes(call) > 0


def _sat_weights(Cout, Cin, k, w_bits, wzp, g):
    """Weights whose codes sit at the grid ends: per-channel delta a third of the max-scaled one (outliers clip), AdaRound
    alpha at +-10 (h(alpha) = 1 or 0 exactly), zero points at 0 / n_levels - 1 ("ends", alternating by channel) or max-init."""
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    w[:, ::7] *= 20.0
    q = _weight_quantizer(w, w_bits, True, g)
    q.delta = q.delta / 3.0
    nl = 2 ** w_bits
    if wzp == "ends":
        z = torch.zeros_like(q.zero_point)
        z.view(-1)[1::2] = nl - 1
        q.zero_point = z
    else:
        q.zero_point = torch.round(q.zero_point / 3.0 + nl / 3.0).clamp(0, nl - 1)
    q.alpha = torch.where(torch.rand(w.shape, generator=g) < 0.5, -10.0, 10.0)
    return w, q


# (id, activation pattern, activation zero point, B, Cin, H, Cout, k, stride, pad)
SAT_CASES = [
    ("a_all_qmax_zp0",         "pos", 0,   2, 64, 12, 96, 3, 1, 1),
    ("a_all_qmin_zp255",       "neg", 255, 2, 64, 12, 96, 3, 1, 1),
    ("a_alternating_zp128",    "alt", 128, 2, 64, 12, 96, 3, 1, 1),
    ("a_nonpos_zp255_s2_pad1", "nonpos", 255, 2, 48, 13, 64, 3, 2, 1),
    ("a_zp0_s2_pad1",          "pos", 0,   1, 32, 11, 160, 3, 2, 1),
]


def _sat_input(kind, B, Cin, H, g):
    x = torch.randn(B, Cin, H, H, generator=g)
    if kind == "pos":
        return x.abs() + 50.0
    if kind == "neg":
        return -x.abs() - 50.0
    if kind == "nonpos":
        return -x.abs()
    s = torch.ones(B, Cin, H, H)
    s.view(-1)[1::2] = -1.0
    return s * (x.abs() + 50.0)


@pytest.mark.parametrize("w_bits", [4, 8])
@pytest.mark.parametrize("wzp", ["ends", "mid"], ids=["wzp_ends", "wzp_mid"])
@pytest.mark.parametrize("case", SAT_CASES, ids=[c[0] for c in SAT_CASES])
def test_conv_saturated_operands(cuda, case, wzp, w_bits):
    """Activation codes all at qmin / qmax / alternating, int4 codes at 0 / 15 and int8 at 0 / 255 around zero points at the
    grid ends: int32 accumulators equal the integer oracle (padding holds the zero point's code); the fp32 rows of the four
    launch variants (K-groups on / off x split-K allowed / forbidden) are bit-identical and match the fake-quant reference."""
    from qdiff import engine, hip
    _, kind, zx, B, Cin, H, Cout, k, stride, pad = case
    g = torch.Generator().manual_seed(sum(map(ord, case[0])) + w_bits)
    x = _sat_input(kind, B, Cin, H, g)
    w, q = _sat_weights(Cout, Cin, k, w_bits, wzp, g)
    bias = torch.randn(Cout, generator=g)
    aq = _aq(0.02, zx)
    wc = _codes(w, q)
    nl = 2 ** w_bits
    assert bool((wc == 0).any()) and bool((wc == nl - 1).any())
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], k, k, stride, pad, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * H, (Cin * H * H, H * H, 1))
    Ho, Wo = engine.conv_out_hw(H, H, plan)
    assert _splitk_chosen(plan, xq, B, H, Ho)
    acc = torch.zeros((B * Ho * Wo, Cout), dtype=torch.int32, device=cuda)
    engine.conv_forward(plan, xq, B, H, H, acc_out=acc)
    outs = []
    try:
        for kg in (1, 0):
            hip.conv_config(kg)
            for sk in (None, False):
                outs.append(engine.conv_forward(plan, xq, B, H, H, out_dtype=torch.float32, splitk=sk).clone())
    finally:
        hip.conv_config(1)
    torch.cuda.synchronize()
    xc = R.uaq_codes(x, aq.delta, zx, 8, False)
    want = R.int_conv_exact(xc, zx, wc, q.zero_point.reshape(-1).long(), "conv2d", dict(stride=stride, padding=pad))
    got = acc.cpu().view(B, Ho, Wo, Cout).permute(0, 3, 1, 2).long()
    assert torch.equal(got, want), f"max |diff| = {(got - want).abs().max().item()}"
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o, outs[0]), f"launch variant {i} differs from variant 0"
    ref = R.quant_module_forward(x, w, bias, "conv2d", dict(stride=stride, padding=pad),
                                 [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=nl)],
                                 [dict(delta=aq.delta, zero_point=zx, n_bits=8, sym=False)])
    o = outs[0].cpu().view(B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    assert (o - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("w_bits", [4, 8])
def test_conv_longest_k_at_saturation(cuda, w_bits):
    """K = taps * Cin = 9 * 3632 = 32688, the longest run() accepts (taps * clen < 32768), with every activation code at 255
    (zero point 0): |Asum| = 255 * 32688 is the largest the 24-bit zero-point multiply is documented for.  Accumulators equal
    the integer oracle and the four launch variants agree bit for bit."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(3632 + w_bits)
    B, Cin, H, Cout, k = 1, 3632, 4, 64, 3
    x = torch.randn(B, Cin, H, H, generator=g).abs() + 50.0
    w, q = _sat_weights(Cout, Cin, k, w_bits, "ends", g)
    aq = _aq(0.02, 0)
    pack = engine.pack_module_weights(w.to(cuda), [q], 0)
    plan = engine.build_conv_plan(pack, [aq], k, k, 1, 1, None)
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * H, (Cin * H * H, H * H, 1))
    assert _splitk_chosen(plan, xq, B, H, H)
    acc = torch.zeros((B * H * H, Cout), dtype=torch.int32, device=cuda)
    engine.conv_forward(plan, xq, B, H, H, acc_out=acc)
    outs = []
    try:
        for kg in (1, 0):
            hip.conv_config(kg)
            for sk in (None, False):
                outs.append(engine.conv_forward(plan, xq, B, H, H, out_dtype=torch.float32, splitk=sk).clone())
    finally:
        hip.conv_config(1)
    torch.cuda.synchronize()
    want = R.int_conv_exact(R.uaq_codes(x, aq.delta, 0, 8, False), 0, _codes(w, q), q.zero_point.reshape(-1).long(), "conv2d",
                            dict(stride=1, padding=1))
    got = acc.cpu().view(B, H, H, Cout).permute(0, 3, 1, 2).long()
    assert torch.equal(got, want), f"max |diff| = {(got - want).abs().max().item()}"
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_conv_k_one_step_past_the_bound_is_refused(cuda):
    """K = 9 * 3648 = 32832 >= 32768: qd_conv2d_i8 refuses with HipEngineError before launching (the output is untouched)."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(3648)
    B, Cin, H, Cout, k = 1, 3648, 4, 64, 3
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    q = _weight_quantizer(w, 4, True, g)
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(0.02, 128)], k, k, 1, 1, None)
    xq = engine.quantize_rows(x.to(cuda), plan, B, Cin, H * H, (Cin * H * H, H * H, 1))
    out = torch.full((B * H * H, Cout), 7.0, device=cuda)
    with pytest.raises(hip.HipEngineError, match="K too long"):
        engine.conv_forward(plan, xq, B, H, H, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------
# (e) grouped launch contract
# ------------------------------------------------------------------------------------------------
def _linear_member(cuda, g, M, K, N):
    from qdiff import engine, hip
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(d, z)],
                                  1, 1, 1, 0, (torch.randn(N, generator=g) * 0.1).to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    out = torch.randn(M, N, generator=g).to(cuda)

    def call(o):                            # in place: the residual IS the output
        return hip.ConvCall(x=xq, w=plan.pack.wq, out=o, bias=plan.bias, residual=o, ldx=plan.ldx, ldk=plan.pack.ldk,
                            ldo=o.stride(0), ldr=o.stride(0), B=1, H=1, W=M, Ho=1, Wo=M, Cout=N, kh=1, kw=1, stride=1,
                            pad_t=0, pad_l=0, wbits=4, w_tiled=True, segs=plan.segs)
    return plan, xq, out, call


def _heads_member(cuda, g, M, K, N):
    from qdiff import engine, hip
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(d, z)],
                                  1, 1, 1, 0, None)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    qp = hip.make_qparams(torch.tensor(0.05, device=cuda), torch.tensor(255.0, device=cuda))   # zero point at the grid end
    out = torch.zeros((M, N), dtype=torch.int8, device=cuda)

    def call(o):
        return hip.ConvCall(x=xq, w=plan.pack.wq, out=o, bias=None, ldx=plan.ldx, ldk=plan.pack.ldk, ldo=0, B=1, H=1, W=M, Ho=1,
                            Wo=M, Cout=N, kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=4, w_tiled=True, segs=plan.segs,
                            epilogue=hip.EPI_HEADS_I8, oq_params=qp, oq_grid=_grid(8, False),
                            heads=dict(H=1, d=N, T=M, Tpad=M, dpad=N, prescale=1.0, sum=None))
    return plan, xq, out, call


@pytest.mark.parametrize("members", ["linear2", "heads_linear", "heads2_linear"])
def test_grouped_launch_with_split_k_linear_members(cuda, members):
    """qd_conv2d_i8_group promises the bytes of its members launched one by one.  Linear members that choose split-K (a
    workspace set by hand in the descriptor), in place (residual == out), first in the group or after one or two head-layout
    members (the probe walks the members until one does not qualify): the group must not run anything of a member before
    the member's real launch."""
    from qdiff import hip
    g = torch.Generator().manual_seed(1790)
    M, K, N = 256, 640, 320
    kinds = {"linear2": ["lin", "lin"], "heads_linear": ["heads", "lin"], "heads2_linear": ["heads", "heads", "lin"]}[members]
    mems = [(_heads_member if kd == "heads" else _linear_member)(cuda, g, M, K, N) for kd in kinds]
    grouped = [m[2].clone() for m in mems]
    single = [m[2].clone() for m in mems]
    calls = [m[3](o) for m, o in zip(mems, grouped)]
    need = max(hip.splitk_ws_bytes(c) for c in calls)
    assert need > 0, "no member chooses split-K at this shape"
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    descs = []
    for c in calls:
        d = hip._conv_desc(c)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
        descs.append(d)
    arr = (ctypes.POINTER(hip.ConvDesc) * len(descs))(*[ctypes.pointer(d) for d in descs])
    hip._check(hip.load().qd_conv2d_i8_group(arr, len(descs), hip._stream()), "qd_conv2d_i8_group")
    for m, o in zip(mems, single):
        c = m[3](o)
        d = hip._conv_desc(c)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
        hip._check(hip.load().qd_conv2d_i8(ctypes.byref(d), hip._stream()), "qd_conv2d_i8")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(grouped, single)):
        assert torch.equal(a, b), f"member {i} ({kinds[i]}): grouped launch differs from the single launch"


# ------------------------------------------------------------------------------------------------
# (b) normalisation producers: clipped grids, degenerate and offset statistics, tie-aware vs fp64
# ------------------------------------------------------------------------------------------------
# Error model of the one-pass statistics (E[x^2] - mean^2 from fp32 partial sums of x and x^2, combined in double): the
# variance carries a relative error of order n_chunk * u * (1 + (mean / std)^2) (u = 2^-24), which reaches the output as
# half that relative error of rstd times |x - mean| * |gamma| * rstd.  The bound below is NOT a worst-case derivation: it is
# that model with the chunk factor set to 1 — an acceptance LIMIT chosen ~4x above what the kernels were measured to do —
# on top of the fp32 bound the suite has always used (1e-5 of the output range).  It is the stated limit of the one-pass
# statistics: 2.5e-4 of the range at a common offset of 64 standard deviations, i.e. a tie window w of
# 0.34 .. 0.57 of a code on these grids (measured on the MI355X: <= 6.1e-5 for GroupNorm, <= 0.03 of a code; 4e-6 at 16 std;
# 3e-7 at 4 std; the windows accepted 0 .. 142 codes per case).  At 16 std and below w stays under 0.05 of a code.
def _norm_tol(scale, offset_ratio):
    return (1e-5 + 2.0 ** -24 * offset_ratio ** 2) * max(1.0, scale)


def _narrow_grid(y64, lo_q=0.15, hi_q=0.85):
    """An 8-bit asymmetric grid over the central quantiles of y (MSE-style scales clip: here ~30 % of the outputs)."""
    flat = y64.flatten().float()
    lo, hi = float(torch.quantile(flat, lo_q)), float(torch.quantile(flat, hi_q))
    lo, hi = min(lo, 0.0), max(hi, 1e-3)
    delta = (hi - lo) / 255.0
    zp = float(min(max(round(-lo / delta), 0), 255))
    return float(torch.tensor(delta, dtype=torch.float32)), zp


# Launch forms of groupnorm_impl (csrc/norm_quant.hip), with the shape that reaches each: (S, ldx - C, yout, part_in).  C = 320,
# 32 groups; "16-byte rows" means ldx = C on a fresh allocation.
GN_APPLY = {
    # with yout: gn_apply_kernel<float> / gn_apply_kernel<__half> (vec = 1), own partials (gn_partial_kernel<float> /
    # gn_partial_h8_kernel), S = 64: eight full chunks of gn_rows(S) = 8
    "yout": (64, 0, True, False),
    # no yout, even S, 16-byte rows: gn_apply_rows_kernel<2> (fp32) / gn_apply_rows_h8_kernel<2> (fp16, ldx % 8 == 0);
    # S = 60 leaves a ragged 4-row last chunk
    "rows": (60, 0, False, False),
    # the same apply forms on statistics handed in: part_in with nchunk_in = 6 chunks of 10 rows and part_ld = C + 32
    "rows_part": (60, 0, False, True),
    # no yout but odd S: gn_apply_kernel (vec = 1)
    "odd_S": (61, 0, False, False),
    # ldx = C + 2 (ldx % 4 != 0): vec = 0 in gn_partial_kernel<float / __half> and gn_apply_kernel; S = 300 -> gn_rows(S) = 32,
    # ragged 12-row last chunk
    "ldx_odd": (300, 2, False, False),
}

U32 = 2.0 ** -24          # unit roundoff of fp32


def _gn_modulation(B, C, silu, g):
    """scale | shift rows of a use_scale_shift_norm block with the value edges of the fold a' = a (1 + scale),
    sh' = sh (1 + scale) + shift: per channel (both samples) scale = -1 exactly (the output is shift), 1 + scale < 0,
    |scale| < 2^-24 (1 + scale rounds to 1), shift +-40 (large against the normalised range: saturates), and shift = +-3e38 /
    +-FLT_MAX / +-inf (with SiLU, -inf is left out: -inf * sigmoid(-inf) is NaN in the reference too).  Returns
    (mod [B][2C], channels whose shift is huge or infinite, channels with scale = -1)."""
    scale, shift = torch.randn(B, C, generator=g) * 0.7, torch.randn(B, C, generator=g) * 0.7
    minus1 = [3, 77, 150]
    scale[:, minus1] = -1.0
    scale[:, [13, 88]] = torch.tensor([-2.5, -1.75])
    scale[:, [23, 99]] = torch.tensor([1e-8, -3e-8])
    shift[:, [43, 53]] = torch.tensor([40.0, -40.0])
    huge = HUGE if not silu else [v for v in HUGE if v != float("-inf")]
    hch = list(range(200, 200 + len(huge)))
    shift[:, hch] = torch.tensor(huge)
    return torch.cat([scale, shift], 1), hch, minus1


@pytest.mark.parametrize("offset,silu,dtype,apply,mod",
                         params([("narrow_grid_const_group_sqrt_eps", 0), ("mean_4std", 4), ("mean_16std", 16), ("mean_64std", 64)],
                                [("silu", True), ("nosilu", False)], [("f32", "f32"), ("f16", "f16")],
                                [(None if k == "yout" else k, k) for k in GN_APPLY], [(None, False), ("mod", True)]))
def test_groupnorm_value_edges(cuda, offset, silu, dtype, apply, mod, record_property):
    """qd_groupnorm_silu_quant / qd_groupnorm_mod_silu_quant vs an fp64 GroupNorm (+ modulation) (+ SiLU) on a grid that clips
    ~30 % of the outputs, on every apply form of the dispatcher (GN_APPLY: the kernel instance and the condition that selects
    it).  offset 0 also holds a constant group (variance 0: the normalised value is exactly beta) and a group with std ~ sqrt(eps);
    offsets 4 / 16 / 64 put a common mean of that many standard deviations on every group.  (The kernel applies the folded affine
    x * a + (beta - mean * a): the constant group's output is beta to within one rounding of |mean * a|, so its constant is
    small, and its codes are checked with that rounding as the window.)  Plain: the fp32 output must lie within _norm_tol of the
    fp64 one; the codes are the quantisation of that fp32 value, so w = _norm_tol / delta (+ 1e-6 for the quotient's own
    rounding).  mod: _gn_modulation's edges, window from the fold's error model (below); channels with scale = -1 bit-exact
    without SiLU, huge / infinite shifts saturated."""
    from qdiff import hip
    S, ldpad, want_y, from_part = GN_APPLY[apply]
    g = torch.Generator().manual_seed(640 + offset + silu + (0 if apply == "yout" else 7 * list(GN_APPLY).index(apply)) + 1000 * mod)
    B, C, G, eps = 2, 320, 32, 1e-6
    x = torch.randn(B, C, S, generator=g) + float(offset)
    if offset == 0:
        x[0, :C // G] = 2.0 ** -8                                  # constant group: variance 0 (dyadic: exact sums)
        x[1, C // G:2 * C // G] = torch.randn(C // G, S, generator=g) * 1e-3    # std ~ sqrt(eps)
    if dtype == "f16":
        x = x.half().float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x64 = x.double().view(B, G, -1)
    mean, var = x64.mean(-1), x64.var(-1, unbiased=False)
    a64 = (gamma.double().view(1, G, C // G) / (var + eps).sqrt().unsqueeze(-1)).reshape(B, C, 1)
    sh64 = beta.double().view(1, C, 1) - mean.repeat_interleave(C // G, 1).unsqueeze(-1) * a64
    y0 = x.double() * a64 + sh64                                    # the fp64 GroupNorm, [B][C][S]
    keep = torch.ones(C, dtype=torch.bool)
    if mod:
        m, hch, minus1 = _gn_modulation(B, C, silu, g)
        keep[hch] = False
        sc64, f64 = 1.0 + m[:, :C].double().unsqueeze(-1), m[:, C:].double().unsqueeze(-1)
        y = y0 * sc64 + f64
    else:
        y = y0
    y64 = y * torch.sigmoid(y) if silu else y
    delta, zp = _narrow_grid(y64[:, keep])
    rows = x.permute(0, 2, 1).reshape(B * S, C)
    rows = device_rows(rows, C + ldpad, 0, torch.float16 if dtype == "f16" else torch.float32, cuda)
    part = None
    if from_part:
        r = rows.double().view(B, 6, S // 6, C)
        part = torch.zeros((B, 6, C + 32, 2), dtype=torch.float32, device=cuda)[:, :, :C]
        part.copy_(torch.stack([r.sum(2), (r * r).sum(2)], dim=-1).float())
        assert hip.part_ld(part) == C + 32
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    yo = torch.empty((B * S, C), dtype=torch.float32, device=cuda) if want_y else None
    hip.groupnorm_silu_quant(rows, B, S, C, rows.stride(0), G, eps, gamma.to(cuda), beta.to(cuda), silu,
                             torch.tensor([delta, zp], device=cuda), _grid(8, False), out, C, ws, yout=yo, ldy=C, part=part,
                             mod=m.to(cuda) if mod else None)
    torch.cuda.synchronize()
    T = lambda t: t.permute(0, 2, 1).reshape(B * S, -1)          # noqa: E731  [B][C][S] -> rows
    yref = T(y64)
    tol = _norm_tol(T(y0).abs().max().item(), offset)
    if mod:
        # Error model of the modulated fold: the plain path's y0 = x * a + sh is within tol of the fp64 one (as above); the
        # kernel then evaluates sc = 1 + scale, a' = a * sc, sh' = sh * sc + shift and y = x * a' + sh' in fp32 — six
        # roundings, each at most u times the value it rounds (u = 2^-24): 1 + s moves y by u |sc| (|x a| + |sh|), a * sc by
        # u |sc| |x a|, sh * sc by u |sc| |sh|, "+ shift" by u (|sc| |sh| + |shift|), x * a' by u |sc| |x a|, "+ sh'" by
        # u (|sc| (|x a| + |sh|) + |shift|): in all u (4 |sc| |x a| + 4 |sc| |sh| + 2 |shift|) <= 4 u Tm to first order, with
        # Tm = |sc| (|x a| + |sh|) + |shift|.  So |y - y64| <= |sc| tol + 4 u Tm, and SiLU (slope <= 1.1, its own expf /
        # reciprocal / product: <= 8 u |y|) maps it to 1.1 (...) + 8 u |y|.
        Tm = sc64.abs() * ((x.double() * a64).abs() + sh64.abs()) + f64.abs()
        err = sc64.abs() * tol + 4 * U32 * Tm
        if silu:
            err = 1.1 * err + 8 * U32 * y.abs()
        err = T(err)
    else:
        err = torch.full_like(yref, tol)
    if want_y:
        e = (yo.cpu().double() - yref).abs()[:, keep]
        assert bool((e <= err[:, keep]).all()), f"max |y - y64| - bound = {(e - err[:, keep]).max().item():.3g}"
    u = yref / delta + zp
    clip = ((u[:, keep] < -0.5) | (u[:, keep] > 255.5)).double().mean().item()
    assert 0.1 <= clip <= 0.4, clip
    got = out.cpu().long() + 128
    name = f"groupnorm[{offset},{'silu' if silu else 'nosilu'},{dtype},{apply}{',mod' if mod else ''}]"
    tie_aware_check(name, got[:, keep], u[:, keep], 0, 255, err[:, keep] / delta + 1e-6, record_property)
    if mod:
        want_h = torch.tensor([255 if v > 0 else (int(zp) if silu else 0) for v in m[0, C:][hch].tolist()])
        assert torch.equal(got[:, hch], want_h.expand(B * S, -1)), f"huge / infinite shifts: got {got[0, hch].tolist()}"
        if not silu:                    # scale = -1: a' = 0 and sh' = shift exactly, so the codes are those of shift
            want_m = R.uaq_codes(m[:, C:][:, minus1], torch.tensor(delta), zp, 8, False)
            assert torch.equal(got.view(B, S, C)[:, :, minus1], want_m.unsqueeze(1).expand(B, S, -1))
    if offset == 0 and not silu:
        # constant group: y = x * a + (beta - mean * a) with x == mean exactly, i.e. beta up to the rounding of the two fp32
        # operations on values of magnitude |beta| and |mean * a| (a = rstd * gamma): a window of 2^-23 of those, not _norm_tol;
        # modulated: times |sc|, plus the fold's own roundings (4 u Tm, as above)
        a = gamma[:C // G].double() / (eps ** 0.5)
        wc = (beta[:C // G].double().abs() + (2.0 ** -8) * a.abs()) * 2.0 ** -23
        if mod:
            wc = sc64[0, :C // G, 0].abs() * wc + 4 * U32 * Tm[0, :C // G].amax(-1)
        wc = float(wc.max()) / delta
        tie_aware_check("groupnorm[constant group]", got.view(B * S, C)[:S, :C // G], u.view(B * S, C)[:S, :C // G], 0, 255, wc,
                        record_property)


# (id, dtype, S, ldx - C, yout): the apply form that quantises the raw second output (the 1x1 skip connection's codes)
RAW_FORMS = [
    ("rows_f32", "f32", 60, 0, False),      # gn_apply_rows_kernel<2>: qd_pack4_t (QB bytes) on the raw values
    ("rows_h8_f16", "f16", 60, 0, False),   # gn_apply_rows_h8_kernel<2>
    ("apply_f32", "f32", 64, 0, True),      # gn_apply_kernel<float> (yout): qd_code_t per element
    ("apply_f16", "f16", 61, 0, False),     # gn_apply_kernel<__half> (odd S)
    ("apply_vec0_f32", "f32", 60, 2, False),   # gn_apply_kernel<float>, ldx % 4 != 0: vec = 0
]
# raw segments (c0, clen, oc0) of a [B*S][ldo] output (ldo): one segment, or the split shortcut's two; c0 / oc0 != 0, and
# the bytes outside [oc0, oc0 + clen) stay untouched
RAW_SEGS = {1: ([(32, 224, 48)], 288), 2: ([(16, 128, 32), (160, 112, 192)], 320)}


@pytest.mark.parametrize("nseg", [1, 2], ids=["one_seg", "two_segs"])
@pytest.mark.parametrize("qgrid", [(8, False), (8, True), (4, False)], ids=["u8", "s8", "u4"])
@pytest.mark.parametrize("form", RAW_FORMS, ids=[f[0] for f in RAW_FORMS])
def test_groupnorm_raw_output_value_edges(cuda, form, qgrid, nseg, record_property):
    """The raw second output of qd_groupnorm_silu_quant (qd_raw_quant: the un-normalised input quantised for the residual
    block's 1x1 skip connection, one quantiser per segment) on every apply form (RAW_FORMS).  Each segment has its own delta,
    small enough that ~30 % of its codes clip at both ends, and its own zero point (at or near the grid ends); its channels
    carry that grid's exact ties (k + 0.5) delta, clamp boundaries and their fp32 neighbours (edge_values), and one (sample,
    group) inside it carries +-3e38 ... +-inf.  Raw codes equal the oracle's codes of the same input bit for bit everywhere
    (no float work before that quantiser); raw bytes outside the segments are untouched; the normalised codes of every other
    (sample, group) are tie-aware against fp64 (w = _norm_tol / delta: nothing leaks from the non-finite groups)."""
    from qdiff import hip
    _, dtype, S, ldpad, want_y = form
    n_bits, sym = qgrid
    g = torch.Generator().manual_seed(4242 + S + ldpad + 10 * nseg + n_bits + 3 * sym)
    B, C, G, eps = 2, 320, 32, 1e-6
    cpg = C // G
    segs, ldo = RAW_SEGS[nseg]
    x = torch.randn(B, S, C, generator=g) * 1.3 + (0.0 if sym else 0.4)      # rows [b][s][c]
    half = dtype == "f16"
    if half:
        x = x.half().float()
    grid = _grid(n_bits, sym)
    qmin, qmax = R.code_range(n_bits, sym)
    bad = torch.zeros(B, G, dtype=torch.bool)
    seg_q = []
    for i, (c0, clen, _) in enumerate(segs):
        v = x[:, :, c0:c0 + clen].flatten()
        if sym:
            delta, zp = float(torch.quantile(v.abs(), 0.7)) / qmax, 0
        else:
            lo, hi = float(torch.quantile(v, 0.15)), float(torch.quantile(v, 0.85))
            delta = (hi - lo) / (qmax - qmin)
            zp = (qmin, qmax)[i] if nseg == 2 else int(round(-lo / delta))   # two segments: zero points at the grid ends
        delta = float(torch.tensor(delta, dtype=torch.float32))
        ev, _ = edge_values(delta, zp, qmin, qmax, 0, g, half=half)
        big = ~torch.isfinite(ev) | (ev.abs() > 1e3)
        # moderate edge values at random places of this segment (sample 0, and sample 1 outside the non-finite group)
        gi = (c0 + cpg - 1) // cpg + 1                                  # a group whose channels lie inside the segment
        assert c0 <= gi * cpg and (gi + 1) * cpg <= c0 + clen
        bad[1, gi] = True
        mod_v = ev[~big]
        for k in range(3):
            pos = torch.randperm(S * clen, generator=g)[:mod_v.numel()]
            b = k % 2
            sl = x[b, :, c0:c0 + clen].reshape(-1)
            if b == 1:                                                  # keep the non-finite group's slots for the huge values
                cc = pos % clen + c0
                pos = pos[(cc < gi * cpg) | (cc >= (gi + 1) * cpg)]
            sl[pos] = mod_v[:pos.numel()]
            x[b, :, c0:c0 + clen] = sl.view(S, clen)
        hv = ev[big]
        blk = x[1, :, gi * cpg:(gi + 1) * cpg].reshape(-1)
        blk[torch.randperm(blk.numel(), generator=g)[:hv.numel()]] = hv
        x[1, :, gi * cpg:(gi + 1) * cpg] = blk.view(S, cpg)
        seg_q.append((delta, zp))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xc = x.permute(0, 2, 1)                                             # [B][C][S]
    with torch.no_grad():
        y64 = F.group_norm(xc.double(), G, gamma.double(), beta.double(), eps)
        y64 = y64 * torch.sigmoid(y64)
    good = ~bad.repeat_interleave(cpg, 1)                               # [B][C]
    y_good = y64.permute(0, 2, 1)[good.unsqueeze(1).expand(B, S, C)]
    delta_n, zp_n = _narrow_grid(y_good)
    rows = device_rows(x.reshape(B * S, C), C + ldpad, 0, torch.float16 if half else torch.float32, cuda)
    rawd = dict(out=torch.full((B * S, ldo), 77, dtype=torch.int8, device=cuda),
                segs=[dict(c0=c0, clen=clen, oc0=oc0, qparams=torch.tensor([d, float(z)], device=cuda), grid=grid)
                      for (c0, clen, oc0), (d, z) in zip(segs, seg_q)])
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    yo = torch.empty((B * S, C), dtype=torch.float32, device=cuda) if want_y else None
    hip.groupnorm_silu_quant(rows, B, S, C, rows.stride(0), G, eps, gamma.to(cuda), beta.to(cuda), True,
                             torch.tensor([delta_n, zp_n], device=cuda), _grid(8, False), out, C, ws, yout=yo, ldy=C, raw=rawd)
    torch.cuda.synchronize()
    raw = rawd["out"].cpu()
    xr = x.reshape(B * S, C)
    touched = torch.zeros(ldo, dtype=torch.bool)
    for (c0, clen, oc0), (d, z) in zip(segs, seg_q):
        want = R.uaq_codes(xr[:, c0:c0 + clen], torch.tensor(d), z, n_bits, sym)
        got = raw[:, oc0:oc0 + clen].long() + grid.off
        assert torch.equal(got, want), (f"raw segment c0={c0}: {int((got != want).sum())} codes differ; inputs "
                                        f"{xr[:, c0:c0 + clen][got != want][:6].tolist()} got {got[got != want][:6].tolist()} "
                                        f"want {want[got != want][:6].tolist()}")
        fin = torch.isfinite(xr[:, c0:c0 + clen])
        lo_share, hi_share = [((want == e) & fin).double().mean().item() for e in (qmin, qmax)]
        assert lo_share + hi_share >= 0.2 and min(lo_share, hi_share) > 0.0, (lo_share, hi_share)
        touched[oc0:oc0 + clen] = True
    assert bool((raw[:, ~touched] == 77).all()), "raw bytes outside the segments were written"
    u = y64.permute(0, 2, 1).reshape(B * S, C) / delta_n + zp_n
    gm = good.unsqueeze(1).expand(B, S, C).reshape(B * S, C)
    tol = _norm_tol(y_good.abs().max().item(), 0)
    tie_aware_check(f"groupnorm_raw[{form[0]},{n_bits}{'s' if sym else 'u'},{nseg}]", (out.cpu().long() + 128)[gm], u[gm], 0, 255,
                    tol / delta_n + 1e-6, record_property)


# Launch forms of qd_layernorm_quant (csrc/norm_quant.hip): (id, C, dtype, ldx - C, element offset of the first row).  vec is
# "x 16- (fp32) / 8-byte (fp16) aligned and ldx % 4 == 0".
LN_FORMS = [
    ("rows8_f32", 320, "f32", 0, 0),        # C == 320 and vec: ln_quant_rows8_kernel<float, 10>
    ("rows8_f16", 320, "f16", 0, 0),        # ln_quant_rows8_kernel<__half, 10>
    ("c320_vec0_f32", 320, "f32", 1, 0),    # C == 320, ldx % 4 != 0: ln_quant_kernel<float, 2> with vec = 0
    ("nv3_f32", 640, "f32", 0, 0),          # ln_quant_kernel<float, 3> (2 rows per wave)
    ("nv5_f32", 1280, "f32", 0, 0),         # ln_quant_kernel<float, 5> (1 row per wave)
    ("nv6_f32", 1536, "f32", 0, 0),         # ln_quant_kernel<float, LN_MAXV = 6>
    ("h8_nv1", 512, "f16", 0, 0),           # fp16, 16-byte aligned rows, ldx % 8 == 0: ln_quant_h8_kernel<1, 2>
    ("h8_nv2", 640, "f16", 0, 0),           # ln_quant_h8_kernel<2, 2>
    ("h8_nv3", 1280, "f16", 0, 0),          # ln_quant_h8_kernel<3, 1>
    ("f16_ldx4", 640, "f16", 4, 0),         # ldx % 8 == 4: ln_quant_kernel<__half, 3> with vec = 1
    ("f16_unaligned", 1280, "f16", 8, 1),   # rows 2 bytes past 16-byte alignment: ln_quant_kernel<__half, 5> with vec = 0
]
_LN_DEFAULT = LN_FORMS[0]


def _ln_rows(cuda, form, x):
    """x [M][C] fp32 -> (x rounded to the form's dtype, device rows in the form's layout)."""
    _, C, dtype, ldpad, shift = form
    if dtype == "f16":
        x = x.half().float()                # the fp64 reference takes the fp16-rounded input
    rows = device_rows(x, C + ldpad, shift, torch.float16 if dtype == "f16" else torch.float32, cuda)
    return x, rows


@pytest.mark.parametrize("offset,form,M", params([("narrow_grid", 0), ("mean_16std", 16), ("mean_64std", 64)],
                                                [(None if f is _LN_DEFAULT else f[0], f) for f in LN_FORMS],
                                                [(None, 70), ("M1", 1)]))
def test_layernorm_value_edges(cuda, offset, form, M, record_property):
    """qd_layernorm_quant on every launch form (LN_FORMS: the kernel instance and the condition that selects it), M = 70 and 1
    (not a multiple of the rows per block), vs an fp64 LayerNorm, tie-aware with the error model of test_groupnorm_value_edges
    (the kernel writes no float output: w = _norm_tol / delta).  One launch with three consumers, zero points 0 / 128 / 255 —
    or the central-quantile one — of one delta; a second launch with two consumers, a symmetric grid (delta 1/127 of the 70 %
    quantile of |y|: ~30 % clip) and the central-quantile grid."""
    from qdiff import hip
    C = form[1]
    g = torch.Generator().manual_seed(320 + offset + (0 if form is _LN_DEFAULT else 13 * LN_FORMS.index(form)) + (M != 70))
    x = torch.randn(M, C, generator=g) * 1.7 + 1.7 * offset
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x, rows = _ln_rows(cuda, form, x)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    delta, zp = _narrow_grid(y64)
    zps = [zp, 0.0, 255.0] if form is _LN_DEFAULT and M == 70 else [0.0, 128.0, 255.0]
    outs = [torch.empty((M, C), dtype=torch.int8, device=cuda) for _ in range(5)]
    dsym = float(torch.tensor(float(torch.quantile(y64.abs().flatten().float(), 0.7)) / 127.0, dtype=torch.float32))
    hip.layernorm_quant(rows, M, C, rows.stride(0), 1e-5, gamma.to(cuda), beta.to(cuda),
                        [torch.tensor([delta, z], device=cuda) for z in zps], [_grid(8, False)] * 3, outs[:3], C)
    hip.layernorm_quant(rows, M, C, rows.stride(0), 1e-5, gamma.to(cuda), beta.to(cuda),
                        [torch.tensor([dsym, 0.0], device=cuda), torch.tensor([delta, zp], device=cuda)],
                        [_grid(8, True), _grid(8, False)], outs[3:], C)
    torch.cuda.synchronize()
    tol = _norm_tol(y64.abs().max().item(), offset)
    for o, z in zip(outs[:3] + outs[4:], zps + [zp]):
        tie_aware_check(f"layernorm[{offset},{form[0]},M{M},zp{int(z)}]", o.cpu().long() + 128, y64 / delta + z, 0, 255,
                        tol / delta + 1e-6, record_property)
    us = y64 / dsym
    clip = ((us < -128.5) | (us > 127.5)).double().mean().item()
    assert 0.15 <= clip <= 0.45 or M == 1, clip
    tie_aware_check(f"layernorm[{offset},{form[0]},M{M},sym]", outs[3].cpu().long(), us, -128, 127, tol / dsym + 1e-6,
                    record_property)


@pytest.mark.parametrize("offset", [0, 16, 64], ids=["bias0", "bias_16std", "bias_64std"])
def test_conv_groupnorm_statistics_at_offsets(cuda, offset, record_property):
    """GroupNorm fed with the statistics the convolution epilogue emits (gn_part) when every output channel carries a common
    offset (the bias) of that many standard deviations: codes vs the fp64 GroupNorm of the conv's own fp32 output, tie-aware
    with w = _norm_tol / delta."""
    from qdiff import engine
    g = torch.Generator().manual_seed(51 + offset)
    B, C, H, Cout, k = 2, 64, 16, 320, 3
    x = F.silu(torch.randn(B, C, H, H, generator=g))
    w = torch.randn(Cout, C, k, k, generator=g) * 0.05
    q = _weight_quantizer(w, 4, True, g)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0), [_aq(d, z)], k, k, 1, 1, None)
    xq = engine.quantize_rows(x.to(cuda), plan, B, C, H * H, (C * H * H, H * H, 1))
    ref = engine.conv_forward(plan, xq, B, H, H, out_dtype=torch.float32, splitk=False)
    std = ref.std().item()
    plan.bias = torch.full((Cout,), offset * std, device=cuda)
    out = engine.conv_forward(plan, xq, B, H, H, out_dtype=torch.float32, gn_stats=True, splitk=False)
    assert hasattr(out, "qd_gn_part")
    gn = torch.nn.GroupNorm(32, Cout, eps=1e-6).to(cuda)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(Cout, generator=g))
        gn.bias.copy_(torch.randn(Cout, generator=g))
    h64 = out.cpu().double().view(B, H * H, Cout).permute(0, 2, 1)
    y64 = F.group_norm(h64, 32, gn.weight.detach().cpu().double(), gn.bias.detach().cpu().double(), 1e-6)
    y64 = y64 * torch.sigmoid(y64)
    dy, zy = _narrow_grid(y64)
    w2 = torch.randn(32, Cout, 1, 1, generator=g) * 0.05
    plan2 = engine.build_conv_plan(engine.pack_module_weights(w2.to(cuda), [_weight_quantizer(w2, 4, True, g)], 0),
                                   [_aq(dy, zy)], 1, 1, 1, 0, None)
    codes, _ = engine.groupnorm_silu_quant(out, B, H * H, Cout, gn, True, plan=plan2, part=out.qd_gn_part)
    torch.cuda.synchronize()
    u = y64.permute(0, 2, 1).reshape(B * H * H, Cout) / dy + zy
    tol = _norm_tol(y64.abs().max().item(), offset)
    tie_aware_check(f"conv_gn_part[{offset}]", codes.cpu()[:, :Cout].long() + 128, u, 0, 255, tol / dy + 1e-6, record_property)


# ------------------------------------------------------------------------------------------------
# first-stage GroupNorm (qd_groupnorm_silu_h16: fp32 rows -> bf16 / fp16 rows, no quantiser)
# ------------------------------------------------------------------------------------------------
# (B, H, C, statistics from qd_conv2d_bf16's gn_part): the finalise pass each reaches (wide when nchunk * C / 32 >= 2048)
FS_STATS = {
    "narrow_own": (2, 16, 128, False),      # own partials: nchunk = 256 / gn_rows(256) = 32, 4 channels per group -> gn_finalize_kernel<64>
    "narrow_conv_part": (2, 16, 128, True),  # the conv's 128-row partials: nchunk = 2 -> gn_finalize_kernel<64>
    "wide_own": (1, 64, 512, False),        # 64x64 map, 512 channels: nchunk = 4096 / 32 = 128, x 16 -> gn_finalize_kernel<256>
    "wide_conv_part": (1, 128, 512, True),   # 128x128 map: the conv's nchunk = 128, x 16 -> gn_finalize_kernel<256>
}


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", ["silu_affine", "nosilu_null_affine"])
@pytest.mark.parametrize("stats", list(FS_STATS))
@pytest.mark.parametrize("offset", [0, 4, 16, 64], ids=["const_group_sqrt_eps", "mean_4std", "mean_16std", "mean_64std"])
def test_first_stage_groupnorm_value_edges(cuda, offset, stats, act, out_dtype):
    """qd_groupnorm_silu_h16 on the fp32 output of a bf16 qd_conv2d_bf16 (3x3, 8 input channels) whose bias puts a common
    offset of 0 / 4 / 16 / 64 output standard deviations on every channel; offset 0 also makes group 0 constant (zero
    weights, equal biases: variance 0) and group 1's std ~ sqrt(eps) (weights scaled by 1e-3).  Statistics from the kernel's
    own partials or from the conv epilogue's gn_part, through the narrow or the wide finalise (FS_STATS); SiLU with gamma /
    beta, or neither (null gamma / beta).  There is no quantiser: the float form of the tie rule is that every output lies in
    [RN(y64 - tol), RN(y64 + tol)], RN rounding fp64 -> fp32 -> the output type (monotone, and what the kernel's fp32 value
    within tol of y64, rounded once to nearest even, gives), tol = _norm_tol of the fp64 output's range at that offset."""
    from qdiff import hip
    B, Hh, C, from_part = FS_STATS[stats]
    silu = act == "silu_affine"
    G, eps, Cin = 32, 1e-6, 8
    cpg = C // G
    g = torch.Generator().manual_seed(777 + offset + C + Hh + from_part)
    x = torch.randn(B, Hh, Hh, Cin, generator=g).to(torch.bfloat16)
    w = torch.randn(C, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5
    bias = torch.full((C,), float(offset))
    if offset == 0:
        w[:cpg] = 0.0
        bias[:cpg] = 0.25
        w[cpg:2 * cpg] *= 1e-3
    S = Hh * Hh
    wt = hip.pack_weights_bf16(w.to(cuda), torch.bfloat16)
    o = torch.empty((B * S, C), dtype=torch.float32, device=cuda)
    part = torch.empty((B, S // 128, C, 2), dtype=torch.float32, device=cuda) if from_part else None
    hip.conv2d_bf16(x.reshape(-1, Cin).to(cuda), wt, bias.to(cuda), o, B, Hh, Hh, Cin, C, k=3, pad=1, gn_part=part)
    gamma, beta = (torch.randn(C, generator=g), torch.randn(C, generator=g)) if silu else (None, None)
    out = torch.full((B * S, C), float("nan"), dtype=out_dtype, device=cuda)
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    hip.groupnorm_silu_bf16(o, B, S, C, G, eps, None if gamma is None else gamma.to(cuda), None if beta is None else beta.to(cuda),
                            silu, out, ws, part=part)
    torch.cuda.synchronize()
    h64 = o.cpu().double().view(B, S, C).permute(0, 2, 1)
    y64 = F.group_norm(h64, G, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)
    if silu:
        y64 = y64 * torch.sigmoid(y64)
    y64 = y64.permute(0, 2, 1).reshape(B * S, C)
    tol = torch.full((C,), _norm_tol(y64.abs().max().item(), offset), dtype=torch.float64)
    if offset == 0:
        # constant group: x * a + (beta - mean * a) with x == mean == 0.25 exactly is beta up to two fp32 roundings of values of
        # magnitude |beta| and |mean * a| (a = gamma / sqrt(eps)), as in test_groupnorm_value_edges; SiLU's slope is <= 1.1
        gm = torch.ones(cpg, dtype=torch.float64) if gamma is None else gamma[:cpg].double()
        bt = torch.zeros(cpg, dtype=torch.float64) if beta is None else beta[:cpg].double()
        tol[:cpg] = torch.maximum(tol[:cpg], 1.1 * (bt.abs() + 0.25 * gm.abs() / eps ** 0.5) * 2.0 ** -23)
    lo, hi = (y64 - tol).float().to(out_dtype).double(), (y64 + tol).float().to(out_dtype).double()
    got = out.cpu().double()
    bad = ~((got >= lo) & (got <= hi))
    assert not bool(bad.any()), (f"{int(bad.sum())} of {got.numel()} outputs outside [RN(y64 - tol), RN(y64 + tol)] (tol {float(tol[-1]):.3g}): "
                                 f"got {got[bad][:4].tolist()} y64 {y64[bad][:4].tolist()}")
    if offset == 0:
        assert float(h64[:, :cpg].std()) == 0.0                       # the input group is constant (variance 0)
        if gamma is None:    # x * a + (0 - mean * a) with x == mean == 0.25: 0.25 * a is exact, so the output is exactly 0
            assert bool((got.view(B * S, C)[:, :cpg] == 0).all()), "the constant group's output is not exactly 0"


# ------------------------------------------------------------------------------------------------
# GEGLU -> codes (qd_geglu_quant: geglu_quant_kernel<float / __half>, qd_erff, qd_code_t)
# ------------------------------------------------------------------------------------------------
def _geglu_edge_inputs(M, Fd, delta, zp, half, g):
    """Values a and gates gt ([M*Fd] fp32, representable in fp16 when `half`): random pairs; gates around qd_erff's branch
    point |g / sqrt 2| = 0.9277 (g = +-1.312); deep negative gates -4 .. -12 (1 + erf cancels: y is a few ulps of erf near -1,
    or exactly 0); exact output ties (gate 8: erf(8 / sqrt 2) is 1 in fp32, gelu = 8 exactly, a = (k + 0.5) delta / 8);
    a = 0 with finite gates; and values / gates whose product is huge or infinite (saturation)."""
    n = M * Fd
    a = torch.randn(n, generator=g) * 1.5
    gt = torch.randn(n, generator=g) * 1.5
    gt[:2000] = torch.where(torch.rand(2000, generator=g) < 0.5, -1.0, 1.0) * (1.3120 + torch.randn(2000, generator=g) * 2e-3)
    gt[2000:3000] = -4.0 - 8.0 * torch.rand(1000, generator=g)
    a[2000:3000] *= 3.0
    ties, nt = edge_values(delta, zp, 0, 255, 0, g, half=half)
    ties = ties[:nt]
    a[3000:3000 + nt], gt[3000:3000 + nt] = ties / 8.0, 8.0
    a[3400:3600] = 0.0
    if half:
        hv = [(6e4, 6e4), (-6e4, 6e4), (6e4, -0.5), (float("inf"), 1.0), (float("-inf"), 1.0), (3e4, 3e4)]
    else:
        hv = [(3e38, 2.0), (-3e38, 2.0), (1e20, 1e20), (-1e20, 1e20), (3e38, -0.5), (float("inf"), 1.0), (float("-inf"), 1.0),
              (3.4028235e38, 3.0)]
    hv = torch.tensor(hv).repeat(8, 1)
    a[3600:3600 + hv.shape[0]], gt[3600:3600 + hv.shape[0]] = hv[:, 0], hv[:, 1]
    p = torch.randperm(n, generator=g)
    a, gt = a[p], gt[p]
    if half:
        a, gt = a.half().float(), gt.half().float()
    return a.view(M, Fd), gt.view(M, Fd), nt


def _geglu64(a, gt):
    return a.double() * (0.5 * gt.double() * (1.0 + torch.erf(gt.double() / 2.0 ** 0.5)))


def _geglu_window(a, gt, y64, delta):
    """Error model of y = a * (0.5 g (1 + qd_erff(g / sqrt 2))) in fp32: qd_erff is within 0.97 ulp of erf (< 2^-24 absolute
    on (-1, 1)) and the rounding of g / sqrt 2 moves erf by < 0.5 * 2^-24, the sum 1 + erf rounds once (2^-24 |1 + erf|): an
    absolute error E = 2^-23 + 2^-24 |1 + erf| on 1 + erf — the whole error in the cancellation of deep negative gates, where
    it scales with |a| |g| and not with |y| — times 0.5 |a| |g|; the two products round (2 * 2^-24 |y|).  Per element, in codes."""
    e = 2.0 ** -23 + 2.0 ** -24 * (1.0 + torch.erf(gt.double() / 2.0 ** 0.5)).abs()
    return (0.5 * a.double().abs() * gt.double().abs() * e + 2 * U32 * y64.abs()) / delta + 1e-6


@pytest.mark.parametrize("zp", ["central", 0, 255], ids=["zp_central", "zp0", "zp255"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_geglu_quant_value_edges(cuda, dtype, zp, record_property):
    """qd_geglu_quant (fp32 h: geglu_quant_kernel<float>; fp16 h: geglu_quant_kernel<__half>) on _geglu_edge_inputs, a grid
    that clips ~30 % of the outputs (delta from the central quantiles; zero point from them, or 0 / 255), tie-aware against
    the fp64 GEGLU with the per-element window of _geglu_window; huge / infinite products saturate, a = 0 gives the zero
    point's code exactly."""
    from qdiff import hip
    g = torch.Generator().manual_seed(5150 + (zp if zp != "central" else 7) + (dtype == "f16"))
    M, Fd = 64, 320
    half = dtype == "f16"
    a0 = torch.randn(4096, generator=g) * 1.5
    y0 = _geglu64(a0, torch.randn(4096, generator=g) * 1.5)
    delta, zc = _narrow_grid(y0)
    if half:            # delta = {2, 3} * 2^e: every tie (k + 0.5) delta of the grid, and a eighth of it, is an fp16 value
        m, e = math.frexp(delta)
        delta = math.ldexp(min(max(round(m * 4.0), 2), 3) / 4.0, e)
    zpv = zc if zp == "central" else float(zp)
    a, gt, nt = _geglu_edge_inputs(M, Fd, delta, zpv, half, g)
    assert nt >= 50, "no exact ties were constructed"
    h = torch.cat([a, gt], 1)
    hd = device_rows(h, 2 * Fd, 0, torch.float16 if half else torch.float32, cuda)
    out = torch.empty((M, Fd), dtype=torch.int8, device=cuda)
    hip.geglu_quant(hd, M, Fd, hd.stride(0), torch.tensor([delta, zpv], device=cuda), _grid(8, False), out, Fd)
    torch.cuda.synchronize()
    y64 = _geglu64(a, gt)
    got = out.cpu().long() + 128
    huge = ~torch.isfinite(y64) | (y64.abs() > 1e6)
    fin = ~huge
    assert int(huge.sum()) >= 30
    want_h = torch.where(y64[huge] > 0, 255, 0)
    assert torch.equal(got[huge], want_h), f"huge / infinite products: got {got[huge][:8].tolist()} want {want_h[:8].tolist()}"
    zero = a == 0
    assert bool((got[zero] == int(zpv)).all())
    # gate 8: gelu is exactly 8 in fp32 (erf(8 / sqrt 2) rounds to 1), so y = fp32(a * 8) = a * 8 and the code is exactly the
    # quantiser's — round half to even at the constructed ties, which the fp64 value (1e-15 below the tie) cannot decide
    g8 = gt == 8.0
    want8 = R.uaq_codes(a[g8] * 8.0, torch.tensor(delta), zpv, 8, False)
    assert torch.equal(got[g8], want8), f"gate-8 codes (exact ties): {int((got[g8] != want8).sum())} differ"
    # the code is round_half_even(y / delta) + zp, so the quotient is compared without the zero point
    u = y64[fin] / delta
    lo, hi = GEGLU_CLIP[zp]
    clip = ((u + zpv < -0.5) | (u + zpv > 255.5)).double().mean().item()
    assert lo <= clip <= hi, clip
    tie_aware_check(f"geglu[{dtype},zp{zp}]", got[fin] - int(zpv), u, -int(zpv), 255 - int(zpv),
                    _geglu_window(a[fin], gt[fin], y64[fin], delta), record_property)


# ------------------------------------------------------------------------------------------------
# int8-output GEMM epilogues (QD_EPI_GEGLU_I8, QD_EPI_HEADS_I8 with a residual, QD_EPI_HEADS_T_I8) at the value edges.
# Their contract: the bytes of the same layer's fp32 LINEAR-epilogue output sent through the standalone quantiser
# (qd_geglu_quant / qd_quantize_heads / the oracle's codes).
# ------------------------------------------------------------------------------------------------
def _linear_plan(cuda, w, q, aq, bias, row_perm=None):
    from qdiff import engine
    return engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0, row_perm=row_perm), [aq], 1, 1, 1, 0,
                                  None if bias is None else bias.to(cuda))


def _next_plan(cuda, Fd, delta, zp, g):
    """A consumer Linear of width Fd whose activation quantiser (delta, zp) the epilogue applies."""
    w2 = torch.randn(32, Fd, generator=g) * 0.05
    return _linear_plan(cuda, w2, _weight_quantizer(w2, 4, True, g), _aq(delta, zp), None)


def _fused_geglu_bytes(fused, xq, M, nxt):
    """engine.conv_forward_geglu under both K-group settings: asserted equal, returned once.  Each is one launch on the only
    form the GEGLU epilogue is built on: 128 x 128 blocks of four waves."""
    from conv_tall_tile_cases import launch_forms, one_form
    from qdiff import engine, hip
    outs = []
    try:
        for kg in (1, 0):
            hip.conv_config(kg)
            with launch_forms() as forms:
                outs.append(engine.conv_forward_geglu(fused, xq, M, nxt).clone())
            one_form(forms, 128, 128, 256)
    finally:
        hip.conv_config(1)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "K-groups on / off give different GEGLU bytes"
    return outs[0]


# clipped share of the finite outputs per zero point: the central grid clips ~30 %; a zero point at a grid end sends one
# whole sign of the (skewed: gelu's negative lobe is small) output distribution to that end as well
GEGLU_CLIP = {"central": (0.1, 0.4), 0: (0.3, 0.75), 255: (0.3, 0.75)}


@pytest.mark.parametrize("zp", ["central", 0, 255], ids=["zp_central", "zp0", "zp255"])
def test_geglu_epilogue_value_edges(cuda, zp, record_property):
    """QD_EPI_GEGLU_I8 (O_GEGLU: qd_bytes2_t, qd_erff2; engine.conv_forward_geglu) with gate biases at qd_erff's branch point
    (g = +-1.312, gate weights scaled down so the gates stay within ~0.02 of it), deep negative gates (-4 .. -12: the 1 + erf
    cancellation), value biases +-3e38 / +-inf (huge or infinite products saturate), on a grid clipping GEGLU_CLIP of the
    outputs.  Bytes == qd_geglu_quant of the same layer's fp32 LINEAR output (the documented contract) under both K-group
    settings, and tie-aware against the fp64 GEGLU of that output (_geglu_window)."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(6161 + (zp if zp != "central" else 7))
    M, K, Fd = 256, 320, 128
    x = torch.randn(M, K, generator=g)
    w = torch.randn(2 * Fd, K, generator=g) * 0.05
    bias = torch.randn(2 * Fd, generator=g) * 0.5
    w[Fd:Fd + 64] *= 0.01                                                 # gates of features 0..63 stay near their bias
    bias[Fd:Fd + 32] = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0) * 1.312
    bias[Fd + 32:Fd + 48] = -4.0 - 8.0 * torch.rand(16, generator=g)
    bias[48:56] = torch.tensor([3e38, -3e38, 3.4028235e38, -3.4028235e38, float("inf"), float("-inf"), 1e38, -1e38])
    bias[Fd + 48:Fd + 56] = 2.0
    q = _weight_quantizer(w, 4, True, g)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    plain = _linear_plan(cuda, w, q, _aq(dx, zx), bias)
    fused = _linear_plan(cuda, w, q, _aq(dx, zx), bias, row_perm=engine.geglu_row_perm(Fd, cuda))
    xq = engine.quantize_rows(x.to(cuda), plain, 1, K, M, (0, 1, K))
    h = engine.conv_forward(plain, xq, 1, 1, M, 1, M, splitk=False)
    hc = h.cpu()
    y64 = _geglu64(hc[:, :Fd], hc[:, Fd:])
    huge = ~torch.isfinite(y64) | (y64.abs() > 1e6)
    assert int(huge.sum()) == 8 * M
    delta, zc = _narrow_grid(y64[~huge])
    zpv = zc if zp == "central" else float(zp)
    nxt = _next_plan(cuda, Fd, delta, zpv, g)
    ref = torch.zeros((M, nxt.ldx), dtype=torch.int8, device=cuda)
    hip.geglu_quant(h, M, Fd, 2 * Fd, nxt.qparams[0], nxt.grids[0], ref, nxt.ldx)
    got8 = _fused_geglu_bytes(fused, xq, M, nxt)
    assert torch.equal(got8[:, :Fd], ref[:, :Fd]), f"{int((got8[:, :Fd] != ref[:, :Fd]).sum())} bytes differ from qd_geglu_quant"
    got = got8[:, :Fd].cpu().long() + 128
    assert torch.equal(got[huge], torch.where(y64[huge] > 0, 255, 0)), "huge / infinite products do not saturate"
    u = y64[~huge] / delta
    lo, hi = GEGLU_CLIP[zp]
    clip = ((u + zpv < -0.5) | (u + zpv > 255.5)).double().mean().item()
    assert lo <= clip <= hi, clip
    tie_aware_check(f"geglu_epilogue[zp{zp}]", got[~huge] - int(zpv), u, -int(zpv), 255 - int(zpv),
                    _geglu_window(hc[:, :Fd][~huge], hc[:, Fd:][~huge], y64[~huge], delta), record_property)


def _key_perm(T):
    """Transposed operand bytes: key slot p = half * 16 + r of a 32-key tile holds key (r & 3) + 8 (r >> 2) + 4 half (the
    attention kernel's operand order) — the key index stored at every slot."""
    p = torch.arange(T)
    r, half = p % 16, p % 32 // 16
    return p - p % 32 + (r & 3) + 8 * (r >> 2) + 4 * half


def _heads_call(plan, xq, out8, B, T, H, d, Tpad, dpad, prescale, qp, hsum=None, transpose=False):
    from qdiff import hip
    return hip.ConvCall(x=xq, w=plan.pack.wq, out=out8, bias=plan.bias, ldx=plan.ldx, ldk=plan.pack.ldk, ldo=0,
                        B=B, H=1, W=T, Ho=1, Wo=T, Cout=H * d, kh=1, kw=1, stride=1, pad_t=0, pad_l=0,
                        wbits=plan.pack.wbits, w_tiled=True, segs=plan.segs,
                        epilogue=hip.EPI_HEADS_T_I8 if transpose else hip.EPI_HEADS_I8, oq_params=qp, oq_grid=_grid(8, False),
                        heads=dict(H=H, d=d, T=T, Tpad=Tpad, dpad=dpad, prescale=prescale, sum=hsum))


@pytest.mark.parametrize("zp", [0, 255], ids=["out_zp0", "out_zp255"])
def test_heads_t_epilogue_value_edges(cuda, zp):
    """QD_EPI_HEADS_T_I8 (O_HTR: the V projection written as transposed, key-permuted attention operand bytes with their
    column sums hd_sum) with prescale = 40^-1/4 (an LDM-style q / k prescale, != 1), bias = +-3e38 ... +-inf on eight columns,
    a grid clipping ~30 % and output zero point 0 / 255; T = 128 tokens padded to Tpad = 160, d = 40 padded to 64.  Bytes ==
    qd_quantize_heads(transpose = 1, same prescale) of the layer's fp32 LINEAR output, which are the oracle's codes of
    fp32(y * prescale); hd_sum == the exact column sums of the stored bytes; pad bytes (t >= T, dd >= d) untouched; a grouped
    launch with a HEADS_I8 member gives the bytes and sums of the single launches."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(4040 + zp)
    B, T, H, d, K = 2, 128, 8, 40, 320
    M, N, Tpad, dpad = B * T, H * d, 160, 64
    pre = float(torch.tensor(40.0 ** -0.25, dtype=torch.float32))
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.1
    bias[5:5 + len(HUGE)] = torch.tensor(HUGE)
    d0, z0 = R.uaq_init_scale(x, 8, False, False, "max")
    plan = _linear_plan(cuda, w, _weight_quantizer(w, 4, True, g), _aq(d0, z0), bias)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    y = engine.conv_forward(plan, xq, 1, 1, M, out_dtype=torch.float32, splitk=False)
    ys = y.cpu() * torch.tensor(pre, dtype=torch.float32)
    fin = torch.ones(N, dtype=torch.bool)
    fin[5:5 + len(HUGE)] = False
    flat = ys[:, fin].flatten()
    lo, hi = float(torch.quantile(flat, 0.15)), float(torch.quantile(flat, 0.85))
    delta = float(torch.tensor((hi - lo) / 255.0, dtype=torch.float32))
    qp = _certified(cuda, delta, zp)
    ref8 = torch.full((B * H, dpad, Tpad), 77, dtype=torch.int8, device=cuda)
    rsum = torch.zeros((B * H, dpad), dtype=torch.int32, device=cuda)
    hip.quantize_heads(y, B, T, H, d, (T * N, N, d, 1), pre, qp, _grid(8, False), True, ref8, rsum, Tpad, dpad)
    res = {}
    for mode in ("single", "grouped"):
        v8 = torch.full((B * H, dpad, Tpad), 77, dtype=torch.int8, device=cuda)
        hs = torch.zeros((B * H, dpad), dtype=torch.int32, device=cuda)
        q8 = torch.full((B * H, Tpad, dpad), 77, dtype=torch.int8, device=cuda)
        calls = [_heads_call(plan, xq, q8, B, T, H, d, Tpad, dpad, pre, qp),
                 _heads_call(plan, xq, v8, B, T, H, d, Tpad, dpad, pre, qp, hsum=hs, transpose=True)]
        if mode == "single":
            for c in calls:
                hip.conv2d_i8(c)
        else:
            hip.conv2d_i8_group(calls)
        torch.cuda.synchronize()
        res[mode] = (q8.cpu(), v8.cpu(), hs.cpu())
    q8, v8, hs = res["single"]
    for a, b in zip(res["single"], res["grouped"]):
        assert torch.equal(a, b), "grouped launch differs from the single launches"
    want = R.uaq_codes(ys, torch.tensor(delta), zp, 8, False).view(B, T, H, d).permute(0, 2, 3, 1).reshape(B * H, d, T) - 128
    assert torch.equal(ref8.cpu()[:, :d, :T].long(), want[:, :, _key_perm(T)])
    got = v8[:, :d, :T].long()
    assert torch.equal(got, ref8.cpu()[:, :d, :T].long()), \
        f"{int((got != ref8.cpu()[:, :d, :T].long()).sum())} bytes differ from qd_quantize_heads(transpose=1)"
    # the 15 / 85 % quantile delta clips ~30 %; the zero point at a grid end clips one whole sign on top
    clip = ((want + 128 == 0) | (want + 128 == 255)).view(B, H * d, T)[:, fin].double().mean().item()
    assert 0.1 <= clip <= 0.75, clip
    assert torch.equal(hs[:, :d].long(), got.sum(-1)), "hd_sum is not the column sum of the stored bytes"
    assert bool((hs[:, d:] == 0).all())
    assert bool((v8[:, :, T:] == 77).all()) and bool((v8[:, d:, :] == 77).all()), "HEADS_T pad bytes were written"
    wq = want.view(B, H, d, T).permute(0, 1, 3, 2).reshape(B * H, T, d)
    assert torch.equal(q8[:, :T, :d].long(), wq) and bool((q8[:, T:, :] == 77).all()) and bool((q8[:, :, d:] == 77).all())


@pytest.mark.parametrize("res_dtype", [torch.float32, torch.float16], ids=["res_f32", "res_f16"])
@pytest.mark.parametrize("zp", [0, 255], ids=["out_zp0", "out_zp255"])
def test_heads_rows_residual_value_edges(cuda, zp, res_dtype):
    """QD_EPI_HEADS_I8 as "Linear + residual -> the next Linear's int8 rows" (engine.linear_to_rows_i8, O_HROWS with res_f16
    off / on) where the residual drives outputs to +-huge / +-inf (fp32: +-3e38, +-FLT_MAX, +-inf; fp16: +-65504, +-inf) on
    some rows of eight columns, on a grid clipping ~30 % with zero point 0 / 255: bytes == the oracle's codes of the same
    layer's fp32 LINEAR output with the residual (widened to fp32) added, saturated where the sum is huge or infinite."""
    from qdiff import engine
    g = torch.Generator().manual_seed(5252 + zp + (res_dtype == torch.float16))
    B, T, K, N = 2, 128, 320, 320
    M = B * T
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    d0, z0 = R.uaq_init_scale(x, 8, False, False, "max")
    plan = _linear_plan(cuda, w, _weight_quantizer(w, 4, True, g), _aq(d0, z0), torch.randn(N, generator=g) * 0.1)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    res = torch.randn(M, N, generator=g)
    big = [3e38, -3e38, 3.4028235e38, -3.4028235e38, float("inf"), float("-inf")] if res_dtype == torch.float32 else \
          [65504.0, -65504.0, float("inf"), float("-inf")]
    big = torch.tensor(big)
    rows = torch.arange(0, M, 3)
    for j, c in enumerate(range(7, 15)):
        res[rows, c] = big[j % len(big)]
    res = res.to(res_dtype)
    y = engine.conv_forward(plan, xq, 1, 1, M, residual=res.float().to(cuda), out_dtype=torch.float32, splitk=False).cpu()
    keep = torch.isfinite(y) & (y.abs() < 1e4)
    lo, hi = float(torch.quantile(y[keep], 0.15)), float(torch.quantile(y[keep], 0.85))
    delta = float(torch.tensor((hi - lo) / 255.0, dtype=torch.float32))
    nxt = _next_plan(cuda, N, delta, zp, g)
    got = engine.linear_to_rows_i8(plan, xq, B, T, nxt, residual=res.to(cuda))
    torch.cuda.synchronize()
    want = R.uaq_codes(y, torch.tensor(delta), zp, 8, False)
    got = got.cpu()[:, :N].long() + 128
    assert bool((~keep).sum() >= 8 * len(rows) // 2)
    assert torch.equal(got[~keep], torch.where(y[~keep] > 0, 255, 0)), "huge / infinite outputs do not saturate"
    clip = ((want[keep] == 0) | (want[keep] == 255)).double().mean().item()
    assert 0.1 <= clip <= 0.75, clip              # ~30 % from the quantile delta, plus one sign for a zero point at a grid end
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("act", [("qmax_zp0", 0), ("qmin_zp255", 255)], ids=["a_qmax_zp0", "a_qmin_zp255"])
@pytest.mark.parametrize("epi", ["geglu", "heads", "heads_t"])
def test_int8_epilogues_longest_k_at_saturation(cuda, epi, act):
    """1x1 layer with K = Cin = 32752, the longest run() accepts (taps * clen < 32768), every activation code at one grid end
    (255 with zero point 0, or 0 with zero point 255: Asum - kz of either sign) and int4 weight codes at 0 / 15 around zero points
    at the ends: the __mul24 zero-point term of the O_GEGLU / O_HROWS / O_HTR epilogues at its largest.  The accumulator is the
    one test_conv_longest_k_at_saturation proves exact; bytes == the codes of the same layer's fp32 LINEAR output
    (qd_geglu_quant / qd_quantize_heads of it; hd_sum == the column sums), under both K-group settings."""
    from qdiff import engine, hip
    kind, zx = act
    g = torch.Generator().manual_seed(32752 + zx + len(epi))
    M, K = 128, 32752
    Cout = 64
    x = torch.randn(M, K, generator=g).abs() + 50.0
    if zx == 255:
        x = -x
    w, q = _sat_weights(Cout, K, 1, 4, "ends", g)
    aq = _aq(0.02, zx)
    plain = _linear_plan(cuda, w, q, aq, None)
    xq = engine.quantize_rows(x.to(cuda), plain, 1, K, M, (0, 1, K))
    y = engine.conv_forward(plain, xq, 1, 1, M, out_dtype=torch.float32, splitk=False)
    yc = y.cpu()
    wc = _codes(w, q)
    assert bool((R.uaq_codes(x, aq.delta, zx, 8, False) == 255 - zx).all()) and bool((wc == 0).any()) and bool((wc == 15).any())
    if epi == "geglu":
        Fd = Cout // 2
        y64 = _geglu64(yc[:, :Fd], yc[:, Fd:])
        delta, zp = _narrow_grid(y64)
        nxt = _next_plan(cuda, Fd, delta, zp, g)
        ref = torch.zeros((M, nxt.ldx), dtype=torch.int8, device=cuda)
        hip.geglu_quant(y, M, Fd, Cout, nxt.qparams[0], nxt.grids[0], ref, nxt.ldx)
        fused = _linear_plan(cuda, w, q, aq, None, row_perm=engine.geglu_row_perm(Fd, cuda))
        got = _fused_geglu_bytes(fused, xq, M, nxt)
        assert torch.equal(got[:, :Fd], ref[:, :Fd]), f"{int((got[:, :Fd] != ref[:, :Fd]).sum())} bytes differ"
        return
    H, d = 2, 32
    delta, zp = _narrow_grid(yc)
    qp = _certified(cuda, delta, int(zp))
    tr = epi == "heads_t"
    ref8 = torch.zeros((H, d, M) if tr else (H, M, d), dtype=torch.int8, device=cuda)
    rsum = torch.zeros((H, d if tr else M), dtype=torch.int32, device=cuda)
    hip.quantize_heads(y, 1, M, H, d, (M * Cout, Cout, d, 1), 1.0, qp, _grid(8, False), tr, ref8, rsum if tr else None, M, d)
    outs = []
    try:
        for kg in (1, 0):
            hip.conv_config(kg)
            o = torch.zeros_like(ref8)
            hs = torch.zeros((H, d), dtype=torch.int32, device=cuda) if tr else None
            hip.conv2d_i8(_heads_call(plain, xq, o, 1, M, H, d, M, d, 1.0, qp, hsum=hs, transpose=tr))
            torch.cuda.synchronize()
            outs.append((o.cpu(), None if hs is None else hs.cpu()))
    finally:
        hip.conv_config(1)
    want = R.uaq_codes(yc, torch.tensor(delta), zp, 8, False) - 128
    want = want.view(M, H, d).permute(1, 2, 0)[:, :, _key_perm(M)] if tr else want.view(M, H, d).permute(1, 0, 2)
    assert torch.equal(ref8.cpu().long(), want)
    for o, hs in outs:
        assert torch.equal(o.long(), want), f"{int((o.long() != want).sum())} bytes differ"
        if tr:
            assert torch.equal(hs.long(), want.sum(-1))


# ------------------------------------------------------------------------------------------------
# packed quotient (qd_bytes2_t / qd_pack4_t: the normalisation byte stores and the GEMM epilogues) on huge and non-finite values
# ------------------------------------------------------------------------------------------------
HUGE = [3e38, -3e38, float("inf"), float("-inf"), 3.4028235e38, -3.4028235e38, 1e38, -1e38]


def _certified(cuda, delta, zp):
    from qdiff import hip
    qp = hip.make_qparams(torch.tensor(delta, device=cuda), torch.tensor(float(zp), device=cuda))
    assert qp.cpu()[3].item() != 0, f"delta {delta!r} is not certified: the case would not reach the fast quotient"
    return qp


@pytest.mark.parametrize("zp,form", params([("zp0", 0), ("zp128", 128), ("zp255", 255)],
                                           [(None if f is _LN_DEFAULT else f[0], f) for f in LN_FORMS]))
def test_layernorm_packed_quotient_huge_and_infinite(cuda, zp, form, record_property):
    """qd_layernorm_quant with beta = +-3e38 / +-FLT_MAX / +-1e38 / +-inf on eight channels, on every launch form (LN_FORMS):
    those outputs are that huge or infinite value and must saturate at qmax / qmin on the fast quotient (the packed form used
    to send every one of them to qmin: y = x * rinv overflowed and e = fma(-y, delta, x) was NaN); the other channels as in
    test_layernorm_value_edges."""
    from qdiff import hip
    C = form[1]
    g = torch.Generator().manual_seed(38 + zp + (0 if form is _LN_DEFAULT else 13 * LN_FORMS.index(form)))
    M = 70
    x = torch.randn(M, C, generator=g) * 1.7
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x, rows = _ln_rows(cuda, form, x)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    delta, _ = _narrow_grid(y64)
    beta[5:5 + len(HUGE)] = torch.tensor(HUGE)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    out = torch.empty((M, C), dtype=torch.int8, device=cuda)
    hip.layernorm_quant(rows, M, C, rows.stride(0), 1e-5, gamma.to(cuda), beta.to(cuda), [_certified(cuda, delta, zp)],
                        [_grid(8, False)], [out], C)
    torch.cuda.synchronize()
    got = out.cpu().long() + 128
    hs = slice(5, 5 + len(HUGE))
    want_h = torch.tensor([255 if v > 0 else 0 for v in HUGE]).expand(M, -1)
    assert torch.equal(got[:, hs], want_h), f"huge / infinite outputs: got {got[0, hs].tolist()} want {want_h[0].tolist()}"
    keep = torch.ones(C, dtype=torch.bool)
    keep[hs] = False
    tie_aware_check(f"layernorm_huge[zp{zp}]", got[:, keep], y64[:, keep] / delta + zp, 0, 255,
                    _norm_tol(y64[:, keep].abs().max().item(), 0) / delta + 1e-6, record_property)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_groupnorm_packed_quotient_huge_and_infinite(cuda, dtype):
    """qd_groupnorm_silu_quant (fp32 rows, and fp16 rows on the 16-byte-lane kernel) with beta = +-3e38 ... +-inf on eight
    channels: the folded shift is that value, the outputs are huge or infinite and must saturate on the fast quotient."""
    from qdiff import hip
    g = torch.Generator().manual_seed(39)
    B, C, S, G = 2, 320, 64, 32
    x = torch.randn(B, C, S, generator=g)
    if dtype == "f16":
        x = x.half().float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    delta, zp = _narrow_grid(F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-6))
    beta[5:5 + len(HUGE)] = torch.tensor(HUGE)
    y64 = F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-6)
    rows = x.permute(0, 2, 1).reshape(B * S, C).contiguous()
    rows = rows.half() if dtype == "f16" else rows
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    hip.groupnorm_silu_quant(rows.to(cuda), B, S, C, C, G, 1e-6, gamma.to(cuda), beta.to(cuda), False,
                             _certified(cuda, delta, zp), _grid(8, False), out, C, ws)
    torch.cuda.synchronize()
    got = out.cpu().long() + 128
    hs = slice(5, 5 + len(HUGE))
    want_h = torch.tensor([255 if v > 0 else 0 for v in HUGE]).expand(B * S, -1)
    assert torch.equal(got[:, hs], want_h), f"huge / infinite outputs: got {got[0, hs].tolist()} want {want_h[0].tolist()}"
    keep = torch.ones(C, dtype=torch.bool)
    keep[hs] = False
    yref = y64.permute(0, 2, 1).reshape(B * S, C)
    tie_aware_check(f"groupnorm_huge[{dtype}]", got[:, keep], yref[:, keep] / delta + zp, 0, 255,
                    _norm_tol(yref[:, keep].abs().max().item(), 0) / delta + 1e-6)


@pytest.mark.parametrize("zp", [0, 255], ids=["out_zp0", "out_zp255"])
def test_heads_epilogue_clipped_grid_huge_and_infinite(cuda, zp):
    """QD_EPI_HEADS_I8 (rows of the next layer's codes written by the GEMM epilogue) on a grid that clips ~30 % of the outputs,
    output zero point at either end, and bias = +-3e38 ... +-inf on eight channels: bytes equal the oracle's codes of the fp32
    linear output of the same layer (the epilogue's documented contract), huge / infinite outputs saturated."""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(767 + zp)
    M, K, N = 256, 320, 320
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.1
    bias[5:5 + len(HUGE)] = torch.tensor(HUGE)
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(d, z)],
                                  1, 1, 1, 0, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, M, (0, 1, K))
    y = engine.conv_forward(plan, xq, 1, 1, M, out_dtype=torch.float32, splitk=False).cpu()
    finite = torch.ones(N, dtype=torch.bool)
    finite[5:5 + len(HUGE)] = False
    flat = y[:, finite].flatten()
    lo, hi = float(torch.quantile(flat, 0.15)), float(torch.quantile(flat, 0.85))
    delta = float(torch.tensor((hi - lo) / 255.0, dtype=torch.float32))
    qp = _certified(cuda, delta, zp)
    out8 = torch.zeros((M, N), dtype=torch.int8, device=cuda)
    call = hip.ConvCall(x=xq, w=plan.pack.wq, out=out8, bias=plan.bias, ldx=plan.ldx, ldk=plan.pack.ldk, ldo=0,
                        B=1, H=1, W=M, Ho=1, Wo=M, Cout=N, kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=4, w_tiled=True,
                        segs=plan.segs, epilogue=hip.EPI_HEADS_I8, oq_params=qp, oq_grid=_grid(8, False),
                        heads=dict(H=1, d=N, T=M, Tpad=M, dpad=N, prescale=1.0, sum=None))
    hip.conv2d_i8(call)
    torch.cuda.synchronize()
    want = R.uaq_codes(y, torch.tensor(delta), zp, 8, False)
    got = out8.cpu().long() + 128
    clip = ((want[:, finite] == 0) | (want[:, finite] == 255)).double().mean().item()
    assert clip >= 0.1, clip
    assert torch.equal(got[:, ~finite], want[:, ~finite]), f"huge / infinite outputs: got {got[0, ~finite].tolist()}"
    assert torch.equal(got, want), f"{int((got != want).sum())} codes differ"
