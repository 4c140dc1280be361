"""GPU tests at the VALUE edges of the integer kernels (the shape edges are tests/test_hip_kernels.py and
tests/test_random_shapes_gpu.py): exact rounding ties, clamp boundaries, +-inf and huge finite inputs, zero points at the grid
ends, grids that clip a large share of their inputs, saturated contraction operands, degenerate and offset normalisation
statistics, and the grouped-launch contract.

Every reference is the oracle (oracle/quant_ref.py) or an fp64 evaluation of the reference formula.  Pure quantisers are
compared bit for bit; producers with float work before the quantiser through tests/edge_util.tie_aware_check (rule and
derivation of its window w in that module and at each use).  Run with -s to see the accepted tie-window mismatches.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from edge_util import edge_values, f32_from_bits, tie_aware_check
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


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "nosilu"])
@pytest.mark.parametrize("offset", [0, 4, 16, 64], ids=["narrow_grid_const_group_sqrt_eps", "mean_4std", "mean_16std", "mean_64std"])
def test_groupnorm_value_edges(cuda, offset, silu, dtype, record_property):
    """qd_groupnorm_silu_quant vs an fp64 GroupNorm (+ SiLU) on a grid that clips ~30 % of the outputs.  offset 0 also holds a
    constant group (variance 0: the normalised value is exactly beta) and a group with std ~ sqrt(eps); offsets 4 / 16 / 64 put a
    common mean of that many standard deviations on every group.  (The kernel applies the folded affine x * a + (beta - mean * a):
    the constant group's output is beta to within one rounding of |mean * a|, so its constant is small, and its codes are checked
    with that rounding as the window.)  The fp32 output must lie within _norm_tol of the fp64 one;
    the codes are the quantisation of that fp32 value, so w = _norm_tol / delta (+ 1e-6 for the quotient's own rounding)."""
    from qdiff import hip
    g = torch.Generator().manual_seed(640 + offset + silu)
    B, C, S, G, eps = 2, 320, 64, 32, 1e-6
    x = torch.randn(B, C, S, generator=g) + float(offset)
    if offset == 0:
        x[0, :C // G] = 2.0 ** -8                                  # constant group: variance 0 (dyadic: exact sums)
        x[1, C // G:2 * C // G] = torch.randn(C // G, S, generator=g) * 1e-3    # std ~ sqrt(eps)
    if dtype == "f16":
        x = x.half().float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y64 = F.group_norm(x.double(), G, gamma.double(), beta.double(), eps)
    y64 = y64 * torch.sigmoid(y64) if silu else y64
    delta, zp = _narrow_grid(y64)
    rows = x.permute(0, 2, 1).reshape(B * S, C).contiguous()
    rows = rows.half() if dtype == "f16" else rows
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=cuda)
    out = torch.empty((B * S, C), dtype=torch.int8, device=cuda)
    yo = torch.empty((B * S, C), dtype=torch.float32, device=cuda)
    hip.groupnorm_silu_quant(rows.to(cuda), B, S, C, C, G, eps, gamma.to(cuda), beta.to(cuda), silu,
                             torch.tensor([delta, zp], device=cuda), _grid(8, False), out, C, ws, yout=yo, ldy=C)
    torch.cuda.synchronize()
    yref = y64.permute(0, 2, 1).reshape(B * S, C)
    scale = yref.abs().max().item()
    err = (yo.cpu().double() - yref).abs().max().item()
    tol = _norm_tol(scale, offset)
    print(f"\n[groupnorm offset {offset}] max |y - y64| = {err / max(1.0, scale):.3g} of range (bound {tol / max(1.0, scale):.3g})")
    assert err <= tol
    u = yref / delta + zp
    clip = ((u < -0.5) | (u > 255.5)).double().mean().item()
    assert 0.1 <= clip <= 0.4, clip
    got = out.cpu().long() + 128
    tie_aware_check(f"groupnorm[{offset},{'silu' if silu else 'nosilu'},{dtype}]", got, u, 0, 255, tol / delta + 1e-6,
                    record_property)
    if offset == 0 and not silu:
        # constant group: y = x * a + (beta - mean * a) with x == mean exactly, i.e. beta up to the rounding of the two fp32
        # operations on values of magnitude |beta| and |mean * a| (a = rstd * gamma): a window of 2^-23 of those, not _norm_tol
        a = gamma[:C // G].double() / (eps ** 0.5)
        wc = float(((beta[:C // G].double().abs() + (2.0 ** -8) * a.abs()) * 2.0 ** -23).max()) / delta
        tie_aware_check("groupnorm[constant group]", got.view(B * S, C)[:S, :C // G], u.view(B * S, C)[:S, :C // G], 0, 255, wc,
                        record_property)


@pytest.mark.parametrize("offset", [0, 16, 64], ids=["narrow_grid", "mean_16std", "mean_64std"])
def test_layernorm_value_edges(cuda, offset, record_property):
    """qd_layernorm_quant (three consumers, zero points 0 / 128 / 255 of one central-quantile delta) vs an fp64 LayerNorm,
    tie-aware with the same error model (the kernel writes no float output: w = _norm_tol / delta)."""
    from qdiff import hip
    g = torch.Generator().manual_seed(320 + offset)
    M, C = 70, 320
    x = torch.randn(M, C, generator=g) * 1.7 + 1.7 * offset
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    delta, zp = _narrow_grid(y64)
    zps = [zp, 0.0, 255.0]
    outs = [torch.empty((M, C), dtype=torch.int8, device=cuda) for _ in zps]
    hip.layernorm_quant(x.to(cuda), M, C, C, 1e-5, gamma.to(cuda), beta.to(cuda),
                        [torch.tensor([delta, z], device=cuda) for z in zps], [_grid(8, False)] * 3, outs, C)
    torch.cuda.synchronize()
    tol = _norm_tol(y64.abs().max().item(), offset)
    for o, z in zip(outs, zps):
        tie_aware_check(f"layernorm[{offset},zp{int(z)}]", o.cpu().long() + 128, y64 / delta + z, 0, 255, tol / delta + 1e-6,
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
# packed quotient (qd_bytes2_t / qd_pack4_t: the normalisation byte stores and the GEMM epilogues) on huge and non-finite values
# ------------------------------------------------------------------------------------------------
HUGE = [3e38, -3e38, float("inf"), float("-inf"), 3.4028235e38, -3.4028235e38, 1e38, -1e38]


def _certified(cuda, delta, zp):
    from qdiff import hip
    qp = hip.make_qparams(torch.tensor(delta, device=cuda), torch.tensor(float(zp), device=cuda))
    assert qp.cpu()[3].item() != 0, f"delta {delta!r} is not certified: the case would not reach the fast quotient"
    return qp


@pytest.mark.parametrize("zp", [0, 128, 255], ids=["zp0", "zp128", "zp255"])
def test_layernorm_packed_quotient_huge_and_infinite(cuda, zp, record_property):
    """qd_layernorm_quant with beta = +-3e38 / +-FLT_MAX / +-1e38 / +-inf on eight channels: those outputs are that huge or
    infinite value and must saturate at qmax / qmin on the fast quotient (the packed form used to send every one of them to
    qmin: y = x * rinv overflowed and e = fma(-y, delta, x) was NaN); the other channels as in test_layernorm_value_edges."""
    from qdiff import hip
    g = torch.Generator().manual_seed(38 + zp)
    M, C = 70, 320
    x = torch.randn(M, C, generator=g) * 1.7
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    delta, _ = _narrow_grid(y64)
    beta[5:5 + len(HUGE)] = torch.tensor(HUGE)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    out = torch.empty((M, C), dtype=torch.int8, device=cuda)
    hip.layernorm_quant(x.to(cuda), M, C, C, 1e-5, gamma.to(cuda), beta.to(cuda), [_certified(cuda, delta, zp)], [_grid(8, False)],
                        [out], C)
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
