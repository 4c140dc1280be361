"""Fused weights-only attention (engine.WEIGHT_ONLY_ATTN, qd_attn_h16) on the GPU.

1. Random draws against an fp64 attention of the SAME operand-rounded q / k / v (q^, k^, v^ = the inputs rounded to the
   operand type u: 2^-11 for fp16, 2^-8 for bf16).  With A[i][c] = sum_j P[i][j] |v^[j][c]| (fp64) the bound per output
   element is
       |out - ref| <= (u + eps_i + S * 2^-22 + 2^-18) * A[i][c] + S * 2^-25 * max|v^| + u_out * |ref|
   where u is P's rounding to the operand type (relative per p), eps_i = 2 * scale * d * 2^-23 * max_j sum_c |q^_ic k^_jc|
   the fp32 score accumulation error carried through exp (a score error of delta changes p by a factor e^delta; the row
   maximum's own error cancels in the normalisation, hence the 2), S * 2^-22 + 2^-18 the fp32 row sum, the P.V accumulation
   and exp2's ulp, S * 2^-25 max|v^| fp16's absolute rounding of subnormal probabilities, u_out = 2^-11 for fp16 rows (0 for
   fp32).  A wrong scale, an unmasked key tail, a stale rescale or a wrong head stride changes outputs by O(A), two to three
   orders of magnitude above the bound.
2. Softmax edges: a dominant key in the last tile (the rescale), equal scores (the mean of v), scores ~1e4 (everything but
   the maximum underflows), S = 1, a query tail of one row.
3. Module level: SD cross_attn_forward and the LDM attention block, knob on vs off; bit-identical where the gate says no.
4. Whole UNets in state (True, False) against the reference's weights-only golden `out_w`.
"""
import random

import pytest
import torch
import torch.nn.functional as F

from golden_util import load_fixture

pytestmark = pytest.mark.gpu

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture
def attn_knob():
    from qdiff import engine
    prev_a, prev_k = engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_KERNEL
    yield engine
    engine.set_weight_only_attention(prev_a)
    engine.set_weight_only_kernel(prev_k)


def _operands(dev, layout, B, T, S, H, d, dt, gen, scale_q=1.0):
    """(q, k, v, q_strides, k_strides, v_strides) of one stride layout, values N(0, 1) (q times scale_q)."""
    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float32).to(dev)
    if layout == "rows":                         # SD: Linear outputs [B, N, H*d]
        q, k, v = rnd(B, T, H * d) * scale_q, rnd(B, S, H * d), rnd(B, S, H * d)
        st = lambda t, n: (n * H * d, H * d, d, 1)
        return q.to(dt), k.to(dt), v.to(dt), st(q, T), st(k, S), st(v, S)
    if layout == "qkv":                          # LDM: channels-last rows of the qkv projection, channel = h*3d + {q,k,v}*d + i
        bq, bkv = rnd(B, T, 3 * H * d), rnd(B, S, 3 * H * d)
        bq[..., :] *= scale_q
        bq, bkv = bq.to(dt), bkv.to(dt)
        st = lambda n: (n * 3 * H * d, 3 * H * d, 3 * d, 1)
        return bq, bkv[..., d:], bkv[..., 2 * d:], st(T), st(S), st(S)
    q, k, v = rnd(B, H, T, d) * scale_q, rnd(B, H, S, d), rnd(B, H, S, d)        # head-major [B, H, N, d]
    st = lambda n: (H * n * d, d, n * d, 1)
    return q.to(dt), k.to(dt), v.to(dt), st(T), st(S), st(S)


def _view(x, B, N, H, d, strides):
    return torch.as_strided(x, (B, N, H, d), strides)


def _reference(q, k, v, B, T, S, H, d, qs, ks, vs, scale, op):
    """fp64 attention of the operand-rounded inputs; returns (ref rows [B*T, H*d], A rows, eps [B*T, H] per query and head)."""
    qh = _view(q, B, T, H, d, qs).to(op).double()
    kh = _view(k, B, S, H, d, ks).to(op).double()
    vh = _view(v, B, S, H, d, vs).to(op).double()
    s = torch.einsum("bthd,bshd->bhts", qh, kh) * scale
    p = torch.softmax(s, dim=-1)
    ref = torch.einsum("bhts,bshd->bthd", p, vh).reshape(B * T, H * d)
    a = torch.einsum("bhts,bshd->bthd", p, vh.abs()).reshape(B * T, H * d)
    m = torch.einsum("bthd,bshd->bhts", qh.abs(), kh.abs()).amax(dim=-1)                   # [B, H, T]
    eps = (2 * scale * d * 2.0 ** -23 * m).permute(0, 2, 1).reshape(B * T, H, 1).expand(B * T, H, d).reshape(B * T, H * d)
    return ref, a, eps, vh.abs().max().item()


def _check(out, ref, a, eps, vmax, S, op, out_dtype):
    u_out = 2.0 ** -11 if out_dtype == torch.float16 else 0.0
    bound = (U[op] + eps + S * 2.0 ** -22 + 2.0 ** -18) * a + S * 2.0 ** -25 * vmax + u_out * ref.abs()
    err = (out.double() - ref).abs()
    assert torch.isfinite(out).all()
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"worst error {ratio:.3f} x the bound (max |err| {err.max().item():.3e})"
    return ratio


def _run(engine, q, k, v, B, T, S, H, d, qs, ks, vs, scale, op, out_dtype):
    engine.set_weight_only_attention(op)
    n0 = engine.ATTN_H16_LAUNCHES
    out = engine.attention_h16(q, k, v, B, T, S, H, d, qs, ks, vs, scale, out_dtype)
    torch.cuda.synchronize()
    assert engine.ATTN_H16_LAUNCHES == n0 + 1
    assert out.shape == (B * T, H * d) and out.dtype == out_dtype
    return out


def _draws(n=100):
    rng = random.Random(20261016)
    ds = [8, 16, 24, 32, 40, 48, 64, 80, 96, 160]
    special = [1, 7, 31, 32, 33, 77, 127, 128, 129, 255, 600]
    out = []
    for i in range(n):
        d = ds[i % len(ds)]
        T = rng.choice(special) if rng.random() < 0.4 else rng.randint(1, 600)
        S = rng.choice(special) if rng.random() < 0.4 else rng.randint(1, 600)
        out.append(dict(d=d, T=T, S=S, H=rng.randint(1, 8), B=rng.randint(1, 3), layout=["rows", "qkv", "heads"][i % 3],
                        dt=[torch.float32, torch.float16, torch.bfloat16][(i // 3) % 3],
                        out=[torch.float32, torch.float16][(i // 2) % 2], op=[torch.float16, torch.bfloat16][(i // 5) % 2],
                        seed=1000 + i))
    return out


@pytest.mark.parametrize("case", _draws(), ids=lambda c: f"d{c['d']}_T{c['T']}_S{c['S']}_H{c['H']}_B{c['B']}_{c['layout']}_"
                         f"{str(c['dt'])[6:]}_{str(c['op'])[6:]}_{str(c['out'])[6:]}")
def test_random_draws_match_fp64_on_rounded_operands(cuda, attn_knob, case):
    c = case
    g = torch.Generator().manual_seed(c["seed"])
    B, T, S, H, d = c["B"], c["T"], c["S"], c["H"], c["d"]
    q, k, v, qs, ks, vs = _operands(cuda, c["layout"], B, T, S, H, d, c["dt"], g)
    scale = d ** -0.5
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, scale, c["op"], c["out"])
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, scale, c["op"])
    _check(out, ref, a, eps, vmax, S, c["op"], c["out"])


def test_wrong_scale_misses_the_bound(cuda, attn_knob):
    """The bound has teeth: the same draw against a reference with 1.1x the scale fails it by far."""
    g = torch.Generator().manual_seed(5)
    B, T, S, H, d = 2, 100, 90, 3, 40
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g)
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16, torch.float32)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, 1.1 * d ** -0.5, torch.float16)
    with pytest.raises(AssertionError):
        _check(out, ref, a, eps, vmax, S, torch.float16, torch.float32)
    ref2, a2, eps2, _ = _reference(q, k, v, B, T, S - 1, H, d, qs, ks, vs, d ** -0.5, torch.float16)   # a key short
    assert ((out.double() - ref2).abs() / ((U[torch.float16] + eps2) * a2)).max().item() > 10


@pytest.mark.parametrize("op", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_dominant_key_in_the_last_tile(cuda, attn_knob, op):
    """A key far above all others in the ragged last tile: every row's maximum moves there, O and l are rescaled."""
    g = torch.Generator().manual_seed(7)
    B, T, S, H, d = 2, 130, 161, 2, 40
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g)
    k4 = k.view(B, S, H, d)
    k4[:, S - 2] = 3.0 * q.view(B, T, H, d).mean(dim=1) / q.view(B, T, H, d).mean(dim=1).norm(dim=-1, keepdim=True) * d ** 0.5
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op, torch.float32)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op)
    _check(out, ref, a, eps, vmax, S, op, torch.float32)


def test_equal_scores_give_the_mean_of_v(cuda, attn_knob):
    g = torch.Generator().manual_seed(8)
    B, T, S, H, d = 1, 65, 77, 4, 80
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g)
    q.zero_()
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16, torch.float32)
    mean = v.view(B, S, H * d).to(torch.float16).double().mean(dim=1).expand(T, H * d)
    a = v.view(B, S, H * d).to(torch.float16).double().abs().mean(dim=1).expand(T, H * d)
    assert ((out.double() - mean).abs() <= (2.0 ** -11 + S * 2.0 ** -22) * a + 1e-7).all()


@pytest.mark.parametrize("op", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_scores_of_magnitude_1e4(cuda, attn_knob, op):
    """Scores ~1e4 apart: every probability but the row maximum's underflows to 0; no NaN / inf, the output is v of the
    maximising key."""
    g = torch.Generator().manual_seed(9)
    B, T, S, H, d = 1, 40, 200, 2, 32
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g, scale_q=60.0)
    k.mul_(60.0)
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op, torch.float32)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op)
    sc = torch.einsum("bthd,bshd->bhts", _view(q, B, T, H, d, qs).to(op).double(), _view(k, B, S, H, d, ks).to(op).double())
    assert sc.abs().max().item() * d ** -0.5 > 3e3
    assert torch.isfinite(out).all()
    _check(out, ref, a, eps, vmax, S, op, torch.float32)


def test_single_key_returns_v(cuda, attn_knob):
    g = torch.Generator().manual_seed(10)
    B, T, S, H, d = 3, 33, 1, 5, 24
    q, k, v, qs, ks, vs = _operands(cuda, "heads", B, T, S, H, d, torch.float16, g)
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16, torch.float32)
    want = _view(v, B, S, H, d, vs).float().reshape(B, 1, H * d).expand(B, T, H * d).reshape(B * T, H * d)
    assert torch.allclose(out, want, rtol=2.0 ** -20, atol=0)          # p = 1: only exp2's rounding of the row reference


def test_query_tail_of_one_row(cuda, attn_knob):
    g = torch.Generator().manual_seed(11)
    B, T, S, H, d = 2, 129, 64, 2, 160
    q, k, v, qs, ks, vs = _operands(cuda, "qkv", B, T, S, H, d, torch.float32, g)
    out = _run(attn_knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.bfloat16, torch.float16)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.bfloat16)
    _check(out, ref, a, eps, vmax, S, torch.bfloat16, torch.float16)


# ---- 3. module level ---------------------------------------------------------------------------------------------------------
def _model(name, dev):
    import os
    import tempfile

    import qdiff
    from golden_util import build_ckpt, build_engine_model, fixture_inputs, quant_params
    from qdiff.utils import resume_cali_model
    fx = load_fixture(f"model_{name}.pt")
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    qnn = qdiff.QuantModel(build_engine_model(spec).to(dev), wq, aq, sm_abit=spec["sm_abit"]).to(dev).eval()
    cal = tuple(a for a in fixture_inputs(fx, "cal") if a is not None)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ckpt.pth")
        torch.save(build_ckpt(fx), path)
        resume_cali_model(qnn, path, cal, quant_act=True, cond=spec["ctx"] is not None)
    return qnn, fx


def _first(qnn, cls):
    return next(m for m in qnn.modules() if isinstance(m, cls))


def _sd_attn(cuda):
    from qdiff.quant_block import QuantBasicTransformerBlock
    qnn, fx = _model("sd_tiny", cuda)
    blk = _first(qnn, QuantBasicTransformerBlock)
    g = torch.Generator().manual_seed(3)
    dim = blk.attn1.to_q.weight.shape[1]
    x = torch.randn(2, 64, dim, generator=g).to(cuda)
    ctx = torch.randn(2, 7, blk.attn2.to_k.weight.shape[1], generator=g).to(cuda)
    return qnn, blk, x, ctx


def _pair(engine, fn):
    engine.set_weight_only_attention(None)
    y0 = fn()
    engine.set_weight_only_attention(torch.float16)
    n0 = engine.ATTN_H16_LAUNCHES
    y1 = fn()
    torch.cuda.synchronize()
    return y0, y1, engine.ATTN_H16_LAUNCHES - n0


def _rel(y, ref):
    return (y.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()


def test_sd_cross_attn_forward_knob_on_vs_off(cuda, attn_knob):
    qnn, blk, x, ctx = _sd_attn(cuda)
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        for att, c in ((blk.attn1, None), (blk.attn2, ctx)):
            y0, y1, n = _pair(attn_knob, lambda: att(x, context=c))
            assert n == 1 and y1.dtype == y0.dtype and y1.shape == y0.shape
            assert _rel(y1, y0) < 5e-3, _rel(y1, y0)


def test_sd_cross_attn_forward_keeps_the_library_path(cuda, attn_knob):
    """A mask, grad enabled, and the states (True, True) / (False, False): bit-identical to the knob off, no launch."""
    qnn, blk, x, ctx = _sd_attn(cuda)
    att = blk.attn2
    mask = torch.ones(2, 7, dtype=torch.bool, device=cuda)
    mask[:, 5:] = False
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        y0, y1, n = _pair(attn_knob, lambda: att(x, context=ctx, mask=mask))
        assert n == 0 and torch.equal(y0, y1)
    y0, y1, n = _pair(attn_knob, lambda: att(x, context=ctx).detach())
    assert n == 0 and torch.equal(y0, y1)
    for state in ((True, True), (False, False)):
        qnn.set_quant_state(*state)
        with torch.no_grad():
            y0, y1, n = _pair(attn_knob, lambda: att(x, context=ctx))
        assert n == 0 and torch.equal(y0, y1), state


def _ldm_block(cuda):
    from qdiff.quant_block import QuantAttentionBlock
    qnn, fx = _model("ldm_tiny", cuda)
    blk = _first(qnn, QuantAttentionBlock)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, blk.channels, 8, 8, generator=g).to(cuda)
    return qnn, blk, x


@pytest.mark.parametrize("layers", [False, True], ids=["attn_only", "with_layer_kernel"])
def test_ldm_attention_block_knob_on_vs_off(cuda, attn_knob, layers):
    qnn, blk, x = _ldm_block(cuda)
    qnn.set_quant_state(True, False)
    attn_knob.set_weight_only_kernel(torch.float16 if layers else None)
    with torch.no_grad():
        y0, y1, n = _pair(attn_knob, lambda: blk(x))
    assert n == 1 and y1.dtype == y0.dtype and y1.shape == y0.shape
    assert _rel(y1, y0) < 5e-3, _rel(y1, y0)
    assert blk.attention.qkv_matmul.scale is not None


def test_ldm_attention_block_keeps_the_library_path(cuda, attn_knob):
    qnn, blk, x = _ldm_block(cuda)
    qnn.set_quant_state(True, False)
    y0, y1, n = _pair(attn_knob, lambda: blk(x).detach())
    assert n == 0 and torch.equal(y0, y1)
    h = blk.attention.qkv_matmul.register_forward_hook(lambda *a: None)
    try:
        with torch.no_grad():
            y0, y1, n = _pair(attn_knob, lambda: blk(x))
        assert n == 0 and torch.equal(y0, y1)
    finally:
        h.remove()
    for state in ((True, True), (False, False)):
        qnn.set_quant_state(*state)
        with torch.no_grad():
            y0, y1, n = _pair(attn_knob, lambda: blk(x))
        assert n == 0 and torch.equal(y0, y1), state


# ---- 4. whole UNets ----------------------------------------------------------------------------------------------------------
MODELS = ["ldm_tiny", "sd_tiny", "ldm_updown_tiny", "ldm_full", "sd_full", "churches_full"]
# (max |diff| / range, min cosine) against the reference's weights-only fp32 golden `out_w`: 2x the worst value measured over
# the six models on an MI355X (max |diff| = 2x, 1 - cosine = 2x):
#   attention fp16 alone:           worst 3.300e-4 of range (sd_tiny), worst cosine 0.9999998 (sd_tiny)  -> 6.60e-4, 0.9999990
#     (two runs: 3.30e-4 / 2.68e-4, cosine 0.9999999 / 0.9999998; a cosine taken in fp32 resolves ~1e-7, so that floor is
#     1 - 1e-6 rather than 2x a difference at the resolution)
#   attention bf16 alone:           worst 1.919e-3 (sd_tiny), worst cosine 0.9999979 (sd_tiny)            -> 3.84e-3, 0.9999958
#   with QDIFF_WEIGHT_ONLY=fp16:    worst 1.207e-3 (sd_tiny), worst cosine 0.9999995 (sd_tiny)            -> 2.41e-3, 0.9999990
#   both fp16 under fp16 autocast:  worst 1.858e-3 (sd_tiny), worst cosine 0.9999979 (sd_full)            -> 3.72e-3, 0.9999958
BOUNDS = {"attn_fp16": (6.60e-4, 0.9999990), "attn_bf16": (3.84e-3, 0.9999958), "both_fp16": (2.41e-3, 0.9999990),
          "autocast": (3.72e-3, 0.9999958)}


def _unet_run(qnn, fx, dev, autocast=False):
    from golden_util import fixture_inputs
    x, t, c = fixture_inputs(fx, "test")
    args = (x.to(dev), t.to(dev)) + ((c.to(dev),) if c is not None else ())
    with torch.no_grad(), torch.autocast("cuda", enabled=autocast):
        y = qnn(*args)
    torch.cuda.synchronize()
    return y


def _metrics(y, ref):
    rng = ref.abs().max().item()
    d = (y.float().cpu() - ref).abs().max().item() / rng
    return d, F.cosine_similarity(y.float().cpu().flatten(), ref.flatten(), dim=0).item()


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("mode", ["attn_fp16", "attn_bf16", "both_fp16", "autocast"])
def test_weight_only_unet_with_fused_attention(cuda, attn_knob, name, mode):
    qnn, fx = _model(name, cuda)
    qnn.set_quant_state(True, False)
    attn_knob.set_weight_only_kernel(torch.float16 if mode in ("both_fp16", "autocast") else None)
    attn_knob.set_weight_only_attention(torch.bfloat16 if mode == "attn_bf16" else torch.float16)
    n0 = attn_knob.ATTN_H16_LAUNCHES
    y = _unet_run(qnn, fx, cuda, autocast=mode == "autocast")
    launches = attn_knob.ATTN_H16_LAUNCHES - n0
    d, cos = _metrics(y, fx["out_w"])
    print(f"\n[{name}] {mode}: {launches} attention launches, {d:.3e} of range, cosine {cos:.7f}")
    assert launches > 0
    tol, cmin = BOUNDS[mode]
    assert d <= tol and cos >= cmin
