"""Wide weights-only fusion (engine.WEIGHT_ONLY_FUSE_WIDE) on the GPU: the GEGLU epilogue of qd_conv2d_wq_h16
(QD_EPI_GEGLU_H16) against the two-launch form it replaces (bit for bit) and against fp64, every transformer block,
SpatialTransformer and attention block against the fused route with the knob off, and whole UNets against the reference's
weights-only golden output.

fp64 bound of the epilogue, per output element, with h = x^ W^T + bias the fp64 projection of the SAME rounded operands
(tests/test_weight_only_gpu.py: |h_kernel - h| <= c = K 2^-26 S + 2^-22 (|bias| + |h|) for the value a and the gate g alike) and
y = a G(g), G(g) = 0.5 g (1 + erf(g / sqrt 2)), |G'| <= 1.13:
    |out - y| <= half an ulp of the output type at y  +  2^-23 |a g| + 3 u |y|          (qd_geglu_h16's bound, test_weight_only_fused_gpu.py)
                 +  |G(g)| c_a + 1.13 |a| c_g + 1.13 c_a c_g                               (the contraction's error carried through)
The output rows have ldo as their row stride AND as the end of the zero padding (as for qd_geglu_h16), so a row has no column
that is neither a feature nor padding: the guards are the rows in front of and behind the M rows, which also covers the rows
of the last 128-row tile past M.
"""
import math
import os
import random
import tempfile
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from golden_util import build_engine_model, load_fixture, quant_params
from test_weight_only_fused_gpu import GUARD, U, _guarded, _half_ulp
from test_weight_only_gpu import BOUNDS, MODELS, _codes, _metrics, _resume, _run, _wquant

pytestmark = pytest.mark.gpu
BRANCH = 0.927734375 * math.sqrt(2.0)          # gate at which qd_erff's argument crosses its branch point


@pytest.fixture
def knob():
    """The engine with all four weights-only knobs and the counters restored afterwards."""
    from qdiff import engine
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE)
    yield engine
    engine.set_weight_only_kernel(prev[0])
    engine.set_weight_only_attention(prev[1])
    engine.set_weight_only_fusion(prev[2])
    engine.set_weight_only_fusion_wide(prev[3])
    for k in ("spatial", "attnblock"):
        engine.WONLY_FUSED.pop(k, None)


def _reset(engine):
    for k in ("spatial", "attnblock"):
        engine.WONLY_FUSED.pop(k, None)
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0
    engine.WONLY_GEGLU_EPI[0] = 0


# ---- the epilogue alone ------------------------------------------------------------------------------------------------------
def _epi_host(seed, wbits, act, Fd, K, M, pad, edges=False, x=None, bias=None, dscale=1.0):
    """Host side of one GEGLU projection [2F][K]: activations, weights, bias and the per-channel quantiser.  x / bias replace the
    drawn ones; dscale (a power of two) scales weights, delta and bias alike: the same codes, every projection times dscale."""
    g = torch.Generator().manual_seed(seed)
    xr = torch.randn(M, K, generator=g)
    w = torch.randn(2 * Fd, K, generator=g) * (2.0 / math.sqrt(K))
    br = torch.randn(2 * Fd, generator=g)
    x = xr if x is None else x.clone()
    bias = br * dscale if bias is None else bias.clone()
    if edges:                                   # rows of zeros: value / gate are then the bias itself, placed at the edges
        x[:min(M, 4)] = 0
        vals = torch.tensor([BRANCH, -BRANCH, 12.0, -12.0, 40.0, -40.0, 0.0, 3e4, -3e4], dtype=torch.float32)
        for d in (0.0, 1.0, -1.0):              # the fp32 neighbours of the branch point too
            vals = torch.cat([vals, torch.nextafter(vals[:2], vals[:2] + d)])
        bias[Fd:Fd + min(Fd, vals.numel())] = vals[:min(Fd, vals.numel())]
    q = _wquant(w, wbits, "range", g)
    q.delta = q.delta * dscale
    return NS(x=x, w=w * dscale, bias=bias, q=q, M=M, F=Fd, K=K, ldo=Fd + pad, act=act)


def _epi_setup(dev, seed, wbits, act, Fd, K, M, pad, via_tiles=False, edges=False, host=None):
    """One GEGLU projection [2F][K]: the un-permuted plan, the interleaved plan, the rounded operand rows and the host copies."""
    from qdiff import engine
    s = host or _epi_host(seed, wbits, act, Fd, K, M, pad, edges)
    Fd, K, M = s.F, s.K, s.M
    qd = NS(**{**vars(s.q), "delta": s.q.delta.to(dev), "zero_point": s.q.zero_point.to(dev)})
    pack = engine.pack_module_weights(s.w.to(dev), [qd], 0)
    perm = engine.geglu_row_perm(Fd, dev)
    gpack = engine.pack_select_tiles(pack, perm) if via_tiles else engine.pack_module_weights(s.w.to(dev), [qd], 0, row_perm=perm)
    plan = engine.build_wonly_plan(pack, 1, 1, 1, 0, s.bias.to(dev), s.act)
    gplan = engine.build_wonly_plan(gpack, 1, 1, 1, 0, s.bias.to(dev), s.act, geglu=True)
    assert plan is not None and gplan is not None
    xh = engine.wonly_rows(s.x.to(dev), plan, 1, K, M, (0, 1, K))
    return NS(**vars(s), plan=plan, gplan=gplan, xh=xh)


def _epi_launch(s, dev, plan=None):
    """One QD_EPI_GEGLU_H16 launch into guarded rows -> (buffer, rows)."""
    from qdiff import hip
    p = plan or s.gplan
    buf, out = _guarded(s.M, s.ldo, s.act, dev)
    call = hip.ConvCall(x=s.xh, w=p.pack.wq, out=out, bias=p.bias, ldx=p.ldx, ldk=p.pack.ldk, ldo=s.ldo, B=1, H=1, W=s.M, Ho=1, Wo=s.M,
                        Cout=p.Cout, kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=p.pack.wbits, w_tiled=True, segs=p.segs,
                        epilogue=hip.EPI_GEGLU_H16)
    hip.conv2d_wq_h16(call, s.act)
    torch.cuda.synchronize()
    return buf, out


def _guards_ok(buf, out, Fd, what):
    assert (buf[:GUARD] == 7.5).all() and (buf[-GUARD:] == 7.5).all(), f"{what}: rows outside [0, M) were written"
    assert (out[:, Fd:] == 0).all(), f"{what}: pad columns are not zero"


GEGLU_F = [256, 512, 1280, 2560, 5120] + [32, 96, 160]          # the golden models' F first; 96 and 160 end in a 64-column block


def _epi_draws(n, seed):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        Fd = GEGLU_F[i % len(GEGLU_F)]
        K = rnd.choice([64, 128, 320] if i % 2 == 0 else [40, 72, 200, 328])           # without / with a 64-channel tail
        M = rnd.choice([1, 77, 130, 257, 300]) if Fd > 1280 else rnd.choice([1, 77, 128, 130, 257, 640, 1100])
        out.append((500 + i, 4 if i % 2 == 0 else 8, torch.float16 if (i // 2) % 2 == 0 else torch.bfloat16, Fd, K, M,
                    rnd.choice([0, 8, 16, 56]), i % 3 == 0))
    return out


def _eid(c):
    return f"{c[0]}-W{c[1]}-{str(c[2])[6:]}-F{c[3]}-K{c[4]}-M{c[5]}-pad{c[6]}-{'tiles' if c[7] else 'packed'}"


@pytest.mark.parametrize("case", _epi_draws(48, 11), ids=_eid)
def test_geglu_epilogue_equals_the_two_launch_form(cuda, case):
    """qd_conv2d_wq_h16 (linear, fp32 out, un-permuted pack) + qd_geglu_h16 — the path of the wide knob off — against ONE launch
    with the GEGLU epilogue on the interleaved pack of the same weights: the same fp32 operations in the same order (the row
    permutation does not change the K order), so the operand rows are equal bit for bit."""
    from qdiff import engine, hip
    seed, wbits, act, Fd, K, M, pad, via_tiles = case
    s = _epi_setup(cuda, seed, wbits, act, Fd, K, M, pad, via_tiles, edges=seed % 4 == 0)
    h = engine.wonly_forward(s.plan, s.xh, 1, 1, M, 1, M)
    rbuf, ref = _guarded(M, s.ldo, act, cuda)
    hip.geglu_h16(h, M, Fd, 2 * Fd, ref, s.ldo)
    buf, out = _epi_launch(s, cuda)
    _guards_ok(buf, out, Fd, _eid(case))
    diff = (out.view(torch.int16) != ref.view(torch.int16))
    n = int(diff.sum().item())
    print(f"\ngeglu epilogue {_eid(case)}: {n} of {out.numel()} elements differ from the two-launch form")
    assert n == 0, f"{n} elements differ; first at {diff.nonzero()[0].tolist()}"


def _epi_ref(s):
    """fp64 value * GELU(gate) of the host projection s (the SAME rounded operands) and the bound of the module docstring:
    (ref, tol, fp64 projection h)."""
    Fd, K, act = s.F, s.K, s.act
    xr = s.x.to(act).double()
    wq = ((_codes(s.w, s.q) - s.q.zero_point.view(-1, 1)) * s.q.delta.view(-1, 1)).double()
    h = xr @ wq.t() + s.bias.double()
    S = xr.abs() @ wq.abs().t()
    c = K * 2.0 ** -26 * S + 2.0 ** -22 * (s.bias.double().abs() + h.abs())
    a, gt, ca, cg = h[:, :Fd], h[:, Fd:], c[:, :Fd], c[:, Fd:]
    G = 0.5 * gt * (1 + torch.erf(gt / math.sqrt(2)))
    ref = a * G
    tol = _half_ulp(ref, act) + 2.0 ** -23 * (a * gt).abs() + 3 * U * ref.abs() + G.abs() * ca + 1.13 * a.abs() * cg + 1.13 * ca * cg
    return ref, tol, h


def _fp64_case(dev, seed, wbits, act, Fd, K, M, pad, mode="kernel"):
    s = _epi_setup(dev, seed, wbits, act, Fd, K, M, pad, edges=True)
    ref, tol, h = _epi_ref(s)
    if mode in ("kernel", "unpermuted"):
        buf, out = _epi_launch(s, dev, plan=None if mode == "kernel" else NS(pack=s.plan.pack, bias=s.plan.bias, ldx=s.plan.ldx,
                                                                             Cout=s.plan.Cout, segs=s.plan.segs))
        _guards_ok(buf, out, Fd, f"fp64 {mode}")
        got = out[:, :Fd].double().cpu()
    else:                                                   # what a wrong epilogue would write, from the exact projection
        hf = h.float()
        af, gf = (hf[:, Fd:], hf[:, :Fd]) if mode == "swapped" else (hf[:, :Fd], hf[:, Fd:])
        got = (af * F.gelu(gf, approximate="tanh" if mode == "tanh" else "none")).to(act).double()
    finite = torch.isfinite(ref) & (ref.abs() < (6e4 if act == torch.float16 else 3e38))
    return ((got - ref).abs() / tol)[finite].max().item()


@pytest.mark.parametrize("case", _epi_draws(24, 12), ids=_eid)
def test_geglu_epilogue_matches_fp64(cuda, case):
    seed, wbits, act, Fd, K, M, pad, _ = case
    worst = _fp64_case(cuda, seed, wbits, act, Fd, K, M, pad)
    print(f"\ngeglu epilogue vs fp64 {_eid(case)}: {worst:.3f} x bound")
    assert worst <= 1.0


@pytest.mark.parametrize("act", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_geglu_epilogue_bound_bites(cuda, act):
    """tanh-GELU, swapped value / gate, and the un-permuted pack under the epilogue each miss the bound."""
    assert _fp64_case(cuda, 21, 4, act, 256, 128, 130, 0) <= 1.0
    for mode in ("tanh", "swapped", "unpermuted"):
        worst = _fp64_case(cuda, 21, 4, act, 256, 128, 130, 0, mode=mode)
        print(f"geglu epilogue negative control {mode} {act}: {worst:.3g} x bound")
        assert worst > 1.0, mode


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def _wide_blocks(qnn):
    from qdiff.arch import ldm_unet
    from qdiff.quant_block import QuantAttentionBlock, QuantBasicTransformerBlock
    kinds = ((QuantBasicTransformerBlock, "transformer"), (ldm_unet.SpatialTransformer, "spatial"), (QuantAttentionBlock, "attnblock"))
    return [(n, m, k) for n, m in qnn.named_modules() for cls, k in kinds if isinstance(m, cls)]


@pytest.mark.parametrize("name", ["sd_tiny", "ldm_tiny", "sd_full", "ldm_full", "churches_full"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_blocks_against_the_fused_route(cuda, knob, name, dt):
    """Every transformer block, SpatialTransformer and attention block, teacher-forced with its input of a knobs-off fp32
    evaluation (the scheme of profiles/wonly_fused_block_parity.txt): the wide route's error against the knobs-off fp32 output
    of the block is at most twice the error of the fused route with the wide knob off on the same input, with a floor of one
    ulp of the operand type (2^-10 / 2^-7) of the range.  A transformer block differs only by the GEGLU epilogue, so it must be
    bit-equal.  Attention knob off and on."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    blocks = _wide_blocks(qnn)
    assert blocks
    rec, hooks = {}, []
    for n, b, _ in blocks:
        hooks.append(b.register_forward_pre_hook(lambda m, a, k, n=n: rec.__setitem__(n, [a, k, None]), with_kwargs=True))
        hooks.append(b.register_forward_hook(lambda m, a, o, n=n: rec[n].__setitem__(2, o)))
    knob.set_weight_only_kernel(None)
    knob.set_weight_only_attention(None)
    knob.set_weight_only_fusion(False)
    knob.set_weight_only_fusion_wide(False)
    try:
        _run(qnn, fx, cuda)
    finally:
        for h in hooks:
            h.remove()
    floor = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_fusion(True)
    bad = []
    for attn in (None, dt):
        knob.set_weight_only_attention(attn)
        for n, b, kind in blocks:
            a, k, ref = rec[n]
            rng = ref.abs().max().item()
            with torch.no_grad():
                knob.set_weight_only_fusion_wide(False)
                y0 = b(*a, **k)
                knob.set_weight_only_fusion_wide(True)
                _reset(knob)
                y1 = b(*a, **k)
            torch.cuda.synchronize()
            e0, e1 = (y0 - ref).abs().max().item() / rng, (y1 - ref).abs().max().item() / rng
            took = knob.WONLY_GEGLU_EPI[0] if kind == "transformer" else knob.WONLY_FUSED.get(kind, 0)
            assert took == 1, f"{n} did not take the wide route"
            assert y1.dtype == ref.dtype and y1.shape == ref.shape
            same = torch.equal(y0, y1)
            print(f"[wide-block-parity] {name} {str(dt)[6:]} attn={'on' if attn else 'off'} {n} ({kind}): wide off {e0:.3e} "
                  f"wide on {e1:.3e} of range, ratio {e1 / max(e0, 1e-30):.3f} (bound {max(2 * e0, floor):.3e}) bit-equal={same}")
            if e1 > max(2 * e0, floor) or (kind == "transformer" and not same):
                bad.append((n, kind, attn, e0, e1, same))
    assert not bad, bad


# ---- whole UNets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("attn", [False, True], ids=["libattn", "attn"])
def test_wide_unet_matches_reference(cuda, knob, name, dt, attn):
    """State (True, False), layer knob, fusion and the wide knob on, against the reference's weights-only golden `out_w`, inside
    tests/test_weight_only_gpu.py's BOUNDS; the counters show which blocks took the route; two runs bit-equal; a model without a
    covered block bit-equal to the wide knob off."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_attention(dt if attn else None)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_wide(False)
    y_off = _run(qnn, fx, cuda)
    knob.set_weight_only_fusion_wide(True)
    _reset(knob)
    y = _run(qnn, fx, cuda)
    took, epi = dict(knob.WONLY_FUSED), knob.WONLY_GEGLU_EPI[0]
    y2 = _run(qnn, fx, cuda)
    blocks = _wide_blocks(qnn)
    count = lambda kind: sum(k == kind for _, _, k in blocks)
    d, cos = _metrics(y, fx["out_w"])
    d0, cos0 = _metrics(y_off, fx["out_w"])
    print(f"\n[{name}] wide {dt} attn={attn}: {took}, {epi} GEGLU epilogues, {d:.3e} of range, cosine {cos:.7f} "
          f"(wide off: {d0:.3e}, {cos0:.7f})")
    assert epi == count("transformer") == took["transformer"]
    assert took.get("spatial", 0) == count("spatial") and took.get("attnblock", 0) == count("attnblock")
    assert y.dtype == torch.float32 and torch.equal(y, y2)
    if not blocks:
        assert torch.equal(y, y_off) and set(took) == {"resblock", "transformer"}
    tol, cmin = BOUNDS[dt]
    assert d <= tol and cos >= cmin


def test_packed_checkpoint_takes_the_epilogue_bit_identically(cuda, knob):
    """save_packed_ckpt -> load_packed_ckpt(free_weights=True) into a model whose fp32 weights differ: the wide route runs from
    the frozen packs (the GEGLU plan gathered tile by tile or taken from the checkpoint's interleaved pack) and gives its source
    model's bits."""
    import qdiff
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    fx = load_fixture("model_sd_tiny.pt")
    src = _resume(fx, cuda)
    knob.set_weight_only_kernel(torch.float16)
    knob.set_weight_only_attention(torch.float16)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_wide(True)
    src.set_quant_state(True, False)
    y_src = _run(src, fx, cuda)
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
    y1 = _run(dst, fx, cuda)
    assert knob.WONLY_GEGLU_EPI[0] == sum(k == "transformer" for _, _, k in _wide_blocks(dst)) > 0
    assert torch.equal(y1, y_src)
