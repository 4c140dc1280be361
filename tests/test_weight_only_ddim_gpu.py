"""The weights-only route of the DDIM family (engine.WEIGHT_ONLY_FUSE_DDIM) on the GPU.

1. qd_attn_h16 at head dims 168 .. 256 (DK = 11 .. 16) against the fp64 attention of the operand-rounded inputs, with the
   bound, the operands and the reference of tests/test_weight_only_attention_gpu.py (the bound carries d): seeded draws over
   every wide DK, the token counts around the 32-key tile and the 128-query block, the three stride layouts, the three input
   types, both operand and both output types; one shape through every instantiation (DK x input type x operand type); the
   softmax edges at d = 256, the wrong-scale case and guard rows.
2. Every QuantResnetBlock / QuantAttnBlock of the CIFAR fixtures, teacher-forced, by the criterion of
   tests/test_weight_only_fused_gpu.py::test_blocks_against_the_unfused_kernel_route.
3. Whole CIFAR UNets against the reference's weights-only golden `out_w` inside tests/test_weight_only_gpu.py's BOUNDS, the
   counters against the block census, run-to-run bits, a packed checkpoint with freed weights.
4. An LDM and an SD fixture: the new knob changes no byte and no counter.
"""
import os
import random

import pytest
import torch

from golden_util import load_fixture
from test_weight_only_attention_gpu import _check, _operands, _reference, _run as _attn_run, _view
from test_weight_only_gpu import BOUNDS, _metrics, _resume, _run

pytestmark = pytest.mark.gpu


@pytest.fixture
def knob():
    """The engine with every weights-only knob and the keys of WONLY_FUSED restored afterwards."""
    from qdiff import engine
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_DDIM)
    keys = set(engine.WONLY_FUSED)
    yield engine
    engine.set_weight_only_kernel(prev[0])
    engine.set_weight_only_attention(prev[1])
    engine.set_weight_only_fusion(prev[2])
    engine.set_weight_only_fusion_ddim(prev[3])
    for k in [k for k in engine.WONLY_FUSED if k not in keys]:
        del engine.WONLY_FUSED[k]


def _reset(engine):
    for k in ("resnetblock", "attnblock_ddim", "head_ddim"):
        engine.WONLY_FUSED.pop(k, None)
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0


# ---- 1. the wide head dims against fp64 -------------------------------------------------------------------------------------
WIDE = [168, 176, 192, 200, 224, 248, 256]                  # DK = 11, 11, 12, 13, 14, 16, 16; 232 / 240 (DK 15) join below
SIZES = [1, 31, 32, 33, 127, 128, 129, 256, 300]


def _draws(n=60):
    rng = random.Random(20261019)
    ds = WIDE + [240]
    out = []
    for i in range(n):
        out.append(dict(d=ds[i % len(ds)], T=rng.choice(SIZES), S=rng.choice(SIZES), H=rng.randint(1, 2), B=rng.randint(1, 3),
                        layout=["rows", "qkv", "heads"][i % 3], dt=[torch.float32, torch.float16, torch.bfloat16][(i // 3) % 3],
                        out=[torch.float32, torch.float16][(i // 2) % 2], op=[torch.float16, torch.bfloat16][(i // 5) % 2],
                        seed=3000 + i))
    return out


@pytest.mark.parametrize("case", _draws(), ids=lambda c: f"d{c['d']}_T{c['T']}_S{c['S']}_H{c['H']}_B{c['B']}_{c['layout']}_"
                         f"{str(c['dt'])[6:]}_{str(c['op'])[6:]}_{str(c['out'])[6:]}")
def test_wide_head_dims_match_fp64_on_rounded_operands(cuda, knob, case):
    c = case
    g = torch.Generator().manual_seed(c["seed"])
    B, T, S, H, d = c["B"], c["T"], c["S"], c["H"], c["d"]
    q, k, v, qs, ks, vs = _operands(cuda, c["layout"], B, T, S, H, d, c["dt"], g)
    scale = d ** -0.5
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, scale, c["op"], c["out"])
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, scale, c["op"])
    ratio = _check(out, ref, a, eps, vmax, S, c["op"], c["out"])
    print(f"\nd={d} T={T} S={S}: worst error {ratio:.3f} x the bound")


@pytest.mark.parametrize("op", [torch.float16, torch.bfloat16], ids=["op_fp16", "op_bf16"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16], ids=["in_fp32", "in_fp16", "in_bf16"])
def test_every_wide_instantiation_at_one_shape(cuda, knob, dt, op):
    """The seeded draws tie d, the input type and the operand type to the draw's index, so some of the 36 instantiations
    (DK 11 .. 16 x input type x operand type) never meet them: here the largest d of every DK runs each combination once, at a
    shape with a query tail, more than one query block and a ragged last key tile."""
    B, T, S, H = 2, 161, 75, 1
    for d in (176, 192, 208, 224, 240, 256):
        g = torch.Generator().manual_seed(4000 + d)
        q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, dt, g)
        out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op, torch.float32)
        _check(out, *_reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op)[:4], S, op, torch.float32)


def test_wrong_scale_misses_the_bound(cuda, knob):
    """The bound has teeth at d = 256 too: the same draw against a reference with 1.1x the scale fails it."""
    g = torch.Generator().manual_seed(5)
    B, T, S, H, d = 2, 100, 90, 1, 256
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g)
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16, torch.float32)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16)
    _check(out, ref, a, eps, vmax, S, torch.float16, torch.float32)
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, 1.1 * d ** -0.5, torch.float16)
    with pytest.raises(AssertionError):
        _check(out, ref, a, eps, vmax, S, torch.float16, torch.float32)


@pytest.mark.parametrize("op", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_softmax_edges_at_d256(cuda, knob, op):
    """The edges of tests/test_weight_only_attention_gpu.py at d = 256: a dominant key in the ragged last tile, equal scores,
    scores ~1e4, S = 1, a query tail of one row."""
    d, H = 256, 1
    sc = d ** -0.5
    g = torch.Generator().manual_seed(7)
    # dominant key in the ragged last tile: every row's maximum moves there, O and l are rescaled
    B, T, S = 2, 130, 161
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, op, g)
    qm = q.float().view(B, T, H, d).mean(dim=1)
    k.view(B, S, H, d)[:, S - 2] = (3.0 * qm / qm.norm(dim=-1, keepdim=True) * d ** 0.5).to(op)
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, sc, op, torch.float32)
    _check(out, *_reference(q, k, v, B, T, S, H, d, qs, ks, vs, sc, op)[:4], S, op, torch.float32)
    # equal scores: the mean of v
    B, T, S = 1, 65, 77
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, op, g)
    q.zero_()
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, sc, op, torch.float32)
    vd = v.view(B, S, H * d).double()
    u = 2.0 ** -11 if op == torch.float16 else 2.0 ** -8
    assert ((out.double() - vd.mean(dim=1).expand(T, H * d)).abs() <= (u + S * 2.0 ** -22) * vd.abs().mean(dim=1).expand(T, H * d) + 1e-7).all()
    # scores ~1e4 apart: everything but the row maximum underflows
    B, T, S = 1, 40, 200
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, g, scale_q=40.0)
    q, k, v = q.to(op), (k * 40.0).to(op), v.to(op)
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, sc, op, torch.float32)
    s = torch.einsum("bthd,bshd->bhts", _view(q, B, T, H, d, qs).double(), _view(k, B, S, H, d, ks).double())
    assert s.abs().max().item() * sc > 3e3 and torch.isfinite(out).all()
    _check(out, *_reference(q, k, v, B, T, S, H, d, qs, ks, vs, sc, op)[:4], S, op, torch.float32)
    # a single key: p = 1, the output is v
    B, T, S = 3, 33, 1
    q, k, v, qs, ks, vs = _operands(cuda, "heads", B, T, S, H, d, op, g)
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, sc, op, torch.float32)
    want = _view(v, B, S, H, d, vs).float().reshape(B, 1, H * d).expand(B, T, H * d).reshape(B * T, H * d)
    assert torch.allclose(out, want, rtol=2.0 ** -20, atol=0)
    # a query tail of one row
    B, T, S = 2, 129, 64
    q, k, v, qs, ks, vs = _operands(cuda, "qkv", B, T, S, H, d, op, g)
    out = _attn_run(knob, q, k, v, B, T, S, H, d, qs, ks, vs, sc, op, torch.float16)
    _check(out, *_reference(q, k, v, B, T, S, H, d, qs, ks, vs, sc, op)[:4], S, op, torch.float16)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_guard_rows_and_columns_stay_untouched(cuda, knob, out_dtype):
    """Nothing outside [0, B T) x [0, H d) of the output is written: rows in front and behind, columns past H d."""
    from qdiff import hip
    g = torch.Generator().manual_seed(13)
    B, T, S, H, d, guard, pad = 2, 65, 33, 1, 248, 3, 8
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float16, g)
    buf = torch.full((B * T + 2 * guard, H * d + pad), 7.5, dtype=out_dtype, device=cuda)
    out = buf[guard:guard + B * T]
    hip.attn_h16(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16, out)
    torch.cuda.synchronize()
    assert (buf[:guard] == 7.5).all() and (buf[-guard:] == 7.5).all() and (out[:, H * d:] == 7.5).all()
    _check(out[:, :H * d], *_reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, torch.float16)[:4], S, torch.float16, out_dtype)


# ---- 2. blocks, teacher-forced ------------------------------------------------------------------------------------------------
def _ddim_blocks(qnn):
    from qdiff.quant_block import QuantAttnBlock, QuantResnetBlock
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, (QuantResnetBlock, QuantAttnBlock))]


def _census(qnn):
    from qdiff.quant_block import QuantAttnBlock, QuantResnetBlock
    blocks = _ddim_blocks(qnn)
    return {"resblock": 0, "transformer": 0, "resnetblock": sum(isinstance(m, QuantResnetBlock) for _, m in blocks),
            "attnblock_ddim": sum(isinstance(m, QuantAttnBlock) for _, m in blocks), "head_ddim": 1}


@pytest.mark.parametrize("name", ["cifar_tiny", "cifar_full"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_blocks_against_the_unfused_kernel_route(cuda, knob, name, dt):
    """The criterion of tests/test_weight_only_fused_gpu.py::test_blocks_against_the_unfused_kernel_route, unchanged: every
    block teacher-forced with its input of a knobs-off fp32 evaluation; the fused route's error against the knobs-off fp32
    output of the block (as a fraction of its range) is at most twice the error of the unfused kernel route — the route before
    this knob, run here on the same input with the same attention knob — with a floor of one ulp of the operand type
    (2^-10 / 2^-7) of the range.  Exactly one counter increment per block.  With the attention knob off and on."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    blocks = _ddim_blocks(qnn)
    assert blocks
    rec, hooks = {}, []
    for n, b in blocks:
        hooks.append(b.register_forward_pre_hook(lambda m, a, k, n=n: rec.__setitem__(n, [a, k, None]), with_kwargs=True))
        hooks.append(b.register_forward_hook(lambda m, a, o, n=n: rec[n].__setitem__(2, o)))
    knob.set_weight_only_kernel(None)
    knob.set_weight_only_attention(None)
    knob.set_weight_only_fusion(False)
    knob.set_weight_only_fusion_ddim(False)
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
        for n, b in blocks:
            a, k, ref = rec[n]
            rng = ref.abs().max().item()
            with torch.no_grad():
                knob.set_weight_only_fusion_ddim(False)
                _reset(knob)
                e0 = (b(*a, **k) - ref).abs().max().item() / rng
                assert sum(knob.WONLY_FUSED.values()) == 0
                knob.set_weight_only_fusion_ddim(True)
                n0 = knob.ATTN_H16_LAUNCHES
                y = b(*a, **k)
                e1 = (y - ref).abs().max().item() / rng
            kind = "attnblock_ddim" if hasattr(b, "proj_out") else "resnetblock"
            assert {k_: v for k_, v in knob.WONLY_FUSED.items() if v} == {kind: 1}, f"{n} did not take the fused route"
            assert knob.ATTN_H16_LAUNCHES - n0 == (1 if attn and kind == "attnblock_ddim" else 0)
            assert y.dtype == ref.dtype and y.shape == ref.shape
            print(f"[block-parity] {name} {str(dt)[6:]} attn={'on' if attn else 'off'} {n} ({type(b).__name__}): "
                  f"unfused {e0:.3e} fused {e1:.3e} of range (bound {max(2 * e0, floor):.3e})")
            if e1 > max(2 * e0, floor):
                bad.append((n, attn, e0, e1))
    assert not bad, bad


# ---- 3. whole UNets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cifar_tiny", "cifar_full"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("attn", [False, True], ids=["libattn", "attn"])
def test_cifar_unet_matches_reference(cuda, knob, name, dt, attn):
    """State (True, False), every weights-only knob on, against the reference's weights-only golden `out_w`, inside
    tests/test_weight_only_gpu.py's BOUNDS (the project's numbers over these same models); the counters equal the block
    census; two runs bit-equal; the knob-off figures are printed beside."""
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_attention(dt if attn else None)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_ddim(False)
    _reset(knob)
    n0 = knob.ATTN_H16_LAUNCHES
    y_off = _run(qnn, fx, cuda)
    assert dict(knob.WONLY_FUSED) == {"resblock": 0, "transformer": 0} and knob.ATTN_H16_LAUNCHES == n0
    knob.set_weight_only_fusion_ddim(True)
    y = _run(qnn, fx, cuda)
    took = dict(knob.WONLY_FUSED)
    launches = knob.ATTN_H16_LAUNCHES - n0
    y2 = _run(qnn, fx, cuda)
    want = _census(qnn)
    d, cos = _metrics(y, fx["out_w"])
    d0, cos0 = _metrics(y_off, fx["out_w"])
    print(f"\n[{name}] DDIM route {dt} attn={attn}: {took}, {d:.3e} of range, cosine {cos:.7f} (knob off: {d0:.3e}, {cos0:.7f})")
    assert took == want and launches == (want["attnblock_ddim"] if attn else 0)
    assert y.dtype == torch.float32 and y.shape == y_off.shape and torch.equal(y, y2)
    tol, cmin = BOUNDS[dt]
    assert d <= tol and cos >= cmin


def test_packed_checkpoint_runs_the_route_bit_identically(cuda, knob):
    """save_packed_ckpt -> load_packed_ckpt(free_weights=True) into a model whose fp32 weights differ: the route gives the
    source model's output bit for bit."""
    import tempfile
    import qdiff
    from golden_util import build_engine_model, quant_params
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    fx = load_fixture("model_cifar_tiny.pt")
    src = _resume(fx, cuda)
    knob.set_weight_only_kernel(torch.float16)
    knob.set_weight_only_attention(torch.float16)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_ddim(True)
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
    assert dict(knob.WONLY_FUSED) == n_src == _census(src)
    assert torch.equal(y, y_src)


# ---- 4. other model families ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ldm_tiny", "sd_tiny"])
def test_other_families_are_untouched(cuda, knob, name):
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob.set_weight_only_kernel(torch.float16)
    knob.set_weight_only_attention(torch.float16)
    knob.set_weight_only_fusion(True)
    runs = []
    for on in (False, True):
        knob.set_weight_only_fusion_ddim(on)
        _reset(knob)
        runs.append((_run(qnn, fx, cuda), dict(knob.WONLY_FUSED)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert not any(k in runs[1][1] for k in ("resnetblock", "attnblock_ddim", "head_ddim"))
