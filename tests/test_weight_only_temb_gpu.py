"""One-launch embedding Linears of the weights-only state (engine.WEIGHT_ONLY_TEMB, qd_temb_mlp_wq_h16) on the GPU.

1. The kernel against the fp64 contraction of the SAME rounded operands: reference and bound are
   tests/test_weight_only_gpu.py::_contraction_ref (kind="linear"), the operand is r(silu_fp64(x)) with r the one correctly
   rounded conversion to fp16 / bf16.  The kernel evaluates SiLU in fp32, so an element whose fp64 SiLU lies within 2^-21
   (relative) of a rounding boundary of the operand type may land on the neighbouring operand value: for those elements
   ulp_operand(x^_k) * |w_kn| is added to the tolerance of the outputs they feed.  Nothing else is widened.
2. Columns outside every layer's slice stay untouched; value edges (0, exp overflow, 1e4, a constant row); a reference with
   z + 1 misses the bound.
3. Whole UNets, teacher-forced: inside BOUNDS of tests/test_weight_only_gpu.py against the golden `out_w`, no further from the
   knob-off output than that is from the golden, three launches per evaluation, no embedding contraction left in the census of
   qd_conv2d_wq_h16, knob off bit-equal run to run with a silent counter.
4. A packed checkpoint with freed weights gives the bytes of the live model.
"""
import os
import random
import tempfile
from types import SimpleNamespace as NS

import pytest
import torch

from golden_util import build_engine_model, load_fixture, quant_params
from test_weight_only_gpu import BOUNDS, _contraction_ref, _metrics, _resume, _run, _wquant

pytestmark = pytest.mark.gpu


@pytest.fixture
def knobs():
    from qdiff import engine
    names = ("WEIGHT_ONLY_KERNEL", "WEIGHT_ONLY_ATTN", "WEIGHT_ONLY_FUSE", "WEIGHT_ONLY_FUSE_WIDE", "WEIGHT_ONLY_FUSE_MOD",
             "WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_SPLITK", "WEIGHT_ONLY_TEMB")
    prev = {n: getattr(engine, n) for n in names}
    fused = dict(engine.WONLY_FUSED)
    yield engine
    for n, v in prev.items():
        setattr(engine, n, v)
    engine.WONLY_FUSED.clear()                         # (the fused routes add their keys on first use: other tests compare the dict)
    engine.WONLY_FUSED.update(fused)


def _all_knobs(engine, dt, on):
    engine.set_weight_only_kernel(dt)
    engine.set_weight_only_attention(dt if on else None)
    for f in (engine.set_weight_only_fusion, engine.set_weight_only_fusion_wide, engine.set_weight_only_fusion_mod,
              engine.set_weight_only_fusion_ddim, engine.set_weight_only_splitk):
        f(on)


# ---- the operand: one correctly rounded conversion of an fp64 value ----------------------------------------------------------
def _ulp(v, act):
    """Spacing of the operand type at |v| (fp64 tensors): 2^(e - p) with the subnormal floor."""
    p, emin = (10, -14) if act == torch.float16 else (7, -126)
    e = torch.frexp(v.abs())[1] - 1                                   # |v| in [2^e, 2^(e+1))
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v), e - p)


def _round_op(v, act):
    """(r(v), ulp at v, distance of v from the nearest rounding boundary) for fp64 v; round to nearest even."""
    u = _ulp(v, act)
    q = v / u                                                          # exact: a power of two
    r = torch.round(q) * u                                             # torch.round: half to even
    frac = q - torch.floor(q)
    return r, u, (frac - 0.5).abs() * u


def _silu64(x):
    return x / (1 + torch.exp(-x))


def _layers(g, K, couts, wbits, zmode, has_bias):
    ws = [torch.randn(c, K, generator=g) * 0.1 for c in couts]
    qs = [_wquant(w, wbits, zmode, g) for w in ws]
    bs = [torch.randn(c, generator=g) if has_bias else None for c in couts]
    return ws, qs, bs


def _launch(dev, x, ws, qs, bs, wbits, act, silu, ldx_extra=0, tail=0):
    """One launch of the layers on x [B][K] (fp32): (out [B][tot + tail] prefilled with NaN, offsets)."""
    from qdiff import engine, hip
    B, K = x.shape
    plans, offs, tot = [], [], 0
    for w, q, b in zip(ws, qs, bs):
        pack = engine.pack_module_weights(w.to(dev), [NS(**{**vars(q), "delta": q.delta.to(dev), "zero_point": q.zero_point.to(dev)})], 0)
        plan = engine.build_wonly_plan(pack, 1, 1, 1, 0, None if b is None else b.to(dev), act)
        assert plan is not None
        plans.append(plan)
        offs.append(tot)
        tot += (w.shape[0] + 63) // 64 * 64
    xd = torch.zeros(B, K + ldx_extra, device=dev)
    xd[:, :K] = x.to(dev)
    out = torch.full((B, tot + tail), float("nan"), device=dev)
    n0 = engine.WONLY_TEMB[0]
    hip.temb_mlp_wq_h16(xd[:, :K], silu, plans, offs, out, act)
    torch.cuda.synchronize()
    assert engine.WONLY_TEMB[0] == n0 + 1
    return out.cpu(), offs


def _check(x, ws, qs, bs, act, silu, out, offs, zshift=0):
    """Worst error / bound over the layers; asserts the guard columns and finiteness.  zshift: a deliberately wrong zero point
    in the REFERENCE."""
    v = x.double()
    if silu:
        v = _silu64(v)
    xr, u, dist = _round_op(v, act)
    near = (dist <= 2.0 ** -21 * v.abs()) if silu else torch.zeros_like(v, dtype=torch.bool)
    worst, seen = 0.0, torch.zeros(out.shape[1], dtype=torch.bool)
    for w, q, b, off in zip(ws, qs, bs, offs):
        Cout = w.shape[0]
        ref, tol, wq = _contraction_ref("linear", xr[None], w, [q], [(0, w.shape[1])], b, None, torch.float64, torch.float32, 1, 0)
        if zshift:                                                     # the same codes against z + zshift
            ref = ref - zshift * xr.sum(1, keepdim=True) * q.delta.double().view(1, -1)
        tol = tol + (near.double() * u) @ wq.abs().t()
        got = out[:, off:off + Cout].double()
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        worst = max(worst, ratio.max().item())
        seen[off:off + Cout] = True
    assert torch.isnan(out[:, ~seen]).all(), "a column outside every slice was written"
    return worst


def _case(dev, K, couts, B, wbits, act, silu, has_bias, ldx_extra, zmode, seed, x=None):
    g = torch.Generator().manual_seed(seed)
    ws, qs, bs = _layers(g, K, couts, wbits, zmode, has_bias)
    if x is None:
        x = torch.randn(B, K, generator=g) * 2
    out, offs = _launch(dev, x, ws, qs, bs, wbits, act, silu, ldx_extra, tail=(seed % 3) * 8)
    worst = _check(x, ws, qs, bs, act, silu, out, offs)
    print(f"\nW{wbits} {act} silu={silu} K={K} Cout={couts} B={B} bias={has_bias} ldx+{ldx_extra} z={zmode}: worst error {worst:.3g} x the bound")
    assert worst <= 1.0
    return x, ws, qs, bs, out, offs


KS, COUTS, BS = [16, 48, 64, 80, 128, 896, 1280], [1, 20, 63, 64, 65, 130, 320], [1, 3, 17, 64, 130]


def _zmode(wbits, act, edges):
    # 8-bit codes with zero points outside the code range exceed |q - z| = 256: not a bf16 layer (the plan refuses it)
    return "edges" if edges and not (wbits == 8 and act == torch.bfloat16) else "range"


def _draws(n=60):
    rnd = random.Random(4321)
    cases = []
    for i in range(n):
        wbits = 4 if i % 2 == 0 else 8
        act = torch.float16 if (i // 2) % 2 == 0 else torch.bfloat16
        nl = [1, 2, 5][i % 3]
        cases.append((rnd.choice(KS), tuple(rnd.choice(COUTS) for _ in range(nl)), rnd.choice(BS), wbits, act, i % 5 != 0, i % 3 != 1,
                      rnd.choice([0, 0, 4, 36]), _zmode(wbits, act, i % 4 == 3), 500 + i))
    return cases


def _grid():
    cases = []
    shapes = [(16, (1,), 1), (48, (63, 64, 65), 3), (64, (20, 65), 17), (80, (130, 20), 17), (128, (64,), 64), (896, (320,), 64),
              (1280, (320, 64, 1, 65, 130), 130)]
    for j, (wbits, act) in enumerate([(4, torch.float16), (4, torch.bfloat16), (8, torch.float16), (8, torch.bfloat16)]):
        for i, (K, couts, B) in enumerate(shapes):
            cases.append((K, couts, B, wbits, act, True, (i + j) % 2 == 0, 4 * ((i + j) % 3), _zmode(wbits, act, True), 900 + 10 * j + i))
    return cases


_ID = lambda c: f"K{c[0]}-C{'_'.join(map(str, c[1]))}-B{c[2]}-W{c[3]}-{str(c[4])[6:]}-silu{int(c[5])}-b{int(c[6])}-{c[-1]}"


@pytest.mark.parametrize("case", _draws() + _grid(), ids=_ID)
def test_kernel_matches_fp64_on_rounded_operands(cuda, case):
    _case(cuda, *case)


@pytest.mark.parametrize("wbits,act", [(4, torch.float16), (4, torch.bfloat16), (8, torch.float16), (8, torch.bfloat16)])
def test_value_edges(cuda, wbits, act):
    """x = 0; x = -100 (exp(100) overflows to +inf in fp32: the operand is -0, never NaN); |x| up to 1e4; a constant row."""
    K, couts = 80, (65, 20)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(7, K, generator=g)
    x[0] = 0
    x[1] = -100
    x[2] = torch.randn(K, generator=g) * 1e4 / 4
    x[2, :4] = torch.tensor([1e4, -1e4, 9999.5, -88.0])
    x[3] = 1.2345
    x[4] = -20 + torch.randn(K, generator=g)                           # SiLU values around the fp16 subnormal range
    for silu in (True, False):
        for has_bias in (False, True):
            _, ws, qs, bs, out, offs = _case(cuda, K, couts, 7, wbits, act, silu, has_bias, 4, _zmode(wbits, act, True), 31, x=x)
            for w, b, off in zip(ws, bs, offs):
                row0 = out[0, off:off + w.shape[0]]
                assert torch.equal(row0, torch.zeros_like(row0) if b is None else b)          # 0 * (q - z) * delta + bias, exactly
                if silu:
                    row1 = out[1, off:off + w.shape[0]]
                    assert not torch.isnan(row1).any() and torch.equal(row1, row0)           # -0 operands: +-0 (+ bias)


def test_wrong_zero_point_has_teeth(cuda):
    """The same draw against a reference whose zero points are one off misses the bound by orders of magnitude."""
    for wbits, act in ((4, torch.float16), (8, torch.bfloat16)):
        g = torch.Generator().manual_seed(5)
        ws, qs, bs = _layers(g, 128, (64, 20), wbits, "range", True)
        x = torch.randn(17, 128, generator=g) * 2
        out, offs = _launch(cuda, x, ws, qs, bs, wbits, act, True)
        assert _check(x, ws, qs, bs, act, True, out, offs) <= 1.0
        bad = _check(x, ws, qs, bs, act, True, out, offs, zshift=1)
        print(f"\nW{wbits} {act}: reference with z + 1 misses the bound {bad:.3g} times")
        assert bad > 100


def test_more_rows_than_one_group_holds_are_the_same_rows(cuda):
    """B = 130 runs as five 32-row tiles: every row equals the same row launched with other neighbours at another place of
    its tile (rows are independent; the accumulation order does not depend on the row's position)."""
    g = torch.Generator().manual_seed(9)
    ws, qs, bs = _layers(g, 1280, (65, 320), 4, "range", True)
    x = torch.randn(130, 1280, generator=g)
    out, offs = _launch(cuda, x, ws, qs, bs, 4, torch.float16, True)
    part, _ = _launch(cuda, x[100:103], ws, qs, bs, 4, torch.float16, True)
    for w, off in zip(ws, offs):
        assert torch.equal(out[100:103, off:off + w.shape[0]], part[:, off:off + w.shape[0]])


@pytest.mark.parametrize("wbits,act", [(4, torch.float16), (4, torch.bfloat16), (8, torch.float16), (8, torch.bfloat16)])
def test_kernel_equals_the_generic_contraction_bit_for_bit(cuda, knobs, wbits, act):
    """The launch against what it replaces — torch SiLU, qd_rows_to_h16, unsplit qd_conv2d_wq_h16 per layer — torch.equal: the
    kernel accumulates every output element with the same instruction in the same K order.  K with a ragged last K-step, row
    tiles with a tail, channel tiles with a tail, with and without SiLU and bias."""
    from qdiff import engine, hip
    import torch.nn.functional as F
    knobs.set_weight_only_splitk(False)
    for K, couts, B, silu, has_bias, seed in ((48, (63, 65), 3, True, True, 1), (1280, (320, 1, 130), 70, True, False, 2),
                                              (80, (20,), 33, False, True, 3), (896, (64, 320), 64, True, True, 4)):
        g = torch.Generator().manual_seed(seed)
        ws, qs, bs = _layers(g, K, couts, wbits, "range", has_bias)
        x = torch.randn(B, K, generator=g) * 2
        out, offs = _launch(cuda, x, ws, qs, bs, wbits, act, silu)
        xd = x.to(cuda)
        xs = F.silu(xd) if silu else xd
        for w, q, b, off in zip(ws, qs, bs, offs):
            pack = engine.pack_module_weights(w.to(cuda), [NS(**{**vars(q), "delta": q.delta.to(cuda), "zero_point": q.zero_point.to(cuda)})], 0)
            plan = engine.build_wonly_plan(pack, 1, 1, 1, 0, None if b is None else b.to(cuda), act)
            xh = engine.wonly_rows(xs, plan, 1, K, B, (0, 1, xs.stride(0)))
            ref = engine.wonly_forward(plan, xh, 1, 1, B, 1, B).cpu()
            assert torch.equal(out[:, off:off + w.shape[0]], ref), (K, couts, B, silu, has_bias)


# ---- the route ----------------------------------------------------------------------------------------------------------------
NAMES = ["cifar_tiny", "ldm_tiny", "sd_tiny", "ldm_updown_tiny"]


def _emb_linears(qnn):
    from qdiff.quant_block import QuantResBlock, QuantResnetBlock
    lins = []
    for m in qnn.modules():
        if isinstance(m, QuantResBlock):
            lins.append(m.emb_layers[-1])
        elif isinstance(m, QuantResnetBlock):
            lins.append(m.temb_proj)
    te = getattr(qnn.model, "time_embed", None)
    return lins + ([te[0], te[2]] if te is not None else list(qnn.model.temb.dense))


def _census(engine, monkeypatch, qnn, fx, dev, temb):
    """(output, Counter of weight pointers seen by hip.conv2d_wq_h16, qd_temb_mlp_wq_h16 launches) of one evaluation."""
    from collections import Counter
    from qdiff import hip
    seen = []
    inner = hip.conv2d_wq_h16
    monkeypatch.setattr(hip, "conv2d_wq_h16", lambda c, dt: (seen.append(c.w.data_ptr()), inner(c, dt))[1])
    engine.set_weight_only_temb(temb)
    n0 = engine.WONLY_TEMB[0]
    try:
        y = _run(qnn, fx, dev)
    finally:
        monkeypatch.setattr(hip, "conv2d_wq_h16", inner)
    return y, Counter(seen), engine.WONLY_TEMB[0] - n0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_unet_route(cuda, knobs, monkeypatch, name, dt):
    """Layer knob alone, then every weights-only knob on (the fused block routes are the other two call sites).

    Measured on one MI355X: knob on equals knob off bit for bit in all sixteen configurations (the kernel accumulates each
    output element as the unsplit qd_conv2d_wq_h16 does, and its SiLU is torch's), so "knob on no further from knob off than
    knob off is from the golden" holds with 0 against 5.7e-4 .. 1.05e-3 (fp16) and 4.9e-3 .. 8.8e-3 (bf16) of range.  An
    earlier form of the kernel that summed in another order (fp32 FMA chains) moved the embedding by 1e-7 relative and the fp16
    outputs of sd_tiny by 1.33e-3 of range, more than their 1.01e-3 from the golden: as much as any re-association of fp32
    sums moves these networks (contractions forced to two split-K slices against unsplit: 1.07e-3)."""
    engine = knobs
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    tol, cmin = BOUNDS[dt]
    further = []
    for fused in (False, True):
        _all_knobs(engine, dt, fused)
        with torch.no_grad():
            ptrs = {l.wonly_plan().pack.wq.data_ptr() for l in _emb_linears(qnn)}
        y0, w0, n0 = _census(engine, monkeypatch, qnn, fx, cuda, False)
        y0b, w0b, n0b = _census(engine, monkeypatch, qnn, fx, cuda, False)
        assert n0 == 0 and n0b == 0 and torch.equal(y0, y0b) and w0 == w0b and all(w0[p] == 1 for p in ptrs)
        y1, w1, n1 = _census(engine, monkeypatch, qnn, fx, cuda, True)
        y1b, _, _ = _census(engine, monkeypatch, qnn, fx, cuda, True)
        assert n1 == 3, f"{n1} qd_temb_mlp_wq_h16 launches"
        assert not any(p in w1 for p in ptrs) and {p: n for p, n in w0.items() if p not in ptrs} == dict(w1)
        assert torch.equal(y1, y1b) and y1.dtype == y0.dtype and y1.shape == y0.shape
        d1, cos1 = _metrics(y1, fx["out_w"])
        d0, cos0 = _metrics(y0, fx["out_w"])
        d10 = (y1 - y0).abs().max().item() / fx["out_w"].abs().max().item()
        print(f"\n[{name}] {dt} fused={fused}: knob on {d1:.3e} of range, cosine {cos1:.7f}; knob off {d0:.3e}, {cos0:.7f}; "
              f"on vs off {d10:.3e} = {d10 / d0:.3f} x (off vs golden)")
        assert d1 <= tol and cos1 >= cmin
        if d10 > d0:
            further.append((fused, d10, d0))
        y2, w2, n2 = _census(engine, monkeypatch, qnn, fx, cuda, False)
        assert n2 == 0 and torch.equal(y2, y0) and w2 == w0
    assert not further, f"knob on is further from knob off than knob off from the golden: (fused, on vs off, off vs golden) = {further}"


def test_packed_checkpoint_with_freed_weights_gives_the_same_bytes(cuda, knobs):
    import qdiff
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    engine = knobs
    fx = load_fixture("model_sd_tiny.pt")
    src = _resume(fx, cuda)
    _all_knobs(engine, torch.float16, False)
    engine.set_weight_only_temb(True)
    src.set_quant_state(True, False)
    n0 = engine.WONLY_TEMB[0]
    y_src = _run(src, fx, cuda)
    assert engine.WONLY_TEMB[0] == n0 + 3
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
    n0 = engine.WONLY_TEMB[0]
    y1 = _run(dst, fx, cuda)
    y2 = _run(dst, fx, cuda)
    assert engine.WONLY_TEMB[0] == n0 + 6
    assert torch.equal(y1, y_src) and torch.equal(y1, y2)
