"""Weights-only layers on the packed codes (engine.WEIGHT_ONLY_KERNEL, qd_conv2d_wq_h16 / qd_rows_to_h16) on the GPU.

1. The contraction against an fp64 convolution of the SAME rounded operands: x^ = x rounded to fp16 / bf16, weight
   (q - z) * delta with the packer's codes.  Bound per output element:
       |out - ref| <= K * 2^-26 * S[m][n] + 2^-22 * (|bias[n]| + |residual[m][n]| + |ref[m][n]|)
   (fp16 rows: that bound times (1 + 2^-11), plus 2^-11 |ref| + 2^-24 for the rounding to fp16)
   with S the same convolution on absolute values: a quarter ulp of S per K element, more than fp32 accumulation of exact
   products can produce, while a wrong zero point, delta, segment or tap misses it by orders of magnitude.
2. Zero points at the ends of and outside the code range; 8-bit codes with |q - z| = 256 in bf16 (exact) and one past it
   (the module keeps the library path, bit for bit).
3. Whole UNets in state (True, False) against the reference's weights-only golden `out_w`.
4. A packed checkpoint loaded into a model whose fp32 weights differ and are freed: bit-identical weights-only output.
"""
import os
import random
import tempfile
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from golden_util import build_ckpt, build_engine_model, fixture_inputs, load_fixture, quant_params

pytestmark = pytest.mark.gpu


@pytest.fixture
def knob():
    from qdiff import engine
    prev = engine.WEIGHT_ONLY_KERNEL
    yield engine.set_weight_only_kernel
    engine.set_weight_only_kernel(prev)


def _wquant(w, n_bits, zmode, g):
    """Per-channel asymmetric quantiser of w [Cout, ...]: delta from the channel range, zero points by `zmode`."""
    L = 2 ** n_bits
    flat = w.reshape(w.shape[0], -1)
    mn, mx = flat.min(1)[0].clamp(max=0), flat.max(1)[0].clamp(min=0)
    d = ((mx - mn) / (L - 1)).clamp(min=1e-8)
    z = torch.round(-mn / d)
    if zmode == "edges":           # 0, L-1, the packer's limits -128 / 255, and in-range values
        pick = torch.tensor([0, L - 1, -128, 255], dtype=torch.float32)
        z = torch.where(torch.rand(z.shape, generator=g) < 0.6, pick[torch.randint(0, 4, z.shape, generator=g)], z)
    return NS(delta=d, zero_point=z, n_bits=n_bits, n_levels=L, sym=False, alpha=None, soft_targets=False)


def _codes(w, q):
    shape = (-1,) + (1,) * (w.dim() - 1)
    return torch.clamp(torch.round(w / q.delta.view(shape)) + q.zero_point.view(shape), 0, q.n_levels - 1)


def _layer(kind, B, Cin, Cout, H, W, k, stride, g):
    if kind == "conv2d":
        return torch.randn(B, Cin, H, W, generator=g), torch.randn(Cout, Cin, k, k, generator=g) * 0.1
    if kind == "conv1d":
        return torch.randn(B, Cin, W, generator=g), torch.randn(Cout, Cin, 1, generator=g) * 0.1
    return torch.randn(B, W, Cin, generator=g), torch.randn(Cout, Cin, generator=g) * 0.1


def _fp64_conv(kind, x, w, stride, pad):
    if kind == "conv2d":
        return F.conv2d(x, w, stride=stride, padding=pad)
    if kind == "conv1d":
        return F.conv1d(x, w)
    return F.linear(x, w)


def _contraction_ref(kind, x, w, qs, bounds, bias, res, act, out_dtype, stride, pad):
    """fp64 contraction of the SAME rounded operands (x rounded to `act`, weight (q - z) * delta per segment of `bounds`) plus
    bias and residual, as rows [M, Cout], and the bound of the module docstring: (ref, tol, dequantised weight [Cout, Cin...])."""
    Cout, Cin = w.shape[0], w.shape[1]
    kh, kw = (w.shape[2], w.shape[3]) if kind == "conv2d" else (1, 1)
    xr = x.to(act).double()
    ref = torch.zeros(())
    S = torch.zeros(())
    wqs = []
    for (a, b), q in zip(bounds, qs):
        wq = ((_codes(w[:, a:b], q) - q.zero_point.view((-1,) + (1,) * (w.dim() - 1))) * q.delta.view((-1,) + (1,) * (w.dim() - 1))).double()
        wqs.append(wq)
        xs = xr[:, a:b] if kind != "linear" else xr[..., a:b]
        ref = ref + _fp64_conv(kind, xs, wq, stride, pad)
        S = S + _fp64_conv(kind, xs.abs(), wq.abs(), stride, pad)
    M = ref.numel() // Cout
    if kind == "conv2d":
        ref, S = ref.permute(0, 2, 3, 1).reshape(M, Cout), S.permute(0, 2, 3, 1).reshape(M, Cout)
    elif kind == "conv1d":
        ref, S = ref.permute(0, 2, 1).reshape(M, Cout), S.permute(0, 2, 1).reshape(M, Cout)
    else:
        ref, S = ref.reshape(M, Cout), S.reshape(M, Cout)
    extra = torch.zeros(M, Cout, dtype=torch.float64)
    if bias is not None:
        ref = ref + bias.double()
        extra = extra + bias.double().abs()
    if res is not None:
        ref = ref + res.double()
        extra = extra + res.double().abs()
    K = kh * kw * Cin
    tol = K * 2.0 ** -26 * S + 2.0 ** -22 * (extra + ref.abs())
    if out_dtype == torch.float16:                     # + the rounding of the fp32 value to fp16 (and its subnormal step)
        tol = tol * (1 + 2.0 ** -11) + 2.0 ** -11 * ref.abs() + 2.0 ** -24
    return ref, tol, torch.cat(wqs, 1)


def _run_case(dev, kind, wbits, act, out_dtype, split, B, Cin, Cout, H, W, k, stride, has_bias, has_res, zmode, seed, x=None, w=None, qs=None):
    """One launch against the fp64 bound; x, w and the per-segment quantisers qs are drawn from `seed` unless given."""
    from qdiff import engine
    g = torch.Generator().manual_seed(seed)
    if x is None:
        x, w = _layer(kind, B, Cin, Cout, H, W, k, stride, g)
    pad = k // 2 if kind == "conv2d" else 0
    bounds = [(0, Cin)] if not split else [(0, split), (split, Cin)]
    if qs is None:
        qs = [_wquant(w[:, a:b], wbits, zmode, g) for a, b in bounds]
    bias = torch.randn(Cout, generator=g) if has_bias else None
    pack = engine.pack_module_weights(w.to(dev), [NS(**{**vars(q), "delta": q.delta.to(dev), "zero_point": q.zero_point.to(dev)})
                                                   for q in qs], split or 0)
    kh, kw = (k, k) if kind == "conv2d" else (1, 1)
    plan = engine.build_wonly_plan(pack, kh, kw, stride if kind == "conv2d" else 1, pad, None if bias is None else bias.to(dev), act)
    assert plan is not None
    xd = x.to(dev)
    if kind == "conv2d":
        xd = xd.contiguous(memory_format=torch.channels_last) if seed % 2 else xd            # NCHW and channels-last producers
        sb, sc, sh, sw = xd.stride()
        xh = engine.wonly_rows(xd, plan, B, Cin, H * W, (sb, sc, sw))
        Ho, Wo = engine.conv_out_hw(H, W, plan)
        geo = (B, H, W, Ho, Wo)
    elif kind == "conv1d":
        xh = engine.wonly_rows(xd, plan, B, Cin, W, xd.stride())
        geo = (B, 1, W, 1, W)
    else:
        rows = xd.reshape(-1, Cin)
        xh = engine.wonly_rows(rows, plan, 1, Cin, rows.shape[0], (0, 1, rows.stride(0)))
        geo = (1, 1, rows.shape[0], 1, rows.shape[0])
    M = geo[0] * geo[3] * geo[4]
    res = torch.randn(M, Cout, generator=g).to(out_dtype) if has_res else None
    out = engine.wonly_forward(plan, xh, *geo, out_dtype=out_dtype, residual=None if res is None else res.to(dev))
    torch.cuda.synchronize()
    got = out.double().cpu()
    ref, tol, _ = _contraction_ref(kind, x, w, qs, bounds, bias, res, act, out_dtype, stride, pad)
    err = (got - ref).abs()
    worst = (err / tol).max().item()
    assert worst <= 1.0, (f"{kind} W{wbits} {act} -> {out_dtype} split={split} B={B} Cin={Cin} Cout={Cout} {H}x{W} k={k} s={stride}: "
                          f"error {worst:.3g} x the bound (max |err| {err.max().item():.3e})")
    return worst


def _draws(n=100):
    rnd = random.Random(1234)
    cases = []
    for i in range(n):
        kind = ["conv2d", "conv2d", "conv2d", "linear", "conv1d"][i % 5]
        wbits = 4 if i % 2 == 0 else 8
        act = torch.float16 if (i // 2) % 2 == 0 else torch.bfloat16
        out_dtype = torch.float32 if (i // 4) % 2 == 0 else torch.float16
        k, stride = (1, 1) if kind != "conv2d" else rnd.choice([(1, 1), (3, 1), (3, 2)])
        Cin = rnd.choice([8, 24, 40, 64, 72, 100, 130, 200, 320])
        Cout = rnd.choice([1, 20, 32, 48, 96, 130, 160, 260])
        split = rnd.choice([0, 0, Cin // 2 // 8 * 8 or 0, Cin // 3]) if Cin >= 16 else 0
        H, W = (rnd.randint(3, 17), rnd.randint(3, 19)) if kind == "conv2d" else (1, rnd.randint(5, 300))
        B = rnd.choice([1, 2])
        cases.append((kind, wbits, act, out_dtype, split, B, Cin, Cout, H, W, k, stride, i % 3 != 0, i % 4 == 1, "range", 100 + i))
    return cases


@pytest.mark.parametrize("case", _draws(), ids=lambda c: f"{c[0]}-W{c[1]}-{str(c[2])[6:]}-{str(c[3])[6:]}-s{c[4]}-{c[-1]}")
def test_contraction_matches_fp64_on_rounded_operands(cuda, case):
    _run_case(cuda, *case)


@pytest.mark.parametrize("wbits,act", [(4, torch.float16), (4, torch.bfloat16), (8, torch.float16)])
@pytest.mark.parametrize("kind,k,stride", [("conv2d", 3, 1), ("conv2d", 3, 2), ("linear", 1, 1)])
def test_zero_points_at_and_outside_the_code_range(cuda, wbits, act, kind, k, stride):
    """Zero points 0, n_levels - 1, -128 and 255 mixed over the channels (4-bit codes: |q - z| <= 255 even in bf16)."""
    for seed, split in ((7, 0), (8, 40)):
        _run_case(cuda, kind, wbits, act, torch.float32, split, 2, 104, 96, 9, 11, k, stride, True, True, "edges", seed)


def _w8_module(dev, zero0):
    """1x1 QuantModule (W8, per channel) whose channel 0 has zero point `zero0` and a weight at code 255."""
    import qdiff
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(64, 40, 1)
    m = qdiff.QuantModule(conv, dict(n_bits=8, channel_wise=True, scale_method="max"),
                          dict(n_bits=8, channel_wise=False, scale_method="max")).to(dev)
    m.set_quant_state(True, False)
    x = torch.randn(2, 64, 6, 6, device=dev)
    with torch.no_grad():
        m(x)                                                   # initialises the weight quantiser (library path)
        wq = m.weight_quantizer
        d = wq.delta.view(-1)[0].item()
        wq.zero_point = wq.zero_point.clone()
        wq.zero_point.view(-1)[0] = float(zero0)
        m.weight.data[0, 0] = (255 - zero0) * d               # code 255 in channel 0: |q - z| = 255 - zero0
    m.invalidate()
    return m, x


def test_bf16_code_span_256_is_exact(cuda, knob):
    """W8 with |q - z| = 256 (z = -1, q = 255) in bf16: the kernel takes the layer and is exact to the fp64 bound."""
    from qdiff import engine
    m, x = _w8_module(cuda, -1)
    knob(torch.bfloat16)
    plan = m.wonly_plan()
    assert plan is not None and engine.wonly_code_span(plan.pack) == 256
    with torch.no_grad():
        y = m(x).double().cpu()
        wq = m.weight_quantizer
        wd = ((_codes(m.weight.cpu(), NS(delta=wq.delta.view(-1).cpu(), zero_point=wq.zero_point.view(-1).cpu(), n_levels=256))
               - wq.zero_point.view(-1, 1, 1, 1).cpu()) * wq.delta.view(-1, 1, 1, 1).cpu()).double()
        xr = x.cpu().to(torch.bfloat16).double()
        ref = F.conv2d(xr, wd, m.bias.detach().cpu().double())
        S = F.conv2d(xr.abs(), wd.abs())
    tol = 64 * 2.0 ** -26 * S + 2.0 ** -22 * (m.bias.detach().cpu().double().abs().view(1, -1, 1, 1) + ref.abs())
    assert ((y - ref).abs() <= tol).all()


def test_bf16_code_span_257_keeps_the_library_path(cuda, knob):
    """One code past (z = -2, q = 255: 257 is not a bf16 integer): no plan in bf16, and the output is the library path's bit
    for bit; fp16 still takes the layer."""
    m, x = _w8_module(cuda, -2)
    with torch.no_grad():
        knob(None)
        y_lib = m(x)
        knob(torch.bfloat16)
        assert m.wonly_plan() is None and not m.wonly_ready()
        y = m(x)
        knob(torch.float16)
        assert m.wonly_ready()
    assert torch.equal(y, y_lib)


def _resume(fx, dev):
    import qdiff
    from qdiff.utils import resume_cali_model
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    qnn = qdiff.QuantModel(build_engine_model(spec).to(dev), wq, aq, sm_abit=spec["sm_abit"]).to(dev).eval()
    cal = tuple(a for a in fixture_inputs(fx, "cal") if a is not None)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ckpt.pth")
        torch.save(build_ckpt(fx), path)
        resume_cali_model(qnn, path, cal, quant_act=True, cond=spec["ctx"] is not None)
    return qnn


def _run(qnn, fx, dev, autocast=False):
    x, t, c = fixture_inputs(fx, "test")
    args = (x.to(dev), t.to(dev)) + ((c.to(dev),) if c is not None else ())
    with torch.no_grad(), torch.autocast("cuda", enabled=autocast):
        y = qnn(*args)
    torch.cuda.synchronize()
    return y


MODELS = ["cifar_tiny", "ldm_tiny", "sd_tiny", "ldm_updown_tiny", "cifar_full", "ldm_full", "sd_full", "churches_full"]
# (max |diff| / range, min cosine) against the reference's weights-only fp32 golden: 2x the worst value measured over the eight
# models on an MI355X (max |diff| = 2x, 1 - cosine = 2x), capped at the ceilings fp16 5e-3 / 0.9999, bf16 4e-2 / 0.999.
#   fp16: worst 1.008e-3 of range (sd_tiny), worst cosine 0.9999994 (sd_tiny)   -> 2.02e-3, 0.9999988
#   bf16: worst 8.308e-3 of range (sd_tiny), worst cosine 0.9999692 (sd_tiny)   -> 1.66e-2, 0.9999384
#   fp16 under autocast (the library's glue in fp16 too; ceilings of fp16): worst 1.824e-3 (sd_full), worst cosine 0.9999979
#   (sd_full) -> 3.65e-3, 0.9999958.  (The kernel-off autocast run measured 1.97e-3 .. 3.25e-3 of range on the same models.)
BOUNDS = {torch.float16: (2.02e-3, 0.9999988), torch.bfloat16: (1.66e-2, 0.9999384), "autocast": (3.65e-3, 0.9999958)}


def _metrics(y, ref):
    rng = ref.abs().max().item()
    d = (y.float().cpu() - ref).abs().max().item() / rng
    return d, F.cosine_similarity(y.float().cpu().flatten(), ref.flatten(), dim=0).item()


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_weight_only_unet_matches_reference(cuda, knob, name, dt):
    """Whole UNets in state (True, False) with the kernel on vs the reference's weights-only golden `out_w` (bounds: BOUNDS)."""
    import qdiff
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob(dt)
    mods = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)]
    with torch.no_grad():
        taken = sum(m.wonly_ready() for m in mods)
    assert not any(m.int_ready() for m in mods)
    assert taken == len(mods), f"only {taken} of {len(mods)} layers take the weights-only kernel"
    y = _run(qnn, fx, cuda)
    assert y.dtype == torch.float32
    d, cos = _metrics(y, fx["out_w"])
    print(f"\n[{name}] weights-only {dt}: {taken}/{len(mods)} layers on the kernel, {d:.3e} of range, cosine {cos:.7f}")
    tol, cmin = BOUNDS[dt]
    assert d <= tol and cos >= cmin


@pytest.mark.parametrize("name", MODELS)
def test_weight_only_unet_under_autocast(cuda, knob, name):
    """The fp16 case under torch.autocast("cuda"): every kernel-run layer returns fp16 (what the library convolution returns
    there), the model returns what it returns with the kernel off, and the output stays within BOUNDS["autocast"]."""
    import qdiff
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob(None)
    y_lib = _run(qnn, fx, cuda, autocast=True)
    knob(torch.float16)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, a, out: seen.append(out.dtype)) for m in qnn.modules() if isinstance(m, qdiff.QuantModule)]
    try:
        y = _run(qnn, fx, cuda, autocast=True)
    finally:
        for h in hooks:
            h.remove()
    assert seen and all(t == torch.float16 for t in seen), set(seen)
    assert y.dtype == y_lib.dtype
    d, cos = _metrics(y, fx["out_w"])
    dl, cosl = _metrics(y_lib, fx["out_w"])
    print(f"\n[{name}] weights-only fp16 under autocast: {d:.3e} of range, cosine {cos:.7f} (kernel off: {dl:.3e}, {cosl:.7f})")
    tol, cmin = BOUNDS["autocast"]
    assert d <= tol and cos >= cmin


def test_packed_checkpoint_runs_weight_only_bit_identically(cuda, knob):
    """save_packed_ckpt -> load_packed_ckpt(free_weights=True) into a model whose fp32 weights differ: with the kernel on, the
    weights-only output equals the source model's bit for bit, and two calls equal each other."""
    import qdiff
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    fx = load_fixture("model_sd_tiny.pt")
    src = _resume(fx, cuda)
    knob(torch.float16)
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
    y1 = _run(dst, fx, cuda)
    y2 = _run(dst, fx, cuda)
    assert torch.equal(y1, y_src) and torch.equal(y1, y2)
    knob(None)
    with pytest.raises(qdiff.hip.HipEngineError, match="WEIGHT_ONLY"):
        _run(dst, fx, cuda)
