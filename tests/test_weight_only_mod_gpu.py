"""The weights-only route of the scale-shift and resampling residual blocks (engine.WEIGHT_ONLY_FUSE_MOD) on the GPU: the two new
producers (qd_groupnorm_mod_h16, qd_groupnorm_resample_h16) through the wrappers of the C ABI, every covered block against today's
unfused kernel route, and whole UNets against the reference's weights-only golden output.

Exact conditions.  qd_groupnorm_mod_h16 with mod = 0 folds a' = a * 1, sh' = sh * 1 + 0: the values of qd_groupnorm_h16.
resample = 2 writes the rounded result of every input pixel to four rows: qd_groupnorm_h16's rows replicated (b, h, 2, w, 2).

Bounded conditions, per output element, against an fp64 evaluation `ref`; u = 2^-24, T the fp32 term of the GroupNorm bound of
tests/test_weight_only_fused_gpu.py (_gn_ref, imported), half ulp as there (_half_ulp):
  mod       GroupNorm with gamma' = gamma (1 + scale_b), beta' = beta (1 + scale_b) + shift_b per sample b is the same function
            of x, so _gn_ref applies with (gamma', beta').  The kernel does not form gamma' but folds the modulation into the
            per-(sample, channel) affine (a, sh) in fp32 — a' = a sc, sh' = sh sc + shift — which adds the roundings of the fold:
            |out - ref| <= half ulp + T(gamma', beta') + 2 u (|a' x| + |b'|),   b' = |sh sc| + |shift|, the magnitudes the
            folded shift is made of.
  average   each of the four post-SiLU fp32 values y_i is within T_i of its fp64 value; (y00 + y01), (y10 + y11), their sum: three
            fp32 additions, each off by at most u times its result, all of magnitude <= 4 |avg| when the signs agree (to first
            order; * 0.25 is exact):  |out - ref| <= half ulp at ref + mean(T_i) + 3 u |avg|.
Each of four mistakes — a dropped shift, scale applied without the `1 +`, the average taken before SiLU, the pool window shifted
by one column — is evaluated in fp64 on the CPU, rounded to the output type, and must MISS its bound (no GPU needed for that).
"""
import functools
import itertools
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

from block_parity_util import _engine_block
from golden_util import build_engine_model, load_fixture, quant_params
from test_weight_only_fused_gpu import GUARD, U, _gn_ref, _guarded, _half_ulp
from test_weight_only_gpu import BOUNDS, MODELS, _metrics, _resume, _run
from wonly_edge_cases import STREAM_PASS, range_ratio

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
EPS = 1e-5
DTYPES = [(F32, F16), (F16, BF16), (F32, BF16), (F16, F16)]


@pytest.fixture
def knob():
    """The engine with the weights-only knobs and the route's counter restored afterwards."""
    from qdiff import engine
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE, engine.WEIGHT_ONLY_FUSE_MOD)
    yield engine
    engine.set_weight_only_kernel(prev[0])
    engine.set_weight_only_attention(prev[1])
    engine.set_weight_only_fusion(prev[2])
    engine.set_weight_only_fusion_wide(prev[3])
    engine.set_weight_only_fusion_mod(prev[4])
    engine.WONLY_FUSED.pop("resblock_mod", None)


def _reset(engine):
    engine.WONLY_FUSED.pop("resblock_mod", None)
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0


# ---- fp64 references (CPU) -----------------------------------------------------------------------------------------------------
def _mod_ref(x, G, gamma, beta, mod, silu, variant=None):
    """x [B, S, C] -> (ref, tol term) rows [B * S, C] of GroupNorm * (1 + scale) + shift (+ SiLU).  variant: a mistaken evaluation
    ("no_shift", "no_one": scale without the 1 +) — its `ref` only."""
    B, S, C = x.shape
    refs, Ts = [], []
    for b in range(B):
        sc, sf = mod[b, :C].double(), mod[b, C:2 * C].double()
        if variant == "no_shift":
            sf = torch.zeros_like(sf)
        one = 0.0 if variant == "no_one" else 1.0
        g2, b2 = gamma.double() * (one + sc), beta.double() * (one + sc) + sf
        ref, T = _gn_ref(x[b:b + 1], G, g2, b2, EPS, silu)
        xd = x[b].double().view(S, G, C // G)
        m, var = xd.mean((0, 2), keepdim=True), xd.var((0, 2), unbiased=False, keepdim=True)
        a = (gamma.double().view(1, G, -1) / torch.sqrt(var + EPS))
        sh = beta.double().view(1, G, -1) - m * a
        scg, sfg = (1 + sc).view(1, G, -1), sf.view(1, G, -1)
        extra = 2 * U * ((a * scg * xd).abs() + (sh * scg).abs() + sfg.abs())
        refs.append(ref)
        Ts.append(T + extra.reshape(S, C))
    return torch.cat(refs), torch.cat(Ts)


def _avg4(y, B, H, W, C, shift=0):
    """rows [B * H * W, C] -> ((y00 + y01) + (y10 + y11)) / 4 as rows [B * H/2 * W/2, C]; shift: the window moved by `shift` columns."""
    y = y.view(B, H, W, C)
    if shift:
        y = torch.roll(y, -shift, dims=2)
    return (((y[:, 0::2, 0::2] + y[:, 0::2, 1::2]) + (y[:, 1::2, 0::2] + y[:, 1::2, 1::2])) * 0.25).reshape(-1, C)


def _down_ref(x, B, H, W, G, gamma, beta, silu, variant=None):
    """x [B, H * W, C] -> (ref, tol term) of the 2x2 average of GroupNorm (+ SiLU).  variant "pre_silu": SiLU of the average of
    the pre-activations; "shifted": the window one column to the right — `ref` only."""
    C = x.shape[2]
    if variant == "pre_silu":
        pre, _ = _gn_ref(x, G, gamma, beta, EPS, False)
        a = _avg4(pre, B, H, W, C)
        return a * torch.sigmoid(a), None
    y, T = _gn_ref(x, G, gamma, beta, EPS, silu)
    ref = _avg4(y, B, H, W, C, shift=1 if variant == "shifted" else 0)
    return ref, _avg4(T, B, H, W, C) + 3 * U * ref.abs()


@functools.lru_cache(maxsize=None)
def _draw(B, H, W, C, xdt, seed=0):
    """One shared, unchanged draw per shape and input type: x [B, H * W, C], gamma, beta, mod [B, 2 C + 8]."""
    g = torch.Generator().manual_seed(9000 + 131 * B + 17 * H + 7 * W + C + seed)
    x = (torch.randn(B, H * W, C, generator=g) * (0.3 + 2 * torch.rand(1, 1, C, generator=g)) + 0.5 * torch.randn(B, 1, C, generator=g)).to(xdt)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    mod = 0.5 * torch.randn(B, 2 * C + 8, generator=g)
    return x, gamma, beta, mod


# ---- launches ------------------------------------------------------------------------------------------------------------------
def _dev_rows(x, dev, xpad):
    """CPU [B, S, C] -> device rows [B * S][C + xpad] (ldx > C when xpad), the pad columns holding a value no output may show."""
    B, S, C = x.shape
    buf = torch.full((B * S, C + xpad), 3e4, dtype=x.dtype, device=dev)
    buf[:, :C] = x.view(B * S, C).to(dev)
    return buf


def _launch(dev, kind, x, B, H, W, G, gamma, beta, odt, pad, xpad, silu=True, mod=None):
    """kind: "plain" | "mod" | "down" | "up" -> (guarded buffer, rows)."""
    from qdiff import hip
    C = x.shape[2]
    S = H * W
    xr = _dev_rows(x, dev, xpad)
    M = B * S // 4 if kind == "down" else B * S * 4 if kind == "up" else B * S
    buf, out = _guarded(M, C + pad, odt, dev)
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=dev)
    gm, bt = gamma.to(dev), beta.to(dev)
    if kind == "plain":
        hip.groupnorm_h16(xr, B, S, C, C + xpad, G, EPS, gm, bt, silu, out, C + pad, ws)
    elif kind == "mod":
        md = mod.to(dev)
        hip.groupnorm_mod_h16(xr, B, S, C, C + xpad, G, EPS, gm, bt, md, md.stride(0), silu, out, C + pad, ws)
    else:
        hip.groupnorm_resample_h16(xr, B, H, W, C, C + xpad, G, EPS, gm, bt, silu, 1 if kind == "down" else 2, out, C + pad, ws)
    torch.cuda.synchronize()
    return buf, out


def _guards_ok(buf, out, C, what):
    assert (buf[:GUARD] == 7.5).all() and (buf[-GUARD:] == 7.5).all(), f"{what}: rows outside [0, M) were written"
    assert (out[:, C:] == 0).all(), f"{what}: pad columns are not zero"


def _replicate(rows, B, H, W):
    return rows.view(B, H, 1, W, 1, rows.shape[1]).expand(B, H, 2, W, 2, rows.shape[1]).reshape(-1, rows.shape[1])


SHAPES = list(itertools.product([1, 3], [(2, 2), (4, 6), (8, 8), (6, 10)], [32, 64, 96, 192]))


@pytest.mark.parametrize("B,hw,C", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_producers_match_fp64_and_the_exact_conditions(cuda, B, hw, C):
    H, W = hw
    G = 32
    i = SHAPES.index((B, hw, C))
    for j, (xdt, odt) in enumerate(DTYPES):
        silu = (i + j) % 3 != 2
        x, gamma, beta, mod = _draw(B, H, W, C, xdt)
        pad, xpad = (8, 8) if (i + j) % 2 == 0 else (24, 16)
        what = f"B={B} {H}x{W} C={C} {xdt}->{odt} silu={silu}"
        bufp, plain = _launch(cuda, "plain", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu)
        # mod = 0: the values of qd_groupnorm_h16
        bufz, modz = _launch(cuda, "mod", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu, mod=torch.zeros_like(mod))
        _guards_ok(bufz, modz, C, what + " mod0")
        assert torch.equal(modz, plain), what + ": mod = 0 differs from qd_groupnorm_h16"
        # mod against fp64, twice bit-equal
        bufm, outm = _launch(cuda, "mod", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu, mod=mod)
        _guards_ok(bufm, outm, C, what + " mod")
        assert torch.equal(bufm.view(torch.int16), _launch(cuda, "mod", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu, mod=mod)[0].view(torch.int16))
        ref, T = _mod_ref(x, G, gamma, beta, mod, silu)
        tol = _half_ulp(ref, odt) + T
        wm = ((outm[:, :C].double().cpu() - ref).abs() / tol).max().item()
        for v in ("no_shift", "no_one"):
            wrong = _mod_ref(x, G, gamma, beta, mod, silu, variant=v)[0].to(odt).double()
            assert ((wrong - ref).abs() / tol).max().item() > 1.0, f"{what}: the mistake {v} passes the bound"
        # nearest 2x: the rows of qd_groupnorm_h16 replicated
        bufu, up = _launch(cuda, "up", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu)
        _guards_ok(bufu, up, C, what + " up")
        assert torch.equal(up, _replicate(plain, B, H, W)), what + ": nearest 2x differs from the replicated rows"
        assert torch.equal(bufu.view(torch.int16), _launch(cuda, "up", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu)[0].view(torch.int16))
        # 2x2 average against fp64
        bufd, down = _launch(cuda, "down", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu)
        _guards_ok(bufd, down, C, what + " down")
        assert torch.equal(bufd.view(torch.int16), _launch(cuda, "down", x, B, H, W, G, gamma, beta, odt, pad, xpad, silu)[0].view(torch.int16))
        refd, Td = _down_ref(x, B, H, W, G, gamma, beta, silu)
        told = _half_ulp(refd, odt) + Td
        wd = ((down[:, :C].double().cpu() - refd).abs() / told).max().item()
        if W > 2:
            wrong = _down_ref(x, B, H, W, G, gamma, beta, silu, variant="shifted")[0].to(odt).double()
            assert ((wrong - refd).abs() / told).max().item() > 1.0, f"{what}: a window shifted by one column passes the bound"
        if silu:
            wrong = _down_ref(x, B, H, W, G, gamma, beta, silu, variant="pre_silu")[0].to(odt).double()
            assert ((wrong - refd).abs() / told).max().item() > 1.0, f"{what}: the average before SiLU passes the bound"
        print(f"\n{what}: mod {wm:.3f} x bound, average {wd:.3f} x bound")
        assert wm <= 1.0 and wd <= 1.0


@pytest.mark.parametrize("kind", ["down", "up"])
@pytest.mark.parametrize("xdt,odt", [(F32, F16), (F16, BF16)], ids=["f32-f16", "f16-bf16"])
def test_resample_past_one_grid_stride_trip(cuda, kind, xdt, odt):
    """C = 8 in rows of ldo = 64 (eight chunks a row, seven of them pad): more than STREAM_PASS chunks, so the kernel's loop takes
    a second trip, which starts inside a sample."""
    C, G, pad = 8, 2, 56
    B, H, W = (5, 460, 460) if kind == "down" else (5, 230, 230)
    rows_thread = B * H * W // 4 if kind == "down" else B * H * W
    assert STREAM_PASS < rows_thread * (C + pad) // 8 < 2 * STREAM_PASS and STREAM_PASS % ((C + pad) // 8 * (rows_thread // B)) != 0
    x, gamma, beta, _ = _draw(B, H, W, C, xdt)
    buf, out = _launch(cuda, kind, x, B, H, W, G, gamma, beta, odt, pad, 8)
    _guards_ok(buf, out, C, f"long {kind}")
    if kind == "up":
        plain = _launch(cuda, "plain", x, B, H, W, G, gamma, beta, odt, pad, 8)[1]
        assert torch.equal(out, _replicate(plain, B, H, W))
        return
    ref, T = _down_ref(x, B, H, W, G, gamma, beta, True)
    r = (out[:, :C].double().cpu() - ref).abs() / (_half_ulp(ref, odt) + T)
    first2 = STREAM_PASS // ((C + pad) // 8)
    print(f"\nlong down {xdt}->{odt}: first trip {r[:first2].max().item():.3f}, second trip {r[first2:].max().item():.3f} x bound")
    assert r.max().item() <= 1.0


# ---- value edges ---------------------------------------------------------------------------------------------------------------
EDGES = ["const_groups", "offset", "past_fp16", "scale_minus_one"]


def _edge_case(kd, xdt):
    B, H, W, C, G = 2, 4, 6, 64, 8
    x, gamma, beta, mod = _draw(B, H, W, C, F32, seed=1)
    x, gamma, beta, mod = x.clone(), gamma.clone(), beta.clone(), mod.clone()
    grp = torch.arange(C) // (C // G)
    if kd == "const_groups":                       # zero variance in every group of sample 0
        x[0] = torch.tensor([0.0, 3.0, -1024.0, 0.5, -7.25, 100.0, 1e-3, -0.0])[grp]
    elif kd == "offset":                           # mean >> std
        x = x + torch.tensor([1e2, 1e3, -1e2, -1e3, 0, 1e3, 1e2, 0])[grp]
    elif kd == "past_fp16":                        # results past 65504 on every third channel
        gamma[::3] = 1e5
    elif kd == "scale_minus_one":                  # the norm is switched off: the result is the shift
        mod[:, :C] = -1.0
    return x.to(xdt), gamma, beta, mod, (B, H, W, C, G)


@pytest.mark.parametrize("kd", EDGES)
@pytest.mark.parametrize("xdt,odt", [(F32, F16), (F16, BF16), (F32, BF16)], ids=["f32-f16", "f16-bf16", "f32-bf16"])
def test_value_edges(cuda, kd, xdt, odt):
    x, gamma, beta, mod, (B, H, W, C, G) = _edge_case(kd, xdt)
    for silu in (True, False):
        plain = _launch(cuda, "plain", x, B, H, W, G, gamma, beta, odt, 8, 8, silu)[1]
        bufm, outm = _launch(cuda, "mod", x, B, H, W, G, gamma, beta, odt, 8, 8, silu, mod=mod)
        bufd, down = _launch(cuda, "down", x, B, H, W, G, gamma, beta, odt, 8, 8, silu)
        bufu, up = _launch(cuda, "up", x, B, H, W, G, gamma, beta, odt, 8, 8, silu)
        for b_, o_, w_ in ((bufm, outm, "mod"), (bufd, down, "down"), (bufu, up, "up")):
            _guards_ok(b_, o_, C, f"{kd} {w_}")
        assert torch.equal(up.view(torch.int16), _replicate(plain, B, H, W).view(torch.int16))      # bits: infinities and zeros alike
        ref, T = _mod_ref(x, G, gamma, beta, mod, silu)
        wm = range_ratio(outm[:, :C].cpu(), ref, _half_ulp(ref, odt) + T, odt)
        refd, Td = _down_ref(x, B, H, W, G, gamma, beta, silu)
        wd = range_ratio(down[:, :C].cpu(), refd, _half_ulp(refd, odt) + Td, odt)
        print(f"\nedge {kd} {xdt}->{odt} silu={silu}: mod {wm:.3f}, average {wd:.3f} x bound")
        assert wm <= 1.0 and wd <= 1.0
        if kd == "scale_minus_one":               # a' = a * 0, sh' = sh * 0 + shift: exactly the shift (+ SiLU), whatever the input
            sf = mod[:, C:2 * C].to(cuda)
            want = (sf * (1.0 / (1.0 + torch.exp(-sf))) if silu else sf)
            got = outm[:, :C].float().view(B, H * W, C)
            assert (got == got[:, :1]).all() and (got[:, 0].double() - want.double()).abs().max() <= (_half_ulp(want.double(), odt) + 8 * U * want.abs().double()).max()
        if kd == "past_fp16" and odt == F16:
            assert torch.isinf(outm.float()).any() and torch.isinf(down.float()).any()


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def _kind(b):
    k = "plain" if not b.updown else ("down" if hasattr(b.h_upd, "op") else "up")
    return k + ("+ss" if b.use_scale_shift_norm else "")


def _sample(blocks, rec, every):
    """every: all blocks; else one block per (kind, input resolution)."""
    if every:
        return blocks
    seen, out = set(), []
    for n, b in blocks:
        key = (_kind(b), rec[n][0][0].shape[2], isinstance(b.skip_connection, torch.nn.Identity))
        if key not in seen:
            seen.add(key)
            out.append((n, b))
    return out


@pytest.mark.parametrize("name", ["ldm_updown_tiny", "churches_full"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_blocks_against_the_unfused_kernel_route(cuda, knob, name, dt):
    """Residual blocks teacher-forced (block_parity_util._engine_block) with their inputs of a knobs-off fp32 evaluation — every
    block of ldm_updown_tiny, one of churches_full per kind (plain / down / up, scale-shift) and resolution: the route's error
    against the knobs-off fp32 output of the block, as a fraction of that output's range, is at most twice that of today's
    unfused kernel route on the same input, with a floor of one ulp of the operand type (2^-10 / 2^-7): the rule of DESIGN.md
    §4.14."""
    from qdiff.quant_block import QuantResBlock
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    blocks = [(n, m) for n, m in qnn.model.named_modules() if isinstance(m, QuantResBlock)]
    assert blocks and all(b.updown or b.use_scale_shift_norm for _, b in blocks)
    rec, hooks = {}, []
    for n, b in blocks:
        hooks.append(b.register_forward_pre_hook(lambda m, a, k, n=n: rec.__setitem__(n, [a, k, None]), with_kwargs=True))
        hooks.append(b.register_forward_hook(lambda m, a, o, n=n: rec[n].__setitem__(2, o)))
    knob.set_weight_only_kernel(None)
    knob.set_weight_only_attention(None)
    knob.set_weight_only_fusion(False)
    knob.set_weight_only_fusion_mod(False)
    try:
        _run(qnn, fx, cuda)
    finally:
        for h in hooks:
            h.remove()
    floor = 2.0 ** -10 if dt == F16 else 2.0 ** -7
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_fusion(True)
    bad, kinds = [], set()
    for n, b in _sample(blocks, rec, name == "ldm_updown_tiny"):
        a, k, ref = rec[n]
        inp = dict(x=a[0], emb=a[1] if len(a) > 1 else k["emb"], split=k.get("split", a[2] if len(a) > 2 else 0))
        rng = ref.abs().max().item()
        knob.set_weight_only_fusion_mod(False)
        e0 = (_engine_block(qnn, "ldm_res", n, inp, cuda) - ref).abs().max().item() / rng
        knob.set_weight_only_fusion_mod(True)
        _reset(knob)
        y = _engine_block(qnn, "ldm_res", n, inp, cuda)
        e1 = (y - ref).abs().max().item() / rng
        assert knob.WONLY_FUSED.get("resblock_mod") == 1, f"{n} did not take the route"
        assert y.dtype == ref.dtype and y.shape == ref.shape
        kinds.add(_kind(b))
        print(f"[mod-block-parity] {name} {str(dt)[6:]} {n} ({_kind(b)}, {a[0].shape[1]} ch {a[0].shape[2]}x{a[0].shape[3]}): unfused {e0:.3e} "
              f"route {e1:.3e} of range, ratio {e1 / max(e0, 1e-30):.2f} (bound {max(2 * e0, floor):.3e})")
        if e1 > max(2 * e0, floor):
            bad.append((n, e0, e1))
    assert any(k.startswith("down") for k in kinds) and any(k.startswith("up") for k in kinds) and any(k.endswith("+ss") for k in kinds)
    assert not bad, bad


# ---- whole UNets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_unet_matches_reference(cuda, knob, name, dt):
    """State (True, False), layer knob, attention, fusion and the route on, against the reference's weights-only golden `out_w`
    inside tests/test_weight_only_gpu.py's BOUNDS; every scale-shift / resampling residual block on the route; two runs bit-equal;
    a model without such a block bit-equal to the knob being off."""
    from qdiff.quant_block import QuantResBlock
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    knob.set_weight_only_kernel(dt)
    knob.set_weight_only_attention(dt)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_mod(False)
    _reset(knob)
    y_off = _run(qnn, fx, cuda)
    assert "resblock_mod" not in knob.WONLY_FUSED
    knob.set_weight_only_fusion_mod(True)
    _reset(knob)
    y = _run(qnn, fx, cuda)
    took = knob.WONLY_FUSED.get("resblock_mod", 0)
    y2 = _run(qnn, fx, cuda)
    want = sum(isinstance(m, QuantResBlock) and bool(m.updown or m.use_scale_shift_norm) for m in qnn.modules())
    d, cos = _metrics(y, fx["out_w"])
    d0, cos0 = _metrics(y_off, fx["out_w"])
    print(f"\n[{name}] mod route {dt}: {took} blocks, {d:.3e} of range, cosine {cos:.7f} (knob off: {d0:.3e}, {cos0:.7f})")
    assert took == want and (want > 0) == (name in ("ldm_updown_tiny", "churches_full"))
    assert y.dtype == torch.float32 and torch.equal(y, y2)
    if not want:
        assert torch.equal(y, y_off) and "resblock_mod" not in knob.WONLY_FUSED
    tol, cmin = BOUNDS[dt]
    assert d <= tol and cos >= cmin


def test_packed_checkpoint_with_freed_weights_gives_the_source_bits(cuda, knob):
    import qdiff
    from qdiff.utils import load_packed_ckpt, save_packed_ckpt
    fx = load_fixture("model_ldm_updown_tiny.pt")
    src = _resume(fx, cuda)
    knob.set_weight_only_kernel(F16)
    knob.set_weight_only_attention(F16)
    knob.set_weight_only_fusion(True)
    knob.set_weight_only_fusion_mod(True)
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
    assert dict(knob.WONLY_FUSED) == n_src and n_src.get("resblock_mod", 0) > 0
    assert torch.equal(y, y_src)
