"""CPU tests (no GPU) of the fused weights-only attention's host logic (engine.WEIGHT_ONLY_ATTN): knob and environment
parsing, which attention calls take the kernel and every fallback to the library path, the stride triples handed to the
kernel, and the output views and dtypes.  qd_attn_h16 runs on an fp64 emulation defined here (attn_h16_emulated)."""
import os
import subprocess
import sys

import pytest
import torch

from golden_util import build_engine_model, fixture_inputs, load_fixture, quant_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def attn_h16_emulated(q, k, v, B, T, S, H, d, q_strides, k_strides, v_strides, scale, op_dtype, out, calls=None):
    """include/qdiff_hip.h qd_attn_h16 in fp64: the inputs rounded to the operand type, softmax(q k^T * scale) v, merged-head
    rows written to out."""
    if calls is not None:
        calls.append(dict(B=B, T=T, S=S, H=H, d=d, q=(q, q_strides), k=(k, k_strides), v=(v, v_strides), scale=scale, op=op_dtype))
    assert q_strides[3] == k_strides[3] == v_strides[3] == 1
    qh, kh, vh = (torch.as_strided(t, (B, n, H, d), st).to(op_dtype).double()
                  for t, n, st in ((q, T, q_strides), (k, S, k_strides), (v, S, v_strides)))
    p = torch.softmax(torch.einsum("bthd,bshd->bhts", qh, kh) * scale, dim=-1)
    out.view(-1, out.stride(0))[:, :H * d] = torch.einsum("bhts,bshd->bthd", p, vh).reshape(B * T, H * d).to(out.dtype)


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine, hip
    calls = []
    monkeypatch.setattr(hip, "attn_h16", lambda *a: attn_h16_emulated(*a, calls=calls))
    monkeypatch.setattr(engine, "wonly_device_ok", lambda t: True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", None)
    engine.calls = calls
    yield engine
    del engine.calls


# ---- knob ----------------------------------------------------------------------------------------------------------------
def test_knob_parsing_and_setter(monkeypatch):
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    for s, want in (("", None), ("off", None), ("0", None), ("fp16", torch.float16), ("half", torch.float16),
                    ("BF16", torch.bfloat16), (" bfloat16 ", torch.bfloat16)):
        assert engine._parse_weight_only_attn(s) == want
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_ATTN"):
        engine._parse_weight_only_attn("fp8")
    engine.set_weight_only_attention("bf16")
    assert engine.WEIGHT_ONLY_ATTN == torch.bfloat16
    engine.set_weight_only_attention(torch.float16)
    assert engine.WEIGHT_ONLY_ATTN == torch.float16
    engine.set_weight_only_attention(None)
    assert engine.WEIGHT_ONLY_ATTN is None
    with pytest.raises(ValueError):
        engine.set_weight_only_attention(torch.float32)


def test_knob_is_independent_of_the_layer_knob(monkeypatch):
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", None)
    engine.set_weight_only_attention(torch.float16)
    assert engine.WEIGHT_ONLY_KERNEL is None
    engine.set_weight_only_attention(None)
    engine.set_weight_only_kernel(torch.bfloat16)
    assert engine.WEIGHT_ONLY_ATTN is None


def test_environment_variable():
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_KERNEL)"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_ATTN="bf16", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["torch.bfloat16", "None"]


def test_head_dims_the_kernel_covers():
    from qdiff import engine
    assert all(engine.wonly_attn_shape_ok(d) for d in (8, 16, 24, 32, 40, 48, 64, 80, 96, 160))
    assert not any(engine.wonly_attn_shape_ok(d) for d in (4, 12, 36, 168, 256))


# ---- models ---------------------------------------------------------------------------------------------------------------
def _model(name, state=(True, False)):
    import qdiff
    fx = load_fixture(f"model_{name}.pt")
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    torch.manual_seed(0)
    qnn = qdiff.QuantModel(build_engine_model(spec), wq, aq, sm_abit=spec["sm_abit"]).eval()
    qnn.set_quant_state(*state)
    return qnn, fx


def _first(qnn, cls):
    return next(m for m in qnn.modules() if isinstance(m, cls))


def _sd(state=(True, False)):
    from qdiff.quant_block import QuantBasicTransformerBlock
    qnn, fx = _model("sd_tiny", state)
    blk = _first(qnn, QuantBasicTransformerBlock)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, blk.attn1.to_q.weight.shape[1], generator=g)
    ctx = torch.randn(2, 7, blk.attn2.to_k.weight.shape[1], generator=g)
    return qnn, blk, x, ctx


def _ldm(state=(True, False)):
    from qdiff.quant_block import QuantAttentionBlock
    qnn, fx = _model("ldm_tiny", state)
    blk = _first(qnn, QuantAttentionBlock)
    x = torch.randn(2, blk.channels, 4, 4, generator=torch.Generator().manual_seed(4))
    return qnn, blk, x


def _on_off(engine, fn, dtype=torch.float16):
    engine.set_weight_only_attention(None)
    y0 = fn()
    engine.set_weight_only_attention(dtype)
    n0 = len(engine.calls)
    y1 = fn()
    return y0, y1, len(engine.calls) - n0


def _close(y1, y0, tol=1e-2):
    return (y1.float() - y0.float()).abs().max().item() <= tol * y0.float().abs().max().item()


def test_sd_attention_takes_the_kernel_in_state_true_false(emu):
    qnn, blk, x, ctx = _sd()
    with torch.no_grad():
        for att, c in ((blk.attn1, None), (blk.attn2, ctx)):
            y0, y1, n = _on_off(emu, lambda: att(x, context=c))
            assert n == 1 and y1.shape == y0.shape and y1.dtype == y0.dtype and _close(y1, y0)


def test_ldm_block_takes_the_kernel_in_state_true_false(emu):
    qnn, blk, x = _ldm()
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk(x))
    assert n == 1 and y1.shape == y0.shape and _close(y1, y0)
    ch = blk.channels // blk.num_heads
    assert abs(blk.attention.qkv_matmul.scale - ch ** -0.25) < 1e-12              # set as QKVAttentionLegacy.forward does
    assert emu.calls[-1]["scale"] == ch ** -0.5


@pytest.mark.parametrize("state", [(False, False)])
def test_other_states_are_untouched(emu, state):
    """(False, False): the fp state calibration takes its targets from (the quantised-activation states run the integer engine,
    which needs a GPU: tests/test_weight_only_attention_gpu.py covers (True, True))."""
    qnn, blk, x, ctx = _sd(state)
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn2(x, context=ctx))
    assert n == 0 and torch.equal(y0, y1)
    qnn, lblk, lx = _ldm(state)
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: lblk(lx))
    assert n == 0 and torch.equal(y0, y1)


def test_mask_grad_and_simulation_keep_the_library_path(emu, monkeypatch):
    qnn, blk, x, ctx = _sd()
    mask = torch.ones(2, 7, dtype=torch.bool)
    mask[:, 4:] = False
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn2(x, context=ctx, mask=mask))
    assert n == 0 and torch.equal(y0, y1)
    y0, y1, n = _on_off(emu, lambda: blk.attn1(x).detach())                   # grad enabled
    assert n == 0 and torch.equal(y0, y1)
    monkeypatch.setattr(emu, "SIMULATE", True)
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn1(x))
    assert n == 0 and torch.equal(y0, y1)


def test_head_dim_outside_the_range_keeps_the_library_path(emu, monkeypatch):
    qnn, blk, x, ctx = _sd()
    monkeypatch.setattr(emu, "WONLY_ATTN_DMAX", 8)                       # the fixture's d = 16 is now outside
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn1(x))
    assert n == 0 and torch.equal(y0, y1)


def test_cpu_tensors_keep_the_library_path(emu, monkeypatch):
    qnn, blk, x, ctx = _sd()
    monkeypatch.setattr(emu, "wonly_device_ok", lambda t: t.is_cuda)
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn1(x))
    assert n == 0 and torch.equal(y0, y1)


@pytest.mark.parametrize("where", ["attention", "qkv_matmul", "smv_matmul"])
@pytest.mark.parametrize("kind", ["hook", "pre_hook"])
def test_hooks_on_the_legacy_attention_keep_the_library_path(emu, where, kind):
    qnn, blk, x = _ldm()
    mod = blk.attention if where == "attention" else getattr(blk.attention, where)
    h = (mod.register_forward_hook(lambda *a: None) if kind == "hook" else mod.register_forward_pre_hook(lambda *a: None))
    try:
        with torch.no_grad():
            y0, y1, n = _on_off(emu, lambda: blk(x))
    finally:
        h.remove()
    assert n == 0 and torch.equal(y0, y1)


def test_cifar_attention_block_keeps_the_library_path(emu):
    qnn, fx = _model("cifar_tiny")
    x, t, _ = fixture_inputs(fx, "test")
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: qnn(x, t))
    assert n == 0 and torch.equal(y0, y1)


# ---- strides and views ----------------------------------------------------------------------------------------------------
def _logical(entry, B, N, H, d):
    t, st = entry
    return torch.as_strided(t, (B, N, H, d), st)


def test_sd_stride_triples_give_the_split_heads_values(emu):
    from qdiff.arch import ldm_unet
    qnn, blk, x, ctx = _sd()
    emu.set_weight_only_attention(torch.float16)
    for att, c in ((blk.attn1, None), (blk.attn2, ctx)):
        with torch.no_grad():
            att(x, context=c)
            cc = x if c is None else c
            ref = [ldm_unet._split_heads(m(src), att.heads) for m, src in ((att.to_q, x), (att.to_k, cc), (att.to_v, cc))]
        call = emu.calls[-1]
        B, T, S, H, d = call["B"], call["T"], call["S"], call["H"], call["d"]
        assert (B, T, S, H) == (2, x.shape[1], cc.shape[1], att.heads)
        for name, n, r in (("q", T, ref[0]), ("k", S, ref[1]), ("v", S, ref[2])):
            got = _logical(call[name], B, n, H, d).permute(0, 2, 1, 3).reshape(B * H, n, d)
            assert torch.equal(got, r), name
        assert call["scale"] == att.scale


@pytest.mark.parametrize("layers", [False, True], ids=["library_qkv", "channels_last_qkv"])
def test_ldm_stride_triples_give_the_legacy_attention_values(emu, layers, monkeypatch):
    import wonly_emulator
    if layers:
        wonly_emulator.install(monkeypatch)
        emu.set_weight_only_kernel(torch.float16)
    qnn, blk, x = _ldm()
    emu.set_weight_only_attention(torch.float16)
    with torch.no_grad():
        blk(x)
        emu.set_weight_only_attention(None)
        qkv = blk.qkv(blk.norm(x.reshape(x.shape[0], x.shape[1], -1)))
    call = emu.calls[-1]
    B, T, H, d = call["B"], call["T"], call["H"], call["d"]
    q, k, v = qkv.reshape(B * H, 3 * d, T).split(d, dim=1)                       # QKVAttentionLegacy.forward
    for name, r in (("q", q), ("k", k), ("v", v)):
        got = _logical(call[name], B, T, H, d).permute(0, 2, 3, 1).reshape(B * H, d, T)
        assert torch.equal(got.float(), r.float()), name
    if layers:
        assert call["q"][0].stride(1) == 1                                        # the layer kernel's rows, read as they are


def test_output_views_and_dtypes(emu):
    qnn, blk, x, ctx = _sd()
    with torch.no_grad():
        y0, y1, n = _on_off(emu, lambda: blk.attn2(x, context=ctx))
    assert n == 1 and y1.dtype == torch.float32 and y1.shape == y0.shape
    qnn, lblk, lx = _ldm()
    seen = []
    h = lblk.proj_out.register_forward_pre_hook(lambda m, a: seen.append((a[0].shape, a[0].dtype)))
    try:
        with torch.no_grad():
            y0, y1, n = _on_off(emu, lambda: lblk(lx))
    finally:
        h.remove()
    assert n == 1 and seen[0] == seen[1]                                         # proj_out sees the library's [B, C, T] view


def test_output_dtype_under_autocast(emu):
    qnn, blk, x, ctx = _sd()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        y0, y1, n = _on_off(emu, lambda: blk.attn2(x, context=ctx))
    assert n == 1 and y1.dtype == y0.dtype == torch.bfloat16 and _close(y1, y0, 3e-2)
    assert emu.calls[-1]["op"] == torch.float16
