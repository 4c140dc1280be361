"""CPU tests (no GPU) of the fused weights-only block route's host logic (engine.WEIGHT_ONLY_FUSE): the knob, which blocks take
the route and what they launch, every fallback, and the argument checks of the new entry points.  The entry points run on
tests/wonly_fused_emulator.py (fp64)."""
import os
import subprocess
import sys
from collections import Counter

import pytest
import torch

import wonly_fused_emulator
from golden_util import build_engine_model, fixture_inputs, load_fixture, quant_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    calls = wonly_fused_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    engine.calls = calls
    yield engine
    del engine.calls


def _model(name):
    import qdiff
    fx = load_fixture(f"model_{name}.pt")
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    torch.manual_seed(0)
    qnn = qdiff.QuantModel(build_engine_model(spec), wq, aq, sm_abit=spec["sm_abit"]).eval()
    qnn.set_quant_state(True, False)
    return qnn, tuple(a for a in fixture_inputs(fx, "test") if a is not None)


def _run(engine, qnn, args, fuse):
    engine.set_weight_only_fusion(fuse)
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0
    del engine.calls[:]
    with torch.no_grad():
        y = qnn(*args)
    return y, Counter(engine.calls), dict(engine.WONLY_FUSED)


def _blocks(qnn):
    from qdiff.quant_block import QuantBasicTransformerBlock, QuantResBlock
    res = [m for m in qnn.modules() if isinstance(m, QuantResBlock)]
    return res, [m for m in qnn.modules() if isinstance(m, QuantBasicTransformerBlock)]


# ---- knob ----------------------------------------------------------------------------------------------------------------
def test_knob_parsing_setter_and_default(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_FUSE is False or os.environ.get("QDIFF_WEIGHT_ONLY_FUSE")       # off by default
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
    for s, want in (("", False), ("0", False), ("off", False), ("1", True), ("ON", True), (" true ", True)):
        assert engine._parse_flag(s, "QDIFF_WEIGHT_ONLY_FUSE") is want
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_FUSE"):
        engine._parse_flag("fp16", "QDIFF_WEIGHT_ONLY_FUSE")
    engine.set_weight_only_fusion(True)
    assert engine.WEIGHT_ONLY_FUSE is True
    engine.set_weight_only_fusion("0")
    assert engine.WEIGHT_ONLY_FUSE is False
    with pytest.raises(ValueError):
        engine.set_weight_only_fusion(None)


def test_environment_variable_and_knob_needs_the_layer_knob(monkeypatch):
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_KERNEL, engine.wonly_fuse_state())"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_FUSE="1", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-3:] == ["True", "None", "False"]           # on, but without effect while the layer knob is off
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.bfloat16)
    with torch.no_grad():
        assert engine.wonly_fuse_state()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_fuse_state()                      # under autocast the route does not engage
    assert not engine.wonly_fuse_state()                              # autograd on


# ---- 1. models: every covered block on the route, launch counts, agreement with the unfused run ---------------------------
@pytest.mark.parametrize("name", ["sd_tiny", "ldm_tiny"])
def test_models_take_the_fused_route(emu, name):
    """State (True, False), fp16 operands.  Launches per evaluation, derived from the block structure: a fused residual block
    replaces the qd_rows_to_h16 passes of conv1 and conv2 by two qd_groupnorm_h16 (its skip connection keeps its own: one per
    segment); a fused transformer block replaces those of attn1.to_q / to_k / to_v, attn2.to_q, the GEGLU projection and the FF
    output — six — by three qd_layernorm_h16 and one qd_geglu_h16, and keeps attn2.to_k / to_v (context) and the two to_out
    (library attention here: its fp32 result goes through qd_rows_to_h16 as before).  Contractions: unchanged.
    Agreement: both runs round the same operands at the same sites, but the fused run evaluates the glue in fp64 (emulator)
    and the unfused one in fp32 (library), so a rounding to fp16 can land on the neighbouring value: one ulp = 2^-10 of the
    element.  To first order (unit gain per site) the outputs differ by at most one ulp of the range per producer call."""
    qnn, args = _model(name)
    res, tr = _blocks(qnn)
    plain = [b for b in res if not b.updown and not b.use_scale_shift_norm]
    assert len(plain) == len(res) > 0
    y0, c0, f0 = _run(emu, qnn, args, False)
    y1, c1, f1 = _run(emu, qnn, args, True)
    assert f0 == {"resblock": 0, "transformer": 0}
    assert f1 == {"resblock": len(plain), "transformer": len(tr)}
    assert not any(k in c0 for k in ("groupnorm_h16", "layernorm_h16", "geglu_h16"))
    assert c1["groupnorm_h16"] == 2 * len(plain) and c1["layernorm_h16"] == 3 * len(tr) and c1["geglu_h16"] == len(tr)
    assert c1["conv2d_wq_h16"] == c0["conv2d_wq_h16"]
    assert c1["rows_to_h16"] == c0["rows_to_h16"] - 2 * len(plain) - 6 * len(tr) < c0["rows_to_h16"]
    sites = c1["groupnorm_h16"] + c1["layernorm_h16"] + c1["geglu_h16"]
    rng = y0.abs().max().item()
    d = (y1 - y0).abs().max().item() / rng
    print(f"\n[{name}] fused vs unfused on the emulator: {d:.3e} of range, bound {sites} x 2^-10 = {sites * 2.0 ** -10:.3e}")
    assert y1.dtype == y0.dtype and y1.shape == y0.shape
    assert 0 < d <= sites * 2.0 ** -10


def test_fused_attention_knob_feeds_to_out_directly(emu, monkeypatch):
    """With engine.WEIGHT_ONLY_ATTN = fp16 the attention kernel writes to_out's fp16 operand rows itself when the layouts agree:
    two more qd_rows_to_h16 passes per transformer block disappear, and self-attention reads fp16 projections."""
    from qdiff import hip
    from test_weight_only_attention_host import attn_h16_emulated
    seen = []
    monkeypatch.setattr(hip, "attn_h16", lambda *a: attn_h16_emulated(*a, calls=seen))
    qnn, args = _model("sd_tiny")
    res, tr = _blocks(qnn)
    emu.set_weight_only_attention(torch.float16)
    y0, c0, _ = _run(emu, qnn, args, False)
    y1, c1, f1 = _run(emu, qnn, args, True)
    assert f1["transformer"] == len(tr) and len(seen) == 4 * len(tr)
    direct = sum(b.attn1.to_out[0].wonly_plan().ldx == b.attn1.to_q.wonly_plan().Cout for b in tr)
    assert direct == len(tr)
    assert c1["rows_to_h16"] == c0["rows_to_h16"] - 2 * len(res) - 8 * len(tr)
    fused_calls = seen[2 * len(tr):]
    assert [c["q"][0].dtype for c in fused_calls[:2]] == [torch.float16, torch.float32]       # self-, then cross-attention
    sites = c1["groupnorm_h16"] + c1["layernorm_h16"] + c1["geglu_h16"]                      # (bound: test_models_take_the_fused_route)
    assert (y1 - y0).abs().max().item() <= sites * 2.0 ** -10 * y0.abs().max().item()


# ---- 2. gate ----------------------------------------------------------------------------------------------------------------
def test_knob_off_is_todays_call_sequence(emu):
    qnn, args = _model("sd_tiny")
    y0, c0, f0 = _run(emu, qnn, args, False)
    assert set(c0) == {"rows_to_h16", "conv2d_wq_h16"} and f0 == {"resblock": 0, "transformer": 0}
    import qdiff
    n = sum(isinstance(m, qdiff.QuantModule) for m in qnn.modules())
    assert c0["conv2d_wq_h16"] == n                         # every QuantModule entered through its own forward, once
    y0b, c0b, _ = _run(emu, qnn, args, False)
    assert c0b == c0 and torch.equal(y0, y0b)


def _block_call(qnn, args, block):
    """The positional / keyword arguments `block` receives inside one evaluation of the model."""
    got = {}
    h = block.register_forward_pre_hook(lambda m, a, k: got.update(a=a, k=k), with_kwargs=True)
    try:
        with torch.no_grad():
            qnn(*args)
    finally:
        h.remove()
    return got["a"], got["k"]


@pytest.mark.parametrize("kind", ["resblock", "transformer"])
def test_block_falls_back(emu, kind):
    """A forward hook on an inner QuantModule, autograd, engine.SIMULATE, autocast, a layer without a plan, a split first
    convolution: the block takes today's composition (no producer launch, counter unchanged) and a hook fires as before."""
    from qdiff import engine
    qnn, args = _model("sd_tiny")
    res, tr = _blocks(qnn)
    blk = res[1] if kind == "resblock" else tr[0]
    inner = blk.in_layers[-1] if kind == "resblock" else blk.ff.net[0].proj
    a, k = _block_call(qnn, args, blk)
    engine.set_weight_only_fusion(True)

    def run():
        n0, c0 = engine.WONLY_FUSED[kind], len(engine.calls)
        y = blk(*a, **k)
        new = Counter(engine.calls[c0:])
        return y, engine.WONLY_FUSED[kind] - n0, sum(new[p] for p in ("groupnorm_h16", "layernorm_h16", "geglu_h16"))

    with torch.no_grad():
        y_fused, took, prod = run()
        assert took == 1 and prod == (2 if kind == "resblock" else 4)
        engine.set_weight_only_fusion(False)
        y_off, took, prod = run()
        assert (took, prod) == (0, 0)
        engine.set_weight_only_fusion(True)
        # hook on an inner module
        fired = []
        h = inner.register_forward_hook(lambda m, i, o: fired.append(1))
        try:
            y, took, prod = run()
        finally:
            h.remove()
        assert (took, prod) == (0, 0) and len(fired) == 1 and torch.equal(y, y_off)
        hp = inner.register_forward_pre_hook(lambda m, i: fired.append(2))
        try:
            assert run()[1:] == (0, 0) and fired[-1] == 2
        finally:
            hp.remove()
        assert run()[1] == 1                                   # hooks gone: fused again
        # simulation mode
        prev = engine.SIMULATE
        engine.SIMULATE = True
        try:
            assert run()[1:] == (0, 0)
        finally:
            engine.SIMULATE = prev
        # autocast
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_fuse_state()
        # a layer the kernel does not take (no plan)
        inner.__dict__["_wonly_cache"] = [None, None]
        orig = type(inner).wonly_plan
        try:
            inner.wonly_plan = lambda: None
            y, took, prod = run()
        finally:
            del inner.wonly_plan
        assert (took, prod) == (0, 0) and orig(inner) is not None      # (that layer itself now runs the library path)
        # live dropout
        if kind == "resblock":
            blk.out_layers[2].p, blk.training = 0.5, True
            blk.__dict__.pop("_qd_has_dropout", None)
            try:
                assert run()[1] == 0
            finally:
                blk.out_layers[2].p, blk.training = 0.0, False
                blk.__dict__.pop("_qd_has_dropout", None)
        assert run()[1] == 1
    y, took, prod = run()                                      # autograd on
    assert (took, prod) == (0, 0)
    assert y_fused.dtype == y_off.dtype and y_fused.shape == y_off.shape


def test_resblock_with_scale_shift_norm_or_updown_keeps_todays_path(emu):
    qnn, args = _model("sd_tiny")
    res, _ = _blocks(qnn)
    blk = res[0]
    a, k = _block_call(qnn, args, blk)
    emu.set_weight_only_fusion(True)
    with torch.no_grad():
        blk(*a, **k)
        assert emu.WONLY_FUSED["resblock"] == 1
        blk.updown = True
        try:
            assert blk._wonly_route(a[0], a[1], blk.in_layers[-1], blk.out_layers[-1]) != "resblock"
        finally:
            blk.updown = False
        blk.use_scale_shift_norm = True
        try:
            assert blk._wonly_route(a[0], a[1], blk.in_layers[-1], blk.out_layers[-1]) != "resblock"
        finally:
            blk.use_scale_shift_norm = False
        assert blk._wonly_route(a[0], a[1], blk.in_layers[-1], blk.out_layers[-1]) == "resblock"


# ---- 3. argument checks before any launch -------------------------------------------------------------------------------------
def test_contraction_still_refuses_statistics_and_upsampling(emu):
    from qdiff import hip
    src = open(os.path.join(ROOT, "q-diffusion_amd", "csrc", "wq_h16.hip")).read()
    body = src[src.index("int plan_wq("):]
    assert "!d->gn_part && !d->upsample2x" in body and "!d->rowbias &&" not in body.split("WqD k{}")[0]
    c = hip.ConvCall(gn_part=torch.zeros(1), upsample2x=False, rowbias=None)
    with pytest.raises(hip.HipEngineError, match="linear epilogue only"):
        wonly_fused_emulator.conv2d_wq_h16(c, torch.float16)
    # the same through the real library on fake pointers: the launcher and its form query refuse, with one message, before any
    # launch; a row bias alone is no reason to refuse
    import ctypes
    from conv_form_util import FAKE
    lib = hip.load()

    def desc(**fields):
        d = hip.ConvDesc()
        d.x = d.w = d.out = d.rowbias = d.seg[0].scale = d.seg[0].zw = FAKE
        d.ldx, d.ldo, d.ld_rowbias = 16, 24, 24
        d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = 2, 5, 5, 5, 5, 24
        d.kh, d.kw, d.stride, d.pad_t, d.pad_l = 3, 3, 1, 1, 1
        d.wbits, d.w_tiled, d.nseg, d.seg[0].clen = 4, 1, 1, 16
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    form = (ctypes.c_int32 * 4)()
    assert lib.qd_conv2d_wq_h16_form(ctypes.byref(desc()), hip.F16, form) == 0 and tuple(form) == (1, 0, 0, 0)
    for bad in (dict(gn_part=FAKE), dict(upsample2x=1)):
        d = desc(**bad)
        assert lib.qd_conv2d_wq_h16_form(ctypes.byref(d), hip.F16, form) != 0
        msg = lib.qd_last_error().decode()
        assert "linear epilogue only (no GroupNorm statistics or up-sampling)" in msg
        assert lib.qd_conv2d_wq_h16(ctypes.byref(d), hip.F16, None) != 0 and lib.qd_last_error().decode() == msg


def test_forward_rows_rowbias_is_validated(emu):
    import qdiff
    torch.manual_seed(0)
    m = qdiff.QuantModule(torch.nn.Conv2d(16, 24, 3, padding=1), dict(n_bits=4, channel_wise=True, scale_method="max"),
                          dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True))
    m.set_quant_state(True, False)
    x = torch.randn(2, 16, 5, 5)
    with torch.no_grad():
        y = m(x)
        plan = m.wonly_plan()
        xh = emu.wonly_rows(x, plan, 2, 16, 25, (x.stride(0), x.stride(1), x.stride(3)))
        rb = torch.randn(2, 24)
        got = m.forward_rows(xh, 2, 5, 5, rowbias=rb).view(2, 5, 5, 24).permute(0, 3, 1, 2)
        assert torch.allclose(got, y + rb[:, :, None, None], atol=1e-5, rtol=1e-5)
        for bad in (rb.double(), rb[:1], rb[:, :20], torch.randn(24, 2).t()):
            with pytest.raises(qdiff.hip.HipEngineError, match="rowbias"):
                m.forward_rows(xh, 2, 5, 5, rowbias=bad)


def test_host_wrappers_validate_before_any_launch(monkeypatch):
    """The real wrappers of qdiff.hip on CPU tensors: a bad dtype, row stride, alignment or width raises before the library is
    even loaded (hip.load would raise its own error without a GPU build)."""
    from qdiff import hip
    monkeypatch.setattr(hip, "load", lambda: pytest.fail("the library was reached"))
    E = hip.HipEngineError
    x32, x16 = torch.zeros(4, 64), torch.zeros(4, 64, dtype=torch.float16)
    out = torch.zeros(4, 64, dtype=torch.float16)
    g = torch.ones(64)
    with pytest.raises(E, match="unsupported dtypes"):
        hip.layernorm_h16(x32.double(), 4, 64, 64, 1e-5, g, g, out, 64)
    with pytest.raises(E, match="unsupported dtypes"):
        hip.layernorm_h16(x32, 4, 64, 64, 1e-5, g, g, out.float(), 64)
    with pytest.raises(E, match="input rows"):
        hip.layernorm_h16(x32, 4, 62, 62, 1e-5, g, g, out, 64)                     # fp32 row stride not a multiple of 4
    with pytest.raises(E, match="input rows"):
        hip.layernorm_h16(x16, 4, 60, 60, 1e-5, g, g, out, 64)                     # fp16 row stride not a multiple of 8
    with pytest.raises(E, match="input rows"):
        hip.layernorm_h16(x32.view(-1)[1:65 * 3 + 1], 3, 64, 64, 1e-5, g, g, out, 64)   # base not 16-byte aligned
    with pytest.raises(E, match="ldo % 8"):
        hip.layernorm_h16(x32, 4, 56, 64, 1e-5, g, g, out, 60)
    with pytest.raises(E, match="ldo % 8"):
        hip.layernorm_h16(x32, 4, 64, 64, 1e-5, g, g, out, 56)                     # ldo < C
    with pytest.raises(E, match="C=4096"):
        hip.layernorm_h16(torch.zeros(1, 4096), 1, 4096, 4096, 1e-5, g, g, torch.zeros(1, 4096, dtype=torch.float16), 4096)
    with pytest.raises(E, match="input rows"):
        hip.geglu_h16(x32, 4, 40, 64, out, 64)                                     # ldh < 2 F
    with pytest.raises(E, match="F=12"):
        hip.geglu_h16(x32, 4, 12, 64, out, 64)
    with pytest.raises(E, match="ldo % 8"):
        hip.geglu_h16(x32, 4, 32, 64, out, 24)
    with pytest.raises(E, match="groups=7"):
        hip.groupnorm_h16(x32, 1, 4, 64, 64, 7, 1e-5, g, g, True, out, 64, torch.zeros(64))
    with pytest.raises(E, match="unsupported dtypes"):
        hip.groupnorm_h16(x32.bfloat16(), 1, 4, 64, 64, 8, 1e-5, g, g, True, out, 64, torch.zeros(64))
    with pytest.raises(E, match="ldo % 8"):
        hip.groupnorm_h16(x32, 1, 4, 64, 64, 8, 1e-5, g, g, True, out, 68, torch.zeros(64))
