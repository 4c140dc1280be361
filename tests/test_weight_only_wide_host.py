"""CPU tests (no GPU) of the wide weights-only fusion's host logic (engine.WEIGHT_ONLY_FUSE_WIDE): the knob, the GEGLU plan over
the interleaved pack, which blocks take the route and what they launch, every fallback, and the wrapper's argument checks for
the GEGLU epilogue.  The entry points run on tests/wonly_wide_emulator.py (fp64)."""
import os
import subprocess
import sys
from collections import Counter

import pytest
import torch

import wonly_wide_emulator
from test_weight_only_fused_host import _block_call, _blocks, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCERS = ("groupnorm_h16", "layernorm_h16", "geglu_h16", "geglu_epi")


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    calls = wonly_wide_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_WIDE", False)
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    monkeypatch.setattr(engine, "WONLY_GEGLU_EPI", [0])
    engine.calls = calls
    yield engine
    del engine.calls


def _run(engine, qnn, args, fuse, wide):
    engine.set_weight_only_fusion(fuse)
    engine.set_weight_only_fusion_wide(wide)
    engine.WONLY_FUSED.clear()
    engine.WONLY_FUSED.update({"resblock": 0, "transformer": 0})
    engine.WONLY_GEGLU_EPI[0] = 0
    del engine.calls[:]
    with torch.no_grad():
        y = qnn(*args)
    return y, Counter(engine.calls), dict(engine.WONLY_FUSED)


def _edges(qnn):
    from qdiff.arch import ldm_unet
    from qdiff.quant_block import QuantAttentionBlock
    return ([m for m in qnn.modules() if isinstance(m, ldm_unet.SpatialTransformer)],
            [m for m in qnn.modules() if isinstance(m, QuantAttentionBlock)])


# ---- knob ----------------------------------------------------------------------------------------------------------------
def test_knob_parsing_setter_and_default(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_FUSE_WIDE is False or os.environ.get("QDIFF_WEIGHT_ONLY_FUSE_WIDE")       # off by default
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_WIDE", False)
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_FUSE_WIDE"):
        engine._parse_flag("fp16", "QDIFF_WEIGHT_ONLY_FUSE_WIDE")
    engine.set_weight_only_fusion_wide(True)
    assert engine.WEIGHT_ONLY_FUSE_WIDE is True
    engine.set_weight_only_fusion_wide("off")
    assert engine.WEIGHT_ONLY_FUSE_WIDE is False
    with pytest.raises(ValueError):
        engine.set_weight_only_fusion_wide(1)
    from qdiff import hip
    assert hip.EPI_GEGLU_H16 == 4 and "QD_EPI_GEGLU_H16 = 4" in open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()


def test_environment_variable_and_knob_needs_the_fusion_knob(monkeypatch):
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_FUSE_WIDE, engine.WEIGHT_ONLY_FUSE, engine.wonly_wide_state())"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_FUSE_WIDE="1", QDIFF_WEIGHT_ONLY="fp16", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY_FUSE", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-3:] == ["True", "False", "False"]
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_WIDE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    with torch.no_grad():
        assert engine.wonly_wide_state()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_wide_state()
        monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
        assert not engine.wonly_wide_state()


def test_wide_knob_alone_changes_nothing(emu):
    """On without QDIFF_WEIGHT_ONLY_FUSE: the unfused call sequence and bytes."""
    qnn, args = _model("sd_tiny")
    y0, c0, f0 = _run(emu, qnn, args, False, False)
    y1, c1, f1 = _run(emu, qnn, args, False, True)
    assert c1 == c0 and f1 == f0 == {"resblock": 0, "transformer": 0} and torch.equal(y0, y1) and emu.WONLY_GEGLU_EPI[0] == 0


# ---- models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sd_tiny", "ldm_tiny"])
def test_models_take_the_wide_route(emu, name):
    """State (True, False), fp16 operands, against the fused run with the wide knob off.  Derived from the module tree: every
    transformer block's qd_geglu_h16 launch disappears into its projection (same number of contractions); every
    SpatialTransformer and attention block replaces the qd_rows_to_h16 pass of proj_in / qkv by one qd_groupnorm_h16.
    Agreement: as in tests/test_weight_only_fused_host.py — the same operands are rounded at the same sites, the glue in front
    of a site is evaluated in fp64 here and in fp32 there, so each producer launch can move one fp16 rounding by one ulp:
    `sites` x 2^-10 of the range, sites = the producer launches of the wide run."""
    qnn, args = _model(name)
    res, tr = _blocks(qnn)
    sts, atts = _edges(qnn)
    plain = [b for b in res if not b.updown and not b.use_scale_shift_norm]
    assert len(sts) + len(atts) > 0
    y0, c0, f0 = _run(emu, qnn, args, True, False)
    assert set(f0) == {"resblock", "transformer"} and "geglu_epi" not in c0 and c0["geglu_h16"] == len(tr)
    y1, c1, f1 = _run(emu, qnn, args, True, True)
    want = {"resblock": len(plain), "transformer": len(tr)}
    if sts:
        want["spatial"] = len(sts)
    if atts:
        want["attnblock"] = len(atts)
    assert f1 == want
    assert c1["geglu_h16"] == 0 and c1["geglu_epi"] == len(tr) == emu.WONLY_GEGLU_EPI[0]
    assert c1["conv2d_wq_h16"] == c0["conv2d_wq_h16"]
    assert c1["layernorm_h16"] == c0["layernorm_h16"] == 3 * len(tr)
    assert c1["groupnorm_h16"] == 2 * len(plain) + len(sts) + len(atts)
    assert c1["rows_to_h16"] == c0["rows_to_h16"] - len(sts) - len(atts)
    sites = sum(c1[k] for k in PRODUCERS)
    rng = y0.abs().max().item()
    d = (y1 - y0).abs().max().item() / rng
    print(f"\n[{name}] wide on vs off on the emulator: {d:.3e} of range, bound {sites} x 2^-10 = {sites * 2.0 ** -10:.3e}")
    assert y1.dtype == y0.dtype and y1.shape == y0.shape
    assert d <= sites * 2.0 ** -10
    # knob off again: the fused route's call sequence of before
    y2, c2, f2 = _run(emu, qnn, args, True, False)
    assert c2 == c0 and f2 == f0 and torch.equal(y2, y0)


# ---- the GEGLU plan ----------------------------------------------------------------------------------------------------------
def _linear(cin, cout, bits=4):
    import qdiff
    torch.manual_seed(0)
    m = qdiff.QuantModule(torch.nn.Linear(cin, cout), dict(n_bits=bits, channel_wise=True, scale_method="max"),
                          dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True))
    m.set_quant_state(True, False)
    with torch.no_grad():
        m(torch.randn(3, cin))                              # initialises the weight quantiser
    return m


def _same_plan(a, b):
    assert torch.equal(a.pack.wq, b.pack.wq) and torch.equal(a.pack.row_perm, b.pack.row_perm)
    assert torch.equal(a.bias, b.bias) and a.ldx == b.ldx and a.Cout == b.Cout and a.act_dtype == b.act_dtype
    for sa, sb in zip(a.segs, b.segs):
        assert torch.equal(sa["scale"], sb["scale"]) and torch.equal(sa["zw"], sb["zw"]) and sa["kstep0"] == sb["kstep0"]


@pytest.mark.parametrize("bits", [4, 8])
def test_geglu_plan_sources_agree_and_follow_the_cache(emu, bits):
    """Gathered tile by tile from the layer's own (then frozen) pack == built from a fresh pack of the permuted rows; the bias
    is permuted with the rows; cached; dropped by invalidate(); the activation quantiser is never touched; a frozen pack whose
    fp32 weights were freed still gives it."""
    m = _linear(40, 192, bits)
    F = 96
    with torch.no_grad():
        p = m.wonly_geglu_plan()
        assert p is not None and m.wonly_geglu_plan() is p and not m.act_quantizer.inited
        perm = emu.geglu_row_perm(F, "cpu")
        fresh = emu.build_wonly_plan(emu.pack_module_weights(m.weight, [m.weight_quantizer], 0, row_perm=perm), 1, 1, 1, 0, m.bias,
                                     torch.float16, geglu=True)
        _same_plan(p, fresh)
        assert torch.equal(p.bias, m.bias.detach()[perm])
        assert emu.build_wonly_plan(fresh.pack, 1, 1, 1, 0, m.bias, torch.float16) is None        # every other caller: refused
        assert emu.build_wonly_plan(m.wonly_plan().pack, 1, 1, 1, 0, m.bias, torch.float16, geglu=True) is None
        m.invalidate()
        p2 = m.wonly_geglu_plan()
        assert p2 is not p
        _same_plan(p2, p)
        # frozen pack, weights freed
        m.load_packed(m.wonly_plan().pack)
        m.weight.data = torch.empty(0)
        m.org_weight = torch.empty(0)
        p3 = m.wonly_geglu_plan()
        assert p3 is not None and p3 is not p2
        _same_plan(p3, p)
        # the interleaved pack of a packed checkpoint comes first
        m.load_packed(m.wonly_plan().pack, geglu_pack=fresh.pack)
        assert m.wonly_geglu_plan().pack is fresh.pack


def test_geglu_plan_refusals(emu):
    import qdiff
    with torch.no_grad():
        assert _linear(40, 80).wonly_geglu_plan() is None                       # F = 40: not whole 32-row tiles
        m = _linear(48, 128)
        assert m.wonly_geglu_plan() is not None
        m.split = 16
        assert m.wonly_geglu_plan() is None
        conv = qdiff.QuantModule(torch.nn.Conv2d(16, 128, 1), dict(n_bits=4, channel_wise=True, scale_method="max"),
                                 dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True))
        conv.set_quant_state(True, False)
        conv(torch.randn(1, 16, 4, 4))
        assert conv.wonly_plan() is not None and conv.wonly_geglu_plan() is None
        emu.WEIGHT_ONLY_KERNEL = None
        assert _linear(48, 128).wonly_geglu_plan() is None


def test_epilogue_equals_linear_plus_geglu_on_the_emulator(emu):
    """engine.wonly_forward_geglu on the interleaved plan against wonly_forward + wonly_geglu_rows of the same layer (fp64
    emulation on both sides: equal up to the fp32 store of the intermediate, i.e. one fp16 ulp), pad channels zero."""
    m = _linear(40, 192)
    nxt = _linear(96, 24)
    with torch.no_grad():
        x = torch.randn(7, 40)
        plan, gplan, nplan = m.wonly_plan(), m.wonly_geglu_plan(), nxt.wonly_plan()
        xh = emu.wonly_rows(x, plan, 1, 40, 7, (0, 1, 40))
        ref = emu.wonly_geglu_rows(emu.wonly_forward(plan, xh, 1, 1, 7, 1, 7), 7, 96, nplan)
        got = emu.wonly_forward_geglu(gplan, xh, 7, nplan)
    assert got.dtype == ref.dtype == torch.float16 and got.shape == ref.shape == (7, nplan.ldx)
    assert (got[:, 96:] == 0).all()
    assert ((got.double() - ref.double()).abs() <= 2.0 ** -10 * ref.double().abs() + 2.0 ** -24).all()
    assert emu.WONLY_GEGLU_EPI[0] == 1
    from qdiff import hip
    with pytest.raises(hip.HipEngineError, match="geglu_row_perm"):
        emu.wonly_forward_geglu(plan, xh, 7, nplan)


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["transformer", "spatial", "attnblock"])
def test_block_falls_back(emu, kind):
    """A hook on a module below the block, a split first projection, autocast, autograd, the wide knob off: today's fused path for
    that block, no wide counter, no GEGLU-epilogue launch."""
    qnn, args = _model("ldm_tiny" if kind == "attnblock" else "sd_tiny")
    _, tr = _blocks(qnn)
    sts, atts = _edges(qnn)
    blk = {"transformer": tr, "spatial": sts, "attnblock": atts}[kind][0]
    inner = {"transformer": lambda: blk.ff.net[0].proj, "spatial": lambda: blk.proj_in, "attnblock": lambda: blk.qkv}[kind]()
    a, k = _block_call(qnn, args, blk)
    emu.set_weight_only_fusion(True)
    emu.set_weight_only_fusion_wide(True)

    def run():
        before = (emu.WONLY_FUSED.get("spatial", 0), emu.WONLY_FUSED.get("attnblock", 0), emu.WONLY_GEGLU_EPI[0])
        c0 = len(emu.calls)
        y = blk(*a, **k)
        after = (emu.WONLY_FUSED.get("spatial", 0), emu.WONLY_FUSED.get("attnblock", 0), emu.WONLY_GEGLU_EPI[0])
        return y, tuple(x - y for x, y in zip(after, before)), Counter(emu.calls[c0:])

    took = {"transformer": (0, 0, 1), "spatial": (1, 0, len(blk.transformer_blocks) if kind == "spatial" else 0), "attnblock": (0, 1, 0)}[kind]
    with torch.no_grad():
        y_on, moved, _ = run()
        assert moved == took
        emu.set_weight_only_fusion_wide(False)
        y_off, moved, c_off = run()
        assert moved == (0, 0, 0) and "geglu_epi" not in c_off
        assert y_on.dtype == y_off.dtype and y_on.shape == y_off.shape
        emu.set_weight_only_fusion_wide(True)
        fired = []
        h = inner.register_forward_hook(lambda m, i, o: fired.append(1))
        try:
            y, moved, c = run()
        finally:
            h.remove()
        # (the transformer blocks inside a SpatialTransformer whose proj_in is hooked keep their own route: the hook is not below them)
        assert moved == ((0, 0, took[2]) if kind == "spatial" else (0, 0, 0)) and fired
        assert run()[1] == took
        if kind != "transformer":
            from qdiff import quant_block as qb
            x, c = a[0], a[0].shape[1]
            gate = (lambda: qb.spatial_wonly_wide(blk, x)) if kind == "spatial" else (lambda: qb._wonly_wide_edges(blk, x, blk.qkv, blk.proj_out, c, c))
            assert gate()
            inner.split = 8                                    # a split first projection: the route's gate says no
            try:
                assert not gate()
            finally:
                inner.split = 0
            assert gate() and run()[1] == took
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not emu.wonly_wide_state()
        prev = emu.SIMULATE
        emu.SIMULATE = True
        try:
            assert run()[1] == (0, 0, 0)
        finally:
            emu.SIMULATE = prev
    assert run()[1] == (0, 0, 0)                               # autograd on
    assert "spatial" not in emu.WONLY_FUSED or kind == "spatial"


def test_transformer_without_a_geglu_plan_keeps_two_launches(emu):
    qnn, args = _model("sd_tiny")
    _, tr = _blocks(qnn)
    blk = tr[0]
    a, k = _block_call(qnn, args, blk)
    emu.set_weight_only_fusion(True)
    emu.set_weight_only_fusion_wide(True)
    proj = blk.ff.net[0].proj
    with torch.no_grad():
        proj.wonly_geglu_plan = lambda: None
        try:
            c0 = len(emu.calls)
            blk(*a, **k)
            c = Counter(emu.calls[c0:])
        finally:
            del proj.wonly_geglu_plan
    assert c["geglu_h16"] == 1 and "geglu_epi" not in c and emu.WONLY_GEGLU_EPI[0] == 0


# ---- argument checks before any launch -------------------------------------------------------------------------------------
def test_wrapper_validates_the_geglu_epilogue_before_any_launch(monkeypatch):
    from qdiff import hip
    monkeypatch.setattr(hip, "load", lambda: pytest.fail("the library was reached"))
    E = hip.HipEngineError
    x = torch.zeros(4, 64, dtype=torch.float16)
    w = torch.zeros(1024 * 4, dtype=torch.uint8)
    seg = [dict(c0=0, clen=64, kofs=0, kstep0=0, scale=torch.ones(128), zw=torch.zeros(128, dtype=torch.int32))]

    def call(**kw):
        base = dict(x=x, w=w, out=torch.zeros(4, 64, dtype=torch.float16), ldx=64, ldk=64, ldo=64, B=1, H=1, W=4, Ho=1, Wo=4, Cout=128,
                    kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=4, w_tiled=True, segs=seg, epilogue=hip.EPI_GEGLU_H16)
        base.update(kw)
        return hip.ConvCall(**base)

    with pytest.raises(E, match="operand rows"):
        hip.conv2d_wq_h16(call(out=torch.zeros(4, 64)), torch.float16)                         # fp32 out
    with pytest.raises(E, match="operand rows"):
        hip.conv2d_wq_h16(call(out=torch.zeros(4, 64, dtype=torch.bfloat16)), torch.float16)   # not the operand type
    with pytest.raises(E, match="ldo >= 64"):
        hip.conv2d_wq_h16(call(ldo=56), torch.float16)
    with pytest.raises(E, match="ldo % 8"):
        hip.conv2d_wq_h16(call(ldo=68), torch.float16)
    with pytest.raises(E, match="no residual and no rowbias"):
        hip.conv2d_wq_h16(call(residual=torch.zeros(4, 64, dtype=torch.float16), ldr=64), torch.float16)
    with pytest.raises(E, match="no residual and no rowbias"):
        hip.conv2d_wq_h16(call(rowbias=torch.zeros(1, 128), ld_rowbias=128), torch.float16)
    with pytest.raises(E, match="F % 32"):
        hip.conv2d_wq_h16(call(Cout=80), torch.float16)
    with pytest.raises(E, match="EPI_LINEAR or EPI_GEGLU_H16"):
        hip.conv2d_wq_h16(call(epilogue=hip.EPI_GEGLU_I8), torch.float16)


def test_library_source_refuses_the_same_before_launching():
    src = open(os.path.join(ROOT, "q-diffusion_amd", "csrc", "wq_h16.hip")).read()
    body = src[src.index("int plan_wq("):]
    head = body.split("WqD k{}")[0]
    for needle in ("QD_EPI_GEGLU_H16", "d->out_dtype == act_dtype", "takes no residual and no rowbias", "d->Cout % 64 == 0",
                   "!d->gn_part && !d->upsample2x"):
        assert needle in head, needle
    # the same through the real library on fake pointers: what the wrapper refuses above, the launcher and its form query refuse
    # too, with one message, before any launch
    import ctypes
    from conv_form_util import FAKE
    from qdiff import hip
    lib = hip.load()

    def desc(**fields):
        d = hip.ConvDesc()
        d.x = d.w = d.out = d.seg[0].scale = d.seg[0].zw = FAKE
        d.ldx, d.ldo = 64, 64
        d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = 1, 1, 4, 1, 4, 128
        d.kh, d.kw, d.stride = 1, 1, 1
        d.wbits, d.w_tiled, d.nseg, d.seg[0].clen = 4, 1, 1, 64
        d.epilogue, d.out_dtype = hip.EPI_GEGLU_H16, hip.F16
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    form = (ctypes.c_int32 * 4)()
    assert lib.qd_conv2d_wq_h16_form(ctypes.byref(desc()), hip.F16, form) == 0 and tuple(form) == (1, 0, 2, 0)
    for bad, needle in ((dict(out_dtype=hip.F32), "out_dtype must be act_dtype (operand rows)"),
                        (dict(out_dtype=hip.BF16), "out_dtype must be act_dtype (operand rows)"),
                        (dict(ldo=56), "ldo >= F"), (dict(ldo=68), "ldo % 8 == 0"),
                        (dict(residual=FAKE, ldr=64), "takes no residual and no rowbias"),
                        (dict(rowbias=FAKE, ld_rowbias=128), "takes no residual and no rowbias"),
                        (dict(Cout=80), "Cout = 2 F with F % 32 == 0 (Cout=80)"),
                        (dict(epilogue=hip.EPI_GEGLU_I8), "linear epilogue only"),
                        (dict(gn_part=FAKE), "linear epilogue only"), (dict(upsample2x=1), "linear epilogue only")):
        d = desc(**bad)
        assert lib.qd_conv2d_wq_h16_form(ctypes.byref(d), hip.F16, form) != 0, bad
        msg = lib.qd_last_error().decode()
        assert needle in msg, (bad, msg)
        assert lib.qd_conv2d_wq_h16(ctypes.byref(d), hip.F16, None) != 0 and lib.qd_last_error().decode() == msg, bad
