"""CPU tests (no GPU) of the one-launch embedding Linears of the weights-only state (engine.WEIGHT_ONLY_TEMB,
qd_temb_mlp_wq_h16): the knob, the launch census of the four model families, every gate refusal, the slice a scale-shift block
receives, the ctypes signature and the argument checks of the C entry.  The entry points run on tests/wonly_temb_emulator.py."""
import ctypes
import os
import re
import subprocess
import sys
from collections import Counter

import pytest
import torch
import torch.nn as nn

import wonly_temb_emulator
from test_weight_only_fused_host import _block_call, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cifar_tiny", "ldm_tiny", "sd_tiny", "ldm_updown_tiny"]


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine, hip
    calls = wonly_temb_emulator.install(monkeypatch)
    ptrs = []
    inner = hip.conv2d_wq_h16

    def conv(c, act_dtype):
        ptrs.append(c.w.data_ptr())
        return inner(c, act_dtype)

    monkeypatch.setattr(hip, "conv2d_wq_h16", conv)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    for name in ("WEIGHT_ONLY_ATTN", ):
        monkeypatch.setattr(engine, name, None)
    for name in ("WEIGHT_ONLY_FUSE", "WEIGHT_ONLY_FUSE_WIDE", "WEIGHT_ONLY_FUSE_MOD", "WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_SPLITK",
                 "WEIGHT_ONLY_TEMB"):
        monkeypatch.setattr(engine, name, False)
    monkeypatch.setattr(engine, "WONLY_TEMB", [0])
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    engine.calls, engine.w_ptrs = calls, ptrs
    yield engine
    del engine.calls, engine.w_ptrs


def _emb_linears(qnn):
    """(the members of the model's EmbGroup as (block, Linear), the two Linears of the timestep MLP)."""
    from qdiff.quant_block import QuantResBlock, QuantResnetBlock
    mem = []
    for m in qnn.modules():
        if isinstance(m, QuantResBlock):
            mem.append((m, m.emb_layers[-1]))
        elif isinstance(m, QuantResnetBlock):
            mem.append((m, m.temb_proj))
    te = getattr(qnn.model, "time_embed", None)
    mlp = (te[0], te[2]) if te is not None else tuple(qnn.model.temb.dense)
    return mem, mlp


def _run(engine, qnn, args, temb, **ctx):
    engine.set_weight_only_temb(temb)
    engine.WONLY_TEMB[0] = 0
    del engine.calls[:], engine.w_ptrs[:]
    with torch.no_grad():
        y = qnn(*args)
    return y, Counter(engine.calls), Counter(engine.w_ptrs), engine.WONLY_TEMB[0]


def _w_ptrs(lins):
    with torch.no_grad():
        return [l.wonly_plan().pack.wq.data_ptr() for l in lins]


# ---- knob, signature, argument checks ---------------------------------------------------------------------------------------
def test_knob_setter_and_state(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_TEMB is False or os.environ.get("QDIFF_WEIGHT_ONLY_TEMB")      # off by default
    monkeypatch.setattr(engine, "WEIGHT_ONLY_TEMB", False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "SIMULATE", False)
    engine.set_weight_only_temb("1")
    assert engine.WEIGHT_ONLY_TEMB is True
    with torch.no_grad():
        assert engine.wonly_temb_state()
        monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", None)
        assert not engine.wonly_temb_state()                          # needs the layer knob
        monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.bfloat16)
        monkeypatch.setattr(engine, "SIMULATE", True)
        assert not engine.wonly_temb_state()
        monkeypatch.setattr(engine, "SIMULATE", False)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_temb_state()
    assert not engine.wonly_temb_state()                              # autograd on
    engine.set_weight_only_temb(False)
    assert engine.WEIGHT_ONLY_TEMB is False
    with pytest.raises(ValueError):
        engine.set_weight_only_temb(None)
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_TEMB"):
        engine.set_weight_only_temb("fp16")


def test_environment_variable():
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_TEMB, engine.WEIGHT_ONLY_KERNEL, engine.wonly_temb_state(), engine.WONLY_TEMB)"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_TEMB="1", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "True None False [0]"
    env["QDIFF_WEIGHT_ONLY_TEMB"] = "maybe"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "QDIFF_WEIGHT_ONLY_TEMB" in r.stderr


def test_ctypes_signature_matches_the_header_and_the_entry_checks_its_arguments():
    """The parameters of qd_temb_mlp_wq_h16 in include/qdiff_hip.h, kind by kind, are what qdiff.hip declares to ctypes; the ABI
    version stays 20; the argument checks that precede any device work are reachable without a GPU (fake non-null pointers
    are never followed on this path)."""
    from qdiff import hip
    lib = hip.load()
    hdr = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    proto = re.search(r"\nint qd_temb_mlp_wq_h16\((.*?)\);", hdr, re.S).group(1)
    kind = lambda t: ctypes.c_void_p if "*" in t else {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[t.split()[0]]
    want = [kind(a.strip()) for a in proto.replace("\n", " ").split(",")]
    assert list(lib.qd_temb_mlp_wq_h16.argtypes) == want and len(want) == 14
    assert "qd_temb_mlp_wq_h16" in hip.EXPORTS
    assert "#define QD_ABI_VERSION 20" in hdr and lib.qd_abi_version() == 20
    assert ctypes.sizeof(hip._TembWqLayer) == 40

    def call(x=64, ldx=32, B=2, K=32, layers=64, wbits=4, dt=hip.F16, blocks=64, out=64):
        rc = lib.qd_temb_mlp_wq_h16(x, ldx, B, K, 1, layers, 1, blocks, 1, wbits, dt, out, 64, None)
        return rc, lib.qd_last_error().decode()

    for kw, word in ((dict(K=24, ldx=24), "multiple of 16"), (dict(x=68), "16-byte aligned"), (dict(ldx=34), "16-byte aligned"),
                     (dict(wbits=5), "wbits"), (dict(dt=hip.F32), "f16/bf16"), (dict(B=0), "bad shape"), (dict(layers=None), "null")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


# ---- the four families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_layer_is_ready_and_three_launches_replace_the_embedding_contractions(emu, name):
    """State (True, False), fp16 operands.  Every QuantModule takes the weights-only kernel (the GPU tests rest on this).
    Knob on: three qd_temb_mlp_wq_h16 launches per evaluation (two for the timestep MLP, one for all blocks), and the
    contractions and qd_rows_to_h16 passes of those Linears are gone from the census — nothing else moves.  The output agrees
    with the knob-off run to the rounding of the embedding operands: both round SiLU(emb) once to fp16, the emulated launch
    from an fp64 SiLU and the module from torch's fp32 one."""
    import qdiff
    qnn, args = _model(name)
    mods = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)]
    with torch.no_grad():
        assert all(m.wonly_ready() for m in mods)
    mem, mlp = _emb_linears(qnn)
    emb_w = set(_w_ptrs([l for _, l in mem] + list(mlp)))
    assert len(emb_w) == len(mem) + 2 and len(mem) >= 2
    y0, c0, w0, n0 = _run(emu, qnn, args, False)
    y1, c1, w1, n1 = _run(emu, qnn, args, True)
    assert n0 == 0 and "temb_mlp_wq_h16" not in c0 and all(w0[p] == 1 for p in emb_w)
    assert n1 == 3 and c1["temb_mlp_wq_h16"] == 3
    assert not any(p in w1 for p in emb_w)
    assert c1["conv2d_wq_h16"] == c0["conv2d_wq_h16"] - len(emb_w) and c1["rows_to_h16"] == c0["rows_to_h16"] - len(emb_w)
    assert {p: n for p, n in w0.items() if p not in emb_w} == dict(w1)
    assert y1.dtype == y0.dtype and y1.shape == y0.shape
    d = (y1 - y0).abs().max().item() / y0.abs().max().item()
    print(f"\n[{name}] knob on vs off on the emulator: {d:.3e} of range, {len(mem)} members")
    assert d <= 2.0 ** -10 * (len(mem) + 2)
    y2, c2, w2, n2 = _run(emu, qnn, args, False)
    assert torch.equal(y2, y0) and c2 == c0 and w2 == w0 and n2 == 0


def test_scale_shift_block_receives_both_halves(emu):
    """ldm_updown_tiny: the slice handed to a `use_scale_shift_norm` block is fp32 [B][2 C] with unit column stride, and equals
    the block's own projection to the rounding of the emulator's fp64 SiLU."""
    qnn, args = _model("ldm_updown_tiny")
    from qdiff.quant_block import QuantResBlock
    blk = next(m for m in qnn.modules() if isinstance(m, QuantResBlock) and m.use_scale_shift_norm)
    a, _ = _block_call(qnn, args, blk)
    emb = a[1]
    emu.set_weight_only_temb(True)
    grp = blk.__dict__["_emb_group"]
    grp.reset()
    with torch.no_grad():
        e = grp.get(blk, emb)
        ref = blk.emb_layers(emb)
    assert e is not None and e.dtype == torch.float32 and e.stride(1) == 1
    assert tuple(e.shape) == (emb.shape[0], 2 * blk.out_channels) == tuple(ref.shape)
    assert (e - ref).abs().max().item() <= 2.0 ** -9 * ref.abs().max().item()
    assert emu.WONLY_TEMB[0] == 1


# ---- gate refusals ----------------------------------------------------------------------------------------------------------
def test_knob_off_changes_nothing(emu):
    qnn, args = _model("ldm_tiny")
    y0, c0, w0, n0 = _run(emu, qnn, args, False)
    assert n0 == 0 and "temb_mlp_wq_h16" not in c0 and set(c0) == {"rows_to_h16", "conv2d_wq_h16"}
    import qdiff
    assert c0["conv2d_wq_h16"] == sum(isinstance(m, qdiff.QuantModule) for m in qnn.modules())


def _refused(emu, qnn, args, enter=None):
    """Knob on under a refusing condition: no launch, every embedding contraction in place, the bytes of the knob-off run."""
    mem, mlp = _emb_linears(qnn)
    emb_w = set(_w_ptrs([l for _, l in mem] + list(mlp))) if emu.WEIGHT_ONLY_KERNEL is not None else set()

    def run(on):
        emu.set_weight_only_temb(on)
        emu.WONLY_TEMB[0] = 0
        del emu.calls[:], emu.w_ptrs[:]
        y = enter(lambda: qnn(*args)) if enter else qnn(*args)
        return y, Counter(emu.w_ptrs), emu.WONLY_TEMB[0]

    y0, w0, n0 = run(False)
    y1, w1, n1 = run(True)
    assert n0 == 0 and n1 == 0 and torch.equal(y0.detach(), y1.detach()) and w0 == w1
    return w1, emb_w


def test_layer_knob_off_refuses(emu):
    qnn, args = _model("ldm_tiny")
    emu.set_weight_only_kernel(None)
    with torch.no_grad():
        w, _ = _refused(emu, qnn, args)
    assert not w                                                      # library path: no weights-only contraction at all


def test_autocast_refuses(emu):
    qnn, args = _model("ldm_tiny")

    def enter(f):
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            return f()

    w, emb_w = _refused(emu, qnn, args, enter)
    assert all(w[p] == 1 for p in emb_w)


def test_autograd_refuses(emu):
    qnn, args = _model("ldm_tiny")
    _refused(emu, qnn, args)                                           # no torch.no_grad(): the layers keep the library path


def test_simulation_refuses(emu, monkeypatch):
    qnn, args = _model("ldm_tiny")
    monkeypatch.setattr(emu, "SIMULATE", True)
    with torch.no_grad():
        _refused(emu, qnn, args)


@pytest.mark.parametrize("where", ["member", "container"])
def test_hooked_module_keeps_seeing_its_calls(emu, where):
    """A forward hook on one member Linear, or on the `emb_layers` container around it: the whole group answers None, every
    block keeps its own projection, and the hook fires once per evaluation.  The timestep MLP (not hooked) still takes its
    two launches."""
    qnn, args = _model("ldm_tiny")
    mem, mlp = _emb_linears(qnn)
    blk, lin = mem[1]
    fired = []
    h = (lin if where == "member" else blk.emb_layers).register_forward_hook(lambda m, a, o: fired.append(1))
    try:
        y1, c1, w1, n1 = _run(emu, qnn, args, True)
    finally:
        h.remove()
    assert len(fired) == 1 and n1 == 2
    assert all(w1[p] == 1 for p in _w_ptrs([l for _, l in mem]))
    assert not any(p in w1 for p in _w_ptrs(mlp))
    y2, c2, w2, n2 = _run(emu, qnn, args, True)
    assert n2 == 3 and len(fired) == 1


def test_hooked_timestep_linear_keeps_the_composition(emu):
    qnn, args = _model("ldm_tiny")
    mem, mlp = _emb_linears(qnn)
    fired = []
    h = mlp[1].register_forward_pre_hook(lambda m, a: fired.append(1))
    try:
        y1, c1, w1, n1 = _run(emu, qnn, args, True)
    finally:
        h.remove()
    assert len(fired) == 1 and n1 == 1 and all(w1[p] == 1 for p in _w_ptrs(mlp))


class _Blk:
    """A stand-in for a residual block: EmbGroup keeps its handle in the block's __dict__."""
    emb_layers = None


def _group(specs, K=32, per_channel=True):
    """A free-standing EmbGroup over QuantModule Linears K -> Cout of the given weight widths, state (True, False)."""
    import qdiff
    from qdiff.quant_block import EmbGroup
    grp, lins, blks = EmbGroup(), [], []
    torch.manual_seed(3)
    for wbits, Cout in specs:
        m = qdiff.QuantModule(nn.Linear(K, Cout), dict(n_bits=wbits, channel_wise=per_channel, scale_method="max"),
                              dict(n_bits=8, channel_wise=False, scale_method="max"))
        m.set_quant_state(True, False)
        b = _Blk()
        grp.register(b, m)
        lins.append(m)
        blks.append(b)
    return grp, lins, blks


def _ask(emu, grp, blks, emb):
    emu.set_weight_only_temb(True)
    emu.WONLY_TEMB[0] = 0
    grp.reset()
    with torch.no_grad():
        return [grp.get(b, emb) for b in blks], emu.WONLY_TEMB[0]


def test_free_standing_group_runs_and_each_shape_refusal_answers_none(emu):
    emb = torch.randn(3, 32)
    grp, lins, blks = _group([(4, 40), (4, 70)])
    es, n = _ask(emu, grp, blks, emb)
    assert n == 1 and [tuple(e.shape) for e in es] == [(3, 40), (3, 70)]
    with torch.no_grad():
        for e, l in zip(es, lins):
            ref = l(torch.nn.functional.silu(emb))
            assert (e - ref).abs().max().item() <= 2.0 ** -9 * ref.abs().max().item()
    # the columns between the slices belong to nobody: padded to 64
    assert grp._offs[id(blks[1])] == (64, 70) and grp._out.shape[1] == 64 + 128
    for bad in (emb.double(), emb.half(), emb[0], emb.view(1, 3, 32)):           # a 2-D fp32 tensor only
        assert _ask(emu, grp, blks, bad) == ([None, None], 0)
    es, n = _ask(emu, grp, blks, emb)
    assert n == 1 and all(e is not None for e in es)                              # (and back)


def test_input_width_not_a_multiple_of_16_refuses(emu):
    from qdiff.quant_block import time_mlp
    grp, lins, blks = _group([(4, 40), (4, 48)], K=24)
    emb = torch.randn(2, 24)
    assert _ask(emu, grp, blks, emb) == ([None, None], 0)
    # the timestep MLP likewise: its first Linear reads 24 features -> the plain composition, the same bytes
    g2, l2, _ = _group([(4, 24)], K=48)
    x = torch.randn(2, 48)
    emu.WONLY_TEMB[0] = 0
    with torch.no_grad():
        y = time_mlp(l2[0], lins[0], x)
        assert emu.WONLY_TEMB[0] == 0 and torch.equal(y, lins[0](torch.nn.functional.silu(l2[0](x))))
        _, l3, _ = _group([(4, 32)], K=40)
        x = torch.randn(2, 24)
        y = time_mlp(lins[0], l3[0], x)                                          # K = 24 in front
        assert emu.WONLY_TEMB[0] == 0 and torch.equal(y, l3[0](torch.nn.functional.silu(lins[0](x))))


def test_timestep_mlp_takes_two_launches(emu):
    from qdiff.quant_block import time_mlp
    _, (l0,), _ = _group([(4, 64)], K=32)
    _, (m1,), _ = _group([(4, 48)], K=64)
    x = torch.randn(5, 32)
    emu.set_weight_only_temb(True)
    emu.WONLY_TEMB[0] = 0
    with torch.no_grad():
        y = time_mlp(l0, m1, x)
        ref = m1(torch.nn.functional.silu(l0(x)))
    assert emu.WONLY_TEMB[0] == 2 and tuple(y.shape) == (5, 48) and y.dtype == torch.float32
    assert (y - ref).abs().max().item() <= 2.0 ** -9 * ref.abs().max().item()


def test_mixed_weight_widths_refuse(emu):
    grp, lins, blks = _group([(4, 40), (8, 40)])
    assert _ask(emu, grp, blks, torch.randn(2, 32)) == ([None, None], 0)


def test_member_that_is_not_ready_refuses(emu):
    """A per-tensor weight quantiser (the packer refuses it): the member keeps the library path, and so does the group."""
    grp, lins, blks = _group([(4, 40), (4, 40)])
    g2, l2, b2 = _group([(4, 40)], per_channel=False)
    with torch.no_grad():
        assert not l2[0].wonly_ready()
    grp.register(b2[0], l2[0])
    assert _ask(emu, grp, blks + b2, torch.randn(2, 32)) == ([None, None, None], 0)


def test_split_member_refuses(emu):
    grp, lins, blks = _group([(4, 40), (4, 40)])
    lins[1].split = 16
    assert _ask(emu, grp, blks, torch.randn(2, 32)) == ([None, None], 0)


def test_single_member_refuses(emu):
    grp, lins, blks = _group([(4, 40)])
    assert _ask(emu, grp, blks, torch.randn(2, 32)) == ([None], 0)


def test_wrapper_refuses_what_the_kernel_cannot_read(monkeypatch):
    """qdiff.hip.temb_mlp_wq_h16 itself (not emulated here): the host checks in front of the C entry."""
    import wonly_emulator
    from qdiff import engine, hip
    wonly_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    grp, lins, blks = _group([(4, 40), (4, 40)])
    with torch.no_grad():
        plans = [l.wonly_plan() for l in lins]
    x, out = torch.randn(2, 32), torch.empty(2, 128)
    with pytest.raises(hip.HipEngineError, match="float16 or bfloat16"):
        hip.temb_mlp_wq_h16(x, True, plans, [0, 64], out, torch.float32)
    with pytest.raises(hip.HipEngineError, match="operand type"):
        hip.temb_mlp_wq_h16(x, True, plans, [0, 64], out, torch.bfloat16)
    with pytest.raises(hip.HipEngineError, match="outside the output rows"):
        hip.temb_mlp_wq_h16(x, True, plans, [0, 100], out, torch.float16)
    with pytest.raises(hip.HipEngineError, match="fp32 rows"):
        hip.temb_mlp_wq_h16(x.double(), True, plans, [0, 64], out, torch.float16)
