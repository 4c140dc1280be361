"""CPU tests (no GPU) of the fused weights-only route of the DDIM family (engine.WEIGHT_ONLY_FUSE_DDIM): the knob, which
blocks take the route and what they launch, every gate refusal, the wide head-dim predicate and the ctypes signature of
qd_attn_h16.  The entry points run on tests/wonly_fused_emulator.py and the fp64 attention of
tests/test_weight_only_attention_host.py."""
import os
import re
import subprocess
import sys
from collections import Counter

import pytest
import torch

import wonly_fused_emulator
from test_weight_only_attention_host import attn_h16_emulated
from test_weight_only_fused_host import _block_call, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"resblock": 0, "transformer": 0}


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine, hip
    calls = wonly_fused_emulator.install(monkeypatch)
    seen = []

    def attn(*a):
        calls.append("attn_h16")
        return attn_h16_emulated(*a, calls=seen)

    monkeypatch.setattr(hip, "attn_h16", attn)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_DDIM", False)
    monkeypatch.setattr(engine, "WONLY_FUSED", dict(BASE))
    engine.calls, engine.attn_calls = calls, seen
    yield engine
    del engine.calls, engine.attn_calls


def _run(engine, qnn, args, ddim, attn=None):
    engine.set_weight_only_fusion_ddim(ddim)
    engine.set_weight_only_attention(attn)
    engine.WONLY_FUSED.clear()
    engine.WONLY_FUSED.update(BASE)
    del engine.calls[:]
    with torch.no_grad():
        y = qnn(*args)
    return y, Counter(engine.calls), dict(engine.WONLY_FUSED)


def _blocks(qnn):
    from qdiff.quant_block import QuantAttnBlock, QuantResnetBlock
    return ([m for m in qnn.modules() if isinstance(m, QuantResnetBlock)], [m for m in qnn.modules() if isinstance(m, QuantAttnBlock)])


def _block_launches(engine, blk, a, k):
    n0, f0 = len(engine.calls), dict(engine.WONLY_FUSED)
    with torch.no_grad():
        y = blk(*a, **k)
    took = {key: v - f0.get(key, 0) for key, v in engine.WONLY_FUSED.items() if v != f0.get(key, 0)}
    return y, engine.calls[n0:], took


# ---- knob, predicates, signature ------------------------------------------------------------------------------------------
def test_knob_setter_and_state(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_FUSE_DDIM is False or os.environ.get("QDIFF_WEIGHT_ONLY_FUSE_DDIM")      # off by default
    for name in ("WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_FUSE"):
        monkeypatch.setattr(engine, name, False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    engine.set_weight_only_fusion_ddim("1")
    assert engine.WEIGHT_ONLY_FUSE_DDIM is True
    with torch.no_grad():
        assert not engine.wonly_ddim_state()                          # needs WEIGHT_ONLY_FUSE
        engine.set_weight_only_fusion(True)
        assert engine.wonly_ddim_state()
        monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", None)
        assert not engine.wonly_ddim_state()                          # and the layer knob
        monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_ddim_state()
    assert not engine.wonly_ddim_state()                              # autograd on
    engine.set_weight_only_fusion_ddim(False)
    assert engine.WEIGHT_ONLY_FUSE_DDIM is False
    with pytest.raises(ValueError):
        engine.set_weight_only_fusion_ddim(None)
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_FUSE_DDIM"):
        engine.set_weight_only_fusion_ddim("fp16")


def test_environment_variable():
    code = ("from qdiff import engine; print(engine.WEIGHT_ONLY_FUSE_DDIM, engine.WEIGHT_ONLY_FUSE, engine.wonly_ddim_state(), "
            "sorted(engine.WONLY_FUSED))")
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_FUSE_DDIM="1", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    for k in ("QDIFF_WEIGHT_ONLY", "QDIFF_WEIGHT_ONLY_FUSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "True False False ['resblock', 'transformer']"
    env["QDIFF_WEIGHT_ONLY_FUSE_DDIM"] = "maybe"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "QDIFF_WEIGHT_ONLY_FUSE_DDIM" in r.stderr


def test_wide_head_dims_are_the_new_routes_only():
    from qdiff import engine
    assert all(engine.wonly_attn_wide_shape_ok(d) for d in (8, 64, 168, 248, 256))
    assert not any(engine.wonly_attn_wide_shape_ok(d) for d in (4, 12, 260, 264))
    assert not engine.wonly_attn_shape_ok(256) and not engine.wonly_attn_shape_ok(168) and engine.WONLY_ATTN_DMAX == 160


def test_ctypes_signature_matches_the_header():
    """The parameters of qd_attn_h16 in include/qdiff_hip.h, kind by kind, are what qdiff.hip declares to ctypes (ABI 20, no new
    parameter), the header states the new range of d, and the argument checks that precede any device work accept d = 256 and
    refuse 264 (fake non-null pointers are never followed on this path)."""
    import ctypes
    from qdiff import hip
    lib = hip.load()
    hdr = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    proto = re.search(r"\nint qd_attn_h16\((.*?)\);", hdr, re.S).group(1)
    kind = lambda t: ctypes.c_void_p if "*" in t else {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[t.split()[0]]
    want = [kind(a.strip()) for a in proto.replace("\n", " ").split(",")]
    assert list(lib.qd_attn_h16.argtypes) == want and len(want) == 27
    assert "a multiple of 8 in [8, 256]" in hdr and "#define QD_ABI_VERSION 20" in hdr and lib.qd_abi_version() == 20
    st = lambda d: (16 * d, d, d, 1)

    def call(d, scale):
        return lib.qd_attn_h16(64, 64, 64, 1, 1, 16, 16, 1, d, *st(d), *st(d), *st(d), scale, 1, 64, 0, d, None)

    assert call(264, 1.0) != 0 and "[8, 256]" in lib.qd_last_error().decode()
    assert call(4, 1.0) != 0 and "[8, 256]" in lib.qd_last_error().decode()
    assert call(256, 0.0) != 0 and "scale" in lib.qd_last_error().decode()          # d = 256 passed the range check


# ---- the model on the route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", [None, torch.float16], ids=["library_attention", "attn_h16"])
def test_cifar_takes_the_route(emu, attn):
    """cifar_tiny in state (True, False), fp16 operands.  Every QuantResnetBlock, every QuantAttnBlock and the head count once.
    Launches: two qd_groupnorm_h16 per residual block, one per attention block, one for the head; the contractions are
    unchanged; of the qd_rows_to_h16 passes there go two per residual block, the three of q / k / v and the head's, and with
    the attention kernel proj_out's too (its fp16 operand rows come from the kernel).
    Agreement with the knob-off run: both round the same operands at the same sites, the fused run evaluating the glue in
    fp64 (emulator) and the unfused one in fp32 (library), so a rounding can land on the neighbouring fp16 value: to first order
    one ulp (2^-10) of the range per producer call.  The attention kernel adds four roundings per block that the fp32 library
    attention does not have (q, k, v and P to fp16): 2^-10 each, by the same rule."""
    qnn, args = _model("cifar_tiny")
    res, att = _blocks(qnn)
    assert len(res) > 0 and len(att) > 0
    y0, c0, f0 = _run(emu, qnn, args, False, attn)
    y1, c1, f1 = _run(emu, qnn, args, True, attn)
    assert f0 == BASE and "attn_h16" not in c0 and "groupnorm_h16" not in c0
    assert f1 == dict(BASE, resnetblock=len(res), attnblock_ddim=len(att), head_ddim=1)
    assert c1["groupnorm_h16"] == 2 * len(res) + len(att) + 1
    assert c1["conv2d_wq_h16"] == c0["conv2d_wq_h16"]
    assert c1["attn_h16"] == (len(att) if attn else 0)
    assert c1["rows_to_h16"] == c0["rows_to_h16"] - 2 * len(res) - (4 if attn else 3) * len(att) - 1
    if attn:
        call = emu.attn_calls[0]
        C, T = att[0].in_channels, call["T"]
        assert (call["H"], call["d"], call["S"]) == (1, C, T) and call["scale"] == C ** -0.5
        assert all(call[n][1] == (T * C, C, C, 1) and call[n][0].dtype == torch.float16 for n in "qkv")
    sites = c1["groupnorm_h16"] + 4 * c1["attn_h16"]
    rng = y0.abs().max().item()
    d = (y1 - y0).abs().max().item() / rng
    print(f"\n[cifar_tiny, attention {attn}] fused vs knob off on the emulator: {d:.3e} of range, bound {sites} x 2^-10 = {sites * 2.0 ** -10:.3e}")
    assert y1.dtype == y0.dtype and y1.shape == y0.shape and y1.stride() == y0.stride()
    assert 0 < d <= sites * 2.0 ** -10


def test_launch_list_per_block(emu):
    qnn, args = _model("cifar_tiny")
    res, att = _blocks(qnn)
    same = next(b for b in res if b.in_channels == b.out_channels)
    wider = next(b for b in res if b.in_channels != b.out_channels)
    calls = {id(b): _block_call(qnn, args, b) for b in (same, wider, att[0])}
    emu.set_weight_only_fusion_ddim(True)
    emu.set_weight_only_attention(torch.float16)
    _, seq, took = _block_launches(emu, same, *calls[id(same)])
    # temb_proj keeps its module call (its own qd_rows_to_h16 and contraction); conv1 and conv2 have no qd_rows_to_h16 left
    assert seq == ["groupnorm_h16", "rows_to_h16", "conv2d_wq_h16", "conv2d_wq_h16", "groupnorm_h16", "conv2d_wq_h16"]
    assert took == {"resnetblock": 1}
    _, seq, took = _block_launches(emu, wider, *calls[id(wider)])
    assert Counter(seq)["groupnorm_h16"] == 2 and Counter(seq)["conv2d_wq_h16"] == 4 and took == {"resnetblock": 1}
    assert Counter(seq)["rows_to_h16"] >= 2                          # temb_proj's, and the shortcut's (one pass per segment)
    _, seq, took = _block_launches(emu, att[0], *calls[id(att[0])])
    assert seq == ["groupnorm_h16"] + ["conv2d_wq_h16"] * 3 + ["attn_h16", "conv2d_wq_h16"] and took == {"attnblock_ddim": 1}
    emu.set_weight_only_attention(None)                                # library attention: the rest of the route is still fused
    _, seq, took = _block_launches(emu, att[0], *calls[id(att[0])])
    assert seq == ["groupnorm_h16"] + ["conv2d_wq_h16"] * 3 + ["rows_to_h16", "conv2d_wq_h16"] and took == {"attnblock_ddim": 1}


def test_width_the_kernel_refuses_keeps_the_library_attention_inside_the_route(emu, monkeypatch):
    qnn, args = _model("cifar_tiny")
    _, att = _blocks(qnn)
    a, k = _block_call(qnn, args, att[0])
    emu.set_weight_only_fusion_ddim(True)
    emu.set_weight_only_attention(torch.float16)
    monkeypatch.setattr(emu, "WONLY_ATTN_WIDE_DMAX", 32)
    _, seq, took = _block_launches(emu, att[0], a, k)
    assert "attn_h16" not in seq and seq.count("groupnorm_h16") == 1 and took == {"attnblock_ddim": 1}


# ---- knob off, and the knob without the knobs below it --------------------------------------------------------------------------
def test_knob_off_is_the_route_before(emu):
    """Knob off (every other weights-only knob on): the call sequence is one qd_rows_to_h16 per segment and one contraction
    per QuantModule, the counters have no new key, no attention launch, and the bytes are those of block fusion off."""
    import qdiff
    qnn, args = _model("cifar_tiny")
    y0, c0, f0 = _run(emu, qnn, args, False, torch.float16)
    assert set(c0) == {"rows_to_h16", "conv2d_wq_h16"} and f0 == BASE and not emu.attn_calls
    assert c0["conv2d_wq_h16"] == sum(isinstance(m, qdiff.QuantModule) for m in qnn.modules())
    emu.set_weight_only_fusion(False)
    y_ref, c_ref, f_ref = _run(emu, qnn, args, False, None)
    assert torch.equal(y0, y_ref) and c_ref == c0 and f_ref == BASE


@pytest.mark.parametrize("missing", ["fuse", "weight_only"])
def test_knob_alone_changes_nothing(emu, monkeypatch, missing):
    qnn, args = _model("cifar_tiny")
    if missing == "fuse":
        emu.set_weight_only_fusion(False)
    else:
        monkeypatch.setattr(emu, "WEIGHT_ONLY_KERNEL", None)
    y0, c0, f0 = _run(emu, qnn, args, False, torch.float16)
    y1, c1, f1 = _run(emu, qnn, args, True, torch.float16)
    assert torch.equal(y0, y1) and c0 == c1 and f0 == f1 == BASE and not emu.attn_calls


# ---- gate refusals -----------------------------------------------------------------------------------------------------------
def _refusal(engine, blk, a, k, key):
    """(output, new launches, counter increments) of one block call; asserts that nothing of the route ran."""
    y, seq, took = _block_launches(engine, blk, a, k)
    assert "groupnorm_h16" not in seq and "attn_h16" not in seq and took == {}, (key, seq, took)
    return y


def test_gate_refusals_keep_todays_path_for_that_block(emu, monkeypatch):
    from qdiff import engine
    qnn, args = _model("cifar_tiny")
    res, att = _blocks(qnn)
    rb, ab = res[2], att[0]
    ra, rk = _block_call(qnn, args, rb)
    aa, ak = _block_call(qnn, args, ab)
    engine.set_weight_only_attention(torch.float16)
    off = {}
    for key, blk, a, k in (("res", rb, ra, rk), ("att", ab, aa, ak)):
        engine.set_weight_only_fusion_ddim(False)
        off[key] = _refusal(engine, blk, a, k, key)
        engine.set_weight_only_fusion_ddim(True)
        assert _block_launches(engine, blk, a, k)[2] == {"resnetblock" if key == "res" else "attnblock_ddim": 1}

    # a hook on q: that attention block only, inside the model
    fired = []
    h = ab.q.register_forward_hook(lambda m, i, o: fired.append(1))
    try:
        assert torch.equal(_refusal(engine, ab, aa, ak, "hook"), off["att"]) and fired == [1]
        _, _, f = _run(engine, qnn, args, True, torch.float16)
        assert f == dict(BASE, resnetblock=len(res), attnblock_ddim=len(att) - 1, head_ddim=1)
    finally:
        h.remove()
    engine.set_weight_only_fusion_ddim(True)
    engine.set_weight_only_attention(torch.float16)
    # live dropout
    rb.dropout.p, rb.training = 0.5, True
    rb.__dict__.pop("_qd_has_dropout", None)
    try:
        torch.manual_seed(1)
        y = _refusal(engine, rb, ra, rk, "dropout")
        engine.set_weight_only_fusion_ddim(False)
        torch.manual_seed(1)
        assert torch.equal(y, _refusal(engine, rb, ra, rk, "dropout off"))
    finally:
        rb.dropout.p, rb.training = 0.0, False
        rb.__dict__.pop("_qd_has_dropout", None)
    engine.set_weight_only_fusion_ddim(True)
    # use_act_quant on the attention block: the quantisers of the reference's composition see their inputs
    ab.use_act_quant = True
    try:
        y = _refusal(engine, ab, aa, ak, "use_act_quant")
        engine.set_weight_only_fusion_ddim(False)
        assert torch.equal(y, _refusal(engine, ab, aa, ak, "use_act_quant off"))
    finally:
        ab.use_act_quant = False
    engine.set_weight_only_fusion_ddim(True)
    # autocast
    with torch.autocast("cpu", dtype=torch.bfloat16):
        ys = [_refusal(engine, blk, a, k, "autocast") for blk, a, k in ((rb, ra, rk), (ab, aa, ak))]
        engine.set_weight_only_fusion_ddim(False)
        assert all(torch.equal(y, _refusal(engine, blk, a, k, "autocast off")) for y, (blk, a, k) in zip(ys, ((rb, ra, rk), (ab, aa, ak))))
    engine.set_weight_only_fusion_ddim(True)
    # a CPU tensor with the real device predicate (every layer then runs the library path)
    monkeypatch.setattr(engine, "wonly_device_ok", lambda t: t.is_cuda)
    ys = [_refusal(engine, blk, a, k, "cpu") for blk, a, k in ((rb, ra, rk), (ab, aa, ak))]
    engine.set_weight_only_fusion_ddim(False)
    assert all(torch.equal(y, _refusal(engine, blk, a, k, "cpu off")) for y, (blk, a, k) in zip(ys, ((rb, ra, rk), (ab, aa, ak))))
    monkeypatch.setattr(engine, "wonly_device_ok", lambda t: True)
    engine.set_weight_only_fusion_ddim(True)
    assert _block_launches(engine, rb, ra, rk)[2] == {"resnetblock": 1} and _block_launches(engine, ab, aa, ak)[2] == {"attnblock_ddim": 1}
    # the head: a hook on conv_out keeps its module call
    h = qnn.model.conv_out.register_forward_hook(lambda m, i, o: fired.append(2))
    try:
        _, _, f = _run(engine, qnn, args, True, torch.float16)
        assert "head_ddim" not in f and fired[-1] == 2
    finally:
        h.remove()


def test_channel_count_that_is_no_multiple_of_8(emu, monkeypatch):
    """Blocks of 12 channels (GroupNorm over 4 groups): the producers write runs of 8 channels, so both blocks keep today's
    path bit for bit."""
    import qdiff
    from qdiff.arch import ddim_unet
    from qdiff.quant_block import QuantAttnBlock, QuantResnetBlock
    monkeypatch.setattr(ddim_unet, "Normalize", lambda c: torch.nn.GroupNorm(4, c, eps=1e-6))
    wq = dict(n_bits=8, channel_wise=True, scale_method="max")
    aq = dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True)
    torch.manual_seed(5)

    def quantised(block):
        for name, child in list(block.named_children()):
            if isinstance(child, (torch.nn.Conv2d, torch.nn.Linear)):
                setattr(block, name, qdiff.QuantModule(child, wq, aq))
        return block

    rb = QuantResnetBlock(quantised(ddim_unet.ResnetBlock(in_channels=12, out_channels=12, dropout=0.0, temb_channels=16)), aq).eval()
    ab = QuantAttnBlock(quantised(ddim_unet.AttnBlock(12)), aq).eval()
    x, temb = torch.randn(2, 12, 4, 4), torch.randn(2, 16)
    for blk, a in ((rb, (x, temb)), (ab, (x,))):
        for m in blk.modules():
            if isinstance(m, (qdiff.QuantModule, type(blk))):
                m.set_quant_state(True, False)
        emu.set_weight_only_fusion_ddim(False)
        y0 = _refusal(emu, blk, a, {}, "off")
        emu.set_weight_only_fusion_ddim(True)
        assert torch.equal(_refusal(emu, blk, a, {}, "C = 12"), y0)
