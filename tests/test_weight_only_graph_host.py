"""CPU tests (no GPU) of the host logic behind HIP-graph replay of weights-only evaluations (engine.WEIGHT_ONLY_GRAPH):
QuantModel._wonly_token, the graph key, the pool handle, and the integer-only features a weights-only evaluation must never
take.  The entry points run on tests/wonly_temb_emulator.py; captures themselves are tested on the GPU
(tests/test_weight_only_graph_gpu.py)."""
import os
import subprocess
import sys

import pytest
import torch

import wonly_temb_emulator
from test_weight_only_fused_host import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("WEIGHT_ONLY_FUSE", "WEIGHT_ONLY_FUSE_WIDE", "WEIGHT_ONLY_FUSE_MOD", "WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_SPLITK",
         "WEIGHT_ONLY_TEMB")


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    wonly_temb_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    for name in FLAGS:
        monkeypatch.setattr(engine, name, False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_GRAPH", True)
    monkeypatch.setattr(engine, "WONLY_TEMB", [0])
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    return engine


def test_knob_and_environment_variable(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_GRAPH is False or os.environ.get("QDIFF_WEIGHT_ONLY_GRAPH")    # off by default
    monkeypatch.setattr(engine, "WEIGHT_ONLY_GRAPH", False)
    engine.set_weight_only_graph("on")
    assert engine.WEIGHT_ONLY_GRAPH is True
    engine.set_weight_only_graph(False)
    assert engine.WEIGHT_ONLY_GRAPH is False
    with pytest.raises(ValueError):
        engine.set_weight_only_graph(None)
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_GRAPH"):
        engine.set_weight_only_graph("fp16")
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_GRAPH, engine.WEIGHT_ONLY_TEMB)"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_GRAPH="1", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY_TEMB", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "True False"
    env["QDIFF_WEIGHT_ONLY_GRAPH"] = "maybe"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "QDIFF_WEIGHT_ONLY_GRAPH" in r.stderr


@pytest.mark.parametrize("name", ["cifar_tiny", "sd_tiny"])
def test_token_is_minus_one_outside_the_weights_only_state(emu, name):
    qnn, args = _model(name)
    with torch.no_grad():
        assert qnn._wonly_token() >= 0
        for state in ((True, True), (False, False), (False, True)):
            qnn.set_quant_state(*state)
            assert qnn._wonly_token() == -1, state
        qnn.set_quant_state(True, False)
        t0 = qnn._wonly_token()
        assert t0 >= 0
        emu.set_weight_only_graph(False)
        assert qnn._wonly_token() == -1                                  # the knob
        emu.set_weight_only_graph(True)
        assert qnn._wonly_token() == t0
        emu.set_weight_only_kernel(None)
        assert qnn._wonly_token() == -1                                  # the layer knob
        emu.set_weight_only_kernel(torch.float16)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert qnn._wonly_token() == -1
        qnn.model.train()
        assert qnn._wonly_token() == -1
        qnn.model.eval()
        emu.SIMULATE, sim = True, emu.SIMULATE
        try:
            assert qnn._wonly_token() == -1
        finally:
            emu.SIMULATE = sim
        assert qnn._wonly_token() == t0
    assert qnn._wonly_token() == -1                                      # autograd on
    assert qnn._state_token() == -1                                      # and the integer token never answered for this state


def test_refused_layer_keeps_the_whole_model_eager(emu):
    """One QuantModule with a per-tensor weight quantiser (the packer refuses it): the token is -1."""
    import qdiff
    from qdiff.quant_layer import UniformAffineQuantizer
    qnn, args = _model("ldm_tiny")
    with torch.no_grad():
        assert qnn._wonly_token() >= 0
        m = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)][3]
        m.weight_quantizer = UniformAffineQuantizer(n_bits=4, channel_wise=False, scale_method="max")
        assert not m.wonly_ready()
        assert qnn._wonly_token() == -1


def test_token_moves_with_the_weights_and_not_with_the_knobs(emu):
    import qdiff
    qnn, args = _model("ldm_tiny")
    with torch.no_grad():
        t0 = qnn._wonly_token()
        assert t0 >= 0 and qnn._wonly_token() == t0
        k0 = qnn._wonly_graph_key()
        keys = {k0}
        # every weights-only knob: the token stays, the graph key moves
        emu.set_weight_only_attention(torch.float16)
        for setter in (emu.set_weight_only_fusion, emu.set_weight_only_fusion_wide, emu.set_weight_only_splitk,
                       emu.set_weight_only_fusion_mod, emu.set_weight_only_fusion_ddim, emu.set_weight_only_temb):
            assert qnn._wonly_token() == t0
            keys.add(qnn._wonly_graph_key())
            setter(True)
        assert qnn._wonly_token() == t0
        keys.add(qnn._wonly_graph_key())
        assert len(keys) == 8 and all(k[0] == "wonly" and len(k) == 9 for k in keys)
        emu.set_weight_only_kernel(torch.bfloat16)                       # (4-bit codes: every layer is a bf16 layer too)
        assert qnn._wonly_token() == t0 and qnn._wonly_graph_key() not in keys
        emu.set_weight_only_kernel(torch.float16)
        m = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)][2]
        m.weight_quantizer.delta = m.weight_quantizer.delta.clone() * 1.5          # re-assigned quantiser parameter
        t1 = qnn._wonly_token()
        assert t1 >= 0 and t1 != t0
        m.weight.mul_(0.5)                                                         # in-place weight edit
        t2 = qnn._wonly_token()
        assert t2 >= 0 and t2 not in (t0, t1)
        assert qnn._wonly_token() == t2
        qnn.invalidate_plans()
        assert qnn._wonly_token() >= 0


def test_weights_only_evaluation_takes_no_integer_only_feature(emu, monkeypatch):
    """With the knob on, a marked guidance pair and a conditioning tensor: engine._PAIR is never set during the walk, nothing is
    prepared (ContextKV.chain_runs / _pins untouched), and the bytes are those of the knob-off evaluation."""
    qnn, args = _model("sd_tiny")
    x, t, c = args
    x, t, c = torch.cat([x, x]), torch.cat([t, t]), torch.cat([c, c])
    ckv = qnn.__dict__["_ctx_kv"]
    seen = []
    h = qnn.model.register_forward_pre_hook(lambda m, a: seen.append((emu._PAIR[0], emu._PAIR_N[0])))
    qnn._own_hooks = qnn._hook_census()
    try:
        with torch.no_grad():
            emu.set_weight_only_graph(False)
            y0 = qnn(x, t, c)
            emu.set_weight_only_graph(True)
            emu.mark_pair(x, t)
            assert qnn._wonly_token() >= 0
            y1 = qnn(x, t, c)
            y2 = qnn(x, t, c)
    finally:
        h.remove()
    assert seen == [(0, 0)] * 3 and qnn.pair_evals == 0
    assert ckv.chain_runs == 0 and not ckv._pins
    assert torch.equal(y0, y1) and torch.equal(y1, y2)
    assert not qnn._graphs and qnn.__dict__.get("_graph_pool") is None          # (CPU tensors: nothing is captured)


def test_pool_handle_goes_when_the_graph_set_becomes_empty(emu):
    qnn, args = _model("cifar_tiny")
    d = qnn.__dict__
    qnn._graphs = {}
    for drop in (qnn._drop_graphs, qnn.invalidate_plans, lambda: qnn.enable_hip_graphs(True), lambda: qnn.enable_hip_graphs(False)):
        if qnn._graphs is None:
            qnn._graphs = {}
        qnn._graphs["k"], d["_graph_pool"] = object(), (1, 2)
        drop()
        assert not qnn._graphs and d["_graph_pool"] is None
