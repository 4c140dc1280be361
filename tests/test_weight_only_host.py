"""CPU tests (no GPU) of the weights-only path's host logic (engine.WEIGHT_ONLY_KERNEL): knob and environment parsing,
which QuantModules take the kernel, every fallback to the library path, int_ready() staying False in state (True, False),
and the error of a model whose fp32 weights were freed.  The two entry points run on tests/wonly_emulator.py."""
import os
import subprocess
import sys

import pytest
import torch

import wonly_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WQ = dict(n_bits=4, channel_wise=True, scale_method="max")
AQ = dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True)


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    wonly_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", None)
    return engine


def _module(layer, wq=WQ, seed=0):
    import qdiff
    torch.manual_seed(seed)
    m = qdiff.QuantModule(layer, dict(wq), dict(AQ))
    m.set_quant_state(True, False)
    return m


def _input(m, seed=1):
    g = torch.Generator().manual_seed(seed)
    if m.kind == "conv2d":
        return torch.randn(2, m.weight.shape[1] * m.fwd_kwargs["groups"], 9, 7, generator=g)
    if m.kind == "conv1d":
        return torch.randn(2, m.weight.shape[1], 13, generator=g)
    return torch.randn(3, 5, m.weight.shape[1], generator=g)


def _library(m, x):
    from qdiff import engine
    prev = engine.WEIGHT_ONLY_KERNEL
    engine.WEIGHT_ONLY_KERNEL = None
    try:
        with torch.no_grad():
            return m(x)
    finally:
        engine.WEIGHT_ONLY_KERNEL = prev


def test_knob_parsing_and_setter():
    from qdiff import engine
    p = engine._parse_weight_only
    assert p(None) is None and p("") is None and p("off") is None and p("0") is None
    assert p("fp16") is torch.float16 and p("HALF") is torch.float16 and p("float16") is torch.float16
    assert p("bf16") is torch.bfloat16 and p("bfloat16") is torch.bfloat16
    with pytest.raises(ValueError):
        p("int8")
    prev = engine.WEIGHT_ONLY_KERNEL
    try:
        engine.set_weight_only_kernel("bf16")
        assert engine.WEIGHT_ONLY_KERNEL is torch.bfloat16
        engine.set_weight_only_kernel(torch.float16)
        assert engine.WEIGHT_ONLY_KERNEL is torch.float16
        engine.set_weight_only_kernel(None)
        assert engine.WEIGHT_ONLY_KERNEL is None
        with pytest.raises(ValueError):
            engine.set_weight_only_kernel(torch.float32)
    finally:
        engine.set_weight_only_kernel(prev)
    assert prev is None                                    # off by default


@pytest.mark.parametrize("env,want", [("fp16", "torch.float16"), ("bf16", "torch.bfloat16"), ("off", "None")])
def test_environment_variable_sets_the_knob(env, want):
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_KERNEL)"
    e = dict(os.environ, QDIFF_WEIGHT_ONLY=env, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "q-diffusion_amd"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == want


@pytest.mark.parametrize("layer", [lambda: torch.nn.Conv2d(40, 24, 3, padding=1), lambda: torch.nn.Conv2d(40, 24, 3, stride=2, padding=1),
                                   lambda: torch.nn.Conv2d(40, 36, 1), lambda: torch.nn.Linear(40, 33), lambda: torch.nn.Conv1d(40, 20, 1)],
                         ids=["conv3x3", "conv3x3s2", "conv1x1", "linear", "conv1d"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_weight_only_modules_take_the_kernel(emu, layer, dt):
    m = _module(layer())
    x = _input(m)
    y_lib = _library(m, x)
    emu.WEIGHT_ONLY_KERNEL = dt
    with torch.no_grad():
        assert m.wonly_ready() and not m.int_ready()
        y = m(x)
    assert y.shape == y_lib.shape and y.dtype == torch.float32
    assert m.__dict__["_wonly_cache"][1] is not None
    # the kernel's operands are the library's weight and x rounded to dt: close, and exactly the emulated contraction
    rel = (y - y_lib).abs().max() / y_lib.abs().max()
    assert rel < (2e-3 if dt == torch.float16 else 2e-2)


def test_which_states_take_the_kernel(emu):
    from qdiff import engine
    m = _module(torch.nn.Conv2d(32, 16, 3, padding=1))
    x = _input(m)
    _library(m, x)                                          # initialises the weight quantiser
    with torch.no_grad():
        assert not m.wonly_ready()                          # knob off
        emu.WEIGHT_ONLY_KERNEL = torch.float16
        assert m.wonly_ready()
        m.set_quant_state(False, False)
        assert not m.wonly_ready()                          # weights not quantised
        m.set_quant_state(True, True)
        assert not m.wonly_ready()                          # activations quantised: the integer path's state
        m.disable_act_quant = True
        assert m.wonly_ready()                              # ... unless they are disabled
        m.disable_act_quant = False
        m.set_quant_state(True, False)
        with engine.simulation():
            assert not m.wonly_ready()                      # the fake-quant denominator stays the library path
    assert not m.wonly_ready()                              # autograd on
    with torch.no_grad():
        assert not m.int_ready()                            # (True, False): the blocks' fused integer routes stay off


def test_activation_quantisers_are_not_touched(emu):
    m = _module(torch.nn.Conv2d(32, 16, 1))
    emu.WEIGHT_ONLY_KERNEL = torch.float16
    with torch.no_grad():
        m(_input(m))
    assert not m.act_quantizer.inited and m._plan is None


@pytest.mark.parametrize("case", ["symmetric", "per_tensor", "grouped", "dilated", "no_gpu_tensor"])
def test_fallbacks_keep_the_library_path(emu, monkeypatch, case):
    wq = dict(WQ)
    layer = torch.nn.Conv2d(32, 16, 3, padding=1)
    if case == "symmetric":
        wq["symmetric"] = True
    elif case == "per_tensor":
        wq["channel_wise"] = False
    elif case == "grouped":
        layer = torch.nn.Conv2d(32, 16, 3, padding=1, groups=2)
    elif case == "dilated":
        layer = torch.nn.Conv2d(32, 16, 3, padding=2, dilation=2)
    m = _module(layer, wq)
    x = _input(m)
    y_lib = _library(m, x)
    if case == "no_gpu_tensor":
        monkeypatch.setattr(emu, "wonly_device_ok", lambda t: t.is_cuda)
    emu.WEIGHT_ONLY_KERNEL = torch.float16
    with torch.no_grad():
        if case != "no_gpu_tensor":
            assert m.wonly_plan() is None and not m.wonly_ready()
        y = m(x)
    assert torch.equal(y, y_lib)


def test_bf16_code_span_past_256_keeps_the_library_path(emu):
    """8-bit codes: |q - z| = 256 is exact in bf16 and takes the kernel; 257 falls back (fp16 takes both)."""
    for z0, ok in ((-1, True), (-2, False)):
        m = _module(torch.nn.Conv2d(32, 16, 1), dict(WQ, n_bits=8))
        x = _input(m)
        _library(m, x)
        wq = m.weight_quantizer
        d = float(wq.delta.view(-1)[0])
        wq.zero_point = wq.zero_point.clone()
        wq.zero_point.view(-1)[0] = float(z0)
        m.weight.data[0, 0] = (255 - z0) * d
        m.invalidate()
        y_lib = _library(m, x)
        emu.WEIGHT_ONLY_KERNEL = torch.bfloat16
        with torch.no_grad():
            assert (m.wonly_plan() is not None) == ok
            y = m(x)
            if not ok:
                assert torch.equal(y, y_lib)
            emu.WEIGHT_ONLY_KERNEL = torch.float16
            assert m.wonly_ready()
        emu.WEIGHT_ONLY_KERNEL = None


def test_split_layer_and_autocast_dtype(emu, monkeypatch):
    m = _module(torch.nn.Conv2d(48, 24, 1))
    x = _input(m)
    with torch.no_grad():
        y_lib = m(x, split=16)                              # the split shortcut: two weight quantisers
    emu.WEIGHT_ONLY_KERNEL = torch.float16
    with torch.no_grad():
        plan = m.wonly_plan()
        assert plan is not None and len(plan.segs) == 2
        y = m(x, split=16)
    assert (y - y_lib).abs().max() / y_lib.abs().max() < 2e-3
    monkeypatch.setattr(emu, "wonly_out_dtype", lambda dev="cuda": (torch.float16, None))
    with torch.no_grad():
        assert m(x, split=16).dtype == torch.float16


def test_plan_cache_follows_the_weight_quantiser(emu):
    m = _module(torch.nn.Conv2d(32, 16, 1))
    x = _input(m)
    emu.WEIGHT_ONLY_KERNEL = torch.float16
    with torch.no_grad():
        p1 = m.wonly_plan()
        assert m.wonly_plan() is p1
        m.weight_quantizer.delta = m.weight_quantizer.delta * 2   # re-assigned quantiser state: a new plan
        p2 = m.wonly_plan()
        assert p2 is not p1
        m.invalidate()
        assert m.wonly_plan() is not p2


def test_freed_weights_need_the_knob(emu):
    """A layer whose fp32 weight was released (load_packed_ckpt(free_weights=True)) runs weights-only from its frozen pack with
    the knob on; with it off the error names the knob instead of failing inside the library convolution."""
    import qdiff
    m = _module(torch.nn.Conv2d(32, 16, 3, padding=1))
    x = _input(m)
    emu.WEIGHT_ONLY_KERNEL = torch.float16
    with torch.no_grad():
        y_live = m(x)
        pack = m._pack                                      # the pack the weights-only plan was built from
        assert pack is not None
        m.load_packed(pack)
        m.weight.data = torch.empty(0)
        m.org_weight = torch.empty(0)
        assert torch.equal(m(x), y_live)
    emu.WEIGHT_ONLY_KERNEL = None
    with torch.no_grad(), pytest.raises(qdiff.hip.HipEngineError, match="QDIFF_WEIGHT_ONLY"):
        m(x)
