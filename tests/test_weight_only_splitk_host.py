"""CPU tests (no GPU) of the weights-only split-K (engine.WEIGHT_ONLY_SPLITK).

1. The policy through the real library: qd_conv2d_wq_h16_splitk_ws_bytes is a pure host function of the descriptor's shape
   fields, and qd_wq_h16_config overrides it.
2. The host logic on the CPU emulators: the knob, which ConvCalls carry `splitk`, and that the emulated outputs do not move.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import wonly_emulator
import wonly_wide_emulator
from test_weight_only_fused_host import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- policy through the library --------------------------------------------------------------------------------------------
@pytest.fixture
def lib():
    from qdiff import hip
    handle = hip.load()
    handle.qd_wq_h16_config(-1)
    yield handle
    handle.qd_wq_h16_config(-1)


def _desc(B, H, W, Cout, k, clens, epilogue=0, stride=1):
    """Shape-only descriptor: every pointer NULL."""
    from qdiff import hip
    d = hip.ConvDesc()
    d.B, d.H, d.W, d.Cout = B, H, W, Cout
    d.Ho, d.Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    d.kh = d.kw = k
    d.stride, d.pad_t, d.pad_l = stride, k // 2, k // 2
    d.wbits, d.w_tiled, d.epilogue, d.nseg = 4, 1, epilogue, len(clens)
    c0 = 0
    for i, c in enumerate(clens):
        d.seg[i].c0, d.seg[i].clen = c0, c
        c0 += c
    return d


def _bytes(lib, d):
    return int(lib.qd_conv2d_wq_h16_splitk_ws_bytes(ctypes.byref(d)))


SD_8x8 = dict(B=16, H=8, W=8, Cout=1280, k=3, clens=[1280])                     # M = 1024: 80 tiles, 180 K-steps
SD_8x8_SHORTCUT = dict(B=16, H=8, W=8, Cout=1280, k=3, clens=[1280, 1280])      # 2560 -> 1280 split shortcut: 360 K-steps
FULL_GRID = dict(B=16, H=64, W=64, Cout=320, k=3, clens=[320])                  # M = 65536: 1536 tiles
GEGLU = dict(B=1, H=1, W=1024, Cout=10240, k=1, clens=[1280], epilogue=4)
ONE_STEP = dict(B=1, H=1, W=32, Cout=64, k=1, clens=[64])
TEMB = dict(B=1, H=1, W=16, Cout=1280, k=1, clens=[1280])                          # 10 tiles, 20 K-steps: too short to pay a second launch


def _nsplit(nbytes, dd):
    mn4 = dd["B"] * dd["H"] * dd["W"] * dd["Cout"] * 4
    assert nbytes % mn4 == 0
    return nbytes // mn4


def test_policy_splits_under_filled_layers_only(lib):
    for dd in (SD_8x8, SD_8x8_SHORTCUT):
        n = _nsplit(_bytes(lib, _desc(**dd)), dd)
        assert 2 <= n <= 32, (dd, n)
    for dd in (FULL_GRID, GEGLU, ONE_STEP, TEMB):
        assert _bytes(lib, _desc(**dd)) == 0, dd
    assert int(lib.qd_conv2d_wq_h16_splitk_ws_bytes(None)) == 0


def test_config_overrides_the_policy(lib):
    policy = {k: _bytes(lib, _desc(**dd)) for k, dd in (("a", SD_8x8), ("b", SD_8x8_SHORTCUT), ("c", FULL_GRID))}
    lib.qd_wq_h16_config(0)
    for dd in (SD_8x8, SD_8x8_SHORTCUT, FULL_GRID, GEGLU, ONE_STEP):
        assert _bytes(lib, _desc(**dd)) == 0
    lib.qd_wq_h16_config(3)
    for dd in (SD_8x8, SD_8x8_SHORTCUT, FULL_GRID):
        assert _bytes(lib, _desc(**dd)) == 3 * dd["B"] * dd["H"] * dd["W"] * dd["Cout"] * 4
    assert _bytes(lib, _desc(**GEGLU)) == 0                      # the GEGLU epilogue never splits
    assert _bytes(lib, _desc(**ONE_STEP)) == 0                   # clamped to the K-step count: one step, one slice
    lib.qd_wq_h16_config(-1)
    assert {k: _bytes(lib, _desc(**dd)) for k, dd in (("a", SD_8x8), ("b", SD_8x8_SHORTCUT), ("c", FULL_GRID))} == policy


def test_forced_count_never_leaves_an_empty_slice(lib):
    """27 K-steps (3 x 3 taps, 130 channels = 3 steps per tap): n slices of ceil(27 / n) steps need ceil(27 / ceil(27 / n))
    slices, and a count past the K-steps is clamped to them."""
    dd = dict(B=2, H=5, W=7, Cout=48, k=3, clens=[136])
    for n, want in ((2, 2), (4, 4), (5, 5), (10, 9), (27, 27), (40, 27)):
        lib.qd_wq_h16_config(n)
        assert _nsplit(_bytes(lib, _desc(**dd)), dd) == want, n


def test_abi_lists_carry_the_new_symbols(lib):
    from qdiff import hip
    header = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    for name in ("qd_conv2d_wq_h16_splitk_ws_bytes", "qd_wq_h16_config", "qd_conv2d_wq_h16_form"):
        assert name in hip.EXPORTS and name + "(" in header and hasattr(lib, name)
    assert lib.qd_abi_version() == 20
    assert "split-K, oq_* / hd_* are ignored" not in header


# ---- host logic on the emulator --------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(monkeypatch):
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_WIDE", False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_SPLITK", False)
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    monkeypatch.setattr(engine, "WONLY_GEGLU_EPI", [0])
    monkeypatch.setattr(engine, "WONLY_SPLITK", [0])
    return engine


def _record(monkeypatch):
    """Wrap the installed hip.conv2d_wq_h16: [(epilogue, splitk)] of every call."""
    from qdiff import hip
    seen, inner = [], hip.conv2d_wq_h16

    def run(c, act_dtype):
        seen.append((c.epilogue, c.splitk))
        return inner(c, act_dtype)

    monkeypatch.setattr(hip, "conv2d_wq_h16", run)
    return seen


def test_knob_parsing_setter_and_default(knobs):
    engine = knobs
    for s, want in (("", False), ("0", False), ("off", False), ("1", True), ("ON", True)):
        assert engine._parse_flag(s, "QDIFF_WEIGHT_ONLY_SPLITK") is want
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_SPLITK"):
        engine.set_weight_only_splitk("fp16")
    engine.set_weight_only_splitk(True)
    assert engine.WEIGHT_ONLY_SPLITK is True
    engine.set_weight_only_splitk("0")
    assert engine.WEIGHT_ONLY_SPLITK is False
    with pytest.raises(ValueError):
        engine.set_weight_only_splitk(1)


def test_environment_variable_sets_the_knob_and_default_is_off():
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_SPLITK)"
    for val, want in ((None, "False"), ("1", "True")):
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
        env.pop("QDIFF_WEIGHT_ONLY_SPLITK", None)
        if val is not None:
            env["QDIFF_WEIGHT_ONLY_SPLITK"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split()[-1] == want


def test_wonly_forward_marks_its_call_only_with_the_knob_on(knobs, monkeypatch):
    import qdiff
    engine = knobs
    wonly_emulator.install(monkeypatch)
    seen = _record(monkeypatch)
    torch.manual_seed(0)
    m = qdiff.QuantModule(torch.nn.Conv2d(24, 40, 3, padding=1), dict(n_bits=4, channel_wise=True, scale_method="max"),
                          dict(n_bits=8, channel_wise=False, scale_method="max")).eval()
    m.set_quant_state(True, False)
    x = torch.randn(2, 24, 6, 5)
    with torch.no_grad():
        y0 = m(x)
        assert seen == [(None, None)] and engine.WONLY_SPLITK[0] == 0
        engine.set_weight_only_splitk(True)
        y1 = m(x)
    assert seen == [(None, None), (None, True)]
    assert engine.WONLY_SPLITK[0] == 0                           # the emulated entry point attaches no workspace
    assert torch.equal(y0, y1)


@pytest.mark.parametrize("fuse", [False, True], ids=["unfused", "fused-wide"])
def test_tiny_model_calls_and_outputs(knobs, monkeypatch, fuse):
    """sd_tiny, state (True, False): knob off = no call carries `splitk`; knob on = every linear-epilogue call does and no
    GEGLU-epilogue call (wonly_forward_geglu) does; the emulated outputs are the same tensors either way."""
    from qdiff import hip
    engine = knobs
    wonly_wide_emulator.install(monkeypatch)
    seen = _record(monkeypatch)
    engine.set_weight_only_fusion(fuse)
    engine.set_weight_only_fusion_wide(fuse)
    qnn, args = _model("sd_tiny")
    with torch.no_grad():
        y0 = qnn(*args)
    off = list(seen)
    assert off and all(s is None for _, s in off) and engine.WONLY_SPLITK[0] == 0
    del seen[:]
    engine.set_weight_only_splitk(True)
    with torch.no_grad():
        y1 = qnn(*args)
    assert [e for e, _ in seen] == [e for e, _ in off]
    geglu = [s for e, s in seen if e == hip.EPI_GEGLU_H16]
    linear = [s for e, s in seen if e != hip.EPI_GEGLU_H16]
    assert linear and all(s is True for s in linear)
    assert all(s is None for s in geglu) and bool(geglu) == fuse
    assert torch.equal(y0, y1)
