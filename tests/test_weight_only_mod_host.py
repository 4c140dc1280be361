"""CPU tests (no GPU) of the weights-only route of the scale-shift and resampling residual blocks (engine.WEIGHT_ONLY_FUSE_MOD):
the exports, the knob, which blocks take the route and what they launch, every refusal of the gate, and the argument checks of
the two new wrappers.  The entry points run on tests/wonly_mod_emulator.py (fp64)."""
import ctypes
import os
import subprocess
import sys
from collections import Counter

import pytest
import torch

import wonly_mod_emulator
from test_weight_only_fused_host import ROOT, _block_call, _blocks, _model

PRODUCERS = ("groupnorm_h16", "groupnorm_mod_h16", "groupnorm_resample_h16")


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    calls = wonly_mod_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_ATTN", None)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_WIDE", False)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_MOD", False)
    monkeypatch.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
    engine.calls = calls
    yield engine
    del engine.calls


def _run(engine, qnn, args, mod, fuse=True):
    engine.set_weight_only_fusion(fuse)
    engine.set_weight_only_fusion_mod(mod)
    engine.WONLY_FUSED.pop("resblock_mod", None)
    for k in engine.WONLY_FUSED:
        engine.WONLY_FUSED[k] = 0
    del engine.calls[:]
    with torch.no_grad():
        y = qnn(*args)
    return y, list(engine.calls), dict(engine.WONLY_FUSED)


# ---- exports and knob ------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_entry_points_and_abi_20():
    from qdiff import hip
    assert "qd_groupnorm_mod_h16" in hip.EXPORTS and "qd_groupnorm_resample_h16" in hip.EXPORTS
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert lib.qd_abi_version() == 20
    for sym in ("qd_groupnorm_mod_h16", "qd_groupnorm_resample_h16"):
        assert getattr(lib, sym) is not None
    hdr = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    assert "int qd_groupnorm_mod_h16(" in hdr and "int qd_groupnorm_resample_h16(" in hdr and "#define QD_ABI_VERSION 20" in hdr


def test_knob_parsing_setter_and_default(monkeypatch):
    from qdiff import engine
    assert engine.WEIGHT_ONLY_FUSE_MOD is False or os.environ.get("QDIFF_WEIGHT_ONLY_FUSE_MOD")        # off by default
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_MOD", False)
    engine.set_weight_only_fusion_mod(True)
    assert engine.WEIGHT_ONLY_FUSE_MOD is True
    engine.set_weight_only_fusion_mod(" off ")
    assert engine.WEIGHT_ONLY_FUSE_MOD is False
    engine.set_weight_only_fusion_mod("ON")
    assert engine.WEIGHT_ONLY_FUSE_MOD is True
    with pytest.raises(ValueError, match="QDIFF_WEIGHT_ONLY_FUSE_MOD"):
        engine.set_weight_only_fusion_mod("fp16")
    with pytest.raises(ValueError):
        engine.set_weight_only_fusion_mod(None)
    assert "resblock_mod" not in engine.WONLY_FUSED


def test_environment_variable_and_knob_needs_the_fusion_knob(monkeypatch):
    code = "from qdiff import engine; print(engine.WEIGHT_ONLY_FUSE_MOD, engine.WEIGHT_ONLY_FUSE, engine.wonly_mod_state())"
    env = dict(os.environ, QDIFF_WEIGHT_ONLY_FUSE_MOD="1", QDIFF_WEIGHT_ONLY="fp16", PYTHONPATH=os.path.join(ROOT, "q-diffusion_amd"))
    env.pop("QDIFF_WEIGHT_ONLY_FUSE", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-3:] == ["True", "False", "False"]          # on, but without effect while QDIFF_WEIGHT_ONLY_FUSE is off
    from qdiff import engine
    monkeypatch.setattr(engine, "WEIGHT_ONLY_KERNEL", torch.float16)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", True)
    monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE_MOD", True)
    with torch.no_grad():
        assert engine.wonly_mod_state()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not engine.wonly_mod_state()
        monkeypatch.setattr(engine, "WEIGHT_ONLY_FUSE", False)
        assert not engine.wonly_mod_state()


def test_knob_without_the_fusion_knob_changes_nothing(emu):
    qnn, args = _model("ldm_updown_tiny")
    y0, c0, f0 = _run(emu, qnn, args, False, fuse=False)
    y1, c1, f1 = _run(emu, qnn, args, True, fuse=False)
    assert c1 == c0 and f1 == f0 and "resblock_mod" not in f1 and torch.equal(y0, y1)
    assert not any(p in c1 for p in PRODUCERS)


# ---- models ----------------------------------------------------------------------------------------------------------------
def test_knob_off_is_todays_call_list(emu):
    """Today's list is recorded in this run with the knob never set (the fixture's default), then with it set to off."""
    qnn, args = _model("ldm_updown_tiny")
    emu.set_weight_only_fusion(True)
    del emu.calls[:]
    with torch.no_grad():
        y_today = qnn(*args)
    today = list(emu.calls)
    y0, c0, f0 = _run(emu, qnn, args, False)
    assert c0 == today and torch.equal(y0, y_today)
    assert "resblock_mod" not in f0 and "groupnorm_mod_h16" not in c0 and "groupnorm_resample_h16" not in c0


@pytest.mark.parametrize("name", ["ldm_updown_tiny", "churches_full"])
def test_every_resblock_takes_the_route(emu, monkeypatch, name):
    """Launches per evaluation, from the block structure: a block on the route replaces the qd_rows_to_h16 passes of conv1 and
    conv2 by two producers: the first is qd_groupnorm_resample_h16 for an `updown` block and qd_groupnorm_h16 otherwise, the
    second qd_groupnorm_mod_h16 for a scale-shift block and qd_groupnorm_h16 otherwise.  Contractions: unchanged.
    Agreement with the knob off (the rule of test_weight_only_fused_host.test_models_take_the_fused_route): both runs round the
    same operands at the same sites, one in fp64 (emulator), one in fp32 (library), so a rounding to fp16 can land on the
    neighbouring value: one ulp = 2^-10 of the range per producer call of the route, to first order."""
    qnn, args = _model(name)
    res, _ = _blocks(qnn)
    modb = [b for b in res if b.updown or b.use_scale_shift_norm]
    assert len(modb) == len(res) > 0
    assert any(b.updown for b in res) and any(b.use_scale_shift_norm for b in res)
    y0, c0, f0 = _run(emu, qnn, args, False)
    from qdiff.quant_block import QuantResBlock
    inside, route = {}, QuantResBlock._forward_wonly

    def spy(self, *a, **k):                                    # (not a hook: a hooked block falls back)
        n0 = len(emu.calls)
        y = route(self, *a, **k)
        inside[self] = Counter(emu.calls[n0:])
        return y
    monkeypatch.setattr(QuantResBlock, "_forward_wonly", spy)
    y1, c1, f1 = _run(emu, qnn, args, True)
    c0, c1 = Counter(c0), Counter(c1)
    assert "resblock_mod" not in f0 and f0["resblock"] == 0
    assert f1["resblock_mod"] == len(res) and f1["resblock"] == 0
    nup, nss = sum(bool(b.updown) for b in res), sum(bool(b.use_scale_shift_norm) for b in res)
    assert c1["groupnorm_resample_h16"] == nup and c1["groupnorm_mod_h16"] == nss
    assert c1["groupnorm_h16"] - c0["groupnorm_h16"] == 2 * len(res) - nup - nss
    assert c0["groupnorm_mod_h16"] == c0["groupnorm_resample_h16"] == 0
    assert c1["conv2d_wq_h16"] == c0["conv2d_wq_h16"]
    assert c1["rows_to_h16"] == c0["rows_to_h16"] - 2 * len(res)
    # no rows_to_h16 remains for conv1 / conv2 of a covered block: the only ones issued inside a block are those of its skip
    # connection (one per segment) and of its embedding projection
    for b in res:
        skip = 0 if isinstance(b.skip_connection, torch.nn.Identity) else len(b.skip_connection.wonly_plan().segs)
        assert inside[b]["rows_to_h16"] == skip + 1 and inside[b]["conv2d_wq_h16"] == 3 + (skip > 0)     # conv1, conv2, embedding, skip
    sites = 2 * len(res)
    rng = y0.abs().max().item()
    d = (y1 - y0).abs().max().item() / rng
    print(f"\n[{name}] route on vs off on the emulator: {d:.3e} of range, bound {sites} x 2^-10 = {sites * 2.0 ** -10:.3e}")
    assert y1.dtype == y0.dtype and y1.shape == y0.shape
    assert 0 < d <= sites * 2.0 ** -10


# ---- gate ------------------------------------------------------------------------------------------------------------------
def _pick(res, **want):
    return next(b for b in res if all(bool(getattr(b, k)) == v for k, v in want.items()))


def test_gate_refusals(emu):
    from qdiff import engine
    qnn, args = _model("ldm_updown_tiny")
    res, _ = _blocks(qnn)
    down = next(b for b in res if b.updown and hasattr(b.h_upd, "op"))
    a, k = _block_call(qnn, args, down)
    conv1, conv2 = down.in_layers[-1], down.out_layers[-1]
    engine.set_weight_only_fusion(True)
    engine.set_weight_only_fusion_mod(True)
    gate = lambda x=a[0]: down._wonly_route(x, a[1], conv1, conv2) == "resblock_mod"

    def run(x=a[0]):
        n0, c0 = engine.WONLY_FUSED.get("resblock_mod", 0), len(engine.calls)
        y = down(x, *a[1:], **k)
        new = Counter(engine.calls[c0:])
        return y, engine.WONLY_FUSED.get("resblock_mod", 0) - n0, sum(new[p] for p in PRODUCERS)

    with torch.no_grad():
        assert gate() and down._wonly_route(a[0], a[1], conv1, conv2) != "resblock"
        y_on, took, prod = run()
        assert (took, prod) == (1, 2)
        engine.set_weight_only_fusion_mod(False)
        y_off, took, prod = run()
        assert (took, prod) == (0, 0) and not gate()
        engine.set_weight_only_fusion_mod(True)
        assert y_on.shape == y_off.shape and y_on.dtype == y_off.dtype
        # autocast
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not gate()
        # a hooked sub-module
        fired = []
        h = conv1.register_forward_hook(lambda m, i, o: fired.append(1))
        try:
            assert not gate()
            y, took, prod = run()
        finally:
            h.remove()
        assert (took, prod) == (0, 0) and fired == [1] and torch.equal(y, y_off)
        # odd H on a `down` block
        xo = torch.randn(a[0].shape[0], a[0].shape[1], 5, 5)
        assert not gate(xo)
        assert run(xo)[1:] == (0, 0)
        # split convolutions
        for m in (conv1, conv2):
            m.split = 8
            try:
                assert not gate()
            finally:
                m.split = 0
        # simulation
        prev = engine.SIMULATE
        engine.SIMULATE = True
        try:
            assert not gate() and run()[1:] == (0, 0)
        finally:
            engine.SIMULATE = prev
        # an h_upd of another make (with a convolution) is refused
        down.h_upd.use_conv = True
        try:
            assert not gate()
        finally:
            down.h_upd.use_conv = False
        assert run()[1:] == (1, 2)
    assert not gate() and run()[1:] == (0, 0)                  # autograd on


def test_wonly_fusable_still_refuses_these_blocks(emu):
    qnn, args = _model("ldm_updown_tiny")
    res, _ = _blocks(qnn)
    emu.set_weight_only_fusion_mod(True)
    with torch.no_grad():
        for b in res:
            a, k = _block_call(qnn, args, b)
            assert b._wonly_route(a[0], a[1], b.in_layers[-1], b.out_layers[-1]) != "resblock"
            assert b._wonly_route(a[0], a[1], b.in_layers[-1], b.out_layers[-1]) == "resblock_mod"


def test_plain_blocks_are_not_asked(emu):
    """A model of plain blocks: the knob changes neither the call list nor a bit, and creates no counter."""
    qnn, args = _model("ldm_tiny")
    y0, c0, f0 = _run(emu, qnn, args, False)
    y1, c1, f1 = _run(emu, qnn, args, True)
    assert c1 == c0 and f1 == f0 and "resblock_mod" not in f1 and torch.equal(y0, y1)


@pytest.mark.parametrize("name, kind", [("ldm_tiny", "resblock"), ("ldm_updown_tiny", "resblock_mod")])
def test_route_is_evaluated_once_per_block_forward(emu, monkeypatch, name, kind):
    """Plain blocks (ldm_tiny) and updown / scale-shift blocks (ldm_updown_tiny), both knobs on: every QuantResBlock forward
    walks its modules for _wonly_fuse_gate once, whichever route it takes."""
    from qdiff import quant_block
    from qdiff.quant_block import QuantResBlock
    qnn, args = _model(name)
    res, _ = _blocks(qnn)
    forwards, gates = Counter(), Counter()
    inner, gate = QuantResBlock._forward, quant_block._wonly_fuse_gate

    def forward(self, *a, **k):                                # (not a hook: a hooked block falls back)
        forwards[self] += 1
        return inner(self, *a, **k)

    def counted(block, layers, tensors):
        if isinstance(block, QuantResBlock):
            gates[block] += 1
        return gate(block, layers, tensors)
    monkeypatch.setattr(QuantResBlock, "_forward", forward)
    monkeypatch.setattr(quant_block, "_wonly_fuse_gate", counted)
    _, _, f = _run(emu, qnn, args, True)
    assert f.get(kind, 0) == len(res) > 0 and sum(f.values()) == len(res)
    assert set(forwards) == set(res) and all(n == 1 for n in forwards.values())
    assert gates == forwards


# ---- argument checks before any launch ---------------------------------------------------------------------------------------
def test_host_wrappers_validate_before_any_launch(monkeypatch):
    from qdiff import hip
    monkeypatch.setattr(hip, "load", lambda: pytest.fail("the library was reached"))
    E = hip.HipEngineError
    x = torch.zeros(2 * 4 * 6, 64)
    out = torch.zeros(2 * 4 * 6 * 4, 64, dtype=torch.float16)
    g, ws = torch.ones(64), torch.zeros(64)
    mod = torch.zeros(2, 128)
    with pytest.raises(E, match="mod_ld"):
        hip.groupnorm_mod_h16(x, 2, 24, 64, 64, 32, 1e-5, g, g, mod, 120, True, out, 64, ws)
    with pytest.raises(E, match="mod_ld"):
        hip.groupnorm_mod_h16(x, 2, 24, 64, 64, 32, 1e-5, g, g, None, 128, True, out, 64, ws)
    with pytest.raises(E, match="mod_ld"):
        hip.groupnorm_mod_h16(x, 2, 24, 64, 64, 32, 1e-5, g, g, mod.double(), 128, True, out, 64, ws)
    with pytest.raises(E, match="ldo % 8"):
        hip.groupnorm_mod_h16(x, 2, 24, 64, 64, 32, 1e-5, g, g, mod, 128, True, out, 68, ws)
    with pytest.raises(E, match="groups=7"):
        hip.groupnorm_mod_h16(x, 2, 24, 64, 64, 7, 1e-5, g, g, mod, 128, True, out, 64, ws)
    with pytest.raises(E, match="even H, W"):
        hip.groupnorm_resample_h16(x, 2, 4, 5, 64, 64, 32, 1e-5, g, g, True, 1, out, 64, ws)            # odd W
    with pytest.raises(E, match="even H, W"):
        hip.groupnorm_resample_h16(x, 2, 3, 6, 64, 64, 32, 1e-5, g, g, True, 1, out, 64, ws)            # odd H
    for bad in (0, 3, -1):
        with pytest.raises(E, match="resample="):
            hip.groupnorm_resample_h16(x, 2, 4, 6, 64, 64, 32, 1e-5, g, g, True, bad, out, 64, ws)
    with pytest.raises(E, match="ldo % 8"):
        hip.groupnorm_resample_h16(x, 2, 4, 6, 64, 64, 32, 1e-5, g, g, True, 2, out, 68, ws)
    with pytest.raises(E, match="unsupported dtypes"):
        hip.groupnorm_resample_h16(x.bfloat16(), 2, 4, 6, 64, 64, 32, 1e-5, g, g, True, 2, out, 64, ws)
    with pytest.raises(E, match="input rows"):
        hip.groupnorm_resample_h16(x, 2, 4, 6, 62, 62, 2, 1e-5, g, g, True, 2, out, 64, ws)


def test_emulated_average_follows_the_header():
    """The emulator's 2x2 average against torch's avg_pool2d, and its nearest 2x against the replicated rows of groupnorm_h16."""
    import torch.nn.functional as F
    import wonly_fused_emulator
    g = torch.Generator().manual_seed(3)
    B, H, W, C = 2, 4, 6, 32
    x = torch.randn(B * H * W, C, generator=g)
    gam, bet = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    full = torch.empty(B * H * W, 40, dtype=torch.float16)
    wonly_fused_emulator.groupnorm_h16(x, B, H * W, C, C, 8, 1e-5, gam, bet, True, full, 40, None)
    up = torch.empty(B * 4 * H * W, 40, dtype=torch.float16)
    wonly_mod_emulator.groupnorm_resample_h16(x, B, H, W, C, C, 8, 1e-5, gam, bet, True, 2, up, 40, None)
    assert torch.equal(up, full.view(B, H, 1, W, 1, 40).expand(B, H, 2, W, 2, 40).reshape(-1, 40))
    down = torch.empty(B * H * W // 4, 40, dtype=torch.float16)
    wonly_mod_emulator.groupnorm_resample_h16(x, B, H, W, C, C, 8, 1e-5, gam, bet, True, 1, down, 40, None)
    y = F.silu(F.group_norm(x.view(B, H * W, C).permute(0, 2, 1).double(), 8, gam.double(), bet.double(), 1e-5)).view(B, C, H, W)
    want = F.avg_pool2d(y, 2).permute(0, 2, 3, 1).reshape(-1, C)
    assert (down[:, :C].double() - want).abs().max() <= 2.0 ** -11 * want.abs().max() and (down[:, C:] == 0).all()
    m = torch.zeros(B, 2 * C)
    modz = torch.empty_like(full)
    wonly_mod_emulator.groupnorm_mod_h16(x, B, H * W, C, C, 8, 1e-5, gam, bet, m, 2 * C, True, modz, 40, None)
    assert torch.equal(modz, full)
