"""CPU test (no GPU) of the fused resampling residual blocks of the integer path (engine.FUSE_UPDOWN): with the knob off the new
entry is never reached (tests/abi_emulator.py has none), and the gate of the route refuses what the kernel does not cover."""
import os

import torch

import abi_emulator
from golden_util import fixture_inputs, load_fixture
from test_host_logic import _resume_cpu


def test_knob_off_changes_nothing_and_the_gate_refuses(monkeypatch):
    from qdiff import engine, hip
    from qdiff.quant_block import QuantResBlock, _parts_of, _res_updown_fused
    assert engine.FUSE_UPDOWN is False or os.environ.get("QDIFF_FUSE_UPDOWN")           # off by default
    abi_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "FUSE_UPDOWN", False)
    monkeypatch.setattr(hip, "groupnorm_resample_silu_quant", None)                      # reaching it raises
    fx = load_fixture("model_ldm_updown_tiny.pt")
    qnn = _resume_cpu(fx)
    x, t, _ = fixture_inputs(fx, "test")
    with torch.no_grad():
        y = qnn(x, t)
    ref = fx["out_wa"]                                # the bound of test_host_logic.test_tiny_unets_on_emulator
    cos = torch.nn.functional.cosine_similarity(y.flatten(), ref.flatten(), dim=0).item()
    assert (y - ref).abs().max().item() <= 0.1 * ref.abs().max().item() and cos >= 0.998
    monkeypatch.setattr(engine, "_EFFECTIVE", [None])
    blk = next(m for m in qnn.modules() if isinstance(m, QuantResBlock) and m.updown and hasattr(m.h_upd, "op"))
    p = _parts_of(blk, blk.in_layers[-1], blk.out_layers[-1], 1)
    x = torch.randn(2, blk.channels, 8, 8)
    assert not _res_updown_fused(p, x)                                           # the knob is off
    monkeypatch.setattr(engine, "FUSE_UPDOWN", True)
    assert _res_updown_fused(p, x)
    assert not _res_updown_fused(p, torch.randn(2, blk.channels, 7, 7))          # an odd map
    with monkeypatch.context() as m:                                             # an uninitialised quantiser
        m.setattr(p.conv1.act_quantizer, "inited", False)
        assert not _res_updown_fused(p, x)
    with monkeypatch.context() as m:                                             # QDIFF_STREAM=fp16
        m.setattr(engine, "STREAM_DTYPE", torch.float16)
        assert not _res_updown_fused(p, x)
    h = blk.x_upd.register_forward_hook(lambda *a: None)                         # a hooked block
    assert not _res_updown_fused(p, x)
    h.remove()
