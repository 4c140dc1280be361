"""CPU emulation of qd_temb_mlp_wq_h16 at the level of qdiff.hip's Python wrapper, for host-logic tests: include/qdiff_hip.h
followed literally in fp64 — SiLU x / (1 + exp(-x)), ONE rounding to the operand type, the tile-ordered t4 / t8 codes of
tests/wonly_emulator.py minus the raw zero point, times delta, plus bias; columns outside the slices are left alone.  Builds on
tests/wonly_fused_emulator.install; the entry point appends its name to the same `calls` list and ticks engine.WONLY_TEMB as
the wrapper does.  The product never uses it."""
from types import SimpleNamespace as NS

import torch

import wonly_emulator
import wonly_fused_emulator


def temb_mlp_wq_h16(x, silu, plans, offsets, out, act_dtype):
    from qdiff import engine
    assert x.dim() == 2 and x.dtype == torch.float32 and out.dtype == torch.float32 and out.stride(1) == 1
    assert act_dtype in (torch.float16, torch.bfloat16)
    B, K = x.shape
    assert K % 16 == 0
    v = x.double()
    if silu:
        v = v / (1 + torch.exp(-v))
    v = v.to(act_dtype).double()
    for p, off in zip(plans, offsets):
        assert len(p.segs) == 1 and p.Cin == K and p.act_dtype == act_dtype and p.pack.wbits == plans[0].pack.wbits
        sg = p.segs[0]
        c = NS(kh=1, kw=1, Cout=p.Cout, wbits=p.pack.wbits, w=p.pack.wq)
        q = wonly_emulator._codes(c, dict(clen=K, kstep0=sg["kstep0"])).double()[:, 0]          # [Cout][K]
        y = (v @ (q - sg["zw"].double().view(-1, 1)).t()) * sg["scale"].double()
        if p.bias is not None:
            y = y + p.bias.double()
        out[:, off:off + p.Cout] = y.float()
    engine.WONLY_TEMB[0] += 1


def install(monkeypatch):
    """wonly_fused_emulator.install plus qd_temb_mlp_wq_h16; returns the call list."""
    from qdiff import hip
    calls = wonly_fused_emulator.install(monkeypatch)

    def run(*a, **k):
        calls.append("temb_mlp_wq_h16")
        return temb_mlp_wq_h16(*a, **k)

    monkeypatch.setattr(hip, "temb_mlp_wq_h16", run)
    return calls
