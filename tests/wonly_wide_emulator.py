"""CPU emulation of the GEGLU epilogue of qd_conv2d_wq_h16 (QD_EPI_GEGLU_H16) at the level of qdiff.hip's Python wrappers, for
host-logic tests: the fp64 contraction of tests/wonly_emulator.py over the (value tile, gate tile) interleaved pack, then
value * gelu(gate) per feature in fp64, ONE rounding to the operand type, channels [F, ldo) zero.  Everything else is deferred to
tests/wonly_fused_emulator.py.  The contraction keeps its name in `calls`; an epilogue launch also appends "geglu_epi".  The
product never uses it."""
import torch
import torch.nn.functional as F

import wonly_emulator
import wonly_fused_emulator


def deinterleave(h):
    """[M][2F] columns in 32-wide tiles value, gate, value, ... -> (value [M][F], gate [M][F])."""
    M, C2 = h.shape
    t = h.view(M, C2 // 64, 2, 32)
    return t[:, :, 0].reshape(M, C2 // 2), t[:, :, 1].reshape(M, C2 // 2)


def conv2d_wq_h16(c, act_dtype):
    from qdiff import hip
    if c.epilogue != hip.EPI_GEGLU_H16:
        return wonly_fused_emulator.conv2d_wq_h16(c, act_dtype)
    Fdim = c.Cout // 2
    assert c.Cout % 64 == 0 and len(c.segs) == 1 and c.residual is None and c.rowbias is None and c.gn_part is None and not c.upsample2x
    assert c.out.dtype == act_dtype and c.ldo >= Fdim and c.ldo % 8 == 0 and (c.kh, c.kw, c.stride) == (1, 1, 1)
    out, ep = c.out, c.epilogue
    acc = torch.empty((c.B * c.Ho * c.Wo, c.Cout), dtype=torch.float64)
    c.out, c.epilogue = acc, None
    try:
        wonly_emulator.conv2d_wq_h16(c, act_dtype)
    finally:
        c.out, c.epilogue = out, ep
    v, g = deinterleave(acc)
    rows = out.view(-1, c.ldo)
    rows[:, :Fdim] = (v * F.gelu(g)).to(out.dtype)
    rows[:, Fdim:] = 0


def install(monkeypatch):
    """wonly_fused_emulator.install plus the epilogue; returns the list every emulated entry point appends its name to."""
    from qdiff import hip
    calls = wonly_fused_emulator.install(monkeypatch)

    def run(c, act_dtype):
        calls.append("conv2d_wq_h16")
        if c.epilogue == hip.EPI_GEGLU_H16:
            calls.append("geglu_epi")
        return conv2d_wq_h16(c, act_dtype)

    monkeypatch.setattr(hip, "conv2d_wq_h16", run)
    return calls
