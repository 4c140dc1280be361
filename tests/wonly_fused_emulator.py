"""CPU emulation of the weights-only producers (qd_layernorm_h16, qd_geglu_h16, qd_groupnorm_h16) and of the row bias of
qd_conv2d_wq_h16, at the level of qdiff.hip's Python wrappers, for host-logic tests: include/qdiff_hip.h followed literally
in fp64, one rounding to the operand type at the store, pad channels zero.  Builds on tests/wonly_emulator.py; every entry
point appends its name to `calls` so that tests can count launches.  The product never uses it."""
import torch
import torch.nn.functional as F

import wonly_emulator


def _store(out, ldo, y):
    rows = out.view(-1, ldo)
    rows[:, :y.shape[1]] = y.to(out.dtype)
    rows[:, y.shape[1]:] = 0


def layernorm_h16(x, M, C, ldx, eps, gamma, beta, out, ldo):
    v = torch.as_strided(x, (M, C), (ldx, 1)).double()
    _store(out, ldo, F.layer_norm(v, (C,), gamma.double(), beta.double(), eps))


def geglu_h16(h, M, Fdim, ldh, out, ldo):
    v = torch.as_strided(h, (M, 2 * Fdim), (ldh, 1)).double()
    _store(out, ldo, v[:, :Fdim] * F.gelu(v[:, Fdim:]))


def groupnorm_h16(x, B, S, C, ldx, groups, eps, gamma, beta, silu, out, ldo, ws):
    v = torch.as_strided(x, (B, S, C), (S * ldx, ldx, 1)).double().permute(0, 2, 1)
    y = F.group_norm(v, groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)
    if silu:
        y = F.silu(y)
    _store(out, ldo, y.permute(0, 2, 1).reshape(B * S, C))


def conv2d_wq_h16(c, act_dtype):
    """tests/wonly_emulator.conv2d_wq_h16 plus the row bias: row b of rowbias added to every output row of sample b, after
    the bias and before the residual; gn_part / upsample2x refused as the library does."""
    from qdiff import hip
    if c.gn_part is not None or c.upsample2x:
        raise hip.HipEngineError("qd_conv2d_wq_h16: linear epilogue only (no GroupNorm statistics or up-sampling)")
    if c.rowbias is None:
        return wonly_emulator.conv2d_wq_h16(c, act_dtype)
    assert c.rowbias.dtype == torch.float32 and c.ld_rowbias >= c.Cout
    res, out = c.residual, c.out
    acc = torch.empty(out.shape, dtype=torch.float64)
    c.residual, c.out = None, acc
    try:
        wonly_emulator.conv2d_wq_h16(c, act_dtype)
    finally:
        c.residual, c.out = res, out
    rb = torch.as_strided(c.rowbias, (c.B, c.Cout), (c.ld_rowbias, 1)).double()
    acc = acc + rb.repeat_interleave(c.Ho * c.Wo, dim=0)
    if res is not None:
        acc = acc + res.double()
    out.copy_(acc.to(out.dtype))


def install(monkeypatch):
    """wonly_emulator.install plus the producers; returns the list every emulated entry point appends its name to."""
    from qdiff import hip
    wonly_emulator.install(monkeypatch)
    calls = []

    def counted(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run

    monkeypatch.setattr(hip, "groupnorm_ws_bytes", lambda B, C, S: 16)
    for name, fn in (("rows_to_h16", wonly_emulator.rows_to_h16), ("conv2d_wq_h16", conv2d_wq_h16), ("layernorm_h16", layernorm_h16),
                     ("geglu_h16", geglu_h16), ("groupnorm_h16", groupnorm_h16)):
        monkeypatch.setattr(hip, name, counted(name, fn))
    return calls
