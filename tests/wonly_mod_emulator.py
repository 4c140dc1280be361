"""CPU emulation of qd_groupnorm_mod_h16 and qd_groupnorm_resample_h16 at the level of qdiff.hip's Python wrappers, for
host-logic tests: include/qdiff_hip.h followed literally in fp64, one rounding to the operand type at the store, pad channels
zero.  Builds on tests/wonly_fused_emulator.py; every entry point appends its name to `calls`.  The product never uses it."""
import torch
import torch.nn.functional as F

import wonly_fused_emulator
from wonly_fused_emulator import _store


def _gn(x, B, S, C, ldx, groups, eps, gamma, beta):
    """fp64 GroupNorm of the rows -> [B, C, S]."""
    v = torch.as_strided(x, (B, S, C), (S * ldx, ldx, 1)).double().permute(0, 2, 1)
    return F.group_norm(v, groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)


def groupnorm_mod_h16(x, B, S, C, ldx, groups, eps, gamma, beta, mod, mod_ld, silu, out, ldo, ws):
    assert mod.dtype == torch.float32 and mod_ld >= 2 * C
    m = torch.as_strided(mod, (B, 2 * C), (mod_ld, 1)).double()
    y = _gn(x, B, S, C, ldx, groups, eps, gamma, beta) * (1 + m[:, :C, None]) + m[:, C:, None]
    if silu:
        y = F.silu(y)
    _store(out, ldo, y.permute(0, 2, 1).reshape(B * S, C))


def groupnorm_resample_h16(x, B, H, W, C, ldx, groups, eps, gamma, beta, silu, resample, out, ldo, ws):
    assert resample in (1, 2) and (resample == 2 or (H % 2 == 0 and W % 2 == 0))
    y = _gn(x, B, H * W, C, ldx, groups, eps, gamma, beta)
    if silu:
        y = F.silu(y)
    y = y.view(B, C, H, W)
    if resample == 1:                    # the header, literally: ((y00 + y01) + (y10 + y11)) * 0.25 of the post-SiLU values
        y = ((y[:, :, 0::2, 0::2] + y[:, :, 0::2, 1::2]) + (y[:, :, 1::2, 0::2] + y[:, :, 1::2, 1::2])) * 0.25
        _store(out, ldo, y.permute(0, 2, 3, 1).reshape(-1, C))
    else:                                # every input pixel's ROUNDED result to its four output rows
        r = y.permute(0, 2, 3, 1).to(out.dtype)
        r = r.view(B, H, 1, W, 1, C).expand(B, H, 2, W, 2, C).reshape(-1, C)
        rows = out.view(-1, ldo)
        rows[:, :C] = r
        rows[:, C:] = 0


def install(monkeypatch):
    """wonly_fused_emulator.install plus the two producers; returns the list every emulated entry point appends its name to."""
    from qdiff import hip
    calls = wonly_fused_emulator.install(monkeypatch)

    def counted(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run

    for name, fn in (("groupnorm_mod_h16", groupnorm_mod_h16), ("groupnorm_resample_h16", groupnorm_resample_h16)):
        monkeypatch.setattr(hip, name, counted(name, fn))
    return calls
