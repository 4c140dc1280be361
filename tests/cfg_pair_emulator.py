"""tests/abi_emulator.py plus the two periods of a classifier-free-guidance pair (include/qdiff_hip.h): the residual row period of
qd_conv2d_i8 (qd_conv_desc.res_period: output row m adds residual row m % P) and the query head period of qd_attn_i8_qp (head bh
reads the q rows of head bh % q_heads).  Both are emulated by materialising the duplicate the kernels never build and handing it
to the unchanged emulation, so "equal to the same launch fed a duplicate" holds by construction here and is what the GPU tests
check of the kernels.  install() returns the list every conv2d_i8 / attn_i8 launch is recorded in.  The product never uses it."""
import torch

import abi_emulator


def conv2d_i8(c, acc_out=None):
    P = int(getattr(c, "res_period", 0) or 0)
    if not P:
        return abi_emulator.conv2d_i8(c, acc_out)
    M = c.B * c.Ho * c.Wo
    assert c.residual is not None and acc_out is None, "res_period needs a residual and the linear epilogue"
    assert (getattr(c, "epilogue", 0) or 0) == 0, "res_period: linear epilogue only"
    assert P > 0 and M % P == 0 and P % (c.Ho * c.Wo) == 0 and c.residual.shape[0] == P
    res = c.residual
    c.residual, c.res_period = res.repeat(M // P, 1), 0
    try:
        return abi_emulator.conv2d_i8(c, acc_out)
    finally:
        c.residual, c.res_period = res, P


def attn_i8(q, k, vt, vsum, BH, H, T, S, d, Tpad, Spad, dpad, prm, wbits, wmin, wmax, q_asym, out, ldo,
            out8=None, oq_params=None, oq_grid=None, kterm=None, q_heads=None):
    if q_heads is not None and q_heads != BH:
        assert q_heads > 0 and BH % q_heads == 0 and q_heads % H == 0 and q.shape[0] == q_heads
        q = q.repeat(BH // q_heads, 1, 1)
    return abi_emulator.attn_i8(q, k, vt, vsum, BH, H, T, S, d, Tpad, Spad, dpad, prm, wbits, wmin, wmax, q_asym, out, ldo,
                                out8=out8, oq_params=oq_params, oq_grid=oq_grid, kterm=kterm)


def install(monkeypatch):
    """abi_emulator.install with the two entries above; returns `calls`: one tuple per launch,
    ("conv", rows M, Cout, res_period) or ("attn", BH, q heads, T, S)."""
    from qdiff import engine, hip
    abi_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "pair_entries_ok", lambda x: True)     # this emulation implements the two periods, on host tensors
    calls = []

    def conv(c, acc_out=None):
        calls.append(("conv", c.B * c.Ho * c.Wo, c.Cout, int(getattr(c, "res_period", 0) or 0)))
        return conv2d_i8(c, acc_out)

    def attn(q, k, vt, vsum, BH, *a, **kw):
        calls.append(("attn", BH, kw.get("q_heads") or BH, a[1], a[2]))
        return attn_i8(q, k, vt, vsum, BH, *a, **kw)

    monkeypatch.setattr(hip, "conv2d_i8", conv)
    monkeypatch.setattr(hip, "attn_i8", attn)
    return calls
