"""CPU emulation of the weights-only entry points (qd_rows_to_h16, qd_conv2d_wq_h16) at the level of qdiff.hip's Python
wrappers, for host-logic tests: it follows include/qdiff_hip.h literally — tile-ordered t4 / t8 codes, raw zero points in
seg.zw, delta_w in seg.scale — with fp64 arithmetic on the rounded activations.  The product never uses it."""
import torch
import torch.nn.functional as F


def rows_to_h16(x, B, C, S, strides, out, ldo, c0, clen, clen_pad, oc0):
    v = torch.as_strided(x, (B, C, S), strides)[:, c0:c0 + clen]
    rows = out.view(-1, ldo)
    rows[:, oc0:oc0 + clen] = v.permute(0, 2, 1).reshape(B * S, clen).to(out.dtype)
    rows[:, oc0 + clen:oc0 + clen_pad] = 0


def _codes(c, seg):
    """raw codes q [Cout, taps, clen] of one segment of the tile-ordered operand."""
    taps = c.kh * c.kw
    ntiles, nst = (c.Cout + 31) // 32, (seg["clen"] + 63) // 64
    k0 = seg.get("kstep0", 0)
    if c.wbits == 8:
        blk = c.w.view(torch.int8).view(-1, ntiles, 4, 32, 16)[k0:k0 + taps * nst].to(torch.int64) + 128
    else:
        by = c.w.view(-1, ntiles, 4, 32, 8)[k0:k0 + taps * nst].to(torch.int64)
        blk = torch.empty(by.shape[:-1] + (16,), dtype=torch.int64)
        for b in range(4):
            blk[..., b], blk[..., 4 + b] = by[..., b] & 15, by[..., b] >> 4
            blk[..., 8 + b], blk[..., 12 + b] = by[..., 4 + b] & 15, by[..., 4 + b] >> 4
    vals = blk.view(taps, nst, ntiles, 4, 32, 16)
    return vals.permute(2, 4, 0, 1, 3, 5).reshape(ntiles * 32, taps, nst * 64)[:c.Cout, :, :seg["clen"]]


def conv2d_wq_h16(c, act_dtype):
    assert c.x.dtype == act_dtype
    B, H, W = c.B, c.H, c.W
    x = c.x.view(B, H, W, c.ldx).double().permute(0, 3, 1, 2)
    total = 0
    for seg in c.segs:
        assert seg.get("zc") is None and seg.get("zfill") is None and seg.get("fill16") is None
        q = _codes(c, seg).double()
        wv = (q - seg["zw"].double().view(-1, 1, 1)) * seg["scale"].double().view(-1, 1, 1)
        wv = wv.view(c.Cout, c.kh, c.kw, seg["clen"]).permute(0, 3, 1, 2)
        xs = x[:, seg["c0"]:seg["c0"] + seg["clen"]]
        xs = F.pad(xs, (c.pad_l, c.pad_l + c.kw, c.pad_t, c.pad_t + c.kh))
        y = F.conv2d(xs, wv, stride=c.stride)[:, :, :c.Ho, :c.Wo]
        total = total + y
    out = total.permute(0, 2, 3, 1).reshape(B * c.Ho * c.Wo, c.Cout)
    if c.bias is not None:
        out = out + c.bias.double()
    if c.residual is not None:
        out = out + c.residual.double()
    c.out.copy_(out.to(c.out.dtype))


def install(monkeypatch):
    """Replace the weights-only entry points of qdiff.hip (and the tile packers, from tests/abi_emulator.py) by the emulation
    and admit CPU tensors to the path."""
    import abi_emulator
    from qdiff import engine, hip
    monkeypatch.setattr(hip, "pack_weights_t4", abi_emulator.pack_weights_t4)
    monkeypatch.setattr(hip, "pack_weights_t8", abi_emulator.pack_weights_t8)
    monkeypatch.setattr(hip, "rows_to_h16", rows_to_h16)
    monkeypatch.setattr(hip, "conv2d_wq_h16", conv2d_wq_h16)
    monkeypatch.setattr(engine, "wonly_device_ok", lambda t: True)
