"""qd_conv2d_bf16 (the bf16 / fp16 mode of csrc/igemm_dma.hip: every convolution of the first-stage decoder) against an exact
reference, element by element: the cases of tests/first_stage_conv_cases.py.  Operands are small integers times powers of two
and every sum stays below 2^24 units, so the fp64 convolution rounded to fp32 is the one possible answer whatever the order of
the kernel's adds: fp32 rows must equal it, 16-bit rows must equal its single round to nearest even, first-level GroupNorm
statistics must equal the reference's sums, all bit for bit, and every byte outside [0, M) x [0, Cout) of the output must be
left alone.  Subnormal 16-bit operands: the launch must equal, as a whole, either the reference that uses them or the one that
reads them as zero; which one the hardware gives is recorded (profiles/first_stage_conv_exact.txt).  No tolerance appears in
this file.

Cases hip.conv2d_bf16 can express go through it (ldx / ldo / ldr from the views' strides); c0 > 0, other strides and paddings
and the launch just under 4 GiB use a hand-built descriptor."""
import ctypes

import pytest
import torch

import first_stage_conv_cases as C

pytestmark = pytest.mark.gpu


def _descriptor(hip, c, x_ptr, wt, bias, out, res, part, H=None):
    d = hip.ConvDesc()
    d.x, d.w, d.out = x_ptr, wt.data_ptr(), out.data_ptr()
    d.bias = None if bias is None else bias.data_ptr()
    d.residual = None if res is None else res.data_ptr()
    d.ldx, d.ldo, d.ldr = c.ldx, c.ldo, c.ldr if res is not None else 0
    H = c.H if H is None else H
    d.B, d.H, d.W = c.B, H, c.W
    d.Ho, d.Wo = (H + 2 * c.pad - c.k) // c.stride + 1, c.Wo
    d.Cout = c.Cout
    d.kh = d.kw = c.k
    d.stride, d.pad_t, d.pad_l = c.stride, c.pad, c.pad
    d.wbits, d.w_tiled, d.epilogue = (17 if c.dtype == torch.float16 else 16), 1, hip.EPI_LINEAR
    d.out_dtype = hip.BF16 if c.odt == torch.bfloat16 else hip.F16 if c.odt == torch.float16 else hip.F32
    if part is not None:
        d.gn_part, d.gn_ld = part.data_ptr(), hip.part_ld(part)
    d.upsample2x = 1 if c.ups else 0
    d.nseg = 1
    d.seg[0].c0, d.seg[0].clen = c.c0, c.cpad
    return d


def _launch(c, cuda):
    """One launch of the case on the device -> (flat output buffer, statistics or None) on the host."""
    from qdiff import hip
    xbuf, outbuf, resbuf = (None if t is None else t.to(cuda) for t in C.make_buffers(c))
    xv, ov, rv = C.views(c, xbuf, outbuf, resbuf)
    wt = hip.pack_weights_bf16(c.w.to(cuda), c.dtype)
    bias = None if c.bias is None else c.bias.to(cuda)
    part = None
    if c.part is not None:
        part = torch.full(tuple(c.part.shape), float("nan"), dtype=torch.float32, device=cuda)
    # the alignment the case is about is the alignment the kernel sees
    esz = ov.element_size()
    assert xv.data_ptr() % 16 == 0 and ov.data_ptr() % 16 == c.out_mis * esz and (rv is None or rv.data_ptr() % 16 == c.res_mis * esz)
    if c.wrapper:
        hip.conv2d_bf16(xv, wt, bias, ov, c.B, c.H, c.W, c.cpad, c.Cout, k=c.k, pad=c.pad, residual=rv, gn_part=part, upsample2x=c.ups)
    else:
        d = _descriptor(hip, c, xbuf.data_ptr() + c.x_pre * 2, wt, bias, ov, rv, part)
        hip._check(hip.load().qd_conv2d_bf16(ctypes.byref(d), hip._stream()), "qd_conv2d_bf16")
    torch.cuda.synchronize()
    return outbuf.cpu(), None if part is None else part.cpu()


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_first_stage_conv_exact(cuda, name, record_property):
    c = C.get(name)
    outbuf, part = _launch(c, cuda)
    errors, which = C.check(c, outbuf, part)
    vec = c.Cout % 4 == 0 and c.ldo % 4 == 0 and c.out_mis == 0 and (c.res is None or (c.ldr % 4 == 0 and c.res_mis == 0))
    tile = "256x128" if c.Cout > 64 and ((c.M + 255) // 256) * ((c.Cout + 127) // 128) >= 256 else "128x128" if c.Cout > 64 else "128x64"
    print(f"{name}: {'FAIL' if errors else 'ok'} M={c.M} Cout={c.Cout} K={c.k * c.k}x{c.cpad} rows={str(c.odt)[6:]} tile={tile} "
          f"stores={'vector' if vec else 'per-element'} via={'wrapper' if c.wrapper else 'descriptor'}"
          + (f" subnormal operands: {which}" if c.want_alt is not None else "")
          + (f" rounding: inexact {c.stats[0]:.2f}, ties {c.stats[1]} towards zero / {c.stats[2]} away" if c.odt != torch.float32 and c.kind == "exact" else ""))
    if c.want_alt is not None:
        record_property("subnormal_operands", which)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_a_refused_descriptor_writes_nothing(cuda, dt):
    """upsample2x with an odd map is refused with the entry's message; the output keeps its bits."""
    from qdiff import hip
    c = C.get(f"b_ups_3x5_B3_{dt}")
    xbuf, outbuf, _ = (None if t is None else t.to(cuda) for t in C.make_buffers(c))
    _, ov, _ = C.views(c, xbuf, outbuf, None)
    wt = hip.pack_weights_bf16(c.w.to(cuda), c.dtype)
    d = _descriptor(hip, c, xbuf.data_ptr() + c.x_pre * 2, wt, c.bias.to(cuda), ov, None, None, H=c.H - 1)
    with pytest.raises(hip.HipEngineError, match="upsample2x needs stride 1, more than one tap, even H and W"):
        hip._check(hip.load().qd_conv2d_bf16(ctypes.byref(d), hip._stream()), "qd_conv2d_bf16")
    torch.cuda.synchronize()
    assert torch.equal(C.bits(outbuf.cpu()), C.bits(C.make_buffers(c)[1]))


def test_first_stage_conv_just_under_4GiB(cuda):
    """523775 rows of 4096 fp16 (4 290 764 800 bytes < 2^32), the last 8 columns live: every output row equals the 8-channel
    511 x 1025 convolution.  One row of the map more (H = 512) is refused with the entry's message and writes nothing.  The
    rows are allocated for H = 512, so either launch stays inside the allocation."""
    from qdiff import hip
    c = C.big_case()
    rows_alloc = (c.H + 1) * c.W
    xbuf = torch.zeros((rows_alloc, c.ldx), dtype=c.dtype, device=cuda)
    xbuf[:c.Mi, c.c0:] = c.x.to(cuda)
    outbuf = C.make_outbuf(c).to(cuda)
    ov = outbuf.as_strided((c.M, c.Cout), (c.ldo, 1), c.out_pre)
    wt = hip.pack_weights_bf16(c.w.to(cuda), c.dtype)
    bias = c.bias.to(cuda)
    d = _descriptor(hip, c, xbuf.data_ptr(), wt, bias, ov, None, None)
    assert d.B * d.H * d.W * d.ldx * 2 == 4290764800
    hip._check(hip.load().qd_conv2d_bf16(ctypes.byref(d), hip._stream()), "qd_conv2d_bf16")
    torch.cuda.synchronize()
    errors, _ = C.check(c, outbuf.cpu())
    print(f"{c.name}: {'FAIL' if errors else 'ok'} M={c.M} Cout={c.Cout} ldx={c.ldx} c0={c.c0} bytes={c.M * c.ldx * 2}")
    assert not errors, "\n".join(errors)
    out2 = torch.zeros((rows_alloc, c.Cout), dtype=torch.float32, device=cuda)
    d = _descriptor(hip, c, xbuf.data_ptr(), wt, bias, out2, None, None, H=c.H + 1)
    with pytest.raises(hip.HipEngineError, match="activation exceeds the 4-GiB offset range"):
        hip._check(hip.load().qd_conv2d_bf16(ctypes.byref(d), hip._stream()), "qd_conv2d_bf16")
    torch.cuda.synchronize()
    assert not bool(out2.any())
