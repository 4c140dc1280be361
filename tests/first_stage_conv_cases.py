"""Cases for the exact-row tests of the first-stage 16-bit convolution (qd_conv2d_bf16: the bf16 / fp16 mode of
csrc/igemm_dma.hip).  CPU only: torch on the host, no device and no import of the library, so the host test can check every
condition the GPU test relies on.

The idea.  The reference is exact, so no tolerance is needed.  Operands are small integers times a power of two (`ux` for the
activations, `uw` for the weights): bf16 and fp16 both hold them exactly, and so every product is an integer multiple of
ux * uw.  Bias and residual are integer multiples of `unit` (ux * uw is one too).  The builder asserts for every case that
sum_K |x||w| + |bias| + |residual| stays below 2^24 units: then every partial sum of every accumulation order is an integer
below 2^24 in units, i.e. an fp32 number, and the MFMA's adds, whatever their order and grouping, round nothing.  The same
holds for the epilogue's two adds (igemm_dma.hip, `single`: float(acc) + bias in phase 1, then + residual in phase 2).  The
fp64 convolution rounded to fp32 is therefore THE answer: fp32 rows must be torch.equal to it, 16-bit rows must be torch.equal
to its .to(dtype) — one round to nearest even.  16-bit-row cases are drawn so that this rounding is at work: at least 200 exact
ties, ties resolved both up and down, at least 10 % inexact elements (asserted per case).

Buffers.  Every tensor the kernel touches is a range of a larger flat buffer filled with a NaN bit pattern (SENT): the
activation rows [c0, c0 + clen) of rows ldx wide with GUARD rows before and after (a tap that wraps over a sample's edge, a
row beyond M, a channel beyond clen reads NaN and poisons an output), the residual likewise, and the output, where every byte
outside [0, M) x [0, Cout) must keep its bits.  `out_mis` / `res_mis` shift a tensor's start by that many ELEMENTS off a
16-byte boundary.

GroupNorm statistics (gn cases).  The kernel adds v = acc + bias + residual into the per-chunk sums — the residual IS part of
the value the statistics take (`gs[e] += v[e]` runs after `v += rs[ps]`) — as fp32 sums and fused multiply-adds over a lane's
rows, a butterfly and a fixed-order LDS reduction.  With integer-valued |v| <= 160 a 128-row sum of squares stays below 2^24,
every order is exact, and gn_part must equal the reference's sums bit for bit.

Values cases (`kind == "values"`) carry non-finite or extreme operands; their expected rows are defined here by fp32 torch
arithmetic in the kernel's order, element by element (accumulate, + bias, + residual): see _plant().  NaN outputs compare as
"is NaN" (the payload is not specified).  Subnormal cases carry two exact references — operands used as they are, and
subnormal 16-bit operands read as zero — and a launch must equal ONE of them as a whole.
"""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

GUARD = 2                       # guard rows before and after every row range
SENT = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float16: (torch.int16, 0x7FA5), torch.bfloat16: (torch.int16, 0x7FA5)}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MIN_TIES, MIN_TIES_EACH_WAY, MIN_INEXACT = 200, 10, 0.10
BIG = dict(B=1, H=511, W=1025, c0=4088, clen=8, ldx=4096, Cout=8)      # the launch just under 4 GiB (fp16 only)


def pad8(n):
    return (n + 7) // 8 * 8


def filled(n, dtype):
    it, pat = SENT[dtype]
    return torch.full((n,), pat, dtype=it).view(dtype)


def bits(t):
    return t.contiguous().view(SENT[t.dtype][0])


def _ints(g, shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=g).double()


# ---- geometry -----------------------------------------------------------------------------------------------------------------

def _geometry(c):
    c.Hs, c.Ws = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)            # the stored map
    c.Mi = c.B * c.Hs * c.Ws
    c.Ho = (c.H + 2 * c.pad - c.k) // c.stride + 1
    c.Wo = (c.W + 2 * c.pad - c.k) // c.stride + 1
    c.M = c.B * c.Ho * c.Wo
    c.cpad = pad8(c.Cin)                                                  # clen of the launch
    c.ldx = c.ldx or c.c0 + c.cpad
    c.ldo = c.ldo or c.Cout
    c.ldr = c.ldr or c.Cout
    assert c.ldx % 8 == 0 and c.c0 % 8 == 0 and c.c0 + c.cpad <= c.ldx and c.ldo >= c.Cout and c.ldr >= c.Cout
    c.x_pre = GUARD * c.ldx
    c.out_pre = pad8(GUARD * c.ldo) + c.out_mis
    c.res_pre = pad8(GUARD * c.ldr) + c.res_mis
    # reachable through hip.conv2d_bf16 (stride-1 'same' convolution, c0 = 0); everything else needs a hand-built descriptor
    c.wrapper = c.c0 == 0 and c.stride == 1 and c.pad == c.k // 2
    return c


def make_outbuf(c):
    return filled(c.out_pre + c.M * c.ldo + GUARD * c.ldo + 8, c.odt)


def make_buffers(c):
    """CPU buffers of one launch: (xbuf, outbuf, resbuf or None), flat, SENT outside the tensors' ranges."""
    xbuf = filled(c.x_pre + c.Mi * c.ldx + GUARD * c.ldx, c.dtype)
    xbuf.as_strided((c.Mi, c.cpad), (c.ldx, 1), c.x_pre + c.c0).copy_(c.x)
    outbuf = make_outbuf(c)
    resbuf = None
    if c.res is not None:
        resbuf = filled(c.res_pre + c.M * c.ldr + GUARD * c.ldr + 8, c.odt)
        resbuf.as_strided((c.M, c.Cout), (c.ldr, 1), c.res_pre).copy_(c.res)
    return xbuf, outbuf, resbuf


def views(c, xbuf, outbuf, resbuf):
    """(x rows [Mi][clen] at column c0, out [M][Cout], residual [M][Cout] or None) as strided views of the flat buffers, on
    whichever device they live."""
    xv = xbuf.as_strided((c.Mi, c.cpad), (c.ldx, 1), c.x_pre + c.c0)
    ov = outbuf.as_strided((c.M, c.Cout), (c.ldo, 1), c.out_pre)
    rv = None if resbuf is None else resbuf.as_strided((c.M, c.Cout), (c.ldr, 1), c.res_pre)
    return xv, ov, rv


# ---- the two references -------------------------------------------------------------------------------------------------------

def _w_padded(c):
    w = torch.zeros((c.Cout, c.cpad, c.k, c.k), dtype=torch.float64)
    w[:, :c.Cin] = c.w.double()
    return w


def conv64(c, x=None, w=None):
    """fp64 F.conv2d (+ F.interpolate(nearest) for the up-sample fold) of the rows x [Mi][clen] -> [M][Cout]."""
    x = c.x.double() if x is None else x
    xi = x.reshape(c.B, c.Hs, c.Ws, c.cpad).permute(0, 3, 1, 2)
    if c.ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xi, _w_padded(c) if w is None else w, None, stride=c.stride, padding=c.pad)
    assert tuple(y.shape[2:]) == (c.Ho, c.Wo)
    return y.permute(0, 2, 3, 1).reshape(c.M, c.Cout)


def conv_int(c, x=None, upmap=lambda i: i >> 1, drop=None):
    """The second computation: gather per tap + int64 matmul, in units of ux * uw.  `upmap`: up-sampled index -> stored index;
    `drop` = (output row m, tap): that tap is left out of that row (a planted mistake of the host test)."""
    x = c.x.double() if x is None else x
    xi = torch.round(x / c.ux).long()
    assert torch.equal(xi.double() * c.ux, x), "activations are not integer multiples of ux"
    wi = torch.round(_w_padded(c) / c.uw).long()
    assert torch.equal(wi.double() * c.uw, _w_padded(c)), "weights are not integer multiples of uw"
    xi = xi.reshape(c.B, c.Hs, c.Ws, c.cpad)
    if c.ups:
        ih, iw = upmap(torch.arange(c.H)).clamp(0, c.Hs - 1), upmap(torch.arange(c.W)).clamp(0, c.Ws - 1)
        xi = xi[:, ih][:, :, iw]
    xp = F.pad(xi.permute(0, 3, 1, 2), (c.pad, c.pad, c.pad, c.pad))
    acc = torch.zeros((c.M, c.Cout), dtype=torch.int64)
    for r in range(c.k):
        for q in range(c.k):
            sl = xp[:, :, r:r + c.stride * (c.Ho - 1) + 1:c.stride, q:q + c.stride * (c.Wo - 1) + 1:c.stride]
            term = sl.permute(0, 2, 3, 1).reshape(c.M, c.cpad) @ wi[:, :, r, q].t()
            if drop is not None and drop[1] == r * c.k + q:
                term[drop[0]] = 0
            acc += term
    return acc


def finish(c, acc32, bias=None, res=None):
    """The epilogue in the kernel's order, in fp32: float(acc) + bias, then + residual."""
    bias = c.bias if bias is None else bias
    res = c.res if res is None else res
    v = acc32.float()
    if bias is not None:
        v = v + bias.float()[None, :]
    if res is not None:
        v = v + res.float()
    return v


def gn_sums(c, v32):
    """[B][Ho*Wo/128][Cout][2] fp32 sums and sums of squares of 128-row chunks (exact: asserted by the builder)."""
    v = v32.double().reshape(c.B, c.Ho * c.Wo // 128, 128, c.Cout)
    return torch.stack([v.sum(2), (v * v).sum(2)], dim=-1).float()


def round_stats(v32, dtype):
    """(inexact fraction, ties rounded towards zero, ties rounded away from zero) of one rounding v32 -> dtype."""
    r = v32.to(dtype)
    d = v32.double() - r.double()
    inexact = d != 0
    # the 16-bit neighbour on the other side of v32: one step in magnitude, up when v32 lies beyond r, down otherwise
    away = (d > 0) == (r.double() > 0)
    nb = (bits(r) + torch.where(away, 1, -1).to(torch.int16)).view(dtype).double()
    tie = inexact & (r.double() != 0) & torch.isfinite(nb) & ((nb - v32.double()).abs() == d.abs())
    return inexact.double().mean().item(), int((tie & away).sum()), int((tie & ~away).sum())


def truncated(v32, dtype):
    """v32 -> dtype by dropping the low bits (the planted mistake 'truncation instead of round to nearest even')."""
    r = v32.to(dtype)
    beyond = r.double().abs() > v32.double().abs()
    return (bits(r) - beyond.to(torch.int16)).view(dtype)


# ---- the builder --------------------------------------------------------------------------------------------------------------

def _make(name, dt, B, H, W, Cin, Cout, k=3, *, rows16=False, res=False, ups=False, stride=1, pad=None, c0=0, ldx=0, ldo=0, ldr=0,
          out_mis=0, res_mis=0, gn=False, seed=0, amp=None, bias_amp=None, res_amp=None, x=None, w=None, bias=None, ux=1.0, uw=1.0,
          unit=0.5, kind="exact", flush_alt=False):
    dtype = DTYPES[dt]
    c = NS(name=name, dt=dt, dtype=dtype, odt=dtype if rows16 else torch.float32, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, ups=ups,
           stride=stride, pad=k // 2 if pad is None else pad, c0=c0, ldx=ldx, ldo=ldo, ldr=ldr, out_mis=out_mis, res_mis=res_mis,
           gn=gn, kind=kind, ux=ux, uw=uw, unit=unit, want_alt=None, part=None, onehot=False)
    _geometry(c)
    g = torch.Generator().manual_seed(1000 + seed)
    # operand amplitudes: sums must reach past the 16-bit significand (8 bits for bf16, 11 for fp16) for the rounding to work
    ax, aw = amp or ((16, 16) if dt == "bf16" else (32, 32))
    c.x = (_ints(g, (c.Mi, c.cpad), ax) * ux if x is None else x.double()).to(dtype)      # pad channels hold data too: their weights are zero
    c.w = (_ints(g, (Cout, Cin, k, k), aw) * uw if w is None else w.double()).float()
    ba = 2 * ax * aw if bias_amp is None else bias_amp
    c.bias = (_ints(g, (Cout,), ba) * unit).float() if bias is None else bias
    if isinstance(c.bias, str):
        c.bias = None                                                                      # bias="none": a null bias pointer
    c.res = None
    if res:
        ra = res_amp or (100 if rows16 else 2000)
        runit = max(unit, 1.0) if rows16 else unit                                         # 16-bit residuals: integers, exact in 8 bits
        c.res = (_ints(g, (c.M, Cout), ra) * runit).to(c.odt)
    assert x is None or torch.equal(c.x.double(), x.double()), f"{name}: the given activations are not exact in {dt}"
    # ---- conditions on the inputs
    assert torch.equal(c.x.double().to(dtype).double(), c.x.double()) and torch.equal(c.w.to(dtype).double(), c.w.double()), \
        f"{name}: operands are not exact in {dt}"
    if kind == "exact":
        _reference(c)
        if flush_alt:
            sub = c.x.double().abs() < (2.0 ** -14 if dt == "fp16" else 2.0 ** -126)
            assert sub.any() and (~sub).any()
            xz = torch.where(sub, 0.0, c.x.double())
            c.want32_alt = finish(c, conv64(c, xz))
            assert torch.equal(c.want32_alt.double(), conv_like(c, xz)), name
            c.want_alt = c.want32_alt.to(c.odt)
            assert not torch.equal(c.want, c.want_alt)
    return c


def conv_like(c, x):
    """fp64 value of the whole epilogue (the exactness check of a reference)."""
    y = conv64(c, x)
    if c.bias is not None:
        y = y + c.bias.double()[None, :]
    if c.res is not None:
        y = y + c.res.double()
    return y


def _reference(c):
    name = c.name
    for t, what in ((c.bias, "bias"), (c.res, "residual")):
        if t is not None:
            assert torch.equal((t.double() / c.unit).round() * c.unit, t.double()), f"{name}: {what} is not a multiple of the unit"
    assert (c.ux * c.uw / c.unit) == round(c.ux * c.uw / c.unit), f"{name}: a product is not a multiple of the unit"
    bound = conv64(c, c.x.double().abs(), _w_padded(c).abs())
    if c.bias is not None:
        bound = bound + c.bias.double().abs()[None, :]
    if c.res is not None:
        bound = bound + c.res.double().abs()
    c.bound_units = bound.max().item() / c.unit
    assert c.bound_units < 2 ** 24, f"{name}: sum |x||w| + |bias| + |residual| = {c.bound_units} units >= 2^24"
    y64 = conv64(c)
    c.acc32 = y64.float()
    assert torch.equal(c.acc32.double(), y64), f"{name}: the fp64 convolution is not an fp32 number"
    c.want32 = finish(c, c.acc32)
    assert torch.equal(c.want32.double(), conv_like(c, c.x.double())), f"{name}: the fp32 epilogue rounded"
    c.want = c.want32.to(c.odt)
    assert torch.isfinite(c.want).all(), f"{name}: a row overflows {c.odt} (that edge belongs to the values cases)"
    if c.odt != torch.float32:
        c.stats = round_stats(c.want32, c.odt)
        inexact, down, up = c.stats
        assert down + up >= MIN_TIES and min(down, up) >= MIN_TIES_EACH_WAY and inexact >= MIN_INEXACT, \
            f"{name}: rounding not exercised: inexact {inexact:.3f}, ties towards zero {down}, away {up}"
    if c.gn:
        assert (c.Ho * c.Wo) % 128 == 0 and c.odt == torch.float32
        v = c.want32.double()
        assert torch.equal(v, v.round()) and v.abs().max().item() <= 160, f"{name}: statistics need integer |y| <= 160"
        c.part = gn_sums(c, c.want32)                          # 128 * 160^2 < 2^24: every partial sum is an fp32 integer


def _receptive(c, hs, ws):
    """[(output pixel (ho, wo), tap)] whose gather reads the stored pixel (hs, ws) — set_tap's arithmetic."""
    hits = []
    for ho in range(c.Ho):
        for wo in range(c.Wo):
            for t in range(c.k * c.k):
                ih, iw = ho * c.stride - c.pad + t // c.k, wo * c.stride - c.pad + t % c.k
                if 0 <= ih < c.H and 0 <= iw < c.W and ((ih >> 1, iw >> 1) if c.ups else (ih, iw)) == (hs, ws):
                    hits.append((ho, wo, t))
    return hits


def _plant(c, b, hs, ws, ch, value):
    """Put `value` (inf / NaN) into channel ch of the stored pixel (b, hs, ws).  Expected rows: the finite accumulator (that
    operand read as zero) plus, tap by tap, fp32(weight) * value in fp32 torch arithmetic, then the epilogue's adds: an output
    whose receptive field holds the pixel becomes +-inf by the weight's sign, NaN where the weight is zero, where two taps
    disagree in sign, or where the operand is NaN; every other output keeps the finite reference's bits."""
    assert c.x[(b * c.Hs + hs) * c.Ws + ws, ch] == 0 and ch < c.Cin
    acc = c.acc32.clone()
    touched = torch.zeros(c.M, dtype=torch.bool)
    val = torch.tensor(value, dtype=torch.float32)
    for ho, wo, t in _receptive(c, hs, ws):
        m = (b * c.Ho + ho) * c.Wo + wo
        acc[m] = acc[m] + c.w[:, ch, t // c.k, t % c.k] * val
        touched[m] = True
    c.x[(b * c.Hs + hs) * c.Ws + ws, ch] = value
    c.kind, c.touched = "values", touched
    finite = c.want32
    c.want32 = finish(c, acc)
    c.want = c.want32.to(c.odt)
    assert touched.any() and not torch.isfinite(c.want32[touched]).any()                   # (no zero weights on a lone tap but the NaN one)
    assert torch.equal(c.want32[~touched], finite[~touched]) and torch.isfinite(finite).all()
    return c


def decode_tap(v):
    """A weight of the one-hot case -> '(n, c, tap)'; anything else -> 'not a single weight'."""
    v = float(v)
    if v <= 0 or v != int(v):
        return "not a single weight"
    v, ch = int(v), 0
    while v % 2 == 0:
        v //= 2
        ch += 1
    code = (v - 1) // 2
    return f"(n={code // 9}, c={ch}, tap={code % 9})" if ch < 8 and code < 36 else "not a single weight"


ONEHOT_PIXELS = [(0, 0), (0, 6), (6, 0), (6, 6), (0, 3), (3, 0), (3, 6), (6, 3), (3, 3)]      # corners, edge midpoints, interior


def _onehot(name, dt):
    """7x7 maps, B = 2: a single 1 at each corner, each edge midpoint and one interior pixel of the first and the last sample
    (channel = pixel index mod 8), weights w[n][c][tap] = (2 * (9 n + tap) + 1) * 2^c: the pixels lie three apart, so every
    output is zero or ONE weight, and a wrong output names the tap it took (decode_tap)."""
    B, H, W, Cin, Cout = 2, 7, 7, 8, 4
    x = torch.zeros((B * H * W, Cin), dtype=torch.float64)
    for b in range(B):
        for i, (h, w) in enumerate(ONEHOT_PIXELS):
            x[(b * H + h) * W + w, (i + 3 * b) % 8] = 1.0
    n, ch, t = torch.meshgrid(torch.arange(Cout), torch.arange(Cin), torch.arange(9), indexing="ij")
    w = ((2 * (9 * n + t) + 1) * 2 ** ch).double().reshape(Cout, Cin, 3, 3)
    c = _make(name, dt, B, H, W, Cin, Cout, x=x, w=w, bias="none", unit=1.0)
    c.onehot = True
    assert all(decode_tap(v) != "not a single weight" for v in c.want32[c.want32 != 0].tolist())
    return c


def _values_max(name, dt):
    """The largest finite operand times +-1 (1x1, one live channel per output): fp32 rows hold it exactly."""
    dtype = DTYPES[dt]
    big = torch.finfo(dtype).max
    M, Cin, Cout = 37, 8, 8
    x = torch.zeros((M, Cin), dtype=torch.float64)
    x[:, 0] = torch.tensor([big, -big, big / 2, 3.0] * 10)[:M]
    x[:, 1:] = _ints(torch.Generator().manual_seed(7), (M, Cin - 1), 8)
    w = torch.zeros((Cout, Cin, 1, 1), dtype=torch.float64)
    w[:, 0, 0, 0] = torch.tensor([1.0, -1.0] * 4)
    c = _make(name, dt, 1, 1, M, Cin, Cout, k=1, x=x, w=w, bias="none", kind="values")
    c.want32 = (c.x[:, 0].float()[:, None] * c.w[:, 0, 0, 0][None, :])                     # one term per output: no order
    c.want = c.want32.to(c.odt)
    assert c.want32.abs().max().item() == big
    return c


def _values_h65520(name, dt):
    """fp16 rows at the top of the range: 65504 + 15 = 65519 rounds to 65504, 65504 + 16 = 65520 is the tie that rounds to inf."""
    assert dt == "fp16"
    M, Cin, Cout = 40, 8, 8
    x = torch.zeros((M, Cin), dtype=torch.float64)
    x[:, 0] = 65504.0
    x[:, 1] = torch.tensor([15.0, 16.0, 17.0, 0.0] * 10)
    w = torch.zeros((Cout, Cin, 1, 1), dtype=torch.float64)
    w[:, 0, 0, 0] = torch.tensor([1.0, -1.0] * 4)
    w[:, 1, 0, 0] = torch.tensor([1.0, -1.0] * 4)
    c = _make(name, dt, 1, 1, M, Cin, Cout, k=1, rows16=True, x=x, w=w, bias="none", kind="values")
    c.want32 = c.x[:, 0].float()[:, None] * c.w[:, 0, 0, 0][None, :] + c.x[:, 1].float()[:, None] * c.w[:, 1, 0, 0][None, :]   # exact in fp32
    c.want = c.want32.to(c.odt)
    assert c.want32[0, 0] == 65519 and c.want[0, 0] == 65504 and c.want32[1, 0] == 65520 and torch.isinf(c.want[1, 0]) and c.want[1, 1] == -float("inf")
    return c


def _values_overflow(name, dt):
    """A product beyond fp32 (bf16 only: 2^100 * 2^100; one such term per output, so no inf - inf): +-inf by the signs."""
    assert dt == "bf16"
    M, Cin, Cout = 33, 8, 8
    x = torch.zeros((M, Cin), dtype=torch.float64)
    x[:, 0] = torch.tensor([2.0 ** 100, -2.0 ** 100, 2.0 ** 20] * 11)
    x[:, 1] = 3.0
    w = torch.zeros((Cout, Cin, 1, 1), dtype=torch.float64)
    w[:, 0, 0, 0] = torch.tensor([2.0 ** 100, -2.0 ** 100] * 4)
    w[:, 1, 0, 0] = 5.0
    c = _make(name, dt, 1, 1, M, Cin, Cout, k=1, x=x, w=w, bias="none", kind="values")
    c.want32 = c.x[:, 0].float()[:, None] * c.w[:, 0, 0, 0][None, :] + 15.0               # inf + 15 = inf; 2^120 + 15 rounds to 2^120 in any order
    c.want = c.want32.to(c.odt)
    assert torch.isinf(c.want32[0]).all() and torch.isfinite(c.want32[2]).all()
    return c


def _planted(name, dt, where, value):
    kw = dict(amp=(8, 8), seed=31)
    if where == "ups":
        c = _make(name, dt, 2, 6, 10, 13, 12, ups=True, **kw)
        b, hs, ws = 1, 1, 2
    else:
        c = _make(name, dt, 3, 5, 6, 13, 12, res=(where == "last"), **kw)
        b, hs, ws = {"interior": (0, 2, 3), "corner": (1, 0, 0), "last": (2, 4, 5)}[where]
    # the planted channel: weights of both signs, never zero except ONE (n = 5, centre tap): inf * 0 = NaN there
    ch = 4
    g = torch.Generator().manual_seed(3)
    wch = _ints(g, (c.Cout, 3, 3), 3)
    wch = torch.where(wch == 0, 2.0, wch)
    wch[5, 1, 1] = 0.0
    c.w[:, ch] = wch.float()
    c.x[(b * c.Hs + hs) * c.Ws + ws, ch] = 0
    _reference(c)
    return _plant(c, b, hs, ws, ch, value)


def _subnormal(name, dt):
    """Subnormal 16-bit activations beside normal ones in every row.  fp16: 2^-24 .. 2^-15 times weights +-2^10 (products
    2^-14 .. 2^-5); bf16: 2^-133 .. 2^-127 times +-2^100.  Two exact references: operands as they are / subnormal operands read
    as zero."""
    M, Cin, Cout = 150, 16, 40
    g = torch.Generator().manual_seed(17)
    lo, hi, wexp = (-24, -15, 10) if dt == "fp16" else (-133, -127, 100)
    e = torch.randint(lo, hi + 1, (M, Cin), generator=g).double()
    x = torch.where(torch.rand((M, Cin), generator=g) < 0.5, 1.0, -1.0) * 2.0 ** e
    normal = (2.0 ** -14 if dt == "fp16" else 2.0 ** -126)
    x[:, ::2] = _ints(g, (M, Cin // 2), 8) * normal                                        # normal operands (and zeros) on the even channels
    x[::7] = torch.where(torch.arange(Cin) % 2 == 0, 0.0, 2.0 ** lo)                       # rows whose only live operands are the smallest subnormal
    w = torch.where(torch.rand((Cout, Cin, 1, 1), generator=g) < 0.5, 1.0, -1.0) * 2.0 ** wexp
    return _make(name, dt, 1, 6, 25, Cin, Cout, k=1, x=x, w=w, bias="none", ux=2.0 ** lo, uw=2.0 ** wexp, unit=2.0 ** (lo + wexp), flush_alt=True)


def _gn(name, dt, B):
    """256-row tiles with first-level GroupNorm statistics: ceil(M / 256) >= 256 at Cout = 128 selects the 256 x 128 tile; with
    B = 513 samples of 8 x 16 = 128 rows the last tile holds 128 real rows (B = 512: none ragged).  x in [-2, 2], w in [-1, 1],
    integer bias and residual in [-8, 8]: |y| <= 160.  The residual is part of the value the statistics take (module docstring)."""
    c = _make(name, dt, B, 8, 16, 8, 128, res=True, gn=True, amp=(2, 1), bias_amp=8, res_amp=8, unit=1.0, seed=B)
    assert (c.M + 255) // 256 >= 256 and ((c.M % 256 == 128) == (B == 513))
    return c


def big_case():
    """The launch just under 4 GiB: rows of ldx = 4096 fp16, the last 8 columns live, B, H, W = 1, 511, 1025 (523775 rows,
    4 290 764 800 bytes < 2^32); 3x3, Cout = 8, fp32 rows.  c.x holds the 8 live columns only: the GPU test allocates the rows."""
    assert BIG["H"] * BIG["W"] * BIG["ldx"] * 2 == 4290764800 < 2 ** 32 <= (BIG["H"] + 1) * BIG["W"] * BIG["ldx"] * 2
    c = _make("just_under_4GiB_fp16", "fp16", 1, BIG["H"], BIG["W"], BIG["clen"], BIG["Cout"], seed=99)
    c.c0, c.ldx, c.x_pre, c.wrapper = BIG["c0"], BIG["ldx"], 0, False
    return c


def _registry():
    R = {}

    def add(name, fn, *a, only=None, **kw):
        for dt in DTYPES:
            if only in (None, dt):
                full = f"{name}_{dt}"
                assert full not in R
                R[full] = functools.partial(fn, full, dt, *a, **kw)
    # ragged M and neighbours: M = 1, 25, 189, 129, 255, 257 (3x3), two of them also 1x1
    add("m_1x1x1_k3", _make, 1, 1, 1, 24, 32, seed=1)
    add("m_1x5x5_k3", _make, 1, 5, 5, 24, 32, seed=2)
    add("m_3x7x9_k3", _make, 3, 7, 9, 40, 64, rows16=True, seed=3)
    add("m_1x3x43_k3", _make, 1, 3, 43, 24, 96, rows16=True, seed=4)
    add("m_1x15x17_k3", _make, 1, 15, 17, 24, 40, rows16=True, seed=5)
    add("m_1x1x257_k3", _make, 1, 1, 257, 24, 32, seed=6)
    add("m_3x7x9_k1", _make, 3, 7, 9, 40, 64, k=1, seed=7)
    add("m_1x1x257_k1", _make, 1, 1, 257, 24, 32, k=1, rows16=True, seed=8)
    # N edges at M = 189: the per-element path (3, 5, 65, 70, 129), the 128-wide tile with 63 / 58 absent columns, a second
    # N-block with one real column (129), three N-blocks (288)
    for n in (3, 5, 64, 65, 70, 129, 288):
        add(f"n_{n}", _make, 3, 7, 9, 16, n, rows16=n in (65, 129, 288), seed=10 + n)
    add("n_64_rows16", _make, 3, 7, 9, 16, 64, rows16=True, seed=9)
    # output and residual as column ranges
    add("col_ldo_rows32", _make, 3, 7, 9, 16, 64, ldo=72, seed=20)
    add("col_ldo_rows16", _make, 3, 7, 9, 16, 64, ldo=72, rows16=True, seed=21)
    add("col_mis128_rows32", _make, 3, 7, 9, 16, 128, out_mis=1, seed=22)
    add("col_mis128_rows16", _make, 3, 7, 9, 16, 128, out_mis=1, rows16=True, seed=23)
    add("col_resmis_rows32", _make, 3, 7, 9, 16, 64, res=True, ldr=68, res_mis=1, seed=24)
    add("col_resmis_rows16", _make, 3, 7, 9, 16, 64, res=True, ldr=68, res_mis=1, rows16=True, seed=25)
    add("col_outmis_rows32", _make, 3, 7, 9, 16, 64, res=True, ldr=68, ldo=72, out_mis=1, seed=26)
    add("col_outmis_rows16", _make, 3, 7, 9, 16, 64, res=True, ldr=68, ldo=72, out_mis=1, rows16=True, seed=27)
    # K edges: Cin_pad in {8, 24, 32, 40, 72} (three channels short of it: zero weights against live pad channels); the
    # activations as a column range of wider rows, every column outside [c0, c0 + clen) NaN
    for cp in (8, 24, 32, 40, 72):
        add(f"k_cpad{cp}", _make, 3, 7, 9, cp - 3, 32, seed=30 + cp)
    add("k_c0_8_ldx48", _make, 3, 7, 9, 21, 32, c0=8, ldx=48, seed=40)
    add("k_c0_24_ldx96", _make, 3, 7, 9, 69, 32, c0=24, ldx=96, rows16=True, seed=41)
    # borders
    add("b_H1", _make, 2, 1, 9, 16, 32, seed=50)
    add("b_W1", _make, 2, 9, 1, 16, 32, seed=51)
    add("b_ups_1x1", _make, 1, 2, 2, 8, 32, ups=True, seed=52)
    add("b_ups_3x5_B3", _make, 3, 6, 10, 16, 32, ups=True, seed=53)
    add("b_ups_8x8_res_rows16", _make, 1, 16, 16, 16, 64, ups=True, res=True, rows16=True, seed=54)
    add("b_onehot", _onehot)
    # other strides and paddings (hand-built descriptor)
    add("s_stride2_pad1_8x8", _make, 2, 8, 8, 16, 32, stride=2, seed=60)
    add("s_pad0_6x6", _make, 2, 6, 6, 16, 32, pad=0, seed=61)
    # 256-row tiles with statistics
    add("gn_B513", _gn, 513)
    add("gn_B512", _gn, 512)
    # values
    add("v_max", _values_max)
    add("v_h65520", _values_h65520, only="fp16")
    add("v_overflow", _values_overflow, only="bf16")
    for where in ("interior", "corner", "ups", "last"):
        add(f"v_inf_{where}", _planted, where, float("inf"))
        add(f"v_nan_{where}", _planted, where, float("nan"))
    add("sub", _subnormal)
    return R


_REG = _registry()
CASE_NAMES = sorted(_REG)


@functools.lru_cache(maxsize=None)
def get(name):
    return _REG[name]()


# ---- the comparison of the GPU test ---------------------------------------------------------------------------------------------

def _where(c, m, n):
    b, rem = divmod(m, c.Ho * c.Wo)
    return f"row {m} (sample {b}, pixel ({rem // c.Wo}, {rem % c.Wo})), column {n}"


def _same(got, want):
    """Element-wise: equal values, or NaN where NaN is expected."""
    return (got == want) | (torch.isnan(got) & torch.isnan(want))


def check(c, outbuf, part=None):
    """outbuf: the flat output buffer after the launch (CPU).  Returns (errors, which): no tolerance anywhere — rows equal the
    reference (one of the two references for subnormal cases, as a whole), every byte outside [0, M) x [0, Cout) keeps SENT."""
    errors = []
    assert outbuf.dtype == c.odt and outbuf.dim() == 1
    inside = torch.zeros(outbuf.numel(), dtype=torch.bool)
    inside.as_strided((c.M, c.Cout), (c.ldo, 1), c.out_pre).fill_(True)
    outside = bits(outbuf)[~inside]
    bad = (outside != SENT[c.odt][1]).nonzero()
    if bad.numel():
        pos = (~inside).nonzero()[bad[0, 0]].item()
        errors.append(f"{c.name}: {bad.shape[0]} elements outside the output changed, first at flat element {pos} "
                      f"(out starts at {c.out_pre}, ldo {c.ldo}, Cout {c.Cout}, M {c.M})")
    got = outbuf.as_strided((c.M, c.Cout), (c.ldo, 1), c.out_pre)
    refs = [("as_is", c.want)] + ([("flushed", c.want_alt)] if c.want_alt is not None else [])
    which, miss = None, None
    for label, want in refs:
        ok = _same(got.float(), want.float())
        if bool(ok.all()):
            which = label
            break
        miss = miss if miss is not None else (~ok, want)
    if which is None:
        wrong, want = miss
        m, n = wrong.nonzero()[0].tolist()
        msg = (f"{c.name}: {int(wrong.sum())} of {wrong.numel()} outputs differ, first at {_where(c, m, n)}: got {got[m, n].item()!r}, "
               f"want {want[m, n].item()!r}" + (f" (fp32 value {c.want32[m, n].item()!r})" if c.odt != torch.float32 else ""))
        if c.onehot:
            msg += f"; got is the weight {decode_tap(got[m, n])}, want {decode_tap(want[m, n])}"
        if c.want_alt is not None:
            msg += f"; neither reference matches as a whole (flushed reference: {int((~_same(got.float(), c.want_alt.float())).sum())} differ)"
        errors.append(msg)
    if c.part is not None:
        if part is None:
            errors.append(f"{c.name}: no statistics returned")
        else:
            wrong = bits(part) != bits(c.part)
            if bool(wrong.any()):
                b, ch, n, s = wrong.nonzero()[0].tolist()
                errors.append(f"{c.name}: {int(wrong.sum())} statistics differ, first at sample {b} chunk {ch} channel {n} "
                              f"{'sum of squares' if s else 'sum'}: got {part[b, ch, n, s].item()!r}, want {c.part[b, ch, n, s].item()!r}")
    return errors, which
