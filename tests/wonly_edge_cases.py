"""Named edge cases of the fp16 / bf16 weights-only kernels, built on the CPU: the inputs, the fp64 reference and the
per-element tolerance of each.  tests/test_weight_only_edges_host.py runs the library's fp32 op + cast through every case (the
bound admits a correct fp32 implementation), tests/test_weight_only_edges_gpu.py runs the kernels.

The references and tolerances are those of the random-draw files (imported, not copied): _ln_ref / _geglu_ref / _gn_ref and
_half_ulp of test_weight_only_fused_gpu.py, _contraction_ref of test_weight_only_gpu.py, _reference / _check of
test_weight_only_attention_gpu.py, _epi_ref of test_weight_only_wide_gpu.py.

A. Launch forms that only the benchmark reaches.  The shapes follow from these launcher constants (q-diffusion_amd/csrc/norm_quant.hip); whoever
   changes a cap resizes the case next to it:
     launch_ln_h16    at most 4096 blocks x 4 waves x 2 rows = LN_PASS = 32768 rows in one trip of ln_h16_kernel's loop
     h16_stream_grid  at most 8192 blocks x 256 threads = STREAM_PASS = 2,097,152 chunks of 8 channels (counted over ldo / 8 per
                      row) in one trip of geglu_h16_kernel's / gn_apply_h16_kernel's loop
     qd_attn_h16      key tiles of 32: S = 4096 is 128 tiles
B. Value edges: rounding ties and subnormal results of the one rounding to the operand type, results past the fp16 range,
   degenerate and offset statistics, qd_erff's branch point and far tails, the cancellation of 1 + erf.
"""
import functools
import math
from types import SimpleNamespace as NS

import torch

from test_weight_only_attention_gpu import _reference
from test_weight_only_fused_gpu import _geglu_ref, _gn_ref, _half_ulp, _ln_ref
from test_weight_only_gpu import _codes, _contraction_ref, _wquant
from test_weight_only_wide_gpu import _epi_host, _epi_ref

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
LN_PASS = 4096 * 4 * 2                 # launch_ln_h16: rows of one trip
STREAM_PASS = 8192 * 256               # h16_stream_grid: 8-channel chunks of one trip
OUT_MAX = {F16: 65504.0, BF16: 3.3895313892515355e38}
EPS = 1e-5


def name(dt):
    return str(dt)[6:]


def range_ratio(got, ref, tol, odt):
    """Worst |got - ref| / tol over the elements whose reference is below 0.99 x the output type's maximum; an fp16 result
    whose reference is past 1.01 x 65520 must be the infinity of the reference's sign; NaN nowhere."""
    got = got.double()
    assert not torch.isnan(got).any(), "NaN in the output"
    inside = ref.abs() < 0.99 * OUT_MAX[odt]
    assert torch.isfinite(got[inside]).all(), "an in-range result is not finite"
    if odt == F16:
        over = ref.abs() > 1.01 * 65520.0
        assert torch.equal(got[over], torch.sign(ref[over]) * math.inf), "a result past the fp16 range is not the signed infinity"
    return ((got - ref).abs() / tol)[inside].max().item()


# ---- A. long launches --------------------------------------------------------------------------------------------------------
LN_LONG_M = LN_PASS + 3                # odd: the last row pair of the second trip is one real row and one clamped row
LN_LONG = [(C, xdt, odt, pad) for C in (8, 320) for xdt in (F32, F16) for odt in (F16, BF16) for pad in (0, 8)]   # C = 8: NV = 1, one chunk


@functools.lru_cache(maxsize=2)
def _ln_long_data(C, xdt):
    g = torch.Generator().manual_seed(7000 + C)
    M = LN_LONG_M
    x = (torch.randn(M, C, generator=g) * (0.2 + 3 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).to(xdt)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return (x, gamma, beta) + _ln_ref(x, gamma, beta, EPS)


def ln_long(C, xdt, odt, pad):
    x, gamma, beta, ref, T = _ln_long_data(C, xdt)
    return NS(kind="ln", x=x, gamma=gamma, beta=beta, eps=EPS, odt=odt, pad=pad, ref=ref, tol=_half_ulp(ref, odt) + T, second_trip=LN_PASS)


# (F, ldo, M): M * ldo / 8 just above STREAM_PASS.  8/64: seven of eight chunks are pad columns; 320/320: none is.
GEGLU_LONG = [(8, 64, STREAM_PASS // 8 + 3, F32, F16), (8, 64, STREAM_PASS // 8 + 3, F16, BF16),
              (320, 320, STREAM_PASS // 40 + 2, F32, BF16), (320, 320, STREAM_PASS // 40 + 2, F16, F16)]


@functools.lru_cache(maxsize=1)
def _geglu_long_data(Fd, M, xdt):
    g = torch.Generator().manual_seed(7100 + Fd)
    h = (torch.randn(M, 2 * Fd, generator=g) * 2.5).to(xdt)
    return (h,) + _geglu_ref(h, Fd)


def geglu_long(Fd, ldo, M, xdt, odt):
    assert M * (ldo // 8) > STREAM_PASS
    h, ref, T = _geglu_long_data(Fd, M, xdt)
    return NS(kind="geglu", h=h, F=Fd, odt=odt, pad=ldo - Fd, ref=ref, tol=_half_ulp(ref, odt) + T,
              second_trip=-(-STREAM_PASS // (ldo // 8)))         # the first row that the first trip does not reach


# C = 32, G = 8, S = 4096 (the workload's), ldo = 40 (5 chunks a row, one of them pad): one trip covers 419430.4 rows, so the second
# trip starts inside row 419430 of sample 102 and crosses into sample 103 at row 421888; B = 104 samples are 2,129,920 chunks.
# (ldo = 32 would start the second trip on row 524288 = 128 * 4096, a sample boundary.)
GN_LONG = [(32, 8, 4096, 104, 8, xdt, odt, silu) for xdt in (F32, F16) for silu in (True, False) for odt in (F16, BF16)]


@functools.lru_cache(maxsize=2)
def _gn_long_data(C, G, S, B, xdt, silu):
    g = torch.Generator().manual_seed(7200 + C)
    # per-sample offsets and spreads: a chunk given the affine of its neighbour sample misses the bound
    x = (torch.randn(B, S, C, generator=g) * (0.3 + 2 * torch.rand(B, 1, C, generator=g)) + 2 * torch.randn(B, 1, C, generator=g)).to(xdt)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return (x, gamma, beta) + _gn_ref(x, G, gamma, beta, EPS, silu)


def gn_long(C, G, S, B, pad, xdt, odt, silu):
    nout = (C + pad) // 8
    assert B * S * nout > STREAM_PASS and STREAM_PASS % (S * nout) != 0 and (STREAM_PASS // (S * nout) + 1) * S * nout < B * S * nout
    x, gamma, beta, ref, T = _gn_long_data(C, G, S, B, xdt, silu)
    return NS(kind="gn", x=x, G=G, gamma=gamma, beta=beta, eps=EPS, silu=silu, odt=odt, pad=pad, ref=ref, tol=_half_ulp(ref, odt) + T,
              second_trip=-(-STREAM_PASS // nout))


ATTN_TILE = 32                          # keys per tile of qd_attn_h16
ATTN_LONG = [(d, op, pat) for d in (40, 160) for op in (F16, BF16) for pat in ("random", "first_tile", "increasing")]


def attn_long(d, op, pattern):
    """S = 4096 keys (128 tiles), T = 33 (one block and a one-row tail), B = 1, H = 2, rows layout [B, N, H * d].
    first_tile: key 5 carries every row's maximum, so no tile after the first rescales; increasing: every tile raises every row's
    maximum, so every tile rescales.  Both premises are asserted here on the operand-rounded scores."""
    B, T, S, H = 1, 33, 4096, 2
    g = torch.Generator().manual_seed(7300 + d)
    u = torch.nn.functional.normalize(torch.randn(H, d, generator=g), dim=-1)
    q = torch.randn(B, T, H, d, generator=g)
    k, v = torch.randn(B, S, H, d, generator=g), torch.randn(B, S, H, d, generator=g)
    if pattern != "random":
        q = 0.5 * q + 3 * u
    if pattern == "first_tile":
        k[:, 5] = 4 * d ** 0.5 * u
    elif pattern == "increasing":
        k = (8 * d ** 0.5 * torch.arange(S).view(1, S, 1, 1) / S) * u
    q, k, v = (t.reshape(B, -1, H * d).contiguous() for t in (q, k, v))
    st = lambda n: (n * H * d, H * d, d, 1)
    scale = d ** -0.5
    if pattern != "random":
        sc = torch.einsum("bthd,bshd->bhts", q.view(B, T, H, d).to(op).double(), k.view(B, S, H, d).to(op).double())
        tmax = sc.view(B, H, T, S // ATTN_TILE, ATTN_TILE).amax(-1)
        if pattern == "first_tile":
            assert (sc.argmax(-1) == 5).all() and (tmax[..., 1:] < tmax[..., :1]).all()
        else:
            assert (tmax[..., 1:] > tmax[..., :-1]).all()
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, st(T), st(S), st(S), scale, op)
    return NS(kind="attn", q=q, k=k, v=v, B=B, T=T, S=S, H=H, d=d, qs=st(T), ks=st(S), vs=st(S), scale=scale, op=op,
              ref=ref, a=a, eps=eps, vmax=vmax)


CONV_LONG = [(wbits, act, split, mode) for wbits, act in ((4, F16), (8, BF16), (4, BF16), (8, F16)) for split in (0, 1280)
             for mode in ("random", "no_cancel")]


def conv_long(wbits, act, split, mode):
    """K = 9 * 2560 = 23040 (SD's deepest up-block contraction), 3 x 3, B = 1, 4 x 4 image, Cout = 40, fp32 output.
    no_cancel: activations >= 0, every code n_levels - 1, zero point 0, so the sum of absolute products S is |ref|."""
    B, Cin, Cout, H, W, k = 1, 2560, 40, 4, 4, 3
    g = torch.Generator().manual_seed(7400 + wbits)
    bounds = [(0, Cin)] if not split else [(0, split), (split, Cin)]
    L = 2 ** wbits
    if mode == "random":
        x, w = torch.randn(B, Cin, H, W, generator=g), torch.randn(Cout, Cin, k, k, generator=g) * 0.1
        qs = [_wquant(w[:, a:b], wbits, "range", g) for a, b in bounds]
    else:
        x = torch.rand(B, Cin, H, W, generator=g) + 0.25
        qs = [NS(delta=0.002 + 0.01 * torch.rand(Cout, generator=g), zero_point=torch.zeros(Cout), n_bits=wbits, n_levels=L, sym=False,
                 alpha=None, soft_targets=False) for _ in bounds]
        w = torch.cat([((L - 1) * q.delta).view(-1, 1, 1, 1).expand(Cout, b - a, k, k) for (a, b), q in zip(bounds, qs)], 1).contiguous()
    ref, tol, wq = _contraction_ref("conv2d", x, w, qs, bounds, None, None, act, F32, 1, 1)
    if mode == "no_cancel":
        assert (ref > 0).all() and (wq > 0).all()
    return NS(kind="conv", x=x, w=w, qs=qs, wq=wq, wbits=wbits, act=act, split=split, shape=(B, Cin, Cout, H, W, k), ref=ref, tol=tol)


# ---- B. value edges ------------------------------------------------------------------------------------------------------------
def _bits16(dt):
    """Every 16-bit pattern of dt, in order."""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)


def rounding_inputs(odt, xdt):
    """The input vector of the cast test as `xdt`.  A 16-bit xdt: every bit pattern of it (fp16 -> bf16 rounds 11 bits to 8 and has
    ties; bf16 -> fp16 overflows, underflows and has ties in the subnormal range).  fp32: every finite value of odt, the midpoint
    of every adjacent pair (exact in fp32) and its two fp32 neighbours, both signs, values that round into the subnormal range of
    fp16, the last value below the overflow threshold and the threshold, +-inf and NaN.  -> (x, ties), ties = the midpoints."""
    if xdt != F32:
        return _bits16(xdt), None
    allv = _bits16(odt)
    fin = allv[torch.isfinite(allv)].float()
    pos = torch.cat([torch.zeros(1), fin[fin > 0].sort()[0]])        # +0 .. max, adjacent in odt
    top = torch.tensor([2.0 ** 16 if odt == F16 else float.fromhex("0x1p+127") * 2], dtype=torch.float64)
    ties = ((torch.cat([pos.double(), top])[1:] + pos.double()) / 2)   # the last one: max | the overflow threshold
    assert (ties.float().double() == ties).all()                     # exactly representable in fp32
    ties = ties.float()
    inf = torch.tensor(math.inf)
    near = torch.cat([ties, torch.nextafter(ties, inf), torch.nextafter(ties, -inf)])
    extra = torch.tensor([0.0, -0.0, 2.0 ** -25, 2.0 ** -26, 1e-8, 3e-8, 5.9e-8, 6e-8, 6.1e-5, 1.1754944e-38, 1e-40, 1e-45, 65519.996, 65520.0,
                          65536.0, 1e5, 3.4028235e38, math.inf, math.nan], dtype=F32)
    x = torch.cat([fin, near, -near, extra, -extra])
    return x, torch.cat([ties, -ties])


ROUNDING = [(xdt, odt, nchw) for odt in (F16, BF16) for xdt in (F32, F16, BF16) for nchw in (True, False)]
ROWS_SEG = NS(C=24, c0=3, clen=13, clen_pad=16, oc0=8, ldo=32)       # c0 != 0, clen < clen_pad, columns outside the segment


def rounding_case(xdt, odt, nchw):
    """The values laid out as channels [c0, c0 + clen) of a logical [1][C][S] tensor with NCHW strides (the kernel's threads
    run along S) or channels-last strides (along the channel groups); expected: the CPU cast, bit for bit."""
    vals, ties = rounding_inputs(odt, xdt)
    sg = ROWS_SEG
    S = -(-vals.numel() // sg.clen)
    seg = torch.zeros(S * sg.clen, dtype=xdt)
    seg[:vals.numel()] = vals
    x = torch.full((S, sg.C), 2.5, dtype=xdt)                        # [S][C]: channels-last storage
    x[:, sg.c0:sg.c0 + sg.clen] = seg.view(S, sg.clen)
    strides = (S * sg.C, 1, sg.C)
    if nchw:
        x, strides = x.t().contiguous(), (S * sg.C, S, 1)            # [C][S] storage
    return NS(kind="rows", x=x, strides=strides, S=S, odt=odt, want=seg.view(S, sg.clen).to(odt), src=seg.view(S, sg.clen), ties=ties)


def geglu_grid():
    """(values, gates) of the GEGLU grid, fp32, every pair: 11 values x 52 gates."""
    b = torch.tensor([0.927734375], dtype=F32)                       # qd_erff's branch point (in erf's argument)
    mags = torch.cat([b, torch.nextafter(b, b + 1), torch.nextafter(b, b - 1),
                      torch.tensor([3, 5, 5.5, 6, 8.5, 12, 40, 300, 1e4], dtype=F32)])
    gates = torch.cat([torch.tensor([0.0, -0.0]), mags, -mags])
    gates = torch.cat([gates, gates * torch.tensor(math.sqrt(2.0), dtype=F32)])
    v = torch.tensor([1e-6, 1e-3, 1, 255, 6e4], dtype=F32)
    values = torch.cat([torch.zeros(1), v, -v])
    vv, gg = torch.meshgrid(values, gates, indexing="ij")
    return vv.reshape(-1), gg.reshape(-1)


GEGLU_EDGES = [(xdt, odt) for xdt in (F32, F16) for odt in (F16, BF16)]


def geglu_edges(xdt, odt):
    """The grid tiled over F = 64 and M = 11 (ragged: the grid wraps round in the last rows), pad 8."""
    Fd, M = 64, 11
    vv, gg = geglu_grid()
    idx = torch.arange(M * Fd) % vv.numel()
    h = torch.cat([vv[idx].view(M, Fd), gg[idx].view(M, Fd)], 1).to(xdt)
    ref, T = _geglu_ref(h, Fd)
    return NS(kind="geglu", h=h, F=Fd, odt=odt, pad=8, ref=ref, tol=_half_ulp(ref, odt) + T)


EPI_EDGES = [(wbits, act, mode) for wbits, act in ((4, F16), (8, BF16), (8, F16), (4, BF16))
             for mode in ("grid", "sub", "normal", "over")]
EPI_DSCALE = {"sub": 2.0 ** -8, "normal": 1.0, "over": 2.0 ** 8}


def epi_edges(wbits, act, mode):
    """The GEGLU projection for the QD_EPI_GEGLU_H16 epilogue.  grid: all-zero activation rows, so the accumulator is 0 and
    value = bias[f], gate = bias[F + f] exactly: the grid in F = 576 features, M = 130 rows (two row tiles).  sub / normal / over:
    random activations with delta (and weights and bias) times 2^-8 / 1 / 2^8: y ~ a g lands in fp16's subnormal range, its normal
    range and past 65504."""
    if mode == "grid":
        vv, gg = geglu_grid()
        Fd, K, M = 576, 64, 130
        assert vv.numel() <= Fd
        bias = torch.zeros(2 * Fd)
        bias[:vv.numel()], bias[Fd:Fd + gg.numel()] = vv, gg
        s = _epi_host(7500, wbits, act, Fd, K, M, 8, x=torch.zeros(M, K), bias=bias)
    else:
        s = _epi_host(7501, wbits, act, 96, 200, 77, 8, dscale=EPI_DSCALE[mode])
    s.kind, s.odt = "epi", act
    s.ref, s.tol, s.h = _epi_ref(s)
    s.wq32 = (_codes(s.w, s.q) - s.q.zero_point.view(-1, 1)) * s.q.delta.view(-1, 1)      # the fp32 weight of a library evaluation
    return s


LN_EDGE_KINDS = ["zero", "const3", "const-1024", "spread1e-4", "mean1e3", "mean1e4", "onehot1e4", "alt65504", "ordinary"]
LN_EDGES = [(C, xdt, odt) for C in (40, 320, 1280) for xdt, odt in ((F32, F16), (F16, BF16), (F32, BF16), (F16, F16))]


def ln_edges(C, xdt, odt):
    """M = 31 rows cycling through LN_EDGE_KINDS, so the two rows of one wave differ in kind; every value fits fp16.
    -> the case, with .kinds the kind index of each row."""
    M = 31
    g = torch.Generator().manual_seed(7600 + C)
    x = torch.zeros(M, C)
    kinds = torch.arange(M) % len(LN_EDGE_KINDS)
    for r in range(M):
        kd = LN_EDGE_KINDS[kinds[r]]
        n = torch.randn(C, generator=g)
        if kd == "const3":
            x[r] = 3
        elif kd == "const-1024":
            x[r] = -1024
        elif kd == "spread1e-4":
            x[r] = 0.5 + 1e-4 * n
        elif kd == "mean1e3":
            x[r] = 1e3 + n
        elif kd == "mean1e4":
            x[r] = 1e4 + n
        elif kd == "onehot1e4":
            x[r, r % C] = 1e4
        elif kd == "alt65504":
            x[r] = 65504.0 * (1 - 2 * (torch.arange(C) % 2))
        elif kd == "ordinary":
            x[r] = 2 * n + 0.3
    x = x.to(xdt)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    ref, T = _ln_ref(x, gamma, beta, EPS)
    return NS(kind="ln", x=x, gamma=gamma, beta=beta, eps=EPS, odt=odt, pad=8, ref=ref, tol=_half_ulp(ref, odt) + T, kinds=kinds)


GN_EDGE_KINDS = ["const_sample", "offset_means", "outlier", "S1", "silu_tail"]
GN_EDGES = [(kd, xdt, odt, silu) for kd in GN_EDGE_KINDS for (xdt, odt) in ((F32, F16), (F16, BF16)) for silu in (True, False)]


def gn_edges(kd, xdt, odt, silu):
    """const_sample: sample 0 constant in every group next to an ordinary sample 1; offset_means: group means 1e2 and 1e3, unit
    spread; outlier: one element of 1e4 in one group; S1: one position; silu_tail: beta = -100 with a small gamma on some
    channels, pre-activations below -90 (under SiLU expf overflows: -0 or a tiny negative)."""
    C, G = 64, 8
    B, S = (3, 1) if kd == "S1" else (2, 67)
    g = torch.Generator().manual_seed(7700 + GN_EDGE_KINDS.index(kd))
    x = torch.randn(B, S, C, generator=g) * (0.3 + 2 * torch.rand(1, 1, C, generator=g)) + 0.5 * torch.randn(1, 1, C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    grp = torch.arange(C) // (C // G)
    if kd == "const_sample":
        x[0] = torch.tensor([0.0, 3.0, -1024.0, 0.5, -7.25, 100.0, 1e-3, -0.0])[grp]
    elif kd == "offset_means":
        x = x + torch.tensor([1e2, 1e3, -1e2, -1e3, 0, 1e3, 1e2, 0])[grp]
    elif kd == "outlier":
        x[1, 13, 20] = 1e4
    elif kd == "silu_tail":
        beta[::3], gamma[::3] = -100.0, 0.5
    x = x.to(xdt)
    ref, T = _gn_ref(x, G, gamma, beta, EPS, silu)
    if kd == "silu_tail":
        assert (_gn_ref(x, G, gamma, beta, EPS, False)[0][:, ::3] < -90).all()
    return NS(kind="gn", x=x, G=G, gamma=gamma, beta=beta, eps=EPS, silu=silu, odt=odt, pad=8, ref=ref, tol=_half_ulp(ref, odt) + T)


def _id(p):
    return "-".join(name(v) if isinstance(v, torch.dtype) else str(v) for v in p)


# every case of every builder: (id, builder, parameters)
ALL = [(f"{fn.__name__}-{_id(p)}", fn, p) for fn, ps in (
    (ln_long, LN_LONG), (geglu_long, GEGLU_LONG), (gn_long, GN_LONG), (attn_long, ATTN_LONG), (conv_long, CONV_LONG),
    (rounding_case, ROUNDING), (geglu_edges, GEGLU_EDGES), (epi_edges, EPI_EDGES), (ln_edges, LN_EDGES), (gn_edges, GN_EDGES)) for p in ps]
