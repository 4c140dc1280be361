"""Every case of tests/wonly_edge_cases.py through the library's plain fp32 op followed by .to(dtype), on the CPU, against the
case's own fp64 reference and tolerance: ratio <= 1 and no NaN where the reference is finite.  Each bound therefore admits a
correct fp32 implementation of that case, and a failure of tests/test_weight_only_edges_gpu.py is the kernel's.  The cast cases
have the cast itself as their reference; what is checked for them is the construction (exact ties, the counts, a truncating cast
differs on them)."""
import pytest
import torch
import torch.nn.functional as F

import wonly_edge_cases as E
from test_weight_only_attention_gpu import _check
from test_weight_only_fused_gpu import _geglu_lib, _gn_lib, _ln_lib


def library_result(c):
    """The library's fp32 evaluation of case c, cast to the case's output type, as rows on the CPU."""
    if c.kind == "ln":
        return _ln_lib(c.x, c.gamma, c.beta, c.eps, c.odt)
    if c.kind == "geglu":
        return _geglu_lib(c.h, c.F, c.odt)
    if c.kind == "gn":
        return _gn_lib(c.x, c.G, c.gamma, c.beta, c.eps, c.silu, c.odt)
    if c.kind == "epi":
        h = c.x.to(c.act).float() @ c.wq32.t() + c.bias
        return _geglu_lib(h, c.F, c.odt)
    if c.kind == "conv":
        y = F.conv2d(c.x.to(c.act).float(), c.wq.float(), padding=1)
        return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])
    if c.kind == "attn":
        B, T, S, H, d = c.B, c.T, c.S, c.H, c.d
        q, k, v = (t.to(c.op).float().view(B, -1, H, d).transpose(1, 2) for t in (c.q, c.k, c.v))
        return F.scaled_dot_product_attention(q, k, v, scale=c.scale).transpose(1, 2).reshape(B * T, H * d)
    raise AssertionError(c.kind)


@pytest.mark.parametrize("builder,params", [pytest.param(fn, p, id=i) for i, fn, p in E.ALL if fn is not E.rounding_case])
def test_library_fp32_meets_the_bound(builder, params):
    c = builder(*params)
    lib = library_result(c)
    assert torch.isfinite(c.ref).all()
    if c.kind == "attn":
        ratio = _check(lib, c.ref, c.a, c.eps, c.vmax, c.S, c.op, torch.float32)
    elif c.kind == "conv":                                   # fp32 rows: no rounding to an operand type
        assert torch.isfinite(lib).all()
        ratio = ((lib.double() - c.ref).abs() / c.tol).max().item()
    else:
        ratio = E.range_ratio(lib, c.ref, c.tol, c.odt)
    print(f"\nlibrary fp32 + cast: {ratio:.3f} x bound")
    assert ratio <= 1.0


@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rounding_inputs_are_what_they_claim(odt):
    """The fp32 input set of the cast test: 31743 (fp16) / 32639 (bf16) positive ties between adjacent finite values plus the
    overflow threshold, each exactly halfway in fp64 between its two neighbours of the output type; the CPU cast sends a tie to
    the even neighbour and the tie's fp32 neighbours to either side; a truncating cast differs on the ties."""
    x, ties = E.rounding_inputs(odt, torch.float32)
    pos = ties[ties > 0]
    assert pos.numel() == (31743 if odt == torch.float16 else 32639) + 1
    lo, hi = torch.nextafter(pos, torch.tensor(0.0)).to(odt), torch.nextafter(pos, torch.tensor(float("inf"))).to(odt)
    fin = torch.isfinite(hi)
    assert int((~fin).sum()) == 1                                              # the overflow threshold alone rounds up to inf
    assert (lo.double() < pos.double()).all() and ((lo.double() + hi.double()) / 2 == pos.double())[fin].all()
    cast = pos.to(odt)
    even = (cast.view(torch.int16) & 1) == 0
    assert even.all() and ((cast == lo) | (cast == hi)).all()
    assert (cast == lo).sum() > 10000 and (cast == hi).sum() > 10000           # both directions occur: half of the ties round up
    if odt == torch.bfloat16:
        trunc = (pos.view(torch.int32) >> 16).to(torch.int16)
        assert (trunc != cast.view(torch.int16)).sum() == (cast == hi).sum()
    for xdt in (torch.float32, torch.float16, torch.bfloat16):
        for nchw in (True, False):
            c = E.rounding_case(xdt, odt, nchw)
            sg = E.ROWS_SEG
            xs = torch.as_strided(c.x, (c.S, sg.C), (c.strides[2], c.strides[1]))
            assert torch.equal(xs[:, sg.c0:sg.c0 + sg.clen].view(torch.int16 if xdt != torch.float32 else torch.int32),
                               c.src.view(torch.int16 if xdt != torch.float32 else torch.int32))


# ---- the edge classes bite: a subtly wrong fp32 implementation misses the bound on the case built for it ----------------------
def _ratio(c, got):
    return E.range_ratio(got, c.ref, c.tol, c.odt)


def test_over_range_and_subnormal_results_bite():
    """A store that saturates at 65504 instead of overflowing, and one that flushes fp16 subnormals to zero."""
    c = E.geglu_edges(torch.float32, torch.float16)
    lib = library_result(c)
    assert torch.isinf(lib).sum() >= 40 and _ratio(c, lib) <= 1.0
    with pytest.raises(AssertionError, match="signed infinity"):
        _ratio(c, lib.float().clamp(-65504, 65504).half())
    c = E.epi_edges(4, torch.float16, "sub")
    lib = library_result(c)
    assert _ratio(c, lib) <= 1.0
    assert _ratio(c, torch.where(lib.abs() < 2.0 ** -14, torch.zeros_like(lib), lib)) > 1.0


@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_erf_grid_bites(odt):
    """tanh-GELU, and an erf that is exact on [-6, 6] only (clamped argument: 1 + erf stops at erfc(6) instead of vanishing)."""
    c = E.geglu_edges(torch.float32, odt)
    a, g = c.h[:, :c.F], c.h[:, c.F:]
    assert _ratio(c, (a * F.gelu(g, approximate="tanh")).to(odt)) > 1.0
    shifted = a.double() * 0.5 * g.double() * (1 + torch.erf(g.double() / 2 ** 0.5) + 2.0 ** -21)      # 2 ulp of the bracket's 1
    assert _ratio(c, shifted.float().to(odt)) > 1.0


def test_degenerate_statistics_bite():
    """A one-pass variance E[x^2] - m^2 in fp32 on the offset rows of LayerNorm; batch-wide statistics on GroupNorm's constant
    sample next to an ordinary one."""
    c = E.ln_edges(320, torch.float32, torch.float16)
    x = c.x.float()
    m = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - m * m).clamp(min=0)
    assert _ratio(c, ((x - m) / torch.sqrt(var + c.eps) * c.gamma + c.beta).to(c.odt)) > 1.0
    c = E.gn_edges("const_sample", torch.float32, torch.float16, False)
    B, S, C = c.x.shape
    batchwide = F.group_norm(c.x.reshape(1, B * S, C).permute(0, 2, 1), c.G, c.gamma, c.beta, c.eps).permute(0, 2, 1).reshape(B * S, C)
    assert _ratio(c, batchwide.to(c.odt)) > 1.0


@pytest.mark.parametrize("builder,params", [pytest.param(fn, p, id=i) for i, fn, p in E.ALL if fn in (E.ln_long, E.geglu_long, E.gn_long)])
def test_second_trip_rows_bite(builder, params):
    """A kernel that stops after one trip of its loop leaves the rows from `second_trip` on at the guard value 7.5: every one of
    those rows (the clamped last pair of LayerNorm and the rows behind GroupNorm's sample crossing included) misses the bound on
    its own, in at least nine of ten elements (an element misses unless its reference happens to lie at 7.5)."""
    c = builder(*params)
    assert 0 < c.second_trip < c.ref.shape[0]
    miss = (7.5 - c.ref[c.second_trip:]).abs() / c.tol[c.second_trip:] > 1.0
    assert miss.any(dim=1).all() and miss.double().mean(dim=1).min() >= 0.9
