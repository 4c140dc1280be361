"""The fp16 / bf16 weights-only kernels on the GPU at the cases of tests/wonly_edge_cases.py: the launch forms that only the
benchmark's shapes reach (second trips of the grid-stride loops, 128 key tiles, K = 23040) and the value edges (rounding ties,
subnormal and over-range results, degenerate statistics, qd_erff's branch point and tails).  Every assertion is against the
case's fp64 reference with the tolerance of the random-draw files, against the CPU cast, or bit equality between two forms;
tests/test_weight_only_edges_host.py shows on the CPU that the library's fp32 op + cast meets every one of these bounds.

Worst error / bound per kernel, measured on an MI355X (every test prints its figure as an "[edges] ..." line under -s; in
brackets the library's fp32 op + cast on the same cases and the same device, where the test measures it):
  qd_rows_to_h16      0 of 254k / 261k (fp32 input to fp16 / bf16) and of 65536 (16-bit input) values differ from the CPU cast, all 12 type / order pairs
  qd_layernorm_h16    second trip 0.996 (0.996), degenerate rows 0.987 (0.987)
  qd_geglu_h16        second trip 1.000 (1.000), grid 1.000 (1.000): the output rounding at a result next to a tie, fp16 -> fp16
  qd_groupnorm_h16    second trip 0.995 (0.995), degenerate groups 0.994 (0.994)
  QD_EPI_GEGLU_H16    grid 0.992, subnormal range 0.986, normal range 0.972, past 65504 0.975; 0 elements differ from the two-launch
                      form in all 16 cases (fp16: 8320 subnormal and 6500 infinite results on the grid, 6607 subnormal in `sub`,
                      2573 infinite in `over`)
  qd_attn_h16         S = 4096: random 0.045, maximum in the first tile 0.019, a rescale in every tile 0.049 (all bf16 operands)
  qd_conv2d_wq_h16    K = 23040: random operands 0.0005 or less, no cancellation 0.005 (W4 fp16, unsplit)
"""
import pytest
import torch

import wonly_edge_cases as E
from test_weight_only_attention_gpu import _check as _attn_check, _run as _attn_run, attn_knob  # noqa: F401  (fixture)
from test_weight_only_fused_gpu import (_check_rows, _geglu_launch, _geglu_lib, _gn_launch, _gn_lib, _guarded, _ln_launch, _ln_lib)
from test_weight_only_gpu import _run_case
from test_weight_only_wide_gpu import _epi_launch, _epi_setup, _guards_ok

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _pid(p):
    return E._id(p)


def _produce(dev, c):
    """Case c through its producer kernel and through the library on the same device -> (buffer, rows, C, library rows on the CPU)."""
    if c.kind == "ln":
        buf, out = _ln_launch(dev, c.x, c.gamma, c.beta, c.eps, c.odt, c.pad)
        return buf, out, c.x.shape[1], _ln_lib(c.x.to(dev), c.gamma, c.beta, c.eps, c.odt).cpu()
    if c.kind == "geglu":
        buf, out = _geglu_launch(dev, c.h, c.F, c.odt, c.pad)
        return buf, out, c.F, _geglu_lib(c.h.to(dev), c.F, c.odt).cpu()
    buf, out = _gn_launch(dev, c.x, c.G, c.gamma, c.beta, c.eps, c.silu, c.odt, c.pad)
    return buf, out, c.x.shape[2], _gn_lib(c.x.to(dev), c.G, c.gamma, c.beta, c.eps, c.silu, c.odt).cpu()


# ---- A. launch forms that only the benchmark reaches -------------------------------------------------------------------------
def _long(dev, c, what):
    """Random values in a launch longer than one trip of the kernel's loop: guards, pad columns, the bound, the library
    cross-check.  (tests/test_weight_only_edges_host.py::test_second_trip_rows_bite: every row of the later trips misses the
    bound if it is left unwritten.)"""
    buf, out, C, lib = _produce(dev, c)
    worst = _check_rows(buf, out, C, c.ref, c.tol, what)
    worst_lib = ((lib.double() - c.ref).abs() / c.tol).max().item()
    print(f"\n[edges] {what}: kernel {worst:.3f} x bound, library fp32 + cast {worst_lib:.3f} x bound")
    assert c.ref.shape[0] > c.second_trip
    assert worst <= 1.0 and worst <= 2 * worst_lib


@pytest.mark.parametrize("p", E.LN_LONG, ids=_pid)
def test_layernorm_second_trip(cuda, p):
    """M = 32768 + 3 rows (launch_ln_h16: 4096 blocks x 4 waves x 2 rows a trip): the second trip ends in a row pair of one real
    and one clamped row; the guard rows behind M show that the clamped row is not stored."""
    _long(cuda, E.ln_long(*p), f"layernorm_h16 long {_pid(p)}")


@pytest.mark.parametrize("p", E.GEGLU_LONG, ids=_pid)
def test_geglu_second_trip(cuda, p):
    """M * ldo / 8 just above 2,097,152 chunks (h16_stream_grid: 8192 blocks x 256 threads a trip)."""
    _long(cuda, E.geglu_long(*p), f"geglu_h16 long {_pid(p)}")


@pytest.mark.parametrize("p", E.GN_LONG, ids=_pid)
def test_groupnorm_second_trip(cuda, p):
    """B * S * ldo / 8 just above 2,097,152 chunks (h16_stream_grid), the second trip starting inside one sample and crossing
    into the next."""
    _long(cuda, E.gn_long(*p), f"groupnorm_h16 long {_pid(p)}")


@pytest.mark.parametrize("p", E.ATTN_LONG, ids=_pid)
def test_attention_128_key_tiles(cuda, attn_knob, p):
    """S = 4096: random scores, the maximum in the first tile (no later rescale), scores rising with the key (every tile
    rescales); the bound of the random draws, unchanged."""
    c = E.attn_long(*p)
    out = _attn_run(attn_knob, c.q.to(cuda), c.k.to(cuda), c.v.to(cuda), c.B, c.T, c.S, c.H, c.d, c.qs, c.ks, c.vs, c.scale, c.op, F32)
    ratio = _attn_check(out.cpu(), c.ref, c.a, c.eps, c.vmax, c.S, c.op, F32)
    print(f"\n[edges] attn_h16 S=4096 {_pid(p)}: kernel {ratio:.3f} x bound")


@pytest.mark.parametrize("p", E.CONV_LONG, ids=_pid)
def test_contraction_depth_23040(cuda, p):
    """K = 9 * 2560, unsplit and split at 1280, against K 2^-26 S + 2^-22 |ref| (test_weight_only_gpu.py's bound, unchanged: the
    library's fp32 convolution stays below 0.01 of it at this depth)."""
    wbits, act, split, mode = p
    c = E.conv_long(*p)
    B, Cin, Cout, H, W, k = c.shape
    for seed in (0, 1):                                      # NCHW and channels-last producers
        worst = _run_case(cuda, "conv2d", wbits, act, F32, split, B, Cin, Cout, H, W, k, 1, False, False, "range", seed, x=c.x, w=c.w, qs=c.qs)
        print(f"\n[edges] conv2d_wq_h16 K=23040 {_pid(p)} seed {seed}: kernel {worst:.3f} x bound")


# ---- B. value edges ------------------------------------------------------------------------------------------------------------
def _rows_launch(dev, c):
    from qdiff import hip
    sg = E.ROWS_SEG
    buf, out = _guarded(c.S, sg.ldo, c.odt, dev)
    hip.rows_to_h16(c.x.to(dev), 1, sg.C, c.S, c.strides, out, sg.ldo, sg.c0, sg.clen, sg.clen_pad, sg.oc0)
    torch.cuda.synchronize()
    assert (buf[:3] == 7.5).all() and (buf[-3:] == 7.5).all(), "rows outside [0, S) were written"
    got = out.cpu()
    assert (got[:, :sg.oc0] == 7.5).all() and (got[:, sg.oc0 + sg.clen_pad:] == 7.5).all(), "columns outside the segment were written"
    assert (got[:, sg.oc0 + sg.clen:sg.oc0 + sg.clen_pad] == 0).all(), "the segment's pad columns are not zero"
    return got[:, sg.oc0:sg.oc0 + sg.clen].contiguous()


@pytest.mark.parametrize("p", E.ROUNDING, ids=_pid)
def test_rows_to_h16_is_the_cpu_cast_bit_for_bit(cuda, p):
    """Every finite value, every tie and its fp32 neighbours, the subnormal range, the overflow threshold, +-inf (NaN: isnan
    only), through both thread orders of rows_h16_kernel and a segment with c0 != 0 and clen < clen_pad."""
    c = E.rounding_case(*p)
    got = _rows_launch(cuda, c)
    nan = torch.isnan(c.want)
    assert torch.equal(torch.isnan(got), nan)
    diff = (got.view(torch.int16) != c.want.view(torch.int16)) & ~nan
    assert not diff.any(), f"{int(diff.sum())} values differ from the cast; first: {c.src[diff][0].item()!r} -> {got[diff][0].item()!r}"


def test_ties_fail_a_truncating_cast(cuda):
    """The tie set bites: the kernel's bf16 bytes differ from the fp32 word's upper half on every tie that rounds up."""
    c = E.rounding_case(F32, BF16, False)
    got = _rows_launch(cuda, c).view(torch.int16).flatten()
    src = c.src.flatten()
    trunc = (src.view(torch.int32) >> 16).to(torch.int16)
    tie = (src.view(torch.int32) & 0xffff) == 0x8000
    up = tie & (((src.view(torch.int32) >> 16) & 1) == 1) & torch.isfinite(src)
    assert int(tie.sum()) >= 2 * 32640 and int(up.sum()) > 30000
    assert (got[up] != trunc[up]).all() and (got[tie & ~up] == trunc[tie & ~up]).all()


def _edge(dev, c, what):
    """A value-edge case of a producer: guards, pad columns, no NaN, the bound inside the output range and the signed infinity
    past it, the library cross-check where the library's own ratio is not zero."""
    buf, out, C, lib = _produce(dev, c)
    _check_rows(buf, out, C, c.ref, c.tol, what)             # guards and pad columns
    got = out[:, :C].cpu()
    worst, worst_lib = E.range_ratio(got, c.ref, c.tol, c.odt), E.range_ratio(lib, c.ref, c.tol, c.odt)
    print(f"\n[edges] {what}: kernel {worst:.3f} x bound, library fp32 + cast {worst_lib:.3f} x bound")
    assert worst <= 1.0 and (worst_lib == 0 or worst <= 2 * worst_lib)
    return got


@pytest.mark.parametrize("p", E.GEGLU_EDGES, ids=_pid)
def test_geglu_h16_on_the_grid(cuda, p):
    """Gates at +-0, qd_erff's branch point and its fp32 neighbours, the cancellation of 1 + erf around -5.5, tails to 1e4 sqrt 2;
    values from 0 to 6e4."""
    _edge(cuda, E.geglu_edges(*p), f"geglu_h16 grid {_pid(p)}")


@pytest.mark.parametrize("p", E.EPI_EDGES, ids=_pid)
def test_geglu_epilogue_on_the_grid_and_across_the_fp16_range(cuda, p):
    """QD_EPI_GEGLU_H16 with the grid injected through the bias (all-zero activation rows) and with random activations whose
    results land in fp16's subnormal range, its normal range and past 65504: the rows equal qd_conv2d_wq_h16 + qd_geglu_h16 bit
    for bit (a conversion fused with the last product would differ exactly at ties and subnormal results) and meet the fp64
    bound of test_weight_only_wide_gpu.py."""
    from qdiff import engine, hip
    c = E.epi_edges(*p)
    s = _epi_setup(cuda, 0, c.q.n_bits, c.act, c.F, c.K, c.M, c.ldo - c.F, host=c)
    h = engine.wonly_forward(s.plan, s.xh, 1, 1, c.M, 1, c.M)
    rbuf, two = _guarded(c.M, c.ldo, c.act, cuda)
    hip.geglu_h16(h, c.M, c.F, 2 * c.F, two, c.ldo)
    buf, out = _epi_launch(s, cuda)
    _guards_ok(buf, out, c.F, f"epilogue {_pid(p)}")
    _guards_ok(rbuf, two, c.F, f"two-launch {_pid(p)}")
    if p[2] == "grid":                                       # the injection is exact: the projection is the bias itself
        assert torch.equal(h.cpu(), c.bias.expand(c.M, 2 * c.F))
    got = out[:, :c.F].cpu()
    worst = E.range_ratio(got, c.ref, c.tol, c.act)
    n = int((out.view(torch.int16) != two.view(torch.int16)).sum().item())
    sub = int(((got != 0) & (got.abs().double() < 2.0 ** -14)).sum()) if c.act == F16 else 0
    print(f"\n[edges] geglu epilogue {_pid(p)}: kernel {worst:.3f} x bound, {n} elements differ from the two-launch form, "
          f"{sub} fp16 subnormal results, {int(torch.isinf(got).sum())} infinite")
    assert n == 0 and worst <= 1.0
    if c.act == F16 and p[2] in ("sub", "over"):             # the case reaches the range it is named after
        assert (sub if p[2] == "sub" else int(torch.isinf(got).sum())) > 100


@pytest.mark.parametrize("p", E.LN_EDGES, ids=_pid)
def test_layernorm_h16_degenerate_rows(cuda, p):
    """Zero, constant, tiny-variance, offset, one-hot and +-65504 rows mixed in one launch; an all-zero row is beta rounded to
    the output type, bit for bit."""
    c = E.ln_edges(*p)
    got = _edge(cuda, c, f"layernorm_h16 edges {_pid(p)}")
    zero = got[c.kinds == E.LN_EDGE_KINDS.index("zero")]
    assert zero.shape[0] >= 3 and torch.isfinite(zero).all()
    assert torch.equal(zero.view(torch.int16), c.beta.to(c.odt).expand_as(zero).contiguous().view(torch.int16))


@pytest.mark.parametrize("p", E.GN_EDGES, ids=_pid)
def test_groupnorm_h16_degenerate_groups(cuda, p):
    """A constant sample next to an ordinary one, offset group means, an outlier, S = 1, and pre-activations below -90."""
    _edge(cuda, E.gn_edges(*p), f"groupnorm_h16 edges {_pid(p)}")
