"""qd_conv2d_i8 on its 256-row tiles (GPU): the tiles the benchmark's hottest layers run (batch 16 at the 64 x 64 level: M = 65536,
N = 320) and the rest of the suite, whose launches stay below 256 blocks of 256 rows, almost never reaches.  What is at stake is
the second 32-row tile of every wave (the `i = 1` half of each `for (i < MT)` loop): its im2col source addresses, row terms and
sample index, M tails that cut it off, the GroupNorm partials summed over both halves and the head-layout stores.

Every launch under test is asserted to be 256 rows by 160 or 128 columns, and every comparison launch 128 rows, by asking the
library (qd_conv2d_i8_form) — so a case means the same in a run of this file alone, in a run of the whole suite (where other
files lower the thresholds of the 128 x 320 tile through the environment) and after a change of the tile policy, which would
fail the assertion instead of silently testing another tile.  Comparisons and shapes: conv_tall_tile_cases.py.

What runs on which tile (F = fp32 rows, H = fp16 rows, each with row bias and a residual of its type):
  256 x 160, int4 (N = 800; N = 160 for two K-groups): F, H; M % 256 = 0, 44, 64, 128, 200; samples of 8, 64, 100, 128, 256 rows;
      asymmetric and symmetric activations; 3 x 3 pad 1, stride 2, upsample2x, 1 x 1; 1, 5, 9 and 18 (ragged) K-steps; concatenation
      slot (F; H through ldo > Cout); res_period (F, H); gn_part alone and with gn_ld > Cout; q and transposed-v head layouts with
      hd_sum; int8 rows of the next Linear with an fp32 / fp16 residual; two K-groups: F with gn_part, q / v head layouts.
  256 x 128, int4 (N = 1024; 1000: ragged last column block, vector stores; 1002: per-element stores): F, H; M % 256 = 0, 64, 128,
      200; samples of 64, 100, 128, 256 rows; asymmetric and symmetric; 3 x 3, stride 2 with 18 ragged K-steps, upsample2x; slot;
      gn_part with gn_ld > Cout; q / v head layouts; int8 rows with a residual; two K-groups: F with gn_part.
  256 x 128, int8 (same widths): F, H; M % 256 = 0, 8, 64, 128, 200; samples of 8, 64, 100, 128, 256 rows; asymmetric and
      symmetric; 3 x 3 and 1 x 1 (one K-step); slot; gn_part; two K-groups: F with gn_part.
Not reachable on 256 rows — the dispatcher builds or chooses these for 128 rows only, so there is nothing to test: exact
accumulators (qd_conv2d_i8_acc), split-K partials, two segments, the GEGLU epilogue, members of a grouped launch, head layouts
with hd_T % 256 != 0, any head layout behind int8 weights; with two K-groups also fp16 rows (four-wave block on these tiles) and
head layouts on 256 x 128; N % 320 == 0 with long K runs the 128 x 320 tile instead.
"""
from types import SimpleNamespace as NS

import pytest
import torch

import conv_tall_tile_cases as T
from oracle import quant_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", T.CASES, ids=[c.name for c in T.CASES])
def test_tall_tile_rows(cuda, c):
    """fp32 / fp16 rows with row bias and residual: bit-equal to the 128-row tile, within the oracle's bound on whole samples,
    and (cases named _acc) the sliced launches' exact accumulators equal the integer oracle's."""
    T.check_case(T.build(cuda, c))


# ------------------------------------------------------------------------------------------------
# teeth: the same comparisons against a deliberately wrong expectation must fail
# ------------------------------------------------------------------------------------------------
def test_comparisons_see_a_neighbouring_samples_row_bias_in_second_half_tiles(cuda):
    """Expectation: rows of the second half of every 256-row tile (m % 256 >= 128) carry the row bias of the NEXT sample — what a
    wrong sample index for the second 32-row tile of a wave would write.  Both comparisons reject it."""
    t = T.build(cuda, T.case("teeth_rowbias", 1024, 125, (8, 8)))
    full, ref = T.check_case(t)
    S, B = t.S, t.c.B
    m = torch.arange(t.M, device=cuda)
    second = (m % 256) >= 128
    b = m // S
    wrong = torch.where(second[:, None], ref - t.rowbias[b] + t.rowbias[(b + 1) % B], ref)
    assert second.any() and not torch.equal(full, wrong)
    assert torch.equal(torch.where(second[:, None], full, wrong), full)           # (the expectation is wrong in those rows only)
    hit = [s for s in range(B) if (s * S) % 256 >= 128][:2]                          # samples that lie in second half-tiles
    assert hit and T.matches_oracle(t, full, samples=hit)
    assert not T.matches_oracle(t, full, samples=hit, rowbias=lambda s: t.rowbias_cpu[(s + 1) % B][None, :])


def test_comparisons_see_a_residual_shifted_by_128_rows(cuda):
    """Expectation: the residual of row m - 128 — what a second half-tile reading the first half's residual rows would add."""
    t = T.build(cuda, T.case("teeth_residual", 800, 52, (16, 16)))
    full, ref = T.check_case(t)
    shifted = t.residual.roll(128, 0)
    wrong = ref - t.residual + shifted
    assert not torch.equal(full, wrong)
    samples = T.oracle_samples(t)
    assert not T.matches_oracle(t, full, samples=samples, residual=lambda s: shifted[s * t.S:(s + 1) * t.S].cpu())


# ------------------------------------------------------------------------------------------------
# output forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,hw,wbits", [(800, 205, (8, 8), 4), (1000, 125, (8, 8), 4), (1002, 63, (8, 16), 8)])
def test_tall_tile_writes_a_concatenation_slot(cuda, N, B, hw, wbits):
    """engine.CatSlot: ldo > Cout at a column offset.  Side 1 of a (36 | N) slot and side 0 of an (N | 28) slot: the rows equal the
    plain launch's on the 128-row tile and the guard columns on either side keep their bytes; fp16 rows the same way into a column
    range of a wider buffer (out=: the slot mechanism follows the process-wide stream type)."""
    from qdiff import engine
    t = T.build(cuda, T.case(f"slot_n{N}", N, B, hw, wbits=wbits))
    ref = T.sliced(t)
    for left, right, side in ((36, N, 1), (N, 28, 0)):
        slot = engine.CatSlot(left, right)
        slot.buf = torch.full((t.M, left + right), -7.5, dtype=torch.float32, device=cuda)
        got = T.launch(t, 256, slot=slot.side(side))
        torch.cuda.synchronize()
        assert got.data_ptr() == slot.buf.data_ptr() + (4 * left if side else 0) and got.stride(0) == left + right
        assert torch.equal(got, ref)
        guard = slot.buf[:, :left] if side else slot.buf[:, left:]
        assert bool((guard == -7.5).all())
    ref16 = T.sliced(t, dt=torch.float16)
    wide = torch.full((t.M, 40 + N + 24), -7.5, dtype=torch.float16, device=cuda)
    got = T.launch(t, 256, dt=torch.float16, out=wide[:, 40:40 + N])
    torch.cuda.synchronize()
    assert torch.equal(got, ref16) and bool((wide[:, :40] == -7.5).all()) and bool((wide[:, 40 + N:] == -7.5).all())
    assert T.matches_oracle(t, ref)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_tall_tile_residual_row_period(cuda, dt):
    """qd_conv_desc.res_period on the tall tile: 206 samples of 64 rows, the residual holds the rows of the first 103 (P = 6592, the
    period ends inside tile 25) — against launches on 128-row tiles, sliced across the period, with an ordinary residual."""
    from qdiff import engine
    t = T.build(cuda, T.case("period", 800, 206, (8, 8), dt=dt))
    P = 103 * t.S
    t.residual[P:] = t.residual[:P]
    t.residual_cpu[P:] = t.residual_cpu[:P]
    ref = T.sliced(t, n=3)
    with T.launch_forms() as forms:
        got = engine.conv_forward(t.plan, t.xq, t.c.B, t.H, t.W, rowbias=t.rowbias, residual=t.residual[:P].to(dt), out_dtype=dt,
                                  splitk=False, res_period=P)
    T.one_form(forms, 256, 160)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert not torch.equal(got[P:], (ref[P:].float() - t.residual[:P] + t.residual[:P].roll(1, 0)).to(dt))      # the period matters
    assert T.matches_oracle(t, T.sliced(t, dt=torch.float32, n=3))


# ------------------------------------------------------------------------------------------------
# GroupNorm statistics from the epilogue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,wbits,shared", [(800, 103, 4, False), (1024, 63, 4, True), (1002, 63, 8, False), (800, 104, 4, True)])
def test_tall_tile_emits_groupnorm_statistics(cuda, N, B, wbits, shared):
    """gn_part from a 256-row block: two 128-row chunks, i.e. two samples of 8 x 16 (an odd B leaves the last block one chunk).  The
    rows stay bit-equal to the 128-row tile; the statistics are two waves' 64-row sums per chunk here and four waves' 32-row sums
    there — another fp32 order by design — so they are held, as in test_conv_emits_groupnorm_statistics, against fp64 sums of the
    rows actually written (1e-4 of their range).  shared: gn_ld > Cout, a column range of a wider statistics buffer
    (engine.CatSlot) whose other columns keep their bytes."""
    from qdiff import engine
    t = T.build(cuda, T.case(f"gn_n{N}", N, B, (8, 16), wbits=wbits))
    assert t.S == 128
    ref = T.sliced(t)
    kw = {}
    if shared:
        slot = engine.CatSlot(36, N)
        slot.buf = torch.full((t.M, 36 + N), -7.5, dtype=torch.float32, device=cuda)
        slot.pbuf = torch.full((B, 36 + N, 2), -7.5, dtype=torch.float32, device=cuda)
        kw = dict(slot=slot.side(1))
    got = T.launch(t, 256, gn_stats=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and hasattr(got, "qd_gn_part") and tuple(got.qd_gn_part.shape) == (B, 1, N, 2)
    if shared:
        assert got.qd_gn_part.stride(1) == (36 + N) * 2 and bool((slot.pbuf[:, :36] == -7.5).all()) and bool((slot.buf[:, :36] == -7.5).all())
    part = got.qd_gn_part.cpu().double()
    ch = got.cpu().double().view(B, 1, 128, N)
    want = torch.stack([ch.sum(2), (ch * ch).sum(2)], dim=-1)
    err, rng = (part - want).abs().max().item(), want.abs().max().item()
    print(f"gn_part: max |diff| {err:.3e}, bound {1e-4 * rng:.3e}")
    assert err <= 1e-4 * rng
    # ... and, sharper (that bound is a few units, about one row's worth of a sum): each entry within the worst case of ANY fp32
    # summation order of its 128 terms, gamma_n * sum |term| with n = 129 (127 additions, and a rounded square per term) and unit
    # roundoff 2^-24 — a row missing from a chunk, or counted in the neighbouring one, is tens of thousands of times that
    gamma = 129 * 2.0 ** -24 / (1 - 129 * 2.0 ** -24)
    cap = gamma * torch.stack([ch.abs().sum(2), (ch * ch).sum(2)], dim=-1)
    assert bool(((part - want).abs() <= cap).all()), ((part - want).abs() / cap).max().item()
    # fp16 rows: the statistics are those of the fp32 values, bit for bit (test_conv_fp16_stream_is_the_rounded_fp32_epilogue)
    if not shared:
        got16 = T.launch(t, 256, dt=torch.float16, gn_stats=True)
        torch.cuda.synchronize()
        assert torch.equal(got16, got.half()) and torch.equal(got16.qd_gn_part, got.qd_gn_part)
    assert T.matches_oracle(t, got)


@pytest.mark.parametrize("N,B,wbits", [(1024, 32, 4), (1024, 32, 8), (160, 256, 4)])
def test_tall_tile_with_two_k_groups(cuda, N, B, wbits):
    """A launch of exactly 256 blocks of 256 rows (B samples of 16 x 16, nine K-steps) still takes the tall tile AND has at most
    one block per CU: igemm_k2_kernel<2,4,4,1>, <2,4,4,1,8> and <2,5,4,1>, 512 threads.  Rows and GroupNorm statistics (two chunks per
    sample) equal the four-wave block's on the same tile bit for bit (integer adds commute), the rows those of the 128-row tile,
    and the oracle's within its bound."""
    from qdiff import hip
    t = T.build(cuda, T.case(f"k2_n{N}_w{wbits}", N, B, (16, 16), wbits=wbits))
    outs = {}
    try:
        for kg in (1, 0):
            hip.conv_config(kgroups=kg)
            outs[kg] = T.launch(t, 256, threads=512 if kg else 256, gn_stats=True)
            torch.cuda.synchronize()
    finally:
        hip.conv_config(kgroups=1)
    ref = T.sliced(t)
    torch.cuda.synchronize()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[1].qd_gn_part, outs[0].qd_gn_part) and torch.equal(outs[1], ref)
    assert tuple(outs[1].qd_gn_part.shape) == (B, 2, N, 2)
    assert T.matches_oracle(t, outs[1])


# ------------------------------------------------------------------------------------------------
# head-layout epilogues
# ------------------------------------------------------------------------------------------------
def _heads_setup(cuda, N, Hh, B, Tk, K=128):
    from qdiff import engine
    g = torch.Generator().manual_seed(31 + N + Tk)
    x = torch.randn(B * Tk, K, generator=g)
    ly = T.layer(cuda, N, K, 1, 4)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    plan = engine.build_conv_plan(ly.pack, [NS(delta=torch.tensor(float(dx)), zero_point=zx, n_bits=8, sym=False)], 1, 1, 1, 0, (ly.bias * 0.1).to(cuda))
    assert engine.heads_fusable(plan, Tk, Hh)
    xq = engine.quantize_rows(x.to(cuda), plan, 1, K, B * Tk, (0, 1, K))
    return plan, xq


@pytest.mark.parametrize("N,Hh,B,K,threads", [(1024, 8, 32, 128, 256), (800, 5, 52, 128, 256), (160, 4, 256, 512, 512)])
def test_tall_tile_head_layout_epilogues(cuda, N, Hh, B, K, threads):
    """engine.project_heads as ONE launch on B samples of T = 256 tokens (hd_T % 256 == 0: a 256-row block stays inside a
    sample): q rows and transposed v with its column sums.  The bytes equal those of B per-sample launches, which run 128-row
    tiles, and the fp32 projection (made on 128-row tiles) followed by qd_quantize_heads, as _heads_epilogue_case checks it.
    N = 160 with 256 samples is exactly 256 blocks and eight K-steps: the two-K-group form of the 256 x 160 head epilogues."""
    from qdiff import engine
    Tk, d = 256, N // Hh
    cols = 160 if N % 160 == 0 else 128
    plan, xq = _heads_setup(cuda, N, Hh, B, Tk, K)
    ys = []
    for b0, b1 in T.slices(B):
        with T.launch_forms() as forms:
            ys.append(engine.conv_forward(plan, xq[b0 * Tk:b1 * Tk], 1, 1, (b1 - b0) * Tk, splitk=False))
        T.one_form(forms, 128, cols)
    y = torch.cat(ys)

    def mk(v):
        dd, zz = R.uaq_init_scale(v, 8, False, False, "max")
        return NS(delta=dd, zero_point=zz, n_bits=8, sym=False)
    yc, pre = y.cpu(), 0.7
    aw = NS(delta=torch.tensor(1.0 / 65535), zero_point=torch.tensor(0.0), n_bits=16, sym=False)
    ap = engine.build_attn_plan(mk(yc * pre), mk(yc * pre), mk(yc), aw, 1.0, pre, cuda)
    Tpad, dpad = engine.pad32(Tk), engine.pad32(d)
    for which in (0, 2):
        shape = (B * Hh, dpad, Tpad) if which == 2 else (B * Hh, Tpad, dpad)
        want, got, per = (torch.zeros(shape, dtype=torch.int8, device=cuda) for _ in range(3))
        ws = torch.zeros((B * Hh, dpad), dtype=torch.int32, device=cuda)
        gs, ps = (torch.full((B * Hh, dpad), 7, dtype=torch.int32, device=cuda) for _ in range(2))      # project_heads zeroes them itself
        engine.heads_from_float(ap, which, y, B, Tk, Hh, d, (Tk * N, N, d, 1), want, ws)
        with T.launch_forms() as forms:
            engine.project_heads(plan, xq, B, Tk, Hh, ap, which, got, gs)
        T.one_form(forms, 256, cols, threads)
        with T.launch_forms() as forms:
            for b in range(B):
                engine.project_heads(plan, xq[b * Tk:(b + 1) * Tk], 1, Tk, Hh, ap, which, per[b * Hh:(b + 1) * Hh], ps[b * Hh:(b + 1) * Hh])
        assert len(forms) == B and all(f[:2] == (128, cols) and f[3] == 1 for f in forms), forms[:2]
        torch.cuda.synchronize()
        assert got.float().abs().max() > 0
        assert torch.equal(got, per), (which, (got != per).float().mean().item())
        assert torch.equal(got, want), (which, (got != want).float().mean().item())
        if which == 2:
            assert torch.equal(gs, ps) and torch.equal(gs, ws)


@pytest.mark.parametrize("N,B", [(800, 52), (1024, 32)])
def test_tall_tile_linear_residual_to_int8_rows(cuda, N, B):
    """engine.linear_to_rows_i8 (QD_EPI_HEADS_I8 with one head as wide as the layer and a residual: the feed-forward output of a
    transformer block written as the next Linear's int8 rows — at the benchmark's 64 x 64 level a 256-row launch) on B samples
    of 256 tokens: the bytes of B per-sample launches on 128-row tiles, and of the fp32 Linear + residual (128-row tiles)
    followed by the quantiser launch, as test_linear_residual_to_int8_rows_matches_unfused checks it; an fp16 residual of the
    same values gives the same bytes."""
    from qdiff import engine
    Tk, cols = 256, 160 if N % 160 == 0 else 128
    plan, xq = _heads_setup(cuda, N, 1, B, Tk)
    g = torch.Generator().manual_seed(N)
    res = torch.randn(B * Tk, N, generator=g).half().float().to(cuda)
    ys = []
    for b0, b1 in T.slices(B):
        with T.launch_forms() as forms:
            ys.append(engine.conv_forward(plan, xq[b0 * Tk:b1 * Tk], 1, 1, (b1 - b0) * Tk, residual=res[b0 * Tk:b1 * Tk], splitk=False))
        T.one_form(forms, 128, cols)
    y = torch.cat(ys)
    dy, zy = R.uaq_init_scale(y.cpu(), 8, False, False, "max")
    nxt = engine.build_conv_plan(T.layer(cuda, 64, N, 1, 4).pack, [NS(delta=torch.tensor(float(dy)), zero_point=zy, n_bits=8, sym=False)], 1, 1, 1, 0, None)
    assert engine.rows_i8_fusable(plan, nxt, Tk)
    want = engine.quantize_rows(y, nxt, 1, N, B * Tk, (0, 1, N))
    for r in (res, res.half()):
        with T.launch_forms() as forms:
            got = engine.linear_to_rows_i8(plan, xq, B, Tk, nxt, residual=r)
        T.one_form(forms, 256, cols)
        with T.launch_forms() as forms:
            per = torch.cat([engine.linear_to_rows_i8(plan, xq[b * Tk:(b + 1) * Tk], 1, Tk, nxt, residual=r[b * Tk:(b + 1) * Tk]) for b in range(B)])
        assert len(forms) == B and all(f[:2] == (128, cols) and f[3] == 1 for f in forms), forms[:2]
        torch.cuda.synchronize()
        assert got.abs().max() > 0 and torch.equal(got, per) and torch.equal(got, want)


def test_head_layouts_of_384_token_samples_stay_on_128_rows(cuda):
    """hd_T % 256 != 0: a 256-row block would straddle two samples, so the launcher must answer 128 rows however many rows there
    are (64 x 384 = 24576 rows of 800 columns: 480 blocks of 256 x 160); the same rows as samples of 256 tokens take the tall tile."""
    from qdiff import engine, hip
    N, Hh = 800, 5
    plan, xq = _heads_setup(cuda, N, Hh, 64, 384)
    aw = NS(delta=torch.tensor(1.0 / 65535), zero_point=torch.tensor(0.0), n_bits=16, sym=False)
    a8 = lambda: NS(delta=torch.tensor(0.05), zero_point=torch.tensor(128.0), n_bits=8, sym=False)
    ap = engine.build_attn_plan(a8(), a8(), a8(), aw, 1.0, 0.7, cuda)
    for Tk, B, rows in ((384, 64, 128), (256, 96, 256)):
        for which in (0, 2):
            shape = (B * Hh, engine.pad32(N // Hh), engine.pad32(Tk)) if which == 2 else (B * Hh, engine.pad32(Tk), engine.pad32(N // Hh))
            out8 = torch.zeros(shape, dtype=torch.int8, device=cuda)
            vs = torch.zeros((B * Hh, engine.pad32(N // Hh)), dtype=torch.int32, device=cuda)
            form = hip.conv2d_i8_form(engine._heads_call(plan, xq, B, Tk, Hh, ap, which, out8, vs))
            assert form[:2] == (rows, 160) and form[3] == 1, (Tk, which, form)
