"""The linear epilogues of qd_conv2d_i8 (GPU): the full-tile body against the generic body and the CPU oracle.

Cases, shapes and comparisons: linear_epilogue_cases.py.  Every launch's block form is asserted through qd_conv2d_i8_form, so a
case cannot silently run another kernel."""
import pytest
import torch
import torch.nn.functional as F

import linear_epilogue_cases as L
import conv_tall_tile_cases as T
from oracle import quant_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", L.CASES, ids=[c.name for c in L.CASES])
def test_full_tile_body_equals_generic_body_and_oracle(cuda, c):
    """Rows (and GroupNorm partials) of the default launch equal those of the launch forced through the generic body bit for bit, in
    the four-wave block and in the two-K-group block; the fp32 rows lie within the oracle's bound; fp16 rows are the fp32 rows
    rounded once."""
    t = L.build(cuda, c)
    first = None
    for kg in c.kgs:
        full, fpart, form = L.run(t, c, kg, generic=False)
        gen, gpart, gform = L.run(t, c, kg, generic=True)
        assert form == gform
        if c.k == 3 and c.dt == L.F32:
            assert form[2] == (512 if kg else 256), form                 # nine K-steps: two K-groups unless switched off
        if c.k == 1:
            assert form[2] == 256, form
        assert full.dtype == c.dt and torch.isfinite(full.float()).all() and full.float().abs().max() > 0
        assert torch.equal(full, gen), f"{(full != gen).any(1).sum().item()} rows differ between the two bodies"
        if c.gn:
            assert torch.equal(fpart, gpart)
        if first is None:
            first = (full.clone(), None if fpart is None else fpart.clone())
        else:
            assert torch.equal(full, first[0]) and (not c.gn or torch.equal(fpart, first[1]))
    full32 = first[0]
    if c.dt != L.F32:
        full32, part32, _ = L.run(t, c, c.kgs[0], generic=False, dt=L.F32)
        assert torch.equal(first[0], full32.half())
        if c.gn:
            assert torch.equal(first[1], part32)                          # the statistics are those of the fp32 values
    assert L.matches_oracle(t, c, full32)
    if c.period:
        P = c.period
        assert not torch.equal(full32[P:2 * P], full32[:P])               # other rows, the same residual rows ...
        shifted = (full32[P:2 * P] - t.residual[:P] + t.residual[:P].roll(1, 0))
        assert not torch.equal(full32[P:2 * P], shifted)                  # ... and which residual row matters


@pytest.mark.parametrize("N,k,wbits", [(320, 1, 4), (320, 3, 4), (300, 3, 4), (320, 1, 8), (300, 3, 8)])
def test_exact_accumulators_through_both_bodies(cuda, N, k, wbits):
    """qd_conv2d_i8_acc (int32 rows of the zero-point-restored accumulators): exactly the integer oracle's, from either body."""
    from qdiff import engine, hip
    c = L.case(f"acc_n{N}_k{k}_w{wbits}", N, k, wbits)
    t = L.build(cuda, c)
    want = L.exact_accumulators(t, c)
    try:
        for generic in (False, True):
            hip.conv_config(kgroups=1, generic_epilogue=generic)
            acc = torch.zeros((t.M, N), dtype=torch.int32, device=cuda)
            engine.conv_forward(t.plan, t.xq, c.B, t.H, t.W, acc_out=acc)
            torch.cuda.synchronize()
            assert torch.equal(acc.cpu().long(), want), (generic, (acc.cpu().long() - want).abs().max().item())
    finally:
        hip.conv_config(kgroups=1)


@pytest.mark.parametrize("wbits", [4, 8])
def test_split_k_partials_through_both_bodies(cuda, wbits):
    """Nine K-steps on four blocks: with a workspace offered the library contracts in K slices (int32 partials, then the finalise
    pass).  The rows equal the one-pass launch's and do not depend on the body that wrote the partials."""
    import abi_emulator
    from qdiff import engine, hip
    c = L.case(f"splitk_w{wbits}", 320, 3, wbits, res="full")
    t = L.build(cuda, c)
    one_pass, _, _ = L.run(t, c, 1, generic=False)
    outs = []
    try:
        for generic in (False, True):
            hip.conv_config(kgroups=1, generic_epilogue=generic)
            seen, real = [], hip.conv2d_i8

            def spy(call, acc_out=None):
                form = hip.conv2d_i8_form(call)
                seen.append((form, abi_emulator.conv2d_i8_form(call, kgroups=1, slices=form[3])))
                return real(call, acc_out=acc_out)
            hip.conv2d_i8 = spy
            try:
                outs.append(engine.conv_forward(t.plan, t.xq, c.B, t.H, t.W, residual=t.residual, out_dtype=L.F32))
            finally:
                hip.conv2d_i8 = real
            torch.cuda.synchronize()
            assert len(seen) == 1 and seen[0][0] == seen[0][1] and seen[0][0][3] >= 2, seen
    finally:
        hip.conv_config(kgroups=1)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], one_pass)


@pytest.mark.parametrize("wbits", [4, 8])
def test_two_segments_through_both_bodies(cuda, wbits):
    """The 1 x 1 split shortcut (two activation and two weight quantisers, the first segment's contribution carried in fp32):
    M = 136 rows, Cout = 320, one K-step per segment; both bodies, and the reference's fake-quantised layer.  (The 128 x 128 tile
    of the int8 weights is built with the generic body only for two segments: that case compares trivially equal.)"""
    from qdiff import engine, hip
    g = torch.Generator().manual_seed(17 + wbits)
    B, C, H, W, Cout, split = 1, 128, 8, 17, 320, 64
    x = F.silu(torch.randn(B, C, H, W, generator=g))
    x[:, split:] *= 3.0
    w = torch.randn(Cout, C, 1, 1, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g)

    def wq(ws):
        delta, zp = R.uaq_init_scale(ws, wbits, False, True, "max")
        return T.NS(delta=delta, zero_point=zp, n_bits=wbits, sym=False, n_levels=2 ** wbits, alpha=torch.rand(ws.shape, generator=g) - 0.5,
                    soft_targets=False)
    q0, q1 = wq(w[:, :split]), wq(w[:, split:])
    aqs = []
    for xs in (x[:, :split], x[:, split:]):
        d, z = R.uaq_init_scale(xs, 8, False, False, "max")
        aqs.append(T.NS(delta=torch.tensor(float(d)), zero_point=z, n_bits=8, sym=False))
    plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q0, q1], split), aqs, 1, 1, 1, 0, bias.to(cuda))
    xq = engine.quantize_rows(x.to(cuda), plan, B, C, H * W, (C * H * W, H * W, 1))
    res = torch.randn(B * H * W, Cout, generator=g)
    outs = []
    try:
        for generic in (False, True):
            hip.conv_config(kgroups=1, generic_epilogue=generic)
            with T.launch_forms() as forms:
                outs.append(engine.conv_forward(plan, xq, B, H, W, residual=res.to(cuda), out_dtype=L.F32, splitk=False))
            T.one_form(forms, 128, 160 if wbits == 4 else 128, 256)
            torch.cuda.synchronize()
    finally:
        hip.conv_config(kgroups=1)
    assert torch.equal(outs[0], outs[1])
    want = R.quant_module_forward(x, w, bias, "conv2d", dict(stride=1, padding=0),
                                  [dict(delta=q.delta, zero_point=q.zero_point, alpha=q.alpha, n_levels=q.n_levels) for q in (q0, q1)],
                                  [dict(delta=a.delta, zero_point=a.zero_point, n_bits=8, sym=False) for a in aqs], split=split)
    want = want[0].permute(1, 2, 0).reshape(H * W, Cout) + res
    assert T.within_oracle_bound(outs[0].cpu(), want)


def test_the_switch_is_a_bit_field_and_resets(cuda):
    """qd_conv_config(0 / 1) restores the default epilogue choice (what every fixture of the suite relies on), and the forms do not
    depend on the epilogue bit."""
    from qdiff import hip
    c = L.case("switch", 320, 3, 4)
    t = L.build(cuda, c)
    a, _, fa = L.run(t, c, 1, generic=True)
    b, _, fb = L.run(t, c, 1, generic=False)
    assert fa == fb and torch.equal(a, b)
    with pytest.raises(ValueError):
        hip.conv_config(generic_epilogue=True)
