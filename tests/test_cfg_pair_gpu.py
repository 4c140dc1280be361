"""GPU tests of the classifier-free-guidance pair route.  Every comparison is torch.equal against the SAME launch
fed a materialised duplicate of the half-batch operand: the residual row period of qd_conv2d_i8 (qd_conv_desc.res_period), the
query head period of qd_attn_i8_qp, and whole evaluations with the knob on and off."""
import ctypes
import os
import tempfile
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from golden_util import build_ckpt, build_engine_model, fixture_inputs, load_fixture, quant_params
from oracle import quant_ref as R

pytestmark = pytest.mark.gpu


def _aq(delta, zp, n_bits=8, sym=False):
    return NS(delta=torch.tensor(float(delta)), zero_point=zp, n_bits=n_bits, sym=sym)


def _weight_quantizer(w, n_bits, g):
    delta, zp = R.uaq_init_scale(w, n_bits, False, True, "max")
    return NS(delta=delta, zero_point=zp, n_bits=n_bits, sym=False, n_levels=2 ** n_bits, alpha=torch.rand(w.shape, generator=g) - 0.5,
              soft_targets=False)


def _linear_plan(cuda, K, Cout, g):
    from qdiff import engine
    w = torch.randn(Cout, K, 1, 1, generator=g) * 0.05
    x = F.silu(torch.randn(64, K, generator=g))
    d, z = R.uaq_init_scale(x, 8, False, False, "max")
    return engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, g)], 0), [_aq(d, z)], 1, 1, 1, 0,
                                  torch.randn(Cout, generator=g).to(cuda))


def _period_case(cuda, plan, K, Cout, groups, P, hw, dt, gn, splitk, seed, form=None):
    """Rows of `groups` x P outputs whose residual holds P rows, against the same launch on the duplicated residual.
    form: the (rows, columns) of the block both launches must take, asserted through qd_conv2d_i8_form."""
    from conv_tall_tile_cases import launch_forms
    from qdiff import engine
    g = torch.Generator().manual_seed(seed)
    M = groups * P
    rows = F.silu(torch.randn(M, K, generator=g)).to(cuda)
    xq = engine.quantize_rows(rows, plan, 1, K, M, (0, 1, K))
    res = torch.randn(P, Cout, generator=g).to(cuda).to(dt)
    B = M // hw
    with launch_forms() as forms:
        got = engine.conv_forward(plan, xq, B, 1, hw, residual=res, out_dtype=dt, splitk=splitk, gn_stats=gn, res_period=P)
        want = engine.conv_forward(plan, xq, B, 1, hw, residual=res.repeat(groups, 1), out_dtype=dt, splitk=False, gn_stats=gn)
    assert form is None or [f[:2] for f in forms] == [form, form], forms
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    # the duplicate matters: group 1 against a residual shifted by one row differs
    assert not torch.equal(got[P:2 * P], want[:P] - res + res.roll(1, 0))
    if gn:
        assert got.qd_gn_part is not None and torch.equal(got.qd_gn_part, want.qd_gn_part)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("K", [64, 1024])            # one K-step: the four-wave block; 16 K-steps on <= 256 tiles: two K-groups
@pytest.mark.parametrize("Cout", [160, 320])
def test_residual_row_period(cuda, Cout, K, dt):
    """B = 2 and 3 samples of T = 128 rows with P = 128, with and without the GroupNorm statistics of the epilogue; one launch
    with a split-K workspace offered (the library must not split such a descriptor: same bytes)."""
    g = torch.Generator().manual_seed(100 + Cout + K)
    plan = _linear_plan(cuda, K, Cout, g)
    for groups in (2, 3):
        for gn in (False, True):
            _period_case(cuda, plan, K, Cout, groups, 128, 128, dt, gn, False, 7 * groups + gn)
    _period_case(cuda, plan, K, Cout, 2, 128, 128, dt, False, None, 3)          # splitk=None: hip.conv2d_i8 offers its workspace


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_residual_row_period_straddles_a_tile(cuda, dt):
    """The mapping is per row: 6 samples of 64 rows with P = 192 (the second 128-row tile holds rows of two groups), and
    2 x 16512 rows whose period ends inside a block.  Which block the second launch takes depends on the process: N = 320 with
    K = 64 runs 256 x 160 blocks (130 x 2 of them: block 64 straddles) under the library's default thresholds, and the 128 x 320
    tile of 2 x 2 waves (block 129 straddles) once test_hip_kernels.py has been imported, which lowers that tile's K threshold to
    64 through the environment — so in a run of the whole suite this is NOT the 256-row tile; test_conv_tall_tiles_gpu.py has the
    period on the 256-row tile in either kind of run."""
    g = torch.Generator().manual_seed(5)
    plan = _linear_plan(cuda, 64, 320, g)
    wide = int(os.environ.get("QD_WIDE_MINK", "1280")) <= 64
    _period_case(cuda, plan, 64, 320, 2, 192, 64, dt, False, False, 11, form=(128, 160))           # three row blocks: too few for either
    _period_case(cuda, plan, 64, 320, 2, 16512, 16512, dt, False, False, 12, form=(128, 320) if wide else (256, 160))
    plan = _linear_plan(cuda, 1024, 160, g)
    _period_case(cuda, plan, 1024, 160, 4, 192, 64, dt, False, False, 13, form=(128, 160))


def test_every_other_entry_refuses_a_period(cuda):
    """A non-zero res_period outside qd_conv2d_i8's linear epilogue is an error with a message, before anything is launched."""
    from qdiff import hip
    lib = hip.load()
    x = torch.zeros((128, 64), dtype=torch.int8, device=cuda)
    w = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    out = torch.zeros((128, 64), dtype=torch.float32, device=cuda)
    res = torch.zeros((128, 64), dtype=torch.float32, device=cuda)
    scale = torch.ones(64, device=cuda)
    oq = torch.tensor([0.1, 0.0, 10.0, 0.0], device=cuda)

    def desc(**kw):
        d = hip.ConvDesc()
        d.x, d.w, d.out, d.residual = x.data_ptr(), w.data_ptr(), out.data_ptr(), res.data_ptr()
        d.ldx, d.ldo, d.ldr = 64, 64, 64
        d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = 1, 1, 128, 1, 128, 64
        d.kh = d.kw = d.stride = 1
        d.wbits, d.w_tiled, d.nseg, d.out_dtype, d.res_period = 4, 1, 1, hip.F32, 128
        d.seg[0].clen, d.seg[0].scale = 64, scale.data_ptr()
        d.oq_params, d.oq_min, d.oq_max, d.oq_off = oq.data_ptr(), 0, 255, 128
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(rc):
        msg = lib.qd_last_error().decode()
        assert rc != 0 and "res_period" in msg, (rc, msg)

    st = hip._stream()
    for epi in (hip.EPI_GEGLU_I8, hip.EPI_HEADS_I8, hip.EPI_HEADS_T_I8):
        refused(lib.qd_conv2d_i8(ctypes.byref(desc(epilogue=epi)), st))
    refused(lib.qd_conv2d_i8(ctypes.byref(desc(residual=None)), st))                       # a period without a residual
    refused(lib.qd_conv2d_i8(ctypes.byref(desc(res_period=96)), st))                       # does not divide M / no whole samples
    refused(lib.qd_conv2d_bf16(ctypes.byref(desc(wbits=16)), st))
    refused(lib.qd_conv2d_wq_h16(ctypes.byref(desc()), hip.F16, st))
    d0 = desc(epilogue=hip.EPI_HEADS_I8)
    arr = (ctypes.POINTER(hip.ConvDesc) * 1)(ctypes.pointer(d0))
    refused(lib.qd_conv2d_i8_group(arr, 1, st))
    assert lib.qd_conv2d_i8_splitk_ws_bytes(ctypes.byref(desc())) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                                    # nothing ran


# ------------------------------------------------------------------------------------------------
# query head period
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("mult", [2, 3])
@pytest.mark.parametrize("d,S,T", [(40, 77, 256),        # register-fed lean kernel
                                   (40, 512, 256),       # statistics + P.V launches
                                   (64, 77, 256),        # attn_kernel
                                   (40, 77, 200)])       # ragged T
def test_query_head_period(cuda, d, S, T, mult, quantised):
    """BH = mult x q_heads heads of keys / values on q_heads heads of queries (two samples of two heads) against the same launch
    on the duplicated query operand; fp32 rows and the quantised rows of the consuming Linear."""
    from qdiff import engine
    g = torch.Generator().manual_seed(1000 + d + S + T)
    H, Bq = 2, 2
    B, C = Bq * mult, H * d
    q = torch.randn(Bq, T, C, generator=g)
    k, v = torch.randn(B, S, C, generator=g), torch.randn(B, S, C, generator=g)

    def mk(t, n_bits=8, always_zero=False):
        dd, zz = R.uaq_init_scale(t, n_bits, False, False, "max", always_zero)
        return NS(delta=dd, zero_point=zz, n_bits=n_bits, sym=False)
    heads = lambda t, n, L: t.view(n, L, H, d).permute(0, 2, 1, 3).reshape(n * H, L, d)
    scale = d ** -0.5
    p = (torch.einsum("bid,bjd->bij", heads(q, Bq, T).repeat(mult, 1, 1), heads(k, B, S)) * scale).softmax(-1)
    ap = engine.build_attn_plan(mk(q), mk(k), mk(v), mk(p, 16, True), scale, 1.0, cuda)
    Tp, Sp, dp = engine.pad32(T), engine.pad32(S), engine.pad32(d)
    q8 = torch.zeros((Bq * H, Tp, dp), dtype=torch.int8, device=cuda)
    k8 = torch.zeros((B * H, Sp, dp), dtype=torch.int8, device=cuda)
    v8 = torch.zeros((B * H, dp, Sp), dtype=torch.int8, device=cuda)
    vsum = torch.zeros((B * H, dp), dtype=torch.int32, device=cuda)
    for which, (t, n, L, buf) in enumerate(((q, Bq, T, q8), (k, B, S, k8), (v, B, S, v8))):
        engine.heads_from_float(ap, which, t.to(cuda), n, L, H, d, (L * C, C, d, 1), buf, vsum)
    out_plan = _linear_plan(cuda, C, 64, g) if quantised else None
    if quantised:
        assert out_plan.ldx == C and len(out_plan.segs) == 1
    got = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d, out_plan=out_plan, q_heads=Bq * H)
    want = engine.attention_codes(ap, q8.repeat(mult, 1, 1), k8, v8, vsum, B, T, S, H, d, out_plan=out_plan)
    torch.cuda.synchronize()
    assert got.shape[0] == B * T and torch.equal(got, want)
    assert want.float().abs().max() > 0 and not torch.equal(want[:T], want[Bq * T:(Bq + 1) * T])      # the groups' keys differ


def test_query_head_period_is_checked(cuda):
    from qdiff import engine, hip
    z8 = lambda *s: torch.zeros(s, dtype=torch.int8, device=cuda)
    ap = NS(prm=torch.zeros(16, device=cuda), wbits=8, wmin=0, wmax=255, asym=False)
    for qh in (3, 2, 0):                     # does not divide BH = 8; no multiple of H = 4; not positive
        with pytest.raises(hip.HipEngineError, match="q_heads"):
            engine.attention_codes(ap, z8(8, 32, 32), z8(8, 32, 32), z8(8, 32, 32), torch.zeros((8, 32), dtype=torch.int32, device=cuda),
                                   2, 32, 32, 4, 32, q_heads=qh)


# ------------------------------------------------------------------------------------------------
# whole evaluations
# ------------------------------------------------------------------------------------------------
def _resume(fx, dev):
    import qdiff
    from qdiff.utils import resume_cali_model
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    qnn = qdiff.QuantModel(build_engine_model(spec).to(dev), wq, aq, sm_abit=spec["sm_abit"]).to(dev).eval()
    cal = tuple(a for a in fixture_inputs(fx, "cal") if a is not None)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ckpt.pth")
        torch.save(build_ckpt(fx), path)
        resume_cali_model(qnn, path, cal, quant_act=True, cond=spec["ctx"] is not None)
    qnn.set_quant_state(True, True)
    return qnn


@pytest.fixture
def knob():
    from qdiff import engine
    before = engine.CFG_SHARE
    yield engine.set_cfg_share
    engine.set_cfg_share(before)


@pytest.mark.parametrize("name", ["sd_tiny", "sd_full"])
def test_shared_evaluation_equals_unshared(cuda, name, knob):
    """Batch 2 with both samples equal: the shared evaluation equals the unshared one bit for bit, eager and through graph replay
    with a prepared context, and pair_evals advances; distinct samples without a mark evaluate as always."""
    from qdiff import engine
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    x, t, c = (a.to(cuda) for a in fixture_inputs(fx, "test"))
    x2, t2 = torch.cat([x[:1]] * 2), torch.cat([t[:1]] * 2)
    qnn.enable_hip_graphs(False)
    with torch.no_grad():
        knob(False)
        want = qnn(x2, t2, c).clone()
        want_distinct = qnn(x, t, c).clone()
        assert qnn.pair_evals == 0
        knob(True)
        assert qnn.prepare_context(c)
        engine.mark_pair(x2, t2)
        eager = qnn(x2, t2, c).clone()
        assert qnn.pair_evals == 1
        distinct = qnn(x, t, c).clone()                           # no mark, same context object: no read-back, no sharing
        assert qnn.pair_evals == 1
        qnn.enable_hip_graphs(True)
        g1 = qnn(x2, t2, c).clone()                               # captures the shared evaluation
        g2 = qnn(x2, t2, c).clone()                               # replays it
        assert qnn.pair_evals == 3
        x3 = x2.clone()                                           # a fresh, unmarked pair and a fresh context with the same bytes:
        g3 = qnn(x3, t2.clone(), c.clone()).clone()               # the halves' equality rides in the context's by-value read-back
        assert qnn.pair_evals == 4
        g4 = qnn(x, t, c).clone()                                 # distinct samples: the unshared graph
        assert qnn.pair_evals == 4
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and not torch.equal(want[0], want[1])      # the contexts differ
    for nm, y in (("eager", eager), ("g1", g1), ("g2", g2), ("g3", g3)):
        assert torch.equal(y, want), (nm, (y - want).abs().max().item())
    assert torch.equal(distinct, want_distinct) and torch.equal(g4, want_distinct)


def test_guided_eps_is_the_same_with_the_knob_on_and_off(cuda, knob):
    from qdiff import sampling
    fx = load_fixture("model_sd_tiny.pt")
    qnn = _resume(fx, cuda)
    x, t, c = (a.to(cuda) for a in fixture_inputs(fx, "test"))
    outs = []
    with torch.no_grad():
        for on in (False, True):
            knob(on)
            before = qnn.pair_evals
            outs.append([sampling.guided_eps(qnn, x, t, c, c.flip(0), 7.5).clone() for _ in range(3)])     # eager, capture, replay
            assert qnn.pair_evals - before == (3 if on else 0)
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
