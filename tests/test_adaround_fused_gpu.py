"""GPU tests of the fused AdaRound route of the weight phase of calibration (engine.FUSED_ADAROUND, csrc/adaround.hip,
DESIGN.md §4.20): the kernels against the fp32 torch composition and an fp64 evaluation on the smallest shapes that reach every
path, the value edges of alpha, the autograd plumbing of a QuantModule with its launch budget, and the whole weight phase
against the reference's fixtures.  Cases, units and the comparison are tests/adaround_cases.py's."""
import pytest
import torch
import torch.nn as nn

import adaround_cases as ac

pytestmark = pytest.mark.gpu

# (weight shape, bits, split: None = whole tensor, s > 0 = weight[:, :s], s < 0 = weight[:, -s:]) — why: see the table in DESIGN §4.20
CASES = [((48, 32, 3, 3), 4, None),       # plain
         ((40, 96), 8, None),             # linear
         ((16, 3, 3, 3), 4, None),        # cols = 27: every row start misaligned, weights read float by float
         ((5, 1031), 8, None),            # odd cols longer than one block's span
         ((1, 1, 1, 1), 4, None),         # a single element
         ((32, 48, 3, 3), 4, 16),         # first half of a split shortcut: ldw != cols
         ((32, 48, 3, 3), 4, -16)]        # second half: offset pointer
PLANTED = (0.0, ac.LOG11, -ac.LOG11, 30.0, -30.0)


@pytest.fixture
def knob_off():
    from qdiff import engine
    prev = engine.FUSED_ADAROUND
    engine.set_fused_adaround(False)
    engine.ADAROUND_LAUNCHES[0] = 0
    yield engine
    engine.set_fused_adaround(prev)


def _case(shape, bits, split, dev, seed=3, planted=PLANTED):
    w = ac.weights(shape, seed, dev)
    if split is not None:
        w = w[:, :split] if split > 0 else w[:, -split:]
    return w, ac.make_quantizer(w, bits, seed + 1, planted)


@pytest.mark.parametrize("shape,bits,split", CASES)
def test_kernels_against_the_composition_and_fp64(cuda, knob_off, shape, bits, split):
    """w_hat, galpha and reg_sum of the fused route and of the fp32 torch composition against the fp64 evaluation of the same
    formulas on the same fp32 floor(w / delta): fused worst <= 2 x composition worst per case and unit; torch.equal w_hat and an
    exactly zero gradient where h is saturated; boundary elements (<= 2 %) take one of the legitimate outcomes.  b in
    {20, 7.3, 2} and no regulariser; codes clamp at both ends (asserted)."""
    w, q = _case(shape, bits, split, cuda)
    gw = torch.randn(w.shape, generator=torch.Generator().manual_seed(11)).to(cuda)
    for b in (20, 7.3, 2, None):
        knob_off.ADAROUND_LAUNCHES[0] = 0
        ef, ec, ref = ac.judge(q, w, b, gw, 0.017, label=f"gpu {shape} split={split}")
        assert knob_off.ADAROUND_LAUNCHES[0] == 2                  # one forward, one backward launch; none for the composition
    if w.numel() > 16:
        assert (ref["c"] < 0).any() and (ref["c"] > ref["top"]).any(), "the case does not clamp codes at both ends"
        d = q.delta.flatten()
        assert d.max() / d.min() > 10, "no outlier channel"


def test_value_edges(cuda, knob_off):
    """Planted into alpha: 0 (h = 0.5, v = 0, sgn = 0), +-log 11 (hr on the clamp boundary: what init_alpha gives a weight on
    the grid), +-30 and +-100 (exp overflows, s is exactly 0 or 1); a constant row and a row of zeros in w.  Everything finite,
    galpha exactly 0 and w_hat bit-equal to the composition's where the target is saturated."""
    w = ac.weights((6, 40), 5, cuda)
    w[1] = 0.0
    w[2] = 0.25
    planted = (0.0, ac.LOG11, -ac.LOG11, 30.0, -30.0, 100.0, -100.0)
    q = ac.make_quantizer(w, 4, 6, planted)
    gw = torch.randn(w.shape, generator=torch.Generator().manual_seed(2)).to(cuda)
    for b in (20, 7.3, 2, None):
        c_w, c_reg, c_g = ac.run_route(q, w, b, gw, 0.01, fused=False)
        f_w, f_reg, f_g = ac.run_route(q, w, b, gw, 0.01, fused=True)
        assert torch.isfinite(f_w).all() and torch.isfinite(f_g).all() and (b is None or torch.isfinite(f_reg))
        sat = slice(3, 7)                                          # +-30, +-100
        assert (f_g.reshape(-1)[sat] == 0).all() and torch.equal(f_w.reshape(-1)[sat], c_w.reshape(-1)[sat])
        a = q.alpha.detach().reshape(-1)
        hard = (a.abs() > 5)                                       # every saturated target, wherever it is (|alpha| > log 11 + margin)
        assert hard.sum() >= 4
        assert (f_g.reshape(-1)[hard] == 0).all() and torch.equal(f_w.reshape(-1)[hard], c_w.reshape(-1)[hard])
        ref = ac.reference64(w.cpu(), ac._cpu_view(q), b, gw.cpu(), 0.01)
        ef, ec = ac.errors(ref, f_w, f_reg, f_g), ac.errors(ref, c_w, c_reg, c_g)
        ac.assert_within(ef, ec, f"value edges b={b}")


def _module(split, dev):
    from qdiff.quant_layer import QuantModule
    torch.manual_seed(0)
    conv = nn.Conv2d(12, 8, 3, padding=1).to(dev)
    m = QuantModule(conv, dict(n_bits=4, channel_wise=True, scale_method='max'), dict(n_bits=8, scale_method='max', leaf_param=True))
    x = torch.randn(4, 12, 6, 6, device=dev)
    m.set_quant_state(True, False)
    with torch.no_grad():
        tgt = conv(x)
        m(x, split=split)
    return m, x, tgt


@pytest.mark.parametrize("split,layer_unit", [(0, True), (5, True), (5, False)])
def test_autograd_plumbing_and_launch_budget(cuda, knob_off, split, layer_unit):
    """alpha.grad of QuantModule forward + ReconstructionObjective + backward through the fused route and through the knob-off
    run on the same tensors, inside engine.simulation() as recon.reconstruct runs, within the bound of the kernel test: a hook on
    each quantiser's output captures the upstream gradient, greg is the objective's weight, and both routes are judged per
    element against the fp64 evaluation (fused worst <= 2 x composition worst) — split halves included.
    engine.ADAROUND_LAUNCHES is one forward and one backward launch per soft quantiser and 0 with the knob off;
    weight_quantizer_0 of a split LAYER unit gets no gradient."""
    from qdiff import engine, recon
    m, x, tgt = _module(split, cuda)
    recon.to_adaround(m, layer_unit=layer_unit)
    qs = m._weight_quantizers()
    with torch.no_grad():
        for q in qs:
            q.alpha.mul_(1.5)
    soft = sum(q.soft_targets for q in qs)
    seen = [ac.Upstream(q) for q in qs]
    weight = 0.01

    def run(fused, calls0):
        obj = recon.ReconstructionObjective(m, iters=1000, weight=weight, b_range=(20, 2), warmup=0.2)
        obj.calls = calls0
        for q in qs:
            q.alpha.grad = None
        engine.ADAROUND_LAUNCHES[0] = 0
        engine.set_fused_adaround(fused)
        try:
            with engine.simulation():
                if fused:
                    obj.arm()
                total = obj(m(x, split=split), tgt)
                total.backward()
        finally:
            obj.disarm()
            engine.set_fused_adaround(False)
        b = obj._exponent(obj.calls)
        errs = []
        for i, (q, up) in enumerate(zip(qs, seen)):
            if q.alpha.grad is None:
                errs.append(None)
                continue
            # the objective regularises weight_quantizer only (index 0): the second half of a split has the reconstruction chain alone
            errs.append(up.errors(q, b if i == 0 else None, weight))
        return total.detach(), errs, engine.ADAROUND_LAUNCHES[0]

    for calls0 in (10, 800):                                       # warm-up: no regulariser; annealing: b between 20 and 2
        t_c, e_c, n_c = run(False, calls0)
        t_f, e_f, n_f = run(True, calls0)
        assert n_c == 0 and n_f == 2 * soft
        assert abs(float(t_f) - float(t_c)) <= 4 * 2.0 ** -23 * abs(float(t_c))
        for i, (ef, ec) in enumerate(zip(e_f, e_c)):
            assert (ef is None) == (ec is None)
            if ef is not None:
                print(f"[adaround module split={split} layer_unit={layer_unit} call {calls0 + 1} quantiser {i}] "
                      + ", ".join(f"{k}: fused {ef[k]:.3e} composition {ec[k]:.3e}" for k in ef))
                ac.assert_within(ef, ec, f"quantiser {i} at call {calls0 + 1}")
        assert sum(e is not None for e in e_f) == soft
        if split and layer_unit:
            assert e_f[1] is None and not qs[1].soft_targets
    for up in seen:
        up.handle.remove()


@pytest.mark.parametrize("name", ["cifar_tiny", "sd_tiny"])
def test_whole_weight_phase_against_the_reference_fixture(cuda, knob_off, name):
    """tests/test_calibration.py's GPU bounds against the REFERENCE's fixtures, unchanged, with the knob on: the reachable
    distance, the l2 of alpha, at most 5e-4 differing rounding decisions, out_w within 2e-3."""
    from test_calibration import _calibration_vs_reference_fixture
    knob_off.set_fused_adaround(True)
    _calibration_vs_reference_fixture(name, cuda, on_gpu=True)
    assert knob_off.ADAROUND_LAUNCHES[0] > 0
