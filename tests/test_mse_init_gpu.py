"""GPU tests of the fused MSE range search that initialises a quantiser (engine.FUSED_MSE_INIT, csrc/mse_search.hip, DESIGN.md
§4.21): the kernel against the torch composition and an fp64 evaluation of the scores on the smallest shapes that reach every
path — both widths of the row form, rows longer than one chunk, misaligned and strided rows, the spread form with one and with
many blocks of partials — the value edges, and the plumbing through QuantModule and QuantModel.  Cases and the judge are
tests/mse_init_cases.py's."""
import pytest
import torch
import torch.nn as nn

import mse_init_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture
def knob_off():
    from qdiff import engine
    prev = engine.FUSED_MSE_INIT
    engine.set_fused_mse_init(False)
    engine.MSE_INIT_SEARCHES[0] = 0
    yield engine
    engine.set_fused_mse_init(prev)


@pytest.mark.parametrize("name,build,per_row,bits,sym,always_zero", mc.CASES, ids=[c[0] for c in mc.CASES])
def test_kernel_against_the_composition_and_fp64(cuda, knob_off, name, build, per_row, bits, sym, always_zero):
    """Exact outputs at the kernel's own pick and bit-identical runs; score error <= 2 x the composition's (floor 4 ulp); picks
    the composition's on >= 98 % of the groups, a neighbouring tie otherwise; degenerate groups take nothing on both routes."""
    x = build(cuda)
    fig = mc.judge(x, per_row, bits, sym, always_zero, label="gpu " + name)
    assert knob_off.MSE_INIT_SEARCHES[0] == 2                       # the judge's two runs; none for the composition
    if name.startswith("edges") and per_row:
        assert fig["picks"][0] == -1 and len(fig["picks"]) > 1


def test_launch_forms_cover_the_cases(cuda):
    """The one rule (qd_mse_search_form): the case list reaches the wave and the block width of the row form, and the spread
    form with a single block and with the 2048-block cap's neighbourhood of many blocks."""
    from qdiff import hip
    forms = {}
    for name, build, per_row, *_ in mc.CASES:
        rows, cols, ldx = hip.adaround_rows(build(torch.device("cpu")))
        forms.setdefault(hip.mse_search_form(rows, cols, per_row), []).append((name, rows * cols))
    assert set(forms) == {hip.MSE_FORM_WAVE, hip.MSE_FORM_BLOCK, hip.MSE_FORM_SPREAD}
    spread = [n for _, n in forms[hip.MSE_FORM_SPREAD]]
    assert min(spread) <= 2048 and max(spread) >= 64 * 2048


def test_split_module_initialises_both_activation_quantisers(cuda, knob_off):
    """A split QuantModule conv fed one fixed input: act_quantizer and act_quantizer_0 take the composition's values, through
    two searches over channel slices read in place."""
    from qdiff.quant_layer import QuantModule

    def init(fused):
        torch.manual_seed(0)
        conv = nn.Conv2d(48, 8, 3, padding=1).to(cuda)
        m = QuantModule(conv, dict(n_bits=8, channel_wise=True, scale_method='max'), dict(n_bits=8, scale_method='mse', leaf_param=True))
        m.set_quant_state(False, True)
        x = mc.activations((2, 48, 7, 7), cuda)
        knob_off.MSE_INIT_SEARCHES[0] = 0
        knob_off.set_fused_mse_init(fused)
        try:
            with torch.no_grad():
                m(x, split=21)
        finally:
            knob_off.set_fused_mse_init(False)
        return m, knob_off.MSE_INIT_SEARCHES[0]

    m_off, n_off = init(False)
    m_on, n_on = init(True)
    assert (n_off, n_on) == (0, 2)
    for a, b in ((m_on.act_quantizer, m_off.act_quantizer), (m_on.act_quantizer_0, m_off.act_quantizer_0)):
        assert a.inited and isinstance(a.delta, nn.Parameter) and a.delta.shape == b.delta.shape == ()
        assert torch.equal(a.delta, b.delta) and torch.equal(a.zero_point, b.zero_point)
        assert torch.equal(a.x_min, b.x_min) and torch.equal(a.x_max, b.x_max)


def test_tiny_model_weight_quantisers_initialise_through_the_route(cuda, knob_off):
    off, n_off = mc.tiny_model_weight_init(cuda, fused=False)
    on, n_on = mc.tiny_model_weight_init(cuda, fused=True)
    assert n_off == 0 and n_on == len(on) == len(off) and any(k.endswith(".1") for k in on)
    differ = {k: int(((on[k][0] != off[k][0]) | (on[k][1] != off[k][1])).sum()) for k in off}
    print("mse_init tiny model: rows differing per quantiser", {k: v for k, v in differ.items() if v}, "of", len(off), "quantisers")
    for k in off:
        assert on[k][0].is_cuda and on[k][0].shape == off[k][0].shape
        assert torch.equal(on[k][0], off[k][0]) and torch.equal(on[k][1], off[k][1]), k
