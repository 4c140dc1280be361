"""Cases and the judge shared by the tests of the fused MSE range search (engine.FUSED_MSE_INIT, qd_mse_search, DESIGN.md
§4.21).  A case is (view, per_row, n_bits, symmetric, always_zero): the view is what the quantiser would be handed — a dense
tensor or a channel slice read in place.  judge() runs hip.mse_search on it (the kernel on the GPU, tests/mse_init_emulator.py
on the host) and holds it to the torch composition and to an fp64 evaluation of the scores, on the view's device."""
import torch

ULP4 = 4 * 2.0 ** -23          # floor of the score bound: the 4-ulp unit of tests/adaround_cases.py


def weights(shape, device, seed=17):
    """randn * rand-per-row: channels of very different ranges."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * torch.rand(shape[0], *([1] * (len(shape) - 1)), generator=g)
    return w.to(device)


def activations(shape, device, seed=5):
    """randn with 0.1 % outliers (x 20): the clipping the search exists for."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    out = torch.rand(shape, generator=g) < 1e-3
    return torch.where(out, x * 20, x).to(device)


def softmax_probs(shape, device, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(shape, generator=g) * 3, dim=-1).to(device)


def value_edges(device):
    """(8, 40): a zero row, a constant row, an all-positive row, an all-negative row, one 50.0 outlier, one NaN, one +inf, and
    an ordinary row."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(8, 40, generator=g)
    x[0] = 0.0
    x[1] = 0.25
    x[2] = x[2].abs() + 0.1
    x[3] = -x[3].abs() - 0.1
    x[4, 7] = 50.0
    x[5, 11] = float("nan")
    x[6, 3] = float("inf")
    return x.to(device)


# (name, builder(device) -> view, per_row, n_bits, symmetric, always_zero)
WEIGHT_CASES = [
    ("w48x32x3x3_4b", lambda d: weights((48, 32, 3, 3), d), True, 4, False, False),
    ("w40x96_8b", lambda d: weights((40, 96), d), True, 8, False, False),
    ("w16x3x3x3_4b_misaligned", lambda d: weights((16, 3, 3, 3), d), True, 4, False, False),
    ("w5x1031_8b_odd_long", lambda d: weights((5, 1031), d), True, 8, False, False),
    ("w1x1x1x1", lambda d: weights((1, 1, 1, 1), d), True, 4, False, False),
    ("w10240x8_4b_short_rows", lambda d: weights((10240, 8), d), True, 4, False, False),
    ("w2x2560x3x3_4b_long_rows", lambda d: weights((2, 2560, 3, 3), d), True, 4, False, False),
    ("w32x48x3x3_first_half", lambda d: weights((32, 48, 3, 3), d)[:, :16], True, 4, False, False),
    ("w32x48x3x3_second_half", lambda d: weights((32, 48, 3, 3), d)[:, -16:], True, 4, False, False),
    ("w40x96_8b_symmetric", lambda d: weights((40, 96), d), True, 8, True, False),
]
ACT_CASES = [
    ("a2x32x16x16_8b", lambda d: activations((2, 32, 16, 16), d), False, 8, False, False),
    ("a2x32x16x16_4b", lambda d: activations((2, 32, 16, 16), d), False, 4, False, False),
    ("a3x5x7x11_odd_tail", lambda d: activations((3, 5, 7, 11), d), False, 8, False, False),
    ("a4x64x32x32_many_blocks", lambda d: activations((4, 64, 32, 32), d), False, 8, False, False),
    ("a2x48x7x7_first_slice", lambda d: activations((2, 48, 7, 7), d)[:, :21], False, 8, False, False),
    ("a2x48x7x7_second_slice", lambda d: activations((2, 48, 7, 7), d)[:, 21:], False, 8, False, False),
    ("softmax8x64x77_16b", lambda d: softmax_probs((8, 64, 77), d), False, 16, False, True),
    ("softmax8x64x77_8b", lambda d: softmax_probs((8, 64, 77), d), False, 8, False, True),
]
EDGE_CASES = [(f"edges_{bits}b_{'rows' if per_row else 'whole'}", value_edges, per_row, bits, False, False)
              for bits in (4, 8) for per_row in (True, False)]
CASES = WEIGHT_CASES + ACT_CASES + EDGE_CASES


def make_quantizer(per_row, n_bits, symmetric, always_zero, leaf_param=False):
    from qdiff.quant_layer import UniformAffineQuantizer
    return UniformAffineQuantizer(n_bits=n_bits, symmetric=symmetric, channel_wise=per_row, scale_method="mse",
                                  leaf_param=leaf_param, always_zero=always_zero)


def groups(x, per_row):
    """[G, N] dense copy of what one search covers."""
    return x.reshape(x.shape[0], -1) if per_row else x.reshape(1, -1)


def candidate(q, x_min, x_max, f):
    """(d, z) of shrink factor f: the composition's torch expressions, on the device of x_min / x_max."""
    levels = 2 ** q.n_bits - 1
    new_max, new_min = x_max * f, x_min * f
    d = (new_max / levels) if q.always_zero else ((new_max - new_min) / levels)
    z = torch.zeros_like(d) if q.always_zero else (-new_min / d).round()
    return d, z


def composition(q, flat, per_row):
    """The product's composition (UniformAffineQuantizer._init_mse_channelwise per row, the scalar branch of
    init_quantization_scale for the whole tensor) with its scores and picks kept, plus the fp64 evaluation of every score:
    |x - xq| from the fp32 torch expressions, then double().pow(2.4).mean().  Returns dict(scores [G, 80] fp32, scores64,
    index [G], delta [G], zero_point [G], x_min, x_max)."""
    x_max, x_min = flat.max(dim=1, keepdim=True)[0], flat.min(dim=1, keepdim=True)[0]
    G = flat.shape[0]
    best = torch.full_like(x_max, 1e+10)
    delta, zero_point = torch.zeros_like(x_max), torch.zeros_like(x_max)
    index = torch.full((G, 1), -1, dtype=torch.int64, device=flat.device)
    scores, scores64 = [], []
    for i in range(80):
        d, z = candidate(q, x_min, x_max, 1.0 - (i * 0.01))
        xq = (torch.clamp(torch.round(flat / d) + z, 0, q.n_levels - 1) - z) * d
        err = (flat - xq).abs()
        score = err.pow(2.4).mean(dim=1, keepdim=True) if per_row else err.pow(2.4).mean().reshape(1, 1)
        scores.append(score)
        scores64.append(err.double().pow(2.4).mean(dim=1, keepdim=True))
        better = score < best
        best = torch.where(better, score, best)
        delta = torch.where(better, d, delta)
        zero_point = torch.where(better, z, zero_point)
        index = torch.where(better, torch.full_like(index, i), index)
    return dict(scores=torch.cat(scores, 1), scores64=torch.cat(scores64, 1), index=index.flatten(), delta=delta.flatten(),
                zero_point=zero_point.flatten(), x_min=x_min.flatten(), x_max=x_max.flatten())


def first_strictly_better(scores):
    """The selection rule on a [G, n] score matrix: best = 1e10, ascending i, taken only when score < best; -1 = none."""
    best = torch.full((scores.shape[0],), 1e+10, dtype=scores.dtype, device=scores.device)
    index = torch.full((scores.shape[0],), -1, dtype=torch.int64, device=scores.device)
    for i in range(scores.shape[1]):
        better = scores[:, i] < best
        best = torch.where(better, scores[:, i], best)
        index = torch.where(better, torch.full_like(index, i), index)
    return index


def same_bits(a, b):
    """torch.equal that also holds a NaN equal to the same NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def worst_rel(scores, scores64):
    """Worst relative error of fp32 scores against the fp64 ones, over the finite positive ones; the others must agree in kind."""
    s, r = scores.double(), scores64
    ok = torch.isfinite(r) & (r > 0)
    assert torch.equal(torch.isnan(s), torch.isnan(r)), "a score is NaN on one side only"
    if not ok.any():
        return 0.0
    return float(((s[ok] - r[ok]).abs() / r[ok]).max())


def judge(x, per_row, n_bits, symmetric, always_zero, label=""):
    """The four-part comparison of one case; returns the measured figures (printed before anything is asserted)."""
    from qdiff import hip
    q = make_quantizer(per_row, n_bits, symmetric, always_zero)
    run = lambda: hip.mse_search(x, per_row, n_bits, q.n_levels, always_zero, want_scores=True)
    delta, zp, x_min, x_max, index, scores = run()
    again = run()
    flat = groups(x, per_row)
    G = flat.shape[0]
    comp = composition(q, flat, per_row)
    err_k, err_c = worst_rel(scores, comp["scores64"]), worst_rel(comp["scores"], comp["scores64"])
    bound = max(2 * err_c, ULP4)
    idx_k, idx_c = index.long(), comp["index"]
    differ = idx_k != idx_c
    fig = dict(label=label, groups=G, err_fused=err_k, err_composition=err_c, bound=bound, picks_differ=int(differ.sum()),
               picks=sorted(set(idx_k.tolist())))
    print(f"mse_init {label}: G={G} score error fused {err_k:.3e} composition {err_c:.3e} bound {bound:.3e} "
          f"picks differing {fig['picks_differ']} picks {fig['picks'][:12]}")
    # 1. exact
    assert delta.shape == zp.shape == x_min.shape == x_max.shape == index.shape == (G,) and scores.shape == (G, 80)
    assert index.dtype == torch.int32 and all(t.dtype == torch.float32 for t in (delta, zp, x_min, x_max, scores))
    assert all(same_bits(a, b) for a, b in zip((delta, zp, x_min, x_max, scores), again[:4] + again[5:])) \
        and torch.equal(index, again[4]), "two runs differ"
    assert torch.equal(idx_k, first_strictly_better(scores)), "index is not the first-strictly-better arg-min of the returned scores"
    assert same_bits(x_min, comp["x_min"]) and same_bits(x_max, comp["x_max"])
    taken = idx_k >= 0
    f = hip.mse_factors(x.device)[idx_k.clamp(min=0)]
    d_at, z_at = candidate(q, comp["x_min"], comp["x_max"], f)
    zero = torch.zeros_like(delta)
    assert torch.equal(delta, torch.where(taken, d_at, zero)) and torch.equal(zp, torch.where(taken, z_at, zero))
    assert torch.equal(idx_k < 0, idx_c < 0), "a degenerate group must take nothing on both routes"
    # 2. scores
    assert err_k <= bound, f"{label}: fused score error {err_k:.3e} > bound {bound:.3e} (composition {err_c:.3e})"
    # 3. picks against the composition
    assert float((~differ).float().mean()) >= 0.98, f"{label}: {int(differ.sum())} of {G} picks differ"
    if differ.any():
        assert ((idx_k - idx_c).abs()[differ] == 1).all(), "a differing pick is more than one 1 % step away"
        rows = differ.nonzero().flatten()
        a = comp["scores64"][rows, idx_k[rows]]
        b = comp["scores64"][rows, idx_c[rows]]
        assert ((a - b).abs() <= 2 * bound * torch.maximum(a, b)).all(), "differing picks whose fp64 scores are not a tie"
    same = ~differ
    assert torch.equal(delta[same], comp["delta"][same]) and torch.equal(zp[same], comp["zero_point"][same])
    return fig


def route(q, x, per_row, fused):
    """(delta, zero_point) of a fresh initialisation through the product's gate, knob on or off; restores the knob."""
    from qdiff import engine
    prev = engine.FUSED_MSE_INIT
    engine.set_fused_mse_init(fused)
    try:
        return q.init_quantization_scale(x, per_row)
    finally:
        engine.set_fused_mse_init(prev)


def tiny_model_weight_init(device, fused):
    """The cifar_tiny QuantModel (split shortcuts) with 'mse' weight quantisers, (True, False), one forward: the
    {name: (delta, zero_point)} of every weight quantiser and the number of searches the initialisation made."""
    import qdiff
    from qdiff import engine
    from qdiff.quant_layer import QuantModule
    from golden_util import build_engine_model, load_fixture
    spec = load_fixture("recon_cifar_tiny.pt")["spec"]
    wq = dict(n_bits=spec["w_bits"], channel_wise=True, scale_method="mse")
    aq = dict(n_bits=spec["a_bits"], channel_wise=False, scale_method="max", leaf_param=True)
    qnn = qdiff.QuantModel(build_engine_model(spec).to(device), wq, aq, sm_abit=spec["sm_abit"]).to(device).eval()
    g = torch.Generator().manual_seed(3)
    xs = torch.randn((2,) + tuple(spec["x"]), generator=g).to(device)
    ts = torch.randint(0, 1000, (2,), generator=g).float().to(device)
    qnn.set_quant_state(True, False)
    prev = engine.FUSED_MSE_INIT
    engine.set_fused_mse_init(fused)
    engine.MSE_INIT_SEARCHES[0] = 0
    try:
        with torch.no_grad():
            qnn(xs, ts)
    finally:
        engine.set_fused_mse_init(prev)
    got = {}
    for name, m in qnn.named_modules():
        if isinstance(m, QuantModule):
            for k, wqz in enumerate(m._weight_quantizers()):
                assert wqz.inited
                got[f"{name}.{k}"] = (wqz.delta.detach().clone(), wqz.zero_point.detach().clone())
    return got, engine.MSE_INIT_SEARCHES[0]
