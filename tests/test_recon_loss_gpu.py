"""GPU tests of the fused reconstruction term (engine.FUSED_RECON_LOSS, csrc/recon_loss.hip) through
hip.recon_loss.  References: the composition of qdiff.recon in fp64 on the gathered rows, differentiated by autograd (loss), and
the same composition in fp32 on the same GPU (gradient, bit for bit)."""
import math

import numpy as np
import pytest
import torch

from golden_util import build_engine_model, load_fixture, quant_params

pytestmark = pytest.mark.gpu

# one element; smaller than a quad / a tile; ragged in both tile axes; whole tiles; several work items per sample, samples that
# start off 16 bytes and a scalar tail; a [B, T, C] transformer output
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 33, 9, 9), (2, 64, 16, 16), (4, 40, 33, 31), (3, 50, 12)]
LAYOUTS = ["nchw", "cl"]
ROWS, GUARD = 6, 777.0


def _dense(rows, shape, layout, dev):
    """(buffer, view): `rows` + 2 dense samples of `shape` in the given order filled with GUARD; the view leaves a guard row on
    either side."""
    buf = torch.full((rows + 2,) + (shape if layout == "nchw" else shape[1:] + shape[:1]), GUARD, device=dev)
    return buf, (buf if layout == "nchw" else buf.movedim(-1, 1))[1:-1]


def _case(dev, shape, pred_layout, cache_layout):
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    B, idx = shape[0], torch.tensor([4, 1, 4, 0][:shape[0]], device=dev)       # unordered, row 4 twice
    bufs, views = zip(*[_dense(n, shape[1:], lay, dev) for n, lay in ((ROWS, cache_layout), (ROWS, cache_layout), (B, pred_layout))])
    tgt, grad, pred = views
    tgt.copy_(torch.randn((ROWS,) + shape[1:], generator=g, device=dev))
    grad.copy_(torch.randn((ROWS,) + shape[1:], generator=g, device=dev))
    noise = torch.randn(shape, generator=g, device=dev) * 0.1
    noise.flatten()[1::5] = 0                                                  # exact zeros in d: sgn(0)
    pred.copy_(tgt[idx] + noise)
    return pred, tgt, grad, idx, bufs


def _composition(mode, pred, tgt, grad, dtype):
    from qdiff.recon import _reconstruction_term
    p = pred.detach().to(dtype).requires_grad_()
    loss = _reconstruction_term(mode, p, tgt.to(dtype), grad.to(dtype), 2.0)
    loss.backward()
    return loss.detach(), p.grad


def _bits(t):
    t = t.contiguous()
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)


def _fused(mode, pred, tgt, grad, idx):
    from qdiff import hip
    return hip.recon_loss(pred, tgt, idx, hip.RECON_MSE if mode == "mse" else hip.RECON_FISHER_DIAG, grad if mode != "mse" else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cache_layout", LAYOUTS)
@pytest.mark.parametrize("pred_layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["mse", "fisher_diag"])
def test_loss_and_gradient_against_the_composition(cuda, mode, pred_layout, cache_layout, shape):
    from qdiff import hip
    pred, tgt, grad, idx, bufs = _case(cuda, shape, pred_layout, cache_layout)
    loss, gpred = _fused(mode, pred, tgt, grad, idx)
    again = _fused(mode, pred, tgt, grad, idx)
    assert torch.equal(_bits(loss), _bits(again[0])) and torch.equal(_bits(gpred), _bits(again[1]))     # a fixed order
    assert gpred.shape == pred.shape and hip.recon_orders(gpred) == hip.recon_orders(pred)              # pred's order
    l32, g32 = _composition(mode, pred, tgt[idx], grad[idx], torch.float32)
    l64, _ = _composition(mode, pred, tgt[idx], grad[idx], torch.float64)
    assert torch.equal(_bits(gpred), _bits(g32)), f"worst difference {(gpred - g32).abs().max().item():.3e}"
    bound = (math.ceil(math.log2(pred.numel())) + 4) * 2.0 ** -24
    err, err32 = (abs(float(v) - float(l64)) / float(l64) for v in (loss, l32))
    print(f"\n[recon_loss {mode} {pred_layout}/{cache_layout} {tuple(shape)}] loss error / fp64: fused {err:.2e}, composition {err32:.2e}, bound {bound:.2e}")
    assert err <= bound
    for buf in bufs[:2]:                                                       # the caches: read in place, nothing written
        assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all())


@pytest.mark.parametrize("cache_layout", LAYOUTS)
@pytest.mark.parametrize("pred_layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["mse", "fisher_diag"])
def test_nan_element_and_guard_rows_around_gpred(cuda, mode, pred_layout, cache_layout):
    """A NaN in pred: the loss is NaN, gpred holds it in that element alone.  The raw entry writes the same gpred into the middle
    of a guarded buffer and leaves the guard rows alone."""
    from qdiff import hip
    shape = SHAPES[2]
    pred, tgt, grad, idx, _ = _case(cuda, shape, pred_layout, cache_layout)
    pred[1, 7, 3, 2] = float("nan")
    loss, gpred = _fused(mode, pred, tgt, grad, idx)
    assert bool(torch.isnan(loss)) and torch.isnan(gpred).nonzero().tolist() == [[1, 7, 3, 2]]
    _, g32 = _composition(mode, pred, tgt[idx], grad[idx], torch.float32)
    assert torch.equal(_bits(gpred), _bits(g32))
    buf, out = _dense(shape[0], shape[1:], pred_layout, cuda)
    lib, cl = hip.load(), lambda lay: int(lay == "cl")
    C, S = shape[1], shape[2] * shape[3]
    ws, raw_loss = torch.empty(lib.qd_recon_loss_ws_bytes(shape[0], C, S) // 4, device=cuda), torch.empty((), device=cuda)
    rc = lib.qd_recon_loss(pred.data_ptr(), C * S, cl(pred_layout), tgt.data_ptr(), grad.data_ptr() if mode != "mse" else None, ROWS, C * S,
                           cl(cache_layout), idx.data_ptr(), shape[0], C, S, int(mode != "mse"), raw_loss.data_ptr(), out.data_ptr(),
                           ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qd_last_error()
    assert torch.equal(_bits(out), _bits(gpred)) and bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all())


def test_backward_applies_an_upstream_gradient(cuda):
    from qdiff import engine, recon
    pred, tgt, grad, idx, _ = _case(cuda, SHAPES[2], "cl", "nchw")
    engine.set_fused_recon_loss(True)
    try:
        grads = []
        for scale in (1.0, 3.0):
            p = pred.detach().requires_grad_()
            (recon._reconstruction_term("mse", p, (tgt, idx), None, 2.0) * scale).backward()
            grads.append(p.grad)
    finally:
        engine.set_fused_recon_loss(False)
    _, g32 = _composition("mse", pred, tgt[idx], grad[idx], torch.float32)
    assert torch.equal(_bits(grads[0]), _bits(g32)) and torch.equal(_bits(grads[1]), _bits(g32 * 3.0))


def _calibrate(dev, fused, iters=12):
    """Weight phase, then activation phase (p = 2), of the first block of the cifar_tiny fixture; the trained alpha and delta."""
    import qdiff
    from qdiff import engine
    from qdiff.adaptive_rounding import AdaRoundQuantizer
    from qdiff.block_recon import block_reconstruction
    from qdiff.quant_block import BaseQuantBlock
    from test_calibration import _inputs
    fx = load_fixture("recon_cifar_tiny.pt")
    spec = fx["spec"]
    cali = _inputs(spec, fx["n_cal"], fx["cal_seed"])[:2]
    qnn = qdiff.QuantModel(build_engine_model(spec).to(dev), *quant_params(spec), sm_abit=spec["sm_abit"]).to(dev).eval()
    unit = next(m for m in qnn.modules() if isinstance(m, BaseQuantBlock))
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    engine.set_fused_recon_loss(fused)
    calls = engine.RECON_LOSS_CALLS[0]
    try:
        for act_quant in (False, True):
            qnn.set_quant_state(True, act_quant)
            with torch.no_grad(), engine.simulation():
                qnn(*(a[:4].to(dev) for a in cali))
            block_reconstruction(qnn, unit, cali_data=cali, batch_size=fx["batch"], iters=iters, weight=0.01, asym=True, b_range=(20, 2),
                                 warmup=0.2, act_quant=act_quant, opt_mode='mse', lr=4e-4, p=2.0)
    finally:
        engine.set_fused_recon_loss(False)
    out = {k + ".alpha": m.alpha.detach() for k, m in unit.named_modules() if isinstance(m, AdaRoundQuantizer)}
    out.update({k: v.detach() for k, v in unit.named_parameters() if k.endswith("delta")})
    return out, engine.RECON_LOSS_CALLS[0] - calls


def test_reconstruct_trains_the_same_parameters(cuda):
    """d loss / d pred is bit-identical and the loss value feeds nothing, but equality of alpha and delta was NOT what the MI355X
    showed: the worst difference after 12 + 12 iterations was 1.192e-07 (2^-23, in conv2.weight_quantizer.alpha) — and two runs
    with the knob OFF differed by the same 1.192e-07, so the unit's own backward does not repeat bit for bit there and the
    difference is not the route's.  Bound: twice the measured figure.  The knob-off rerun is printed next to it."""
    want, n_off = _calibrate(cuda, False)
    got, n_on = _calibrate(cuda, True)
    assert n_off == 0 and n_on == 2 * 12 and set(got) == set(want) and len(got) > 2
    worst, key = max((float((got[k] - want[k]).abs().max()), k) for k in want)
    rerun = max(float((v - want[k]).abs().max()) for k, v in _calibrate(cuda, False)[0].items())
    print(f"\n[recon_loss cifar_tiny first block, 12 + 12 iterations] worst |difference| of alpha / delta: on vs off {worst:.3e} ({key}), "
          f"off vs off again {rerun:.3e}")
    assert worst <= 2 * 2.0 ** -23
