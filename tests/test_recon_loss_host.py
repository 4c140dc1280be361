"""CPU tests (no GPU) of the fused reconstruction term (engine.FUSED_RECON_LOSS, csrc/recon_loss.hip): the new
names are declared, bound and exported; the entry refuses bad arguments on fake pointers before any launch; the objective
returns today's bits whenever the route does not engage, and the gate refuses each unsupported case on its own."""
import os
import re

import pytest
import torch

P = 0x10000                                                         # a fake, 16-byte aligned device pointer: nothing is launched
NAMES = ["qd_recon_loss", "qd_recon_loss_ws_bytes", "qd_recon_loss_scale"]


def test_new_names_are_declared_bound_and_exported():
    from qdiff import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qdiff_hip.h")).read()
    lib = hip.load()
    for name in NAMES:
        assert name in hip.EXPORTS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert lib.qd_recon_loss_ws_bytes(2, 3, 4) == 2048 * 4 and lib.qd_recon_loss_ws_bytes(2, 0, 4) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(gpred=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(mode=1, grad=None), "reads grad_cache"), (dict(mode=2), "unknown mode"), (dict(B=0), "empty tensor"), (dict(rows=0), "empty tensor"),
    (dict(ldp=23), "sample stride"), (dict(ldc=23), "row stride"), (dict(pred=P + 2), "4-byte aligned"), (dict(idx=P + 4), "8-byte aligned")])
def test_entry_refuses_bad_arguments_before_any_launch(kw, word):
    from qdiff import hip
    a = dict(pred=P, ldp=24, tgt=P, grad=P, rows=6, ldc=24, idx=P, B=2, mode=0, loss=P, gpred=P, ws=P)
    a.update(kw)
    lib = hip.load()
    rc = lib.qd_recon_loss(a["pred"], a["ldp"], 0, a["tgt"], a["grad"], a["rows"], a["ldc"], 1, a["idx"], a["B"], 3, 8, a["mode"], a["loss"],
                           a["gpred"], a["ws"], None)
    msg = lib.qd_last_error().decode()
    assert rc != 0 and word in msg and msg.startswith("qd_recon_loss"), (kw, msg)
    assert lib.qd_recon_loss_scale(None, 4, P, None) != 0 and lib.qd_recon_loss_scale(P, 0, P, None) != 0


def _objective(kind, p):
    from qdiff.recon import ReconstructionObjective
    return ReconstructionObjective(torch.nn.Identity(), 10, regularise=False, kind=kind, p=p)


def _tensors(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    cache, gcache = torch.randn(6, 5, 4, 3, generator=g).to(dtype), torch.randn(6, 5, 4, 3, generator=g).to(dtype)
    idx = torch.tensor([4, 1, 4])
    pred = (cache[idx] + 0.1).requires_grad_()
    return pred, cache, gcache, idx


@pytest.mark.parametrize("kind", ["mse", "fisher_diag"])
@pytest.mark.parametrize("knob", [False, True])
def test_objective_returns_todays_bits_off_the_route(monkeypatch, kind, knob):
    """Knob off, or knob on with CPU tensors: the composition, for a plain target and for (cache, idx) alike."""
    from qdiff import engine
    from qdiff.quant_layer import lp_loss
    pred, cache, gcache, idx = _tensors()
    tgt, grad = cache[idx], gcache[idx]
    want = lp_loss(pred, tgt, p=2.0) if kind == "mse" else ((pred - tgt).pow(2) * grad.pow(2)).sum(1).mean()
    monkeypatch.setattr(engine, "FUSED_RECON_LOSS", knob)
    before = engine.RECON_LOSS_CALLS[0]
    for t, g in ((tgt, grad), ((cache, idx), (gcache, idx))):
        got = _objective(kind, 2.0)(pred, t, g)
        assert torch.equal(got, want) and got.grad_fn is not None
    assert engine.RECON_LOSS_CALLS[0] == before


@pytest.mark.parametrize("case", ["p2.4", "fisher_full", "fp16", "host_cache", "strided_pred", "no_grad", "served"])
def test_gate_refuses_each_case_on_its_own(monkeypatch, case):
    """Every tensor passes for a device tensor unless the case says otherwise; 'served' shows that the gate then engages."""
    from qdiff import engine, recon
    pred, cache, gcache, idx = _tensors(torch.float16 if case == "fp16" else torch.float32)
    monkeypatch.setattr(engine, "FUSED_RECON_LOSS", True)
    monkeypatch.setattr(engine, "recon_loss_device_ok", (lambda t: t is pred) if case == "host_cache" else (lambda t: True))
    kind, p = ("fisher_full", 2.0) if case == "fisher_full" else ("mse", 2.4 if case == "p2.4" else 2.0)
    if case == "strided_pred":
        pred = pred[:, :, ::2]
        cache = cache[:, :, ::2].contiguous()
    if case == "no_grad":
        pred = pred.detach()
    fused = recon._fused_term(kind, pred, (cache, idx), (gcache, idx), p)
    assert (fused is not None) == (case == "served")
    if case == "served":
        assert fused[1] is cache and fused[2] is idx and recon._fused_term("fisher_diag", pred, (cache, idx), (gcache, idx), 2.0)[3] is gcache
        engine.set_fused_recon_loss("1")
        assert engine.FUSED_RECON_LOSS is True
        engine.set_fused_recon_loss(False)
        assert engine.FUSED_RECON_LOSS is False
