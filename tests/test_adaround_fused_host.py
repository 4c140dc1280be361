"""CPU tests (no GPU) of the fused AdaRound route of the weight phase of calibration (engine.FUSED_ADAROUND, qd_adaround_fwd /
qd_adaround_bwd): the autograd Function against autograd's composition, every refusal of the gate, the
objective that takes the stashed regulariser, the reference's calibration fixture with the route on, the ctypes signatures and
the argument checks of the C entries.  The entry points run on tests/adaround_emulator.py."""
import ctypes
import logging
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import adaround_cases as ac
import adaround_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    calls = adaround_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "FUSED_ADAROUND", False)
    yield SimpleNamespace(engine=engine, calls=calls, monkeypatch=monkeypatch)


def _case(shape, bits, seed=0, planted=(), split=None):
    w = ac.weights(shape, seed, CPU)
    if split is not None:
        w = w[:, :split] if split > 0 else w[:, -split:]
    return w, ac.make_quantizer(w, bits, seed + 1, planted)


CASES = [((48, 32, 3, 3), 4, None), ((40, 96), 8, None), ((16, 3, 3, 3), 4, None), ((5, 1031), 8, None), ((1, 1, 1, 1), 4, None),
         ((32, 48, 3, 3), 4, 16), ((32, 48, 3, 3), 4, -16)]


def test_knob_defaults_off_and_is_a_flag(monkeypatch):
    from qdiff import engine
    assert engine._parse_flag(os.environ.get("QDIFF_FUSED_ADAROUND"), "QDIFF_FUSED_ADAROUND") == engine.FUSED_ADAROUND
    if os.environ.get("QDIFF_FUSED_ADAROUND") is None:
        assert engine.FUSED_ADAROUND is False
    monkeypatch.setattr(engine, "FUSED_ADAROUND", False)
    engine.set_fused_adaround("1")
    assert engine.FUSED_ADAROUND is True
    engine.set_fused_adaround(False)
    assert engine.FUSED_ADAROUND is False
    with pytest.raises(ValueError):
        engine.set_fused_adaround(2)
    assert not engine.adaround_device_ok(torch.zeros(1))


@pytest.mark.parametrize("shape,bits,split", CASES)
@pytest.mark.parametrize("b", [20, 7.3, 2, None])
def test_function_gradients_match_autograd(emu, shape, bits, split, b):
    """FusedAdaRound on the emulated entry points against autograd's composition on the same tensors: both within the issue's
    relative bound of the fp64 evaluation, and a few ulp from each other: galpha within 4 ulp of the per-element unit of
    adaround_cases, reg_sum within 4 ulp of its unit, w_hat bit-equal — the emulator follows the header, the header follows
    autograd; the association of the products is all that differs."""
    w, q = _case(shape, bits, seed=3, planted=(0.0, ac.LOG11, -ac.LOG11, 30.0, -30.0), split=split)
    g = torch.Generator().manual_seed(11)
    gw = torch.randn(w.shape, generator=g)
    greg = 0.017
    ef, ec, ref = ac.judge(q, w, b, gw, greg, label=f"host {shape} split={split}")
    c_w, c_reg, c_g = ac.run_route(q, w, b, gw, greg, fused=False)
    n0 = len(emu.calls)
    f_w, f_reg, f_g = ac.run_route(q, w, b, gw, greg, fused=True)
    assert emu.calls[n0:] == ["adaround_fwd", "adaround_bwd"]
    cols = w.numel() // w.shape[0]
    assert adaround_emulator.GW_STRIDES[-1] == (cols, 2 * cols if w.shape[0] > 1 else cols)      # the gradient slice, in place
    keep = ~ref["near"]
    unit = ref["unit"]
    d = (f_g.double() - c_g.double()).abs().reshape(unit.shape)
    assert (d[keep] <= 4 * 2.0 ** -23 * unit[keep] + 1e-30).all()
    assert torch.equal(f_w, c_w)
    if b is not None:
        assert abs(float(f_reg) - float(c_reg)) <= 4 * 2.0 ** -23 * float(ref["reg_mag"])


def test_value_edges_on_the_emulated_route(emu):
    """alpha = 0, +-log 11, +-30, +-100, a constant row, a row of zeros in w: finite, exact zeros where the target saturates."""
    w = ac.weights((6, 40), 5, CPU)
    w[1] = 0.0
    w[2] = 0.25
    q = ac.make_quantizer(w, 4, 6, planted=(0.0, ac.LOG11, -ac.LOG11, 30.0, -30.0, 100.0, -100.0))
    gw = torch.randn(w.shape, generator=torch.Generator().manual_seed(2))
    for b in (20, 2):
        c_w, _, c_g = ac.run_route(q, w, b, gw, 0.01, fused=False)
        f_w, f_reg, f_g = ac.run_route(q, w, b, gw, 0.01, fused=True)
        assert torch.isfinite(f_w).all() and torch.isfinite(f_g).all() and torch.isfinite(f_reg)
        assert (f_g.reshape(-1)[3:7] == 0).all() and torch.equal(f_w.reshape(-1)[3:7], c_w.reshape(-1)[3:7])
        assert torch.equal(f_g.reshape(-1)[3:7], c_g.reshape(-1)[3:7])
        assert torch.equal(f_w[1:3], c_w[1:3]) or (f_w[1:3] - c_w[1:3]).abs().max() <= 2.0 ** -20


def _gate_quantizer():
    w, q = _case((8, 12), 4, seed=1)
    return w, q


def test_gate_each_single_miss_keeps_the_composition(emu):
    from qdiff import engine

    def launches(q, w, knob=True, grad=True):
        emu.engine.ADAROUND_LAUNCHES[0] = 0
        engine.set_fused_adaround(knob)
        try:
            with torch.set_grad_enabled(grad):
                y = q(w)
        finally:
            engine.set_fused_adaround(False)
        return emu.engine.ADAROUND_LAUNCHES[0], y

    w, q = _gate_quantizer()
    n, y_fused = launches(q, w)
    assert n == 1                                                  # every condition met: the route engages
    n, y_off = launches(q, w, knob=False)
    assert n == 0                                                  # the knob
    assert (y_fused - y_off).abs().max() <= 2.0 ** -20 * q.delta.max()
    assert launches(q, w, grad=False)[0] == 0                      # autograd off
    q.soft_targets = False
    assert launches(q, w)[0] == 0                                  # hard rounding
    q.soft_targets = True
    q.round_mode = 'nearest'
    assert launches(q, w)[0] == 0                                  # another rounding mode
    q.round_mode = 'learned_hard_sigmoid'
    q.alpha.requires_grad_(False)
    assert launches(q, w)[0] == 0                                  # alpha is not being trained
    q.alpha.requires_grad_(True)
    assert launches(q, w)[0] == 1
    # fp16
    w16, q16 = _gate_quantizer()
    q16.alpha = nn.Parameter(q16.alpha.detach().half())
    q16.delta, q16.zero_point = q16.delta.half(), q16.zero_point.half()
    assert launches(q16, w16.half())[0] == 0
    # a device the kernels do not run on
    emu.monkeypatch.setattr(engine, "adaround_device_ok", lambda t: False)
    assert launches(q, w)[0] == 0
    emu.monkeypatch.setattr(engine, "adaround_device_ok", lambda t: True)
    # delta neither per row nor a scalar
    wd, qd = _gate_quantizer()
    qd.delta = qd.delta.expand(8, 12).clone()
    n, y = launches(qd, wd)
    assert n == 0 and y.shape == wd.shape
    # a scalar delta / python zero point is fine
    ws, qs = _gate_quantizer()
    qs.delta, qs.zero_point = qs.delta.max().reshape(()), 7.0
    n, y = launches(qs, ws)
    n0, y0 = launches(qs, ws, knob=False)
    assert (n, n0) == (1, 0) and (y - y0).abs().max() <= 2.0 ** -20 * float(qs.delta)
    kept = qs.__dict__['_row_cache']['delta'][1]
    launches(qs, ws)
    assert qs.__dict__['_row_cache']['delta'][1] is kept          # the expansion of a scalar is made once
    # rows that are not dense in memory, rows that overlap
    wt = ac.weights((12, 8), 1, CPU).t()
    assert launches(q, wt)[0] == 0
    assert launches(q, ac.weights((1, 12), 1, CPU).expand(8, 12))[0] == 0
    # a 1-D delta of `rows` values on a weight whose last dimension is `rows` too: the composition broadcasts it along the LAST axis
    w1 = ac.weights((8, 8), 1, CPU)
    q1 = ac.make_quantizer(w1, 4, 2)
    q1.delta, q1.zero_point = q1.delta.reshape(8), q1.zero_point.reshape(8)
    n, y = launches(q1, w1)
    n0, y0 = launches(q1, w1, knob=False)
    assert n == 0 and torch.equal(y, y0)


def _unit(split):
    """A small QuantModule (optionally with a split input) in the weights-only state, its input, and a target."""
    import qdiff
    from qdiff.quant_layer import QuantModule
    torch.manual_seed(0)
    conv = nn.Conv2d(12, 8, 3, padding=1)
    m = QuantModule(conv, dict(n_bits=4, channel_wise=True, scale_method='max'), dict(n_bits=8, scale_method='max', leaf_param=True))
    x = torch.randn(4, 12, 6, 6)
    m.set_quant_state(True, False)
    with torch.no_grad():
        tgt = conv(x)
        m(x, split=split)
    return m, x, tgt


@pytest.mark.parametrize("split,layer_unit", [(0, True), (5, True), (5, False)])
def test_objective_total_and_log_value_equal_the_compositions(emu, caplog, split, layer_unit):
    """ReconstructionObjective with the stashed reg_sum against the second get_soft_targets() graph: the same `total`, the same
    500-call log line, the warm-up rule, alpha.grad within the Function's bound — and weight_quantizer_0 of a split layer
    reconstructed as a layer stays hard: no launch, no gradient."""
    from qdiff import recon
    m, x, tgt = _unit(split)
    recon.to_adaround(m, layer_unit=layer_unit)
    for q in m._weight_quantizers():
        with torch.no_grad():
            q.alpha.mul_(1.5)
    nq = len(m._weight_quantizers())
    soft = sum(q.soft_targets for q in m._weight_quantizers())
    assert soft == (1 if (split and layer_unit) or not split else 2)
    seen = [ac.Upstream(q) for q in m._weight_quantizers()]

    def run(fused, calls0):
        obj = recon.ReconstructionObjective(m, iters=1000, weight=0.01, b_range=(20, 2), warmup=0.2)
        obj.calls = calls0
        for q in m._weight_quantizers():
            q.alpha.grad = None
        emu.engine.ADAROUND_LAUNCHES[0] = 0
        emu.engine.set_fused_adaround(fused)
        try:
            if fused:
                obj.arm()
            with caplog.at_level(logging.INFO, logger="qdiff.recon"):
                caplog.clear()
                total = obj(m(x, split=split), tgt)
            total.backward()
        finally:
            obj.disarm()
            emu.engine.set_fused_adaround(False)
        logs = [r.getMessage() for r in caplog.records if "Total loss" in r.getMessage()]
        return total.detach(), logs, [None if q.alpha.grad is None else q.alpha.grad.clone() for q in m._weight_quantizers()], \
            emu.engine.ADAROUND_LAUNCHES[0]

    for calls0 in (10, 499, 800):                                  # warm-up (no regulariser), the logging call, annealing
        t_c, log_c, g_c, n_c = run(False, calls0)
        t_f, log_f, g_f, n_f = run(True, calls0)
        assert n_c == 0 and n_f == 2 * soft                        # one forward + one backward launch per soft quantiser
        assert all('_reg_b' not in q.__dict__ and '_reg_sum' not in q.__dict__ for q in m._weight_quantizers())
        assert abs(float(t_f) - float(t_c)) <= 4 * 2.0 ** -23 * abs(float(t_c))
        assert log_f == log_c and len(log_c) == (1 if calls0 == 499 else 0)
        b = recon.ReconstructionObjective(m, iters=1000, b_range=(20, 2), warmup=0.2)._exponent(calls0 + 1)
        for i, (q, up, a, c) in enumerate(zip(m._weight_quantizers(), seen, g_f, g_c)):
            assert (a is None) == (c is None)
            if a is not None:                                      # a few ulp of the per-element unit, as in the Function's test
                ref = ac.reference64(up.w, ac._cpu_view(q), b if i == 0 else None, up.gw, 0.01)
                d = (a.double() - c.double()).abs().reshape(ref["unit"].shape)
                assert (d[~ref["near"]] <= 4 * 2.0 ** -23 * ref["unit"][~ref["near"]] + 1e-30).all()
        if split and layer_unit:
            assert g_f[1] is None, "weight_quantizer_0 of a split layer unit must receive no gradient"
        if split:                                                  # the halves' gradients are slices of the torch.cat gradient, taken in place
            taken = adaround_emulator.GW_STRIDES[-soft:]
            assert all(ldg == 12 * 9 and cols in (5 * 9, 7 * 9) for cols, ldg in taken), taken
    assert nq == (2 if split else 1)


def test_calibration_fixture_bounds_hold_with_the_emulated_route(emu):
    """tests/test_calibration.py's bounds against the REFERENCE's cifar_tiny fixture, weight phase through the fused route."""
    from test_calibration import _calibration_vs_reference_fixture
    emu.engine.set_fused_adaround(True)
    try:
        _calibration_vs_reference_fixture("cifar_tiny", CPU)
    finally:
        emu.engine.set_fused_adaround(False)
    assert emu.engine.ADAROUND_LAUNCHES[0] > 0 and emu.engine.ADAROUND_LAUNCHES[0] % 2 == 0


def test_prototypes_argtypes_exports_and_abi():
    from qdiff import hip
    lib = hip.load()
    assert lib.qd_abi_version() == 20
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qdiff_hip.h")).read(), flags=re.S)
    i64, i32, vp, f32 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    kinds = {"ptr": vp, "int": i32, "int64_t": i64, "float": f32}
    for name in ("qd_adaround_blocks", "qd_adaround_fwd", "qd_adaround_bwd"):
        assert name in hip.EXPORTS and hasattr(lib, name)
        args = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", h, flags=re.S).group(1)
        want = [kinds["ptr" if "*" in a else a.replace("const", "").split()[0]] for a in args.split(",")]
        assert list(getattr(lib, name).argtypes) == want, name
    assert len(lib.qd_adaround_fwd.argtypes) == 14 and len(lib.qd_adaround_bwd.argtypes) == 16
    assert lib.qd_adaround_blocks.restype is i64
    assert lib.qd_adaround_blocks(5, 1031) == (5 * 1031 + 1023) // 1024 and lib.qd_adaround_blocks(0, 4) == 0
    doc = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    assert "adaptive_rounding.py:39-74" in doc and "block_recon.py:217-229" in doc


def test_entry_points_refuse_null_empty_and_misaligned_arguments():
    """The argument checks come before the launch: on fake pointers, without a GPU, through qd_last_error."""
    from qdiff import hip
    lib = hip.load()
    P = 0x10000

    def fwd(w=P, rows=4, cols=8, ldw=8, alpha=P, delta=P, zp=P, n_levels=16, gamma=-0.1, zeta=1.1, b=0.0, w_hat=P, part=None):
        rc = lib.qd_adaround_fwd(w, rows, cols, ldw, alpha, delta, zp, n_levels, gamma, zeta, b, w_hat, part, None)
        return rc, lib.qd_last_error().decode()

    def bwd(gw=P, ldg=8, w=P, rows=4, cols=8, ldw=8, alpha=P, delta=P, zp=P, n_levels=16, gamma=-0.1, zeta=1.1, b=0.0, greg=None,
            galpha=P):
        rc = lib.qd_adaround_bwd(gw, ldg, w, rows, cols, ldw, alpha, delta, zp, n_levels, gamma, zeta, b, greg, galpha, None)
        return rc, lib.qd_last_error().decode()

    for call, name in ((fwd, "qd_adaround_fwd"), (bwd, "qd_adaround_bwd")):
        for kw in (dict(w=None), dict(alpha=None), dict(delta=None), dict(zp=None)):
            rc, msg = call(**kw)
            assert rc != 0 and name in msg and "null pointer" in msg, (kw, msg)
        for kw in (dict(rows=0), dict(cols=0)):
            rc, msg = call(**kw)
            assert rc != 0 and "empty tensor" in msg, (kw, msg)
        rc, msg = call(ldw=7)
        assert rc != 0 and "row stride" in msg
        rc, msg = call(rows=1 << 20, cols=1 << 11, ldw=1 << 11)
        assert rc != 0 and "31-bit" in msg
        rc, msg = call(n_levels=1)
        assert rc != 0 and "n_levels" in msg
        rc, msg = call(gamma=1.1, zeta=1.1)
        assert rc != 0 and "zeta > gamma" in msg
        rc, msg = call(alpha=P + 4)
        assert rc != 0 and "16-byte aligned" in msg
    rc, msg = fwd(w_hat=None)
    assert rc != 0 and "null pointer" in msg
    rc, msg = fwd(w_hat=P + 8)
    assert rc != 0 and "w_hat must be 16-byte aligned" in msg
    rc, msg = fwd(b=20.0, part=None)
    assert rc != 0 and "partial sums" in msg
    rc, msg = bwd(gw=None)
    assert rc != 0 and "null pointer" in msg
    rc, msg = bwd(ldg=7)
    assert rc != 0 and "gw row stride" in msg
    rc, msg = bwd(galpha=P + 4)
    assert rc != 0 and "16-byte aligned" in msg
