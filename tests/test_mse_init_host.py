"""CPU tests (no GPU) of the fused MSE range search that initialises a quantiser (engine.FUSED_MSE_INIT, qd_mse_search,
DESIGN.md §4.21): the knob, every refusal of the gate, what the gate returns in each form, the ctypes signatures and the argument
checks of the C entries, and a tiny QuantModel initialised through the route.  The entry runs on tests/mse_init_emulator.py."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import mse_init_cases as mc
import mse_init_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    seen = mse_init_emulator.install(monkeypatch)
    monkeypatch.setattr(engine, "FUSED_MSE_INIT", False)
    yield SimpleNamespace(engine=engine, seen=seen, monkeypatch=monkeypatch)


def _both(q, x, per_row, engine):
    """((delta, zp) knob off, (delta, zp) knob on, searches of the knob-on call)."""
    off = mc.route(q, x, per_row, fused=False)
    assert engine.MSE_INIT_SEARCHES[0] == 0
    on = mc.route(q, x, per_row, fused=True)
    n = engine.MSE_INIT_SEARCHES[0]
    engine.MSE_INIT_SEARCHES[0] = 0
    return off, on, n


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device \
            and torch.equal(a, b)
    return type(a) is type(b) and a == b


def test_knob_defaults_off_and_is_a_flag(monkeypatch):
    from qdiff import engine
    assert engine._parse_flag(os.environ.get("QDIFF_FUSED_MSE_INIT"), "QDIFF_FUSED_MSE_INIT") == engine.FUSED_MSE_INIT
    if os.environ.get("QDIFF_FUSED_MSE_INIT") is None:
        assert engine.FUSED_MSE_INIT is False
    monkeypatch.setattr(engine, "FUSED_MSE_INIT", False)
    engine.set_fused_mse_init("1")
    assert engine.FUSED_MSE_INIT is True
    engine.set_fused_mse_init(False)
    assert engine.FUSED_MSE_INIT is False
    with pytest.raises(ValueError):
        engine.set_fused_mse_init(2)
    assert not engine.mse_init_device_ok(torch.zeros(1))
    assert engine.MSE_INIT_SEARCHES == [0] or isinstance(engine.MSE_INIT_SEARCHES[0], int)


def test_gate_each_single_miss_keeps_the_composition(emu):
    """Knob off, 'max', fp16, rows not consecutive, a host tensor without the patch: no search, and what today's code returns."""
    w = mc.weights((8, 12), CPU)

    def searches(q, x, per_row, knob=True):
        emu.engine.MSE_INIT_SEARCHES[0] = 0
        got = mc.route(q, x, per_row, fused=knob)
        return emu.engine.MSE_INIT_SEARCHES[0], got

    q = mc.make_quantizer(True, 4, False, False)
    n, on = searches(q, w, True)
    assert n == 1                                                   # every condition met: the route engages
    n, off = searches(q, w, True, knob=False)
    assert n == 0 and _same(on[0], off[0]) and _same(on[1], off[1])
    qmax = mc.make_quantizer(True, 4, False, False)
    qmax.scale_method = 'max'
    n, got = searches(qmax, w, True)
    assert n == 0 and all(_same(a, b) for a, b in zip(got, searches(qmax, w, True, knob=False)[1]))
    # fp16 (the product converts before it initialises; a direct call keeps the composition)
    a = mc.activations((2, 6, 4, 4), CPU)
    qa = mc.make_quantizer(False, 8, False, False)
    n, got = searches(qa, a.half(), False)
    assert n == 0 and got[0].dtype == torch.float16
    # rows that are not consecutive in memory: the per-channel loop runs, and its scalar searches stay on the composition too
    wt = mc.weights((12, 8), CPU).t()
    n, got = searches(q, wt, True)
    assert n == 0 and all(_same(a, b) for a, b in zip(got, searches(q, wt, True, knob=False)[1]))
    at = a.permute(0, 2, 3, 1)
    n, got = searches(qa, at, False)
    assert n == 0 and all(_same(a_, b_) for a_, b_ in zip(got, searches(qa, at, False, knob=False)[1]))
    # a device the kernel does not run on
    emu.monkeypatch.setattr(emu.engine, "mse_init_device_ok", lambda t: t.is_cuda)
    assert searches(q, w, True)[0] == 0 and searches(qa, a, False)[0] == 0
    emu.monkeypatch.setattr(emu.engine, "mse_init_device_ok", lambda t: True)
    assert searches(qa, a, False)[0] == 1


@pytest.mark.parametrize("shape,bits,sym", [((48, 32, 3, 3), 4, False), ((40, 96), 8, False), ((16, 3, 3, 3), 4, False),
                                            ((40, 96), 8, True)])
def test_channelwise_returns_what_the_composition_returns(emu, shape, bits, sym):
    w = mc.weights(shape, CPU)
    q = mc.make_quantizer(True, bits, sym, False)
    off, on, n = _both(q, w, True, emu.engine)
    assert n == 1 and emu.seen[-1] == (shape[0], w[0].numel(), w[0].numel(), True)
    want = (-1,) + (1,) * (w.dim() - 1)
    for a, b in zip(on, off):
        assert a.shape == b.shape == torch.empty(shape[0]).view(want).shape and a.dtype == b.dtype == torch.float32
    same = (on[0] == off[0]).flatten() & (on[1] == off[1]).flatten()
    assert same.float().mean() >= 0.98                              # the cap of test_vectorised_mse_range_search_matches_the_per_channel_loop
    ratio = on[0].flatten()[~same] / off[0].flatten()[~same]
    assert ((ratio - 1).abs() <= 0.015).all()


def test_split_weight_slices_are_read_in_place(emu):
    w = mc.weights((32, 48, 3, 3), CPU)
    q = mc.make_quantizer(True, 4, False, False)
    for view, cols in ((w[:, :16], 16 * 9), (w[:, 16:], 32 * 9)):
        off, on, n = _both(q, view, True, emu.engine)
        assert n == 1 and emu.seen[-1] == (32, cols, 48 * 9, True)  # the strides the entry saw: the parent's rows
        assert on[0].shape == (32, 1, 1, 1) and _same(on[0], off[0]) and _same(on[1], off[1])


@pytest.mark.parametrize("always_zero,bits", [(False, 8), (False, 4), (True, 16), (True, 8)])
@pytest.mark.parametrize("leaf_param", [False, True])
def test_scalar_returns_types_shapes_and_the_range(emu, always_zero, bits, leaf_param):
    x = mc.softmax_probs((4, 16, 24), CPU) if always_zero else mc.activations((2, 32, 8, 8), CPU)
    qs = [mc.make_quantizer(False, bits, False, always_zero, leaf_param=leaf_param) for _ in range(2)]
    off = mc.route(qs[0], x, False, fused=False)
    emu.engine.MSE_INIT_SEARCHES[0] = 0
    on = mc.route(qs[1], x, False, fused=True)
    assert emu.engine.MSE_INIT_SEARCHES[0] == 1 and emu.seen[-1] == (1, x.numel(), x.numel(), False)
    assert _same(on[0], off[0]) and on[0].dim() == 0
    assert _same(on[1], off[1]) and ((on[1] == 0 and type(on[1]) is int) if always_zero else on[1].dim() == 0)
    if leaf_param:
        assert _same(qs[1].x_min, qs[0].x_min) and _same(qs[1].x_max, qs[0].x_max) and qs[1].x_min.dim() == 0
    q3 = mc.make_quantizer(False, bits, False, always_zero, leaf_param=leaf_param)
    emu.engine.set_fused_mse_init(True)
    try:
        y = q3(x)                                                   # the whole quantiser: ensure_init wraps delta as it always did
    finally:
        emu.engine.set_fused_mse_init(False)
    assert q3.inited and isinstance(q3.delta, nn.Parameter) == leaf_param and y.shape == x.shape


def test_activation_channel_slices_are_strided_rows(emu):
    x = mc.activations((2, 48, 7, 7), CPU)
    q = mc.make_quantizer(False, 8, False, False, leaf_param=True)
    for view, c in ((x[:, :21], 21), (x[:, 21:], 27)):
        off, on, n = _both(q, view, False, emu.engine)
        assert n == 1 and emu.seen[-1] == (2, c * 49, 48 * 49, False)
        assert _same(on[0], off[0]) and _same(on[1], off[1])
        assert float(q.x_min) == float(view.min()) and float(q.x_max) == float(view.max())


def test_nothing_picked_in_both_forms(emu):
    """index = -1: a channel-wise row holds (0, 0) as the composition's; the scalar form hands the call to the composition."""
    x = mc.value_edges(CPU)
    q = mc.make_quantizer(True, 4, False, False)
    q_vec = mc.make_quantizer(True, 4, False, False)
    on = mc.route(q, x, True, fused=True)
    assert emu.engine.MSE_INIT_SEARCHES[0] == 1
    want = q_vec._init_mse_channelwise(x)
    assert on[0].shape == (8, 1) and torch.equal(on[0], want[0]) and torch.equal(on[1], want[1])
    dead = [0, 1, 5, 6]                                             # zeros, constant, NaN, +inf
    assert (on[0].flatten()[dead] == 0).all() and (on[1].flatten()[dead] == 0).all() and (on[0].flatten()[[2, 3, 4, 7]] > 0).all()
    d, z, mn, mx, idx, sc = mse_init_emulator.mse_search(x, True, 4, 16, False, want_scores=True)
    assert idx.tolist()[0] == idx.tolist()[1] == idx.tolist()[5] == idx.tolist()[6] == -1 and torch.isnan(mn[5]) and torch.isnan(mx[5])
    qs = mc.make_quantizer(False, 8, False, False, leaf_param=True)
    for view in (x[1:2], x[0:1], x):                                # constant, zeros, a NaN somewhere
        emu.engine.MSE_INIT_SEARCHES[0] = 0
        got = mc.route(qs, view, False, fused=True)
        assert emu.engine.MSE_INIT_SEARCHES[0] == 1 and got == (None, None) == mc.route(qs, view, False, fused=False)


@pytest.mark.parametrize("name", ["w16x3x3x3_4b_misaligned", "w5x1031_8b_odd_long", "w32x48x3x3_second_half", "w40x96_8b_symmetric",
                                  "a3x5x7x11_odd_tail", "a2x48x7x7_second_slice", "softmax8x64x77_8b", "edges_4b_rows",
                                  "edges_8b_whole"])
def test_the_judge_passes_the_emulated_entry(emu, name):
    """The comparison the GPU tests hold the kernel to, on the emulation: the header's letter meets it."""
    case = {c[0]: c for c in mc.CASES}[name]
    fig = mc.judge(case[1](CPU), *case[2:], label="host " + name)
    assert fig["picks_differ"] == 0


def test_tiny_model_weight_quantisers_initialise_through_the_route(emu):
    off, n_off = mc.tiny_model_weight_init(CPU, fused=False)
    on, n_on = mc.tiny_model_weight_init(CPU, fused=True)
    assert n_off == 0 and n_on == len(on) == len(off) and any(k.endswith(".1") for k in on), "no split half among the quantisers"
    for k in off:
        assert _same(on[k][0], off[k][0]) and _same(on[k][1], off[k][1]), k


def test_prototypes_argtypes_exports_and_abi():
    from qdiff import hip
    lib = hip.load()
    assert lib.qd_abi_version() == 20
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qdiff_hip.h")).read(), flags=re.S)
    i64, i32, vp, f32 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    kinds = {"ptr": vp, "int": i32, "int64_t": i64, "float": f32}
    for name in ("qd_mse_search_form", "qd_mse_search_ws_bytes", "qd_mse_search"):
        assert name in hip.EXPORTS and hasattr(lib, name)
        args = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", h, flags=re.S).group(1)
        want = [kinds["ptr" if "*" in a else a.replace("const", "").split()[0]] for a in args.split(",")]
        assert list(getattr(lib, name).argtypes) == want, name
    assert len(lib.qd_mse_search.argtypes) == 18 and lib.qd_mse_search_ws_bytes.restype is i64
    doc = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()
    assert "quant_layer.py:138-140" in doc and ":162-177" in doc and ":183-190" in doc
    # the one rule of the launch form, and the workspace it implies
    assert [lib.qd_mse_search_form(r, c, p) for r, c, p in ((48, 288, 1), (5, 512, 1), (5, 513, 1), (2, 23040, 1), (2, 100, 0),
                                                            (1, 1 << 24, 0), (0, 4, 1))] == [0, 0, 1, 1, 2, 2, -1]
    assert [mse_init_emulator.mse_search_form(r, c, p) for r, c, p in ((48, 288, 1), (5, 513, 1), (2, 100, 0), (0, 4, 1))] == [0, 1, 2, -1]
    assert lib.qd_mse_search_ws_bytes(48, 288, 1, 80) == 0
    assert lib.qd_mse_search_ws_bytes(1, 2048 * 3 + 1, 0, 80) == 4 * (2 * 4 + 80 * 8)          # 4 blocks: min / max + 80 doubles each
    assert lib.qd_mse_search_ws_bytes(1, 1 << 30, 0, 80) == 2048 * (2 * 4 + 80 * 8)            # capped at 2048 blocks


def test_entry_refuses_bad_arguments_before_any_launch():
    """On fake pointers, without a GPU, through qd_last_error."""
    from qdiff import hip
    lib = hip.load()
    P = 0x10000

    def call(x=P, rows=4, cols=8, ldx=8, per_row=1, factors=P, n_cand=80, levels=15, qmax=15, az=0, delta=P, zp=P, x_min=P,
             x_max=P, index=P, scores=None, ws=None):
        rc = lib.qd_mse_search(x, rows, cols, ldx, per_row, factors, n_cand, levels, qmax, az, delta, zp, x_min, x_max, index,
                               scores, ws, None)
        return rc, lib.qd_last_error().decode()

    for kw in (dict(x=None), dict(factors=None), dict(delta=None), dict(zp=None), dict(x_min=None), dict(x_max=None), dict(index=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "qd_mse_search" in msg and "null pointer" in msg, (kw, msg)
    for kw in (dict(n_cand=0), dict(n_cand=81)):
        rc, msg = call(**kw)
        assert rc != 0 and "n_cand" in msg, (kw, msg)
    for kw in (dict(rows=0), dict(cols=0)):
        rc, msg = call(**kw)
        assert rc != 0 and "empty tensor" in msg, (kw, msg)
    rc, msg = call(rows=1 << 20, cols=1 << 11, ldx=1 << 11)
    assert rc != 0 and "31-bit" in msg
    rc, msg = call(ldx=7)
    assert rc != 0 and "row stride" in msg
    rc, msg = call(levels=0)
    assert rc != 0 and "levels" in msg
    rc, msg = call(x=P + 2)
    assert rc != 0 and "4-byte aligned" in msg
    rc, msg = call(per_row=0, ws=None)
    assert rc != 0 and "workspace" in msg
    rc, msg = call(per_row=0, ws=P + 8)
    assert rc != 0 and "workspace" in msg
