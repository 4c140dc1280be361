"""Host checks of the exact standalone-matmul cases (tests/bmm_exact_cases.py): the case list, the int32 bounds and the coverage
conditions the GPU test relies on, the emulated qd_bmm_qk_i8 / qd_bmm_pv_i8 against the same oracle bit for bit, and the gates
of QuantQKMatMul / QuantSMVMatMul: what the launchers refuse keeps the reference's composition."""
import numpy as np
import pytest
import torch

import abi_emulator
import bmm_exact_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


def test_case_list_is_complete(cases):
    assert sorted(C.CASE_NAMES) == sorted(cases) and len(set(C.CASE_NAMES)) == len(C.CASE_NAMES)
    assert set(C.PRODUCER_NAMES) <= set(cases)
    assert len(C.CASE_NAMES) <= 200


def test_every_instantiation_and_shape_is_reached(cases):
    qk = {c.DT for c in cases.values() if "qk" in c.kinds}
    pv = {(c.DT, c.wbits) for c in cases.values() if "pv" in c.kinds}
    assert qk == {1, 2, 3, 4, 5, 8}
    assert pv == {(dt, b) for dt in (1, 2, 3, 4, 5, 8) for b in (8, 16)}
    for dt in (1, 2, 3, 4, 5, 8):                                       # a full and a ragged d-pad of every DT
        ds = {c.d for c in cases.values() if c.DT == dt and c.name.startswith("inst_")}
        assert any(d % 32 == 0 for d in ds) and any(d % 32 for d in ds), dt
    g = [c for c in cases.values() if c.name.startswith("geom_")]
    assert {c.T for c in g} == {1, 31, 32, 33, 129, 160} and {c.S for c in g} == {1, 31, 32, 33, 77, 97}
    assert {(129, 97), (1, 1)} <= {(c.T, c.S) for c in g}
    assert {c.BH for c in g} == {1, 3, 5}
    big = cases["geom_T129_S97"].lay
    assert big.qk_ldo > 97 and big.qk_rows > 129 and big.pv_ldo > 129 and big.pv_rows > 40
    wide = cases["geom_T31_S77"]
    assert wide.lay.ldw > wide.S and wide.lay.w_rows > wide.T and torch.isnan(wide.w_full[:, :, wide.S:]).all()
    assert torch.isnan(wide.w_full[:, wide.T:]).all() and torch.isfinite(C.w_view(wide)).all()
    assert all(c.T <= 160 and c.S <= 97 and c.d <= 256 and c.BH <= 5 for c in cases.values())
    zp = {(c.d, c.zq, c.zk) for c in cases.values() if c.name.startswith("zp_")}
    assert zp == {(d, a, b) for d in (40, 256) for a in C.ZP_SET for b in C.ZP_SET}
    assert {(c.zv, c.wbits) for c in cases.values() if c.name.startswith("zv")} == {(z, b) for z in (-128, 0, 127) for b in (8, 16)}
    assert {(c.grid, c.zpw) for c in cases.values() if c.name.startswith("grid_")} == {(g_, z) for g_ in C.GRIDS for z in (0, 3, g_[1], g_[2])}


def test_pads_are_poisoned(cases):
    inv = lambda Spad: torch.argsort(abi_emulator._perm_index(Spad))
    for c in cases.values():
        assert all(t.is_contiguous() for t in (c.q8, c.k8, c.vt, c.vsum, c.prm, c.w_full))      # the kernels address raw memory
        assert c.q8.shape == (c.BH, c.Tpad, c.dpad) and c.k8.shape == (c.BH, c.Spad, c.dpad) and c.vt.shape == (c.BH, c.dpad, c.Spad)
        assert np.array_equal(c.q8[:, :c.T, :c.d].numpy(), c.qs) and np.array_equal(c.k8[:, :c.S, :c.d].numpy(), c.ks)
        assert not c.q8[:, :c.T, c.d:].any() and not c.k8[:, :, c.d:].any()             # d-pad columns of live rows / of every k row
        nat = c.vt[:, :, inv(c.Spad)]
        assert np.array_equal(nat[:, :c.d, :c.S].permute(0, 2, 1).numpy(), c.vs)
        assert np.array_equal(c.vsum[:, :c.d].numpy(), c.vs.sum(1)) and (c.vsum[:, c.d:] == C.POISON_SUM).all()
        if c.Tpad - c.T >= 4:
            assert c.q8[:, c.T:].any()
        if c.Spad - c.S >= 4:
            assert c.k8[:, c.S:, :c.d].any() and nat[:, :c.d, c.S:].any()
        if c.dpad - c.d >= 4:
            assert nat[:, c.d:, :].any()


def test_int32_bounds_hold(cases):
    """Every |I| and every 32-bit intermediate of the kernels stays below 2^31."""
    for c in cases.values():
        for what, v in C.int32_bounds(c).items():
            assert 0 <= v < 2 ** 31, (c.name, what, v)
    assert C.int32_bounds(cases["sat_qk_neg_d256"])["qk_I"] == 16646400 == C.int32_bounds(cases["sat_qk_pos_d256"])["qk_I"]
    assert (cases["sat_qk_mixed_d256"].I_qk[0] == -16646400).all()
    s = cases["sat_pv_p16"]
    assert (s.u == 65535).all() and np.abs(s.I_pv).max() == 97 * 65535 * 255 == C.int32_bounds(s)["pv_I"]
    assert C.int32_bounds(s)["pv_code_sum"] == 97 * 65535


def test_rounding_coverage(cases):
    """Conversion rounding: outputs with |I| > 2^24 whose integer is NOT an fp32 number exist; product rounding: cs (QK) or
    dw*dv (PV) is no power of two in at least half of the cases."""
    inexact = 0
    big = 0
    for c in cases.values():
        if "pv" in c.kinds:
            over = np.abs(c.I_pv) > 2 ** 24
            big += int(over.sum())
            inexact += int((c.I_pv.astype(np.float32).astype(np.int64) != c.I_pv).sum())
    assert big > 10000 and inexact > 1000
    flags = [not (C.is_pow2(c.cs) if "qk" in c.kinds else True) or not (C.is_pow2(c.oscale) if "pv" in c.kinds else True) for c in cases.values()]
    assert sum(flags) * 2 >= len(flags)
    assert not all(flags)                                                # power-of-two scales are there too
    print(f"{len(cases)} cases, {sum(flags)} with a scale that is no power of two; |I| > 2^24: {big} outputs, {inexact} of them not fp32 numbers")


def test_grid_cases_hold_the_rounding_edges(cases):
    for c in (c for c in cases.values() if c.name.startswith("grid_")):
        assert C.is_pow2(c.dw)
        w = C.w_view(c).numpy()
        lo, hi = c.wmin - c.zpw, c.wmax - c.zpw
        for bh in range(c.BH):
            row = lambda key: w[bh, (C.GRID_ROWS[key] + 7 * bh) % c.T].astype(np.float64)
            u = lambda key: c.u[bh, (C.GRID_ROWS[key] + 7 * bh) % c.T]
            assert set(row("zero_one")) == {0.0, 1.0}
            for key, parity in (("ties_even", 0), ("ties_odd", 1)):
                x = row(key) / c.dw
                n = np.floor(x)
                assert (x - n == 0.5).all() and (n % 2 == parity).all() and n.min() == lo + (lo % 2 != parity) and n.max() >= hi - 2
                assert ((u(key) - c.zpw) % 2 == 0).all() and (np.abs(u(key) - c.zpw - x) == 0.5).all()       # half to even, unclamped
            assert (row("above") / c.dw > hi + 0.5).all() and (u("above") == c.wmax).all()
            assert (u("to_wmin") == c.wmin).all() and (row("to_wmin") / c.dw < lo).any() and (row("to_wmin") / c.dw > lo).any()
            assert abs(row("softmax").sum() - 1) < 1e-5 and (row("softmax") > 0).all()
        assert c.u.min() == c.wmin and c.u.max() == c.wmax


def _run_emulated(c, kind):
    full, win = C.out_buffers(c, kind)
    if kind == "qk":
        abi_emulator.bmm_qk_i8(c.q8, c.k8, c.BH, c.T, c.S, c.d, c.Tpad, c.Spad, c.dpad, c.prm, win)
    else:
        abi_emulator.bmm_pv_i8(C.w_view(c), c.vt, c.vsum, c.BH, c.T, c.S, c.d, c.Spad, c.dpad, c.prm, c.wbits, c.wmin, c.wmax, win)
    return full


def test_emulator_reproduces_every_case_bit_for_bit(cases):
    for c in cases.values():
        for kind in c.kinds:
            ok, rep = C.check_output(c, kind, _run_emulated(c, kind))
            assert ok, (c.name, kind, vars(rep))


def test_criterion_sees_an_integer_off_by_one_and_a_spill(cases):
    """What 2e-6 of range lets through: one integer off by one at |I| ~ 6e5, and a write outside the window."""
    c = cases["geom_T129_S97"]
    full = _run_emulated(c, "qk")
    i = np.unravel_index(np.abs(c.I_qk).argmax(), c.I_qk.shape)
    off = full.clone()
    off[i] = float(np.float32(c.I_qk[i] + 1) * np.float32(c.cs))
    ok, rep = C.check_output(c, "qk", off)
    assert not ok and rep.mismatches == 1 and rep.first["I"] == c.I_qk[i]
    c = cases["geom_T31_S77"]
    full = _run_emulated(c, "pv")
    i = np.unravel_index(np.abs(np.abs(c.I_pv) - 1.0e6).argmin(), c.I_pv.shape)
    assert 6e5 < abs(int(c.I_pv[i])) < 2 ** 24
    off = full.clone()
    off[i] = float(np.float32(c.I_pv[i] + 1) * np.float32(c.oscale))
    assert abs(float(off[i]) - float(full[i])) <= 2e-6 * float(c.want_pv.abs().max())      # the old tolerance passes it
    ok, rep = C.check_output(c, "pv", off)
    assert not ok and rep.mismatches == 1 and rep.first["element"] == tuple(int(x) for x in i)
    c = cases["geom_T129_S97"]
    spill = _run_emulated(c, "pv")
    spill[0, 0, c.T] = 0.0
    ok, rep = C.check_output(c, "pv", spill)
    assert not ok and rep.spilled == 1 and rep.mismatches == 0


def test_emulator_refuses_what_the_library_refuses(cases):
    from qdiff import hip
    c = cases["inst_d40_p8"]
    _, win = C.out_buffers(c, "qk")
    with pytest.raises(hip.HipEngineError, match="head dim pad 224 unsupported"):
        abi_emulator.bmm_qk_i8(c.q8, c.k8, c.BH, c.T, c.S, 200, c.Tpad, c.Spad, 224, c.prm, win)
    _, win = C.out_buffers(c, "pv")
    pv = lambda **kw: abi_emulator.bmm_pv_i8(C.w_view(c), c.vt, c.vsum, c.BH, c.T, kw.get("S", c.S), c.d, c.Spad, kw.get("dpad", c.dpad), c.prm,
                                             kw.get("wbits", 8), kw.get("wmin", 0), kw.get("wmax", 255), win)
    for kw, text in ((dict(dpad=192), "head dim pad 192 unsupported"), (dict(wbits=12, wmax=4095), "must be 8 or 16"),
                     (dict(wmax=256), "wider than 8 bits"), (dict(wbits=16, wmax=65535, S=32769), "overflows"), (dict(S=131072), "overflows")):
        with pytest.raises(hip.HipEngineError, match=text):
            pv(**kw)


# ---- the gates of the drop-in modules ---------------------------------------------------------------------------------------
def gate_modules(d, sm_bits, seed=0, device="cpu"):
    """QuantQKMatMul / QuantSMVMatMul with initialised quantisers and inputs [BH, d, L] for them."""
    from qdiff.quant_block import QuantQKMatMul, QuantSMVMatMul
    g = torch.Generator().manual_seed(seed)
    aq = dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True)
    qk, smv = QuantQKMatMul(aq), QuantSMVMatMul(aq, sm_abit=sm_bits)
    qk.scale = d ** -0.25
    BH, T, S = 2, 9, 13
    q, k, v = (torch.randn(BH, d, L, generator=g) for L in (T, S, S))
    w = torch.softmax(torch.randn(BH, T, S, generator=g) * 2, dim=-1)
    for quantizer, delta, zp in ((qk.act_quantizer_q, 0.023, 131.0), (qk.act_quantizer_k, 0.019, 120.0), (smv.act_quantizer_v, 0.027, 125.0),
                                 (smv.act_quantizer_w, 1.0 / (2 ** sm_bits - 1), 0.0)):
        quantizer.delta = torch.nn.Parameter(torch.tensor(delta, device=device))
        quantizer.zero_point = torch.tensor(zp, device=device)
        quantizer.inited = True
    qk.use_act_quant = smv.use_act_quant = True
    return qk.to(device), smv.to(device), tuple(t.to(device) for t in (q, k, v, w))


GATE_CASES = [(192, 8, False, False), (200, 8, False, False), (40, 12, True, False), (40, 8, True, True), (256, 16, True, True), (40, 4, True, True)]


def run_gate_case(monkeypatch, d, sm_bits, qk_int, smv_int, device="cpu"):
    """Module outputs against the module's own non-engine branch; the integer path is taken exactly where expected."""
    from qdiff import engine, hip
    calls = []
    for name in ("bmm_qk_i8", "bmm_pv_i8"):
        inner = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _n=name, _f=inner: (calls.append(_n), _f(*a))[1])
    qk, smv, (q, k, v, w) = gate_modules(d, sm_bits, device=device)
    with torch.no_grad():
        got_s, got_o = qk(q, k), smv(w, v)
        assert calls == ["bmm_qk_i8"] * qk_int + ["bmm_pv_i8"] * smv_int, calls
        with engine.simulation():
            ref_s, ref_o = qk(q, k), smv(w, v)
        assert len(calls) == qk_int + smv_int
    for got, ref, integer in ((got_s, ref_s, qk_int), (got_o, ref_o, smv_int)):
        if integer:
            assert (got - ref).abs().max() <= 1e-4 * ref.abs().max()
        else:
            assert torch.equal(got, ref)


@pytest.mark.parametrize("d,sm_bits,qk_int,smv_int", GATE_CASES)
def test_gates_keep_the_composition_where_the_launchers_refuse(monkeypatch, d, sm_bits, qk_int, smv_int):
    abi_emulator.install(monkeypatch)
    run_gate_case(monkeypatch, d, sm_bits, qk_int, smv_int)


def test_gate_predicate():
    from types import SimpleNamespace as NS
    from qdiff import engine
    ok = [c for c in range(4, 300, 4) if engine.bmm_shape_ok(c)]
    assert ok == [c for c in range(4, 300, 4) if c <= 160 or 224 < c <= 256]
    w = lambda bits, sym=False: NS(n_bits=bits, sym=sym)
    assert [b for b in range(2, 18) if engine.bmm_shape_ok(40, w(b))] == [2, 3, 4, 5, 6, 7, 8, 16]
    assert engine.bmm_shape_ok(40, w(16), 32768) and not engine.bmm_shape_ok(40, w(16), 32769)
    assert engine.bmm_shape_ok(40, w(16, True), 32768) and not engine.bmm_shape_ok(40, w(16, True), 32769)
    assert engine.bmm_shape_ok(40, w(8), 131071) and not engine.bmm_shape_ok(40, w(8), 131072)
    assert not engine.bmm_shape_ok(192, w(8), 77)
