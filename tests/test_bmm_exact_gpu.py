"""The standalone attention matmuls (csrc/bmm_i8.hip) against the integer oracle of tests/bmm_exact_cases.py, bit for bit:
(a) every case through hip.bmm_qk_i8 / hip.bmm_pv_i8 on hand-built operand bytes with poisoned pads, outputs pre-filled with a
NaN sentinel that must survive everywhere outside the written window; (b) engine.qk_matmul_int / engine.smv_matmul_int on float
"bct" inputs that reproduce a subset of the codes (through qd_quantize_heads, strided and split inputs included); (c) the gates of
QuantQKMatMul / QuantSMVMatMul on the device; (d) what the launchers refuse, by the error text, with nothing launched.

Figures of the run that introduced this file: profiles/bmm_exact.txt."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import bmm_exact_cases as C
from test_bmm_exact_host import GATE_CASES, run_gate_case

pytestmark = pytest.mark.gpu


# ---- (a) ABI level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_bmm_abi_exact(cuda, name, record_property):
    from qdiff import hip
    c = C.all_cases()[name]
    prm = c.prm.to(cuda)
    for kind in c.kinds:
        full, win = C.out_buffers(c, kind, cuda)
        if kind == "qk":
            hip.bmm_qk_i8(c.q8.to(cuda), c.k8.to(cuda), c.BH, c.T, c.S, c.d, c.Tpad, c.Spad, c.dpad, prm, win)
        else:
            w = C.w_view(c, c.w_full.to(cuda))
            assert (w.stride(1), w.stride(0)) == (c.lay.ldw, c.lay.w_rows * c.lay.ldw)
            hip.bmm_pv_i8(w, c.vt.to(cuda), c.vsum.to(cuda), c.BH, c.T, c.S, c.d, c.Spad, c.dpad, prm, c.wbits, c.wmin, c.wmax, win)
        torch.cuda.synchronize()
        ok, rep = C.check_output(c, kind, full)
        I = c.I_qk if kind == "qk" else c.I_pv
        print(f"bmm_exact {name} {kind} DT={c.DT} P{c.wbits if kind == 'pv' else 0} compared {rep.compared} mismatches {rep.mismatches} "
              f"spilled {rep.spilled} max|I| {int(np.abs(I).max())} above2^24 {int((np.abs(I) > 2 ** 24).sum())} first {rep.first}")
        record_property(kind + "_compared", rep.compared)
        assert ok, (name, kind, vars(rep))


# ---- (b) producer level -------------------------------------------------------------------------------------------------------
def _float_inputs(c):
    """q, k, v as fp32 "bct" [BH, d, L] whose quantisation gives the case's stored bytes."""
    if c.floats is not None:
        return tuple(torch.from_numpy(c.floats[key]) for key in "qkv")
    out = []
    for stored, z, delta in ((c.qs, c.zq, c.dq), (c.ks, c.zk, c.dk), (c.vs, c.zv, c.dv)):
        x = (stored - z).astype(np.float64) * delta                     # (code - zp) * delta, exact for a power-of-two delta
        assert C.is_pow2(delta) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
        out.append(torch.from_numpy(np.ascontiguousarray(np.swapaxes(x.astype(np.float32), 1, 2))))
    return tuple(out)


def _same_bits(got, want):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", C.PRODUCER_NAMES)
def test_bmm_from_float_inputs_exact(cuda, name):
    from qdiff import engine
    c = C.all_cases()[name]
    q, k, v = _float_inputs(c)
    if name.endswith("_split"):
        # the way QKVAttentionLegacy hands them over: slices of one [BH, 3 * ch, L] tensor (batch stride 3 * ch * L)
        q, k, v = torch.cat([q, k, v], dim=1).to(cuda).split(c.d, dim=1)
        assert q.stride(0) == 3 * c.d * c.T and k.data_ptr() != q.data_ptr()
    else:
        q, k, v = q.to(cuda), k.to(cuda), v.to(cuda)
    aq = lambda delta, z: NS(delta=torch.tensor(delta, dtype=torch.float32), zero_point=z + 128, n_bits=8, sym=False)
    got = engine.qk_matmul_int(aq(c.dq, c.zq), aq(c.dk, c.zk), q, k, c.scale)
    torch.cuda.synchronize()
    assert _same_bits(got, c.want_qk), name
    aq_w = NS(delta=torch.tensor(c.dw, dtype=torch.float32), zero_point=c.zpw, n_bits=c.w_nbits, sym=c.w_sym)
    w = C.w_view(c).contiguous()
    wide = torch.full((c.BH, c.T + 2, c.S + 3), float("nan"))
    wide[:, :c.T, :c.S] = w
    forms = dict(contiguous=w.to(cuda), padded_rows=wide.to(cuda)[:, :c.T, :c.S], transposed=w.permute(0, 2, 1).contiguous().to(cuda).permute(0, 2, 1))
    assert forms["padded_rows"].stride(2) == 1 and not forms["padded_rows"].is_contiguous() and forms["transposed"].stride(2) != 1
    for form, weight in forms.items():
        got = engine.smv_matmul_int(aq_w, aq(c.dv, c.zv), weight, v)
        torch.cuda.synchronize()
        assert _same_bits(got, c.want_pv), (name, form)


# ---- (c) module level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,sm_bits,qk_int,smv_int", GATE_CASES)
def test_gates_on_the_device(cuda, monkeypatch, d, sm_bits, qk_int, smv_int):
    run_gate_case(monkeypatch, d, sm_bits, qk_int, smv_int, device=cuda)


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------
def _full_buffers(cuda, BH, T, S, d, dpad=None):
    """Every operand at its full declared size, so that a missing refusal is a failed assertion and never a stray read."""
    Tpad, Spad, dpad = C.pad32(T), C.pad32(S), dpad or C.pad32(d)
    z8 = lambda *shape: torch.zeros(shape, dtype=torch.int8, device=cuda)
    prm = torch.tensor([2.0 ** -8, 0, 0, 2.0 ** -8, 0, 2.0 ** -12, 0, 0], dtype=torch.float32, device=cuda)
    return NS(q8=z8(BH, Tpad, dpad), k8=z8(BH, Spad, dpad), vt=z8(BH, dpad, Spad), vsum=torch.zeros((BH, dpad), dtype=torch.int32, device=cuda),
              w=torch.zeros((BH, T, S), device=cuda), prm=prm, Tpad=Tpad, Spad=Spad, dpad=dpad, qk=C.sentinel((BH, T, S), cuda), pv=C.sentinel((BH, d, T), cuda))


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t.view(torch.int32) == C.SENTINEL_BITS).all())


def test_head_dim_pad_224_is_refused(cuda):
    from qdiff import hip
    BH, T, S, d = 1, 5, 7, 200
    b = _full_buffers(cuda, BH, T, S, d)
    assert b.dpad == 224
    with pytest.raises(hip.HipEngineError, match="qd_bmm_qk_i8: head dim pad 224 unsupported"):
        hip.bmm_qk_i8(b.q8, b.k8, BH, T, S, d, b.Tpad, b.Spad, b.dpad, b.prm, b.qk)
    with pytest.raises(hip.HipEngineError, match="qd_bmm_pv_i8: head dim pad 224 unsupported"):
        hip.bmm_pv_i8(b.w, b.vt, b.vsum, BH, T, S, d, b.Spad, b.dpad, b.prm, 8, 0, 255, b.pv)
    assert _untouched(b.qk) and _untouched(b.pv)


def test_twelve_bit_probabilities_are_refused(cuda):
    from qdiff import hip
    BH, T, S, d = 1, 5, 7, 40
    b = _full_buffers(cuda, BH, T, S, d)
    with pytest.raises(hip.HipEngineError, match="probability bits must be 8 or 16 \\(got 12\\)"):
        hip.bmm_pv_i8(b.w, b.vt, b.vsum, BH, T, S, d, b.Spad, b.dpad, b.prm, 12, 0, 4095, b.pv)
    with pytest.raises(hip.HipEngineError, match="wider than 8 bits"):
        hip.bmm_pv_i8(b.w, b.vt, b.vsum, BH, T, S, d, b.Spad, b.dpad, b.prm, 8, 0, 256, b.pv)
    assert _untouched(b.pv)


@pytest.mark.parametrize("wbits,wmin,wmax,S,text", [(16, 0, 65535, 32769, "overflow the int32 code sum"),
                                                   (16, -32768, 32767, 32769, "overflow the int32 code sum"),
                                                   (8, 0, 255, 131072, "S < 131072")])
def test_key_counts_beyond_the_int32_bounds_are_refused(cuda, wbits, wmin, wmax, S, text):
    """S * (wmax - wmin) >= 2^31 wraps the per-query code sum, S * 2^14 >= 2^31 the byte accumulators (include/qdiff_hip.h)."""
    from qdiff import hip
    BH, T, d = 1, 1, 4
    b = _full_buffers(cuda, BH, T, S, d)
    with pytest.raises(hip.HipEngineError, match=text):
        hip.bmm_pv_i8(b.w, b.vt, b.vsum, BH, T, S, d, b.Spad, b.dpad, b.prm, wbits, wmin, wmax, b.pv)
    assert _untouched(b.pv)
    # the largest key count each grid still takes is not refused by the predicate of the modules' gates either way round
    from qdiff import engine
    aq_w = NS(n_bits=wbits, sym=wmin < 0)
    assert not engine.bmm_shape_ok(d, aq_w, S) and engine.bmm_shape_ok(d, aq_w, S - 1)
