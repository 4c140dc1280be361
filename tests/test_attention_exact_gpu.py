"""Fused int8 attention (csrc/attn_i8.hip) against the integer oracle, row by row: the cases of tests/attn_exact_cases.py on every
launch form eligible for their shape.  Decided rows (every probability code known: see the margin derived in attn_exact_cases)
must equal float32(I) * float32(dw*dv) — bit for bit where dw and dv are powers of two, within 1 fp32 ulp otherwise; rows with
undecided keys stay within dw*dv * sum_undecided |v_j - zv| + 1 ulp.  No output is exempt.  Bytes: the lean and LDS-staged
forms (key term from the table, from constant-operand MFMAs or none) evaluate the same float expressions in the same order and
must return the same bytes on EVERY row, and so must the float entry, run on the first of them.  Head dims of the lean family
are also run on attn_kernel (lean = 0), a form beyond the lean family's own: its softmax is a different fp32 computation (a
running maximum per half-wave, rescales), so on a key within m_j of a tie it may take the other neighbour — it is held to the
same row criteria and to the same bytes as the other forms on every decided row.  Operand bytes come from engine.heads_from_float (the production producer: V^T permutation, vsum) and are read back
against the expected codes.

Pads.  include/qdiff_hip.h requires the pad bytes of k to be zero for qd_attn_keyterm and says qd_quantize_heads writes every
pad as zero; qd_attn_i8 itself needs q.k over the d-pad columns to vanish and nothing else.  After producing the operands the
test overwrites with random bytes: q rows [T, Tpad), k rows [S, Spad) (their d-pad columns stay zero), the V^T columns of the keys
[S, Spad) (permuted inside the ragged tile like every key) in every row, V^T rows [d, dpad), and vsum[d:dpad].  The d-pad columns
of live q / k rows are left alone.

Figures of the run that introduced this file (MI355X; decided rows / rows summed over cases and forms; worst error / tolerance on
rows with undecided keys; details in profiles/attn_exact.txt): attn_kernel 14090/14410, 0.034; lean 34908/35868, 0.038;
LDS-staged 11432/11752, 0.038; float entry 14090/14410, 0.038.  No output missed its criterion; the undecided rows are those of
dense_long_4096 (none decided, 199 undecided keys per row) and a few of the saturated d = 80 cases.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import attn_exact_cases as A
from test_hip_kernels import _aq, _weight_quantizer

pytestmark = pytest.mark.gpu

# names are listed statically so that collection builds nothing (test_case_list_is_complete holds the list to the builder)
CASE_NAMES = (["geom_S%d_T129_d40" % S for S in A.GEOM_S] + ["geom_S%d_T%d_d40" % (S, T) for S in (33, 77) for T in (1, 31, 33)]
              + ["form_d%d_%s_p%d" % (d, q, w) for d in (32, 64, 96, 128, 160, 256, 24, 40, 80) for q in ("asym", "sym") for w in (16, 8)]
              + ["form_d40_scale_prescale", "zq-128_d40", "zq-128_d32", "zq-128_d80"]
              + ["sat_d%d_zq%d_zk%d_zv%d" % (d, z, z, z) for d in (256, 80, 60) for z in (0, 255)] + ["sat_d256_zq0_zk255_zv0"]
              + ["epi_dw2^-24_S160_clamped", "epi_dw2^-23_S256", "epi_dw2^-22_S128_small", "epi_p8_zpw3", "epi_p8_sym_cifar",
                 "bytes_p16", "dynamics_S77", "dense_long_4096", "sparse_long_4096"])
QUANTISED_OUTPUT = ("form_d40_asym_p16", "form_d64_asym_p8", "bytes_p16", "sat_d256_zq0_zk0_zv0")


def test_case_list_is_complete():
    assert sorted(CASE_NAMES) == sorted(A.all_cases())


def forms_of(d, asym):
    """(family, pipe_mode, ktab, lean, form4) of every launch form that takes head dim d; form4 = what qd_attn_i8_form must answer
    under those knobs: (0 attn_kernel / 1 lean / 2 LDS-staged, DT, per-key term mode — q_asym for attn_kernel —, launches)."""
    DT, kt = (d + 31) // 32, 2 if asym else 0
    dense = (0, DT, 1 if asym else 0, 1)
    if d % 32 and d < 96:
        L = 3 if d >= 64 else 1
        out = [("lean_kt2" if asym else "lean_kt0", 0, 1, L, (1, DT, kt, 1))]
        if asym:
            out.append(("lean_kt1", 0, 0, L, (1, DT, 1, 1)))
        if d < 64:
            out.append(("lds_kt2" if asym else "lds_kt0", 3, 1, L, (2, DT, kt, 3)))
            if asym:
                out.append(("lean_kt1_pipe3", 3, 0, L, (1, DT, 1, 1)))             # no table: the LDS path hands over to the register-fed kernel
        out.append(("attn_kernel", 2, 1, 0, dense))
        return out
    return [("attn_kernel", 2, 1, 1, dense)]


def _vt_pad_columns(S):
    """Columns of V^T that hold the keys [S, Spad): inside a 32-key tile key j sits in slot 16 * (bit 2 of j) + (j & 3) + 4 * (j >> 3)
    (the MFMA C layout of the transposed scores)."""
    base = (S // 32) * 32
    return [base + 16 * ((j >> 2) & 1) + (j & 3) + 4 * (j >> 3) for j in range(S % 32, 32)] if S % 32 else []


def _rows(out, c):
    return out.float().cpu().view(c.B, c.T, c.H, c.d).permute(0, 2, 1, 3).reshape(c.B * c.H, c.T, c.d).numpy()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_attention_exact_rows(cuda, name, record_property):
    from qdiff import engine, hip
    c = A.all_cases()[name]
    B, H, T, S, d = c.B, c.H, c.T, c.S, c.d
    C = H * d
    ns = lambda a: NS(**a)
    ap = engine.build_attn_plan(ns(c.aq_q), ns(c.aq_k), ns(c.aq_v), ns(c.aq_w), c.scale, c.prescale, cuda)
    Tp, Sp, dp = engine.pad32(T), engine.pad32(S), engine.pad32(d)
    q8 = torch.zeros((B * H, Tp, dp), dtype=torch.int8, device=cuda)
    k8 = torch.zeros((B * H, Sp, dp), dtype=torch.int8, device=cuda)
    v8 = torch.zeros((B * H, dp, Sp), dtype=torch.int8, device=cuda)
    vsum = torch.zeros((B * H, dp), dtype=torch.int32, device=cuda)
    for which, (t, L, buf) in enumerate(((c.q, T, q8), (c.k, S, k8), (c.v, S, v8))):
        engine.heads_from_float(ap, which, t.to(cuda), B, L, H, d, (L * C, C, d, 1), buf, vsum)
    torch.cuda.synchronize()
    # the operand codes survived the device quantiser (stored byte = code - off)
    off = 0 if c.spec.qsym else 128
    assert np.array_equal(q8.cpu().numpy()[:, :T, :d].astype(np.int64) + off, c.qc)
    assert np.array_equal(k8.cpu().numpy()[:, :S, :d].astype(np.int64) + off, c.kc)
    assert np.array_equal(vsum.cpu().numpy()[:, :d].astype(np.int64), (c.vc - off).sum(1))
    # pads the contract leaves free (module docstring)
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, generator=g).to(cuda)
    if Tp > T:
        q8[:, T:, :] = rnd(B * H, Tp - T, dp)
    if Sp > S:
        k8[:, S:, :d] = rnd(B * H, Sp - S, d)
        v8[:, :, _vt_pad_columns(S)] = rnd(B * H, dp, Sp - S)
    if dp > d:
        v8[:, d:, :] = rnd(B * H, dp - d, Sp)
        vsum[:, d:] = 123456789
    outs = {}
    rows = torch.empty((B * T, C), dtype=torch.float32, device=cuda)        # the query's output argument: never written
    try:
        for fam, pipe, ktab, lean, form in forms_of(d, ap.asym):
            hip.attn_config(pipe_mode=pipe, ktab=ktab, lean=lean)
            # the kernel this output will be labelled with is the kernel the launcher takes for the call below
            assert hip.attn_i8_form(q8, k8, v8, vsum, B * H, H, T, S, d, Tp, Sp, dp, ap.prm, ap.wbits, ap.wmin, ap.wmax, ap.asym,
                                    rows, rows.stride(0)) == form, (name, fam)
            o = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d)
            torch.cuda.synchronize()
            outs[fam] = o.clone()
        # the float entry (its own operand buffers, zero pads and producer calls) on the first form
        fam, pipe, ktab, lean, _ = forms_of(d, ap.asym)[0]
        hip.attn_config(pipe_mode=pipe, ktab=ktab, lean=lean)
        outs["float_entry"] = engine.attention(ap, c.q.to(cuda), c.k.to(cuda), c.v.to(cuda), B, T, S, H, d,
                                               (T * C, C, d, 1), (S * C, C, d, 1), (S * C, C, d, 1)).clone()
        torch.cuda.synchronize()
        out8 = None
        if name in QUANTISED_OUTPUT:
            hip.attn_config(pipe_mode=2, ktab=1, lean=1)
            do = 2.0 ** int(np.ceil(np.log2(max(float(np.abs(c.want).max()), 1e-30) / 127.0)))
            w = torch.randn(C, C, generator=g) * 0.05
            plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [_weight_quantizer(w, 4, True, g)], 0), [_aq(do, 128)], 1, 1, 1, 0, None)
            out8 = engine.attention_codes(ap, q8, k8, v8, vsum, B, T, S, H, d, out_plan=plan)
            torch.cuda.synchronize()
    finally:
        hip.attn_config(pipe_mode=2, ktab=1, lean=1)
    worst = 0.0
    for fam, o in outs.items():
        assert torch.isfinite(o).all(), fam
        ok, rep = A.check_rows(c, _rows(o, c))
        print(f"{name} {fam}: decided {rep.decided_rows}/{rep.rows} bad_decided {rep.bad_decided} bad_undecided {rep.bad_undecided} "
              f"worst_undecided_ratio {rep.worst_undecided_ratio:.4f} first_bad {rep.first_bad}")
        worst = max(worst, rep.worst_undecided_ratio)
        assert ok, (name, fam, vars(rep))
    record_property("decided_rows", int(c.decided.sum()))
    record_property("rows", int(c.decided.size))
    record_property("worst_undecided_error_over_tolerance", worst)
    ref_fam = next(iter(outs))
    cross = ref_fam != "attn_kernel"                               # attn_kernel as the extra form of a lean head dim (module docstring)
    dec = torch.from_numpy(np.ascontiguousarray(c.decided.reshape(B, H, T).transpose(0, 2, 1))).reshape(B * T, H, 1).to(cuda)
    for fam, o in outs.items():
        if cross and fam == "attn_kernel":
            same = (outs[ref_fam].view(B * T, H, d) == o.view(B * T, H, d)) | ~dec
            assert bool(same.all()), (name, ref_fam, fam, "decided rows")
        else:
            assert torch.equal(outs[ref_fam], o), (name, ref_fam, fam)
    if out8 is not None:
        # int8 input rows of the consuming Linear (delta a power of two, zero point 128): exact off the ties
        x = c.want.astype(np.float64) / do
        lo = np.clip(np.floor(x + 0.5 - 1e-9) + 128, 0, 255) - 128
        hi = np.clip(np.ceil(x - 0.5 + 1e-9) + 128, 0, 255) - 128
        tie = np.abs(x - np.floor(x) - 0.5) <= A.ulp32(c.want) / do
        got8 = out8.cpu().view(B, T, H, d).permute(0, 2, 1, 3).reshape(B * H, T, d).numpy().astype(np.float64)
        dec = np.broadcast_to(c.decided[:, :, None], x.shape)
        exact = np.where(x - np.floor(x) < 0.5, lo, hi)
        assert (got8[dec & ~tie] == exact[dec & ~tie]).all()
        assert ((got8 == lo) | (got8 == hi))[dec & tie].all()
