"""The output epilogue of the fused int8 attention (csrc/attn_i8.hip, attn_write_rows) on every kernel family that leaves through
it, with both outputs: fp32 rows and the int8 input rows of the consuming Linear.

The launcher is called directly on buffers the test owns: out8 with ldo8 = H*d + 16, out with ldo = H*d + 4, both pre-filled with
a sentinel and eight rows longer than B*T.  For every form, T in {1, 33, 129} (a wave with one live row; a full wave plus a
ragged one; more than one block of 128 queries) and both restorations (32-bit, and the 64-bit one that dw = 2^-23 selects):
  * the fp32 entry and the out8 entry run on the same operand bytes, and EVERY byte must equal
    clamp(rint(out / delta) + zp, qmin, qmax) - off, evaluated in numpy float32 (correctly rounded division, half-even rint),
    for a hand-written qparams vector {delta, zp, rinv, 0} (exact division in the kernel, delta not a power of two, zp = 119,
    a grid that clips both ends) and for a power-of-two delta that qd_make_qparams certifies as fast;
  * pad columns [H*d, ld) and the rows behind B*T still hold the sentinel in both buffers;
  * the fp32 rows meet the integer oracle's row criteria (attn_exact_cases.check_rows: bit for bit on decided rows) and are
    bit-equal to the twin form that tests/test_attention_exact_gpu.py declares byte-equal (table / constant-operand key term,
    register-fed / LDS-staged).
The lo-only P.V launch takes blocks whose probability codes all stay below 256: such rows cannot be had under dw = 2^-23 with
512 keys, so that form is run with the 32-bit restoration only.  Which of the two P.V launches a block takes is decided on the
device; the cases are built so that the host's exact codes leave no doubt (asserted below).

The transposed-heads epilogue of the integer contraction (O_HTR) on the two-K-group kernel needs no case here:
tests/test_conv_tall_tiles_gpu.py::test_tall_tile_head_layout_epilogues[160-4-256-512-512] runs it (256 blocks, eight K-steps,
512 threads asserted) against qd_quantize_heads of the fp32 projection.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import attn_exact_cases as A

pytestmark = pytest.mark.gpu

SENT8, SENT32 = -77, 12345.0
B, H = 2, 2

# name -> (d, S, wbits, (pipe_mode, ktab, lean), twin config or None, rows)
FORMS = {
    "attn_kernel_d32": (32, 45, 16, (2, 1, 1), None, "dense"),
    "attn_kernel_d80": (80, 45, 16, (2, 1, 1), None, "dense"),
    "attn_kernel_d160": (160, 45, 16, (2, 1, 1), None, "dense"),
    "lean_d40_S77_table": (40, 77, 16, (0, 1, 1), (0, 0, 1), "dense"),
    "lean_d40_S77_const": (40, 77, 16, (0, 0, 1), (3, 1, 1), "dense"),
    "lean_d24_p8": (24, 45, 8, (0, 1, 1), (3, 1, 1), "dense"),
    "lds_d40_S512_hilo": (40, 512, 16, (2, 1, 1), (0, 1, 1), "dense"),
    "lds_d40_S512_lo": (40, 512, 16, (2, 1, 1), (0, 1, 1), "diffuse"),
}
CASES = [(f, T, r) for f in FORMS for T in (1, 33, 129) for r in ("r32", "r64") if not (f == "lds_d40_S512_lo" and r == "r64")]
_BUILT = {}


def _case(form, T, rest):
    key = (form, T, rest)
    if key in _BUILT:
        return _BUILT[key]
    d, S, wbits, _, _, rows = FORMS[form]
    seed = sorted(FORMS).index(form) * 8 + T % 7
    if rest == "r64":
        # equal scores (q~ = 0) under dw = 2^-23: code_sum * 255 > 2e9, the 64-bit restoration (codes clamp where 1/S is off the grid)
        spec = A.Spec(f"{form}_T{T}_r64", B, H, T, S, d, wbits=wbits, dw=2.0 ** -23, zv=0, cs=2.0 ** -9, seed=seed)
        qc = np.full((spec.BH, T, d), spec.zq, dtype=np.int64)
        kc = spec.rng.integers(0, 256, size=(spec.BH, S, d))
        vc = spec.rng.integers(0, 256, size=(spec.BH, S, d))
    else:
        dw = 2.0 ** -(8 if wbits == 8 else (16 if S >= 512 else 12))
        spec = A.Spec(f"{form}_T{T}_r32", B, H, T, S, d, wbits=wbits, dw=dw, cs=2.0 ** -9 / (2 if d > 128 else 1), seed=seed)
        amp = max(6, int(24 * (32.0 / d) ** 0.5))
        qc, kc, vc = A.dense(spec, 1, 4) if rows == "diffuse" else A.dense(spec, amp, amp)
    c = A.finish(spec, qc, kc, vc, A.all_rows(spec))
    _BUILT[key] = c
    return c


def _launch(hip, engine, ap, ops, c, out=None, out8=None, oq=None, grid=None):
    q8, k8, v8, vsum = ops
    T, S, d = c.T, c.S, c.d
    hip.attn_i8(q8, k8, v8, vsum, B * H, H, T, S, d, engine.pad32(T), engine.pad32(S), engine.pad32(d), ap.prm, ap.wbits, ap.wmin,
                ap.wmax, ap.asym, out, out.stride(0) if out is not None else 0, out8=out8, oq_params=oq, oq_grid=grid)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form,T,rest", CASES, ids=["%s-T%d-%s" % k for k in CASES])
def test_attention_epilogue(cuda, form, T, rest):
    from qdiff import engine, hip
    d, S, wbits, cfg, twin, rows = FORMS[form]
    c = _case(form, T, rest)
    C = H * d
    if form.startswith("lds") and rest == "r32":
        # exact codes of the decided keys: every block of 128 queries of a "hilo" case holds a code well above 255, no code of a
        # "lo" case comes near it
        top = (c.ev.pu * c.ev.dec_keys).reshape(B * H, T, S).max(-1)
        if rows == "diffuse":
            assert top.max() < 200
        else:
            assert all(top[:, i:i + 128].max(-1).min() >= 512 for i in range(0, T, 128))
    ns = lambda a: NS(**a)
    ap = engine.build_attn_plan(ns(c.aq_q), ns(c.aq_k), ns(c.aq_v), ns(c.aq_w), c.scale, c.prescale, cuda)
    Tp, Sp, dp = engine.pad32(T), engine.pad32(S), engine.pad32(d)
    q8 = torch.zeros((B * H, Tp, dp), dtype=torch.int8, device=cuda)
    k8 = torch.zeros((B * H, Sp, dp), dtype=torch.int8, device=cuda)
    v8 = torch.zeros((B * H, dp, Sp), dtype=torch.int8, device=cuda)
    vsum = torch.zeros((B * H, dp), dtype=torch.int32, device=cuda)
    for which, (t, L, buf) in enumerate(((c.q, T, q8), (c.k, S, k8), (c.v, S, v8))):
        engine.heads_from_float(ap, which, t.to(cuda), B, L, H, d, (L * C, C, d, 1), buf, vsum)
    ops = (q8, k8, v8, vsum)
    ldo, ldo8, nrow = C + 4, C + 16, B * T + 8
    grid = engine.act_grid(8, False)                               # codes [0, 255], stored code - 128
    try:
        hip.attn_config(pipe_mode=cfg[0], ktab=cfg[1], lean=cfg[2])
        out = torch.full((nrow, ldo), SENT32, dtype=torch.float32, device=cuda)
        _launch(hip, engine, ap, ops, c, out=out)
        o = out.cpu().numpy()
        assert (o[B * T:] == SENT32).all() and (o[:, C:] == SENT32).all(), "fp32 pad columns / rows behind B*T"
        live = np.ascontiguousarray(o[:B * T, :C])
        assert np.isfinite(live).all()
        amax = float(np.abs(live).max())
        assert amax > 0
        # the two quantisers: exact division with hand-written parameters; a certified power-of-two delta
        dslow = np.float32(amax / 150.0 * 1.013)                   # codes would span ~ +-148 around zp = 119: both ends clip
        qslow = torch.tensor([float(dslow), 119.0, float(np.float32(1.0) / dslow), 0.0], dtype=torch.float32, device=cuda)
        dfast = np.float32(2.0 ** int(np.ceil(np.log2(amax / 120.0))))
        qfast = hip.make_qparams(torch.tensor(float(dfast), device=cuda), torch.tensor(128.0, device=cuda))
        torch.cuda.synchronize()
        assert float(qfast[3]) != 0.0, "qd_make_qparams must certify a power-of-two delta"
        for tag, oq, delta, zp in (("fast0", qslow, dslow, 119.0), ("fast1", qfast, dfast, 128.0)):
            out8 = torch.full((nrow, ldo8), SENT8, dtype=torch.int8, device=cuda)
            _launch(hip, engine, ap, ops, c, out8=out8, oq=oq, grid=grid)
            g8 = out8.cpu().numpy()
            assert (g8[B * T:] == SENT8).all() and (g8[:, C:] == SENT8).all(), (tag, "int8 pad columns / rows behind B*T")
            want = np.clip(np.rint(live / np.float32(delta)) + np.float32(zp), np.float32(grid.qmin), np.float32(grid.qmax)) - np.float32(grid.off)
            assert want.dtype == np.float32
            bad = np.argwhere(g8[:B * T, :C].astype(np.float32) != want)
            assert len(bad) == 0, (tag, len(bad), bad[:4].tolist())
        if twin is not None:
            hip.attn_config(pipe_mode=twin[0], ktab=twin[1], lean=twin[2])
            out2 = torch.full((nrow, ldo), SENT32, dtype=torch.float32, device=cuda)
            _launch(hip, engine, ap, ops, c, out=out2)
            assert torch.equal(out, out2), "fp32 rows differ between byte-equal forms"
    finally:
        hip.attn_config(pipe_mode=2, ktab=1, lean=1)
    got = live.reshape(B, T, H, d).transpose(0, 2, 1, 3).reshape(B * H, T, d)
    ok, rep = A.check_rows(c, got)
    assert ok, (form, T, rest, vars(rep))
