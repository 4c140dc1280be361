"""Split-K of the weights-only contraction (qd_conv2d_wq_h16 with a workspace, engine.WEIGHT_ONLY_SPLITK) on
the GPU.

Reference: the fp64 contraction of the same rounded operands as tests/test_weight_only_gpu.py (_contraction_ref).  Bound: that
file's bound plus nsplit * 2^-23 * S[m][n] — per slice one rounding of the scaled partial and one of the addition in the
finalise, each at most 2^-24 * S (S: the contraction on absolute values).  A row bias joins bias and residual in the `extra`
term, as in tests/test_weight_only_fused_gpu.py.

Every kernel case is one small launch with its own workspace: need + GUARD bytes, all 0xFF (NaN as fp32) before the launch.  A
finite, in-bound output shows that every partial the finalise read was written; the guard bytes show that nothing past
nsplit * M * Cout * 4 was.  The slice count is forced with hip.wq_h16_config.
"""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

from golden_util import load_fixture
from test_weight_only_gpu import BOUNDS, _contraction_ref, _fp64_conv, _layer, _metrics, _resume, _run, _wquant

pytestmark = pytest.mark.gpu

GUARD = 4096
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@pytest.fixture
def knobs():
    """The four host knobs and the library's slice count, restored afterwards."""
    from qdiff import engine, hip
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_SPLITK, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE)
    hip.wq_h16_config(-1)
    yield engine
    engine.set_weight_only_kernel(prev[0])
    engine.set_weight_only_splitk(prev[1])
    engine.set_weight_only_fusion(prev[2])
    engine.set_weight_only_fusion_wide(prev[3])
    hip.wq_h16_config(-1)


class Launcher:
    """Stands in for hip.conv2d_wq_h16 under engine.wonly_forward: the same descriptor, launched with a workspace of this
    test's own.  ws_bytes: None = no workspace; "need" = what the library asks for; an int = that many bytes (a non-positive
    int is relative to `need`)."""

    def __init__(self, dev, ws_bytes):
        self.dev, self.ws_bytes, self.need, self.ws = dev, ws_bytes, None, None

    def __call__(self, c, act_dtype):
        from qdiff import hip
        lib = hip.load()
        d = hip._conv_desc(c)
        self.need = int(lib.qd_conv2d_wq_h16_splitk_ws_bytes(ctypes.byref(d)))
        if self.ws_bytes is not None:
            n = self.need if self.ws_bytes == "need" else (self.ws_bytes if self.ws_bytes > 0 else self.need + self.ws_bytes)
            self.ws = torch.full((max(n, self.need) + GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
            d.splitk_ws, d.splitk_ws_bytes = self.ws.data_ptr(), n
        hip._check(lib.qd_conv2d_wq_h16(ctypes.byref(d), hip._H16[act_dtype], hip._stream()), "qd_conv2d_wq_h16")


def _setup(dev, kind, wbits, act, out_dtype, split, B, Cin, Cout, H, W, k, stride, has_bias, has_res, has_rb, seed):
    """Operands on the host and on the device, and the arguments of engine.wonly_forward."""
    from qdiff import engine
    g = torch.Generator().manual_seed(seed)
    x, w = _layer(kind, B, Cin, Cout, H, W, k, stride, g)
    pad = k // 2 if kind == "conv2d" else 0
    bounds = [(0, Cin)] if not split else [(0, split), (split, Cin)]
    qs = [_wquant(w[:, a:b], wbits, "range", g) for a, b in bounds]
    bias = torch.randn(Cout, generator=g) if has_bias else None
    pack = engine.pack_module_weights(w.to(dev), [NS(**{**vars(q), "delta": q.delta.to(dev), "zero_point": q.zero_point.to(dev)})
                                                   for q in qs], split or 0)
    kh, kw = (k, k) if kind == "conv2d" else (1, 1)
    plan = engine.build_wonly_plan(pack, kh, kw, stride if kind == "conv2d" else 1, pad, None if bias is None else bias.to(dev), act)
    assert plan is not None
    xd = x.to(dev)
    if kind == "conv2d":
        sb, sc, sh, sw = xd.stride()
        xh = engine.wonly_rows(xd, plan, B, Cin, H * W, (sb, sc, sw))
        Ho, Wo = engine.conv_out_hw(H, W, plan)
        geo = (B, H, W, Ho, Wo)
    else:                                                        # linear on [B, W, Cin] tokens: B samples of W rows
        rows = xd.reshape(-1, Cin)
        xh = engine.wonly_rows(rows, plan, 1, Cin, rows.shape[0], (0, 1, rows.stride(0)))
        geo = (B, 1, W, 1, W)
    M = geo[0] * geo[3] * geo[4]
    res = torch.randn(M, Cout, generator=g).to(out_dtype) if has_res else None
    rb = torch.randn(B, Cout + 8, generator=g) * 2 if has_rb else None          # rows wider than Cout: ld_rowbias is honoured
    kwargs = dict(out_dtype=out_dtype, residual=None if res is None else res.to(dev),
                  rowbias=None if rb is None else rb.to(dev)[:, :Cout])
    return NS(kind=kind, x=x, w=w, qs=qs, bounds=bounds, bias=bias, res=res, rb=rb, act=act, out_dtype=out_dtype, stride=stride,
              pad=pad, plan=plan, xh=xh, geo=geo, M=M, Cout=Cout, B=B, kwargs=kwargs)


def _launch(s, monkeypatch, ws_bytes):
    """One engine.wonly_forward through a Launcher: (output, launcher)."""
    from qdiff import engine, hip
    la = Launcher(s.xh.device, ws_bytes)
    monkeypatch.setattr(hip, "conv2d_wq_h16", la)
    out = engine.wonly_forward(s.plan, s.xh, *s.geo, **s.kwargs)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return out, la


def _bound(s, nsplit):
    """(fp64 reference rows, tolerance): tests/test_weight_only_gpu.py's bound, |rowbias| in its `extra` term, plus
    nsplit * 2^-23 * S."""
    ref, tol, wd = _contraction_ref(s.kind, s.x, s.w, s.qs, s.bounds, s.bias, s.res, s.act, F32, s.stride, s.pad)
    xr = s.x.to(s.act).double().abs()
    S = _fp64_conv(s.kind, xr, wd.abs(), s.stride, s.pad)
    S = S.permute(0, 2, 3, 1).reshape(s.M, s.Cout) if s.kind == "conv2d" else S.reshape(s.M, s.Cout)
    if s.rb is not None:
        rbm = s.rb[:, :s.Cout].double().repeat_interleave(s.M // s.B, dim=0)
        tol = tol + 2.0 ** -22 * (rbm.abs() + (ref + rbm).abs() - ref.abs())
        ref = ref + rbm
    if s.out_dtype == F16:
        tol = tol * (1 + 2.0 ** -11) + 2.0 ** -11 * ref.abs() + 2.0 ** -24
    return ref, tol + nsplit * 2.0 ** -23 * S


def _case(dev, monkeypatch, nsplit, *args, want=None):
    """Force `nsplit` slices, launch once on a NaN-filled workspace, check the slice count the library chose (`want`, default
    nsplit), the fp64 bound, that every partial was written and that nothing past them was."""
    from qdiff import hip
    s = _setup(dev, *args)
    hip.wq_h16_config(nsplit)
    out, la = _launch(s, monkeypatch, "need")
    want = nsplit if want is None else want
    assert la.need == want * s.M * s.Cout * 4, f"library asks for {la.need} bytes, {want} slices are {want * s.M * s.Cout * 4}"
    ref, tol = _bound(s, want)
    err = (out.double().cpu() - ref).abs()
    worst = (err / tol).max().item()
    print(f"\n{args}: nsplit {want}, error {worst:.3g} x the bound (max |err| {err.max().item():.3e})")
    assert torch.isfinite(out).all(), "an unwritten (NaN) partial reached the output"
    assert worst <= 1.0, f"{args} nsplit={want}: error {worst:.3g} x the bound (max |err| {err.max().item():.3e})"
    ws = la.ws.cpu()
    assert torch.isfinite(ws[:la.need].view(torch.float32)).all(), "a partial inside nsplit * M * Cout was not written"
    assert (ws[la.need:] == 0xFF).all(), "bytes past nsplit * M * Cout * 4 were written"
    return s, out


# kind, wbits, act, out_dtype, split, B, Cin, Cout, H, W, k, stride, has_bias, has_res, has_rb, seed
def _geometry(wbits, act, out_dtype, has_bias, has_res, seed):
    """Linear, M = 70, Cin = 320 split at 128 (segment 0 = 2 K-steps, segment 1 = 3), Cout = 130 (scalar finalise)."""
    return ("linear", wbits, act, out_dtype, 128, 1, 320, 130, 1, 70, 1, 1, has_bias, has_res, False, seed)


@pytest.mark.parametrize("nsplit,variant", [(2, (4, F16, F32, True, False, 11)), (3, (8, BF16, F16, False, True, 12)),
                                            (5, (4, BF16, F32, True, True, 13)), (3, (8, F16, F32, True, False, 14))],
                         ids=["n2-straddle", "n3-whole-segments", "n5-boundary-on-edge", "n3-w8-fp16"])
def test_slices_against_the_segment_boundary(cuda, knobs, monkeypatch, nsplit, variant):
    """5 K-steps, boundary after step 2.  2 slices: [0,3) straddles, [3,5) in segment 1.  3 slices: [0,2) is segment 0 and ends
    at the boundary, [2,4) and [4,5) lie in segment 1.  5 slices: one step each, the boundary on a slice edge."""
    _case(cuda, monkeypatch, nsplit, *_geometry(*variant))


def _taps(i, stride, split):
    wbits, act, out_dtype = [(4, F16, F32), (8, BF16, F16), (4, BF16, F32), (8, F16, F16)][i % 4]
    return ("conv2d", wbits, act, out_dtype, split, 2, 130, 48, 5, 7, 3, stride, i % 2 == 0, i % 3 != 0, i % 2 == 1, 20 + i)


TAPS = [(n, stride, split) for split in (0, 64) for stride in (1, 2) for n in (4, 27)]


@pytest.mark.parametrize("i", range(len(TAPS)), ids=[f"n{n}-s{st}-split{sp}" for n, st, sp in TAPS])
def test_uneven_slices_over_taps(cuda, knobs, monkeypatch, i):
    """3 x 3 convolution, B = 2, 5 x 7, Cin = 130 (3 K-steps per tap, 27 in all; split at 64: 9 + 18), Cout = 48.  4 slices hold
    7, 7, 7, 6 steps and start inside a tap; 27 slices hold one step each.  Odd cases carry a row bias (B = 2)."""
    n, stride, split = TAPS[i]
    _case(cuda, monkeypatch, n, *_taps(i, stride, split))


TAILS = [  # M, Cout, Cin, split, wbits, act, out_dtype, has_bias, has_res
    (130, 1, 72, 0, 4, F16, F32, True, True),        # second M block of 2 rows; one column: scalar finalise
    (1, 20, 100, 0, 8, F16, F16, True, False),       # one row; 16-byte finalise with 8-byte fp16 stores
    (130, 260, 100, 0, 4, BF16, F32, False, True),   # three column blocks, the last 4 wide; 16-byte finalise
    (1, 260, 72, 40, 8, BF16, F16, True, True),      # split shortcut with one K-step per segment
    (130, 20, 72, 0, 4, F16, F16, False, False),
]


@pytest.mark.parametrize("i", range(len(TAILS)), ids=[f"M{t[0]}-N{t[1]}-K{t[2]}" for t in TAILS])
def test_m_n_and_k_tails(cuda, knobs, monkeypatch, i):
    """Two K-steps (the second a K tail), one per slice."""
    M, Cout, Cin, split, wbits, act, out_dtype, has_bias, has_res = TAILS[i]
    _case(cuda, monkeypatch, 2, "linear", wbits, act, out_dtype, split, 1, Cin, Cout, 1, M, 1, 1, has_bias, has_res, False, 40 + i)


def test_forced_count_is_clamped_to_the_k_steps(cuda, knobs, monkeypatch):
    """Two K-steps, 7 slices asked: two slices run."""
    _case(cuda, monkeypatch, 7, "linear", 4, F16, F32, 0, 1, 100, 36, 1, 9, 1, 1, True, False, False, 50, want=2)


def test_same_launch_twice_is_bit_identical(cuda, knobs, monkeypatch):
    s, out = _case(cuda, monkeypatch, 4, *_taps(1, 1, 64))
    out2, _ = _launch(s, monkeypatch, "need")
    assert torch.equal(out, out2)


def test_nothing_leaks_without_workspace_config_or_knob(cuda, knobs, monkeypatch):
    """Bit-equal to a launch without a workspace: qd_wq_h16_config(0) with a workspace attached, a workspace one byte too
    small (left untouched), and the host path with the knob off; with the knob on the host attaches the scratch and counts."""
    from qdiff import engine, hip
    s = _setup(cuda, *_taps(0, 1, 64))
    hip.wq_h16_config(3)
    base, la = _launch(s, monkeypatch, None)
    assert la.need == 3 * s.M * s.Cout * 4
    hip.wq_h16_config(0)
    out, la = _launch(s, monkeypatch, 1 << 20)
    assert la.need == 0 and torch.equal(out, base) and (la.ws == 0xFF).all()
    hip.wq_h16_config(3)
    out, la = _launch(s, monkeypatch, -1)
    assert torch.equal(out, base) and (la.ws == 0xFF).all()
    engine.WONLY_SPLITK[0] = 0
    engine.set_weight_only_splitk(False)
    out = engine.wonly_forward(s.plan, s.xh, *s.geo, **s.kwargs)
    assert torch.equal(out, base) and engine.WONLY_SPLITK[0] == 0
    engine.set_weight_only_splitk(True)
    out = engine.wonly_forward(s.plan, s.xh, *s.geo, **s.kwargs)
    torch.cuda.synchronize()
    assert engine.WONLY_SPLITK[0] == 1
    ref, tol = _bound(s, 3)
    assert ((out.double().cpu() - ref).abs() <= tol).all()
    hip.wq_h16_config(0)
    out = engine.wonly_forward(s.plan, s.xh, *s.geo, **s.kwargs)
    assert torch.equal(out, base) and engine.WONLY_SPLITK[0] == 1


# ---- whole models ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sd_tiny", "ldm_tiny"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_models_with_the_knob_on(cuda, knobs, name, dt):
    """State (True, False) against the reference's weights-only golden `out_w` within tests/test_weight_only_gpu.py's BOUNDS:
    once under the library's policy, once with two slices forced so that the tiny layers split at all."""
    from qdiff import hip
    engine = knobs
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    engine.set_weight_only_kernel(dt)
    engine.set_weight_only_splitk(True)
    tol, cmin = BOUNDS[dt]
    for force in (-1, 2):
        hip.wq_h16_config(force)
        engine.WONLY_SPLITK[0] = 0
        y = _run(qnn, fx, cuda)
        d, cos = _metrics(y, fx["out_w"])
        print(f"\n[{name}] {dt} split-K config({force}): {engine.WONLY_SPLITK[0]} split launches, {d:.3e} of range, cosine {cos:.7f}")
        assert d <= tol and cos >= cmin
    assert engine.WONLY_SPLITK[0] > 0


def test_fused_routes_split_too(cuda, knobs):
    """sd_tiny with QDIFF_WEIGHT_ONLY_FUSE and _FUSE_WIDE on: the row-bias and residual launches of the fused routes go through
    wonly_forward and split; the GEGLU epilogue launches do not.  Bounds: BOUNDS, as the fused tests use."""
    from qdiff import hip
    engine = knobs
    fx = load_fixture("model_sd_tiny.pt")
    qnn = _resume(fx, cuda)
    qnn.set_quant_state(True, False)
    engine.set_weight_only_kernel(F16)
    engine.set_weight_only_fusion(True)
    engine.set_weight_only_fusion_wide(True)
    engine.set_weight_only_splitk(True)
    hip.wq_h16_config(2)
    engine.WONLY_SPLITK[0] = 0
    engine.WONLY_GEGLU_EPI[0] = 0
    y = _run(qnn, fx, cuda)
    d, cos = _metrics(y, fx["out_w"])
    print(f"\n[sd_tiny] fused + wide, split-K config(2): {engine.WONLY_SPLITK[0]} split launches, {engine.WONLY_GEGLU_EPI[0]} GEGLU "
          f"epilogues, {d:.3e} of range, cosine {cos:.7f}")
    tol, cmin = BOUNDS[F16]
    assert engine.WONLY_SPLITK[0] > 0 and engine.WONLY_GEGLU_EPI[0] > 0
    assert d <= tol and cos >= cmin
