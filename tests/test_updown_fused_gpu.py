"""qd_groupnorm_resample_silu_quant (engine.FUSE_UPDOWN) on the GPU against the float64 torch composition GroupNorm -> SiLU ->
avg_pool2d / nearest 2x -> oracle.quant_ref.uaq_codes, its refusals, and `ldm_updown_tiny` on the route.  Codes: none off by more than
one, at most 0.1 % off by one (test_hip_kernels.test_groupnorm_silu_quant), which the fp32 composition on the CPU must itself meet.
Skip rows: nearest 2x is a copy; the 2x2 average is two levels of fp32 additions and an exact * 0.25: <= 2 * 2^-24 * max|x|, asserted at twice that."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from golden_util import load_fixture
from oracle import quant_ref as R

pytestmark = pytest.mark.gpu
EPS = 1e-5
SHAPES = [(3, 32, 32, 2, 2, True, False),        # (B, C, groups, H, W, SiLU, part_in): one window, one channel per group
          (2, 48, 16, 6, 10, True, False),       # W / 2 odd, groups of three channels straddle the 16-channel chunks
          (2, 64, 32, 16, 16, True, True),       # two 128-row chunks of part_in
          (2, 32, 8, 4, 6, False, False)]        # no SiLU


def _mismatch(got, want):
    diff = (got.long() - want.long()).abs()
    return diff.max().item(), (diff > 0).double().mean().item()


def _case(shape, resample):
    """One case on the CPU: x, gamma, beta, fp32 delta, zero point, float64 codes and float64 raw rows, resampled."""
    B, C, G, H, W, silu, _ = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    pool = (lambda t: F.avg_pool2d(t, 2)) if resample == 1 else (lambda t: F.interpolate(t, scale_factor=2, mode="nearest"))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    def compose(dt):
        y = F.group_norm(x.to(dt), G, gamma.to(dt), beta.to(dt), EPS)
        return pool(y * torch.sigmoid(y) if silu else y)
    y64, y32 = compose(torch.float64), compose(torch.float32)
    d, z = R.uaq_init_scale(y32, 8, False, False, "max")
    d = torch.tensor(float(d), dtype=torch.float32)                   # the delta the kernel reads
    want = R.uaq_codes(y64, float(d), z, 8, False)
    mx, frac = _mismatch(R.uaq_codes(y32, d, z, 8, False), want)
    assert mx <= 1 and frac <= 1e-3, "the inputs put the fp32 composition itself outside the cap: another seed / scale"
    return x, gamma, beta, float(d), float(z), rows(want) - 128, rows(pool(x.double()))


@pytest.mark.parametrize("resample", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-G%d-%dx%d-silu%d-part%d" % s)
def test_kernel_matches_the_float64_composition(cuda, shape, resample):
    from qdiff import engine, hip
    B, C, G, H, W, silu, from_part = shape
    x, gamma, beta, d, z, want, xr64 = _case(shape, resample)
    M, ldx, ldo, ldr = B * H * W, C + 4, C + 16, C + 8
    Mq, Mr = (M // 4, M // 4) if resample == 1 else (M, 4 * M)
    xb = torch.full((M, ldx), 9e9, device=cuda)                       # ldx, ldo, ldr > C; one sentinel row on each side of both outputs
    xb[:, :C] = x.to(cuda).permute(0, 2, 3, 1).reshape(M, C)
    part = None
    if from_part:                                                     # as the convolution's epilogue writes it: per 128-row chunk
        r = xb[:, :C].view(B, H * W // 128, 128, C)
        part = torch.stack([r.sum(2), (r * r).sum(2)], dim=-1).contiguous()
    out, xr = torch.full((Mq + 2, ldo), 0x55, dtype=torch.int8, device=cuda), torch.full((Mr + 2, ldr), -777.0, device=cuda)
    ws = torch.empty(hip.groupnorm_ws_bytes(B, C, H * W), dtype=torch.uint8, device=cuda)
    hip.groupnorm_resample_silu_quant(xb, B, H, W, C, ldx, G, EPS, gamma.to(cuda), beta.to(cuda), silu, resample,
                                      torch.tensor([d, z], device=cuda), engine.act_grid(8, False), out[1:], ldo, ws,
                                      xr=xr[1:], ldr=ldr, part=part)
    out, xr = out.cpu(), xr.cpu()
    assert (out[[0, -1]] == 0x55).all() and (out[:, C:] == 0x55).all()         # sentinel rows and pad columns are never touched
    assert (xr[[0, -1]] == -777.0).all() and (xr[:, C:] == -777.0).all()
    codes, got = out[1:-1, :C], xr[1:-1, :C].double()
    if resample == 2:                                                 # the small map: the convolution's gather replicates it
        codes = codes.view(B, H, 1, W, 1, C).expand(B, H, 2, W, 2, C).reshape(-1, C)
    mx, frac = _mismatch(codes, want)
    assert mx <= 1 and frac <= 1e-3
    assert torch.equal(got, xr64) if resample == 2 else (got - xr64).abs().max().item() <= 2.0 ** -22 * x.abs().max().item()


@pytest.mark.parametrize("H,C,resample", [(5, 32, 1), (4, 32, 3), (4, 24, 1)], ids=["odd-H", "resample-3", "C-24"])
def test_refusals_write_nothing(cuda, H, C, resample):
    from qdiff import hip
    lib = hip.load()
    x = torch.randn(H * 4, 32, device=cuda)
    out, xr = torch.full((4 * H * 4, 32), 0x55, dtype=torch.int8, device=cuda), torch.full((4 * H * 4, 32), -777.0, device=cuda)
    ws = torch.empty(hip.groupnorm_ws_bytes(1, 32, H * 4), dtype=torch.uint8, device=cuda)
    qp = hip.make_qparams(torch.tensor(0.05, device=cuda), torch.tensor(128.0, device=cuda))
    rc = lib.qd_groupnorm_resample_silu_quant(x.data_ptr(), 1, H, 4, C, 32, 8, EPS, None, None, 1, resample, qp.data_ptr(), 0, 255, 128,
                                              out.data_ptr(), 32, xr.data_ptr(), 32, ws.data_ptr(), None, 0, 0,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"qd_groupnorm_resample_silu_quant" in lib.qd_last_error() and (out == 0x55).all() and (xr == -777.0).all()


def test_updown_model_on_the_fused_route(cuda):
    """Every `updown` block launches the producer once, none with the knob off; the output inside the default route's envelope."""
    from qdiff import engine
    from qdiff.quant_block import QuantResBlock
    from test_engine_models import _assert_envelope, _resume, _run
    fx = load_fixture("model_ldm_updown_tiny.pt")
    qnn = _resume(fx, cuda)
    qnn.enable_hip_graphs(False)                                       # a replay runs no Python: the counter would stand still
    blocks = [m for m in qnn.modules() if isinstance(m, QuantResBlock) and m.updown]
    n_down = sum(hasattr(b.h_upd, "op") for b in blocks)
    prev, count = engine.FUSE_UPDOWN, dict(engine.UPDOWN_FUSED)
    try:
        engine.set_fused_updown(False)
        _run(qnn, fx, cuda)
        assert engine.UPDOWN_FUSED == count
        engine.set_fused_updown(True)
        y = _run(qnn, fx, cuda)
        assert 0 < n_down < len(blocks) and engine.UPDOWN_FUSED == {"down": count["down"] + n_down, "up": count["up"] + len(blocks) - n_down}
    finally:
        engine.set_fused_updown(prev)
    _assert_envelope("ldm_updown_tiny", y, fx)
