"""Fused attention for head dims 264 .. 512 (qd_attn_h16_wide: the head dim split across the four waves of a block) and the
first-stage decoder on it (QDIFF_DECODER_ATTN=hip), on the GPU.  Reference: the fp64 attention of the operand-rounded inputs;
bound: the derived per-element bound of tests/test_weight_only_attention_gpu.py, unchanged (it carries d and S, the fixed-order
fp32 sum of the partial score tiles is inside its eps_i term), with u_out = 2^-8 for the bf16 rows that are new here."""
import random

import pytest
import torch

from golden_util import load_fixture
from test_first_stage import _build
from test_first_stage_hip import DECODER_TOL, ENGINE
from test_weight_only_attention_gpu import U, _operands, _reference, _view

pytestmark = pytest.mark.gpu

U_OUT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
OPS = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]


def _run_and_check(q, k, v, B, T, S, H, d, qs, ks, vs, op, out):
    from qdiff import hip
    hip.attn_h16_wide(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op, out)
    torch.cuda.synchronize()
    ref, a, eps, vmax = _reference(q, k, v, B, T, S, H, d, qs, ks, vs, d ** -0.5, op)
    bound = (U[op] + eps + S * 2.0 ** -22 + 2.0 ** -18) * a + S * 2.0 ** -25 * vmax + U_OUT[out.dtype] * ref.abs()
    ratio = ((out.double() - ref).abs() / bound).max().item()
    assert torch.isfinite(out).all() and ratio <= 1.0, f"worst error {ratio:.3f} x the bound"


def _draws(n=12):
    """a seeded subset of the product: every axis is dealt out in full before it repeats, so every value appears"""
    rng = random.Random(20261126)
    axes = dict(d=[264, 384, 392, 512], T=[1, 31, 33], S=[1, 31, 32, 33, 65], H=[1, 2], B=[1, 2], layout=["rows", "qkv", "heads"],
                dt=[torch.float32, torch.float16, torch.bfloat16], op=[torch.float16, torch.bfloat16],
                out=[torch.float32, torch.float16, torch.bfloat16])
    cols = {name: rng.sample((vals * n)[:n], n) for name, vals in axes.items()}
    return [dict({name: cols[name][i] for name in axes}, seed=3000 + i) for i in range(n)]


@pytest.mark.parametrize("c", _draws(), ids=lambda c: f"d{c['d']}_T{c['T']}_S{c['S']}_H{c['H']}_B{c['B']}_{c['layout']}_"
                         f"{str(c['dt'])[6:]}_{str(c['op'])[6:]}_{str(c['out'])[6:]}")
def test_draws_match_fp64_on_rounded_operands(cuda, c):
    B, T, S, H, d = c["B"], c["T"], c["S"], c["H"], c["d"]
    q, k, v, qs, ks, vs = _operands(cuda, c["layout"], B, T, S, H, d, c["dt"], torch.Generator().manual_seed(c["seed"]))
    _run_and_check(q, k, v, B, T, S, H, d, qs, ks, vs, c["op"], torch.empty((B * T, H * d), dtype=c["out"], device=cuda))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("edge", ["dominant_key_in_the_last_tile", "rescale_on_every_tile", "scores_of_magnitude_1e4", "single_key"])
def test_softmax_edges_at_512_channels(cuda, edge, op):
    B, T, H, d = 2, 33, 1, 512
    S = 1 if edge == "single_key" else 97                                          # three full key tiles and one key
    big = 60.0 if edge == "scores_of_magnitude_1e4" else 1.0
    q, k, v, qs, ks, vs = _operands(cuda, "rows", B, T, S, H, d, torch.float32, torch.Generator().manual_seed(12), scale_q=big)
    k.mul_(big)
    if edge == "dominant_key_in_the_last_tile":                                    # every row's maximum moves in the last tile
        mq = q.mean(dim=1)
        k[:, S - 1] = 3.0 * mq / mq.norm(dim=-1, keepdim=True) * d ** 0.5
    if edge == "rescale_on_every_tile":                                            # scores q_i0 * 4j * scale: strictly increasing in j
        q[..., 1:], k[..., 1:] = 0, 0
        q[..., 0] = q[..., 0].abs() + 1
        k[..., 0] = 4.0 * torch.arange(S, device=cuda, dtype=torch.float32)
    if edge == "scores_of_magnitude_1e4":
        sc = torch.einsum("bthd,bshd->bhts", _view(q, B, T, H, d, qs).to(op).double(), _view(k, B, S, H, d, ks).to(op).double())
        assert sc.abs().max().item() * d ** -0.5 > 3e3
    out = torch.empty((B * T, d), dtype=torch.float32, device=cuda)
    _run_and_check(q, k, v, B, T, S, H, d, qs, ks, vs, op, out)
    if edge == "single_key":      # P = 1 exactly; the row sum is exp2 of the fma's residual of s * c2 (|s * c2| < 8: 2^-22) and one ulp
        assert torch.allclose(out, v.to(op).float().expand(B, T, d).reshape(B * T, d), rtol=2.0 ** -20, atol=0)


def test_guard_bytes_and_run_to_run_bits(cuda):
    """ldo > H*d and one spare row past B*T keep their sentinel bit for bit; two runs of one case give the same bits"""
    B, T, S, H, d, pad = 2, 33, 65, 1, 392, 8
    q, k, v, qs, ks, vs = _operands(cuda, "qkv", B, T, S, H, d, torch.float16, torch.Generator().manual_seed(13))
    bufs = [torch.full((B * T + 1, H * d + pad), -1234.0, dtype=torch.bfloat16, device=cuda) for _ in range(2)]
    for buf in bufs:
        _run_and_check(q, k, v, B, T, S, H, d, qs, ks, vs, torch.float16, buf[:B * T, :H * d])
    bits = [buf.view(torch.int16) for buf in bufs]
    sentinel = torch.full((1,), -1234.0, dtype=torch.bfloat16, device=cuda).view(torch.int16)
    assert (bits[0][:, H * d:] == sentinel).all() and (bits[0][B * T:] == sentinel).all() and torch.equal(bits[0], bits[1])


@pytest.fixture
def hip_attention(monkeypatch):
    """the decoder knob on, and the names of the attention wrappers the decode called"""
    from qdiff import first_stage_hip as fh, hip
    calls = []
    for name in ("attn_h16", "attn_h16_wide"):
        monkeypatch.setattr(hip, name, lambda *a, _f=getattr(hip, name), _n=name: (calls.append(_n), _f(*a))[1])
    monkeypatch.setattr(fh, "DECODER_ATTN", "hip")
    return calls


@pytest.mark.parametrize("dtype", OPS)
@pytest.mark.parametrize("name,kind", [("kl_tiny", "kl"), ("vq_tiny", "vq")])
def test_tiny_decoders_with_hip_attention_match_the_reference_golden(cuda, hip_attention, name, kind, dtype):
    from qdiff.arch import first_stage as fs
    case = load_fixture("first_stage.pt")[name]
    out = fs.decode_first_stage(_build(case, kind).to(cuda), case["z"].to(cuda), 1.0, force_not_quantize=True, engine=ENGINE[dtype])
    err = (out.cpu() - case["out"]).abs().max().item() / case["out"].abs().max().item()
    print(f"{name} {dtype}: hip-attention decoder max err {err:.3e} of range, wrappers {hip_attention}")
    assert len(hip_attention) > 0 and err <= DECODER_TOL[dtype], (name, err)


def test_sd_shaped_decode_with_hip_attention(cuda, hip_attention):
    """one SD latent (4 x 64 x 64: 512 channels, 4096 tokens in the mid block; key-derived synthetic weights): the decode on
    qd_attn_h16_wide against the fp32 library decode at the decoder's fp16 bound; its distance to the library-attention decode
    on the same kernels is printed beside it"""
    from qdiff import first_stage_hip as fh, synthetic
    from qdiff.arch import first_stage as fs
    m, _ = fs.sd_v1_first_stage()
    m.load_state_dict({k: synthetic.tensor_for(k, v.shape, seed=0) for k, v in m.state_dict().items()})
    m = m.eval().to(cuda)
    z = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(3)).to(cuda)
    ref = fs.decode_first_stage(m, z, 1.0)
    out = fs.decode_first_stage(m, z, 1.0, engine="hip")
    fh.set_decoder_attention("library")
    lib = fs.decode_first_stage(m, z, 1.0, engine="hip")
    assert hip_attention == ["attn_h16_wide"]
    scale = ref.abs().max().item()
    err, dist = (out - ref).abs().max().item() / scale, (out - lib).abs().max().item() / scale
    print(f"sd kl-f8 decoder, hip attention: vs library fp32 {err:.3e} of range, vs library-attention hip decode {dist:.3e}")
    assert out.shape == (1, 3, 512, 512) and err <= DECODER_TOL[torch.float16]
