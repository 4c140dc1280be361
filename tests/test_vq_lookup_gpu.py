"""qd_vq_lookup (nearest codebook row without the [pixels][n_e] distance matrix) and the VQ first stage on it
(QDIFF_DECODER_VQ=hip), on the GPU.  Reference: fp64 squared distances on the CPU, of z as rounded to the kernel's input type.

Bound (derived, not measured): the kernel minimises s_j = |e_j|^2/2 - z.e_j = (d_j - |z|^2) / 2, computed with e_dim fmas on an
h_j that carries one rounding (+ its fp64 sum) — n = e_dim + 3 covers the e_dim + 2 operations — so
|s^_j - s_j| <= gamma_n m_j with m_j = |e_j|^2/2 + sum_c |z_c e_jc|, and for the kernel's j* against the true minimiser j0
d[j*] - d[j0] = 2 (s[j*] - s[j0]) <= 2 (gamma m[j*] + gamma m[j0]) <= 4 gamma max(m[j*], m[j0])."""
import pytest
import torch

from golden_util import load_fixture
from test_first_stage import _build
from test_first_stage_hip import DECODER_TOL, ENGINE
from vq_lookup_cases import BF16, F16, F32, FORCED, MAX_SLICES, MIN_SLICE, STAGE, _assert_nearest, _margins, _run

pytestmark = pytest.mark.gpu


@pytest.fixture
def lib():
    from qdiff import hip
    lib = hip.load()
    yield lib
    lib.qd_vq_config(-1)


def _z(cuda, B, E, H, W, layout, dtype, g):
    z = (torch.randn(B, E, H, W, generator=g) * 1.5).to(dtype).to(cuda)
    return z.contiguous(memory_format=torch.channels_last) if layout == "cl" else z


CASES = [  # B, H, W (pixels B*H*W), n_e, e_dim, t_dim (None: the codebook), layout, input, output, ldo
    (1, 1, 1, 1, 3, None, "nchw", F32, F32, 4),
    (1, 7, 9, 2, 1, 5, "cl", F16, F16, 8),
    (1, 5, 13, STAGE - 1, 4, 3, "nchw", BF16, BF16, 16),
    (3, 11, 31, STAGE, 8, 2, "cl", F32, F16, 8),
    (1, 25, 41, STAGE + 1, 3, 8, "nchw", F16, F32, 12),
    (7, 1, 293, 2 * STAGE + 1, 3, 3, "cl", F32, BF16, 8),
    (1, 5, 13, 8192, 3, 3, "cl", F32, F16, 8),
    (1, 7, 9, 8192, 8, None, "nchw", BF16, F32, 8),
    (5, 1, 13, 8192, 4, 1, "cl", F16, BF16, 24),
    (1, 1, 63, 8192, 1, 4, "nchw", F32, F32, 8),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"P{c[0] * c[1] * c[2]}_n{c[3]}_e{c[4]}_t{c[5]}_{c[6]}_{str(c[7])[6:]}_{str(c[8])[6:]}")
def test_lookup_against_fp64_distances(cuda, lib, case):
    B, H, W, n_e, E, T, layout, zdt, odt, ldo = case
    from qdiff import hip
    g = torch.Generator().manual_seed(1000 + n_e + E)
    z = _z(cuda, B, E, H, W, layout, zdt, g)
    cb = torch.randn(n_e, E, generator=g).to(cuda)
    table = None if T is None else torch.randn(n_e, T, generator=g).to(cuda)
    got = [_run(lib, cuda, z, cb, table, odt, ldo, s) for s in FORCED]
    assert all(torch.equal(got[0], other) for other in got[1:])          # the merge does not change the function
    _assert_nearest(z, cb, got[0])
    most = min(MAX_SLICES, -(-n_e // MIN_SLICE))
    for s, want in zip(FORCED[1:], (1, min(2, most), most)):
        lib.qd_vq_config(s)
        assert hip.vq_lookup_form(B, H * W, n_e) == (want, 2 if want > 1 else 1)


def test_the_rule_takes_one_launch_and_two(lib):
    """pixel tiles x code slices reaches two blocks per CU, or the tiles fill the chip alone (DESIGN.md §4.11 addendum 2)"""
    from qdiff import hip
    lib.qd_vq_config(-1)
    assert hip.vq_lookup_form(1, 4096, 8192) == (64, 2) and hip.vq_lookup_form(10, 4096, 8192) == (13, 2)
    assert hip.vq_lookup_form(16, 4096, 8192) == (8, 2) and hip.vq_lookup_form(64, 4096, 8192) == (1, 1)
    assert hip.vq_lookup_form(1, 65, MIN_SLICE) == (1, 1) and hip.vq_lookup_form(1, 65, 8192) == (64, 2)
    assert lib.qd_vq_lookup_ws_bytes(10, 4096, 8192) == 13 * 40960 * 8 and lib.qd_vq_lookup_ws_bytes(64, 4096, 8192) == 0


@pytest.mark.parametrize("slices", FORCED)
def test_planted_minimisers(cuda, lib, slices):
    """pixels EQUAL to codebook rows at the first and last code of the first and last slice (two slices of 4096; 64 of 128) and of
    an LDS stage; a row duplicated in a later slice loses to the lower index; a NaN pixel gives 0; an all-zero pixel goes
    through the margin check"""
    g = torch.Generator().manual_seed(77)
    cb = torch.randn(8192, 3, generator=g)
    cb[5000], cb[8191 - 64] = cb[100], cb[STAGE]                         # duplicates across slices and stages
    planted = [0, MIN_SLICE - 1, MIN_SLICE, STAGE - 1, STAGE, 4095, 4096, 8191 - MIN_SLICE + 1, 8191, 100]
    z = torch.cat([cb[planted], torch.zeros(1, 3), torch.tensor([[0.5, float("nan"), 1.0]])]).t().reshape(1, 3, 1, -1).contiguous().to(cuda)
    idx = _run(lib, cuda, z, cb.to(cuda), None, F32, 4, slices)
    assert idx.tolist()[:len(planted)] == planted and idx[-1].item() == 0
    _assert_nearest(z, cb, idx)


@pytest.mark.parametrize("dtype", [pytest.param(F16, id="fp16"), pytest.param(BF16, id="bf16")])
def test_vq_first_stage_on_the_kernel(cuda, monkeypatch, dtype):
    """VQModelDecoder of the tiny VQ-shaped golden configuration with the knob on: quantize() equals the knob-off composition
    wherever the indices are determined, and decode_first_stage(engine="hip*") — lookup, folded post_quant_conv and conv_in's
    operand rows in one launch — stays inside the decoder's bound against the fp32 decode of the same module."""
    from qdiff import first_stage_hip as fh, hip
    from qdiff.arch import first_stage as fs
    case = load_fixture("first_stage.pt")["vq_tiny"]
    cpu = _build(case, "vq")
    m, z = _build(case, "vq").to(cuda), case["z"].to(cuda)
    calls = []
    monkeypatch.setattr(hip, "vq_lookup", lambda *a, _f=hip.vq_lookup, **k: (calls.append(sorted(k)), _f(*a, **k))[1])
    with torch.no_grad():
        off = m.quantize(z)
        assert not calls
        monkeypatch.setattr(fh, "DECODER_VQ", "hip")
        on, idx = m.quantize(z), m.quantize.indices(z)
        ref = cpu.decode(case["z"])
    assert calls == [["out"], ["indices"]] and on.shape == off.shape and idx.dtype == torch.int64
    _assert_nearest(z, m.quantize.embedding.weight.detach(), idx)
    d, mm, gamma, _ = _margins(z, m.quantize.embedding.weight.detach())
    two = d.topk(2, dim=1, largest=False)
    det = (two.values[:, 1] - two.values[:, 0] > 4 * gamma * mm.max(1).values).to(cuda)
    same = (on == off).permute(0, 2, 3, 1).reshape(-1, on.shape[1]).all(1)
    assert det.any() and same[det].all() and torch.equal(on, m.quantize.embedding.weight.detach()[idx].view(*[z.shape[i] for i in (0, 2, 3, 1)]).permute(0, 3, 1, 2))
    out = fs.decode_first_stage(m, z, 1.0, engine=ENGINE[dtype])
    err = (out.cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"vq_tiny {dtype}: fused VQ head + hip decoder max err {err:.3e} of range")
    assert calls[-1] == ["out", "table"] and len(calls) == 3 and err <= DECODER_TOL[dtype]
