"""CPU tests (no GPU) of the first-stage decoder's attention knob (first_stage_hip.DECODER_ATTN, HipDecoder(attention=...)).
hip.attn_h16 / hip.attn_h16_wide run on the fp64 emulation of tests/test_weight_only_attention_host.py, the rest of the decoder
on tests/abi_emulator.py; the argument checks of qd_attn_h16_wide run on the built library."""
import pytest
import torch
import torch.nn.functional as F

from golden_util import load_fixture
from test_first_stage import _build
from test_first_stage_hip import DECODER_TOL, ENGINE
from test_weight_only_attention_host import attn_h16_emulated

DTYPES = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]
CASES = [("kl_tiny", "kl"), ("vq_tiny", "vq")]


@pytest.fixture
def emu(monkeypatch):
    """(first_stage_hip, calls): launch wrappers on the emulators, the attention wrappers recording (name, arguments)"""
    import abi_emulator
    from qdiff import first_stage_hip as fh, hip
    abi_emulator.install(monkeypatch)
    calls = []
    for name in ("attn_h16", "attn_h16_wide"):
        getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _n=name: (calls.append((_n, a)), attn_h16_emulated(*a))[1])
    monkeypatch.setattr(fh, "DECODER_ATTN", "library")
    return fh, calls


def _decode(name, kind, dtype):
    from qdiff.arch import first_stage as fs
    case = load_fixture("first_stage.pt")[name]
    m = _build(case, kind)
    out = fs.decode_first_stage(m, case["z"], 1.0, force_not_quantize=True, engine=ENGINE[dtype])
    return case, m, out, sum(1 for mod in m.decoder.modules() if isinstance(mod, fs.AttnBlock))


@pytest.mark.parametrize("name,kind", CASES)
def test_knob_off_is_the_library_call(emu, monkeypatch, name, kind):
    """default: every AttnBlock is one scaled_dot_product_attention and no wrapper call; an instance pinned to "library" gives
    the same bytes while the module knob says "hip" """
    fh, calls = emu
    sdpa, real = [], F.scaled_dot_product_attention
    monkeypatch.setattr(fh.F, "scaled_dot_product_attention", lambda *a, **k: (sdpa.append(1), real(*a, **k))[1])
    case, m, out, nblocks = _decode(name, kind, torch.float16)
    assert nblocks > 0 and len(sdpa) == nblocks and not calls
    fh.set_decoder_attention("hip")
    pinned = fh.HipDecoder(m.decoder, attention="library")(m.post_quant_conv(case["z"]).float())
    assert torch.equal(pinned, out) and not calls


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kind", CASES)
def test_knob_on_takes_one_kernel_per_attention_block(emu, name, kind, dtype):
    fh, calls = emu
    fh.set_decoder_attention("hip")
    case, _, out, nblocks = _decode(name, kind, dtype)
    err = (out - case["out"]).abs().max().item() / case["out"].abs().max().item()
    assert len(calls) == nblocks and err <= DECODER_TOL[dtype], (name, len(calls), err)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,route", [(64, "attn_h16"), (256, "attn_h16"), (288, "attn_h16_wide"), (512, "attn_h16_wide"), (544, None)])
def test_routing_and_strides_by_channel_count(emu, C, route, dtype):
    """an injected AttnBlock of C channels: <= 256 -> attn_h16, <= 512 -> attn_h16_wide, wider -> the library; the operands are
    the three column ranges of ONE [B*S][3C] tensor with strides (S*3C, 3C, C, 1), the output rows are proj_out's operand type
    (attn_h16 has no bf16 rows: fp32 there)"""
    from qdiff.arch import first_stage as fs
    fh, calls = emu
    torch.manual_seed(C)
    B, H, W = 2, 2, 3
    att, x = fs.AttnBlock(C).eval(), torch.randn(B * H * W, C)
    want = att(x.view(B, H, W, C).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(B * H * W, C)
    hd = fh.HipDecoder(_build(load_fixture("first_stage.pt")["kl_tiny"], "kl").decoder, dtype, attention="hip")
    got, _ = hd._attn("injected", att, x, None, B, H, W)
    assert (got - want).abs().max().item() <= DECODER_TOL[dtype] * want.abs().max().item()
    assert [n for n, _ in calls] == ([route] if route else [])
    if route:
        q, k, v, b, T, S, heads, d, qs, ks, vs, scale, op, out = calls[0][1]
        assert (b, T, S, heads, d, scale, op) == (B, H * W, H * W, 1, C, C ** -0.5, dtype)
        assert qs == ks == vs == (H * W * 3 * C, 3 * C, C, 1) and q.dtype == dtype
        assert [t.data_ptr() - q.data_ptr() for t in (k, v)] == [C * q.element_size(), 2 * C * q.element_size()]
        assert out.dtype == (torch.float32 if (route == "attn_h16" and dtype == torch.bfloat16) else dtype) and out.shape == (B * H * W, C)


def test_argument_checks_of_the_built_library():
    """qd_attn_h16_wide has qd_attn_h16's parameter list, takes d = 264 and 512 as far as the next check and refuses 256 and 520
    with its own range (the checks precede any device work: the fake non-null pointers are never followed)"""
    from qdiff import hip
    lib = hip.load()
    assert list(lib.qd_attn_h16_wide.argtypes) == list(lib.qd_attn_h16.argtypes)
    st = lambda d: (16 * d, d, d, 1)
    call = lambda d, scale: lib.qd_attn_h16_wide(64, 64, 64, 1, 1, 16, 16, 1, d, *st(d), *st(d), *st(d), scale, 1, 64, hip.BF16, d, None)
    for d in (256, 520):
        assert call(d, 1.0) != 0 and "[264, 512]" in lib.qd_last_error().decode(), d
    for d in (264, 512):
        assert call(d, 0.0) != 0 and "scale" in lib.qd_last_error().decode(), d
