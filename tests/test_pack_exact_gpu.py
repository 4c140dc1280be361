"""GPU tests of the tile-ordered weight packers qd_pack_weights_t4 / _t8 (pack_t4_kernel / pack_t8_kernel, csrc/igemm_dma.hip) and
of every reader of their layout, without tolerance.

(a) Byte image: every case of tests/pack_exact_cases.py through hip.pack_weights_t4 / _t8 into a sentinel-filled buffer with a
    spare K-step on each side; the WHOLE buffer and `wsum` must equal the index formula's.  One case through mode 0 of the row-major
    qd_pack_weights.
(b) Decode probes: a Linear whose weight holds every code against every zero point, contracted with the rows of +-identity, so
    that each output element is ONE product (exact in fp32): qd_conv2d_i8_acc, qd_conv2d_i8 (fp32 rows with a bias), qd_conv2d_wq_h16
    (fp16 and bf16 rows, split-K forced on and off), hip.temb_mlp and hip.temb_mlp_wq_h16 must each return every code value."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import pack_exact_cases as C
from conv_tall_tile_cases import launch_forms

pytestmark = pytest.mark.gpu


# ---- (a) byte image --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.FAMILIES)
def test_packed_image_is_exact(cuda, record_property, family):
    from qdiff import hip
    total = 0
    for c in C.by_family(family):
        for order in c.orders:
            buf, wsum = C.run_packers(c, order, hip.pack_weights_t4, hip.pack_weights_t8, cuda)
            nsum = 0 if c.want_wsum is None else c.want_wsum.size
            print(f"[pack_exact] {c.name} order {order}: {buf.size} bytes, {nsum} sums compared")
            assert np.array_equal(buf, c.want_buf), C.first_difference(c, buf)
            if c.want_wsum is not None:
                bad = np.flatnonzero(wsum != c.want_wsum)
                assert bad.size == 0, f"{c.name}: wsum[{bad[0]}] = {wsum[bad[0]]}, want {c.want_wsum[bad[0]]} (zero point {c.segs[0].zp[bad[0]]})"
            total += buf.size
        record_property(c.name, int(c.want_buf.size) * len(c.orders))
    print(f"[pack_exact] family {family}: {len(C.by_family(family))} cases, {total} bytes compared")
    record_property("bytes", total)
    assert total > 0


def test_row_major_packer_mode0_image_is_exact(cuda):
    """qd_pack_weights, mode 0 (stored s8 = W - zw, row-major [n][tap][ldk]): the grid values of a 6-bit grid against zero points
    that keep W - zw in int8, at a column offset inside sentinel-filled rows; codes, bytes, pads and sums."""
    from qdiff import hip
    L, taps, kofs = 64, 3, 16
    zps = [0, 1, 32, 63, 64, 128]
    tg = torch.arange(-3, L + 3, dtype=torch.float64)
    clen, Cout = tg.numel(), len(zps)
    pad, ldk = C.pad16(clen), C.pad16(clen) + 32
    z = torch.tensor([float(v) for v in zps])
    d = torch.tensor([2.0 ** -(2 + i) for i in range(Cout)])
    w = ((tg.view(1, -1, 1) + torch.arange(taps).view(1, 1, -1) - z.double().view(-1, 1, 1)) * d.double().view(-1, 1, 1)).float()
    want = torch.clamp(torch.round(w / d.view(-1, 1, 1)) + z.view(-1, 1, 1), 0, L - 1).long()          # [Cout][clen][taps]
    assert want.min() == 0 and want.max() == L - 1 and len(want.unique()) == L
    stored = want - z.long().view(-1, 1, 1)
    assert stored.min() == -128 and stored.max() == L - 1
    rows = np.full((Cout, taps, ldk), C.SENTINEL, dtype=np.uint8)
    rows[:, :, kofs:kofs + pad] = 0
    rows[:, :, kofs:kofs + clen] = (stored.permute(0, 2, 1).numpy() & 0xff).astype(np.uint8)
    wq = torch.full((Cout * taps * ldk,), C.SENTINEL, dtype=torch.uint8, device=cuda)
    wsum = (torch.arange(Cout, dtype=torch.int32) * 11 - 5).to(cuda)
    codes = torch.full((Cout, clen, taps), -1, dtype=torch.int32, device=cuda)
    hip.pack_weights(w.to(cuda), None, d.to(cuda), z.to(cuda), Cout, clen, taps, 0, clen, L, 0, wq, ldk, kofs, wsum, codes)
    torch.cuda.synchronize()
    assert torch.equal(codes.cpu().long(), want)
    assert np.array_equal(wq.cpu().numpy().reshape(Cout, taps, ldk), rows)
    assert torch.equal(wsum.cpu().long(), torch.arange(Cout) * 11 - 5 + stored.sum(dim=(1, 2)))


# ---- (b) decode probes -----------------------------------------------------------------------------------------------------
N_OUT = 64


def _engine_zero_points(L):
    """The zero points of the case file that engine.pack_module_weights accepts (-128 ... 255)."""
    return [z for z in C.zero_points(L) if -128 <= z <= 255]


@functools.lru_cache(maxsize=None)
def probe(device, bits, alpha, narrow=False):
    """The probe layer: w[n][k] = (code(k) - z[n]) * delta[n], code(k) = k mod L, K = 64 (4-bit) / 256 (8-bit), Cout = 64, z[n]
    cycling over the zero points, delta[n] a power of two.  alpha: AdaRound with alpha of both signs and w shifted by
    -(alpha >= 0) * delta (the same codes).  narrow: only zero points whose span max |q - z| is <= 256 (bf16 operands)."""
    from qdiff import engine
    L = 16 if bits == 4 else 256
    K = 64 if bits == 4 else 256
    zl = [z for z in _engine_zero_points(L) if not narrow or max(abs(0 - z), abs(L - 1 - z)) <= 256]
    z = torch.tensor([float(zl[n % len(zl)]) for n in range(N_OUT)])
    d = torch.tensor([2.0 ** -(2 + (n // len(zl)) % 5) for n in range(N_OUT)])
    code = (torch.arange(K) % L).double()
    al, up = None, torch.zeros(N_OUT, K, dtype=torch.float64)
    if alpha:
        al = torch.where((torch.arange(N_OUT).view(-1, 1) * 3 + torch.arange(K).view(1, -1)) % 3 == 0, -0.3, 0.7).float().view(N_OUT, K, 1, 1)
        up = (al.view(N_OUT, K) >= 0).double()
    w64 = (code.view(1, -1) - z.double().view(-1, 1) - up) * d.double().view(-1, 1)
    w = w64.float()
    assert torch.equal(w.double(), w64)
    q = NS(delta=d.view(-1, 1, 1, 1), zero_point=z.view(-1, 1, 1, 1), n_bits=bits, sym=False, n_levels=L, alpha=al, soft_targets=False)
    pack = engine.pack_module_weights(w.view(N_OUT, K, 1, 1).to(device), [q], 0)
    assert pack.wbits == bits and pack.tiled and len(pack.segs) == 1
    # the engine's pack holds the bytes of the index formula (one more case of (a), through the engine's own call)
    c = C.make_case("probe", bits, L, w.view(N_OUT, K, 1), [dict(c0=0, clen=K, delta=d, zp=z, alpha=None if al is None else al.view(N_OUT, K, 1))], K, 1)
    inner = c.want_buf.reshape(c.total_steps, -1)[1:-1].reshape(-1)
    assert np.array_equal(pack.wq.cpu().numpy(), inner) and np.array_equal(pack.segs[0]["wsum"].cpu().numpy().astype(np.int64), c.want_wsum)
    codes = C.seg_codes(c, c.segs[0])[:, :, 0]                                         # [Cout][K]
    assert torch.equal(codes, (torch.arange(K) % L).view(1, -1).expand(N_OUT, K))
    bias = ((torch.arange(N_OUT) % 7) - 3).float() * 0.25                              # multiples of 1/4: every fma below is exact
    return NS(bits=bits, L=L, K=K, z=z.long(), d=d, code=(torch.arange(K) % L), pack=pack, bias=bias, zl=zl)


def _report(p, got, want, sign):
    """got / want [K][Cout]: None when the bits agree, else the first differing (n, k) with its code and zero point."""
    if got.dtype.is_floating_point:
        same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    else:
        same = got == want
    if bool(same.all()):
        return None
    k, n = [int(v) for v in (~same).nonzero()[0]]
    return (f"{int((~same).sum())} of {same.numel()} outputs differ, first at n = {n}, k = {k}: code {int(p.code[k])}, zero point {int(p.z[n])}, "
            f"delta {float(p.d[n])}, sign {sign}: got {got[k, n].item()!r}, want {want[k, n].item()!r}")


def _want_int(p, sign):
    return (sign * (p.code.view(-1, 1) - p.z.view(1, -1))).to(torch.int32)                     # [K][Cout]


def _want_f32(p, sign, bias):
    v = _want_int(p, sign).double() * p.d.double().view(1, -1) + (bias.double().view(1, -1) if bias is not None else 0.0)
    assert torch.equal(v.float().double(), v)                                                # exact in fp32: no rounding to argue about
    return v.float()


def _act(zx):
    return NS(delta=torch.tensor(1.0), zero_point=zx, n_bits=8, sym=False)


def _signs(zx):
    """identity where zx + 1 is on the grid, -identity where zx - 1 is."""
    return [s for s in (1, -1) if 0 <= zx + s <= 255]


BITS_ALPHA = [(4, False), (4, True), (8, False), (8, True)]
_IDS = [f"w{b}-{'adaround' if a else 'nearest'}" for b, a in BITS_ALPHA]


@pytest.mark.parametrize("bits,alpha", BITS_ALPHA, ids=_IDS)
def test_int8_contraction_returns_every_code(cuda, record_property, bits, alpha):
    """qd_conv2d_i8_acc (exact accumulators, 128-row tiles) and qd_conv2d_i8 (fp32 rows, fma(I, dx * dw[n], bias[n])) with the
    activation quantiser dx = 1, zx in {0, 128, 255}."""
    from qdiff import engine
    p = probe(cuda, bits, alpha)
    K, n = p.K, 0
    for zx in (0, 128, 255):
        plan = engine.build_conv_plan(p.pack, [_act(zx)], 1, 1, 1, 0, p.bias.to(cuda))
        for sign in _signs(zx):
            x = (sign * torch.eye(K)).view(K, K, 1).to(cuda)                                   # [B = K rows][C = K][S = 1]
            xq = engine.quantize_rows(x, plan, K, K, 1, (K, 1, 1))
            stored = xq.cpu().long() + 128
            assert torch.equal(stored[:, :K], zx + sign * torch.eye(K, dtype=torch.long))      # one code off the zero point per row
            acc = torch.full((K, N_OUT), 12345, dtype=torch.int32, device=cuda)
            engine.conv_forward(plan, xq, 1, 1, K, Ho=1, Wo=K, acc_out=acc)
            torch.cuda.synchronize()
            why = _report(p, acc.cpu(), _want_int(p, sign), sign)
            assert why is None, f"qd_conv2d_i8_acc, zx {zx}: {why}"
            for splitk in (False, None):
                with launch_forms() as forms:
                    out = engine.conv_forward(plan, xq, 1, 1, K, Ho=1, Wo=K, out_dtype=torch.float32, splitk=splitk)
                torch.cuda.synchronize()
                # K rows x 64 columns is one block of rows at most twice: the 256-row tile needs 256 blocks and cannot be taken here
                assert len(forms) == 1 and forms[0][0] == 128, forms
                why = _report(p, out.cpu(), _want_f32(p, sign, p.bias), sign)
                assert why is None, f"qd_conv2d_i8, zx {zx}, form {forms[0]}: {why}"
                n += 2 * K * N_OUT if splitk is False else K * N_OUT
    print(f"[pack_exact] int8 contraction w{bits}: {n} outputs compared, launch form {forms[0]}")
    record_property("outputs", n)


def _wq_call(plan, xh, K, splitk):
    from qdiff import hip
    out = torch.full((K, plan.Cout), float("nan"), dtype=torch.float32, device=xh.device)
    return out, hip.ConvCall(x=xh, w=plan.pack.wq, out=out, bias=plan.bias, ldx=plan.ldx, ldk=plan.pack.ldk, ldo=out.stride(0), ldr=0, ld_rowbias=0,
                             B=1, H=1, W=K, Ho=1, Wo=K, Cout=plan.Cout, kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=plan.pack.wbits,
                             w_tiled=True, segs=plan.segs, splitk=splitk)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("bits,alpha", BITS_ALPHA, ids=_IDS)
def test_weights_only_contraction_returns_every_code(cuda, record_property, bits, alpha, dtype):
    """qd_conv2d_wq_h16: out[k][n] = delta[n] * (code(k) - z[n]) + bias[n] from the 1024 + q / -(1024 + z) halves, against every zero
    point with fp16 rows; with bf16 rows against those whose span is at most 256, the plan being refused for a wider one.  One
    pass and split-K (forced through hip.wq_h16_config)."""
    from qdiff import engine, hip
    wide = probe(cuda, bits, alpha)
    assert set(wide.zl) == set(_engine_zero_points(wide.L))
    span = int((wide.code.view(-1, 1) - wide.z.view(1, -1)).abs().max())
    assert engine.wonly_code_span(wide.pack) == (255 if bits == 4 else span)
    p = wide
    if dtype == torch.bfloat16 and bits == 8:
        assert span == 255 + 128 and engine.build_wonly_plan(wide.pack, 1, 1, 1, 0, wide.bias.to(cuda), dtype) is None
        p = probe(cuda, bits, alpha, narrow=True)
        assert set(p.zl) == {-1, 0, 255} and engine.wonly_code_span(p.pack) == 256
    plan = engine.build_wonly_plan(p.pack, 1, 1, 1, 0, p.bias.to(cuda), dtype)
    assert plan is not None
    K, n, seen = p.K, 0, set()
    try:
        for sign in (1, -1):
            x = (sign * torch.eye(K)).view(K, K, 1).to(cuda)
            xh = engine.wonly_rows(x, plan, K, K, 1, (K, 1, 1))
            for knob, splitk in ((0, None), (0, True), (2, True), (4, True)):
                hip.wq_h16_config(knob)
                out, call = _wq_call(plan, xh, K, splitk)
                form = hip.conv2d_wq_h16_form(call, dtype)
                hip.conv2d_wq_h16(call, dtype)
                torch.cuda.synchronize()
                assert form[0] == (min(knob, K // 64) if knob and K > 64 else 1), (knob, form)     # slices never outnumber the K-steps
                seen.add(form[0])
                why = _report(p, out.cpu(), _want_f32(p, sign, p.bias), sign)
                assert why is None, f"qd_conv2d_wq_h16 {dtype}, K slices {form[0]}: {why}"
                n += K * N_OUT
    finally:
        hip.wq_h16_config(-1)
    assert seen == ({1} if bits == 4 else {1, 2, 4})
    print(f"[pack_exact] weights-only contraction w{bits} {dtype}: {n} outputs compared, K slices {sorted(seen)}")
    record_property("outputs", n)


@pytest.mark.parametrize("bits,alpha", BITS_ALPHA, ids=_IDS)
def test_temb_mlp_returns_every_code(cuda, record_property, bits, alpha):
    """hip.temb_mlp (int8: its own quantiser, temb_kernel's hand-computed tile addresses) on one-layer MLPs without SiLU; the
    wrapper feeds the rows in the groups the launcher accepts (its LDS holds a group's K-wide rows)."""
    from qdiff import engine, hip
    p = probe(cuda, bits, alpha)
    K, n = p.K, 0
    for zx in (0, 128, 255):
        plan = engine.build_conv_plan(p.pack, [_act(zx)], 1, 1, 1, 0, p.bias.to(cuda))
        for sign in _signs(zx):
            x = (sign * torch.eye(K)).to(cuda)
            out = torch.full((K, N_OUT + 8), float("nan"), dtype=torch.float32, device=cuda)
            hip.temb_mlp(x, False, [plan], [4], out)
            torch.cuda.synchronize()
            got = out.cpu()
            assert torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + N_OUT:]).all()
            why = _report(p, got[:, 4:4 + N_OUT], _want_f32(p, sign, p.bias), sign)
            assert why is None, f"qd_temb_mlp, zx {zx}: {why}"
            n += K * N_OUT
    print(f"[pack_exact] temb_mlp w{bits}: {n} outputs compared")
    record_property("outputs", n)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("bits,alpha", BITS_ALPHA, ids=_IDS)
def test_temb_mlp_wq_h16_returns_every_code(cuda, record_property, bits, alpha, dtype):
    """qd_temb_mlp_wq_h16 (wq_magic / wq_frag of csrc/wq_codes.h behind its own tile addresses), any number of rows per call."""
    from qdiff import engine, hip
    p = probe(cuda, bits, alpha, narrow=(dtype == torch.bfloat16 and bits == 8))
    plan = engine.build_wonly_plan(p.pack, 1, 1, 1, 0, p.bias.to(cuda), dtype)
    assert plan is not None
    K, n = p.K, 0
    for sign in (1, -1):
        x = (sign * torch.eye(K)).to(cuda)
        out = torch.full((K, N_OUT + 8), float("nan"), dtype=torch.float32, device=cuda)
        hip.temb_mlp_wq_h16(x, False, [plan], [4], out, dtype)
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + N_OUT:]).all()
        why = _report(p, got[:, 4:4 + N_OUT], _want_f32(p, sign, p.bias), sign)
        assert why is None, f"qd_temb_mlp_wq_h16 {dtype}: {why}"
        n += K * N_OUT
    print(f"[pack_exact] temb_mlp_wq_h16 w{bits} {dtype}: {n} outputs compared")
    record_property("outputs", n)
