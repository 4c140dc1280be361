"""Host side of the exact-row tests of the first-stage 16-bit convolution: every condition tests/first_stage_conv_cases.py
promises holds for every case (exact operands, the 2^24 bound, tie counts, two independent references that agree), the ABI
emulator passes the cases the wrapper can reach, and the comparison the GPU test uses catches each of a list of planted
mistakes.  No GPU, no library."""
import pytest
import torch

import abi_emulator as E
import first_stage_conv_cases as C


def _deliver(c, rows, part=None, mutate=None):
    """What check() says when a launch had written `rows` (and `part`) — the GPU test's comparison on a modelled launch."""
    xbuf, outbuf, resbuf = C.make_buffers(c)
    C.views(c, xbuf, outbuf, resbuf)[1].copy_(rows)
    if mutate is not None:
        mutate(outbuf)
    return C.check(c, outbuf, c.part if part is None else part)


def test_case_list():
    names = C.CASE_NAMES
    assert len(names) == len(set(names)) and all(n.endswith(("_bf16", "_fp16")) for n in names)
    for stem in ("m_1x1x1_k3", "m_1x5x5_k3", "m_3x7x9_k3", "m_1x3x43_k3", "m_1x15x17_k3", "m_1x1x257_k3", "m_3x7x9_k1", "m_1x1x257_k1",
                 "n_3", "n_5", "n_64", "n_65", "n_70", "n_129", "n_288", "k_cpad8", "k_cpad24", "k_cpad32", "k_cpad40", "k_cpad72",
                 "k_c0_8_ldx48", "k_c0_24_ldx96", "b_H1", "b_W1", "b_ups_1x1", "b_ups_3x5_B3", "b_ups_8x8_res_rows16", "b_onehot",
                 "s_stride2_pad1_8x8", "s_pad0_6x6", "gn_B513", "gn_B512", "v_max", "sub"):
        assert stem + "_bf16" in names and stem + "_fp16" in names, stem
    assert "v_h65520_fp16" in names and "v_overflow_bf16" in names
    ms = {C.get(n).M for n in names if n.startswith("m_")}
    assert ms == {1, 25, 189, 129, 255, 257}
    assert all(C.get(n).M == 189 for n in names if n.startswith(("n_", "col_", "k_")))
    small = [C.get(n) for n in names if not n.startswith("gn_")]
    assert all(c.Cin <= 72 and c.H * c.W <= 257 for c in small)


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_case_conditions(name):
    c = C.get(name)
    # the operands are exact in the operand type (NaN / inf planted ones aside), the weights too
    x = c.x.double()
    fin = torch.isfinite(x)
    assert torch.equal(x[fin].to(c.dtype).double(), x[fin]) and torch.equal(c.w.to(c.dtype).float(), c.w)
    assert c.want.dtype == c.odt and tuple(c.want.shape) == (c.M, c.Cout)
    if c.kind == "values":
        if hasattr(c, "touched"):
            assert 0 < int(c.touched.sum()) < c.M and int((~fin).sum()) == 1
            assert torch.isfinite(c.want32[~c.touched]).all() and not torch.isfinite(c.want32[c.touched]).any()
            if torch.isnan(x).any():
                assert torch.isnan(c.want32[c.touched]).all()
            else:
                t = c.want32[c.touched]
                assert (t == float("inf")).any() and (t == -float("inf")).any() and torch.isnan(t).any()
        return
    # the second computation: gather + int64 matmul, then the same two adds in fp64
    acc = C.conv_int(c).double() * (c.ux * c.uw)
    assert torch.equal(acc, C.conv64(c))
    v = acc
    if c.bias is not None:
        v = v + c.bias.double()[None, :]
    if c.res is not None:
        v = v + c.res.double()
    assert torch.equal(v, c.want32.double())
    # the 2^24 bound from integers: sum |x||w| with |w| through a second pass of the integer gather
    cw = C.NS(**{**vars(c), "w": c.w.abs()})
    bound = C.conv_int(cw, x=x.abs()).double() * (c.ux * c.uw)
    if c.bias is not None:
        bound = bound + c.bias.double().abs()[None, :]
    if c.res is not None:
        bound = bound + c.res.double().abs()
    assert bound.max().item() / c.unit < 2 ** 24 and bound.max().item() / c.unit == c.bound_units
    assert torch.equal((v / c.unit).round() * c.unit, v)
    if c.odt != torch.float32:
        inexact, down, up = C.round_stats(c.want32, c.odt)
        assert down + up >= 200 and min(down, up) >= 10 and inexact >= 0.10, (inexact, down, up)
        # ties by their definition, without the bit trick of round_stats: v32 is the mean of two neighbouring 16-bit numbers
        r = c.want.double()
        d = c.want32.double() - r
        other = (c.want32.double() + d).to(c.odt).double()
        ties = (d != 0) & (other == c.want32.double() + d) & ((other - r).abs() == 2 * d.abs())
        assert int(ties.sum()) == down + up
        assert c.res is None or c.res.dtype == c.odt
    if c.want_alt is not None:
        assert not torch.equal(c.want, c.want_alt) and (c.want[::7] != c.want_alt[::7]).any()
    if c.part is not None:
        assert tuple(c.part.shape) == (c.B, 1, c.Cout, 2) and c.part[..., 1].max().item() < 2 ** 24
        assert c.res is not None and not torch.equal(C.gn_sums(c, C.finish(c, c.acc32, res=c.res * 0)), c.part)   # the residual counts


def test_big_case_conditions():
    c = C.big_case()
    assert (c.M, c.Cout, c.c0, c.ldx) == (523775, 8, 4088, 4096) and tuple(c.x.shape) == (523775, 8) and c.odt == torch.float32
    assert c.M * c.ldx * 2 == 4290764800 < 2 ** 32 <= 512 * 1025 * c.ldx * 2
    assert torch.equal(C.conv_int(c).double(), C.conv64(c)) and c.bound_units < 2 ** 24


HAND_BUILT = ("k_c0_", "s_")          # c0 > 0, other strides and paddings: not calls hip.conv2d_bf16 can make


@pytest.mark.parametrize("name", [n for n in C.CASE_NAMES if not n.startswith(HAND_BUILT)])
def test_cases_through_the_emulator(name):
    c = C.get(name)
    assert c.wrapper and all(not C.get(n).wrapper for n in C.CASE_NAMES if n.startswith(HAND_BUILT))
    xbuf, outbuf, resbuf = C.make_buffers(c)
    xv, ov, rv = C.views(c, xbuf, outbuf, resbuf)
    wt = E.pack_weights_bf16(c.w, c.dtype)
    part = torch.zeros_like(c.part) if c.part is not None else None
    E.conv2d_bf16(xv, wt, c.bias, ov, c.B, c.H, c.W, c.cpad, c.Cout, k=c.k, pad=c.pad, residual=rv, gn_part=part, upsample2x=c.ups)
    errors, which = C.check(c, outbuf, part)
    assert not errors, errors
    assert which == "as_is"


def test_check_accepts_both_subnormal_references():
    for dt in C.DTYPES:
        c = C.get(f"sub_{dt}")
        assert _deliver(c, c.want) == ([], "as_is") and _deliver(c, c.want_alt) == ([], "flushed")


# ---- planted mistakes: each must be caught by the comparison the GPU test uses ---------------------------------------------------

def _caught(c, rows, part=None, mutate=None, needle=None):
    errors, which = _deliver(c, rows, part, mutate)
    assert errors, (c.name, which)
    if needle:
        assert any(needle in e for e in errors), errors
    return errors


def _rows(c, acc, **kw):
    return C.finish(c, acc.float(), **kw).to(c.odt)


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_planted_tap_dropped_at_a_border_pixel(dt):
    c = C.get(f"b_onehot_{dt}")
    # the corner one-hot of sample 0 sits at pixel (0, 0): output pixel (0, 0) reads it through the centre tap
    rows = _rows(c, C.conv_int(c, drop=(0, 4)).double())
    _caught(c, rows, needle="want (n=0, c=0, tap=4)")
    # ... and the last sample's one-hot at its last pixel (6, 6): row M - 1, centre tap
    _caught(c, _rows(c, C.conv_int(c, drop=(c.M - 1, 4)).double()), needle=f"row {c.M - 1} (sample 1, pixel (6, 6))")
    c = C.get(f"m_1x5x5_k3_{dt}")
    _caught(c, _rows(c, C.conv_int(c, drop=(4, 3)).double() * (c.ux * c.uw)), needle="row 4 (sample 0, pixel (0, 4))")


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["b_ups_1x1", "b_ups_3x5_B3", "b_ups_8x8_res_rows16"])
def test_planted_upsample_map_rounds_up(dt, stem):
    c = C.get(f"{stem}_{dt}")
    acc = C.conv_int(c, upmap=lambda i: (i + 1) >> 1).double() * (c.ux * c.uw)
    if stem == "b_ups_1x1":                                  # a 1x1 stored map has one pixel whatever the map: nothing to catch
        assert _deliver(c, _rows(c, acc))[0] == []
    else:
        _caught(c, _rows(c, acc))


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["m_3x7x9_k3", "n_65", "col_mis128_rows16", "b_ups_8x8_res_rows16"])
def test_planted_truncation(dt, stem):
    c = C.get(f"{stem}_{dt}")
    rows = C.truncated(c.want32, c.odt)
    assert (rows.double().abs() <= c.want32.double().abs()).all() and not torch.equal(rows, c.want)
    _caught(c, rows)
    # round half away from zero instead of half to even
    r = c.want.double()
    d = c.want32.double() - r
    other = (c.want32.double() + d).to(c.odt)
    tie_down = (d != 0) & (other.double() == c.want32.double() + d) & (r.abs() < c.want32.double().abs())
    assert tie_down.any()
    _caught(c, torch.where(tie_down, other, c.want))


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["m_1x3x43_k3", "m_1x1x1_k3", "m_1x1x257_k3", "gn_B513"])
def test_planted_last_row_unwritten(dt, stem):
    c = C.get(f"{stem}_{dt}")

    def unwrite(outbuf):
        outbuf.as_strided((c.M, c.Cout), (c.ldo, 1), c.out_pre)[c.M - 1] = C.filled(c.Cout, c.odt)
    _caught(c, c.want, mutate=unwrite, needle=f"row {c.M - 1} ")


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["k_c0_8_ldx48", "k_c0_24_ldx96"])
def test_planted_channels_read_from_before_c0(dt, stem):
    c = C.get(f"{stem}_{dt}")
    xbuf = C.make_buffers(c)[0]
    x = xbuf.as_strided((c.Mi, c.cpad), (c.ldx, 1), c.x_pre + c.c0 - 8).double()
    assert torch.isnan(x[:, :8]).all() and torch.equal(x[:, 8:], c.x.double()[:, :-8])
    _caught(c, _rows(c, C.conv64(c, x)))
    # the same with finite bytes in front of c0: still wrong
    _caught(c, _rows(c, C.conv64(c, torch.nan_to_num(x, nan=1.0))))


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["col_resmis_rows32", "col_resmis_rows16", "col_outmis_rows16", "b_ups_8x8_res_rows16"])
def test_planted_residual_shifted_by_one_row(dt, stem):
    c = C.get(f"{stem}_{dt}")
    _caught(c, _rows(c, c.acc32, res=torch.roll(c.res, 1, 0)))


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["n_70", "n_129", "n_5"])
def test_planted_bias_of_the_next_column_in_the_tail(dt, stem):
    c = C.get(f"{stem}_{dt}")
    tail = c.Cout // 32 * 32 if c.Cout % 32 else c.Cout - 32
    bias = c.bias.clone()
    bias[tail:-1] = c.bias[tail + 1:]
    bias[-1] = 0.0                                              # the column after the last: what a zero-filled constant gives
    assert not torch.equal(bias, c.bias)
    _caught(c, _rows(c, c.acc32, bias=bias))


@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("stem", ["col_ldo_rows32", "col_ldo_rows16", "col_mis128_rows16", "n_3", "m_1x1x1_k3"])
def test_planted_sentinel_byte(dt, stem):
    c = C.get(f"{stem}_{dt}")
    esz = 4 if c.odt == torch.float32 else 2
    spots = [c.out_pre - 1, c.out_pre + c.M * c.ldo - (c.ldo - c.Cout), 0]          # before row 0, after the last row, the buffer's start
    if c.ldo > c.Cout:
        spots += [c.out_pre + c.Cout, c.out_pre + 5 * c.ldo + c.ldo - 1]             # the pad columns of rows 0 and 5
    for pos in spots:
        for byte in range(esz):
            def flip(outbuf, pos=pos, byte=byte):
                raw = outbuf.view(torch.uint8)
                raw[pos * esz + byte] ^= 1
            _caught(c, c.want, mutate=flip, needle="outside the output changed")


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_planted_one_flushed_subnormal(dt):
    c = C.get(f"sub_{dt}")
    m, n = (c.want != c.want_alt).nonzero()[3].tolist()
    for base, other in ((c.want, c.want_alt), (c.want_alt, c.want)):
        rows = base.clone()
        rows[m, n] = other[m, n]
        _caught(c, rows, needle="neither reference matches")
    # a third result: the operand flushed to the smallest normal number instead of zero
    rows = c.want.clone()
    rows[0] = rows[0] * 2
    _caught(c, rows)


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_planted_statistics_of_the_last_chunk_over_256_rows(dt):
    c = C.get(f"gn_B513_{dt}")
    v = c.want32.double()[-256:]
    part = c.part.clone()
    part[-1, 0] = torch.stack([v.sum(0), (v * v).sum(0)], dim=-1).float()
    _caught(c, c.want, part=part, needle=f"sample {c.B - 1} chunk 0")
    # the statistics without the residual
    _caught(c, c.want, part=C.gn_sums(c, C.finish(c, c.acc32, res=c.res * 0)), needle="statistics differ")
    # one sum of squares off by one unit in the last place
    part = c.part.clone()
    part[7, 0, 100, 1] = torch.nextafter(part[7, 0, 100, 1], torch.tensor(float("inf")))
    _caught(c, c.want, part=part, needle="sample 7 chunk 0 channel 100 sum of squares")


@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_planted_non_finite_spread(dt):
    """inf / NaN cases: one more, or one fewer, non-finite output than the receptive field gives is caught; so is -inf for +inf."""
    for stem in ("v_inf_corner", "v_nan_ups", "v_inf_last"):
        c = C.get(f"{stem}_{dt}")
        rows = c.want.clone()
        m = int((~c.touched).nonzero()[0])
        rows[m, 0] = float("nan")
        _caught(c, rows, needle=f"row {m} ")
        rows = c.want.clone()
        m = int(c.touched.nonzero()[-1])
        rows[m, 3] = 1.0
        _caught(c, rows, needle=f"row {m} ")
        if "inf" in stem:
            rows = torch.where(torch.isinf(c.want), -c.want, c.want)
            _caught(c, rows)
