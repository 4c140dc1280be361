"""Host checks of the tile-ordered weight packer cases (tests/pack_exact_cases.py): the conditions the case list must meet
(computed on the expected data alone), the emulated packers (tests/abi_emulator.py) against the index formula byte for byte, the
Python decode of the layout (engine.wonly_code_span), mutations of the emulator's packers that the comparison must catch, and
every refusal of qd_pack_weights_t4 / _t8 through the real library with nothing launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import abi_emulator
import pack_exact_cases as C
from conv_form_util import FAKE


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


def _emulated(c, order=None):
    return C.run_packers(c, order or c.orders[0], abi_emulator.pack_weights_t4, abi_emulator.pack_weights_t8)


def _same(c, buf, wsum):
    return np.array_equal(buf, c.want_buf) and (c.want_wsum is None or np.array_equal(wsum, c.want_wsum))


# ---- the case list ---------------------------------------------------------------------------------------------------------
def test_case_list_conditions(cases):
    assert {c.family for c in cases.values()} == set(C.FAMILIES)
    for bits, L in ((4, 16), (8, 256)):
        mine = [c for c in cases.values() if c.bits == bits and c.n_levels == L]
        seen = np.zeros(L, dtype=bool)
        for c in mine:
            for s in c.segs:
                seen[np.unique(C.seg_codes(c, s).numpy())] = True
        assert seen.all(), (bits, np.flatnonzero(~seen))                       # every code value occurs
    # both clamp ends occur: an unclamped value below 0 and one above L - 1, against every zero point of the list
    for name in ("grid_t4", "grid_t8", "grid_t4_alpha", "grid_t8_alpha"):
        c = cases[name]
        s = c.segs[0]
        raw = torch.round(c.w / s.delta.view(-1, 1, 1)) + (0 if s.alpha is None else 1) + s.zp.view(-1, 1, 1)
        assert set(s.zp.tolist()) == set(float(z) for z in C.zero_points(c.n_levels))
        assert ((raw < 0).any(dim=(1, 2)) & (raw > c.n_levels - 1).any(dim=(1, 2))).all(), name
        codes = C.seg_codes(c, s)
        assert (codes.amin(dim=(1, 2)) == 0).all() and (codes.amax(dim=(1, 2)) == c.n_levels - 1).all()
    # ties of both parities, the ties that land on the clamp ends included
    for name in ("ties_t4", "ties_t8"):
        c = cases[name]
        s = c.segs[0]
        q = (c.w / s.delta.view(-1, 1, 1)).double()
        assert torch.equal(q - torch.floor(q), torch.full_like(q, 0.5))
        fl = torch.floor(q).long()
        assert (fl % 2 == 0).any() and (fl % 2 == 1).any()
        unclamped = torch.round(q) + s.zp.view(-1, 1, 1)
        assert (unclamped == 0).any() and (unclamped == c.n_levels).any() and (unclamped < 0).any()
    # pads in K and in N
    assert any(s.clen % 16 for c in cases.values() for s in c.segs) and any(C.pad16(s.clen) % 64 for c in cases.values() for s in c.segs)
    assert any(c.Cout % 32 for c in cases.values())
    g = [c for c in cases.values() if c.family == "geom"]
    assert {(c.bits, c.Cout, c.segs[0].clen, c.taps) for c in g} == {(b, n, k, t) for b in (4, 8) for n in C.COUTS for k in C.CLENS for t in C.TAPS}
    assert any(c.wsum0 is None for c in cases.values()) and any(c.wsum0 is not None and c.wsum0.any() for c in cases.values())
    assert {c.n_levels for c in cases.values() if c.bits == 4} == {2, 4, 8, 16}
    assert {c.n_levels for c in cases.values() if c.bits == 8} == {16, 32, 64, 128, 256}
    for bits in (4, 8):
        al = cases[f"alphasign_t{bits}"].segs[0].alpha[:, 0, 0]
        assert sorted(al.tolist()) == sorted(torch.tensor(C.ALPHAS).tolist()) and {math.copysign(1.0, a) for a in al.tolist() if a == 0} == {1.0, -1.0}
        two = cases[f"twoseg_t{bits}"]
        assert [(s.c0, s.clen) for s in two.segs] == [(5, 17), (22, 42)] and two.Cin_total == 64 and two.orders == [[0, 1], [1, 0]]


def test_reciprocal_multiply_changes_the_near_integer_family(cases, record_property):
    """From the reference alone: at least 5 % of the family's elements change code when the quotient is w * fl(1 / delta), so a
    packer that multiplied by a reciprocal could not pass the family.  (Half of the family cannot change by construction: w =
    fl(k * delta) under round-to-nearest and w = fl((k + 1/2) * delta) under floor are half a step away from the next code.)"""
    changed = total = 0
    for c in C.by_family("nearint"):
        ch, n = C.reciprocal_changes(c)
        print(f"[pack_exact] {c.name}: {ch} of {n} elements ({100 * ch / n:.2f} %) change code under a reciprocal multiply")
        record_property(c.name, round(ch / n, 4))
        assert ch > 0, c.name
        changed, total = changed + ch, total + n
    print(f"[pack_exact] near-integer family: {changed} of {total} elements ({100 * changed / total:.2f} %)")
    record_property("family", round(changed / total, 4))
    assert changed / total >= 0.05
    # the exactly representable families do not tell the two apart: the near-integer family is what does
    assert C.reciprocal_changes(cases["grid_t4"])[0] == 0 and C.reciprocal_changes(cases["ties_t8"])[0] == 0


def test_fp64_quotient_is_another_function(cases):
    """Why the oracle is fp32 IEEE division and not a higher precision: the fp64 quotient gives other codes on this family."""
    for c in C.by_family("nearint"):
        s = c.segs[0]
        q = c.w.double() / s.delta.view(-1, 1, 1).double()
        q = torch.floor(q) + (s.alpha >= 0).double() if s.alpha is not None else torch.round(q)
        other = torch.clamp(q + s.zp.view(-1, 1, 1), 0, c.n_levels - 1).long()
        n = int((other != C.seg_codes(c, s)).sum())
        print(f"[pack_exact] {c.name}: {n} of {other.numel()} codes differ under an fp64 quotient")
        assert n > 0, c.name


# ---- emulator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.FAMILIES)
def test_emulated_packers_reproduce_the_image(family):
    n = 0
    for c in C.by_family(family):
        for order in c.orders:
            buf, wsum = _emulated(c, order)
            assert np.array_equal(buf, c.want_buf), C.first_difference(c, buf)
            assert c.want_wsum is None or np.array_equal(wsum, c.want_wsum), (c.name, order)
        n += 1
    assert n > 0


# ---- Python decode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.FAMILIES)
def test_python_decode_of_the_layout(family):
    """engine.wonly_code_span reads the stored bytes of a pack: max |q - z| over the rows below Cout of the segments' own K-steps,
    the K-pad bytes of a t8 tile counting as code 128 (a 4-bit pack answers its bound, 255, without looking)."""
    from types import SimpleNamespace as NS
    from qdiff import engine
    for c in C.by_family(family):
        pack = NS(mode=c.bits, Cout=c.Cout, taps=c.taps, wq=torch.from_numpy(c.want_buf.copy()),
                  segs=[dict(kstep0=s.kstep0, clen_pad=C.pad16(s.clen), zw=(s.zp - (128 if c.bits == 8 else 0)).to(torch.int32)) for s in c.segs])
        want = 0
        for s in c.segs:
            z = s.zp.long().view(-1, 1, 1)
            want = max(want, int((C.seg_codes(c, s) - z).abs().max()))
            if c.bits == 8 and C.nsteps(s.clen) * 64 > s.clen:
                want = max(want, int((128 - z).abs().max()))
        got = engine.wonly_code_span(pack)
        if c.bits == 8:
            assert got == want, (c.name, got, want)
        else:
            assert got == 255 >= want, (c.name, got, want)


# ---- mutations of the emulator's packers -----------------------------------------------------------------------------------
def _mut_alpha_gt(w, alpha, delta, zp, Cout, Cin_total, taps, c0, clen, n_levels):
    wv = w.reshape(Cout, Cin_total, taps)[:, c0:c0 + clen].float()
    d, z = delta.view(-1, 1, 1), zp.view(-1, 1, 1)
    q = (torch.floor(wv / d) + (alpha.reshape(Cout, clen, taps) > 0).float()) if alpha is not None else torch.round(wv / d)
    return torch.clamp(q + z, 0, n_levels - 1).to(torch.int64)


def _mut_round_half_up(w, alpha, delta, zp, Cout, Cin_total, taps, c0, clen, n_levels):
    wv = w.reshape(Cout, Cin_total, taps)[:, c0:c0 + clen].float()
    d, z = delta.view(-1, 1, 1), zp.view(-1, 1, 1)
    q = (torch.floor(wv / d) + (alpha.reshape(Cout, clen, taps) >= 0).float()) if alpha is not None else torch.floor(wv / d + 0.5)
    return torch.clamp(q + z, 0, n_levels - 1).to(torch.int64)


def _mut_clamp_to_levels(w, alpha, delta, zp, Cout, Cin_total, taps, c0, clen, n_levels):
    wv = w.reshape(Cout, Cin_total, taps)[:, c0:c0 + clen].float()
    d, z = delta.view(-1, 1, 1), zp.view(-1, 1, 1)
    q = (torch.floor(wv / d) + (alpha.reshape(Cout, clen, taps) >= 0).float()) if alpha is not None else torch.round(wv / d)
    return torch.clamp(q + z, 0, n_levels).to(torch.int64)


def _mut_nibble_halves(ch):
    by = torch.empty(ch.shape[:-1] + (8,), dtype=torch.int64)
    for b in range(4):
        by[..., b] = ch[..., 4 + b] | (ch[..., b] << 4)
        by[..., 4 + b] = ch[..., 12 + b] | (ch[..., 8 + b] << 4)
    return by


def _mut_kh4_nn(units):
    # [jt, nn, t, cs, kh4, e] -> [t, cs, jt, nn, kh4, e] squeezed into the [.., 4, 32, e] slots
    return units.permute(2, 3, 0, 1, 4, 5).contiguous()


def _mut_wsum_assign(wsum, s):
    if wsum is not None:
        wsum.copy_(s.to(torch.int32))


def _mut_pad_is_zero_point(stored, zp, Cout, clen, taps, ntiles, nst):
    full = torch.zeros(ntiles * 32, taps, nst * 64, dtype=torch.int64)
    full[:Cout] = zp.long().view(-1, 1, 1)
    full[:Cout, :, :clen] = stored.permute(0, 2, 1)
    return full


# (what is replaced in abi_emulator, the mutant, the named case that must catch it)
MUTATIONS = {
    "alpha > 0 instead of >= 0": ("_tiled_codes", _mut_alpha_gt, "alphasign_t4"),
    "floor(x + 1/2) instead of round-half-even": ("_tiled_codes", _mut_round_half_up, "ties_t8"),
    "clamp to n_levels instead of n_levels - 1": ("_tiled_codes", _mut_clamp_to_levels, "grid_t8"),
    "swapped nibble halves": ("_nibble_bytes", _mut_nibble_halves, "grid_t4"),
    "kh4 and nn exchanged": ("_tile_order", _mut_kh4_nn, "geom_t8_N33_c65_t4"),
    "wsum assigned instead of added": ("_wsum_add", _mut_wsum_assign, "grid_t4_alpha"),
    "pad nibble written as the zero point": ("_tiled_canvas", _mut_pad_is_zero_point, "geom_t4_N31_c17_t1"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_mutated_emulator_is_caught(cases, monkeypatch, record_property, what):
    attr, mutant, named = MUTATIONS[what]
    assert all(_same(c, *_emulated(c)) for c in (cases[named],))                # passes unmutated
    monkeypatch.setattr(abi_emulator, attr, mutant)
    caught = [c.name for c in cases.values() if not _same(c, *_emulated(c))]
    print(f"[pack_exact] mutation '{what}': caught by {len(caught)} of {len(cases)} cases, named case {named}")
    record_property("caught_by", len(caught))
    assert named in caught, (what, caught[:5])


# ---- refusals of the real library, nothing launched ------------------------------------------------------------------------
@pytest.fixture
def lib():
    from qdiff import hip
    return hip.load()


# accepted arguments: w, alpha, delta, zp, Cout, Cin_total, taps, c0, clen, clen_pad, n_levels, wt, kstep0, ntiles, wsum, stream
def _args(**kw):
    a = dict(w=FAKE, alpha=None, delta=FAKE, zp=FAKE, Cout=33, Cin_total=64, taps=4, c0=5, clen=17, clen_pad=32, n_levels=16, wt=FAKE,
             kstep0=1, ntiles=2, wsum=None, stream=None)
    a.update(kw)
    return list(a.values())


REFUSALS = [
    ("levels-1", 4, dict(n_levels=1), "n_levels 1 does not fit a nibble"),
    ("levels-17-t4", 4, dict(n_levels=17), "n_levels 17 does not fit a nibble"),
    ("levels-1-t8", 8, dict(n_levels=1), "n_levels 1 does not fit a byte"),
    ("levels-257-t8", 8, dict(n_levels=257), "n_levels 257 does not fit a byte"),
    ("ntiles-short", 4, dict(ntiles=1), "bad tile layout"),
    ("ntiles-long", 8, dict(ntiles=3), "bad tile layout"),
    ("clen-pad-not-16", 4, dict(clen_pad=24), "clen_pad must be a multiple of 16"),
    ("clen-pad-below-clen", 8, dict(clen_pad=16), "clen_pad must be a multiple of 16"),
    ("past-cin-total", 4, dict(c0=48), "bad shape"),
    ("past-cin-total-t8", 8, dict(Cin_total=21), "bad shape"),
    ("wt-misaligned", 4, dict(wt=FAKE + 8), "bad tile layout"),
    ("wt-misaligned-t8", 8, dict(wt=FAKE + 4), "bad tile layout"),
    ("null-w", 4, dict(w=None), "null pointer"),
    ("null-delta", 8, dict(delta=None), "null pointer"),
    ("null-zp", 4, dict(zp=None), "null pointer"),
    ("null-wt", 8, dict(wt=None), "null pointer"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_packers_refuse_before_any_launch(lib, case):
    _, bits, change, needle = case
    fn = lib.qd_pack_weights_t4 if bits == 4 else lib.qd_pack_weights_t8
    assert FAKE % 16 == 0
    rc = fn(*_args(**change))
    msg = lib.qd_last_error().decode()
    assert rc != 0 and needle in msg and msg.startswith(f"qd_pack_weights_t{bits}: "), msg
